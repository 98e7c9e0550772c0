// gs_topk_rows.hip -- gs_topk_rows_u32: the first k of the stable sort of every row of a matrix.
//
// Row r of the result is what gs_topk_u32 writes for row r alone, bit for bit.  Every row has the same length, so the
// launches are decided on the host from num_cols and k:
//
//   path 1   num_cols <= 1024: one wave per row, four rows per workgroup.  The row sits in registers (1, 4, 8 or 16 elements
//            per lane) as (image, column) pairs, takes the stable LSD wave sort of gs_seg_wave_body.inc on all 32 bits, and
//            only its first k are stored.  No workgroup barrier.
//   path 2   num_cols <= CH = 8192: one workgroup of 512 threads per row.  The row is read once into registers, 16 per
//            thread in (wave, row, lane) order; a radix select runs on it where it sits (four rounds of a 256-bin LDS
//            histogram of the next byte over the elements that still match the prefix, and a pick); an ordered two-group
//            compaction (before the k-th image / the first `take` equal to it) moves the k selected (image, column) pairs
//            into LDS; one wave sorts them with the wave sort of path 1 and stores them.
//   path 3   longer rows: level 0 runs the path-2 kernel per (row, chunk of CH columns) and writes each chunk's
//            min(k, chunk length) sorted (key, column) pairs, chunk after chunk, into a candidate row of the workspace;
//            level i + 1 runs the same kernel over the candidate rows, ranking by key, breaking ties by position and passing
//            the carried columns through; the level whose source fits one chunk writes the outputs.
//
// Why path 3 is exact: an element of a row's first k has fewer than k elements before it in (image, column) order, so the
// same holds inside its chunk; equal images inside a chunk's output are in column order and chunks are concatenated in
// column order, so position order among equal images is column order at every level.  Equal keys land in ONE group of the
// compaction in input order, so the stable finish reproduces the definition (the argument of section 10g).  No kernel waits
// on another workgroup, there is no global atomic, and no element of paths 1 and 2 touches the workspace.
#include "gs_device.hpp"
#include "gs_host.hpp"

// the geometry, the wave sort, the select and the compaction (wave_sort_bits, tr_select, tr_compact: here on all 32 bits) and
// the host's plan: shared with gs_topk_rows_narrow.hip
#include "gs_topk_rows.inc"

namespace gs {

// ------------------------------------------------------------------ path 1 --
// One wave per row of up to WKPT * 64 columns, four rows per workgroup; waves past the last row leave (no barrier follows).
template <int WKPT, bool HV>
__global__ __launch_bounds__(256) void topk_rows_wave_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vals_in,
                                                             uint32_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                             uint32_t rows, uint32_t cols, uint32_t stride, uint32_t k, int f32, uint32_t x)
{
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][RADIX];
    __shared__ uint32_t stage_k[4][CAP];
    __shared__ uint32_t stage_v[HV ? 4 : 1][HV ? CAP : 1];
    const int w = wave_id(), lane = lane_id();
    const uint32_t r = blockIdx.x * 4u + (uint32_t)w;
    if (r >= rows) return;
    const size_t in0 = (size_t)r * stride, out0 = (size_t)r * k;
    uint32_t key[WKPT], val[HV ? WKPT : 1];
    const uint32_t last = cols - 1u;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = __builtin_nontemporal_load(keys + in0 + (idx < last ? idx : last));
    }
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = idx < cols ? twiddle_in(key[i], f32, x) : 0xffffffffu;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx;
    }
    wave_sort_bits<32, WKPT, HV>(key, val, hist[w], stage_k[w], stage_v[HV ? w : 0]);
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        if (idx < k) {
            keys_out[out0 + idx] = twiddle_out(key[i], f32, x);
            if (HV) vals_out[out0 + idx] = vals_in ? vals_in[in0 + (val[i] < cols ? val[i] : last)] : val[i];
        }
    }
}

// ------------------------------------------------------------ paths 2 and 3 --
// One workgroup per (row, chunk of TR_CH elements) of a source matrix with rows of n elements at src_stride.  Selects the
// first keff = min(k, chunk length) of the chunk's stable sort and writes them, sorted, at dst + row * dst_stride +
// chunk * k.  SRC_IDX: the source carries columns (src_i, a candidate row of an earlier level); otherwise an element's
// column is its position in the row.  FINAL: dst are the caller's outputs (keys, and in the pairs form vals_in[column] of
// the caller's matrix of vals_cols columns at vals_stride); otherwise a candidate row: keys in the caller's bit patterns, and columns.
// WKPT * 64 >= k is what the finishing wave holds.
template <int WKPT, bool HV, bool SRC_IDX, bool FINAL>
__global__ __launch_bounds__(TR_THREADS) void topk_rows_block_kernel(const uint32_t *__restrict__ src_k, const uint32_t *__restrict__ src_i,
                                                                     uint32_t src_stride, uint32_t n, uint32_t chunks,
                                                                     uint32_t *__restrict__ dst_k, uint32_t *__restrict__ dst_v,
                                                                     uint32_t dst_stride, const uint32_t *__restrict__ vals_in,
                                                                     uint32_t vals_stride, uint32_t vals_cols, uint32_t k, int f32,
                                                                     uint32_t x)
{
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];   // the select's histogram, then the finishing wave's counters
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    __shared__ uint32_t stage_k[CAP], sort_k[CAP];
    __shared__ uint32_t stage_v[HV ? CAP : 1], sort_v[HV ? CAP : 1];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / chunks, c = blockIdx.x - r * chunks;
    const uint32_t lo = c * TR_CH, len = n - lo < TR_CH ? n - lo : TR_CH, keff = k < len ? k : len;
    const size_t base = (size_t)r * src_stride + lo;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;

    uint32_t img[TR_KPT];
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        img[u] = j < len ? __builtin_nontemporal_load(src_k + base + j) : 0u;
    }
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) img[u] = twiddle_in(img[u], f32, x);

    // radix select of the keff-th image on the registers, then the ordered compaction of the keff selected pairs into LDS
    uint32_t less;
    const uint32_t kth = tr_select<32>(img, first, len, keff, tid, h, scratch, sel, less);
    tr_compact<HV, SRC_IDX, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v, SRC_IDX ? src_i + base : nullptr, lo);

    // finish: one wave sorts the keff staged pairs and stores them
    if (w != 0) return;
    uint32_t key[WKPT], val[HV ? WKPT : 1];
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        key[i] = idx < keff ? stage_k[idx] : 0xffffffffu;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx < keff ? stage_v[idx] : 0u;
    }
    wave_sort_bits<32, WKPT, HV>(key, val, h, sort_k, sort_v);
    const size_t out0 = (size_t)r * dst_stride + (size_t)c * k;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        if (idx < keff) {
            dst_k[out0 + idx] = twiddle_out(key[i], f32, x);
            if (HV) {
                if (FINAL && vals_in) dst_v[out0 + idx] = vals_in[(size_t)r * vals_stride + (val[i] < vals_cols ? val[i] : vals_cols - 1u)];
                else dst_v[out0 + idx] = val[i];
            }
        }
    }
}

// ------------------------------------------------------------------------- host --
template <int WKPT, bool HV>
static void tr_launch_wave(hipStream_t s, const uint32_t *ki, const uint32_t *vi, uint32_t *ko, uint32_t *vo, uint32_t rows, uint32_t cols,
                           uint32_t stride, uint32_t k, int f32, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows_wave_kernel<WKPT, HV>), dim3((rows + 3u) / 4u), dim3(256), 0, s, ki, vi, ko, vo, rows, cols, stride, k,
                       f32, x);
}

struct BlockArgs {
    const uint32_t *src_k, *src_i;
    uint32_t src_stride, n, chunks;
    uint32_t *dst_k, *dst_v;
    uint32_t dst_stride;
    const uint32_t *vals_in;
    uint32_t vals_stride, vals_cols, k;
    int f32;
    uint32_t x, rows;
};

template <int WKPT, bool HV, bool SRC_IDX, bool FINAL>
static void tr_launch_block4(hipStream_t s, const BlockArgs &a)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows_block_kernel<WKPT, HV, SRC_IDX, FINAL>), dim3(a.rows * a.chunks), dim3(TR_THREADS), 0, s, a.src_k, a.src_i,
                       a.src_stride, a.n, a.chunks, a.dst_k, a.dst_v, a.dst_stride, a.vals_in, a.vals_stride, a.vals_cols, a.k, a.f32, a.x);
}

template <int WKPT>
static void tr_launch_block(hipStream_t s, const BlockArgs &a, bool hv, bool src_idx, bool final)
{
    if (!hv) {   // keys alone: no columns to read or carry
        if (final) tr_launch_block4<WKPT, false, false, true>(s, a);
        else tr_launch_block4<WKPT, false, false, false>(s, a);
    } else if (src_idx) {
        if (final) tr_launch_block4<WKPT, true, true, true>(s, a);
        else tr_launch_block4<WKPT, true, true, false>(s, a);
    } else {
        if (final) tr_launch_block4<WKPT, true, false, true>(s, a);
        else tr_launch_block4<WKPT, true, false, false>(s, a);
    }
}

}  // namespace gs

using namespace gs;

extern "C" {

uint32_t gs_topk_rows_max_k(void) { return TR_MAX_K; }

int gs_topk_rows_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!tr_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;   // such a call enqueues nothing
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);
    out[0] = p.path; out[1] = p.levels; out[2] = TR_CH; out[3] = p.chunks0; out[4] = p.cand0; out[5] = TR_MAX_K;
    return hipSuccess;
}

size_t gs_topk_rows_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    if (!tr_shape_ok(num_rows, num_cols, k)) return 0;
    if (num_rows == 0 || num_cols == 0 || k == 0) return 0;
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);
    const size_t v = has_values ? 2 : 1;
    size_t total = 0;
    if (p.levels > 1) total += v * tr_align((size_t)4 * num_rows * p.n[1]);
    if (p.levels > 2) total += v * tr_align((size_t)4 * num_rows * p.n[2]);
    return total + GS_WS_SLACK;
}

int gs_topk_rows_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                     uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                     int key_type, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!tr_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (row_stride < num_cols || tr_mul_ge_2p32(num_rows, row_stride)) return hipErrorInvalidValue;
    if (key_type < GS_KEY_U32 || key_type > GS_KEY_F32) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < gs_topk_rows_temp_bytes(num_rows, num_cols, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_vals_in | (uintptr_t)d_keys_out | (uintptr_t)d_vals_out) & 3u) != 0) return hipErrorInvalidValue;
    {
        const size_t in_bytes = (size_t)4 * ((num_rows - 1) * row_stride + num_cols), out_bytes = (size_t)4 * num_rows * k;
        const void *arr[4] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out};
        const size_t bytes[4] = {in_bytes, in_bytes, out_bytes, out_bytes};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (tr_overlaps(arr[i], bytes[i], arr[j], bytes[j])) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t rows = (uint32_t)num_rows, cols = (uint32_t)num_cols, stride = (uint32_t)row_stride, kk = (uint32_t)k;
    const int f32 = key_type == GS_KEY_F32;
    const uint32_t x = (key_type == GS_KEY_I32 ? 0x80000000u : 0u) ^ (descending ? 0xffffffffu : 0u);
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);

    if (p.path == 1) {
#define GS_TR_WAVE(W)                                                                                                   \
    do {                                                                                                                \
        if (hv) tr_launch_wave<W, true>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, f32, x); \
        else tr_launch_wave<W, false>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, f32, x);   \
    } while (0)
        if (cols <= 64) GS_TR_WAVE(1);
        else if (cols <= 256) GS_TR_WAVE(4);
        else if (cols <= 512) GS_TR_WAVE(8);
        else GS_TR_WAVE(16);
#undef GS_TR_WAVE
        return (int)hipGetLastError();
    }

    // paths 2 and 3: level i reads rows of n[i] elements; the candidate rows alternate between two areas of the workspace
    const size_t v = hv ? 2 : 1;
    char *wsb = gs_ws_base(d_temp);
    uint32_t *area_k[2] = {nullptr, nullptr}, *area_i[2] = {nullptr, nullptr};
    {
        size_t off = 0;
        for (uint32_t a = 0; a < 2 && a + 1 < p.levels; ++a) {
            const size_t bytes = tr_align((size_t)4 * num_rows * p.n[a + 1]);
            area_k[a] = (uint32_t *)(wsb + off); off += bytes;
            if (v == 2) { area_i[a] = (uint32_t *)(wsb + off); off += bytes; }
        }
    }
    for (uint32_t lvl = 0; lvl < p.levels; ++lvl) {
        const bool final = lvl + 1 == p.levels;
        BlockArgs a;
        a.src_k = lvl == 0 ? d_keys_in : area_k[(lvl - 1) & 1];
        a.src_i = lvl == 0 ? nullptr : area_i[(lvl - 1) & 1];
        a.src_stride = lvl == 0 ? stride : (uint32_t)p.n[lvl];
        a.n = (uint32_t)p.n[lvl];
        a.chunks = (uint32_t)((p.n[lvl] + TR_CH - 1) / TR_CH);
        a.dst_k = final ? d_keys_out : area_k[lvl & 1];
        a.dst_v = final ? d_vals_out : area_i[lvl & 1];
        a.dst_stride = final ? kk : (uint32_t)p.n[lvl + 1];
        a.vals_in = d_vals_in;
        a.vals_stride = stride;
        a.vals_cols = cols;
        a.k = kk; a.f32 = f32; a.x = x; a.rows = rows;
        if (kk <= 64) tr_launch_block<1>(s, a, hv, lvl != 0, final);
        else if (kk <= 256) tr_launch_block<4>(s, a, hv, lvl != 0, final);
        else if (kk <= 512) tr_launch_block<8>(s, a, hv, lvl != 0, final);
        else tr_launch_block<16>(s, a, hv, lvl != 0, final);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
