// gs_topk_rows_narrow.hip -- gs_topk_rows_u16: the first k of the stable sort of every row of a matrix of 16-bit keys
// (DESIGN.md section 10i).
//
// Row r of the result is bit for bit what gs_topk_rows_u32 gives on the matrix (uint32_t)key << 16 with the key type widened
// (U16 -> U32, I16 -> I32, F16 / BF16 -> F32) and the returned keys shifted back.  The geometry, the three paths and the
// plan are those of gs_topk_rows.hip (gs_topk_rows.inc); what differs is what the key width changes:
//
//   the image    a 16-bit word in a 32-bit register whose upper half is zero: float_flip<16>(key) for the float types, xor
//                x16 (0x8000 for I16 / F16 / BF16, 0xffff when descending).  The pad image is 0xffff -- an ORDINARY image
//                here (the u16 key 0xffff, the largest positive NaN, ...): a pad loses to a real key of that image by
//                position alone, in the stable wave sort (pads sit behind every real element) and in the select (pads are
//                out of range and never counted or placed).
//   the passes   two digit passes in the wave sort and two select rounds (shift 8, then 0) in place of four.
//   the memory   one 2-byte load or store per key, so a row base r * row_stride and an output base r * k may be odd: nothing
//                wider than an element is ever touched.  Candidate rows hold 16-bit keys and u32 columns.
#include "gs_device.hpp"
#include "gs_host.hpp"
#include "gs_topk_rows.inc"

namespace gs {

constexpr int TR16_BITS = 16;
constexpr uint32_t TR16_MASK = 0xffffu;          // the image's bits; also the pad image

__device__ __forceinline__ uint32_t image16_in(uint32_t k, int flt, uint32_t x16) { return (flt ? float_flip<16>(k) : k) ^ x16; }
__device__ __forceinline__ uint32_t image16_out(uint32_t k, int flt, uint32_t x16)
{
    k ^= x16;
    return flt ? float_flip<16>(k) : k;   // float_flip leaves the sign bit alone: its own inverse
}

// ------------------------------------------------------------------ path 1 --
// One wave per row of up to WKPT * 64 columns, four rows per workgroup; waves past the last row leave (no barrier follows).
template <int WKPT, bool HV>
__global__ __launch_bounds__(256) void topk_rows16_wave_kernel(const uint16_t *__restrict__ keys, const uint32_t *__restrict__ vals_in,
                                                               uint16_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                               uint32_t rows, uint32_t cols, uint32_t stride, uint32_t k, int flt,
                                                               uint32_t x16)
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
        key[i] = __builtin_nontemporal_load(keys + in0 + (idx < last ? idx : last));   // past the end: the row's last element again
    }
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = idx < cols ? image16_in(key[i], flt, x16) : TR16_MASK;   // pads: last in position, largest in both digits
        if (HV) val[i] = idx;
    }
    wave_sort_bits<TR16_BITS, WKPT, HV>(key, val, hist[w], stage_k[w], stage_v[HV ? w : 0]);
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        if (idx < k) {
            keys_out[out0 + idx] = (uint16_t)image16_out(key[i], flt, x16);
            if (HV) vals_out[out0 + idx] = vals_in ? vals_in[in0 + (val[i] < cols ? val[i] : last)] : val[i];
        }
    }
}

// ------------------------------------------------------------ paths 2 and 3 --
// One workgroup per (row, chunk of TR_CH elements) of a source matrix with rows of n elements at src_stride: the kernel of
// gs_topk_rows.hip with 16-bit keys at both ends.  SRC_IDX: the source carries columns (src_i, a candidate row of an earlier
// level); FINAL: dst are the caller's outputs, otherwise a candidate row (16-bit keys in the caller's bit patterns, u32 columns).
template <int WKPT, bool HV, bool SRC_IDX, bool FINAL>
__global__ __launch_bounds__(TR_THREADS) void topk_rows16_block_kernel(const uint16_t *__restrict__ src_k, const uint32_t *__restrict__ src_i,
                                                                       uint32_t src_stride, uint32_t n, uint32_t chunks,
                                                                       uint16_t *__restrict__ dst_k, uint32_t *__restrict__ dst_v,
                                                                       uint32_t dst_stride, const uint32_t *__restrict__ vals_in,
                                                                       uint32_t vals_stride, uint32_t vals_cols, uint32_t k, int flt,
                                                                       uint32_t x16)
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
        img[u] = j < len ? (uint32_t)__builtin_nontemporal_load(src_k + base + j) : 0u;
    }
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) img[u] = image16_in(img[u], flt, x16);

    // radix select of the keff-th image on the registers, then the ordered compaction of the keff selected pairs into LDS
    uint32_t less;
    const uint32_t kth = tr_select<TR16_BITS>(img, first, len, keff, tid, h, scratch, sel, less);
    tr_compact<HV, SRC_IDX, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v, SRC_IDX ? src_i + base : nullptr, lo);

    // finish: one wave sorts the keff staged pairs and stores them
    if (w != 0) return;
    uint32_t key[WKPT], val[HV ? WKPT : 1];
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        key[i] = idx < keff ? stage_k[idx] : TR16_MASK;   // pads: last in position, largest in both digits
        if (HV) val[i] = idx < keff ? stage_v[idx] : 0u;
    }
    wave_sort_bits<TR16_BITS, WKPT, HV>(key, val, h, sort_k, sort_v);
    const size_t out0 = (size_t)r * dst_stride + (size_t)c * k;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        if (idx < keff) {
            dst_k[out0 + idx] = (uint16_t)image16_out(key[i], flt, x16);
            if (HV) {
                if (FINAL && vals_in) dst_v[out0 + idx] = vals_in[(size_t)r * vals_stride + (val[i] < vals_cols ? val[i] : vals_cols - 1u)];
                else dst_v[out0 + idx] = val[i];
            }
        }
    }
}

// ------------------------------------------------------------------------- host --
template <int WKPT, bool HV>
static void tr16_launch_wave(hipStream_t s, const uint16_t *ki, const uint32_t *vi, uint16_t *ko, uint32_t *vo, uint32_t rows, uint32_t cols,
                             uint32_t stride, uint32_t k, int flt, uint32_t x16)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows16_wave_kernel<WKPT, HV>), dim3((rows + 3u) / 4u), dim3(256), 0, s, ki, vi, ko, vo, rows, cols, stride, k,
                       flt, x16);
}

struct Block16Args {
    const uint16_t *src_k;
    const uint32_t *src_i;
    uint32_t src_stride, n, chunks;
    uint16_t *dst_k;
    uint32_t *dst_v;
    uint32_t dst_stride;
    const uint32_t *vals_in;
    uint32_t vals_stride, vals_cols, k;
    int flt;
    uint32_t x16, rows;
};

template <int WKPT, bool HV, bool SRC_IDX, bool FINAL>
static void tr16_launch_block4(hipStream_t s, const Block16Args &a)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows16_block_kernel<WKPT, HV, SRC_IDX, FINAL>), dim3(a.rows * a.chunks), dim3(TR_THREADS), 0, s, a.src_k,
                       a.src_i, a.src_stride, a.n, a.chunks, a.dst_k, a.dst_v, a.dst_stride, a.vals_in, a.vals_stride, a.vals_cols, a.k,
                       a.flt, a.x16);
}

template <int WKPT>
static void tr16_launch_block(hipStream_t s, const Block16Args &a, bool hv, bool src_idx, bool final)
{
    if (!hv) {   // keys alone: no columns to read or carry
        if (final) tr16_launch_block4<WKPT, false, false, true>(s, a);
        else tr16_launch_block4<WKPT, false, false, false>(s, a);
    } else if (src_idx) {
        if (final) tr16_launch_block4<WKPT, true, true, true>(s, a);
        else tr16_launch_block4<WKPT, true, true, false>(s, a);
    } else {
        if (final) tr16_launch_block4<WKPT, true, false, true>(s, a);
        else tr16_launch_block4<WKPT, true, false, false>(s, a);
    }
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_topk_rows_u16_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    if (!tr_shape_ok(num_rows, num_cols, k)) return 0;
    if (num_rows == 0 || num_cols == 0 || k == 0) return 0;
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);
    size_t total = 0;
    for (uint32_t a = 1; a <= 2 && a < p.levels; ++a) {
        total += tr_align((size_t)2 * num_rows * p.n[a]);                   // 16-bit keys
        if (has_values) total += tr_align((size_t)4 * num_rows * p.n[a]);   // u32 columns
    }
    return total + GS_WS_SLACK;
}

int gs_topk_rows_u16(void *d_temp, size_t temp_bytes, const uint16_t *d_keys_in, const uint32_t *d_vals_in, uint16_t *d_keys_out,
                     uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                     int key_type, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!tr_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (row_stride < num_cols || tr_mul_ge_2p32(num_rows, row_stride)) return hipErrorInvalidValue;
    if (key_type != GS_KEY_U16 && key_type != GS_KEY_I16 && key_type != GS_KEY_F16 && key_type != GS_KEY_BF16) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < gs_topk_rows_u16_temp_bytes(num_rows, num_cols, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & 1u) != 0) return hipErrorInvalidValue;
    if ((((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & 3u) != 0) return hipErrorInvalidValue;
    {
        const size_t in_elems = (size_t)((num_rows - 1) * row_stride + num_cols), out_elems = (size_t)(num_rows * k);
        const void *arr[4] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out};
        const size_t bytes[4] = {2 * in_elems, 4 * in_elems, 2 * out_elems, 4 * out_elems};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (tr_overlaps(arr[i], bytes[i], arr[j], bytes[j])) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t rows = (uint32_t)num_rows, cols = (uint32_t)num_cols, stride = (uint32_t)row_stride, kk = (uint32_t)k;
    const int flt = key_type == GS_KEY_F16 || key_type == GS_KEY_BF16;
    const uint32_t x16 = (key_type == GS_KEY_U16 ? 0u : 0x8000u) ^ (descending ? TR16_MASK : 0u);
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);

    if (p.path == 1) {
#define GS_TR16_WAVE(W)                                                                                                     \
    do {                                                                                                                    \
        if (hv) tr16_launch_wave<W, true>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, flt, x16); \
        else tr16_launch_wave<W, false>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, flt, x16);   \
    } while (0)
        if (cols <= 64) GS_TR16_WAVE(1);
        else if (cols <= 256) GS_TR16_WAVE(4);
        else if (cols <= 512) GS_TR16_WAVE(8);
        else GS_TR16_WAVE(16);
#undef GS_TR16_WAVE
        return (int)hipGetLastError();
    }

    // paths 2 and 3: level i reads rows of n[i] elements; the candidate rows alternate between two areas of the workspace
    char *wsb = gs_ws_base(d_temp);
    uint16_t *area_k[2] = {nullptr, nullptr};
    uint32_t *area_i[2] = {nullptr, nullptr};
    {
        size_t off = 0;
        for (uint32_t a = 0; a < 2 && a + 1 < p.levels; ++a) {
            area_k[a] = (uint16_t *)(wsb + off); off += tr_align((size_t)2 * num_rows * p.n[a + 1]);
            if (hv) { area_i[a] = (uint32_t *)(wsb + off); off += tr_align((size_t)4 * num_rows * p.n[a + 1]); }
        }
    }
    for (uint32_t lvl = 0; lvl < p.levels; ++lvl) {
        const bool final = lvl + 1 == p.levels;
        Block16Args a;
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
        a.k = kk; a.flt = flt; a.x16 = x16; a.rows = rows;
        if (kk <= 64) tr16_launch_block<1>(s, a, hv, lvl != 0, final);
        else if (kk <= 256) tr16_launch_block<4>(s, a, hv, lvl != 0, final);
        else if (kk <= 512) tr16_launch_block<8>(s, a, hv, lvl != 0, final);
        else tr16_launch_block<16>(s, a, hv, lvl != 0, final);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
