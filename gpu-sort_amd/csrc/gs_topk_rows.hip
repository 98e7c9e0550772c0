// gs_topk_rows.hip -- gs_topk_rows_u32 and gs_topk_rows_u16: the first k of the stable sort of every row of a matrix, for
// 32-bit keys and 16-bit keys (section 10i).  One set of kernels and one host path, instantiated
// over a key-traits type (TrKey32, TrKey16); one geometry and one plan, so gs_topk_rows_plan answers for both entry points.
//
// Row r of the result is what gs_topk_u32 writes for row r alone, bit for bit.  Every row has the same length, so the
// launches are decided on the host from num_cols and k:
//
//   path 1   num_cols <= 1024: one wave per row, four rows per workgroup.  The row sits in registers (1, 4, 8 or 16 elements
//            per lane) as (image, column) pairs, takes the stable LSD wave sort of gs_seg_wave_body.inc on all bits of the
//            image, and only its first k are stored.  No workgroup barrier.
//   path 2   num_cols <= CH = 8192: one workgroup of 512 threads per row.  The row is read once into registers, 16 per
//            thread in (wave, row, lane) order; a radix select runs on it where it sits (one round per byte of the image:
//            a 256-bin LDS histogram of the next byte over the elements that still match the prefix, and a pick); an ordered
//            two-group compaction (before the k-th image / the first `take` equal to it) moves the k selected (image, column)
//            pairs into LDS; one wave sorts them with the wave sort of path 1 and stores them.
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
//
// 16-bit keys: row r of the result is bit for bit what gs_topk_rows_u32 gives on the matrix (uint32_t)key << 16 with the key
// type widened (U16 -> U32, I16 -> I32, F16 / BF16 -> F32) and the returned keys shifted back.  What the key width changes:
//
//   the image    a 16-bit word in a 32-bit register whose upper half is zero: float_flip<16>(key) for the float types, xor
//                x (0x8000 for I16 / F16 / BF16, 0xffff when descending).  The pad image is 0xffff -- an ORDINARY image
//                here (the u16 key 0xffff, the largest positive NaN, ...): a pad loses to a real key of that image by
//                position alone, in the stable wave sort (pads sit behind every real element) and in the select (pads are
//                out of range and never counted or placed).
//   the passes   two digit passes in the wave sort and two select rounds (shift 8, then 0) in place of four.
//   the memory   one 2-byte load or store per key, so a row base r * row_stride and an output base r * k may be odd: nothing
//                wider than an element is ever touched.  Candidate rows hold 16-bit keys and u32 columns.
#include "gs_device.hpp"
#include "gs_host.hpp"

namespace gs {

constexpr int TR_THREADS = 512;                  // 8 waves
constexpr int TR_WAVES = TR_THREADS / WAVE;
constexpr int TR_KPT = 16;
constexpr uint32_t TR_CH = TR_THREADS * TR_KPT;  // 8192: the elements one workgroup selects from
constexpr uint32_t TR_MAX_K = 1024;              // what one wave sorts: 16 per lane
constexpr uint32_t TR_WAVE_COLS = 1024;          // longest row of path 1
static_assert(TR_MAX_K <= TR_CH && TR_MAX_K == 16 * WAVE, "a chunk gives up to k sorted by one wave");

// What the key width changes.  T: the element in memory; BITS: the width of the image, which sits in a 32-bit register;
// PAD: the image of an element past the end (largest in every digit); in / out: the caller's bit pattern to the image and
// back, flt for the float types, x the xor mask of xor_of; type_ok / is_float / xor_of: the key types the entry point takes.
struct TrKey32 {
    using T = uint32_t;
    static constexpr int BITS = 32;
    static constexpr uint32_t PAD = 0xffffffffu;
    static __device__ __forceinline__ uint32_t in(uint32_t k, int flt, uint32_t x) { return twiddle_in(k, flt, x); }
    static __device__ __forceinline__ uint32_t out(uint32_t k, int flt, uint32_t x) { return twiddle_out(k, flt, x); }
    static bool type_ok(int key_type) { return key_type >= GS_KEY_U32 && key_type <= GS_KEY_F32; }
    static int is_float(int key_type) { return key_type == GS_KEY_F32; }
    static uint32_t xor_of(int key_type, int descending)
    {
        return (key_type == GS_KEY_I32 ? 0x80000000u : 0u) ^ (descending ? 0xffffffffu : 0u);
    }
};

struct TrKey16 {
    using T = uint16_t;
    static constexpr int BITS = 16;
    static constexpr uint32_t PAD = 0xffffu;   // the image's bits; an ordinary image too (see the header)
    static __device__ __forceinline__ uint32_t in(uint32_t k, int flt, uint32_t x) { return (flt ? float_flip<16>(k) : k) ^ x; }
    static __device__ __forceinline__ uint32_t out(uint32_t k, int flt, uint32_t x)
    {
        k ^= x;
        return flt ? float_flip<16>(k) : k;   // float_flip leaves the sign bit alone: its own inverse
    }
    static bool type_ok(int key_type)
    {
        return key_type == GS_KEY_U16 || key_type == GS_KEY_I16 || key_type == GS_KEY_F16 || key_type == GS_KEY_BF16;
    }
    static int is_float(int key_type) { return key_type == GS_KEY_F16 || key_type == GS_KEY_BF16; }
    static uint32_t xor_of(int key_type, int descending) { return (key_type == GS_KEY_U16 ? 0u : 0x8000u) ^ (descending ? PAD : 0u); }
};

// One wave: the stable LSD sort, on the low BITS bits, of WKPT * 64 (image, value) pairs in registers; element i * 64 + lane
// is key[i].  The passes of gs_seg_wave_body.inc: per-digit ranks by match_digit, the wave's own 256 counters, a scan of 4 per
// lane, and a trip through the wave's staging rows.  All 64 lanes must be active.  BITS / 8 passes: four for a 32-bit image,
// two for a 16-bit one (whose upper half is zero in every element, so the two passes left out would move nothing).
template <int BITS, int WKPT, bool HV>
__device__ __forceinline__ void wave_sort_bits(uint32_t (&key)[WKPT], uint32_t (&val)[HV ? WKPT : 1], uint32_t *__restrict__ my,
                                               uint32_t *__restrict__ sk, uint32_t *__restrict__ sv)
{
    static_assert(BITS == 16 || BITS == 32, "whole digits of a 16- or 32-bit image");
    const int lane = lane_id();
    auto fence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (uint32_t sh = 0; sh < (uint32_t)BITS; sh += (uint32_t)RADIX_BITS) {
        uint32_t pos[WKPT];
        reinterpret_cast<uint4 *>(my)[lane] = make_uint4(0u, 0u, 0u, 0u);
        fence();
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t d = __builtin_amdgcn_ubfe(key[i], sh, RADIX_BITS);
            uint32_t lo, hi;
            match_digit(d, lo, hi);
            const uint32_t lower = count_lower(lo, hi);
            pos[i] = my[d] + lower;
            if (lower == 0) my[d] += (uint32_t)(__popc(lo) + __popc(hi));   // one lane per digit: no two writers of a word
            fence();
        }
        {   // exclusive scan of the 256 counters, 4 per lane
            const uint4 c = reinterpret_cast<const uint4 *>(my)[lane];
            const uint32_t sum = c.x + c.y + c.z + c.w;
            const uint32_t ex = wave_inclusive_scan(sum) - sum;
            reinterpret_cast<uint4 *>(my)[lane] = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
        }
        fence();
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t at = pos[i] + my[__builtin_amdgcn_ubfe(key[i], sh, RADIX_BITS)];
            sk[at] = key[i];
            if (HV) sv[at] = val[i];
        }
        fence();
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            key[i] = sk[i * WAVE + lane];
            if (HV) val[i] = sv[i * WAVE + lane];
        }
        fence();
    }
}

// One workgroup of TR_THREADS: the radix select of the keff-th image among the len elements it holds in registers, 16 per
// thread in (wave, row, lane) order (element j = first + u * 64 of the chunk is img[u]; those with j >= len do not count), most
// significant byte first: BITS / 8 rounds of a 256-bin LDS histogram of the next byte over the elements that still match the
// prefix, and a pick.  Returns the image; less = elements before it, so that keff - less are taken from its run of equal images.
template <int BITS>
__device__ __forceinline__ uint32_t tr_select(uint32_t (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t keff, uint32_t tid,
                                              uint32_t *__restrict__ h, uint32_t *__restrict__ scratch, uint32_t *__restrict__ sel,
                                              uint32_t &less)
{
    static_assert(BITS == 16 || BITS == 32, "whole digits of a 16- or 32-bit image");
    uint32_t prefix = 0, krem = keff;
    less = 0;
    for (uint32_t shift = (uint32_t)BITS - 8u;; shift -= 8u) {
        const uint32_t mask = 0xffffff00u << shift;   // the bytes above this one (none in the first round: a 16-bit image has zeros there)
        if (tid < (uint32_t)RADIX) h[tid] = 0;
        __syncthreads();
        uint32_t lenv = len;
        asm volatile("" : "+v"(lenv));   // compare again each round: sixteen range masks kept across the rounds would not fit the SGPRs
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            if (j < lenv && ((img[u] ^ prefix) & mask) == 0u) hist_add(h, (img[u] >> shift) & 255u);
        }
        __syncthreads();
        const uint32_t cnt = tid < (uint32_t)RADIX ? h[tid] : 0u;
        const uint32_t ex = block_exclusive_scan_256(cnt, scratch, nullptr);
        if (tid < (uint32_t)RADIX && ex < krem && krem - ex <= cnt) {
            sel[0] = prefix | (tid << shift);
            sel[1] = less + ex;
            sel[2] = krem - ex;
        }
        __syncthreads();
        prefix = sel[0]; less = sel[1]; krem = sel[2];
        if (shift == 0u) break;
    }
    return prefix;   // less + krem == keff: the tie run is cut at keff
}

// The ordered two-group compaction of the selected elements into LDS: group A (before the k-th image) at [0, less), group B
// (equal to it) behind, cut at keff; (wave, row, lane) is input order.  stage_v[pos] gets src_i[j] where the source carries
// columns (SRC_IDX), otherwise col0 + j.  Ends with a workgroup barrier.
template <bool HV, bool SRC_IDX, int CAP>
__device__ __forceinline__ void tr_compact(uint32_t (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t keff, uint32_t kth, uint32_t less,
                                           uint32_t w, uint32_t lane, uint32_t (&wcnt)[2][TR_WAVES], uint32_t *__restrict__ stage_k,
                                           uint32_t *__restrict__ stage_v, const uint32_t *__restrict__ src_i, uint32_t col0)
{
    uint32_t nA = 0, nB = 0, lenc = len;
    asm volatile("" : "+v"(lenc));   // (range compares again, as in the select rounds; once more before the scatter loop)
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < lenc && img[u] < kth));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < lenc && img[u] == kth));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    uint32_t baseA = 0, baseB = less;
    for (uint32_t q = 0; q < w; ++q) { baseA += wcnt[0][q]; baseB += wcnt[1][q]; }
    if (baseA < less || baseB < keff) {   // wave-uniform: this wave still has something to place
        asm volatile("" : "+v"(lenc));
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            asm volatile("" : "+v"(img[u]));   // ballot again: 32 masks kept from the counting loop would not fit the SGPRs
            const bool a = j < lenc && img[u] < kth, b = j < lenc && img[u] == kth;
            const unsigned long long mA = __builtin_amdgcn_ballot_w64(a), mB = __builtin_amdgcn_ballot_w64(b);
            const uint32_t pos = a ? baseA + count_lower(mA) : baseB + count_lower(mB);
            if ((a || b) && pos < keff && pos < (uint32_t)CAP) {   // (group A never passes `less`; group B is cut at keff = less + take)
                stage_k[pos] = img[u];
                if (HV) stage_v[pos] = SRC_IDX ? src_i[j] : col0 + j;
            }
            baseA += (uint32_t)__popcll(mA);
            baseB += (uint32_t)__popcll(mB);
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------ path 1 --
// One wave per row of up to WKPT * 64 columns, four rows per workgroup; waves past the last row leave (no barrier follows).
template <typename KT, int WKPT, bool HV>
__global__ __launch_bounds__(256) void topk_rows_wave_kernel(const typename KT::T *__restrict__ keys, const uint32_t *__restrict__ vals_in,
                                                             typename KT::T *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                             uint32_t rows, uint32_t cols, uint32_t stride, uint32_t k, int flt, uint32_t x)
{
    using T = typename KT::T;
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
        key[i] = (uint32_t)__builtin_nontemporal_load(keys + in0 + (idx < last ? idx : last));   // past the end: the row's last element again
    }
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = idx < cols ? KT::in(key[i], flt, x) : KT::PAD;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx;
    }
    wave_sort_bits<KT::BITS, WKPT, HV>(key, val, hist[w], stage_k[w], stage_v[HV ? w : 0]);
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        if (idx < k) {
            keys_out[out0 + idx] = (T)KT::out(key[i], flt, x);
            if (HV) vals_out[out0 + idx] = vals_in ? vals_in[in0 + (val[i] < cols ? val[i] : last)] : val[i];
        }
    }
}

// ------------------------------------------------------------ paths 2 and 3 --
// One workgroup per (row, chunk of TR_CH elements) of a source matrix with rows of n elements at src_stride.  Selects the
// first keff = min(k, chunk length) of the chunk's stable sort and writes them, sorted, at dst + row * dst_stride +
// chunk * k.  SRC_IDX: the source carries columns (src_i, a candidate row of an earlier level); otherwise an element's
// column is its position in the row.  FINAL: dst are the caller's outputs (keys, and in the pairs form vals_in[column] of
// the caller's matrix of vals_cols columns at vals_stride); otherwise a candidate row: keys in the caller's bit patterns
// and width, and u32 columns.  WKPT * 64 >= k is what the finishing wave holds.
template <typename KT, int WKPT, bool HV, bool SRC_IDX, bool FINAL>
__global__ __launch_bounds__(TR_THREADS) void topk_rows_block_kernel(const typename KT::T *__restrict__ src_k,
                                                                     const uint32_t *__restrict__ src_i, uint32_t src_stride, uint32_t n,
                                                                     uint32_t chunks, typename KT::T *__restrict__ dst_k,
                                                                     uint32_t *__restrict__ dst_v, uint32_t dst_stride,
                                                                     const uint32_t *__restrict__ vals_in, uint32_t vals_stride,
                                                                     uint32_t vals_cols, uint32_t k, int flt, uint32_t x)
{
    using T = typename KT::T;
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
    for (int u = 0; u < TR_KPT; ++u) img[u] = KT::in(img[u], flt, x);

    // radix select of the keff-th image on the registers, then the ordered compaction of the keff selected pairs into LDS
    uint32_t less;
    const uint32_t kth = tr_select<KT::BITS>(img, first, len, keff, tid, h, scratch, sel, less);
    tr_compact<HV, SRC_IDX, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v, SRC_IDX ? src_i + base : nullptr, lo);

    // finish: one wave sorts the keff staged pairs and stores them
    if (w != 0) return;
    uint32_t key[WKPT], val[HV ? WKPT : 1];
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        key[i] = idx < keff ? stage_k[idx] : KT::PAD;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx < keff ? stage_v[idx] : 0u;
    }
    wave_sort_bits<KT::BITS, WKPT, HV>(key, val, h, sort_k, sort_v);
    const size_t out0 = (size_t)r * dst_stride + (size_t)c * k;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        if (idx < keff) {
            dst_k[out0 + idx] = (T)KT::out(key[i], flt, x);
            if (HV) {
                if (FINAL && vals_in) dst_v[out0 + idx] = vals_in[(size_t)r * vals_stride + (val[i] < vals_cols ? val[i] : vals_cols - 1u)];
                else dst_v[out0 + idx] = val[i];
            }
        }
    }
}

// ------------------------------------------------------------------------- host --
struct RowsPlan {
    uint32_t path, levels, chunks0, cand0;
    uint64_t n[12];         // n[i]: elements per (candidate) row that level i reads
};

static inline uint64_t tr_next(uint64_t n, uint64_t k)
{
    const uint64_t ch = (n + TR_CH - 1) / TR_CH, tail = n - (ch - 1) * TR_CH;
    return (ch - 1) * k + (k < tail ? k : tail);
}

static inline bool tr_mul_ge_2p32(uint64_t a, uint64_t b) { return a != 0 && b > 0xffffffffull / a; }

// shape refusals shared by the plan, the size queries and the calls (row_stride is the call's own)
static inline bool tr_shape_ok(uint64_t rows, uint64_t cols, uint64_t k)
{
    if (k > cols || k > TR_MAX_K) return false;
    if (tr_mul_ge_2p32(rows, cols) || tr_mul_ge_2p32(rows, k)) return false;
    return true;
}

static inline void tr_make_plan(uint64_t cols, uint64_t k, RowsPlan *p)
{
    *p = RowsPlan{};
    p->n[0] = cols;
    p->levels = 1;
    p->chunks0 = 1;
    p->cand0 = (uint32_t)k;
    if (cols <= TR_WAVE_COLS) { p->path = 1; return; }
    if (cols <= TR_CH) { p->path = 2; return; }
    p->path = 3;
    p->chunks0 = (uint32_t)((cols + TR_CH - 1) / TR_CH);
    while (p->n[p->levels - 1] > TR_CH) {   // every level shrinks a full chunk from TR_CH to k <= TR_CH / 8: at most 5 levels below 2^32
        p->n[p->levels] = tr_next(p->n[p->levels - 1], k);
        ++p->levels;
    }
    p->cand0 = (uint32_t)p->n[1];
}

template <typename KT, int WKPT, bool HV>
static void tr_launch_wave(hipStream_t s, const typename KT::T *ki, const uint32_t *vi, typename KT::T *ko, uint32_t *vo, uint32_t rows,
                           uint32_t cols, uint32_t stride, uint32_t k, int flt, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows_wave_kernel<KT, WKPT, HV>), dim3((rows + 3u) / 4u), dim3(256), 0, s, ki, vi, ko, vo, rows, cols, stride, k,
                       flt, x);
}

template <typename T> struct BlockArgs {
    const T *src_k;
    const uint32_t *src_i;
    uint32_t src_stride, n, chunks;
    T *dst_k;
    uint32_t *dst_v;
    uint32_t dst_stride;
    const uint32_t *vals_in;
    uint32_t vals_stride, vals_cols, k;
    int flt;
    uint32_t x, rows;
};

template <typename KT, int WKPT, bool HV, bool SRC_IDX, bool FINAL>
static void tr_launch_block4(hipStream_t s, const BlockArgs<typename KT::T> &a)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows_block_kernel<KT, WKPT, HV, SRC_IDX, FINAL>), dim3(a.rows * a.chunks), dim3(TR_THREADS), 0, s, a.src_k,
                       a.src_i, a.src_stride, a.n, a.chunks, a.dst_k, a.dst_v, a.dst_stride, a.vals_in, a.vals_stride, a.vals_cols, a.k,
                       a.flt, a.x);
}

template <typename KT, int WKPT>
static void tr_launch_block(hipStream_t s, const BlockArgs<typename KT::T> &a, bool hv, bool src_idx, bool final)
{
    if (!hv) {   // keys alone: no columns to read or carry
        if (final) tr_launch_block4<KT, WKPT, false, false, true>(s, a);
        else tr_launch_block4<KT, WKPT, false, false, false>(s, a);
    } else if (src_idx) {
        if (final) tr_launch_block4<KT, WKPT, true, true, true>(s, a);
        else tr_launch_block4<KT, WKPT, true, true, false>(s, a);
    } else {
        if (final) tr_launch_block4<KT, WKPT, true, false, true>(s, a);
        else tr_launch_block4<KT, WKPT, true, false, false>(s, a);
    }
}

// The workspace: up to two areas of candidate rows, each the keys (of the caller's width) and, with values, the u32 columns.
template <typename KT>
static size_t tr_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    if (!tr_shape_ok(num_rows, num_cols, k)) return 0;
    if (num_rows == 0 || num_cols == 0 || k == 0) return 0;
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);
    size_t total = 0;
    for (uint32_t a = 1; a <= 2 && a < p.levels; ++a) {
        total += gs_ws_align(sizeof(typename KT::T) * num_rows * p.n[a]);
        if (has_values) total += gs_ws_align((size_t)4 * num_rows * p.n[a]);
    }
    return total + GS_WS_SLACK;
}

template <typename KT>
static int tr_run(void *d_temp, size_t temp_bytes, const typename KT::T *d_keys_in, const uint32_t *d_vals_in, typename KT::T *d_keys_out,
                  uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending, int key_type,
                  void *stream)
{
    using T = typename KT::T;
    GS_CLEAR_STALE_ERROR();
    if (!tr_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (row_stride < num_cols || tr_mul_ge_2p32(num_rows, row_stride)) return hipErrorInvalidValue;
    if (!KT::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < tr_temp_bytes<KT>(num_rows, num_cols, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & (sizeof(T) - 1)) != 0) return hipErrorInvalidValue;
    if ((((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & 3u) != 0) return hipErrorInvalidValue;
    {
        const size_t in_elems = (size_t)((num_rows - 1) * row_stride + num_cols), out_elems = (size_t)(num_rows * k);
        const void *arr[4] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out};
        const size_t bytes[4] = {sizeof(T) * in_elems, 4 * in_elems, sizeof(T) * out_elems, 4 * out_elems};
        if (gs_any_overlap4(arr, bytes)) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t rows = (uint32_t)num_rows, cols = (uint32_t)num_cols, stride = (uint32_t)row_stride, kk = (uint32_t)k;
    const int flt = KT::is_float(key_type);
    const uint32_t x = KT::xor_of(key_type, descending);
    RowsPlan p;
    tr_make_plan(num_cols, k, &p);

    if (p.path == 1) {
#define GS_TR_WAVE(W)                                                                                                         \
    do {                                                                                                                      \
        if (hv) tr_launch_wave<KT, W, true>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, flt, x); \
        else tr_launch_wave<KT, W, false>(s, d_keys_in, d_vals_in, d_keys_out, d_vals_out, rows, cols, stride, kk, flt, x);   \
    } while (0)
        if (cols <= 64) GS_TR_WAVE(1);
        else if (cols <= 256) GS_TR_WAVE(4);
        else if (cols <= 512) GS_TR_WAVE(8);
        else GS_TR_WAVE(16);
#undef GS_TR_WAVE
        return (int)hipGetLastError();
    }

    // paths 2 and 3: level i reads rows of n[i] elements; the candidate rows alternate between two areas of the workspace
    char *wsb = gs_ws_base(d_temp);
    T *area_k[2] = {nullptr, nullptr};
    uint32_t *area_i[2] = {nullptr, nullptr};
    {
        size_t off = 0;
        for (uint32_t a = 0; a < 2 && a + 1 < p.levels; ++a) {
            area_k[a] = (T *)(wsb + off); off += gs_ws_align(sizeof(T) * num_rows * p.n[a + 1]);
            if (hv) { area_i[a] = (uint32_t *)(wsb + off); off += gs_ws_align((size_t)4 * num_rows * p.n[a + 1]); }
        }
    }
    for (uint32_t lvl = 0; lvl < p.levels; ++lvl) {
        const bool final = lvl + 1 == p.levels;
        BlockArgs<T> a;
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
        a.k = kk; a.flt = flt; a.x = x; a.rows = rows;
        if (kk <= 64) tr_launch_block<KT, 1>(s, a, hv, lvl != 0, final);
        else if (kk <= 256) tr_launch_block<KT, 4>(s, a, hv, lvl != 0, final);
        else if (kk <= 512) tr_launch_block<KT, 8>(s, a, hv, lvl != 0, final);
        else tr_launch_block<KT, 16>(s, a, hv, lvl != 0, final);
    }
    return (int)hipGetLastError();
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
    return tr_temp_bytes<TrKey32>(num_rows, num_cols, k, has_values);
}

size_t gs_topk_rows_u16_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    return tr_temp_bytes<TrKey16>(num_rows, num_cols, k, has_values);
}

int gs_topk_rows_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                     uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                     int key_type, void *stream)
{
    return tr_run<TrKey32>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

int gs_topk_rows_u16(void *d_temp, size_t temp_bytes, const uint16_t *d_keys_in, const uint32_t *d_vals_in, uint16_t *d_keys_out,
                     uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                     int key_type, void *stream)
{
    return tr_run<TrKey16>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

}  // extern "C"
