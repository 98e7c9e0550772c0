// gs_topk_rows.hip -- gs_topk_rows_u32, gs_topk_rows_u16 and gs_topk_rows_u64: the first k of the stable sort of every row of a
// matrix, for 32-bit keys, 16-bit keys (section 10i) and 64-bit keys (section 10n).  One set of kernels
// and one host path, instantiated over a key-traits type (TrKey32, TrKey16, TrKey64); one geometry and one plan, so
// gs_topk_rows_plan answers for all three entry points.
// gs_topk_segmented_u32 (section 10k), gs_topk_segmented_u16 (section 10l) and gs_topk_segmented_u64 (section 10o), the same for
// ragged segments given by device offsets, follow them: they run the same device functions per record of lists that a classify
// kernel fills (see "ragged segments" below), instantiated over the same three key-traits types.
// gs_topk_rows_anyk_u32 (section 10p) and gs_topk_rows_anyk_u16 (section 10q), the rows form without the cap on k, are at the end
// (see "any k" below): their selects stage the k selected pairs of every row in the outputs and gs_segmented_sort_u32 /
// gs_segmented_sort_narrow finishes them.  gs_topk_rows_anyk_u64 (section 10r) follows them: path 1 is the same kernel at
// TrKey64, path 2 a descent of its own (see "any k, 64-bit keys" below), and gs_segmented_sort_wide finishes.
// gs_topk_segmented_anyk_u32 (section 10s), the ragged form without the cap on k, is the last (see "any k, ragged segments"): the
// classify, expand and wave kernels of the ragged form as they are, the any-k selects per record and per (record, tile) task.
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
//
// 64-bit keys: row r of the result is bit for bit what gs_topk_u64 gives for that row alone; on the matrix (uint64_t)key << 32
// of 32-bit keys with the key type widened it is what gs_topk_rows_u32 gives, the keys shifted back.  What the width changes:
//
//   the image    a 64-bit word in a register pair (the traits' image type I; uint32_t for the two other widths); the LDS
//                staging rows, the select's prefix and mask are 64 bits wide, values and columns stay u32.  The pad image is
//                all ones -- again an ORDINARY image (the u64 maximum, the positive NaN 0xffff...f ascending): a pad loses
//                to a real key of that image by position alone, in the stable wave sort (pads sit behind every real element
//                at the start, carry the largest digit in every pass, and every pass is stable) and in the select (pads are
//                out of range and never counted or placed).
//   the passes   up to eight, but only for bytes that can decide.  The wave sort reduces the AND and the OR of the real
//                elements' images over the wave and runs the pass of a byte only where AND ^ OR is non-zero there.  A
//                skipped pass would have been the identity: the real elements share the digit, so the stable pass keeps
//                their order, and the pads, whose digit is at least as large and which are already behind every real
//                element, stay where they are.  The decision is wave-uniform: the rows of one path-1 workgroup may run
//                different pass sets, and no barrier follows.  The select reduces AND and OR over the workgroup's in-range
//                elements once; a round whose byte is constant takes that byte into the prefix without a histogram, and a
//                chunk of one image runs no round (less = 0, the tie run cut at keff).  That decision is workgroup-uniform:
//                every thread reaches every __syncthreads.
//   the memory   one 8-byte load or store per key; candidate rows hold 8-byte keys and u32 columns.
//   the mask     the kernels take the xor mask as one 32-bit argument at every width (see TrKey64::xmask).
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
// back, flt for the float types, x the xor mask xmask(xor_of); type_ok / is_float / xor_of: the key types the entry point takes.
struct TrKey32 {
    using T = uint32_t;
    using I = uint32_t;
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
    static __device__ __forceinline__ uint32_t xmask(uint32_t x) { return x; }
};

struct TrKey16 {
    using T = uint16_t;
    using I = uint32_t;
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
    static __device__ __forceinline__ uint32_t xmask(uint32_t x) { return x; }
};

// 64-bit keys: the image fills a register pair, and so do the prefix and the mask of the select and the words of the staging
// rows.  PAD is all ones -- an ordinary image (the u64 maximum, the positive NaN 0xffff...f ascending): see the header.
struct TrKey64 {
    using T = uint64_t;
    using I = uint64_t;
    static constexpr int BITS = 64;
    static constexpr uint64_t PAD = ~0ull;
    static __device__ __forceinline__ uint64_t in(uint64_t k, int flt, uint64_t x)
    {
        if (flt) k ^= (uint64_t)((int64_t)k >> 63) | 0x8000000000000000ull;
        return k ^ x;
    }
    static __device__ __forceinline__ uint64_t out(uint64_t k, int flt, uint64_t x)
    {
        k ^= x;
        if (flt) k ^= ~(uint64_t)((int64_t)k >> 63) | 0x8000000000000000ull;
        return k;
    }
    static bool type_ok(int key_type) { return key_type >= GS_KEY_U64 && key_type <= GS_KEY_F64; }
    static int is_float(int key_type) { return key_type == GS_KEY_F64; }
    // The kernels take the xor mask as one 32-bit argument at every width: here its upper half.  The lower half is all ones
    // exactly when descending, which is bit 0 of the upper half (0, 0x80000000, 0xffffffff or 0x7fffffff).
    static uint32_t xor_of(int key_type, int descending) { return (key_type == GS_KEY_I64 ? 0x80000000u : 0u) ^ (descending ? 0xffffffffu : 0u); }
    static __device__ __forceinline__ uint64_t xmask(uint32_t x) { return ((uint64_t)x << 32) | (uint32_t)(0u - (x & 1u)); }
};

// One wave: the stable LSD sort, on the low BITS bits, of WKPT * 64 (image, value) pairs in registers; element i * 64 + lane
// is key[i].  The passes of gs_seg_wave_body.inc: per-digit ranks by match_digit, the wave's own 256 counters, a scan of 4 per
// lane, and a trip through the wave's staging rows.  All 64 lanes must be active.  BITS / 8 passes: four for a 32-bit image,
// two for a 16-bit one (whose upper half is zero in every element, so the two passes left out would move nothing).
template <int BITS, int WKPT, bool HV>
__device__ __forceinline__ void wave_sort_bits(uint32_t (&key)[WKPT], uint32_t (&val)[HV ? WKPT : 1], uint32_t /*nreal*/,
                                               uint32_t *__restrict__ my, uint32_t *__restrict__ sk, uint32_t *__restrict__ sv)
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

// A 64-bit value that is the same in every lane, from its halves: in scalar registers.  (readfirstlane returns an int: each
// half goes through uint32_t, or the low one would sign-extend into the high one.)
__device__ __forceinline__ uint64_t uniform64(uint32_t lo, uint32_t hi)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(hi) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(lo);
}

// AND and OR of a 64-bit value over the wave, in every lane.
__device__ __forceinline__ void wave_and_or64(uint64_t &a, uint64_t &o)
{
    uint32_t al = (uint32_t)a, ah = (uint32_t)(a >> 32), ol = (uint32_t)o, oh = (uint32_t)(o >> 32);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        al &= __shfl_xor(al, d, WAVE); ah &= __shfl_xor(ah, d, WAVE);
        ol |= __shfl_xor(ol, d, WAVE); oh |= __shfl_xor(oh, d, WAVE);
    }
    a = uniform64(al, ah);
    o = uniform64(ol, oh);
}

// The same sort for a 64-bit image in a register pair; the staging row sk holds 64-bit words.  Elements i * 64 + lane below
// nreal are real, the others pads (all ones, behind every real element).  A digit pass runs only for a byte in which two
// real images differ (AND ^ OR over the real elements, reduced over the wave: a wave-uniform decision, so the waves of one
// workgroup may run different pass sets -- nothing here waits on another wave).  A skipped pass would have been the
// identity: the real elements share the digit, so a stable pass keeps them in order, and the pads, whose digit is the
// largest, stay behind them where they already are.
template <int BITS, int WKPT, bool HV>
__device__ __forceinline__ void wave_sort_bits(uint64_t (&key)[WKPT], uint32_t (&val)[HV ? WKPT : 1], uint32_t nreal,
                                               uint32_t *__restrict__ my, uint64_t *__restrict__ sk, uint32_t *__restrict__ sv)
{
    static_assert(BITS == 64, "whole digits of a 64-bit image");
    const int lane = lane_id();
    auto fence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    uint64_t all_and = ~0ull, all_or = 0ull;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        if ((uint32_t)(i * WAVE + lane) < nreal) { all_and &= key[i]; all_or |= key[i]; }
    }
    wave_and_or64(all_and, all_or);
    const uint64_t differ = all_and ^ all_or;   // (no real element: ~0, every pass runs on pads alone)
#pragma unroll 1
    for (uint32_t sh = 0; sh < 64u; sh += (uint32_t)RADIX_BITS) {
        if (((differ >> sh) & 255ull) == 0ull) continue;
        uint32_t pos[WKPT];
        reinterpret_cast<uint4 *>(my)[lane] = make_uint4(0u, 0u, 0u, 0u);
        fence();
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t d = (uint32_t)(key[i] >> sh) & 255u;
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
            const uint32_t at = pos[i] + my[(uint32_t)(key[i] >> sh) & 255u];
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

// The same select for a 64-bit image: prefix and mask are 64 bits wide.  The AND and the OR of the in-range images are reduced
// over the workgroup once; a round whose byte is the same in all of them takes that byte into the prefix without a histogram
// (every in-range element still matches the prefix there, so the round would have put all of them into one bin and picked
// it), and a chunk of one image runs no round: less = 0 and the tie run is cut at keff.  The reduced words are the same in
// every thread, so every thread reaches the same barriers.
template <int BITS>
__device__ __forceinline__ uint64_t tr_select(uint64_t (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t keff, uint32_t tid,
                                              uint32_t *__restrict__ h, uint32_t *__restrict__ scratch, uint32_t *__restrict__ sel,
                                              uint32_t &less)
{
    static_assert(BITS == 64, "whole digits of a 64-bit image");
    __shared__ uint64_t red[2][TR_WAVES];
    __shared__ uint64_t sel_prefix;
    uint64_t all_and = ~0ull, all_or = 0ull;
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        if (j < len) { all_and &= img[u]; all_or |= img[u]; }
    }
    wave_and_or64(all_and, all_or);
    if ((tid & 63u) == 0u) { red[0][tid >> 6] = all_and; red[1][tid >> 6] = all_or; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < TR_WAVES; ++q) { all_and &= red[0][q]; all_or |= red[1][q]; }
    all_and = uniform64((uint32_t)all_and, (uint32_t)(all_and >> 32));
    all_or = uniform64((uint32_t)all_or, (uint32_t)(all_or >> 32));
    const uint64_t differ = all_and ^ all_or;
    uint64_t prefix = 0;
    uint32_t krem = keff;
    less = 0;
#pragma unroll 1
    for (int b = 7; b >= 0; --b) {
        const uint32_t shift = (uint32_t)b * 8u;
        if (((differ >> shift) & 255ull) == 0ull) {   // workgroup-uniform
            prefix |= all_and & (255ull << shift);
            continue;
        }
        const uint64_t mask = b == 7 ? 0ull : ~0ull << (shift + 8u);   // the bytes above this one
        if (tid < (uint32_t)RADIX) h[tid] = 0;
        __syncthreads();
        uint32_t lenv = len;
        asm volatile("" : "+v"(lenv));   // (as in the 32-bit select)
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            if (j < lenv && ((img[u] ^ prefix) & mask) == 0ull) hist_add(h, (uint32_t)(img[u] >> shift) & 255u);
        }
        __syncthreads();
        const uint32_t cnt = tid < (uint32_t)RADIX ? h[tid] : 0u;
        const uint32_t ex = block_exclusive_scan_256(cnt, scratch, nullptr);
        if (tid < (uint32_t)RADIX && ex < krem && krem - ex <= cnt) {
            sel_prefix = prefix | ((uint64_t)tid << shift);
            sel[1] = less + ex;
            sel[2] = krem - ex;
        }
        __syncthreads();
        prefix = sel_prefix; less = sel[1]; krem = sel[2];
    }
    return prefix;   // less + krem == keff: the tie run is cut at keff
}

// The ordered two-group compaction of the selected elements into LDS: group A (before the k-th image) at [0, less), group B
// (equal to it) behind, cut at keff; (wave, row, lane) is input order.  stage_v[pos] gets value_of(u, j), the value of element
// j = first + u * 64 (img[u]).  Ends with a workgroup barrier.
template <bool HV, int CAP, typename I, typename ValueOf>
__device__ __forceinline__ void tr_compact_with(I (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t keff, I kth,
                                                uint32_t less, uint32_t w, uint32_t lane, uint32_t (&wcnt)[2][TR_WAVES],
                                                I *__restrict__ stage_k, uint32_t *__restrict__ stage_v, ValueOf value_of)
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
                if (HV) stage_v[pos] = value_of(u, j);
            }
            baseA += (uint32_t)__popcll(mA);
            baseB += (uint32_t)__popcll(mB);
        }
    }
    __syncthreads();
}

// tr_compact_with for a source in memory: stage_v[pos] gets src_i[j] where the source carries columns (SRC_IDX), otherwise
// col0 + j.
template <bool HV, bool SRC_IDX, int CAP, typename I>
__device__ __forceinline__ void tr_compact(I (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t keff, I kth, uint32_t less,
                                           uint32_t w, uint32_t lane, uint32_t (&wcnt)[2][TR_WAVES], I *__restrict__ stage_k,
                                           uint32_t *__restrict__ stage_v, const uint32_t *__restrict__ src_i, uint32_t col0)
{
    tr_compact_with<HV, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v,
                             [=](int, uint32_t j) { return SRC_IDX ? src_i[j] : col0 + j; });
}

// ------------------------------------------------------------------ path 1 --
// One wave per row of up to WKPT * 64 columns, four rows per workgroup; waves past the last row leave (no barrier follows).
template <typename KT, int WKPT, bool HV>
__global__ __launch_bounds__(256) void topk_rows_wave_kernel(const typename KT::T *__restrict__ keys, const uint32_t *__restrict__ vals_in,
                                                             typename KT::T *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                             uint32_t rows, uint32_t cols, uint32_t stride, uint32_t k, int flt, uint32_t x32)
{
    using T = typename KT::T;
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][RADIX];
    __shared__ I stage_k[4][CAP];
    __shared__ uint32_t stage_v[HV ? 4 : 1][HV ? CAP : 1];
    const int w = wave_id(), lane = lane_id();
    const uint32_t r = blockIdx.x * 4u + (uint32_t)w;
    if (r >= rows) return;
    const size_t in0 = (size_t)r * stride, out0 = (size_t)r * k;
    I key[WKPT];
    uint32_t val[HV ? WKPT : 1];
    const uint32_t last = cols - 1u;
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = (I)__builtin_nontemporal_load(keys + in0 + (idx < last ? idx : last));   // past the end: the row's last element again
    }
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)(i * WAVE + lane);
        key[i] = idx < cols ? KT::in(key[i], flt, x) : KT::PAD;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx;
    }
    wave_sort_bits<KT::BITS, WKPT, HV>(key, val, cols, hist[w], stage_k[w], stage_v[HV ? w : 0]);
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
                                                                     uint32_t vals_cols, uint32_t k, int flt, uint32_t x32)
{
    using T = typename KT::T;
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];   // the select's histogram, then the finishing wave's counters
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    __shared__ I stage_k[CAP], sort_k[CAP];
    __shared__ uint32_t stage_v[HV ? CAP : 1], sort_v[HV ? CAP : 1];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / chunks, c = blockIdx.x - r * chunks;
    const uint32_t lo = c * TR_CH, len = n - lo < TR_CH ? n - lo : TR_CH, keff = k < len ? k : len;
    const size_t base = (size_t)r * src_stride + lo;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;

    I img[TR_KPT];
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        img[u] = j < len ? (I)__builtin_nontemporal_load(src_k + base + j) : (I)0u;
    }
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) img[u] = KT::in(img[u], flt, x);

    // radix select of the keff-th image on the registers, then the ordered compaction of the keff selected pairs into LDS
    uint32_t less;
    const I kth = tr_select<KT::BITS>(img, first, len, keff, tid, h, scratch, sel, less);
    tr_compact<HV, SRC_IDX, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v, SRC_IDX ? src_i + base : nullptr, lo);

    // finish: one wave sorts the keff staged pairs and stores them
    if (w != 0) return;
    I key[WKPT];
    uint32_t val[HV ? WKPT : 1];
#pragma unroll
    for (int i = 0; i < WKPT; ++i) {
        const uint32_t idx = (uint32_t)i * WAVE + lane;
        key[i] = idx < keff ? stage_k[idx] : KT::PAD;   // pads: last in position, largest in every digit
        if (HV) val[i] = idx < keff ? stage_v[idx] : 0u;
    }
    wave_sort_bits<KT::BITS, WKPT, HV>(key, val, keff, h, sort_k, sort_v);
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

template <typename KT> struct BlockArgs {
    using T = typename KT::T;
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
static void tr_launch_block4(hipStream_t s, const BlockArgs<KT> &a)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_rows_block_kernel<KT, WKPT, HV, SRC_IDX, FINAL>), dim3(a.rows * a.chunks), dim3(TR_THREADS), 0, s, a.src_k,
                       a.src_i, a.src_stride, a.n, a.chunks, a.dst_k, a.dst_v, a.dst_stride, a.vals_in, a.vals_stride, a.vals_cols, a.k,
                       a.flt, a.x);
}

template <typename KT, int WKPT>
static void tr_launch_block(hipStream_t s, const BlockArgs<KT> &a, bool hv, bool src_idx, bool final)
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
        BlockArgs<KT> a;
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

// ------------------------------------------------------------ ragged segments --
// gs_topk_segmented_u32 / _u16 / _u64 (DESIGN.md sections 10k, 10l, 10o): the k best of every segment of a flat array, the segments given by device
// offsets.  The lengths are on the device, so a classify kernel sorts the segments into six lists of records by length and
// the kernels above run per record: the four wave classes of path 1 (<= 64 / 256 / 512 / 1024 elements), the workgroup of
// path 2 (<= CH), and for longer segments level 0 of path 3 per (record, chunk) task followed by ONE streaming final per
// segment: a workgroup reads its candidate row CH elements at a time, the carried best k of the rounds before in front of the
// new candidates, and selects again.  Carried elements are in the order the last compaction left them (group A in input
// order, then the cut tie run in input order) and precede every new candidate, so equal images stay in position order from
// round to round and the one stable wave sort at the end reproduces the definition.
// Every record, task and cursor read from the workspace is clamped against the arguments before it becomes an address.
constexpr uint32_t TS_MAX_GRID = 16384;   // workgroups per launch; the kernels stride over longer lists
constexpr int TS_BLOCK = 4, TS_LONG = 5;   // lists 0..3: the wave classes
// words of the state block: [0..4] the counts of the wave and block lists, [5] long segments that found room, [6] dropped
// segments, [7] the chunk tasks of [5]; the cursors the long segments claim from: [8..9] chunk-task slots (64 bits: what
// overlapping segments ask for together may pass 2^32), [10] records
constexpr int TS_LONG_OK = 5, TS_DROPPED = 6, TS_TASKS_OK = 7, TS_TASK_CUR = 8, TS_REC_CUR = 10, TS_STATE_BYTES = 4096;

struct TsRec { uint32_t base, len, seg, row; };   // row: the first chunk-task slot of a long segment (its candidate row is row * k)
struct TsTask { uint32_t rec, chunk; };
static_assert(sizeof(TsRec) == 16 && sizeof(TsTask) == 8, "the sizes of the header's workspace formula");

struct TsWs {
    uint32_t *state;
    TsRec *list[6];
    TsTask *tasks;
    void *cand_k;                // candidate rows: images, as wide as the key (KT::T), and
    uint32_t *cand_p;            // (with values) positions within the segment
    uint32_t nseg, lmax, tmax;
};

// A kernel argument that is uniform but used rarely (an output pointer that only the finishing wave needs, a bound checked
// once per record): kept in vector registers across the select and the compaction, whose ballots need the scalar ones.
template <typename P> __device__ __forceinline__ P *ts_in_vgprs(P *p)
{
    unsigned long long v = (unsigned long long)(uintptr_t)p;
    asm volatile("" : "+v"(v));
    return (P *)(uintptr_t)v;
}
__device__ __forceinline__ uint32_t ts_in_vgpr(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// a record of the kernels' own lists, clamped like a caller's offsets: false when nothing of it may be touched
__device__ __forceinline__ bool ts_load_rec(const TsRec *__restrict__ list, uint32_t at, uint32_t num_items, uint32_t nseg, uint32_t cap,
                                            uint32_t &base, uint32_t &len, uint32_t &seg, uint32_t &row)
{
    const uint4 rv = reinterpret_cast<const uint4 *>(list)[at];
    base = __builtin_amdgcn_readfirstlane(rv.x); len = __builtin_amdgcn_readfirstlane(rv.y);
    seg = __builtin_amdgcn_readfirstlane(rv.z); row = __builtin_amdgcn_readfirstlane(rv.w);
    if (__builtin_amdgcn_readfirstlane(base >= num_items || seg >= nseg || len == 0u)) return false;
    const uint32_t room = num_items - base, most = room < cap ? room : cap;
    if (len > most) len = __builtin_amdgcn_readfirstlane(most);
    return true;
}

// Four segments per thread, one LDS atomic per thread and list, one global atomic per workgroup and list (the pattern of
// seg_classify_kernel).  A long segment claims a record slot and ceil(len / CH) chunk-task slots the same way: its share of
// the workgroup's LDS counter (records and tasks packed into one word, so the two shares are taken in one order), then of
// the two cursors the workgroup advanced once.  A claim is made once and never retried.  One that passes either capacity
// drops the segment: count 0, nothing of it written (its record slot, if it got one, holds an empty record).  The cursors
// only grow, so after one dropped segment a later one may be dropped although it alone would have fitted.
__global__ __launch_bounds__(256) void topk_seg_classify_kernel(TsWs ws, const int *__restrict__ seg_begin, const int *__restrict__ seg_end,
                                                                uint32_t num_items, uint32_t k, uint32_t *__restrict__ counts_out)
{
    constexpr int SPT = 4, NL = 5;
    __shared__ uint32_t s_cnt[NL], s_base[NL + 1];   // s_base[NL]: the first record slot of the workgroup's long segments
    __shared__ unsigned long long s_long, s_task_base;   // s_long: their number (high half) and their chunk tasks (low half)
    const int tid = threadIdx.x;
    const uint32_t nseg = ws.nseg;
    for (uint32_t base = blockIdx.x * (256u * SPT); base < nseg; base += gridDim.x * (256u * SPT)) {
        if (tid < NL) s_cnt[tid] = 0;
        if (tid == NL) s_long = 0;
        __syncthreads();
        uint32_t b[SPT], size[SPT], off[NL], cnt[NL], lrec[SPT], ltask[SPT];
        int list[SPT];
#pragma unroll
        for (int q = 0; q < NL; ++q) cnt[q] = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            const uint32_t sg = base + (uint32_t)tid * SPT + j;
            b[j] = 0; size[j] = 0; list[j] = -1;
            if (sg < nseg) {
                int lo = seg_begin[sg], hi = seg_end[sg];
                if (lo < 0) lo = 0;                                 // offsets outside [0, num_items] are clamped so that they
                if (hi > (int)num_items) hi = (int)num_items;       // cannot become out-of-bounds accesses
                if (hi > lo) { b[j] = (uint32_t)lo; size[j] = (uint32_t)(hi - lo); }
            }
            const uint32_t sz = size[j];
            lrec[j] = 0; ltask[j] = 0;
            if (sz != 0u && sz <= TR_WAVE_COLS) list[j] = sz <= (uint32_t)WAVE ? 0 : sz <= 256u ? 1 : sz <= 512u ? 2 : 3;
            else if (sz != 0u && sz <= TR_CH) list[j] = TS_BLOCK;
            else if (sz != 0u) {          // rare: an LDS atomic each (1024 segments of fewer than 2^18 chunks: the low half holds them)
                list[j] = TS_LONG;
                const unsigned long long mine = atomicAdd(&s_long, (1ull << 32) | (unsigned long long)((sz + TR_CH - 1u) / TR_CH));
                lrec[j] = (uint32_t)(mine >> 32);
                ltask[j] = (uint32_t)mine;
            }
            if (sg < nseg && counts_out && list[j] != TS_LONG) counts_out[sg] = sz < k ? sz : k;
#pragma unroll
            for (int q = 0; q < NL; ++q) cnt[q] += list[j] == q ? 1u : 0u;
        }
#pragma unroll
        for (int q = 0; q < NL; ++q) off[q] = cnt[q] ? atomicAdd(&s_cnt[q], cnt[q]) : 0u;       // LDS
        __syncthreads();
        if (tid < NL && s_cnt[tid] != 0u) s_base[tid] = atomicAdd(&ws.state[tid], s_cnt[tid]);
        if (tid == NL && s_long != 0ull) {
            s_base[NL] = atomicAdd(&ws.state[TS_REC_CUR], (uint32_t)(s_long >> 32));
            s_task_base = atomicAdd(reinterpret_cast<unsigned long long *>(ws.state + TS_TASK_CUR), s_long & 0xffffffffull);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                if (list[j] != q) continue;
                const uint32_t at = s_base[q] + off[q]++;
                if (at < nseg) ws.list[q][at] = TsRec{b[j], size[j], base + (uint32_t)tid * SPT + j, 0u};
            }
            if (list[j] == TS_LONG) {
                const uint32_t sg = base + (uint32_t)tid * SPT + j, chunks = (size[j] + TR_CH - 1u) / TR_CH;
                const uint32_t rec = s_base[NL] + lrec[j];
                const unsigned long long task = s_task_base + ltask[j];
                const bool fits = rec < ws.lmax && task + chunks <= (unsigned long long)ws.tmax;
                if (fits) {
                    ws.list[TS_LONG][rec] = TsRec{b[j], size[j], sg, (uint32_t)task};
                    atomicAdd(&ws.state[TS_LONG_OK], 1u);
                    atomicAdd(&ws.state[TS_TASKS_OK], chunks);
                } else {
                    if (rec < ws.lmax) ws.list[TS_LONG][rec] = TsRec{0u, 0u, 0u, 0u};
                    atomicAdd(&ws.state[TS_DROPPED], 1u);
                }
                if (counts_out) counts_out[sg] = fits ? (size[j] < k ? size[j] : k) : 0u;
            }
        }
        __syncthreads();
    }
}

// topk_rows_wave_kernel per record of wave list LIST: base and length from the record, stores at seg * k + idx for idx < kept.
// (The 64-bit wave sort decides its passes per wave: the four segments of a workgroup may run different sets, and no
// workgroup barrier follows anywhere in this kernel.)
template <typename KT, int WKPT, bool HV>
__global__ __launch_bounds__(256) void topk_seg_wave_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                            const uint32_t *__restrict__ vals_in, typename KT::T *__restrict__ keys_out,
                                                            uint32_t *__restrict__ vals_out, uint32_t num_items, uint32_t k, int flt, uint32_t x32)
{
    using T = typename KT::T;
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    constexpr int CAP = WKPT * WAVE, LIST = WKPT == 1 ? 0 : WKPT == 4 ? 1 : WKPT == 8 ? 2 : 3;
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][RADIX];
    __shared__ I stage_k[4][CAP];
    __shared__ uint32_t stage_v[HV ? 4 : 1][HV ? CAP : 1];
    const int w = wave_id(), lane = lane_id();
    uint32_t count = ws.state[LIST];
    if (count > ws.nseg) count = ws.nseg;
    for (uint32_t t = blockIdx.x * 4u + (uint32_t)w; t < count; t += gridDim.x * 4u) {
        uint32_t base, cols, seg, row;
        if (!ts_load_rec(ws.list[LIST], t, num_items, ws.nseg, (uint32_t)CAP, base, cols, seg, row)) continue;
        const size_t in0 = base, out0 = (size_t)seg * k;
        const uint32_t kept = k < cols ? k : cols;
        I key[WKPT];
        uint32_t val[HV ? WKPT : 1];
        const uint32_t last = cols - 1u;
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t idx = (uint32_t)(i * WAVE + lane);
            key[i] = (I)__builtin_nontemporal_load(keys + in0 + (idx < last ? idx : last));   // past the end: the last element again
        }
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t idx = (uint32_t)(i * WAVE + lane);
            key[i] = idx < cols ? KT::in(key[i], flt, x) : KT::PAD;   // pads: last in position, largest in every digit
            if (HV) val[i] = idx;
        }
        wave_sort_bits<KT::BITS, WKPT, HV>(key, val, cols, hist[w], stage_k[w], stage_v[HV ? w : 0]);
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t idx = (uint32_t)(i * WAVE + lane);
            if (idx < kept) {
                keys_out[out0 + idx] = (T)KT::out(key[i], flt, x);
                if (HV) vals_out[out0 + idx] = vals_in ? vals_in[in0 + (val[i] < cols ? val[i] : last)] : val[i];
            }
        }
    }
}

// topk_rows_block_kernel's body per record of the block list, or (CHUNK) per (record, chunk) task of the long list.  The
// block list's results go to the caller's outputs at seg * k; a chunk's min(k, chunk length) sorted (image, position in the
// segment) pairs go to slot row + chunk of the candidate area (every chunk but the last gives k, so the segment's candidate
// row is dense).  Candidate rows hold images, stored KT::T wide (the image of a 16-bit key has a zero upper half): the final
// widens them back into the register.
template <typename KT, int WKPT, bool HV, bool CHUNK>
__global__ __launch_bounds__(TR_THREADS) void topk_seg_block_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                                    const uint32_t *__restrict__ vals_in,
                                                                    typename KT::T *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                                    uint32_t num_items, uint32_t k, int flt, uint32_t x32)
{
    using T = typename KT::T;
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];   // the select's histogram, then the finishing wave's counters
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    __shared__ I stage_k[CAP], sort_k[CAP];
    __shared__ uint32_t stage_v[HV ? CAP : 1], sort_v[HV ? CAP : 1];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    uint32_t count, nrec = 0;
    if (CHUNK) {   // the cursors, not the counts of completed claims: a dropped segment leaves a hole behind it
        count = ws.state[TS_TASK_CUR + 1] != 0u ? ws.tmax : ws.state[TS_TASK_CUR];
        nrec = ws.state[TS_REC_CUR];
        if (count > ws.tmax) count = ws.tmax;
        if (nrec > ws.lmax) nrec = ws.lmax;
        nrec = ts_in_vgpr(nrec);
    } else {
        count = ws.state[TS_BLOCK];
        if (count > ws.nseg) count = ws.nseg;
    }
    const TsRec *const recs = ts_in_vgprs(ws.list[CHUNK ? TS_LONG : TS_BLOCK]);
    const TsTask *const tasks = ts_in_vgprs(ws.tasks);
    T *const dst_ck = ts_in_vgprs((T *)ws.cand_k);
    uint32_t *const dst_cp = ts_in_vgprs(ws.cand_p);
    const uint32_t *const vin = ts_in_vgprs(vals_in);
    T *const kout = ts_in_vgprs(keys_out);
    uint32_t *const vout = ts_in_vgprs(vals_out);
    const uint32_t nseg = ts_in_vgpr(ws.nseg), tmax = ts_in_vgpr(ws.tmax), nitems = ts_in_vgpr(num_items);
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {   // (t and everything decided from it are uniform: the barriers are safe)
        uint32_t base, slen, seg, row, c = 0, at = t;
        if (CHUNK) {
            const TsTask task = tasks[t];
            at = __builtin_amdgcn_readfirstlane(task.rec); c = __builtin_amdgcn_readfirstlane(task.chunk);
            if (__builtin_amdgcn_readfirstlane(at >= nrec)) continue;
        }
        if (!ts_load_rec(recs, at, nitems, nseg, CHUNK ? nitems : TR_CH, base, slen, seg, row)) continue;
        // (a slot whose claim was dropped was never written by the expand kernel: whatever it holds is not the task of this slot)
        if (CHUNK && __builtin_amdgcn_readfirstlane(c >= (slen + TR_CH - 1u) / TR_CH || row >= tmax || c >= tmax - row || row + c != t)) continue;
        const uint32_t lo = c * TR_CH, len = slen - lo < TR_CH ? slen - lo : TR_CH, keff = k < len ? k : len;
        const size_t in0 = (size_t)base + lo;

        I img[TR_KPT];
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            img[u] = j < len ? (I)__builtin_nontemporal_load(keys + in0 + j) : (I)0u;
        }
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) img[u] = KT::in(img[u], flt, x);
        // where the result goes, and the segment the values come from: for the stores at the end.  The 16-bit kernels with
        // values are two scalar registers short across the select; the 32-bit ones are not, and keep the code they had; the
        // 64-bit ones are not either (at most 104 scalar registers, no spill: DESIGN.md section 10o).
        uint32_t slot = CHUNK ? row + c : seg, vbase = base, vlen = slen;
        if (sizeof(T) == 2) { slot = ts_in_vgpr(slot); vbase = ts_in_vgpr(vbase); vlen = ts_in_vgpr(vlen); }

        uint32_t less;
        const I kth = tr_select<KT::BITS>(img, first, len, keff, tid, h, scratch, sel, less);
        tr_compact<HV, false, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v, nullptr, lo);

        if (w == 0) {   // finish: one wave sorts the keff staged pairs and stores them
            I key[WKPT];
            uint32_t val[HV ? WKPT : 1];
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t idx = (uint32_t)i * WAVE + lane;
                key[i] = idx < keff ? stage_k[idx] : KT::PAD;   // pads: last in position, largest in every digit
                if (HV) val[i] = idx < keff ? stage_v[idx] : 0u;
            }
            wave_sort_bits<KT::BITS, WKPT, HV>(key, val, keff, h, sort_k, sort_v);
            const size_t out0 = (size_t)slot * k;
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t idx = (uint32_t)i * WAVE + lane;
                if (idx < keff) {
                    if (CHUNK) {
                        dst_ck[out0 + idx] = (T)key[i];
                        if (HV) dst_cp[out0 + idx] = val[i];
                    } else {
                        kout[out0 + idx] = (T)KT::out(key[i], flt, x);
                        if (HV) vout[out0 + idx] = vin ? vin[(size_t)vbase + (val[i] < vlen ? val[i] : vlen - 1u)] : val[i];
                    }
                }
            }
        }
        __syncthreads();   // the finishing wave is done with h and the stage before the next record's select
    }
}

// One workgroup per long record writes the (record, chunk) pairs of its task slots.
__global__ __launch_bounds__(256) void topk_seg_expand_kernel(TsWs ws, uint32_t num_items)
{
    uint32_t nrec = ws.state[TS_REC_CUR];
    if (nrec > ws.lmax) nrec = ws.lmax;
    for (uint32_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        uint32_t base, len, seg, row;
        if (!ts_load_rec(ws.list[TS_LONG], r, num_items, ws.nseg, num_items, base, len, seg, row)) continue;
        const uint32_t chunks = (len + TR_CH - 1u) / TR_CH;
        if (row >= ws.tmax || chunks > ws.tmax - row) continue;
        for (uint32_t c = threadIdx.x; c < chunks; c += 256u) ws.tasks[row + c] = TsTask{r, c};
    }
}

// The streaming final: one workgroup per long record.  A round holds a virtual chunk of up to CH elements in registers:
// the kc carried pairs from the stage first, in the order the last compaction left them, then the next CH - kc candidates
// of the segment's row; tr_select and the compaction put the best min(k, elements so far) back into the stage.  After the
// last round wave 0 sorts the stage and stores.  A row that fits one chunk is one round.
template <typename KT, int WKPT, bool HV>
__global__ __launch_bounds__(TR_THREADS) void topk_seg_final_kernel(TsWs ws, const uint32_t *__restrict__ vals_in,
                                                                    typename KT::T *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                                    uint32_t num_items, uint32_t k, int flt, uint32_t x32)
{
    using T = typename KT::T;
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    constexpr int CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    __shared__ I stage_k[CAP], sort_k[CAP];
    __shared__ uint32_t stage_v[HV ? CAP : 1], sort_v[HV ? CAP : 1];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    uint32_t nrec = ws.state[TS_REC_CUR];
    if (nrec > ws.lmax) nrec = ws.lmax;
    const TsRec *const recs = ts_in_vgprs(ws.list[TS_LONG]);
    const T *const src_ck = ts_in_vgprs((const T *)ws.cand_k);
    const uint32_t *const src_cp = ts_in_vgprs(ws.cand_p);
    const uint32_t *const vin = ts_in_vgprs(vals_in);
    T *const kout = ts_in_vgprs(keys_out);
    uint32_t *const vout = ts_in_vgprs(vals_out);
    const uint32_t nseg = ts_in_vgpr(ws.nseg), tmax = ts_in_vgpr(ws.tmax), nitems = ts_in_vgpr(num_items);
    for (uint32_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        uint32_t base, slen, seg, row;
        if (!ts_load_rec(recs, r, nitems, nseg, nitems, base, slen, seg, row)) continue;
        const uint32_t chunks = (slen + TR_CH - 1u) / TR_CH, tail = slen - (chunks - 1u) * TR_CH;
        if (__builtin_amdgcn_readfirstlane(row >= tmax || chunks > tmax - row)) continue;
        const uint32_t n1 = (chunks - 1u) * k + (k < tail ? k : tail);      // next(len): the candidates the chunks left
        const T *ck = src_ck + (size_t)row * k;
        const uint32_t *cp = src_cp + (size_t)row * k;
        base = ts_in_vgpr(base); slen = ts_in_vgpr(slen); seg = ts_in_vgpr(seg);   // for the stores at the end
        uint32_t kc = 0, pos = 0;
        do {
            const uint32_t room = TR_CH - kc, left = n1 - pos, take = left < room ? left : room, len = kc + take;
            const uint32_t keff = k < len ? k : len;
            I img[TR_KPT];
            uint32_t val[HV ? TR_KPT : 1];
#pragma unroll
            for (int u = 0; u < TR_KPT; ++u) {
                const uint32_t j = first + (uint32_t)u * WAVE;
                if (j < kc) {
                    img[u] = stage_k[j];
                    if (HV) val[u] = stage_v[j];
                } else if (j < len) {
                    img[u] = (I)__builtin_nontemporal_load(ck + pos + (j - kc));
                    if (HV) val[u] = __builtin_nontemporal_load(cp + pos + (j - kc));
                } else {
                    img[u] = (I)0u;
                    if (HV) val[u] = 0u;
                }
            }
            // The select's first barrier orders the stage reads above before the compaction's writes.  The 64-bit select always
            // has one: the barrier behind its `red` words comes first whatever rounds it then skips.  Its AND / OR run over
            // img[] of this virtual chunk, the carried pairs and the new candidates alike, so a byte that only one carried
            // element varies still gets its round.  Between this round's reads of `red` (and of the picked prefix) and the next
            // round's writes lie the two barriers of the compaction.
            uint32_t less;
            const I kth = tr_select<KT::BITS>(img, first, len, keff, tid, h, scratch, sel, less);
            tr_compact_with<HV, CAP>(img, first, len, keff, kth, less, w, lane, wcnt, stage_k, stage_v,
                                     [&](int u, uint32_t) { return val[HV ? u : 0]; });
            kc = keff;
            pos += take;
        } while (pos < n1);

        if (w == 0) {
            I key[WKPT];
            uint32_t val[HV ? WKPT : 1];
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t idx = (uint32_t)i * WAVE + lane;
                key[i] = idx < kc ? stage_k[idx] : KT::PAD;
                if (HV) val[i] = idx < kc ? stage_v[idx] : 0u;
            }
            wave_sort_bits<KT::BITS, WKPT, HV>(key, val, kc, h, sort_k, sort_v);
            const size_t out0 = (size_t)seg * k;
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t idx = (uint32_t)i * WAVE + lane;
                if (idx < kc) {
                    kout[out0 + idx] = (T)KT::out(key[i], flt, x);
                    if (HV) vout[out0 + idx] = vin ? vin[(size_t)base + (val[i] < slen ? val[i] : slen - 1u)] : val[i];
                }
            }
        }
        __syncthreads();
    }
}

// ---- host
struct TsGeom { uint64_t lmax, tmax; };

static inline bool ts_shape_ok(uint64_t num_items, uint64_t num_segments, uint64_t k)
{
    return k <= TR_MAX_K && num_items < (1ull << 31) && !tr_mul_ge_2p32(num_segments, k);
}

static inline TsGeom ts_geom(uint64_t num_items, uint64_t num_segments)
{
    TsGeom g;
    g.lmax = num_items / (TR_CH + 1);
    if (g.lmax > num_segments) g.lmax = num_segments;
    g.tmax = g.lmax ? num_items / TR_CH + g.lmax : 0;
    return g;
}

// the carve and the size query in one walk (base may be null: the query).  key_bytes: the width of a candidate image, the
// only term that depends on the key; the state block comes first at every width, so ts_status reads any of the workspaces.
static size_t ts_carve(char *base, uint64_t num_items, uint64_t num_segments, uint64_t k, bool hv, size_t key_bytes, TsWs *ws)
{
    const TsGeom g = ts_geom(num_items, num_segments);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = (char *)((uintptr_t)base + off); off += gs_ws_align(bytes); return p; };
    TsWs w{};
    w.state = (uint32_t *)take(TS_STATE_BYTES);
    for (int q = 0; q < 5; ++q) w.list[q] = (TsRec *)take(sizeof(TsRec) * num_segments);
    w.list[TS_LONG] = (TsRec *)take(sizeof(TsRec) * g.lmax);
    w.tasks = (TsTask *)take(sizeof(TsTask) * g.tmax);
    w.cand_k = take(key_bytes * k * g.tmax);
    w.cand_p = (uint32_t *)w.cand_k;   // (never read without values)
    if (hv) w.cand_p = (uint32_t *)take((size_t)4 * k * g.tmax);
    w.nseg = (uint32_t)num_segments; w.lmax = (uint32_t)g.lmax; w.tmax = (uint32_t)g.tmax;
    if (ws) *ws = w;
    return off;
}

static size_t ts_temp_bytes(uint64_t num_items, uint64_t num_segments, uint64_t k, int has_values, size_t key_bytes)
{
    if (!ts_shape_ok(num_items, num_segments, k)) return 0;
    if (num_items == 0 || num_segments == 0 || k == 0) return 0;
    return ts_carve(nullptr, num_items, num_segments, k, has_values != 0, key_bytes, nullptr) + GS_WS_SLACK;
}

// the launch groups of a shape: bit 0 wave, bit 1 block, bit 2 long
static inline uint32_t ts_groups(uint64_t num_items) { return 1u | (num_items > TR_WAVE_COLS ? 2u : 0u) | (num_items > TR_CH ? 4u : 0u); }
static inline uint32_t ts_launches(uint32_t groups) { return 2u + 4u + ((groups & 2u) ? 1u : 0u) + ((groups & 4u) ? 3u : 0u); }

template <typename KT, int WKPT, bool HV>
static void ts_launch_wave(hipStream_t s, const TsWs &ws, uint32_t grid, const typename KT::T *ki, const uint32_t *vi, typename KT::T *ko,
                           uint32_t *vo, uint32_t n, uint32_t k, int flt, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_seg_wave_kernel<KT, WKPT, HV>), dim3(grid), dim3(256), 0, s, ws, ki, vi, ko, vo, n, k, flt, x);
}

template <typename KT, int WKPT, bool HV>
static void ts_launch_select(hipStream_t s, const TsWs &ws, uint32_t groups, const typename KT::T *ki, const uint32_t *vi,
                             typename KT::T *ko, uint32_t *vo, uint32_t n, uint32_t k, int flt, uint32_t x)
{
    const uint32_t gb = ws.nseg < TS_MAX_GRID ? ws.nseg : TS_MAX_GRID;
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL((topk_seg_block_kernel<KT, WKPT, HV, false>), dim3(gb), dim3(TR_THREADS), 0, s, ws, ki, vi, ko, vo, n, k, flt, x); }
    if (!(groups & 4u)) return;
    const uint32_t gl = ws.lmax < TS_MAX_GRID ? ws.lmax : TS_MAX_GRID, gt = ws.tmax < TS_MAX_GRID ? ws.tmax : TS_MAX_GRID;
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk_seg_expand_kernel, dim3(gl), dim3(256), 0, s, ws, n); }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL((topk_seg_block_kernel<KT, WKPT, HV, true>), dim3(gt), dim3(TR_THREADS), 0, s, ws, ki, vi, ko, vo, n, k, flt, x); }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL((topk_seg_final_kernel<KT, WKPT, HV>), dim3(gl), dim3(TR_THREADS), 0, s, ws, vi, ko, vo, n, k, flt, x); }
}

template <typename KT>
static int ts_run(void *d_temp, size_t temp_bytes, const typename KT::T *d_keys_in, const uint32_t *d_vals_in, typename KT::T *d_keys_out,
                  uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments, const int32_t *d_begin_offsets,
                  const int32_t *d_end_offsets, uint64_t k, int descending, int key_type, void *stream)
{
    using T = typename KT::T;
    GS_CLEAR_STALE_ERROR();
    if (!ts_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (!KT::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out || !d_begin_offsets || !d_end_offsets) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < ts_temp_bytes(num_items, num_segments, k, hv, sizeof(T))) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & (sizeof(T) - 1)) != 0) return hipErrorInvalidValue;
    if ((((uintptr_t)d_vals_in | (uintptr_t)d_vals_out | (uintptr_t)d_counts_out | (uintptr_t)d_begin_offsets | (uintptr_t)d_end_offsets) & 3u) != 0)
        return hipErrorInvalidValue;
    {   // no array may share a byte with another, except that the two offset arrays (both only read) may: begin + 1 == end is usual
        const size_t out_elems = (size_t)num_segments * k;
        const void *arr[7] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, d_begin_offsets, d_end_offsets};
        const size_t bytes[7] = {sizeof(T) * num_items, 4 * num_items, sizeof(T) * out_elems, 4 * out_elems, (size_t)4 * num_segments,
                                 (size_t)4 * num_segments, (size_t)4 * num_segments};
        for (int i = 0; i < 7; ++i)
            for (int j = i + 1; j < 7; ++j)
                if (!(i == 5 && j == 6) && gs_ranges_overlap(arr[i], bytes[i], arr[j], bytes[j])) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_items, kk = (uint32_t)k;
    const int flt = KT::is_float(key_type);
    const uint32_t x = KT::xor_of(key_type, descending);
    TsWs ws;
    ts_carve(gs_ws_base(d_temp), num_items, num_segments, k, hv, sizeof(T), &ws);
    const uint32_t groups = ts_groups(num_items);

    hipError_t e = zero_async(ws.state, TS_STATE_BYTES, s);
    if (e != hipSuccess) return (int)e;
    { KernelTimer kt(GS_K_OTHER, s);
      const uint32_t g = (num_segments + 1023u) / 1024u;
      hipLaunchKernelGGL(topk_seg_classify_kernel, dim3(g < 4096u ? g : 4096u), dim3(256), 0, s, ws, d_begin_offsets, d_end_offsets, n, kk,
                         d_counts_out); }
    {
        const uint32_t wg = (num_segments + 3u) / 4u, grid = wg < TS_MAX_GRID ? wg : TS_MAX_GRID;
#define GS_TS_WAVE(W)                                                                                               \
    do {                                                                                                            \
        if (hv) ts_launch_wave<KT, W, true>(s, ws, grid, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x); \
        else ts_launch_wave<KT, W, false>(s, ws, grid, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x);   \
    } while (0)
        GS_TS_WAVE(1); GS_TS_WAVE(4); GS_TS_WAVE(8); GS_TS_WAVE(16);
#undef GS_TS_WAVE
    }
    if (groups & 2u) {
#define GS_TS_SELECT(W)                                                                                                  \
    do {                                                                                                                 \
        if (hv) ts_launch_select<KT, W, true>(s, ws, groups, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x); \
        else ts_launch_select<KT, W, false>(s, ws, groups, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x);   \
    } while (0)
        if (kk <= 64) GS_TS_SELECT(1);
        else if (kk <= 256) GS_TS_SELECT(4);
        else if (kk <= 512) GS_TS_SELECT(8);
        else GS_TS_SELECT(16);
#undef GS_TS_SELECT
    }
    return (int)hipGetLastError();
}

static int ts_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, uint32_t out[8])
{
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!ts_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;   // such a call enqueues nothing
    const TsGeom g = ts_geom(num_items, num_segments);
    out[0] = ts_groups(num_items); out[1] = ts_launches(out[0]); out[2] = TR_CH; out[3] = (uint32_t)g.lmax; out[4] = (uint32_t)g.tmax;
    out[5] = TR_MAX_K;
    return hipSuccess;
}

static int ts_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!ts_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;   // such a call enqueued nothing
    if (!d_temp) return hipErrorInvalidValue;
    TsWs ws;
    ts_carve(gs_ws_base(d_temp), num_items, num_segments, k, has_values != 0, 4, &ws);   // (only the state block, the first term, is read)
    uint32_t st[16];
    hipError_t e = hipMemcpyAsync(st, ws.state, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    for (int q = 0; q < 5; ++q) out[q] = st[q];
    out[5] = st[TS_LONG_OK]; out[6] = st[TS_TASKS_OK]; out[7] = st[TS_DROPPED];
    return hipSuccess;
}

// ------------------------------------------------------------------- any k --
// gs_topk_rows_anyk_u32: the k best of every row with no cap on k.  A select stages the k selected
// (key, column) pairs of every row, unsorted but with equal keys in column order, at [r * k, r * k + k) of the outputs, and
// gs_segmented_sort_u32 with the regular offsets r * k finishes them, stably, on all 32 bits.  Two selects, by num_cols alone:
//
//   path 1   num_cols <= CH: one workgroup per row, the row read once: tr_select for the k-th image, then the ordered two-group
//            placement straight into the row's k slots in global memory.  No global atomic, no histogram in memory.
//   path 2   longer rows: a radix select over all rows at once in three counting rounds on image bits 31-21, 20-10 and 9-0.  A
//            count kernel, one workgroup per (row, slab of whole tiles of CH columns), histograms the round's digit in LDS over
//            the elements that match the row's prefix so far and adds its non-zero bins to the row's histogram in memory
//            (integer adds: the sums do not depend on their order); a pick kernel, one workgroup per row, scans the bins, picks
//            the digit that holds the krem-th element, updates the row's record and clears the histogram.  Then per (row, tile)
//            two counts (before / equal to the k-th image), a scan per row, and a scatter that places group A in column order
//            at [r * k, r * k + less) and the first `take` of group B behind it, by ballot ranks on top of the scanned bases.
//
// No atomic decides a position and no kernel waits on another workgroup: a staged row is a function of the input alone.  Equal
// keys land in ONE group in column order (section 10g), so the stable finish reproduces the definition.
//
// gs_topk_rows_anyk_u16 (section 10q) is the same host code and the same kernels at TrKey16: path 2 runs two counting rounds on
// image bits 15-8 and 7-0 with 256 bins (TaWidth / TaRound below), and the finish is gs_segmented_sort_narrow on bits 0 .. 16.
constexpr uint32_t TA_TILE = TR_CH;
constexpr uint32_t TA_SLAB_TILES = 4;      // tiles one count workgroup histograms before it adds its bins (1, 4 and 16 measured: section 10p)
constexpr uint32_t TA_LDS_WORDS = 2048;    // the count kernel's LDS histogram at either width
constexpr uint32_t TA_STATE_WORDS = 8;     // per row: k-th image (the prefix so far), less, take (krem), 0, matched after round 0, after round 1, 0, 0

// What the image width changes in the counting rounds of path 2 (gs_topk_rows_anyk_u16, section 10q, is the 16-bit one).
// ROUNDS: how many; BINS: the words of a row's histogram in memory (the widest round's bins); COPIES: the LDS histogram of a count
// workgroup holds that many interleaved copies of every bin, TA_LDS_WORDS words in all, and a lane adds to copy lane % COPIES.
//   32 bits   three rounds on image bits 31-21, 20-10 and 9-0: 2048, 2048 and 1024 bins, one copy.
//   16 bits   two rounds on image bits 15-8 and 7-0: 256 bins, eight copies.  The top byte of a half or bfloat16 score is its sign
//             and most of its exponent: a wave's 64 images fall into a handful of bins, and same-address lanes of an LDS atomic
//             serialise (see hist_add).  Eight copies cut such a run of lanes by eight in the LDS the 32-bit rounds use anyway.
template <int BITS> struct TaWidth;
template <> struct TaWidth<32> { static constexpr int ROUNDS = 3; static constexpr uint32_t BINS = 2048u, COPIES = 1u; };
template <> struct TaWidth<16> { static constexpr int ROUNDS = 2; static constexpr uint32_t BINS = 256u, COPIES = 8u; };
template <> struct TaWidth<64> { static constexpr int ROUNDS = 6; static constexpr uint32_t BINS = 2048u, COPIES = 1u; };   // (a descent of its own: see "any k, 64-bit keys")
static_assert(TaWidth<32>::BINS * TaWidth<32>::COPIES == TA_LDS_WORDS && TaWidth<16>::BINS * TaWidth<16>::COPIES == TA_LDS_WORDS, "one LDS budget");

template <int BITS, int ROUND> struct TaRound;
template <int ROUND> struct TaRound<32, ROUND> {
    static constexpr uint32_t SHIFT = ROUND == 0 ? 21u : ROUND == 1 ? 10u : 0u;
    static constexpr uint32_t BINS = ROUND == 2 ? 1024u : 2048u;
    static constexpr uint32_t MASK = ROUND == 0 ? 0u : ROUND == 1 ? 0xffe00000u : 0xfffffc00u;   // the digits above this one
};
template <int ROUND> struct TaRound<16, ROUND> {
    static_assert(ROUND < 2, "two rounds");
    static constexpr uint32_t SHIFT = ROUND == 0 ? 8u : 0u;
    static constexpr uint32_t BINS = 256u;
    static constexpr uint32_t MASK = ROUND == 0 ? 0u : 0xff00u;   // (a 16-bit image has zeros above bit 15)
};

// hist_add into copy lane % COPIES of bin d.  One copy: hist_add itself.  A wave of one digit still adds once.
template <uint32_t COPIES>
__device__ __forceinline__ void ta_hist_add(uint32_t *hist, uint32_t d, uint32_t lane)
{
    if (COPIES == 1u) { hist_add(hist, d); return; }
    const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__builtin_amdgcn_ballot_w64(d == d0) == act) {
        if (count_lower_mask(act) == 0) atomicAdd(&hist[d0 * COPIES], (uint32_t)__popcll(act));
    } else {
        atomicAdd(&hist[d * COPIES + (lane & (COPIES - 1u))], 1u);
    }
}

// The row record by image width: its words, the word that holds `less`, and the k-th image from it.  Eight words with the image
// in word 0 at 16 and 32 bits; sixteen with the image in words 0 (low) and 1 (high) at 64 (see "any k, 64-bit keys" below).
template <typename KT> struct TaRec {
    static constexpr uint32_t WORDS = TA_STATE_WORDS, LESS = 1;
    static __device__ __forceinline__ uint32_t kth(const uint32_t *__restrict__ rec) { return rec[0]; }
};
template <> struct TaRec<TrKey64> {
    static constexpr uint32_t WORDS = 16, LESS = 2;
    static __device__ __forceinline__ uint64_t kth(const uint32_t *__restrict__ rec) { return ((uint64_t)rec[1] << 32) | rec[0]; }
};

// One workgroup: a tile of up to CH elements of a row into registers as images, in the (wave, row, lane) order of the block kernel.
template <typename KT>
__device__ __forceinline__ void ta_load_tile(const typename KT::T *__restrict__ src, uint32_t first, uint32_t len, int flt,
                                             typename KT::I x, typename KT::I (&img)[TR_KPT])
{
    using I = typename KT::I;
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        img[u] = j < len ? (I)__builtin_nontemporal_load(src + j) : (I)0u;
    }
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) img[u] = KT::in(img[u], flt, x);
}

// tr_compact_with for a destination in global memory that is shared by the tiles of a row: group A from baseA, group B from
// baseB (both include what the tiles before this one place; baseB starts at `less`), B cut at kk.  Stores the caller's bit
// pattern, and with HV the column col0 + j.  Ends with a workgroup barrier.
template <typename KT, bool HV>
__device__ __forceinline__ void ta_place(typename KT::I (&img)[TR_KPT], uint32_t first, uint32_t len, uint32_t kk, typename KT::I kth,
                                         uint32_t less, uint32_t baseA, uint32_t baseB, uint32_t w, uint32_t lane,
                                         uint32_t (&wcnt)[2][TR_WAVES], typename KT::T *__restrict__ dst_k, uint32_t *__restrict__ dst_c,
                                         uint32_t col0, int flt, typename KT::I x)
{
    using T = typename KT::T;
    uint32_t nA = 0, nB = 0, lenc = len;
    asm volatile("" : "+v"(lenc));   // (range compares again, as in tr_compact_with)
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < lenc && img[u] < kth));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < lenc && img[u] == kth));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    for (uint32_t q = 0; q < w; ++q) { baseA += wcnt[0][q]; baseB += wcnt[1][q]; }
    if (baseA < less || baseB < kk) {   // wave-uniform: this wave still has something to place
        asm volatile("" : "+v"(lenc));
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            asm volatile("" : "+v"(img[u]));
            const bool a = j < lenc && img[u] < kth, b = j < lenc && img[u] == kth;
            const unsigned long long mA = __builtin_amdgcn_ballot_w64(a), mB = __builtin_amdgcn_ballot_w64(b);
            const uint32_t pos = a ? baseA + count_lower(mA) : baseB + count_lower(mB);
            if ((a || b) && pos < kk) {   // (group A never passes `less`; group B is cut at kk = less + take)
                dst_k[pos] = (T)KT::out(img[u], flt, x);
                if (HV) dst_c[pos] = col0 + j;
            }
            baseA += (uint32_t)__popcll(mA);
            baseB += (uint32_t)__popcll(mB);
        }
    }
    __syncthreads();
}

// offsets[i] = i * k for i in [0, rows]: the regular segments of the finish.
__global__ __launch_bounds__(256) void topk_anyk_offsets_kernel(int32_t *__restrict__ offsets, uint32_t rows, uint32_t k)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i <= rows) offsets[i] = (int32_t)(i * k);
}

// Path 1: one workgroup per row of up to CH columns.
template <typename KT, bool HV>
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_block_kernel(const typename KT::T *__restrict__ keys, uint32_t stride, uint32_t cols,
                                                                     uint32_t k, typename KT::T *__restrict__ dst_k,
                                                                     uint32_t *__restrict__ dst_c, uint32_t *__restrict__ state, int flt,
                                                                     uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    I img[TR_KPT];
    ta_load_tile<KT>(keys + (size_t)r * stride, first, cols, flt, x, img);
    uint32_t less;
    const I kth = tr_select<KT::BITS>(img, first, cols, k, tid, h, scratch, sel, less);
    const size_t out0 = (size_t)r * k;
    ta_place<KT, HV>(img, first, cols, k, kth, less, 0u, less, w, lane, wcnt, dst_k + out0, HV ? dst_c + out0 : nullptr, 0u, flt, x);
    if constexpr (KT::BITS == 64) {   // the sixteen-word record of gs_topk_rows_anyk_u64: both halves of the image, mode 0
        if (tid < TaRec<KT>::WORDS)
            state[(size_t)r * TaRec<KT>::WORDS + tid] =
                tid == 0 ? (uint32_t)kth : tid == 1 ? (uint32_t)(kth >> 32) : tid == TaRec<KT>::LESS ? less : tid == 3 ? k - less : 0u;
    } else {
        if (tid < TA_STATE_WORDS) state[(size_t)r * TA_STATE_WORDS + tid] = tid == 0 ? (uint32_t)kth : tid == 1 ? less : tid == 2 ? k - less : 0u;
    }
}

// Path 2, a counting round: one workgroup per (row, slab of slab_tiles tiles).
template <typename KT, int ROUND>
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_count_kernel(const typename KT::T *__restrict__ keys, uint32_t stride, uint32_t cols,
                                                                     uint32_t tiles, uint32_t slabs, uint32_t slab_tiles,
                                                                     const uint32_t *__restrict__ state, uint32_t *__restrict__ hist, int flt,
                                                                     uint32_t x32)
{
    using I = typename KT::I;
    using W = TaWidth<KT::BITS>;
    using R = TaRound<KT::BITS, ROUND>;
    const I x = KT::xmask(x32);
    __shared__ uint32_t h[TA_LDS_WORDS];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / slabs, sl = blockIdx.x - r * slabs;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    for (uint32_t i = tid; i < R::BINS * W::COPIES; i += TR_THREADS) h[i] = 0;
    const uint32_t prefix = ROUND == 0 ? 0u : state[(size_t)r * TA_STATE_WORDS];
    __syncthreads();
    const uint32_t t0 = sl * slab_tiles, t1 = t0 + slab_tiles < tiles ? t0 + slab_tiles : tiles;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t lo = t * TA_TILE, len = cols - lo < TA_TILE ? cols - lo : TA_TILE;
        I img[TR_KPT];
        ta_load_tile<KT>(keys + (size_t)r * stride + lo, first, len, flt, x, img);
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            if (j < len && (((uint32_t)img[u] ^ prefix) & R::MASK) == 0u)
                ta_hist_add<W::COPIES>(h, ((uint32_t)img[u] >> R::SHIFT) & (R::BINS - 1u), lane);
        }
    }
    __syncthreads();
    uint32_t *__restrict__ g = hist + (size_t)r * W::BINS;
    for (uint32_t i = tid; i < R::BINS; i += TR_THREADS) {   // a wave over contiguous bins; only what this slab holds
        uint32_t c = h[i * W::COPIES];
#pragma unroll
        for (uint32_t q = 1; q < W::COPIES; ++q) c += h[i * W::COPIES + q];
        if (c) atomicAdd(g + i, c);
    }
}

// Path 2, a pick: one workgroup of 256 per row scans the round's bins, picks the one that holds the krem-th element, updates the
// row's record and clears the histogram for the next round (and the next call).
template <int BITS, int ROUND>
__global__ __launch_bounds__(256) void topk_anyk_pick_kernel(uint32_t *__restrict__ state, uint32_t *__restrict__ hist, uint32_t k)
{
    using W = TaWidth<BITS>;
    using R = TaRound<BITS, ROUND>;
    constexpr uint32_t PER = R::BINS / 256u;
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    uint32_t *__restrict__ h = hist + (size_t)blockIdx.x * W::BINS + tid * PER;
    uint32_t *__restrict__ st = state + (size_t)blockIdx.x * TA_STATE_WORDS;
    const uint32_t prefix = ROUND == 0 ? 0u : st[0], less = ROUND == 0 ? 0u : st[1], krem = ROUND == 0 ? k : st[2];
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) { c[i] = h[i]; sum += c[i]; }
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) h[i] = 0;
    uint32_t ex = block_exclusive_scan_256(sum, scratch, nullptr);   // (its barriers: every thread has read the record before one writes it)
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        if (ex < krem && krem - ex <= c[i]) {   // one bin of the row: the counts of the bins sum to at least krem
            st[0] = prefix | ((tid * PER + i) << R::SHIFT);
            st[1] = less + ex;
            st[2] = krem - ex;
            if (ROUND + 1 < W::ROUNDS) st[4 + ROUND] = c[i];
        }
        ex += c[i];
    }
    if (ROUND == 0 && tid == 0) {   // (the words no pick writes: with two rounds word 5 as well)
        st[3] = 0; st[6] = 0; st[7] = 0;
        if (W::ROUNDS < 3) st[5] = 0;
    }
}

// Path 2, the select's counts: per (row, tile) the elements before the k-th image and those equal to it.
template <typename KT>
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_tilecount_kernel(const typename KT::T *__restrict__ keys, uint32_t stride,
                                                                         uint32_t cols, uint32_t tiles, const uint32_t *__restrict__ state,
                                                                         uint2 *__restrict__ counts, int flt, uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / tiles, t = blockIdx.x - r * tiles;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t lo = t * TA_TILE, len = cols - lo < TA_TILE ? cols - lo : TA_TILE;
    const I kth = TaRec<KT>::kth(state + (size_t)r * TaRec<KT>::WORDS);
    I img[TR_KPT];
    ta_load_tile<KT>(keys + (size_t)r * stride + lo, first, len, flt, x, img);
    uint32_t nA = 0, nB = 0;
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < len && img[u] < kth));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < len && img[u] == kth));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int q = 0; q < TR_WAVES; ++q) { a += wcnt[0][q]; b += wcnt[1][q]; }
        counts[blockIdx.x] = make_uint2(a, b);
    }
}

// Path 2, the select's scan: one workgroup of 256 per row turns its tiles' counts into bases, group A from 0, group B from less.
__global__ __launch_bounds__(256) void topk_anyk_scan_kernel(const uint32_t *__restrict__ state, uint2 *__restrict__ counts, uint32_t tiles)
{
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    uint2 *__restrict__ c = counts + (size_t)blockIdx.x * tiles;
    uint32_t carryA = 0, carryB = state[(size_t)blockIdx.x * TA_STATE_WORDS + 1];
    for (uint32_t base = 0; base < tiles; base += 256u) {
        const uint32_t i = base + tid;
        const uint2 v = i < tiles ? c[i] : make_uint2(0u, 0u);
        uint32_t totA, totB;
        const uint32_t exA = block_exclusive_scan_256(v.x, scratch, &totA);
        const uint32_t exB = block_exclusive_scan_256(v.y, scratch, &totB);
        if (i < tiles) c[i] = make_uint2(carryA + exA, carryB + exB);
        carryA += totA; carryB += totB;
    }
}
// The same scan over the sixteen-word records of the 64-bit call (a kernel of its own: the one above keeps its code).
__global__ __launch_bounds__(256) void topk_anyk_wide_scan_kernel(const uint32_t *__restrict__ state, uint2 *__restrict__ counts, uint32_t tiles)
{
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    uint2 *__restrict__ c = counts + (size_t)blockIdx.x * tiles;
    uint32_t carryA = 0, carryB = state[(size_t)blockIdx.x * TaRec<TrKey64>::WORDS + TaRec<TrKey64>::LESS];
    for (uint32_t base = 0; base < tiles; base += 256u) {
        const uint32_t i = base + tid;
        const uint2 v = i < tiles ? c[i] : make_uint2(0u, 0u);
        uint32_t totA, totB;
        const uint32_t exA = block_exclusive_scan_256(v.x, scratch, &totA);
        const uint32_t exB = block_exclusive_scan_256(v.y, scratch, &totB);
        if (i < tiles) c[i] = make_uint2(carryA + exA, carryB + exB);
        carryA += totA; carryB += totB;
    }
}

// Path 2, the select's scatter: one workgroup per (row, tile) places its part of the two groups.
template <typename KT, bool HV>
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_scatter_kernel(const typename KT::T *__restrict__ keys, uint32_t stride, uint32_t cols,
                                                                       uint32_t tiles, uint32_t k, const uint32_t *__restrict__ state,
                                                                       const uint2 *__restrict__ counts, typename KT::T *__restrict__ dst_k,
                                                                       uint32_t *__restrict__ dst_c, int flt, uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / tiles, t = blockIdx.x - r * tiles;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t lo = t * TA_TILE, len = cols - lo < TA_TILE ? cols - lo : TA_TILE;
    const I kth = TaRec<KT>::kth(state + (size_t)r * TaRec<KT>::WORDS);
    const uint32_t less = state[(size_t)r * TaRec<KT>::WORDS + TaRec<KT>::LESS];
    const uint2 base = counts[blockIdx.x];
    if (base.x >= less && base.y >= k) return;   // workgroup-uniform: both groups are full before this tile
    I img[TR_KPT];
    ta_load_tile<KT>(keys + (size_t)r * stride + lo, first, len, flt, x, img);
    const size_t out0 = (size_t)r * k;
    ta_place<KT, HV>(img, first, len, k, kth, less, base.x, base.y, w, lane, wcnt, dst_k + out0, HV ? dst_c + out0 : nullptr, lo, flt, x);
}

// The pairs form's last step: vals_out[r * k + i] = vals_in[r * stride + column].
__global__ __launch_bounds__(256) void topk_anyk_gather_kernel(const uint32_t *__restrict__ vals_in, const uint32_t *__restrict__ col,
                                                               uint32_t *__restrict__ vals_out, uint32_t total, uint32_t k, uint32_t stride,
                                                               uint32_t cols)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t r = i / k, c = col[i];
        vals_out[i] = vals_in[(size_t)r * stride + (c < cols ? c : cols - 1u)];
    }
}

// ------------------------------------------------------ any k, 64-bit keys --
// gs_topk_rows_anyk_u64.  Path 1 is topk_anyk_block_kernel at TrKey64.  Path 2 is a descent of its own:
// counting rounds on 11-bit digits that go straight to the bits that can differ, and that stop reading the matrix for a row as
// soon as the bucket of its k-th element fits the row's list.  Every launch of the worst case (six rounds) is always enqueued; a
// workgroup whose row is decided reads the row's record and returns.
//
//   a round at shift s (53 first)   a count workgroup per (row, slab) histograms (image >> s) & 2047 in LDS over the elements whose
//            image matches the row's prefix on the bits at and above s + 11, and reduces the OR of those images and the OR of their
//            complements (AND = ~that; a zeroed word is neutral for both): per wave, then in LDS, then one pair of 64-bit atomic ORs
//            per workgroup into the record.  The adds and ORs are commutative: their results do not depend on their order.
//   a pick   one workgroup per row takes the bin d of the krem-th element, puts d into prefix bits [s, s + 11), updates less and
//            krem, and with c the bin's count and v = (AND ^ OR) below s -- AND and OR are those of the round's matched set, a
//            superset of the bucket -- decides:  s == 0 or v == 0: every element of the bucket equals prefix | (AND below s), the
//            row is decided (mode 2, a tie run cut at krem);  else c <= L: the bucket goes to the row's list (mode 1);  else, with
//            hb the highest set bit of v, bits (hb, s) are constant over the matched set and come from the AND, and the next round
//            runs at max(hb - 10, 0).  The shifts fall by at least 11 until they reach 0: 53, <= 42, <= 31, <= 20, <= 9, 0.
//   collect  one workgroup per (row, tile), rows in mode 1: appends the images that match the prefix at and above s to the row's
//            list.  A workgroup claims its range from the row's cursor with one atomic add.  That atomic decides positions IN THE
//            LIST only; the list is read as a multiset (an image and two counts come out of it) and never reaches an output position.
//   list select   one workgroup per row in mode 1 loads the <= L images as path 1 loads a row and runs tr_select with k = krem.
//   then the tile counts, the per-row scan and the scatter of the 32-bit call, at TrKey64.
//
// The record, sixteen words per row: k-th image (the prefix so far) low, high; less; krem / take; mode (0 descending or path 1,
// 1 list, 2 tie run); D, the rounds taken; the shift of the next round (of the last one once decided); the list's cursor; the
// OR word low, high; the OR-of-complements word low, high; c of the last pick; three zero words.
constexpr uint32_t TA64_TAKE = 3, TA64_MODE = 4, TA64_D = 5, TA64_SHIFT = 6, TA64_LIST = 7, TA64_OR = 8, TA64_ORN = 10, TA64_C = 12;
constexpr uint32_t TA64_DIGIT = 11, TA64_BINS = 2048, TA64_SHIFT0 = 53, TA64_ROUNDS = 6;
static_assert(TA64_BINS == TA_LDS_WORDS && (1u << TA64_DIGIT) == TA64_BINS && TA64_SHIFT0 + TA64_DIGIT == 64, "one LDS budget, whole image");

__global__ __launch_bounds__(TR_THREADS) void topk_anyk_wide_count_kernel(const uint64_t *__restrict__ keys, uint32_t stride, uint32_t cols,
                                                                          uint32_t tiles, uint32_t slabs, uint32_t slab_tiles,
                                                                          uint32_t *__restrict__ state, uint32_t *__restrict__ hist, int flt,
                                                                          uint32_t x32, int first_round)
{
    using KT = TrKey64;
    const uint64_t x = KT::xmask(x32);
    __shared__ uint32_t h[TA_LDS_WORDS];
    __shared__ unsigned long long red[2];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / slabs, sl = blockIdx.x - r * slabs;
    uint32_t *__restrict__ rec = state + (size_t)r * TaRec<KT>::WORDS;
    uint32_t shift = TA64_SHIFT0;
    uint64_t prefix = 0;
    if (!first_round) {
        if (rec[TA64_MODE] != 0u) return;   // workgroup-uniform: the row is decided
        shift = (uint32_t)__builtin_amdgcn_readfirstlane(rec[TA64_SHIFT]);
        prefix = uniform64(rec[0], rec[1]);
    }
    const uint64_t mask = shift >= TA64_SHIFT0 ? 0ull : ~0ull << (shift + TA64_DIGIT);   // the bits above this digit
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    for (uint32_t i = tid; i < TA64_BINS; i += TR_THREADS) h[i] = 0;
    if (tid < 2u) red[tid] = 0ull;
    __syncthreads();
    uint64_t all_or = 0ull, all_orn = 0ull;
    const uint32_t t0 = sl * slab_tiles, t1 = t0 + slab_tiles < tiles ? t0 + slab_tiles : tiles;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t lo = t * TA_TILE, len = cols - lo < TA_TILE ? cols - lo : TA_TILE;
        uint64_t img[TR_KPT];
        ta_load_tile<KT>(keys + (size_t)r * stride + lo, first, len, flt, x, img);
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            if (j < len && ((img[u] ^ prefix) & mask) == 0ull) {
                hist_add(h, (uint32_t)(img[u] >> shift) & (TA64_BINS - 1u));
                all_or |= img[u];
                all_orn |= ~img[u];
            }
        }
    }
    {   // OR over the wave, then one LDS atomic pair per wave that matched something
        uint32_t ol = (uint32_t)all_or, oh = (uint32_t)(all_or >> 32), nl = (uint32_t)all_orn, nh = (uint32_t)(all_orn >> 32);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            ol |= __shfl_xor(ol, d, WAVE); oh |= __shfl_xor(oh, d, WAVE);
            nl |= __shfl_xor(nl, d, WAVE); nh |= __shfl_xor(nh, d, WAVE);
        }
        if (lane == 0u && (ol | oh | nl | nh) != 0u) {
            atomicOr(&red[0], ((unsigned long long)oh << 32) | ol);
            atomicOr(&red[1], ((unsigned long long)nh << 32) | nl);
        }
    }
    __syncthreads();
    uint32_t *__restrict__ g = hist + (size_t)r * TA64_BINS;
    for (uint32_t i = tid; i < TA64_BINS; i += TR_THREADS) {   // a wave over contiguous bins; only what this slab holds
        const uint32_t c = h[i];
        if (c) atomicAdd(g + i, c);
    }
    if (tid == 0u && (red[0] | red[1]) != 0ull) {   // (the record is 64 bytes at a 256-byte base: the words are 8-byte aligned)
        atomicOr(reinterpret_cast<unsigned long long *>(rec + TA64_OR), red[0]);
        atomicOr(reinterpret_cast<unsigned long long *>(rec + TA64_ORN), red[1]);
    }
}

// A pick of the 64-bit descent: see the rule above.  Clears the bins and the reduction words for the next round and the next call.
__global__ __launch_bounds__(256) void topk_anyk_wide_pick_kernel(uint32_t *__restrict__ state, uint32_t *__restrict__ hist, uint32_t k,
                                                                  uint32_t list_cap, int first_round)
{
    constexpr uint32_t PER = TA64_BINS / 256u;
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    uint32_t *__restrict__ h = hist + (size_t)blockIdx.x * TA64_BINS + tid * PER;
    uint32_t *__restrict__ st = state + (size_t)blockIdx.x * TaRec<TrKey64>::WORDS;
    if (!first_round && st[TA64_MODE] != 0u) return;   // workgroup-uniform: decided, and its bins are clear
    const uint32_t shift = first_round ? TA64_SHIFT0 : st[TA64_SHIFT];
    const uint64_t prefix = first_round ? 0ull : ((uint64_t)st[1] << 32) | st[0];
    const uint32_t less = first_round ? 0u : st[TaRec<TrKey64>::LESS], krem = first_round ? k : st[TA64_TAKE];
    const uint32_t rounds = first_round ? 0u : st[TA64_D];
    const uint64_t all_or = ((uint64_t)st[TA64_OR + 1] << 32) | st[TA64_OR];
    const uint64_t all_and = ~(((uint64_t)st[TA64_ORN + 1] << 32) | st[TA64_ORN]);
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) { c[i] = h[i]; sum += c[i]; }
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) h[i] = 0;
    uint32_t ex = block_exclusive_scan_256(sum, scratch, nullptr);   // (its barriers: every thread has read the record before one writes it)
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        if (ex < krem && krem - ex <= c[i]) {   // one bin of the row: the counts of the bins sum to at least krem
            const uint64_t low = shift ? (1ull << shift) - 1ull : 0ull;
            const uint64_t v = (all_and ^ all_or) & low;
            uint64_t p = prefix | ((uint64_t)(tid * PER + i) << shift);
            uint32_t mode = 0u, next = shift;
            if (shift == 0u || v == 0ull) {
                p |= all_and & low;
                mode = 2u;
            } else if (c[i] <= list_cap) {
                mode = 1u;
            } else {
                const uint32_t hb = 63u - (uint32_t)__builtin_clzll(v);   // hb < shift
                p |= all_and & low & ~((2ull << hb) - 1ull);              // bits (hb, shift): the same in every matched image
                next = hb >= TA64_DIGIT - 1u ? hb - (TA64_DIGIT - 1u) : 0u;
            }
            st[0] = (uint32_t)p; st[1] = (uint32_t)(p >> 32);
            st[TaRec<TrKey64>::LESS] = less + ex;
            st[TA64_TAKE] = krem - ex;
            st[TA64_MODE] = mode;
            st[TA64_D] = rounds + 1u;
            st[TA64_SHIFT] = next;
            st[TA64_LIST] = 0u;
            st[TA64_OR] = 0u; st[TA64_OR + 1] = 0u; st[TA64_ORN] = 0u; st[TA64_ORN + 1] = 0u;
            st[TA64_C] = c[i];
            st[13] = 0u; st[14] = 0u; st[15] = 0u;
        }
        ex += c[i];
    }
}

// Collect: one workgroup per (row, tile) of a row in mode 1 appends its images of the bucket to the row's list.
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_wide_collect_kernel(const uint64_t *__restrict__ keys, uint32_t stride, uint32_t cols,
                                                                            uint32_t tiles, uint32_t *__restrict__ state,
                                                                            uint64_t *__restrict__ lists, uint32_t list_cap, int flt,
                                                                            uint32_t x32)
{
    using KT = TrKey64;
    const uint64_t x = KT::xmask(x32);
    __shared__ uint32_t wcnt[TR_WAVES];
    __shared__ uint32_t claimed;
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t r = blockIdx.x / tiles, t = blockIdx.x - r * tiles;
    uint32_t *__restrict__ rec = state + (size_t)r * TaRec<KT>::WORDS;
    if (rec[TA64_MODE] != 1u) return;   // workgroup-uniform
    const uint32_t shift = (uint32_t)__builtin_amdgcn_readfirstlane(rec[TA64_SHIFT]);   // 1 .. 53 in mode 1
    const uint64_t prefix = uniform64(rec[0], rec[1]);
    const uint64_t mask = ~0ull << shift;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t lo = t * TA_TILE, len = cols - lo < TA_TILE ? cols - lo : TA_TILE;
    uint64_t img[TR_KPT];
    ta_load_tile<KT>(keys + (size_t)r * stride + lo, first, len, flt, x, img);
    uint32_t n = 0;
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        n += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < len && ((img[u] ^ prefix) & mask) == 0ull));
    }
    if (lane == 0u) wcnt[w] = n;
    __syncthreads();
    uint32_t base = 0, total = 0;
    for (uint32_t q = 0; q < (uint32_t)TR_WAVES; ++q) { if (q < w) base += wcnt[q]; total += wcnt[q]; }
    if (total == 0u) return;   // workgroup-uniform
    if (tid == 0u) claimed = atomicAdd(rec + TA64_LIST, total);
    __syncthreads();
    base += claimed;
    uint64_t *__restrict__ dst = lists + (size_t)r * list_cap;
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        const bool m = j < len && ((img[u] ^ prefix) & mask) == 0ull;
        const unsigned long long mm = __builtin_amdgcn_ballot_w64(m);
        const uint32_t pos = base + count_lower(mm);
        if (m && pos < list_cap) dst[pos] = img[u];   // (the bucket holds c <= list_cap elements: the bound never cuts)
        base += (uint32_t)__popcll(mm);
    }
}

// List select: one workgroup per row in mode 1 finds the krem-th image of the row's list.
__global__ __launch_bounds__(TR_THREADS) void topk_anyk_wide_listselect_kernel(uint32_t *__restrict__ state,
                                                                               const uint64_t *__restrict__ lists, uint32_t list_cap)
{
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    uint32_t *__restrict__ rec = state + (size_t)blockIdx.x * TaRec<TrKey64>::WORDS;
    if (rec[TA64_MODE] != 1u) return;   // workgroup-uniform
    const uint32_t c = rec[TA64_C], n = c < list_cap ? c : list_cap;
    const uint32_t less0 = rec[TaRec<TrKey64>::LESS], krem = rec[TA64_TAKE];
    const uint64_t *__restrict__ src = lists + (size_t)blockIdx.x * list_cap;
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    uint64_t img[TR_KPT];
#pragma unroll
    for (int u = 0; u < TR_KPT; ++u) {
        const uint32_t j = first + (uint32_t)u * WAVE;
        img[u] = j < n ? src[j] : 0ull;
    }
    uint32_t less;
    const uint64_t kth = tr_select<64>(img, first, n, krem, tid, h, scratch, sel, less);   // (its barriers: the record is read before it is written)
    if (tid == 0u) {
        rec[0] = (uint32_t)kth; rec[1] = (uint32_t)(kth >> 32);
        rec[TaRec<TrKey64>::LESS] = less0 + less;
        rec[TA64_TAKE] = krem - less;
    }
}

struct TaPlan { uint32_t path, launches, slab_tiles, slabs, tiles, list_cap; };

// L, the capacity of a row's list in the 64-bit descent: an eighth of the row, at least 1024, at most one tile.
static inline uint32_t ta_list_cap(uint64_t cols)
{
    const uint64_t e = cols / 8;
    return (uint32_t)(e < 1024 ? 1024 : e > TR_CH ? TR_CH : e);
}

static inline bool ta_shape_ok(uint64_t rows, uint64_t cols, uint64_t k)
{
    if (k > cols) return false;
    if (tr_mul_ge_2p32(rows, cols)) return false;
    if (rows != 0 && k > 0x7fffffffull / rows) return false;   // num_rows * k >= 2^31: the finish has int offsets
    return true;
}

template <typename KT>
static inline TaPlan ta_make_plan(uint64_t cols)
{
    TaPlan p{};
    if (cols <= TR_CH) { p.path = 1; p.launches = 2; p.slab_tiles = 1; p.slabs = 1; p.tiles = 1; return p; }
    p.path = 2;
    p.launches = 5u + 2u * (uint32_t)TaWidth<KT::BITS>::ROUNDS;   // zero, offsets, ROUNDS times (count, pick), tile counts, scan, scatter
    if (KT::BITS == 64) { p.launches += 2u; p.list_cap = ta_list_cap(cols); }   // collect and list select
    p.tiles = (uint32_t)((cols + TA_TILE - 1) / TA_TILE);
    p.slab_tiles = TA_SLAB_TILES;
    p.slabs = (p.tiles + p.slab_tiles - 1) / p.slab_tiles;
    return p;
}

// The finish by key width: the segmented sort of the staged pairs on the whole image, and its size query.
template <typename KT> struct TaFinish;
template <> struct TaFinish<TrKey32> {
    static size_t temp_bytes(uint64_t items, bool hv, uint64_t rows) { return gs_segmented_temp_bytes(items, hv ? 1 : 0, (uint32_t)rows); }
    static int sort(void *ws, size_t ws_bytes, uint32_t *dk[2], uint32_t *dv[2], int *selector, uint32_t items, uint32_t rows,
                    const int32_t *offsets, int descending, int key_type, hipStream_t s)
    {
        return gs_segmented_sort_u32(ws, ws_bytes, dk, dv, selector, items, rows, offsets, offsets + 1, 0, 32, descending, key_type, s);
    }
};
template <> struct TaFinish<TrKey16> {
    static size_t temp_bytes(uint64_t items, bool hv, uint64_t rows)
    {
        return gs_segmented_narrow_temp_bytes(items, GS_KEY_U16, hv ? 4 : 0, (uint32_t)rows);
    }
    static int sort(void *ws, size_t ws_bytes, uint16_t *dk[2], uint32_t *dv[2], int *selector, uint32_t items, uint32_t rows,
                    const int32_t *offsets, int descending, int key_type, hipStream_t s)
    {
        void *k2[2] = {dk[0], dk[1]}, *v2[2] = {dv ? dv[0] : nullptr, dv ? dv[1] : nullptr};
        return gs_segmented_sort_narrow(ws, ws_bytes, k2, dv ? v2 : nullptr, selector, items, rows, offsets, offsets + 1, key_type,
                                        dv ? 4 : 0, 0, 16, descending, s);
    }
};

template <> struct TaFinish<TrKey64> {
    static size_t temp_bytes(uint64_t items, bool hv, uint64_t rows) { return gs_segmented_wide_temp_bytes(items, 8, hv ? 4 : 0, (uint32_t)rows); }
    static int sort(void *ws, size_t ws_bytes, uint64_t *dk[2], uint32_t *dv[2], int *selector, uint32_t items, uint32_t rows,
                    const int32_t *offsets, int descending, int key_type, hipStream_t s)
    {
        void *k2[2] = {dk[0], dk[1]}, *v2[2] = {dv ? dv[0] : nullptr, dv ? dv[1] : nullptr};
        return gs_segmented_sort_wide(ws, ws_bytes, k2, dv ? v2 : nullptr, selector, items, rows, offsets, offsets + 1, 8, dv ? 4 : 0, 0, 64,
                                      descending, key_type, s);
    }
};

template <typename KT>
struct TaWs {
    uint32_t *state;
    int32_t *offsets;
    uint32_t *hist;
    uint2 *counts;
    uint64_t *lists;   // (64-bit keys, path 2)
    size_t zero_bytes; // from `state`: the records, the offsets and the histograms are one area
    typename KT::T *keys1;
    uint32_t *cols1, *cols0;
    char *seg;
    size_t seg_bytes;
};

// The header's workspace formula, term by term; returns the bytes carved (without the slack).
template <typename KT>
static size_t ta_carve(char *base, uint64_t rows, uint64_t cols, uint64_t k, bool hv, bool pairs, TaWs<KT> *ws)
{
    using T = typename KT::T;
    const TaPlan p = ta_make_plan<KT>(cols);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base + off; off += gs_ws_align(bytes); return q; };
    ws->state = (uint32_t *)take((size_t)4 * TaRec<KT>::WORDS * rows);
    ws->offsets = (int32_t *)take((size_t)4 * (rows + 1));
    ws->hist = nullptr; ws->counts = nullptr; ws->lists = nullptr; ws->zero_bytes = 0;
    if (p.path == 2) {
        ws->hist = (uint32_t *)take((size_t)4 * TaWidth<KT::BITS>::BINS * rows);
        ws->zero_bytes = off;
        ws->counts = (uint2 *)take((size_t)8 * rows * p.tiles);
        if (KT::BITS == 64) ws->lists = (uint64_t *)take((size_t)8 * p.list_cap * rows);
    }
    ws->keys1 = (T *)take(sizeof(T) * rows * k);
    ws->cols1 = hv ? (uint32_t *)take((size_t)4 * rows * k) : nullptr;
    ws->cols0 = pairs ? (uint32_t *)take((size_t)4 * rows * k) : nullptr;
    ws->seg_bytes = TaFinish<KT>::temp_bytes(rows * k, hv, rows);
    ws->seg = take(ws->seg_bytes);
    return off;
}

// (The size query has no pointers to tell pairs from arguments: with values it holds the first half of the columns too.)
template <typename KT>
static size_t ta_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    if (!ta_shape_ok(num_rows, num_cols, k)) return 0;
    if (num_rows == 0 || num_cols == 0 || k == 0) return 0;
    TaWs<KT> ws;
    return ta_carve<KT>(nullptr, num_rows, num_cols, k, has_values != 0, has_values != 0, &ws) + GS_WS_SLACK;
}

template <typename KT, int ROUND>
static void ta_launch_round(hipStream_t s, const TaPlan &p, const TaWs<KT> &ws, const typename KT::T *ki, uint32_t rows, uint32_t cols,
                            uint32_t stride, uint32_t k, int flt, uint32_t x)
{
    hipLaunchKernelGGL((topk_anyk_count_kernel<KT, ROUND>), dim3(rows * p.slabs), dim3(TR_THREADS), 0, s, ki, stride, cols, p.tiles, p.slabs,
                       p.slab_tiles, (const uint32_t *)ws.state, ws.hist, flt, x);
    hipLaunchKernelGGL((topk_anyk_pick_kernel<KT::BITS, ROUND>), dim3(rows), dim3(256), 0, s, ws.state, ws.hist, k);
}

template <typename KT, bool HV>
static void ta_launch_select(hipStream_t s, const TaPlan &p, const TaWs<KT> &ws, const typename KT::T *ki, typename KT::T *dk, uint32_t *dc,
                             uint32_t rows, uint32_t cols, uint32_t stride, uint32_t k, int flt, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    if (p.path == 1) {
        hipLaunchKernelGGL((topk_anyk_block_kernel<KT, HV>), dim3(rows), dim3(TR_THREADS), 0, s, ki, stride, cols, k, dk, dc, ws.state, flt, x);
        return;
    }
    const dim3 gtile(rows * p.tiles), grow(rows), wg(TR_THREADS);
    if constexpr (KT::BITS == 64) {   // the worst case of the descent, always: a decided row's workgroups return at once
        for (uint32_t round = 0; round < TA64_ROUNDS; ++round) {
            hipLaunchKernelGGL(topk_anyk_wide_count_kernel, dim3(rows * p.slabs), wg, 0, s, ki, stride, cols, p.tiles, p.slabs, p.slab_tiles,
                               ws.state, ws.hist, flt, x, round == 0 ? 1 : 0);
            hipLaunchKernelGGL(topk_anyk_wide_pick_kernel, grow, dim3(256), 0, s, ws.state, ws.hist, k, p.list_cap, round == 0 ? 1 : 0);
        }
        hipLaunchKernelGGL(topk_anyk_wide_collect_kernel, gtile, wg, 0, s, ki, stride, cols, p.tiles, ws.state, ws.lists, p.list_cap, flt, x);
        hipLaunchKernelGGL(topk_anyk_wide_listselect_kernel, grow, wg, 0, s, ws.state, (const uint64_t *)ws.lists, p.list_cap);
    } else {
        ta_launch_round<KT, 0>(s, p, ws, ki, rows, cols, stride, k, flt, x);
        ta_launch_round<KT, 1>(s, p, ws, ki, rows, cols, stride, k, flt, x);
        if constexpr (TaWidth<KT::BITS>::ROUNDS == 3) ta_launch_round<KT, 2>(s, p, ws, ki, rows, cols, stride, k, flt, x);
    }
    hipLaunchKernelGGL((topk_anyk_tilecount_kernel<KT>), gtile, wg, 0, s, ki, stride, cols, p.tiles, (const uint32_t *)ws.state, ws.counts, flt,
                       x);
    if constexpr (KT::BITS == 64) hipLaunchKernelGGL(topk_anyk_wide_scan_kernel, grow, dim3(256), 0, s, (const uint32_t *)ws.state, ws.counts, p.tiles);
    else hipLaunchKernelGGL(topk_anyk_scan_kernel, grow, dim3(256), 0, s, (const uint32_t *)ws.state, ws.counts, p.tiles);
    hipLaunchKernelGGL((topk_anyk_scatter_kernel<KT, HV>), gtile, wg, 0, s, ki, stride, cols, p.tiles, k, (const uint32_t *)ws.state,
                       (const uint2 *)ws.counts, dk, dc, flt, x);
}

template <typename KT>
static int ta_run(void *d_temp, size_t temp_bytes, const typename KT::T *d_keys_in, const uint32_t *d_vals_in, typename KT::T *d_keys_out,
                  uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending, int key_type,
                  void *stream)
{
    using T = typename KT::T;
    GS_CLEAR_STALE_ERROR();
    if (!ta_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (row_stride < num_cols || tr_mul_ge_2p32(num_rows, row_stride)) return hipErrorInvalidValue;
    if (!KT::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr, pairs = d_vals_in != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < ta_temp_bytes<KT>(num_rows, num_cols, k, hv)) return hipErrorInvalidValue;
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
    const uint32_t total = rows * kk;
    const int flt = KT::is_float(key_type);
    const uint32_t x = KT::xor_of(key_type, descending);
    const TaPlan p = ta_make_plan<KT>(num_cols);
    TaWs<KT> ws;
    ta_carve<KT>(gs_ws_base(d_temp), num_rows, num_cols, k, hv, pairs, &ws);

    if (p.path == 2) {   // the histograms start at zero; every pick leaves them so
        // (64-bit keys: the records, whose cursors and reduction words must start at zero, sit in one area with them)
        const hipError_t e = KT::BITS == 64 ? zero_async(ws.state, ws.zero_bytes, s)
                                            : zero_async(ws.hist, (size_t)4 * TaWidth<KT::BITS>::BINS * rows, s);
        if (e != hipSuccess) return (int)e;
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_anyk_offsets_kernel, dim3(rows / 256u + 1u), dim3(256), 0, s, ws.offsets, rows, kk);
    }
    // the select stages row r's k (key, column) pairs at [r * k, r * k + k): the keys in d_keys_out, the columns in d_vals_out
    // (arguments) or in the workspace (pairs)
    uint32_t *col0 = !hv ? nullptr : pairs ? ws.cols0 : d_vals_out;
    if (hv) ta_launch_select<KT, true>(s, p, ws, d_keys_in, d_keys_out, col0, rows, cols, stride, kk, flt, x);
    else ta_launch_select<KT, false>(s, p, ws, d_keys_in, d_keys_out, col0, rows, cols, stride, kk, flt, x);
    int err = (int)hipGetLastError();
    if (err) return err;

    // the finish: an even number of passes over the whole image (eight of 64 bits, four of 32, two of 16) leaves the result in half 0, where
    // the pairs were staged
    T *dk[2] = {d_keys_out, ws.keys1};
    uint32_t *dv[2] = {col0, ws.cols1};
    int selector = 0;
    err = TaFinish<KT>::sort(ws.seg, ws.seg_bytes, dk, hv ? dv : nullptr, &selector, total, rows, ws.offsets, descending, key_type, s);
    if (err) return err;
    if (selector != 0) return hipErrorUnknown;
    if (pairs) {
        KernelTimer kt(GS_K_OTHER, s);
        const uint32_t g = (total + 255u) / 256u;
        hipLaunchKernelGGL(topk_anyk_gather_kernel, dim3(g < 65536u ? g : 65536u), dim3(256), 0, s, d_vals_in, (const uint32_t *)ws.cols0,
                           d_vals_out, total, kk, stride, cols);
    }
    return (int)hipGetLastError();
}

template <typename KT>
static int ta_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, uint32_t out[8])
{
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!ta_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;   // such a call enqueues nothing
    const TaPlan p = ta_make_plan<KT>(num_cols);
    out[0] = p.path; out[1] = p.launches; out[2] = TR_CH; out[3] = TA_TILE; out[4] = p.slab_tiles; out[5] = p.slabs; out[6] = p.tiles;
    out[7] = p.list_cap;   // (0 at 16 and 32 bits and on path 1)
    return hipSuccess;
}

template <typename KT>
static int ta_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint64_t row, uint32_t out[8],
                     void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!ta_shape_ok(num_rows, num_cols, k)) return hipErrorInvalidValue;
    if (num_rows == 0 || num_cols == 0 || k == 0) return hipSuccess;   // such a call enqueued nothing
    if (!d_temp || row >= num_rows) return hipErrorInvalidValue;
    TaWs<KT> ws;
    ta_carve<KT>(gs_ws_base(d_temp), num_rows, num_cols, k, has_values != 0, false, &ws);   // (only the records, the first term, are read)
    uint32_t st[TaRec<KT>::WORDS];
    hipError_t e = hipMemcpyAsync(st, ws.state + row * TaRec<KT>::WORDS, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    out[0] = ta_make_plan<KT>(num_cols).path;
    if (KT::BITS == 64) {
        out[1] = st[0]; out[2] = st[1]; out[3] = st[TaRec<KT>::LESS]; out[4] = st[TA64_TAKE]; out[5] = st[TA64_D]; out[6] = st[TA64_MODE];
        out[7] = st[TA64_MODE] == 1u ? st[TA64_LIST] : 0u;
    } else {
        out[1] = st[0]; out[2] = st[1]; out[3] = st[2]; out[4] = st[4]; out[5] = st[5];
    }
    return hipSuccess;
}

// ----------------------------------------------------- any k, ragged segments --
// gs_topk_segmented_anyk_u32: the k best of every ragged segment with no cap on k.  The workspace begins
// with the TsWs layout, so topk_seg_classify_kernel sorts the segments into the same six lists, with the same Lmax / Tmax bounds
// and the same drop rule, and topk_seg_expand_kernel writes the (record, tile) tasks of the long ones.  Then, by length:
//
//   <= 1024   the four topk_seg_wave_kernel launches as they are: k is their output stride and min(k, len) their cut.  What they
//             write is final and sorted; these segments skip the finish.
//   <= CH     one workgroup per record of the block list: topk_anyk_block_kernel's body (tr_select, then ta_place at seg * k).
//   longer    path 2 of gs_topk_rows_anyk_u32 over all long segments at once, (row, tile) = blockIdx replaced by a lookup in the
//             task list: three counting rounds into 2048 bins per long record, a pick per record after each, two counts per task, a
//             scan per record and a scatter in position order.  A count workgroup takes the slab of TA_SLAB_TILES consecutive
//             tiles that starts at its task (a segment's tasks are consecutive slots); the others go on to their next slot.
//
// The selects stage the kept (key, position) pairs of a segment, unsorted but with equal keys in position order, at
// [seg * k, seg * k + kept), and write seg * k + kept into the end array of the finish: gs_segmented_sort_u32 over the
// num_segments * k slots with begin = seg * k.  The end array starts equal to the begin array, so an empty, a wave-class or a
// dropped segment is an empty range of the finish and none of its slots is touched.  Every record and task read from the
// workspace is clamped against the arguments before it becomes an address; no atomic decides an output position.
struct TsaWs {
    uint32_t *state;             // eight words per long record: k-th image (the prefix so far), less, take, 0, matched after round 0, 1, 0, 0
    uint32_t *hist;              // TaWidth<32>::BINS per long record
    uint2 *counts;               // per task slot
    int32_t *begin, *end;        // the finish's offsets
    uint32_t *keys1, *pos1, *pos0;
    char *seg;
    size_t seg_bytes;
};

__device__ __forceinline__ uint32_t tsa_task_count(const TsWs &ws)
{   // the cursor, not the count of completed claims: a dropped segment leaves a hole behind it
    const uint32_t c = ws.state[TS_TASK_CUR + 1] != 0u ? ws.tmax : ws.state[TS_TASK_CUR];
    return __builtin_amdgcn_readfirstlane(c > ws.tmax ? ws.tmax : c);
}
__device__ __forceinline__ uint32_t tsa_rec_count(const TsWs &ws)
{
    const uint32_t c = ws.state[TS_REC_CUR];
    return __builtin_amdgcn_readfirstlane(c > ws.lmax ? ws.lmax : c);
}

// a long record, clamped; false when nothing of it may be touched (an empty record is a dropped segment's)
__device__ __forceinline__ bool tsa_load_long(const TsWs &ws, uint32_t rec, uint32_t num_items, uint32_t &base, uint32_t &slen, uint32_t &seg,
                                              uint32_t &row, uint32_t &chunks)
{
    if (!ts_load_rec(ws.list[TS_LONG], rec, num_items, ws.nseg, num_items, base, slen, seg, row)) return false;
    chunks = (slen + TA_TILE - 1u) / TA_TILE;
    return !__builtin_amdgcn_readfirstlane(row >= ws.tmax || chunks > ws.tmax - row);
}

// task slot t: its record and tile, and the record's fields.  A slot whose claim was dropped was never written by the expand
// kernel: whatever it holds is not the task of this slot.  Everything returned is uniform.
__device__ __forceinline__ bool tsa_load_task(const TsWs &ws, uint32_t t, uint32_t nrec, uint32_t num_items, uint32_t &rec, uint32_t &c,
                                              uint32_t &base, uint32_t &slen, uint32_t &seg, uint32_t &chunks)
{
    const TsTask task = ws.tasks[t];
    rec = __builtin_amdgcn_readfirstlane(task.rec); c = __builtin_amdgcn_readfirstlane(task.chunk);
    if (__builtin_amdgcn_readfirstlane(rec >= nrec)) return false;
    uint32_t row;
    if (!tsa_load_long(ws, rec, num_items, base, slen, seg, row, chunks)) return false;
    return !__builtin_amdgcn_readfirstlane(c >= chunks || row + c != t);
}

// begin[s] = end[s] = s * k: every segment starts as an empty range of the finish.
__global__ __launch_bounds__(256) void topk_seganyk_offsets_kernel(int32_t *__restrict__ begin, int32_t *__restrict__ end, uint32_t nseg,
                                                                   uint32_t k)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nseg) { begin[i] = (int32_t)(i * k); end[i] = (int32_t)(i * k); }
}

// Segments of 1025 .. CH elements: one workgroup per record of the block list, topk_anyk_block_kernel's body.
template <typename KT, bool HV>
__global__ __launch_bounds__(TR_THREADS) void topk_seganyk_block_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                                        typename KT::T *__restrict__ dst_k, uint32_t *__restrict__ dst_c,
                                                                        int32_t *__restrict__ end, uint32_t num_items, uint32_t k, int flt,
                                                                        uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ __attribute__((aligned(16))) uint32_t h[RADIX];
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t sel[3];
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    uint32_t count = ws.state[TS_BLOCK];
    if (count > ws.nseg) count = ws.nseg;
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {   // (t and everything decided from it are uniform: the barriers are safe)
        uint32_t base, len, seg, row;
        if (!ts_load_rec(ws.list[TS_BLOCK], t, num_items, ws.nseg, TR_CH, base, len, seg, row)) continue;
        const uint32_t kept = k < len ? k : len;
        I img[TR_KPT];
        ta_load_tile<KT>(keys + base, first, len, flt, x, img);
        uint32_t less;
        const I kth = tr_select<KT::BITS>(img, first, len, kept, tid, h, scratch, sel, less);
        const size_t out0 = (size_t)seg * k;
        ta_place<KT, HV>(img, first, len, kept, kth, less, 0u, less, w, lane, wcnt, dst_k + out0, HV ? dst_c + out0 : nullptr, 0u, flt, x);
        if (tid == 0u) end[seg] = (int32_t)(seg * k + kept);
    }
}

// The histograms of the long records in use start at zero; every pick leaves them so for the next round.
__global__ __launch_bounds__(256) void topk_seganyk_clear_kernel(TsWs ws, uint32_t *__restrict__ hist)
{
    const uint32_t nrec = tsa_rec_count(ws);
    for (uint32_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        uint4 *__restrict__ h = reinterpret_cast<uint4 *>(hist + (size_t)r * TaWidth<32>::BINS);
        for (uint32_t i = threadIdx.x; i < TaWidth<32>::BINS / 4u; i += 256u) h[i] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// A counting round: the workgroup that meets the first task of a slab histograms the slab's tiles in LDS and adds its non-zero
// bins to the record's histogram (integer adds: the sums do not depend on their order).
template <typename KT, int ROUND>
__global__ __launch_bounds__(TR_THREADS) void topk_seganyk_count_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                                        const uint32_t *__restrict__ state, uint32_t *__restrict__ hist,
                                                                        uint32_t num_items, int flt, uint32_t x32)
{
    using I = typename KT::I;
    using R = TaRound<KT::BITS, ROUND>;
    const I x = KT::xmask(x32);
    __shared__ uint32_t h[TA_LDS_WORDS];
    const uint32_t tid = threadIdx.x, w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t count = tsa_task_count(ws), nrec = tsa_rec_count(ws);
    // Workgroup b starts at slot (b % q) * TA_SLAB_TILES + b / q, q a TA_SLAB_TILES-th of the grid (a multiple of it): where every
    // segment is a whole number of slabs, the slots that start a slab are those of the first q workgroups -- consecutive ones,
    // which the dispatcher spreads over all dies -- and not every TA_SLAB_TILES-th one.
    const uint32_t q = gridDim.x / TA_SLAB_TILES;
    for (uint32_t t = (blockIdx.x % q) * TA_SLAB_TILES + blockIdx.x / q; t < count; t += gridDim.x) {
        uint32_t rec, c, base, slen, seg, chunks;
        if (!tsa_load_task(ws, t, nrec, num_items, rec, c, base, slen, seg, chunks)) continue;
        if (c % TA_SLAB_TILES != 0u) continue;   // the slab belongs to the workgroup of its first task
        for (uint32_t i = tid; i < R::BINS; i += TR_THREADS) h[i] = 0;
        const uint32_t prefix = ROUND == 0 ? 0u : state[(size_t)rec * TA_STATE_WORDS];
        __syncthreads();
        const uint32_t c1 = c + TA_SLAB_TILES < chunks ? c + TA_SLAB_TILES : chunks;
        for (uint32_t tile = c; tile < c1; ++tile) {
            const uint32_t lo = tile * TA_TILE, len = slen - lo < TA_TILE ? slen - lo : TA_TILE;
            I img[TR_KPT];
            ta_load_tile<KT>(keys + (size_t)base + lo, first, len, flt, x, img);
#pragma unroll
            for (int u = 0; u < TR_KPT; ++u) {
                const uint32_t j = first + (uint32_t)u * WAVE;
                if (j < len && (((uint32_t)img[u] ^ prefix) & R::MASK) == 0u) hist_add(h, ((uint32_t)img[u] >> R::SHIFT) & (R::BINS - 1u));
            }
        }
        __syncthreads();
        uint32_t *__restrict__ g = hist + (size_t)rec * TaWidth<KT::BITS>::BINS;
        for (uint32_t i = tid; i < R::BINS; i += TR_THREADS) {   // a wave over contiguous bins; only what this slab holds
            const uint32_t v = h[i];
            if (v) atomicAdd(g + i, v);
        }
        __syncthreads();   // h is read before the next slab clears it
    }
}

// A pick: one workgroup of 256 per long record, topk_anyk_pick_kernel's body with krem = min(k, len) in the first round.
template <int BITS, int ROUND>
__global__ __launch_bounds__(256) void topk_seganyk_pick_kernel(TsWs ws, uint32_t *__restrict__ state, uint32_t *__restrict__ hist,
                                                                uint32_t num_items, uint32_t k)
{
    using W = TaWidth<BITS>;
    using R = TaRound<BITS, ROUND>;
    constexpr uint32_t PER = R::BINS / 256u;
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    const uint32_t nrec = tsa_rec_count(ws);
    for (uint32_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        uint32_t base, slen, seg, row, chunks;
        if (!tsa_load_long(ws, r, num_items, base, slen, seg, row, chunks)) continue;
        uint32_t *__restrict__ h = hist + (size_t)r * W::BINS + tid * PER;
        uint32_t *__restrict__ st = state + (size_t)r * TA_STATE_WORDS;
        const uint32_t prefix = ROUND == 0 ? 0u : st[0], less = ROUND == 0 ? 0u : st[1], krem = ROUND == 0 ? (k < slen ? k : slen) : st[2];
        uint32_t c[PER], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) { c[i] = h[i]; sum += c[i]; }
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) h[i] = 0;
        uint32_t ex = block_exclusive_scan_256(sum, scratch, nullptr);   // (its barriers: every thread has read the record before one writes it)
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            if (ex < krem && krem - ex <= c[i]) {   // one bin of the record: the counts of the bins sum to at least krem
                st[0] = prefix | ((tid * PER + i) << R::SHIFT);
                st[1] = less + ex;
                st[2] = krem - ex;
                if (ROUND + 1 < W::ROUNDS) st[4 + ROUND] = c[i];
            }
            ex += c[i];
        }
        if (ROUND == 0 && tid == 0) { st[3] = 0; st[6] = 0; st[7] = 0; }
    }
}

// The select's counts: per task the elements of its tile before the k-th image and those equal to it.
template <typename KT>
__global__ __launch_bounds__(TR_THREADS) void topk_seganyk_tilecount_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                                            const uint32_t *__restrict__ state, uint2 *__restrict__ counts,
                                                                            uint32_t num_items, int flt, uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t count = tsa_task_count(ws), nrec = tsa_rec_count(ws);
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {
        uint32_t rec, c, base, slen, seg, chunks;
        if (!tsa_load_task(ws, t, nrec, num_items, rec, c, base, slen, seg, chunks)) continue;
        const uint32_t lo = c * TA_TILE, len = slen - lo < TA_TILE ? slen - lo : TA_TILE;
        const I kth = state[(size_t)rec * TA_STATE_WORDS];
        I img[TR_KPT];
        ta_load_tile<KT>(keys + (size_t)base + lo, first, len, flt, x, img);
        uint32_t nA = 0, nB = 0;
#pragma unroll
        for (int u = 0; u < TR_KPT; ++u) {
            const uint32_t j = first + (uint32_t)u * WAVE;
            nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < len && img[u] < kth));
            nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(j < len && img[u] == kth));
        }
        if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t a = 0, b = 0;
            for (int q = 0; q < TR_WAVES; ++q) { a += wcnt[0][q]; b += wcnt[1][q]; }
            counts[t] = make_uint2(a, b);
        }
        __syncthreads();   // wcnt is read before the next task writes it
    }
}

// The select's scan: one workgroup of 256 per long record turns its tasks' counts into bases, group A from 0, group B from less,
// and writes the end of the segment's range of the finish -- here, for the records that found room, and nowhere else.
__global__ __launch_bounds__(256) void topk_seganyk_scan_kernel(TsWs ws, const uint32_t *__restrict__ state, uint2 *__restrict__ counts,
                                                                int32_t *__restrict__ end, uint32_t num_items, uint32_t k)
{
    __shared__ uint32_t scratch[8];
    const uint32_t tid = threadIdx.x;
    const uint32_t nrec = tsa_rec_count(ws);
    for (uint32_t r = blockIdx.x; r < nrec; r += gridDim.x) {
        uint32_t base0, slen, seg, row, tiles;
        if (!tsa_load_long(ws, r, num_items, base0, slen, seg, row, tiles)) continue;
        uint2 *__restrict__ c = counts + row;
        uint32_t carryA = 0, carryB = state[(size_t)r * TA_STATE_WORDS + 1];
        for (uint32_t base = 0; base < tiles; base += 256u) {
            const uint32_t i = base + tid;
            const uint2 v = i < tiles ? c[i] : make_uint2(0u, 0u);
            uint32_t totA, totB;
            const uint32_t exA = block_exclusive_scan_256(v.x, scratch, &totA);
            const uint32_t exB = block_exclusive_scan_256(v.y, scratch, &totB);
            if (i < tiles) c[i] = make_uint2(carryA + exA, carryB + exB);
            carryA += totA; carryB += totB;
        }
        if (tid == 0u) end[seg] = (int32_t)(seg * k + (k < slen ? k : slen));
    }
}

// The select's scatter: per task, its tile's part of the two groups, at the scanned bases.
template <typename KT, bool HV>
__global__ __launch_bounds__(TR_THREADS) void topk_seganyk_scatter_kernel(TsWs ws, const typename KT::T *__restrict__ keys,
                                                                          const uint32_t *__restrict__ state, const uint2 *__restrict__ counts,
                                                                          typename KT::T *__restrict__ dst_k, uint32_t *__restrict__ dst_c,
                                                                          uint32_t num_items, uint32_t k, int flt, uint32_t x32)
{
    using I = typename KT::I;
    const I x = KT::xmask(x32);
    __shared__ uint32_t wcnt[2][TR_WAVES];
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = w * (uint32_t)(WAVE * TR_KPT) + lane;
    const uint32_t count = tsa_task_count(ws), nrec = tsa_rec_count(ws);
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {
        uint32_t rec, c, base, slen, seg, chunks;
        if (!tsa_load_task(ws, t, nrec, num_items, rec, c, base, slen, seg, chunks)) continue;
        const uint32_t lo = c * TA_TILE, len = slen - lo < TA_TILE ? slen - lo : TA_TILE, kept = k < slen ? k : slen;
        const I kth = state[(size_t)rec * TA_STATE_WORDS];
        const uint32_t less = __builtin_amdgcn_readfirstlane(state[(size_t)rec * TA_STATE_WORDS + 1]);
        const uint2 at = counts[t];
        if (__builtin_amdgcn_readfirstlane(at.x >= less && at.y >= kept)) continue;   // both groups are full before this tile
        I img[TR_KPT];
        ta_load_tile<KT>(keys + (size_t)base + lo, first, len, flt, x, img);
        const size_t out0 = (size_t)seg * k;
        ta_place<KT, HV>(img, first, len, kept, kth, less, at.x, at.y, w, lane, wcnt, dst_k + out0, HV ? dst_c + out0 : nullptr, lo, flt, x);
    }
}

// The pairs form's last step, over the ranges of the finish only: vals_out[seg * k + i] = vals_in[b + position], b the
// segment's clamped begin.  (A wave-class segment's range is empty: its slots already hold values.)
__global__ __launch_bounds__(256) void topk_seganyk_gather_kernel(const uint32_t *__restrict__ vals_in, const uint32_t *__restrict__ pos,
                                                                  uint32_t *__restrict__ vals_out, const int32_t *__restrict__ end,
                                                                  const int *__restrict__ seg_begin, uint32_t nseg, uint32_t num_items,
                                                                  uint32_t k)
{
    for (uint32_t s = blockIdx.x; s < nseg; s += gridDim.x) {
        const uint32_t out0 = s * k, e = (uint32_t)end[s];
        if (e <= out0) continue;
        const uint32_t cnt = e - out0 < k ? e - out0 : k;
        int lo = seg_begin[s];
        if (lo < 0) lo = 0;
        if ((uint32_t)lo >= num_items) continue;
        const uint32_t last = num_items - 1u - (uint32_t)lo;
        for (uint32_t i = threadIdx.x; i < cnt; i += 256u) {
            const uint32_t p = pos[out0 + i];
            vals_out[out0 + i] = vals_in[(size_t)lo + (p < last ? p : last)];
        }
    }
}

// ---- host
static inline bool tsa_shape_ok(uint64_t num_items, uint64_t num_segments, uint64_t k)
{
    if (num_items >= (1ull << 31)) return false;
    if (num_segments != 0 && k > 0x7fffffffull / num_segments) return false;   // num_segments * k >= 2^31: the finish has int offsets
    return true;
}

// The header's workspace formula, term by term, behind the TsWs front (without candidate rows); returns the bytes carved.
static size_t tsa_carve(char *base, uint64_t num_items, uint64_t num_segments, uint64_t k, bool hv, bool pairs, TsWs *front, TsaWs *ws)
{
    size_t off = ts_carve(base, num_items, num_segments, 0, false, 4, front);
    const TsGeom g = ts_geom(num_items, num_segments);
    auto take = [&](size_t bytes) { char *q = (char *)((uintptr_t)base + off); off += gs_ws_align(bytes); return q; };
    ws->state = (uint32_t *)take((size_t)4 * TA_STATE_WORDS * g.lmax);
    ws->hist = (uint32_t *)take((size_t)4 * TaWidth<32>::BINS * g.lmax);
    ws->counts = (uint2 *)take((size_t)8 * g.tmax);
    ws->begin = (int32_t *)take((size_t)4 * num_segments);
    ws->end = (int32_t *)take((size_t)4 * num_segments);
    ws->keys1 = (uint32_t *)take((size_t)4 * num_segments * k);
    ws->pos1 = hv ? (uint32_t *)take((size_t)4 * num_segments * k) : nullptr;
    ws->pos0 = pairs ? (uint32_t *)take((size_t)4 * num_segments * k) : nullptr;
    ws->seg_bytes = gs_segmented_temp_bytes(num_segments * k, hv ? 1 : 0, (uint32_t)num_segments);
    ws->seg = take(ws->seg_bytes);
    return off;
}

// (The size query has no pointers to tell pairs from arguments: with values it holds the first half of the positions too.)
static size_t tsa_temp_bytes(uint64_t num_items, uint64_t num_segments, uint64_t k, int has_values)
{
    if (!tsa_shape_ok(num_items, num_segments, k)) return 0;
    if (num_items == 0 || num_segments == 0 || k == 0) return 0;
    TsWs front;
    TsaWs ws;
    return tsa_carve(nullptr, num_items, num_segments, k, has_values != 0, has_values != 0, &front, &ws) + GS_WS_SLACK;
}

// launches before the finish: zero, classify and four wave kernels; offsets and the block kernel; expand, clear, three times
// (count, pick), tile counts, scan and scatter
static inline uint32_t tsa_launches(uint32_t groups) { return 6u + ((groups & 2u) ? 2u : 0u) + ((groups & 4u) ? 11u : 0u); }

template <typename KT, int ROUND>
static void tsa_launch_round(hipStream_t s, const TsWs &front, const TsaWs &ws, uint32_t gt, uint32_t gl, const typename KT::T *ki, uint32_t n,
                             uint32_t k, int flt, uint32_t x)
{
    const uint32_t gc = (gt + TA_SLAB_TILES - 1u) / TA_SLAB_TILES * TA_SLAB_TILES;   // (a workgroup past the last slot returns at once)
    hipLaunchKernelGGL((topk_seganyk_count_kernel<KT, ROUND>), dim3(gc), dim3(TR_THREADS), 0, s, front, ki, (const uint32_t *)ws.state, ws.hist,
                       n, flt, x);
    hipLaunchKernelGGL((topk_seganyk_pick_kernel<KT::BITS, ROUND>), dim3(gl), dim3(256), 0, s, front, ws.state, ws.hist, n, k);
}

template <typename KT, bool HV>
static void tsa_launch_select(hipStream_t s, const TsWs &front, const TsaWs &ws, uint32_t groups, const typename KT::T *ki,
                              typename KT::T *dk, uint32_t *dc, uint32_t n, uint32_t k, int flt, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    const uint32_t gb = front.nseg < TS_MAX_GRID ? front.nseg : TS_MAX_GRID;
    hipLaunchKernelGGL(topk_seganyk_offsets_kernel, dim3((front.nseg + 255u) / 256u), dim3(256), 0, s, ws.begin, ws.end, front.nseg, k);
    hipLaunchKernelGGL((topk_seganyk_block_kernel<KT, HV>), dim3(gb), dim3(TR_THREADS), 0, s, front, ki, dk, dc, ws.end, n, k, flt, x);
    if (!(groups & 4u)) return;
    const uint32_t gl = front.lmax < TS_MAX_GRID ? front.lmax : TS_MAX_GRID, gt = front.tmax < TS_MAX_GRID ? front.tmax : TS_MAX_GRID;
    hipLaunchKernelGGL(topk_seg_expand_kernel, dim3(gl), dim3(256), 0, s, front, n);
    hipLaunchKernelGGL(topk_seganyk_clear_kernel, dim3(gl), dim3(256), 0, s, front, ws.hist);
    tsa_launch_round<KT, 0>(s, front, ws, gt, gl, ki, n, k, flt, x);
    tsa_launch_round<KT, 1>(s, front, ws, gt, gl, ki, n, k, flt, x);
    tsa_launch_round<KT, 2>(s, front, ws, gt, gl, ki, n, k, flt, x);
    hipLaunchKernelGGL((topk_seganyk_tilecount_kernel<KT>), dim3(gt), dim3(TR_THREADS), 0, s, front, ki, (const uint32_t *)ws.state, ws.counts, n,
                       flt, x);
    hipLaunchKernelGGL(topk_seganyk_scan_kernel, dim3(gl), dim3(256), 0, s, front, (const uint32_t *)ws.state, ws.counts, ws.end, n, k);
    hipLaunchKernelGGL((topk_seganyk_scatter_kernel<KT, HV>), dim3(gt), dim3(TR_THREADS), 0, s, front, ki, (const uint32_t *)ws.state,
                       (const uint2 *)ws.counts, dk, dc, n, k, flt, x);
}

static int tsa_run(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                   uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments, const int32_t *d_begin_offsets,
                   const int32_t *d_end_offsets, uint64_t k, int descending, int key_type, void *stream)
{
    using KT = TrKey32;
    GS_CLEAR_STALE_ERROR();
    if (!tsa_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (!KT::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr, pairs = d_vals_in != nullptr;
    if (!d_keys_in || !d_keys_out || !d_begin_offsets || !d_end_offsets) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < tsa_temp_bytes(num_items, num_segments, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out | (uintptr_t)d_vals_in | (uintptr_t)d_vals_out | (uintptr_t)d_counts_out |
          (uintptr_t)d_begin_offsets | (uintptr_t)d_end_offsets) & 3u) != 0)
        return hipErrorInvalidValue;
    {   // no array may share a byte with another, except that the two offset arrays (both only read) may: begin + 1 == end is usual
        const size_t out_elems = (size_t)num_segments * k;
        const void *arr[7] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, d_begin_offsets, d_end_offsets};
        const size_t bytes[7] = {4 * num_items, 4 * num_items, 4 * out_elems, 4 * out_elems, (size_t)4 * num_segments, (size_t)4 * num_segments,
                                 (size_t)4 * num_segments};
        for (int i = 0; i < 7; ++i)
            for (int j = i + 1; j < 7; ++j)
                if (!(i == 5 && j == 6) && gs_ranges_overlap(arr[i], bytes[i], arr[j], bytes[j])) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_items, kk = (uint32_t)k;
    const int flt = KT::is_float(key_type);
    const uint32_t x = KT::xor_of(key_type, descending);
    TsWs front;
    TsaWs ws;
    tsa_carve(gs_ws_base(d_temp), num_items, num_segments, k, hv, pairs, &front, &ws);
    const uint32_t groups = ts_groups(num_items);

    hipError_t e = zero_async(front.state, TS_STATE_BYTES, s);
    if (e != hipSuccess) return (int)e;
    { KernelTimer kt(GS_K_OTHER, s);
      const uint32_t g = (num_segments + 1023u) / 1024u;
      hipLaunchKernelGGL(topk_seg_classify_kernel, dim3(g < 4096u ? g : 4096u), dim3(256), 0, s, front, d_begin_offsets, d_end_offsets, n, kk,
                         d_counts_out); }
    {
        const uint32_t wg = (num_segments + 3u) / 4u, grid = wg < TS_MAX_GRID ? wg : TS_MAX_GRID;
#define GS_TSA_WAVE(W)                                                                                                    \
    do {                                                                                                                  \
        if (hv) ts_launch_wave<KT, W, true>(s, front, grid, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x); \
        else ts_launch_wave<KT, W, false>(s, front, grid, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, kk, flt, x);   \
    } while (0)
        GS_TSA_WAVE(1); GS_TSA_WAVE(4); GS_TSA_WAVE(8); GS_TSA_WAVE(16);
#undef GS_TSA_WAVE
    }
    int err = (int)hipGetLastError();
    if (err || !(groups & 2u)) return err;   // (num_items <= 1024: every segment is of a wave class, and final)

    // the selects stage a segment's kept (key, position) pairs at [seg * k, seg * k + kept): the keys in d_keys_out, the positions
    // in d_vals_out (arguments) or in the workspace (pairs)
    uint32_t *pos0 = !hv ? nullptr : pairs ? ws.pos0 : d_vals_out;
    if (hv) tsa_launch_select<KT, true>(s, front, ws, groups, d_keys_in, d_keys_out, pos0, n, kk, flt, x);
    else tsa_launch_select<KT, false>(s, front, ws, groups, d_keys_in, d_keys_out, pos0, n, kk, flt, x);
    err = (int)hipGetLastError();
    if (err) return err;

    // the finish: four passes over the whole image leave the result in half 0, where the pairs were staged
    uint32_t *dk[2] = {d_keys_out, ws.keys1};
    uint32_t *dv[2] = {pos0, ws.pos1};
    int selector = 0;
    err = gs_segmented_sort_u32(ws.seg, ws.seg_bytes, dk, hv ? dv : nullptr, &selector, (uint64_t)num_segments * kk, num_segments, ws.begin,
                                ws.end, 0, 32, descending, key_type, s);
    if (err) return err;
    if (selector != 0) return hipErrorUnknown;
    if (pairs) {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_seganyk_gather_kernel, dim3(num_segments < TS_MAX_GRID ? num_segments : TS_MAX_GRID), dim3(256), 0, s, d_vals_in,
                           (const uint32_t *)ws.pos0, d_vals_out, (const int32_t *)ws.end, d_begin_offsets, num_segments, n, kk);
    }
    return (int)hipGetLastError();
}

static int tsa_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, uint32_t out[8])
{
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!tsa_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;   // such a call enqueues nothing
    const TsGeom g = ts_geom(num_items, num_segments);
    out[0] = ts_groups(num_items); out[1] = tsa_launches(out[0]); out[2] = TR_CH; out[3] = TA_TILE; out[4] = TA_SLAB_TILES;
    out[5] = (uint32_t)g.lmax; out[6] = (uint32_t)g.tmax;
    return hipSuccess;
}

static int tsa_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, uint32_t out[8], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!out) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!tsa_shape_ok(num_items, num_segments, k)) return hipErrorInvalidValue;
    if (num_items == 0 || num_segments == 0 || k == 0) return hipSuccess;   // such a call enqueued nothing
    if (!d_temp) return hipErrorInvalidValue;
    uint32_t st[16];   // the state block is the first term of the workspace
    hipError_t e = hipMemcpyAsync(st, gs_ws_base(d_temp), sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    for (int q = 0; q < 5; ++q) out[q] = st[q];
    out[5] = st[TS_LONG_OK]; out[6] = st[TS_TASKS_OK]; out[7] = st[TS_DROPPED];
    return hipSuccess;
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

size_t gs_topk_rows_u64_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    return tr_temp_bytes<TrKey64>(num_rows, num_cols, k, has_values);
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

int gs_topk_rows_u64(void *d_temp, size_t temp_bytes, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t *d_keys_out,
                     uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                     int key_type, void *stream)
{
    return tr_run<TrKey64>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

size_t gs_topk_segmented_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values)
{
    return ts_temp_bytes(num_items, num_segments, k, has_values, 4);
}

size_t gs_topk_segmented_u16_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values)
{
    return ts_temp_bytes(num_items, num_segments, k, has_values, 2);
}

size_t gs_topk_segmented_u64_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values)
{
    return ts_temp_bytes(num_items, num_segments, k, has_values, 8);
}

int gs_topk_segmented_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                          uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments,
                          const int32_t *d_begin_offsets, const int32_t *d_end_offsets, uint64_t k, int descending, int key_type, void *stream)
{
    return ts_run<TrKey32>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, num_items, num_segments,
                           d_begin_offsets, d_end_offsets, k, descending, key_type, stream);
}

int gs_topk_segmented_u16(void *d_temp, size_t temp_bytes, const uint16_t *d_keys_in, const uint32_t *d_vals_in, uint16_t *d_keys_out,
                          uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments,
                          const int32_t *d_begin_offsets, const int32_t *d_end_offsets, uint64_t k, int descending, int key_type, void *stream)
{
    return ts_run<TrKey16>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, num_items, num_segments,
                           d_begin_offsets, d_end_offsets, k, descending, key_type, stream);
}

int gs_topk_segmented_u64(void *d_temp, size_t temp_bytes, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t *d_keys_out,
                          uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments,
                          const int32_t *d_begin_offsets, const int32_t *d_end_offsets, uint64_t k, int descending, int key_type, void *stream)
{
    return ts_run<TrKey64>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, num_items, num_segments,
                           d_begin_offsets, d_end_offsets, k, descending, key_type, stream);
}

int gs_topk_segmented_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    return ts_plan(num_items, num_segments, k, out);
}

int gs_topk_segmented_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8],
                             void *stream)
{
    return ts_status(d_temp, num_items, num_segments, k, has_values, out, stream);
}

size_t gs_topk_rows_anyk_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    return ta_temp_bytes<TrKey32>(num_rows, num_cols, k, has_values);
}

int gs_topk_rows_anyk_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                          uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                          int key_type, void *stream)
{
    return ta_run<TrKey32>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

int gs_topk_rows_anyk_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    return ta_plan<TrKey32>(num_rows, num_cols, k, out);
}

int gs_topk_rows_anyk_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint64_t row, uint32_t out[8],
                             void *stream)
{
    return ta_status<TrKey32>(d_temp, num_rows, num_cols, k, has_values, row, out, stream);
}

size_t gs_topk_rows_anyk_u16_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    return ta_temp_bytes<TrKey16>(num_rows, num_cols, k, has_values);
}

int gs_topk_rows_anyk_u16(void *d_temp, size_t temp_bytes, const uint16_t *d_keys_in, const uint32_t *d_vals_in, uint16_t *d_keys_out,
                          uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                          int key_type, void *stream)
{
    return ta_run<TrKey16>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

int gs_topk_rows_anyk_u16_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    return ta_plan<TrKey16>(num_rows, num_cols, k, out);
}

int gs_topk_rows_anyk_u16_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint64_t row,
                                 uint32_t out[8], void *stream)
{
    return ta_status<TrKey16>(d_temp, num_rows, num_cols, k, has_values, row, out, stream);
}

size_t gs_topk_rows_anyk_u64_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values)
{
    return ta_temp_bytes<TrKey64>(num_rows, num_cols, k, has_values);
}

int gs_topk_rows_anyk_u64(void *d_temp, size_t temp_bytes, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t *d_keys_out,
                          uint32_t *d_vals_out, uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k, int descending,
                          int key_type, void *stream)
{
    return ta_run<TrKey64>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_rows, num_cols, row_stride, k, descending,
                           key_type, stream);
}

int gs_topk_rows_anyk_u64_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    return ta_plan<TrKey64>(num_rows, num_cols, k, out);
}

int gs_topk_rows_anyk_u64_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint64_t row,
                                 uint32_t out[8], void *stream)
{
    return ta_status<TrKey64>(d_temp, num_rows, num_cols, k, has_values, row, out, stream);
}

size_t gs_topk_segmented_anyk_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values)
{
    return tsa_temp_bytes(num_items, num_segments, k, has_values);
}

int gs_topk_segmented_anyk_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                               uint32_t *d_vals_out, uint32_t *d_counts_out, uint64_t num_items, uint32_t num_segments,
                               const int32_t *d_begin_offsets, const int32_t *d_end_offsets, uint64_t k, int descending, int key_type,
                               void *stream)
{
    return tsa_run(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, d_counts_out, num_items, num_segments, d_begin_offsets,
                   d_end_offsets, k, descending, key_type, stream);
}

int gs_topk_segmented_anyk_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8])
{
    (void)has_values;
    return tsa_plan(num_items, num_segments, k, out);
}

int gs_topk_segmented_anyk_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8],
                                  void *stream)
{
    (void)has_values;
    return tsa_status(d_temp, num_items, num_segments, k, out, stream);
}

}  // extern "C"
