// gs_topk.hip -- gs_topk_u32: the first k elements of the stable LSB sort, by radix select.
//
// The result is defined by the sort: S = gs_lsb_sort_copy_u32(..., 0, 32, descending, key_type) of the same input, and the
// call leaves S[0..k) in the outputs.  Instead of sorting n elements it finds the image of S[k-1] digit by digit, most
// significant byte first, and sorts only the k elements that belong to the result:
//
//   round one   lsb_upsweep at shift 24 + lsb_scan: per-digit totals, per-chunk prefixes (spine) and per-tile prefix16 of
//               the top byte of the image (complemented when descending); topk_pick0 finds the digit d0 that holds the
//               k-th element and opens the state block
//   filter      second read of the input, one workgroup per tile: elements whose top byte sorts before d0 are certainly
//               selected and go, in input order, to the staging area; those with top byte d0 go, in input order, to the
//               candidate list (route 1: the list holds them all).  Positions come from the tables of round one.
//   rounds 2-4  filtered histogram of the next byte + pick, over the candidate list (route 1) or over the input itself
//               with the prefix filter (route 2: more elements share the top byte than the list holds).  Source and count
//               are read from the state block, so both routes are the same launches; workgroups past the count return.
//   select      count / scan / scatter over the same source: every element of the bucket sorting before the k-th image,
//               then the first `take` elements equal to it, appended to the staging area in input order
//   finish      the library's own stable sort of the k staged (key, index) pairs into the outputs, and in pairs mode the
//               gather vals_out[i] = vals_in[idx[i]]
//
// Equal keys always land in ONE group of the staging area (before d0 / before the k-th image / equal to it) and every
// group is filled in input order, so the stable finish reproduces S bit for bit.  No kernel waits on another workgroup
// and no atomic decides a position: the only global atomics are the integer adds of the workgroups' histograms.
// Arrays that fit one workgroup (route 3) are sorted whole into the workspace and the first k copied out.
//
// gs_topk_u16 is the same plan on the 16-bit image of GS_KEY_U16 / I16 / F16 / BF16, at two digits:
// the pick, compaction, filter, histogram, count, select and route-3 kernels below are templates over the element type
// (TkKey<T>: the image and the position of its top byte), instantiated for uint32_t and uint16_t.  Round one is the narrow
// upsweep at shift 8 (narrow_slice_count: one spine column per tile, no prefix16), one round of histogram + pick finds the
// low byte, and the finish is gs_lsb_sort_narrow.  Candidates and staged keys stay 2 bytes wide; indices are u32.  The one
// routine of their own that 16-bit keys have is compact_tile16: the filter and the select read them two to an aligned word.
//
// The host plan is written once too: tk_temp_bytes / tk_run / tk_status over a description of the width (TkKeys32, TkKeys16),
// with one workspace carve, behind the six entry points.  The argument checks, the launches of the pick, filter, histogram,
// count, scan, select, gather and of route 3's iota and copy-out are shared.  A width keeps what the plan calls by name: its
// key types and twiddle, the shape of round one's tables, the launches that count the top byte, the number of rounds below
// it, route 3's limit, arrays and sort, and the sort of the staged pairs with its size query.
//
// gs_topk_u64 shares TkKey<T>, the candidate capacity and the gather, and has a plan of its own at the
// end of this file (topk64_* kernels, TkKeys64, tk64_run): with eight bytes per key the descent skips the bytes that cannot
// differ and moves the bucket to the list at whatever byte it fits.
#include "gs_device.hpp"
#include "gs_lsb.hpp"

namespace gs {

constexpr int TK_THREADS = LSB_THREADS;          // 8 waves
constexpr int TK_WAVES = TK_THREADS / WAVE;
constexpr int TK_KPT = LSB_KPT;                  // 16 elements per thread: a tile is LSB_TILE
constexpr uint32_t TK_MIN_CAND = 65536;          // smallest candidate list; also holds route 3's copies (2 * 32768)
static_assert(TK_THREADS * TK_KPT == LSB_TILE, "the filter walks the tiles of the LSB upsweep");

// state block (u32 words): 0..7 are gs_topk_status' words
enum { TK_ROUTE = 0, TK_KTH = 1, TK_LESS = 2, TK_TAKE = 3, TK_TOP = 4, TK_STAGED0 = 8, TK_D0 = 9, TK_SRC_COUNT = 10, TK_WORDS = 64 };

// What the element width changes in the kernels: the order-preserving image of a raw key (f: the float twiddle, x: the
// uniform xor of sign flip and descending complement, at the key's own width) and the shift of the image's top byte.
// Img is the type of the image, KPT the keys a thread holds of one tile (a tile is TK_THREADS * KPT elements).
template <typename T> struct TkKey;
template <> struct TkKey<uint32_t> {
    using Img = uint32_t;
    static constexpr uint32_t TOP = 24;
    static constexpr int KPT = TK_KPT;
    static __device__ __forceinline__ uint32_t image(uint32_t raw, int f, uint32_t x) { return twiddle_in(raw, f, x); }
};
template <> struct TkKey<uint16_t> {
    using Img = uint32_t;
    static constexpr uint32_t TOP = 8;
    static constexpr int KPT = TK_KPT;
    static __device__ __forceinline__ uint32_t image(uint32_t raw, int f, uint32_t x) { return (f ? float_flip<16>(raw) : raw) ^ x; }
};
// 64-bit keys (gs_topk_u64): the tiles are the wide pass's, 4096 elements at 8 keys per thread
template <> struct TkKey<uint64_t> {
    using Img = uint64_t;
    static constexpr uint32_t TOP = 56;
    static constexpr int KPT = 8;
    static __device__ __forceinline__ uint64_t image(uint64_t raw, int f, uint64_t x)
    {
        if (f) raw ^= (uint64_t)((int64_t)raw >> 63) | 0x8000000000000000ull;
        return raw ^ x;
    }
};

static inline uint64_t tk_tiles(uint64_t n) { const uint64_t t = (n + LSB_TILE - 1) / LSB_TILE; return t ? t : 1; }
static inline uint64_t tk_grid(uint64_t n) { return (tk_tiles(n) + LSB_CHUNK - 1) / LSB_CHUNK; }
static inline uint64_t tk_cand_cap(uint64_t n) { return n / 32 > TK_MIN_CAND ? n / 32 : TK_MIN_CAND; }

// ---------------------------------------------------------------- round one: pick --
// One workgroup: the digit d0 whose run of S holds position k - 1.  Opens the state block and clears the histograms of
// rounds two to four.
template <uint32_t TOP>
__global__ __launch_bounds__(RADIX) void topk_pick0_kernel(const uint32_t *__restrict__ totals, uint32_t *__restrict__ state,
                                                           uint32_t *__restrict__ hist, uint32_t n, uint32_t k, uint32_t cap)
{
    __shared__ uint32_t scratch[8];
    const uint32_t t = threadIdx.x, c = totals[t];
    const uint32_t ex = block_exclusive_scan_256(c, scratch, nullptr);
    for (uint32_t i = t; i < 3u * RADIX; i += RADIX) hist[i] = 0;
    if (t >= 5 && t < TK_WORDS && t != TK_STAGED0 && t != TK_D0 && t != TK_SRC_COUNT) state[t] = 0;
    if (ex < k && k - ex <= c) {
        const bool fits = c <= cap;
        state[TK_ROUTE] = fits ? 1u : 2u;
        state[TK_KTH] = t << TOP;
        state[TK_LESS] = ex;
        state[TK_TAKE] = k - ex;
        state[TK_TOP] = c;
        state[TK_STAGED0] = ex;
        state[TK_D0] = t;
        state[TK_SRC_COUNT] = fits ? c : n;
    }
}

// Rounds two to four: the digit at `shift` that holds the k-th element among those matching the prefix so far.
__global__ __launch_bounds__(RADIX) void topk_pick_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ state, uint32_t shift)
{
    __shared__ uint32_t scratch[8];
    const uint32_t t = threadIdx.x, c = hist[t];
    const uint32_t krem = state[TK_TAKE], less = state[TK_LESS], kth = state[TK_KTH];
    const uint32_t ex = block_exclusive_scan_256(c, scratch, nullptr);   // (its barriers order the reads above before the writes below)
    if (ex < krem && krem - ex <= c) {
        state[TK_KTH] = kth | (t << shift);
        state[TK_LESS] = less + ex;
        state[TK_TAKE] = krem - ex;
    }
}

// ------------------------------------------------- ordered two-group compaction --
// One workgroup, one tile of `src` starting at element lo: wave w owns elements [w * 1024, (w + 1) * 1024) of the tile
// and reads them in 16 coalesced rows, so (wave, row, lane) is the input order.  cls(raw key) says 0 = drop, 1 = group A,
// 2 = group B.  Element number r of a group inside the tile goes to position base + r of that group's arrays, when
// below lim (group B's limit cuts the tie run; the others only fence the arrays).  IDX: also write the element's index --
// src_idx[i], or i itself when src_idx is null.
template <bool IDX, typename T, typename Cls>
__device__ __forceinline__ void compact_tile(const T *__restrict__ src, const uint32_t *__restrict__ src_idx, uint32_t lo,
                                             uint32_t count, Cls cls, uint32_t baseA, uint32_t limA, T *__restrict__ ak,
                                             uint32_t *__restrict__ ai, uint32_t baseB, uint32_t limB, T *__restrict__ bk,
                                             uint32_t *__restrict__ bi, uint32_t (*wcnt)[TK_WAVES])
{
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = lo + w * (uint32_t)(WAVE * TK_KPT) + lane;
    uint32_t raw[TK_KPT], c[TK_KPT];
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        raw[u] = (i < count && i >= lo) ? (uint32_t)__builtin_nontemporal_load(src + i) : 0u;
    }
    uint32_t nA = 0, nB = 0;
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        c[u] = (i < count && i >= lo) ? cls(raw[u]) : 0u;
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(c[u] == 1u));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(c[u] == 2u));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    uint32_t tot = 0;
    for (uint32_t j = 0; j < (uint32_t)TK_WAVES; ++j) {
        const uint32_t a = wcnt[0][j], b = wcnt[1][j];
        tot += a + b;
        if (j < w) { baseA += a; baseB += b; }
    }
    if (tot == 0) return;   // nothing of either group in this tile (workgroup-uniform)
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        asm volatile("" : "+v"(c[u]));   // ballot again: 32 masks kept from the counting loop would not fit the SGPRs
        const unsigned long long mA = __builtin_amdgcn_ballot_w64(c[u] == 1u), mB = __builtin_amdgcn_ballot_w64(c[u] == 2u);
        if (c[u] == 1u) {
            const uint32_t pos = baseA + count_lower(mA);
            if (pos < limA) {
                ak[pos] = (T)raw[u];
                if (IDX) ai[pos] = src_idx ? src_idx[i] : i;
            }
        } else if (c[u] == 2u) {
            const uint32_t pos = baseB + count_lower(mB);
            if (pos < limB) {
                bk[pos] = (T)raw[u];
                if (IDX) bi[pos] = src_idx ? src_idx[i] : i;
            }
        }
        baseA += (uint32_t)__popcll(mA);
        baseB += (uint32_t)__popcll(mB);
    }
}

// The same for 16-bit keys with packed loads: a lane reads aligned 4-byte words of two neighbouring elements, eight rows of 64
// words per wave, and a ninth word when the wave's span starts in the upper half of a word (the array may start at any even
// address; only words that hold an element of the span are touched).  The input order is (wave, row, lane, position in
// the word): word indices, and so element indices, still grow along it.
#ifndef GS_TOPK16_PACKED
#define GS_TOPK16_PACKED 1
#endif
template <bool IDX, typename Cls>
__device__ __forceinline__ void compact_tile16(const uint16_t *__restrict__ src, const uint32_t *__restrict__ src_idx, uint32_t lo,
                                               uint32_t count, Cls cls, uint32_t baseA, uint32_t limA, uint16_t *__restrict__ ak,
                                               uint32_t *__restrict__ ai, uint32_t baseB, uint32_t limB, uint16_t *__restrict__ bk,
                                               uint32_t *__restrict__ bi, uint32_t (*wcnt)[TK_WAVES])
{
    constexpr int ROWS = TK_KPT / 2 + 1;
    constexpr uint32_t SPAN = (uint32_t)(WAVE * TK_KPT);          // elements of one wave
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t e0 = lo + w * SPAN;                            // the wave's first element
    const uint32_t len = (e0 >= lo && e0 < count) ? (count - e0 < SPAN ? count - e0 : SPAN) : 0u;
    const uintptr_t addr = (uintptr_t)src + 2 * (uintptr_t)e0;
    const uint32_t par = (uint32_t)(addr >> 1) & 1u;              // 1: element e0 is the upper half of its word
    const uint32_t *W = reinterpret_cast<const uint32_t *>(addr - 2 * par);
    uint32_t word[ROWS], c[ROWS];                                 // c: class of the lower element | class of the upper one << 2
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint32_t j = (uint32_t)r * WAVE + lane, a = 2u * j - par;       // word j holds elements a and a + 1 of the span
        word[r] = (a < len || a + 1u < len) ? __builtin_nontemporal_load(W + j) : 0u;     // (a = 0xffffffff for j = 0, par = 1)
    }
    uint32_t nA = 0, nB = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint32_t j = (uint32_t)r * WAVE + lane, a = 2u * j - par;
        const uint32_t ca = a < len ? cls(word[r] & 0xffffu) : 0u, cb = a + 1u < len ? cls(word[r] >> 16) : 0u;
        c[r] = ca | (cb << 2);
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ca == 1u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cb == 1u));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(ca == 2u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cb == 2u));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    uint32_t tot = 0;
    for (uint32_t j = 0; j < (uint32_t)TK_WAVES; ++j) {
        const uint32_t a = wcnt[0][j], b = wcnt[1][j];
        tot += a + b;
        if (j < w) { baseA += a; baseB += b; }
    }
    if (tot == 0) return;   // nothing of either group in this tile (workgroup-uniform)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const uint32_t j = (uint32_t)r * WAVE + lane, i = e0 + 2u * j - par;      // index of the lower element
        asm volatile("" : "+v"(c[r]));   // ballot again, as in compact_tile
        const uint32_t ca = c[r] & 3u, cb = c[r] >> 2;
        const unsigned long long mA0 = __builtin_amdgcn_ballot_w64(ca == 1u), mA1 = __builtin_amdgcn_ballot_w64(cb == 1u);
        const unsigned long long mB0 = __builtin_amdgcn_ballot_w64(ca == 2u), mB1 = __builtin_amdgcn_ballot_w64(cb == 2u);
        const uint32_t pA = baseA + count_lower(mA0) + count_lower(mA1), pB = baseB + count_lower(mB0) + count_lower(mB1);
        if (ca) {
            const uint32_t pos = ca == 1u ? pA : pB;
            if (pos < (ca == 1u ? limA : limB)) {
                (ca == 1u ? ak : bk)[pos] = (uint16_t)word[r];
                if (IDX) (ca == 1u ? ai : bi)[pos] = src_idx ? src_idx[i] : i;
            }
        }
        if (cb) {
            const uint32_t pos = cb == 1u ? pA + (ca == 1u ? 1u : 0u) : pB + (ca == 2u ? 1u : 0u);
            if (pos < (cb == 1u ? limA : limB)) {
                (cb == 1u ? ak : bk)[pos] = (uint16_t)(word[r] >> 16);
                if (IDX) (cb == 1u ? ai : bi)[pos] = src_idx ? src_idx[i + 1u] : i + 1u;
            }
        }
        baseA += (uint32_t)__popcll(mA0) + (uint32_t)__popcll(mA1);
        baseB += (uint32_t)__popcll(mB0) + (uint32_t)__popcll(mB1);
    }
}

// the compaction an element type takes
template <bool IDX, typename T, typename Cls>
__device__ __forceinline__ void compact_any(const T *__restrict__ src, const uint32_t *__restrict__ src_idx, uint32_t lo, uint32_t count,
                                            Cls cls, uint32_t baseA, uint32_t limA, T *__restrict__ ak, uint32_t *__restrict__ ai,
                                            uint32_t baseB, uint32_t limB, T *__restrict__ bk, uint32_t *__restrict__ bi,
                                            uint32_t (*wcnt)[TK_WAVES])
{
    if constexpr (sizeof(T) == 2 && GS_TOPK16_PACKED) compact_tile16<IDX>(src, src_idx, lo, count, cls, baseA, limA, ak, ai, baseB, limB, bk, bi, wcnt);
    else compact_tile<IDX>(src, src_idx, lo, count, cls, baseA, limA, ak, ai, baseB, limB, bk, bi, wcnt);
}

// --------------------------------------------------------------------- filter --
// Second read of the input, one workgroup per tile of the upsweep.  Group A: top byte before d0 -> staging area, at the
// number of such elements in front of the tile (sum over the digits below d0 of spine + prefix16).  Group B (route 1
// only): top byte d0 -> candidate list, at spine[d0] + prefix16[d0].  16-bit keys: round one was the narrow upsweep, whose
// spine has one column per tile (grid = the number of tiles) and no prefix16, so spine[d][tile] alone is the digit's base.
template <bool IDX, typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_filter_kernel(const T *__restrict__ keys, const uint32_t *__restrict__ spine,
                                                                 const uint16_t *__restrict__ prefix16, const uint32_t *__restrict__ state,
                                                                 T *__restrict__ stage_keys, uint32_t *__restrict__ stage_idx,
                                                                 T *__restrict__ cand_keys, uint32_t *__restrict__ cand_idx, uint32_t n,
                                                                 uint32_t grid, uint32_t k, uint32_t cap, int f32, uint32_t x)
{
    __shared__ uint32_t wcnt[2][TK_WAVES];
    __shared__ uint32_t wsum[TK_WAVES];
    __shared__ uint32_t cbase;
    const uint32_t tile = blockIdx.x, chunk = tile / (uint32_t)LSB_CHUNK, tid = threadIdx.x;
    const uint32_t d0 = state[TK_D0], route = state[TK_ROUTE];
    uint32_t below = 0;
    if (tid <= d0) {   // d0 < 256: only the digits that count are read
        uint32_t v;
        if constexpr (sizeof(T) == 4) v = spine[(size_t)tid * grid + chunk] + prefix16[(size_t)tile * RADIX + tid];
        else v = spine[(size_t)tid * grid + tile];
        if (tid < d0) below = v;
        if (tid == d0) cbase = v;
    }
    below = wave_reduce_sum(below);
    if (lane_id() == 0) wsum[wave_id()] = below;
    __syncthreads();
    uint32_t baseA = 0;
    for (int j = 0; j < RADIX / WAVE; ++j) baseA += wsum[j];
    const uint32_t baseB = cbase;
    auto cls = [&](uint32_t raw) -> uint32_t {
        const uint32_t tb = TkKey<T>::image(raw, f32, x) >> TkKey<T>::TOP;
        return tb < d0 ? 1u : (tb == d0 && route == 1u) ? 2u : 0u;
    };
    compact_any<IDX>(keys, (const uint32_t *)nullptr, tile * (uint32_t)LSB_TILE, n, cls, baseA, k, stage_keys, stage_idx, baseB, cap, cand_keys, cand_idx, wcnt);
}

// ------------------------------------------------------ rounds two to four: count --
// Histogram of the byte at `shift` over the source elements whose bytes above it equal the prefix found so far.  LDS
// histogram per workgroup, then one integer add per non-empty bin.
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_hist_kernel(const T *__restrict__ keys, const T *__restrict__ cand_keys,
                                                               const uint32_t *__restrict__ state, uint32_t *__restrict__ hist,
                                                               uint32_t shift, int f32, uint32_t x)
{
    __shared__ uint32_t h[RADIX];
    const uint32_t count = state[TK_SRC_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * LSB_TILE;
    if (lo64 >= count) return;
    const uint32_t lo = (uint32_t)lo64, tid = threadIdx.x;
    const T *src = state[TK_ROUTE] == 1u ? cand_keys : keys;
    const uint32_t prefix = state[TK_KTH], mask = 0xffffff00u << shift;
    if (tid < (uint32_t)RADIX) h[tid] = 0;
    __syncthreads();
    uint32_t raw[TK_KPT];
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = lo + (uint32_t)u * TK_THREADS + tid;
        raw[u] = (i < count && i >= lo) ? (uint32_t)__builtin_nontemporal_load(src + i) : 0u;
    }
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = lo + (uint32_t)u * TK_THREADS + tid;
        const uint32_t img = TkKey<T>::image(raw[u], f32, x);
        if (i < count && i >= lo && ((img ^ prefix) & mask) == 0u) hist_add(h, (img >> shift) & 255u);
    }
    __syncthreads();
    if (tid < (uint32_t)RADIX && h[tid]) atomicAdd(&hist[tid], h[tid]);
}

// -------------------------------------------------------- final ordered select --
// count: per source tile, the elements of the bucket that sort before the k-th image and those equal to it
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_count_kernel(const T *__restrict__ keys, const T *__restrict__ cand_keys,
                                                                const uint32_t *__restrict__ state, uint32_t *__restrict__ tilecnt,
                                                                int f32, uint32_t x)
{
    __shared__ uint32_t wl[TK_WAVES], we[TK_WAVES];
    const uint32_t count = state[TK_SRC_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * LSB_TILE;
    if (lo64 >= count) return;
    const uint32_t lo = (uint32_t)lo64, tid = threadIdx.x;
    const T *src = state[TK_ROUTE] == 1u ? cand_keys : keys;
    const uint32_t kth = state[TK_KTH], lowest = kth & (0xffu << TkKey<T>::TOP);
    uint32_t raw[TK_KPT];
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = lo + (uint32_t)u * TK_THREADS + tid;
        raw[u] = (i < count && i >= lo) ? (uint32_t)__builtin_nontemporal_load(src + i) : 0u;
    }
    uint32_t l = 0, e = 0;
#pragma unroll
    for (int u = 0; u < TK_KPT; ++u) {
        const uint32_t i = lo + (uint32_t)u * TK_THREADS + tid;
        const uint32_t img = TkKey<T>::image(raw[u], f32, x);
        const bool ok = i < count && i >= lo;
        l += (ok && img >= lowest && img < kth) ? 1u : 0u;
        e += (ok && img == kth) ? 1u : 0u;
    }
    l = wave_reduce_sum(l);
    e = wave_reduce_sum(e);
    if (lane_id() == 0) { wl[wave_id()] = l; we[wave_id()] = e; }
    __syncthreads();
    if (tid == 0) {
        uint32_t sl = 0, se = 0;
        for (int j = 0; j < TK_WAVES; ++j) { sl += wl[j]; se += we[j]; }
        tilecnt[2u * blockIdx.x] = sl;
        tilecnt[2u * blockIdx.x + 1u] = se;
    }
}

// scan: one workgroup, exclusive prefixes of both counts over the source tiles, in place
constexpr int TK_SCAN_THREADS = 1024;
__global__ __launch_bounds__(TK_SCAN_THREADS) void topk_scan_kernel(const uint32_t *__restrict__ state, uint32_t *__restrict__ tilecnt)
{
    __shared__ uint32_t wsl[TK_SCAN_THREADS / WAVE], wse[TK_SCAN_THREADS / WAVE];
    const uint32_t count = state[TK_SRC_COUNT];
    const uint32_t tiles = (uint32_t)(((uint64_t)count + LSB_TILE - 1) / LSB_TILE);
    const int w = wave_id(), lane = lane_id();
    uint32_t carry_l = 0, carry_e = 0;
    for (uint32_t base = 0; base < tiles; base += TK_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t l = i < tiles ? tilecnt[2u * i] : 0u, e = i < tiles ? tilecnt[2u * i + 1u] : 0u;
        const uint32_t il = wave_inclusive_scan(l), ie = wave_inclusive_scan(e);
        if (lane == 63) { wsl[w] = il; wse[w] = ie; }
        __syncthreads();
        uint32_t bl = 0, be = 0, tl = 0, te = 0;
        for (int j = 0; j < TK_SCAN_THREADS / WAVE; ++j) {
            const uint32_t a = wsl[j], b = wse[j];
            if (j < w) { bl += a; be += b; }
            tl += a; te += b;
        }
        if (i < tiles) {
            tilecnt[2u * i] = carry_l + bl + il - l;
            tilecnt[2u * i + 1u] = carry_e + be + ie - e;
        }
        carry_l += tl; carry_e += te;
        __syncthreads();
    }
}

// scatter: group A = the bucket's elements before the k-th image, behind the staged elements of the filter; group B = the
// elements equal to it, behind all that sort before it, cut after `take` of them
template <bool IDX, typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_select_kernel(const T *__restrict__ keys, const T *__restrict__ cand_keys,
                                                                 const uint32_t *__restrict__ cand_idx, const uint32_t *__restrict__ state,
                                                                 const uint32_t *__restrict__ tilecnt, T *__restrict__ stage_keys,
                                                                 uint32_t *__restrict__ stage_idx, uint32_t k, int f32, uint32_t x)
{
    __shared__ uint32_t wcnt[2][TK_WAVES];
    const uint32_t count = state[TK_SRC_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * LSB_TILE;
    if (lo64 >= count) return;
    const bool list = state[TK_ROUTE] == 1u;
    const uint32_t kth = state[TK_KTH], lowest = kth & (0xffu << TkKey<T>::TOP), less = state[TK_LESS], take = state[TK_TAKE];
    const uint32_t baseA = state[TK_STAGED0] + tilecnt[2u * blockIdx.x], baseB = less + tilecnt[2u * blockIdx.x + 1u];
    const uint32_t limB = less + take < k ? less + take : k;
    auto cls = [&](uint32_t raw) -> uint32_t {
        const uint32_t img = TkKey<T>::image(raw, f32, x);
        return img == kth ? 2u : (img >= lowest && img < kth) ? 1u : 0u;
    };
    compact_any<IDX>(list ? cand_keys : keys, list ? cand_idx : (const uint32_t *)nullptr, (uint32_t)lo64, count, cls, baseA, k, stage_keys, stage_idx,
                      baseB, limB, stage_keys, stage_idx, wcnt);
}

// --------------------------------------------------------------------- finish --
__global__ __launch_bounds__(256) void topk_gather_kernel(const uint32_t *__restrict__ vals_in, const uint32_t *__restrict__ idx,
                                                          uint32_t *__restrict__ vals_out, uint32_t k, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k) return;
    const uint32_t j = idx[i];
    if (j < n) vals_out[i] = vals_in[j];
}

__global__ __launch_bounds__(256) void topk_iota_kernel(uint32_t *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = i;
}

// Route 3, one workgroup: copy the first k of the sorted array out and write the status words from it.
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_small_finish_kernel(const T *__restrict__ sk, const uint32_t *__restrict__ sv,
                                                                       T *__restrict__ keys_out, uint32_t *__restrict__ vals_out,
                                                                       uint32_t *__restrict__ state, uint32_t n, uint32_t k, int f32, uint32_t x)
{
    __shared__ uint32_t acc[2];
    const uint32_t tid = threadIdx.x;
    if (tid < 2) acc[tid] = 0;
    __syncthreads();
    const uint32_t kth = TkKey<T>::image(sk[k - 1u], f32, x);
    uint32_t less = 0, top = 0;
    for (uint32_t i = tid; i < n; i += TK_THREADS) {
        const uint32_t raw = sk[i], img = TkKey<T>::image(raw, f32, x);
        less += img < kth ? 1u : 0u;
        top += (img >> TkKey<T>::TOP) == (kth >> TkKey<T>::TOP) ? 1u : 0u;
        if (i < k) {
            keys_out[i] = (T)raw;
            if (vals_out) vals_out[i] = sv[i];
        }
    }
    less = wave_reduce_sum(less);
    top = wave_reduce_sum(top);
    if (lane_id() == 0) { atomicAdd(&acc[0], less); atomicAdd(&acc[1], top); }
    __syncthreads();
    if (tid < (uint32_t)TK_WORDS) {
        uint32_t v = 0;
        if (tid == TK_ROUTE) v = 3u;
        else if (tid == TK_KTH) v = kth;
        else if (tid == TK_LESS) v = acc[0];
        else if (tid == TK_TAKE) v = k - acc[0];
        else if (tid == TK_TOP) v = acc[1];
        state[tid] = v;
    }
}

// ----------------------------------------------------------------------- host --
template <typename T> struct TopkWs {
    uint32_t *state, *hist;          // [64], [3][256] (16-bit keys have one round: [256])
    char *scratch;                   // 512 bytes for small_stable_sort (route 3 of 32-bit keys)
    uint32_t *spine, *totals;
    uint16_t *prefix16;              // null without KT::PREFIX16
    uint32_t *tilecnt;               // [tiles][2]: {before the k-th image, equal to it} per source tile, scanned in place
    T *cand_keys;                    // the candidate area: keys, then (has_values) indices; route 3 lays its arrays over both
    uint32_t *cand_idx;
    T *stage_keys;
    uint32_t *stage_idx, *idx_sorted;
    char *sort_ws;
    size_t sort_ws_bytes;
};

// route 3's arrays (inside the candidate area) and the workspace of its sort
template <typename T> struct TopkSmall {
    T *keys;
    uint32_t *vals, *iota;
    char *sort_ws;
    size_t sort_ws_bytes;
};

// route 3's arrays for 16-bit keys, as offsets into the candidate area (at least 2 * TK_MIN_CAND = 128 KiB; 384 KiB with
// values): the sorted keys, the sorted values, the iota of the arguments form, then the workspace of the sort of at most
// LSB_TILE elements
constexpr size_t TK16_SMALL_VALS = (size_t)LSB_TILE * 2, TK16_SMALL_IOTA = TK16_SMALL_VALS + (size_t)LSB_TILE * 4,
                 TK16_SMALL_WS = TK16_SMALL_IOTA + (size_t)LSB_TILE * 4;

// What the key width changes on the host, and nothing else; tk_temp_bytes / tk_run / tk_status below are the plan itself.
//   T, type_ok, twiddle   the element, the key types the entry point takes, TkKey<T>::image's (f, x) for a type and direction
//   spine_cols, PREFIX16  round one's tables: spine columns (one per chunk, or one per tile) and whether there is a prefix16
//   sort_temp_bytes       the size query of sort_staged
//   EMPTY_QUERY_IS_ZERO   the public size query answers 0 for k == 0 or n == 0
//   small_limit / small_area / small_sort   route 3: the longest array it takes, its arrays (false: they would not fit) and
//                         the stable sort of the whole array into them
//   count_top_byte        round one's launches: per-digit totals and per-tile bases of the image's top byte
//   ROUNDS                histogram + pick rounds below the top byte, at shifts 8 * (ROUNDS - 1), ..., 0
//   sort_staged           the stable sort of the k staged (key, index) pairs into the outputs
namespace {   // (their member functions are this file's alone: nothing is added to the library's symbols)
struct TkKeys32 {
    using T = uint32_t;
    static constexpr bool PREFIX16 = true, EMPTY_QUERY_IS_ZERO = false;
    static constexpr int ROUNDS = 3;
    static bool type_ok(int key_type) { return key_type >= GS_KEY_U32 && key_type <= GS_KEY_F32; }
    static void twiddle(int key_type, int descending, int *f, uint32_t *x)
    {
        PassParams p{};
        lsb_twiddle_masks(key_type, descending, true, true, p);
        *f = p.f32_in; *x = p.xor_in;
    }
    static uint64_t spine_cols(uint64_t n) { return tk_grid(n); }
    static size_t sort_temp_bytes(uint64_t k, bool hv) { return gs_lsb_copy_temp_bytes(k, hv ? 1 : 0); }
    static uint32_t small_limit(bool hv) { return small_sort_capacity(hv); }
    // keys | indices of the arguments form in the first list, values in the second
    static bool small_area(const TopkWs<T> &ws, uint32_t, bool hv, int, TopkSmall<T> *a)
    {
        if (small_sort_capacity(hv) > TK_MIN_CAND / 2) return false;
        *a = {ws.cand_keys, ws.cand_idx, ws.cand_keys + TK_MIN_CAND / 2, ws.scratch, 512};
        return true;
    }
    static int small_sort(const TopkSmall<T> &a, const T *keys_in, const uint32_t *vals_in, bool hv, uint32_t n, int key_type, int descending,
                          hipStream_t s)
    {
        int f;
        uint32_t x;
        twiddle(key_type, descending, &f, &x);
        return small_stable_sort(a.sort_ws, a.sort_ws_bytes, keys_in, a.keys, vals_in, hv ? a.vals : nullptr, n, 0, 32, f, x, f, x, s);
    }
    static int count_top_byte(const T *keys_in, uint64_t n, int key_type, int descending, const TopkWs<T> &ws, hipStream_t s)
    {
        PassParams p = lsb_make_params(n, 24, 8);
        lsb_twiddle_masks(key_type, descending, true, true, p);
        const int e = lsb_upsweep(keys_in, ws.spine, ws.prefix16, p, s);
        return e ? e : lsb_scan(ws.spine, ws.totals, p.grid, s);
    }
    static int sort_staged(const TopkWs<T> &ws, T *keys_out, uint32_t *idx_out, uint64_t k, bool hv, int key_type, int descending, hipStream_t s)
    {
        return gs_lsb_sort_copy_u32(ws.sort_ws, ws.sort_ws_bytes, ws.stage_keys, keys_out, hv ? ws.stage_idx : nullptr, idx_out, k, 0, 32,
                                    descending, key_type, s);
    }
};

struct TkKeys16 {
    using T = uint16_t;
    static constexpr bool PREFIX16 = false, EMPTY_QUERY_IS_ZERO = true;
    static constexpr int ROUNDS = 1;
    static bool type_ok(int key_type) { return key_type == GS_KEY_U16 || key_type == GS_KEY_I16 || key_type == GS_KEY_F16 || key_type == GS_KEY_BF16; }
    static void twiddle(int key_type, int descending, int *f, uint32_t *x)
    {
        *f = (key_type == GS_KEY_F16 || key_type == GS_KEY_BF16) ? 1 : 0;
        *x = (key_type == GS_KEY_U16 ? 0u : 0x8000u) ^ (descending ? 0xffffu : 0u);   // the image stays 16 bits wide
    }
    static uint64_t spine_cols(uint64_t n) { return tk_tiles(n); }
    static size_t sort_temp_bytes(uint64_t k, bool hv) { return gs_lsb_narrow_temp_bytes(k, GS_KEY_U16, hv ? 4 : 0); }
    static uint32_t small_limit(bool) { return (uint32_t)LSB_TILE; }
    static bool small_area(const TopkWs<T> &ws, uint32_t n, bool hv, int key_type, TopkSmall<T> *a)
    {
        char *area = (char *)ws.cand_keys;
        const size_t sort_bytes = gs_lsb_narrow_temp_bytes(n, key_type, hv ? 4 : 0);
        if (TK16_SMALL_WS + sort_bytes > (size_t)(hv ? 6 : 2) * TK_MIN_CAND) return false;
        *a = {(T *)area, (uint32_t *)(area + TK16_SMALL_VALS), (uint32_t *)(area + TK16_SMALL_IOTA), area + TK16_SMALL_WS, sort_bytes};
        return true;
    }
    static int small_sort(const TopkSmall<T> &a, const T *keys_in, const uint32_t *vals_in, bool hv, uint32_t n, int key_type, int descending,
                          hipStream_t s)
    {
        return gs_lsb_sort_narrow(a.sort_ws, a.sort_ws_bytes, keys_in, a.keys, hv ? vals_in : nullptr, hv ? a.vals : nullptr, n, key_type,
                                  hv ? 4 : 0, 0, 16, descending, s);
    }
    // the narrow upsweep and its spine scan
    static int count_top_byte(const T *keys_in, uint64_t n, int key_type, int descending, const TopkWs<T> &ws, hipStream_t s)
    {
        const LargeDigit dg = {8, 8, key_type, descending ? 1 : 0, true, true};
        return narrow_slice_count(keys_in, n, 4, dg, ws.spine, ws.totals, s);
    }
    static int sort_staged(const TopkWs<T> &ws, T *keys_out, uint32_t *idx_out, uint64_t k, bool hv, int key_type, int descending, hipStream_t s)
    {
        return gs_lsb_sort_narrow(ws.sort_ws, ws.sort_ws_bytes, ws.stage_keys, keys_out, hv ? ws.stage_idx : nullptr, idx_out, k, key_type,
                                  hv ? 4 : 0, 0, 16, descending, s);
    }
};
}  // namespace

template <typename KT>
static size_t tk_carve(char *base, uint64_t n, uint64_t k, bool hv, TopkWs<typename KT::T> *ws)
{
    using T = typename KT::T;
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = (char *)((uintptr_t)base + off); off += gs_ws_align(bytes); return p; };   // (base may be null: the size query)
    char *head = take(4096);
    char *spine = take((size_t)RADIX * 4 * KT::spine_cols(n));
    char *totals = take(RADIX * 4);
    char *prefix16 = KT::PREFIX16 ? take((size_t)RADIX * 2 * tk_tiles(n)) : nullptr;
    char *tilecnt = take((size_t)8 * tk_tiles(n));
    char *ck = take(sizeof(T) * tk_cand_cap(n));
    char *ci = hv ? take((size_t)4 * tk_cand_cap(n)) : nullptr;
    char *sk = take(sizeof(T) * k);
    char *si = hv ? take((size_t)4 * k) : nullptr;
    char *is = hv ? take((size_t)4 * k) : nullptr;
    const size_t sort_bytes = KT::sort_temp_bytes(k, hv);
    char *sw = take(sort_bytes);
    if (ws) {
        ws->state = (uint32_t *)head; ws->hist = (uint32_t *)(head + 256); ws->scratch = head + 256 + 3 * RADIX * 4;
        ws->spine = (uint32_t *)spine; ws->totals = (uint32_t *)totals; ws->prefix16 = (uint16_t *)prefix16;
        ws->tilecnt = (uint32_t *)tilecnt; ws->cand_keys = (T *)ck; ws->cand_idx = (uint32_t *)ci;
        ws->stage_keys = (T *)sk; ws->stage_idx = (uint32_t *)si; ws->idx_sorted = (uint32_t *)is;
        ws->sort_ws = sw; ws->sort_ws_bytes = sort_bytes;
    }
    return off;
}

template <typename KT>
static size_t tk_temp_bytes(uint64_t num_items, uint64_t k, int has_values)
{
    if (KT::EMPTY_QUERY_IS_ZERO && (k == 0 || num_items == 0)) return 0;
    return tk_carve<KT>(nullptr, num_items, k, has_values != 0, nullptr) + GS_WS_SLACK;
}

// the launches that come in a form with indices (IDX) and one without
template <bool IDX, typename T>
static void tk_launch_filter(hipStream_t s, const T *keys_in, const TopkWs<T> &ws, uint32_t n, uint32_t tiles, uint32_t cols, uint32_t k,
                             uint32_t cap, int f, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_filter_kernel<IDX, T>), dim3(tiles), dim3(TK_THREADS), 0, s, keys_in, ws.spine, (const uint16_t *)ws.prefix16,
                       ws.state, ws.stage_keys, ws.stage_idx, ws.cand_keys, ws.cand_idx, n, cols, k, cap, f, x);
}

template <bool IDX, typename T>
static void tk_launch_select(hipStream_t s, const T *keys_in, const TopkWs<T> &ws, uint32_t tiles, uint32_t k, int f, uint32_t x)
{
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL((topk_select_kernel<IDX, T>), dim3(tiles), dim3(TK_THREADS), 0, s, keys_in, (const T *)ws.cand_keys,
                       (const uint32_t *)ws.cand_idx, ws.state, ws.tilecnt, ws.stage_keys, ws.stage_idx, k, f, x);
}

template <typename KT>
static int tk_run(void *d_temp, size_t temp_bytes, const typename KT::T *d_keys_in, const uint32_t *d_vals_in, typename KT::T *d_keys_out,
                  uint32_t *d_vals_out, uint64_t num_items, uint64_t k, int descending, int key_type, void *stream)
{
    using T = typename KT::T;
    GS_CLEAR_STALE_ERROR();
    if (num_items >= (1ull << 32) || k > num_items) return hipErrorInvalidValue;
    if (!KT::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (k == 0 || num_items == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < tk_temp_bytes<KT>(num_items, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & (sizeof(T) - 1)) != 0 || (((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & 3u) != 0)
        return hipErrorInvalidValue;
    {
        const void *arr[4] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out};
        const size_t bytes[4] = {(size_t)num_items * sizeof(T), (size_t)num_items * 4, (size_t)k * sizeof(T), (size_t)k * 4};
        if (gs_any_overlap4(arr, bytes)) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_items, kk = (uint32_t)k;
    TopkWs<T> ws;
    tk_carve<KT>(gs_ws_base(d_temp), num_items, k, hv, &ws);
    int f, e;
    uint32_t x;
    KT::twiddle(key_type, descending, &f, &x);

    if (n <= KT::small_limit(hv)) {
        // route 3: the array fits one workgroup (32-bit keys) or one tile (16-bit keys).  Sorted whole into the candidate
        // area, then the first k are copied out.
        TopkSmall<T> a;
        if (!KT::small_area(ws, n, hv, key_type, &a)) return hipErrorInvalidValue;   // (the copies would not fit)
        const uint32_t *vin = d_vals_in;
        if (hv && !vin) {
            KernelTimer kt(GS_K_OTHER, s);
            hipLaunchKernelGGL(topk_iota_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, a.iota, n);
            vin = a.iota;
        }
        if ((e = KT::small_sort(a, d_keys_in, vin, hv, n, key_type, descending, s))) return e;
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_small_finish_kernel<T>, dim3(1), dim3(TK_THREADS), 0, s, (const T *)a.keys, (const uint32_t *)a.vals, d_keys_out,
                           d_vals_out, ws.state, n, kk, f, x);
        return (int)hipGetLastError();
    }

    // round one: the top byte's counts, the pick
    const uint32_t tiles = (uint32_t)tk_tiles(num_items), cols = (uint32_t)KT::spine_cols(num_items);
    if ((e = KT::count_top_byte(d_keys_in, num_items, key_type, descending, ws, s))) return e;
    const uint32_t cap = (uint32_t)tk_cand_cap(num_items);
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_pick0_kernel<TkKey<T>::TOP>, dim3(1), dim3(RADIX), 0, s, ws.totals, ws.state, ws.hist, n, kk, cap);
    }
    // filter
    if (hv) tk_launch_filter<true>(s, d_keys_in, ws, n, tiles, cols, kk, cap, f, x);
    else tk_launch_filter<false>(s, d_keys_in, ws, n, tiles, cols, kk, cap, f, x);
    // the rounds below the top byte
    for (int r = 0; r < KT::ROUNDS; ++r) {
        const uint32_t shift = 8u * (uint32_t)(KT::ROUNDS - 1 - r);
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk_hist_kernel<T>, dim3(tiles), dim3(TK_THREADS), 0, s, d_keys_in, (const T *)ws.cand_keys, ws.state,
                             ws.hist + r * RADIX, shift, f, x); }
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(RADIX), 0, s, ws.hist + r * RADIX, ws.state, shift); }
    }
    // final ordered select
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk_count_kernel<T>, dim3(tiles), dim3(TK_THREADS), 0, s, d_keys_in, (const T *)ws.cand_keys, ws.state, ws.tilecnt,
                         f, x); }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, ws.state, ws.tilecnt); }
    if (hv) tk_launch_select<true>(s, d_keys_in, ws, tiles, kk, f, x);
    else tk_launch_select<false>(s, d_keys_in, ws, tiles, kk, f, x);
    if ((e = (int)hipGetLastError())) return e;
    // finish: the stable sort of the k staged pairs; the indices are the values of the arguments form
    uint32_t *idx_out = !hv ? nullptr : d_vals_in ? ws.idx_sorted : d_vals_out;
    if ((e = KT::sort_staged(ws, d_keys_out, idx_out, k, hv, key_type, descending, s))) return e;
    if (d_vals_in) {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_gather_kernel, dim3((kk + 255u) / 256u), dim3(256), 0, s, d_vals_in, ws.idx_sorted, d_vals_out, kk, n);
    }
    return (int)hipGetLastError();
}

template <typename KT>
static int tk_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!out || num_items >= (1ull << 32) || k > num_items) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (k == 0 || num_items == 0) return hipSuccess;   // such a call enqueued nothing
    if (!d_temp) return hipErrorInvalidValue;
    TopkWs<typename KT::T> ws;
    tk_carve<KT>(gs_ws_base(d_temp), num_items, k, has_values != 0, &ws);
    hipError_t e = hipMemcpyAsync(out, ws.state, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return (int)e;
}

// =================================================================== 64-bit keys --
// gs_topk_u64.  With eight bytes per key "everything shares the top byte" is the normal case, so the
// descent does not walk the bytes one by one over the input: every counting round over the input also reduces the AND and the
// OR of the images of its set M, the next round counts the next lower byte at which they differ (bytes constant over M are
// filled into the k-th image from the AND), and the bucket moves to the candidate list as soon as it holds at most C elements,
// at whatever byte that happens.  The launches, all enqueued whatever the data (the state block tells the workgroups of a
// launch that is not needed to return at once):
//   round one   wide_slice_count at shift 56 (the wide upsweep and the spine scan) + topk64_pick0: digit d0, count c
//   pass two    topk64_filter, one workgroup per tile: elements with top byte before d0 go to the staging area (they are
//               selected whatever follows).  c <= C (route 1, D = 1): the bucket goes to the candidate list.  Otherwise the
//               same read is round two: it reduces AND / OR over all elements (round one's M) and over the bucket (round
//               two's M), counts each of the seven lower bytes over the bucket, and stages the bucket's first elements behind
//               the others, which is the result when pick two finds every lower byte constant (route 2 at D = 1).
//   rounds 3-8  topk64_round + topk64_pick: byte j over M, AND / OR over M; pick two chooses its byte among the seven counts
//   D >= 2      topk64_count / scan / select over the input: everything of bucket d0 that sorts before the final bucket is
//               staged; the final bucket goes to the candidate list (route 1) or, cut after `take`, to the staging area
//               (route 2: no byte left, the bucket is the run of keys equal to the k-th image and longer than C)
//   route 1     seven list rounds (topk64_listhist + topk64_listpick at bytes 6 .. 0; those at or above the byte where the
//               bucket fitted return at once) and count / scan / select over the list
//   finish      gs_lsb_sort_wide of the k staged (key, index) pairs inside the workspace, the copy-out, the gather of pairs
// Passes over the input: 2 when D = 1 (either route), D + 2 otherwise.
constexpr int T6_KPT = TkKey<uint64_t>::KPT;
constexpr int T6_TILE = TK_THREADS * T6_KPT;     // 4096: W_TILE of gs_wide.hip, whose spine and prefix16 the filter reads
constexpr int T6_CHUNK = TK_WAVES;               // tiles per spine column (W_CHUNK)
// The histograms: 13 of the rounds over the input (bytes 0..6 of round two, then rounds three to eight), each in T6_COPIES
// copies -- a workgroup adds to copy blockIdx % T6_COPIES and the pick sums them -- because 65536 workgroups adding to one
// word (a byte that is constant over the array) wait for each other at that word; then the 7 of the list rounds, one copy.
constexpr int T6_COPIES = 16;
constexpr int T6_ROW_ROUND3 = 7, T6_INPUT_ROWS = 13, T6_LIST_ROWS = 7;
constexpr int T6_HIST_WORDS = (T6_INPUT_ROWS * T6_COPIES + T6_LIST_ROWS) * RADIX;
constexpr size_t T6_AO_OFF = 256, T6_HIST_OFF = 512, T6_HEAD = 221184;

// state block (u32 words): 0..7 are gs_topk_u64_status' words
enum { T6_ROUTE = 0, T6_KTH_LO = 1, T6_KTH_HI = 2, T6_LESS = 3, T6_TAKE = 4, T6_D = 5, T6_PASSES = 6, T6_MOVED = 7,
       T6_STAGED0 = 8,      // elements before digit d0: staged by the filter
       T6_D0 = 9,
       T6_ACTIVE = 10,      // the descent over the input goes on: the next round runs
       T6_J = 11,           // the byte it counts
       T6_MASK_LO = 12, T6_MASK_HI = 13,   // the bytes of the k-th image found so far (always a run of top bytes)
       T6_IN_COUNT = 14,    // num_items when D >= 2 (the count and the scatter over the input run), else 0
       T6_LIST_COUNT = 15,  // elements of the candidate list (route 1)
       T6_JFIT = 16,        // the byte at which the bucket fitted the list
       T6_STAGED1 = 17 };   // elements before the bucket: staged before the list select

static inline uint64_t tk64_tiles(uint64_t n) { const uint64_t t = (n + T6_TILE - 1) / T6_TILE; return t ? t : 1; }

__device__ __forceinline__ uint64_t t6_word64(const uint32_t *state, int lo) { return (uint64_t)state[lo] | ((uint64_t)state[lo + 1] << 32); }
// AND / OR over the 64 lanes of a wave, all of them active: four DPP row shifts leave each row's result in its lane 15 (a
// lane without a source keeps the identity), four lane reads combine the rows.  No LDS traffic; the result is wave-uniform.
template <bool AND> __device__ __forceinline__ uint32_t t6_wave_bits32(uint32_t v)
{
    constexpr int ID = AND ? -1 : 0;
    auto op = [](uint32_t p, uint32_t q) { return AND ? (p & q) : (p | q); };
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(ID, (int)v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(ID, (int)v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(ID, (int)v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(ID, (int)v, 0x118, 0xf, 0xf, false));   // row_shr:8
    return op(op((uint32_t)__builtin_amdgcn_readlane((int)v, 15), (uint32_t)__builtin_amdgcn_readlane((int)v, 31)),
              op((uint32_t)__builtin_amdgcn_readlane((int)v, 47), (uint32_t)__builtin_amdgcn_readlane((int)v, 63)));
}
__device__ __forceinline__ uint64_t t6_wave_and(uint64_t v)
{
    return (uint64_t)t6_wave_bits32<true>((uint32_t)v) | ((uint64_t)t6_wave_bits32<true>((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint64_t t6_wave_or(uint64_t v)
{
    return (uint64_t)t6_wave_bits32<false>((uint32_t)v) | ((uint64_t)t6_wave_bits32<false>((uint32_t)(v >> 32)) << 32);
}

// One workgroup's AND and OR (per-thread a, o; the identity where a thread saw nothing) into the global pair ao[0], ao[1].
// Integer atomics like the histogram adds: the result does not depend on their order.
__device__ __forceinline__ void t6_reduce_and_or(uint64_t a, uint64_t o, uint64_t (*wao)[TK_WAVES], unsigned long long *__restrict__ ao)
{
    a = t6_wave_and(a);
    o = t6_wave_or(o);
    if (lane_id() == 0) { wao[0][wave_id()] = a; wao[1][wave_id()] = o; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < TK_WAVES; ++j) { a &= wao[0][j]; o |= wao[1][j]; }
        // Every workgroup hits the same two words, so one that would change nothing stays away.  The AND only loses bits and
        // the OR only gains them, so a value read earlier -- however stale -- that the atomic would leave unchanged says
        // the same of the current one.
        const unsigned long long ca = __builtin_nontemporal_load(&ao[0]), co = __builtin_nontemporal_load(&ao[1]);
        if ((ca & a) != ca) atomicAnd(&ao[0], (unsigned long long)a);
        if ((co | o) != co) atomicOr(&ao[1], (unsigned long long)o);
    }
}

// a thread's eight keys of the tile at lo: wave w owns elements [w * 512, (w + 1) * 512) of the tile in eight coalesced rows
__device__ __forceinline__ void t6_load_rows(const uint64_t *__restrict__ src, uint32_t lo, uint32_t count, uint64_t (&raw)[T6_KPT])
{
    const uint32_t first = lo + (uint32_t)wave_id() * (uint32_t)(WAVE * T6_KPT) + (uint32_t)lane_id();
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        raw[u] = (i < count && i >= lo) ? (uint64_t)__builtin_nontemporal_load(src + i) : 0ull;
    }
}

// compact_tile for 64-bit keys that the caller has loaded with t6_load_rows: (wave, row, lane) is the input order.
template <bool IDX, typename Cls>
__device__ __forceinline__ void compact_tile64(const uint64_t (&raw)[T6_KPT], const uint32_t *__restrict__ src_idx, uint32_t lo, uint32_t count,
                                               Cls cls, uint32_t baseA, uint32_t limA, uint64_t *__restrict__ ak, uint32_t *__restrict__ ai,
                                               uint32_t baseB, uint32_t limB, uint64_t *__restrict__ bk, uint32_t *__restrict__ bi,
                                               uint32_t (*wcnt)[TK_WAVES])
{
    const uint32_t w = (uint32_t)wave_id(), lane = (uint32_t)lane_id();
    const uint32_t first = lo + w * (uint32_t)(WAVE * T6_KPT) + lane;
    uint32_t c[T6_KPT];
    uint32_t nA = 0, nB = 0;
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        c[u] = (i < count && i >= lo) ? cls(raw[u]) : 0u;
        nA += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(c[u] == 1u));
        nB += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(c[u] == 2u));
    }
    if (lane == 0) { wcnt[0][w] = nA; wcnt[1][w] = nB; }
    __syncthreads();
    uint32_t tot = 0;
    for (uint32_t j = 0; j < (uint32_t)TK_WAVES; ++j) {
        const uint32_t a = wcnt[0][j], b = wcnt[1][j];
        tot += a + b;
        if (j < w) { baseA += a; baseB += b; }
    }
    if (tot == 0) return;   // nothing of either group in this tile (workgroup-uniform)
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        const unsigned long long mA = __builtin_amdgcn_ballot_w64(c[u] == 1u), mB = __builtin_amdgcn_ballot_w64(c[u] == 2u);
        if (c[u] == 1u) {
            const uint32_t pos = baseA + count_lower(mA);
            if (pos < limA) {
                ak[pos] = raw[u];
                if (IDX) ai[pos] = src_idx ? src_idx[i] : i;
            }
        } else if (c[u] == 2u) {
            const uint32_t pos = baseB + count_lower(mB);
            if (pos < limB) {
                bk[pos] = raw[u];
                if (IDX) bi[pos] = src_idx ? src_idx[i] : i;
            }
        }
        baseA += (uint32_t)__popcll(mA);
        baseB += (uint32_t)__popcll(mB);
    }
}

// Round one's pick, one workgroup: the digit d0 whose run of S holds position k - 1.  Opens the state block, clears the
// histograms and sets the AND / OR pairs of every later round to their identities.
__global__ __launch_bounds__(RADIX) void topk64_pick0_kernel(const uint32_t *__restrict__ totals, uint32_t *__restrict__ state,
                                                             uint32_t *__restrict__ hist, unsigned long long *__restrict__ ao, uint32_t k,
                                                             uint32_t cap)
{
    __shared__ uint32_t scratch[8];
    const uint32_t t = threadIdx.x, c = totals[t];
    const uint32_t ex = block_exclusive_scan_256(c, scratch, nullptr);
    for (uint32_t i = t; i < (uint32_t)T6_HIST_WORDS; i += RADIX) hist[i] = 0;
    if (t < 18u) ao[t] = (t & 1u) ? 0ull : ~0ull;   // pair r at ao[2r]: r = 1 all elements, r = 2..8 the set of round r
    if (ex < k && k - ex <= c) {   // exactly one thread
        const bool fits = c <= cap;
        for (uint32_t i = 0; i < (uint32_t)TK_WORDS; ++i) state[i] = 0;
        state[T6_ROUTE] = fits ? 1u : 0u;   // 0: still descending
        state[T6_KTH_HI] = t << 24;
        state[T6_LESS] = ex;
        state[T6_TAKE] = k - ex;
        state[T6_D] = 1u;
        state[T6_PASSES] = 2u;
        state[T6_MOVED] = c;
        state[T6_STAGED0] = ex;
        state[T6_D0] = t;
        state[T6_ACTIVE] = fits ? 0u : 1u;
        state[T6_MASK_HI] = 0xff000000u;
        state[T6_LIST_COUNT] = fits ? c : 0u;
        state[T6_JFIT] = 7u;
        state[T6_STAGED1] = ex;
    }
}

// Pass two, one workgroup per tile of the wide upsweep.  Group A: top byte before d0 -> staging area, at the number of such
// elements in front of the tile (spine + prefix16 of round one, summed over the digits below d0).  Group B: top byte d0, at
// spine[d0] + prefix16[d0] -> candidate list (route 1), or behind group A's total in the staging area while the descent goes
// on.  Then it is round two as well: AND / OR over every element into ao[2..3] and over the bucket into ao[4..5], and the
// counts of bytes 0..6 over the bucket into hist rows 0..6.
template <bool IDX>
__global__ __launch_bounds__(TK_THREADS) void topk64_filter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ spine,
                                                                   const uint16_t *__restrict__ prefix16, const uint32_t *__restrict__ state,
                                                                   uint32_t *__restrict__ hist, unsigned long long *__restrict__ ao,
                                                                   uint64_t *__restrict__ stage_keys, uint32_t *__restrict__ stage_idx,
                                                                   uint64_t *__restrict__ cand_keys, uint32_t *__restrict__ cand_idx, uint32_t n,
                                                                   uint32_t grid, uint32_t k, uint32_t cap, int f, uint64_t x)
{
    __shared__ uint32_t wcnt[2][TK_WAVES];
    __shared__ uint32_t wsum[TK_WAVES];
    __shared__ uint32_t cbase;
    __shared__ uint32_t h[7 * RADIX];
    __shared__ uint64_t wao[2][TK_WAVES];
    const uint32_t tile = blockIdx.x, chunk = tile / (uint32_t)T6_CHUNK, tid = threadIdx.x;
    const uint32_t d0 = state[T6_D0], staged0 = state[T6_STAGED0];
    const bool list = state[T6_ROUTE] == 1u;
    uint32_t below = 0;
    if (tid <= d0) {   // d0 < 256: only the digits that count are read
        const uint32_t v = spine[(size_t)tid * grid + chunk] + prefix16[(size_t)tile * RADIX + tid];
        if (tid < d0) below = v;
        if (tid == d0) cbase = v;
    }
    below = wave_reduce_sum(below);
    if (lane_id() == 0) wsum[wave_id()] = below;
    if (!list)
        for (uint32_t i = tid; i < 7u * RADIX; i += TK_THREADS) h[i] = 0;
    __syncthreads();
    uint32_t baseA = 0;
    for (int j = 0; j < TK_WAVES; ++j) baseA += wsum[j];
    const uint32_t lo = tile * (uint32_t)T6_TILE;
    uint64_t raw[T6_KPT];
    t6_load_rows(keys, lo, n, raw);
    auto cls = [&](uint64_t r) -> uint32_t {
        const uint32_t tb = (uint32_t)(TkKey<uint64_t>::image(r, f, x) >> 56);
        return tb < d0 ? 1u : tb == d0 ? 2u : 0u;
    };
    compact_tile64<IDX>(raw, (const uint32_t *)nullptr, lo, n, cls, baseA, k, stage_keys, stage_idx, list ? cbase : staged0 + cbase,
                        list ? cap : k, list ? cand_keys : stage_keys, list ? cand_idx : stage_idx, wcnt);
    if (list) return;   // (workgroup-uniform)
    const uint32_t first = lo + (uint32_t)wave_id() * (uint32_t)(WAVE * T6_KPT) + (uint32_t)lane_id();
    uint64_t a_all = ~0ull, o_all = 0ull, a_b = ~0ull, o_b = 0ull;
    uint32_t inb = 0, nb = 0;   // bit u: element u is in the bucket
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        if (i < n && i >= lo) {
            const uint64_t img = TkKey<uint64_t>::image(raw[u], f, x);
            a_all &= img; o_all |= img;
            if ((uint32_t)(img >> 56) == d0) { a_b &= img; o_b |= img; inb |= 1u << u; ++nb; }
        }
    }
    // A byte that is constant over the wave's bucket elements -- the usual case for the bytes this pass exists to skip -- is
    // counted by one add of their number; only the others go through the per-element increments.
    const uint64_t wa = t6_wave_and(a_b), wdiff = wa ^ t6_wave_or(o_b);
    const uint32_t wn = wave_reduce_sum(nb);
    if (wn) {
#pragma unroll
        for (int b = 0; b < 7; ++b) {
            if (((wdiff >> (8 * b)) & 255ull) == 0ull) {   // (wave-uniform)
                if (lane_id() == 0) atomicAdd(&h[b * RADIX + ((uint32_t)(wa >> (8 * b)) & 255u)], wn);
            } else {
#pragma unroll
                for (int u = 0; u < T6_KPT; ++u)
                    if (inb & (1u << u)) hist_add(h + b * RADIX, (uint32_t)(TkKey<uint64_t>::image(raw[u], f, x) >> (8 * b)) & 255u);
            }
        }
    }
    t6_reduce_and_or(a_all, o_all, wao, ao + 2);
    __syncthreads();
    t6_reduce_and_or(a_b, o_b, wao, ao + 4);
    const uint32_t copy = blockIdx.x % (uint32_t)T6_COPIES;
    for (uint32_t i = tid; i < 7u * RADIX; i += TK_THREADS)   // row i / 256, digit i % 256
        if (h[i]) atomicAdd(&hist[((i >> RADIX_BITS) * (uint32_t)T6_COPIES + copy) * (uint32_t)RADIX + (i & (uint32_t)(RADIX - 1))], h[i]);
}

// Rounds three to eight over the input: the counts of byte state[T6_J] over M -- the elements whose image agrees with the
// k-th image on the bytes found so far -- and the AND / OR of the images of M.
__global__ __launch_bounds__(TK_THREADS) void topk64_round_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ state,
                                                                  uint32_t *__restrict__ hist, unsigned long long *__restrict__ ao, uint32_t n,
                                                                  int f, uint64_t x)
{
    __shared__ uint32_t h[RADIX];
    __shared__ uint64_t wao[2][TK_WAVES];
    if (state[T6_ACTIVE] == 0u) return;
    const uint32_t lo = blockIdx.x * (uint32_t)T6_TILE, tid = threadIdx.x;
    const uint32_t shift = 8u * state[T6_J];
    const uint64_t prefix = t6_word64(state, T6_KTH_LO), mask = t6_word64(state, T6_MASK_LO);
    if (tid < (uint32_t)RADIX) h[tid] = 0;
    __syncthreads();
    uint64_t raw[T6_KPT];
    t6_load_rows(keys, lo, n, raw);
    const uint32_t first = lo + (uint32_t)wave_id() * (uint32_t)(WAVE * T6_KPT) + (uint32_t)lane_id();
    uint64_t a = ~0ull, o = 0ull;
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        const uint64_t img = TkKey<uint64_t>::image(raw[u], f, x);
        if (i < n && i >= lo && ((img ^ prefix) & mask) == 0ull) {
            a &= img; o |= img;
            hist_add(h, (uint32_t)(img >> shift) & 255u);
        }
    }
    t6_reduce_and_or(a, o, wao, ao);
    if (tid < (uint32_t)RADIX && h[tid]) atomicAdd(&hist[(blockIdx.x % (uint32_t)T6_COPIES) * (uint32_t)RADIX + tid], h[tid]);
}

// The pick of round r = 2..8, one workgroup.  ao_prev: AND / OR of round r - 1's set (read by pick two, which has to find its
// byte first: hist then holds the seven rows of pass two); ao_cur: those of round r's set, which choose the next byte.
__global__ __launch_bounds__(RADIX) void topk64_pick_kernel(uint32_t *__restrict__ state, const uint32_t *__restrict__ hist,
                                                            const unsigned long long *__restrict__ ao_prev,
                                                            const unsigned long long *__restrict__ ao_cur, uint32_t r, uint32_t n, uint32_t cap)
{
    __shared__ uint32_t scratch[8];
    if (state[T6_ACTIVE] == 0u) return;   // (workgroup-uniform: the state is written behind a barrier)
    const uint32_t t = threadIdx.x;
    uint64_t prefix = t6_word64(state, T6_KTH_LO), mask = t6_word64(state, T6_MASK_LO);
    const uint32_t krem = state[T6_TAKE], less = state[T6_LESS];
    uint32_t j = state[T6_J];
    if (r == 2u) {
        const uint64_t a = ao_prev[0], o = ao_prev[1], diff = (a ^ o) & ~mask;
        if (diff == 0ull) {
            // every byte below the top one is constant over the array: the bucket is the run of keys equal to the k-th image,
            // and pass two has staged its first elements (route 2 at D = 1)
            __syncthreads();
            if (t == 0) {
                prefix |= a & ~mask;
                state[T6_KTH_LO] = (uint32_t)prefix; state[T6_KTH_HI] = (uint32_t)(prefix >> 32);
                state[T6_MASK_LO] = 0xffffffffu; state[T6_MASK_HI] = 0xffffffffu;
                state[T6_ROUTE] = 2u;
                state[T6_ACTIVE] = 0u;
            }
            return;
        }
        j = (uint32_t)(63 - __builtin_clzll(diff)) >> 3;
        const uint64_t fill = ~mask & ~((1ull << (8u * (j + 1u))) - 1ull);   // the constant bytes between
        prefix |= a & fill;
        mask |= fill;
    }
    uint32_t c = 0;
    for (uint32_t cp = 0; cp < (uint32_t)T6_COPIES; ++cp) c += hist[((r == 2u ? j : 0u) * (uint32_t)T6_COPIES + cp) * (uint32_t)RADIX + t];
    const uint32_t ex = block_exclusive_scan_256(c, scratch, nullptr);   // (its barriers order the reads above before the writes below)
    if (ex < krem && krem - ex <= c) {
        prefix |= (uint64_t)t << (8u * j);
        mask |= 0xffull << (8u * j);
        state[T6_LESS] = less + ex;
        state[T6_TAKE] = krem - ex;
        state[T6_D] = r;
        state[T6_PASSES] = r + 2u;
        state[T6_MOVED] = c;
        if (c <= cap) {
            state[T6_ROUTE] = 1u;
            state[T6_ACTIVE] = 0u;
            state[T6_IN_COUNT] = n;
            state[T6_LIST_COUNT] = c;
            state[T6_JFIT] = j;
            state[T6_STAGED1] = less + ex;
        } else {
            const uint64_t a = ao_cur[0], o = ao_cur[1], diff = (a ^ o) & ~mask;
            if (diff == 0ull) {   // no byte left: the bucket is the tie run, longer than the list
                prefix |= a & ~mask;
                mask = ~0ull;
                state[T6_ROUTE] = 2u;
                state[T6_ACTIVE] = 0u;
                state[T6_IN_COUNT] = n;
            } else {
                const uint32_t jn = (uint32_t)(63 - __builtin_clzll(diff)) >> 3;
                const uint64_t fill = ~mask & ~((1ull << (8u * (jn + 1u))) - 1ull);
                prefix |= a & fill;
                mask |= fill;
                state[T6_J] = jn;
            }
        }
        state[T6_KTH_LO] = (uint32_t)prefix; state[T6_KTH_HI] = (uint32_t)(prefix >> 32);
        state[T6_MASK_LO] = (uint32_t)mask; state[T6_MASK_HI] = (uint32_t)(mask >> 32);
    }
}

// A list round at byte b: the counts of byte b over the list's elements that agree with the k-th image above it.
__global__ __launch_bounds__(TK_THREADS) void topk64_listhist_kernel(const uint64_t *__restrict__ cand_keys, const uint32_t *__restrict__ state,
                                                                     uint32_t *__restrict__ hist, uint32_t b, int f, uint64_t x)
{
    __shared__ uint32_t h[RADIX];
    if (state[T6_ROUTE] != 1u || b >= state[T6_JFIT]) return;
    const uint32_t count = state[T6_LIST_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * T6_TILE;
    if (lo64 >= count) return;
    const uint32_t lo = (uint32_t)lo64, tid = threadIdx.x;
    const uint64_t prefix = t6_word64(state, T6_KTH_LO);
    if (tid < (uint32_t)RADIX) h[tid] = 0;
    __syncthreads();
    uint64_t raw[T6_KPT];
    t6_load_rows(cand_keys, lo, count, raw);
    const uint32_t first = lo + (uint32_t)wave_id() * (uint32_t)(WAVE * T6_KPT) + (uint32_t)lane_id();
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        const uint64_t img = TkKey<uint64_t>::image(raw[u], f, x);
        if (i < count && i >= lo && ((img ^ prefix) >> (8u * (b + 1u))) == 0ull) hist_add(h, (uint32_t)(img >> (8u * b)) & 255u);
    }
    __syncthreads();
    if (tid < (uint32_t)RADIX && h[tid]) atomicAdd(&hist[tid], h[tid]);
}

__global__ __launch_bounds__(RADIX) void topk64_listpick_kernel(const uint32_t *__restrict__ hist, uint32_t *__restrict__ state, uint32_t b)
{
    __shared__ uint32_t scratch[8];
    if (state[T6_ROUTE] != 1u || b >= state[T6_JFIT]) return;
    const uint32_t t = threadIdx.x, c = hist[t];
    const uint32_t krem = state[T6_TAKE], less = state[T6_LESS];
    const uint64_t kth = t6_word64(state, T6_KTH_LO);
    const uint32_t ex = block_exclusive_scan_256(c, scratch, nullptr);
    if (ex < krem && krem - ex <= c) {
        const uint64_t v = kth | ((uint64_t)t << (8u * b));
        state[T6_KTH_LO] = (uint32_t)v; state[T6_KTH_HI] = (uint32_t)(v >> 32);
        state[T6_LESS] = less + ex;
        state[T6_TAKE] = krem - ex;
    }
}

// The ordered select, over the input (LIST false: D >= 2) or over the candidate list.  Group A: the elements of bucket d0 that
// sort before the bucket found (input) or before the k-th image (list); group B: the bucket's elements (input) or the elements
// equal to the k-th image (list).  count: both numbers per source tile.
template <bool LIST>
__global__ __launch_bounds__(TK_THREADS) void topk64_count_kernel(const uint64_t *__restrict__ src, const uint32_t *__restrict__ state,
                                                                  uint32_t *__restrict__ tilecnt, int f, uint64_t x)
{
    __shared__ uint32_t wl[TK_WAVES], we[TK_WAVES];
    const uint32_t count = state[LIST ? T6_LIST_COUNT : T6_IN_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * T6_TILE;
    if (lo64 >= count) return;
    const uint32_t lo = (uint32_t)lo64, tid = threadIdx.x;
    const uint64_t kth = t6_word64(state, T6_KTH_LO), mask = LIST ? ~0ull : t6_word64(state, T6_MASK_LO), d0 = state[T6_D0];
    uint64_t raw[T6_KPT];
    t6_load_rows(src, lo, count, raw);
    const uint32_t first = lo + (uint32_t)wave_id() * (uint32_t)(WAVE * T6_KPT) + (uint32_t)lane_id();
    uint32_t l = 0, e = 0;
#pragma unroll
    for (int u = 0; u < T6_KPT; ++u) {
        const uint32_t i = first + (uint32_t)u * WAVE;
        const uint64_t img = TkKey<uint64_t>::image(raw[u], f, x);
        const bool ok = i < count && i >= lo;
        l += (ok && (img >> 56) == d0 && (img & mask) < (kth & mask)) ? 1u : 0u;
        e += (ok && ((img ^ kth) & mask) == 0ull) ? 1u : 0u;
    }
    l = wave_reduce_sum(l);
    e = wave_reduce_sum(e);
    if (lane_id() == 0) { wl[wave_id()] = l; we[wave_id()] = e; }
    __syncthreads();
    if (tid == 0) {
        uint32_t sl = 0, se = 0;
        for (int j = 0; j < TK_WAVES; ++j) { sl += wl[j]; se += we[j]; }
        tilecnt[2u * blockIdx.x] = sl;
        tilecnt[2u * blockIdx.x + 1u] = se;
    }
}

// scan: topk_scan_kernel over tiles of 4096 elements, the source's count in state[word]
__global__ __launch_bounds__(TK_SCAN_THREADS) void topk64_scan_kernel(const uint32_t *__restrict__ state, uint32_t *__restrict__ tilecnt, uint32_t word)
{
    __shared__ uint32_t wsl[TK_SCAN_THREADS / WAVE], wse[TK_SCAN_THREADS / WAVE];
    const uint32_t count = state[word];
    const uint32_t tiles = (uint32_t)(((uint64_t)count + T6_TILE - 1) / T6_TILE);
    const int w = wave_id(), lane = lane_id();
    uint32_t carry_l = 0, carry_e = 0;
    for (uint32_t base = 0; base < tiles; base += TK_SCAN_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t l = i < tiles ? tilecnt[2u * i] : 0u, e = i < tiles ? tilecnt[2u * i + 1u] : 0u;
        const uint32_t il = wave_inclusive_scan(l), ie = wave_inclusive_scan(e);
        if (lane == 63) { wsl[w] = il; wse[w] = ie; }
        __syncthreads();
        uint32_t bl = 0, be = 0, tl = 0, te = 0;
        for (int j = 0; j < TK_SCAN_THREADS / WAVE; ++j) {
            const uint32_t a = wsl[j], b = wse[j];
            if (j < w) { bl += a; be += b; }
            tl += a; te += b;
        }
        if (i < tiles) {
            tilecnt[2u * i] = carry_l + bl + il - l;
            tilecnt[2u * i + 1u] = carry_e + be + ie - e;
        }
        carry_l += tl; carry_e += te;
        __syncthreads();
    }
}

// scatter.  Input: group A behind the filter's elements in the staging area; group B to the candidate list (route 1) or, cut
// after `take`, behind everything that sorts before it (route 2).  List: group A behind the elements staged before the bucket,
// group B behind everything that sorts before the k-th image, cut after `take`.
template <bool IDX, bool LIST>
__global__ __launch_bounds__(TK_THREADS) void topk64_select_kernel(const uint64_t *__restrict__ src, const uint32_t *__restrict__ src_idx,
                                                                   const uint32_t *__restrict__ state, const uint32_t *__restrict__ tilecnt,
                                                                   uint64_t *__restrict__ stage_keys, uint32_t *__restrict__ stage_idx,
                                                                   uint64_t *__restrict__ cand_keys, uint32_t *__restrict__ cand_idx, uint32_t k,
                                                                   uint32_t cap, int f, uint64_t x)
{
    __shared__ uint32_t wcnt[2][TK_WAVES];
    const uint32_t count = state[LIST ? T6_LIST_COUNT : T6_IN_COUNT];
    const uint64_t lo64 = (uint64_t)blockIdx.x * T6_TILE;
    if (lo64 >= count) return;
    const uint32_t lo = (uint32_t)lo64;
    const uint64_t kth = t6_word64(state, T6_KTH_LO), mask = LIST ? ~0ull : t6_word64(state, T6_MASK_LO), d0 = state[T6_D0];
    const bool to_list = !LIST && state[T6_ROUTE] == 1u;
    const uint32_t baseA = state[LIST ? T6_STAGED1 : T6_STAGED0] + tilecnt[2u * blockIdx.x];
    const uint32_t baseB = (to_list ? 0u : state[T6_LESS]) + tilecnt[2u * blockIdx.x + 1u];
    uint64_t raw[T6_KPT];
    t6_load_rows(src, lo, count, raw);
    auto cls = [&](uint64_t r) -> uint32_t {
        const uint64_t img = TkKey<uint64_t>::image(r, f, x);
        return ((img ^ kth) & mask) == 0ull ? 2u : ((img >> 56) == d0 && (img & mask) < (kth & mask)) ? 1u : 0u;
    };
    compact_tile64<IDX>(raw, src_idx, lo, count, cls, baseA, k, stage_keys, stage_idx, baseB, to_list ? cap : k, to_list ? cand_keys : stage_keys,
                        to_list ? cand_idx : stage_idx, wcnt);
}

// the sorted pairs leave the workspace
__global__ __launch_bounds__(256) void topk64_copy_kernel(const uint64_t *__restrict__ sk, const uint32_t *__restrict__ sv,
                                                          uint64_t *__restrict__ keys_out, uint32_t *__restrict__ vals_out, uint32_t k)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k) return;
    keys_out[i] = sk[i];
    if (vals_out) vals_out[i] = sv[i];
}

// ----------------------------------------------------------------------- host --
// The width's description, as TkKeys32 / TkKeys16 above; the plan itself (tk64_run) is its own: the launches differ.
namespace {
struct TkKeys64 {
    using T = uint64_t;
    static bool type_ok(int key_type) { return key_type >= GS_KEY_U64 && key_type <= GS_KEY_F64; }
    static void twiddle(int key_type, int descending, int *f, uint64_t *x)
    {
        *f = key_type == GS_KEY_F64 ? 1 : 0;
        *x = (key_type == GS_KEY_I64 ? 0x8000000000000000ull : 0ull) ^ (descending ? ~0ull : 0ull);
    }
    static size_t sort_temp_bytes(uint64_t k, bool hv) { return gs_lsb_wide_temp_bytes(k, 8, hv ? 4 : 0); }
};

struct Topk64Ws {
    uint32_t *state, *hist;
    unsigned long long *ao;
    uint32_t *spine, *totals;
    uint16_t *prefix16;
    uint32_t *tilecnt;
    uint64_t *cand_keys;
    uint32_t *cand_idx;
    uint64_t *stage_keys[2];     // the staged keys and the other buffer of their sort
    uint32_t *stage_idx[2];
    char *sort_ws;
    size_t sort_ws_bytes;
};
}  // namespace

static size_t tk64_carve(char *base, uint64_t n, uint64_t k, bool hv, Topk64Ws *ws)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = (char *)((uintptr_t)base + off); off += gs_ws_align(bytes); return p; };
    size_t spine_bytes, prefix_bytes;
    wide_slice_bytes(n, spine_bytes, prefix_bytes);
    char *head = take(T6_HEAD);
    char *spine = take(spine_bytes);
    char *totals = take(RADIX * 4);
    char *prefix16 = take(prefix_bytes);
    char *tilecnt = take((size_t)8 * tk64_tiles(n));
    char *ck = take((size_t)8 * tk_cand_cap(n));
    char *ci = hv ? take((size_t)4 * tk_cand_cap(n)) : nullptr;
    char *sk0 = take((size_t)8 * k);
    char *sk1 = take((size_t)8 * k);
    char *si0 = hv ? take((size_t)4 * k) : nullptr;
    char *si1 = hv ? take((size_t)4 * k) : nullptr;
    const size_t sort_bytes = TkKeys64::sort_temp_bytes(k, hv);
    char *sw = take(sort_bytes);
    if (ws) {
        ws->state = (uint32_t *)head; ws->ao = (unsigned long long *)(head + T6_AO_OFF); ws->hist = (uint32_t *)(head + T6_HIST_OFF);
        ws->spine = (uint32_t *)spine; ws->totals = (uint32_t *)totals; ws->prefix16 = (uint16_t *)prefix16;
        ws->tilecnt = (uint32_t *)tilecnt; ws->cand_keys = (uint64_t *)ck; ws->cand_idx = (uint32_t *)ci;
        ws->stage_keys[0] = (uint64_t *)sk0; ws->stage_keys[1] = (uint64_t *)sk1;
        ws->stage_idx[0] = (uint32_t *)si0; ws->stage_idx[1] = (uint32_t *)si1;
        ws->sort_ws = sw; ws->sort_ws_bytes = sort_bytes;
    }
    return off;
}
static_assert(T6_HIST_OFF + (size_t)T6_HIST_WORDS * 4 <= T6_HEAD && T6_HEAD % 256 == 0, "the histograms fit the head");

static size_t tk64_temp_bytes(uint64_t num_items, uint64_t k, int has_values)
{
    if (k == 0 || num_items == 0) return 0;
    return tk64_carve(nullptr, num_items, k, has_values != 0, nullptr) + GS_WS_SLACK;
}

template <bool IDX>
static void tk64_launch_indexed(hipStream_t s, const uint64_t *keys_in, const Topk64Ws &ws, uint32_t n, uint32_t tiles, uint32_t grid,
                                uint32_t list_tiles, uint32_t k, uint32_t cap, int f, uint64_t x, int which)
{
    KernelTimer kt(GS_K_OTHER, s);
    if (which == 0)
        hipLaunchKernelGGL(topk64_filter_kernel<IDX>, dim3(tiles), dim3(TK_THREADS), 0, s, keys_in, (const uint32_t *)ws.spine,
                           (const uint16_t *)ws.prefix16, (const uint32_t *)ws.state, ws.hist, ws.ao, ws.stage_keys[0], ws.stage_idx[0],
                           ws.cand_keys, ws.cand_idx, n, grid, k, cap, f, x);
    else if (which == 1)
        hipLaunchKernelGGL((topk64_select_kernel<IDX, false>), dim3(tiles), dim3(TK_THREADS), 0, s, keys_in, (const uint32_t *)nullptr,
                           (const uint32_t *)ws.state, (const uint32_t *)ws.tilecnt, ws.stage_keys[0], ws.stage_idx[0], ws.cand_keys,
                           ws.cand_idx, k, cap, f, x);
    else
        hipLaunchKernelGGL((topk64_select_kernel<IDX, true>), dim3(list_tiles), dim3(TK_THREADS), 0, s, (const uint64_t *)ws.cand_keys,
                           (const uint32_t *)ws.cand_idx, (const uint32_t *)ws.state, (const uint32_t *)ws.tilecnt, ws.stage_keys[0],
                           ws.stage_idx[0], ws.cand_keys, ws.cand_idx, k, cap, f, x);
}

static int tk64_run(void *d_temp, size_t temp_bytes, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t *d_keys_out,
                    uint32_t *d_vals_out, uint64_t num_items, uint64_t k, int descending, int key_type, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (num_items >= (1ull << 32) || k > num_items) return hipErrorInvalidValue;
    if (!TkKeys64::type_ok(key_type)) return hipErrorInvalidValue;
    if (d_vals_in && !d_vals_out) return hipErrorInvalidValue;
    if (k == 0 || num_items == 0) return hipSuccess;
    const bool hv = d_vals_out != nullptr;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < tk64_temp_bytes(num_items, k, hv)) return hipErrorInvalidValue;
    if ((((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & 7u) != 0 || (((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & 3u) != 0)
        return hipErrorInvalidValue;
    {
        const void *arr[4] = {d_keys_in, d_vals_in, d_keys_out, d_vals_out};
        const size_t bytes[4] = {(size_t)num_items * 8, (size_t)num_items * 4, (size_t)k * 8, (size_t)k * 4};
        if (gs_any_overlap4(arr, bytes)) return hipErrorInvalidValue;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)num_items, kk = (uint32_t)k;
    Topk64Ws ws;
    tk64_carve(gs_ws_base(d_temp), num_items, k, hv, &ws);
    int f, e;
    uint64_t x;
    TkKeys64::twiddle(key_type, descending, &f, &x);
    const uint32_t tiles = (uint32_t)tk64_tiles(num_items), grid = (tiles + T6_CHUNK - 1) / T6_CHUNK;
    const uint32_t cap = (uint32_t)tk_cand_cap(num_items);
    const uint32_t list_tiles = (uint32_t)tk64_tiles(cap < num_items ? cap : num_items);
    const uint32_t *state = ws.state;

    // round one: the wide upsweep on the top byte of the image, the spine scan, the pick
    const LargeDigit dg = {56, 8, key_type, descending ? 1 : 0, true, true};
    if ((e = wide_slice_count(d_keys_in, num_items, 8, dg, ws.spine, ws.prefix16, ws.totals, s))) return e;
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_pick0_kernel, dim3(1), dim3(RADIX), 0, s, (const uint32_t *)ws.totals, ws.state, ws.hist, ws.ao, kk, cap); }
    // pass two: the filter, and round two when the bucket does not fit
    if (hv) tk64_launch_indexed<true>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 0);
    else tk64_launch_indexed<false>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 0);
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_pick_kernel, dim3(1), dim3(RADIX), 0, s, ws.state, (const uint32_t *)ws.hist,
                         (const unsigned long long *)(ws.ao + 2), (const unsigned long long *)(ws.ao + 4), 2u, n, cap); }
    // rounds three to eight
    for (uint32_t r = 3; r <= 8; ++r) {
        uint32_t *hist = ws.hist + (T6_ROW_ROUND3 + (r - 3u)) * T6_COPIES * RADIX;
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk64_round_kernel, dim3(tiles), dim3(TK_THREADS), 0, s, d_keys_in, state, hist, ws.ao + 2u * r, n, f, x); }
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk64_pick_kernel, dim3(1), dim3(RADIX), 0, s, ws.state, (const uint32_t *)hist,
                             (const unsigned long long *)(ws.ao + 2u * (r - 1u)), (const unsigned long long *)(ws.ao + 2u * r), r, n, cap); }
    }
    // D >= 2: the count and the scatter over the input
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_count_kernel<false>, dim3(tiles), dim3(TK_THREADS), 0, s, d_keys_in, state, ws.tilecnt, f, x); }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, state, ws.tilecnt, (uint32_t)T6_IN_COUNT); }
    if (hv) tk64_launch_indexed<true>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 1);
    else tk64_launch_indexed<false>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 1);
    // route 1: the bytes below the one where the bucket fitted, over the list; the ordered select over the list
    for (int b = 6; b >= 0; --b) {
        uint32_t *hist = ws.hist + (T6_INPUT_ROWS * T6_COPIES + b) * RADIX;
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk64_listhist_kernel, dim3(list_tiles), dim3(TK_THREADS), 0, s, (const uint64_t *)ws.cand_keys, state, hist,
                             (uint32_t)b, f, x); }
        { KernelTimer kt(GS_K_OTHER, s);
          hipLaunchKernelGGL(topk64_listpick_kernel, dim3(1), dim3(RADIX), 0, s, (const uint32_t *)hist, ws.state, (uint32_t)b); }
    }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_count_kernel<true>, dim3(list_tiles), dim3(TK_THREADS), 0, s, (const uint64_t *)ws.cand_keys, state, ws.tilecnt,
                         f, x); }
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_scan_kernel, dim3(1), dim3(TK_SCAN_THREADS), 0, s, state, ws.tilecnt, (uint32_t)T6_LIST_COUNT); }
    if (hv) tk64_launch_indexed<true>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 2);
    else tk64_launch_indexed<false>(s, d_keys_in, ws, n, tiles, grid, list_tiles, kk, cap, f, x, 2);
    if ((e = (int)hipGetLastError())) return e;
    // finish: the stable sort of the k staged pairs (eight passes: the result is back in the first buffer), the copy-out
    void *sort_keys[2] = {ws.stage_keys[0], ws.stage_keys[1]}, *sort_vals[2] = {ws.stage_idx[0], ws.stage_idx[1]};
    int sel = 0;
    if ((e = gs_lsb_sort_wide(ws.sort_ws, ws.sort_ws_bytes, sort_keys, hv ? sort_vals : nullptr, &sel, k, 8, hv ? 4 : 0, 0, 64, descending,
                              key_type, s)))
        return e;
    { KernelTimer kt(GS_K_OTHER, s);
      hipLaunchKernelGGL(topk64_copy_kernel, dim3((kk + 255u) / 256u), dim3(256), 0, s, (const uint64_t *)sort_keys[sel],
                         (const uint32_t *)(hv && !d_vals_in ? sort_vals[sel] : nullptr), d_keys_out, d_vals_in ? nullptr : d_vals_out, kk); }
    if (d_vals_in) {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(topk_gather_kernel, dim3((kk + 255u) / 256u), dim3(256), 0, s, d_vals_in, (const uint32_t *)sort_vals[sel], d_vals_out,
                           kk, n);
    }
    return (int)hipGetLastError();
}

static int tk64_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!out || num_items >= (1ull << 32) || k > num_items) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (k == 0 || num_items == 0) return hipSuccess;   // such a call enqueued nothing
    if (!d_temp) return hipErrorInvalidValue;
    Topk64Ws ws;
    tk64_carve(gs_ws_base(d_temp), num_items, k, has_values != 0, &ws);
    hipError_t e = hipMemcpyAsync(out, ws.state, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return (int)e;
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_topk_temp_bytes(uint64_t num_items, uint64_t k, int has_values) { return tk_temp_bytes<TkKeys32>(num_items, k, has_values); }

size_t gs_topk_u16_temp_bytes(uint64_t num_items, uint64_t k, int has_values) { return tk_temp_bytes<TkKeys16>(num_items, k, has_values); }

int gs_topk_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in, const uint32_t *d_vals_in, uint32_t *d_keys_out,
                uint32_t *d_vals_out, uint64_t num_items, uint64_t k, int descending, int key_type, void *stream)
{
    return tk_run<TkKeys32>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_items, k, descending, key_type, stream);
}

int gs_topk_u16(void *d_temp, size_t temp_bytes, const uint16_t *d_keys_in, const uint32_t *d_vals_in, uint16_t *d_keys_out,
                uint32_t *d_vals_out, uint64_t num_items, uint64_t k, int descending, int key_type, void *stream)
{
    return tk_run<TkKeys16>(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_items, k, descending, key_type, stream);
}

int gs_topk_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    return tk_status<TkKeys32>(d_temp, num_items, k, has_values, out, stream);
}

int gs_topk_u16_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    return tk_status<TkKeys16>(d_temp, num_items, k, has_values, out, stream);
}

size_t gs_topk_u64_temp_bytes(uint64_t num_items, uint64_t k, int has_values) { return tk64_temp_bytes(num_items, k, has_values); }

int gs_topk_u64(void *d_temp, size_t temp_bytes, const uint64_t *d_keys_in, const uint32_t *d_vals_in, uint64_t *d_keys_out,
                uint32_t *d_vals_out, uint64_t num_items, uint64_t k, int descending, int key_type, void *stream)
{
    return tk64_run(d_temp, temp_bytes, d_keys_in, d_vals_in, d_keys_out, d_vals_out, num_items, k, descending, key_type, stream);
}

int gs_topk_u64_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream)
{
    return tk64_status(d_temp, num_items, k, has_values, out, stream);
}

}  // extern "C"
