// gs_topk_rows.inc -- what gs_topk_rows.hip (32-bit keys) and gs_topk_rows_narrow.hip (16-bit keys) share: the geometry, the
// wave sort and the workgroup's radix select with a compile-time key width, the compaction of the selected elements, and the
// host's plan (DESIGN.md sections 10h and 10i).  Include after gs_device.hpp
// and gs_host.hpp.  One geometry and one plan for both entry points: gs_topk_rows_plan answers for both.
#pragma once

namespace gs {

constexpr int TR_THREADS = 512;                  // 8 waves
constexpr int TR_WAVES = TR_THREADS / WAVE;
constexpr int TR_KPT = 16;
constexpr uint32_t TR_CH = TR_THREADS * TR_KPT;  // 8192: the elements one workgroup selects from
constexpr uint32_t TR_MAX_K = 1024;              // what one wave sorts: 16 per lane
constexpr uint32_t TR_WAVE_COLS = 1024;          // longest row of path 1
static_assert(TR_MAX_K <= TR_CH && TR_MAX_K == 16 * WAVE, "a chunk gives up to k sorted by one wave");

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

static inline size_t tr_align(size_t x) { return (x + 255) & ~(size_t)255; }

static inline bool tr_overlaps(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    if (!a || !b || !abytes || !bbytes) return false;
    const char *p = (const char *)a, *q = (const char *)b;
    return p < q + bbytes && q < p + abytes;
}

}  // namespace gs
