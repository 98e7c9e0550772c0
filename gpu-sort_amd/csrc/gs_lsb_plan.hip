// gs_lsb_plan.hip -- the keys-only plan of gs_lsb_sort_u32: full-width 32-bit keys without values are sorted by two
// scatter passes and one in-LDS local sort per group of equal top 16 bits, where the data allows it, and by the four
// passes where it does not -- decided on the device, with one fixed launch sequence.  A translation unit of its own: the
// pass slots are new instantiations of the upsweep / downsweep code (gs_lsb_upsweep.inc, gs_lsb_downsweep.inc), and the
// kernels of gs_lsb.hip compile exactly as they did without it.
#include "gs_device.hpp"
#include "gs_lsb.hpp"
#include "gs_msb_tasks.hpp"
#ifndef GS_PLAN_N_MIN
#define GS_PLAN_N_MIN (1ull << 28)
#endif
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace gs {

#include "gs_lsb_upsweep.inc"

#include "gs_lsb_downsweep.inc"

// --------------------------------------------------------- keys-only plan --
// A full-width keys-only sort needs no four stable scatters: equal keys are indistinguishable.  Two stable scatters on the
// top two bytes leave 65536 groups of equal top 16 bits, each of which one local sort (gs_msb.hip) finishes on its low 16
// bits in LDS: 24 + 8 B/key through HBM instead of 48.  That only works while every group fits the largest local sort, and
// the sort may neither wait on the host nor change its launches with the data.  So:
//   look      one read of the input: the exact histogram of the top 16 bits of the twiddled keys (lsb_plan_look_kernel:
//             a table of 65536 16-bit counters in LDS per workgroup, partial tables in the alternate key buffer, which is
//             free until the first scatter; lsb_plan_reduce_kernel sums them; lsb_plan_decide_kernel writes the PlanBlock).
//             The same read counts bits 16-23 per tile and leaves the spine and prefix16 of the first PLANNED scatter;
//   slots     the usual four passes, as kernels that take their digit position from the PlanBlock: shifts 16, 24, skip,
//             skip when PLANNED, 0, 8, 16, 24 when CLASSIC (a group above the cap).  A skipped slot's blocks return at once,
//             and so do those of slot 1's upsweep when PLANNED: the look has done its work;
//   finish    lsb_plan_tasks_kernel turns the group table into the local sorts' task lists (nothing when CLASSIC), and the
//             local sorts run in place over worst-case grids: with empty lists their blocks exit.
//   peek      that fixed sequence pays for both routes.  Outside stream capture the host reads the decision while the first
//             slot runs and enqueues only what the route needs (see PlanPeek below); GS_LSB_PLAN_PEEK=0 keeps the fixed sequence.
// The buffer ping-pong is the four passes' on both routes, so the selector and the result buffer do not depend on the route.
//   cursors   the finish sorts every group, so the second PLANNED scatter need not be stable: it only has to put every key
//             into the range of its group, which the look knows exactly (offsets[]).  So it has no upsweep: a tile claims
//             count(d2) places in group (d2, d1) with one returning add per d2 on a table of cursors (downsweep_tile's
//             CURSOR mode), which the launch that would have been the upsweep sets to the groups' starts.  The few tiles
//             that hold keys of more than one d1, and the partial last tile, are placed key by key by a small kernel
//             afterwards.  GS_LSB_PLAN_SCATTER2=stable keeps the stable scatter with its upsweep.
constexpr uint32_t PLAN_GROUPS = 65536;
constexpr uint32_t PLAN_WORDS = PLAN_GROUPS / 2;          // 16-bit counters, two to a word: 128 KiB of LDS
constexpr uint32_t PLAN_PLANNED = 1u, PLAN_CLASSIC = 2u;  // route word (0: no sort has run on this workspace)
constexpr uint32_t PLAN_SKIP = 0xffffffffu;               // shift of a slot that does nothing
// The look's wave-private digit histograms have the 32 KiB of LDS that the table leaves: one copy per wave (the upsweep's
// four do not fit), 1024 threads = two chunks at a time.  Two packed 16-bit copies per wave were as fast and 512 threads
// with two copies slower (profiles/fused_look_layouts.json).
constexpr int PLAN_LOOK_THREADS = 1024, PLAN_LOOK_WAVES = PLAN_LOOK_THREADS / WAVE, PLAN_LOOK_BATCH = 32;
constexpr uint32_t PLAN_LOOK_HALVES = PLAN_LOOK_WAVES / LSB_CHUNK;   // chunks a look workgroup counts at a time
static_assert(PLAN_LOOK_WAVES % LSB_CHUNK == 0, "a look workgroup takes whole chunks");
constexpr uint32_t PLAN_LOOK_MAX_GRID = MI355X_CUS;       // one resident workgroup per CU
constexpr uint32_t PLAN_BLOCKS = 128, PLAN_BLOCK_WORDS = PLAN_WORDS / PLAN_BLOCKS, PLAN_BLOCK_GROUPS = PLAN_GROUPS / PLAN_BLOCKS;
constexpr int PLAN_SORT_BITS = 16;
constexpr int PLAN_SKEW_LANES = 8;                      // look: lanes of a wave in one group from which a batch counts as skewed
constexpr uint32_t PLAN_IRR_CAP = RADIX - 1;            // tiles of the first scatter's output that straddle two of its digit runs: one per boundary at most
constexpr size_t PLAN_CURSOR_BYTES = (size_t)PLAN_GROUPS * sizeof(uint32_t);

struct PlanBlock {
    // head: what gs_lsb_plan_status returns
    uint32_t route, max_group, nonempty, tasks[MSB_NCLASS], total;
    uint32_t shift[4];                                     // digit position of each pass slot
    uint32_t ups_skip[4];                                  // the slot's upsweep has nothing to do (the look left slot 1's counts)
    MsbLevel level[2];                                     // [0]: the finish's task counts; [1]: read by the sample look
    union {
        uint32_t wg_bad[PLAN_LOOK_MAX_GRID];               // look: the workgroup's table does not add up (a counter wrapped)
        // the same words once the decision has read them, until the next look: [0] = tiles of the second scatter left to the
        // follow-up kernel (cursor mode; set to 0 with the cursors), [1..] = which
        uint32_t irr[1 + PLAN_IRR_CAP];
    };
    uint32_t blk_total[PLAN_BLOCKS], blk_max[PLAN_BLOCKS], blk_nonempty[PLAN_BLOCKS];
    uint32_t blk_class[PLAN_BLOCKS][MSB_NCLASS];           // groups per local-sort class among the block's 512 groups
    uint32_t blk_class_base[PLAN_BLOCKS][MSB_NCLASS];      // the same, summed over the earlier blocks
    uint32_t offsets[PLAN_GROUPS + 1];                     // exclusive scan of the group sizes
    uint32_t cursor_mode;                                  // this sort's second scatter claims its places with cursors
};
static_assert(1 + PLAN_IRR_CAP <= PLAN_LOOK_MAX_GRID, "the list of straddling tiles fits the look's flags");
static_assert(sizeof(MsbLevel) == 64 && offsetof(PlanBlock, level) == 64, "plan block layout");

__device__ __forceinline__ int plan_class_of(uint32_t size)
{
    return size <= msb_class_cap(0) ? 0 : size <= msb_class_cap(1) ? 1 : size <= msb_class_cap(2) ? 2 : 3;
}

// The look counts two things per key: its group (top 16 bits, into the workgroup's packed table) and the digit of the first
// PLANNED scatter, bits 16-23 = group & 0xff, into a histogram private to the wave (= the tile).  One count of each; a group
// shared by the whole wave (constant high bytes) is one add to each, not 64 queued ones.
__device__ __forceinline__ void look_add(uint32_t *tab, uint32_t *my, uint32_t g)
{
    const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
    const uint32_t g0 = __builtin_amdgcn_readfirstlane(g);
    if (__builtin_amdgcn_ballot_w64(g == g0) == act) {
        if (count_lower_mask(act) == 0) {
            atomicAdd(&tab[g0 >> 1], (uint32_t)__popcll(act) << ((g0 & 1u) * 16u));
            atomicAdd(&my[g0 & 0xffu], (uint32_t)__popcll(act));
        }
    } else {
        atomicAdd(&tab[g >> 1], 1u << ((g & 1u) * 16u));
        atomicAdd(&my[g & 0xffu], 1u);
    }
}

// The same for a full wave of keys that looks skewed (see the look kernel): the two most likely shared groups -- that of the
// first lane, then that of the first lane left over -- are one add each, the other lanes add for themselves.  Lanes that
// add to the same counter in one instruction are served one after the other: with half of the keys in one group that was
// 20-35 % of the whole sort.  Lanes that share a group share its digit.
__device__ __forceinline__ void look_add_skew(uint32_t *tab, uint32_t *my, uint32_t g, int lane)
{
    unsigned long long rest = ~0ull;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (rest == 0ull) break;
        const int lead = __builtin_amdgcn_readfirstlane(__builtin_ctzll(rest));
        const uint32_t g0 = (uint32_t)__builtin_amdgcn_readlane((int)g, lead);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(g == g0) & rest;
        if (lane == lead) {
            atomicAdd(&tab[g0 >> 1], (uint32_t)__popcll(m) << ((g0 & 1u) * 16u));
            atomicAdd(&my[g0 & 0xffu], (uint32_t)__popcll(m));
        }
        rest &= ~m;
    }
    if ((rest >> lane) & 1ull) {
        atomicAdd(&tab[g >> 1], 1u << ((g & 1u) * 16u));
        atomicAdd(&my[g & 0xffu], 1u);
    }
}

// Look workgroup b -> the position of its first unit of PLAN_LOOK_HALVES chunks: under round-robin dispatch the workgroups
// of one XCD take consecutive units, so the chunk totals that share a 64-byte line of a spine row meet in one L2 (as
// chunk_of_block does for the upsweep).  Speed only: any bijection gives the same result.
__device__ __forceinline__ uint32_t look_slot_of_block(uint32_t b, uint32_t grid)
{
    if (grid % MI355X_XCDS) return b;
    return (b % MI355X_XCDS) * (grid / MI355X_XCDS) + b / MI355X_XCDS;
}

// The fused look.  The unit of work is the upsweep's chunk of LSB_CHUNK tiles, one wave per tile; a workgroup of 16 waves
// takes PLAN_LOOK_HALVES = 2 neighbouring chunks at a time and walks the units slot, slot + grid, ...  Besides the group
// table it leaves, per chunk, exactly what upsweep_chunk<false, false> writes for shift 16, bits 8 (the first scatter of the
// PLANNED route): prefix16[tile][d] = keys of digit d in the earlier tiles of the chunk, spine[d][chunk] = the chunk's total.
// So the slot-1 upsweep has nothing to do when the plan is PLANNED; when CLASSIC it runs at shift 0 and overwrites both.
// A 16-bit counter of the table wraps only when the workgroup saw 65536 keys of one group -- far above the cap -- and then
// the table no longer sums to the keys counted (a wrap of the low half carries into the high half: -65535; of the high
// half: -65536): the workgroup reports that, and the plan is CLASSIC.
struct LookSmem {
    uint32_t tab[PLAN_WORDS];
    uint32_t hist[PLAN_LOOK_WAVES][RADIX + 1];   // (rows padded as in UpsweepSmem)
    uint32_t red[2];
};
static_assert(sizeof(LookSmem) <= 160 * 1024, "the look's LDS");

__global__ __launch_bounds__(PLAN_LOOK_THREADS) void lsb_plan_look_kernel(const uint32_t *__restrict__ keys, uint32_t *__restrict__ partial,
                                                                          PlanBlock *__restrict__ plan, uint32_t *__restrict__ spine,
                                                                          uint16_t *__restrict__ prefix16, uint32_t n, uint32_t chunks,
                                                                          int f32_in, uint32_t xor_in)
{
    __shared__ LookSmem sm;
    uint32_t *tab = sm.tab;
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    for (uint32_t i = tid; i < PLAN_WORDS; i += PLAN_LOOK_THREADS) tab[i] = 0;
    for (uint32_t i = tid; i < sizeof(sm.hist) / sizeof(uint32_t); i += PLAN_LOOK_THREADS) (&sm.hist[0][0])[i] = 0;
    if (tid < 2) sm.red[tid] = 0;
    __syncthreads();
    uint32_t *my = sm.hist[w];
    const uint32_t num_tiles = n / (uint32_t)LSB_TILE + (n % (uint32_t)LSB_TILE ? 1u : 0u);
    const uint32_t units = (chunks + PLAN_LOOK_HALVES - 1u) / PLAN_LOOK_HALVES;
    auto group_of = [&](uint32_t raw) { return twiddle_in(raw, f32_in, xor_in) >> 16; };
    uint32_t counted = 0;   // wave-uniform
    constexpr int GB = PLAN_LOOK_BATCH;
#pragma unroll 1
    for (uint32_t unit = look_slot_of_block(blockIdx.x, gridDim.x); unit < units; unit += gridDim.x) {
        const uint32_t tile = unit * (uint32_t)PLAN_LOOK_WAVES + (uint32_t)w;      // wave w: tile w % 8 of the unit's chunk w / 8
        if (tile < num_tiles) {
        const uint32_t lo = tile * (uint32_t)LSB_TILE;                       // < n < 2^32
        const uint32_t len = (n - lo < (uint32_t)LSB_TILE) ? n - lo : (uint32_t)LSB_TILE;
        const uint32_t *src = keys + lo;
        counted += len;
        if (len == (uint32_t)LSB_TILE) {
#pragma unroll 1
            for (uint32_t j = 0; j < (uint32_t)LSB_TILE; j += GB * WAVE) {
                const uint32_t *at = src + j + lane;
                uint32_t v[GB];
#pragma unroll
                for (int u = 0; u < GB; ++u) v[u] = __builtin_nontemporal_load(at + u * WAVE);
                const uint32_t ga = group_of(v[0]), gb = group_of(v[GB / 2]);
                // how many lanes share the first lane's group, on two keys of the batch: all of them (constant high bytes),
                // PLAN_SKEW_LANES or more (a few heavy groups), or hardly any (the usual case: two plain adds per key)
                const unsigned long long ma = __builtin_amdgcn_ballot_w64(ga == __builtin_amdgcn_readfirstlane(ga)),
                                         mb = __builtin_amdgcn_ballot_w64(gb == __builtin_amdgcn_readfirstlane(gb));
                if (ma == ~0ull || mb == ~0ull) {
#pragma unroll
                    for (int u = 0; u < GB; ++u) look_add(tab, my, group_of(v[u]));
                } else if (__popcll(ma) >= PLAN_SKEW_LANES || __popcll(mb) >= PLAN_SKEW_LANES) {
#pragma unroll
                    for (int u = 0; u < GB; ++u) look_add_skew(tab, my, group_of(v[u]), lane);
                } else {
#pragma unroll
                    for (int u = 0; u < GB; ++u) {
                        const uint32_t g = group_of(v[u]);
                        atomicAdd(&tab[g >> 1], 1u << ((g & 1u) * 16u));
                        atomicAdd(&my[g & 0xffu], 1u);
                    }
                }
            }
        } else {
            // the array's ragged last tile: loads from clamped indices, guarded counts
            const uint32_t last = len - 1u;
#pragma unroll 1
            for (uint32_t j = 0; j < len; j += GB * WAVE) {
                uint32_t v[GB];
#pragma unroll
                for (int u = 0; u < GB; ++u) {
                    const uint32_t idx = j + u * WAVE + lane;
                    v[u] = src[idx < last ? idx : last];
                }
#pragma unroll
                for (int u = 0; u < GB; ++u)
                    if (j + u * WAVE + lane < len) look_add(tab, my, group_of(v[u]));
            }
        }
        }
        __syncthreads();
        // the unit's results, one thread per chunk and digit; the thread clears the counters it has read
        if (tid < (int)PLAN_LOOK_HALVES * RADIX) {
            const uint32_t half = (uint32_t)tid / RADIX, d = (uint32_t)tid % RADIX, chunk = unit * PLAN_LOOK_HALVES + half;
            uint32_t run = 0;
#pragma unroll
            for (int j = 0; j < LSB_CHUNK; ++j) {
                const uint32_t t = chunk * LSB_CHUNK + (uint32_t)j;
                if (t < num_tiles) prefix16[(size_t)t * RADIX + d] = (uint16_t)run;
                uint32_t *c = &sm.hist[half * LSB_CHUNK + j][d];
                run += *c;
                *c = 0;
            }
            if (chunk < chunks) spine[d * chunks + chunk] = run;
        }
        __syncthreads();
    }
    uint32_t sum = 0;
    uint32_t *out = partial + (size_t)blockIdx.x * PLAN_WORDS;
    for (uint32_t i = tid; i < PLAN_WORDS; i += PLAN_LOOK_THREADS) {
        const uint32_t c = tab[i];
        sum += (c & 0xffffu) + (c >> 16);
        out[i] = c;
    }
    sum = wave_reduce_sum(sum);
    if (lane == 0) { atomicAdd(&sm.red[0], sum); atomicAdd(&sm.red[1], counted); }
    __syncthreads();
    if (tid == 0) plan->wg_bad[blockIdx.x] = sm.red[0] != sm.red[1] ? 1u : 0u;
}

// Block b sums the partial tables of the groups [512 b, 512 b + 512): sizes -> block-local exclusive scan (into `offsets`),
// the block's total, largest group, non-empty groups and groups per class.
__global__ __launch_bounds__(RADIX) void lsb_plan_reduce_kernel(const uint32_t *__restrict__ partial, PlanBlock *__restrict__ plan, uint32_t parts)
{
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t red[2 + MSB_NCLASS];
    const uint32_t tid = threadIdx.x, wi = blockIdx.x * PLAN_BLOCK_WORDS + tid;
    if (tid < 2 + MSB_NCLASS) red[tid] = 0;
    uint32_t c0 = 0, c1 = 0;
#pragma unroll 8
    for (uint32_t g = 0; g < parts; ++g) {
        const uint32_t v = partial[(size_t)g * PLAN_WORDS + wi];
        c0 += v & 0xffffu;
        c1 += v >> 16;
    }
    uint32_t total = 0;
    const uint32_t ex = block_exclusive_scan_256(c0 + c1, scratch, &total);   // (its barriers also cover `red`)
    plan->offsets[2 * wi] = ex;
    plan->offsets[2 * wi + 1] = ex + c0;
    atomicMax(&red[0], c0 > c1 ? c0 : c1);
    if (c0) { atomicAdd(&red[1], 1u); atomicAdd(&red[2 + plan_class_of(c0)], 1u); }
    if (c1) { atomicAdd(&red[1], 1u); atomicAdd(&red[2 + plan_class_of(c1)], 1u); }
    __syncthreads();
    if (tid == 0) {
        plan->blk_total[blockIdx.x] = total;
        plan->blk_max[blockIdx.x] = red[0];
        plan->blk_nonempty[blockIdx.x] = red[1];
    }
    if (tid < MSB_NCLASS) plan->blk_class[blockIdx.x][tid] = red[2 + tid];
}

// Every block scans the 128 block records (a few hundred words) for itself and makes its 512 offsets global; block 0 also
// writes the decision: PLANNED if and only if no look workgroup reported a wrapped counter, the sizes add up to n and no
// group exceeds the largest local sort.  The level records of the finish are (re)written here on every sort, so stale
// lists of an earlier sort on the same workspace never run.
// `mailbox` (or null): the host's look at the decision (see PlanPeek) -- the plan block's head and the scatter mode, written to
// a pinned host mailbox by the thread that decides; the host reads them behind an event recorded after this launch.
constexpr int PLAN_PEEK_WORDS = 9;   // route, max_group, nonempty, tasks[4], total, cursor_mode
__global__ __launch_bounds__(RADIX) void lsb_plan_decide_kernel(PlanBlock *__restrict__ plan, uint32_t n, uint32_t parts, uint32_t cursor_on,
                                                                uint32_t *mailbox)
{
    __shared__ uint32_t s_base, s_total, s_max, s_nz, s_cls[MSB_NCLASS], s_clsbase[MSB_NCLASS];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    if (tid == 0) {
        uint32_t base = 0, total = 0, mx = 0, nz = 0;
        for (uint32_t i = 0; i < PLAN_BLOCKS; ++i) {
            if (i == b) base = total;
            total += plan->blk_total[i];
            const uint32_t m = plan->blk_max[i];
            mx = m > mx ? m : mx;
            nz += plan->blk_nonempty[i];
        }
        s_base = base; s_total = total; s_max = mx; s_nz = nz;
    } else if (tid <= MSB_NCLASS) {
        const uint32_t c = tid - 1u;
        uint32_t base = 0, total = 0;
        for (uint32_t i = 0; i < PLAN_BLOCKS; ++i) {
            if (i == b) base = total;
            total += plan->blk_class[i][c];
        }
        s_cls[c] = total; s_clsbase[c] = base;
    }
    const int any_bad = __syncthreads_or(tid < parts ? (int)plan->wg_bad[tid] : 0);
    const uint32_t g = b * PLAN_BLOCK_GROUPS + 2u * tid;
    plan->offsets[g] += s_base;
    plan->offsets[g + 1] += s_base;
    if (tid < MSB_NCLASS) plan->blk_class_base[b][tid] = s_clsbase[tid];
    if (b == 0 && tid == 0) {
        const bool planned = !any_bad && s_total == n && s_max <= msb_class_cap(MSB_NCLASS - 1);
        plan->route = planned ? PLAN_PLANNED : PLAN_CLASSIC;
        plan->max_group = s_max;
        plan->nonempty = s_nz;
        plan->total = s_total;
        MsbLevel l0{}, l1{};
        for (int c = 0; c < MSB_NCLASS; ++c) {
            plan->tasks[c] = planned ? s_cls[c] : 0u;
            l0.task_count[c] = planned ? s_cls[c] : 0u;
        }
        l0.keys = n;
        l1.packed = planned ? (1ull << 32) : 0ull;   // "the level showed skew": the sample look runs, so tasks of few distinct values get their plan
        plan->level[0] = l0;
        plan->level[1] = l1;
        for (int q = 0; q < 4; ++q) {
            plan->shift[q] = planned ? (q < 2 ? 16u + 8u * (uint32_t)q : PLAN_SKIP) : 8u * (uint32_t)q;
            plan->ups_skip[q] = planned && q != 1 ? 1u : 0u;   // PLANNED: slot 1 scans and scatters on the look's counts
        }
        plan->offsets[PLAN_GROUPS] = n;
        const uint32_t mode = planned && cursor_on ? 1u : 0u;
        plan->cursor_mode = mode;
        if (mailbox) {
            mailbox[0] = planned ? PLAN_PLANNED : PLAN_CLASSIC;
            mailbox[1] = s_max;
            mailbox[2] = s_nz;
            for (int c = 0; c < MSB_NCLASS; ++c) mailbox[3 + c] = planned ? s_cls[c] : 0u;
            mailbox[3 + MSB_NCLASS] = s_total;
            mailbox[PLAN_PEEK_WORDS - 1] = mode;
            __threadfence_system();
        }
    }
}
static_assert(offsetof(PlanBlock, total) == (PLAN_PEEK_WORDS - 2) * sizeof(uint32_t) && PLAN_PEEK_WORDS == 5 + MSB_NCLASS, "the head is eight words");

// The finish's task lists: one task per non-empty group, in group order inside each class.  Nothing when CLASSIC.
struct PlanLists { MsbTask *tasks[MSB_NCLASS]; uint32_t cap[MSB_NCLASS]; };
__global__ __launch_bounds__(PLAN_BLOCK_GROUPS) void lsb_plan_tasks_kernel(const PlanBlock *__restrict__ plan, PlanLists lists)
{
    __shared__ uint32_t wcnt[PLAN_BLOCK_GROUPS / WAVE][MSB_NCLASS];
    if (plan->route != PLAN_PLANNED) return;
    const uint32_t tid = threadIdx.x, g = blockIdx.x * PLAN_BLOCK_GROUPS + tid;
    const int w = wave_id(), lane = lane_id();
    const uint32_t off = plan->offsets[g], size = plan->offsets[g + 1] - off;
    const int cls = size ? plan_class_of(size) : -1;
    uint32_t lower = 0;
#pragma unroll
    for (int c = 0; c < MSB_NCLASS; ++c) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(cls == c);
        if (cls == c) lower = count_lower_mask(m);
        if (lane == 0) wcnt[w][c] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (cls >= 0) {
        uint32_t idx = plan->blk_class_base[blockIdx.x][cls] + lower;
        for (int j = 0; j < w; ++j) idx += wcnt[j][cls];
        if (idx < lists.cap[cls]) lists.tasks[cls][idx] = MsbTask{off, size, (uint32_t)PLAN_SORT_BITS, 0u};
    }
}

// The pass slots: lsb_upsweep_kernel / lsb_downsweep_kernel with the digit position read from the plan (one scalar load).
// The upsweep also returns when the plan says that the look has already left this slot's spine and prefix16.
template <bool PLAIN>
__global__ __launch_bounds__(LSB_THREADS, GS_EXP_UPS_WPE) void lsb_plan_upsweep_kernel(const uint32_t *__restrict__ keys,
                                                                       uint32_t *__restrict__ spine, uint16_t *__restrict__ prefix16,
                                                                       const uint32_t *__restrict__ slot_shift,
                                                                       const uint32_t *__restrict__ slot_ups_skip, PassParams p)
{
    __shared__ UpsweepSmem<false, false> sm;
    const uint32_t sh = *slot_shift;
    if (sh == PLAN_SKIP || *slot_ups_skip) return;
    p.shift = sh;
    upsweep_chunk<false, false, PLAIN>(sm, keys, chunk_of_block(blockIdx.x, p.grid), spine, prefix16, nullptr, nullptr, p, PipeParams{});
}

template <bool TAIL, int TW, bool BIG>
__global__ __launch_bounds__(LSB_THREADS, 6) void lsb_plan_downsweep_kernel(const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out,
                                                                            const uint32_t *__restrict__ totals, const uint32_t *__restrict__ spine,
                                                                            const uint16_t *__restrict__ prefix16,
                                                                            const uint32_t *__restrict__ slot_shift, PassParams p)
{
    __shared__ __attribute__((aligned(16))) DownsweepSmem<false> sm;
    const uint32_t sh = *slot_shift;
    if (sh == PLAN_SKIP) return;
    p.shift = sh;
    const uint32_t full_tiles = p.n / (uint32_t)LSB_TILE;
    if (!TAIL && blockIdx.x >= full_tiles) return;
    const uint32_t t = TAIL ? full_tiles : tile_of_item_wide(blockIdx.x, full_tiles);
    downsweep_tile<false, TAIL, TW, BIG, false>(sm, t, keys_in, keys_out, nullptr, nullptr, spine, prefix16, totals, p, nullptr, 0u, nullptr);
}

// The second pass slot's own kernels.  They are the slot kernels above, and in cursor mode (PLANNED, see the top):
//   upsweep   sets the cursors, laid out [d1][d2] so that a tile's claims are four 256-byte wave instructions, to the starts
//             of the groups (d2, d1), and the list of straddling tiles to empty (its words are the look's flags, which the
//             decide kernel's workgroups are still reading when the mode is written); no look at the keys;
//   scatter   downsweep_tile in CURSOR mode on the full tiles; the partial tile's launch returns;
//   irregular places the keys of the listed tiles (one workgroup each) and of the partial tile (the last workgroup): see
//             lsb_plan_irregular_kernel.
template <bool PLAIN>
__global__ __launch_bounds__(LSB_THREADS, GS_EXP_UPS_WPE) void lsb_plan_upsweep2_kernel(const uint32_t *__restrict__ keys,
                                                                        uint32_t *__restrict__ spine, uint16_t *__restrict__ prefix16,
                                                                        PlanBlock *__restrict__ plan, uint32_t *__restrict__ cursor,
                                                                        PassParams p)
{
    __shared__ UpsweepSmem<false, false> sm;
    if (plan->cursor_mode) {
        if (blockIdx.x == 0 && threadIdx.x == 0) plan->irr[0] = 0;
        for (uint32_t i = blockIdx.x * (uint32_t)LSB_THREADS + threadIdx.x; i < PLAN_GROUPS; i += gridDim.x * (uint32_t)LSB_THREADS)
            cursor[i] = plan->offsets[((i & (uint32_t)(RADIX - 1)) << RADIX_BITS) | (i >> RADIX_BITS)];
        return;
    }
    const uint32_t sh = plan->shift[1];
    if (sh == PLAN_SKIP || plan->ups_skip[1]) return;
    p.shift = sh;
    upsweep_chunk<false, false, PLAIN>(sm, keys, chunk_of_block(blockIdx.x, p.grid), spine, prefix16, nullptr, nullptr, p, PipeParams{});
}

template <bool TAIL, bool BIG>
__global__ __launch_bounds__(LSB_THREADS, 6) void lsb_plan_scatter2_kernel(const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out,
                                                                           const uint32_t *__restrict__ totals, const uint32_t *__restrict__ spine,
                                                                           const uint16_t *__restrict__ prefix16, PlanBlock *__restrict__ plan,
                                                                           uint32_t *__restrict__ cursor, PassParams p)
{
    __shared__ __attribute__((aligned(16))) DownsweepSmem<false> sm;
    const uint32_t sh = plan->shift[1];
    if (sh == PLAN_SKIP) return;
    p.shift = sh;
    const uint32_t full_tiles = p.n / (uint32_t)LSB_TILE;
    const uint32_t mode = plan->cursor_mode;
    if constexpr (TAIL) {
        if (mode) return;
        downsweep_tile<false, true, 2, true, false>(sm, full_tiles, keys_in, keys_out, nullptr, nullptr, spine, prefix16, totals, p, nullptr, 0u,
                                                    nullptr);
    } else {
        if (blockIdx.x >= full_tiles) return;
        const uint32_t t = tile_of_item_wide(blockIdx.x, full_tiles);
        if (mode)
            downsweep_tile<false, false, 0, BIG, false, false, true>(sm, t, keys_in, keys_out, nullptr, nullptr, spine, prefix16, totals, p,
                                                                     nullptr, 0u, nullptr, threadIdx.x, nullptr, cursor, plan->irr, PLAN_IRR_CAP);
        else
            downsweep_tile<false, false, 0, BIG, false>(sm, t, keys_in, keys_out, nullptr, nullptr, spine, prefix16, totals, p, nullptr, 0u,
                                                        nullptr);
    }
}

// The cursor set-up and the scatter of a sort whose host has seen PLANNED and cursor mode before it enqueues the second slot
// (lsb_plan_slot2_cursor): the set-up is the 65536 words and nothing else -- no workgroup per chunk, no upsweep LDS -- and the
// scatter takes its digit position from the host and its mode from the template, so it reads nothing from the plan block
// but the list of straddling tiles it appends to.  The partial tile is the follow-up kernel's.
__global__ __launch_bounds__(LSB_THREADS) void lsb_plan_cursor_init_kernel(PlanBlock *__restrict__ plan, uint32_t *__restrict__ cursor)
{
    const uint32_t i = blockIdx.x * (uint32_t)LSB_THREADS + threadIdx.x;   // the grid covers the cursors exactly
    if (i == 0) plan->irr[0] = 0;
    cursor[i] = plan->offsets[((i & (uint32_t)(RADIX - 1)) << RADIX_BITS) | (i >> RADIX_BITS)];
}
static_assert(PLAN_GROUPS % LSB_THREADS == 0, "whole workgroups set the cursors");

// GS_PLAN_RANK_FREE (default 1; 0: the stable ballot-match ranking, for A/B builds): the order of the keys inside a digit run
// does not show in the result, so this scatter ranks with one returning add per key on the wave's own LDS counters.
#ifndef GS_PLAN_RANK_FREE
#define GS_PLAN_RANK_FREE 1
#endif
template <bool BIG>
__global__ __launch_bounds__(LSB_THREADS, 6) void lsb_plan_scatter2_cursor_kernel(const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out,
                                                                                  uint32_t *__restrict__ irr, uint32_t *__restrict__ cursor,
                                                                                  PassParams p)
{
    __shared__ __attribute__((aligned(16))) DownsweepSmem<false> sm;
    const uint32_t full_tiles = p.n / (uint32_t)LSB_TILE;
    if (blockIdx.x >= full_tiles) return;
    const uint32_t t = tile_of_item_wide(blockIdx.x, full_tiles);
    constexpr bool RANK_FREE = GS_PLAN_RANK_FREE != 0;
    downsweep_tile<false, false, 0, BIG, false, false, true, RANK_FREE>(sm, t, keys_in, keys_out, nullptr, nullptr, nullptr, nullptr, nullptr, p, nullptr,
                                                                        0u, nullptr, threadIdx.x, nullptr, cursor, irr, PLAN_IRR_CAP);
}

// The follow-up kernel: one workgroup per listed tile and one for the partial tile, LSB_KPT rounds of LSB_THREADS keys.  Every
// key's place comes from an add on its group's cursor, and a round trip to the cursors is microseconds, so nothing here
// waits for memory more than three times: all loads of the tile are issued (clamped indices for the partial tile), then all
// claims, and only then are places computed and keys stored.
// The tile is sorted on d1 (bits 16-23), and nearly always holds two values of it, so the groups of its first and of its last
// d1 are counted in LDS -- a returning add per key gives its rank inside the tile's share of the group -- and claimed with one
// add per group and tile: 512 adds on the cursors at the most, not 8192 (with an add per key the launch was bound by the
// rate of the adds, not by their latency: 255 tiles of uniform keys, 2.1 M adds, took 71 us with all of them in flight
// against 63 us one after the other).  Keys of a d1 in between (a tile with three and more values) claim for themselves;
// the claims of a wave round there: the first two groups met are one add each, by their first lane, every lane left over
// adds for itself -- so a lane issues at most one such add per round.
constexpr int PLAN_IRR_ROUNDS = LSB_TILE / LSB_THREADS;
static_assert(LSB_THREADS == 2 * RADIX, "the follow-up kernel: one thread per group of the tile's first and last d1");
__global__ __launch_bounds__(LSB_THREADS, 4) void lsb_plan_irregular_kernel(const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out,
                                                                            const PlanBlock *__restrict__ plan, uint32_t *__restrict__ cursor,
                                                                            uint32_t n)
{
    __shared__ uint32_t edge[2 * RADIX];           // [first d1 | last d1][d2]: keys of the tile, then the places claimed for them
    // (the three words of the plan block in one round trip, not one behind the other)
    const uint32_t mode = plan->cursor_mode, count = plan->irr[0], t = plan->irr[blockIdx.x < PLAN_IRR_CAP ? 1u + blockIdx.x : 1u];
    asm volatile("" ::"s"(mode), "s"(count), "s"(t));   // (all three requested before the first is looked at)
    if (!mode) return;
    const uint32_t full_tiles = n / (uint32_t)LSB_TILE;
    uint32_t lo, len;
    if (blockIdx.x == PLAN_IRR_CAP) {
        lo = full_tiles * (uint32_t)LSB_TILE;
        len = n - lo;
        if (len == 0u) return;                     // (never launched then)
    } else {
        const uint32_t listed = count < PLAN_IRR_CAP ? count : PLAN_IRR_CAP;
        if (blockIdx.x >= listed) return;
        if (t >= full_tiles) return;
        lo = t * (uint32_t)LSB_TILE;
        len = (uint32_t)LSB_TILE;
    }
    const int lane = lane_id();
    const uint32_t tid = threadIdx.x, last = len - 1u;
    const uint32_t *src = keys_in + lo;
    uint32_t k[PLAN_IRR_ROUNDS];
#pragma unroll
    for (int r = 0; r < PLAN_IRR_ROUNDS; ++r) {
        const uint32_t i = tid + (uint32_t)r * (uint32_t)LSB_THREADS;
        k[r] = src[i < last ? i : last];
    }
    const uint32_t k_first = src[0], k_last = src[last];
    asm volatile("" ::"s"(k_first), "s"(k_last));       // (both requested before either is looked at)
    const uint32_t d1_first = (k_first >> 16) & (uint32_t)(RADIX - 1), d1_last = (k_last >> 16) & (uint32_t)(RADIX - 1);
    edge[tid] = 0;
    __syncthreads();
    // per round, claim[r] = the lane whose add covers this key | this key's rank among that add's keys << 8 | what this lane
    // itself adds to its own group's cursor << 16 (0: nothing; always 0 for a key counted in LDS); got[r] = what the lane's
    // own add returned: the key's rank in `edge`, or the place claimed on the cursor
    uint32_t claim[PLAN_IRR_ROUNDS], got[PLAN_IRR_ROUNDS];
    auto cursor_of = [](uint32_t key) {            // cursor of group (d2, d1): [d1][d2]
        const uint32_t g = key >> 16;
        return ((g & (uint32_t)(RADIX - 1)) << RADIX_BITS) | (g >> RADIX_BITS);
    };
    auto edge_of = [&](uint32_t key) {             // the key's counter in `edge`, or 2 * RADIX: it has none
        const uint32_t d1 = (key >> 16) & (uint32_t)(RADIX - 1);
        return d1 == d1_first ? key >> 24 : d1 == d1_last ? (uint32_t)RADIX + (key >> 24) : 2u * (uint32_t)RADIX;
    };
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < PLAN_IRR_ROUNDS; ++r) {
        const bool have = tid + (uint32_t)r * (uint32_t)LSB_THREADS < len;
        const uint32_t e = edge_of(k[r]), c = cursor_of(k[r]);
        const bool mid = have && e == 2u * (uint32_t)RADIX;
        got[r] = 0;
        if (have && !mid) got[r] = atomicAdd(&edge[e], 1u);
        unsigned long long rest = __builtin_amdgcn_ballot_w64(mid);
        uint32_t cl = (uint32_t)lane;
        if (rest != 0ull) {                        // (wave-uniform; the usual tile has no such key)
#pragma unroll
            for (int q = 0; q < 2; ++q) {          // (nothing left: m = 0, and nothing happens)
                const int lead = __builtin_amdgcn_readfirstlane(rest ? __builtin_ctzll(rest) : 0);
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)c, lead);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(mid && c == c0) & rest;
                if ((m >> lane) & 1ull) cl = (uint32_t)lead | ((uint32_t)__popcll(m & below) << 8) | (lane == lead ? (uint32_t)__popcll(m) << 16 : 0u);
                rest &= ~m;
            }
            if ((rest >> lane) & 1ull) cl |= 1u << 16;
        }
        claim[r] = cl;
    }
#pragma unroll
    for (int r = 0; r < PLAN_IRR_ROUNDS; ++r)
        if (claim[r] >> 16) got[r] = __hip_atomic_fetch_add(cursor + cursor_of(k[r]), claim[r] >> 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    {   // thread tid claims for the counter it zeroed, and leaves the place in its stead
        const uint32_t mine = edge[tid], d1 = tid < (uint32_t)RADIX ? d1_first : d1_last;
        if (mine) edge[tid] = __hip_atomic_fetch_add(cursor + ((d1 << RADIX_BITS) | (tid & (uint32_t)(RADIX - 1))), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PLAN_IRR_ROUNDS; ++r) {
        const bool have = tid + (uint32_t)r * (uint32_t)LSB_THREADS < len;
        const uint32_t e = edge_of(k[r]);
        uint32_t at = (uint32_t)__shfl((int)got[r], (int)(claim[r] & 0xffu)) + ((claim[r] >> 8) & 0xffu);
        if (e < 2u * (uint32_t)RADIX) at += edge[e];
        if (have && at < n) keys_out[at] = k[r];
    }
}

// ------------------------------------------------------------------- host --
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// GS_LSB_KEYS_PLAN=classic|auto (default auto): classic = the four passes, always.  GS_LSB_PLAN_MIN_ITEMS=<n> (tests only)
// moves the lower end of the size window, so that small inputs reach the plan.  Both are read once per process.
static inline bool plan_enabled()
{
    static const bool v = [] { const char *e = getenv("GS_LSB_KEYS_PLAN"); return !(e && strcmp(e, "classic") == 0); }();
    return v;
}
// GS_LSB_PLAN_SCATTER2=cursor|stable (default cursor): stable = the second PLANNED scatter keeps its upsweep and its order.
static inline bool plan_cursor_enabled()
{
    static const bool v = [] { const char *e = getenv("GS_LSB_PLAN_SCATTER2"); return !(e && strcmp(e, "stable") == 0); }();
    return v;
}
// N_MAX: 65536 groups of uniform keys are binomial with mean m = n / 65536 and deviation sqrt(m); the largest of 65536 such
// groups lies 4 to 5 deviations above the mean, so m + 6 sqrt(m) <= 17408 (m = 16620, sqrt(m) = 129) keeps uniform keys
// PLANNED with a chance of failure below 1e-4 per sort.  Above it the look would nearly always say CLASSIC.
constexpr uint64_t PLAN_N_MAX = (uint64_t)PLAN_GROUPS * 16620u;
constexpr uint64_t PLAN_N_FLOOR = 65536;            // the partial tables need room in the alternate buffer: two look workgroups at least
constexpr uint64_t PLAN_N_MIN = GS_PLAN_N_MIN;      // 2^28: the smallest measured size from which PLANNED wins by more than 5 % on uniform keys
static inline uint64_t plan_min_items()
{
    static const uint64_t v = [] {
        const char *e = getenv("GS_LSB_PLAN_MIN_ITEMS");
        if (!e) return PLAN_N_MIN;
        const uint64_t x = strtoull(e, nullptr, 10);
        return x < PLAN_N_FLOOR ? PLAN_N_FLOOR : x;
    }();
    return v;
}
// sizes whose workspace carries the plan block (every size from the window's lower end up: the query stays monotone)
static inline bool plan_has_block(uint64_t n) { return !lsb_pipe_enabled() && n >= plan_min_items(); }
static inline bool plan_size_ok(uint64_t n) { return plan_has_block(n) && n <= PLAN_N_MAX; }
// the lists' capacities: one task per non-empty group, and a class-c task holds more than cap(c - 1) keys
static inline uint32_t plan_list_cap(uint64_t n, int c)
{
    const uint64_t m = c == 0 ? n : n / ((uint64_t)msb_class_cap(c - 1) + 1u) + 1u;
    return (uint32_t)(m < PLAN_GROUPS ? m : PLAN_GROUPS);
}
static inline size_t plan_lists_bytes(uint64_t n)
{
    size_t b = 0;
    for (int c = 0; c < MSB_NCLASS; ++c) b += (size_t)plan_list_cap(n, c) * sizeof(MsbTask);
    return b;
}
// Layout: the plan block follows the four-pass workspace.  The task lists END where the plan block starts and reach back
// over the spine / totals / prefix16 / pass-totals region, which is dead by the time they are written (PLANNED: the last
// real pass is slot 2; the lists are written after slot 4); only arrays too small for that (test sizes) get extra room.
static inline size_t plan_block_offset(uint64_t n)
{
    const size_t a = lsb_temp_bytes(n), b = plan_lists_bytes(n);
    return align256(a > b ? a : b);
}
static inline size_t plan_temp_bytes(uint64_t n) { return plan_block_offset(n) + align256(sizeof(PlanBlock)); }
// The cursors take the last 256 KiB below the plan block: inside the task lists' region (never below 1 MiB), which is written
// only after the last slot, and above the spine and the totals, which the scans of the later slots rewrite.  What lies there
// during the first scatter -- the last rows of prefix16 -- is dead once that scatter has run, and the cursors are set after it.
static inline uint32_t *plan_cursors(char *base, uint64_t n) { return (uint32_t *)(base + plan_block_offset(n) - PLAN_CURSOR_BYTES); }

template <int TW, bool BIG>
static void launch_plan_downsweep(const uint32_t *kin, uint32_t *kout, const LsbWorkspace &ws, const uint32_t *slot_shift,
                                  const PassParams &p, hipStream_t s)
{
    hipLaunchKernelGGL((lsb_plan_downsweep_kernel<false, TW, BIG>), dim3(p.ds_grid), dim3(LSB_THREADS), 0, s, kin, kout, ws.totals,
                       ws.spine, ws.prefix16, slot_shift, p);
}

// one pass slot: upsweep, scan, downsweep (+ the partial last tile); `real`: a slot that scatters on both routes;
// `ups_real`: its upsweep counts on both routes too (slot 1's does so only when CLASSIC, which the host does not know)
static int lsb_plan_slot2(const uint32_t *kin, uint32_t *kout, const LsbWorkspace &ws, PlanBlock *plan, uint32_t *cursor,
                          const PassParams &p, hipStream_t s);
static int lsb_plan_slot(const uint32_t *kin, uint32_t *kout, const LsbWorkspace &ws, const uint32_t *slot_shift,
                         const uint32_t *slot_ups_skip, const PassParams &p, bool real, bool ups_real, hipStream_t s)
{
    {
        KernelTimer kt(ups_real ? GS_K_LSB_UPSWEEP : GS_K_OTHER, s);
        if (!p.f32_in && !p.xor_in)
            hipLaunchKernelGGL(lsb_plan_upsweep_kernel<true>, dim3(p.grid), dim3(LSB_THREADS), 0, s, kin, ws.spine, ws.prefix16, slot_shift,
                               slot_ups_skip, p);
        else
            hipLaunchKernelGGL(lsb_plan_upsweep_kernel<false>, dim3(p.grid), dim3(LSB_THREADS), 0, s, kin, ws.spine, ws.prefix16, slot_shift,
                               slot_ups_skip, p);
    }
    {   // (on a skipped slot the scan rescans the spine of the slot before: harmless, nothing reads it)
        if (const int e = lsb_scan_as(ws.spine, ws.totals, p.grid, s, real ? GS_K_LSB_SCAN : GS_K_OTHER)) return e;
    }
    {
        KernelTimer kt(real ? GS_K_LSB_DOWNSWEEP : GS_K_OTHER, s);
        if (p.n >= (uint32_t)LSB_TILE) {
            const int tw = (p.f32_in || p.f32_out) ? 2 : ((p.xor_in | p.xor_out) ? 1 : 0);
            const bool big = p.n > (1u << 30);
#define GS_PDS(TW_, BIG_) launch_plan_downsweep<TW_, BIG_>(kin, kout, ws, slot_shift, p, s)
            if (big) { if (tw == 2) GS_PDS(2, true); else if (tw == 1) GS_PDS(1, true); else GS_PDS(0, true); }
            else { if (tw == 2) GS_PDS(2, false); else if (tw == 1) GS_PDS(1, false); else GS_PDS(0, false); }
#undef GS_PDS
        }
        if (p.n % (uint32_t)LSB_TILE)
            hipLaunchKernelGGL((lsb_plan_downsweep_kernel<true, 2, true>), dim3(1), dim3(LSB_THREADS), 0, s, kin, kout, ws.totals,
                               (const uint32_t *)nullptr, (const uint16_t *)nullptr, slot_shift, p);
    }
    return (int)hipGetLastError();
}

// The second slot with the cursor switch on: the same three steps from the slot's own kernels, then the follow-up kernel.
// Its upsweep launch counts only when CLASSIC (when PLANNED it sets the cursors), so it is timed with the other such launches.
static int lsb_plan_slot2(const uint32_t *kin, uint32_t *kout, const LsbWorkspace &ws, PlanBlock *plan, uint32_t *cursor,
                          const PassParams &p, hipStream_t s)
{
    if (p.f32_in || p.f32_out || p.xor_in || p.xor_out) return hipErrorInvalidValue;   // a middle pass: keys travel twiddled
    if ((char *)cursor < (char *)ws.prefix16) return hipErrorInvalidValue;             // (never: see plan_cursors)
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(lsb_plan_upsweep2_kernel<true>, dim3(p.grid), dim3(LSB_THREADS), 0, s, kin, ws.spine, ws.prefix16, plan, cursor, p);
    }
    if (const int e = lsb_scan_as(ws.spine, ws.totals, p.grid, s, GS_K_LSB_SCAN)) return e;   // (cursor mode: nothing reads it)
    {
        KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
        if (p.n >= (uint32_t)LSB_TILE) {
            if (p.n > (1u << 30))
                hipLaunchKernelGGL((lsb_plan_scatter2_kernel<false, true>), dim3(p.ds_grid), dim3(LSB_THREADS), 0, s, kin, kout, ws.totals,
                                   ws.spine, ws.prefix16, plan, cursor, p);
            else
                hipLaunchKernelGGL((lsb_plan_scatter2_kernel<false, false>), dim3(p.ds_grid), dim3(LSB_THREADS), 0, s, kin, kout, ws.totals,
                                   ws.spine, ws.prefix16, plan, cursor, p);
        }
        if (p.n % (uint32_t)LSB_TILE)
            hipLaunchKernelGGL((lsb_plan_scatter2_kernel<true, true>), dim3(1), dim3(LSB_THREADS), 0, s, kin, kout, ws.totals,
                               (const uint32_t *)nullptr, (const uint16_t *)nullptr, plan, cursor, p);
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(lsb_plan_irregular_kernel, dim3(PLAN_IRR_CAP + (p.n % (uint32_t)LSB_TILE ? 1u : 0u)), dim3(LSB_THREADS), 0, s, kin,
                           kout, plan, cursor, p.n);
    }
    return (int)hipGetLastError();
}

// the look: one workgroup per CU at most, each with room for its 128 KiB table in the alternate buffer; its spine and
// prefix16 are those of a pass at shift 16 (lsb_make_params' grid)
static int lsb_plan_look(const uint32_t *keys, uint32_t *alt, const LsbWorkspace &ws, PlanBlock *plan, uint64_t n, const PassParams &tw,
                         hipStream_t s, uint32_t *mailbox = nullptr)
{
    const uint32_t parts = (uint32_t)(n / PLAN_WORDS < PLAN_LOOK_MAX_GRID ? n / PLAN_WORDS : PLAN_LOOK_MAX_GRID);
    const uint32_t chunks = lsb_make_params(n, 16, RADIX_BITS).grid;
    KernelTimer kt(GS_K_OTHER, s);
    hipLaunchKernelGGL(lsb_plan_look_kernel, dim3(parts), dim3(PLAN_LOOK_THREADS), 0, s, keys, alt, plan, ws.spine, ws.prefix16, (uint32_t)n,
                       chunks, tw.f32_in, tw.xor_in);
    hipLaunchKernelGGL(lsb_plan_reduce_kernel, dim3(PLAN_BLOCKS), dim3(RADIX), 0, s, alt, plan, parts);
    hipLaunchKernelGGL(lsb_plan_decide_kernel, dim3(PLAN_BLOCKS), dim3(RADIX), 0, s, plan, (uint32_t)n, parts, plan_cursor_enabled() ? 1u : 0u,
                       mailbox);
    return (int)hipGetLastError();
}

// The second slot of a sort that the host has seen to be PLANNED in cursor mode: the cursor set-up and the scatter of the full
// tiles, by the kernels that know their route, and the follow-up kernel, which also places the partial tile.  No scan (nothing
// reads it) and no partial-tile launch (it returns at once in this mode).
static int lsb_plan_slot2_cursor(const uint32_t *kin, uint32_t *kout, const LsbWorkspace &ws, PlanBlock *plan, uint32_t *cursor,
                                 const PassParams &p, hipStream_t s)
{
    if (p.f32_in || p.f32_out || p.xor_in || p.xor_out) return hipErrorInvalidValue;
    if ((char *)cursor < (char *)ws.prefix16) return hipErrorInvalidValue;
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(lsb_plan_cursor_init_kernel, dim3(PLAN_GROUPS / LSB_THREADS), dim3(LSB_THREADS), 0, s, plan, cursor);
    }
    if (p.n >= (uint32_t)LSB_TILE) {
        KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
        PassParams q = p;
        q.shift = 24;                                      // what the decide kernel wrote to shift[1] of a PLANNED sort
        if (p.n > (1u << 30))
            hipLaunchKernelGGL((lsb_plan_scatter2_cursor_kernel<true>), dim3(p.ds_grid), dim3(LSB_THREADS), 0, s, kin, kout, plan->irr, cursor, q);
        else
            hipLaunchKernelGGL((lsb_plan_scatter2_cursor_kernel<false>), dim3(p.ds_grid), dim3(LSB_THREADS), 0, s, kin, kout, plan->irr, cursor, q);
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(lsb_plan_irregular_kernel, dim3(PLAN_IRR_CAP + (p.n % (uint32_t)LSB_TILE ? 1u : 0u)), dim3(LSB_THREADS), 0, s, kin,
                           kout, plan, cursor, p.n);
    }
    return (int)hipGetLastError();
}

// ---- the host's look at the decision.  The fixed sequence pays for both routes: a PLANNED sort launches two pass slots and
// up to eight local-sort kernels that find nothing, a CLASSIC one the cursor set-up, the follow-up kernel, the task builder
// and a finish over empty lists -- 0.3 ms at 2^30 keys, mostly workgroups that load one word and leave.  So, when the stream
// is not being captured: the look's decide kernel also writes the decision to a pinned host mailbox and an event is recorded
// behind it; the first slot, which is the same on both routes, is enqueued (milliseconds of work), and only then the host
// waits for the event and enqueues what the route needs.  The discipline is the MSB sort's (MsbPeek in gs_msb.hip): one
// mailbox per calling thread and device, released when the thread ends; under capture, with GS_LSB_PLAN_PEEK=0 (read once per
// process) and on any failure the fixed sequence runs, which is right for any data.
struct PlanPeek {
    uint32_t *host = nullptr, *dev = nullptr;
    hipEvent_t ev = nullptr;
    int device = -1;
    bool armed = false;
};
static bool plan_peek_enabled()
{
    static const bool on = [] { const char *e = getenv("GS_LSB_PLAN_PEEK"); return !(e && e[0] == '0'); }();
    return on;
}
constexpr int PLAN_PEEK_DEVICES = 16;
struct PlanPeekTable {
    PlanPeek slot[PLAN_PEEK_DEVICES];
    ~PlanPeekTable()
    {
        for (PlanPeek &pk : slot) {
            if (pk.ev) (void)hipEventDestroy(pk.ev);
            if (pk.host) (void)hipHostFree(pk.host);
        }
    }
};
// the calling thread's mailbox for the current device, or nullptr (then the caller runs the fixed sequence)
static PlanPeek *plan_peek_get(hipStream_t s)
{
    if (!plan_peek_enabled()) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
    thread_local PlanPeekTable table;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= PLAN_PEEK_DEVICES) { (void)hipGetLastError(); return nullptr; }
    PlanPeek &pk = table.slot[dev];
    if (pk.device != dev) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess ||
            hipHostGetDevicePointer(&d, h, 0) != hipSuccess ||
            hipEventCreateWithFlags(&pk.ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (h) (void)hipHostFree(h);
            pk.ev = nullptr;
            return nullptr;
        }
        pk.host = (uint32_t *)h; pk.dev = (uint32_t *)d; pk.device = dev;
    }
    // a look armed by an earlier call that returned early (an error between arm and wait): its kernel may still be about
    // to write the mailbox -- wait it out before the words are reused
    if (pk.armed) { (void)hipEventSynchronize(pk.ev); (void)hipGetLastError(); }
    pk.armed = false;
    return &pk;
}
// before the look is enqueued: the words the decide kernel will write
static uint32_t *plan_peek_clear(PlanPeek *pk)
{
    if (!pk) return nullptr;
    for (int i = 0; i < PLAN_PEEK_WORDS; ++i) ((volatile uint32_t *)pk->host)[i] = 0;   // route 0: not plausible
    return pk->dev;
}
// right behind the look's decide launch
static void plan_peek_arm(PlanPeek *pk, hipStream_t s)
{
    if (!pk) return;
    pk->armed = hipEventRecord(pk->ev, s) == hipSuccess;
    if (!pk->armed) (void)hipGetLastError();
}
struct PlanSeen { bool ok = false; uint32_t route = 0, tasks[MSB_NCLASS] = {0, 0, 0, 0}, cursor_mode = 0; };
// to be called once the first slot has been enqueued behind the look (the device is busy while the host waits).  The words
// must be plausible -- a route, all n keys counted when PLANNED and no more than n when CLASSIC, class counts that sum to the
// non-empty groups (to 0 when CLASSIC), none above its list -- or the caller runs the fixed sequence.
static PlanSeen plan_peek_wait(PlanPeek *pk, uint64_t n)
{
    PlanSeen seen;
    if (!pk || !pk->armed) return seen;
    pk->armed = false;
    if (hipEventSynchronize(pk->ev) != hipSuccess) { (void)hipGetLastError(); return seen; }
    uint32_t w[PLAN_PEEK_WORDS];
    for (int i = 0; i < PLAN_PEEK_WORDS; ++i) w[i] = ((const volatile uint32_t *)pk->host)[i];
    const uint32_t route = w[0], nonempty = w[2], total = w[7], mode = w[8];
    if (route != PLAN_PLANNED && route != PLAN_CLASSIC) return seen;
    // (CLASSIC after a counter of the look wrapped -- a group of 65536 keys or more in one workgroup: the words are those of
    // the wrapped counters, and fewer than n keys were counted)
    if (route == PLAN_PLANNED ? (uint64_t)total != n : (uint64_t)total > n) return seen;
    if (mode > 1u || (mode && route != PLAN_PLANNED)) return seen;
    uint64_t sum = 0;
    for (int c = 0; c < MSB_NCLASS; ++c) {
        if (w[3 + c] > plan_list_cap(n, c)) return seen;
        sum += w[3 + c];
    }
    if (route == PLAN_PLANNED ? sum != nonempty : sum != 0) return seen;
    seen.ok = true;
    seen.route = route;
    seen.cursor_mode = mode;
    for (int c = 0; c < MSB_NCLASS; ++c) seen.tasks[c] = w[3 + c];
    return seen;
}
// The finish's two launches behind the one-pass local sort (few distinct values, flagged) usually find nothing left: a
// workgroup per task, 16384 at 2^30 keys, then costs 23-29 us per launch for reading one word each.  They stride over the
// lists, so they get PLAN_FINISH_CAP workgroups at the most: the largest of 512 / 1024 / 2048 whose empty launch stays within
// 5 us (DESIGN.md section 3 has both ends: nothing left, and every group left).  GS_LSB_PLAN_FINISH_CAP=512|1024|2048
// (measurements; read once per process) overrides it.
#ifndef GS_PLAN_FINISH_CAP
#define GS_PLAN_FINISH_CAP 2048
#endif
constexpr uint32_t PLAN_FINISH_CAP = GS_PLAN_FINISH_CAP;
static_assert(PLAN_FINISH_CAP == 512 || PLAN_FINISH_CAP == 1024 || PLAN_FINISH_CAP == 2048, "the finish's cap");
static uint32_t plan_finish_cap()
{
    static const uint32_t v = [] {
        const char *e = getenv("GS_LSB_PLAN_FINISH_CAP");
        const unsigned long x = e ? strtoul(e, nullptr, 10) : 0ul;
        return x == 512ul || x == 1024ul || x == 2048ul ? (uint32_t)x : PLAN_FINISH_CAP;
    }();
    return v;
}
// The one-pass launch of the finish gets PLAN_ONEPASS_GRID workgroups at the most (gs_msb.hip, launch_local_sorts); with fewer
// workgroups than tasks they stride over the list.  Measured at 2^30 uniform keys, 65536 tasks of class 3, parent and new
// alternating in one process (tools/lookahead_ab.py): every value below the local sorts' own 16384 is
// slower, 32768 is no faster, and a workgroup per task -- 65536, the most groups there are -- is 0.13-0.15 ms faster.
// GS_LSB_PLAN_ONEPASS_GRID=512|1024|...|65536 (a power of two; measurements and tests; read once per process) overrides it;
// any other value is ignored.  gs_lsb_plan_onepass_grid() returns the value in force.  GS_PLAN_ONEPASS_GRID=16384 builds the
// launch as it was.
#ifndef GS_PLAN_ONEPASS_GRID
#define GS_PLAN_ONEPASS_GRID 65536
#endif
constexpr uint32_t PLAN_ONEPASS_GRID = GS_PLAN_ONEPASS_GRID;
static constexpr bool plan_onepass_grid_ok(unsigned long x) { return x >= 512ul && x <= 65536ul && (x & (x - 1ul)) == 0ul; }
static_assert(plan_onepass_grid_ok(PLAN_ONEPASS_GRID), "the one-pass launch's grid");
static uint32_t plan_onepass_grid()
{
    static const uint32_t v = [] {
        const char *e = getenv("GS_LSB_PLAN_ONEPASS_GRID");
        const unsigned long x = e ? strtoul(e, nullptr, 10) : 0ul;
        return plan_onepass_grid_ok(x) ? (uint32_t)x : PLAN_ONEPASS_GRID;
    }();
    return v;
}
// gs_lsb_plan_peek_status: what the calling thread's last planned sort did
static thread_local uint32_t plan_peek_last[4] = {0, 0, 0, 0};

int lsb_plan_sort(char *base, uint32_t *d_keys[2], int *selector, uint64_t n, int descending, int key_type, hipStream_t s)
{
    const LsbWorkspace ws = lsb_carve(base, n);
    char *lists_end = base + plan_block_offset(n);
    PlanBlock *plan = (PlanBlock *)lists_end;
    PlanLists lists;
    for (int c = MSB_NCLASS - 1; c >= 0; --c) {
        lists.cap[c] = plan_list_cap(n, c);
        lists_end -= (size_t)lists.cap[c] * sizeof(MsbTask);
        lists.tasks[c] = (MsbTask *)lists_end;
    }
    int sel = *selector, e;
    PassParams tw{};
    lsb_twiddle_masks(key_type, descending, true, true, tw);
    PlanPeek *peek = plan_peek_get(s);
    e = lsb_plan_look(d_keys[sel], d_keys[sel ^ 1], ws, plan, n, tw, s, plan_peek_clear(peek));
    // (also when the look's launches failed: the decide kernel may have been enqueued and may still write the mailbox)
    plan_peek_arm(peek, s);
    if (e) return e;
    PlanSeen seen;   // (!ok: the fixed sequence)
    plan_peek_last[0] = plan_peek_last[1] = 0; plan_peek_last[2] = 4; plan_peek_last[3] = (1u << MSB_NCLASS) - 1u;
    // The buffer ping-pong counts four slots on every path: a slot that is not enqueued flips the selector like one that skips.
    for (int slot = 0; slot < 4; ++slot) {
        PassParams p = lsb_make_params(n, 0, RADIX_BITS);   // (the shift comes from the plan)
        lsb_twiddle_masks(key_type, descending, slot == 0, slot == 3, p);
        const uint32_t *kin = d_keys[sel];
        uint32_t *kout = d_keys[sel ^ 1];
        e = hipSuccess;
        if (seen.ok && seen.route == PLAN_CLASSIC)          // the host has seen CLASSIC: every slot is a real pass
            e = lsb_plan_slot(kin, kout, ws, &plan->shift[slot], &plan->ups_skip[slot], p, true, true, s);
        else if (seen.ok && slot >= 2)                      // the host has seen PLANNED: slots 3 and 4 do nothing
            ;
        else if (seen.ok && slot == 1 && seen.cursor_mode)
            e = lsb_plan_slot2_cursor(kin, kout, ws, plan, plan_cursors(base, n), p, s);
        else if (slot == 1 && plan_cursor_enabled())
            e = lsb_plan_slot2(kin, kout, ws, plan, plan_cursors(base, n), p, s);
        else
            e = lsb_plan_slot(kin, kout, ws, &plan->shift[slot], &plan->ups_skip[slot], p, slot < 2, slot == 1, s);
        if (e) return e;
        sel ^= 1;
        if (slot == 0) {
            // the first slot is enqueued: now the host may wait for the look (the device is busy with that slot)
            seen = plan_peek_wait(peek, n);
            if (seen.ok) {
                plan_peek_last[0] = 1; plan_peek_last[1] = seen.route; plan_peek_last[2] = seen.route == PLAN_PLANNED ? 2 : 4;
                plan_peek_last[3] = 0;
                for (int c = 0; c < MSB_NCLASS; ++c) plan_peek_last[3] |= seen.tasks[c] ? 1u << c : 0u;
            }
        }
    }
    if (seen.ok && seen.route == PLAN_CLASSIC) {            // the fourth pass has written the result
        *selector = sel;
        return hipSuccess;
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(lsb_plan_tasks_kernel, dim3(PLAN_BLOCKS), dim3(PLAN_BLOCK_GROUPS), 0, s, plan, lists);
    }
    if ((e = (int)hipGetLastError())) return e;
    if ((e = msb_local_sorts_in_place(plan->level, lists.tasks, PLAN_GROUPS, PLAN_GROUPS, d_keys[sel], PLAN_SORT_BITS, n, tw.f32_out,
                                      tw.xor_out, s, seen.ok ? seen.tasks : nullptr, plan_finish_cap(), plan_onepass_grid())))
        return e;
    *selector = sel;
    return hipSuccess;
}


bool lsb_plan_has_block(uint64_t n) { return plan_has_block(n); }
size_t lsb_plan_temp_bytes(uint64_t n) { return plan_temp_bytes(n); }
bool lsb_plan_applies(uint64_t n) { return plan_enabled() && plan_size_ok(n); }

}  // namespace gs

using namespace gs;

extern "C" {

int gs_lsb_plan_status(void *d_temp, uint64_t num_items, uint32_t out[8], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!d_temp || !out || num_items >= (1ull << 32)) return hipErrorInvalidValue;
    memset(out, 0, 8 * sizeof(uint32_t));
    if (!plan_enabled() || !plan_size_ok(num_items)) return hipSuccess;   // such sorts never look
    const PlanBlock *plan = (const PlanBlock *)(gs_ws_base(d_temp) + plan_block_offset(num_items));
    hipError_t e = hipMemcpyAsync(out, plan, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return (int)e;
}

// out[0]: the last sort's second scatter ran in cursor mode; out[1]: tiles its follow-up kernel placed (listed tiles and the
// partial tile); out[2]: the listed tiles alone; out[3]: 0.  All 0 when the sort was CLASSIC or the switch says stable.
int gs_lsb_plan_cursor_status(void *d_temp, uint64_t num_items, uint32_t out[4], void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!d_temp || !out || num_items >= (1ull << 32)) return hipErrorInvalidValue;
    memset(out, 0, 4 * sizeof(uint32_t));
    if (!plan_enabled() || !plan_size_ok(num_items)) return hipSuccess;
    const PlanBlock *plan = (const PlanBlock *)(gs_ws_base(d_temp) + plan_block_offset(num_items));
    uint32_t w[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(&w[0], &plan->cursor_mode, sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&w[1], &plan->irr[0], sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (w[0] == 1u) {
        out[0] = 1;
        out[2] = w[1];
        out[1] = w[1] + (num_items % (uint64_t)LSB_TILE ? 1u : 0u);
    }
    return hipSuccess;
}

// The calling thread's last planned sort.  out[0]: the host looked at the decision; out[1]: the route it read (0: no look);
// out[2]: pass slots enqueued, 2 or 4; out[3]: bit c set when class c's local sorts were enqueued.  All 0 before the first.
int gs_lsb_plan_peek_status(uint32_t out[4])
{
    if (!out) return hipErrorInvalidValue;
    memcpy(out, plan_peek_last, sizeof(plan_peek_last));
    return hipSuccess;
}

uint32_t gs_lsb_plan_finish_cap(void) { return plan_finish_cap(); }

uint32_t gs_lsb_plan_onepass_grid(void) { return plan_onepass_grid(); }

int gs_lsb_plan_look_only(void *d_temp, const void *d_keys, void *d_alt, uint64_t num_items, int key_type, int descending, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!d_temp || !d_keys || !d_alt || num_items >= (1ull << 32)) return hipErrorInvalidValue;
    if (!plan_enabled() || !plan_size_ok(num_items)) return hipErrorInvalidValue;   // such sorts never look
    char *base = gs_ws_base(d_temp);
    PassParams tw{};
    lsb_twiddle_masks(key_type, descending, true, true, tw);
    return lsb_plan_look((const uint32_t *)d_keys, (uint32_t *)d_alt, lsb_carve(base, num_items), (PlanBlock *)(base + plan_block_offset(num_items)),
                         num_items, tw, (hipStream_t)stream);
}

int gs_lsb_plan_layout(uint64_t num_items, uint64_t out[4])
{
    if (!out || num_items >= (1ull << 32) || !plan_enabled() || !plan_size_ok(num_items)) return hipErrorInvalidValue;
    char *base = (char *)(uintptr_t)GS_WS_ALIGN;   // (any aligned address: only the differences are used)
    const LsbWorkspace ws = lsb_carve(base, num_items);
    out[0] = (uint64_t)((char *)ws.spine - base);
    out[1] = (uint64_t)((char *)ws.prefix16 - base);
    out[2] = plan_block_offset(num_items);
    out[3] = lsb_make_params(num_items, 16, RADIX_BITS).grid;
    return hipSuccess;
}

}  // extern "C"
