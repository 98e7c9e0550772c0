// gs_msb_tasks.hpp -- the local-sort task lists of the MSB sort (gs_msb.hip): size classes, task and level records, and
// the host entry that runs the local sorts over lists somebody else has written.  Shared with the keys-only plan of
// the LSB sort (gs_lsb.hip), whose finish is these local sorts over the 65536 groups of equal top 16 bits.
#pragma once

#include "gs_host.hpp"

namespace gs {

constexpr int MSB_NCLASS = 4;                      // local-sort size classes (reference: 7-9 configs)
// local-sort classes: threads x keys per thread = capacity 2048, 4608, 9216, 17408.  The two big
// classes run 1024 threads so that two workgroups per CU give 32 waves.
#ifndef GS_LS3_THREADS
#define GS_LS3_THREADS 1024
#define GS_LS3_KPT 17
#endif
#ifndef GS_LS2_THREADS
#define GS_LS2_THREADS 512
#define GS_LS2_KPT 18
#endif
#ifndef GS_LS1_THREADS
#define GS_LS1_THREADS 512
#define GS_LS1_KPT 9
#endif
#ifndef GS_LS0_THREADS
#define GS_LS0_THREADS 512
#define GS_LS0_KPT 4
#endif
__host__ __device__ constexpr int msb_class_threads(int c) { return c == 0 ? GS_LS0_THREADS : c == 1 ? GS_LS1_THREADS : c == 2 ? GS_LS2_THREADS : GS_LS3_THREADS; }
__host__ __device__ constexpr int msb_class_kpt(int c) { return c == 0 ? GS_LS0_KPT : c == 1 ? GS_LS1_KPT : c == 2 ? GS_LS2_KPT : GS_LS3_KPT; }
__host__ __device__ constexpr uint32_t msb_class_cap(int c) { return (uint32_t)(msb_class_kpt(c) * msb_class_threads(c)); }
struct MsbTask { uint32_t offset, size, sort_bits, pad; };      // a range to finish with a local sort
struct MsbLevel {
    unsigned long long packed;           // hi32: buckets to partition at this level, lo32: their tiles
    uint32_t task_count[MSB_NCLASS];     // local-sort tasks emitted by this level's classification
    uint32_t flagged;                    // != 0: the one-pass local sort left tasks to the general kernel (a plain store:
                                         // thousands of atomics on one word would cost a millisecond)
    uint32_t overflow;                   // level 0's record only: != 0 once ANY device-side append of the sort was clamped by a list
                                         // capacity (a bucket, tile or task record dropped: the result is then wrong).  "Never by
                                         // sizing" (msb_max_*) is an argument; this word is the check.
    unsigned long long unused1;
    unsigned long long keys;             // level 0: the array's size (census)
    unsigned long long unused2;
    uint32_t census_blocks, pad;         // slots of MsbWs::census this level's classification wrote
};

// The local sorts of level record `level[0]` over the lists tasks[c] (level[0].task_count[c] records of class c, at most
// max_tasks each; level[1] must exist: the sample look reads its bucket count), in place in `keys`: every task's keys are
// in registers or LDS before its first store, and stores stay inside the task's range.  Keys are in twiddled form; the
// output twiddle is applied on the way out.  No host wait: worst-case grids (`bound` tasks per class at most), blocks
// that find no task exit.  `known_tasks`: the caller has read level[0].task_count on the host -- classes without tasks are
// not launched and the grids are exact.  `leftover_cap` != 0: at most that many workgroups for each of the two launches
// that take what the one-pass sort left (they stride over the lists); 0: no cap.  `onepass_cap` != 0: the most workgroups of
// the one-pass launch itself, in place of the local sorts' own 16384 (a value above that counts only with `known_tasks`).
int msb_local_sorts_in_place(MsbLevel *level, MsbTask *const tasks[MSB_NCLASS], uint32_t max_tasks, uint32_t bound, uint32_t *keys,
                             int sort_bits, uint64_t num_items, int f32_out, uint32_t xor_out, hipStream_t s,
                             const uint32_t *known_tasks = nullptr, uint32_t leftover_cap = 0u, uint32_t onepass_cap = 0u);

}  // namespace gs
