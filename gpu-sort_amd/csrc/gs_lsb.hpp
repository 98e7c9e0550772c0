// gs_lsb.hpp -- geometry, pass parameters and host entry points of the LSB
// three-kernel pass, shared with the MSB driver (its top-byte partition is one
// LSB pass at shift 24).
#pragma once

#include "gs_host.hpp"

namespace gs {

constexpr int LSB_THREADS = 512;                     // 8 waves
constexpr int LSB_WAVES = LSB_THREADS / WAVE;
constexpr int LSB_KPT = 16;                          // keys per thread per tile
constexpr int LSB_TILE = LSB_THREADS * LSB_KPT;      // 8192 keys = 32 KiB
constexpr int LSB_CHUNK = LSB_WAVES;                 // tiles per chunk = waves per upsweep block
constexpr int MI355X_CUS = 256;
constexpr int MI355X_XCDS = 8;
// Tiles are handed out in groups of LSB_GROUP consecutive tiles; inside a group the blocks of one
// XCD take a contiguous slice (tile_of_item), so neighbouring digit runs meet in the same L2.
#ifndef LSB_GROUP
#define LSB_GROUP 512
#endif
constexpr uint32_t LSB_RESIDENT = LSB_GROUP;

struct PassParams {
    uint32_t n;          // number of keys
    uint32_t num_tiles;  // ceil(n / LSB_TILE)
    uint32_t grid;       // chunks = upsweep blocks = spine row length
    uint32_t ds_grid;    // downsweep blocks = full tiles
    uint32_t shift;      // digit = (key >> shift) & mask
    uint32_t bits;       // digit width (<= 8)
    uint32_t mask;
    int f32_in, f32_out;          // float twiddle on read / undo on write
    uint32_t xor_in, xor_out;     // uniform xor on read / write (sign flip, descending)
};

// Block i -> tile.  Blocks are dispatched in order, so the resident blocks work on
// consecutive tiles; inside every group of
// LSB_RESIDENT items the blocks of one XCD (same b % 8 under round-robin dispatch) take
// a contiguous slice.  Speed only: any bijection gives the same result.
__device__ __forceinline__ uint32_t tile_of_item(uint32_t i, uint32_t full_tiles)
{
    const uint32_t base = (i / LSB_RESIDENT) * LSB_RESIDENT;
    if (base + LSB_RESIDENT > full_tiles) return i;   // ragged last group: identity
    const uint32_t r = i - base;
    return base + (r % MI355X_XCDS) * (LSB_RESIDENT / MI355X_XCDS) + r / MI355X_XCDS;
}

// The same with groups as large as the array allows (the three-launch LSB downsweep, round 3): groups of 2^k items, k <= 13, the
// remainder cut into smaller powers of two the same way, so that arrays of any size keep XCD-contiguous slices.  In-process A/B
// on the same buffers at 2^30 keys (tools/ab_inproc.py): groups of 256 items 1.810 ms, 512 1.766-1.775, 1024 1.781, 2048 1.792,
// 4096 1.772, 8192 1.758, 32768 1.764, all items 1.743-1.756 ms per launch: slices of >= 1024 consecutive tiles per XCD are worth 1 %.
constexpr uint32_t LSB_WIDE_GROUP = 8192;
__device__ __forceinline__ uint32_t tile_of_item_wide(uint32_t i, uint32_t full_tiles)
{
    uint32_t base = 0, rem = full_tiles;
    for (;;) {
        const uint32_t G = rem >= LSB_WIDE_GROUP ? LSB_WIDE_GROUP : (1u << (31u - (uint32_t)__builtin_clz(rem | 1u)));
        if (G < 2u * MI355X_XCDS) return i;                 // a handful of tiles: identity
        const uint32_t span = (rem / G) * G;                // whole groups of this size
        if (i < base + span) {
            const uint32_t r = (i - base) % G;
            return i - r + (r % MI355X_XCDS) * (G / MI355X_XCDS) + r / MI355X_XCDS;
        }
        base += span; rem -= span;
        if (rem == 0) return i;                             // (i >= full_tiles: not a tile; callers guard)
    }
}

// Upsweep block i -> chunk: inside every group of LSB_UPSWEEP_GROUP blocks the blocks of one XCD take consecutive
// chunks (their totals are neighbours in the spine rows).  Speed only.
#ifndef GS_EXP_UPS_GROUP
#define GS_EXP_UPS_GROUP 256
#endif
constexpr uint32_t LSB_UPSWEEP_GROUP = GS_EXP_UPS_GROUP;
__device__ __forceinline__ uint32_t chunk_of_block(uint32_t b, uint32_t grid)
{
    const uint32_t base = (b / LSB_UPSWEEP_GROUP) * LSB_UPSWEEP_GROUP;
    if (base + LSB_UPSWEEP_GROUP > grid) return b;   // ragged last group: identity
    const uint32_t r = b - base;
    return base + (r % MI355X_XCDS) * (LSB_UPSWEEP_GROUP / MI355X_XCDS) + r / MI355X_XCDS;
}

// Pipelined pass (gs_lsb.hip, lsb_pipe_pass_kernel): the three steps of a pass run inside ONE launch, the upsweep a
// bounded distance ahead of the downsweep, so that the downsweep's re-read of the keys is served by the Infinity Cache.
struct PipeParams {
    uint32_t tag;                  // pass index + 1: marks the words this pass published (never 0)
    uint32_t lead_chunks;          // upsweep blocks dispatched before the first downsweep block (multiple of 8)
    uint32_t scan_rows;            // rows the scanner walks: the chunks, rounded up to whole scanner batches
    uint32_t next_shift, next_bits;   // digit of the NEXT pass, whose totals the upsweep gathers on the way (0 bits: none)
    uint32_t test_drop_chunk_plus1;   // test hook (GS_LSB_PIPE_TEST_DROP): the upsweep role of this chunk (+ 1) publishes nothing,
                                      // so the waits behind it give up -- tests/test_lsb_gpu.py::test_one_launch_pass_give_up_stores_nothing
};
constexpr uint32_t PIPE_LEAD_CHUNKS = 128;   // 1024 tiles = 32 MiB of keys ahead (re-read window of the Infinity Cache: < 2048 tiles)
constexpr uint32_t PIPE_SUB_BLOCKS = 72;     // 8 upsweep blocks (chunks) followed by the 64 downsweep blocks of 64 tiles
constexpr uint32_t PIPE_GROUP_BLOCKS = PIPE_SUB_BLOCKS * (LSB_GROUP / 64);

struct LsbWorkspace {
    uint32_t *spine;
    uint32_t *totals;
    uint16_t *prefix16;
    // pipelined passes: all zeroed once per sort
    uint32_t *cc;           // [chunks][256] chunk counts, tag in bits 31:28
    uint64_t *sc;           // [chunks][256] {tag, exclusive prefix over the earlier chunks}
    uint32_t *ptotals;      // [5][256] digit totals of pass q in row q (row 0 unused: the scan kernel writes `totals`)
    uint32_t *error_word;   // set if a bounded spin ever gave up
};

size_t lsb_temp_bytes(uint64_t n);
LsbWorkspace lsb_carve(void *temp, uint64_t n);
PassParams lsb_make_params(uint64_t n, int shift, int bits);
void lsb_twiddle_masks(int key_type, int descending, bool first, bool last, PassParams &p);
int lsb_upsweep(const uint32_t *keys, uint32_t *spine, uint16_t *prefix16, const PassParams &p, hipStream_t s);
int lsb_scan(uint32_t *spine, uint32_t *totals, uint32_t grid, hipStream_t s);
int lsb_scan_as(uint32_t *spine, uint32_t *totals, uint32_t grid, hipStream_t s, int timer_id);   // timed under another profiling id
int lsb_downsweep(const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, const uint32_t *spine,
                  const uint16_t *prefix16, const uint32_t *totals, const PassParams &p, hipStream_t s);
// the downsweep of one slice (p.n < 2^31 keys) of the 64-bit pass (gs_large.hip): spine / prefix16 / totals are the slice's
// own (lsb_upsweep + lsb_scan on it), dbase[256] the absolute u64 start of the slice's run of each digit in kout / vout
int lsb_downsweep64(const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, const uint32_t *spine,
                    const uint16_t *prefix16, const uint32_t *totals, const uint64_t *dbase, const PassParams &p, hipStream_t s);

// gs_lsb_plan.hip: the keys-only plan of gs_lsb_sort_u32 (full-width keys without values, sizes inside its window).
// lsb_plan_has_block: the workspace of n keys carries the plan block (lsb_plan_temp_bytes instead of lsb_temp_bytes);
// lsb_plan_applies: a keys-only sort of n keys on all 32 bits takes lsb_plan_sort.  `base` is the aligned workspace.
bool lsb_pipe_enabled();   // GS_LSB_MODE=pipe: such processes have no plan
bool lsb_plan_has_block(uint64_t n);
size_t lsb_plan_temp_bytes(uint64_t n);
bool lsb_plan_applies(uint64_t n);
int lsb_plan_sort(char *base, uint32_t *d_keys[2], int *selector, uint64_t n, int descending, int key_type, hipStream_t s);

// gs_wide.hip: digit totals of the last wide pass inside its workspace
const uint32_t *wide_totals_ptr(void *d_temp, uint64_t n);
// The digit of one 64-bit pass (gs_large.hip) and the key twiddle around it: digit = (key >> shift) & ((1 << bits) - 1) of
// the key mapped by key_type's order-preserving twiddle (complemented when descending), which is applied on read when `first`
// and undone on write when `last` (lsb_twiddle_masks' rule).  Keys between a first and a last pass stay twiddled.
struct LargeDigit {
    int shift, bits;
    int key_type, descending;
    bool first, last;
};

// gs_wide.hip: one slice (len < 2^31 elements) of the 64-bit pass over the wide element types (gs_large.hip).  The count
// runs the wide upsweep and the spine scan (digit totals of the slice into totals[256]); the scatter writes the slice
// through dbase[256], the absolute u64 start of its run of each digit in kout / vout.
void wide_slice_bytes(uint64_t S, size_t &spine, size_t &prefix);
int wide_slice_count(const void *kin, uint64_t len, int key_bytes, const LargeDigit &d, uint32_t *spine, uint16_t *prefix16,
                     uint32_t *totals, hipStream_t s);
int wide_slice_scatter(const void *kin, void *kout, const void *vin, void *vout, uint64_t len, int key_bytes, int val_bytes,
                       const LargeDigit &d, const uint32_t *spine, const uint16_t *prefix16, const uint64_t *dbase, hipStream_t s);
// gs_narrow.hip: one slice (len < 2^31 elements) of the 64-bit pass over 8- and 16-bit keys (gs_large.hip), the narrow
// counterparts of wide_slice_*: the spine of a slice is narrow_slice_spine_bytes(S, val_bytes) bytes (one u32 per digit and
// tile, no prefix16), d.key_type is the narrow key type (its width is narrow_key_bytes, 0 for every other type) and keys are
// never rewritten (d.first / d.last are ignored).  narrow_fill_large sorts 8-bit keys alone over all 8 bits by a histogram
// with u64 counters (counts[256]) and a fill, for n < 2^40; narrow_copy_bytes is the copy of begin_bit == end_bit.
int narrow_key_bytes(int key_type);
size_t narrow_slice_spine_bytes(uint64_t S, int val_bytes);
int narrow_slice_count(const void *kin, uint64_t len, int val_bytes, const LargeDigit &d, uint32_t *spine, uint32_t *totals, hipStream_t s);
int narrow_slice_scatter(const void *kin, void *kout, const void *vin, void *vout, uint64_t len, int val_bytes, const LargeDigit &d,
                         const uint32_t *spine, const uint64_t *dbase, hipStream_t s);
int narrow_fill_large(const void *kin, void *kout, uint64_t n, int key_type, int descending, uint64_t *counts, hipStream_t s);
int narrow_copy_bytes(const void *in, void *out, uint64_t bytes, hipStream_t s);
// gs_msb.hip: the wide MSB levels for the large sort (gs_large.hip).  msb_wide_finish sorts a group of m < 2^31 elements that
// lies in src (partitioned on the byte at `shift`, every byte above it equal; h_counts[256] its bucket sizes) and reports in
// *in_src whether the result landed in src (1) or in oth (0); the workspace is gs_msb_wide_temp_bytes(m) bytes, 256-byte aligned.
// A synchronous finish checks the overflow word of its lists.  msb_wide_overflow checks the word gs_msb_sort_wide left (at
// gs_ws_base of its d_temp).
int msb_wide_finish(void *d_temp, void *src_k, void *src_v, void *oth_k, void *oth_v, uint64_t m, int key_bytes, int val_bytes,
                    const uint64_t *h_counts, int shift, int key_type, hipStream_t s, int synchronize, int *in_src);
int msb_wide_overflow(void *d_temp, uint64_t n, int key_bytes, int val_bytes, hipStream_t s);

// single-workgroup stable sort of a small array (gs_msb.hip): n <= small_sort_capacity(pairs)
uint32_t small_sort_capacity(bool pairs);
int small_stable_sort(void *scratch, size_t scratch_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout,
                      uint32_t n, int begin_bit, int end_bit, int f32_in, uint32_t xor_in, int f32_out, uint32_t xor_out,
                      hipStream_t s);

}  // namespace gs
