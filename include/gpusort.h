/*
 * gpusort.h -- C ABI of the MI355X-native radix sort (libgpusort.so).
 *
 * This is the drop-in boundary for the two sort drivers of
 * anilshanbhag/gpu-sort.  The reference has no FFI of its own (both sorts are
 * header templates instantiated in the caller's translation unit, SURVEY.md
 * 8b); each entry point below names the reference call it replaces.  All
 * citations are relative to the reference tree.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller;
 *   - return value: 0 (= hipSuccess) or a hipError_t value; nothing throws;
 *   - entry points are re-entrant given distinct streams and workspaces (tests/test_concurrency_gpu.py); `stream`
 *     is a hipStream_t passed as void*.  State outside the caller's buffers: a few switches read from the
 *     environment (most once per process; INTEGRATION.md lists them), and per host thread one pinned 64-byte
 *     mailbox + event per device the thread has run an MSB sort on (the "look" of DESIGN.md section 1), released
 *     when the thread ends; nothing else persists between calls;
 *   - LSB entry points only enqueue work on `stream` and return (like
 *     cub::DeviceRadixSort, dispatch_radix_sort.cuh:899-979);
 *   - counts are 64-bit in the signature; the current kernels index with
 *     32-bit offsets, so num_items must be < 2^32 (the reference caps at
 *     int / unsigned, device_radix_sort.cuh:599,606, gpu_radix_sort.h:526).
 *     The exceptions are gs_msb_sort_large_u32, gs_msb_sort_large_wide
 *     and the stable gs_lsb_sort_large (num_items < 2^40), the branch the
 *     reference left commented out (gpu_radix_sort.h:526-529).
 */
#ifndef GPUSORT_H_
#define GPUSORT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_VERSION 100

/* Key categories: the order-preserving key -> u32 map applied on the first
 * read and undone on the last write (cub::Traits<K>::TwiddleIn/Out,
 * lsb/cub/cub/util_type.cuh:966-974, 1009-1017, 1079-1089). */
enum gs_key_type {
    GS_KEY_U32 = 0,   /* identity                                  */
    GS_KEY_I32 = 1,   /* flip the sign bit                         */
    GS_KEY_F32 = 2,   /* negative: flip all bits; else flip sign   */
    GS_KEY_U64 = 3,   /* 64-bit keys: gs_lsb_sort_wide only        */
    GS_KEY_I64 = 4,
    GS_KEY_F64 = 5,
    GS_KEY_U8 = 6,    /* 8- and 16-bit keys: gs_lsb_sort_narrow/any */
    GS_KEY_I8 = 7,    /* (bool / unsigned char: U8; char / signed   */
    GS_KEY_U16 = 8,   /*  char: I8; unsigned short / short)         */
    GS_KEY_I16 = 9,
    GS_KEY_F16 = 10,  /* IEEE half, and                            */
    GS_KEY_BF16 = 11, /* bfloat16: the same kernels, another name  */
    GS_KEY_F8 = 12    /* every 8-bit sign-magnitude float: e4m3fn, e5m2 and their fnuz forms */
};
/* GS_KEY_F16 / BF16 / F8 (gs_lsb_sort_narrow, _narrow_large, _any and gs_segmented_sort_narrow) use GS_KEY_F32's map at the
 * key's own width W (16, 16, 8): image(k) = k ^ (sign bit of k set ? all W ones : the sign bit only); bit ranges
 * [begin_bit, end_bit) apply to that image.  The order is the one of GS_KEY_F32 / F64: negative NaNs first, ordered by their
 * bits, then -inf ... -0.0, +0.0 ... +inf, then positive NaNs, ordered by their bits.  This is not torch.sort's order ("all
 * NaNs last, -0 equal to +0").  Outputs hold the caller's bit patterns, NaN payloads included: keys are never rewritten. */

int         gs_version(void);
const char *gs_error_string(int err);

/* ------------------------------------------------------------------ LSB --
 * Stable least-significant-digit radix sort, 8-bit digits, three kernels per
 * pass (upsweep histogram -> spine scan -> downsweep scatter).
 * Replaces cub::DeviceRadixSort::SortKeys / SortPairs / SortKeysDescending /
 * SortPairsDescending, DoubleBuffer overloads
 * (lsb/cub/cub/device/device_radix_sort.cuh:248-272, 595-621, 754-780),
 * as called from lsb/sort.cu:36,42,59,65.                                   */

/* Bytes of temp storage for a sort of num_items (spine, digit totals and the
 * per-tile u16 prefixes: about 1.6 % of the key bytes).
 * Replaces the d_temp_storage==NULL size query
 * (dispatch_radix_sort.cuh:1094-1110).  has_values is accepted for symmetry;
 * like CUB with is_overwrite_okay the value path needs no extra scratch.
 *
 * Alignment, for every entry point of this header: d_temp may have ANY
 * alignment.  The workspace is carved from d_temp rounded up to 256 bytes,
 * and every *_temp_bytes query includes the 256 bytes of slack that rounding
 * may take (cub's AliasTemporaries, util_device.cuh:68-96), so exactly the
 * queried size is enough at any address.  Data arrays (keys, values, their
 * alternates and outputs, segment offsets, bucket counts) need the natural
 * alignment of their element; the 16-byte values of gs_lsb_sort_any and
 * gs_lsb_sort_narrow need 16 bytes.  A call writes only inside the arrays and the workspace it was
 * given, and a refused call (hipErrorInvalidValue) writes nothing.          */
size_t gs_lsb_temp_bytes(uint64_t num_items, int has_values);

/* d_keys[2] / d_vals[2] are the two halves of a DoubleBuffer
 * (util_type.cuh:785-817); *selector says which half is current on entry and
 * which half holds the result on return.  d_vals == NULL sorts keys only.
 * Both halves may be overwritten.  Sorts on key bits [begin_bit, end_bit).
 * Errors: hipErrorInvalidValue for a NULL/too-small workspace, bad bit range
 * or num_items >= 2^32 (util_device.cuh:90-93 behaviour).
 *
 * Keys only on all 32 bits, for num_items inside a size window (DESIGN.md
 * section 3, "keys-only plan"): the sort first reads the input once and
 * counts the keys of each of the 65536 values of the top 16 bits.  If every
 * such group fits the largest in-LDS local sort, two scatter passes (bits
 * 16-23, 24-31) and one local sort per group replace the four passes; if
 * not, the four passes run.  The decision is taken on the device, and the
 * selector and the result buffer are those of the four passes.
 * GS_LSB_KEYS_PLAN=classic (environment, read once per process) switches
 * the plan off.
 * The host's look: such a call BLOCKS the calling thread until the look at
 * the input has run on the device (0.8 ms at 2^30 keys on an idle stream,
 * plus whatever the stream holds before it) -- with the first scatter pass
 * already enqueued, so the device stays busy -- and then enqueues only the
 * launches that the route needs; the result does not depend on it.  Unless:
 * `stream` is being captured into a HIP graph, or GS_LSB_PLAN_PEEK=0 is set
 * (environment, read once per process), or the pinned mailbox cannot be had
 * or read; then one fixed launch sequence that serves both routes is
 * enqueued whatever the data and nothing waits on the host.  (A host wait is
 * not allowed while ANOTHER stream of the process is being captured in the
 * global capture mode: set GS_LSB_PLAN_PEEK=0 there.)                       */
int gs_lsb_sort_u32(void *d_temp, size_t temp_bytes,
                    uint32_t *d_keys[2], uint32_t *d_vals[2], int *selector,
                    uint64_t num_items, int begin_bit, int end_bit,
                    int descending, int key_type, void *stream);

/* Non-overwriting form (the plain-pointer overloads of cub::DeviceRadixSort,
 * lsb/cub/cub/device/device_radix_sort.cuh:156-180,503-527 with
 * is_overwrite_okay == false, dispatch_radix_sort.cuh:1099-1129): the input
 * arrays are left untouched, the result is written to d_*_out, and the extra
 * ping-pong buffers are part of the workspace.                              */
size_t gs_lsb_copy_temp_bytes(uint64_t num_items, int has_values);
int gs_lsb_sort_copy_u32(void *d_temp, size_t temp_bytes,
                         const uint32_t *d_keys_in, uint32_t *d_keys_out,
                         const uint32_t *d_vals_in, uint32_t *d_vals_out,
                         uint64_t num_items, int begin_bit, int end_bit,
                         int descending, int key_type, void *stream);

/* Wider element types of the DeviceRadixSort contract
 * (lsb/cub/test/test_device_radix_sort.cu:934-943,1244-1265): keys of
 * key_bytes = 4 or 8 (GS_KEY_U32..F32 / GS_KEY_U64..F64), values of val_bytes =
 * 0 (keys only), 4 or 8.  Same DoubleBuffer/selector semantics as
 * gs_lsb_sort_u32; bits [begin_bit, end_bit) with end_bit <= 8*key_bytes.
 * General kernels (gs_wide.hip); the u32 / (u32,u32) cases are served faster
 * by gs_lsb_sort_u32.                                                       */
size_t gs_lsb_wide_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes);
int gs_lsb_sort_wide(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2],
                     int *selector, uint64_t num_items, int key_bytes, int val_bytes,
                     int begin_bit, int end_bit, int descending, int key_type, void *stream);

/* Bring-up / test access to the three kernels of one pass (SURVEY.md 8a rows
 * L4-L6), all working on the same d_temp workspace (gs_lsb_temp_bytes):
 *   upsweep   -> spine[digit*grid + chunk] (u32 counts per chunk of
 *                tiles_per_chunk tiles) and prefix16[tile*256 + digit] (u16:
 *                count of the digit in the chunk's earlier tiles);
 *   scan      -> spine rows exclusive-scanned in place + totals[256];
 *   downsweep -> stable scatter of one pass.
 * gs_lsb_geometry reports the decomposition used for num_items so the oracle
 * can mirror it; gs_lsb_workspace_layout reports where the three arrays live
 * inside d_temp.                                                            */
void gs_lsb_geometry(uint64_t num_items, int has_values, uint32_t *grid, uint32_t *tile,
                     uint32_t *tiles_per_chunk);
int  gs_lsb_workspace_layout(void *d_temp, uint64_t num_items, uint32_t **d_spine,
                             uint32_t **d_totals, uint16_t **d_prefix16);
/* Pipelined passes (one launch per pass, the three steps as roles of its workgroups): every wait
 * inside such a launch is bounded; a wait that gave up sets a bit of the workspace's status word
 * (1 = a downsweep tile, 2 = the scanner) and the sort's output is then invalid.  Copies the word of
 * the last sort that used d_temp to *h_status after synchronising `stream` (0 = clean, also for
 * sorts that ran no pipelined pass).  Diagnostic: tests and benches read it.                      */
int  gs_lsb_pipe_status(void *d_temp, uint64_t num_items, uint32_t *h_status, void *stream);
/* What the keys-only plan of the last full-width keys-only gs_lsb_sort_u32 on d_temp decided, after
 * synchronising `stream`: out[0] = route (1 = two scatters + local sorts, 2 = the four passes),
 * out[1] = keys in the largest group of equal top 16 bits, out[2] = non-empty groups, out[3..6] =
 * local-sort tasks per size class (zeros on route 2), out[7] = keys counted.  With a group of 65536
 * keys or more a 16-bit counter of the look may wrap: the route is then 2, and out[1], out[2] and
 * out[7] are those of the wrapped counters.  All zeros for sizes outside the plan's window and when
 * the plan is switched off.  Diagnostic: tests read it.                                           */
int  gs_lsb_plan_status(void *d_temp, uint64_t num_items, uint32_t out[8], void *stream);
/* How the second scatter of that sort ran, after synchronising `stream`: out[0] = 1 when it claimed
 * its places with cursors and had no upsweep (route 1, unless GS_LSB_PLAN_SCATTER2=stable), out[1] =
 * tiles that its follow-up kernel placed key by key (tiles that straddle two runs of the first
 * scatter, and the partial last tile), out[2] = the straddling tiles alone, out[3] = 0.  All zeros
 * on route 2, with the stable scatter and wherever gs_lsb_plan_status reports zeros.  Diagnostic.  */
int  gs_lsb_plan_cursor_status(void *d_temp, uint64_t num_items, uint32_t out[4], void *stream);
/* What the host did in the calling thread's last full-width keys-only gs_lsb_sort_u32 inside the
 * plan's window (see "The host's look" at gs_lsb_sort_u32): out[0] = 1 if the host looked at the
 * decision, else 0 (stream under capture, GS_LSB_PLAN_PEEK=0, no mailbox); out[1] = the route it
 * read (0 without a look); out[2] = pass slots enqueued, 2 or 4; out[3] = bit c set when the local
 * sorts of size class c were enqueued (0xf without a look, 0 on route 2).  No device access, no
 * synchronisation; all zeros before the thread's first such sort.  Diagnostic: tests read it.      */
int  gs_lsb_plan_peek_status(uint32_t out[4]);
/* The most workgroups the plan's finish gives each of the two local-sort launches that take what the
 * one-pass sort left over (they stride over the task lists): 512, 1024 or 2048.  Tests size by it.  */
uint32_t gs_lsb_plan_finish_cap(void);
/* The most workgroups the plan's finish gives the one-pass local-sort launch itself (with fewer than
 * tasks they stride over the task lists): a power of two from 512 to 65536; built in is 65536, a
 * workgroup per task.  A value above 16384 counts only in sorts whose host has read the plan's
 * decision (not under stream capture or GS_LSB_PLAN_PEEK=0, which launch worst-case grids).
 * GS_LSB_PLAN_ONEPASS_GRID (read once per process) overrides the built-in value with one of these
 * eight; any other value is ignored.  Tests size by it.                                             */
uint32_t gs_lsb_plan_onepass_grid(void);
/* Test hooks of the keys-only plan.  gs_lsb_plan_look_only runs the look alone (the fused look, the
 * reduction of its tables and the decision) on a workspace of gs_lsb_temp_bytes(num_items) bytes and
 * returns without sorting: d_keys is read, the first num_items * 4 bytes of d_alt are scratch.  What
 * it leaves -- the spine and prefix16 of a pass on bits 16-23 and the plan block -- lies at the byte
 * offsets gs_lsb_plan_layout reports, counted from d_temp rounded up to 256 bytes: out[0] = spine
 * (u32 [256][grid]), out[1] = prefix16 (u16 [tiles][256]), out[2] = plan block (its first eight words
 * are gs_lsb_plan_status', the next four the digit positions of the pass slots, the next four the
 * flags "this slot's upsweep has nothing to do"), out[3] = grid.  Both return hipErrorInvalidValue for
 * null pointers and for sizes outside the plan's window (or when the plan is switched off).         */
int  gs_lsb_plan_look_only(void *d_temp, const void *d_keys, void *d_alt, uint64_t num_items,
                           int key_type, int descending, void *stream);
int  gs_lsb_plan_layout(uint64_t num_items, uint64_t out[4]);
int  gs_lsb_upsweep_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in,
                        uint64_t num_items, int shift, int bits, int descending,
                        int key_type_in, void *stream);
int  gs_lsb_scan_spine(void *d_temp, size_t temp_bytes, uint64_t num_items, void *stream);
int  gs_lsb_downsweep_u32(void *d_temp, size_t temp_bytes,
                          const uint32_t *d_keys_in, uint32_t *d_keys_out,
                          const uint32_t *d_vals_in, uint32_t *d_vals_out,
                          uint64_t num_items, int shift, int bits, int descending,
                          int key_type_in, int key_type_out, void *stream);

/* The rest of DeviceRadixSort's type contract (lsb/cub/test/test_device_radix_sort.cu:930-945,1244-1265): keys of 8, 16, 32
 * or 64 bits (key_type names width and category) with values of ANY size -- none (val_bytes 0), the 1- and 2-byte values of
 * TestBackend<KeyT, KeyT>, the 16-byte TestFoo (test_util.h:1004-1010), ... -- stable, ascending or descending, on the bits
 * [begin_bit, end_bit) of the key's own width.  Plain-pointer form: the input arrays are untouched, the result is written
 * to the output arrays (which must not alias the inputs; 16-byte values must be 16-byte aligned).  Built on the library's
 * stable sort of (order-preserving sort key, index) pairs and one gather (gs_any.hip); only enqueues work on `stream`.   */
size_t gs_lsb_any_temp_bytes(uint64_t num_items, int key_type, int val_bytes);
int gs_lsb_sort_any(void *d_temp, size_t temp_bytes, const void *d_keys_in, void *d_keys_out,
                    const void *d_vals_in, void *d_vals_out, uint64_t num_items, int key_type, int val_bytes,
                    int begin_bit, int end_bit, int descending, void *stream);

/* 8- and 16-bit keys on kernels of their own (gs_narrow.hip): key_type GS_KEY_U8 / GS_KEY_I8 / GS_KEY_U16 / GS_KEY_I16, or
 * the float categories GS_KEY_F16 / GS_KEY_BF16 (16 bits) / GS_KEY_F8 (8 bits) in the order stated at the enum, with
 * val_bytes 0, 1, 2, 4, 8 or 16.  The contract is gs_lsb_sort_any's, so a caller can move from one to the other: plain
 * pointers, the inputs are never written, the outputs must not alias the inputs, stable, ascending or descending, on the bits
 * [begin_bit, end_bit) of the key's own width (begin_bit == end_bit copies input to output in input order), num_items < 2^32
 * (0 succeeds with null pointers), only enqueues work on `stream` (no host synchronisation, allocation or read-back; calls
 * may follow each other on one stream with one workspace).  Every other key type or value size is refused with
 * hipErrorInvalidValue and its size query returns 0: those stay with gs_lsb_sort_any.  Keys and values move at their own
 * width: one 8-bit digit pass for 8-bit keys, two for 16-bit keys (only the passes that hold bits of the range run), and a
 * 256-bin histogram and fill, without a scatter, for 8-bit keys alone over all 8 bits.  The alignment paragraph above holds:
 * a u8 array may start at any byte address, a u16 array at any even one, values at a multiple of their size.
 * Workspace, with T = gs_lsb_narrow_tile(key_type, val_bytes) elements per tile (8192 for values of <= 4 bytes, 4096 /
 * 2048 for 8 / 16 bytes) and every term rounded up to 256 bytes:
 *   256 * 4 * max(1, ceil(num_items / T))  the spine, one u32 per digit and tile
 * + 256 * 4                                 the digit totals (the histogram of the fill path)
 * + 16-bit keys only: 2 * num_items + val_bytes * num_items   the intermediate keys and values of the pass in -> temp -> out
 * + 256 bytes of alignment slack.                                                                                       */
size_t gs_lsb_narrow_temp_bytes(uint64_t num_items, int key_type, int val_bytes);
int gs_lsb_sort_narrow(void *d_temp, size_t temp_bytes, const void *d_keys_in, void *d_keys_out,
                       const void *d_vals_in, void *d_vals_out, uint64_t num_items, int key_type, int val_bytes,
                       int begin_bit, int end_bit, int descending, void *stream);
/* elements per tile of the digit pass for this key type and value size (0: not served); tests sweep sizes around it */
uint32_t gs_lsb_narrow_tile(int key_type, int val_bytes);

/* ------------------------------------------------------------------ MSB --
 * Unstable most-significant-digit hybrid radix sort, ascending.
 * Replaces rdxsrt_unstable_sort<K,V,IndexT>
 * (msb/src/sort/gpu_radix_sort.h:197-507) as called from
 * msb/src/test.cu:53,55 and gpu_radix_sort.h:529,570.                        */

/* Workspace bytes (replaces RDXSRT_GPUDataManager sizing,
 * gpu_radix_sort.h:50-166; one allocation instead of eight). */
size_t gs_msb_temp_bytes(uint64_t num_items, int has_values);

/* d_keys/d_vals: input arrays (d_vals NULL = keys only); d_keys_alt /
 * d_vals_alt: scratch of the same size.  On return *d_sorted_keys /
 * *d_sorted_vals point at the arrays holding the result -- for 32-bit keys
 * these are the caller's INPUT arrays, as in the reference
 * (gpu_radix_sort.h:359-360, 505-506).  Enqueues on `stream` and, when
 * `synchronize` is nonzero, waits for completion like the reference does
 * (gpu_radix_sort.h:489-491).  Unless `stream` is being captured into a HIP
 * graph (or GS_MSB_PEEK=0 is set), the call also waits -- with the level's
 * scatter already enqueued, so the device stays busy -- until each level's
 * classification has run, to size or skip the next level's launches
 * (DESIGN.md section 1); the result does not depend on it.  (A host wait is
 * not allowed while ANOTHER stream of the process is being captured in the
 * global capture mode: set GS_MSB_PEEK=0 there.)                             */
int gs_msb_sort_u32(void *d_temp, size_t temp_bytes,
                    uint32_t *d_keys, uint32_t *d_vals, uint64_t num_items,
                    uint32_t *d_keys_alt, uint32_t *d_vals_alt,
                    uint32_t **d_sorted_keys, uint32_t **d_sorted_vals,
                    int key_type, void *stream, int synchronize);

/* The same sort for the wider element types the reference instantiates (RadixSortConfig<8,*>,
 * msb/src/sort/gpu_sort_config.h:179-198; msb/tests/test_sort_keys.cu:154-195, test_sort_pairs.cu:223-281): 64-bit keys
 * (GS_KEY_U64 / I64 / F64) with no, 32-bit or 64-bit values, and 32-bit keys with 64-bit values.  MSD hybrid like
 * gs_msb_sort_u32 (top byte by one stable pass, then byte levels on bucket lists, buckets of <= 8192 elements finished
 * by an LSD local sort in LDS); ascending, unstable; the result is in the caller's input arrays.                        */
size_t gs_msb_wide_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes);
int gs_msb_sort_wide(void *d_temp, size_t temp_bytes, void *d_keys, void *d_vals, uint64_t num_items,
                     void *d_keys_alt, void *d_vals_alt, int key_bytes, int val_bytes,
                     void **d_sorted_keys, void **d_sorted_vals, int key_type, void *stream, int synchronize);

/* The same sort as gs_msb_sort_u32 for num_items of 2^32 and more (up to 2^40): 32-bit keys (GS_KEY_U32 / I32 / F32) with
 * no (d_vals NULL) or 32-bit values; d_keys_alt / d_vals_alt are scratch of the same size; ascending, unstable; the result
 * is ALWAYS in the caller's input arrays d_keys / d_vals.  One stable partition on the top byte with 64-bit offsets
 * (keys -> alternates), then the buckets are finished in groups of < 2^32 keys by gs_msb_finish_u32; a bucket larger than
 * a group is partitioned again on its next byte.  Arrays of up to one group (2^31 keys) simply take
 * gs_msb_sort_u32.  The call BLOCKS the host: it reads the 256 bucket counts back after the first pass, and again after
 * every partition of an oversized bucket; with `synchronize` it also waits for the end of the sort.  While `stream` is
 * being captured into a HIP graph it returns hipErrorStreamCaptureUnsupported and enqueues nothing.
 * Errors: hipErrorInvalidValue for a NULL or too-small workspace, overlapping arrays, a bad key_type or
 * num_items >= 2^40; a synchronous call whose finish overflowed a device-side list returns hipErrorUnknown.
 * gs_msb_large_temp_bytes is a pure host function.                                                                    */
size_t gs_msb_large_temp_bytes(uint64_t num_items, int has_values);
int    gs_msb_sort_large_u32(void *d_temp, size_t temp_bytes,
                             uint32_t *d_keys, uint32_t *d_vals, uint64_t num_items,
                             uint32_t *d_keys_alt, uint32_t *d_vals_alt,
                             int key_type, void *stream, int synchronize);

/* The same for the wide element types of gs_msb_sort_wide, for num_items of 2^32 and more (up to 2^40): 64-bit keys
 * (GS_KEY_U64 / I64 / F64) with no (d_vals NULL, val_bytes 0), 32-bit or 64-bit values, and 32-bit keys (GS_KEY_U32 / I32 /
 * F32) with 64-bit values -- e.g. row ids for an argsort of a column of more than 2^32 rows.  (u32, none) and (u32, u32) are
 * gs_msb_sort_large_u32's and return hipErrorInvalidValue.  The contract is gs_msb_sort_large_u32's: ascending, unstable,
 * the result ALWAYS in d_keys / d_vals, the alternates scratch of the same size, the call blocks the host and refuses
 * stream capture (hipErrorStreamCaptureUnsupported, nothing enqueued), num_items == 0 needs no arguments.  The first pass
 * is the wide LSB pass with 64-bit output offsets; groups of <= 2^31 elements are finished by the wide MSB levels.  Arrays
 * of up to one group take gs_msb_sort_wide.  Errors: hipErrorInvalidValue for a NULL or too-small workspace, a bad
 * combination of key_bytes / val_bytes / key_type, missing alternates, values without a value alternate, overlapping
 * arrays (at their element sizes) or num_items >= 2^40; a synchronous call whose finish overflowed a device-side list
 * returns hipErrorUnknown.  gs_msb_large_wide_temp_bytes is a pure host function.                                    */
size_t gs_msb_large_wide_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes);
int    gs_msb_sort_large_wide(void *d_temp, size_t temp_bytes, void *d_keys, void *d_vals, uint64_t num_items,
                              void *d_keys_alt, void *d_vals_alt, int key_bytes, int val_bytes, int key_type,
                              void *stream, int synchronize);

/* The stable LSB sort for num_items of 2^32 and more (up to 2^40): gs_lsb_sort_wide's contract above 2^32.  Keys of
 * key_bytes = 4 (GS_KEY_U32 / I32 / F32) or 8 (GS_KEY_U64 / I64 / F64), values of val_bytes = 0 (d_vals NULL), 4 or 8;
 * stable, ascending or descending, on key bits [begin_bit, end_bit).  DoubleBuffer: both halves may be overwritten and
 * *selector flips once per 8-bit pass, ceil((end_bit - begin_bit) / 8) times.  The call only enqueues work on `stream`
 * (no host read-back: the 64-bit offsets are computed on the device), so it may be captured into a HIP graph.  One pass
 * per digit: per slice of 2^31 elements the LSB upsweep and spine scan, u64 digit starts over all slices, then the
 * downsweep of every slice through them.  Arrays of up to one slice take gs_lsb_sort_u32 ((4, 0),
 * (4, 4)) or gs_lsb_sort_wide with the same arguments, which give the same result.  num_items == 0 or begin_bit ==
 * end_bit is a no-op: it returns 0, needs no workspace and leaves *selector alone.  Errors (hipErrorInvalidValue, checked
 * before anything is enqueued, nothing written): a NULL or too-small workspace, a bad bit range, a bad combination of
 * key_bytes / val_bytes / key_type, a missing buffer half, values without val_bytes (or val_bytes without values),
 * overlapping arrays (at their element sizes) or num_items >= 2^40.  gs_lsb_large_temp_bytes is a pure host function:
 * about 2 % of the key bytes for 32-bit keys.                                                                           */
size_t gs_lsb_large_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes);
int    gs_lsb_sort_large(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2], int *selector,
                         uint64_t num_items, int key_bytes, int val_bytes, int begin_bit, int end_bit,
                         int descending, int key_type, void *stream);

/* gs_lsb_sort_narrow for num_items of 2^32 and more (up to 2^40): 8- and 16-bit keys (GS_KEY_U8 / I8 / U16 / I16 and
 * the float categories GS_KEY_F16 / BF16 / F8, which size and behave as U16 / U16 / U8 but for the order) with
 * values of 0, 1, 2, 4, 8 or 16 bytes -- e.g. a dictionary-coded column of more than 2^32 rows with u64 row ids.  The
 * argument list and the contract are gs_lsb_sort_narrow's: plain pointers, the inputs are never written, stable, ascending or
 * descending, on the bits [begin_bit, end_bit) of the key's own width (begin_bit == end_bit copies input to output),
 * num_items == 0 succeeds with null pointers, a u8 array may start at any byte address, a u16 array at any even one, values
 * at a multiple of their size, d_temp anywhere.  The call only enqueues work on `stream` (no host read-back, allocation or
 * synchronisation), so it may be captured into a HIP graph, and calls may follow each other on one stream with one
 * workspace.  One 64-bit pass per 8-bit digit of the range: per slice of 2^31 elements the narrow
 * upsweep and spine scan, u64 digit starts over all slices, then the downsweep of every slice through them; 16-bit keys over
 * more than 8 bits take two passes, in -> workspace -> out.  8-bit keys alone over all 8 bits take a histogram with 64-bit
 * counts and a fill.  Arrays of up to one slice take gs_lsb_sort_narrow with the same arguments, which gives the same result.
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written): every other key type or value size
 * (the size query returns 0 for those and for num_items >= 2^40), num_items >= 2^40, a bad bit range, a NULL or too-small
 * workspace, values without val_bytes (or val_bytes without values), a misaligned array, input and output arrays that share
 * a byte (at their element sizes).
 * Workspace: a pure host function of its arguments, a multiple of 256.  With S = 2^31 elements per slice, slices =
 * max(1, ceil(num_items / S)), T = gs_lsb_narrow_tile(key_type, val_bytes) and every term rounded up to 256 bytes:
 *   slices * 256 * 4 * ceil(S / T)          per slice, a spine sized for a full slice
 * + slices * 256 * 4                        the slices' digit totals
 * + slices * 256 * 8                        the slices' u64 digit starts
 * + 256 * 8                                 the u64 counts (the histogram of the fill path)
 * + 16-bit keys only: 2 * num_items + val_bytes * num_items   the intermediate keys and values of the pass in -> temp -> out
 * + 256 bytes of alignment slack;
 * or gs_lsb_narrow_temp_bytes(min(num_items, S), ...) where that is larger (arrays of up to one slice).                   */
size_t gs_lsb_narrow_large_temp_bytes(uint64_t num_items, int key_type, int val_bytes);
int    gs_lsb_sort_narrow_large(void *d_temp, size_t temp_bytes, const void *d_keys_in, void *d_keys_out,
                                const void *d_vals_in, void *d_vals_out, uint64_t num_items, int key_type,
                                int val_bytes, int begin_bit, int end_bit, int descending, void *stream);

/* ---------------------------------------------------------------- top k --
 * The first k elements of the stable sort, by radix select (gs_topk.hip): an ORDER BY ... LIMIT k, or
 * the k best of a column of scores with their row ids, without sorting the rest.  The result is defined by the sort: with S =
 * the output of gs_lsb_sort_copy_u32(..., 0, 32, descending, key_type) on the same input -- the stable sort on all 32 bits of
 * key_type's order-preserving image (GS_KEY_U32 / I32 / F32), reversed when descending -- d_keys_out[0..k) and
 * d_vals_out[0..k) are S[0..k), bit for bit.  Keys keep the caller's bit patterns (NaN payloads included); GS_KEY_F32 follows
 * the order stated at the enum (negative NaNs first and positive NaNs last ascending, so positive NaNs first descending; -0.0
 * before +0.0); where the cut falls inside a run of equal keys, the ones taken are those S puts first (ascending or
 * descending: the lowest input indices).  Three forms:
 *   keys only   d_vals_in == NULL and d_vals_out == NULL;
 *   pairs       both given: values travel with their keys;
 *   arguments   d_vals_in == NULL, d_vals_out != NULL: the values written are the elements' input indices (u32), an argsort
 *               of the top k.
 * has_values of the two queries is non-zero for pairs and arguments.
 * The contract is gs_lsb_sort_narrow's: plain pointers, the inputs are never written, the outputs must not share a byte with
 * the inputs or with each other, nothing outside [0, k) of the outputs is written, d_temp anywhere (the alignment paragraph
 * above holds), num_items < 2^32 and 1 <= k <= num_items (k == 0 or num_items == 0 returns 0, writes nothing and needs no
 * workspace).  The call only enqueues work on `stream` (no host read-back, allocation or synchronisation); the same kernels
 * are launched in the same order whatever the data (every decision is taken on the device), so it may be captured into a HIP
 * graph; calls may follow each other on one stream with one workspace, and two runs on the same input give identical bytes.
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written): a NULL or too-small workspace,
 * k > num_items, num_items >= 2^32, a key_type other than GS_KEY_U32 / I32 / F32, d_vals_in without d_vals_out, a NULL key
 * pointer, an array not aligned to 4 bytes, arrays that share a byte (inputs at num_items, outputs at k elements).
 * Cost: two reads of the input plus work proportional to k and to the elements that share the top byte of the k-th one, as
 * long as those fit the candidate list of C elements below (route 1); otherwise -- all keys in a narrow range, a heavy
 * hitter -- the later rounds read the input itself, seven reads in all (route 2).  An array that fits one workgroup
 * (<= 17408 elements) is sorted whole into the workspace and its first k copied out (route 3).  There is no "k too large to
 * pay" shortcut: a large k only makes the final sort of the k selected elements the larger part of the call, and a whole-array
 * sort inside the call would need a workspace of 20 bytes per element for every k, or a query that is not monotone in k.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in num_items and in k.  With tiles =
 * max(1, ceil(num_items / 8192)), chunks = ceil(tiles / 8), C = max(65536, num_items / 32), V = 2 with has_values else 1, and
 * every term rounded up to 256 bytes:
 *   4096                                      the state block, the histograms of rounds two to four, small-sort scratch
 * + 256 * 4 * chunks + 1024 + 256 * 2 * tiles the spine, digit totals and prefix16 of round one (the LSB upsweep at shift 24)
 * + 8 * tiles                                 two counts per source tile of the final select
 * + V * 4 * C                                 the candidate list: keys (and indices)
 * + V * 4 * k                                 the staging area: the k selected keys (and indices)
 * + has_values: 4 * k                         the sorted indices on their way through the gather of the pairs form
 * + gs_lsb_copy_temp_bytes(k, has_values)     the workspace of the final sort
 * + 256 bytes of alignment slack.                                                                                         */
size_t gs_topk_temp_bytes(uint64_t num_items, uint64_t k, int has_values);
int    gs_topk_u32(void *d_temp, size_t temp_bytes,
                   const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                   uint32_t *d_keys_out, uint32_t *d_vals_out,
                   uint64_t num_items, uint64_t k, int descending, int key_type, void *stream);
/* What the last gs_topk_u32 on d_temp (same num_items, k and has_values) decided, after synchronising `stream`:
 * out[0] = route (1 = candidate list, 2 = input re-read, 3 = whole-array sort of an array that fits one workgroup),
 * out[1] = image of S[k - 1], the k-th element (key_type's order-preserving u32, complemented when descending),
 * out[2] = elements whose image sorts strictly before it, out[3] = k - out[2], the number taken from its run of equal keys,
 * out[4] = elements that share its top byte, out[5..7] = 0.  All zeros for k == 0 or num_items == 0.  Diagnostic: tests and
 * benches read it.                                                                                                         */
int    gs_topk_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream);

/* ------------------------------------------------------- top k, 16-bit keys --
 * gs_topk_u32 for a flat array of 16-bit keys, its kernels instantiated for them (gs_topk.hip): the
 * best k of a column of bfloat16 or half scores with their row ids, without widening the keys or sorting the array.
 * key_type is GS_KEY_U16, GS_KEY_I16, GS_KEY_F16 or GS_KEY_BF16, in the order stated at the enum (GS_KEY_F32's map at width
 * 16: negative NaNs first, positive NaNs last, -0 before +0).  With S = the output of gs_lsb_sort_narrow(..., key_type,
 * val_bytes = 0 or 4, begin_bit 0, end_bit 16, descending) on the same input, d_keys_out[0..k) and d_vals_out[0..k) are
 * S[0..k), bit for bit: keys keep the caller's bit patterns, and where the cut falls inside a run of equal keys the lowest
 * input indices are taken.  Equivalently it is bit for bit what gs_topk_u32 gives on the array (uint32_t)key << 16 with the
 * key type widened (U16 -> U32, I16 -> I32, F16 / BF16 -> F32), the returned keys shifted right by 16, values and indices
 * unchanged (for F16 too: the order is sign-magnitude on the bits, whatever the exponent width).
 * Forms: gs_topk_u32's -- keys only; pairs, with u32 values; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 input
 * index).  has_values of the two queries is non-zero for the last two.
 * The contract is gs_topk_u32's: plain pointers, the inputs are never written, nothing outside [0, k) of the outputs is
 * written, d_temp anywhere, 1 <= k <= num_items < 2^32 (k == 0 or num_items == 0 returns 0, writes nothing and needs no
 * workspace: the query returns 0).  The call only enqueues work on `stream` (no host read-back, allocation or
 * synchronisation); the same kernels are launched in the same order whatever the data (every decision is taken on the
 * device), so it may be captured into a HIP graph on one plain stream; calls may follow each other on one stream with one
 * workspace, and two runs on the same input give identical bytes.
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written): a NULL or too-small workspace,
 * k > num_items, num_items >= 2^32, any other key_type, d_vals_in without d_vals_out, a NULL key pointer, a key array not
 * aligned to 2 bytes or a value array not aligned to 4, arrays that share a byte (2 bytes per key, 4 per value; inputs at
 * num_items elements, outputs at k).  A key array at an even address that is not a multiple of 4 is served like any other.
 * Cost: two digits of 8 bits where gs_topk_u32 has four.  Round one (the narrow upsweep on the image's top byte) and the
 * filter read the input once each, 2 bytes per key; one histogram round and the select then run over the candidate list of
 * C elements when the elements sharing the k-th one's top byte fit it (route 1), otherwise over the input itself, five reads
 * in all (route 2).  An array of one tile (num_items <= gs_lsb_narrow_tile(key_type, 4) = 8192) is sorted whole into the
 * workspace and its first k copied out (route 3).  The finish is gs_lsb_sort_narrow of the k selected (key, index) pairs.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in num_items and in k.  With tiles =
 * max(1, ceil(num_items / 8192)), C = max(65536, num_items / 32), hv = 1 with has_values else 0, and every term rounded up to
 * 256 bytes:
 *   4096                                      the state block, the histogram of round two, scratch
 * + 256 * 4 * tiles + 1024                    the spine (one column per tile) and the digit totals of round one
 * + 8 * tiles                                 two counts per source tile of the final select
 * + 2 * C + hv * 4 * C                        the candidate list: 16-bit keys (and u32 indices); route 3's copies, iota and
 *                                             sort workspace lie inside this area
 * + 2 * k + hv * 4 * k                        the staging area: the k selected keys (and indices)
 * + hv * 4 * k                                the sorted indices on their way through the gather of the pairs form
 * + gs_lsb_narrow_temp_bytes(k, GS_KEY_U16, hv ? 4 : 0)   the workspace of the final sort
 * + 256 bytes of alignment slack.                                                                                         */
size_t gs_topk_u16_temp_bytes(uint64_t num_items, uint64_t k, int has_values);
int    gs_topk_u16(void *d_temp, size_t temp_bytes,
                   const uint16_t *d_keys_in, const uint32_t *d_vals_in,
                   uint16_t *d_keys_out, uint32_t *d_vals_out,
                   uint64_t num_items, uint64_t k, int descending, int key_type, void *stream);
/* gs_topk_status for gs_topk_u16: out[0] = route (1, 2 or 3), out[1] = the 16-bit image of S[k - 1], complemented when
 * descending, in the low 16 bits, out[2] = elements whose image sorts strictly before it, out[3] = k - out[2], out[4] =
 * elements that share its top byte, out[5..7] = 0.  All zeros for k == 0 or num_items == 0.                                */
int    gs_topk_u16_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream);

/* ------------------------------------------------------- top k, 64-bit keys --
 * gs_topk_u32 for a flat array of 64-bit keys (gs_topk.hip): the ORDER BY ... LIMIT k of an int64 id or
 * timestamp column, of double scores, of 64-bit hashes, without sorting the column.  key_type is GS_KEY_U64, GS_KEY_I64 or
 * GS_KEY_F64.  With S = the output of gs_lsb_sort_wide (key_bytes 8, val_bytes 0 or 4, bits 0..64, descending, key_type) on
 * the same input, d_keys_out[0..k) and d_vals_out[0..k) are S[0..k), bit for bit: keys keep the caller's bit patterns (NaN
 * payloads included), GS_KEY_F64 follows GS_KEY_F32's order (negative NaNs first and positive NaNs last ascending, -0 before
 * +0), and where the cut falls inside a run of equal keys the lowest input indices are taken.
 * Forms: gs_topk_u32's -- keys only; pairs, with u32 values; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 input
 * index).  has_values of the two queries is non-zero for the last two.
 * The contract is gs_topk_u32's: plain pointers, the inputs are never written, nothing outside [0, k) of the outputs is
 * written, d_temp anywhere, 1 <= k <= num_items < 2^32 (k == 0 or num_items == 0 returns 0, writes nothing and needs no
 * workspace: the query returns 0).  The call only enqueues work on `stream`; the launches are a function of the arguments
 * alone (every decision is taken on the device), so it may be captured into a HIP graph on one plain stream; calls may follow
 * each other on one stream with one workspace, two runs on the same input give identical bytes, and no atomic decides a
 * position (the only global atomics are the integer adds of the histograms and the AND / OR of the reductions).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written): a NULL or too-small workspace,
 * k > num_items, num_items >= 2^32, any other key_type, d_vals_in without d_vals_out, a NULL key pointer, a key array not
 * aligned to 8 bytes or a value array not aligned to 4, arrays that share a byte (8 bytes per key, 4 per value; inputs at
 * num_items elements, outputs at k).
 * The way down.  With C = max(65536, num_items / 32), byte 7 the top byte of the 64-bit image, krem = k and M = all elements:
 *   1. A counting round over the input reads it once: it counts byte j of the image over M (first round: j = 7) and reduces
 *      the AND and the OR of the images of M.  It picks the digit d whose bucket holds the krem-th element, subtracts from krem
 *      the elements of M below d and narrows M to that bucket (c elements).  D is the number of such rounds.
 *   2. If c <= C the descent over the input stops: the bucket goes to the candidate list in input order (route 1).
 *   3. Otherwise the next round counts the next lower byte at which AND and OR of this round's M differ; the bytes between
 *      are constant over M, so over the bucket, and are filled into the k-th image from the AND without a round.  If no byte
 *      is left, M is the run of keys equal to the k-th image and longer than C (route 2): its first krem elements are staged
 *      directly from the input.  Otherwise go to 1.
 *   4. On route 1 the remaining bytes are found by histogram rounds over the list, one per byte (constant bytes are not
 *      skipped there), and the ordered select runs over the list.
 *   5. The finish is gs_lsb_sort_wide of the k staged (key, index) pairs inside the workspace and a copy-out; the pairs form
 *      also gathers.
 * There is no route 3: an array of one element takes the same launches, and num_items <= C always fits at D = 1.  Every
 * launch of the worst case is always enqueued -- eight input rounds and seven list rounds, about sixty launches with the
 * finish; the workgroups of a launch that the state block says is not needed return at once.
 * Passes over the input: exactly 2 when D == 1 -- round one is the wide upsweep at shift 56, whose spine and prefix16 place the
 * elements that the second read stages (everything before digit d, and the bucket: into the list on route 1, or its first
 * krem elements on route 2); D + 2 otherwise -- round one, the second read (which then is round two: it reduces AND / OR of
 * round one's M and of the bucket, and counts all seven lower bytes of the bucket, since the byte to count is known only
 * when the read is over), rounds three to D, then a count and a scatter that stage everything below the final bucket and
 * move the bucket.  D + 1 is not reached.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in num_items and in k.  With tiles =
 * max(1, ceil(num_items / 4096)), chunks = ceil(tiles / 8), C as above, hv = 1 with has_values else 0, and every term rounded
 * up to 256 bytes:
 *   221184                                    the state block, the AND / OR pairs, the histograms (those of the rounds over
 *                                             the input in 16 copies, which the picks sum)
 * + 256 * 4 * chunks + 1024 + 256 * 2 * tiles the spine, digit totals and prefix16 of round one (the wide upsweep at shift 56)
 * + 8 * tiles                                 two counts per source tile of a select
 * + 8 * C + hv * 4 * C                        the candidate list: keys (and indices)
 * + 2 * (8 * k) + hv * 2 * (4 * k)            the staged keys (and indices) and the second buffer of their sort
 * + gs_lsb_wide_temp_bytes(k, 8, hv ? 4 : 0)  the workspace of the final sort
 * + 256 bytes of alignment slack.
 * At num_items = 2^28, k = 2^20 with values that is 161 MiB, under an eighth of the 2 GiB of keys.                          */
size_t gs_topk_u64_temp_bytes(uint64_t num_items, uint64_t k, int has_values);
int    gs_topk_u64(void *d_temp, size_t temp_bytes,
                   const uint64_t *d_keys_in, const uint32_t *d_vals_in,
                   uint64_t *d_keys_out, uint32_t *d_vals_out,
                   uint64_t num_items, uint64_t k, int descending, int key_type, void *stream);
/* What the last gs_topk_u64 on d_temp (same num_items, k and has_values) decided, after synchronising `stream`:
 * out[0] = route (1 or 2), out[1], out[2] = low and high word of the image of S[k - 1] (complemented when descending),
 * out[3] = elements whose image sorts strictly before it, out[4] = k - out[3], out[5] = D, out[6] = passes over the input,
 * out[7] = elements of the bucket moved to the list (route 1) or of the tie run (route 2).  All zeros for k == 0 or
 * num_items == 0.                                                                                                         */
int    gs_topk_u64_status(void *d_temp, uint64_t num_items, uint64_t k, int has_values, uint32_t out[8], void *stream);

/* ------------------------------------------------------- top k of every row --
 * The k best of every row of a matrix (gs_topk_rows.hip): MoE routing, top-k sampling over a
 * vocabulary, beam search, re-ranking.  Row r is d_keys_in[r * row_stride .. r * row_stride + num_cols) (the values of the
 * pairs form use the same stride), and its result is exactly what gs_topk_u32 above writes for that row alone, bit for bit:
 * the first k of the stable sort on key_type's 32-bit image (GS_KEY_U32 / I32 / F32; complemented when descending), the
 * lowest column indices where the cut falls inside a run of equal keys, the caller's bit patterns kept (NaN payloads and the
 * order of the GS_KEY_F32 note included).  Row r's result goes to d_keys_out[r * k .. r * k + k) and the same range of
 * d_vals_out: the outputs are dense with stride k.  The three forms are gs_topk_u32's: keys only; pairs; arguments
 * (d_vals_in == NULL, d_vals_out != NULL), where the value written is the element's column index within its row (u32).
 * The contract is gs_topk_u32's: plain pointers, the inputs are never written (the stride gap is never read either),
 * nothing outside [0, num_rows * k) of the outputs is written, d_temp anywhere, enqueue-only (no host read-back, allocation
 * or synchronisation), the launches are a function of the arguments alone (gs_topk_rows_plan reports them), so the call may
 * be captured into a HIP graph; calls may follow each other on one stream with one workspace; two runs give identical
 * bytes.  num_rows == 0, num_cols == 0 or k == 0 returns 0, writes nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a
 * refused shape, the convention of gs_lsb_narrow_temp_bytes): k > num_cols, k > gs_topk_rows_max_k() (1024: such callers
 * keep gs_topk_u32 per row), row_stride < num_cols, num_rows * row_stride >= 2^32, num_rows * k >= 2^32, a key_type other
 * than GS_KEY_U32 / I32 / F32, d_vals_in without d_vals_out, a NULL key pointer, a NULL or too-small workspace, an array
 * not aligned to 4 bytes, arrays that share a byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at
 * num_rows * k).
 * Paths, by num_cols alone: up to 1024 columns one wave sorts a row in registers and stores its first k (path 1); up to
 * CH = 8192 one workgroup reads the row once, selects the k-th image by radix select in registers and LDS, compacts the k
 * selected (key, column) pairs in input order and sorts them with one wave (path 2); longer rows are cut into chunks of CH
 * columns, every chunk gives its first min(k, chunk length) as sorted (key, column) pairs to a candidate row in the
 * workspace, and the same kernel runs over the candidate rows, level after level, until a row fits one chunk (path 3).
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With
 * next(n) = (ceil(n / CH) - 1) * k + min(k, n - (ceil(n / CH) - 1) * CH), the candidates a row of n elements leaves,
 * n1 = next(num_cols) if num_cols > CH else 0, n2 = next(n1) if n1 > CH else 0, V = 2 with has_values else 1, and every term
 * rounded up to 256 bytes:
 *   V * 4 * num_rows * n1                     the candidate rows of the even levels: keys (and columns)
 * + V * 4 * num_rows * n2                     the candidate rows of the odd levels (later levels are shorter and alternate)
 * + 256 bytes of alignment slack.
 * Paths 1 and 2 copy no element into the workspace (n1 = n2 = 0).                                                          */
size_t   gs_topk_rows_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_u32(void *d_temp, size_t temp_bytes,
                          const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                          uint32_t *d_keys_out, uint32_t *d_vals_out,
                          uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                          int descending, int key_type, void *stream);
uint32_t gs_topk_rows_max_k(void);
/* What gs_topk_rows_u32 -- and gs_topk_rows_u16 below, which has the same geometry -- launches for a shape: a pure host
 * function (no device, no workspace, no synchronisation).
 * out[0] = path (1 = one wave per row, 2 = one workgroup per row, 3 = chunked), out[1] = select levels launched (1 on paths
 * 1 and 2), out[2] = CH, the elements one workgroup selects from, out[3] = chunks per row at level 0, out[4] = candidates per
 * row after level 0 (k on paths 1 and 2, n1 of the workspace formula on path 3), out[5] = gs_topk_rows_max_k(), out[6..7] = 0.
 * A refused shape (k > num_cols, k > max_k, num_rows * num_cols >= 2^32, num_rows * k >= 2^32) returns hipErrorInvalidValue
 * and all zeros; a no-op shape returns 0 and all zeros.                                                                    */
int      gs_topk_rows_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8]);

/* ------------------------------------------- top k of every row, 16-bit keys --
 * gs_topk_rows_u32 for 16-bit keys, its kernels instantiated for them (gs_topk_rows.hip): bfloat16 or half
 * scores of a router, a vocabulary or a beam, without widening them.  key_type is GS_KEY_U16, GS_KEY_I16, GS_KEY_F16 or
 * GS_KEY_BF16, in the order stated at the enum for gs_lsb_sort_narrow (GS_KEY_F32's map at width 16: negative NaNs first,
 * positive NaNs last, -0 before +0).  Row r of the result is exactly the first k of the stable sort of row r on the 16-bit
 * image (complemented when descending): the lowest column indices where the cut falls inside a run of equal keys, the
 * caller's bit patterns kept.  Equivalently it is bit for bit what gs_topk_rows_u32 gives on the matrix (uint32_t)key << 16
 * with the key type widened (U16 -> U32, I16 -> I32, F16 / BF16 -> F32), the returned keys shifted right by 16, values and
 * column indices unchanged (for F16 too: the order is sign-magnitude on the bits, whatever the exponent width).
 * Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 column index).  Values are u32 and sit
 * at the same row_stride counted in elements (row r's values start at d_vals_in + r * row_stride); the outputs are dense with
 * stride k.  The contract is gs_topk_rows_u32's: the inputs are never written, the values of the stride gap never influence a
 * result, nothing outside [0, num_rows * k) of the outputs is written, d_temp anywhere, enqueue-only (no host read-back,
 * allocation or synchronisation), the launches are a function of the arguments alone, so the call may be captured into a HIP
 * graph; calls may follow each other on one stream with one workspace; two runs give identical bytes.  num_rows == 0,
 * num_cols == 0 or k == 0 returns 0, writes nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a refused
 * shape): k > num_cols, k > gs_topk_rows_max_k() (1024), row_stride < num_cols, num_rows * row_stride >= 2^32,
 * num_rows * k >= 2^32, a key_type other than GS_KEY_U16 / I16 / F16 / BF16, d_vals_in without d_vals_out, a NULL key pointer,
 * a NULL or too-small workspace, a key array not aligned to 2 bytes or a value array not aligned to 4, arrays that share a
 * byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at num_rows * k; 2 bytes per key, 4 per value).
 * Geometry: gs_topk_rows_u32's, on purpose -- path 1 up to 1024 columns, path 2 up to CH = 8192, path 3 chunked with the same
 * next(n), gs_topk_rows_max_k() = 1024 -- so gs_topk_rows_plan above answers for both entry points.  Every key is read and
 * written with one 2-byte access, so any row_stride and any k, odd ones included, are served alike.
 * Workspace: candidate rows hold 16-bit keys and u32 columns.  With next(n), n1 and n2 as in gs_topk_rows_temp_bytes,
 * hv = 1 with has_values else 0, and every term rounded up to 256 bytes:
 *   2 * num_rows * n1                         the candidate keys of the even levels
 * + hv * 4 * num_rows * n1                    their columns
 * + 2 * num_rows * n2                         the candidate keys of the odd levels
 * + hv * 4 * num_rows * n2                    their columns
 * + 256 bytes of alignment slack.
 * Never more than gs_topk_rows_temp_bytes of the same arguments.  Paths 1 and 2 copy no element into the workspace.        */
size_t   gs_topk_rows_u16_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_u16(void *d_temp, size_t temp_bytes,
                          const uint16_t *d_keys_in, const uint32_t *d_vals_in,
                          uint16_t *d_keys_out, uint32_t *d_vals_out,
                          uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                          int descending, int key_type, void *stream);

/* ------------------------------------------- top k of every row, 64-bit keys --
 * gs_topk_rows_u32 for 64-bit keys, its kernels instantiated for them (gs_topk_rows.hip): a matrix of
 * int64 ids or timestamps, double scores or 64-bit hashes -- a per-group ORDER BY ... LIMIT k, per-query candidate lists scored
 * in double precision, a k-way merge of per-shard lists.  key_type is GS_KEY_U64, GS_KEY_I64 or GS_KEY_F64; doubles take the
 * order stated at the enum (negative NaNs first, positive NaNs last, -0 before +0).  Row r of the result is bit for bit what
 * gs_topk_u64 writes for that row alone: the first k of the stable sort of row r on the full 64-bit order-preserving image
 * (complemented when descending), the lowest column indices where the cut falls inside a run of equal keys, the caller's
 * bit patterns kept (NaN payloads included).  On the matrix (uint64_t)key << 32 of 32-bit keys, with the key type widened
 * (U32 -> U64, I32 -> I64, F32 -> F64), it gives what gs_topk_rows_u32 gives on the keys themselves, the returned keys
 * shifted right by 32, values and column indices unchanged.
 * Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 column index).  Values are u32 and sit
 * at the same row_stride counted in elements; the outputs are dense with stride k.  The contract is gs_topk_rows_u32's: the
 * inputs are never written, the values of the stride gap never influence a result, nothing outside [0, num_rows * k) of the
 * outputs is written, d_temp anywhere, enqueue-only (no host read-back, allocation or synchronisation, no global atomic), the
 * launches are a function of the arguments alone, so the call may be captured into a HIP graph; calls may follow each other
 * on one stream with one workspace; two runs give identical bytes.  num_rows == 0, num_cols == 0 or k == 0 returns 0, writes
 * nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a refused
 * shape): k > num_cols, k > gs_topk_rows_max_k() (1024), row_stride < num_cols, num_rows * row_stride >= 2^32,
 * num_rows * k >= 2^32, a key_type other than GS_KEY_U64 / I64 / F64, d_vals_in without d_vals_out, a NULL key pointer,
 * a NULL or too-small workspace, a key array not aligned to 8 bytes or a value array not aligned to 4, arrays that share a
 * byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at num_rows * k; 8 bytes per key, 4 per value).
 * Geometry: gs_topk_rows_u32's, on purpose -- path 1 up to 1024 columns, path 2 up to CH = 8192, path 3 chunked with the same
 * next(n), gs_topk_rows_max_k() = 1024 -- so gs_topk_rows_plan above answers for all three entry points.  What the width
 * adds: the kernels reduce the AND and the OR of a row's (or chunk's) images and leave out every digit pass of the wave sort
 * and every round of the select whose byte is the same in all of them, so int64 ids below 2^24, timestamps of one day or
 * widened 32-bit keys cost as many passes as they have bytes that differ, and a row of one key costs none.
 * Workspace: candidate rows hold 8-byte keys and u32 columns.  With next(n), n1 and n2 as in gs_topk_rows_temp_bytes,
 * hv = 1 with has_values else 0, and every term rounded up to 256 bytes:
 *   8 * num_rows * n1                         the candidate keys of the even levels
 * + hv * 4 * num_rows * n1                    their columns
 * + 8 * num_rows * n2                         the candidate keys of the odd levels
 * + hv * 4 * num_rows * n2                    their columns
 * + 256 bytes of alignment slack.
 * Never more than twice gs_topk_rows_temp_bytes of the same arguments.  Paths 1 and 2 copy no element into the workspace.  */
size_t   gs_topk_rows_u64_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_u64(void *d_temp, size_t temp_bytes,
                          const uint64_t *d_keys_in, const uint32_t *d_vals_in,
                          uint64_t *d_keys_out, uint32_t *d_vals_out,
                          uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                          int descending, int key_type, void *stream);

/* ------------------------------------------------ top k of every row, any k --
 * gs_topk_rows_u32 without the cap at gs_topk_rows_max_k() (gs_topk_rows.hip): the 2000 ... 12000 box
 * scores a detector keeps per image, a few thousand candidates per query, a per-group ORDER BY ... LIMIT 5000, a wide nucleus.
 * 1 <= k <= num_cols; everything else is gs_topk_rows_u32's contract word for word.  Row r of the result is bit for bit what
 * gs_topk_u32 writes for that row alone: the first k of the stable sort on key_type's 32-bit image (GS_KEY_U32 / I32 / F32;
 * complemented when descending), the lowest column indices where the cut falls inside a run of equal keys, the caller's bit
 * patterns kept (NaN payloads included).  Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32
 * column index).  Values are u32 at the same row_stride; the outputs are dense with stride k.  The inputs and the stride gap
 * are never written, the gap's contents never influence a result, nothing outside [0, num_rows * k) of the outputs and the
 * workspace is written, d_temp anywhere, enqueue-only (no host read-back, allocation or synchronisation), the launches are a
 * function of the arguments alone (gs_topk_rows_anyk_plan reports them), so the call may be captured into a HIP graph on one
 * stream; calls may follow each other on one stream with one workspace; two runs give identical bytes.  num_rows == 0,
 * num_cols == 0 or k == 0 returns 0, writes nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a refused
 * shape): k > num_cols, row_stride < num_cols, num_rows * row_stride >= 2^32 (the size query and the plan, which have no
 * stride, refuse num_rows * num_cols >= 2^32), num_rows * k >= 2^31 (the finish has int offsets), a key_type other than
 * GS_KEY_U32 / I32 / F32, d_vals_in without d_vals_out, a NULL key pointer, a NULL or too-small workspace, an array not
 * aligned to 4 bytes, arrays that share a byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at
 * num_rows * k).  A k of 1024 and below is served too, with gs_topk_rows_u32's result; that call remains the faster one there.
 * Paths, by num_cols alone.  Path 1, num_cols <= CH = 8192: one workgroup reads the row once, selects the k-th image in
 * registers and LDS and places the k selected (key, column) pairs, equal keys in column order, into the row's k output slots.
 * Path 2, longer rows: a radix select over all rows at once in three counting rounds on image bits 31-21, 20-10 and 9-0 (one
 * workgroup per row and slab of whole tiles of 8192 columns adds its LDS histogram to the row's 2048 bins; one workgroup per
 * row picks the bin), then per (row, tile) two counts, a scan per row and a scatter in column order: five reads of the matrix.
 * Both paths finish with gs_segmented_sort_u32 on the num_rows * k staged pairs with the regular offsets r * k, all 32 bits.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With T = ceil(num_cols /
 * 8192), hv = 1 with has_values else 0, p2 = 1 if num_cols > 8192 else 0, and every term rounded up to 256 bytes:
 *   32 * num_rows                             a record per row: k-th image, less, take, 0, matched after rounds one and two, 0, 0
 * + 4 * (num_rows + 1)                        the offsets r * k of the finish
 * + p2 * 4 * 2048 * num_rows                  the rows' histograms
 * + p2 * 8 * num_rows * T                     two u32 counts per (row, tile)
 * + 4 * num_rows * k                          the second half of the staged keys (the first is d_keys_out)
 * + hv * 4 * num_rows * k                     the second half of the columns (the first is d_vals_out in the arguments form)
 * + hv * 4 * num_rows * k                     the first half of the columns, used by the pairs form
 * + gs_segmented_temp_bytes(num_rows * k, has_values, num_rows)
 * + 256 bytes of alignment slack.
 * No element of the matrix is copied into it except the k selected per row.                                               */
size_t   gs_topk_rows_anyk_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_anyk_u32(void *d_temp, size_t temp_bytes,
                               const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                               uint32_t *d_keys_out, uint32_t *d_vals_out,
                               uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                               int descending, int key_type, void *stream);
/* What gs_topk_rows_anyk_u32 launches for a shape: a pure host function.  out[0] = path (1 or 2), out[1] = kernel launches
 * before the finish (path 1: offsets and select; path 2: zero, offsets, three times count and pick, tile counts, scan,
 * scatter), out[2] = CH, out[3] = the tile (8192), out[4] = tiles per slab, out[5] = slabs per row, out[6] = tiles per row
 * (1, 1, 1 on path 1), out[7] = 0.  A refused shape (k > num_cols, num_rows * num_cols >= 2^32, num_rows * k >= 2^31)
 * returns hipErrorInvalidValue and all zeros; a no-op shape returns 0 and all zeros.                                       */
int      gs_topk_rows_anyk_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8]);
/* What the select found for one row of the last gs_topk_rows_anyk_u32 on d_temp with these arguments (read back after
 * synchronising `stream`; no kernel runs).  out[0] = path, out[1] = the image of that row's k-th element, out[2] = elements
 * whose image sorts strictly before it, out[3] = k - out[2], out[4] = elements that matched the prefix after round one
 * (path 2; 0 on path 1), out[5] = the same after round two, out[6..7] = 0.  All zeros for a no-op shape; hipErrorInvalidValue
 * for a refused shape, row >= num_rows, or a NULL d_temp or out.                                                            */
int      gs_topk_rows_anyk_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values,
                                  uint64_t row, uint32_t out[8], void *stream);

/* ------------------------------------- top k of every row, any k, 16-bit keys --
 * gs_topk_rows_anyk_u32 for 16-bit keys, its kernels instantiated for them (gs_topk_rows.hip): a wide
 * nucleus over bfloat16 logits, the 2000 ... 12000 half scores a detector keeps per image, a few thousand candidates per query,
 * without widening the matrix and without a loop of gs_topk_u16 over the rows.  key_type is GS_KEY_U16, GS_KEY_I16, GS_KEY_F16 or
 * GS_KEY_BF16, in the order stated at the enum for gs_lsb_sort_narrow (GS_KEY_F32's map at width 16: negative NaNs first,
 * positive NaNs last, -0 before +0).  1 <= k <= num_cols; everything else is gs_topk_rows_anyk_u32's contract word for word,
 * with 2-byte keys.  Row r of the result is bit for bit what gs_topk_u16 writes for that row alone: the first k of the stable
 * sort on the 16-bit order-preserving image (complemented at 16 bits when descending), the lowest column indices where the cut
 * falls inside a run of equal keys, the caller's bit patterns kept (NaN payloads included).  Equivalently it is what
 * gs_topk_rows_anyk_u32 gives on the matrix (uint32_t)key << 16 with the key type widened (U16 -> U32, I16 -> I32, F16 / BF16 ->
 * F32), the returned keys shifted right by 16, values and column indices unchanged.  A k of 1024 and below is served too, with
 * gs_topk_rows_u16's bytes; that call remains the faster one there.
 * Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 column index).  Values are u32 and sit at
 * the same row_stride counted in elements (row r's values start at d_vals_in + r * row_stride); the outputs are dense with
 * stride k.  The inputs and the stride gap are never written, the gap's contents never influence a result, nothing outside
 * [0, num_rows * k) of the outputs and the workspace is written, d_temp anywhere, enqueue-only (no host read-back, allocation or
 * synchronisation), the launches are a function of the arguments alone (gs_topk_rows_anyk_u16_plan reports them), so the call
 * may be captured into a HIP graph on one plain stream; calls may follow each other on one stream with one workspace; two runs
 * give identical bytes.  num_rows == 0, num_cols == 0 or k == 0 returns 0, writes nothing and needs no workspace (the query
 * returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 and the plan
 * zeros for a refused shape; the checks run in gs_topk_rows_anyk_u32's order): k > num_cols, row_stride < num_cols,
 * num_rows * row_stride >= 2^32 (the size query and the plan, which have no stride, refuse num_rows * num_cols >= 2^32),
 * num_rows * k >= 2^31 (the finish has int offsets), a key_type other than GS_KEY_U16 / I16 / F16 / BF16, d_vals_in without
 * d_vals_out, a NULL key pointer, a NULL or too-small workspace, a key array not aligned to 2 bytes or a value array not
 * aligned to 4, arrays that share a byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at num_rows * k;
 * 2 bytes per key, 4 per value).  A key pointer at 2 mod 4 and an odd row_stride are served like any other: every key is read
 * and written with one 2-byte access, as in gs_topk_rows_u16.
 * Paths, by num_cols alone, with gs_topk_rows_anyk_u32's geometry (CH = tile = 8192, four tiles per slab).  Path 1, num_cols <=
 * 8192: one workgroup reads the row once, selects the k-th image in registers and LDS in two byte rounds and places the k
 * selected (key, column) pairs, equal keys in column order, into the row's k output slots.  Path 2, longer rows: a radix select
 * over all rows at once in two counting rounds on image bits 15-8 and 7-0 (one workgroup per row and slab adds its LDS
 * histogram to the row's 256 bins; one workgroup per row picks the bin), then per (row, tile) two counts, a scan per row and a
 * scatter in column order: four reads of the matrix at 2 bytes a key.  The integer adds of the histograms are the only global
 * atomics; none decides a position.  Both paths finish with gs_segmented_sort_narrow on the num_rows * k staged pairs with the
 * regular offsets r * k, bits 0 .. 16, in the caller's key_type and direction.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With T = ceil(num_cols /
 * 8192), hv = 1 with has_values else 0, p2 = 1 if num_cols > 8192 else 0, and every term rounded up to 256 bytes:
 *   32 * num_rows                             a record per row: k-th image (low 16 bits), less, take, 0, matched after round one, 0, 0, 0
 * + 4 * (num_rows + 1)                        the offsets r * k of the finish
 * + p2 * 4 * 256 * num_rows                   the rows' histograms
 * + p2 * 8 * num_rows * T                     two u32 counts per (row, tile)
 * + 2 * num_rows * k                          the second half of the staged keys (the first is d_keys_out)
 * + hv * 4 * num_rows * k                     the second half of the columns (the first is d_vals_out in the arguments form)
 * + hv * 4 * num_rows * k                     the first half of the columns, used by the pairs form
 * + gs_segmented_narrow_temp_bytes(num_rows * k, GS_KEY_U16, 4 with has_values else 0, num_rows)
 * + 256 bytes of alignment slack.
 * Never more than gs_topk_rows_anyk_temp_bytes of the same arguments.  No element of the matrix is copied into it except the
 * k selected per row.                                                                                                      */
size_t   gs_topk_rows_anyk_u16_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_anyk_u16(void *d_temp, size_t temp_bytes,
                               const uint16_t *d_keys_in, const uint32_t *d_vals_in,
                               uint16_t *d_keys_out, uint32_t *d_vals_out,
                               uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                               int descending, int key_type, void *stream);
/* What gs_topk_rows_anyk_u16 launches for a shape: a pure host function.  out[0] = path (1 or 2), out[1] = kernel launches
 * before the finish (path 1: 2, offsets and select; path 2: 9, zero, offsets, twice count and pick, tile counts, scan,
 * scatter), out[2..6] = gs_topk_rows_anyk_plan's geometry words (CH, the tile, tiles per slab, slabs per row, tiles per row),
 * out[7] = 0.  A refused shape (k > num_cols, num_rows * num_cols >= 2^32, num_rows * k >= 2^31) returns hipErrorInvalidValue
 * and all zeros; a no-op shape returns 0 and all zeros.                                                                    */
int      gs_topk_rows_anyk_u16_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8]);
/* What the select found for one row of the last gs_topk_rows_anyk_u16 on d_temp with these arguments (read back after
 * synchronising `stream`; no kernel runs).  out[0] = path, out[1] = the 16-bit image of that row's k-th element, out[2] =
 * elements whose image sorts strictly before it, out[3] = k - out[2], out[4] = elements that share its top byte (matched after
 * round one; path 2, 0 on path 1), out[5..7] = 0.  All zeros for a no-op shape; hipErrorInvalidValue for a refused shape,
 * row >= num_rows, or a NULL d_temp or out.                                                                                 */
int      gs_topk_rows_anyk_u16_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values,
                                      uint64_t row, uint32_t out[8], void *stream);

/* ------------------------------------- top k of every row, any k, 64-bit keys --
 * gs_topk_rows_anyk_u32 for 64-bit keys (gs_topk_rows.hip): a matrix of int64 ids or timestamps, double
 * scores or 64-bit hashes and more than gs_topk_rows_max_k() of every row -- a per-group ORDER BY ... LIMIT 5000, a few thousand
 * candidates per query scored in double precision, a k-way merge of per-shard lists -- without a segmented sort of a copy of
 * the whole matrix and without a loop of gs_topk_u64 over the rows.  key_type is GS_KEY_U64, GS_KEY_I64 or GS_KEY_F64 (doubles
 * in the order of GS_KEY_F32 at width 64: negative NaNs first, positive NaNs last ascending, -0 before +0).  1 <= k <= num_cols;
 * everything else is gs_topk_rows_anyk_u32's contract word for word, with 8-byte keys.  Row r of the result is bit for bit what
 * gs_topk_u64 writes for that row alone: the first k of the stable sort on the 64-bit order-preserving image (complemented
 * when descending), the lowest column indices where the cut falls inside a run of equal keys, the caller's bit patterns kept
 * (NaN payloads included).  A k of 1024 and below is served too, with gs_topk_rows_u64's bytes; that call remains the faster
 * one there.
 * Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 column index).  Values are u32 and sit at
 * the same row_stride counted in elements; the outputs are dense with stride k.  The inputs and the stride gap are never
 * written, the gap is never read, nothing outside [0, num_rows * k) of the outputs and the workspace is written, d_temp
 * anywhere, enqueue-only (no host read-back, allocation or synchronisation), the launches are a function of the arguments
 * alone (gs_topk_rows_anyk_u64_plan reports them), so the call may be captured into a HIP graph on one plain stream; calls may
 * follow each other on one stream with one workspace; two runs give identical output bytes (the order inside a row's list in
 * the workspace may differ: see collect below).  num_rows == 0, num_cols == 0 or k == 0 returns 0, writes nothing and needs no
 * workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 and the plan
 * zeros for a refused shape; the checks run in gs_topk_rows_anyk_u32's order): k > num_cols, row_stride < num_cols,
 * num_rows * row_stride >= 2^32 (the size query and the plan, which have no stride, refuse num_rows * num_cols >= 2^32),
 * num_rows * k >= 2^31 (the finish has int offsets), a key_type other than GS_KEY_U64 / I64 / F64, d_vals_in without
 * d_vals_out, a NULL key pointer, a NULL or too-small workspace, a key array not aligned to 8 bytes or a value array not
 * aligned to 4, arrays that share a byte (inputs at (num_rows - 1) * row_stride + num_cols elements, outputs at num_rows * k;
 * 8 bytes per key, 4 per value).
 * Paths, by num_cols alone, with gs_topk_rows_anyk_u32's geometry (CH = tile = 8192, four tiles per slab).
 * Path 1, num_cols <= 8192: one workgroup reads the row once, selects the k-th image in registers and LDS (a byte round only
 * for a byte in which two images of the row differ) and places the k selected (key, column) pairs, equal keys in column order,
 * into the row's k output slots.  2 launches before the finish: offsets, select.
 * Path 2, longer rows: a radix select over all rows at once on 11-bit digits (2048 bins, 8 KB of LDS per count workgroup), with
 * a decision per row on the device.  L = min(8192, max(1024, num_cols / 8)) is the capacity of a row's list.
 *   A counting round at shift s (the first has s = 53): one workgroup per (row, slab) histograms (image >> s) & 2047 over the
 *   elements of the row whose image matches the row's prefix on the bits at and above s + 11, and reduces the OR of those
 *   images and the OR of their complements (the AND is the complement of the latter; a zeroed word is neutral for both): per
 *   wave, in LDS, then one pair of 64-bit atomic ORs per workgroup.  The bins are added to the row's histogram with integer
 *   atomic adds.  Neither result depends on the order of the atomics.
 *   A pick, one workgroup per row: take the bin d that holds the krem-th element; set prefix bits [s, s + 11) to d; update less
 *   and krem; let c be the bin's count and v = (AND ^ OR) restricted to the bits below s -- AND and OR are those of the round's
 *   matched set, not of the bucket.  If s == 0 or v == 0, every element of the bucket equals the k-th image, whose bits below s
 *   come from the AND: the row is decided (a tie run, mode 2).  Else if c <= L the bucket goes to the row's list (mode 1).
 *   Else, with hb the highest set bit of v, the bits between hb and s are constant over the bucket and come from the AND, and
 *   the next round runs at s' = max(hb - 10, 0).  The pick clears the bins and the two reduction words.
 *   The shifts fall by at least 11 until they reach 0, so six rounds are the worst case: 53, <= 42, <= 31, <= 20, <= 9, 0.  All
 *   six (count, pick) pairs are always enqueued; a workgroup whose row is decided reads the row's record and returns at once.
 *   Collect, one workgroup per (row, tile), rows in mode 1 only: appends the images of the elements that match the full prefix
 *   to the row's list.  A workgroup claims its range from the row's cursor with ONE atomic add: that atomic decides positions
 *   in the list only; the list is read as a multiset and never reaches an output position.
 *   List select, one workgroup per row in mode 1: loads the <= L images as path 1 loads a row, selects the krem-th among them
 *   and writes the k-th image, less and take into the record.
 *   Then per (row, tile) two counts (before / equal to the k-th image), a scan per row and a scatter: group A in column order
 *   from 0, the first `take` of the tie run in column order from `less`.  No atomic decides an output position.
 *   19 launches before the finish: zero (records, offsets and histograms are one area), offsets, six times (count, pick),
 *   collect, list select, tile counts, scan, scatter.  A row that took D rounds is read D + 3 times in list mode and D + 2
 *   times for a tie run: uniform u64 D = 1; N(0, 1) doubles, int64 below 2^24 and the timestamps of one day D = 2 (their first
 *   round only learns AND and OR); a row of one key D = 1, a tie run.
 * Both paths finish with gs_segmented_sort_wide on the num_rows * k staged pairs with the regular offsets r * k, key_bytes 8,
 * val_bytes 0 or 4, bits 0 .. 64, in the caller's key_type and direction: eight passes end in the half they started from.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With T = ceil(num_cols /
 * 8192), hv = 1 with has_values else 0, p2 = 1 if num_cols > 8192 else 0, L as above, and every term rounded up to 256 bytes:
 *   64 * num_rows                             a record of sixteen words per row: the k-th image low, high; less; krem / take; the
 *                                             mode; D; the next shift; the list count; the OR word low, high; the OR of the
 *                                             complements low, high; c of the last pick; three zero words
 * + 4 * (num_rows + 1)                        the offsets r * k of the finish
 * + p2 * 4 * 2048 * num_rows                  the rows' histograms
 * + p2 * 8 * num_rows * T                     two u32 counts per (row, tile)
 * + p2 * 8 * L * num_rows                     the rows' lists (images only): never above an eighth of the dense matrix bytes
 * + 8 * num_rows * k                          the second half of the staged keys (the first is d_keys_out)
 * + hv * 4 * num_rows * k                     the second half of the columns (the first is d_vals_out in the arguments form)
 * + hv * 4 * num_rows * k                     the first half of the columns, used by the pairs form
 * + gs_segmented_wide_temp_bytes(num_rows * k, 8, 4 with has_values else 0, num_rows)
 * + 256 bytes of alignment slack.                                                                                          */
size_t   gs_topk_rows_anyk_u64_temp_bytes(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values);
int      gs_topk_rows_anyk_u64(void *d_temp, size_t temp_bytes,
                               const uint64_t *d_keys_in, const uint32_t *d_vals_in,
                               uint64_t *d_keys_out, uint32_t *d_vals_out,
                               uint64_t num_rows, uint64_t num_cols, uint64_t row_stride, uint64_t k,
                               int descending, int key_type, void *stream);
/* What gs_topk_rows_anyk_u64 launches for a shape: a pure host function.  out[0] = path (1 or 2), out[1] = kernel launches
 * before the finish (path 1: 2; path 2: 19, as listed above), out[2..6] = gs_topk_rows_anyk_plan's geometry words (CH, the
 * tile, tiles per slab, slabs per row, tiles per row), out[7] = L, the capacity of a row's list (0 on path 1).  A refused shape
 * (k > num_cols, num_rows * num_cols >= 2^32, num_rows * k >= 2^31) returns hipErrorInvalidValue and all zeros; a no-op shape
 * returns 0 and all zeros.                                                                                                  */
int      gs_topk_rows_anyk_u64_plan(uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values, uint32_t out[8]);
/* What the select found for one row of the last gs_topk_rows_anyk_u64 on d_temp with these arguments (read back after
 * synchronising `stream`; no kernel runs).  out[0] = path, out[1], out[2] = the low and the high word of the image of that
 * row's k-th element, out[3] = elements whose image sorts strictly before it, out[4] = k - out[3], out[5] = D, the counting
 * rounds the row took (0 on path 1), out[6] = how the descent ended (0 path 1, 1 from the row's list, 2 a tie run), out[7] =
 * elements put on the list (0 otherwise).  All zeros for a no-op shape; hipErrorInvalidValue for a refused shape,
 * row >= num_rows, or a NULL d_temp or out.                                                                                 */
int      gs_topk_rows_anyk_u64_status(void *d_temp, uint64_t num_rows, uint64_t num_cols, uint64_t k, int has_values,
                                      uint64_t row, uint32_t out[8], void *stream);

/* ------------------------------------------------ top k of every ragged segment --
 * The k best of every segment of a flat array, the segments given by device offsets (gs_topk_rows.hip, DESIGN.md section
 * 10k): per-query candidate lists, variable-length sequences, per-image box scores, the neighbour lists of a CSR graph.
 * The offsets are those of gs_segmented_sort_u32 (cub::DeviceSegmentedRadixSort).
 * Segment s is d_keys_in[b .. e) with b = max(d_begin_offsets[s], 0) and e = min(d_end_offsets[s], num_items); it is empty
 * when e <= b.  The clamping happens on the device.  With len = e - b and kept = min(k, len), d_keys_out[s * k .. s * k + kept)
 * and the same range of d_vals_out are exactly what gs_topk_u32 writes for that sub-array alone with k = kept, bit for bit:
 * the first kept of the stable sort on key_type's 32-bit image (GS_KEY_U32 / I32 / F32; complemented when descending), the
 * lowest positions where the cut falls inside a run of equal keys, the caller's bit patterns kept (the NaN order of the
 * GS_KEY_F32 note included).  d_counts_out[s] = kept (u32); the array may be NULL.  Output slots [s * k + kept, (s + 1) * k)
 * are NOT written.
 * Forms: keys only; pairs (d_vals_out gets d_vals_in[b + position]: d_vals_in is flat and indexed like the keys);
 * arguments (d_vals_in == NULL, d_vals_out != NULL), where the value written is the element's position within its segment,
 * counted from the clamped b, as u32 -- the column index of gs_topk_rows_u32.
 * Segments may come in any order, leave gaps, repeat and, up to CH = 8192 elements each, overlap freely (the input is only
 * read): a sliding window is a list of offsets.  The lengths of the segments LONGER than CH must together not exceed
 * num_items, which holds whenever those segments do not overlap.  Where they do exceed it, a long segment that finds no
 * room in the workspace is DROPPED: d_counts_out[s] = 0, nothing of it is written, and gs_topk_segmented_status counts it
 * (the room is claimed from cursors that only grow: after one dropped segment, later long ones may be dropped as well).
 * The contract is gs_topk_rows_u32's: plain pointers, inputs and offsets are never written, nothing is written outside
 * [0, num_segments * k) of the outputs, [0, num_segments) of the counts and the workspace, d_temp anywhere, enqueue-only (no
 * host read-back, allocation or synchronisation); the launches are a function of (num_items, num_segments, k, has_values)
 * alone (gs_topk_segmented_plan reports them without a device), so the call may be captured into a HIP graph on one plain
 * stream; calls may follow each other on one stream with one workspace; two runs give identical output bytes (the
 * workspace bytes may differ: the lists are filled in device order).  num_items == 0, num_segments == 0 or k == 0 returns 0,
 * writes nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a
 * refused shape): k > gs_topk_rows_max_k() (1024), num_items >= 2^31 (int offsets), num_segments * k >= 2^32, a key_type other
 * than GS_KEY_U32 / I32 / F32, d_vals_in without d_vals_out, NULL keys or NULL offsets, a NULL or too-small workspace, an array
 * not aligned to 4 bytes, arrays that share a byte (inputs at num_items elements, outputs at num_segments * k, the counts
 * and the offsets at num_segments; the two offset arrays, both only read, may share bytes with each other, as in
 * end = begin + 1).  k may exceed num_items or any segment's length: that is what kept is for.
 * Launches: the state block is zeroed; a classify kernel writes every count and sorts the segments by length into six lists
 * of records; four wave kernels take the segments of up to 64 / 256 / 512 / 1024 elements, one wave per segment (path 1 of
 * gs_topk_rows_u32); one kernel takes those of up to CH, one workgroup per segment (path 2); longer segments take three
 * launches: their (segment, chunk of CH) tasks are written, every task gives its first min(k, chunk length) as sorted
 * (key, position) pairs to the segment's candidate row (level 0 of path 3), and ONE workgroup per segment streams that row
 * with a running best k, CH - k new candidates per round.  The host leaves out only what the arguments exclude: no
 * workgroup or long-segment launches when num_items <= 1024, no long-segment launches when num_items <= CH.
 * Cost of a very long segment: its final is one workgroup's sequential rounds, ceil(len / CH) * k / (CH - k) of them (a
 * row that fits one chunk, ceil(len / CH) * k <= CH, is one round); a caller with a few huge segments keeps gs_topk_u32.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With S = num_segments,
 * n = num_items, Lmax = min(S, n / (CH + 1)), Tmax = n / CH + Lmax (0 when Lmax is 0), V = 2 with has_values else 1, a
 * record of 16 bytes (base, length, segment, first task slot: four u32), a task of 8 bytes (record, chunk: two u32), and
 * every term rounded up to 256 bytes:
 *   4096                                      the state block: list counts, the long segments' claim, the dropped word
 * + 5 * (16 * S)                              the four wave lists and the workgroup list, each sized for S records
 * + 16 * Lmax                                 the long records
 * + 8 * Tmax                                  the chunk tasks
 * + V * (4 * k * Tmax)                        the candidate rows: images (and positions), k per task slot
 * + 256 bytes of alignment slack.
 * The long-segment areas vanish when n <= CH (Lmax = Tmax = 0).                                                           */
size_t gs_topk_segmented_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values);
int    gs_topk_segmented_u32(void *d_temp, size_t temp_bytes,
                             const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                             uint32_t *d_keys_out, uint32_t *d_vals_out, uint32_t *d_counts_out,
                             uint64_t num_items, uint32_t num_segments,
                             const int32_t *d_begin_offsets, const int32_t *d_end_offsets,
                             uint64_t k, int descending, int key_type, void *stream);
/* What gs_topk_segmented_u32 -- and gs_topk_segmented_u16 / _u64 below, which have the same geometry -- launches for a shape: a pure
 * host function (no device, no workspace, no synchronisation).
 * out[0] = bit mask of the launch groups the call enqueues (bit 0 the wave kernels, bit 1 the workgroup kernel, bit 2 the
 * long-segment kernels), out[1] = kernel launches (6, 7 or 10: the zeroing and the classify kernel included), out[2] = CH,
 * out[3] = Lmax, out[4] = Tmax, out[5] = gs_topk_rows_max_k(), out[6..7] = 0.  A refused shape (k > max k, num_items >= 2^31,
 * num_segments * k >= 2^32) returns hipErrorInvalidValue and all zeros; a no-op shape returns 0 and all zeros.              */
int    gs_topk_segmented_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8]);
/* What the last gs_topk_segmented_u32, _u16 or _u64 on d_temp (same num_items, num_segments, k and has_values)
 * decided (the state block is the first term of every workspace, so a workspace of any entry point is read as it is), after
 * synchronising `stream`: out[0..3] = segments in the four wave lists (<= 64, <= 256, <= 512, <= 1024 elements), out[4] =
 * the workgroup list (1025 .. CH), out[5] = the long list (> CH, dropped ones not counted), out[6] = chunk tasks, out[7] =
 * dropped segments.  All zeros for a no-op shape.  Diagnostic: tests and benches read it.                                   */
int    gs_topk_segmented_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values,
                                uint32_t out[8], void *stream);

/* ----------------------------------------- top k of every ragged segment, any k --
 * gs_topk_segmented_u32 without the cap at gs_topk_rows_max_k() (gs_topk_rows.hip): the 2000 ... 12000
 * box scores a detector keeps per image, a few thousand candidates per query, a per-group ORDER BY ... LIMIT 5000, where the
 * lists rarely have equal lengths.  1 <= k; everything else is gs_topk_segmented_u32's contract word for word.
 * Segment s is d_keys_in[b .. e) with b = max(d_begin_offsets[s], 0) and e = min(d_end_offsets[s], num_items); it is empty
 * when e <= b.  The clamping happens on the device.  With len = e - b and kept = min(k, len), d_keys_out[s * k .. s * k + kept)
 * and the same range of d_vals_out are exactly what gs_topk_u32 writes for that sub-array alone with k = kept, bit for bit:
 * the first kept of the stable sort on key_type's 32-bit image (GS_KEY_U32 / I32 / F32; complemented when descending), the
 * lowest positions where the cut falls inside a run of equal keys, the caller's bit patterns kept (the NaN order of the
 * GS_KEY_F32 note included).  d_counts_out[s] = kept (u32); the array may be NULL.  Output slots [s * k + kept, (s + 1) * k)
 * are NOT written.
 * Forms: keys only; pairs (d_vals_out gets d_vals_in[b + position]: d_vals_in is flat and indexed like the keys);
 * arguments (d_vals_in == NULL, d_vals_out != NULL), where the value written is the element's position within its segment,
 * counted from the clamped b, as u32.
 * Segments may come in any order, leave gaps, repeat and, up to CH = 8192 elements each, overlap freely (the input is only
 * read).  The lengths of the segments LONGER than CH must together not exceed num_items, which holds whenever those segments
 * do not overlap.  Where they do exceed it, a long segment that finds no room in the workspace is DROPPED: d_counts_out[s] =
 * 0, nothing of it is written, and gs_topk_segmented_anyk_status counts it (the room is claimed from cursors that only grow:
 * after one dropped segment, later long ones may be dropped as well).
 * Plain pointers, inputs and offsets are never written, nothing is written outside [0, num_segments * k) of the outputs,
 * [0, num_segments) of the counts and the workspace, d_temp anywhere, enqueue-only (no host read-back, allocation or
 * synchronisation); the launches are a function of (num_items, num_segments, k, has_values) alone
 * (gs_topk_segmented_anyk_plan reports them without a device), so the call may be captured into a HIP graph on one plain
 * stream; calls may follow each other on one stream with one workspace; two runs give identical output bytes (the
 * workspace bytes may differ: the lists are filled in device order); no atomic decides an output position.  num_items == 0,
 * num_segments == 0 or k == 0 returns 0, writes nothing and needs no workspace (the query returns 0).
 * Errors (hipErrorInvalidValue, checked before anything is enqueued, nothing written; the size query returns 0 for a
 * refused shape): num_items >= 2^31 (int offsets), num_segments * k >= 2^31 (the finish has int offsets), a key_type other
 * than GS_KEY_U32 / I32 / F32, d_vals_in without d_vals_out, NULL keys or NULL offsets, a NULL or too-small workspace, an array
 * not aligned to 4 bytes, arrays that share a byte (inputs at num_items elements, outputs at num_segments * k, the counts
 * and the offsets at num_segments; the two offset arrays, both only read, may share bytes with each other, as in
 * end = begin + 1).  k may exceed num_items or any segment's length: that is what kept is for.  A k of 1024 and below is
 * served too, with gs_topk_segmented_u32's bytes; gs_topk_segmented_u32 itself keeps refusing k > 1024.
 * Paths, decided on the device per segment by its length; one classify kernel sorts the segments into gs_topk_segmented_u32's
 * six lists, with the same Lmax / Tmax bounds and the same drop rule.  Up to 1024 elements: the four wave kernels of
 * gs_topk_segmented_u32 as they are; their output is final and sorted, and these segments skip the finish.  1025 .. CH: one
 * workgroup per segment reads it once, selects the kept-th image in registers and LDS and places the kept (key, position)
 * pairs, equal keys in position order, at s * k.  Longer: one radix select over all long segments at once on their
 * (segment, tile of 8192) tasks -- three counting rounds on image bits 31-21, 20-10 and 9-0 into 2048 bins per long segment
 * (a workgroup histograms a slab of consecutive tiles of one segment in LDS before it adds to the bins; one workgroup per
 * segment picks the bin), then two counts per task, a scan per segment and a scatter in position order: five reads of a
 * long segment.  The finish is gs_segmented_sort_u32 on the num_segments * k slots, all 32 bits, with the begin offsets s * k
 * and the end offsets s * k + kept that the two selects wrote (equal to the begin for empty, wave-class and dropped
 * segments, whose slots it therefore never touches); the pairs form ends with a gather over those ranges.  The host leaves
 * out only what the arguments exclude: the workgroup kernel, the long-segment kernels and the finish when num_items <= 1024,
 * the long-segment kernels when num_items <= CH.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  With S = num_segments,
 * n = num_items, Lmax = min(S, n / (CH + 1)), Tmax = n / CH + Lmax (0 when Lmax is 0), hv = 1 with has_values else 0, and
 * every term rounded up to 256 bytes:
 *   4096                                      the state block: list counts, the long segments' claim, the dropped word
 * + 5 * (16 * S)                              the four wave lists and the workgroup list, each sized for S records
 * + 16 * Lmax                                 the long records
 * + 8 * Tmax                                  the tile tasks
 * + 32 * Lmax                                 a record per long segment: k-th image, less, take, 0, matched after rounds one and two, 0, 0
 * + 4 * 2048 * Lmax                           the long segments' histograms
 * + 8 * Tmax                                  two u32 counts per task
 * + 2 * (4 * S)                               the begin and the end offsets of the finish
 * + 4 * S * k                                 the second half of the staged keys (the first is d_keys_out)
 * + hv * 4 * S * k                            the second half of the positions (the first is d_vals_out in the arguments form)
 * + hv * 4 * S * k                            the first half of the positions, used by the pairs form
 * + gs_segmented_temp_bytes(S * k, has_values, S)
 * + 256 bytes of alignment slack.
 * The histograms are at most about one byte per key (4 * 2048 * Lmax <= 8192 * n / 8193); only those of the long segments
 * in use are zeroed, on the device.  The long-segment areas vanish when n <= CH (Lmax = Tmax = 0).  No element of the input is
 * copied into the workspace except the kept ones.                                                                          */
size_t gs_topk_segmented_anyk_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values);
int    gs_topk_segmented_anyk_u32(void *d_temp, size_t temp_bytes,
                                  const uint32_t *d_keys_in, const uint32_t *d_vals_in,
                                  uint32_t *d_keys_out, uint32_t *d_vals_out, uint32_t *d_counts_out,
                                  uint64_t num_items, uint32_t num_segments,
                                  const int32_t *d_begin_offsets, const int32_t *d_end_offsets,
                                  uint64_t k, int descending, int key_type, void *stream);
/* What gs_topk_segmented_anyk_u32 launches for a shape: a pure host function (no device, no workspace, no synchronisation).
 * out[0] = bit mask of the launch groups the call enqueues (bit 0 the wave kernels, bit 1 the workgroup kernel, bit 2 the
 * long-segment kernels; by num_items, as in gs_topk_segmented_plan), out[1] = kernel launches before the finish (6: the
 * zeroing, the classify kernel and four wave kernels; 8 with the offsets and the workgroup kernel; 19 with the long segments'
 * tasks, the clearing of their histograms, three times count and pick, tile counts, scan and scatter), out[2] = CH, out[3] =
 * the tile (8192), out[4] = tiles per slab, out[5] = Lmax, out[6] = Tmax, out[7] = 0.  A refused shape (num_items >= 2^31,
 * num_segments * k >= 2^31) returns hipErrorInvalidValue and all zeros; a no-op shape returns 0 and all zeros.             */
int    gs_topk_segmented_anyk_plan(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values, uint32_t out[8]);
/* What the last gs_topk_segmented_anyk_u32 on d_temp (same num_items, num_segments, k and has_values) decided, after
 * synchronising `stream`, aggregated like gs_topk_segmented_status: out[0..3] = segments in the four wave lists (<= 64,
 * <= 256, <= 512, <= 1024 elements), out[4] = the workgroup list (1025 .. CH), out[5] = the long list (> CH, dropped ones not
 * counted), out[6] = tile tasks, out[7] = dropped segments.  All zeros for a no-op shape; hipErrorInvalidValue for a refused
 * shape or a NULL d_temp or out.  Diagnostic: tests and benches read it.                                                   */
int    gs_topk_segmented_anyk_status(void *d_temp, uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values,
                                     uint32_t out[8], void *stream);

/* -------------------------------- top k of every ragged segment, 16-bit keys --
 * gs_topk_segmented_u32 for 16-bit keys, its kernels instantiated for them (gs_topk_rows.hip): bfloat16 or
 * half candidate scores, logits of variable-length sequences, box scores, CSR weights, without widening them.  key_type is
 * GS_KEY_U16, GS_KEY_I16, GS_KEY_F16 or GS_KEY_BF16, in the order stated at the enum for gs_lsb_sort_narrow (GS_KEY_F32's map
 * at width 16: negative NaNs first, positive NaNs last, -0 before +0; the image complemented at 16 bits when descending).
 * With b, e, len and kept = min(k, len) as at gs_topk_segmented_u32, d_keys_out[s * k .. s * k + kept) and the same range of
 * d_vals_out are bit for bit what gs_topk_u16 writes for d_keys_in[b .. e) alone with k = kept; d_counts_out[s] = kept; the
 * slots behind are NOT written.  Equivalently it is what gs_topk_segmented_u32 gives on (uint32_t)key << 16 with the key type
 * widened (U16 -> U32, I16 -> I32, F16 / BF16 -> F32) and the returned keys shifted right by 16, values and positions
 * unchanged.  Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 position within the clamped
 * segment).
 * The contract is gs_topk_segmented_u32's, word for word, with 2-byte keys: the key arrays need 2-byte alignment, any even
 * address is served like any other and a segment may start at any element (every key is read and written with one 2-byte
 * access); the overlap checks count 2 bytes per key; values, counts and offsets stay u32 / int32, aligned to 4.  Unchanged:
 * the limits (k <= gs_topk_rows_max_k(), num_items < 2^31, num_segments * k < 2^32), the order of the checks, refused calls
 * write nothing and their size query is 0, no-op shapes return 0 with a size query of 0, segments of up to CH = 8192 elements
 * may overlap freely, the drop rule for long segments that find no room, enqueue-only and graph-capturable on one plain
 * stream, identical output bytes on two runs.
 * Geometry: gs_topk_segmented_u32's, on purpose -- six lists, CH = 8192, the same Lmax and Tmax, the same 6 / 7 / 10 launches
 * for a shape -- so gs_topk_segmented_plan above answers for both entry points, and gs_topk_segmented_status reads the state
 * of a workspace of this one as it is (the state block is the first term of both workspaces).
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  The candidate rows hold
 * 16-bit images and u32 positions.  With S, Lmax and Tmax as in gs_topk_segmented_temp_bytes, hv = 1 with has_values else 0,
 * and every term rounded up to 256 bytes:
 *   4096 + 5 * (16 * S) + 16 * Lmax + 8 * Tmax  the state block, the lists, the long records and the chunk tasks
 * + 2 * k * Tmax                              the candidate images, 16 bits wide
 * + hv * 4 * k * Tmax                         their positions
 * + 256 bytes of alignment slack.
 * The long-segment terms vanish when num_items <= CH.  Never more than gs_topk_segmented_temp_bytes of the same arguments.  */
size_t gs_topk_segmented_u16_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values);
int    gs_topk_segmented_u16(void *d_temp, size_t temp_bytes,
                             const uint16_t *d_keys_in, const uint32_t *d_vals_in,
                             uint16_t *d_keys_out, uint32_t *d_vals_out, uint32_t *d_counts_out,
                             uint64_t num_items, uint32_t num_segments,
                             const int32_t *d_begin_offsets, const int32_t *d_end_offsets,
                             uint64_t k, int descending, int key_type, void *stream);

/* -------------------------------- top k of every ragged segment, 64-bit keys --
 * gs_topk_segmented_u32 for 64-bit keys, its kernels instantiated for them (gs_topk_rows.hip): int64 ids
 * or timestamps, double scores or 64-bit hashes grouped by device offsets -- per-query candidate lists, a per-group
 * ORDER BY ... LIMIT k, per-sequence sampling with ragged lengths.  key_type is GS_KEY_U64, GS_KEY_I64 or GS_KEY_F64; doubles
 * take the order stated at the enum (negative NaNs first, positive NaNs last, -0 before +0).
 * With b, e, len and kept = min(k, len) as at gs_topk_segmented_u32, d_keys_out[s * k .. s * k + kept) and the same range of
 * d_vals_out are bit for bit what gs_topk_u64 writes for d_keys_in[b .. e) alone with k = kept; d_counts_out[s] = kept; the
 * slots behind are NOT written.  Equivalently it is what gs_topk_segmented_u32 gives on (uint64_t)key << 32 of 32-bit keys with
 * the key type widened (U32 -> U64, I32 -> I64, F32 -> F64) and the returned keys shifted right by 32, values and positions
 * unchanged.  Forms: keys only; pairs; arguments (d_vals_in == NULL, d_vals_out != NULL: the u32 position within the clamped
 * segment).
 * The contract is gs_topk_segmented_u32's, word for word, with 8-byte keys: the key arrays need 8-byte alignment (a pointer
 * at 4 mod 8 is refused with hipErrorInvalidValue and nothing is written); the overlap checks count 8 bytes per key; values,
 * counts and offsets stay u32 / int32, aligned to 4.  Unchanged: the limits (k <= gs_topk_rows_max_k(), num_items < 2^31,
 * num_segments * k < 2^32), the order of the checks, refused calls write nothing and their size query is 0, no-op shapes
 * return 0 with a size query of 0, segments of up to CH = 8192 elements may overlap freely, the drop rule for long segments
 * that find no room, enqueue-only and graph-capturable on one plain stream, identical output bytes on two runs.  A caller with
 * a few huge segments keeps gs_topk_u64 per segment.
 * Geometry: gs_topk_segmented_u32's, on purpose -- six lists, CH = 8192, the same Lmax and Tmax, the same 6 / 7 / 10 launches
 * for a shape -- so gs_topk_segmented_plan above answers for all three entry points, and gs_topk_segmented_status reads the
 * state of a workspace of this one as it is (the state block is the first term of all three workspaces).  What the width adds
 * is gs_topk_rows_u64's: the kernels reduce the AND and the OR of a segment's (or chunk's, or streaming round's) images and
 * leave out every digit pass and every select round whose byte is the same in all of them.
 * Workspace: a pure host function of its arguments, a multiple of 256, monotone in each of them.  The candidate rows hold
 * 8-byte images and u32 positions.  With S, Lmax and Tmax as in gs_topk_segmented_temp_bytes, hv = 1 with has_values else 0,
 * and _a() rounding up to 256 bytes:
 *   4096 + 5 * _a(16 * S) + _a(16 * Lmax) + _a(8 * Tmax) + _a(8 * k * Tmax) + hv * _a(4 * k * Tmax) + 256
 * (the state block, the five lists, the long records, the chunk tasks, the candidate images, their positions, the alignment
 * slack).  The long-segment terms vanish when num_items <= CH.  Never more than twice gs_topk_segmented_temp_bytes of the
 * same arguments.  */
size_t gs_topk_segmented_u64_temp_bytes(uint64_t num_items, uint32_t num_segments, uint64_t k, int has_values);
int    gs_topk_segmented_u64(void *d_temp, size_t temp_bytes,
                             const uint64_t *d_keys_in, const uint32_t *d_vals_in,
                             uint64_t *d_keys_out, uint32_t *d_vals_out, uint32_t *d_counts_out,
                             uint64_t num_items, uint32_t num_segments,
                             const int32_t *d_begin_offsets, const int32_t *d_end_offsets,
                             uint64_t k, int descending, int key_type, void *stream);

/* Census of the last gs_msb_sort_u32 that used d_temp (read back after synchronising `stream`): what every level
 * partitioned and what it handed to local sorts.  SURVEY.md 8d: the MSB path's algorithmic bytes are data-dependent --
 * "the harness must log the per-pass census and compute bytes from it": level 0 moves every key once (12 B/key), a level
 * L >= 1 reads its `keys` once for the histogram (4 B/key) and moves the ones outside heavy-hitter buckets (8 B/key;
 * 16 B/pair), heavy-hitter buckets are read once more (4 B/key), and every key is finished by exactly one local sort
 * (`task_keys`, 8 B/key; 16 B/pair), by the last level's scatter, or inside a heavy-hitter bucket.                     */
typedef struct gs_msb_level_census {
    uint64_t buckets;         /* buckets partitioned at this level (level 0: the whole array)            */
    uint64_t tiles;           /* their 8192-key tiles                                                     */
    uint64_t keys;            /* keys in them                                                             */
    uint64_t pivot_buckets;   /* of those, buckets finished by the heavy-hitter path                      */
    uint64_t pivot_keys;      /* keys in them                                                             */
    uint64_t task_keys;       /* keys handed to local sorts by this level's classification                */
    uint32_t tasks[4];        /* local-sort tasks per size class (2048 / 4608 / 9216 / 17408)             */
    uint32_t flagged;         /* != 0: some tasks needed the general local-sort plan                      */
    uint32_t overflow;        /* != 0: a device-side list of the sort overflowed and a record was dropped:  */
                              /* the result is WRONG (same word in all four records).  A synchronous        */
                              /* gs_msb_sort_u32 returns hipErrorUnknown in that case.                      */
} gs_msb_level_census;
int gs_msb_census(void *d_temp, uint64_t num_items, int has_values, gs_msb_level_census out[4], void *stream);
/* The same for the last gs_msb_sort_wide that used d_temp with these num_items, key_bytes and val_bytes (read back after
 * synchronising `stream`; no kernel runs).  A key of key_bytes bytes has key_bytes byte levels: out[L] for L < key_bytes
 * holds `buckets` and `tiles` (tiles of 4096 elements) partitioned at level L, `keys` in them (level 0: num_items), the
 * local-sort `tasks[0]` (<= 2048 elements) and `tasks[1]` (<= 8192) that level L's classification emitted, their
 * `task_keys`, and `flagged` / `overflow` as in gs_msb_census.  The wide sort has no heavy-hitter path and two size
 * classes: pivot_buckets, pivot_keys, tasks[2] and tasks[3] are 0.  The last level emits no tasks (its scatter finishes
 * every key it gets) and levels the data never reached are all zeros, as are the records of levels >= key_bytes.
 * An array of <= 8192 elements is one task and no classification runs: out[0] has buckets 1, tiles 1 or 2, keys
 * num_items and one task in its class, but task_keys 0.  num_items == 0: all zeros.  Errors: hipErrorInvalidValue for a
 * NULL d_temp or out, num_items >= 2^32 or a key_bytes / val_bytes combination gs_msb_sort_wide refuses.              */
int gs_msb_wide_census(void *d_temp, uint64_t num_items, int key_bytes, int val_bytes, gs_msb_level_census out[8], void *stream);
/* Capacities of the workspace's device-side lists for num_items (records): buckets a level may hold, local-sort tasks per
 * size class, tile records.  The sizing argument (gs_msb.hip, msb_max_*): a level's buckets are > the largest local sort
 * each; a task is >= 3000 keys or followed by something that did not merge with it (<= 2n / 3000, + 256 per bucket's
 * ragged end).  Exposed so that tests can hold the bounds against adversarial size patterns (tests/test_oracle.py).      */
void gs_msb_capacities(uint64_t num_items, int has_values, uint32_t *max_buckets, uint32_t *max_tasks, uint32_t *max_tiles);

/* Test access to the classification (cuda_radix_sort.h:1084-1087,1241-1247,
 * cuda_radix_sort_config.h:9).  Runs the sort of gs_msb_sort_u32 up to and including the classification of
 * `stop_level` (0..2; that level's scatter and everything after it do not run, so the arrays hold an intermediate
 * state) and leaves its lists in the workspace; `flags` bit 0 switches the heavy-hitter path off.
 * gs_msb_read_lists then copies them out: the buckets the classification passed to level stop_level + 1 as
 * {offset, size} pairs and the local-sort tasks of every class as {offset, size, sort_bits} triples (in device order,
 * which is not deterministic: compare as sets).  Counts are returned through n_buckets / n_tasks[4]; at most
 * max_buckets / max_tasks entries are copied per list.                                                              */
int gs_msb_classify_upto(void *d_temp, size_t temp_bytes, uint32_t *d_keys, uint32_t *d_keys_alt, uint64_t num_items,
                         int stop_level, int flags, void *stream);
int gs_msb_read_lists(void *d_temp, uint64_t num_items, int has_values, int level,
                      uint32_t *h_buckets, uint32_t max_buckets, uint32_t *n_buckets,
                      uint32_t *h_tasks[4], uint32_t max_tasks, uint32_t n_tasks[4], void *stream);

/* ------------------------------------------------ multi-GPU shard helpers --
 * One process per GPU; the exchange itself (one all-to-all over RCCL/xGMI)
 * is issued by the host between these calls (no reference
 * counterpart -- the reference is single-GPU).                               */

/* cub::DeviceSegmentedRadixSort (lsb/cub/cub/device/device_segmented_radix_sort.cuh:77-861;
 * DeviceSegmentedRadixSortKernel, dispatch_radix_sort.cuh:321-432): every segment
 * [d_begin_offsets[i], d_end_offsets[i]) of the keys (and values) is sorted on its own, stably,
 * on bits [begin_bit, end_bit); segments must not overlap, empty ones are fine, and positions
 * outside every segment are not written (offsets outside [0, num_items] are clamped on the device).  DoubleBuffer semantics as gs_lsb_sort_u32 (both
 * halves may be clobbered, the result is d_keys[*selector] after the call).  num_items < 2^31.
 * Segments that fit one workgroup (<= 17408 keys or pairs) cost one read and one write; the
 * larger ones are partitioned together, one 8-bit digit per pass.                       */
size_t gs_segmented_temp_bytes(uint64_t num_items, int has_values, uint32_t num_segments);
int gs_segmented_sort_u32(void *d_temp, size_t temp_bytes, uint32_t *d_keys[2], uint32_t *d_vals[2],
                          int *selector, uint64_t num_items, uint32_t num_segments,
                          const int32_t *d_begin_offsets, const int32_t *d_end_offsets, int begin_bit,
                          int end_bit, int descending, int key_type, void *stream);

/* The same for the wider element types (64-bit keys: GS_KEY_U64 / I64 / F64, with no, 32-bit or 64-bit values; 32-bit keys
 * with 64-bit values) -- cub's segmented dispatch is type-generic (dispatch_radix_sort.cuh:321-432).  Stable; bits
 * [begin_bit, end_bit) of the key; segments of <= 8192 elements cost one read and one write.  num_items < 2^31.        */
size_t gs_segmented_wide_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes, uint32_t num_segments);
int gs_segmented_sort_wide(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2], int *selector,
                           uint64_t num_items, uint32_t num_segments, const int32_t *d_begin_offsets,
                           const int32_t *d_end_offsets, int key_bytes, int val_bytes, int begin_bit, int end_bit,
                           int descending, int key_type, void *stream);

/* The same for 8- and 16-bit keys on kernels of their own (gs_seg_narrow.inc): key_type GS_KEY_U8 / GS_KEY_I8 / GS_KEY_U16 /
 * GS_KEY_I16, or the float categories GS_KEY_F16 / GS_KEY_BF16 / GS_KEY_F8 in the order stated at the enum (a short tile is
 * padded with the preimage of the all-ones image, 0x7fff / 0x7f ascending and 0xffff / 0xff descending), with val_bytes 0
 * (d_vals == NULL), 4 or 8.  Every other key type or value size is refused with
 * hipErrorInvalidValue, and both queries below return 0 for it (the convention of gs_lsb_narrow_temp_bytes).
 * Stable, ascending or descending, on bits [begin_bit, end_bit) of the key's order-preserving image at its own width
 * (end_bit <= 8 or <= 16).  DoubleBuffer semantics as gs_segmented_sort_u32: both halves may be overwritten inside segments,
 * and *selector flips once per 8-bit pass, ceil((end_bit - begin_bit) / 8) times -- once for 8-bit keys; for 16-bit keys over
 * all bits it ends where it started.  Positions outside every segment are not written, in either half of either array: every
 * store is one element wide, so no byte next to a segment is touched.  Segments must not overlap; empty segments and
 * end < begin are ignored; offsets outside [0, num_items] are clamped on the device.  The alignment paragraph above holds: a u8
 * array may start at any byte address, a u16 array at any even one, values at a multiple of their size, d_temp anywhere.
 * num_items == 0, num_segments == 0 or begin_bit == end_bit returns 0, writes nothing, needs no workspace and leaves
 * *selector alone.  num_items < 2^31 (int offsets).  The call only enqueues work on `stream` (no host synchronisation,
 * allocation or read-back); calls may follow each other on one stream with one workspace.  Refused with
 * hipErrorInvalidValue before anything is enqueued or written: a NULL or too-small workspace, a selector other than 0 or 1,
 * a missing buffer half, values without val_bytes or val_bytes without values, a bad bit range, num_items >= 2^31, NULL
 * offsets, a misaligned array.
 * Segments of up to gs_segmented_narrow_cap elements (8192) cost one read and one write; the larger ones are partitioned
 * together, one 8-bit digit per pass, in tiles of gs_lsb_narrow_tile(key_type, val_bytes) elements.
 * Workspace (a pure host function of its arguments, a multiple of 256): the list workspace of gs_segmented_sort_wide's
 * geometry -- with B = num_items / 8192 + 257 buckets, T = 8 * ((num_items / 4096 + B + num_items / 2^20 + 2) / 8 + 2) tile
 * records and K = 2 * num_items / 3000 + 3 * B + 512 + num_segments task records per class, every term rounded up to 256
 * bytes: 10 level records of 64 bytes, 2 * 16 B bucket records, 16 T tile records, 1024 B cursors, 128 T spine, 512 T
 * in-chunk prefixes, 4 * 16 K task records, 32 B heavy-hitter records (unused here), 10 * 4096 * 32 census bytes -- plus
 * 256 bytes of alignment slack.  No element is ever copied into the workspace.                                          */
size_t gs_segmented_narrow_temp_bytes(uint64_t num_items, int key_type, int val_bytes, uint32_t num_segments);
int gs_segmented_sort_narrow(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2], int *selector,
                             uint64_t num_items, uint32_t num_segments, const int32_t *d_begin_offsets,
                             const int32_t *d_end_offsets, int key_type, int val_bytes, int begin_bit, int end_bit,
                             int descending, void *stream);
/* the largest segment, in elements, that one workgroup sorts for this key type and value size (0: not served); tests sweep
 * sizes around it */
uint32_t gs_segmented_narrow_cap(int key_type, int val_bytes);

/* The MSB path cut at the exchange point (north_star: "a single RCCL all-to-all after the
 * first digit pass"): gs_msb_first_pass_u32 is the top-byte partition on its own -- keys (and
 * values) leave grouped by top byte in d_*_out, in their order-preserving u32 form, and
 * d_bucket_counts[256] (u64) gets the bucket sizes; d_temp sized by gs_lsb_temp_bytes.  The
 * host assigns contiguous bucket ranges to ranks, so every rank's share is one contiguous
 * slice of d_keys_out and goes out in ONE all-to-all.  gs_msb_finish_u32 completes the sort on
 * the receiving rank: d_keys holds, source after source, each source's slice (its buckets in
 * byte order); h_piece_counts[num_src][256] (HOST memory) are the piece sizes.  The buckets are
 * picked up where they lie -- no regrouping pass -- and the sorted keys (in key_type's own
 * representation) land in d_keys_out; d_keys / d_vals are clobbered.  d_temp sized by
 * gs_msb_finish_temp_bytes.  h_piece_counts is read before the call returns; the call itself
 * is asynchronous on `stream` unless `synchronize` is set, so a host that cuts the exchange
 * into several collectives can enqueue one finish per group of buckets behind its collective
 * (pointers offset to the group's slice of the receive and output buffers, one d_temp per
 * finish that may be in flight -- calls on one stream may share it).              */
int gs_msb_first_pass_u32(void *d_temp, size_t temp_bytes, const uint32_t *d_keys_in,
                          uint32_t *d_keys_out, const uint32_t *d_vals_in, uint32_t *d_vals_out,
                          uint64_t num_items, int key_type, uint64_t *d_bucket_counts, void *stream);
size_t gs_msb_finish_temp_bytes(uint64_t num_items, int has_values, int num_src);
int gs_msb_finish_u32(void *d_temp, size_t temp_bytes, uint32_t *d_keys, uint32_t *d_vals,
                      uint32_t *d_keys_out, uint32_t *d_vals_out, uint64_t num_items,
                      const uint64_t *h_piece_counts, int num_src, int key_type, void *stream,
                      int synchronize);

/* 2^bits-bin histogram (u64 counts) of the top `bits` bits of each key. */
int gs_shard_histogram_u32(const uint32_t *d_keys, uint64_t num_items, int bits,
                           uint64_t *d_hist, int key_type, void *stream);
/* Partition by destination rank:
 * d_dest_of_bin[top `bits` bits] gives the rank (monotone non-decreasing,
 * < num_ranks <= 256).  Writes keys (and values) grouped by rank into d_*_out
 * and the per-rank counts into d_counts[num_ranks] (u64).  The order inside a
 * rank's group is the input order (deterministic).  d_bin_hist: accepted for
 * compatibility and ignored (the partition counts per tile itself), may be
 * NULL.  d_temp sized by gs_msb_temp_bytes.                                   */
int gs_shard_partition_u32(void *d_temp, size_t temp_bytes,
                           const uint32_t *d_keys_in, uint32_t *d_keys_out,
                           const uint32_t *d_vals_in, uint32_t *d_vals_out,
                           uint64_t num_items, int bits, const uint8_t *d_dest_of_bin,
                           int num_ranks, const uint64_t *d_bin_hist, uint64_t *d_counts,
                           int key_type, void *stream);

/* -------------------------------------------------- on-device test inputs --
 * Counter-based generators identical to oracle/oracle.c; they
 * replace the cuRAND fills of lsb/sort.cu:125-131, msb/src/test.cu:38-43 and
 * msb/tests/data_gen.h:33-84.                                                */
enum gs_gen_kind { GS_GEN_UNIFORM = 0, GS_GEN_ZIPF = 1, GS_GEN_ENTROPY_AND = 2, GS_GEN_ENUMERATED = 3 };
int gs_generate_u32(uint32_t *d_out, uint64_t num_items, int kind, uint64_t seed,
                    uint64_t start_index, int level, void *stream);

/* Size-independent result checks run on the device (used at full BASELINE
 * sizes where a host oracle would take minutes): d_result[0] = number of
 * adjacent inversions, [1] = sum of splitmix64(key), [2] = xor of the same. */
int gs_check_sorted_u32(const uint32_t *d_keys, uint64_t num_items, int descending,
                        uint64_t *d_result, void *stream);
/* d_result[0] = number of i with d_keys_in[d_vals[i]] != d_keys_sorted[i] or
 * d_vals[i] >= num_items, [1] = sum of d_vals (msb/tests/test_sort_pairs.cu
 * :141-146,166-176 on the device).                                           */
int gs_check_pairs_enumerated_u32(const uint32_t *d_keys_in, const uint32_t *d_keys_sorted,
                                  const uint32_t *d_vals, uint64_t num_items,
                                  uint64_t *d_result, void *stream);
/* 64-bit keys (key_type GS_KEY_U64 / I64 / F64): d_result[0] = adjacent inversions in the order the sort produces (the key
 * type's order-preserving map: -0.0 before +0.0, NaNs by their bits), [1] / [2] = sum / xor of splitmix64(key).       */
int gs_check_sorted_u64(const uint64_t *d_keys, uint64_t num_items, int key_type, uint64_t *d_result, void *stream);
/* 64-bit values, 32- or 64-bit keys (key_bytes): d_result[0] = number of i with d_vals[i] >= num_items or
 * d_keys_in[d_vals[i]] != d_keys_sorted[i] (bitwise), [1] = sum of d_vals mod 2^64.                                   */
int gs_check_pairs_enumerated_wide(const void *d_keys_in, const void *d_keys_sorted, const uint64_t *d_vals,
                                   uint64_t num_items, int key_bytes, uint64_t *d_result, void *stream);
/* The result of a stable sort (gs_lsb_sort_large): d_result[0] = number of adjacent positions out of the sort's order on
 * bits [begin_bit, end_bit) of the key type's order-preserving map (reversed when descending), plus, when d_rowids is not
 * NULL, the number of adjacent equal sort keys whose row ids do not strictly increase.  32- or 64-bit keys (key_bytes with
 * a matching key_type); u64 indices.  With gs_check_pairs_enumerated_wide on the same output (every row id points at a
 * bitwise-equal input key) it proves the output is THE stable sort of the input.                                      */
int gs_check_sorted_stable(const void *d_keys_sorted, const uint64_t *d_rowids, uint64_t num_items, int key_bytes,
                           int key_type, int begin_bit, int end_bit, int descending, uint64_t *d_result, void *stream);

/* ------------------------------------------------------ kernel timing hook --
 * Optional per-kernel device timing with hipEvents recorded on the SAME stream
 * the kernels are launched on (replaces the reference's cudaEvent pairs,
 * lsb/gpu_utils.h:3-11, and its gated per-pass BM_* events,
 * msb/src/sort/gpu_radix_sort.h:266-269).  While a profile is bound to the
 * calling thread (gs_profile_begin .. gs_profile_end) every kernel the library
 * launches from that thread is bracketed by an event pair.  gs_profile_read
 * waits for the recorded events and accumulates milliseconds and launch counts
 * per kernel id; it may be called once the work has been enqueued.            */
enum gs_kernel_id {
    GS_K_LSB_UPSWEEP = 0, GS_K_LSB_SCAN = 1, GS_K_LSB_DOWNSWEEP = 2,
    GS_K_MSB_HISTOGRAM = 3, GS_K_MSB_CLASSIFY = 4, GS_K_MSB_PARTITION = 5, GS_K_MSB_LOCAL_SORT = 6,
    GS_K_SHARD = 7, GS_K_OTHER = 8,
    GS_K_LSB_PASS = 9,   /* a whole pass in one launch (upsweep / scan / downsweep as roles of one kernel) */
    GS_K_COUNT = 10
};
typedef struct gs_profile gs_profile;
gs_profile *gs_profile_create(void);
void        gs_profile_destroy(gs_profile *p);
void        gs_profile_begin(gs_profile *p);   /* bind to this thread */
void        gs_profile_end(void);              /* unbind              */
int         gs_profile_read(gs_profile *p, double total_ms[GS_K_COUNT], uint64_t launches[GS_K_COUNT]);
const char *gs_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* GPUSORT_H_ */
