// gs_large.hip -- the MSB sort of 2^32 keys and more on one GPU (gs_msb_sort_large_u32): the single-GPU form of the
// multi-GPU design, first digit pass then independent finishes.
//
//   1. the 64-bit pass: one stable partition on the top byte, keys -> alt, with 64-bit output offsets.  The input is
//      cut into slices of <= 2^31 keys; every slice gets the LSB pass's own upsweep and spine scan (32-bit counts
//      inside the slice), large_offsets_kernel turns the (slice, digit) totals into absolute u64 starts, and the
//      downsweep of every slice (lsb_downsweep64: the LSB tile code with a u64 base per digit) writes through them.
//      12 B/key (16 + 4 with values), like the 32-bit pass;
//   2. the host reads the 256 bucket sizes and packs consecutive buckets into groups of <= LARGE_GROUP keys; each
//      group is finished by gs_msb_finish_u32 (one source, pointer-offset slices: alt -> keys), one workspace reused
//      by all of them on the stream;
//   3. a bucket larger than a group is partitioned again by the 64-bit pass on its next byte and planned the same
//      way (skewed inputs only).  After the last byte a range is sorted; only the twiddle is undone.
// gs_msb_sort_large_wide is the same planner for the wide element types: the pass is the wide
// LSB pass per slice (wide_slice_count / wide_slice_scatter: wide_downsweep64_kernel), keys keep their representation,
// and groups are finished by msb_wide_finish (the wide MSB levels, started from the group's counts).
// gs_lsb_sort_large is the stable LSB sort over the same pass: one 64-bit pass per digit of
// [begin_bit, end_bit), ping-ponging between the DoubleBuffer halves, keys twiddled on the first pass and restored on the
// last (lsb_run_passes' rule).  Its offsets are computed on the device, so the sort only enqueues work and can be captured.
// gs_lsb_sort_narrow_large is gs_lsb_sort_narrow's plain-pointer contract over the same pass for 8- and 16-bit
// keys: per slice the narrow upsweep and downsweep (narrow_slice_count / narrow_slice_scatter: narrow_downsweep64_kernel), one or
// two passes, in -> (workspace ->) out; 8-bit keys alone take a histogram with 64-bit counts and a fill (narrow_fill_large).
#include "gs_device.hpp"
#include "gs_lsb.hpp"
#include <cstdlib>

namespace gs {

constexpr uint64_t LARGE_GROUP = 1ull << 31;   // keys per finish and per slice of the 64-bit pass
constexpr uint64_t LARGE_MAX = 1ull << 40;     // num_items limit of the entry point
constexpr uint32_t LARGE_MIN_TEST_LIMIT = 256;

// Test hook (tests/test_msb_large_gpu.py, tests/test_lsb_large_gpu.py, tests/test_narrow_large_gpu.py): GS_MSB_LARGE_TEST_LIMIT=k
// lowers the group size and the slice size to k keys, so that small arrays take multi-slice passes, multi-group finishes and splits
// (and, in gs_lsb_sort_large and gs_lsb_sort_narrow_large, arrays of more than k elements the 64-bit passes).  Read on every call;
// never set in production.
static uint64_t large_limit()
{
    if (const char *e = getenv("GS_MSB_LARGE_TEST_LIMIT")) {
        const uint64_t k = strtoull(e, nullptr, 10);
        if (k >= LARGE_MIN_TEST_LIMIT && k < LARGE_GROUP) return k;
    }
    return LARGE_GROUP;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace of the 64-bit pass over m elements in slices of S: per slice its spine and prefix16 (the layout of gs_lsb.hip's
// pass, or of gs_wide.hip's for the wide element types), then the slices' digit totals [slices][256] u32, the digit starts
// [slices][256] u64 and the bucket sizes [256] u64
struct LargePassWs {
    char *slice_ws;          // slice i: spine at slice_ws + i * per_slice, prefix16 behind it
    size_t per_slice, spine_bytes;
    uint32_t *totals;
    uint64_t *dbase;
    uint64_t *counts;
};
static inline uint64_t large_slices(uint64_t m, uint64_t S) { return m ? (m + S - 1) / S : 1; }
static inline void large_slice_bytes(uint64_t S, bool wide, size_t &spine, size_t &prefix)
{
    if (wide) { wide_slice_bytes(S, spine, prefix); return; }
    const PassParams p = lsb_make_params(S, 24, 8);
    spine = align256((size_t)RADIX * p.grid * sizeof(uint32_t));
    prefix = align256((size_t)p.num_tiles * RADIX * sizeof(uint16_t));
}
// (every slice is carved at the size of a full one: the last one is never larger)
static size_t large_pass_bytes(uint64_t m, uint64_t S, bool wide)
{
    size_t sp, pf;
    large_slice_bytes(S, wide, sp, pf);
    const uint64_t ns = large_slices(m, S);
    return (size_t)ns * (sp + pf) + align256((size_t)ns * RADIX * sizeof(uint32_t)) + align256((size_t)ns * RADIX * sizeof(uint64_t)) +
           align256(RADIX * sizeof(uint64_t));
}
static LargePassWs large_pass_carve(void *temp, uint64_t m, uint64_t S, bool wide)
{
    LargePassWs w;
    size_t pf;
    large_slice_bytes(S, wide, w.spine_bytes, pf);
    w.per_slice = w.spine_bytes + pf;
    const uint64_t ns = large_slices(m, S);
    char *c = (char *)temp;
    w.slice_ws = c; c += (size_t)ns * w.per_slice;
    w.totals = (uint32_t *)c; c += align256((size_t)ns * RADIX * sizeof(uint32_t));
    w.dbase = (uint64_t *)c; c += align256((size_t)ns * RADIX * sizeof(uint64_t));
    w.counts = (uint64_t *)c;
    return w;
}

// one block, thread d: the runs of digit d, slice after slice, behind the runs of all smaller digits
__global__ __launch_bounds__(RADIX) void large_offsets_kernel(const uint32_t *__restrict__ totals, uint32_t slices,
                                                              unsigned long long *__restrict__ dbase, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long sc[RADIX];
    const uint32_t d = threadIdx.x;
    unsigned long long run = 0;
    for (uint32_t s = 0; s < slices; ++s) {
        dbase[(size_t)s * RADIX + d] = run;
        run += totals[(size_t)s * RADIX + d];
    }
    counts[d] = run;
    sc[d] = run;
    __syncthreads();
    for (uint32_t off = 1; off < RADIX; off <<= 1) {
        const unsigned long long v = d >= off ? sc[d - off] : 0ull;
        __syncthreads();
        sc[d] += v;
        __syncthreads();
    }
    const unsigned long long start = sc[d] - run;
    for (uint32_t s = 0; s < slices; ++s) dbase[(size_t)s * RADIX + d] += start;
}

// undo the key twiddle of a sorted range (grid-stride; src == dst allowed)
__global__ __launch_bounds__(256) void large_untwiddle_kernel(const uint32_t *src, uint32_t *dst, unsigned long long n, int f32,
                                                              uint32_t x)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = twiddle_out(src[i], f32, x);
}

struct LargeCtx {
    char *k[2], *v[2];       // [0] = the caller's arrays (where the result goes), [1] = the alternates
    int kb, vb;              // element sizes: key bytes (4 | 8), value bytes (0: keys only)
    bool wide;               // the wide kernel set (gs_msb_sort_large_wide); otherwise u32 keys with no or u32 values
    int key_type;
    uint64_t L;              // group size and slice size
    char *pass_ws;
    char *fin_ws;
    size_t fin_bytes;
    hipStream_t s;
    int synchronize;
};

// The 64-bit pass: stable partition of m elements on the digit d (d.bits wide at d.shift), kin -> kout, with d's twiddle
// (LargeDigit), through the workspace w carved for m.  When h_counts is given, the 256 bucket sizes are copied to it and the
// call waits for them; otherwise the pass only enqueues work.
static int large_pass(const LargeCtx &c, const LargePassWs &w, const char *kin, char *kout, const char *vin, char *vout, uint64_t m,
                      const LargeDigit &d, uint64_t *h_counts)
{
    const uint64_t S = c.L;
    const hipStream_t s = c.s;
    const uint64_t ns = large_slices(m, S);
    int e;
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = m - off < S ? m - off : S;
        uint32_t *spine = (uint32_t *)(w.slice_ws + i * w.per_slice);
        uint16_t *prefix16 = (uint16_t *)(w.slice_ws + i * w.per_slice + w.spine_bytes);
        if (c.wide) {
            if ((e = wide_slice_count(kin + off * c.kb, len, c.kb, d, spine, prefix16, w.totals + i * RADIX, s))) return e;
            continue;
        }
        PassParams p = lsb_make_params(len, d.shift, d.bits);
        lsb_twiddle_masks(d.key_type, d.descending, d.first, d.last, p);
        if ((e = lsb_upsweep((const uint32_t *)kin + off, spine, prefix16, p, s))) return e;
        if ((e = lsb_scan(spine, w.totals + i * RADIX, p.grid, s))) return e;
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(large_offsets_kernel, dim3(1), dim3(RADIX), 0, s, (const uint32_t *)w.totals, (uint32_t)ns,
                           (unsigned long long *)w.dbase, (unsigned long long *)w.counts);
    }
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = m - off < S ? m - off : S;
        const uint32_t *spine = (const uint32_t *)(w.slice_ws + i * w.per_slice);
        const uint16_t *prefix16 = (const uint16_t *)(w.slice_ws + i * w.per_slice + w.spine_bytes);
        if (c.wide) {
            if ((e = wide_slice_scatter(kin + off * c.kb, kout, vin ? vin + off * c.vb : nullptr, vout, len, c.kb, c.vb, d, spine,
                                        prefix16, w.dbase + i * RADIX, s)))
                return e;
            continue;
        }
        PassParams p = lsb_make_params(len, d.shift, d.bits);
        lsb_twiddle_masks(d.key_type, d.descending, d.first, d.last, p);
        if ((e = lsb_downsweep64((const uint32_t *)kin + off, (uint32_t *)kout, vin ? (const uint32_t *)vin + off : nullptr,
                                 (uint32_t *)vout, spine, prefix16, w.totals + i * RADIX, w.dbase + i * RADIX, p, s)))
            return e;
    }
    if (!h_counts) return hipSuccess;
    hipError_t he = hipMemcpyAsync(h_counts, w.counts, RADIX * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    return (int)he;
}

static int large_copy_back(const LargeCtx &c, uint64_t off, uint64_t m)
{
    hipError_t e = hipMemcpyAsync(c.k[0] + off * c.kb, c.k[1] + off * c.kb, m * c.kb, hipMemcpyDeviceToDevice, c.s);
    if (e == hipSuccess && c.vb) e = hipMemcpyAsync(c.v[0] + off * c.vb, c.v[1] + off * c.vb, m * c.vb, hipMemcpyDeviceToDevice, c.s);
    return (int)e;
}

// finish the group [off, off + m) that lies in buffer `b`, its buckets (by the byte at `shift`, just partitioned) sized gcounts
static int large_finish_group(const LargeCtx &c, int b, uint64_t off, uint64_t m, const uint64_t *gcounts, int shift)
{
    const int o = b ^ 1;
    char *kb_ = c.k[b] + off * c.kb, *ko = c.k[o] + off * c.kb;
    char *vb_ = c.vb ? c.v[b] + off * c.vb : nullptr, *vo = c.vb ? c.v[o] + off * c.vb : nullptr;
    int e, res = o;   // the buffer the result lands in
    if (c.wide) {
        // the levels below `shift` only: the result lands in either buffer, by the parity of the bytes left (msb_wide_levels)
        int in_src = 0;
        e = msb_wide_finish(c.fin_ws, kb_, vb_, ko, vo, m, c.kb, c.vb, gcounts, shift, c.key_type, c.s, c.synchronize, &in_src);
        if (in_src) res = b;
    } else {
        e = gs_msb_finish_u32(c.fin_ws, c.fin_bytes, (uint32_t *)kb_, (uint32_t *)vb_, (uint32_t *)ko, (uint32_t *)vo, m, gcounts, 1,
                              c.key_type, c.s, c.synchronize);
    }
    if (e) return e;
    return res == 0 ? 0 : large_copy_back(c, off, m);   // (a split range of odd depth: the result landed in the alternates)
}

// The range [off, off + m) lies in buffer `cur`; its keys agree on every byte above `shift` (in the twiddled order).  Partition
// it on the byte at `shift` into the other buffer, then finish its buckets in groups, splitting the ones larger than a group.
static int large_range(const LargeCtx &c, uint64_t off, uint64_t m, int cur, int shift, int key_type_in)
{
    uint64_t counts[RADIX];
    const int nb = cur ^ 1;
    // the u32 path keeps its keys twiddled until the range is sorted (GS_KEY_U32 below the first pass: none); the wide path
    // writes them back in their own representation
    const LargeDigit d{shift, RADIX_BITS, key_type_in, 0, true, c.wide};
    int e = large_pass(c, large_pass_carve(c.pass_ws, m, c.L, c.wide), c.k[cur] + off * c.kb, c.k[nb] + off * c.kb,
                       c.vb ? c.v[cur] + off * c.vb : nullptr, c.vb ? c.v[nb] + off * c.vb : nullptr, m, d, counts);
    if (e) return e;
    if (shift == 0) {
        // every byte is ordered: the range is sorted, each bucket one value.  Wide keys are in their own representation;
        // u32 keys have their twiddle undone on the way to the caller's arrays.
        if (c.wide) return nb == 0 ? 0 : large_copy_back(c, off, m);
        PassParams tw{};
        lsb_twiddle_masks(c.key_type, 0, false, true, tw);
        if (nb == 0 && !tw.f32_out && !tw.xor_out) return 0;
        KernelTimer kt(GS_K_OTHER, c.s);
        const uint64_t blocks = (m + 255) / 256;
        hipLaunchKernelGGL(large_untwiddle_kernel, dim3(blocks < 8192 ? (uint32_t)blocks : 8192u), dim3(256), 0, c.s,
                           (const uint32_t *)c.k[nb] + off, (uint32_t *)c.k[0] + off, (unsigned long long)m, tw.f32_out, tw.xor_out);
        if ((e = (int)hipGetLastError())) return e;
        if (nb == 1 && c.vb)
            e = (int)hipMemcpyAsync(c.v[0] + off * c.vb, c.v[1] + off * c.vb, m * c.vb, hipMemcpyDeviceToDevice, c.s);
        return e;
    }
    uint64_t gcounts[RADIX] = {};
    uint64_t at = off, gstart = off, gsize = 0;
    for (int b = 0; b < RADIX; ++b) {
        const uint64_t n_b = counts[b];
        if (n_b == 0) continue;
        if (gsize && (n_b > c.L || gsize + n_b > c.L)) {
            if ((e = large_finish_group(c, nb, gstart, gsize, gcounts, shift))) return e;
            for (int q = 0; q < RADIX; ++q) gcounts[q] = 0;
            gsize = 0;
        }
        if (n_b > c.L) {
            if ((e = large_range(c, at, n_b, nb, shift - 8, c.wide ? c.key_type : GS_KEY_U32))) return e;
        } else {
            if (gsize == 0) gstart = at;
            gcounts[b] = n_b;
            gsize += n_b;
        }
        at += n_b;
    }
    if (gsize) e = large_finish_group(c, nb, gstart, gsize, gcounts, shift);
    return e;
}

// `ws`: the caller's workspace rounded up (gs_ws_base); the pass's workspace, then the finishes' one (sized by the public
// query of gs_msb_finish_temp_bytes / gs_msb_wide_temp_bytes, so it starts 256-byte aligned too)
static int large_run(LargeCtx &c, char *ws, uint64_t num_items, size_t pass_bytes)
{
    c.pass_ws = ws;
    c.fin_ws = ws + align256(pass_bytes);
    int e = large_range(c, 0, num_items, 0, 8 * c.kb - 8, c.key_type);
    if (e) return e;
    if ((e = (int)hipGetLastError())) return e;
    return c.synchronize ? (int)hipStreamSynchronize(c.s) : 0;
}

static bool overlaps(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    if (!a || !b) return false;
    const char *x = (const char *)a, *y = (const char *)b;
    return x < y + bbytes && y < x + abytes;
}

// no two of the arrays share a byte (sizes: the elements they hold)
static bool any_overlap(const void *const arr[4], const size_t bytes[4])
{
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (overlaps(arr[i], bytes[i], arr[j], bytes[j])) return true;
    return false;
}

// the call reads bucket sizes back to the host: refused inside a capture (nothing is enqueued); 0 = not capturing
static int large_capture_check(hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) return (int)hipGetLastError();
    return cs != hipStreamCaptureStatusNone ? (int)hipErrorStreamCaptureUnsupported : 0;
}

// the element types of gs_msb_sort_wide: 64-bit keys with no, 32-bit or 64-bit values, 32-bit keys with 64-bit values
static bool wide_types_ok(int key_bytes, int val_bytes, int key_type)
{
    if (key_bytes == 8) return (val_bytes == 0 || val_bytes == 4 || val_bytes == 8) && key_type >= GS_KEY_U64 && key_type <= GS_KEY_F64;
    return key_bytes == 4 && val_bytes == 8 && key_type >= GS_KEY_U32 && key_type <= GS_KEY_F32;
}

// ---- gs_lsb_sort_large: the stable LSB sort above 2^32 elements, the 64-bit pass once per digit.
// The element types of gs_lsb_sort_wide: 32- or 64-bit keys with no, 32-bit or 64-bit values.
static bool lsb_large_types_ok(int key_bytes, int val_bytes, int key_type)
{
    if (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) return false;
    if (key_bytes == 8) return key_type >= GS_KEY_U64 && key_type <= GS_KEY_F64;
    return key_bytes == 4 && key_type >= GS_KEY_U32 && key_type <= GS_KEY_F32;
}
// (u32, none | u32) take gs_lsb.hip's kernels (and gs_lsb_sort_u32 for one slice), the others the wide set (gs_lsb_sort_wide)
static inline bool lsb_large_wide(int key_bytes, int val_bytes) { return key_bytes == 8 || val_bytes == 8; }

// one 64-bit pass per digit of [begin_bit, end_bit), d_keys[sel] -> d_keys[sel ^ 1] (c.k / c.v hold the DoubleBuffer halves),
// all through the one workspace w; the bucket sizes stay on the device, so the host never waits
static int lsb_large_passes(const LargeCtx &c, const LargePassWs &w, int *selector, uint64_t n, int begin_bit, int end_bit, int descending)
{
    const int num_passes = (end_bit - begin_bit + RADIX_BITS - 1) / RADIX_BITS;
    int sel = *selector;
    for (int pass = 0; pass < num_passes; ++pass) {
        const int shift = begin_bit + pass * RADIX_BITS;
        const LargeDigit d{shift, end_bit - shift < RADIX_BITS ? end_bit - shift : RADIX_BITS, c.key_type, descending, pass == 0,
                           pass == num_passes - 1};
        if (int e = large_pass(c, w, c.k[sel], c.k[sel ^ 1], c.vb ? c.v[sel] : nullptr, c.vb ? c.v[sel ^ 1] : nullptr, n, d, nullptr))
            return e;
        sel ^= 1;
    }
    if (int e = (int)hipGetLastError()) return e;
    *selector = sel;
    return hipSuccess;
}

// ---- gs_lsb_sort_narrow_large: 8- and 16-bit keys above 2^32 elements, gs_lsb_sort_narrow's
// plain-pointer contract over the 64-bit pass.  The workspace: per slice a spine sized for a full slice, the slices' digit
// totals [slices][256] u32, the digit starts [slices][256] u64, the counts [256] u64 (the histogram of the fill path), then
// for 16-bit keys the intermediate keys and values of the pass in -> workspace -> out.
struct NarrowLargeWs {
    char *spines;
    size_t spine_bytes;      // of one slice
    uint32_t *totals;
    uint64_t *dbase;
    uint64_t *counts;
    char *tk, *tv;           // 16-bit keys only
};
static size_t narrow_large_pass_bytes(uint64_t n, uint64_t S, int kb, int vb)
{
    const uint64_t ns = large_slices(n, S);
    size_t b = (size_t)ns * narrow_slice_spine_bytes(S, vb) + align256((size_t)ns * RADIX * sizeof(uint32_t)) +
               align256((size_t)ns * RADIX * sizeof(uint64_t)) + align256(RADIX * sizeof(uint64_t));
    if (kb == 2) b += align256((size_t)n * 2) + align256((size_t)n * (size_t)vb);
    return b;
}
static NarrowLargeWs narrow_large_carve(char *c, uint64_t n, uint64_t S, int vb)
{
    NarrowLargeWs w;
    const uint64_t ns = large_slices(n, S);
    w.spine_bytes = narrow_slice_spine_bytes(S, vb);
    w.spines = c; c += (size_t)ns * w.spine_bytes;
    w.totals = (uint32_t *)c; c += align256((size_t)ns * RADIX * sizeof(uint32_t));
    w.dbase = (uint64_t *)c; c += align256((size_t)ns * RADIX * sizeof(uint64_t));
    w.counts = (uint64_t *)c; c += align256(RADIX * sizeof(uint64_t));
    w.tk = c;
    w.tv = c + align256((size_t)n * 2);
    return w;
}

// one stable 8-bit pass over n elements in slices of S: kin -> kout through 64-bit digit starts (large_pass for the narrow types)
static int narrow_large_pass(const NarrowLargeWs &w, const char *kin, char *kout, const char *vin, char *vout, uint64_t n, uint64_t S,
                             int kb, int vb, const LargeDigit &d, hipStream_t s)
{
    const uint64_t ns = large_slices(n, S);
    int e;
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = n - off < S ? n - off : S;
        if ((e = narrow_slice_count(kin + off * kb, len, vb, d, (uint32_t *)(w.spines + i * w.spine_bytes), w.totals + i * RADIX, s)))
            return e;
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(large_offsets_kernel, dim3(1), dim3(RADIX), 0, s, (const uint32_t *)w.totals, (uint32_t)ns,
                           (unsigned long long *)w.dbase, (unsigned long long *)w.counts);
    }
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = n - off < S ? n - off : S;
        if ((e = narrow_slice_scatter(kin + off * kb, kout, vin ? vin + off * vb : nullptr, vout, len, vb, d,
                                      (const uint32_t *)(w.spines + i * w.spine_bytes), w.dbase + i * RADIX, s)))
            return e;
    }
    return hipSuccess;
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_msb_large_temp_bytes(uint64_t num_items, int has_values)
{
    const uint64_t L = large_limit();
    return align256(large_pass_bytes(num_items, L, false)) + gs_msb_finish_temp_bytes(L, has_values, 1) + GS_WS_SLACK;
}

int gs_msb_sort_large_u32(void *d_temp, size_t temp_bytes, uint32_t *d_keys, uint32_t *d_vals, uint64_t num_items,
                          uint32_t *d_keys_alt, uint32_t *d_vals_alt, int key_type, void *stream, int synchronize)
{
    // argument checks touch no device
    if (num_items >= LARGE_MAX) return hipErrorInvalidValue;
    if (key_type < GS_KEY_U32 || key_type > GS_KEY_F32) return hipErrorInvalidValue;
    if (num_items == 0) return hipSuccess;
    const bool pairs = d_vals != nullptr;
    if (!d_keys || !d_keys_alt || (pairs && !d_vals_alt)) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < gs_msb_large_temp_bytes(num_items, pairs)) return hipErrorInvalidValue;
    {
        const void *arr[4] = {d_keys, d_keys_alt, d_vals, pairs ? d_vals_alt : nullptr};
        const size_t b = num_items * sizeof(uint32_t), bytes[4] = {b, b, b, b};
        if (any_overlap(arr, bytes)) return hipErrorInvalidValue;
    }
    GS_CLEAR_STALE_ERROR();
    hipStream_t s = (hipStream_t)stream;
    if (int ce = large_capture_check(s)) return ce;

    const uint64_t L = large_limit();
    // one group: the plain MSB sort on the caller's workspace, which it rounds up the same way (its query fits in the finish's,
    // both sized for L keys)
    if (num_items <= L)
        return gs_msb_sort_u32(d_temp, temp_bytes, d_keys, d_vals, num_items, d_keys_alt, d_vals_alt, nullptr, nullptr, key_type,
                               stream, synchronize);

    LargeCtx c;
    c.k[0] = (char *)d_keys; c.k[1] = (char *)d_keys_alt;
    c.v[0] = (char *)d_vals; c.v[1] = pairs ? (char *)d_vals_alt : nullptr;
    c.kb = 4; c.vb = pairs ? 4 : 0;
    c.wide = false;
    c.key_type = key_type;
    c.L = L;
    c.fin_bytes = gs_msb_finish_temp_bytes(L, pairs, 1);
    c.s = s;
    c.synchronize = synchronize;
    return large_run(c, gs_ws_base(d_temp), num_items, large_pass_bytes(num_items, L, false));
}

size_t gs_msb_large_wide_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes)
{
    const uint64_t L = large_limit();
    return align256(large_pass_bytes(num_items, L, true)) + gs_msb_wide_temp_bytes(L, key_bytes, val_bytes) + GS_WS_SLACK;
}

int gs_msb_sort_large_wide(void *d_temp, size_t temp_bytes, void *d_keys, void *d_vals, uint64_t num_items, void *d_keys_alt,
                           void *d_vals_alt, int key_bytes, int val_bytes, int key_type, void *stream, int synchronize)
{
    // argument checks touch no device
    if (num_items >= LARGE_MAX) return hipErrorInvalidValue;
    if (!wide_types_ok(key_bytes, val_bytes, key_type)) return hipErrorInvalidValue;   // (u32, none | u32): gs_msb_sort_large_u32
    if (num_items == 0) return hipSuccess;
    const bool pairs = val_bytes != 0;
    if (pairs != (d_vals != nullptr)) return hipErrorInvalidValue;
    if (!d_keys || !d_keys_alt || (pairs && !d_vals_alt)) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < gs_msb_large_wide_temp_bytes(num_items, key_bytes, val_bytes)) return hipErrorInvalidValue;
    {
        const void *arr[4] = {d_keys, d_keys_alt, d_vals, pairs ? d_vals_alt : nullptr};
        const size_t kb = num_items * (size_t)key_bytes, vb = num_items * (size_t)val_bytes, bytes[4] = {kb, kb, vb, vb};
        if (any_overlap(arr, bytes)) return hipErrorInvalidValue;
    }
    GS_CLEAR_STALE_ERROR();
    hipStream_t s = (hipStream_t)stream;
    if (int ce = large_capture_check(s)) return ce;

    const uint64_t L = large_limit();
    if (num_items <= L) {   // one group: the plain wide MSB sort, whose list overflow is checked here
        int e = gs_msb_sort_wide(d_temp, temp_bytes, d_keys, d_vals, num_items, d_keys_alt, d_vals_alt, key_bytes, val_bytes, nullptr,
                                 nullptr, key_type, stream, 0);
        if (e) return e;
        return synchronize ? msb_wide_overflow(gs_ws_base(d_temp), num_items, key_bytes, val_bytes, s) : 0;
    }

    LargeCtx c;
    c.k[0] = (char *)d_keys; c.k[1] = (char *)d_keys_alt;
    c.v[0] = (char *)d_vals; c.v[1] = pairs ? (char *)d_vals_alt : nullptr;
    c.kb = key_bytes; c.vb = val_bytes;
    c.wide = true;
    c.key_type = key_type;
    c.L = L;
    c.fin_bytes = gs_msb_wide_temp_bytes(L, key_bytes, val_bytes);
    c.s = s;
    c.synchronize = synchronize;
    return large_run(c, gs_ws_base(d_temp), num_items, large_pass_bytes(num_items, L, true));
}

// the 64-bit pass's workspace, or the delegate's for arrays of one slice, whichever is larger (both grow with n)
size_t gs_lsb_large_temp_bytes(uint64_t num_items, int key_bytes, int val_bytes)
{
    const uint64_t L = large_limit();
    const bool wide = lsb_large_wide(key_bytes, val_bytes);
    const uint64_t m = num_items < L ? num_items : L;
    const size_t pass = align256(large_pass_bytes(num_items, L, wide)) + GS_WS_SLACK;
    const size_t one = wide ? gs_lsb_wide_temp_bytes(m, key_bytes, val_bytes) : gs_lsb_temp_bytes(m, val_bytes != 0);
    return pass > one ? pass : one;
}

int gs_lsb_sort_large(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2], int *selector, uint64_t num_items,
                      int key_bytes, int val_bytes, int begin_bit, int end_bit, int descending, int key_type, void *stream)
{
    // argument checks touch no device, and all of them come before anything is enqueued
    if (!selector || (*selector != 0 && *selector != 1) || !d_keys) return hipErrorInvalidValue;
    if (!lsb_large_types_ok(key_bytes, val_bytes, key_type)) return hipErrorInvalidValue;
    if ((val_bytes != 0) != (d_vals != nullptr)) return hipErrorInvalidValue;
    if (begin_bit < 0 || end_bit > 8 * key_bytes || begin_bit > end_bit) return hipErrorInvalidValue;
    if (num_items >= LARGE_MAX) return hipErrorInvalidValue;
    if (num_items == 0 || begin_bit == end_bit) return hipSuccess;
    if (!d_temp || temp_bytes < gs_lsb_large_temp_bytes(num_items, key_bytes, val_bytes)) return hipErrorInvalidValue;
    if (!d_keys[0] || !d_keys[1] || (d_vals && (!d_vals[0] || !d_vals[1]))) return hipErrorInvalidValue;
    const bool pairs = d_vals != nullptr;
    {
        const void *arr[4] = {d_keys[0], d_keys[1], pairs ? d_vals[0] : nullptr, pairs ? d_vals[1] : nullptr};
        const size_t kb = num_items * (size_t)key_bytes, vb = num_items * (size_t)val_bytes, bytes[4] = {kb, kb, vb, vb};
        if (any_overlap(arr, bytes)) return hipErrorInvalidValue;
    }
    GS_CLEAR_STALE_ERROR();
    const bool wide = lsb_large_wide(key_bytes, val_bytes);
    const uint64_t L = large_limit();
    if (num_items <= L) {   // one slice: the plain LSB sort on the same arguments (a stable sort's result is unique)
        if (wide)
            return gs_lsb_sort_wide(d_temp, temp_bytes, d_keys, d_vals, selector, num_items, key_bytes, val_bytes, begin_bit, end_bit,
                                    descending, key_type, stream);
        uint32_t *k2[2] = {(uint32_t *)d_keys[0], (uint32_t *)d_keys[1]};
        uint32_t *v2[2] = {pairs ? (uint32_t *)d_vals[0] : nullptr, pairs ? (uint32_t *)d_vals[1] : nullptr};
        return gs_lsb_sort_u32(d_temp, temp_bytes, k2, pairs ? v2 : nullptr, selector, num_items, begin_bit, end_bit, descending,
                               key_type, stream);
    }

    LargeCtx c{};
    c.k[0] = (char *)d_keys[0]; c.k[1] = (char *)d_keys[1];
    c.v[0] = pairs ? (char *)d_vals[0] : nullptr; c.v[1] = pairs ? (char *)d_vals[1] : nullptr;
    c.kb = key_bytes; c.vb = val_bytes;
    c.wide = wide;
    c.key_type = key_type;
    c.L = L;
    c.pass_ws = gs_ws_base(d_temp);
    c.s = (hipStream_t)stream;
    return lsb_large_passes(c, large_pass_carve(c.pass_ws, num_items, L, wide), selector, num_items, begin_bit, end_bit, descending);
}

// the 64-bit pass's workspace, or gs_lsb_sort_narrow's for arrays of one slice, whichever is larger (both grow with n)
size_t gs_lsb_narrow_large_temp_bytes(uint64_t num_items, int key_type, int val_bytes)
{
    const int kb = narrow_key_bytes(key_type);
    if (kb == 0 || gs_lsb_narrow_tile(key_type, val_bytes) == 0 || num_items >= LARGE_MAX) return 0;
    const uint64_t L = large_limit();
    const size_t pass = narrow_large_pass_bytes(num_items, L, kb, val_bytes) + GS_WS_SLACK;
    const size_t one = gs_lsb_narrow_temp_bytes(num_items < L ? num_items : L, key_type, val_bytes);
    return pass > one ? pass : one;
}

int gs_lsb_sort_narrow_large(void *d_temp, size_t temp_bytes, const void *d_keys_in, void *d_keys_out, const void *d_vals_in,
                             void *d_vals_out, uint64_t num_items, int key_type, int val_bytes, int begin_bit, int end_bit,
                             int descending, void *stream)
{
    // argument checks touch no device, and all of them come before anything is enqueued
    const int kb = narrow_key_bytes(key_type);
    if (kb == 0 || gs_lsb_narrow_tile(key_type, val_bytes) == 0) return hipErrorInvalidValue;
    if (begin_bit < 0 || end_bit > 8 * kb || begin_bit > end_bit) return hipErrorInvalidValue;
    if (num_items >= LARGE_MAX) return hipErrorInvalidValue;
    if (num_items == 0) return hipSuccess;              // (empty arrays may come with null pointers)
    if ((val_bytes != 0) != (d_vals_in != nullptr) || (val_bytes != 0) != (d_vals_out != nullptr)) return hipErrorInvalidValue;
    if (!d_keys_in || !d_keys_out) return hipErrorInvalidValue;
    if (((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & (uintptr_t)(kb - 1)) return hipErrorInvalidValue;
    if (val_bytes && (((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & (uintptr_t)(val_bytes - 1))) return hipErrorInvalidValue;
    {
        const void *arr[4] = {d_keys_in, d_keys_out, d_vals_in, d_vals_out};
        const size_t kbytes = num_items * (size_t)kb, vbytes = num_items * (size_t)val_bytes, bytes[4] = {kbytes, kbytes, vbytes, vbytes};
        if (any_overlap(arr, bytes)) return hipErrorInvalidValue;
    }
    if (!d_temp || temp_bytes < gs_lsb_narrow_large_temp_bytes(num_items, key_type, val_bytes)) return hipErrorInvalidValue;
    const uint64_t L = large_limit();
    if (num_items <= L)     // one slice: the plain narrow sort on the same arguments (a stable sort's result is unique)
        return gs_lsb_sort_narrow(d_temp, temp_bytes, d_keys_in, d_keys_out, d_vals_in, d_vals_out, num_items, key_type, val_bytes,
                                  begin_bit, end_bit, descending, stream);
    GS_CLEAR_STALE_ERROR();
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = num_items;
    const NarrowLargeWs w = narrow_large_carve(gs_ws_base(d_temp), n, L, val_bytes);

    if (begin_bit == end_bit) {
        if (int e = narrow_copy_bytes(d_keys_in, d_keys_out, n * (uint64_t)kb, s)) return e;
        return val_bytes ? narrow_copy_bytes(d_vals_in, d_vals_out, n * (uint64_t)val_bytes, s) : 0;
    }
    if (kb == 1 && val_bytes == 0 && begin_bit == 0 && end_bit == 8)   // count and fill: nothing is scattered, no slices
        return narrow_fill_large(d_keys_in, d_keys_out, n, key_type, descending, w.counts, s);

    const int num_passes = (end_bit - begin_bit + RADIX_BITS - 1) / RADIX_BITS;   // 1 or 2: in -> (workspace ->) out
    for (int pass = 0; pass < num_passes; ++pass) {
        const int shift = begin_bit + pass * RADIX_BITS;
        const bool first = pass == 0, last = pass == num_passes - 1;
        const LargeDigit d{shift, end_bit - shift < RADIX_BITS ? end_bit - shift : RADIX_BITS, key_type, descending, first, last};
        const char *kin = first ? (const char *)d_keys_in : w.tk;
        const char *vin = !val_bytes ? nullptr : first ? (const char *)d_vals_in : w.tv;
        char *kout = last ? (char *)d_keys_out : w.tk;
        char *vout = !val_bytes ? nullptr : last ? (char *)d_vals_out : w.tv;
        if (int e = narrow_large_pass(w, kin, kout, vin, vout, n, L, kb, val_bytes, d, s)) return e;
    }
    return (int)hipGetLastError();
}

}  // extern "C"
