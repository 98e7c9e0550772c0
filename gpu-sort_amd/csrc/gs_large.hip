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
#include "gs_device.hpp"
#include "gs_lsb.hpp"
#include <cstdlib>

namespace gs {

constexpr uint64_t LARGE_GROUP = 1ull << 31;   // keys per finish and per slice of the 64-bit pass
constexpr uint64_t LARGE_MAX = 1ull << 40;     // num_items limit of the entry point
constexpr uint32_t LARGE_MIN_TEST_LIMIT = 256;

// Test hook (tests/test_msb_large_gpu.py): GS_MSB_LARGE_TEST_LIMIT=k lowers the group size and the slice size to k keys,
// so that small arrays take multi-slice passes, multi-group finishes and splits.  Read on every call; never set in production.
static uint64_t large_limit()
{
    if (const char *e = getenv("GS_MSB_LARGE_TEST_LIMIT")) {
        const uint64_t k = strtoull(e, nullptr, 10);
        if (k >= LARGE_MIN_TEST_LIMIT && k < LARGE_GROUP) return k;
    }
    return LARGE_GROUP;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace of the 64-bit pass over m keys in slices of S: per slice its spine and prefix16 (gs_lsb.hip layout), then
// the slices' digit totals [slices][256] u32, the digit starts [slices][256] u64 and the bucket sizes [256] u64
struct LargePassWs {
    char *slice_ws;          // slice i: spine at slice_ws + i * per_slice, prefix16 behind it
    size_t per_slice, spine_bytes;
    uint32_t *totals;
    uint64_t *dbase;
    uint64_t *counts;
};
static inline uint64_t large_slices(uint64_t m, uint64_t S) { return m ? (m + S - 1) / S : 1; }
static inline void large_slice_bytes(uint64_t S, size_t &spine, size_t &prefix)
{
    const PassParams p = lsb_make_params(S, 24, 8);
    spine = align256((size_t)RADIX * p.grid * sizeof(uint32_t));
    prefix = align256((size_t)p.num_tiles * RADIX * sizeof(uint16_t));
}
// (every slice is carved at the size of a full one: the last one is never larger)
static size_t large_pass_bytes(uint64_t m, uint64_t S)
{
    size_t sp, pf;
    large_slice_bytes(S, sp, pf);
    const uint64_t ns = large_slices(m, S);
    return (size_t)ns * (sp + pf) + align256((size_t)ns * RADIX * sizeof(uint32_t)) + align256((size_t)ns * RADIX * sizeof(uint64_t)) +
           align256(RADIX * sizeof(uint64_t));
}
static LargePassWs large_pass_carve(void *temp, uint64_t m, uint64_t S)
{
    LargePassWs w;
    size_t pf;
    large_slice_bytes(S, w.spine_bytes, pf);
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

// The 64-bit pass: stable partition of m keys (and values) on the byte at `shift`, kin -> kout, with key_type's twiddle
// applied on read (GS_KEY_U32: none); the bucket sizes are copied to h_counts (the call waits for them).
static int large_pass(void *temp, uint64_t S, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, uint64_t m,
                      int shift, int key_type, uint64_t *h_counts, hipStream_t s)
{
    const LargePassWs w = large_pass_carve(temp, m, S);
    const uint64_t ns = large_slices(m, S);
    int e;
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = m - off < S ? m - off : S;
        PassParams p = lsb_make_params(len, shift, 8);
        lsb_twiddle_masks(key_type, 0, true, false, p);
        uint32_t *spine = (uint32_t *)(w.slice_ws + i * w.per_slice);
        uint16_t *prefix16 = (uint16_t *)(w.slice_ws + i * w.per_slice + w.spine_bytes);
        if ((e = lsb_upsweep(kin + off, spine, prefix16, p, s))) return e;
        if ((e = lsb_scan(spine, w.totals + i * RADIX, p.grid, s))) return e;
    }
    {
        KernelTimer kt(GS_K_OTHER, s);
        hipLaunchKernelGGL(large_offsets_kernel, dim3(1), dim3(RADIX), 0, s, (const uint32_t *)w.totals, (uint32_t)ns,
                           (unsigned long long *)w.dbase, (unsigned long long *)w.counts);
    }
    for (uint64_t i = 0; i < ns; ++i) {
        const uint64_t off = i * S, len = m - off < S ? m - off : S;
        PassParams p = lsb_make_params(len, shift, 8);
        lsb_twiddle_masks(key_type, 0, true, false, p);
        const uint32_t *spine = (const uint32_t *)(w.slice_ws + i * w.per_slice);
        const uint16_t *prefix16 = (const uint16_t *)(w.slice_ws + i * w.per_slice + w.spine_bytes);
        if ((e = lsb_downsweep64(kin + off, kout, vin ? vin + off : nullptr, vout, spine, prefix16, w.totals + i * RADIX,
                                 w.dbase + i * RADIX, p, s)))
            return e;
    }
    hipError_t he = hipMemcpyAsync(h_counts, w.counts, RADIX * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    return (int)he;
}

struct LargeCtx {
    uint32_t *k[2], *v[2];   // [0] = the caller's arrays (where the result goes), [1] = the alternates
    bool pairs;
    int key_type;
    uint64_t L;              // group size and slice size
    char *pass_ws;
    char *fin_ws;
    size_t fin_bytes;
    hipStream_t s;
    int synchronize;
};

static int large_copy_back(const LargeCtx &c, uint64_t off, uint64_t m)
{
    hipError_t e = hipMemcpyAsync(c.k[0] + off, c.k[1] + off, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.s);
    if (e == hipSuccess && c.pairs) e = hipMemcpyAsync(c.v[0] + off, c.v[1] + off, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.s);
    return (int)e;
}

// finish the group [off, off + m) that lies in buffer `b`, its buckets (by the byte just partitioned) sized gcounts
static int large_finish_group(const LargeCtx &c, int b, uint64_t off, uint64_t m, const uint64_t *gcounts)
{
    const int o = b ^ 1;
    int e = gs_msb_finish_u32(c.fin_ws, c.fin_bytes, c.k[b] + off, c.pairs ? c.v[b] + off : nullptr, c.k[o] + off,
                              c.pairs ? c.v[o] + off : nullptr, m, gcounts, 1, c.key_type, c.s, c.synchronize);
    if (e) return e;
    return o == 0 ? 0 : large_copy_back(c, off, m);   // (a split range of odd depth: the result landed in the alternates)
}

// The range [off, off + m) lies in buffer `cur`; its keys agree on every byte above `shift` (twiddled form).  Partition it on
// the byte at `shift` into the other buffer, then finish its buckets in groups, splitting the ones larger than a group.
static int large_range(const LargeCtx &c, uint64_t off, uint64_t m, int cur, int shift, int key_type_in)
{
    uint64_t counts[RADIX];
    const int nb = cur ^ 1;
    int e = large_pass(c.pass_ws, c.L, c.k[cur] + off, c.k[nb] + off, c.pairs ? c.v[cur] + off : nullptr,
                       c.pairs ? c.v[nb] + off : nullptr, m, shift, key_type_in, counts, c.s);
    if (e) return e;
    if (shift == 0) {
        // every byte is ordered: the range is sorted, each bucket one value.  Undo the twiddle on the way to the caller's arrays.
        PassParams tw{};
        lsb_twiddle_masks(c.key_type, 0, false, true, tw);
        if (nb == 0 && !tw.f32_out && !tw.xor_out) return 0;
        KernelTimer kt(GS_K_OTHER, c.s);
        const uint64_t blocks = (m + 255) / 256;
        hipLaunchKernelGGL(large_untwiddle_kernel, dim3(blocks < 8192 ? (uint32_t)blocks : 8192u), dim3(256), 0, c.s,
                           (const uint32_t *)(c.k[nb] + off), c.k[0] + off, (unsigned long long)m, tw.f32_out, tw.xor_out);
        if ((e = (int)hipGetLastError())) return e;
        if (nb == 1 && c.pairs)
            e = (int)hipMemcpyAsync(c.v[0] + off, c.v[1] + off, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.s);
        return e;
    }
    uint64_t gcounts[RADIX] = {};
    uint64_t at = off, gstart = off, gsize = 0;
    for (int b = 0; b < RADIX; ++b) {
        const uint64_t n_b = counts[b];
        if (n_b == 0) continue;
        if (gsize && (n_b > c.L || gsize + n_b > c.L)) {
            if ((e = large_finish_group(c, nb, gstart, gsize, gcounts))) return e;
            for (int q = 0; q < RADIX; ++q) gcounts[q] = 0;
            gsize = 0;
        }
        if (n_b > c.L) {
            if ((e = large_range(c, at, n_b, nb, shift - 8, GS_KEY_U32))) return e;
        } else {
            if (gsize == 0) gstart = at;
            gcounts[b] = n_b;
            gsize += n_b;
        }
        at += n_b;
    }
    if (gsize) e = large_finish_group(c, nb, gstart, gsize, gcounts);
    return e;
}

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_msb_large_temp_bytes(uint64_t num_items, int has_values)
{
    const uint64_t L = large_limit();
    return align256(large_pass_bytes(num_items, L)) + gs_msb_finish_temp_bytes(L, has_values, 1);
}

static bool overlaps(const uint32_t *a, const uint32_t *b, uint64_t n)
{
    if (!a || !b) return false;
    return a < b + n && b < a + n;
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
        const uint32_t *arr[4] = {d_keys, d_keys_alt, d_vals, pairs ? d_vals_alt : nullptr};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (overlaps(arr[i], arr[j], num_items)) return hipErrorInvalidValue;
    }
    GS_CLEAR_STALE_ERROR();
    hipStream_t s = (hipStream_t)stream;
    // the call reads bucket sizes back to the host: not allowed inside a capture, and nothing is enqueued
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) return (int)hipGetLastError();
    if (cs != hipStreamCaptureStatusNone) return hipErrorStreamCaptureUnsupported;

    const uint64_t L = large_limit();
    if (num_items <= L)   // one group: the plain MSB sort (its workspace fits in the finish's, both sized for L keys)
        return gs_msb_sort_u32(d_temp, temp_bytes, d_keys, d_vals, num_items, d_keys_alt, d_vals_alt, nullptr, nullptr, key_type,
                               stream, synchronize);

    LargeCtx c;
    c.k[0] = d_keys; c.k[1] = d_keys_alt;
    c.v[0] = d_vals; c.v[1] = pairs ? d_vals_alt : nullptr;
    c.pairs = pairs;
    c.key_type = key_type;
    c.L = L;
    c.pass_ws = (char *)d_temp;
    c.fin_ws = (char *)d_temp + align256(large_pass_bytes(num_items, L));
    c.fin_bytes = gs_msb_finish_temp_bytes(L, pairs, 1);
    c.s = s;
    c.synchronize = synchronize;
    int e = large_range(c, 0, num_items, 0, 24, key_type);
    if (e) return e;
    if ((e = (int)hipGetLastError())) return e;
    return synchronize ? (int)hipStreamSynchronize(s) : 0;
}

}  // extern "C"
