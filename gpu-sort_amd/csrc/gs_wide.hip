// gs_wide.hip -- the LSB three-kernel pass for the wider element types of the
// DeviceRadixSort contract (lsb/cub/test/test_device_radix_sort.cu
// :934-943,1244-1265): 64-bit keys (unsigned, signed, double) with no / 32-bit / 64-bit
// values, and 32-bit keys with 64-bit values.  The graded u32 / (u32,u32) configurations
// stay on the tuned kernels of gs_lsb.hip; this file trades some speed for generality:
//   - tiles of 4096 keys, 8 keys per thread, one tile per block in dispatch order;
//   - the same decomposition (spine per chunk of 8 tiles + u16 in-chunk prefixes), the
//     same wave64 ballot/popcount ranking and LDS staging;
//   - keys and values go through ONE staging buffer one after the other (a tile of
//     64-bit keys fills it), and partial tiles are handled in place with guarded loads.
#include "gs_device.hpp"
#include "gs_lsb.hpp"
#include <type_traits>

namespace gs {

constexpr int W_THREADS = 512;
constexpr int W_WAVES = W_THREADS / WAVE;
constexpr int W_KPT = 8;
constexpr int W_TILE = W_THREADS * W_KPT;   // 4096 elements
constexpr int W_CHUNK = W_WAVES;            // tiles per chunk (one wave per tile in the upsweep)

struct NoVal {};

struct WideParams {
    uint64_t n;
    uint32_t num_tiles, grid;       // grid = chunks
    uint32_t shift, bits, mask;
    int f_in, f_out;                // float twiddle on read / undo on write
    uint64_t xor_in, xor_out;       // sign flip and descending complement
};

template <typename K> __device__ __forceinline__ K w_twiddle_in(K k, int f, uint64_t x);
template <typename K> __device__ __forceinline__ K w_twiddle_out(K k, int f, uint64_t x);
template <> __device__ __forceinline__ uint32_t w_twiddle_in<uint32_t>(uint32_t k, int f, uint64_t x) { return twiddle_in(k, f, (uint32_t)x); }
template <> __device__ __forceinline__ uint32_t w_twiddle_out<uint32_t>(uint32_t k, int f, uint64_t x) { return twiddle_out(k, f, (uint32_t)x); }
// lsb/cub/cub/util_type.cuh:1079-1089 for 64-bit: negative -> flip all bits, else flip the sign bit
template <> __device__ __forceinline__ uint64_t w_twiddle_in<uint64_t>(uint64_t k, int f, uint64_t x)
{
    if (f) k ^= (uint64_t)((int64_t)k >> 63) | 0x8000000000000000ull;
    return k ^ x;
}
template <> __device__ __forceinline__ uint64_t w_twiddle_out<uint64_t>(uint64_t k, int f, uint64_t x)
{
    k ^= x;
    if (f) k ^= ~(uint64_t)((int64_t)k >> 63) | 0x8000000000000000ull;
    return k;
}
template <typename K> __device__ __forceinline__ uint32_t w_digit(K k, const WideParams &p) { return (uint32_t)(k >> p.shift) & p.mask; }

// ---------------------------------------------------------------- upsweep --
template <typename K>
__global__ __launch_bounds__(W_THREADS) void wide_upsweep_kernel(const K *__restrict__ keys, uint32_t *__restrict__ spine,
                                                                 uint16_t *__restrict__ prefix16, WideParams p)
{
    __shared__ uint32_t hist[W_WAVES][RADIX];
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    uint32_t *my = hist[w];
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    const uint32_t chunk = blockIdx.x;
    const uint32_t tile = chunk * W_CHUNK + (uint32_t)w;
    if (tile < p.num_tiles) {
        const uint64_t lo = (uint64_t)tile * W_TILE;
        const uint32_t len = (p.n - lo < (uint64_t)W_TILE) ? (uint32_t)(p.n - lo) : (uint32_t)W_TILE;
        const K *src = keys + lo;
        // batches of 16 loads from clamped indices (a loop of one guarded load per trip is latency-bound)
        constexpr int GB = 16;
        const uint32_t last = len - 1u;
#pragma unroll 1
        for (uint32_t j = 0; j < len; j += GB * WAVE) {
            K v[GB];
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const uint32_t idx = j + u * WAVE + lane;
                v[u] = __builtin_nontemporal_load(&src[idx < last ? idx : last]);
            }
#pragma unroll
            for (int u = 0; u < GB; ++u)
                if (j + u * WAVE + lane < len) hist_add(my, w_digit(w_twiddle_in<K>(v[u], p.f_in, p.xor_in), p));
        }
    }
    __syncthreads();
    if (tid < RADIX) {
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < W_WAVES; ++j) {
            const uint32_t t = chunk * W_CHUNK + (uint32_t)j;
            if (t < p.num_tiles) prefix16[(size_t)t * RADIX + tid] = (uint16_t)run;
            run += hist[j][tid];
        }
        spine[(uint32_t)tid * p.grid + chunk] = run;
    }
}

// the spine scan is gs_lsb.hip's (same layout)
int lsb_scan(uint32_t *spine, uint32_t *totals, uint32_t grid, hipStream_t s);

// -------------------------------------------------------------- downsweep --
template <typename K, typename V>
__global__ __launch_bounds__(W_THREADS, 4) void wide_downsweep_kernel(const K *__restrict__ keys_in, K *__restrict__ keys_out,
                                                                     const V *__restrict__ vals_in, V *__restrict__ vals_out,
                                                                     const uint32_t *__restrict__ spine,
                                                                     const uint16_t *__restrict__ prefix16,
                                                                     const uint32_t *__restrict__ totals, WideParams p)
{
    constexpr bool HAS_VALUES = !std::is_same<V, NoVal>::value, OFF64 = false;
    constexpr size_t ELEM = sizeof(K) > (HAS_VALUES ? sizeof(V) : 1) ? sizeof(K) : sizeof(V);
    using Off = uint32_t;
    __shared__ uint32_t whist[W_WAVES][RADIX];
    __shared__ uint32_t gbase[RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[W_TILE * ELEM];
    const uint64_t *dbase = nullptr;
#include "gs_wide_tile.inc"
}

// the downsweep of one slice of the 64-bit pass (gs_large.hip): keys_in / vals_in point at the slice, keys_out / vals_out at
// the whole output range, dbase[256] holds the slice's absolute u64 digit starts in it
template <typename K, typename V>
__global__ __launch_bounds__(W_THREADS, 4) void wide_downsweep64_kernel(const K *__restrict__ keys_in, K *__restrict__ keys_out,
                                                                       const V *__restrict__ vals_in, V *__restrict__ vals_out,
                                                                       const uint32_t *__restrict__ spine,
                                                                       const uint16_t *__restrict__ prefix16,
                                                                       const uint64_t *__restrict__ dbase, WideParams p)
{
    constexpr bool HAS_VALUES = !std::is_same<V, NoVal>::value, OFF64 = true;
    constexpr size_t ELEM = sizeof(K) > (HAS_VALUES ? sizeof(V) : 1) ? sizeof(K) : sizeof(V);
    using Off = uint64_t;
    __shared__ uint32_t whist[W_WAVES][RADIX];
    __shared__ __attribute__((aligned(16))) uint64_t gbase[RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[W_TILE * ELEM];
    const uint32_t *totals = nullptr;
#include "gs_wide_tile.inc"
}

// ------------------------------------------------------------------- host --
static inline size_t w_align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline uint32_t w_tiles(uint64_t n) { return (uint32_t)((n + W_TILE - 1) / W_TILE); }
static inline uint32_t w_grid(uint64_t n) { const uint32_t t = w_tiles(n); return t ? (t + W_CHUNK - 1) / W_CHUNK : 1u; }
static inline size_t w_spine_bytes(uint64_t n) { return w_align256((size_t)RADIX * w_grid(n) * 4); }
static inline size_t w_totals_bytes() { return w_align256(RADIX * 4); }
static inline size_t w_prefix_bytes(uint64_t n) { return w_align256((size_t)(w_tiles(n) ? w_tiles(n) : 1) * RADIX * 2); }

template <typename K, typename V>
static int wide_pass(const K *kin, K *kout, const V *vin, V *vout, uint32_t *spine, uint32_t *totals, uint16_t *prefix16,
                     const WideParams &p, hipStream_t s)
{
    { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
      hipLaunchKernelGGL(wide_upsweep_kernel<K>, dim3(p.grid), dim3(W_THREADS), 0, s, kin, spine, prefix16, p); }
    int e = lsb_scan(spine, totals, p.grid, s);
    if (e) return e;
    { KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
      hipLaunchKernelGGL((wide_downsweep_kernel<K, V>), dim3(p.num_tiles), dim3(W_THREADS), 0, s, kin, kout, vin, vout,
                         (const uint32_t *)spine, (const uint16_t *)prefix16, (const uint32_t *)totals, p); }
    return (int)hipGetLastError();
}

template <typename K, typename V>
static int wide_sort(void *d_temp, void *d_keys[2], void *d_vals[2], int *selector, uint64_t n, int begin_bit, int end_bit,
                     int descending, int key_type, hipStream_t s)
{
    char *c = (char *)d_temp;
    uint32_t *spine = (uint32_t *)c;
    uint32_t *totals = (uint32_t *)(c + w_spine_bytes(n));
    uint16_t *prefix16 = (uint16_t *)(c + w_spine_bytes(n) + w_totals_bytes());
    const int num_passes = (end_bit - begin_bit + RADIX_BITS - 1) / RADIX_BITS;
    const bool is_float = key_type == GS_KEY_F32 || key_type == GS_KEY_F64;
    const bool is_signed = key_type == GS_KEY_I32 || key_type == GS_KEY_I64;
    const uint64_t sign = is_signed ? (sizeof(K) == 8 ? 0x8000000000000000ull : 0x80000000ull) : 0ull;
    const uint64_t flip = descending ? ~0ull : 0ull;
    int sel = *selector;
    for (int pass = 0; pass < num_passes; ++pass) {
        WideParams p{};
        p.n = n; p.num_tiles = w_tiles(n); p.grid = w_grid(n);
        p.shift = (uint32_t)(begin_bit + pass * RADIX_BITS);
        p.bits = (uint32_t)((end_bit - (int)p.shift < RADIX_BITS) ? end_bit - (int)p.shift : RADIX_BITS);
        p.mask = (1u << p.bits) - 1u;
        const bool first = pass == 0, last = pass == num_passes - 1;
        p.f_in = (first && is_float) ? 1 : 0;
        p.f_out = (last && is_float) ? 1 : 0;
        p.xor_in = first ? (sign ^ flip) : 0ull;
        p.xor_out = last ? (sign ^ flip) : 0ull;
        const int e = wide_pass<K, V>((const K *)d_keys[sel], (K *)d_keys[sel ^ 1], d_vals ? (const V *)d_vals[sel] : nullptr,
                                      d_vals ? (V *)d_vals[sel ^ 1] : nullptr, spine, totals, prefix16, p, s);
        if (e) return e;
        sel ^= 1;
    }
    *selector = sel;
    return hipSuccess;
}

// ---- the 64-bit pass over the wide element types (gs_large.hip), one slice of < 2^31 elements at a time, on the digit
// d.bits wide at d.shift.  The key type's twiddle (and the descending complement) is applied on read when d.first and undone on
// write when d.last, the rule of wide_sort's passes; the MSB large sort sets both, so its keys keep the caller's representation.
void wide_slice_bytes(uint64_t S, size_t &spine, size_t &prefix)
{
    spine = w_spine_bytes(S);
    prefix = w_prefix_bytes(S);
}

static WideParams wide_slice_params(uint64_t len, int key_bytes, const LargeDigit &d)
{
    WideParams p{};
    p.n = len; p.num_tiles = w_tiles(len); p.grid = w_grid(len);
    p.shift = (uint32_t)d.shift; p.bits = (uint32_t)d.bits; p.mask = (1u << d.bits) - 1u;
    const int f = (d.key_type == GS_KEY_F32 || d.key_type == GS_KEY_F64) ? 1 : 0;
    const uint64_t sign = (d.key_type == GS_KEY_I32 || d.key_type == GS_KEY_I64) ? (key_bytes == 8 ? 0x8000000000000000ull : 0x80000000ull) : 0ull;
    const uint64_t x = sign ^ (d.descending ? ~0ull : 0ull);
    p.f_in = d.first ? f : 0;
    p.f_out = d.last ? f : 0;
    p.xor_in = d.first ? x : 0ull;
    p.xor_out = d.last ? x : 0ull;
    return p;
}

int wide_slice_count(const void *kin, uint64_t len, int key_bytes, const LargeDigit &d, uint32_t *spine, uint16_t *prefix16,
                     uint32_t *totals, hipStream_t s)
{
    const WideParams p = wide_slice_params(len, key_bytes, d);
    { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
      if (key_bytes == 8) hipLaunchKernelGGL(wide_upsweep_kernel<uint64_t>, dim3(p.grid), dim3(W_THREADS), 0, s, (const uint64_t *)kin, spine, prefix16, p);
      else hipLaunchKernelGGL(wide_upsweep_kernel<uint32_t>, dim3(p.grid), dim3(W_THREADS), 0, s, (const uint32_t *)kin, spine, prefix16, p); }
    return lsb_scan(spine, totals, p.grid, s);
}

int wide_slice_scatter(const void *kin, void *kout, const void *vin, void *vout, uint64_t len, int key_bytes, int val_bytes,
                       const LargeDigit &d, const uint32_t *spine, const uint16_t *prefix16, const uint64_t *dbase, hipStream_t s)
{
    const WideParams p = wide_slice_params(len, key_bytes, d);
    KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
#define GS_W64(K, V) hipLaunchKernelGGL((wide_downsweep64_kernel<K, V>), dim3(p.num_tiles), dim3(W_THREADS), 0, s, (const K *)kin, (K *)kout, \
                                        (const V *)vin, (V *)vout, spine, prefix16, dbase, p)
    if (key_bytes == 8) {
        if (val_bytes == 0) GS_W64(uint64_t, NoVal);
        else if (val_bytes == 4) GS_W64(uint64_t, uint32_t);
        else GS_W64(uint64_t, uint64_t);
    } else {
        GS_W64(uint32_t, uint64_t);
    }
#undef GS_W64
    return (int)hipGetLastError();
}

// where a wide pass leaves its digit totals inside the workspace (the MSB path for wide types reads them after its
// top-byte partition, which is one wide pass)
const uint32_t *wide_totals_ptr(void *d_temp, uint64_t n) { return (const uint32_t *)((char *)d_temp + w_spine_bytes(n)); }

}  // namespace gs

using namespace gs;

extern "C" {

size_t gs_lsb_wide_temp_bytes(uint64_t num_items, int /*key_bytes*/, int /*val_bytes*/)
{
    return w_spine_bytes(num_items) + w_totals_bytes() + w_prefix_bytes(num_items) + GS_WS_SLACK;
}

int gs_lsb_sort_wide(void *d_temp, size_t temp_bytes, void *d_keys[2], void *d_vals[2], int *selector, uint64_t num_items,
                     int key_bytes, int val_bytes, int begin_bit, int end_bit, int descending, int key_type, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    if (!selector || (*selector != 0 && *selector != 1) || !d_keys) return hipErrorInvalidValue;
    if (key_bytes != 4 && key_bytes != 8) return hipErrorInvalidValue;
    if (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) return hipErrorInvalidValue;
    if ((val_bytes != 0) != (d_vals != nullptr)) return hipErrorInvalidValue;
    if (begin_bit < 0 || end_bit > 8 * key_bytes || begin_bit > end_bit) return hipErrorInvalidValue;
    if (num_items >= (1ull << 32)) return hipErrorInvalidValue;
    const bool k64 = key_bytes == 8;
    if (k64 ? (key_type < GS_KEY_U64 || key_type > GS_KEY_F64) : (key_type < GS_KEY_U32 || key_type > GS_KEY_F32))
        return hipErrorInvalidValue;
    if (num_items == 0 || begin_bit == end_bit) return hipSuccess;
    if (!d_temp || temp_bytes < gs_lsb_wide_temp_bytes(num_items, key_bytes, val_bytes)) return hipErrorInvalidValue;
    if (!d_keys[0] || !d_keys[1] || (d_vals && (!d_vals[0] || !d_vals[1]))) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
#define GS_WIDE(K, V) return wide_sort<K, V>(gs_ws_base(d_temp), d_keys, d_vals, selector, num_items, begin_bit, end_bit, descending, key_type, s)
    if (k64) {
        if (val_bytes == 0) GS_WIDE(uint64_t, NoVal);
        if (val_bytes == 4) GS_WIDE(uint64_t, uint32_t);
        GS_WIDE(uint64_t, uint64_t);
    }
    if (val_bytes == 0) GS_WIDE(uint32_t, NoVal);
    if (val_bytes == 4) GS_WIDE(uint32_t, uint32_t);
    GS_WIDE(uint32_t, uint64_t);
#undef GS_WIDE
}

}  // extern "C"
