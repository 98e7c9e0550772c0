// gs_narrow.hip -- the LSB sort of 8- and 16-bit keys (bool / char / signed char / unsigned char / short / unsigned short)
// with no values or values of 1, 2, 4, 8 or 16 bytes, on kernels of its own: keys and values stay at their own width in HBM
// and in LDS.  gs_lsb_sort_any (gs_any.hip) widens such keys to (u32 sort key, u32 index) pairs, sorts those and gathers;
// this file is the native route for the same plain-pointer contract.
//   (a) the digit pass: a stable 8-bit pass of upsweep, spine scan (gs_lsb.hip's) and downsweep, the decomposition of
//       gs_wide.hip with K = 1 or 2 bytes.  One pass serves 8-bit keys, two serve 16-bit keys (in -> workspace -> out);
//       a bit range of 8 bits or fewer is one pass whatever the key's width.
//       - The tile is sized by its bytes in LDS and its registers: 512 threads x 16 / 8 / 4 elements for values of <= 4 / 8 / 16
//         bytes (8192, 4096, 2048 elements): the one staging buffer (keys, then values) is 8 to 32 KiB, and 16 elements per
//         thread keep the downsweep at 4 waves per SIMD (32 per thread took 184-226 VGPRs: 2 waves per SIMD).
//       - Keys, and 1- and 2-byte values, are read from HBM as aligned 16-byte chunks into LDS (a u8 array may start at any
//         byte and a u16 array at any even one: the chunks are read from the aligned address below, and only chunks that
//         hold an element of the array are touched), and each lane takes its elements from there: element i of lane l of
//         wave w is element w * 64 * KPT + i * 64 + l of the tile, the wave-striped order the ballot ranking needs.
//       - The spine has one column per TILE ([256][tiles] u32, 1 KiB per tile) instead of the wide pass's chunks of 8 tiles
//         with u16 in-chunk prefixes: a third more workspace, one array less.
//       - Keys are never rewritten: the sign flip and the descending complement are an xor on the way to the digit.
//   (b) 8-bit keys, keys only, all 8 bits (the default SortKeys call): a 256-bin histogram and a fill of the output with
//       runs; nothing is scattered.  Descending and signed keys only change the order the bins are walked in.
// 16-bit keys, keys only, take two passes of (a): the 65536-bin fill is not built.
//   (c) above 2^32 elements (gs_lsb_sort_narrow_large, host loop in gs_large.hip): the slice functions at the end of this file run
//       (a) on slices of 2^31 elements with u64 digit starts (narrow_downsweep64_kernel) and (b) with u64 counts.
#include "gs_device.hpp"
#include "gs_lsb.hpp"

namespace gs {

constexpr int N_THREADS = 512;
constexpr int N_WAVES = N_THREADS / WAVE;
constexpr uint32_t N_SHARED_TILES = 2048;   // up to this many tiles, an upsweep block counts one tile with all its waves

constexpr int narrow_kpt(int vb) { return vb <= 4 ? 16 : vb == 8 ? 8 : 4; }
constexpr int narrow_tile(int vb) { return N_THREADS * narrow_kpt(vb); }

template <int B> struct NElem;
template <> struct NElem<1> { typedef uint8_t type; };
template <> struct NElem<2> { typedef uint16_t type; };
template <> struct NElem<4> { typedef uint32_t type; };
template <> struct NElem<8> { typedef uint64_t type; };
template <> struct NElem<16> { typedef uint4 type; };

struct NarrowParams {
    uint64_t n;
    uint32_t num_tiles;
    uint32_t shift, mask;   // digit = ((key ^ xr) >> shift) & mask
    uint32_t xr;            // sign flip of the key's own width, complement when descending
};

// FK: the key is a sign-magnitude float of KB bytes (GS_KEY_F8 / F16 / BF16): a set sign bit flips the magnitude bits as well
// (cub::Traits<float>::TwiddleIn at the key's own width; the sign flip itself is in xr, as for a signed integer).  A template
// parameter, so that the integer kernels keep the code they had.
template <int KB, bool FK>
__device__ __forceinline__ uint32_t n_digit(uint32_t k, const NarrowParams &p)
{
    return ((float_flip<FK ? 8 * KB : 0>(k) ^ p.xr) >> p.shift) & p.mask;
}

// ---------------------------------------------------------------- upsweep --
// A block counts tpb tiles (8: one wave per tile; 1: the 8 waves share one tile, for arrays of few tiles, where 8 tiles
// per block would leave most of the chip idle): a wave reads 16-byte chunks that hold its share of the tile and counts the
// digits of the elements that belong to it in a wave-private LDS histogram.
template <int KB, int TILE, bool FK>
__global__ __launch_bounds__(N_THREADS) void narrow_upsweep_kernel(const void *__restrict__ keys, uint32_t *__restrict__ spine,
                                                                   NarrowParams p, uint32_t tpb)
{
    __shared__ uint32_t hist[N_WAVES][RADIX];
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    uint32_t *my = hist[w];
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    const uint32_t wpt = (uint32_t)N_WAVES / tpb;                 // waves per tile
    const uint32_t tile = blockIdx.x * tpb + (uint32_t)w / wpt;
    if (tile < p.num_tiles) {
        const uint64_t tile_base = (uint64_t)tile * TILE;
        const uint32_t valid = (p.n - tile_base < (uint64_t)TILE) ? (uint32_t)(p.n - tile_base) : (uint32_t)TILE;
        const uint32_t a = (uint32_t)((uintptr_t)keys & 15u);
        const uint4 *A = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(keys) - a) + tile_base * KB / 16;
        const uint32_t end_byte = a + valid * KB;                 // the tile's elements are bytes [a, end_byte) from A
        const uint32_t nch = (end_byte + 15u) / 16u;
        constexpr int GB = 4;
#pragma unroll 1
        for (uint32_t j = ((uint32_t)w % wpt) * (GB * WAVE); j < nch; j += wpt * (GB * WAVE)) {
            uint4 v[GB];
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const uint32_t c = j + u * WAVE + lane;
                v[u] = A[c < nch ? c : nch - 1u];
            }
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const uint32_t c = j + u * WAVE + lane;
                if (c >= nch) continue;
                const uint32_t b0 = c * 16u;
                const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                if (b0 >= a && b0 + 16u <= end_byte) {
#pragma unroll
                    for (int q = 0; q < 16 / KB; ++q) {
                        const uint32_t k = (x[q * KB / 4] >> (8 * (q * KB % 4))) & (KB == 1 ? 0xffu : 0xffffu);
                        hist_add(my, n_digit<KB, FK>(k, p));
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 16 / KB; ++q) {
                        const uint32_t k = (x[q * KB / 4] >> (8 * (q * KB % 4))) & (KB == 1 ? 0xffu : 0xffffu);
                        const uint32_t b = b0 + q * KB;
                        if (b >= a && b < end_byte) hist_add(my, n_digit<KB, FK>(k, p));
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid < RADIX) {
        for (uint32_t j = 0; j < tpb; ++j) {
            const uint32_t t = blockIdx.x * tpb + j;
            uint32_t sum = 0;
            for (uint32_t u = 0; u < wpt; ++u) sum += hist[j * wpt + u][tid];
            if (t < p.num_tiles) spine[(size_t)tid * p.num_tiles + t] = sum;
        }
    }
}

// -------------------------------------------------------------- downsweep --
// the aligned 16-byte chunks that hold `bytes` bytes starting `a` (< 16) bytes into chunk 0 of A, copied to raw
template <int MAX_CHUNKS>
__device__ __forceinline__ void n_stage_in(const uint4 *__restrict__ A, uint32_t nch, unsigned char *raw)
{
    constexpr int IT = (MAX_CHUNKS + N_THREADS - 1) / N_THREADS;
    uint4 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t c = (uint32_t)threadIdx.x + it * N_THREADS;
        v[it] = A[c < nch ? c : nch - 1u];          // unconditional loads from clamped chunks
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t c = (uint32_t)threadIdx.x + it * N_THREADS;
        if (c < nch) reinterpret_cast<uint4 *>(raw)[c] = v[it];
    }
}

// OFF64 = false (narrow_downsweep_kernel): the tile of a whole array (n < 2^32): the digit starts are the exclusive scan of
// totals[256].  OFF64 = true (narrow_downsweep64_kernel): the tile belongs to one slice (< 2^31 elements) of a larger array
// (gs_large.hip's 64-bit pass): keys_in / vals_in point at the slice, keys_out / vals_out at the whole output, spine is the
// slice's own and dbase[d] the absolute u64 start of the slice's run of digit d, so gbase (1 KiB more LDS) and the
// destination indices are u64.  The body is gs_narrow_tile.inc.
template <int KB, int VB, bool FK>
__global__ __launch_bounds__(N_THREADS) void narrow_downsweep_kernel(const void *__restrict__ keys_in, void *__restrict__ keys_out,
                                                                     const void *__restrict__ vals_in, void *__restrict__ vals_out,
                                                                     const uint32_t *__restrict__ spine,
                                                                     const uint32_t *__restrict__ totals, NarrowParams p)
{
    typedef typename NElem<KB>::type K;
    constexpr int KPT = narrow_kpt(VB), TILE = narrow_tile(VB);
    constexpr int ELEM = KB > VB ? KB : VB;
    __shared__ uint32_t whist[N_WAVES][RADIX];
    __shared__ uint32_t gbase[RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[TILE * ELEM + 16];   // (+ 16: the chunk a misaligned tile spills into)
    constexpr bool OFF64 = false;
    typedef uint32_t Off;
    const uint64_t *dbase = nullptr;
#include "gs_narrow_tile.inc"
}

template <int KB, int VB, bool FK>
__global__ __launch_bounds__(N_THREADS) void narrow_downsweep64_kernel(const void *__restrict__ keys_in, void *__restrict__ keys_out,
                                                                       const void *__restrict__ vals_in, void *__restrict__ vals_out,
                                                                       const uint32_t *__restrict__ spine,
                                                                       const uint64_t *__restrict__ dbase, NarrowParams p)
{
    typedef typename NElem<KB>::type K;
    constexpr int KPT = narrow_kpt(VB), TILE = narrow_tile(VB);
    constexpr int ELEM = KB > VB ? KB : VB;
    __shared__ uint32_t whist[N_WAVES][RADIX];
    __shared__ uint64_t gbase[RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[TILE * ELEM + 16];
    constexpr bool OFF64 = true;
    typedef uint64_t Off;
    const uint32_t *totals = nullptr;
#include "gs_narrow_tile.inc"
}

// ------------------------------------------- 8-bit keys only: count, fill --
constexpr int NF_THREADS = 256;
constexpr int NF_WAVES = NF_THREADS / WAVE;
constexpr uint32_t NF_MAX_BLOCKS = 2048;

// counts[v] += number of keys with the byte value v (no twiddle: the fill walks the bins in the order asked for).
// C = uint64_t (narrow_count8_large_kernel, n < 2^40): only the global counters are 64-bit.  A block's partial sums stay
// u32: the grid-stride loop gives a block at most ceil(chunks / gridDim.x) rounds of NF_THREADS chunks of 16 keys, and above
// 2^32 keys the grid is NF_MAX_BLOCKS = 2048 blocks (n_count_grid), so a block sees fewer than 2^40 / 2048 + 16 * NF_THREADS
// = 2^29 + 4096 keys in all, and the sum of its four wave histograms cannot wrap.
template <typename C>
__device__ __forceinline__ void narrow_count8_body(const void *__restrict__ keys, C *__restrict__ counts, uint64_t n)
{
    __shared__ uint32_t hist[NF_WAVES][RADIX];
    const int w = wave_id(), lane = lane_id();
    uint32_t *my = hist[w];
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    const uint32_t a = (uint32_t)((uintptr_t)keys & 15u);
    const uint4 *A = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(keys) - a);
    const uint64_t end_byte = a + n;                       // the keys are bytes [a, end_byte) from A
    const uint64_t nch = (end_byte + 15u) / 16u;
    const uint64_t stride = (uint64_t)gridDim.x * NF_THREADS;
    for (uint64_t c = (uint64_t)blockIdx.x * NF_THREADS + threadIdx.x; c < nch; c += stride) {
        const uint4 v = A[c];
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        const uint64_t b0 = c * 16u;
        if (b0 >= a && b0 + 16u <= end_byte) {
#pragma unroll
            for (int q = 0; q < 16; ++q) hist_add(my, (x[q / 4] >> (8 * (q % 4))) & 0xffu);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (b0 + q >= a && b0 + q < end_byte) hist_add(my, (x[q / 4] >> (8 * (q % 4))) & 0xffu);
        }
    }
    __syncthreads();
    const uint32_t d = threadIdx.x;
    const uint32_t sum = hist[0][d] + hist[1][d] + hist[2][d] + hist[3][d];
    if constexpr (sizeof(C) == 8) {
        if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(&counts[d]), (unsigned long long)sum);
    } else {
        if (sum) atomicAdd(&counts[d], sum);
    }
}

__global__ __launch_bounds__(NF_THREADS) void narrow_count8_kernel(const void *__restrict__ keys, uint32_t *__restrict__ counts, uint64_t n)
{
    narrow_count8_body<uint32_t>(keys, counts, n);
}

__global__ __launch_bounds__(NF_THREADS) void narrow_count8_large_kernel(const void *__restrict__ keys, uint64_t *__restrict__ counts, uint64_t n)
{
    narrow_count8_body<uint64_t>(keys, counts, n);
}

// bin j of the walk holds the key whose image, complemented when descending, is j: the image is key ^ sign for the integer
// types (sign = 0x80 for I8) and, for GS_KEY_F8 (sign = 0x80, mag = 0x7f; mag = 0 otherwise), key ^ (key & 0x80 ? 0xff : 0x80)
__device__ __forceinline__ uint32_t nf_key(uint32_t j, uint32_t sign, uint32_t mag, int descending)
{
    const uint32_t u = ((descending ? 255u - j : j) ^ sign) & 0xffu;
    return u ^ ((0u - (u >> 7)) & mag);
}

// out[i] = the key of rank i
__global__ __launch_bounds__(NF_THREADS) void narrow_fill8_kernel(void *__restrict__ keys_out, const uint32_t *__restrict__ counts, uint64_t n,
                                                                  uint32_t sign, uint32_t mag, int descending)
{
    __shared__ uint32_t scratch[8];
    __shared__ uint32_t ends[RADIX];            // ends[j]: number of keys in bins 0..j (n < 2^32)
    const uint32_t j0 = threadIdx.x;
    const uint32_t cnt = counts[nf_key(j0, sign, mag, descending)];
    ends[j0] = block_exclusive_scan_256(cnt, scratch, nullptr) + cnt;
    __syncthreads();
    const uint32_t a = (uint32_t)((uintptr_t)keys_out & 15u);
    unsigned char *A = reinterpret_cast<unsigned char *>(keys_out) - a;
    const uint64_t end_byte = a + n;
    const uint64_t nch = (end_byte + 15u) / 16u;
    const uint64_t stride = (uint64_t)gridDim.x * NF_THREADS;
    for (uint64_t c = (uint64_t)blockIdx.x * NF_THREADS + threadIdx.x; c < nch; c += stride) {
        const uint64_t b0 = c * 16u;
        const uint64_t lo = b0 < a ? a : b0, hi = b0 + 16u < end_byte ? b0 + 16u : end_byte;   // bytes [lo, hi) of this chunk are keys
        const uint32_t e = (uint32_t)(lo - a);             // rank of the first of them
        uint32_t j = 0;                                     // smallest j with ends[j] > e
#pragma unroll
        for (uint32_t s = 128; s > 0; s >>= 1)
            if (ends[j + s - 1] <= e) j += s;
        const uint32_t v = nf_key(j, sign, mag, descending);
        if (hi - lo == 16u && ends[j] - e >= 16u) {         // a whole chunk inside one run
            const uint32_t v4 = v * 0x01010101u;
            *reinterpret_cast<uint4 *>(A + b0) = make_uint4(v4, v4, v4, v4);
        } else if (hi - lo == 16u) {
            uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                while (ends[j] <= e + q) ++j;
                x[q / 4] |= nf_key(j, sign, mag, descending) << (8 * (q % 4));
            }
            *reinterpret_cast<uint4 *>(A + b0) = make_uint4(x[0], x[1], x[2], x[3]);
        } else {                                            // the array's first or last chunk: byte stores
            for (uint64_t b = lo; b < hi; ++b) {
                while (ends[j] <= (uint32_t)(b - a)) ++j;
                A[b] = (unsigned char)nf_key(j, sign, mag, descending);
            }
        }
    }
}

// the same for n < 2^40 (gs_lsb_sort_narrow_large): the counts, ends[], the rank e and the search are 64-bit
__global__ __launch_bounds__(NF_THREADS) void narrow_fill8_large_kernel(void *__restrict__ keys_out, const uint64_t *__restrict__ counts, uint64_t n,
                                                                        uint32_t sign, uint32_t mag, int descending)
{
    __shared__ uint64_t ends[RADIX];            // ends[j]: number of keys in bins 0..j
    const uint32_t j0 = threadIdx.x;
    const uint64_t cnt = counts[nf_key(j0, sign, mag, descending)];
    ends[j0] = cnt;                             // inclusive scan in place, once per block
    __syncthreads();
    for (uint32_t off = 1; off < RADIX; off <<= 1) {
        const uint64_t v = j0 >= off ? ends[j0 - off] : 0ull;
        __syncthreads();
        ends[j0] += v;
        __syncthreads();
    }
    const uint32_t a = (uint32_t)((uintptr_t)keys_out & 15u);
    unsigned char *A = reinterpret_cast<unsigned char *>(keys_out) - a;
    const uint64_t end_byte = a + n;
    const uint64_t nch = (end_byte + 15u) / 16u;
    const uint64_t stride = (uint64_t)gridDim.x * NF_THREADS;
    for (uint64_t c = (uint64_t)blockIdx.x * NF_THREADS + threadIdx.x; c < nch; c += stride) {
        const uint64_t b0 = c * 16u;
        const uint64_t lo = b0 < a ? a : b0, hi = b0 + 16u < end_byte ? b0 + 16u : end_byte;   // bytes [lo, hi) of this chunk are keys
        const uint64_t e = lo - a;                         // rank of the first of them
        uint32_t j = 0;                                     // smallest j with ends[j] > e
#pragma unroll
        for (uint32_t s = 128; s > 0; s >>= 1)
            if (ends[j + s - 1] <= e) j += s;
        const uint32_t v = nf_key(j, sign, mag, descending);
        if (hi - lo == 16u && ends[j] - e >= 16u) {         // a whole chunk inside one run
            const uint32_t v4 = v * 0x01010101u;
            *reinterpret_cast<uint4 *>(A + b0) = make_uint4(v4, v4, v4, v4);
        } else if (hi - lo == 16u) {
            uint32_t x[4] = {0, 0, 0, 0};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                while (ends[j] <= e + q) ++j;
                x[q / 4] |= nf_key(j, sign, mag, descending) << (8 * (q % 4));
            }
            *reinterpret_cast<uint4 *>(A + b0) = make_uint4(x[0], x[1], x[2], x[3]);
        } else {                                            // the array's first or last chunk: byte stores
            for (uint64_t b = lo; b < hi; ++b) {
                while (ends[j] <= b - a) ++j;
                A[b] = (unsigned char)nf_key(j, sign, mag, descending);
            }
        }
    }
}

// begin_bit == end_bit: the output is the input
__global__ __launch_bounds__(256) void narrow_copy_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, uint64_t bytes)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < bytes; i += stride) out[i] = in[i];
}

// ------------------------------------------------------------------- host --
static inline size_t n_align256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int n_key_bytes(int key_type)
{
    switch (key_type) {
    case GS_KEY_U8: case GS_KEY_I8: case GS_KEY_F8: return 1;
    case GS_KEY_U16: case GS_KEY_I16: case GS_KEY_F16: case GS_KEY_BF16: return 2;
    default: return 0;
    }
}
static inline bool n_float(int key_type) { return key_type == GS_KEY_F8 || key_type == GS_KEY_F16 || key_type == GS_KEY_BF16; }
// the sign bit of the signed types, at the key's own width (0 for the unsigned ones)
static inline uint32_t n_sign(int key_type)
{
    switch (key_type) {
    case GS_KEY_I8: case GS_KEY_F8: return 0x80u;
    case GS_KEY_I16: case GS_KEY_F16: case GS_KEY_BF16: return 0x8000u;
    default: return 0u;
    }
}
static inline bool n_val_ok(int vb) { return vb == 0 || vb == 1 || vb == 2 || vb == 4 || vb == 8 || vb == 16; }
static inline uint32_t n_tiles(uint64_t n, int vb)
{
    const uint64_t T = (uint64_t)narrow_tile(vb);
    const uint64_t t = (n + T - 1) / T;
    return (uint32_t)(t ? t : 1);
}
static inline size_t n_spine_bytes(uint64_t n, int vb) { return n_align256((size_t)RADIX * n_tiles(n, vb) * 4); }
static inline size_t n_totals_bytes() { return n_align256(RADIX * 4); }

template <int KB, int VB, bool FK>
static int narrow_pass(const void *kin, void *kout, const void *vin, void *vout, uint32_t *spine, uint32_t *totals,
                       const NarrowParams &p, hipStream_t s)
{
    constexpr int TILE = narrow_tile(VB);
    const uint32_t tpb = p.num_tiles > N_SHARED_TILES ? (uint32_t)N_WAVES : 1u;
    { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
      hipLaunchKernelGGL((narrow_upsweep_kernel<KB, TILE, FK>), dim3((p.num_tiles + tpb - 1) / tpb), dim3(N_THREADS), 0, s, kin, spine, p, tpb); }
    const int e = lsb_scan(spine, totals, p.num_tiles, s);
    if (e) return e;
    { KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
      hipLaunchKernelGGL((narrow_downsweep_kernel<KB, VB, FK>), dim3(p.num_tiles), dim3(N_THREADS), 0, s, kin, kout, vin, vout,
                         (const uint32_t *)spine, (const uint32_t *)totals, p); }
    return (int)hipGetLastError();
}

static int narrow_pass_dispatch(int kb, int vb, bool fk, const void *kin, void *kout, const void *vin, void *vout, uint32_t *spine,
                                uint32_t *totals, const NarrowParams &p, hipStream_t s)
{
#define GS_N(KB_, VB_) do { if (fk) return narrow_pass<KB_, VB_, true>(kin, kout, vin, vout, spine, totals, p, s); \
                            return narrow_pass<KB_, VB_, false>(kin, kout, vin, vout, spine, totals, p, s); } while (0)
#define GS_NV(KB_) switch (vb) { case 0: GS_N(KB_, 0); case 1: GS_N(KB_, 1); case 2: GS_N(KB_, 2); case 4: GS_N(KB_, 4); \
                                 case 8: GS_N(KB_, 8); default: GS_N(KB_, 16); }
    if (kb == 1) GS_NV(1)
    GS_NV(2)
#undef GS_NV
#undef GS_N
}

static inline dim3 n_stream_grid(uint64_t items, uint32_t per_block)
{
    const uint64_t b = (items + per_block - 1) / per_block;
    return dim3((unsigned)(b < 1 ? 1 : (b > NF_MAX_BLOCKS ? NF_MAX_BLOCKS : b)));
}

// the grid of the count and the fill over n keys: one chunk per thread up to 256 blocks, then more chunks per thread (every
// block ends with 256 global atomics on the same 256 counters: 2^24 keys took 0.056 ms with 2048 blocks and 0.034 ms with
// 512), up to 2048 blocks
static inline dim3 n_count_grid(uint64_t n)
{
    const uint64_t chunks = (n + 15) / 16 + 1;
    return chunks <= 256ull * NF_THREADS * 8 ? n_stream_grid(chunks < 256ull * NF_THREADS ? chunks : 256ull * NF_THREADS, NF_THREADS)
                                             : n_stream_grid(chunks, NF_THREADS * 8);
}

// ---- the 64-bit pass over 8- and 16-bit keys (gs_large.hip: gs_lsb_sort_narrow_large), one slice of < 2^31 elements at a
// time, on the digit d.bits wide at d.shift of the key mapped by d.key_type's sign flip (complemented when d.descending).
// Keys are never rewritten, so d.first / d.last play no part.  The count runs the upsweep and the spine scan (digit totals of
// the slice into totals[256]); the scatter writes the slice through dbase[256], the absolute u64 start of its run of each
// digit in kout / vout.  The slice pointers may have any alignment the element size allows.
int narrow_key_bytes(int key_type) { return n_key_bytes(key_type); }
size_t narrow_slice_spine_bytes(uint64_t S, int val_bytes) { return n_spine_bytes(S, val_bytes); }

static NarrowParams narrow_slice_params(uint64_t len, int val_bytes, const LargeDigit &d)
{
    NarrowParams p{};
    p.n = len; p.num_tiles = n_tiles(len, val_bytes);
    p.shift = (uint32_t)d.shift;
    p.mask = (1u << d.bits) - 1u;
    p.xr = n_sign(d.key_type) ^ (d.descending ? 0xffffffffu : 0u);
    return p;
}

int narrow_slice_count(const void *kin, uint64_t len, int val_bytes, const LargeDigit &d, uint32_t *spine, uint32_t *totals, hipStream_t s)
{
    const NarrowParams p = narrow_slice_params(len, val_bytes, d);
    const uint32_t tpb = p.num_tiles > N_SHARED_TILES ? (uint32_t)N_WAVES : 1u;
    const dim3 grid((p.num_tiles + tpb - 1) / tpb), block(N_THREADS);
    { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
#define GS_NU(KB_, VB_) do { if (n_float(d.key_type)) hipLaunchKernelGGL((narrow_upsweep_kernel<KB_, narrow_tile(VB_), true>), grid, block, 0, s, kin, spine, p, tpb); \
                             else hipLaunchKernelGGL((narrow_upsweep_kernel<KB_, narrow_tile(VB_), false>), grid, block, 0, s, kin, spine, p, tpb); } while (0)
      if (n_key_bytes(d.key_type) == 1) { if (val_bytes <= 4) GS_NU(1, 4); else if (val_bytes == 8) GS_NU(1, 8); else GS_NU(1, 16); }
      else { if (val_bytes <= 4) GS_NU(2, 4); else if (val_bytes == 8) GS_NU(2, 8); else GS_NU(2, 16); }
#undef GS_NU
    }
    return lsb_scan(spine, totals, p.num_tiles, s);
}

template <int KB, bool FK>
static void narrow_scatter64(int vb, const void *kin, void *kout, const void *vin, void *vout, const uint32_t *spine,
                             const uint64_t *dbase, const NarrowParams &p, hipStream_t s)
{
#define GS_N64(VB_) hipLaunchKernelGGL((narrow_downsweep64_kernel<KB, VB_, FK>), dim3(p.num_tiles), dim3(N_THREADS), 0, s, kin, kout, vin, vout, \
                                       spine, dbase, p)
    switch (vb) {
    case 0: GS_N64(0); break;
    case 1: GS_N64(1); break;
    case 2: GS_N64(2); break;
    case 4: GS_N64(4); break;
    case 8: GS_N64(8); break;
    default: GS_N64(16); break;
    }
#undef GS_N64
}

int narrow_slice_scatter(const void *kin, void *kout, const void *vin, void *vout, uint64_t len, int val_bytes, const LargeDigit &d,
                         const uint32_t *spine, const uint64_t *dbase, hipStream_t s)
{
    const NarrowParams p = narrow_slice_params(len, val_bytes, d);
    KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
    const bool fk = n_float(d.key_type);
    if (n_key_bytes(d.key_type) == 1) {
        if (fk) narrow_scatter64<1, true>(val_bytes, kin, kout, vin, vout, spine, dbase, p, s);
        else narrow_scatter64<1, false>(val_bytes, kin, kout, vin, vout, spine, dbase, p, s);
    } else {
        if (fk) narrow_scatter64<2, true>(val_bytes, kin, kout, vin, vout, spine, dbase, p, s);
        else narrow_scatter64<2, false>(val_bytes, kin, kout, vin, vout, spine, dbase, p, s);
    }
    return (int)hipGetLastError();
}

// 8-bit keys alone over all 8 bits, n < 2^40: the histogram with u64 counters (counts[256], zeroed here) and the fill
int narrow_fill_large(const void *kin, void *kout, uint64_t n, int key_type, int descending, uint64_t *counts, hipStream_t s)
{
    hipError_t ze = zero_async(counts, RADIX * sizeof(uint64_t), s);
    if (ze != hipSuccess) return (int)ze;
    const dim3 g = n_count_grid(n);
    { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
      hipLaunchKernelGGL(narrow_count8_large_kernel, g, dim3(NF_THREADS), 0, s, kin, counts, n); }
    { KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
      hipLaunchKernelGGL(narrow_fill8_large_kernel, g, dim3(NF_THREADS), 0, s, kout, (const uint64_t *)counts, n,
                         n_sign(key_type), n_float(key_type) ? 0x7fu : 0u, descending ? 1 : 0); }
    return (int)hipGetLastError();
}

// begin_bit == end_bit: the output is the input (bytes of either array)
int narrow_copy_bytes(const void *in, void *out, uint64_t bytes, hipStream_t s)
{
    hipLaunchKernelGGL(narrow_copy_kernel, n_stream_grid(bytes, 256 * 16), dim3(256), 0, s, (const unsigned char *)in, (unsigned char *)out, bytes);
    return (int)hipGetLastError();
}

}  // namespace gs

using namespace gs;

extern "C" {

uint32_t gs_lsb_narrow_tile(int key_type, int val_bytes)
{
    if (n_key_bytes(key_type) == 0 || !n_val_ok(val_bytes)) return 0;
    return (uint32_t)narrow_tile(val_bytes);
}

size_t gs_lsb_narrow_temp_bytes(uint64_t num_items, int key_type, int val_bytes)
{
    const int kb = n_key_bytes(key_type);
    if (kb == 0 || !n_val_ok(val_bytes) || num_items >= (1ull << 32)) return 0;
    size_t b = n_spine_bytes(num_items, val_bytes) + n_totals_bytes() + GS_WS_SLACK;
    if (kb == 2) b += n_align256((size_t)num_items * 2) + n_align256((size_t)num_items * (size_t)val_bytes);
    return b;
}

int gs_lsb_sort_narrow(void *d_temp, size_t temp_bytes, const void *d_keys_in, void *d_keys_out, const void *d_vals_in,
                       void *d_vals_out, uint64_t num_items, int key_type, int val_bytes, int begin_bit, int end_bit,
                       int descending, void *stream)
{
    GS_CLEAR_STALE_ERROR();
    const int kb = n_key_bytes(key_type);
    if (kb == 0 || !n_val_ok(val_bytes)) return hipErrorInvalidValue;
    if (begin_bit < 0 || end_bit > 8 * kb || begin_bit > end_bit) return hipErrorInvalidValue;
    if (num_items >= (1ull << 32)) return hipErrorInvalidValue;
    if (num_items == 0) return hipSuccess;              // (empty arrays may come with null pointers)
    if ((val_bytes != 0) != (d_vals_in != nullptr) || (val_bytes != 0) != (d_vals_out != nullptr)) return hipErrorInvalidValue;
    if (!d_keys_in || !d_keys_out || d_keys_in == d_keys_out || (val_bytes && d_vals_in == d_vals_out)) return hipErrorInvalidValue;
    if (((uintptr_t)d_keys_in | (uintptr_t)d_keys_out) & (uintptr_t)(kb - 1)) return hipErrorInvalidValue;
    if (val_bytes && (((uintptr_t)d_vals_in | (uintptr_t)d_vals_out) & (uintptr_t)(val_bytes - 1))) return hipErrorInvalidValue;
    if (!d_temp || temp_bytes < gs_lsb_narrow_temp_bytes(num_items, key_type, val_bytes)) return hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = num_items;
    char *c = gs_ws_base(d_temp);   // spine, totals, then (16-bit keys) the intermediate keys and values
    uint32_t *spine = (uint32_t *)c;
    uint32_t *totals = (uint32_t *)(c + n_spine_bytes(n, val_bytes));
    const uint32_t sign = n_sign(key_type);
    const bool fk = n_float(key_type);

    if (begin_bit == end_bit) {
        hipLaunchKernelGGL(narrow_copy_kernel, n_stream_grid(n * kb, 256 * 16), dim3(256), 0, s, (const unsigned char *)d_keys_in,
                           (unsigned char *)d_keys_out, n * (uint64_t)kb);
        if (val_bytes)
            hipLaunchKernelGGL(narrow_copy_kernel, n_stream_grid(n * val_bytes, 256 * 16), dim3(256), 0, s,
                               (const unsigned char *)d_vals_in, (unsigned char *)d_vals_out, n * (uint64_t)val_bytes);
        return (int)hipGetLastError();
    }
    if (kb == 1 && val_bytes == 0 && begin_bit == 0 && end_bit == 8) {   // (b): count and fill
        hipError_t ze = zero_async(totals, RADIX * 4, s);
        if (ze != hipSuccess) return (int)ze;
        const dim3 g = n_count_grid(n);
        { KernelTimer kt(GS_K_LSB_UPSWEEP, s);
          hipLaunchKernelGGL(narrow_count8_kernel, g, dim3(NF_THREADS), 0, s, d_keys_in, totals, n); }
        { KernelTimer kt(GS_K_LSB_DOWNSWEEP, s);
          hipLaunchKernelGGL(narrow_fill8_kernel, g, dim3(NF_THREADS), 0, s, d_keys_out, (const uint32_t *)totals, n, sign, fk ? 0x7fu : 0u, descending ? 1 : 0); }
        return (int)hipGetLastError();
    }

    const int num_passes = (end_bit - begin_bit + RADIX_BITS - 1) / RADIX_BITS;   // 1 or 2
    void *tk = nullptr, *tv = nullptr;
    if (kb == 2) {
        tk = c + n_spine_bytes(n, val_bytes) + n_totals_bytes();
        tv = (char *)tk + n_align256((size_t)n * 2);
    }
    for (int pass = 0; pass < num_passes; ++pass) {
        NarrowParams p{};
        p.n = n; p.num_tiles = n_tiles(n, val_bytes);
        p.shift = (uint32_t)(begin_bit + pass * RADIX_BITS);
        const int bits = (end_bit - (int)p.shift < RADIX_BITS) ? end_bit - (int)p.shift : RADIX_BITS;
        p.mask = (1u << bits) - 1u;
        p.xr = sign ^ (descending ? 0xffffffffu : 0u);
        const bool first = pass == 0, last = pass == num_passes - 1;
        const void *kin = first ? d_keys_in : tk;
        const void *vin = first ? d_vals_in : tv;
        void *kout = last ? d_keys_out : tk;
        void *vout = last ? d_vals_out : tv;
        const int e = narrow_pass_dispatch(kb, val_bytes, fk, kin, kout, val_bytes ? vin : nullptr, val_bytes ? vout : nullptr, spine, totals, p, s);
        if (e) return e;
    }
    return hipSuccess;
}

}  // extern "C"
