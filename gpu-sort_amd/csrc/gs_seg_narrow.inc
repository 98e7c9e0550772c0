// gs_seg_narrow.inc -- cub::DeviceSegmentedRadixSort for 8- and 16-bit keys (gs_segmented_sort_narrow), included by gs_msb.hip
// inside namespace gs: the library is built without relocatable device code, and these kernels work on the MsbWs lists that
// seg_classify_kernel, msb_expand_kernel, msb_scan_kernel and msb_classify_kernel of that file produce.
// The structure is seg_wide_sort's with a kernel set for 1- and 2-byte keys (DESIGN.md 10e):
//   - segments of up to SN_CAP elements are stable local-sort tasks (classes of 2048 and 8192), the smallest ones go to the
//     one-wave lists when the values are absent or 4 bytes wide; larger segments are the buckets of level 1, partitioned once
//     per 8-bit digit from begin_bit up (at most twice);
//   - a tile is 512 threads x 16 elements (no or 4-byte values) or x 8 (8-byte values), the sizes of gs_narrow.hip's passes;
//   - keys come from HBM as aligned 16-byte chunks into LDS -- a tile or a segment may start at any element, so the chunks are
//     taken from the aligned address below its first byte, and only chunks that hold one of its bytes are read -- and each
//     lane takes its elements from there in wave-striped order (element i of lane l of wave w is w * 64 * KPT + i * 64 + l);
//   - keys stay in the caller's representation: the sign flip of the key's own width and the descending complement are one
//     xor on the way to the digit; the float categories (FK) add float_flip at the key's width in front of it.  A pad is the
//     preimage of the all-ones image, the largest digit in every pass, ranked last because it comes last: ~xr for the
//     integer types; for a float key ~xr with the magnitude bits set (0x7fff / 0x7f ascending, 0xffff / 0xff descending:
//     a descending ~xr alone, 0x8000, has the sign set and the image 0x8000);
//   - every store is one element wide and goes to a position inside the segment, so no byte outside a segment is written
//     and no dword is shared between two workgroups' stores.
constexpr int SN_THREADS = 512, SN_WAVES = SN_THREADS / WAVE;
constexpr uint32_t SN_CAP = 8192;                 // largest segment one workgroup sorts
constexpr int sn_kpt(int vb) { return vb == 8 ? 8 : 16; }
static_assert(SN_WAVES == MSB_WAVES, "the spine has one column per MSB_WAVES tiles");

template <int B> struct SnKey;
template <> struct SnKey<1> { typedef uint8_t type; };
template <> struct SnKey<2> { typedef uint16_t type; };

template <int KB, bool FK>
__device__ __forceinline__ uint32_t sn_digit(uint32_t k, uint32_t xr, uint32_t shift, uint32_t mask)
{
    return ((float_flip<FK ? 8 * KB : 0>(k) ^ xr) >> shift) & mask;
}
template <int KB, bool FK> __device__ __forceinline__ uint32_t sn_pad(uint32_t xr) { return FK ? (~xr | (KB == 1 ? 0x7fu : 0x7fffu)) : ~xr; }

// the aligned 16-byte chunks that hold elements [first, first + count) of `base` (count >= 1), copied to raw; returns the
// offset of element `first` in raw (< 16)
template <int KB, int MAX_CHUNKS>
__device__ __forceinline__ uint32_t sn_stage_in(const void *__restrict__ base, uint32_t first, uint32_t count, unsigned char *raw)
{
    const uintptr_t addr = (uintptr_t)base + (size_t)first * KB;
    const uint32_t a = (uint32_t)(addr & 15u);
    const uint4 *A = reinterpret_cast<const uint4 *>(addr - a);
    const uint32_t nch = (a + count * KB + 15u) / 16u;
    constexpr int IT = (MAX_CHUNKS + SN_THREADS - 1) / SN_THREADS;
    uint4 v[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t c = (uint32_t)threadIdx.x + it * SN_THREADS;
        v[it] = A[c < nch ? c : nch - 1u];          // unconditional loads from clamped chunks
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const uint32_t c = (uint32_t)threadIdx.x + it * SN_THREADS;
        if (c < nch && c < (uint32_t)MAX_CHUNKS) reinterpret_cast<uint4 *>(raw)[c] = v[it];
    }
    return a;
}

// digit counts of the level's tiles: one wave per tile, MSB_WAVES tiles per block and step (mw_upsweep_kernel's layout of
// the spine and the in-chunk prefixes), the keys read as aligned chunks (narrow_upsweep_kernel)
template <int KB, bool FK>
__global__ __launch_bounds__(SN_THREADS) void sn_upsweep_kernel(MsbWs ws, int L, const void *__restrict__ src, uint32_t shift,
                                                                uint32_t mask, uint32_t xr)
{
    __shared__ uint32_t lh[SN_WAVES][RADIX];
    uint32_t ntiles = (uint32_t)ws.level[L].packed;
    if (ntiles > ws.max_tiles - SN_WAVES) ntiles = ws.max_tiles - SN_WAVES;
    const uint32_t nchunks = ntiles / SN_WAVES + 1;
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    uint32_t *my = lh[w];
    constexpr int GB = 4;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
        const uint32_t g = c * SN_WAVES + (uint32_t)w;
        if (g < ntiles) {
            const MsbTile T = ws.tiles[g];
            const uintptr_t addr = (uintptr_t)src + (size_t)T.lo * KB;
            const uint32_t a = (uint32_t)(addr & 15u);
            const uint4 *A = reinterpret_cast<const uint4 *>(addr - a);
            const uint32_t end_byte = a + T.valid * KB;           // the tile's elements are bytes [a, end_byte) from A
            const uint32_t nch = T.valid ? (end_byte + 15u) / 16u : 0u;
#pragma unroll 1
            for (uint32_t j = 0; j < nch; j += GB * WAVE) {
                uint4 v[GB];
#pragma unroll
                for (int u = 0; u < GB; ++u) {
                    const uint32_t ch = j + u * WAVE + lane;
                    v[u] = A[ch < nch ? ch : nch - 1u];
                }
#pragma unroll
                for (int u = 0; u < GB; ++u) {
                    const uint32_t ch = j + u * WAVE + lane;
                    if (ch >= nch) continue;
                    const uint32_t b0 = ch * 16u;
                    const uint32_t x[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                    if (b0 >= a && b0 + 16u <= end_byte) {
#pragma unroll
                        for (int q = 0; q < 16 / KB; ++q) {
                            const uint32_t k = (x[q * KB / 4] >> (8 * (q * KB % 4))) & (KB == 1 ? 0xffu : 0xffffu);
                            hist_add(my, sn_digit<KB, FK>(k, xr, shift, mask));
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 16 / KB; ++q) {
                            const uint32_t k = (x[q * KB / 4] >> (8 * (q * KB % 4))) & (KB == 1 ? 0xffu : 0xffffu);
                            const uint32_t b = b0 + q * KB;
                            if (b >= a && b < end_byte) hist_add(my, sn_digit<KB, FK>(k, xr, shift, mask));
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (tid < RADIX) {
            uint32_t run = 0;
#pragma unroll
            for (int j = 0; j < SN_WAVES; ++j) {
                ws.prefix16[(size_t)(c * SN_WAVES + j) * RADIX + tid] = (uint16_t)run;
                run += lh[j][tid];
            }
            ws.spine[(size_t)tid * ws.stride + c] = run;
        }
        __syncthreads();
    }
}

// one level tile: stable counting-sort scatter on the digit at `shift` (mw_scatter_kernel's bases from cursors, spine and
// prefix16; narrow_downsweep_kernel's staging, ranking and per-element stores).  Pads rank last and are not stored.
template <int KB, typename V, bool FK>
__global__ __launch_bounds__(SN_THREADS) void sn_scatter_kernel(MsbWs ws, int L, const void *__restrict__ src_k, void *__restrict__ dst_k,
                                                                const V *__restrict__ src_v, V *__restrict__ dst_v, uint32_t shift,
                                                                uint32_t mask, uint32_t xr)
{
    typedef typename SnKey<KB>::type K;
    constexpr bool HAS_VALUES = !std::is_same<V, MwNoVal>::value;
    constexpr int VB = HAS_VALUES ? (int)sizeof(V) : 0, KPT = sn_kpt(VB), TILE = SN_THREADS * KPT, ELEM = KB > VB ? KB : VB;
    __shared__ __attribute__((aligned(16))) uint32_t whist[SN_WAVES][RADIX];
    __shared__ __attribute__((aligned(16))) uint32_t gbase[RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[TILE * ELEM + 16];   // (+ 16: the chunk a misaligned tile spills into)
    const uint32_t ntiles = (uint32_t)ws.level[L].packed;
    if (blockIdx.x >= ntiles || blockIdx.x >= ws.max_tiles) return;
    const uint32_t g = tile_of_item(blockIdx.x, ntiles);
    const MsbTile T = ws.tiles[g];
    const uint32_t valid = T.valid < (uint32_t)TILE ? T.valid : (uint32_t)TILE;
    if (valid == 0u) return;
    const int lane = lane_id(), w = wave_id();
    uint32_t *my = whist[w];
    const uint32_t wbase = (uint32_t)w * (WAVE * KPT) + lane;

    const uint32_t ka = sn_stage_in<KB, TILE * KB / 16 + 1>(src_k, T.lo, valid, stage_raw);
    uint32_t tbase[4] = {0, 0, 0, 0};
    if (w == 0) {
        const uint4 cur = reinterpret_cast<const uint4 *>(ws.cursors + (size_t)T.bucket * RADIX)[lane];
        const uint32_t *sp = ws.spine + g / SN_WAVES + (size_t)(4 * lane) * ws.stride;
        const uint2 pf = reinterpret_cast<const uint2 *>(ws.prefix16 + (size_t)g * RADIX)[lane];
        tbase[0] = cur.x + sp[0] + (pf.x & 0xffffu);
        tbase[1] = cur.y + sp[ws.stride] + (pf.x >> 16);
        tbase[2] = cur.z + sp[2 * (size_t)ws.stride] + (pf.y & 0xffffu);
        tbase[3] = cur.w + sp[3 * (size_t)ws.stride] + (pf.y >> 16);
    }
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    __syncthreads();

    uint32_t key[KPT], pos[KPT];
    const uint32_t pad = sn_pad<KB, FK>(xr);    // digit `mask`, the largest: ranked last, behind every element of the tile
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * WAVE;
        const uint32_t k = *reinterpret_cast<const K *>(stage_raw + ka + (idx < valid ? idx : 0u) * KB);
        key[i] = (idx < valid) ? k : pad;
    }
    mw_rank<KPT>(my, pos, [&](int i) { return sn_digit<KB, FK>(key[i], xr, shift, mask); });
    __syncthreads();                            // every key is in registers: the raw chunks may be overwritten
    if (w == 0) {
        uint32_t ex[4];
        mw_scan_rows<SN_WAVES>(whist, ex);
        reinterpret_cast<uint4 *>(gbase)[lane] = make_uint4(tbase[0] - ex[0], tbase[1] - ex[1], tbase[2] - ex[2], tbase[3] - ex[3]);
    }
    __syncthreads();
    K *stage_k = reinterpret_cast<K *>(stage_raw);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        pos[i] += my[sn_digit<KB, FK>(key[i], xr, shift, mask)];
        stage_k[pos[i]] = (K)key[i];
    }
    __syncthreads();
    uint32_t dst[KPT];
    K *kout = reinterpret_cast<K *>(dst_k);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t slot = wbase + i * WAVE;          // wave-contiguous slots
        const K k = stage_k[slot];
        dst[i] = gbase[sn_digit<KB, FK>(k, xr, shift, mask)] + slot;
        if (slot < valid) kout[dst[i]] = k;
    }
    if constexpr (HAS_VALUES) {
        V *stage_v = reinterpret_cast<V *>(stage_raw);
        V val[KPT];
        const V *pv = src_v + T.lo;
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = wbase + i * WAVE;
            val[i] = pv[idx < valid ? idx : valid - 1u];
        }
        __syncthreads();                        // everyone is done reading the keys
#pragma unroll
        for (int i = 0; i < KPT; ++i) stage_v[pos[i]] = val[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t slot = wbase + i * WAVE;
            if (slot < valid) dst_v[dst[i]] = stage_v[slot];
        }
    }
}

// local sort of one class: the segment is read once (keys as aligned chunks through LDS, values straight into registers),
// sorted by stable LSD passes of 8 bits over the task's `sort_bits` bits from bit `pad` (one pass for 8-bit keys, two for 16-bit
// keys, fewer for a narrower bit range), keys and values exchanged through one LDS buffer after every pass, and written once.
// Everything is in registers before the first store, so source and destination may be the same array.
template <int KB, typename V, int KPT, bool FK>
__global__ __launch_bounds__(SN_THREADS) void sn_local_sort_kernel(MsbWs ws, int L, int cls, const void *__restrict__ src_k,
                                                                   void *__restrict__ dst_k, const V *__restrict__ src_v,
                                                                   V *__restrict__ dst_v, uint32_t xr)
{
    typedef typename SnKey<KB>::type K;
    constexpr bool HAS_VALUES = !std::is_same<V, MwNoVal>::value;
    constexpr int VB = HAS_VALUES ? (int)sizeof(V) : 0, CAP = SN_THREADS * KPT, ELEM = KB > VB ? KB : VB;
    __shared__ __attribute__((aligned(16))) uint32_t whist[SN_WAVES][RADIX];
    __shared__ __attribute__((aligned(16))) unsigned char stage_raw[CAP * ELEM + 16];
    K *stage_k = reinterpret_cast<K *>(stage_raw);
    V *stage_v = reinterpret_cast<V *>(stage_raw);
    K *kout = reinterpret_cast<K *>(dst_k);
    uint32_t ntasks = ws.level[L].task_count[cls];
    if (ntasks > ws.max_tasks) ntasks = ws.max_tasks;
    const int lane = lane_id(), w = wave_id();
    uint32_t *my = whist[w];
    const uint32_t wbase = (uint32_t)w * (WAVE * KPT) + lane;
    const uint32_t pad = sn_pad<KB, FK>(xr);
    for (uint32_t t = blockIdx.x; t < ntasks; t += gridDim.x) {
        const MsbTask T = ws.tasks[cls][t];
        const uint32_t size = T.size < (uint32_t)CAP ? T.size : (uint32_t)CAP;
        if (size == 0u) continue;               // (uniform; never emitted)
        uint32_t key[KPT], pos[KPT];
        V val[HAS_VALUES ? KPT : 1];
        const uint32_t ka = sn_stage_in<KB, CAP * KB / 16 + 1>(src_k, T.offset, size, stage_raw);
        if constexpr (HAS_VALUES) {
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t idx = wbase + i * WAVE;
                val[i] = src_v[T.offset + (idx < size ? idx : size - 1u)];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = wbase + i * WAVE;
            const uint32_t k = *reinterpret_cast<const K *>(stage_raw + ka + (idx < size ? idx : 0u) * KB);
            key[i] = (idx < size) ? k : pad;
        }
        __syncthreads();                        // every key is in registers: the buffer takes the passes' exchanges
#pragma unroll 1
        for (uint32_t done = 0; done < T.sort_bits; done += 8) {
            const uint32_t shift = T.pad + done, dm = (T.sort_bits - done < 8u) ? ((1u << (T.sort_bits - done)) - 1u) : 0xffu;
#pragma unroll
            for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
            mw_rank<KPT>(my, pos, [&](int i) { return sn_digit<KB, FK>(key[i], xr, shift, dm); });
            __syncthreads();
            if (w == 0) { uint32_t ex[4]; mw_scan_rows<SN_WAVES>(whist, ex); }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                pos[i] += my[sn_digit<KB, FK>(key[i], xr, shift, dm)];
                stage_k[pos[i]] = (K)key[i];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) key[i] = stage_k[wbase + i * WAVE];
            if constexpr (HAS_VALUES) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < KPT; ++i) stage_v[pos[i]] = val[i];
                __syncthreads();
#pragma unroll
                for (int i = 0; i < KPT; ++i) val[i] = stage_v[wbase + i * WAVE];
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t idx = wbase + i * WAVE;
            if (idx < size) {
                kout[T.offset + idx] = (K)key[i];
                if constexpr (HAS_VALUES) dst_v[T.offset + idx] = val[i];
            }
        }
        __syncthreads();
    }
}

template <int KB, typename V, bool FK>
static int seg_narrow_sort(void *d_temp, void *d_keys[2], void *d_vals[2], int *selector, uint64_t num_items, uint32_t num_segments,
                           const int32_t *d_begin_offsets, const int32_t *d_end_offsets, int begin_bit, int end_bit, int descending,
                           uint32_t sign, hipStream_t s)
{
    typedef typename SnKey<KB>::type K;
    constexpr bool pairs = !std::is_same<V, MwNoVal>::value;
    constexpr int VB = pairs ? (int)sizeof(V) : 0, nclass = 2, TILE = SN_THREADS * sn_kpt(VB), FW = FK ? 8 * KB : 0;
    // the lists are carved for tiles of 4096 elements (tile_shift 12), which bounds the tiles of 8192 the narrower values use:
    // msb_carve derives the list capacities from the tile size, never from the tile_shift field, which only expand and
    // classify read on the device -- so the larger tile is set on the carved struct, and a carve that ever came back with
    // another geometry is refused instead of being patched
    static_assert(TILE == 4096 || TILE == 8192, "level tiles of 4096 or 8192 elements");
    MsbWs ws = msb_carve(d_temp, num_items, pairs, 0, num_segments, SN_CAP, (uint32_t)(8 * KB));
    if (ws.tile_shift != 12u || ws.max_tiles < num_items / 4096u + ws.max_buckets) return (int)hipErrorInvalidValue;
    ws.tile_shift = TILE == 8192 ? 13u : 12u;
    const int num_bits = end_bit - begin_bit, passes = (num_bits + RADIX_BITS - 1) / RADIX_BITS;   // 1 or 2
    const int sel = *selector, fin = sel ^ (passes & 1);
    const uint32_t xr = sign ^ (descending ? 0xffffffffu : 0u);
    const K *ksel = (const K *)d_keys[sel];
    K *kfin = (K *)d_keys[fin];
    hipError_t e = zero_async(ws.level, MSB_LEVELS * sizeof(MsbLevel), s);
    if (e != hipSuccess) return (int)e;
    { KernelTimer kt(GS_K_MSB_CLASSIFY, s);
      const uint32_t g = (num_segments + 1023u) / 1024u;
      hipLaunchKernelGGL(seg_classify_kernel, dim3(g < 4096u ? g : 4096u), dim3(256), 0, s, ws, d_begin_offsets, d_end_offsets,
                         num_segments, nclass, (uint32_t)num_bits, (uint32_t)begin_bit, (uint32_t)num_items,
                         VB == 8 ? 0u : SEG_TINY); }
    { KernelTimer kt(GS_K_MSB_LOCAL_SORT, s);
      if constexpr (VB != 8) {   // tiny segments: one wave each (the values are absent or u32)
          const uint32_t *vsel = pairs ? (const uint32_t *)d_vals[sel] : nullptr;
          uint32_t *vfin = pairs ? (uint32_t *)d_vals[fin] : nullptr;
          const uint32_t wg = (num_segments + 3u) / 4u, wg4 = (num_segments + 15u) / 16u;
          const dim3 grid(wg < MSB_MAX_GRID ? wg : MSB_MAX_GRID), grid4(wg4 < MSB_MAX_GRID ? wg4 : MSB_MAX_GRID);
          hipLaunchKernelGGL((seg_wave_sort_narrow_kernel<pairs, 4, K, FW>), grid, dim3(256), 0, s, ws, ksel, kfin, vsel, vfin, 0, xr, 0, xr);
          hipLaunchKernelGGL((seg_wave_sort_narrow_kernel<pairs, 8, K, FW>), grid, dim3(256), 0, s, ws, ksel, kfin, vsel, vfin, 0, xr, 0, xr);
          hipLaunchKernelGGL((seg_wave_sort_narrow_kernel<pairs, 16, K, FW>), grid, dim3(256), 0, s, ws, ksel, kfin, vsel, vfin, 0, xr, 0, xr);
          hipLaunchKernelGGL((seg_wave4_sort_narrow_kernel<pairs, K, FW>), grid4, dim3(256), 0, s, ws, ksel, kfin, vsel, vfin, 0, xr, 0, xr);
      }
      const uint32_t g = ws.max_tasks < MSB_MAX_GRID ? ws.max_tasks : MSB_MAX_GRID;
      const V *vsel = pairs ? (const V *)d_vals[sel] : nullptr;
      V *vfin = pairs ? (V *)d_vals[fin] : nullptr;
      hipLaunchKernelGGL((sn_local_sort_kernel<KB, V, 4, FK>), dim3(g), dim3(SN_THREADS), 0, s, ws, 1, 0, (const void *)ksel, (void *)kfin, vsel, vfin, xr);
      hipLaunchKernelGGL((sn_local_sort_kernel<KB, V, 16, FK>), dim3(g), dim3(SN_THREADS), 0, s, ws, 1, 1, (const void *)ksel, (void *)kfin, vsel, vfin, xr); }
    // large segments: `passes` stable partitions of the same bucket list, 8 bits at a time from begin_bit
    const uint32_t max_b = ws.max_buckets;
    const uint32_t tiles_ub = (uint32_t)(num_items / TILE) + max_b;
    { KernelTimer kt(GS_K_MSB_HISTOGRAM, s);
      hipLaunchKernelGGL(msb_expand_kernel, dim3(max_b < 4096u ? max_b : 4096u), dim3(256), 0, s, ws, 1, (const uint32_t *)nullptr); }
    for (int p = 0; p < passes; ++p) {
        const uint32_t shift = (uint32_t)(begin_bit + p * RADIX_BITS);
        const int bits = (end_bit - (int)shift < RADIX_BITS) ? end_bit - (int)shift : RADIX_BITS;
        const uint32_t mask = (1u << bits) - 1u;
        const void *sk = d_keys[sel ^ (p & 1)];
        void *dk = d_keys[sel ^ ((p + 1) & 1)];
        const V *sv = pairs ? (const V *)d_vals[sel ^ (p & 1)] : nullptr;
        V *dv = pairs ? (V *)d_vals[sel ^ ((p + 1) & 1)] : nullptr;
        { KernelTimer kt(GS_K_MSB_HISTOGRAM, s);
          const uint32_t hg_ub = tiles_ub / SN_WAVES + 1;
          hipLaunchKernelGGL((sn_upsweep_kernel<KB, FK>), dim3(hg_ub < MSB_MAX_GRID ? hg_ub : MSB_MAX_GRID), dim3(SN_THREADS), 0, s, ws, 1, sk,
                             shift, mask, xr);
          hipLaunchKernelGGL(msb_scan_kernel, dim3(RADIX), dim3(1024), 0, s, ws, 1); }
        { KernelTimer kt(GS_K_MSB_CLASSIFY, s);
          hipLaunchKernelGGL((msb_classify_kernel<true, false>), dim3(max_b < 4096u ? max_b : 4096u), dim3(256), 0, s, ws, 1,
                             (const uint32_t *)nullptr, nclass); }
        { KernelTimer kt(GS_K_MSB_PARTITION, s);
          hipLaunchKernelGGL((sn_scatter_kernel<KB, V, FK>), dim3(tiles_ub), dim3(SN_THREADS), 0, s, ws, 1, sk, dk, sv, dv, shift, mask, xr); }
    }
    *selector = fin;
    return (int)hipGetLastError();
}
