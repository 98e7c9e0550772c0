// The tile body shared by narrow_downsweep_kernel and narrow_downsweep64_kernel in gs_narrow.hip.  It is a fragment rather
// than a device function so that the first kernel compiles to the code it had before the second one existed (as
// gs_wide_tile.inc).  The including kernel defines K, Off, OFF64, KPT, TILE, the LDS arrays whist / gbase / stage_raw and
// FK (n_digit's float term) and
// both of totals and dbase (the one it does not take as an argument is a null pointer that is never read).

    const int lane = lane_id(), w = wave_id();
    const uint32_t t = tile_of_item(blockIdx.x, p.num_tiles);   // XCD-contiguous slices: neighbouring runs meet in one L2
    const uint64_t tile_base = (uint64_t)t * TILE;
    const uint32_t valid = (p.n - tile_base < (uint64_t)TILE) ? (uint32_t)(p.n - tile_base) : (uint32_t)TILE;
    uint32_t *my = whist[w];
    const uint32_t wbase = (uint32_t)w * (WAVE * KPT) + lane;

    // the tile's keys: aligned chunks -> LDS
    const uint32_t ka = (uint32_t)((uintptr_t)keys_in & 15u);
    n_stage_in<TILE * KB / 16 + 1>(reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(keys_in) - ka) + tile_base * KB / 16,
                                   (ka + valid * KB + 15u) / 16u, stage_raw);

    // wave 0, lane l: global start of digits 4l..4l+3 for this tile
    Off g0[4] = {0, 0, 0, 0};
    if constexpr (OFF64) {
        if (w == 0) {
            const uint32_t *sp = spine + (size_t)(4 * lane) * p.num_tiles + t;
#pragma unroll
            for (int j = 0; j < 4; ++j) g0[j] = dbase[4 * lane + j] + sp[j * (size_t)p.num_tiles];
        }
    } else if (w == 0) {
        const uint4 tot = reinterpret_cast<const uint4 *>(totals)[lane];
        const uint32_t lane_sum = tot.x + tot.y + tot.z + tot.w;
        const uint32_t ex = wave_inclusive_scan(lane_sum) - lane_sum;
        const uint32_t *sp = spine + (size_t)(4 * lane) * p.num_tiles + t;
        g0[0] = ex + sp[0];
        g0[1] = ex + tot.x + sp[p.num_tiles];
        g0[2] = ex + tot.x + tot.y + sp[2 * (size_t)p.num_tiles];
        g0[3] = ex + tot.x + tot.y + tot.z + sp[3 * (size_t)p.num_tiles];
    }
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    __syncthreads();

    uint32_t key[KPT];
    uint32_t pos[KPT];
    // digit p.mask, the largest: ranked last, behind every element of the tile (a float key's pad is the preimage of all ones:
    // a descending ~xr has the sign bit set, and the float term would flip its magnitude bits back to zero)
    const uint32_t pad = FK ? (~p.xr | (KB == 1 ? 0x7fu : 0x7fffu)) : ~p.xr;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t idx = wbase + i * WAVE;
        const uint32_t k = *reinterpret_cast<const K *>(stage_raw + ka + (idx < valid ? idx : 0u) * KB);
        key[i] = (idx < valid) ? k : pad;
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t d = n_digit<KB, FK>(key[i], p);
        uint32_t plo, phi;
        match_digit(d, plo, phi);
        const uint32_t lower = count_lower(plo, phi);
        pos[i] = my[d] + lower;
        if (lower == 0)
            __hip_atomic_fetch_add(&my[d], (uint32_t)(__popc(plo) + __popc(phi)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) asm volatile("" : "+v"(pos[i]));
    __syncthreads();                            // every key is in registers: the raw chunks may be overwritten
    if (w == 0) {
        uint32_t run[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < N_WAVES; ++j) {
            const uint4 x = reinterpret_cast<const uint4 *>(whist[j])[lane];
            run[0] += x.x; run[1] += x.y; run[2] += x.z; run[3] += x.w;
        }
        const uint32_t lane_sum = run[0] + run[1] + run[2] + run[3];
        uint4 e4;
        e4.x = wave_inclusive_scan(lane_sum) - lane_sum;
        e4.y = e4.x + run[0];
        e4.z = e4.y + run[1];
        e4.w = e4.z + run[2];
        if constexpr (OFF64) {
            gbase[4 * lane] = g0[0] - e4.x; gbase[4 * lane + 1] = g0[1] - e4.y;
            gbase[4 * lane + 2] = g0[2] - e4.z; gbase[4 * lane + 3] = g0[3] - e4.w;
        } else {
            reinterpret_cast<uint4 *>(gbase)[lane] = make_uint4(g0[0] - e4.x, g0[1] - e4.y, g0[2] - e4.z, g0[3] - e4.w);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < N_WAVES; ++j) {
            const uint4 x = reinterpret_cast<const uint4 *>(whist[j])[lane];
            reinterpret_cast<uint4 *>(whist[j])[lane] = e4;
            e4.x += x.x; e4.y += x.y; e4.z += x.z; e4.w += x.w;
        }
    }
    __syncthreads();
    K *stage_k = reinterpret_cast<K *>(stage_raw);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        pos[i] += my[n_digit<KB, FK>(key[i], p)];
        stage_k[pos[i]] = (K)key[i];
    }
    __syncthreads();
    Off dst[KPT];
    K *kout = reinterpret_cast<K *>(keys_out);
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
        const uint32_t slot = (uint32_t)w * (WAVE * KPT) + i * WAVE + lane;   // wave-contiguous
        const K k = stage_k[slot];
        dst[i] = gbase[n_digit<KB, FK>(k, p)] + slot;
        if (slot < valid) kout[dst[i]] = k;
    }
    if constexpr (VB != 0) {
        typedef typename NElem<VB>::type V;
        V *stage_v = reinterpret_cast<V *>(stage_raw);
        V val[KPT];
        __syncthreads();                        // everyone is done reading the keys
        if constexpr (VB <= 2) {                // narrow values come the way the keys did
            const uint32_t va = (uint32_t)((uintptr_t)vals_in & 15u);
            n_stage_in<TILE * VB / 16 + 1>(reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(vals_in) - va) + tile_base * VB / 16,
                                           (va + valid * VB + 15u) / 16u, stage_raw);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t idx = wbase + i * WAVE;
                val[i] = *reinterpret_cast<const V *>(stage_raw + va + (idx < valid ? idx : 0u) * VB);
            }
            __syncthreads();
        } else {
            const V *vin = reinterpret_cast<const V *>(vals_in) + tile_base;
#pragma unroll
            for (int i = 0; i < KPT; ++i) {
                const uint32_t idx = wbase + i * WAVE;
                val[i] = vin[idx < valid ? idx : valid - 1u];
            }
        }
#pragma unroll
        for (int i = 0; i < KPT; ++i) stage_v[pos[i]] = val[i];
        __syncthreads();
        V *vout = reinterpret_cast<V *>(vals_out);
#pragma unroll
        for (int i = 0; i < KPT; ++i) {
            const uint32_t slot = (uint32_t)w * (WAVE * KPT) + i * WAVE + lane;
            if (slot < valid) vout[dst[i]] = stage_v[slot];
        }
    }
