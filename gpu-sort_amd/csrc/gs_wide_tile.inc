// gs_wide_tile.inc -- the body of the wide downsweep (one tile of 4096 elements), included by wide_downsweep_kernel and
// wide_downsweep64_kernel in gs_wide.hip.  It is a fragment rather than a device function so that the first kernel compiles
// to exactly the code it had before the second one existed: an inlined function is simplified twice, which reorders some
// of its arithmetic.
// The including kernel declares: K, V (template parameters), HAS_VALUES, OFF64, Off (the type of a global offset: u32, or
// u64 when OFF64), the LDS arrays whist[W_WAVES][RADIX], gbase[RADIX] (of Off) and stage_raw, and the pointers keys_in,
// keys_out, vals_in, vals_out, spine, prefix16, totals (read unless OFF64) and dbase (read when OFF64), and p.
// OFF64: the tile belongs to one slice (< 2^31 elements) of the 64-bit pass (gs_large.hip): the spine and prefix16 are the
// slice's own, dbase[d] is the absolute u64 start of the slice's run of digit d in the output, so a digit's global base is
// a u64 and the stores index with 64 bits.
    K *stage_k = reinterpret_cast<K *>(stage_raw);

    const int lane = lane_id(), w = wave_id();
    const uint32_t t = tile_of_item(blockIdx.x, p.num_tiles);   // XCD-contiguous slices: neighbouring runs meet in one L2
    const uint64_t tile_base = (uint64_t)t * W_TILE;
    const uint32_t valid = (p.n - tile_base < (uint64_t)W_TILE) ? (uint32_t)(p.n - tile_base) : (uint32_t)W_TILE;
    uint32_t *my = whist[w];
    const uint32_t wbase = (uint32_t)w * (WAVE * W_KPT) + lane;

    // wave 0, lane l: global start of digits 4l..4l+3 and this tile's offset inside them
    Off g0[4] = {0, 0, 0, 0};
    if constexpr (OFF64) {
        if (w == 0) {
            const uint32_t *sp = spine + (uint32_t)(4 * lane) * p.grid + t / W_CHUNK;
            const uint2 pf = reinterpret_cast<const uint2 *>(prefix16 + (size_t)t * RADIX)[lane];
            const ulonglong2 d01 = reinterpret_cast<const ulonglong2 *>(dbase)[2 * lane];
            const ulonglong2 d23 = reinterpret_cast<const ulonglong2 *>(dbase)[2 * lane + 1];
            g0[0] = d01.x + (sp[0] + (pf.x & 0xffffu));
            g0[1] = d01.y + (sp[p.grid] + (pf.x >> 16));
            g0[2] = d23.x + (sp[2 * p.grid] + (pf.y & 0xffffu));
            g0[3] = d23.y + (sp[3 * p.grid] + (pf.y >> 16));
        }
    } else if (w == 0) {
        const uint4 tot = reinterpret_cast<const uint4 *>(totals)[lane];
        const uint32_t lane_sum = tot.x + tot.y + tot.z + tot.w;
        const uint32_t ex = wave_inclusive_scan(lane_sum) - lane_sum;
        const uint32_t *sp = spine + (uint32_t)(4 * lane) * p.grid + t / W_CHUNK;
        const uint2 pf = reinterpret_cast<const uint2 *>(prefix16 + (size_t)t * RADIX)[lane];
        g0[0] = ex + sp[0] + (pf.x & 0xffffu);
        g0[1] = ex + tot.x + sp[p.grid] + (pf.x >> 16);
        g0[2] = ex + tot.x + tot.y + sp[2 * p.grid] + (pf.y & 0xffffu);
        g0[3] = ex + tot.x + tot.y + tot.z + sp[3 * p.grid] + (pf.y >> 16);
    }

    K key[W_KPT];
    uint32_t pos[W_KPT];
    const K pad = (K)~(K)0;                     // twiddled all-ones: largest digit, ranked last
    // unconditional loads from clamped indices (predicated loads are issued one round trip at a time)
    const K *kin = keys_in + tile_base;
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) {
        const uint32_t idx = wbase + i * WAVE;
        key[i] = kin[idx < valid ? idx : valid - 1u];
    }
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) {
        const uint32_t idx = wbase + i * WAVE;
        const K k = w_twiddle_in<K>(key[i], p.f_in, p.xor_in);
        key[i] = (idx < valid) ? k : pad;
    }
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) {
        const uint32_t d = w_digit(key[i], p);
        uint32_t plo, phi;
        match_digit(d, plo, phi);
        const uint32_t lower = count_lower(plo, phi);
        pos[i] = my[d] + lower;
        if (lower == 0)
            __hip_atomic_fetch_add(&my[d], (uint32_t)(__popc(plo) + __popc(phi)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) asm volatile("" : "+v"(pos[i]));
    __syncthreads();
    if (w == 0) {
        uint32_t run[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < W_WAVES; ++j) {
            const uint4 x = reinterpret_cast<const uint4 *>(whist[j])[lane];
            run[0] += x.x; run[1] += x.y; run[2] += x.z; run[3] += x.w;
        }
        const uint32_t lane_sum = run[0] + run[1] + run[2] + run[3];
        uint4 e4;
        e4.x = wave_inclusive_scan(lane_sum) - lane_sum;
        e4.y = e4.x + run[0];
        e4.z = e4.y + run[1];
        e4.w = e4.z + run[2];
        if constexpr (OFF64) {   // (mod 2^64; exact once the slot is added)
            reinterpret_cast<ulonglong2 *>(gbase)[2 * lane] = make_ulonglong2(g0[0] - e4.x, g0[1] - e4.y);
            reinterpret_cast<ulonglong2 *>(gbase)[2 * lane + 1] = make_ulonglong2(g0[2] - e4.z, g0[3] - e4.w);
        } else {
            reinterpret_cast<uint4 *>(gbase)[lane] = make_uint4(g0[0] - e4.x, g0[1] - e4.y, g0[2] - e4.z, g0[3] - e4.w);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < W_WAVES; ++j) {
            const uint4 x = reinterpret_cast<const uint4 *>(whist[j])[lane];
            reinterpret_cast<uint4 *>(whist[j])[lane] = e4;
            e4.x += x.x; e4.y += x.y; e4.z += x.z; e4.w += x.w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) {
        pos[i] += my[w_digit(key[i], p)];
        stage_k[pos[i]] = key[i];
    }
    __syncthreads();
    Off dst[W_KPT];
#pragma unroll
    for (int i = 0; i < W_KPT; ++i) {
        const uint32_t slot = (uint32_t)w * (WAVE * W_KPT) + i * WAVE + lane;   // wave-contiguous (see lsb_downsweep_kernel)
        const K k = stage_k[slot];
        dst[i] = gbase[w_digit(k, p)] + slot;
        if (slot < valid) keys_out[dst[i]] = w_twiddle_out<K>(k, p.f_out, p.xor_out);
    }
    if constexpr (HAS_VALUES) {
        V *stage_v = reinterpret_cast<V *>(stage_raw);
        V val[W_KPT];
        const V *vin = vals_in + tile_base;
#pragma unroll
        for (int i = 0; i < W_KPT; ++i) {
            const uint32_t idx = wbase + i * WAVE;
            val[i] = vin[idx < valid ? idx : valid - 1u];
        }
        __syncthreads();                       // everyone is done reading the keys
#pragma unroll
        for (int i = 0; i < W_KPT; ++i) stage_v[pos[i]] = val[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < W_KPT; ++i) {
            const uint32_t slot = (uint32_t)w * (WAVE * W_KPT) + i * WAVE + lane;
            if (slot < valid) vals_out[dst[i]] = stage_v[slot];
        }
    }
