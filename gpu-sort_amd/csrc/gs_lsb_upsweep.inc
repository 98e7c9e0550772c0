// gs_lsb_upsweep.inc -- the upsweep of an LSB pass (device code): included by gs_lsb.hip and by gs_lsb_plan.hip, whose pass
// slots are further instantiations of the same code.
// ---------------------------------------------------------------- upsweep --
#ifndef UPSWEEP_BATCH
#define UPSWEEP_BATCH 64   // dword loads in flight per lane (a tile is 128 per lane).  In-process A/B at 2^30 keys (round 3, tools/ab_inproc.py):
                           // 16 -> 0.751 ms, 32 -> 0.709-0.721, 64 -> 0.685-0.694, 128 -> 0.707 ms per launch (64: 150 VGPRs, one workgroup per CU)
#endif
#ifndef UPSWEEP_SUB
#define UPSWEEP_SUB 4      // histogram copies per wave (power of two)
#endif
// relaxed agent-scope accesses = `sc1` loads / write-through stores: what workgroups of one launch may exchange
// without fences (cdna_hip_programming.md Guideline 16, forms R1 / R2; compiler-visible, so hipcc counts their waits)
__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint64_t ld_agent(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// NEXT: the wave also counts the digit of the FOLLOWING pass (one plain histogram copy per wave) and the block adds
// its sums to `next_totals` -- the pipelined pass needs the digit totals before its first tile is scattered.
// PIPE: the block is one role of lsb_pipe_pass_kernel: key loads with the default cache policy (they must stay in the
// Infinity Cache for the downsweep role; the streaming hint would keep them out), results published write-through.
template <bool NEXT, bool PIPE>
struct UpsweepSmem {
    // every wave counts into UPSWEEP_SUB copies of its histogram (lane & 3 picks one; rows padded by one word so
    // equal digits of different copies sit in different banks): under skew the lanes that share a hot digit
    // spread over four banks instead of queueing on one (Zipf keys: 1.40 -> ~1.0 ms at level 1 of the MSB sort)
    uint32_t hist[LSB_WAVES][UPSWEEP_SUB][RADIX + 1];
    uint32_t hist2[NEXT ? LSB_WAVES : 1][NEXT ? RADIX : 1];
    alignas(8) uint16_t pre[PIPE ? LSB_WAVES : 1][PIPE ? RADIX : 4];   // prefix16 rows on their way to 8-byte stores
    alignas(8) uint32_t tot[PIPE ? RADIX : 2];
};

// Plain dword loads in batches beat 16-byte loads here (0.81 vs 0.84 ms at 2^30) and need no alignment.
// PLAIN: the keys need no transform on the way in (u32 ascending, and every pass after the first: keys travel
// twiddled between passes), so the full-tile path below is load, v_bfe, address, ds_add and nothing else.
template <bool NEXT, bool PIPE, bool PLAIN = false>
__device__ __forceinline__ void upsweep_chunk(UpsweepSmem<NEXT, PIPE> &sm, const uint32_t *__restrict__ keys, uint32_t chunk,
                                              uint32_t *__restrict__ spine, uint16_t *__restrict__ prefix16,
                                              uint32_t *__restrict__ cc, uint32_t *__restrict__ next_totals, const PassParams &p,
                                              const PipeParams &q)
{
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    uint32_t *my = sm.hist[w][lane & (UPSWEEP_SUB - 1)];
    for (int i = lane; i < UPSWEEP_SUB * (RADIX + 1); i += WAVE) (&sm.hist[w][0][0])[i] = 0;
    if (NEXT)
        for (int i = lane; i < RADIX; i += WAVE) sm.hist2[w][i] = 0;

    const uint32_t tile = chunk * LSB_CHUNK + (uint32_t)w;
    if (tile < p.num_tiles) {
        const uint64_t lo = (uint64_t)tile * LSB_TILE;
        const uint32_t len = (p.n - lo < (uint64_t)LSB_TILE) ? (uint32_t)(p.n - lo) : (uint32_t)LSB_TILE;
        const uint32_t *src = keys + lo;
        auto count = [&](uint32_t raw) {
            const uint32_t k = twiddle_in(raw, p.f32_in, p.xor_in);
            hist_add(my, __builtin_amdgcn_ubfe(k, p.shift, p.bits));        // wave-private ds_add_u32
            if (NEXT) hist_add(sm.hist2[w], __builtin_amdgcn_ubfe(k, q.next_shift, q.next_bits));
        };
        constexpr int GB = UPSWEEP_BATCH;
        if (!NEXT && !PIPE && len == (uint32_t)LSB_TILE) {
            // full tile (all but the array's last one): no clamps, no guards, and the test for a digit shared by the
            // whole wave (a hot bucket, constant high bytes: 64 lanes would queue on 4 counters) is made on two keys
            // of the batch instead of on each -- 15 -> 4 vector instructions per key
            uint32_t wbits = p.bits;
            asm volatile("" : "+v"(wbits));   // v_bfe_u32 takes one scalar operand (the shift)
            auto digit_of = [&](uint32_t raw) {
                return __builtin_amdgcn_ubfe(PLAIN ? raw : twiddle_in(raw, p.f32_in, p.xor_in), p.shift, wbits);
            };
#pragma unroll 1
            for (uint32_t j = 0; j < (uint32_t)LSB_TILE; j += GB * WAVE) {
                const uint32_t *at = src + j + lane;
                uint32_t v[GB];
#pragma unroll
                for (int u = 0; u < GB; ++u) v[u] = __builtin_nontemporal_load(at + u * WAVE);
                const uint32_t da = digit_of(v[0]), db = digit_of(v[GB / 2]);
                const bool hot = __builtin_amdgcn_ballot_w64(da == __builtin_amdgcn_readfirstlane(da)) == ~0ull ||
                                 __builtin_amdgcn_ballot_w64(db == __builtin_amdgcn_readfirstlane(db)) == ~0ull;
                if (hot) {
#pragma unroll
                    for (int u = 0; u < GB; ++u) hist_add(my, digit_of(v[u]));
                } else {
#pragma unroll
                    for (int u = 0; u < GB; ++u) atomicAdd(&my[digit_of(v[u])], 1u);
                }
            }
        } else {
        // batches of dword loads from clamped indices: one code path for partial and misaligned tiles
        // (a loop of one guarded load per trip would pay one HBM round trip per 64 keys)
        const uint32_t last = len - 1u;
#pragma unroll 1
        for (uint32_t j = 0; j < len; j += GB * WAVE) {
            uint32_t v[GB];
#pragma unroll
            for (int u = 0; u < GB; ++u) {
                const uint32_t idx = j + u * WAVE + lane;
                const uint32_t *at = &src[idx < last ? idx : last];
                v[u] = PIPE ? *at : __builtin_nontemporal_load(at);   // streaming hint: 0.80 -> 0.76 ms
            }
#pragma unroll
            for (int u = 0; u < GB; ++u)
                if (j + u * WAVE + lane < len) count(v[u]);
        }
        }
    }
    __syncthreads();
#if defined(GS_EXP_UPS) && GS_EXP_UPS == 4
    if (!PIPE && !NEXT && (chunk & 7u) != 0u) return;     // timing experiment: only one workgroup in eight writes its results
#endif
#if defined(GS_EXP_UPS) && GS_EXP_UPS >= 1 && GS_EXP_UPS <= 3
    // timing experiments only (results land in the wrong layout): 1 = the chunk's prefix16 rows as ONE 16-byte store per
    // digit thread (4 KiB per workgroup in four wave instructions instead of 32), 2 = also the spine as one 1 KiB row per
    // chunk, 3 = no result stores at all
    if (!PIPE && !NEXT && tid < RADIX) {
        uint32_t run = 0, pk[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < LSB_WAVES; ++j) {
            pk[j >> 1] |= (run & 0xffffu) << (16 * (j & 1));
            uint32_t c = 0;
#pragma unroll
            for (int u = 0; u < UPSWEEP_SUB; ++u) c += sm.hist[j][u][tid];
            run += c;
        }
#if GS_EXP_UPS < 3
        reinterpret_cast<uint4 *>(prefix16 + (size_t)chunk * LSB_CHUNK * RADIX)[tid] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
#if GS_EXP_UPS == 2
        spine[(size_t)chunk * RADIX + tid] = run;
#else
        spine[(uint32_t)tid * p.grid + chunk] = run;
#endif
#else
        if (run == 0xffffffffu) spine[0] = pk[0] + pk[1] + pk[2] + pk[3];
#endif
        return;
    }
#endif
    if (tid < RADIX) {
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < LSB_WAVES; ++j) {
            const uint32_t t = chunk * LSB_CHUNK + (uint32_t)j;
            if (PIPE) sm.pre[j][tid] = (uint16_t)run;
            else if (t < p.num_tiles) prefix16[(size_t)t * RADIX + tid] = (uint16_t)run;
            uint32_t c = 0;
#pragma unroll
            for (int u = 0; u < UPSWEEP_SUB; ++u) c += sm.hist[j][u][tid];
            run += c;
        }
        if (PIPE) sm.tot[tid] = run | (q.tag << 28);       // run <= 65536
        else spine[(uint32_t)tid * p.grid + chunk] = run;
        if (NEXT) {
            uint32_t s2 = 0;
#pragma unroll
            for (int j = 0; j < LSB_WAVES; ++j) s2 += sm.hist2[j][tid];
            if (s2) atomicAdd(&next_totals[tid], s2);
        }
    }
    if (PIPE) {
        // publish: the chunk's prefix16 rows (wave w = tile w, 8 bytes per lane), drained by every storing wave,
        // then -- behind the workgroup's barrier -- the tagged count words the scanner role polls
        __syncthreads();
        uint32_t tid2 = threadIdx.x;
        asm volatile("" : "+v"(tid2));   // recomputed from scratch: otherwise `tile` lives (and spills) across the counting loop
        const uint32_t tile2 = chunk * LSB_CHUNK + (tid2 >> 6);
        if (tile2 < p.num_tiles)
            st_agent(reinterpret_cast<uint64_t *>(prefix16 + (size_t)tile2 * RADIX) + lane,
                     reinterpret_cast<const uint64_t *>(sm.pre[tile2 - chunk * LSB_CHUNK])[lane]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid < RADIX / 2)
            st_agent(reinterpret_cast<uint64_t *>(cc + (size_t)chunk * RADIX) + tid, reinterpret_cast<const uint64_t *>(sm.tot)[tid]);
    }
}

#ifndef GS_EXP_UPS_WPE
#define GS_EXP_UPS_WPE 1
#endif
template <bool NEXT, bool PLAIN = false>
__global__ __launch_bounds__(LSB_THREADS, GS_EXP_UPS_WPE) void lsb_upsweep_kernel(const uint32_t *__restrict__ keys,
                                                                  uint32_t *__restrict__ spine,
                                                                  uint16_t *__restrict__ prefix16,
                                                                  uint32_t *__restrict__ next_totals, PassParams p, PipeParams q)
{
    // blocks are dispatched round-robin over the 8 XCDs; the blocks of one XCD take CONSECUTIVE chunks, so the 16 chunk
    // totals that share a 64-byte line of a spine row are merged in one L2 instead of leaving eight L2s as partial
    // lines (0.736 -> 0.708 ms per launch at 2^30 keys)
    __shared__ UpsweepSmem<NEXT, false> sm;
    upsweep_chunk<NEXT, false, PLAIN>(sm, keys, chunk_of_block(blockIdx.x, p.grid), spine, prefix16, nullptr, next_totals, p, q);
}
