// gs_lsb_downsweep.inc -- one tile of the downsweep of an LSB pass (device code): included by gs_lsb.hip and by
// gs_lsb_plan.hip, whose pass slots are further instantiations of the same code.
#ifndef GS_EXP_SLEEP_MODE
#define GS_EXP_SLEEP_MODE 0
#endif
#ifndef GS_EXP_SLEEP_MIN_TILES
#define GS_EXP_SLEEP_MIN_TILES 49152u
#endif
#ifndef GS_EXP_SLEEP_PAIRS
#define GS_EXP_SLEEP_PAIRS 0
#endif
// -------------------------------------------------------------- downsweep --
// Stable scatter, one tile at a time:
//   1. wave-striped coalesced load (key i of lane l of wave w sits at
//      tile + w*1024 + i*64 + l, so position order = (w, i, l)); HBM latency
//      is covered by the other blocks resident on the CU;
//   2. rank inside the wave: the set of lanes holding the same digit (ballot
//      match) gives the rank inside the group by popcount of the lower lanes;
//      the wave's running count of the digit (wave-private LDS histogram) gives
//      the rank of the group.  Every lane reads the count, the first lane of the
//      group then adds the group size with a no-return LDS atomic; LDS executes
//      one wave's operations in order, so round i+1 sees round i's add without a
//      wait.  The match set comes either from 8 VALU ballots (match_digit) or
//      from LDS: each lane ORs its lane bit into the wave's mask entry of its
//      digit, reads the entry back and clears its bit again.  Both are exact;
//      `valu_rounds` splits the 16 rounds between the two pipes;
//   3. the 8 wave histograms become tile-absolute bases per (wave, digit) (4 digits
//      per lane, b128 LDS accesses, DPP scan), by wave 0 alone (keys only, 3
//      blocks/CU) or redundantly by every wave for its own row, which removes a
//      barrier and the serial section (pairs, 2 blocks/CU); wave 0 publishes, per
//      digit, the tile's global base = digit start + scanned chunk count + prefix16;
//   4. keys (and values) go to LDS at their tile rank and are read back in rank
//      order: consecutive lanes hit consecutive addresses inside a digit run.
// Two (pairs) or three (keys only) block barriers per tile.
// OFF64: the 64-bit pass (lsb_downsweep64): gbase holds absolute u64 element offsets instead of u32 ones.
template <bool HAS_VALUES, bool OFF64 = false>
struct DownsweepSmem {
    uint32_t whist[LSB_WAVES][RADIX];                     // wave-private digit counters, then bases (byte offsets)
#ifdef GS_EXP_ALLWAVE_KEYS
    uint16_t wbase[LSB_WAVES][RADIX];
#else
    uint16_t wbase[HAS_VALUES ? LSB_WAVES : 1][RADIX];    // pairs: tile-absolute base of (wave, digit), < 8192
#endif
    std::conditional_t<OFF64, uint64_t, uint32_t> gbase[RADIX];   // global offset of digit run - tile-local start
    uint32_t stage[LSB_TILE * (HAS_VALUES ? 2 : 1)];      // tile in rank order; pairs interleaved {key,val}
    uint32_t dead;                                        // pipelined pass only: wave 0's wait gave up -> the tile stores nothing
};

#ifdef GS_EXP_PHASES
// experiment builds only (tools/phase_exp.py): shader-clock length of every phase of wave 0
__device__ uint32_t gs_phase_buf[131072 * 16];   // [block][phase], n <= 2^30
#define GS_PHASE(k)                                                                          \
    do {                                                                                     \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                        \
        if (tid == 0 && t < 131072u) gs_phase_buf[t * 16 + (k)] = (uint32_t)(now_ - tprev_); \
        tprev_ = now_;                                                                       \
    } while (0)
#define GS_PHASE_WAIT(what) asm volatile("s_waitcnt " what ::: "memory")
#else
#define GS_PHASE(k) do { } while (0)
#define GS_PHASE_WAIT(what) do { } while (0)
#endif

// The kernel is VALU-bound on MI355X (about 900 vector instructions per wave and tile, 57 % of
// them the ballot match; measured with tools/phase_exp.py and an ISA count), so the template
// parameters exist to keep instructions out of the hot variants:
// TAIL = false: one of the array's FULL tiles.
// TAIL = true: one block handles the last, partial tile (guarded loads); being
// last in key order, its keys of digit d sit at the very end of digit d's global
// range, so it needs only the digit totals.  Splitting it off keeps the guarded
// path's registers out of the hot kernel.
// TW: key transform on read / write.  0 = none (u32 ascending, and every middle pass: keys
// travel twiddled between passes), 1 = xor mask (signed keys, descending), 2 = float + xor.
// BIG = false: n <= 2^30, so byte offsets into the output fit 32 bits and a store needs no
// 64-bit address arithmetic.
// PIPE = true: the tile is one block of lsb_pipe_pass_kernel; its chunk's scanned counts come from the scanner
// role as {tag, value} granules (`sc`), its in-chunk prefixes from the upsweep role (`prefix16`), both published
// write-through inside the same launch and read here with agent-scope loads.
// OFF64 = true: the tile belongs to one slice (< 2^31 keys) of a larger array (lsb_downsweep64_kernel): the spine,
// prefix16 and totals are the slice's own, and dbase[d] is the absolute u64 output offset of the slice's run of digit
// d, so the global base of a digit run is dbase[d] + (signed 32-bit in-slice offset) and the stores index with 64 bits.
// CURSOR = true (gs_lsb_plan.hip, the second scatter of the PLANNED route): the order of the keys inside a digit run does not
// matter, so the tile takes no base from a spine: all its keys share the digit below the scatter's (the input is sorted on
// it), which selects one row of `cursor` ([lower digit][digit], initialised to the start of every (digit, lower digit)
// group), and wave 0 claims count(d) places for every digit d with one returning add per digit.  The adds are issued after
// barrier 1 and their returns are used just before barrier 3, behind the LDS scatter.  A tile whose first and last key
// differ in the lower digit stores nothing and appends its index to irr[1..] (count in irr[0]): another kernel places it.
// RANK_FREE = true (cursor mode only): step 2 ranks with one returning LDS add per key instead of the stable ballot match.
constexpr uint32_t PIPE_SPIN_LIMIT = 1u << 18;   // polls (each >= one memory round trip) before a wait gives up

template <bool HAS_VALUES, bool TAIL, int TW, bool BIG, bool PIPE, bool OFF64 = false, bool CURSOR = false, bool RANK_FREE = false>
__device__ __forceinline__ void downsweep_tile(DownsweepSmem<HAS_VALUES, OFF64> &sm, const uint32_t t,
    const uint32_t *__restrict__ keys_in, uint32_t *__restrict__ keys_out, const uint32_t *__restrict__ vals_in,
    uint32_t *__restrict__ vals_out, const uint32_t *__restrict__ spine, const uint16_t *__restrict__ prefix16,
    const uint32_t *__restrict__ totals, const PassParams &p, const uint64_t *__restrict__ sc, uint32_t tag,
    uint32_t *__restrict__ error_word, const uint32_t tid_ = threadIdx.x, const uint64_t *__restrict__ dbase = nullptr,
    uint32_t *__restrict__ cursor = nullptr, uint32_t *__restrict__ irr = nullptr, const uint32_t irr_cap = 0u)
{
    static_assert(!CURSOR || (!HAS_VALUES && !TAIL && !PIPE && !OFF64), "cursor mode: full tiles of keys-only three-launch passes");
#ifdef GS_EXP_ALLWAVE_KEYS
    constexpr bool ALLWAVE = true;          // experiment: every wave computes its own bases for keys too (no second barrier)
#else
    constexpr bool ALLWAVE = HAS_VALUES;   // see step 3
#endif

    [[maybe_unused]] const int tid = (int)tid_;
    const int lane = (int)(tid_ & 63u), w = (int)(tid_ >> 6);
    const uint32_t full_tiles = p.n / (uint32_t)LSB_TILE;
    auto tw_in = [&](uint32_t k) { return TW == 0 ? k : twiddle_in(k, TW == 2 ? p.f32_in : 0, p.xor_in); };
    auto tw_out = [&](uint32_t k) { return TW == 0 ? k : twiddle_out(k, TW == 2 ? p.f32_out : 0, p.xor_out); };
    // the digit width lives in a vector register: v_bfe_u32 takes one scalar operand (the shift)
    uint32_t wbits = p.bits;
    asm volatile("" : "+v"(wbits));
    auto digit = [&](uint32_t k) { return __builtin_amdgcn_ubfe(k, p.shift, wbits); };

    uint32_t *my = sm.whist[w];
    const uint16_t *mybase = sm.wbase[w];
    const uint32_t wbase = (uint32_t)w * (WAVE * LSB_KPT) + lane;
    const uint32_t tail_valid = p.n - full_tiles * (uint32_t)LSB_TILE;   // used when TAIL
    (void)full_tiles;

#ifdef GS_EXP_PHASES
    unsigned long long tprev_ = __builtin_amdgcn_s_memtime();
    const unsigned long long t0_ = tprev_, r0_ = __builtin_amdgcn_s_memrealtime();
#endif
    // keys only: the waves that issue loads and stores get priority over the ones that rank, so the memory
    // pipes are fed as early as possible (1.87 -> 1.82 ms; with values it costs 7 %, so pairs keep the default)
#ifdef GS_EXP_SLEEP_START
    __builtin_amdgcn_s_sleep(GS_EXP_SLEEP_START);
#endif
    if (!HAS_VALUES) __builtin_amdgcn_s_setprio(3);
    const uint64_t tile_base = (uint64_t)t * LSB_TILE;
    const uint32_t valid = TAIL ? tail_valid : (uint32_t)LSB_TILE;

    // pipelined pass: the chunk's scanned counts are requested first, so they are back before the keys are
    uint64_t scg[4] = {0, 0, 0, 0};
    const uint64_t *scrow = nullptr;
    if (PIPE && w == 0) {
        scrow = sc + (size_t)(t / LSB_CHUNK) * RADIX + 4 * lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) scg[q] = ld_agent(scrow + q);
    }

    // 1. wave-striped coalesced load
    uint32_t key[LSB_KPT], val[HAS_VALUES ? LSB_KPT : 1], pos[LSB_KPT];
    {
        const uint32_t *kin = keys_in + tile_base;
        if (!TAIL) {
#pragma unroll
            for (int i = 0; i < LSB_KPT; ++i) key[i] = kin[wbase + i * WAVE];
        } else {
            // pad with keys whose twiddled form is all ones (largest digit; ranked after
            // every real key of that digit because they sit at the tail)
            const uint32_t pad = twiddle_out(0xffffffffu, TW == 2 ? p.f32_in : 0, TW ? p.xor_in : 0u);
#pragma unroll
            for (int i = 0; i < LSB_KPT; ++i) {
                const uint32_t idx = wbase + i * WAVE;
                key[i] = pad;
                if (idx < tail_valid) key[i] = kin[idx];
            }
        }
    }
    // cursor mode, wave 0: the tile's first and last key (two scalar loads, used only before barrier 1)
    [[maybe_unused]] uint32_t cur_lo = 0, cur_hi = 0, claim[4] = {0, 0, 0, 0};
    if constexpr (CURSOR) {
        if (w == 0) {
            cur_lo = (tw_in(keys_in[tile_base]) >> (p.shift - (uint32_t)RADIX_BITS)) & (uint32_t)(RADIX - 1);
            cur_hi = (tw_in(keys_in[tile_base + (LSB_TILE - 1)]) >> (p.shift - (uint32_t)RADIX_BITS)) & (uint32_t)(RADIX - 1);
        }
    }
    GS_PHASE(0);                                   // load issue
#ifndef GS_EXP_RANK_PRIO
#define GS_EXP_RANK_PRIO 0
#endif
    if (!HAS_VALUES) __builtin_amdgcn_s_setprio(GS_EXP_RANK_PRIO);
    if (HAS_VALUES) {
        const uint32_t *vin = vals_in + tile_base;
#pragma unroll
        for (int i = 0; i < LSB_KPT; ++i) {
            const uint32_t idx = wbase + i * WAVE;
            val[i] = 0;
            if (!TAIL || idx < valid) val[i] = vin[idx];
        }
    }
    // (after the key loads are in flight) wave 0, lane l: global start of digits 4l..4l+3 (exclusive scan of the totals)
    // (TAIL: inclusive scan; the tile's own counts are subtracted later)
    uint32_t dstart[4] = {0, 0, 0, 0};
    if constexpr (OFF64) {
        // digit starts are dbase[d] (added in publish_gbase); TAIL: the slice's run of d ends at dbase[d] + totals[d]
        if (TAIL && w == 0) {
            const uint4 tot = reinterpret_cast<const uint4 *>(totals)[lane];
            dstart[0] = tot.x; dstart[1] = tot.y; dstart[2] = tot.z; dstart[3] = tot.w;
        }
    } else if (!CURSOR && w == 0) {
        const uint4 tot = reinterpret_cast<const uint4 *>(totals)[lane];
        const uint32_t lane_sum = tot.x + tot.y + tot.z + tot.w;
        const uint32_t ex = wave_inclusive_scan(lane_sum) - lane_sum;
        dstart[0] = ex + (TAIL ? tot.x : 0u);
        dstart[1] = dstart[0] + (TAIL ? tot.y : tot.x);
        dstart[2] = dstart[1] + (TAIL ? tot.z : tot.y);
        dstart[3] = dstart[2] + (TAIL ? tot.w : tot.z);
    }

    // this tile's global offsets (wave 0): scanned chunk count + count of the chunk's earlier tiles
    uint32_t tbase[4] = {0, 0, 0, 0};
    if (!TAIL && !PIPE && !CURSOR && w == 0) {
        const uint32_t *sp = spine + (uint32_t)(4 * lane) * p.grid + t / LSB_CHUNK;
        const uint2 pf = reinterpret_cast<const uint2 *>(prefix16 + (size_t)t * RADIX)[lane];
        tbase[0] = sp[0] + (pf.x & 0xffffu);
        tbase[1] = sp[p.grid] + (pf.x >> 16);
        tbase[2] = sp[2 * p.grid] + (pf.y & 0xffffu);
        tbase[3] = sp[3 * p.grid] + (pf.y >> 16);
    }

    if (PIPE && !TAIL && w == 0) {
        // every granule carries this pass's tag once the scanner has written it (normally long ago: the upsweep
        // role runs PIPE_LEAD_CHUNKS ahead); only then may the prefix16 row be read (it was published before the
        // counts the scanner waited for).  Bounded: a wait that gives up flags the sort instead of hanging the GPU --
        // and the tile then stores NOTHING: its offsets would come from untagged words (stale values of another pass
        // can exceed n: an out-of-bounds scatter), so the whole workgroup leaves behind the first barrier.
        uint32_t spins = 0;
        bool gave_up = false;
        for (;;) {
            const bool ok = (uint32_t)(scg[0] >> 32) == tag && (uint32_t)(scg[1] >> 32) == tag &&
                            (uint32_t)(scg[2] >> 32) == tag && (uint32_t)(scg[3] >> 32) == tag;
            if (__builtin_amdgcn_ballot_w64(!ok) == 0) break;
            if (++spins > PIPE_SPIN_LIMIT) {
                if (lane == 0) atomicOr(error_word, 1u);
                gave_up = true;
                break;
            }
            __builtin_amdgcn_s_sleep(8);
#pragma unroll
            for (int q = 0; q < 4; ++q) scg[q] = ld_agent(scrow + q);
        }
        if (lane == 0) sm.dead = gave_up ? 1u : 0u;
        const uint64_t pf = ld_agent(reinterpret_cast<const uint64_t *>(prefix16 + (size_t)t * RADIX) + lane);
        tbase[0] = (uint32_t)scg[0] + (uint32_t)(pf & 0xffffu);
        tbase[1] = (uint32_t)scg[1] + (uint32_t)((pf >> 16) & 0xffffu);
        tbase[2] = (uint32_t)scg[2] + (uint32_t)((pf >> 32) & 0xffffu);
        tbase[3] = (uint32_t)scg[3] + (uint32_t)(pf >> 48);
    }

    // global base of digit run = digit start + tile offset - tile-local start (wave 0, lane l: digits 4l..4l+3)
    auto publish_gbase = [&](const uint32_t (&ex)[4], const uint32_t (&run)[4]) {
        uint32_t g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) g[q] = dstart[q] + tbase[q] - ex[q];
        if (TAIL) {   // keys of digit d end exactly at the inclusive total of d
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] -= run[q];
            // padded keys inflate the count of the largest digit only, and they are never stored
            const uint32_t pads = (uint32_t)LSB_TILE - valid, dmax = p.mask;
            if (lane == (int)(dmax >> 2)) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((dmax & 3u) == (uint32_t)q) g[q] += pads;
            }
        }
        if constexpr (OFF64) {   // in-slice offsets are in (-2^13, 2^31): signed 32-bit
#pragma unroll
            for (int q = 0; q < 4; ++q) sm.gbase[4 * lane + q] = dbase[4 * lane + q] + (uint64_t)(int64_t)(int32_t)g[q];
        } else {
            if (!BIG) {   // byte offsets (mod 2^32; exact once the slot is added)
#pragma unroll
                for (int q = 0; q < 4; ++q) g[q] <<= 2;
            }
            reinterpret_cast<uint4 *>(sm.gbase)[lane] = make_uint4(g[0], g[1], g[2], g[3]);
        }
    };

    // 2. rank inside the wave (the LDS count of round i is consumed one round later, so
    //    its latency hides behind the match of round i+1)
#pragma unroll
    for (int i = lane; i < RADIX; i += WAVE) my[i] = 0;
    GS_PHASE_WAIT("vmcnt(0)");
    GS_PHASE(1);                                   // load wait
#pragma unroll
    for (int i = 0; i < LSB_KPT; ++i) key[i] = tw_in(key[i]);
    if constexpr (RANK_FREE) {
        // cursor mode, where the finish sorts every group: any order inside a digit run will do, so a key's rank is what one returning
        // add on the wave's own counter gives -- no 32-instruction ballot match per key, which is what makes this kernel VALU-bound
        // (gs_lsb_plan.hip, GS_PLAN_RANK_FREE; DESIGN.md section 3 has the measurement)
        static_assert(!RANK_FREE || CURSOR, "only the cursor scatter is free to rank in any order");
#pragma unroll
        for (int i = 0; i < LSB_KPT; ++i) pos[i] = __hip_atomic_fetch_add(&my[digit(key[i])], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    } else {
        uint32_t d_prev = 0, plo = 0, phi = 0;
#pragma unroll
        for (int i = 0; i <= LSB_KPT; ++i) {
            uint32_t d_cur = 0, clo = 0, chi = 0;
            if (i < LSB_KPT) {
                d_cur = digit(key[i]);
                match_digit(d_cur, clo, chi);
            }
            if (i > 0) {
                const uint32_t lower = count_lower(plo, phi);
                pos[i - 1] = my[d_prev] + lower;            // LDS read, all lanes
                if (lower == 0)                             // first lane of the group adds the group size
                    __hip_atomic_fetch_add(&my[d_prev], (uint32_t)(__popc(plo) + __popc(phi)), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WAVEFRONT);
            }
            d_prev = d_cur; plo = clo; phi = chi;
        }
    }
#pragma unroll
    for (int i = 0; i < LSB_KPT; ++i) {
        // finish the adds before the barrier, and make the keys opaque so their LDS
        // histogram addresses are recomputed after the barrier instead of kept live
        asm volatile("" : "+v"(pos[i]), "+v"(key[i]));
    }
    if constexpr (CURSOR) {
        if (w == 0 && lane == 0) {
            const bool straddles = cur_lo != cur_hi;
            sm.dead = straddles ? 1u : 0u;
            if (straddles) {
                const uint32_t at = atomicAdd(&irr[0], 1u);
                if (at < irr_cap) irr[1u + at] = t;
            }
        }
    }
    GS_PHASE_WAIT("lgkmcnt(0)");
    GS_PHASE(2);                                   // rank
    __syncthreads();
    GS_PHASE(3);                                   // barrier 1
    if (PIPE && !TAIL && sm.dead) return;          // the wait for this tile's offsets gave up: no global store (all waves alike)
    if (CURSOR && sm.dead) return;                 // the tile straddles two rows of the cursors: listed, placed later

    // 3. wave histograms -> tile-absolute base of every (wave, digit) + global base per digit.
    //    4 digits per lane, b128 LDS accesses, DPP scan of the 256 digit totals.
    if constexpr (ALLWAVE) {
        // every wave sums the 8 rows and keeps only its own row's bases (own row of `wbase`), so
        // there is no serial section and no second barrier: best at 2 blocks/CU (pairs)
        uint32_t run[4] = {0, 0, 0, 0}, below[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < LSB_WAVES; ++j) {
            const uint4 x = reinterpret_cast<const uint4 *>(sm.whist[j])[lane];
            run[0] += x.x; run[1] += x.y; run[2] += x.z; run[3] += x.w;
            if (j < w) { below[0] += x.x; below[1] += x.y; below[2] += x.z; below[3] += x.w; }
        }
        const uint32_t lane_sum = run[0] + run[1] + run[2] + run[3];
        uint32_t ex[4];
        ex[0] = wave_inclusive_scan(lane_sum) - lane_sum;
        ex[1] = ex[0] + run[0];
        ex[2] = ex[1] + run[1];
        ex[3] = ex[2] + run[2];
        reinterpret_cast<uint2 *>(sm.wbase[w])[lane] =
            make_uint2((ex[0] + below[0]) | ((ex[1] + below[1]) << 16), (ex[2] + below[2]) | ((ex[3] + below[3]) << 16));
        if (w == 0) publish_gbase(ex, run);
    } else {
        // wave 0 alone, two sweeps over the 8 rows (only one row in registers at a time), bases
        // written back in place as BYTE offsets into `stage`; the other waves wait at the barrier
        // while the CU's other two blocks run: best at 3 blocks/CU (keys only)
        if (w == 0) {
            uint32_t run[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < LSB_WAVES; ++j) {
                const uint4 x = reinterpret_cast<const uint4 *>(sm.whist[j])[lane];
                run[0] += x.x; run[1] += x.y; run[2] += x.z; run[3] += x.w;
            }
            const uint32_t lane_sum = run[0] + run[1] + run[2] + run[3];
            uint32_t ex[4];
            ex[0] = wave_inclusive_scan(lane_sum) - lane_sum;
            ex[1] = ex[0] + run[0];
            ex[2] = ex[1] + run[1];
            ex[3] = ex[2] + run[2];
            if constexpr (CURSOR) {
                // the tile-local starts go to `gbase` for now; lane l claims for digits l, 64 + l, 128 + l, 192 + l, so that
                // each of the four adds covers 256 contiguous bytes of the row (LDS serves one wave's accesses in order)
                reinterpret_cast<uint4 *>(sm.gbase)[lane] = make_uint4(ex[0], ex[1], ex[2], ex[3]);
                uint32_t *row = cursor + (size_t)__builtin_amdgcn_readfirstlane(cur_lo) * RADIX;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int d = q * WAVE + lane;
                    const uint32_t e0 = sm.gbase[d], e1 = sm.gbase[d == RADIX - 1 ? d : d + 1];
                    const uint32_t cnt = (d == RADIX - 1 ? (uint32_t)LSB_TILE : e1) - e0;
                    claim[q] = __hip_atomic_fetch_add(row + d, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            } else {
                publish_gbase(ex, run);
            }
            asm volatile("" ::: "memory");   // re-read the rows instead of keeping 32 registers live
            uint4 e4 = make_uint4(ex[0] << 2, ex[1] << 2, ex[2] << 2, ex[3] << 2);
#pragma unroll
            for (int j = 0; j < LSB_WAVES; ++j) {
                const uint4 x = reinterpret_cast<const uint4 *>(sm.whist[j])[lane];
                reinterpret_cast<uint4 *>(sm.whist[j])[lane] = e4;
                e4.x += x.x << 2; e4.y += x.y << 2; e4.z += x.z << 2; e4.w += x.w << 2;
            }
        }
        __syncthreads();
    }
    GS_PHASE(4);                                   // scan + barrier 2

    // 4. tile -> LDS in rank order -> global.  All 16 base reads are issued before the first
    //    write so the LDS round trip is paid once, not per key.
    {
        uint32_t wb[LSB_KPT];
#pragma unroll
        for (int i = 0; i < LSB_KPT; ++i) {
            const uint32_t d = digit(key[i]);
            wb[i] = ALLWAVE ? (uint32_t)mybase[d] : my[d];
        }
#pragma unroll
        for (int i = 0; i < LSB_KPT; ++i) {
            if (HAS_VALUES) {
                reinterpret_cast<uint2 *>(sm.stage)[pos[i] + wb[i]] = make_uint2(key[i], val[i]);
            } else if (ALLWAVE) {
                sm.stage[pos[i] + wb[i]] = key[i];
            } else {
                const uint32_t at = (pos[i] << 2) + wb[i];       // bytes
                *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(sm.stage) + at) = key[i];
            }
        }
    }
    if constexpr (CURSOR) {
        // the claims are back by now (or waited for here): global base of digit run = claimed place - tile-local start
        if (w == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = q * WAVE + lane;
                const uint32_t g = claim[q] - sm.gbase[d];
                sm.gbase[d] = BIG ? g : g << 2;
            }
        }
    }
    GS_PHASE_WAIT("lgkmcnt(0)");
    GS_PHASE(5);                                   // LDS scatter
    __syncthreads();
    GS_PHASE(6);                                   // barrier 3
    // Pacing (round 3, in-process A/B on the same buffers, tools/ab_inproc.py): every wave pauses 32 x 64 cycles (~0.9 us) between
    // barrier 3 and its 16 stores.  What it buys depends on where the driver placed the arrays: on placements where the kernel
    // runs 1.89-1.94 ms per launch without the pause it runs 1.78-1.79 ms with it; on placements where it runs 1.74 ms without,
    // the pause costs 0.7-1.5 % (1.755-1.77 ms) -- profiles/r03_ab_pacing.txt has both kinds, from the same box and process
    // sequence.  So the pause takes 8 % off the slow placements and the spread between placements shrinks from 11 % to 2 %.
    // Pauses of 8/16/24 recover less of the slow case (1.91/1.88/1.81 ms), 40-64 cost more of the fast one; pausing only the odd
    // waves (behind a scalar branch) 1.85 ms.  Only from 2^29 keys up: below, the launch is not bound by the memory system
    // and the pause is latency (2^28 keys: +1 %; 2^22-2^24: +5 %).  Pairs gain nothing from it (3.57-3.62 ms with 16/32, 3.71 with
    // 64, 3.58-3.60 without).  GS_EXP_SLEEP* override all of it for experiments.
#ifndef GS_EXP_SLEEP
#define GS_EXP_SLEEP 32
#define GS_EXP_SLEEP_MODE_DEFAULT 0
#else
#define GS_EXP_SLEEP_MODE_DEFAULT GS_EXP_SLEEP_MODE
#endif
    if ((!HAS_VALUES || GS_EXP_SLEEP_PAIRS) && full_tiles >= GS_EXP_SLEEP_MIN_TILES) {
        // s_sleep is a scalar instruction: it must sit behind a SCALAR branch (a branch on a vector condition only masks lanes
        // and the wave sleeps all the same), hence the readfirstlane
        [[maybe_unused]] const int ws = __builtin_amdgcn_readfirstlane(w);
#if GS_EXP_SLEEP_MODE_DEFAULT == 3
        if (ws & 1) __builtin_amdgcn_s_sleep(GS_EXP_SLEEP); else __builtin_amdgcn_s_sleep(GS_EXP_SLEEP_B);
#elif GS_EXP_SLEEP_MODE_DEFAULT == 4
        if (ws >= 4) __builtin_amdgcn_s_sleep(GS_EXP_SLEEP);
#elif GS_EXP_SLEEP_MODE_DEFAULT == 1
        if (ws & 1) __builtin_amdgcn_s_sleep(GS_EXP_SLEEP);
#elif GS_EXP_SLEEP_MODE_DEFAULT == 0
        __builtin_amdgcn_s_sleep(GS_EXP_SLEEP);
#endif
    }
#ifndef GS_EXP_STORE_PRIO
#define GS_EXP_STORE_PRIO 3
#endif
    if (!HAS_VALUES) __builtin_amdgcn_s_setprio(GS_EXP_STORE_PRIO);
#pragma unroll
    for (int i = 0; i < LSB_KPT; ++i) {
        // a wave stores 1024 CONSECUTIVE slots (not every 512th 64-slot group): its 16 store instructions walk ~32
        // neighbouring digit runs in order instead of touching ~48 runs all over the output -- keys 1.92 -> 1.81 ms,
        // pairs 4.37 -> 4.15 ms per pass on the same box (the output pages are reused by consecutive instructions)
        const uint32_t slot = (uint32_t)w * (WAVE * LSB_KPT) + i * WAVE + lane;
        uint32_t k, v = 0;
        if (HAS_VALUES) {
            const uint2 kv = reinterpret_cast<const uint2 *>(sm.stage)[slot];
            k = kv.x; v = kv.y;
        } else {
            k = sm.stage[slot];
        }
        const auto g = sm.gbase[digit(k)];
        if (!TAIL || slot < valid) {
            if constexpr (OFF64) {
                const uint64_t dst = g + slot;
                keys_out[dst] = tw_out(k);
                if (HAS_VALUES) vals_out[dst] = v;
            } else if (BIG) {
                const uint32_t dst = g + slot;
                keys_out[dst] = tw_out(k);
                if (HAS_VALUES) vals_out[dst] = v;
            } else {
                const uint32_t off = g + slot * 4u;             // 32-bit byte offset: scalar base + vector offset
                *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(keys_out) + off) = tw_out(k);
                if (HAS_VALUES) *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(vals_out) + off) = v;
            }
        }
    }
    GS_PHASE(7);                                   // store issue
#ifdef GS_EXP_DRAIN
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // experiment: the wave stays until its stores are acknowledged
#endif
    GS_PHASE_WAIT("vmcnt(0)");
    GS_PHASE(8);                                   // store drain
#ifdef GS_EXP_PHASES
    if (tid == 0 && t < 131072u) {                 // clock calibration: shader clocks vs 100 MHz real time; who and where
        gs_phase_buf[t * 16 + 9] = (uint32_t)(__builtin_amdgcn_s_memtime() - t0_);
        gs_phase_buf[t * 16 + 10] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - r0_);
        gs_phase_buf[t * 16 + 11] = (uint32_t)r0_;
        gs_phase_buf[t * 16 + 12] = blockIdx.x;
        gs_phase_buf[t * 16 + 13] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
        gs_phase_buf[t * 16 + 14] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID
    }
#endif
}
