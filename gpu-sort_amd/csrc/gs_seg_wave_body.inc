// gs_seg_wave_body.inc -- the body of seg_wave_sort_kernel (gs_msb.hip): one wave sorts a segment of up to WKPT * 64 elements.
// A fragment, like gs_wide_tile.inc, so that the u32 kernel compiles to exactly the code it had before the key type became a
// parameter.  The including kernel declares K (the element type of src_k / dst_k; keys live in registers as u32), HAS_VALUES,
// WKPT, FW (the width of a narrow float key for float_flip, 0 for every other key: the identity) and the parameters ws, src_k, dst_k, src_v, dst_v, f32_in, xor_in, f32_out, xor_out.
    constexpr int LIST = WKPT == 4 ? 0 : WKPT == 8 ? 1 : 2, CAP = WKPT * WAVE;
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][RADIX];
    __shared__ uint32_t stage_k[4][CAP];
    __shared__ uint32_t stage_v[HAS_VALUES ? 4 : 1][HAS_VALUES ? CAP : 1];
    const int w = wave_id(), lane = lane_id();
    uint32_t ntasks = ws.level[2].task_count[LIST];
    if (ntasks > ws.max_tasks) ntasks = ws.max_tasks;
    uint32_t *my = hist[w];
    auto fence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (uint32_t t = blockIdx.x * 4u + (uint32_t)w; t < ntasks; t += gridDim.x * 4u) {
        const MsbTask Tv = ws.tasks[LIST][ws.max_tasks - 1u - t];
        const uint32_t off = __builtin_amdgcn_readfirstlane(Tv.offset), size = __builtin_amdgcn_readfirstlane(Tv.size);
        const uint32_t B = __builtin_amdgcn_readfirstlane(Tv.sort_bits), shift0 = __builtin_amdgcn_readfirstlane(Tv.pad);
        uint32_t key[WKPT], val[HAS_VALUES ? WKPT : 1], pos[WKPT];
        const uint32_t last = size - 1u;
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t idx = (uint32_t)(i * WAVE + lane), at = off + (idx < last ? idx : last);
            key[i] = src_k[at];
            if (HAS_VALUES) val[i] = src_v[at];
        }
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t k = twiddle_in(float_flip<FW>(key[i]), f32_in, xor_in);
            key[i] = ((uint32_t)(i * WAVE + lane) < size) ? k : 0xffffffffu;   // pads: last in position, largest in every digit
        }
        for (uint32_t done = 0; done < B; done += RADIX_BITS) {
            const uint32_t bw = B - done < (uint32_t)RADIX_BITS ? B - done : (uint32_t)RADIX_BITS, sh = shift0 + done;
            reinterpret_cast<uint4 *>(my)[lane] = make_uint4(0u, 0u, 0u, 0u);
            fence();
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t d = __builtin_amdgcn_ubfe(key[i], sh, bw);
                uint32_t lo, hi;
                match_digit(d, lo, hi);
                const uint32_t lower = count_lower(lo, hi);
                pos[i] = my[d] + lower;
                if (lower == 0) my[d] += (uint32_t)(__popc(lo) + __popc(hi));   // one lane per digit: no two writers of a word
                fence();
            }
            {   // exclusive scan of the 256 counters, 4 per lane
                const uint4 c = reinterpret_cast<const uint4 *>(my)[lane];
                const uint32_t sum = c.x + c.y + c.z + c.w;
                const uint32_t ex = wave_inclusive_scan(sum) - sum;
                reinterpret_cast<uint4 *>(my)[lane] = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
            }
            fence();
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                const uint32_t at = pos[i] + my[__builtin_amdgcn_ubfe(key[i], sh, bw)];
                stage_k[w][at] = key[i];
                if (HAS_VALUES) stage_v[w][at] = val[i];
            }
            fence();
#pragma unroll
            for (int i = 0; i < WKPT; ++i) {
                key[i] = stage_k[w][i * WAVE + lane];
                if (HAS_VALUES) val[i] = stage_v[w][i * WAVE + lane];
            }
            fence();
        }
#pragma unroll
        for (int i = 0; i < WKPT; ++i) {
            const uint32_t idx = (uint32_t)(i * WAVE + lane);
            if (idx < size) {
                dst_k[off + idx] = (K)float_flip<FW>(twiddle_out(key[i], f32_out, xor_out));
                if (HAS_VALUES) dst_v[off + idx] = val[i];
            }
        }
    }
