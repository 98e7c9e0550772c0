// gs_seg_wave4_body.inc -- the body of seg_wave4_sort_kernel (gs_msb.hip): one wave sorts four segments of up to 64 elements.
// A fragment for the same reason as gs_seg_wave_body.inc; the including kernel declares K, HAS_VALUES, FW and the same parameters.
    constexpr int NS = 4;                                          // segments per wave and step
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][NS][RADIX];
    __shared__ uint32_t stage_k[4][NS * WAVE];
    __shared__ uint32_t stage_v[HAS_VALUES ? 4 : 1][HAS_VALUES ? NS * WAVE : 1];
    const int w = wave_id(), lane = lane_id();
    uint32_t ntasks = ws.level[2].task_count[3];
    if (ntasks > ws.max_tasks) ntasks = ws.max_tasks;
    auto fence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (uint32_t t0 = (blockIdx.x * 4u + (uint32_t)w) * NS; t0 < ntasks; t0 += gridDim.x * 4u * NS) {
        uint32_t off[NS], size[NS], key[NS], val[HAS_VALUES ? NS : 1], pos[NS];
        uint32_t B = 0, shift0 = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            off[i] = 0; size[i] = 0;
            if (t0 + i < ntasks) {                                 // wave-uniform
                const MsbTask Tv = ws.tasks[3][ws.max_tasks - 1u - (t0 + i)];
                off[i] = __builtin_amdgcn_readfirstlane(Tv.offset); size[i] = __builtin_amdgcn_readfirstlane(Tv.size);
                B = __builtin_amdgcn_readfirstlane(Tv.sort_bits); shift0 = __builtin_amdgcn_readfirstlane(Tv.pad);   // the same for every segment of a call
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            key[i] = 0xffffffffu;
            if (HAS_VALUES) val[i] = 0;
            if ((uint32_t)lane < size[i]) {
                key[i] = twiddle_in(float_flip<FW>(src_k[off[i] + lane]), f32_in, xor_in);
                if (HAS_VALUES) val[i] = src_v[off[i] + lane];
            } else {
                key[i] = 0xffffffffu;                              // pads: behind the segment's elements, largest in every digit
            }
        }
        for (uint32_t done = 0; done < B; done += RADIX_BITS) {
            const uint32_t bw = B - done < (uint32_t)RADIX_BITS ? B - done : (uint32_t)RADIX_BITS, sh = shift0 + done;
#pragma unroll
            for (int i = 0; i < NS; ++i) reinterpret_cast<uint4 *>(hist[w][i])[lane] = make_uint4(0u, 0u, 0u, 0u);
            fence();
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const uint32_t d = __builtin_amdgcn_ubfe(key[i], sh, bw);
                uint32_t lo, hi;
                match_digit(d, lo, hi);
                pos[i] = count_lower(lo, hi);
                if (pos[i] == 0) hist[w][i][d] = (uint32_t)(__popc(lo) + __popc(hi));
            }
            fence();
#pragma unroll
            for (int i = 0; i < NS; ++i) {   // exclusive scan of segment i's 256 counters, 4 per lane
                const uint4 c = reinterpret_cast<const uint4 *>(hist[w][i])[lane];
                const uint32_t sum = c.x + c.y + c.z + c.w;
                const uint32_t ex = wave_inclusive_scan(sum) - sum;
                reinterpret_cast<uint4 *>(hist[w][i])[lane] = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
            }
            fence();
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const uint32_t at = (uint32_t)(i * WAVE) + pos[i] + hist[w][i][__builtin_amdgcn_ubfe(key[i], sh, bw)];
                stage_k[w][at] = key[i];
                if (HAS_VALUES) stage_v[w][at] = val[i];
            }
            fence();
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                key[i] = stage_k[w][i * WAVE + lane];
                if (HAS_VALUES) val[i] = stage_v[w][i * WAVE + lane];
            }
            fence();
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if ((uint32_t)lane < size[i]) {
                dst_k[off[i] + lane] = (K)float_flip<FW>(twiddle_out(key[i], f32_out, xor_out));
                if (HAS_VALUES) dst_v[off[i] + lane] = val[i];
            }
        }
    }
