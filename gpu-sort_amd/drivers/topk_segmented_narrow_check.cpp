// topk_segmented_narrow_check.cpp -- gpusort::DeviceTopKSegmented on 16-bit keys (gs_topk_segmented_u16) against
// gpusort::DeviceTopK (gs_topk_u16), compiled against gpusort.hpp: the ragged set of topk_segmented_check (every list of the
// classify kernel: empty, one wave of each class, one workgroup, chunked; a gap of 5, so that segments start at odd elements;
// a repeat, clamped offsets, a segment in reverse place) is taken in one call and segment by segment with DeviceTopK at
// k = min(k, length), in the keys, pairs and arguments forms, Min and Max, for unsigned short / short / _Float16 /
// __hip_bfloat16 keys; every segment's first count elements and the counts must agree bit for bit, and the slots behind a
// segment's count must keep their fill.
//   usage: topk_segmented_narrow_check     prints OK and exits 0 iff every case matches; stops at the first case with a mismatch
#include "topk_check_common.hpp"

// input 0: every 16th key at one end of the image, the pad's too, in turn; input 1: one top byte, the second select round
// decides; input 2: eight values
static const Inputs<uint16_t> INPUTS = {0x00ffu, 0x3f00u, 0x8003u, 0, 16, {0x0000u, 0xffffu}};

// k = 1, an odd k inside a class and the odd k below the maximum; both directions at every k; the three inputs in turn
template <typename KeyT>
static int test_type()
{
    const size_t ks[] = {1, 51, 1023};
    int i = 0;
    for (size_t k : ks)
        for (int desc = 0; desc < 2; ++desc, ++i)
            if (segmented_case<KeyT>(k, desc != 0, i % 3, 5231 + k * 3 + i % 3, INPUTS, gs_topk_segmented_u16_temp_bytes)) return 1;
    return 0;
}

int main()
{
    int bad = test_type<unsigned short>();
    if (!bad) bad = test_type<short>();
    if (!bad) bad = test_type<_Float16>();
    if (!bad) bad = test_type<__hip_bfloat16>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
