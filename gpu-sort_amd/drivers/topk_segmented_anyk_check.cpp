// topk_segmented_anyk_check.cpp -- gpusort::DeviceTopKSegmentedAnyK against gpusort::DeviceTopK, compiled against gpusort.hpp:
// the ragged set of topk_segmented_check with a segment of 8193 elements and one of 3 tiles + 1 more is taken in one call and
// segment by segment with DeviceTopK at k = min(k, length), in the keys, pairs and arguments forms, Min and Max, for unsigned
// int / int / float keys, at k = 1, 1024, 1025 and 5000; every segment's first count elements and the counts must agree bit for
// bit, and the slots behind a segment's count must keep their fill.
//   usage: topk_segmented_anyk_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, the later counting rounds work; input 2: eight values
static const Inputs<unsigned int> INPUTS = {0x00ffffffu, 0x3f000000u, 0x80000003u, 0, 0, {}};

template <typename KeyT>
static int test_type(int first)
{
    int bad = 0;
    const size_t ks[] = {1, 1024, 1025, 5000};
    int i = first;
    for (size_t k : ks) {   // the input rotates with k and with the type: every k meets all three over the three types
        const int spread = i % 3;
        bad += segmented_case<KeyT>(k, (i & 1) != 0, spread, 5177 + k * 3 + spread, INPUTS, gs_topk_segmented_anyk_temp_bytes,
                                    gpusort::DeviceTopKSegmentedAnyK(), true);
        ++i;
    }
    return bad;
}

int main()
{
    int bad = 0;
    bad += test_type<unsigned int>(0);
    bad += test_type<int>(1);
    bad += test_type<float>(2);
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
