// topk_segmented_check.cpp -- gpusort::DeviceTopKSegmented against gpusort::DeviceTopK, compiled against gpusort.hpp: one
// ragged set of segments (every list of the classify kernel: empty, one wave of each class, one workgroup, chunked; a gap, a
// repeat, a segment in reverse place) is taken in one call and segment by segment with DeviceTopK at k = min(k, length), in the
// keys, pairs and arguments forms, Min and Max, for unsigned int / int / float keys; every segment's first count elements and
// the counts must agree bit for bit, and the slots behind a segment's count must keep their fill.
//   usage: topk_segmented_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, the later select rounds work; input 2: eight values
static const Inputs<unsigned int> INPUTS = {0x00ffffffu, 0x3f000000u, 0x80000003u, 0, 0, {}};

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t ks[] = {1, 50, 1024};
    int i = 0;
    for (size_t k : ks)
        for (int spread = 0; spread < 3; ++spread, ++i)
            bad += segmented_case<KeyT>(k, (i & 1) != 0, spread, 4177 + k * 3 + spread, INPUTS, gs_topk_segmented_temp_bytes);
    return bad;
}

int main()
{
    int bad = 0;
    bad += test_type<unsigned int>();
    bad += test_type<int>();
    bad += test_type<float>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
