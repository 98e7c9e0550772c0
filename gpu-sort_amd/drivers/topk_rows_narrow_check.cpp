// topk_rows_narrow_check.cpp -- gpusort::DeviceTopKRows on 16-bit keys (gs_topk_rows_u16), compiled against gpusort.hpp: for
// shapes on each of the three paths and unsigned short / short / _Float16 / __hip_bfloat16 keys, take the top k of every row
// in the keys, pairs and arguments forms, Min and Max, and check every row against a stable sort on the host of the 16-bit
// image (GS_KEY_F32's map at width 16 for the float types).  The rows sit at a stride of num_cols + 3, so row bases alternate
// between 2- and 4-byte alignment.
//   usage: topk_rows_narrow_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, the second select round works; input 2: eight values
static const Inputs<uint16_t> INPUTS = {0x00ffu, 0x3f00u, 0x8003u, 0, 0, {}};

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][3] = {{9, 64, 7}, {5, 257, 101}, {3, 1024, 1024}, {3, 1025, 65}, {2, 8192, 1000}, {2, 8197, 1023}, {2, 20000, 50}};
    int i = 0;
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread, ++i)
            bad += rows_case<gpusort::DeviceTopKRows, KeyT>(s[0], s[1], s[2], (i & 1) != 0, spread, 1977 + s[0] * 7 + s[1] * 3 + s[2], INPUTS,
                                                            gs_topk_rows_u16_temp_bytes);
    return bad;
}

int main()
{
    int bad = 0;
    bad += test_type<unsigned short>();
    bad += test_type<short>();
    bad += test_type<_Float16>();
    bad += test_type<__hip_bfloat16>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
