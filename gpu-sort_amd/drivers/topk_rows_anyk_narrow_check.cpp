// topk_rows_anyk_narrow_check.cpp -- gpusort::DeviceTopKRowsAnyK on 16-bit keys (gs_topk_rows_anyk_u16), compiled against
// gpusort.hpp: the cases of topk_rows_anyk_check -- shapes on both paths (one workgroup per row up to 8192 columns, the radix
// select over all rows above), k below and above what the segmented finish sorts in one workgroup -- for unsigned short / short /
// _Float16 / __hip_bfloat16 keys, in the keys, pairs and arguments forms, Min and Max; every row must be, bit for bit, the first k
// of the host's stable sort of that row on the 16-bit image (GS_KEY_F32's map at width 16 for the float types).  The rows sit at
// a stride of num_cols + 3, so row bases alternate between 2- and 4-byte alignment; the row of 70001 columns has ties by force.
//   usage: topk_rows_anyk_narrow_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, the second counting round works; input 2: eight values
static const Inputs<uint16_t> INPUTS = {0x00ffu, 0x3f00u, 0x8003u, 0, 0, {}};

template <typename KeyT>
static int test_type(int first)
{
    int bad = 0;
    const size_t shapes[][3] = {{3, 1025, 1025}, {2, 8192, 3000}, {2, 8193, 2000}, {3, 40000, 9000}, {2, 70001, 20000}, {1, 33000, 33000}};
    int i = first;
    for (const auto &s : shapes) {
        bad += rows_case<gpusort::DeviceTopKRowsAnyK, KeyT>(s[0], s[1], s[2], (i & 1) != 0, i % 3, 1977 + s[0] * 7 + s[1] * 3 + s[2], INPUTS,
                                                            gs_topk_rows_anyk_u16_temp_bytes);
        ++i;
    }
    return bad;
}

int main()
{
    int bad = 0;
    bad += test_type<unsigned short>(0);
    bad += test_type<short>(1);
    bad += test_type<_Float16>(2);
    bad += test_type<__hip_bfloat16>(3);
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
