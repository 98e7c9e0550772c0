// topk_rows_anyk_check.cpp -- gpusort::DeviceTopKRowsAnyK against std::stable_sort, compiled against gpusort.hpp: for shapes on
// both paths (one workgroup per row up to 8192 columns, the radix select over all rows above), k below and above what the
// segmented finish sorts in one workgroup, and unsigned int / int / float keys, take the top k of every row in one call, in the
// keys, pairs and arguments forms, Min and Max; every row must be, bit for bit, the first k of the host's stable sort of that
// row on the key type's order-preserving image.  The rows sit at a stride of num_cols + 3.
//   usage: topk_rows_anyk_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: twelve shared top bits, the later rounds work; input 2: eight values
static const Inputs<unsigned int> INPUTS = {0x000fffffu, 0x3f000000u, 0x80000003u, 0, 0, {}};

template <typename KeyT>
static int test_type(int first)
{
    int bad = 0;
    const size_t shapes[][3] = {{3, 1025, 1025}, {2, 8192, 3000}, {2, 8193, 2000}, {3, 40000, 9000}, {2, 70001, 20000}, {1, 33000, 33000}};
    int i = first;
    for (const auto &s : shapes) {
        bad += rows_case<gpusort::DeviceTopKRowsAnyK, KeyT>(s[0], s[1], s[2], (i & 1) != 0, i % 3, 1977 + s[0] * 7 + s[1] * 3 + s[2], INPUTS,
                                                            gs_topk_rows_anyk_temp_bytes);
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
