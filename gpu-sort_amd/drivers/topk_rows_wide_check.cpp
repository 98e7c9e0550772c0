// topk_rows_wide_check.cpp -- gpusort::DeviceTopKRows on 64-bit keys (gs_topk_rows_u64), compiled against gpusort.hpp: for
// shapes on each of the three paths and unsigned long long / long long / double keys, take the top k of every row in the
// keys, pairs and arguments forms, Min and Max, and check every row against a stable sort on the host of the 64-bit image
// (GS_KEY_F32's map at width 64 for double).  The rows sit at a stride of num_cols + 3.  Three inputs per shape: random
// words, integers below 2^24 (five bytes shared: the kernels leave their passes and rounds out), and eight values (the cut
// falls inside a run of equal keys).
//   usage: topk_rows_wide_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

static const Inputs<uint64_t> INPUTS = {0xffffffull, 0, 0x8000000000000003ull, 0, 0, {}};

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][3] = {{9, 64, 7}, {5, 257, 101}, {3, 1024, 1024}, {3, 1025, 65}, {2, 8192, 1000}, {2, 8197, 1023}, {2, 20000, 50}};
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread)
            for (int descending = 0; descending < 2; ++descending)
                bad += rows_case<gpusort::DeviceTopKRows, KeyT>(s[0], s[1], s[2], descending != 0, spread, 1977 + s[0] * 7 + s[1] * 3 + s[2],
                                                                INPUTS, gs_topk_rows_u64_temp_bytes);
    return bad;
}

int main()
{
    int bad = 0;
    bad += test_type<unsigned long long>();
    bad += test_type<long long>();
    bad += test_type<double>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
