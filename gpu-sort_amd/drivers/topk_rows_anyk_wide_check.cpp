// topk_rows_anyk_wide_check.cpp -- gpusort::DeviceTopKRowsAnyK on 64-bit keys (gs_topk_rows_anyk_u64), compiled against
// gpusort.hpp: shapes on both paths (one workgroup per row up to 8192 columns, the descent over all rows above), k below and
// above what the segmented finish sorts in one workgroup, for unsigned long long / long long / double keys, in the keys, pairs
// and arguments forms, Min and Max; every row must be, bit for bit, the first k of the host's std::stable_sort of that row on
// the 64-bit image (GS_KEY_F32's map at width 64 for double).  The rows sit at a stride of num_cols + 3: the gap holds random
// words that would win.  Three inputs per shape: random words (a list after one round); integers below 2^24 (the first round
// only learns the bits that differ, the second one decides: more than one round); eight values (a tie run, the cut inside it).
// A fourth case per type is a matrix of one key.
//   usage: topk_rows_anyk_wide_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

static const Inputs<uint64_t> INPUTS = {0xffffffull, 0, 0x8000000000000003ull, 0, 0, {}};
static const Inputs<uint64_t> ONE_KEY = {0, 0x3ff0000000000123ull, 0, 0x3ff0000000000123ull, 0, {}};

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][3] = {{3, 1025, 1025}, {2, 8192, 3000}, {2, 8193, 2000}, {3, 40000, 9000}, {1, 33000, 33000}};
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread)
            for (int descending = 0; descending < 2; ++descending)
                bad += rows_case<gpusort::DeviceTopKRowsAnyK, KeyT>(s[0], s[1], s[2], descending != 0, spread, 1977 + s[0] * 7 + s[1] * 3 + s[2],
                                                                    INPUTS, gs_topk_rows_anyk_u64_temp_bytes);
    bad += rows_case<gpusort::DeviceTopKRowsAnyK, KeyT>(2, 35000, 5000, false, 1, 7, ONE_KEY, gs_topk_rows_anyk_u64_temp_bytes);
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
