// topk_segmented_wide_check.cpp -- gpusort::DeviceTopKSegmented on 64-bit keys (gs_topk_segmented_u64) against std::stable_sort
// of every segment on the host, compiled against gpusort.hpp: for each of the six lists of the classify kernel (the four wave
// classes, one workgroup, chunked) a call whose segments all fall into that list -- laid out with a gap of 5, with an empty
// segment, a repeat and offsets that need clamping --, in the keys, pairs and arguments forms, Min and Max, for unsigned long
// long / long long / double keys; every segment's first count elements and the counts must agree bit for bit, and the slots
// behind a segment's count must keep their fill.
//   usage: topk_segmented_wide_check     prints OK and exits 0 iff every case matches; stops at the first mismatch
#include "topk_check_common.hpp"

// input 0: every third key a special value; input 1: integers below 2^24, five bytes are constant; input 2: eight values, the
// cut falls inside a tie run
static const Inputs<uint64_t> INPUTS = {0xffffffull, 0, 0x8000000000000003ull, 0x3ff0000000000000ull, 3,
                                        {0x7ff8000000000001ull, 0xfff8000000000001ull, 0xffffffffffffffffull, 0x7ff0000000000000ull,
                                         0xfff0000000000000ull, 0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull,
                                         0x7fffffffffffffffull, 0x3ff0000000000000ull, 0xbff0000000000000ull}};

static const size_t CLASS_LENS[6][4] = {{1, 40, 64, 0}, {65, 200, 256, 0}, {257, 400, 512, 0}, {513, 900, 1024, 0},
                                        {1025, 3000, 8192, 0}, {8193, 20000, 0, 0}};

template <typename KeyT>
static int test_case(int cls, int mode, bool descending, size_t k, int spread)
{
    static_assert(sizeof(KeyT) == 8, "64-bit keys");
    constexpr int kt = gpusort::KeyTraits<KeyT>::type;
    std::vector<int> begin, end;
    size_t n = 3;
    for (int j = 0; j < 4 && CLASS_LENS[cls][j]; ++j) {
        begin.push_back((int)n); end.push_back((int)(n + CLASS_LENS[cls][j]));
        n += CLASS_LENS[cls][j] + 5;
    }
    const size_t first_len = CLASS_LENS[cls][0];
    // segments longer than CH = 8192 must together not exceed num_items: the chunked list's repeat and its two clamped
    // segments get that many more elements behind the others
    if (first_len > 8192) n += CLASS_LENS[cls][1] + 2 * first_len;
    begin.push_back(begin[1]); end.push_back(end[1]);                         // a repeated segment
    begin.push_back(500); end.push_back(100);                                 // end < begin: empty
    begin.push_back(-7); end.push_back((int)first_len);                       // clamped below: the first first_len elements
    begin.push_back((int)(n - first_len)); end.push_back((int)n + 100);       // clamped above: the last first_len elements
    const size_t S = begin.size();
    std::mt19937_64 rng(7121 + 31 * cls + 7 * mode + k + spread);
    std::vector<uint64_t> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    fill(rng, spread, INPUTS, h_keys, h_vals);
    KeyT *d_in, *d_out;
    unsigned int *d_vin, *d_vout, *d_counts;
    int *d_begin, *d_end;
    HIP_OK(hipMalloc(&d_in, n * 8)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, S * k * 8)); HIP_OK(hipMalloc(&d_vout, S * k * 4));
    HIP_OK(hipMalloc(&d_counts, S * 4)); HIP_OK(hipMalloc(&d_begin, S * 4)); HIP_OK(hipMalloc(&d_end, S * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_begin, begin.data(), S * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_end, end.data(), S * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0xee, S * k * 8)); HIP_OK(hipMemset(d_vout, 0xee, S * k * 4)); HIP_OK(hipMemset(d_counts, 0xee, S * 4));

    const unsigned int *vin = mode == 1 ? d_vin : nullptr;
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
    auto run = [&]() -> hipError_t {
        return top<gpusort::DeviceTopKSegmented>(mode, descending, d_temp, temp_bytes, d_in, d_out, vin, d_vout, d_counts, n, (uint32_t)S,
                                                 d_begin, d_end, k);
    };
    HIP_OK(run());
    if (temp_bytes == 0 || temp_bytes != gs_topk_segmented_u64_temp_bytes(n, (uint32_t)S, k, mode != 0)) {
        printf("the shim asked another size query n=%zu S=%zu k=%zu\n", n, S, k);
        return 1;
    }
    HIP_OK(hipMalloc(&d_temp, temp_bytes));
    HIP_OK(run());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipFree(d_temp));

    std::vector<uint64_t> got_k(S * k), want_k(S * k, 0xeeeeeeeeeeeeeeeeull);
    std::vector<unsigned int> got_v(S * k), want_v(S * k, 0xeeeeeeeeu), counts(S);
    HIP_OK(hipMemcpy(got_k.data(), d_out, S * k * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(got_v.data(), d_vout, S * k * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(counts.data(), d_counts, S * 4, hipMemcpyDeviceToHost));
    int b = 0;
    for (size_t s = 0; s < S; ++s) {   // the reference: std::stable_sort of the clamped segment's positions by image
        const long lo = std::max<long>(begin[s], 0), hi = std::min<long>(end[s], (long)n);
        const size_t len = hi > lo ? (size_t)(hi - lo) : 0, kept = std::min(k, len);
        if (counts[s] != kept) b = 1;
        std::vector<unsigned int> order(len);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](unsigned int x, unsigned int y) {
            return image_of(h_keys[lo + x], kt, descending) < image_of(h_keys[lo + y], kt, descending);
        });
        for (size_t i = 0; i < kept; ++i) {
            want_k[s * k + i] = h_keys[lo + order[i]];
            if (mode) want_v[s * k + i] = mode == 1 ? h_vals[lo + order[i]] : order[i];
        }
    }
    // the reference buffers keep the fill behind every count, so whole-buffer equality also proves the unwritten slots
    if (memcmp(got_k.data(), want_k.data(), S * k * 8) != 0) b = 1;
    if (memcmp(got_v.data(), want_v.data(), S * k * 4) != 0) b = 1;
    printf("%s keys, %s, list %d, segments=%zu, items=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(), mode_name(mode), cls, S, n, k,
           descending ? "max" : "min", spread, b ? "FAIL" : "CORRECT");
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    HIP_OK(hipFree(d_counts)); HIP_OK(hipFree(d_begin)); HIP_OK(hipFree(d_end));
    return b;
}

// every list x form x direction; k = 1, an odd k inside a class and the odd k below the maximum, and the three inputs, in turn
template <typename KeyT>
static int test_type()
{
    const size_t ks[] = {1, 51, 1023};
    int i = 0;
    for (int cls = 0; cls < 6; ++cls)
        for (int mode = 0; mode < 3; ++mode)
            for (int desc = 0; desc < 2; ++desc, ++i)
                if (test_case<KeyT>(cls, mode, desc != 0, ks[(i + cls) % 3], (i / 2 + cls) % 3)) return 1;
    return 0;
}

int main()
{
    int bad = test_type<unsigned long long>();
    if (!bad) bad = test_type<long long>();
    if (!bad) bad = test_type<double>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
