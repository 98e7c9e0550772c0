// topk_wide_check.cpp -- gpusort::DeviceTopK on 64-bit keys (gs_topk_u64), compiled against gpusort.hpp: for unsigned long
// long / long long / double keys, sizes from one element to several tiles and inputs that end the descent at D = 1, by the
// skip of constant bytes, and on a run of equal keys, take the top k of a flat array in the keys, pairs and arguments forms,
// Min and Max, and check the result against a stable sort on the host of the 64-bit image.  The key input starts one element
// into its allocation in every second case.
//   usage: topk_wide_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: integers below 2^24, bytes 6..3 are skipped; input 2: four values, the cut falls inside a run of equal keys (route
// 2 once a run is longer than the candidate list)
static const Inputs<uint64_t> INPUTS = {0xffffffull, 0, 0x8000000000000001ull, 0, 0, {}};

template <typename KeyT>
static int test_case(size_t n, size_t k, bool descending, int spread, size_t in_off)
{
    constexpr int kt = gpusort::KeyTraits<KeyT>::type;
    std::mt19937_64 rng(2024 + n * 7 + k * 3 + spread);
    std::vector<uint64_t> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    fill(rng, spread, INPUTS, h_keys, h_vals);
    uint64_t *d_alloc;
    KeyT *d_out;
    unsigned int *d_vin, *d_vout;
    HIP_OK(hipMalloc(&d_alloc, (n + in_off) * 8)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, k * 8)); HIP_OK(hipMalloc(&d_vout, k * 4));
    const KeyT *d_in = reinterpret_cast<const KeyT *>(d_alloc + in_off);
    HIP_OK(hipMemcpy(d_alloc + in_off, h_keys.data(), n * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: the stable order on the image
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return image_of(h_keys[a], kt, descending) < image_of(h_keys[b], kt, descending); });

    int bad = 0;
    std::vector<uint64_t> got_k(k);
    std::vector<unsigned int> got_v(k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_out, 0xee, k * 8)); HIP_OK(hipMemset(d_vout, 0xee, k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t { return top<gpusort::DeviceTopK>(mode, descending, d_temp, temp_bytes, d_in, d_out, vin, d_vout, n, k); };
        HIP_OK(run());
        if (temp_bytes == 0 || temp_bytes != gs_topk_u64_temp_bytes(n, k, mode != 0)) { printf("the shim asked another size query\n"); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        uint32_t st[8];
        HIP_OK((hipError_t)gs_topk_u64_status(d_temp, n, k, mode != 0, st, nullptr));
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_out, k * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_vout, k * 4, hipMemcpyDeviceToHost));
        int b = 0;
        for (size_t i = 0; i < k; ++i) {
            const uint32_t j = order[i];
            if (got_k[i] != h_keys[j]) b = 1;
            if (mode == 1 && got_v[i] != h_vals[j]) b = 1;
            if (mode == 2 && got_v[i] != j) b = 1;
        }
        const uint64_t kth = image_of(h_keys[order[k - 1]], kt, descending);
        if (st[1] != (uint32_t)kth || st[2] != (uint32_t)(kth >> 32) || st[3] + st[4] != k) b = 1;
        if (st[6] != (st[5] == 1 ? 2u : st[5] + 2u)) b = 1;
        bad += b;
        printf("%s keys, %s, n=%zu, k=%zu, %s, input %d, offset %zu, route %u, D %u: %s\n", name_of<KeyT>(), mode_name(mode), n, k,
               descending ? "max" : "min", spread, in_off, st[0], st[5], b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_alloc)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    return bad;
}

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][2] = {{1, 1}, {777, 100}, {4096, 4096}, {4097, 1}, {24581, 5000}, {70001, 70001}, {100003, 1000},
                                {300007, 65537}};
    int i = 0;
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread, ++i) bad += test_case<KeyT>(s[0], s[1], (i & 1) != 0, spread, (size_t)((i >> 1) & 1));
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
