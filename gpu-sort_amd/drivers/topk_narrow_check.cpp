// topk_narrow_check.cpp -- gpusort::DeviceTopK on 16-bit keys (gs_topk_u16), compiled against gpusort.hpp: for sizes on each of
// the three routes and unsigned short / short / _Float16 / __hip_bfloat16 keys, take the top k of a flat array in the keys,
// pairs and arguments forms, Min and Max, and check the result against a stable sort on the host of the 16-bit image
// (GS_KEY_F32's map at width 16 for the float types).  The key input starts one element into its allocation in every second
// case, so its base alternates between 4- and 2-byte alignment.
//   usage: topk_narrow_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, past 65536 elements the input is re-read; input 2: eight values
static const Inputs<uint16_t> INPUTS = {0x00ffu, 0x3f00u, 0x8003u, 0, 0, {}};

template <typename KeyT>
static int test_case(size_t n, size_t k, bool descending, int spread, size_t in_off)
{
    constexpr int kt = gpusort::KeyTraits<KeyT>::type;
    std::mt19937_64 rng(2024 + n * 7 + k * 3 + spread);
    std::vector<uint16_t> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    fill(rng, spread, INPUTS, h_keys, h_vals);
    uint16_t *d_alloc;
    KeyT *d_out;
    unsigned int *d_vin, *d_vout;
    HIP_OK(hipMalloc(&d_alloc, (n + in_off) * 2)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, k * 2)); HIP_OK(hipMalloc(&d_vout, k * 4));
    const KeyT *d_in = reinterpret_cast<const KeyT *>(d_alloc + in_off);
    HIP_OK(hipMemcpy(d_alloc + in_off, h_keys.data(), n * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: the stable order on the image
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return image_of(h_keys[a], kt, descending) < image_of(h_keys[b], kt, descending); });

    int bad = 0;
    std::vector<uint16_t> got_k(k);
    std::vector<unsigned int> got_v(k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_out, 0xee, k * 2)); HIP_OK(hipMemset(d_vout, 0xee, k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t { return top<gpusort::DeviceTopK>(mode, descending, d_temp, temp_bytes, d_in, d_out, vin, d_vout, n, k); };
        HIP_OK(run());
        if (temp_bytes == 0 || temp_bytes != gs_topk_u16_temp_bytes(n, k, mode != 0)) { printf("the shim asked another size query\n"); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        uint32_t st[8];
        HIP_OK((hipError_t)gs_topk_u16_status(d_temp, n, k, mode != 0, st, nullptr));
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_out, k * 2, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_vout, k * 4, hipMemcpyDeviceToHost));
        int b = 0;
        for (size_t i = 0; i < k; ++i) {
            const uint32_t j = order[i];
            if (got_k[i] != h_keys[j]) b = 1;
            if (mode == 1 && got_v[i] != h_vals[j]) b = 1;
            if (mode == 2 && got_v[i] != j) b = 1;
        }
        if (st[1] != image_of(h_keys[order[k - 1]], kt, descending) || st[2] + st[3] != k) b = 1;
        bad += b;
        printf("%s keys, %s, n=%zu, k=%zu, %s, input %d, offset %zu, route %u: %s\n", name_of<KeyT>(), mode_name(mode), n, k,
               descending ? "max" : "min", spread, in_off, st[0], b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_alloc)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    return bad;
}

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][2] = {{1, 1}, {777, 100}, {8192, 8192}, {8193, 1}, {24581, 5000}, {70001, 70001}, {100003, 1000},
                                {300007, 65537}};
    int i = 0;
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread, ++i) bad += test_case<KeyT>(s[0], s[1], (i & 1) != 0, spread, (size_t)((i >> 1) & 1));
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
