// topk_rows_check.cpp -- gpusort::DeviceTopKRows against gpusort::DeviceTopK, compiled against gpusort.hpp: for shapes on each
// of the three paths (one wave per row, one workgroup per row, chunked) and unsigned int / int / float keys, take the top k of
// every row in one call and of each row alone with DeviceTopK, in the keys, pairs and arguments forms, Min and Max; every row
// must agree bit for bit.  The rows sit at a stride of num_cols + 3.
//   usage: topk_rows_check     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

// input 1: one top byte, the later select rounds work; input 2: eight values
static const Inputs<unsigned int> INPUTS = {0x00ffffffu, 0x3f000000u, 0x80000003u, 0, 0, {}};

template <typename KeyT>
static int test_case(size_t rows, size_t cols, size_t k, bool descending, int spread)
{
    const size_t stride = cols + 3, n = rows * stride;
    std::mt19937_64 rng(977 + rows * 7 + cols * 3 + k);
    std::vector<unsigned int> h_keys(n), h_vals(n);
    fill(rng, spread, INPUTS, h_keys, h_vals);
    KeyT *d_in, *d_rows, *d_one;
    unsigned int *d_vin, *d_rows_v, *d_one_v;
    HIP_OK(hipMalloc(&d_in, n * 4)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_rows, rows * k * 4)); HIP_OK(hipMalloc(&d_rows_v, rows * k * 4));
    HIP_OK(hipMalloc(&d_one, rows * k * 4)); HIP_OK(hipMalloc(&d_one_v, rows * k * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    int bad = 0;
    std::vector<unsigned int> got_k(rows * k), got_v(rows * k), want_k(rows * k), want_v(rows * k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_rows, 0xee, rows * k * 4)); HIP_OK(hipMemset(d_rows_v, 0xee, rows * k * 4));
        HIP_OK(hipMemset(d_one, 0xee, rows * k * 4)); HIP_OK(hipMemset(d_one_v, 0xee, rows * k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        HIP_OK((top<gpusort::DeviceTopKRows>(mode, descending, d_temp, temp_bytes, d_in, d_rows, vin, d_rows_v, rows, cols, stride, k)));
        if (temp_bytes == 0) { printf("size query refused rows=%zu cols=%zu k=%zu\n", rows, cols, k); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK((top<gpusort::DeviceTopKRows>(mode, descending, d_temp, temp_bytes, d_in, d_rows, vin, d_rows_v, rows, cols, stride, k)));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        // the reference: DeviceTopK on each row alone
        d_temp = nullptr; temp_bytes = 0;
        auto one = [&](size_t r) -> hipError_t {
            return top<gpusort::DeviceTopK>(mode, descending, d_temp, temp_bytes, d_in + r * stride, d_one + r * k,
                                            vin ? vin + r * stride : nullptr, d_one_v + r * k, cols, k);
        };
        HIP_OK(one(0));
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        for (size_t r = 0; r < rows; ++r) HIP_OK(one(r));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_rows, rows * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_rows_v, rows * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_k.data(), d_one, rows * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_v.data(), d_one_v, rows * k * 4, hipMemcpyDeviceToHost));
        int b = memcmp(got_k.data(), want_k.data(), rows * k * 4) != 0;
        if (mode && memcmp(got_v.data(), want_v.data(), rows * k * 4) != 0) b = 1;
        bad += b;
        printf("%s keys, %s, rows=%zu, cols=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(), mode_name(mode), rows, cols, k,
               descending ? "max" : "min", spread, b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_rows)); HIP_OK(hipFree(d_rows_v));
    HIP_OK(hipFree(d_one)); HIP_OK(hipFree(d_one_v));
    return bad;
}

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][3] = {{9, 64, 8}, {5, 257, 100}, {3, 1024, 1024}, {3, 1025, 64}, {2, 8192, 1000}, {2, 8197, 1024}, {2, 20000, 50}};
    int i = 0;
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread, ++i) bad += test_case<KeyT>(s[0], s[1], s[2], (i & 1) != 0, spread);
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
