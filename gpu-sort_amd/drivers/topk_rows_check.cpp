// topk_rows_check.cpp -- gpusort::DeviceTopKRows against gpusort::DeviceTopK, compiled against gpusort.hpp: for shapes on each
// of the three paths (one wave per row, one workgroup per row, chunked) and unsigned int / int / float keys, take the top k of
// every row in one call and of each row alone with DeviceTopK, in the keys, pairs and arguments forms, Min and Max; every row
// must agree bit for bit.  The rows sit at a stride of num_cols + 3.
//   usage: topk_rows_check     prints OK and exits 0 iff every case matches
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gpusort.hpp"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); exit(2); } } while (0)

template <typename T> static const char *name_of();
template <> const char *name_of<unsigned int>() { return "u32"; }
template <> const char *name_of<int>() { return "i32"; }
template <> const char *name_of<float>() { return "f32"; }

template <typename KeyT>
static int test_case(size_t rows, size_t cols, size_t k, bool descending, int spread)
{
    const size_t stride = cols + 3, n = rows * stride;
    std::mt19937_64 rng(977 + rows * 7 + cols * 3 + k);
    std::vector<unsigned int> h_keys(n), h_vals(n);
    for (size_t i = 0; i < n; ++i) {
        unsigned int bits = (unsigned int)rng();
        if (spread == 1) bits = (bits & 0x00ffffffu) | 0x3f000000u;   // one top byte: the later select rounds work
        if (spread == 2) bits &= 0x80000003u;                          // eight values: the cut falls inside a run of equal keys
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
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
        auto run = [&]() -> hipError_t {
            if (mode == 0)
                return descending ? gpusort::DeviceTopKRows::MaxKeys(d_temp, temp_bytes, d_in, d_rows, rows, cols, stride, k)
                                  : gpusort::DeviceTopKRows::MinKeys(d_temp, temp_bytes, d_in, d_rows, rows, cols, stride, k);
            return descending ? gpusort::DeviceTopKRows::MaxPairs(d_temp, temp_bytes, d_in, d_rows, vin, d_rows_v, rows, cols, stride, k)
                              : gpusort::DeviceTopKRows::MinPairs(d_temp, temp_bytes, d_in, d_rows, vin, d_rows_v, rows, cols, stride, k);
        };
        HIP_OK(run());
        if (temp_bytes == 0) { printf("size query refused rows=%zu cols=%zu k=%zu\n", rows, cols, k); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        // the reference: DeviceTopK on each row alone
        d_temp = nullptr; temp_bytes = 0;
        auto one = [&](size_t r) -> hipError_t {
            const KeyT *ki = d_in + r * stride;
            const unsigned int *vi = vin ? vin + r * stride : nullptr;
            if (mode == 0)
                return descending ? gpusort::DeviceTopK::MaxKeys(d_temp, temp_bytes, ki, d_one + r * k, cols, k)
                                  : gpusort::DeviceTopK::MinKeys(d_temp, temp_bytes, ki, d_one + r * k, cols, k);
            return descending ? gpusort::DeviceTopK::MaxPairs(d_temp, temp_bytes, ki, d_one + r * k, vi, d_one_v + r * k, cols, k)
                              : gpusort::DeviceTopK::MinPairs(d_temp, temp_bytes, ki, d_one + r * k, vi, d_one_v + r * k, cols, k);
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
        printf("%s keys, %s, rows=%zu, cols=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(),
               mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments", rows, cols, k, descending ? "max" : "min", spread,
               b ? "FAIL" : "CORRECT");
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
