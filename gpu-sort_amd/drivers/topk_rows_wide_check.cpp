// topk_rows_wide_check.cpp -- gpusort::DeviceTopKRows on 64-bit keys (gs_topk_rows_u64), compiled against gpusort.hpp: for
// shapes on each of the three paths and unsigned long long / long long / double keys, take the top k of every row in the
// keys, pairs and arguments forms, Min and Max, and check every row against a stable sort on the host of the 64-bit image
// (GS_KEY_F32's map at width 64 for double).  The rows sit at a stride of num_cols + 3.  Three inputs per shape: random
// words, integers below 2^24 (five bytes shared: the kernels leave their passes and rounds out), and eight values (the cut
// falls inside a run of equal keys).
//   usage: topk_rows_wide_check     prints OK and exits 0 iff every case matches
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>

#include "gpusort.hpp"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); exit(2); } } while (0)

template <typename T> static const char *name_of();
template <> const char *name_of<unsigned long long>() { return "u64"; }
template <> const char *name_of<long long>() { return "i64"; }
template <> const char *name_of<double>() { return "f64"; }

// the order-preserving 64-bit image of a key's bit pattern
static uint64_t image64(uint64_t k, int key_type, bool descending)
{
    if (key_type == GS_KEY_I64) k ^= 0x8000000000000000ull;
    else if (key_type == GS_KEY_F64) k = (k >> 63) ? ~k : (k ^ 0x8000000000000000ull);
    return descending ? ~k : k;
}

template <typename KeyT>
static int test_case(size_t rows, size_t cols, size_t k, bool descending, int spread)
{
    constexpr int kt = gpusort::KeyTraits<KeyT>::type;
    const size_t stride = cols + 3, n = rows * stride;
    std::mt19937_64 rng(1977 + rows * 7 + cols * 3 + k);
    std::vector<uint64_t> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t bits = rng();
        if (spread == 1) bits &= 0xffffffull;                          // below 2^24: five bytes shared
        if (spread == 2) bits &= 0x8000000000000003ull;                // eight values
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
    KeyT *d_in, *d_out;
    unsigned int *d_vin, *d_vout;
    HIP_OK(hipMalloc(&d_in, n * 8)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, rows * k * 8)); HIP_OK(hipMalloc(&d_vout, rows * k * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: every row's stable order on the image
    std::vector<uint32_t> order(rows * cols);
    for (size_t r = 0; r < rows; ++r) {
        uint32_t *o = order.data() + r * cols;
        std::iota(o, o + cols, 0u);
        const uint64_t *row = h_keys.data() + r * stride;
        std::stable_sort(o, o + cols, [&](uint32_t a, uint32_t b) { return image64(row[a], kt, descending) < image64(row[b], kt, descending); });
    }

    int bad = 0;
    std::vector<uint64_t> got_k(rows * k);
    std::vector<unsigned int> got_v(rows * k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_out, 0xee, rows * k * 8)); HIP_OK(hipMemset(d_vout, 0xee, rows * k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t {
            if (mode == 0)
                return descending ? gpusort::DeviceTopKRows::MaxKeys(d_temp, temp_bytes, d_in, d_out, rows, cols, stride, k)
                                  : gpusort::DeviceTopKRows::MinKeys(d_temp, temp_bytes, d_in, d_out, rows, cols, stride, k);
            return descending ? gpusort::DeviceTopKRows::MaxPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k)
                              : gpusort::DeviceTopKRows::MinPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k);
        };
        HIP_OK(run());
        if (temp_bytes == 0) { printf("size query refused rows=%zu cols=%zu k=%zu\n", rows, cols, k); return 1; }
        if (temp_bytes != gs_topk_rows_u64_temp_bytes(rows, cols, k, mode != 0)) { printf("the shim asked another size query\n"); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_out, rows * k * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_vout, rows * k * 4, hipMemcpyDeviceToHost));
        int b = 0;
        for (size_t r = 0; r < rows && !b; ++r)
            for (size_t i = 0; i < k; ++i) {
                const uint32_t col = order[r * cols + i];
                if (got_k[r * k + i] != h_keys[r * stride + col]) b = 1;
                if (mode == 1 && got_v[r * k + i] != h_vals[r * stride + col]) b = 1;
                if (mode == 2 && got_v[r * k + i] != col) b = 1;
            }
        bad += b;
        printf("%s keys, %s, rows=%zu, cols=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(),
               mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments", rows, cols, k, descending ? "max" : "min", spread,
               b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    return bad;
}

template <typename KeyT>
static int test_type()
{
    int bad = 0;
    const size_t shapes[][3] = {{9, 64, 7}, {5, 257, 101}, {3, 1024, 1024}, {3, 1025, 65}, {2, 8192, 1000}, {2, 8197, 1023}, {2, 20000, 50}};
    for (const auto &s : shapes)
        for (int spread = 0; spread < 3; ++spread)
            for (int descending = 0; descending < 2; ++descending) bad += test_case<KeyT>(s[0], s[1], s[2], descending != 0, spread);
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
