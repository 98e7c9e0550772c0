// topk_rows_anyk_check.cpp -- gpusort::DeviceTopKRowsAnyK against std::stable_sort, compiled against gpusort.hpp: for shapes on
// both paths (one workgroup per row up to 8192 columns, the radix select over all rows above), k below and above what the
// segmented finish sorts in one workgroup, and unsigned int / int / float keys, take the top k of every row in one call, in the
// keys, pairs and arguments forms, Min and Max; every row must be, bit for bit, the first k of the host's stable sort of that
// row on the key type's order-preserving image.  The rows sit at a stride of num_cols + 3.
//   usage: topk_rows_anyk_check     prints OK and exits 0 iff every case matches
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "gpusort.hpp"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); exit(2); } } while (0)

template <typename T> struct Kind;
template <> struct Kind<unsigned int> { static const char *name() { return "u32"; } static unsigned int image(unsigned int b) { return b; } };
template <> struct Kind<int> { static const char *name() { return "i32"; } static unsigned int image(unsigned int b) { return b ^ 0x80000000u; } };
template <> struct Kind<float> {
    static const char *name() { return "f32"; }
    static unsigned int image(unsigned int b) { return (b & 0x80000000u) ? ~b : b ^ 0x80000000u; }   // negative NaNs first, -0 before +0
};

template <typename KeyT>
static int test_case(size_t rows, size_t cols, size_t k, bool descending, int spread)
{
    const size_t stride = cols + 3, n = rows * stride;
    std::mt19937_64 rng(1977 + rows * 7 + cols * 3 + k);
    std::vector<unsigned int> h_keys(n), h_vals(n);
    for (size_t i = 0; i < n; ++i) {
        unsigned int bits = (unsigned int)rng();
        if (spread == 1) bits = (bits & 0x000fffffu) | 0x3f000000u;   // twelve shared top bits: the later rounds work
        if (spread == 2) bits &= 0x80000003u;                          // eight values: the cut falls inside a run of equal keys
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
    KeyT *d_in, *d_out;
    unsigned int *d_vin, *d_vout;
    HIP_OK(hipMalloc(&d_in, n * 4)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, rows * k * 4)); HIP_OK(hipMalloc(&d_vout, rows * k * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: every row's stable order on the image
    std::vector<unsigned int> order(rows * cols);
    for (size_t r = 0; r < rows; ++r) {
        unsigned int *o = order.data() + r * cols;
        const unsigned int *row = h_keys.data() + r * stride;
        std::iota(o, o + cols, 0u);
        std::stable_sort(o, o + cols, [&](unsigned int a, unsigned int b) {
            const unsigned int ia = Kind<KeyT>::image(row[a]) ^ (descending ? ~0u : 0u), ib = Kind<KeyT>::image(row[b]) ^ (descending ? ~0u : 0u);
            return ia < ib;
        });
    }

    int bad = 0;
    std::vector<unsigned int> got_k(rows * k), got_v(rows * k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_out, 0xee, rows * k * 4)); HIP_OK(hipMemset(d_vout, 0xee, rows * k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t {
            if (mode == 0)
                return descending ? gpusort::DeviceTopKRowsAnyK::MaxKeys(d_temp, temp_bytes, d_in, d_out, rows, cols, stride, k)
                                  : gpusort::DeviceTopKRowsAnyK::MinKeys(d_temp, temp_bytes, d_in, d_out, rows, cols, stride, k);
            return descending ? gpusort::DeviceTopKRowsAnyK::MaxPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k)
                              : gpusort::DeviceTopKRowsAnyK::MinPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k);
        };
        HIP_OK(run());
        if (temp_bytes == 0) { printf("size query refused rows=%zu cols=%zu k=%zu\n", rows, cols, k); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_out, rows * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_vout, rows * k * 4, hipMemcpyDeviceToHost));
        int b = 0;
        for (size_t r = 0; r < rows && !b; ++r)
            for (size_t i = 0; i < k; ++i) {
                const unsigned int c = order[r * cols + i];
                if (got_k[r * k + i] != h_keys[r * stride + c]) b = 1;
                if (mode == 1 && got_v[r * k + i] != h_vals[r * stride + c]) b = 1;
                if (mode == 2 && got_v[r * k + i] != c) b = 1;
            }
        bad += b;
        printf("%s keys, %s, rows=%zu, cols=%zu, k=%zu, %s, input %d: %s\n", Kind<KeyT>::name(),
               mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments", rows, cols, k, descending ? "max" : "min", spread,
               b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    return bad;
}

template <typename KeyT>
static int test_type(int first)
{
    int bad = 0;
    const size_t shapes[][3] = {{3, 1025, 1025}, {2, 8192, 3000}, {2, 8193, 2000}, {3, 40000, 9000}, {2, 70001, 20000}, {1, 33000, 33000}};
    int i = first;
    for (const auto &s : shapes) {
        bad += test_case<KeyT>(s[0], s[1], s[2], (i & 1) != 0, i % 3);
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
