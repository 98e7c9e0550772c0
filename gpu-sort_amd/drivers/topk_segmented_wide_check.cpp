// topk_segmented_wide_check.cpp -- gpusort::DeviceTopKSegmented on 64-bit keys (gs_topk_segmented_u64) against std::stable_sort
// of every segment on the host, compiled against gpusort.hpp: for each of the six lists of the classify kernel (the four wave
// classes, one workgroup, chunked) a call whose segments all fall into that list -- laid out with a gap of 5, with an empty
// segment, a repeat and offsets that need clamping --, in the keys, pairs and arguments forms, Min and Max, for unsigned long
// long / long long / double keys; every segment's first count elements and the counts must agree bit for bit, and the slots
// behind a segment's count must keep their fill.
//   usage: topk_segmented_wide_check     prints OK and exits 0 iff every case matches; stops at the first mismatch
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

// the order-preserving image of a key's bit pattern (the maps stated at the GS_KEY_* enum), complemented when descending
template <typename T> static uint64_t image_of(uint64_t bits, bool descending);
template <> uint64_t image_of<unsigned long long>(uint64_t b, bool d) { return d ? ~b : b; }
template <> uint64_t image_of<long long>(uint64_t b, bool d) { b ^= 0x8000000000000000ull; return d ? ~b : b; }
template <> uint64_t image_of<double>(uint64_t b, bool d)
{
    b = (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
    return d ? ~b : b;
}

static const uint64_t SPECIALS[] = {0x7ff8000000000001ull, 0xfff8000000000001ull, 0xffffffffffffffffull, 0x7ff0000000000000ull,
                                    0xfff0000000000000ull, 0x0000000000000000ull, 0x8000000000000000ull, 0x0000000000000001ull,
                                    0x7fffffffffffffffull, 0x3ff0000000000000ull, 0xbff0000000000000ull};

static const size_t CLASS_LENS[6][4] = {{1, 40, 64, 0}, {65, 200, 256, 0}, {257, 400, 512, 0}, {513, 900, 1024, 0},
                                        {1025, 3000, 8192, 0}, {8193, 20000, 0, 0}};

template <typename KeyT>
static int test_case(int cls, int mode, bool descending, size_t k, int spread)
{
    static_assert(sizeof(KeyT) == 8, "64-bit keys");
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
    for (size_t i = 0; i < n; ++i) {
        uint64_t bits = rng();
        if (spread == 1) bits &= 0xffffffull;                                 // integers below 2^24: five bytes are constant
        if (spread == 2) bits = (bits & 0x8000000000000003ull) | 0x3ff0000000000000ull;   // eight values: the cut falls inside a tie run
        if (spread == 0 && (i % 3) == 0) bits = SPECIALS[(i / 3) % (sizeof(SPECIALS) / sizeof(SPECIALS[0]))];
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
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
        using D = gpusort::DeviceTopKSegmented;
        if (mode == 0)
            return descending ? D::MaxKeys(d_temp, temp_bytes, d_in, d_out, d_counts, n, (uint32_t)S, d_begin, d_end, k)
                              : D::MinKeys(d_temp, temp_bytes, d_in, d_out, d_counts, n, (uint32_t)S, d_begin, d_end, k);
        return descending ? D::MaxPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, d_counts, n, (uint32_t)S, d_begin, d_end, k)
                          : D::MinPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, d_counts, n, (uint32_t)S, d_begin, d_end, k);
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
            return image_of<KeyT>(h_keys[lo + x], descending) < image_of<KeyT>(h_keys[lo + y], descending);
        });
        for (size_t i = 0; i < kept; ++i) {
            want_k[s * k + i] = h_keys[lo + order[i]];
            if (mode) want_v[s * k + i] = mode == 1 ? h_vals[lo + order[i]] : order[i];
        }
    }
    // the reference buffers keep the fill behind every count, so whole-buffer equality also proves the unwritten slots
    if (memcmp(got_k.data(), want_k.data(), S * k * 8) != 0) b = 1;
    if (memcmp(got_v.data(), want_v.data(), S * k * 4) != 0) b = 1;
    printf("%s keys, %s, list %d, segments=%zu, items=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(),
           mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments", cls, S, n, k, descending ? "max" : "min", spread, b ? "FAIL" : "CORRECT");
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
