// topk_segmented_narrow_check.cpp -- gpusort::DeviceTopKSegmented on 16-bit keys (gs_topk_segmented_u16) against
// gpusort::DeviceTopK (gs_topk_u16), compiled against gpusort.hpp: the ragged set of topk_segmented_check (every list of the
// classify kernel: empty, one wave of each class, one workgroup, chunked; a gap of 5, so that segments start at odd elements;
// a repeat, clamped offsets, a segment in reverse place) is taken in one call and segment by segment with DeviceTopK at
// k = min(k, length), in the keys, pairs and arguments forms, Min and Max, for unsigned short / short / _Float16 /
// __hip_bfloat16 keys; every segment's first count elements and the counts must agree bit for bit, and the slots behind a
// segment's count must keep their fill.
//   usage: topk_segmented_narrow_check     prints OK and exits 0 iff every case matches; stops at the first mismatch
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include "gpusort.hpp"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); exit(2); } } while (0)

template <typename T> static const char *name_of();
template <> const char *name_of<unsigned short>() { return "u16"; }
template <> const char *name_of<short>() { return "i16"; }
template <> const char *name_of<_Float16>() { return "f16"; }
template <> const char *name_of<__hip_bfloat16>() { return "bf16"; }

static const unsigned int FILL = 0xeeeeeeeeu;

template <typename KeyT>
static int test_case(size_t k, bool descending, int spread)
{
    static_assert(sizeof(KeyT) == 2, "16-bit keys");
    // lengths in the order the segments are listed; laid out with a gap of 5 between them, the last one first in memory
    const size_t lens[] = {0, 1, 64, 65, 256, 300, 512, 700, 1024, 1025, 5000, 8192, 8193, 20000, 40000};
    const size_t S0 = sizeof(lens) / sizeof(lens[0]);
    std::vector<int> begin, end;
    size_t n = 0;
    {
        std::vector<size_t> at(S0);
        at[S0 - 1] = 3; n = 3 + lens[S0 - 1] + 5;                       // the longest segment sits first, at an odd element
        for (size_t s = 0; s + 1 < S0; ++s) { at[s] = n; n += lens[s] + 5; }
        for (size_t s = 0; s < S0; ++s) { begin.push_back((int)at[s]); end.push_back((int)(at[s] + lens[s])); }
        begin.push_back(begin[5]); end.push_back(end[5]);               // a repeated segment
        begin.push_back(-7); end.push_back(40);                         // clamped below: [0, 40)
        begin.push_back((int)n - 30); end.push_back((int)n + 100);      // clamped above: the last 30
        begin.push_back(500); end.push_back(100);                       // end < begin: empty
    }
    const size_t S = begin.size();
    std::mt19937_64 rng(5231 + k * 3 + spread);
    std::vector<uint16_t> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    for (size_t i = 0; i < n; ++i) {
        uint16_t bits = (uint16_t)rng();
        if (spread == 1) bits = (uint16_t)((bits & 0x00ffu) | 0x3f00u);   // one top byte: the second select round decides
        if (spread == 2) bits &= 0x8003u;                                  // eight values: the cut falls inside a run of equal keys
        if (spread == 0 && (i & 15) == 0) bits = (uint16_t)(0xffffu * ((i >> 4) & 1));   // both ends of the image, the pad's too
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
    KeyT *d_in, *d_seg, *d_one;
    unsigned int *d_vin, *d_seg_v, *d_one_v, *d_counts;
    int *d_begin, *d_end;
    HIP_OK(hipMalloc(&d_in, n * 2)); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_seg, S * k * 2)); HIP_OK(hipMalloc(&d_seg_v, S * k * 4));
    HIP_OK(hipMalloc(&d_one, S * k * 2)); HIP_OK(hipMalloc(&d_one_v, S * k * 4));
    HIP_OK(hipMalloc(&d_counts, S * 4)); HIP_OK(hipMalloc(&d_begin, S * 4)); HIP_OK(hipMalloc(&d_end, S * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_begin, begin.data(), S * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_end, end.data(), S * 4, hipMemcpyHostToDevice));

    int bad = 0;
    std::vector<uint16_t> got_k(S * k), want_k(S * k);
    std::vector<unsigned int> got_v(S * k), want_v(S * k), counts(S);
    for (int mode = 0; mode < 3 && !bad; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_seg, 0xee, S * k * 2)); HIP_OK(hipMemset(d_seg_v, 0xee, S * k * 4));
        HIP_OK(hipMemset(d_one, 0xee, S * k * 2)); HIP_OK(hipMemset(d_one_v, 0xee, S * k * 4));
        HIP_OK(hipMemset(d_counts, 0xee, S * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t {
            using D = gpusort::DeviceTopKSegmented;
            if (mode == 0)
                return descending ? D::MaxKeys(d_temp, temp_bytes, d_in, d_seg, d_counts, n, (uint32_t)S, d_begin, d_end, k)
                                  : D::MinKeys(d_temp, temp_bytes, d_in, d_seg, d_counts, n, (uint32_t)S, d_begin, d_end, k);
            return descending ? D::MaxPairs(d_temp, temp_bytes, d_in, d_seg, vin, d_seg_v, d_counts, n, (uint32_t)S, d_begin, d_end, k)
                              : D::MinPairs(d_temp, temp_bytes, d_in, d_seg, vin, d_seg_v, d_counts, n, (uint32_t)S, d_begin, d_end, k);
        };
        HIP_OK(run());
        if (temp_bytes == 0 || temp_bytes != gs_topk_segmented_u16_temp_bytes(n, (uint32_t)S, k, mode != 0)) {
            printf("the shim asked another size query n=%zu S=%zu k=%zu\n", n, S, k);
            return 1;
        }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        // the reference: DeviceTopK on each clamped segment alone, with k = min(k, length)
        int b = 0;
        HIP_OK(hipMemcpy(counts.data(), d_counts, S * 4, hipMemcpyDeviceToHost));
        for (size_t s = 0; s < S; ++s) {
            const long lo = std::max<long>(begin[s], 0), hi = std::min<long>(end[s], (long)n);
            const size_t len = hi > lo ? (size_t)(hi - lo) : 0, kept = std::min(k, len);
            if (counts[s] != kept) b = 1;
            if (kept == 0) continue;
            const KeyT *ki = d_in + lo;
            const unsigned int *vi = vin ? vin + lo : nullptr;
            d_temp = nullptr; temp_bytes = 0;
            auto one = [&]() -> hipError_t {
                if (mode == 0)
                    return descending ? gpusort::DeviceTopK::MaxKeys(d_temp, temp_bytes, ki, d_one + s * k, len, kept)
                                      : gpusort::DeviceTopK::MinKeys(d_temp, temp_bytes, ki, d_one + s * k, len, kept);
                return descending ? gpusort::DeviceTopK::MaxPairs(d_temp, temp_bytes, ki, d_one + s * k, vi, d_one_v + s * k, len, kept)
                                  : gpusort::DeviceTopK::MinPairs(d_temp, temp_bytes, ki, d_one + s * k, vi, d_one_v + s * k, len, kept);
            };
            HIP_OK(one());
            HIP_OK(hipMalloc(&d_temp, temp_bytes));
            HIP_OK(one());
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipFree(d_temp));
        }
        HIP_OK(hipMemcpy(got_k.data(), d_seg, S * k * 2, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_seg_v, S * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_k.data(), d_one, S * k * 2, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_v.data(), d_one_v, S * k * 4, hipMemcpyDeviceToHost));
        // the reference buffers keep their fill behind every count, so whole-buffer equality also proves the unwritten slots
        if (memcmp(got_k.data(), want_k.data(), S * k * 2) != 0) b = 1;
        if (mode && memcmp(got_v.data(), want_v.data(), S * k * 4) != 0) b = 1;
        if (!mode) for (size_t i = 0; i < S * k; ++i) if (got_v[i] != FILL) b = 1;
        bad += b;
        printf("%s keys, %s, segments=%zu, items=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(),
               mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments", S, n, k, descending ? "max" : "min", spread,
               b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_seg)); HIP_OK(hipFree(d_seg_v));
    HIP_OK(hipFree(d_one)); HIP_OK(hipFree(d_one_v)); HIP_OK(hipFree(d_counts)); HIP_OK(hipFree(d_begin)); HIP_OK(hipFree(d_end));
    return bad;
}

// k = 1, an odd k inside a class and the odd k below the maximum; both directions at every k; the three inputs in turn
template <typename KeyT>
static int test_type()
{
    const size_t ks[] = {1, 51, 1023};
    int i = 0;
    for (size_t k : ks)
        for (int desc = 0; desc < 2; ++desc, ++i)
            if (test_case<KeyT>(k, desc != 0, i % 3)) return 1;
    return 0;
}

int main()
{
    int bad = test_type<unsigned short>();
    if (!bad) bad = test_type<short>();
    if (!bad) bad = test_type<_Float16>();
    if (!bad) bad = test_type<__hip_bfloat16>();
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
