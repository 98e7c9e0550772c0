// lsb_halfs.cpp -- DeviceRadixSort on 16-bit float keys through gpusort.hpp: __half keys alone, ascending, and
// (__hip_bfloat16, int) pairs, descending.  The keys are random 16-bit patterns (NaNs of both signs, infinities and both
// zeros among them) next to a block of every special value.  Host check: std::stable_sort of the indices by the key's image
// (GS_KEY_F16 / GS_KEY_BF16 in gpusort.h: bits ^ (sign set ? 0xffff : 0x8000)), complemented when descending; keys must
// match bit for bit and the values must be the indices in that order.
//   usage: lsb_halfs [num_items]     prints PASS and exits 0 iff both cases match
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "gpusort.hpp"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at %s:%d\n", (int)e_, __FILE__, __LINE__); exit(2); } } while (0)

static_assert(sizeof(__half) == 2 && sizeof(__hip_bfloat16) == 2, "16-bit keys");
static_assert(gpusort::KeyTraits<__half>::type == GS_KEY_F16 && gpusort::KeyTraits<_Float16>::type == GS_KEY_F16, "half is GS_KEY_F16");
static_assert(gpusort::KeyTraits<__hip_bfloat16>::type == GS_KEY_BF16, "bfloat16 is GS_KEY_BF16");

static std::vector<unsigned short> make_bits(int n, unsigned seed)
{
    static const unsigned short special[] = {0x0000, 0x8000, 0x7c00, 0xfc00, 0x7f80, 0xff80, 0x7e00, 0xfe00, 0x7fff, 0xffff,
                                             0x7fc1, 0xffc1, 0x0001, 0x8001, 0x3c00, 0xbc00};
    std::mt19937 rng(seed);
    std::vector<unsigned short> b(n);
    for (int i = 0; i < n; ++i) b[i] = (i % 7 == 3) ? special[rng() % 16] : (unsigned short)(rng() & rng());
    return b;
}

static std::vector<int> expected_order(const std::vector<unsigned short> &bits, bool descending)
{
    std::vector<int> idx(bits.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    auto image = [&](int i) {
        const unsigned b = bits[i], im = (b & 0x8000u) ? (b ^ 0xffffu) : (b ^ 0x8000u);
        return descending ? (im ^ 0xffffu) : im;
    };
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return image(a) < image(b); });
    return idx;
}

template <typename KeyT, bool PAIRS>
static int run_case(int n, bool descending, const char *name)
{
    const std::vector<unsigned short> bits = make_bits(n, 77u + (unsigned)n + (PAIRS ? 1u : 0u));
    const std::vector<int> want = expected_order(bits, descending);
    std::vector<int> h_vals(n);
    for (int i = 0; i < n; ++i) h_vals[i] = i;
    KeyT *d_k[2];
    int *d_v[2] = {nullptr, nullptr};
    HIP_OK(hipMalloc(&d_k[0], (size_t)n * 2)); HIP_OK(hipMalloc(&d_k[1], (size_t)n * 2));
    HIP_OK(hipMemcpy(d_k[0], bits.data(), (size_t)n * 2, hipMemcpyHostToDevice));
    if (PAIRS) {
        HIP_OK(hipMalloc(&d_v[0], (size_t)n * 4)); HIP_OK(hipMalloc(&d_v[1], (size_t)n * 4));
        HIP_OK(hipMemcpy(d_v[0], h_vals.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    gpusort::DoubleBuffer<KeyT> keys(d_k[0], d_k[1]);
    gpusort::DoubleBuffer<int> vals(d_v[0], d_v[1]);
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
    auto run = [&]() -> hipError_t {
        if constexpr (PAIRS)
            return descending ? gpusort::DeviceRadixSort::SortPairsDescending(d_temp, temp_bytes, keys, vals, n)
                              : gpusort::DeviceRadixSort::SortPairs(d_temp, temp_bytes, keys, vals, n);
        else
            return descending ? gpusort::DeviceRadixSort::SortKeysDescending(d_temp, temp_bytes, keys, n)
                              : gpusort::DeviceRadixSort::SortKeys(d_temp, temp_bytes, keys, n);
    };
    HIP_OK(run());
    HIP_OK(hipMalloc(&d_temp, temp_bytes ? temp_bytes : 1));
    HIP_OK(run());
    HIP_OK(hipDeviceSynchronize());
    std::vector<unsigned short> out_k(n);
    std::vector<int> out_v(n);
    HIP_OK(hipMemcpy(out_k.data(), keys.Current(), (size_t)n * 2, hipMemcpyDeviceToHost));
    if (PAIRS) HIP_OK(hipMemcpy(out_v.data(), vals.Current(), (size_t)n * 4, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int i = 0; i < n && !bad; ++i) {
        if (out_k[i] != bits[want[i]]) bad = 1;
        if (PAIRS && out_v[i] != want[i]) bad = 1;
    }
    printf("%s, n=%d, %s: %s\n", name, n, descending ? "descending" : "ascending", bad ? "FAIL" : "CORRECT");
    HIP_OK(hipFree(d_k[0])); HIP_OK(hipFree(d_k[1])); HIP_OK(hipFree(d_temp));
    if (PAIRS) { HIP_OK(hipFree(d_v[0])); HIP_OK(hipFree(d_v[1])); }
    return bad;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 300007;
    int bad = 0;
    bad += run_case<__half, false>(n, false, "__half keys");
    bad += run_case<__hip_bfloat16, true>(n, true, "(__hip_bfloat16, int) pairs");
    printf("%s\n", bad ? "FAIL" : "PASS");
    return bad ? 1 : 0;
}
