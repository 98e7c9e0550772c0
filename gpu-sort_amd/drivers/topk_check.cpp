// topk_check.cpp -- gpusort::DeviceTopK against gpusort::DeviceRadixSort, compiled against gpusort.hpp: for a few sizes and
// unsigned int / int / float keys, sort a copy of the input with the stable pair sort and take the top k of the original,
// in all four call shapes (Min / Max, keys / pairs with the input indices as values); the first k must agree bit for bit.
//   usage: topk_check [num_items]     prints OK and exits 0 iff every case matches
#include "topk_check_common.hpp"

template <typename KeyT>
static int test_case(size_t n, size_t k, bool descending, int spread)
{
    std::mt19937_64 rng(4321 + n * 3 + k);
    std::vector<KeyT> h_keys(n);
    for (auto &x : h_keys) {
        unsigned int bits = (unsigned int)rng();
        if (spread == 1) bits = (bits & 0x00ffffffu) | 0x3f000000u;   // one top byte: the input re-read route
        if (spread == 2) bits &= 0x80000003u;                          // eight values: long runs of equal keys
        memcpy(&x, &bits, 4);
    }
    std::vector<unsigned int> h_idx(n);
    for (size_t i = 0; i < n; ++i) h_idx[i] = (unsigned int)i;

    KeyT *d_in, *d_sorted, *d_top;
    unsigned int *d_idx, *d_idx_sorted, *d_top_idx;
    HIP_OK(hipMalloc(&d_in, n * 4)); HIP_OK(hipMalloc(&d_sorted, n * 4)); HIP_OK(hipMalloc(&d_top, k * 4));
    HIP_OK(hipMalloc(&d_idx, n * 4)); HIP_OK(hipMalloc(&d_idx_sorted, n * 4)); HIP_OK(hipMalloc(&d_top_idx, k * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_idx, h_idx.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: the stable pair sort of the whole input (plain-pointer form; descending through the DoubleBuffer form)
    void *d_temp = nullptr;
    size_t temp_bytes = 0;
    if (!descending) {
        HIP_OK(gpusort::DeviceRadixSort::SortPairs(d_temp, temp_bytes, d_in, d_sorted, d_idx, d_idx_sorted, (int)n));
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(gpusort::DeviceRadixSort::SortPairs(d_temp, temp_bytes, d_in, d_sorted, d_idx, d_idx_sorted, (int)n));
    } else {
        HIP_OK(hipMemcpy(d_sorted, d_in, n * 4, hipMemcpyDeviceToDevice));
        HIP_OK(hipMemcpy(d_idx_sorted, d_idx, n * 4, hipMemcpyDeviceToDevice));
        KeyT *d_alt; unsigned int *d_ialt;
        HIP_OK(hipMalloc(&d_alt, n * 4)); HIP_OK(hipMalloc(&d_ialt, n * 4));
        gpusort::DoubleBuffer<KeyT> kb(d_sorted, d_alt);
        gpusort::DoubleBuffer<unsigned int> vb(d_idx_sorted, d_ialt);
        HIP_OK(gpusort::DeviceRadixSort::SortPairsDescending(d_temp, temp_bytes, kb, vb, (int)n));
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(gpusort::DeviceRadixSort::SortPairsDescending(d_temp, temp_bytes, kb, vb, (int)n));
        HIP_OK(hipDeviceSynchronize());
        if (kb.Current() != d_sorted) {
            HIP_OK(hipMemcpy(d_sorted, kb.Current(), n * 4, hipMemcpyDeviceToDevice));
            HIP_OK(hipMemcpy(d_idx_sorted, vb.Current(), n * 4, hipMemcpyDeviceToDevice));
        }
        HIP_OK(hipFree(d_alt)); HIP_OK(hipFree(d_ialt));
    }
    HIP_OK(hipDeviceSynchronize());
    std::vector<KeyT> want_k(k);
    std::vector<unsigned int> want_i(k);
    HIP_OK(hipMemcpy(want_k.data(), d_sorted, k * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(want_i.data(), d_idx_sorted, k * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_temp));

    int bad = 0;
    std::vector<KeyT> got_k(k);
    std::vector<unsigned int> got_i(k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_top, 0xee, k * 4));
        HIP_OK(hipMemset(d_top_idx, 0xee, k * 4));
        const unsigned int *vin = mode == 1 ? d_idx : nullptr;
        d_temp = nullptr; temp_bytes = 0;
        auto run = [&]() -> hipError_t {
            return top<gpusort::DeviceTopK>(mode, descending, d_temp, temp_bytes, d_in, d_top, vin, d_top_idx, n, k);
        };
        HIP_OK(run());
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK(run());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got_k.data(), d_top, k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_i.data(), d_top_idx, k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(d_temp));
        int b = memcmp(got_k.data(), want_k.data(), k * 4) != 0;
        if (mode && memcmp(got_i.data(), want_i.data(), k * 4) != 0) b = 1;
        bad += b;
        printf("%s keys, %s, n=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(), mode_name(mode), n, k, descending ? "max" : "min", spread,
               b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_sorted)); HIP_OK(hipFree(d_top));
    HIP_OK(hipFree(d_idx)); HIP_OK(hipFree(d_idx_sorted)); HIP_OK(hipFree(d_top_idx));
    return bad;
}

template <typename KeyT>
static int test_type(size_t max_items)
{
    int bad = 0;
    const size_t sizes[] = {max_items, 65537, 17409, 1000, 1};
    for (size_t n : sizes) {
        if (n > max_items) continue;
        const size_t ks[] = {1, 100, n / 3, n};
        for (size_t k : ks) {
            if (k < 1 || k > n) continue;
            for (int spread = 0; spread < 3; ++spread) {
                bad += test_case<KeyT>(n, k, false, spread);
                bad += test_case<KeyT>(n, k, true, spread);
            }
        }
    }
    return bad;
}

int main(int argc, char **argv)
{
    const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 300007;
    int bad = 0;
    bad += test_type<unsigned int>(n);
    bad += test_type<int>(n);
    bad += test_type<float>(n);
    printf("%s\n", bad ? "SOME CASES FAILED" : "OK");
    return bad ? 1 : 0;
}
