// lsb_large.cpp -- gpusort::DeviceRadixSortLarge (the stable sort above 2^32 elements) on device-generated keys, checked on
// the device; prints one line ending in "verified=1" (or "verified=0").  Arguments: N (default 2^24), the mode, then options:
//   keys   (default) uniform u32 keys;
//   pairs  u32 keys with their enumerated positions as u32 values (N < 2^32: the positions are 32-bit);
//   u64    uniform u64 keys;
//   rowid  u32 keys of 16 distinct values with their u64 row ids (a stable argsort: ties everywhere);
//   u8 | i16            uniform unsigned char / short keys (gs_lsb_sort_narrow_large underneath);
//   u8rowid | i16rowid  such keys of 16 distinct values with their u64 row ids;
//   desc   descending;   B:E   sort on key bits [B, E) only.
// Checks: the keys are in the sort's order on the bits (gs_check_sorted_stable) and the same multiset as the input (sum and
// xor of splitmix64); rowid: equal sort keys keep increasing row ids and every row id names an equal input key
// (gs_check_pairs_enumerated_wide), which together make the output THE stable sort; pairs: every value names an equal key.
// The narrow modes are checked by kernels of this file: the keys in the sort's order on the bits, the output's per-value counts
// equal to the input's, and with row ids: equal sort keys keep increasing row ids, every row id is < N and names an equal input key.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "gpusort.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void row_ids_kernel(unsigned long long *out, unsigned long long n)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = i;
}

__global__ void low_bits_kernel(unsigned int *keys, unsigned long long n, unsigned int mask)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) keys[i] &= mask;
}

static dim3 grid_for(unsigned long long n)
{
    const unsigned long long blocks = (n + 255) / 256;
    return dim3(blocks < 8192 ? (unsigned)(blocks ? blocks : 1) : 8192u);
}

template <typename K, typename V>
static hipError_t sort(void *keys, void *alt, void *vals, void *vals_alt, unsigned long long n, int bb, int eb, bool desc, int &sel,
                       float &ms)
{
    gpusort::DoubleBuffer<K> dk((K *)keys, (K *)alt);
    gpusort::DoubleBuffer<V> dv((V *)vals, (V *)vals_alt);
    size_t bytes = 0;
    const bool pairs = !std::is_same<V, gpusort::NullType>::value;
    if (pairs) gpusort::DeviceRadixSortLarge::SortPairs(nullptr, bytes, dk, dv, n, bb, eb);
    else gpusort::DeviceRadixSortLarge::SortKeys(nullptr, bytes, dk, n, bb, eb);
    void *temp;
    CHECK(hipMalloc(&temp, bytes ? bytes : 1));
    hipEvent_t start, stop;
    CHECK(hipEventCreate(&start)); CHECK(hipEventCreate(&stop));
    CHECK(hipEventRecord(start, 0));
    hipError_t e;
    if (pairs) e = desc ? gpusort::DeviceRadixSortLarge::SortPairsDescending(temp, bytes, dk, dv, n, bb, eb)
                        : gpusort::DeviceRadixSortLarge::SortPairs(temp, bytes, dk, dv, n, bb, eb);
    else e = desc ? gpusort::DeviceRadixSortLarge::SortKeysDescending(temp, bytes, dk, n, bb, eb)
                  : gpusort::DeviceRadixSortLarge::SortKeys(temp, bytes, dk, n, bb, eb);
    CHECK(hipEventRecord(stop, 0));
    CHECK(hipEventSynchronize(stop));
    CHECK(hipEventElapsedTime(&ms, start, stop));
    CHECK(hipFree(temp));
    sel = dk.selector;
    if (pairs && dv.selector != sel) return hipErrorUnknown;
    return e;
}

// ---- the narrow modes: 8- and 16-bit keys
template <typename K>
__global__ void narrow_hist_kernel(const K *keys, unsigned long long n, unsigned long long *hist)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    typedef typename std::make_unsigned<K>::type U;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        atomicAdd(&hist[(U)keys[i]], 1ull);
}

__global__ void narrow_hist_diff_kernel(const unsigned long long *a, const unsigned long long *b, unsigned int bins, unsigned long long *res)
{
    for (unsigned int i = blockIdx.x * blockDim.x + threadIdx.x; i < bins; i += gridDim.x * blockDim.x)
        if (a[i] != b[i]) atomicAdd(res, 1ull);
}

// res[0]: adjacent positions out of the sort's order on the bits (with row ids: also equal sort keys whose row ids do not
// increase); res[1]: row ids >= n or naming an input key that differs from the key that came out
template <typename K>
__global__ void narrow_check_kernel(const K *out, const unsigned long long *rid, const K *orig, unsigned long long n, int bb, int eb,
                                    int desc, unsigned long long *res)
{
    typedef typename std::make_unsigned<K>::type U;
    const unsigned int sign = std::is_signed<K>::value ? 1u << (8 * sizeof(K) - 1) : 0u, mask = (1u << (eb - bb)) - 1u;
    auto sk = [&](K k) { const unsigned int m = ((((unsigned int)(U)k) ^ sign) >> bb) & mask; return desc ? ~m & mask : m; };
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad = 0, badp = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (i) {
            const unsigned int a = sk(out[i - 1]), b = sk(out[i]);
            if (a > b || (rid && a == b && rid[i - 1] >= rid[i])) ++bad;
        }
        if (rid && (rid[i] >= n || orig[rid[i]] != out[i])) ++badp;
    }
    if (bad) atomicAdd(&res[0], bad);
    if (badp) atomicAdd(&res[1], badp);
}

template <typename K>
static int run_narrow(unsigned long long n, const char *mode, bool rowid, bool desc, int bb, int eb)
{
    const size_t kbytes = sizeof(K) * (n ? n : 1), words = (kbytes + 3) / 4;
    const unsigned int bins = 1u << (8 * sizeof(K));
    void *keys, *alt, *orig, *vals = nullptr, *vals_alt = nullptr;
    unsigned long long *hist, *d_res;
    CHECK(hipMalloc(&keys, words * 4)); CHECK(hipMalloc(&alt, kbytes)); CHECK(hipMalloc(&orig, kbytes));
    CHECK(hipMalloc(&hist, 2 * bins * sizeof(unsigned long long))); CHECK(hipMalloc(&d_res, 3 * sizeof(unsigned long long)));
    CHECK(hipMemset(hist, 0, 2 * bins * sizeof(unsigned long long))); CHECK(hipMemset(d_res, 0, 3 * sizeof(unsigned long long)));
    CHECK((hipError_t)gs_generate_u32((uint32_t *)keys, words, GS_GEN_UNIFORM, 7, 0, 1, 0));
    if (rowid) {   // 16 distinct values, the sign bit among their bits
        hipLaunchKernelGGL(low_bits_kernel, grid_for(words), dim3(256), 0, 0, (unsigned int *)keys, words,
                           sizeof(K) == 1 ? 0xF0F0F0F0u : 0xF000F000u);
        CHECK(hipGetLastError());
        CHECK(hipMalloc(&vals, 8 * (n ? n : 1))); CHECK(hipMalloc(&vals_alt, 8 * (n ? n : 1)));
        hipLaunchKernelGGL(row_ids_kernel, grid_for(n), dim3(256), 0, 0, (unsigned long long *)vals, n);
        CHECK(hipGetLastError());
    }
    CHECK(hipMemcpy(orig, keys, kbytes, hipMemcpyDeviceToDevice));
    int sel = 0;
    float ms = 0.f;
    const hipError_t e = rowid ? sort<K, unsigned long long>(keys, alt, vals, vals_alt, n, bb, eb, desc, sel, ms)
                               : sort<K, gpusort::NullType>(keys, alt, nullptr, nullptr, n, bb, eb, desc, sel, ms);
    const bool ok = e == hipSuccess;
    if (!ok) fprintf(stderr, "lsb_large: sort returned %s\n", hipGetErrorString(e));
    const K *out_k = (const K *)(sel ? alt : keys);
    const unsigned long long *out_v = (const unsigned long long *)(sel ? vals_alt : vals);
    hipLaunchKernelGGL(narrow_hist_kernel<K>, grid_for(n), dim3(256), 0, 0, (const K *)orig, n, hist);
    hipLaunchKernelGGL(narrow_hist_kernel<K>, grid_for(n), dim3(256), 0, 0, out_k, n, hist + bins);
    hipLaunchKernelGGL(narrow_hist_diff_kernel, dim3(64), dim3(256), 0, 0, hist, hist + bins, bins, d_res + 2);
    hipLaunchKernelGGL(narrow_check_kernel<K>, grid_for(n), dim3(256), 0, 0, out_k, rowid ? out_v : nullptr, (const K *)orig, n, bb, eb,
                       desc ? 1 : 0, d_res);
    CHECK(hipGetLastError());
    unsigned long long res[3];
    CHECK(hipMemcpy(res, d_res, sizeof(res), hipMemcpyDeviceToHost));
    const bool same = res[2] == 0;
    const bool verified = ok && res[0] == 0 && same && res[1] == 0 && (n == 0 || sel == 1);   // the result is in the alternates
    printf("lsb_large: n=%llu %s%s bits=%d:%d ms=%.3f selector=%d disorder=%llu multiset=%s bad_pairs=%llu verified=%d\n", n, mode,
           desc ? " desc" : "", bb, eb, ms, sel, res[0], same ? "equal" : "DIFFERENT", res[1], verified ? 1 : 0);
    CHECK(hipFree(keys)); CHECK(hipFree(alt)); CHECK(hipFree(orig)); CHECK(hipFree(hist)); CHECK(hipFree(d_res));
    if (vals) { CHECK(hipFree(vals)); CHECK(hipFree(vals_alt)); }
    return verified ? 0 : 1;
}

int main(int argc, char **argv)
{
    const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : (1ull << 24);
    const char *mode = argc > 2 ? argv[2] : "keys";
    {
        const bool u8 = strcmp(mode, "u8") == 0 || strcmp(mode, "u8rowid") == 0, i16 = strcmp(mode, "i16") == 0 || strcmp(mode, "i16rowid") == 0;
        if (u8 || i16) {
            const int bits = u8 ? 8 : 16;
            bool desc = false;
            int bb = 0, eb = bits;
            for (int a = 3; a < argc; ++a) {
                if (strcmp(argv[a], "desc") == 0) desc = true;
                else if (sscanf(argv[a], "%d:%d", &bb, &eb) != 2 || bb < 0 || eb > bits || bb > eb) {
                    fprintf(stderr, "lsb_large: bad option %s (desc | B:E)\n", argv[a]);
                    return 2;
                }
            }
            const bool rowid = strstr(mode, "rowid") != nullptr;
            return u8 ? run_narrow<unsigned char>(n, mode, rowid, desc, bb, eb) : run_narrow<short>(n, mode, rowid, desc, bb, eb);
        }
    }
    const bool pairs = strcmp(mode, "pairs") == 0, u64 = strcmp(mode, "u64") == 0, rowid = strcmp(mode, "rowid") == 0;
    if (!pairs && !u64 && !rowid && strcmp(mode, "keys") != 0) {
        fprintf(stderr, "lsb_large: unknown mode %s (keys | pairs | u64 | rowid | u8 | i16 | u8rowid | i16rowid)\n", mode);
        return 2;
    }
    const int kb = u64 ? 8 : 4;
    bool desc = false;
    int bb = 0, eb = 8 * kb;
    for (int a = 3; a < argc; ++a) {
        if (strcmp(argv[a], "desc") == 0) desc = true;
        else if (sscanf(argv[a], "%d:%d", &bb, &eb) != 2 || bb < 0 || eb > 8 * kb || bb > eb) {
            fprintf(stderr, "lsb_large: bad option %s (desc | B:E)\n", argv[a]);
            return 2;
        }
    }
    const int key_type = u64 ? GS_KEY_U64 : GS_KEY_U32;
    const size_t kbytes = (size_t)kb * (n ? n : 1), vbytes = (size_t)(rowid ? 8 : 4) * (n ? n : 1);
    void *keys, *alt, *vals = nullptr, *vals_alt = nullptr, *orig = nullptr;
    uint64_t *d_res;
    CHECK(hipMalloc(&keys, kbytes)); CHECK(hipMalloc(&alt, kbytes)); CHECK(hipMalloc(&d_res, 3 * sizeof(uint64_t)));
    CHECK((hipError_t)gs_generate_u32((uint32_t *)keys, u64 ? 2 * n : n, GS_GEN_UNIFORM, 7, 0, 1, 0));   // u64 keys: 2n u32 words
    if (rowid) {
        hipLaunchKernelGGL(low_bits_kernel, grid_for(n), dim3(256), 0, 0, (unsigned int *)keys, n, 0xF0000000u);
        CHECK(hipGetLastError());
    }
    if (pairs || rowid) {
        CHECK(hipMalloc(&vals, vbytes)); CHECK(hipMalloc(&vals_alt, vbytes)); CHECK(hipMalloc(&orig, kbytes));
        if (rowid) {
            hipLaunchKernelGGL(row_ids_kernel, grid_for(n), dim3(256), 0, 0, (unsigned long long *)vals, n);
            CHECK(hipGetLastError());
        } else {
            CHECK((hipError_t)gs_generate_u32((uint32_t *)vals, n, GS_GEN_ENUMERATED, 0, 0, 1, 0));
        }
        CHECK(hipMemcpy(orig, keys, kbytes, hipMemcpyDeviceToDevice));
    }
    // sum / xor of splitmix64 over the keys (result[1], [2]; the order word is not used)
    auto multiset = [&](const void *k, uint64_t out[3]) {
        if (u64) CHECK((hipError_t)gs_check_sorted_u64((const uint64_t *)k, n, GS_KEY_U64, d_res, 0));
        else CHECK((hipError_t)gs_check_sorted_u32((const uint32_t *)k, n, 0, d_res, 0));
        CHECK(hipMemcpy(out, d_res, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    };
    uint64_t before[3], after[3], disorder = 0, pcheck[3] = {0, 0, 0};
    multiset(keys, before);

    int sel = 0;
    float ms = 0.f;
    hipError_t e;
    if (pairs) e = sort<unsigned int, unsigned int>(keys, alt, vals, vals_alt, n, bb, eb, desc, sel, ms);
    else if (rowid) e = sort<unsigned int, unsigned long long>(keys, alt, vals, vals_alt, n, bb, eb, desc, sel, ms);
    else if (u64) e = sort<unsigned long long, gpusort::NullType>(keys, alt, nullptr, nullptr, n, bb, eb, desc, sel, ms);
    else e = sort<unsigned int, gpusort::NullType>(keys, alt, nullptr, nullptr, n, bb, eb, desc, sel, ms);
    const bool ok = e == hipSuccess;
    if (!ok) fprintf(stderr, "lsb_large: sort returned %s\n", hipGetErrorString(e));
    const void *out_k = sel ? alt : keys;
    const void *out_v = sel ? vals_alt : vals;

    multiset(out_k, after);
    CHECK((hipError_t)gs_check_sorted_stable(out_k, rowid ? (const uint64_t *)out_v : nullptr, n, kb, key_type, bb, eb, desc ? 1 : 0,
                                             d_res, 0));
    CHECK(hipMemcpy(&disorder, d_res, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (pairs) {
        CHECK((hipError_t)gs_check_pairs_enumerated_u32((const uint32_t *)orig, (const uint32_t *)out_k, (const uint32_t *)out_v, n,
                                                        d_res, 0));
        CHECK(hipMemcpy(pcheck, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    } else if (rowid) {
        CHECK((hipError_t)gs_check_pairs_enumerated_wide(orig, out_k, (const uint64_t *)out_v, n, 4, d_res, 0));
        CHECK(hipMemcpy(pcheck, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    const bool same = before[1] == after[1] && before[2] == after[2];
    const bool verified = ok && disorder == 0 && same && pcheck[0] == 0;
    printf("lsb_large: n=%llu %s%s bits=%d:%d ms=%.3f selector=%d disorder=%llu multiset=%s bad_pairs=%llu verified=%d\n", n, mode,
           desc ? " desc" : "", bb, eb, ms, sel, (unsigned long long)disorder, same ? "equal" : "DIFFERENT",
           (unsigned long long)pcheck[0], verified ? 1 : 0);
    CHECK(hipFree(keys)); CHECK(hipFree(alt)); CHECK(hipFree(d_res));
    if (vals) { CHECK(hipFree(vals)); CHECK(hipFree(vals_alt)); CHECK(hipFree(orig)); }
    return verified ? 0 : 1;
}
