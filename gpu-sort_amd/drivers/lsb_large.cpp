// lsb_large.cpp -- gpusort::DeviceRadixSortLarge (the stable sort above 2^32 elements) on device-generated keys, checked on
// the device; prints one line ending in "verified=1" (or "verified=0").  Arguments: N (default 2^24), the mode, then options:
//   keys   (default) uniform u32 keys;
//   pairs  u32 keys with their enumerated positions as u32 values (N < 2^32: the positions are 32-bit);
//   u64    uniform u64 keys;
//   rowid  u32 keys of 16 distinct values with their u64 row ids (a stable argsort: ties everywhere);
//   desc   descending;   B:E   sort on key bits [B, E) only.
// Checks: the keys are in the sort's order on the bits (gs_check_sorted_stable) and the same multiset as the input (sum and
// xor of splitmix64); rowid: equal sort keys keep increasing row ids and every row id names an equal input key
// (gs_check_pairs_enumerated_wide), which together make the output THE stable sort; pairs: every value names an equal key.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

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

int main(int argc, char **argv)
{
    const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : (1ull << 24);
    const char *mode = argc > 2 ? argv[2] : "keys";
    const bool pairs = strcmp(mode, "pairs") == 0, u64 = strcmp(mode, "u64") == 0, rowid = strcmp(mode, "rowid") == 0;
    if (!pairs && !u64 && !rowid && strcmp(mode, "keys") != 0) {
        fprintf(stderr, "lsb_large: unknown mode %s (keys | pairs | u64 | rowid)\n", mode);
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
