// msb_large.cpp -- gpusort::rdxsrt_unstable_sort_large on device-generated keys, checked on the device; prints one line
// ending in "verified=1" (or "verified=0").  Arguments: N (default 2^24), then the mode:
//   keys   (default) uniform u32 keys;
//   pairs  uniform u32 keys with their enumerated positions as u32 values;
//   u64    uniform u64 keys;
//   rowid  uniform u32 keys with their u64 row ids as values (an argsort);
//   host   uniform u32 keys through the host-pointer convenience rdxsrt_unstable_sort_keys (above UINT_MAX keys it takes
//          the large sort), the sorted copy moved back to the device for the check.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpusort.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

__global__ void row_ids_kernel(unsigned long long *out, unsigned long long n)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = i;
}

int main(int argc, char **argv)
{
    const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : (1ull << 24);
    const char *mode = argc > 2 ? argv[2] : "keys";
    const bool pairs = strcmp(mode, "pairs") == 0, u64 = strcmp(mode, "u64") == 0, rowid = strcmp(mode, "rowid") == 0,
               host = strcmp(mode, "host") == 0;
    if (!pairs && !u64 && !rowid && !host && strcmp(mode, "keys") != 0) {
        fprintf(stderr, "msb_large: unknown mode %s (keys | pairs | u64 | rowid | host)\n", mode);
        return 2;
    }
    const size_t kbytes = (u64 ? 8 : 4) * (size_t)(n ? n : 1), vbytes = (rowid ? 8 : 4) * (size_t)(n ? n : 1);
    void *keys, *alt = nullptr, *vals = nullptr, *vals_alt = nullptr, *orig = nullptr;
    uint64_t *d_res;
    CHECK(hipMalloc(&keys, kbytes)); CHECK(hipMalloc(&d_res, 3 * sizeof(uint64_t)));
    if (!host) CHECK(hipMalloc(&alt, kbytes));
    // u64 keys: 2n uniform u32 words
    CHECK((hipError_t)gs_generate_u32((uint32_t *)keys, u64 ? 2 * n : n, GS_GEN_UNIFORM, 7, 0, 1, 0));
    if (pairs || rowid) {
        CHECK(hipMalloc(&vals, vbytes)); CHECK(hipMalloc(&vals_alt, vbytes)); CHECK(hipMalloc(&orig, kbytes));
        if (rowid) {
            const unsigned long long blocks = (n + 255) / 256;
            hipLaunchKernelGGL(row_ids_kernel, dim3(blocks < 8192 ? (unsigned)(blocks ? blocks : 1) : 8192u), dim3(256), 0, 0,
                               (unsigned long long *)vals, n);
            CHECK(hipGetLastError());
        } else {
            CHECK((hipError_t)gs_generate_u32((uint32_t *)vals, n, GS_GEN_ENUMERATED, 0, 0, 1, 0));
        }
        CHECK(hipMemcpy(orig, keys, kbytes, hipMemcpyDeviceToDevice));
    }
    auto check_keys = [&](uint64_t out[3]) {
        if (u64) CHECK((hipError_t)gs_check_sorted_u64((const uint64_t *)keys, n, GS_KEY_U64, d_res, 0));
        else CHECK((hipError_t)gs_check_sorted_u32((const uint32_t *)keys, n, 0, d_res, 0));
        CHECK(hipMemcpy(out, d_res, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    };
    uint64_t before[3], after[3], pcheck[3] = {0, 0, 0};
    check_keys(before);

    std::vector<unsigned int> h_keys, h_out;
    if (host) {
        h_keys.resize(n);
        h_out.resize(n);
        CHECK(hipMemcpy(h_keys.data(), keys, 4 * n, hipMemcpyDeviceToHost));
        CHECK(hipMemset(keys, 0, kbytes));   // (the sorted copy must come through the convenience)
    }
    hipEvent_t start, stop;
    CHECK(hipEventCreate(&start)); CHECK(hipEventCreate(&stop));
    CHECK(hipEventRecord(start, 0));
    bool ok = true;
    if (pairs)
        ok = gpusort::rdxsrt_unstable_sort_large<unsigned int, unsigned int>((unsigned int *)keys, (unsigned int *)vals, n,
                                                                            (unsigned int *)alt, (unsigned int *)vals_alt).sorted_keys != nullptr;
    else if (rowid)
        ok = gpusort::rdxsrt_unstable_sort_large<unsigned int, unsigned long long>(
                 (unsigned int *)keys, (unsigned long long *)vals, n, (unsigned int *)alt, (unsigned long long *)vals_alt).sorted_keys != nullptr;
    else if (u64)
        ok = gpusort::rdxsrt_unstable_sort_large<unsigned long long, gpusort::NullType>((unsigned long long *)keys, nullptr, n,
                                                                                        (unsigned long long *)alt, nullptr).sorted_keys != nullptr;
    else if (host)
        rdxsrt_unstable_sort_keys<unsigned int>(h_keys.data(), n, h_out.data());   // (a failure reports itself; the check sees it)
    else
        ok = gpusort::rdxsrt_unstable_sort_large<unsigned int, gpusort::NullType>((unsigned int *)keys, nullptr, n, (unsigned int *)alt,
                                                                                  nullptr).sorted_keys != nullptr;
    CHECK(hipEventRecord(stop, 0));
    CHECK(hipEventSynchronize(stop));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, start, stop));
    if (host) CHECK(hipMemcpy(keys, h_out.data(), 4 * n, hipMemcpyHostToDevice));

    check_keys(after);
    if (pairs) {
        CHECK((hipError_t)gs_check_pairs_enumerated_u32((const uint32_t *)orig, (const uint32_t *)keys, (const uint32_t *)vals, n, d_res, 0));
        CHECK(hipMemcpy(pcheck, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    } else if (rowid) {
        CHECK((hipError_t)gs_check_pairs_enumerated_wide(orig, keys, (const uint64_t *)vals, n, 4, d_res, 0));
        CHECK(hipMemcpy(pcheck, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    const bool multiset = before[1] == after[1] && before[2] == after[2];
    const bool verified = ok && after[0] == 0 && multiset && pcheck[0] == 0;
    printf("msb_large: n=%llu %s ms=%.3f inversions=%llu multiset=%s bad_pairs=%llu verified=%d\n", n, mode, ms,
           (unsigned long long)after[0], multiset ? "equal" : "DIFFERENT", (unsigned long long)pcheck[0], verified ? 1 : 0);
    CHECK(hipFree(keys)); CHECK(hipFree(d_res));
    if (alt) CHECK(hipFree(alt));
    if (vals) { CHECK(hipFree(vals)); CHECK(hipFree(vals_alt)); CHECK(hipFree(orig)); }
    return verified ? 0 : 1;
}
