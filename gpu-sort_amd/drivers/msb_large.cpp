// msb_large.cpp -- gpusort::rdxsrt_unstable_sort_large on device-generated keys: sorts N uniform u32 keys (keys only, or
// with their enumerated positions as values), checks the result on the device and prints one line ending in
// "verified=1" (or "verified=0").  Arguments: N (default 2^24), then "pairs" for key-value pairs.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gpusort.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

int main(int argc, char **argv)
{
    const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : (1ull << 24);
    const bool pairs = argc > 2 && strcmp(argv[2], "pairs") == 0;
    const size_t bytes = sizeof(unsigned int) * (size_t)(n ? n : 1);
    unsigned int *keys, *alt, *vals = nullptr, *vals_alt = nullptr, *orig = nullptr;
    uint64_t *d_res;
    CHECK(hipMalloc(&keys, bytes)); CHECK(hipMalloc(&alt, bytes)); CHECK(hipMalloc(&d_res, 3 * sizeof(uint64_t)));
    CHECK((hipError_t)gs_generate_u32(keys, n, GS_GEN_UNIFORM, 7, 0, 1, 0));
    if (pairs) {
        CHECK(hipMalloc(&vals, bytes)); CHECK(hipMalloc(&vals_alt, bytes)); CHECK(hipMalloc(&orig, bytes));
        CHECK((hipError_t)gs_generate_u32(vals, n, GS_GEN_ENUMERATED, 0, 0, 1, 0));
        CHECK(hipMemcpy(orig, keys, bytes, hipMemcpyDeviceToDevice));
    }
    uint64_t before[3], after[3], pcheck[3] = {0, 0, 0};
    CHECK((hipError_t)gs_check_sorted_u32(keys, n, 0, d_res, 0));
    CHECK(hipMemcpy(before, d_res, sizeof(before), hipMemcpyDeviceToHost));

    hipEvent_t start, stop;
    CHECK(hipEventCreate(&start)); CHECK(hipEventCreate(&stop));
    CHECK(hipEventRecord(start, 0));
    bool ok;
    if (pairs) ok = gpusort::rdxsrt_unstable_sort_large<unsigned int, unsigned int>(keys, vals, n, alt, vals_alt).sorted_keys != nullptr;
    else ok = gpusort::rdxsrt_unstable_sort_large<unsigned int, gpusort::NullType>(keys, nullptr, n, alt, nullptr).sorted_keys != nullptr;
    CHECK(hipEventRecord(stop, 0));
    CHECK(hipEventSynchronize(stop));
    float ms = 0.f;
    CHECK(hipEventElapsedTime(&ms, start, stop));

    CHECK((hipError_t)gs_check_sorted_u32(keys, n, 0, d_res, 0));
    CHECK(hipMemcpy(after, d_res, sizeof(after), hipMemcpyDeviceToHost));
    if (pairs) {
        CHECK((hipError_t)gs_check_pairs_enumerated_u32(orig, keys, vals, n, d_res, 0));
        CHECK(hipMemcpy(pcheck, d_res, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    const bool multiset = before[1] == after[1] && before[2] == after[2];
    const bool verified = ok && after[0] == 0 && multiset && pcheck[0] == 0;
    printf("msb_large: n=%llu %s ms=%.3f inversions=%llu multiset=%s bad_pairs=%llu verified=%d\n", n, pairs ? "pairs" : "keys", ms,
           (unsigned long long)after[0], multiset ? "equal" : "DIFFERENT", (unsigned long long)pcheck[0], verified ? 1 : 0);
    CHECK(hipFree(keys)); CHECK(hipFree(alt)); CHECK(hipFree(d_res));
    if (pairs) { CHECK(hipFree(vals)); CHECK(hipFree(vals_alt)); CHECK(hipFree(orig)); }
    return verified ? 0 : 1;
}
