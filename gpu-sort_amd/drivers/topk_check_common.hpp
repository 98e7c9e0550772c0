// topk_check_common.hpp -- what the topk_*_check programs share: the HIP_OK macro, the printed names of the ten key types, the
// order-preserving image of a key at its width, the generator of a case's input, and the two cases that more than one program
// runs: the rows case against std::stable_sort (topk_rows_narrow / _wide / _anyk_check) and the segmented case against
// gpusort::DeviceTopK (topk_segmented_check / _narrow_check / _anyk_check).  The programs with a reference of their own keep their case and
// take the rest from here; every program states its types, shapes, k's, directions, inputs and seed itself.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
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
template <> const char *name_of<unsigned int>() { return "u32"; }
template <> const char *name_of<int>() { return "i32"; }
template <> const char *name_of<float>() { return "f32"; }
template <> const char *name_of<unsigned long long>() { return "u64"; }
template <> const char *name_of<long long>() { return "i64"; }
template <> const char *name_of<double>() { return "f64"; }

static const char *mode_name(int mode) { return mode == 0 ? "keys" : mode == 1 ? "pairs" : "arguments"; }

// the host word that holds a key's bit pattern
template <size_t Bytes> struct WordOf;
template <> struct WordOf<2> { typedef uint16_t type; };
template <> struct WordOf<4> { typedef unsigned int type; };
template <> struct WordOf<8> { typedef uint64_t type; };
template <typename KeyT> using word_of = typename WordOf<sizeof(KeyT)>::type;

// the order-preserving image of a key's bit pattern at the width of W (the maps stated at the GS_KEY_* enum: the floats with
// negative NaNs first and -0 before +0), complemented when descending
template <typename W>
static W image_of(W k, int key_type, bool descending)
{
    const W sign = (W)((W)1 << (8 * sizeof(W) - 1));
    if (key_type == GS_KEY_I16 || key_type == GS_KEY_I32 || key_type == GS_KEY_I64) k ^= sign;
    else if (key_type == GS_KEY_F16 || key_type == GS_KEY_BF16 || key_type == GS_KEY_F32 || key_type == GS_KEY_F64)
        k = (k & sign) ? (W)~k : (W)(k ^ sign);
    return descending ? (W)~k : k;
}

// The three inputs of a case.  0: random words, with every `every`-th one (0: none) taken in turn from `specials`; 1: (word &
// and1) | or1, shared top bytes, so that the later select rounds work; 2: (word & and2) | or2, a few values, so that the cut
// falls inside a run of equal keys.
template <typename W> struct Inputs { W and1, or1, and2, or2; size_t every; std::vector<W> specials; };

// a case's keys and values: per element one draw truncated to the key word, then one truncated to 32 bits
template <typename W>
static void fill(std::mt19937_64 &rng, int spread, const Inputs<W> &in, std::vector<W> &h_keys, std::vector<unsigned int> &h_vals)
{
    for (size_t i = 0; i < h_keys.size(); ++i) {
        W bits = (W)rng();
        if (spread == 1) bits = (W)((bits & in.and1) | in.or1);
        if (spread == 2) bits = (W)((bits & in.and2) | in.or2);
        if (spread == 0 && in.every && i % in.every == 0) bits = in.specials[(i / in.every) % in.specials.size()];
        h_keys[i] = bits;
        h_vals[i] = (unsigned int)rng();
    }
}

// the four forms of a shim class as one call: the keys form at mode 0, else the pairs form, Max when descending; `shape` is
// what stands between the buffers and the end of the argument list
template <typename D, typename KeyT, typename... Shape>
static hipError_t top(int mode, bool descending, void *d_temp, size_t &temp_bytes, const KeyT *d_in, KeyT *d_out, const unsigned int *vin,
                      unsigned int *d_vout, Shape... shape)
{
    if (mode == 0)
        return descending ? D::MaxKeys(d_temp, temp_bytes, d_in, d_out, shape...) : D::MinKeys(d_temp, temp_bytes, d_in, d_out, shape...);
    return descending ? D::MaxPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, shape...)
                      : D::MinPairs(d_temp, temp_bytes, d_in, d_out, vin, d_vout, shape...);
}

// The rows case: the top k of every row of a matrix at a stride of cols + 3 through the shim class D, in the keys, pairs and
// arguments forms, against the stable sort on the host of every row's image.  The size the shim asks for must be that of
// `size_query`.  Prints one line per form and returns the number that failed.
template <typename D, typename KeyT, typename SizeQuery>
static int rows_case(size_t rows, size_t cols, size_t k, bool descending, int spread, uint64_t seed, const Inputs<word_of<KeyT>> &in,
                     SizeQuery size_query)
{
    typedef word_of<KeyT> W;
    constexpr int kt = gpusort::KeyTraits<KeyT>::type;
    const size_t stride = cols + 3, n = rows * stride;
    std::mt19937_64 rng(seed);
    std::vector<W> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    fill(rng, spread, in, h_keys, h_vals);
    KeyT *d_in, *d_out;
    unsigned int *d_vin, *d_vout;
    HIP_OK(hipMalloc(&d_in, n * sizeof(W))); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_out, rows * k * sizeof(W))); HIP_OK(hipMalloc(&d_vout, rows * k * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * sizeof(W), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));

    // the reference: every row's stable order on the image
    std::vector<uint32_t> order(rows * cols);
    for (size_t r = 0; r < rows; ++r) {
        uint32_t *o = order.data() + r * cols;
        std::iota(o, o + cols, 0u);
        const W *row = h_keys.data() + r * stride;
        std::stable_sort(o, o + cols, [&](uint32_t a, uint32_t b) { return image_of(row[a], kt, descending) < image_of(row[b], kt, descending); });
    }

    int bad = 0;
    std::vector<W> got_k(rows * k);
    std::vector<unsigned int> got_v(rows * k);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_out, 0xee, rows * k * sizeof(W))); HIP_OK(hipMemset(d_vout, 0xee, rows * k * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        HIP_OK((top<D>(mode, descending, d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k)));
        if (temp_bytes == 0) { printf("size query refused rows=%zu cols=%zu k=%zu\n", rows, cols, k); return 1; }
        if (temp_bytes != size_query(rows, cols, k, mode != 0)) { printf("the shim asked another size query\n"); return 1; }
        HIP_OK(hipMalloc(&d_temp, temp_bytes));
        HIP_OK((top<D>(mode, descending, d_temp, temp_bytes, d_in, d_out, vin, d_vout, rows, cols, stride, k)));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(d_temp));
        HIP_OK(hipMemcpy(got_k.data(), d_out, rows * k * sizeof(W), hipMemcpyDeviceToHost));
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
        printf("%s keys, %s, rows=%zu, cols=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(), mode_name(mode), rows, cols, k,
               descending ? "max" : "min", spread, b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_vout));
    return bad;
}

// The ragged set of the segmented case, as int32 begins and ends into n keys: every list of the classify kernel (empty, one
// wave of each class, one workgroup, chunked), laid out in the order listed with a gap of 5 between them, so that segments
// start at odd elements, but the longest one first in memory; then a repeat, two segments that need clamping and one whose
// end lies before its begin.  more: two further segments in front of the longest, of 8193 elements and of 3 tiles + 1.
static size_t ragged_segments(std::vector<int> &begin, std::vector<int> &end, bool more = false)
{
    std::vector<size_t> lens = {0, 1, 64, 65, 256, 300, 512, 700, 1024, 1025, 5000, 8192, 8193, 20000};
    if (more) { lens.push_back(8193); lens.push_back(3 * 8192 + 1); }
    lens.push_back(40000);
    const size_t S0 = lens.size();
    std::vector<size_t> at(S0);
    at[S0 - 1] = 3;
    size_t n = 3 + lens[S0 - 1] + 5;
    for (size_t s = 0; s + 1 < S0; ++s) { at[s] = n; n += lens[s] + 5; }
    for (size_t s = 0; s < S0; ++s) { begin.push_back((int)at[s]); end.push_back((int)(at[s] + lens[s])); }
    begin.push_back(begin[5]); end.push_back(end[5]);               // a repeated segment
    begin.push_back(-7); end.push_back(40);                         // clamped below: [0, 40)
    begin.push_back((int)n - 30); end.push_back((int)n + 100);      // clamped above: the last 30
    begin.push_back(500); end.push_back(100);                       // end < begin: empty
    return n;
}

// The segmented case: ragged_segments() through gpusort::DeviceTopKSegmented in one call and segment by segment through
// gpusort::DeviceTopK at k = min(k, length), in the keys, pairs and arguments forms.  Every segment's first count elements and
// the counts must agree bit for bit, the slots behind a segment's count must keep their fill, and the size the shim asks for
// must be that of `size_query`.  Prints one line per form and returns the number that failed.  D: the shim class of the one
// call (gpusort::DeviceTopKSegmentedAnyK in topk_segmented_anyk_check, which also asks for the longer ragged set).
template <typename KeyT, typename SizeQuery, typename D = gpusort::DeviceTopKSegmented>
static int segmented_case(size_t k, bool descending, int spread, uint64_t seed, const Inputs<word_of<KeyT>> &in, SizeQuery size_query,
                          D = D(), bool more = false)
{
    typedef word_of<KeyT> W;
    std::vector<int> begin, end;
    const size_t n = ragged_segments(begin, end, more), S = begin.size();
    std::mt19937_64 rng(seed);
    std::vector<W> h_keys(n);
    std::vector<unsigned int> h_vals(n);
    fill(rng, spread, in, h_keys, h_vals);
    KeyT *d_in, *d_seg, *d_one;
    unsigned int *d_vin, *d_seg_v, *d_one_v, *d_counts;
    int *d_begin, *d_end;
    HIP_OK(hipMalloc(&d_in, n * sizeof(W))); HIP_OK(hipMalloc(&d_vin, n * 4));
    HIP_OK(hipMalloc(&d_seg, S * k * sizeof(W))); HIP_OK(hipMalloc(&d_seg_v, S * k * 4));
    HIP_OK(hipMalloc(&d_one, S * k * sizeof(W))); HIP_OK(hipMalloc(&d_one_v, S * k * 4));
    HIP_OK(hipMalloc(&d_counts, S * 4)); HIP_OK(hipMalloc(&d_begin, S * 4)); HIP_OK(hipMalloc(&d_end, S * 4));
    HIP_OK(hipMemcpy(d_in, h_keys.data(), n * sizeof(W), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_vin, h_vals.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_begin, begin.data(), S * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_end, end.data(), S * 4, hipMemcpyHostToDevice));

    int bad = 0;
    std::vector<W> got_k(S * k), want_k(S * k);
    std::vector<unsigned int> got_v(S * k), want_v(S * k), counts(S);
    for (int mode = 0; mode < 3; ++mode) {   // keys, pairs, arguments
        HIP_OK(hipMemset(d_seg, 0xee, S * k * sizeof(W))); HIP_OK(hipMemset(d_seg_v, 0xee, S * k * 4));
        HIP_OK(hipMemset(d_one, 0xee, S * k * sizeof(W))); HIP_OK(hipMemset(d_one_v, 0xee, S * k * 4));
        HIP_OK(hipMemset(d_counts, 0xee, S * 4));
        const unsigned int *vin = mode == 1 ? d_vin : nullptr;
        void *d_temp = nullptr;
        size_t temp_bytes = 0;
        auto run = [&]() -> hipError_t {
            return top<D>(mode, descending, d_temp, temp_bytes, d_in, d_seg, vin, d_seg_v, d_counts, n, (uint32_t)S, d_begin, d_end, k);
        };
        HIP_OK(run());
        if (temp_bytes == 0) { printf("size query refused n=%zu S=%zu k=%zu\n", n, S, k); return 1; }
        if (temp_bytes != size_query(n, (uint32_t)S, k, mode != 0)) { printf("the shim asked another size query n=%zu S=%zu k=%zu\n", n, S, k); return 1; }
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
            d_temp = nullptr; temp_bytes = 0;
            auto one = [&]() -> hipError_t {
                return top<gpusort::DeviceTopK>(mode, descending, d_temp, temp_bytes, d_in + lo, d_one + s * k, vin ? vin + lo : nullptr,
                                                d_one_v + s * k, len, kept);
            };
            HIP_OK(one());
            HIP_OK(hipMalloc(&d_temp, temp_bytes));
            HIP_OK(one());
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipFree(d_temp));
        }
        HIP_OK(hipMemcpy(got_k.data(), d_seg, S * k * sizeof(W), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_v.data(), d_seg_v, S * k * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_k.data(), d_one, S * k * sizeof(W), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(want_v.data(), d_one_v, S * k * 4, hipMemcpyDeviceToHost));
        // the reference buffers keep their fill behind every count, so whole-buffer equality also proves the unwritten slots
        if (memcmp(got_k.data(), want_k.data(), S * k * sizeof(W)) != 0) b = 1;
        if (mode && memcmp(got_v.data(), want_v.data(), S * k * 4) != 0) b = 1;
        if (!mode) for (size_t i = 0; i < S * k; ++i) if (got_v[i] != 0xeeeeeeeeu) b = 1;
        bad += b;
        printf("%s keys, %s, segments=%zu, items=%zu, k=%zu, %s, input %d: %s\n", name_of<KeyT>(), mode_name(mode), S, n, k,
               descending ? "max" : "min", spread, b ? "FAIL" : "CORRECT");
    }
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_vin)); HIP_OK(hipFree(d_seg)); HIP_OK(hipFree(d_seg_v));
    HIP_OK(hipFree(d_one)); HIP_OK(hipFree(d_one_v)); HIP_OK(hipFree(d_counts)); HIP_OK(hipFree(d_begin)); HIP_OK(hipFree(d_end));
    return bad;
}
