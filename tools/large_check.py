"""Sorts above 2^32 keys through gs_msb_sort_large_u32 and gs_msb_sort_large_wide, checked on the device
(tests/test_msb_large_gpu.py::test_above_2p32, tests/test_msb_large_wide_gpu.py::test_above_2p32).

    python tools/large_check.py CASE...
    CASE: uniform | pairs | equal | const_top | uniform_2p33    (u32 keys, gs_msb_sort_large_u32)
          u64 | u64_equal | rowid                               (gs_msb_sort_large_wide)

Keys: 0 adjacent inversions and the same multiset (sum and xor of splitmix64 over the keys, gs_check_sorted_u32 /
gs_check_sorted_u64) as the input.  Pairs: every value is a fixed function of its key, f(k) = k * 0x9E3779B1 + 0x7F4A7C15
mod 2^32, checked chunk-wise as v == f(k) after the sort.  rowid: u32 keys with their u64 row ids as values, every row id
checked to point at an equal input key (gs_check_pairs_enumerated_wide) and their sum to be n(n-1)/2.  u64_equal: all keys
equal, so the range is split down to the last byte.  Prints "<case> -> OK" per case; exits 1 at the first failure.  Each
case runs once."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd.datagen import check_pairs_enumerated_wide, check_sorted_u64  # noqa: E402

CHUNK = 1 << 28
N_ODD = (1 << 32) + (1 << 21) + 7


def _value_of(k):
    """f(k) on an int32 chunk holding u32 keys, as int32 bit patterns."""
    x = ((k.to(torch.int64) & 0xFFFFFFFF) * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF
    return torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32)


def _fill(case, n, dev):
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    if case == "equal":
        keys.fill_(0x1234567)
    else:
        gs.generate_uniform_keys(n, seed=17, out=keys)
        if case == "const_top":
            for i in range(0, n, CHUNK):
                c = keys[i:i + CHUNK]
                c.bitwise_and_(0x00FFFFFF).bitwise_or_(0x6B000000)
    return keys


def run_wide(case, dev):
    """u64: 2^32 + 2^21 + 7 uniform u64 keys; u64_equal: the same count of equal u64 keys; rowid: as many u32 keys with their
    u64 row ids (about 112 GiB of device memory)."""
    n = N_ODD
    rowid = case == "rowid"
    if rowid:
        keys = gs.generate_uniform_keys(n, seed=23, device=dev)
        orig = torch.empty_like(keys)
        vals = torch.empty(n, dtype=torch.int64, device=dev)
        for i in range(0, n, CHUNK):   # (chunk by chunk, like every elementwise op on these tensors)
            orig[i:i + CHUNK].copy_(keys[i:i + CHUNK])
            torch.arange(i, min(i + CHUNK, n), dtype=torch.int64, out=vals[i:i + CHUNK])
        vals_alt = torch.empty(n, dtype=torch.int64, device=dev)
        _, sum0, xor0 = gs.check_sorted(keys, n)
    else:
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        if case == "u64_equal":
            for i in range(0, n, CHUNK):
                keys[i:i + CHUNK].fill_(0x0123456789ABCDEF)
        else:
            gs.generate_uniform_keys(2 * n, seed=29, out=keys.view(torch.int32))
        vals = vals_alt = None
        _, sum0, xor0 = check_sorted_u64(keys, n)
    alt = torch.empty_like(keys)
    torch.cuda.synchronize()
    t0 = time.time()
    seq = gs.rdxsrt_unstable_sort_large_wide(keys, vals, n, alt, vals_alt, key_type=gs.GS_KEY_U32 if rowid else gs.GS_KEY_U64)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert seq.sorted_keys is keys
    del alt
    inv, sum1, xor1 = gs.check_sorted(keys, n) if rowid else check_sorted_u64(keys, n)
    ok = inv == 0 and sum1 == sum0 and xor1 == xor0
    bad_vals = 0
    if rowid:
        bad_vals, vsum = check_pairs_enumerated_wide(orig, keys, vals, n)
        ok = ok and bad_vals == 0 and vsum == (n * (n - 1) // 2) % (1 << 64)
    print("%s n=%d: %.3f s (host wall), inversions=%d multiset=%s bad_values=%d -> %s"
          % (case, n, dt, inv, "equal" if (sum1, xor1) == (sum0, xor0) else "DIFFERENT", bad_vals, "OK" if ok else "FAIL"), flush=True)
    return ok


def run(case, dev):
    if case in ("u64", "u64_equal", "rowid"):
        return run_wide(case, dev)
    n = {"uniform": N_ODD, "pairs": N_ODD, "equal": (1 << 32) + 3, "const_top": (1 << 32) + (1 << 20),
         "uniform_2p33": 1 << 33}[case]
    pairs = case == "pairs"
    keys = _fill(case, n, dev)
    alt = torch.empty(n, dtype=torch.int32, device=dev)
    vals = vals_alt = None
    if pairs:
        vals = torch.empty(n, dtype=torch.int32, device=dev)
        for i in range(0, n, CHUNK):
            vals[i:i + CHUNK] = _value_of(keys[i:i + CHUNK])
        vals_alt = torch.empty(n, dtype=torch.int32, device=dev)
    _, sum0, xor0 = gs.check_sorted(keys, n)
    torch.cuda.synchronize()
    t0 = time.time()
    seq = gs.rdxsrt_unstable_sort_large(keys, vals, n, alt, vals_alt)
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert seq.sorted_keys is keys
    inv, sum1, xor1 = gs.check_sorted(keys, n)
    ok = inv == 0 and sum1 == sum0 and xor1 == xor0
    bad_vals = 0
    if pairs:
        for i in range(0, n, CHUNK):
            bad_vals += int((vals[i:i + CHUNK] != _value_of(keys[i:i + CHUNK])).sum().item())
        ok = ok and bad_vals == 0
    print("%s n=%d: %.3f s (host wall), inversions=%d multiset=%s bad_values=%d -> %s"
          % (case, n, dt, inv, "equal" if (sum1, xor1) == (sum0, xor0) else "DIFFERENT", bad_vals, "OK" if ok else "FAIL"), flush=True)
    return ok


def main():
    dev = torch.device("cuda:0")
    for case in sys.argv[1:]:
        ok = run(case, dev)
        torch.cuda.empty_cache()
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
