"""Sorts above 2^32 keys through gs_msb_sort_large_u32, checked on the device (tests/test_msb_large_gpu.py::test_above_2p32).

    python tools/large_check.py CASE...     CASE: uniform | pairs | equal | const_top | uniform_2p33

Keys: 0 adjacent inversions and the same multiset (sum and xor of splitmix64 over the keys, gs_check_sorted_u32) as the
input.  Pairs: every value is a fixed function of its key, f(k) = k * 0x9E3779B1 + 0x7F4A7C15 mod 2^32, checked chunk-wise
as v == f(k) after the sort.  Prints "<case> -> OK" per case; exits 1 at the first failure.  Each case runs once."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

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


def run(case, dev):
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
