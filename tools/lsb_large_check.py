"""The stable sort above 2^32 elements (gs_lsb_sort_large, through DeviceRadixSortLarge), checked on the device
(tests/test_lsb_large_gpu.py::test_above_2p32).

    python tools/lsb_large_check.py CASE...
    CASE: keys_2p33    2^33 uniform u32 keys, ascending: in order, and the input's multiset (sum and xor of splitmix64);
          rowid        u32 keys of 16 distinct values with their u64 row ids, 2^32 + 2^21 + 7 elements, ascending;
          rowid_desc   the same, descending;
          i64_bits     as many i64 keys with u64 row ids, sorted descending on bits [5, 61), where they take 64 distinct values;
          pairs32      the rowid keys with u32 values (the row ids mod 2^32): keys and values equal the rowid run's result,
                       keys bit for bit and values to the low 32 bits (the stable result is unique).
The row-id cases are exact: gs_check_sorted_stable (the sort's order on the bits, and row ids strictly increasing inside
every run of equal sort keys) and gs_check_pairs_enumerated_wide (every row id names a bitwise-equal input key) together
make the output THE stable sort of the input.  Inputs are built chunk by chunk (a whole-tensor torch.arange of this size
has returned wrong entries).  Prints "<case> -> OK" per case; exits 1 at the first failure.  Each case runs once, and frees
its tensors before the next one (pairs32 takes over what rowid kept: run it right after rowid)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd._lib import check  # noqa: E402
from gpu_sort_amd.datagen import check_pairs_enumerated_wide  # noqa: E402

CHUNK = 1 << 28
N_ODD = (1 << 32) + (1 << 21) + 7
I64_MASK = 0xF7000000000000FF           # bits 56-58 and 5-7 inside [5, 61): 64 sort keys; bits 0-4 and 60-63 outside
_rowid_result = {}                      # the ascending rowid run's sorted keys and row ids mod 2^32, for pairs32


def _signed(x, bits):
    return x - (1 << bits) if x >= 1 << (bits - 1) else x


def check_sorted_stable(keys, rowids, n, kt, bb, eb, desc):
    res = torch.zeros(1, dtype=torch.int64, device=keys.device)
    check(gs.lib.gs_check_sorted_stable(keys.data_ptr(), rowids.data_ptr() if rowids is not None else None, n, keys.element_size(),
                                        kt, bb, eb, int(desc), res.data_ptr(), None), "gs_check_sorted_stable")
    return int(res.item())


def _row_ids(n, dev):
    v = torch.empty(n, dtype=torch.int64, device=dev)
    for i in range(0, n, CHUNK):
        torch.arange(i, min(i + CHUNK, n), dtype=torch.int64, out=v[i:i + CHUNK])
    return v


def _rowid_keys(n, dev):
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    gs.generate_uniform_keys(n, seed=23, out=keys)
    for i in range(0, n, CHUNK):
        keys[i:i + CHUNK].bitwise_and_(_signed(0xF0000000, 32))     # 16 distinct keys: runs of 2^28 ties
    return keys


def _sort(k0, v0, n, kt, bb, eb, desc):
    """DeviceRadixSortLarge on (k0, v0) with fresh alternates; -> (sorted keys, sorted values, host seconds)."""
    dk = gs.DoubleBuffer(k0, torch.empty_like(k0))
    dv = gs.DoubleBuffer(v0, torch.empty_like(v0)) if v0 is not None else None
    L = gs.DeviceRadixSortLarge
    if dv is None:
        fn = L.SortKeysDescending if desc else L.SortKeys
        args = (dk, n, bb, eb, None, kt)
    else:
        fn = L.SortPairsDescending if desc else L.SortPairs
        args = (dk, dv, n, bb, eb, None, kt)
    nbytes = fn(None, 0, *args)
    temp = torch.empty(nbytes, dtype=torch.uint8, device=k0.device)
    torch.cuda.synchronize()
    t0 = time.time()
    fn(temp, nbytes, *args)
    torch.cuda.synchronize()
    dt = time.time() - t0
    passes = (eb - bb + 7) // 8
    assert dk.selector == passes % 2, (dk.selector, passes)
    out_k, out_v = dk.Current(), (dv.Current() if dv is not None else None)
    dk.d_buffers[dk.selector ^ 1] = None
    if dv is not None:
        dv.d_buffers[dv.selector ^ 1] = None
    return out_k, out_v, dt


def run(case, dev):
    if case == "keys_2p33":
        n = 1 << 33
        keys = torch.empty(n, dtype=torch.int32, device=dev)
        gs.generate_uniform_keys(n, seed=17, out=keys)
        _, s0, x0 = gs.check_sorted(keys, n)
        out, _, dt = _sort(keys, None, n, gs.GS_KEY_U32, 0, 32, False)
        del keys
        disorder = check_sorted_stable(out, None, n, gs.GS_KEY_U32, 0, 32, False)
        _, s1, x1 = gs.check_sorted(out, n)
        ok = disorder == 0 and (s1, x1) == (s0, x0)
        print("%s n=%d: %.3f s (host wall), disorder=%d multiset=%s -> %s"
              % (case, n, dt, disorder, "equal" if (s1, x1) == (s0, x0) else "DIFFERENT", "OK" if ok else "FAIL"), flush=True)
        return ok

    n = N_ODD
    if case in ("rowid", "rowid_desc", "i64_bits"):
        if case == "i64_bits":
            keys = torch.empty(n, dtype=torch.int64, device=dev)
            gs.generate_uniform_keys(2 * n, seed=29, out=keys.view(torch.int32))
            for i in range(0, n, CHUNK):
                keys[i:i + CHUNK].bitwise_and_(_signed(I64_MASK, 64))
            kt, bb, eb, desc = gs.GS_KEY_I64, 5, 61, True
        else:
            keys = _rowid_keys(n, dev)
            kt, bb, eb, desc = gs.GS_KEY_U32, 0, 32, case == "rowid_desc"
        orig = torch.empty_like(keys)
        for i in range(0, n, CHUNK):
            orig[i:i + CHUNK].copy_(keys[i:i + CHUNK])
        out_k, out_v, dt = _sort(keys, _row_ids(n, dev), n, kt, bb, eb, desc)
        del keys
        disorder = check_sorted_stable(out_k, out_v, n, kt, bb, eb, desc)
        bad, vsum = check_pairs_enumerated_wide(orig, out_k, out_v, n)
        ok = disorder == 0 and bad == 0 and vsum == (n * (n - 1) // 2) % (1 << 64)
        if case == "rowid" and ok:
            _rowid_result["keys"] = out_k
            _rowid_result["lo"] = out_v
            for i in range(0, n, CHUNK):
                out_v[i:i + CHUNK].bitwise_and_(0xFFFFFFFF)
        print("%s n=%d: %.3f s (host wall), disorder=%d bad_row_ids=%d -> %s"
              % (case, n, dt, disorder, bad, "OK" if ok else "FAIL"), flush=True)
        return ok

    if case == "pairs32":
        if "keys" not in _rowid_result and not run("rowid", dev):
            return False
        ref_k, ref_lo = _rowid_result.pop("keys"), _rowid_result.pop("lo")
        keys = _rowid_keys(n, dev)
        vals = torch.empty(n, dtype=torch.int32, device=dev)
        gs.generate_enumerated_values(n, out=vals)                   # (u32) position: the row ids mod 2^32
        out_k, out_v, dt = _sort(keys, vals, n, gs.GS_KEY_U32, 0, 32, False)
        del keys, vals
        bad_k = bad_v = 0
        for i in range(0, n, CHUNK):
            bad_k += int((out_k[i:i + CHUNK] != ref_k[i:i + CHUNK]).sum().item())
            bad_v += int(((out_v[i:i + CHUNK].to(torch.int64) & 0xFFFFFFFF) != ref_lo[i:i + CHUNK]).sum().item())
        ok = bad_k == 0 and bad_v == 0
        print("%s n=%d: %.3f s (host wall), keys_differing=%d values_differing=%d -> %s"
              % (case, n, dt, bad_k, bad_v, "OK" if ok else "FAIL"), flush=True)
        return ok
    raise SystemExit("unknown case %s" % case)


def main():
    dev = torch.device("cuda:0")
    for case in sys.argv[1:]:
        ok = run(case, dev)
        torch.cuda.empty_cache()
        if not ok:
            sys.exit(1)


if __name__ == "__main__":
    main()
