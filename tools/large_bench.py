"""Device-timed MSB sort above 2^32 keys (gs_msb_sort_large_u32, gs_msb_sort_large_wide) against the plain MSB sorts at 2^31
in the same process.

    python tools/large_bench.py [--reps R] [--warmup W] [--profile] [--cases msb_2p31,keys_2p33,pairs_2p32]

Cases: msb_2p31 = gs_msb_sort_u32 on 2^31 uniform keys (the yardstick), keys_2p33 = 2^33 uniform keys, pairs_2p32 =
2^32 + 2^21 uniform keys with 32-bit values (each a fixed function of its key, checked after the sort).  The wide element
types (gs_msb_sort_large_wide), each on 2^32 + 2^21 elements with its yardstick gs_msb_sort_wide on 2^31 elements of the
same types: u64_2p32 (u64 keys; yardstick u64_2p31), rowid_2p32 (u32 keys with u64 row ids; rowid_2p31) and
u64pairs_2p32 (u64 keys with u64 row ids; u64pairs_2p31).  Row ids are checked with gs_check_pairs_enumerated_wide against
a copy of the input keys; `ratio_<case>` is a case's rate over its yardstick's.  Every repetition sorts freshly generated keys; ms is the median of the
repetitions, timed with events on the sort's stream (host waits of the large sort included).  Prints one JSON line;
`verified` = 0 inversions and the input's multiset (gs_check_sorted_u32) after the last repetition.  --profile adds the
per-kernel device times (gs_profile_*) of one more repetition of each case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd.msb import rdxsrt_unstable_sort_wide  # noqa: E402
from large_check import CHUNK, _value_of  # noqa: E402

from gpu_sort_amd.datagen import check_pairs_enumerated_wide, check_sorted_u64  # noqa: E402

SIZES = {"msb_2p31": 1 << 31, "keys_2p33": 1 << 33, "pairs_2p32": (1 << 32) + (1 << 21)}
# wide cases: (key bytes, value bytes) and n; the 2p31 ones are the yardsticks (gs_msb_sort_wide)
WIDE = {"u64_2p32": (8, 0), "rowid_2p32": (4, 8), "u64pairs_2p32": (8, 8)}
WIDE.update({k.replace("2p32", "2p31"): v for k, v in list(WIDE.items())})
YARDSTICK = {k: k.replace("2p32", "2p31") for k in WIDE if k.endswith("2p32")}
YARDSTICK["keys_2p33"] = "msb_2p31"


def bench_wide(case, reps, warmup, profile, dev):
    kb, vb = WIDE[case]
    n = (1 << 31) if case.endswith("2p31") else (1 << 32) + (1 << 21)
    kdt = torch.int64 if kb == 8 else torch.int32
    kt = gs.GS_KEY_U64 if kb == 8 else gs.GS_KEY_U32
    keys, alt = torch.empty(n, dtype=kdt, device=dev), torch.empty(n, dtype=kdt, device=dev)
    vals = torch.empty(n, dtype=torch.int64, device=dev) if vb else None
    vals_alt = torch.empty(n, dtype=torch.int64, device=dev) if vb else None
    orig = torch.empty(n, dtype=kdt, device=dev) if vb else None
    if case.endswith("2p31"):
        dm = torch.empty(gs.lib.gs_msb_wide_temp_bytes(n, kb, vb), dtype=torch.uint8, device=dev)
        sort = lambda: rdxsrt_unstable_sort_wide(keys, vals, n, alt, vals_alt, key_type=kt, dm=dm)  # noqa: E731
    else:
        dm = torch.empty(gs.lib.gs_msb_large_wide_temp_bytes(n, kb, vb), dtype=torch.uint8, device=dev)
        sort = lambda: gs.rdxsrt_unstable_sort_large_wide(keys, vals, n, alt, vals_alt, key_type=kt, pre_allocated_dm=dm)  # noqa: E731
    check_keys = (lambda: check_sorted_u64(keys, n)) if kb == 8 else (lambda: gs.check_sorted(keys, n))

    def fresh(rep):
        gs.generate_uniform_keys(n * kb // 4, seed=200 + rep, out=keys.view(torch.int32))
        if vb:   # row ids, chunk by chunk (like every elementwise op on these tensors)
            for i in range(0, n, CHUNK):
                torch.arange(i, min(i + CHUNK, n), dtype=torch.int64, out=vals[i:i + CHUNK])

    times = []
    for rep in range(warmup + reps):
        fresh(rep)
        if rep == warmup + reps - 1:
            _, s0, x0 = check_keys()
            if vb:
                for i in range(0, n, CHUNK):
                    orig[i:i + CHUNK].copy_(keys[i:i + CHUNK])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sort()
        b.record()
        b.synchronize()
        if rep >= warmup:
            times.append(a.elapsed_time(b))
    inv, s1, x1 = check_keys()
    verified = inv == 0 and (s1, x1) == (s0, x0)
    if vb:
        bad, vsum = check_pairs_enumerated_wide(orig, keys, vals, n)
        verified = verified and bad == 0 and vsum == (n * (n - 1) // 2) % (1 << 64)
    ms = statistics.median(times)
    out = {"n": n, "key_bytes": kb, "val_bytes": vb, "ms": round(ms, 3), "gkeys_s": round(n / ms / 1e6, 2),
           "runs_ms": [round(t, 3) for t in times], "verified": bool(verified)}
    if profile:
        fresh(0)
        torch.cuda.synchronize()
        with gs.KernelProfile() as prof:
            sort()
        torch.cuda.synchronize()
        out["kernels_ms"] = {k: [round(v[0], 3), v[1]] for k, v in prof.read().items()}
    del keys, alt, vals, vals_alt, orig, dm
    torch.cuda.empty_cache()
    return out


def bench(case, reps, warmup, profile, dev):
    if case in WIDE:
        return bench_wide(case, reps, warmup, profile, dev)
    n = SIZES[case]
    pairs = case.startswith("pairs")
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    alt = torch.empty(n, dtype=torch.int32, device=dev)
    vals = torch.empty(n, dtype=torch.int32, device=dev) if pairs else None
    vals_alt = torch.empty(n, dtype=torch.int32, device=dev) if pairs else None
    if case == "msb_2p31":
        dm = torch.empty(gs.lib.gs_msb_temp_bytes(n, 0), dtype=torch.uint8, device=dev)
        sort = lambda: gs.rdxsrt_unstable_sort(keys, None, n, alt, None, pre_allocated_dm=dm)  # noqa: E731
    else:
        dm = torch.empty(gs.lib.gs_msb_large_temp_bytes(n, int(pairs)), dtype=torch.uint8, device=dev)
        sort = lambda: gs.rdxsrt_unstable_sort_large(keys, vals, n, alt, vals_alt, pre_allocated_dm=dm)  # noqa: E731

    def fresh(rep):
        gs.generate_uniform_keys(n, seed=100 + rep, out=keys)
        if pairs:   # every value a fixed function of its key (enumerated values would wrap above 2^32)
            for i in range(0, n, CHUNK):
                vals[i:i + CHUNK] = _value_of(keys[i:i + CHUNK])

    times = []
    for rep in range(warmup + reps):
        fresh(rep)
        if rep == warmup + reps - 1:
            _, s0, x0 = gs.check_sorted(keys, n)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sort()
        b.record()
        b.synchronize()
        if rep >= warmup:
            times.append(a.elapsed_time(b))
    inv, s1, x1 = gs.check_sorted(keys, n)
    verified = inv == 0 and (s1, x1) == (s0, x0)
    if pairs:
        bad = sum(int((vals[i:i + CHUNK] != _value_of(keys[i:i + CHUNK])).sum().item()) for i in range(0, n, CHUNK))
        verified = verified and bad == 0
    ms = statistics.median(times)
    out = {"n": n, "ms": round(ms, 3), "gkeys_s": round(n / ms / 1e6, 2), "runs_ms": [round(t, 3) for t in times],
           "verified": bool(verified)}
    if profile:
        fresh(0)
        torch.cuda.synchronize()
        with gs.KernelProfile() as prof:
            sort()
        torch.cuda.synchronize()
        out["kernels_ms"] = {k: [round(v[0], 3), v[1]] for k, v in prof.read().items()}
    del keys, alt, vals, vals_alt, dm
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--cases", default="msb_2p31,keys_2p33,pairs_2p32",
                    help="also: u64_2p31,u64_2p32,rowid_2p31,rowid_2p32,u64pairs_2p31,u64pairs_2p32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {c: bench(c, a.reps, a.warmup, a.profile, dev) for c in a.cases.split(",")}
    if "msb_2p31" in res and "keys_2p33" in res:
        res["ratio_2p33_vs_2p31"] = round(res["keys_2p33"]["gkeys_s"] / res["msb_2p31"]["gkeys_s"], 3)
    for c, y in YARDSTICK.items():
        if c in WIDE and c in res and y in res:
            res["ratio_" + c] = round(res[c]["gkeys_s"] / res[y]["gkeys_s"], 3)
    res["verified"] = all(v["verified"] for v in res.values() if isinstance(v, dict))
    print(json.dumps(res), flush=True)
    return 0 if res["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
