"""Device-timed MSB sort above 2^32 keys (gs_msb_sort_large_u32) against the plain MSB sort at 2^31 in the same process.

    python tools/large_bench.py [--reps R] [--warmup W] [--profile] [--cases msb_2p31,keys_2p33,pairs_2p32]

Cases: msb_2p31 = gs_msb_sort_u32 on 2^31 uniform keys (the yardstick), keys_2p33 = 2^33 uniform keys, pairs_2p32 =
2^32 + 2^21 uniform keys with 32-bit values (each a fixed function of its key, checked after the sort).  Every repetition sorts freshly generated keys; ms is the median of the
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
from large_check import CHUNK, _value_of  # noqa: E402

SIZES = {"msb_2p31": 1 << 31, "keys_2p33": 1 << 33, "pairs_2p32": (1 << 32) + (1 << 21)}


def bench(case, reps, warmup, profile, dev):
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
    ap.add_argument("--cases", default="msb_2p31,keys_2p33,pairs_2p32")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {c: bench(c, a.reps, a.warmup, a.profile, dev) for c in a.cases.split(",")}
    if "msb_2p31" in res and "keys_2p33" in res:
        res["ratio_2p33_vs_2p31"] = round(res["keys_2p33"]["gkeys_s"] / res["msb_2p31"]["gkeys_s"], 3)
    res["verified"] = all(v["verified"] for v in res.values() if isinstance(v, dict))
    print(json.dumps(res), flush=True)
    return 0 if res["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
