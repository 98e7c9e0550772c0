"""Device-timed sorts of 8- and 16-bit keys: the native kernels (gs_lsb_sort_narrow) against the adapter (gs_lsb_sort_any,
the (u32 sort key, u32 index) sort and gather) on the same input in the same process.

    python tools/narrow_bench.py [--reps R] [--warmup W] [--cases u8,u8_u32,...] [--sizes 20,24,28] [--profile]

Cases: u8 and u16 keys alone (the default SortKeys call: 8-bit keys take the histogram-and-fill path), the same with
begin_bit = 1 (`u8_b1`, `u16_b1`: the digit passes), (u8, u8), (u8, u32), (u8, u64), (u8, 16-byte), (u16, u16), (u16, u32) and
(u16, u64); each at 2^20, 2^24 and 2^28 elements of uniform keys, and at 2^28 with all keys equal (`dist: equal`).  Every
repetition sorts freshly generated keys; the two sorts alternate inside each repetition; ms is the median of the
repetitions, timed with events on the sort's stream.  `ratio` is any_ms / narrow_ms (above 1: the native path is faster).
`bytes_per_elem` counts the native path's HBM traffic per element (each pass reads the keys for the histogram and reads and
writes keys and values in the scatter; the fill path reads the keys once and writes them once) and `frac_8TBps` is that
traffic over the time as a fraction of 8 TB/s.  `verified`: after the last repetition the native path's keys are in order on
the sorted bits and have the input's per-value counts, checked on the device, and equal the adapter's output byte for byte.
--profile adds the per-kernel device times (gs_profile_*) of one more repetition of the native sort.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd._lib import check  # noqa: E402

# name -> (key bytes, value bytes, begin_bit)
CASES = {"u8": (1, 0, 0), "u8_b1": (1, 0, 1), "u8_u8": (1, 1, 0), "u8_u32": (1, 4, 0), "u8_u64": (1, 8, 0), "u8_v16": (1, 16, 0),
         "u16": (2, 0, 0), "u16_b1": (2, 0, 1), "u16_u16": (2, 2, 0), "u16_u32": (2, 4, 0), "u16_u64": (2, 8, 0)}


def bytes_per_elem(kb, vb, begin):
    if kb == 1 and vb == 0 and begin == 0:
        return 2                                    # histogram 1 + fill 1
    return kb * (kb + 2 * (kb + vb))                # kb passes: upsweep kb, downsweep (kb + vb) in and out


def _fill_keys(k, kb, dist, rep, g):
    n = k.numel()
    if dist == "equal":
        k.fill_(37 + rep)
    elif kb == 1:
        k.copy_(torch.randint(0, 256, (n,), device=k.device, generator=g, dtype=torch.int32).to(torch.uint8))
    else:
        k.copy_(torch.randint(-2**15, 2**15, (n,), device=k.device, generator=g, dtype=torch.int32).to(torch.int16))


def _verify(kin, kout, kany, vout, vany, kb, begin):
    card = 256 if kb == 1 else 65536
    off = 0 if kb == 1 else 32768
    if not torch.equal(kout, kany) or (vout is not None and not torch.equal(vout, vany)):
        return False
    a = torch.bincount(kin.to(torch.int64) + off, minlength=card)
    b = torch.bincount(kout.to(torch.int64) + off, minlength=card)
    if not torch.equal(a, b):
        return False
    d = (kout.to(torch.int32) & (card - 1)) >> begin    # the sorted bits of the unsigned pattern
    return bool((d[1:] >= d[:-1]).all())


def bench(case, lg, dist, reps, warmup, profile, dev):
    kb, vb, begin = CASES[case]
    n = 1 << lg
    kt = gs.GS_KEY_U8 if kb == 1 else gs.GS_KEY_U16
    end = 8 * kb
    kdt = torch.uint8 if kb == 1 else torch.int16
    kin = torch.empty(n, dtype=kdt, device=dev)
    kout, kany = torch.empty_like(kin), torch.empty_like(kin)
    vin = vout = vany = None
    if vb:
        vin = torch.empty(n * vb, dtype=torch.uint8, device=dev)
        if vb >= 4:
            vin.view(torch.int32).view(n, vb // 4)[:, 0] = torch.arange(n, dtype=torch.int32, device=dev)
        else:
            vin.copy_(torch.arange(n * vb, device=dev, dtype=torch.int32).to(torch.uint8))
        vout, vany = torch.empty_like(vin), torch.empty_like(vin)
    nb_n = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    nb_a = gs.lib.gs_lsb_any_temp_bytes(n, kt, vb)
    ws_n = torch.empty(nb_n, dtype=torch.uint8, device=dev)
    ws_a = torch.empty(nb_a, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731

    def run_narrow():
        check(gs.lib.gs_lsb_sort_narrow(ws_n.data_ptr(), nb_n, kin.data_ptr(), kout.data_ptr(), p(vin), p(vout), n, kt, vb, begin, end,
                                        0, sp), "gs_lsb_sort_narrow")

    def run_any():
        check(gs.lib.gs_lsb_sort_any(ws_a.data_ptr(), nb_a, kin.data_ptr(), kany.data_ptr(), p(vin), p(vany), n, kt, vb, begin, end,
                                     0, sp), "gs_lsb_sort_any")

    g = torch.Generator(device=dev)
    g.manual_seed(1000 + lg)
    t_n, t_a = [], []
    for rep in range(warmup + reps):
        _fill_keys(kin, kb, dist, rep, g)
        order = (run_narrow, run_any) if rep % 2 == 0 else (run_any, run_narrow)
        ms = {}
        for fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms[fn] = a.elapsed_time(b)
        if rep >= warmup:
            t_n.append(ms[run_narrow])
            t_a.append(ms[run_any])
    torch.cuda.synchronize()
    verified = _verify(kin, kout, kany, vout, vany, kb, begin)
    mn, ma = statistics.median(t_n), statistics.median(t_a)
    bpe = bytes_per_elem(kb, vb, begin)
    r = {"case": case, "log2_n": lg, "dist": dist, "narrow_ms": round(mn, 4), "any_ms": round(ma, 4), "ratio": round(ma / mn, 3),
         "bytes_per_elem": bpe, "frac_8TBps": round(bpe * n / (mn * 1e-3) / 8e12, 4), "verified": verified}
    if profile:
        with gs.KernelProfile() as prof:
            run_narrow()
            torch.cuda.synchronize()
        r["kernels_ms"] = {k: round(v[0], 4) for k, v in prof.read().items()}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--sizes", default="20,24,28")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for case in args.cases.split(","):
        sizes = [int(x) for x in args.sizes.split(",")]
        for lg in sizes:
            rows.append(bench(case, lg, "uniform", args.reps, args.warmup, args.profile, dev))
        if 28 in sizes:
            rows.append(bench(case, 28, "equal", args.reps, args.warmup, args.profile, dev))
    print(json.dumps({"tool": "narrow_bench", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                      "all_verified": all(r["verified"] for r in rows), "rows": rows}))


if __name__ == "__main__":
    main()
