"""Device-timed segmented sorts of 8- and 16-bit keys: the native route (gs_segmented_sort_narrow) against the detour a caller
without it has to take for the same job, on the same input in the same process:

    1. one elementwise widening of the keys to u32 (torch),
    2. gs_segmented_sort_u32 on bits [0, 8 * key_bytes), or gs_segmented_sort_wide for 8-byte values,
    3. one narrowing back.

    python tools/segmented_narrow_bench.py [--reps R] [--warmup W] [--cases u8,u16_u32,...] [--segs 5,8,...,all] [--out FILE]

Cases: u8 and u16 keys with no values and with u32 values at 2^28 elements, (u16, u64) at 2^27; uniform keys in equal segments
of 32, 256, 1024, 2048, 8192, 2^14, 2^17, 2^20 and 2^24 elements and one segment of everything, plus one all-equal-keys row per
key width at segments of 2^17.  Every repetition sorts freshly generated keys; the two routes alternate inside each
repetition; ms is the median of the repetitions, timed with events on the sort's stream, and the min and max of each route's
times are kept.  `detour_sort_ms` is the sort-only part of the detour (median).  `ratio` is detour_ms / native_ms (above 1:
the native route is faster).  `lost`: the native median exceeds the detour's median by more than the detour's own max - min
spread in that row.  `bytes_per_elem` counts the native route's HBM traffic per element by the algorithm (segments above the
one-workgroup cap: per 8-bit pass the keys are read for the histogram and keys and values are read and written by the
scatter; up to the cap: one read and one write) and `frac_8TBps` is that traffic over the time as a fraction of 8 TB/s.
`verified`: after the last repetition, on the device, both routes' keys and values are equal, every segment's keys are in
order and the per-value counts equal the input's.  Prints one JSON line (and writes it to --out)."""
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

# name -> (key bytes, value bytes, log2 of the elements)
CASES = {"u8": (1, 0, 28), "u8_u32": (1, 4, 28), "u16": (2, 0, 28), "u16_u32": (2, 4, 28), "u16_u64": (2, 8, 27)}
SEGS = ("5", "8", "10", "11", "13", "14", "17", "20", "24", "all")


def bytes_per_elem(kb, vb, seg, cap):
    if seg <= cap:
        return 2 * (kb + vb)
    return kb * (kb + 2 * (kb + vb))


def bench(case, seglg, dist, reps, warmup, dev):
    kb, vb, lg = CASES[case]
    n = 1 << lg
    seg = n if seglg == "all" else 1 << int(seglg)
    if seg > n:
        return None
    nseg = n // seg
    kt = gs.GS_KEY_U8 if kb == 1 else gs.GS_KEY_U16
    end = 8 * kb
    kdt = torch.uint8 if kb == 1 else torch.int16          # (int16 holds the u16 bit patterns)
    vdt = torch.int32 if vb == 4 else torch.int64
    kin = torch.empty(n, dtype=kdt, device=dev)
    vin = torch.arange(n, dtype=vdt, device=dev) if vb else None
    nk = [torch.empty_like(kin), torch.empty_like(kin)]
    nv = [torch.empty_like(vin), torch.empty_like(vin)] if vb else None
    wk = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
    wv = [torch.empty_like(vin), torch.empty_like(vin)] if vb else None
    dk = torch.empty_like(kin)                             # the detour's narrowed result
    offs = torch.arange(0, n + 1, seg, dtype=torch.int64, device=dev).to(torch.int32)
    ob, oe = offs[:-1].contiguous(), offs[1:].contiguous()
    nb_n = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, nseg)
    nb_d = gs.lib.gs_segmented_wide_temp_bytes(n, 4, 8, nseg) if vb == 8 else gs.lib.gs_segmented_temp_bytes(n, int(vb != 0), nseg)
    ws_n = torch.empty(nb_n, dtype=torch.uint8, device=dev)
    ws_d = torch.empty(nb_d, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    cap = gs.lib.gs_segmented_narrow_cap(kt, vb)
    pair = lambda t: (C.c_void_p * 2)(t[0].data_ptr(), t[1].data_ptr()) if t is not None else None   # noqa: E731
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    res = {}

    def run_native():
        nk[0].copy_(kin)
        if vb:
            nv[0].copy_(vin)
        sel = C.c_int(0)
        a, b = ev(), ev()
        a.record(stream)
        check(gs.lib.gs_segmented_sort_narrow(ws_n.data_ptr(), nb_n, pair(nk), pair(nv), C.byref(sel), n, nseg, ob.data_ptr(), oe.data_ptr(),
                                              kt, vb, 0, end, 0, sp), "gs_segmented_sort_narrow")
        b.record(stream)
        b.synchronize()
        res["native"] = (nk[sel.value], nv[sel.value] if vb else None)
        return a.elapsed_time(b), None

    def run_detour():
        if vb:
            wv[0].copy_(vin)
        sel = C.c_int(0)
        a, s0, s1, b = ev(), ev(), ev(), ev()
        a.record(stream)
        wk[0].copy_(kin)                                   # widen (a sign-extended u16 pattern keeps its low 16 bits)
        s0.record(stream)
        if vb == 8:
            check(gs.lib.gs_segmented_sort_wide(ws_d.data_ptr(), nb_d, pair(wk), pair(wv), C.byref(sel), n, nseg, ob.data_ptr(), oe.data_ptr(),
                                                4, 8, 0, end, 0, gs.GS_KEY_U32, sp), "gs_segmented_sort_wide")
        else:
            check(gs.lib.gs_segmented_sort_u32(ws_d.data_ptr(), nb_d, pair(wk), pair(wv), C.byref(sel), n, nseg, ob.data_ptr(), oe.data_ptr(),
                                               0, end, 0, gs.GS_KEY_U32, sp), "gs_segmented_sort_u32")
        s1.record(stream)
        dk.copy_(wk[sel.value])                            # narrow back
        b.record(stream)
        b.synchronize()
        res["detour"] = (dk, wv[sel.value] if vb else None)
        return a.elapsed_time(b), s0.elapsed_time(s1)

    g = torch.Generator(device=dev)
    g.manual_seed(1000 + lg + seg % 1000)
    t_n, t_d, t_s = [], [], []
    for rep in range(warmup + reps):
        if dist == "equal":
            kin.fill_(37 + rep)
        elif kb == 1:
            kin.copy_(torch.randint(0, 256, (n,), device=dev, generator=g, dtype=torch.int32).to(torch.uint8))
        else:
            kin.copy_(torch.randint(-2**15, 2**15, (n,), device=dev, generator=g, dtype=torch.int32).to(torch.int16))
        torch.cuda.synchronize()
        order = (run_native, run_detour) if rep % 2 == 0 else (run_detour, run_native)
        ms = {fn: fn() for fn in order}
        if rep >= warmup:
            t_n.append(ms[run_native][0])
            t_d.append(ms[run_detour][0])
            t_s.append(ms[run_detour][1])
    torch.cuda.synchronize()
    # verification on the device (n <= 2^28: one chunk)
    (k1, v1), (k2, v2) = res["native"], res["detour"]
    card, off = (256, 0) if kb == 1 else (65536, 32768)
    verified = torch.equal(k1, k2) and (not vb or torch.equal(v1, v2))
    u = (k1.to(torch.int32) & (card - 1)).view(nseg, seg)
    verified = verified and bool((u[:, 1:] >= u[:, :-1]).all())
    verified = verified and torch.equal(torch.bincount(kin.to(torch.int64) + off, minlength=card),
                                        torch.bincount(k1.to(torch.int64) + off, minlength=card))
    if vb:
        verified = verified and torch.equal(kin[v1.to(torch.int64)], k1)
    mn, md = statistics.median(t_n), statistics.median(t_d)
    bpe = bytes_per_elem(kb, vb, seg, cap)
    return {"case": case, "log2_n": lg, "segment": seg, "segments": nseg, "dist": dist,
            "native_ms": round(mn, 4), "native_min": round(min(t_n), 4), "native_max": round(max(t_n), 4),
            "detour_ms": round(md, 4), "detour_min": round(min(t_d), 4), "detour_max": round(max(t_d), 4),
            "detour_sort_ms": round(statistics.median(t_s), 4), "ratio": round(md / mn, 3),
            "lost": bool(mn - md > max(t_d) - min(t_d)), "elems_per_s": round(n / (mn * 1e-3), 0),
            "bytes_per_elem": bpe, "frac_8TBps": round(bpe * n / (mn * 1e-3) / 8e12, 4), "verified": bool(verified)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--segs", default=",".join(SEGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for case in args.cases.split(","):
        for s in args.segs.split(","):
            r = bench(case, s, "uniform", args.reps, args.warmup, dev)
            if r:
                rows.append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        if case in ("u8", "u16") and "17" in args.segs.split(","):
            rows.append(bench(case, "17", "equal", args.reps, args.warmup, dev))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = json.dumps({"tool": "segmented_narrow_bench", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                      "all_verified": all(r["verified"] for r in rows), "lost": [(r["case"], r["segment"], r["dist"]) for r in rows if r["lost"]],
                      "rows": rows})
    print(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
