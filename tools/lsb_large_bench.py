"""Device-timed stable sort above 2^32 elements (gs_lsb_sort_large) against two yardsticks in the same process:
(a) the plain stable sort (gs_lsb_sort_u32 / gs_lsb_sort_wide) on 2^31 elements of the same types, and (b) the MSB large sort
(gs_msb_sort_large_u32 / gs_msb_sort_large_wide) on the same input.

    python tools/lsb_large_bench.py [--reps R] [--warmup W] [--profile] [--cases keys_2p33,pairs_2p32,...]

Cases: keys_2p33 = 2^33 uniform u32 keys, all 32 bits; at 2^32 + 2^21 elements: pairs_2p32 (u32, u32), rowid_2p32 (u32 keys,
u64 row ids), u64_2p32 (u64 keys) and u64pairs_2p32 (u64, u64).  Every repetition sorts freshly generated keys (values:
enumerated u32, or u64 row ids); the three sorts of a case alternate inside each repetition; ms is the median of the
repetitions, timed with events on the sort's stream (the MSB large sort's host waits included).  `ratio_a` / `ratio_b` is
the case's rate (elements per ms) over yardstick (a)'s / (b)'s.  `verified`: after the last repetition the LSB large sort's
keys are in order (gs_check_sorted_stable; with row ids also stable) and the input's multiset (sum and xor of splitmix64).
--profile adds the per-kernel device times (gs_profile_*) of one more repetition of each sort.  Prints one JSON line."""
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
from gpu_sort_amd.datagen import check_sorted_u64  # noqa: E402

CHUNK = 1 << 28
N2P32 = (1 << 32) + (1 << 21)
N2P31 = 1 << 31
CASES = {"keys_2p33": (4, 0, 1 << 33), "pairs_2p32": (4, 4, N2P32), "rowid_2p32": (4, 8, N2P32), "u64_2p32": (8, 0, N2P32),
         "u64pairs_2p32": (8, 8, N2P32)}
TDT = {4: torch.int32, 8: torch.int64}


def _fill(k, v, n, kb, vb, rep):
    gs.generate_uniform_keys(n * kb // 4, seed=300 + rep, out=k[:n].view(torch.int32))
    if vb == 4:
        gs.generate_enumerated_values(n, out=v[:n])
    elif vb == 8:   # row ids, chunk by chunk (a whole-tensor torch.arange of this size has returned wrong entries)
        for i in range(0, n, CHUNK):
            torch.arange(i, min(i + CHUNK, n), dtype=torch.int64, out=v[i:min(i + CHUNK, n)])


def _multiset(k, n, kb):
    if kb == 8:
        return check_sorted_u64(k, n)[1:]
    return gs.check_sorted(k, n)[1:]


def _stable_disorder(k, rowids, n, kb, kt):
    res = torch.zeros(1, dtype=torch.int64, device=k.device)
    check(gs.lib.gs_check_sorted_stable(k.data_ptr(), rowids.data_ptr() if rowids is not None else None, n, kb, kt, 0, 8 * kb, 0,
                                        res.data_ptr(), None), "gs_check_sorted_stable")
    return int(res.item())


def bench(case, reps, warmup, profile, dev):
    kb, vb, n = CASES[case]
    kt = gs.GS_KEY_U64 if kb == 8 else gs.GS_KEY_U32
    wide = kb == 8 or vb == 8
    k = [torch.empty(n, dtype=TDT[kb], device=dev) for _ in range(2)]
    v = [torch.empty(n, dtype=TDT[vb], device=dev) for _ in range(2)] if vb else None
    q_lsb = gs.lib.gs_lsb_large_temp_bytes(n, kb, vb)
    q_a = gs.lib.gs_lsb_wide_temp_bytes(N2P31, kb, vb) if wide else gs.lib.gs_lsb_temp_bytes(N2P31, int(vb != 0))
    q_b = gs.lib.gs_msb_large_wide_temp_bytes(n, kb, vb) if wide else gs.lib.gs_msb_large_temp_bytes(n, int(vb != 0))
    ws = torch.empty(max(q_lsb, q_a, q_b), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream()
    kk = (C.c_void_p * 2)(k[0].data_ptr(), k[1].data_ptr())
    vv = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr()) if vb else None
    sel = C.c_int(0)

    def lsb_large():
        sel.value = 0
        check(gs.lib.gs_lsb_sort_large(ws.data_ptr(), q_lsb, kk, vv, C.byref(sel), n, kb, vb, 0, 8 * kb, 0, kt, s.cuda_stream),
              "gs_lsb_sort_large")

    def lsb_2p31():
        sel.value = 0
        if wide:
            e = gs.lib.gs_lsb_sort_wide(ws.data_ptr(), q_a, kk, vv, C.byref(sel), N2P31, kb, vb, 0, 8 * kb, 0, kt, s.cuda_stream)
        else:
            e = gs.lib.gs_lsb_sort_u32(ws.data_ptr(), q_a, kk, vv, C.byref(sel), N2P31, 0, 32, 0, kt, s.cuda_stream)
        check(e, "plain LSB sort")

    def msb_large():
        vp = (v[0].data_ptr(), v[1].data_ptr()) if vb else (None, None)
        if wide:
            e = gs.lib.gs_msb_sort_large_wide(ws.data_ptr(), q_b, k[0].data_ptr(), vp[0], n, k[1].data_ptr(), vp[1], kb, vb, kt,
                                              s.cuda_stream, 0)
        else:
            e = gs.lib.gs_msb_sort_large_u32(ws.data_ptr(), q_b, k[0].data_ptr(), vp[0], n, k[1].data_ptr(), vp[1], kt, s.cuda_stream, 0)
        check(e, "MSB large sort")

    sorts = {"lsb_large": (lsb_large, n), "lsb_2p31": (lsb_2p31, N2P31), "msb_large": (msb_large, n)}
    times = {name: [] for name in sorts}
    verified = False
    for rep in range(warmup + reps):
        for name, (fn, m) in sorts.items():
            _fill(k[0], v[0] if vb else None, m, kb, vb, rep)
            last = name == "lsb_large" and rep == warmup + reps - 1
            if last:
                before = _multiset(k[0], n, kb)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
            if last:
                out_k, out_v = k[sel.value], (v[sel.value] if vb == 8 else None)
                disorder = _stable_disorder(out_k, out_v, n, kb, kt)
                verified = disorder == 0 and _multiset(out_k, n, kb) == before
    out = {"n": n, "key_bytes": kb, "val_bytes": vb, "verified": bool(verified)}
    for name, (fn, m) in sorts.items():
        ms = statistics.median(times[name])
        out[name] = {"n": m, "ms": round(ms, 3), "g_per_s": round(m / ms / 1e6, 2), "runs_ms": [round(t, 3) for t in times[name]]}
    out["ratio_a"] = round(out["lsb_large"]["g_per_s"] / out["lsb_2p31"]["g_per_s"], 3)
    out["ratio_b"] = round(out["lsb_large"]["g_per_s"] / out["msb_large"]["g_per_s"], 3)
    if profile:
        for name, (fn, m) in sorts.items():
            _fill(k[0], v[0] if vb else None, m, kb, vb, 0)
            torch.cuda.synchronize()
            with gs.KernelProfile() as prof:
                fn()
            torch.cuda.synchronize()
            out[name]["kernels_ms"] = {kn: [round(x[0], 3), x[1]] for kn, x in prof.read().items()}
    del k, v, ws
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {c: bench(c, a.reps, a.warmup, a.profile, dev) for c in a.cases.split(",")}
    res["verified"] = all(v["verified"] for v in res.values() if isinstance(v, dict))
    print(json.dumps(res), flush=True)
    return 0 if res["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
