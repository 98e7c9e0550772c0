"""Device-timed sort of 8- and 16-bit keys above 2^32 elements (gs_lsb_sort_narrow_large) against two yardsticks in the same
process: (a) gs_lsb_sort_narrow on 2^31 elements of the same types, and (b) the detour a caller had to take before, on the same
input: widen the keys to u32, gs_lsb_sort_large on the key's bits, narrow the keys back (all three steps timed).

    python tools/narrow_large_bench.py [--reps R] [--warmup W] [--profile] [--cases u8,u8_u32,...] [--out FILE]

Cases, at 2^32 + 2^21 elements: u8 (keys), u8_u32, u8_u64 (u64 row ids), u16 (keys), u16_u64.  Every repetition sorts freshly
generated uniform keys (values: enumerated u32, or u64 row ids); the three sorts of a case alternate inside each repetition; ms
is the median of the repetitions, timed with events on the sort's stream.  `ratio_a` / `ratio_b` is the case's rate (elements
per ms) over yardstick (a)'s / (b)'s.  `verified`: after the last repetition the native sort's keys are in order with the input's
per-value counts, row ids ascend inside every key and name an equal input key, and the detour's keys and values are identical
to the native sort's (a stable sort's result is unique); all checked on the device in chunks.  --profile adds the per-kernel
device times (gs_profile_*) of one more repetition of the native sort.  Prints one JSON line (and writes it to --out)."""
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

CHUNK = 1 << 28
N = (1 << 32) + (1 << 21)
N2P31 = 1 << 31
CASES = {"u8": (1, 0), "u8_u32": (1, 4), "u8_u64": (1, 8), "u16": (2, 0), "u16_u64": (2, 8)}
KDT = {1: torch.uint8, 2: torch.int16}      # (u16 keys are held in int16 tensors)
VDT = {4: torch.int32, 8: torch.int64}


def _chunks(n):
    return [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]


def _fill(k, v, n, kb, vb, rep):
    gs.generate_uniform_keys(n * kb // 4, seed=500 + rep, out=k[:n].view(torch.int32))
    if vb == 4:
        gs.generate_enumerated_values(n, out=v[:n])
    elif vb == 8:   # row ids, chunk by chunk (a whole-tensor torch.arange of this size has returned wrong entries)
        for lo, hi in _chunks(n):
            torch.arange(lo, hi, dtype=torch.int64, out=v[lo:hi])


def _bits(t, kb):
    """the keys' bit patterns as int32 (u16 keys live in an int16 tensor)"""
    return t.to(torch.int32) & (0xFF if kb == 1 else 0xFFFF)


def _verify(kin, kout, vout, kout_b, vout_b, n, kb, vb):
    card = 1 << (8 * kb)
    cin, cout = (torch.zeros(card, dtype=torch.int64, device=kin.device) for _ in range(2))
    ok = True
    for lo, hi in _chunks(n):
        cin += torch.bincount(_bits(kin[lo:hi], kb), minlength=card)
        cout += torch.bincount(_bits(kout[lo:hi], kb), minlength=card)
        p = max(lo - 1, 0)
        ks = _bits(kout[p:hi], kb)
        ok = ok and bool((ks[1:] >= ks[:-1]).all())
        if vb == 8:
            vs, v = vout[p:hi], vout[lo:hi]
            ok = ok and not bool(((ks[1:] == ks[:-1]) & (vs[1:] <= vs[:-1])).any())
            ok = ok and bool(((v >= 0) & (v < n)).all()) and bool((kin[v.clamp(0, n - 1)] == kout[lo:hi]).all())
        ok = ok and bool(torch.equal(kout[lo:hi], kout_b[lo:hi]))
        if vb:
            ok = ok and bool(torch.equal(vout[lo:hi], vout_b[lo:hi]))
    return ok and bool(torch.equal(cin, cout))


def bench(case, reps, warmup, profile, dev):
    kb, vb = CASES[case]
    bits = 8 * kb
    kt = gs.GS_KEY_U8 if kb == 1 else gs.GS_KEY_U16
    n = N
    kin, kout, kout_b = (torch.empty(n, dtype=KDT[kb], device=dev) for _ in range(3))
    k32 = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    v = [torch.empty(n, dtype=VDT[vb], device=dev) for _ in range(2)] if vb else None     # the detour's DoubleBuffer; v[0] the input
    vout = torch.empty(n, dtype=VDT[vb], device=dev) if vb else None
    q_n = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
    q_a = gs.lib.gs_lsb_narrow_temp_bytes(N2P31, kt, vb)
    q_b = gs.lib.gs_lsb_large_temp_bytes(n, 4, vb)
    ws = torch.empty(max(q_n, q_a, q_b), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream()
    kk = (C.c_void_p * 2)(k32[0].data_ptr(), k32[1].data_ptr())
    vv = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr()) if vb else None
    sel = C.c_int(0)
    vp = (v[0].data_ptr(), vout.data_ptr()) if vb else (None, None)

    def native():
        check(gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), q_n, kin.data_ptr(), kout.data_ptr(), vp[0], vp[1], n, kt, vb, 0, bits, 0,
                                              s.cuda_stream), "gs_lsb_sort_narrow_large")

    def narrow_2p31():
        check(gs.lib.gs_lsb_sort_narrow(ws.data_ptr(), q_a, kin.data_ptr(), kout.data_ptr(), vp[0], vp[1], N2P31, kt, vb, 0, bits, 0,
                                        s.cuda_stream), "gs_lsb_sort_narrow")

    def detour():
        for lo, hi in _chunks(n):
            k32[0][lo:hi].copy_(kin[lo:hi])                       # widen (the bits above the key's are not sorted on)
        sel.value = 0
        check(gs.lib.gs_lsb_sort_large(ws.data_ptr(), q_b, kk, vv, C.byref(sel), n, 4, vb, 0, bits, 0, gs.GS_KEY_U32, s.cuda_stream),
              "gs_lsb_sort_large")
        for lo, hi in _chunks(n):
            kout_b[lo:hi].copy_(k32[sel.value][lo:hi])            # narrow back

    # (in this order the native result is still in kout / vout when the detour's is compared with it)
    sorts = {"narrow_2p31": (narrow_2p31, N2P31), "native": (native, n), "detour": (detour, n)}
    times = {name: [] for name in sorts}
    verified = True
    for rep in range(warmup + reps):
        last = rep == warmup + reps - 1
        for name, (fn, m) in sorts.items():
            # fresh input for every sort; the native sort and the detour of a repetition get the same one
            _fill(kin, v[0] if vb else None, m, kb, vb, 100 + rep if name == "narrow_2p31" else rep)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= warmup:
                times[name].append(a.elapsed_time(b))
            if last and name == "detour":
                verified = _verify(kin, kout, vout, kout_b, v[sel.value] if vb else None, n, kb, vb)
    out = {"n": n, "key_bytes": kb, "val_bytes": vb, "verified": bool(verified)}
    for name, (fn, m) in sorts.items():
        ms = statistics.median(times[name])
        out[name] = {"n": m, "ms": round(ms, 3), "g_per_s": round(m / ms / 1e6, 2), "runs_ms": [round(t, 3) for t in times[name]]}
    out["ratio_a"] = round(out["native"]["g_per_s"] / out["narrow_2p31"]["g_per_s"], 3)
    out["ratio_b"] = round(out["native"]["g_per_s"] / out["detour"]["g_per_s"], 3)
    if profile:
        _fill(kin, v[0] if vb else None, n, kb, vb, 0)
        torch.cuda.synchronize()
        with gs.KernelProfile() as prof:
            native()
        torch.cuda.synchronize()
        out["native"]["kernels_ms"] = {kn: [round(x[0], 3), x[1]] for kn, x in prof.read().items()}
    del kin, kout, kout_b, k32, v, vout, ws
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for c in a.cases.split(","):
        res[c] = bench(c, a.reps, a.warmup, a.profile, dev)
        print("%s: %s" % (c, json.dumps(res[c])), file=sys.stderr, flush=True)
    res["verified"] = all(v["verified"] for v in res.values() if isinstance(v, dict))
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
