"""Device-timed measurements behind the float key categories of 8 and 16 bits.

    python tools/halfkeys_bench.py [--parent-lib PATH/libgpusort.so] [--runs 5] [--sections int,f16] [--out FILE.json]

Sections (each row: the times of every run in ms, `best` and `worst`):
  int     the integer narrow classes of this build against the parent commit's library (--parent-lib, loaded into the same
          process), at 2^28 elements: u16 keys over 8 bits (one pass), (u16, u32), (u8, u32), and segmented (u16, u32) in
          segments of 256 and of 2^20.  `ratio` = parent best / this build's best; 0.97 and above is a tie.
  f16     the same classes with GS_KEY_F16 / GS_KEY_F8 keys against GS_KEY_U16 / GS_KEY_U8 on the same bits, this build only:
          `ratio` = integer best / float best (what the float term costs).
The two builds alternate run by run on the same input; a run is one sort timed with events on its stream, after one
untimed sort per build.  Without --parent-lib the section that needs it is skipped.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402
from gpu_sort_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--sections", default="int,f16")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
USED = ("gs_lsb_narrow_temp_bytes", "gs_lsb_sort_narrow", "gs_segmented_narrow_temp_bytes", "gs_segmented_sort_narrow")


def bind(path):
    lib = C.CDLL(path)
    for name in USED:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


new = gs.lib
parent = bind(args.parent_lib) if args.parent_lib else None


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns):
    """fns: {name: callable}; one untimed call each, then args.runs rounds, the builds alternating inside a round"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, f in fns.items():
            out[k].append(round(timed(f), 4))
    return out


def plain(lib, kt, vb, n, kin, kout, vin, vout, ws, nb, bb, eb):
    def f():
        err = lib.gs_lsb_sort_narrow(ws.data_ptr(), nb, kin.data_ptr(), kout.data_ptr(), vin.data_ptr() if vb else None,
                                     vout.data_ptr() if vb else None, n, kt, vb, bb, eb, 0, None)
        assert err == 0, err
    return f


def segmented(lib, kt, n, keep_k, keep_v, k, v, offs, nseg, ws, nb):
    def f():
        k[0].copy_(keep_k)
        v[0].copy_(keep_v)
        kp = (C.c_void_p * 2)(k[0].data_ptr(), k[1].data_ptr())
        vp = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr())
        sel = C.c_int(0)
        err = lib.gs_segmented_sort_narrow(ws.data_ptr(), nb, kp, vp, C.byref(sel), n, nseg, offs.data_ptr(), offs.data_ptr() + 4,
                                           kt, 4, 0, 16, 0, None)
        assert err == 0, err
    return f


def row(times):
    return {k: {"ms": v, "best": min(v), "worst": max(v)} for k, v in times.items()}


def rand_keys(n, kb, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    dt = torch.uint8 if kb == 1 else torch.int16
    k = torch.empty(n, dtype=dt, device=dev)
    step = 1 << 26
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        k[lo:hi] = torch.randint(0, 256 ** kb, (hi - lo,), device=dev, generator=g, dtype=torch.int32).to(dt)
    return k


CLASSES = (("u16_8bits", 2, 0, 0, 8), ("u16_u32", 2, 4, 0, 16), ("u8_u32", 1, 4, 0, 8))
INT_KT = {1: gs.GS_KEY_U8, 2: gs.GS_KEY_U16}
FLT_KT = {1: gs.GS_KEY_F8, 2: gs.GS_KEY_F16}
SEG_SIZES = (256, 1 << 20)


def classes_section(pairs):
    """pairs: [(label, lib, key-type table)]: every class of CLASSES and the segmented ones at 2^28, the labels alternating"""
    n = 1 << 28
    rows = []
    for name, kb, vb, bb, eb in CLASSES:
        kin = rand_keys(n, kb, 1)
        kout = torch.empty_like(kin)
        vin = torch.arange(n, dtype=torch.int32, device=dev) if vb else None
        vout = torch.empty_like(vin) if vb else None
        nb = max(lib.gs_lsb_narrow_temp_bytes(n, kts[kb], vb) for _, lib, kts in pairs)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        t = alternate({lab: plain(lib, kts[kb], vb, n, kin, kout, vin, vout, ws, nb, bb, eb) for lab, lib, kts in pairs})
        rows.append(dict(case=name, n=n, **row(t)))
        del kin, kout, vin, vout, ws
    for seg in SEG_SIZES:
        nseg = n // seg
        keep_k, keep_v = rand_keys(n, 2, 2), torch.arange(n, dtype=torch.int32, device=dev)
        k = [torch.empty_like(keep_k), torch.empty_like(keep_k)]
        v = [torch.empty_like(keep_v), torch.empty_like(keep_v)]
        offs = (torch.arange(nseg + 1, dtype=torch.int64, device=dev) * seg).to(torch.int32)
        nb = max(lib.gs_segmented_narrow_temp_bytes(n, kts[2], 4, nseg) for _, lib, kts in pairs)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        t = alternate({lab: segmented(lib, kts[2], n, keep_k, keep_v, k, v, offs, nseg, ws, nb) for lab, lib, kts in pairs})
        rows.append(dict(case="seg_u16_u32_%d" % seg, n=n, note="each run includes the copy of the input into the buffer", **row(t)))
        del keep_k, keep_v, k, v, offs, ws
    a, b = pairs[0][0], pairs[1][0]
    for r in rows:
        r["ratio"] = round(r[a]["best"] / r[b]["best"], 4)
    return rows


res = {"device": torch.cuda.get_device_name(0), "runs": args.runs}
sections = args.sections.split(",")
if "int" in sections and parent is not None:
    res["int_vs_parent"] = classes_section([("parent", parent, INT_KT), ("this", new, INT_KT)])
if "f16" in sections:
    res["f16_vs_u16"] = classes_section([("integer", new, INT_KT), ("float", new, FLT_KT)])
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
