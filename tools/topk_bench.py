"""gs_topk_u32 against the detour a caller takes without it: gs_lsb_sort_copy_u32 of the whole input, keeping the first k.

    python tools/topk_bench.py [--sizes 24,28,30] [--ks 10,16,20] [--runs 5] [--out profiles/topk_bench.json]

One process.  For every size (log2), distribution (uniform keys, Zipf keys, keys sharing one top byte: route 2), form (keys,
pairs, arguments) and k (log2): one untimed call of each side, then `runs` rounds with the two sides alternating, each call
timed with events on its stream.  The detour sorts (key, row id) pairs for the pairs and arguments forms and keys alone for the
keys form.  After the timed runs the first k of both sides are compared on the device (`verified`).  Every row, won or lost,
goes into the JSON: times of every run in ms, `best` of each side, `ratio` = detour best / top-k best (above 1: the select
wins), the route gs_topk_status reports, and `read_rate_TBps` = 8 bytes per key (the two input reads) over the top-k's best
time -- a whole-call figure, not a kernel's share."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="24,28,30")
ap.add_argument("--ks", default="10,16,20")
ap.add_argument("--dists", default="uniform,zipf,topbyte")
ap.add_argument("--modes", default="keys,pairs,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_keys(dist, n):
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    kind = gs.GS_GEN_ZIPF if dist == "zipf" else gs.GS_GEN_UNIFORM
    gs._lib.check(lib.gs_generate_u32(keys.data_ptr(), n, kind, 12345, 0, 0, None), "gs_generate_u32")
    if dist == "topbyte":
        keys.bitwise_and_(0x00FFFFFF).bitwise_or_(0x42000000)
    torch.cuda.synchronize()
    return keys


rows = []
for lg in [int(x) for x in args.sizes.split(",")]:
    n = 1 << lg
    rowids = torch.arange(n, dtype=torch.int32, device=dev)
    sort_k = torch.empty(n, dtype=torch.int32, device=dev)
    sort_v = torch.empty(n, dtype=torch.int32, device=dev)
    sort_nb = {hv: lib.gs_lsb_copy_temp_bytes(n, hv) for hv in (0, 1)}
    sort_temp = torch.empty(sort_nb[1], dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        keys = make_keys(dist, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            for lk in [int(x) for x in args.ks.split(",")]:
                k = 1 << lk
                if k > n:
                    continue
                nb = lib.gs_topk_temp_bytes(n, k, hv)
                temp = torch.empty(nb, dtype=torch.uint8, device=dev)
                ko = torch.empty(k, dtype=torch.int32, device=dev)
                vo = torch.empty(k, dtype=torch.int32, device=dev)

                def topk():
                    gs._lib.check(lib.gs_topk_u32(temp.data_ptr(), nb, keys.data_ptr(), rowids.data_ptr() if mode == "pairs" else None,
                                                  ko.data_ptr(), vo.data_ptr() if hv else None, n, k, 0, gs.GS_KEY_U32, None), "gs_topk_u32")

                def detour():
                    gs._lib.check(lib.gs_lsb_sort_copy_u32(sort_temp.data_ptr(), sort_nb[hv], keys.data_ptr(), sort_k.data_ptr(),
                                                           rowids.data_ptr() if hv else None, sort_v.data_ptr() if hv else None, n, 0, 32, 0,
                                                           gs.GS_KEY_U32, None), "gs_lsb_sort_copy_u32")

                topk()
                detour()
                torch.cuda.synchronize()
                t_top, t_det = [], []
                for _ in range(args.runs):
                    t_top.append(timed(topk))
                    t_det.append(timed(detour))
                ok = bool(torch.equal(ko, sort_k[:k])) and (not hv or bool(torch.equal(vo, sort_v[:k])))
                st = (C.c_uint32 * 8)()
                lib.gs_topk_status(temp.data_ptr(), n, k, hv, st, None)
                row = {"log2_n": lg, "dist": dist, "mode": mode, "log2_k": lk, "route": int(st[0]), "verified": ok,
                       "topk_ms": [round(t, 4) for t in t_top], "detour_ms": [round(t, 4) for t in t_det],
                       "topk_best": round(min(t_top), 4), "detour_best": round(min(t_det), 4),
                       "ratio": round(min(t_det) / min(t_top), 3),
                       "read_rate_TBps": round(8.0 * n / (min(t_top) * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
                del temp, ko, vo
        del keys
    del rowids, sort_k, sort_v, sort_temp
    torch.cuda.empty_cache()

lost = [r for r in rows if r["ratio"] <= 1.0]
result = {"bench": "topk_vs_sort_prefix", "runs": args.runs, "rows": rows, "all_verified": all(r["verified"] for r in rows),
          "lost": [[r["log2_n"], r["dist"], r["mode"], r["log2_k"], r["ratio"]] for r in lost]}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(rows), "all_verified": result["all_verified"], "lost": result["lost"]}))
