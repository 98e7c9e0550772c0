"""gs_topk_rows_u32 against the two detours a caller takes without it.

    python tools/topk_rows_bench.py [--shapes 20x64x8,...] [--runs 5] [--out profiles/topk_rows_bench.json]

One process.  For every shape (log2 rows or rows, cols, k), distribution (uniform keys; keys sharing one top byte on two
shapes) and form (keys, arguments): one untimed call of each side, then `runs` rounds with the sides alternating, each call
timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_u32 with regular offsets on a copy of the matrix (column indices as values for the arguments form),
      keeping the first k of every row.  Neither the copy nor the strided gather of the first k is timed: both omissions
      favour the detour.
  (B) a host loop of gs_topk_u32 per row on one workspace, on shapes of up to 256 rows only.
After the timed runs every row's outputs are compared on the device with the first k of (A)'s sorted rows (`verified`).  Every
row of the table, won or lost, goes into the JSON: the times of every run in ms, `best` of each side, `ratio_A` / `ratio_B` =
detour best / rows best (above 1: the rows call wins), the plan gs_topk_rows_plan reports, and `read_rate_TBps` = 4 bytes per key
over the rows call's best time -- a whole-call figure, not a kernel's share."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

SHAPES = "2^20x64x8,2^20x256x8,2^18x1024x64,2^16x4096x64,2^15x8192x256,2^12x65536x100,1024x151936x50,256x2^20x1024,32x2^23x1024"
TOPBYTE = "2^18x1024x64,1024x151936x50"

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--topbyte", default=TOPBYTE)
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib


def num(s):
    return 1 << int(s[2:]) if s.startswith("2^") else int(s)


def parse(spec):
    return [tuple(num(x) for x in s.split("x")) for s in spec.split(",") if s]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def make_keys(dist, n):
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    gs._lib.check(lib.gs_generate_u32(keys.data_ptr(), n, gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    if dist == "topbyte":
        keys.bitwise_and_(0x00FFFFFF).bitwise_or_(0x42000000)
    torch.cuda.synchronize()
    return keys


table = []
topbyte = set(parse(args.topbyte))
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_temp_bytes(n, hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for dist in ["uniform"] + (["topbyte"] if (rows, cols, k) in topbyte else []):
        keys = make_keys(dist, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.empty(rows * k, dtype=torch.int32, device=dev)
            vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKRows.Plan(rows, cols, k, hv)

            def rows_call():
                gs._lib.check(lib.gs_topk_rows_u32(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None,
                                                   rows, cols, cols, k, 0, gs.GS_KEY_U32, None), "gs_topk_rows_u32")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(colids)
                    seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                                  0, 32, False, None, gs.GS_KEY_U32)

            loop_b = rows <= 256
            if loop_b:
                b_nb = lib.gs_topk_temp_bytes(cols, k, hv)
                b_temp = torch.empty(b_nb, dtype=torch.uint8, device=dev)
                b_ko = torch.empty(rows * k, dtype=torch.int32, device=dev)
                b_vo = torch.empty(rows * k, dtype=torch.int32, device=dev)

                def detour_b():
                    for r in range(rows):
                        gs._lib.check(lib.gs_topk_u32(b_temp.data_ptr(), b_nb, keys.data_ptr() + 4 * r * cols, None,
                                                      b_ko.data_ptr() + 4 * r * k, b_vo.data_ptr() + 4 * r * k if hv else None, cols, k, 0,
                                                      gs.GS_KEY_U32, None), "gs_topk_u32")

            rows_call()
            refill()
            detour_a()
            if loop_b:
                detour_b()
            torch.cuda.synchronize()
            t_rows, t_a, t_b = [], [], []
            for _ in range(args.runs):
                t_rows.append(timed(rows_call))
                refill()
                torch.cuda.synchronize()
                t_a.append(timed(detour_a))
                if loop_b:
                    t_b.append(timed(detour_b))
            sk = seg_k.Current().view(rows, cols)[:, :k]
            ok = bool(torch.equal(ko.view(rows, k), sk))
            if hv:
                ok = ok and bool(torch.equal(vo.view(rows, k), seg_v.Current().view(rows, cols)[:, :k]))
            if loop_b:
                ok = ok and bool(torch.equal(ko, b_ko)) and (not hv or bool(torch.equal(vo, b_vo)))
            best = min(t_rows)
            row = {"rows": rows, "cols": cols, "k": k, "dist": dist, "mode": mode, "path": plan[0], "levels": plan[1], "verified": ok,
                   "rows_ms": [round(t, 4) for t in t_rows], "segsort_ms": [round(t, 4) for t in t_a],
                   "rows_best": round(best, 4), "segsort_best": round(min(t_a), 4), "ratio_A": round(min(t_a) / best, 3),
                   "read_rate_TBps": round(4.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            if loop_b:
                row.update({"loop_ms": [round(t, 4) for t in t_b], "loop_best": round(min(t_b), 4), "ratio_B": round(min(t_b) / best, 3)})
                del b_temp, b_ko, b_vo
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, ko, vo
        del keys
    del offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

lost = [[r["rows"], r["cols"], r["k"], r["dist"], r["mode"], side, r[key]] for r in table
        for side, key in (("A", "ratio_A"), ("B", "ratio_B")) if key in r and r[key] <= 1.0]
result = {"bench": "topk_rows_vs_segmented_sort_and_row_loop", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost": lost}))
