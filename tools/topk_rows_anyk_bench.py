"""gs_topk_rows_anyk_u32 against the two detours a caller with k above gs_topk_rows_max_k() takes without it.

    python tools/topk_rows_anyk_bench.py [--shapes 2^15x8192x2048,...] [--runs 5] [--out profiles/topk_rows_anyk_bench.json]

One process.  For every shape (log2 rows or rows, cols, k), distribution (uniform u32 keys smallest first; N(0, 1) floats
largest first) and form (keys, arguments): one untimed call of each side, then `runs` rounds with the sides alternating, each
call timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_u32 with regular offsets on a copy of the matrix (column indices as values for the arguments form),
      keeping the first k of every row.  Neither the copy nor the strided gather of the first k is timed: both omissions
      favour the detour.
  (B) a host loop of gs_topk_u32 per row on one workspace (what topk_rows() does above the cap), on shapes of up to 1024 rows.
After the timed runs every row's outputs are compared on the device with the first k of (A)'s sorted rows (`verified`), and
with (B)'s where it ran.  Every row of the table, won or lost, goes into the JSON: the times of every run in ms, `best` of each
side, `ratio_A` / `ratio_B` = detour best / any-k best (above 1: the any-k call wins), `ratio_min` = the smaller of the two,
the plan gs_topk_rows_anyk_plan reports, and `read_rate_TBps` = 4 bytes per key over the any-k call's best time -- a
whole-call figure, not a kernel's share.  `conditioned` marks the rows the project holds to ratio_min >= 1.0: at least 256
rows of at least 65536 columns."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

SHAPES = ("2^15x8192x2048,4096x20000x2000,2^12x65536x2048,2^12x65536x8192,1024x151936x2048,1024x151936x4096,256x2^20x4096,"
          "256x2^20x65536,32x2^23x65536")

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--dists", default="uniform,normal")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--loop-rows", type=int, default=1024, help="detour (B) runs on shapes of up to this many rows")
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
    """-> (int32 bit patterns, key type, descending)"""
    if dist == "normal":
        g = torch.Generator(device=dev).manual_seed(12345)
        keys = torch.randn(n, dtype=torch.float32, device=dev, generator=g).view(torch.int32)
        torch.cuda.synchronize()
        return keys, gs.GS_KEY_F32, True
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    gs._lib.check(lib.gs_generate_u32(keys.data_ptr(), n, gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    torch.cuda.synchronize()
    return keys, gs.GS_KEY_U32, False


table = []
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_temp_bytes(n, hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        keys, kt, desc = make_keys(dist, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.empty(rows * k, dtype=torch.int32, device=dev)
            vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKRowsAnyK.Plan(rows, cols, k, hv)

            def anyk_call():
                gs._lib.check(lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                        vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None),
                              "gs_topk_rows_anyk_u32")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(colids)
                    seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                                  0, 32, desc, None, kt)

            loop_b = rows <= args.loop_rows
            if loop_b:
                b_nb = lib.gs_topk_temp_bytes(cols, k, hv)
                b_temp = torch.empty(b_nb, dtype=torch.uint8, device=dev)
                b_ko = torch.empty(rows * k, dtype=torch.int32, device=dev)
                b_vo = torch.empty(rows * k, dtype=torch.int32, device=dev)

                def detour_b():
                    for r in range(rows):
                        gs._lib.check(lib.gs_topk_u32(b_temp.data_ptr(), b_nb, keys.data_ptr() + 4 * r * cols, None,
                                                      b_ko.data_ptr() + 4 * r * k, b_vo.data_ptr() + 4 * r * k if hv else None, cols, k,
                                                      int(desc), kt, None), "gs_topk_u32")

            anyk_call()
            refill()
            detour_a()
            if loop_b:
                detour_b()
            torch.cuda.synchronize()
            t_any, t_a, t_b = [], [], []
            for _ in range(args.runs):
                t_any.append(timed(anyk_call))
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
            best = min(t_any)
            row = {"rows": rows, "cols": cols, "k": k, "dist": dist, "mode": mode, "path": plan[0], "launches": plan[1],
                   "tiles_per_slab": plan[4], "slabs_per_row": plan[5], "conditioned": rows >= 256 and cols >= 65536, "verified": ok,
                   "anyk_ms": [round(t, 4) for t in t_any], "segsort_ms": [round(t, 4) for t in t_a],
                   "anyk_best": round(best, 4), "segsort_best": round(min(t_a), 4), "ratio_A": round(min(t_a) / best, 3),
                   "read_rate_TBps": round(4.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            ratios = [row["ratio_A"]]
            if loop_b:
                row.update({"loop_ms": [round(t, 4) for t in t_b], "loop_best": round(min(t_b), 4), "ratio_B": round(min(t_b) / best, 3)})
                ratios.append(row["ratio_B"])
                del b_temp, b_ko, b_vo
            row["ratio_min"] = min(ratios)
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, ko, vo
        del keys
    del offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

lost = [[r["rows"], r["cols"], r["k"], r["dist"], r["mode"], r["ratio_min"]] for r in table if r["ratio_min"] < 1.0]
result = {"bench": "topk_rows_anyk_vs_segmented_sort_and_row_loop", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost,
          "condition_met": all(r["ratio_min"] >= 1.0 for r in table if r["conditioned"])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "condition_met": result["condition_met"], "lost": lost}))
