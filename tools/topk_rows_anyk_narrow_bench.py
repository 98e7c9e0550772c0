"""gs_topk_rows_anyk_u16 on bfloat16 keys against the three detours a caller with k above gs_topk_rows_max_k() takes without it.

    python tools/topk_rows_anyk_narrow_bench.py [--shapes 2^15x8192x2048,...] [--runs 5] [--out profiles/topk_rows_anyk_narrow_bench.json]

One process.  For every shape (log2 rows or rows, cols, k), distribution (uniform 16-bit patterns read as bfloat16, smallest
first; N(0, 1) rounded to bfloat16, largest first) and form (keys, arguments): one untimed call of each side, then `runs` rounds
with the sides alternating, each call timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_narrow (GS_KEY_BF16) with regular offsets on a copy of the matrix (column indices as values for the
      arguments form), keeping the first k of every row.  Neither the copy nor the strided gather of the first k is timed: both
      omissions favour the detour.
  (B) widen on the device (x.view(int16).to(int32) << 16), then gs_topk_rows_anyk_u32 with GS_KEY_F32.  The widening is timed:
      it is what such a caller pays.
  (C) a host loop of gs_topk_u16 per row on one workspace, on shapes of up to 1024 rows.
After the timed runs every row's outputs are compared on the device with the first k of (A)'s sorted rows, with (B)'s (keys
shifted back) and with (C)'s where it ran (`verified`).  Every row of the table, won or lost, goes into the JSON: the times of
every run in ms, `best` of each side, `ratio_A` / `ratio_B` / `ratio_C` = detour best / any-k best (above 1: the any-k call
wins), `ratio_min` = the smallest of them, the plan gs_topk_rows_anyk_u16_plan reports, and `read_rate_TBps` = 2 bytes per key
over the any-k call's best time -- a whole-call figure, not a kernel's share.  `conditioned` marks the rows the project holds to
ratio_min >= 1.0: at least 256 rows of at least 65536 columns."""
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
ap.add_argument("--loop-rows", type=int, default=1024, help="detour (C) runs on shapes of up to this many rows")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib
BF16 = gs.GS_KEY_BF16


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
    """-> (n bfloat16 keys, descending)"""
    if dist == "normal":
        g = torch.Generator(device=dev).manual_seed(12345)
        keys = torch.randn(n, dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
        torch.cuda.synchronize()
        return keys, True
    words = torch.empty((n + 1) // 2, dtype=torch.int32, device=dev)
    gs._lib.check(lib.gs_generate_u32(words.data_ptr(), words.numel(), gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    torch.cuda.synchronize()
    return words.view(torch.bfloat16)[:n], False


table = []
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_narrow_temp_bytes(n, BF16, 4 * hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        keys, desc = make_keys(dist, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, hv)
            nb32 = lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            temp32 = torch.empty(nb32, dtype=torch.uint8, device=dev)
            ko = torch.empty(rows * k, dtype=torch.bfloat16, device=dev)
            vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
            ko32 = torch.empty(rows * k, dtype=torch.int32, device=dev)
            vo32 = torch.empty(rows * k, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKRowsAnyK16.Plan(rows, cols, k, hv)

            def anyk_call():
                gs._lib.check(lib.gs_topk_rows_anyk_u16(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                        vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), BF16, None),
                              "gs_topk_rows_anyk_u16")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(colids)
                seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                                  0, 16, desc, None, BF16)

            def detour_b():
                wide = keys.view(torch.int16).to(torch.int32) << 16
                gs._lib.check(lib.gs_topk_rows_anyk_u32(temp32.data_ptr(), nb32, wide.data_ptr(), None, ko32.data_ptr(),
                                                        vo32.data_ptr() if hv else None, rows, cols, cols, k, int(desc), gs.GS_KEY_F32,
                                                        None), "gs_topk_rows_anyk_u32")

            loop_c = rows <= args.loop_rows
            if loop_c:
                c_nb = lib.gs_topk_u16_temp_bytes(cols, k, hv)
                c_temp = torch.empty(c_nb, dtype=torch.uint8, device=dev)
                c_ko = torch.empty(rows * k, dtype=torch.bfloat16, device=dev)
                c_vo = torch.empty(rows * k, dtype=torch.int32, device=dev)

                def detour_c():
                    for r in range(rows):
                        gs._lib.check(lib.gs_topk_u16(c_temp.data_ptr(), c_nb, keys.data_ptr() + 2 * r * cols, None,
                                                      c_ko.data_ptr() + 2 * r * k, c_vo.data_ptr() + 4 * r * k if hv else None, cols, k,
                                                      int(desc), BF16, None), "gs_topk_u16")

            anyk_call()
            detour_b()
            refill()
            detour_a()
            if loop_c:
                detour_c()
            torch.cuda.synchronize()
            t_any, t_a, t_b, t_c = [], [], [], []
            for _ in range(args.runs):
                t_any.append(timed(anyk_call))
                t_b.append(timed(detour_b))
                refill()
                torch.cuda.synchronize()
                t_a.append(timed(detour_a))
                if loop_c:
                    t_c.append(timed(detour_c))
            got = ko.view(torch.int16).view(rows, k)
            ok = bool(torch.equal(got, seg_k.Current().view(torch.int16).view(rows, cols)[:, :k]))
            ok = ok and bool(torch.equal(got, (ko32 >> 16).to(torch.int16).view(rows, k))) and bool((ko32 & 0xFFFF).eq(0).all())
            if hv:
                ok = ok and bool(torch.equal(vo.view(rows, k), seg_v.Current().view(rows, cols)[:, :k])) and bool(torch.equal(vo, vo32))
            if loop_c:
                ok = ok and bool(torch.equal(ko.view(torch.int16), c_ko.view(torch.int16))) and (not hv or bool(torch.equal(vo, c_vo)))
            best = min(t_any)
            row = {"rows": rows, "cols": cols, "k": k, "dist": dist, "mode": mode, "path": plan[0], "launches": plan[1],
                   "tiles_per_slab": plan[4], "slabs_per_row": plan[5], "conditioned": rows >= 256 and cols >= 65536, "verified": ok,
                   "anyk_ms": [round(t, 4) for t in t_any], "segsort_ms": [round(t, 4) for t in t_a],
                   "widen_u32_ms": [round(t, 4) for t in t_b], "anyk_best": round(best, 4), "segsort_best": round(min(t_a), 4),
                   "widen_u32_best": round(min(t_b), 4), "ratio_A": round(min(t_a) / best, 3), "ratio_B": round(min(t_b) / best, 3),
                   "read_rate_TBps": round(2.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            ratios = [row["ratio_A"], row["ratio_B"]]
            if loop_c:
                row.update({"loop_ms": [round(t, 4) for t in t_c], "loop_best": round(min(t_c), 4), "ratio_C": round(min(t_c) / best, 3)})
                ratios.append(row["ratio_C"])
                del c_temp, c_ko, c_vo
            row["ratio_min"] = min(ratios)
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, temp32, ko, vo, ko32, vo32
        del keys
    del offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

lost = [[r["rows"], r["cols"], r["k"], r["dist"], r["mode"], r["ratio_min"]] for r in table if r["ratio_min"] < 1.0]
result = {"bench": "topk_rows_anyk_u16_bf16_vs_segmented_sort_narrow_widen_then_anyk_u32_and_row_loop", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost,
          "condition_met": all(r["ratio_min"] >= 1.0 for r in table if r["conditioned"])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "condition_met": result["condition_met"], "lost": lost}))
