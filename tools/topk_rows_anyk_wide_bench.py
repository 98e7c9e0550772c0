"""gs_topk_rows_anyk_u64 against the two detours a caller with 64-bit keys and k above gs_topk_rows_max_k() takes without it.

    python tools/topk_rows_anyk_wide_bench.py [--shapes 2^15x8192x2048,...] [--runs 5] [--out profiles/topk_rows_anyk_wide_bench.json]

One process.  For every shape (log2 rows or rows, cols, k), input (uniform u64, smallest first; N(0, 1) doubles, largest first;
int64 below 2^24, smallest first) and form (keys, arguments): one untimed call of each side, then `runs` rounds with the sides
alternating, each call timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_wide with regular offsets on a copy of the matrix (column indices as values for the arguments form),
      keeping the first k of every row.  Neither the copy nor the strided gather of the first k is timed: both omissions
      favour the detour.
  (B) a host loop of gs_topk_u64 per row on one workspace -- what topk_rows64() runs above its cap --, on shapes of up to 1024
      rows.
After the timed runs every row's outputs are compared on the device with the first k of (A)'s sorted rows and with (B)'s where
it ran (`verified`).  Every row of the table, won or lost, goes into the JSON: the times of every run in ms, `best` of each
side, `ratio_A` / `ratio_B` = detour best / any-k best (above 1: the any-k call wins), `ratio_best` = against the faster detour
that ran, the plan and row 0's status (D, how the descent ended, the list count, and `passes` = the reads of the matrix: D + 3
from the list, D + 2 for a tie run, 1 on path 1), and `read_rate_TBps` = 8 bytes per key over the any-k call's best time -- a
whole-call figure, not a kernel's share.  `conditioned` marks the rows the project holds to ratio_best >= 1.0: at least 256
rows of at least 65536 columns.  `small_vs_uniform` is, per shape and form, the any-k time on int64 below 2^24 over the time on
uniform words: whether leaving out the constant bits pays.  `kernel_times` splits one path-2 call by the library's timing hook
(one category for the select's launches, the finish's own categories)."""
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
ap.add_argument("--dists", default="uniform,normal,small")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--loop-rows", type=int, default=1024, help="detour (B) runs on shapes of up to this many rows")
ap.add_argument("--profile-shape", default="1024x151936x4096", help="the path-2 shape whose call is split by the timing hook")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib
KEY_TYPE = {"uniform": gs.GS_KEY_U64, "normal": gs.GS_KEY_F64, "small": gs.GS_KEY_I64}


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
    """-> (n 8-byte keys as int64 bit patterns, descending)"""
    g = torch.Generator(device=dev).manual_seed(12345)
    if dist == "normal":
        keys = torch.randn(n, dtype=torch.float64, device=dev, generator=g).view(torch.int64)
    elif dist == "small":
        keys = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device=dev, generator=g)
    else:
        keys = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), dtype=torch.int64, device=dev, generator=g)
    torch.cuda.synchronize()
    return keys, dist == "normal"


table, kernel_times = [], None
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_wide_temp_bytes(n, 8, 4 * hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        keys, desc = make_keys(dist, n)
        kt = KEY_TYPE[dist]
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.empty(rows * k, dtype=torch.int64, device=dev)
            vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKRowsAnyK64.Plan(rows, cols, k, hv)

            def anyk_call():
                gs._lib.check(lib.gs_topk_rows_anyk_u64(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                        vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None),
                              "gs_topk_rows_anyk_u64")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(colids)
                seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                                  0, 64, desc, None, kt)

            loop_b = rows <= args.loop_rows
            if loop_b:
                b_nb = lib.gs_topk_u64_temp_bytes(cols, k, hv)
                b_temp = torch.empty(b_nb, dtype=torch.uint8, device=dev)
                b_ko = torch.empty(rows * k, dtype=torch.int64, device=dev)
                b_vo = torch.empty(rows * k, dtype=torch.int32, device=dev)

                def detour_b():
                    for r in range(rows):
                        gs._lib.check(lib.gs_topk_u64(b_temp.data_ptr(), b_nb, keys.data_ptr() + 8 * r * cols, None,
                                                      b_ko.data_ptr() + 8 * r * k, b_vo.data_ptr() + 4 * r * k if hv else None, cols, k,
                                                      int(desc), kt, None), "gs_topk_u64")

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
            got = ko.view(rows, k)
            ok = bool(torch.equal(got, seg_k.Current().view(rows, cols)[:, :k]))
            if hv:
                ok = ok and bool(torch.equal(vo.view(rows, k), seg_v.Current().view(rows, cols)[:, :k]))
            if loop_b:
                ok = ok and bool(torch.equal(ko, b_ko)) and (not hv or bool(torch.equal(vo, b_vo)))
            st = gs.DeviceTopKRowsAnyK64.Status(temp, rows, cols, k, hv, 0)
            best = min(t_any)
            row = {"rows": rows, "cols": cols, "k": k, "dist": dist, "mode": mode, "path": plan[0], "launches": plan[1],
                   "list_cap": plan[7], "D": st[5], "end": st[6], "list": st[7],
                   "passes": 1 if plan[0] == 1 else st[5] + (3 if st[6] == 1 else 2),
                   "conditioned": rows >= 256 and cols >= 65536, "verified": ok,
                   "anyk_ms": [round(t, 4) for t in t_any], "segsort_ms": [round(t, 4) for t in t_a],
                   "anyk_best": round(best, 4), "segsort_best": round(min(t_a), 4), "ratio_A": round(min(t_a) / best, 3),
                   "read_rate_TBps": round(8.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            ratios = [row["ratio_A"]]
            if loop_b:
                row.update({"loop_ms": [round(t, 4) for t in t_b], "loop_best": round(min(t_b), 4), "ratio_B": round(min(t_b) / best, 3)})
                ratios.append(row["ratio_B"])
                del b_temp, b_ko, b_vo
            row["ratio_best"] = min(ratios)
            table.append(row)
            print(json.dumps(row), flush=True)
            if kernel_times is None and (rows, cols, k) == parse(args.profile_shape)[0] and plan[0] == 2:
                torch.cuda.synchronize()
                prof = gs.KernelProfile()
                with prof:
                    anyk_call()
                    torch.cuda.synchronize()
                kernel_times = {"shape": [rows, cols, k], "dist": dist, "mode": mode,
                                "by_category_ms_launches": {name: [round(ms, 4), cnt] for name, (ms, cnt) in prof.read().items()}}
                prof.close()
                print(json.dumps(kernel_times), flush=True)
            del temp, ko, vo
        del keys
    del offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

small_vs_uniform = []
for r in table:
    if r["dist"] == "small":
        u = [x for x in table if x["dist"] == "uniform" and (x["rows"], x["cols"], x["k"], x["mode"]) == (r["rows"], r["cols"], r["k"], r["mode"])]
        if u:
            small_vs_uniform.append([r["rows"], r["cols"], r["k"], r["mode"], round(r["anyk_best"] / u[0]["anyk_best"], 3)])
lost = [[r["rows"], r["cols"], r["k"], r["dist"], r["mode"], r["ratio_best"]] for r in table if r["ratio_best"] < 1.0]
result = {"bench": "topk_rows_anyk_u64_vs_segmented_sort_wide_and_row_loop_of_topk_u64", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost, "small_vs_uniform": small_vs_uniform,
          "kernel_times": kernel_times,
          "condition_met": all(r["ratio_best"] >= 1.0 for r in table if r["conditioned"])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "condition_met": result["condition_met"], "lost": lost,
                  "small_vs_uniform": small_vs_uniform}))
