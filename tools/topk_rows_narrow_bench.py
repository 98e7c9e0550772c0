"""gs_topk_rows_u16 on bfloat16 keys against the two detours a caller takes without it.

    python tools/topk_rows_narrow_bench.py [--shapes 2^20x64x8,...] [--runs 5] [--out profiles/topk_rows_narrow_bench.json]

One process.  For every shape (rows, cols, k) and form (keys, arguments): one untimed call of each side, then `runs` rounds
with the sides alternating, each call timed with events on its stream; the best of the runs counts.  Keys are uniform 16-bit
patterns read as bfloat16 (GS_KEY_BF16), ascending.
  (B) the detour through this library's own rows top-k: widen on the device (x.view(int16).to(int32) << 16), then
      gs_topk_rows_u32 with GS_KEY_F32.  The widening is timed: it is what such a caller pays.
  (A) gs_segmented_sort_narrow (GS_KEY_BF16) with regular offsets on a copy of the matrix (column indices as values for the
      arguments form), keeping the first k of every row.  Neither the copy nor the strided gather of the first k is timed.
After the timed runs every row's outputs are compared on the device with (B)'s (keys shifted back) and with the first k of
(A)'s sorted rows (`verified`).  Every row of the table, won or lost, goes into the JSON: the times of every run in ms, `best`
of each side, `ratio_B` / `ratio_A` = detour best / rows best (above 1: the 16-bit call wins), the plan, and `read_rate_TBps`
= 2 bytes per key over the 16-bit call's best time -- a whole-call figure, not a kernel's share."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

SHAPES = "2^20x64x8,2^20x256x8,2^18x1024x64,2^16x4096x64,2^15x8192x256,2^12x65536x100,1024x151936x50,256x2^20x1024"

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
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


def make_keys(n):
    """n uniform 16-bit patterns, as bfloat16."""
    words = torch.empty((n + 1) // 2, dtype=torch.int32, device=dev)
    gs._lib.check(lib.gs_generate_u32(words.data_ptr(), words.numel(), gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    torch.cuda.synchronize()
    return words.view(torch.bfloat16)[:n]


table = []
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_narrow_temp_bytes(n, gs.GS_KEY_BF16, 4 * hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    keys = make_keys(n)
    for mode in args.modes.split(","):
        hv = int(mode != "keys")
        nb = lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv)
        nb32 = lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        temp32 = torch.empty(nb32, dtype=torch.uint8, device=dev)
        ko = torch.empty(rows * k, dtype=torch.bfloat16, device=dev)
        vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
        ko32 = torch.empty(rows * k, dtype=torch.int32, device=dev)
        vo32 = torch.empty(rows * k, dtype=torch.int32, device=dev)
        plan = gs.DeviceTopKRows.Plan(rows, cols, k, hv)

        def rows_call():
            gs._lib.check(lib.gs_topk_rows_u16(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None,
                                               rows, cols, cols, k, 0, gs.GS_KEY_BF16, None), "gs_topk_rows_u16")

        def detour_b():
            wide = keys.view(torch.int16).to(torch.int32) << 16
            gs._lib.check(lib.gs_topk_rows_u32(temp32.data_ptr(), nb32, wide.data_ptr(), None, ko32.data_ptr(),
                                               vo32.data_ptr() if hv else None, rows, cols, cols, k, 0, gs.GS_KEY_F32, None),
                          "gs_topk_rows_u32")

        def refill():          # untimed: the segmented sort works in place on a copy
            seg_k.d_buffers[0].copy_(keys)
            seg_k.selector = 0
            if hv:
                seg_v.d_buffers[0].copy_(colids)
            seg_v.selector = 0

        def detour_a():
            gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                              0, 16, False, None, gs.GS_KEY_BF16)

        rows_call()
        detour_b()
        refill()
        detour_a()
        torch.cuda.synchronize()
        t_rows, t_a, t_b = [], [], []
        for _ in range(args.runs):
            t_rows.append(timed(rows_call))
            t_b.append(timed(detour_b))
            refill()
            torch.cuda.synchronize()
            t_a.append(timed(detour_a))
        got = ko.view(torch.int16).view(rows, k)
        ok_b = bool(torch.equal(got, (ko32 >> 16).to(torch.int16).view(rows, k))) and bool((ko32 & 0xFFFF).eq(0).all())
        ok_a = bool(torch.equal(got, seg_k.Current().view(torch.int16).view(rows, cols)[:, :k]))
        if hv:
            ok_b = ok_b and bool(torch.equal(vo, vo32))
            ok_a = ok_a and bool(torch.equal(vo.view(rows, k), seg_v.Current().view(rows, cols)[:, :k]))
        best = min(t_rows)
        row = {"rows": rows, "cols": cols, "k": k, "mode": mode, "path": plan[0], "levels": plan[1], "verified": ok_a and ok_b,
               "rows_ms": [round(t, 4) for t in t_rows], "widen_u32_ms": [round(t, 4) for t in t_b],
               "segsort_ms": [round(t, 4) for t in t_a], "rows_best": round(best, 4), "widen_u32_best": round(min(t_b), 4),
               "segsort_best": round(min(t_a), 4), "ratio_B": round(min(t_b) / best, 3), "ratio_A": round(min(t_a) / best, 3),
               "read_rate_TBps": round(2.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
        table.append(row)
        print(json.dumps(row), flush=True)
        del temp, temp32, ko, vo, ko32, vo32
    del keys, offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

lost = [[r["rows"], r["cols"], r["k"], r["mode"], r["ratio_B"]] for r in table if r["ratio_B"] < 1.0]
result = {"bench": "topk_rows_u16_bf16_vs_widen_then_rows_u32_and_segmented_sort_narrow", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost_to_B": lost}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost_to_B": lost}))
