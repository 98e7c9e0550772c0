"""gs_topk_rows_u64 against the two detours a caller with a matrix of 64-bit keys takes without it.

    python tools/topk_rows_wide_bench.py [--shapes 2^20x64x8,...] [--sets uniform,normal,small] [--runs 5]
                                         [--out profiles/topk_rows_wide_bench.json]

One process.  For every shape (rows, cols, k), key set and form (keys, arguments): one untimed call of each side, then `runs`
rounds with the sides alternating, each call timed with events on its stream; the best of the runs counts.  Key sets:
  uniform   uniform 64-bit words as GS_KEY_U64, smallest first
  normal    N(0, 1) doubles as GS_KEY_F64, largest first
  small     int64 below 2^24 as GS_KEY_I64, smallest first: five bytes are shared, so the kernels leave out five of eight
            passes and rounds -- recorded beside `uniform` so that the effect is on file
  (A) gs_segmented_sort_wide (8-byte keys, 0- or 4-byte values) with regular offsets on a copy of the matrix (column indices
      as values for the arguments form), keeping the first k of every row.  Neither the copy nor the strided gather of the
      first k is timed.
  (B) a host loop of gs_topk_u64, one call per row on one workspace; on the shapes with at most 256 rows.
After the timed runs every row's outputs are compared on the device with the first k of (A)'s sorted rows, and (B)'s too
(`verified`).  Every row of the table, won or lost, goes into the JSON: the times of every run in ms, `best` of each side,
`ratio_A` / `ratio_B` = detour best / rows best (above 1: the rows call wins), the plan, and `read_rate_TBps` = 8 bytes per key
over the rows call's best time -- a whole-call figure, not a kernel's share."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

SHAPES = ("2^20x64x8,2^20x256x8,2^18x1024x64,2^16x4096x64,2^15x8192x256,2^12x65536x100,1024x151936x50,256x2^20x1024,"
          "32x2^23x1024")
LOOP_ROWS = 256       # detour (B) on the shapes with at most this many rows

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--sets", default="uniform,normal,small")
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


def make_keys(kind, n):
    """(n keys as int64 bit patterns, key type, descending)."""
    g = torch.Generator(device=dev)
    g.manual_seed(12345)
    if kind == "uniform":
        hi = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int64, device=dev, generator=g)
        lo = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=dev, generator=g)
        return (hi << 32) | lo, gs.GS_KEY_U64, False
    if kind == "normal":
        return torch.randn(n, dtype=torch.float64, device=dev, generator=g).view(torch.int64), gs.GS_KEY_F64, True
    assert kind == "small"
    return torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device=dev, generator=g), gs.GS_KEY_I64, False


table = []
for rows, cols, k in parse(args.shapes):
    n = rows * cols
    offsets = torch.arange(rows + 1, dtype=torch.int64, device=dev).mul_(cols).to(torch.int32)
    colids = torch.arange(cols, dtype=torch.int32, device=dev).repeat(rows)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_wide_temp_bytes(n, 8, 4 * hv, rows) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for kind in args.sets.split(","):
        keys, kt, desc = make_keys(kind, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.empty(rows * k, dtype=torch.int64, device=dev)
            vo = torch.empty(rows * k, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKRows64.Plan(rows, cols, k, hv)
            loop = rows <= LOOP_ROWS
            if loop:
                nbf = lib.gs_topk_u64_temp_bytes(cols, k, hv)
                tempf = torch.empty(nbf, dtype=torch.uint8, device=dev)
                kof = torch.empty(rows * k, dtype=torch.int64, device=dev)
                vof = torch.empty(rows * k, dtype=torch.int32, device=dev)

            def rows_call():
                gs._lib.check(lib.gs_topk_rows_u64(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                   vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None),
                              "gs_topk_rows_u64")

            def detour_b():
                kin, kout, vout = keys.data_ptr(), kof.data_ptr(), vof.data_ptr()
                for r in range(rows):
                    gs._lib.check(lib.gs_topk_u64(tempf.data_ptr(), nbf, kin + 8 * r * cols, None, kout + 8 * r * k,
                                                  vout + 4 * r * k if hv else None, cols, k, int(desc), kt, None), "gs_topk_u64")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(colids)
                seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, rows, offsets, offsets[1:],
                                                  0, 64, desc, None, kt)

            rows_call()
            if loop:
                detour_b()
            refill()
            detour_a()
            torch.cuda.synchronize()
            t_rows, t_a, t_b = [], [], []
            for _ in range(args.runs):
                t_rows.append(timed(rows_call))
                if loop:
                    t_b.append(timed(detour_b))
                refill()
                torch.cuda.synchronize()
                t_a.append(timed(detour_a))
            got = ko.view(rows, k)
            ok = bool(torch.equal(got, seg_k.Current().view(rows, cols)[:, :k]))
            if hv:
                ok = ok and bool(torch.equal(vo.view(rows, k), seg_v.Current().view(rows, cols)[:, :k]))
            if loop:
                ok = ok and bool(torch.equal(ko, kof)) and (not hv or bool(torch.equal(vo, vof)))
            best = min(t_rows)
            row = {"rows": rows, "cols": cols, "k": k, "set": kind, "mode": mode, "path": plan[0], "levels": plan[1], "verified": ok,
                   "rows_ms": [round(t, 4) for t in t_rows], "segsort_ms": [round(t, 4) for t in t_a],
                   "loop_ms": [round(t, 4) for t in t_b] if loop else None, "rows_best": round(best, 4),
                   "segsort_best": round(min(t_a), 4), "loop_best": round(min(t_b), 4) if loop else None,
                   "ratio_A": round(min(t_a) / best, 3), "ratio_B": round(min(t_b) / best, 3) if loop else None,
                   "read_rate_TBps": round(8.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, ko, vo
            if loop:
                del tempf, kof, vof
        del keys
    del offsets, colids, seg_k, seg_v, seg_temp
    torch.cuda.empty_cache()

lost = [[r["rows"], r["cols"], r["k"], r["set"], r["mode"], r["ratio_A"]] for r in table if r["ratio_A"] < 1.0]
lost_b = [[r["rows"], r["cols"], r["k"], r["set"], r["mode"], r["ratio_B"]] for r in table if r["ratio_B"] is not None and r["ratio_B"] < 1.0]
result = {"bench": "topk_rows_u64_vs_segmented_sort_wide_and_loop_of_topk_u64", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost_to_A": lost, "lost_to_B": lost_b}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost_to_A": lost, "lost_to_B": lost_b}))
