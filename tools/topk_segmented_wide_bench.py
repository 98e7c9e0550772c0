"""gs_topk_segmented_u64 against the detours a caller with ragged segments of 64-bit keys takes without it.

    python tools/topk_segmented_wide_bench.py [--shapes 2^20x64x8,...] [--layouts equal,spread] [--sets uniform,normal,small]
                                              [--runs 5] [--out profiles/topk_segmented_wide_bench.json]

One process.  For every shape (segments, mean length, k), layout, key set and form (keys, arguments): one untimed call of each
side, then `runs` rounds with the sides alternating, each call timed with events on its stream; the best of the runs counts.
Layouts: `equal` (every segment has the mean length) and `spread` (lengths uniform in [mean / 2, 3 * mean / 2] from a seed, the
same number of segments); the shape of 32 segments of 2^23 is run in the equal layout only.  Key sets:
  uniform   uniform 64-bit words as GS_KEY_U64, smallest first
  normal    N(0, 1) doubles as GS_KEY_F64, largest first
  small     int64 below 2^24 as GS_KEY_I64, smallest first: five bytes are shared, so the kernels leave out five of eight
            passes and rounds -- recorded beside `uniform` (`skip_ratio` = uniform best / small best per shape, layout and form)
  (A) gs_segmented_sort_wide (8-byte keys, 0- or 4-byte values) with the same offsets on a copy of the keys (positions within
      the segment as values for the arguments form), keeping the first k of every segment.  Neither the copy nor the gather of
      the first k is timed: both omissions favour the detour.
  (B) on the equal layout only, gs_topk_rows_u64 on the same matrix: the price of taking the lengths from the device.
  (C) on the shapes with at most 256 segments, a host loop of gs_topk_u64, one call per segment on one workspace (possible
      here because the host made the offsets).
After the timed runs the outputs are compared on the device with the first kept of (A)'s sorted segments, with (B)'s and with
(C)'s (`verified`, and per side), the counts with min(k, length).  Every row, won or lost, goes into the JSON: the times of
every run in ms, `best` of each side, `ratio_A` / `ratio_B` / `ratio_C` = detour best / segmented best (above 1: the segmented
call wins), the list counts of gs_topk_segmented_status, and `read_rate_TBps` = 8 bytes per key over the call's best time -- a
whole-call figure, not a kernel's share.  The condition: on every row whose mean length is between 4096 and 2^20, ratio_A
above 1; a row that misses it is in `lost`, and every row behind ANY side is in `behind`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

SHAPES = ("2^20x64x8,2^18x1024x64,2^16x4096x64,2^15x8192x256,2^12x65536x100,1024x151936x50,256x2^20x1024,"
          "32x2^23x1024")
LOOP_SEGMENTS = 256       # detour (C) on the shapes with at most this many segments
EQUAL_ONLY = 1 << 23      # a mean length from which only the equal layout is run

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--layouts", default="equal,spread")
ap.add_argument("--sets", default="uniform,normal,small")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib


def num(s):
    return 1 << int(s[2:]) if s.startswith("2^") else int(s)


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


def lengths_of(layout, segments, mean, seed):
    if layout == "equal":
        return np.full(segments, mean, np.int64)
    assert layout == "spread"
    return np.random.default_rng(seed).integers(mean // 2, mean + mean // 2 + 1, segments).astype(np.int64)


sets = []       # (segments, mean, k, layout, lengths)
for s in args.shapes.split(","):
    if s:
        segments, mean, k = (num(x) for x in s.split("x"))
        for layout in args.layouts.split(","):
            if layout == "equal" or mean < EQUAL_ONLY:
                sets.append((segments, mean, k, layout, lengths_of(layout, segments, mean, args.seed)))

table = []
for segments, mean, k, layout, lengths in sets:
    S, n = int(lengths.size), int(lengths.sum())
    assert n < 1 << 31
    h_off = np.concatenate([[0], np.cumsum(lengths)])
    offsets = torch.from_numpy(h_off.astype(np.int32)).to(dev)
    begin, end = offsets[:-1], offsets[1:]
    d_len = torch.from_numpy(lengths).to(dev)
    positions = (torch.arange(n, dtype=torch.int64, device=dev) - torch.repeat_interleave(begin.long(), d_len)).to(torch.int32)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_wide_temp_bytes(n, 8, 4 * hv, S) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    kept = torch.clamp(d_len, max=k)
    written = torch.arange(k, device=dev)[None, :] < kept[:, None]                 # [S, k]: the slots a segment fills
    src = (begin.long()[:, None] + torch.arange(k, device=dev)[None, :])[written]   # where (A) has them after its sort
    loop = S <= LOOP_SEGMENTS
    for kind in args.sets.split(","):
        keys, kt, desc = make_keys(kind, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.empty(S * k, dtype=torch.int64, device=dev)
            vo = torch.empty(S * k, dtype=torch.int32, device=dev)
            co = torch.empty(S, dtype=torch.int32, device=dev)

            def seg_call():
                gs._lib.check(lib.gs_topk_segmented_u64(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                        vo.data_ptr() if hv else None, co.data_ptr(), n, S, begin.data_ptr(),
                                                        end.data_ptr(), k, int(desc), kt, None), "gs_topk_segmented_u64")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(positions)
                seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, S, begin, end, 0, 64, desc, None, kt)

            sides = {"seg": seg_call, "A": detour_a}
            if layout == "equal":
                b_nb = lib.gs_topk_rows_u64_temp_bytes(S, mean, k, hv)
                b_temp = torch.empty(max(b_nb, 256), dtype=torch.uint8, device=dev)
                b_ko = torch.empty(S * k, dtype=torch.int64, device=dev)
                b_vo = torch.empty(S * k, dtype=torch.int32, device=dev)

                def detour_b():
                    gs._lib.check(lib.gs_topk_rows_u64(b_temp.data_ptr(), b_nb, keys.data_ptr(), None, b_ko.data_ptr(),
                                                       b_vo.data_ptr() if hv else None, S, mean, mean, k, int(desc), kt, None),
                                  "gs_topk_rows_u64")
                sides["B"] = detour_b
            if loop:
                c_nb = max(lib.gs_topk_u64_temp_bytes(int(ln), min(k, int(ln)), hv) for ln in set(lengths.tolist()))
                c_temp = torch.empty(c_nb, dtype=torch.uint8, device=dev)
                c_ko = torch.empty(S * k, dtype=torch.int64, device=dev)
                c_vo = torch.empty(S * k, dtype=torch.int32, device=dev)

                def detour_c():
                    kin, kout, vout = keys.data_ptr(), c_ko.data_ptr(), c_vo.data_ptr()
                    for s_ in range(S):
                        ln = int(lengths[s_])
                        gs._lib.check(lib.gs_topk_u64(c_temp.data_ptr(), c_nb, kin + 8 * int(h_off[s_]), None, kout + 8 * s_ * k,
                                                      vout + 4 * s_ * k if hv else None, ln, min(k, ln), int(desc), kt, None), "gs_topk_u64")
                sides["C"] = detour_c

            for side, fn in sides.items():
                if side == "A":
                    refill()
                fn()
            torch.cuda.synchronize()
            times = {side: [] for side in sides}
            for _ in range(args.runs):
                for side, fn in sides.items():
                    if side == "A":
                        refill()
                        torch.cuda.synchronize()
                    times[side].append(timed(fn))
            status = gs.DeviceTopKSegmented64.Status(temp, n, S, k, hv)
            mine_k = ko.view(S, k)[written]
            mine_v = vo.view(S, k)[written] if hv else None
            ok = {"counts": bool(torch.equal(co.long(), kept)) and status[7] == 0}
            ok["A"] = bool(torch.equal(mine_k, seg_k.Current()[src])) and (not hv or bool(torch.equal(mine_v, seg_v.Current()[src])))
            if "B" in sides:
                ok["B"] = bool(torch.equal(ko, b_ko)) and (not hv or bool(torch.equal(vo, b_vo)))
            if loop:
                ok["C"] = bool(torch.equal(mine_k, c_ko.view(S, k)[written])) and (not hv or bool(torch.equal(mine_v, c_vo.view(S, k)[written])))
            best = min(times["seg"])
            row = {"segments": S, "mean": mean, "k": k, "layout": layout, "items": n, "set": kind, "mode": mode,
                   "longest": int(lengths.max()), "lists": status, "verified": all(ok.values()), "verified_sides": ok,
                   "seg_ms": [round(t, 4) for t in times["seg"]], "seg_best": round(best, 4),
                   "read_rate_TBps": round(8.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            for side, label in (("A", "segsort"), ("B", "rows_u64"), ("C", "loop")):
                if side in sides:
                    row.update({label + "_ms": [round(t, 4) for t in times[side]], label + "_best": round(min(times[side]), 4),
                                "ratio_" + side: round(min(times[side]) / best, 3)})
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, ko, vo, co, sides, mine_k, mine_v
            b_temp = b_ko = b_vo = c_temp = c_ko = c_vo = None      # the detours' buffers go with them
        del keys
    del offsets, begin, end, d_len, positions, seg_k, seg_v, seg_temp, kept, written, src
    torch.cuda.empty_cache()


def key_of(r):
    return (r["segments"], r["mean"], r["k"], r["layout"], r["mode"])


uniform = {key_of(r): r["seg_best"] for r in table if r["set"] == "uniform"}
skip = [list(key_of(r)) + [round(uniform[key_of(r)] / r["seg_best"], 3)] for r in table if r["set"] == "small" and key_of(r) in uniform]
lost = [[r["segments"], r["mean"], r["k"], r["layout"], r["set"], r["mode"], r["ratio_A"]] for r in table
        if 4096 <= r["mean"] <= 1 << 20 and r["ratio_A"] <= 1.0]
behind = [[r["segments"], r["mean"], r["k"], r["layout"], r["set"], r["mode"], side, r["ratio_" + side]] for r in table for side in "ABC"
          if r.get("ratio_" + side, 2.0) <= 1.0]
result = {"bench": "topk_segmented_u64_vs_segmented_sort_wide_rows_u64_and_loop_of_topk_u64", "runs": args.runs, "seed": args.seed,
          "rows": table, "all_verified": all(r["verified"] for r in table), "lost": lost, "behind": behind, "skip_ratio": skip}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost": lost, "behind": behind, "skip_ratio": skip}))
