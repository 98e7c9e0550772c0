"""gs_topk_segmented_u16 on bfloat16 keys against the detours a caller takes without it.

    python tools/topk_segmented_narrow_bench.py [--shapes 2^20x64x8,...] [--ragged lognormal:2^26,...] [--runs 5] [--out profiles/topk_segmented_narrow_bench.json]

One process.  For every set of segments and form (keys, arguments): one untimed call of each side, then `runs` rounds with the
sides alternating, each call timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_narrow (GS_KEY_BF16) with the same offsets on a copy of the keys (positions within the segment as
      values for the arguments form), keeping the first k of every segment.  Neither the copy nor the gather of the first k
      is timed: both omissions favour the detour.
  (B) widening on the device (one conversion kernel, bfloat16 -> float32, which is key << 16 bit for bit) and
      gs_topk_segmented_u32 with GS_KEY_F32 on the result.  The widening is timed: it is part of the detour.
  (C) on equal-length sets only, gs_topk_rows_u16 on the same matrix: the price of taking the lengths from the device.
Sets: those of tools/topk_segmented_bench.py -- regular offsets rows x cols x k; ragged sets of a total size, generated from
a seed (`lognormal`: lengths exp(N(ln 512, 1)) capped at 65536; `zipf`: 4 * Zipf(1.5) capped at 8 * CH) at k = 32 and 256 --
with uniform 16-bit patterns as bfloat16 keys (NaNs of both signs included: every side orders them alike), ascending.
After the timed runs the outputs of every side are compared on the device with every other's (`verified`, and per side).
Every row, won or lost, goes into the JSON: the times of every run in ms, `best` of each side, `ratio_A` / `ratio_B` /
`ratio_C` = detour best / segmented best (above 1: the 16-bit call wins), the list counts of gs_topk_segmented_status, and
`read_rate_TBps` = 2 bytes per key over the 16-bit call's best time.  The condition: every row whose segments all fit CH, and
every ragged row, at least 1.0 x (B); a row that misses it is in `lost`, and every row behind ANY side is in `behind`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

CH = 8192
SHAPES = "2^20x64x8,2^18x1024x64,2^16x4096x64,2^15x8192x256,1024x151936x50,32x2^23x1024"
RAGGED = "lognormal:2^26,lognormal:2^28,zipf:2^26,zipf:2^28"

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=SHAPES)
ap.add_argument("--ragged", default=RAGGED)
ap.add_argument("--ragged-ks", default="32,256")
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


def ragged_lengths(kind, total, seed):
    """Segment lengths of one ragged set: drawn until they fill `total` keys, the last one dropped."""
    rng = np.random.default_rng(seed)
    if kind == "lognormal":
        draw = np.clip(np.exp(rng.normal(np.log(512.0), 1.0, total // 400 + 1000)).astype(np.int64), 1, 65536)
    elif kind == "zipf":
        draw = np.clip(rng.zipf(1.5, total // 20 + 1000) * 4, 1, 8 * CH).astype(np.int64)
    else:
        raise SystemExit("unknown ragged set " + kind)
    count = int(np.searchsorted(np.cumsum(draw), total, side="right"))
    assert 0 < count < draw.size
    return draw[:count]


sets = []       # (name, lengths as int64 numpy, k, equal (rows, cols) or None)
for s in args.shapes.split(","):
    if s:
        rows, cols, k = (num(x) for x in s.split("x"))
        sets.append(("%dx%d" % (rows, cols), np.full(rows, cols, np.int64), k, (rows, cols)))
for s in args.ragged.split(","):
    if s:
        kind, total = s.split(":")
        lengths = ragged_lengths(kind, num(total), args.seed)
        for k in (int(x) for x in args.ragged_ks.split(",")):
            sets.append(("%s:%s" % (kind, total), lengths, k, None))

table = []
for name, lengths, k, equal in sets:
    S, n = int(lengths.size), int(lengths.sum())
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).to(dev)
    begin, end = offsets[:-1], offsets[1:]
    d_len = torch.from_numpy(lengths).to(dev)
    positions = (torch.arange(n, dtype=torch.int64, device=dev) - torch.repeat_interleave(begin.long(), d_len)).to(torch.int32)
    words = torch.empty((n + 1) // 2, dtype=torch.int32, device=dev)       # uniform 32-bit words: two uniform 16-bit keys each
    gs._lib.check(lib.gs_generate_u32(words.data_ptr(), words.numel(), gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    keys = words.view(torch.bfloat16)[:n]
    wide = torch.empty(n, dtype=torch.float32, device=dev)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.bfloat16, device=dev), torch.empty(n, dtype=torch.bfloat16, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_narrow_temp_bytes(n, gs.GS_KEY_BF16, 4 * hv, S) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    kept = torch.clamp(d_len, max=k)
    written = torch.arange(k, device=dev)[None, :] < kept[:, None]                 # [S, k]: the slots a segment fills
    src = (begin.long()[:, None] + torch.arange(k, device=dev)[None, :])[written]   # where (A) has them after its sort
    for mode in args.modes.split(","):
        hv = int(mode != "keys")
        nb = lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        temp = torch.empty(nb, dtype=torch.uint8, device=dev)
        ko = torch.empty(S * k, dtype=torch.int16, device=dev)
        vo = torch.empty(S * k, dtype=torch.int32, device=dev)
        co = torch.empty(S, dtype=torch.int32, device=dev)

        def seg_call():
            gs._lib.check(lib.gs_topk_segmented_u16(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None,
                                                    co.data_ptr(), n, S, begin.data_ptr(), end.data_ptr(), k, 0, gs.GS_KEY_BF16, None),
                          "gs_topk_segmented_u16")

        def refill():          # untimed: the segmented sort works in place on a copy
            seg_k.d_buffers[0].copy_(keys)
            seg_k.selector = 0
            if hv:
                seg_v.d_buffers[0].copy_(positions)
                seg_v.selector = 0

        def detour_a():
            gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, S, begin, end, 0, 16, False, None,
                                              gs.GS_KEY_BF16)

        b_nb = lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        b_temp = torch.empty(b_nb, dtype=torch.uint8, device=dev)
        b_ko = torch.empty(S * k, dtype=torch.int32, device=dev)
        b_vo = torch.empty(S * k, dtype=torch.int32, device=dev)
        b_co = torch.empty(S, dtype=torch.int32, device=dev)

        def detour_b():
            wide.copy_(keys)
            gs._lib.check(lib.gs_topk_segmented_u32(b_temp.data_ptr(), b_nb, wide.data_ptr(), None, b_ko.data_ptr(),
                                                    b_vo.data_ptr() if hv else None, b_co.data_ptr(), n, S, begin.data_ptr(), end.data_ptr(),
                                                    k, 0, gs.GS_KEY_F32, None), "gs_topk_segmented_u32")

        sides = {"seg": seg_call, "A": detour_a, "B": detour_b}
        c_ko = c_vo = None
        if equal:
            rows, cols = equal
            c_nb = lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv)
            c_temp = torch.empty(max(c_nb, 256), dtype=torch.uint8, device=dev)
            c_ko = torch.empty(S * k, dtype=torch.int16, device=dev)
            c_vo = torch.empty(S * k, dtype=torch.int32, device=dev)

            def detour_c():
                gs._lib.check(lib.gs_topk_rows_u16(c_temp.data_ptr(), c_nb, keys.data_ptr(), None, c_ko.data_ptr(),
                                                   c_vo.data_ptr() if hv else None, rows, cols, cols, k, 0, gs.GS_KEY_BF16, None),
                              "gs_topk_rows_u16")
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
        status = gs.DeviceTopKSegmented.Status(temp, n, S, k, hv)
        mine_k = ko.view(S, k)[written]
        mine_v = vo.view(S, k)[written] if hv else None
        ok = {"counts": bool(torch.equal(co.long(), kept)) and status[7] == 0}
        ok["A"] = bool(torch.equal(mine_k, seg_k.Current().view(torch.int16)[src]))
        ok["B"] = bool(torch.equal(mine_k.int() & 0xFFFF, (b_ko.view(S, k)[written] >> 16) & 0xFFFF)) and bool(torch.equal(co, b_co))
        if hv:
            ok["A"] = ok["A"] and bool(torch.equal(mine_v, seg_v.Current()[src]))
            ok["B"] = ok["B"] and bool(torch.equal(mine_v, b_vo.view(S, k)[written]))
        if equal:
            ok["C"] = bool(torch.equal(mine_k, c_ko.view(S, k)[written]))
            ok["C"] = ok["C"] and (not hv or bool(torch.equal(mine_v, c_vo.view(S, k)[written])))
        best = min(times["seg"])
        row = {"set": name, "segments": S, "items": n, "k": k, "mode": mode, "longest": int(lengths.max()), "lists": status,
               "verified": all(ok.values()), "verified_sides": ok, "seg_ms": [round(t, 4) for t in times["seg"]],
               "seg_best": round(best, 4), "read_rate_TBps": round(2.0 * n / (best * 1e-3) / 1e12, 3),
               "workspace_MiB": round(nb / 2**20, 2), "workspace_u32_MiB": round(b_nb / 2**20, 2)}
        for side, label in (("A", "segsort"), ("B", "widen_u32"), ("C", "rows_u16")):
            if side in sides:
                row.update({label + "_ms": [round(t, 4) for t in times[side]], label + "_best": round(min(times[side]), 4),
                            "ratio_" + side: round(min(times[side]) / best, 3)})
        table.append(row)
        print(json.dumps(row), flush=True)
        del temp, ko, vo, co, sides, b_temp, b_ko, b_vo, b_co, mine_k, mine_v
        c_temp = c_ko = c_vo = None      # the detours' buffers go with them
    del offsets, begin, end, d_len, positions, words, keys, wide, seg_k, seg_v, seg_temp, kept, written, src
    torch.cuda.empty_cache()

# the condition: every set whose segments all fit CH, and every ragged set, at least 1.0 x (B)
lost = [[r["set"], r["k"], r["mode"], r["ratio_B"]] for r in table if (r["longest"] <= CH or ":" in r["set"]) and r["ratio_B"] < 1.0]
behind = [[r["set"], r["k"], r["mode"], side, r["ratio_" + side]] for r in table for side in "ABC"
          if r.get("ratio_" + side, 1.0) < 1.0]
result = {"bench": "topk_segmented_u16_vs_segmented_sort_narrow_widening_and_rows_u16", "keys": "bfloat16, uniform 16-bit patterns",
          "runs": args.runs, "seed": args.seed, "rows": table, "all_verified": all(r["verified"] for r in table), "lost": lost,
          "behind": behind}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost": lost, "behind": behind}))
