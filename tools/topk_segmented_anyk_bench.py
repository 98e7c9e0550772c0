"""gs_topk_segmented_anyk_u32 against the detours a caller with ragged segments and k above gs_topk_rows_max_k() takes without it.

    python tools/topk_segmented_anyk_bench.py [--sets equal,spread,lognormal,zipf,capped] [--runs 5]
                                              [--out profiles/topk_segmented_anyk_bench.json]

One process.  For every set of segments (packed one after the other, lengths drawn on the host with a fixed seed), distribution
(uniform u32 keys smallest first; N(0, 1) floats largest first) and form (keys, positions): one untimed call of each side, then
`runs` rounds with the sides alternating, each call timed with events on its stream; the best of the runs counts.
  (A) gs_segmented_sort_u32 with the same offsets on a copy of the keys (positions within the segment as values for the
      positions form), keeping the first min(k, length) of every segment.  Neither the copy nor the gather is timed: both
      omissions favour the detour.
  (B) on sets of equal lengths, gs_topk_rows_anyk_u32 on the same keys as a matrix: recorded only, the price of lengths that are
      on the device.
  (C) on sets of up to 1024 segments, a host loop of gs_topk_u32 per segment at min(k, length) on one workspace.
  capped: 32 segments of 2^23 at k = 1024 against gs_topk_segmented_u32 itself (ratio_capped).
After the timed runs every segment's outputs and the counts are compared on the device with the first min(k, length) of (A)'s
sorted segments (`verified`), and with (B)'s, (C)'s and the capped call's where they ran.  Every row of the table, won or lost,
goes into the JSON: the times of every run in ms, `best` of each side, ratio_X = detour best / any-k best (above 1: the any-k
call wins), the status words of the call, and `read_rate_TBps` = 4 bytes per key over the any-k call's best time -- a whole-call
figure.  `conditioned` marks the rows the project holds to ratio_A >= 1.0: at least 256 segments of a mean length of at least
65536."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="equal,spread,lognormal,zipf,capped")
ap.add_argument("--dists", default="uniform,normal")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--scale", type=int, default=0, help="divide every set's segment count by 2^scale (a quick look)")
ap.add_argument("--loop-segments", type=int, default=1024, help="detour (C) runs on sets of up to this many segments")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib
SEED = 20262

EQUAL = [(1 << 15, 8192, 2048), (1024, 151936, 4096), (256, 1 << 20, 4096), (32, 1 << 23, 65536)]


def make_sets():
    """-> [(name, lengths (int64 numpy), k, equal)]"""
    rng = np.random.default_rng(SEED)
    sh = args.scale
    sets = []
    for S, mean, k in EQUAL:
        S = max(1, S >> sh)
        if "equal" in args.sets:
            sets.append(("equal %dx%d" % (S, mean), np.full(S, mean, np.int64), k, True))
        if "spread" in args.sets:
            sets.append(("spread %dx%d" % (S, mean), rng.integers(mean // 2, 3 * mean // 2 + 1, S), k, False))
    total = (1 << 28) >> sh
    if "lognormal" in args.sets:
        lens = np.maximum(1, np.exp(rng.normal(np.log(20000.0), 0.6, 2 * total // 20000)).astype(np.int64))
        lens = lens[:int(np.searchsorted(np.cumsum(lens), total))]
        for k in (2000, 12000):
            sets.append(("lognormal 20000", lens, k, False))
    if "zipf" in args.sets:
        S = (1 << 17) >> sh
        w = 1.0 / np.arange(1, S + 1)
        lens = np.maximum(16, (w * (total / w.sum())).astype(np.int64))
        sets.append(("zipf", rng.permutation(lens), 2048, False))
    if "capped" in args.sets:
        sets.append(("capped 32x2^23", np.full(max(1, 32 >> sh), 1 << 23, np.int64), 1024, True))
    return sets


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
for name, lens, k, equal in make_sets():
    S, n = int(lens.size), int(lens.sum())
    assert n < 1 << 31 and S * k < 1 << 31, (name, S, n, k)
    h_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    offsets = torch.from_numpy(h_begin.astype(np.int32)).to(dev)
    d_lens = torch.from_numpy(lens).to(dev)
    kept = torch.clamp(d_lens, max=k)
    # slot (s, i) of the outputs for i < kept[s], and the element begin[s] + i of a sorted copy it must equal
    seg_of = torch.repeat_interleave(torch.arange(S, device=dev), kept)
    within = torch.arange(int(kept.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(kept, 0) - kept, kept)
    out_at = seg_of * k + within
    src_at = offsets[:-1].long()[seg_of] + within
    del seg_of, within
    positions = (torch.arange(n, device=dev) - torch.repeat_interleave(offsets[:-1].long(), d_lens)).to(torch.int32)
    seg_k = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_v = gs.DoubleBuffer(torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    seg_nb = {hv: lib.gs_segmented_temp_bytes(n, hv, S) for hv in (0, 1)}
    seg_temp = torch.empty(max(seg_nb.values()), dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        keys, kt, desc = make_keys(dist, n)
        for mode in args.modes.split(","):
            hv = int(mode != "keys")
            nb = lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, hv)
            temp = torch.empty(nb, dtype=torch.uint8, device=dev)
            ko = torch.full((S * k,), -1, dtype=torch.int32, device=dev)
            vo = torch.full((S * k,), -1, dtype=torch.int32, device=dev)
            co = torch.full((S,), -1, dtype=torch.int32, device=dev)
            plan = gs.DeviceTopKSegmentedAnyK.Plan(n, S, k, hv)

            def anyk_call():
                gs._lib.check(lib.gs_topk_segmented_anyk_u32(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(),
                                                             vo.data_ptr() if hv else None, co.data_ptr(), n, S, offsets.data_ptr(),
                                                             offsets.data_ptr() + 4, k, int(desc), kt, None), "gs_topk_segmented_anyk_u32")

            def refill():          # untimed: the segmented sort works in place on a copy
                seg_k.d_buffers[0].copy_(keys)
                seg_k.selector = 0
                if hv:
                    seg_v.d_buffers[0].copy_(positions)
                    seg_v.selector = 0

            def detour_a():
                gs.DeviceSegmentedRadixSort._sort(seg_temp, seg_nb[hv], seg_k, seg_v if hv else None, n, S, offsets, offsets[1:],
                                                  0, 32, desc, None, kt)

            others = {}            # name -> (call, its keys, its values)
            if equal and name.startswith("equal"):
                cols = int(lens[0])
                b_nb = lib.gs_topk_rows_anyk_temp_bytes(S, cols, k, hv)
                b_temp = torch.empty(b_nb, dtype=torch.uint8, device=dev)
                b_ko, b_vo = torch.full_like(ko, -1), torch.full_like(vo, -1)

                def detour_b():
                    gs._lib.check(lib.gs_topk_rows_anyk_u32(b_temp.data_ptr(), b_nb, keys.data_ptr(), None, b_ko.data_ptr(),
                                                            b_vo.data_ptr() if hv else None, S, cols, cols, k, int(desc), kt, None),
                                  "gs_topk_rows_anyk_u32")
                others["B"] = (detour_b, b_ko, b_vo)
            if S <= args.loop_segments:
                c_nb = max(lib.gs_topk_temp_bytes(int(x), min(k, int(x)), hv) for x in set(lens.tolist()))
                c_temp = torch.empty(c_nb, dtype=torch.uint8, device=dev)
                c_ko, c_vo = torch.full_like(ko, -1), torch.full_like(vo, -1)

                def detour_c():
                    for s in range(S):
                        ln = int(lens[s])
                        gs._lib.check(lib.gs_topk_u32(c_temp.data_ptr(), c_nb, keys.data_ptr() + 4 * int(h_begin[s]), None,
                                                      c_ko.data_ptr() + 4 * s * k, c_vo.data_ptr() + 4 * s * k if hv else None, ln,
                                                      min(k, ln), int(desc), kt, None), "gs_topk_u32")
                others["C"] = (detour_c, c_ko, c_vo)
            if name.startswith("capped"):
                d_nb = lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
                d_temp = torch.empty(d_nb, dtype=torch.uint8, device=dev)
                d_ko, d_vo = torch.full_like(ko, -1), torch.full_like(vo, -1)

                def capped_call():
                    gs._lib.check(lib.gs_topk_segmented_u32(d_temp.data_ptr(), d_nb, keys.data_ptr(), None, d_ko.data_ptr(),
                                                            d_vo.data_ptr() if hv else None, None, n, S, offsets.data_ptr(),
                                                            offsets.data_ptr() + 4, k, int(desc), kt, None), "gs_topk_segmented_u32")
                others["capped"] = (capped_call, d_ko, d_vo)

            anyk_call()
            refill()
            detour_a()
            for fn, _, _ in others.values():
                fn()
            torch.cuda.synchronize()
            status = gs.DeviceTopKSegmentedAnyK.Status(temp, n, S, k, hv)
            t_any, t_a, t_o = [], [], {x: [] for x in others}
            for _ in range(args.runs):
                t_any.append(timed(anyk_call))
                refill()
                torch.cuda.synchronize()
                t_a.append(timed(detour_a))
                for x, (fn, _, _) in others.items():
                    t_o[x].append(timed(fn))
            ok = bool(torch.equal(co.long(), kept)) and bool(torch.equal(ko[out_at], seg_k.Current()[src_at]))
            if hv:
                ok = ok and bool(torch.equal(vo[out_at], seg_v.Current()[src_at]))
            for x, (_, o_k, o_v) in others.items():
                ok = ok and bool(torch.equal(ko[out_at], o_k[out_at])) and (not hv or bool(torch.equal(vo[out_at], o_v[out_at])))
            best = min(t_any)
            row = {"set": name, "segments": S, "items": n, "k": k, "mean_len": round(n / S, 1), "max_len": int(lens.max()),
                   "min_len": int(lens.min()), "dist": dist, "mode": mode, "groups": plan[0], "launches": plan[1], "status": status,
                   "conditioned": S >= 256 and n / S >= 65536, "verified": ok,
                   "anyk_ms": [round(t, 4) for t in t_any], "segsort_ms": [round(t, 4) for t in t_a],
                   "anyk_best": round(best, 4), "segsort_best": round(min(t_a), 4), "ratio_A": round(min(t_a) / best, 3),
                   "read_rate_TBps": round(4.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
            for x, label in (("B", "rows_anyk"), ("C", "loop"), ("capped", "capped")):
                if x in others:
                    row.update({label + "_ms": [round(t, 4) for t in t_o[x]], label + "_best": round(min(t_o[x]), 4),
                                "ratio_" + x: round(min(t_o[x]) / best, 3)})
            table.append(row)
            print(json.dumps(row), flush=True)
            del temp, ko, vo, co, others
        del keys
    del offsets, positions, seg_k, seg_v, seg_temp, out_at, src_at, kept, d_lens
    torch.cuda.empty_cache()

lost = [[r["set"], r["k"], r["dist"], r["mode"], r["ratio_A"]] for r in table if r["ratio_A"] < 1.0]
result = {"bench": "topk_segmented_anyk_vs_segmented_sort_rows_anyk_and_segment_loop", "runs": args.runs, "seed": SEED, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost,
          "condition_met": all(r["ratio_A"] >= 1.0 for r in table if r["conditioned"])}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "condition_met": result["condition_met"], "lost": lost}))
