"""gs_topk_u16 on a flat array of bfloat16 keys against the two detours a caller takes without it.

    python tools/topk_narrow_bench.py [--sizes 2^24,2^28,2^30] [--ks 2^10,2^16,2^20] [--runs 5] [--out profiles/topk_narrow_bench.json]

One process.  For every input, size n, k and form (keys, arguments): one untimed call of each side, then `runs` rounds with the
sides alternating, each call timed with events on its stream; the best of the runs counts.  Inputs (GS_KEY_BF16):
  uniform    uniform 16-bit patterns, smallest first
  normal     bfloat16 scores drawn from N(0, 1), largest first: the realistic case; the route depends on k and is reported
  onebyte    keys that all share one top byte (random low byte), smallest first: route 2
Sides:
  (A) gs_lsb_sort_narrow of the whole input (GS_KEY_BF16), with an index array as 4-byte values for the arguments form, keeping
      the first k.  The fill of the index array is not timed.
  (B) widen on the device (x.view(int16).to(int32) << 16), then gs_topk_u32 with GS_KEY_F32.  The widening is timed: it is what
      such a caller pays.
After the timed runs the outputs are compared on the device with the first k of (A)'s and with (B)'s (keys shifted back)
(`verified`).  Every row, won or lost, goes into the JSON: the times of every run in ms, `best` of each side, `ratio_A` /
`ratio_B` = detour best / gs_topk_u16 best (above 1: the 16-bit call wins), the route from gs_topk_u16_status, and
`read_rate_TBps` = 2 bytes per key over the call's best time -- a whole-call figure, not a kernel's share."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2^24,2^28,2^30")
ap.add_argument("--ks", default="2^10,2^16,2^20")
ap.add_argument("--inputs", default="uniform,normal,onebyte")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib
BF16 = gs.GS_KEY_BF16


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
    """(n bfloat16 keys, descending)."""
    if kind == "normal":
        g = torch.Generator(device=dev).manual_seed(12345)
        x = torch.empty(n, dtype=torch.bfloat16, device=dev)
        step = 1 << 26
        for lo in range(0, n, step):
            x[lo:lo + step] = torch.randn(min(step, n - lo), dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
        return x, 1
    words = torch.empty((n + 1) // 2, dtype=torch.int32, device=dev)
    gs._lib.check(lib.gs_generate_u32(words.data_ptr(), words.numel(), gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
    if kind == "onebyte":
        words.bitwise_and_(0x00FF00FF).bitwise_or_(0x3F003F00)
    torch.cuda.synchronize()
    return words.view(torch.bfloat16)[:n], 0


table = []
for n in [num(s) for s in args.sizes.split(",") if s]:
    iota = torch.arange(n, dtype=torch.int64, device=dev).to(torch.int32) if "args" in args.modes else None    # (u32 bit patterns)
    sort_nb = {hv: lib.gs_lsb_narrow_temp_bytes(n, BF16, 4 * hv) for hv in (0, 1)}
    sort_temp = torch.empty(max(sort_nb.values()), dtype=torch.uint8, device=dev)
    sorted_k = torch.empty(n, dtype=torch.bfloat16, device=dev)
    sorted_v = torch.empty(n, dtype=torch.int32, device=dev) if iota is not None else None
    for kind in args.inputs.split(","):
        keys, desc = make_keys(kind, n)
        for k in [num(s) for s in args.ks.split(",") if s]:
            for mode in args.modes.split(","):
                hv = int(mode != "keys")
                nb, nb32 = lib.gs_topk_u16_temp_bytes(n, k, hv), lib.gs_topk_temp_bytes(n, k, hv)
                temp = torch.empty(nb, dtype=torch.uint8, device=dev)
                temp32 = torch.empty(nb32, dtype=torch.uint8, device=dev)
                ko = torch.empty(k, dtype=torch.bfloat16, device=dev)
                vo, ko32, vo32 = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(3))

                def call16():
                    gs._lib.check(lib.gs_topk_u16(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None,
                                                  n, k, desc, BF16, None), "gs_topk_u16")

                def detour_a():
                    gs._lib.check(lib.gs_lsb_sort_narrow(sort_temp.data_ptr(), sort_nb[hv], keys.data_ptr(), sorted_k.data_ptr(),
                                                         iota.data_ptr() if hv else None, sorted_v.data_ptr() if hv else None, n, BF16,
                                                         4 * hv, 0, 16, desc, None), "gs_lsb_sort_narrow")

                def detour_b():
                    wide = keys.view(torch.int16).to(torch.int32) << 16
                    gs._lib.check(lib.gs_topk_u32(temp32.data_ptr(), nb32, wide.data_ptr(), None, ko32.data_ptr(),
                                                  vo32.data_ptr() if hv else None, n, k, desc, gs.GS_KEY_F32, None), "gs_topk_u32")

                call16()
                detour_a()
                detour_b()
                torch.cuda.synchronize()
                t16, t_a, t_b = [], [], []
                for _ in range(args.runs):
                    t16.append(timed(call16))
                    t_a.append(timed(detour_a))
                    t_b.append(timed(detour_b))
                status = gs.DeviceTopK16.Status(temp, n, k, hv)
                got = ko.view(torch.int16)
                ok_a = bool(torch.equal(got, sorted_k.view(torch.int16)[:k]))
                ok_b = bool(torch.equal(got, (ko32 >> 16).to(torch.int16))) and bool((ko32 & 0xFFFF).eq(0).all())
                if hv:
                    ok_a = ok_a and bool(torch.equal(vo, sorted_v[:k]))
                    ok_b = ok_b and bool(torch.equal(vo, vo32))
                best = min(t16)
                row = {"input": kind, "n": n, "k": k, "mode": mode, "descending": desc, "route": status[0], "top_byte_bucket": status[4],
                       "verified": ok_a and ok_b, "topk_u16_ms": [round(t, 4) for t in t16], "sort_narrow_ms": [round(t, 4) for t in t_a],
                       "widen_u32_ms": [round(t, 4) for t in t_b], "topk_u16_best": round(best, 4), "sort_narrow_best": round(min(t_a), 4),
                       "widen_u32_best": round(min(t_b), 4), "ratio_A": round(min(t_a) / best, 3), "ratio_B": round(min(t_b) / best, 3),
                       "read_rate_TBps": round(2.0 * n / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
                table.append(row)
                print(json.dumps(row), flush=True)
                del temp, temp32, ko, vo, ko32, vo32
        del keys
        torch.cuda.empty_cache()
    del iota, sort_temp, sorted_k, sorted_v
    torch.cuda.empty_cache()

lost = [[r["input"], r["n"], r["k"], r["mode"], r["ratio_A"], r["ratio_B"]] for r in table if min(r["ratio_A"], r["ratio_B"]) < 1.0]
held = [r for r in table if r["input"] in ("uniform", "normal") and r["n"] >= 1 << 28]
result = {"bench": "topk_u16_bf16_vs_sort_narrow_and_widen_then_topk_u32", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost,
          "condition_rows": len(held), "condition_met": all(min(r["ratio_A"], r["ratio_B"]) >= 1.0 for r in held)}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost": lost, "condition_met": result["condition_met"]}))
