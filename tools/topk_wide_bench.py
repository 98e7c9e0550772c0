"""gs_topk_u64 on a flat array of 64-bit keys against the two detours a caller takes without it: sorting the whole column.

    python tools/topk_wide_bench.py [--sizes 2^24,2^28] [--ks 2^10,2^16,2^20] [--runs 5] [--out profiles/topk_wide_bench.json]

One process.  For every input, size n, k and form (keys, arguments): one untimed call of each side, then `runs` rounds with the
sides alternating, each call timed with events on its stream; the best of the runs counts.  Inputs:
  uniform      uniform 64-bit patterns as GS_KEY_U64, smallest first
  normal       doubles drawn from N(0, 1), largest first
  small        int64 below 2^24, smallest first: one top byte for all, bytes 6..3 constant
  timestamps   int64 nanoseconds of one day, latest first
  equal        all keys equal: route 2
Sides:
  (A) gs_msb_sort_wide (unstable, ascending, in place) of a copy of the input, with an index array as 4-byte values for the
      arguments form, keeping the first k (the last k for the inputs taken largest first).  The copy and the fill of the index
      array are not timed.
  (B) gs_lsb_sort_wide (stable, in the direction asked) of a copy, likewise.
After the timed runs the outputs are compared on the device with the first k of (B)'s keys and indices and with (A)'s keys
(`verified`; (A) is unstable, so its indices are not comparable).  Every row, won or lost, goes into the JSON: the times of every
run in ms, `best` of each side, `ratio_A` / `ratio_B` = detour best / gs_topk_u64 best (above 1: the call wins), route, D and
passes from gs_topk_u64_status, and `read_rate_TBps` = 8 bytes per key and pass over the call's best time -- a whole-call figure,
not a kernel's share."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpu_sort_amd as gs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2^24,2^28")
ap.add_argument("--ks", default="2^10,2^16,2^20")
ap.add_argument("--inputs", default="uniform,normal,small,timestamps,equal")
ap.add_argument("--modes", default="keys,args")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
lib = gs.lib
check = gs._lib.check


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
    """(n keys as an int64 tensor of their bit patterns, key type, descending)."""
    g = torch.Generator(device=dev).manual_seed(12345)
    step = 1 << 26
    if kind == "uniform":
        words = torch.empty(2 * n, dtype=torch.int32, device=dev)
        check(lib.gs_generate_u32(words.data_ptr(), words.numel(), gs.GS_GEN_UNIFORM, 12345, 0, 0, None), "gs_generate_u32")
        torch.cuda.synchronize()
        return words.view(torch.int64), gs.GS_KEY_U64, 0
    if kind == "equal":
        return torch.full((n,), 0x3FF0000000000000, dtype=torch.int64, device=dev), gs.GS_KEY_U64, 0
    x = torch.empty(n, dtype=torch.int64, device=dev)
    for lo in range(0, n, step):
        m = min(step, n - lo)
        if kind == "normal":
            x[lo:lo + m] = torch.randn(m, dtype=torch.float64, device=dev, generator=g).view(torch.int64)
        elif kind == "small":
            x[lo:lo + m] = torch.randint(0, 1 << 24, (m,), dtype=torch.int64, device=dev, generator=g)
        else:
            assert kind == "timestamps"
            x[lo:lo + m] = torch.randint(0, 86_400 * 10 ** 9, (m,), dtype=torch.int64, device=dev, generator=g) + 1_718_000_000 * 10 ** 9
    return (x, gs.GS_KEY_F64, 1) if kind == "normal" else (x, gs.GS_KEY_I64, 1 if kind == "timestamps" else 0)


table = []
for n in [num(s) for s in args.sizes.split(",") if s]:
    iota = torch.arange(n, dtype=torch.int64, device=dev).to(torch.int32)    # (u32 bit patterns)
    msb_nb = {hv: lib.gs_msb_wide_temp_bytes(n, 8, 4 * hv) for hv in (0, 1)}
    lsb_nb = {hv: lib.gs_lsb_wide_temp_bytes(n, 8, 4 * hv) for hv in (0, 1)}
    sort_temp = torch.empty(max(list(msb_nb.values()) + list(lsb_nb.values())), dtype=torch.uint8, device=dev)
    kbuf = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
    vbuf = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
    for kind in args.inputs.split(","):
        keys, kt, desc = make_keys(kind, n)
        for k in [num(s) for s in args.ks.split(",") if s]:
            for mode in args.modes.split(","):
                hv = int(mode != "keys")
                nb = lib.gs_topk_u64_temp_bytes(n, k, hv)
                temp = torch.empty(nb, dtype=torch.uint8, device=dev)
                ko = torch.empty(k, dtype=torch.int64, device=dev)
                vo = torch.empty(k, dtype=torch.int32, device=dev)
                where = {}

                def call64():
                    check(lib.gs_topk_u64(temp.data_ptr(), nb, keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None, n, k,
                                          desc, kt, None), "gs_topk_u64")

                def refill():
                    kbuf[0].copy_(keys)
                    if hv:
                        vbuf[0].copy_(iota)

                def detour_a():
                    sk, sv = C.c_void_p(), C.c_void_p()
                    check(lib.gs_msb_sort_wide(sort_temp.data_ptr(), msb_nb[hv], kbuf[0].data_ptr(), vbuf[0].data_ptr() if hv else None, n,
                                               kbuf[1].data_ptr(), vbuf[1].data_ptr() if hv else None, 8, 4 * hv, C.byref(sk),
                                               C.byref(sv), kt, None, 1), "gs_msb_sort_wide")
                    where["a"] = 0 if sk.value == kbuf[0].data_ptr() else 1

                def detour_b():
                    kp = (C.c_void_p * 2)(kbuf[0].data_ptr(), kbuf[1].data_ptr())
                    vp = (C.c_void_p * 2)(vbuf[0].data_ptr(), vbuf[1].data_ptr())
                    sel = C.c_int(0)
                    check(lib.gs_lsb_sort_wide(sort_temp.data_ptr(), lsb_nb[hv], kp, vp if hv else None, C.byref(sel), n, 8, 4 * hv, 0, 64,
                                               desc, kt, None), "gs_lsb_sort_wide")
                    where["b"] = sel.value

                call64()
                refill()
                detour_a()
                refill()
                detour_b()
                torch.cuda.synchronize()
                t64, t_a, t_b = [], [], []
                ok_a = ok_b = True
                for run in range(args.runs):
                    t64.append(timed(call64))
                    refill()
                    t_a.append(timed(detour_a))
                    if run == args.runs - 1:
                        sorted_a = kbuf[where["a"]]
                        ok_a = bool(torch.equal(ko, sorted_a[n - k:].flip(0) if desc else sorted_a[:k]))
                    refill()
                    t_b.append(timed(detour_b))
                ok_b = bool(torch.equal(ko, kbuf[where["b"]][:k])) and (not hv or bool(torch.equal(vo, vbuf[where["b"]][:k])))
                status = gs.DeviceTopK64.Status(temp, n, k, hv)
                best = min(t64)
                row = {"input": kind, "n": n, "k": k, "mode": mode, "descending": desc, "route": status[0], "D": status[5],
                       "passes": status[6], "bucket": status[7], "verified": ok_a and ok_b, "topk_u64_ms": [round(t, 4) for t in t64],
                       "msb_sort_wide_ms": [round(t, 4) for t in t_a], "lsb_sort_wide_ms": [round(t, 4) for t in t_b],
                       "topk_u64_best": round(best, 4), "msb_sort_wide_best": round(min(t_a), 4), "lsb_sort_wide_best": round(min(t_b), 4),
                       "ratio_A": round(min(t_a) / best, 3), "ratio_B": round(min(t_b) / best, 3),
                       "read_rate_TBps": round(8.0 * n * status[6] / (best * 1e-3) / 1e12, 3), "workspace_MiB": round(nb / 2**20, 2)}
                table.append(row)
                print(json.dumps(row), flush=True)
                del temp, ko, vo
        del keys
        torch.cuda.empty_cache()
    del iota, sort_temp, kbuf, vbuf
    torch.cuda.empty_cache()

lost = [[r["input"], r["n"], r["k"], r["mode"], r["ratio_A"], r["ratio_B"]] for r in table if min(r["ratio_A"], r["ratio_B"]) < 1.0]
held = [r for r in table if r["input"] in ("uniform", "normal") and r["n"] >= 1 << 28]
result = {"bench": "topk_u64_vs_msb_sort_wide_and_lsb_sort_wide", "runs": args.runs, "rows": table,
          "all_verified": all(r["verified"] for r in table), "lost": lost,
          "condition_rows": len(held), "condition_met": all(min(r["ratio_A"], r["ratio_B"]) >= 1.0 for r in held)}
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps({"rows": len(table), "all_verified": result["all_verified"], "lost": lost, "condition_met": result["condition_met"]}))
