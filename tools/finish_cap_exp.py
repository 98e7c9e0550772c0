"""The grid cap of the keys-only plan's two leftover local-sort launches (gs_lsb_plan_finish_cap, GS_LSB_PLAN_FINISH_CAP):
what it costs and saves at the two ends, 2^LOG2N keys each.

    python tools/finish_cap_exp.py run [LOG2N] [REPS] [--root TREE]     sorts to put under rocprofv3 --kernel-trace
    python tools/finish_cap_exp.py summary TRACE_DIR                     per-launch times from that run's kernel trace

run: REPS sorts of uniform keys (nothing is left over: both launches find `flagged == 0`), then REPS sorts of keys whose top
16 bits are uniform and whose low 16 bits come from 40 values (every group is left over: the few-distinct-values launch
finishes all of them), each event-timed; prints one JSON line.  The cap is read once per process, so one process per value:
GS_LSB_PLAN_FINISH_CAP=512|1024|2048.  --root: the tree whose package is loaded (another build, e.g. one without the cap).
summary: per input, the mean duration of the few-distinct-values launch (local-sort MODE 3), the flagged launch (MODE 2) and
the one-pass launch (MODE 1), and the kernel time of a whole sort."""
import csv
import glob
import json
import os
import re
import sys


def run(log2n, reps, root):
    sys.path.insert(0, root)
    import torch
    import gpu_sort_amd as gs
    dev = torch.device("cuda:0")
    n = 1 << log2n
    uni = gs.generate_uniform_keys(n, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    values = torch.randint(0, 1 << 16, (40,), device=dev, generator=g, dtype=torch.int32)
    few = (uni & -65536) | values[torch.randint(0, 40, (n,), device=dev, generator=g)]
    a, b = torch.empty_like(uni), torch.empty_like(uni)
    nb = gs.lib.gs_lsb_temp_bytes(n, 0)
    temp = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = {"log2n": log2n, "cap": int(gs.lib.gs_lsb_plan_finish_cap()) if hasattr(gs.lib, "gs_lsb_plan_finish_cap") else None,
           "lib": gs.LIB_PATH}
    for name, src in (("uniform", uni), ("few40", few)):
        _, want_sum, want_xor = gs.check_sorted(src)
        ms = []
        for _ in range(reps + 1):
            a.copy_(src)
            dk = gs.DoubleBuffer(a, b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 4))
        inv, got_sum, got_xor = gs.check_sorted(dk.Current())
        assert inv == 0 and got_sum == want_sum and got_xor == want_xor, name
        out[name] = {"ms": ms[1:], "first_ms": ms[0]}
    print(json.dumps(out))


def summary(trace_dir):
    path = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    sorts, cur = [], None
    for r in rows:
        name = r["Kernel_Name"]
        if "lsb_plan_look_kernel" in name:
            cur = {"total": 0.0}
            sorts.append(cur)
        if cur is None or not re.search(r"gs::(lsb_|msb_)", name):
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        cur["total"] += us
        m = re.search(r"msb_local_sort_kernel<\d+, \d+, false, false, (\d)", name)
        if m:
            cur["mode%s" % m.group(1)] = cur.get("mode%s" % m.group(1), 0.0) + us
        for k in ("msb_task_sample_kernel", "lsb_plan_irregular_kernel"):
            if k in name:
                cur[k] = us
    half = len(sorts) // 2
    for tag, part in (("uniform", sorts[1:half]), ("few40", sorts[half + 1:])):      # (the first sort of each input left out)
        keys = sorted(set().union(*part))
        print(tag, "sorts", len(part), " ".join("%s %.1f us" % (k, sum(s.get(k, 0.0) for s in part) / len(part)) for k in keys))


if __name__ == "__main__":
    if sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        args = [x for x in sys.argv[2:] if not x.startswith("--")]
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if "--root" in sys.argv:
            root = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
            args = [x for x in args if os.path.abspath(x) != root]
        run(int(args[0]) if args else 30, int(args[1]) if len(args) > 1 else 4, root)
