"""The look and the finish of the keys-only plan, each measured ALONE, builds and one-pass grids (GS_LSB_PLAN_ONEPASS_GRID)
alternating INSIDE one process on the SAME buffers (placement moves a kernel by several percent from one allocation to the
next, profiles/README.md).  Written to try the look with loads in flight across its unit epilogue, the one-pass local sort
with its task records two ahead and its zeroing before the wait for the keys, and the one-pass launch's grid, one at a
time (only the grid was kept).

    python tools/lookahead_ab.py [--log2n 30] [--reps 9] [--out FILE.json] SPEC SPEC ...

SPEC = LABEL=LIBRARY[@GRID]: a library inside gpu-sort_amd/lib (libgpusort.so, or a variant built with other -D switches),
loaded from a private copy so that every SPEC has its own process-wide switches; @GRID sets GS_LSB_PLAN_ONEPASS_GRID for that
copy's first sort (the value is read once per loaded library).

Per input -- uniform, zipf, and few40 (top 16 bits uniform, low 16 bits from 40 values: the one-pass sort leaves every group
over) -- and per SPEC, in microseconds, median / min / max of the repetitions:
  look    gs_lsb_plan_look_only (look, reduction, decision) between two events         [uniform, zipf]
  finish  the local sorts of a whole sort, from the library's own per-kernel event hook  [uniform, few40]
  sort    the whole sort between two events                                             [uniform, few40]
One JSON line per input; the first repetition of every SPEC is a warm-up and is left out."""
import argparse, ctypes as C, json, os, shutil, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("GS_LSB_PLAN_ONEPASS_GRID", None)
import torch
import gpu_sort_amd as gs

ap = argparse.ArgumentParser()
ap.add_argument("--log2n", type=int, default=30)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--out", default=None)
ap.add_argument("specs", nargs="+")
args = ap.parse_args()
dev = torch.device("cuda:0")
n = 1 << args.log2n
libdir = os.path.join(ROOT, "gpu-sort_amd", "lib")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
LOCAL = [i for i in range(10) if gs.lib.gs_kernel_name(i) == b"msb_local_sort"]
assert len(LOCAL) == 1, "the local sorts' kernel id"


def bind(L):
    L.gs_lsb_sort_u32.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.gs_lsb_plan_look_only.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    L.gs_profile_create.restype = C.c_void_p
    L.gs_profile_begin.argtypes = [C.c_void_p]
    L.gs_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    return L


a, b = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
nb = gs.lib.gs_lsb_temp_bytes(n, 0)
temp = torch.empty(nb, dtype=torch.uint8, device=dev)


def sort(L, prof=None):
    keys = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    sel = C.c_int(0)
    if prof: L.gs_profile_begin(prof)
    e = L.gs_lsb_sort_u32(temp.data_ptr(), nb, keys, None, C.byref(sel), n, 0, 32, 0, 0, stream)
    if prof: L.gs_profile_end()
    assert e == 0, e
    return (a, b)[sel.value]


tmp = tempfile.mkdtemp()
libs = []
warm = gs.generate_uniform_keys(n, device=dev)
for i, spec in enumerate(args.specs):
    label, rest = spec.split("=", 1)
    name, _, grid = rest.partition("@")
    copy = os.path.join(tmp, "gsab_%d.so" % i)
    shutil.copy(os.path.join(libdir, name), copy)
    if grid: os.environ["GS_LSB_PLAN_ONEPASS_GRID"] = grid
    L = bind(C.CDLL(copy))
    a.copy_(warm)
    sort(L)                                     # the copy's first sort fixes its switches
    torch.cuda.synchronize()
    os.environ.pop("GS_LSB_PLAN_ONEPASS_GRID", None)
    libs.append((label, L, C.c_void_p(L.gs_profile_create())))
del warm


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}


def few40():
    g = torch.Generator(device=dev); g.manual_seed(5)
    values = torch.randint(0, 1 << 16, (40,), device=dev, generator=g, dtype=torch.int32)
    return (gs.generate_uniform_keys(n, device=dev) & -65536) | values[torch.randint(0, 40, (n,), device=dev, generator=g)]


rows = []
for dist, make in (("uniform", lambda: gs.generate_uniform_keys(n, device=dev)), ("zipf", lambda: gs.generate_zipf_keys(n, device=dev)), ("few40", few40)):
    src = make().contiguous()
    _, want_sum, want_xor = gs.check_sorted(src)
    row = {"n": n, "dist": dist}
    if dist != "few40":
        us = {label: [] for label, _, _ in libs}
        for rep in range(args.reps + 1):
            for label, L, _ in libs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                e = L.gs_lsb_plan_look_only(temp.data_ptr(), src.data_ptr(), b.data_ptr(), n, 0, 0, stream)
                e1.record(); e1.synchronize()
                assert e == 0, e
                if rep: us[label].append(e0.elapsed_time(e1) * 1e3)
        row["look_us"] = {k: stats(v) for k, v in us.items()}
    if dist != "zipf":
        fin = {label: [] for label, _, _ in libs}
        tot = {label: [] for label, _, _ in libs}
        for rep in range(args.reps + 1):
            for label, L, prof in libs:
                a.copy_(src); torch.cuda.synchronize()
                ms0, c0, ms1, c1 = (C.c_double * 10)(), (C.c_uint64 * 10)(), (C.c_double * 10)(), (C.c_uint64 * 10)()
                L.gs_profile_read(prof, ms0, c0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out = sort(L, prof); e1.record(); e1.synchronize()
                L.gs_profile_read(prof, ms1, c1)
                if rep:
                    fin[label].append((ms1[LOCAL[0]] - ms0[LOCAL[0]]) * 1e3)
                    tot[label].append(e0.elapsed_time(e1) * 1e3)
                else:
                    inv, got_sum, got_xor = gs.check_sorted(out)
                    assert inv == 0 and got_sum == want_sum and got_xor == want_xor, (dist, label)
        row["finish_us"] = {k: stats(v) for k, v in fin.items()}
        row["sort_us"] = {k: stats(v) for k, v in tot.items()}
    rows.append(row)
    print(json.dumps(row), flush=True)
    del src
if args.out:
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
shutil.rmtree(tmp, ignore_errors=True)
