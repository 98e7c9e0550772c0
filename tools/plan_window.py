"""The two routes of the keys-only plan of gs_lsb_sort_u32 side by side, INSIDE one process on the SAME buffers (placement moves
a sort by +-3 %, profiles/README.md): the library is loaded twice -- once as built, with GS_LSB_PLAN_MIN_ITEMS at its floor so
that every size reaches the plan, and once from a copy whose first sort sees GS_LSB_KEYS_PLAN=classic (both switches are read
once per loaded library) -- and the two sort the same input alternately.  Per case: device time per sort (median, min, max of
the repetitions), what the plan decided, and whether both routes return the same bytes.

    python tools/plan_window.py [--sizes 27,28,29,30,max] [--dists uniform,zipf,...] [--reps 5] [--profile] [--out FILE.json]
                                [--versus classic|stable|nopeek]

--versus stable compares the plan as built (its second scatter in cursor mode) with the plan whose second scatter is the stable
one (the copy's first sort sees GS_LSB_PLAN_SCATTER2=stable) instead of with the four passes; --versus nopeek compares it with
the plan whose host never looks at the decision (GS_LSB_PLAN_PEEK=0: one fixed launch sequence for both routes).  --profile adds the per-kernel-id device times (gs_profile_*) of one more sort per route."""
import argparse, ctypes as C, json, os, shutil, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GS_LSB_PLAN_MIN_ITEMS"] = "65536"
os.environ.pop("GS_LSB_KEYS_PLAN", None)
os.environ.pop("GS_LSB_PLAN_SCATTER2", None)
os.environ.pop("GS_LSB_PLAN_PEEK", None)
import torch
import gpu_sort_amd as gs

N_MAX = 65536 * 16620
DISTS = ("uniform", "zipf", "const", "few4", "sorted", "reverse", "ones_half", "low16", "hot_top_byte", "and2", "and5")
ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="27,28,29,30,max")
ap.add_argument("--dists", default="uniform")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--versus", choices=["classic", "stable", "nopeek"], default="classic")
args = ap.parse_args()
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev); gen.manual_seed(1)


def bind(L):
    L.gs_lsb_temp_bytes.restype = C.c_size_t
    L.gs_lsb_temp_bytes.argtypes = [C.c_uint64, C.c_int]
    L.gs_lsb_sort_u32.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.gs_lsb_plan_status.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p]
    L.gs_profile_create.restype = C.c_void_p
    L.gs_profile_begin.argtypes = [C.c_void_p]
    L.gs_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.gs_kernel_name.restype = C.c_char_p
    return L


def make(kind, n):
    def rnd():
        return torch.randint(-2**31, 2**31, (n,), dtype=torch.int64, device=dev, generator=gen).to(torch.int32)
    if kind == "uniform": return gs.generate_uniform_keys(n, device=dev)
    if kind == "zipf": return gs.generate_zipf_keys(n, device=dev)
    if kind == "const": return torch.full((n,), 123456789, dtype=torch.int32, device=dev)
    if kind == "few4": return rnd()[:4][torch.randint(0, 4, (n,), device=dev, generator=gen)]
    if kind == "sorted": return torch.sort(rnd())[0]
    if kind == "reverse": return torch.sort(rnd(), descending=True)[0]
    if kind == "ones_half":
        k = rnd(); k[torch.rand(n, device=dev, generator=gen) < 0.5] = -1; return k
    if kind == "low16": return rnd() & 0xFFFF
    if kind == "hot_top_byte": return (rnd() & 0x00FFFFFF) | (0x5A << 24)
    k = rnd()
    for _ in range(int(kind[3:])): k &= rnd()
    return k


tmp = tempfile.mkdtemp()
copy = os.path.join(tmp, "libgpusort_classic.so")
shutil.copy(gs.LIB_PATH, copy)
plan_lib = bind(C.CDLL(gs.LIB_PATH))
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sort(L, temp, nb, a, b, n, prof=None):
    keys = (C.c_void_p * 2)(a.data_ptr(), b.data_ptr())
    sel = C.c_int(0)
    if prof: L.gs_profile_begin(prof)
    e = L.gs_lsb_sort_u32(temp.data_ptr(), nb, keys, None, C.byref(sel), n, 0, 32, 0, 0, stream)
    if prof: L.gs_profile_end()
    assert e == 0, e
    return sel.value


# the first sort of each copy fixes its switches
w = gs.generate_uniform_keys(1 << 17, device=dev); wb = torch.empty_like(w)
wt = torch.empty(plan_lib.gs_lsb_temp_bytes(1 << 17, 0), dtype=torch.uint8, device=dev)
sort(plan_lib, wt, wt.numel(), w, wb, 1 << 17)
OTHER = args.versus
switch = {"classic": ("GS_LSB_KEYS_PLAN", "classic"), "stable": ("GS_LSB_PLAN_SCATTER2", "stable"), "nopeek": ("GS_LSB_PLAN_PEEK", "0")}[OTHER]
os.environ[switch[0]] = switch[1]
classic_lib = bind(C.CDLL(copy))
sort(classic_lib, wt, wt.numel(), w, wb, 1 << 17)
torch.cuda.synchronize()
os.environ.pop(switch[0])
libs = (("plan", plan_lib), (OTHER, classic_lib))
rows = []
for size in args.sizes.split(","):
    n = N_MAX if size == "max" else 1 << int(size)
    a, b, keep = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    nb = plan_lib.gs_lsb_temp_bytes(n, 0)
    temp = torch.empty(nb, dtype=torch.uint8, device=dev)
    for dist in args.dists.split(","):
        src = make(dist, n).contiguous()
        ms = {"plan": [], OTHER: []}
        status = (C.c_uint32 * 8)()
        same = None
        for rep in range(args.reps + 1):
            for name, L in libs:
                a.copy_(src); torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); sel = sort(L, temp, nb, a, b, n); e1.record(); e1.synchronize()
                if rep:
                    ms[name].append(e0.elapsed_time(e1))
                elif name == "plan":
                    assert L.gs_lsb_plan_status(temp.data_ptr(), n, status, None) == 0
                    keep.copy_((a, b)[sel])
                else:
                    same = bool(torch.equal(keep, (a, b)[sel])) and gs.check_sorted((a, b)[sel])[0] == 0
        row = {"n": n, "dist": dist, "route": status[0], "largest_group": status[1], "groups": status[2], "same_bytes_and_sorted": same}
        for name in ms:
            v = sorted(ms[name])
            row[name + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        row["plan_over_" + OTHER] = round(row["plan_ms"]["median"] / row[OTHER + "_ms"]["median"], 4)
        if args.profile:
            for name, L in libs:
                prof = C.c_void_p(L.gs_profile_create())
                a.copy_(src); torch.cuda.synchronize()
                sort(L, temp, nb, a, b, n, prof); torch.cuda.synchronize()
                t, c = (C.c_double * 10)(), (C.c_uint64 * 10)()
                L.gs_profile_read(prof, t, c)
                row[name + "_kernels_ms"] = {L.gs_kernel_name(i).decode(): [round(t[i], 4), int(c[i])] for i in range(10) if c[i]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del src
    del a, b, keep, temp
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(rows, f, indent=1)
shutil.rmtree(tmp, ignore_errors=True)
