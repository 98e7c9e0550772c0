"""Child process of tests/test_lsb_plan_gpu.py: runs every case of the keys-only plan of gs_lsb_sort_u32 in THIS process's
mode (GS_LSB_KEYS_PLAN and GS_LSB_PLAN_MIN_ITEMS are read once per process) and writes one JSON record per case:

    python tests/lsb_plan_child.py OUT.json

Each record holds: ok_numpy (the result equals numpy's sort of the key type's order-preserving map, byte for byte),
sha (of the result bytes), sel (the selector on return), status (gs_lsb_plan_status' eight words) and guards (guard bands
around both key buffers and the workspace intact).  The parent compares the records of the two modes."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

U32, I32, F32 = 0, 1, 2
CAP = (2048, 4608, 9216, 17408)          # local-sort classes; CAP[3] is the plan's cap on a group
EDGE_SIZES = [0, 1, 63, 2048, 2049, 4608, 4609, 9216, 9217, 17407, 17408, 17408, 5000, 12000, 2, 64]
EDGE_PREFIXES = [0x0000, 0x0001, 0x00ff, 0x0100, 0x7ffe, 0x7fff, 0x8000, 0x8001, 0x9abc, 0xc000, 0xfffe, 0xffff, 0x1234, 0x4321,
                 0x00fe, 0xff00]


def ordmap(keys, kt, desc):
    """Order-preserving u32 map of the key type (what the sort calls the twiddled key), complemented when descending."""
    k = keys.astype(np.uint32)
    if kt == I32:
        k = k ^ np.uint32(0x80000000)
    elif kt == F32:
        k = np.where(k & np.uint32(0x80000000) != 0, ~k, k | np.uint32(0x80000000)).astype(np.uint32)
    return ~k if desc else k


def plan_rule(keys, kt, desc):
    """The plan rule restated: route, largest group, non-empty groups, tasks per class, keys."""
    sizes = np.bincount(ordmap(keys, kt, desc) >> np.uint32(16), minlength=65536)
    planned = int(sizes.max()) <= CAP[3]
    nz = sizes[sizes > 0]
    cls = np.searchsorted(np.array(CAP), nz, side="left")       # smallest class whose capacity holds the group
    tasks = [int((cls == c).sum()) if planned else 0 for c in range(4)]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    assert offsets[-1] == keys.size
    return [1 if planned else 2, int(sizes.max()), int(nz.size)] + tasks + [int(keys.size)]


def grouped(rng, prefixes, sizes, low=None):
    parts = []
    for p, s in zip(prefixes, sizes):
        lo = rng.integers(0, 1 << 16, size=s, dtype=np.uint32) if low is None else np.full(s, low, np.uint32)
        parts.append((np.uint32(p) << np.uint32(16)) | lo)
    k = np.concatenate(parts).astype(np.uint32)
    rng.shuffle(k)
    return k


def f32_specials(rng, n):
    k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    tiny = np.finfo(np.float32).smallest_subnormal
    sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.nan, -np.nan], np.float32).view(np.uint32)
    sp = np.concatenate([sp, np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32)])          # NaN payloads
    idx = rng.random(n) < 0.5
    k[idx] = sp[rng.integers(0, sp.size, size=int(idx.sum()))]
    return k


def make_cases():
    """name -> (keys, key type, descending, workspace offset, data offset in elements)"""
    rng = np.random.default_rng(20260)
    uni = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    c = {}
    c["cap_edge_planned"] = (grouped(rng, EDGE_PREFIXES, EDGE_SIZES), U32, 0, 0, 0)
    sizes = list(EDGE_SIZES)
    sizes[10] = 17409
    c["cap_edge_classic"] = (grouped(rng, EDGE_PREFIXES, sizes), U32, 0, 0, 0)
    for n in (1 << 17, (1 << 17) + 1, 17 * 8192 - 1, 17 * 8192 + 4099):
        c["size_%d" % n] = (uni(n), U32, 0, 0, 0)
    c["tiny_groups"] = (uni((1 << 20) + 4099), U32, 0, 0, 0)
    n = (1 << 17) + 4099
    for kt, name in ((U32, "u32"), (I32, "i32"), (F32, "f32")):
        for desc in (0, 1):
            keys = f32_specials(rng, n) if kt == F32 else uni(n)
            c["type_%s_%s" % (name, "desc" if desc else "asc")] = (keys, kt, desc, 0, 0)
    n = (1 << 17) + 77
    c["all_equal"] = (np.full(n, 0xdeadbeef, np.uint32), U32, 0, 0, 0)
    c["sorted"] = (np.sort(uni(n)), U32, 0, 0, 0)
    c["reversed"] = (np.sort(uni(n))[::-1].copy(), U32, 0, 0, 0)
    c["low16_constant"] = (grouped(rng, rng.choice(65536, 24, replace=False), [8000 + 37 * i for i in range(24)], low=0x1234), U32, 0, 0, 0)
    c["low16_few_values"] = ((grouped(rng, rng.choice(65536, 12, replace=False), [17000] * 12) & np.uint32(0xffff00ff)), U32, 0, 0, 0)
    c["top16_constant"] = ((uni(n) & np.uint32(0xffff)) | np.uint32(0x80010000), I32, 1, 0, 0)
    c["ws_offset_4"] = (uni((1 << 17) + 4099), U32, 0, 4, 0)
    c["ws_offset_255_data_offset"] = (uni(17 * 8192 + 5), F32, 1, 255, 3)
    return c


def main(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib

    def run(arena, n, kt, desc, ws_bytes):
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        rc = lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, desc, kt, None)
        assert rc == 0, rc
        st = (C.c_uint32 * 8)()
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, None) == 0
        torch.cuda.synchronize()
        return sel.value, list(st)

    def record(keys, kt, desc, got, sel, st, guards):
        exp = keys[np.argsort(ordmap(keys, kt, desc), kind="stable")]
        return {"ok_numpy": bool(np.array_equal(got, exp)), "sha": hashlib.sha256(got.tobytes()).hexdigest(), "sel": sel,
                "status": st, "rule": plan_rule(keys, kt, desc), "guards": guards, "n": int(keys.size)}

    def guards_ok(arena):
        try:
            arena.check()
            return True
        except AssertionError as e:
            print("guard:", e)
            return False

    res = {}
    for name, (keys, kt, desc, ws_off, data_off) in make_cases().items():
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=1)
        arena.add("k0", 4 * n, offset=4 * data_off, data=keys).add("k1", 4 * n, offset=4 * data_off, fill="random")
        arena.add("ws", ws_bytes, offset=ws_off, fill="random").build()
        sel, st = run(arena, n, kt, desc, ws_bytes)
        res[name] = record(keys, kt, desc, arena.read("k%d" % sel, np.uint32), sel, st, guards_ok(arena))

    # one workspace, sort after sort: PLANNED, CLASSIC, PLANNED, CLASSIC -- stale lists and stale decisions must not run
    rng = np.random.default_rng(7)
    n = (1 << 17) + 4099
    ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
    seq = [rng.integers(0, 1 << 32, size=n, dtype=np.uint32), rng.integers(0, 1 << 16, size=n, dtype=np.uint32) | np.uint32(0x00050000),
           grouped(rng, EDGE_PREFIXES, [n // 16] * 15 + [n - 15 * (n // 16)]), np.full(n, 7, np.uint32)]
    arena = Arena(dev, seed=2)
    arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="ff").build()
    k0 = arena.slots["k0"][0]
    for i, keys in enumerate(seq):
        arena.mem[k0:k0 + 4 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
        sel, st = run(arena, n, U32, 0, ws_bytes)
        res["reuse_%d" % i] = record(keys, U32, 0, arena.read("k%d" % sel, np.uint32), sel, st, guards_ok(arena))

    # stream capture: one captured sort replayed on inputs that flip the route
    src = torch.empty(n, dtype=torch.int32, device=dev)
    a, b = torch.empty_like(src), torch.empty_like(src)
    dk = gs.DoubleBuffer(a, b)
    nb = gs.DeviceRadixSort.SortKeys(None, 0, dk, n)
    assert nb == ws_bytes
    temp = torch.empty(nb, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    src.copy_(torch.from_numpy(seq[0].view(np.int32).copy()).to(dev))
    with torch.cuda.stream(side):
        a.copy_(src)
        gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    dk.selector = 0
    with torch.cuda.graph(g, stream=side):
        a.copy_(src)
        gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
    sel = dk.selector
    out = dk.Current()
    for i, keys in enumerate([seq[0], seq[1], seq[1], seq[2]]):
        src.copy_(torch.from_numpy(keys.view(np.int32).copy()).to(dev))
        g.replay()
        torch.cuda.synchronize()
        st = (C.c_uint32 * 8)()
        assert lib.gs_lsb_plan_status(temp.data_ptr(), n, st, None) == 0
        res["graph_%d" % i] = record(keys, U32, 0, out.cpu().numpy().view(np.uint32), sel, list(st), True)

    with open(out_path, "w") as f:
        json.dump(res, f)
    print("plan child ok", len(res))


if __name__ == "__main__":
    main(sys.argv[1])
