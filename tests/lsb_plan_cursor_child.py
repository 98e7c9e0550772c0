"""Child process of tests/test_lsb_plan_cursor_gpu.py: runs every case of the cursor-mode second scatter of the keys-only
plan (gs_lsb_plan.hip) in THIS process's mode -- GS_LSB_KEYS_PLAN, GS_LSB_PLAN_SCATTER2 and GS_LSB_PLAN_MIN_ITEMS are read
once per process -- and writes one JSON record per case:

    python tests/lsb_plan_cursor_child.py OUT.json

Each record holds: ok_numpy (the result equals numpy's sort of the order-mapped keys, byte for byte), sha (of the result
bytes), sel (the selector on return), status (gs_lsb_plan_status' eight words), cursor (gs_lsb_plan_cursor_status' four
words), rule (the plan rule restated in numpy), irregular (the tiles the follow-up kernel has to place, counted in numpy:
the full tiles of the d1-sorted key sequence whose first and last d1 differ, plus the partial tile) and guards (guard bands
around both key buffers and the workspace intact).  The parent compares the records of the three modes."""
import ctypes as C
import hashlib
import json
import sys

import numpy as np

from lsb_plan_child import CAP, EDGE_PREFIXES, EDGE_SIZES, F32, I32, U32, f32_specials, grouped, ordmap, plan_rule

TILE = 8192
N_CAMPAIGN = 40


def irregular_tiles(keys, kt, desc):
    """Tiles of the first scatter's output (the keys in d1 order, d1 = bits 16-23 of the mapped key) that the second scatter
    cannot claim from one cursor row: full tiles whose first and last d1 differ, and the partial last tile."""
    d1 = np.sort((ordmap(keys, kt, desc) >> np.uint32(16)) & np.uint32(0xff))
    full = keys.size // TILE
    first, last = d1[0:full * TILE:TILE], d1[TILE - 1:full * TILE:TILE]
    return int((first != last).sum()) + (1 if keys.size % TILE else 0)


def by_groups(rng, sizes):
    """sizes: {(d2, d1): keys} -> shuffled keys with random low 16 bits"""
    parts = []
    for (d2, d1), s in sizes.items():
        top = np.uint32((d2 << 8) | d1) << np.uint32(16)
        parts.append(top | rng.integers(0, 1 << 16, size=s, dtype=np.uint32))
    k = np.concatenate(parts).astype(np.uint32)
    rng.shuffle(k)
    return k


def regions(rng, region_sizes):
    """region_sizes[d1] keys in every d1 region, spread evenly over the 256 d2 (groups of 33 keys at the most here)"""
    sizes = {}
    for d1, s in enumerate(region_sizes):
        for d2 in range(256):
            c = s // 256 + (1 if d2 < s % 256 else 0)
            if c:
                sizes[(d2, d1)] = c
    return by_groups(rng, sizes)


def campaign_case(i):
    """A random layout of at most 2^18 keys: some d1 regions, in each some d2 groups of random sizes; every eighth layout has
    one group above the cap."""
    rng = np.random.default_rng(9000 + i)
    n_target = int(rng.integers(65536, (1 << 18) - 20000))
    d1s = rng.choice(256, int(rng.integers(1, 40)), replace=False)
    sizes, total = {}, 0
    while total < n_target:
        g = (int(rng.integers(0, 256)), int(rng.choice(d1s)))
        if g in sizes:
            continue
        s = int(min(rng.choice([1, 3, 64, 2048, 5000, 8191, 8192, 8193, 17408]), rng.integers(1, 17409)))
        sizes[g] = s
        total += s
    if i % 8 == 7:
        g = next(iter(sizes))
        sizes[g] = int(rng.integers(17409, 20000))
    kt, desc = int(rng.integers(0, 3)), int(rng.integers(0, 2))
    # the layout is one of mapped keys: map back, so that the sort's own map gives these groups
    k = by_groups(rng, sizes)
    if desc:
        k = ~k
    if kt == I32:
        k = k ^ np.uint32(0x80000000)
    elif kt == F32:
        k = np.where(k & np.uint32(0x80000000) != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return k, kt, desc


def make_cases():
    """name -> (keys, key type, descending)"""
    rng = np.random.default_rng(20261)
    uni = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    c = {}
    for n in (65536, 65537, 17 * TILE - 1, (1 << 20) + 4099):
        c["uniform_%d" % n] = (uni(n), U32, 0)
    c["regions_aligned"] = (regions(rng, [TILE] * 256), U32, 0)
    c["region0_8191"] = (regions(rng, [TILE - 1] + [TILE] * 255), U32, 0)
    c["region0_8193"] = (regions(rng, [TILE + 1] + [TILE] * 255), U32, 0)
    c["many_boundaries"] = (regions(rng, [8 * TILE - 400] + [3] * 255), U32, 0)      # 133 boundaries in the last full tile
    sizes = [0] * 256
    for d1, s in ((3, 30000), (77, 8192), (78, 1), (200, 41000), (255, 12345)):
        sizes[d1] = s
    c["empty_regions"] = (regions(rng, sizes), U32, 0)
    hot = {(d2, 0x5a): int(s) for d2, s in zip(range(0, 256, 4), rng.integers(1, CAP[3] + 1, size=64))}
    hot[(0, 0x5a)] = CAP[3]
    c["hot_row"] = (by_groups(rng, hot), U32, 0)
    c["one_d2"] = (by_groups(rng, {(0xc3, d1): int(s) for d1, s in enumerate(rng.integers(1, 4000, size=256))}), U32, 0)
    c["cap_edge_planned"] = (grouped(rng, EDGE_PREFIXES, EDGE_SIZES), U32, 0)
    edge = list(EDGE_SIZES)
    edge[10] = CAP[3] + 1
    c["cap_edge_classic"] = (grouped(rng, EDGE_PREFIXES, edge), U32, 0)
    n = (1 << 17) + 4099
    for kt, name in ((U32, "u32"), (I32, "i32"), (F32, "f32")):
        for desc in (0, 1):
            c["type_%s_%s" % (name, "desc" if desc else "asc")] = (f32_specials(rng, n) if kt == F32 else uni(n), kt, desc)
    n = (1 << 17) + 77
    c["sorted"] = (np.sort(uni(n)), U32, 0)
    c["reversed"] = (np.sort(uni(n))[::-1].copy(), U32, 0)
    for i in range(N_CAMPAIGN):
        c["campaign_%02d" % i] = campaign_case(i)
    return c


def main(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib

    def statuses(ws_ptr, n):
        st, cu = (C.c_uint32 * 8)(), (C.c_uint32 * 4)()
        assert lib.gs_lsb_plan_status(ws_ptr, n, st, None) == 0
        assert lib.gs_lsb_plan_cursor_status(ws_ptr, n, cu, None) == 0
        return list(st), list(cu)

    def run(arena, n, kt, desc, ws_bytes):
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        rc = lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, desc, kt, None)
        assert rc == 0, rc
        st, cu = statuses(arena.ptr("ws"), n)
        torch.cuda.synchronize()
        return sel.value, st, cu

    def record(keys, kt, desc, got, sel, st, cu, guards):
        exp = keys[np.argsort(ordmap(keys, kt, desc), kind="stable")]
        return {"ok_numpy": bool(np.array_equal(got, exp)), "sha": hashlib.sha256(got.tobytes()).hexdigest(), "sel": sel,
                "status": st, "cursor": cu, "rule": plan_rule(keys, kt, desc), "irregular": irregular_tiles(keys, kt, desc),
                "guards": guards, "n": int(keys.size)}

    def guards_ok(arena):
        try:
            arena.check()
            return True
        except AssertionError as e:
            print("guard:", e)
            return False

    res = {}
    for name, (keys, kt, desc) in make_cases().items():
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=3)
        arena.add("k0", 4 * n, data=keys).add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="random").build()
        sel, st, cu = run(arena, n, kt, desc, ws_bytes)
        res[name] = record(keys, kt, desc, arena.read("k%d" % sel, np.uint32), sel, st, cu, guards_ok(arena))

    # one workspace, sort after sort: CLASSIC, PLANNED, PLANNED on other data -- stale cursors and stale lists must not be used
    rng = np.random.default_rng(11)
    n = 17 * TILE + 4099
    ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
    seq = [np.full(n, 0x00070007, np.uint32), rng.integers(0, 1 << 32, size=n, dtype=np.uint32),
           regions(rng, [TILE - 1, TILE + 1, 5, 0, 3 * TILE] + [0] * 250 + [n - 5 * TILE - 5])]
    arena = Arena(dev, seed=4)
    arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="ff").build()
    k0 = arena.slots["k0"][0]
    for i, keys in enumerate(seq):
        arena.mem[k0:k0 + 4 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
        sel, st, cu = run(arena, n, U32, 0, ws_bytes)
        res["reuse_%d" % i] = record(keys, U32, 0, arena.read("k%d" % sel, np.uint32), sel, st, cu, guards_ok(arena))

    # one captured sort, replayed twice; the graph restores the input before the sort
    keys = seq[2]
    src = torch.from_numpy(keys.view(np.int32).copy()).to(dev)
    a, b = torch.empty_like(src), torch.empty_like(src)
    dk = gs.DoubleBuffer(a, b)
    nb = gs.DeviceRadixSort.SortKeys(None, 0, dk, n)
    assert nb == ws_bytes
    temp = torch.empty(nb, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
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
    for i in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        st, cu = statuses(temp.data_ptr(), n)
        res["graph_%d" % i] = record(keys, U32, 0, out.cpu().numpy().view(np.uint32), sel, st, cu, True)

    with open(out_path, "w") as f:
        json.dump(res, f)
    print("cursor child ok", len(res))


if __name__ == "__main__":
    import os
    HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(HERE))
    main(sys.argv[1])
