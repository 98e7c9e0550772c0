"""Child process of tests/test_lsb_plan_fused_gpu.py: the fused look of the keys-only plan (gs_lsb_plan.hip) in THIS
process's mode (GS_LSB_KEYS_PLAN and GS_LSB_PLAN_MIN_ITEMS are read once per process); one JSON record per case:

    python tests/lsb_plan_fused_child.py OUT.json

look_*  gs_lsb_plan_look_only alone, on a workspace of random bytes: the spine and prefix16 it leaves against numpy (per-tile
        bincount of bits 16-23 of the mapped keys, exclusive prefix over the tiles of a chunk, chunk totals), word for word,
        and the first sixteen words of the plan block.  They run before any sort.  With the plan switched off the hook must
        refuse: that process records the one case look_refused.
sort_*, reuse_*, graph_*  whole sorts, recorded as tests/lsb_plan_child.py records them."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lsb_plan_child import F32, I32, U32, f32_specials, ordmap, plan_rule  # noqa: E402

TILE, CHUNK_TILES, RADIX = 8192, 8, 256
CHUNK = TILE * CHUNK_TILES
N_ONE = CHUNK                                   # one chunk, two look workgroups
N_TWO_TILES = 9 * TILE + 1                      # the second chunk holds two tiles, the last of one key
N_255, N_256 = 255 * CHUNK, 256 * CHUNK         # one chunk fewer than, and as many chunks as, look workgroups
N_257 = 257 * CHUNK + 3 * TILE + 5              # more chunks than workgroups, ragged last chunk and tile
N_WALK = 3 * (1 << 23) + 3 * TILE + 5           # 385 chunks = 193 units of two chunks: more chunks than one round of the grid holds
# A look workgroup counts LOOK_UNIT_CHUNKS chunks at a time (one unit) and walks the units slot, slot + grid, ...; between two
# units it writes the unit's results and clears its wave counters.  N_THREE_UNITS has more than two units per workgroup of the
# full grid, so that every workgroup walks at least two and some walk three, with a ragged last chunk and tile.
LOOK_GRID, LOOK_UNIT_CHUNKS = 256, 2
N_THREE_UNITS = (2 * LOOK_GRID * LOOK_UNIT_CHUNKS + 5) * CHUNK + 3 * TILE + 5   # 1030 chunks = 515 units
N_SPECIAL = 1 << 24
INVALID_VALUE = 1                               # hipErrorInvalidValue


def unmap(m, kt, desc):
    """Inverse of ordmap."""
    m = (~m if desc else m).astype(np.uint32)
    if kt == I32:
        return m ^ np.uint32(0x80000000)
    if kt == F32:
        return np.where(m & np.uint32(0x80000000) != 0, m ^ np.uint32(0x80000000), ~m).astype(np.uint32)
    return m


def look_reference(keys, kt, desc):
    """(spine [256][grid] u32, prefix16 [tiles][256] u16) of a pass on bits 16-23 of the mapped keys."""
    n = keys.size
    tiles = (n + TILE - 1) // TILE
    grid = max((tiles + CHUNK_TILES - 1) // CHUNK_TILES, 1)
    digit = ((ordmap(keys, kt, desc) >> np.uint32(16)) & np.uint32(0xFF)).astype(np.int64)
    digit += (np.arange(n, dtype=np.int64) // TILE) * RADIX
    counts = np.zeros((grid * CHUNK_TILES, RADIX), np.int64)
    counts[:tiles] = np.bincount(digit, minlength=tiles * RADIX).reshape(tiles, RADIX)
    per_chunk = counts.reshape(grid, CHUNK_TILES, RADIX)
    incl = np.cumsum(per_chunk, axis=1)
    prefix = (incl - per_chunk).reshape(grid * CHUNK_TILES, RADIX)[:tiles].astype(np.uint16)
    spine = incl[:, -1, :].T.astype(np.uint32).copy()          # [256][grid]
    return spine, prefix


def planted(rng, n, prefix, size):
    """Uniform keys with exactly `size` keys whose top 16 bits are `prefix`."""
    k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    hit = (k >> np.uint32(16)) == np.uint32(prefix)
    k[hit] ^= np.uint32(0x00010000)
    at = rng.choice(n, size, replace=False)
    k[at] = (k[at] & np.uint32(0xFFFF)) | (np.uint32(prefix) << np.uint32(16))
    return k


def look_cases(rng):
    """name -> (keys, key type, descending, workspace offset)"""
    uni = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    c = {}
    for n in (N_ONE, N_TWO_TILES, N_255, N_256, N_257, N_WALK, N_THREE_UNITS):
        c["look_uniform_%d" % n] = (uni(n), U32, 0, 4 if n == N_TWO_TILES else 0)
    n = N_SPECIAL
    c["look_sorted"] = (np.sort(uni(n)), U32, 0, 0)                                  # every wave shares one group
    runs = ((np.arange(n, dtype=np.uint32) >> np.uint32(4)) & np.uint32(0xFFFF)) << np.uint32(16)
    c["look_runs_of_16"] = (runs | rng.integers(0, 1 << 16, size=n, dtype=np.uint32), U32, 0, 0)   # 16 lanes share a group
    c["look_i32_desc"] = (uni(n), I32, 1, 0)
    c["look_f32_specials"] = (f32_specials(rng, n), F32, 0, 0)
    return c


def main(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib
    plan_on = os.environ.get("GS_LSB_KEYS_PLAN") != "classic"
    res = {}

    def guards_ok(arena):
        try:
            arena.check()
            return True
        except AssertionError as e:
            print("guard:", e)
            return False

    # ---- the look alone, before any sort
    cases = look_cases(np.random.default_rng(20261)) if plan_on else {"look_refused": (np.zeros(N_ONE, np.uint32), U32, 0, 0)}
    for name, (keys, kt, desc, ws_off) in cases.items():
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=3)
        arena.add("k0", 4 * n, data=keys, const=True).add("k1", 4 * n, fill="ff").add("ws", ws_bytes, offset=ws_off, fill="random").build()
        lay = (C.c_uint64 * 4)()
        rc_layout = lib.gs_lsb_plan_layout(n, lay)
        rc = lib.gs_lsb_plan_look_only(arena.ptr("ws"), arena.ptr("k0"), arena.ptr("k1"), n, kt, desc, None)
        torch.cuda.synchronize()
        if not plan_on:
            res[name] = {"refused": rc == INVALID_VALUE and rc_layout == INVALID_VALUE, "guards": guards_ok(arena)}
            continue
        assert rc == 0 and rc_layout == 0, (rc, rc_layout)
        spine_off, prefix_off, plan_off, grid = (int(x) for x in lay)
        base = ((arena.ptr("ws") + 255) & ~255) - arena.mem.data_ptr()
        tiles = (n + TILE - 1) // TILE
        read = lambda off, nbytes, dt: arena.mem[base + off:base + off + nbytes].cpu().numpy().view(dt)
        spine = read(spine_off, RADIX * grid * 4, np.uint32).reshape(RADIX, grid)
        prefix = read(prefix_off, tiles * RADIX * 2, np.uint16).reshape(tiles, RADIX)
        head = read(plan_off, 64, np.uint32)
        exp_spine, exp_prefix = look_reference(keys, kt, desc)
        res[name] = {"n": n, "grid": grid, "grid_expected": int(exp_spine.shape[1]),
                     "spine_bad": int((spine != exp_spine).sum()), "prefix_bad": int((prefix != exp_prefix).sum()),
                     "head": [int(x) for x in head], "rule": plan_rule(keys, kt, desc), "guards": guards_ok(arena)}

    # ---- whole sorts
    def run(arena, n, kt, desc, ws_bytes):
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        rc = lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, desc, kt, None)
        assert rc == 0, rc
        st = (C.c_uint32 * 8)()
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, None) == 0
        torch.cuda.synchronize()
        return sel.value, list(st)

    expected = {}    # id of a key array -> (sorted bytes, plan rule): computed once per input, shared by the cases that use it

    def record(tag, keys, kt, desc, got, sel, st, guards):
        if tag not in expected:
            expected[tag] = (unmap(np.sort(ordmap(keys, kt, desc)), kt, desc), plan_rule(keys, kt, desc))
        exp, rule = expected[tag]
        return {"ok_numpy": bool(np.array_equal(got, exp)), "sha": hashlib.sha256(got.tobytes()).hexdigest(), "sel": sel,
                "status": st, "rule": rule, "guards": guards, "n": int(keys.size)}

    rng = np.random.default_rng(20262)
    uni = lambda n: rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    walk_p, walk_c = uni(N_WALK), planted(rng, N_WALK, 0x5A17, 17409)
    big_p, big_c = uni(N_THREE_UNITS), planted(rng, N_THREE_UNITS, 0xC3D2, 17409)
    singles = {"sort_uniform_257": ("u257", uni(N_257), U32, 0), "sort_uniform_walk": ("walk_p", walk_p, U32, 0),
               "sort_planted_walk": ("walk_c", walk_c, U32, 0), "sort_uniform_three_units": ("big_p", big_p, U32, 0),
               "sort_planted_three_units": ("big_c", big_c, U32, 0), "sort_i32_desc": ("i257", uni(N_257), I32, 1),
               "sort_f32_asc": ("f257", f32_specials(rng, N_257), F32, 0)}
    for name, (tag, keys, kt, desc) in singles.items():
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=1)
        arena.add("k0", 4 * n, data=keys).add("k1", 4 * n, fill="ff").add("ws", ws_bytes, fill="random").build()
        sel, st = run(arena, n, kt, desc, ws_bytes)
        res[name] = record(tag, keys, kt, desc, arena.read("k%d" % sel, np.uint32), sel, st, guards_ok(arena))
        del arena

    def reuse_and_graph(suffix, tag_p, keys_p, tag_c, keys_c):
        # one workspace, sort after sort: PLANNED, CLASSIC, PLANNED, CLASSIC -- a stale spine or stale flags must not be used.
        # (The reversed arrays sort to the same bytes with other counts per tile.)
        n = keys_p.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        seq = [(tag_p, keys_p), (tag_c, keys_c), (tag_p, keys_p[::-1].copy()), (tag_c, keys_c[::-1].copy())]
        arena = Arena(dev, seed=2)
        arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="ff").add("ws", ws_bytes, fill="ff").build()
        k0 = arena.slots["k0"][0]
        for i, (tag, keys) in enumerate(seq):
            arena.mem[k0:k0 + 4 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
            sel, st = run(arena, n, U32, 0, ws_bytes)
            res["reuse%s_%d" % (suffix, i)] = record(tag, keys, U32, 0, arena.read("k%d" % sel, np.uint32), sel, st, guards_ok(arena))
        del arena

        # stream capture: one captured sort, its buffers between guard bands, replayed on inputs whose routes go P, C, C, P
        arena = Arena(dev, seed=4)
        arena.add("src", 4 * n, fill="00").add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="ff").add("ws", ws_bytes, fill="random").build()
        view = lambda name, dt: arena.mem[arena.slots[name][0]:arena.slots[name][0] + arena.slots[name][1]].view(dt)
        src, a, b, temp = view("src", torch.int32), view("k0", torch.int32), view("k1", torch.int32), view("ws", torch.uint8)
        dk = gs.DoubleBuffer(a, b)
        assert gs.DeviceRadixSort.SortKeys(None, 0, dk, n) == ws_bytes
        side = torch.cuda.Stream()
        src.copy_(torch.from_numpy(keys_p.view(np.int32).copy()).to(dev))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            a.copy_(src)
            gs.DeviceRadixSort.SortKeys(temp, ws_bytes, dk, n, key_type=gs.GS_KEY_U32)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        dk.selector = 0
        with torch.cuda.graph(g, stream=side):
            a.copy_(src)
            gs.DeviceRadixSort.SortKeys(temp, ws_bytes, dk, n, key_type=gs.GS_KEY_U32)
        sel = dk.selector
        for i, (tag, keys) in enumerate([seq[0], seq[1], seq[3], seq[2]]):
            src.copy_(torch.from_numpy(keys.view(np.int32).copy()).to(dev))
            g.replay()
            torch.cuda.synchronize()
            st = (C.c_uint32 * 8)()
            assert lib.gs_lsb_plan_status(temp.data_ptr(), n, st, None) == 0
            res["graph%s_%d" % (suffix, i)] = record(tag, keys, U32, 0, arena.read("k%d" % sel, np.uint32), sel, list(st), guards_ok(arena))
        del g, arena

    reuse_and_graph("", "walk_p", walk_p, "walk_c", walk_c)
    reuse_and_graph("_three_units", "big_p", big_p, "big_c", big_c)

    with open(out_path, "w") as f:
        json.dump(res, f)
    print("fused child ok", len(res))


if __name__ == "__main__":
    main(sys.argv[1])
