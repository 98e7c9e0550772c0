"""Child process of tests/test_lsb_plan_trim_gpu.py: the small launches of the keys-only plan (gs_lsb_plan.hip) -- the
follow-up kernel of the cursor scatter, the cursor set-up and the scatter that know their route, the decide kernel's
mailbox and the capped leftover launches of the finish -- in THIS process's mode (GS_LSB_PLAN_PEEK, GS_LSB_KEYS_PLAN and
GS_LSB_PLAN_MIN_ITEMS are read once per process).  Writes one JSON record per sort:

    python tests/lsb_plan_trim_child.py OUT.json

A record of a small case holds what tests/lsb_plan_cursor_child.py records (ok_numpy, sha, sel, status, cursor, rule,
irregular, guards, n) plus peek (gs_lsb_plan_peek_status).  A record of a capped case (about 13 300 keys per group times
1.5 gs_lsb_plan_finish_cap() groups, built and checked on the device) holds sha, sel, status, cursor, peek, guards, n,
groups, inversions and multiset (the result's adjacent inversions, and whether its multiset sum and xor are the
input's)."""
import ctypes as C
import hashlib
import json
import sys

import numpy as np

from lsb_plan_child import U32, ordmap, plan_rule
from lsb_plan_cursor_child import TILE, irregular_tiles
from lsb_plan_peek_child import route_inputs

ROUND = 512                        # keys of a tile that the follow-up kernel's workgroup takes at a time
TAILS = (1, 63, 64, 65, 4097, 8191)


def layout(rng, segments):
    """segments: (d1, d2, count) in non-decreasing d1 -> keys in that order, i.e. as the first scatter (stable, on d1 = bits
    16-23) leaves them when it gets them in this order.  d2 (bits 24-31): a number, None for random, or "lane" for
    position % 256 (64 neighbours never share a group).  Random low 16 bits."""
    parts, at = [], 0
    for d1, d2, count in segments:
        if d2 is None:
            hi = rng.integers(0, 256, size=count, dtype=np.uint32)
        elif isinstance(d2, str):
            hi = ((at + np.arange(count, dtype=np.uint32)) % np.uint32(256)).astype(np.uint32)
        else:
            hi = np.full(count, d2, np.uint32)
        parts.append((hi << np.uint32(24)) | (np.uint32(d1) << np.uint32(16)) | rng.integers(0, 1 << 16, size=count, dtype=np.uint32))
        at += count
    k = np.concatenate(parts).astype(np.uint32)
    assert np.all(np.diff(((k >> np.uint32(16)) & np.uint32(0xff)).astype(np.int64)) >= 0)
    return k


def make_cases():
    """name -> keys (u32, ascending: the key is its own order-preserving image)"""
    rng = np.random.default_rng(20263)
    c = {}
    # tile 3: 8191 keys of one group, then one key of the next d1 -- one hot cursor in every wave round -- and the mirror image
    c["straddle_hot_then_one"] = layout(rng, [(5, None, 3 * TILE), (5, 7, TILE - 1), (6, 7, 1), (6, None, 5 * TILE)])
    c["straddle_one_then_hot"] = layout(rng, [(5, None, 3 * TILE), (5, 7, 1), (6, 7, TILE - 1), (6, None, 5 * TILE)])
    # tile 2: d1 boundaries at positions 63, 64 and 65 of a round (either side of the first wave's edge), then four groups
    # inside the second wave of a round (65, 67, 70): three and more groups in one wave round
    cuts = [5 * ROUND + 63, 5 * ROUND + 65, 9 * ROUND + 64, 9 * ROUND + 65, 12 * ROUND + 65, 12 * ROUND + 67, 12 * ROUND + 70]
    seg, at = [(10, None, 2 * TILE), (10, 3, cuts[0])], 2 * TILE + cuts[0]
    for i, cut in enumerate(cuts):
        end = 2 * TILE + (cuts[i + 1] if i + 1 < len(cuts) else TILE)
        seg.append((11 + i, 3, end - at))
        at = end
    seg.append((11 + len(cuts), None, 6 * TILE))
    c["three_groups_in_a_wave"] = layout(rng, seg)
    # tile 4 straddles, and every lane of every wave round meets another group
    c["every_lane_its_group"] = layout(rng, [(20, None, 4 * TILE), (20, "lane", TILE // 2), (21, "lane", TILE // 2), (21, None, 4 * TILE)])
    for r in TAILS:
        c["tail_%d" % r] = rng.integers(0, 1 << 32, size=8 * TILE + r, dtype=np.uint32)
    # the partial tile is the only tile of its d1
    c["tail_alone_in_its_d1"] = layout(rng, [(d1, None, TILE) for d1 in range(8)] + [(200, None, 100)])
    return c


IRREGULAR = {"straddle_hot_then_one": 1, "straddle_one_then_hot": 1, "three_groups_in_a_wave": 1, "every_lane_its_group": 1,
             "tail_alone_in_its_d1": 1}


def capped_keys(torch, dev, groups, seed, kind):
    """`groups` groups of 9217 ... 17408 keys (local-sort class 3), shuffled.  kind "few": the low 16 bits of every group come
    from 40 values; "heavy": 30 % of every group is one value, the rest are distinct."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(9217, 17409, size=groups)
    sizes[0], sizes[-1] = 9217, 17408
    prefixes = np.sort(rng.choice(65536, groups, replace=False))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sz = torch.from_numpy(sizes).to(dev)
    gid = torch.repeat_interleave(torch.arange(groups, device=dev), sz)
    n = int(gid.numel())
    top = torch.from_numpy(prefixes.astype(np.int64)).to(dev)[gid] << 16
    if kind == "few":
        values = torch.from_numpy(rng.choice(65536, 40, replace=False).astype(np.int64)).to(dev)
        low = values[torch.randint(0, 40, (n,), device=dev, generator=g)]
    else:
        start = torch.cumsum(sz, 0) - sz
        idx = torch.arange(n, device=dev) - start[gid]              # position inside the group
        low = torch.where(idx * 10 < sz[gid] * 3, torch.full_like(idx, 0x1234), (idx * 3 + 7) & 0xffff)   # (idx < 17408: idx * 3 + 7 is distinct)
    keys = (top | low)[torch.randperm(n, device=dev, generator=g)]
    return torch.where(keys >= (1 << 31), keys - (1 << 32), keys).to(torch.int32)    # the same 32 bits


def main(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib

    def run(arena, n, ws_bytes):
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        rc = lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, 0, U32, None)
        assert rc == 0, rc
        pk, st, cu = (C.c_uint32 * 4)(), (C.c_uint32 * 8)(), (C.c_uint32 * 4)()
        assert lib.gs_lsb_plan_peek_status(pk) == 0
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, None) == 0
        assert lib.gs_lsb_plan_cursor_status(arena.ptr("ws"), n, cu, None) == 0
        torch.cuda.synchronize()
        return sel.value, list(st), list(cu), list(pk)

    def record(keys, got, sel, st, cu, pk, guards):
        exp = keys[np.argsort(ordmap(keys, U32, 0), kind="stable")]
        return {"ok_numpy": bool(np.array_equal(got, exp)), "sha": hashlib.sha256(got.tobytes()).hexdigest(), "sel": sel,
                "status": st, "cursor": cu, "peek": pk, "rule": plan_rule(keys, U32, 0), "irregular": irregular_tiles(keys, U32, 0),
                "guards": guards, "n": int(keys.size)}

    def guards_ok(arena):
        try:
            arena.check()
            return True
        except AssertionError as e:
            print("guard:", e)
            return False

    res = {}
    for name, keys in make_cases().items():
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=9)
        arena.add("k0", 4 * n, data=keys).add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="random").build()
        sel, st, cu, pk = run(arena, n, ws_bytes)
        res[name] = record(keys, arena.read("k%d" % sel, np.uint32), sel, st, cu, pk, guards_ok(arena))
        if name in IRREGULAR:
            assert res[name]["irregular"] == IRREGULAR[name], (name, res[name]["irregular"])

    # more class-3 groups than the finish's leftover launches have workgroups: they stride
    cap = int(lib.gs_lsb_plan_finish_cap())
    groups = cap + cap // 2
    for kind in ("few", "heavy"):
        keys = capped_keys(torch, dev, groups, 77, kind)
        n = int(keys.numel())
        _, want_sum, want_xor = gs.check_sorted(keys)
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=10)
        arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="random").build()
        k0 = arena.slots["k0"][0]
        arena.mem[k0:k0 + 4 * n] = keys.view(torch.uint8)
        del keys
        sel, st, cu, pk = run(arena, n, ws_bytes)
        start = arena.slots["k%d" % sel][0]
        out = arena.mem[start:start + 4 * n].view(torch.int32)
        inv, got_sum, got_xor = gs.check_sorted(out)
        res["capped_" + kind] = {"sha": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), "sel": sel, "status": st, "cursor": cu,
                                 "peek": pk, "guards": guards_ok(arena), "n": n, "groups": groups, "inversions": inv,
                                 "multiset": bool(got_sum == want_sum and got_xor == want_xor)}
        del arena, out

    # one workspace, sort after sort: PLANNED, CLASSIC, CLASSIC, PLANNED
    n = 17 * TILE + 4099
    p0, c0 = route_inputs(41, n)
    p1, c1 = route_inputs(42, n)
    ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
    arena = Arena(dev, seed=11)
    arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="ff").build()
    k0 = arena.slots["k0"][0]
    for i, keys in enumerate([p0, c0, c1, p1]):
        arena.mem[k0:k0 + 4 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(dev)
        sel, st, cu, pk = run(arena, n, ws_bytes)
        res["reuse_%d" % i] = record(keys, arena.read("k%d" % sel, np.uint32), sel, st, cu, pk, guards_ok(arena))

    # one captured sort (no mailbox: the fixed sequence), replayed on a PLANNED and on a CLASSIC input
    src = torch.empty(n, dtype=torch.int32, device=dev)
    a, b = torch.empty_like(src), torch.empty_like(src)
    dk = gs.DoubleBuffer(a, b)
    nb = gs.DeviceRadixSort.SortKeys(None, 0, dk, n)
    temp = torch.empty(nb, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    src.copy_(torch.from_numpy(p0.view(np.int32).copy()).to(dev))
    with torch.cuda.stream(side):
        a.copy_(src)
        gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    dk.selector = 0
    with torch.cuda.graph(g, stream=side):
        a.copy_(src)
        gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
        pk = (C.c_uint32 * 4)()
        assert lib.gs_lsb_plan_peek_status(pk) == 0
    sel = dk.selector
    out = dk.Current()
    for i, keys in enumerate([p1, c1]):
        src.copy_(torch.from_numpy(keys.view(np.int32).copy()).to(dev))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        st, cu = (C.c_uint32 * 8)(), (C.c_uint32 * 4)()
        assert lib.gs_lsb_plan_status(temp.data_ptr(), n, st, None) == 0
        assert lib.gs_lsb_plan_cursor_status(temp.data_ptr(), n, cu, None) == 0
        res["graph_%d" % i] = record(keys, out.cpu().numpy().view(np.uint32), sel, list(st), list(cu), list(pk), True)

    with open(out_path, "w") as f:
        json.dump(res, f)
    print("trim child ok", len(res))


if __name__ == "__main__":
    main(sys.argv[1])
