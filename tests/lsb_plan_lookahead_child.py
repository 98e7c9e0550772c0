"""Child process of tests/test_lsb_plan_lookahead_gpu.py: the look of the keys-only plan at the edges of its walk over units,
and the one-pass local sort on a grid smaller than its task list (gs_lsb_plan.hip, gs_msb.hip), in THIS process's mode
(GS_LSB_KEYS_PLAN, GS_LSB_PLAN_MIN_ITEMS and GS_LSB_PLAN_ONEPASS_GRID are read once per process):

    python tests/lsb_plan_lookahead_child.py look|finish OUT.json

look    per case: gs_lsb_plan_look_only alone on a workspace of random bytes -- spine and prefix16 against look_reference of
        tests/lsb_plan_fused_child.py, the head of the plan block -- and then a whole sort between guard bands: sha of the
        result, selector, gs_lsb_plan_status, the plan rule.  With GS_LSB_KEYS_PLAN=classic only the sorts run.
finish  lists of class-3 groups that number grid - 1, grid, grid + 1 and 2 grid + 1 (grid = gs_lsb_plan_onepass_grid()), built
        and checked on the device; in some groups one value repeats so often that the one-pass sort must leave them."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from lsb_plan_child import F32, I32, U32, f32_specials, plan_rule  # noqa: E402
from lsb_plan_fused_child import look_reference  # noqa: E402

TILE, UNIT, GRID = 8192, 131072, 256            # a look workgroup takes a unit of 16 tiles at a time; 256 workgroups at the most
ROUND = GRID * UNIT                             # 2^25 keys: one unit for every workgroup
N_MIN = 65536
N_FEW_UNITS = 5 * UNIT + 3 * TILE + 63          # six workgroups, one unit each; the last one's waves 4 ... 15 have no tile
N_ONE_EACH = ROUND
N_ONE_MORE = ROUND + UNIT                       # one workgroup has two units
N_MIXED = ROUND + 5 * UNIT + 777                # six have two; the last unit holds one tile of 777 keys: its other waves find nothing
N_SOME_WAVES = ROUND + 5 * TILE + 4099          # the second unit of one workgroup: five full tiles, a ragged one, ten waves without a tile
N_ONE_CHUNK = ROUND + 8 * TILE                  # a last unit of one chunk
N_THREE_EACH = 3 * ROUND
TAILS = (1, 63, 64, 8191)                       # a last unit of one chunk whose last tile is ragged: ROUND + 7 tiles + r
SIZES = (N_MIN, N_FEW_UNITS, N_ONE_EACH, N_ONE_MORE, N_MIXED, N_SOME_WAVES, N_ONE_CHUNK, N_THREE_EACH) + tuple(ROUND + 7 * TILE + r for r in TAILS)
TYPE_SIZES = (N_ONE_MORE, N_MIXED, ROUND + 7 * TILE + 63)
KEY_SIZES = (N_MIXED, N_SOME_WAVES)
INVALID_VALUE = 1


def look_cases():
    """name -> (make keys, key type, descending)"""
    c = {}
    uni = lambda n: (lambda rng: rng.integers(0, 1 << 32, size=n, dtype=np.uint32))
    for n in SIZES:
        c["uniform_%d" % n] = (uni(n), U32, 0)
    for n in KEY_SIZES:
        c["constant_%d" % n] = (lambda rng, n=n: np.full(n, 0x9E3779B9, np.uint32), U32, 0)                # the whole-wave path

        def half_ones(rng, n=n):                                                                          # the skew path
            k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
            k[rng.random(n) < 0.5] = np.uint32(0xFFFFFFFF)
            return k
        c["half_ones_%d" % n] = (half_ones, U32, 0)

        # up to 70000 keys of one group inside one workgroup's SECOND unit: at N_MIXED its 16-bit counter wraps; at N_SOME_WAVES
        # the unit ends after 44959 of them: CLASSIC without a wrap
        def wrapped(rng, n=n):
            k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
            at = ROUND + 100
            k[at:at + 70000] = (k[at:at + 70000] & np.uint32(0xFFFF)) | np.uint32(0x5A17 << 16)
            return k
        c["wrapped_%d" % n] = (wrapped, U32, 0)
    for n in TYPE_SIZES:
        for kt, tag in ((U32, "u32"), (I32, "i32"), (F32, "f32")):
            for desc in (0, 1):
                if kt == U32 and not desc:
                    continue
                # (f32 descending: half of the keys are a dozen special values -- CLASSIC; every other case is PLANNED)
                make = (lambda rng, n=n: f32_specials(rng, n)) if kt == F32 and desc else uni(n)
                c["%s_%s_%d" % (tag, "desc" if desc else "asc", n)] = (make, kt, desc)
    return c


def guards_ok(arena):
    try:
        arena.check()
        return True
    except AssertionError as e:
        print("guard:", e)
        return False


def main_look(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib
    plan_on = os.environ.get("GS_LSB_KEYS_PLAN") != "classic"
    res = {}
    for i, (name, (make, kt, desc)) in enumerate(look_cases().items()):
        keys = make(np.random.default_rng(30000 + i))
        n = keys.size
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        r = {"n": n}
        if plan_on:
            arena = Arena(dev, seed=3)
            arena.add("k0", 4 * n, data=keys, const=True).add("k1", 4 * n, fill="ff").add("ws", ws_bytes, fill="random").build()
            lay = (C.c_uint64 * 4)()
            assert lib.gs_lsb_plan_layout(n, lay) == 0
            assert lib.gs_lsb_plan_look_only(arena.ptr("ws"), arena.ptr("k0"), arena.ptr("k1"), n, kt, desc, None) == 0
            torch.cuda.synchronize()
            spine_off, prefix_off, plan_off, grid = (int(x) for x in lay)
            base = ((arena.ptr("ws") + 255) & ~255) - arena.mem.data_ptr()
            tiles = (n + TILE - 1) // TILE
            read = lambda off, nbytes, dt: arena.mem[base + off:base + off + nbytes].cpu().numpy().view(dt)
            spine = read(spine_off, 256 * grid * 4, np.uint32).reshape(256, grid)
            prefix = read(prefix_off, tiles * 256 * 2, np.uint16).reshape(tiles, 256)
            exp_spine, exp_prefix = look_reference(keys, kt, desc)
            r.update({"grid": grid, "grid_expected": int(exp_spine.shape[1]), "spine_bad": int((spine != exp_spine).sum()),
                      "prefix_bad": int((prefix != exp_prefix).sum()), "head": [int(x) for x in read(plan_off, 64, np.uint32)],
                      "rule": plan_rule(keys, kt, desc), "look_guards": guards_ok(arena)})
            del arena, spine, prefix, exp_spine, exp_prefix
        arena = Arena(dev, seed=1)
        arena.add("k0", 4 * n, data=keys).add("k1", 4 * n, fill="ff").add("ws", ws_bytes, fill="random").build()
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        assert lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, desc, kt, None) == 0
        st = (C.c_uint32 * 8)()
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, None) == 0
        torch.cuda.synchronize()
        start = arena.slots["k%d" % sel.value][0]
        out = arena.mem[start:start + 4 * n].view(torch.int32)
        inv = gs.check_sorted(out, descending=False)[0] if (kt == U32 and not desc) else None
        r.update({"sha": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), "sel": sel.value, "status": list(st),
                  "inversions": inv, "guards": guards_ok(arena)})
        res[name] = r
        del arena, out, keys
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("lookahead child ok", len(res))


# ---- the finish: class-3 groups on the device (as tests/lsb_plan_trim_child.py builds its capped case)
HEAVY = {"every2_300": (2, 300), "last_300": (0, 300), "every2_20": (2, 20), "last_20": (0, 20), "every2_third": (2, -3)}


def finish_keys(torch, dev, sizes, seed, kind):
    """Groups of the given sizes under distinct random prefixes, shuffled; uniform low 16 bits.  kind (HEAVY): in every second
    class-3 group, or in the last one alone, the first `count` keys share one value (count -3: a third of the group)."""
    rng = np.random.default_rng(seed)
    groups = len(sizes)
    prefixes = np.sort(rng.choice(65536, groups, replace=False))
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    sz = torch.from_numpy(np.asarray(sizes, np.int64)).to(dev)
    gid = torch.repeat_interleave(torch.arange(groups, device=dev), sz)
    n = int(gid.numel())
    low = torch.randint(0, 1 << 16, (n,), device=dev, generator=g)
    every, count = HEAVY[kind]
    big = np.flatnonzero(np.asarray(sizes) > 9216)                      # the class-3 groups, in list order
    chosen = big[::2] if every == 2 else big[-1:]
    mark = torch.zeros(groups, dtype=torch.bool, device=dev)
    mark[torch.from_numpy(chosen).to(dev)] = True
    idx = torch.arange(n, device=dev) - (torch.cumsum(sz, 0) - sz)[gid]    # position inside the group
    limit = sz[gid] // 3 if count < 0 else torch.full_like(idx, count)
    low = torch.where(mark[gid] & (idx < limit), torch.full_like(low, 0x1234), low)
    keys = ((torch.from_numpy(prefixes.astype(np.int64)).to(dev)[gid] << 16) | low)[torch.randperm(n, device=dev, generator=g)]
    return torch.where(keys >= (1 << 31), keys - (1 << 32), keys).to(torch.int32), int(chosen.size)


def finish_cases(grid):
    rng = np.random.default_rng(4711)
    c = {}
    for groups in (grid - 1, grid, grid + 1, 2 * grid + 1):
        sizes = rng.integers(9217, 17409, size=groups)
        sizes[0], sizes[-1] = 9217, 17408
        for kind in HEAVY:
            c["%s_%d" % (kind, groups)] = (sizes, kind)
    # all four classes at once, more class-3 groups than workgroups
    sizes = np.concatenate([rng.integers(1, 2049, 300), rng.integers(2049, 4609, 300), rng.integers(4609, 9217, 300),
                            rng.integers(9217, 17409, grid + 3)])
    rng.shuffle(sizes)
    c["four_classes"] = (sizes, "every2_300")
    return c


def main_finish(out_path):
    import torch
    import gpu_sort_amd as gs
    from guarded import Arena

    dev = torch.device("cuda:0")
    lib = gs.lib
    grid = int(lib.gs_lsb_plan_onepass_grid())
    res = {"grid": grid}
    for i, (name, (sizes, kind)) in enumerate(finish_cases(grid).items()):
        keys, heavy = finish_keys(torch, dev, sizes, 900 + i, kind)
        n = int(keys.numel())
        _, want_sum, want_xor = gs.check_sorted(keys)
        ws_bytes = lib.gs_lsb_temp_bytes(n, 0)
        arena = Arena(dev, seed=10)
        arena.add("k0", 4 * n, fill="00").add("k1", 4 * n, fill="random").add("ws", ws_bytes, fill="random").build()
        k0 = arena.slots["k0"][0]
        arena.mem[k0:k0 + 4 * n] = keys.view(torch.uint8)
        del keys
        kp = (C.c_void_p * 2)(arena.ptr("k0"), arena.ptr("k1"))
        sel = C.c_int(0)
        assert lib.gs_lsb_sort_u32(arena.ptr("ws"), ws_bytes, kp, None, C.byref(sel), n, 0, 32, 0, U32, None) == 0
        pk, st = (C.c_uint32 * 4)(), (C.c_uint32 * 8)()
        assert lib.gs_lsb_plan_peek_status(pk) == 0
        assert lib.gs_lsb_plan_status(arena.ptr("ws"), n, st, None) == 0
        torch.cuda.synchronize()
        start = arena.slots["k%d" % sel.value][0]
        out = arena.mem[start:start + 4 * n].view(torch.int32)
        inv, got_sum, got_xor = gs.check_sorted(out)
        classes = [int((np.searchsorted([2048, 4608, 9216, 17408], sizes, side="left") == c).sum()) for c in range(4)]
        res[name] = {"sha": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), "sel": sel.value, "status": list(st), "peek": list(pk),
                     "guards": guards_ok(arena), "n": n, "classes": classes, "heavy": heavy, "inversions": inv,
                     "multiset": bool(got_sum == want_sum and got_xor == want_xor)}
        del arena, out
    with open(out_path, "w") as f:
        json.dump(res, f)
    print("lookahead child ok", len(res))


if __name__ == "__main__":
    {"look": main_look, "finish": main_finish}[sys.argv[1]](sys.argv[2])
