"""gs_topk_u32 on the device: the first k of the stable sort, bit for bit against tests/topk_ref.py (keys, values or indices,
and the four status words), over sizes, k values, distributions, directions, forms and key types; the buffer contract with
guarded arenas; workspace reuse; graph capture; the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_ref as R
from guarded import Arena
from topk_cases import DISTS, gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
CAP = R.SMALL_CAP
ROUTES_SEEN = set()


# ------------------------------------------------------------------------------------------------------- inputs --
def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def values_for(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


class Case:
    """One input on the device with its reference; .check(k, mode) runs the C entry point and compares everything."""

    def __init__(self, gs, cuda, keys, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.n = gs, cuda, kt, desc, keys.size
        self.vals = values_for(keys.size)
        self.ref = {False: R.Ref(keys, kt, desc), True: R.Ref(keys, kt, desc, self.vals)}
        self.d_keys, self.d_vals = dev(keys, cuda), dev(self.vals, cuda)

    def check(self, k, mode, expect_route=None):
        gs, n = self.gs, self.n
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_temp_bytes(n, k, hv)
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((k,), -1, dtype=torch.int32, device=self.cuda)
        vo = torch.full((k,), -1, dtype=torch.int32, device=self.cuda) if hv else None
        rc = gs.lib.gs_topk_u32(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                ko.data_ptr(), vo.data_ptr() if hv else None, n, k, int(self.desc), self.kt, None)
        assert rc == 0, (rc, n, k, mode)
        st = (C.c_uint32 * 8)()
        assert gs.lib.gs_topk_status(temp.data_ptr(), n, k, hv, st, None) == 0
        what = "n=%d k=%d %s kt=%d desc=%d" % (n, k, mode, self.kt, self.desc)
        ek, ev, est = self.ref[mode == PAIRS].topk(k)
        assert list(st)[1:5] == est and list(st)[5:] == [0, 0, 0], (what, list(st), est)
        route = self.ref[False].route(k)
        assert st[0] == route, (what, st[0], route)
        if expect_route is not None:
            assert route == expect_route, (what, route)
        ROUTES_SEEN.add(int(st[0]))
        assert np.array_equal(host(ko), ek), what
        if hv:
            assert np.array_equal(host(vo), ev), what
        return int(st[0])


def k_values(n):
    return sorted({k for k in (1, 2, 64, 8192, 8193, n // 2, n - 1, n) if 1 <= k <= n})


# ------------------------------------------------------------------------------------------------ sizes and k --
SIZES = [1, 2, 63, 64, 65, 8191, 8192, 8193, 65535, 65536, 65537, CAP - 1, CAP, CAP + 1, 100003, (1 << 20) + 3]


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_k_values(gs, cuda, n):
    """Uniform keys (route 1 above one workgroup's capacity, route 3 below), every k of the list; form, key type and direction
    rotate with k so that every size sees them all."""
    i = SIZES.index(n)
    cases = {}
    for j, k in enumerate(k_values(n)):
        kt, desc, mode = (U32, I32, F32)[(i + j) % 3], bool((i + j // 3) % 2), MODES[(i + j // 2) % 3]
        if (kt, desc) not in cases:
            cases[(kt, desc)] = Case(gs, cuda, gen("uniform", n, seed=i), kt, desc)
        cases[(kt, desc)].check(k, mode, expect_route=3 if n <= CAP else 1)


# ------------------------------------------------------------------------------------------------ distributions --
@pytest.mark.parametrize("kind", DISTS)
def test_distributions_directions_forms_types(gs, cuda, kind):
    """Every distribution in both directions, the three forms and the three key types, at a size past the candidate list's
    smallest capacity (so that keys sharing a top byte take route 2) with a partial last tile."""
    n = 100003
    for kt in (U32, I32, F32):
        keys = gen(kind, n, seed=7, kt=kt)
        for desc in (False, True):
            c = Case(gs, cuda, keys, kt, desc)
            for j, k in enumerate((1, 777, 8193, n // 2, n - 1)):
                for mode in MODES if j in (1, 3) else (MODES[(j + kt) % 3],):
                    c.check(k, mode)


@pytest.mark.parametrize("kind,route", [("topbyte", 2), ("top3", 2), ("equal", 2), ("zipf", None), ("uniform", 1), ("five", 2)])
def test_distributions_at_the_largest_size(gs, cuda, kind, route):
    n = (1 << 20) + 3
    keys = gen(kind, n, seed=11)
    for kt, desc, mode in [(U32, False, PAIRS), (F32, True, ARGS), (I32, True, KEYS)]:
        c = Case(gs, cuda, keys, kt, desc)
        for k in (1, 8192, n // 2) if mode != KEYS else (64, n - 1):
            c.check(k, mode, expect_route=route)


def test_routes_one_two_and_three_are_all_taken(gs, cuda):
    assert Case(gs, cuda, gen("uniform", 300007), U32, False).check(1000, PAIRS) == 1
    assert Case(gs, cuda, gen("topbyte", 300007), U32, False).check(1000, PAIRS) == 2
    assert Case(gs, cuda, gen("uniform", 9000), U32, False).check(1000, PAIRS) == 3
    # a heavy hitter: one value holds half the array, the rest is uniform
    keys = gen("uniform", 300007, seed=5)
    keys[::2] = 0x80000000
    assert Case(gs, cuda, keys, U32, False).check(200000, ARGS) == 2
    assert Case(gs, cuda, keys, U32, False).check(1000, ARGS) == 1
    assert {1, 2, 3} <= ROUTES_SEEN


# ------------------------------------------------------------------------------------ cuts on tile boundaries --
def test_cut_on_every_tile_boundary_of_a_tie_run_in_the_input(gs, cuda):
    """All keys equal, read from the input itself (route 2): the cut after every whole tile of the run, and one to each side."""
    n = 100003
    for desc, mode in [(False, ARGS), (True, PAIRS)]:
        c = Case(gs, cuda, gen("equal", n), F32, desc)
        for t in range(1, n // 8192 + 1):
            for k in (8192 * t - 1, 8192 * t, 8192 * t + 1) if t in (1, 8, 12) else (8192 * t,):
                c.check(k, mode, expect_route=2)


def test_cut_on_every_tile_boundary_of_a_tie_run_in_the_candidate_list(gs, cuda):
    """20000 small keys, 50000 equal keys with another top byte and 30003 large ones, shuffled: the 50000 form the candidate
    list (route 1) and the cut falls after every whole tile of it, and of the input."""
    n = 100003
    keys = np.concatenate([np.arange(20000, dtype=np.uint32) % 977, np.full(50000, 0x20000000, np.uint32),
                           np.full(30003, 0xF0000000, np.uint32)])
    keys = keys[np.random.default_rng(2).permutation(n)]
    for desc, mode in [(False, ARGS), (True, KEYS), (False, PAIRS)]:
        c = Case(gs, cuda, keys, U32, desc)
        before = 30003 if desc else 20000
        ks = {before + 8192 * t for t in range(0, 7)} | {before + 8192 * 3 - 1, before + 8192 * 3 + 1, before + 1, before + 50000}
        ks |= {8192 * t for t in range(4, 9)}
        for k in sorted(ks):
            c.check(k, mode, expect_route=1)


# ------------------------------------------------------------------------------------------- buffer contract --
def _arena_run(gs, cuda, keys, k, kt, desc, mode, fill, seed, temp_offset=1, out_offset=4, spare=0, short_by=0):
    """One call with every buffer in a guarded arena.  Outputs hold k + spare elements; the spare ones must keep their fill."""
    n = keys.size
    hv = int(mode != KEYS)
    vals = values_for(n, seed + 1)
    nb = gs.lib.gs_topk_temp_bytes(n, k, hv)
    a = Arena(cuda, seed=seed, all_const=bool(short_by))
    a.add("keys_in", 4 * n, offset=12, data=keys, const=True)
    if mode == PAIRS:
        a.add("vals_in", 4 * n, offset=20, data=vals, const=True)
    a.add("keys_out", 4 * (k + spare), offset=out_offset, fill=fill)
    if hv:
        a.add("vals_out", 4 * (k + spare), offset=(out_offset + 8) % 256, fill=fill)
    a.add("temp", nb - short_by, offset=temp_offset, fill=fill)
    a.build()
    rc = gs.lib.gs_topk_u32(a.ptr("temp"), nb - short_by, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None,
                            a.ptr("keys_out"), a.ptr("vals_out") if hv else None, n, k, int(desc), kt, None)
    if short_by:
        assert rc == 1
        a.check()          # a refused call writes nothing: every buffer is byte-identical
        return
    assert rc == 0
    st = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_status(a.ptr("temp"), n, k, hv, st, None) == 0
    a.check()
    ref = R.Ref(keys, kt, desc, vals if mode == PAIRS else None)
    ek, ev, est = ref.topk(k)
    assert list(st)[1:5] == est
    ROUTES_SEEN.add(int(st[0]))
    got = a.read("keys_out", np.uint32)
    assert np.array_equal(got[:k], ek)
    assert np.array_equal(got[k:].view(np.uint8), a.init["keys_out"][4 * k:]), "written beyond k"
    if hv:
        got = a.read("vals_out", np.uint32)
        assert np.array_equal(got[:k], ev)
        assert np.array_equal(got[k:].view(np.uint8), a.init["vals_out"][4 * k:]), "written beyond k"
    return int(st[0])


@pytest.mark.parametrize("fill", ["00", "ff", "random"])
def test_guarded_offset_and_dirty_buffers(gs, cuda, fill):
    """Outputs at odd 4-byte offsets, d_temp + 1 with exactly the queried size, dirty outputs and workspace: guards and
    inputs unchanged, nothing written beyond k, results right -- on each route and in each form."""
    seed = ["00", "ff", "random"].index(fill)
    routes = set()
    for i, (kind, n, k, kt, desc, mode) in enumerate([
            ("uniform", 100003, 5000, U32, False, PAIRS), ("topbyte", 100003, 8193, F32, True, ARGS),
            ("zipf", 70001, 70001, I32, False, KEYS), ("uniform", CAP, 300, F32, True, PAIRS),
            ("five", CAP + 1, CAP, U32, True, ARGS), ("special", 40000, 1, I32, True, KEYS), ("uniform", 1, 1, U32, False, ARGS)]):
        routes.add(_arena_run(gs, cuda, gen(kind, n, seed=20 + i, kt=kt), k, kt, desc, mode, fill, seed * 10 + i,
                              temp_offset=(1, 255, 3)[i % 3], out_offset=(4, 12, 252)[i % 3], spare=(0, 5, 1000)[i % 3]))
    assert routes == {1, 2, 3}


def test_one_byte_less_of_workspace_is_refused_and_nothing_is_written(gs, cuda):
    for i, (n, k, mode) in enumerate([(100003, 5000, PAIRS), (100003, 5000, KEYS), (9000, 10, ARGS)]):
        _arena_run(gs, cuda, gen("uniform", n, seed=30 + i), k, U32, False, mode, "random", 40 + i, short_by=1)


# --------------------------------------------------------------------------------- reuse, repeat, capture --
def test_two_calls_share_a_workspace_and_a_repeat_gives_identical_bytes(gs, cuda):
    """Different inputs, k, forms and routes back to back on one stream and one workspace, no synchronisation between them."""
    a, b = gen("uniform", 300007, seed=41), gen("topbyte", 200003, seed=42)
    va = values_for(a.size)
    da, db, dva = dev(a, cuda), dev(b, cuda), dev(va, cuda)
    ka, kb = 40000, 7
    nb = max(gs.DeviceTopK.MinPairs(None, 0, None, None, None, None, a.size, ka), gs.DeviceTopK.MaxKeys(None, 0, None, None, b.size, kb))
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    outs = []
    for rep in range(2):
        oka, ova = (torch.full((ka,), -1, dtype=torch.int32, device=cuda) for _ in range(2))
        okb = torch.full((kb,), -1, dtype=torch.int32, device=cuda)
        oka2 = torch.full((ka,), -1, dtype=torch.int32, device=cuda)
        gs.DeviceTopK.MinPairs(temp, nb, da, oka, dva, ova, a.size, ka, key_type=gs.GS_KEY_U32)
        gs.DeviceTopK.MaxKeys(temp, nb, db, okb, b.size, kb, key_type=gs.GS_KEY_F32)
        gs.DeviceTopK.MinKeys(temp, nb, da, oka2, a.size, ka, key_type=gs.GS_KEY_U32)
        torch.cuda.synchronize()
        outs.append((host(oka).tobytes(), host(ova).tobytes(), host(okb).tobytes(), host(oka2).tobytes()))
    ek, ev, _ = R.topk(a, ka, U32, False, va)
    assert outs[0][0] == ek.tobytes() and outs[0][1] == ev.tobytes() and outs[0][3] == ek.tobytes()
    assert outs[0][2] == R.topk(b, kb, F32, True)[0].tobytes()
    assert outs[0] == outs[1]


def test_topk_convenience_form(gs, cuda):
    keys = gen("special", 250001, seed=50, kt=F32)
    t = torch.from_numpy(keys.view(np.float32).copy()).to(cuda)
    ko, vo = gs.topk(t, 1000, largest=True, indices=True)
    ek, ev, _ = R.topk(keys, 1000, F32, True)
    assert ko.dtype == torch.float32 and np.array_equal(ko.cpu().numpy().view(np.uint32), ek) and np.array_equal(host(vo), ev)
    vals = values_for(keys.size)
    ko, vo = gs.topk(dev(keys, cuda), 33, values=dev(vals, cuda))
    ek, ev, _ = R.topk(keys, 33, I32, False, vals)
    assert np.array_equal(host(ko), ek) and np.array_equal(host(vo), ev)
    ko, vo = gs.topk(dev(keys, cuda), 0)
    assert ko.numel() == 0 and vo is None


def test_topk_is_capturable_in_a_hip_graph(gs, cuda):
    """Captured once on a side stream, replayed on new data in the same buffers: uniform keys (route 1), keys sharing a top
    byte (route 2), uniform again -- the same launches whatever the data."""
    n, k = 150001, 5000
    sets = [gen(kind, n, seed=60 + i) for i, kind in enumerate(("uniform", "topbyte", "zipf"))]
    src = dev(sets[0], cuda)
    ko = torch.full((k,), -1, dtype=torch.int32, device=cuda)
    vo = torch.full((k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopK.MaxPairs(None, 0, None, None, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopK.MaxPairs(temp, nb, src, ko, None, vo, n, k, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopK.MaxPairs(temp, nb, src, ko, None, vo, n, k, key_type=gs.GS_KEY_U32)
    routes = []
    for keys in sets:
        src.copy_(dev(keys, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev, est = R.topk(keys, k, U32, True)
        assert np.array_equal(host(ko), ek) and np.array_equal(host(vo), ev)
        st = gs.DeviceTopK.Status(temp, n, k, True)
        assert st[1:5] == est
        routes.append(st[0])
    assert routes[:2] == [1, 2]


# ------------------------------------------------------------------------------------------------- property --
@pytest.mark.parametrize("desc", [False, True])
def test_property_at_4m_against_numpys_stable_argsort(gs, cuda, desc):
    n, k = 1 << 22, 1 << 16
    keys = gen("uniform", n, seed=70)
    vals = np.arange(n, dtype=np.uint32)                      # enumerated values
    order = np.argsort(~keys if desc else keys, kind="stable")[:k]
    nb = gs.lib.gs_topk_temp_bytes(n, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = torch.empty(k, dtype=torch.int32, device=cuda), torch.empty(k, dtype=torch.int32, device=cuda)
    fn = gs.DeviceTopK.MaxPairs if desc else gs.DeviceTopK.MinPairs
    fn(temp, nb, dev(keys, cuda), ko, dev(vals, cuda), vo, n, k, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    assert np.array_equal(host(vo), order.astype(np.uint32)) and np.array_equal(host(ko), keys[order])
    assert gs.DeviceTopK.Status(temp, n, k, True)[0] == 1


# -------------------------------------------------------------------------------------------------- driver --
def test_topk_check_driver():
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_check")
    assert os.path.exists(exe), "run build() first"
    r = subprocess.run([exe, "200003"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "OK" and "FAIL" not in r.stdout
