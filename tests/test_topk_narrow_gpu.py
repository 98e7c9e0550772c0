"""gs_topk_u16 on the device, bit for bit against tests/topk_narrow_ref.py (keys, values or indices, and the eight status words):
route 3 up to one tile, the first general shapes, the candidate list exactly full and one too many at its smallest capacity and
where n / 32 sets it, k-th images whose bytes are 0x00 and 0xff, cuts on the edges of top-byte buckets and tie runs, all keys
equal, the float orders, k = 1 and k = n, 2-byte alignment of the key arrays, guarded, offset and dirty buffers, refused calls,
workspace reuse, identical bytes, graph capture, the widen identity against gs_topk_u32, the Python front ends and the C++
driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_narrow_ref as N
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = N.U16, N.I16, N.F16, N.BF16
KEYS, PAIRS, ARGS, MODES = N.KEYS, N.PAIRS, N.ARGS, N.MODES
TILE = N.TILE
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, k) is written
ROUTES_SEEN = set()


def dev16(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(cuda)


def dev32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def status(gs, temp_ptr, n, k, hv):
    st = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_u16_status(temp_ptr, n, k, hv, st, None) == 0
    return [int(x) for x in st]


class Case:
    """One input on the device with its reference (one stable argsort); .check(k, mode) runs the C entry point on a workspace
    filled with 0xA5 and outputs filled with -1 and compares keys, values or indices, the sentinels behind the outputs and the
    eight status words.  in_off / out_off: the key input / output starts that many elements into its allocation."""

    def __init__(self, gs, cuda, keys, kt, desc, what="", in_off=0):
        self.gs, self.cuda, self.kt, self.desc, self.n, self.what, self.in_off = gs, cuda, kt, desc, keys.size, what, in_off
        self.vals = np.random.default_rng(3).integers(0, 1 << 32, keys.size, dtype=np.uint64).astype(np.uint32)
        self.ref = N.Ref16(keys, kt, desc)
        self.d_keys = dev16(np.concatenate([np.full(in_off, 0x5A5A, np.uint16), keys]), cuda)
        self.d_vals = dev32(self.vals, cuda)

    def check(self, k, mode, expect_route=None, expect_top=None, out_off=0):
        gs, n = self.gs, self.n
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_u16_temp_bytes(n, k, hv)
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((out_off + k + TAIL,), -1, dtype=torch.int16, device=self.cuda)
        vo = torch.full((k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_u16(temp.data_ptr(), nb, self.d_keys.data_ptr() + 2 * self.in_off,
                                self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr() + 2 * out_off,
                                vo.data_ptr() if hv else None, n, k, int(self.desc), self.kt, None)
        what = "%s n=%d k=%d %s kt=%d desc=%d off=%d/%d" % (self.what, n, k, mode, self.kt, self.desc, self.in_off, out_off)
        assert rc == 0, (rc, what)
        st = status(gs, temp.data_ptr(), n, k, hv)
        ek, idx, est = self.ref.topk(k)
        route = self.ref.route(k)
        if expect_route is not None:
            assert route == expect_route, (what, route)
        if expect_top is not None:
            assert est[3] == expect_top, (what, est)
        assert st == [route] + est + [0, 0, 0], (what, st, [route] + est)
        ROUTES_SEEN.add(st[0])
        gk, gv = host16(ko), host32(vo)
        assert (gk[:out_off] == 0xFFFF).all() and (gk[out_off + k:] == 0xFFFF).all() and gk[out_off + k:].size == TAIL, what
        assert np.array_equal(gk[out_off:out_off + k], ek), what
        if hv:
            assert np.array_equal(gv[:k], self.vals[idx] if mode == PAIRS else idx), what
            assert (gv[k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        return st[0]


def rotate(i):
    return N.KEY_TYPES[i % 4], bool((i // 4) % 2), MODES[(i // 2) % 3]


# ------------------------------------------------------------------------------------------------------ route 3 --
@pytest.mark.parametrize("n", [1, 2, 8191, 8192])
def test_route3_up_to_one_tile(gs, cuda, n):
    for i, kind in enumerate(("uniform", "five", "special", "topbyte")):
        kt, desc, _ = rotate(i + n)
        case = Case(gs, cuda, N.gen16(kind, n, seed=i + 1, kt=kt), kt, desc, kind)
        for k in sorted({1, (n + 1) // 2, n}):
            for mode in MODES:
                case.check(k, mode, expect_route=3)


# ----------------------------------------------------------------------------------------- first general shapes --
@pytest.mark.parametrize("n", [8193, 3 * 8192 + 5])
def test_first_general_shapes(gs, cuda, n):
    """Two tiles, the last of one element; four tiles with a ragged last one.  Every distribution, key type and form."""
    for i, kind in enumerate(N.DISTS):
        kt, desc, _ = rotate(i)
        case = Case(gs, cuda, N.gen16(kind, n, seed=10 + i, kt=kt), kt, desc, kind)
        for j, k in enumerate(sorted({1, 2, n // 3, 8192, 8193, n - 1, n})):
            for mode in MODES if j % 3 == 0 else (MODES[(i + j) % 3],):
                assert case.check(k, mode) in (1, 2)


# ---------------------------------------------------------------------------------------------- capacity boundary --
CAPACITY = [(70001, 65536), ((1 << 21) + 3 * 8192 + 1, ((1 << 21) + 3 * 8192 + 1) // 32)]


@pytest.mark.parametrize("n,cap", CAPACITY)
@pytest.mark.parametrize("dc", [0, 1])
def test_candidate_list_exactly_full_and_one_too_many(gs, cuda, n, cap, dc):
    """A top-byte bucket of cap and cap + 1 elements behind 2000 smaller ones: the list takes cap of them (route 1, the last at
    cand[cap - 1]) and not one more (route 2), at the smallest capacity and where n / 32 sets it."""
    assert N.cap(n) == cap
    c, below = cap + dc, 2000
    for i, (kt, desc) in enumerate(((U16, False), (BF16, True)) if n < 100000 else ((I16, bool(dc)),)):
        case = Case(gs, cuda, N.bucket_case16(n, c, below, 0x42, n + dc, kt, desc), kt, desc, "bucket c=%d" % c)
        for j, (k, inside) in enumerate(N.bucket_ks(below, c)):
            for mode in MODES if j == 3 else (MODES[(j + i + dc) % 3],):
                case.check(k, mode, expect_route=2 if inside and dc == 1 else 1, expect_top=c if inside else None)


# -------------------------------------------------------------------------------------------------- digit edges --
@pytest.mark.parametrize("route,top", [(1, 0x00), (2, 0x00), (2, 0xFF)])
@pytest.mark.parametrize("kt", N.KEY_TYPES)
def test_extreme_digits_and_the_three_cuts_around_every_tie_run(gs, cuda, route, top, kt):
    """Runs of twelve images whose bytes are 0x00, 0x01, 0x7f, 0x80, 0xfe and 0xff: both picks meet digit 0 and digit 255, on
    the candidate list and (route 2) on the input; k is the last of each run, the first of the next, and one before, which are
    also the first and last elements of the top-byte buckets."""
    for desc in (False, True):
        case = Case(gs, cuda, N.digit_edge_case16(route, top, kt, desc), kt, desc, "digits route=%d top=%#x" % (route, top))
        ks = sorted(set(N.run_cuts(case.ref)) | set(N.bucket_cuts(case.ref)))
        routes = {case.check(k, MODES[j % 3]) for j, k in enumerate(ks)}
        assert routes == ({1, 2} if route == 2 else {1})


def test_cuts_on_the_first_and_last_element_of_top_byte_buckets(gs, cuda):
    case = Case(gs, cuda, N.gen16("uniform", 50021, seed=5, kt=F16), F16, True, "uniform")
    cuts = N.bucket_cuts(case.ref)
    for j, k in enumerate(cuts[:6] + cuts[250:256] + cuts[-6:]):
        case.check(k, MODES[j % 3], expect_route=1)


# ------------------------------------------------------------------------------------------------------- ties --
def test_all_keys_equal(gs, cuda):
    n = 20000
    for kt, desc, pattern in ((U16, False, 0x3F80), (BF16, True, 0x3F80), (I16, True, 0x8000), (F16, False, 0xFFFF)):
        case = Case(gs, cuda, np.full(n, pattern, np.uint16), kt, desc, "equal")
        for k in (1, 7777, n):
            for mode in MODES:
                case.check(k, mode, expect_route=1, expect_top=n)
            assert np.array_equal(case.ref.topk(k)[1], np.arange(k, dtype=np.uint32))      # the arguments form: 0 .. k - 1


def test_eight_values(gs, cuda):
    n = 70001
    rng = np.random.default_rng(8)
    for i, kt in enumerate(N.KEY_TYPES):
        keys = (rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16) & np.uint16(0x8003))
        case = Case(gs, cuda, keys, kt, bool(i % 2), "eight values")
        assert np.unique(keys).size == 8
        for j, k in enumerate(N.run_cuts(case.ref)):
            case.check(k, MODES[(i + j) % 3])


# ------------------------------------------------------------------------------------------------- float orders --
@pytest.mark.parametrize("kt", [F16, BF16, I16])
def test_special_patterns_in_both_directions(gs, cuda, kt):
    """NaNs of both signs, +-0, +-inf and denormals (the extremes for I16), six in ten elements: negative NaNs first and
    positive NaNs last ascending, -0 before +0, keys in the caller's bit patterns."""
    sp = N.specials16(kt)
    for desc in (False, True):
        for n in (5000, 40013):
            keys = N.gen16("special", n, seed=n, kt=kt)
            assert np.isin(sp, keys).all()
            case = Case(gs, cuda, keys, kt, desc, "special")
            cuts = N.run_cuts(case.ref)
            for j, k in enumerate(sorted(set(cuts[:9] + cuts[-9:] + [n // 2]))):
                case.check(k, MODES[j % 3])
        if kt != I16:
            neg_nan, pos_nan = (0xFE00, 0x7E00) if kt == F16 else (0xFFC0, 0x7FC0)
            keys = np.array([0x0000, pos_nan, 0x8000, neg_nan, 0x3C00, 0xBC00], np.uint16)
            ek = N.Ref16(keys, kt, desc).topk(6)[0].tolist()
            want = [neg_nan, 0xBC00, 0x8000, 0x0000, 0x3C00, pos_nan]
            assert ek == (want[::-1] if desc else want)
            Case(gs, cuda, keys, kt, desc).check(6, ARGS, expect_route=3)


# ------------------------------------------------------------------------------------------------ k = 1, k = n --
@pytest.mark.parametrize("kind,route", [("uniform", 1), ("top3", 2)])
def test_k_is_one_and_k_is_n(gs, cuda, kind, route):
    """k = n selects everything: the result is the whole stable sort."""
    n = 100003
    for i, (kt, desc) in enumerate(((U16, True), (BF16, False))):
        case = Case(gs, cuda, N.gen16(kind, n, seed=40 + i, kt=kt), kt, desc, kind)
        for mode in MODES:
            case.check(1, mode, expect_route=route)
            case.check(n, mode, expect_route=route)
        assert np.array_equal(case.ref.topk(n)[1], case.ref.order)


# ----------------------------------------------------------------------------------------------------- layout --
@pytest.mark.parametrize("n,k", [(777, 333), (24583, 5001), (100003, 65537)])
def test_two_byte_alignment_of_the_key_arrays(gs, cuda, n, k):
    """Odd n and odd k; the key input and the key output at the start of their allocations and one element (2 bytes) in; the
    input is unchanged after the calls."""
    assert n % 2 == 1 and k % 2 == 1
    for i, (kt, desc) in enumerate(((U16, False), (F16, True))):
        keys = np.clip(N.gen16("uniform" if i else "zipf", n, seed=50 + i, kt=U16), 1, 0xFFFE)
        for in_off in (0, 1):
            case = Case(gs, cuda, keys, kt, desc, "layout", in_off=in_off)
            before_k, before_v = case.d_keys.clone(), case.d_vals.clone()
            assert (case.d_keys.data_ptr() + 2 * in_off) % 4 == 2 * in_off
            for out_off in (0, 1):
                for mode in MODES:
                    case.check(k, mode, out_off=out_off)
            assert torch.equal(case.d_keys, before_k) and torch.equal(case.d_vals, before_v)


# -------------------------------------------------------------------------------------------- buffer contracts --
GUARDED = [(5000, 777, 3), (8193, 8193, 1), (70001, 30001, 1), (200003, 1000, 2)]      # (n, k, route)


@pytest.mark.parametrize("n,k,route", GUARDED)
def test_guarded_offset_dirty_buffers(gs, cuda, n, k, route):
    """Every array in a slot of its own between guard zones, the key arrays at byte offsets 2, 6 and 10, ... from a 256-byte
    boundary (the workspace at an odd one), outputs and workspace dirty."""
    for i, mode in enumerate(MODES):
        kt, desc = (U16, F16, BF16)[i], bool(i % 2)
        keys = N.gen16("top3" if route == 2 else "uniform", n, seed=90 + i, kt=kt)
        vals = np.random.default_rng(9).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        ref = N.Ref16(keys, kt, desc, vals if mode == PAIRS else None)
        assert ref.route(k) == route
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_u16_temp_bytes(n, k, hv)
        a = Arena(cuda, seed=i)
        a.add("keys_in", 2 * n, offset=(2, 6, 10)[i], data=keys, const=True)
        a.add("vals_in", 4 * n, offset=12, data=vals, const=True)
        a.add("keys_out", 2 * k, offset=(6, 2, 14)[i], fill="random")
        a.add("vals_out", 4 * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 130)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_u16(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                a.ptr("vals_out") if hv else None, n, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev, est = ref.topk(k)
        assert status(gs, a.ptr("temp"), n, k, hv) == [route] + est + [0, 0, 0]
        assert np.array_equal(a.read("keys_out", np.uint16), ek), (mode, n, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32), ev), (mode, n, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    n, k = 30000, 10
    nb = gs.lib.gs_topk_u16_temp_bytes(n, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 2 * n, fill="random").add("keys_out", 2 * k, fill="random")
    a.add("vals_out", 4 * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), n=n, k=k, kt=U16)
        p.update(kw)
        return gs.lib.gs_topk_u16(p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["n"], p["k"], 0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=n + 1), dict(n=1 << 32), dict(kt=2), dict(kt=5), dict(kt=6),
               dict(kout=a.ptr("keys_in") + 2), dict(vout=a.ptr("keys_out") + ((2 * k - 1) & ~3)), dict(vin=a.ptr("keys_in"), vout=None),
               dict(kin=a.ptr("keys_in") + 1), dict(kout=a.ptr("keys_out") + 1), dict(vout=a.ptr("vals_out") + 2), dict(kin=None)):
        assert call(**kw) == 1, kw
    a.check()


def test_arrays_packed_at_two_bytes_per_key_are_accepted(gs, cuda):
    """The overlap check uses 2-byte key extents: values directly behind the keys' last byte (rounded up to 4) and outputs
    directly behind those share no byte and are served; one element closer, and they do."""
    n, k = 9001, 7
    keys = N.gen16("uniform", n, seed=7, kt=BF16)
    vals = np.random.default_rng(1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    a_vin = (2 * n + 3) & ~3
    a_kout = a_vin + 4 * n
    a_vout = (a_kout + 2 * k + 3) & ~3
    a_temp = a_vout + 4 * k
    nb = gs.lib.gs_topk_u16_temp_bytes(n, k, 1)
    buf = torch.zeros(a_temp + nb, dtype=torch.uint8, device=cuda)
    buf[:2 * n] = torch.from_numpy(keys.view(np.uint8).copy()).to(cuda)
    buf[a_vin:a_vin + 4 * n] = torch.from_numpy(vals.view(np.uint8).copy()).to(cuda)
    p = buf.data_ptr()
    assert p % 4 == 0 and a_vin < 4 * n
    assert gs.lib.gs_topk_u16(p + a_temp, nb, p, p + a_vin, p + a_kout, p + a_vout, n, k, 1, BF16, None) == 0
    ek, ev, _ = N.Ref16(keys, BF16, True, vals).topk(k)
    out = buf.cpu().numpy()
    assert np.array_equal(out[a_kout:a_kout + 2 * k].view(np.uint16), ek) and np.array_equal(out[a_vout:a_vout + 4 * k].view(np.uint32), ev)
    assert np.array_equal(out[:2 * n].view(np.uint16), keys)
    assert gs.lib.gs_topk_u16(p + a_temp, nb, p, p + a_vin - 4, p + a_kout, p + a_vout, n, k, 1, BF16, None) == 1
    assert gs.lib.gs_topk_u16(p + a_temp, nb, p, p + a_vin, p + a_kout, p + a_vout - 4, n, k, 1, BF16, None) == 1


def test_two_shapes_on_one_workspace_and_identical_bytes(gs, cuda):
    """A route-1 pairs call, a route-2 keys call and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    n, k, m, j = 150001, 4097, 90001, 50000
    a = Case(gs, cuda, N.gen16("uniform", n, seed=100, kt=BF16), BF16, True)
    b = Case(gs, cuda, N.gen16("top3", m, seed=101, kt=I16), I16, False)
    assert a.ref.route(k) == 1 and b.ref.route(j) == 2
    nb = max(gs.lib.gs_topk_u16_temp_bytes(n, k, 1), gs.lib.gs_topk_u16_temp_bytes(m, j, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((k,), -1, dtype=torch.int16, device=cuda), torch.full((k,), -1, dtype=torch.int32, device=cuda)) for _ in range(2)]
    kb = torch.full((j,), -1, dtype=torch.int16, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_u16(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), n, k, 1,
                                  BF16, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_u16(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, m, j, 0, I16, None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, idx, _ = a.ref.topk(k)
    assert np.array_equal(host16(outs[0][0]), ek) and np.array_equal(host32(outs[0][1]), a.vals[idx])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host16(kb), b.ref.topk(j)[0])


@pytest.mark.parametrize("n,k", [(5000, 100), (100003, 3001)])
def test_topk_is_capturable_in_a_hip_graph(gs, cuda, n, k):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers: inputs of
    route 1 and of route 2 go through the same launches."""
    sets = [N.gen16(kind, n, seed=110 + i, kt=BF16) for i, kind in enumerate(("uniform", "top3", "five"))]
    src = dev16(sets[0], cuda).view(torch.bfloat16)
    ko = torch.zeros(k, dtype=torch.bfloat16, device=cuda)
    vo = torch.full((k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopK16.MaxPairs(None, 0, None, None, None, None, n, k)
    assert nb == gs.lib.gs_topk_u16_temp_bytes(n, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopK16.MaxPairs(temp, nb, src, ko, None, vo, n, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopK16.MaxPairs(temp, nb, src, ko, None, vo, n, k)
    routes = set()
    for keys in sets:
        src.copy_(dev16(keys, cuda).view(torch.bfloat16))
        ko.view(torch.int16).fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ref = N.Ref16(keys, BF16, True)
        ek, ev, est = ref.topk(k)
        assert np.array_equal(host16(ko.view(torch.int16)), ek) and np.array_equal(host32(vo), ev)
        assert gs.DeviceTopK16.Status(temp, n, k, True) == [ref.route(k)] + est + [0, 0, 0]
        routes.add(ref.route(k))
    assert routes == ({3} if n <= TILE else {1, 2})


# ------------------------------------------------------------------------------------------ the widen identity --
@pytest.mark.parametrize("n,k,kind,route", [(6001, 257, "uniform", 3), (100003, 5000, "uniform", 1), (100003, 5000, "top3", 2)])
def test_the_widen_identity_on_the_device(gs, cuda, n, k, kind, route):
    """gs_topk_u16 against gs_topk_u32 on (uint32_t)key << 16 with the widened key type: the keys shifted back, values and
    indices unchanged, bit for bit, in all three forms.  (n is between the two calls' route-3 limits, 8192 and 17408, in no
    case: both take the same route.)"""
    for i, kt in enumerate(N.KEY_TYPES):
        desc = bool(i % 2)
        keys = N.gen16(kind, n, seed=130 + i, kt=kt)
        vals = np.random.default_rng(i).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        d16, d32, dv = dev16(keys, cuda), dev32(N.widen(keys), cuda), dev32(vals, cuda)
        for mode in MODES:
            hv = int(mode != KEYS)
            nb16, nb32 = gs.lib.gs_topk_u16_temp_bytes(n, k, hv), gs.lib.gs_topk_temp_bytes(n, k, hv)
            t16 = torch.full((nb16,), 0xA5, dtype=torch.uint8, device=cuda)
            t32 = torch.full((nb32,), 0xA5, dtype=torch.uint8, device=cuda)
            k16 = torch.full((k,), -1, dtype=torch.int16, device=cuda)
            k32, v16, v32 = (torch.full((k,), -1, dtype=torch.int32, device=cuda) for _ in range(3))
            vin = dv.data_ptr() if mode == PAIRS else None
            assert gs.lib.gs_topk_u16(t16.data_ptr(), nb16, d16.data_ptr(), vin, k16.data_ptr(), v16.data_ptr() if hv else None, n, k,
                                      int(desc), kt, None) == 0
            assert gs.lib.gs_topk_u32(t32.data_ptr(), nb32, d32.data_ptr(), vin, k32.data_ptr(), v32.data_ptr() if hv else None, n, k,
                                      int(desc), N.WIDE[kt], None) == 0
            w = host32(k32)
            assert (w & 0xFFFF == 0).all() and np.array_equal((w >> 16).astype(np.uint16), host16(k16)), (kt, mode)
            assert torch.equal(v16, v32), (kt, mode)
            st16 = status(gs, t16.data_ptr(), n, k, hv)
            st32 = (C.c_uint32 * 8)()
            assert gs.lib.gs_topk_status(t32.data_ptr(), n, k, hv, st32, None) == 0
            assert st16[0] == route == st32[0] and st16[1] == st32[1] >> 16 and st16[2:] == list(st32)[2:], (kt, mode)


# ------------------------------------------------------------------------------------------------- front ends --
def _scores(n, dtype, seed):
    """Scores on a coarse grid, many of them equal, without NaN or zero of either sign."""
    rng = np.random.default_rng(seed)
    if dtype == torch.int16:
        return torch.from_numpy(rng.integers(-3000, 3000, n).astype(np.int16))
    x = torch.from_numpy((rng.integers(-200, 200, n) / 8.0 + 0.0625).astype(np.float32)).to(dtype)
    assert not torch.isnan(x.float()).any() and (x.float() != 0).all()
    return x


_KT = {torch.int16: I16, torch.float16: F16, torch.bfloat16: BF16}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.int16])
@pytest.mark.parametrize("n,k", [(5000, 50), (100003, 1000)])
def test_topk_against_torch_topk(gs, cuda, dtype, n, k):
    """Values equal torch.topk's; the indices equal the reference (torch.topk does not promise the lowest index among ties, and
    16-bit data is full of ties); the input at the indices gives the values back."""
    wide = _scores(n + 40, dtype, seed=n).to(cuda)
    for lo in (0, 17):        # the second: a slice whose data pointer is 2- but not 4-aligned
        x = wide[lo:lo + n]
        bits = x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        for largest in (False, True):
            want = torch.topk(x, k, largest=largest, sorted=True)
            ko, io = gs.topk(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (k,) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values)
            ek, ev, _ = N.Ref16(bits, _KT[dtype], largest).topk(k)
            assert np.array_equal(host16(ko.view(torch.int16)), ek) and np.array_equal(host32(io), ev)
            assert torch.equal(x[io.long()], ko)
            k2, none = gs.topk(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(n + 40, dtype=torch.int32, device=cuda) * 3
    ko, vo = gs.topk(wide[3:3 + n], k, largest=True, values=vals[3:3 + n])
    _, io = gs.topk(wide[3:3 + n], k, largest=True, indices=True)
    assert torch.equal(ko, torch.topk(wide[3:3 + n], k, largest=True).values) and torch.equal(vo, vals[3:3 + n][io.long()])


def test_device_topk16_two_phase_form_and_refusals(gs, cuda):
    n, k = 30000, 123
    bits = N.gen16("uniform", n, seed=9, kt=BF16)
    x = dev16(bits, cuda)
    nb = gs.DeviceTopK16.MinPairs(None, 0, None, None, None, None, n, k)
    assert nb == gs.lib.gs_topk_u16_temp_bytes(n, k, 1) >= gs.DeviceTopK16.MinKeys(None, 0, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = torch.empty(k, dtype=torch.int16, device=cuda), torch.empty(k, dtype=torch.int32, device=cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) + 5
    # an explicit key type decides the order: int16 storage read as bfloat16, and as itself
    for kt, dtype_kt in ((gs.GS_KEY_BF16, BF16), (None, I16), (gs.GS_KEY_U16, U16), (gs.GS_KEY_F16, F16)):
        for desc, keys_form, pairs_form in ((False, gs.DeviceTopK16.MinKeys, gs.DeviceTopK16.MinPairs),
                                            (True, gs.DeviceTopK16.MaxKeys, gs.DeviceTopK16.MaxPairs)):
            ek, ei, est = N.Ref16(bits, dtype_kt, desc).topk(k)
            ko.fill_(-1)
            keys_form(temp, nb, x, ko, n, k, key_type=kt)
            assert np.array_equal(host16(ko), ek)
            assert gs.DeviceTopK16.Status(temp, n, k, False) == [1] + est + [0, 0, 0]
            pairs_form(temp, nb, x, ko, None, vo, n, k, key_type=kt)
            assert np.array_equal(host16(ko), ek) and np.array_equal(host32(vo), ei)
            pairs_form(temp, nb, x, ko, vals, vo, n, k, key_type=kt)
            assert np.array_equal(host32(vo), ei + 5)
    with pytest.raises(TypeError):
        gs.DeviceTopK16.MinKeys(temp, nb, x.int(), ko.int(), n, k)                                  # 4-byte keys
    with pytest.raises(TypeError):
        gs.DeviceTopK16.MinKeys(temp, nb, x.float(), ko.float(), n, k, key_type=gs.GS_KEY_BF16)
    with pytest.raises(TypeError):
        gs.DeviceTopK16.MinKeys(temp, nb, x, ko, n, k, key_type=gs.GS_KEY_F32)                      # a 32-bit type for 2-byte keys
    with pytest.raises(ValueError):
        gs.DeviceTopK16.MinKeys(temp, nb, x, ko.int(), n, k)                                        # a 4-byte key output
    with pytest.raises(ValueError):
        gs.DeviceTopK16.MinKeys(temp, nb, x, ko[:k - 1], n, k)                                      # a short output
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopK16.MinKeys(temp, gs.DeviceTopK16.MinKeys(None, 0, None, None, n, k) - 256, x, ko, n, k)   # a short workspace
    with pytest.raises(TypeError):
        gs.topk(x.to(torch.int8), 2)


# --------------------------------------------------------------------------------------------------- launches --
# (n, k, route): one tile (route 3); uniform key words (route 1); one top byte for all 70001 keys, 4465 more than the candidate
# list of 65536 holds (route 2).  k = 100: the sort of the staged elements takes its small path; k = 40000: it spans tiles.
LAUNCH_SHAPES = [(1000, 100, 3), (70001, 100, 1), (70001, 40000, 1), (70001, 100, 2), (70001, 40000, 2)]
# {kernel name: launches} of KernelProfile.read(), per (key bits, n, k, route) in the order keys, pairs, arguments.  Recorded
# on an MI355X from this test at the commit before the two widths' host plans became one (the commit that added gs_topk_u16),
# not derived from the code.  'other' holds the top-k kernels themselves; the rest is the sort of the staged elements, for
# 16-bit keys also round one's narrow upsweep and spine scan, and in route 3 the sort of the whole array.
_SMALL32 = {'lsb_upsweep': 1, 'lsb_scan': 1, 'msb_local_sort': 1}
_TILES32 = {'lsb_upsweep': 5, 'lsb_scan': 5, 'lsb_downsweep': 4}
_NARROW = {'lsb_upsweep': 3, 'lsb_scan': 3, 'lsb_downsweep': 2}
_ROUTE3_16 = {'lsb_upsweep': 2, 'lsb_scan': 2, 'lsb_downsweep': 2}
LAUNCHES = {
    (32, 1000, 100, 3): ({'msb_local_sort': 1, 'other': 1}, {'msb_local_sort': 1, 'other': 1}, {'msb_local_sort': 1, 'other': 2}),
    (32, 70001, 100, 1): ({**_SMALL32, 'other': 11}, {**_SMALL32, 'other': 12}, {**_SMALL32, 'other': 11}),
    (32, 70001, 40000, 1): ({**_TILES32, 'other': 11}, {**_TILES32, 'other': 12}, {**_TILES32, 'other': 11}),
    (32, 70001, 100, 2): ({**_SMALL32, 'other': 11}, {**_SMALL32, 'other': 12}, {**_SMALL32, 'other': 11}),
    (32, 70001, 40000, 2): ({**_TILES32, 'other': 11}, {**_TILES32, 'other': 12}, {**_TILES32, 'other': 11}),
    (16, 1000, 100, 3): ({**_ROUTE3_16, 'other': 1}, {**_ROUTE3_16, 'other': 1}, {**_ROUTE3_16, 'other': 2}),
    (16, 70001, 100, 1): ({**_NARROW, 'other': 7}, {**_NARROW, 'other': 8}, {**_NARROW, 'other': 7}),
    (16, 70001, 40000, 1): ({**_NARROW, 'other': 7}, {**_NARROW, 'other': 8}, {**_NARROW, 'other': 7}),
    (16, 70001, 100, 2): ({**_NARROW, 'other': 7}, {**_NARROW, 'other': 8}, {**_NARROW, 'other': 7}),
    (16, 70001, 40000, 2): ({**_NARROW, 'other': 7}, {**_NARROW, 'other': 8}, {**_NARROW, 'other': 7}),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,k,route", LAUNCH_SHAPES)
@pytest.mark.parametrize("bits", [32, 16])
def test_launches_of_every_route_and_form(gs, cuda, bits, n, k, route, mode):
    """The launches of one call, by kernel name, for both widths: the plan enqueues the same kernels whatever the data, so the
    whole dict is pinned.  The route is read back from the status words, and the keys are the first k of the sorted words."""
    front, np_t, torch_t, to_dev, to_host = ((gs.DeviceTopK16, np.uint16, torch.int16, dev16, host16) if bits == 16 else
                                             (gs.DeviceTopK, np.uint32, torch.int32, dev32, host32))
    words = np.random.default_rng(bits + n).integers(0, 1 << bits, n, dtype=np.uint64)
    if route == 2:
        words = (words >> np.uint64(8)) | np.uint64(0x42 << (bits - 8))
    words = words.astype(np_t)
    d_keys = to_dev(words, cuda)
    ko = torch.empty(k, dtype=torch_t, device=cuda)
    vo = torch.empty(k, dtype=torch.int32, device=cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) if mode == PAIRS else None
    kt = gs.GS_KEY_U16 if bits == 16 else gs.GS_KEY_U32
    hv = mode != KEYS
    if hv:
        nb = front.MinPairs(None, 0, None, None, None, None, n, k)
    else:
        nb = front.MinKeys(None, 0, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    with gs.KernelProfile() as prof:
        if hv:
            front.MinPairs(temp, nb, d_keys, ko, vals, vo, n, k, key_type=kt)
        else:
            front.MinKeys(temp, nb, d_keys, ko, n, k, key_type=kt)
    got = {name: launches for name, (_, launches) in prof.read().items()}
    print("LAUNCHES", (bits, n, k, route), mode, got)
    assert front.Status(temp, n, k, hv)[0] == route
    assert np.array_equal(to_host(ko), np.sort(words, kind="stable")[:k])
    assert got == LAUNCHES[(bits, n, k, route)][MODES.index(mode)]


def test_every_route_is_taken_in_this_file(gs, cuda):
    assert Case(gs, cuda, N.gen16("uniform", 4000, seed=1), U16, False).check(100, PAIRS) == 3
    assert Case(gs, cuda, N.gen16("uniform", 90000, seed=1), U16, False).check(100, PAIRS) == 1
    assert Case(gs, cuda, N.gen16("top3", 90000, seed=1), U16, False).check(100, PAIRS) == 2
    assert {1, 2, 3} <= ROUTES_SEEN


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_narrow_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 4 * 8 * 3 * 3
    assert all(("route %d" % r) in out.stdout for r in (1, 2, 3))
