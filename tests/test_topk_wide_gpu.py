"""gs_topk_u64 on the device, bit for bit against tests/topk_wide_ref.py (keys, values or indices, and the eight status words,
so route, D and the passes over the input): the first shapes over every key type, direction and form, the candidate list exactly
full and one too many, D = 2 by the skip of constant bytes, D = 3 with an outlier, D = 8, route 2 on a tie run and on equal
keys, k-th images with 0x00 and 0xff at each byte, cuts on tie runs, the float specials and integer extremes, offset and
guarded buffers, refused calls, workspace reuse, identical bytes, graph capture, gs_lsb_sort_wide's own output, the Python front
ends and the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_wide_ref as W
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, I64, F64 = W.U64, W.I64, W.F64
KEYS, PAIRS, ARGS, MODES = W.KEYS, W.PAIRS, W.ARGS, W.MODES
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, k) is written
SEEN = set()         # (route, D) of every checked call


def dev64(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(cuda)


def dev32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def status(gs, temp_ptr, n, k, hv):
    st = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_u64_status(temp_ptr, n, k, hv, st, None) == 0
    return [int(x) for x in st]


class Case:
    """One input on the device with its reference (one stable argsort); .check(k, mode) runs the C entry point on a workspace
    filled with 0xA5 and outputs filled with -1 and compares keys, values or indices, the sentinels around the outputs and the
    eight status words.  in_off / out_off: the key input / output starts that many elements into its allocation."""

    def __init__(self, gs, cuda, keys, kt, desc, what="", in_off=0):
        self.gs, self.cuda, self.kt, self.desc, self.n, self.what, self.in_off = gs, cuda, kt, desc, keys.size, what, in_off
        self.vals = np.random.default_rng(3).integers(0, 1 << 32, keys.size, dtype=np.uint64).astype(np.uint32)
        self.ref = W.Ref64(keys, kt, desc)
        self.d_keys = dev64(np.concatenate([np.full(in_off, 0x5A5A5A5A5A5A5A5A, np.uint64), W.u64(keys)]), cuda)
        self.d_vals = dev32(self.vals, cuda)

    def check(self, k, mode, route=None, D=None, out_off=0):
        gs, n = self.gs, self.n
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_u64_temp_bytes(n, k, hv)
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((out_off + k + TAIL,), -1, dtype=torch.int64, device=self.cuda)
        vo = torch.full((k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_u64(temp.data_ptr(), nb, self.d_keys.data_ptr() + 8 * self.in_off,
                                self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr() + 8 * out_off,
                                vo.data_ptr() if hv else None, n, k, int(self.desc), self.kt, None)
        what = "%s n=%d k=%d %s kt=%d desc=%d off=%d/%d" % (self.what, n, k, mode, self.kt, self.desc, self.in_off, out_off)
        assert rc == 0, (rc, what)
        st = status(gs, temp.data_ptr(), n, k, hv)
        est = self.ref.status(k)
        if route is not None:
            assert est[0] == route, (what, est)
        if D is not None:
            assert est[5] == D, (what, est)
        assert est[6] == (2 if est[5] == 1 else est[5] + 2), (what, est)
        assert st == est, (what, st, est)
        SEEN.add((st[0], st[5]))
        ek, idx = self.ref.topk(k)
        gk, gv = host64(ko), host32(vo)
        assert (gk[:out_off] == W.ONES).all() and (gk[out_off + k:] == W.ONES).all() and gk[out_off + k:].size == TAIL, what
        assert np.array_equal(gk[out_off:out_off + k], ek), what
        if hv:
            assert np.array_equal(gv[:k], self.vals[idx] if mode == PAIRS else idx), what
            assert (gv[k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        return st


def rotate(i):
    return W.KEY_TYPES[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


# ------------------------------------------------------------------------------------------------- first shapes --
@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 3 * 4096 + 5])
def test_first_shapes_over_every_key_type_direction_and_form(gs, cuda, n):
    """One element, one tile less one, one tile, two tiles with a last one of one element, four with a ragged last one."""
    for kt in W.KEY_TYPES:
        for desc in (False, True):
            for i, kind in enumerate(W.DISTS):
                if (i + kt + desc) % 2 and kind not in ("uniform", "special"):
                    continue
                case = Case(gs, cuda, W.gen64(kind, n, seed=10 + i, kt=kt), kt, desc, kind)
                ks = sorted(k for k in {1, 2, n // 3, 4096, 4097, n - 1, n} if 1 <= k <= n)
                for j, k in enumerate(ks):
                    for mode in MODES if (i + j) % 4 == 0 else (MODES[(i + j + kt) % 3],):
                        case.check(k, mode, route=1, D=1)


# ---------------------------------------------------------------------------------------------- capacity boundary --
CAPACITY = [(70001, 65536), ((1 << 21) + 3 * 4096 + 1, ((1 << 21) + 3 * 4096 + 1) // 32)]


@pytest.mark.parametrize("n,cap", CAPACITY)
@pytest.mark.parametrize("dc", [0, 1])
def test_candidate_list_exactly_full_and_one_too_many(gs, cuda, n, cap, dc):
    """A top-byte bucket of cap and cap + 1 elements behind 2000 smaller ones: the list takes cap of them at D = 1 (the last
    at cand[cap - 1]) and not one more (a second round over the input, D = 2)."""
    assert W.cap(n) == cap
    c, below = cap + dc, 2000
    for i, (kt, desc) in enumerate(((U64, False), (F64, True)) if n < 100000 else ((I64, bool(dc)),)):
        case = Case(gs, cuda, W.bucket_case64(n, c, below, 0x42, n + dc, kt, desc), kt, desc, "bucket c=%d" % c)
        for j, (k, inside) in enumerate(W.bucket_ks(below, c)):
            for mode in MODES if j == 3 else (MODES[(j + i + dc) % 3],):
                st = case.check(k, mode, route=1, D=2 if inside and dc == 1 else 1)
                assert st[7] == c or not inside or dc == 1


# ------------------------------------------------------------------------------------------------- the way down --
def test_small_integers_take_two_rounds_by_the_skip_and_three_with_an_outlier(gs, cuda):
    n = 70001
    for i, desc in enumerate((False, True)):
        case = Case(gs, cuda, W.small_ints(n, 5 + i), I64, desc, "small ints")
        for j, k in enumerate((1, 1000, 40000, n)):
            st = case.check(k, MODES[(i + j) % 3], route=1, D=2)
            assert st[6] == 4
        case = Case(gs, cuda, W.small_ints(n, 7 + i, outlier=True), I64, desc, "small ints and -1")
        for j, k in enumerate((2, 1000, 40000, n - 1)):
            st = case.check(k, MODES[(i + j + 1) % 3], route=1, D=3)
            assert st[6] == 5
        case.check(n if desc else 1, ARGS, route=1, D=1)          # the outlier itself
    case = Case(gs, cuda, W.timestamps(n, 11), I64, True, "timestamps")
    for j, k in enumerate((1, 5000, n)):
        assert case.check(k, MODES[j], route=1)[5] in (2, 3)


@pytest.mark.parametrize("kt,desc", [(U64, False), (I64, True), (F64, True)])
def test_eight_rounds_over_the_input(gs, cuda, kt, desc):
    """Seven outliers, one per level, keep every byte alive; the last byte splits a bucket of cap + 1 in two."""
    case = Case(gs, cuda, W.deep_case64(kt, desc, seed=kt), kt, desc, "deep")
    n = case.n
    depths = set()
    for j, k in enumerate((1, 2, 3, 30000, 32771, 32772, n - 4, n - 3, n - 2, n - 1, n)):
        depths.add(case.check(k, MODES[(j + kt) % 3], route=1)[5])
    assert depths == {2, 3, 4, 5, 6, 7, 8}
    st = case.check(40000, PAIRS, route=1, D=8)
    assert st[6] == 10 and st[7] in (32768, 32769)


def test_route_two_on_a_tie_run_and_on_equal_keys(gs, cuda):
    n, run = 100003, 65537
    for i, (kt, desc) in enumerate(((U64, False), (F64, True), (I64, False))):
        case = Case(gs, cuda, W.tie_case64(n, run, 20 + i, kt, desc), kt, desc, "tie run")
        less = int((case.ref.img < np.uint64(0x8000000000000001)).sum())
        for j, k in enumerate((less, less + 1, less + 30000, less + run, less + run + 1)):
            st = case.check(k, MODES[(i + j) % 3], route=2 if 0 < k - less <= run else 1)
            assert k - less > run or k == less or (st[7] == run and st[3] == less and st[5] >= 2)
        case = Case(gs, cuda, W.tie_case64(n, run - 1, 30 + i, kt, desc), kt, desc, "tie run that fits")
        less = int((case.ref.img < np.uint64(0x8000000000000001)).sum())
        assert case.check(less + 5, MODES[i], route=1)[7] == run - 1
    for kt, desc, pattern in ((U64, False, 0x3FF0000000000000), (F64, True, 0xFFFFFFFFFFFFFFFF), (I64, True, 0x8000000000000000)):
        for n in (20000, 65537, 70001):
            case = Case(gs, cuda, np.full(n, pattern, np.uint64), kt, desc, "equal")
            for k in (1, 7777, n):
                for mode in MODES if k == 7777 else (MODES[(k + n) % 3],):
                    st = case.check(k, mode, route=1 if n <= 65536 else 2, D=1)      # two passes on either route
                    assert st[6] == 2 and st[7] == n and st[3] == 0
            assert np.array_equal(case.ref.topk(n)[1], np.arange(n, dtype=np.uint32))


# -------------------------------------------------------------------------------------------------- digit edges --
@pytest.mark.parametrize("p", range(8))
def test_kth_images_with_0x00_and_0xff_at_every_byte(gs, cuda, p):
    for i, (v, deep) in enumerate(((0x00, False), (0xFF, False), (0x00, True), (0xFF, True))):
        kt, desc, _ = rotate(i + p)
        case = Case(gs, cuda, W.byte_edge_case64(p, v, deep, kt, desc), kt, desc, "byte %d = %#x deep=%d" % (p, v, deep))
        ks = np.flatnonzero(W.byte_of(case.ref.sorted_img, p) == v) + 1
        for j, k in enumerate((int(ks[0]), int(ks[ks.size // 2]), int(ks[-1]))):
            st = case.check(k, MODES[(i + j) % 3], D=((2 if p in (0, 7) else 3) if deep else 1))
            assert ((st[1] | (st[2] << 32)) >> (8 * p)) & 0xFF == v


def test_cuts_on_bucket_edges_and_inside_tie_runs(gs, cuda):
    rng = np.random.default_rng(8)
    for i, kt in enumerate(W.KEY_TYPES):
        n = 70001
        keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) & np.uint64(0xC000000000000100)      # eight values
        case = Case(gs, cuda, keys, kt, bool(i % 2), "eight values")
        assert np.unique(keys).size == 8
        for j, k in enumerate(W.run_cuts(case.ref)):
            case.check(k, MODES[(i + j) % 3])
    case = Case(gs, cuda, W.gen64("uniform", 50021, seed=5), F64, True, "uniform")
    tops = np.flatnonzero(np.diff(W.byte_of(case.ref.sorted_img, 7))) + 1
    for j, k in enumerate(tops[:3].tolist() + (tops[:3] + 1).tolist() + tops[-3:].tolist()):
        case.check(k, MODES[j % 3], route=1, D=1)


# ------------------------------------------------------------------------------------------------- float orders --
@pytest.mark.parametrize("kt", [F64, I64, U64])
def test_special_patterns_in_both_directions(gs, cuda, kt):
    """NaNs of both signs with payloads, +-0, +-inf and denormals (the extremes for the integer types), six in ten elements."""
    sp = W.specials64(kt)
    for desc in (False, True):
        for n in (5000, 80021):
            keys = W.gen64("special", n, seed=n, kt=kt)
            assert np.isin(sp, keys).all()
            case = Case(gs, cuda, keys, kt, desc, "special")
            cuts = W.run_cuts(case.ref)
            for j, k in enumerate(sorted(set(cuts[:7] + cuts[-7:] + [n // 2]))):
                case.check(k, MODES[j % 3])
    if kt == F64:
        keys = np.array([0, 0x7FF8000000000001, 1 << 63, 0xFFF8000000000001, 0x3FF0000000000000, 0xBFF0000000000000], np.uint64)
        want = [keys[i] for i in (3, 5, 2, 0, 4, 1)]
        assert W.Ref64(keys, F64).topk(6)[0].tolist() == want
        Case(gs, cuda, keys, F64, False).check(6, ARGS)
        Case(gs, cuda, keys, F64, True).check(6, PAIRS)


# ----------------------------------------------------------------------------------------------------- layout --
@pytest.mark.parametrize("n,k", [(777, 333), (24583, 5001), (100003, 65537)])
def test_key_arrays_offset_by_one_element(gs, cuda, n, k):
    for i, (kt, desc) in enumerate(((U64, False), (F64, True))):
        keys = W.gen64("uniform" if i else "small", n, seed=50 + i)
        for in_off in (0, 1):
            case = Case(gs, cuda, keys, kt, desc, "layout", in_off=in_off)
            before_k, before_v = case.d_keys.clone(), case.d_vals.clone()
            for out_off in (0, 1):
                for mode in MODES:
                    case.check(k, mode, out_off=out_off)
            assert torch.equal(case.d_keys, before_k) and torch.equal(case.d_vals, before_v)


GUARDED = [(5000, 777, 1, 1), (4097, 4097, 1, 1), (70001, 30001, 1, 2), (70001, 1000, 2, 1)]      # (n, k, route, D)


@pytest.mark.parametrize("n,k,route,D", GUARDED)
def test_guarded_offset_dirty_buffers(gs, cuda, n, k, route, D):
    """Every array in a slot of its own between guard zones, the key arrays at byte offsets 8, 24 and 40, ... from a 256-byte
    boundary (the workspace at an odd one), outputs and workspace dirty."""
    for i, mode in enumerate(MODES):
        kt, desc = W.KEY_TYPES[i], bool(i % 2)
        keys = (np.full(n, 0x4045, np.uint64) if route == 2 else W.small_ints(n, 90 + i) if D == 2 else W.gen64("uniform", n, 90 + i))
        vals = np.random.default_rng(9).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        ref = W.Ref64(keys, kt, desc, vals if mode == PAIRS else None)
        est = ref.status(k)
        assert est[0] == route and est[5] == D
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_u64_temp_bytes(n, k, hv)
        a = Arena(cuda, seed=i)
        a.add("keys_in", 8 * n, offset=(8, 24, 40)[i], data=keys, const=True)
        a.add("vals_in", 4 * n, offset=12, data=vals, const=True)
        a.add("keys_out", 8 * k, offset=(24, 8, 56)[i], fill="random")
        a.add("vals_out", 4 * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 130)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_u64(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                a.ptr("vals_out") if hv else None, n, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev = ref.topk(k)
        assert status(gs, a.ptr("temp"), n, k, hv) == est
        assert np.array_equal(a.read("keys_out", np.uint64), ek), (mode, n, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32), ev), (mode, n, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    n, k = 30000, 10
    nb = gs.lib.gs_topk_u64_temp_bytes(n, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 8 * n, fill="random").add("keys_out", 8 * k, fill="random")
    a.add("vals_out", 4 * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), n=n, k=k, kt=U64)
        p.update(kw)
        return gs.lib.gs_topk_u64(p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["n"], p["k"], 0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=n + 1), dict(n=1 << 32), dict(kt=2), dict(kt=8), dict(kt=6),
               dict(kout=a.ptr("keys_in") + 8), dict(vout=a.ptr("keys_out") + 8 * k - 4), dict(vin=a.ptr("keys_in"), vout=None),
               dict(kin=a.ptr("keys_in") + 4), dict(kout=a.ptr("keys_out") + 4), dict(vout=a.ptr("vals_out") + 2), dict(kin=None)):
        assert call(**kw) == 1, kw
    a.check()


def test_two_shapes_on_one_workspace_and_identical_bytes(gs, cuda):
    """A D = 1 pairs call, a D = 2 keys call of another shape and the first one again, on one stream and one workspace without
    a synchronisation between them: the third call's bytes equal the first's."""
    n, k, m, j = 150001, 4097, 90001, 50000
    a = Case(gs, cuda, W.gen64("uniform", n, seed=100), F64, True)
    b = Case(gs, cuda, W.small_ints(m, 101), I64, False)
    assert a.ref.status(k)[5] == 1 and b.ref.status(j)[5] == 2
    nb = max(gs.lib.gs_topk_u64_temp_bytes(n, k, 1), gs.lib.gs_topk_u64_temp_bytes(m, j, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((k,), -1, dtype=torch.int64, device=cuda), torch.full((k,), -1, dtype=torch.int32, device=cuda)) for _ in range(2)]
    kb = torch.full((j,), -1, dtype=torch.int64, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_u64(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), n, k, 1,
                                  F64, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_u64(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, m, j, 0, I64, None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, idx = a.ref.topk(k)
    assert np.array_equal(host64(outs[0][0]), ek) and np.array_equal(host32(outs[0][1]), a.vals[idx])
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host64(kb), b.ref.topk(j)[0])


@pytest.mark.parametrize("n,k", [(5000, 100), (100003, 3001)])
def test_topk_is_capturable_in_a_hip_graph(gs, cuda, n, k):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers: inputs that
    stop at D = 1, take the skip, and end on a tie run go through the same launches."""
    sets = [W.gen64("uniform", n, 110), W.small_ints(n, 111), np.full(n, 5, np.uint64), W.gen64("five", n, 112)]
    src = dev64(sets[0], cuda)
    ko = torch.zeros(k, dtype=torch.int64, device=cuda)
    vo = torch.full((k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopK64.MaxPairs(None, 0, None, None, None, None, n, k)
    assert nb == gs.lib.gs_topk_u64_temp_bytes(n, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopK64.MaxPairs(temp, nb, src, ko, None, vo, n, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopK64.MaxPairs(temp, nb, src, ko, None, vo, n, k)
    seen = set()
    for keys in sets:
        src.copy_(dev64(keys, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ref = W.Ref64(keys, I64, True)
        ek, ev = ref.topk(k)
        assert np.array_equal(host64(ko), ek) and np.array_equal(host32(vo), ev)
        st = gs.DeviceTopK64.Status(temp, n, k, True)
        assert st == ref.status(k)
        seen.add((st[0], st[5]))
    assert seen == ({(1, 1)} if n <= 65536 else {(1, 1), (1, 2), (2, 1)})


def test_against_the_wide_sort_on_the_device(gs, cuda):
    """S itself: gs_lsb_sort_wide of the (key, index) pairs, its first k against the call's output, bit for bit."""
    n, k = 200003, 70001
    for kt, desc, keys in ((F64, True, W.gen64("special", n, 1, F64)), (I64, False, W.small_ints(n, 2, outlier=True))):
        d_keys = dev64(keys, cuda)
        bufs = [d_keys.clone(), torch.empty_like(d_keys)]
        vals = [torch.arange(n, dtype=torch.int32, device=cuda), torch.empty(n, dtype=torch.int32, device=cuda)]
        nb = gs.lib.gs_lsb_wide_temp_bytes(n, 8, 4)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        sel = C.c_int(0)
        kp, vp = (C.c_void_p * 2)(bufs[0].data_ptr(), bufs[1].data_ptr()), (C.c_void_p * 2)(vals[0].data_ptr(), vals[1].data_ptr())
        assert gs.lib.gs_lsb_sort_wide(temp.data_ptr(), nb, kp, vp, C.byref(sel), n, 8, 4, 0, 64, int(desc), kt, None) == 0
        torch.cuda.synchronize()
        ko, vo = gs.topk(d_keys if kt == I64 else d_keys.view(torch.float64), k, largest=desc, indices=True)
        assert torch.equal(ko.view(torch.int64), bufs[sel.value][:k]) and torch.equal(vo, vals[sel.value][:k])


# ------------------------------------------------------------------------------------------------- front ends --
@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
@pytest.mark.parametrize("n,k", [(5000, 50), (100003, 1000)])
def test_topk_against_torch_topk(gs, cuda, dtype, n, k):
    """Values equal torch.topk's; the indices equal the reference (torch.topk does not promise the lowest index among ties);
    the input at the indices gives the values back."""
    rng = np.random.default_rng(n)
    if dtype == torch.int64:
        wide = torch.from_numpy(rng.integers(-3000, 3000, n + 8).astype(np.int64)).to(cuda)
    else:
        wide = torch.from_numpy(rng.integers(-200, 200, n + 8) / 8.0 + 0.0625).to(cuda)
    for lo in (0, 3):
        x = wide[lo:lo + n]
        bits = x.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)
        for largest in (False, True):
            want = torch.topk(x, k, largest=largest, sorted=True)
            ko, io = gs.topk(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (k,) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values)
            ek, ev = W.Ref64(bits, I64 if dtype == torch.int64 else F64, largest).topk(k)
            assert np.array_equal(host64(ko.view(torch.int64)), ek) and np.array_equal(host32(io), ev)
            assert torch.equal(x[io.long()], ko)
            k2, none = gs.topk(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(n + 8, dtype=torch.int32, device=cuda) * 3
    ko, vo = gs.topk(wide[3:3 + n], k, largest=True, values=vals[3:3 + n])
    _, io = gs.topk(wide[3:3 + n], k, largest=True, indices=True)
    assert torch.equal(ko, torch.topk(wide[3:3 + n], k, largest=True).values) and torch.equal(vo, vals[3:3 + n][io.long()])


def test_device_topk64_two_phase_form_and_refusals(gs, cuda):
    n, k = 30000, 123
    bits = W.gen64("uniform", n, seed=9)
    x = dev64(bits, cuda)
    nb = gs.DeviceTopK64.MinPairs(None, 0, None, None, None, None, n, k)
    assert nb == gs.lib.gs_topk_u64_temp_bytes(n, k, 1) >= gs.DeviceTopK64.MinKeys(None, 0, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = torch.empty(k, dtype=torch.int64, device=cuda), torch.empty(k, dtype=torch.int32, device=cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) + 5
    # an explicit key type decides the order: int64 storage read as doubles, as unsigned, and as itself
    for kt, ref_kt in ((gs.GS_KEY_F64, F64), (None, I64), (gs.GS_KEY_U64, U64)):
        for desc, keys_form, pairs_form in ((False, gs.DeviceTopK64.MinKeys, gs.DeviceTopK64.MinPairs),
                                            (True, gs.DeviceTopK64.MaxKeys, gs.DeviceTopK64.MaxPairs)):
            ref = W.Ref64(bits, ref_kt, desc)
            ek, ei = ref.topk(k)
            ko.fill_(-1)
            keys_form(temp, nb, x, ko, n, k, key_type=kt)
            assert np.array_equal(host64(ko), ek)
            assert gs.DeviceTopK64.Status(temp, n, k, False) == ref.status(k)
            pairs_form(temp, nb, x, ko, None, vo, n, k, key_type=kt)
            assert np.array_equal(host64(ko), ek) and np.array_equal(host32(vo), ei)
            pairs_form(temp, nb, x, ko, vals, vo, n, k, key_type=kt)
            assert np.array_equal(host32(vo), ei + 5)
    with pytest.raises(TypeError):
        gs.DeviceTopK64.MinKeys(temp, nb, x.int(), ko.int(), n, k)                                  # 4-byte keys
    with pytest.raises(TypeError):
        gs.DeviceTopK64.MinKeys(temp, nb, x, ko, n, k, key_type=gs.GS_KEY_F32)                      # a 32-bit type for 8-byte keys
    with pytest.raises(TypeError):
        gs.DeviceTopK.MinKeys(temp, nb, x, ko, n, k)                                                # the 32-bit class keeps refusing
    with pytest.raises(ValueError):
        gs.DeviceTopK64.MinKeys(temp, nb, x, ko.int(), n, k)                                        # a 4-byte key output
    with pytest.raises(ValueError):
        gs.DeviceTopK64.MinKeys(temp, nb, x, ko[:k - 1], n, k)                                      # a short output
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopK64.MinKeys(temp, gs.DeviceTopK64.MinKeys(None, 0, None, None, n, k) - 256, x, ko, n, k)   # a short workspace


def test_every_way_down_is_taken_in_this_file(gs, cuda):
    assert Case(gs, cuda, W.gen64("uniform", 90000, 1), U64, False).check(100, PAIRS)[:1] == [1]
    assert Case(gs, cuda, np.full(90000, 9, np.uint64), U64, False).check(100, PAIRS)[:1] == [2]
    assert {(1, 1), (1, 2), (1, 3), (1, 8), (2, 1)} <= SEEN and any(r == 2 and d >= 2 for r, d in SEEN)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_wide_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 3 * 8 * 3 * 3
    assert all(("route %d" % r) in out.stdout for r in (1, 2)) and "D 2" in out.stdout
