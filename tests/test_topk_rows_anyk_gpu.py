"""gs_topk_rows_anyk_u32 on the device: every row bit for bit against tests/topk_rows_anyk_ref.py (keys, values or columns) and
every row's status words, over the shapes of both paths read from the plan, the digit edges of the three counting rounds, tie
runs across tile and slab boundaries, agreement with gs_topk_rows_u32 and gs_topk_u32, a row stride with a gap that would win,
guarded, offset and dirty buffers, refused calls, workspace reuse, identical bytes, graph capture, the Python front end and the
C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_ref as R
import topk_rows_anyk_ref as RA
from guarded import Arena
from topk_cases import DISTS, gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written


@pytest.fixture(scope="module")
def geom(gs):
    """(T, S): the tile and the slab in columns, read from the plan; the shape tables of the reference module assume them."""
    p = gs.DeviceTopKRowsAnyK.Plan(1, 1 << 20, 5000)
    assert p[0] == 2 and p[2] == RA.CH and p[3] == RA.TILE and p[3] * p[4] == RA.SLAB
    return p[3], p[3] * p[4]


# ------------------------------------------------------------------------------------------------------- inputs --
def matrix(rows, cols, kt, seed, stride=None, kinds=DISTS):
    """[rows, stride] keys: row r has its own data of distribution kinds[r % len(kinds)]; the gap is filled by the caller."""
    stride = stride or cols
    m = np.zeros((rows, stride), np.uint32)
    for r in range(rows):
        m[r, :cols] = gen(kinds[(r + seed) % len(kinds)], cols, seed=seed * 1009 + r + 1, kt=kt)
    return m


def values_for(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def status_of(gs, temp, rows, cols, k, hv, row):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_rows_anyk_status(temp.data_ptr(), rows, cols, k, hv, row, out, None) == 0
    return list(out)


class Case:
    """One matrix on the device with its reference; .check(rows, k, mode) runs the C entry point on the first `rows` rows and
    compares every row and, for up to eight rows, every status word.  Returns the status of row 0."""

    def __init__(self, gs, cuda, mat, cols, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride = mat, mat.shape[1]
        self.vals = values_for(mat.shape)
        self.d_keys, self.d_vals = dev(mat, cuda), dev(self.vals, cuda)
        self.order = {}

    def expect(self, rows, k, mode):
        ko, vo = np.empty((rows, k), np.uint32), np.empty((rows, k), np.uint32)
        for r in range(rows):
            if r not in self.order:
                self.order[r] = R.ranks(self.mat[r, :self.cols], self.kt, self.desc)
            o = self.order[r][:k]
            ko[r] = self.mat[r, o]
            vo[r] = self.vals[r, o] if mode == PAIRS else o
        return ko, vo

    def check(self, rows, k, mode, path=None):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc)
        if path is not None:
            assert gs.DeviceTopKRowsAnyK.Plan(rows, cols, k, hv)[0] == path, what
        nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                          ko.data_ptr(), vo.data_ptr() if hv else None, rows, cols, self.stride, k, int(self.desc),
                                          self.kt, None)
        assert rc == 0, (rc, what)
        ek, ev = self.expect(rows, k, mode)
        gk, gv = host(ko), host(vo)
        bad = np.nonzero((gk[:rows * k].reshape(rows, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of rows", bad[:8])
        assert (gk[rows * k:] == 0xFFFFFFFF).all(), what
        if hv:
            bad = np.nonzero((gv[:rows * k].reshape(rows, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of rows", bad[:8])
            assert (gv[rows * k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        first = None
        for r in range(min(rows, 8)):
            got = status_of(gs, temp, rows, cols, k, hv, r)
            assert got == RA.status(self.mat[r, :cols], k, self.kt, self.desc), (what, "status of row", r)
            first = first or got
        return first


def rotate(i):
    return (U32, I32, F32)[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def test_the_rotation_reaches_every_type_direction_and_form():
    seen = {rotate(i) for i in range(18)}
    assert {s[0] for s in seen} == {U32, I32, F32} and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == set(MODES)


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RA.PATH1_COLS)
def test_path1_one_workgroup_per_row(gs, cuda, cols):
    ci = RA.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RA.path1_ks(cols)):
        for i, rows in enumerate(RA.PATH1_ROWS):
            kt, desc, mode = rotate(3 * ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, matrix(max(RA.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, path=1)


def test_path1_every_type_direction_and_form(gs, cuda):
    cols, rows, k = 5000, 3, 1500
    for kt in (U32, I32, F32):
        for desc in (False, True):
            c = Case(gs, cuda, matrix(rows, cols, kt, seed=30 + kt), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=1)


# ------------------------------------------------------------------------------------------------------- path 2 --
@pytest.mark.parametrize("cols", RA.PATH2_COLS)
def test_path2_radix_select_over_all_rows(gs, cuda, geom, cols):
    ci = RA.PATH2_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RA.path2_ks(cols)):
        for i, rows in enumerate(RA.PATH2_ROWS):
            kt, desc, mode = rotate(ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, matrix(max(RA.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, path=2)


def test_path2_every_type_direction_and_form(gs, cuda, geom):
    T, S = geom
    cols, rows, k = S + T + 3, 2, 3000
    for kt in (U32, I32, F32):
        for desc in (False, True):
            c = Case(gs, cuda, matrix(rows, cols, kt, seed=40 + kt, kinds=["uniform", "zipf", "special"]), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=2)


def test_path2_many_rows_of_one_slab(gs, cuda, geom):
    rows, cols, k = RA.MANY_ROWS
    p = gs.DeviceTopKRowsAnyK.Plan(rows, cols, k)
    assert p[0] == 2 and p[5] == 1
    c = Case(gs, cuda, matrix(rows, cols, F32, seed=50), cols, F32, True)
    c.check(rows, k, ARGS, path=2)
    c.check(rows, k, KEYS, path=2)


# -------------------------------------------------------------------------------------------------- digit edges --
def _rng_row(rng, cols, lo, hi):
    return rng.integers(lo, hi, cols, dtype=np.uint64).astype(np.uint32)


def test_every_image_shares_its_top_11_or_22_bits(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 77, 2
    rng = np.random.default_rng(7)
    top11 = np.stack([_rng_row(rng, cols, 0, 1 << 21) | np.uint32(0x5A2 << 21) for _ in range(rows)])
    st = Case(gs, cuda, top11, cols, U32, False).check(rows, 2000, ARGS, path=2)
    assert st[4] == cols and st[1] >> 21 == 0x5A2 and st[5] < cols
    top22 = np.stack([_rng_row(rng, cols, 0, 1 << 10) | np.uint32(0x2AAAAA << 10) for _ in range(rows)])
    for desc in (False, True):
        st = Case(gs, cuda, top22, cols, U32, desc).check(rows, 2000, PAIRS, path=2)
        assert st[4] == cols and st[5] == cols


def test_kth_in_the_first_and_the_last_bin_of_round_one(gs, cuda, geom):
    T, S = geom
    cols, rows = S + T + 1, 2
    rng = np.random.default_rng(8)
    mat = np.stack([_rng_row(rng, cols, 1 << 21, 0xFFE00000) for _ in range(rows)])     # bins 1 .. 2046
    low, high = rng.choice(cols, 3000, replace=False), rng.choice(cols, 2500, replace=False)
    m0, m1 = mat.copy(), mat.copy()
    m0[:, low] = _rng_row(rng, 3000, 0, 1 << 21)                    # 3000 elements in bin 0
    m1[:, high] = _rng_row(rng, 2500, 0xFFE00000, 1 << 32)          # 2500 elements in bin 2047
    st = Case(gs, cuda, m0, cols, U32, False).check(rows, 1500, ARGS, path=2)
    assert st[1] >> 21 == 0 and st[4] == 3000
    st = Case(gs, cuda, m1, cols, U32, False).check(rows, cols - 1200, KEYS, path=2)
    assert st[1] >> 21 == 2047 and st[4] == 2500
    st = Case(gs, cuda, m1, cols, U32, True).check(rows, 1200, ARGS, path=2)     # descending: the same elements, image bin 0
    assert st[1] >> 21 == 0 and st[4] == 2500
    st = Case(gs, cuda, m0, cols, U32, False).check(rows, 3000, PAIRS, path=2)   # the picked bin holds exactly krem elements
    assert st[1] >> 21 == 0 and st[4] == 3000 and st[2] + st[3] == 3000


def test_kth_in_bin_1023_of_round_three_with_krem_one(gs, cuda, geom):
    """k - 1 keys below bin 0x200 of round one, then one key 0x400003ff alone in its bins, the rest far above: after round one
    krem is 1 and one element matches; the last digit is 1023."""
    T, S = geom
    cols, rows, k = 2 * S + 5, 2, 4097
    rng = np.random.default_rng(9)
    mat = np.stack([_rng_row(rng, cols, 0x50000000, 1 << 32) for _ in range(rows)])
    for r in range(rows):
        at = rng.choice(cols, k, replace=False)
        mat[r, at[:-1]] = _rng_row(rng, k - 1, 0, 0x3FE00000)
        mat[r, at[-1]] = 0x400003FF
    st = Case(gs, cuda, mat, cols, U32, False).check(rows, k, ARGS, path=2)
    assert st[1] == 0x400003FF and st[1] & 1023 == 1023 and st[2] == k - 1 and st[3] == 1 and st[4] == 1 and st[5] == 1
    # a picked bin that holds exactly krem elements, in rounds two and three: 600 keys share the k-th element's top 11 bits, 40 of them
    # its top 22, and the k-th is the last of both groups
    mat2 = mat.copy()
    for r in range(rows):
        far = np.nonzero(mat2[r] >= 0x50000000)[0]
        mat2[r, far[:560]] = _rng_row(rng, 560, 0x40000400, 0x40100000) & np.uint32(0xFFFFFC00)
        mat2[r, far[560:599]] = _rng_row(rng, 39, 0x40000000, 0x400003FF)
    st = Case(gs, cuda, mat2, cols, U32, False).check(rows, k + 39, PAIRS, path=2)
    assert st[1] == 0x400003FF and st[4] == 600 and st[5] == 40 and st[3] == 1


def test_f32_specials_and_i32_around_zero(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 9, 2
    rng = np.random.default_rng(10)
    tiny = np.finfo(np.float32).smallest_subnormal
    sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5], np.float32).view(np.uint32)
    sp = np.concatenate([sp, np.array([0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFC00002, 0x7F800001, 0xFF800001], np.uint32)])   # NaNs of both signs
    mat = sp[rng.integers(0, sp.size, (rows, cols))]
    run = cols // sp.size
    for desc in (False, True):
        c = Case(gs, cuda, mat, cols, F32, desc)
        for i, k in enumerate((1, run, 4 * run + 1, cols // 2, cols - run, cols - 1)):     # cuts inside the NaN, inf and zero runs
            c.check(rows, k, MODES[i % 3], path=2)
    ints = rng.integers(-40, 41, (rows, cols)).astype(np.int32).view(np.uint32)
    neg = int((ints[0].view(np.int32) < 0).sum())
    for desc in (False, True):
        c = Case(gs, cuda, ints, cols, I32, desc)
        for i, k in enumerate((neg - 1, neg, neg + 1, cols - neg)):
            c.check(rows, k, MODES[(i + 1) % 3], path=2)
    small = Case(gs, cuda, mat[:, :5000].copy(), 5000, F32, True)
    small.check(rows, 2500, PAIRS, path=1)


# --------------------------------------------------------------------------------------------------------- ties --
def test_all_keys_equal_gives_the_first_columns(gs, cuda, geom):
    T, S = geom
    rows, cols, k = 2, 2 * S + 5, S + 3
    for kt, desc in ((U32, False), (F32, True)):
        c = Case(gs, cuda, np.full((rows, cols), 0x3F800000, np.uint32), cols, kt, desc)
        assert np.array_equal(c.expect(rows, k, ARGS)[1], np.tile(np.arange(k, dtype=np.uint32), (rows, 1)))
        for mode in MODES:
            st = c.check(rows, k, mode, path=2)
            assert st[2] == 0 and st[3] == k and st[4] == cols and st[5] == cols
    c = Case(gs, cuda, np.full((rows, 6000), 7, np.uint32), 6000, I32, True)
    c.check(rows, 3000, ARGS, path=1)


def test_tie_runs_across_a_tile_and_a_slab_boundary_with_the_cut_inside(gs, cuda, geom):
    """Ten smaller keys, then a run of equal keys that starts five columns before a boundary: the cut falls behind the boundary."""
    T, S = geom
    rows, cols = 2, S + 2 * T
    rng = np.random.default_rng(5)
    for edge in (T, S):
        mat = rng.integers(1 << 20, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
        for r in range(rows):
            mat[r, edge - 5 - r:edge + 3000] = 1000
            mat[r, rng.choice(np.r_[0:edge - 30, edge + 3100:cols], 10, replace=False)] = np.arange(10, dtype=np.uint32)
        c = Case(gs, cuda, mat, cols, U32, False)
        for k in (10 + 3, 10 + 5, 10 + 6, 10 + 1500):
            ev = c.expect(rows, k, ARGS)[1]
            assert list(ev[0, 10:]) == list(range(edge - 5, edge - 5 + k - 10))
            for mode in (ARGS, PAIRS):
                st = c.check(rows, k, mode, path=2)
                assert st[1] == 1000 and st[2] == 10 and st[3] == k - 10
        Case(gs, cuda, ~mat, cols, U32, True).check(rows, 10 + 1500, ARGS, path=2)


def test_an_empty_before_group_and_a_take_of_one(gs, cuda, geom):
    T, S = geom
    rows, cols = 2, S + 100
    rng = np.random.default_rng(6)
    mat = rng.integers(1 << 20, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    mat[:, rng.choice(cols, 5000, replace=False)] = 77           # the minimum, 5000 times: less == 0 for k <= 5000
    c = Case(gs, cuda, mat, cols, U32, False)
    st = c.check(rows, 2000, ARGS, path=2)
    assert st[2] == 0 and st[3] == 2000
    uniq = np.stack([rng.permutation(cols).astype(np.uint32) * np.uint32(40503) for _ in range(rows)])     # distinct keys: take == 1
    st = Case(gs, cuda, uniq, cols, U32, False).check(rows, 2000, PAIRS, path=2)
    assert st[2] == 1999 and st[3] == 1


# -------------------------------------------------------------------------------- agreement with the other calls --
@pytest.mark.parametrize("rows,cols,path", RA.AGREE_SHAPES)
def test_agrees_with_topk_rows_and_with_a_loop_of_topk(gs, cuda, rows, cols, path):
    mat = matrix(rows, cols, F32, seed=70, kinds=["uniform", "five", "zipf"])
    d_keys = dev(mat, cuda)
    assert gs.DeviceTopKRowsAnyK.Plan(rows, cols, 3000)[0] == path

    def anyk(k):
        nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko, vo = torch.empty(rows * k, dtype=torch.int32, device=cuda), torch.empty(rows * k, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k,
                                            1, F32, None) == 0
        return ko, vo
    for k in (64, 1024):
        nb = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko, vo = torch.empty(rows * k, dtype=torch.int32, device=cuda), torch.empty(rows * k, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_rows_u32(temp.data_ptr(), nb, d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                                       F32, None) == 0
        ak, av = anyk(k)
        assert torch.equal(ak, ko) and torch.equal(av, vo)
    k = 3000
    nb = gs.lib.gs_topk_temp_bytes(cols, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = torch.empty(rows * k, dtype=torch.int32, device=cuda), torch.empty(rows * k, dtype=torch.int32, device=cuda)
    for r in range(rows):
        assert gs.lib.gs_topk_u32(temp.data_ptr(), nb, d_keys.data_ptr() + 4 * r * cols, None, ko.data_ptr() + 4 * r * k,
                                  vo.data_ptr() + 4 * r * k, cols, k, 1, F32, None) == 0
    ak, av = anyk(k)
    assert torch.equal(ak, ko) and torch.equal(av, vo)


# ------------------------------------------------------------------------------------------------- row stride --
@pytest.mark.parametrize("cols,k,path", RA.STRIDE_SHAPES)
def test_row_stride_with_a_gap_that_would_win(gs, cuda, cols, k, path):
    """row_stride = cols + 3; the gap holds 0x00000000 and 0xFFFFFFFF, the extremes of the u32 order in both directions, and no
    key of the rows equals either.  None may appear in the output, and the input is unchanged after the call."""
    rows, stride = 5, cols + 3
    for desc in (False, True):
        mat = matrix(rows, cols, U32, seed=80, stride=stride, kinds=["uniform", "topbyte", "zipf"])
        mat[:, :cols] = np.clip(mat[:, :cols], 1, 0xFFFFFFFE)
        mat[:, cols:] = np.array([0, 0xFFFFFFFF, 0 if desc else 0xFFFFFFFF], np.uint32)
        mat[:, cols] = 0xFFFFFFFF if desc else 0
        c = Case(gs, cuda, mat, cols, U32, desc)
        before_k, before_v = c.d_keys.clone(), c.d_vals.clone()
        for mode in MODES:
            ek, ev = c.expect(rows, k, mode)
            assert not np.isin(ek, [0, 0xFFFFFFFF]).any() and (mode != ARGS or (ev < cols).all())
            c.check(rows, k, mode, path=path)
        assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path", RA.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path):
    """Every array in a slot of its own between guard zones, at byte offsets 4, 8, 12, ... from a 256-byte boundary (the
    workspace at an odd one), outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = (U32, I32, F32)[i], bool(i % 2)
        mat = matrix(rows, cols, kt, seed=90 + i, stride=stride)
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRowsAnyK.Plan(rows, cols, k, hv)[0] == path
        a = Arena(cuda, seed=i)
        a.add("keys_in", 4 * span, offset=4, data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 4 * rows * k, offset=8, fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_rows_anyk_u32(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None,
                                          a.ptr("keys_out"), a.ptr("vals_out") if hv else None, rows, cols, stride, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev = RA.rows_topk(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint32).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    rows, cols, k = 3, 9000, 2000
    nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 4 * rows * cols, fill="random").add("vals_in", 4 * rows * cols, fill="random")
    a.add("keys_out", 4 * rows * k, fill="random").add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows,
                 cols=cols, stride=cols, k=k, kt=0)
        p.update(kw)
        return gs.lib.gs_topk_rows_anyk_u32(p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["rows"], p["cols"],
                                            p["stride"], p["k"], 0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=cols + 1), dict(stride=cols - 1), dict(kt=5), dict(kt=8),
               dict(rows=1 << 18, stride=1 << 14), dict(rows=1 << 20, cols=2048, stride=2048, k=2048),
               dict(vin=a.ptr("vals_in"), vout=None), dict(kin=None), dict(kout=None),
               dict(kout=a.ptr("keys_in") + 4), dict(vout=a.ptr("keys_out") + 4 * (rows * k - 1)), dict(kin=a.ptr("keys_in") + 2),
               dict(vout=a.ptr("vals_out") + 1), dict(vin=a.ptr("keys_in") + 4 * (rows * cols - 1))):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A pairs call on path 2, a keys call on path 1 and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, p2), (rows_b, cols_b, k_b, p1) = RA.REUSE_SHAPES
    assert (p2, p1) == (2, 1)
    a = Case(gs, cuda, matrix(rows, cols, F32, seed=100), cols, F32, True)
    b = Case(gs, cuda, matrix(rows_b, cols_b, I32, seed=101), cols_b, I32, False)
    nb = max(gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_anyk_temp_bytes(rows_b, cols_b, k_b, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int32, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((rows_b * k_b,), -1, dtype=torch.int32, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(),
                                            rows, cols, cols, k, 1, F32, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, rows_b, cols_b, cols_b, k_b,
                                        0, I32, None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host(kb).reshape(rows_b, k_b), b.expect(rows_b, k_b, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path", RA.GRAPH_SHAPES)
def test_topk_rows_anyk_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers."""
    sets = [matrix(rows, cols, U32, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "five"))]
    src = dev(sets[0], cuda)
    ko = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopKRowsAnyK.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert gs.DeviceTopKRowsAnyK.Plan(rows, cols, k, True)[0] == path
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopKRowsAnyK.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopKRowsAnyK.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U32)
    for mat in sets:
        src.copy_(dev(mat, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = RA.rows_topk(mat, cols, k, U32, True)
        assert np.array_equal(host(ko).reshape(rows, k), ek) and np.array_equal(host(vo).reshape(rows, k), ev)


# ------------------------------------------------------------------------------------------------- front ends --
def _distinct_floats(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.stack([(rng.permutation(cols) - cols / 3).astype(np.float32) for _ in range(rows)])     # tie-free, NaN-free


@pytest.mark.parametrize("rows,cols,k", [(4, 5000, 1500), (3, 40000, 3000)])
def test_topk_rows_anyk_against_torch_topk(gs, cuda, rows, cols, k):
    wide = torch.from_numpy(_distinct_floats(rows, cols + 40, seed=cols)).to(cuda)
    for x in (wide[:, :cols].contiguous(), wide[:, 17:17 + cols]):        # the second: a column slice
        for largest in (False, True):
            want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
            ko, io = gs.topk_rows_anyk(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values) and torch.equal(io.long(), want.indices)
            k2, none = gs.topk_rows_anyk(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows_anyk(x, k, largest=True, values=v)
    want = torch.topk(x, k, dim=1, largest=True)
    assert torch.equal(ko, want.values) and torch.equal(vo, torch.gather(v, 1, want.indices))
    ko, vo = gs.topk_rows_anyk(x, 0, indices=True)
    assert tuple(ko.shape) == (rows, 0) and tuple(vo.shape) == (rows, 0)
    ko, vo = gs.topk_rows_anyk(x[:0], k, indices=True)
    assert tuple(ko.shape) == (0, k) and tuple(vo.shape) == (0, k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(x.double(), k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(x.half(), k)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_anyk_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 6 * 3 * 3
