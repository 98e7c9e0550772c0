"""gs_topk_rows_anyk_u16 on the device: every row bit for bit against tests/topk_rows_anyk_narrow_ref.py (keys, values or columns)
and every row's status words, over the shapes of both paths read from the plan, the digit edges of the two counting rounds, tie
runs across tile and slab boundaries and rows longer than the 65536 patterns, the four key types with their special values,
agreement with gs_topk_rows_u16, gs_topk_u16, gs_topk_rows_anyk_u32 on the widened matrix and torch.topk, a row stride with a
gap that would win, a key base at 2 mod 4, guarded, offset and dirty buffers, refused calls, workspace reuse, identical bytes,
graph capture, the Python front end and the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_rows_anyk_narrow_ref as RN
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = RN.KEY_TYPES
KEYS, PAIRS, ARGS, MODES = RN.KEYS, RN.PAIRS, RN.ARGS, RN.MODES
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written


@pytest.fixture(scope="module")
def geom(gs):
    """(T, S): the tile and the slab in columns, read from the plan; the shape tables of the reference module assume them."""
    p = gs.DeviceTopKRowsAnyK16.Plan(1, 1 << 20, 5000)
    assert p[0] == 2 and p[1] == 9 and p[2] == RN.CH and p[3] == RN.TILE and p[3] * p[4] == RN.SLAB
    assert gs.lib.gs_segmented_narrow_cap(U16, 4) == 8192 == gs.lib.gs_segmented_narrow_cap(U16, 0)      # the k = 8192 / 8193 edge
    return p[3], p[3] * p[4]


# ------------------------------------------------------------------------------------------------------- inputs --
def values_for(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def dev16(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(cuda)


def dev32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def status_of(gs, temp, rows, cols, k, hv, row):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_rows_anyk_u16_status(temp.data_ptr(), rows, cols, k, hv, row, out, None) == 0
    return list(out)


def anyk16(gs, temp, nb, kin, vin, kout, vout, rows, cols, stride, k, desc, kt):
    return gs.lib.gs_topk_rows_anyk_u16(temp, nb, kin, vin, kout, vout, rows, cols, stride, k, int(desc), kt, None)


class Case:
    """One matrix of uint16 bit patterns on the device with its reference (one stable argsort per row, computed once);
    .check(rows, k, mode) runs the C entry point on the first `rows` rows and compares every row and, for up to eight rows,
    every status word.  Returns the status of row 0."""

    def __init__(self, gs, cuda, mat, cols, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride = np.ascontiguousarray(mat, dtype=np.uint16), mat.shape[1]
        self.vals = values_for(mat.shape)
        self.d_keys, self.d_vals = dev16(self.mat, cuda), dev32(self.vals, cuda)
        self.order = RN.rows_order(self.mat, cols, kt, desc)

    def expect(self, rows, k, mode):
        return RN.rows_topk16(self.mat[:rows], self.cols, k, self.kt, self.desc, self.vals[:rows] if mode == PAIRS else None,
                              order=self.order[:rows])

    def check(self, rows, k, mode, path=None):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc)
        if path is not None:
            assert gs.DeviceTopKRowsAnyK16.Plan(rows, cols, k, hv)[0] == path, what
        nb = gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((rows * k + TAIL,), -1, dtype=torch.int16, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = anyk16(gs, temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                    vo.data_ptr() if hv else None, rows, cols, self.stride, k, self.desc, self.kt)
        assert rc == 0, (rc, what)
        ek, ev = self.expect(rows, k, mode)
        gk, gv = host16(ko), host32(vo)
        bad = np.nonzero((gk[:rows * k].reshape(rows, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of rows", bad[:8])
        assert (gk[rows * k:] == 0xFFFF).all(), what
        if hv:
            bad = np.nonzero((gv[:rows * k].reshape(rows, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of rows", bad[:8])
            assert (gv[rows * k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        first = None
        for r in range(min(rows, 8)):
            got = status_of(gs, temp, rows, cols, k, hv, r)
            assert got == RN.status(self.mat[r, :cols], k, self.kt, self.desc), (what, "status of row", r)
            first = first or got
        return first


def rotate(i):
    return RN.KEY_TYPES[i % 4], bool((i // 4) % 2), MODES[(i // 2) % 3]


def test_the_rotation_reaches_every_type_direction_and_form():
    seen = {rotate(i) for i in range(24)}
    assert {s[0] for s in seen} == set(RN.KEY_TYPES) and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == set(MODES)


def images(rng, n, lo, hi):
    return rng.integers(lo, hi, n, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RN.PATH1_COLS)
def test_path1_one_workgroup_per_row(gs, cuda, cols):
    ci = RN.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RN.path1_ks(cols)):
        for i, rows in enumerate(RN.PATH1_ROWS):
            kt, desc, mode = rotate(5 * ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, RN.matrix16(max(RN.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, path=1)


def test_path1_every_type_direction_and_form(gs, cuda):
    cols, rows, k = 5000, 3, 1500
    for kt in RN.KEY_TYPES:
        for desc in (False, True):
            c = Case(gs, cuda, RN.matrix16(rows, cols, kt, seed=30 + kt, kinds=["uniform", "special", "zipf"]), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=1)


# ------------------------------------------------------------------------------------------------------- path 2 --
@pytest.mark.parametrize("cols", RN.PATH2_COLS)
def test_path2_radix_select_over_all_rows(gs, cuda, geom, cols):
    ci = RN.PATH2_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RN.path2_ks(cols)):
        for i, rows in enumerate(RN.PATH2_ROWS):
            kt, desc, mode = rotate(ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, RN.matrix16(max(RN.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, path=2)


def test_path2_every_type_direction_and_form(gs, cuda, geom):
    T, S = geom
    cols, rows, k = S + T + 3, 2, 3000
    for kt in RN.KEY_TYPES:
        for desc in (False, True):
            c = Case(gs, cuda, RN.matrix16(rows, cols, kt, seed=40 + kt, kinds=["uniform", "zipf", "special"]), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=2)


def test_path2_many_rows_of_one_slab(gs, cuda, geom):
    rows, cols, k = RN.MANY_ROWS
    p = gs.DeviceTopKRowsAnyK16.Plan(rows, cols, k)
    assert p[0] == 2 and p[5] == 1
    c = Case(gs, cuda, RN.matrix16(rows, cols, BF16, seed=50), cols, BF16, True)
    c.check(rows, k, ARGS, path=2)
    c.check(rows, k, KEYS, path=2)


# -------------------------------------------------------------------------------------------------- digit edges --
def test_every_image_shares_its_top_byte(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 77, 2
    rng = np.random.default_rng(7)
    img = np.stack([images(rng, cols, 0, 256) | np.uint64(0x5A00) for _ in range(rows)])
    for kt, desc, mode in ((U16, False, ARGS), (BF16, True, PAIRS), (I16, False, KEYS)):
        st = Case(gs, cuda, RN.keys_of(img, kt, desc), cols, kt, desc).check(rows, 2000, mode, path=2)
        assert st[4] == cols and st[1] >> 8 == 0x5A and st[5] == 0


def test_kth_in_the_first_and_the_last_bin_of_round_one(gs, cuda, geom):
    """The k-th image's top byte 0x00 and 0xff; a picked bin that holds exactly krem elements."""
    T, S = geom
    cols, rows = S + T + 1, 2
    rng = np.random.default_rng(8)
    img = np.stack([images(rng, cols, 0x0100, 0xFF00) for _ in range(rows)])       # bins 1 .. 254
    low, high = rng.choice(cols, 3000, replace=False), rng.choice(cols, 2500, replace=False)
    m0, m1 = img.copy(), img.copy()
    m0[:, low] = images(rng, 3000, 0, 0x0100)                      # 3000 elements in bin 0
    m1[:, high] = images(rng, 2500, 0xFF00, 0x10000)               # 2500 elements in bin 255
    st = Case(gs, cuda, RN.keys_of(m0, U16), cols, U16, False).check(rows, 1500, ARGS, path=2)
    assert st[1] >> 8 == 0 and st[4] == 3000
    st = Case(gs, cuda, RN.keys_of(m1, F16), cols, F16, False).check(rows, cols - 1200, KEYS, path=2)
    assert st[1] >> 8 == 255 and st[4] == 2500
    st = Case(gs, cuda, RN.keys_of(m1, U16), cols, U16, True).check(rows, 1200, ARGS, path=2)     # descending: the same elements, image bin 0
    assert st[1] >> 8 == 0 and st[4] == 2500
    st = Case(gs, cuda, RN.keys_of(m0, BF16), cols, BF16, False).check(rows, 3000, PAIRS, path=2)  # the picked bin holds exactly krem elements
    assert st[1] >> 8 == 0 and st[4] == 3000 and st[2] + st[3] == 3000


def test_kth_in_the_first_and_the_last_bin_of_round_two_and_krem_one(gs, cuda, geom):
    """below images under 0x3F00, then a top byte 0x40 that holds 300 times 0x4000, 560 images in between and 40 times 0x40FF, the
    rest far above: the k-th image's low byte is 0x00 and 0xFF, the picked bin of round two holds exactly krem, and with one
    image alone in its top byte krem is 1 after round one."""
    T, S = geom
    cols, rows, below = 2 * S + 5, 2, 4096
    rng = np.random.default_rng(9)
    img = np.stack([images(rng, cols, 0x5000, 0x10000) for _ in range(rows)])
    for r in range(rows):
        at = rng.choice(cols, below + 900, replace=False)
        img[r, at[:below]] = images(rng, below, 0, 0x3F00)
        img[r, at[below:below + 300]] = 0x4000
        img[r, at[below + 300:below + 860]] = images(rng, 560, 0x4001, 0x40FF)
        img[r, at[below + 860:]] = 0x40FF
    for kt, desc in ((U16, False), (BF16, True)):
        c = Case(gs, cuda, RN.keys_of(img, kt, desc), cols, kt, desc)
        st = c.check(rows, below + 1, ARGS, path=2)                 # low byte 0x00, krem 1 in round two
        assert st[1] == 0x4000 and st[2] == below and st[3] == 1 and st[4] == 900
        st = c.check(rows, below + 300, PAIRS, path=2)              # bin 0x00 of round two holds exactly krem
        assert st[1] == 0x4000 and st[3] == 300
        st = c.check(rows, below + 861, KEYS, path=2)               # low byte 0xFF
        assert st[1] == 0x40FF and st[2] == below + 860 and st[3] == 1
        st = c.check(rows, below + 900, ARGS, path=2)               # both picked bins hold exactly krem
        assert st[1] == 0x40FF and st[3] == 40 and st[2] + st[3] == below + 900
    one = img.copy()
    for r in range(rows):
        top = np.nonzero(one[r] >> np.uint64(8) == 0x40)[0]
        one[r, top[1:]] = images(rng, top.size - 1, 0x5000, 0x10000)
        one[r, top[0]] = 0x40FF
    st = Case(gs, cuda, RN.keys_of(one, I16), cols, I16, False).check(rows, below + 1, ARGS, path=2)
    assert st == [2, 0x40FF, below, 1, 1, 0, 0, 0]                  # krem == 1 after round one, one element matches


def test_float_specials_and_i16_around_zero(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 9, 2
    rng = np.random.default_rng(10)
    for kt in (F16, BF16):
        sp = RN.specials16(kt)                                      # +-NaN with payloads, +-inf, +-0, subnormals
        mat = sp[rng.integers(0, sp.size, (rows, cols))]
        run = cols // sp.size
        for desc in (False, True):
            c = Case(gs, cuda, mat, cols, kt, desc)
            for i, k in enumerate((1, run, 4 * run + 1, cols // 2, cols - run, cols - 1)):     # cuts inside the NaN, inf and zero runs
                c.check(rows, k, MODES[i % 3], path=2)
        Case(gs, cuda, mat[:, :5000].copy(), 5000, kt, True).check(rows, 2500, PAIRS, path=1)
    ints = rng.integers(-40, 41, (rows, cols)).astype(np.int16).view(np.uint16)
    neg = int((ints[0].view(np.int16) < 0).sum())
    for desc in (False, True):
        c = Case(gs, cuda, ints, cols, I16, desc)
        for i, k in enumerate((neg - 1, neg, neg + 1, cols - neg)):
            c.check(rows, k, MODES[(i + 1) % 3], path=2)


# --------------------------------------------------------------------------------------------------------- ties --
def test_all_keys_equal_gives_the_first_columns(gs, cuda, geom):
    T, S = geom
    rows, cols, k = 2, 2 * S + 5, S + 3
    for kt, desc in ((U16, False), (BF16, True)):
        c = Case(gs, cuda, np.full((rows, cols), 0x3F80, np.uint16), cols, kt, desc)
        assert np.array_equal(c.expect(rows, k, ARGS)[1], np.tile(np.arange(k, dtype=np.uint32), (rows, 1)))
        for mode in MODES:
            st = c.check(rows, k, mode, path=2)
            assert st[2] == 0 and st[3] == k and st[4] == cols and st[5] == 0
    c = Case(gs, cuda, np.full((rows, 6000), 7, np.uint16), 6000, I16, True)
    c.check(rows, 3000, ARGS, path=1)


def test_tie_runs_across_a_tile_and_a_slab_boundary_with_the_cut_inside(gs, cuda, geom):
    """Ten smaller keys, then a run of equal keys that starts five columns before a boundary: the cut falls behind the boundary."""
    T, S = geom
    rows, cols = 2, S + 2 * T
    rng = np.random.default_rng(5)
    for edge in (T, S):
        mat = images(rng, rows * cols, 0x0400, 0x10000).astype(np.uint16).reshape(rows, cols)
        for r in range(rows):
            mat[r, edge - 5 - r:edge + 3000] = 1000
            mat[r, rng.choice(np.r_[0:edge - 30, edge + 3100:cols], 10, replace=False)] = np.arange(10, dtype=np.uint16)
        c = Case(gs, cuda, mat, cols, U16, False)
        for k in (10 + 3, 10 + 5, 10 + 6, 10 + 1500):
            ev = c.expect(rows, k, ARGS)[1]
            assert list(ev[0, 10:]) == list(range(edge - 5, edge - 5 + k - 10))
            for mode in (ARGS, PAIRS):
                st = c.check(rows, k, mode, path=2)
                assert st[1] == 1000 and st[2] == 10 and st[3] == k - 10
        Case(gs, cuda, ~mat, cols, U16, True).check(rows, 10 + 1500, ARGS, path=2)


def test_an_empty_before_group_and_a_take_of_one(gs, cuda, geom):
    T, S = geom
    rows, cols = 2, S + 100
    rng = np.random.default_rng(6)
    mat = images(rng, rows * cols, 0x0400, 0x10000).astype(np.uint16).reshape(rows, cols)
    mat[:, rng.choice(cols, 5000, replace=False)] = 77           # the minimum, 5000 times: less == 0 for k <= 5000
    c = Case(gs, cuda, mat, cols, U16, False)
    st = c.check(rows, 2000, ARGS, path=2)
    assert st[2] == 0 and st[3] == 2000
    assert cols <= 65536
    uniq = np.stack([rng.permutation(65536)[:cols].astype(np.uint16) for _ in range(rows)])     # distinct keys: take == 1
    for kt, desc in ((I16, False), (F16, True)):
        st = Case(gs, cuda, uniq, cols, kt, desc).check(rows, 2000, PAIRS, path=2)
        assert st[2] == 1999 and st[3] == 1


def test_a_row_longer_than_the_patterns_has_ties_by_force(gs, cuda, geom):
    rows, cols = 2, RN.LONG_COLS
    assert cols > 65536
    mat = RN.matrix16(rows, cols, BF16, seed=60, kinds=["uniform"])
    c = Case(gs, cuda, mat, cols, BF16, True)
    st = c.check(rows, 40000, ARGS, path=2)
    assert st[3] >= 1 and st[4] > 256 * 0.5
    c.check(rows, cols - 1, KEYS, path=2)
    Case(gs, cuda, mat, cols, U16, False).check(rows, 8193, PAIRS, path=2)


# -------------------------------------------------------------------------------- agreement with the other calls --
@pytest.mark.parametrize("rows,cols,path", RN.AGREE_SHAPES)
def test_agrees_with_topk_rows_u16_a_loop_of_topk_u16_and_the_widened_anyk_u32(gs, cuda, rows, cols, path):
    mat = RN.matrix16(rows, cols, BF16, seed=70, kinds=["uniform", "five", "zipf"])
    d_keys = dev16(mat, cuda)
    assert gs.DeviceTopKRowsAnyK16.Plan(rows, cols, 3000)[0] == path

    def outs(k, kdtype=torch.int16):
        return torch.empty(rows * k, dtype=kdtype, device=cuda), torch.empty(rows * k, dtype=torch.int32, device=cuda)

    def anyk(k):
        nb = gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko, vo = outs(k)
        assert anyk16(gs, temp.data_ptr(), nb, d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1, BF16) == 0
        return ko, vo
    for k in (64, 1024):
        nb = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(max(nb, 256), dtype=torch.uint8, device=cuda)
        ko, vo = outs(k)
        assert gs.lib.gs_topk_rows_u16(temp.data_ptr(), nb, d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                                       BF16, None) == 0
        ak, av = anyk(k)
        assert torch.equal(ak, ko) and torch.equal(av, vo)
    k = 3000
    nb = gs.lib.gs_topk_u16_temp_bytes(cols, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = outs(k)
    for r in range(rows):
        assert gs.lib.gs_topk_u16(temp.data_ptr(), nb, d_keys.data_ptr() + 2 * r * cols, None, ko.data_ptr() + 2 * r * k,
                                  vo.data_ptr() + 4 * r * k, cols, k, 1, BF16, None) == 0
    ak, av = anyk(k)
    assert torch.equal(ak, ko) and torch.equal(av, vo)
    k = 2000
    d_wide = dev32(RN.widen(mat), cuda)
    nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = outs(k, torch.int32)
    assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, d_wide.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                                        RN.WIDE[BF16], None) == 0
    ak, av = anyk(k)
    assert np.array_equal(host32(ko) >> np.uint32(16), host16(ak)) and (host32(ko) & 0xFFFF == 0).all() and torch.equal(av, vo)


# ------------------------------------------------------------------------------------------------- row stride --
@pytest.mark.parametrize("cols,k,path", RN.STRIDE_SHAPES)
def test_row_stride_with_a_gap_that_would_win(gs, cuda, cols, k, path):
    """row_stride = cols + 3 (odd or even: the row bases alternate between 2 and 0 mod 4); the gap holds 0x0000 and 0xFFFF, the
    extremes of the u16 order in both directions, and no key of the rows equals either.  None may appear in the output, and the
    input is unchanged after the call."""
    rows, stride = 5, cols + 3
    for desc in (False, True):
        mat = RN.matrix16(rows, cols, U16, seed=80, stride=stride, kinds=["uniform", "topbyte", "zipf"])
        mat[:, :cols] = np.clip(mat[:, :cols], 1, 0xFFFE)
        mat[:, cols:] = np.array([0, 0xFFFF, 0 if desc else 0xFFFF], np.uint16)
        mat[:, cols] = 0xFFFF if desc else 0
        c = Case(gs, cuda, mat, cols, U16, desc)
        before_k, before_v = c.d_keys.clone(), c.d_vals.clone()
        for mode in MODES:
            ek, ev = c.expect(rows, k, mode)
            assert not np.isin(ek, [0, 0xFFFF]).any() and (mode != ARGS or (ev < cols).all())
            c.check(rows, k, mode, path=path)
        assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


@pytest.mark.parametrize("rows,cols,k,path", [(3, 6001, 2001, 1), (2, RN.SLAB + 12, 3001, 2)])
def test_key_arrays_at_2_mod_4_and_an_odd_stride(gs, cuda, rows, cols, k, path):
    stride = cols + 2 if cols % 2 else cols + 3
    assert stride % 2 == 1 and k % 2 == 1
    mat = RN.matrix16(rows, cols, F16, seed=85, stride=stride, kinds=["uniform", "special"])
    span = (rows - 1) * stride + cols
    d_in = torch.zeros(span + 1, dtype=torch.int16, device=cuda)
    d_in[1:] = dev16(mat.reshape(-1)[:span], cuda)
    ko = torch.full((rows * k + 2,), -1, dtype=torch.int16, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, 1)
    assert gs.DeviceTopKRowsAnyK16.Plan(rows, cols, k, 1)[0] == path
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    kin, kout = d_in.data_ptr() + 2, ko.data_ptr() + 2
    assert kin % 4 == 2 and kout % 4 == 2
    assert anyk16(gs, temp.data_ptr(), nb, kin, None, kout, vo.data_ptr(), rows, cols, stride, k, True, F16) == 0
    ek, ev = RN.rows_topk16(mat, cols, k, F16, True)
    got = host16(ko)
    assert got[0] == 0xFFFF and got[-1] == 0xFFFF
    assert np.array_equal(got[1:-1].reshape(rows, k), ek) and np.array_equal(host32(vo).reshape(rows, k), ev)


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path", RN.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path):
    """Every array in a slot of its own between guard zones, the key arrays at 2 and 6 bytes from a 256-byte boundary, the value
    arrays at 12 and 20, the workspace at an odd one, outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = (U16, BF16, F16)[i], bool(i % 2)
        mat = RN.matrix16(rows, cols, kt, seed=90 + i, stride=stride)
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRowsAnyK16.Plan(rows, cols, k, hv)[0] == path
        a = Arena(cuda, seed=i)
        a.add("keys_in", 2 * span, offset=2, data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 2 * rows * k, offset=6, fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        rc = anyk16(gs, a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                    a.ptr("vals_out") if hv else None, rows, cols, stride, k, desc, kt)
        assert rc == 0
        a.check()
        ek, ev = RN.rows_topk16(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint16).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    rows, cols, k = 3, 9000, 2000
    nb = gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 2 * rows * cols, fill="random").add("vals_in", 4 * rows * cols, fill="random")
    a.add("keys_out", 2 * rows * k, fill="random").add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows,
                 cols=cols, stride=cols, k=k, kt=BF16)
        p.update(kw)
        return anyk16(gs, p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["rows"], p["cols"], p["stride"], p["k"], 0,
                      p["kt"])
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=cols + 1), dict(stride=cols - 1), dict(kt=0), dict(kt=2), dict(kt=5), dict(kt=12),
               dict(rows=1 << 18, stride=1 << 14), dict(rows=1 << 20, cols=2048, stride=2048, k=2048),
               dict(vin=a.ptr("vals_in"), vout=None), dict(kin=None), dict(kout=None),
               dict(kout=a.ptr("keys_in") + 4), dict(vout=a.ptr("keys_out") + 2 * (rows * k - 2)), dict(kin=a.ptr("keys_in") + 1),
               dict(kout=a.ptr("keys_out") + 1), dict(vout=a.ptr("vals_out") + 2), dict(vin=a.ptr("keys_in") + 2 * (rows * cols - 2))):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A pairs call on path 2, a keys call on path 1 and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, p2), (rows_b, cols_b, k_b, p1) = RN.REUSE_SHAPES
    assert (p2, p1) == (2, 1)
    a = Case(gs, cuda, RN.matrix16(rows, cols, BF16, seed=100), cols, BF16, True)
    b = Case(gs, cuda, RN.matrix16(rows_b, cols_b, I16, seed=101), cols_b, I16, False)
    nb = max(gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows_b, cols_b, k_b, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int16, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((rows_b * k_b,), -1, dtype=torch.int16, device=cuda)

    def run_a(ko, vo):
        assert anyk16(gs, temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                      BF16) == 0
    run_a(*outs[0])
    assert anyk16(gs, temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, rows_b, cols_b, cols_b, k_b, 0, I16) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host16(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host32(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host16(kb).reshape(rows_b, k_b), b.expect(rows_b, k_b, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path", RN.GRAPH_SHAPES)
def test_topk_rows_anyk16_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers."""
    sets = [RN.matrix16(rows, cols, U16, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "five"))]
    src = dev16(sets[0], cuda)
    ko = torch.full((rows * k,), -1, dtype=torch.int16, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    front = gs.DeviceTopKRowsAnyK16
    nb = front.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert front.Plan(rows, cols, k, True)[0] == path
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        front.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        front.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U16)
    for mat in sets:
        src.copy_(dev16(mat, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = RN.rows_topk16(mat, cols, k, U16, True)
        assert np.array_equal(host16(ko).reshape(rows, k), ek) and np.array_equal(host32(vo).reshape(rows, k), ev)
        assert front.Status(temp, rows, cols, k, True, rows - 1) == RN.status(mat[rows - 1], k, U16, True)


# ------------------------------------------------------------------------------------------------- front ends --
def _distinct_bf16(rows, cols, seed, cuda):
    """Tie-free, NaN-free bfloat16 rows: distinct finite bit patterns (no infinities, one zero)."""
    rng = np.random.default_rng(seed)
    pats = np.concatenate([np.arange(0x0000, 0x7F80), np.arange(0x8001, 0xFF80)]).astype(np.uint16)
    assert cols <= pats.size
    mat = np.stack([rng.permutation(pats)[:cols] for _ in range(rows)])
    return torch.from_numpy(mat.view(np.int16).copy()).to(cuda).view(torch.bfloat16)


@pytest.mark.parametrize("rows,cols,k", [(4, 5000, 1500), (3, 40000, 3000)])
def test_topk_rows_anyk16_against_torch_topk(gs, cuda, rows, cols, k):
    wide = _distinct_bf16(rows, cols + 40, cols, cuda)
    for x in (wide[:, :cols].contiguous(), wide[:, 17:17 + cols]):        # the second: a column slice at an odd element offset
        for largest in (False, True):
            want = torch.topk(x.float(), k, dim=1, largest=largest, sorted=True)      # (exact: float32 holds every bfloat16)
            ko, io = gs.topk_rows_anyk16(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == torch.bfloat16 and io.dtype == torch.int32
            assert torch.equal(ko.float(), want.values) and torch.equal(io.long(), want.indices)
            k2, none = gs.topk_rows_anyk16(x, k, largest=largest)
            assert none is None and torch.equal(k2, ko)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows_anyk16(x, k, largest=True, values=v)
    want = torch.topk(x.float(), k, dim=1, largest=True)
    assert torch.equal(ko.float(), want.values) and torch.equal(vo, torch.gather(v, 1, want.indices))
    for other in (x.view(torch.int16), x.view(torch.float16)):           # the other dtypes come back as they went in
        ko, _ = gs.topk_rows_anyk16(other, k)
        assert ko.dtype == other.dtype and tuple(ko.shape) == (rows, k)
    ko, vo = gs.topk_rows_anyk16(x, 0, indices=True)
    assert tuple(ko.shape) == (rows, 0) and tuple(vo.shape) == (rows, 0)
    ko, vo = gs.topk_rows_anyk16(x[:0], k, indices=True)
    assert tuple(ko.shape) == (0, k) and tuple(vo.shape) == (0, k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk16(x.float(), k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(x, k)
    with pytest.raises(ValueError):
        gs.topk_rows(x, k)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_anyk_narrow_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 6 * 3 * 4
