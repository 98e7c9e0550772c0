"""gs_topk_rows_anyk_u64 on the device: every row bit for bit against tests/topk_rows_anyk_wide_ref.py (keys, values or columns)
and the status words of up to eight rows per call against the host model of the descent, over the shapes of both paths read from
the plan, every depth D = 1 .. 6 of the descent and both of its ends, lists of exactly 1, L and L + 1, the bin edges of round one,
outliers that alone make a high bit vary, small integers, timestamps, the pad image, tie runs across a tile and a slab boundary,
NaNs and +-0, agreement with gs_topk_rows_u64, gs_topk_u64, gs_topk_rows_anyk_u32 on the widened matrix and torch.topk, a row
stride with a gap that would win, guarded, offset and dirty buffers, refused calls, workspace reuse, identical bytes, graph
capture, a seeded campaign, the Python front end and the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_rows_anyk_wide_ref as RA
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, I64, F64 = RA.KEY_TYPES
KEYS, PAIRS, ARGS, MODES = RA.KEYS, RA.PAIRS, RA.ARGS, RA.MODES
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written


@pytest.fixture(scope="module")
def geom(gs):
    """(T, S): the tile and the slab in columns, read from the plan; the shape tables of the reference module assume them."""
    p = gs.DeviceTopKRowsAnyK64.Plan(1, 1 << 20, 5000)
    assert p == RA.plan(1, 1 << 20, 5000) and p[0] == 2 and p[1] == 19 and p[2] == RA.CH and p[3] == RA.TILE and p[3] * p[4] == RA.SLAB
    assert gs.DeviceTopKRowsAnyK64.Plan(1, RA.DEEP_COLS, 5)[7] == 3072
    return p[3], p[3] * p[4]


# ------------------------------------------------------------------------------------------------------- inputs --
def values_for(shape, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def dev64(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(cuda)


def dev32(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def status_of(gs, temp, rows, cols, k, hv, row):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_rows_anyk_u64_status(temp.data_ptr(), rows, cols, k, hv, row, out, None) == 0
    return list(out)


def anyk64(gs, temp, nb, kin, vin, kout, vout, rows, cols, stride, k, desc, kt):
    return gs.lib.gs_topk_rows_anyk_u64(temp, nb, kin, vin, kout, vout, rows, cols, stride, k, int(desc), kt, None)


class Case:
    """One matrix of uint64 bit patterns on the device with its reference (one stable argsort per row, computed once);
    .check(rows, k, mode) runs the C entry point on the first `rows` rows and compares every row and, for up to eight rows,
    every status word.  Returns the status of row 0."""

    def __init__(self, gs, cuda, mat, cols, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride = np.ascontiguousarray(mat, dtype=np.uint64), mat.shape[1]
        self.vals = values_for(mat.shape)
        self.d_keys, self.d_vals = dev64(self.mat, cuda), dev32(self.vals, cuda)
        self.order = RA.rows_order(self.mat, cols, kt, desc)

    def expect(self, rows, k, mode):
        return RA.rows_topk64(self.mat[:rows], self.cols, k, self.kt, self.desc, self.vals[:rows] if mode == PAIRS else None,
                              order=self.order[:rows])

    def check(self, rows, k, mode, path=None):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc)
        if path is not None:
            assert gs.DeviceTopKRowsAnyK64.Plan(rows, cols, k, hv)[0] == path, what
        nb = gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((rows * k + TAIL,), -1, dtype=torch.int64, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = anyk64(gs, temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                    vo.data_ptr() if hv else None, rows, cols, self.stride, k, self.desc, self.kt)
        assert rc == 0, (rc, what)
        ek, ev = self.expect(rows, k, mode)
        gk, gv = host64(ko), host32(vo)
        bad = np.nonzero((gk[:rows * k].reshape(rows, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of rows", bad[:8])
        assert (gk[rows * k:] == RA.ONES).all(), what
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
    return RA.KEY_TYPES[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def test_the_rotation_reaches_every_type_direction_and_form():
    seen = {rotate(i) for i in range(18)}
    assert {s[0] for s in seen} == set(RA.KEY_TYPES) and {s[1] for s in seen} == {False, True} and {s[2] for s in seen} == set(MODES)


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RA.PATH1_COLS)
def test_path1_one_workgroup_per_row(gs, cuda, cols):
    ci = RA.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RA.path1_ks(cols)):
        for i, rows in enumerate(RA.PATH1_ROWS):
            kt, desc, mode = rotate(5 * ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, RA.matrix64(max(RA.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
            st = cases[(kt, desc)].check(rows, k, mode, path=1)
            assert st[5:] == [0, 0, 0]


def test_path1_every_type_direction_and_form(gs, cuda):
    cols, rows, k = 5000, 3, 1500
    for kt in RA.KEY_TYPES:
        for desc in (False, True):
            c = Case(gs, cuda, RA.matrix64(rows, cols, kt, seed=30 + kt, kinds=["uniform", "special", "small"]), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=1)


# ------------------------------------------------------------------------------------------------------- path 2 --
@pytest.mark.parametrize("cols", RA.PATH2_COLS)
def test_path2_descent_over_all_rows(gs, cuda, geom, cols):
    ci = RA.PATH2_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RA.path2_ks(cols)):
        for i, rows in enumerate(RA.PATH2_ROWS):
            kt, desc, mode = rotate(ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, RA.matrix64(max(RA.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, path=2)


def test_path2_every_type_direction_and_form(gs, cuda, geom):
    T, S = geom
    cols, rows, k = S + T + 3, 2, 3000
    for kt in RA.KEY_TYPES:
        for desc in (False, True):
            c = Case(gs, cuda, RA.matrix64(rows, cols, kt, seed=40 + kt, kinds=["uniform", "normal", "special"]), cols, kt, desc)
            for mode in MODES:
                c.check(rows, k, mode, path=2)


def test_path2_many_rows_of_one_slab(gs, cuda, geom):
    rows, cols, k = RA.MANY_ROWS
    p = gs.DeviceTopKRowsAnyK64.Plan(rows, cols, k)
    assert p[0] == 2 and p[5] == 1
    c = Case(gs, cuda, RA.matrix64(rows, cols, F64, seed=50), cols, F64, True)
    c.check(rows, k, ARGS, path=2)
    c.check(rows, k, KEYS, path=2)


# --------------------------------------------------------------------------------------------------- the descent --
def test_every_depth_in_one_call_and_both_ends(gs, cuda, geom):
    """Rows of D = 1 .. 6 in one call (six rounds at L = 3072), a tie run decided by v == 0 and one by s == 0 among them."""
    cols = RA.DEEP_COLS
    built = [RA.depth_row(cols, d, seed=d) for d in range(1, 7)]
    k = built[5][1]
    assert all(b[1] >= k for b in built[1:])           # one k for all rows: inside every core
    tie = RA.tie_run_row(cols, RA.TILE - 2000, 4000, seed=9)
    img = np.stack([b[0] for b in built] + [tie[0]])
    for kt, desc, mode in ((U64, False, ARGS), (F64, True, PAIRS), (I64, False, KEYS)):
        c = Case(gs, cuda, RA.keys_of(img, kt, desc), cols, kt, desc)
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_anyk_u64_temp_bytes(7, cols, k, hv)
        c.check(7, k, mode, path=2)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.empty(7 * k, dtype=torch.int64, device=cuda)
        vo = torch.empty(7 * k, dtype=torch.int32, device=cuda)
        assert anyk64(gs, temp.data_ptr(), nb, c.d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr() if hv else None, 7, cols, cols, k,
                      desc, kt) == 0
        sts = [status_of(gs, temp, 7, cols, k, hv, r) for r in range(7)]
        assert [s[5] for s in sts[:6]] == [1, 2, 3, 4, 5, 6]
        assert [s[6] for s in sts[:6]] == [1, 1, 1, 1, 1, 2] and sts[5][7] == 0     # D = 6 ends at shift 0: a tie run
    c = Case(gs, cuda, RA.keys_of(img[6:], U64), cols, U64, False)
    st = c.check(1, tie[1], ARGS, path=2)
    assert st[5] == 2 and st[6] == 2 and st[3] == tie[2] and st[4] == tie[1] - tie[2]      # v == 0 in round two


def test_a_list_of_exactly_one_of_l_and_of_l_plus_one(gs, cuda, geom):
    T, S = geom
    cols = S + 5
    L = RA.list_cap(cols)
    for c_n, want in ((L, (1, 1, L)), (L + 1, (2, 1, None))):
        img, k = RA.bucket_row(cols, c_n, seed=c_n)
        st = Case(gs, cuda, RA.keys_of(img[None, :], I64), cols, I64, False).check(1, k, ARGS, path=2)
        assert (st[5], st[6]) == want[:2] and (want[2] is None or st[7] == want[2])
        assert want[2] is not None or 0 < st[7] < L
    img, k = RA.single_row(cols, seed=2)
    st = Case(gs, cuda, RA.keys_of(img[None, :], F64, True), cols, F64, True).check(1, k, PAIRS, path=2)
    assert st[3:] == [k - 1, 1, 1, 1, 1]                 # krem == 1, take == 1, a list of one


def test_kth_in_the_first_and_the_last_bin_of_round_one_and_less_zero(gs, cuda, geom):
    T, S = geom
    cols, rows = S + T + 1, 2
    rng = np.random.default_rng(8)
    img = np.stack([RA.uniform_images(rng, cols) for _ in range(rows)])
    img = (img >> np.uint64(1)) | np.uint64(1 << 62)            # top digits 1024 .. 1535
    lo, hi = img.copy(), img.copy()
    at = rng.choice(cols, 3000, replace=False)
    lo[:, at] = RA.uniform_images(rng, 3000) >> np.uint64(RA.DIGIT)          # 3000 images in bin 0
    hi[:, at] = RA.uniform_images(rng, 3000) | np.uint64(2047 << 53)         # 3000 images in bin 2047
    st = Case(gs, cuda, RA.keys_of(lo, U64), cols, U64, False).check(rows, 1500, ARGS, path=2)
    assert st[2] >> 21 == 0 and st[5:] == [1, 1, 3000]
    st = Case(gs, cuda, RA.keys_of(hi, F64), cols, F64, False).check(rows, cols - 1200, KEYS, path=2)
    assert st[2] >> 21 == 2047 and st[5:] == [1, 1, 3000]
    st = Case(gs, cuda, RA.keys_of(lo, I64), cols, I64, False).check(rows, 1, PAIRS, path=2)       # the minimum: less == 0, take == 1
    assert st[3:5] == [0, 1]
    mins = hi.copy()
    mins[:, at] = np.uint64(77)                                  # the minimum 3000 times, all of bin 0: less == 0, a list of one image
    st = Case(gs, cuda, RA.keys_of(mins, U64), cols, U64, False).check(rows, 2000, ARGS, path=2)
    assert st[1:5] == [77, 0, 0, 2000] and st[5:] == [1, 1, 3000]


def test_one_outlier_makes_a_high_bit_vary(gs, cuda, geom):
    T, S = geom
    cols = S + 100
    plain = RA.status(RA.RW.small_int_rows(1, cols, 5)[0], 2000, I64)
    assert plain[5] == 2                                         # without the outlier: round one learns AND / OR only
    for at in RA.outlier_positions(cols):
        keys = RA.outlier_row(cols, at, seed=4)
        for desc, mode in ((False, ARGS), (True, KEYS)):
            st = Case(gs, cuda, keys[None, :], cols, I64, desc).check(1, 2000, mode, path=2)
            assert st[5] == 3 and st[6] == 1


def test_small_integers_timestamps_pads_and_one_key(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 77, 2
    st = Case(gs, cuda, RA.RW.small_int_rows(rows, cols, 1), cols, I64, False).check(rows, 3000, ARGS, path=2)
    assert st[5] == 2 and st[6] == 1
    st = Case(gs, cuda, RA.RW.timestamp_rows(rows, cols, 2), cols, I64, True).check(rows, 3000, PAIRS, path=2)
    assert st[5] == 2
    pads = RA.RW.pad_image_rows(3, cols, 40, seed=3)             # all ones but for 40 per row; the last row nothing else
    c = Case(gs, cuda, RA.keys_of(pads, U64), cols, U64, False)
    c.check(3, 30, KEYS, path=2)
    st = c.check(3, 5000, ARGS, path=2)
    assert st[1:3] == [0xFFFFFFFF, 0xFFFFFFFF] and st[3] == 40
    one = RA.RW.one_key_rows(rows, cols)
    for kt, desc in ((U64, False), (F64, True)):
        st = Case(gs, cuda, RA.keys_of(one, kt, desc), cols, kt, desc).check(rows, 2500, ARGS, path=2)
        assert st[3:] == [0, 2500, 1, 2, 0]                      # a row of one key: one round, a tie run
    for b in (11, 30, 53):
        img = np.stack([RA.shared_top_row(cols, b, seed=b + r) for r in range(rows)])
        Case(gs, cuda, RA.keys_of(img, U64), cols, U64, False).check(rows, 2222, PAIRS, path=2)


def test_tie_runs_across_a_tile_and_a_slab_boundary(gs, cuda, geom):
    T, S = geom
    cols = S + T + 1
    L = RA.list_cap(cols)
    for start, length in ((T - 3000, L + 900), (S - 3000, L + 900), (S - 100, L + 1)):
        assert length > L and start < (start + length - 1) // T * T
        img, k, below = RA.tie_run_row(cols, start, length, seed=start)
        for kt, desc, mode in ((U64, False, ARGS), (F64, True, PAIRS)):
            c = Case(gs, cuda, RA.keys_of(img[None, :], kt, desc), cols, kt, desc)
            st = c.check(1, k, mode, path=2)
            assert st[3] == below and st[4] == k - below and st[6] == 2
            c.check(1, below + 1, mode, path=2)
            c.check(1, below + length, mode, path=2)


def test_nans_zeros_and_i64_around_zero(gs, cuda, geom):
    T, S = geom
    cols, rows = S + 9, 2
    mat = RA.specials_matrix(rows, cols, F64, seed=10)
    run = cols // 13
    for desc in (False, True):
        c = Case(gs, cuda, mat, cols, F64, desc)
        for i, k in enumerate((1, run, 4 * run + 1, cols // 2, cols - run, cols - 1)):
            c.check(rows, k, MODES[i % 3], path=2)
    Case(gs, cuda, mat[:, :5000].copy(), 5000, F64, True).check(rows, 2500, PAIRS, path=1)
    ints = RA.around_zero(rows, cols, seed=11)
    neg = int((ints[0].view(np.int64) < 0).sum())
    c = Case(gs, cuda, ints, cols, I64, False)
    for i, k in enumerate((neg, neg + 1, cols // 2, 1025)):
        c.check(rows, k, MODES[i % 3], path=2)
    Case(gs, cuda, ints, cols, I64, True).check(rows, 3000, ARGS, path=2)


# -------------------------------------------------------------------------------- agreement with the other calls --
@pytest.mark.parametrize("rows,cols,path", RA.AGREE_SHAPES)
def test_agrees_with_topk_rows_u64_a_loop_of_topk_u64_and_the_widened_anyk_u32(gs, cuda, rows, cols, path):
    mat = RA.matrix64(rows, cols, F64, seed=70, kinds=["uniform", "five", "normal"])
    d_keys = dev64(mat, cuda)
    assert gs.DeviceTopKRowsAnyK64.Plan(rows, cols, 3000)[0] == path

    def outs(k, kdtype=torch.int64):
        return torch.empty(rows * k, dtype=kdtype, device=cuda), torch.empty(rows * k, dtype=torch.int32, device=cuda)

    def anyk(k, src=d_keys, kt=F64):
        nb = gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko, vo = outs(k)
        assert anyk64(gs, temp.data_ptr(), nb, src.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1, kt) == 0
        return ko, vo
    for k in (64, 1024):
        nb = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1)
        temp = torch.empty(max(nb, 256), dtype=torch.uint8, device=cuda)
        ko, vo = outs(k)
        assert gs.lib.gs_topk_rows_u64(temp.data_ptr(), nb, d_keys.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                                       F64, None) == 0
        ak, av = anyk(k)
        assert torch.equal(ak, ko) and torch.equal(av, vo)
    k = 3000
    nb = gs.lib.gs_topk_u64_temp_bytes(cols, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = outs(k)
    for r in range(rows):
        assert gs.lib.gs_topk_u64(temp.data_ptr(), nb, d_keys.data_ptr() + 8 * r * cols, None, ko.data_ptr() + 8 * r * k,
                                  vo.data_ptr() + 4 * r * k, cols, k, 1, F64, None) == 0
    ak, av = anyk(k)
    assert torch.equal(ak, ko) and torch.equal(av, vo)
    k = 2000
    narrow = np.random.default_rng(71).standard_normal((rows, cols)).astype(np.float32).view(np.uint32)
    d_narrow = dev32(narrow, cuda)
    nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 1)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ko, vo = outs(k, torch.int32)
    assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, d_narrow.data_ptr(), None, ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                                        gs.GS_KEY_F32, None) == 0
    ak, av = anyk(k, dev64(RA.widen32(narrow), cuda), F64)
    got = host64(ak)
    assert np.array_equal((got >> np.uint64(32)).astype(np.uint32), host32(ko)) and (got & np.uint64(0xFFFFFFFF) == 0).all()
    assert torch.equal(av, vo)


# ------------------------------------------------------------------------------------------------- row stride --
@pytest.mark.parametrize("cols,k,path", RA.STRIDE_SHAPES)
def test_row_stride_with_a_gap_that_would_win(gs, cuda, cols, k, path):
    """row_stride = cols + 3; the gap holds 0 and all ones, the extremes of the u64 order in both directions, and no key of the
    rows equals either.  None may appear in the output, and the input is unchanged after the call."""
    rows, stride = 5, cols + 3
    for desc in (False, True):
        mat = RA.matrix64(rows, cols, U64, seed=80, stride=stride, kinds=["uniform", "small", "normal"])
        mat[:, :cols] = np.clip(mat[:, :cols], np.uint64(1), RA.ONES - np.uint64(1))
        mat[:, cols:] = np.array([0, RA.ONES, 0 if desc else RA.ONES], np.uint64)
        mat[:, cols] = RA.ONES if desc else 0
        c = Case(gs, cuda, mat, cols, U64, desc)
        before_k, before_v = c.d_keys.clone(), c.d_vals.clone()
        for mode in MODES:
            ek, ev = c.expect(rows, k, mode)
            assert not np.isin(ek, [0, RA.ONES]).any() and (mode != ARGS or (ev < cols).all())
            c.check(rows, k, mode, path=path)
        assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path", RA.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path):
    """Every array in a slot of its own between guard zones, the key arrays at 8 and 24 bytes from a 256-byte boundary, the value
    arrays at 12 and 20, the workspace at an odd one, outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = RA.KEY_TYPES[i], bool(i % 2)
        mat = RA.matrix64(rows, cols, kt, seed=90 + i, stride=stride)
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRowsAnyK64.Plan(rows, cols, k, hv)[0] == path
        a = Arena(cuda, seed=i)
        a.add("keys_in", 8 * span, offset=8, data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 8 * rows * k, offset=24, fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        rc = anyk64(gs, a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                    a.ptr("vals_out") if hv else None, rows, cols, stride, k, desc, kt)
        assert rc == 0
        a.check()
        ek, ev = RA.rows_topk64(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint64).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    rows, cols, k = 3, 9000, 2000
    nb = gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 8 * rows * cols, fill="random").add("vals_in", 4 * rows * cols, fill="random")
    a.add("keys_out", 8 * rows * k, fill="random").add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows,
                 cols=cols, stride=cols, k=k, kt=F64)
        p.update(kw)
        return anyk64(gs, p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["rows"], p["cols"], p["stride"], p["k"], 0,
                      p["kt"])
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=cols + 1), dict(stride=cols - 1), dict(kt=0), dict(kt=2), dict(kt=6), dict(kt=9),
               dict(rows=1 << 18, stride=1 << 14), dict(rows=1 << 20, cols=2048, stride=2048, k=2048),
               dict(vin=a.ptr("vals_in"), vout=None), dict(kin=None), dict(kout=None),
               dict(kout=a.ptr("keys_in") + 8), dict(vout=a.ptr("keys_out") + 8 * (rows * k - 1)), dict(kin=a.ptr("keys_in") + 4),
               dict(kout=a.ptr("keys_out") + 4), dict(vout=a.ptr("vals_out") + 2), dict(vin=a.ptr("keys_in") + 8 * (rows * cols - 1))):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A pairs call on path 2, a keys call on path 1 and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, p2), (rows_b, cols_b, k_b, p1) = RA.REUSE_SHAPES
    assert (p2, p1) == (2, 1)
    a = Case(gs, cuda, RA.matrix64(rows, cols, F64, seed=100), cols, F64, True)
    b = Case(gs, cuda, RA.matrix64(rows_b, cols_b, I64, seed=101), cols_b, I64, False)
    nb = max(gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows_b, cols_b, k_b, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int64, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((rows_b * k_b,), -1, dtype=torch.int64, device=cuda)

    def run_a(ko, vo):
        assert anyk64(gs, temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), rows, cols, cols, k, 1,
                      F64) == 0
    run_a(*outs[0])
    assert anyk64(gs, temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, rows_b, cols_b, cols_b, k_b, 0, I64) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host64(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host32(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host64(kb).reshape(rows_b, k_b), b.expect(rows_b, k_b, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path", RA.GRAPH_SHAPES)
def test_topk_rows_anyk64_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers: rows of other
    depths and ends run through the same launches."""
    sets = [RA.matrix64(rows, cols, U64, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "small", "five"))]
    src = dev64(sets[0], cuda)
    ko = torch.full((rows * k,), -1, dtype=torch.int64, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    front = gs.DeviceTopKRowsAnyK64
    nb = front.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert front.Plan(rows, cols, k, True)[0] == path
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        front.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U64)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        front.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U64)
    for mat in sets:
        src.copy_(dev64(mat, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = RA.rows_topk64(mat, cols, k, U64, True)
        assert np.array_equal(host64(ko).reshape(rows, k), ek) and np.array_equal(host32(vo).reshape(rows, k), ev)
        assert front.Status(temp, rows, cols, k, True, rows - 1) == RA.status(mat[rows - 1], k, U64, True)


def test_a_small_seeded_campaign(gs, cuda, geom):
    rng = np.random.default_rng(2024)
    for i in range(10):
        kt, desc, mode = rotate(int(rng.integers(0, 18)))
        rows = int(rng.integers(1, 6))
        cols = int(rng.integers(1100, 8193)) if i % 2 == 0 else int(rng.integers(8193, 3 * RA.SLAB))
        k = int(rng.integers(1, cols + 1))
        stride = cols + int(rng.integers(0, 5))
        kinds = [RA.RW.W.DISTS[int(j)] for j in rng.integers(0, len(RA.RW.W.DISTS), 3)]
        mat = RA.matrix64(rows, cols, kt, seed=200 + i, stride=stride, kinds=kinds)
        Case(gs, cuda, mat, cols, kt, desc).check(rows, k, mode)


# ------------------------------------------------------------------------------------------------- front ends --
@pytest.mark.parametrize("rows,cols,k", [(4, 5000, 1500), (3, 40000, 3000)])
def test_topk_rows_anyk64_against_torch_topk(gs, cuda, rows, cols, k):
    g = torch.Generator(device="cpu").manual_seed(cols)
    wide = torch.randn(rows, cols + 40, generator=g, dtype=torch.float64)
    assert all(torch.unique(wide[r]).numel() == cols + 40 for r in range(rows))       # distinct doubles
    wide = wide.to(cuda)
    for x in (wide[:, :cols].contiguous(), wide[:, 17:17 + cols]):        # the second: a column slice at an odd element offset
        for largest in (False, True):
            want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
            ko, io = gs.topk_rows_anyk64(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == torch.float64 and io.dtype == torch.int32
            assert torch.equal(ko, want.values) and torch.equal(io.long(), want.indices)
            k2, none = gs.topk_rows_anyk64(x, k, largest=largest)
            assert none is None and torch.equal(k2, ko)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows_anyk64(x, k, largest=True, values=v)
    want = torch.topk(x, k, dim=1, largest=True)
    assert torch.equal(ko, want.values) and torch.equal(vo, torch.gather(v, 1, want.indices))
    ints = x.view(torch.int64)
    ko, io = gs.topk_rows_anyk64(ints, k, indices=True)
    want = torch.sort(ints, dim=1, stable=True)
    assert ko.dtype == torch.int64 and torch.equal(ko, want.values[:, :k]) and torch.equal(io.long(), want.indices[:, :k])
    ko, vo = gs.topk_rows_anyk64(x, 0, indices=True)
    assert tuple(ko.shape) == (rows, 0) and tuple(vo.shape) == (rows, 0)
    ko, vo = gs.topk_rows_anyk64(x[:0], k, indices=True)
    assert tuple(ko.shape) == (0, k) and tuple(vo.shape) == (0, k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk64(x.float(), k)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(x, k)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_anyk_wide_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 3 * (5 * 3 * 2 + 1) * 3
