"""gs_topk_rows_u64 on the device: every row bit for bit against tests/topk_rows_wide_ref.py (keys, values or columns), over the
shapes of the three paths, k values, row counts, distributions mixed across the rows of one call, directions, forms and the
three key types; the edges the byte skip brings (exactly one varying byte, rows of one key, one outlier that alone makes a
byte vary, rows and chunks with different constant bytes, small integers, timestamps), rows of the pad image, ties across
every chunk of a long row, NaNs of both signs; strides; guarded, offset and dirty buffers; refusals; workspace reuse; graph
capture; the widen identity against gs_topk_rows_u32; the Python front ends and the C++ driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_ref as R
import topk_rows_ref as RR
import topk_rows_wide_ref as N
from guarded import Arena
from topk_cases import gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, I64, F64 = N.U64, N.I64, N.F64
KEYS, PAIRS, ARGS = N.KEYS, N.PAIRS, N.ARGS
MODES = N.MODES
CH = RR.CH
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


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


class Case:
    """One matrix on the device with its reference; .check(rows, k, mode) runs the C entry point on the first `rows` rows and
    compares every row."""

    def __init__(self, gs, cuda, mat, cols, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride = N.u64(mat), mat.shape[1]
        self.vals = values_for(mat.shape)
        self.d_keys = dev64(self.mat, cuda)
        self.d_vals = dev32(self.vals, cuda)
        self.order = N.rows_order(self.mat, cols, kt, desc)          # computed once, shared by every k, row count and form

    def expect(self, rows, k, mode):
        return N.rows_topk64(self.mat[:rows], self.cols, k, self.kt, self.desc, self.vals[:rows] if mode == PAIRS else None,
                             order=self.order[:rows])

    def check(self, rows, k, mode, plan=None):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc)
        if plan is not None:
            assert gs.DeviceTopKRows64.Plan(rows, cols, k, hv)[:2] == list(plan), what
        nb = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((rows * k + TAIL,), -1, dtype=torch.int64, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_rows_u64(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                     ko.data_ptr(), vo.data_ptr() if hv else None, rows, cols, self.stride, k, int(self.desc), self.kt,
                                     None)
        assert rc == 0, (rc, what)
        ek, ev = self.expect(rows, k, mode)
        gk, gv = host64(ko), host32(vo)
        bad = np.nonzero((gk[:rows * k].reshape(rows, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of rows", bad[:8])
        assert gk[rows * k:].size == TAIL and (gk[rows * k:] == ONES).all(), what
        if hv:
            bad = np.nonzero((gv[:rows * k].reshape(rows, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of rows", bad[:8])
            assert (gv[rows * k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        return ek, ev


def rotate(i):
    return N.KEY_TYPES[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def image_case(gs, cuda, img, kt, desc):
    """A case from images: the keys are their preimages, so the images on the device are exactly these."""
    img = np.ascontiguousarray(img, dtype=np.uint64)
    mat = N.preimage(img, kt, desc).reshape(img.shape)
    assert (N.image(mat, kt, desc).reshape(img.shape) == img).all()
    return Case(gs, cuda, mat, img.shape[1], kt, desc)


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RR.PATH1_COLS)
def test_path1_one_wave_per_row(gs, cuda, cols):
    """Every k and row count of the list; 1000 rows cover four rows per workgroup and (with 1, 3, 5) a ragged last one.  The
    distributions are mixed across the rows (so the waves of a workgroup skip different passes); form, key type and direction
    rotate."""
    ci = RR.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RR.path1_ks(cols)):
        for i, rows in enumerate(RR.PATH1_ROWS):
            kt, desc, mode = rotate(ci + 3 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, N.matrix64(max(RR.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, plan=(1, 1))


# ------------------------------------------------------------------------------------------------------- path 2 --
@pytest.mark.parametrize("cols", RR.PATH2_COLS)
def test_path2_one_workgroup_per_row(gs, cuda, cols):
    ci = RR.PATH2_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RR.PATH2_KS):
        for i, rows in enumerate(RR.PATH2_ROWS):
            kt, desc, mode = rotate(ci + 3 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, N.matrix64(max(RR.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, plan=(2, 1))


# ------------------------------------------------------------------------------------------------------- path 3 --
@pytest.mark.parametrize("shape", RR.PATH3_SHAPES)
def test_path3_chunked(gs, cuda, shape):
    rows, cols, k, levels = shape
    si = RR.PATH3_SHAPES.index(shape)
    for i in range(3):
        kt, desc, _ = rotate(si + 4 * i)
        c = Case(gs, cuda, N.matrix64(rows, cols, kt, seed=60 + si), cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


@pytest.mark.parametrize("shape", RR.MIDDLE_SHAPES)
def test_path3_middle_level_in_every_class_of_the_finishing_wave(gs, cuda, shape):
    """Three levels at k = 64, 256 and 512: the middle level reads 64-bit candidate keys with their columns and writes a
    candidate row again, with a finishing wave of 1, 4 and 8 per lane (PATH3_SHAPES has three levels at k = 1024 alone)."""
    rows, cols, k, levels = shape
    kt, desc, _ = rotate(2 + 4 * RR.MIDDLE_SHAPES.index(shape))
    c = Case(gs, cuda, N.matrix64(rows, cols, kt, seed=80 + k, kinds=["five", "uniform", "special"]), cols, kt, desc)
    for mode in MODES:
        c.check(rows, k, mode, plan=(3, levels))


# ------------------------------------------------------------------------------------------------ the byte skip --
EDGE_SHAPES = [(5, 700, 100, 1, 1), (3, 5000, 1000, 2, 1), (2, 2 * CH + 9, 1024, 3, 2)]     # (rows, cols, k, path, levels)


@pytest.mark.parametrize("rows,cols,k,path,levels", EDGE_SHAPES)
def test_rows_in_which_exactly_one_byte_varies(gs, cuda, rows, cols, k, path, levels):
    """For each of the eight byte positions: seven passes of the wave sort and seven rounds of the select are left out."""
    for b in range(8):
        kt, desc, mode = rotate(b)
        c = image_case(gs, cuda, N.one_byte_rows(rows, cols, b, seed=200 + b), kt, desc)
        c.check(rows, k, mode, plan=(path, levels))
        c.check(rows, k, ARGS)


@pytest.mark.parametrize("rows,cols,k,path,levels", EDGE_SHAPES)
def test_rows_of_one_key_give_the_first_k_columns(gs, cuda, rows, cols, k, path, levels):
    """No pass and no round runs: less = 0 and the tie run is cut at k."""
    for i, (kt, desc) in enumerate(((U64, False), (I64, True), (F64, True), (F64, False))):
        c = image_case(gs, cuda, N.one_key_rows(rows, cols, N.BASE if i < 3 else ONES), kt, desc)
        for mode in MODES:
            ek, ev = c.check(rows, k, mode, plan=(path, levels))
        assert np.array_equal(ev, np.tile(np.arange(k, dtype=np.uint32), (rows, 1)))


@pytest.mark.parametrize("rows,cols,k,path,levels", EDGE_SHAPES)
def test_one_outlier_alone_makes_a_byte_vary(gs, cuda, rows, cols, k, path, levels):
    """The outlier at the first column, at the last column and in the last, partly filled register (or thread slot): a
    reduction that misses it would skip a byte that decides where it goes."""
    places = [0, cols - 1, (cols - 1) // 64 * 64, cols // 2]
    for i, at in enumerate(places):
        for b in (7, 3, 1):
            kt, desc, mode = rotate(i + b)
            c = image_case(gs, cuda, N.outlier_rows(rows, cols, b, at, seed=220 + i), kt, desc)
            c.check(rows, k, mode, plan=(path, levels))
            c.check(rows, min(cols, 3), ARGS)


@pytest.mark.parametrize("cols,k", [(64, 9), (700, 100), (1024, 1024)])
def test_waves_of_one_workgroup_take_different_pass_sets(gs, cuda, cols, k):
    """One path-1 call whose neighbouring rows have different constant bytes (one of them none, one all)."""
    rows = 19
    img, sets = N.mixed_constant_rows(rows, cols, seed=cols)
    assert len(set(sets)) >= 7
    for i, (kt, desc) in enumerate(((U64, False), (I64, True), (F64, False))):
        c = image_case(gs, cuda, img, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(1, 1))
        c.check(5, 1, MODES[i])


def test_small_integers_and_timestamps_on_all_three_paths(gs, cuda):
    for rows, cols, k, path, levels in EDGE_SHAPES:
        for i, mat in enumerate((N.small_int_rows(rows, cols, seed=cols), N.timestamp_rows(rows, cols, seed=cols + 1))):
            for desc in (False, True):
                c = Case(gs, cuda, mat, cols, I64, desc)
                c.check(rows, k, MODES[(i + desc) % 3], plan=(path, levels))
                c.check(rows, k, ARGS)


def test_a_chunked_row_whose_chunks_have_different_constant_bytes(gs, cuda):
    cols, k = 9 * CH + 33, 300
    img = np.stack([N.chunked_constant_row(cols, seed=s) for s in (1, 2)])
    for kt, desc in ((U64, False), (F64, True)):
        c = image_case(gs, cuda, img, kt, desc)
        for mode in MODES:
            c.check(2, k, mode, plan=(3, 2))


# ------------------------------------------------------------------------------------------------ the pad image --
@pytest.mark.parametrize("cols", [61, 65, 300, 1000, 1500, CH - 3, CH + 37])
def test_rows_full_of_the_pad_image_lose_no_key_to_a_pad(gs, cuda, cols):
    """Rows whose keys have the image 0xffff...f -- the pad's -- but for a few smaller ones, at column counts off the multiples
    of 64 and with k reaching into them: the pads of the last registers have the same image and must lose by position alone,
    so the columns of the run come out in order and none is past the row's end."""
    rows = 4
    few = min(5, cols // 8)
    for i, kt in enumerate(N.KEY_TYPES):
        desc = bool(i % 2)
        c = image_case(gs, cuda, N.pad_image_rows(rows, cols, few, seed=cols + i), kt, desc)
        for k in sorted({min(cols, 1024), min(cols, 1024) - 1, min(cols, 1024) // 2 + 1, few + 1}):
            ek, ev = c.check(rows, k, ARGS)
            assert (ev < cols).all() and np.array_equal(ev[rows - 1], np.arange(k, dtype=np.uint32))
            assert (np.diff(ev[:, few:].astype(np.int64), axis=1) > 0).all()
            c.check(rows, k, (KEYS, PAIRS)[i % 2])


def test_a_row_longer_than_65536_with_ties_across_every_chunk(gs, cuda):
    """70001 columns of eight values at k = 1024 (nine chunks leave 9216 candidates: three levels): every chunk hands over 1024
    candidates out of tie runs, and the cut falls inside a run that crosses every chunk boundary."""
    rows, cols, k = 2, 70001, 1024
    rng = np.random.default_rng(9)
    for kt, desc in ((F64, True), (U64, False)):
        mat = rng.integers(0, 1 << 63, (rows, cols), dtype=np.uint64) * np.uint64(2) & np.uint64(0x8000000000030000)
        mat[1] = 0x8000000000030000                           # one run over the whole row
        mat[1, ::9000] = 0x0000000000010000
        c = Case(gs, cuda, mat, cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, 3))


def test_double_rows_with_nans_of_both_signs_and_signed_zeros(gs, cuda):
    inf = 0x7FF0000000000000
    for desc in (False, True):
        for rows, cols, k, path in ((6, 500, 60, 1), (3, 3000, 300, 2), (2, CH + 100, 500, 3)):
            c = Case(gs, cuda, N.matrix64(rows, cols, F64, seed=140 + cols % 11, kinds=["special"]), cols, F64, desc)
            ek, _ = c.check(rows, k, ARGS, plan=(path, 2 if path == 3 else 1))
            c.check(rows, k, PAIRS)
            first = ek[:, 0]
            assert ((first & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(inf)).all()            # a NaN:
            assert ((first >> np.uint64(63)) == (0 if desc else 1)).all()                       # positive largest, negative smallest
        # -0 before +0 ascending, +0 before -0 descending, columns in order inside each; denormals around them
        z, m = 0x0000000000000000, 0x8000000000000000
        mat = np.tile(np.array([z, m, m, z, z], np.uint64), (2, 60))
        c = Case(gs, cuda, mat, 300, F64, desc)
        ek, ev = c.check(2, 200, ARGS)
        assert (ek[:, :120] == (z if desc else m)).all() and (ek[:, 180:] == (m if desc else z)).all()
        mat = np.tile(np.array([z, m, 1, m | 1, 0x000FFFFFFFFFFFFF, inf, m | inf], np.uint64), (2, 50))
        Case(gs, cuda, mat, 350, F64, desc).check(2, 349, PAIRS)


# ------------------------------------------------------------------------------------------------------ strides --
@pytest.mark.parametrize("cols,k,path,levels", RR.STRIDE_SHAPES)
def test_the_stride_gap_holds_the_keys_that_would_win(gs, cuda, cols, k, path, levels):
    rows, stride = 5, cols + 3
    for desc in (False, True):
        mat = N.matrix64(rows, cols, U64, seed=80 + cols % 7, stride=stride, kinds=["uniform", "small", "five"])
        mat[:, :cols] = np.clip(mat[:, :cols], np.uint64(1), ONES - np.uint64(1))
        mat[:, cols:] = ONES if desc else 0
        mat[:, cols + 1] = 0 if desc else ONES
        c = Case(gs, cuda, mat, cols, U64, desc)
        before_k, before_v = c.d_keys.clone(), c.d_vals.clone()
        for mode in MODES:
            ek, ev = c.check(rows, k, mode, plan=(path, levels))
            assert not np.isin(ek, np.array([0, ONES], dtype=np.uint64)).any() and (mode != ARGS or (ev < cols).all())
        assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path, levels):
    """Every array in a slot of its own between guard zones, the key arrays at 8-byte offsets off a 256-byte boundary, the
    workspace at an odd one, outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = N.KEY_TYPES[i], bool(i % 2)
        mat = N.matrix64(rows, cols, kt, seed=90 + i, stride=stride)
        mat[:, cols:] = ONES if desc else 0
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRows64.Plan(rows, cols, k, hv)[:2] == [path, levels]
        a = Arena(cuda, seed=i)
        a.add("keys_in", 8 * span, offset=(8, 24, 40)[i], data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 8 * rows * k, offset=(24, 8, 56)[i], fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_rows_u64(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                     a.ptr("vals_out") if hv else None, rows, cols, stride, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev = N.rows_topk64(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint64).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    """Every refusal of the contract, on an arena in which no byte may change; key extents are 8 bytes per key (an output at
    the input's last key shares a byte with it, which a 4-byte extent would not see)."""
    rows, cols, k = 3, 9000, 10
    nb = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 8 * rows * cols, fill="random").add("vals_in", 4 * rows * cols, fill="random")
    a.add("keys_out", 8 * rows * k, fill="random").add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), vin=None, kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows,
                 cols=cols, stride=cols, k=k, kt=U64)
        p.update(kw)
        return gs.lib.gs_topk_rows_u64(p["temp"], p["nb"], p["kin"], p["vin"], p["kout"], p["vout"], p["rows"], p["cols"], p["stride"],
                                       p["k"], 0, p["kt"], None)
    refusals = (dict(k=cols + 1), dict(k=1025), dict(stride=cols - 1), dict(rows=1 << 20, cols=10, stride=1 << 12),
                dict(rows=1 << 20, cols=1 << 12, stride=1 << 12), dict(rows=1 << 23, cols=1000, stride=1000, k=512), dict(kt=0),
                dict(kt=2), dict(kt=8), dict(kt=6), dict(kt=-1), dict(vin=a.ptr("vals_in"), vout=None), dict(kin=None), dict(kout=None),
                dict(nb=nb - 1), dict(temp=None), dict(kin=a.ptr("keys_in") + 4), dict(kout=a.ptr("keys_out") + 4),
                dict(vout=a.ptr("vals_out") + 2), dict(vin=a.ptr("vals_in") + 2), dict(kout=a.ptr("keys_in") + 8),
                dict(kout=a.ptr("keys_in") + 8 * rows * cols - 8), dict(vout=a.ptr("keys_out") + 8 * rows * k - 4),
                dict(vin=a.ptr("keys_in") + 8 * rows * cols - 4))
    for kw in refusals:
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A chunked pairs call, a one-workgroup keys call and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, _, _), second = RR.REUSE_SHAPES
    assert second[:3] == (6, 5000, 77)
    a = Case(gs, cuda, N.matrix64(rows, cols, F64, seed=100), cols, F64, True)
    b = Case(gs, cuda, N.matrix64(6, 5000, I64, seed=101), 5000, I64, False)
    nb = max(gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_u64_temp_bytes(6, 5000, 77, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int64, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((6 * 77,), -1, dtype=torch.int64, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_rows_u64(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), rows,
                                       cols, cols, k, 1, F64, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_rows_u64(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, 6, 5000, 5000, 77, 0, I64,
                                   None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host64(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host32(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host64(kb).reshape(6, 77), b.expect(6, 77, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GRAPH_SHAPES)
def test_topk_rows64_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path, levels):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers."""
    sets = [N.matrix64(rows, cols, F64, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("normal", "small", "five"))]
    src = dev64(sets[0], cuda).view(torch.float64)
    ko = torch.zeros(rows * k, dtype=torch.float64, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopKRows64.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert nb == gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1)
    assert gs.DeviceTopKRows64.Plan(rows, cols, k, True)[:2] == [path, levels]
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopKRows64.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopKRows64.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k)
    for mat in sets:
        src.copy_(dev64(mat, cuda).view(torch.float64))
        ko.view(torch.int64).fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = N.rows_topk64(mat, cols, k, F64, True)
        assert np.array_equal(host64(ko.view(torch.int64)).reshape(rows, k), ek) and np.array_equal(host32(vo).reshape(rows, k), ev)


# ------------------------------------------------------------------------------------------ the widen identity --
@pytest.mark.parametrize("rows,cols,k,path", [(37, 333, 50, 1), (5, 6001, 257, 2), (3, 3 * CH + 11, 1024, 3)])
def test_the_widen_identity_on_the_device(gs, cuda, rows, cols, k, path):
    """gs_topk_rows_u64 on (uint64_t)key << 32 with the widened key type against gs_topk_rows_u32 on the keys: the keys shifted
    back, values and columns unchanged, bit for bit, in all three forms.  F32 rows of mixed sign make the low four bytes of the
    image two-valued (0x00000000 under a positive key, 0xffffffff under a negative one): the skip must not take them for
    constant."""
    stride = cols + 1
    for i, kt in enumerate((R.U32, R.I32, R.F32)):
        desc = bool(i % 2)
        mat = np.zeros((rows, stride), np.uint32)
        for r in range(rows):
            mat[r, :cols] = gen(("uniform", "zipf", "topbyte")[(r + i) % 3], cols, seed=130 + 7 * i + r, kt=kt)
        if kt == R.F32:
            assert ((mat[:, :cols] >> 31).min(axis=1) == 0).any() and ((mat[:, :cols] >> 31).max(axis=1) == 1).any()
        vals = values_for(mat.shape, seed=i)
        d32, d64, dv = dev32(mat, cuda), dev64(N.widen32(mat), cuda), dev32(vals, cuda)
        assert gs.DeviceTopKRows64.Plan(rows, cols, k, 1)[0] == path
        for mode in MODES:
            hv = int(mode != KEYS)
            nb64, nb32 = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv), gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
            t64 = torch.full((nb64,), 0xA5, dtype=torch.uint8, device=cuda)
            t32 = torch.full((nb32,), 0xA5, dtype=torch.uint8, device=cuda)
            k64 = torch.full((rows * k,), -1, dtype=torch.int64, device=cuda)
            k32, v64, v32 = (torch.full((rows * k,), -1, dtype=torch.int32, device=cuda) for _ in range(3))
            vin = dv.data_ptr() if mode == PAIRS else None
            assert gs.lib.gs_topk_rows_u64(t64.data_ptr(), nb64, d64.data_ptr(), vin, k64.data_ptr(), v64.data_ptr() if hv else None, rows,
                                           cols, stride, k, int(desc), N.WIDE[kt], None) == 0
            assert gs.lib.gs_topk_rows_u32(t32.data_ptr(), nb32, d32.data_ptr(), vin, k32.data_ptr(), v32.data_ptr() if hv else None, rows,
                                           cols, stride, k, int(desc), kt, None) == 0
            w = host64(k64)
            assert (w & np.uint64(0xFFFFFFFF) == 0).all() and np.array_equal((w >> np.uint64(32)).astype(np.uint32), host32(k32)), (kt, mode)
            assert torch.equal(v64, v32), (kt, mode)


# ------------------------------------------------------------------------------------------------- front ends --
def _scores(rows, cols, dtype, seed):
    """Scores on a coarse grid, many of them equal, without NaN or zero of either sign."""
    rng = np.random.default_rng(seed)
    if dtype == torch.int64:
        return torch.from_numpy(rng.integers(-3000, 3000, (rows, cols)).astype(np.int64) * (1 << 33))
    x = torch.from_numpy(rng.integers(-200, 200, (rows, cols)) / 8.0 + 0.0625).to(dtype)
    assert not torch.isnan(x).any() and (x != 0).all()
    return x


_KT = {torch.int64: I64, torch.float64: F64}


@pytest.mark.parametrize("dtype", [torch.float64, torch.int64])
@pytest.mark.parametrize("rows,cols,k", [(33, 100, 5), (4, 5000, 50), (3, 20000, 1000)])
def test_topk_rows64_against_torch_topk(gs, cuda, dtype, rows, cols, k):
    """Values equal torch.topk's; the indices equal the reference (torch.topk does not promise the lowest index among ties);
    gathering the input at the indices gives the values back."""
    wide = _scores(rows, cols + 40, dtype, seed=cols).to(cuda)
    for lo in (0, 17):        # the second: a non-contiguous column slice
        x = wide[:, :cols].contiguous() if lo == 0 else wide[:, lo:lo + cols]
        bits = x.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)
        for largest in (False, True):
            want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
            ko, io = gs.topk_rows64(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values)
            ek, ev = N.rows_topk64(bits, cols, k, _KT[dtype], largest)
            assert np.array_equal(host64(ko.view(torch.int64)).reshape(rows, k), ek)
            assert np.array_equal(host32(io).reshape(rows, k), ev)
            assert torch.equal(x.gather(1, io.long()), ko)
            k2, none = gs.topk_rows64(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows64(x, k, largest=True, values=v)
    _, io = gs.topk_rows64(x, k, largest=True, indices=True)
    assert torch.equal(ko, torch.topk(x, k, dim=1, largest=True).values) and torch.equal(vo, torch.gather(v, 1, io.long()))


def test_topk_rows64_above_max_k_loops_the_flat_top_k(gs, cuda):
    rows, cols = 3, 5000
    k = gs.DeviceTopKRows64.MaxK() + 76
    assert gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1) == 0
    x = _scores(rows, cols + 8, torch.float64, seed=5).to(cuda)[:, 4:4 + cols]
    bits = x.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)
    for largest in (False, True):
        ko, io = gs.topk_rows64(x, k, largest=largest, indices=True)
        ek, ev = N.rows_topk64(bits, cols, k, F64, largest)
        assert np.array_equal(host64(ko.view(torch.int64)).reshape(rows, k), ek) and np.array_equal(host32(io).reshape(rows, k), ev)


def test_device_topk_rows64_two_phase_and_explicit_key_type(gs, cuda):
    tmp = torch.empty(256, dtype=torch.uint8, device=cuda)
    bits = torch.tensor([[0x3FF0000000000000, -0x4010000000000000, 0, -0x4000000000000000, 0x4000000000000000]], dtype=torch.int64,
                        device=cuda)                                                                # 1, -1, 0, -2, 2 as doubles
    o = torch.empty(5, dtype=torch.int64, device=cuda)
    gs.DeviceTopKRows64.MinKeys(tmp, 256, bits, o, 1, 5, 5, 5, key_type=gs.GS_KEY_F64)
    assert o.view(torch.float64).tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    gs.DeviceTopKRows64.MinKeys(tmp, 256, bits, o, 1, 5, 5, 5)                                   # as int64
    assert o.tolist() == [-0x4010000000000000, -0x4000000000000000, 0, 0x3FF0000000000000, 0x4000000000000000]
    gs.DeviceTopKRows64.MaxKeys(tmp, 256, bits, o, 1, 5, 5, 5, key_type=gs.GS_KEY_U64)           # negative patterns are the largest
    assert o.tolist() == [-0x4000000000000000, -0x4010000000000000, 0x4000000000000000, 0x3FF0000000000000, 0]
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopKRows64.MinKeys(tmp, 256, bits, o, 1, 5, 4, 5)                               # row_stride < num_cols
    with pytest.raises(ValueError):
        gs.DeviceTopKRows64.MinKeys(tmp, 256, bits, o.int(), 1, 5, 5, 5)                         # a 4-byte key output


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_wide_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 3 * 7 * 3 * 2 * 3
