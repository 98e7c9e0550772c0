"""gs_topk_rows_u16 on the device: every row bit for bit against tests/topk_rows_narrow_ref.py (keys, values or columns), over
the shapes of the three paths, k values, row counts, distributions mixed across the rows of one call, directions, forms and
the four key types; 2-byte alignment of row bases and output rows; the edges the key width brings (a shared top byte, rows of
the pad image, ties across every chunk of a long row, NaNs of both signs); guarded, offset and dirty buffers; workspace reuse;
identical bytes; graph capture; the widen identity against gs_topk_rows_u32; the Python front ends and the C++ driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_rows_ref as RR
import topk_rows_narrow_ref as N
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U16, I16, F16, BF16 = N.U16, N.I16, N.F16, N.BF16
KEYS, PAIRS, ARGS = N.KEYS, N.PAIRS, N.ARGS
MODES = N.MODES
CH = RR.CH
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written


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


class Case:
    """One matrix on the device with its reference; .check(rows, k, mode) runs the C entry point on the first `rows` rows and
    compares every row.  in_off / out_off: the key input / output starts that many elements into its allocation."""

    def __init__(self, gs, cuda, mat, cols, kt, desc, in_off=0):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride, self.in_off = mat, mat.shape[1], in_off
        self.vals = values_for(mat.shape)
        self.d_keys = dev16(np.concatenate([np.full(in_off, 0x5A5A, np.uint16), mat.reshape(-1)]), cuda)
        self.d_vals = dev32(self.vals, cuda)
        self.order = N.rows_order(mat, cols, kt, desc)          # computed once, shared by every k, row count and form

    def expect(self, rows, k, mode):
        return N.rows_topk16(self.mat[:rows], self.cols, k, self.kt, self.desc, self.vals[:rows] if mode == PAIRS else None,
                             order=self.order[:rows])

    def check(self, rows, k, mode, plan=None, out_off=0):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d off=%d/%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc,
                                                                                self.in_off, out_off)
        if plan is not None:
            assert gs.DeviceTopKRows.Plan(rows, cols, k, hv)[:2] == list(plan), what
        nb = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((out_off + rows * k + TAIL,), -1, dtype=torch.int16, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_rows_u16(temp.data_ptr(), nb, self.d_keys.data_ptr() + 2 * self.in_off,
                                     self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr() + 2 * out_off,
                                     vo.data_ptr() if hv else None, rows, cols, self.stride, k, int(self.desc), self.kt, None)
        assert rc == 0, (rc, what)
        ek, ev = self.expect(rows, k, mode)
        gk, gv = host16(ko), host32(vo)
        assert (gk[:out_off] == 0xFFFF).all(), what
        gk = gk[out_off:]
        bad = np.nonzero((gk[:rows * k].reshape(rows, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of rows", bad[:8])
        assert gk[rows * k:].size == TAIL and (gk[rows * k:] == 0xFFFF).all(), what
        if hv:
            bad = np.nonzero((gv[:rows * k].reshape(rows, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of rows", bad[:8])
            assert (gv[rows * k:] == 0xFFFFFFFF).all(), what
        else:
            assert (gv == 0xFFFFFFFF).all(), what
        return ek, ev


def rotate(i):
    return N.KEY_TYPES[i % 4], bool((i // 4) % 2), MODES[(i // 2) % 3]


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RR.PATH1_COLS)
def test_path1_one_wave_per_row(gs, cuda, cols):
    """Every k and row count of the list; 1000 rows cover four rows per workgroup and (with 1, 3, 5) a ragged last one.  The
    distributions are mixed across the rows; form, key type and direction rotate."""
    ci = RR.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RR.path1_ks(cols)):
        for i, rows in enumerate(RR.PATH1_ROWS):
            kt, desc, mode = rotate(ci + 3 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, N.matrix16(max(RR.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
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
                cases[(kt, desc)] = Case(gs, cuda, N.matrix16(max(RR.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, plan=(2, 1))


# ------------------------------------------------------------------------------------------------------- path 3 --
@pytest.mark.parametrize("shape", RR.PATH3_SHAPES)
def test_path3_chunked(gs, cuda, shape):
    rows, cols, k, levels = shape
    si = RR.PATH3_SHAPES.index(shape)
    for i in range(4):
        kt, desc, _ = rotate(si + 5 * i)
        c = Case(gs, cuda, N.matrix16(rows, cols, kt, seed=60 + si), cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


@pytest.mark.parametrize("shape", RR.MIDDLE_SHAPES)
def test_path3_middle_level_in_every_class_of_the_finishing_wave(gs, cuda, shape):
    """Three levels at k = 64, 256 and 512: the middle level reads 16-bit candidate keys with their columns and writes a
    candidate row again, with a finishing wave of 1, 4 and 8 per lane (PATH3_SHAPES has three levels at k = 1024 alone)."""
    rows, cols, k, levels = shape
    kt, desc, _ = rotate(2 + 3 * RR.MIDDLE_SHAPES.index(shape))
    c = Case(gs, cuda, N.matrix16(rows, cols, kt, seed=80 + k, kinds=["five", "uniform", "special"]), cols, kt, desc)
    for mode in MODES:
        c.check(rows, k, mode, plan=(3, levels))


# ---------------------------------------------------------------------------------------------------- alignment --
ALIGN_SHAPES = [(257, 101, 1, 1), (1024, 1023, 1, 1), (4001, 65, 2, 1), (CH + 5, 1023, 3, 2)]     # (cols, odd k, path, levels)


@pytest.mark.parametrize("cols,k,path,levels", ALIGN_SHAPES)
def test_two_byte_alignment_of_row_bases_and_output_rows(gs, cuda, cols, k, path, levels):
    """An odd row_stride, so that row bases alternate between 2- and 4-byte alignment; the key input at the start of its
    allocation and one element in; an odd k, so that output rows alternate too; the key output at the start and one element
    in.  The stride gap holds the keys that would win (0x0000 and 0xFFFF, the extremes of the u16 order in both directions),
    which no key of the rows equals: none may appear in the output, and the input is unchanged after the call."""
    rows = 5
    stride = cols + 3 if (cols + 3) % 2 else cols + 4
    assert stride % 2 == 1 and k % 2 == 1
    for desc in (False, True):
        mat = N.matrix16(rows, cols, U16, seed=80 + cols % 7, stride=stride, kinds=["uniform", "topbyte", "zipf"])
        mat[:, :cols] = np.clip(mat[:, :cols], 1, 0xFFFE)
        mat[:, cols:] = 0xFFFF if desc else 0
        mat[:, cols + 1] = 0 if desc else 0xFFFF
        for in_off in (0, 1):
            c = Case(gs, cuda, mat, cols, U16, desc, in_off=in_off)
            before_k, before_v = c.d_keys.clone(), c.d_vals.clone()
            for out_off in (0, 1):
                for mode in MODES:
                    ek, ev = c.check(rows, k, mode, plan=(path, levels), out_off=out_off)
                    assert not np.isin(ek, [0, 0xFFFF]).any() and (mode != ARGS or (ev < cols).all())
            assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


def test_arrays_packed_at_two_bytes_per_key_are_accepted(gs, cuda):
    """The overlap check uses 2-byte key extents: values directly behind the keys' last byte (rounded up to 4) and outputs
    directly behind those share no byte and are served; a 4-byte key extent would reach into them."""
    rows, cols, k = 3, 301, 7
    span = rows * cols
    mat = N.matrix16(rows, cols, BF16, seed=7)
    vals = values_for(mat.shape)
    a_vin = (2 * span + 3) & ~3
    a_kout = a_vin + 4 * span
    a_vout = (a_kout + 2 * rows * k + 3) & ~3
    a_temp = a_vout + 4 * rows * k
    nb = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
    buf = torch.zeros(a_temp + nb, dtype=torch.uint8, device=cuda)
    buf[:2 * span] = torch.from_numpy(mat.reshape(-1).view(np.uint8).copy()).to(cuda)
    buf[a_vin:a_vin + 4 * span] = torch.from_numpy(vals.reshape(-1).view(np.uint8).copy()).to(cuda)
    p = buf.data_ptr()
    assert p % 4 == 0 and a_vin < 4 * span
    rc = gs.lib.gs_topk_rows_u16(p + a_temp, nb, p, p + a_vin, p + a_kout, p + a_vout, rows, cols, cols, k, 1, BF16, None)
    assert rc == 0
    ek, ev = N.rows_topk16(mat, cols, k, BF16, True, vals)
    out = buf.cpu().numpy()
    assert np.array_equal(out[a_kout:a_kout + 2 * rows * k].view(np.uint16).reshape(rows, k), ek)
    assert np.array_equal(out[a_vout:a_vout + 4 * rows * k].view(np.uint32).reshape(rows, k), ev)
    assert np.array_equal(out[:2 * span].view(np.uint16), mat.reshape(-1))
    # one element closer, and they share a byte
    assert gs.lib.gs_topk_rows_u16(p + a_temp, nb, p, p + a_vin - 4, p + a_kout, p + a_vout, rows, cols, cols, k, 1, BF16, None) == 1
    assert gs.lib.gs_topk_rows_u16(p + a_temp, nb, p, p + a_vin, p + a_kout, p + a_vout - 4, rows, cols, cols, k, 1, BF16, None) == 1


# ------------------------------------------------------------------------------------------ width-specific edges --
EDGE_SHAPES = [(5, 700, 100, 1, 1), (3, 5000, 1000, 2, 1), (2, 2 * CH + 9, 1024, 3, 2)]     # (rows, cols, k, path, levels)


@pytest.mark.parametrize("rows,cols,k,path,levels", EDGE_SHAPES)
def test_rows_whose_keys_share_the_top_byte_and_rows_of_one_key(gs, cuda, rows, cols, k, path, levels):
    """One top byte: the first select round and the second pass of the wave sort decide nothing.  All keys equal: the result
    is the first k columns."""
    for i, (kt, desc) in enumerate(((U16, False), (I16, True), (F16, True), (BF16, False))):
        c = Case(gs, cuda, N.matrix16(rows, cols, kt, seed=120 + i, kinds=["topbyte", "top3"]), cols, kt, desc)
        assert (np.unique(c.mat >> 8, axis=1).shape[1] == 1)
        for mode in MODES:
            c.check(rows, k, mode, plan=(path, levels))
        c = Case(gs, cuda, np.full((rows, cols), 0x3F80, np.uint16), cols, kt, desc)
        assert np.array_equal(c.expect(rows, k, ARGS)[1], np.tile(np.arange(k, dtype=np.uint32), (rows, 1)))
        for mode in MODES:
            c.check(rows, k, mode, plan=(path, levels))


@pytest.mark.parametrize("cols", [61, 65, 300, 1000, 1500, CH - 3, CH + 37])
def test_rows_full_of_the_pad_image_lose_no_key_to_a_pad(gs, cuda, cols):
    """Rows whose keys have the image 0xffff -- the pad's -- but for a few smaller ones, at column counts off the multiples of
    64 and with k reaching into them: the pads of the last registers have the same image and must lose by position alone, so
    the columns of the run come out in order and none is past the row's end."""
    rows = 4
    rng = np.random.default_rng(cols)
    for i, kt in enumerate(N.KEY_TYPES):
        desc = bool(i % 2)
        img = np.full((rows, cols), 0xFFFF, np.uint16)
        few = min(5, cols // 8)
        for r in range(rows):
            img[r, rng.choice(cols, few, replace=False)] = rng.integers(0, 0xFFFF, few, dtype=np.uint32).astype(np.uint16)
        img[rows - 1] = 0xFFFF                                  # and a row of nothing else
        mat = N.preimage16(img, kt, desc)
        assert (N.image16(mat, kt, desc) == img).all()
        c = Case(gs, cuda, mat, cols, kt, desc)
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
    for kt, desc in ((BF16, True), (U16, False)):
        mat = (rng.integers(0, 1 << 16, (rows, cols), dtype=np.uint32).astype(np.uint16) & np.uint16(0x8003))
        mat[1] = 0x8003                                      # one run over the whole row
        mat[1, ::9000] = 0x0001
        c = Case(gs, cuda, mat, cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, 3))


@pytest.mark.parametrize("kt", [F16, BF16])
def test_float_rows_with_nans_of_both_signs_and_signed_zeros(gs, cuda, kt):
    inf = 0x7C00 if kt == F16 else 0x7F80
    for desc in (False, True):
        for rows, cols, k, path in ((6, 500, 60, 1), (3, 3000, 300, 2), (2, CH + 100, 500, 3)):
            c = Case(gs, cuda, N.matrix16(rows, cols, kt, seed=140 + cols % 11, kinds=["special"]), cols, kt, desc)
            ek, _ = c.check(rows, k, ARGS, plan=(path, 2 if path == 3 else 1))
            c.check(rows, k, PAIRS)
            first = ek[:, 0]
            if desc:        # the largest: positive NaNs
                assert ((first & 0x7FFF) > inf).all() and (first < 0x8000).all()
            else:           # the smallest: negative NaNs
                assert ((first & 0x7FFF) > inf).all() and (first >= 0x8000).all()
        # -0 before +0 ascending, +0 before -0 descending, columns in order inside each
        mat = np.tile(np.array([0x0000, 0x8000, 0x8000, 0x0000, 0x0000], np.uint16), (2, 60))
        c = Case(gs, cuda, mat, 300, kt, desc)
        ek, ev = c.check(2, 200, ARGS)
        assert (ek[:, :120] == (0x0000 if desc else 0x8000)).all() and (ek[:, 180:] == (0x8000 if desc else 0x0000)).all()


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path, levels):
    """Every array in a slot of its own between guard zones, the key arrays at byte offsets 2, 6 and 10, ... from a 256-byte
    boundary (the workspace at an odd one), outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = (U16, F16, BF16)[i], bool(i % 2)
        mat = N.matrix16(rows, cols, kt, seed=90 + i, stride=stride)
        mat[:, cols:] = 0xFFFF if desc else 0
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRows.Plan(rows, cols, k, hv)[:2] == [path, levels]
        a = Arena(cuda, seed=i)
        a.add("keys_in", 2 * span, offset=(2, 6, 10)[i], data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 2 * rows * k, offset=(6, 2, 14)[i], fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 130)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_rows_u16(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                     a.ptr("vals_out") if hv else None, rows, cols, stride, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev = N.rows_topk16(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint16).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    rows, cols, k = 3, 9000, 10
    nb = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 2 * rows * cols, fill="random").add("keys_out", 2 * rows * k, fill="random")
    a.add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows, cols=cols,
                 stride=cols, k=k, kt=U16)
        p.update(kw)
        return gs.lib.gs_topk_rows_u16(p["temp"], p["nb"], p["kin"], None, p["kout"], p["vout"], p["rows"], p["cols"], p["stride"], p["k"],
                                       0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=cols + 1), dict(k=1025), dict(stride=cols - 1), dict(kt=2), dict(kt=5),
               dict(kt=6), dict(kout=a.ptr("keys_in") + 2), dict(vout=a.ptr("keys_out") + ((2 * rows * k - 1) & ~3)),
               dict(kin=a.ptr("keys_in") + 1), dict(kout=a.ptr("keys_out") + 1), dict(vout=a.ptr("vals_out") + 2)):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A chunked pairs call, a one-workgroup keys call and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, _, _), second = RR.REUSE_SHAPES
    assert second[:3] == (6, 5000, 77)
    a = Case(gs, cuda, N.matrix16(rows, cols, BF16, seed=100), cols, BF16, True)
    b = Case(gs, cuda, N.matrix16(6, 5000, I16, seed=101), 5000, I16, False)
    nb = max(gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_u16_temp_bytes(6, 5000, 77, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int16, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((6 * 77,), -1, dtype=torch.int16, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_rows_u16(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), rows,
                                       cols, cols, k, 1, BF16, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_rows_u16(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, 6, 5000, 5000, 77, 0, I16,
                                   None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host16(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host32(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host16(kb).reshape(6, 77), b.expect(6, 77, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GRAPH_SHAPES)
def test_topk_rows_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path, levels):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers."""
    sets = [N.matrix16(rows, cols, BF16, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "five"))]
    src = dev16(sets[0], cuda).view(torch.bfloat16)
    ko = torch.zeros(rows * k, dtype=torch.bfloat16, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopKRows.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k, key_type=gs.GS_KEY_BF16)
    assert nb == gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
    assert gs.DeviceTopKRows.Plan(rows, cols, k, True)[:2] == [path, levels]
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopKRows.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopKRows.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k)
    for mat in sets:
        src.copy_(dev16(mat, cuda).view(torch.bfloat16))
        ko.view(torch.int16).fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = N.rows_topk16(mat, cols, k, BF16, True)
        assert np.array_equal(host16(ko.view(torch.int16)).reshape(rows, k), ek) and np.array_equal(host32(vo).reshape(rows, k), ev)


# ------------------------------------------------------------------------------------------ the widen identity --
@pytest.mark.parametrize("rows,cols,k,path", [(37, 333, 50, 1), (5, 6001, 257, 2), (3, 3 * CH + 11, 1024, 3)])
def test_the_widen_identity_on_the_device(gs, cuda, rows, cols, k, path):
    """gs_topk_rows_u16 against gs_topk_rows_u32 on (uint32_t)key << 16 with the widened key type: the keys shifted back,
    values and columns unchanged, bit for bit, in all three forms."""
    stride = cols + 1
    for i, kt in enumerate(N.KEY_TYPES):
        desc = bool(i % 2)
        mat = N.matrix16(rows, cols, kt, seed=130 + i, stride=stride)
        vals = values_for(mat.shape, seed=i)
        d16, d32, dv = dev16(mat, cuda), dev32(N.widen(mat), cuda), dev32(vals, cuda)
        assert gs.DeviceTopKRows.Plan(rows, cols, k, 1)[0] == path
        for mode in MODES:
            hv = int(mode != KEYS)
            nb16, nb32 = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv), gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
            t16 = torch.full((nb16,), 0xA5, dtype=torch.uint8, device=cuda)
            t32 = torch.full((nb32,), 0xA5, dtype=torch.uint8, device=cuda)
            k16 = torch.full((rows * k,), -1, dtype=torch.int16, device=cuda)
            k32, v16, v32 = (torch.full((rows * k,), -1, dtype=torch.int32, device=cuda) for _ in range(3))
            vin = dv.data_ptr() if mode == PAIRS else None
            assert gs.lib.gs_topk_rows_u16(t16.data_ptr(), nb16, d16.data_ptr(), vin, k16.data_ptr(), v16.data_ptr() if hv else None, rows,
                                           cols, stride, k, int(desc), kt, None) == 0
            assert gs.lib.gs_topk_rows_u32(t32.data_ptr(), nb32, d32.data_ptr(), vin, k32.data_ptr(), v32.data_ptr() if hv else None, rows,
                                           cols, stride, k, int(desc), N.WIDE[kt], None) == 0
            w = host32(k32)
            assert (w & 0xFFFF == 0).all() and np.array_equal((w >> 16).astype(np.uint16), host16(k16)), (kt, mode)
            assert torch.equal(v16, v32), (kt, mode)


# ------------------------------------------------------------------------------------------------- front ends --
def _scores(rows, cols, dtype, seed):
    """Scores on a coarse grid, many of them equal, without NaN or zero of either sign."""
    rng = np.random.default_rng(seed)
    if dtype == torch.int16:
        return torch.from_numpy(rng.integers(-3000, 3000, (rows, cols)).astype(np.int16))
    x = torch.from_numpy((rng.integers(-200, 200, (rows, cols)) / 8.0 + 0.0625).astype(np.float32)).to(dtype)
    assert not torch.isnan(x.float()).any() and (x.float() != 0).all()
    return x


_KT = {torch.int16: I16, torch.float16: F16, torch.bfloat16: BF16}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.int16])
@pytest.mark.parametrize("rows,cols,k", [(33, 100, 5), (4, 5000, 50), (3, 20000, 1000)])
def test_topk_rows_against_torch_topk(gs, cuda, dtype, rows, cols, k):
    """Values equal torch.topk's; the indices equal the reference (torch.topk does not promise the lowest index among ties, and
    16-bit rows are full of ties); gathering the input at the indices gives the values back."""
    wide = _scores(rows, cols + 40, dtype, seed=cols).to(cuda)
    for lo in (0, 17):        # the second: a non-contiguous row slice, and its data pointer is 2- but not 4-aligned
        x = wide[:, :cols].contiguous() if lo == 0 else wide[:, lo:lo + cols]
        bits = x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        for largest in (False, True):
            want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
            ko, io = gs.topk_rows(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values)
            ek, ev = N.rows_topk16(bits, cols, k, _KT[dtype], largest)
            assert np.array_equal(host16(ko.view(torch.int16)).reshape(rows, k), ek)
            assert np.array_equal(host32(io).reshape(rows, k), ev)
            assert torch.equal(x.gather(1, io.long()), ko)
            k2, none = gs.topk_rows(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows(x, k, largest=True, values=v)
    _, io = gs.topk_rows(x, k, largest=True, indices=True)
    assert torch.equal(ko, torch.topk(x, k, dim=1, largest=True).values) and torch.equal(vo, torch.gather(v, 1, io.long()))


def test_topk_rows_refusals_and_the_two_phase_form(gs, cuda):
    x = torch.zeros((4, 3000), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(ValueError):
        gs.topk_rows(x, gs.DeviceTopKRows.MaxK() + 1)                 # no flat 16-bit top-k to loop over
    with pytest.raises(ValueError):
        gs.topk_rows(x, 3001)
    with pytest.raises(ValueError):
        gs.topk_rows(x[:, ::2], 2)
    with pytest.raises(ValueError):
        gs.topk_rows(x, 2, values=x)                                  # 2-byte values
    with pytest.raises(TypeError):
        gs.topk_rows(x.double(), 2)
    out = torch.empty(4 * 2, dtype=torch.bfloat16, device=cuda)
    tmp = torch.empty(256, dtype=torch.uint8, device=cuda)
    with pytest.raises(TypeError):
        gs.DeviceTopKRows.MinKeys(tmp, 256, x, out, 4, 3000, 3000, 2, key_type=gs.GS_KEY_F32)      # a 32-bit type for 2-byte keys
    with pytest.raises(TypeError):
        gs.DeviceTopKRows.MinKeys(tmp, 256, x.float(), out.float(), 4, 3000, 3000, 2, key_type=gs.GS_KEY_BF16)
    with pytest.raises(ValueError):
        gs.DeviceTopKRows.MinKeys(tmp, 256, x, out.float(), 4, 3000, 3000, 2)                      # a 4-byte key output
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopKRows.MinKeys(tmp, 256, x, out, 4, 3000, 50, 2)                                # row_stride < num_cols
    # an explicit key type decides the order: int16 storage read as bfloat16
    bits = torch.tensor([[0x3F80, -0x4080, 0x0000, -0x4000, 0x4000]], dtype=torch.int16, device=cuda)   # 1, -1, 0, -2, 2
    o = torch.empty(5, dtype=torch.int16, device=cuda)
    gs.DeviceTopKRows.MinKeys(tmp, 256, bits, o, 1, 5, 5, 5, key_type=gs.GS_KEY_BF16)
    assert o.tolist() == [-0x4000, -0x4080, 0x0000, 0x3F80, 0x4000]                                # -2, -1, 0, 1, 2
    gs.DeviceTopKRows.MinKeys(tmp, 256, bits, o, 1, 5, 5, 5)
    assert o.tolist() == [-0x4080, -0x4000, 0x0000, 0x3F80, 0x4000]                                # as int16
    ko, vo = gs.topk_rows(x, 0, indices=True)
    assert tuple(ko.shape) == (4, 0) and tuple(vo.shape) == (4, 0)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_narrow_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 4 * 7 * 3 * 3
