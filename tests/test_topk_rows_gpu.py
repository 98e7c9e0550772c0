"""gs_topk_rows_u32 on the device: every row bit for bit against tests/topk_rows_ref.py (keys, values or columns), over the
shapes of the three paths, k values, row counts, distributions mixed across the rows of one call, directions, forms and key
types; a row stride with a gap that would win; guarded, offset and dirty buffers; workspace reuse; identical bytes; graph
capture; the Python front ends and the C++ driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_ref as R
import topk_rows_ref as RR
from guarded import Arena
from topk_cases import DISTS, gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
CH = RR.CH
TAIL = 64            # sentinel elements behind the outputs: nothing outside [0, rows * k) is written


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


class Case:
    """One matrix on the device with its reference; .check(rows, k, mode) runs the C entry point on the first `rows` rows and
    compares every row."""

    def __init__(self, gs, cuda, mat, cols, kt, desc):
        self.gs, self.cuda, self.kt, self.desc, self.cols = gs, cuda, kt, desc, cols
        self.mat, self.stride = mat, mat.shape[1]
        self.vals = values_for(mat.shape)
        self.d_keys, self.d_vals = dev(mat, cuda), dev(self.vals, cuda)
        self.order = {}

    def expect(self, rows, k, mode):
        """Reference rows, from each row's stable order computed once."""
        ko, vo = np.empty((rows, k), np.uint32), np.empty((rows, k), np.uint32)
        for r in range(rows):
            if r not in self.order:
                self.order[r] = R.ranks(self.mat[r, :self.cols], self.kt, self.desc)
            o = self.order[r][:k]
            ko[r] = self.mat[r, o]
            vo[r] = self.vals[r, o] if mode == PAIRS else o
        return ko, vo

    def check(self, rows, k, mode, plan=None):
        gs, cols = self.gs, self.cols
        hv = int(mode != KEYS)
        what = "rows=%d cols=%d stride=%d k=%d %s kt=%d desc=%d" % (rows, cols, self.stride, k, mode, self.kt, self.desc)
        if plan is not None:
            assert gs.DeviceTopKRows.Plan(rows, cols, k, hv)[:2] == list(plan), what
        nb = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
        assert nb > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        vo = torch.full((rows * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_rows_u32(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
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


def rotate(i):
    return (U32, I32, F32)[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


# ------------------------------------------------------------------------------------------------------- path 1 --
@pytest.mark.parametrize("cols", RR.PATH1_COLS)
def test_path1_one_wave_per_row(gs, cuda, cols):
    """Every k and row count of the list; 1000 rows cover four rows per workgroup and (with 1, 3, 5) a ragged last one.  The
    distributions are mixed across the rows; form, key type and direction rotate."""
    ci = RR.PATH1_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RR.path1_ks(cols)):
        for i, rows in enumerate(RR.PATH1_ROWS):
            kt, desc, mode = rotate(ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, matrix(max(RR.PATH1_ROWS), cols, kt, seed=ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, plan=(1, 1))


# ------------------------------------------------------------------------------------------------------- path 2 --
@pytest.mark.parametrize("cols", RR.PATH2_COLS)
def test_path2_one_workgroup_per_row(gs, cuda, cols):
    ci = RR.PATH2_COLS.index(cols)
    cases = {}
    for j, k in enumerate(RR.PATH2_KS):
        for i, rows in enumerate(RR.PATH2_ROWS):
            kt, desc, mode = rotate(ci + 2 * j + i)
            if (kt, desc) not in cases:
                cases[(kt, desc)] = Case(gs, cuda, matrix(max(RR.PATH2_ROWS), cols, kt, seed=20 + ci), cols, kt, desc)
            cases[(kt, desc)].check(rows, k, mode, plan=(2, 1))


@pytest.mark.parametrize("kind", DISTS)
def test_path2_every_distribution_alone(gs, cuda, kind):
    """Each distribution in every row of a call (a full chunk minus one), all forms, types and directions."""
    cols, rows = CH - 1, 3
    for i in range(6):
        kt, desc = (U32, I32, F32)[i % 3], bool(i // 3)
        c = Case(gs, cuda, matrix(rows, cols, kt, seed=40 + i, kinds=[kind]), cols, kt, desc)
        for j, k in enumerate((1, 100, 1024)):
            c.check(rows, k, MODES[(i + j) % 3], plan=(2, 1))


# ------------------------------------------------------------------------------------------------------- path 3 --
@pytest.mark.parametrize("shape", RR.PATH3_SHAPES)
def test_path3_chunked(gs, cuda, shape):
    rows, cols, k, levels = shape
    si = RR.PATH3_SHAPES.index(shape)
    for i in range(3):
        kt, desc, _ = rotate(si + i)
        c = Case(gs, cuda, matrix(rows, cols, kt, seed=60 + si), cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


def test_path3_all_keys_equal_gives_the_first_columns(gs, cuda):
    rows, cols, k = 2, 2 * CH + 1, 1000
    for kt, desc in ((U32, False), (F32, True)):
        c = Case(gs, cuda, np.full((rows, cols), 0x3F800000, np.uint32), cols, kt, desc)
        assert np.array_equal(c.expect(rows, k, ARGS)[1], np.tile(np.arange(k, dtype=np.uint32), (rows, 1)))
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, 2))


def test_path3_tie_run_across_a_chunk_boundary_with_the_cut_inside(gs, cuda):
    """Ten smaller keys scattered over three chunks, then a run of equal keys from CH - 20 to CH + 20: k = 25 takes the ten and
    the first fifteen of the run (all in chunk 0), k = 40 crosses into chunk 1 and cuts the run there."""
    rows, cols = 2, 3 * CH
    rng = np.random.default_rng(5)
    mat = rng.integers(1 << 20, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    for r in range(rows):
        mat[r, CH - 20 - r:CH + 20] = 1000
        mat[r, rng.choice(np.r_[0:CH - 30, CH + 30:cols], 10, replace=False)] = np.arange(10, dtype=np.uint32)
    c = Case(gs, cuda, mat, cols, U32, False)
    for k in (25, 40, 50, 51):
        ev = c.expect(rows, k, ARGS)[1]
        if k == 40:
            assert list(ev[0, 10:]) == list(range(CH - 20, CH + 10))
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, 2))
    mat_desc = ~mat
    c = Case(gs, cuda, mat_desc, cols, U32, True)
    c.check(rows, 40, ARGS, plan=(3, 2))


# ------------------------------------------------------------------------------------------------- row stride --
@pytest.mark.parametrize("cols,k,path,levels", RR.STRIDE_SHAPES)
def test_row_stride_with_a_gap_that_would_win(gs, cuda, cols, k, path, levels):
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
            c.check(rows, k, mode, plan=(path, levels))
        assert torch.equal(c.d_keys, before_k) and torch.equal(c.d_vals, before_v)


# ----------------------------------------------------------------------------------------- buffers and reuse --
@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GUARDED_SHAPES)
def test_guarded_offset_dirty_buffers(gs, cuda, rows, cols, k, path, levels):
    """Every array in a slot of its own between guard zones, at byte offsets 4, 8, 12, ... from a 256-byte boundary (the
    workspace at an odd one), outputs and workspace dirty."""
    stride = cols + 3
    for i, mode in enumerate(MODES):
        kt, desc = (U32, I32, F32)[i], bool(i % 2)
        mat = matrix(rows, cols, kt, seed=90 + i, stride=stride)
        vals = values_for(mat.shape, seed=9)
        span = (rows - 1) * stride + cols
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
        assert gs.DeviceTopKRows.Plan(rows, cols, k, hv)[:2] == [path, levels]
        a = Arena(cuda, seed=i)
        a.add("keys_in", 4 * span, offset=4, data=mat.reshape(-1)[:span], const=True)
        a.add("vals_in", 4 * span, offset=12, data=vals.reshape(-1)[:span], const=True)
        a.add("keys_out", 4 * rows * k, offset=8, fill="random")
        a.add("vals_out", 4 * rows * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("temp", nb, offset=(1, 7, 130)[i], fill="random")
        a.build()
        rc = gs.lib.gs_topk_rows_u32(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                     a.ptr("vals_out") if hv else None, rows, cols, stride, k, int(desc), kt, None)
        assert rc == 0
        a.check()
        ek, ev = RR.rows_topk(mat, cols, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("keys_out", np.uint32).reshape(rows, k), ek), (mode, rows, cols, k)
        if hv:
            assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev), (mode, rows, cols, k)
        else:
            assert np.array_equal(a.read("vals_out", np.uint8), a.init["vals_out"])


def test_refused_calls_write_nothing(gs, cuda):
    rows, cols, k = 3, 9000, 10
    nb = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 4 * rows * cols, fill="random").add("keys_out", 4 * rows * k, fill="random")
    a.add("vals_out", 4 * rows * k, fill="random").add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), rows=rows, cols=cols,
                 stride=cols, k=k, kt=0)
        p.update(kw)
        return gs.lib.gs_topk_rows_u32(p["temp"], p["nb"], p["kin"], None, p["kout"], p["vout"], p["rows"], p["cols"], p["stride"], p["k"],
                                       0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=cols + 1), dict(k=1025), dict(stride=cols - 1), dict(kt=5),
               dict(kout=a.ptr("keys_in") + 4), dict(vout=a.ptr("keys_out") + 4 * (rows * k - 1)), dict(kin=a.ptr("keys_in") + 2)):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A chunked pairs call, a one-workgroup keys call and the first one again, on one stream and one workspace without a
    synchronisation between them: the third call's bytes equal the first's."""
    (rows, cols, k, _, _), second = RR.REUSE_SHAPES
    assert second[:3] == (6, 5000, 77)
    a = Case(gs, cuda, matrix(rows, cols, F32, seed=100), cols, F32, True)
    b = Case(gs, cuda, matrix(6, 5000, I32, seed=101), 5000, I32, False)
    nb = max(gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1), gs.lib.gs_topk_rows_temp_bytes(6, 5000, 77, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((rows * k,), -1, dtype=torch.int32, device=cuda), torch.full((rows * k,), -1, dtype=torch.int32, device=cuda))
            for _ in range(2)]
    kb = torch.full((6 * 77,), -1, dtype=torch.int32, device=cuda)

    def run_a(ko, vo):
        assert gs.lib.gs_topk_rows_u32(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), rows,
                                       cols, cols, k, 1, F32, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_rows_u32(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, 6, 5000, 5000, 77, 0, I32,
                                   None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    ek, ev = a.expect(rows, k, PAIRS)
    assert np.array_equal(host(outs[0][0]).reshape(rows, k), ek) and np.array_equal(host(outs[0][1]).reshape(rows, k), ev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert np.array_equal(host(kb).reshape(6, 77), b.expect(6, 77, KEYS)[0])


@pytest.mark.parametrize("rows,cols,k,path,levels", RR.GRAPH_SHAPES)
def test_topk_rows_is_capturable_in_a_hip_graph(gs, cuda, rows, cols, k, path, levels):
    """Captured once on one plain side stream (no parallel branches), replayed on new data in the same buffers."""
    sets = [matrix(rows, cols, U32, seed=110 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "five"))]
    src = dev(sets[0], cuda)
    ko = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
    nb = gs.DeviceTopKRows.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert gs.DeviceTopKRows.Plan(rows, cols, k, True)[:2] == [path, levels]
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.DeviceTopKRows.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gs.DeviceTopKRows.MaxPairs(temp, nb, src, ko, None, vo, rows, cols, cols, k, key_type=gs.GS_KEY_U32)
    for mat in sets:
        src.copy_(dev(mat, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev = RR.rows_topk(mat, cols, k, U32, True)
        assert np.array_equal(host(ko).reshape(rows, k), ek) and np.array_equal(host(vo).reshape(rows, k), ev)


# ------------------------------------------------------------------------------------------------- front ends --
def _distinct_floats(rows, cols, seed):
    rng = np.random.default_rng(seed)
    return np.stack([(rng.permutation(cols) - cols / 3).astype(np.float32) for _ in range(rows)])     # tie-free, NaN-free


@pytest.mark.parametrize("rows,cols,k", [(33, 100, 5), (4, 5000, 50), (3, 20000, 1000)])
def test_topk_rows_against_torch_topk(gs, cuda, rows, cols, k):
    wide = torch.from_numpy(_distinct_floats(rows, cols + 40, seed=cols)).to(cuda)
    for x in (wide[:, :cols].contiguous(), wide[:, 17:17 + cols]):        # the second: a non-contiguous row slice
        for largest in (False, True):
            want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
            ko, io = gs.topk_rows(x, k, largest=largest, indices=True)
            assert tuple(ko.shape) == (rows, k) and ko.dtype == x.dtype and io.dtype == torch.int32
            assert torch.equal(ko, want.values) and torch.equal(io.long(), want.indices)
            k2, none = gs.topk_rows(x, k, largest=largest)
            assert none is None and torch.equal(k2, want.values)
    vals = torch.arange(rows * (cols + 40), dtype=torch.int32, device=cuda).reshape(rows, cols + 40)
    x, v = wide[:, 3:3 + cols], vals[:, 3:3 + cols]
    ko, vo = gs.topk_rows(x, k, largest=True, values=v)
    want = torch.topk(x, k, dim=1, largest=True)
    assert torch.equal(ko, want.values) and torch.equal(vo, torch.gather(v, 1, want.indices))


def test_topk_rows_falls_back_to_the_flat_top_k_above_max_k(gs, cuda):
    rows, cols, k = 3, 6000, gs.DeviceTopKRows.MaxK() + 476
    assert gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1) == 0
    wide = torch.from_numpy(_distinct_floats(rows, cols + 8, seed=1)).to(cuda)
    copy = wide.clone()                                                  # the values: the keys again, in arrays of their own
    for x, v in ((wide[:, :cols].contiguous(), copy[:, :cols].contiguous()), (wide[:, 5:5 + cols], copy[:, 5:5 + cols])):
        want = torch.topk(x, k, dim=1, largest=True)
        ko, io = gs.topk_rows(x, k, largest=True, indices=True)
        assert torch.equal(ko, want.values) and torch.equal(io.long(), want.indices)
        ko, vo = gs.topk_rows(x, k, values=v)
        assert torch.equal(ko, torch.topk(x, k, dim=1, largest=False).values) and torch.equal(vo, ko)


def test_topk_rows_refusals(gs, cuda):
    x = torch.zeros((4, 100), dtype=torch.float32, device=cuda)
    with pytest.raises(ValueError):
        gs.topk_rows(x, 101)
    with pytest.raises(ValueError):
        gs.topk_rows(x.t(), 2)
    with pytest.raises(ValueError):
        gs.topk_rows(x[:, ::2], 2)
    with pytest.raises(ValueError):
        gs.topk_rows(x, 2, values=x, indices=True)
    with pytest.raises(ValueError):
        gs.topk_rows(x, 2, values=x[:, :50])
    with pytest.raises(TypeError):
        gs.topk_rows(x.double(), 2)
    with pytest.raises(gs.GpuSortError):
        out = torch.empty(4 * 2, dtype=torch.float32, device=cuda)
        tmp = torch.empty(256, dtype=torch.uint8, device=cuda)
        gs.DeviceTopKRows.MinKeys(tmp, 256, x, out, 4, 100, 50, 2)           # row_stride < num_cols
    ko, vo = gs.topk_rows(x, 0, indices=True)
    assert tuple(ko.shape) == (4, 0) and tuple(vo.shape) == (4, 0)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_rows_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 3 * 7 * 3 * 3
