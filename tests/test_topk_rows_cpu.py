"""gs_topk_rows_u32 without a device: the per-row reference against the CPU oracle, the numpy model of the chunked scheme
against the reference, every refusal and no-op of the contract, the workspace query against the header's formula, the plan
of every shape the GPU file runs, and the size-query phase of the Python front end."""
import ctypes as C

import numpy as np
import pytest

import topk_ref as R
import topk_rows_ref as RR

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U32, I32, F32 = R.U32, R.I32, R.F32


def _special_f32():
    tiny = np.finfo(np.float32).smallest_subnormal
    sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5, np.nan, -np.nan], np.float32).view(np.uint32)
    return np.concatenate([sp, np.array([0x7FC00001, 0xFFC00002], np.uint32)])


# ------------------------------------------------------------------------------------------------ the reference --
@pytest.mark.parametrize("descending", [False, True])
def test_row_reference_matches_oracle_ranks(oracle, descending):
    rng = np.random.default_rng(11)
    rows, cols, stride = 6, 333, 340
    mat = rng.integers(0, 1 << 32, (rows, stride), dtype=np.uint64).astype(np.uint32)
    mat[:, :cols][rng.random((rows, cols)) < 0.3] = 77           # ties: stability shows
    vals = rng.integers(0, 1 << 32, (rows, stride), dtype=np.uint64).astype(np.uint32)
    for k in (1, 100, cols):
        ko, co = RR.rows_topk(mat, cols, k, U32, descending)
        kv, vo = RR.rows_topk(mat, cols, k, U32, descending, vals)
        for r in range(rows):
            want = oracle.lsb_reference_ranks(np.ascontiguousarray(mat[r, :cols]), 0, 32, descending)[:k]
            assert np.array_equal(co[r], want) and np.array_equal(ko[r], mat[r, want])
            assert np.array_equal(kv[r], ko[r]) and np.array_equal(vo[r], vals[r, want])


def _model_inputs(rng, n, kind, kt):
    if kind == "uniform":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "equal":
        k = np.full(n, 0x3F800000, np.uint32)
    elif kind == "three":
        k = np.array([5, 0x80000001, 0xFFFFFFF0], np.uint32)[rng.integers(0, 3, n)]
    elif kind == "topbyte":
        k = rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32) | np.uint32(0x42000000)
    else:
        sp = _special_f32() if kt == F32 else np.array([0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000], np.uint32)
        k = sp[rng.integers(0, sp.size, n)]
    return k


def test_chunk_model_matches_the_reference():
    """300 random cases: CH 8..64, k <= CH / 2, n up to three levels and more; ties, one shared top byte, specials, all key
    types, both directions, with and without carried columns."""
    rng = np.random.default_rng(2024)
    kinds = ("uniform", "equal", "three", "topbyte", "special")
    deepest = 0
    for case in range(300):
        ch = int(rng.integers(8, 65))
        k = int(rng.integers(1, ch // 2 + 1))
        n = int(rng.integers(max(k, 1), ch * 12))
        kt, desc, kind = case % 3, bool((case // 3) % 2), kinds[case % 5]
        keys = _model_inputs(rng, n, kind, kt)
        ek, ev, _ = R.topk(keys, k, kt, desc)
        mk, mc, levels = RR.chunk_model(keys, k, kt, desc, ch)
        assert np.array_equal(mk, ek) and np.array_equal(mc, ev), (case, ch, k, n, kt, desc, kind)
        mk0, none, _ = RR.chunk_model(keys, k, kt, desc, ch, carry_columns=False)
        assert none is None and np.array_equal(mk0, ek)
        assert levels == len(RR.level_sizes(n, k, ch))
        deepest = max(deepest, levels)
    assert deepest >= 3


def test_chunk_model_tie_run_across_a_chunk_boundary():
    ch, k = 16, 6
    keys = np.full(40, 9, np.uint32)
    keys[[3, 20]] = 1                       # two smaller keys, then the tie run of 9s from column 0 on, across chunks
    mk, mc, _ = RR.chunk_model(keys, k, U32, False, ch)
    assert list(mk) == [1, 1, 9, 9, 9, 9] and list(mc) == [3, 20, 0, 1, 2, 4]
    mk, mc, _ = RR.chunk_model(np.full(40, 9, np.uint32), k, U32, True, ch)
    assert list(mc) == list(range(k))


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc=0, kt=0):
    return gs.lib.gs_topk_rows_u32(temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc, kt, None)


@pytest.mark.parametrize("cols", [700, 5000, 20000])
def test_refusals_and_noops_without_a_device(gs, cols):
    rows, stride, k = 50, cols + 3, 100
    need = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1)
    assert need > 0
    span = (rows - 1) * stride + cols
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 26), BASE + (2 << 26), BASE + (3 << 26), BASE + (4 << 26)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, rows=rows, cols=cols, stride=stride, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0), # too small
        dict(k=cols + 1),                              # k > num_cols
        dict(k=1025, cols=max(cols, 2000), stride=max(cols, 2000)),   # k > max_k
        dict(stride=cols - 1),                         # row_stride < num_cols
        dict(rows=1 << 20, stride=1 << 12, cols=700),  # num_rows * row_stride >= 2^32
        dict(rows=(1 << 32) // stride + 1),
        dict(rows=1 << 23, cols=700, stride=700, k=512),   # num_rows * k >= 2^32 (k <= row_stride: rows * stride too)
        dict(rows=1 << 32, cols=1, stride=1, k=1),
        dict(kt=3), dict(kt=-1), dict(kt=6), dict(kt=12),   # key types other than U32 / I32 / F32
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 2), dict(kout=kout + 1), dict(vin=vin + 3), dict(vout=vout + 2),   # misaligned arrays
        dict(kout=kin), dict(kout=kin + 4 * (span - 1)),   # output inside the keys
        dict(vout=kin + 4 * 10), dict(vout=vin), dict(kout=vin + 4 * (span - 1)),
        dict(vout=kout), dict(vout=kout + 4 * (rows * k - 1)), dict(kout=vout + 4 * (rows * k - 1)),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 4 * (span - 1)),     # inputs share a byte
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # an output in the last row's stride gap shares nothing: refused only for the workspace, accepted as far as the checks go
    assert _call(gs, **dict(ok, kout=kin + 4 * span, temp_bytes=need - 1)) == INVALID
    # the arguments and keys-only forms size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed
    for kt in (0, 1, 2):
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, cols, stride, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, rows, cols, stride, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 1) == INVALID          # k > num_cols, even for empty rows
    assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, 0, 7) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, 0, cols, cols - 1, k) == INVALID   # a short stride before the no-op


def test_max_k(gs):
    assert gs.lib.gs_topk_rows_max_k() >= 1024
    assert gs.lib.gs_topk_rows_max_k() == RR.MAX_K == gs.DeviceTopKRows.MaxK()


# --------------------------------------------------------------------------------------------- the size query --
COLS = [0, 1, 2, 64, 65, 1024, 1025, 8191, 8192, 8193, 8197, 16384, 16385, 65536, 65537, 151936, 1 << 20, (1 << 23) + 9]
KS = [0, 1, 2, 8, 64, 65, 1000, 1023, 1024]
ROWS = [0, 1, 3, 7, 256, 1000]


def test_temp_bytes_is_the_headers_formula(gs):
    for rows in ROWS:
        for cols in COLS:
            for k in KS + [1025, cols + 1]:
                for hv in (0, 1):
                    got = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
                    assert got % 256 == 0
                    assert got == RR.temp_bytes(rows, cols, k, hv), (rows, cols, k, hv)
    # refused shapes return 0
    assert gs.lib.gs_topk_rows_temp_bytes(10, 100, 101, 0) == 0
    assert gs.lib.gs_topk_rows_temp_bytes(10, 5000, 1025, 0) == 0
    assert gs.lib.gs_topk_rows_temp_bytes(1 << 20, 1 << 12, 10, 0) == 0
    assert gs.lib.gs_topk_rows_temp_bytes(1 << 23, 700, 512, 1) == 0
    # paths 1 and 2 copy nothing into the workspace
    assert gs.lib.gs_topk_rows_temp_bytes(1 << 20, 256, 8, 1) == 256 and gs.lib.gs_topk_rows_temp_bytes(1000, 8192, 1024, 1) == 256


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(rows, cols, k, hv):
        return last if RR.refused(rows, cols, k) else gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
    for hv in (0, 1):
        for rows in ROWS[1:]:
            for k in KS[1:]:
                last = 0
                for cols in [c for c in COLS if c >= k]:
                    b = tb(rows, cols, k, hv)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
            for cols in COLS[1:]:
                last = 0
                for k in [x for x in KS[1:] if x <= cols]:
                    b = tb(rows, cols, k, hv)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
        for cols in COLS[1:]:
            for k in [x for x in KS[1:] if x <= cols]:
                last = 0
                for rows in ROWS[1:]:
                    b = tb(rows, cols, k, hv)
                    assert b >= last
                    last = b
        # fine steps around the chunk edges
        for k in (1, 100, 1024):
            last = 0
            for cols in list(range(8100, 8300, 3)) + list(range(16300, 16500, 3)) + list(range(65500, 65600)):
                b = tb(5, cols, k, hv)
                assert b >= last, (cols, k)
                last = b
    last = 0
    assert tb(100, 1 << 20, 100, 1) > tb(100, 1 << 20, 100, 0)


# --------------------------------------------------------------------------------------------------- the plan --
def _plan(gs, rows, cols, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    rc = gs.lib.gs_topk_rows_plan(rows, cols, k, hv, out)
    return rc, list(out)


def test_plan_is_the_reference_plan(gs):
    for rows in ROWS:
        for cols in COLS:
            for k in KS + [1025, cols + 1]:
                want = RR.plan(rows, cols, k)
                rc, got = _plan(gs, rows, cols, k)
                if want is None:
                    assert rc == INVALID and got == [0] * 8, (rows, cols, k)
                else:
                    assert rc == 0 and got == want, (rows, cols, k, got, want)
    assert _plan(gs, 1 << 20, 1 << 12, 10) == (INVALID, [0] * 8)
    assert gs.lib.gs_topk_rows_plan(1, 1, 1, 0, None) == INVALID
    assert gs.DeviceTopKRows.Plan(3, 20000, 50) == RR.plan(3, 20000, 50)


def test_plan_of_every_gpu_shape(gs):
    """What each shape of tests/test_topk_rows_gpu.py is meant to exercise, asserted with the plan alone."""
    assert _plan(gs, 1, 1, 1)[1][2] == RR.CH
    for cols in RR.PATH1_COLS:
        for k in RR.path1_ks(cols):
            for rows in RR.PATH1_ROWS:
                assert _plan(gs, rows, cols, k)[1][:2] == [1, 1]
    for cols in RR.PATH2_COLS:
        for k in RR.PATH2_KS:
            for rows in RR.PATH2_ROWS:
                assert _plan(gs, rows, cols, k)[1][:2] == [2, 1]
    for rows, cols, k, levels in RR.PATH3_SHAPES:
        rc, p = _plan(gs, rows, cols, k)
        assert rc == 0 and p[:2] == [3, levels] and p[3] == -(-cols // RR.CH), (rows, cols, k, p)
        assert rows * cols <= 1 << 22
    for rows, cols, k, levels in RR.MIDDLE_SHAPES:      # the smallest rows of three levels in their class: one column fewer has two
        assert _plan(gs, rows, cols, k)[1][:2] == [3, 3] and _plan(gs, rows, cols - 1, k)[1][:2] == [3, 2], (cols, k)
        assert _plan(gs, rows, cols, k)[1][4] == RR.CH + 1 and levels == 3
    assert sorted(-(-k // 64) for _, _, k, _ in RR.MIDDLE_SHAPES) == [1, 4, 8]
    for cols, k, path, levels in RR.STRIDE_SHAPES:
        assert _plan(gs, 5, cols, k)[1][:2] == [path, levels], (cols, k)
    for rows, cols, k, path, levels in RR.GUARDED_SHAPES + RR.GRAPH_SHAPES + RR.REUSE_SHAPES:
        assert _plan(gs, rows, cols, k)[1][:2] == [path, levels], (rows, cols, k)
    # CH + 5 at k = 1024: the last chunk gives fewer than k
    assert _plan(gs, 2, RR.CH + 5, 1024)[1][4] == 1024 + 5
    assert _plan(gs, 3, RR.THREE_LEVELS_COLS, 1024)[1][4] == 8 * 1024 + 1


# ------------------------------------------------------------------------------------------------ front ends --
def test_device_topk_rows_size_query_phase(gs):
    """d_temp_storage=None returns the size and touches nothing: no tensor is needed."""
    rows, cols, k = 40, 30000, 200
    for fn in (gs.DeviceTopKRows.MinKeys, gs.DeviceTopKRows.MaxKeys):
        assert fn(None, 0, None, None, rows, cols, cols, k) == gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 0) > 256
    for fn in (gs.DeviceTopKRows.MinPairs, gs.DeviceTopKRows.MaxPairs):
        assert fn(None, 0, None, None, None, None, rows, cols, cols, k) == gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1)
    assert gs.DeviceTopKRows.MinKeys(None, 0, None, None, rows, cols, cols, 2000) == 0      # refused: k > max_k
    assert callable(gs.topk_rows) and "DeviceTopKRows" in gs.__all__ and "topk_rows" in gs.__all__


def test_topk_rows_argument_checks_need_no_device(gs):
    import torch
    t = torch.zeros((4, 10), dtype=torch.int32)
    with pytest.raises(ValueError):
        gs.topk_rows(t, 11)
    with pytest.raises(ValueError):
        gs.topk_rows(t, 2, values=t, indices=True)
    with pytest.raises(ValueError):
        gs.topk_rows(t.reshape(-1), 2)
    with pytest.raises(ValueError):
        gs.topk_rows(t.t(), 2)                                       # the last dimension is not contiguous
    with pytest.raises(ValueError):
        gs.topk_rows(t, 2, values=torch.zeros((4, 9), dtype=torch.int32))
    with pytest.raises(TypeError):
        gs.topk_rows(torch.zeros((4, 10), dtype=torch.int64), 2)
    ko, vo = gs.topk_rows(t, 0, indices=True)
    assert tuple(ko.shape) == (4, 0) and tuple(vo.shape) == (4, 0)
