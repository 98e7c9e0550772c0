"""gs_topk_rows_anyk_u16 without a device: the workspace query against the header's formula, the plan of every shape, every
refusal and no-op of the contract, what stays as it was at the 32-bit and the capped entry points, and the argument checks of
topk_rows_anyk16()."""
import ctypes as C

import numpy as np
import pytest

import topk_rows_anyk_narrow_ref as RN
from test_topk_rows_cpu import COLS as ROWS_COLS, ROWS

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
COLS = sorted(set(ROWS_COLS + RN.SLAB_EDGE_COLS))
U16, I16, F16, BF16 = RN.KEY_TYPES


def ks_of(cols):
    return [0, 1, 1024, 1025, 8192, 8193, cols, cols + 1]


def _tb(gs, rows, cols, k, hv):
    return gs.lib.gs_topk_rows_anyk_u16_temp_bytes(rows, cols, k, hv)


def _want_tb(gs, rows, cols, k, hv):
    if RN.refused(rows, cols, k) or 0 in (rows, cols, k):
        return 0
    return RN.temp_bytes(rows, cols, k, hv, gs.lib.gs_segmented_narrow_temp_bytes(rows * k, U16, 4 * hv, rows))


def _plan(gs, rows, cols, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    rc = gs.lib.gs_topk_rows_anyk_u16_plan(rows, cols, k, hv, out)
    return rc, list(out)


# --------------------------------------------------------------------------------------------- the size query --
def test_temp_bytes_is_the_headers_formula(gs):
    for rows in ROWS:
        for cols in COLS:
            for k in ks_of(cols):
                for hv in (0, 1):
                    got = _tb(gs, rows, cols, k, hv)
                    assert got % 256 == 0
                    assert got == _want_tb(gs, rows, cols, k, hv), (rows, cols, k, hv)
                    assert got <= gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv), (rows, cols, k, hv)
                    if k > cols or 0 in (rows, cols, k):
                        assert got == 0
                    elif not RN.refused(rows, cols, k):
                        assert got >= 2 * rows * k + 256
    # refused shapes return 0
    assert _tb(gs, 10, 100, 101, 0) == 0
    assert _tb(gs, 1 << 20, 1 << 12, 10, 0) == 0                 # rows * cols >= 2^32
    assert _tb(gs, 1 << 20, 2048, 2048, 1) == 0                  # rows * k >= 2^31
    assert _tb(gs, (1 << 20) - 1, 2048, 2048, 1) > 0
    assert _tb(gs, 100, 1 << 20, 5000, 1) > _tb(gs, 100, 1 << 20, 5000, 0)


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(rows, cols, k, hv, last):
        return last if RN.refused(rows, cols, k) else _tb(gs, rows, cols, k, hv)
    all_ks = sorted({k for cols in COLS[1:] for k in ks_of(cols) if k > 0})
    for hv in (0, 1):
        for rows in ROWS[1:]:
            for k in all_ks:
                last = 0
                for cols in [c for c in COLS if c >= k]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
            for cols in COLS[1:]:
                last = 0
                for k in [x for x in all_ks if x <= cols]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
        for cols in COLS[1:]:
            for k in [x for x in all_ks if x <= cols]:
                last = 0
                for rows in ROWS[1:]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
        for k in (1, 1025, 8000):        # fine steps around the path edge and the slab edges
            last = 0
            for cols in list(range(8100, 8300, 3)) + list(range(RN.SLAB - 50, RN.SLAB + 50)) + list(range(2 * RN.SLAB - 9, 2 * RN.SLAB + 9)):
                b = tb(5, cols, k, hv, last)
                assert b >= last, (cols, k)
                last = b
    for rows, cols, k in ((5, 20000, 3000), (300, 9000, 1100), (2, 1 << 20, 70000)):
        assert _tb(gs, rows, cols, k, 1) >= _tb(gs, rows, cols, k, 0)


# --------------------------------------------------------------------------------------------------- the plan --
def test_plan_is_the_reference_plan(gs):
    rc, p = _plan(gs, 3, 100000, 2000)
    assert rc == 0 and p[3] * p[4] == RN.SLAB and p[2] == RN.CH and p[3] == RN.TILE      # the tables of the reference module
    assert p[:2] == [2, 9] and _plan(gs, 3, 8000, 2000)[1][:2] == [1, 2]
    wide = (C.c_uint32 * 8)()
    for rows in ROWS:
        for cols in COLS:
            for k in ks_of(cols):
                want = RN.plan(rows, cols, k)
                for hv in (0, 1):
                    rc, got = _plan(gs, rows, cols, k, hv)
                    if want is None:
                        assert rc == INVALID and got == [0] * 8, (rows, cols, k)
                    else:
                        assert rc == 0 and got == want, (rows, cols, k, got, want)
                        assert gs.lib.gs_topk_rows_anyk_plan(rows, cols, k, hv, wide) == 0
                        assert got[2:7] == list(wide)[2:7] and got[0] == wide[0]      # the geometry words are the 32-bit call's
    assert _plan(gs, 1, 8192, 5000)[1][0] == 1 and _plan(gs, 1, 8193, 5000)[1][0] == 2        # path 1 up to 8192 columns
    assert _plan(gs, 1 << 20, 1 << 12, 10) == (INVALID, [0] * 8)
    assert gs.lib.gs_topk_rows_anyk_u16_plan(1, 1, 1, 0, None) == INVALID
    assert gs.DeviceTopKRowsAnyK16.Plan(3, 20000, 5000) == RN.plan(3, 20000, 5000)
    assert gs.DeviceTopKRowsAnyK.Plan(3, 20000, 5000)[1] == 11                               # the 32-bit class keeps its own


def test_plan_of_every_gpu_shape(gs):
    for cols in RN.PATH1_COLS:
        for k in RN.path1_ks(cols):
            assert 1 <= k <= cols and _plan(gs, 7, cols, k)[1][0] == 1
    for cols in RN.PATH2_COLS:
        for k in RN.path2_ks(cols):
            p = _plan(gs, 3, cols, k)[1]
            assert 1 <= k <= cols and p[0] == 2 and p[6] == -(-cols // RN.TILE) and p[5] == -(-cols // RN.SLAB)
    assert [_plan(gs, 1, c, 1)[1][5] for c in RN.PATH2_COLS] == [1, 1, 1, 2, 3, 4]
    assert _plan(gs, *RN.MANY_ROWS)[1][5] == 1 and _plan(gs, *RN.MANY_ROWS)[1][6] == 2
    for rows, cols, k, path in RN.GUARDED_SHAPES + RN.GRAPH_SHAPES + RN.REUSE_SHAPES:
        assert _plan(gs, rows, cols, k)[1][0] == path and k > 1024
    for cols, k, path in RN.STRIDE_SHAPES:
        assert _plan(gs, 5, cols, k)[1][0] == path
    for rows, cols, path in RN.AGREE_SHAPES:
        assert _plan(gs, rows, cols, 3000)[1][0] == path
    assert RN.LONG_COLS > 65536 and _plan(gs, 2, RN.LONG_COLS, 40000)[1][0] == 2
    # the finish's one-workgroup class ends at 8192 elements, with and without values
    assert gs.lib.gs_segmented_narrow_cap(U16, 4) == 8192 == gs.lib.gs_segmented_narrow_cap(U16, 0)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc=0, kt=BF16):
    return gs.lib.gs_topk_rows_anyk_u16(temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc, kt, None)


@pytest.mark.parametrize("cols", [5000, 20000])
def test_refusals_and_noops_without_a_device(gs, cols):
    rows, stride, k = 50, cols + 3, 2000
    need = _tb(gs, rows, cols, k, 1)
    assert need > 0
    span = (rows - 1) * stride + cols
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 26), BASE + (2 << 26), BASE + (3 << 26), BASE + (4 << 26)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, rows=rows, cols=cols, stride=stride, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0), # too small
        dict(k=cols + 1),                              # k > num_cols
        dict(stride=cols - 1),                         # row_stride < num_cols
        dict(rows=1 << 20, stride=1 << 12, cols=700, k=100),  # num_rows * row_stride >= 2^32
        dict(rows=(1 << 32) // stride + 1),
        dict(rows=1 << 20, cols=2048, stride=2048, k=2048),   # num_rows * k >= 2^31
        dict(rows=1 << 31, cols=1, stride=1, k=1),
        dict(kt=0), dict(kt=1), dict(kt=2), dict(kt=3), dict(kt=-1), dict(kt=6), dict(kt=7), dict(kt=12),   # other key types
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 1), dict(kin=kin + 3), dict(kout=kout + 1),          # a key pointer at an odd address
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 3), dict(vout=vout + 1),   # a value pointer at 2 mod 4, at an odd address
        dict(kout=kin), dict(kout=kin + 2 * (span - 1)),   # output inside the keys
        dict(vout=kin + 2 * 10), dict(vout=vin), dict(kout=vin + 4 * (span - 1) + 2),
        dict(vout=kout), dict(vout=kout + 2 * (rows * k - 2)), dict(kout=vout + 4 * (rows * k - 1) + 2),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + ((2 * (span - 2)) & ~3)),     # inputs share a byte
    ]
    for change in bad:
        assert _call(gs, **dict(ok, **change)) == INVALID, change
    # an output in the last row's stride gap, or right behind 2-byte keys, shares nothing: refused only for the workspace
    assert _call(gs, **dict(ok, kout=kin + 2 * span, temp_bytes=need - 1)) == INVALID
    assert _call(gs, **dict(ok, vout=kout + 2 * rows * k, temp_bytes=need - 1)) == INVALID
    need0 = _tb(gs, rows, cols, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    for kt in RN.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, cols, stride, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 1) == INVALID          # k > num_cols, even for empty rows
    assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, 0, 2) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, 0, cols, cols - 1, k) == INVALID   # a short stride before the no-op
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_rows_anyk_u16_status(None, rows, cols, k, 1, 0, out, None) == INVALID and list(out) == [0] * 8
    assert gs.lib.gs_topk_rows_anyk_u16_status(temp, rows, cols, k, 1, rows, out, None) == INVALID       # no such row
    assert gs.lib.gs_topk_rows_anyk_u16_status(None, rows, cols, 0, 1, 0, out, None) == 0 and list(out) == [0] * 8


def test_a_key_pointer_at_2_mod_4_and_an_odd_stride_pass_the_checks(gs):
    """Both are served: with everything else in order the only refusal left is the workspace's."""
    rows, cols, k = 5, 9001, 1500
    need = _tb(gs, rows, cols, k, 1)
    kin, vin, kout, vout, temp = BASE + 2, BASE + (1 << 26), BASE + (2 << 26) + 2, BASE + (3 << 26), BASE + (4 << 26) + 1
    assert _call(gs, temp, need - 1, kin, vin, kout, vout, rows, cols, cols + 2, k) == INVALID
    assert _call(gs, temp, need, kin + 1, vin, kout, vout, rows, cols, cols + 2, k) == INVALID


def test_the_other_entry_points_stay_as_they_were(gs):
    rows, cols, k = 4, 5000, 2000
    need = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 0)
    for kt in RN.KEY_TYPES:        # gs_topk_rows_anyk_u32 still refuses the 16-bit key types
        assert gs.lib.gs_topk_rows_anyk_u32(BASE + (4 << 26), need, BASE, None, BASE + (2 << 26), None, rows, cols, cols, k, 0, kt, None) == INVALID
    assert gs.lib.gs_topk_rows_u16_temp_bytes(10, 5000, 1025, 0) == 0 and gs.lib.gs_topk_rows_u16_temp_bytes(10, 50000, 1025, 1) == 0
    assert gs.lib.gs_topk_rows_u16(BASE + (4 << 26), 1 << 20, BASE, None, BASE + (2 << 26), None, 10, 5000, 5000, 1025, 0, BF16, None) == INVALID
    assert gs.lib.gs_topk_rows_u16_temp_bytes(10, 50000, 1024, 1) > 0
    assert gs.lib.gs_topk_rows_max_k() == 1024 == gs.DeviceTopKRows.MaxK()
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_rows_anyk_plan(3, 100000, 2000, 0, out) == 0 and list(out)[:2] == [2, 11]


# ------------------------------------------------------------------------------------------------ front ends --
def test_size_query_phase_and_exports(gs):
    rows, cols, k = 40, 30000, 2000
    front = gs.DeviceTopKRowsAnyK16
    for kt in (None, gs.GS_KEY_F16):
        for fn in (front.MinKeys, front.MaxKeys):
            assert fn(None, 0, None, None, rows, cols, cols, k, key_type=kt) == _tb(gs, rows, cols, k, 0) > 256
        for fn in (front.MinPairs, front.MaxPairs):
            assert fn(None, 0, None, None, None, None, rows, cols, cols, k, key_type=kt) == _tb(gs, rows, cols, k, 1)
    assert front.MinKeys(None, 0, None, None, rows, cols, cols, cols + 1) == 0
    with pytest.raises(TypeError):
        front.MinKeys(None, 0, None, None, rows, cols, cols, k, key_type=gs.GS_KEY_F32)
    assert issubclass(front, gs.DeviceTopKRowsAnyK) and not hasattr(front, "MaxK")
    assert sorted(a for a in dir(front) if not a.startswith("_")) == ["MaxKeys", "MaxPairs", "MinKeys", "MinPairs", "Plan", "Status"]
    assert callable(gs.topk_rows_anyk16) and "DeviceTopKRowsAnyK16" in gs.__all__ and "topk_rows_anyk16" in gs.__all__


def test_topk_rows_anyk16_argument_checks_need_no_device(gs):
    import torch
    t = torch.zeros((4, 3000), dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t, 3001)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t, 2000, values=torch.zeros((4, 3000), dtype=torch.int32), indices=True)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t.reshape(-1), 2)                             # not 2-D
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t.t(), 2)                                     # the last dimension is not contiguous
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t[:, ::2], 2)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t, 2, values=torch.zeros((4, 2999), dtype=torch.int32))
    with pytest.raises(ValueError):
        gs.topk_rows_anyk16(t, 2, values=torch.zeros((4, 3000), dtype=torch.int16))      # 2-byte values
    for dtype in (torch.int32, torch.float32, torch.int64, torch.uint8):
        with pytest.raises(TypeError):
            gs.topk_rows_anyk16(torch.zeros((4, 3000), dtype=dtype), 2000)
    for dtype in (torch.int16, torch.uint16, torch.float16, torch.bfloat16):
        ko, vo = gs.topk_rows_anyk16(torch.zeros((4, 3000), dtype=dtype), 0, indices=True)
        assert tuple(ko.shape) == (4, 0) and tuple(vo.shape) == (4, 0) and ko.dtype == dtype and vo.dtype == torch.int32
    ko, vo = gs.topk_rows_anyk16(t[:0], 2000)                             # k above 1024 is no ValueError here
    assert tuple(ko.shape) == (0, 2000) and vo is None


def test_the_capped_front_ends_keep_their_errors(gs):
    import torch
    with pytest.raises(ValueError):
        gs.topk_rows(torch.zeros((4, 3000), dtype=torch.float16), 2000)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(torch.zeros((4, 3000), dtype=torch.float16), 2000)
    with pytest.raises(TypeError):
        gs.topk_rows_anyk(torch.zeros((4, 3000), dtype=torch.bfloat16), 2000)


def test_status_reference_on_a_small_row():
    keys = np.array([5, 5, 1, 9, 5, 0], np.uint16)
    assert RN.status(keys, 4, RN.U16) == [1, 5, 2, 2, 0, 0, 0, 0]
    assert RN.status(keys, 1, RN.U16, True) == [1, 0xFFFF - 9, 0, 1, 0, 0, 0, 0]
    long = np.arange(9000, dtype=np.uint16)
    assert RN.status(long, 300, RN.U16) == [2, 299, 299, 1, 256, 0, 0, 0]
