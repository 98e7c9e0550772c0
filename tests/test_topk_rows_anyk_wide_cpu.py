"""gs_topk_rows_anyk_u64 without a device: the workspace query against the header's formula, the plan of every shape, every
refusal and no-op of the contract in the stated order, what stays as it was at the capped and the 32-bit entry points, the
argument checks of topk_rows_anyk64(), and every builder of tests/topk_rows_anyk_wide_ref.py held to its intent by the host
model of the descent."""
import ctypes as C

import numpy as np
import pytest

import topk_rows_anyk_wide_ref as RA

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
ROWS = [0, 1, 3, 300]
COLS = RA.SIZE_COLS
U64, I64, F64 = RA.KEY_TYPES


def ks_of(cols):
    return [0] + RA.size_ks(cols) + [cols + 1]


def _tb(gs, rows, cols, k, hv):
    return gs.lib.gs_topk_rows_anyk_u64_temp_bytes(rows, cols, k, hv)


def _want_tb(gs, rows, cols, k, hv):
    if RA.refused(rows, cols, k) or 0 in (rows, cols, k):
        return 0
    return RA.temp_bytes(rows, cols, k, hv, gs.lib.gs_segmented_wide_temp_bytes(rows * k, 8, 4 * hv, rows))


def _plan(gs, rows, cols, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    rc = gs.lib.gs_topk_rows_anyk_u64_plan(rows, cols, k, hv, out)
    return rc, list(out)


# --------------------------------------------------------------------------------------------- the size query --
def test_temp_bytes_is_the_headers_formula(gs):
    assert COLS == [1, 1024, 1025, 8191, 8192, 8193, RA.SLAB - 1, RA.SLAB, RA.SLAB + 1, 65536, 151936]
    for rows in ROWS:
        for cols in COLS:
            for k in ks_of(cols):
                for hv in (0, 1):
                    got = _tb(gs, rows, cols, k, hv)
                    assert got % 256 == 0
                    assert got == _want_tb(gs, rows, cols, k, hv), (rows, cols, k, hv)
                    if k > cols or 0 in (rows, cols, k):
                        assert got == 0
                    else:
                        assert got >= 8 * rows * k + 256
    assert _tb(gs, 10, 100, 101, 0) == 0
    assert _tb(gs, 1 << 20, 1 << 12, 10, 0) == 0                 # rows * cols >= 2^32
    assert _tb(gs, 1 << 20, 2048, 2048, 1) == 0                  # rows * k >= 2^31
    assert _tb(gs, (1 << 20) - 1, 2048, 2048, 1) > 0
    assert _tb(gs, 100, 1 << 20, 5000, 1) > _tb(gs, 100, 1 << 20, 5000, 0)


def test_the_list_term_follows_l(gs):
    assert [RA.list_cap(c) for c in (8193, 65535, 65536, 1 << 20)] == [1024, 8191, 8192, 8192]
    rows, k = 3, 2000
    for cols in (8193, 65535, 65536, 1 << 20):
        L = RA.list_cap(cols)
        assert _plan(gs, rows, cols, k)[1][7] == L
        tiles = -(-cols // RA.TILE)
        seg = gs.lib.gs_segmented_wide_temp_bytes(rows * k, 8, 0, rows)
        a = RA._a
        assert _tb(gs, rows, cols, k, 0) == (a(64 * rows) + a(4 * (rows + 1)) + a(4 * 2048 * rows) + a(8 * rows * tiles) + a(8 * L * rows)
                                             + a(8 * rows * k) + a(seg) + 256)
        assert 8 * L * rows <= max(8 * cols * rows // 8, 8 * 1024 * rows)     # an eighth of the dense matrix (1024 at least)
    assert _plan(gs, rows, 8192, k)[1][7] == 0


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(rows, cols, k, hv, last):
        return last if RA.refused(rows, cols, k) else _tb(gs, rows, cols, k, hv)
    all_ks = sorted({k for cols in COLS for k in RA.size_ks(cols)})
    for hv in (0, 1):
        for rows in ROWS[1:]:
            for k in all_ks:
                last = 0
                for cols in [c for c in COLS if c >= k]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
            for cols in COLS:
                last = 0
                for k in [x for x in all_ks if x <= cols]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
        for cols in COLS:
            for k in [x for x in all_ks if x <= cols]:
                last = 0
                for rows in ROWS[1:]:
                    b = tb(rows, cols, k, hv, last)
                    assert b >= last, (rows, cols, k, hv)
                    last = b
        for k in (1, 1025, 8000):        # fine steps around the path edge, the slab edge and where L starts to grow and stops
            last = 0
            for cols in list(range(8100, 8300, 3)) + list(range(RA.SLAB - 50, RA.SLAB + 50)) + list(range(65500, 65600, 7)):
                b = tb(5, cols, k, hv, last)
                assert b >= last, (cols, k)
                last = b
    for rows, cols, k in ((5, 20000, 3000), (300, 9000, 1100), (2, 1 << 20, 70000)):
        assert _tb(gs, rows, cols, k, 1) >= _tb(gs, rows, cols, k, 0)


# --------------------------------------------------------------------------------------------------- the plan --
def test_plan_is_the_reference_plan(gs):
    rc, p = _plan(gs, 3, 100000, 2000)
    assert rc == 0 and p[3] * p[4] == RA.SLAB and p[2] == RA.CH and p[3] == RA.TILE      # the tables of the reference module
    assert p[:2] == [2, 19] and p[7] == 8192 and _plan(gs, 3, 8000, 2000)[1] == [1, 2, 8192, 8192, 1, 1, 1, 0]
    narrow = (C.c_uint32 * 8)()
    for rows in ROWS:
        for cols in COLS:
            for k in ks_of(cols):
                want = RA.plan(rows, cols, k)
                for hv in (0, 1):
                    rc, got = _plan(gs, rows, cols, k, hv)
                    if want is None:
                        assert rc == INVALID and got == [0] * 8, (rows, cols, k)
                    else:
                        assert rc == 0 and got == want, (rows, cols, k, got, want)
                        assert gs.lib.gs_topk_rows_anyk_plan(rows, cols, k, hv, narrow) == 0
                        assert got[2:7] == list(narrow)[2:7] and got[0] == narrow[0]      # the geometry words are the 32-bit call's
    assert _plan(gs, 1, 8192, 5000)[1][0] == 1 and _plan(gs, 1, 8193, 5000)[1][0] == 2        # path 1 up to 8192 columns
    assert _plan(gs, 1 << 20, 1 << 12, 10) == (INVALID, [0] * 8)
    assert gs.lib.gs_topk_rows_anyk_u64_plan(1, 1, 1, 0, None) == INVALID
    assert gs.DeviceTopKRowsAnyK64.Plan(3, 20000, 5000) == RA.plan(3, 20000, 5000)
    assert gs.DeviceTopKRowsAnyK.Plan(3, 20000, 5000)[1] == 11 and gs.DeviceTopKRowsAnyK16.Plan(3, 20000, 5000)[1] == 9


def test_plan_of_every_gpu_shape(gs):
    for cols in RA.PATH1_COLS:
        for k in RA.path1_ks(cols):
            assert 1 <= k <= cols and _plan(gs, 7, cols, k)[1][0] == 1
    for cols in RA.PATH2_COLS:
        for k in RA.path2_ks(cols):
            p = _plan(gs, 3, cols, k)[1]
            assert 1 <= k <= cols and p[0] == 2 and p[6] == -(-cols // RA.TILE) and p[5] == -(-cols // RA.SLAB)
    assert [_plan(gs, 1, c, 1)[1][5] for c in RA.PATH2_COLS] == [1, 1, 1, 2, 3, 4]
    assert _plan(gs, *RA.MANY_ROWS)[1][5] == 1 and _plan(gs, *RA.MANY_ROWS)[1][6] == 2
    for rows, cols, k, path in RA.GUARDED_SHAPES + RA.GRAPH_SHAPES + RA.REUSE_SHAPES:
        assert _plan(gs, rows, cols, k)[1][0] == path and k > 1024
    for cols, k, path in RA.STRIDE_SHAPES:
        assert _plan(gs, 5, cols, k)[1][0] == path
    for rows, cols, path in RA.AGREE_SHAPES:
        assert _plan(gs, rows, cols, 3000)[1][0] == path
    assert _plan(gs, 1, RA.DEEP_COLS, 5)[1][7] == 3072


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc=0, kt=F64):
    return gs.lib.gs_topk_rows_anyk_u64(temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc, kt, None)


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
        dict(kt=0), dict(kt=1), dict(kt=2), dict(kt=-1), dict(kt=6), dict(kt=7), dict(kt=9), dict(kt=12),   # other key types
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 4), dict(kout=kout + 4), dict(kin=kin + 1), dict(kout=kout + 2),     # a key pointer at 4 mod 8, and worse
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 3), dict(vout=vout + 1),     # a value pointer not at 0 mod 4
        dict(kout=kin), dict(kout=kin + 8 * (span - 1)),   # output inside the keys
        dict(vout=kin + 8 * 10), dict(vout=vin), dict(kout=vin + 4 * (span - 2)),
        dict(vout=kout), dict(vout=kout + 8 * (rows * k - 1) + 4), dict(kout=vout + 4 * (rows * k - 2)),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 8 * (span - 1) + 4),          # inputs share a byte
    ]
    for change in bad:
        assert _call(gs, **dict(ok, **change)) == INVALID, change
    # the stated order: a shape refusal comes before the key type, the key type before the pointers, a no-op before the pointers
    assert _call(gs, **dict(ok, k=cols + 1, kt=0, kin=None)) == INVALID
    assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, 0, 2) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, 0, cols, cols - 1, k) == INVALID   # a short stride before the no-op
    assert _call(gs, None, 0, None, vin, None, None, rows, cols, stride, 0) == INVALID   # values in without values out before the no-op
    # an output in the last row's stride gap, or right behind the keys, shares nothing: refused only for the workspace
    assert _call(gs, **dict(ok, kout=kin + 8 * span, temp_bytes=need - 1)) == INVALID
    assert _call(gs, **dict(ok, vout=kout + 8 * rows * k, temp_bytes=need - 1)) == INVALID
    need0 = _tb(gs, rows, cols, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    for kt in RA.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, cols, stride, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 1) == INVALID          # k > num_cols, even for empty rows
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_rows_anyk_u64_status(None, rows, cols, k, 1, 0, out, None) == INVALID and list(out) == [0] * 8
    assert gs.lib.gs_topk_rows_anyk_u64_status(temp, rows, cols, k, 1, rows, out, None) == INVALID       # no such row
    assert gs.lib.gs_topk_rows_anyk_u64_status(None, rows, cols, 0, 1, 0, out, None) == 0 and list(out) == [0] * 8
    assert gs.lib.gs_topk_rows_anyk_u64_status(temp, rows, cols, cols + 1, 1, 0, out, None) == INVALID


def test_the_other_entry_points_stay_as_they_were(gs):
    import torch
    rows, cols, k = 4, 5000, 2000
    need = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, 0)
    for kt in RA.KEY_TYPES:        # gs_topk_rows_anyk_u32 and _u16 still refuse the 64-bit key types
        assert gs.lib.gs_topk_rows_anyk_u32(BASE + (4 << 26), need, BASE, None, BASE + (2 << 26), None, rows, cols, cols, k, 0, kt, None) == INVALID
        assert gs.lib.gs_topk_rows_anyk_u16(BASE + (4 << 26), need, BASE, None, BASE + (2 << 26), None, rows, cols, cols, k, 0, kt, None) == INVALID
    # gs_topk_rows_u64 still refuses k = 1025
    assert gs.lib.gs_topk_rows_u64_temp_bytes(10, 5000, 1025, 0) == 0 and gs.lib.gs_topk_rows_u64_temp_bytes(10, 50000, 1025, 1) == 0
    assert gs.lib.gs_topk_rows_u64(BASE + (4 << 26), 1 << 20, BASE, None, BASE + (2 << 26), None, 10, 5000, 5000, 1025, 0, F64, None) == INVALID
    assert gs.lib.gs_topk_rows_u64_temp_bytes(10, 50000, 1024, 1) > 0
    assert gs.lib.gs_topk_rows_max_k() == 1024 == gs.DeviceTopKRows64.MaxK()
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_rows_anyk_plan(3, 100000, 2000, 0, out) == 0 and list(out) == [2, 11, 8192, 8192, 4, 4, 13, 0]
    assert gs.lib.gs_topk_rows_anyk_u16_plan(3, 100000, 2000, 0, out) == 0 and list(out) == [2, 9, 8192, 8192, 4, 4, 13, 0]
    for dtype in (torch.int64, torch.float64):       # topk_rows_anyk() and its class keep raising TypeError for 8-byte keys
        with pytest.raises(TypeError):
            gs.topk_rows_anyk(torch.zeros((4, 3000), dtype=dtype), 2000)
        with pytest.raises(TypeError):
            gs.topk_rows_anyk16(torch.zeros((4, 3000), dtype=dtype), 2000)
    with pytest.raises(TypeError):
        gs.DeviceTopKRowsAnyK.MinKeys(torch.zeros(1), 0, torch.zeros((4, 3000), dtype=torch.int64), None, 4, 3000, 3000, 2000)


# ------------------------------------------------------------------------------------------------ front ends --
def test_size_query_phase_and_exports(gs):
    rows, cols, k = 40, 30000, 2000
    front = gs.DeviceTopKRowsAnyK64
    for kt in (None, gs.GS_KEY_F64):
        for fn in (front.MinKeys, front.MaxKeys):
            assert fn(None, 0, None, None, rows, cols, cols, k, key_type=kt) == _tb(gs, rows, cols, k, 0) > 256
        for fn in (front.MinPairs, front.MaxPairs):
            assert fn(None, 0, None, None, None, None, rows, cols, cols, k, key_type=kt) == _tb(gs, rows, cols, k, 1)
    assert front.MinKeys(None, 0, None, None, rows, cols, cols, cols + 1) == 0
    with pytest.raises(TypeError):
        front.MinKeys(None, 0, None, None, rows, cols, cols, k, key_type=gs.GS_KEY_F32)
    assert issubclass(front, gs.DeviceTopKRowsAnyK) and not hasattr(front, "MaxK")
    assert sorted(a for a in dir(front) if not a.startswith("_")) == ["MaxKeys", "MaxPairs", "MinKeys", "MinPairs", "Plan", "Status"]
    assert callable(gs.topk_rows_anyk64) and "DeviceTopKRowsAnyK64" in gs.__all__ and "topk_rows_anyk64" in gs.__all__
    for name in ("gs_topk_rows_anyk_u64", "gs_topk_rows_anyk_u64_temp_bytes", "gs_topk_rows_anyk_u64_plan", "gs_topk_rows_anyk_u64_status"):
        assert getattr(gs.lib, name).argtypes is not None


def test_topk_rows_anyk64_argument_checks_need_no_device(gs):
    import torch
    t = torch.zeros((4, 3000), dtype=torch.float64)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t, 3001)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t, 2000, values=torch.zeros((4, 3000), dtype=torch.int32), indices=True)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t.reshape(-1), 2)                             # not 2-D
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t.t(), 2)                                     # the last dimension is not contiguous
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t[:, ::2], 2)
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t, 2, values=torch.zeros((4, 2999), dtype=torch.int32))
    with pytest.raises(ValueError):
        gs.topk_rows_anyk64(t, 2, values=torch.zeros((4, 3000), dtype=torch.int64))      # 8-byte values
    for dtype in (torch.int32, torch.float32, torch.int16, torch.bfloat16, torch.uint8):
        with pytest.raises(TypeError):
            gs.topk_rows_anyk64(torch.zeros((4, 3000), dtype=dtype), 2000)
    for dtype in (torch.int64, torch.uint64, torch.float64):
        ko, vo = gs.topk_rows_anyk64(torch.zeros((4, 3000), dtype=dtype), 0, indices=True)
        assert tuple(ko.shape) == (4, 0) and tuple(vo.shape) == (4, 0) and ko.dtype == dtype and vo.dtype == torch.int32
    ko, vo = gs.topk_rows_anyk64(t[:0], 2000)
    assert tuple(ko.shape) == (0, 2000) and vo is None


# ------------------------------------------------------------------------------- the host model and the builders --
def test_status_reference_on_small_rows():
    keys = np.array([5, 5, 1, 9, 5, 0], np.uint64)
    assert RA.status(keys, 4, U64) == [1, 5, 0, 2, 2, 0, 0, 0]
    assert RA.status(keys, 1, U64, True) == [1, 0xFFFFFFFF - 9, 0xFFFFFFFF, 0, 1, 0, 0, 0]
    long = np.arange(9000, dtype=np.uint64)          # round one learns that only 14 bits vary; round two at shift 3 lists 8 images
    assert RA.descent(long, 300)["shifts"] == [53, 3] and RA.status(long, 300, U64) == [2, 299, 0, 299, 1, 2, 1, 8]
    same = np.full(9000, 7, np.uint64)
    assert RA.status(same, 300, I64) == [2, 7, 0x80000000, 0, 300, 1, 2, 0]


def test_the_model_agrees_with_a_sort_on_every_builder():
    cols = RA.SLAB + 5
    rows = [RA.depth_row(cols, d, seed=d) for d in range(1, 7)] + [RA.bucket_row(cols, RA.list_cap(cols), 1), RA.single_row(cols, 2),
                                                                      RA.tie_run_row(cols, 100, 6000, 3)[:2]]
    for img, k in rows:
        for kk in (1, k, cols):
            d = RA.descent(img, kk)
            s = np.sort(img)
            assert d["kth"] == int(s[kk - 1]) and d["less"] == int(np.searchsorted(s, s[kk - 1])) and d["less"] + d["take"] == kk
            assert all(a - b >= 11 or b == 0 for a, b in zip(d["shifts"], d["shifts"][1:])) and len(d["shifts"]) <= 6


def test_the_depth_builder_reaches_every_depth():
    for cols in (RA.DEEP_COLS, RA.SLAB + 9):
        for depth in range(1, 7):
            img, k = RA.depth_row(cols, depth, seed=depth)
            d = RA.descent(img, k)
            assert d["D"] == depth and d["shifts"] == RA.SHIFTS[:depth], (cols, depth, d)
            assert d["mode"] == (2 if depth == 6 else 1)
            assert all(c > RA.list_cap(cols) for c in d["c"][:depth - 1])         # nested above L until the last round
    img, k = RA.depth_row(RA.DEEP_COLS, 6, seed=6)
    assert RA.list_cap(RA.DEEP_COLS) == 3072 and len(RA.descent(img, k)["c"]) == 6


def test_the_bucket_builders_hit_l_and_l_plus_one():
    cols = RA.SLAB + 5
    L = RA.list_cap(cols)
    img, k = RA.bucket_row(cols, L, seed=L)
    d = RA.descent(img, k)
    assert (d["D"], d["mode"], d["list"]) == (1, 1, L)
    img, k = RA.bucket_row(cols, L + 1, seed=L + 1)
    d = RA.descent(img, k)
    assert d["D"] == 2 and d["mode"] == 1 and d["c"][0] == L + 1 and 0 < d["list"] < L
    img, k = RA.single_row(cols, seed=2)
    d = RA.descent(img, k)
    assert (d["D"], d["mode"], d["list"], d["take"], d["less"]) == (1, 1, 1, 1, k - 1)


def test_the_outlier_alone_makes_its_bit_vary():
    cols = RA.SLAB + 100
    pos = RA.outlier_positions(cols)
    assert pos[0] == 0 and pos[1] == cols - 1 and pos[2] // 64 == (cols - 1) // 64 and pos[2] % 64 == 0
    for at in pos:
        keys = RA.outlier_row(cols, at, seed=4)
        d = int(np.bitwise_and.reduce(keys) ^ np.bitwise_or.reduce(keys))
        assert d >> 24 == 1 << (40 - 24)
        rest = np.delete(keys, at)
        assert int(np.bitwise_and.reduce(rest) ^ np.bitwise_or.reduce(rest)) >> 24 == 0
        assert RA.descent(RA.image(keys, I64), 2000)["shifts"] == [53, 30, 13]
    assert RA.descent(RA.image(RA.RW.small_int_rows(1, cols, 5)[0], I64), 2000)["shifts"] == [53, 13]


def test_the_tie_run_builder_and_the_shared_top_rows():
    cols = RA.SLAB + RA.TILE + 1
    L = RA.list_cap(cols)
    for start in (RA.TILE - 3000, RA.SLAB - 3000):
        img, k, below = RA.tie_run_row(cols, start, L + 900, seed=start)
        d = RA.descent(img, k)
        assert (d["mode"], d["D"], d["less"], d["take"]) == (2, 2, below, k - below) and below < k < below + L + 900
        run = np.nonzero(img == np.uint64(d["kth"]))[0]
        assert run[0] == start and run[-1] == start + L + 899 and run[0] // RA.TILE != run[-1] // RA.TILE
    for b in (0, 11, 30, 53, 64):
        img = RA.shared_top_row(cols, b, seed=b)
        diff = int(np.bitwise_and.reduce(img) ^ np.bitwise_or.reduce(img))
        assert diff >> (64 - b) == 0 if b else True
        assert b == 64 or diff.bit_length() == 64 - b
    sp = RA.specials_matrix(2, 5000, F64, 1)
    for pattern in (0x7FF8000000000001, 0xFFF8000000000001, 0, 0x8000000000000000):     # NaNs of both signs, +-0
        assert (sp == np.uint64(pattern)).any()
    assert RA.image(np.array([0x8000000000000000], np.uint64), F64)[0] < RA.image(np.array([0], np.uint64), F64)[0]      # -0 before +0
    z = RA.around_zero(2, 5000, 1).view(np.int64)
    assert z.min() == -40 and z.max() == 40
