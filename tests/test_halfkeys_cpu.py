"""The float key categories of 8 and 16 bits (GS_KEY_F16 / GS_KEY_BF16 / GS_KEY_F8) without a GPU: the enum values, the size
queries (the same as the integer type of the same width gives), the argument checks that answer before the device is
touched, the Python front ends' size queries and refusals, and the numpy reference's own placement of the special values."""
import ctypes as C

import numpy as np
import pytest
import torch

import halfkeys_ref as R

INVALID = 1                     # hipErrorInvalidValue
SIZES = (1, 100003, 1 << 28, 1 << 33)


def _pairs(gs):
    return [(getattr(gs, f), getattr(gs, u), bits) for f, u, bits in R.KINDS.values()]


def test_enum_values_exported_and_bound(gs):
    from gpu_sort_amd import _lib
    assert (gs.GS_KEY_F16, gs.GS_KEY_BF16, gs.GS_KEY_F8) == (10, 11, 12)
    assert (_lib.GS_KEY_F16, _lib.GS_KEY_BF16, _lib.GS_KEY_F8) == (10, 11, 12)
    for name in ("GS_KEY_F16", "GS_KEY_BF16", "GS_KEY_F8"):
        assert name in gs.__all__
    with open(_lib.INCLUDE_DIR + "/gpusort.h") as f:
        h = f.read()
    for name, v in (("GS_KEY_F16", 10), ("GS_KEY_BF16", 11), ("GS_KEY_F8", 12)):
        assert "%s = %d" % (name, v) in h


def test_size_queries_equal_the_integer_types(gs):
    L = gs.lib
    for kf, ku, _ in _pairs(gs):
        for vb in (0, 1, 2, 3, 4, 8, 16, 32):
            assert L.gs_lsb_narrow_tile(kf, vb) == L.gs_lsb_narrow_tile(ku, vb)
            for n in SIZES:
                assert L.gs_lsb_narrow_temp_bytes(n, kf, vb) == L.gs_lsb_narrow_temp_bytes(n, ku, vb), (kf, vb, n)
                assert L.gs_lsb_narrow_large_temp_bytes(n, kf, vb) == L.gs_lsb_narrow_large_temp_bytes(n, ku, vb), (kf, vb, n)
                assert L.gs_lsb_any_temp_bytes(n, kf, vb) == L.gs_lsb_any_temp_bytes(n, ku, vb) > 0, (kf, vb, n)
                for nseg in (1, 4097):
                    assert (L.gs_segmented_narrow_temp_bytes(n, kf, vb, nseg) ==
                            L.gs_segmented_narrow_temp_bytes(n, ku, vb, nseg)), (kf, vb, n, nseg)
        assert L.gs_lsb_narrow_tile(kf, 0) > 0 and L.gs_lsb_narrow_temp_bytes(100003, kf, 4) > 0
        assert L.gs_lsb_narrow_large_temp_bytes(1 << 33, kf, 0) > 0
        assert L.gs_segmented_narrow_temp_bytes(100003, kf, 8, 7) > 0


def test_segmented_cap(gs):
    for kf, ku, _ in _pairs(gs):
        for vb in (0, 4, 8):
            assert gs.lib.gs_segmented_narrow_cap(kf, vb) == gs.lib.gs_segmented_narrow_cap(ku, vb) > 0
        for vb in (1, 2, 16):
            assert gs.lib.gs_segmented_narrow_cap(kf, vb) == 0


def test_argument_checks_answer_before_the_device(gs):
    # hipErrorInvalidValue (1) before the device is touched: the pointers are never dereferenced
    f, q = gs.lib.gs_lsb_sort_narrow, gs.lib.gs_lsb_narrow_temp_bytes
    F16, BF16, F8 = gs.GS_KEY_F16, gs.GS_KEY_BF16, gs.GS_KEY_F8
    ws, kin, kout, vin, vout, n = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 1000
    assert f(ws, q(n, F16, 0), kin, kout, None, None, n, F16, 0, 0, 17, 0, None) == INVALID       # end_bit beyond the key
    assert f(ws, q(n, BF16, 0), kin, kout, None, None, n, BF16, 0, 0, 17, 0, None) == INVALID
    assert f(ws, q(n, F8, 0), kin, kout, None, None, n, F8, 0, 0, 9, 0, None) == INVALID
    assert f(ws, q(n, F16, 0), kin + 1, kout, None, None, n, F16, 0, 0, 16, 0, None) == INVALID   # odd address
    assert f(ws, q(n, F16, 0), kin, kout + 1, None, None, n, F16, 0, 0, 16, 0, None) == INVALID
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, F16, 3, 0, 16, 0, None) == INVALID             # not a listed value size
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, F8, 3, 0, 8, 0, None) == INVALID
    assert f(ws, q(n, F16, 0) - 1, kin, kout, None, None, n, F16, 0, 0, 16, 0, None) == INVALID   # workspace too small
    g = gs.lib.gs_lsb_sort_any
    assert g(ws, 1 << 30, kin, kout, None, None, n, F16, 0, 0, 17, 0, None) == INVALID
    assert g(ws, 1 << 30, kin, kout, None, None, n, F8, 0, 0, 9, 0, None) == INVALID
    s = gs.lib.gs_segmented_sort_narrow
    kp = (C.c_void_p * 2)(kin, kout)
    sel = C.c_int(0)
    nb = gs.lib.gs_segmented_narrow_temp_bytes(n, F16, 0, 3)
    assert s(ws, nb, kp, None, C.byref(sel), n, 3, vin, vout, F16, 0, 0, 17, 0, None) == INVALID
    assert s(ws, nb, kp, None, C.byref(sel), n, 3, vin, vout, F8, 0, 0, 9, 0, None) == INVALID
    kodd = (C.c_void_p * 2)(kin + 1, kout)
    assert s(ws, nb, kodd, None, C.byref(sel), n, 3, vin, vout, BF16, 0, 0, 16, 0, None) == INVALID
    lg = gs.lib.gs_lsb_sort_narrow_large
    assert lg(ws, 1 << 40, kin, kout, None, None, 1 << 33, F16, 0, 0, 17, 0, None) == INVALID
    assert lg(ws, 1 << 40, kin, kout, vin, vout, 1 << 33, F8, 3, 0, 8, 0, None) == INVALID


def test_empty_sort_succeeds_with_null_pointers(gs):
    for kf, _, bits in _pairs(gs):
        for vb in (0, 4, 16):
            assert gs.lib.gs_lsb_sort_narrow(None, 0, None, None, None, None, 0, kf, vb, 0, bits, 0, None) == 0
            assert gs.lib.gs_lsb_sort_narrow_large(None, 0, None, None, None, None, 0, kf, vb, 0, bits, 1, None) == 0
        assert gs.lib.gs_lsb_sort_any(None, 0, None, None, None, None, 0, kf, 3, 0, bits, 0, None) == 0
        sel = C.c_int(1)
        assert gs.lib.gs_segmented_sort_narrow(None, 0, None, None, C.byref(sel), 0, 0, None, None, kf, 0, 0, bits, 0, None) == 0
        assert sel.value == 1


def _float8_dtypes():
    return [getattr(torch, n) for n in ("float8_e4m3fn", "float8_e5m2", "float8_e4m3fnuz", "float8_e5m2fnuz") if hasattr(torch, n)]


def test_plain_front_end_sizes_float_tensors(gs):
    n = 100003
    cases = [(torch.float16, gs.GS_KEY_F16), (torch.bfloat16, gs.GS_KEY_BF16)] + [(d, gs.GS_KEY_F8) for d in _float8_dtypes()]
    for dt, kt in cases:
        dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
        want = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, 0)
        assert gs.DeviceRadixSort.SortKeys(None, 0, dk, n) == want > 0
        assert gs.DeviceRadixSort.SortKeysDescending(None, 0, dk, n) == want
        dv = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32))
        assert gs.DeviceRadixSort.SortPairs(None, 0, dk, dv, n) == gs.lib.gs_lsb_narrow_temp_bytes(n, kt, 4) > 0
        d3 = gs.DoubleBuffer(torch.zeros((n, 3), dtype=torch.uint8), torch.zeros((n, 3), dtype=torch.uint8))
        assert gs.DeviceRadixSort.SortPairs(None, 0, dk, d3, n) == gs.lib.gs_lsb_any_temp_bytes(n, kt, 3) > 0
        big = 1 << 33
        dkl = gs.DoubleBuffer(torch.zeros(1, dtype=dt), torch.zeros(1, dtype=dt))
        assert gs.DeviceRadixSortLarge.SortKeys(None, 0, dkl, big) == gs.lib.gs_lsb_narrow_large_temp_bytes(big, kt, 0) > 0


def test_segmented_front_end_needs_the_explicit_float_key_type(gs):
    S = gs.DeviceSegmentedRadixSort
    n, nseg = 1000, 3
    offs = torch.zeros(nseg + 1, dtype=torch.int32)
    for dt, kt, name in ((torch.float16, gs.GS_KEY_F16, "GS_KEY_F16"), (torch.bfloat16, gs.GS_KEY_BF16, "GS_KEY_BF16")):
        dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
        want = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, 0, nseg)
        assert S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=kt) == want > 0
        dv = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64))
        assert (S.SortPairsDescending(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:], key_type=kt) ==
                gs.lib.gs_segmented_narrow_temp_bytes(n, kt, 8, nseg) > 0)
        with pytest.raises(TypeError, match=name):              # the message names the key_type to pass
            S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:])
        with pytest.raises(TypeError, match="no key category"):
            S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_I16)
        with pytest.raises(TypeError):                          # a float key_type of another width
            S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_F8)
    for dt in _float8_dtypes():
        dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
        assert (S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_F8) ==
                gs.lib.gs_segmented_narrow_temp_bytes(n, gs.GS_KEY_F8, 0, nseg) > 0)
        with pytest.raises(TypeError):
            S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_F16)


def test_reference_places_the_special_values_where_the_header_says():
    """the numpy reference itself: negative NaNs first by their bits, -inf ... -0.0, +0.0 ... +inf, positive NaNs last by
    their bits; and the pad patterns of the segmented kernels sit at the ends"""
    nan_n2, nan_n1, ninf, m1, nz, pz, p1, pinf, nan_p1, nan_p2 = 0xffff, 0xfe00, 0xfc00, 0xbc00, 0x8000, 0x0000, 0x3c00, 0x7c00, 0x7e00, 0x7fff
    b = np.array([p1, nan_p2, nz, ninf, nan_n1, pz, pinf, m1, nan_n2, nan_p1], dtype=np.uint16)
    asc = b[R.order(b, 16, 0, 16, False)]
    assert asc.tolist() == [nan_n2, nan_n1, ninf, m1, nz, pz, p1, pinf, nan_p1, nan_p2]
    assert b[R.order(b, 16, 0, 16, True)].tolist() == asc.tolist()[::-1]
    vals = torch.from_numpy(asc[2:8].view(np.int16).copy()).view(torch.float16).float()
    assert bool((vals[1:] >= vals[:-1]).all())                  # the finite part and the infinities are in value order
    assert R.image(np.array([0x7fff, 0xffff, 0x8000], np.uint16), 16).tolist() == [0xffff, 0x0000, 0x7fff]
    assert R.image(np.array([0x7f, 0xff, 0x80], np.uint8), 8).tolist() == [0xff, 0x00, 0x7f]
    for bits in (8, 16):                                        # the image is a bijection and monotone in the value
        allb = np.arange(1 << bits, dtype=np.uint32)
        assert np.array_equal(np.sort(R.image(allb, bits)), allb)
    f = torch.arange(0, 0x7c01, dtype=torch.int32).to(torch.int16).view(torch.float16).float().numpy()   # +0 ... +inf
    assert np.all(np.diff(f) > 0) and np.all(np.diff(R.image(np.arange(0, 0x7c01), 16).astype(np.int64)) > 0)
    f = torch.arange(0x8000, 0xfc01, dtype=torch.int32).to(torch.int16).view(torch.float16).float().numpy()   # -0 ... -inf
    assert np.all(np.diff(f) < 0) and np.all(np.diff(R.image(np.arange(0x8000, 0xfc01), 16).astype(np.int64)) < 0)

