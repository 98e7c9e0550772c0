"""Host-side contract of the stable sort above 2^32 elements (gs_lsb_large_temp_bytes, gs_lsb_sort_large) and of its device
check gs_check_sorted_stable: workspace sizing, argument validation and the no-op cases, none of which touches a device."""
import ctypes as C

import pytest

INVALID = 1                      # hipErrorInvalidValue
SLICE = 1 << 31                  # elements per slice of the 64-bit pass (gs_large.hip, LARGE_GROUP)
U32, I32, F32, U64, I64, F64 = range(6)
COMBOS = [(4, 0, U32), (4, 4, I32), (4, 8, F32), (8, 0, U64), (8, 4, I64), (8, 8, F64)]   # (key bytes, value bytes, a key type)
K0, K1, V0, V1 = 1 << 40, 2 << 40, 3 << 40, 4 << 40   # distinct, non-overlapping fake device addresses (never dereferenced)
WS = 1 << 44


def _sizes():
    out = {1, 2, 255, 256, 4095, 4096, 4097, 8192, 100003}
    for b in range(10, 38):
        out |= {(1 << b) - 1, 1 << b, (1 << b) + 1, (1 << b) + (1 << (b - 1))}
    return sorted(out)


def _delegate_bytes(lib, n, kb, vb):
    if kb == 4 and vb != 8:
        return lib.gs_lsb_temp_bytes(n, int(vb != 0))
    return lib.gs_lsb_wide_temp_bytes(n, kb, vb)


def _db(a, b):
    return (C.c_void_p * 2)(a, b)


@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_temp_bytes_multiple_of_256_monotone_and_cover_the_delegate(gs, kb, vb, kt):
    lib = gs.lib
    prev = 0
    for n in _sizes():
        b = lib.gs_lsb_large_temp_bytes(n, kb, vb)
        assert b % 256 == 0 and b >= prev, (n, b, prev)
        if n <= SLICE:           # arrays of one slice take gs_lsb_sort_u32 / gs_lsb_sort_wide in the same workspace
            assert b >= _delegate_bytes(lib, n, kb, vb), n
        prev = b
    assert lib.gs_lsb_large_temp_bytes(1 << 36, kb, vb) > lib.gs_lsb_large_temp_bytes(1 << 33, kb, vb)


def test_temp_bytes_about_two_percent_of_the_keys_at_2p33(gs):
    """Each slice of 2^31 u32 keys carries its own spine (32 MiB) and prefix16 (128 MiB): 4 slices of 160 MiB for 32 GiB of keys."""
    n = 1 << 33
    b = gs.lib.gs_lsb_large_temp_bytes(n, 4, 0)
    assert b >= 4 * (160 << 20)
    assert 0.018 < b / (4 * n) < 0.021, b / (4 * n)
    assert gs.lib.gs_lsb_large_temp_bytes(n, 4, 4) == b          # values need no scratch of their own


def test_temp_bytes_follow_the_test_limit(gs, monkeypatch):
    lib = gs.lib
    full = lib.gs_lsb_large_temp_bytes(1 << 20, 8, 8)
    monkeypatch.setenv("GS_MSB_LARGE_TEST_LIMIT", "4096")            # read on every call
    small = lib.gs_lsb_large_temp_bytes(1 << 20, 8, 8)
    assert small != full and small % 256 == 0
    assert lib.gs_lsb_large_temp_bytes(4096, 8, 8) >= lib.gs_lsb_wide_temp_bytes(4096, 8, 8)
    monkeypatch.delenv("GS_MSB_LARGE_TEST_LIMIT")
    assert lib.gs_lsb_large_temp_bytes(1 << 20, 8, 8) == full


def test_every_refusal_without_gpu(gs):
    lib = gs.lib
    f = lib.gs_lsb_sort_large
    n = 1 << 33
    for kb, vb, kt in COMBOS:
        big = lib.gs_lsb_large_temp_bytes(n, kb, vb)
        vv = _db(V0, V1) if vb else None
        end = 8 * kb

        def call(ws=WS, nbytes=big, keys=None, vals=vv, sel=0, num=n, kb_=kb, vb_=vb, bb=0, eb=end, kt_=kt):
            s = C.c_int(sel)
            rc = f(ws, nbytes, _db(K0, K1) if keys is None else keys, vals, C.byref(s), num, kb_, vb_, bb, eb, 0, kt_, None)
            assert s.value == sel, "a refused call changed the selector"
            return rc

        assert call(ws=None) == INVALID                               # NULL workspace
        assert call(nbytes=1000) == INVALID                           # workspace too small
        assert call(nbytes=big - 1) == INVALID
        assert call(num=1 << 40) == INVALID                           # n >= 2^40
        assert call(num=(1 << 40) + 5, ws=None, nbytes=0) == INVALID
        for bb, eb in [(-1, end), (0, end + 1), (9, 8), (end, end + 8)]:   # bad bit ranges
            assert call(bb=bb, eb=eb) == INVALID, (bb, eb)
        assert call(keys=_db(None, K1)) == INVALID                    # a missing key half
        assert call(keys=_db(K0, None)) == INVALID
        assert f(WS, big, None, vv, C.byref(C.c_int(0)), n, kb, vb, 0, end, 0, kt, None) == INVALID   # no key buffer at all
        s = C.c_int(2)
        assert f(WS, big, _db(K0, K1), vv, C.byref(s), n, kb, vb, 0, end, 0, kt, None) == INVALID and s.value == 2
        assert f(WS, big, _db(K0, K1), vv, None, n, kb, vb, 0, end, 0, kt, None) == INVALID         # no selector
        # overlapping arrays, at the real element sizes: the alternate starting on the last key, or on the first
        assert call(keys=_db(K0, K0 + kb * (n - 1))) == INVALID
        assert call(keys=_db(K0, K0)) == INVALID
        if vb:
            assert call(vals=_db(V0, None)) == INVALID                # a missing value half
            assert call(vals=_db(None, V1)) == INVALID
            assert call(vals=None) == INVALID                         # val_bytes without values
            assert call(vals=_db(V0, V0 + vb * (n - 1))) == INVALID
            assert call(vals=_db(V0, K1 + 4096)) == INVALID           # a value half inside the key alternate
            assert call(vals=_db(K0 + kb * (n - 1), V1)) == INVALID
        else:
            assert call(vals=_db(V0, V1)) == INVALID                  # values with val_bytes 0
    # keys that end exactly where the alternate starts do not overlap (the NULL workspace is what is refused)
    assert f(None, 1 << 40, _db(K0, K0 + 8 * n), None, C.byref(C.c_int(0)), n, 8, 0, 0, 64, 0, U64, None) == INVALID
    # bad combinations of key bytes, value bytes and key type
    for kb, vb, kt in [(4, 0, U64), (4, 8, F64), (8, 0, U32), (8, 8, F32), (2, 0, 8), (1, 0, 6), (16, 0, U64), (8, 2, U64),
                       (8, 16, U64), (4, 12, U32), (8, 8, -1), (8, 8, 6), (4, 0, 9)]:
        vv = _db(V0, V1) if vb else None
        assert f(WS, 1 << 44, _db(K0, K1), vv, C.byref(C.c_int(0)), n, kb, vb, 0, 8 * max(kb, 1), 0, kt, None) == INVALID, (kb, vb, kt)


@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_no_op_cases_need_nothing_and_keep_the_selector(gs, kb, vb, kt):
    f = gs.lib.gs_lsb_sort_large
    vv = _db(V0, V1) if vb else None
    for sel in (0, 1):
        s = C.c_int(sel)
        assert f(None, 0, _db(K0, K1), vv, C.byref(s), 0, kb, vb, 0, 8 * kb, 0, kt, None) == 0 and s.value == sel   # n == 0
        for bit in (0, 3, 8 * kb):                                                                                     # empty bit range
            assert f(None, 0, _db(K0, K1), vv, C.byref(s), 1 << 34, kb, vb, bit, bit, 1, kt, None) == 0 and s.value == sel


def test_plain_lsb_sorts_still_refuse_2p32(gs):
    """The large sort is the exception to the 2^32 limit: gs_lsb_sort_u32 and gs_lsb_sort_wide keep refusing it."""
    lib = gs.lib
    sel = C.c_int(0)
    assert lib.gs_lsb_sort_u32(WS, WS, _db(K0, K1), None, C.byref(sel), 1 << 32, 0, 32, 0, U32, None) == INVALID
    assert lib.gs_lsb_sort_wide(WS, WS, _db(K0, K1), None, C.byref(sel), 1 << 32, 8, 0, 0, 64, 0, U64, None) == INVALID
    assert sel.value == 0


def test_check_sorted_stable_refuses_bad_arguments(gs):
    f = gs.lib.gs_check_sorted_stable
    for kb, kt, bb, eb in [(4, U64, 0, 32), (8, U32, 0, 64), (2, U32, 0, 16), (4, U32, 0, 33), (8, I64, -1, 64), (8, F64, 9, 8),
                           (4, 7, 0, 32)]:
        assert f(K0, None, 100, kb, kt, bb, eb, 0, V0, None) == INVALID, (kb, kt, bb, eb)


def test_python_size_query(gs):
    import torch
    lsb = gs.DeviceRadixSortLarge
    k = gs.DoubleBuffer(torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64))
    v = gs.DoubleBuffer(torch.empty(0, dtype=torch.int32), torch.empty(0, dtype=torch.int32))
    n = (1 << 32) + 7
    assert lsb.SortKeys(None, 0, k, n) == gs.lib.gs_lsb_large_temp_bytes(n, 8, 0)
    assert lsb.SortPairsDescending(None, 0, k, v, n) == gs.lib.gs_lsb_large_temp_bytes(n, 8, 4)
