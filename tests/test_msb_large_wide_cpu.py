"""Host-side contract of the wide MSB sort above 2^32 elements (gs_msb_large_wide_temp_bytes, gs_msb_sort_large_wide):
workspace sizing and argument validation, neither of which touches a device."""
import ctypes as C

import pytest

INVALID = 1                      # hipErrorInvalidValue
GROUP = 1 << 31                  # elements per finish of the large sort (gs_large.hip, LARGE_GROUP)
COMBOS = [(8, 0, 3), (8, 4, 4), (8, 8, 5), (4, 8, 0), (4, 8, 2)]   # (key bytes, value bytes, a key type)


def _sizes():
    out = {0, 1, 2, 255, 256, 4095, 4096, 4097, 8192, 100003}
    for b in range(10, 37):
        out |= {(1 << b) - 1, 1 << b, (1 << b) + 1, (1 << b) + (1 << (b - 1))}
    return sorted(out)


@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_temp_bytes_nonzero_and_monotone(gs, kb, vb, kt):
    lib = gs.lib
    prev = 0
    for n in _sizes():
        b = lib.gs_msb_large_wide_temp_bytes(n, kb, vb)
        assert b > 0 and b >= prev, (n, b, prev)
        assert b >= lib.gs_msb_wide_temp_bytes(GROUP, kb, vb)
        if n <= GROUP:           # arrays of one group take gs_msb_sort_wide in the same workspace
            assert b >= lib.gs_msb_wide_temp_bytes(n, kb, vb)
        prev = b
    assert lib.gs_msb_large_wide_temp_bytes(1 << 36, kb, vb) > lib.gs_msb_large_wide_temp_bytes(1 << 33, kb, vb)


def test_temp_bytes_follow_the_test_limit(gs, monkeypatch):
    lib = gs.lib
    full = lib.gs_msb_large_wide_temp_bytes(1 << 20, 8, 8)
    monkeypatch.setenv("GS_MSB_LARGE_TEST_LIMIT", "8192")            # read on every call
    small = lib.gs_msb_large_wide_temp_bytes(1 << 20, 8, 8)
    assert 0 < small < full
    assert small >= lib.gs_msb_wide_temp_bytes(8192, 8, 8)
    monkeypatch.delenv("GS_MSB_LARGE_TEST_LIMIT")
    assert lib.gs_msb_large_wide_temp_bytes(1 << 20, 8, 8) == full


def test_argument_validation_without_gpu(gs):
    lib = gs.lib
    n = 1 << 33
    k, ka, v, va = 1 << 40, 2 << 40, 3 << 40, 4 << 40                # distinct, non-overlapping fake device addresses
    ws = 1 << 44
    f = lib.gs_msb_sort_large_wide
    for kb, vb, kt in COMBOS:
        big = lib.gs_msb_large_wide_temp_bytes(n, kb, vb)
        vv, vva = (v, va) if vb else (None, None)
        assert f(None, 0, k, vv, n, ka, vva, kb, vb, kt, None, 1) == INVALID                       # NULL workspace
        assert f(ws, 1000, k, vv, n, ka, vva, kb, vb, kt, None, 1) == INVALID                      # workspace too small
        assert f(ws, big - 1, k, vv, n, ka, vva, kb, vb, kt, None, 1) == INVALID
        assert f(ws, big, k, vv, 1 << 40, ka, vva, kb, vb, kt, None, 1) == INVALID                 # n >= 2^40
        assert f(ws, big, None, vv, n, ka, vva, kb, vb, kt, None, 1) == INVALID                    # no keys
        assert f(ws, big, k, vv, n, None, vva, kb, vb, kt, None, 1) == INVALID                     # no key alternate
        # overlapping arrays, at the real element sizes: an alternate starting on the last key
        assert f(ws, big, k, vv, n, k + kb * (n - 1), vva, kb, vb, kt, None, 1) == INVALID
        assert f(ws, big, k, vv, n, k, vva, kb, vb, kt, None, 1) == INVALID
        if vb:
            assert f(ws, big, k, v, n, ka, None, kb, vb, kt, None, 1) == INVALID                  # values without an alternate
            assert f(ws, big, k, None, n, ka, va, kb, vb, kt, None, 1) == INVALID                 # val_bytes without values
            assert f(ws, big, k, v, n, ka, v + vb * (n - 1), kb, vb, kt, None, 1) == INVALID
            assert f(ws, big, k, v, n, ka, k + 4096, kb, vb, kt, None, 1) == INVALID
            assert f(ws, big, k, k + kb * (n - 1), n, ka, va, kb, vb, kt, None, 1) == INVALID
        else:
            assert f(ws, big, k, v, n, ka, va, kb, vb, kt, None, 1) == INVALID                    # values with val_bytes 0
        # n == 0 is a no-op that needs nothing
        assert f(None, 0, None, None, 0, None, None, kb, vb, kt, None, 1) == 0
    # 8-byte keys end exactly where the alternate starts: no overlap, nothing rejected for it (a NULL workspace is)
    big = lib.gs_msb_large_wide_temp_bytes(n, 8, 0)
    assert f(None, big, k, None, n, k + 8 * n, None, 8, 0, 3, None, 1) == INVALID
    # bad combinations of key bytes, value bytes and key type
    big = lib.gs_msb_large_wide_temp_bytes(n, 8, 8)
    for kb, vb, kt in [(4, 0, 0), (4, 4, 0), (4, 4, 2), (8, 8, 0), (8, 8, 2), (8, 0, 6), (4, 8, 3), (4, 8, 5), (2, 8, 0),
                       (8, 2, 3), (8, 16, 3), (16, 8, 3), (8, 8, -1), (8, 8, 9)]:
        vv, vva = (v, va) if vb else (None, None)
        assert f(ws, big, k, vv, n, ka, vva, kb, vb, kt, None, 1) == INVALID, (kb, vb, kt)


def test_existing_entry_points_still_reject_2p32(gs):
    """The large sorts are the exception to the 2^32 limit: the plain wide sorts keep rejecting it."""
    lib = gs.lib
    sk, sv = C.c_void_p(), C.c_void_p()
    n = 1 << 32
    assert lib.gs_msb_sort_wide(1 << 44, 1 << 44, 1 << 40, None, n, 2 << 40, None, 8, 0, C.byref(sk), C.byref(sv), 3, None, 1) == INVALID
    assert lib.gs_msb_sort_wide(1 << 44, 1 << 44, 1 << 40, 3 << 40, n, 2 << 40, 4 << 40, 4, 8, C.byref(sk), C.byref(sv), 0, None,
                                1) == INVALID
    sel = C.c_int(0)
    keys = (C.c_void_p * 2)(1 << 40, 2 << 40)
    assert lib.gs_lsb_sort_wide(1 << 44, 1 << 44, keys, None, C.byref(sel), n, 8, 0, 0, 64, 0, 3, None) == INVALID
