"""Host-side contract of the MSB sort above 2^32 keys (gs_msb_large_temp_bytes, gs_msb_sort_large_u32): workspace sizing
and argument validation, neither of which touches a device."""
import ctypes as C

import pytest

INVALID = 1                      # hipErrorInvalidValue
GROUP = 1 << 31                  # keys per finish of the large sort (gs_large.hip, LARGE_GROUP)


def _sizes():
    out = {0, 1, 2, 255, 256, 8191, 8192, 8193, 100003}
    for b in range(10, 37):
        out |= {(1 << b) - 1, 1 << b, (1 << b) + 1, (1 << b) + (1 << (b - 1))}
    return sorted(out)


@pytest.mark.parametrize("has_values", [0, 1])
def test_temp_bytes_nonzero_and_monotone(gs, has_values):
    lib = gs.lib
    prev = 0
    for n in _sizes():
        b = lib.gs_msb_large_temp_bytes(n, has_values)
        assert b > 0 and b >= prev, (n, b, prev)
        assert b >= lib.gs_msb_finish_temp_bytes(GROUP, has_values, 1)
        if n <= GROUP:           # arrays of one group take the plain MSB sort in the same workspace
            assert b >= lib.gs_msb_temp_bytes(n, has_values)
        prev = b
    # the 64-bit pass's tables grow with n: 2^36 keys need more than 2^33
    assert lib.gs_msb_large_temp_bytes(1 << 36, has_values) > lib.gs_msb_large_temp_bytes(1 << 33, has_values)


def test_temp_bytes_follow_the_test_limit(gs, monkeypatch):
    lib = gs.lib
    full = lib.gs_msb_large_temp_bytes(1 << 20, 0)
    monkeypatch.setenv("GS_MSB_LARGE_TEST_LIMIT", "8192")            # read on every call
    small = lib.gs_msb_large_temp_bytes(1 << 20, 0)
    assert 0 < small < full
    assert small >= lib.gs_msb_finish_temp_bytes(8192, 0, 1)
    monkeypatch.delenv("GS_MSB_LARGE_TEST_LIMIT")
    assert lib.gs_msb_large_temp_bytes(1 << 20, 0) == full


def test_argument_validation_without_gpu(gs):
    lib = gs.lib
    n = 1 << 33
    k, ka, v, va = 1 << 40, 2 << 40, 3 << 40, 4 << 40                # distinct, non-overlapping fake device addresses
    big = lib.gs_msb_large_temp_bytes(n, 1)
    f = lib.gs_msb_sort_large_u32
    assert f(None, 0, k, None, n, ka, None, 0, None, 1) == INVALID                       # NULL workspace
    assert f(1 << 44, 1000, k, None, n, ka, None, 0, None, 1) == INVALID                 # workspace too small
    assert f(1 << 44, big, k, None, 1 << 40, ka, None, 0, None, 1) == INVALID            # n >= 2^40
    assert f(1 << 44, big, k, None, (1 << 40) + 5, ka, None, 0, None, 1) == INVALID
    for kt in (-1, 3, 5, 9):                                                             # 32-bit key types only
        assert f(1 << 44, big, k, None, n, ka, None, kt, None, 1) == INVALID
    assert f(1 << 44, big, None, None, n, ka, None, 0, None, 1) == INVALID               # no keys
    assert f(1 << 44, big, k, None, n, None, None, 0, None, 1) == INVALID                # no alternate
    assert f(1 << 44, big, k, v, n, ka, None, 0, None, 1) == INVALID                     # values without an alternate
    # overlapping arrays
    assert f(1 << 44, big, k, None, n, k, None, 0, None, 1) == INVALID
    assert f(1 << 44, big, k, None, n, k + 4 * (n - 1), None, 0, None, 1) == INVALID
    assert f(1 << 44, big, k, v, n, ka, k + 4096, 0, None, 1) == INVALID
    assert f(1 << 44, big, k, v, n, ka, ka, 0, None, 1) == INVALID
    assert f(1 << 44, big, k, v, n, ka, v, 0, None, 1) == INVALID
    # n == 0 is a no-op that needs nothing
    assert f(None, 0, None, None, 0, None, None, 0, None, 1) == 0
    assert f(None, 0, k, v, 0, ka, va, 2, None, 1) == 0


def test_existing_entry_points_still_reject_2p32(gs):
    """The large sort is the one exception to the 2^32 limit: the plain MSB sort keeps rejecting it."""
    lib = gs.lib
    sk, sv = C.c_void_p(), C.c_void_p()
    assert lib.gs_msb_sort_u32(1 << 44, 1 << 40, 1 << 40, None, 1 << 32, 2 << 40, None, C.byref(sk), C.byref(sv), 0, None, 1) == INVALID
