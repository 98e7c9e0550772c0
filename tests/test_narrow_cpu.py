"""CPU tests of gs_lsb_sort_narrow (8- and 16-bit keys on kernels of their own): the symbols, the host-side sizing and the
argument checks, which all answer before the device is touched.  No GPU needed."""
import ctypes as C

import pytest

INVALID = 1                     # hipErrorInvalidValue
VAL_BYTES = (0, 1, 2, 4, 8, 16)


def _narrow_types(gs):
    return {gs.GS_KEY_U8: 1, gs.GS_KEY_I8: 1, gs.GS_KEY_U16: 2, gs.GS_KEY_I16: 2}


def test_symbols_exported_and_bound(gs):
    from gpu_sort_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for s in ("gs_lsb_narrow_temp_bytes", "gs_lsb_sort_narrow"):
        assert hasattr(raw, s), s
        assert s in _lib.SIGNATURES, s
        assert getattr(gs.lib, s).argtypes is not None
    assert _lib.SIGNATURES["gs_lsb_sort_narrow"] == _lib.SIGNATURES["gs_lsb_sort_any"]      # the same contract


def test_temp_bytes(gs):
    q = gs.lib.gs_lsb_narrow_temp_bytes
    assert q(1000, gs.GS_KEY_U32, 0) == 0 and q(1000, gs.GS_KEY_U64, 4) == 0 and q(1000, 99, 0) == 0
    assert q(1000, gs.GS_KEY_U8, 3) == 0 and q(1000, gs.GS_KEY_U8, 32) == 0 and q(1000, gs.GS_KEY_I16, 3) == 0
    assert gs.lib.gs_lsb_narrow_tile(gs.GS_KEY_U32, 0) == 0 and gs.lib.gs_lsb_narrow_tile(gs.GS_KEY_U8, 3) == 0
    sizes = (0, 1, 777, 100003, (1 << 24) + 7, 1 << 28, (1 << 32) - 1)
    for kt, kb in _narrow_types(gs).items():
        for vb in VAL_BYTES:
            tile = gs.lib.gs_lsb_narrow_tile(kt, vb)
            assert tile >= 2048 and tile % 512 == 0
            prev = 0
            for n in sizes:
                b = q(n, kt, vb)
                assert b > 0 and b % 256 == 0 and b >= prev, (kt, vb, n, b)
                prev = b
                if kb == 2:       # the intermediate keys and values of the pass in -> temp -> out
                    assert b >= n * (2 + vb)
                    assert b <= n * (2 + vb) + n * (2 + vb) // 8 + 4096
            if kb == 1:           # spine and totals only: 1 KiB per tile of `tile` elements, the 1 KiB of totals and the slack,
                n = 1 << 28       # which is far below the key bytes plus the value bytes (a quarter at the very most)
                assert q(n, kt, vb) <= 1024 * (n // tile) + 1024 + 2 * 256, (kt, vb)
                assert q(n, kt, vb) * 4 <= n * (1 + vb), (kt, vb)


def test_argument_validation_without_gpu(gs):
    # these return hipErrorInvalidValue (1) before touching the device: the pointers are never dereferenced
    f, q = gs.lib.gs_lsb_sort_narrow, gs.lib.gs_lsb_narrow_temp_bytes
    U8, U16 = gs.GS_KEY_U8, gs.GS_KEY_U16
    n = 1000
    ws, kin, kout, vin, vout = 0x10000, 0x200000, 0x300000, 0x400000, 0x500000
    nb = q(n, U8, 0)
    nb4 = q(n, U8, 4)
    assert f(None, nb, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID              # no workspace
    assert f(ws, 0, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID                 # too small
    assert f(ws, nb - 1, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, q(n, U16, 8) - 1, kin, kout, vin, vout, n, U16, 8, 0, 16, 0, None) == INVALID
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, 0, 9, 0, None) == INVALID                # end_bit beyond the key
    assert f(ws, q(n, U16, 0), kin, kout, None, None, n, U16, 0, 0, 17, 0, None) == INVALID
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, 5, 4, 0, None) == INVALID                # begin_bit > end_bit
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, -1, 4, 0, None) == INVALID
    assert f(ws, 1 << 40, kin, kout, None, None, 1 << 32, U8, 0, 0, 8, 0, None) == INVALID     # num_items = 2^32
    assert f(ws, nb, kin, kin, None, None, n, U8, 0, 0, 8, 0, None) == INVALID                 # input == output
    assert f(ws, nb4, kin, kout, vin, vin, n, U8, 4, 0, 8, 0, None) == INVALID
    assert f(ws, nb, kin, kout, vin, vout, n, U8, 0, 0, 8, 0, None) == INVALID                 # values given with val_bytes 0
    assert f(ws, nb4, kin, kout, None, None, n, U8, 4, 0, 8, 0, None) == INVALID               # values missing
    assert f(ws, nb4, kin, kout, vin, None, n, U8, 4, 0, 8, 0, None) == INVALID
    assert f(ws, nb4, kin, kout, None, vout, n, U8, 4, 0, 8, 0, None) == INVALID
    nb16 = q(n, U8, 16)
    assert f(ws, nb16, kin, kout, vin + 8, vout, n, U8, 16, 0, 8, 0, None) == INVALID          # misaligned 16-byte values
    assert f(ws, nb16, kin, kout, vin, vout + 4, n, U8, 16, 0, 8, 0, None) == INVALID
    assert f(ws, q(n, U16, 0), kin + 1, kout, None, None, n, U16, 0, 0, 16, 0, None) == INVALID   # odd address for u16 keys
    assert f(ws, q(n, U16, 0), kin, kout + 1, None, None, n, U16, 0, 0, 16, 0, None) == INVALID
    assert f(ws, 1 << 30, kin, kout, None, None, n, gs.GS_KEY_U32, 0, 0, 8, 0, None) == INVALID   # not a narrow key type
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, U8, 3, 0, 8, 0, None) == INVALID               # not a listed value size
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, U8, 32, 0, 8, 0, None) == INVALID


def test_empty_sort_succeeds_with_null_pointers(gs):
    f = gs.lib.gs_lsb_sort_narrow
    for kt in _narrow_types(gs):
        for vb in VAL_BYTES:
            assert f(None, 0, None, None, None, None, 0, kt, vb, 0, 8, 0, None) == 0
            assert f(None, 0, None, None, None, None, 0, kt, vb, 3, 3, 1, None) == 0
