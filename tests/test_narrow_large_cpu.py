"""CPU tests of gs_lsb_sort_narrow_large (8- and 16-bit keys above 2^32 elements): the symbols, the host-side sizing (against a
restatement of the header's formula) and the argument checks, which all answer before the device is touched.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

INVALID = 1                     # hipErrorInvalidValue
VAL_BYTES = (0, 1, 2, 4, 8, 16)
LIMIT_ENV = "GS_MSB_LARGE_TEST_LIMIT"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 777, 100_003, (1 << 24) + 7, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 32, (1 << 32) + (1 << 21) + 7, 1 << 33,
         (1 << 36) + 5, (1 << 40) - 1)


def _narrow_types(gs):
    return {gs.GS_KEY_U8: 1, gs.GS_KEY_I8: 1, gs.GS_KEY_U16: 2, gs.GS_KEY_I16: 2}


def _a256(x):
    return (x + 255) & ~255


def formula(n, kb, vb, S=1 << 31):
    """The header's workspace formula, restated: the 64-bit pass's workspace, or gs_lsb_sort_narrow's for one slice."""
    T = 8192 if vb <= 4 else (4096 if vb == 8 else 2048)
    tiles = lambda m: max(1, -(-m // T))
    slices = max(1, -(-n // S))
    big = slices * _a256(256 * 4 * tiles(S)) + _a256(slices * 256 * 4) + _a256(slices * 256 * 8) + _a256(256 * 8) + 256
    m = min(n, S)
    one = _a256(256 * 4 * tiles(m)) + _a256(256 * 4) + 256
    if kb == 2:
        big += _a256(2 * n) + _a256(vb * n)
        one += _a256(2 * m) + _a256(vb * m)
    return max(big, one)


def test_symbols_declared_exported_and_bound(gs):
    from gpu_sort_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    for s in ("gs_lsb_narrow_large_temp_bytes", "gs_lsb_sort_narrow_large"):
        assert re.search(r"\b%s\(" % s, header), s
        assert hasattr(raw, s), s
        assert s in _lib.SIGNATURES, s
        assert getattr(gs.lib, s).argtypes is not None
    assert _lib.SIGNATURES["gs_lsb_sort_narrow_large"] == _lib.SIGNATURES["gs_lsb_sort_narrow"]      # the same argument list
    assert _lib.SIGNATURES["gs_lsb_narrow_large_temp_bytes"] == _lib.SIGNATURES["gs_lsb_narrow_temp_bytes"]
    assert gs.lib.gs_version() == 100


def test_temp_bytes(gs, monkeypatch):
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    q, q1 = gs.lib.gs_lsb_narrow_large_temp_bytes, gs.lib.gs_lsb_narrow_temp_bytes
    assert q(1000, gs.GS_KEY_U32, 0) == 0 and q(1000, gs.GS_KEY_U64, 4) == 0 and q(1000, 99, 0) == 0
    assert q(1000, gs.GS_KEY_U8, 3) == 0 and q(1000, gs.GS_KEY_U8, 32) == 0 and q(1000, gs.GS_KEY_I16, 3) == 0
    for kt, kb in _narrow_types(gs).items():
        for vb in VAL_BYTES:
            assert q(1 << 40, kt, vb) == 0 and q((1 << 40) + 1, kt, vb) == 0 and q(1 << 63, kt, vb) == 0
            prev = 0
            for n in SIZES:
                b = q(n, kt, vb)
                assert b > 0 and b % 256 == 0 and b >= prev, (kt, vb, n, b)
                prev = b
                if n < 1 << 32:
                    assert b >= q1(n, kt, vb), (kt, vb, n)
                assert b == formula(n, kb, vb), (kt, vb, n, b, formula(n, kb, vb))
                if kb == 2:
                    assert b >= n * (2 + vb)
            if kb == 1:           # no intermediate: 1 KiB of spine per tile, far below the key bytes plus the value bytes (an
                n = 1 << 33       # eighth at the very most), and what 4 slices add to gs_lsb_sort_narrow's layout is 14 KiB
                assert q(n, kt, vb) * 4 <= n * (1 + vb), (kt, vb)
                assert q(n, kt, vb) <= 4 * q1(1 << 31, kt, vb) + 14 * 1024, (kt, vb)


def test_hook_is_read_on_every_call(gs, monkeypatch):
    q = gs.lib.gs_lsb_narrow_large_temp_bytes
    U8, I16 = gs.GS_KEY_U8, gs.GS_KEY_I16
    n = 100_001
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    plain = (q(n, U8, 8), q(n, I16, 4))
    assert plain == (formula(n, 1, 8), formula(n, 2, 4))
    for k in (256, 4096, 8193):
        monkeypatch.setenv(LIMIT_ENV, str(k))
        hooked = (q(n, U8, 8), q(n, I16, 4))
        assert hooked == (formula(n, 1, 8, k), formula(n, 2, 4, k)), k
        assert hooked[0] != plain[0] and hooked[1] != plain[1], k   # (smaller: the spines are sized for slices of k)
    monkeypatch.setenv(LIMIT_ENV, "100")               # below the smallest limit: ignored
    assert (q(n, U8, 8), q(n, I16, 4)) == plain
    monkeypatch.delenv(LIMIT_ENV)
    assert (q(n, U8, 8), q(n, I16, 4)) == plain


@pytest.mark.parametrize("limit", [None, "4096"])
def test_argument_validation_without_gpu(gs, monkeypatch, limit):
    """hipErrorInvalidValue (1) before the device is touched: the pointers are never dereferenced.  With the hook, n = 100 000 is a
    multi-slice call; without it, it is the one-slice route: both refuse the same things."""
    if limit:
        monkeypatch.setenv(LIMIT_ENV, limit)
    else:
        monkeypatch.delenv(LIMIT_ENV, raising=False)
    f, q = gs.lib.gs_lsb_sort_narrow_large, gs.lib.gs_lsb_narrow_large_temp_bytes
    U8, U16 = gs.GS_KEY_U8, gs.GS_KEY_U16
    n = 100_000
    ws, kin, kout, vin, vout = 0x10000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
    nb, nb4, nb16, nbu16 = q(n, U8, 0), q(n, U8, 4), q(n, U8, 16), q(n, U16, 0)
    assert f(None, nb, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID              # no workspace
    assert f(ws, 0, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID                 # too small
    assert f(ws, nb - 1, kin, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, nb - 1, kin, kout, None, None, n, U8, 0, 4, 4, 0, None) == INVALID            # ... for the copy too
    assert f(ws, q(n, U16, 8) - 1, kin, kout, vin, vout, n, U16, 8, 0, 16, 0, None) == INVALID
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, 0, 9, 0, None) == INVALID                # end_bit beyond the key
    assert f(ws, nbu16, kin, kout, None, None, n, U16, 0, 0, 17, 0, None) == INVALID
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, 5, 4, 0, None) == INVALID                # begin_bit > end_bit
    assert f(ws, nb, kin, kout, None, None, n, U8, 0, -1, 4, 0, None) == INVALID
    assert f(ws, 1 << 62, kin, kout, None, None, 1 << 40, U8, 0, 0, 8, 0, None) == INVALID     # num_items = 2^40
    assert f(ws, 1 << 62, kin, kout, None, None, (1 << 40) + 1, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, nb, kin, kin, None, None, n, U8, 0, 0, 8, 0, None) == INVALID                 # input == output
    assert f(ws, nb4, kin, kout, vin, vin, n, U8, 4, 0, 8, 0, None) == INVALID
    assert f(ws, nb, kin, kin + n - 1, None, None, n, U8, 0, 0, 8, 0, None) == INVALID         # the arrays share one byte
    assert f(ws, nb, kin + n - 1, kin, None, None, n, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, nbu16, kin, kin + 2 * n - 2, None, None, n, U16, 0, 0, 16, 0, None) == INVALID   # ... at the keys' size
    assert f(ws, nb4, kin, kout, vin, vin + 4 * n - 4, n, U8, 4, 0, 8, 0, None) == INVALID        # ... at the values' size
    assert f(ws, nb4, kin, kout, kout + n - 4, vout, n, U8, 4, 0, 8, 0, None) == INVALID          # keys out and values in
    assert f(ws, nb4, kin, kout, vin, kin + n - 4, n, U8, 4, 0, 8, 0, None) == INVALID            # keys in and values out
    assert f(ws, nb, kin, kout, vin, vout, n, U8, 0, 0, 8, 0, None) == INVALID                 # values given with val_bytes 0
    assert f(ws, nb4, kin, kout, None, None, n, U8, 4, 0, 8, 0, None) == INVALID               # values missing
    assert f(ws, nb4, kin, kout, vin, None, n, U8, 4, 0, 8, 0, None) == INVALID
    assert f(ws, nb4, kin, kout, None, vout, n, U8, 4, 0, 8, 0, None) == INVALID
    assert f(ws, nb, None, kout, None, None, n, U8, 0, 0, 8, 0, None) == INVALID               # keys missing
    assert f(ws, nb, kin, None, None, None, n, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, nb16, kin, kout, vin + 8, vout, n, U8, 16, 0, 8, 0, None) == INVALID          # misaligned 16-byte values
    assert f(ws, nb16, kin, kout, vin, vout + 4, n, U8, 16, 0, 8, 0, None) == INVALID
    assert f(ws, nb4, kin, kout, vin + 2, vout, n, U8, 4, 0, 8, 0, None) == INVALID            # misaligned 4-byte values
    assert f(ws, nbu16, kin + 1, kout, None, None, n, U16, 0, 0, 16, 0, None) == INVALID       # odd address for u16 keys
    assert f(ws, nbu16, kin, kout + 1, None, None, n, U16, 0, 0, 16, 0, None) == INVALID
    assert f(ws, 1 << 30, kin, kout, None, None, n, gs.GS_KEY_U32, 0, 0, 8, 0, None) == INVALID   # not a narrow key type
    assert f(ws, 1 << 30, kin, kout, None, None, n, gs.GS_KEY_U64, 0, 0, 8, 0, None) == INVALID
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, U8, 3, 0, 8, 0, None) == INVALID               # not a listed value size
    assert f(ws, 1 << 30, kin, kout, vin, vout, n, U8, 32, 0, 8, 0, None) == INVALID
    # the same refusals above 2^32 elements, where no delegate can answer for it
    big = (1 << 32) + 5
    assert f(ws, q(big, U8, 0) - 1, kin, 0x7000_0000_0000, None, None, big, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, q(big, U8, 0), kin, kin + big - 1, None, None, big, U8, 0, 0, 8, 0, None) == INVALID
    assert f(ws, q(big, U8, 0), kin, 0x7000_0000_0000, None, None, big, U8, 0, 0, 9, 0, None) == INVALID


def test_noops_succeed_with_null_buffers(gs):
    f = gs.lib.gs_lsb_sort_narrow_large
    for kt in _narrow_types(gs):
        for vb in VAL_BYTES:
            assert f(None, 0, None, None, None, None, 0, kt, vb, 0, 8, 0, None) == 0
            assert f(None, 0, None, None, None, None, 0, kt, vb, 3, 3, 1, None) == 0


def test_python_size_query_matches_the_c_query(gs, monkeypatch):
    """DeviceRadixSortLarge on CPU tensors of every narrow dtype: the size query needs no device."""
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    L = gs.DeviceRadixSortLarge
    dts = [(torch.uint8, gs.GS_KEY_U8), (torch.bool, gs.GS_KEY_U8), (torch.int8, gs.GS_KEY_I8), (torch.int16, gs.GS_KEY_I16)]
    if hasattr(torch, "uint16"):
        dts.append((torch.uint16, gs.GS_KEY_U16))
    vals = [(torch.uint8, (), 1), (torch.int16, (), 2), (torch.int32, (), 4), (torch.int64, (), 8), (torch.int64, (2,), 16), (torch.int32, (4,), 16)]
    for n in (10, 100_003):
        for dt, kt in dts:
            dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
            assert L.SortKeys(None, 0, dk, n) == gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, 0)
            assert L.SortKeysDescending(None, 0, dk, n) == gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, 0)
            for vdt, row, vb in vals:
                dv = gs.DoubleBuffer(torch.zeros((n,) + row, dtype=vdt), torch.zeros((n,) + row, dtype=vdt))
                assert L.SortPairs(None, 0, dk, dv, n) == gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb), (dt, vdt, row)
                assert L.SortPairsDescending(None, 0, dk, dv, n) == gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
            dv = gs.DoubleBuffer(torch.zeros((n, 3), dtype=torch.uint8), torch.zeros((n, 3), dtype=torch.uint8))
            with pytest.raises(ValueError, match="3 bytes"):
                L.SortPairs(None, 0, dk, dv, n)
    # the 32- and 64-bit routing is unchanged
    dk = gs.DoubleBuffer(torch.zeros(10, dtype=torch.int32), torch.zeros(10, dtype=torch.int32))
    assert L.SortKeys(None, 0, dk, 10) == gs.lib.gs_lsb_large_temp_bytes(10, 4, 0)
