"""CPU tests of gs_segmented_sort_narrow (segmented sort of 8- and 16-bit keys): the symbols, the host-side sizing, the argument
checks and the Python front end's size query, which all answer before the device is touched.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

INVALID = 1                     # hipErrorInvalidValue
SERVED_VB = (0, 4, 8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_segmented_narrow_temp_bytes", "gs_segmented_sort_narrow", "gs_segmented_narrow_cap")


def _narrow_types(gs):
    return {gs.GS_KEY_U8: 1, gs.GS_KEY_I8: 1, gs.GS_KEY_U16: 2, gs.GS_KEY_I16: 2}


def _other_types(gs):
    return [getattr(gs, "GS_KEY_" + t) for t in ("U32", "I32", "F32", "U64", "I64", "F64")]


def test_declared_exported_and_bound(gs):
    from gpu_sort_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpusort.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for s in NAMES:
        assert re.search(r"\b%s\s*\(" % s, header), s + " is not declared in gpusort.h"
        assert hasattr(raw, s), s
        assert s in _lib.SIGNATURES, s
        assert getattr(gs.lib, s).argtypes is not None
    # the argument list of gs_segmented_sort_wide with (key_type, val_bytes) in place of (key_bytes, val_bytes, ..., key_type)
    assert len(_lib.SIGNATURES["gs_segmented_sort_narrow"][1]) == len(_lib.SIGNATURES["gs_segmented_sort_wide"][1]) - 1


def test_temp_bytes_and_cap(gs):
    q, cap = gs.lib.gs_segmented_narrow_temp_bytes, gs.lib.gs_segmented_narrow_cap
    for kt in _narrow_types(gs):
        for vb in SERVED_VB:
            assert cap(kt, vb) > 0
            prev = 0
            for n in (1, 777, 100003, (1 << 24) + 7, 1 << 28, (1 << 31) - 1):
                b = q(n, kt, vb, 100)
                assert b > 0 and b % 256 == 0 and b >= prev, (kt, vb, n, b)
                prev = b
            prev = 0
            for nseg in (1, 2, 1000, 1 << 20, 1 << 24):
                b = q(1 << 24, kt, vb, nseg)
                assert b > 0 and b % 256 == 0 and b >= prev, (kt, vb, nseg, b)
                prev = b
        for vb in (1, 2, 3, 16):
            assert q(100003, kt, vb, 10) == 0 and cap(kt, vb) == 0, (kt, vb)
    for kt in _other_types(gs) + [99, -1]:
        for vb in SERVED_VB:
            assert q(100003, kt, vb, 10) == 0 and cap(kt, vb) == 0, (kt, vb)


def test_workspace_holds_no_elements(gs):
    """the lists only: far below the keys' own bytes at sizes that matter"""
    q = gs.lib.gs_segmented_narrow_temp_bytes
    n = 1 << 28
    assert q(n, gs.GS_KEY_U8, 0, 1 << 10) * 2 < n


def test_argument_validation_without_gpu(gs):
    # these return hipErrorInvalidValue (1) before touching the device: the pointers are never dereferenced
    f, q = gs.lib.gs_segmented_sort_narrow, gs.lib.gs_segmented_narrow_temp_bytes
    U8, I16 = gs.GS_KEY_U8, gs.GS_KEY_I16
    n, nseg = 100000, 10
    ws, ob, oe = 0x10000, 0x900000, 0xA00000
    keys = (C.c_void_p * 2)(0x200000, 0x300000)
    vals = (C.c_void_p * 2)(0x400000, 0x500000)

    def call(d_temp=ws, nbytes=None, k=keys, v=None, selector=0, items=n, segs=nseg, b=ob, e=oe, kt=U8, vb=0, bb=0, eb=8):
        sel = C.c_int(selector)
        nbytes = max(q(items, kt, vb, segs), 1 << 24) if nbytes is None else nbytes
        r = f(d_temp, nbytes, k, v, C.byref(sel), items, segs, b, e, kt, vb, bb, eb, 0, None)
        assert sel.value == selector
        return r

    assert call(d_temp=None) == INVALID                                           # no workspace
    assert call(nbytes=0) == INVALID
    assert call(nbytes=q(n, U8, 0, nseg) - 1) == INVALID                          # one byte short
    assert call(nbytes=q(n, I16, 8, nseg) - 1, kt=I16, vb=8, v=vals, eb=16) == INVALID
    assert call(selector=2) == INVALID and call(selector=-1) == INVALID
    assert f(ws, 1 << 24, keys, None, None, n, nseg, ob, oe, U8, 0, 0, 8, 0, None) == INVALID     # no selector
    assert call(k=None) == INVALID
    assert call(k=(C.c_void_p * 2)(0x200000, None)) == INVALID                    # a missing half
    assert call(k=(C.c_void_p * 2)(None, 0x300000)) == INVALID
    assert call(v=(C.c_void_p * 2)(0x400000, None), vb=4) == INVALID
    assert call(v=vals, vb=0) == INVALID                                          # values without val_bytes
    assert call(v=None, vb=4) == INVALID                                          # val_bytes without values
    assert call(eb=9) == INVALID and call(kt=I16, eb=17) == INVALID               # past the key's width
    assert call(bb=5, eb=4) == INVALID and call(bb=-1, eb=4) == INVALID
    assert call(items=1 << 31, nbytes=1 << 40) == INVALID
    assert call(b=None) == INVALID and call(e=None) == INVALID
    for kt in _other_types(gs):
        assert call(kt=kt, nbytes=1 << 30) == INVALID
    for vb in (1, 2, 3, 16):
        assert call(v=vals, vb=vb, nbytes=1 << 30) == INVALID
    assert call(kt=I16, eb=16, k=(C.c_void_p * 2)(0x200001, 0x300000)) == INVALID     # odd address for 16-bit keys
    assert call(v=(C.c_void_p * 2)(0x400002, 0x500000), vb=4) == INVALID              # values not at a multiple of their size


def test_noops_succeed_with_null_buffers(gs):
    f = gs.lib.gs_segmented_sort_narrow
    nul = (C.c_void_p * 2)(None, None)
    for kt, kb in _narrow_types(gs).items():
        for vb in SERVED_VB:
            for sel0 in (0, 1):
                for items, segs, bb, eb in ((0, 5, 0, 8 * kb), (1000, 0, 0, 8 * kb), (1000, 5, 3, 3), (0, 0, 8 * kb, 8 * kb)):
                    sel = C.c_int(sel0)
                    assert f(None, 0, nul, nul if vb else None, C.byref(sel), items, segs, None, None, kt, vb, bb, eb, 1, None) == 0
                    assert sel.value == sel0
                    sel = C.c_int(sel0)
                    assert f(None, 0, None, None, C.byref(sel), items, segs, None, None, kt, vb, bb, eb, 0, None) == 0
                    assert sel.value == sel0


def _dtypes():
    d = [(torch.uint8, "GS_KEY_U8"), (torch.bool, "GS_KEY_U8"), (torch.int8, "GS_KEY_I8"), (torch.int16, "GS_KEY_I16")]
    if hasattr(torch, "uint16"):
        d.append((torch.uint16, "GS_KEY_U16"))
    return d


def test_front_end_size_query_on_cpu_tensors(gs):
    S = gs.DeviceSegmentedRadixSort
    n, nseg = 123457, 321
    offs = torch.zeros(nseg + 1, dtype=torch.int32)
    for dt, ktname in _dtypes():
        kt = getattr(gs, ktname)
        dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
        assert S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_narrow_temp_bytes(n, kt, 0, nseg) > 0
        assert S.SortKeysDescending(None, 0, dk, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_narrow_temp_bytes(n, kt, 0, nseg)
        for vdt, vb in ((torch.int32, 4), (torch.float32, 4), (torch.int64, 8)):
            dv = gs.DoubleBuffer(torch.zeros(n, dtype=vdt), torch.zeros(n, dtype=vdt))
            want = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, nseg)
            assert S.SortPairs(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:]) == want > 0
            assert S.SortPairsDescending(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:]) == want
        for vdt in (torch.int16, torch.uint8):
            dv = gs.DoubleBuffer(torch.zeros(n, dtype=vdt), torch.zeros(n, dtype=vdt))
            with pytest.raises(ValueError, match="%d bytes" % dv.d_buffers[0].element_size()):
                S.SortPairs(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:])


def test_front_end_size_query_of_wider_keys_is_unchanged(gs):
    S = gs.DeviceSegmentedRadixSort
    n, nseg = 123457, 321
    offs = torch.zeros(nseg + 1, dtype=torch.int32)
    k32 = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32))
    k64 = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64))
    v32 = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32))
    v64 = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64))
    assert S.SortKeys(None, 0, k32, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_temp_bytes(n, 0, nseg)
    assert S.SortPairs(None, 0, k32, v32, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_temp_bytes(n, 1, nseg)
    assert S.SortPairs(None, 0, k32, v64, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_wide_temp_bytes(n, 4, 8, nseg)
    assert S.SortKeys(None, 0, k64, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_wide_temp_bytes(n, 8, 0, nseg)
    assert S.SortPairs(None, 0, k64, v32, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_wide_temp_bytes(n, 8, 4, nseg)
    assert S.SortPairs(None, 0, k64, v64, n, nseg, offs[:-1], offs[1:]) == gs.lib.gs_segmented_wide_temp_bytes(n, 8, 8, nseg)


def test_half_precision_keys_are_refused(gs):
    """float16 / bfloat16 keys have no key category: refused with and without an explicit key_type, nothing is sent down"""
    S = gs.DeviceSegmentedRadixSort
    n, nseg = 1000, 3
    offs = torch.zeros(nseg + 1, dtype=torch.int32)
    for dt in (torch.float16, torch.bfloat16):
        dk = gs.DoubleBuffer(torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt))
        for kt in (None, gs.GS_KEY_U16, gs.GS_KEY_I16):
            with pytest.raises(TypeError, match="no key category"):
                S.SortKeys(None, 0, dk, n, nseg, offs[:-1], offs[1:], key_type=kt)
