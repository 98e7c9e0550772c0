"""GPU tests of gs_lsb_sort_narrow_large (8- and 16-bit keys above 2^32 elements), of DeviceRadixSortLarge on such keys and of
the lsb_large driver's narrow modes.

Small arrays take the 64-bit passes through the test hook GS_MSB_LARGE_TEST_LIMIT=k (read on every call), which lowers the slice
size to k elements.  k is a slice of one partial tile (256) or sits on a tile edge of one of the three tile sizes (2048, 4096,
8192 elements for values of 16, 8 and <= 4 bytes); the odd values put every later slice of a u8 array, or of a 1-byte value
array, on an unaligned address.  n = q * k + 1: q full slices and a last slice of one element.

Every case has two witnesses.  The expectation is numpy's stable argsort of the key's order-preserving map masked to the bit
range (descending: the complement of the masked map): keys and values are compared bit for bit.  And gs_lsb_sort_narrow, which
knows nothing of the hook, sorts the same input into buffers of its own, which must come out byte for byte the same (a stable
sort's result is unique).  Sizes above 2^32 run in a child process (tools/narrow_large_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from guarded import Arena, FILLS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_ENV = "GS_MSB_LARGE_TEST_LIMIT"
INVALID = 1
KEY_KINDS = {"u8": ("GS_KEY_U8", 8, False), "i8": ("GS_KEY_I8", 8, True), "u16": ("GS_KEY_U16", 16, False), "i16": ("GS_KEY_I16", 16, True)}
VAL_BYTES = (0, 1, 2, 4, 8, 16)
LIMITS = (256, 2047, 2048, 2049, 4096, 8191, 8192, 8193, 32768)
INPUTS = ("equal", "two", "sorted", "reverse", "every", "and2")


def _utype(bits):
    return np.uint8 if bits == 8 else np.uint16


def tile_of(vb):
    return 8192 if vb <= 4 else (4096 if vb == 8 else 2048)


def n_for(k):
    q = 40 if k < 4096 else (25 if k < 32768 else 20)
    return q * k + 1


def gen_keys(kind, n, inp, seed):
    """unsigned bit patterns of n keys"""
    _, bits, signed = KEY_KINDS[kind]
    card = 1 << bits
    rng = np.random.default_rng(seed)
    if inp == "uniform":
        raw = rng.integers(0, card, size=n, dtype=np.uint32)
    elif inp == "and2":
        raw = rng.integers(0, card, size=n, dtype=np.uint32) & rng.integers(0, card, size=n, dtype=np.uint32)
    elif inp == "equal":                                    # one run that spans every slice
        raw = np.full(n, int(rng.integers(0, card)), dtype=np.uint32)
    elif inp == "two":
        a, b = (int(x) for x in rng.choice(card, size=2, replace=False))
        raw = np.where(rng.integers(0, 2, size=n) == 1, a, b).astype(np.uint32)
    elif inp in ("sorted", "reverse"):
        sign = np.uint32(1 << (bits - 1)) if signed else np.uint32(0)
        raw = np.sort(rng.integers(0, card, size=n, dtype=np.uint32) ^ sign) ^ sign
        if inp == "reverse":
            raw = raw[::-1].copy()
    elif inp == "every":                                    # every value of the type, as evenly as n allows
        raw = rng.permutation(np.arange(n, dtype=np.uint32) % np.uint32(card))
    else:
        raise ValueError(inp)
    return raw.astype(_utype(bits))


def gen_vals(n, vb, seed):
    """(n, vb) uint8: row indices where the size allows (stability is visible), random bytes otherwise"""
    rng = np.random.default_rng(seed + 1)
    if vb == 0:
        return None
    if vb in (1, 2):
        return rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
    if vb == 4:
        return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    if vb == 8:
        return np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    v = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    v[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    return v


def stable_order(kind, keys, bb, eb, desc):
    _, bits, signed = KEY_KINDS[kind]
    m = keys.astype(np.uint32)
    if signed:
        m = m ^ np.uint32(1 << (bits - 1))
    mask = np.uint32((1 << (eb - bb)) - 1)
    m = (m >> np.uint32(bb)) & mask
    if desc:
        m = ~m & mask
    return np.argsort(m, kind="stable")


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(cuda)


def narrow_witness(gs, cuda, kt, vb, keys, vals, bb, eb, desc):
    """gs_lsb_sort_narrow (the parent's code: it never reads the hook) on the same input: (key bytes, value bytes)"""
    n = keys.size
    nb = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    tk = _dev(keys, cuda)
    ok = torch.empty_like(tk)
    tv = _dev(vals, cuda) if vb else None
    ov = torch.empty_like(tv) if vb else None
    err = gs.lib.gs_lsb_sort_narrow(ws.data_ptr(), nb, tk.data_ptr(), ok.data_ptr(), tv.data_ptr() if vb else None,
                                    ov.data_ptr() if vb else None, n, kt, vb, bb, eb, int(desc), None)
    assert err == 0
    torch.cuda.synchronize()
    return ok.cpu().numpy(), (ov.cpu().numpy() if vb else None)


def run_case(gs, cuda, kind, vb, n, bb, eb, desc, inp="uniform", seed=1, koff=0, voff=0, wsoff=0, fill="ff"):
    """One call in a guarded arena: result against numpy and against gs_lsb_sort_narrow, guards intact, inputs unchanged."""
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb = getattr(gs, ktname), bits // 8
    keys, vals = gen_keys(kind, n, inp, seed), gen_vals(n, vb, seed)
    nb = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
    assert nb > 0 and nb % 256 == 0
    A = Arena(cuda, seed=seed)
    A.add("kin", n * kb, koff, data=keys, const=True).add("kout", n * kb, koff, fill=fill)
    if vb:
        A.add("vin", n * vb, voff, data=vals, const=True).add("vout", n * vb, voff, fill=fill)
    A.add("ws", nb, wsoff, fill=fill)
    A.build()
    err = gs.lib.gs_lsb_sort_narrow_large(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if vb else None,
                                          A.ptr("vout") if vb else None, n, kt, vb, bb, eb, int(desc), None)
    tag = (kind, vb, n, bb, eb, desc, inp, koff, voff, wsoff, fill, os.environ.get(LIMIT_ENV))
    assert err == 0, tag
    A.check()                                               # guards intact, inputs byte-identical
    order = stable_order(kind, keys, bb, eb, desc)
    gk = A.read("kout", _utype(bits), n)
    assert np.array_equal(gk, keys[order]), ("keys", tag, int(np.argmax(gk != keys[order])))
    gv = None
    if vb:
        gv = A.read("vout", np.uint8).reshape(n, vb)
        assert np.array_equal(gv, vals[order]), ("values", tag, int(np.argmax((gv != vals[order]).any(axis=1))))
    wk, wv = narrow_witness(gs, cuda, kt, vb, keys, vals, bb, eb, desc)
    assert np.array_equal(wk, gk.view(np.uint8)), ("keys differ from gs_lsb_sort_narrow", tag)
    if vb:
        assert np.array_equal(wv, gv.reshape(-1)), ("values differ from gs_lsb_sort_narrow", tag)


# ------------------------------------------------------------------------------------------------- the 64-bit pass --
def _limits_for(i, vb):
    """the three edges of this value size's tile (4096 has its neighbours added), the one-partial-tile slice, the largest, and
    one more of the list by rotation"""
    t = tile_of(vb)
    return sorted({t - 1, t, t + 1, 256, 32768, LIMITS[i % len(LIMITS)]})


ALL_BITS = [(kind, vb, k) for i, kind in enumerate(KEY_KINDS) for j, vb in enumerate(VAL_BYTES) for k in _limits_for(6 * i + j, vb)]


@pytest.mark.parametrize("kind,vb,limit", ALL_BITS)
def test_every_combination_both_orders(gs, cuda, monkeypatch, kind, vb, limit):
    monkeypatch.setenv(LIMIT_ENV, str(limit))
    bits = KEY_KINDS[kind][1]
    for desc in (False, True):
        run_case(gs, cuda, kind, vb, n_for(limit), 0, bits, desc, seed=limit + vb + int(desc))


def _ranges(bits):
    r = [(0, 8), (1, 8), (3, 5), (4, 4)]
    return r + [(0, 16), (1, 16), (7, 9), (8, 16)] if bits == 16 else r


@pytest.mark.parametrize("vb", (0, 1, 8))
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_bit_ranges(gs, cuda, monkeypatch, kind, vb):
    """the fill path ((0, 8) of 8-bit keys alone), the copy ((4, 4)), one digit pass and two"""
    for i, (bb, eb) in enumerate(_ranges(KEY_KINDS[kind][1])):
        limit = (4096, 2049, 8193)[i % 3]
        monkeypatch.setenv(LIMIT_ENV, str(limit))
        for desc in (False, True):
            run_case(gs, cuda, kind, vb, n_for(limit), bb, eb, desc, inp=("uniform", "and2")[i % 2], seed=20 + i)


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_inputs(gs, cuda, monkeypatch, kind, inp):
    """`equal` is the stability-across-slices case: one run spans every slice, and the row ids must come out 0, 1, 2, ..."""
    bits = KEY_KINDS[kind][1]
    for vb, limit in ((0, 8193), (8, 4096), (1, 2047)):
        monkeypatch.setenv(LIMIT_ENV, str(limit))
        n = n_for(limit) if inp != "every" or bits == 8 else 3 * 65536 + 1
        for desc in (False, True):
            run_case(gs, cuda, kind, vb, n, 0, bits, desc, inp=inp, seed=31)
        run_case(gs, cuda, kind, vb, n, 1, bits - 1, True, inp=inp, seed=32)


@pytest.mark.parametrize("kind", ["u8", "i8"])
def test_fill_path_at_output_offsets(gs, cuda, monkeypatch, kind):
    """8-bit keys alone over all 8 bits: the output 1, 7 and 15 bytes past a 16-byte boundary, arrays shorter than, equal to and
    just longer than one 16-byte chunk (the one-slice route) and the multi-slice size (the 64-bit counts), both orders"""
    limit = 2049
    monkeypatch.setenv(LIMIT_ENV, str(limit))
    for koff in (1, 7, 15):
        for n in (1, 15, 16, 17, n_for(limit)):
            for desc in (False, True):
                for inp in ("and2", "two") if n > 17 else ("uniform",):
                    run_case(gs, cuda, kind, 0, n, 0, 8, desc, inp=inp, seed=koff + n, koff=koff, wsoff=koff, fill=FILLS[(koff + n) % 3])


# ------------------------------------------------------------------------------------------------ buffer contract --
def _placements(elem):
    return (0, 1, 3, 7) if elem == 1 else (0, 2, 6) if elem == 2 else (0, elem)


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_buffer_contract(gs, cuda, monkeypatch, kind, vb):
    """keys and values at every listed byte offset from a 256-byte boundary, the workspace 0, 1 and 255 bytes off, outputs and
    workspace pre-filled with each fill (0xFF among them): result exact, guards intact, inputs untouched (run_case checks all
    three).  The arena puts a guard right behind the queried workspace, so no byte past the query is written."""
    bits = KEY_KINDS[kind][1]
    limit = tile_of(vb) + 1
    monkeypatch.setenv(LIMIT_ENV, str(limit))
    i = 0
    for koff in _placements(bits // 8):
        for voff in (_placements(vb) if vb else (0,)):
            wsoff = (0, 1, 255)[i % 3]
            full = i % 2 == 0
            run_case(gs, cuda, kind, vb, 5 * limit + 1000 + 37 * i, 0 if full else 1, bits if full else bits - 1, bool(i & 2), inp="and2",
                     seed=300 + i, koff=koff, voff=voff, wsoff=wsoff, fill=FILLS[i % 3])
            i += 1
    for fill in FILLS:              # each fill on the dirtiest placement
        run_case(gs, cuda, kind, vb, 3 * limit + 5, 0, bits, True, seed=401, fill=fill, koff=bits // 8, voff=vb, wsoff=255)


@pytest.mark.parametrize("kind,vb", [("u8", 0), ("u8", 4), ("u16", 2), ("i16", 16)])
def test_refused_call_writes_nothing(gs, cuda, monkeypatch, kind, vb):
    monkeypatch.setenv(LIMIT_ENV, "2048")
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n = getattr(gs, ktname), bits // 8, 50_001
    nb = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
    for fill in FILLS:
        A = Arena(cuda, seed=3, all_const=True)
        A.add("kin", n * kb, 0, data=gen_keys(kind, n, "uniform", 1)).add("kout", n * kb, 0, fill=fill)
        if vb:
            A.add("vin", n * vb, 0, data=gen_vals(n, vb, 1)).add("vout", n * vb, 0, fill=fill)
        A.add("ws", nb, 1, fill=fill)
        A.build()
        f = gs.lib.gs_lsb_sort_narrow_large
        ws, ki, ko = A.ptr("ws"), A.ptr("kin"), A.ptr("kout")
        vi, vo = (A.ptr("vin"), A.ptr("vout")) if vb else (None, None)
        assert f(ws, nb - 1, ki, ko, vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(None, nb, ki, ko, vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(ws, nb, ki, ko, vi, vo, n, kt, vb, 0, bits + 1, 0, None) == INVALID
        assert f(ws, nb, ki, ko, vi, vo, n, kt, vb, 3, 2, 0, None) == INVALID
        assert f(ws, nb, ki, ki, vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(ws, nb, ki, ki + (n - 1) * kb, vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID      # one shared element
        assert f(ws, nb, ki, ko, vi, vo, n, kt, 3, 0, bits, 0, None) == INVALID
        assert f(ws, nb, ki, ko, vi, vo, n, gs.GS_KEY_U32, vb, 0, 8, 0, None) == INVALID
        assert f(ws, 1 << 62, ki, ko, vi, vo, 1 << 40, kt, vb, 0, bits, 0, None) == INVALID
        if vb:
            assert f(ws, nb, ki, ko, vi, None, n, kt, vb, 0, bits, 0, None) == INVALID
            assert f(ws, nb, ki, ko, vi, vi, n, kt, vb, 0, bits, 0, None) == INVALID
            assert f(ws, nb, ki, ko, vi, vi + (n - 1) * vb, n, kt, vb, 0, bits, 0, None) == INVALID
        else:
            assert f(ws, nb, ki, ko, ki, ko, n, kt, 0, 0, bits, 0, None) == INVALID
        if kb == 2:
            assert f(ws, nb, ki + 1, ko, vi, vo, n - 1, kt, vb, 0, bits, 0, None) == INVALID
        if vb == 16:
            assert f(ws, nb, ki, ko, vi + 8, vo, n - 1, kt, vb, 0, bits, 0, None) == INVALID
        A.check()


@pytest.mark.parametrize("kind,vb", [("u8", 0), ("i8", 4), ("u16", 0), ("i16", 8), ("u8", 1)])
def test_one_workspace_two_sorts_back_to_back(gs, cuda, monkeypatch, kind, vb):
    """two sorts of different inputs, sizes, bit ranges and orders follow each other on a non-default stream with one (dirty)
    workspace and no synchronisation"""
    monkeypatch.setenv(LIMIT_ENV, "8191")
    ktname, bits, _ = KEY_KINDS[kind]
    kt = getattr(gs, ktname)
    calls = [(200_003, 0, bits, False, "uniform"), (70_001, 1, bits - 1, True, "and2")]
    nb = max(gs.lib.gs_lsb_narrow_large_temp_bytes(c[0], kt, vb) for c in calls)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=cuda)
    ins, outs = [], []
    for j, (n, bb, eb, desc, inp) in enumerate(calls):
        keys, vals = gen_keys(kind, n, inp, 50 + j), gen_vals(n, vb, 60 + j)
        tk, tv = _dev(keys, cuda), (_dev(vals, cuda) if vb else None)
        ins.append((keys, vals, tk, tv))
        outs.append((torch.empty_like(tk), torch.empty_like(tv) if vb else None))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=cuda)
    for j, (n, bb, eb, desc, inp) in enumerate(calls):
        (_, _, tk, tv), (ok, ov) = ins[j], outs[j]
        err = gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), nb, tk.data_ptr(), ok.data_ptr(), tv.data_ptr() if vb else None,
                                              ov.data_ptr() if vb else None, n, kt, vb, bb, eb, int(desc), C.c_void_p(stream.cuda_stream))
        assert err == 0
    stream.synchronize()
    for j, (n, bb, eb, desc, inp) in enumerate(calls):
        order = stable_order(kind, ins[j][0], bb, eb, desc)
        assert np.array_equal(outs[j][0].cpu().numpy().view(_utype(bits)), ins[j][0][order]), (kind, vb, j)
        if vb:
            assert np.array_equal(outs[j][1].cpu().numpy().reshape(n, vb), ins[j][1][order]), (kind, vb, j)


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_without_the_hook_same_bytes_as_the_plain_sort(gs, cuda, monkeypatch, kind, vb):
    """Arrays of one slice take gs_lsb_sort_narrow: the same bytes as a direct call.  (Plain tensors, not an arena: without the
    hook the workspace holds a spine for a slice of 2^31 elements, up to 1 GiB.)"""
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    ktname, bits, _ = KEY_KINDS[kind]
    kt = getattr(gs, ktname)
    for n, bb, eb, desc, inp in [(100_003, 0, bits, False, "and2"), (100_003, 1, bits - 1, True, "uniform"), (777, 3, 3, False, "uniform")]:
        keys, vals = gen_keys(kind, n, inp, 70 + n % 7), gen_vals(n, vb, 71)
        nb = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
        assert nb >= gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
        ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
        tk, tv = _dev(keys, cuda), (_dev(vals, cuda) if vb else None)
        ok, ov = torch.zeros_like(tk), (torch.zeros_like(tv) if vb else None)
        err = gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), nb, tk.data_ptr(), ok.data_ptr(), tv.data_ptr() if vb else None,
                                              ov.data_ptr() if vb else None, n, kt, vb, bb, eb, int(desc), None)
        assert err == 0
        torch.cuda.synchronize()
        del ws
        wk, wv = narrow_witness(gs, cuda, kt, vb, keys, vals, bb, eb, desc)
        order = stable_order(kind, keys, bb, eb, desc)
        assert np.array_equal(ok.cpu().numpy(), wk) and np.array_equal(wk.view(_utype(bits)), keys[order]), (kind, vb, n, bb, eb)
        if vb:
            assert np.array_equal(ov.cpu().numpy(), wv) and np.array_equal(wv.reshape(n, vb), vals[order]), (kind, vb, n, bb, eb)


# ------------------------------------------------------------------------------------------------------- capture --
def test_capture_and_replay(gs, cuda, monkeypatch):
    """One multi-slice (u8, u32) call captured into a graph on a side stream (a linear chain of kernels); replayed on fresh input
    copied into the same buffers, it gives what an eager call gives."""
    monkeypatch.setenv(LIMIT_ENV, "8192")
    n, kt, vb = 100_003, gs.GS_KEY_U8, 4
    k0, k1 = torch.empty(n, dtype=torch.uint8, device=cuda), torch.empty(n, dtype=torch.uint8, device=cuda)
    v0, v1 = torch.empty(n, dtype=torch.int32, device=cuda), torch.empty(n, dtype=torch.int32, device=cuda)
    nbytes = gs.lib.gs_lsb_narrow_large_temp_bytes(n, kt, vb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    k0.copy_(_dev(gen_keys("u8", n, "uniform", 1), cuda))
    v0.copy_(torch.arange(n, dtype=torch.int32, device=cuda))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            rc = gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), nbytes, k0.data_ptr(), k1.data_ptr(), v0.data_ptr(), v1.data_ptr(), n, kt,
                                                 vb, 0, 8, 1, s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert rc == 0
    for rep in range(3):
        keys = gen_keys("u8", n, ("and2", "two", "uniform")[rep], 10 + rep)
        k0.copy_(_dev(keys, cuda))
        v0.copy_(torch.arange(n, dtype=torch.int32, device=cuda))
        k1.fill_(0)
        v1.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        order = stable_order("u8", keys, 0, 8, True)
        assert np.array_equal(k1.cpu().numpy(), keys[order]), rep
        assert np.array_equal(v1.cpu().numpy().astype(np.int64), order), rep
        assert np.array_equal(k0.cpu().numpy(), keys), rep                         # the input is never written
    del g


# ---------------------------------------------------------------------------------------- public surfaces, driver --
@pytest.mark.parametrize("dt,kind", [(torch.uint8, "u8"), (torch.int8, "i8"), (torch.int16, "i16")])
def test_python_device_radix_sort_large(gs, cuda, monkeypatch, dt, kind):
    """int64 row ids; the result lands in the alternate buffer and the selector flips once, whatever the number of passes"""
    monkeypatch.setenv(LIMIT_ENV, "4096")
    n = 50_001
    bits = KEY_KINDS[kind][1]
    keys = gen_keys(kind, n, "and2", 3)
    L = gs.DeviceRadixSortLarge
    for desc in (False, True):
        for sel0 in (0, 1):
            dk = gs.DoubleBuffer(torch.empty(n, dtype=dt, device=cuda), torch.empty(n, dtype=dt, device=cuda))
            dv = gs.DoubleBuffer(torch.empty(n, dtype=torch.int64, device=cuda), torch.empty(n, dtype=torch.int64, device=cuda))
            dk.selector = dv.selector = sel0
            dk.Current().copy_(_dev(keys, cuda).view(dt))
            dv.Current().copy_(torch.arange(n, dtype=torch.int64, device=cuda))
            fn = L.SortPairsDescending if desc else L.SortPairs
            nbytes = fn(None, 0, dk, dv, n)
            assert nbytes == gs.lib.gs_lsb_narrow_large_temp_bytes(n, getattr(gs, KEY_KINDS[kind][0]), 8)
            fn(torch.empty(nbytes, dtype=torch.uint8, device=cuda), nbytes, dk, dv, n)      # key type from the dtype
            torch.cuda.synchronize()
            order = stable_order(kind, keys, 0, bits, desc)
            assert dk.selector == sel0 ^ 1 and dv.selector == sel0 ^ 1
            assert np.array_equal(dk.Current().cpu().numpy().view(_utype(bits)), keys[order])
            assert np.array_equal(dv.Current().cpu().numpy(), order)
            assert np.array_equal(dk.Alternate().cpu().numpy().view(_utype(bits)), keys)    # the input half is untouched
    dk = gs.DoubleBuffer(_dev(keys, cuda).view(dt), torch.empty(n, dtype=dt, device=cuda))
    nbytes = L.SortKeysDescending(None, 0, dk, n, 1, bits - 1)
    L.SortKeysDescending(torch.empty(nbytes, dtype=torch.uint8, device=cuda), nbytes, dk, n, 1, bits - 1)
    torch.cuda.synchronize()
    assert dk.selector == 1
    assert np.array_equal(dk.Current().cpu().numpy().view(_utype(bits)), keys[stable_order(kind, keys, 1, bits - 1, True)])
    dv = gs.DoubleBuffer(torch.zeros((n, 3), dtype=torch.uint8, device=cuda), torch.zeros((n, 3), dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError, match="3 bytes"):
        L.SortPairs(None, 0, dk, dv, n)


@pytest.mark.parametrize("args", [["u8"], ["u8", "desc"], ["u8", "1:8"], ["i16"], ["i16", "desc", "7:9"], ["u8rowid"], ["u8rowid", "desc"],
                                  ["i16rowid"], ["i16rowid", "desc", "1:16"]])
def test_lsb_large_driver_narrow_modes(args):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "lsb_large")
    out = subprocess.run([exe, str((1 << 22) + 77)] + args, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **{LIMIT_ENV: str(1 << 20)}))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "verified=1" in out.stdout and "disorder=0" in out.stdout


# ------------------------------------------------------------------------------------------------------ above 2^32 --
def test_above_2p32(cuda):
    """u8 keys at 2^32 + 2^21 + 7 with more than 2^32 of one value (the only shape at which a 32-bit count can wrap); (u8, u64 row
    id) at the same size in both orders; u16 keys at 2^32 + 4099 (two passes through the workspace intermediate) -- checked on the
    device in chunks (tools/narrow_large_check.py), in a child process.  The row-id cases hold about 75 GiB."""
    free, _ = torch.cuda.mem_get_info()
    if free < 75 * (1 << 30):
        pytest.skip("needs 75 GiB of free device memory, %.0f GiB free" % (free / (1 << 30)))
    tool = os.path.join(ROOT, "tools", "narrow_large_check.py")
    cases = ["u8_heavy", "u8_rowid", "u8_rowid_desc", "u16_keys"]
    out = subprocess.run([sys.executable, tool] + cases, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("-> OK") == len(cases), out.stdout[-3000:]
