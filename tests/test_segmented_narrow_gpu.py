"""GPU tests of gs_segmented_sort_narrow through the C ABI: segmented sort of 8- and 16-bit keys (bool / u8 / i8 / u16 / i16)
with no, 4-byte or 8-byte values.

Every case runs in a guarded Arena (tests/guarded.py): u8 arrays at odd byte offsets and u16 arrays at even ones, the
workspace at an arbitrary offset, the alternate halves and the workspace pre-filled, and afterwards every guard byte and every
const input (the offsets) must be intact.  The expectation, per segment, is oracle.lsb_reference_ranks on the key's
order-preserving u32 image (sign bit of the key's own width flipped for signed keys: the rule of
tests/test_narrow_gpu.py::expected); keys and values are compared bit for bit (a stable sort's result is unique), and
every position outside the segments must hold what it held before, in both halves of both arrays.  On a subset the second
witness runs: the image widened to u32 and sorted with row indices by gs_segmented_sort_u32 must give the oracle's
permutation, which is also the native result's.

The two large cases are checked on the device in chunks of at most 2^28 elements (whole-tensor torch operations at larger
sizes have returned wrong entries, tools/lsb_large_bench.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from guarded import Arena, FILLS
from test_narrow_gpu import INPUTS, KEY_KINDS, gen_keys

pytestmark = pytest.mark.gpu

INVALID = 1
CHUNK = 1 << 28
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USED_INPUTS = ("and2", "equal", "every", "uniform", "two")
assert set(USED_INPUTS) <= set(INPUTS)


def _utype(bits):
    return np.uint8 if bits == 8 else np.uint16


def gen_vals(n, vb):
    """(n, vb) uint8 rows holding the row index (stability is visible), or None"""
    if vb == 0:
        return None
    if vb == 4:
        return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    return (np.arange(n, dtype=np.uint64) * np.uint64(0x100000001)).view(np.uint8).reshape(n, 8)


def image(kind, keys):
    _, bits, signed = KEY_KINDS[kind]
    img = keys.astype(np.uint32)
    return img ^ np.uint32(1 << (bits - 1)) if signed else img


def clamped(begins, ends, n):
    """the segments the device sorts: offsets clamped to [0, n], empty and inverted ones dropped"""
    out = []
    for b, e in zip(begins.tolist(), ends.tolist()):
        lo, hi = max(b, 0), min(e, n)
        if hi > lo:
            out.append((lo, hi))
    return out


def expected_perm(oracle, kind, keys, segs, bb, eb, desc):
    """perm[i] = input row that lands at position i (identity outside the segments), and the mask of covered positions"""
    n = keys.size
    img = image(kind, keys)
    perm = np.arange(n, dtype=np.int64)
    inside = np.zeros(n, dtype=bool)
    for lo, hi in segs:
        perm[lo:hi] = lo + oracle.lsb_reference_ranks(img[lo:hi], bb, eb, desc).astype(np.int64)
        inside[lo:hi] = True
    return perm, inside


def with_gaps(rng, n, nseg):
    """nseg segments in order with random gaps between them (some empty), as (begins, ends)"""
    cuts = np.sort(rng.integers(0, n + 1, size=2 * nseg))
    return cuts[0::2].astype(np.int32), cuts[1::2].astype(np.int32)


def adjacent(rng, n, nseg):
    cuts = np.sort(rng.integers(0, n + 1, size=nseg - 1)) if nseg > 1 else np.zeros(0, np.int64)
    offs = np.concatenate([[0], cuts, [n]]).astype(np.int32)
    return offs[:-1].copy(), offs[1:].copy()


def passes_of(bb, eb):
    return (eb - bb + 7) // 8


def run_case(gs, cuda, oracle, kind, vb, keys, begins, ends, bb, eb, desc, seed=1, koff=0, voff=0, wsoff=0, fill="ff",
             alt_keys=None, alt_vals=None, sel0=0, witness=False, tag=None):
    """one call in an arena; checks the return code, the selector, the guards, the segments and every position outside them"""
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n, nseg = getattr(gs, ktname), bits // 8, keys.size, begins.size
    vals = gen_vals(n, vb)
    nb = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, nseg)
    assert nb > 0 and nb % 256 == 0
    cur, alt = "k%d" % sel0, "k%d" % (sel0 ^ 1)
    A = Arena(cuda, seed=seed)
    A.add(cur, n * kb, koff, data=keys)
    if alt_keys is not None:
        A.add(alt, n * kb, koff, data=alt_keys)
    else:
        A.add(alt, n * kb, koff, fill=fill)
    if vb:
        A.add("v%d" % sel0, n * vb, voff, data=vals)
        if alt_vals is not None:
            A.add("v%d" % (sel0 ^ 1), n * vb, voff, data=alt_vals)
        else:
            A.add("v%d" % (sel0 ^ 1), n * vb, voff, fill=fill)
    A.add("ob", 4 * nseg, 0, data=begins.astype(np.int32), const=True).add("oe", 4 * nseg, 0, data=ends.astype(np.int32), const=True)
    A.add("ws", nb, wsoff, fill=fill)
    A.build()
    kp = (C.c_void_p * 2)(A.ptr("k0"), A.ptr("k1"))
    vp = (C.c_void_p * 2)(A.ptr("v0"), A.ptr("v1")) if vb else None
    sel = C.c_int(sel0)
    err = gs.lib.gs_segmented_sort_narrow(A.ptr("ws"), nb, kp, vp, C.byref(sel), n, nseg, A.ptr("ob"), A.ptr("oe"), kt, vb, bb, eb,
                                          int(desc), None)
    tag = (kind, vb, n, nseg, bb, eb, desc, koff, voff, wsoff, fill, sel0) if tag is None else tag
    assert err == 0, tag
    assert sel.value == sel0 ^ (passes_of(bb, eb) & 1), ("selector", tag)
    A.check()
    segs = clamped(begins, ends, n)
    perm, inside = expected_perm(oracle, kind, keys, segs, bb, eb, desc)
    ut = _utype(bits)
    fin = sel.value
    got = {h: A.read("k%d" % h, ut, n) for h in (0, 1)}
    init = {h: A.init["k%d" % h].view(ut) for h in (0, 1)}
    ek = np.where(inside, keys[perm], init[fin])
    assert np.array_equal(got[fin], ek), ("keys", tag, int(np.argmax(got[fin] != ek)))
    oth = fin ^ 1
    bad = (got[oth] != init[oth]) & ~inside
    assert not bad.any(), ("key outside every segment written in the other half", tag, int(np.argmax(bad)))
    if vb:
        gv = {h: A.read("v%d" % h, np.uint8).reshape(n, vb) for h in (0, 1)}
        iv = {h: A.init["v%d" % h].reshape(n, vb) for h in (0, 1)}
        ev = np.where(inside[:, None], vals[perm], iv[fin])
        assert np.array_equal(gv[fin], ev), ("values", tag, int(np.argmax((gv[fin] != ev).any(axis=1))))
        bad = (gv[oth] != iv[oth]).any(axis=1) & ~inside
        assert not bad.any(), ("value outside every segment written in the other half", tag, int(np.argmax(bad)))
    if witness and n:
        wperm = u32_witness(gs, cuda, image(kind, keys), begins, ends, bb, eb, desc)
        assert np.array_equal(wperm[inside], perm[inside]), ("gs_segmented_sort_u32 differs from the oracle", tag)
        assert np.array_equal(keys[wperm][inside], got[fin][inside]), ("keys differ from gs_segmented_sort_u32's order", tag)
        if vb == 4:
            assert np.array_equal(gv[fin].view(np.uint32).reshape(n)[inside], wperm.astype(np.uint32)[inside]), ("values", tag)
    return perm, inside


def u32_witness(gs, cuda, img, begins, ends, bb, eb, desc):
    """the permutation gs_segmented_sort_u32 gives on the widened image with row indices"""
    n, nseg = img.size, begins.size
    k = [torch.from_numpy(img.view(np.int32).copy()).to(cuda), torch.zeros(n, dtype=torch.int32, device=cuda)]
    v = [torch.arange(n, dtype=torch.int32, device=cuda), torch.arange(n, dtype=torch.int32, device=cuda)]
    ob, oe = torch.from_numpy(begins.astype(np.int32)).to(cuda), torch.from_numpy(ends.astype(np.int32)).to(cuda)
    nb = gs.lib.gs_segmented_temp_bytes(n, 1, nseg)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    kp = (C.c_void_p * 2)(k[0].data_ptr(), k[1].data_ptr())
    vp = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr())
    sel = C.c_int(0)
    err = gs.lib.gs_segmented_sort_u32(ws.data_ptr(), nb, kp, vp, C.byref(sel), n, nseg, ob.data_ptr(), oe.data_ptr(), bb, eb, int(desc),
                                       gs.GS_KEY_U32, None)
    assert err == 0
    torch.cuda.synchronize()
    return v[sel.value].cpu().numpy().view(np.uint32).astype(np.int64)


def sub_ranges(bits):
    return [(3, 7)] if bits == 8 else [(4, 12), (0, 8), (8, 16)]


def all_ranges(bits):
    return [(0, bits)] + sub_ranges(bits) + [(bits - 1, bits)]


def _koffs(kb, i):
    return ((1, 3, 7, 0) if kb == 1 else (2, 6, 0, 10))[i % 4]


SHAPES = [(1, 1), (5000, 3), (100003, 1), (100003, 700), (1200007, 5), (1200007, 30000)]


# ------------------------------------------------------------------------------------------------------ 1: oracle parity --
@pytest.mark.parametrize("n,nseg", SHAPES)
@pytest.mark.parametrize("vb", (0, 4, 8))
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_oracle_parity(gs, cuda, oracle, kind, vb, n, nseg):
    """ascending over all bits (adjacent segments), descending with gaps over all bits, the sub-ranges with gaps, a descending
    one-bit range; the input kind, the byte offsets, the fill and the starting selector rotate"""
    bits = KEY_KINDS[kind][1]
    kb = bits // 8
    rng = np.random.default_rng(n * 31 + nseg)
    cases = [((0, bits), False, adjacent(rng, n, nseg)), ((0, bits), True, with_gaps(rng, n, nseg))]
    cases += [(r, bool(j & 1), with_gaps(rng, n, nseg)) for j, r in enumerate(sub_ranges(bits))]
    cases += [((bits - 1, bits), True, adjacent(rng, n, nseg))]
    for i, ((bb, eb), desc, (ob, oe)) in enumerate(cases):
        j = i + vb + n % 5
        keys = gen_keys(kind, n, USED_INPUTS[j % len(USED_INPUTS)], seed=1000 + j)
        run_case(gs, cuda, oracle, kind, vb, keys, ob, oe, bb, eb, desc, seed=j, koff=_koffs(kb, j), voff=(0, vb)[j % 2] if vb else 0,
                 wsoff=(0, 1, 77, 255)[j % 4], fill=FILLS[j % 3], sel0=j & 1, witness=(i < 2 and n <= 100003))


# ---------------------------------------------------------------------------------------------------- 2: every path's edges --
def edge_sizes(gs, kt, vb):
    cap, tile = gs.lib.gs_segmented_narrow_cap(kt, vb), gs.lib.gs_lsb_narrow_tile(kt, vb)
    assert cap > 0 and tile > 0
    return [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, cap - 1, cap, cap + 1, 2 * cap + 1,
            tile - 1, tile, tile + 1, 3 * tile + 1]


@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("vb", (0, 4, 8))
@pytest.mark.parametrize("kind", ("u8", "u16"))
def test_every_paths_edges(gs, cuda, oracle, kind, vb, desc):
    ktname, bits, _ = KEY_KINDS[kind]
    rng = np.random.default_rng(vb + bits)
    sizes = np.array(edge_sizes(gs, getattr(gs, ktname), vb))
    sizes = sizes[rng.permutation(sizes.size)]
    ends = np.cumsum(sizes).astype(np.int32)
    begins = (ends - sizes).astype(np.int32)
    n = int(ends[-1])
    for inp in ("and2", "every"):
        keys = gen_keys(kind, n, inp, seed=vb + 5)
        run_case(gs, cuda, oracle, kind, vb, keys, begins, ends, 0, bits, desc, koff=bits // 8, wsoff=3, fill="random",
                 witness=(inp == "and2"))
    # a segment that starts at every residue of a 16-byte chunk: one-wave, workgroup and level paths
    for size in (40, 700, 3000, int(sizes.max())):
        b = np.array([r * (size + 16) + r for r in range(16)], dtype=np.int32)
        e = b + size
        keys = gen_keys(kind, int(e[-1]) + 5, "uniform", seed=size)
        run_case(gs, cuda, oracle, kind, vb, keys, b, e, 0, bits, desc, koff=0, fill="00")


# ----------------------------------------------------------------------------------------------------------- 3: neighbours --
@pytest.mark.parametrize("kind,vb", [("u8", 0), ("u8", 4), ("u16", 0), ("u16", 4)])
def test_neighbours_one_element_gaps(gs, cuda, oracle, kind, vb):
    """segments of odd sizes separated by gaps of exactly one element; the two halves are pre-filled with different bytes and
    every gap position of both halves of keys and values must hold its pre-fill byte afterwards"""
    bits = KEY_KINDS[kind][1]
    kb = bits // 8
    rng = np.random.default_rng(9)
    cap, tile = gs.lib.gs_segmented_narrow_cap(getattr(gs, KEY_KINDS[kind][0]), vb), gs.lib.gs_lsb_narrow_tile(getattr(gs, KEY_KINDS[kind][0]), vb)
    sizes = np.concatenate([rng.integers(0, 600, size=400) * 2 + 1, [cap - 1, cap + 1, 2 * tile + 1, 3 * cap + 1, 1, 3, 5]])
    sizes = sizes[rng.permutation(sizes.size)]
    begins = (np.cumsum(sizes + 1) - sizes).astype(np.int32)         # one gap element before every segment
    ends = (begins + sizes).astype(np.int32)
    n = int(ends[-1]) + 1
    gap = np.ones(n, dtype=bool)
    for lo, hi in zip(begins, ends):
        gap[lo:hi] = False
    assert gap.sum() == sizes.size + 1
    for sel0 in (0, 1):
        keys = gen_keys(kind, n, "uniform", seed=sel0)
        keys[gap] = np.array([0xA5A5], dtype=np.uint16).astype(keys.dtype)[0]
        alt = np.full(n * kb, 0x3C, dtype=np.uint8)
        altv = np.full(n * vb, 0xC3, dtype=np.uint8) if vb else None
        for bb, eb in ((0, bits), (0, 8)):
            run_case(gs, cuda, oracle, kind, vb, keys, begins, ends, bb, eb, bool(sel0), koff=kb, voff=0, wsoff=1, alt_keys=alt,
                     alt_vals=altv, sel0=sel0)


# -------------------------------------------------------------------------------------------------------- 4: selector rule --
@pytest.mark.parametrize("kind", ("u8", "i8", "u16", "i16"))
def test_selector_rule_and_empty_bit_range(gs, cuda, oracle, kind):
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n = getattr(gs, ktname), bits // 8, 50000
    rng = np.random.default_rng(4)
    ob, oe = with_gaps(rng, n, 9)
    keys = gen_keys(kind, n, "uniform", seed=4)
    for bb, eb in all_ranges(bits):
        for sel0 in (0, 1):
            run_case(gs, cuda, oracle, kind, 4, keys, ob, oe, bb, eb, False, sel0=sel0)     # (asserts the selector)
    for vb in (0, 4):
        for sel0 in (0, 1):
            A = Arena(cuda, seed=1, all_const=True)
            A.add("k0", n * kb, 0, data=keys).add("k1", n * kb, 0, fill="random")
            if vb:
                A.add("v0", n * vb, 0, data=gen_vals(n, vb)).add("v1", n * vb, 0, fill="ff")
            A.add("ob", 4 * 9, 0, data=ob).add("oe", 4 * 9, 0, data=oe)
            A.build()
            kp = (C.c_void_p * 2)(A.ptr("k0"), A.ptr("k1"))
            vp = (C.c_void_p * 2)(A.ptr("v0"), A.ptr("v1")) if vb else None
            sel = C.c_int(sel0)
            assert gs.lib.gs_segmented_sort_narrow(None, 0, kp, vp, C.byref(sel), n, 9, A.ptr("ob"), A.ptr("oe"), kt, vb, 5, 5, 0, None) == 0
            assert sel.value == sel0
            A.check()


# ------------------------------------------------------------------------------------------------ 5: refusals write nothing --
@pytest.mark.parametrize("kind,vb", [("u8", 0), ("i8", 4), ("u16", 8), ("i16", 4)])
def test_refused_calls_write_nothing(gs, cuda, kind, vb):
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n, nseg = getattr(gs, ktname), bits // 8, 20000, 4
    nb = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, nseg)
    ob, oe = np.array([0, 100, 5000, 9000], dtype=np.int32), np.array([100, 4000, 9000, 20000], dtype=np.int32)
    for fill in FILLS:
        A = Arena(cuda, seed=2, all_const=True)
        A.add("k0", n * kb, kb, data=gen_keys(kind, n, "uniform", 1)).add("k1", n * kb, kb, fill=fill)
        if vb:
            A.add("v0", n * vb, 0, data=gen_vals(n, vb)).add("v1", n * vb, 0, fill=fill)
        A.add("ob", 16, 0, data=ob).add("oe", 16, 0, data=oe).add("ws", nb, 1, fill=fill)
        A.build()
        kp = (C.c_void_p * 2)(A.ptr("k0"), A.ptr("k1"))
        vp = (C.c_void_p * 2)(A.ptr("v0"), A.ptr("v1")) if vb else None
        f = gs.lib.gs_segmented_sort_narrow

        def call(ws=A.ptr("ws"), nbytes=nb, keys=kp, vals=vp, selector=0, items=n, b=A.ptr("ob"), e=A.ptr("oe"), key_type=kt, val_bytes=vb,
                 bb=0, eb=bits):
            sel = C.c_int(selector)
            r = f(ws, nbytes, keys, vals, C.byref(sel), items, nseg, b, e, key_type, val_bytes, bb, eb, 0, None)
            assert sel.value == selector
            return r

        assert call(nbytes=nb - 1) == INVALID
        assert call(ws=None) == INVALID
        assert call(key_type=gs.GS_KEY_U32) == INVALID
        assert call(key_type=gs.GS_KEY_F64) == INVALID
        for bad_vb in (1, 2, 3, 16):
            assert call(val_bytes=bad_vb) == INVALID
        assert call(val_bytes=0 if vb else 4) == INVALID                       # values without val_bytes / val_bytes without values
        assert call(eb=bits + 1) == INVALID
        assert call(bb=-1) == INVALID
        assert call(bb=5, eb=4) == INVALID
        assert call(selector=2) == INVALID
        assert call(keys=(C.c_void_p * 2)(A.ptr("k0"), None)) == INVALID
        assert call(keys=(C.c_void_p * 2)(None, A.ptr("k1"))) == INVALID
        if vb:
            assert call(vals=(C.c_void_p * 2)(A.ptr("v0"), None)) == INVALID
        assert call(b=None) == INVALID
        assert call(e=None) == INVALID
        assert call(items=1 << 31) == INVALID
        A.check()


# --------------------------------------------------------------------------------------------------------------- 6: offsets --
@pytest.mark.parametrize("kind,vb", [("u8", 4), ("i16", 0), ("u16", 8)])
def test_offsets_clamped_inverted_empty(gs, cuda, oracle, kind, vb):
    bits = KEY_KINDS[kind][1]
    n = 60001
    begins = np.array([-500, 300, 900, 900, 20000, 5000, 45000, 70000], dtype=np.int32)
    ends = np.array([200, 900, 900, 800, 41000, 4000, 2000000000, 80000], dtype=np.int32)
    assert clamped(begins, ends, n) == [(0, 200), (300, 900), (20000, 41000), (45000, n)]
    keys = gen_keys(kind, n, "and2", seed=6)
    for desc in (False, True):
        run_case(gs, cuda, oracle, kind, vb, keys, begins, ends, 0, bits, desc, koff=bits // 8, wsoff=9, fill="random")


# ------------------------------------------------------------------------------------------------------ 7: shared workspace --
def test_two_sorts_one_workspace_side_stream(gs, cuda, oracle):
    """u8 keys, then (i16, u32) pairs, back to back on a side stream with one workspace and no synchronisation between them"""
    n, nseg = 400009, 300
    rng = np.random.default_rng(7)
    jobs = []
    for kind, vb, desc in (("u8", 0, False), ("i16", 4, True)):
        ktname, bits, _ = KEY_KINDS[kind]
        keys = gen_keys(kind, n, "and2", seed=bits)
        ob, oe = with_gaps(rng, n, nseg)
        ob[0], oe[0] = 0, 40000                                    # a level bucket in both
        ob[1:], oe[1:] = np.maximum(ob[1:], 40000), np.maximum(oe[1:], 40000)
        vals = gen_vals(n, vb)
        k = [torch.from_numpy(keys.view(np.uint8).copy()).to(cuda), torch.zeros(n * bits // 8, dtype=torch.uint8, device=cuda)]
        v = [torch.from_numpy(vals.copy()).to(cuda), torch.zeros((n, vb), dtype=torch.uint8, device=cuda)] if vb else None
        jobs.append((kind, vb, desc, keys, vals, ob, oe, k, v, torch.from_numpy(ob).to(cuda), torch.from_numpy(oe).to(cuda), getattr(gs, ktname), bits))
    nb = max(gs.lib.gs_segmented_narrow_temp_bytes(n, j[11], j[1], nseg) for j in jobs)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=cuda)
    sels = []
    for kind, vb, desc, keys, vals, ob, oe, k, v, dob, doe, kt, bits in jobs:
        kp = (C.c_void_p * 2)(k[0].data_ptr(), k[1].data_ptr())
        vp = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr()) if vb else None
        sel = C.c_int(0)
        assert gs.lib.gs_segmented_sort_narrow(ws.data_ptr(), nb, kp, vp, C.byref(sel), n, nseg, dob.data_ptr(), doe.data_ptr(), kt, vb, 0, bits,
                                               int(desc), C.c_void_p(stream.cuda_stream)) == 0
        sels.append(sel.value)
    stream.synchronize()
    for (kind, vb, desc, keys, vals, ob, oe, k, v, _, _, _, bits), fin in zip(jobs, sels):
        perm, inside = expected_perm(oracle, kind, keys, clamped(ob, oe, n), 0, bits, desc)
        got = k[fin].cpu().numpy().view(_utype(bits))
        assert np.array_equal(got[inside], keys[perm][inside]), (kind, vb)
        if vb:
            assert np.array_equal(v[fin].cpu().numpy()[inside], vals[perm][inside]), (kind, vb)


# ------------------------------------------------------------------------------------------- 8: large, checked on the device --
def _chunks(n):
    return [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]


def _counts(t, card, offset):
    c = torch.zeros(card, dtype=torch.int64, device=t.device)
    for lo, hi in _chunks(t.numel()):
        c += torch.bincount(t.reshape(-1)[lo:hi].to(torch.int64) + offset, minlength=card)
    return c


def _sort_rows(gs, cuda, kt, vb, k, v, rows, cols, bits, desc):
    n = rows * cols
    offs = torch.arange(0, n + 1, cols, dtype=torch.int32, device=cuda)
    nb = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, rows)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=cuda)
    kp = (C.c_void_p * 2)(k[0].data_ptr(), k[1].data_ptr())
    vp = (C.c_void_p * 2)(v[0].data_ptr(), v[1].data_ptr()) if vb else None
    sel = C.c_int(0)
    assert gs.lib.gs_segmented_sort_narrow(ws.data_ptr(), nb, kp, vp, C.byref(sel), n, rows, offs[:-1].data_ptr(), offs[1:].data_ptr(), kt, vb,
                                           0, bits, int(desc), None) == 0
    torch.cuda.synchronize()
    return sel.value


def test_large_rows_u16_with_column_ids_descending(gs, cuda):
    """2048 rows of 131072 u16 keys (torch.int16 holding the bit patterns) with u32 column ids, descending"""
    rows, cols = 2048, 131072
    n = rows * cols
    assert n <= CHUNK
    g = torch.Generator(device=cuda)
    g.manual_seed(8)
    kin = torch.randint(0, 65536, (n,), device=cuda, generator=g, dtype=torch.int32).to(torch.int16)
    vin = torch.arange(cols, dtype=torch.int32, device=cuda).repeat(rows)
    k = [kin.clone(), torch.zeros_like(kin)]
    v = [vin.clone(), torch.zeros_like(vin)]
    fin = _sort_rows(gs, cuda, gs.GS_KEY_U16, 4, k, v, rows, cols, 16, True)
    assert fin == 0                                                 # two passes
    ko = (k[fin].to(torch.int32) & 0xFFFF).view(rows, cols)
    vo = v[fin].view(rows, cols)
    assert bool((ko[:, 1:] <= ko[:, :-1]).all()), "keys of a row out of order"
    assert bool(((vo >= 0) & (vo < cols)).all()), "column id out of range"
    assert bool(((ko[:, 1:] < ko[:, :-1]) | (vo[:, 1:] > vo[:, :-1])).all()), "column ids do not ascend inside a key"
    ki = (kin.to(torch.int32) & 0xFFFF).view(rows, cols)
    assert torch.equal(torch.gather(ki, 1, vo.to(torch.int64)), ko), "the input key at a column id differs from the key that came out"
    assert torch.equal(_counts(ki, 65536, 0), _counts(ko, 65536, 0))


def test_large_2p20_segments_of_256_i8_keys(gs, cuda):
    rows, cols = 1 << 20, 256
    n = rows * cols
    assert n <= CHUNK
    g = torch.Generator(device=cuda)
    g.manual_seed(9)
    kin = torch.randint(0, 256, (n,), device=cuda, generator=g, dtype=torch.int32).to(torch.int8)
    k = [kin.clone(), torch.zeros_like(kin)]
    fin = _sort_rows(gs, cuda, gs.GS_KEY_I8, 0, k, None, rows, cols, 8, False)
    assert fin == 1
    ko = k[fin].view(rows, cols)
    assert bool((ko[:, 1:] >= ko[:, :-1]).all()), "keys of a segment out of order"
    ki = kin.view(rows, cols)
    assert torch.equal(_counts(ki, 256, 128), _counts(ko, 256, 128))
    assert torch.equal(ki.sum(dim=1, dtype=torch.int64), ko.sum(dim=1, dtype=torch.int64)), "a segment's keys changed"
    sq_i, sq_o = ki.to(torch.int32) ** 2, ko.to(torch.int32) ** 2
    assert torch.equal(sq_i.sum(dim=1, dtype=torch.int64), sq_o.sum(dim=1, dtype=torch.int64)), "a segment's keys changed"


# ------------------------------------------------------------------------------------------------------------ 9: front ends --
@pytest.mark.parametrize("dtype", ("int16", "uint8", "bool"))
def test_python_front_end(gs, cuda, oracle, dtype):
    kind = {"int16": "i16", "uint8": "u8", "bool": "bool"}[dtype]
    tdt = getattr(torch, dtype)
    bits = KEY_KINDS[kind][1]
    n, nseg = 250007, 61
    rng = np.random.default_rng(11)
    ob, oe = with_gaps(rng, n, nseg)
    ob[0], oe[0] = 0, 30011
    ob[1:], oe[1:] = np.maximum(ob[1:], 30011), np.maximum(oe[1:], 30011)
    keys = gen_keys(kind, n, "uniform", seed=12)
    segs = clamped(ob, oe, n)
    dob, doe = torch.from_numpy(ob).to(cuda), torch.from_numpy(oe).to(cuda)
    S = gs.DeviceSegmentedRadixSort

    def dev_keys():
        t = torch.from_numpy(keys.view(np.uint8).copy()).to(cuda).view(torch.int16 if bits == 16 else torch.uint8)
        return t.view(tdt) if dtype == "bool" else t.to(tdt) if t.dtype != tdt else t

    for vdt in (torch.int32, torch.int64):
        dk = gs.DoubleBuffer(dev_keys(), torch.zeros(n, dtype=tdt, device=cuda))
        dv = gs.DoubleBuffer(torch.arange(n, dtype=vdt, device=cuda), torch.zeros(n, dtype=vdt, device=cuda))
        nb = S.SortPairs(None, 0, dk, dv, n, nseg, dob, doe)
        assert nb == gs.lib.gs_segmented_narrow_temp_bytes(n, getattr(gs, KEY_KINDS[kind][0]), dv.d_buffers[0].element_size(), nseg)
        ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
        S.SortPairs(ws, nb, dk, dv, n, nseg, dob, doe)
        torch.cuda.synchronize()
        perm, inside = expected_perm(oracle, kind, keys, segs, 0, bits, False)
        assert dk.selector == dv.selector == passes_of(0, bits) & 1
        assert np.array_equal(dk.Current().cpu().numpy().view(_utype(bits))[inside], keys[perm][inside]), (dtype, vdt)
        assert np.array_equal(dv.Current().cpu().numpy().astype(np.int64)[inside], perm[inside]), (dtype, vdt)
    dk = gs.DoubleBuffer(dev_keys(), torch.zeros(n, dtype=tdt, device=cuda))
    nb = S.SortKeysDescending(None, 0, dk, n, nseg, dob, doe)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    S.SortKeysDescending(ws, nb, dk, n, nseg, dob, doe)
    torch.cuda.synchronize()
    perm, inside = expected_perm(oracle, kind, keys, segs, 0, bits, True)
    assert np.array_equal(dk.Current().cpu().numpy().view(_utype(bits))[inside], keys[perm][inside]), dtype
    dv = gs.DoubleBuffer(torch.zeros(n, dtype=torch.int16, device=cuda), torch.zeros(n, dtype=torch.int16, device=cuda))
    with pytest.raises(ValueError, match="2 bytes"):
        S.SortPairs(None, 0, dk, dv, n, nseg, dob, doe)


def test_lsb_types_driver_segmented_narrow_rows():
    """the typed C++ driver (include/gpusort.hpp) in a process of its own: its segmented rows for the four narrow key types"""
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "lsb_types")
    assert os.path.exists(exe), exe + " is not built"
    out = subprocess.run([exe, "200003"], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    assert not any("FAIL" in line for line in out)
    for name in ("u8", "i8", "u16", "i16"):            # unsigned char, signed char, unsigned short, short
        rows = [l for l in out if l.startswith("segmented " + name + " keys,")]
        assert len(rows) >= 3 and all(l.endswith(": CORRECT") for l in rows), (name, rows)
