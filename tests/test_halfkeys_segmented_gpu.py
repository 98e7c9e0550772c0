"""GPU tests of gs_segmented_sort_narrow on the float key categories of 8 and 16 bits (GS_KEY_F16 / GS_KEY_BF16 / GS_KEY_F8)
with no, 4-byte or 8-byte values.

One call sorts segments of every size at which the code takes another path -- the one-wave lists (up to 64, 256, 512 and
1024 elements), the two workgroup classes up to the cap, and the partition path with a short last tile -- mixed with empty
segments and gaps.  The expectation, per segment, is numpy's (tests/halfkeys_ref.py): stable argsort of the digit of the
image, complemented when descending; keys and row-id values are compared bit for bit, the selector must have flipped once per
8-bit pass, and every position outside the segments must hold what it held before in both halves of both arrays.

The pad case: a short tile is padded with keys that must rank behind every real key in every pass.  For a float key that is
the preimage of the all-ones image (0x7fff / 0x7f ascending, 0xffff / 0xff descending), not ~xr: the data holds those
patterns, 0x8000 / 0x80, and negative keys in every segment, so a wrong pad shows as a wrong last tile."""
import ctypes as C

import numpy as np
import pytest
import torch

import halfkeys_ref as R
from guarded import Arena, FILLS

pytestmark = pytest.mark.gpu

KINDS = list(R.KINDS)
PADS = {16: (0x7fff, 0xffff, 0x8000), 8: (0x7f, 0xff, 0x80)}


def gen_vals(n, vb):
    return R.row_ids(n, vb)


def seg_keys(kind, n, seed):
    """uniform bits (half of them negative) with the pad patterns at every eighth position or so"""
    bits = R.KINDS[kind][2]
    rng = np.random.default_rng(seed)
    k = R.gen_bits(kind, n, "uniform", seed)
    at = rng.integers(0, 8, size=n) == 0
    k[at] = np.array(PADS[bits], dtype=k.dtype)[rng.integers(0, 3, size=int(at.sum()))]
    return k


def layout(sizes, rng):
    """the sizes in random order, a gap of 0 to 3 elements before each, an empty segment after every third: (begins, ends, n)"""
    sizes = np.asarray(sizes)[rng.permutation(len(sizes))]
    begins, ends, at = [], [], 0
    for i, s in enumerate(sizes.tolist()):
        at += int(rng.integers(0, 4))
        begins.append(at); ends.append(at + s)
        at += s
        if i % 3 == 2:
            begins.append(at); ends.append(at)          # empty
    at += 2
    return np.array(begins, dtype=np.int32), np.array(ends, dtype=np.int32), at


def run_case(gs, cuda, kind, vb, keys, begins, ends, bb, eb, desc, seed=1, koff=0, wsoff=0, fill="ff", sel0=0):
    ktname, _, bits = R.KINDS[kind]
    kt, kb, n, nseg = getattr(gs, ktname), bits // 8, keys.size, begins.size
    vals = gen_vals(n, vb)
    nb = gs.lib.gs_segmented_narrow_temp_bytes(n, kt, vb, nseg)
    assert nb > 0
    A = Arena(cuda, seed=seed)
    A.add("k%d" % sel0, n * kb, koff, data=keys).add("k%d" % (sel0 ^ 1), n * kb, koff, fill=fill)
    if vb:
        A.add("v%d" % sel0, n * vb, 0, data=vals).add("v%d" % (sel0 ^ 1), n * vb, 0, fill=fill)
    A.add("ob", 4 * nseg, 0, data=begins, const=True).add("oe", 4 * nseg, 0, data=ends, const=True)
    A.add("ws", nb, wsoff, fill=fill)
    A.build()
    kp = (C.c_void_p * 2)(A.ptr("k0"), A.ptr("k1"))
    vp = (C.c_void_p * 2)(A.ptr("v0"), A.ptr("v1")) if vb else None
    sel = C.c_int(sel0)
    err = gs.lib.gs_segmented_sort_narrow(A.ptr("ws"), nb, kp, vp, C.byref(sel), n, nseg, A.ptr("ob"), A.ptr("oe"), kt, vb, bb, eb,
                                          int(desc), None)
    tag = (kind, vb, n, nseg, bb, eb, desc, koff, wsoff, fill, sel0)
    assert err == 0, tag
    assert sel.value == sel0 ^ (((eb - bb + 7) // 8) & 1), ("selector", tag)
    A.check()
    perm = np.arange(n, dtype=np.int64)
    inside = np.zeros(n, dtype=bool)
    for lo, hi in zip(begins.tolist(), ends.tolist()):
        if hi > lo:
            perm[lo:hi] = lo + R.order(keys[lo:hi], bits, bb, eb, desc)
            inside[lo:hi] = True
    ut = R.utype(bits)
    fin, oth = sel.value, sel.value ^ 1
    got = {h: A.read("k%d" % h, ut, n) for h in (0, 1)}
    init = {h: A.init["k%d" % h].view(ut) for h in (0, 1)}
    ek = np.where(inside, keys[perm], init[fin])
    if not np.array_equal(got[fin], ek):
        i = int(np.argmax(got[fin] != ek))
        s = int(np.searchsorted(ends, i, side="right"))
        raise AssertionError(("keys", tag, "first difference at", i, "segment", (int(begins[s]), int(ends[s])) if s < nseg else None))
    bad = (got[oth] != init[oth]) & ~inside
    assert not bad.any(), ("key outside every segment written in the other half", tag, int(np.argmax(bad)))
    if vb:
        gv = {h: A.read("v%d" % h, np.uint8).reshape(n, vb) for h in (0, 1)}
        iv = {h: A.init["v%d" % h].reshape(n, vb) for h in (0, 1)}
        ev = np.where(inside[:, None], vals[perm], iv[fin])
        assert np.array_equal(gv[fin], ev), ("values", tag, int(np.argmax((gv[fin] != ev).any(axis=1))))
        bad = (gv[oth] != iv[oth]).any(axis=1) & ~inside
        assert not bad.any(), ("value outside every segment written in the other half", tag, int(np.argmax(bad)))


def path_sizes(gs, kt, vb):
    cap = gs.lib.gs_segmented_narrow_cap(kt, vb)
    assert cap > 0
    return [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, cap - 1, cap, cap + 1, 20000]


@pytest.mark.parametrize("desc", (False, True))
@pytest.mark.parametrize("vb", (0, 4, 8))
@pytest.mark.parametrize("kind", KINDS)
def test_every_path_with_gaps_and_pad_patterns(gs, cuda, kind, vb, desc):
    ktname, _, bits = R.KINDS[kind]
    rng = np.random.default_rng(bits + vb + int(desc))
    begins, ends, n = layout(path_sizes(gs, getattr(gs, ktname), vb), rng)
    keys = seg_keys(kind, n, seed=vb + 7)
    for j, (bb, eb) in enumerate([(0, bits)] + ([(4, 12)] if bits == 16 else [])):
        run_case(gs, cuda, kind, vb, keys, begins, ends, bb, eb, desc, seed=j, koff=(bits // 8) * (1 + 2 * j), wsoff=(3, 255)[j],
                 fill=FILLS[(j + vb) % 3], sel0=j)


@pytest.mark.parametrize("kind", KINDS)
def test_pads_alone_and_negative_last_tiles(gs, cuda, kind):
    """segments that hold nothing but the pad patterns and negative keys, at sizes that leave every class and the partition
    path a short last tile: descending, a pad of ~xr (0x8000 / 0x80) would rank in front of them"""
    ktname, _, bits = R.KINDS[kind]
    kt = getattr(gs, ktname)
    rng = np.random.default_rng(5)
    S = 1 << (bits - 1)
    for vb in (0, 4):
        begins, ends, n = layout([3, 70, 300, 1500, 5000, 8192 + 77, 2 * 8192 + 5], rng)
        pool = np.array(list(PADS[bits]) + [S | 1, S | (S - 2), S | (S >> 1)], dtype=R.utype(bits))
        keys = pool[rng.integers(0, pool.size, size=n)]
        for desc in (True, False):
            run_case(gs, cuda, kind, vb, keys, begins, ends, 0, bits, desc, seed=vb, koff=bits // 8, fill="random")


def test_reference_ranks_the_pad_patterns_at_the_ends():
    """the numpy reference itself (no device): ascending, 0x7fff is the largest key and 0xffff the smallest; descending, the
    complement makes 0xffff the last -- the keys whose image a pad must equal"""
    for bits, (p_asc, p_desc, not_a_pad) in PADS.items():
        allb = np.arange(1 << bits, dtype=np.uint32).astype(R.utype(bits))
        asc, desc = allb[R.order(allb, bits, 0, bits, False)], allb[R.order(allb, bits, 0, bits, True)]
        assert asc[-1] == p_asc and asc[0] == p_desc
        assert desc[-1] == p_desc and desc[0] == p_asc
        assert desc[-1] != not_a_pad and int(np.argmax(desc == not_a_pad)) == (1 << (bits - 1))   # -0.0: in the middle
        assert R.sort_key(np.array([p_asc]), bits, 0, bits, False)[0] == (1 << bits) - 1
        assert R.sort_key(np.array([p_desc]), bits, 0, bits, True)[0] == (1 << bits) - 1


def test_python_front_end(gs, cuda):
    """a float16 tensor sorts with key_type=GS_KEY_F16 and is still refused without it"""
    n, nseg = 30000, 4
    bits_in = seg_keys("f16", n, 11)
    offs = torch.tensor([0, 100, 100, 9000, n], dtype=torch.int32, device=cuda)
    cur = torch.from_numpy(bits_in.view(np.int16).copy()).to(cuda).view(torch.float16)
    dk = gs.DoubleBuffer(cur, torch.zeros_like(cur))
    dv = gs.DoubleBuffer(torch.arange(n, dtype=torch.int32, device=cuda), torch.zeros(n, dtype=torch.int32, device=cuda))
    S = gs.DeviceSegmentedRadixSort
    with pytest.raises(TypeError, match="no key category"):
        S.SortPairs(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:])
    nb = S.SortPairsDescending(None, 0, dk, dv, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_F16)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    S.SortPairsDescending(ws, nb, dk, dv, n, nseg, offs[:-1], offs[1:], key_type=gs.GS_KEY_F16)
    torch.cuda.synchronize()
    gk = dk.Current().view(torch.int16).cpu().numpy().view(np.uint16)
    gv = dv.Current().cpu().numpy()
    o = offs.cpu().numpy()
    for lo, hi in zip(o[:-1], o[1:]):
        if hi > lo:
            p = lo + R.order(bits_in[lo:hi], 16, 0, 16, True)
            assert np.array_equal(gk[lo:hi], bits_in[p]) and np.array_equal(gv[lo:hi], p)
