"""The buffer contract of every sort entry point of the C ABI, with guarded buffers (tests/guarded.py).

Every entry point must write only inside the buffers it was given, accept the alignments its contract allows (a workspace
of any alignment; data arrays at their element's natural alignment) and not depend on what the buffers held before.  One
row per entry point: an adapter places the buffers in an Arena, calls gs.lib.* with raw pointers and checks the result
against a host reference in exact integer arithmetic (numpy's stable argsort of the key type's order-preserving map; for
the unstable MSB family the sorted keys bit for bit, the enumerated values a permutation that names equal keys).

Placements: P0 every buffer on a 256-byte boundary (the control); P1 every data array one element off the boundary (three
for 32-bit arrays) and the workspace one byte off; P2 data on the boundary and the workspace 4, 8, 100 or 255 bytes off.
The workspace is exactly the queried size and its trailing guard starts right behind it.  Fills of workspace, alternates
and outputs: 0xFF and random bytes (and 0x00 for the control)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from guarded import Arena

pytestmark = pytest.mark.gpu

U32, I32, F32, U64, I64, F64, U8, I8, U16, I16 = range(10)
KEY_BYTES = {U32: 4, I32: 4, F32: 4, U64: 8, I64: 8, F64: 8, U8: 1, I8: 1, U16: 2, I16: 2}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
INVALID = 1                     # hipErrorInvalidValue
LIMIT_ENV = "GS_MSB_LARGE_TEST_LIMIT"
BIG = (1 << 21) + 77

PLACEMENTS = {"P0": 0, "P1": 1, "P2+4": 4, "P2+8": 8, "P2+100": 100, "P2+255": 255}   # name -> workspace offset
COMBOS = [("P0", "00"), ("P0", "ff"), ("P0", "random")] + [(p, f) for p in PLACEMENTS if p != "P0" for f in ("ff", "random")]


def data_off(pl, elem_bytes):
    """Byte offset of a data array of elem_bytes elements from the 256-byte boundary under placement pl."""
    if pl != "P1":
        return 0
    return 3 * elem_bytes if elem_bytes == 4 else elem_bytes


# ---------------------------------------------------------------------------------------------------- references --
def ordmap(keys, kt):
    """The key type's order-preserving unsigned map (-0.0 before +0.0, NaNs by their bits), as uint64."""
    bits = 8 * KEY_BYTES[kt]
    k = keys.astype(np.uint64)
    sign = np.uint64(1 << (bits - 1))
    mask = np.uint64((1 << bits) - 1)
    if kt in (I32, I64, I8, I16):
        return k ^ sign
    if kt in (F32, F64):
        return np.where(k & sign != 0, ~k & mask, k | sign)
    return k


def stable_order(keys, kt, begin=0, end=None, descending=False):
    bits = 8 * KEY_BYTES[kt]
    end = bits if end is None else end
    m = (ordmap(keys, kt) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)
    return np.argsort(~m if descending else m, kind="stable")


def check_unstable(keys, kt, got_k, got_v, what):
    exp = keys[stable_order(keys, kt)]
    assert np.array_equal(got_k, exp), what + ": keys differ from the reference"
    if got_v is not None:
        v = got_v.astype(np.int64)
        assert np.array_equal(np.sort(v), np.arange(keys.size)), what + ": values are not a permutation of 0..n-1"
        assert np.array_equal(keys[v], got_k), what + ": a value names a different key"


# ------------------------------------------------------------------------------------------------------- inputs --
KINDS = ["uniform", "few", "pad", "zipf", "special"]


def gen_keys(kt, kind, n, seed):
    kb = KEY_BYTES[kt]
    ut = UINT[kb]
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    if kb < 8:
        full = full >> np.uint64(64 - 8 * kb)
    k = full.astype(ut)
    if kind == "few":
        k = k[:5][rng.integers(0, 5, size=n)] if n >= 5 else k
    elif kind == "pad":                       # all ones: the pad pattern and the 0xFF fill
        k = np.full(n, np.iinfo(ut).max, ut)
    elif kind == "zipf":                      # one heavy hitter with a 0.9 share
        if n:
            k[rng.random(n) < 0.9] = k[0]
    elif kind == "special":
        if kt in (F32, F64):
            ft = np.float32 if kt == F32 else np.float64
            tiny = np.finfo(ft).smallest_subnormal
            sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.nan, -np.nan], ft).view(ut)
            sp = np.concatenate([sp, np.array([0x7FC00001 if kb == 4 else 0x7FF8000000000001], ut)])   # a NaN payload
        else:
            mx = np.iinfo(ut).max
            sp = np.array([0, 1, mx, mx - 1, mx >> 1, (mx >> 1) + 1], ut)     # with the sign bit of the signed types
        idx = rng.random(n) < 0.5
        k[idx] = sp[rng.integers(0, sp.size, size=int(idx.sum()))]
    return k


# ------------------------------------------------------------------------------------------------------- rows --
class Call:
    """One prepared call: query (workspace bytes), launch(ws_ptr, ws_bytes) -> return code, verify(arena)."""

    def __init__(self, query, launch, verify):
        self.query, self.launch, self.verify = query, launch, verify


def _db(arena, a, b):
    return (C.c_void_p * 2)(arena.ptr(a), arena.ptr(b))


def row_lsb_u32(gs, A, tag, n, kind, var, pl, fill, seed):
    kt, pairs, (bb, eb), desc = var
    keys = gen_keys(kt, kind, n, seed)
    vals = np.arange(n, dtype=np.uint32)
    o = data_off(pl, 4)
    A.add(tag + "k0", 4 * n, o, data=keys).add(tag + "k1", 4 * n, o, fill)
    if pairs:
        A.add(tag + "v0", 4 * n, o, data=vals).add(tag + "v1", 4 * n, o, fill)
    sel = C.c_int(0)

    def launch(ws, nbytes):
        return gs.lib.gs_lsb_sort_u32(ws, nbytes, _db(A, tag + "k0", tag + "k1"),
                                      _db(A, tag + "v0", tag + "v1") if pairs else None, C.byref(sel), n, bb, eb, desc, kt, None)

    def verify(A):
        order = stable_order(keys, kt, bb, eb, desc)
        assert np.array_equal(A.read(tag + "k%d" % sel.value, np.uint32), keys[order]), "keys"
        if pairs:
            assert np.array_equal(A.read(tag + "v%d" % sel.value, np.uint32), vals[order]), "values"
    return Call(gs.lib.gs_lsb_temp_bytes(n, int(pairs)), launch, verify)


def row_lsb_copy(gs, A, tag, n, kind, var, pl, fill, seed):
    kt, pairs, (bb, eb), desc = var
    keys = gen_keys(kt, kind, n, seed)
    vals = np.arange(n, dtype=np.uint32)
    o = data_off(pl, 4)
    A.add(tag + "kin", 4 * n, o, data=keys, const=True).add(tag + "kout", 4 * n, o, fill)
    if pairs:
        A.add(tag + "vin", 4 * n, o, data=vals, const=True).add(tag + "vout", 4 * n, o, fill)

    def launch(ws, nbytes):
        return gs.lib.gs_lsb_sort_copy_u32(ws, nbytes, A.ptr(tag + "kin"), A.ptr(tag + "kout"), A.ptr(tag + "vin") if pairs else None,
                                           A.ptr(tag + "vout") if pairs else None, n, bb, eb, desc, kt, None)

    def verify(A):
        order = stable_order(keys, kt, bb, eb, desc)
        assert np.array_equal(A.read(tag + "kout", np.uint32), keys[order]), "keys"
        if pairs:
            assert np.array_equal(A.read(tag + "vout", np.uint32), vals[order]), "values"
    return Call(gs.lib.gs_lsb_copy_temp_bytes(n, int(pairs)), launch, verify)


def row_lsb_wide(gs, A, tag, n, kind, var, pl, fill, seed):
    kt, vb, (bb, eb), desc = var
    kb = KEY_BYTES[kt]
    keys = gen_keys(kt, kind, n, seed)
    vals = np.arange(n, dtype=UINT[vb]) if vb else None
    A.add(tag + "k0", kb * n, data_off(pl, kb), data=keys).add(tag + "k1", kb * n, data_off(pl, kb), fill)
    if vb:
        A.add(tag + "v0", vb * n, data_off(pl, vb), data=vals).add(tag + "v1", vb * n, data_off(pl, vb), fill)
    sel = C.c_int(0)

    def launch(ws, nbytes):
        return gs.lib.gs_lsb_sort_wide(ws, nbytes, _db(A, tag + "k0", tag + "k1"), _db(A, tag + "v0", tag + "v1") if vb else None,
                                       C.byref(sel), n, kb, vb, bb, eb, desc, kt, None)

    def verify(A):
        order = stable_order(keys, kt, bb, eb, desc)
        assert np.array_equal(A.read(tag + "k%d" % sel.value, UINT[kb]), keys[order]), "keys"
        if vb:
            assert np.array_equal(A.read(tag + "v%d" % sel.value, UINT[vb]), vals[order]), "values"
    return Call(gs.lib.gs_lsb_wide_temp_bytes(n, kb, vb), launch, verify)


def row_lsb_any(gs, A, tag, n, kind, var, pl, fill, seed):
    kt, vb, (bb, eb), desc = var
    kb = KEY_BYTES[kt]
    keys = gen_keys(kt, kind, n, seed)
    vals = np.random.default_rng(seed + 1).integers(0, 256, size=n * vb, dtype=np.uint8).reshape(n, vb) if vb else None
    voff = 0 if pl != "P1" else (16 if vb == 16 else vb)       # 16-byte values stay 16-byte aligned (the contract)
    A.add(tag + "kin", kb * n, data_off(pl, kb), data=keys, const=True).add(tag + "kout", kb * n, data_off(pl, kb), fill)
    if vb:
        A.add(tag + "vin", vb * n, voff, data=vals, const=True).add(tag + "vout", vb * n, voff, fill)

    def launch(ws, nbytes):
        return gs.lib.gs_lsb_sort_any(ws, nbytes, A.ptr(tag + "kin"), A.ptr(tag + "kout"), A.ptr(tag + "vin") if vb else None,
                                      A.ptr(tag + "vout") if vb else None, n, kt, vb, bb, eb, desc, None)

    def verify(A):
        order = stable_order(keys, kt, bb, eb, desc)
        assert np.array_equal(A.read(tag + "kout", UINT[kb]), keys[order]), "keys"
        if vb:
            assert np.array_equal(A.read(tag + "vout", np.uint8).reshape(n, vb), vals[order]), "values"
    return Call(gs.lib.gs_lsb_any_temp_bytes(n, kt, vb), launch, verify)


def row_msb_u32(gs, A, tag, n, kind, var, pl, fill, seed, large=False):
    kt, pairs = var
    keys = gen_keys(kt, kind, n, seed)
    o = data_off(pl, 4)
    A.add(tag + "k", 4 * n, o, data=keys).add(tag + "ka", 4 * n, o, fill)
    if pairs:
        A.add(tag + "v", 4 * n, o, data=np.arange(n, dtype=np.uint32)).add(tag + "va", 4 * n, o, fill)

    def launch(ws, nbytes):
        k, ka = A.ptr(tag + "k"), A.ptr(tag + "ka")
        v, va = (A.ptr(tag + "v"), A.ptr(tag + "va")) if pairs else (None, None)
        if large:
            return gs.lib.gs_msb_sort_large_u32(ws, nbytes, k, v, n, ka, va, kt, None, 1)
        return gs.lib.gs_msb_sort_u32(ws, nbytes, k, v, n, ka, va, None, None, kt, None, 1)

    def verify(A):
        check_unstable(keys, kt, A.read(tag + "k", np.uint32), A.read(tag + "v", np.uint32) if pairs else None, tag)
    q = gs.lib.gs_msb_large_temp_bytes(n, int(pairs)) if large else gs.lib.gs_msb_temp_bytes(n, int(pairs))
    return Call(q, launch, verify)


def row_msb_wide(gs, A, tag, n, kind, var, pl, fill, seed, large=False):
    kt, vb = var
    kb = KEY_BYTES[kt]
    keys = gen_keys(kt, kind, n, seed)
    A.add(tag + "k", kb * n, data_off(pl, kb), data=keys).add(tag + "ka", kb * n, data_off(pl, kb), fill)
    if vb:
        A.add(tag + "v", vb * n, data_off(pl, vb), data=np.arange(n, dtype=UINT[vb])).add(tag + "va", vb * n, data_off(pl, vb), fill)

    def launch(ws, nbytes):
        k, ka = A.ptr(tag + "k"), A.ptr(tag + "ka")
        v, va = (A.ptr(tag + "v"), A.ptr(tag + "va")) if vb else (None, None)
        if large:
            return gs.lib.gs_msb_sort_large_wide(ws, nbytes, k, v, n, ka, va, kb, vb, kt, None, 1)
        return gs.lib.gs_msb_sort_wide(ws, nbytes, k, v, n, ka, va, kb, vb, None, None, kt, None, 1)

    def verify(A):
        check_unstable(keys, kt, A.read(tag + "k", UINT[kb]), A.read(tag + "v", UINT[vb]) if vb else None, tag)
    q = gs.lib.gs_msb_large_wide_temp_bytes(n, kb, vb) if large else gs.lib.gs_msb_wide_temp_bytes(n, kb, vb)
    return Call(q, launch, verify)


def row_large_u32(gs, *a):
    return row_msb_u32(gs, *a, large=True)


def row_large_wide(gs, *a):
    return row_msb_wide(gs, *a, large=True)


def segments(n, seed):
    """Non-overlapping segments with gaps between them, some empty; for n > 40000 one segment above 17408 elements."""
    rng = np.random.default_rng(seed)
    b, e, at = [], [], 0
    if n > 40000:
        b.append(0); e.append(n // 2); at = n // 2 + 3
    while at < n:
        length = int(rng.integers(0, 3000)) if rng.random() < 0.9 else 0
        b.append(at); e.append(min(n, at + length))
        at = e[-1] + int(rng.integers(0, 40))
    return np.array(b, np.int32), np.array(e, np.int32)


def row_segmented(gs, A, tag, n, kind, var, pl, fill, seed, wide=False):
    kt, vb, (bb, eb), desc = var
    kb = KEY_BYTES[kt]
    keys = gen_keys(kt, kind, n, seed)
    vals = np.arange(n, dtype=UINT[vb]) if vb else None
    sb, se = segments(n, seed)
    ns = sb.size
    A.add(tag + "k0", kb * n, data_off(pl, kb), data=keys).add(tag + "k1", kb * n, data_off(pl, kb), fill)
    if vb:
        A.add(tag + "v0", vb * n, data_off(pl, vb), data=vals).add(tag + "v1", vb * n, data_off(pl, vb), fill)
    A.add(tag + "sb", 4 * ns, data_off(pl, 4), data=sb, const=True).add(tag + "se", 4 * ns, data_off(pl, 4), data=se, const=True)
    sel = C.c_int(0)

    def launch(ws, nbytes):
        kk, vv = _db(A, tag + "k0", tag + "k1"), (_db(A, tag + "v0", tag + "v1") if vb else None)
        if wide:
            return gs.lib.gs_segmented_sort_wide(ws, nbytes, kk, vv, C.byref(sel), n, ns, A.ptr(tag + "sb"), A.ptr(tag + "se"), kb, vb,
                                                 bb, eb, desc, kt, None)
        return gs.lib.gs_segmented_sort_u32(ws, nbytes, kk, vv, C.byref(sel), n, ns, A.ptr(tag + "sb"), A.ptr(tag + "se"), bb, eb,
                                            desc, kt, None)

    def verify(A):
        seg = np.full(n, -1, np.int64)
        for i in range(ns):
            seg[sb[i]:se[i]] = i
        inside = seg >= 0
        m = (ordmap(keys, kt) >> np.uint64(bb)) & np.uint64((1 << (eb - bb)) - 1)
        order = np.lexsort((~m if desc else m, seg))
        order = order[inside[order]]                 # segment after segment, each stably sorted
        name = tag + "k%d" % sel.value
        got = A.read(name, UINT[kb])
        assert np.array_equal(got[inside], keys[order]), "keys"
        init = A.init[name].view(UINT[kb])
        assert np.array_equal(got[~inside], init[~inside]), "a gap element was written"
        if vb:
            name = tag + "v%d" % sel.value
            gv = A.read(name, UINT[vb])
            assert np.array_equal(gv[inside], vals[order]), "values"
            assert np.array_equal(gv[~inside], A.init[name].view(UINT[vb])[~inside]), "a gap value was written"
    q = gs.lib.gs_segmented_wide_temp_bytes(n, kb, vb, ns) if wide else gs.lib.gs_segmented_temp_bytes(n, int(vb != 0), ns)
    return Call(q, launch, verify)


def row_segmented_wide(gs, *a):
    return row_segmented(gs, *a, wide=True)


def row_first_pass(gs, A, tag, n, kind, var, pl, fill, seed):
    kt, pairs = var
    keys = gen_keys(kt, kind, n, seed)
    vals = np.arange(n, dtype=np.uint32)
    o = data_off(pl, 4)
    A.add(tag + "kin", 4 * n, o, data=keys, const=True).add(tag + "kout", 4 * n, o, fill)
    if pairs:
        A.add(tag + "vin", 4 * n, o, data=vals, const=True).add(tag + "vout", 4 * n, o, fill)
    A.add(tag + "counts", 8 * 256, data_off(pl, 8), fill)

    def launch(ws, nbytes):
        return gs.lib.gs_msb_first_pass_u32(ws, nbytes, A.ptr(tag + "kin"), A.ptr(tag + "kout"), A.ptr(tag + "vin") if pairs else None,
                                            A.ptr(tag + "vout") if pairs else None, n, kt, A.ptr(tag + "counts"), None)

    def verify(A):
        o32 = ordmap(keys, kt).astype(np.uint32)
        top = o32 >> np.uint32(24)
        order = np.argsort(top, kind="stable")
        assert np.array_equal(A.read(tag + "counts", np.uint64), np.bincount(top, minlength=256).astype(np.uint64)), "counts"
        assert np.array_equal(A.read(tag + "kout", np.uint32), o32[order]), "keys"
        if pairs:
            assert np.array_equal(A.read(tag + "vout", np.uint32), vals[order]), "values"
    return Call(gs.lib.gs_lsb_temp_bytes(n, int(pairs)), launch, verify)


def row_finish(gs, A, tag, n, kind, var, pl, fill, seed):
    """gs_msb_finish_u32 with one source, fed by gs_msb_first_pass_u32 (own guarded workspace) and its bucket counts."""
    kt, pairs = var
    keys = gen_keys(kt, kind, n, seed)
    o = data_off(pl, 4)
    # (the first pass's outputs and workspace are written even when the finish is refused: const=False)
    A.add(tag + "kin", 4 * n, o, data=keys, const=True).add(tag + "kg", 4 * n, o, fill, const=False).add(tag + "kout", 4 * n, o, fill)
    if pairs:
        A.add(tag + "vin", 4 * n, o, data=np.arange(n, dtype=np.uint32), const=True)
        A.add(tag + "vg", 4 * n, o, fill, const=False).add(tag + "vout", 4 * n, o, fill)
    A.add(tag + "counts", 8 * 256, data_off(pl, 8), fill, const=False)
    fp_bytes = gs.lib.gs_lsb_temp_bytes(n, int(pairs))
    A.add(tag + "fpws", fp_bytes, PLACEMENTS[pl], fill, const=False)

    def launch(ws, nbytes):
        v = lambda s: A.ptr(tag + s) if pairs else None
        e = gs.lib.gs_msb_first_pass_u32(A.ptr(tag + "fpws"), fp_bytes, A.ptr(tag + "kin"), A.ptr(tag + "kg"), v("vin"), v("vg"), n, kt,
                                         A.ptr(tag + "counts"), None)
        if e:
            return e
        torch.cuda.synchronize()
        counts = np.ascontiguousarray(A.read(tag + "counts", np.uint64))
        return gs.lib.gs_msb_finish_u32(ws, nbytes, A.ptr(tag + "kg"), v("vg"), A.ptr(tag + "kout"), v("vout"), n,
                                        counts.ctypes.data_as(C.c_void_p), 1, kt, None, 1)

    def verify(A):
        check_unstable(keys, kt, A.read(tag + "kout", np.uint32), A.read(tag + "vout", np.uint32) if pairs else None, tag)
    return Call(gs.lib.gs_msb_finish_temp_bytes(n, int(pairs), 1), launch, verify)


SHARD_BITS = 12


def row_shard_partition(gs, A, tag, n, kind, var, pl, fill, seed):
    ranks, pairs = var
    keys = gen_keys(U32, kind, n, seed)
    vals = np.arange(n, dtype=np.uint32)
    dest = np.sort(np.random.default_rng(seed + 2).integers(0, ranks, size=1 << SHARD_BITS)).astype(np.uint8)
    o = data_off(pl, 4)
    A.add(tag + "kin", 4 * n, o, data=keys, const=True).add(tag + "kout", 4 * n, o, fill)
    if pairs:
        A.add(tag + "vin", 4 * n, o, data=vals, const=True).add(tag + "vout", 4 * n, o, fill)
    A.add(tag + "dest", dest.size, 1 if pl == "P1" else 0, data=dest, const=True)
    A.add(tag + "counts", 8 * ranks, data_off(pl, 8), fill)

    def launch(ws, nbytes):
        return gs.lib.gs_shard_partition_u32(ws, nbytes, A.ptr(tag + "kin"), A.ptr(tag + "kout"), A.ptr(tag + "vin") if pairs else None,
                                             A.ptr(tag + "vout") if pairs else None, n, SHARD_BITS, A.ptr(tag + "dest"), ranks, None,
                                             A.ptr(tag + "counts"), U32, None)

    def verify(A):
        r = dest[keys >> np.uint32(32 - SHARD_BITS)]
        order = np.argsort(r, kind="stable")
        assert np.array_equal(A.read(tag + "counts", np.uint64), np.bincount(r, minlength=ranks).astype(np.uint64)), "counts"
        assert np.array_equal(A.read(tag + "kout", np.uint32), keys[order]), "keys"
        if pairs:
            assert np.array_equal(A.read(tag + "vout", np.uint32), vals[order]), "values"
    return Call(gs.lib.gs_msb_temp_bytes(n, int(pairs)), launch, verify)


def row_shard_histogram(gs, A, tag, n, kind, var, pl, fill, seed):
    """gs_shard_histogram_u32 takes no workspace (query 0).  The variant's flag picks the width: 12 bits or 11.  Under P1 the
    keys lie three elements off a 16-byte boundary, which is the scalar kernel.  Asked for a short workspace (-1 bytes),
    the row makes the call that is refused for its width instead, 13 bits: the histogram must stay as it was."""
    kt, wide = var
    bits = SHARD_BITS if wide else SHARD_BITS - 1
    keys = gen_keys(kt, kind, n, seed)
    A.add(tag + "kin", 4 * n, data_off(pl, 4), data=keys, const=True).add(tag + "hist", 8 << bits, data_off(pl, 8), fill)

    def launch(ws, nbytes):
        return gs.lib.gs_shard_histogram_u32(A.ptr(tag + "kin"), n, bits if nbytes >= 0 else SHARD_BITS + 1, A.ptr(tag + "hist"), kt, None)

    def verify(A):
        want = np.bincount(ordmap(keys, kt).astype(np.uint32) >> np.uint32(32 - bits), minlength=1 << bits).astype(np.uint64)
        assert np.array_equal(A.read(tag + "hist", np.uint64), want), "histogram"
    return Call(0, launch, verify)


LSB_VARS = [(U32, False, (0, 32), 0), (I32, True, (0, 32), 0), (F32, True, (0, 32), 1), (U32, True, (3, 29), 0),
            (F32, False, (0, 32), 0), (I32, False, (5, 21), 1)]
WIDE_LSB_VARS = [(U64, 0, (0, 64), 0), (I64, 4, (0, 64), 1), (F64, 8, (0, 64), 0), (F32, 8, (0, 32), 0), (U64, 8, (7, 45), 0),
                 (I32, 8, (0, 32), 1)]
ANY_VARS = [(U8, 1, (0, 8), 0), (I16, 2, (0, 16), 1), (U64, 16, (0, 64), 0), (F32, 3, (0, 32), 0), (I8, 0, (1, 7), 0),
            (F64, 4, (0, 64), 1), (U16, 16, (0, 16), 0)]
MSB_VARS = [(U32, False), (I32, True), (F32, True), (U32, True), (F32, False)]
WIDE_MSB_VARS = [(U64, 0), (I64, 4), (F64, 8), (F32, 8), (U32, 8), (U64, 8)]
SEG_VARS = [(U32, 0, (0, 32), 0), (I32, 4, (0, 32), 1), (F32, 4, (0, 32), 0), (U32, 4, (4, 20), 0)]
SEG_WIDE_VARS = [(U64, 0, (0, 64), 0), (I64, 4, (0, 64), 1), (F64, 8, (0, 64), 0), (F32, 8, (0, 32), 0), (U64, 8, (8, 40), 0)]
FP_VARS = [(U32, True), (I32, False), (F32, True)]
SHARD_VARS = [(8, True), (3, False), (1, True), (256, True)]

U32_SIZES = [0, 1, 2, 2047, 2049, 4607, 4609, 8191, 8193, 9215, 9217, 17407, 17409, 100003]
WIDE_SIZES = [0, 1, 2, 2047, 2049, 4095, 4097, 8191, 8193, 100003]

ROWS = {
    "gs_lsb_sort_u32": (row_lsb_u32, LSB_VARS, U32_SIZES),
    "gs_lsb_sort_copy_u32": (row_lsb_copy, LSB_VARS, U32_SIZES),
    "gs_lsb_sort_wide": (row_lsb_wide, WIDE_LSB_VARS, WIDE_SIZES),
    "gs_lsb_sort_any": (row_lsb_any, ANY_VARS, WIDE_SIZES),
    "gs_msb_sort_u32": (row_msb_u32, MSB_VARS, U32_SIZES),
    "gs_msb_sort_wide": (row_msb_wide, WIDE_MSB_VARS, WIDE_SIZES),
    "gs_msb_sort_large_u32": (row_large_u32, MSB_VARS, U32_SIZES),
    "gs_msb_sort_large_wide": (row_large_wide, WIDE_MSB_VARS, WIDE_SIZES),
    "gs_segmented_sort_u32": (row_segmented, SEG_VARS, U32_SIZES),
    "gs_segmented_sort_wide": (row_segmented_wide, SEG_WIDE_VARS, WIDE_SIZES),
    "gs_msb_first_pass_u32": (row_first_pass, FP_VARS, U32_SIZES),
    "gs_msb_finish_u32": (row_finish, FP_VARS, U32_SIZES),
    "gs_shard_partition_u32": (row_shard_partition, SHARD_VARS, U32_SIZES),
    "gs_shard_histogram_u32": (row_shard_histogram, FP_VARS, U32_SIZES),
}


def run(gs, cuda, row, calls, pl, fill, seed, short=False):
    """Place every call's buffers and one workspace (sized for the largest query; `short`: one byte less) in an arena,
    enqueue the calls one behind the other, then check the guards and inputs and every call's result."""
    fn = ROWS[row][0]
    A = Arena(cuda, seed=seed, all_const=short)
    prepared = [fn(gs, A, "c%d_" % i, n, kind, var, pl, fill, seed + 7 * i) for i, (n, kind, var) in enumerate(calls)]
    wsz = max(c.query for c in prepared)
    A.add("ws", max(wsz - 1, 0) if short else wsz, PLACEMENTS[pl], fill)        # (a row without a workspace queries 0)
    A.build()
    what = "%s %s fill=%s calls=%s" % (row, pl, fill, [(n, k, v) for n, k, v in calls])
    for c in prepared:
        rc = c.launch(A.ptr("ws"), c.query - 1 if short else c.query)
        assert rc == (INVALID if short else 0), "%s: returned %d" % (what, rc)
    try:
        A.check()
        if not short:
            for c in prepared:
                c.verify(A)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None


@pytest.fixture
def large_limit(monkeypatch):
    monkeypatch.setenv(LIMIT_ENV, "4096")


@pytest.mark.parametrize("pl,fill", COMBOS, ids=["%s-%s" % c for c in COMBOS])
@pytest.mark.parametrize("row", list(ROWS))
def test_small_sizes_every_placement_and_fill(gs, cuda, large_limit, row, pl, fill):
    """Every row at the edge sizes (0-2, tile and local-sort class capacities +-1, 100003) under every placement and fill;
    key kinds and variants rotate with the size."""
    _, variants, sizes = ROWS[row]
    c = COMBOS.index((pl, fill))
    for i, n in enumerate(sizes):
        run(gs, cuda, row, [(n, KINDS[(i + c) % len(KINDS)], variants[(i + 2 * c) % len(variants)])], pl, fill, seed=100 * i + c)


@pytest.mark.parametrize("pl,fill", [("P1", "random"), ("P2+255", "ff")])
@pytest.mark.parametrize("row", list(ROWS))
def test_big_size(gs, cuda, large_limit, row, pl, fill):
    """One size of 2^21 + 77 per row: the MSB levels, several LSB chunks, many slices and group finishes of the large sorts."""
    _, variants, _ = ROWS[row]
    k = list(ROWS).index(row)
    run(gs, cuda, row, [(BIG, "uniform" if pl == "P1" else "zipf", variants[k % len(variants)])], pl, fill, seed=k)


@pytest.mark.parametrize("row", list(ROWS))
def test_every_key_kind_and_variant(gs, cuda, large_limit, row):
    """Each variant (key type, values, bits, order) of the row with each key kind, at a size whose passes all run."""
    _, variants, _ = ROWS[row]
    for j, var in enumerate(variants):
        for i, kind in enumerate(KINDS):
            pl, fill = COMBOS[(i + j) % len(COMBOS)]
            run(gs, cuda, row, [(30011, kind, var)], pl, fill, seed=10 * j + i)


@pytest.mark.parametrize("pl,fill", [("P1", "random"), ("P2+100", "ff"), ("P0", "random")])
@pytest.mark.parametrize("row", list(ROWS))
def test_reuse_of_a_dirty_workspace(gs, cuda, large_limit, row, pl, fill):
    """A second call in the workspace the first one left behind, enqueued right behind it on the same stream, with another
    size and input: both results are right."""
    _, variants, _ = ROWS[row]
    run(gs, cuda, row, [(100003, "uniform", variants[0]), (9217, "zipf", variants[1 % len(variants)])], pl, fill, seed=3)
    run(gs, cuda, row, [(4097, "few", variants[-1]), (70001, "special", variants[0])], pl, fill, seed=4)


@pytest.mark.parametrize("ws_off", [0, 1])
@pytest.mark.parametrize("row", list(ROWS))
def test_short_workspace_is_refused_and_touches_nothing(gs, cuda, large_limit, row, ws_off):
    """query - 1 bytes, with real guarded buffers: hipErrorInvalidValue, and every byte of the arena is unchanged."""
    _, variants, _ = ROWS[row]
    pl = "P0" if ws_off == 0 else "P1"
    for n in (1000, 100003):
        run(gs, cuda, row, [(n, "uniform", variants[0])], pl, "random", seed=n, short=True)


@pytest.mark.parametrize("pl", ["P1", "P2+255"])
def test_census_after_msb_sort_in_an_offset_workspace(gs, cuda, pl):
    """gs_msb_census reads the workspace a gs_msb_sort_u32 left at an offset base: level 0 holds n keys and the levels add up."""
    from gpu_sort_amd.msb import _LevelCensus
    for n, kind in ((BIG, "uniform"), (300007, "zipf")):
        A = Arena(cuda, seed=1)
        call = row_msb_u32(gs, A, "", n, kind, (U32, False), pl, "random", 5)
        A.add("ws", call.query, PLACEMENTS[pl], "random").build()
        assert call.launch(A.ptr("ws"), call.query) == 0
        A.check()
        call.verify(A)
        out = (_LevelCensus * 4)()
        assert gs.lib.gs_msb_census(A.ptr("ws"), n, 0, C.cast(out, C.c_void_p), None) == 0
        cen = list(out)
        assert cen[0].keys == n and cen[0].buckets == 1 and cen[0].overflow == 0
        for L in range(3):
            assert cen[L + 1].keys <= cen[L].keys
        tasks = sum(c.task_keys for c in cen)
        assert tasks + cen[3].keys <= n <= tasks + cen[3].keys + sum(c.pivot_keys for c in cen)


def test_guard_names_a_buffer_one_element_short(gs, cuda):
    """The harness itself: an output buffer placed one element short of what the sort writes must trip its trailing guard,
    and the message must name that buffer (the stray store stays inside the arena)."""
    n = 5000
    keys = gen_keys(U32, "uniform", n, 0)
    A = Arena(cuda)
    q = gs.lib.gs_lsb_copy_temp_bytes(n, 0)
    A.add("kin", 4 * n, data=keys, const=True).add("short_out", 4 * (n - 1), 12).add("ws", q, 1).build()
    assert gs.lib.gs_lsb_sort_copy_u32(A.ptr("ws"), q, A.ptr("kin"), A.ptr("short_out"), None, None, n, 0, 32, 0, U32, None) == 0
    with pytest.raises(AssertionError, match=r"guard hit after buffer 'short_out'") as hit:
        A.check()
    off = int(re.search(r"the first (\d+) byte\(s\) past its end", str(hit.value)).group(1))
    assert off < 4, str(hit.value)                   # in the element just past the buffer
