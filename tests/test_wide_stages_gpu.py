"""The wide LSB pass (gs_wide.hip, gs_wide_tile.inc) through gs_lsb_sort_wide and gs_lsb_sort_any at every type row, tile, chunk
and group edge.

A bit range of at most 8 bits is ONE pass, so a raw gs_lsb_sort_wide call on such a range runs the three kernels once and leaves
their products -- the scanned spine, the digit totals, prefix16 -- in the workspace, where these tests read them (the layout is the
pass's internal one, restated in tests/wide_stages_ref.py; wide_totals_ptr depends on the same layout).  Every comparison is
equality of bytes with that reference, which tests/test_wide_stages_cpu.py holds against the oracle and shows to tell nine plausible
wrong kernels from the right one (a tenth turns out to be no fault).  Values are enumerated at the value's own width, so equality with the reference proves
stability.  All buffers live in an Arena (tests/guarded.py): a stray store trips a guard instead of faulting."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import wide_stages_ref as R
from guarded import Arena
from wide_stages_ref import TILE, KT_NAME

pytestmark = pytest.mark.gpu

DIRTY = 0xA5                    # what the workspace holds before a call
UNWRITTEN = 0x5A                # what an output holds before a call
NP_UINT = {4: np.uint32, 8: np.uint64}


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(cuda)


def _slot(A, name):
    start, nbytes = A.slots[name][:2]
    return A.mem[start:start + nbytes]


def _db(A, a, b):
    return (C.c_void_p * 2)(A.ptr(a), A.ptr(b))


def _read(A, name, nbytes_elem):
    return A.read(name, NP_UINT[nbytes_elem])


def _pass_arena(gs, cuda, n, kb, vb, seed):
    q = gs.lib.gs_lsb_wide_temp_bytes(n, kb, vb)
    assert q == R.temp_bytes(n)
    A = Arena(cuda, seed=seed)
    A.add("ws", q, 0, "random").add("k0", kb * n).add("k1", kb * n)
    if vb:
        A.add("v0", vb * n).add("v1", vb * n)
    A.build()
    assert A.ptr("ws") % 256 == 0
    return A, q


def _check_products(got, n, prod, where):
    """The scanned spine, the totals and prefix16 a pass left in the workspace bytes `got`; the slack behind them untouched."""
    sp, tot, pf, size = R.layout(n)
    grid, tiles = R.grid_of(n), R.num_tiles(n)
    spine = got[sp:sp + 1024 * grid].view(np.uint32).reshape(256, grid)
    totals = got[tot:tot + 1024].view(np.uint32)
    prefix16 = got[pf:pf + 512 * tiles].view(np.uint16).reshape(tiles, 256)
    assert np.array_equal(totals, prod["totals"]), where
    assert np.array_equal(spine, prod["spine"]), where
    assert np.array_equal(prefix16, prod["prefix16"]), where
    assert int(totals.astype(np.int64).sum()) == n
    assert np.all(got[pf + 512 * tiles:] == DIRTY), where


def _run_passes(gs, cuda, n, row, calls):
    """One-pass sorts of n keys of one row: one Arena, refilled for every call; the starting selector alternates."""
    kb, vb, kt, desc = row
    A, q = _pass_arena(gs, cuda, n, kb, vb, n)
    vals = R.enumerated(n, vb) if vb else None
    staged_v = _dev(vals, cuda) if vb else None
    for turn, (shift, bits, name) in enumerate(calls):
        where = (R.row_name(row), n, shift, bits, name)
        start = turn & 1
        keys = R.build_keys(name, n, kt, desc, shift, bits)
        want_k, want_v, prod = R.pass_ref(keys, vals, kt, desc, shift, bits)
        staged_k = _dev(keys, cuda)
        _slot(A, "ws").fill_(DIRTY)
        _slot(A, "k%d" % start).copy_(staged_k)
        _slot(A, "k%d" % (start ^ 1)).fill_(UNWRITTEN)
        if vb:
            _slot(A, "v%d" % start).copy_(staged_v)
            _slot(A, "v%d" % (start ^ 1)).fill_(UNWRITTEN)
        sel = C.c_int(start)
        assert gs.lib.gs_lsb_sort_wide(A.ptr("ws"), q, _db(A, "k0", "k1"), _db(A, "v0", "v1") if vb else None, C.byref(sel), n, kb, vb,
                                       shift, shift + bits, desc, kt, None) == 0, where
        assert sel.value == start ^ 1, where
        got_ws = A.read("ws", np.uint8)
        assert torch.equal(_slot(A, "k%d" % start), staged_k), where          # a pass reads its input only
        assert np.array_equal(_read(A, "k%d" % sel.value, kb), want_k), where
        if vb:
            assert torch.equal(_slot(A, "v%d" % start), staged_v), where
            assert np.array_equal(_read(A, "v%d" % sel.value, vb), want_v), where
        _check_products(got_ws, n, prod, where)
        if name == "equal" and n >= 9 * TILE:
            assert int(prod["prefix16"].max()) == 7 * TILE
    A.check()


# ---------------------------------------------------------------------------------------------------- one pass --
def _size_kind(n):
    full, tail = n // TILE, n % TILE
    return "%dtiles%s-%dchunks" % (full, "+%d" % tail if tail else "", R.grid_of(n))


_ONE = [(n, row) for n in R.SIZES for row in R.ROWS]


@pytest.mark.parametrize("n,row", _ONE, ids=["n%d-%s-%s" % (n, _size_kind(n), R.row_name(row)) for n, row in _ONE])
def test_one_pass_every_digit_position(gs, cuda, n, row):
    """One (K, V) kernel, key type and direction at one size: every digit position of the key's width with every input.  Keys,
    values, scanned spine, totals and prefix16."""
    calls = R.one_pass_calls(n, row)
    _run_passes(gs, cuda, n, row, calls)


_TAIL = [(n, row) for n in R.TAIL_SIZES for row in R.ROWS]


@pytest.mark.parametrize("n,row", _TAIL, ids=["n%d-%s-%s" % (n, _size_kind(n), R.row_name(row)) for n, row in _TAIL])
def test_real_keys_of_the_all_ones_image_rank_before_the_pads(gs, cuda, n, row):
    """The partial last tile holds nothing but keys whose image is all ones (~0 ascending, 0 descending, INT_MAX, the largest
    positive NaN ...): they share the pads' digit bucket at every digit position and must all come out, with their values."""
    _run_passes(gs, cuda, n, row, R.tail_calls(n, row))


# ------------------------------------------------------------------------------------------------ group shapes --
_GROUPS = R.group_cases()


@pytest.fixture(scope="module")
def big_pattern(cuda):
    """The guard pattern at the size of the largest arena below, made once (guarded._pattern regrows it otherwise)."""
    n = max(R.GROUP_TILES) * TILE
    guarded._pattern(4 * 8 * n + R.temp_bytes(n) + 16 * guarded.GUARD, cuda)


@pytest.mark.parametrize("T,last,row,shift,bits,name", _GROUPS,
                         ids=["T%d-last%d-%s-shift%d-bits%d-%s" % (T, last, R.row_name(row), s, b, name) for T, last, row, s, b, name in _GROUPS])
def test_group_shapes_of_the_tile_map(gs, cuda, big_pattern, T, last, row, shift, bits, name):
    """511 to 1025 tiles: tile_of_item permutes the tiles of every whole group of 512 and leaves the ragged group alone; the last
    tile is full or holds 4091 keys, inside a permuted group (512, 1024 tiles) or behind one (513, 1025)."""
    n = (T - 1) * TILE + last
    assert R.num_tiles(n) == T
    _run_passes(gs, cuda, n, row, [(shift, bits, name)])


# ------------------------------------------------------------------------------------------------- whole sorts --
_SORTS = [(kt, desc, n) for kt in R.SORT_TYPES for desc in (0, 1) for n in R.SORT_SIZES]


@pytest.mark.parametrize("kt,desc,n", _SORTS, ids=["%s-%s-n%d" % (KT_NAME[kt], "desc" if d else "asc", n) for kt, d, n in _SORTS])
def test_whole_sorts_every_range_selector_and_value_form(gs, cuda, kt, desc, n):
    """gs_lsb_sort_wide on every bit range of the table, from selector 0 and 1, keys only and with values.  Float keys carry
    +-0, +-inf, subnormals and NaNs of both signs with several payloads; the outputs hold the caller's bit patterns.  The
    selector ends at start xor (passes mod 2); for begin == end neither buffer changes."""
    kb = R.width(kt) // 8
    q = gs.lib.gs_lsb_wide_temp_bytes(n, kb, 8)
    A = Arena(cuda, seed=n + kt)
    A.add("ws", q, 0, "random").add("k0", kb * n).add("k1", kb * n)
    for vb in (4, 8):
        A.add("v%d0" % vb, vb * n).add("v%d1" % vb, vb * n)
    A.build()
    keys = R.build_keys(R.sort_input(kt), n, kt, desc)
    staged_k = _dev(keys, cuda)
    for begin, end, start, vb in R.sort_calls(kt, desc, n):
        where = (begin, end, start, vb)
        vals = R.enumerated(n, vb) if vb else None
        want_k, want_v, want_sel = R.sort_ref(keys, vals, kt, desc, begin, end, start)
        names = ["k%d" % start, "k%d" % (start ^ 1)] + (["v%d%d" % (vb, start), "v%d%d" % (vb, start ^ 1)] if vb else [])
        _slot(A, "ws").fill_(DIRTY)
        _slot(A, names[0]).copy_(staged_k)
        _slot(A, names[1]).fill_(UNWRITTEN)
        if vb:
            _slot(A, names[2]).copy_(_dev(vals, cuda))
            _slot(A, names[3]).fill_(UNWRITTEN)
        sel = C.c_int(start)
        assert gs.lib.gs_lsb_sort_wide(A.ptr("ws"), q, _db(A, "k0", "k1"), _db(A, "v%d0" % vb, "v%d1" % vb) if vb else None, C.byref(sel),
                                       n, kb, vb, begin, end, desc, kt, None) == 0, where
        assert sel.value == want_sel == start ^ (R.num_passes(begin, end) & 1), where
        assert np.array_equal(_read(A, "k%d" % sel.value, kb), want_k), where
        if vb:
            assert np.array_equal(_read(A, "v%d%d" % (vb, sel.value), vb), want_v), where
        if begin == end:            # nothing to do: both buffers as they were
            assert sel.value == start and torch.equal(_slot(A, names[0]), staged_k) and bool((_slot(A, names[1]) == UNWRITTEN).all()), where
            assert not vb or bool((_slot(A, names[3]) == UNWRITTEN).all()), where
            assert bool((_slot(A, "ws") == DIRTY).all()), where
    A.check()


def test_two_sorts_of_different_rows_back_to_back_on_one_workspace(gs, cuda):
    """(u64, u64) F64 descending on all 64 bits, then (u32, none) I32 ascending on (7, 24), then (u64, u32) U64 on (31, 33): one
    workspace, one stream, no synchronisation in between.  Each sort's passes must see their own spine, totals and prefix16."""
    plan = (((8, 8, R.F64, 1), 100003, 0, 64), ((4, 0, R.I32, 0), 8 * TILE + 1, 7, 24), ((8, 4, R.U64, 0), 4097, 31, 33))
    q = max(gs.lib.gs_lsb_wide_temp_bytes(n, row[0], row[1]) for row, n, _, _ in plan)
    A = Arena(cuda, seed=3)
    A.add("ws", q, 0, "random")
    for i, (row, n, _, _) in enumerate(plan):
        kb, vb, kt, desc = row
        A.add("k%d0" % i, kb * n, data=R.build_keys(R.sort_input(kt), n, kt, desc, seed=i)).add("k%d1" % i, kb * n)
        if vb:
            A.add("v%d0" % i, vb * n, data=R.enumerated(n, vb)).add("v%d1" % i, vb * n)
    A.build()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    sels = [C.c_int(0) for _ in plan]
    for i, (row, n, begin, end) in enumerate(plan):
        kb, vb, kt, desc = row
        assert gs.lib.gs_lsb_sort_wide(A.ptr("ws"), q, _db(A, "k%d0" % i, "k%d1" % i), _db(A, "v%d0" % i, "v%d1" % i) if vb else None,
                                       C.byref(sels[i]), n, kb, vb, begin, end, desc, kt, stream.cuda_stream) == 0
    stream.synchronize()
    for i, (row, n, begin, end) in enumerate(plan):
        kb, vb, kt, desc = row
        keys = R.build_keys(R.sort_input(kt), n, kt, desc, seed=i)
        want_k, want_v, want_sel = R.sort_ref(keys, R.enumerated(n, vb) if vb else None, kt, desc, begin, end, 0)
        assert sels[i].value == want_sel, i
        assert np.array_equal(_read(A, "k%d%d" % (i, want_sel), kb), want_k), i
        if vb:
            assert np.array_equal(_read(A, "v%d%d" % (i, want_sel), vb), want_v), i
    A.check()


def test_refused_sorts_write_nothing(gs, cuda):
    """The refusals of tests/test_wide_stages_cpu.py with real buffers: 1 comes back and no byte of the workspace, of either key
    buffer or of either value buffer changes; the same call with good arguments is then taken."""
    n, kb, vb = 4097, 8, 8
    q = gs.lib.gs_lsb_wide_temp_bytes(n, kb, vb)
    keys, vals = R.build_keys("special", n, R.F64, 0), R.enumerated(n, vb)
    A = Arena(cuda, seed=5, all_const=True)
    A.add("ws", q, 0, "random").add("k0", kb * n, data=keys).add("k1", kb * n).add("v0", vb * n, data=vals).add("v1", vb * n)
    A.build()

    def call(q=q, sel=0, kb=kb, vb=vb, begin=0, end=64, kt=R.F64, k1="k1"):
        s = C.c_int(sel)
        r = gs.lib.gs_lsb_sort_wide(A.ptr("ws"), q, (C.c_void_p * 2)(A.ptr("k0"), A.ptr(k1) if k1 else None), _db(A, "v0", "v1"),
                                    C.byref(s), n, kb, vb, begin, end, 0, kt, None)
        return r, s.value
    for kw in (dict(q=q - 1), dict(sel=2), dict(kb=5), dict(vb=3), dict(end=65), dict(begin=9, end=8), dict(kt=R.F32), dict(k1=None)):
        assert call(**kw) == (1, kw.get("sel", 0)), kw
    assert call(begin=20, end=20) == (0, 0) and call(begin=20, end=20, sel=1) == (0, 1)      # nothing to do
    A.check()
    A._const.clear()                                                    # from here on the buffers may change
    assert call() == (0, 0)                                             # eight passes
    want_k, want_v, _ = R.sort_ref(keys, vals, R.F64, 0, 0, 64)
    assert np.array_equal(_read(A, "k0", kb), want_k) and np.array_equal(_read(A, "v0", vb), want_v)
    A.check()


# ---------------------------------------------------------------------------------------------- gs_lsb_sort_any --
def _any_offset(vb):
    return 0 if vb in (0, 16) else 2 if vb == 2 else 1       # 16-byte values must be aligned; byte-wise values need not be


def _any_arena(gs, cuda, n, kt, vb, seed, voff=None, all_const=False):
    kb = R.width(kt) // 8
    keys = R.build_keys(R.sort_input(kt), n, kt, 0, seed=seed)
    vals = np.random.default_rng([seed, n, vb]).integers(0, 256, (n, max(vb, 1)), dtype=np.uint8)
    q = gs.lib.gs_lsb_any_temp_bytes(n, kt, min(vb, 4096))
    A = Arena(cuda, seed=seed, all_const=all_const)
    A.add("ws", q, 0, "random").add("kin", kb * n, data=keys, const=True).add("kout", kb * n)
    if vb:
        off = _any_offset(vb) if voff is None else voff
        A.add("vin", vb * n, off, data=vals, const=True).add("vout", vb * n, off)
    A.build()
    return A, q, keys, vals


_ANY = [(kt, vb) for kt in R.ANY_TYPES for vb in R.ANY_VALUE_BYTES]


@pytest.mark.parametrize("kt,vb", _ANY, ids=["%s-v%d" % (KT_NAME[kt], vb) for kt, vb in _ANY])
def test_sort_any_every_value_size(gs, cuda, kt, vb):
    """The plain-pointer form with const inputs: 64-bit keys go through any_prepare64_kernel, the wide sort of (key, u32 index)
    and the gather; 32-bit keys through the 32-bit pairs sort and the same gather.  Value sizes 1, 2 and 16 take the typed
    moves, 3, 12, 24 and 4096 the byte-wise one, 0 the gather with no values.  Full range, a sub-range and begin == end (the
    output is the input in input order), both directions; float keys carry NaNs.  The inputs stay unchanged."""
    kb = R.width(kt) // 8
    for n in R.any_sizes(vb):
        A, q, keys, vals = _any_arena(gs, cuda, n, kt, vb, seed=n + vb)
        for begin, end in R.ANY_RANGES[R.width(kt)]:
            for desc in (0, 1):
                where = (n, begin, end, desc)
                _slot(A, "kout").fill_(UNWRITTEN)
                if vb:
                    _slot(A, "vout").fill_(UNWRITTEN)
                assert gs.lib.gs_lsb_sort_any(A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if vb else None,
                                              A.ptr("vout") if vb else None, n, kt, vb, begin, end, desc, None) == 0, where
                A.check()                                               # guards, and kin / vin unchanged
                order = R.stable_order(keys, kt, desc, begin, end)
                assert np.array_equal(_read(A, "kout", kb), keys[order]), where
                if vb:
                    assert np.array_equal(A.read("vout", np.uint8).reshape(n, vb), vals[order]), where


@pytest.mark.parametrize("kt", R.ANY_TYPES, ids=KT_NAME.get)
def test_sort_any_refuses_values_of_4097_bytes_and_misaligned_16_byte_values(gs, cuda, kt):
    n = 4097 if kt != R.U64 else 1
    w = R.width(kt)
    for vb, voff, why in ((4097, 1, "value size above 4096"), (16, 8, "16-byte values at an address that is 8 mod 16")):
        A, q, _, _ = _any_arena(gs, cuda, n, kt, vb, seed=7, voff=voff, all_const=True)
        for vin, vout in ((A.ptr("vin"), A.ptr("vout")),) + (((A.ptr("vin") + 8, A.ptr("vout")), (A.ptr("vin"), A.ptr("vout") + 8)) if vb == 16 else ()):
            if vb == 16 and (vin | vout) % 16 == 0:
                continue
            assert gs.lib.gs_lsb_sort_any(A.ptr("ws"), A.nbytes("ws"), A.ptr("kin"), A.ptr("kout"), vin, vout, n, kt, vb, 0, w, 0, None) == 1, why
        A.check()                                                       # refused: nothing written anywhere
    A, q, keys, vals = _any_arena(gs, cuda, n, kt, 16, seed=7)          # the same call with aligned values is taken
    assert gs.lib.gs_lsb_sort_any(A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin"), A.ptr("vout"), n, kt, 16, 0, w, 0, None) == 0
    A.check()
    order = R.stable_order(keys, kt, 0, 0, w)
    assert np.array_equal(A.read("vout", np.uint8).reshape(n, 16), vals[order])
