"""The three kernels of one LSB pass through their stage calls -- gs_lsb_upsweep_u32, gs_lsb_scan_spine, gs_lsb_downsweep_u32 --
at every kernel variant, geometry and digit edge, and gs_lsb_sort_u32 / gs_lsb_sort_copy_u32 at their route boundaries.

The stage calls run the large-array kernels at any size, so a few thousand keys reach every branch.  Every comparison is
equality of bytes with tests/lsb_stages_ref.py (guarded on the CPU by tests/test_lsb_stages_cpu.py, which also shows that
these case tables tell eight plausible wrong kernels from the right one).  Buffers of the host-checked cases live in an
Arena (tests/guarded.py); above 2^22 keys the expected result is built with torch.sort(stable=True) and compared on the
device, and only a mismatch count and the first mismatching index come back.  The test ids name the branch a case is for."""
import ctypes as C

import numpy as np
import pytest
import torch

import lsb_stages_ref as R
import msb_cases
from guarded import Arena
from lsb_stages_ref import U32, F32, TILE, KT_NAME

pytestmark = pytest.mark.gpu

BAND = 64 * 1024                # guard elements (u32) on either side of a device-checked output: more than a tile
DIRTY = 0xA5                    # what the workspace holds before a call


def _geometry(gs, n):
    g, t, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    gs.lib.gs_lsb_geometry(n, 0, C.byref(g), C.byref(t), C.byref(c))
    assert (t.value, c.value) == (R.TILE, R.TPC) and g.value == R.grid_of(n)
    return g.value


def _layout(gs, ws_ptr, n):
    """Byte offsets of the spine, the totals and prefix16 from the workspace pointer (gs_lsb_workspace_layout)."""
    sp, tot, pf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert gs.lib.gs_lsb_workspace_layout(ws_ptr, n, C.byref(sp), C.byref(tot), C.byref(pf)) == 0
    return sp.value - ws_ptr, tot.value - ws_ptr, pf.value - ws_ptr


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(cuda)


def _slot(A, name, dtype=torch.int32):
    start, nbytes = A.slots[name][:2]
    return A.mem[start:start + nbytes].view(dtype)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _sentinel(*expected):
    """A word that occurs in none of the expected arrays, so a slot that still holds it was never written."""
    for c in (0xFFFFFFFF, 0xA5A5A5A5, 0x5A5A5A5A, 0x0F0F0F0F, 0xDEADBEEF, 0x13579BDF, 0x2468ACE0):
        if not any((e == np.uint32(c)).any() for e in expected):
            return c
    raise AssertionError("no free sentinel")


# ----------------------------------------------------------------------------------------------------- upsweep --
def _up_id(n, kt, desc, name):
    s = "n%d-%s-%s-%s-%s" % (n, R.upsweep_kernel_name(kt, desc), KT_NAME[kt], "desc" if desc else "asc", name)
    if name == "equal" and n > 4 * TILE:
        s += "-prefix16-at-0x8000-and-above"
    if name == "hot_by_sample" and n >= TILE:
        s += "-hot-true-on-a-mixed-batch"
    return s


_UP = [(n, kt, desc, name) for n in R.UPSWEEP_SIZES for kt, desc in R.UPSWEEP_TYPES for name in R.UPSWEEP_INPUTS]


@pytest.mark.parametrize("n,kt,desc,name", _UP, ids=[_up_id(*c) for c in _UP])
def test_upsweep_counts_and_prefixes(gs, cuda, n, kt, desc, name):
    """Spine counts and prefix16 of one upsweep, at every digit position: (U32, ascending) is lsb_upsweep_kernel<false, true>,
    the other five types the transforming kernel; the rows of the digits the field cannot hold are zero."""
    grid, tiles = _geometry(gs, n), R.num_tiles(n)
    q = gs.lib.gs_lsb_temp_bytes(n, 0)
    A = Arena(cuda, seed=n)
    A.add("ws", q, 0, "random").add("kin", 4 * n).build()
    sp, tot, pf = _layout(gs, A.ptr("ws"), n)
    ws, kin = _slot(A, "ws", torch.uint8), _slot(A, "kin")
    for shift, bits in R.DIGITS:
        keys = R.build_keys(name, n, kt, desc, shift, bits)
        staged = _dev(keys, cuda)
        kin.copy_(staged)
        ws.fill_(DIRTY)
        assert gs.lib.gs_lsb_upsweep_u32(A.ptr("ws"), q, A.ptr("kin"), n, shift, bits, desc, kt, None) == 0
        got = ws.cpu().numpy()
        assert torch.equal(kin, staged), "the upsweep changed its input"
        spine = got[sp:sp + 4 * 256 * grid].view(np.uint32).reshape(256, grid)
        prefix16 = got[pf:pf + 2 * 256 * tiles].view(np.uint16).reshape(tiles, 256)
        want_spine, want_prefix16 = R.upsweep(keys, kt, desc, shift, bits)
        where = (shift, bits)
        assert np.array_equal(spine, want_spine), where
        assert np.array_equal(prefix16, want_prefix16), where
        assert not spine[1 << bits:].any(), where                       # unused rows
        assert np.all(got[tot:tot + 1024] == DIRTY), where              # the totals are the scan's to write
        if name == "equal" and n > 4 * TILE:
            assert int(prefix16.max()) >= 0x8000
    A.check()


def _device_upsweep_reference(img, shift, bits, n):
    """(spine[256][grid], prefix16[tiles][256]) of the images, as int64 tensors on the device."""
    tiles, grid = R.num_tiles(n), R.grid_of(n)
    d = (img >> shift) & ((1 << bits) - 1)
    t = torch.arange(n, device=img.device, dtype=torch.int64) // TILE
    counts = torch.bincount(t * 256 + d, minlength=grid * R.TPC * 256).reshape(grid, R.TPC, 256)
    before = torch.cumsum(counts, dim=1) - counts
    return counts.sum(dim=1).t().contiguous(), before.reshape(grid * R.TPC, 256)[:tiles]


def _mismatch(got, want):
    """(count, first index) of the elements that differ; two numbers cross to the host."""
    bad = got.reshape(-1) != want.reshape(-1)
    count = int(bad.sum())
    return count, (int(torch.nonzero(bad)[0]) if count else -1)


@pytest.mark.parametrize("name", ["uniform", "hot_by_sample"])
def test_upsweep_beyond_one_group_of_256_workgroups(gs, cuda, name):
    """256 * 8 * 8192 + 8193 keys: chunk_of_block permutes a whole group of 256 workgroups and leaves the ragged group behind it
    alone; the last chunk holds one full tile and one key.  One type (the plain kernel); expected and compared on the device."""
    n = R.UPSWEEP_LARGE
    kt, desc = R.UPSWEEP_LARGE_TYPE
    grid, tiles = _geometry(gs, n), R.num_tiles(n)
    assert grid == 257 and tiles == 2050
    q = gs.lib.gs_lsb_temp_bytes(n, 0)
    ws = torch.full((q,), DIRTY, dtype=torch.uint8, device=cuda)
    sp, tot, pf = _layout(gs, ws.data_ptr(), n)
    g = torch.Generator(device=cuda).manual_seed(11)
    for shift, bits in ((8, 8), (29, 3)):
        img = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=cuda, generator=g)
        if name == "hot_by_sample":
            i = torch.arange(n, device=cuda, dtype=torch.int64)
            pos = i % R.BATCH
            sampled = (pos < 64) | ((pos >= 2048) & (pos < 2112))
            field = ((1 << bits) - 1) << shift
            img = torch.where(sampled, (img & ~field) | ((((i // R.BATCH) * 7 + 3) % (1 << bits)) << shift), img)
        keys = _to_i32(_t_twiddle_out(img, kt, desc))
        assert gs.lib.gs_lsb_upsweep_u32(ws.data_ptr(), q, keys.data_ptr(), n, shift, bits, desc, kt, None) == 0
        want_spine, want_prefix16 = _device_upsweep_reference(img, shift, bits, n)
        spine = ws[sp:sp + 4 * 256 * grid].view(torch.int32).to(torch.int64)
        prefix16 = ws[pf:pf + 2 * 256 * tiles].view(torch.int16).to(torch.int64) & 0xFFFF
        assert _mismatch(spine, want_spine) == (0, -1), (shift, bits)
        assert _mismatch(prefix16, want_prefix16) == (0, -1), (shift, bits)
        assert int(want_spine[1 << bits:].sum()) == 0 and int(want_spine.sum()) == n


# -------------------------------------------------------------------------------------------------------- scan --
def _scan_id(grid):
    s = "grid%d" % grid
    if grid > 1024:
        s += "-row-longer-than-%d" % (1024 * ((grid - 1) // 1024))
    if grid == 16384:
        s += "-the-2^30-keys-spine"
    if grid * R.SCAN_MAX_COUNT >= 1 << 31:
        s += "-total-at-2^31"
    return s


@pytest.mark.parametrize("grid", R.SCAN_GRIDS, ids=_scan_id)
def test_scan_of_a_synthetic_spine(gs, cuda, grid):
    """gs_lsb_scan_spine needs no keys: a [256][grid] array of counts <= 65536 goes into the spine of a workspace of the
    smallest num_items with that grid, and the rows and totals come back.  Rows 0 to 5 are all zero, all 65536, and a single
    entry at 0, 1023, 1024 and grid - 1; the others are random.  The reference asserts that every total stays below 2^32.

    From 2^28 keys on gs_lsb_temp_bytes includes the keys-only plan's block, but the layout call and the scan both carve
    with lsb_carve from the same base, so the pointers the test writes through are the ones the kernel reads."""
    n = R.items_for_grid(grid)
    assert _geometry(gs, n) == grid
    q = gs.lib.gs_lsb_temp_bytes(n, 0)
    guard = 4096
    buf = torch.full((guard + q + guard,), DIRTY, dtype=torch.uint8, device=cuda)
    ws = buf[guard:guard + q]
    assert ws.data_ptr() % 256 == 0
    sp, tot, pf = _layout(gs, ws.data_ptr(), n)
    assert sp + 4 * 256 * grid <= tot and tot + 1024 <= pf <= q
    spine = R.scan_input(grid)
    want_rows, want_totals = R.scan(spine)
    ws[sp:sp + 4 * 256 * grid].copy_(torch.from_numpy(spine.view(np.uint8).reshape(-1)).to(cuda))
    assert gs.lib.gs_lsb_scan_spine(ws.data_ptr(), q, n, None) == 0
    rows = _host(ws[sp:sp + 4 * 256 * grid], np.uint32).reshape(256, grid)
    totals = _host(ws[tot:tot + 1024], np.uint32)
    for r in range(256):
        assert np.array_equal(rows[r], want_rows[r]), "row %d (%s)" % (r, R.SCAN_ROWS[r] if r < 6 else "random")
    assert np.array_equal(totals, want_totals)
    if grid == 32769:
        assert 1 << 31 <= int(totals[1]) < 1 << 32
    # nothing but the rows and the totals changed: the gap between them, prefix16 and whatever lies behind, and the guards
    assert bool((ws[sp + 4 * 256 * grid:tot] == DIRTY).all()) and bool((ws[tot + 1024:] == DIRTY).all())
    assert bool((buf[:guard] == DIRTY).all()) and bool((buf[guard + q:] == DIRTY).all())


# --------------------------------------------------------------------------------------------------- downsweep --
def _three_calls(gs, ws_ptr, q, kin, kout, vin, vout, n, shift, bits, row):
    """The library's own upsweep and scan (verified above), then the downsweep under test."""
    key_in, key_out, desc, _ = row
    assert gs.lib.gs_lsb_upsweep_u32(ws_ptr, q, kin, n, shift, bits, desc, key_in, None) == 0
    assert gs.lib.gs_lsb_scan_spine(ws_ptr, q, n, None) == 0
    assert gs.lib.gs_lsb_downsweep_u32(ws_ptr, q, kin, kout, vin, vout, n, shift, bits, desc, key_in, key_out, None) == 0


def _run_downsweeps(gs, cuda, n, calls):
    """Host-checked downsweeps of n keys: one Arena, its buffers refilled for every call.  Outputs start as a sentinel that
    the expected result does not contain; equality with the reference then says that every element was written, the guards
    that nothing outside [0, n) was, and the input is compared with what was put there."""
    _geometry(gs, n)
    q = gs.lib.gs_lsb_temp_bytes(n, 0)
    A = Arena(cuda, seed=n)
    A.add("ws", q, 0, "random").add("kin", 4 * n).add("vin", 4 * n).add("kout", 4 * n).add("vout", 4 * n).build()
    ws, kin, vin, kout, vout = _slot(A, "ws", torch.uint8), _slot(A, "kin"), _slot(A, "vin"), _slot(A, "kout"), _slot(A, "vout")
    index = np.arange(n, dtype=np.uint32)
    staged_index = _dev(index, cuda)
    vin.copy_(staged_index)
    for row, pairs, shift, bits, name in calls:
        key_in, key_out, desc, _ = row
        where = (R.row_name(row), "pairs" if pairs else "keys", shift, bits, name)
        keys = R.build_keys(name, n, key_in, desc, shift, bits)
        want_k, want_v = R.downsweep(keys, index if pairs else None, key_in, key_out, desc, shift, bits)
        fill = _sentinel(want_k)
        staged = _dev(keys, cuda)
        kin.copy_(staged)
        ws.fill_(DIRTY)
        kout.fill_(fill - (1 << 32) if fill >= 1 << 31 else fill)
        vout.fill_(-1)
        _three_calls(gs, A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if pairs else None,
                     A.ptr("vout") if pairs else None, n, shift, bits, row)
        got_k, got_v = _host(kout, np.uint32), _host(vout, np.uint32)
        assert torch.equal(kin, staged) and torch.equal(vin, staged_index), where
        assert np.array_equal(got_k, want_k), where
        if pairs:
            assert np.array_equal(got_v, want_v), where
            if name in R.STABILITY_INPUTS:          # stable across waves, rounds and tiles: ascending inside every digit run
                d = R.digit(got_k, key_out, desc, shift, bits).astype(np.int64)
                assert np.all((np.diff(got_v.astype(np.int64)) > 0) | (np.diff(d) != 0)), where
        else:
            assert np.all(got_v == 0xFFFFFFFF), where                   # no values given: none written
    A.check()


def _size_kind(n):
    full, tail = n // TILE, n % TILE
    return ("tail-only" if not full else "full-tiles-only" if not tail else "full-and-tail") + "-" + R.shape_name(full)


_DS_SMALL = [(sid, n, row, pairs) for sid, n in R.downsweep_sizes() if n <= R.DS_EVERY_CASE_MAX
             for row in R.DOWNSWEEP_ROWS for pairs in (False, True)]


@pytest.mark.parametrize("sid,n,row,pairs", _DS_SMALL,
                         ids=["%s-%s-%s-%s" % (sid, _size_kind(n), R.row_name(row), "pairs" if p else "keys") for sid, n, row, p in _DS_SMALL])
def test_downsweep_every_digit_and_input(gs, cuda, sid, n, row, pairs):
    """One (key_type_in, key_type_out, descending) row and one form at one size, at all nine digit positions and all ten inputs.
    The full tiles run lsb_downsweep_kernel<pairs, false, TW, false> with the row's TW; the partial tile the general kernel."""
    calls = R.downsweep_calls(n, row, pairs)
    assert len(calls) == len(R.DIGITS) * len(R.DOWNSWEEP_INPUTS)
    _run_downsweeps(gs, cuda, n, calls)


_DS_MEDIUM = [(sid, n) for sid, n in R.downsweep_sizes() if R.DS_EVERY_CASE_MAX < n <= R.DS_HOST_MAX]


@pytest.mark.parametrize("sid,n", _DS_MEDIUM, ids=["%s-%s" % (sid, _size_kind(n)) for sid, n in _DS_MEDIUM])
def test_downsweep_every_row_at_each_shape_of_the_tile_map(gs, cuda, sid, n):
    """The tile counts at which tile_of_item_wide's decomposition changes shape (one group, a group and a smaller one, a
    remainder below 16): every row in both forms, three (digit position, input) pairs each, rotating."""
    calls = R.downsweep_calls(n)
    assert len(calls) == 60
    _run_downsweeps(gs, cuda, n, calls)


def _t_mask(kt, desc):
    return int(R.xor_mask(kt, desc))


def _t_twiddle_in(b, kt, desc):
    """twiddle_in on the device; b holds the keys' bit patterns as int64 in [0, 2^32)."""
    if kt == F32:
        b = b ^ torch.where(b >= 1 << 31, torch.full_like(b, 0xFFFFFFFF), torch.full_like(b, 0x80000000))
    return b ^ _t_mask(kt, desc)


def _t_twiddle_out(img, kt, desc):
    b = img ^ _t_mask(kt, desc)
    if kt == F32:
        b = b ^ torch.where(b >= 1 << 31, torch.full_like(b, 0x80000000), torch.full_like(b, 0xFFFFFFFF))
    return b


def _to_i32(b):
    return torch.where(b >= 1 << 31, b - (1 << 32), b).to(torch.int32)


def _banded(n, fill, cuda):
    """(whole tensor, the n elements in its middle): an output with BAND guard elements on either side."""
    whole = torch.full((n + 2 * BAND,), fill, dtype=torch.int32, device=cuda)
    return whole, whole[BAND:BAND + n]


def _bands_intact(whole, n, fill):
    return bool((whole[:BAND] == fill).all()) and bool((whole[BAND + n:] == fill).all())


def _downsweep_on_device(gs, cuda, n, row, pairs, shift, bits, img):
    """One downsweep whose expected result is torch.sort(stable=True) of the digit, compared on the device.  img: int64 images."""
    key_in, key_out, desc, _ = row
    where = (R.row_name(row), "pairs" if pairs else "keys", shift, bits)
    keys = _to_i32(_t_twiddle_out(img, key_in, desc))
    staged = keys.clone()
    perm = torch.sort((img >> shift) & ((1 << bits) - 1), stable=True)[1]
    want_k = _to_i32(_t_twiddle_out(img[perm], key_out, desc))
    q = gs.lib.gs_lsb_temp_bytes(n, 0)
    ws = torch.full((q,), DIRTY, dtype=torch.uint8, device=cuda)
    kw, kout = _banded(n, -1, cuda)
    vw, vout = _banded(n, -1, cuda)
    vin = torch.arange(n, dtype=torch.int32, device=cuda) if pairs else None
    _three_calls(gs, ws.data_ptr(), q, keys.data_ptr(), kout.data_ptr(), vin.data_ptr() if pairs else None,
                 vout.data_ptr() if pairs else None, n, shift, bits, row)
    assert _mismatch(kout, want_k) == (0, -1), where
    if pairs:
        assert _mismatch(vout, perm.to(torch.int32)) == (0, -1), where     # every index once, in the stable order
    else:
        assert bool((vout == -1).all()), where
    assert torch.equal(keys, staged), where
    assert _bands_intact(kw, n, -1) and _bands_intact(vw, n, -1), where


_DS_LARGE = [(sid, n) for sid, n in R.downsweep_sizes() if n > R.DS_HOST_MAX]


@pytest.mark.parametrize("sid,n", _DS_LARGE, ids=["%s-%s" % (sid, _size_kind(n)) for sid, n in _DS_LARGE])
def test_downsweep_a_thousand_tiles(gs, cuda, sid, n):
    """1000, 1024 and 1025 full tiles: ten calls, every row once, the forms alternating.  Inputs from the host builders."""
    calls = R.downsweep_calls(n)
    assert len(calls) == 10 and {c[0] for c in calls} == set(R.DOWNSWEEP_ROWS)
    for row, pairs, shift, bits, name in calls:
        img = torch.from_numpy(R.build_image(name, n, shift, bits, 0).astype(np.int64)).to(cuda)
        _downsweep_on_device(gs, cuda, n, row, pairs, shift, bits, img)


@pytest.mark.parametrize("row,pairs", [(R.DOWNSWEEP_ROWS[0], False), (R.DOWNSWEEP_ROWS[3], True), (R.DOWNSWEEP_ROWS[7], True)],
                         ids=lambda v: R.row_name(v) if isinstance(v, tuple) else ("pairs" if v else "keys"))
def test_downsweep_whole_groups_of_8192_tiles(gs, cuda, row, pairs):
    """8192 * 8192 + 16 * 8192 + 77 keys: tile_of_item_wide's full-size group, then a group of 16, then the partial tile."""
    n = R.DS_LARGE
    assert R.shape_name(n // TILE) == "1x8192+1x16" and n % TILE == 77 and n <= 1 << 30
    g = torch.Generator(device=cuda).manual_seed(n % 1000 + int(pairs))
    img = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=cuda, generator=g)
    _downsweep_on_device(gs, cuda, n, row, pairs, 8, 8, img)


# ------------------------------------------------------------------------------- route boundaries of the full sort --
_ROUTES = [(rid, n, kt, desc) for rid, n in R.ROUTE_SIZES for kt, desc in R.ROUTE_TYPES]


@pytest.mark.parametrize("rid,n,kt,desc", _ROUTES,
                         ids=["%s-n%d-%s-%s" % (rid, n, KT_NAME[kt], "desc" if desc else "asc") for rid, n, kt, desc in _ROUTES])
def test_full_sort_at_the_switch_between_the_small_and_the_large_kernels(gs, cuda, rid, n, kt, desc):
    """gs_lsb_sort_u32 with index values at 2041 to 2049 tiles: up to 2048 tiles (256 chunks, the last one ragged or full)
    lsb_upsweep_small_kernel and lsb_scan_small_kernel run, from 2049 on the kernels of the staged tests.  Keys of three
    random bytes under a constant top byte; bit ranges (0, 16) and (8, 32).  The expected permutation is the stable argsort of
    the digit field, taken with torch.sort(stable=True) on the device because the arrays are above 2^22 keys
    (tests/test_lsb_stages_cpu.py holds that sort against numpy's).  The selector flips once per pass."""
    g = torch.Generator(device=cuda).manual_seed(n % 9973 + kt)
    bits24 = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device=cuda, generator=g)
    raw = bits24 | (0x3F << 24)                                     # as floats: finite and positive
    keys = _to_i32(raw)
    img = _t_twiddle_in(raw, kt, desc)
    index = torch.arange(n, dtype=torch.int32, device=cuda)
    fn = gs.DeviceRadixSort.SortPairsDescending if desc else gs.DeviceRadixSort.SortPairs
    for begin, end in R.ROUTE_RANGES:
        perm = torch.sort((img >> begin) & ((1 << (end - begin)) - 1), stable=True)[1]
        k0w, k0 = _banded(n, -1, cuda)
        k1w, k1 = _banded(n, -1, cuda)
        v0w, v0 = _banded(n, -1, cuda)
        v1w, v1 = _banded(n, -1, cuda)
        k0.copy_(keys)
        v0.copy_(index)
        dk, dv = gs.DoubleBuffer(k0, k1), gs.DoubleBuffer(v0, v1)
        q = fn(None, 0, dk, dv, n)
        temp = torch.full((q,), DIRTY, dtype=torch.uint8, device=cuda)
        fn(temp, q, dk, dv, n, begin, end, key_type=kt)
        passes = (end - begin + 7) // 8
        assert dk.selector == dv.selector == passes & 1, (begin, end)
        assert _mismatch(dk.Current(), keys[perm]) == (0, -1), (begin, end)
        assert _mismatch(dv.Current(), perm.to(torch.int32)) == (0, -1), (begin, end)
        assert all(_bands_intact(w, n, -1) for w in (k0w, k1w, v0w, v1w)), (begin, end)


@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("over", [0, 1], ids=["at-the-single-workgroup-capacity", "one-key-above-it"])
def test_copy_form_in_two_passes(gs, cuda, over, pairs):
    """gs_lsb_sort_copy_u32 on bits (4, 20), two passes: at small_sort_capacity (one workgroup, straight from IN to OUT) and
    one key above it (the first pass writes the scratch in the workspace, the second OUT).  The input stays untouched."""
    n = msb_cases.CAP_MAX + over
    begin, end = R.COPY_RANGE
    index = np.arange(n, dtype=np.uint32)
    for kt, desc in R.ROUTE_TYPES:
        keys = R.build_keys("uniform", n, kt, desc, 8, 8, seed=over)
        order = np.argsort((R.twiddle_in(keys, kt, desc) >> np.uint32(begin)) & np.uint32((1 << (end - begin)) - 1), kind="stable")
        q = gs.lib.gs_lsb_copy_temp_bytes(n, int(pairs))
        A = Arena(cuda, seed=n + kt)
        A.add("ws", q, 0, "random").add("kin", 4 * n, data=keys, const=True).add("kout", 4 * n)
        A.add("vin", 4 * n, data=index, const=True).add("vout", 4 * n)
        A.build()
        with gs.KernelProfile() as prof:
            assert gs.lib.gs_lsb_sort_copy_u32(A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if pairs else None,
                                               A.ptr("vout") if pairs else None, n, begin, end, desc, kt, None) == 0
        A.check()                                                   # guards, and kin / vin unchanged
        launches = {name: count for name, (_, count) in prof.read().items()}
        assert launches == ({"lsb_upsweep": 2, "lsb_scan": 2, "lsb_downsweep": 2} if over else {"msb_local_sort": 1}), launches
        assert np.array_equal(A.read("kout", np.uint32), keys[order]), (KT_NAME[kt], desc)
        if pairs:
            assert np.array_equal(A.read("vout", np.uint32), order.astype(np.uint32)), (KT_NAME[kt], desc)
        else:
            assert np.all(A.read("vout", np.uint32) == 0xFFFFFFFF)
