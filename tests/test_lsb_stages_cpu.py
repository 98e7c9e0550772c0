"""Guards tests/lsb_stages_ref.py, the reference and the case tables of tests/test_lsb_stages_gpu.py: the numpy restatement of
the three pass kernels agrees with the oracle and with stable argsorts of the key images; tile_of_item_wide is a bijection at
every size; every plausible wrong kernel is told from the reference by at least one case of the tables (the negative control:
no wrong kernel ever runs on a GPU); the stage calls' argument checks answer before the device is touched.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import lsb_stages_ref as R
from lsb_stages_ref import U32, I32, F32, TILE

INVALID = 1                     # hipErrorInvalidValue


# ------------------------------------------------------------------------------------------------- key images --
@pytest.mark.parametrize("kt", (U32, I32, F32), ids=R.KT_NAME.get)
def test_twiddles_invert_each_other_and_order_the_keys(kt):
    rng = np.random.default_rng(kt)
    raw = np.concatenate([rng.integers(0, 1 << 32, 20000, dtype=np.uint32), R.F32_SPECIALS,
                          np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)])
    for desc in (0, 1):
        img = R.twiddle_in(raw, kt, desc)
        assert img.dtype == np.uint32 and np.array_equal(R.twiddle_out(img, kt, desc), raw)
        assert np.array_equal(img, R.twiddle_in(raw, kt, 0) ^ np.uint32(0xFFFFFFFF if desc else 0))
    by_image = raw[np.argsort(R.twiddle_in(raw, kt, 0), kind="stable")]
    if kt == U32:
        assert np.all(np.diff(by_image.astype(np.int64)) >= 0)
    if kt == I32:
        assert np.all(np.diff(by_image.view(np.int32).astype(np.int64)) >= 0)
    if kt == F32:
        f = by_image.view(np.float32)
        num = f[~np.isnan(f)]
        assert np.all(num[1:] >= num[:-1]) and np.isnan(f[0]) and np.isnan(f[-1])
        assert R.twiddle_in(np.array([0x80000000], np.uint32), F32, 0)[0] == 0x7FFFFFFF      # -0.0 just below +0.0
        assert R.twiddle_in(np.array([0], np.uint32), F32, 0)[0] == 0x80000000
    assert R.twiddle_in(np.array([0x80000000], np.uint32), I32, 0)[0] == 0
    assert R.twiddle_in(np.array([5], np.uint32), U32, 1)[0] == 0xFFFFFFFA


def test_the_oracles_twiddles_agree(oracle):
    L = oracle.lib()
    for k in [int(x) for x in R.F32_SPECIALS] + [0, 1, 0x12345678, 0x87654321]:
        one = np.array([k], np.uint32)
        assert L.orc_twiddle_in_u32(k) == R.twiddle_in(one, U32, 0)[0]
        assert L.orc_twiddle_in_i32(k) == R.twiddle_in(one, I32, 0)[0]
        assert L.orc_twiddle_in_f32(k) == R.twiddle_in(one, F32, 0)[0]
        assert L.orc_twiddle_out_f32(k) == R.twiddle_out(one, F32, 0)[0]


def test_f32_uniform_inputs_carry_the_special_values():
    for n in (65, 4096, 17 * TILE + 5):
        f = R.build_keys("uniform", n, F32, 0, 8, 8).view(np.float32)
        bits = f.view(np.uint32)
        assert {0x00000000, 0x80000000, 0x7F800000, 0xFF800000} <= set(int(x) for x in bits)
        sub = (bits & np.uint32(0x7F800000) == 0) & (bits & np.uint32(0x007FFFFF) != 0)
        assert {bool(s) for s in np.signbit(f[sub])} == {True, False}
        assert {bool(s) for s in np.signbit(f[np.isnan(f)])} == {True, False}


# ------------------------------------------------------------------------------- the reference against the oracle --
@pytest.mark.parametrize("shift,bits", R.DIGITS)
@pytest.mark.parametrize("n", [1, 8191, 8 * TILE + 1, 17 * TILE + 5])
def test_three_stages_agree_with_the_oracle_for_u32_ascending(oracle, n, shift, bits):
    keys, vals = oracle.gen_uniform(n, seed=shift + bits), oracle.gen_enumerated(n)
    spine, prefix16 = R.upsweep(keys, U32, 0, shift, bits)
    grid = R.grid_of(n)
    want = oracle.upsweep(keys, shift, bits, R.TILE, R.TPC, grid)
    assert spine.shape == (256, grid) and np.array_equal(spine[:1 << bits].reshape(-1), want) and not spine[1 << bits:].any()
    dig = R.digit(keys, U32, 0, shift, bits)
    for t in range(R.num_tiles(n)):                 # prefix16 by its definition, tile by tile
        c0 = (t // R.TPC) * R.TPC
        assert np.array_equal(prefix16[t].astype(np.int64), np.bincount(dig[c0 * TILE:t * TILE], minlength=256))
    rows, totals = R.scan(spine)
    flat = (rows + (np.cumsum(totals, dtype=np.uint64) - totals).astype(np.uint32)[:, None])[:1 << bits].reshape(-1)
    assert np.array_equal(flat, oracle.exclusive_scan(want))
    ko, vo = R.downsweep(keys, vals, U32, U32, 0, shift, bits)
    wk, wv = oracle.downsweep(keys, vals, shift, bits)
    assert np.array_equal(ko, wk) and np.array_equal(vo, wv)
    ko, none = R.downsweep(keys, None, U32, U32, 0, shift, bits)
    assert none is None and np.array_equal(ko, wk)


def test_passes_chained_are_the_oracles_sort(oracle):
    n = 3 * TILE + 77
    keys, vals = oracle.gen_uniform(n, seed=9), oracle.gen_enumerated(n)
    for begin, end in ((0, 32), (4, 20), (8, 32), (3, 4)):
        k, v = keys, vals
        for shift in range(begin, end, 8):
            k, v = R.downsweep(k, v, U32, U32, 0, shift, min(8, end - shift))
        wk, wv = oracle.lsb_sort_pairs(keys, vals, begin, end)
        assert np.array_equal(k, wk) and np.array_equal(v, wv)


@pytest.mark.parametrize("row", R.DOWNSWEEP_ROWS, ids=R.row_name)
def test_downsweep_is_the_stable_argsort_of_the_image(row):
    kin, kout, desc, _ = row
    n = 2 * TILE + 513
    vals = np.arange(n, dtype=np.uint32)
    for shift, bits in R.DIGITS:
        keys = R.build_keys("uniform", n, kin, desc, shift, bits, seed=3)
        img = R.twiddle_in(keys, kin, desc)
        order = np.argsort((img >> np.uint32(shift)) & np.uint32((1 << bits) - 1), kind="stable")
        ko, vo = R.downsweep(keys, vals, kin, kout, desc, shift, bits)
        assert np.array_equal(vo, order) and np.array_equal(R.twiddle_in(ko, kout, desc), img[order])
        if kin == kout:
            assert np.array_equal(ko, keys[order])
        # the kernel's own route to a destination (digit start + scanned chunk + prefix16 + rank in tile) is the same scatter
        dst = R.destinations(R.digit_of_image(img, shift, bits), bits)
        assert np.array_equal(dst[order], np.arange(n))


@pytest.mark.parametrize("kt", (I32, F32), ids=R.KT_NAME.get)
def test_a_sort_in_four_staged_passes_orders_the_keys(kt):
    """First pass kt -> U32 (keys leave twiddled), two middle passes, last pass U32 -> kt: the type's ascending stable sort."""
    n = TILE + 4097
    keys = R.build_keys("uniform", n, kt, 0, 0, 8, seed=kt)
    k, v = keys, np.arange(n, dtype=np.uint32)
    for p, (a, b) in enumerate(((kt, U32), (U32, U32), (U32, U32), (U32, kt))):
        k, v = R.downsweep(k, v, a, b, 0, 8 * p, 8)
    order = np.argsort(R.twiddle_in(keys, kt, 0), kind="stable")
    assert np.array_equal(k, keys[order]) and np.array_equal(v, order)


def test_torch_stable_sort_is_numpys_stable_argsort():
    """The cases above 2^22 keys take their expected permutation from torch.sort(stable=True) of the digit field."""
    rng = np.random.default_rng(4)
    for width in (1, 8, 16, 24):
        d = rng.integers(0, 1 << width, 200001, dtype=np.int64)
        assert np.array_equal(torch.sort(torch.from_numpy(d), stable=True)[1].numpy(), np.argsort(d, kind="stable"))


# ------------------------------------------------------------------------------------------------ the builders --
@pytest.mark.parametrize("shift,bits", R.DIGITS)
def test_inputs_are_what_their_names_say(shift, bits):
    D, n = 1 << bits, 17 * TILE + 5
    for kt, desc in R.UPSWEEP_TYPES:
        def dig(name, n=n):
            return R.digit(R.build_keys(name, n, kt, desc, shift, bits), kt, desc, shift, bits).astype(np.int64)
        sampled = R.sampled_positions(n)
        assert sampled[:64].all() and sampled[2048:2112].all() and sampled[:4096].sum() == 128
        assert np.unique(dig("equal")).size == 1
        assert np.array_equal(dig("every"), np.arange(n) % D)
        d = dig("two_by_tile")
        assert np.unique(d).size == 2 and all(np.unique(d[t * TILE:(t + 1) * TILE]).size == 1 for t in range(18)) and d[0] != d[TILE]
        d = dig("two_by_key")
        assert np.unique(d).size == 2 and np.all(d[1:] != d[:-1])
        d = dig("hot_by_sample")
        for lo in range(0, 17 * TILE, R.BATCH):
            b = d[lo:lo + R.BATCH]
            assert np.unique(b[:64]).size == 1 and np.array_equal(b[2048:2112], b[:64]) and np.unique(b).size > 1
        d = dig("hot_but_one")
        for lo in range(0, 17 * TILE, R.BATCH):
            b = d[lo:lo + R.BATCH]
            odd = np.flatnonzero(b != b[0])
            assert odd.size == 1 and not sampled[odd[0]]
        d = dig("sample_differs")
        rest = d[~sampled]
        assert np.unique(rest).size == 1 and np.all(d[sampled] != rest[0])
        assert np.all(np.diff(dig("sorted")) >= 0) and np.all(np.diff(dig("reverse")) <= 0)
        d = dig("last_digit_tail")
        assert np.all(d[17 * TILE:] == D - 1) and np.unique(d[:17 * TILE]).size == min(D, 256)
        for name, s in (("one_stranger_0", 0), ("one_stranger_max", D - 1)):
            d = dig(name)
            at = np.flatnonzero(d == s)
            assert np.array_equal(at, np.sort(np.concatenate([np.arange(18) * TILE, np.arange(1, 18) * TILE - 1, [n - 1]])))
            assert np.unique(d[d != s]).size == 1
    # random bits outside the field: stability and a too-wide digit mask show in the keys
    img = R.build_image("equal", 4096, shift, bits, 0)
    assert np.unique(img).size > 4000


def test_prefix16_reaches_0x8000_and_scan_totals_2_to_the_31():
    _, prefix16 = R.upsweep(R.build_keys("equal", 9 * TILE, I32, 1, 8, 8), I32, 1, 8, 8)
    assert sorted(set(int(x) for x in prefix16.max(axis=1))) == [0x2000 * j for j in range(8)]        # ... 0x8000 ... 0xE000
    for grid in R.SCAN_GRIDS:
        s = R.scan_input(grid)
        assert s.shape == (256, grid) and int(s.max()) <= R.SCAN_MAX_COUNT and R.grid_of(R.items_for_grid(grid)) == grid
        assert R.grid_of(R.items_for_grid(grid) - 1) == max(1, grid - 1)
        assert not s[0].any() and np.all(s[1] == R.SCAN_MAX_COUNT)
        for row, at in ((2, 0), (3, 1023), (4, 1024), (5, grid - 1)):
            assert np.count_nonzero(s[row]) == (1 if at < grid else 0) and (at >= grid or s[row, at])
        rows, totals = R.scan(s)                                        # asserts every total < 2^32
        assert np.array_equal(totals.astype(np.uint64), s.sum(axis=1, dtype=np.uint64))
        assert np.array_equal(R.model_scan(s, 1)[0], rows) and np.array_equal(R.model_scan(s, 1)[1], totals)
    assert 1 << 31 <= int(R.scan(R.scan_input(32769))[1][1]) < 1 << 32
    with pytest.raises(AssertionError):
        R.scan(np.full((256, 65537), 65536, dtype=np.uint32))


def test_case_tables_hold_what_the_branches_need():
    assert len(R.DOWNSWEEP_ROWS) == 10 and {r[3] for r in R.DOWNSWEEP_ROWS} == {0, 1, 2}
    ids = [i for i, _ in R.downsweep_sizes()]
    assert len(ids) == len(set(ids)) == 7 + 18 + 8
    shapes = {t: R.shape_name(t) for t in R.DS_FULL_TILES}
    assert shapes[1] == "id1" and shapes[15] == "id15" and shapes[16] == "1x16" and shapes[17] == "1x16+id1"
    assert shapes[48] == "1x32+1x16" and shapes[63] == "1x32+1x16+id15" and shapes[1000] == "1x512+1x256+1x128+1x64+1x32+id8"
    assert R.shape_name(R.DS_LARGE // TILE) == "1x8192+1x16" and R.DS_LARGE % TILE == 77
    for _, n in R.downsweep_sizes():
        calls = R.downsweep_calls(n)
        assert {c[0] for c in calls} == set(R.DOWNSWEEP_ROWS)
        if n <= R.DS_HOST_MAX:
            assert {(c[0], c[1]) for c in calls} == {(r, p) for r in R.DOWNSWEEP_ROWS for p in (False, True)}
        if n <= R.DS_EVERY_CASE_MAX:
            assert len(set(calls)) == 10 * 2 * 9 * len(R.DOWNSWEEP_INPUTS)
    rotated = [c for _, n in R.downsweep_sizes() if n > R.DS_EVERY_CASE_MAX for c in R.downsweep_calls(n)]
    assert {(c[2], c[3]) for c in rotated} == set(R.DIGITS) and {c[4] for c in rotated} == set(R.DOWNSWEEP_INPUTS)
    assert R.grid_of(R.UPSWEEP_LARGE) == 257 and R.num_tiles(R.UPSWEEP_LARGE) == 2050 and R.UPSWEEP_LARGE % TILE == 1
    assert [R.num_tiles(n) for _, n in R.ROUTE_SIZES] == [2041, 2048, 2048, 2049, 2049]


# --------------------------------------------------------------------------------------------------- bijection --
def _is_bijection(T):
    out = R.tile_of_item_wide(np.arange(T), T)
    return out.min() >= 0 and out.max() < T and np.all(np.bincount(out, minlength=T) == 1)


@pytest.mark.parametrize("lo", range(1, 20001, 4000))
def test_tile_of_item_wide_is_a_bijection_up_to_20000_tiles(lo):
    for T in range(lo, lo + 4000):
        assert _is_bijection(T), T


def test_tile_of_item_wide_is_a_bijection_where_its_groups_change_shape():
    top = 524287                                    # num_items < 2^32: at most this many full tiles
    sizes = {top}
    for k in range(0, 20):
        sizes |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    for m in range(1, 64):
        sizes |= {8192 * m + r for r in (0, 1, 15, 16, 17, 4095, 8191)}
    for T in sorted(s for s in sizes if 1 <= s <= top):
        assert _is_bijection(T), T
    # and it is the layout the header describes: inside a group, the items of one XCD (i % 8) take consecutive tiles
    out = R.tile_of_item_wide(np.arange(8192 + 16 + 3), 8192 + 16 + 3)
    assert np.array_equal(out[0:8192:8], np.arange(1024)) and np.array_equal(out[1:8192:8], 1024 + np.arange(1024))
    assert np.array_equal(out[8192:8208], 8192 + np.array([0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]))
    assert np.array_equal(out[8208:], 8208 + np.arange(3))


# -------------------------------------------------------------------------- the inputs discriminate (CPU only) --
def _upsweep_table():
    for n in R.UPSWEEP_SIZES:
        for case in R.upsweep_cases(n):
            yield (n,) + case


def _downsweep_table():
    for _, n in R.downsweep_sizes():
        if n <= R.DS_HOST_MAX:
            for case in R.downsweep_calls(n):
                yield (n,) + case


def _first(table, differs, hint):
    """The first case of the table, among those the hint keeps (a shortcut for the search, not for the assertion), on which
    the model differs from the reference."""
    for case in table:
        if hint(case) and differs(case):
            return case
    return None


def _ds_digits(case):
    n, (kin, kout, desc, _), pairs, shift, bits, name = case
    keys = R.build_keys(name, n, kin, desc, shift, bits)
    return keys, R.digit(keys, kin, desc, shift, bits)


def test_model_a_prefix16_read_as_signed_is_noticed():
    def differs(case):
        _, dig = _ds_digits(case)
        return not np.array_equal(R.destinations(dig, case[4], prefix_signed=True), R.destinations(dig, case[4]))
    found = _first(_downsweep_table(), differs, lambda c: c[0] >= 5 * TILE and c[5] == "equal")
    assert found is not None and found[0] <= R.DS_EVERY_CASE_MAX, found
    # and the upsweep's own table holds a prefix16 entry at or above 0x8000 (the value a signed read would change)
    assert any(int(R.upsweep(R.build_keys(name, n, kt, desc, s, b), kt, desc, s, b)[1].max()) >= 0x8000
               for n in R.UPSWEEP_SIZES if n >= 8 * TILE - 1 for kt, desc, s, b, name in R.upsweep_cases(n)[:7] if name == "equal")


@pytest.mark.parametrize("factor,what", [(0, "b-no-carry"), (2, "c-carry-twice")])
def test_models_b_c_scan_carry_dropped_or_doubled_is_noticed(factor, what):
    telling = []
    for grid in R.SCAN_GRIDS:
        s = R.scan_input(grid)
        rows, totals = R.scan(s)
        mrows, mtotals = R.model_scan(s, factor)
        if not (np.array_equal(mrows, rows) and np.array_equal(mtotals, totals)):
            telling.append(grid)
        for row in (1, 3, 6):               # full, one entry at 1023, random: each tells as soon as there is a second segment
            assert np.array_equal(mrows[row], rows[row]) == (grid <= 1024), (grid, row)
        assert np.array_equal(mrows[4], rows[4]) == (grid <= 2048), grid       # one entry at 1024: from the third segment on
    assert telling == [g for g in R.SCAN_GRIDS if g > 1024] and len(telling) >= 7


def test_model_d_hot_batch_counted_as_one_digit_is_noticed():
    def differs(case):
        n, kt, desc, shift, bits, name = case
        dig = R.digit(R.build_keys(name, n, kt, desc, shift, bits), kt, desc, shift, bits)
        return not np.array_equal(R.model_hot_upsweep_counts(dig), R.tile_counts(dig))
    for name in ("hot_by_sample", "hot_but_one"):
        for kernel in ("plain", "transform"):
            found = _first(_upsweep_table(), differs, lambda c: c[5] == name and c[0] >= TILE and R.upsweep_kernel_name(c[1], c[2]) == kernel)
            assert found is not None, (name, kernel)
    # the model is the reference where no batch is hot, and where a hot batch really holds one digit
    for name in ("every", "equal"):
        dig = R.digits_of(name, 2 * TILE + 5, 8, np.random.default_rng(0))
        assert np.array_equal(R.model_hot_upsweep_counts(dig), R.tile_counts(dig))


def test_model_e_unstable_inside_a_wave_is_noticed():
    def differs(case):
        _, dig = _ds_digits(case)
        return not np.array_equal(R.destinations(dig, case[4], reverse_in_wave=True), R.destinations(dig, case[4]))
    for pairs in (False, True):         # keys only: the keys' other bits differ, so the order shows in the keys themselves
        for name in R.STABILITY_INPUTS + ("uniform",):
            found = _first(_downsweep_table(), differs, lambda c: c[2] == pairs and c[5] == name and c[0] >= 64)
            assert found is not None, (pairs, name)
            keys, dig = _ds_digits(found)
            dst = R.destinations(dig, found[4], reverse_in_wave=True)
            assert np.array_equal(np.sort(dst), np.arange(keys.size))       # still a permutation: only the order inside runs is off
            out = np.empty_like(keys)
            out[dst] = keys
            assert not np.array_equal(out, R.downsweep(keys, None, found[1][0], found[1][0], found[1][2], found[3], found[4])[0])


def test_model_f_pad_keys_before_the_last_digit_is_noticed():
    def differs(case):
        _, dig = _ds_digits(case)
        return not np.array_equal(R.destinations(dig, case[4], pads_first=True), R.destinations(dig, case[4]))
    for hint in (lambda c: c[5] == "last_digit_tail" and c[0] < TILE, lambda c: c[5] == "last_digit_tail" and c[0] > TILE and c[0] % TILE):
        assert _first(_downsweep_table(), differs, hint) is not None
    for row in R.DOWNSWEEP_ROWS:         # the pad is the key whose image is all ones, whatever the in-type
        assert _first(_downsweep_table(), differs, lambda c: c[1] == row and c[5] == "last_digit_tail" and c[0] % TILE) is not None
    full_only = R.digits_of("last_digit_tail", 2 * TILE, 8, np.random.default_rng(0))
    assert np.array_equal(R.destinations(full_only, 8, pads_first=True), R.destinations(full_only, 8))


def test_model_g_out_twiddle_of_the_in_type_is_noticed():
    def differs(row):
        def f(case):
            n, (kin, kout, desc, _), pairs, shift, bits, name = case
            keys = R.build_keys(name, n, kin, desc, shift, bits)
            return not np.array_equal(R.downsweep(keys, None, kin, kin, desc, shift, bits)[0], R.downsweep(keys, None, kin, kout, desc, shift, bits)[0])
        return f
    for row in R.DOWNSWEEP_ROWS:
        if row[0] != row[1]:            # (rows of one type: the model is the kernel)
            assert _first(_downsweep_table(), differs(row), lambda c: c[1] == row) is not None, row
    assert sum(r[0] != r[1] for r in R.DOWNSWEEP_ROWS) == 4


def test_model_h_eight_bit_mask_on_a_narrow_digit_is_noticed():
    def up_differs(case):
        n, kt, desc, shift, bits, name = case
        keys = R.build_keys(name, n, kt, desc, shift, bits)
        return not np.array_equal(R.upsweep(keys, kt, desc, shift, 8)[0], R.upsweep(keys, kt, desc, shift, bits)[0])

    def down_differs(case):
        n, (kin, kout, desc, _), pairs, shift, bits, name = case
        keys = R.build_keys(name, n, kin, desc, shift, bits)
        return not np.array_equal(R.downsweep(keys, None, kin, kout, desc, shift, 8)[0], R.downsweep(keys, None, kin, kout, desc, shift, bits)[0])
    for shift, bits in R.DIGITS:
        if bits < 8 and shift + bits < 32:          # there are bits above the field
            assert _first(_upsweep_table(), up_differs, lambda c: (c[3], c[4]) == (shift, bits) and c[0] >= 64) is not None
            assert _first(_downsweep_table(), down_differs, lambda c: (c[3], c[4]) == (shift, bits) and c[0] >= 64) is not None
        else:
            assert not up_differs((4097, F32, 1, shift, bits, "uniform"))
    assert sum(b < 8 and s + b < 32 for s, b in R.DIGITS) == 2


# --------------------------------------------------------------------------------------------- argument checks --
def test_stage_calls_refuse_bad_arguments_before_the_device(gs):
    """hipErrorInvalidValue (1) before any device work: the pointers are never dereferenced."""
    lib = gs.lib
    ws, kin, kout, vin, vout, n = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 100003
    q = lib.gs_lsb_temp_bytes(n, 0)

    def up(ws=ws, q=q, n=n, shift=8, bits=8):
        return lib.gs_lsb_upsweep_u32(ws, q, kin, n, shift, bits, 0, gs.GS_KEY_U32, None)

    def down(ws=ws, q=q, n=n, shift=8, bits=8, vin=None, vout=None):
        return lib.gs_lsb_downsweep_u32(ws, q, kin, kout, vin, vout, n, shift, bits, 0, gs.GS_KEY_I32, gs.GS_KEY_F32, None)

    def scan(ws=ws, q=q, n=n):
        return lib.gs_lsb_scan_spine(ws, q, n, None)

    for call in (up, down):
        assert call(bits=0) == INVALID and call(bits=9) == INVALID
        assert call(shift=25, bits=8) == INVALID and call(shift=32, bits=1) == INVALID        # shift + bits > 32
        assert call(shift=-1) == INVALID
    for call in (up, down, scan):
        assert call(n=1 << 32, q=lib.gs_lsb_temp_bytes((1 << 32) - 1, 0)) == INVALID
        assert call(ws=None) == INVALID
        assert call(q=q - 1) == INVALID                                                         # one byte short
        assert call(n=0) == 0 and call(n=0, q=lib.gs_lsb_temp_bytes(0, 0)) == 0
    assert down(vin=vin) == INVALID and down(vout=vout) == INVALID                              # values in without values out
    assert down(n=0, vin=vin, vout=vout) == 0
    for big in (1 << 28, (1 << 31) + 1):            # the sizes whose workspace carries the keys-only plan's block
        qb = lib.gs_lsb_temp_bytes(big, 0)
        assert up(n=big, q=qb - 1) == INVALID and scan(n=big, q=qb - 1) == INVALID and down(n=big, q=qb - 1) == INVALID


def test_geometry_is_the_references(gs):
    g, t, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    for n in list(R.UPSWEEP_SIZES) + [R.UPSWEEP_LARGE, R.DS_LARGE] + [R.items_for_grid(x) for x in R.SCAN_GRIDS] + [n for _, n in R.downsweep_sizes()]:
        gs.lib.gs_lsb_geometry(n, 0, C.byref(g), C.byref(t), C.byref(c))
        assert (g.value, t.value, c.value) == (R.grid_of(n), R.TILE, R.TPC), n
