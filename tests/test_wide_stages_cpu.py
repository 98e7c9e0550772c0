"""Guards tests/wide_stages_ref.py, the reference and the case tables of tests/test_wide_stages_gpu.py: the numpy restatement of
the wide LSB pass agrees with the oracle on a sample of every row and range; its tile-by-tile simulation of the downsweep is the
same scatter; tile_of_item is a bijection; gs_lsb_wide_temp_bytes is the restated layout; gs_lsb_sort_wide refuses what it must
before the device is touched; and the negative control: every plausible wrong kernel, written as a numpy variant of the
reference, differs from it on a named case of the GPU tables -- but for `valid` taken from the block index, which is shown to
be the kernel.  No wrong kernel ever runs on a GPU.  No GPU here."""
import ctypes as C

import numpy as np
import pytest

import wide_stages_ref as R
from wide_stages_ref import U32, I32, F32, U64, I64, F64, TILE

INVALID = 1                     # hipErrorInvalidValue


# ------------------------------------------------------------------------------------------------- key images --
def _oracle_image(oracle, keys, kt):
    """The ascending image by the oracle's own scalar twiddles."""
    L = oracle.lib()
    f = getattr(L, "orc_twiddle_in_%s%d" % ("uif"[R.kind(kt)], R.width(kt)))
    return np.array([f(int(k)) for k in keys], dtype=R.utype(R.width(kt)))


@pytest.mark.parametrize("kt", R.SORT_TYPES, ids=R.KT_NAME.get)
def test_twiddles_invert_each_other_and_order_the_keys(oracle, kt):
    w = R.width(kt)
    dt = R.utype(w)
    rng = np.random.default_rng(kt)
    edge = np.array([0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1], dtype=dt)
    raw = np.concatenate([rng.integers(0, 1 << w, 5000, dtype=dt), edge] + ([R.specials(kt)] if R.kind(kt) == R.F else []))
    for desc in (0, 1):
        img = R.twiddle_in(raw, kt, desc)
        assert img.dtype == dt and np.array_equal(R.twiddle_out(img, kt, desc), raw)
        assert np.array_equal(img, R.twiddle_in(raw, kt, 0) ^ dt(((1 << w) - 1) if desc else 0))
    assert np.array_equal(R.twiddle_in(raw, kt, 0), _oracle_image(oracle, raw, kt))
    by_image = raw[np.argsort(R.twiddle_in(raw, kt, 0), kind="stable")]
    if R.kind(kt) == R.U:
        assert np.all(by_image[1:] >= by_image[:-1])
    if R.kind(kt) == R.I:
        s = by_image.view(np.int32 if w == 32 else np.int64)
        assert np.all(s[1:] >= s[:-1])
    if R.kind(kt) == R.F:
        f = by_image.view(np.float32 if w == 32 else np.float64)
        nan = np.isnan(f)
        num = f[~nan]
        assert np.all(num[1:] >= num[:-1])
        first, last = np.flatnonzero(~nan)[[0, -1]]
        assert nan[:first].all() and nan[last + 1:].all() and first > 0 and last < f.size - 1      # negative NaNs, numbers, positive NaNs
        assert np.all(np.signbit(f[:first])) and not np.any(np.signbit(f[last + 1:]))
        assert np.all(np.diff(by_image[:first].astype(np.float64)) <= 0) and np.all(np.diff(by_image[last + 1:].astype(np.float64)) >= 0)
    # the keys whose image is all ones, the pad of a partial tile
    ones = dt((1 << w) - 1)
    want = {(R.U, 0): ones, (R.U, 1): 0, (R.I, 0): (1 << (w - 1)) - 1, (R.I, 1): 1 << (w - 1), (R.F, 0): (1 << (w - 1)) - 1, (R.F, 1): ones}
    for desc in (0, 1):
        assert int(R.twiddle_out(np.array([ones]), kt, desc)[0]) == int(want[(R.kind(kt), desc)])
    if R.kind(kt) == R.F:
        assert np.isnan(R.twiddle_out(np.array([ones]), kt, 0).view(np.float32 if w == 32 else np.float64)[0])


# ------------------------------------------------------------------------------- the reference against the oracle --
def _oracle_ranks(oracle, keys, kt, desc, begin, end):
    """Ranks of the stable sort on bits [begin, end) of the image: the oracle sorts the ascending image, taken with its own
    twiddles, as an unsigned key."""
    img = _oracle_image(oracle, keys, kt)
    if R.width(kt) == 32:
        return oracle.lsb_reference_ranks(img, begin, end, bool(desc))
    return oracle.lsb_reference_ranks_u64(img, 3, begin, end, bool(desc))


@pytest.mark.parametrize("row", R.ROWS, ids=R.row_name)
def test_one_pass_agrees_with_the_oracle_on_every_row_and_digit(oracle, row):
    kb, vb, kt, desc = row
    n = TILE + 1501
    vals = R.enumerated(n, vb) if vb else None
    index = np.arange(n, dtype=np.uint32)
    for shift, bits in R.DIGITS[8 * kb]:
        for name in ("uniform", "ones_image_tail"):
            keys = R.build_keys(name, n, kt, desc, shift, bits, seed=1)
            ranks = _oracle_ranks(oracle, keys, kt, desc, shift, shift + bits)
            ko, vo, prod = R.pass_ref(keys, vals, kt, desc, shift, bits)
            assert np.array_equal(ko, keys[ranks]), (shift, bits, name)
            if vb:
                assert np.array_equal(vo, vals[ranks])
            assert np.array_equal(R.pass_ref(keys, index, kt, desc, shift, bits)[1], ranks)
            # the products by their definitions
            dig = R.digit_of_image(R.twiddle_in(keys, kt, desc), shift, bits).astype(np.int64)
            assert np.array_equal(prod["totals"], np.bincount(dig, minlength=256))
            assert np.array_equal(prod["spine_raw"][:, 0], np.bincount(dig, minlength=256)) and not prod["spine"].any()
            assert not prod["prefix16"][0].any() and np.array_equal(prod["prefix16"][1], np.bincount(dig[:TILE], minlength=256))
            # and the kernel's own route to a destination is the same scatter
            sk, sv = R.scattered(*R.simulate_pass(keys, vals, kt, desc, shift, bits), n)
            assert np.array_equal(sk, ko) and (not vb or np.array_equal(sv, vo))


def test_typed_oracle_agrees_on_full_64_bit_sorts(oracle):
    """The oracle's typed comparison (no twiddles): U64, I64 and NaN-free F64 on all 64 bits, I64 on ranges with and without
    the sign bit."""
    n = 2 * TILE + 77
    index = np.arange(n, dtype=np.uint32)
    for kt in (U64, I64, F64):
        keys = R.build_keys("uniform_and", n, kt, 0, seed=5) if kt != F64 else \
            np.random.default_rng(6).standard_normal(n).view(np.uint64) | (np.arange(n, dtype=np.uint64) % np.uint64(3) << np.uint64(63))
        for desc in (0, 1):
            ranges = ((0, 64),) if kt == F64 else ((0, 64), (1, 63), (40, 64), (31, 33))
            for begin, end in ranges:
                ranks = oracle.lsb_reference_ranks_u64(keys, kt if end == 64 else 3, begin, end, bool(desc))
                ko, vo, sel = R.sort_ref(keys, index, kt, desc, begin, end)
                assert np.array_equal(vo, ranks) and np.array_equal(ko, keys[ranks]) and sel == R.num_passes(begin, end) & 1


@pytest.mark.parametrize("kt", R.SORT_TYPES, ids=R.KT_NAME.get)
def test_whole_sorts_agree_with_the_oracle_on_every_range(oracle, kt):
    n = 4097
    keys = R.build_keys(R.sort_input(kt), n, kt, 0, seed=2)
    index = np.arange(n, dtype=np.uint32)
    for desc in (0, 1):
        for begin, end in R.SORT_RANGES[R.width(kt)]:
            for sel in (0, 1):
                ko, vo, so = R.sort_ref(keys, index, kt, desc, begin, end, sel)
                if begin == end:
                    assert so == sel and np.array_equal(ko, keys) and np.array_equal(vo, index)
                    continue
                ranks = _oracle_ranks(oracle, keys, kt, desc, begin, end)
                assert np.array_equal(vo, ranks) and np.array_equal(ko, keys[ranks]) and so == sel ^ (R.num_passes(begin, end) & 1)
                assert np.array_equal(R.stable_order(keys, kt, desc, begin, end), ranks)
    assert R.sort_ref(keys[:0], None, kt, 0, 0, 8, 1)[2] == 1                       # no keys: the selector stays
    for begin, end in R.ANY_RANGES[R.width(kt)]:
        if begin != end:
            assert np.array_equal(R.stable_order(keys, kt, 1, begin, end), _oracle_ranks(oracle, keys, kt, 1, begin, end))
        else:
            assert np.array_equal(R.stable_order(keys, kt, 1, begin, end), index)


# ------------------------------------------------------------------------------------------------ the builders --
def test_inputs_are_what_their_names_say():
    n = 17 * TILE + 5
    for kt, desc in ((U64, 0), (I64, 1), (F64, 1), (U32, 1), (I32, 0), (F32, 0)):
        for shift, bits in R.DIGITS[R.width(kt)]:
            D = 1 << bits

            def dig(name):
                return R.digit_of_image(R.twiddle_in(R.build_keys(name, n, kt, desc, shift, bits), kt, desc), shift, bits).astype(np.int64)
            assert np.unique(dig("equal")).size == 1
            assert np.array_equal(dig("every"), np.arange(n) % D)
            d = dig("two_by_tile")
            assert np.unique(d).size == 2 and all(np.unique(d[t * TILE:(t + 1) * TILE]).size == 1 for t in range(18)) and d[0] != d[TILE]
            d = dig("two_by_key")
            assert np.unique(d).size == 2 and np.all(d[1:] != d[:-1])
            d = dig("hot_but_one")
            for lo in range(0, 17 * TILE, TILE):
                assert np.flatnonzero(d[lo:lo + TILE] != d[lo]).size == 1
            assert np.all(np.diff(dig("sorted")) >= 0) and np.all(np.diff(dig("reverse")) <= 0)
            assert np.unique(dig("uniform")).size == D
            img = R.twiddle_in(R.build_keys("ones_image_tail", n, kt, desc, shift, bits), kt, desc)
            ones = img == img.dtype.type((1 << R.width(kt)) - 1)
            assert ones[17 * TILE:].all() and 1000 < ones[:17 * TILE].sum() < 1300 and np.all(dig("ones_image_tail")[ones] == D - 1)
        # random bits outside the field: stability and a too-wide mask show in the keys themselves
        assert np.unique(R.build_keys("equal", 4096, kt, desc, 0, 8)).size > 4000
    _, _, prod = R.pass_ref(R.build_keys("equal", 9 * TILE, F64, 1, 56, 8), None, F64, 1, 56, 8)
    assert int(prod["prefix16"].max()) == 7 * TILE and int(prod["prefix16"][8].max()) == 0      # the largest prefix16 there is
    for kt in (F32, F64):
        for n in (1, 4097):
            keys = R.build_keys("special", n, kt, 0)
            assert keys.size == n
        f = keys.view(np.float32 if kt == F32 else np.float64)
        assert set(int(x) for x in R.specials(kt)) <= set(int(x) for x in keys)
        nan = np.isnan(f)
        assert {bool(s) for s in np.signbit(f[nan])} == {True, False} and np.unique(keys[nan]).size >= 8
    k = R.build_keys("uniform_and", 100003, U64, 0)
    assert 6 < np.unpackbits(k.view(np.uint8)).mean() * 64 < 10
    for vb in (4, 8):
        v = R.enumerated(100003, vb)
        assert v.dtype.itemsize == vb and np.unique(v).size == v.size and all(np.unique(v.view(np.uint8)[b::vb]).size > 200 for b in range(vb))


def test_case_tables_hold_what_the_issue_asks():
    assert len(R.ROWS) == 36 and len(set(R.ROWS)) == 36
    for row in R.ROWS:              # the full product at every size
        for n in R.SIZES:
            assert set(R.one_pass_calls(n, row)) == {(s, b, name) for s, b in R.DIGITS[8 * row[0]] for name in R.INPUTS}
    assert [n % TILE for n in R.TAIL_SIZES] == [1, 2049, 1, 5]
    assert len(R.group_cases()) == 48
    for kt in R.SORT_TYPES:
        for n in R.SORT_SIZES:
            calls = R.sort_calls(kt, 1, n)
            assert {(b, e) for b, e, _, _ in calls} == set(R.SORT_RANGES[R.width(kt)])
            assert {(s, bool(v)) for _, _, s, v in calls} == {(0, False), (0, True), (1, False), (1, True)}
    assert {v for kt in R.SORT_TYPES for n in R.SORT_SIZES for d in (0, 1) for _, _, _, v in R.sort_calls(kt, d, n)} == {0, 4, 8}


# --------------------------------------------------------------------------------------------------- geometry --
def test_tile_of_item_is_a_bijection_for_1_to_4100_tiles():
    for T in range(1, 4101):
        out = R.tile_of_item(np.arange(T), T)
        assert out.min() >= 0 and out.max() < T and np.all(np.bincount(out, minlength=T) == 1), T
        # the last tile is its own block at every size: last of a whole group (r = 511 -> 7 * 64 + 63), or in the ragged one
        assert out[T - 1] == T - 1
    out = R.tile_of_item(np.arange(512 + 3), 512 + 3)
    assert np.array_equal(out[0:512:8], np.arange(64)) and np.array_equal(out[1:512:8], 64 + np.arange(64))
    assert np.array_equal(out[512:], 512 + np.arange(3))
    assert np.array_equal(R.tile_of_item(np.arange(511), 511), np.arange(511))


def _table_sizes():
    sizes = set(R.SIZES) | set(R.TAIL_SIZES) | set(R.SORT_SIZES) | set(R.ANY_SIZES) | {0, 2, 1 << 27, (1 << 32) - 1}
    return sorted(sizes | {(T - 1) * TILE + last for T in R.GROUP_TILES for last in R.GROUP_LAST})


def test_temp_bytes_is_the_restated_layout(gs):
    for n in _table_sizes():
        sp, tot, pf, size = R.layout(n)
        assert (sp, tot) == (0, R._align(1024 * R.grid_of(n))) and pf == tot + 1024 and size == pf + R._align(512 * max(1, R.num_tiles(n)))
        for kb, vb in R.KV:
            assert gs.lib.gs_lsb_wide_temp_bytes(n, kb, vb) == R.temp_bytes(n), (n, kb, vb)
    assert R.grid_of(8 * TILE) == 1 and R.grid_of(8 * TILE + 1) == 2 and R.grid_of(0) == 1 and R.num_tiles(4097) == 2


# --------------------------------------------------------------------------------------------- argument checks --
def test_sort_wide_refuses_bad_arguments_before_the_device(gs):
    """hipErrorInvalidValue (1) before any device work, the selector and the pointer pairs left as they were; the no-ops return
    0 and leave the selector alone.  The pointers are never dereferenced."""
    lib = gs.lib
    ws, n = 0x100000, 100003
    good = dict(ws=ws, q=None, keys=(0x200000, 0x300000), vals=(0x400000, 0x500000), sel=0, n=n, kb=8, vb=8, begin=0, end=64, desc=0, kt=U64)

    def call(**kw):
        a = dict(good, **kw)
        q = lib.gs_lsb_wide_temp_bytes(min(a["n"], (1 << 32) - 1), 8, 8) if a["q"] is None else a["q"]
        keys = None if a["keys"] is None else (C.c_void_p * 2)(*a["keys"])
        vals = None if a["vals"] is None else (C.c_void_p * 2)(*a["vals"])
        sel = C.c_int(a["sel"])
        r = lib.gs_lsb_sort_wide(a["ws"], q, keys, vals, C.byref(sel), a["n"], a["kb"], a["vb"], a["begin"], a["end"], a["desc"], a["kt"], None)
        assert sel.value == a["sel"], kw                             # refused or nothing to do: the selector stays
        for arr, src in ((keys, a["keys"]), (vals, a["vals"])):
            assert arr is None or [arr[0], arr[1]] == list(src)
        return r

    q = lib.gs_lsb_wide_temp_bytes(n, 8, 8)
    for kb in (0, 1, 2, 3, 5, 16, -8):
        assert call(kb=kb, kt=U64) == INVALID and call(kb=kb, kt=U32, end=8) == INVALID
    for vb in (1, 2, 3, 5, 12, 16, -4):
        assert call(vb=vb) == INVALID
    assert call(vb=0) == INVALID and call(vals=None) == INVALID                      # values without val_bytes, and the reverse
    assert call(kb=4, kt=U32, end=32, vb=0) == INVALID and call(kb=4, kt=U32, end=32, vals=None, vb=4) == INVALID
    assert call(end=65) == INVALID and call(kb=4, kt=F32, end=33) == INVALID         # end_bit above the width
    assert call(begin=9, end=8) == INVALID and call(begin=-1) == INVALID and call(begin=64, end=63) == INVALID
    assert call(n=1 << 32) == INVALID and call(n=(1 << 32) + 5, begin=3, end=3) == INVALID
    for kt in (U32, I32, F32, 6, 12, -1):
        assert call(kt=kt) == INVALID                                                # a 32-bit (or narrow) key type with 8-byte keys
    for kt in (U64, I64, F64, 6):
        assert call(kb=4, kt=kt, end=32) == INVALID                                  # and the reverse
    assert call(sel=2) == INVALID and call(sel=-1) == INVALID and call(sel=2, n=0) == INVALID
    assert lib.gs_lsb_sort_wide(ws, q, (C.c_void_p * 2)(1, 2), None, None, n, 8, 0, 0, 64, 0, U64, None) == INVALID
    assert call(keys=None) == INVALID
    assert call(q=q - 1) == INVALID and call(ws=None) == INVALID and call(q=0) == INVALID        # one byte short
    for kb, vb, kt, end in ((4, 8, I32, 32), (8, 4, F64, 64), (4, 4, U32, 32)):
        assert call(kb=kb, vb=vb, kt=kt, end=end, q=lib.gs_lsb_wide_temp_bytes(n, kb, vb) - 1) == INVALID
    assert call(keys=(None, 0x300000)) == INVALID and call(keys=(0x200000, None)) == INVALID     # a null half of either buffer
    assert call(vals=(None, 0x500000)) == INVALID and call(vals=(0x400000, None)) == INVALID
    # nothing to do: 0, the selector as it was, whatever the workspace
    for sel in (0, 1):
        assert call(n=0, sel=sel) == 0 and call(n=0, sel=sel, ws=None, q=0) == 0
        assert call(begin=20, end=20, sel=sel) == 0 and call(begin=64, end=64, sel=sel, ws=None, q=0) == 0
        assert call(kb=4, vb=0, vals=None, kt=I32, begin=16, end=16, sel=sel) == 0
        assert call(n=0, sel=sel, keys=(None, None), vals=(None, None)) == 0
    assert call(n=0, kb=3) == INVALID and call(begin=20, end=20, kt=U32) == INVALID              # the checks come first


# -------------------------------------------------------------------------- the inputs discriminate (CPU only) --
def _one_pass_table():
    for n in R.SIZES:
        for row in R.ROWS:
            for s, b, name in R.one_pass_calls(n, row):
                yield ("one-pass", n, row, s, b, name)


def _tail_table():
    for n in R.TAIL_SIZES:
        for row in R.ROWS:
            for s, b, name in R.tail_calls(n, row):
                yield ("tail", n, row, s, b, name)


def _pass_differs(case, model):
    _, n, (kb, vb, kt, desc), shift, bits, name = case
    keys = R.build_keys(name, n, kt, desc, shift, bits)
    return R.model_differs(keys, R.enumerated(n, vb) if vb else None, kt, desc, shift, bits, (model,))


def _first(table, model, hint):
    """The first case of the table, among those the hint keeps (a shortcut for the search, not for the assertion), on which the
    model differs from the reference."""
    for case in table:
        if hint(case) and _pass_differs(case, model):
            return case[:2] + (R.row_name(case[2]),) + case[3:]
    return None


def test_the_kernel_model_without_a_fault_is_the_reference():
    for case in [c for c in _one_pass_table() if c[1] in (4097, 17 * TILE + 5)][::37]:
        assert not _pass_differs(case, "none") and not _pass_differs(case, "valid_from_block")


def test_model_pads_before_real_keys_of_the_same_digit_is_noticed():
    """Keys only, the model stores the pad where the real key of the all-ones image belongs: the same bytes, no fault.  With
    values the pad's value shows -- a clamped load of the tile's last value, so a tail of ONE key (4097, 8 * 4096 + 1) gets its
    own value back and only the tails of 2049 and 5 keys tell.  There every row with values does."""
    assert _first(_tail_table(), "pads_first", lambda c: c[2][1] != 0) == ("tail", TILE + 2049, "k64-v32-U64-asc", 0, 8, "ones_image_tail")
    for n in R.TAIL_SIZES:
        for row in R.ROWS:
            assert (_first(_tail_table(), "pads_first", lambda c: c[1] == n and c[2] == row and c[3] == 0) is not None) == (row[1] != 0 and n % TILE > 1), (n, row)
    assert _first(_tail_table(), "pads_first", lambda c: c[2][1] == 0 and c[1] == TILE + 2049) is None


def test_model_f64_out_twiddle_without_its_complement_is_noticed():
    assert _first(_one_pass_table(), "out_no_complement", lambda c: c[2][2] == F64) == ("one-pass", 1, "k64-v0-F64-asc", 0, 8, "uniform")
    assert _first(_one_pass_table(), "out_no_complement", lambda c: c[2][2] != F64 and c[1] == 4097 and c[5] == "uniform") is None
    for row in R.ROWS:
        if row[2] == F64:
            assert _first(_one_pass_table(), "out_no_complement", lambda c: c[2] == row) is not None


def test_model_complement_on_the_low_word_only_is_noticed():
    found = _first(_one_pass_table(), "xor_low_word", lambda c: c[2][0] == 8 and c[2][3] == 1 and c[3] >= 32 and c[1] > 64)
    assert found == ("one-pass", 65, "k64-v0-U64-desc", 32, 8, "uniform")
    # the sign bit of I64 lies in the high word too
    assert _first(_one_pass_table(), "xor_low_word", lambda c: c[2][2] == I64 and c[2][3] == 0 and c[3] + c[4] == 64 and c[1] > 64) is not None
    assert _first(_one_pass_table(), "xor_low_word", lambda c: c[2][0] == 4 and c[1] == 4097 and c[5] == "uniform") is None


def _sort_table():
    for kt in R.SORT_TYPES:
        for desc in (0, 1):
            for n in R.SORT_SIZES:
                for begin, end, sel, vb in R.sort_calls(kt, desc, n):
                    yield (kt, desc, n, begin, end, sel, vb)


def test_model_f_out_on_every_pass_is_noticed():
    def differs(case):
        kt, desc, n, begin, end, sel, vb = case
        keys = R.build_keys(R.sort_input(kt), n, kt, desc)
        return not np.array_equal(R.sort_ref(keys, None, kt, desc, begin, end, sel, ("f_out_every_pass",))[0], R.sort_ref(keys, None, kt, desc, begin, end, sel)[0])
    for kt, want in ((F64, (F64, 0, 1, 0, 64, 0, 0)), (F32, (F32, 0, 1, 0, 32, 0, 0))):
        assert next(c for c in _sort_table() if c[0] == kt and differs(c)) == want
    assert not any(differs(c) for c in _sort_table() if R.kind(c[0]) != R.F and c[2] <= 4097)
    assert not any(differs(c) for c in _sort_table() if c[2] == 4097 and R.num_passes(c[3], c[4]) <= 1)      # one pass: it is the last


def test_model_prefix16_restarted_every_16_tiles_is_noticed():
    found = _first(_one_pass_table(), "prefix16_every_16", lambda c: c[1] > 8 * TILE)
    assert found == ("one-pass", 8 * TILE + 1, "k64-v0-U64-asc", 0, 8, "uniform")
    assert _first(_one_pass_table(), "prefix16_every_16", lambda c: c[1] == 8 * TILE and c[2][2] in (U64, F32) and c[5] in ("uniform", "equal")) is None


def test_model_eight_bit_mask_on_a_narrower_digit_is_noticed():
    for w in (64, 32):
        for shift, bits in R.DIGITS[w]:
            tells = bits < 8 and shift + bits < w           # there are bits above the field
            found = _first(_one_pass_table(), "mask8", lambda c: 8 * c[2][0] == w and (c[3], c[4]) == (shift, bits) and (c[1] >= 64 if tells else c[1] == 4097))
            assert (found is not None) == tells, (w, shift, bits)
    assert sum(b < 8 and s + b < 64 for s, b in R.DIGITS[64]) == 2 and sum(b < 8 and s + b < 32 for s, b in R.DIGITS[32]) == 1


def test_model_ranks_reversed_inside_a_wave_is_noticed():
    assert _first(_one_pass_table(), "reverse_in_wave", lambda c: True) == ("one-pass", 1, "k64-v0-U64-asc", 63, 1, "uniform")      # one key of the pads' digit: a pad takes its place
    for row in R.ROWS:          # keys only too: the keys' other bits differ, so the order shows in the keys themselves
        assert _first(_one_pass_table(), "reverse_in_wave", lambda c: c[2] == row and c[1] >= 64) is not None


def test_model_descending_as_reversed_ascending_is_noticed():
    assert _first(_one_pass_table(), "desc_as_reversed", lambda c: c[2][3] == 1 and c[1] > 1) == ("one-pass", 63, "k64-v0-U64-desc", 0, 8, "uniform")
    for row in R.ROWS:
        assert (_first(_one_pass_table(), "desc_as_reversed", lambda c: c[2] == row and c[1] == 4097) is not None) == (row[3] == 1)


def test_model_values_through_another_key_slot_is_noticed():
    assert _first(_one_pass_table(), "value_slot_swap", lambda c: c[2][1] != 0 and c[1] > 64) == ("one-pass", 65, "k64-v32-U64-asc", 0, 8, "uniform")
    for row in R.ROWS:
        assert (_first(_one_pass_table(), "value_slot_swap", lambda c: c[2] == row and c[1] == 4097) is not None) == (row[1] != 0)


def test_model_valid_from_the_block_index_is_the_kernel():
    """`valid` from the block index instead of the mapped tile is no fault: tile_of_item maps the last tile to the block of the
    same index at every tile count (the bijection test above asserts it for 1 to 4100 tiles: the last tile of a whole group of
    512 is r = 511 -> 7 * 64 + 63, and a ragged group is the identity), and every other tile is full.  So no table can tell
    this model from the kernel; the group-shape cases still pin the partial tile behind permuted groups."""
    for T, last in ((512, 4091), (513, 4091), (1024, 4091)):
        assert R.tile_of_item(np.array([T - 1]), T)[0] == T - 1
    T, last, row, shift, bits, name = next(c for c in R.group_cases() if c[0] == 512 and c[1] == 4091 and c[2][0] == 4 and c[5] == "uniform")
    n = (T - 1) * TILE + last
    keys = R.build_keys(name, n, row[2], row[3], shift, bits)
    assert not R.model_differs(keys, None, row[2], row[3], shift, bits, ("valid_from_block",))
