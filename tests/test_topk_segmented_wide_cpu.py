"""gs_topk_segmented_u64 without a device: the per-segment reference against a plain sorted() with a key, the 64-bit image round
trips, the widening identity, the long-segment model with the select's byte skip, the workspace query against the header's
formula (and within [the 32-bit query, twice it]), every refusal and no-op of the contract in the order of the checks, the one
plan for three widths, and the argument checks of the Python front ends on host tensors."""
import ctypes as C

import numpy as np
import pytest

import topk_ref as R
import topk_rows_wide_ref as WR
import topk_segmented_ref as SR
import topk_segmented_wide_ref as SW
from test_topk_segmented_cpu import KS, NS, SS

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U64, I64, F64 = SW.KEY_TYPES
CH = SR.CH


def _call(gs, temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc=0, kt=U64):
    return gs.lib.gs_topk_segmented_u64(temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc, kt, None)


def _tb(gs, n, S, k, hv):
    return gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)


# ------------------------------------------------------------------------------------------------ the reference --
def _sort_key(kt, descending):
    """A Python key function that states the order in words: integers as they are, doubles by sign and magnitude, negative
    NaNs first and positive NaNs last (the order at the enum), all of it reversed when descending."""
    def asc(bits):
        bits = int(bits)
        if kt == U64:
            return bits
        if kt == I64:
            return bits - (1 << 64) if bits >> 63 else bits
        sign, mag = bits >> 63, bits & ((1 << 63) - 1)
        return (0, -mag) if sign else (1, mag)

    def neg(v):
        return tuple(-x for x in v) if isinstance(v, tuple) else -v
    return (lambda bits: neg(asc(bits))) if descending else asc


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kt", SW.KEY_TYPES)
def test_segment_reference_is_a_plain_stable_sorted_with_a_key(kt, descending):
    """Ties (30 % one key), the specials, clamped, empty, reversed and repeated segments; Python's sorted() is stable."""
    rng = np.random.default_rng(11 + kt)
    n = 3000
    keys = SW.W.gen64("special", n, seed=5, kt=kt)
    keys[rng.random(n) < 0.3] = np.uint64(0x3FF0000000000000)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    begin = np.array([0, 10, 500, 2000, 1500, -5, 2990, 100, 100, 1, 10], np.int32)
    end = np.array([10, 400, 500, 2999, 1600, 7, 3100, 50, 101, 2998, 400], np.int32)
    key_fn = _sort_key(kt, descending)
    for k in (1, 100, 1024):
        ko, po, counts = SW.seg_topk64(keys, begin, end, k, kt, descending)
        kv, vo, _ = SW.seg_topk64(keys, begin, end, k, kt, descending, vals)
        assert ko.dtype == np.uint64 and po.dtype == np.uint32 and counts.dtype == np.uint32
        for s in range(begin.size):
            lo, hi = max(int(begin[s]), 0), min(int(end[s]), n)
            kept = min(k, max(hi - lo, 0))
            assert counts[s] == kept
            assert (ko[s, kept:] == SW.FILL64).all() and (po[s, kept:] == SW.FILL).all()
            if kept:
                want = sorted(range(hi - lo), key=lambda j: key_fn(keys[lo + j]))[:kept]
                assert list(po[s, :kept]) == want and np.array_equal(ko[s, :kept], keys[lo:hi][want])
                assert np.array_equal(kv[s, :kept], ko[s, :kept]) and np.array_equal(vo[s, :kept], vals[lo:hi][want])
    assert list(SW.seg_topk64(keys, begin, end, 5, kt)[2]) == [5, 5, 0, 5, 5, 5, 5, 0, 1, 5, 5]


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kt", SW.KEY_TYPES)
def test_image_round_trips_and_keeps_the_order(kt, descending):
    keys = np.concatenate([SW.W.specials64(kt), SW.W.gen64("uniform", 500, 3), SW.W.gen64("normal", 500, 4), SW.W.gen64("small", 100, 5)])
    img = SW.image(keys, kt, descending)
    assert img.dtype == np.uint64 and np.array_equal(SW.preimage(img, kt, descending), keys)
    assert np.array_equal(SW.image(keys, kt, not descending), ~img)
    key_fn = _sort_key(kt, descending)
    order = np.argsort(img, kind="stable")
    assert list(order) == sorted(range(keys.size), key=lambda j: key_fn(keys[j]))


def test_reference_orders_the_specials_as_stated_at_the_enum():
    pnan, nnan, pinf, ninf = 0x7FF8000000000001, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000
    keys = np.array([pnan, 0, pinf, 1 << 63, ninf, nnan], np.uint64)
    ko, po, _ = SW.seg_topk64(keys, [0], [6], 6, F64)
    assert list(ko[0]) == [nnan, ninf, 1 << 63, 0, pinf, pnan] and list(po[0]) == [5, 4, 3, 1, 2, 0]
    ko, _, _ = SW.seg_topk64(keys, [0], [6], 6, F64, True)
    assert list(ko[0]) == [pnan, pinf, 0, 1 << 63, ninf, nnan]
    ko, _, _ = SW.seg_topk64(np.array([(1 << 63) - 1, 0, (1 << 64) - 1, 1 << 63], np.uint64), [0], [4], 4, I64)
    assert list(ko[0]) == [1 << 63, (1 << 64) - 1, 0, (1 << 63) - 1]


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kt32", [R.U32, R.I32, R.F32])
def test_widening_identity_in_numpy(kt32, descending):
    """The 64-bit reference on (uint64_t)key << 32 with the key type widened is the 32-bit reference, the keys shifted."""
    rng = np.random.default_rng(3 + kt32)
    n = 6000
    keys32 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys32[rng.random(n) < 0.2] = 0x3F800000
    keys32[:6] = [0x7FC00001, 0xFFC00001, 0, 0x80000000, 0x7F800000, 0xFF800000]
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    begin = np.array([0, 100, 700, 5990, -3, 3000, 50], np.int32)
    end = np.array([100, 700, 5000, 7000, 6, 3000, 49], np.int32)
    for k in (1, 64, 1000):
        for v in (None, vals):
            wk, wv, wc = SW.via_widening(keys32, begin, end, k, kt32, descending, v)
            ko, vo, counts = SW.seg_topk64(WR.widen32(keys32), begin, end, k, SW.WIDE[kt32], descending, v)
            assert np.array_equal(ko, wk) and np.array_equal(vo, wv) and np.array_equal(counts, wc)


# ------------------------------------------------------------------------- the model of the long-segment kernels --
def _plain(img, k):
    order = np.argsort(img, kind="stable")[:k]
    return img[order], order.astype(np.uint32)


@pytest.mark.parametrize("ch,k,n", [(64, 8, 64 * 9 + 1), (64, 16, 1000), (32, 31, 777), (64, 1, 200)])
def test_stream_model_with_the_byte_skip_is_the_stable_sort(ch, k, n):
    for seed, kind in enumerate(SW.W.DISTS):
        keys = SW.W.gen64(kind, n, seed=seed + 1, kt=F64)
        for kt, desc in ((U64, False), (I64, True), (F64, False)):
            ko, po, rounds, ran = SW.stream_model64(keys, k, kt, desc, ch=ch)
            wk, wp = _plain(SW.image(keys, kt, desc), k)
            assert np.array_equal(ko, SW.preimage(wk, kt, desc)) and np.array_equal(po, wp), (kind, kt, desc)
            assert rounds == SR.final_rounds(n, k, ch) == len(ran)
            if kind == "small" and kt == U64 and not desc:
                assert all(set(r) <= {0, 1, 2} for r in ran)       # integers below 2^24: five of the eight rounds never run


def test_select_skip_runs_a_round_exactly_for_the_bytes_that_differ():
    for b in range(8):
        img = WR.one_byte_rows(1, 300, b, seed=b)[0]
        kth, less, ran = SW.select_skip(img, 100)
        assert ran == [b] and kth == np.sort(img)[99] and less == int((img < kth).sum())
    kth, less, ran = SW.select_skip(WR.one_key_rows(1, 300)[0], 7)
    assert ran == [] and kth == WR.BASE and less == 0
    img = WR.outlier_rows(1, 300, 5, 299, seed=1)[0]
    assert SW.select_skip(img, 10)[2] == [5, 0]


def test_the_reduction_of_a_streaming_round_must_see_the_carried_pairs():
    """A byte that is constant among a round's new candidates but differs in one carried element still needs its round: the
    model whose AND / OR see the new candidates alone gives a wrong answer on these segments, the right one the stable sort."""
    k, ch = 16, 128
    n = 15 * ch + 1
    for b in range(8):
        m = np.uint64(0xFF) << np.uint64(8 * b)
        small = (WR.BASE & ~m) | (np.uint64(1) << np.uint64(8 * b))
        img = np.full(n, WR.BASE + np.uint64(1), np.uint64)
        img[:k] = WR.BASE
        img[5] = small                                       # carried from round one on; the later candidates are one image
        ko, po, rounds, ran = SW.stream_model64(img, k, U64, ch=ch)
        wk, wp = _plain(img, k)
        assert rounds >= 2 and np.array_equal(ko, wk) and np.array_equal(po, wp) and po[0] == 5
        assert all(b in r for r in ran)                      # byte b gets its round in every streaming round
        bad = SW.stream_model64(img, k, U64, ch=ch, variant="reduce_new_only")
        assert not (np.array_equal(bad[0], wk) and np.array_equal(bad[1], wp))
        # the mirror: the carried pairs are all equal, the outlier is a new candidate of the last round
        img = np.full(n, WR.BASE, np.uint64)
        img[n - 1] = small
        ko, po, rounds, ran = SW.stream_model64(img, k, U64, ch=ch)
        assert po[0] == n - 1 and list(po[1:]) == list(range(k - 1)) and ko[0] == small and (ko[1:] == WR.BASE).all()
        assert ran[-1] == [b] and all(r == [] for r in ran[:-1])


# --------------------------------------------------------------------------------------------- the size query --
def test_temp_bytes_is_the_headers_formula_within_the_32_bit_query_and_twice_it(gs):
    for n in NS:
        for S in SS:
            for k in KS + [1025]:
                for hv in (0, 1):
                    got, q32 = _tb(gs, n, S, k, hv), gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
                    assert got % 256 == 0 and got == SW.temp_bytes64(n, S, k, hv), (n, S, k, hv)
                    assert q32 <= got <= 2 * q32 and (got == 0) == (q32 == 0), (n, S, k, hv)
    rng = np.random.default_rng(7)
    larger = 0
    for _ in range(400):
        n = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        S = int(rng.integers(1, 1 << int(rng.integers(1, 23))))
        k = int(rng.integers(1, 1100))
        hv = int(rng.integers(0, 2))
        got, q32 = _tb(gs, n, S, k, hv), gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        assert got == SW.temp_bytes64(n, S, k, hv) and got % 256 == 0 and q32 <= got <= 2 * q32, (n, S, k, hv)
        larger += got > q32
    assert larger > 50
    # the long-segment terms vanish when num_items <= CH; one element more brings one record, two task slots and 2 * k images
    for k in (1, 1023, 1024):
        assert _tb(gs, CH, 16, k, 1) == _tb(gs, CH, 16, k, 0) == 4096 + 5 * 256 + 256
        assert _tb(gs, CH + 1, 16, k, 0) == 4096 + 5 * 256 + 256 + 256 + ((8 * k * 2 + 255) & ~255) + 256
        assert _tb(gs, CH + 1, 16, k, 1) == _tb(gs, CH + 1, 16, k, 0) + ((4 * k * 2 + 255) & ~255)
    # the other two queries are what they were
    assert gs.lib.gs_topk_segmented_temp_bytes(CH + 1, 16, 1024, 0) == 4096 + 5 * 256 + 256 + 256 + 8192 + 256
    assert gs.lib.gs_topk_segmented_u16_temp_bytes(CH + 1, 16, 1024, 0) == 4096 + 5 * 256 + 256 + 256 + 4096 + 256


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(n, S, k, hv):
        return None if SR.refused(n, S, k) else _tb(gs, n, S, k, hv)

    def rising(values):
        values = [v for v in values if v is not None]
        assert all(a <= b for a, b in zip(values, values[1:])), values
    fine = list(range(8100, 8300, 3)) + list(range(16300, 16500, 3)) + list(range(3 * CH - 5, 3 * (CH + 1) + 5))
    for hv in (0, 1):
        for S in SS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for n in NS[1:]])
                rising([tb(n, S, k, hv) for n in fine])
        for n in NS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for S in SS[1:]])
            for S in SS[1:]:
                rising([tb(n, S, k, hv) for k in KS[1:]])
    assert tb(1 << 20, 100, 100, 1) > tb(1 << 20, 100, 100, 0)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
@pytest.mark.parametrize("n", [700, 5000, 200000])
def test_refusals_and_noops_without_a_device(gs, n):
    S, k = 50, 100
    need = _tb(gs, n, S, k, 1)
    assert need > 0
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, counts=counts, n=n, S=S, begin=begin, end=end, k=k)
    bad = [
        dict(k=1025),                                      # k > max k
        dict(n=1 << 31), dict(n=(1 << 31) + 5),            # int offsets
        dict(S=1 << 23, k=512), dict(S=(1 << 32) - 1, k=2),    # num_segments * k >= 2^32
        dict(kt=0), dict(kt=1), dict(kt=2),                # the 32-bit key types
        dict(kt=8), dict(kt=9), dict(kt=10), dict(kt=11),  # the 16-bit ones
        dict(kt=-1), dict(kt=6), dict(kt=7), dict(kt=12),  # and the others
        dict(vout=None),                                   # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None), dict(begin=None), dict(end=None),   # NULL keys or offsets
        dict(temp=None),                                   # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0),     # one byte short, nothing
        dict(kin=kin + 4), dict(kout=kout + 4), dict(kin=kin + 1), dict(kin=kin + 2), dict(kout=kout + 12), dict(kout=kout + 255),
        dict(vin=vin + 2), dict(vin=vin + 3), dict(vout=vout + 2), dict(vout=vout + 1),      # u32 arrays not aligned to 4
        dict(counts=counts + 2), dict(counts=counts + 1), dict(begin=begin + 2), dict(begin=begin + 1), dict(end=end + 2),
        dict(end=end + 3),
        # every pair of arrays sharing a byte, at 8 bytes per key and 4 per value, count and offset
        dict(kout=kin), dict(kout=kin + 8 * (n - 1)), dict(kin=kout + 8 * (S * k - 1)),          # keys_in / keys_out
        dict(vin=kin), dict(vin=kin + 8 * n - 4), dict(kin=vin + 4 * n - 8),                     # keys_in / vals_in
        dict(vout=kin), dict(vout=kin + 8 * n - 4), dict(kin=vout + 4 * S * k - 8),              # keys_in / vals_out
        dict(counts=kin), dict(counts=kin + 8 * n - 4), dict(kin=counts + 4 * S - 8),            # keys_in / counts
        dict(begin=kin + 8 * n - 4), dict(end=kin), dict(kin=begin + 4 * S - 8), dict(kin=end + 4 * S - 8),   # keys_in / offsets
        dict(kout=vin), dict(kout=vin + 4 * n - 8),     dict(vin=kout + 8 * S * k - 4),          # vals_in / keys_out
        dict(vout=vin), dict(vout=vin + 4 * (n - 1)), dict(vin=vout + 4 * (S * k - 1)),          # vals_in / vals_out
        dict(counts=vin + 4 * (n - 1)), dict(begin=vin), dict(end=vin + 4 * (n - 1)),            # vals_in / counts, offsets
        dict(vout=kout), dict(vout=kout + 8 * S * k - 4), dict(kout=vout + 4 * S * k - 8),       # keys_out / vals_out
        dict(counts=kout + 8 * S * k - 4), dict(kout=counts + 4 * S - 8),                        # keys_out / counts
        dict(begin=kout), dict(end=kout + 8 * S * k - 4), dict(kout=end + 4 * S - 8),            # keys_out / offsets
        dict(counts=vout + 4 * (S * k - 1)), dict(begin=vout), dict(end=vout + 4 * (S * k - 1)),     # vals_out / counts, offsets
        dict(counts=begin + 4 * (S - 1)), dict(counts=end), dict(begin=counts + 4 * (S - 1)),    # counts / offsets
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # the order of the checks, each pair with the earlier one in order and the later one broken too: were the later one checked
    # first the answer would be the same, so every step is shown by a NO-OP that the earlier refusal must come before, and by
    # a call that only the workspace refuses (an accepted call would launch: not tried on fake addresses)
    short = dict(temp_bytes=need - 1)
    assert _call(gs, **dict(ok, kout=kin + 8 * n, **short)) == INVALID       # adjacent arrays do not overlap: only the workspace
    assert _call(gs, **dict(ok, counts=None, **short)) == INVALID
    assert _call(gs, **dict(ok, end=begin + 4, **short)) == INVALID          # the offsets may share: S + 1 offsets in one array
    assert _call(gs, **dict(ok, vin=None, **short)) == INVALID
    need0 = _tb(gs, n, S, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed, and the query returns 0
    for kt in SW.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, 0, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin + 4, None, kout + 4, vout, counts, n, S, begin, end, 0, desc, kt) == 0   # before the alignment
    for hv in (0, 1):
        assert _tb(gs, 0, S, k, hv) == 0 and _tb(gs, n, 0, k, hv) == 0 and _tb(gs, n, S, 0, hv) == 0
        # refused shapes: the query returns 0
        assert _tb(gs, n, S, 1025, hv) == 0 and _tb(gs, 1 << 31, S, k, hv) == 0 and _tb(gs, n, 1 << 23, 512, hv) == 0
        assert _tb(gs, n, (1 << 32) - 1, 2, hv) == 0
    for kt in (0, 1, 2, 8, 9, 10, 11, 12):
        assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, 0, kt) == INVALID   # a bad key type before the no-op
        assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, 0, kt) == INVALID
    assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, 1025) == INVALID      # k > max k before the no-op
    assert _call(gs, None, 0, kin, vin, kout, None, None, n, S, None, None, 0) == INVALID           # values in without out, too
    # k may exceed num_items and every segment's length
    assert _tb(gs, 10, 3, 1024, 1) > 0
    assert _call(gs, **dict(ok, n=10, k=1024, temp_bytes=_tb(gs, 10, S, 1024, 1) - 1)) == INVALID


def test_the_two_offset_arrays_may_share_and_nothing_else(gs):
    """On fake addresses only refusals can be called.  The counts on either offset array are refused with a workspace of the
    right size; the accepted case, both offsets in one array, runs on the device (topk_segmented64() in the GPU file)."""
    n, S, k = 5000, 50, 100
    need = _tb(gs, n, S, k, 1)
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    assert _call(gs, temp, need, kin, vin, kout, vout, begin, n, S, begin, end, k) == INVALID       # counts on begin
    assert _call(gs, temp, need, kin, vin, kout, vout, end, n, S, begin, end, k) == INVALID         # counts on end
    assert _call(gs, temp, need - 1, kin, vin, kout, vout, counts, n, S, begin, begin, k) == INVALID    # only the workspace


def test_one_plan_and_one_status_for_three_widths(gs):
    """One plan function: the geometry is the 32-bit one.  The status of refused and no-op shapes needs no device."""
    for n, S, k in ((20000, 3, 50), (1000, 7, 1024), (5000, 2, 1), (1 << 24, 4000, 333), (0, 5, 5), (5, 5, 0)):
        assert gs.DeviceTopKSegmented64.Plan(n, S, k) == gs.DeviceTopKSegmented.Plan(n, S, k) == SR.plan(n, S, k)
    assert gs.DeviceTopKSegmented64.Plan(20000, 3, 50) == [7, 10, CH, 2, 4, 1024, 0, 0]
    assert gs.DeviceTopKSegmented64.MaxK() == 1024
    assert not hasattr(gs.lib, "gs_topk_segmented_u64_plan") and not hasattr(gs.lib, "gs_topk_segmented_u64_status")
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_segmented_status(BASE, 5000, 3, 1025, 1, out, None) == INVALID and list(out) == [0] * 8
    with pytest.raises(gs.GpuSortError):
        gs.DeviceTopKSegmented64.Plan(5000, 3, 1025)


# ------------------------------------------------------------------------------------------------ front ends --
def test_device_topk_segmented64_size_query(gs):
    n, S, k = 300000, 40, 200
    D = gs.DeviceTopKSegmented64
    for kt in (None,) + SW.KEY_TYPES:
        for fn in (D.MinKeys, D.MaxKeys):
            assert fn(None, 0, None, None, None, n, S, None, None, k, key_type=kt) == _tb(gs, n, S, k, 0) > 4096
        for fn in (D.MinPairs, D.MaxPairs):
            assert fn(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=kt) == _tb(gs, n, S, k, 1)
    assert D.MinKeys(None, 0, None, None, None, n, S, None, None, 2000) == 0     # refused: k > max k
    assert (gs.GS_KEY_U64, gs.GS_KEY_I64, gs.GS_KEY_F64) == SW.KEY_TYPES
    for kt in (gs.GS_KEY_U32, gs.GS_KEY_F32, gs.GS_KEY_BF16, gs.GS_KEY_U16):
        with pytest.raises(TypeError):
            D.MinKeys(None, 0, None, None, None, n, S, None, None, k, key_type=kt)


def test_other_widths_and_key_types_raise_type_error(gs):
    """Raised before any buffer check or call: host tensors serve."""
    import torch
    D = gs.DeviceTopKSegmented64
    temp = torch.zeros(1 << 16, dtype=torch.uint8)
    off = torch.tensor([0, 4, 10], dtype=torch.int32)
    for dtype in (torch.int16, torch.bfloat16, torch.int32, torch.float32, torch.int8):
        t = torch.zeros(10, dtype=dtype)
        with pytest.raises(TypeError):
            D.MinKeys(temp, temp.numel(), t, torch.zeros(4, dtype=dtype), None, 10, 2, off[:-1], off[1:], 2)
        with pytest.raises(TypeError):
            D.MaxPairs(temp, temp.numel(), t, torch.zeros(4, dtype=dtype), None, torch.zeros(4, dtype=torch.int32), None, 10, 2,
                       off[:-1], off[1:], 2, key_type=gs.GS_KEY_I64)
        with pytest.raises(TypeError):
            gs.topk_segmented64(t, off, 2)
    wide = torch.zeros(10, dtype=torch.int64)
    for kt in (gs.GS_KEY_U32, gs.GS_KEY_I32, gs.GS_KEY_F32, gs.GS_KEY_U16, gs.GS_KEY_BF16):
        with pytest.raises(TypeError):
            D.MinKeys(temp, temp.numel(), wide, torch.zeros(4, dtype=torch.int64), None, 10, 2, off[:-1], off[1:], 2, key_type=kt)
    # the 32- / 16-bit front ends keep refusing 8-byte tensors
    with pytest.raises(TypeError):
        gs.topk_segmented(wide, off, 2)
    with pytest.raises(TypeError):
        gs.topk_segmented(torch.zeros(10, dtype=torch.float64), off, 2, indices=True)
    with pytest.raises(TypeError):
        gs.DeviceTopKSegmented.MinKeys(temp, temp.numel(), wide, torch.zeros(4, dtype=torch.int64), None, 10, 2, off[:-1], off[1:], 2)


def test_topk_segmented64_argument_checks_on_host_tensors(gs):
    import torch
    off = torch.tensor([0, 4, 10], dtype=torch.int32)
    for dtype in (torch.int64, torch.float64, torch.uint64):
        t = torch.zeros(10, dtype=dtype)
        v = torch.zeros(10, dtype=torch.int32)
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, 2, values=v, indices=True)
        with pytest.raises(TypeError):
            gs.topk_segmented64(t.reshape(2, 5), off, 2)
        with pytest.raises(TypeError):
            gs.topk_segmented64(t, off.long(), 2)
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, 2, end_offsets=off[:2])
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, 2, values=t)                      # 8-byte values
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, 2, values=torch.zeros(9, dtype=torch.int32))
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, -1)
        with pytest.raises(ValueError):
            gs.topk_segmented64(t, off, gs.DeviceTopKSegmented64.MaxK() + 1)
        ko, vo, counts = gs.topk_segmented64(t, off, 0, indices=True)
        assert tuple(ko.shape) == (2, 0) and ko.dtype == dtype and tuple(vo.shape) == (2, 0) and vo.dtype == torch.int32
        assert tuple(counts.shape) == (2,) and counts.dtype == torch.int32
        ko, vo, counts = gs.topk_segmented64(t, off[:1], 3)
        assert tuple(ko.shape) == (0, 3) and ko.dtype == dtype and vo is None and tuple(counts.shape) == (0,)
    with pytest.raises(TypeError):
        gs.topk_segmented64(torch.zeros(10, dtype=torch.complex64), off, 2)     # 8 bytes, but no key category
