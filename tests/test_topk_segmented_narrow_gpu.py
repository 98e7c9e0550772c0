"""gs_topk_segmented_u16 on the device: every segment bit for bit against tests/topk_segmented_narrow_ref.py (keys, values or
positions, counts, and the sentinel in every slot that must stay unwritten), with the list counts of
gs_topk_segmented_status asserted against the ref in every case: lengths at every class edge in a layout whose segments
start at odd elements, the pad image as an ordinary key, special values, long segments and their streaming rounds with
ties everywhere, one class at a time, odd layouts, clamped offsets, dropped segments, guarded buffers at even addresses that
are no multiple of 4, workspace reuse, graph capture, the widening identity against gs_topk_segmented_u32, gs_topk_rows_u16 on
equal segments, the Python front end and the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_segmented_narrow_ref as SN
import topk_segmented_ref as SR
from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR = SN.NR
U16, I16, F16, BF16 = SN.KEY_TYPES
WIDE = SN.WIDE
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
CH = SR.CH
TAIL = 64            # sentinel elements behind the outputs and the counts
FILL, FILL16 = SN.FILL, SN.FILL16


# ------------------------------------------------------------------------------------------------------- inputs --
def values_for(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def dev16(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def host16(t):
    return t.cpu().numpy().view(np.uint16)


def rotate(i):
    return SN.KEY_TYPES[i % 4], bool((i // 4) % 2), MODES[(i // 2) % 3]


def status_of(gs, temp_ptr, n, S, k, hv):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_segmented_status(temp_ptr, n, S, k, hv, out, None) == 0
    return list(out)


class Case:
    """One flat array of 16-bit keys and one set of offsets on the device; .check(k, kt, desc, mode) runs the C entry point
    and compares outputs, counts, unwritten slots and the status words.  The stable orders of the reference are computed
    once per (key type, direction) and shared by every k and form."""

    def __init__(self, gs, cuda, keys, begin, end):
        self.gs, self.cuda = gs, cuda
        self.keys, self.vals = np.ascontiguousarray(keys, np.uint16), values_for(len(keys))
        self.begin, self.end = np.asarray(begin, np.int32), np.asarray(end, np.int32)
        self.n, self.S = self.keys.size, self.begin.size
        self.d_keys, self.d_vals = dev16(self.keys, cuda), dev(self.vals, cuda)
        self.d_begin, self.d_end = dev(self.begin, cuda), dev(self.end, cuda)
        self.cache = {}
        self.status = SR.status(self.begin, self.end, self.n)

    def expect(self, k, kt, desc, mode):
        c = self.cache.setdefault((kt, desc), {})
        return SN.seg_topk16(self.keys, self.begin, self.end, k, kt, desc, self.vals if mode == PAIRS else None, cache=c)

    def check(self, k, kt, desc, mode, counts=True):
        gs, n, S = self.gs, self.n, self.S
        hv = int(mode != KEYS)
        what = "n=%d S=%d k=%d %s kt=%d desc=%d" % (n, S, k, mode, kt, desc)
        nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        assert nb == SN.temp_bytes16(n, S, k, hv) > 0, what
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((S * k + TAIL,), -1, dtype=torch.int16, device=self.cuda)
        vo = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        co = torch.full((S + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_segmented_u16(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                          ko.data_ptr(), vo.data_ptr() if hv else None, co.data_ptr() if counts else None, n, S,
                                          self.d_begin.data_ptr(), self.d_end.data_ptr(), k, int(desc), kt, None)
        assert rc == 0, (rc, what)
        assert gs.DeviceTopKSegmented.Status(temp, n, S, k, hv) == self.status, what
        ek, ev, ec = self.expect(k, kt, desc, mode)
        gk, gv, gc = host16(ko), host(vo), host(co)
        bad = np.nonzero((gk[:S * k].reshape(S, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of segments", bad[:8], "lengths", (self.end - self.begin)[bad[:8]])
        assert (gk[S * k:] == FILL16).all(), what
        if hv:
            bad = np.nonzero((gv[:S * k].reshape(S, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of segments", bad[:8], "lengths", (self.end - self.begin)[bad[:8]])
            assert (gv[S * k:] == FILL).all(), what
        else:
            assert (gv == FILL).all(), what
        if counts:
            assert np.array_equal(gc[:S], ec) and (gc[S:] == FILL).all(), what
        else:
            assert (gc == FILL).all(), what


# ------------------------------------------------------------------------------------------ lengths at every edge --
@pytest.fixture(scope="module")
def edge_cases(gs, cuda):
    """One Case per key type on the edge layout: 0, 1, 2, 63 .. 2 * CH + 1 with three elements between the segments, the first
    at element 1, so that segments start at odd and at even elements.  Shared by the six k."""
    begin, end, n = SR.packed(SR.EDGE_LENGTHS, gap=3, first=1)
    assert sum(int(b) & 1 for b in begin) >= 6 and sum(1 - (int(b) & 1) for b in begin) >= 6
    return {kt: Case(gs, cuda, SN.flat_keys16(n, kt, seed=kt), begin, end) for kt in SN.KEY_TYPES}


@pytest.mark.parametrize("k", SR.EDGE_KS)
def test_lengths_at_every_edge_in_one_ragged_call(edge_cases, k):
    """Every key type, both directions and the three forms at every k."""
    for kt in SN.KEY_TYPES:
        c = edge_cases[kt]
        assert c.status == [4, 3, 3, 3, 3, 2, 5, 0]
        for desc in (False, True):
            for mode in MODES:
                c.check(k, kt, desc, mode)
    edge_cases[BF16].check(k, BF16, True, ARGS, counts=False)


# ------------------------------------------------------------------------------------- pads and special values --
PAD_LENGTHS = [1, 63, 65, 1025, CH + 1]          # a wave with one pad lane, the next class, a workgroup, two chunks


def special_sets(kt):
    if kt == F16:
        return [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7FFF, 0xFFFF, 0x7D55, 0xFD55, 0x3C00, 0xBC00]
    if kt == BF16:
        return [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF, 0x7FAA, 0xFFAA, 0x3F80, 0xBF80]
    if kt == I16:
        return [0x8000, 0xFFFF, 0x0000, 0x7FFF]          # -32768, -1, 0, 32767
    return [0x0000, 0x0001, 0xFFFE, 0xFFFF]


@pytest.mark.parametrize("kt", SN.KEY_TYPES)
def test_the_pad_image_is_an_ordinary_key(gs, cuda, kt):
    """Segments made of nothing but the key whose image is 0xffff -- the pad's -- in the direction at hand, and segments where
    it is one key in three: the positions of equal keys come out in input order, so a pad taken for a key would show as a
    position past the segment or as a missing one."""
    begin, end, n = SR.packed(PAD_LENGTHS, gap=3, first=1)
    rng = np.random.default_rng(40 + kt)
    for desc in (False, True):
        top = NR.preimage16([0xFFFF], kt, desc)[0]
        assert NR.image16(np.array([top], np.uint16), kt, desc)[0] == 0xFFFF
        only = np.full(n, top, np.uint16)
        mixed = np.where(rng.random(n) < 0.34, top, rng.integers(0, 1 << 16, n).astype(np.uint16)).astype(np.uint16)
        for keys in (only, mixed):
            c = Case(gs, cuda, keys, begin, end)
            assert c.status == [2, 1, 0, 0, 1, 1, 2, 0]
            for k in (1, 64, 1024):
                for mode in MODES:
                    c.check(k, kt, desc, mode)
        ev = Case(gs, cuda, only, begin, end).expect(64, kt, desc, ARGS)[1]
        assert list(ev[1, :63]) == list(range(63)) and ev[1, 63] == FILL


@pytest.mark.parametrize("kt", SN.KEY_TYPES)
def test_special_values(gs, cuda, kt):
    """Half / bfloat16 +-0, +-inf, NaNs of both signs with distinct payloads, I16 at -32768 / -1 / 0 / 32767: nine keys in
    ten are specials, so every segment is full of them and of ties."""
    begin, end, n = SR.packed(PAD_LENGTHS, gap=3, first=1)
    rng = np.random.default_rng(50 + kt)
    sp = np.array(special_sets(kt), np.uint16)
    keys = np.where(rng.random(n) < 0.9, sp[rng.integers(0, sp.size, n)], rng.integers(0, 1 << 16, n).astype(np.uint16)).astype(np.uint16)
    c = Case(gs, cuda, keys, begin, end)
    for desc in (False, True):
        for k in (1, 65, 1024):
            for mode in MODES:
                c.check(k, kt, desc, mode)
    if kt in (F16, BF16):      # the order stated at the enum, ascending: negative NaNs first, -0 before +0, positive NaNs last
        first = c.expect(1024, kt, False, KEYS)[0][4]
        img = NR.image16(first, kt)
        assert (np.diff(img.astype(np.int64)) >= 0).all() and (first[0] & 0x8000) and (first[0] & 0x7FFF) > (sp[2] & 0x7FFF)


# ------------------------------------------------------------------------------------------------ long segments --
@pytest.mark.parametrize("length,k,rounds", SR.LONG_SHAPES)
def test_long_segments_and_their_streaming_rounds(gs, cuda, length, k, rounds):
    """One long segment behind a short one, starting at an odd element: one, two and three streaming rounds.  Every 16-bit
    distribution repeats its values at these lengths, so the cut falls into ties."""
    assert SR.final_rounds(length, k) == rounds
    si = [s[0] for s in SR.LONG_SHAPES].index(length)
    begin, end, n = SR.packed([100, length], gap=1)
    assert begin[1] & 1
    for i in range(2):
        kt, desc, _ = rotate(2 * si + i)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=30 + si + i), begin, end)
        assert c.status == [0, 1, 0, 0, 0, 1, -(-length // CH), 0]
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_long_segment_all_keys_equal_gives_the_first_positions(gs, cuda):
    length, k = 8 * CH + 1, 1000
    for kt, desc in ((U16, False), (BF16, True)):
        c = Case(gs, cuda, np.full(length + 7, 0x3F80, np.uint16), [7], [7 + length])
        assert np.array_equal(c.expect(k, kt, desc, ARGS)[1][0], np.arange(k, dtype=np.uint32))
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_long_segment_tie_runs_across_chunk_and_round_boundaries_with_the_cut_inside(gs, cuda):
    """15 * CH + 1 keys: 990 smaller keys scattered over all chunks, and three runs of one equal key: across the boundary of
    chunks 0 and 1, across that of chunks 7 and 8 (where the final's first round ends and its second begins), and the
    segment's last three elements.  k = 1000 and 1010 cut the first run before and behind its chunk boundary, 1017 the
    second behind its round boundary, 1024 the third -- there the new candidate ties with carried ones and must lose.  The
    keys above the runs are 16-bit random: tied among themselves everywhere."""
    length = 15 * CH + 1
    rng = np.random.default_rng(5)
    keys = rng.integers(2000, 1 << 16, length).astype(np.uint16)
    runs = np.r_[CH - 10:CH + 11, 8 * CH - 5:8 * CH + 6, length - 3:length]
    keys[runs] = 1000
    free = np.setdiff1d(np.arange(length), runs)
    keys[rng.choice(free, 990, replace=False)] = np.arange(990, dtype=np.uint16)
    c = Case(gs, cuda, np.r_[np.uint16(7), keys], [1], [1 + length])        # the segment starts at an odd element
    assert SR.final_rounds(length, 1024) == 3
    for k, last in ((1000, CH - 1), (1010, CH + 9), (1017, 8 * CH), (1024, length - 2)):
        ev = c.expect(k, U16, False, ARGS)[1][0]
        assert list(ev[990:]) == list(runs[:k - 990]) and ev[-1] == last
        for mode in MODES:
            c.check(k, U16, False, mode)
    c = Case(gs, cuda, np.r_[np.uint16(7), ~keys], [1], [1 + length])
    c.check(1024, U16, True, ARGS)


@pytest.mark.parametrize("k", [1023, 1])
def test_nine_chunks_of_uniform_patterns_at_odd_k(gs, cuda, k):
    """One segment of 9 * CH + 1 uniform 16-bit patterns -- more elements than patterns, so every value repeats -- at odd k:
    chunk c's candidates start at element c * k of a 2-byte row, an odd offset for every odd c."""
    length = 9 * CH + 1
    assert length > 1 << 16 and k & 1
    keys = np.random.default_rng(77).integers(0, 1 << 16, length + 3).astype(np.uint16)
    c = Case(gs, cuda, keys, [3], [3 + length])
    assert c.status == [0, 0, 0, 0, 0, 1, 10, 0]
    for i, kt in enumerate(SN.KEY_TYPES):
        for mode in MODES:
            c.check(k, kt, bool(i & 1), mode)


# ------------------------------------------------------------------------------------------- one class at a time --
@pytest.mark.parametrize("count", [1, 4, 5, 1000])
def test_one_class_at_a_time(gs, cuda, count):
    """`count` segments of ONE class per call: the four wave classes, the workgroup class (short segments overlap freely:
    the input is only read) and the long class (packed: long segments must not overlap)."""
    ci = [1, 4, 5, 1000].index(count)
    i = np.arange(count)
    for q, length in enumerate(SR.CLASS_LENGTHS + [1100]):
        lens = length - (i % 7)
        n = 20001
        begin = ((i * 37) % (n - length)).astype(np.int32)
        kt, desc, mode = rotate(ci + q)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=50 + q), begin, begin + lens.astype(np.int32))
        assert c.status[q] == count and sum(c.status) == count
        c.check((8, 100, 300, 1024, 64)[q], kt, desc, mode)
    lens = CH + 1 + (i % 7)
    begin, end, n = SR.packed(list(lens), first=1)
    kt, desc, mode = rotate(ci + 5)
    c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=57, kinds=["uniform", "five", "topbyte"]), begin, end)
    assert c.status == [0, 0, 0, 0, 0, count, 2 * count, 0]
    c.check(17, kt, desc, mode)


def test_all_six_lists_in_one_call_in_shuffled_order(gs, cuda):
    rng = np.random.default_rng(8)
    lens = np.concatenate([rng.integers(1, 65, 300), rng.integers(65, 257, 200), rng.integers(257, 513, 150), rng.integers(513, 1025, 100),
                           rng.integers(1025, CH + 1, 20), rng.integers(CH + 1, 4 * CH, 6), np.zeros(10, np.int64)])
    begin, end, n = SR.packed(list(lens))
    order = rng.permutation(lens.size)
    begin, end = begin[order], end[order]
    for i, k in enumerate((5, 71, 1024)):
        kt, desc, _ = rotate(i + 1)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=60 + i), begin, end)
        assert c.status[:6] == [300, 200, 150, 100, 20, 6] and c.status[7] == 0
        for mode in MODES:
            c.check(k, kt, desc, mode)


# --------------------------------------------------------------------------------------------- segment layout --
def test_gaps_reverse_order_and_a_repeated_segment(gs, cuda):
    lens = [5, 300, 0, 1024, 2000, CH + 9, 64, 700]
    begin, end, n = SR.packed(lens, gap=11, first=3)
    begin, end = begin[::-1].copy(), end[::-1].copy()                   # the segments in reverse order
    begin, end = np.r_[begin, begin[[0, 3, 6]]], np.r_[end, end[[0, 3, 6]]]     # 700, 2000 and 300 once more
    for i, k in enumerate((3, 129, 1000)):
        kt, desc, _ = rotate(i)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=70 + i), begin.astype(np.int32), end.astype(np.int32))
        assert c.status[5] == 1
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_sliding_windows_of_100_with_step_1(gs, cuda):
    n = 5000
    begin = np.arange(0, n - 100 + 1, dtype=np.int32)
    for i, k in enumerate((1, 10, 100)):
        kt, desc, mode = rotate(i + 2)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=80 + i, kinds=["uniform", "five", "sorted", "zipf"]), begin, begin + 100)
        assert c.status == [0, begin.size, 0, 0, 0, 0, 0, 0]
        c.check(k, kt, desc, mode)


def test_device_offsets_that_need_clamping(gs, cuda):
    """Offsets below 0 and above num_items, and end < begin: clamped on the device, positions counted from the clamped begin.
    Every array sits between guard zones, the keys at an even address that is no multiple of 4."""
    n, k = 3 * CH, 50
    big = (1 << 31) - 1
    begin = np.array([-5, -(1 << 31), n - 10, n - 5000, 500, n, n + 5, -100, -(1 << 31), -7], np.int32)
    end = np.array([40, 3, n + 1000, big, 100, n + 9, n + 2, -3, 2000, n + 7], np.int32)
    _, ln = SR.clamp(begin, end, n)
    assert list(ln) == [40, 3, 10, 5000, 0, 0, 0, 0, 2000, n]
    S = begin.size
    want = SR.status(begin, end, n)
    assert want == [3, 0, 0, 0, 2, 1, 3, 0]
    for i, mode in enumerate(MODES):
        kt, desc = (F16, U16, I16)[i], bool(i % 2)
        keys, vals = SN.flat_keys16(n, kt, seed=90 + i), values_for(n, seed=4)
        hv = int(mode != KEYS)
        ek, ev, ec = SN.seg_topk16(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=1)
        a.add("keys_in", 2 * n, offset=2, data=keys, const=True).add("vals_in", 4 * n, data=vals, const=True)
        a.add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, offset=8, data=end, const=True)
        a.add("keys_out", 2 * S * k, offset=6, fill="ff").add("vals_out", 4 * S * k, fill="ff")
        a.add("counts", 4 * S, fill="ff").add("temp", nb, offset=3, fill="random").build()
        assert gs.lib.gs_topk_segmented_u16(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                            a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, int(desc),
                                            kt, None) == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == want
        assert np.array_equal(a.read("counts", np.uint32), ec)
        assert np.array_equal(a.read("keys_out", np.uint16).reshape(S, k), ek), mode
        assert np.array_equal(a.read("vals_out", np.uint32).reshape(S, k), ev if hv else np.full((S, k), FILL, np.uint32)), mode


# ------------------------------------------------------------------------------------------- dropped segments --
def test_dropped_segments(gs, cuda):
    """Three copies of one segment of num_items = 4 * CH elements at k = 1024.  Lmax = 3 records would hold them, but each needs
    four of the Tmax = 7 chunk-task slots: exactly one completes, whichever it is, and is correct; the others are dropped:
    count 0, slots unwritten, out[7] = 2.  No guard byte anywhere is changed."""
    n, S, k = 4 * CH, 3, 1024
    lmax, tmax = SR.geometry(n, S)
    fit = min(lmax, tmax // 4)
    assert (lmax, tmax, fit) == (3, 7, 1)
    keys = SN.flat_keys16(n, I16, seed=95)
    begin, end = np.zeros(S, np.int32), np.full(S, n, np.int32)
    ek, ev, ec = SN.seg_topk16(keys, begin[:1], end[:1], k, I16, False)
    for mode in (ARGS, KEYS):
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=2)
        a.add("keys_in", 2 * n, offset=2, data=keys, const=True).add("begin", 4 * S, data=begin, const=True)
        a.add("end", 4 * S, data=end, const=True)
        a.add("keys_out", 2 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff").add("counts", 4 * S, fill="ff")
        a.add("temp", nb, offset=1, fill="random").build()
        assert gs.lib.gs_topk_segmented_u16(a.ptr("temp"), nb, a.ptr("keys_in"), None, a.ptr("keys_out"), a.ptr("vals_out") if hv else None,
                                            a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, 0, I16, None) == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == [0, 0, 0, 0, 0, fit, 4 * fit, S - fit]
        gk, gv = a.read("keys_out", np.uint16).reshape(S, k), a.read("vals_out", np.uint32).reshape(S, k)
        gc = a.read("counts", np.uint32)
        assert sorted(gc) == [0] * (S - fit) + [k] * fit
        for s in range(S):
            if gc[s]:
                assert np.array_equal(gk[s], ek[0]) and (not hv or np.array_equal(gv[s], ev[0]))
            else:
                assert (gk[s] == FILL16).all()
            assert hv or (gv[s] == FILL).all()
            assert gc[s] or (gv[s] == FILL).all()


def test_dropped_segments_without_a_record_slot(gs, cuda):
    """Five copies of one segment of CH + 1 elements in num_items = 2 * CH + 2: Lmax = 2 and Tmax = 4, two chunk tasks a copy.
    The claims of one classify workgroup are taken in one order, so exactly two copies complete, whichever they are; three find
    no record slot and are dropped: count 0, slots unwritten, out[7] = 3.  No guard byte is changed."""
    n, S, k = 2 * CH + 2, 5, 100
    assert SR.geometry(n, S) == (2, 4)
    keys = SN.flat_keys16(n, U16, seed=96)
    begin, end = np.full(S, 1, np.int32), np.full(S, CH + 2, np.int32)
    ek, ev, _ = SN.seg_topk16(keys, begin[:1], end[:1], k, U16, True)
    nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, 1)
    a = Arena(cuda, seed=3)
    a.add("keys_in", 2 * n, data=keys, const=True).add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, data=end, const=True)
    a.add("keys_out", 2 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff").add("counts", 4 * S, fill="ff")
    a.add("temp", nb, offset=5, fill="random").build()
    assert gs.lib.gs_topk_segmented_u16(a.ptr("temp"), nb, a.ptr("keys_in"), None, a.ptr("keys_out"), a.ptr("vals_out"), a.ptr("counts"), n, S,
                                        a.ptr("begin"), a.ptr("end"), k, 1, U16, None) == 0
    a.check()
    assert status_of(gs, a.ptr("temp"), n, S, k, 1) == [0, 0, 0, 0, 0, 2, 4, 3]
    gk, gv = a.read("keys_out", np.uint16).reshape(S, k), a.read("vals_out", np.uint32).reshape(S, k)
    gc = a.read("counts", np.uint32)
    assert sorted(gc) == [0, 0, 0, k, k]
    for s in range(S):
        if gc[s]:
            assert np.array_equal(gk[s], ek[0]) and np.array_equal(gv[s], ev[0])
        else:
            assert (gk[s] == FILL16).all() and (gv[s] == FILL).all()


# ----------------------------------------------------------------------------------------- buffers and reuse --
GUARDED = [([5, 300, 0, 64, 1000], 7), ([4000, 70, 1025], 101), ([CH + 5, 2, 3 * CH + 1, 600], 1023)]


@pytest.mark.parametrize("lens,k", GUARDED)
def test_guarded_offset_dirty_buffers(gs, cuda, lens, k):
    """Every array in a slot of its own between guard zones: the key arrays at even byte offsets that are no multiple of 4
    (2, 6, 10, 14 past a 256-byte boundary), the u32 arrays at multiples of 4, the workspace at an odd one; outputs, counts
    and workspace dirty; the slots past a segment's count keep their bytes.  An odd k puts every second output row at such
    an address as well."""
    begin, end, n = SR.packed(lens, gap=1)
    S = len(lens)
    for i, mode in enumerate(MODES):
        kt, desc = (BF16, I16, F16)[i], bool(i % 2)
        keys, vals = SN.flat_keys16(n, kt, seed=100 + i), values_for(n, seed=9)
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=i)
        a.add("keys_in", 2 * n, offset=(2, 6, 10)[i], data=keys, const=True)
        a.add("vals_in", 4 * n, offset=12, data=vals, const=True)
        a.add("begin", 4 * S, offset=16, data=begin, const=True)
        a.add("end", 4 * S, offset=28, data=end, const=True)
        a.add("keys_out", 2 * S * k, offset=(14, 2, 6)[i], fill="random")
        a.add("vals_out", 4 * S * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("counts", 4 * S, offset=36, fill="random")
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        assert a.ptr("keys_in") % 4 == 2 and a.ptr("keys_out") % 4 == 2 and a.ptr("temp") % 2 == 1
        rc = gs.lib.gs_topk_segmented_u16(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                          a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, int(desc),
                                          kt, None)
        assert rc == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == SR.status(begin, end, n)
        ek, ev, ec = SN.seg_topk16(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("counts", np.uint32), ec)
        written = (np.arange(k)[None, :] < ec[:, None])
        gk, ik = a.read("keys_out", np.uint16).reshape(S, k), a.init["keys_out"].view(np.uint16).reshape(S, k)
        assert np.array_equal(gk, np.where(written, ek, ik)), (mode, lens, k)
        gv, iv = a.read("vals_out", np.uint32).reshape(S, k), a.init["vals_out"].view(np.uint32).reshape(S, k)
        assert np.array_equal(gv, np.where(written, ev, iv) if hv else iv), (mode, lens, k)


def test_refused_calls_write_nothing(gs, cuda):
    n, S, k = 9000, 3, 10
    nb = gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 2 * n, fill="random").add("keys_out", 2 * S * k, fill="random").add("vals_out", 4 * S * k, fill="random")
    a.add("counts", 4 * S, fill="random").add("begin", 4 * S, data=np.array([0, 100, 200], np.int32))
    a.add("end", 4 * S, data=np.array([100, 200, 9000], np.int32)).add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), counts=a.ptr("counts"),
                 n=n, S=S, begin=a.ptr("begin"), end=a.ptr("end"), k=k, kt=U16)
        p.update(kw)
        return gs.lib.gs_topk_segmented_u16(p["temp"], p["nb"], p["kin"], None, p["kout"], p["vout"], p["counts"], p["n"], p["S"], p["begin"],
                                            p["end"], p["k"], 0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=1025), dict(n=1 << 31), dict(kt=0), dict(kt=2), dict(kt=12), dict(begin=None),
               dict(end=None), dict(kout=a.ptr("keys_in") + 2), dict(vout=a.ptr("keys_out") + 2 * S * k - 4), dict(kin=a.ptr("keys_in") + 1),
               dict(kout=a.ptr("keys_out") + 1), dict(vout=a.ptr("vals_out") + 2), dict(counts=a.ptr("begin")),
               dict(counts=a.ptr("keys_out"))):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A ragged pairs call with long segments, a keys call on other offsets and the first one again, on one stream and one
    workspace without a synchronisation between them: the third call's bytes equal the first's."""
    lens_a, ka = [2 * CH + 9, 300, 5000, 9 * CH + 3, 40], 301
    begin_a, end_a, na = SR.packed(lens_a, first=1)
    a = Case(gs, cuda, SN.flat_keys16(na, BF16, seed=110), begin_a, end_a)
    begin_b, end_b, nb_items = SR.packed([5000, 77, CH + 1, 1])
    b = Case(gs, cuda, SN.flat_keys16(nb_items, I16, seed=111), begin_b, end_b)
    nb = max(gs.lib.gs_topk_segmented_u16_temp_bytes(na, a.S, ka, 1), gs.lib.gs_topk_segmented_u16_temp_bytes(nb_items, b.S, 77, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((a.S * ka,), -1, dtype=torch.int16, device=cuda), torch.full((a.S * ka,), -1, dtype=torch.int32, device=cuda),
             torch.full((a.S,), -1, dtype=torch.int32, device=cuda)) for _ in range(2)]
    kb = torch.full((b.S * 77,), -1, dtype=torch.int16, device=cuda)

    def run_a(ko, vo, co):
        assert gs.lib.gs_topk_segmented_u16(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(),
                                            co.data_ptr(), na, a.S, a.d_begin.data_ptr(), a.d_end.data_ptr(), ka, 1, BF16, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_segmented_u16(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, None, nb_items, b.S,
                                        b.d_begin.data_ptr(), b.d_end.data_ptr(), 77, 0, I16, None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    assert gs.DeviceTopKSegmented.Status(temp, na, a.S, ka, 1) == a.status
    ek, ev, ec = a.expect(ka, BF16, True, PAIRS)
    assert np.array_equal(host16(outs[0][0]).reshape(a.S, ka), ek) and np.array_equal(host(outs[0][1]).reshape(a.S, ka), ev)
    assert np.array_equal(host(outs[0][2]), ec)
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert np.array_equal(host16(kb).reshape(b.S, 77), b.expect(77, I16, False, KEYS)[0])


def test_topk_segmented_u16_is_capturable_in_a_hip_graph(gs, cuda):
    """Captured once on one plain side stream (no parallel branches), all ten launches, replayed on new data in the same
    buffers; the status is read after every replay."""
    lens, k = [8 * CH + 1, 500, 2 * CH, 3000, 9], 1023
    begin, end, n = SR.packed(lens, gap=1, first=1)
    S = len(lens)
    sets = [SN.flat_keys16(n, BF16, seed=120 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "special"))]
    src, d_begin, d_end = dev16(sets[0], cuda), dev(begin, cuda), dev(end, cuda)
    ko = torch.full((S * k,), -1, dtype=torch.int16, device=cuda)
    vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
    co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
    D = gs.DeviceTopKSegmented
    nb = D.MaxPairs(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=gs.GS_KEY_BF16)
    assert nb == SN.temp_bytes16(n, S, k, 1) and D.Plan(n, S, k, True) == SR.plan(n, S, k) and D.Plan(n, S, k, True)[1] == 10
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_BF16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_BF16)
    for keys in sets[1:] + sets[:1]:
        src.copy_(dev16(keys, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        co.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev, ec = SN.seg_topk16(keys, begin, end, k, BF16, True)
        assert np.array_equal(host16(ko).reshape(S, k), ek) and np.array_equal(host(vo).reshape(S, k), ev)
        assert np.array_equal(host(co), ec)
        assert D.Status(temp, n, S, k, True, stream=side) == SR.status(begin, end, n)     # the state block is zeroed in every replay


# ------------------------------------------------------------------------------------------- widening identity --
LIST_SHAPES = [([40, 1, 64], 8), ([200, 65, 256], 100), ([400, 257, 512], 300), ([900, 513, 1024], 1024), ([3000, 1025, CH], 65),
               ([CH + 5, 2 * CH + 1], 1023)]


@pytest.mark.parametrize("lens,k", LIST_SHAPES)
def test_equals_the_32_bit_entry_point_on_the_widened_keys(gs, cuda, lens, k):
    """gs_topk_segmented_u32 on (uint32_t)key << 16 with the key type widened, its keys shifted right by 16: one shape per
    list, every key type, the directions and forms in turn; compared on the device's own outputs."""
    q = [s[0] for s in LIST_SHAPES].index(lens)
    begin, end, n = SR.packed(lens, gap=1, first=1)
    S = len(lens)
    assert SR.status(begin, end, n)[q] == S
    for i, kt in enumerate(SN.KEY_TYPES):
        desc, mode = bool((i + q) & 1), MODES[(i + q) % 3]
        hv = int(mode != KEYS)
        c = Case(gs, cuda, SN.flat_keys16(n, kt, seed=140 + q, kinds=["uniform", "special", "five", "topbyte"]), begin, end)
        c.check(k, kt, desc, mode)
        wide = dev(NR.widen(c.keys), cuda)
        nb = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        assert nb >= gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_segmented_u32(temp.data_ptr(), nb, wide.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                                            vo.data_ptr() if hv else None, co.data_ptr(), n, S, c.d_begin.data_ptr(), c.d_end.data_ptr(), k,
                                            int(desc), WIDE[kt], None) == 0
        ek, ev, ec = c.expect(k, kt, desc, mode)
        assert np.array_equal((host(ko) >> 16).astype(np.uint16).reshape(S, k), ek)
        assert (not hv or np.array_equal(host(vo).reshape(S, k), ev)) and np.array_equal(host(co), ec)


@pytest.mark.parametrize("rows,cols,k", [(37, 301, 21), (5, 3001, 100), (3, 2 * CH + 9, 301)])
def test_regular_offsets_equal_topk_rows_u16(gs, cuda, rows, cols, k):
    """gs_topk_segmented_u16 on regular offsets against gs_topk_rows_u16 on the same matrix, one shape per path of the rows
    entry point (odd columns: every second row starts at an odd element), all forms."""
    begin = (np.arange(rows) * cols).astype(np.int32)
    for i, mode in enumerate(MODES):
        kt, desc = (BF16, U16, F16)[i], bool((i + 1) % 2)
        c = Case(gs, cuda, SN.flat_keys16(rows * cols, kt, seed=130 + i), begin, begin + cols)
        hv = int(mode != KEYS)
        nb = max(gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv), 256)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((rows * k,), -1, dtype=torch.int16, device=cuda)
        vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_rows_u16(temp.data_ptr(), nb, c.d_keys.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                                       vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None) == 0
        ek, ev, _ = c.expect(k, kt, desc, mode)
        assert np.array_equal(host16(ko).reshape(rows, k), ek) and (not hv or np.array_equal(host(vo).reshape(rows, k), ev))
        c.check(k, kt, desc, mode)


# ------------------------------------------------------------------------------------------------- front ends --
def _tie_free(dtype, lens, rng):
    """Per segment, distinct bit patterns of the dtype: for the float types finite and non-zero (no NaN, no signed zero)."""
    if dtype == torch.int16:
        pool = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    else:
        inf = 0x7C00 if dtype == torch.float16 else 0x7F80
        mag = np.arange(1, inf, dtype=np.uint32)
        pool = np.concatenate([mag, mag | 0x8000]).astype(np.uint16)
    return np.concatenate([rng.choice(pool, ln, replace=False) for ln in lens] + [np.empty(0, np.uint16)])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.int16])
def test_topk_segmented_against_torch_topk(gs, cuda, dtype):
    rng = np.random.default_rng(17)
    lens = [0, 1, 5, 100, 1000, 3001, CH + 50, 20000, 64]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(offsets[-1])
    x = dev16(_tie_free(dtype, lens, rng), cuda).view(dtype)
    off = torch.from_numpy(offsets).to(cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) * 3
    for k in (1, 51, 1024):
        for largest in (False, True):
            ko, io, counts = gs.topk_segmented(x, off, k, largest=largest, indices=True)
            k2, none, c2 = gs.topk_segmented(x, off[:-1].contiguous(), k, largest=largest, end_offsets=off[1:].contiguous())
            k3, v3, _ = gs.topk_segmented(x, off, k, largest=largest, values=vals)
            assert tuple(ko.shape) == (len(lens), k) and ko.dtype == dtype and io.dtype == torch.int32 and counts.dtype == torch.int32
            assert none is None and torch.equal(counts, c2)
            assert counts.tolist() == [min(k, ln) for ln in lens]
            for s, ln in enumerate(lens):
                kept = min(k, ln)
                if kept == 0:
                    continue
                seg = x[offsets[s]:offsets[s + 1]]
                want = torch.topk(seg, kept, largest=largest, sorted=True)
                assert torch.equal(ko[s, :kept], want.values) and torch.equal(io[s, :kept].long(), want.indices), (s, k, largest)
                assert torch.equal(k2[s, :kept], want.values) and torch.equal(k3[s, :kept], want.values)
                assert torch.equal(v3[s, :kept].long(), (want.indices + int(offsets[s])) * 3)
    with pytest.raises(ValueError):
        gs.topk_segmented(x, off, 1025)


def test_device_topk_segmented_with_an_explicit_key_type_on_an_int16_tensor(gs, cuda):
    """key_type=GS_KEY_U16 on an int16 tensor orders the bit patterns as unsigned; without it the tensor's own type (I16)
    holds; a 32-bit key type on it raises TypeError."""
    lens, k = [70, 2000, CH + 3, 5], 33
    begin, end, n = SR.packed(lens, gap=2, first=1)
    S = len(lens)
    keys = SN.flat_keys16(n, U16, seed=150, kinds=["uniform"])
    src, d_begin, d_end = dev16(keys, cuda), dev(begin, cuda), dev(end, cuda)
    D = gs.DeviceTopKSegmented
    for key_type, kt in ((gs.GS_KEY_U16, U16), (None, I16)):
        ko = torch.full((S * k,), -1, dtype=torch.int16, device=cuda)
        vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
        nb = D.MinPairs(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=gs.GS_KEY_U16)
        assert nb == SN.temp_bytes16(n, S, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        assert D.MinPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=key_type) == nb
        assert D.Status(temp, n, S, k, True) == SR.status(begin, end, n)
        ek, ev, ec = SN.seg_topk16(keys, begin, end, k, kt, False)
        assert np.array_equal(host16(ko).reshape(S, k), ek) and np.array_equal(host(vo).reshape(S, k), ev) and np.array_equal(host(co), ec)
    assert not np.array_equal(SN.seg_topk16(keys, begin, end, k, U16)[0], SN.seg_topk16(keys, begin, end, k, I16)[0])
    with pytest.raises(TypeError):
        D.MinPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_U32)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_segmented_narrow_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 4 * 3 * 2 * 3
