"""gs_topk_segmented_u64 on the device: every segment bit for bit against tests/topk_segmented_wide_ref.py (keys, values or
positions, counts, and the sentinel in every slot that must stay unwritten), with the list counts of
gs_topk_segmented_status asserted against the ref in every case: lengths at every class edge, the byte skip of the 64-bit wave
sort and select at its edges in every kernel class, long segments and their streaming rounds (a carried element that alone
varies a byte, the mirror case, chunks with different constant bytes, ties everywhere), the pad image as an ordinary key,
special values, one class at a time, odd layouts, clamped offsets, dropped segments, guarded buffers, refused calls, workspace
reuse, graph capture, the widening identity against gs_topk_segmented_u32, gs_topk_rows_u64 on equal segments, gs_topk_u64 on
single segments, the Python front ends and the C++ driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_ref as R
import topk_rows_wide_ref as WR
import topk_segmented_ref as SR
import topk_segmented_wide_ref as SW
from guarded import Arena
from test_topk_segmented_narrow_gpu import GUARDED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = SW.W
U64, I64, F64 = SW.KEY_TYPES
KEYS, PAIRS, ARGS = SW.KEYS, SW.PAIRS, SW.ARGS
MODES = SW.MODES
CH = SR.CH
TAIL = 64            # sentinel elements behind the outputs and the counts
FILL, FILL64 = SW.FILL, SW.FILL64


# ------------------------------------------------------------------------------------------------------- inputs --
def values_for(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def dev64(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def rotate(i):
    return SW.KEY_TYPES[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def status_of(gs, temp_ptr, n, S, k, hv):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_segmented_status(temp_ptr, n, S, k, hv, out, None) == 0
    return list(out)


class Case:
    """One flat array of 64-bit keys and one set of offsets on the device; .check(k, kt, desc, mode) runs the C entry point
    and compares outputs, counts, unwritten slots and the status words.  The stable orders of the reference are computed
    once per (key type, direction) and shared by every k and form."""

    def __init__(self, gs, cuda, keys, begin, end):
        self.gs, self.cuda = gs, cuda
        self.keys, self.vals = np.ascontiguousarray(keys, np.uint64), values_for(len(keys))
        self.begin, self.end = np.asarray(begin, np.int32), np.asarray(end, np.int32)
        self.n, self.S = self.keys.size, self.begin.size
        self.d_keys, self.d_vals = dev64(self.keys, cuda), dev(self.vals, cuda)
        self.d_begin, self.d_end = dev(self.begin, cuda), dev(self.end, cuda)
        self.cache = {}
        self.status = SR.status(self.begin, self.end, self.n)

    def expect(self, k, kt, desc, mode):
        c = self.cache.setdefault((kt, desc), {})
        return SW.seg_topk64(self.keys, self.begin, self.end, k, kt, desc, self.vals if mode == PAIRS else None, cache=c)

    def run(self, k, kt, desc, mode, counts=True):
        gs, n, S = self.gs, self.n, self.S
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)
        assert nb == SW.temp_bytes64(n, S, k, hv) > 0
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((S * k + TAIL,), -1, dtype=torch.int64, device=self.cuda)
        vo = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        co = torch.full((S + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = gs.lib.gs_topk_segmented_u64(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                          ko.data_ptr(), vo.data_ptr() if hv else None, co.data_ptr() if counts else None, n, S,
                                          self.d_begin.data_ptr(), self.d_end.data_ptr(), k, int(desc), kt, None)
        assert rc == 0, rc
        return temp, ko, vo, co

    def check(self, k, kt, desc, mode, counts=True):
        n, S = self.n, self.S
        hv = int(mode != KEYS)
        what = "n=%d S=%d k=%d %s kt=%d desc=%d" % (n, S, k, mode, kt, desc)
        temp, ko, vo, co = self.run(k, kt, desc, mode, counts)
        assert self.gs.DeviceTopKSegmented64.Status(temp, n, S, k, hv) == self.status, what
        ek, ev, ec = self.expect(k, kt, desc, mode)
        gk, gv, gc = host64(ko), host(vo), host(co)
        bad = np.nonzero((gk[:S * k].reshape(S, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of segments", bad[:8], "lengths", (self.end - self.begin)[bad[:8]])
        assert (gk[S * k:] == FILL64).all(), what
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


# --------------------------------------------------------------------------------------- 1. lengths at every edge --
@pytest.fixture(scope="module")
def edge_cases(gs, cuda):
    """One Case per key type on the edge layout: 0, 1, 2, 63 .. 2 * CH + 1 with three elements between the segments, the first
    at element 1.  Shared by the six k."""
    begin, end, n = SR.packed(SR.EDGE_LENGTHS, gap=3, first=1)
    return {kt: Case(gs, cuda, SW.flat_keys64(n, kt, seed=kt), begin, end) for kt in SW.KEY_TYPES}


@pytest.mark.parametrize("k", SR.EDGE_KS)
def test_lengths_at_every_edge_in_one_ragged_call(edge_cases, k):
    """The three forms at every k; the key types and the directions rotate over the cases."""
    ki = SR.EDGE_KS.index(k)
    for j, mode in enumerate(MODES):
        kt, desc = SW.KEY_TYPES[(ki + j) % 3], bool((ki + j // 2) % 2)
        c = edge_cases[kt]
        assert c.status == [4, 3, 3, 3, 3, 2, 5, 0]
        c.check(k, kt, desc, mode)
        c.check(k, kt, not desc, mode)
    edge_cases[F64].check(k, F64, True, ARGS, counts=False)


# ---------------------------------------------------------------------------------------------- 2. the byte skip --
SKIP_LENGTHS = [40, 900, 3000, 2 * CH + 9]        # two wave classes, the workgroup, a long segment (three chunks, one round)


def _skip_case(gs, cuda, make, kt, desc):
    """make(length, index) -> the images of one segment; the key patterns are their preimages under (kt, desc)."""
    begin, end, n = SR.packed(SKIP_LENGTHS, gap=1, first=1)
    img = np.full(n, WR.BASE ^ np.uint64(0x5555), np.uint64)
    for i, (b, ln) in enumerate(zip(begin, SKIP_LENGTHS)):
        img[b:b + ln] = make(ln, i)
    c = Case(gs, cuda, SW.preimage(img, kt, desc), begin, end)
    assert c.status == [1, 0, 0, 1, 1, 1, 3, 0]
    return c


@pytest.mark.parametrize("b", range(8))
def test_exactly_one_varying_byte(gs, cuda, b):
    kt, desc, _ = rotate(b)
    c = _skip_case(gs, cuda, lambda ln, i: WR.one_byte_rows(1, ln, b, seed=10 * b + i)[0], kt, desc)
    for k, mode in ((1, KEYS), (33, PAIRS), (1024, ARGS)):
        c.check(k, kt, desc, mode)


def test_segments_of_one_key(gs, cuda):
    """No pass of the wave sort and no round of the select runs: the first positions come out."""
    for i in range(3):
        kt, desc, _ = rotate(i + 1)
        c = _skip_case(gs, cuda, lambda ln, j: WR.one_key_rows(1, ln, WR.BASE + np.uint64(j))[0], kt, desc)
        ev = c.expect(100, kt, desc, ARGS)[1]
        assert list(ev[0, :40]) == list(range(40)) and all(list(ev[s]) == list(range(100)) for s in (1, 2, 3))
        for k, mode in ((1, KEYS), (100, ARGS), (1024, PAIRS)):
            c.check(k, kt, desc, mode)


@pytest.mark.parametrize("where", ["first", "last", "last_register"])
def test_one_outlier_makes_a_byte_vary(gs, cuda, where):
    """Byte 0 varies everywhere; ONE element per segment differs in another byte too: the first element, the last, or the
    first of the last, partly filled register (element 64 * ((len - 1) // 64))."""
    wi = ["first", "last", "last_register"].index(where)
    at = {"first": lambda ln: 0, "last": lambda ln: ln - 1, "last_register": lambda ln: 64 * ((ln - 1) // 64)}[where]
    for b in (7, 4, 1):
        kt, desc, _ = rotate(b + wi)
        c = _skip_case(gs, cuda, lambda ln, i: WR.outlier_rows(1, ln, b, at(ln), seed=20 + b + i)[0], kt, desc)
        for k, mode in ((1, ARGS), (65, KEYS), (1000, PAIRS)):
            c.check(k, kt, desc, mode)


# ------------------------------------------------------------------------------------------ 3. streaming final --
@pytest.mark.parametrize("length,k,rounds", SR.LONG_SHAPES)
def test_long_segments_and_their_streaming_rounds(gs, cuda, length, k, rounds):
    assert SR.final_rounds(length, k) == rounds
    si = [s[0] for s in SR.LONG_SHAPES].index(length)
    begin, end, n = SR.packed([100, length], gap=1)
    for i in range(2):
        kt, desc, _ = rotate(2 * si + i)
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=30 + si + i), begin, end)
        assert c.status == [0, 1, 0, 0, 0, 1, -(-length // CH), 0]
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_a_carried_element_alone_varies_a_byte_in_the_later_rounds(gs, cuda):
    """Three streaming rounds at k = 1024.  From round two on the new candidates are ONE image and the carried best k are one
    other image but for a single element that differs from them in byte b alone: the round of byte b must still run, or the
    outlier loses its first place."""
    k = 1024
    for b in range(8):
        kt, desc, mode = rotate(b)
        img, at = SW.carried_outlier_segment(k, b, seed=b)
        assert SR.final_rounds(img.size, k) == 3
        c = Case(gs, cuda, SW.preimage(img, kt, desc), [0], [img.size])
        ev = c.expect(k, kt, desc, ARGS)[1][0]
        assert ev[0] == at and sorted(ev) == list(range(k))
        c.check(k, kt, desc, mode)
    c.check(k, kt, desc, ARGS)


def test_the_outlier_is_a_new_candidate_of_the_last_round(gs, cuda):
    """The mirror: the carried elements are all equal (no round runs while that lasts) and the one smaller image arrives
    with the last round's candidates."""
    k = 1024
    for b in (0, 3, 7):
        kt, desc, mode = rotate(b + 1)
        img, at = SW.late_outlier_segment(k, b)
        c = Case(gs, cuda, SW.preimage(img, kt, desc), [0], [img.size])
        ev = c.expect(k, kt, desc, ARGS)[1][0]
        assert ev[0] == at and list(ev[1:]) == list(range(k - 1))
        c.check(k, kt, desc, mode)
        c.check(k, kt, desc, ARGS)


def test_chunks_with_different_constant_bytes(gs, cuda):
    length = 15 * CH + 1
    img = WR.chunked_constant_row(length, seed=4)
    for i, k in enumerate((1024, 300, 1)):
        kt, desc, _ = rotate(i)
        c = Case(gs, cuda, np.r_[np.uint64(7), SW.preimage(img, kt, desc)], [1], [1 + length])
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_long_segment_all_keys_equal_gives_the_first_positions(gs, cuda):
    length, k = 8 * CH + 1, 1000
    for kt, desc in ((U64, False), (F64, True)):
        c = Case(gs, cuda, np.full(length + 7, 0x3FF0000000000000, np.uint64), [7], [7 + length])
        assert np.array_equal(c.expect(k, kt, desc, ARGS)[1][0], np.arange(k, dtype=np.uint32))
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_long_segment_tie_runs_across_chunk_and_round_boundaries_with_the_cut_inside(gs, cuda):
    """15 * CH + 1 keys: 990 smaller keys scattered over all chunks, and three runs of one equal key: across the boundary of
    chunks 0 and 1, across that of chunks 7 and 8 (where the final's first round ends and its second begins), and the
    segment's last three elements.  k = 1000 and 1010 cut the first run before and behind its chunk boundary, 1017 the
    second behind its round boundary, 1024 the third -- there the new candidate ties with carried ones and must lose.  The
    keys above the runs take 16-bit values: tied among themselves everywhere, six bytes constant."""
    length = 15 * CH + 1
    rng = np.random.default_rng(5)
    keys = rng.integers(2000, 1 << 16, length).astype(np.uint64)
    runs = np.r_[CH - 10:CH + 11, 8 * CH - 5:8 * CH + 6, length - 3:length]
    keys[runs] = 1000
    free = np.setdiff1d(np.arange(length), runs)
    keys[rng.choice(free, 990, replace=False)] = np.arange(990, dtype=np.uint64)
    c = Case(gs, cuda, np.r_[np.uint64(7), keys], [1], [1 + length])
    assert SR.final_rounds(length, 1024) == 3
    for k, last in ((1000, CH - 1), (1010, CH + 9), (1017, 8 * CH), (1024, length - 2)):
        ev = c.expect(k, U64, False, ARGS)[1][0]
        assert list(ev[990:]) == list(runs[:k - 990]) and ev[-1] == last
        for mode in MODES:
            c.check(k, U64, False, mode)
    c = Case(gs, cuda, np.r_[np.uint64(7), ~keys], [1], [1 + length])
    c.check(1024, U64, True, ARGS)


# ------------------------------------------------------------------------------- 4., 5. pads and special values --
PAD_LENGTHS = [1, 63, 65, 1025, CH + 1]          # a wave with one pad lane, the next class, a workgroup, two chunks


@pytest.mark.parametrize("kt", SW.KEY_TYPES)
def test_the_pad_image_is_an_ordinary_key(gs, cuda, kt):
    """Segments made of nothing but the key whose image is all ones -- the pad's -- in the direction at hand, and segments
    where it is mixed with a few others: the positions of equal keys come out in input order, so a pad taken for a key would
    show as a position past the segment or as a missing one."""
    begin, end, n = SR.packed(PAD_LENGTHS, gap=3, first=1)
    rng = np.random.default_rng(40 + kt)
    for desc in (False, True):
        top = SW.preimage(np.array([SW.FILL64]), kt, desc)[0]
        assert SW.image(np.array([top], np.uint64), kt, desc)[0] == SW.FILL64
        only = np.full(n, top, np.uint64)
        mixed = np.where(rng.random(n) < 0.9, top, W.gen64("uniform", n, seed=41)).astype(np.uint64)
        for keys in (only, mixed):
            c = Case(gs, cuda, keys, begin, end)
            assert c.status == [2, 1, 0, 0, 1, 1, 2, 0]
            for k in (1, 64, 1024):
                for mode in MODES:
                    c.check(k, kt, desc, mode)
        ev = Case(gs, cuda, only, begin, end).expect(64, kt, desc, ARGS)[1]
        assert list(ev[1, :63]) == list(range(63)) and ev[1, 63] == FILL


@pytest.mark.parametrize("kt", SW.KEY_TYPES)
def test_special_values(gs, cuda, kt):
    """F64 +-0, +-inf, denormals, NaNs of both signs with payloads, I64 / U64 at their extremes: nine keys in ten are
    specials, so every segment is full of them and of ties."""
    begin, end, n = SR.packed(PAD_LENGTHS, gap=3, first=1)
    rng = np.random.default_rng(50 + kt)
    sp = W.specials64(kt)
    keys = np.where(rng.random(n) < 0.9, sp[rng.integers(0, sp.size, n)], W.gen64("uniform", n, seed=51)).astype(np.uint64)
    c = Case(gs, cuda, keys, begin, end)
    for desc in (False, True):
        for k in (1, 65, 1024):
            for mode in MODES:
                c.check(k, kt, desc, mode)
    if kt == F64:      # the order stated at the enum: negative NaNs first ascending, positive NaNs first descending
        first, last = c.expect(1024, kt, False, KEYS)[0][4], c.expect(1024, kt, True, KEYS)[0][4]
        assert first[0] >> np.uint64(63) and (first[0] & np.uint64((1 << 63) - 1)) > np.uint64(0x7FF0000000000000)
        assert not last[0] >> np.uint64(63) and last[0] > np.uint64(0x7FF0000000000000)


# ------------------------------------------------------------------------------------ 6. the lists and the offsets --
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
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=50 + q), begin, begin + lens.astype(np.int32))
        assert c.status[q] == count and sum(c.status) == count
        c.check((8, 100, 300, 1024, 64)[q], kt, desc, mode)
    lens = CH + 1 + (i % 7)
    begin, end, n = SR.packed(list(lens), first=1)
    kt, desc, mode = rotate(ci + 5)
    c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=57, kinds=["uniform", "five", "small"]), begin, end)
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
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=60 + i), begin, end)
        assert c.status[:6] == [300, 200, 150, 100, 20, 6] and c.status[7] == 0
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_gaps_reverse_order_and_a_repeated_segment(gs, cuda):
    lens = [5, 300, 0, 1024, 2000, CH + 9, 64, 700]
    begin, end, n = SR.packed(lens, gap=11, first=3)
    begin, end = begin[::-1].copy(), end[::-1].copy()                   # the segments in reverse order
    begin, end = np.r_[begin, begin[[0, 3, 6]]], np.r_[end, end[[0, 3, 6]]]     # 700, 2000 and 300 once more
    for i, k in enumerate((3, 129, 1000)):
        kt, desc, _ = rotate(i)
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=70 + i), begin.astype(np.int32), end.astype(np.int32))
        assert c.status[5] == 1
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_sliding_windows_of_100_with_step_1(gs, cuda):
    n = 5000
    begin = np.arange(0, n - 100 + 1, dtype=np.int32)
    for i, k in enumerate((1, 10, 100)):
        kt, desc, mode = rotate(i + 2)
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=80 + i, kinds=["uniform", "five", "small", "normal"]), begin, begin + 100)
        assert c.status == [0, begin.size, 0, 0, 0, 0, 0, 0]
        c.check(k, kt, desc, mode)


def test_odd_element_offsets(gs, cuda):
    """Every segment starts at an odd element and has an odd length, k is odd: every output row and every second candidate
    row start at an odd element too."""
    lens = [33, 255, 777, 2001, CH + 1, 3 * CH + 5]
    begin, end, n = SR.packed(lens, gap=1, first=1)
    assert all(int(b) & 1 for b in begin)
    for i, k in enumerate((1, 63, 1023)):
        kt, desc, mode = rotate(i)
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=85 + i), begin, end)
        c.check(k, kt, desc, mode)


def test_device_offsets_that_need_clamping(gs, cuda):
    """Offsets below 0 and above num_items, and end < begin: clamped on the device, positions counted from the clamped begin.
    Every array sits between guard zones."""
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
        kt, desc = (F64, U64, I64)[i], bool(i % 2)
        keys, vals = SW.flat_keys64(n, kt, seed=90 + i), values_for(n, seed=4)
        hv = int(mode != KEYS)
        ek, ev, ec = SW.seg_topk64(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=1)
        a.add("keys_in", 8 * n, offset=8, data=keys, const=True).add("vals_in", 4 * n, data=vals, const=True)
        a.add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, offset=8, data=end, const=True)
        a.add("keys_out", 8 * S * k, offset=24, fill="ff").add("vals_out", 4 * S * k, fill="ff")
        a.add("counts", 4 * S, fill="ff").add("temp", nb, offset=3, fill="random").build()
        assert gs.lib.gs_topk_segmented_u64(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                            a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, int(desc),
                                            kt, None) == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == want
        assert np.array_equal(a.read("counts", np.uint32), ec)
        assert np.array_equal(a.read("keys_out", np.uint64).reshape(S, k), ek), mode
        assert np.array_equal(a.read("vals_out", np.uint32).reshape(S, k), ev if hv else np.full((S, k), FILL, np.uint32)), mode


def test_dropped_segments(gs, cuda):
    """Three copies of one segment of num_items = 4 * CH elements at k = 1024.  Lmax = 3 records would hold them, but each needs
    four of the Tmax = 7 chunk-task slots: exactly one completes, whichever it is, and is correct; the others are dropped:
    count 0, slots unwritten, out[7] = 2.  No guard byte anywhere is changed."""
    n, S, k = 4 * CH, 3, 1024
    lmax, tmax = SR.geometry(n, S)
    fit = min(lmax, tmax // 4)
    assert (lmax, tmax, fit) == (3, 7, 1)
    keys = SW.flat_keys64(n, I64, seed=95)
    begin, end = np.zeros(S, np.int32), np.full(S, n, np.int32)
    ek, ev, ec = SW.seg_topk64(keys, begin[:1], end[:1], k, I64, False)
    for mode in (ARGS, KEYS):
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=2)
        a.add("keys_in", 8 * n, offset=8, data=keys, const=True).add("begin", 4 * S, data=begin, const=True)
        a.add("end", 4 * S, data=end, const=True)
        a.add("keys_out", 8 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff").add("counts", 4 * S, fill="ff")
        a.add("temp", nb, offset=1, fill="random").build()
        assert gs.lib.gs_topk_segmented_u64(a.ptr("temp"), nb, a.ptr("keys_in"), None, a.ptr("keys_out"), a.ptr("vals_out") if hv else None,
                                            a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, 0, I64, None) == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == [0, 0, 0, 0, 0, fit, 4 * fit, S - fit]
        gk, gv = a.read("keys_out", np.uint64).reshape(S, k), a.read("vals_out", np.uint32).reshape(S, k)
        gc = a.read("counts", np.uint32)
        assert sorted(gc) == [0] * (S - fit) + [k] * fit
        for s in range(S):
            if gc[s]:
                assert np.array_equal(gk[s], ek[0]) and (not hv or np.array_equal(gv[s], ev[0]))
            else:
                assert (gk[s] == FILL64).all()
            assert hv or (gv[s] == FILL).all()
            assert gc[s] or (gv[s] == FILL).all()


def test_dropped_segments_without_a_record_slot(gs, cuda):
    """Five copies of one segment of CH + 1 elements in num_items = 2 * CH + 2: Lmax = 2 and Tmax = 4, two chunk tasks a copy.
    Exactly two copies complete, whichever they are; three find no record slot and are dropped: count 0, slots unwritten,
    out[7] = 3.  No guard byte is changed."""
    n, S, k = 2 * CH + 2, 5, 100
    assert SR.geometry(n, S) == (2, 4)
    keys = SW.flat_keys64(n, U64, seed=96)
    begin, end = np.full(S, 1, np.int32), np.full(S, CH + 2, np.int32)
    ek, ev, _ = SW.seg_topk64(keys, begin[:1], end[:1], k, U64, True)
    nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, 1)
    a = Arena(cuda, seed=3)
    a.add("keys_in", 8 * n, data=keys, const=True).add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, data=end, const=True)
    a.add("keys_out", 8 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff").add("counts", 4 * S, fill="ff")
    a.add("temp", nb, offset=5, fill="random").build()
    assert gs.lib.gs_topk_segmented_u64(a.ptr("temp"), nb, a.ptr("keys_in"), None, a.ptr("keys_out"), a.ptr("vals_out"), a.ptr("counts"), n, S,
                                        a.ptr("begin"), a.ptr("end"), k, 1, U64, None) == 0
    a.check()
    assert status_of(gs, a.ptr("temp"), n, S, k, 1) == [0, 0, 0, 0, 0, 2, 4, 3]
    gk, gv = a.read("keys_out", np.uint64).reshape(S, k), a.read("vals_out", np.uint32).reshape(S, k)
    gc = a.read("counts", np.uint32)
    assert sorted(gc) == [0, 0, 0, k, k]
    for s in range(S):
        if gc[s]:
            assert np.array_equal(gk[s], ek[0]) and np.array_equal(gv[s], ev[0])
        else:
            assert (gk[s] == FILL64).all() and (gv[s] == FILL).all()


# ------------------------------------------------------------------------------- 7. - 9. buffers and reuse --
@pytest.mark.parametrize("lens,k", GUARDED)
def test_guarded_offset_dirty_buffers(gs, cuda, lens, k):
    """Every array in a slot of its own between guard zones: the key arrays at byte offsets that are odd multiples of 8 past
    a 256-byte boundary, the u32 arrays at multiples of 4, the workspace at an odd one; outputs, counts and workspace dirty;
    the slots past a segment's count keep their bytes."""
    begin, end, n = SR.packed(lens, gap=1)
    S = len(lens)
    for i, mode in enumerate(MODES):
        kt, desc = (F64, I64, U64)[i], bool(i % 2)
        keys, vals = SW.flat_keys64(n, kt, seed=100 + i), values_for(n, seed=9)
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv)
        a = Arena(cuda, seed=i)
        a.add("keys_in", 8 * n, offset=(8, 24, 40)[i], data=keys, const=True)
        a.add("vals_in", 4 * n, offset=12, data=vals, const=True)
        a.add("begin", 4 * S, offset=16, data=begin, const=True)
        a.add("end", 4 * S, offset=28, data=end, const=True)
        a.add("keys_out", 8 * S * k, offset=(56, 8, 24)[i], fill="random")
        a.add("vals_out", 4 * S * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("counts", 4 * S, offset=36, fill="random")
        a.add("temp", nb, offset=(1, 7, 131)[i], fill="random")
        a.build()
        assert a.ptr("keys_in") % 16 == 8 and a.ptr("keys_out") % 16 == 8 and a.ptr("temp") % 2 == 1
        rc = gs.lib.gs_topk_segmented_u64(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                                          a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, int(desc),
                                          kt, None)
        assert rc == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == SR.status(begin, end, n)
        ek, ev, ec = SW.seg_topk64(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        assert np.array_equal(a.read("counts", np.uint32), ec)
        written = (np.arange(k)[None, :] < ec[:, None])
        gk, ik = a.read("keys_out", np.uint64).reshape(S, k), a.init["keys_out"].view(np.uint64).reshape(S, k)
        assert np.array_equal(gk, np.where(written, ek, ik)), (mode, lens, k)
        gv, iv = a.read("vals_out", np.uint32).reshape(S, k), a.init["vals_out"].view(np.uint32).reshape(S, k)
        assert np.array_equal(gv, np.where(written, ev, iv) if hv else iv), (mode, lens, k)


def test_refused_calls_write_nothing(gs, cuda):
    n, S, k = 9000, 3, 10
    nb = gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 8 * n, fill="random").add("keys_out", 8 * S * k, fill="random").add("vals_out", 4 * S * k, fill="random")
    a.add("counts", 4 * S, fill="random").add("begin", 4 * S, data=np.array([0, 100, 200], np.int32))
    a.add("end", 4 * S, data=np.array([100, 200, 9000], np.int32)).add("temp", nb, fill="random").build()

    def call(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), counts=a.ptr("counts"),
                 n=n, S=S, begin=a.ptr("begin"), end=a.ptr("end"), k=k, kt=U64)
        p.update(kw)
        return gs.lib.gs_topk_segmented_u64(p["temp"], p["nb"], p["kin"], None, p["kout"], p["vout"], p["counts"], p["n"], p["S"], p["begin"],
                                            p["end"], p["k"], 0, p["kt"], None)
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=1025), dict(n=1 << 31), dict(kt=0), dict(kt=2), dict(kt=8), dict(kt=11), dict(kt=12),
               dict(begin=None), dict(end=None), dict(kout=a.ptr("keys_in") + 8), dict(vout=a.ptr("keys_out") + 8 * S * k - 4),
               dict(kin=a.ptr("keys_in") + 4), dict(kout=a.ptr("keys_out") + 4), dict(kin=a.ptr("keys_in") + 1),
               dict(vout=a.ptr("vals_out") + 2), dict(counts=a.ptr("begin")), dict(counts=a.ptr("keys_out"))):
        assert call(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A ragged pairs call with long segments, a keys call on other offsets and the first one again, on one stream and one
    workspace without a synchronisation between them: the third call's bytes equal the first's."""
    lens_a, ka = [2 * CH + 9, 300, 5000, 9 * CH + 3, 40], 301
    begin_a, end_a, na = SR.packed(lens_a, first=1)
    a = Case(gs, cuda, SW.flat_keys64(na, F64, seed=110), begin_a, end_a)
    begin_b, end_b, nb_items = SR.packed([5000, 77, CH + 1, 1])
    b = Case(gs, cuda, SW.flat_keys64(nb_items, I64, seed=111), begin_b, end_b)
    nb = max(gs.lib.gs_topk_segmented_u64_temp_bytes(na, a.S, ka, 1), gs.lib.gs_topk_segmented_u64_temp_bytes(nb_items, b.S, 77, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [(torch.full((a.S * ka,), -1, dtype=torch.int64, device=cuda), torch.full((a.S * ka,), -1, dtype=torch.int32, device=cuda),
             torch.full((a.S,), -1, dtype=torch.int32, device=cuda)) for _ in range(2)]
    kb = torch.full((b.S * 77,), -1, dtype=torch.int64, device=cuda)

    def run_a(ko, vo, co):
        assert gs.lib.gs_topk_segmented_u64(temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(),
                                            co.data_ptr(), na, a.S, a.d_begin.data_ptr(), a.d_end.data_ptr(), ka, 1, F64, None) == 0
    run_a(*outs[0])
    assert gs.lib.gs_topk_segmented_u64(temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, None, nb_items, b.S,
                                        b.d_begin.data_ptr(), b.d_end.data_ptr(), 77, 0, I64, None) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    assert gs.DeviceTopKSegmented64.Status(temp, na, a.S, ka, 1) == a.status
    ek, ev, ec = a.expect(ka, F64, True, PAIRS)
    assert np.array_equal(host64(outs[0][0]).reshape(a.S, ka), ek) and np.array_equal(host(outs[0][1]).reshape(a.S, ka), ev)
    assert np.array_equal(host(outs[0][2]), ec)
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert np.array_equal(host64(kb).reshape(b.S, 77), b.expect(77, I64, False, KEYS)[0])


# ------------------------------------------------------------------------------------------- 10. graph capture --
def test_topk_segmented_u64_is_capturable_in_a_hip_graph(gs, cuda):
    """Captured once on one plain side stream (no parallel branches), all ten launches, replayed once on new data in the same
    buffers; the status is read after the replay."""
    lens, k = [8 * CH + 1, 500, 2 * CH, 3000, 9], 1023
    begin, end, n = SR.packed(lens, gap=1, first=1)
    S = len(lens)
    sets = [SW.flat_keys64(n, F64, seed=120 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "special"))]
    src, d_begin, d_end = dev64(sets[0], cuda), dev(begin, cuda), dev(end, cuda)
    ko = torch.full((S * k,), -1, dtype=torch.int64, device=cuda)
    vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
    co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
    D = gs.DeviceTopKSegmented64
    nb = D.MaxPairs(None, 0, None, None, None, None, None, n, S, None, None, k)
    assert nb == SW.temp_bytes64(n, S, k, 1) and D.Plan(n, S, k, True) == SR.plan(n, S, k) and D.Plan(n, S, k, True)[1] == 10
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_F64)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_F64)
    keys = sets[1]
    src.copy_(dev64(keys, cuda))
    ko.fill_(-1)
    vo.fill_(-1)
    co.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    ek, ev, ec = SW.seg_topk64(keys, begin, end, k, F64, True)
    assert np.array_equal(host64(ko).reshape(S, k), ek) and np.array_equal(host(vo).reshape(S, k), ev)
    assert np.array_equal(host(co), ec)
    assert D.Status(temp, n, S, k, True, stream=side) == SR.status(begin, end, n)     # the state block is zeroed in the replay


# ------------------------------------------------------------------------------------------- 11. identities --
LIST_SHAPES = [([40, 1, 64], 8), ([200, 65, 256], 100), ([400, 257, 512], 300), ([900, 513, 1024], 1024), ([3000, 1025, CH], 65),
               ([CH + 5, 2 * CH + 1], 1023)]


@pytest.mark.parametrize("lens,k", LIST_SHAPES)
def test_equals_the_32_bit_entry_point_on_the_widened_keys(gs, cuda, lens, k):
    """gs_topk_segmented_u32 on 32-bit keys against gs_topk_segmented_u64 on (uint64_t)key << 32 with the key type widened:
    one shape per list, every key type, the directions and forms in turn; compared on the device's own outputs."""
    q = [s[0] for s in LIST_SHAPES].index(lens)
    begin, end, n = SR.packed(lens, gap=1, first=1)
    S = len(lens)
    assert SR.status(begin, end, n)[q] == S
    rng = np.random.default_rng(140 + q)
    for i, kt32 in enumerate((R.U32, R.I32, R.F32)):
        desc, mode = bool((i + q) & 1), MODES[(i + q) % 3]
        hv = int(mode != KEYS)
        keys32 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        keys32 = np.where(rng.random(n) < 0.3, keys32[:5][rng.integers(0, 5, n)], keys32)      # ties: three in ten take one of five keys
        c = Case(gs, cuda, WR.widen32(keys32), begin, end)
        kt = SW.WIDE[kt32]
        c.check(k, kt, desc, mode)
        _, ko64, vo64, co64 = c.run(k, kt, desc, mode)
        narrow = dev(keys32, cuda)
        nb = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        assert nb <= gs.lib.gs_topk_segmented_u64_temp_bytes(n, S, k, hv) <= 2 * nb
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_segmented_u32(temp.data_ptr(), nb, narrow.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                                            vo.data_ptr() if hv else None, co.data_ptr(), n, S, c.d_begin.data_ptr(), c.d_end.data_ptr(), k,
                                            int(desc), kt32, None) == 0
        gc = host(co)
        written = np.arange(k)[None, :] < gc[:, None]
        g64, g32 = host64(ko64)[:S * k].reshape(S, k), host(ko).reshape(S, k)
        assert np.array_equal(gc, host(co64)[:S])
        assert np.array_equal((g64 >> np.uint64(32)).astype(np.uint32)[written], g32[written]) and not (g64[written] & np.uint64(0xFFFFFFFF)).any()
        assert not hv or np.array_equal(host(vo64)[:S * k].reshape(S, k)[written], host(vo).reshape(S, k)[written])


@pytest.mark.parametrize("rows,cols,k", [(37, 301, 21), (5, 3001, 100), (3, 2 * CH + 9, 301)])
def test_regular_offsets_equal_topk_rows_u64(gs, cuda, rows, cols, k):
    """gs_topk_segmented_u64 on regular offsets against gs_topk_rows_u64 on the same matrix, one shape per path of the rows
    entry point, all forms."""
    begin = (np.arange(rows) * cols).astype(np.int32)
    for i, mode in enumerate(MODES):
        kt, desc = (F64, U64, I64)[i], bool((i + 1) % 2)
        c = Case(gs, cuda, SW.flat_keys64(rows * cols, kt, seed=130 + i), begin, begin + cols)
        hv = int(mode != KEYS)
        nb = max(gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv), 256)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((rows * k,), -1, dtype=torch.int64, device=cuda)
        vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_rows_u64(temp.data_ptr(), nb, c.d_keys.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                                       vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None) == 0
        _, sk, sv, _ = c.run(k, kt, desc, mode)
        assert torch.equal(sk[:rows * k], ko) and (not hv or torch.equal(sv[:rows * k], vo))
        c.check(k, kt, desc, mode)


def test_a_handful_of_segments_equal_topk_u64_on_the_sub_array(gs, cuda):
    lens, k = [50, 700, 3000, 2 * CH + 9, 8], 40
    begin, end, n = SR.packed(lens, gap=2, first=2)
    for i, mode in enumerate((PAIRS, ARGS)):
        kt, desc = (I64, F64)[i], bool(i)
        c = Case(gs, cuda, SW.flat_keys64(n, kt, seed=160 + i), begin, end)
        _, sk, sv, sc = c.run(k, kt, desc, mode)
        for s, ln in enumerate(lens):
            kept = min(k, ln)
            lo = int(begin[s])
            nb = gs.lib.gs_topk_u64_temp_bytes(ln, kept, 1)
            temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
            ko = torch.empty(kept, dtype=torch.int64, device=cuda)
            vo = torch.empty(kept, dtype=torch.int32, device=cuda)
            assert gs.lib.gs_topk_u64(temp.data_ptr(), nb, c.d_keys[lo:].data_ptr(), c.d_vals[lo:].data_ptr() if mode == PAIRS else None,
                                      ko.data_ptr(), vo.data_ptr(), ln, kept, int(desc), kt, None) == 0
            assert torch.equal(sk[s * k:s * k + kept], ko) and torch.equal(sv[s * k:s * k + kept], vo) and int(sc[s]) == kept


def _tie_free(dtype, lens, rng):
    """Per segment, distinct values: int64 anywhere in its range, float64 finite and non-zero."""
    out = []
    for ln in lens:
        if dtype == torch.int64:
            v = np.unique(rng.integers(-(1 << 63), (1 << 63) - 1, 2 * ln + 8, dtype=np.int64))
        else:
            v = np.unique(rng.standard_normal(2 * ln + 8) * 10.0 ** rng.integers(-200, 200, 2 * ln + 8))
            v = v[np.isfinite(v) & (v != 0)]
        out.append(rng.permutation(v)[:ln])
        assert out[-1].size == ln
    return np.concatenate(out + [np.empty(0, out[0].dtype)])


@pytest.mark.parametrize("dtype", [torch.int64, torch.float64])
def test_topk_segmented64_against_torch_topk(gs, cuda, dtype):
    rng = np.random.default_rng(17)
    lens = [0, 1, 5, 100, 1000, 3001, CH + 50, 20000, 64]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(offsets[-1])
    x = torch.from_numpy(_tie_free(dtype, lens, rng)).to(cuda)
    assert x.dtype == dtype
    off = torch.from_numpy(offsets).to(cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) * 3
    for k in (1, 51, 1024):
        for largest in (False, True):
            ko, io, counts = gs.topk_segmented64(x, off, k, largest=largest, indices=True)
            k2, none, c2 = gs.topk_segmented64(x, off[:-1].contiguous(), k, largest=largest, end_offsets=off[1:].contiguous())
            k3, v3, _ = gs.topk_segmented64(x, off, k, largest=largest, values=vals)
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
        gs.topk_segmented64(x, off, 1025)
    with pytest.raises(TypeError):
        gs.topk_segmented(x, off, 5)


def test_device_topk_segmented64_with_an_explicit_key_type_on_a_uint64_as_int64_tensor(gs, cuda):
    """key_type=GS_KEY_U64 on an int64 tensor orders the bit patterns as unsigned; without it the tensor's own type (I64)
    holds; a 32-bit key type on it raises TypeError."""
    lens, k = [70, 2000, CH + 3, 5], 33
    begin, end, n = SR.packed(lens, gap=2, first=1)
    S = len(lens)
    keys = SW.flat_keys64(n, U64, seed=150, kinds=["uniform"])
    src, d_begin, d_end = dev64(keys, cuda), dev(begin, cuda), dev(end, cuda)
    D = gs.DeviceTopKSegmented64
    for key_type, kt in ((gs.GS_KEY_U64, U64), (None, I64)):
        ko = torch.full((S * k,), -1, dtype=torch.int64, device=cuda)
        vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
        co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
        nb = D.MinPairs(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=gs.GS_KEY_U64)
        assert nb == SW.temp_bytes64(n, S, k, 1)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        assert D.MinPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=key_type) == nb
        assert D.Status(temp, n, S, k, True) == SR.status(begin, end, n)
        ek, ev, ec = SW.seg_topk64(keys, begin, end, k, kt, False)
        assert np.array_equal(host64(ko).reshape(S, k), ek) and np.array_equal(host(vo).reshape(S, k), ev) and np.array_equal(host(co), ec)
    assert not np.array_equal(SW.seg_topk64(keys, begin, end, k, U64)[0], SW.seg_topk64(keys, begin, end, k, I64)[0])
    with pytest.raises(TypeError):
        D.MinPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_U32)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_segmented_wide_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 3 * 3 * 2 * 6
