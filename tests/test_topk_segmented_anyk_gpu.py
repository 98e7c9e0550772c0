"""gs_topk_segmented_anyk_u32 on the device: every segment bit for bit against tests/topk_segmented_anyk_ref.py (keys, values
or positions, counts, and the sentinel in every slot that must stay unwritten), with the list counts of
gs_topk_segmented_anyk_status asserted against the ref: lengths at every edge with k below, at and above each, tie runs across
tiles, keys that leave the decision to the second and third counting round, float specials, every offset pattern, the drop
rule, list sizes, guarded buffers, refusals, workspace reuse, graph capture, the cross-checks against gs_topk_rows_anyk_u32,
gs_topk_segmented_u32 and torch.sort, the C++ driver and a seeded sweep."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import topk_campaign as TC
import topk_ref as R
import topk_segmented_anyk_ref as AR
from guarded import Arena
from topk_cases import DISTS, gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
CH = AR.CH
TAIL = 64            # sentinel elements behind the outputs and the counts


# ------------------------------------------------------------------------------------------------------- inputs --
def flat_keys(n, kt, seed, kinds=DISTS):
    """n keys in pieces of different distributions, so that the segments of one call see all of them."""
    piece = max(1, -(-n // (2 * len(kinds))))
    parts = [gen(kinds[(i + seed) % len(kinds)], min(piece, n - lo), seed=seed * 1009 + i + 1, kt=kt)
             for i, lo in enumerate(range(0, n, piece))]
    return np.concatenate(parts).astype(np.uint32)


def values_for(n, seed=3):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def rotate(i):
    return (U32, I32, F32)[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def need_bytes(gs, n, S, k, hv):
    nb = gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, hv)
    assert nb == AR.temp_bytes(n, S, k, hv, gs.lib.gs_segmented_temp_bytes(S * k, hv, S)) > 0, (n, S, k, hv)
    return nb


def call(gs, temp, nb, kin, vin, kout, vout, counts, n, S, begin, end, k, desc, kt, stream=None):
    return gs.lib.gs_topk_segmented_anyk_u32(temp, nb, kin, vin, kout, vout, counts, n, S, begin, end, k, int(desc), kt, stream)


def status_of(gs, temp, n, S, k, hv):
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_segmented_anyk_status(temp, n, S, k, hv, out, None) == 0
    return list(out)


class Case:
    """One flat array and one set of offsets on the device; .check(k, kt, desc, mode) runs the C entry point and compares
    outputs, counts, unwritten slots and the status words."""

    def __init__(self, gs, cuda, keys, begin, end, status=True):
        self.gs, self.cuda = gs, cuda
        self.keys, self.vals = np.ascontiguousarray(keys, np.uint32), values_for(len(keys))
        self.begin, self.end = np.asarray(begin, np.int32), np.asarray(end, np.int32)
        self.n, self.S = self.keys.size, self.begin.size
        self.d_keys, self.d_vals = dev(self.keys, cuda), dev(self.vals, cuda)
        self.d_begin, self.d_end = dev(self.begin, cuda), dev(self.end, cuda)
        self.cache = {}
        self.status = AR.status(self.begin, self.end, self.n) if status else None

    def expect(self, k, kt, desc, mode):
        c = self.cache.setdefault((kt, desc), {})
        return AR.seg_topk(self.keys, self.begin, self.end, k, kt, desc, self.vals if mode == PAIRS else None, cache=c)

    def run(self, k, kt, desc, mode, counts=True):
        gs, n, S = self.gs, self.n, self.S
        hv = int(mode != KEYS)
        nb = need_bytes(gs, n, S, k, hv)
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        vo = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        co = torch.full((S + TAIL,), -1, dtype=torch.int32, device=self.cuda)
        rc = call(gs, temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None, ko.data_ptr(),
                  vo.data_ptr() if hv else None, co.data_ptr() if counts else None, n, S, self.d_begin.data_ptr(), self.d_end.data_ptr(),
                  k, desc, kt)
        assert rc == 0, (rc, n, S, k, mode)
        return status_of(gs, temp.data_ptr(), n, S, k, hv), host(ko), host(vo), host(co)

    def check(self, k, kt, desc, mode, counts=True):
        S = self.S
        hv = int(mode != KEYS)
        what = "n=%d S=%d k=%d %s kt=%d desc=%d" % (self.n, S, k, mode, kt, desc)
        st, gk, gv, gc = self.run(k, kt, desc, mode, counts)
        assert st == self.status, (what, st, self.status)
        ek, ev, ec = self.expect(k, kt, desc, mode)
        bad = np.nonzero((gk[:S * k].reshape(S, k) != ek).any(axis=1))[0]
        assert bad.size == 0, (what, "keys of segments", bad[:8], "lengths", (self.end - self.begin)[bad[:8]])
        assert (gk[S * k:] == AR.FILL).all(), what
        if hv:
            bad = np.nonzero((gv[:S * k].reshape(S, k) != ev).any(axis=1))[0]
            assert bad.size == 0, (what, "values of segments", bad[:8], "lengths", (self.end - self.begin)[bad[:8]])
            assert (gv[S * k:] == AR.FILL).all(), what
        else:
            assert (gv == AR.FILL).all(), what
        if counts:
            assert np.array_equal(gc[:S], ec) and (gc[S:] == AR.FILL).all(), what
        else:
            assert (gc == AR.FILL).all(), what

    def check_all(self, k, directions=(False, True), types=(U32, I32, F32), modes=MODES):
        for kt in types:
            for desc in directions:
                for mode in modes:
                    self.check(k, kt, desc, mode)


# ------------------------------------------------------------------------------------------ lengths at every edge --
@pytest.fixture(scope="module")
def edge_case(gs, cuda):
    begin, end, n, _ = AR.shuffled_edges()
    c = Case(gs, cuda, flat_keys(n, F32, seed=1), begin, end)
    assert c.status == AR.EDGE_STATUS and c.status[7] == 0
    return c


@pytest.mark.parametrize("k", AR.EDGE_KS)
def test_lengths_at_every_edge_in_one_ragged_call(edge_case, k):
    """0 .. 65537 in one call, in shuffled order at odd, unaligned starts; k below, at and above every length; all three forms,
    both directions, the three key types, and once without counts."""
    edge_case.check_all(k)
    edge_case.check(k, U32, True, ARGS, counts=False)


# ------------------------------------------------------------------------------------------------ long segments --
@pytest.mark.parametrize("k", AR.EQUAL_KS)
def test_long_segment_all_keys_equal_gives_the_first_positions(gs, cuda, k):
    """20000 equal keys: the cut falls inside a tie run that crosses tiles, and the positions must be 0 .. k - 1."""
    n = AR.EQUAL_LENGTH
    c = Case(gs, cuda, np.full(n + 7, 0x3F800000, np.uint32), [7], [7 + n])
    assert c.status == [0, 0, 0, 0, 0, 1, 3, 0]
    assert np.array_equal(c.expect(k, F32, True, ARGS)[1][0], np.arange(k, dtype=np.uint32))
    c.check_all(k)


@pytest.mark.parametrize("shared", [11, 22, "two"])
def test_keys_that_share_their_leading_bits(gs, cuda, shared):
    """Images that share their top 11 or top 22 bits, so that the second or the third counting round decides; and exactly two
    distinct values.  One long segment of 3 tiles + 1 next to one of 8193 and a short one."""
    rng = np.random.default_rng(31)
    lens = [3 * CH + 1, 500, CH + 1]
    begin, end, n = AR.packed(lens, gap=3, first=1)
    if shared == "two":
        img = np.where(rng.random(n) < 0.5, np.uint32(0x9E3779B9), np.uint32(0x9E3779BA)).astype(np.uint32)
    else:
        low = 32 - shared
        img = (np.uint32(0xA5C3F00F) & np.uint32((0xFFFFFFFF << low) & 0xFFFFFFFF)) | rng.integers(0, 1 << low, n, dtype=np.uint64).astype(np.uint32)
    for kt, desc in ((U32, False), (I32, True), (F32, False), (F32, True)):
        c = Case(gs, cuda, R.preimage(img, kt, desc), begin, end)
        assert c.status == [0, 0, 1, 0, 0, 2, 4 + 2, 0]
        for k in (1, 3000, 8193, 24000):
            for mode in MODES:
                c.check(k, kt, desc, mode)


def test_float_specials_in_a_long_segment(gs, cuda):
    """NaNs of both signs with payloads, +-0, +-inf and denormals, six in ten elements of a long segment, both directions."""
    rng = np.random.default_rng(33)
    first, n = 2 * CH + 77, 3 * CH + 78
    keys = TC.make_keys(rng, "specials", n, TC.F32, False).astype(np.uint32)
    assert np.isnan(keys.view(np.float32)).sum() > 1000 and (keys == 0x80000000).sum() > 100 and (keys == 0).sum() > 100
    c = Case(gs, cuda, keys, [0, first], [first, n])
    assert c.status == [0, 0, 0, 0, 0, 2, 3 + 2, 0]
    for k in (100, 5000, first - 1, first):
        c.check_all(k, types=(F32,))


def test_k_at_and_above_the_length_returns_the_whole_segment_sorted(gs, cuda):
    lens = [2 * CH + 5, 1500, 100]
    begin, end, n = AR.packed(lens, gap=1)
    for i, k in enumerate((2 * CH + 5, 2 * CH + 6, 50000)):
        kt, desc, _ = rotate(i)
        c = Case(gs, cuda, flat_keys(n, kt, seed=40 + i), begin, end)
        ek, ev, ec = c.expect(k, kt, desc, ARGS)
        assert list(ec) == lens
        assert np.array_equal(np.sort(ev[0, :lens[0]]), np.arange(lens[0], dtype=np.uint32))      # the whole segment, each element once
        for mode in MODES:
            c.check(k, kt, desc, mode)


# --------------------------------------------------------------------------------------------- segment layout --
def test_gaps_reverse_order_and_repeated_segments(gs, cuda):
    lens = [5, 300, 0, 1024, 2000, CH + 9, 64, 7000, 2 * CH + 3]
    begin, end, n = AR.packed(lens, gap=11, first=4)
    begin, end = begin[::-1].copy(), end[::-1].copy()                   # the segments in reverse order
    begin, end = np.r_[begin, begin[[1, 4, 7]]], np.r_[end, end[[1, 4, 7]]]     # 7000, 2000 and 300 once more: none of them long
    for i, k in enumerate((3, 1025, 6000)):
        kt, desc, _ = rotate(i)
        c = Case(gs, cuda, flat_keys(n, kt, seed=70 + i), begin.astype(np.int32), end.astype(np.int32))
        assert c.status[5] == 2 and c.status[4] == 4 and c.status[7] == 0
        for mode in MODES:
            c.check(k, kt, desc, mode)


def test_sliding_windows_of_3000_with_step_7(gs, cuda):
    n = 6000
    begin = np.arange(0, n - 3000 + 1, 7, dtype=np.int32)
    for i, k in enumerate((1, 1500, 3000, 3001)):
        kt, desc, mode = rotate(i + 2)
        c = Case(gs, cuda, flat_keys(n, kt, seed=80 + i, kinds=["uniform", "five", "sorted", "zipf"]), begin, begin + 3000)
        assert c.status == [0, 0, 0, 0, begin.size, 0, 0, 0]
        c.check(k, kt, desc, mode)


def test_device_offsets_that_need_clamping(gs, cuda):
    """Offsets below 0 and above num_items, and end < begin: clamped on the device, positions counted from the clamped begin.
    Every array sits between guard zones."""
    n, k = 3 * CH, 2500
    big = (1 << 31) - 1
    begin = np.array([-5, -(1 << 31), n - 10, n - 5000, 500, n, n + 5, -100, -(1 << 31), -7], np.int32)
    end = np.array([40, 3, n + 1000, big, 100, n + 9, n + 2, -3, 2000, n + 7], np.int32)
    _, ln = AR.clamp(begin, end, n)
    assert list(ln) == [40, 3, 10, 5000, 0, 0, 0, 0, 2000, n]
    S = begin.size
    want = AR.status(begin, end, n)
    assert want == [3, 0, 0, 0, 2, 1, 3, 0]
    for i, mode in enumerate(MODES):
        kt, desc = (F32, U32, I32)[i], bool(i % 2)
        keys, vals = flat_keys(n, kt, seed=90 + i), values_for(n, seed=4)
        hv = int(mode != KEYS)
        ek, ev, ec = AR.seg_topk(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        nb = need_bytes(gs, n, S, k, hv)
        a = Arena(cuda, seed=1)
        a.add("keys_in", 4 * n, offset=4, data=keys, const=True).add("vals_in", 4 * n, data=vals, const=True)
        a.add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, offset=8, data=end, const=True)
        a.add("keys_out", 4 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff")
        a.add("counts", 4 * S, fill="ff").add("temp", nb, offset=3, fill="random").build()
        assert call(gs, a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                    a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, desc, kt) == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == want
        assert np.array_equal(a.read("counts", np.uint32), ec)
        assert np.array_equal(a.read("keys_out", np.uint32).reshape(S, k), ek), mode
        assert np.array_equal(a.read("vals_out", np.uint32).reshape(S, k), ev if hv else np.full((S, k), AR.FILL, np.uint32)), mode


# ------------------------------------------------------------------------------------------- dropped segments --
@pytest.mark.parametrize("k", [1000, 9000])
def test_dropped_segments(gs, cuda, k):
    """Two overlapping long segments that together exceed num_items, next to a short and a workgroup-class one: whichever is
    dropped has count 0 and untouched slots and is counted by the status; every kept segment equals the reference.  No guard
    byte anywhere is changed."""
    n = 4 * CH
    begin = np.array([10, 0, 5, 100], np.int32)
    end = np.array([310, 3 * CH + 1, n, 5000], np.int32)
    S = begin.size
    lmax, tmax = AR.geometry(n, S)
    assert (lmax, tmax) == (3, 7) and 4 + 4 > tmax                    # four tile tasks each: only one of the two finds room
    keys, vals = flat_keys(n, I32, seed=95), values_for(n, seed=5)
    for mode in MODES:
        hv = int(mode != KEYS)
        ek, ev, ec = AR.seg_topk(keys, begin, end, k, I32, True, vals if mode == PAIRS else None)
        nb = need_bytes(gs, n, S, k, hv)
        a = Arena(cuda, seed=2)
        a.add("keys_in", 4 * n, data=keys, const=True).add("vals_in", 4 * n, data=vals, const=True)
        a.add("begin", 4 * S, data=begin, const=True).add("end", 4 * S, data=end, const=True)
        a.add("keys_out", 4 * S * k, fill="ff").add("vals_out", 4 * S * k, fill="ff").add("counts", 4 * S, fill="ff")
        a.add("temp", nb, offset=1, fill="random").build()
        assert call(gs, a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                    a.ptr("vals_out") if hv else None, a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, 1, I32) == 0
        a.check()
        st = status_of(gs, a.ptr("temp"), n, S, k, hv)
        gk, gv = a.read("keys_out", np.uint32).reshape(S, k), a.read("vals_out", np.uint32).reshape(S, k)
        gc = a.read("counts", np.uint32)
        dropped = [s for s in (1, 2) if gc[s] == 0]
        assert len(dropped) >= 1 and st == [0, 0, 1, 0, 1, 2 - len(dropped), 4 * (2 - len(dropped)), len(dropped)], (st, gc)
        for s in range(S):
            if s in dropped:
                assert (gk[s] == AR.FILL).all() and (gv[s] == AR.FILL).all()
            else:
                assert gc[s] == ec[s] and np.array_equal(gk[s], ek[s]), (mode, s)
                assert np.array_equal(gv[s], ev[s] if hv else np.full(k, AR.FILL, np.uint32)), (mode, s)


# ------------------------------------------------------------------------------------------------- list sizes --
def test_many_long_segments_spread_over_classify_workgroups(gs, cuda):
    """1030 long segments of CH + 1 elements: two classify workgroups claim records and task slots, the second from cursors
    that are no longer zero, and more records than one pick workgroup per multiprocessor."""
    count = AR.LONG_COUNT
    begin, end, n = AR.packed([CH + 1] * count)
    c = Case(gs, cuda, flat_keys(n, U32, seed=57, kinds=["uniform", "five", "topbyte"]), begin, end)
    assert c.status == [0, 0, 0, 0, 0, count, 2 * count, 0]
    c.check(1100, U32, False, ARGS)
    c.check(9000, U32, True, KEYS)


@pytest.mark.parametrize("count", AR.BLOCK_COUNTS)
def test_block_list_sizes_around_a_classify_workgroups_share(gs, cuda, count):
    """`count` segments of 1025 .. 1100 elements, which overlap freely (the input is only read)."""
    i = np.arange(count)
    lens = 1100 - (i % 76)
    n = 20000
    begin = ((i * 37) % (n - 1100)).astype(np.int32)
    kt, desc, mode = rotate(AR.BLOCK_COUNTS.index(count))
    c = Case(gs, cuda, flat_keys(n, kt, seed=50), begin, begin + lens.astype(np.int32))
    assert c.status == [0, 0, 0, 0, count, 0, 0, 0]
    c.check(1060, kt, desc, mode)


# ----------------------------------------------------------------------------------------- buffers and reuse --
GUARDED = [([5, 300, 0, 64, 1000], 1500), ([4000, 70, 1025], 1025), ([CH + 5, 2, 3 * CH + 1, 600], 9000)]


@pytest.mark.parametrize("lens,k", GUARDED)
def test_guarded_offset_dirty_buffers(gs, cuda, lens, k):
    """Every array in a slot of its own between guard zones, at byte offsets 4, 8, 12, ... from a 256-byte boundary (the
    workspace at an odd one), outputs, counts and workspace dirty; the slots past a segment's count keep their bytes; once
    without counts."""
    begin, end, n = AR.packed(lens, gap=1)
    S = len(lens)
    for i, mode in enumerate(MODES):
        kt, desc = (U32, I32, F32)[i], bool(i % 2)
        keys, vals = flat_keys(n, kt, seed=100 + i), values_for(n, seed=9)
        hv = int(mode != KEYS)
        nb = need_bytes(gs, n, S, k, hv)
        a = Arena(cuda, seed=i)
        a.add("keys_in", 4 * n, offset=4, data=keys, const=True)
        a.add("vals_in", 4 * n, offset=12, data=vals, const=True)
        a.add("begin", 4 * S, offset=16, data=begin, const=True)
        a.add("end", 4 * S, offset=28, data=end, const=True)
        a.add("keys_out", 4 * S * k, offset=8, fill="random")
        a.add("vals_out", 4 * S * k, offset=20, fill=("00", "ff", "random")[i])
        a.add("counts", 4 * S, offset=36, fill="random", const=(i == 2))
        a.add("temp", nb, offset=(1, 7, 130)[i], fill="random")
        a.build()
        rc = call(gs, a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in") if mode == PAIRS else None, a.ptr("keys_out"),
                  a.ptr("vals_out") if hv else None, None if i == 2 else a.ptr("counts"), n, S, a.ptr("begin"), a.ptr("end"), k, desc, kt)
        assert rc == 0
        a.check()
        assert status_of(gs, a.ptr("temp"), n, S, k, hv) == AR.status(begin, end, n)
        ek, ev, ec = AR.seg_topk(keys, begin, end, k, kt, desc, vals if mode == PAIRS else None)
        if i != 2:
            assert np.array_equal(a.read("counts", np.uint32), ec)
        written = (np.arange(k)[None, :] < ec[:, None])
        gk, ik = a.read("keys_out", np.uint32).reshape(S, k), a.init["keys_out"].view(np.uint32).reshape(S, k)
        assert np.array_equal(gk, np.where(written, ek, ik)), (mode, lens, k)
        gv, iv = a.read("vals_out", np.uint32).reshape(S, k), a.init["vals_out"].view(np.uint32).reshape(S, k)
        assert np.array_equal(gv, np.where(written, ev, iv) if hv else iv), (mode, lens, k)


def test_refused_calls_write_nothing(gs, cuda):
    n, S, k = 20000, 3, 2000
    nb = gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, 1)
    a = Arena(cuda, all_const=True)
    a.add("keys_in", 4 * n, fill="random").add("keys_out", 4 * S * k, fill="random").add("vals_out", 4 * S * k, fill="random")
    a.add("counts", 4 * S, fill="random").add("begin", 4 * S, data=np.array([0, 100, 2000], np.int32))
    a.add("end", 4 * S, data=np.array([100, 2000, 20000], np.int32)).add("temp", nb, fill="random").build()

    def refused(**kw):
        p = dict(temp=a.ptr("temp"), nb=nb, kin=a.ptr("keys_in"), kout=a.ptr("keys_out"), vout=a.ptr("vals_out"), counts=a.ptr("counts"),
                 n=n, S=S, begin=a.ptr("begin"), end=a.ptr("end"), k=k, kt=0)
        p.update(kw)
        return call(gs, p["temp"], p["nb"], p["kin"], None, p["kout"], p["vout"], p["counts"], p["n"], p["S"], p["begin"], p["end"],
                    p["k"], 0, p["kt"])
    for kw in (dict(nb=nb - 1), dict(temp=None), dict(k=1 << 30), dict(n=1 << 31), dict(kt=5), dict(begin=None), dict(end=None),
               dict(kout=a.ptr("keys_in") + 4), dict(vout=a.ptr("keys_out") + 4 * (S * k - 1)), dict(kin=a.ptr("keys_in") + 2),
               dict(counts=a.ptr("begin")), dict(counts=a.ptr("keys_out"))):
        assert refused(**kw) == 1, kw
    a.check()


def test_two_different_calls_on_one_workspace_and_identical_bytes(gs, cuda):
    """A ragged pairs call with long segments, a keys call on other offsets and the first one again, on one stream and one
    workspace without a synchronisation between them: the third call's bytes equal the first's."""
    lens_a, ka = [2 * CH + 9, 300, 5000, 5 * CH + 3, 40], 3000
    begin_a, end_a, na = AR.packed(lens_a)
    a = Case(gs, cuda, flat_keys(na, F32, seed=110), begin_a, end_a)
    begin_b, end_b, nb_items = AR.packed([5000, 77, CH + 1, 1])
    b = Case(gs, cuda, flat_keys(nb_items, I32, seed=111), begin_b, end_b)
    kb_ = 1200
    nb = max(need_bytes(gs, na, a.S, ka, 1), need_bytes(gs, nb_items, b.S, kb_, 0))
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    outs = [tuple(torch.full((a.S * ka,), -1, dtype=torch.int32, device=cuda) for _ in range(2)) +
            (torch.full((a.S,), -1, dtype=torch.int32, device=cuda),) for _ in range(2)]
    kb = torch.full((b.S * kb_,), -1, dtype=torch.int32, device=cuda)

    def run_a(ko, vo, co):
        assert call(gs, temp.data_ptr(), nb, a.d_keys.data_ptr(), a.d_vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), co.data_ptr(), na, a.S,
                    a.d_begin.data_ptr(), a.d_end.data_ptr(), ka, 1, F32) == 0
    run_a(*outs[0])
    assert call(gs, temp.data_ptr(), nb, b.d_keys.data_ptr(), None, kb.data_ptr(), None, None, nb_items, b.S, b.d_begin.data_ptr(),
                b.d_end.data_ptr(), kb_, 0, I32) == 0
    run_a(*outs[1])
    torch.cuda.synchronize()
    assert status_of(gs, temp.data_ptr(), na, a.S, ka, 1) == a.status
    ek, ev, ec = a.expect(ka, F32, True, PAIRS)
    assert np.array_equal(host(outs[0][0]).reshape(a.S, ka), ek) and np.array_equal(host(outs[0][1]).reshape(a.S, ka), ev)
    assert np.array_equal(host(outs[0][2]), ec)
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert np.array_equal(host(kb).reshape(b.S, kb_), b.expect(kb_, I32, False, KEYS)[0])


def test_capturable_in_a_hip_graph(gs, cuda):
    """A mixed-class shape captured once on one plain side stream (no parallel branches), replayed twice on new data in the same
    buffers."""
    lens, k = [3 * CH + 1, 500, 2 * CH, 3000, 0, 60], 2500
    begin, end, n = AR.packed(lens, gap=2)
    S = len(lens)
    sets = [flat_keys(n, U32, seed=120 + i, kinds=[kind]) for i, kind in enumerate(("uniform", "topbyte", "five"))]
    src, d_begin, d_end = dev(sets[0], cuda), dev(begin, cuda), dev(end, cuda)
    ko = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
    vo = torch.full((S * k,), -1, dtype=torch.int32, device=cuda)
    co = torch.full((S,), -1, dtype=torch.int32, device=cuda)
    D = gs.DeviceTopKSegmentedAnyK
    nb = D.MaxPairs(None, 0, None, None, None, None, None, n, S, None, None, k)
    assert D.Plan(n, S, k, True) == AR.plan(n, S, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_U32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        D.MaxPairs(temp, nb, src, ko, None, vo, co, n, S, d_begin, d_end, k, key_type=gs.GS_KEY_U32)
    for keys in sets[1:]:
        src.copy_(dev(keys, cuda))
        ko.fill_(-1)
        vo.fill_(-1)
        co.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ek, ev, ec = AR.seg_topk(keys, begin, end, k, U32, True)
        assert np.array_equal(host(ko).reshape(S, k), ek) and np.array_equal(host(vo).reshape(S, k), ev)
        assert np.array_equal(host(co), ec)
        assert D.Status(temp, n, S, k, True, stream=side) == AR.status(begin, end, n)     # the state block is zeroed in every replay


# ------------------------------------------------------------------------------------------------ cross-checks --
@pytest.mark.parametrize("rows,cols", [(5, CH), (5, 20000)])
def test_regular_offsets_equal_topk_rows_anyk(gs, cuda, rows, cols):
    k = 3000
    begin = (np.arange(rows) * cols).astype(np.int32)
    for i, mode in enumerate(MODES):
        kt, desc = (F32, U32, I32)[i], bool((i + 1) % 2)
        c = Case(gs, cuda, flat_keys(rows * cols, kt, seed=130 + i), begin, begin + cols)
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_rows_anyk_temp_bytes(rows, cols, k, hv)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
        vo = torch.full((rows * k,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_rows_anyk_u32(temp.data_ptr(), nb, c.d_keys.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None,
                                            ko.data_ptr(), vo.data_ptr() if hv else None, rows, cols, cols, k, int(desc), kt, None) == 0
        _, gk, gv, _ = c.run(k, kt, desc, mode)
        assert np.array_equal(gk[:rows * k], host(ko)) and (not hv or np.array_equal(gv[:rows * k], host(vo)))
        c.check(k, kt, desc, mode)


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_small_k_equals_the_capped_call(gs, cuda, k):
    lens = [0, 5, 64, 65, 300, 600, 1024, 1025, 5000, CH, CH + 1, 3 * CH + 7, 40]
    begin, end, n = AR.packed(lens, gap=3)
    for i, mode in enumerate(MODES):
        kt, desc = (I32, F32, U32)[i], bool(i % 2)
        c = Case(gs, cuda, flat_keys(n, kt, seed=140 + i), begin, end)
        hv = int(mode != KEYS)
        S = c.S
        nb = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
        ko = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=cuda)
        vo = torch.full((S * k + TAIL,), -1, dtype=torch.int32, device=cuda)
        co = torch.full((S + TAIL,), -1, dtype=torch.int32, device=cuda)
        assert gs.lib.gs_topk_segmented_u32(temp.data_ptr(), nb, c.d_keys.data_ptr(), c.d_vals.data_ptr() if mode == PAIRS else None,
                                            ko.data_ptr(), vo.data_ptr() if hv else None, co.data_ptr(), n, S, c.d_begin.data_ptr(),
                                            c.d_end.data_ptr(), k, int(desc), kt, None) == 0
        st, gk, gv, gc = c.run(k, kt, desc, mode)
        assert st == gs.DeviceTopKSegmented.Status(temp, n, S, k, hv)
        assert np.array_equal(gk, host(ko)) and np.array_equal(gv, host(vo)) and np.array_equal(gc, host(co))
        c.check(k, kt, desc, mode)


def test_front_end_against_torch_sort(gs, cuda):
    rng = np.random.default_rng(17)
    lens = [0, 1, 5, 100, 1000, 3000, CH + 50, 20000, 64]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n = int(offsets[-1])
    x = torch.from_numpy(rng.integers(-50, 50, n).astype(np.float32)).to(cuda)        # NaN-free, with many ties
    off = torch.from_numpy(offsets).to(cuda)
    vals = torch.arange(n, dtype=torch.int32, device=cuda) * 3
    for k in (1, 1500, 25000):
        for largest in (False, True):
            ko, io, counts = gs.topk_segmented_anyk(x, off, k, largest=largest, indices=True)
            k2, none, c2 = gs.topk_segmented_anyk(x, off[:-1].contiguous(), k, largest=largest, end_offsets=off[1:].contiguous())
            k3, v3, _ = gs.topk_segmented_anyk(x, off, k, largest=largest, values=vals)
            assert tuple(ko.shape) == (len(lens), k) and ko.dtype == x.dtype and io.dtype == torch.int32 and counts.dtype == torch.int32
            assert none is None and torch.equal(counts, c2)
            assert counts.tolist() == [min(k, ln) for ln in lens]
            for s, ln in enumerate(lens):
                kept = min(k, ln)
                if kept == 0:
                    continue
                seg = x[offsets[s]:offsets[s + 1]]
                want = torch.sort(seg, stable=True, descending=largest)
                assert torch.equal(ko[s, :kept], want.values[:kept]) and torch.equal(io[s, :kept].long(), want.indices[:kept]), (s, k, largest)
                assert torch.equal(k2[s, :kept], want.values[:kept]) and torch.equal(k3[s, :kept], want.values[:kept])
                assert torch.equal(v3[s, :kept].long(), (want.indices[:kept] + int(offsets[s])) * 3)
    with pytest.raises(ValueError):
        gs.topk_segmented(x, off, 1025)
    with pytest.raises(TypeError):
        gs.topk_segmented_anyk(x.double(), off, 1025)


def test_cpp_driver(gs):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "topk_segmented_anyk_check")
    assert os.path.exists(exe), "drivers not built (run __graft_entry__.build())"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-3000:] + out.stderr[-2000:]
    assert "FAIL" not in out.stdout and out.stdout.count("CORRECT") == 4 * 3 * 3


# ------------------------------------------------------------------------------------------------ seeded sweep --
@pytest.mark.parametrize("part", range(4))
def test_seeded_sweep(gs, cuda, part):
    """40 cases in four parts: random S <= 40, lengths log-uniform in [0, 40000], random k in [1, 45000], inputs from the
    campaign's generators; form, key type and direction rotate.  Long segments do not overlap, so nothing may be dropped."""
    per = AR.SWEEP_CASES // 4
    for index in range(part * per, (part + 1) * per):
        rng, begin, end, n, k = AR.sweep_case(index)
        kt, desc, mode = rotate(index)
        kind = TC.DISTS[int(rng.integers(0, len(TC.DISTS)))]
        keys = TC.make_keys(rng, kind, n, kt, desc).astype(np.uint32)
        c = Case(gs, cuda, keys, begin, end)
        assert c.status[7] == 0
        try:
            c.check(k, kt, desc, mode)
        except AssertionError as e:
            raise AssertionError("sweep seed %d case %d (%s, k=%d, S=%d, n=%d): %s" % (AR.SWEEP_SEED, index, kind, k, len(begin), n, e))
