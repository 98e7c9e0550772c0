"""The four stage calls of the bucket-sharded sort -- gs_shard_histogram_u32, gs_shard_partition_u32,
gs_msb_first_pass_u32, gs_msb_finish_u32 -- at every key type, layout and depth, on one GPU and in this process.

Raw gs.lib calls on buffers of an Arena (tests/guarded.py): every call's guard bands and const inputs are checked.  The
references, the crafted piece tables and the emulated sharded sort come from tests/shard_stages_ref.py (guarded on the
CPU by tests/test_shard_stages_cpu.py); every comparison is bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest

import shard_stages_ref as R
from guarded import Arena
from shard_stages_ref import U32, I32, F32, KEY_TYPES, KT_NAME

pytestmark = pytest.mark.gpu

INVALID = 1                     # hipErrorInvalidValue
WS_OFFSETS = (0, 1, 100, 255)   # the workspace may lie anywhere
_turn = itertools.count()


def _table(pieces):
    t = np.ascontiguousarray(pieces, dtype=np.uint64)
    return t, t.ctypes.data_as(C.c_void_p)


# --------------------------------------------------------------------------------------------------- histogram --
def _hist_call(gs, A, tag, bits, kt, n=None):
    return gs.lib.gs_shard_histogram_u32(A.ptr(tag + "k"), A.nbytes(tag + "k") // 4 if n is None else n, bits, A.ptr(tag + "h"), kt, None)


def _run_histograms(gs, cuda, calls, seed):
    """calls: (keys, kt, bits, element offset of the key pointer past a 16-byte boundary)"""
    A = Arena(cuda, seed=seed)
    for i, (keys, kt, bits, off) in enumerate(calls):
        A.add("c%dk" % i, 4 * keys.size, 4 * off, data=keys, const=True)
        A.add("c%dh" % i, 8 << bits, 8 * (i % 2), ("ff", "random")[i % 2])
    A.build()
    for i, (keys, kt, bits, off) in enumerate(calls):
        assert A.ptr("c%dk" % i) % 16 == 4 * off
        assert _hist_call(gs, A, "c%d" % i, bits, kt) == 0
    A.check()
    for i, (keys, kt, bits, off) in enumerate(calls):
        try:
            R.check_histogram(A.read("c%dh" % i, np.uint64), keys, kt, bits)
        except AssertionError as e:
            raise AssertionError("n=%d %s bits=%d offset=%d: %s" % (keys.size, KT_NAME[kt], bits, off, e)) from None


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("n", R.HIST_SIZES)
def test_histogram_every_size_offset_width_and_distribution(gs, cuda, n, kt):
    """Key pointer 0 to 3 elements past a 16-byte boundary (1 to 3: the scalar kernel), bits 1 / 8 / 11 / 12, three
    distributions, sizes around the vector width and the tile."""
    rng = np.random.default_rng([n, kt])
    calls = [(R.hist_keys(kt, dist, n, bits, rng), kt, bits, off) for off in range(4) for bits in R.HIST_BITS for dist in R.HIST_DISTS]
    assert len(calls) == 48
    _run_histograms(gs, cuda, calls, seed=n + kt)


@pytest.fixture(scope="module")
def large_bits():
    return np.random.default_rng(99).integers(0, 1 << 32, size=R.HIST_LARGE, dtype=np.uint32)


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
def test_histogram_at_the_grid_cap(gs, cuda, large_bits, kt):
    """2048 * 8192 + 3 * 8192 + 5 keys: the grid stops at 2048 workgroups, so in the aligned call the unrolled loop (two
    trips), the single-vector loop and the scalar tail all run; the same size through the scalar kernel, and with every
    key in one bin."""
    rng = np.random.default_rng(kt)
    keys = large_bits.copy()
    if kt == F32:
        R.sprinkle_specials(keys, rng)
    bits = (12, 11, 8)[kt]
    _run_histograms(gs, cuda, [(keys, kt, bits, 0)], seed=1)
    _run_histograms(gs, cuda, [(keys, kt, (1, 12, 11)[kt], 1 + kt)], seed=2)
    one = R.unmap((large_bits >> np.uint32(bits)) | np.uint32(((1 << bits) - 1 - kt) << (32 - bits)), kt)
    _run_histograms(gs, cuda, [(one, kt, bits, 0)], seed=3)


def test_histogram_refusals_touch_nothing_and_empty_input_zeroes(gs, cuda):
    keys = R.raw_keys(F32, 1000, np.random.default_rng(0))
    A = Arena(cuda, seed=5, all_const=True)
    A.add("k", 4 * keys.size, data=keys).add("h", 8 << 12, 0, "random").build()
    for bits, kt in ((0, U32), (13, U32), (-1, I32), (32, F32), (12, 3), (12, -1), (12, 13)):
        assert gs.lib.gs_shard_histogram_u32(A.ptr("k"), keys.size, bits, A.ptr("h"), kt, None) == INVALID, (bits, kt)
    assert gs.lib.gs_shard_histogram_u32(A.ptr("k"), keys.size, 12, None, U32, None) == INVALID
    A.check()
    for kt in KEY_TYPES:                      # no keys, no key pointer: a histogram of zeros
        for bits in R.HIST_BITS:
            B = Arena(cuda, seed=6)
            B.add("h", 8 << bits, 8, "random").build()
            assert gs.lib.gs_shard_histogram_u32(None, 0, bits, B.ptr("h"), kt, None) == 0
            B.check()
            assert not B.read("h", np.uint64).any()


# --------------------------------------------------------------------------------------------------- partition --
@pytest.mark.parametrize("si", range(len(R.PART_SIZES)), ids=["n%d" % n for n in R.PART_SIZES])
def test_partition_is_the_stable_reference(gs, cuda, si):
    """Every key type x pairs x bits x rank count at this size (R.partition_plan), the dest table's kind rotating: keys in
    the caller's representation, values and counts equal the stable reference exactly."""
    n = R.PART_SIZES[si]
    plan = R.partition_plan(si)
    vals = np.arange(n, dtype=np.uint32)
    for kt in KEY_TYPES:
        for pairs in (False, True):
            rng = np.random.default_rng([n, kt, int(pairs)])
            keys = R.raw_keys(kt, n, rng)
            todo = [c for c in plan if c[0] == kt and c[1] == pairs]
            assert len(todo) == len(R.PART_BITS) * len(R.PART_RANKS)
            off = 4 * ((si + kt) % 4)
            A = Arena(cuda, seed=si)
            A.add("kin", 4 * n, off, data=keys, const=True)
            if pairs:
                A.add("vin", 4 * n, off, data=vals, const=True)
            dests = []
            for i, (_, _, bits, ranks, kind) in enumerate(todo):
                dests.append(R.dest_table(kind, bits, ranks, rng))
                A.add("c%dkout" % i, 4 * n, off, "ff")
                if pairs:
                    A.add("c%dvout" % i, 4 * n, off, "random")
                A.add("c%ddest" % i, dests[i].size, i % 2, data=dests[i], const=True)
                A.add("c%dcounts" % i, 8 * ranks, 8 * (i % 2), "random")
            q = gs.lib.gs_msb_temp_bytes(n, int(pairs))
            A.add("ws", q, WS_OFFSETS[(si + kt) % 4], "random").build()
            for i, (_, _, bits, ranks, kind) in enumerate(todo):
                rc = gs.lib.gs_shard_partition_u32(A.ptr("ws"), q, A.ptr("kin"), A.ptr("c%dkout" % i), A.ptr("vin") if pairs else None,
                                                   A.ptr("c%dvout" % i) if pairs else None, n, bits, A.ptr("c%ddest" % i), ranks, None,
                                                   A.ptr("c%dcounts" % i), kt, None)
                assert rc == 0, (todo[i], rc)
            A.check()
            for i, (_, _, bits, ranks, kind) in enumerate(todo):
                try:
                    R.check_partition(A.read("c%dkout" % i, np.uint32), A.read("c%dvout" % i, np.uint32) if pairs else None,
                                      A.read("c%dcounts" % i, np.uint64), keys, vals if pairs else None, kt, bits, dests[i], ranks)
                except AssertionError as e:
                    raise AssertionError("n=%d %s pairs=%s bits=%d ranks=%d dest=%s: %s" % (n, KT_NAME[kt], pairs, bits, ranks, kind, e)) from None


def test_partition_table_reaches_every_combination():
    want = {(kt, p, b, r) for kt in KEY_TYPES for p in (False, True) for b in R.PART_BITS for r in R.PART_RANKS}
    seen = set()
    for si in range(len(R.PART_SIZES)):
        plan = R.partition_plan(si)
        assert {c[:4] for c in plan} == want
        seen |= set(plan)
    assert len(want) == 90 and seen == {c + (k,) for c in want for k in R.DEST_KINDS}


# ------------------------------------------------------------------------------------ finish on crafted tables --
def _finish_bytes(gs, L, pairs):
    return gs.lib.gs_msb_finish_temp_bytes(L.keys.size, int(pairs), L.num_src)


def _run_finishes(gs, cuda, calls, seed=0, synchronize=1):
    """calls: (Layout, kt, pairs).  Every call gets its own receive and output buffers; all share one workspace, sized for
    the largest query and used one call behind the other on the stream."""
    A = Arena(cuda, seed=seed)
    t = next(_turn)
    off = 4 * (t % 4)
    for i, (L, kt, pairs) in enumerate(calls):
        n = L.keys.size
        A.add("c%drk" % i, 4 * n, off, data=L.keys).add("c%dok" % i, 4 * n, off, ("ff", "random")[i % 2])
        if pairs:
            A.add("c%drv" % i, 4 * n, off, data=np.arange(n, dtype=np.uint32)).add("c%dov" % i, 4 * n, off, ("random", "ff")[i % 2])
    q = max(_finish_bytes(gs, L, pairs) for L, kt, pairs in calls)
    A.add("ws", q, WS_OFFSETS[t % 4], ("ff", "random")[t % 2]).build()
    for i, (L, kt, pairs) in enumerate(calls):
        tab, ptr = _table(L.pieces)
        rc = gs.lib.gs_msb_finish_u32(A.ptr("ws"), _finish_bytes(gs, L, pairs), A.ptr("c%drk" % i), A.ptr("c%drv" % i) if pairs else None,
                                      A.ptr("c%dok" % i), A.ptr("c%dov" % i) if pairs else None, L.keys.size, ptr, L.num_src, kt, None,
                                      synchronize)
        assert rc == 0, (L.name, KT_NAME[kt], pairs, rc)
    A.check()
    for i, (L, kt, pairs) in enumerate(calls):
        try:
            R.check_finish(A.read("c%dok" % i, np.uint32), A.read("c%dov" % i, np.uint32) if pairs else None, L.keys,
                           np.arange(L.keys.size, dtype=np.uint32) if pairs else None, kt)
        except AssertionError as e:
            raise AssertionError("%s %s pairs=%s: %s" % (L.name, KT_NAME[kt], pairs, e)) from None


VARIANTS = [(kt, pairs) for kt in KEY_TYPES for pairs in (False, True)]


@pytest.mark.parametrize("which", ["full_table", "full_column", "one_source"])
def test_finish_with_256_sources(gs, cuda, which):
    """All 65536 pieces non-empty; one bucket in every one of 256 sources; one source of 256 holding everything."""
    L = {"full_table": R.layout_full_table, "full_column": R.layout_full_column, "one_source": R.layout_one_source}[which](np.random.default_rng(11))
    assert L.num_src == 256
    _run_finishes(gs, cuda, [(L, kt, pairs) for kt, pairs in VARIANTS], seed=1)


@pytest.mark.parametrize("size", R.THRESHOLD_SIZES)
def test_finish_pieces_at_the_tile_and_alignment_thresholds(gs, cuda, size):
    """One piece of `size` keys starting at (offset & 63) of 0, 1 and 63, a second bucket behind it: sizes around one tile and
    around the 16 tiles from which an unaligned piece gets a short first tile."""
    calls = []
    for start in R.THRESHOLD_STARTS:
        L = R.layout_threshold(np.random.default_rng([size, start]), size, start)
        calls += [(L, kt, pairs) for kt, pairs in VARIANTS]
    _run_finishes(gs, cuda, calls, seed=size)


@pytest.mark.parametrize("equal", [False, True], ids=["low_bytes_differ", "all_equal"])
def test_finish_a_pieced_bucket_through_every_level(gs, cuda, equal):
    """40 000 keys that share their top 24 bits, in 3 pieces: the pieced level 1 and levels 2 and 3 all partition it."""
    L = R.layout_depth(np.random.default_rng(12), equal)
    _run_finishes(gs, cuda, [(L, kt, pairs) for kt, pairs in VARIANTS], seed=2)


def test_finish_a_heavy_hitter_behind_a_pieced_level(gs, cuda):
    """Keys only: 60 000 keys in 4 pieces, one key holding 0.9 of them; level 2 meets the heavy hitter."""
    L = R.layout_heavy(np.random.default_rng(13))
    _run_finishes(gs, cuda, [(L, kt, False) for kt in KEY_TYPES], seed=3)
    _run_finishes(gs, cuda, [(L, kt, False) for kt in KEY_TYPES], seed=4, synchronize=0)


def test_finish_empty_and_tiny(gs, cuda):
    rng = np.random.default_rng(14)
    for total in (1, 2):
        _run_finishes(gs, cuda, [(R.layout_tiny(rng, total), kt, pairs) for kt, pairs in VARIANTS], seed=total)
        _run_finishes(gs, cuda, [(R.layout_tiny(rng, total, num_src=256), kt, pairs) for kt, pairs in VARIANTS], seed=total)
    L = R.layout_tiny(rng, 0)
    q = gs.lib.gs_msb_finish_temp_bytes(0, 1, L.num_src)
    A = Arena(cuda, seed=9, all_const=True)
    for name in ("rk", "rv", "ok", "ov"):
        A.add(name, 64, 0, "random")
    A.add("ws", q, 0, "random").build()
    tab, ptr = _table(L.pieces)
    for kt, pairs in VARIANTS:
        assert gs.lib.gs_msb_finish_u32(A.ptr("ws"), q, A.ptr("rk"), A.ptr("rv") if pairs else None, A.ptr("ok"),
                                        A.ptr("ov") if pairs else None, 0, ptr, L.num_src, kt, None, 1) == 0
        assert gs.lib.gs_msb_finish_u32(None, 0, None, None, None, None, 0, ptr, L.num_src, kt, None, 0) == 0
    A.check()


def test_finish_refusals_write_nothing(gs, cuda):
    L = R.layout_threshold(np.random.default_rng(15), 8193, 1)
    n = L.keys.size
    big = np.zeros((257, 256), np.uint64)
    big[:2] = L.pieces
    for pairs in (False, True):
        q = _finish_bytes(gs, L, pairs)
        q257 = gs.lib.gs_msb_finish_temp_bytes(n, int(pairs), 257)
        A = Arena(cuda, seed=10, all_const=True)
        A.add("rk", 4 * n, data=L.keys).add("ok", 4 * n, 0, "random")
        A.add("rv", 4 * n, data=np.arange(n, dtype=np.uint32)).add("ov", 4 * n, 0, "random")
        A.add("ws", max(q, q257), 0, "random").add("short", q - 1, 1, "random").build()

        def call(ws, nbytes, num_items, table, num_src, kt=F32):
            tab, ptr = _table(table)
            return gs.lib.gs_msb_finish_u32(A.ptr(ws), nbytes, A.ptr("rk"), A.ptr("rv") if pairs else None, A.ptr("ok"),
                                            A.ptr("ov") if pairs else None, num_items, ptr, num_src, kt, None, 1)
        assert call("ws", q, n - 1, L.pieces, 2) == INVALID            # the table adds up to more than num_items
        assert call("ws", q, n + 1, L.pieces, 2) == INVALID            # ... to less
        less = L.pieces.copy()
        less[1][0xFF] -= 1
        assert call("ws", q, n, less, 2) == INVALID
        assert call("ws", q, n, big, 0) == INVALID
        assert call("ws", q257, n, big, 257) == INVALID
        assert call("ws", q, n, big, -1) == INVALID
        assert call("short", q - 1, n, L.pieces, 2) == INVALID         # one byte short of the query
        assert call("ws", q, n, L.pieces, 2, kt=3) == INVALID
        assert gs.lib.gs_msb_finish_u32(A.ptr("ws"), q, A.ptr("rk"), None, A.ptr("ok"), None, n, None, 2, U32, None, 1) == INVALID
        A.check()


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs"])
def test_two_finishes_share_one_workspace_on_slices_of_one_buffer(gs, cuda, kt, pairs):
    """The per-group calls of sharded.py: two finishes enqueued back to back on one stream, one workspace, each on a
    pointer-offset slice of one receive and one output buffer, its table zero outside its own buckets.  Both slices are
    right, and the elements between and around them are untouched."""
    G = R.layout_groups(np.random.default_rng([16, kt]))
    gap = 67                                        # elements no call owns, between the two slices
    n0, n1 = G[0].keys.size, G[1].keys.size
    at = [0, n0 + gap]
    total = n0 + gap + n1
    recv = np.full(total, 0xA5A5A5A5, np.uint32)
    recv[:n0], recv[at[1]:] = G[0].keys, G[1].keys
    labels = np.arange(total, dtype=np.uint32)
    A = Arena(cuda, seed=11)
    A.add("rk", 4 * total, 4, data=recv).add("ok", 4 * total, 4, "random")
    if pairs:
        A.add("rv", 4 * total, 4, data=labels).add("ov", 4 * total, 4, "random")
    q = max(_finish_bytes(gs, L, pairs) for L in G)
    A.add("ws", q, 255, "random").build()
    keep = [_table(L.pieces) for L in G]            # the tables are read before each call returns; kept alive all the same
    for g, L in enumerate(G):
        o = 4 * at[g]
        rc = gs.lib.gs_msb_finish_u32(A.ptr("ws"), q, A.ptr("rk") + o, A.ptr("rv") + o if pairs else None, A.ptr("ok") + o,
                                      A.ptr("ov") + o if pairs else None, L.keys.size, keep[g][1], L.num_src, kt, None, 0)
        assert rc == 0
    A.check()
    ok, ov = A.read("ok", np.uint32), (A.read("ov", np.uint32) if pairs else None)
    for g, L in enumerate(G):
        sl = slice(at[g], at[g] + L.keys.size)
        R.check_finish(ok[sl], ov[sl] if pairs else None, L.keys, labels[sl] if pairs else None, kt)
    between = slice(n0, n0 + gap)
    assert np.array_equal(ok[between], A.init["ok"].view(np.uint32)[between]), "an output element between the slices was written"
    if pairs:
        assert np.array_equal(ov[between], A.init["ov"].view(np.uint32)[between]), "an output value between the slices was written"
        assert np.array_equal(A.read("rv", np.uint32)[between], labels[between])
    assert np.all(A.read("rk", np.uint32)[between] == 0xA5A5A5A5), "a received element between the slices was written"


# ------------------------------------------------------------------------------------ the emulated sharded sort --
def gpu_ops(gs, cuda):
    """The four calls on numpy arrays, each in an Arena of its own (guards and const inputs checked)."""
    def first_pass(keys, vals, kt):
        n, pairs, t = keys.size, vals is not None, next(_turn)
        off = 4 * (t % 4)
        A = Arena(cuda, seed=t)
        A.add("kin", 4 * n, off, data=keys, const=True).add("kout", 4 * n, off, "ff")
        if pairs:
            A.add("vin", 4 * n, off, data=vals, const=True).add("vout", 4 * n, off, "random")
        q = gs.lib.gs_lsb_temp_bytes(n, int(pairs))
        A.add("counts", 8 * 256, 8 * (t % 2), "random").add("ws", q, WS_OFFSETS[t % 4], "random").build()
        rc = gs.lib.gs_msb_first_pass_u32(A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if pairs else None,
                                          A.ptr("vout") if pairs else None, n, kt, A.ptr("counts"), None)
        assert rc == 0, rc
        A.check()
        return A.read("kout", np.uint32), (A.read("vout", np.uint32) if pairs else None), A.read("counts", np.uint64)

    def finish(recv_k, recv_v, pieces, kt):
        n, pairs, t = recv_k.size, recv_v is not None, next(_turn)
        off = 4 * (t % 4)
        tab, ptr = _table(pieces)
        A = Arena(cuda, seed=t)
        A.add("rk", 4 * n, off, data=recv_k).add("ok", 4 * n, off, "random")
        if pairs:
            A.add("rv", 4 * n, off, data=recv_v).add("ov", 4 * n, off, "ff")
        q = gs.lib.gs_msb_finish_temp_bytes(n, int(pairs), tab.shape[0])
        A.add("ws", q, WS_OFFSETS[t % 4], "random").build()
        rc = gs.lib.gs_msb_finish_u32(A.ptr("ws"), q, A.ptr("rk"), A.ptr("rv") if pairs else None, A.ptr("ok"),
                                      A.ptr("ov") if pairs else None, n, ptr, tab.shape[0], kt, None, t % 2)
        assert rc == 0, rc
        A.check()
        return A.read("ok", np.uint32), (A.read("ov", np.uint32) if pairs else None)

    def histogram(keys, kt, bits):
        t = next(_turn)
        A = Arena(cuda, seed=t)
        A.add("k", 4 * keys.size, 4 * (t % 4), data=keys, const=True).add("h", 8 << bits, 0, "random").build()
        assert _hist_call(gs, A, "", bits, kt) == 0
        A.check()
        return A.read("h", np.uint64)

    def partition(keys, vals, kt, bits, dest, ranks):
        n, pairs, t = keys.size, vals is not None, next(_turn)
        off = 4 * (t % 4)
        A = Arena(cuda, seed=t)
        A.add("kin", 4 * n, off, data=keys, const=True).add("kout", 4 * n, off, "random")
        if pairs:
            A.add("vin", 4 * n, off, data=vals, const=True).add("vout", 4 * n, off, "ff")
        q = gs.lib.gs_msb_temp_bytes(n, int(pairs))
        A.add("dest", dest.size, t % 2, data=dest, const=True).add("counts", 8 * ranks, 0, "random")
        A.add("ws", q, WS_OFFSETS[t % 4], "random").build()
        rc = gs.lib.gs_shard_partition_u32(A.ptr("ws"), q, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if pairs else None,
                                           A.ptr("vout") if pairs else None, n, bits, A.ptr("dest"), ranks, None, A.ptr("counts"), kt, None)
        assert rc == 0, rc
        A.check()
        return A.read("kout", np.uint32), (A.read("vout", np.uint32) if pairs else None), A.read("counts", np.uint64)

    return {"first_pass": first_pass, "finish": finish, "histogram": histogram, "partition": partition}


@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs"])
@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("world", R.WORLDS)
def test_emulated_sharded_sort(gs, cuda, world, kt, pairs):
    """First pass, split, exchange layout and finish composed for every rank of `world`, with the caller's key type in
    both device calls: the ranks' outputs one behind the other are the global sort bit for bit, every rank holds
    per_rank keys, the first pass's keys, values and counts equal the reference."""
    ops = gpu_ops(gs, cuda)
    for name in R.sharded_inputs(kt):
        shards = R.sharded_shards(name, kt, world)
        try:
            res = R.emulate_sharded_sort(shards, kt, pairs, world, ops)
            R.check_sharded(res, shards, kt, pairs, world)
        except AssertionError as e:
            raise AssertionError("input %s: %s" % (name, e)) from None


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("world", [3, 8])
def test_emulated_partition_pipeline(gs, cuda, world, kt):
    """The fallback's stages composed the same way: histogram and partition with the caller's key type on 12 bits."""
    ops = gpu_ops(gs, cuda)
    for name, pairs in (("uniform", True), ("hot_key", False), ("uneven", True)):
        shards = R.sharded_shards(name, kt, world)
        res = R.emulate_sharded_sort(shards, kt, pairs, world, ops, pipeline="partition")
        R.check_sharded(res, shards, kt, pairs, world, pipeline="partition")
