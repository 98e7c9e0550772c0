"""Guards tests/shard_stages_ref.py, the reference and the case generators of tests/test_shard_stages_gpu.py: the emulated
sharded sort with numpy stand-ins for the four stage calls gives the global sort; every generated layout has the
property its name claims; the checkers fail on a wrong result.  No GPU."""
import numpy as np
import pytest

import shard_stages_ref as R
from shard_stages_ref import I32, F32, KEY_TYPES, KT_NAME


# ------------------------------------------------------------------------------------------------------ the map --
@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
def test_ordmap_is_monotone_and_unmap_inverts_it(kt):
    rng = np.random.default_rng(kt)
    raw = np.concatenate([R.raw_keys(kt, 20000, rng), R.F32_SPECIALS, np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)])
    m = R.ordmap(raw, kt)
    assert m.dtype == np.uint32 and np.array_equal(R.unmap(m, kt), raw)
    assert np.array_equal(R.ordmap(R.unmap(m, kt), kt), m)
    order = np.argsort(m, kind="stable")
    if kt == I32:
        assert np.all(np.diff(raw[order].view(np.int32).astype(np.int64)) >= 0)
    if kt == F32:
        f = raw[order].view(np.float32)
        num = f[~np.isnan(f)]
        assert np.all(num[1:] >= num[:-1])                                      # numbers in numeric order
        z = np.nonzero(num == 0)[0]
        assert np.all(np.diff(np.signbit(num[z]).astype(int)) <= 0)             # -0.0 before +0.0
        assert np.isnan(f[0]) and np.isnan(f[-1])                               # NaNs by their bits: at both ends
    assert R.ordmap(np.array([0x80000000], np.uint32), I32)[0] == 0
    assert R.ordmap(np.array([0x80000000], np.uint32), F32)[0] == 0x7FFFFFFF    # -0.0
    assert R.ordmap(np.array([0], np.uint32), F32)[0] == 0x80000000             # +0.0
    assert R.ordmap(np.array([0xFFC12345], np.uint32), F32)[0] == 0x003EDCBA    # a negative NaN with a payload


def test_the_specials_cover_what_the_issue_names():
    f = R.F32_SPECIALS.view(np.float32)
    assert {0x00000000, 0x80000000, 0x7F800000, 0xFF800000} <= set(int(x) for x in R.F32_SPECIALS)      # +-0, +-inf
    sub = (R.F32_SPECIALS & np.uint32(0x7F800000) == 0) & (R.F32_SPECIALS & np.uint32(0x007FFFFF) != 0)
    assert sub.sum() >= 2 and {bool(s) for s in np.signbit(f[sub])} == {True, False}                      # subnormals
    nan = np.isnan(f)
    assert {bool(s) for s in np.signbit(f[nan])} == {True, False}                                         # NaNs of both signs
    assert (R.F32_SPECIALS[nan] & np.uint32(0x003FFFFF) != 0).sum() >= 2                                  # with payloads
    assert set(int(x) >> 24 for x in R.MAPPED_SPECIALS) == {0x00, 0x7F, 0x80, 0xFF}
    for n in (200, R.SHARD_KEYS):
        assert R.has_f32_specials(R.raw_keys(F32, n, np.random.default_rng(n)))
    k = R.raw_keys(I32, 1000, np.random.default_rng(1)).view(np.int32)
    assert k.min() < 0 < k.max()


# --------------------------------------------------------------------------------------------- emulated sorting --
def _cases():
    return [(w, kt, p, name) for w in R.WORLDS for kt in KEY_TYPES for p in (False, True) for name in R.sharded_inputs(kt)]


@pytest.mark.parametrize("world,kt,pairs,name", _cases(),
                         ids=["w%d-%s-%s-%s" % (w, KT_NAME[kt], "pairs" if p else "keys", name) for w, kt, p, name in _cases()])
def test_emulation_with_numpy_stand_ins_is_the_global_sort(world, kt, pairs, name):
    shards = R.sharded_shards(name, kt, world)
    res = R.emulate_sharded_sort(shards, kt, pairs, world, R.numpy_ops())
    R.check_sharded(res, shards, kt, pairs, world)
    want = R.unmap(np.sort(R.ordmap(np.concatenate(shards), kt)), kt)
    at = 0
    for r in range(world):                                       # rank by rank
        c = int(res.per_rank[r])
        assert np.array_equal(res.out_k[r], want[at:at + c])
        at += c
    assert at == want.size


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("world", [3, 8])
def test_emulation_of_the_partition_pipeline(world, kt):
    for name in ("uniform", "hot_key"):
        shards = R.sharded_shards(name, kt, world)
        res = R.emulate_sharded_sort(shards, kt, True, world, R.numpy_ops(), pipeline="partition")
        R.check_sharded(res, shards, kt, True, world, pipeline="partition")


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
@pytest.mark.parametrize("world", R.WORLDS)
def test_sharded_inputs_are_what_their_names_say(world, kt):
    n = R.SHARD_KEYS
    for name in R.sharded_inputs(kt):
        shards = R.sharded_shards(name, kt, world)
        assert len(shards) == world and all(s.dtype == np.uint32 for s in shards)
        allk = np.concatenate(shards)
        m = R.ordmap(allk, kt)
        if name in ("uniform", "hot_key", "hot_byte", "sorted"):
            assert [s.size for s in shards] == [n] * world
            if kt == F32:
                assert R.has_f32_specials(allk), name
            if kt == I32:
                assert allk.view(np.int32).min() < 0 <= allk.view(np.int32).max(), name
        if name == "hot_key":
            for s in shards:
                assert np.bincount(np.unique(s, return_inverse=True)[1]).max() >= 0.88 * n
        if name == "hot_byte":
            for s in shards:
                assert np.bincount(R.ordmap(s, kt) >> np.uint32(24)).max() >= 0.78 * n
        if name == "all_equal":
            assert np.unique(allk).size == 1 and allk.size == n * world
        if name == "sorted":
            assert np.all(np.diff(m.astype(np.int64)) >= 0) and np.unique(m).size > n // 2
        if name == "f32_negative":
            assert np.all(allk & R.SIGN != 0) and np.isnan(allk.view(np.float32)).any() and (allk == 0x80000000).any()
        if name == "tiny":
            sizes = [s.size for s in shards]
            assert max(sizes) <= 5 and sum(sizes) > 0 and (world == 1 or 0 in sizes)
        if name == "uneven":
            sizes = [s.size for s in shards]
            assert world == 1 or max(sizes) >= 1000 * max(1, min(sizes))
    vals = R.shard_values(R.sharded_shards("uneven", kt, world))
    assert np.unique(np.concatenate(vals)).size == sum(v.size for v in vals)


# --------------------------------------------------------------------------------------------- crafted layouts --
def _layout_ok(L):
    """A layout's keys lie where its table says, with the top byte of their piece."""
    top = np.repeat(np.tile(np.arange(256, dtype=np.uint32), L.num_src), L.pieces.reshape(-1).astype(np.int64))
    assert np.array_equal(L.keys >> np.uint32(24), top) and L.keys.dtype == np.uint32


def test_full_table_column_and_single_source():
    rng = np.random.default_rng(1)
    L = R.layout_full_table(rng)
    _layout_ok(L)
    assert L.num_src == 256 and np.count_nonzero(L.pieces) == 65536 and L.pieces.min() >= 1 and L.pieces.max() <= 5
    assert 150000 < L.keys.size < 250000 and R.has_f32_specials(R.unmap(L.keys, F32))
    L = R.layout_full_column(rng)
    _layout_ok(L)
    assert L.num_src == 256 and np.all(L.pieces[:, L.meta["bucket"]] > 0) and np.count_nonzero(L.pieces) == 256
    L = R.layout_one_source(rng)
    _layout_ok(L)
    assert L.num_src == 256 and np.count_nonzero(L.pieces.sum(axis=1)) == 1 and np.count_nonzero(L.pieces[L.meta["src"]]) == 256
    assert R.has_f32_specials(R.unmap(L.keys, F32))


@pytest.mark.parametrize("size", R.THRESHOLD_SIZES)
def test_threshold_pieces_start_and_end_where_they_should(size):
    assert set(R.THRESHOLD_SIZES) == {8191, 8192, 8193, 16 * 8192 - 1, 16 * 8192, 16 * 8192 + 1, 17 * 8192 + 5}
    for start in R.THRESHOLD_STARTS:
        L = R.layout_threshold(np.random.default_rng(size + start), size, start)
        _layout_ok(L)
        s, b = L.meta["piece"]
        off = int(R.piece_offsets(L.pieces)[s][b])
        assert off & 63 == start and off == L.meta["offset"] and int(L.pieces[s][b]) == size
        assert np.count_nonzero(L.pieces[:, b]) == 2                       # the bucket arrives in pieces
        nxt = np.nonzero(L.pieces.sum(axis=0))[0]
        assert nxt[list(nxt).index(b) + 1] == b + 1                         # a second bucket follows the ragged one
        ragged = start != 0 and size >= 16 * 8192                           # only then the first tile is the short one
        assert R.piece_tiles(off, size) == (1 + -(-(size - (8192 - start)) // 8192) if ragged else -(-size // 8192))
        assert R.has_f32_specials(R.unmap(L.keys, F32))
    assert R.piece_tiles(1, 16 * 8192 - 1) == 16 and R.piece_tiles(1, 16 * 8192) == 17 and R.piece_tiles(64, 16 * 8192) == 16
    assert R.piece_tiles(2, 17 * 8192 - 1) == 18                            # short at both ends


def test_depth_and_heavy_hitter_buckets():
    for equal in (False, True):
        L = R.layout_depth(np.random.default_rng(2), equal)
        _layout_ok(L)
        assert L.keys.size == R.DEPTH_KEYS == 40000 > R.LOCAL_SORT_MAX == 17408
        assert np.count_nonzero(L.pieces) == 3 and np.count_nonzero(L.pieces.sum(axis=1)) == 3
        assert np.unique(L.keys >> np.uint32(8)).size == 1                  # more than 17408 keys share their top 24 bits
        assert np.unique(L.keys).size == (1 if equal else 256)
        # as F32: -0.0, and negative subnormals where the keys differ
        assert ({0x80000000} if equal else {0x80000000, 0x80000001, 0x80000003}) <= set(int(x) for x in R.unmap(L.keys, F32))
    L = R.layout_heavy(np.random.default_rng(3))
    _layout_ok(L)
    assert L.keys.size == 60000 and np.count_nonzero(L.pieces) == 4 and np.count_nonzero(L.pieces.sum(axis=0)) == 1
    share = float((L.keys == L.meta["key"]).mean())
    assert 0.88 < share < 0.92
    below, above = int((L.keys < L.meta["key"]).sum()), int((L.keys > L.meta["key"]).sum())
    assert below <= R.LOCAL_SORT_MAX and above <= R.LOCAL_SORT_MAX          # the strangers on each side fit a local sort
    assert np.unique(L.keys >> np.uint32(16)).size > 200                    # ... and spread over level 1's digit


def test_tiny_and_group_layouts():
    for total in (0, 1, 2):
        L = R.layout_tiny(np.random.default_rng(total), total)
        _layout_ok(L)
        assert L.keys.size == total and L.num_src == 3
    groups = R.layout_groups(np.random.default_rng(4))
    assert len(groups) == 2
    for L in groups:
        _layout_ok(L)
        lo, hi = L.meta["buckets"]
        assert L.pieces[:, :lo].sum() == 0 and L.pieces[:, hi:].sum() == 0 and np.count_nonzero(L.pieces.sum(axis=1)) == 3


def test_histogram_and_partition_inputs():
    rng = np.random.default_rng(5)
    for kt in KEY_TYPES:
        for bits in (1, 8, 11, 12):
            h = R.ref_histogram(R.hist_keys(kt, "one_bin", 5000, bits, rng), kt, bits)
            assert h.size == 1 << bits and np.count_nonzero(h) == 1 and h.sum() == 5000
            h = R.ref_histogram(R.hist_keys(kt, "first_last", 5000, bits, rng), kt, bits)
            assert h[0] > 0 and h[-1] > 0 and h[0] + h[-1] == 5000
            h = R.ref_histogram(R.hist_keys(kt, "uniform", 50000, bits, rng), kt, bits)
            assert np.count_nonzero(h) > (1 << bits) // 2
    for bits in (1, 8, 12):
        for ranks in (1, 2, 3, 255, 256):
            for kind in R.DEST_KINDS:
                d = R.dest_table(kind, bits, ranks, rng)
                assert d.dtype == np.uint8 and d.size == 1 << bits and np.all(np.diff(d.astype(int)) >= 0) and int(d.max()) < ranks
                if kind == "all_last":
                    assert np.all(d == ranks - 1)
                if kind == "gaps" and ranks >= 3:
                    assert 0 not in d and np.unique(d).size <= ranks // 2 + 1
    assert np.unique(R.dest_table("random", 12, 256, rng)).size > 200
    assert np.unique(R.dest_table("gaps", 12, 256, rng)).size > 100


def test_partition_plan_reaches_every_combination():
    assert R.PART_SIZES == (1, 8191, 8192, 8193, 65535, 65536, 65537, 100003) and R.HIST_LARGE == 2048 * 8192 + 3 * 8192 + 5
    want = {(kt, p, b, r) for kt in KEY_TYPES for p in (False, True) for b in (1, 8, 12) for r in (1, 2, 3, 255, 256)}
    seen = set()
    for si in range(len(R.PART_SIZES)):
        plan = R.partition_plan(si)
        assert {c[:4] for c in plan} == want and len(plan) == len(want)          # every size runs every combination
        seen |= set(plan)
    assert seen == {c + (k,) for c in want for k in R.DEST_KINDS}                # and each meets every kind of table


# ----------------------------------------------------------------------------------- the checkers notice a fault --
def _flip(a, i):
    b = a.copy()
    b[i] ^= np.uint32(1 << 7)
    return b


def _swap(a, i, j):
    b = a.copy()
    b[i], b[j] = a[j], a[i]
    return b


def _bump(c, i=0):
    d = c.copy()
    d[i] += np.uint64(1)
    return d


@pytest.mark.parametrize("kt", KEY_TYPES, ids=KT_NAME.get)
def test_checkers_fail_on_a_flipped_bit_swapped_values_and_a_count_off_by_one(kt):
    rng = np.random.default_rng(7 + kt)
    n = 5000
    keys, vals = R.raw_keys(kt, n, rng), np.arange(n, dtype=np.uint32)
    # histogram
    h = R.ref_histogram(keys, kt, 12)
    R.check_histogram(h, keys, kt, 12)
    with pytest.raises(AssertionError):
        R.check_histogram(_bump(h, 77), keys, kt, 12)
    # partition
    dest = R.dest_table("random", 8, 3, rng)
    pk, pv, pc = R.ref_partition(keys, vals, kt, 8, dest, 3)
    R.check_partition(pk, pv, pc, keys, vals, kt, 8, dest, 3)
    for bad in ((_flip(pk, 100), pv, pc), (pk, _swap(pv, 10, 11), pc), (pk, pv, _bump(pc)), (_swap(pk, 10, 11), _swap(pv, 10, 11), pc)):
        with pytest.raises(AssertionError):
            R.check_partition(*bad, keys, vals, kt, 8, dest, 3)
    # first pass
    gk, gv, gc = R.ref_first_pass(keys, vals, kt)
    R.check_first_pass(gk, gv, gc, keys, vals, kt)
    for bad in ((_flip(gk, 100), gv, gc), (gk, _swap(gv, 10, 11), gc), (gk, gv, _bump(gc, 255))):
        with pytest.raises(AssertionError):
            R.check_first_pass(*bad, keys, vals, kt)
    # finish: equal keys may trade their values, different keys may not
    L = R.layout_threshold(rng, 8193, 1)
    fk, fv = R.numpy_ops()["finish"](L.keys, np.arange(L.keys.size, dtype=np.uint32), L.pieces, kt)
    labels = np.arange(L.keys.size, dtype=np.uint32)
    R.check_finish(fk, fv, L.keys, labels, kt)
    i = int(np.nonzero(fk[1:] != fk[:-1])[0][0])
    for bad in ((_flip(fk, 100), fv), (fk, _swap(fv, i, i + 1))):
        with pytest.raises(AssertionError):
            R.check_finish(*bad, L.keys, labels, kt)
    with pytest.raises(AssertionError):
        R.check_finish(fk[:-1], fv[:-1], L.keys, labels, kt)
    eq = np.full(100, L.keys[0], np.uint32)
    R.check_finish(R.unmap(eq, kt), np.arange(100, dtype=np.uint32)[::-1].copy(), eq, np.arange(100, dtype=np.uint32), kt)
    # the whole sharded sort
    shards = [s[:3000] for s in R.sharded_shards("uniform", kt, 3)]
    res = R.emulate_sharded_sort(shards, kt, True, 3, R.numpy_ops())
    R.check_sharded(res, shards, kt, True, 3)
    good = res.out_k[1], res.out_v[1], res.counts[2]
    j = int(np.nonzero(good[0][1:] != good[0][:-1])[0][0])
    for k_, v_, c_ in ((_flip(good[0], 9), good[1], good[2]), (good[0], _swap(good[1], j, j + 1), good[2]), (good[0], good[1], _bump(good[2], 3))):
        res.out_k[1], res.out_v[1], res.counts[2] = k_, v_, c_
        with pytest.raises(AssertionError):
            R.check_sharded(res, shards, kt, True, 3)
    res.out_k[1], res.out_v[1], res.counts[2] = good
    res.out_k[0], res.out_k[1] = np.concatenate([res.out_k[0], good[0][:1]]), good[0][1:]     # one key on the wrong rank
    with pytest.raises(AssertionError, match="the split gives it"):
        R.check_sharded(res, shards, kt, True, 3)
