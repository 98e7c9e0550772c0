"""The inputs of tests/test_topk_edges_gpu.py without a device: every builder of tests/topk_cases.py is held to its intent
with the numpy reference alone -- the route, the size of the k-th element's top-byte bucket (the TOP word), d0, the LESS and
TAKE words of the cuts around tie runs, the tile layout -- so a builder that stops producing its edge fails here."""
import numpy as np
import pytest

import topk_cases as T
import topk_ref as R

TYPES_DIRS = [(kt, desc) for kt in T.KEY_TYPES for desc in (False, True)]


# ------------------------------------------------------------------------------------------------------ preimage --
@pytest.mark.parametrize("kt,desc", TYPES_DIRS)
def test_image_of_preimage_is_the_identity(kt, desc):
    rng = np.random.default_rng(9)
    words = np.concatenate([rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32), np.array(T.IMAGES20, np.uint32)])
    keys = R.preimage(words, kt, desc)
    assert keys.dtype == np.uint32 and np.array_equal(R.image(keys, kt, desc), words)
    assert np.array_equal(R.preimage(R.image(words, kt, desc), kt, desc), words)        # and the other way round


def test_preimage_of_known_images():
    assert list(R.preimage(np.array([0, 0xFFFFFFFF], np.uint32), R.I32).view(np.int32)) == [-2**31, 2**31 - 1]
    assert list(R.preimage(np.array([0, 0xFFFFFFFF], np.uint32), R.I32, True).view(np.int32)) == [2**31 - 1, -2**31]
    f = R.preimage(np.array([0x007FFFFF, 0x7FFFFFFF, 0x80000000, 0xFF800000], np.uint32), R.F32)
    assert list(f[:1]) == [0xFF800000] and list(f[1:].view(np.float32)) == [-0.0, 0.0, np.inf]      # -inf by its bits, then values


# ---------------------------------------------------------------------------------------------- capacity boundary --
def test_capacities_of_the_table():
    assert [T.cap(n) for n, _ in T.CAPACITY] == [c for _, c in T.CAPACITY] == [65536, 65537, 93750]


@pytest.mark.parametrize("n,cap", T.CAPACITY)
@pytest.mark.parametrize("dc", [-1, 0, 1])
def test_bucket_case_routes(n, cap, dc):
    """c = cap - 1 and cap: route 1 at every k; c = cap + 1: route 2 inside the bucket, route 1 one before and one past it."""
    c, below, d0 = cap + dc, T.CAP_BELOW, T.CAP_D0
    for kt, desc in TYPES_DIRS if n == T.CAPACITY[0][0] else [(R.U32, False), (R.U32, True)]:
        ref = R.Ref(T.bucket_case(n, c, below, d0, n + dc, kt, desc), kt, desc)
        assert int(ref.tops[d0]) == c and int(ref.tops[:d0].sum()) == below
        for k, inside in T.capacity_ks(below, c):
            kth, less, take, top = ref.topk(k)[2]
            assert (kth >> 24 == d0) == inside and (top == c) == inside, (n, c, k)
            assert ref.route(k) == (2 if inside and dc == 1 else 1), (n, c, k)
            assert top <= cap or inside


# ------------------------------------------------------------------------------------------------------ layout --
def test_layer_sizes_are_23_24_and_25_tiles():
    assert [T.tiles(n) for n in T.LAYER_SIZES] == [23, 24, 25]
    assert [n % T.TILE != 0 for n in T.LAYER_SIZES] == [True, False, True]


@pytest.mark.parametrize("n,c,route", T.LAYERED)
def test_layered_case_layout_and_routes(n, c, route):
    d0, low = T.LAYER_D0, T.LAYER_LOW
    for kt, desc in [(R.U32, False), (R.F32, True), (R.I32, True)]:
        keys, below = T.layered_case(n, c, n + c, kt, desc)
        ref = R.Ref(keys, kt, desc)
        top = ref.img >> np.uint32(24)
        assert keys.size == n and int(ref.tops[d0]) == c and int(ref.tops[:d0].sum()) == below
        assert np.all(top[:15 * T.TILE] == low) and np.all(top[15 * T.TILE:16 * T.TILE] == d0)
        # the table the filter reads: digit `low` in front of tile 15 inside its chunk is at the 16-bit table's ceiling
        assert int(np.count_nonzero(top[T.CHUNK:15 * T.TILE] == low)) == 57344
        # the mixed tiles hold every population, several digits below d0 among them
        mixed = top[2 * T.CHUNK:]
        assert np.unique(mixed[mixed < d0]).size >= 4 and {0, low, d0 - 1} <= set(mixed[mixed < d0].tolist())
        assert np.any(mixed == d0) == (c > T.TILE) and np.any(mixed > d0)
        for k in T.layered_ks(below, c):
            kth, less, take, t = ref.topk(k)[2]
            assert kth >> 24 == d0 and t == c and ref.route(k) == route, (n, c, k)
        assert ref.topk(below)[2][0] >> 24 < d0


# -------------------------------------------------------------------------------------------------- digit edges --
def test_the_twenty_images_and_their_runs():
    assert len(T.IMAGES20) == len(T.RUNS20) == 20 and sorted(set(T.IMAGES20)) == T.IMAGES20
    assert set(T.RUNS20) == {1, 2, 63, 64, 65, 8191, 8192, 8193}
    for route, top in T.DIGIT_EDGES:
        runs = T.digit_edge_runs(route, top)
        per_top = {}
        for img, ln in runs:
            per_top[img >> 24] = per_top.get(img >> 24, 0) + ln
        n = sum(ln for _, ln in runs)
        assert 90000 <= n <= 130000 and T.cap(n) == 65536
        over = {t for t, s in per_top.items() if s > 65536}
        assert over == ({top} if route == 2 else set()), (route, top, per_top)
        assert per_top[0x00] != 65536 and per_top[0xFF] != 65536


@pytest.mark.parametrize("route,top", T.DIGIT_EDGES)
def test_digit_edge_cuts(route, top):
    """Every k of run_cuts: TAKE is the whole run at its end C, 1 at C + 1, all but one at C - 1; LESS is the runs in front;
    d0 = 0 and d0 = 255 and k-th images with 0x00 and 0xFF in every lower byte are among them, on the intended route."""
    runs = T.digit_edge_runs(route, top)
    n = sum(ln for _, ln in runs)
    for kt, desc in TYPES_DIRS:
        ref = R.Ref(T.digit_edge_case(route, top, kt, desc), kt, desc)
        assert np.array_equal(np.unique(ref.img), np.array(T.IMAGES20, np.uint32)) and ref.keys.size == n
        cuts = T.run_cuts(ref)
        want, kths, routes, C = set(), set(), set(), 0
        for img, ln in runs:
            start, C = C, C + ln
            want |= {k for k in (C - 1, C, C + 1) if 1 <= k <= n}
            assert ref.topk(C)[2][:3] == [img, start, ln]
            if C < n:
                assert ref.topk(C + 1)[2][1:3] == [C, 1]
            if ln > 1:
                assert ref.topk(C - 1)[2][:3] == [img, start, ln - 1]
            assert ref.route(C) == (2 if route == 2 and img >> 24 == top else 1), (img, C)
        assert set(cuts) == want and cuts == sorted(cuts)
        for k in cuts:
            kths.add(ref.topk(k)[2][0])
            routes.add(ref.route(k))
        assert kths == set(T.IMAGES20) and routes == ({1, 2} if route == 2 else {1})


def test_run_cuts_on_a_small_input():
    ref = R.Ref(np.array([7, 3, 7, 3, 7, 1, 7], np.uint32), R.U32)      # runs end at 1, 3, 7
    assert T.run_cuts(ref) == [1, 2, 3, 4, 6, 7]
    assert T.run_cuts(R.Ref(np.array([5], np.uint32), R.U32)) == [1]


# ------------------------------------------------------------------------------------------------- scan batches --
def test_scan_sizes_reach_the_second_and_third_batch_and_a_permuted_chunk_group():
    tl = [T.tiles(n) for n in T.SCAN_SIZES]
    assert tl == [1024, 1025, 1026, 2050]
    assert [-(-t // T.SCAN_BATCH) for t in tl] == [1, 2, 2, 3]
    chunks = [-(-t // T.CHUNK_TILES) for t in tl]
    assert chunks == [128, 129, 129, 257] and [c // T.SPINE_GROUP for c in chunks] == [0, 0, 0, 1]
    for n in T.SCAN_SIZES:
        assert all(1 <= k <= n for k in T.scan_equal_ks(n) + T.scan_random_ks(n))
        assert {1024 * T.TILE - 1, 1024 * T.TILE, n} <= set(T.scan_equal_ks(n))
    assert T.scan_equal_ks(T.SCAN_SIZES[0]) == [1024 * T.TILE - 1, 1024 * T.TILE]
    assert {2048 * T.TILE, 2048 * T.TILE + 1, 1024 * T.TILE + 8193} <= set(T.scan_equal_ks(T.SCAN_SIZES[3]))


@pytest.mark.parametrize("n", T.SCAN_SIZES)
def test_scan_inputs_share_one_top_byte_and_take_route_two(n):
    """The bucket is the whole input (TOP = n, past the capacity): route 2 at every k, without sorting 16M keys here."""
    i = T.SCAN_SIZES.index(n)
    kt, desc = T.KEY_TYPES[i % 3], bool(i % 2)
    for keys in (T.equal_case(n, kt, desc), T.topbyte_case(n, 3 + i, kt, desc)):
        tops = np.bincount(R.image(keys, kt, desc) >> np.uint32(24), minlength=256)
        assert keys.size == n and int(tops.max()) == n > T.cap(n)
    assert np.unique(T.equal_case(1000, kt, desc)).size == 1
    low = R.image(T.topbyte_case(n, 3 + i, kt, desc), kt, desc) & np.uint32(0xFFFFFF)
    assert np.unique(low[:100000]).size > 99000                      # random low bits: rounds two to four do real work


def test_uniform_input_of_the_largest_scan_size_takes_route_one():
    n = T.SCAN_SIZES[-1]
    tops = np.bincount(T.uniform_case(n, 8) >> np.uint32(24), minlength=256)
    assert int(tops.max()) <= T.cap(n) and int(np.cumsum(tops)[0]) < T.SPINE_K      # the k-th top byte has whole buckets in front


# -------------------------------------------------------------------------------------------------- class edges --
def test_class_edge_inputs():
    assert all(n <= R.SMALL_CAP for n in T.CLASS_EDGES) and T.CLASS_N > R.SMALL_CAP
    assert T.CLASS_KS == [2048, 2049, 4608, 4609, 9216, 9217, 17408, 17409, 65536, 65537]
    for n in T.CLASS_EDGES:
        assert R.Ref(T.uniform_case(n, n), R.U32).route(n // 2) == 3
    u, t = R.Ref(T.uniform_case(T.CLASS_N, 1), R.U32), R.Ref(T.topbyte_case(T.CLASS_N, 2), R.U32)
    for k in T.CLASS_KS:
        assert u.route(k) == 1 and t.route(k) == 2


# ----------------------------------------------------------------------------------------------------- campaign --
@pytest.mark.parametrize("seed", T.CAMPAIGN_SEEDS)
def test_campaign_cases_are_well_formed_and_reach_everything(seed):
    dists, routes, forms, types = set(), set(), set(), set()
    for i in range(T.CAMPAIGN_CASES):
        what, keys, kt, desc, rng = T.campaign_case(seed, i)
        n = keys.size
        assert min(abs(n - a) for a in T.CAMPAIGN_ANCHORS) <= 40 and keys.dtype == np.uint32, what
        ref = R.Ref(keys, kt, desc)
        ks = T.campaign_ks(ref, rng)
        assert len(ks) == 4 and all(1 <= k <= n and m in T.MODES for k, m in ks), what
        if i % 10 == 0:
            what2, keys2, _, _, rng2 = T.campaign_case(seed, i)         # a case is a function of (seed, index) alone
            assert what2 == what and np.array_equal(keys2, keys) and T.campaign_ks(ref, rng2) == ks
        dists.add(what.split()[2])
        types.add((kt, desc))
        for k, m in ks:
            routes.add(ref.route(k))
            forms.add(m)
    assert dists == set(T.CAMPAIGN_DISTS) and routes == {1, 2, 3} and forms == set(T.MODES) and len(types) == 6


# ---------------------------------------------------------------------------------------------------- workspace --
def test_temp_bytes_is_the_formula_at_the_new_sizes(gs):
    sizes = [n for n, _ in T.CAPACITY] + T.LAYER_SIZES + T.SCAN_SIZES + T.CLASS_EDGES + [T.CLASS_N]
    sizes += [sum(ln for _, ln in T.digit_edge_runs(r, t)) for r, t in T.DIGIT_EDGES]
    sizes += [a + d for a in T.CAMPAIGN_ANCHORS for d in (-40, 0, 40)]
    for n in sizes:
        ks = {1, n // 2, n - 1, n, T.CAP_BELOW + T.cap(n), T.SPINE_K} | set(T.CLASS_KS) | set(T.scan_equal_ks(n))
        for k in sorted(k for k in ks if 1 <= k <= n):
            for hv in (0, 1):
                assert gs.lib.gs_topk_temp_bytes(n, k, hv) == R.temp_bytes(n, k, hv, gs.lib.gs_lsb_copy_temp_bytes(k, hv)), (n, k, hv)
