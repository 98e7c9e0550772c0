"""The top-k campaign before a device sees it (tests/topk_campaign.py): the cases are pure functions of (family, seed, index),
image() agrees with every existing reference module and with the order of the values themselves, the committed seeds reach
every (entry point, key type, direction, form), plan path, level count, flat route, 64-bit depth and segmented length class
often enough, the segmented cases can never drop a segment, and check() reports every single mutation of a correct output."""
import collections
import functools
import importlib

import numpy as np
import pytest

import topk_campaign as T

FAMILIES = tuple(T.FAMILIES)


@functools.lru_cache(maxsize=None)
def cases_of(family):
    """[(case, reference)] of the committed seeds, built once and left unchanged."""
    return [(c, T.reference(c)) for c in (T.case(family, seed, i) for seed in T.SEEDS for i in range(T.CASES))]


FIELDS = ("family", "seed", "index", "shape", "width", "key_type", "descending", "form", "dist", "k", "alloc", "n", "S",
          "rows", "cols", "stride", "key_in_off", "key_out_off")
ARRAYS = ("keys", "vals", "begin", "end")


# ---------------------------------------------------------------------------------------------- 1. pure functions --
@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_is_a_pure_function_of_family_seed_and_index(family):
    for c, _ in cases_of(family):
        d = T.case(c.family, c.seed, c.index)
        for f in FIELDS:
            assert getattr(c, f, None) == getattr(d, f, None), (c.name(), f)
        for f in ARRAYS:
            a, b = getattr(c, f, None), getattr(d, f, None)
            assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a, b)), (c.name(), f)


# ------------------------------------------------------------------------------------------------- 2. the image --
def patterns(key_type, n=20000, seed=5):
    """Random patterns, every special one, and the neighbours of the specials."""
    dt = T.UINT[T.WIDTH[key_type]]
    rng = np.random.default_rng([seed, key_type])
    sp = T.specials(key_type)
    return np.concatenate([rng.integers(0, 1 << T.WIDTH[key_type], n, dtype=np.uint64).astype(dt), sp, sp + dt(1), sp - dt(1),
                           T.make_keys(rng, "specials", n, key_type, False)])


# (module, the path to its image function, the key types it serves): what each of the per-entry-point references selects on
EXISTING = [("topk_ref", "image", 32), ("topk_narrow_ref", "image16", 16), ("topk_wide_ref", "image", 64),
            ("topk_rows_ref", "R.image", 32), ("topk_rows_narrow_ref", "image16", 16), ("topk_rows_wide_ref", "W.image", 64),
            ("topk_segmented_ref", "R.image", 32), ("topk_segmented_narrow_ref", "NR.image16", 16),
            ("topk_segmented_wide_ref", "W.image", 64), ("topk_rows_anyk_ref", "R.image", 32),
            ("topk_rows_anyk_narrow_ref", "image16", 16)]


@pytest.mark.parametrize("module,path,width", EXISTING, ids=[e[0] for e in EXISTING])
def test_image_agrees_with_every_existing_reference_module(module, path, width):
    fn = importlib.import_module(module)
    for part in path.split("."):
        fn = getattr(fn, part)
    for kt in T.TYPES[width]:
        p = patterns(kt)
        for desc in (False, True):
            mine, theirs = T.image(p, kt, desc), fn(p, kt, desc)
            assert mine.dtype == theirs.dtype and np.array_equal(mine, theirs), (module, T.KEY_NAMES[kt], desc)
            assert np.array_equal(T.preimage(mine, kt, desc), p), (T.KEY_NAMES[kt], desc)


def values_of(p, key_type):
    """The values the patterns stand for, in a type numpy orders by itself."""
    w = T.WIDTH[key_type]
    if key_type == T.BF16:
        return (p.astype(np.uint32) << np.uint32(16)).view(np.float32)          # exact
    if key_type in T.FLOATS:
        return p.view({16: np.float16, 32: np.float32, 64: np.float64}[w])
    if key_type in T.SIGNED:
        return p.view({16: np.int16, 32: np.int32, 64: np.int64}[w])
    return p


@pytest.mark.parametrize("key_type", sorted(T.WIDTH), ids=lambda kt: T.KEY_NAMES[kt])
def test_image_orders_the_values_as_numpy_orders_them(key_type):
    """On finite non-zero values a stable argsort of image() is a stable argsort of the values themselves (descending: of the
    values mirrored, -v for the floats, ~v for the integers): an order none of this project's code computes."""
    p = patterns(key_type)
    v = values_of(p, key_type)
    if key_type in T.FLOATS:
        keep = np.isfinite(v) & (v != 0)
        p, v = p[keep], v[keep]
        assert p.size > 10000
    p = np.concatenate([p, p[:3000]])                 # ties, so that the stability is part of the claim
    v = np.concatenate([v, v[:3000]])
    for desc in (False, True):
        mirrored = v if not desc else (-v if key_type in T.FLOATS else ~v)
        assert np.array_equal(np.argsort(T.image(p, key_type, desc), kind="stable"), np.argsort(mirrored, kind="stable")), desc


# ------------------------------------------------------------------------------------------------- 3. the census --
FLOOR, TRIPLE_FLOOR = 5, 4
REACHED = {
    T.FLAT: {32: ("route 1", "route 2", "route 3"), 16: ("route 1", "route 2", "route 3"),
             64: ("route 1", "route 2", "D 1", "D 2", "D 3")},
    T.ROWS: dict.fromkeys((16, 32, 64), ("path 1", "path 2", "path 3", "levels 1", "levels 2", "levels 3")),
    T.ANYK: dict.fromkeys((16, 32), ("path 1", "path 2", "slabs 1", "slabs several", "k <= 1024", "k > 1024")),
    T.SEG: dict.fromkeys((16, 32, 64), ("launch groups 1", "launch groups 3", "launch groups 7", "k above a segment", "clamped")
                         + tuple("class %d" % q for q in range(6))),
}


def census_of(gs, family):
    count = collections.Counter()
    for c, r in cases_of(family):
        count.update(T.census(c, r, gs.lib))
    return count


@pytest.mark.parametrize("family", FAMILIES)
def test_census_of_the_committed_seeds(gs, family):
    """Per entry point: every (key type, direction, form) at least 4 times; every plan path, select level count, flat route,
    the 64-bit D >= 3 ("D 3" counts 3 and more) and every segmented length class at least 5 times; the cut strictly inside a
    tie run in at least a fifth of the cases."""
    shape, width = T.FAMILIES[family][:2]
    count = census_of(gs, family)
    print(family, sorted(count.items()))
    triples = {k: v for k, v in count.items() if k.startswith("triple ")}
    assert len(triples) == 6 * len(T.TYPES[width]) and min(triples.values()) >= TRIPLE_FLOOR, triples
    for tag in REACHED[shape][width]:
        assert count[tag] >= FLOOR, (family, tag, count[tag])
    assert 5 * count["cut inside a tie run"] >= len(cases_of(family)), count["cut inside a tie run"]


# --------------------------------------------------------------------------------- 4. no segment can be dropped --
@pytest.mark.parametrize("family", [f for f in FAMILIES if T.FAMILIES[f][0] == T.SEG])
def test_long_segments_are_disjoint_and_every_shape_is_served(gs, family):
    for c, r in cases_of(family):
        b, ln = T.clamp(c)
        long_ = np.flatnonzero(ln > T.CH)
        order = long_[np.argsort(b[long_])]
        assert (b[order][1:] >= (b[order] + ln[order])[:-1]).all(), c.name()
        assert int(ln[long_].sum()) <= c.n and c.n <= 400000, c.name()
        assert c.S * c.k < 1 << 32 and 1 <= c.k <= T.MAX_K, c.name()
        lists, tasks = T.seg_lists(c)
        lmax = min(c.S, c.n // (T.CH + 1))                    # the room the header's workspace formula keeps
        assert lists[5] <= lmax and tasks <= (c.n // T.CH + lmax if lmax else 0), c.name()
        assert np.array_equal(r.counts, np.minimum(ln, c.k)), c.name()


@pytest.mark.parametrize("family", FAMILIES)
def test_every_case_is_inside_its_entry_points_limits(family):
    for c, _ in cases_of(family):
        isz = c.width // 8
        assert c.key_in_off in (0, 1) and c.key_out_off in (0, 1) and (c.width != 64 or c.key_in_off == c.key_out_off == 0)
        assert c.keys.dtype == T.UINT[c.width] and c.keys.size == c.alloc and (c.keys.nbytes == c.alloc * isz)
        if c.shape == T.FLAT:
            assert 1 <= c.k <= c.n <= 400000, c.name()
        elif c.shape == T.SEG:
            assert c.begin.dtype == c.end.dtype == np.int32 and c.begin.size == c.end.size == c.S >= 1
        else:
            assert c.rows * c.stride <= 1500000 and c.cols <= c.stride and c.alloc == (c.rows - 1) * c.stride + c.cols
            assert 1 <= c.k <= c.cols and (c.shape == T.ANYK or c.k <= T.MAX_K) and c.rows * c.k < 1 << 31, c.name()


# --------------------------------------------------------------------------------------- 5. the checker has teeth --
def correct(c, r):
    """A HostArena after a correct call: the reference's outputs in the written slots, everything else as laid out."""
    a = T.HostArena(T.layout(c, 4096))
    S, k = r.counts.size, c.k
    a.view("keys_out", T.UINT[c.width]).reshape(S, k)[r.written] = r.keys[r.written]
    if c.form != T.KEYS:
        a.view("vals_out", np.uint32).reshape(S, k)[r.written] = r.vals[r.written]
    if c.shape == T.SEG:
        a.view("counts", np.uint32)[:] = r.counts
    return a


def _tied_slots(c, r):
    """(s, j): slots j and j + 1 of row s are written and hold equal keys with different values."""
    if c.form == T.KEYS:
        return None
    hit = (r.keys[:, 1:] == r.keys[:, :-1]) & r.written[:, 1:] & (r.vals[:, 1:] != r.vals[:, :-1])
    return divmod(int(np.flatnonzero(hit.reshape(-1))[0]), c.k - 1) if hit.any() else None


def flip_key_bit(c, r, a):
    s = int(np.flatnonzero(r.counts)[-1])
    a.view("keys_out", T.UINT[c.width])[s * c.k + int(r.counts[s]) - 1] ^= T.UINT[c.width](1 << (c.index % c.width))
    return True


def swap_tied_indices(c, r, a):
    at = _tied_slots(c, r)
    if at is None:
        return False
    v = a.view("vals_out", np.uint32)
    i = at[0] * c.k + at[1]
    v[i], v[i + 1] = v[i + 1], v[i]
    return True


def later_member_of_the_tie_run(c, r, a):
    """The last element taken from the k-th key's run replaced by the run's next member, which the stable sort puts behind."""
    if c.form == T.KEYS or not r.inside.any():
        return False
    s = int(np.flatnonzero(r.inside)[0])
    base, length = T.subarrays(c)
    b, n, kept = int(base[s]), int(length[s]), int(r.counts[s])
    run = np.flatnonzero(T.image(c.keys[b:b + n], c.key_type, c.descending) == r.kth[s])
    q = int(run[int(r.take[s])])
    new = q if c.form == T.ARGS else int(c.vals[b + q])
    v = a.view("vals_out", np.uint32)
    if v[s * c.k + kept - 1] == new:
        return False
    v[s * c.k + kept - 1] = new
    return True


def value_from_a_neighbouring_row(c, r, a):
    if c.form == T.KEYS or r.counts.size < 2:
        return False
    both = r.written[:-1] & r.written[1:] & (r.vals[:-1] != r.vals[1:])
    if not both.any():
        return False
    s, j = divmod(int(np.flatnonzero(both.reshape(-1))[0]), c.k)
    a.view("vals_out", np.uint32)[s * c.k + j] = r.vals[s + 1, j]
    return True


def count_off_by_one(c, r, a):
    if c.shape != T.SEG:
        return False
    counts = a.view("counts", np.uint32)
    s = c.index % c.S
    counts[s] = counts[s] - 1 if c.index % 2 and counts[s] else counts[s] + 1
    return True


def write_behind_kept(c, r, a):
    if r.written.all():
        return False
    s, j = divmod(int(np.flatnonzero(~r.written.reshape(-1))[0]), c.k)
    a.view("keys_out", T.UINT[c.width])[s * c.k + j] ^= T.UINT[c.width](1)
    return True


def guard_byte(c, r, a):
    names = list(a.slots)
    start, nbytes, lo, hi = a.slots[names[c.index % len(names)]]
    a.mem[start + nbytes if c.index % 2 else start - 1] ^= 0x10
    return True


def input_element(c, r, a):
    name = ("keys_in", "vals_in", "begin", "end")[c.index % 4]
    if name not in a.slots:
        name = "keys_in"
    a.mem[a.slots[name][0] + (c.index * 7919) % a.slots[name][1]] ^= 0x01
    return True


MUTATIONS = [flip_key_bit, swap_tied_indices, later_member_of_the_tie_run, value_from_a_neighbouring_row, count_off_by_one,
             write_behind_kept, guard_byte, input_element]
# what a shape cannot show: one row has no neighbour; counts and slots behind kept are the segmented calls'
INAPPLICABLE = {(T.FLAT, "value_from_a_neighbouring_row"), (T.FLAT, "count_off_by_one"), (T.FLAT, "write_behind_kept"),
                (T.ROWS, "count_off_by_one"), (T.ROWS, "write_behind_kept"),
                (T.ANYK, "count_off_by_one"), (T.ANYK, "write_behind_kept")}
SAMPLE = 36         # cases per family: two turns of the rotation of the three-type families, more than one of the 16-bit ones


@pytest.mark.parametrize("family", FAMILIES)
def test_check_accepts_the_reference_and_reports_every_single_mutation(family):
    applied = collections.Counter()
    for c, r in cases_of(family)[:SAMPLE]:
        assert T.check(c, correct(c, r).snapshot(), r) is None, c.name()
        for m in MUTATIONS:
            a = correct(c, r)
            if m(c, r, a):
                applied[m.__name__] += 1
                assert T.check(c, a.snapshot(), r) is not None, (c.describe(), m.__name__)
    shape = T.FAMILIES[family][0]
    for m in MUTATIONS:
        if (shape, m.__name__) not in INAPPLICABLE:
            assert applied[m.__name__] >= 3, (family, m.__name__, applied)
