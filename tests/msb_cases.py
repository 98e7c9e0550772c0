"""Built inputs for gs_msb_sort_u32, path by path: numpy builders, a restatement of what every level must do with them, and the
tables the two test modules share (tests/test_msb_paths_cpu.py holds the builders to their intent without a device,
tests/test_msb_paths_gpu.py runs them).  No GPU and no library here.

Every input is laid out in the order-preserving IMAGE of the key (what the device holds after level 0: to_image), shuffled with a
fixed seed, and mapped back for int32 and float32 keys with from_image; images below 0x80000000 are negative keys, and the
float rows carry -0.0 and NaN patterns as ordinary keys.  Where a decision of the sort depends on POSITIONS (the heavy-hitter
probes, the 64 sampled keys of a task, the 64 neighbours the one-pass plan adds at once) the shuffled input is then re-arranged
inside the bucket: every partition is stable, so a bucket's keys lie on the device in input order.

Expectations come from oracle/oracle.py (msb_classify_counts, msb_heavy_hitter, msb_level_lists) through `restate`, never from
the library.

LOCAL-SORT PLANS (launch_local_sorts / GS_LS, onepass_possible, local_b1, DD in gs_msb.hip).  b1 = local_b1(cap) is 11 / 12 /
13 / 14 for the classes 2048 / 4608 / 9216 / 17408; the one-pass plan holds 2^ob byte counters with ob = local_b1(cap) + 2 for
keys (13 / 14 / 15 / 16) and local_b1(2 * cap) + 2 for pairs (14 / 15 / 16 / 16); the few-distinct-values plan is compiled where
cap * (pairs ? 2 : 1) >= 8192.  A launch is decided per (level, class) from the level's `min_bits` (32: the single task of an
array that fits one workgroup; 24 / 16 / 8: levels 0 / 1 / 2, whose tasks have min_bits bits, or 8 more when merged or when they
are the strangers of a heavy-hitter bucket):

    min_bits   class (cap)    keys                             pairs
    32, 24     every class    ALL                              ALL
    16, 8      0 (2048)       ALL                              ALL
    16, 8      1 (4608)       ALL                              [DEDUPE_ALL] ALL
    16, 8      2 (9216)       [DEDUPE_ALL] ALL                 ONEPASS [DEDUPE] FLAGGED
    16, 8      3 (17408)      ONEPASS [DEDUPE] FLAGGED         ONEPASS [DEDUPE] FLAGGED

[...] only when the level showed skew (it opened a next level) and GS_MSB_DEDUPE is not 0.  ONEPASS, DEDUPE and DEDUPE_ALL only
ever take tasks of exactly 16 bits (b1 < bits <= ob resp. 16); every other task of such a class is left to FLAGGED / ALL.  So
the plans differ for 16-bit tasks only: unmerged tasks of level 1, merged tasks of level 2 (below 3000 keys: classes 0 and 1)
and the strangers of a level-2 heavy hitter (any class).  PLAN_TABLE below is this table; plan_from_code derives it again from
the rules, and tests/test_msb_paths_cpu.py holds the two together.

The census word `flagged` of a level (predict_flagged) is nonzero exactly when, in a class that launches ONEPASS,
  (b) a task has other than 16 bits (ONEPASS passes it by and flags it), or
  (c) a 16-bit task holds a value 16 times or more (a nibble count overflows; the byte counter's limit of 255 lies above that,
      so the two abandon conditions cannot be told apart from outside), or
  (a) the level showed skew and 3 of a 16-bit task's 64 sampled keys (task of 64 keys or more) are equal: the sample look flags it.
Level 0 and the single task never set it."""
import collections
import functools

import numpy as np

from oracle import oracle as O

U32, I32, F32 = 0, 1, 2                    # GS_KEY_U32 / I32 / F32
KEY_TYPES = (U32, I32, F32)
CAPS = O.MSB_CLASS_CAPS                    # 2048, 4608, 9216, 17408
CAP_MAX = CAPS[-1]
MERGE = O.MSB_MERGE                        # 3000
TILE = 8192                                # MSB_TILE
ALIGN_MIN_TILES = 256                      # ws_first_tile: buckets of this many tiles get a short first tile at an odd offset

ALL, ONEPASS, FLAGGED, DEDUPE, DEDUPE_ALL = "ALL", "ONEPASS", "FLAGGED", "DEDUPE", "DEDUPE_ALL"
PLAN_TABLE = {}                            # (min_bits, class, pairs) -> launch sequence; optional launches in a tuple
for _mb in (32, 24, 16, 8):
    for _c in range(4):
        for _p in (False, True):
            if _mb >= 24 or _c == 0 or (_c == 1 and not _p):
                seq = (ALL,)
            elif (_c == 1 and _p) or (_c == 2 and not _p):
                seq = ((DEDUPE_ALL,), ALL)
            else:
                seq = (ONEPASS, (DEDUPE,), FLAGGED)
            PLAN_TABLE[(_mb, _c, _p)] = seq
LEVEL_MIN_BITS = {0: 24, 1: 16, 2: 8}


def local_b1(cap):
    return 14 if cap >= 16384 else 13 if cap >= 8192 else 12 if cap >= 4096 else 11


def plan_from_code(min_bits, cls, pairs):
    """The same table from the rules of the code (onepass_possible, DD), to hold PLAN_TABLE to."""
    b1 = local_b1(CAPS[cls])
    ob = local_b1(CAPS[cls] * (2 if pairs else 1)) + 2
    dd = CAPS[cls] * (2 if pairs else 1) >= 4096 + 4096

    def possible(hi):
        return (b1 < min_bits <= hi) or (b1 < min_bits + 8 <= hi)
    opt = dd and possible(16)
    if not possible(ob):
        return (((DEDUPE_ALL,),) if opt else ()) + (ALL,)
    return (ONEPASS,) + (((DEDUPE,),) if opt else ()) + (FLAGGED,)


def onepass_classes(pairs):
    return (2, 3) if pairs else (3,)


def dedupe_classes(pairs):
    return (1, 2, 3) if pairs else (2, 3)


# ------------------------------------------------------------------------------------------------- key images --
def to_image(keys, kt):
    """uint32 bit patterns of key type kt -> their order-preserving images (test_buffer_contracts_gpu.ordmap for 32-bit keys)."""
    k = keys.astype(np.uint32)
    if kt == I32:
        return k ^ np.uint32(0x80000000)
    if kt == F32:
        return np.where(k & np.uint32(0x80000000) != 0, ~k, k | np.uint32(0x80000000)).astype(np.uint32)
    return k


def from_image(img, kt):
    img = img.astype(np.uint32)
    if kt == I32:
        return img ^ np.uint32(0x80000000)
    if kt == F32:
        return np.where(img & np.uint32(0x80000000) != 0, img ^ np.uint32(0x80000000), ~img).astype(np.uint32)
    return img


# ------------------------------------------------------------------------------------------------ restatement --
Task = collections.namedtuple("Task", "level cls offset size bits merged stranger content")   # content: device order, None = unknown
Restated = collections.namedtuple("Restated", "census tasks buckets")


def _zero():
    return {"buckets": 0, "keys": 0, "pivot_buckets": 0, "pivot_keys": 0, "task_keys": 0, "tasks": [0, 0, 0, 0]}


CENSUS_FIELDS = ("buckets", "keys", "pivot_buckets", "pivot_keys", "task_keys", "tasks")


def restate(img, pivot=True):
    """What gs_msb_sort_u32 does with keys whose images are `img` (keys and pairs alike: the same four classes): the census of
    the four levels, every local-sort task (with its keys in device order where the partition is stable; the strangers of a
    heavy-hitter bucket are written by another route, their order is not restated) and the buckets of every level."""
    img = np.ascontiguousarray(img, dtype=np.uint32)
    n = int(img.size)
    cen, tasks, buckets = [_zero() for _ in range(4)], [], {0: [(0, n)]}
    cen[0].update(buckets=1, keys=n)
    if n <= CAP_MAX:                                  # one task on all 32 bits; no classification, task_keys stays 0
        cls = O.msb_class_of(n)
        cen[0]["tasks"][cls] = 1
        tasks.append(Task(0, cls, 0, n, 32, False, False, img))
        return Restated(cen, tasks, buckets)
    level_buckets = [(0, n, img)]
    for L in range(4):
        if L:
            if not level_buckets:
                break
            cen[L].update(buckets=len(level_buckets), keys=sum(s for _, s, _ in level_buckets))
            buckets[L] = [(o, s) for o, s, _ in level_buckets]
        if L == 3:                                    # the last scatter finishes every key it gets
            break
        c, rb, nxt = cen[L], 24 - 8 * L, []
        for off, size, content in level_buckets:
            hh = O.msb_heavy_hitter(content) if (pivot and L >= 1) else None
            if hh is not None:
                cand, less, eq = hh
                c["pivot_buckets"] += 1
                c["pivot_keys"] += size
                for o, s in ((off, less), (off + less + eq, size - less - eq)):
                    if s:
                        c["tasks"][O.msb_class_of(s)] += 1
                        c["task_keys"] += s
                        tasks.append(Task(L, O.msb_class_of(s), o, s, rb + 8, False, True, None))
                continue
            digit = ((content >> np.uint32(rb)) & np.uint32(0xff)).astype(np.int64)
            b, t = O.msb_classify_counts(np.bincount(digit, minlength=256), off, L)
            by_digit = content[np.argsort(digit, kind="stable")]
            for cls, o, s, bits in t:
                c["tasks"][cls] += 1
                c["task_keys"] += s
                tasks.append(Task(L, cls, o, s, bits, bits == rb + 8, False, by_digit[o - off:o - off + s]))
            for o, s in b:
                nxt.append((o, s, by_digit[o - off:o - off + s]))
        level_buckets = nxt
    return Restated(cen, tasks, buckets)


def task_lists(r, level):
    """The lists of gs_msb_classify_upto(stop_level=level) from a restatement: (bucket set, {class: set of (offset, size, bits)})."""
    return (set(r.buckets.get(level + 1, [])),
            {c: {(t.offset, t.size, t.bits) for t in r.tasks if t.level == level and t.cls == c} for c in range(4)})


def sample_positions(size):
    """The 64 positions of a task that msb_task_sample_kernel reads: 8 clusters of 8 neighbours."""
    return [(((size - 8) * (2 * c + 1)) >> 4) + j for c in range(8) for j in range(8)]


def sample_counts(content, bits):
    """(keys of the 64 sampled that occur 3 times or more among them, sampled keys that have a twin)."""
    s = content[sample_positions(content.size)] & np.uint32((1 << bits) - 1)
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    mult = cnt[inv]
    return int((mult >= 3).sum()), int((mult >= 2).sum())


def fullest_bin(content, bits):
    """Keys in the fullest bin of the one-pass plan: the bins are the values of the task's sort bits."""
    return int(np.unique(content & np.uint32((1 << bits) - 1), return_counts=True)[1].max())


def predict_flagged(r, level, pairs):
    """The census word `flagged` of `level` by the rule in the module docstring: True / False, or None where it hangs on the
    sampled keys of a task whose order on the device is not restated (strangers of a heavy hitter)."""
    if level == 0 or level == 3:
        return False
    skew = bool(r.buckets.get(level + 1))
    flagged, unknown = False, False
    for t in r.tasks:
        if t.level != level or t.cls not in onepass_classes(pairs):
            continue
        if t.bits != 16:
            flagged = True                                                # (b)
        elif t.content is None:
            unknown = True
        else:
            if fullest_bin(t.content, 16) >= 16:
                flagged = True                                            # (c)
            if skew and t.size >= 64 and sample_counts(t.content, 16)[0]:
                flagged = True                                            # (a)
    return True if flagged else (None if unknown else False)


# --------------------------------------------------------------------------------------------------- builders --
def _prefix(bytes_):
    p = 0
    for b in bytes_:
        p = (p << 8) | b
    return p


def under(prefix, low):
    """Images with the bytes `prefix` on top of the values `low` (which fill the remaining bits)."""
    rbt = 32 - 8 * len(prefix)
    low = np.asarray(low, dtype=np.uint64)
    assert low.size == 0 or int(low.max()) < (1 << rbt)
    return ((np.uint64(_prefix(prefix)) << np.uint64(rbt)) | low).astype(np.uint32)


def rand_low(rng, bits, m, ones_every=0):
    """m random values of `bits` bits; every ones_every-th (and the first) all ones: they tie with a local sort's padding."""
    v = rng.integers(0, 1 << bits, size=m, dtype=np.uint64) if bits else np.zeros(m, np.uint64)
    if ones_every and m:
        v[::ones_every] = (1 << bits) - 1
    return v


def positions_of(img, prefix):
    """Input positions of the keys under `prefix`, in input order = the order the bucket's keys have on the device."""
    return np.flatnonzero((img >> np.uint32(32 - 8 * len(prefix))) == np.uint32(_prefix(prefix)))


def put(content, positions, wanted):
    """Re-order `content` (in place) so that content[positions[i]] == wanted[i]: one key of each wanted value is taken out of
    the array, the others keep their order in the places that are left."""
    positions, wanted = np.asarray(positions, np.int64), np.asarray(wanted, np.uint32)
    assert np.unique(positions).size == positions.size == wanted.size
    order = np.argsort(content, kind="stable")
    by_value, used, nth = content[order], np.zeros(content.size, bool), {}
    for w in wanted:
        at = int(np.searchsorted(by_value, w, side="left")) + nth.get(int(w), 0)
        assert at < content.size and by_value[at] == w, "not enough keys of a wanted value"
        used[order[at]] = True
        nth[int(w)] = nth.get(int(w), 0) + 1
    rest = content[~used]
    free = np.ones(content.size, bool)
    free[positions] = False
    content[free] = rest
    content[positions] = wanted
    return content


def rearrange(img, prefix, fn):
    """Apply fn(content) -> content to the keys under `prefix`, in place in input order."""
    idx = positions_of(img, prefix)
    img[idx] = fn(img[idx].copy())


def finish(parts, seed, fixups=()):
    """Concatenate, shuffle with a fixed seed, apply the positional fix-ups [(prefix, fn)], freeze."""
    img = np.concatenate(parts).astype(np.uint32)
    np.random.default_rng(seed).shuffle(img)
    for prefix, fn in fixups:
        rearrange(img, prefix, fn)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------- 1. classification: count tables --
# A table lists what the 256 consecutive digits of ONE bucket hold: ("run", counts) must become one merged task (zeros inside
# are empty digits), ("single", c) one unmerged task, ("bucket", c) a bucket of the next level, ("gap", k) k empty digits.
SEP = ("single", MERGE)                    # 3000 keys: joins no run and lets none pass
TABLES = {
    # sums of 2999 merge, sums of 3000 do not (a run grows while sum + c < 3000); runs of 2 and 3 sub-buckets; starts at digit 0
    "merge_sums": [("run", [2000, 999]), SEP, ("single", 2000), ("single", 1000), SEP, ("run", [1000, 1000, 999]), SEP,
                   ("run", [1000, 1000]), ("single", 1000), SEP],
    "run255_2999": [("run", [11] * 254 + [205]), ("bucket", CAP_MAX + 1)],
    "run255_3000": [("run", [11] * 254), ("single", 206), ("bucket", CAP_MAX + 1)],
    "ends_at_255": [("bucket", CAP_MAX + 1), ("gap", 253), ("run", [1500, 1499])],
    # empty digits inside a run; a sub-bucket too large for a local sort in the middle of what would be a run; a sub-bucket of
    # 3000 ... 17408 between tiny ones joins no run, and a later run still forms
    "boundaries": [("run", [500, 0, 0, 700, 0, 900]), SEP, ("single", 1000), ("bucket", CAP_MAX + 1), ("single", 1000), SEP,
                   ("single", 10), ("single", 5000), ("run", [10, 20]), SEP],
    # no non-empty sub-bucket below 3000: the shortcut; its neighbour has exactly one: the full walk
    "no_small": [("single", 3000), ("single", 4608), ("bucket", CAP_MAX + 1), ("single", 9216), ("gap", 2), ("single", CAP_MAX),
                 ("single", 3001)],
    "one_small": [("single", 3000), ("single", 4608), ("bucket", CAP_MAX + 1), ("single", 9216), ("gap", 2), ("single", CAP_MAX),
                  ("single", 3001), ("single", 2999)],
    # every class at and next to its cap, unmerged and merged; the sizes 1, 63, 64 (the sample look starts at 64)
    "caps": [SEP, ("single", 1), SEP, ("single", 63), SEP, ("single", 64), SEP, ("single", 2047), ("single", 2048), ("single", 2049),
             ("single", 4607), ("single", 4608), ("single", 4609), ("single", 9215), ("single", 9216), ("single", 9217),
             ("single", CAP_MAX - 1), ("single", CAP_MAX), ("bucket", CAP_MAX + 1), SEP, ("run", [1, 1]), SEP, ("run", [31, 32]), SEP,
             ("run", [32, 32]), SEP, ("run", [1024, 1023]), SEP, ("run", [1024, 1024]), SEP, ("run", [1024, 1025]), SEP,
             ("run", [1500, 1499]), SEP],
}
TABLE_NAMES = tuple(TABLES)


def table_counts(name):
    """(256 counts, expected [(kind, first digit, size, sub-buckets)]) of a table."""
    counts, expect = [], []
    for kind, x in TABLES[name]:
        if kind == "gap":
            counts += [0] * x
        elif kind == "run":
            expect.append(("run", len(counts), sum(x), sum(1 for c in x if c)))
            counts += list(x)
        else:
            expect.append((kind, len(counts), x, 1))
            counts.append(x)
    assert len(counts) <= 256, name
    counts += [0] * (256 - len(counts))
    return np.array(counts, np.int64), expect


def bucket_from_counts(prefix, counts, rng):
    """Keys under `prefix` whose next byte d occurs counts[d] times; the bits below are random, every 8th key's all ones."""
    rb = 24 - 8 * len(prefix)
    return [under(tuple(prefix) + (d,), rand_low(rng, rb, int(c), ones_every=8)) for d, c in enumerate(counts) if c]


TABLE_TOPS = (0x05, 0x2B, 0x60, 0x7F, 0x80, 0xA4, 0xD0, 0xFF)      # one top byte per table: negative and positive keys
LEAD = 777                                                        # keys in front of everything: later offsets are odd


@functools.lru_cache(maxsize=None)
def classify_input(level, table=None):
    """Level 0: the array IS the bucket, one table per input.  Levels 1 and 2: every table is a bucket of that level under its
    own top byte (level 2: under the second byte 0x33 as well), behind 777 keys of the top byte 0."""
    rng = np.random.default_rng(1000 + level)
    if level == 0:
        return finish(bucket_from_counts((), table_counts(table)[0], rng), seed=level)
    parts = [under((0x00,), rand_low(rng, 24, LEAD))]
    for top, name in zip(TABLE_TOPS, TABLE_NAMES):
        parts += bucket_from_counts((top,) if level == 1 else (top, 0x33), table_counts(name)[0], rng)
    return finish(parts, seed=level)


def classify_inputs():
    """[(label, level, images)] of section 1."""
    out = [(f"L0-{name}", 0, classify_input(0, name)) for name in TABLE_NAMES]
    return out + [("L1-tables", 1, classify_input(1)), ("L2-tables", 2, classify_input(2))]


@functools.lru_cache(maxsize=None)
def level3_input(which):
    """'one': 17409 keys that share three bytes and spread over 256 last bytes -- the only bucket of levels 1, 2 and 3.
    'three': three such buckets (17409, 17411, 20001 keys) behind odd-sized neighbours."""
    rng = np.random.default_rng(33)
    if which == "one":
        return finish([under((0x9C, 0x01, 0xFE), rand_low(rng, 8, CAP_MAX + 1))], seed=33)
    parts = [under((0x00,), rand_low(rng, 24, LEAD))]
    for pre, m in (((0x11, 0x22, 0x33), CAP_MAX + 1), ((0x80, 0x00, 0x00), CAP_MAX + 3), ((0xFF, 0x00, 0xFF), 20001)):
        parts.append(under(pre, rand_low(rng, 8, m)))
        parts.append(under((pre[0], pre[1] ^ 0x55), rand_low(rng, 16, 333)))
    return finish(parts, seed=34)


MANY = 250


@functools.lru_cache(maxsize=None)
def many_buckets_input():
    """250 buckets at level 1 and 250 at level 2: every top byte 3 .. 252 holds 17409 + i keys that share their second byte."""
    rng = np.random.default_rng(44)
    return finish([under((3 + i, (7 * i) & 0xff), rand_low(rng, 16, CAP_MAX + 1 + i)) for i in range(MANY)], seed=44)


# --------------------------------------------------------------------------------------------- 2. heavy hitters --
HH = collections.namedtuple("HH", "name less eq greater seen taken")
HH_CASES = (
    HH("half_even", 10000, 20000, 10000, True, True),              # eq exactly half of an even size
    HH("below_half_even", 10000, 19999, 10001, True, False),
    HH("below_half_odd", 10000, 20000, 10001, True, False),        # 20000 of 40001
    HH("less_at_cap", CAP_MAX, 20000, 5, True, True),
    HH("less_over_cap", CAP_MAX + 1, 20000, 5, True, False),
    HH("greater_at_cap", 5, 20000, CAP_MAX, True, True),
    HH("greater_over_cap", 5, 20000, CAP_MAX + 1, True, False),
    HH("all_equal", 0, CAP_MAX + 1, 0, True, True),                # no stranger task at all
    HH("none_and_one", 0, 20000, 1, True, True),
    HH("class0_class1", 2048, 17500, 2049, True, True),
    HH("class1_class2", 4608, 20000, 4609, True, True),
    HH("class2_class3", 9216, 30001, 9217, True, True),
    HH("unseen", 3000, 20000, 3000, False, False),                 # the probes and the samples all miss the dominant value
    HH("two_samples", 3000, 20000, 3000, 2, False),                # at the three probes, but in 2 of the 16 samples: not examined
    HH("three_samples", 3000, 20000, 3000, 3, True),               # in 3 of the 16 samples: examined, and taken
    HH("tiles_full", 2000, 3 * TILE - 4000, 2000, True, True),     # 8192 * 3 keys
    HH("tiles_ragged", 2000, 3 * TILE - 3999, 2000, True, True),   # 8192 * 3 + 1
)
HH_TOPS = tuple(0x08 + 0x0E * i for i in range(len(HH_CASES)))     # 0x08 .. 0xE8: both signs


def hh_probes(size):
    q = size // 4
    return [q, 2 * q, 3 * q]


def hh_samples(size):
    return [(size * (2 * i + 1)) >> 5 for i in range(16)]


def hh_positions(size):
    return sorted(set(hh_probes(size)) | set(hh_samples(size)))


def hh_keys(prefix, case, rng):
    """(keys of a bucket under `prefix` with case.less / eq / greater keys below / at / above one value, that value)."""
    rbt = 32 - 8 * len(prefix)
    dom_low = (0x5A5A5A >> (24 - rbt)) | (1 << (rbt - 1))
    less = rng.integers(0, dom_low, size=case.less, dtype=np.uint64)
    greater = rng.integers(dom_low + 1, 1 << rbt, size=case.greater, dtype=np.uint64)
    keys = under(prefix, np.concatenate((less, np.full(case.eq, dom_low, np.uint64), greater)))
    return keys, int(under(prefix, [dom_low])[0])


def hh_fix(case, dom):
    """Decide the heavy-hitter look by construction.  case.seen True: every probed and sampled position holds the dominant value;
    False: none does; a number k: the three probes and exactly the first k of the 16 samples do."""
    def fn(content):
        S = np.array(hh_positions(content.size))
        assert S.size == 19                               # the probes and the samples are different positions
        if case.seen is True:
            W = S
        elif case.seen is False:
            W = S[:0]
        else:
            W = np.array(hh_probes(content.size) + hh_samples(content.size)[:case.seen])
        N = np.setdiff1d(S, W)
        free = np.ones(content.size, bool)
        free[S] = False
        is_dom = content == np.uint32(dom)
        for bad, donors in ((W[~is_dom[W]], np.flatnonzero(free & is_dom)), (N[is_dom[N]], np.flatnonzero(free & ~is_dom))):
            donors = donors[:bad.size]
            assert donors.size == bad.size
            content[bad], content[donors] = content[donors].copy(), content[bad].copy()
        return content
    return fn


@functools.lru_cache(maxsize=None)
def hh_input(level):
    """(images, [(case, prefix, dominant image)]).  Level 1: one bucket per case under its own top byte.  Level 2: two cases share
    a top byte (second bytes 0x40 and 0xC0) with a filler spread over other second bytes, so that the level-1 bucket holds no
    value in half of its keys -- two dominated level-2 buckets under a level-1 bucket that is not."""
    rng = np.random.default_rng(200 + level)
    parts, info, fix = [under((0x00,), rand_low(rng, 24, LEAD))], [], []
    if level == 1:
        for top, case in zip(HH_TOPS, HH_CASES):
            keys, dom = hh_keys((top,), case, rng)
            parts.append(keys)
            info.append((case, (top,), dom))
    else:
        for i in range(0, len(HH_CASES), 2):
            pair, top, sizes = HH_CASES[i:i + 2], HH_TOPS[i], []
            for case, second in zip(pair, (0x40, 0xC0)):
                keys, dom = hh_keys((top, second), case, rng)
                parts.append(keys)
                info.append((case, (top, second), dom))
                sizes.append(keys.size)
            f = (abs(sizes[0] - sizes[1]) if len(sizes) == 2 else sizes[0]) + 1001
            second = rng.choice([b for b in range(256) if b not in (0x40, 0xC0)], size=f).astype(np.uint64)
            parts.append(under((top,), (second << np.uint64(16)) | rand_low(rng, 16, f)))
    for case, prefix, dom in info:
        fix.append((prefix, hh_fix(case, dom)))
    return finish(parts, seed=200 + level, fixups=fix), info


@functools.lru_cache(maxsize=None)
def hh_big_input():
    """A dominated level-1 bucket of 256 tiles and 4097 keys behind neighbours of 777 and 20001 keys: it starts off a
    64-element boundary and gets the short first tile of ws_first_tile."""
    rng = np.random.default_rng(210)
    case = HH("big_odd_offset", 9000, ALIGN_MIN_TILES * TILE + 4097 - 26000, 17000, True, True)
    keys, dom = hh_keys((0xB7,), case, rng)
    parts = [under((0x00,), rand_low(rng, 24, LEAD)), under((0x31,), rand_low(rng, 24, 20001)), keys]
    return finish(parts, seed=210, fixups=[((0xB7,), hh_fix(case, dom))]), [(case, (0xB7,), dom)]


@functools.lru_cache(maxsize=None)
def hh_whole_array_input():
    """One value holds 30000 of 30100 keys; the others have other top bytes.  Level 0 knows no heavy hitters: the value's top
    byte becomes a level-1 bucket, and that one is dominated."""
    rng = np.random.default_rng(220)
    dom = 0x6B5A5A5A
    others = np.concatenate((rng.integers(0, 0x6B000000, 50, dtype=np.uint64), rng.integers(0x6C000000, 1 << 32, 50, dtype=np.uint64)))
    return finish([np.full(30000, dom, np.uint32), others.astype(np.uint32)], seed=220), dom


# ------------------------------------------------------------------------------------------- 3. local-sort plans --
SINGLE_SIZES = (1, 63, 64, 2047, 2048, 4607, 4608, 9215, 9216, CAP_MAX - 1, CAP_MAX)


@functools.lru_cache(maxsize=None)
def single_task_input(n):
    """An array that is one task on all 32 bits; one key in 8 is all ones."""
    rng = np.random.default_rng(300 + n)
    return finish([rand_low(rng, 32, n, ones_every=8).astype(np.uint32)], seed=n)


def distinct_values(rng, m, exclude=()):
    """m distinct 16-bit values, none of `exclude`."""
    pool = np.setdiff1d(np.arange(65536, dtype=np.uint64), np.array(exclude, np.uint64))
    return rng.permutation(pool)[:m]


OP = collections.namedtuple("OP", "name k front value look flagged")
# the one-pass plan's limits, in a level without skew (the sample look does not run, the attempt is made): the fullest bin holds
# k keys, scattered or as neighbours at the start of the task (the wave-uniform branch adds 64 at once; 4 x 64 crosses 255 in
# that branch, 3 x 64 + 63 and 3 x 64 + 62 end in the other one)
OP_CASES = (
    OP("k15", 15, False, 0x1234, None, False),
    OP("k15_ones", 15, False, 0xFFFF, None, False),
    OP("k16", 16, False, 0x1234, None, True),
    OP("k16_ones", 16, False, 0xFFFF, None, True),
    OP("k254", 254, False, 0x8001, None, True),
    OP("k255", 255, False, 0x8001, None, True),
    OP("k256", 256, False, 0xFFFF, None, True),
    OP("k254_front", 254, True, 0xFFFF, None, True),
    OP("k255_front", 255, True, 0x0000, None, True),
    OP("k256_front", 256, True, 0x8001, None, True),
    # the same level with one oversized sub-bucket: the look runs.  3 equal keys among the 64 sampled flag a task the plan would
    # have sorted; 4 twins mark it for the few-distinct plan and leave it to the one-pass plan; heavy repeats the look misses are
    # attempted and abandoned; a task within the limits stays unflagged
    OP("look_flag", 3, False, 0x4321, "triple", True),
    OP("look_dd", 2, False, 0x4321, "twins", False),
    OP("look_missed", 40, False, 0x4321, "distinct", True),
    OP("look_none", 15, False, 0xFFFF, "distinct", False),
)
OP_TOP, OP_TASK, OP_FILL, OP_OVER = 0x9A, 0x10, 0x20, 0xF0
OP_TASK_SIZE = {2: 6000, 3: 12000}


def op_fix(case, pre):
    def fn(content):
        v = np.uint32(_prefix(pre + (case.value >> 8, case.value & 0xff)))
        if case.front:
            put(content, list(range(case.k)), [v] * case.k)
        if case.look:
            pos = sample_positions(content.size)
            singles = [x for x in np.unique(content) if x != v][:64]
            if case.look == "triple":
                wanted = [v, v, v] + singles[:61]
            elif case.look == "twins":
                tw = [x for x, c in zip(*np.unique(content, return_counts=True)) if c == 2][:4]
                assert len(tw) == 4
                rest = [x for x in singles if x not in tw]
                wanted = [tw[0], tw[0], tw[1], tw[1], tw[2], tw[2], tw[3], tw[3]] + rest[:56]
            else:
                wanted = singles[:64]
            put(content, pos, wanted)
        return content
    return fn


@functools.lru_cache(maxsize=None)
def onepass_input(case_name, cls):
    """One level-1 bucket (top byte 0x9A): the case's 16-bit task of class `cls`, a task of 12000 distinct values that fills
    the bucket past a local sort, and -- for the look cases -- a sub-bucket of 17409 keys that opens level 2."""
    case = next(c for c in OP_CASES if c.name == case_name)
    rng = np.random.default_rng(310 + cls)
    m = OP_TASK_SIZE[cls]
    if case.look == "twins":                            # four values twice, everything else once: the fullest bin holds 2
        vals = distinct_values(rng, m - 4)
        low = np.concatenate((vals, vals[:4]))
    else:                                               # one value k times, everything else once
        low = np.concatenate((np.full(case.k, case.value, np.uint64), distinct_values(rng, m - case.k, exclude=(case.value,))))
    assert low.size == m
    parts = [under((OP_TOP, OP_TASK), low), under((OP_TOP, OP_FILL), distinct_values(rng, 12000))]
    if case.look:
        parts.append(under((OP_TOP, OP_OVER), rand_low(rng, 16, CAP_MAX + 1)))
    return finish(parts, seed=310, fixups=[((OP_TOP, OP_TASK), op_fix(case, (OP_TOP, OP_TASK)))])


FD_DISTINCT = (1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
FD_PATTERN = [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4] + list(range(5, 58))          # sampled keys: one value 3 times, four twice


def fd_values(rng, size, D):
    """`size` 16-bit values, exactly D distinct ones (all ones among them), skewed multiplicities, every value present."""
    vals = np.concatenate(([0xFFFF], distinct_values(rng, D - 1, exclude=(0xFFFF,)))).astype(np.uint64)
    idx = np.minimum((rng.random(size) ** 2 * D).astype(np.int64), D - 1)
    idx[:D] = np.arange(D)
    return vals[idx], vals


def fd_fix(vals, pre):
    def fn(content):
        wanted = [np.uint32(_prefix(pre) << 16 | int(vals[j % vals.size])) for j in FD_PATTERN]
        return put(content, sample_positions(content.size), wanted)
    return fn


@functools.lru_cache(maxsize=None)
def few_distinct_input(pairs):
    """16-bit tasks of level 1 with exactly D distinct values, D in FD_DISTINCT, in every class where the few-distinct plan is
    compiled (sizes cap and cap - 1 in turn), next to a sub-bucket of 17409 keys (skew: the look runs).  Among every task's 64
    sampled keys one value shows 3 times and four show twice: LS_FLAG and LS_DD, which both entrances of the plan need.
    Returns (images, [(class, D, prefix, size)])."""
    rng = np.random.default_rng(320 + int(pairs))
    parts, info, fix = [], [], []
    for top, cls in zip((0x22, 0x8D, 0xE1), dedupe_classes(pairs)):
        for j, D in enumerate(FD_DISTINCT):
            size = CAPS[cls] - (j & 1)
            low, vals = fd_values(rng, size, D)
            pre = (top, 2 * j + 1)
            parts.append(under(pre, low))
            info.append((cls, D, pre, size))
            fix.append((pre, fd_fix(vals, pre)))
        parts.append(under((top, 0xFE), rand_low(rng, 16, CAP_MAX + 1)))
    return finish(parts, seed=320, fixups=fix), info


# --------------------------------------------------------------------------------------------------- coverage --
def coverage(pairs):
    """{(level, class, bits)} of every task over all inputs of this module, from the restatement."""
    seen = set()
    imgs = [img for _, _, img in classify_inputs()] + [hh_input(1)[0], hh_input(2)[0], few_distinct_input(pairs)[0]]
    imgs += [single_task_input(n) for n in SINGLE_SIZES]
    imgs += [onepass_input(c.name, cls) for c in OP_CASES for cls in onepass_classes(pairs)]
    for img in imgs:
        seen |= {(t.level, t.cls, t.bits) for t in restate_cached(img).tasks}
    return seen


_RESTATED = {}


def restate_cached(img, pivot=True):
    """restate(), remembered per input (the inputs are frozen arrays that live as long as the process)."""
    key = (id(img), pivot)
    if key not in _RESTATED:
        _RESTATED[key] = (img, restate(img, pivot))
    return _RESTATED[key][1]
