"""gs_msb_sort_wide path by path: every level depth, both task classes at and next to their caps, merged tasks, and the two
plans of the wide local sort on both sides of the crowded-bin limit.

The inputs are BUILT so that the classification of every level is known: they are laid out in the order-preserving image of
the key type (test_buffer_contracts_gpu.ordmap) and mapped back, so the float rows hold negative keys, -0.0 and NaN
patterns as ordinary keys.  gs_msb_wide_census reads back what every level did, and `wide_restatement` below says what it
must have done: the classification rule of oracle.msb_classify_counts (reference rules: oracle/oracle.py, "M4") with the wide
geometry -- caps 2048 / 8192, merge threshold 3000, no heavy-hitter rule, no tasks at the last level.

The builders, the restatement and the assertions about the inputs themselves need no GPU; tests/test_msb_wide_paths_cpu.py
runs them."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_buffer_contracts_gpu import F32, F64, I64, KEY_BYTES, U32, U64, UINT, check_unstable, ordmap, stable_order

pytestmark = pytest.mark.gpu

ROWS = [(U64, 0), (I64, 4), (F64, 8), (U64, 8), (U32, 8), (F32, 8)]                 # (key type, value bytes)
ROW_IDS = ["u64", "i64_u32", "f64_u64", "u64_u64", "u32_u64", "f32_u64"]
SWITCH_ROWS = [(U64, 0), (F64, 8), (U64, 4)]

WIDE_CAPS = (2048, 8192)            # MsbWs::caps of the wide geometry (MW_CAP)
WIDE_MERGE = 3000                   # MSB_MERGE
WIDE_TILE = 4096                    # MW_TILE
BINS, BIN_BITS, BIN_LIMIT = 2048, 11, 24      # the order-free plan: abandoned when a bin holds BIN_LIMIT keys or more


# ------------------------------------------------------------------------------------------------- key images --
def from_image(img, kt):
    """Keys of type kt (as unsigned bit patterns) whose order-preserving image is img: the inverse of ordmap."""
    bits = 8 * KEY_BYTES[kt]
    sign, mask = np.uint64(1 << (bits - 1)), np.uint64((1 << bits) - 1)
    img = img.astype(np.uint64)
    if kt in (I64,):
        k = img ^ sign
    elif kt in (F32, F64):
        k = np.where(img & sign != 0, img ^ sign, ~img & mask)
    else:
        k = img
    return k.astype(UINT[KEY_BYTES[kt]])


# ------------------------------------------------------------------------------------------------ restatement --
def wide_classify_counts(counts, offset, rb, caps=WIDE_CAPS, merge=WIDE_MERGE):
    """One bucket with its 256 sub-bucket counts, starting at `offset`, `rb` key bits below this level's byte: returns
    (next-level buckets [(offset, size)], tasks [(class, offset, size, sort_bits, sub-buckets)]).  A sub-bucket is empty,
    larger than the largest cap (a bucket of the next level; it ends a run) or local; adjacent local sub-buckets merge while
    the sum stays below `merge`; a merged range sorts this level's byte again; first class whose cap holds the range."""
    buckets, tasks = [], []
    starts = offset + np.concatenate(([0], np.cumsum(counts[:-1]))).astype(np.int64)
    run = None                      # [start offset, sum, non-empty sub-buckets]

    def flush():
        nonlocal run
        if run is not None:
            cls = next(c for c, cap in enumerate(caps) if run[1] <= cap)
            tasks.append((cls, int(run[0]), int(run[1]), rb + (8 if run[2] > 1 else 0), run[2]))
            run = None

    for d in range(256):
        c = int(counts[d])
        if c == 0:
            continue
        if c > caps[-1]:
            flush()
            buckets.append((int(starts[d]), c))
            continue
        if run is not None and run[1] + c < merge:
            run[1] += c
            run[2] += 1
        else:
            flush()
            run = [starts[d], c, 1]
    flush()
    return buckets, tasks


def wide_tiles_of(off, size):
    """Tile records of a bucket (ws_first_tile / ws_tiles_of_at): a bucket of 256 tiles or more that starts off a 64-element
    boundary gets a short first tile."""
    r = off & 63
    first = min(size, WIDE_TILE) if (r == 0 or size < 256 * WIDE_TILE) else WIDE_TILE - r
    return 1 + -(-(size - first) // WIDE_TILE)


def _zero_record():
    return {"buckets": 0, "tiles": 0, "keys": 0, "task_keys": 0, "tasks": [0, 0, 0, 0]}


def wide_restatement(img, key_bits, caps=WIDE_CAPS, merge=WIDE_MERGE):
    """What gs_msb_sort_wide does with keys whose order-preserving images are `img`: (census, tasks).  census: 8 records
    with the fields of gs_msb_wide_census that depend on the input; tasks: dicts (level, cls, offset, size, sort_bits,
    merged).  The levels are walked as oracle.msb_level_lists walks them; a bucket's digit counts do not depend on the
    order of its keys, so its content is read from the sorted images at its offset."""
    levels, n = key_bits // 8, int(img.size)
    cen = [_zero_record() for _ in range(8)]
    tasks = []
    if n == 0:
        return cen, tasks
    if n <= caps[-1]:                          # one task on all bits, no classification: task_keys is not written (0)
        cls = 0 if n <= caps[0] else 1
        cen[0].update(buckets=1, tiles=-(-n // WIDE_TILE), keys=n)
        cen[0]["tasks"][cls] = 1
        tasks.append(dict(level=0, cls=cls, offset=0, size=n, sort_bits=key_bits, merged=False))
        return cen, tasks
    S = np.sort(img.astype(np.uint64))
    level_buckets = [(0, n)]
    for L in range(levels):
        if not level_buckets:
            break
        c = cen[L]
        c["buckets"] = len(level_buckets)
        c["tiles"] = -(-n // WIDE_TILE) if L == 0 else sum(wide_tiles_of(o, s) for o, s in level_buckets)
        c["keys"] = sum(s for _, s in level_buckets)
        if L == levels - 1:                    # the last scatter finishes every key it gets
            break
        rb = key_bits - 8 - 8 * L
        nxt = []
        for off, size in level_buckets:
            digit = ((S[off:off + size] >> np.uint64(rb)) & np.uint64(0xff)).astype(np.int64)
            b, t = wide_classify_counts(np.bincount(digit, minlength=256), off, rb, caps, merge)
            nxt += b
            for cls, o, s, bits, nsub in t:
                c["tasks"][cls] += 1
                c["task_keys"] += s
                tasks.append(dict(level=L, cls=cls, offset=o, size=s, sort_bits=bits, merged=nsub > 1))
        level_buckets = nxt
    return cen, tasks


def fullest_bin(task_img, sort_bits):
    """Keys in the fullest of the 2048 bins of the order-free plan: the bins are the top 11 of the task's sort bits."""
    b = (task_img.astype(np.uint64) >> np.uint64(sort_bits - BIN_BITS)) & np.uint64(BINS - 1)
    return int(np.bincount(b.astype(np.int64), minlength=BINS).max())


def task_fullest_bins(img, tasks):
    """fullest_bin of every task of wide_restatement that has more than 16 bits to sort (the tasks the order-free plan may take)."""
    S = np.sort(img.astype(np.uint64))
    return [(t, fullest_bin(S[t["offset"]:t["offset"] + t["size"]], t["sort_bits"])) for t in tasks if t["sort_bits"] > 16]


def assert_census(got, exp, what):
    """Level by level: buckets, tiles, keys, task_keys, tasks; no overflow, no heavy hitters, nothing past the key's levels."""
    for L in range(8):
        g, e = got[L], exp[L]
        for f in ("buckets", "tiles", "keys", "task_keys", "tasks"):
            assert g[f] == e[f], f"{what}: level {L} {f}: census {g[f]}, restatement {e[f]}"
        assert g["overflow"] == 0 and g["pivot_buckets"] == 0 and g["pivot_keys"] == 0 and g["flagged"] == 0, f"{what}: level {L} {g}"


# ------------------------------------------------------------------------------------------------------ ladder --
LADDER_COUNTS = (2999, 1, 5, 700, 8193, 2047, 2048, 2049, 1500, 1499, 8192, 8191, 3000, 4096)
# After one empty digit, a pair that sums to the threshold exactly and so must stay two tasks.  The counts above alone leave
# a threshold of 3001 invisible to a census of task counts: 2999 + 1 would merge, but into tasks of 3000 and 705 keys, which
# fall into the same classes as 2999 and 706.
LADDER_PAIR = (2000, 1000)
FIXED = (0x00, 0xFF, 0xA5)
LADDER_TOP = {1: 0x00, 2: 0xFF, 3: 0xA5, 4: 0x80, 5: 0x3C, 6: 0xC3}     # top byte of the group of depth d; depth 0: 0x40..0x50
LADDER_DEEP, LADDER_EQUAL = 20000, 9000


def _rand_bits(rng, bits, m):
    return rng.integers(0, 1 << bits, size=m, dtype=np.uint64) if bits else np.zeros(m, np.uint64)


def _prefix(bytes_):
    p = 0
    for b in bytes_:
        p = (p << 8) | b
    return p


@functools.lru_cache(maxsize=None)
def build_ladder(key_bits):
    """The depth ladder as order-preserving images (uint64, shuffled).  Group d (0 .. levels-2) holds its top d bytes
    constant and gives the byte of level d the consecutive digits of LADDER_COUNTS (and LADDER_PAIR); the bytes below are random.  One more
    group differs in the lowest byte only, and one run of equal images has all bits below the top byte set (as doubles:
    -0.0): both reach the last scatter."""
    rng = np.random.default_rng(key_bits)
    levels = key_bits // 8
    parts = []
    for d in range(levels - 1):
        fixed = [LADDER_TOP[d]] + [FIXED[(d + j + 1) % 3] for j in range(1, d)] if d else []
        start = 0x40 if d == 0 else (0, 239, 0x60)[d % 3]
        rb = key_bits - 8 - 8 * d
        digits = list(range(len(LADDER_COUNTS))) + [len(LADDER_COUNTS) + 1, len(LADDER_COUNTS) + 2]
        for i, c in zip(digits, LADDER_COUNTS + LADDER_PAIR):
            parts.append(np.uint64(_prefix(fixed + [start + i]) << rb) | _rand_bits(rng, rb, c))
    deep = [0x7E] + [FIXED[j % 3] for j in range(levels - 2)]
    parts.append(np.uint64(_prefix(deep) << 8) | _rand_bits(rng, 8, LADDER_DEEP))
    parts.append(np.full(LADDER_EQUAL, (0x7F << (key_bits - 8)) | ((1 << (key_bits - 8)) - 1), np.uint64))
    img = np.concatenate(parts)
    rng.shuffle(img)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ladder_restatement(key_bits):
    return wide_restatement(build_ladder(key_bits), key_bits)


def assert_ladder_reaches_every_level(key_bits, tasks):
    """Every level 0 .. levels-2 emits at least one task of each class and at least one merged task."""
    for L in range(key_bits // 8 - 1):
        at = [t for t in tasks if t["level"] == L]
        for cls in (0, 1):
            assert any(t["cls"] == cls for t in at), f"no task of class {cls} at level {L}"
        assert any(t["merged"] for t in at), f"no merged task at level {L}"
        sizes = {t["size"] for t in at if not t["merged"]}
        assert {2047, 2048, 2049, 8191, 8192, 3000, 2999, 4096, 2000, 1000} <= sizes, f"level {L}: unmerged sizes {sorted(sizes)}"
        assert {706, 2999} <= {t["size"] for t in at if t["merged"]}, f"level {L}: merged sizes"


# ----------------------------------------------------------------------------------------------- plan boundary --
SIZES = (1, 2, 511, 2048, 2049, 8191, 8192)
FULLEST = (22, 23, 24, 25)
BIN_AT = {"first": 0, "last": BINS - 1, "mid": 1000}
COMPOSITIONS = ("equal", "distinct", "half")


def task_values(sb, size, k, binpos, comp, rng):
    """`size` values of `sb` bits (>= 16) whose fullest bin -- bin BIN_AT[binpos] of the top 11 bits -- holds exactly
    min(k, size) of them: all equal, all distinct, or half and half.  The other values are dealt out over the other bins
    (at most 4 each) and are distinct inside a bin, so a "distinct" task holds no two equal values at all.  The equal value
    of the last bin is all ones: what a pad looks like inside a local sort.  (A bin of equal keys only comes out right whatever
    ranks its keys get; "half" puts other keys next to them, so that a wrong rank among equal keys moves a key that differs.)"""
    lb = sb - BIN_BITS
    lm = (1 << lb) - 1
    step = (int(rng.integers(0, 1 << lb)) | 1) & lm
    B = BIN_AT[binpos]
    kk = min(k, size)
    v = {"first": 0, "last": lm, "mid": int(rng.integers(0, 1 << lb))}[binpos]
    j = np.arange(kk, dtype=np.int64)
    if comp == "equal":
        low = np.full(kk, v, np.int64)
    elif comp == "distinct":
        low = v + j * step
    else:
        low = np.where(j < kk // 2, v, v + (j + 1) * step)
    crowded = (np.uint64(B) << np.uint64(lb)) | (low.astype(np.uint64) & np.uint64(lm))
    m = size - kk
    others = np.array([b for b in rng.permutation(BINS) if b != B], np.int64)
    assert m <= 4 * others.size and 4 < min(FULLEST) and (kk + 1) <= (1 << lb)
    i = np.arange(m, dtype=np.int64)
    ob = others[i % others.size]
    base = rng.integers(0, 1 << lb, size=BINS, dtype=np.int64)
    olow = (base[ob] + (i // others.size) * step).astype(np.uint64) & np.uint64(lm)
    return np.concatenate((crowded, (ob.astype(np.uint64) << np.uint64(lb)) | olow))


def all_ones_values(sb, size, rng):
    """A task the order-free plan abandons, full of values whose `sb` bits are all ones (4 of 5; the others share their bin)."""
    lb = sb - BIN_BITS
    v = np.full(size, (1 << sb) - 1, np.uint64)
    idx = rng.permutation(size)[:size // 5]
    v[idx] = (np.uint64(BINS - 1) << np.uint64(lb)) | _rand_bits(rng, lb, idx.size)
    return v


def embed_tasks(key_bits, cases, seed):
    """One array (order-preserving images, shuffled) that holds every case as an UNMERGED task of level `depth`: the case's
    values are the low bits under a prefix of `depth` bytes (top byte `top`, then FIXED bytes) and the digit `digit` at
    level `depth`; sub-buckets of 3000 random keys at the digits `flank` keep the task from merging and push the bucket
    past the largest local sort, so that it is partitioned down to that level.  Depth 0: `digit` and `flank` are top bytes.
    cases: dicts with label, depth, digit, flank, values (a function of (sort_bits, rng)) and, for depth >= 1, top.
    Returns (images, [(label, depth, sort_bits, prefix of the task, lowest and highest top byte of the case)])."""
    rng = np.random.default_rng(seed)
    parts, info = [], []
    for c in cases:
        d = c["depth"]
        sb = key_bits - 8 - 8 * d
        fixed = [c["top"]] + [FIXED[(c["top"] + j) % 3] for j in range(1, d)] if d else []
        vals = c["values"](sb, rng)
        assert vals.size + 3000 * len(c["flank"]) > WIDE_CAPS[-1] or d == 0
        tp = _prefix(fixed + [c["digit"]])
        parts.append(np.uint64(tp << sb) | vals)
        for fd in c["flank"]:
            parts.append(np.uint64(_prefix(fixed + [fd]) << sb) | _rand_bits(rng, sb, 3000))
        tops = [c["top"]] if d else [c["digit"]] + list(c["flank"])
        info.append((c["label"], d, sb, tp, min(tops), max(tops)))
    img = np.concatenate(parts)
    rng.shuffle(img)
    return img, info


def assert_embedded(key_bits, img, info, tasks, expect_fullest):
    """Every case of embed_tasks is an unmerged task of its level in the restatement, and its fullest bin is what its label
    says (expect_fullest[label]; None: not asserted)."""
    S = np.sort(img)
    by_off = {(t["level"], t["offset"]): t for t in tasks}
    for label, d, sb, tp, _, _ in info:
        lo = int(np.searchsorted(S, np.uint64(tp << sb), side="left"))
        hi = int(np.searchsorted(S, np.uint64(((tp + 1) << sb) - 1), side="right"))
        t = by_off.get((d, lo))
        assert t is not None and t["size"] == hi - lo and t["sort_bits"] == sb and not t["merged"], f"{label}: {t}"
        if expect_fullest.get(label) is not None:
            assert fullest_bin(S[lo:hi], sb) == expect_fullest[label], label


def level1_cases(key_bits, k, sizes=SIZES):
    """Tasks of level 1 (48 sort bits under a 64-bit key): every size x bin position x composition with a fullest bin of k."""
    cases, fullest = [], {}
    for size in sizes:
        for binpos in BIN_AT:
            for comp in COMPOSITIONS:
                idx = len(cases)
                label = f"L1 size={size} k={k} bin={binpos} {comp}"
                digit = (1, 100, 253)[idx % 3]
                cases.append(dict(label=label, depth=1, top=(37 * idx + 5) % 256, digit=digit, flank=(digit - 1, digit + 1, digit + 2),
                                  values=functools.partial(_tv, size, k, binpos, comp)))
                fullest[label] = min(k, size)
    return cases, fullest


def _tv(size, k, binpos, comp, sb, rng):
    return task_values(sb, size, k, binpos, comp, rng)


def deep_cases(key_bits):
    """Tasks with 24, 32 and 40 bits left (and the level-0 task: all bits below the top byte), a crowded and an uncrowded
    variant each at a size that leaves pads; and a level-1 task full of images whose sort bits are all ones (under top byte
    0x7F: as doubles, -0.0)."""
    cases, fullest = [], {}
    depths = [0] + [d for d in range(2, key_bits // 8) if 24 <= key_bits - 8 - 8 * d <= 40]
    for d in depths:
        for k, binpos, comp in ((22, "mid", "half"), (23, "last", "equal"), (25, "first", "half"), (24, "last", "equal")):
            idx = len(cases)
            label = f"L{d} bits={key_bits - 8 - 8 * d} size=5000 k={k} bin={binpos} {comp}"
            if d == 0:                                    # top bytes 8.., 16.., 24.., 32..: below the tops of the deeper cases
                digit = 8 * (idx + 1)
                cases.append(dict(label=label, depth=0, digit=digit, flank=(digit - 1, digit + 1), values=functools.partial(_tv, 5000, k, binpos, comp)))
            else:
                digit = (1, 100, 253)[idx % 3]
                cases.append(dict(label=label, depth=d, top=64 + 3 * idx, digit=digit, flank=(digit - 1, digit + 1, digit + 2),
                                  values=functools.partial(_tv, 5000, k, binpos, comp)))
            fullest[label] = k
    cases.append(dict(label="L1 all ones size=5000", depth=1, top=0x7F, digit=255, flank=(253, 254),
                      values=lambda sb, rng: all_ones_values(sb, 5000, rng)))
    fullest["L1 all ones size=5000"] = None
    return cases, fullest


@functools.lru_cache(maxsize=None)
def level1_input(key_bits, k, sizes=SIZES):
    """(images, case info, expected fullest bins, restatement) of the level-1 cases."""
    cases, fullest = level1_cases(key_bits, k, sizes)
    img, info = embed_tasks(key_bits, cases, seed=100 + k)
    img.setflags(write=False)
    return img, info, fullest, wide_restatement(img, key_bits)


@functools.lru_cache(maxsize=None)
def deep_input(key_bits):
    cases, fullest = deep_cases(key_bits)
    img, info = embed_tasks(key_bits, cases, seed=7)
    img.setflags(write=False)
    return img, info, fullest, wide_restatement(img, key_bits)


@functools.lru_cache(maxsize=None)
def single_task_inputs(key_bits, k):
    """Arrays that are one task on all key bits: [(label, images, fullest bin)], every size x bin position x composition, and
    one of 5000 images that are all ones (the abandoned task's pads look the same)."""
    rng = np.random.default_rng(1000 + k)
    out = []
    for size in SIZES:
        for binpos in BIN_AT:
            for comp in COMPOSITIONS:
                img = task_values(key_bits, size, k, binpos, comp, rng)
                rng.shuffle(img)
                out.append((f"single size={size} k={k} bin={binpos} {comp}", img, min(k, size)))
    out.append(("single all ones size=5000", all_ones_values(key_bits, 5000, rng), None))
    return out


def failing_cases(got_img, exp_img, info, key_bits):
    """Labels of the embedded cases in whose range of top bytes the sorted images differ."""
    bad = []
    top = (exp_img >> np.uint64(key_bits - 8)).astype(np.int64)
    for label, _, _, _, t_lo, t_hi in info:
        lo, hi = np.searchsorted(top, t_lo, side="left"), np.searchsorted(top, t_hi, side="right")
        if not np.array_equal(got_img[lo:hi], exp_img[lo:hi]):
            bad.append(label)
    return bad


# ----------------------------------------------------------------------------------------------------- running --
def make_values(n, vb, mode, rng):
    if not vb:
        return None
    if mode == "enumerated":
        return np.arange(n, dtype=UINT[vb])
    return rng.integers(0, 1 << (8 * vb), size=n, dtype=np.uint64).astype(UINT[vb])


def run_sort(dev, keys, kt, vals, dm=None):
    """gs_msb_sort_wide on `keys` (bit patterns of key type kt) and `vals`: (sorted keys, sorted values, census, workspace)."""
    from gpu_sort_amd.msb import msb_wide_census, rdxsrt_unstable_sort_wide
    kb, n = KEY_BYTES[kt], keys.size
    vb = vals.dtype.itemsize if vals is not None else 0
    signed = {4: np.int32, 8: np.int64}
    dk = torch.from_numpy(keys.view(signed[kb]).copy()).to(dev)
    dv = torch.from_numpy(vals.view(signed[vb]).copy()).to(dev) if vb else None
    seq, dm = rdxsrt_unstable_sort_wide(dk, dv, n, torch.empty_like(dk), torch.empty_like(dv) if vb else None, key_type=kt, dm=dm)
    got_k = seq.sorted_keys.cpu().numpy().view(UINT[kb])
    got_v = seq.sorted_values.cpu().numpy().view(UINT[vb]) if vb else None
    return got_k, got_v, msb_wide_census(dm, n, kb, vb), dm


def check_result(keys, kt, vals, mode, got_k, got_v, what):
    """Keys bit for bit against numpy's stable argsort of the order map; enumerated values a permutation that names equal
    keys; random values the same multiset inside every run of equal keys (tests/test_msb_wide_gpu.py::_check)."""
    if vals is None or mode == "enumerated":
        check_unstable(keys, kt, got_k, got_v, what)
        return
    order = stable_order(keys, kt)
    exp, ev = keys[order], vals[order]
    assert np.array_equal(got_k, exp), what + ": keys differ from the reference"
    run_id = np.cumsum(np.concatenate(([0], exp[1:] != exp[:-1])))
    a, b = np.lexsort((ev, run_id)), np.lexsort((got_v, run_id))
    assert np.array_equal(ev[a], got_v[b]), what + ": the values of a run of equal keys differ from the input's"


def sort_and_check(dev, img, kt, vb, mode, what, census=None, dm=None, seed=0):
    keys = from_image(img, kt)
    vals = make_values(keys.size, vb, mode, np.random.default_rng(seed))
    got_k, got_v, cen, dm = run_sort(dev, keys, kt, vals, dm)
    check_result(keys, kt, vals, mode, got_k, got_v, what)
    if census is not None:
        assert_census(cen, census, what)
    return got_k, cen, dm


def value_modes(rows=ROWS, ids=ROW_IDS):
    """(row, mode) pairs: keys-only rows once, pairs rows with enumerated and with random values."""
    out = []
    for (kt, vb), name in zip(rows, ids):
        for mode in (("enumerated", "random") if vb else ("none",)):
            out.append(pytest.param(kt, vb, mode, id=f"{name}-{mode}"))
    return out


# ------------------------------------------------------------------------------------------------------- tests --
@pytest.mark.parametrize("kt,vb", ROWS, ids=ROW_IDS)
def test_depth_ladder(gs, cuda, kt, vb):
    """Tasks of known sizes at every level 0 .. levels-2, a group and a run of equal keys for the last scatter: the result is
    right and every level's census is the restatement's."""
    key_bits = 8 * KEY_BYTES[kt]
    img = build_ladder(key_bits)
    cen, tasks = ladder_restatement(key_bits)
    assert_ladder_reaches_every_level(key_bits, tasks)            # on the CPU, before the GPU is touched
    assert cen[key_bits // 8 - 1]["buckets"] >= 3 and cen[key_bits // 8 - 1]["keys"] >= LADDER_DEEP + LADDER_EQUAL + 8193
    sort_and_check(cuda, img, kt, vb, "enumerated", "ladder", cen)


@pytest.mark.parametrize("k", FULLEST)
@pytest.mark.parametrize("kt,vb,mode", value_modes())
def test_plan_boundary_single_tasks(gs, cuda, kt, vb, mode, k):
    """Arrays of one task on all key bits (keys only: the order-free plan unless a bin holds 24 keys), every size class edge,
    fullest bin k at the first, the last or a middle bin, of equal, distinct or half equal keys."""
    key_bits = 8 * KEY_BYTES[kt]
    for i, (label, img, full) in enumerate(single_task_inputs(key_bits, k)):
        if full is not None:
            assert fullest_bin(img, key_bits) == full, label
        cen, _ = wide_restatement(img, key_bits)
        sort_and_check(cuda, img, kt, vb, mode, label, cen, seed=i)


@pytest.mark.parametrize("k", FULLEST)
@pytest.mark.parametrize("kt,vb,mode", value_modes())
def test_plan_boundary_level1_tasks(gs, cuda, kt, vb, mode, k):
    """The same tasks one level down, inside a larger array (64-bit keys: 48 sort bits, so the pairs rows take the order-free
    plan too, with the element's index packed under the key)."""
    key_bits = 8 * KEY_BYTES[kt]
    img, info, fullest, (cen, tasks) = level1_input(key_bits, k)
    assert_embedded(key_bits, img, info, tasks, fullest)
    keys = from_image(img, kt)
    vals = make_values(keys.size, vb, mode, np.random.default_rng(k))
    got_k, got_v, got_cen, _ = run_sort(cuda, keys, kt, vals)
    bad = failing_cases(ordmap(got_k, kt), np.sort(img), info, key_bits)
    assert not bad, f"keys differ from the reference in {len(bad)} cases: {bad}"
    check_result(keys, kt, vals, mode, got_k, got_v, f"level-1 tasks k={k}")
    assert_census(got_cen, cen, f"level-1 tasks k={k}")


@pytest.mark.parametrize("kt,vb,mode", value_modes())
def test_plan_boundary_deep_tasks_and_all_ones(gs, cuda, kt, vb, mode):
    """Tasks with 24, 32 and 40 bits left (bin shifts 13, 21, 29) and the level-0 task, crowded and uncrowded, at a size that
    leaves pads; and an abandoned task full of keys whose sort bits are all ones, which only their place in the order the
    stable passes keep tells from the pads (as doubles: -0.0)."""
    key_bits = 8 * KEY_BYTES[kt]
    img, info, fullest, (cen, tasks) = deep_input(key_bits)
    assert_embedded(key_bits, img, info, tasks, fullest)
    if kt == F64:
        assert np.count_nonzero(from_image(img, kt) == np.uint64(1 << 63)) >= 4000          # -0.0
    sort_and_check(cuda, img, kt, vb, mode, "deep tasks", cen, seed=3)


def switch_inputs(kt):
    key_bits = 8 * KEY_BYTES[kt]
    return [("ladder", build_ladder(key_bits)), ("level-1 k=23", level1_input(key_bits, 23, (511, 8192))[0]),
            ("level-1 k=24", level1_input(key_bits, 24, (511, 8192))[0])]


def switch_child_report():
    """Runs in a child process (the switches are read once per process): sorts the ladder and boundary inputs for SWITCH_ROWS,
    checks every result against numpy and returns [[row, input, right, census]]."""
    dev = torch.device("cuda:0")
    out = []
    for kt, vb in SWITCH_ROWS:
        for name, img in switch_inputs(kt):
            right, cen = True, None
            try:
                _, cen, _ = sort_and_check(dev, img, kt, vb, "enumerated", name)
            except AssertionError as e:
                right = str(e)
            out.append([[kt, vb], name, right, cen])
    return out


@pytest.mark.parametrize("switch", ["GS_MSB_WIDE_FAST", "GS_MSB_PEEK"])
def test_switches_do_not_change_results(switch):
    """GS_MSB_WIDE_FAST=0 (every task takes the LSD passes) and GS_MSB_PEEK=0 (every level launches, with worst-case grids, on
    lists that are mostly empty) against the defaults, one child process per setting: every result right, the same census."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys, json\nsys.path[:0] = [%r, %r]\nimport test_msb_wide_paths_gpu as P\n"
              "print(json.dumps(P.switch_child_report()))\n") % (root, os.path.join(root, "tests"))
    res = {}
    for setting in ("0", "1"):
        env = dict(os.environ, **{switch: setting})
        r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, f"{switch}={setting}: {r.stderr[-2000:]}"
        res[setting] = json.loads(r.stdout.strip().splitlines()[-1])
    for setting, rep in res.items():
        assert len(rep) == len(SWITCH_ROWS) * 3
        for row, name, right, cen in rep:
            assert right is True, f"{switch}={setting} {row} {name}: {right}"
    assert res["0"] == res["1"]
    for (row, name, _, cen) in res["0"]:                              # ... and it is the restatement's
        assert_census(cen, wide_restatement(dict(switch_inputs(row[0]))[name], 8 * KEY_BYTES[row[0]])[0], f"{switch}=0 {row} {name}")


@pytest.mark.parametrize("kt,vb", ROWS, ids=ROW_IDS)
def test_workspace_reuse_across_depth_profiles(gs, cuda, kt, vb):
    """One workspace, three sorts of the same size back to back: the ladder (every level), uniform keys (level 0 or 1 only), equal
    keys (every level, no tasks), and uniform keys again.  A level record of a deeper sort must not show in a shallower one."""
    key_bits = 8 * KEY_BYTES[kt]
    ladder = build_ladder(key_bits)
    n = ladder.size
    rng = np.random.default_rng(5)
    uniform = _rand_bits(rng, key_bits, n)
    equal = np.full(n, 0x5A5A5A5A5A5A5A5A & ((1 << key_bits) - 1), np.uint64)
    ucen = wide_restatement(uniform, key_bits)[0]
    ecen = wide_restatement(equal, key_bits)[0]
    assert ucen[2]["buckets"] == 0 and all(ecen[L]["buckets"] == 1 and ecen[L]["tasks"] == [0, 0, 0, 0] for L in range(key_bits // 8))
    dm = None
    for name, img, cen in (("ladder", ladder, ladder_restatement(key_bits)[0]), ("uniform", uniform, ucen), ("equal", equal, ecen),
                           ("uniform again", uniform, ucen)):
        _, _, dm2 = sort_and_check(cuda, img, kt, vb, "enumerated", "reuse: " + name, cen, dm=dm)
        assert dm is None or dm2 is dm
        dm = dm2
