"""The three kernels of one LSB pass -- upsweep, spine scan, downsweep (gs_lsb_upsweep.inc, gs_lsb.hip, gs_lsb_downsweep.inc) --
restated in numpy, with the case tables and input builders of tests/test_lsb_stages_gpu.py and the "plausible wrong kernels"
that tests/test_lsb_stages_cpu.py holds those tables against.  No GPU, no torch.

Keys are uint32 bit patterns throughout.  A key's IMAGE is twiddle_in(key): the unsigned word whose order is the key order;
the digit of a pass is a bit field of the image."""
import functools
import itertools

import numpy as np

U32, I32, F32 = 0, 1, 2                 # GS_KEY_U32 / I32 / F32
KT_NAME = {U32: "U32", I32: "I32", F32: "F32"}
TILE, TPC, RADIX = 8192, 8, 256         # gs_lsb_geometry's tile and tiles per chunk (the tests hold them against the call)
CHUNK = TILE * TPC
BATCH, WAVE = 4096, 64                  # the upsweep loads 64 keys per lane at a time; it samples loads 0 and 32 of a batch
SCAN_SEG = 1024                         # lsb_scan_kernel sweeps a row in segments of 1024 entries
ONES = np.uint32(0xFFFFFFFF)
SIGN = np.uint32(0x80000000)

F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,        # +-0, +-inf
                         0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,        # denormals
                         0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFC12345],   # NaNs of both signs
                        dtype=np.uint32)


# ------------------------------------------------------------------------------------------------- key images --
def xor_mask(kt, descending):
    """lsb_twiddle_masks: the sign flip of I32 and the complement of a descending sort, as one xor."""
    return np.uint32((0x80000000 if kt == I32 else 0) ^ (0xFFFFFFFF if descending else 0))


def twiddle_in(keys, kt, descending):
    """lsb_twiddle_masks(first = true) + twiddle_in: F32 flips all bits of a negative and the sign of the rest, then the xor."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    if kt == F32:
        k = k ^ np.where(k & SIGN != 0, ONES, SIGN)
    return k ^ xor_mask(kt, descending)


def twiddle_out(img, kt, descending):
    """lsb_twiddle_masks(last = true) + twiddle_out: the inverse of twiddle_in for the same type and direction."""
    k = np.ascontiguousarray(img, dtype=np.uint32) ^ xor_mask(kt, descending)
    if kt == F32:
        k = k ^ np.where(k & SIGN != 0, SIGN, ONES)
    return k


def digit_of_image(img, shift, bits):
    return (img >> np.uint32(shift)) & np.uint32((1 << bits) - 1)


def digit(keys, key_type_in, descending, shift, bits):
    return digit_of_image(twiddle_in(keys, key_type_in, descending), shift, bits)


# ---------------------------------------------------------------------------------------------------- geometry --
def num_tiles(n):
    return (n + TILE - 1) // TILE


def grid_of(n):
    return max(1, (num_tiles(n) + TPC - 1) // TPC)


def items_for_grid(grid):
    """The smallest num_items whose spine rows have `grid` entries."""
    return (grid - 1) * CHUNK + 1


# ----------------------------------------------------------------------------------------------------- upsweep --
def tile_counts(dig, width=RADIX):
    """[tile][d]: how many keys of the tile have digit d."""
    n = dig.size
    t = np.arange(n, dtype=np.int64) // TILE
    return np.bincount(t * width + dig.astype(np.int64), minlength=num_tiles(n) * width).reshape(num_tiles(n), width)


def spine_and_prefix16(counts):
    """Per-tile counts -> (spine[256][grid] u32: the chunk's count of d; prefix16[tile][256] u16: the count of d in the chunk's
    earlier tiles)."""
    tiles, g = counts.shape[0], max(1, (counts.shape[0] + TPC - 1) // TPC)
    padded = np.zeros((g * TPC, RADIX), dtype=np.int64)
    padded[:tiles] = counts
    per_chunk = padded.reshape(g, TPC, RADIX)
    before = np.cumsum(per_chunk, axis=1) - per_chunk
    assert before.max(initial=0) < 1 << 16
    spine = np.ascontiguousarray(per_chunk.sum(axis=1).T).astype(np.uint32)
    return spine, before.reshape(g * TPC, RADIX)[:tiles].astype(np.uint16)


def upsweep(keys, key_type_in, descending, shift, bits):
    return spine_and_prefix16(tile_counts(digit(keys, key_type_in, descending, shift, bits)))


# -------------------------------------------------------------------------------------------------------- scan --
def scan(spine):
    """Row-exclusive prefix and row totals of a [256][grid] u32 array, computed in uint64; every total must fit 32 bits."""
    s = np.asarray(spine).astype(np.uint64)
    inc = np.cumsum(s, axis=1, dtype=np.uint64)
    totals = inc[:, -1]
    assert int(totals.max()) < 1 << 32, "a digit total of 2^32 or more: not a spine of a real pass"
    return (inc - s).astype(np.uint32), totals.astype(np.uint32)


# --------------------------------------------------------------------------------------------------- downsweep --
def downsweep(keys, vals, key_type_in, key_type_out, descending, shift, bits):
    """The stable scatter on one digit: keys leave as twiddle_out(twiddle_in(key)) for the in / out types."""
    img = twiddle_in(keys, key_type_in, descending)
    perm = np.argsort(digit_of_image(img, shift, bits).astype(np.uint8), kind="stable")
    return twiddle_out(img[perm], key_type_out, descending), (None if vals is None else np.ascontiguousarray(vals)[perm])


def rank_in_group(group, dig):
    """For every key, the number of earlier keys of the same group with the same digit."""
    key = group.astype(np.int64) * RADIX + dig.astype(np.int64)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    start = np.flatnonzero(np.concatenate(([True], sk[1:] != sk[:-1])))
    run = np.repeat(start, np.diff(np.concatenate((start, [sk.size]))))
    rank = np.empty(key.size, dtype=np.int64)
    rank[order] = np.arange(key.size) - run
    return rank


def destinations(dig, bits, prefix_signed=False, pads_first=False, reverse_in_wave=False):
    """Where the downsweep kernel stores every key, from the parts it uses: start of the digit (exclusive scan of the totals) +
    scanned chunk count + prefix16 + rank inside the tile; the partial last tile ends at the digit's inclusive total.  The
    three flags are wrong-kernel models (a), (f) and (e) of tests/test_lsb_stages_cpu.py.  int64, may leave [0, n)."""
    n = dig.size
    counts = tile_counts(dig)
    spine, prefix16 = spine_and_prefix16(counts)
    rows, totals = scan(spine)
    dstart = np.cumsum(totals.astype(np.int64)) - totals
    idx = np.arange(n, dtype=np.int64)
    t, d = idx // TILE, dig.astype(np.int64)
    rank = rank_in_group(t, dig)
    if reverse_in_wave:             # the lanes of one round that share a digit take their places in reverse
        g = idx // WAVE
        r = rank_in_group(g, dig)
        size = np.bincount(g * RADIX + d, minlength=(int(g[-1]) + 1) * RADIX)[g * RADIX + d]
        rank = rank - r + (size - 1 - r)
    pf = prefix16.astype(np.int16).astype(np.int64) if prefix_signed else prefix16.astype(np.int64)
    dst = dstart[d] + rows.astype(np.int64)[d, t // TPC] + pf[t, d] + rank
    full = n // TILE
    if n % TILE:
        tail = t == full
        end = dstart + totals
        dt = d[tail]
        dst[tail] = end[dt] - counts[full][dt] + rank[tail]
        if pads_first:              # the pad keys of the partial tile (largest digit) rank before its real keys of that digit
            dmax = (1 << bits) - 1
            dst[tail] += np.where(dt == dmax, TILE - n % TILE, 0)
    return dst


# ------------------------------------------------------------------------------------------- tile_of_item_wide --
XCDS, WIDE_GROUP = 8, 8192


def tile_of_item_wide(items, full_tiles):
    """gs_lsb.hpp tile_of_item_wide for an array of item indices below full_tiles: groups of 2^k items, k <= 13, the remainder
    cut into smaller powers of two; inside a group item r takes tile (r % 8) * (G / 8) + r / 8; groups below 16 are identity."""
    i = np.asarray(items, dtype=np.int64)
    out, todo = i.copy(), np.ones(i.shape, dtype=bool)
    base, rem = 0, int(full_tiles)
    while rem:
        G = WIDE_GROUP if rem >= WIDE_GROUP else 1 << (rem.bit_length() - 1)
        if G < 2 * XCDS:
            break
        span = (rem // G) * G
        m = todo & (i < base + span)
        r = (i[m] - base) % G
        out[m] = i[m] - r + (r % XCDS) * (G // XCDS) + r // XCDS
        todo &= ~m
        base, rem = base + span, rem - span
    return out


def wide_groups(full_tiles):
    """The decomposition itself: [(group size, how many)], a trailing identity remainder as (rem, 0)."""
    out, rem = [], int(full_tiles)
    while rem:
        G = WIDE_GROUP if rem >= WIDE_GROUP else 1 << (rem.bit_length() - 1)
        if G < 2 * XCDS:
            out.append((rem, 0))
            break
        out.append((G, rem // G))
        rem -= (rem // G) * G
    return out


# ---------------------------------------------------------------------------------------------- input builders --
UPSWEEP_INPUTS = ("uniform", "equal", "two_by_tile", "every", "hot_by_sample", "hot_but_one", "sample_differs")
DOWNSWEEP_INPUTS = ("uniform", "equal", "two_by_key", "two_by_tile", "every", "sorted", "reverse", "last_digit_tail",
                    "one_stranger_0", "one_stranger_max")
STABILITY_INPUTS = ("equal", "two_by_key", "two_by_tile")      # pairs: values ascending inside every digit run


def sampled_positions(n):
    """The keys the upsweep's `hot` test looks at: the first 64 and the 64 at offset 2048 of every batch of 4096."""
    pos = np.arange(n, dtype=np.int64) % BATCH
    return (pos < WAVE) | ((pos >= BATCH // 2) & (pos < BATCH // 2 + WAVE))


def digits_of(name, n, bits, rng):
    """The digit of every key of input `name` (uint32, below 2^bits)."""
    D = 1 << bits
    i = np.arange(n, dtype=np.int64)
    d0, lo, hi = (2 * D) // 3, D // 3, D - 1
    uni = rng.integers(0, D, n, dtype=np.int64)
    if name == "uniform":
        d = uni
    elif name == "equal":
        d = np.full(n, d0)
    elif name == "two_by_tile":
        d = np.where((i // TILE) & 1, hi, lo)
    elif name == "two_by_key":
        d = np.where(i & 1, hi, lo)
    elif name == "every":
        d = i % D
    elif name == "hot_by_sample":       # the sampled keys of a batch share a digit, the batch is mixed
        d = np.where(sampled_positions(n), ((i // BATCH) * 7 + 3) % D, uni)
    elif name == "hot_but_one":         # a batch of one digit with one stranger the samples do not see
        h = ((i // BATCH) * 5 + 1) % D
        d = np.where(i % BATCH == 100 + (i // BATCH) % 1000, (h + 1) % D, h)
    elif name == "sample_differs":      # one digit everywhere except at exactly the sampled positions
        d = np.where(sampled_positions(n), (d0 + 1 + i % (D - 1)) % D, d0)
    elif name == "sorted":
        d = np.sort(uni)
    elif name == "reverse":
        d = np.sort(uni)[::-1]
    elif name == "last_digit_tail":     # the partial tile holds the largest digit only
        d = np.where(i >= (n // TILE) * TILE, hi, uni)
    elif name in ("one_stranger_0", "one_stranger_max"):
        s = 0 if name.endswith("_0") else hi
        other = 1 if s == 0 else s - 1
        first = i % TILE == 0
        last = (i % TILE == TILE - 1) | (i == n - 1)
        d = np.where(first | last, s, other)
    else:
        raise ValueError(name)
    return d.astype(np.uint32)


def build_image(name, n, shift, bits, seed):
    """The keys' images (read-only): the digits of `name` in the field, random bits everywhere else."""
    return (_build_image_kept if n <= 1 << 20 else _build_image)(name, n, shift, bits, seed)


def _build_image(name, n, shift, bits, seed):
    rng = np.random.default_rng([seed, n, shift, bits, sum(map(ord, name))])
    field = np.uint32(((1 << bits) - 1) << shift)
    noise = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    img = (noise & ~field) | (digits_of(name, n, bits, rng) << np.uint32(shift))
    img.setflags(write=False)
    return img


_build_image_kept = functools.lru_cache(maxsize=100)(_build_image)      # the rows and forms of one size share their inputs


def build_keys(name, n, key_type_in, descending, shift, bits, seed=0):
    """Keys of type key_type_in whose digit (descending as given) follows input `name`.  F32 uniform keys carry the special values."""
    keys = twiddle_out(build_image(name, n, shift, bits, seed), key_type_in, descending)
    if key_type_in == F32 and name == "uniform":
        rng = np.random.default_rng([seed, n, 77])
        at = rng.permutation(n)[:F32_SPECIALS.size]
        keys[at] = F32_SPECIALS[rng.permutation(F32_SPECIALS.size)[:at.size]]
    return keys


# ------------------------------------------------------------------------------------------------- case tables --
DIGITS = ((0, 8), (8, 8), (16, 8), (24, 8), (31, 1), (29, 3), (0, 1), (5, 7), (25, 7))
UPSWEEP_TYPES = ((U32, 0), (U32, 1), (I32, 0), (I32, 1), (F32, 0), (F32, 1))      # (U32, 0): the PLAIN kernel
UPSWEEP_SIZES = (1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1, 9 * TILE, 17 * TILE + 5)
UPSWEEP_LARGE = 256 * CHUNK + TILE + 1          # 256 chunks, a tile and a key: chunk_of_block's group of 256 blocks and a ragged group
UPSWEEP_LARGE_TYPE = (U32, 0)


def upsweep_kernel_name(kt, descending):
    return "plain" if (kt, descending) == (U32, 0) else "transform"


def upsweep_cases(n):
    """(key type, descending, shift, bits, input) of every upsweep call at size n."""
    return [(kt, desc, shift, bits, name) for (kt, desc) in UPSWEEP_TYPES for (shift, bits) in DIGITS for name in UPSWEEP_INPUTS]


SCAN_GRIDS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1, 16384, 16385, 32769)
SCAN_MAX_COUNT = CHUNK                          # a chunk holds 65536 keys
SCAN_ROWS = ("zero", "full", "one_at_0", "one_at_1023", "one_at_1024", "one_at_last")     # rows 0..5; the others are random


def scan_input(grid):
    """A [256][grid] spine as an upsweep could leave it: rows 0 to 5 as SCAN_ROWS names them, the others random <= 65536."""
    rng = np.random.default_rng([5, grid])
    s = rng.integers(0, SCAN_MAX_COUNT + 1, (RADIX, grid), dtype=np.uint32)
    s[:6] = 0
    s[1] = SCAN_MAX_COUNT
    for row, at in ((2, 0), (3, 1023), (4, 1024), (5, grid - 1)):
        if at < grid:
            s[row, at] = 1 + (row * 9973) % SCAN_MAX_COUNT
    return s


# (key_type_in, key_type_out, descending, TW of the full-tile kernel)
DOWNSWEEP_ROWS = ((U32, U32, 0, 0), (U32, U32, 1, 1), (I32, I32, 0, 1), (I32, I32, 1, 1), (I32, U32, 0, 1), (U32, I32, 0, 1),
                  (F32, F32, 0, 2), (F32, F32, 1, 2), (F32, U32, 0, 2), (U32, F32, 0, 2))


def row_name(row):
    kin, kout, desc, tw = row
    return "TW%d-%s-%s-%s" % (tw, KT_NAME[kin], KT_NAME[kout], "desc" if desc else "asc")


DS_TAIL_ONLY = (1, 63, 64, 65, 511, 513, 8191)
DS_FULL_TILES = (1, 8, 15, 16, 17, 24, 31, 32, 33, 40, 48, 63, 64, 65, 96, 1000, 1024, 1025)
DS_BOTH_TILES = (1, 16, 17, 33)
DS_BOTH_EXTRA = (1, 8191)
DS_EVERY_CASE_MAX = 17 * TILE + TILE - 1        # up to here every (row, form, digit, input) runs; above, a rotation
DS_HOST_MAX = 1 << 22                           # above: the expected result is built and compared on the device
DS_LARGE = WIDE_GROUP * TILE + 16 * TILE + 77   # whole groups of 8192 tiles, a group of 16, the tail


def downsweep_sizes():
    """[(id, n)]: tail only, full tiles only, both."""
    out = [("tail-n%d" % n, n) for n in DS_TAIL_ONLY]
    out += [("full-T%d" % t, t * TILE) for t in DS_FULL_TILES]
    out += [("both-T%d+%d" % (t, e), t * TILE + e) for t in DS_BOTH_TILES for e in DS_BOTH_EXTRA]
    return out


def shape_name(full_tiles):
    """The decomposition tile_of_item_wide makes of this many tiles, for the test ids."""
    return "+".join("id%d" % g if k == 0 else "%dx%d" % (k, g) for g, k in wide_groups(full_tiles)) or "none"


def downsweep_calls(n, row=None, pairs=None):
    """(row, pairs, shift, bits, input) of the downsweep calls at size n.  Small sizes: every combination.  Larger ones: every
    row and both forms, with the digit positions and the inputs rotating (three calls per row and form up to 2^22 keys: every
    digit position and input at every size; above, ten calls per size)."""
    rows = DOWNSWEEP_ROWS if row is None else (row,)
    forms = (False, True) if pairs is None else (pairs,)
    if n <= DS_EVERY_CASE_MAX:
        return [(r, p, s, b, name) for r in rows for p in forms for (s, b) in DIGITS for name in DOWNSWEEP_INPUTS]
    out, per = [], (3 if n <= DS_HOST_MAX else 1)
    turn = itertools.count(n // TILE)
    for r in rows:
        for p in forms:
            if n > DS_HOST_MAX and DOWNSWEEP_ROWS.index(r) % 2 != int(p):      # 8 M keys: ten calls, each row in one form
                continue
            for _ in range(per):
                k = next(turn)
                s, b = DIGITS[k % len(DIGITS)]
                out.append((r, p, s, b, DOWNSWEEP_INPUTS[(k // 2) % len(DOWNSWEEP_INPUTS)]))
    return out


ROUTE_SIZES = (("small-scan-256-chunks-ragged", 2040 * TILE + 1), ("small-scan-256-chunks-one-short", 2048 * TILE - 1),
               ("small-scan-256-chunks-full", 2048 * TILE), ("large-kernels-first-size", 2048 * TILE + 1),
               ("large-kernels-2049-tiles", 2049 * TILE))
ROUTE_RANGES = ((0, 16), (8, 32))
ROUTE_TYPES = ((U32, 0), (F32, 1))
COPY_RANGE = (4, 20)                            # two passes


# --------------------------------------------------------------------------------------- plausible wrong kernels --
def model_scan(spine, carry_factor):
    """lsb_scan_kernel with its carry between the segments of 1024 entries dropped (0) or added twice (2); 1 is the kernel."""
    s = np.asarray(spine).astype(np.uint64)
    grid = s.shape[1]
    rows, carry = np.zeros_like(s), np.zeros(s.shape[0], dtype=np.uint64)
    for base in range(0, grid, SCAN_SEG):
        seg = s[:, base:base + SCAN_SEG]
        inc = np.cumsum(seg, axis=1, dtype=np.uint64)
        rows[:, base:base + SCAN_SEG] = np.uint64(carry_factor) * carry[:, None] + inc - seg
        carry = carry + inc[:, -1]
    totals = carry if carry_factor else inc[:, -1]
    return (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32), (totals & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def model_hot_upsweep_counts(dig):
    """(d): a full tile's batch of 4096 keys counts as one digit when the sampled keys at offset 0 or at offset 2048 share one."""
    d = dig.astype(np.int64).copy()
    for lo in range(0, (d.size // TILE) * TILE, BATCH):
        for at in (lo, lo + BATCH // 2):
            s = d[at:at + WAVE]
            if (s == s[0]).all():
                d[lo:lo + BATCH] = s[0]
                break
    return tile_counts(d)
