"""Reference of gs_topk_rows_anyk_u64 (tests/test_topk_rows_anyk_wide_cpu.py, tests/test_topk_rows_anyk_wide_gpu.py): the per-row
stable argsort of the 64-bit image of topk_rows_wide_ref, the plan, the workspace formula and the status of a row recomputed
from the header's text -- the status through a host model of the descent (shift sequence, D, mode, list count) --, the shape
tables the two files share, and the builders of the inputs that the descent must survive."""
import numpy as np

import topk_rows_wide_ref as RW

U64, I64, F64, KEY_TYPES = RW.U64, RW.I64, RW.F64, RW.KEY_TYPES
KEYS, PAIRS, ARGS, MODES = RW.KEYS, RW.PAIRS, RW.ARGS, RW.MODES
image, preimage, u64, ONES = RW.image, RW.preimage, RW.u64, RW.ONES
rows_order, rows_topk64, matrix64, widen32 = RW.rows_order, RW.rows_topk64, RW.matrix64, RW.widen32
CH = 8192             # longest row of path 1
TILE = 8192
BINS = 2048
DIGIT = 11
SHIFTS = [53, 42, 31, 20, 9, 0]     # the worst case: six rounds
LAUNCHES = {1: 2, 2: 19}            # before the finish (the header's text at gs_topk_rows_anyk_u64_plan)
REC_WORDS = 16


def keys_of(img, key_type, descending=False):
    """Key bit patterns whose images are `img`."""
    return preimage(np.ascontiguousarray(img, dtype=np.uint64), key_type, descending)


def refused(rows, cols, k):
    return k > cols or rows * cols >= 1 << 32 or rows * k >= 1 << 31


def list_cap(cols):
    """L, the capacity of a row's list."""
    return min(8192, max(1024, cols // 8))


def plan(rows, cols, k, slab_tiles=4):
    """gs_topk_rows_anyk_u64_plan's eight words (None for a refused shape)."""
    if refused(rows, cols, k):
        return None
    if rows == 0 or cols == 0 or k == 0:
        return [0] * 8
    if cols <= CH:
        return [1, LAUNCHES[1], CH, TILE, 1, 1, 1, 0]
    tiles = -(-cols // TILE)
    return [2, LAUNCHES[2], CH, TILE, slab_tiles, -(-tiles // slab_tiles), tiles, list_cap(cols)]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(rows, cols, k, has_values, wide_temp_bytes):
    """The formula of the header comment; wide_temp_bytes = gs_segmented_wide_temp_bytes(rows * k, 8, 4 with values else 0, rows)."""
    if refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    hv = 1 if has_values else 0
    total = _a(4 * REC_WORDS * rows) + _a(4 * (rows + 1))
    if cols > CH:
        total += _a(4 * BINS * rows) + _a(8 * rows * -(-cols // TILE)) + _a(8 * list_cap(cols) * rows)
    total += _a(8 * rows * k) + 2 * hv * _a(4 * rows * k)
    return total + _a(wide_temp_bytes) + 256


def descent(img, k):
    """The descent of the header comment on the images of one row: a dict of kth, less, take, D, mode (0 path 1, 1 list, 2 tie
    run), list (elements put on the list), shifts (the shift of every round taken) and c (the count of every picked bin)."""
    img = u64(img)
    if img.size <= CH:
        s = np.sort(img)
        kth = int(s[k - 1])
        less = int(np.searchsorted(s, np.uint64(kth), side="left"))
        return dict(kth=kth, less=less, take=k - less, D=0, mode=0, list=0, shifts=[], c=[])
    L = list_cap(img.size)
    shift, prefix, less, krem, shifts, cs = 53, 0, 0, k, [], []
    while True:
        shifts.append(shift)
        hi = shift + DIGIT
        matched = img if hi >= 64 else img[(img >> np.uint64(hi)) == np.uint64(prefix >> hi)]
        cnt = np.bincount(((matched >> np.uint64(shift)) & np.uint64(BINS - 1)).astype(np.int64), minlength=BINS)
        cum = np.cumsum(cnt)
        d = int(np.searchsorted(cum, krem, side="left"))
        ex = int(cum[d] - cnt[d])
        prefix |= d << shift
        less, krem, c = less + ex, krem - ex, int(cnt[d])
        cs.append(c)
        all_and, all_or = int(np.bitwise_and.reduce(matched)), int(np.bitwise_or.reduce(matched))
        low = (1 << shift) - 1
        v = (all_and ^ all_or) & low
        if shift == 0 or v == 0:
            prefix |= all_and & low
            return dict(kth=prefix, less=less, take=krem, D=len(shifts), mode=2, list=0, shifts=shifts, c=cs)
        if c <= L:
            bucket = np.sort(img[(img >> np.uint64(shift)) == np.uint64(prefix >> shift)])
            assert bucket.size == c
            kth = int(bucket[krem - 1])
            below = int(np.searchsorted(bucket, np.uint64(kth), side="left"))
            return dict(kth=kth, less=less + below, take=krem - below, D=len(shifts), mode=1, list=c, shifts=shifts, c=cs)
        hb = v.bit_length() - 1
        prefix |= all_and & low & ~((2 << hb) - 1)
        shift = max(hb - (DIGIT - 1), 0)


def status(row_keys, k, key_type, descending=False):
    """gs_topk_rows_anyk_u64_status's eight words for one row (uint64 bit patterns)."""
    d = descent(image(row_keys, key_type, descending), k)
    path = 1 if np.asarray(row_keys).size <= CH else 2
    return [path, d["kth"] & 0xFFFFFFFF, d["kth"] >> 32, d["less"], d["take"], d["D"], d["mode"], d["list"]]


# ------------------------------------------------------------------------------------------ the shared shape tables --
SLAB = 4 * TILE       # asserted against the plan by both files before it is used
PATH1_COLS = [1025, CH - 1, CH]
PATH1_ROWS = [1, 7]


def path1_ks(cols):
    return sorted({1, 1024, 1025, cols - 1, cols})


PATH2_COLS = [CH + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 5, 3 * SLAB + TILE + 1]
PATH2_ROWS = [1, 3]


def path2_ks(cols):
    return sorted({1, 1025, 8192, 8193, cols - 1, cols})     # 8192 / 8193: the finish leaves its one-workgroup class


SIZE_COLS = [1, 1024, 1025, 8191, 8192, 8193, SLAB - 1, SLAB, SLAB + 1, 65536, 151936]


def size_ks(cols):
    return sorted({k for k in (1, 1024, 1025, 8192, 8193, cols) if k <= cols})


MANY_ROWS = (300, 9000, 1100)
DEEP_COLS = 3 * TILE              # L = 3072: the six-round row
GUARDED_SHAPES = [(3, 5000, 1500, 1), (2, SLAB + TILE + 7, 3000, 2)]     # (rows, cols, k, path)
GRAPH_SHAPES = [(5, 6000, 2000, 1), (2, SLAB + 9, 1500, 2)]
STRIDE_SHAPES = [(4000, 1200, 1), (CH, 1025, 1), (CH + 5, 2000, 2), (SLAB + 1, 9000, 2)]      # (cols, k, path) at row_stride = cols + 3
REUSE_SHAPES = [(3, SLAB + 9, 1300, 2), (6, 5000, 1100, 1)]
AGREE_SHAPES = [(4, 6000, 1), (3, SLAB + 77, 2)]                         # (rows, cols, path)


# ------------------------------------------------------------------------------------------------------ builders --
def uniform_images(rng, n):
    return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)


def shared_top_row(cols, b, seed):
    """Images of one row that share their top b bits (0 <= b <= 64) and are uniform below them."""
    rng = np.random.default_rng(seed)
    base = np.uint64(0xA5C3960F1E2D4B78)
    if b == 0:
        return uniform_images(rng, cols)
    if b == 64:
        return np.full(cols, base, np.uint64)
    low = np.uint64((1 << (64 - b)) - 1)
    return (base & ~low) | (uniform_images(rng, cols) & low)


TOP = 0x2A5           # the top digit of the buckets that the builders below make; fillers lie above it


def _fillers(rng, n):
    """Uniform images whose top digit is above TOP."""
    top = rng.integers(TOP + 1, BINS, n, dtype=np.uint64)
    return (top << np.uint64(53)) | (uniform_images(rng, n) >> np.uint64(DIGIT))


def bucket_row(cols, c, seed):
    """(images, k): c images with top digit TOP and uniform lower bits among fillers above them; k is in the middle of the
    bucket, which holds exactly c elements after round one."""
    rng = np.random.default_rng(seed)
    img = _fillers(rng, cols)
    at = rng.choice(cols, c, replace=False)
    img[at] = (np.uint64(TOP) << np.uint64(53)) | (uniform_images(rng, c) >> np.uint64(DIGIT))
    return img, (c + 1) // 2


def depth_row(cols, depth, seed, core=None):
    """(images, k) of a row that takes `depth` rounds (1 .. 6).  A core of L + 1 + 200 images shares every bit at and above
    SHIFTS[depth - 2] and is uniform below: it sits in one bin, above L, in every round before the last one.  In round j
    of the first depth - 2, one spoiler that matches the core at and above SHIFTS[j] but differs at bit SHIFTS[j] - 1 keeps
    the next shift at SHIFTS[j] - 11; the round before the last finds that bit varying in the core itself.  Fillers lie above.
    depth 6 ends at shift 0 (a tie run), the others in the list."""
    rng = np.random.default_rng(seed)
    L = list_cap(cols)
    if depth == 1:
        return uniform_images(rng, cols), cols // 3
    n = core or L + 201
    t = SHIFTS[depth - 2]                             # the core varies below bit t: one bin in the round before the last
    p = (TOP << 53) | (0x0F0F0F0F0F0F0 & ((1 << 53) - 1))
    for s in SHIFTS[:depth - 2]:
        p &= ~(1 << (s - 1))                          # (the spoilers flip these bits to one: they lie above the core)
    p &= ~((1 << t) - 1)
    img = _fillers(rng, cols)
    at = rng.choice(cols, n + depth, replace=False)
    img[at[:n]] = np.uint64(p) | (uniform_images(rng, n) & np.uint64((1 << t) - 1))
    for j, s in enumerate(SHIFTS[:depth - 2]):
        img[at[n + j]] = np.uint64(p | (1 << (s - 1)))
    return img, n // 2


def single_row(cols, seed):
    """(images, k): one image alone in top digit TOP, `below` images under it, fillers above: a list of exactly one."""
    rng = np.random.default_rng(seed)
    below = 1500
    img = _fillers(rng, cols)
    at = rng.choice(cols, below + 1, replace=False)
    img[at[:below]] = uniform_images(rng, below) >> np.uint64(DIGIT + 2)          # top digits under 512 <= TOP
    img[at[below]] = (np.uint64(TOP) << np.uint64(53)) | np.uint64(12345)
    return img, below + 1


def outlier_positions(cols):
    """The first column, the last, and the first element of the last, partly filled register of the last tile."""
    last_tile = (cols - 1) // TILE * TILE
    part = last_tile + (cols - last_tile) // 64 * 64
    assert part < cols - 1 and (cols - last_tile) % 64 > 1
    return [0, cols - 1, part]


def outlier_row(cols, at, seed, bit=40):
    """Key patterns: int64 below 2^24 but for ONE element, at column `at`, that has `bit` set too: it alone makes the bits
    between 24 and `bit` vary."""
    keys = np.random.default_rng(seed).integers(0, 1 << 24, cols, dtype=np.uint64)
    keys[at] |= np.uint64(1 << bit)
    return keys


def tie_run_row(cols, start, length, seed):
    """(images, k, below): one image `length` times at columns [start, start + length), `below` smaller images and the rest
    above; k cuts the run inside."""
    rng = np.random.default_rng(seed)
    below = 700
    run = np.uint64((TOP << 53) | 0x1234567)
    img = _fillers(rng, cols)
    img[start:start + length] = run
    free = np.concatenate([np.arange(0, start), np.arange(start + length, cols)])
    img[rng.choice(free, below, replace=False)] = uniform_images(rng, below) >> np.uint64(DIGIT + 2)
    return img, below + length // 2, below


def specials_matrix(rows, cols, kt, seed):
    """NaNs of both signs and +-0 and their like (F64), the extremes (I64 / U64), drawn uniformly."""
    sp = RW.W.specials64(kt)
    return sp[np.random.default_rng(seed).integers(0, sp.size, (rows, cols))]


def around_zero(rows, cols, seed):
    """I64 patterns in [-40, 40]."""
    return np.random.default_rng(seed).integers(-40, 41, (rows, cols)).astype(np.int64).view(np.uint64)
