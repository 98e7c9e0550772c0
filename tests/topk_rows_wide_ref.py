"""numpy reference of gs_topk_rows_u64 (tests/test_topk_rows_wide_cpu.py, tests/test_topk_rows_wide_gpu.py): built on the
64-bit image maps of topk_wide_ref, the per-row stable argsort of the image, the first k of every row, the workspace formula
recomputed from the header's text, the widening that the identity of the header speaks of ((uint64_t)key << 32 with the key
type mapped U32 -> U64, I32 -> I64, F32 -> F64), a numpy model of the chunked scheme at 64 bits, matrices whose rows take
the distributions of topk_wide_ref.gen64, and the builders of the inputs that the byte skip and the pad image must survive."""
import numpy as np

import topk_ref as R
import topk_rows_ref as RR
import topk_wide_ref as W

U64, I64, F64 = W.U64, W.I64, W.F64
KEY_TYPES = W.KEY_TYPES
WIDE = {R.U32: U64, R.I32: I64, R.F32: F64}
CH, MAX_K = RR.CH, RR.MAX_K
KEYS, PAIRS, ARGS = W.KEYS, W.PAIRS, W.ARGS
MODES = W.MODES
ONES = W.ONES
image, preimage, u64 = W.image, W.preimage, W.u64


def rows_order(mat, cols, key_type, descending=False):
    """[rows, cols] column indices: row r is the stable argsort of the 64-bit image of mat[r, :cols]."""
    img = image(np.ascontiguousarray(u64(mat)[:, :cols]), key_type, descending)
    return np.argsort(img, axis=1, kind="stable").astype(np.uint32)


def rows_topk64(mat, cols, k, key_type, descending=False, values=None, order=None):
    """mat: [rows, stride] uint64 bit patterns, of which the first `cols` of every row count.  -> (keys [rows, k] uint64,
    values or column indices [rows, k] uint32): the first k of every row's stable sort on the 64-bit image."""
    mat = u64(mat)
    o = (rows_order(mat, cols, key_type, descending) if order is None else order)[:, :k]
    ko = np.take_along_axis(mat, o.astype(np.int64), axis=1)
    vo = o if values is None else np.take_along_axis(np.ascontiguousarray(values).view(np.uint32), o.astype(np.int64), axis=1)
    return np.ascontiguousarray(ko), np.ascontiguousarray(vo, dtype=np.uint32)


def widen32(mat):
    """(uint64_t)key << 32 of u32 bit patterns."""
    return (np.ascontiguousarray(mat).view(np.uint32).astype(np.uint64) << np.uint64(32)).astype(np.uint64)


def _a(x):
    return (x + 255) & ~255


def temp_bytes64(rows, cols, k, has_values):
    """The formula of the header comment of gs_topk_rows_u64_temp_bytes."""
    if RR.refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    n1 = RR._next(cols, k) if cols > CH else 0
    n2 = RR._next(n1, k) if n1 > CH else 0
    hv = 1 if has_values else 0
    return _a(8 * rows * n1) + hv * _a(4 * rows * n1) + _a(8 * rows * n2) + hv * _a(4 * rows * n2) + 256


def chunk_model64(keys, k, key_type, descending=False, ch=CH):
    """topk_rows_ref.chunk_model at 64 bits: every level cuts its source into chunks of `ch`, takes each chunk's first
    min(k, length) by (image, position) and concatenates them.  -> (keys_out, columns, levels)."""
    img = image(u64(keys), key_type, descending)
    col = np.arange(img.size, dtype=np.uint32)
    levels = 0
    while True:
        levels += 1
        out_i, out_c = [], []
        for lo in range(0, img.size, ch):
            seg = img[lo:lo + ch]
            order = np.argsort(seg, kind="stable")[:min(k, seg.size)]
            out_i.append(seg[order])
            out_c.append(col[lo:lo + ch][order])
        single = img.size <= ch
        img, col = np.concatenate(out_i), np.concatenate(out_c)
        if single:
            break
    return preimage(img, key_type, descending), col, levels


# ------------------------------------------------------------------------------------------------------ inputs --
def matrix64(rows, cols, kt, seed, stride=None, kinds=W.DISTS):
    """[rows, stride] uint64: row r has its own data of distribution kinds[(r + seed) % len(kinds)]; the gap is zero."""
    stride = stride or cols
    m = np.zeros((rows, stride), np.uint64)
    for r in range(rows):
        m[r, :cols] = W.gen64(kinds[(r + seed) % len(kinds)], cols, seed=seed * 1009 + r + 1, kt=kt)
    return m


def differ(img):
    """AND ^ OR of every row of images: the bits in which two elements of the row differ."""
    img = u64(img)
    return np.bitwise_and.reduce(img, axis=1) ^ np.bitwise_or.reduce(img, axis=1)


def differing_bytes(img):
    """Per row, the set of byte positions 0..7 in which two images of the row differ."""
    d = differ(img)
    return [frozenset(b for b in range(8) if (int(x) >> (8 * b)) & 255) for x in d]


BASE = np.uint64(0x6A4B3C2D1E0F7183)


def one_byte_rows(rows, cols, b, seed, base=BASE):
    """Images: every row shares `base` but for byte b, which takes every value it can (256 if the row is long enough)."""
    rng = np.random.default_rng(seed)
    m = np.uint64(255) << np.uint64(8 * b)
    v = rng.integers(0, 256, (rows, cols), dtype=np.uint64)
    if cols >= 2:
        v[:, 0], v[:, 1] = 0, 255
    return (base & ~m) | (v << np.uint64(8 * b))


def one_key_rows(rows, cols, image_value=BASE):
    return np.full((rows, cols), image_value, np.uint64)


def outlier_rows(rows, cols, b, at, seed, base=BASE):
    """Images that vary in byte 0 alone, but for ONE element per row, at column `at`, whose byte b differs too: it alone
    makes byte b vary."""
    img = one_byte_rows(rows, cols, 0, seed, base)
    img[:, at] ^= np.uint64(0x40) << np.uint64(8 * b)
    return img


def mixed_constant_rows(rows, cols, seed):
    """Row r varies exactly in the bytes of the set r picks (cycling through subsets of different sizes), so that neighbouring
    rows -- the waves of one path-1 workgroup -- take different pass sets."""
    sets = [(0,), (7,), (0, 7), (3,), (1, 2, 5), (), (0, 1, 2, 3, 4, 5, 6, 7), (4, 6)]
    rng = np.random.default_rng(seed)
    img = np.empty((rows, cols), np.uint64)
    for r in range(rows):
        row = np.full(cols, BASE + np.uint64(r), np.uint64)
        for b in sets[r % len(sets)]:
            m = np.uint64(255) << np.uint64(8 * b)
            v = rng.integers(0, 256, cols, dtype=np.uint64)
            if cols >= 2:
                v[0], v[cols - 1] = 0, 255
            row = (row & ~m) | (v << np.uint64(8 * b))
        img[r] = row
    return img, [frozenset(s if cols >= 2 else ()) for s in (sets[r % len(sets)] for r in range(rows))]


def chunked_constant_row(cols, seed):
    """One row of images whose chunk c (CH columns) varies in byte (c % 8) alone and shares the others inside the chunk; the
    chunks differ from each other in byte 7 or 6, so a path-3 row's workgroups run different rounds."""
    rng = np.random.default_rng(seed)
    img = np.empty(cols, np.uint64)
    for c, lo in enumerate(range(0, cols, CH)):
        n = min(CH, cols - lo)
        b = c % 8
        base = BASE ^ (np.uint64(c % 3) << np.uint64(56 if b != 7 else 48))
        m = np.uint64(255) << np.uint64(8 * b)
        img[lo:lo + n] = (base & ~m) | (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(8 * b))
    return img


def small_int_rows(rows, cols, seed):
    """int64 below 2^24 (key patterns)."""
    return np.random.default_rng(seed).integers(0, 1 << 24, (rows, cols), dtype=np.uint64)


def timestamp_rows(rows, cols, seed):
    """int64 nanoseconds of one day (key patterns)."""
    return W.timestamps(rows * cols, seed).reshape(rows, cols)


def pad_image_rows(rows, cols, few, seed):
    """Images: all ones -- the pad's -- but for `few` smaller ones per row; the last row is nothing else."""
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), ONES, np.uint64)
    for r in range(rows - 1):
        img[r, rng.choice(cols, few, replace=False)] = rng.integers(0, 1 << 63, few, dtype=np.uint64)
    return img
