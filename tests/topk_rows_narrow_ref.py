"""numpy reference of gs_topk_rows_u16 (tests/test_topk_rows_narrow_cpu.py, tests/test_topk_rows_narrow_gpu.py): the 16-bit
image maps and their inverse on uint16 bit patterns, the per-row stable argsort of the image, the workspace formula
recomputed from the header's text, the widening that the identity of the header speaks of ((uint32_t)key << 16 with the key
type mapped U16 -> U32, I16 -> I32, F16 / BF16 -> F32), and a generator that turns the distributions of topk_cases.gen into
16-bit patterns."""
import numpy as np

import topk_ref as R
import topk_rows_ref as RR
from topk_cases import DISTS, gen

U16, I16, F16, BF16 = 8, 9, 10, 11               # GS_KEY_U16 / I16 / F16 / BF16 of include/gpusort.h
KEY_TYPES = (U16, I16, F16, BF16)
WIDE = {U16: R.U32, I16: R.I32, F16: R.F32, BF16: R.F32}
CH, MAX_K = RR.CH, RR.MAX_K
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)


def _u16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def image16(keys, key_type, descending=False):
    """key_type's order-preserving 16-bit image of uint16 bit patterns (GS_KEY_F32's map at width 16 for the float types),
    complemented when descending."""
    k = _u16(keys)
    if key_type == I16:
        k = k ^ np.uint16(0x8000)
    elif key_type in (F16, BF16):
        neg = (k >> np.uint16(15)).astype(bool)
        k = np.where(neg, ~k, k ^ np.uint16(0x8000))
    else:
        assert key_type == U16
    k = k.astype(np.uint16)
    return (~k).astype(np.uint16) if descending else k


def preimage16(img, key_type, descending=False):
    """The inverse of image16()."""
    k = _u16(np.asarray(img, dtype=np.uint16))
    if descending:
        k = ~k
    if key_type == I16:
        k = k ^ np.uint16(0x8000)
    elif key_type in (F16, BF16):
        nonneg = (k >> np.uint16(15)).astype(bool)      # the images of the non-negative floats have the top bit set
        k = np.where(nonneg, k ^ np.uint16(0x8000), ~k)
    else:
        assert key_type == U16
    return np.ascontiguousarray(k, dtype=np.uint16)


def rows_order(mat, cols, key_type, descending=False):
    """[rows, cols] column indices: row r is the stable argsort of the image of mat[r, :cols]."""
    img = image16(np.ascontiguousarray(_u16(mat)[:, :cols]), key_type, descending)
    return np.argsort(img, axis=1, kind="stable").astype(np.uint32)


def rows_topk16(mat, cols, k, key_type, descending=False, values=None, order=None):
    """mat: [rows, stride] uint16 bit patterns, of which the first `cols` of every row count.  -> (keys [rows, k] uint16,
    values or column indices [rows, k] uint32): the first k of every row's stable sort on the 16-bit image."""
    mat = _u16(mat)
    o = (rows_order(mat, cols, key_type, descending) if order is None else order)[:, :k]
    ko = np.take_along_axis(mat, o.astype(np.int64), axis=1)
    vo = o if values is None else np.take_along_axis(np.ascontiguousarray(values).view(np.uint32), o.astype(np.int64), axis=1)
    return np.ascontiguousarray(ko), np.ascontiguousarray(vo, dtype=np.uint32)


def widen(mat):
    """(uint32_t)key << 16."""
    return (_u16(mat).astype(np.uint32) << np.uint32(16)).astype(np.uint32)


def _a(x):
    return (x + 255) & ~255


def temp_bytes16(rows, cols, k, has_values):
    """The formula of the header comment of gs_topk_rows_u16_temp_bytes."""
    if RR.refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    n1 = RR._next(cols, k) if cols > CH else 0
    n2 = RR._next(n1, k) if n1 > CH else 0
    hv = 1 if has_values else 0
    return _a(2 * rows * n1) + hv * _a(4 * rows * n1) + _a(2 * rows * n2) + hv * _a(4 * rows * n2) + 256


# ------------------------------------------------------------------------------------------------------ inputs --
def specials16(key_type):
    """Patterns every test should meet: the extremes of the type, for the float types +-0, +-inf, NaNs of both signs (quiet,
    with payloads), denormals, and for every type the two patterns whose image is 0xffff (ascending and descending)."""
    if key_type == F16:
        sp = [0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF,
              0x3E00, 0xBE00]
    elif key_type == BF16:
        sp = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x007F, 0x807F,
              0x3FC0, 0xBFC0]
    else:
        sp = [0, 1, 0xFFFF, 0xFFFE, 0x7FFF, 0x8000]     # MIN, MAX, -1, 0 of the signed type
    sp = np.array(sp, np.uint16)
    return np.unique(np.concatenate([sp, preimage16([0xFFFF], key_type, False), preimage16([0xFFFF], key_type, True)]))


def gen16(kind, n, seed=1, kt=U16):
    """n 16-bit key patterns of distribution `kind` of topk_cases.DISTS: the upper half of gen()'s words ("top3": the lower
    half, whose top byte is shared and whose low byte is random), and for "special" the patterns of specials16 mixed into
    random keys.  65536 patterns at most: every distribution is full of ties once n is large."""
    if kind == "special":
        rng = np.random.default_rng(seed * 1000003 + n)
        sp = specials16(kt)
        k = rng.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
        pick = rng.random(n) < 0.6
        k[pick] = sp[rng.integers(0, sp.size, int(pick.sum()))]
        return np.ascontiguousarray(k)
    w = gen(kind, n, seed=seed, kt=WIDE[kt])
    if kind == "top3":
        return np.ascontiguousarray((w & np.uint32(0xFFFF)).astype(np.uint16))
    return np.ascontiguousarray((w >> np.uint32(16)).astype(np.uint16))


def matrix16(rows, cols, kt, seed, stride=None, kinds=DISTS):
    """[rows, stride] uint16: row r has its own data of distribution kinds[(r + seed) % len(kinds)]; the gap is zero."""
    stride = stride or cols
    m = np.zeros((rows, stride), np.uint16)
    for r in range(rows):
        m[r, :cols] = gen16(kinds[(r + seed) % len(kinds)], cols, seed=seed * 1009 + r + 1, kt=kt)
    return m
