"""numpy reference of gs_topk_u64 (tests/test_topk_wide_cpu.py, tests/test_topk_wide_gpu.py): the 64-bit image maps and their
inverse, a stable argsort, the first k, the descent rule of the header comment (route, D, passes, the bucket) and so all eight
status words, the workspace formula recomputed from the header's text, and the builders of the test inputs."""
import numpy as np

U64, I64, F64 = 3, 4, 5
KEY_TYPES = (U64, I64, F64)
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
TILE, CHUNK = 4096, 8
SIGN = np.uint64(1 << 63)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def u64(x):
    return np.ascontiguousarray(x).view(np.uint64)


def image(keys, key_type, descending=False):
    """key_type's order-preserving u64 image of u64 bit patterns, complemented when descending."""
    k = u64(keys)
    if key_type == I64:
        k = k ^ SIGN
    elif key_type == F64:
        neg = (k >> np.uint64(63)).astype(bool)
        k = np.where(neg, ~k, k ^ SIGN)
    else:
        assert key_type == U64
    return np.ascontiguousarray(~k if descending else k, dtype=np.uint64)


def preimage(img, key_type, descending=False):
    """The inverse of image()."""
    k = u64(img)
    if descending:
        k = ~k
    if key_type == I64:
        k = k ^ SIGN
    elif key_type == F64:
        nonneg = (k >> np.uint64(63)).astype(bool)
        k = np.where(nonneg, k ^ SIGN, ~k)
    else:
        assert key_type == U64
    return np.ascontiguousarray(k, dtype=np.uint64)


def cap(n):
    return max(65536, n // 32)


def byte_of(img, j):
    return ((img >> np.uint64(8 * j)) & np.uint64(255)).astype(np.int64)


def descent(img, k):
    """The way down of the header comment on the images of one input: (route, D, passes, c), c the bucket moved to the list
    (route 1) or the tie run (route 2)."""
    n, cur, krem, j, D = img.size, img, k, 7, 0
    while True:
        D += 1
        b = byte_of(cur, j)
        cum = np.cumsum(np.bincount(b, minlength=256))
        d = int(np.searchsorted(cum, krem, side="left"))
        c = int(cum[d] - (cum[d - 1] if d else 0))
        krem -= int(cum[d]) - c
        if c <= cap(n):
            route = 1
            break
        diff = int(np.bitwise_and.reduce(cur) ^ np.bitwise_or.reduce(cur)) & ((1 << (8 * j)) - 1)
        if diff == 0:
            route = 2
            break
        cur = cur[b == d]
        j = (diff.bit_length() - 1) // 8
    return route, D, 2 if D == 1 else D + 2, c


class Ref64:
    """S of one input, computed once: .topk(k) and .status(k) for any k."""

    def __init__(self, keys, key_type, descending=False, values=None):
        self.keys = u64(keys)
        self.img = image(self.keys, key_type, descending)
        self.order = np.argsort(self.img, kind="stable").astype(np.uint32)
        self.sorted_img = self.img[self.order]
        self.values = None if values is None else np.ascontiguousarray(values).view(np.uint32)

    def topk(self, k):
        """(keys_out, values_or_indices_out) of the first k elements of S."""
        r = self.order[:k]
        return self.keys[r], (r if self.values is None else self.values[r])

    def status(self, k):
        """The eight words of gs_topk_u64_status."""
        kth = int(self.sorted_img[k - 1])
        less = int(np.searchsorted(self.sorted_img, np.uint64(kth), side="left"))
        route, D, passes, c = descent(self.img, k)
        return [route, kth & 0xFFFFFFFF, kth >> 32, less, k - less, D, passes, c]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(n, k, has_values, wide_temp_bytes):
    """The formula of the header comment; wide_temp_bytes = gs_lsb_wide_temp_bytes(k, 8, has_values ? 4 : 0)."""
    if n == 0 or k == 0:
        return 0
    tiles = max(1, -(-n // TILE))
    chunks = -(-tiles // CHUNK)
    hv = 1 if has_values else 0
    total = 221184 + _a(256 * 4 * chunks) + 1024 + _a(256 * 2 * tiles) + _a(8 * tiles)
    total += _a(8 * cap(n)) + hv * _a(4 * cap(n))
    total += 2 * _a(8 * k) + hv * 2 * _a(4 * k)
    return total + _a(wide_temp_bytes) + 256


# ------------------------------------------------------------------------------------------------------ builders --
def specials64(kt):
    """F64: NaNs of both signs with payloads, +-0, +-inf, denormals, +-1; I64 / U64: the extremes and their neighbours."""
    if kt == F64:
        return np.array([0x7FF8000000000001, 0xFFF8000000000001, 0x7FF00000DEADBEEF, 0xFFFFFFFFFFFFFFFF, 0x7FF0000000000000,
                         0xFFF0000000000000, 0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001,
                         0x000FFFFFFFFFFFFF, 0x3FF0000000000000, 0xBFF0000000000000], dtype=np.uint64)
    return np.array([0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 0, 1, 0xFFFFFFFFFFFFFFFF, 0x8000000000000001, 0x7FFFFFFFFFFFFFFE],
                    dtype=np.uint64)


DISTS = ("uniform", "normal", "small", "five", "special")


def gen64(kind, n, seed, kt=U64):
    """u64 bit patterns: uniform words; N(0, 1) doubles; integers below 2^24; five distinct values; the specials among
    uniform words, six elements in ten."""
    rng = np.random.default_rng(seed)
    uni = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    if kind == "uniform":
        return uni
    if kind == "normal":
        return rng.standard_normal(n).view(np.uint64).copy()
    if kind == "small":
        return rng.integers(0, 1 << 24, n, dtype=np.uint64)
    if kind == "five":
        return uni[:5][rng.integers(0, min(5, n), n)] if n else uni
    assert kind == "special"
    sp = specials64(kt)
    return np.where(rng.random(n) < 0.6, sp[rng.integers(0, sp.size, n)], uni)


def shuffle(img, seed):
    return img[np.random.default_rng(seed).permutation(img.size)]


def bucket_case64(n, c, below, top, seed, kt, desc):
    """Images: `below` elements with a top byte under `top`, c with top byte `top` and random lower bytes, the rest above."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 1 << 56, n, dtype=np.uint64)
    tb = np.concatenate([rng.integers(0, top, below), np.full(c, top), rng.integers(top + 1, 256, n - c - below)]).astype(np.uint64)
    return preimage(shuffle((tb << np.uint64(56)) | low, seed + 1), kt, desc)


def bucket_ks(below, c):
    """(k, inside the bucket): the edges of the bucket and its middle."""
    return [(below, False), (below + 1, True), (below + c // 2, True), (below + c, True), (below + c + 1, False)]


def small_ints(n, seed, outlier=False):
    """int64 below 2^24; outlier: one -1 among them (it defeats the skip of round one, not that of round two)."""
    keys = np.random.default_rng(seed).integers(0, 1 << 24, n, dtype=np.uint64)
    if outlier:
        keys[n // 2] = ONES
    return keys


def timestamps(n, seed):
    """int64 nanoseconds of one day of 2024."""
    day0 = 1_718_000_000 * 10 ** 9
    return (np.random.default_rng(seed).integers(0, 86_400 * 10 ** 9, n, dtype=np.int64) + day0).view(np.uint64)


DEEP_BASE = 0x4142434445464700


def deep_case64(kt, desc, seed=0):
    """D = 8: cap + 1 elements that share bytes 7..1 and split on byte 0 in two halves, and seven outliers, the one of level
    b = 6..0 sharing the bytes above b and differing at b, so that every round finds the next byte alive."""
    c = 65536 + 1
    main = np.full(c, DEEP_BASE, dtype=np.uint64) | np.where(np.arange(c) % 2 == 0, np.uint64(0x10), np.uint64(0x20))
    out = [DEEP_BASE ^ ((0x03 if b % 2 else 0xC0) << (8 * b)) for b in range(7)]
    out[0] = DEEP_BASE | 0x18
    return preimage(shuffle(np.concatenate([main, np.array(out, dtype=np.uint64)]), seed), kt, desc)


def tie_case64(n, run, seed, kt, desc):
    """`run` equal keys among uniform ones, in the middle of the order."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2)
    img[:run] = np.uint64(0x8000000000000001)
    return preimage(shuffle(img, seed + 1), kt, desc)


def byte_edge_case64(p, v, deep, kt, desc, seed=0):
    """The k-th image has byte p equal to v (0x00 or 0xff).  deep False: 20000 uniform images with byte p forced to v (the pick
    of the list round at p, or of round one for p = 7, meets digit v).  deep True: 70001 images that share the bytes above p, 66000
    of them with byte p = v and the rest with byte p = 0x55, random below: a round over the input picks digit v at byte p."""
    rng = np.random.default_rng(seed + 8 * p + v)
    n = 70001 if deep else 20000
    img = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    m = np.uint64(0xFF) << np.uint64(8 * p)
    if deep:
        above = ~((np.uint64(1) << np.uint64(8 * p)) - np.uint64(1)) & ~m if p < 7 else np.uint64(0)
        img = (img & ~above & ~m) | (np.uint64(0x6A6B6C6D6E6F7071) & above)
        bp = np.where(np.arange(n) < 66000, np.uint64(v), np.uint64(0x55))
        img = shuffle(img | (bp << np.uint64(8 * p)), seed)
    else:
        img = (img & ~m) | (np.uint64(v) << np.uint64(8 * p))
    return preimage(img, kt, desc)


def run_cuts(ref):
    """k at the last element of every run of equal keys, at the first of the next and one before (all within 1..n)."""
    s, n = ref.sorted_img, ref.sorted_img.size
    ends = np.flatnonzero(s[1:] != s[:-1]) + 1
    ks = set()
    for e in ends.tolist() + [n]:
        ks.update(k for k in (e - 1, e, e + 1) if 1 <= k <= n)
    return sorted(ks)
