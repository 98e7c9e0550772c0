"""numpy reference of gs_topk_u16 (tests/test_topk_narrow_cpu.py, tests/test_topk_narrow_gpu.py): one stable argsort of the
16-bit image per input, the first k, the status words and the route, the workspace formula recomputed from the header's text,
and builders that lay out 16-bit IMAGES (top-byte buckets, tie runs) and return the keys that have them.  The image maps and
the special patterns are those of tests/topk_rows_narrow_ref.py, the distributions those of tests/topk_cases.py."""
import numpy as np

from topk_cases import DISTS, gen                                     # noqa: F401  (re-exported for the tests)
from topk_rows_narrow_ref import (U16, I16, F16, BF16, KEY_TYPES, WIDE, KEYS, PAIRS, ARGS, MODES,      # noqa: F401
                                  image16, preimage16, specials16, gen16, widen)

TILE = 8192                # gs_lsb_narrow_tile(key_type, 4): one workgroup of the narrow upsweep, the filter and the select
MIN_CAND = 65536


def cap(n):
    """Capacity of the candidate list."""
    return max(MIN_CAND, n // 32)


class Ref16:
    """S of one input of uint16 bit patterns, computed once: .topk(k) for any k."""

    def __init__(self, keys, key_type, descending=False, values=None):
        self.keys = np.ascontiguousarray(keys).view(np.uint16)
        self.img = image16(self.keys, key_type, descending)
        self.order = np.argsort(self.img, kind="stable").astype(np.uint32)
        self.sorted_img = self.img[self.order]
        self.values = None if values is None else np.ascontiguousarray(values).view(np.uint32)
        self.tops = np.bincount(self.img >> np.uint16(8), minlength=256)

    def topk(self, k):
        """(keys_out, values_or_indices_out, status[1..4]) of the first k elements of S."""
        r = self.order[:k]
        kth = int(self.sorted_img[k - 1])
        less = int(np.searchsorted(self.sorted_img, np.uint16(kth), side="left"))
        vals = r if self.values is None else self.values[r]
        return self.keys[r], vals, [kth, less, k - less, int(self.tops[kth >> 8])]

    def route(self, k):
        n = self.keys.size
        if n <= TILE:
            return 3
        return 1 if self.topk(k)[2][3] <= cap(n) else 2


def _a(x):
    return (x + 255) & ~255


def temp_bytes16(n, k, has_values, narrow_temp_bytes):
    """The formula of the header comment; narrow_temp_bytes = gs_lsb_narrow_temp_bytes(k, GS_KEY_U16, 4 with values else 0)."""
    if n == 0 or k == 0:
        return 0
    tiles = max(1, -(-n // TILE))
    c = cap(n)
    hv = 1 if has_values else 0
    total = 4096 + _a(256 * 4 * tiles) + 1024 + _a(8 * tiles)
    total += _a(2 * c) + hv * _a(4 * c) + _a(2 * k) + hv * _a(4 * k) + hv * _a(4 * k)
    return total + _a(narrow_temp_bytes) + 256


def narrow_temp_bytes(k, has_values):
    """gs_lsb_narrow_temp_bytes(k, GS_KEY_U16, 4 or 0) from ITS header text: spine (1 KiB per tile of 8192), digit totals,
    slack, and for 16-bit keys the intermediate keys and values."""
    tiles = max(1, -(-k // TILE))
    return _a(256 * 4 * tiles) + 1024 + 256 + _a(2 * k) + _a(4 * k if has_values else 0)


# ------------------------------------------------------------------------------------------------------ inputs --
def keys_of(img, key_type, descending=False):
    return preimage16(np.asarray(img, dtype=np.uint64).astype(np.uint16), key_type, descending)


def bucket_case16(n, c, below, d0, seed, key_type=U16, descending=False):
    """`below` images under d0 << 8, exactly c with top byte d0, the rest above; shuffled."""
    assert 0 < d0 < 255 and below + c <= n
    rng = np.random.default_rng(seed)
    img = np.concatenate([rng.integers(0, d0 << 8, below, dtype=np.uint64),
                          rng.integers(0, 256, c, dtype=np.uint64) | np.uint64(d0 << 8),
                          rng.integers((d0 + 1) << 8, 1 << 16, n - below - c, dtype=np.uint64)])
    return keys_of(img[rng.permutation(n)], key_type, descending)


def bucket_ks(below, c):
    """(k, inside the bucket): the last before the bucket, its first, middle and last, the first after it."""
    return [(below, False), (below + 1, True), (below + c // 2, True), (below + c, True), (below + c + 1, False)]


# images whose bytes are 0x00 and 0xff, and their neighbours: every pick meets digit 0 and digit 255
IMAGES12 = [0x0000, 0x0001, 0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFE00, 0xFEFF, 0xFF00, 0xFF01, 0xFFFE, 0xFFFF]
RUNS12 = [8193, 1, 8191, 64, 8192, 63, 2, 8193, 8192, 65, 1, 8191]


def digit_edge_case16(route, top=0x00, key_type=U16, descending=False, seed=5):
    """One tie run per image of IMAGES12, shuffled.  route 2: the long runs under the top byte `top` are four tiles longer, which
    takes that byte's bucket past 65536."""
    assert route in (1, 2) and top in (0x00, 0xFF)
    runs = [ln + 4 * TILE if route == 2 and img >> 8 == top and ln >= TILE - 1 else ln for img, ln in zip(IMAGES12, RUNS12)]
    img = np.repeat(np.array(IMAGES12, np.uint64), runs)
    return keys_of(img[np.random.default_rng(seed).permutation(img.size)], key_type, descending)


def run_cuts(ref):
    """For every tie run of ref's sorted images, with cumulative end C: the k values C - 1, C and C + 1, clipped to [1, n]."""
    s = ref.sorted_img
    ends = np.append(np.flatnonzero(s[1:] != s[:-1]) + 1, s.size).astype(np.int64)
    ks = np.unique(np.clip(np.concatenate([ends - 1, ends, ends + 1]), 1, s.size))
    return [int(k) for k in ks]


def bucket_cuts(ref):
    """k on the first and the last element of every top-byte bucket of ref's sorted images."""
    ends = np.cumsum(ref.tops)
    ends = ends[ref.tops > 0]
    starts = np.concatenate([[0], ends[:-1]])
    return sorted({int(k) for k in np.concatenate([starts + 1, ends])})
