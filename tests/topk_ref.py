"""numpy reference of gs_topk_u32 (tests/test_topk_cpu.py, tests/test_topk_gpu.py, tests/test_topk_edges_*.py): the image maps
and their inverse, a stable argsort, the first k, the status words, and the workspace formula of the header comment recomputed
from its text."""
import numpy as np

U32, I32, F32 = 0, 1, 2
TILE, CHUNK = 8192, 8
SMALL_CAP = 17408          # elements one workgroup sorts (route 3)


def image(keys, key_type, descending=False):
    """key_type's order-preserving u32 image of u32 bit patterns, complemented when descending."""
    k = np.ascontiguousarray(keys).view(np.uint32)
    if key_type == I32:
        k = k ^ np.uint32(0x80000000)
    elif key_type == F32:
        neg = (k >> np.uint32(31)).astype(bool)
        k = np.where(neg, ~k, k ^ np.uint32(0x80000000)).astype(np.uint32)
    else:
        assert key_type == U32
    return (~k).astype(np.uint32) if descending else k.astype(np.uint32)


def preimage(img, key_type, descending=False):
    """The inverse of image(): the u32 bit patterns of the keys whose image is img."""
    k = np.ascontiguousarray(img).view(np.uint32)
    if descending:
        k = ~k
    if key_type == I32:
        k = k ^ np.uint32(0x80000000)
    elif key_type == F32:
        nonneg = (k >> np.uint32(31)).astype(bool)      # the images of the non-negative floats have the top bit set
        k = np.where(nonneg, k ^ np.uint32(0x80000000), ~k)
    else:
        assert key_type == U32
    return np.ascontiguousarray(k, dtype=np.uint32)


def ranks(keys, key_type, descending=False):
    """ranks[i] = input index of element i of S, the stable sort on the image."""
    return np.argsort(image(keys, key_type, descending), kind="stable").astype(np.uint32)


class Ref:
    """S of one input, computed once: .topk(k) for any k."""

    def __init__(self, keys, key_type, descending=False, values=None):
        self.keys = np.ascontiguousarray(keys).view(np.uint32)
        self.img = image(self.keys, key_type, descending)
        self.order = np.argsort(self.img, kind="stable").astype(np.uint32)
        self.sorted_img = self.img[self.order]
        self.values = None if values is None else np.ascontiguousarray(values).view(np.uint32)
        self.tops = np.bincount(self.img >> np.uint32(24), minlength=256)

    def topk(self, k):
        """(keys_out, values_or_indices_out, status[1..4]) of the first k elements of S."""
        r = self.order[:k]
        kth = int(self.sorted_img[k - 1])
        less = int(np.searchsorted(self.sorted_img, np.uint32(kth), side="left"))
        vals = r if self.values is None else self.values[r]
        return self.keys[r], vals, [kth, less, k - less, int(self.tops[kth >> 24])]

    def route(self, k):
        n = self.keys.size
        if n <= SMALL_CAP:
            return 3
        return 1 if self.topk(k)[2][3] <= max(65536, n // 32) else 2


def topk(keys, k, key_type, descending=False, values=None):
    return Ref(keys, key_type, descending, values).topk(k)


def expected_route(keys, k, key_type, descending=False):
    return Ref(keys, key_type, descending).route(k)


def _a(x):
    return (x + 255) & ~255


def temp_bytes(n, k, has_values, copy_temp_bytes):
    """The formula of the header comment; copy_temp_bytes = gs_lsb_copy_temp_bytes(k, has_values)."""
    tiles = max(1, -(-n // TILE))
    chunks = -(-tiles // CHUNK)
    cand = max(65536, n // 32)
    v = 2 if has_values else 1
    total = 4096 + _a(256 * 4 * chunks) + 1024 + _a(256 * 2 * tiles) + _a(8 * tiles)
    total += v * _a(4 * cand) + v * _a(4 * k) + (_a(4 * k) if has_values else 0)
    return total + _a(copy_temp_bytes) + 256
