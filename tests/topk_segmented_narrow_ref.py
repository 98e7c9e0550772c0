"""numpy reference of gs_topk_segmented_u16 (tests/test_topk_segmented_narrow_cpu.py, tests/test_topk_segmented_narrow_gpu.py),
built on topk_segmented_ref (clamping, geometry, status, shapes) and topk_rows_narrow_ref (the 16-bit image maps): the
per-segment reference on the 16-bit image, the workspace formula recomputed from the header's text, and the widening identity
of the header ((uint32_t)key << 16 through the 32-bit reference, the returned keys shifted right by 16)."""
import numpy as np

import topk_rows_narrow_ref as NR
import topk_segmented_ref as SR

U16, I16, F16, BF16 = NR.U16, NR.I16, NR.F16, NR.BF16
KEY_TYPES = NR.KEY_TYPES
WIDE = NR.WIDE
CH, MAX_K = SR.CH, SR.MAX_K
FILL = SR.FILL           # unwritten u32 slots (values, positions, counts)
FILL16 = 0xFFFF          # unwritten key slots


def seg_topk16(keys, begin, end, k, key_type, descending=False, values=None, cache=None):
    """-> (keys_out [S, k] uint16, values or positions [S, k] uint32, counts [S] uint32): segment s is the first
    kept = min(k, len) of the stable sort of its clamped sub-array on the 16-bit image; the slots past kept hold the fill.
    cache: a dict that keeps the stable order of every distinct (b, len)."""
    keys = np.ascontiguousarray(keys).view(np.uint16)
    b, ln = SR.clamp(begin, end, keys.size)
    S = b.size
    ko, vo = np.full((S, k), FILL16, np.uint16), np.full((S, k), FILL, np.uint32)
    counts = np.minimum(ln, k).astype(np.uint32)
    cache = {} if cache is None else cache
    vals = None if values is None else np.ascontiguousarray(values).view(np.uint32)
    for s in range(S):
        kept, lo, n = int(counts[s]), int(b[s]), int(ln[s])
        if kept == 0:
            continue
        order = cache.get((lo, n))
        if order is None:
            img = NR.image16(keys[lo:lo + n], key_type, descending)
            order = cache[(lo, n)] = np.argsort(img, kind="stable").astype(np.uint32)
        o = order[:kept]
        ko[s, :kept] = keys[lo:lo + n][o]
        vo[s, :kept] = o if vals is None else vals[lo:lo + n][o]
    return ko, vo, counts


def via_widening(keys, begin, end, k, key_type, descending=False, values=None):
    """The identity of the header: the 32-bit reference on (uint32_t)key << 16 with the key type widened, the returned keys
    shifted right by 16 (an unwritten slot's 0xffffffff becomes 0xffff)."""
    ko, vo, counts = SR.seg_topk(NR.widen(keys), begin, end, k, WIDE[key_type], descending, values)
    return (ko >> np.uint32(16)).astype(np.uint16), vo, counts


def _a(x):
    return (x + 255) & ~255


def temp_bytes16(n, S, k, has_values):
    """The formula of the header comment of gs_topk_segmented_u16_temp_bytes."""
    if SR.refused(n, S, k) or n == 0 or S == 0 or k == 0:
        return 0
    lmax, tmax = SR.geometry(n, S)
    hv = 1 if has_values else 0
    return (4096 + 5 * _a(SR.REC_BYTES * S) + _a(SR.REC_BYTES * lmax) + _a(SR.TASK_BYTES * tmax)
            + _a(2 * k * tmax) + hv * _a(4 * k * tmax) + 256)


def flat_keys16(n, kt, seed, kinds=NR.DISTS):
    """n 16-bit keys in pieces of different distributions, so that the segments of one call see all of them."""
    piece = max(1, -(-n // (2 * len(kinds))))
    parts = [NR.gen16(kinds[(i + seed) % len(kinds)], min(piece, n - lo), seed=seed * 1009 + i + 1, kt=kt)
             for i, lo in enumerate(range(0, n, piece))]
    return np.concatenate(parts).astype(np.uint16)
