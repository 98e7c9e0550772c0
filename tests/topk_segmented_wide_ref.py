"""numpy reference of gs_topk_segmented_u64 (tests/test_topk_segmented_wide_cpu.py, tests/test_topk_segmented_wide_gpu.py), built
on topk_segmented_ref (clamping, geometry, status, shapes) and topk_rows_wide_ref / topk_wide_ref (the 64-bit image maps, the
builders): the per-segment stable argsort of the 64-bit image, the workspace formula recomputed from the header's text, the
widening identity of the header ((uint64_t)key << 32 through the 32-bit reference, the returned keys shifted right by 32), and
a model of the long-segment kernels at 64 bits: topk_segmented_ref.stream_model with the select written out byte by byte and
the AND / OR skip of its rounds."""
import numpy as np

import topk_rows_wide_ref as WR
import topk_segmented_ref as SR
import topk_wide_ref as W

U64, I64, F64 = W.U64, W.I64, W.F64
KEY_TYPES = W.KEY_TYPES
WIDE = WR.WIDE
KEYS, PAIRS, ARGS = W.KEYS, W.PAIRS, W.ARGS
MODES = W.MODES
CH, MAX_K = SR.CH, SR.MAX_K
FILL = SR.FILL                                  # unwritten u32 slots (values, positions, counts)
FILL64 = np.uint64(0xFFFFFFFFFFFFFFFF)          # unwritten key slots
image, preimage, u64 = W.image, W.preimage, W.u64


def seg_topk64(keys, begin, end, k, key_type, descending=False, values=None, cache=None):
    """-> (keys_out [S, k] uint64, values or positions [S, k] uint32, counts [S] uint32): segment s is the first
    kept = min(k, len) of the stable sort of its clamped sub-array on the 64-bit image; the slots past kept hold the fill.
    cache: a dict that keeps the stable order of every distinct (b, len)."""
    keys = u64(keys)
    b, ln = SR.clamp(begin, end, keys.size)
    S = b.size
    ko, vo = np.full((S, k), FILL64, np.uint64), np.full((S, k), FILL, np.uint32)
    counts = np.minimum(ln, k).astype(np.uint32)
    cache = {} if cache is None else cache
    vals = None if values is None else np.ascontiguousarray(values).view(np.uint32)
    for s in range(S):
        kept, lo, n = int(counts[s]), int(b[s]), int(ln[s])
        if kept == 0:
            continue
        order = cache.get((lo, n))
        if order is None:
            order = cache[(lo, n)] = np.argsort(image(keys[lo:lo + n], key_type, descending), kind="stable").astype(np.uint32)
        o = order[:kept]
        ko[s, :kept] = keys[lo:lo + n][o]
        vo[s, :kept] = o if vals is None else vals[lo:lo + n][o]
    return ko, vo, counts


def via_widening(keys32, begin, end, k, key_type32, descending=False, values=None):
    """The identity of the header, from the 32-bit side: what gs_topk_segmented_u64 must give on (uint64_t)key << 32 with the
    key type widened is the 32-bit reference's answer with the keys shifted left by 32 (an unwritten slot stays all ones)."""
    ko, vo, counts = SR.seg_topk(keys32, begin, end, k, key_type32, descending, values)
    wide = ko.astype(np.uint64) << np.uint64(32)
    for s in range(ko.shape[0]):
        wide[s, int(counts[s]):] = FILL64
    return wide, vo, counts


def _a(x):
    return (x + 255) & ~255


def temp_bytes64(n, S, k, has_values):
    """The formula of the header comment of gs_topk_segmented_u64_temp_bytes."""
    if SR.refused(n, S, k) or n == 0 or S == 0 or k == 0:
        return 0
    lmax, tmax = SR.geometry(n, S)
    hv = 1 if has_values else 0
    return (4096 + 5 * _a(SR.REC_BYTES * S) + _a(SR.REC_BYTES * lmax) + _a(SR.TASK_BYTES * tmax)
            + _a(8 * k * tmax) + hv * _a(4 * k * tmax) + 256)


# ------------------------------------------------------------------------ the model of the long-segment kernels --
def select_skip(img, keff, reduce_over=None):
    """The 64-bit select on one (virtual) chunk: AND and OR over the in-range images, then most significant byte first, a
    round (a 256-bin histogram over the elements that still match the prefix, and a pick) for every byte in which two of them
    differ; a constant byte goes into the prefix as it is.  -> (k-th image, less, the bytes that took a round).
    reduce_over: the elements the AND / OR see -- all of them (None) in the kernel; a WRONG model passes a part."""
    seen = img if reduce_over is None else reduce_over
    a, o = int(np.bitwise_and.reduce(seen)), int(np.bitwise_or.reduce(seen))
    differ = a ^ o
    prefix, less, krem, ran = 0, 0, keff, []
    for b in range(7, -1, -1):
        shift = 8 * b
        if (differ >> shift) & 255 == 0:
            prefix |= a & (255 << shift)
            continue
        ran.append(b)
        mask = 0 if b == 7 else (~0 << (shift + 8)) & 0xFFFFFFFFFFFFFFFF
        match = ((img ^ np.uint64(prefix)) & np.uint64(mask)) == 0
        cnt = np.bincount(W.byte_of(img[match], b), minlength=256)
        ex = np.cumsum(cnt) - cnt
        pick = np.flatnonzero((ex < krem) & (krem - ex <= cnt))
        assert pick.size == 1, "exactly one bin holds the k-th element"
        d = int(pick[0])
        prefix |= d << shift
        less += int(ex[d])
        krem -= int(ex[d])
    return np.uint64(prefix), less, ran


def _compact(img, pos, keff, kth, less):
    a = np.nonzero(img < kth)[0]
    b = np.nonzero(img == kth)[0][:keff - less]
    sel = np.concatenate([a[:less], b])
    return img[sel], pos[sel]


def stream_model64(keys, k, key_type, descending=False, ch=CH, variant=None):
    """topk_segmented_ref.stream_model at 64 bits, the select by select_skip: every chunk of ch gives its first
    min(k, length) by (image, position), sorted, to the candidate row; the final streams that row in rounds -- the kc carried
    pairs first, then the next ch - kc candidates --, selects with the byte skip, compacts, and sorts the stage stably at the
    end.  -> (keys_out, positions, streaming rounds, per round the bytes whose select round ran).
    variant "reduce_new_only": a deliberately WRONG model whose AND / OR see the new candidates alone, not the carried pairs."""
    img = image(u64(keys), key_type, descending)
    ci, cp = [], []
    for lo in range(0, img.size, ch):
        seg = img[lo:lo + ch]
        order = np.argsort(seg, kind="stable")[:min(k, seg.size)]
        ci.append(seg[order])
        cp.append((lo + order).astype(np.uint32))
    ci, cp = np.concatenate(ci), np.concatenate(cp)
    assert ci.size == SR.next_of(img.size, k, ch)
    si, sp = np.empty(0, np.uint64), np.empty(0, np.uint32)
    at, rounds, ran = 0, 0, []
    while True:
        take = min(ch - si.size, ci.size - at)
        vi, vp = np.concatenate([si, ci[at:at + take]]), np.concatenate([sp, cp[at:at + take]])
        keff = min(k, vi.size)
        kth, less, r = select_skip(vi, keff, ci[at:at + take] if variant == "reduce_new_only" else None)
        si, sp = _compact(vi, vp, keff, kth, less)
        ran.append(r)
        at, rounds = at + take, rounds + 1
        if at >= ci.size:
            break
    order = np.argsort(si, kind="stable")
    return preimage(si[order], key_type, descending), sp[order], rounds, ran


# ------------------------------------------------------------------------------------------------------ inputs --
def flat_keys64(n, kt, seed, kinds=W.DISTS):
    """n 64-bit keys in pieces of different distributions, so that the segments of one call see all of them."""
    piece = max(1, -(-n // (2 * len(kinds))))
    parts = [W.gen64(kinds[(i + seed) % len(kinds)], min(piece, n - lo), seed=seed * 1009 + i + 1, kt=kt)
             for i, lo in enumerate(range(0, n, piece))]
    return np.concatenate(parts).astype(np.uint64)


def carried_outlier_segment(k, b, seed=0):
    """Images of one long segment (three streaming rounds at k = 1024): chunk 0 holds the k smallest images, all BASE but for
    ONE that differs from BASE in byte b alone (smaller); every later chunk is BASE + 1 throughout.  After round one the stage
    carries chunk 0's k; the later rounds' new candidates are one image, and only the carried outlier makes byte b vary."""
    n = 15 * CH + 1
    img = np.full(n, WR.BASE + np.uint64(1), np.uint64)
    img[:k] = WR.BASE
    at = int(np.random.default_rng(seed).integers(0, k))
    img[at] = WR.BASE & ~(np.uint64(0xFF) << np.uint64(8 * b)) | (np.uint64(0x01) << np.uint64(8 * b))
    return img, at


def late_outlier_segment(k, b):
    """The mirror: every image is BASE, so the carried pairs are all equal, but for one in the LAST chunk -- a new candidate
    of the last round -- that is smaller in byte b alone.  It must come out first; the other k - 1 are positions 0 .. k - 2."""
    n = 15 * CH + 1
    img = np.full(n, WR.BASE, np.uint64)
    at = n - 1
    img[at] = WR.BASE & ~(np.uint64(0xFF) << np.uint64(8 * b)) | (np.uint64(0x01) << np.uint64(8 * b))
    return img, at
