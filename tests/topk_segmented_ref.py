"""numpy reference of gs_topk_segmented_u32 (tests/test_topk_segmented_cpu.py, tests/test_topk_segmented_gpu.py): the
per-segment reference built from topk_ref.Ref (clamping, empty segments, kept), the workspace formula and the plan recomputed
from the header's text, the list every segment must land in, a numpy model of the chunk level plus the streaming final with
the chunk size as a parameter, and the shapes the GPU file runs."""
import numpy as np

import topk_ref as R

U32, I32, F32 = R.U32, R.I32, R.F32
CH = 8192            # elements one workgroup selects from (gs_topk_segmented_plan's out[2])
MAX_K = 1024         # gs_topk_rows_max_k()
FILL = 0xFFFFFFFF    # what the tests put into the outputs before a call: slots that are not written keep it
REC_BYTES, TASK_BYTES = 16, 8


# ------------------------------------------------------------------------------------------------ the reference --
def clamp(begin, end, n):
    """(b, len) of every segment after the device's clamping: b = max(begin, 0), e = min(end, n), empty when e <= b."""
    b = np.maximum(np.asarray(begin, np.int64), 0)
    e = np.minimum(np.asarray(end, np.int64), n)
    ln = np.where(e > b, e - b, 0)
    return np.where(ln > 0, b, 0), ln


def seg_topk(keys, begin, end, k, key_type, descending=False, values=None, cache=None):
    """-> (keys_out [S, k], values or positions [S, k], counts [S]): segment s is topk_ref's answer for its clamped sub-array
    alone at kept = min(k, len); the slots past kept hold FILL.  cache: a dict that keeps the Ref of every distinct (b, len)."""
    keys = np.ascontiguousarray(keys).view(np.uint32)
    b, ln = clamp(begin, end, keys.size)
    S = b.size
    ko, vo = np.full((S, k), FILL, np.uint32), np.full((S, k), FILL, np.uint32)
    counts = np.minimum(ln, k).astype(np.uint32)
    cache = {} if cache is None else cache
    for s in range(S):
        kept, lo, n = int(counts[s]), int(b[s]), int(ln[s])
        if kept == 0:
            continue
        ref = cache.get((lo, n))
        if ref is None:
            ref = cache[(lo, n)] = R.Ref(keys[lo:lo + n], key_type, descending)
        order = ref.order[:kept]
        ko[s, :kept] = ref.keys[order]
        vo[s, :kept] = order if values is None else np.ascontiguousarray(values).view(np.uint32)[lo:lo + n][order]
    return ko, vo, counts


# ----------------------------------------------------------------------------------- the plan and the workspace --
def refused(n, S, k):
    return k > MAX_K or n >= 1 << 31 or S * k >= 1 << 32


def geometry(n, S):
    lmax = min(S, n // (CH + 1))
    return lmax, (n // CH + lmax if lmax else 0)


def plan(n, S, k):
    """gs_topk_segmented_plan's eight words (None for a refused shape)."""
    if refused(n, S, k):
        return None
    if n == 0 or S == 0 or k == 0:
        return [0] * 8
    groups = 1 | (2 if n > 1024 else 0) | (4 if n > CH else 0)
    launches = 2 + 4 + (1 if groups & 2 else 0) + (3 if groups & 4 else 0)
    lmax, tmax = geometry(n, S)
    return [groups, launches, CH, lmax, tmax, MAX_K, 0, 0]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(n, S, k, has_values):
    """The formula of the header comment."""
    if refused(n, S, k) or n == 0 or S == 0 or k == 0:
        return 0
    lmax, tmax = geometry(n, S)
    v = 2 if has_values else 1
    return 4096 + 5 * _a(REC_BYTES * S) + _a(REC_BYTES * lmax) + _a(TASK_BYTES * tmax) + v * _a(4 * k * tmax) + 256


def list_of(length):
    """The list a segment of `length` elements lands in: 0..3 the wave lists, 4 the workgroup list, 5 the long list, None."""
    if length == 0:
        return None
    for q, cap in enumerate((64, 256, 512, 1024, CH)):
        if length <= cap:
            return q
    return 5


def status(begin, end, n):
    """gs_topk_segmented_status's eight words for offsets whose long segments all find room (nothing dropped)."""
    _, ln = clamp(begin, end, n)
    out = [0] * 8
    for x in ln:
        q = list_of(int(x))
        if q is not None:
            out[q] += 1
            if q == 5:
                out[6] += -(-int(x) // CH)
    lmax, tmax = geometry(n, len(ln))
    assert out[5] <= lmax and out[6] <= tmax, "these offsets would drop a segment: the lengths above CH exceed num_items"
    return out


def next_of(n, k, ch=CH):
    c = -(-n // ch)
    return (c - 1) * k + min(k, n - (c - 1) * ch)


def final_rounds(length, k, ch=CH):
    """Streaming rounds of the final of a long segment: the first takes ch candidates, every later one ch - k."""
    n1, rounds, pos, kc = next_of(length, k, ch), 0, 0, 0
    while True:
        take = min(ch - kc, n1 - pos)
        kc, pos, rounds = min(k, kc + take), pos + take, rounds + 1
        if pos >= n1:
            return rounds


# ------------------------------------------------------------------------ the model of the long-segment kernels --
def _select_compact(img, pos, keff, variant=None):
    """tr_select + the ordered compaction on one (virtual) chunk in input order: group A (before the keff-th image) in input
    order, then the first keff - |A| of the elements equal to it, in input order.  variant: a WRONG version (see stream_model)."""
    kth = np.sort(img, kind="stable")[keff - 1]
    a = np.nonzero(img < kth)[0]
    b = np.nonzero(img == kth)[0]
    take = keff - a.size
    if variant == "unstable_cut":
        b = b[b.size - take:]                 # the LAST of the tie run
    elif variant == "cut_early":
        b = b[:take - 1]
    elif variant == "cut_late":
        b = b[1:take + 1]                     # the window into the tie run starts one late
    else:
        b = b[:take]
    sel = np.concatenate([a, b])
    return img[sel], pos[sel]


def stream_model(keys, k, key_type, descending=False, ch=CH, variant=None):
    """One segment longer than ch, as the kernels do it: every chunk of ch gives its first min(k, length) by (image, position),
    sorted, to the candidate row; the final streams that row in rounds -- the kc carried pairs first, in the order the last
    compaction left them, then the next ch - kc candidates -- selects and compacts again, and sorts the stage (stably, by
    image) at the end.  -> (keys_out, positions, rounds).
    variant names a deliberately wrong model: "carried_after" (carried pairs behind the new candidates), "unstable_cut",
    "cut_early", "cut_late" (the tie run cut at the wrong place)."""
    keys = np.ascontiguousarray(keys).view(np.uint32)
    img = R.image(keys, key_type, descending)
    ci, cp = [], []
    for lo in range(0, img.size, ch):
        seg = img[lo:lo + ch]
        order = np.argsort(seg, kind="stable")[:min(k, seg.size)]
        ci.append(seg[order])
        cp.append((lo + order).astype(np.uint32))
    ci, cp = np.concatenate(ci), np.concatenate(cp)
    assert ci.size == next_of(img.size, k, ch)
    si, sp = np.empty(0, np.uint32), np.empty(0, np.uint32)
    at = rounds = 0
    while True:
        take = min(ch - si.size, ci.size - at)
        if variant == "carried_after":
            vi, vp = np.concatenate([ci[at:at + take], si]), np.concatenate([cp[at:at + take], sp])
        else:
            vi, vp = np.concatenate([si, ci[at:at + take]]), np.concatenate([sp, cp[at:at + take]])
        si, sp = _select_compact(vi, vp, min(k, vi.size), variant)
        at, rounds = at + take, rounds + 1
        if at >= ci.size:
            break
    order = np.argsort(si, kind="stable")
    return R.preimage(si[order], key_type, descending), sp[order], rounds


# ------------------------------------------------------------------------------------------ the GPU file's shapes --
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, CH - 1, CH, CH + 1, 2 * CH + 1]
EDGE_LISTS = [None, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5]
EDGE_KS = [1, 8, 64, 65, 1000, 1024]

# (length, k, streaming rounds of the final)
LONG_SHAPES = [(8 * CH + 1, 1024, 2), (15 * CH + 1, 1024, 3), (3 * CH + 77, 1, 1)]

LIST_COUNTS = [1, 3, 4, 5, 1000, 4099]          # segments of one class: around a workgroup's share of four, and a strided grid
CLASS_LENGTHS = [40, 200, 400, 900]             # one length per wave class for those


def packed(lengths, gap=0, first=0):
    """Offsets of segments laid one after the other: -> (begin, end, num_items)."""
    begin, at = [], first
    for x in lengths:
        begin.append(at)
        at += x + gap
    begin = np.array(begin, np.int32)
    return begin, (begin + np.array(lengths, np.int32)).astype(np.int32), at
