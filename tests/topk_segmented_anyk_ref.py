"""numpy reference of gs_topk_segmented_anyk_u32 (tests/test_topk_segmented_anyk_cpu.py, tests/test_topk_segmented_anyk_gpu.py):
the per-segment reference, which is topk_segmented_ref.seg_topk as it stands (FILL in the unwritten slots), the workspace
formula and the plan recomputed from the header's text, the list every length must land in, and the shapes the GPU file runs."""
import numpy as np

import topk_segmented_ref as SR

U32, I32, F32 = SR.U32, SR.I32, SR.F32
CH = SR.CH                    # elements one workgroup selects from; also the tile of the long segments' tasks
TILE = 8192
SLAB_TILES = 4                # tiles a count workgroup histograms before it adds to the segment's bins
BINS = 2048
FILL = SR.FILL
REC_BYTES, TASK_BYTES = SR.REC_BYTES, SR.TASK_BYTES

seg_topk = SR.seg_topk        # the reference: every segment is topk_ref's answer for its clamped sub-array at min(k, len)
clamp = SR.clamp
geometry = SR.geometry
list_of = SR.list_of
packed = SR.packed
status = SR.status            # the same eight words, aggregated the same way


# ----------------------------------------------------------------------------------- the plan and the workspace --
def refused(n, S, k):
    return n >= 1 << 31 or S * k >= 1 << 31


def plan(n, S, k):
    """gs_topk_segmented_anyk_plan's eight words (None for a refused shape)."""
    if refused(n, S, k):
        return None
    if n == 0 or S == 0 or k == 0:
        return [0] * 8
    groups = 1 | (2 if n > 1024 else 0) | (4 if n > CH else 0)
    launches = 6 + (2 if groups & 2 else 0) + (11 if groups & 4 else 0)
    lmax, tmax = geometry(n, S)
    return [groups, launches, CH, TILE, SLAB_TILES, lmax, tmax, 0]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(n, S, k, has_values, segmented_temp_bytes):
    """The formula of the header comment; segmented_temp_bytes = gs_segmented_temp_bytes(S * k, has_values, S)."""
    if refused(n, S, k) or n == 0 or S == 0 or k == 0:
        return 0
    lmax, tmax = geometry(n, S)
    hv = 1 if has_values else 0
    total = 4096 + 5 * _a(REC_BYTES * S) + _a(REC_BYTES * lmax) + _a(TASK_BYTES * tmax)
    total += _a(32 * lmax) + _a(4 * BINS * lmax) + _a(8 * tmax) + 2 * _a(4 * S)
    total += _a(4 * S * k) + 2 * hv * _a(4 * S * k)
    return total + _a(segmented_temp_bytes) + 256


# ------------------------------------------------------------------------------------------ the GPU file's shapes --
EDGE_LENGTHS = [0, 1, 64, 65, 256, 257, 512, 513, 1024, 1025, 8191, 8192, 8193, 16384, 16385, 32768, 32769, 65537]
EDGE_LISTS = [None, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 5, 5, 5, 5, 5]
EDGE_KS = [1, 1024, 1025, 5000, 8192, 8193, 40000, 70000]
EDGE_STATUS = [2, 2, 2, 2, 3, 6, 2 + 2 + 3 + 4 + 5 + 9, 0]

EQUAL_LENGTH, EQUAL_KS = 20000, [1, 8193, 19999]
LONG_COUNT = 1030             # long segments of CH + 1 elements: two classify workgroups
BLOCK_COUNTS = [1, 1023, 1025]
SWEEP_SEED, SWEEP_CASES = 20261, 40


def shuffled_edges(seed=1):
    """The edge lengths in shuffled order, laid out with odd gaps: -> (begin, end, num_items, lengths in call order)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(EDGE_LENGTHS))
    begin, end, at = np.zeros(len(order), np.int32), np.zeros(len(order), np.int32), 3
    for s in order:                      # segment s sits where the shuffle put it; the call lists them in EDGE_LENGTHS order
        begin[s], end[s] = at, at + EDGE_LENGTHS[s]
        at += EDGE_LENGTHS[s] + 1 + 2 * int(rng.integers(0, 4))
    return begin, end, at + 5, list(EDGE_LENGTHS)


def sweep_case(index, seed=SWEEP_SEED):
    """Case `index` of the seeded sweep: S <= 40 non-overlapping segments of log-uniform lengths in [0, 40000] in shuffled
    order with gaps, k in [1, 45000]: -> (rng, begin, end, num_items, k)."""
    rng = np.random.default_rng([seed, index])
    S = int(rng.integers(1, 41))
    lens = np.floor(np.exp(rng.uniform(0.0, np.log(40001.0), S))).astype(np.int64) - 1
    lens = np.clip(lens, 0, 40000)
    gaps = rng.integers(0, 4, S)
    order = rng.permutation(S)
    begin, end, at = np.zeros(S, np.int32), np.zeros(S, np.int32), int(rng.integers(0, 5))
    for s in order:
        begin[s], end[s] = at, at + int(lens[s])
        at += int(lens[s]) + int(gaps[s])
    k = int(np.floor(np.exp(rng.uniform(0.0, np.log(45000.0)))))
    return rng, begin, end, max(at, 1), max(1, min(k, 45000))
