"""Reference of gs_topk_rows_anyk_u32 (tests/test_topk_rows_anyk_cpu.py, tests/test_topk_rows_anyk_gpu.py): the per-row
reference (topk_rows_ref.rows_topk, which is topk_ref.Ref per row), the plan and the workspace formula recomputed from the
header's text, the expected status of a row, and the shape tables the two files share."""
import numpy as np

import topk_ref as R
import topk_rows_ref as RR

U32, I32, F32 = R.U32, R.I32, R.F32
rows_topk = RR.rows_topk
CH = 8192             # longest row of path 1
TILE = 8192
BINS = 2048
ROUND_SHIFTS = (21, 10, 0)          # the three digits: image bits 31-21, 20-10, 9-0
LAUNCHES = {1: 2, 2: 11}            # before the finish (the header's text at gs_topk_rows_anyk_plan)


def refused(rows, cols, k):
    return k > cols or rows * cols >= 1 << 32 or rows * k >= 1 << 31


def plan(rows, cols, k, slab_tiles=4):
    """gs_topk_rows_anyk_plan's eight words (None for a refused shape).  slab_tiles: what the library's rule gives."""
    if refused(rows, cols, k):
        return None
    if rows == 0 or cols == 0 or k == 0:
        return [0] * 8
    if cols <= CH:
        return [1, LAUNCHES[1], CH, TILE, 1, 1, 1, 0]
    tiles = -(-cols // TILE)
    return [2, LAUNCHES[2], CH, TILE, slab_tiles, -(-tiles // slab_tiles), tiles, 0]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(rows, cols, k, has_values, segmented_temp_bytes):
    """The formula of the header comment; segmented_temp_bytes = gs_segmented_temp_bytes(rows * k, has_values, rows)."""
    if refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    hv = 1 if has_values else 0
    total = _a(32 * rows) + _a(4 * (rows + 1))
    if cols > CH:
        total += _a(4 * BINS * rows) + _a(8 * rows * -(-cols // TILE))
    total += _a(4 * rows * k) + 2 * hv * _a(4 * rows * k)
    return total + _a(segmented_temp_bytes) + 256


def status(row_keys, k, key_type, descending=False):
    """gs_topk_rows_anyk_status's eight words for one row (u32 bit patterns)."""
    img = np.sort(R.image(row_keys, key_type, descending))
    kth = int(img[k - 1])
    less = int(np.searchsorted(img, np.uint32(kth), side="left"))
    path = 1 if img.size <= CH else 2
    m1 = m2 = 0
    if path == 2:
        m1 = int(np.count_nonzero((img >> np.uint32(21)) == (kth >> 21)))
        m2 = int(np.count_nonzero((img >> np.uint32(10)) == (kth >> 10)))
    return [path, kth, less, k - less, m1, m2, 0, 0]


# ------------------------------------------------------------------------------------------ the shared shape tables --
SLAB = 4 * TILE       # asserted against the plan by both files before it is used
PATH1_COLS = [1025, CH - 1, CH]
PATH1_ROWS = [1, 7]


def path1_ks(cols):
    return sorted({1, 1024, 1025, cols - 1, cols})


PATH2_COLS = [CH + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 5, 3 * SLAB + TILE + 1]
PATH2_ROWS = [1, 3]


def path2_ks(cols):
    ks = {1, 1025, 8192, cols - 1, cols}
    if cols == max(PATH2_COLS):
        ks |= {17408, 17409}        # the finish leaves the segmented sort's one-workgroup class
    return sorted(ks)


MANY_ROWS = (300, 9000, 1100)       # many rows of one slab each
SLAB_EDGE_COLS = [SLAB - 1, SLAB, SLAB + 1, 2 * SLAB, 2 * SLAB + 1]
GUARDED_SHAPES = [(3, 5000, 1500, 1), (2, SLAB + TILE + 7, 3000, 2)]     # (rows, cols, k, path)
GRAPH_SHAPES = [(5, 6000, 2000, 1), (2, SLAB + 9, 1500, 2)]
STRIDE_SHAPES = [(4000, 1200, 1), (CH, 1025, 1), (CH + 5, 2000, 2), (SLAB + 1, 9000, 2)]      # (cols, k, path) at row_stride = cols + 3
REUSE_SHAPES = [(3, SLAB + 9, 1300, 2), (6, 5000, 1100, 1)]
AGREE_SHAPES = [(4, 6000, 1), (3, SLAB + 77, 2)]                         # (rows, cols, path)
