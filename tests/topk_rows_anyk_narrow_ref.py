"""Reference of gs_topk_rows_anyk_u16 (tests/test_topk_rows_anyk_narrow_cpu.py, tests/test_topk_rows_anyk_narrow_gpu.py): the
per-row reference of topk_rows_narrow_ref / topk_narrow_ref (one stable argsort of the 16-bit image per row), the plan, the
workspace formula and the status of a row recomputed from the header's text, and the shape tables the two files share."""
import numpy as np

import topk_narrow_ref as N
import topk_rows_narrow_ref as NR

U16, I16, F16, BF16, KEY_TYPES, WIDE = NR.U16, NR.I16, NR.F16, NR.BF16, NR.KEY_TYPES, NR.WIDE
KEYS, PAIRS, ARGS, MODES = NR.KEYS, NR.PAIRS, NR.ARGS, NR.MODES
image16, preimage16, rows_topk16, rows_order, widen, matrix16, gen16, specials16 = (
    NR.image16, NR.preimage16, NR.rows_topk16, NR.rows_order, NR.widen, NR.matrix16, NR.gen16, NR.specials16)
keys_of = N.keys_of
CH = 8192             # longest row of path 1
TILE = 8192
BINS = 256
LAUNCHES = {1: 2, 2: 9}             # before the finish (the header's text at gs_topk_rows_anyk_u16_plan)


def refused(rows, cols, k):
    return k > cols or rows * cols >= 1 << 32 or rows * k >= 1 << 31


def plan(rows, cols, k, slab_tiles=4):
    """gs_topk_rows_anyk_u16_plan's eight words (None for a refused shape)."""
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


def temp_bytes(rows, cols, k, has_values, narrow_temp_bytes):
    """The formula of the header comment; narrow_temp_bytes = gs_segmented_narrow_temp_bytes(rows * k, GS_KEY_U16, 4 with values
    else 0, rows)."""
    if refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    hv = 1 if has_values else 0
    total = _a(32 * rows) + _a(4 * (rows + 1))
    if cols > CH:
        total += _a(4 * BINS * rows) + _a(8 * rows * -(-cols // TILE))
    total += _a(2 * rows * k) + 2 * hv * _a(4 * rows * k)
    return total + _a(narrow_temp_bytes) + 256


def status(row_keys, k, key_type, descending=False):
    """gs_topk_rows_anyk_u16_status's eight words for one row (uint16 bit patterns)."""
    img = np.sort(image16(row_keys, key_type, descending)).astype(np.uint32)
    kth = int(img[k - 1])
    less = int(np.searchsorted(img, np.uint32(kth), side="left"))
    path = 1 if img.size <= CH else 2
    m1 = int(np.count_nonzero((img >> np.uint32(8)) == (kth >> 8))) if path == 2 else 0
    return [path, kth, less, k - less, m1, 0, 0, 0]


# ------------------------------------------------------------------------------------------ the shared shape tables --
SLAB = 4 * TILE       # asserted against the plan by both files before it is used
PATH1_COLS = [1025, CH - 1, CH]
PATH1_ROWS = [1, 7]


def path1_ks(cols):
    return sorted({1, 1024, 1025, cols - 1, cols})


PATH2_COLS = [CH + 1, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 5, 3 * SLAB + TILE + 1]
PATH2_ROWS = [1, 3]


def path2_ks(cols):
    return sorted({1, 1025, 8192, 8193, cols - 1, cols})     # 8192 / 8193: the finish leaves its one-workgroup class


MANY_ROWS = (300, 9000, 1100)       # many rows of one slab each
SLAB_EDGE_COLS = [SLAB - 1, SLAB, SLAB + 1, 2 * SLAB, 2 * SLAB + 1]
LONG_COLS = 65536 + 4097            # more columns than 16-bit patterns: ties by force
GUARDED_SHAPES = [(3, 5000, 1500, 1), (2, SLAB + TILE + 7, 3000, 2)]     # (rows, cols, k, path)
GRAPH_SHAPES = [(5, 6000, 2000, 1), (2, SLAB + 9, 1500, 2)]
STRIDE_SHAPES = [(4000, 1200, 1), (CH, 1025, 1), (CH + 5, 2000, 2), (SLAB + 1, 9000, 2)]      # (cols, k, path) at row_stride = cols + 3
REUSE_SHAPES = [(3, SLAB + 9, 1300, 2), (6, 5000, 1100, 1)]
AGREE_SHAPES = [(4, 6000, 1), (3, SLAB + 77, 2)]                         # (rows, cols, path)
