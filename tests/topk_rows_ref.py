"""numpy reference of gs_topk_rows_u32 (tests/test_topk_rows_cpu.py, tests/test_topk_rows_gpu.py): the per-row reference built
from topk_ref.Ref, the plan and the workspace formula recomputed from the header's text, a numpy model of the chunked
scheme of path 3, and the shapes the GPU file runs (so that the CPU file can assert each shape's path with the plan alone)."""
import numpy as np

import topk_ref as R

U32, I32, F32 = R.U32, R.I32, R.F32
CH = 8192            # elements one workgroup selects from (gs_topk_rows_plan's out[2])
MAX_K = 1024         # gs_topk_rows_max_k()
WAVE_COLS = 1024     # longest row of path 1


def rows_topk(mat, cols, k, key_type, descending=False, values=None):
    """mat: [rows, stride] u32 bit patterns, of which the first `cols` of every row count.  -> (keys [rows, k],
    values or column indices [rows, k]): row r is topk_ref's answer for mat[r, :cols] alone."""
    mat = np.ascontiguousarray(mat).view(np.uint32)
    rows = mat.shape[0]
    ko, vo = np.empty((rows, k), np.uint32), np.empty((rows, k), np.uint32)
    for r in range(rows):
        ref = R.Ref(mat[r, :cols], key_type, descending, None if values is None else values[r, :cols])
        ko[r], vo[r], _ = ref.topk(k)
    return ko, vo


def _next(n, k, ch=CH):
    c = -(-n // ch)
    return (c - 1) * k + min(k, n - (c - 1) * ch)


def level_sizes(cols, k, ch=CH):
    """Elements per (candidate) row that each level reads: [cols, n1, n2, ...]; the last one fits a chunk."""
    ns = [cols]
    while ns[-1] > ch:
        ns.append(_next(ns[-1], k, ch))
    return ns


def refused(rows, cols, k):
    return k > cols or k > MAX_K or rows * cols >= 1 << 32 or rows * k >= 1 << 32


def plan(rows, cols, k):
    """gs_topk_rows_plan's eight words (None for a refused shape)."""
    if refused(rows, cols, k):
        return None
    if rows == 0 or cols == 0 or k == 0:
        return [0] * 8
    if cols <= WAVE_COLS:
        return [1, 1, CH, 1, k, MAX_K, 0, 0]
    if cols <= CH:
        return [2, 1, CH, 1, k, MAX_K, 0, 0]
    ns = level_sizes(cols, k)
    return [3, len(ns), CH, -(-cols // CH), ns[1], MAX_K, 0, 0]


def _a(x):
    return (x + 255) & ~255


def temp_bytes(rows, cols, k, has_values):
    """The formula of the header comment."""
    if refused(rows, cols, k) or rows == 0 or cols == 0 or k == 0:
        return 0
    n1 = _next(cols, k) if cols > CH else 0
    n2 = _next(n1, k) if n1 > CH else 0
    v = 2 if has_values else 1
    return v * _a(4 * rows * n1) + v * _a(4 * rows * n2) + 256


def chunk_model(keys, k, key_type, descending=False, ch=CH, carry_columns=True):
    """The chunked scheme of path 3 on one row, in numpy: every level cuts its source into chunks of `ch`, takes each chunk's
    first min(k, length) by (image, position) and concatenates them; with one chunk left, that chunk's answer is the result.
    carry_columns=False is the keys-only form: keys travel alone.  -> (keys_out, columns or None, levels)."""
    keys = np.ascontiguousarray(keys).view(np.uint32)
    img = R.image(keys, key_type, descending)
    col = np.arange(keys.size, dtype=np.uint32)
    levels = 0
    while True:
        levels += 1
        out_i, out_c = [], []
        for lo in range(0, img.size, ch):
            seg = img[lo:lo + ch]
            order = np.argsort(seg, kind="stable")[:min(k, seg.size)]      # ties by position in the source row
            out_i.append(seg[order])
            out_c.append(col[lo:lo + ch][order])
        single = img.size <= ch
        img, col = np.concatenate(out_i), np.concatenate(out_c)
        if single:
            break
    return R.preimage(img, key_type, descending), (col if carry_columns else None), levels


# ------------------------------------------------------------------------------------------ the GPU file's shapes --
PATH1_COLS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
PATH1_ROWS = [1, 3, 4, 5, 1000]


def path1_ks(cols):
    return sorted({k for k in (1, 2, cols // 2, cols - 1, cols) if 1 <= k <= cols})


PATH2_COLS = [1025, CH - 1, CH]
PATH2_KS = [1, 64, 65, 1023, 1024]
PATH2_ROWS = [1, 7]

THREE_LEVELS_COLS = CH * -(-CH // 1024) + 1          # at k = 1024: level 0 leaves more than one chunk of candidates
# (rows, cols, k, expected levels)
PATH3_SHAPES = [
    (3, CH + 1, 64, 2),
    (2, CH + 5, 1024, 2),          # the last chunk gives fewer than k
    (5, 2 * CH, 100, 2),
    (2, 2 * CH + 1, 1023, 2),
    (3, THREE_LEVELS_COLS, 1024, 3),
    (4, 3 * CH + 77, 1, 2),
]

# the other tests' shapes, each with the (path, levels) it is meant to take
# (rows, cols, k, levels): three levels with a finishing wave of 1, 4 and 8 per lane -- the smallest row whose level 0 leaves more
# than one chunk of candidates, CH * (CH / k) + 1 columns -- so that the middle level (a source that carries columns, a
# destination that is a candidate row again) runs in every class; THREE_LEVELS_COLS above is the one of 16 per lane
MIDDLE_SHAPES = [(1, CH * (CH // k) + 1, k, 3) for k in (64, 256, 512)]
STRIDE_SHAPES = [      # (cols, k, path, levels) at 5 rows and row_stride = cols + 3
    (5, 5, 1, 1), (64, 8, 1, 1), (257, 100, 1, 1), (1024, 1024, 1, 1), (1025, 64, 2, 1), (CH, 1024, 2, 1), (CH + 5, 1024, 3, 2),
    (2 * CH + 1, 50, 3, 2),
]
GUARDED_SHAPES = [(5, 300, 7, 1, 1), (3, 4000, 100, 2, 1), (2, CH + 5, 1024, 3, 2), (2, THREE_LEVELS_COLS, 64, 3, 2)]   # (rows, cols, k, ..)
GRAPH_SHAPES = [(9, 200, 8, 1, 1), (3, 3000, 64, 2, 1), (2, THREE_LEVELS_COLS, 1024, 3, 3)]
REUSE_SHAPES = [(4, 2 * CH + 9, 300, 3, 2), (6, 5000, 77, 2, 1)]
