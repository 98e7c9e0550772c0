"""Input builders and shape tables of the top-k-rows edge tests (tests/test_topk_rows_edges_cpu.py,
tests/test_topk_rows_edges_gpu.py): plain numpy.

As in tests/topk_cases.py, every builder lays out IMAGES -- the order-preserving u32 words the kernels select on -- and
returns the keys that have those images for the given key type and direction (topk_ref.preimage), so a case's k-th image,
its cut and the wave or chunk that holds its winners are the same whatever the type and direction.  Position j of a chunk of
CH = 8192 elements is wave j // 1024, ballot row (j % 1024) // 64, lane j % 64 of the block kernel.  The CPU file holds
every case to its intent before a device sees it."""
import numpy as np

import topk_cases as T
import topk_ref as R
import topk_rows_ref as RR

U32, I32, F32 = R.U32, R.I32, R.F32
KEY_TYPES = (U32, I32, F32)
TYPES_DIRS = [(kt, desc) for kt in KEY_TYPES for desc in (False, True)]
KEYS, PAIRS, ARGS = T.KEYS, T.PAIRS, T.ARGS
MODES = T.MODES
CH = RR.CH
WAVE_ELEMS = 1024         # elements of a chunk one wave of the block kernel holds: 16 ballot rows of 64 lanes
PAD = 0xFFFFFFFF          # the image of a pad, in path 1 and in the finishing wave


def rotate(i):
    """(key type, descending, form) of the i-th case of a group."""
    return KEY_TYPES[i % 3], bool((i // 3) % 2), MODES[(i // 2) % 3]


def where(j):
    """(wave, ballot row, lane) of position j of a chunk."""
    return j // WAVE_ELEMS, (j % WAVE_ELEMS) // 64, j % 64


def k_class(k):
    """WKPT of the finishing wave: tr_launch_block's class in k."""
    return 1 if k <= 64 else 4 if k <= 256 else 8 if k <= 512 else 16


def cols_class(cols):
    """WKPT of path 1: the class in cols."""
    return 1 if cols <= 64 else 4 if cols <= 256 else 8 if cols <= 512 else 16


def _keys(img, kt, desc):
    return R.preimage(np.ascontiguousarray(np.asarray(img, dtype=np.uint64).astype(np.uint32)), kt, desc)


def dist_matrix(rows, cols, kt, seed, kinds, stride=None):
    """[rows, stride] key words: row r is topk_cases.gen(kinds[(r + seed) % len(kinds)]) on a seed of its own."""
    m = np.zeros((rows, stride or cols), np.uint32)
    for r in range(rows):
        m[r, :cols] = T.gen(kinds[(r + seed) % len(kinds)], cols, seed=seed * 1009 + r + 1, kt=kt)
    return m


# ---------------------------------------------------------------------------- 1. deep levels and workspace reuse --
# (rows, cols, k, levels): 2 levels with one full chunk of candidates, the full boundary below 4 and below 5 levels and the
# first shape above each, and the same edges at k = 512 and around k = 256 (the class edge of the finishing wave)
DEEP_SHAPES = [
    (2, 65536, 1024, 2),
    (2, 524288, 1024, 3),
    (2, 524289, 1024, 4),
    (1, 4194304, 1024, 4),
    (1, 4194305, 1024, 5),
    (1, 2097153, 512, 4),
    (2, 262145, 256, 3),
    (2, 262145, 257, 3),
]
DEEP_KINDS = ("uniform", "five", "special")
# the two 16 MiB rows: one key type, direction and distribution each (a reference is one stable argsort of 4M keys)
DEEP_SINGLE = {4194304: (F32, False, "special"), 4194305: (I32, True, "five")}
DEEP_EQUAL = [(2, 524288, 1024, 3), (2, 524289, 1024, 4)]
DEEP_ARENA = (2, 524289, 1024, 4)


def deep_runs(shape):
    """[(key type, descending, kinds of the rows)] of a deep shape: every distribution with every key type somewhere, the f32
    specials (NaNs, -0.0, the infinities) always as f32."""
    rows, cols, k, _ = shape
    if cols in DEEP_SINGLE:
        kt, desc, kind = DEEP_SINGLE[cols]
        return [(kt, desc, [kind])]
    si = DEEP_SHAPES.index(shape)
    return [(U32, bool(si % 2), ["uniform", "five"]), (I32, not si % 2, ["five", "uniform"]), (F32, bool(si // 2 % 2), ["special", "five"]),
            (F32, not si // 2 % 2, ["uniform", "special"])]


def deep_matrix(shape, run):
    rows, cols, _, _ = shape
    kt, _, kinds = run
    return dist_matrix(rows, cols, kt, 7 + DEEP_SHAPES.index(shape), kinds)


def deep_row_kinds(shape, run):
    """The distribution of every row of deep_matrix(shape, run)."""
    seed = 7 + DEEP_SHAPES.index(shape)
    return [run[2][(r + seed) % len(run[2])] for r in range(shape[0])]


def equal_matrix(rows, cols, kt, desc, img=0x42A55A01):
    return np.tile(T.equal_case(cols, kt, desc, img), (rows, 1))


# ------------------------------------------------------------------------------ 2. finishing-wave classes in k --
CLASS_KS = [63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
CLASS_SHAPES = [(3, CH, 2, 1), (2, 2 * CH + 1, 3, 2)]               # (rows, cols, path, levels)
CLASS_KINDS = ("uniform", "five")


# --------------------------------------------------------------------------- 3. row lengths of the block kernel --
LENGTH_COLS = [1025, 1087, 1088, 1089, 2047, 2048, 2049, 4095, 4096, 4097, 7167, 7168, 7169, 8191, 8192]
LENGTH_ROWS = 3
LENGTH_KINDS = ("uniform", "five", "special")
TAIL_KS = [100, 1024]


def length_ks(cols):
    return [1, 64, min(cols, 1024)]


def tail_lengths(k):
    """Lengths of the short last chunk of a path-3 row of CH + t columns."""
    return [1, 63, 64, 65, k - 1, k, k + 1]


# ------------------------------------------------------------------------------ 4. select-digit edges and pads --
DIGIT_RUN_LENGTHS = (1, 2, 63, 64, 65)
DIGIT_BASE = sum(DIGIT_RUN_LENGTHS) * len(T.IMAGES20) // len(DIGIT_RUN_LENGTHS)          # 780
DIGIT_VARIANTS = [("a", DIGIT_BASE), ("b", 5000), ("b", 2 * CH + 77), ("c", 5000), ("c", 2 * CH + 77)]     # (variant, cols)
DIGIT_ROWS = 2
PAD_COLS = [1, 63, 65, 257, 1000]
PAD_ROWS = 5


def digit_runs():
    """[(image, run length)] of the base row: the twenty images, run lengths cycling through 1, 2, 63, 64, 65."""
    return [(img, DIGIT_RUN_LENGTHS[i % len(DIGIT_RUN_LENGTHS)]) for i, img in enumerate(T.IMAGES20)]


def digit_images(cols, variant, seed):
    """One shuffled row of images.  a: the base row (cols <= 780 takes that many of its elements at random, the campaign's
    short rows); b: filled up to cols with further copies of the pad image 0xFFFFFFFF; c: filled with image 0 instead."""
    rng = np.random.default_rng([seed, cols])
    base = np.repeat(np.array([i for i, _ in digit_runs()], np.uint64), [ln for _, ln in digit_runs()])
    if cols <= base.size:
        assert variant == "a" or cols < base.size
        return base[rng.permutation(base.size)[:cols]]
    assert variant in ("b", "c")
    img = np.concatenate([base, np.full(cols - base.size, PAD if variant == "b" else 0, np.uint64)])
    return img[rng.permutation(cols)]


def digit_matrix(variant, cols, kt, desc, rows=DIGIT_ROWS, seed=5):
    """Rows with the same images in shuffles of their own: the cuts of one row are the cuts of all."""
    return np.stack([_keys(digit_images(cols, variant, seed + r), kt, desc) for r in range(rows)])


def digit_ks(variant, cols, ref):
    """[(k, form)]: every k of run_cuts up to min(cols, 1024), and 1 and that limit.  Variant c's first run is longer than 1024,
    so every k cuts it and run_cuts has no k in range: it runs the cuts of the base row.  The form rotates; the arguments
    form is run at least at every run's end."""
    lim = min(cols, 1024)
    ks = set(k for k in T.run_cuts(ref) if k <= lim) | {1, lim}
    ends = set(np.cumsum([ln for _, ln in digit_runs()]).tolist())
    if variant == "c":
        ks |= set(k for e in ends for k in (e - 1, e, e + 1) if 1 <= k <= lim)
    return [(k, ARGS if k in ends else MODES[j % 3]) for j, k in enumerate(sorted(ks))]


def pad_matrix(cols, kt, desc, rows=PAD_ROWS):
    """Every key has the image of a pad."""
    return np.tile(_keys(np.full(cols, PAD, np.uint64), kt, desc), (rows, 1))


def pad_ks(cols):
    return sorted({cols, cols // 2 + 1})


# ---------------------------------------------------------------------------------------- 5. compaction edges --
CUT_T = 0x40000000           # the image of the tie run
CUT_BELOW = 5                # a: images below T, two in wave 0 and three in wave 7 behind elements equal to T
CUT_LEAD = 30                # the run starts 30 elements before the wave boundary 1024 * w
CUT_TS = [1, 29, 30, 31, 94, 95]
CUT_WAVES = list(range(1, 8))
ONE_WAVE_KS = [64, 63]
COMPACT_FORMS = [(1, 2, 1), (2, 3, 2)]             # (chunks, path, levels): the chunk alone, and as chunk 1 behind a chunk of losers


def _losers(rng, count, above):
    return rng.integers(above + 1, 1 << 32, count, dtype=np.uint64)


def _in_chunks(img, chunks, rng):
    """The chunk as the last of `chunks`: the chunks in front hold only losers (images above every image of the chunk's first k)."""
    if chunks == 1:
        return img
    return np.concatenate([_losers(rng, (chunks - 1) * CH, CUT_T), img])


def cut_images(w, chunks, seed=11):
    """Image T at every position from 1024 * w - 30 to the chunk's end, larger random images before; two images below T in
    wave 0, three in wave 7 at least two ballot rows behind its start (so behind elements equal to T, and behind every cut)."""
    rng = np.random.default_rng([seed, w])
    img = np.full(CH, CUT_T, np.uint64)
    start = WAVE_ELEMS * w - CUT_LEAD
    img[:start] = _losers(rng, start, CUT_T)
    below = np.uint64(CUT_T) - 1 - rng.permutation(CUT_BELOW).astype(np.uint64)
    at = np.concatenate([rng.choice(900, 2, replace=False), 7 * WAVE_ELEMS + 128 + rng.choice(WAVE_ELEMS - 128, 3, replace=False)])
    img[at] = below
    return _in_chunks(img, chunks, rng)


def cut_matrix(chunks, kt, desc):
    return np.stack([_keys(cut_images(w, chunks), kt, desc) for w in CUT_WAVES])


def one_wave_images(w, chunks, seed=13):
    """64 winners at random positions of wave w, everything else larger."""
    rng = np.random.default_rng([seed, w])
    img = _losers(rng, CH, CUT_T)
    img[WAVE_ELEMS * w + rng.choice(WAVE_ELEMS, 64, replace=False)] = rng.integers(0, CUT_T, 64, dtype=np.uint64)
    return _in_chunks(img, chunks, rng)


def one_wave_matrix(chunks, kt, desc):
    return np.stack([_keys(one_wave_images(w, chunks), kt, desc) for w in range(8)])


# ------------------------------------------------------------------------------- 6. where the winners lie --
SPREAD_COLS = 3 * CH + 77                    # four chunks, the last one short
SPREAD_K = 70
SPREAD_TIE_KS = [10, 15, 16, 25, 26, 35]
L1_COLS, L1_K, L1_N1 = 10 * CH, 1024, 10240  # 3 levels: level 1 reads two chunks of candidates, 8192 and 2048
L1_KS = [1000, 1001, 1024]
L1_ROWS = 2


def _chunk_positions(rng, cols, c, count):
    lo, hi = c * CH, min(cols, (c + 1) * CH)
    return lo + rng.choice(hi - lo, count, replace=False)


def one_chunk_images(c, seed=17):
    """All 70 winners in chunk c: every other chunk contributes 70 losing candidates."""
    rng = np.random.default_rng([seed, c])
    img = _losers(rng, SPREAD_COLS, CUT_T)
    img[_chunk_positions(rng, SPREAD_COLS, c, SPREAD_K)] = rng.integers(0, CUT_T, SPREAD_K, dtype=np.uint64)
    return img


def one_chunk_matrix(kt, desc):
    return np.stack([_keys(one_chunk_images(c), kt, desc) for c in range(4)])


def one_per_chunk_images(seed=19):
    rng = np.random.default_rng(seed)
    img = _losers(rng, SPREAD_COLS, CUT_T)
    for c in range(4):
        img[_chunk_positions(rng, SPREAD_COLS, c, 1)] = rng.integers(0, CUT_T, 1, dtype=np.uint64)
    return img


def thin_tie_images(seed=23):
    """T at ten scattered positions in each of chunks 0, 1 and 2, five images below T (in chunks 1 and 3), the rest above."""
    rng = np.random.default_rng(seed)
    img = _losers(rng, SPREAD_COLS, CUT_T)
    for c in range(3):
        img[_chunk_positions(rng, SPREAD_COLS, c, 10)] = CUT_T
    free = np.flatnonzero(img != CUT_T)
    free = free[((free >= CH) & (free < 2 * CH)) | (free >= 3 * CH)]
    img[rng.choice(free, CUT_BELOW, replace=False)] = np.uint64(CUT_T) - 1 - rng.permutation(CUT_BELOW).astype(np.uint64)
    return img


def level1_images(r, seed=29):
    """1000 copies of T scattered over chunks 0-7 and 50 over chunks 8-9, the rest above T: at k = 1024 the last 24 winners
    are ties of the second level-1 chunk, ordered there by candidate position with carried columns."""
    rng = np.random.default_rng([seed, r])
    img = _losers(rng, L1_COLS, CUT_T)
    img[rng.choice(8 * CH, 1000, replace=False)] = CUT_T
    img[8 * CH + rng.choice(2 * CH, 50, replace=False)] = CUT_T
    return img


def level1_matrix(kt, desc):
    return np.stack([_keys(level1_images(r), kt, desc) for r in range(L1_ROWS)])


# --------------------------------------------------------------------------------------------- 7. many rows --
MANY_ROWS = [(100003, 7, 3, 1, 1), (600, 1025, 3, 2, 1), (97, 2 * CH + 1, 5, 3, 2)]       # (rows, cols, k, path, levels)


def many_rows_matrix(rows, cols, kt, desc, seed=31):
    """Every row from a seed of its own (a 64-bit mix of the row's seed and the column, so 100003 rows cost one numpy
    expression); every third row keeps two bits of its images, so that ties decide most of its k."""
    s = (np.arange(rows, dtype=np.uint64) + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)
    z = s[:, None] + (np.arange(cols, dtype=np.uint64) + np.uint64(1)) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    img = ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)
    img[::3] &= np.uint32(3)
    return R.preimage(img, kt, desc)


# ----------------------------------------------------------------------------------------------- 8. campaign --
CAMPAIGN_SEEDS = (31337, 31338)
CAMPAIGN_CASES = 40
CAMPAIGN_PARTS = 4
CAMPAIGN_ANCHORS = (64, 256, 512, 1024, 1025, CH, CH + 1, 2 * CH, 65537)
CAMPAIGN_GAPS = (0, 1, 3, 17)
CAMPAIGN_DISTS = tuple(T.DISTS) + ("digits",)


def campaign_case(seed, index):
    """Case `index` of campaign `seed`: (description, matrix [rows, stride], cols, key type, descending, kinds, rng for the k values)."""
    rng = np.random.default_rng([seed, index])
    cols = max(1, int(rng.choice(CAMPAIGN_ANCHORS)) + int(rng.integers(-40, 41)))
    rows = int(rng.integers(1, 10))
    stride = cols + int(rng.choice(CAMPAIGN_GAPS))
    kt, desc = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
    mat = np.zeros((rows, stride), np.uint32)
    kinds = []
    for r in range(rows):
        kind = CAMPAIGN_DISTS[int(rng.integers(0, len(CAMPAIGN_DISTS)))]
        s = int(rng.integers(0, 1 << 20))
        if kind == "digits":
            variant = "a" if cols <= DIGIT_BASE else ("b", "c")[int(rng.integers(0, 2))]
            mat[r, :cols] = _keys(digit_images(cols, variant, s), kt, desc)
        else:
            mat[r, :cols] = T.gen(kind, cols, seed=s, kt=kt)
        kinds.append(kind)
    mat[:, cols:] = np.array([0, 0xFFFFFFFF], np.uint32)[(np.arange(stride - cols) + index) % 2]
    what = "seed=%d case=%d rows=%d cols=%d stride=%d kt=%d desc=%d %s" % (seed, index, rows, cols, stride, kt, desc, ",".join(kinds))
    return what, mat, cols, kt, desc, kinds, rng


def campaign_ks(ref0, cols, rng):
    """[(k, form)]: two cuts around tie runs of row 0, clipped to min(cols, 1024), and two random k."""
    lim = min(cols, 1024)
    cuts = T.run_cuts(ref0)
    ks = [min(lim, int(cuts[int(rng.integers(0, len(cuts)))])) for _ in range(2)] + [int(rng.integers(1, lim + 1)) for _ in range(2)]
    return [(k, MODES[int(rng.integers(0, 3))]) for k in ks]


# ---------------------------------------------------------------------------------------------- 9. front end --
FRONT_SHAPES = [(5, 300), (1, 5000), (4, 1)]


def front_ks(cols):
    return sorted({1, min(cols, 7), min(cols, 300)})


def distinct_int32(rows, cols, seed):
    """Tie-free rows of both signs."""
    rng = np.random.default_rng(seed)
    return np.stack([(rng.permutation(cols) - cols // 3).astype(np.int32) * np.int32(7919) for _ in range(rows)])
