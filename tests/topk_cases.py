"""Input builders of the top-k edge tests (tests/test_topk_edges_cpu.py, tests/test_topk_edges_gpu.py): plain numpy.

Every builder lays out IMAGES -- the order-preserving u32 words the kernels select on -- and returns the keys that have those
images for the given key type and direction (topk_ref.preimage).  So the top-byte buckets, the tile layout and the k-th image
are the same whatever the type and direction, and test_topk_edges_cpu.py holds each case to its intent (route, bucket size,
cut) with the numpy reference alone, before a device sees it.  gen() and DISTS are the exception: the distributions of key
words that tests/test_topk_gpu.py and the rows tests mix across their inputs, kept here so that no builder imports a GPU file."""
import numpy as np

import topk_ref as R

U32, I32, F32 = R.U32, R.I32, R.F32
KEY_TYPES = (U32, I32, F32)
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
MODES = (KEYS, PAIRS, ARGS)
TILE, CHUNK_TILES = R.TILE, R.CHUNK
CHUNK = TILE * CHUNK_TILES          # 65536 elements: one workgroup of the upsweep, one column of the spine
MIN_CAND = 65536
SCAN_BATCH = 1024                   # tiles the scan kernel takes per iteration of its carry loop
SPINE_GROUP = 256                   # chunks per permuted group of the upsweep's block -> chunk map


def cap(n):
    """Capacity of the candidate list."""
    return max(MIN_CAND, n // 32)


def tiles(n):
    return max(1, -(-n // TILE))


def _u32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32))


def _low24(rng, count):
    return rng.integers(0, 1 << 24, count, dtype=np.uint64)


def _keys(img, key_type, descending):
    return R.preimage(_u32(img), key_type, descending)


# ------------------------------------------------------------------------------------ distributions of key words --
DISTS = ["uniform", "equal", "five", "topbyte", "top3", "zipf", "sorted", "reversed", "special"]


def gen(kind, n, seed=1, kt=U32):
    """n key words (not images) of distribution `kind`: what tests/test_topk_gpu.py and the rows tests mix across their inputs."""
    rng = np.random.default_rng(seed * 1000003 + n)
    if kind == "uniform":
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    elif kind == "equal":
        k = np.full(n, 0x3F800000, np.uint32)
    elif kind == "five":
        k = np.array([0x00000007, 0x3F800000, 0x3F800001, 0xBF800000, 0xFFFFFFF0], np.uint32)[rng.integers(0, 5, n)]
    elif kind == "topbyte":      # one top byte, random low bytes: rounds two to four do real work on the input itself
        k = (rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)) | np.uint32(0x42000000)
    elif kind == "top3":         # the top three bytes shared
        k = (rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32)) | np.uint32(0xC1A25500)
    elif kind == "zipf":
        k = (rng.zipf(1.3, size=n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(13)).astype(np.uint32)
    elif kind == "sorted":
        k = np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    elif kind == "reversed":
        k = np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))[::-1].copy()
    elif kind == "special":      # the special sets of test_lsb_large_gpu.py, mixed into random keys
        if kt == F32:
            tiny = np.finfo(np.float32).smallest_subnormal
            sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5, np.nan, -np.nan], np.float32).view(np.uint32)
            sp = np.concatenate([sp, np.array([0x7FC00001], np.uint32)])      # a NaN payload
        else:
            mx = np.uint32(0xFFFFFFFF)
            sp = np.array([0, 1, mx, mx - 1, mx >> 1, (mx >> 1) + 1], np.uint32)   # MIN, MAX, -1, 0 of the signed type
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        pick = rng.random(n) < 0.6
        k[pick] = sp[rng.integers(0, sp.size, int(pick.sum()))]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(k, dtype=np.uint32)


# ------------------------------------------------------------------------------------------- plain distributions --
def uniform_case(n, seed, key_type=U32, descending=False):
    return _keys(np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64), key_type, descending)


def topbyte_case(n, seed, key_type=U32, descending=False, top=0x42):
    """One top byte of the image, random low 24 bits: the bucket is the whole input."""
    return _keys(_low24(np.random.default_rng(seed), n) | np.uint64(top << 24), key_type, descending)


def equal_case(n, key_type=U32, descending=False, img=0x42A55A01):
    return _keys(np.full(n, img, np.uint64), key_type, descending)


def few_case(n, seed, key_type=U32, descending=False):
    rng = np.random.default_rng(seed)
    five = np.array(IMAGES20, np.uint64)[rng.choice(len(IMAGES20), 5, replace=False)]
    return _keys(five[rng.integers(0, 5, n)], key_type, descending)


def heavy_case(n, seed, key_type=U32, descending=False, img=0x80000000):
    """Uniform images, every second one replaced by one value: its bucket is past any capacity."""
    x = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64)
    x[::2] = img
    return _keys(x, key_type, descending)


# ---------------------------------------------------------------------------------------------- capacity boundary --
CAPACITY = [(100003, 65536), (2097215, 65537), (3000003, 93750)]     # (n, cap): the floor, n / 32 one above it, n / 32
CAP_BELOW, CAP_D0 = 20000, 0x42


def bucket_case(n, c, below, d0, seed, key_type=U32, descending=False):
    """`below` images under d0 << 24, exactly c with top byte d0, the rest above; shuffled."""
    assert 0 < d0 < 255 and below + c <= n
    rng = np.random.default_rng(seed)
    img = np.concatenate([rng.integers(0, d0 << 24, below, dtype=np.uint64),
                          _low24(rng, c) | np.uint64(d0 << 24),
                          rng.integers((d0 + 1) << 24, 1 << 32, n - below - c, dtype=np.uint64)])
    return _keys(img[rng.permutation(n)], key_type, descending)


def capacity_ks(below, c):
    """(k, inside the bucket): the last before the bucket, its first, middle and last, the first after it."""
    return [(below, False), (below + 1, True), (below + c // 2, True), (below + c, True), (below + c + 1, False)]


# ------------------------------------------------------------------------------------------------------ layout --
LAYER_D0, LAYER_LOW = 0x9C, 0x17
LAYER_SIZES = [22 * TILE + 4097, 24 * TILE, 24 * TILE + 77]         # 23, 24 and 25 tiles
# (n, bucket size, route of a k inside the bucket); the bucket past 65536 needs n >= 24 tiles behind the leading 15 tiles
LAYERED = [(n, 30000, 1) for n in LAYER_SIZES] + [(n, 66000, 2) for n in LAYER_SIZES[1:]]


def layered_case(n, c, seed, key_type=U32, descending=False, d0=LAYER_D0, low=LAYER_LOW):
    """The populations of bucket_case in whole tiles and chunks: chunk 0 is all of the digit `low` (< d0); chunk 1 is seven
    tiles of `low` and one tile of bucket elements, so that tile's prefix16[low] is 57344, the most a tile can have in front of
    it inside its chunk; the rest is shuffled: the other c - 8192 bucket elements, digits below d0 (0, low, d0 - 1 and random
    ones) and digits above.  Returns (keys, number of images below d0 << 24)."""
    m = n - 2 * CHUNK
    assert 0 < low < d0 < 255 and c >= TILE and m >= c - TILE
    rng = np.random.default_rng(seed)
    n_under = (m - (c - TILE)) // 2
    n_over = m - (c - TILE) - n_under
    under_digits = np.concatenate([np.array([0, low, d0 - 1], np.uint64), rng.integers(0, d0, 13, dtype=np.uint64)])
    mixed = np.concatenate([_low24(rng, c - TILE) | np.uint64(d0 << 24),
                            _low24(rng, n_under) | (under_digits[rng.integers(0, under_digits.size, n_under)] << np.uint64(24)),
                            rng.integers((d0 + 1) << 24, 1 << 32, n_over, dtype=np.uint64)])
    img = np.concatenate([_low24(rng, CHUNK + 7 * TILE) | np.uint64(low << 24),
                          _low24(rng, TILE) | np.uint64(d0 << 24),
                          mixed[rng.permutation(m)]])
    assert img.size == n
    return _keys(img, key_type, descending), CHUNK + 7 * TILE + n_under


def layered_ks(below, c):
    return [below + 1, below + c // 2, below + c]


# -------------------------------------------------------------------------------------------------- digit edges --
IMAGES20 = [0x00000000, 0x00000001, 0x000000FF, 0x00000100, 0x0000FF00, 0x0000FFFF, 0x00010000, 0x00FF0000, 0x00FFFFFF,
            0x01000000, 0x7FFFFFFF, 0x80000000, 0xFEFFFFFF, 0xFF000000, 0xFF0000FF, 0xFF00FF00, 0xFFFF0000, 0xFFFFFF00,
            0xFFFFFFFE, 0xFFFFFFFF]
# one run per image, lengths from 1, 2, 63, 64, 65, 8191, 8192, 8193: the top bytes 0x00 and 0xFF hold 32964 and 32898
RUNS20 = [8193, 1, 64, 8191, 2, 8192, 63, 65, 8193,
          8192, 8191, 8193, 1, 8192, 2, 8193, 63, 8191, 65, 8192]
DIGIT_EDGES = [(1, 0x00), (2, 0x00), (2, 0xFF)]                      # (route, top byte whose runs are scaled for route 2)


def digit_edge_runs(route, top=0x00):
    """[(image, run length)]: RUNS20, and for route 2 every run of a tile or so under the top byte `top` one tile longer
    (16383, 16384, 16385), which takes that byte's bucket past 65536."""
    assert route in (1, 2) and top in (0x00, 0xFF)
    return [(img, ln + TILE if route == 2 and img >> 24 == top and ln >= TILE - 1 else ln) for img, ln in zip(IMAGES20, RUNS20)]


def digit_edge_case(route, top=0x00, key_type=U32, descending=False, seed=5):
    runs = digit_edge_runs(route, top)
    img = np.repeat(np.array([i for i, _ in runs], np.uint64), [ln for _, ln in runs])
    return _keys(img[np.random.default_rng(seed).permutation(img.size)], key_type, descending)


def run_cuts(ref):
    """For every tie run of ref's sorted images, with cumulative end C: the k values C - 1, C and C + 1, clipped to [1, n]."""
    s = ref.sorted_img
    ends = np.append(np.flatnonzero(s[1:] != s[:-1]) + 1, s.size).astype(np.int64)
    ks = np.unique(np.clip(np.concatenate([ends - 1, ends, ends + 1]), 1, s.size))
    return [int(k) for k in ks]


# ------------------------------------------------------------------------------------------------- scan batches --
SCAN_SIZES = [1024 * TILE, 1024 * TILE + 1, 1025 * TILE + 5, 2049 * TILE + 77]      # 1024, 1025, 1026 and 2050 tiles
SPINE_K = 100000


def scan_equal_ks(n):
    ks = [1024 * TILE - 1, 1024 * TILE, 1024 * TILE + 1, 1024 * TILE + 8193, n]
    if n > 2048 * TILE + 1:
        ks += [2048 * TILE, 2048 * TILE + 1]
    return sorted({k for k in ks if k <= n})


def scan_random_ks(n):
    return [1, n // 2, n - 1]


# -------------------------------------------------------------------------------------------------- class edges --
CLASS_EDGES = [2048, 2049, 4608, 4609, 9216, 9217]                  # the local sort's classes: in n (route 3) or in k
CLASS_KS = CLASS_EDGES + [17408, 17409, 65536, 65537]
CLASS_N = 100003


# ----------------------------------------------------------------------------------------------------- campaign --
CAMPAIGN_SEEDS = (20250, 20251)
CAMPAIGN_CASES = 60
CAMPAIGN_ANCHORS = (17408, 65536, TILE * CHUNK_TILES, 100003, 300007)     # (one workgroup's capacity | the list's floor = a chunk)
CAMPAIGN_DISTS = ("uniform", "few", "topbyte", "layered", "heavy")


def campaign_case(seed, index):
    """Case `index` of campaign `seed`: (description, keys, key type, descending, rng for the k values)."""
    rng = np.random.default_rng([seed, index])
    dist = CAMPAIGN_DISTS[int(rng.integers(0, len(CAMPAIGN_DISTS)))]
    anchor = 300007 if dist == "layered" else int(rng.choice(CAMPAIGN_ANCHORS))       # (layered needs its two leading chunks)
    n = anchor + int(rng.integers(-40, 41))
    kt, desc = int(rng.integers(0, 3)), bool(rng.integers(0, 2))
    s = int(rng.integers(0, 1 << 30))
    if dist == "uniform":
        keys = uniform_case(n, s, kt, desc)
    elif dist == "few":
        keys = few_case(n, s, kt, desc)
    elif dist == "topbyte":
        keys = topbyte_case(n, s, kt, desc, top=int(rng.integers(0, 256)))
    elif dist == "layered":
        keys, _ = layered_case(n, int(rng.choice([TILE, 30000, 65536, 65537, 90000])), s, kt, desc)
    else:
        keys = heavy_case(n, s, kt, desc, img=int(rng.choice(IMAGES20)))
    return "seed=%d case=%d %s n=%d kt=%d desc=%d" % (seed, index, dist, n, kt, desc), keys, kt, desc, rng


def campaign_ks(ref, rng):
    """[(k, form)]: two cuts around tie runs, two random k."""
    n = ref.keys.size
    cuts = run_cuts(ref)
    ks = [int(cuts[int(rng.integers(0, len(cuts)))]) for _ in range(2)] + [int(rng.integers(1, n + 1)) for _ in range(2)]
    return [(k, MODES[int(rng.integers(0, 3))]) for k in ks]
