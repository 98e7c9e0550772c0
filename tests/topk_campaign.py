"""The seeded campaign over all eleven top-k entry points (tests/test_topk_campaign_cpu.py, tests/test_topk_campaign_gpu.py):
plain numpy, no torch, no library, and none of the per-entry-point reference modules.

One sentence of include/gpusort.h defines every entry point: the first k of the stable sort on the key type's order-preserving
image, lowest index first inside a run of equal keys.  This module states it once:

  image(bits, key_type, descending)   the image map of all ten key types, generic in the width;
  case(family, seed, index)           a pure function: shape, key type, direction, form, distribution, k, stride, offsets
                                      and the element offset of every key array inside its allocation;
  reference(case)                     np.argsort(image(sub), kind="stable")[:kept] of every row or clamped segment, and
                                      the k-th image, `less` and `take` of the status calls;
  layout(case, temp_bytes)            the buffers of one call, for guarded.Arena on the device and HostArena here;
  check(case, snapshot, ref)          keys, values, counts, the pre-fill behind kept, the inputs and the guard bands, bit
                                      for bit; returns a description of the first difference, or None.

A family is named by its C entry point.  The (key type, direction, form) triple is rotated by the index and the shape kind by
the index modulo a number coprime to the rotation's period, so the floors that test_topk_campaign_cpu.py counts hold by
construction; everything else is drawn from np.random.default_rng([family, seed, index])."""
import numpy as np

# GS_KEY_* of include/gpusort.h
U32, I32, F32, U64, I64, F64, U16, I16, F16, BF16 = 0, 1, 2, 3, 4, 5, 8, 9, 10, 11
KEY_NAMES = {U32: "U32", I32: "I32", F32: "F32", U64: "U64", I64: "I64", F64: "F64",
             U16: "U16", I16: "I16", F16: "F16", BF16: "BF16"}
WIDTH = {U16: 16, I16: 16, F16: 16, BF16: 16, U32: 32, I32: 32, F32: 32, U64: 64, I64: 64, F64: 64}
UINT = {16: np.uint16, 32: np.uint32, 64: np.uint64}
SIGNED = (I16, I32, I64)
FLOATS = (F16, BF16, F32, F64)
EXP_BITS = {F16: 5, BF16: 8, F32: 8, F64: 11}
TYPES = {16: (U16, I16, F16, BF16), 32: (U32, I32, F32), 64: (U64, I64, F64)}
WIDEN = {U16: U32, I16: I32, F16: F32, BF16: F32, U32: U64, I32: I64, F32: F64}
NARROW32 = {U64: U32, I64: I32, F64: F32}          # the 32-bit type whose patterns, shifted left by 32, the header speaks of
NARROW16 = {U32: U16, I32: I16, F32: BF16}
KEYS, PAIRS, ARGS = "keys", "pairs", "args"
FORMS = (KEYS, PAIRS, ARGS)
FLAT, ROWS, ANYK, SEG = "flat", "rows", "anyk", "segmented"
CH = 8192                  # the elements one workgroup selects from (rows, any-k, segmented)
MAX_K = 1024               # gs_topk_rows_max_k()
MIN_CAND = 65536           # the floor of the flat candidate list
SMALL = {32: 17408, 16: 8192}      # flat arrays that one workgroup sorts whole (route 3); the 64-bit call has no route 3

# family -> (shape, key width, size query, status call or None)
FAMILIES = {
    "gs_topk_u32": (FLAT, 32, "gs_topk_temp_bytes", "gs_topk_status"),
    "gs_topk_u16": (FLAT, 16, "gs_topk_u16_temp_bytes", "gs_topk_u16_status"),
    "gs_topk_u64": (FLAT, 64, "gs_topk_u64_temp_bytes", "gs_topk_u64_status"),
    "gs_topk_rows_u32": (ROWS, 32, "gs_topk_rows_temp_bytes", None),
    "gs_topk_rows_u16": (ROWS, 16, "gs_topk_rows_u16_temp_bytes", None),
    "gs_topk_rows_u64": (ROWS, 64, "gs_topk_rows_u64_temp_bytes", None),
    "gs_topk_rows_anyk_u32": (ANYK, 32, "gs_topk_rows_anyk_temp_bytes", "gs_topk_rows_anyk_status"),
    "gs_topk_rows_anyk_u16": (ANYK, 16, "gs_topk_rows_anyk_u16_temp_bytes", "gs_topk_rows_anyk_u16_status"),
    "gs_topk_segmented_u32": (SEG, 32, "gs_topk_segmented_temp_bytes", "gs_topk_segmented_status"),
    "gs_topk_segmented_u16": (SEG, 16, "gs_topk_segmented_u16_temp_bytes", "gs_topk_segmented_status"),
    "gs_topk_segmented_u64": (SEG, 64, "gs_topk_segmented_u64_temp_bytes", "gs_topk_segmented_status"),
}
FAMILY_ORDER = tuple(FAMILIES)
FAMILY_OF = {(v[0], v[1]): f for f, v in FAMILIES.items()}
SEEDS = (1, 2)
CASES = 96                 # per (family, seed)


def cap(n):
    """Capacity of the flat candidate list."""
    return max(MIN_CAND, n // 32)


# ------------------------------------------------------------------------------------------------------ the image --
def image(bits, key_type, descending=False):
    """key_type's order-preserving unsigned image of the keys' bit patterns, at the key's own width: the sign bit flipped for
    the signed integers; for the float categories all bits flipped where the sign bit is set and the sign bit alone where it
    is clear; complemented when descending."""
    w = WIDTH[key_type]
    dt = UINT[w]
    k = np.ascontiguousarray(bits)
    assert k.dtype.itemsize * 8 == w, (k.dtype, key_type)
    k = k.view(dt)
    sign = dt(1 << (w - 1))
    if key_type in SIGNED:
        k = k ^ sign
    elif key_type in FLOATS:
        k = np.where((k & sign) != 0, ~k, k ^ sign)
    if descending:
        k = ~k
    return np.ascontiguousarray(k, dtype=dt)


def preimage(img, key_type, descending=False):
    """The inverse of image(): the bit patterns whose image is img."""
    w = WIDTH[key_type]
    dt = UINT[w]
    k = np.ascontiguousarray(img, dtype=dt)
    sign = dt(1 << (w - 1))
    if descending:
        k = ~k
    if key_type in SIGNED:
        k = k ^ sign
    elif key_type in FLOATS:
        k = np.where((k & sign) != 0, k ^ sign, ~k)         # the images of the non-negative floats have the top bit set
    return np.ascontiguousarray(k, dtype=dt)


# -------------------------------------------------------------------------------------------------- distributions --
DISTS = ("uniform", "few", "equal", "topbyte", "lowbyte", "heavy", "sorted", "reversed", "smallint", "deep", "widened",
         "specials", "mixed")
_PLAIN = DISTS[:-1]


def _rand(rng, n, bits):
    if bits <= 0:
        return np.zeros(n, np.uint64)
    return rng.integers(0, 1 << bits, n, dtype=np.uint64)


def images(rng, kind, n, w):
    """n images of `w` bits of distribution `kind`, as uint64."""
    if kind == "uniform":
        x = _rand(rng, n, w)
    elif kind == "few":                               # 2 to 9 distinct values
        d = int(rng.integers(2, 10))
        x = _rand(rng, d, w)[rng.integers(0, d, n)]
    elif kind == "equal":
        x = np.full(n, _rand(rng, 1, w)[0], np.uint64)
    elif kind == "topbyte":                           # one shared top byte: the first digit decides nothing
        x = (_rand(rng, 1, 8)[0] << np.uint64(w - 8)) | _rand(rng, n, w - 8)
    elif kind == "lowbyte":                           # all but the lowest byte shared
        x = (_rand(rng, 1, w)[0] & ~np.uint64(0xFF)) | _rand(rng, n, 8)
    elif kind == "heavy":                             # every second key one heavy value
        x = _rand(rng, n, w)
        x[::2] = _rand(rng, 1, w)[0]
    elif kind in ("sorted", "reversed"):
        x = np.sort(_rand(rng, n, w))
        if kind == "reversed":
            x = x[::-1].copy()
    elif kind == "smallint":                          # small integers; at 64 bits under constant upper bytes
        base = (_rand(rng, 1, 40)[0] << np.uint64(24)) if w == 64 else np.uint64(0)
        x = base | _rand(rng, n, 10)
    elif kind == "deep":                              # two values in each of several bytes, constant bytes between them
        two = lambda: rng.choice(256, 2, replace=False).astype(np.uint64)[rng.integers(0, 2, n)]
        if w == 64:
            x = (two() << np.uint64(56)) | (two() << np.uint64(40)) | (two() << np.uint64(16)) | _rand(rng, n, 16)
        elif w == 32:
            x = (two() << np.uint64(24)) | (two() << np.uint64(8)) | _rand(rng, n, 8)
        else:
            x = (two() << np.uint64(8)) | _rand(rng, n, 8)
    else:
        raise ValueError(kind)
    return x


def specials(key_type):
    """Bit patterns at the edges of key_type's order: NaNs of both signs with payloads, +-0, +-inf, denormals, +-1 for the
    floats; the extremes and the neighbours of the sign change for the integers."""
    w = WIDTH[key_type]
    if key_type in FLOATS:
        e = EXP_BITS[key_type]
        m = w - 1 - e
        sign, inf, quiet, mant = 1 << (w - 1), ((1 << e) - 1) << m, 1 << (m - 1), (1 << m) - 1
        one = ((1 << (e - 1)) - 1) << m
        pos = [0, 1, mant, one, inf, inf | 1, inf | quiet, inf | quiet | 5, inf | mant]
        sp = pos + [sign | p for p in pos]
    else:
        mx = (1 << w) - 1
        sp = [0, 1, 2, mx, mx - 1, mx >> 1, (mx >> 1) + 1, (mx >> 1) - 1, (mx >> 1) + 2]
    return np.array(sp, dtype=np.uint64).astype(UINT[w])


def make_keys(rng, kind, n, key_type, descending):
    """n key patterns of key_type.  The distributions are laid out on images and mapped back, so a shared top byte is shared
    whatever the type and direction; `widened` and `specials` are patterns of the keys themselves."""
    w = WIDTH[key_type]
    dt = UINT[w]
    if kind == "mixed":                               # blocks of different distributions
        out = np.empty(n, dt)
        at = 0
        while at < n:
            ln = min(n - at, int(rng.integers(1, max(2, n // 2 + 1))))
            out[at:at + ln] = make_keys(rng, _PLAIN[int(rng.integers(0, len(_PLAIN)))], ln, key_type, descending)
            at += ln
        return out
    if kind == "widened":                             # patterns of half the width, shifted up: they feed the equalities
        if w == 16:
            kind = "uniform"
        else:
            nt = NARROW32[key_type] if w == 64 else NARROW16[key_type]
            sub = ("uniform", "few", "topbyte", "heavy", "specials", "smallint")[int(rng.integers(0, 6))]
            return make_keys(rng, sub, n, nt, descending).astype(dt) << dt(w // 2)
    if kind == "specials":                            # six in ten elements
        keys = preimage(images(rng, "uniform", n, w).astype(dt), key_type, descending)
        sp = specials(key_type)
        pick = rng.random(n) < 0.6
        keys[pick] = sp[rng.integers(0, sp.size, int(pick.sum()))]
        return keys
    return preimage(images(rng, kind, n, w).astype(dt), key_type, descending)


# ------------------------------------------------------------------------------------------------------ the cases --
class Case:
    """One call.  keys: the whole key allocation's content behind its element offset (a matrix with its stride gaps);
    vals: the u32 values of the pairs form in the same layout, else None."""

    def name(self):
        return "(%s, %d, %d)" % (self.family, self.seed, self.index)

    def describe(self):
        d = "%s %s %s desc=%d %s dist=%s k=%d" % (self.name(), self.shape, KEY_NAMES[self.key_type], self.descending,
                                                 self.form, self.dist, self.k)
        if self.shape == FLAT:
            return d + " n=%d" % self.n
        if self.shape == SEG:
            return d + " num_items=%d segments=%d" % (self.n, self.S)
        return d + " rows=%d cols=%d stride=%d" % (self.rows, self.cols, self.stride)


def rotate(family, index):
    """(key type, descending, form) of case `index`: every triple comes round once in 6 * (number of types) cases."""
    types = TYPES[FAMILIES[family][1]]
    t = len(types)
    c = index % (6 * t)
    return types[c % t], bool((c // t) % 2), FORMS[(c // (2 * t)) % 3]


def _rng(family, seed, index, salt=0):
    return np.random.default_rng([FAMILY_ORDER.index(family), seed, index, salt])


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _around(rng, x):
    return x + int(rng.integers(-1, 2))


def _tie_k(rng, simg, mode):
    """A k at the first, middle or last position of a tie run of the sorted images simg: the run that holds a random rank,
    or (mode 'longest-*') the longest run."""
    n = simg.size
    starts = np.concatenate([[0], np.flatnonzero(simg[1:] != simg[:-1]) + 1, [n]])
    if mode.startswith("longest"):
        i = int(np.argmax(np.diff(starts)))
    else:
        i = int(np.searchsorted(starts, int(rng.integers(0, n)), side="right")) - 1
    lo, hi = int(starts[i]), int(starts[i + 1])
    if mode.endswith("first"):
        return lo + 1
    if mode.endswith("last"):
        return hi
    return lo + 1 + (hi - lo - 1) // 2


_TIE_MODES = ("tie-first", "tie-middle", "tie-last")


def _choose_k(rng, sub_keys, key_type, descending, kmax, fixed, longest=False):
    """k in [1, kmax]: one of `fixed`, a random one, or a position of a tie run of sub_keys (the flat array, or row 0)."""
    n = sub_keys.size
    mode = _pick(rng, ("fixed", "fixed", "random") + _TIE_MODES + _TIE_MODES)
    if longest:
        mode = "longest-" + _pick(rng, ("first", "middle", "last"))
    if mode == "fixed":
        k = _pick(rng, fixed)
    elif mode == "random":
        k = int(rng.integers(1, kmax + 1))
    else:
        k = _tie_k(rng, np.sort(image(sub_keys, key_type, descending)), mode)
    return max(1, min(int(k), kmax, n))


def _flat(c, rng):
    w = c.width
    kind = c.index % 11
    longest = False
    dist = _pick(rng, DISTS)
    if kind == 0:
        n = _pick(rng, (1, 2, 63, 64, 65))
    elif kind == 1:
        n = _around(rng, _pick(rng, (4096, 8192)))
    elif kind == 2:
        n = _around(rng, 17408)
    elif kind == 3:
        n = _around(rng, 65536)
    elif kind == 4:                                   # route 1: no bucket past the list
        n, dist = int(rng.integers(17410, 400001)), "uniform"
    elif kind == 5:                                   # a shared top byte longer than the list
        n, dist = int(rng.integers(70000, 400001)), "topbyte"
    elif kind == 6:                                   # a tie run longer than the list, and the cut inside it
        n, dist, longest = int(rng.integers(131200, 400001)), _pick(rng, ("heavy", "heavy", "equal")), True
    elif kind == 7:
        n = int(rng.integers(65538, 400001))
    elif kind == 8:                                   # three buckets past the list under each other (64-bit: D = 3)
        n, dist = int(rng.integers(290000, 400001)), "deep"
    elif kind == 9:
        n = int(rng.integers(3, 17408))
    else:
        n = int(rng.integers(8193, 17409))
    c.n, c.dist = n, dist
    c.keys = make_keys(rng, dist, n, c.key_type, c.descending)
    c.k = _choose_k(rng, c.keys, c.key_type, c.descending, n, (1, 2, n - 1, n), longest)
    c.alloc = n


ROW_COUNTS = (1, 2, 3, 64, 65, 97, 200, 333, 600)


def _matrix(c, rng, cols, kfun):
    """Rows, stride, keys with their gaps and k = kfun(row 0) for a matrix of `cols` columns."""
    stride = cols + _pick(rng, (0, 0, 1, 3, 17))
    budget = _pick(rng, (60000, 150000, 150000, 400000, 1500000))
    fit = [r for r in ROW_COUNTS if r * stride <= max(budget, stride)]
    rows = _pick(rng, fit) if c.max_rows is None else min(_pick(rng, fit), c.max_rows)
    dist = _pick(rng, DISTS)
    dt = UINT[c.width]
    alloc = (rows - 1) * stride + cols
    # the gap holds keys that would win if they were read: the pattern of image 0
    keys = np.full(alloc, preimage(np.zeros(1, dt), c.key_type, c.descending)[0], dt)
    for r in range(rows):
        kind = _PLAIN[int(rng.integers(0, len(_PLAIN)))] if dist == "mixed" else dist       # mixed: one per row
        keys[r * stride:r * stride + cols] = make_keys(rng, kind, cols, c.key_type, c.descending)
    c.rows, c.cols, c.stride, c.dist, c.keys, c.alloc = rows, cols, stride, dist, keys, alloc
    c.k = kfun(keys[:cols])


def _rows(c, rng):
    kind = c.index % 13
    c.max_rows = None
    force_k = None
    if kind == 0:
        cols = _pick(rng, (1, 2, 63, 64, 65))
    elif kind == 1:
        cols = _around(rng, _pick(rng, (256, 512)))
    elif kind == 2:
        cols = _around(rng, 1024)
    elif kind == 3:
        cols = int(rng.integers(2, 1025))
    elif kind == 4:
        cols = int(rng.integers(1026, 8191))
    elif kind == 5:
        cols = _around(rng, 8192)
    elif kind == 6:
        cols = _around(rng, 16384)
    elif kind == 7:
        cols = int(rng.integers(8194, 40001))
    elif kind == 8:                                   # three select levels: more than eight chunks at k = 1024
        cols, c.max_rows, force_k = int(rng.integers(65537, 80001)), 8, 1024
    elif kind == 9:
        cols = int(rng.integers(8194, 40001))
    elif kind == 10:
        cols, force_k = int(rng.integers(1025, 2049)), 1024
    elif kind == 11:                                  # cols = k
        cols = int(rng.integers(1, 1025))
        force_k = cols
    else:
        cols = int(rng.integers(1, 40001))
    kmax = min(cols, MAX_K)

    def kfun(row0):
        if force_k is not None:
            return force_k
        if kind == 9:
            return int(rng.integers(1, 9))
        return _choose_k(rng, row0, c.key_type, c.descending, kmax, (1, 2, kmax - 1, kmax))
    _matrix(c, rng, cols, kfun)


def _anyk(c, rng):
    kind = c.index % 11
    c.max_rows = None
    if kind == 0:
        cols = _pick(rng, (1, 2, 63, 64, 65))
    elif kind == 1:
        cols = _around(rng, _pick(rng, (256, 512, 1024)))
    elif kind == 2:
        cols = int(rng.integers(1026, 8191))
    elif kind == 3:
        cols = _around(rng, 8192)
    elif kind == 4:
        cols = _around(rng, 16384)
    elif kind == 5:                                   # path 2, one slab of four tiles
        cols = int(rng.integers(8194, 32768))
    elif kind == 6:
        cols = _around(rng, 32768)
    elif kind == 7:                                   # several slabs
        cols = int(rng.integers(32770, 80001))
    elif kind == 8:
        cols = _around(rng, 65536)
    elif kind == 9:
        cols = int(rng.integers(2, 4000))
    else:
        cols = _pick(rng, (79999, 80000, 40000))

    def kfun(row0):
        return _choose_k(rng, row0, c.key_type, c.descending, cols,
                         (1, 1024, 1025, 2047, 2048, 2049, cols - 1, cols))
    _matrix(c, rng, cols, kfun)


SEG_EDGES = (0, 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4000, 8191, 8192)
SEG_KS = (1, 7, 64, 100, 1023, 1024)


def _segmented(c, rng):
    kind = c.index % 7
    if kind == 0:
        n = _pick(rng, (1, 64, 65, 700, 1024))
    elif kind == 1:
        n = _pick(rng, (1025, 5000, 8191, 8192))
    elif kind == 2:
        n = int(rng.integers(8193, 30001))
    elif kind == 3:
        n = int(rng.integers(30000, 120001))
    elif kind == 4:
        n = int(rng.integers(200000, 400001))
    elif kind == 5:
        n = int(rng.integers(9000, 40001))
    else:
        n = int(rng.integers(8193, 400001))
    begin, end = [], []
    # the segments longer than CH: laid out one behind the other, so pairwise disjoint after the clamping too
    at = int(rng.integers(0, 4))
    first_long = True
    for _ in range(0 if kind == 5 else int(rng.integers(1, 4))):
        room = n - at
        if room <= CH:
            break
        ln = min(room, _pick(rng, (CH + 1, CH + 2, 2 * CH - 1, 2 * CH, 2 * CH + 1, int(rng.integers(CH + 1, 100001)),
                                   int(rng.integers(CH + 1, 100001)))))
        b, e = at, at + ln
        if first_long and b == 0 and rng.random() < 0.5:
            b = -int(rng.integers(1, 50))             # clamped to 0 on the device
        if e == n and rng.random() < 0.5:
            e = n + int(rng.integers(1, 50))          # clamped to num_items
        begin.append(b)
        end.append(e)
        first_long = False
        at += ln + int(rng.integers(0, 600))
    # the short ones: anywhere, overlapping freely
    for _ in range(int(rng.integers(150, 400)) if kind == 5 else int(rng.integers(3, 60))):
        ln = _pick(rng, SEG_EDGES) if rng.random() < 0.7 else int(rng.integers(1, CH + 1))
        ln = min(ln, n)
        b = int(rng.integers(0, n - ln + 1))
        e = b + ln
        how = rng.random()
        if ln == 0 and how < 0.5:
            e = b - int(rng.integers(1, 100))         # an end before the begin is empty as well
        elif ln > 0 and how < 0.1:                    # a negative begin: the clamped segment is [0, ln)
            b, e = -int(rng.integers(1, 50)), ln
        elif ln > 0 and how < 0.2:                    # an end past num_items: the clamped segment is [n - ln, n)
            b, e = n - ln, n + int(rng.integers(1, 50))
        begin.append(b)
        end.append(e)
    for _ in range(2):                                # repeats
        j = int(rng.integers(0, len(begin)))
        if end[j] - max(begin[j], 0) <= CH:
            begin.append(begin[j])
            end.append(end[j])
    perm = rng.permutation(len(begin))
    c.begin = np.array(begin, np.int32)[perm]
    c.end = np.array(end, np.int32)[perm]
    c.n, c.S, c.alloc = n, len(begin), n
    c.dist = _pick(rng, DISTS)
    c.keys = make_keys(rng, c.dist, n, c.key_type, c.descending)
    c.k = _pick(rng, SEG_KS)


def case(family, seed, index):
    """Case `index` of campaign `seed` for the entry point `family`: a pure function of its three arguments."""
    c = Case()
    c.family, c.seed, c.index = family, seed, index
    c.shape, c.width = FAMILIES[family][:2]
    c.key_type, c.descending, c.form = rotate(family, index)
    rng = _rng(family, seed, index)
    {FLAT: _flat, ROWS: _rows, ANYK: _anyk, SEG: _segmented}[c.shape](c, rng)
    c.vals = rng.integers(0, 1 << 32, c.alloc, dtype=np.uint64).astype(np.uint32) if c.form == PAIRS else None
    # 16- and 32-bit key arrays start 0 or 1 element into their allocation (a 16-bit array then sits at 2 mod 4); the
    # 64-bit ones stay 8-byte aligned
    c.key_in_off, c.key_out_off = (0, 0) if c.width == 64 else (int(rng.integers(0, 2)), int(rng.integers(0, 2)))
    return c


def clamp(c):
    """(b, len) of every segment after the device's clamping: b = max(begin, 0), e = min(end, num_items)."""
    b = np.maximum(c.begin.astype(np.int64), 0)
    e = np.minimum(c.end.astype(np.int64), c.n)
    return b, np.where(e > b, e - b, 0)


def subarrays(c):
    """(base, length) of every row or clamped segment inside c.keys."""
    if c.shape == FLAT:
        return np.zeros(1, np.int64), np.array([c.n], np.int64)
    if c.shape == SEG:
        return clamp(c)
    return np.arange(c.rows, dtype=np.int64) * c.stride, np.full(c.rows, c.cols, np.int64)


# -------------------------------------------------------------------------------------------------- the reference --
class Ref:
    """keys / vals: [S, k] in the key's dtype / u32; written: [S, k] bool, the slots the call must write; counts: [S];
    kth / less / take: per row or segment (kth 0 where kept is 0), as the header defines them for the status calls:
    the image of S[kept - 1], the elements whose image sorts strictly before it, kept - less; inside: the cut falls strictly
    inside a run of equal keys (the next element of the stable sort has the k-th image)."""


def reference(c):
    base, length = subarrays(c)
    S, k = base.size, c.k
    dt = UINT[c.width]
    img = image(c.keys, c.key_type, c.descending)
    r = Ref()
    r.keys, r.vals = np.zeros((S, k), dt), np.zeros((S, k), np.uint32)
    r.counts = np.minimum(length, k).astype(np.uint32)
    r.written = np.arange(k)[None, :] < r.counts[:, None]
    r.kth, r.less, r.take = np.zeros(S, dt), np.zeros(S, np.int64), np.zeros(S, np.int64)
    r.inside, r.top_share, r.run = np.zeros(S, bool), np.zeros(S, np.int64), np.zeros(S, np.int64)
    done = {}
    for s in range(S):
        kept, b, n = int(r.counts[s]), int(base[s]), int(length[s])
        if kept == 0:
            continue
        if (b, n) in done:                            # a repeated segment
            t = done[(b, n)]
            for a in (r.keys, r.vals, r.kth, r.less, r.take, r.inside, r.top_share, r.run):
                a[s] = a[t]
            continue
        done[(b, n)] = s
        sub = img[b:b + n]
        order = np.argsort(sub, kind="stable")[:kept]
        r.keys[s, :kept] = c.keys[b:b + n][order]
        r.vals[s, :kept] = order if c.vals is None else c.vals[b:b + n][order]
        kth = sub[order[-1]]
        r.kth[s] = kth
        r.less[s] = int(np.count_nonzero(sub < kth))
        r.take[s] = kept - r.less[s]
        r.run[s] = int(np.count_nonzero(sub == kth))
        r.inside[s] = r.take[s] < r.run[s]
        r.top_share[s] = int(np.count_nonzero((sub >> dt(c.width - 8)) == (kth >> dt(c.width - 8))))
    return r


def seg_lists(c):
    """The six list counts of gs_topk_segmented_status by clamped length (<= 64, 256, 512, 1024, CH, longer), and the chunk
    tasks of the long ones."""
    _, ln = clamp(c)
    edges = (0, 64, 256, 512, 1024, CH, 1 << 40)
    lists = [int(np.count_nonzero((ln > edges[i]) & (ln <= edges[i + 1]))) for i in range(6)]
    return lists, int(np.sum(-(-ln[ln > CH] // CH)))


def flat_route(c, r):
    """The route the header states for a flat case, from the reference's bucket and tie-run sizes against the list: (route, D)
    with D the counting rounds over the input of the 64-bit descent (1 for the other widths)."""
    n, C = c.n, cap(c.n)
    if c.width != 64:
        if n <= SMALL[c.width]:
            return 3, 1
        return (1 if int(r.top_share[0]) <= C else 2), 1
    img = image(c.keys, c.key_type, c.descending)
    kth = r.kth[0]
    M, j, D = img, 7, 0
    while True:
        D += 1
        shift = np.uint64(8 * j)
        bucket = M[(M >> shift) == (kth >> shift)]    # every byte above j is constant over M already
        if bucket.size <= C:
            return 1, D
        differ = int(np.bitwise_and.reduce(M) ^ np.bitwise_or.reduce(M))       # over this round's M, as the header has it
        lower = [b for b in range(j) if (differ >> (8 * b)) & 0xFF]
        if not lower:
            return 2, D
        j, M = max(lower), bucket


# ------------------------------------------------------------------------------------------- buffers and checking --
def prefill(c, name, nbytes):
    return _rng(c.family, c.seed, c.index, 1 + ("keys_out", "vals_out", "counts").index(name)).integers(
        0, 256, nbytes, dtype=np.uint8)


def layout(c, temp_bytes):
    """[(name, nbytes, byte offset past a 256-byte boundary, content as bytes, is an input)] of one call: inputs, pre-filled
    outputs, and a workspace of exactly temp_bytes bytes of 0xA5."""
    isz = c.width // 8
    S = subarrays(c)[0].size
    specs = [("keys_in", c.keys.view(np.uint8), c.key_in_off * isz, True)]
    if c.form == PAIRS:
        specs.append(("vals_in", c.vals.view(np.uint8), 4 * (c.index % 2), True))
    if c.shape == SEG:
        specs.append(("begin", c.begin.view(np.uint8), 0, True))
        specs.append(("end", c.end.view(np.uint8), 4, True))
    specs.append(("keys_out", prefill(c, "keys_out", S * c.k * isz), c.key_out_off * isz, False))
    if c.form != KEYS:
        specs.append(("vals_out", prefill(c, "vals_out", S * c.k * 4), 4 * ((c.index // 2) % 2), False))
    if c.shape == SEG:
        specs.append(("counts", prefill(c, "counts", S * 4), 0, False))
    specs.append(("temp", np.full(temp_bytes, 0xA5, np.uint8), 0, False))
    return [(name, data.size, off, data, const) for name, data, off, const in specs]


class HostArena:
    """guarded.Arena's slot layout in host memory, for the tests that run without a device: a guard band, the buffer at its
    offset past a 256-byte boundary, a guard band behind it.  snapshot() is what check() reads."""

    def __init__(self, specs, guard=512, seed=0x6A4D):
        self.slots, at = {}, 0
        for name, nbytes, off, _, _ in specs:
            start = at + guard + off
            end = (start + nbytes + guard + 255) & ~255
            self.slots[name] = (start, nbytes, at, end)
            at = end
        self.pattern = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
        self.mem = self.pattern.copy()
        for name, nbytes, _, data, _ in specs:
            start = self.slots[name][0]
            self.mem[start:start + nbytes] = data

    def view(self, name, dtype):
        start, nbytes = self.slots[name][:2]
        return self.mem[start:start + nbytes].view(dtype)

    def snapshot(self):
        return {"mem": self.mem, "pattern": self.pattern, "slots": self.slots}


def _buffer(snap, name, dtype):
    start, nbytes = snap["slots"][name][:2]
    return snap["mem"][start:start + nbytes].view(dtype)


def _first(diff):
    return int(np.flatnonzero(diff)[0])


def check(c, snap, r=None):
    """Everything one call must leave behind, bit for bit, against reference r: the first `kept` keys and values of every row
    or segment, the counts, the pre-fill in the slots [kept, k), the inputs, and every guard band of the arena.  snap is
    {"mem": the arena's bytes, "pattern": the guard pattern, "slots": name -> (start, nbytes, slot begin, slot end)}.
    -> None, or a description of the first difference."""
    r = reference(c) if r is None else r
    dt = UINT[c.width]
    S, k = r.counts.size, c.k
    who = "segment" if c.shape == SEG else "row"
    outs = [("keys", "keys_out", dt, r.keys)]
    if c.form != KEYS:
        outs.append(("values", "vals_out", np.uint32, r.vals))
    for what, name, t, want in outs:
        got = _buffer(snap, name, t).reshape(S, k)
        bad = (got != want) & r.written
        if bad.any():
            s, j = divmod(_first(bad.reshape(-1)), k)
            return "%s of %s %d (%d kept), slot %d: got 0x%x, expected 0x%x" % (what, who, s, r.counts[s], j, got[s, j], want[s, j])
    for what, name, t, want in outs:
        got = _buffer(snap, name, t).reshape(S, k)
        fill = prefill(c, name, got.nbytes).view(t).reshape(S, k)
        bad = (got != fill) & ~r.written
        if bad.any():
            s, j = divmod(_first(bad.reshape(-1)), k)
            return "%s of %s %d: slot %d behind the %d kept was written (0x%x over the pre-fill 0x%x)" % (
                what, who, s, j, r.counts[s], got[s, j], fill[s, j])
    if c.shape == SEG:
        got = _buffer(snap, "counts", np.uint32)
        bad = got != r.counts
        if bad.any():
            s = _first(bad)
            return "count of segment %d: got %d, expected %d" % (s, got[s], r.counts[s])
    ins = [("keys_in", c.keys)] + ([("vals_in", c.vals)] if c.form == PAIRS else [])
    if c.shape == SEG:
        ins += [("begin", c.begin), ("end", c.end)]
    for name, want in ins:
        got = _buffer(snap, name, want.dtype)
        bad = got != want
        if bad.any():
            i = _first(bad)
            return "input %s changed at element %d: 0x%x, was 0x%x" % (name, i, got[i], want[i])
    mem, pattern = snap["mem"], snap["pattern"]
    for name, (start, nbytes, lo, hi) in snap["slots"].items():
        for side, a, b in (("before", lo, start), ("behind", start + nbytes, hi)):
            bad = mem[a:b] != pattern[a:b]
            if bad.any():
                i = _first(bad)
                return "guard %s buffer %s changed: %d byte(s), the first %d byte(s) %s" % (
                    side, name, int(bad.sum()), start - (a + i) if side == "before" else i,
                    "before its start" if side == "before" else "past its end")
    return None


# ----------------------------------------------------------------------------------------------------- the census --
def census(c, r, lib):
    """What one case reaches, as a list of labels: the (key type, direction, form) triple, the path, levels, slabs and launch
    groups that the library's pure host plan functions report for its shape (lib: the loaded C library), the flat route and D
    from the reference's bucket and tie-run sizes, the segmented length classes, and whether a cut falls inside a tie run."""
    import ctypes
    out = (ctypes.c_uint32 * 8)()
    hv = int(c.form != KEYS)
    tags = ["triple %s %s %s" % (KEY_NAMES[c.key_type], "desc" if c.descending else "asc", c.form)]
    if c.shape == FLAT:
        route, D = flat_route(c, r)
        tags.append("route %d" % route)
        if c.width == 64:
            tags.append("D %d" % min(D, 3))
    elif c.shape == ROWS:
        assert lib.gs_topk_rows_plan(c.rows, c.cols, c.k, hv, out) == 0
        tags += ["path %d" % out[0], "levels %d" % out[1]]
    elif c.shape == ANYK:
        plan = lib.gs_topk_rows_anyk_plan if c.width == 32 else lib.gs_topk_rows_anyk_u16_plan
        assert plan(c.rows, c.cols, c.k, hv, out) == 0
        tags += ["path %d" % out[0], "k %s 1024" % ("<=" if c.k <= MAX_K else ">")]
        if out[0] == 2:
            tags.append("slabs %s" % ("1" if out[5] == 1 else "several"))
    else:
        assert lib.gs_topk_segmented_plan(c.n, c.S, c.k, hv, out) == 0
        tags.append("launch groups %d" % out[0])
        lists, _ = seg_lists(c)
        tags += ["class %d" % q for q in range(6) if lists[q]]
        _, ln = clamp(c)
        if (ln < c.k).any():
            tags.append("k above a segment")
        if ((c.begin < 0) | (c.end > c.n)).any():
            tags.append("clamped")
    if r.inside.any():
        tags.append("cut inside a tie run")
    return tags
