"""The wide LSB pass -- wide_upsweep_kernel, the spine scan, wide_downsweep_kernel (gs_wide.hip, gs_wide_tile.inc) -- and the sorts
made of it (gs_lsb_sort_wide, the 64-bit branch of gs_lsb_sort_any) restated in numpy, with the case tables and input builders of
tests/test_wide_stages_gpu.py and the "plausible wrong kernels" that tests/test_wide_stages_cpu.py holds those tables against.
No GPU, no torch.

Keys are uint32 or uint64 bit patterns.  A key's IMAGE is the unsigned word whose order is the key order (include/gpusort.h):
float keys get the sign bit flipped if positive and all bits if negative, signed keys the sign bit flipped, and a descending
sort complements the lot.  The digit of a pass is a bit field of the image.  Between the first and the last pass of a sort the
buffers hold images, not keys."""
import functools

import numpy as np

from lsb_stages_ref import scan          # row-exclusive scan of a [256][grid] spine in 64 bits, every total asserted < 2^32

U32, I32, F32, U64, I64, F64 = 0, 1, 2, 3, 4, 5          # GS_KEY_*
KT_NAME = {U32: "U32", I32: "I32", F32: "F32", U64: "U64", I64: "I64", F64: "F64"}
U, I, F = 0, 1, 2
RADIX, WAVE = 256, 64


def width(kt):
    return 32 if kt < U64 else 64


def kind(kt):
    return kt % 3


def utype(w):
    return np.uint32 if w == 32 else np.uint64


def types_of_width(w):
    return (U32, I32, F32) if w == 32 else (U64, I64, F64)


# ------------------------------------------------------------------------------------------------- key images --
def xor_mask(kt, descending, model=()):
    """wide_sort's sign ^ flip: the sign bit of a signed type, all ones for a descending sort."""
    w = width(kt)
    m = ((1 << (w - 1)) if kind(kt) == I else 0) ^ (((1 << w) - 1) if descending else 0)
    if "xor_low_word" in model and w == 64:
        m &= 0xFFFFFFFF
    return utype(w)(m)


def twiddle_in(keys, kt, descending, model=()):
    """w_twiddle_in with f_in / xor_in of a first pass."""
    w = width(kt)
    dt = utype(w)
    k = np.ascontiguousarray(keys, dtype=dt)
    sign, ones = dt(1 << (w - 1)), dt((1 << w) - 1)
    if kind(kt) == F:
        k = k ^ np.where(k & sign != 0, ones, sign)
    return k ^ xor_mask(kt, descending, model)


def twiddle_out(img, kt, descending, model=()):
    """w_twiddle_out with f_out / xor_out of a last pass: the inverse of twiddle_in."""
    w = width(kt)
    dt = utype(w)
    k = np.ascontiguousarray(img, dtype=dt) ^ xor_mask(kt, descending, model)
    sign, ones = dt(1 << (w - 1)), dt((1 << w) - 1)
    if kind(kt) == F:
        if "out_no_complement" in model and w == 64:
            k = k ^ np.where(k & sign != 0, ones, sign)
        else:
            k = k ^ np.where(k & sign != 0, sign, ones)
    return k


def digit_of_image(img, shift, bits, model=()):
    dt = img.dtype.type
    return ((img >> dt(shift)) & dt(0xFF if "mask8" in model else (1 << bits) - 1)).astype(np.uint8)


def _read(stored, kt, desc, first, model):
    return twiddle_in(stored, kt, desc, model) if first else np.ascontiguousarray(stored, dtype=utype(width(kt)))


def _write(img, kt, desc, last, model):
    if last:
        return twiddle_out(img, kt, desc, model)
    if "f_out_every_pass" in model and kind(kt) == F:
        return twiddle_out(img, kt, 0, model)          # f_out without xor_out
    return img


# ---------------------------------------------------------------------------------------------------- geometry --
# gs_wide.hip: W_TILE, W_CHUNK, w_tiles, w_grid, w_spine_bytes, w_totals_bytes, w_prefix_bytes; the slack and the rounding of
# d_temp are gs_host.hpp's GS_WS_SLACK and gs_ws_base.  This is the pass's INTERNAL layout, the one wide_totals_ptr depends on.
TILE, CHUNK_TILES, WS_ALIGN = 4096, 8, 256
CHUNK = TILE * CHUNK_TILES


def _align(x):
    return (x + WS_ALIGN - 1) & ~(WS_ALIGN - 1)


def num_tiles(n):
    return (n + TILE - 1) // TILE


def grid_of(n):
    return max(1, (num_tiles(n) + CHUNK_TILES - 1) // CHUNK_TILES)


def layout(n):
    """(spine offset, totals offset, prefix16 offset, bytes) from the workspace pointer rounded up to 256: spine u32[256][grid],
    totals u32[256], prefix16 u16[tiles][256], each rounded up to 256 bytes."""
    spine = _align(RADIX * grid_of(n) * 4)
    totals = _align(RADIX * 4)
    prefix = _align(max(1, num_tiles(n)) * RADIX * 2)
    return 0, spine, spine + totals, spine + totals + prefix


def temp_bytes(n):
    return layout(n)[3] + WS_ALIGN


GROUP, XCDS = 512, 8


def tile_of_item(items, tiles):
    """gs_lsb.hpp tile_of_item: whole groups of 512 blocks take (r % 8) * 64 + r / 8 inside the group; the ragged last group is
    the identity."""
    i = np.asarray(items, dtype=np.int64)
    base = (i // GROUP) * GROUP
    r = i - base
    return np.where(base + GROUP > tiles, i, base + (r % XCDS) * (GROUP // XCDS) + r // XCDS)


# ---------------------------------------------------------------------------------------------------- one pass --
def tile_counts(dig):
    """[tile][d]: how many keys of the tile have digit d."""
    n = dig.size
    t = np.arange(n, dtype=np.int64) // TILE
    return np.bincount(t * RADIX + dig.astype(np.int64), minlength=num_tiles(n) * RADIX).reshape(num_tiles(n), RADIX)


def products(dig, prefix_span=CHUNK_TILES):
    """What a pass leaves in the workspace: the spine as the upsweep wrote it (u32[256][grid]: the chunk's count of d), the spine
    after the scan (row-exclusive), the totals, and prefix16[tile][d] (the count of d in the chunk's earlier tiles).
    prefix_span = 16 is a wrong-kernel model."""
    counts = tile_counts(dig)
    tiles, g = counts.shape[0], max(1, (counts.shape[0] + CHUNK_TILES - 1) // CHUNK_TILES)
    g2 = (g * CHUNK_TILES + prefix_span - 1) // prefix_span
    padded = np.zeros((g2 * prefix_span, RADIX), dtype=np.int64)
    padded[:tiles] = counts
    per = padded.reshape(g2, prefix_span, RADIX)
    before = (np.cumsum(per, axis=1) - per).reshape(g2 * prefix_span, RADIX)[:tiles]
    assert before.max(initial=0) < 1 << 16
    raw = np.ascontiguousarray(padded[:g * CHUNK_TILES].reshape(g, CHUNK_TILES, RADIX).sum(axis=1).T).astype(np.uint32)
    rows, totals = scan(raw)
    return {"counts": counts, "spine_raw": raw, "spine": rows, "totals": totals, "prefix16": before.astype(np.uint16)}


def pass_ref(stored, vals, kt, desc, shift, bits, first=True, last=True, model=()):
    """One pass as its definition: the stable scatter of keys and values on the digit at (shift, bits) of the image; keys are read
    through the in-twiddle on a first pass and leave through the out-twiddle on a last one.  -> (keys, values, products)."""
    img = _read(stored, kt, desc, first, model)
    dig = digit_of_image(img, shift, bits, model)
    if "desc_as_reversed" in model and desc and first:
        asc = _read(stored, kt, 0, first, model)
        perm = np.argsort(digit_of_image(asc, shift, bits, model), kind="stable")[::-1]
    else:
        perm = np.argsort(dig, kind="stable")
    out = _write(img[perm], kt, desc, last, model)
    return out, (None if vals is None else np.ascontiguousarray(vals)[perm]), products(dig)


def num_passes(begin, end):
    return (end - begin + 7) // 8


def sort_ref(keys, vals, kt, desc, begin, end, selector=0, model=()):
    """gs_lsb_sort_wide as a composition of passes -> (keys, values, selector).  The selector flips once per pass: it is
    unchanged for begin == end and for no keys."""
    k, v = np.ascontiguousarray(keys, dtype=utype(width(kt))), vals
    passes = num_passes(begin, end) if k.size else 0
    for p in range(passes):
        shift = begin + 8 * p
        k, v, _ = pass_ref(k, v, kt, desc, shift, min(8, end - shift), p == 0, p == passes - 1, model)
    return k, v, selector ^ (passes & 1)


def stable_order(keys, kt, desc, begin, end):
    """The permutation of a stable sort on bits [begin, end) of the image (gs_lsb_sort_any's contract)."""
    img = twiddle_in(keys, kt, desc)
    if begin == end:
        return np.arange(img.size)
    dt = img.dtype.type
    field = (img >> dt(begin)) & dt((1 << (end - begin)) - 1)
    return np.argsort(field, kind="stable")


SIM_MODELS = ("pads_first", "reverse_in_wave", "prefix16_every_16", "value_slot_swap", "valid_from_block")


def simulate_pass(stored, vals, kt, desc, shift, bits, first=True, last=True, model=()):
    """The downsweep the way the kernel does it, tile by tile: clamped loads, pads of the all-ones image behind the valid keys,
    ranks in (digit, slot) order, the staging buffer, destination = digit start + scanned spine + prefix16 - the tile's own
    exclusive digit count + slot, stores guarded by slot < valid.  -> (dst, keys, values) of every store, in store order; dst is
    int64 and a wrong model may leave [0, n) or repeat a destination, so nothing is scattered here (see `scattered`).
    model: any of SIM_MODELS, and the key-level models of twiddle_in / twiddle_out / digit_of_image."""
    dt = utype(width(kt))
    n, T = stored.size, num_tiles(stored.size)
    real_img = _read(stored, kt, desc, first, model)
    prod = products(digit_of_image(real_img, shift, bits, model), 16 if "prefix16_every_16" in model else CHUNK_TILES)
    j = np.arange(T * TILE, dtype=np.int64)
    t, s = j // TILE, j % TILE
    tile = np.arange(T, dtype=np.int64)
    valid = np.minimum(TILE, n - tile * TILE)
    if "valid_from_block" in model:         # the block that runs tile t is the one tile_of_item maps to it
        block = np.empty(T, dtype=np.int64)
        block[tile_of_item(tile, T)] = tile
        valid = np.minimum(TILE, n - block * TILE)
    real = s < valid[t]
    src = np.minimum(np.where(real, j, t * TILE + valid[t] - 1), n - 1)
    img = real_img[src]
    img[~real] = dt((1 << width(kt)) - 1)
    d = digit_of_image(img, shift, bits, model).astype(np.int64)
    sub = (s // WAVE) * WAVE + (WAVE - 1 - s % WAVE) if "reverse_in_wave" in model else s
    key = ((d * 2 + real) if "pads_first" in model else d) * TILE + sub
    order = np.argsort(key.reshape(T, TILE), axis=1, kind="stable")
    pos = np.empty((T, TILE), dtype=np.int64)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(TILE), (T, TILE)), axis=1)
    stage_k = np.empty((T, TILE), dtype=dt)
    np.put_along_axis(stage_k, pos, img.reshape(T, TILE), axis=1)
    sd = digit_of_image(stage_k, shift, bits, model).astype(np.int64)
    staged_counts = np.bincount((t * RADIX + sd.reshape(-1)), minlength=T * RADIX).reshape(T, RADIX)
    tile_excl = np.cumsum(staged_counts, axis=1) - staged_counts
    totals = prod["totals"].astype(np.int64)
    dstart = np.cumsum(totals) - totals
    gbase = dstart[None, :] + prod["spine"].astype(np.int64).T[tile // CHUNK_TILES] + prod["prefix16"].astype(np.int64) - tile_excl
    slot = np.broadcast_to(np.arange(TILE), (T, TILE))
    dst = np.take_along_axis(gbase, sd, axis=1) + slot
    written = slot < valid[:, None]
    out_k = _write(stage_k[written], kt, desc, last, model)
    out_v = None
    if vals is not None:
        pos_v = pos
        if "value_slot_swap" in model:      # the value of key slot i goes where key slot 7 - i went
            w_, i_, l_ = s // (WAVE * 8), (s // WAVE) % 8, s % WAVE
            pos_v = pos.reshape(-1)[t * TILE + w_ * (WAVE * 8) + (7 - i_) * WAVE + l_].reshape(T, TILE)
        stage_v = np.empty((T, TILE), dtype=vals.dtype)
        np.put_along_axis(stage_v, pos_v, np.ascontiguousarray(vals)[src].reshape(T, TILE), axis=1)
        out_v = stage_v[written]
    return dst[written], out_k, out_v


def scattered(dst, k, v, n):
    """The output arrays of a simulated pass whose stores are a permutation of [0, n)."""
    assert dst.size == n and np.array_equal(np.sort(dst), np.arange(n))
    out_k = np.empty(n, dtype=k.dtype)
    out_k[dst] = k
    out_v = None
    if v is not None:
        out_v = np.empty(n, dtype=v.dtype)
        out_v[dst] = v
    return out_k, out_v


def model_differs(stored, vals, kt, desc, shift, bits, model, first=True, last=True):
    """Whether a pass under the wrong-kernel model leaves other bytes than the reference (or stores somewhere else)."""
    if any(m in SIM_MODELS for m in model):
        a, b = simulate_pass(stored, vals, kt, desc, shift, bits, first, last, model), simulate_pass(stored, vals, kt, desc, shift, bits, first, last)
        ka, kb = np.argsort(a[0], kind="stable"), np.argsort(b[0], kind="stable")
        return any(x is not None and not np.array_equal(x[ka], y[kb]) for x, y in zip(a, b))
    a, b = pass_ref(stored, vals, kt, desc, shift, bits, first, last, model), pass_ref(stored, vals, kt, desc, shift, bits, first, last)
    return not np.array_equal(a[0], b[0]) or (vals is not None and not np.array_equal(a[1], b[1])) or \
        any(not np.array_equal(a[2][f], b[2][f]) for f in ("spine", "totals", "prefix16"))


# ---------------------------------------------------------------------------------------------- input builders --
INPUTS = ("uniform", "equal", "two_by_key", "two_by_tile", "every", "sorted", "reverse", "hot_but_one")


def digits_of(name, n, bits, rng):
    """The digit of every key of input `name` (int64, below 2^bits)."""
    D = 1 << bits
    i = np.arange(n, dtype=np.int64)
    d0, lo, hi = (2 * D) // 3, D // 3, D - 1
    uni = rng.integers(0, D, n, dtype=np.int64)
    if name in ("uniform", "ones_image_tail"):
        return uni
    if name == "equal":                 # prefix16 up to 7 * 4096 from nine tiles on
        return np.full(n, d0)
    if name == "two_by_key":
        return np.where(i & 1, hi, lo)
    if name == "two_by_tile":
        return np.where((i // TILE) & 1, hi, lo)
    if name == "every":
        return i % D
    if name == "sorted":
        return np.sort(uni)
    if name == "reverse":
        return np.sort(uni)[::-1]
    if name == "hot_but_one":           # every tile holds one digit and one stranger
        h = ((i // TILE) * 5 + 1) % D
        return np.where(i % TILE == 100 + (i // TILE) % 1000, (h + 1) % D, h)
    raise ValueError(name)


def ones_image_slots(n):
    """ones_image_tail: the whole partial last tile and every 61st slot before it."""
    i = np.arange(n, dtype=np.int64)
    return (i >= (n // TILE) * TILE) | (i % 61 == 7)


def _build_image(name, n, w, shift, bits, seed):
    dt = utype(w)
    rng = np.random.default_rng([seed, n, w, shift, bits, sum(map(ord, name))])
    field = dt(((1 << bits) - 1) << shift)
    noise = rng.integers(0, 1 << w, n, dtype=dt)
    img = (noise & ~field) | (digits_of(name, n, bits, rng).astype(dt) << dt(shift))
    if name == "ones_image_tail":
        img[ones_image_slots(n)] = dt((1 << w) - 1)
    img.setflags(write=False)
    return img


_build_image_kept = functools.lru_cache(maxsize=160)(_build_image)


def build_image(name, n, w, shift, bits, seed=0):
    """The keys' images (read-only): the digits of `name` in the field, random bits everywhere else."""
    return (_build_image_kept if n <= 1 << 20 else _build_image)(name, n, w, shift, bits, seed)


F64_SPECIALS = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,    # +-0, +-inf
                         0x0000000000000001, 0x8000000000000001,                                            # +- smallest subnormal
                         0x7FF8000000000000, 0xFFF8000000000000,                                            # +-NaN
                         0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,    # NaNs, distinct payloads
                         0x7FF8000012345678, 0xFFF4ABCDEF012345,
                         0x3FF8000000000000, 0xBFF8000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF], dtype=np.uint64)
F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7FC00000, 0xFFC00000,
                         0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFFA54321,
                         0x3FC00000, 0xBFC00000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32)


def specials(kt):
    assert kind(kt) == F
    return F32_SPECIALS if kt == F32 else F64_SPECIALS


def build_keys(name, n, kt, desc, shift=0, bits=8, seed=0):
    """Keys of type kt whose digit at (shift, bits), in the given direction, follows input `name`.
    `special` (float types): two keys in three are one of the special values, the third is random bits.
    `uniform_and`: random bits ANDed three times (about an eighth of the bits set), the entropy reduction of the parity tests."""
    w = width(kt)
    dt = utype(w)
    if name == "special":
        rng = np.random.default_rng([seed, n, kt, 31])
        sp = specials(kt)
        keys = rng.integers(0, 1 << w, n, dtype=dt)
        pick = rng.integers(0, 3, n) != 0
        keys[pick] = sp[rng.integers(0, sp.size, n)][pick]
        if n >= sp.size:                # every special value at least once
            keys[rng.permutation(n)[:sp.size]] = sp
        return keys
    if name == "uniform_and":
        rng = np.random.default_rng([seed, n, kt, 32])
        keys = rng.integers(0, 1 << w, n, dtype=dt)
        for _ in range(2):
            keys &= rng.integers(0, 1 << w, n, dtype=dt)
        return keys
    return twiddle_out(build_image(name, n, w, shift, bits, seed), kt, desc)


def enumerated(n, vb):
    """Values enumerated at the value's own width: every byte of the value is used."""
    i = np.arange(n, dtype=np.uint64)
    return i.astype(np.uint32) * np.uint32(0x9E3779B1) if vb == 4 else i * np.uint64(0x9E3779B97F4A7C15)


# ------------------------------------------------------------------------------------------------- case tables --
KV = ((8, 0), (8, 4), (8, 8), (4, 0), (4, 4), (4, 8))          # the six kernels of the entry's dispatch
ROWS = tuple((kb, vb, kt, desc) for kb, vb in KV for kt in types_of_width(8 * kb) for desc in (0, 1))
DIGITS = {64: ((0, 8), (24, 8), (32, 8), (56, 8), (63, 1), (61, 3), (0, 1), (29, 7), (57, 7)),
          32: ((0, 8), (24, 8), (31, 1), (29, 3), (5, 7))}
SIZES = (1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1, 9 * TILE, 16 * TILE + 1, 17 * TILE + 5)
TAIL_SIZES = (4097, TILE + 2049, 8 * TILE + 1, 17 * TILE + 5)     # (a tail of one key cannot tell a pad from it: see the CPU file)


def row_name(row):
    kb, vb, kt, desc = row
    return "k%d-v%d-%s-%s" % (8 * kb, 8 * vb, KT_NAME[kt], "desc" if desc else "asc")


def one_pass_calls(n, row):
    """(shift, bits, input) of the one-pass calls of a row at size n: every digit position of the key's width with every input
    (the full product: 72 calls for 64-bit keys, 40 for 32-bit keys, about half a millisecond each on the device)."""
    return [(s, b, name) for s, b in DIGITS[8 * row[0]] for name in INPUTS]


def tail_calls(n, row):
    """ones_image_tail at every digit position of the row's width."""
    return [(s, b, "ones_image_tail") for s, b in DIGITS[8 * row[0]]]


GROUP_TILES = (511, 512, 513, 1023, 1024, 1025)
GROUP_LAST = (TILE, 4091)
GROUP_ROWS = (((8, 8, F64, 1), (56, 8)), ((4, 8, I32, 0), (29, 3)))        # (row, its digit position)
GROUP_INPUTS = ("uniform", "two_by_tile")


def group_cases():
    """(tiles, elements of the last tile, row, shift, bits, input)"""
    return [(T, last, row, s, b, name) for T in GROUP_TILES for last in GROUP_LAST for row, (s, b) in GROUP_ROWS for name in GROUP_INPUTS]


SORT_RANGES = {64: ((0, 64), (1, 63), (31, 33), (40, 64), (20, 20)), 32: ((0, 32), (7, 24), (16, 16))}
SORT_SIZES = (1, 4097, 8 * TILE + 1, 100003)
SORT_TYPES = (U64, I64, F64, U32, I32, F32)


def sort_input(kt):
    return "special" if kind(kt) == F else "uniform_and"


def sort_calls(kt, desc, n):
    """(begin, end, starting selector, value bytes) of the whole sorts of one type, direction and size: every range with both
    selectors, with and without values; the value width alternates between the two the key width allows."""
    w = width(kt)
    out = []
    for ri, (begin, end) in enumerate(SORT_RANGES[w]):
        for sel in (0, 1):
            out.append((begin, end, sel, 0))
            out.append((begin, end, sel, (4, 8)[(ri + sel + desc + SORT_SIZES.index(n)) & 1]))
    return out


ANY_TYPES = (U64, I64, F64, U32, F32)
ANY_VALUE_BYTES = (0, 1, 2, 3, 12, 16, 24, 4096)
ANY_SIZES = (1, 4097, 40009)
ANY_RANGES = {64: ((0, 64), (9, 50), (33, 33)), 32: ((0, 32), (5, 22), (12, 12))}


def any_sizes(vb):
    return ANY_SIZES[:2] if vb == 4096 else ANY_SIZES
