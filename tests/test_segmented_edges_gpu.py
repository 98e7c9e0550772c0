"""The segmented sorts at every path edge, odd layout and long segment: gs_segmented_sort_u32 and gs_segmented_sort_wide
(and gs_segmented_sort_narrow for the long segments) through the C ABI.

Every case runs in a guarded Arena (tests/guarded.py): keys and values one element off the 256-byte boundary, the workspace
1, 77 or 255 bytes off and exactly the queried size, the offsets arrays const, the alternate halves given explicit pre-fill
data (keys 0x3C bytes, values 0xC3 bytes) or one of the arena's fills, the starting selector 0 or 1 -- all rotating with
the call.  After the call: return code 0, every guard byte and const input intact, the selector sel0 ^ (passes & 1), keys and
values inside the segments bit-equal to the reference, and outside every segment BOTH halves of BOTH arrays byte for byte
what they held before.

Reference, in exact integers on the host: per clamped segment numpy's stable argsort of (ordmap(key) >> begin_bit) & mask,
complemented for descending (ordmap: the key type's order-preserving unsigned map of tests/test_buffer_contracts_gpu.py).
Values are the row indices at the value's width, so a stable sort's values are the reference permutation itself.  Second
witness: for full-width cases of 32- and 64-bit keys with at most 100 003 elements the oracle's reference ranks
(oracle.lsb_reference_ranks / lsb_reference_ranks_u64 on the order-preserving image), per segment, must be that permutation.

Nothing is sampled and nothing has a tolerance: every element inside and outside the segments is compared."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Arena, FILLS
from test_buffer_contracts_gpu import F32, F64, I32, I64, KEY_BYTES, U8, U16, U32, U64, UINT, gen_keys, ordmap

gpu = pytest.mark.gpu

# Path edges of gs_segmented_sort_u32: include/gpusort.h:285 (local-sort classes 2048 / 4608 / 9216 / 17408), :280 (tiles of 8192
# keys), :323 (segments of <= 17408 keys or pairs are one task; larger ones are buckets of the level)
U32_TILE, U32_CAP = 8192, 17408
# ... and of gs_segmented_sort_wide: include/gpusort.h:333 (segments of <= 8192 elements are one task), :359 (tile records per 4096
# elements: the geometry the narrow sort borrows from the wide one)
WIDE_TILE, WIDE_CAP = 4096, 8192
WITNESS_MAX = 100003
ALIGN_MIN_TILES = 256          # a bucket of this many tiles at an offset that is no multiple of 64 gets a short first tile (ws_first_tile)

ROWS = {"u32": [(U32, 0), (F32, 4), (I32, 4)],
        "wide": [(U64, 0), (I64, 4), (F64, 8), (U32, 8)],
        "narrow": [(U8, 0), (U16, 8)]}
GEOMETRY = {"u32": (U32_TILE, U32_CAP), "wide": (WIDE_TILE, WIDE_CAP)}
EDGE_SIZES = {
    "u32": [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025,          # wave lists
            2047, 2048, 2049, 4607, 4608, 4609,                                        # classes
            U32_TILE - 1, U32_TILE, U32_TILE + 1,                                      # tile
            9215, 9216, 9217,                                                          # class
            U32_CAP - 1, U32_CAP, U32_CAP + 1,                                         # cap
            2 * U32_CAP + 1, 3 * U32_TILE + 1],                                        # level path
    "wide": [1, 2, 63, 64, 65,                                                         # small
             2047, 2048, 2049,                                                         # class 2048
             WIDE_TILE - 1, WIDE_TILE, WIDE_TILE + 1,                                  # tile
             WIDE_CAP - 1, WIDE_CAP, WIDE_CAP + 1,                                     # cap
             2 * WIDE_CAP + 1, 3 * WIDE_TILE + 1],                                     # level path
}
RESIDUE_SIZES = {"u32": [40, 700, 3000, 9216, 17409], "wide": [40, 2048, 8192, 8193]}


def row_id(row):
    names = {U32: "u32", I32: "i32", F32: "f32", U64: "u64", I64: "i64", F64: "f64", U8: "u8", U16: "u16"}
    return "%s-v%d" % (names[row[0]], row[1])


ENTRY_ROWS = [pytest.param(e, r, id="%s-%s" % (e, row_id(r))) for e in ("u32", "wide") for r in ROWS[e]]
ENTRY_ROWS_ALL = ENTRY_ROWS + [pytest.param("narrow", r, id="narrow-" + row_id(r)) for r in ROWS["narrow"]]


# ------------------------------------------------------------------------------------------------------------ reference --
def passes_of(bb, eb):
    return (eb - bb + 7) // 8


def clamped(begins, ends, n):
    """the segments the device sorts: offsets clamped to [0, n], empty and inverted ones dropped"""
    b = np.maximum(np.asarray(begins, dtype=np.int64), 0)
    e = np.minimum(np.asarray(ends, dtype=np.int64), n)
    keep = e > b
    return list(zip(b[keep].tolist(), e[keep].tolist()))


class Spec:
    """what one call is asked to do"""

    def __init__(self, entry, kt, vb, keys, begins, ends, bb, eb, desc, sel0):
        self.entry, self.kt, self.vb, self.keys, self.bb, self.eb, self.desc, self.sel0 = entry, kt, vb, keys, bb, eb, bool(desc), sel0
        self.kb, self.n = KEY_BYTES[kt], keys.size
        assert keys.dtype == UINT[self.kb]
        self.vals = np.arange(self.n, dtype=UINT[vb]) if vb else None         # row indices: stability is visible
        self.segs = clamped(begins, ends, self.n)

    def __repr__(self):
        return "%s kt=%d vb=%d n=%d segs=%d bits=[%d,%d) desc=%d sel0=%d" % (self.entry, self.kt, self.vb, self.n, len(self.segs), self.bb,
                                                                              self.eb, self.desc, self.sel0)


def reference(spec):
    """perm[i] = input row that lands at position i (identity outside the segments), and the mask of covered positions"""
    width = spec.eb - spec.bb
    mask = np.uint64((1 << width) - 1)
    d = (ordmap(spec.keys, spec.kt) >> np.uint64(spec.bb)) & mask
    if spec.desc:
        d = mask - d                                       # the complement inside the sorted bits
    d = d.astype(UINT[1 if width <= 8 else 2 if width <= 16 else 4 if width <= 32 else 8])     # (same order, a faster sort)
    perm = np.arange(spec.n, dtype=np.int64)
    inside = np.zeros(spec.n, dtype=bool)
    for lo, hi in spec.segs:
        assert not inside[lo:hi].any(), "the case's segments overlap"
        perm[lo:hi] = lo + np.argsort(d[lo:hi], kind="stable")
        inside[lo:hi] = True
    return perm, inside


def verify(spec, sel_out, init, got, oracle=None):
    """init / got: {"k0", "k1"[, "v0", "v1"]} -> what the halves held before / hold after the call, as arrays of the element type.
    Raises an AssertionError that starts with the kind of the failure: selector, keys, stability, values, gap, witness."""
    assert sel_out == spec.sel0 ^ (passes_of(spec.bb, spec.eb) & 1), "selector: %d after the call, %s" % (sel_out, spec)
    perm, inside = reference(spec)
    fin = sel_out
    ek = spec.keys[perm]
    gk = got["k%d" % fin]
    bad = (gk != ek) & inside
    assert not bad.any(), "keys: %d differ from the reference inside the segments, the first at %d; %s" % (bad.sum(), np.argmax(bad), spec)
    if spec.vb:
        gv = got["v%d" % fin]
        bad = (gv != spec.vals[perm]) & inside
        if bad.any():
            at = int(np.argmax(bad))
            rows = np.minimum(gv[bad].astype(np.uint64), np.uint64(spec.n - 1)).astype(np.int64)
            kind = "stability: values of equal keys are not in input order" if np.array_equal(spec.keys[rows], ek[bad]) else \
                "values: they name rows that hold other keys"
            raise AssertionError("%s; %d differ from the reference, the first at %d; %s" % (kind, bad.sum(), at, spec))
    for name in sorted(got):
        bad = (got[name] != init[name]) & ~inside
        assert not bad.any(), "gap: %d position(s) outside every segment written in %s (the result is in half %d), the first at %d; %s" % (
            bad.sum(), name, fin, np.argmax(bad), spec)
    if oracle is not None and spec.bb == 0 and spec.eb == 8 * spec.kb and spec.kb >= 4 and spec.n <= WITNESS_MAX:
        img = ordmap(spec.keys, spec.kt)
        for lo, hi in spec.segs:
            if spec.kb == 4:
                r = oracle.lsb_reference_ranks(img[lo:hi].astype(np.uint32), 0, 32, spec.desc)
            else:
                r = oracle.lsb_reference_ranks_u64(img[lo:hi], U64, 0, 64, spec.desc)
            assert np.array_equal(lo + r.astype(np.int64), perm[lo:hi]), "witness: the oracle's ranks of segment [%d, %d) differ; %s" % (lo, hi, spec)


# -------------------------------------------------------------------------------------------------------------- harness --
def rotation(rot):
    """(workspace offset, workspace fill, pre-fill of the alternate halves, starting selector) of the rot-th call"""
    alt = ("explicit",) + FILLS
    return (1, 77, 255)[rot % 3], FILLS[rot % 3], alt[rot % 4], bin(rot).count("1") & 1


class Case:
    """one prepared call: place(A) reserves its buffers, launch() enqueues it, check() reads the arena and verifies"""

    def __init__(self, gs, entry, row, keys, begins, ends, bb, eb, desc, rot=0, sel0=None, alt=None, offsets=None, tag=""):
        kt, vb = row
        _, _, alt_r, sel_r = rotation(rot)
        self.gs, self.tag, self.alt = gs, tag, alt_r if alt is None else alt
        self.offsets = offsets                       # one array of nseg + 1 entries viewed as [:-1] / [1:]
        if offsets is not None:
            begins, ends = offsets[:-1], offsets[1:]
        self.begins, self.ends = np.asarray(begins, dtype=np.int32), np.asarray(ends, dtype=np.int32)
        self.nseg = self.begins.size
        self.spec = Spec(entry, kt, vb, keys, self.begins, self.ends, bb, eb, desc, sel_r if sel0 is None else sel0)
        self.sel = C.c_int(self.spec.sel0)

    def query(self):
        s, lib = self.spec, self.gs.lib
        if s.entry == "u32":
            return lib.gs_segmented_temp_bytes(s.n, int(s.vb != 0), self.nseg)
        if s.entry == "wide":
            return lib.gs_segmented_wide_temp_bytes(s.n, s.kb, s.vb, self.nseg)
        return lib.gs_segmented_narrow_temp_bytes(s.n, s.kt, s.vb, self.nseg)

    def place(self, A):
        s, t = self.spec, self.tag
        cur, oth = s.sel0, s.sel0 ^ 1
        for name, eb, data, byte in (("k", s.kb, s.keys, 0x3C), ("v", s.vb, s.vals, 0xC3)):
            if eb == 0:
                continue
            A.add(t + name + str(cur), s.n * eb, eb, data=data)
            if self.alt == "explicit":
                A.add(t + name + str(oth), s.n * eb, eb, data=np.full(s.n * eb, byte, dtype=np.uint8))
            else:
                A.add(t + name + str(oth), s.n * eb, eb, fill=self.alt)
        if self.offsets is not None:
            A.add(t + "offs", 4 * (self.nseg + 1), 0, data=np.asarray(self.offsets, dtype=np.int32), const=True)
        else:
            A.add(t + "ob", 4 * self.nseg, 0, data=self.begins, const=True).add(t + "oe", 4 * self.nseg, 0, data=self.ends, const=True)

    def launch(self, A, ws, nbytes, stream=None):
        s, t, lib = self.spec, self.tag, self.gs.lib
        kp = (C.c_void_p * 2)(A.ptr(t + "k0"), A.ptr(t + "k1"))
        vp = (C.c_void_p * 2)(A.ptr(t + "v0"), A.ptr(t + "v1")) if s.vb else None
        if self.offsets is not None:
            ob, oe = A.ptr(t + "offs"), A.ptr(t + "offs") + 4
        else:
            ob, oe = A.ptr(t + "ob"), A.ptr(t + "oe")
        sel = C.byref(self.sel)
        if s.entry == "u32":
            return lib.gs_segmented_sort_u32(ws, nbytes, kp, vp, sel, s.n, self.nseg, ob, oe, s.bb, s.eb, int(s.desc), s.kt, stream)
        if s.entry == "wide":
            return lib.gs_segmented_sort_wide(ws, nbytes, kp, vp, sel, s.n, self.nseg, ob, oe, s.kb, s.vb, s.bb, s.eb, int(s.desc), s.kt, stream)
        return lib.gs_segmented_sort_narrow(ws, nbytes, kp, vp, sel, s.n, self.nseg, ob, oe, s.kt, s.vb, s.bb, s.eb, int(s.desc), stream)

    def check(self, A, oracle=None):
        s, t = self.spec, self.tag
        names = [("k0", s.kb), ("k1", s.kb)] + ([("v0", s.vb), ("v1", s.vb)] if s.vb else [])
        init = {nm: A.init[t + nm].view(UINT[eb]) for nm, eb in names}
        got = {nm: A.read(t + nm, UINT[eb], s.n) for nm, eb in names}
        verify(s, self.sel.value, init, got, oracle)
        return got["k%d" % self.sel.value], (got["v%d" % self.sel.value] if s.vb else None)


def run_prepared(cuda, oracle, case, rot):
    """the prepared call in an arena of its own; returns the final halves of keys and values"""
    wsoff, wsfill, _, _ = rotation(rot)
    nb = case.query()
    assert nb > 0
    A = Arena(cuda, seed=rot)
    case.place(A)
    A.add("ws", nb, wsoff, fill=wsfill).build()
    rc = case.launch(A, A.ptr("ws"), nb)
    assert rc == 0, "returned %d; %s" % (rc, case.spec)
    A.check()
    return case.check(A, oracle)


def run_case(gs, cuda, oracle, entry, row, keys, begins, ends, bb, eb, desc, rot=0, **kw):
    return run_prepared(cuda, oracle, Case(gs, entry, row, keys, begins, ends, bb, eb, desc, rot=rot, **kw), rot)


def plain_kind(kt):
    """the float rows get the `special` kind (+-0, +-inf, subnormals, NaN payloads among uniform keys) where the others get uniform keys"""
    return "special" if kt in (F32, F64) else "uniform"


def full_bits(kt):
    return 8 * KEY_BYTES[kt]


def and_keys(kt, n, seed):
    """AND of four (32-bit keys) or five (64-bit keys) uniform draws: two set bits on average, so many duplicates"""
    kb = KEY_BYTES[kt]
    k = gen_keys(kt, "uniform", n, seed)
    for j in range(3 if kb == 4 else 4):
        k &= gen_keys(kt, "uniform", n, seed + 1000 * (j + 1))
    return k


def adjacent(sizes):
    ends = np.cumsum(sizes).astype(np.int64)
    return ends - np.asarray(sizes), ends


def one_element_gaps(sizes):
    """every segment preceded by a gap of exactly one element, and one more behind the last: (begins, ends, n)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    begins = np.cumsum(sizes + 1) - sizes
    return begins, begins + sizes, int(begins[-1] + sizes[-1]) + 1


def edge_layout(entry, seed):
    """case 2's segments: every edge size, shuffled and adjacent"""
    sizes = np.array(EDGE_SIZES[entry])
    sizes = sizes[np.random.default_rng(seed).permutation(sizes.size)]
    b, e = adjacent(sizes)
    return b, e, int(e[-1])


# --------------------------------------------------------------------------------------------- host-only: the yardsticks --
def test_cap_17408_is_what_the_capacities_imply(gs):
    """gs_msb_capacities sizes the bucket list as num_items / (largest local sort) + a constant: max_buckets grows by one exactly
    when num_items passes a multiple of 17408, for keys and for pairs.  If the local-sort classes change, this fails and the
    edge lists above have to follow."""
    def buckets(n, pairs):
        mb = C.c_uint32(0)
        gs.lib.gs_msb_capacities(n, pairs, C.byref(mb), None, None)
        return mb.value

    for pairs in (0, 1):
        base = buckets(0, pairs)
        assert buckets(U32_CAP - 1, pairs) == base
        for m in (1, 2, 3, 7, 100, 12345):
            at = m * U32_CAP
            assert buckets(at - 1, pairs) == base + m - 1, (pairs, m)
            assert buckets(at, pairs) == base + m, (pairs, m)
            assert buckets(at + 1, pairs) == base + m, (pairs, m)
            assert buckets(at + U32_CAP - 1, pairs) == base + m, (pairs, m)
        # no other step in between: over a stretch of consecutive sizes the list grows only at the multiples
        grown = [n for n in range(1, 4 * U32_CAP + 2) if buckets(n, pairs) != buckets(n - 1, pairs)]
        assert grown == [U32_CAP, 2 * U32_CAP, 3 * U32_CAP, 4 * U32_CAP], (pairs, grown)
    assert {U32_CAP - 1, U32_CAP, U32_CAP + 1} <= set(EDGE_SIZES["u32"])


def test_the_checker_can_fail():
    """verify() on a correct synthetic result (built here with Python's own stable sort, not with reference()), then on four
    corrupted ones: each must be refused with an error that names its kind."""
    rng = np.random.default_rng(5)
    n, bb, eb, sel0 = 300, 4, 12, 1                             # one pass: the result lands in half 0
    keys = (rng.integers(0, 6, size=n).astype(np.uint32) << np.uint32(6)) | rng.integers(0, 2, size=n).astype(np.uint32)   # a bit below begin_bit differs
    begins, ends = np.array([3, 120, 120, 200]), np.array([120, 120, 190, 290])     # adjacent, empty, gaps at both ends and at 190
    spec = Spec("u32", U32, 4, keys, begins, ends, bb, eb, False, sel0)
    assert spec.segs == [(3, 120), (120, 190), (200, 290)]
    init = {"k1": keys.copy(), "v1": spec.vals.copy(), "k0": np.full(n, 0x3C3C3C3C, np.uint32), "v0": np.full(n, 0xC3C3C3C3, np.uint32)}
    good = {nm: a.copy() for nm, a in init.items()}
    for lo, hi in spec.segs:
        order = sorted(range(lo, hi), key=lambda i: (int(keys[i]) >> bb) & 0xFF)
        good["k0"][lo:hi], good["v0"][lo:hi] = keys[order], spec.vals[order]
        good["k1"][lo:hi] = 0                                    # the other half may be overwritten inside the segments
    verify(spec, 0, init, good)

    def corrupted(**changes):
        bad = {nm: a.copy() for nm, a in good.items()}
        for nm, (i, j) in changes.items():
            bad[nm][[i, j]] = bad[nm][[j, i]]
        return bad

    run = next(i for i in range(3, 119) if good["k0"][i] == good["k0"][i + 1])      # two neighbours with equal keys
    with pytest.raises(AssertionError, match="^stability"):
        verify(spec, 0, init, corrupted(v0=(run, run + 1)), None)
    gap = {nm: a.copy() for nm, a in good.items()}
    gap["k1"].view(np.uint8)[4 * 195 + 2] ^= 0x10                                  # one byte of a gap key in the non-final half
    with pytest.raises(AssertionError, match="^gap.*k1"):
        verify(spec, 0, init, gap)
    assert good["k0"][119] != good["k0"][120]
    with pytest.raises(AssertionError, match="^keys"):                             # across the boundary of two adjacent segments
        verify(spec, 0, init, corrupted(k0=(119, 120), v0=(119, 120)))
    with pytest.raises(AssertionError, match="^selector"):
        verify(spec, 1, init, good)
    moved = corrupted(v0=(10, 150))                                                # a value that names another segment's key
    with pytest.raises(AssertionError, match="^values"):
        verify(spec, 0, init, moved)


# -------------------------------------------------------------------------- 1: long segments at unaligned offsets --
MIDDLE_RANGE = {32: (8, 24), 64: (20, 36), 16: (4, 12), 8: (3, 7)}       # two passes (u8: one), so the selector flips twice


@gpu
@pytest.mark.parametrize("entry,row", ENTRY_ROWS_ALL)
def test_long_segments_at_unaligned_offsets(gs, cuda, oracle, entry, row):
    """Three segments of 256 * tile - 1, 256 * tile and 256 * tile + 3 elements that begin at offsets = 5, 63 and 1 (mod 64):
    buckets of >= 256 tiles at unaligned offsets, which get a short first tile (ws_first_tile's tl - r branch) in the
    classification, the tile records, the histogram and the scatter of each kernel set.  Every gap is one element wide; two
    short segments (57 and 64 elements, each between one-element gaps) carry the layout from one residue to the next, since
    with one-element gaps alone the three begins cannot have these residues."""
    kt, vb = row
    tile = GEOMETRY[entry][0] if entry != "narrow" else gs.lib.gs_lsb_narrow_tile(kt, vb)
    assert tile in (4096, 8192)
    big = ALIGN_MIN_TILES * tile
    sizes = [big - 1, 57, big, 64, big + 3]
    begins, ends, at = [], [], 5
    for s in sizes:
        begins.append(at); ends.append(at + s)
        at += s + 1
    assert [begins[i] % 64 for i in (0, 2, 4)] == [5, 63, 1]
    n = ends[-1] + 1
    bits = full_bits(kt)
    for i, ((bb, eb), desc) in enumerate((((0, bits), False), (MIDDLE_RANGE[bits], True))):
        for j, kind in enumerate((plain_kind(kt), "few")):
            keys = gen_keys(kt, kind, n, seed=10 * i + j)
            run_case(gs, cuda, oracle, entry, row, keys, begins, ends, bb, eb, desc, rot=2 * i + j + vb)


# ---------------------------------------------------------------------------------------------- 2: every path's edges --
SUB_RANGE = {32: (3, 29), 64: (7, 53)}


@gpu
@pytest.mark.parametrize("desc", (False, True), ids=("asc", "desc"))
@pytest.mark.parametrize("entry,row", ENTRY_ROWS)
def test_every_paths_edges(gs, cuda, oracle, entry, row, desc):
    """One call whose segments have every size at which the classification takes another path (wave lists, local-sort classes,
    the tile, the cap where a segment becomes a bucket of the level, two level-path sizes), shuffled and adjacent: AND-reduced
    keys with many duplicates and the all-ones key (the local sorts' pad pattern ascending, the image 0 descending), over all
    bits and over a sub-range.  Then one size per path started at each of the 16 residues of a 16-element vector."""
    kt, vb = row
    bits = full_bits(kt)
    begins, ends, n = edge_layout(entry, seed=vb + bits)
    rot = int(desc) + 2 * vb
    for keys in (and_keys(kt, n, seed=vb + 5), gen_keys(kt, "pad", n, seed=0)):
        for bb, eb in ((0, bits), SUB_RANGE[bits]):
            run_case(gs, cuda, oracle, entry, row, keys, begins, ends, bb, eb, desc, rot=rot)
            rot += 1
    for size in RESIDUE_SIZES[entry]:
        b = np.array([r * (size + 16) + r for r in range(16)], dtype=np.int64)
        e = b + size
        run_case(gs, cuda, oracle, entry, row, gen_keys(kt, plain_kind(kt), int(e[-1]) + 5, seed=size), b, e, 0, bits, desc, rot=rot)
        rot += 1


# ----------------------------------------------------------------------------------------------------------- 3: neighbours --
NEIGHBOUR_ROWS = [pytest.param(e, r, id="%s-%s" % (e, row_id(r))) for e, r in (("u32", (U32, 0)), ("u32", (I32, 4)), ("wide", (U64, 0)),
                                                                                 ("wide", (F64, 8)))]


@gpu
@pytest.mark.parametrize("entry,row", NEIGHBOUR_ROWS)
def test_neighbours_one_element_gaps(gs, cuda, oracle, entry, row):
    """Segments of odd sizes -- four hundred small ones, the cap -1 and +1 and three level-path sizes -- shuffled, each preceded
    by a gap of exactly one element that holds a marker; the alternate halves are pre-filled with other bytes.  Both starting
    selectors; all bits, and a one-pass range so that the result lands in the other half.  Every gap position of both halves
    of keys and values must be unchanged (verify's "gap" check)."""
    kt, vb = row
    tile, cap = GEOMETRY[entry]
    bits = full_bits(kt)
    rng = np.random.default_rng(9)
    sizes = np.concatenate([rng.integers(0, 600, size=400) * 2 + 1, [cap - 1, cap + 1, 2 * tile + 1, 3 * cap + 1, 1, 3, 5]])
    sizes = sizes[rng.permutation(sizes.size)]
    begins, ends, n = one_element_gaps(sizes)
    gap = np.ones(n, dtype=bool)
    for lo, hi in zip(begins, ends):
        gap[lo:hi] = False
    assert gap.sum() == sizes.size + 1 and gap[0] and gap[-1]
    rot = 0
    for sel0 in (0, 1):
        keys = gen_keys(kt, plain_kind(kt), n, seed=sel0)
        keys[gap] = UINT[KEY_BYTES[kt]](0xA5A5A5A5A5A5A5A5 >> (64 - bits))
        for bb, eb in ((0, bits), (5, 13)):
            run_case(gs, cuda, oracle, entry, row, keys, begins, ends, bb, eb, bool(sel0), rot=rot, sel0=sel0, alt="explicit")
            rot += 1


# -------------------------------------------------------------------------------------------------------------- 4: layouts --
LAYOUT_ROW = {"u32": (I32, 4), "wide": (I64, 4)}
ONE_BIT, NINE_BITS = (5, 6), (4, 13)                # nine bits: two passes, the second of one bit


@gpu
@pytest.mark.parametrize("entry", ("u32", "wide"))
def test_segments_listed_in_any_order(gs, cuda, oracle, entry):
    """(a) case 2's segments passed in reversed and in shuffled order: the result is identical to the ordered call's"""
    row = LAYOUT_ROW[entry]
    kt, vb = row
    begins, ends, n = edge_layout(entry, seed=4)
    order = np.argsort(begins)
    keys = and_keys(kt, n, seed=41)
    results = []
    for pick in (order, order[::-1], np.random.default_rng(42).permutation(order)):
        results.append(run_case(gs, cuda, oracle, entry, row, keys, begins[pick], ends[pick], 0, full_bits(kt), False, rot=3))
    for k, v in results[1:]:
        assert np.array_equal(k, results[0][0]) and np.array_equal(v, results[0][1])


@gpu
@pytest.mark.parametrize("entry", ("u32", "wide"))
def test_many_more_segments_than_items(gs, cuda, oracle, entry):
    """(b) 5000 items, 200 000 segments: 150 real ones scattered among empty (b == e) and inverted (e < b) ones"""
    row = LAYOUT_ROW[entry]
    kt, vb = row
    n, nseg, real = 5000, 200000, 150
    rng = np.random.default_rng(43)
    cuts = np.sort(rng.choice(n + 1, size=2 * real, replace=False))
    begins = rng.integers(0, n + 1, size=nseg)
    ends = begins.copy()                                           # empty ...
    inv = rng.random(nseg) < 0.5
    ends[inv] = begins[inv] - rng.integers(1, 3000, size=int(inv.sum()))      # ... or inverted (some ends below 0)
    at = rng.choice(nseg, size=real, replace=False)
    begins[at], ends[at] = cuts[0::2], cuts[1::2]
    assert len(clamped(begins, ends, n)) == real
    for i, desc in enumerate((False, True)):
        run_case(gs, cuda, oracle, entry, row, and_keys(kt, n, seed=44 + i), begins, ends, 0, full_bits(kt), desc, rot=i)
    run_case(gs, cuda, oracle, entry, row, gen_keys(kt, "uniform", n, seed=46), begins, ends, *NINE_BITS, False, rot=2)


@gpu
@pytest.mark.parametrize("entry", ("u32", "wide"))
def test_one_offsets_array_with_head_and_tail_gaps(gs, cuda, oracle, entry):
    """(c) one offsets array of k + 1 entries passed as [:-1] / [1:], the first cut above 0 and the last below n"""
    row = LAYOUT_ROW[entry]
    kt, vb = row
    tile, cap = GEOMETRY[entry]
    sizes = np.array([700, 0, cap + 1, 1, 64, 2 * tile + 1, 0, 0, 3000, cap, 257])
    offs = 3 + np.concatenate([[0], np.cumsum(sizes)])
    n = int(offs[-1]) + 7
    for i, (bb, eb) in enumerate(((0, full_bits(kt)), ONE_BIT)):
        run_case(gs, cuda, oracle, entry, row, gen_keys(kt, "few" if i else "uniform", n, seed=47 + i), None, None, bb, eb, bool(i),
                 rot=i + 1, offsets=offs)


def long_equal_case(gs, entry, row, bb, eb, desc, rot, tag=""):
    """(d) a segment of 3 * cap + 1 equal keys and one in which one value holds 90 %, a gap of three elements between them.  The
    equal key is the one whose sorted image is all ones -- the local sorts' pad pattern: the all-ones key ascending, 0 descending."""
    kt, vb = row
    m = 3 * GEOMETRY[entry][1] + 1
    ut = UINT[KEY_BYTES[kt]]
    equal = np.full(m, 0 if desc else np.iinfo(ut).max, dtype=ut)
    keys = np.concatenate([gen_keys(kt, "uniform", 2, seed=1), equal, gen_keys(kt, "uniform", 3, seed=2), gen_keys(kt, "zipf", m, seed=3 + rot),
                           gen_keys(kt, "uniform", 1, seed=4)])
    return Case(gs, entry, row, keys, [2, m + 5], [m + 2, 2 * m + 5], bb, eb, desc, rot=rot, tag=tag)


@gpu
@pytest.mark.parametrize("entry", ("u32", "wide"))
def test_long_segments_of_equal_and_of_skewed_keys(gs, cuda, oracle, entry):
    row = LAYOUT_ROW[entry]
    rot = 0
    for bb, eb in ((0, full_bits(row[0])), ONE_BIT, NINE_BITS):
        for desc in (False, True):
            run_prepared(cuda, oracle, long_equal_case(gs, entry, row, bb, eb, desc, rot), rot)
            rot += 1


# ------------------------------------------------------------------------------- 5: two sorts, one workspace, side stream --
@gpu
@pytest.mark.parametrize("entry", ("u32", "wide"))
def test_two_sorts_one_workspace_side_stream(gs, cuda, oracle, entry):
    """case 2's call, then case 4 (d)'s, back to back on a side stream in one workspace sized for the larger query, with no
    synchronisation between them; both results are checked"""
    row = LAYOUT_ROW[entry]
    kt, vb = row
    begins, ends, n = edge_layout(entry, seed=5)
    first = Case(gs, entry, row, and_keys(kt, n, seed=51), begins, ends, *SUB_RANGE[full_bits(kt)], True, rot=1, tag="a_")
    second = long_equal_case(gs, entry, row, *NINE_BITS, False, rot=2, tag="b_")
    nb = max(first.query(), second.query())
    assert first.query() != second.query()
    A = Arena(cuda, seed=5)
    first.place(A)
    second.place(A)
    A.add("ws", nb, 77, fill="random").build()
    stream = torch.cuda.Stream(device=cuda)
    for case in (first, second):
        rc = case.launch(A, A.ptr("ws"), nb, C.c_void_p(stream.cuda_stream))
        assert rc == 0, "returned %d; %s" % (rc, case.spec)
    stream.synchronize()
    A.check()
    first.check(A, oracle)
    second.check(A, oracle)
