"""References, checkers and case generators for the four stage calls of the bucket-sharded sort: gs_shard_histogram_u32,
gs_shard_partition_u32, gs_msb_first_pass_u32 and gs_msb_finish_u32 (tests/test_shard_stages_cpu.py guards this module,
tests/test_shard_stages_gpu.py runs the cases on the device).

numpy only.  Keys are uint32 bit patterns throughout; every comparison is np.array_equal on uint32 / uint64, there is no
tolerance anywhere.  "Mapped" means the key type's order-preserving u32 form (ordmap), "raw" the caller's representation.

A piece table is a (num_src, 256) uint64 array: pieces[s][b] keys of top byte b came from source s.  The buffer it
describes is source-major, and inside a source the buckets lie in byte order."""
import numpy as np

from lsb_plan_child import f32_specials

U32, I32, F32 = 0, 1, 2
KEY_TYPES = (U32, I32, F32)
KT_NAME = {U32: "u32", I32: "i32", F32: "f32"}
SIGN = np.uint32(0x80000000)
TILE = 8192                    # keys per tile of the MSB levels (MSB_TILE)
PIECE_ALIGN_MIN_TILES = 16     # a piece of that many tiles or more gets a short first tile when it starts unaligned
TILE_ALIGN = 64                # ... unaligned = (offset & 63) != 0
LOCAL_SORT_MAX = 17408         # the largest local sort (keys alone; with values it is no larger)


# ------------------------------------------------------------------------------------------------------ the map --
def ordmap(keys, kt):
    """The order-preserving u32 map: I32 flips the sign bit; F32 complements negative keys and sets the sign bit of the
    others, so -0.0 sorts before +0.0 and NaNs sort by their bits."""
    k = np.asarray(keys, dtype=np.uint32)
    if kt == I32:
        return k ^ SIGN
    if kt == F32:
        return np.where(k & SIGN != 0, ~k, k | SIGN).astype(np.uint32)
    assert kt == U32, kt
    return k.copy()


def unmap(mapped, kt):
    """The inverse of ordmap."""
    m = np.asarray(mapped, dtype=np.uint32)
    if kt == I32:
        return m ^ SIGN
    if kt == F32:
        return np.where(m & SIGN != 0, m ^ SIGN, ~m).astype(np.uint32)
    assert kt == U32, kt
    return m.copy()


def f32_special_bits():
    """Every special f32_specials can draw: +-0, +-inf, +-subnormals, NaNs of both signs with payloads (raw bits)."""
    k = f32_specials(np.random.default_rng(0), 4096)
    tiny = np.finfo(np.float32).smallest_subnormal
    base = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, np.nan, -np.nan], np.float32).view(np.uint32)
    sp = np.unique(np.concatenate([base, np.array([0x7FC00001, 0xFFC12345, 0x7F800001], np.uint32)]))
    assert np.isin(sp, k).all(), "f32_specials no longer draws every special listed here"
    return sp


F32_SPECIALS = f32_special_bits()
MAPPED_SPECIALS = ordmap(F32_SPECIALS, F32)          # their top bytes are 0x00, 0x7f, 0x80 and 0xff


def has_f32_specials(raw):
    return bool(np.isin(F32_SPECIALS, raw).all())


def sprinkle_specials(raw, rng, where=None):
    """Overwrite F32_SPECIALS.size distinct positions of raw (among `where`, default anywhere) with the specials."""
    idx = np.arange(raw.size) if where is None else np.asarray(where)
    assert idx.size >= F32_SPECIALS.size
    raw[rng.choice(idx, F32_SPECIALS.size, replace=False)] = F32_SPECIALS
    return raw


def raw_keys(kt, n, rng):
    """Random key bits of every magnitude: I32 keys straddle zero, F32 keys carry f32_specials' mix."""
    if kt == F32 and n:
        k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        m = max(1, n // 16)
        sp = f32_specials(rng, m)
        k[rng.choice(n, m, replace=False)] = sp
        if n >= 4 * F32_SPECIALS.size:
            sprinkle_specials(k, rng)
        return k
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint32)


# --------------------------------------------------------------------------------------- references and checkers --
def ref_histogram(keys, kt, bits):
    return np.bincount(ordmap(keys, kt) >> np.uint32(32 - bits), minlength=1 << bits).astype(np.uint64)


def ref_partition(keys, vals, kt, bits, dest, ranks):
    """Stable group-by-destination: keys stay raw.  -> (keys, vals or None, counts[ranks])"""
    r = np.asarray(dest, np.uint8)[ordmap(keys, kt) >> np.uint32(32 - bits)]
    order = np.argsort(r, kind="stable")
    return keys[order], (None if vals is None else vals[order]), np.bincount(r, minlength=ranks).astype(np.uint64)


def ref_first_pass(keys, vals, kt):
    """Stable partition on the mapped top byte: keys leave mapped.  -> (keys, vals or None, counts[256])"""
    m = ordmap(keys, kt)
    top = m >> np.uint32(24)
    order = np.argsort(top, kind="stable")
    return m[order], (None if vals is None else vals[order]), np.bincount(top, minlength=256).astype(np.uint64)


def ref_finish_keys(recv_mapped, kt):
    return unmap(np.sort(np.asarray(recv_mapped, np.uint32)), kt)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s%s against %s%s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s: %d of %d differ, the first at %d: got 0x%x, expected 0x%x"
                             % (what, int((got != want).sum()), got.size, i, int(got[i]), int(want[i])))


def check_histogram(got, keys, kt, bits):
    _same(np.asarray(got, np.uint64), ref_histogram(keys, kt, bits), "histogram")


def check_partition(got_k, got_v, got_counts, keys, vals, kt, bits, dest, ranks):
    ek, ev, ec = ref_partition(keys, vals, kt, bits, dest, ranks)
    _same(np.asarray(got_counts, np.uint64), ec, "partition counts")
    _same(got_k, ek, "partition keys")
    if vals is not None:
        _same(got_v, ev, "partition values")


def check_first_pass(got_k, got_v, got_counts, keys, vals, kt):
    ek, ev, ec = ref_first_pass(keys, vals, kt)
    _same(np.asarray(got_counts, np.uint64), ec, "first-pass counts")
    _same(got_k, ek, "first-pass keys")
    if vals is not None:
        _same(got_v, ev, "first-pass values")


def check_finish(got_k, got_v, recv_k, recv_v, kt):
    """recv_k: the received buffer (mapped keys); recv_v: any labels.  The sort is unstable: the keys are fixed bit for
    bit, the values must be a permutation of recv_v in which every value still goes with its key."""
    _same(got_k, ref_finish_keys(recv_k, kt), "finish keys")
    if recv_v is not None:
        sh = np.uint64(32)
        got = (ordmap(got_k, kt).astype(np.uint64) << sh) | np.asarray(got_v, np.uint32).astype(np.uint64)
        want = (np.asarray(recv_k, np.uint32).astype(np.uint64) << sh) | np.asarray(recv_v, np.uint32).astype(np.uint64)
        _same(np.sort(got), np.sort(want), "finish (key, value) pairs")


# -------------------------------------------------------------------------------- histogram and partition inputs --
HIST_DISTS = ("uniform", "one_bin", "first_last")


def hist_keys(kt, dist, n, bits, rng):
    """Raw keys of the named distribution over the 2^bits bins of the MAPPED key."""
    if dist == "uniform":
        return raw_keys(kt, n, rng)
    low = rng.integers(0, 1 << (32 - bits), size=n, dtype=np.uint64)
    nb = 1 << bits
    if dist == "one_bin":                      # one LDS counter takes the whole input
        bins = np.full(n, int(rng.integers(0, nb)), np.uint64)
    else:
        assert dist == "first_last"
        bins = np.where(rng.random(n) < 0.5, 0, nb - 1).astype(np.uint64)
    return unmap(((bins << np.uint64(32 - bits)) | low).astype(np.uint32), kt)


DEST_KINDS = ("random", "gaps", "all_last")


def dest_table(kind, bits, ranks, rng):
    """A monotone bin -> rank table of 2^bits entries, every entry < ranks."""
    nb = 1 << bits
    if kind == "random":
        d = np.sort(rng.integers(0, ranks, size=nb))
    elif kind == "gaps":                       # about half of the ranks own no bin (rank 0 among them when there are 3 or more)
        owners = np.arange(ranks)[1::2] if ranks >= 3 else np.arange(ranks)[-1:]
        d = np.sort(owners[rng.integers(0, owners.size, size=nb)])
    else:
        assert kind == "all_last"
        d = np.full(nb, ranks - 1)
    return d.astype(np.uint8)


HIST_SIZES = (0, 1, 3, 4, 5, 8191, 8192, 8193, 100003)
HIST_LARGE = 2048 * TILE + 3 * TILE + 5      # the grid is capped at 2048 workgroups: unrolled loop, vector loop and tail all run
HIST_BITS = (1, 8, 11, 12)
PART_SIZES = (1, 8191, 8192, 8193, 8 * TILE - 1, 8 * TILE, 8 * TILE + 1, 100003)
PART_BITS = (1, 8, 12)
PART_RANKS = (1, 2, 3, 255, 256)


def partition_plan(size_index):
    """The partition calls made at PART_SIZES[size_index]: every key type x pairs x bits x rank count, the dest table's
    kind rotating with the combination and the size.  -> [(kt, pairs, bits, ranks, dest kind)]"""
    plan = []
    for kt in KEY_TYPES:
        for pairs in (False, True):
            for bits in PART_BITS:
                for ranks in PART_RANKS:
                    plan.append((kt, pairs, bits, ranks, DEST_KINDS[(len(plan) + size_index) % len(DEST_KINDS)]))
    return plan


# ------------------------------------------------------------------------------------------ crafted piece tables --
def build_receive(pieces, rng, low=None, specials=None):
    """The receive buffer of a piece table, built without any first pass: source after source, each source's buckets in
    byte order, every piece filled with mapped keys of its top byte.  low(b, size, rng) gives the low 24 bits of a piece
    of bucket b (default: random).  specials: mapped keys; each one whose bucket is not empty overwrites one key of it."""
    pieces = np.asarray(pieces, np.uint64)
    assert pieces.ndim == 2 and pieces.shape[1] == 256
    parts = []
    for s in range(pieces.shape[0]):
        for b in np.nonzero(pieces[s])[0]:
            c = int(pieces[s][b])
            lo = rng.integers(0, 1 << 24, size=c, dtype=np.uint32) if low is None else np.asarray(low(int(b), c, rng), np.uint32)
            assert lo.size == c and (not c or int(lo.max()) < (1 << 24))
            parts.append((np.uint32(b) << np.uint32(24)) | lo)
    keys = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    if specials is not None and keys.size:
        top = keys >> np.uint32(24)
        taken = set()
        for sp in np.asarray(specials, np.uint32):
            cand = [int(i) for i in np.nonzero(top == (sp >> np.uint32(24)))[0] if int(i) not in taken][:64]
            if cand:
                i = cand[int(rng.integers(0, len(cand)))]
                taken.add(i)
                keys[i] = sp
    return keys


def piece_offsets(pieces):
    """offset[s][b] of every piece in the buffer build_receive lays out."""
    flat = np.asarray(pieces, np.uint64).reshape(-1)
    return (np.cumsum(flat) - flat).reshape(np.asarray(pieces).shape)


def piece_tiles(off, size):
    """Tiles of a piece as the finish cuts it (msb_piece_first_tile / msb_piece_tiles)."""
    r = off & (TILE_ALIGN - 1)
    first = min(size, TILE) if (r == 0 or size < PIECE_ALIGN_MIN_TILES * TILE) else TILE - r
    return 1 + (size - first + TILE - 1) // TILE


class Layout:
    def __init__(self, name, pieces, keys, **meta):
        self.name, self.pieces, self.keys, self.meta = name, np.ascontiguousarray(pieces, dtype=np.uint64), keys, meta
        assert int(self.pieces.sum()) == keys.size

    @property
    def num_src(self):
        return self.pieces.shape[0]


def layout_full_table(rng):
    """256 sources, all 65536 pieces non-empty, 1 to 5 keys each."""
    pieces = rng.integers(1, 6, size=(256, 256)).astype(np.uint64)
    return Layout("full_table", pieces, build_receive(pieces, rng, specials=MAPPED_SPECIALS))


def layout_full_column(rng, bucket=0x7F):
    """256 sources, one bucket present in every source, everything else empty."""
    pieces = np.zeros((256, 256), np.uint64)
    pieces[:, bucket] = rng.integers(1, 400, size=256)
    sp = MAPPED_SPECIALS[MAPPED_SPECIALS >> np.uint32(24) == bucket]
    return Layout("full_column", pieces, build_receive(pieces, rng, specials=sp), bucket=bucket)


def layout_one_source(rng, src=137, n=30000):
    """A single source of 256 holds everything."""
    pieces = np.zeros((256, 256), np.uint64)
    pieces[src] = np.bincount(rng.integers(0, 256, size=n), minlength=256)
    pieces[src][[0x00, 0x7F, 0x80, 0xFF]] += 3
    return Layout("one_source", pieces, build_receive(pieces, rng, specials=MAPPED_SPECIALS), src=src)


THRESHOLD_SIZES = (TILE - 1, TILE, TILE + 1, 16 * TILE - 1, 16 * TILE, 16 * TILE + 1, 17 * TILE + 5)
THRESHOLD_STARTS = (0, 1, 63)


def layout_threshold(rng, size, start):
    """Source 0: a piece of 64 + start keys (bucket 0x00) shifts the piece under test (bucket 0x7f, `size` keys) to an
    offset with (offset & 63) == start; bucket 0x80 follows it, so a second bucket's tile range comes behind the ragged
    one.  Source 1 adds a piece to each of the two buckets and one to 0xff, so both buckets arrive in pieces."""
    pieces = np.zeros((2, 256), np.uint64)
    pieces[0][0x00] = 64 + start
    pieces[0][0x7F] = size
    pieces[0][0x80] = 5000
    pieces[1][0x7F] = 3001
    pieces[1][0x80] = 2999
    pieces[1][0xFF] = 7
    keys = build_receive(pieces, rng, specials=MAPPED_SPECIALS)
    return Layout("threshold_%d_%d" % (size, start), pieces, keys, piece=(0, 0x7F), offset=64 + start, size=size)


DEPTH_KEYS = 40000
DEPTH_PREFIX = 0x7FFFFF       # mapped; as F32 these are -0.0 and the 255 smallest negative subnormals


def layout_depth(rng, equal=False):
    """One bucket of 40 000 keys that share their top 24 bits (all equal: share all 32), in 3 pieces across 3 sources:
    too large for a local sort, and no byte separates it before the last one (none at all when equal)."""
    pieces = np.zeros((3, 256), np.uint64)
    pieces[:, DEPTH_PREFIX >> 16] = (13333, 13334, 13333)

    def low(b, c, r):
        last = np.full(c, 0xFF, np.uint32) if equal else r.integers(0, 256, size=c, dtype=np.uint32)
        return np.uint32((DEPTH_PREFIX & 0xFFFF) << 8) | last
    keys = build_receive(pieces, rng, low=low)
    if not equal:
        keys[[5, 20000, 39999]] = (0x7FFFFFFF, 0x7FFFFFFE, 0x7FFFFFFC)       # -0.0, -tiny, -3 tiny
    return Layout("depth_equal" if equal else "depth", pieces, keys, bucket=DEPTH_PREFIX >> 16)


HEAVY_KEYS, HEAVY_SHARE, HEAVY_KEY = 60000, 0.9, 0x80000000      # mapped; +0.0 as F32, 0 as I32


def layout_heavy(rng):
    """One bucket of 60 000 keys in 4 pieces, in which one key has a 0.9 share."""
    pieces = np.zeros((4, 256), np.uint64)
    pieces[:, HEAVY_KEY >> 24] = HEAVY_KEYS // 4

    def low(b, c, r):
        lo = r.integers(0, 1 << 24, size=c, dtype=np.uint32)
        lo[r.random(c) < HEAVY_SHARE] = HEAVY_KEY & 0xFFFFFF
        return lo
    keys = build_receive(pieces, rng, low=low)
    keys[[1, 59999]] = (0x80000001, 0x80000003)                               # +tiny, +3 tiny
    return Layout("heavy", pieces, keys, bucket=HEAVY_KEY >> 24, key=HEAVY_KEY)


def layout_tiny(rng, total, num_src=3):
    """`total` keys (0, 1 or 2) in a table of num_src sources."""
    pieces = np.zeros((num_src, 256), np.uint64)
    for i in range(total):
        pieces[(2 * i + 1) % num_src][(0x80, 0x7F)[i % 2]] += 1
    return Layout("tiny_%d" % total, pieces, build_receive(pieces, rng, specials=MAPPED_SPECIALS[:1]))


def layout_groups(rng, cuts=(0, 100, 256), num_src=3, per_piece=90):
    """A receive buffer as sharded.py lays it out for several groups: group-major, source-major inside a group.  Group g
    owns the buckets [cuts[g], cuts[g + 1]); -> one Layout per group (its table is zero outside its own bucket range)."""
    full = rng.integers(0, 2 * per_piece, size=(num_src, 256)).astype(np.uint64)
    out = []
    for g in range(len(cuts) - 1):
        pieces = np.zeros_like(full)
        pieces[:, cuts[g]:cuts[g + 1]] = full[:, cuts[g]:cuts[g + 1]]
        out.append(Layout("group%d" % g, pieces, build_receive(pieces, rng, specials=MAPPED_SPECIALS), buckets=(cuts[g], cuts[g + 1])))
    return out


# ------------------------------------------------------------------------------------- the emulated sharded sort --
SHARD_KEYS = 50000
WORLDS = (1, 2, 3, 8)
SHARDED_INPUTS = ("uniform", "hot_key", "hot_byte", "all_equal", "sorted", "f32_negative", "tiny", "uneven")
TINY_SIZES = (5, 0, 3, 1, 0, 2, 4, 0)
UNEVEN_SIZES = (SHARD_KEYS, 17, 0, 9001, 120000, 1, 8192, 30011)


def sharded_inputs(kt):
    return [i for i in SHARDED_INPUTS if i != "f32_negative" or kt == F32]


def sharded_shards(name, kt, world, seed=0):
    """The raw shards of the named input, one per rank."""
    rng = np.random.default_rng([seed, kt, world, SHARDED_INPUTS.index(name)])
    n = SHARD_KEYS
    if name == "uniform":
        return [raw_keys(kt, n, rng) for _ in range(world)]
    if name == "hot_key":                       # one key with a 0.9 share
        hot = {U32: 0x9E3779B9, I32: 0xFFFFFFFF, F32: 0x80000000}[kt]            # I32: -1, F32: -0.0
        out = []
        for _ in range(world):
            k = raw_keys(kt, n, rng)
            k[F32_SPECIALS.size:][rng.random(n - F32_SPECIALS.size) < 0.9] = hot
            if kt == F32:
                k[:F32_SPECIALS.size] = F32_SPECIALS
            out.append(k)
        return out
    if name == "hot_byte":                      # one hot top byte (of the mapped key) on every rank
        out = []
        for _ in range(world):
            m = ordmap(raw_keys(kt, n, rng), kt)
            hot = np.nonzero(rng.random(n) < 0.8)[0]
            m[hot] = np.uint32(0x80 << 24) | (m[hot] & np.uint32(0xFFFFFF))
            k = unmap(m, kt)
            out.append(sprinkle_specials(k, rng) if kt == F32 else k)
        return out
    if name == "all_equal":
        return [np.full(n, {U32: 0xDEADBEEF, I32: 0xFFFFFFFF, F32: 0x80000000}[kt], np.uint32) for _ in range(world)]
    if name == "sorted":                        # already sorted across the ranks
        k = raw_keys(kt, n * world, rng)
        m = np.sort(ordmap(k, kt))
        return [unmap(m[r * n:(r + 1) * n], kt) for r in range(world)]
    if name == "f32_negative":
        assert kt == F32
        neg = F32_SPECIALS[F32_SPECIALS & SIGN != 0]
        out = []
        for _ in range(world):
            k = rng.integers(0, 1 << 32, size=n, dtype=np.uint32) | SIGN
            k[rng.choice(n, neg.size, replace=False)] = neg
            out.append(k)
        return out
    if name == "tiny":                          # shards of 0 to 5 keys, some ranks empty
        pool = F32_SPECIALS if kt == F32 else np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x12345678], np.uint32)
        return [pool[rng.integers(0, pool.size, size=TINY_SIZES[r])].astype(np.uint32) for r in range(world)]
    assert name == "uneven"                     # sources of very different size
    return [raw_keys(kt, UNEVEN_SIZES[r], rng) for r in range(world)]


def shard_values(shards):
    """value = rank * n + index (n: the largest shard), so a value names its key globally."""
    n = max([s.size for s in shards] + [1])
    return [(np.uint32(r * n) + np.arange(s.size, dtype=np.uint32)).astype(np.uint32) for r, s in enumerate(shards)]


class Sharded:
    """What emulate_sharded_sort produced: per source rank the grouped shard and its counts, the map and the plan, per
    destination rank the received buffer, its piece table and the finished slice."""

    def __init__(self):
        self.grouped_k, self.grouped_v, self.counts = [], [], []
        self.recv_k, self.recv_v, self.pieces, self.out_k, self.out_v = [], [], [], [], []
        self.dest = self.per_rank = None


def emulate_sharded_sort(shards, kt, pairs, world, ops, pipeline="msb", bits=12):
    """The steps of gs_msb_sort_u32_sharded for every rank of `world`, on one device, in one process, with no collective:
    per source rank a first pass with kt; sharded.compute_splits / sharded.exchange_plan on the gathered counts; the
    receive buffers cut out of the grouped shards at the plan's offsets (source-major); per destination rank one finish
    with kt (none for an empty receive, as the C++ host does).  ops: {"first_pass": f(keys, vals, kt) -> (keys, vals,
    counts), "finish": f(recv_k, recv_v, pieces, kt) -> (keys, vals), "histogram": f(keys, kt, bits) -> hist, "partition":
    f(keys, vals, kt, bits, dest, ranks) -> (keys, vals, counts)} on numpy arrays; vals is None for keys alone.
    pipeline "partition": the fallback's stages instead -- histogram, split on `bits` bits, partition (keys stay raw),
    and a host sort of what arrived in place of the local sort, which is none of the four calls."""
    from gpu_sort_amd import sharded
    assert len(shards) == world and pipeline in ("msb", "partition")
    vals = shard_values(shards) if pairs else [None] * world
    R = Sharded()
    if pipeline == "msb":
        for r in range(world):
            gk, gv, c = ops["first_pass"](shards[r], vals[r], kt)
            R.grouped_k.append(gk); R.grouped_v.append(gv); R.counts.append(np.asarray(c, np.uint64))
        hist_all = np.stack(R.counts)
    else:
        hist_all = np.stack([np.asarray(ops["histogram"](shards[r], kt, bits), np.uint64) for r in range(world)])
    R.dest, R.per_rank = sharded.compute_splits(hist_all, world)
    if pipeline == "partition":
        for r in range(world):
            gk, gv, c = ops["partition"](shards[r], vals[r], kt, bits, R.dest, world)
            R.grouped_k.append(gk); R.grouped_v.append(gv); R.counts.append(np.asarray(c, np.uint64))
    send = [sharded.exchange_plan(hist_all, R.dest, s, world)[0] for s in range(world)]
    soff = [np.concatenate(([0], np.cumsum(x))).astype(np.int64) for x in send]
    for d in range(world):
        recv = sharded.exchange_plan(hist_all, R.dest, d, world)[1]
        assert [int(send[s][d]) for s in range(world)] == [int(x) for x in recv]
        cut = lambda g: np.concatenate([g[s][soff[s][d]:soff[s][d + 1]] for s in range(world)])
        rk = cut(R.grouped_k)
        rv = cut(R.grouped_v) if pairs else None
        pieces = np.where(R.dest[None, :] == d, hist_all, 0).astype(np.uint64)
        R.recv_k.append(rk); R.recv_v.append(rv); R.pieces.append(pieces)
        if pipeline == "partition":
            order = np.argsort(ordmap(rk, kt), kind="stable")
            ok, ov = rk[order], (rv[order] if pairs else None)
        elif rk.size == 0:
            ok, ov = np.zeros(0, np.uint32), (np.zeros(0, np.uint32) if pairs else None)
        else:
            ok, ov = ops["finish"](rk, rv, pieces, kt)
        R.out_k.append(ok); R.out_v.append(ov)
    return R


def check_sharded(R, shards, kt, pairs, world, pipeline="msb", bits=12):
    """The ranks' outputs, one behind the other, equal the global reference bit for bit; every rank's count equals per_rank
    of the split; every stage output equals its own reference; every value still names its key."""
    allk = np.concatenate(shards) if shards else np.zeros(0, np.uint32)
    vals = shard_values(shards)
    for r in range(world):
        if pipeline == "msb":
            check_first_pass(R.grouped_k[r], R.grouped_v[r], R.counts[r], shards[r], vals[r] if pairs else None, kt)
        else:
            check_partition(R.grouped_k[r], R.grouped_v[r], R.counts[r], shards[r], vals[r] if pairs else None, kt, bits, R.dest, world)
        assert R.out_k[r].size == int(R.per_rank[r]), "rank %d holds %d keys, the split gives it %d" % (r, R.out_k[r].size, int(R.per_rank[r]))
    _same(np.concatenate(R.out_k), unmap(np.sort(ordmap(allk, kt)), kt), "sharded keys")
    if pairs:
        gv = np.concatenate(R.out_v)
        allv = np.concatenate(vals)
        _same(np.sort(gv), np.sort(allv), "sharded values (a permutation)")
        n = max([s.size for s in shards] + [1])
        table = np.zeros(world * n, np.uint32)
        for r, s in enumerate(shards):
            table[r * n:r * n + s.size] = s
        _same(table[gv], np.concatenate(R.out_k), "sharded values (each names its key)")


def numpy_ops():
    """numpy stand-ins for the four calls (the references themselves; the finish also checks that the piece table
    describes the buffer it is given)."""
    def finish(recv_k, recv_v, pieces, kt):
        pieces = np.asarray(pieces, np.uint64)
        assert int(pieces.sum()) == recv_k.size, "piece table and buffer differ in size"
        top = np.repeat(np.tile(np.arange(256, dtype=np.uint32), pieces.shape[0]), pieces.reshape(-1).astype(np.int64))
        assert np.array_equal(recv_k >> np.uint32(24), top), "piece table does not describe the received buffer"
        order = np.argsort(recv_k, kind="stable")
        return unmap(recv_k[order], kt), (None if recv_v is None else recv_v[order])
    return {"first_pass": ref_first_pass, "finish": finish, "histogram": lambda k, kt, bits: ref_histogram(k, kt, bits),
            "partition": ref_partition}
