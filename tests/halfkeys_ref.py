"""The numpy reference of the 8- and 16-bit float key categories (GS_KEY_F16 / GS_KEY_BF16 / GS_KEY_F8), shared by the
test_halfkeys_* modules.  Nothing here calls the library: the image is np.where(b & S, b ^ ALL, b ^ S), the sort key is
the digit [begin_bit, end_bit) of it, complemented when descending, and the order is np.argsort(kind="stable")."""
import numpy as np

KINDS = {               # name -> (gs key type name, the integer type of the same width, bits)
    "f16": ("GS_KEY_F16", "GS_KEY_U16", 16),
    "bf16": ("GS_KEY_BF16", "GS_KEY_U16", 16),
    "f8": ("GS_KEY_F8", "GS_KEY_U8", 8),
}


def utype(bits):
    return np.uint8 if bits == 8 else np.uint16


def image(b, bits):
    """the order-preserving image of bit patterns b (any unsigned integer array) at width `bits`, as uint32"""
    b = b.astype(np.uint32)
    S, ALL = np.uint32(1 << (bits - 1)), np.uint32((1 << bits) - 1)
    return np.where(b & S, b ^ ALL, b ^ S).astype(np.uint32)


def sort_key(b, bits, bb, eb, desc):
    d = (image(b, bits) >> np.uint32(bb)) & np.uint32((1 << (eb - bb)) - 1)
    return (np.uint32((1 << (eb - bb)) - 1) - d) if desc else d


def order(b, bits, bb, eb, desc):
    """rows of b in sorted order (stable)"""
    return np.argsort(sort_key(b, bits, bb, eb, desc), kind="stable")


def gen_bits(kind, n, inp, seed):
    """n bit patterns.  every: each pattern of the width the same number of times where n allows, shuffled (both zeros, both
    infinities and NaNs of both signs among them); uniform: random bits; equal: one negative value; two: two magnitudes with
    both signs; clean: finite non-zero values only (no NaN, no infinity, no zero), for the comparison with torch.sort"""
    bits = KINDS[kind][2]
    card = 1 << bits
    rng = np.random.default_rng(seed)
    S = 1 << (bits - 1)
    if inp == "every":
        raw = rng.permutation(np.arange(n, dtype=np.uint32) % np.uint32(card))
    elif inp == "uniform":
        raw = rng.integers(0, card, size=n, dtype=np.uint32)
    elif inp == "equal":
        raw = np.full(n, S | int(rng.integers(1, S >> 2)), dtype=np.uint32)
    elif inp == "two":
        a, b = (int(x) for x in rng.choice(np.arange(1, S >> 2), size=2, replace=False))
        raw = np.array([a, b, a | S, b | S], dtype=np.uint32)[rng.integers(0, 4, size=n)]
    elif inp == "clean":
        # magnitudes from 1 up to below the first all-ones exponent of any of the formats (e5m2 / f16: five exponent bits;
        # e4m3 / bf16: below 0x70 / 0x7000 is finite and no NaN in every reading)
        top = 0x70 if bits == 8 else 0x7000
        raw = rng.integers(1, top, size=n, dtype=np.uint32) | (rng.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(bits - 1))
    else:
        raise ValueError(inp)
    return raw.astype(utype(bits))


def row_ids(n, vb):
    """(n, vb) uint8 rows that hold the row index in their first bytes (stability is visible), or None"""
    if vb == 0:
        return None
    if vb == 1:
        return (np.arange(n, dtype=np.uint32) & 0xff).astype(np.uint8).reshape(n, 1)
    if vb == 2:
        return (np.arange(n, dtype=np.uint32) & 0xffff).astype(np.uint16).view(np.uint8).reshape(n, 2)
    if vb == 3:
        return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)[:, :3].copy()
    if vb == 4:
        return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    v = np.zeros((n, vb), dtype=np.uint8)
    v[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    v[:, 8:] = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(24)).astype(np.uint8)[:, None]
    return v
