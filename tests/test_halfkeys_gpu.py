"""GPU tests of the plain sorts on the float key categories of 8 and 16 bits (GS_KEY_F16 / GS_KEY_BF16 / GS_KEY_F8), straight
through the C ABI: gs_lsb_sort_narrow with values of 0, 1, 2, 4, 8 and 16 bytes and gs_lsb_sort_any for other value sizes.

Every expectation is computed here with numpy (tests/halfkeys_ref.py): the image np.where(b & S, b ^ ALL, b ^ S), the digit
[begin_bit, end_bit) of it, complemented when descending, np.argsort(kind="stable").  Keys and values must match bit for
bit; the values hold row ids, so stability is visible.  Every case runs in a guarded Arena (tests/guarded.py): the inputs
must come out unchanged and nothing outside the outputs and the workspace may be written."""
import numpy as np
import pytest
import torch

import halfkeys_ref as R
from guarded import Arena, FILLS

pytestmark = pytest.mark.gpu

KINDS = list(R.KINDS)
INPUTS = ("every", "uniform", "equal", "two")


def ranges(bits):
    """all bits, [0, 8), [8, 16), [3, 13), [5, 5) -- those that fit the width (8-bit keys: all bits, [3, 7), [5, 5))"""
    return [(0, 16), (0, 8), (8, 16), (3, 13), (5, 5)] if bits == 16 else [(0, 8), (3, 7), (5, 5)]


def run_case(gs, cuda, kind, vb, n, bb, eb, desc, inp="uniform", seed=1, koff=0, voff=0, wsoff=0, fill="ff", keys=None,
             fn="gs_lsb_sort_narrow"):
    ktname, _, bits = R.KINDS[kind]
    kt, kb = getattr(gs, ktname), bits // 8
    if keys is None:
        keys = R.gen_bits(kind, n, inp, seed)
    vals = R.row_ids(n, vb)
    nb = getattr(gs.lib, fn.replace("sort_", "") + "_temp_bytes")(n, kt, vb)
    assert nb > 0
    A = Arena(cuda, seed=seed)
    A.add("kin", n * kb, koff, data=keys, const=True).add("kout", n * kb, koff, fill=fill)
    if vb:
        A.add("vin", n * vb, voff, data=vals, const=True).add("vout", n * vb, voff, fill=fill)
    A.add("ws", nb, wsoff, fill=fill)
    A.build()
    err = getattr(gs.lib, fn)(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if vb else None,
                              A.ptr("vout") if vb else None, n, kt, vb, bb, eb, int(desc), None)
    tag = (fn, kind, vb, n, bb, eb, desc, inp, koff, voff, wsoff, fill)
    assert err == 0, tag
    A.check()                                               # guards intact, inputs byte-identical
    o = R.order(keys, bits, bb, eb, desc)
    gk = A.read("kout", R.utype(bits), n)
    assert np.array_equal(gk, keys[o]), ("keys", tag, int(np.argmax(gk != keys[o])))
    if vb:
        gv = A.read("vout", np.uint8).reshape(n, vb)
        assert np.array_equal(gv, vals[o]), ("values", tag, int(np.argmax((gv != vals[o]).any(axis=1))))
    return gk, o


@pytest.mark.parametrize("vb", (0, 1, 2, 4, 8, 16))
@pytest.mark.parametrize("kind", KINDS)
def test_size_sweep_every_value_size(gs, cuda, kind, vb):
    """1, 2, T - 1, T, T + 1, 3T + 5 and 100003 elements with every value size; ranges, directions and inputs rotate"""
    ktname, _, bits = R.KINDS[kind]
    T = gs.lib.gs_lsb_narrow_tile(getattr(gs, ktname), vb)
    assert T > 0
    rs = ranges(bits)
    i = 0
    for n in (1, 2, T - 1, T, T + 1, 3 * T + 5, 100003):
        for desc in (False, True):
            bb, eb = rs[i % len(rs)]
            run_case(gs, cuda, kind, vb, n, bb, eb, desc, inp=INPUTS[i % 4], seed=10 + i)
            run_case(gs, cuda, kind, vb, n, 0, bits, not desc, inp=INPUTS[(i + 1) % 4], seed=50 + i)
            i += 1


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_ranges_directions_inputs(gs, cuda, kind, inp):
    """every bit range x both directions x every input, keys alone, with row ids and with 16-byte records; `every` holds each
    of the 65536 or 256 patterns several times (both zeros, both infinities, NaNs of both signs), shuffled"""
    bits = R.KINDS[kind][2]
    n = 3 * 65536 if bits == 16 else 80 * 256
    for vb in (0, 4, 16):
        for bb, eb in ranges(bits):
            for desc in (False, True):
                run_case(gs, cuda, kind, vb, n, bb, eb, desc, inp=inp, seed=3 + vb)


@pytest.mark.parametrize("desc", (False, True))
def test_f8_fill_sizes_and_offsets(gs, cuda, desc):
    """8-bit float keys alone over all bits (the histogram and fill): small sizes around one 16-byte chunk, key arrays that
    start 1, 2 and 3 bytes off a 16-byte boundary"""
    i = 0
    for n in (1, 15, 16, 17, 4099, 100003):
        for koff in (1, 2, 3):
            run_case(gs, cuda, "f8", 0, n, 0, 8, desc, inp=INPUTS[i % 4], seed=200 + i, koff=koff, fill=FILLS[i % 3])
            i += 1
    run_case(gs, cuda, "f8", 0, 100003, 0, 8, desc, inp="every", seed=9, koff=3)


def _as_float(kind, bits_arr):
    """the values of finite bit patterns as float32 (exact: every one of these formats is a subset of float32)"""
    if kind == "f16":
        return torch.from_numpy(bits_arr.view(np.int16).copy()).view(torch.float16).float()
    if kind == "bf16":
        return torch.from_numpy(bits_arr.view(np.int16).copy()).view(torch.bfloat16).float()
    # an e5m2 byte is the top byte of the half with the same value (the clean magnitudes are finite in e4m3 as well, and the
    # image is monotone in the byte whichever 8-bit format reads it)
    return torch.from_numpy((bits_arr.astype(np.uint16) << np.uint16(8)).view(np.int16).copy()).view(torch.float16).float()


@pytest.mark.parametrize("kind", KINDS)
def test_clean_values_match_torch_sort(gs, cuda, kind):
    """no NaN, no infinity, no zero: there the order of the category is torch.sort's; values and indices of a stable
    torch.sort on the CPU must be the keys and the row ids that come out, ascending and descending"""
    bits = R.KINDS[kind][2]
    n = 100003
    keys = R.gen_bits(kind, n, "clean", 5)
    f = _as_float(kind, keys)
    assert bool(torch.isfinite(f).all()) and bool((f != 0).all())
    for desc in (False, True):
        gk, o = run_case(gs, cuda, kind, 4, n, 0, bits, desc, keys=keys, inp="clean")
        tv, ti = torch.sort(f, stable=True, descending=desc)
        assert np.array_equal(ti.numpy(), o), (kind, desc)
        assert torch.equal(_as_float(kind, gk), tv), (kind, desc)


@pytest.mark.parametrize("kind", KINDS)
def test_buffer_contract_pairs(gs, cuda, kind):
    """one pairs case per kind at odd placements with each fill: inputs untouched, nothing outside outputs and workspace"""
    ktname, _, bits = R.KINDS[kind]
    kb = bits // 8
    T = gs.lib.gs_lsb_narrow_tile(getattr(gs, ktname), 4)
    for i, (koff, voff, wsoff) in enumerate(((kb, 4, 1), (3 * kb, 0, 255), (0, 4, 77))):
        run_case(gs, cuda, kind, 4, 2 * T + 1000 + 37 * i, 0, bits, bool(i & 1), inp="uniform", seed=300 + i, koff=koff, voff=voff,
                 wsoff=wsoff, fill=FILLS[i])
        run_case(gs, cuda, kind, 8, T + 5, 1, bits - 1, not (i & 1), inp="every", seed=310 + i, koff=koff, voff=8, wsoff=wsoff,
                 fill=FILLS[i])


@pytest.mark.parametrize("vb", (3, 32))
def test_any_other_value_sizes(gs, cuda, vb):
    """gs_lsb_sort_any: half keys with values of 3 and 32 bytes (prepare maps the key, the gather moves the caller's bits)"""
    for desc in (False, True):
        for bb, eb in ((0, 16), (3, 13)):
            run_case(gs, cuda, "f16", vb, 5000, bb, eb, desc, inp="every", seed=vb, fn="gs_lsb_sort_any")
    run_case(gs, cuda, "f16", 0, 5000, 0, 16, True, inp="every", seed=1, fn="gs_lsb_sort_any")      # narrow-back undoes the map
    run_case(gs, cuda, "f8", 0, 5000, 0, 8, False, inp="every", seed=2, fn="gs_lsb_sort_any")
    run_case(gs, cuda, "bf16", vb, 5000, 0, 16, False, inp="two", seed=3, fn="gs_lsb_sort_any")
