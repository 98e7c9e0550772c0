"""GPU tests of gs_lsb_sort_narrow, straight through the C ABI: 8- and 16-bit keys (bool / u8 / i8 / u16 / i16) with no
values or values of 1, 2, 4, 8 and 16 bytes on the native kernels of gs_narrow.hip.

Every case has two witnesses.  The expectation is oracle.lsb_reference_ranks on the key's order-preserving u32 image (the
rule of tests/test_small_types_gpu.py): keys and values are compared bit for bit.  And gs_lsb_sort_any sorts the same input
into buffers of its own, which must come out byte for byte the same (a stable sort's result is unique).  Every case runs in
a guarded Arena (tests/guarded.py): keys, values and the workspace sit at chosen byte offsets, outputs and workspace are
pre-filled, and afterwards every guard byte must be intact and every input unchanged.

The three large cases are checked on the device in chunks of 2^28 elements at most (whole-tensor torch operations at these
sizes have returned wrong entries, tools/lsb_large_bench.py): per-value counts equal to the input's, keys in order, and for
the pairs case row ids ascending inside each key and the input key at each row id equal to the key that came out."""
import ctypes as C

import numpy as np
import pytest
import torch

from guarded import Arena, FILLS

pytestmark = pytest.mark.gpu

KEY_KINDS = {               # name -> (gs key type name, bits, signed)
    "bool": ("GS_KEY_U8", 8, False),
    "u8": ("GS_KEY_U8", 8, False),
    "i8": ("GS_KEY_I8", 8, True),
    "u16": ("GS_KEY_U16", 16, False),
    "i16": ("GS_KEY_I16", 16, True),
}
VAL_BYTES = (0, 1, 2, 4, 8, 16)
INPUTS = ("uniform", "and2", "equal", "two", "sorted", "reverse", "every")
INVALID = 1
CHUNK = 1 << 28


def _utype(bits):
    return np.uint8 if bits == 8 else np.uint16


def gen_keys(kind, n, inp, seed):
    """unsigned bit patterns of n keys"""
    bits = KEY_KINDS[kind][1]
    card = 2 if kind == "bool" else 1 << bits
    rng = np.random.default_rng(seed)
    if inp == "uniform":
        raw = rng.integers(0, card, size=n, dtype=np.uint32)
    elif inp == "and2":
        raw = rng.integers(0, 1 << bits, size=n, dtype=np.uint32) & rng.integers(0, 1 << bits, size=n, dtype=np.uint32)
        if kind == "bool":
            raw &= 1
    elif inp == "equal":
        raw = np.full(n, int(rng.integers(0, card)), dtype=np.uint32)
    elif inp == "two":
        a, b = (0, 1) if kind == "bool" else (int(x) for x in rng.choice(card, size=2, replace=False))
        raw = np.where(rng.integers(0, 2, size=n) == 1, a, b).astype(np.uint32)
    elif inp in ("sorted", "reverse"):
        raw = np.sort(rng.integers(0, card, size=n, dtype=np.uint32))
        if KEY_KINDS[kind][2]:                              # sorted as signed keys
            raw = np.sort(raw ^ np.uint32(1 << (bits - 1))) ^ np.uint32(1 << (bits - 1))
        if inp == "reverse":
            raw = raw[::-1].copy()
    elif inp == "every":                                    # every value of the type the same number of times (n a multiple of card)
        raw = rng.permutation(np.arange(n, dtype=np.uint32) % np.uint32(card))
    else:
        raise ValueError(inp)
    return raw.astype(_utype(bits))


def gen_vals(n, vb, seed):
    """(n, vb) uint8: row indices where the size allows (stability is visible), random bytes otherwise"""
    rng = np.random.default_rng(seed + 1)
    if vb == 0:
        return None
    if vb in (1, 2):
        return rng.integers(0, 256, size=(n, vb), dtype=np.uint8)
    if vb == 4:
        return np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    if vb == 8:
        return (np.arange(n, dtype=np.uint64) * np.uint64(0x100000001)).view(np.uint8).reshape(n, 8)
    v = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    v[:, :8] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    return v


def bit_ranges(bits):
    r = [(0, bits), (3, 3), (bits - 1, bits), (1, bits - 1)]
    if bits == 16:
        r += [(4, 12), (0, 8), (8, 16)]
    return r


def expected(oracle, kind, keys, vals, bb, eb, desc):
    _, bits, signed = KEY_KINDS[kind]
    img = keys.astype(np.uint32)
    if signed:
        img = img ^ np.uint32(1 << (bits - 1))
    ranks = oracle.lsb_reference_ranks(img, bb, eb, desc)
    return keys[ranks], (None if vals is None else vals[ranks])


def run_case(gs, cuda, oracle, kind, vb, n, bb, eb, desc, inp="and2", seed=1, koff=0, voff=0, wsoff=0, fill="ff", stream=None):
    ktname, bits, _ = KEY_KINDS[kind]
    kt = getattr(gs, ktname)
    kb = bits // 8
    keys = gen_keys(kind, n, inp, seed)
    vals = gen_vals(n, vb, seed)
    nb = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    assert nb > 0 and nb % 256 == 0
    A = Arena(cuda, seed=seed)
    A.add("kin", n * kb, koff, data=keys, const=True).add("kout", n * kb, koff, fill=fill)
    if vb:
        A.add("vin", n * vb, voff, data=vals, const=True).add("vout", n * vb, voff, fill=fill)
    A.add("ws", nb, wsoff, fill=fill)
    A.build()
    sp = C.c_void_p(stream.cuda_stream) if stream is not None else None
    err = gs.lib.gs_lsb_sort_narrow(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), A.ptr("vin") if vb else None,
                                    A.ptr("vout") if vb else None, n, kt, vb, bb, eb, int(desc), sp)
    tag = (kind, vb, n, bb, eb, desc, inp, koff, voff, wsoff, fill)
    assert err == 0, tag
    A.check()                                               # guards intact, inputs byte-identical
    ek, ev = expected(oracle, kind, keys, vals, bb, eb, desc)
    gk = A.read("kout", _utype(bits), n)
    assert np.array_equal(gk, ek), ("keys", tag, int(np.argmax(gk != ek)) if n else 0)
    if vb:
        gv = A.read("vout", np.uint8).reshape(n, vb)
        assert np.array_equal(gv, ev), ("values", tag, int(np.argmax((gv != ev).any(axis=1))) if n else 0)
    # the second witness: gs_lsb_sort_any on the same input
    if n:
        nba = gs.lib.gs_lsb_any_temp_bytes(n, kt, vb)
        wsa = torch.empty(nba, dtype=torch.uint8, device=cuda)
        tk = torch.from_numpy(keys.view(np.uint8).copy()).to(cuda)
        ok = torch.empty_like(tk)
        tv = ov = None
        if vb:
            tv = torch.from_numpy(vals.copy()).to(cuda)
            ov = torch.empty_like(tv)
        err = gs.lib.gs_lsb_sort_any(wsa.data_ptr(), nba, tk.data_ptr(), ok.data_ptr(), tv.data_ptr() if vb else None,
                                     ov.data_ptr() if vb else None, n, kt, vb, bb, eb, int(desc), None)
        assert err == 0, tag
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy().view(_utype(bits)), gk), ("keys differ from gs_lsb_sort_any", tag)
        if vb:
            assert np.array_equal(ov.cpu().numpy().reshape(n, vb), gv), ("values differ from gs_lsb_sort_any", tag)


def sizes_for(gs, kind, vb):
    tile = gs.lib.gs_lsb_narrow_tile(getattr(gs, KEY_KINDS[kind][0]), vb)
    assert tile > 0
    return [0, 1, 63, 64, 65, 777, tile - 1, tile, tile + 1]


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_sizes_ranges_directions(gs, cuda, oracle, kind, vb):
    """every small size and the sizes around one tile x every bit range x both directions; the input kind rotates"""
    bits = KEY_KINDS[kind][1]
    i = 0
    for n in sizes_for(gs, kind, vb):
        for bb, eb in bit_ranges(bits):
            for desc in (False, True):
                run_case(gs, cuda, oracle, kind, vb, n, bb, eb, desc, inp=INPUTS[i % 6], seed=100 + i)
                i += 1


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_100003(gs, cuda, oracle, kind, vb):
    bits = KEY_KINDS[kind][1]
    for i, (bb, eb) in enumerate(bit_ranges(bits)):
        run_case(gs, cuda, oracle, kind, vb, 100003, bb, eb, bool(i & 1), inp="and2", seed=7 + i)
        run_case(gs, cuda, oracle, kind, vb, 100003, bb, eb, not (i & 1), inp="uniform", seed=70 + i)


@pytest.mark.parametrize("inp", INPUTS)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_inputs(gs, cuda, oracle, kind, inp):
    """every input kind, keys only (the fill path for 8-bit keys), with row ids and with 16-byte records, 2 x 65536 elements
    (`every`: each value of the type exactly n / 256 or n / 65536 times) and 100003"""
    bits = KEY_KINDS[kind][1]
    for n in ((1 << 17), 100003):
        if inp == "every" and n % (1 << bits):
            continue
        for vb in (0, 4, 16):
            for desc in (False, True):
                run_case(gs, cuda, oracle, kind, vb, n, 0, bits, desc, inp=inp, seed=11)
                run_case(gs, cuda, oracle, kind, vb, n, 1, bits - 1, desc, inp=inp, seed=12)


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", list(KEY_KINDS))
def test_2p24_plus_7(gs, cuda, oracle, kind, vb):
    bits = KEY_KINDS[kind][1]
    desc = (vb in (1, 4, 16)) != (kind in ("i8", "u16"))
    run_case(gs, cuda, oracle, kind, vb, (1 << 24) + 7, 0, bits, desc, inp="uniform" if vb else "and2", seed=24)


def test_2p24_plus_7_other_paths(gs, cuda, oracle):
    n = (1 << 24) + 7
    run_case(gs, cuda, oracle, "u8", 0, n, 0, 8, False, inp="equal", seed=5)      # fill path, one bin
    run_case(gs, cuda, oracle, "u8", 0, n, 1, 8, True, inp="two", seed=6)         # digit pass, keys only
    run_case(gs, cuda, oracle, "i16", 0, n, 0, 16, False, inp="equal", seed=7)
    run_case(gs, cuda, oracle, "u16", 4, n, 4, 12, True, inp="every" if n % 65536 == 0 else "sorted", seed=8)
    run_case(gs, cuda, oracle, "i16", 8, n, 8, 16, False, inp="reverse", seed=9)


# ------------------------------------------------------------------------------------------------ buffer contract --
def _placements(elem):
    return (0, 1, 3, 7) if elem == 1 else (0, 2, 6) if elem == 2 else (0, elem)


@pytest.mark.parametrize("vb", VAL_BYTES)
@pytest.mark.parametrize("kind", ["u8", "i8", "u16", "i16"])
def test_buffer_contract(gs, cuda, oracle, kind, vb):
    """keys and values at every listed byte offset from a 256-byte boundary, the workspace 0, 1 and 255 bytes off, outputs and
    workspace pre-filled with each fill: result exact, guards intact, inputs untouched (run_case checks all three)"""
    bits = KEY_KINDS[kind][1]
    tile = gs.lib.gs_lsb_narrow_tile(getattr(gs, KEY_KINDS[kind][0]), vb)
    i = 0
    for koff in _placements(bits // 8):
        for voff in (_placements(vb) if vb else (0,)):
            for wsoff in (0, 1, 255):
                fill = FILLS[i % 3]
                n = 2 * tile + 1000 + 37 * i
                full = i % 2 == 0
                run_case(gs, cuda, oracle, kind, vb, n, 0 if full else 1, bits if full else bits - 1, bool(i & 2), inp="and2",
                         seed=300 + i, koff=koff, voff=voff, wsoff=wsoff, fill=fill)
                i += 1
    for fill in FILLS:              # each fill at least once on the plain placement, both paths
        run_case(gs, cuda, oracle, kind, vb, tile + 5, 0, bits, False, seed=400, fill=fill)
        run_case(gs, cuda, oracle, kind, vb, tile + 5, 2, bits, True, seed=401, fill=fill, koff=bits // 8, wsoff=255)


@pytest.mark.parametrize("kind,vb", [("u8", 0), ("u8", 4), ("u16", 2), ("i16", 16)])
def test_refused_call_writes_nothing(gs, cuda, kind, vb):
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n = getattr(gs, ktname), bits // 8, 5000
    nb = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    for fill in FILLS:
        A = Arena(cuda, seed=3, all_const=True)
        A.add("kin", n * kb, 0, data=gen_keys(kind, n, "uniform", 1)).add("kout", n * kb, 0, fill=fill)
        if vb:
            A.add("vin", n * vb, 0, data=gen_vals(n, vb, 1)).add("vout", n * vb, 0, fill=fill)
        A.add("ws", nb, 1, fill=fill)
        A.build()
        f = gs.lib.gs_lsb_sort_narrow
        vi, vo = (A.ptr("vin"), A.ptr("vout")) if vb else (None, None)
        assert f(A.ptr("ws"), nb - 1, A.ptr("kin"), A.ptr("kout"), vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(None, nb, A.ptr("kin"), A.ptr("kout"), vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, vo, n, kt, vb, 0, bits + 1, 0, None) == INVALID
        assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, vo, n, kt, vb, 3, 2, 0, None) == INVALID
        assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kin"), vi, vo, n, kt, vb, 0, bits, 0, None) == INVALID
        assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, vo, n, kt, 3, 0, bits, 0, None) == INVALID
        assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, vo, n, gs.GS_KEY_U32, vb, 0, 8, 0, None) == INVALID
        if vb:
            assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, None, n, kt, vb, 0, bits, 0, None) == INVALID
            assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi, vi, n, kt, vb, 0, bits, 0, None) == INVALID
        else:
            assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), A.ptr("kin"), A.ptr("kout"), n, kt, 0, 0, bits, 0, None) == INVALID
        if kb == 2:
            assert f(A.ptr("ws"), nb, A.ptr("kin") + 1, A.ptr("kout"), vi, vo, n - 1, kt, vb, 0, bits, 0, None) == INVALID
        if vb == 16:
            assert f(A.ptr("ws"), nb, A.ptr("kin"), A.ptr("kout"), vi + 8, vo, n - 1, kt, vb, 0, bits, 0, None) == INVALID
        A.check()


@pytest.mark.parametrize("kind,vb", [("u8", 0), ("i8", 4), ("u16", 0), ("i16", 8), ("u8", 1)])
def test_one_workspace_two_sorts_back_to_back(gs, cuda, oracle, kind, vb):
    """two sorts of different inputs follow each other on a non-default stream with one workspace and no synchronisation"""
    ktname, bits, _ = KEY_KINDS[kind]
    kt, kb, n = getattr(gs, ktname), bits // 8, 300007
    nb = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    ins, outs = [], []
    for j in range(2):
        keys, vals = gen_keys(kind, n, ("uniform", "and2")[j], 50 + j), gen_vals(n, vb, 60 + j)
        tk = torch.from_numpy(keys.view(np.uint8).copy()).to(cuda)
        tv = torch.from_numpy(vals.copy()).to(cuda) if vb else None
        ins.append((keys, vals, tk, tv))
        outs.append((torch.empty_like(tk), torch.empty_like(tv) if vb else None))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=cuda)
    for j in range(2):
        (_, _, tk, tv), (ok, ov) = ins[j], outs[j]
        err = gs.lib.gs_lsb_sort_narrow(ws.data_ptr(), nb, tk.data_ptr(), ok.data_ptr(), tv.data_ptr() if vb else None,
                                        ov.data_ptr() if vb else None, n, kt, vb, 0, bits, j, C.c_void_p(stream.cuda_stream))
        assert err == 0
    stream.synchronize()
    for j in range(2):
        ek, ev = expected(oracle, kind, ins[j][0], ins[j][1], 0, bits, bool(j))
        assert np.array_equal(outs[j][0].cpu().numpy().view(_utype(bits)), ek), (kind, vb, j)
        if vb:
            assert np.array_equal(outs[j][1].cpu().numpy().reshape(n, vb), ev), (kind, vb, j)


# ---------------------------------------------------------------------------------------------------- large cases --
def _chunks(n):
    return [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]


def _fill_random(t, card, seed):
    g = torch.Generator(device=t.device)
    g.manual_seed(seed)
    for lo, hi in _chunks(t.numel()):
        t[lo:hi] = torch.randint(0, card, (hi - lo,), device=t.device, generator=g, dtype=torch.int32).to(t.dtype)


def _counts(t, card, offset):
    c = torch.zeros(card, dtype=torch.int64, device=t.device)
    for lo, hi in _chunks(t.numel()):
        c += torch.bincount(t[lo:hi].to(torch.int64) + offset, minlength=card)
    return c


def _assert_ascending(t):
    for lo, hi in _chunks(t.numel()):
        s = t[max(lo - 1, 0):hi]
        assert bool((s[1:] >= s[:-1]).all()), "keys out of order in chunk at %d" % lo


def _any_witness(gs, cuda, kt, vb, kin, vin, kout, vout, n, bits):
    nba = gs.lib.gs_lsb_any_temp_bytes(n, kt, vb)
    wsa = torch.empty(nba, dtype=torch.uint8, device=cuda)
    ok = torch.empty_like(kin)
    ov = torch.empty_like(vin) if vb else None
    err = gs.lib.gs_lsb_sort_any(wsa.data_ptr(), nba, kin.data_ptr(), ok.data_ptr(), vin.data_ptr() if vb else None,
                                 ov.data_ptr() if vb else None, n, kt, vb, 0, bits, 0, None)
    assert err == 0
    torch.cuda.synchronize()
    del wsa
    for lo, hi in _chunks(n):
        assert torch.equal(ok[lo:hi], kout[lo:hi]), "keys differ from gs_lsb_sort_any in chunk at %d" % lo
        if vb:
            assert torch.equal(ov[lo:hi], vout[lo:hi]), "values differ from gs_lsb_sort_any in chunk at %d" % lo


def _sort_large(gs, cuda, kt, vb, kin, vin, n, bits):
    nb = gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=cuda)
    kout = torch.empty_like(kin)
    vout = torch.empty_like(vin) if vb else None
    keep = kin[: 1 << 20].clone()
    err = gs.lib.gs_lsb_sort_narrow(ws.data_ptr(), nb, kin.data_ptr(), kout.data_ptr(), vin.data_ptr() if vb else None,
                                    vout.data_ptr() if vb else None, n, kt, vb, 0, bits, 0, None)
    assert err == 0
    torch.cuda.synchronize()
    assert torch.equal(keep, kin[: 1 << 20])
    return kout, vout


def test_large_u8_keys_2p32_minus_1(gs, cuda):
    n = (1 << 32) - 1
    kin = torch.empty(n, dtype=torch.uint8, device=cuda)
    _fill_random(kin, 256, 1)
    kout, _ = _sort_large(gs, cuda, gs.GS_KEY_U8, 0, kin, None, n, 8)
    assert torch.equal(_counts(kin, 256, 0), _counts(kout, 256, 0))
    _assert_ascending(kout)
    _any_witness(gs, cuda, gs.GS_KEY_U8, 0, kin, None, kout, None, n, 8)


def test_large_i16_keys_2p31_plus_12345(gs, cuda):
    n = (1 << 31) + 12345
    kin = torch.empty(n, dtype=torch.int16, device=cuda)
    _fill_random(kin, 65536, 2)             # (the conversion wraps: every bit pattern)
    kout, _ = _sort_large(gs, cuda, gs.GS_KEY_I16, 0, kin, None, n, 16)
    assert torch.equal(_counts(kin, 65536, 32768), _counts(kout, 65536, 32768))
    _assert_ascending(kout)
    _any_witness(gs, cuda, gs.GS_KEY_I16, 0, kin, None, kout, None, n, 16)


def test_large_u8_u64_pairs_2p29_plus_4099(gs, cuda):
    """the value byte offsets pass 2^32"""
    n = (1 << 29) + 4099
    kin = torch.empty(n, dtype=torch.uint8, device=cuda)
    _fill_random(kin, 256, 3)
    vin = torch.empty(n, dtype=torch.int64, device=cuda)
    for lo, hi in _chunks(n):
        vin[lo:hi] = torch.arange(lo, hi, dtype=torch.int64, device=cuda)
    kout, vout = _sort_large(gs, cuda, gs.GS_KEY_U8, 8, kin, vin, n, 8)
    assert torch.equal(_counts(kin, 256, 0), _counts(kout, 256, 0))
    _assert_ascending(kout)
    for lo, hi in _chunks(n):
        a = max(lo - 1, 0)
        k, v = kout[a:hi], vout[a:hi]
        assert bool(((k[1:] > k[:-1]) | (v[1:] > v[:-1])).all()), "row ids do not ascend inside a key, chunk at %d" % lo
        v = vout[lo:hi]
        assert bool(((v >= 0) & (v < n)).all())
        assert torch.equal(kin[v], kout[lo:hi]), "key at a row id differs, chunk at %d" % lo
    _any_witness(gs, cuda, gs.GS_KEY_U8, 8, kin, vin, kout, vout, n, 8)
