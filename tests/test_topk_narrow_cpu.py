"""gs_topk_u16 without a device: the numpy reference against tests/topk_ref.py on the widened keys (the identity of the
header), the builders of tests/topk_narrow_ref.py held to their intent, the workspace query against the header's formula,
every refusal and no-op of the contract, and the argument checks of DeviceTopK16 / topk()."""
import numpy as np
import pytest

import topk_ref as R
import topk_narrow_ref as N

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U16, I16, F16, BF16 = N.U16, N.I16, N.F16, N.BF16


# ------------------------------------------------------------------------------------------------ the reference --
@pytest.mark.parametrize("kt", N.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_ref16_is_the_32_bit_reference_on_the_widened_keys(kt, descending):
    """Forty seeded inputs per type and direction, heavy with ties (nine distributions, the special patterns among them):
    keys shifted back, indices and values equal, the status words those of the 32-bit reference with the image shifted."""
    rng = np.random.default_rng(100 * kt + descending)
    for j in range(40):
        kind = N.DISTS[j % len(N.DISTS)]
        n = int(rng.integers(1, 3000))
        keys = N.gen16(kind, n, seed=j + 1, kt=kt)
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        narrow, wide = N.Ref16(keys, kt, descending, vals), R.Ref(N.widen(keys), N.WIDE[kt], descending, vals)
        args = N.Ref16(keys, kt, descending)
        assert np.array_equal(narrow.order, wide.order)
        for k in sorted({1, n, (n + 1) // 2, int(rng.integers(1, n + 1))}):
            gk, gv, st = narrow.topk(k)
            wk, wv, wst = wide.topk(k)
            what = (kind, n, k)
            assert gk.dtype == np.uint16 and np.array_equal(gk, (wk >> np.uint32(16)).astype(np.uint16)), what
            assert (wk & np.uint32(0xFFFF) == 0).all() and np.array_equal(gv, wv), what
            assert np.array_equal(args.topk(k)[1], wide.order[:k]), what
            # the widened image is the 16-bit one in the upper half (the lower half is a function of the upper one)
            assert wst[0] >> 16 == st[0], what
            assert st[1:3] == wst[1:3] and st[3] == wst[3], what
            assert st[1] + st[2] == k and 0 < st[2] and st[3] >= st[2], what


def test_builders_hold_their_intent():
    for kt, desc in ((U16, False), (BF16, True), (I16, True), (F16, False)):
        for n, c in ((70001, 65536), (70001, 65537)):
            below = 2000
            ref = N.Ref16(N.bucket_case16(n, c, below, 0x42, 7, kt, desc), kt, desc)
            assert ref.tops[0x42] == c and ref.tops[:0x42].sum() == below
            for k, inside in N.bucket_ks(below, c):
                assert ref.route(k) == (2 if inside and c > 65536 else 1), (n, c, k)
                assert (ref.topk(k)[2][0] >> 8 == 0x42) == inside
        for route, top in ((1, 0x00), (2, 0x00), (2, 0xFF)):
            ref = N.Ref16(N.digit_edge_case16(route, top, kt, desc), kt, desc)
            assert sorted(set(ref.img.tolist())) == N.IMAGES12
            routes = {ref.route(k) for k in N.run_cuts(ref)}
            assert routes == ({1, 2} if route == 2 else {1})
            assert ref.route(1) == (2 if route == 2 and top == 0 else 1) and ref.route(ref.keys.size) == (2 if top == 0xFF and route == 2 else 1)
    ref = N.Ref16(N.gen16("uniform", 30000, seed=3), U16)
    cuts = N.bucket_cuts(ref)
    assert cuts[0] == 1 and cuts[-1] == 30000 and all(ref.topk(k)[2][1] + ref.topk(k)[2][2] == k for k in cuts[:8])
    assert N.Ref16(np.zeros(8192, np.uint16), U16).route(5) == 3 and N.Ref16(np.zeros(8193, np.uint16), U16).route(5) == 1


# --------------------------------------------------------------------------------------------- the size query --
SIZES = [1, 2, 8191, 8192, 8193, 65536, 65537, 100003, 1 << 21, (1 << 21) + 1, 1 << 24, (1 << 30) + 7, (1 << 32) - 1]


def test_temp_bytes_is_the_headers_formula_a_multiple_of_256_and_monotone(gs):
    lib = gs.lib
    for hv in (0, 1):
        last_n = 0
        for n in SIZES:
            ks = sorted(k for k in {1, 2, 1000, 8192, 8193, 65536, 65537, n // 2 + 1, n} if 1 <= k <= n)
            last_k = 0
            for k in ks:
                got = lib.gs_topk_u16_temp_bytes(n, k, hv)
                sort_ws = lib.gs_lsb_narrow_temp_bytes(k, U16, 4 if hv else 0)
                assert sort_ws == N.narrow_temp_bytes(k, hv), (k, hv)
                assert got == N.temp_bytes16(n, k, hv, sort_ws) and got % 256 == 0 and got > 0, (n, k, hv)
                assert got >= last_k, (n, k, hv)
                last_k = got
            at_one = lib.gs_topk_u16_temp_bytes(n, 1, hv)
            assert at_one >= last_n, (n, hv)
            last_n = at_one
            assert lib.gs_topk_u16_temp_bytes(n, 0, hv) == 0
        assert lib.gs_topk_u16_temp_bytes(0, 0, hv) == 0
    # monotone in n at a fixed k, across the tile and capacity edges
    for k in (1, 5000):
        sizes = [n for n in SIZES if n >= k]
        got = [lib.gs_topk_u16_temp_bytes(n, k, 1) for n in sizes]
        assert got == sorted(got)
    # 2 B per candidate and staged key where the 32-bit query has 4
    n, k = 1 << 24, 1 << 16
    assert lib.gs_topk_u16_temp_bytes(n, k, 0) < lib.gs_topk_temp_bytes(n, k, 0)
    assert lib.gs_topk_u16_temp_bytes(n, k, 1) < lib.gs_topk_temp_bytes(n, k, 1)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def al4(x):
    return x & ~3       # the 4-byte word that holds byte x


def _call(gs, temp, temp_bytes, kin, vin, kout, vout, n, k, desc=0, kt=U16):
    return gs.lib.gs_topk_u16(temp, temp_bytes, kin, vin, kout, vout, n, k, desc, kt, None)


@pytest.mark.parametrize("n", [5000, 100003])
def test_refusals_and_noops_without_a_device(gs, n):
    k = 100
    need = gs.lib.gs_topk_u16_temp_bytes(n, k, 1)
    assert need > 0
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 26), BASE + (2 << 26), BASE + (3 << 26), BASE + (4 << 26)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, n=n, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0), # too small
        dict(k=n + 1),                                 # k > num_items
        dict(n=1 << 32), dict(n=1 << 32, k=1 << 32), dict(n=(1 << 40) + 5),       # num_items >= 2^32
        dict(kt=0), dict(kt=1), dict(kt=2),            # 32-bit key types
        dict(kt=3), dict(kt=4), dict(kt=5),            # 64-bit key types
        dict(kt=6), dict(kt=7), dict(kt=12), dict(kt=13), dict(kt=-1),   # 8-bit key types and no type at all
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 1), dict(kout=kout + 1), dict(kin=kin + 3),       # a key pointer at an odd byte address
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 1), dict(vout=vout + 3),   # a value pointer that is not 4-aligned
        dict(kout=kin), dict(kout=kin + 2 * (n - 1)),  # output inside the keys (2-byte key extents)
        dict(vout=kin + al4(2 * n - 1)), dict(vout=vin), dict(kout=vin + 4 * n - 2),
        dict(vout=kout), dict(vout=kout + al4(2 * k - 1)), dict(kout=vout + 4 * k - 2),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + al4(2 * n - 1)),  # inputs share a byte
    ]
    for change in bad:
        assert _call(gs, **dict(ok, **change)) == INVALID, change
    # the arguments and keys-only forms size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_u16_temp_bytes(n, k, 0)
    assert 0 < need0 < need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed
    for kt in N.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, n, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, n, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, 0, 1) == INVALID             # k > num_items, even for an empty array
    assert _call(gs, None, 0, None, None, None, None, n, 0, 0, 2) == INVALID       # a bad key type before the no-op
    assert _call(gs, None, 0, None, vin, None, None, n, 0) == INVALID              # values in without values out, before the no-op


def test_status_of_a_noop_and_its_refusals(gs):
    import ctypes as C
    st = (C.c_uint32 * 8)(*([7] * 8))
    assert gs.lib.gs_topk_u16_status(None, 1000, 0, 0, st, None) == 0 and list(st) == [0] * 8
    st = (C.c_uint32 * 8)(*([7] * 8))
    assert gs.lib.gs_topk_u16_status(None, 0, 0, 1, st, None) == 0 and list(st) == [0] * 8
    assert gs.lib.gs_topk_u16_status(None, 1000, 10, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u16_status(BASE, 10, 11, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u16_status(BASE, 1 << 32, 10, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u16_status(BASE, 1000, 10, 0, None, None) == INVALID


# ------------------------------------------------------------------------------------------------ front ends --
def test_front_end_argument_checks_need_no_device(gs):
    import torch
    assert gs.DeviceTopK16 is not gs.DeviceTopK
    for hv, form in ((0, gs.DeviceTopK16.MinKeys), (0, gs.DeviceTopK16.MaxKeys)):
        assert form(None, 0, None, None, 100003, 77) == gs.lib.gs_topk_u16_temp_bytes(100003, 77, hv)
    for form in (gs.DeviceTopK16.MinPairs, gs.DeviceTopK16.MaxPairs):
        assert form(None, 0, None, None, None, None, 100003, 77) == gs.lib.gs_topk_u16_temp_bytes(100003, 77, 1)
        for kt in N.KEY_TYPES:
            assert form(None, 0, None, None, None, None, 100003, 77, key_type=kt) == gs.lib.gs_topk_u16_temp_bytes(100003, 77, 1)
        for kt in (gs.GS_KEY_U32, gs.GS_KEY_F32, gs.GS_KEY_U64, gs.GS_KEY_U8, gs.GS_KEY_F8):
            with pytest.raises(TypeError):
                form(None, 0, None, None, None, None, 100003, 77, key_type=kt)
    tmp = torch.zeros(256, dtype=torch.uint8)
    for dtype in (torch.int32, torch.float32, torch.int64, torch.int8):
        x = torch.zeros(10, dtype=dtype)
        with pytest.raises(TypeError):
            gs.DeviceTopK16.MinKeys(tmp, 256, x, x.clone(), 10, 2)
    x16 = torch.zeros(10, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        gs.DeviceTopK16.MinKeys(tmp, 256, x16, x16.clone(), 10, 2)               # not a device tensor
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        t = torch.zeros(10, dtype=dtype)
        with pytest.raises(ValueError):
            gs.topk(t, 11)
        with pytest.raises(ValueError):
            gs.topk(t, 2, values=torch.zeros(10, dtype=torch.int32), indices=True)
        ko, vo = gs.topk(t, 0, indices=True)
        assert ko.numel() == 0 and ko.dtype == dtype and vo.numel() == 0 and vo.dtype == torch.int32
        ko, vo = gs.topk(t, 0)
        assert ko.dtype == dtype and vo is None
