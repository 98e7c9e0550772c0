"""gs_topk_u64 without a device: the numpy reference against tests/topk_ref.py on keys whose low 32 bits are zero, the builders
of tests/topk_wide_ref.py held to their intent (D and route included), the workspace query against the header's formula, every
refusal and no-op of the contract, and the argument checks of DeviceTopK64 / topk()."""
import numpy as np
import pytest

import topk_ref as R
import topk_wide_ref as W

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U64, I64, F64 = W.U64, W.I64, W.F64
NARROW = {U64: R.U32, I64: R.I32, F64: R.F32}


# ------------------------------------------------------------------------------------------------ the reference --
@pytest.mark.parametrize("kt", W.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_ref64_is_the_32_bit_reference_on_keys_with_zero_low_words(kt, descending):
    """(uint64_t)key << 32 with the key type widened: the same order, the keys shifted back, indices and values equal, the
    high word of the k-th image and the count before it those of the 32-bit reference."""
    rng = np.random.default_rng(100 * kt + descending)
    special = np.array([0, 0x80000000, 0x7FC00001, 0xFFC00001, 0x7F800000, 0xFF800000, 1, 0x80000001, 0xFFFFFFFF], np.uint32)
    for j in range(30):
        n = int(rng.integers(1, 3000))
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        if j % 3 == 1:
            keys = np.where(rng.random(n) < 0.6, special[rng.integers(0, special.size, n)], keys)
        elif j % 3 == 2:
            keys = keys & np.uint32(0xC0000003)
        vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        wide_keys = keys.astype(np.uint64) << np.uint64(32)
        wide, narrow = W.Ref64(wide_keys, kt, descending, vals), R.Ref(keys, NARROW[kt], descending, vals)
        assert np.array_equal(wide.order, narrow.order)
        assert np.array_equal(W.preimage(wide.img, kt, descending), wide_keys)
        for k in sorted({1, n, (n + 1) // 2, int(rng.integers(1, n + 1))}):
            gk, gv = wide.topk(k)
            nk, nv, nst = narrow.topk(k)
            st = wide.status(k)
            assert gk.dtype == np.uint64 and np.array_equal((gk >> np.uint64(32)).astype(np.uint32), nk), (n, k)
            assert np.array_equal(gv, nv) and np.array_equal(W.Ref64(wide_keys, kt, descending).topk(k)[1], narrow.order[:k])
            assert st[2] == nst[0] and st[1] in (0, 0xFFFFFFFF), (n, k)       # (the low word: zeros, complemented or not)
            assert st[3] == nst[1] and st[4] == nst[2] and st[3] + st[4] == k
            assert st[0] == 1 and st[5] == 1 and st[6] == 2 and st[7] == nst[3]       # n <= C: always fits at D = 1


def test_image_orders_of_the_three_key_types():
    f = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 5e-324, -5e-324]).view(np.uint64)
    f[0], f[1] = 0x7FF8000000000001, 0xFFF8000000000001
    asc = W.Ref64(f, F64).topk(10)[0].tolist()
    assert asc == [f[i] for i in (1, 5, 7, 9, 3, 2, 8, 6, 4, 0)]
    assert W.Ref64(f, F64, True).topk(10)[0].tolist() == asc[::-1]
    i = np.array([0, -1, 1, -(1 << 63), (1 << 63) - 1], np.int64)
    assert W.Ref64(i, I64).topk(5)[0].view(np.int64).tolist() == sorted(i.tolist())
    assert W.Ref64(i, U64).topk(5)[0].tolist() == sorted(i.view(np.uint64).tolist())


# -------------------------------------------------------------------------------------------------- the builders --
def test_the_descent_table_of_the_issue():
    """n = 2^22 as in the table is minutes of numpy; 2^20 keeps every row's D (C = 65536 there too)."""
    n = 1 << 20
    ks = (1 << 10, 1 << 16, 1 << 18)
    assert [W.descent(W.image(W.gen64("uniform", n, 1), U64), k)[:2] for k in ks] == [(1, 1)] * 3
    small = W.small_ints(n, 2)
    assert [W.descent(W.image(small, I64), k)[:2] for k in ks] == [(1, 2)] * 3
    assert [W.descent(W.image(W.small_ints(n, 2, outlier=True), I64), k)[:2] for k in ks] == [(1, 3)] * 3
    # a day spans 2^46.3 ns: bytes 7 and 6 are skipped unless the day crosses a multiple of 2^48, so D is 2 or 3
    assert all(W.descent(W.image(W.timestamps(n, 3), I64, True), k)[:2] in ((1, 2), (1, 3)) for k in ks)
    for desc in (False, True):
        for k in ks:
            route, D, passes, _ = W.descent(W.image(W.gen64("normal", n, 4), F64, desc), k)
            assert route == 1 and D in (1, 2) and passes == (2 if D == 1 else D + 2)
    assert W.descent(W.image(np.full(n, 77, np.uint64), U64), 5) == (2, 1, 2, n)
    assert W.descent(W.image(np.full(65536, 77, np.uint64), U64), 5) == (1, 1, 2, 65536)


def test_builders_hold_their_intent():
    for kt, desc in ((U64, False), (F64, True), (I64, True)):
        for n, cap in ((70001, 65536), ((1 << 21) + 3 * 4096 + 1, ((1 << 21) + 3 * 4096 + 1) // 32)):
            if n > 100000 and kt != I64:
                continue
            assert W.cap(n) == cap
            for c in (cap, cap + 1):
                ref = W.Ref64(W.bucket_case64(n, c, 2000, 0x42, 7, kt, desc), kt, desc)
                tops = np.bincount(W.byte_of(ref.img, 7), minlength=256)
                assert tops[0x42] == c and tops[:0x42].sum() == 2000
                for k, inside in W.bucket_ks(2000, c):
                    st = ref.status(k)
                    assert st[0] == 1 and st[5] == (2 if inside and c > cap else 1), (n, c, k, st)
                    assert (st[2] >> 24 == 0x42) == inside and st[6] == (2 if st[5] == 1 else 4)
        # the skip: D = 2 without an outlier, 3 with one
        n = 70001
        assert W.Ref64(W.small_ints(n, 5), I64, desc).status(1000)[:1] + W.Ref64(W.small_ints(n, 5), I64, desc).status(1000)[5:7] == [1, 2, 4]
        assert W.Ref64(W.small_ints(n, 5, True), I64, desc).status(1000)[5:7] == [3, 5]
        # D = 8
        ref = W.Ref64(W.deep_case64(kt, desc), kt, desc)
        assert ref.keys.size == 65544
        st = ref.status(30000)
        assert st[0] == 1 and st[5:] == [8, 10, 32769 if st[1] & 0xFF == 0x10 else 32768], st
        assert {ref.status(k)[5] for k in range(1, 9)} | {ref.status(ref.keys.size - j)[5] for j in range(8)} >= {2, 3, 4, 5, 6, 7, 8}
        # route 2: the tie run holds the cut, and does not
        ref = W.Ref64(W.tie_case64(100003, 65537, 9, kt, desc), kt, desc)
        less = int((ref.img < np.uint64(0x8000000000000001)).sum())
        assert ref.status(less + 5)[0] == 2 and ref.status(less + 5)[7] == 65537 and ref.status(less + 5)[5] >= 2
        assert ref.status(less + 65537)[0] == 2 and ref.status(less)[0] == 1 and ref.status(less + 65538)[0] == 1
        assert W.Ref64(W.tie_case64(100003, 65536, 9, kt, desc), kt, desc).status(less + 5)[0] == 1
        # bytes 0x00 and 0xff of the k-th image
        for p in range(8):
            for v in (0x00, 0xFF):
                for deep in (False, True):
                    ref = W.Ref64(W.byte_edge_case64(p, v, deep, kt, desc), kt, desc)
                    ks = np.flatnonzero(W.byte_of(ref.sorted_img, p) == v) + 1
                    assert ks.size == (66000 if deep else 20000)
                    st = ref.status(int(ks[ks.size // 2]))
                    kth = st[1] | (st[2] << 32)
                    # deep: round one (all share the top byte, or p = 7 itself), the round at p, and one more below it unless
                    # p = 0, where the 66000 are equal keys (route 2)
                    assert (kth >> (8 * p)) & 0xFF == v and st[5] == ((2 if p in (0, 7) else 3) if deep else 1), (p, v, deep, st)
                    assert st[0] == (2 if deep and p == 0 else 1)
    sp = W.specials64(F64)
    assert np.isin(sp, W.gen64("special", 5000, 1, F64)).all() and np.isnan(sp[:4].view(np.float64)).all()


# --------------------------------------------------------------------------------------------- the size query --
SIZES = [1, 2, 4095, 4096, 4097, 65536, 65537, 100003, 1 << 21, (1 << 21) + 1, 1 << 24, 1 << 28, (1 << 30) + 7, (1 << 32) - 1]


def test_temp_bytes_is_the_headers_formula_a_multiple_of_256_and_monotone(gs):
    lib = gs.lib
    for hv in (0, 1):
        last_n = 0
        for n in SIZES:
            ks = sorted(k for k in {1, 2, 1000, 4096, 4097, 65536, 65537, 1 << 20, n // 2 + 1, n} if 1 <= k <= n)
            last_k = 0
            for k in ks:
                got = lib.gs_topk_u64_temp_bytes(n, k, hv)
                sort_ws = lib.gs_lsb_wide_temp_bytes(k, 8, 4 if hv else 0)
                assert got == W.temp_bytes(n, k, hv, sort_ws) and got % 256 == 0 and got > 0, (n, k, hv)
                assert got >= last_k, (n, k, hv)
                last_k = got
            at_one = lib.gs_topk_u64_temp_bytes(n, 1, hv)
            assert at_one >= last_n, (n, hv)
            last_n = at_one
            assert lib.gs_topk_u64_temp_bytes(n, 0, hv) == 0
        assert lib.gs_topk_u64_temp_bytes(0, 0, hv) == 0
    for k in (1, 5000):
        got = [lib.gs_topk_u64_temp_bytes(n, k, 1) for n in SIZES if n >= k]
        assert got == sorted(got)
    # under one eighth of the key bytes at 2^28 keys, k <= 2^20, with values
    assert lib.gs_topk_u64_temp_bytes(1 << 28, 1 << 20, 1) < (8 << 28) // 8
    assert lib.gs_topk_u64_temp_bytes(1 << 28, 1 << 10, 1) < lib.gs_topk_u64_temp_bytes(1 << 28, 1 << 20, 1)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, n, k, desc=0, kt=U64):
    return gs.lib.gs_topk_u64(temp, temp_bytes, kin, vin, kout, vout, n, k, desc, kt, None)


@pytest.mark.parametrize("n", [5000, 100003])
def test_refusals_and_noops_without_a_device(gs, n):
    k = 100
    need = gs.lib.gs_topk_u64_temp_bytes(n, k, 1)
    assert need > 0
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 26), BASE + (2 << 26), BASE + (3 << 26), BASE + (4 << 26)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, n=n, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0), # too small
        dict(k=n + 1),                                 # k > num_items
        dict(n=1 << 32), dict(n=1 << 32, k=1 << 32), dict(n=(1 << 40) + 5),       # num_items >= 2^32
        dict(kt=0), dict(kt=1), dict(kt=2),            # 32-bit key types
        dict(kt=6), dict(kt=8), dict(kt=11), dict(kt=12), dict(kt=13), dict(kt=-1),   # narrow key types and no type at all
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 4), dict(kout=kout + 4), dict(kin=kin + 1), dict(kout=kout + 2),   # a key pointer not aligned to 8 bytes
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 1), dict(vout=vout + 3),   # a value pointer that is not 4-aligned
        dict(kout=kin), dict(kout=kin + 8 * (n - 1)),  # output inside the keys (8-byte key extents)
        dict(vout=kin + 8 * n - 4), dict(vout=vin), dict(kout=vin + 4 * n - 4 - (4 * n - 4) % 8),
        dict(vout=kout), dict(vout=kout + 8 * k - 4), dict(kout=vout + 4 * k - 8),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 8 * n - 4),      # inputs share a byte
    ]
    for change in bad:
        assert _call(gs, **dict(ok, **change)) == INVALID, change
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_u64_temp_bytes(n, k, 0)
    assert 0 < need0 < need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    for kt in W.KEY_TYPES:
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
    assert gs.lib.gs_topk_u64_status(None, 1000, 0, 0, st, None) == 0 and list(st) == [0] * 8
    st = (C.c_uint32 * 8)(*([7] * 8))
    assert gs.lib.gs_topk_u64_status(None, 0, 0, 1, st, None) == 0 and list(st) == [0] * 8
    assert gs.lib.gs_topk_u64_status(None, 1000, 10, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u64_status(BASE, 10, 11, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u64_status(BASE, 1 << 32, 10, 0, st, None) == INVALID
    assert gs.lib.gs_topk_u64_status(BASE, 1000, 10, 0, None, None) == INVALID


# ------------------------------------------------------------------------------------------------ front ends --
def test_front_end_argument_checks_need_no_device(gs):
    import torch
    assert gs.DeviceTopK64 is not gs.DeviceTopK and gs.DeviceTopK64 is not gs.DeviceTopK16
    for form in (gs.DeviceTopK64.MinKeys, gs.DeviceTopK64.MaxKeys):
        assert form(None, 0, None, None, 100003, 77) == gs.lib.gs_topk_u64_temp_bytes(100003, 77, 0)
    for form in (gs.DeviceTopK64.MinPairs, gs.DeviceTopK64.MaxPairs):
        assert form(None, 0, None, None, None, None, 100003, 77) == gs.lib.gs_topk_u64_temp_bytes(100003, 77, 1)
        for kt in W.KEY_TYPES:
            assert form(None, 0, None, None, None, None, 100003, 77, key_type=kt) == gs.lib.gs_topk_u64_temp_bytes(100003, 77, 1)
        for kt in (gs.GS_KEY_U32, gs.GS_KEY_F32, gs.GS_KEY_U16, gs.GS_KEY_BF16, gs.GS_KEY_U8, gs.GS_KEY_F8):
            with pytest.raises(TypeError):
                form(None, 0, None, None, None, None, 100003, 77, key_type=kt)
    tmp = torch.zeros(256, dtype=torch.uint8)
    for dtype in (torch.int32, torch.float32, torch.int16, torch.int8):
        x = torch.zeros(10, dtype=dtype)
        with pytest.raises(TypeError):
            gs.DeviceTopK64.MinKeys(tmp, 256, x, x.clone(), 10, 2)
    x64 = torch.zeros(10, dtype=torch.float64)
    with pytest.raises(ValueError):
        gs.DeviceTopK64.MinKeys(tmp, 256, x64, x64.clone(), 10, 2)               # not a device tensor
    for dtype in (torch.int64, torch.float64):
        t = torch.zeros(10, dtype=dtype)
        with pytest.raises(ValueError):
            gs.topk(t, 11)
        with pytest.raises(ValueError):
            gs.topk(t, 2, values=torch.zeros(10, dtype=torch.int32), indices=True)
        ko, vo = gs.topk(t, 0, indices=True)
        assert ko.numel() == 0 and ko.dtype == dtype and vo.numel() == 0 and vo.dtype == torch.int32
        ko, vo = gs.topk(t, 0)
        assert ko.dtype == dtype and vo is None
    with pytest.raises(TypeError):
        gs.topk(torch.zeros(10, dtype=torch.complex64), 2)                       # 8 bytes, no key category
