"""gs_topk_u32 without a device: the numpy reference against the CPU oracle, every refusal and no-op of the contract, the
workspace query against the header's formula, and the size-query phase of the Python front end."""
import numpy as np
import pytest

import topk_ref as R

INVALID = 1          # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing


def _special_f32():
    tiny = np.finfo(np.float32).smallest_subnormal
    sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5, np.nan, -np.nan], np.float32).view(np.uint32)
    return np.concatenate([sp, np.array([0x7FC00001, 0xFFC00002], np.uint32)])


@pytest.mark.parametrize("descending", [False, True])
def test_reference_matches_oracle_ranks_u32(oracle, descending):
    rng = np.random.default_rng(5)
    for n in (1, 2, 65, 1000, 20011):
        keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        keys[rng.random(n) < 0.3] = keys[0]                     # ties: stability shows
        want = oracle.lsb_reference_ranks(keys, 0, 32, descending)
        assert np.array_equal(R.ranks(keys, R.U32, descending), want)
        for k in sorted({1, n // 2 or 1, n}):
            ko, vo, st = R.topk(keys, k, R.U32, descending)
            assert np.array_equal(vo, want[:k]) and np.array_equal(ko, keys[want[:k]])
            assert st[1] + st[2] == k and 1 <= st[2] and st[1] < k <= st[1] + np.count_nonzero(R.image(keys, R.U32, descending) == st[0])


def test_reference_images_of_signed_and_float_keys(oracle):
    """The i32 / f32 images are the oracle's order on the mapped keys: -1 < 0, MIN first; negative NaNs, -inf .. -0.0, +0.0 ..
    +inf, positive NaNs."""
    i = np.array([0, -1, 2**31 - 1, -2**31, 5, -5], np.int32).view(np.uint32)
    assert list(i[R.ranks(i, R.I32)].view(np.int32)) == [-2**31, -5, -1, 0, 5, 2**31 - 1]
    assert list(i[R.ranks(i, R.I32, True)].view(np.int32)) == [2**31 - 1, 5, 0, -1, -5, -2**31]
    f = _special_f32()
    s = f[R.ranks(f, R.F32)]
    assert s[0] == 0xFFC00002 and s[1] == np.array([-np.nan], np.float32).view(np.uint32)[0]       # negative NaNs by their bits
    assert list(s[2:10].view(np.float32)) == [-np.inf, -1.5, -np.finfo(np.float32).smallest_subnormal, -0.0, 0.0,
                                              np.finfo(np.float32).smallest_subnormal, 1.5, np.inf]
    assert s[5] == 0x80000000 and s[6] == 0                                                          # -0.0 before +0.0
    assert list(s[10:]) == [0x7FC00000, 0x7FC00001]
    # the oracle sorts the images as plain u32: same ranks
    assert np.array_equal(R.ranks(f, R.F32), oracle.lsb_reference_ranks(R.image(f, R.F32), 0, 32, False))
    assert np.array_equal(R.ranks(f, R.F32, True), oracle.lsb_reference_ranks(R.image(f, R.F32), 0, 32, True))


def test_reference_cut_inside_a_tie_run_takes_the_lowest_indices():
    keys = np.array([7, 3, 7, 3, 7, 1, 7], np.uint32)
    ko, vo, st = R.topk(keys, 5, R.U32)
    assert list(ko) == [1, 3, 3, 7, 7] and list(vo) == [5, 1, 3, 0, 2] and st == [7, 3, 2, 7]
    ko, vo, st = R.topk(keys, 2, R.U32, True)
    assert list(ko) == [7, 7] and list(vo) == [0, 2] and st[1:3] == [0, 2]


def _call(gs, temp, temp_bytes, kin, vin, kout, vout, n, k, desc=0, kt=0):
    return gs.lib.gs_topk_u32(temp, temp_bytes, kin, vin, kout, vout, n, k, desc, kt, None)


def test_refusals_and_noops_without_a_device(gs):
    n, k = 100000, 1000
    need = gs.lib.gs_topk_temp_bytes(n, k, 1)
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 24), BASE + (2 << 24), BASE + (3 << 24), BASE + (4 << 24)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, n=n, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1),                     # too small
        dict(temp_bytes=0),
        dict(k=n + 1),                                 # k > num_items
        dict(n=1 << 32, k=1),                          # num_items >= 2^32
        dict(n=(1 << 32) + 5, k=(1 << 32) + 5),
        dict(kt=3), dict(kt=-1), dict(kt=6), dict(kt=12),   # key types other than U32 / I32 / F32
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 2), dict(kout=kout + 1), dict(vin=vin + 3), dict(vout=vout + 2),   # misaligned arrays
        dict(kout=kin), dict(kout=kin + 4 * (n - 1)),  # output inside the keys
        dict(vout=kin + 4 * 10), dict(vout=vin), dict(kout=vin + 4 * (n - 1)),
        dict(vout=kout), dict(vout=kout + 4 * (k - 1)), dict(kout=vout + 4 * (k - 1)),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 4 * (n - 1)),    # inputs share a byte
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # the arguments form (no d_vals_in) and the keys-only form size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_temp_bytes(n, k, 0)
    assert need0 < need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # adjacent arrays are fine as far as the checks go: refused only for the workspace
    assert _call(gs, **dict(ok, kout=kin + 4 * n, temp_bytes=need - 1)) == INVALID
    # no-ops: nothing is needed
    for kt in (0, 1, 2):
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, n, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, n, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, 0, 1) == INVALID       # k > num_items, even for an empty array
    assert _call(gs, None, 0, None, None, None, None, n, 0, 0, 7) == INVALID  # a bad key type is refused before the no-op


def test_status_refusals_and_noops_without_a_device(gs):
    import ctypes as C
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_status(None, 0, 0, 0, out, None) == 0 and list(out) == [0] * 8
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_status(None, 1000, 0, 1, out, None) == 0 and list(out) == [0] * 8
    assert gs.lib.gs_topk_status(None, 1000, 10, 0, out, None) == INVALID
    assert gs.lib.gs_topk_status(BASE, 1000, 1001, 0, out, None) == INVALID
    assert gs.lib.gs_topk_status(BASE, 1 << 32, 1, 0, out, None) == INVALID
    assert gs.lib.gs_topk_status(BASE, 1000, 10, 0, None, None) == INVALID


SIZES = [0, 1, 2, 63, 8191, 8192, 8193, 17407, 17408, 17409, 65535, 65536, 65537, 100003, (1 << 20) + 3, (1 << 21) - 1, 1 << 21,
         (1 << 21) + 1, 1 << 24, (1 << 28) + 5, 1 << 30, (1 << 32) - 1]


def test_temp_bytes_is_the_headers_formula(gs):
    for n in SIZES:
        for k in sorted({0, 1, 2, 64, 8192, 8193, n // 2, max(n - 1, 0), n}):
            if k > n:
                continue
            for hv in (0, 1):
                got = gs.lib.gs_topk_temp_bytes(n, k, hv)
                assert got % 256 == 0
                assert got == R.temp_bytes(n, k, hv, gs.lib.gs_lsb_copy_temp_bytes(k, hv)), (n, k, hv)


def test_temp_bytes_is_monotone(gs):
    ks = [0, 1, 2, 64, 1000, 8192, 8193, 17408, 17409, 65536, 100003, 1 << 20, (1 << 20) + 3, 1 << 24]
    for hv in (0, 1):
        for k in ks:
            last = 0
            for n in [s for s in SIZES if s >= k]:
                b = gs.lib.gs_topk_temp_bytes(n, k, hv)
                assert b >= last, (n, k, hv)
                last = b
        for n in SIZES:
            last = 0
            for k in [x for x in ks if x <= n] + [n]:
                b = gs.lib.gs_topk_temp_bytes(n, k, hv)
                assert b >= last, (n, k, hv)
                last = b
        # fine steps around the tile, chunk and candidate-list edges
        last = 0
        for n in list(range(8000, 8400, 7)) + list(range(65400, 65700, 5)) + list(range((1 << 21) - 40, (1 << 21) + 40)):
            b = gs.lib.gs_topk_temp_bytes(n, 100, hv)
            assert b >= last
            last = b
    assert gs.lib.gs_topk_temp_bytes(1 << 20, 100, 1) > gs.lib.gs_topk_temp_bytes(1 << 20, 100, 0)


def test_device_topk_size_query_phase(gs):
    """d_temp_storage=None returns the size and touches nothing: no tensor is needed."""
    n, k = 300007, 4096
    for fn in (gs.DeviceTopK.MinKeys, gs.DeviceTopK.MaxKeys):
        assert fn(None, 0, None, None, n, k) == gs.lib.gs_topk_temp_bytes(n, k, 0)
    for fn in (gs.DeviceTopK.MinPairs, gs.DeviceTopK.MaxPairs):
        assert fn(None, 0, None, None, None, None, n, k) == gs.lib.gs_topk_temp_bytes(n, k, 1)
    assert callable(gs.topk) and "DeviceTopK" in gs.__all__ and "topk" in gs.__all__
