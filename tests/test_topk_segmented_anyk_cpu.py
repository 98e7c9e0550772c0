"""gs_topk_segmented_anyk_u32 without a device: every refusal and no-op of the contract, the workspace query against the
header's formula and its monotonicity, the plan of every shape the GPU file runs, gs_topk_segmented_u32 and topk_segmented()
still capped at 1024, and the argument checks of topk_segmented_anyk()."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_segmented_anyk_ref as AR
import topk_segmented_ref as SR

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
CH = AR.CH


def _seg_bytes(gs, S, k, hv):
    return gs.lib.gs_segmented_temp_bytes(S * k, hv, S)


def _want(gs, n, S, k, hv):
    if AR.refused(n, S, k) or n == 0 or S == 0 or k == 0:
        return 0
    return AR.temp_bytes(n, S, k, hv, _seg_bytes(gs, S, k, hv))


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc=0, kt=0):
    return gs.lib.gs_topk_segmented_anyk_u32(temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc, kt, None)


@pytest.mark.parametrize("n,k", [(700, 100), (5000, 1025), (200000, 5000)])
def test_refusals_and_noops_without_a_device(gs, n, k):
    S = 50
    need = gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, 1)
    assert need > 0
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, counts=counts, n=n, S=S, begin=begin, end=end, k=k)
    bad = [
        dict(temp=None),                                   # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0),     # too small
        dict(n=1 << 31), dict(n=(1 << 31) + 5),            # int offsets
        dict(S=1 << 22, k=512), dict(S=(1 << 31) - 1, k=2), dict(S=1, k=1 << 31), dict(S=3, k=1 << 62),   # num_segments * k >= 2^31
        dict(kt=3), dict(kt=-1), dict(kt=6), dict(kt=12),  # key types other than U32 / I32 / F32
        dict(vout=None),                                   # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None), dict(begin=None), dict(end=None),   # NULL keys or offsets
        dict(kin=kin + 2), dict(kout=kout + 1), dict(vin=vin + 3), dict(vout=vout + 2), dict(counts=counts + 2),
        dict(begin=begin + 1), dict(end=end + 2),          # misaligned arrays
        dict(kout=kin), dict(kout=kin + 4 * (n - 1)),      # an output inside the keys
        dict(vout=kin + 4 * 10), dict(vout=vin), dict(kout=vin + 4 * (n - 1)),
        dict(vout=kout), dict(vout=kout + 4 * (S * k - 1)), dict(kout=vout + 4 * (S * k - 1)),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 4 * (n - 1)),        # inputs share a byte
        dict(counts=kout + 4 * (S * k - 1)), dict(counts=kin), dict(counts=begin + 4 * (S - 1)), dict(counts=end),
        dict(begin=kout), dict(end=vout + 4 * (S * k - 1)), dict(begin=kin + 4 * (n - 1)), dict(end=vin),
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # what shares nothing passes the checks: refused only for the workspace
    assert _call(gs, **dict(ok, kout=kin + 4 * n, temp_bytes=need - 1)) == INVALID
    assert _call(gs, **dict(ok, counts=None, temp_bytes=need - 1)) == INVALID
    assert _call(gs, **dict(ok, end=begin + 4, temp_bytes=need - 1)) == INVALID          # S + 1 offsets in one array
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID               # the arguments form
    need0 = gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, 0)
    assert 0 < need0 < need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed, and the query returns 0
    for kt in (0, 1, 2):
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, 0, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, counts, n, S, begin, end, 0, desc, kt) == 0
    for hv in (0, 1):
        q = gs.lib.gs_topk_segmented_anyk_temp_bytes
        assert q(0, S, k, hv) == 0 and q(n, 0, k, hv) == 0 and q(n, S, 0, hv) == 0
        assert q(1 << 31, S, k, hv) == 0 and q(n, 1 << 22, 512, hv) == 0 and q(n, 1, 1 << 31, hv) == 0   # refused shapes
        assert q(n, (1 << 22) - 1, 512, hv) > 0
    assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, 0, 7) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, None, 0, 1, None, None, 1 << 31) == INVALID   # the limit before the no-op
    # k may exceed num_items and every segment's length
    assert gs.lib.gs_topk_segmented_anyk_temp_bytes(10, 3, 70000, 1) > 0
    assert _call(gs, **dict(ok, n=10, k=70000, temp_bytes=gs.lib.gs_topk_segmented_anyk_temp_bytes(10, S, 70000, 1) - 1)) == INVALID


# --------------------------------------------------------------------------------------------- the size query --
NS = [0, 1, 2, 64, 1024, 1025, 8191, 8192, 8193, 16384, 16386, 24579, 65536, 151936, 1 << 20, (1 << 26) + 9, (1 << 31) - 1]
KS = [0, 1, 2, 64, 1000, 1024, 1025, 5000, 8192, 8193, 70000, 1 << 20]
SS = [0, 1, 2, 3, 7, 256, 1000, 1 << 15]


def test_temp_bytes_is_the_headers_formula(gs):
    seen = 0
    for n in NS:
        for S in SS:
            for k in KS + [1 << 31]:
                for hv in (0, 1):
                    got = gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, hv)
                    assert got % 256 == 0 and got == _want(gs, n, S, k, hv), (n, S, k, hv)
                    seen += got > 0
    assert seen > 1000
    rng = np.random.default_rng(7)
    for _ in range(400):
        n = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        S = int(rng.integers(1, 1 << int(rng.integers(1, 20))))
        k = int(rng.integers(1, 1 << int(rng.integers(1, 18))))
        hv = int(rng.integers(0, 2))
        assert gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, hv) == _want(gs, n, S, k, hv), (n, S, k, hv)
    # the long-segment areas vanish when num_items <= CH; the histograms are at most about one byte per key
    front = 4096 + 5 * 256
    for hv in (0, 1):
        tail = 2 * 256 + (1 + 2 * hv) * AR._a(4 * 16 * 2000) + AR._a(_seg_bytes(gs, 16, 2000, hv)) + 256
        assert gs.lib.gs_topk_segmented_anyk_temp_bytes(CH, 16, 2000, hv) == front + tail
        assert gs.lib.gs_topk_segmented_anyk_temp_bytes(CH + 1, 16, 2000, hv) == front + 256 + 256 + 256 + 4 * 2048 + 256 + tail
    for n in (CH + 1, 1 << 20, (1 << 31) - 1):
        lmax, _ = AR.geometry(n, 1 << 20)
        assert 4 * AR.BINS * lmax <= 8192 * n // 8193


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0), with fine steps around n = 1024, CH and the slab."""
    def tb(n, S, k, hv):
        return None if AR.refused(n, S, k) else gs.lib.gs_topk_segmented_anyk_temp_bytes(n, S, k, hv)

    def rising(values):
        values = [v for v in values if v is not None]
        assert all(a <= b for a, b in zip(values, values[1:])), values
    slab = AR.SLAB_TILES * AR.TILE
    fine = sorted(list(range(1000, 1050)) + list(range(8100, 8300, 3)) + list(range(16300, 16500, 3)) +
                  list(range(slab - 20, slab + 20)) + list(range(3 * CH - 5, 3 * (CH + 1) + 5)))
    for hv in (0, 1):
        for S in SS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for n in NS[1:]])
            for k in (1, 1025, 70000):
                rising([tb(n, S, k, hv) for n in fine])
        for n in NS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for S in SS[1:]])
            for S in SS[1:]:
                rising([tb(n, S, k, hv) for k in KS[1:]])
                rising([tb(n, S, k, hv) for k in range(1000, 1050)])
    assert tb(1 << 20, 100, 5000, 1) > tb(1 << 20, 100, 5000, 0)


# --------------------------------------------------------------------------------------------------- the plan --
def _plan(gs, n, S, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    rc = gs.lib.gs_topk_segmented_anyk_plan(n, S, k, hv, out)
    return rc, list(out)


def test_plan_is_the_reference_plan(gs):
    for n in NS:
        for S in SS:
            for k in KS + [1 << 31]:
                want = AR.plan(n, S, k)
                rc, got = _plan(gs, n, S, k, k & 1)
                if want is None:
                    assert rc == INVALID and got == [0] * 8, (n, S, k)
                else:
                    assert rc == 0 and got == want, (n, S, k, got, want)
    assert gs.lib.gs_topk_segmented_anyk_plan(1, 1, 1, 0, None) == INVALID
    D = gs.DeviceTopKSegmentedAnyK
    assert D.Plan(20000, 3, 5000) == AR.plan(20000, 3, 5000) == [7, 19, CH, 8192, 4, 2, 4, 0]
    assert D.Plan(1024, 9, 5000)[:2] == [1, 6] and D.Plan(CH, 9, 5000)[:2] == [3, 8]
    assert not hasattr(D, "MaxK")
    assert sorted(a for a in dir(D) if not a.startswith("_")) == ["MaxKeys", "MaxPairs", "MinKeys", "MinPairs", "Plan", "Status"]
    with pytest.raises(gs.GpuSortError):
        D.Plan(1 << 31, 3, 5)
    for hv, form in ((0, D.MinKeys), (0, D.MaxKeys)):
        assert form(None, 0, None, None, None, 20000, 3, None, None, 5000) == gs.lib.gs_topk_segmented_anyk_temp_bytes(20000, 3, 5000, hv)
    for form in (D.MinPairs, D.MaxPairs):
        assert form(None, 0, None, None, None, None, None, 20000, 3, None, None, 5000) == gs.lib.gs_topk_segmented_anyk_temp_bytes(20000, 3, 5000, 1)


def test_plan_of_every_gpu_shape(gs):
    """What each shape of tests/test_topk_segmented_anyk_gpu.py is meant to exercise, asserted with the ref and the plan alone."""
    assert [AR.list_of(x) for x in AR.EDGE_LENGTHS] == AR.EDGE_LISTS
    begin, end, n, lens = AR.shuffled_edges()
    assert sorted(end - begin) == sorted(AR.EDGE_LENGTHS) and list(end - begin) == lens
    assert np.any(begin % 2 == 1) and np.any(begin % 4 != 0) and list(np.argsort(begin)) != list(range(len(begin)))
    order = np.argsort(begin)
    assert np.all(begin[order][1:] >= end[order][:-1]) and end.max() <= n        # no overlap: nothing can be dropped
    assert AR.status(begin, end, n) == AR.EDGE_STATUS
    for k in AR.EDGE_KS:
        assert _plan(gs, n, len(begin), k) == (0, AR.plan(n, len(begin), k)) and AR.plan(n, len(begin), k)[:2] == [7, 19]
    for x in AR.EDGE_LENGTHS[1:]:        # k runs below, at and above every length (at: 1, 1024, 1025, 8192, 8193 are lengths too)
        assert any(k < x for k in AR.EDGE_KS) or x == 1
        assert any(k > x for k in AR.EDGE_KS)
    assert all(k in AR.EDGE_LENGTHS for k in (1, 1024, 1025, 8192, 8193))
    assert AR.list_of(AR.EQUAL_LENGTH) == 5 and -(-AR.EQUAL_LENGTH // AR.TILE) == 3 and max(AR.EQUAL_KS) < AR.EQUAL_LENGTH
    assert AR.EQUAL_KS[1] > AR.TILE          # the cut of the tie run lies in the second tile
    assert AR.LONG_COUNT > 1024 and AR.geometry(AR.LONG_COUNT * (CH + 1), AR.LONG_COUNT) == (AR.LONG_COUNT, 2 * AR.LONG_COUNT - 1 + 1)
    for i in range(AR.SWEEP_CASES):
        _, b, e, n, k = AR.sweep_case(i)
        assert 1 <= len(b) <= 40 and 1 <= k <= 45000 and 0 <= (e - b).min() and (e - b).max() <= 40000 and e.max() <= n
        o = np.argsort(b, kind="stable")
        o = o[(e > b)[o]]                   # the segments that hold something do not overlap
        assert np.all(b[o][1:] >= e[o][:-1])
        assert AR.status(b, e, n)[7] == 0
    lens = np.concatenate([AR.sweep_case(i)[2] - AR.sweep_case(i)[1] for i in range(AR.SWEEP_CASES)])
    assert {AR.list_of(int(x)) for x in lens} == {None, 0, 1, 2, 3, 4, 5}


# ------------------------------------------------------------------------------ the capped call stays capped --
def test_the_capped_call_keeps_refusing_k_above_1024(gs):
    for hv in (0, 1):
        assert gs.lib.gs_topk_segmented_temp_bytes(200000, 50, 1025, hv) == 0
        assert gs.lib.gs_topk_segmented_temp_bytes(200000, 50, 1024, hv) == SR.temp_bytes(200000, 50, 1024, hv) > 0
    step = 1 << 26
    p = [BASE + i * step for i in range(8)]
    assert gs.lib.gs_topk_segmented_u32(p[7], 1 << 30, p[0], None, p[2], None, None, 200000, 50, p[5], p[6], 1025, 0, 0, None) == INVALID
    out = (C.c_uint32 * 8)()
    assert gs.lib.gs_topk_segmented_plan(200000, 50, 1025, 0, out) == INVALID
    assert gs.DeviceTopKSegmented.MaxK() == 1024


def test_topk_segmented_still_raises_above_1024(gs):
    """On the host: the refusal comes from the size query, before anything touches a device."""
    keys = torch.zeros(3000, dtype=torch.int32)
    off = torch.tensor([0, 1500, 3000], dtype=torch.int32)
    with pytest.raises(ValueError, match="k <= 1024"):
        gs.topk_segmented(keys, off, 1025)


# --------------------------------------------------------------------------------------------- the front end --
def test_topk_segmented_anyk_argument_checks(gs):
    keys = torch.zeros(3000, dtype=torch.float32)
    off = torch.tensor([0, 1500, 3000], dtype=torch.int32)
    f = gs.topk_segmented_anyk
    assert "topk_segmented_anyk" in gs.__all__ and "DeviceTopKSegmentedAnyK" in gs.__all__
    with pytest.raises(ValueError, match="not both"):
        f(keys, off, 2000, values=torch.zeros(3000, dtype=torch.int32), indices=True)
    for bad in (torch.zeros(3000, dtype=torch.float16), torch.zeros(3000, dtype=torch.int64), torch.zeros(3000, dtype=torch.float64),
                torch.zeros(3000, dtype=torch.bfloat16), torch.zeros(3000, dtype=torch.int16)):
        with pytest.raises(TypeError, match="32-bit keys"):
            f(bad, off, 2000)
    with pytest.raises(TypeError):
        f(keys.reshape(2, 1500), off, 2000)
    with pytest.raises(TypeError, match="int32 offsets"):
        f(keys, off.long(), 2000)
    with pytest.raises(TypeError, match="int32 offsets"):
        f(keys, off[:-1], 2000, end_offsets=off[1:].long())
    with pytest.raises(ValueError, match="S \\+ 1"):
        f(keys, off[:0], 2000)
    with pytest.raises(ValueError, match="as many ends"):
        f(keys, off[:-1], 2000, end_offsets=off)
    with pytest.raises(ValueError, match="k >= 0"):
        f(keys, off, -1)
    with pytest.raises(ValueError, match="values must"):
        f(keys, off, 2000, values=torch.zeros(2999, dtype=torch.int32))
    with pytest.raises(ValueError, match="values must"):
        f(keys, off, 2000, values=torch.zeros(3000, dtype=torch.int64))
    with pytest.raises(ValueError, match="segments \\* k below 2\\^31"):
        f(keys, off, 1 << 30)
    # the outputs of a call that has nothing to do: [S, k] keys in the input dtype, int32 values and counts
    ko, vo, counts = f(keys, off, 0, indices=True)
    assert tuple(ko.shape) == (2, 0) and ko.dtype == torch.float32 and vo.dtype == torch.int32 and counts.tolist() == [0, 0]
    ko, vo, counts = f(keys[:0], off, 5000)
    assert tuple(ko.shape) == (2, 5000) and vo is None and counts.tolist() == [0, 0]
    import inspect
    assert ([(p.name, p.default) for p in inspect.signature(f).parameters.values()]
            == [(p.name, p.default) for p in inspect.signature(gs.topk_segmented).parameters.values()])
