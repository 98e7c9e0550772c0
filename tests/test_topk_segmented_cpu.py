"""gs_topk_segmented_u32 without a device: every refusal and no-op of the contract, the workspace query against the header's
formula, the plan of every shape the GPU file runs, the per-segment reference against the CPU oracle, and the numpy model of
the chunk level plus the streaming final against the reference -- with wrong variants of the model that must differ."""
import ctypes as C

import numpy as np
import pytest

import topk_ref as R
import topk_segmented_ref as SR

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U32, I32, F32 = R.U32, R.I32, R.F32
CH = SR.CH


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc=0, kt=0):
    return gs.lib.gs_topk_segmented_u32(temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc, kt, None)


@pytest.mark.parametrize("n", [700, 5000, 200000])
def test_refusals_and_noops_without_a_device(gs, n):
    S, k = 50, 100
    need = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, 1)
    assert need > 0
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, counts=counts, n=n, S=S, begin=begin, end=end, k=k)
    bad = [
        dict(temp=None),                                   # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0),     # too small
        dict(k=1025),                                      # k > max k
        dict(n=1 << 31), dict(n=(1 << 31) + 5),            # int offsets
        dict(S=1 << 23, k=512), dict(S=(1 << 32) - 1, k=2),    # num_segments * k >= 2^32
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
    # S + 1 offsets in one array: the ends are the begins one further on
    assert _call(gs, **dict(ok, end=begin + 4, temp_bytes=need - 1)) == INVALID
    # the arguments and keys-only forms size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed, and the query returns 0
    for kt in (0, 1, 2):
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, 0, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, counts, n, S, begin, end, 0, desc, kt) == 0
    for hv in (0, 1):
        assert gs.lib.gs_topk_segmented_temp_bytes(0, S, k, hv) == 0 and gs.lib.gs_topk_segmented_temp_bytes(n, 0, k, hv) == 0
        assert gs.lib.gs_topk_segmented_temp_bytes(n, S, 0, hv) == 0
        # refused shapes: the query returns 0
        assert gs.lib.gs_topk_segmented_temp_bytes(n, S, 1025, hv) == 0
        assert gs.lib.gs_topk_segmented_temp_bytes(1 << 31, S, k, hv) == 0
        assert gs.lib.gs_topk_segmented_temp_bytes(n, 1 << 23, 512, hv) == 0
    assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, 0, 7) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, 1025) == INVALID      # k > max k before the no-op
    # k may exceed num_items and every segment's length
    assert gs.lib.gs_topk_segmented_temp_bytes(10, 3, 1024, 1) > 0
    assert _call(gs, **dict(ok, n=10, k=1024, temp_bytes=gs.lib.gs_topk_segmented_temp_bytes(10, S, 1024, 1) - 1)) == INVALID


# --------------------------------------------------------------------------------------------- the size query --
NS = [0, 1, 2, 64, 1024, 1025, 8191, 8192, 8193, 16384, 16386, 24579, 65536, 151936, 1 << 20, (1 << 26) + 9, (1 << 31) - 1]
KS = [0, 1, 2, 8, 64, 65, 1000, 1023, 1024]
SS = [0, 1, 2, 3, 7, 256, 1000, 1 << 20]


def test_temp_bytes_is_the_headers_formula(gs):
    for n in NS:
        for S in SS:
            for k in KS + [1025]:
                for hv in (0, 1):
                    got = gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
                    assert got % 256 == 0 and got == SR.temp_bytes(n, S, k, hv), (n, S, k, hv)
    rng = np.random.default_rng(7)
    for _ in range(400):
        n = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        S = int(rng.integers(1, 1 << int(rng.integers(1, 23))))
        k = int(rng.integers(1, 1100))
        hv = int(rng.integers(0, 2))
        assert gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv) == SR.temp_bytes(n, S, k, hv), (n, S, k, hv)
    # the long-segment areas vanish when num_items <= CH
    for k in (1, 1024):
        assert gs.lib.gs_topk_segmented_temp_bytes(CH, 16, k, 1) == 4096 + 5 * 256 + 256
        assert gs.lib.gs_topk_segmented_temp_bytes(CH + 1, 16, k, 0) == 4096 + 5 * 256 + 256 + 256 + ((4 * k * 2 + 255) & ~255) + 256


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(n, S, k, hv):
        return None if SR.refused(n, S, k) else gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)

    def rising(values):
        values = [v for v in values if v is not None]
        assert all(a <= b for a, b in zip(values, values[1:])), values
    fine = list(range(8100, 8300, 3)) + list(range(16300, 16500, 3)) + list(range(3 * CH - 5, 3 * (CH + 1) + 5))
    for hv in (0, 1):
        for S in SS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for n in NS[1:]])
                rising([tb(n, S, k, hv) for n in fine])
        for n in NS[1:]:
            for k in KS[1:]:
                rising([tb(n, S, k, hv) for S in SS[1:]])
            for S in SS[1:]:
                rising([tb(n, S, k, hv) for k in KS[1:]])
    assert tb(1 << 20, 100, 100, 1) > tb(1 << 20, 100, 100, 0)


# --------------------------------------------------------------------------------------------------- the plan --
def _plan(gs, n, S, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    rc = gs.lib.gs_topk_segmented_plan(n, S, k, hv, out)
    return rc, list(out)


def test_plan_is_the_reference_plan(gs):
    for n in NS:
        for S in SS:
            for k in KS + [1025]:
                want = SR.plan(n, S, k)
                rc, got = _plan(gs, n, S, k, k & 1)
                if want is None:
                    assert rc == INVALID and got == [0] * 8, (n, S, k)
                else:
                    assert rc == 0 and got == want, (n, S, k, got, want)
    assert gs.lib.gs_topk_segmented_plan(1, 1, 1, 0, None) == INVALID
    assert gs.DeviceTopKSegmented.Plan(20000, 3, 50) == SR.plan(20000, 3, 50) == [7, 10, CH, 2, 4, 1024, 0, 0]
    assert gs.DeviceTopKSegmented.Plan(1024, 9, 50)[:2] == [1, 6] and gs.DeviceTopKSegmented.Plan(CH, 9, 50)[:2] == [3, 7]
    assert gs.DeviceTopKSegmented.MaxK() == SR.MAX_K


def test_plan_of_every_gpu_shape(gs):
    """What each shape of tests/test_topk_segmented_gpu.py is meant to exercise, asserted with the ref and the plan alone."""
    assert [SR.list_of(x) for x in SR.EDGE_LENGTHS] == SR.EDGE_LISTS
    begin, end, n = SR.packed(SR.EDGE_LENGTHS, gap=3)
    st = SR.status(begin, end, n)
    assert st == [4, 3, 3, 3, 3, 2, 2 + 3, 0] and all(c > 0 for c in st[:7])
    for k in SR.EDGE_KS:
        assert _plan(gs, n, len(begin), k) == (0, SR.plan(n, len(begin), k)) and SR.plan(n, len(begin), k)[0] == 7
    for q in range(6):      # over the k values, k < len occurs in every list and k > len in every wave list (k <= 1024 < the others)
        lens = [x for x in SR.EDGE_LENGTHS if SR.list_of(x) == q]
        assert any(k < x for k in SR.EDGE_KS for x in lens)
        assert q >= 4 or any(k > x for k in SR.EDGE_KS for x in lens)
    for length, k, rounds in SR.LONG_SHAPES:
        assert SR.final_rounds(length, k) == rounds and SR.list_of(length) == 5
    assert SR.next_of(8 * CH + 1, 1024) == 8193
    assert SR.final_rounds(8 * CH, 1024) == 1 and SR.final_rounds(8 * CH + 1, 1024) == 2     # a row that fits one chunk is one round
    for c in SR.LIST_COUNTS:
        for q, length in enumerate(SR.CLASS_LENGTHS):
            assert SR.list_of(length) == q
    # three copies of one segment of 4 * CH elements: the task capacity holds one of them
    lmax, tmax = SR.geometry(4 * CH, 3)
    assert (lmax, tmax) == (3, 7) and min(lmax, tmax // 4) == 1


# ------------------------------------------------------------------------------------------------ the reference --
@pytest.mark.parametrize("descending", [False, True])
def test_segment_reference_matches_oracle_ranks(oracle, descending):
    rng = np.random.default_rng(11)
    n = 4000
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[rng.random(n) < 0.3] = 77           # ties: stability shows
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    begin = np.array([0, 10, 500, 3000, 2000, -5, 3990, 100, 100], np.int32)
    end = np.array([10, 400, 500, 3999, 2100, 7, 4100, 50, 101], np.int32)
    for k in (1, 100, 1024):
        ko, po, counts = SR.seg_topk(keys, begin, end, k, U32, descending)
        kv, vo, _ = SR.seg_topk(keys, begin, end, k, U32, descending, vals)
        for s in range(begin.size):
            lo, hi = max(int(begin[s]), 0), min(int(end[s]), n)
            ln = max(hi - lo, 0)
            kept = min(k, ln)
            assert counts[s] == kept
            assert (ko[s, kept:] == SR.FILL).all() and (po[s, kept:] == SR.FILL).all()
            if kept:
                want = oracle.lsb_reference_ranks(np.ascontiguousarray(keys[lo:hi]), 0, 32, descending)[:kept]
                assert np.array_equal(po[s, :kept], want) and np.array_equal(ko[s, :kept], keys[lo:hi][want])
                assert np.array_equal(kv[s, :kept], ko[s, :kept]) and np.array_equal(vo[s, :kept], vals[lo:hi][want])
    assert list(SR.seg_topk(keys, begin, end, 5, U32)[2]) == [5, 5, 0, 5, 5, 5, 5, 0, 1]


# ------------------------------------------------------------------------------------------ the streaming model --
def _model_inputs(rng, n, kind, kt):
    if kind == "uniform":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "equal":
        return np.full(n, 0x3F800000, np.uint32)
    if kind == "three":
        return np.array([5, 0x80000001, 0xFFFFFFF0], np.uint32)[rng.integers(0, 3, n)]
    if kind == "few":
        return rng.integers(0, 7, n, dtype=np.uint64).astype(np.uint32) * np.uint32(0x11111111)
    return rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32) | np.uint32(0x42000000)


def test_stream_model_matches_the_reference():
    """400 random cases with heavy ties: chunk 4..40, k up to half of it, lengths up to many streaming rounds; all key types,
    both directions."""
    rng = np.random.default_rng(2025)
    kinds = ("uniform", "equal", "three", "few", "topbyte")
    most = 0
    for case in range(400):
        ch = int(rng.integers(4, 41))
        k = int(rng.integers(1, ch // 2 + 1))
        n = int(rng.integers(ch + 1, ch * 40))
        kt, desc, kind = case % 3, bool((case // 3) % 2), kinds[case % 5]
        keys = _model_inputs(rng, n, kind, kt)
        ek, ev, _ = R.topk(keys, min(k, n), kt, desc)
        mk, mp, rounds = SR.stream_model(keys, k, kt, desc, ch)
        assert np.array_equal(mk, ek) and np.array_equal(mp, ev), (case, ch, k, n, kt, desc, kind)
        assert rounds == SR.final_rounds(n, k, ch)
        most = max(most, rounds)
    assert most >= 5


def test_wrong_variants_of_the_model_differ():
    """Cases built so that each mistake shows: two streaming rounds at least, ties that the cut falls into."""
    ch, k = 8, 4
    # all equal: positions 0..3 win; the carried ones must stay in front of every new candidate
    keys = np.full(40, 9, np.uint32)
    assert SR.final_rounds(40, k, ch) >= 2
    good = SR.stream_model(keys, k, U32, False, ch)
    assert list(good[1]) == [0, 1, 2, 3]
    for variant in ("carried_after", "unstable_cut", "cut_early", "cut_late"):
        bad = SR.stream_model(keys, k, U32, False, ch, variant)
        assert not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])), variant
    # a tie run across the first round's boundary with smaller keys behind it: the cut falls inside the run in round two
    keys = np.full(48, 9, np.uint32)
    keys[[30, 41]] = 1
    good = SR.stream_model(keys, k, U32, False, ch)
    assert list(good[0]) == [1, 1, 9, 9] and list(good[1]) == [30, 41, 0, 1]
    for variant in ("carried_after", "unstable_cut", "cut_early", "cut_late"):
        bad = SR.stream_model(keys, k, U32, False, ch, variant)
        assert not (np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])), variant
    # distinct keys: no variant of the TIE handling can show, the order of carried and new does not matter either
    keys = np.random.default_rng(3).permutation(48).astype(np.uint32)
    good = SR.stream_model(keys, k, U32, False, ch)
    for variant in ("carried_after", "unstable_cut"):
        bad = SR.stream_model(keys, k, U32, False, ch, variant)
        assert np.array_equal(bad[0], good[0]) and np.array_equal(bad[1], good[1])


# ------------------------------------------------------------------------------------------------ front ends --
def test_device_topk_segmented_size_query_phase(gs):
    """d_temp_storage=None returns the size and touches nothing: no tensor is needed."""
    n, S, k = 300000, 40, 200
    D = gs.DeviceTopKSegmented
    for fn in (D.MinKeys, D.MaxKeys):
        assert fn(None, 0, None, None, None, n, S, None, None, k) == gs.lib.gs_topk_segmented_temp_bytes(n, S, k, 0) > 4096
    for fn in (D.MinPairs, D.MaxPairs):
        assert fn(None, 0, None, None, None, None, None, n, S, None, None, k) == gs.lib.gs_topk_segmented_temp_bytes(n, S, k, 1)
    assert D.MinKeys(None, 0, None, None, None, n, S, None, None, 2000) == 0      # refused: k > max k
    assert callable(gs.topk_segmented) and "DeviceTopKSegmented" in gs.__all__ and "topk_segmented" in gs.__all__


def test_topk_segmented_argument_checks_need_no_device(gs):
    import torch
    t = torch.zeros(10, dtype=torch.int32)
    off = torch.tensor([0, 4, 10], dtype=torch.int32)
    with pytest.raises(ValueError):
        gs.topk_segmented(t, off, 2, values=t, indices=True)
    with pytest.raises(TypeError):
        gs.topk_segmented(t.reshape(2, 5), off, 2)
    with pytest.raises(TypeError):
        gs.topk_segmented(t, off.long(), 2)
    with pytest.raises(TypeError):
        gs.topk_segmented(t.long(), off, 2)
    with pytest.raises(ValueError):
        gs.topk_segmented(t, off, 2, end_offsets=off[:2])
    with pytest.raises(ValueError):
        gs.topk_segmented(t, off, 2, values=torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError):
        gs.topk_segmented(t, off, -1)
    ko, vo, counts = gs.topk_segmented(t, off, 0, indices=True)
    assert tuple(ko.shape) == (2, 0) and tuple(vo.shape) == (2, 0) and tuple(counts.shape) == (2,)


def test_status_of_refused_and_noop_shapes_needs_no_device(gs):
    """A refused shape returns hipErrorInvalidValue and zeros, a no-op shape 0 and zeros: nothing is left of what the array held."""
    for n, S, k, rc in ((5000, 3, 1025, INVALID), (1 << 31, 3, 8, INVALID), (5000, 1 << 23, 512, INVALID), (0, 3, 8, 0), (5000, 0, 8, 0),
                        (5000, 3, 0, 0)):
        out = (C.c_uint32 * 8)(*([9] * 8))
        assert gs.lib.gs_topk_segmented_status(BASE, n, S, k, 1, out, None) == rc and list(out) == [0] * 8, (n, S, k)
    assert gs.lib.gs_topk_segmented_status(BASE, 5000, 3, 8, 1, None, None) == INVALID
