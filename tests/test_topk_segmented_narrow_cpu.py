"""gs_topk_segmented_u16 without a device: every refusal and no-op of the contract with its size query, the workspace query
against the header's formula (and never above the 32-bit query), the per-segment reference against the CPU oracle's stable
ranks on the widened keys and against the widening identity, and the routing of the Python front ends by key width."""
import ctypes as C

import numpy as np
import pytest

import topk_ref as R
import topk_segmented_narrow_ref as SN
import topk_segmented_ref as SR
from test_topk_segmented_cpu import KS, NS, SS

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U16, I16, F16, BF16 = SN.KEY_TYPES
CH = SR.CH


def _call(gs, temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc=0, kt=U16):
    return gs.lib.gs_topk_segmented_u16(temp, temp_bytes, kin, vin, kout, vout, counts, n, S, begin, end, k, desc, kt, None)


def _tb(gs, n, S, k, hv):
    return gs.lib.gs_topk_segmented_u16_temp_bytes(n, S, k, hv)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
@pytest.mark.parametrize("n", [700, 5000, 200000])
def test_refusals_and_noops_without_a_device(gs, n):
    S, k = 50, 100
    need = _tb(gs, n, S, k, 1)
    assert need > 0
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, counts=counts, n=n, S=S, begin=begin, end=end, k=k)
    bad = [
        dict(temp=None),                                   # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0),     # one byte short, nothing
        dict(k=1025),                                      # k > max k
        dict(n=1 << 31), dict(n=(1 << 31) + 5),            # int offsets
        dict(S=1 << 23, k=512), dict(S=(1 << 32) - 1, k=2),    # num_segments * k >= 2^32
        dict(kt=0), dict(kt=1), dict(kt=2),                # the 32-bit key types
        dict(kt=3), dict(kt=-1), dict(kt=6), dict(kt=7), dict(kt=12),   # and the others
        dict(vout=None),                                   # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None), dict(begin=None), dict(end=None),   # NULL keys or offsets
        dict(kin=kin + 1), dict(kin=kin + 3), dict(kout=kout + 1), dict(kout=kout + 255),    # odd key pointers
        dict(vin=vin + 2), dict(vin=vin + 3), dict(vout=vout + 2), dict(vout=vout + 1),      # u32 arrays not aligned to 4
        dict(counts=counts + 2), dict(counts=counts + 1), dict(begin=begin + 2), dict(begin=begin + 1), dict(end=end + 2),
        dict(end=end + 3),
        # every pair of arrays sharing a byte, at 2 bytes per key and 4 per value, count and offset
        dict(kout=kin), dict(kout=kin + 2 * (n - 1)), dict(kin=kout + 2 * (S * k - 1)),          # keys_in / keys_out
        dict(vin=kin), dict(vin=kin + 2 * n - 4), dict(kin=vin + 4 * n - 2),                     # keys_in / vals_in
        dict(vout=kin), dict(vout=kin + 2 * n - 4), dict(kin=vout + 4 * S * k - 2),              # keys_in / vals_out
        dict(counts=kin), dict(counts=kin + 2 * n - 4), dict(kin=counts + 4 * S - 2),            # keys_in / counts
        dict(begin=kin + 2 * n - 4), dict(end=kin), dict(kin=begin + 4 * S - 2), dict(kin=end + 4 * S - 2),   # keys_in / offsets
        dict(kout=vin), dict(kout=vin + 4 * n - 2), dict(vin=kout + 2 * S * k - 4),              # vals_in / keys_out
        dict(vout=vin), dict(vout=vin + 4 * (n - 1)), dict(vin=vout + 4 * (S * k - 1)),          # vals_in / vals_out
        dict(counts=vin + 4 * (n - 1)), dict(begin=vin), dict(end=vin + 4 * (n - 1)),            # vals_in / counts, offsets
        dict(vout=kout), dict(vout=kout + 2 * S * k - 4), dict(kout=vout + 4 * S * k - 2),       # keys_out / vals_out
        dict(counts=kout + 2 * S * k - 4), dict(kout=counts + 4 * S - 2),                        # keys_out / counts
        dict(begin=kout), dict(end=kout + 2 * S * k - 4), dict(kout=end + 4 * S - 2),            # keys_out / offsets
        dict(counts=vout + 4 * (S * k - 1)), dict(begin=vout), dict(end=vout + 4 * (S * k - 1)),     # vals_out / counts, offsets
        dict(counts=begin + 4 * (S - 1)), dict(counts=end), dict(begin=counts + 4 * (S - 1)),    # counts / offsets
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # a workspace one byte short refuses what is otherwise in order (an accepted call would launch: not tried on fake addresses)
    short = dict(temp_bytes=need - 1)
    assert _call(gs, **dict(ok, kout=kin + 2 * n, **short)) == INVALID
    assert _call(gs, **dict(ok, counts=None, **short)) == INVALID
    # the offsets may share: S + 1 offsets in one array, or both pointers the same
    assert _call(gs, **dict(ok, end=begin + 4, **short)) == INVALID
    assert _call(gs, **dict(ok, vin=None, **short)) == INVALID
    need0 = _tb(gs, n, S, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed, and the query returns 0
    for kt in SN.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, 0, None, None, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, counts, n, S, begin, end, 0, desc, kt) == 0
    for hv in (0, 1):
        assert _tb(gs, 0, S, k, hv) == 0 and _tb(gs, n, 0, k, hv) == 0 and _tb(gs, n, S, 0, hv) == 0
        # refused shapes: the query returns 0
        assert _tb(gs, n, S, 1025, hv) == 0 and _tb(gs, 1 << 31, S, k, hv) == 0 and _tb(gs, n, 1 << 23, 512, hv) == 0
        assert _tb(gs, n, (1 << 32) - 1, 2, hv) == 0
    for kt in (0, 1, 2, 7, 12):
        assert _call(gs, None, 0, None, None, None, None, None, n, S, None, None, 0, 0, kt) == INVALID   # a bad key type before the no-op
        assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, k, 0, kt) == INVALID
    assert _call(gs, None, 0, None, None, None, None, None, 0, S, None, None, 1025) == INVALID      # k > max k before the no-op
    # k may exceed num_items and every segment's length
    assert _tb(gs, 10, 3, 1024, 1) > 0
    assert _call(gs, **dict(ok, n=10, k=1024, temp_bytes=_tb(gs, 10, S, 1024, 1) - 1)) == INVALID


def test_the_two_offset_arrays_may_share_and_nothing_else(gs):
    """On fake addresses only refusals can be called (an accepted call would launch).  So the allowance is shown from the
    other side: the counts on either offset array are refused with a workspace of the right size; the accepted case, both
    offsets in one array, runs on the device (topk_segmented() in tests/test_topk_segmented_narrow_gpu.py)."""
    n, S, k = 5000, 50, 100
    need = _tb(gs, n, S, k, 1)
    step = 1 << 26
    kin, vin, kout, vout, counts, begin, end, temp = (BASE + i * step for i in range(8))
    assert _call(gs, temp, need, kin, vin, kout, vout, begin, n, S, begin, end, k) == INVALID       # counts on begin
    assert _call(gs, temp, need, kin, vin, kout, vout, end, n, S, begin, end, k) == INVALID         # counts on end
    assert _call(gs, temp, need - 1, kin, vin, kout, vout, counts, n, S, begin, begin, k) == INVALID    # only the workspace


# --------------------------------------------------------------------------------------------- the size query --
def test_temp_bytes_is_the_headers_formula_and_never_above_the_32_bit_query(gs):
    for n in NS:
        for S in SS:
            for k in KS + [1025]:
                for hv in (0, 1):
                    got = _tb(gs, n, S, k, hv)
                    assert got % 256 == 0 and got == SN.temp_bytes16(n, S, k, hv), (n, S, k, hv)
                    assert got <= gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv), (n, S, k, hv)
                    assert (got == 0) == (gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv) == 0)
    rng = np.random.default_rng(7)
    smaller = 0
    for _ in range(400):
        n = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
        S = int(rng.integers(1, 1 << int(rng.integers(1, 23))))
        k = int(rng.integers(1, 1100))
        hv = int(rng.integers(0, 2))
        got, wide = _tb(gs, n, S, k, hv), gs.lib.gs_topk_segmented_temp_bytes(n, S, k, hv)
        assert got == SN.temp_bytes16(n, S, k, hv) and got % 256 == 0 and got <= wide, (n, S, k, hv)
        smaller += got < wide
    assert smaller > 50
    # the long-segment terms vanish when num_items <= CH; one element more brings one record, two task slots and 2 * k images
    for k in (1, 1023, 1024):
        assert _tb(gs, CH, 16, k, 1) == _tb(gs, CH, 16, k, 0) == 4096 + 5 * 256 + 256
        assert _tb(gs, CH + 1, 16, k, 0) == 4096 + 5 * 256 + 256 + 256 + ((2 * k * 2 + 255) & ~255) + 256
        assert _tb(gs, CH + 1, 16, k, 1) == _tb(gs, CH + 1, 16, k, 0) + ((4 * k * 2 + 255) & ~255)
    # the 32-bit query is what it was
    assert gs.lib.gs_topk_segmented_temp_bytes(CH + 1, 16, 1024, 0) == 4096 + 5 * 256 + 256 + 256 + 8192 + 256


def test_temp_bytes_is_monotone(gs):
    """Over the shapes the entry point accepts (a refused shape answers 0)."""
    def tb(n, S, k, hv):
        return None if SR.refused(n, S, k) else _tb(gs, n, S, k, hv)

    def rising(values):
        values = [v for v in values if v is not None]
        assert all(a <= b for a, b in zip(values, values[1:])), values
    fine = list(range(8100, 8300, 3)) + list(range(16300, 16500, 3)) + list(range(3 * CH - 5, 3 * (CH + 1) + 5))
    for S in SS[1:]:
        for k in KS[1:]:
            for n in NS[1:]:
                assert tb(n, S, k, 0) is None or tb(n, S, k, 0) <= tb(n, S, k, 1)
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


def test_plan_and_status_serve_both_widths(gs):
    """One plan function: the geometry is the 32-bit one.  The status of refused and no-op shapes needs no device."""
    assert gs.DeviceTopKSegmented.Plan(20000, 3, 50) == SR.plan(20000, 3, 50) == [7, 10, CH, 2, 4, 1024, 0, 0]
    assert not hasattr(gs.lib, "gs_topk_segmented_u16_plan") and not hasattr(gs.lib, "gs_topk_segmented_u16_status")
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_segmented_status(BASE, 5000, 3, 1025, 1, out, None) == INVALID and list(out) == [0] * 8


# ------------------------------------------------------------------------------------------------ the reference --
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kt", SN.KEY_TYPES)
def test_segment_reference_matches_oracle_ranks_on_the_widened_keys(oracle, kt, descending):
    """The oracle ranks unsigned 32-bit words, so it is given the widened key's ascending 32-bit image and the direction:
    its stable ranks, cut at kept, are the segment's answer.  Ties (30 % one key, and only 65536 patterns), clamped and
    empty segments."""
    rng = np.random.default_rng(11 + kt)
    n = 4000
    keys = SN.NR.gen16("special", n, seed=5, kt=kt)
    keys[rng.random(n) < 0.3] = 0x3C00
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    begin = np.array([0, 10, 500, 3000, 2000, -5, 3990, 100, 100, 1], np.int32)
    end = np.array([10, 400, 500, 3999, 2100, 7, 4100, 50, 101, 3998], np.int32)
    wide_img = R.image(SN.NR.widen(keys), SN.WIDE[kt], False)
    for k in (1, 100, 1024):
        ko, po, counts = SN.seg_topk16(keys, begin, end, k, kt, descending)
        kv, vo, _ = SN.seg_topk16(keys, begin, end, k, kt, descending, vals)
        wk, wp, wc = SN.via_widening(keys, begin, end, k, kt, descending)
        assert np.array_equal(ko, wk) and np.array_equal(po, wp) and np.array_equal(counts, wc)
        assert ko.dtype == np.uint16 and po.dtype == np.uint32
        for s in range(begin.size):
            lo, hi = max(int(begin[s]), 0), min(int(end[s]), n)
            ln = max(hi - lo, 0)
            kept = min(k, ln)
            assert counts[s] == kept
            assert (ko[s, kept:] == SN.FILL16).all() and (po[s, kept:] == SN.FILL).all()
            if kept:
                want = oracle.lsb_reference_ranks(np.ascontiguousarray(wide_img[lo:hi]), 0, 32, descending)[:kept]
                assert np.array_equal(po[s, :kept], want) and np.array_equal(ko[s, :kept], keys[lo:hi][want])
                assert np.array_equal(kv[s, :kept], ko[s, :kept]) and np.array_equal(vo[s, :kept], vals[lo:hi][want])
    assert list(SN.seg_topk16(keys, begin, end, 5, kt)[2]) == [5, 5, 0, 5, 5, 5, 5, 0, 1, 5]


def test_reference_orders_the_specials_as_stated_at_the_enum():
    for kt, ninf, pinf, nnan, pnan in ((F16, 0xFC00, 0x7C00, 0xFE01, 0x7E01), (BF16, 0xFF80, 0x7F80, 0xFFC1, 0x7FC1)):
        keys = np.array([pnan, 0x0000, pinf, 0x8000, ninf, nnan], np.uint16)
        ko, po, _ = SN.seg_topk16(keys, [0], [6], 6, kt)
        assert list(ko[0]) == [nnan, ninf, 0x8000, 0x0000, pinf, pnan] and list(po[0]) == [5, 4, 3, 1, 2, 0]
        ko, _, _ = SN.seg_topk16(keys, [0], [6], 6, kt, True)
        assert list(ko[0]) == [pnan, pinf, 0x0000, 0x8000, ninf, nnan]
    ko, _, _ = SN.seg_topk16(np.array([0x7FFF, 0, 0xFFFF, 0x8000], np.uint16), [0], [4], 4, I16)
    assert list(ko[0]) == [0x8000, 0xFFFF, 0, 0x7FFF]


# ------------------------------------------------------------------------------------------------ front ends --
def test_device_topk_segmented_size_query_takes_a_key_type(gs):
    n, S, k = 300000, 40, 200
    D = gs.DeviceTopKSegmented
    for kt in SN.KEY_TYPES:
        for fn in (D.MinKeys, D.MaxKeys):
            assert fn(None, 0, None, None, None, n, S, None, None, k, key_type=kt) == _tb(gs, n, S, k, 0) > 4096
        for fn in (D.MinPairs, D.MaxPairs):
            assert fn(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=kt) == _tb(gs, n, S, k, 1)
    wide = D.MaxPairs(None, 0, None, None, None, None, None, n, S, None, None, k)
    assert wide == gs.lib.gs_topk_segmented_temp_bytes(n, S, k, 1) > _tb(gs, n, S, k, 1)
    assert D.MaxPairs(None, 0, None, None, None, None, None, n, S, None, None, k, key_type=gs.GS_KEY_F32) == wide
    assert D.MinKeys(None, 0, None, None, None, n, S, None, None, 2000, key_type=gs.GS_KEY_BF16) == 0     # refused: k > max k
    assert (gs.GS_KEY_U16, gs.GS_KEY_I16, gs.GS_KEY_F16, gs.GS_KEY_BF16) == SN.KEY_TYPES


def test_mismatched_tensor_width_and_key_type_raise_type_error(gs):
    """Raised before any buffer check or call: host tensors serve."""
    import torch
    D = gs.DeviceTopKSegmented
    temp = torch.zeros(1 << 16, dtype=torch.uint8)
    off = torch.tensor([0, 4, 10], dtype=torch.int32)
    narrow, wide = torch.zeros(10, dtype=torch.int16), torch.zeros(10, dtype=torch.int32)
    for kt in (gs.GS_KEY_U32, gs.GS_KEY_I32, gs.GS_KEY_F32):
        with pytest.raises(TypeError):
            D.MinKeys(temp, temp.numel(), narrow, torch.zeros(4, dtype=torch.int16), None, 10, 2, off[:-1], off[1:], 2, key_type=kt)
    for kt in SN.KEY_TYPES:
        with pytest.raises(TypeError):
            D.MaxPairs(temp, temp.numel(), wide, torch.zeros(4, dtype=torch.int32), None, torch.zeros(4, dtype=torch.int32), None, 10, 2,
                       off[:-1], off[1:], 2, key_type=kt)
    with pytest.raises(TypeError):      # a 2-byte tensor resolves its own type; 8-byte and 1-byte keys have none
        D.MinKeys(temp, temp.numel(), torch.zeros(10, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), None, 10, 2, off[:-1],
                  off[1:], 2)
    with pytest.raises(TypeError):
        D.MinKeys(temp, temp.numel(), torch.zeros(10, dtype=torch.int8), torch.zeros(4, dtype=torch.int8), None, 10, 2, off[:-1],
                  off[1:], 2)


def test_topk_segmented_argument_checks_on_two_byte_tensors(gs):
    import torch
    off = torch.tensor([0, 4, 10], dtype=torch.int32)
    for dtype in (torch.int16, torch.uint16, torch.float16, torch.bfloat16):
        t = torch.zeros(10, dtype=dtype)
        v = torch.zeros(10, dtype=torch.int32)
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, 2, values=v, indices=True)
        with pytest.raises(TypeError):
            gs.topk_segmented(t.reshape(2, 5), off, 2)
        with pytest.raises(TypeError):
            gs.topk_segmented(t, off.long(), 2)
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, 2, end_offsets=off[:2])
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, 2, values=t)                      # 2-byte values
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, 2, values=torch.zeros(9, dtype=torch.int32))
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, -1)
        with pytest.raises(ValueError):
            gs.topk_segmented(t, off, gs.DeviceTopKSegmented.MaxK() + 1)    # as for 32-bit keys
        ko, vo, counts = gs.topk_segmented(t, off, 0, indices=True)
        assert tuple(ko.shape) == (2, 0) and ko.dtype == dtype and tuple(vo.shape) == (2, 0) and vo.dtype == torch.int32
        assert tuple(counts.shape) == (2,) and counts.dtype == torch.int32
        ko, vo, counts = gs.topk_segmented(t, off[:1], 3)
        assert tuple(ko.shape) == (0, 3) and ko.dtype == dtype and vo is None and tuple(counts.shape) == (0,)
    with pytest.raises(TypeError):
        gs.topk_segmented(torch.zeros(10, dtype=torch.int64), off, 2)
    with pytest.raises(TypeError):
        gs.topk_segmented(torch.zeros(10, dtype=torch.int8), off, 2)
