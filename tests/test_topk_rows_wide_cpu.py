"""gs_topk_rows_u64 without a device: the per-row reference against a plain sorted(), the 64-bit image round trips, the widen
identity of the header on the numpy references, the chunked scheme's model at 64 bits, every refusal and no-op of the
contract, the workspace query against the header's formula and against the 32-bit query, the argument checks of the Python
front ends, and every builder of an edge input held to what it is meant to build."""
import numpy as np
import pytest

import topk_ref as R
import topk_rows_ref as RR
import topk_rows_wide_ref as N
import topk_wide_ref as W
from topk_cases import gen

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U64, I64, F64 = N.U64, N.I64, N.F64
CH = RR.CH


# --------------------------------------------------------------------------------------------- the reference --
def test_reference_against_a_plain_sorted_per_row():
    rng = np.random.default_rng(64)
    for case in range(60):
        kt, desc, mode = N.KEY_TYPES[case % 3], bool((case // 3) % 2), N.MODES[(case // 6) % 3]
        rows, cols = int(rng.integers(1, 5)), int(rng.integers(1, 70))
        stride, k = cols + int(rng.integers(0, 3)), int(rng.integers(1, cols + 1))
        mat = N.matrix64(rows, cols, kt, seed=case, stride=stride, kinds=["five", "special", "small", "normal", "uniform"])
        mat[:, cols:] = rng.integers(0, 1 << 63, (rows, stride - cols), dtype=np.uint64)
        vals = rng.integers(0, 1 << 32, mat.shape, dtype=np.uint64).astype(np.uint32) if mode == N.PAIRS else None
        gk, gv = N.rows_topk64(mat, cols, k, kt, desc, vals)
        for r in range(rows):
            img = [int(x) for x in N.image(mat[r, :cols], kt, desc)]
            order = sorted(range(cols), key=lambda c: (img[c], c))[:k]
            assert gk[r].tolist() == [int(mat[r, c]) for c in order], (case, r)
            assert gv[r].tolist() == [int(vals[r, c]) if vals is not None else c for c in order], (case, r)


@pytest.mark.parametrize("kt", N.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_image_round_trips(kt, descending):
    keys = np.concatenate([W.gen64(kind, 5000, seed=7, kt=kt) for kind in W.DISTS] + [W.specials64(kt)])
    img = N.image(keys, kt, descending)
    assert img.dtype == np.uint64 and np.array_equal(N.preimage(img, kt, descending), keys)
    assert np.array_equal(N.image(N.preimage(keys, kt, descending), kt, descending), keys)
    assert np.array_equal(N.image(keys, kt, not descending), ~img)


def test_image_orders_the_doubles_as_stated_at_the_enum():
    """Negative NaNs, -inf, ..., -0, +0, ..., +inf, positive NaNs; the pad image is the positive NaN of all ones."""
    ninf, pinf, one, s = 0xFFF0000000000000, 0x7FF0000000000000, 0x3FF0000000000000, 1 << 63
    seq = np.array([0xFFFFFFFFFFFFFFFF, ninf + 1, ninf, one | s, s | 1, s, 0, 1, one, pinf, pinf + 1, 0x7FFFFFFFFFFFFFFF], np.uint64)
    img = [int(x) for x in N.image(seq, F64)]
    assert img == sorted(img) and len(set(img)) == len(img) and img[0] == 0 and img[-1] == 0xFFFFFFFFFFFFFFFF
    assert [int(x) for x in N.image(seq, F64, True)] == [0xFFFFFFFFFFFFFFFF - x for x in img]
    assert [int(x) for x in N.image(np.array([s, s - 1, 0xFFFFFFFFFFFFFFFF, 0], np.uint64), I64)] == [0, 0xFFFFFFFFFFFFFFFF, s - 1, s]


# ----------------------------------------------------------------------------------------- the widen identity --
def _mat32(rows, cols, kt, seed, stride):
    m = np.zeros((rows, stride), np.uint32)
    for r in range(rows):
        m[r, :cols] = gen(("uniform", "zipf", "topbyte", "five")[(r + seed) % 4], cols, seed=seed * 31 + r, kt=kt)
    return m


def test_widen_identity_on_the_references_for_all_three_types():
    """rows_topk64 on (uint64_t)key << 32 with the widened type equals the 32-bit reference on the keys: keys shifted back,
    values and columns unchanged.  Float rows hold both signs (the low half of the image is then two-valued)."""
    rng = np.random.default_rng(3264)
    for case in range(90):
        kt, desc, mode = (R.U32, R.I32, R.F32)[case % 3], bool((case // 3) % 2), N.MODES[(case // 6) % 3]
        cols = int(rng.choice([1, 2, 63, 300, 1024, 1025, 5000, CH + 1]))
        rows, stride = int(rng.integers(1, 4)), cols + int(rng.integers(0, 4))
        k = int(rng.integers(1, min(cols, 1024) + 1))
        mat = _mat32(rows, cols, kt, case, stride)
        if case % 5 == 0:
            mat[:, :cols] &= np.uint32(0x80030000)
        if kt == R.F32 and cols > 1:
            mat[:, 0] &= np.uint32(0x7FFFFFFF)
            mat[:, 1] |= np.uint32(0x80000000)
            lowhalf = N.image(N.widen32(mat[:, :cols]), F64, desc) & np.uint64(0xFFFFFFFF)
            assert all(np.unique(lowhalf[r]).size == 2 for r in range(rows))
        vals = rng.integers(0, 1 << 32, mat.shape, dtype=np.uint64).astype(np.uint32) if mode == N.PAIRS else None
        gk, gv = N.rows_topk64(N.widen32(mat), cols, k, N.WIDE[kt], desc, vals)
        wk, wv = RR.rows_topk(mat, cols, k, kt, desc, vals)
        assert (gk & np.uint64(0xFFFFFFFF) == 0).all() and np.array_equal((gk >> np.uint64(32)).astype(np.uint32), wk), case
        assert np.array_equal(gv, wv), case


def test_widened_image_is_the_32_bit_image_in_the_upper_half():
    keys = np.concatenate([gen("uniform", 4000, seed=1, kt=R.F32), np.array([0, 0x80000000, 0x7FC00001, 0xFFC00001, 0x7F800000], np.uint32)])
    for kt in (R.U32, R.I32, R.F32):
        for desc in (False, True):
            wide = N.image(N.widen32(keys), N.WIDE[kt], desc)
            assert np.array_equal((wide >> np.uint64(32)).astype(np.uint32), R.image(keys, kt, desc))
            assert np.array_equal(np.argsort(wide, kind="stable"), np.argsort(R.image(keys, kt, desc), kind="stable"))


# -------------------------------------------------------------------------------------------- the chunk model --
def test_chunk_model_at_64_bits_agrees_with_the_direct_answer_on_rows_full_of_ties():
    """ch = 16: many chunks and several levels on short rows of eight values, so the cut falls inside runs that cross chunks."""
    rng = np.random.default_rng(16)
    for case in range(120):
        kt, desc = N.KEY_TYPES[case % 3], bool((case // 3) % 2)
        cols = int(rng.integers(1, 400))
        k = int(rng.integers(1, min(cols, 8) + 1))          # k <= ch / 2: every level shrinks its source
        keys = rng.integers(0, 1 << 63, cols, dtype=np.uint64) * np.uint64(2) & np.uint64(0x8000000300000000)
        if case % 4 == 0:
            keys[:] = keys[0]
        mk, mc, levels = N.chunk_model64(keys, k, kt, desc, ch=16)
        ek, ev = N.rows_topk64(keys[None, :], cols, k, kt, desc)
        assert np.array_equal(mk, ek[0]) and np.array_equal(mc, ev[0]), case
        assert levels == len(RR.level_sizes(cols, k, 16))


@pytest.mark.parametrize("shape", RR.PATH3_SHAPES[:4])
def test_chunk_model_at_the_real_chunk_size(shape):
    rows, cols, k, levels = shape
    si = RR.PATH3_SHAPES.index(shape)
    kt, desc = N.KEY_TYPES[si % 3], bool(si % 2)
    mat = N.matrix64(1, cols, kt, seed=70 + si, kinds=["five", "small"])
    ek, ev = N.rows_topk64(mat, cols, k, kt, desc)
    mk, mc, lv = N.chunk_model64(mat[0], k, kt, desc)
    assert lv == levels and np.array_equal(mk, ek[0]) and np.array_equal(mc, ev[0])


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def _call(gs, temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc=0, kt=U64):
    return gs.lib.gs_topk_rows_u64(temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc, kt, None)


@pytest.mark.parametrize("cols", [700, 5000, 20000])
def test_refusals_and_noops_without_a_device(gs, cols):
    rows, stride, k = 50, cols + 3, 100
    need = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1)
    assert need > 0
    span = (rows - 1) * stride + cols
    kin, vin, kout, vout, temp = BASE, BASE + (1 << 26), BASE + (2 << 26), BASE + (3 << 26), BASE + (4 << 26)
    ok = dict(temp=temp, temp_bytes=need, kin=kin, vin=vin, kout=kout, vout=vout, rows=rows, cols=cols, stride=stride, k=k)
    bad = [
        dict(temp=None),                               # NULL workspace
        dict(temp_bytes=need - 1), dict(temp_bytes=0), # too small
        dict(k=cols + 1),                              # k > num_cols
        dict(k=1025, cols=max(cols, 2000), stride=max(cols, 2000)),   # k > max_k
        dict(stride=cols - 1),                         # row_stride < num_cols
        dict(rows=1 << 20, stride=1 << 12, cols=700),  # num_rows * row_stride >= 2^32
        dict(rows=(1 << 32) // stride + 1),
        dict(rows=1 << 23, cols=700, stride=700, k=512),   # num_rows * k >= 2^32
        dict(rows=1 << 32, cols=1, stride=1, k=1),
        dict(kt=0), dict(kt=1), dict(kt=2),            # 32-bit key types
        dict(kt=6), dict(kt=7), dict(kt=8), dict(kt=9), dict(kt=10), dict(kt=11), dict(kt=12), dict(kt=13), dict(kt=-1),
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 4), dict(kout=kout + 4), dict(kin=kin + 1), dict(kout=kout + 2),     # key pointers not 8-byte aligned
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 1), dict(vout=vout + 3),   # a value pointer that is not 4-aligned
        dict(kout=kin), dict(kout=kin + 8 * (span - 1)),   # output inside the keys (8-byte key extents)
        dict(vout=kin + 8 * span - 4), dict(vout=vin), dict(kout=vin + 4 * span - 4),
        dict(vout=kout), dict(vout=kout + 8 * rows * k - 4), dict(kout=vout + 4 * rows * k - 4),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + 8 * span - 4),   # inputs share a byte
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # the arguments and keys-only forms size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 0)
    assert 0 < need0 <= need and _call(gs, **dict(ok, vin=None, vout=None, temp_bytes=need0 - 1)) == INVALID
    # no-ops: nothing is needed
    for kt in N.KEY_TYPES:
        for desc in (0, 1):
            assert _call(gs, None, 0, None, None, None, None, 0, cols, stride, k, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, desc, kt) == 0
            assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 0, desc, kt) == 0
            assert _call(gs, None, 0, kin, None, kout, vout, rows, cols, stride, 0, desc, kt) == 0
    assert _call(gs, None, 0, None, None, None, None, rows, 0, 0, 1) == INVALID          # k > num_cols, even for empty rows
    assert _call(gs, None, 0, None, None, None, None, rows, cols, stride, 0, 0, 2) == INVALID   # a bad key type before the no-op
    assert _call(gs, None, 0, None, None, None, None, 0, cols, cols - 1, k) == INVALID   # a short stride before the no-op


# --------------------------------------------------------------------------------------------- the size query --
COLS = [0, 1, 2, 64, 65, 1024, 1025, 8191, 8192, 8193, 8197, 16384, 16385, 65536, 65537, 151936, 1 << 20, (1 << 23) + 9]
KS = [0, 1, 2, 8, 64, 65, 1000, 1023, 1024]
ROWS = [0, 1, 3, 7, 256, 1000]


def test_temp_bytes_is_the_headers_formula_and_within_the_32_bit_query_and_twice_it(gs):
    for rows in ROWS:
        for cols in COLS:
            for k in KS + [1025, cols + 1]:
                for hv in (0, 1):
                    got = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, hv)
                    narrow = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv)
                    assert got % 256 == 0
                    assert got == N.temp_bytes64(rows, cols, k, hv), (rows, cols, k, hv)
                    assert (got == 0) == (narrow == 0)
                    if got:
                        assert narrow - 256 <= got <= 2 * narrow, (rows, cols, k, hv)
    assert gs.lib.gs_topk_rows_u64_temp_bytes(10, 100, 101, 0) == 0
    assert gs.lib.gs_topk_rows_u64_temp_bytes(10, 5000, 1025, 0) == 0
    assert gs.lib.gs_topk_rows_u64_temp_bytes(1 << 20, 1 << 12, 10, 0) == 0
    assert gs.lib.gs_topk_rows_u64_temp_bytes(1 << 23, 700, 512, 1) == 0
    # paths 1 and 2 copy nothing into the workspace; path 3 keeps 8 B per candidate key and 4 B per column
    assert gs.lib.gs_topk_rows_u64_temp_bytes(1 << 20, 256, 8, 1) == 256 and gs.lib.gs_topk_rows_u64_temp_bytes(1000, 8192, 1024, 1) == 256
    assert gs.lib.gs_topk_rows_u64_temp_bytes(64, 2 * CH, 128, 0) == 8 * 64 * 256 + 256
    assert gs.lib.gs_topk_rows_u64_temp_bytes(64, 2 * CH, 128, 1) == 12 * 64 * 256 + 256


def test_the_plan_answers_for_the_64_bit_entry_point_unchanged(gs):
    for rows, cols, k, levels in RR.PATH3_SHAPES + RR.MIDDLE_SHAPES:
        assert gs.DeviceTopKRows64.Plan(rows, cols, k, True) == gs.DeviceTopKRows.Plan(rows, cols, k, True) == RR.plan(rows, cols, k)
        assert gs.DeviceTopKRows64.Plan(rows, cols, k)[:2] == [3, levels]
    assert gs.DeviceTopKRows64.MaxK() == gs.DeviceTopKRows.MaxK() == RR.MAX_K


# ------------------------------------------------------------------------------------------------ front ends --
def test_device_topk_rows64_size_query_needs_no_tensor(gs):
    rows, cols, k = 40, 30000, 200
    want0, want1 = gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 0), gs.lib.gs_topk_rows_u64_temp_bytes(rows, cols, k, 1)
    assert want1 > want0 > 256
    for kt in (None, gs.GS_KEY_U64, gs.GS_KEY_I64, gs.GS_KEY_F64):
        assert gs.DeviceTopKRows64.MinKeys(None, 0, None, None, rows, cols, cols, k, key_type=kt) == want0
        assert gs.DeviceTopKRows64.MaxKeys(None, 0, None, None, rows, cols, cols, k, key_type=kt) == want0
        assert gs.DeviceTopKRows64.MinPairs(None, 0, None, None, None, None, rows, cols, cols, k, key_type=kt) == want1
        assert gs.DeviceTopKRows64.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k, key_type=kt) == want1
    assert gs.DeviceTopKRows64.MinKeys(None, 0, None, None, rows, cols, cols, 2000) == 0                  # k > max_k
    assert (gs.GS_KEY_U64, gs.GS_KEY_I64, gs.GS_KEY_F64) == N.KEY_TYPES
    for kt in (gs.GS_KEY_U32, gs.GS_KEY_F32, gs.GS_KEY_BF16, gs.GS_KEY_U8):
        with pytest.raises(TypeError):
            gs.DeviceTopKRows64.MinKeys(None, 0, None, None, rows, cols, cols, k, key_type=kt)


def test_device_topk_rows64_type_errors_need_no_device(gs):
    import torch
    tmp = torch.zeros(256, dtype=torch.uint8)
    for dtype in (torch.int32, torch.float32, torch.int16, torch.bfloat16, torch.uint8):
        t = torch.zeros((4, 10), dtype=dtype)
        with pytest.raises(TypeError):
            gs.DeviceTopKRows64.MinKeys(tmp, 256, t, t.clone(), 4, 10, 10, 2)
        with pytest.raises(TypeError):
            gs.DeviceTopKRows64.MaxPairs(tmp, 256, t, t.clone(), None, torch.zeros(8, dtype=torch.int32), 4, 10, 10, 2,
                                         key_type=gs.GS_KEY_I64)
    t = torch.zeros((4, 10), dtype=torch.int64)
    with pytest.raises(TypeError):
        gs.DeviceTopKRows64.MinKeys(tmp, 256, t, t.clone(), 4, 10, 10, 2, key_type=gs.GS_KEY_I32)
    with pytest.raises(TypeError):
        gs.DeviceTopKRows64.MinKeys(tmp, 256, None, None, 4, 10, 10, 2)


def test_topk_rows64_argument_checks_need_no_device(gs):
    import torch
    for dtype in (torch.int64, torch.float64):
        t = torch.zeros((4, 10), dtype=dtype)
        v = torch.zeros((4, 10), dtype=torch.int32)
        with pytest.raises(ValueError):
            gs.topk_rows64(t, 11)
        with pytest.raises(ValueError):
            gs.topk_rows64(t, -1)
        with pytest.raises(ValueError):
            gs.topk_rows64(t, 2, values=v, indices=True)
        with pytest.raises(ValueError):
            gs.topk_rows64(t.t(), 2)
        with pytest.raises(ValueError):
            gs.topk_rows64(t[0], 2)                                         # 1-D
        with pytest.raises(ValueError):
            gs.topk_rows64(t, 2, values=t)                                  # 8-byte values
        with pytest.raises(ValueError):
            gs.topk_rows64(t, 2, values=torch.zeros((4, 9), dtype=torch.int32))
        ko, vo = gs.topk_rows64(t, 0, indices=True)
        assert tuple(ko.shape) == (4, 0) and ko.dtype == dtype and tuple(vo.shape) == (4, 0) and vo.dtype == torch.int32
        ko, vo = gs.topk_rows64(t[:0], 3)
        assert tuple(ko.shape) == (0, 3) and vo is None
    for dtype in (torch.int32, torch.float32, torch.int16, torch.bfloat16, torch.int8):
        with pytest.raises(TypeError):
            gs.topk_rows64(torch.zeros((4, 10), dtype=dtype), 2)
    with pytest.raises(TypeError):
        gs.topk_rows64(torch.zeros((4, 10), dtype=torch.complex64), 2)      # 8 bytes, but no key category


def test_topk_rows_still_refuses_eight_byte_keys(gs):
    import torch
    with pytest.raises(TypeError):
        gs.topk_rows(torch.zeros((4, 10), dtype=torch.int64), 2)
    with pytest.raises(TypeError):
        gs.topk_rows(torch.zeros((4, 10), dtype=torch.float64), 2)
    assert "topk_rows64" in gs.__all__ and "DeviceTopKRows64" in gs.__all__


# ------------------------------------------------------------------------------ the builders of the edge inputs --
@pytest.mark.parametrize("cols", [2, 61, 700, 5000])
def test_one_byte_rows_vary_in_exactly_that_byte(cols):
    for b in range(8):
        img = N.one_byte_rows(3, cols, b, seed=b)
        assert N.differing_bytes(img) == [frozenset([b])] * 3
        assert ((N.differ(img) >> np.uint64(8 * b)) & np.uint64(255) == 255).all()       # every bit of it


def test_one_key_rows_vary_nowhere():
    assert N.differing_bytes(N.one_key_rows(3, 100)) == [frozenset()] * 3
    assert (N.differ(N.one_key_rows(2, 7, W.ONES)) == 0).all()


@pytest.mark.parametrize("cols", [700, 5000, 2 * CH + 9])
def test_outlier_rows_one_element_alone_makes_the_byte_vary(cols):
    for b in (7, 3, 1):
        for at in (0, cols - 1, (cols - 1) // 64 * 64, cols // 2):
            img = N.outlier_rows(2, cols, b, at, seed=at)
            assert N.differing_bytes(img) == [frozenset([0, b])] * 2
            assert N.differing_bytes(np.delete(img, at, axis=1)) == [frozenset([0])] * 2
    assert (cols - 1) // 64 * 64 + 64 > cols - 1 >= (cols - 1) // 64 * 64        # the last, partly filled register of a wave


def test_mixed_constant_rows_differ_from_row_to_row():
    for cols in (64, 700, 1024):
        img, sets = N.mixed_constant_rows(19, cols, seed=cols)
        assert N.differing_bytes(img) == sets
        assert len(set(sets)) == 8 and frozenset() in sets and frozenset(range(8)) in sets
        assert all(sets[r] != sets[r + 1] for r in range(18))                      # neighbours: the waves of one workgroup


def test_chunked_constant_row_has_chunks_with_different_constant_bytes():
    cols = 9 * CH + 33
    img = N.chunked_constant_row(cols, seed=1)
    per_chunk = [N.differing_bytes(img[None, lo:lo + CH])[0] for lo in range(0, cols, CH)]
    assert per_chunk == [frozenset([c % 8]) for c in range(10)]
    assert len(N.differing_bytes(img[None, :])[0]) == 8


def test_small_integers_and_timestamps_share_their_upper_bytes():
    assert all(s <= frozenset([0, 1, 2]) and len(s) == 3 for s in N.differing_bytes(N.image(N.small_int_rows(3, 5000, 1), I64)))
    ts = N.differing_bytes(N.image(N.timestamp_rows(3, 5000, 2), I64))
    assert all(7 not in s and 6 not in s and {0, 1, 2, 3} <= s for s in ts)


def test_pad_image_rows_are_the_pad_image_but_for_a_few():
    for kt in N.KEY_TYPES:
        for desc in (False, True):
            img = N.pad_image_rows(4, 300, 5, seed=3)
            assert ((img != W.ONES).sum(axis=1) == [5, 5, 5, 0]).all()
            keys = N.preimage(img, kt, desc)
            assert np.array_equal(N.image(keys, kt, desc).reshape(img.shape), img)
    assert int(N.preimage(np.array([W.ONES]), F64, False)[0]) == 0x7FFFFFFFFFFFFFFF       # the positive NaN of all ones


def test_widen32_is_a_shift():
    k = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)
    assert [int(x) for x in N.widen32(k)] == [0, 1 << 32, 1 << 63, 0xFFFFFFFF00000000]
    assert N.WIDE == {R.U32: U64, R.I32: I64, R.F32: F64}
