"""gs_topk_rows_u16 without a device: the 16-bit image maps (a bijection, and the upper half of the 32-bit image of the
widened key), the widen identity of the header on the numpy references, the chunked scheme's model through the widened
matrix, every refusal and no-op of the contract, the workspace query against the header's formula and against the 32-bit
query, and the argument checks of the Python front end."""
import numpy as np
import pytest

import topk_ref as R
import topk_rows_ref as RR
import topk_rows_narrow_ref as N

INVALID = 1             # hipErrorInvalidValue
BASE = 0x7F0000000000   # fake device addresses: a refused call dereferences nothing
U16, I16, F16, BF16 = N.U16, N.I16, N.F16, N.BF16
ALL = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


# ------------------------------------------------------------------------------------------------- the image --
@pytest.mark.parametrize("kt", N.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_image16_is_a_bijection_with_its_inverse(kt, descending):
    img = N.image16(ALL, kt, descending)
    assert img.dtype == np.uint16 and np.unique(img).size == 1 << 16
    assert np.array_equal(N.preimage16(img, kt, descending), ALL)
    assert np.array_equal(N.image16(N.preimage16(ALL, kt, descending), kt, descending), ALL)


@pytest.mark.parametrize("kt", N.KEY_TYPES)
@pytest.mark.parametrize("descending", [False, True])
def test_image16_is_the_upper_half_of_the_widened_image(kt, descending):
    """image16(p) == image32(p << 16) >> 16, so the two images order every pair of patterns alike (the lower half of the
    32-bit image is a function of the upper one: it never decides)."""
    wide = R.image(N.widen(ALL), N.WIDE[kt], descending)
    img = N.image16(ALL, kt, descending)
    assert np.array_equal((wide >> np.uint32(16)).astype(np.uint16), img)
    o16, o32 = np.argsort(img, kind="stable"), np.argsort(wide, kind="stable")
    assert np.array_equal(o16, o32)
    assert (np.diff(wide[o16].astype(np.int64)) > 0).all()


def test_image16_orders_the_floats_as_stated_at_the_enum():
    """Negative NaNs, -inf, ..., -0, +0, ..., +inf, positive NaNs, for both exponent widths."""
    for kt, ninf, pinf, one in ((F16, 0xFC00, 0x7C00, 0x3C00), (BF16, 0xFF80, 0x7F80, 0x3F80)):
        seq = np.array([0xFFFF, ninf + 1, ninf, one | 0x8000, 0x8001, 0x8000, 0x0000, 0x0001, one, pinf, pinf + 1, 0x7FFF], np.uint16)
        img = N.image16(seq, kt).astype(np.int64)
        assert (np.diff(img) > 0).all() and img[0] == 0 and img[-1] == 0xFFFF
        assert (np.diff(N.image16(seq, kt, True).astype(np.int64)) < 0).all()
    assert N.image16(np.array([0x8000, 0x7FFF, 0xFFFF, 0], np.uint16), I16).tolist() == [0, 0xFFFF, 0x7FFF, 0x8000]


def test_the_generator_covers_the_specials_and_the_pad_image():
    for kt in N.KEY_TYPES:
        keys = N.gen16("special", 4000, seed=3, kt=kt)
        for desc in (False, True):
            assert (N.image16(keys, kt, desc) == 0xFFFF).sum() > 10
        if kt in (F16, BF16):
            inf = 0x7C00 if kt == F16 else 0x7F80
            for p in (0x0000, 0x8000, inf, inf | 0x8000, 0x0001, 0x8001):
                assert (keys == p).any(), hex(p)
            mag = keys & 0x7FFF
            assert ((mag > inf) & (keys < 0x8000)).any() and ((mag > inf) & (keys >= 0x8000)).any()      # NaNs of both signs
    for kind in N.DISTS:
        assert N.gen16(kind, 100, seed=1, kt=U16).dtype == np.uint16


# ----------------------------------------------------------------------------------------- the widen identity --
def test_reference_equals_the_32_bit_reference_on_the_widened_matrix():
    """200 seeded cases over key types, directions and forms, cols up to 3 * CH, heavy ties."""
    rng = np.random.default_rng(1610)
    for case in range(200):
        kt, desc, mode = N.KEY_TYPES[case % 4], bool((case // 4) % 2), N.MODES[(case // 8) % 3]
        cols = int(rng.choice([1, 2, 63, 300, 1024, 1025, 5000, RR.CH, RR.CH + 1, 2 * RR.CH + 7, 3 * RR.CH])) if case % 3 else int(
            rng.integers(1, 3 * RR.CH + 1))
        rows, stride = int(rng.integers(1, 4)), cols + int(rng.integers(0, 4))
        k = int(min(cols, rng.choice([1, 2, 64, 65, 1000, 1024]))) if case % 2 else int(rng.integers(1, min(cols, 1024) + 1))
        kind = N.DISTS[case % len(N.DISTS)]
        mat = N.matrix16(rows, cols, kt, seed=case, stride=stride, kinds=[kind, "five", "special"])
        if case % 5 == 0:
            mat[:, :cols] &= np.uint16(0x8003)          # eight values: the cut falls inside a run of equal keys
        mat[:, cols:] = rng.integers(0, 1 << 16, (rows, stride - cols), dtype=np.uint32).astype(np.uint16)
        vals = rng.integers(0, 1 << 32, mat.shape, dtype=np.uint64).astype(np.uint32) if mode == N.PAIRS else None
        gk, gv = N.rows_topk16(mat, cols, k, kt, desc, vals)
        wk, wv = RR.rows_topk(N.widen(mat), cols, k, N.WIDE[kt], desc, vals)
        what = (case, kt, desc, mode, rows, cols, k, kind)
        assert np.array_equal(gk, (wk >> np.uint32(16)).astype(np.uint16)), what
        assert (wk & np.uint32(0xFFFF) == 0).all() and np.array_equal(gv, wv), what


@pytest.mark.parametrize("shape", RR.PATH3_SHAPES)
def test_chunk_model_through_the_widened_matrix(shape):
    """The numpy model of path 3 (chunks of CH, levels of candidates) on the widened rows gives the 16-bit reference."""
    rows, cols, k, levels = shape
    si = RR.PATH3_SHAPES.index(shape)
    kt, desc = N.KEY_TYPES[si % 4], bool(si % 2)
    mat = N.matrix16(rows, cols, kt, seed=70 + si)
    ek, ev = N.rows_topk16(mat, cols, k, kt, desc)
    for r in range(rows):
        mk, mc, lv = RR.chunk_model(N.widen(mat[r]), k, N.WIDE[kt], desc)
        assert lv == levels
        assert np.array_equal((mk >> np.uint32(16)).astype(np.uint16), ek[r]) and np.array_equal(mc, ev[r]), (shape, r)


# ---------------------------------------------------------------------------------------- refusals and no-ops --
def al4(x):
    return x & ~3       # the 4-byte word that holds byte x


def _call(gs, temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc=0, kt=U16):
    return gs.lib.gs_topk_rows_u16(temp, temp_bytes, kin, vin, kout, vout, rows, cols, stride, k, desc, kt, None)


@pytest.mark.parametrize("cols", [700, 5000, 20000])
def test_refusals_and_noops_without_a_device(gs, cols):
    rows, stride, k = 50, cols + 3, 100
    need = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
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
        dict(kt=3), dict(kt=4), dict(kt=5),            # 64-bit key types
        dict(kt=6), dict(kt=7), dict(kt=12), dict(kt=13), dict(kt=-1),   # 8-bit key types and no type at all
        dict(vout=None),                               # d_vals_in without d_vals_out
        dict(kin=None), dict(kout=None),               # NULL key pointers
        dict(kin=kin + 1), dict(kout=kout + 1), dict(kin=kin + 3),       # a key pointer at an odd byte address
        dict(vin=vin + 2), dict(vout=vout + 2), dict(vin=vin + 1), dict(vout=vout + 3),   # a value pointer that is not 4-aligned
        dict(kout=kin), dict(kout=kin + 2 * (span - 1)),   # output inside the keys (2-byte key extents)
        dict(vout=kin + al4(2 * span - 1)), dict(vout=vin), dict(kout=vin + 4 * span - 2),
        dict(vout=kout), dict(vout=kout + al4(2 * rows * k - 1)), dict(kout=vout + 4 * rows * k - 2),   # outputs share a byte
        dict(vin=kin), dict(vin=kin + al4(2 * span - 1)),   # inputs share a byte
    ]
    for change in bad:
        a = dict(ok, **change)
        assert _call(gs, **a) == INVALID, change
    # the arguments and keys-only forms size their own workspaces
    assert _call(gs, **dict(ok, vin=None, temp_bytes=need - 1)) == INVALID
    need0 = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 0)
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


def test_temp_bytes_is_the_headers_formula_and_never_above_the_32_bit_query(gs):
    for rows in ROWS:
        for cols in COLS:
            for k in KS + [1025, cols + 1]:
                for hv in (0, 1):
                    got = gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, hv)
                    assert got % 256 == 0
                    assert got == N.temp_bytes16(rows, cols, k, hv), (rows, cols, k, hv)
                    assert got <= gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv), (rows, cols, k, hv)
                    assert (got == 0) == (gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv) == 0)
    assert gs.lib.gs_topk_rows_u16_temp_bytes(10, 100, 101, 0) == 0
    assert gs.lib.gs_topk_rows_u16_temp_bytes(10, 5000, 1025, 0) == 0
    assert gs.lib.gs_topk_rows_u16_temp_bytes(1 << 20, 1 << 12, 10, 0) == 0
    assert gs.lib.gs_topk_rows_u16_temp_bytes(1 << 23, 700, 512, 1) == 0
    # paths 1 and 2 copy nothing into the workspace; path 3 keeps 2 B per candidate key and 4 B per column
    assert gs.lib.gs_topk_rows_u16_temp_bytes(1 << 20, 256, 8, 1) == 256 and gs.lib.gs_topk_rows_u16_temp_bytes(1000, 8192, 1024, 1) == 256
    assert gs.lib.gs_topk_rows_u16_temp_bytes(64, 2 * RR.CH, 128, 0) == 2 * 64 * 256 + 256
    assert gs.lib.gs_topk_rows_u16_temp_bytes(64, 2 * RR.CH, 128, 1) == 6 * 64 * 256 + 256


def test_device_topk_rows_size_query_takes_a_key_type(gs):
    rows, cols, k = 40, 30000, 200
    for kt in N.KEY_TYPES:
        assert gs.DeviceTopKRows.MinKeys(None, 0, None, None, rows, cols, cols, k, key_type=kt) == \
            gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 0) > 256
        assert gs.DeviceTopKRows.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k, key_type=kt) == \
            gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
    wide = gs.DeviceTopKRows.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k)
    assert wide == gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1) >= gs.lib.gs_topk_rows_u16_temp_bytes(rows, cols, k, 1)
    assert gs.DeviceTopKRows.MaxPairs(None, 0, None, None, None, None, rows, cols, cols, k, key_type=gs.GS_KEY_F32) == wide
    assert gs.DeviceTopKRows.MinKeys(None, 0, None, None, rows, cols, cols, 2000, key_type=gs.GS_KEY_BF16) == 0     # k > max_k
    assert (gs.GS_KEY_U16, gs.GS_KEY_I16, gs.GS_KEY_F16, gs.GS_KEY_BF16) == N.KEY_TYPES


# ------------------------------------------------------------------------------------------------ front ends --
def test_topk_rows_argument_checks_need_no_device(gs):
    import torch
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        t = torch.zeros((4, 10), dtype=dtype)
        v = torch.zeros((4, 10), dtype=torch.int32)
        with pytest.raises(ValueError):
            gs.topk_rows(t, 11)
        with pytest.raises(ValueError):
            gs.topk_rows(t, 2, values=v, indices=True)
        with pytest.raises(ValueError):
            gs.topk_rows(t.t(), 2)
        with pytest.raises(ValueError):
            gs.topk_rows(t, 2, values=t)                                  # 2-byte values
        with pytest.raises(ValueError):
            gs.topk_rows(t, 2, values=torch.zeros((4, 9), dtype=torch.int32))
        ko, vo = gs.topk_rows(t, 0, indices=True)
        assert tuple(ko.shape) == (4, 0) and ko.dtype == dtype and tuple(vo.shape) == (4, 0) and vo.dtype == torch.int32
        big = torch.zeros((2, 3000), dtype=dtype)
        with pytest.raises(ValueError):
            gs.topk_rows(big, gs.DeviceTopKRows.MaxK() + 1)               # no flat 16-bit top-k to loop over
    with pytest.raises(TypeError):
        gs.topk_rows(torch.zeros((4, 10), dtype=torch.int64), 2)
    with pytest.raises(TypeError):
        gs.topk_rows(torch.zeros((4, 10), dtype=torch.int8), 2)
