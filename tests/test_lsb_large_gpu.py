"""GPU tests of the stable sort above 2^32 elements (gs_lsb_sort_large, DeviceRadixSortLarge) and of its device check
gs_check_sorted_stable.

Small arrays take the 64-bit passes through the test hook GS_MSB_LARGE_TEST_LIMIT=k (read on every call), which lowers the slice
size to k elements: multi-slice passes, ragged last slices and slices of one tile.  A stable sort's output is unique, so keys AND
values must equal, bit for bit, the oracle's stable order (oracle.lsb_reference_ranks / _u64 of the key type's order-preserving
map, masked to the bit range, descending by reverse / stable sort / reverse).  Sizes above 2^32 run in a child process
(tools/lsb_large_check.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from guarded import Arena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_ENV = "GS_MSB_LARGE_TEST_LIMIT"
INVALID = 1
U32, I32, F32, U64, I64, F64 = range(6)
UINT = {4: np.uint32, 8: np.uint64}
TDT = {4: torch.int32, 8: torch.int64}
COMBOS = [(4, 0, U32), (4, 4, I32), (4, 8, F32), (8, 0, U64), (8, 4, I64), (8, 8, F64)]   # (key bytes, value bytes, key type)


# ------------------------------------------------------------------------------------------------------ reference --
def ordmap(keys, kt):
    """The key type's order-preserving unsigned map (-0.0 before +0.0, NaNs by their bits), in the keys' own width."""
    t = keys.dtype.type
    bits = 8 * keys.dtype.itemsize
    sign = t(1 << (bits - 1))
    if kt in (I32, I64):
        return keys ^ sign
    if kt in (F32, F64):
        return np.where(keys & sign != 0, ~keys, keys | sign).astype(keys.dtype)
    return keys


def ranks(oracle, keys, kt, bb, eb, desc):
    m = ordmap(keys, kt)
    if keys.dtype == np.uint32:
        return oracle.lsb_reference_ranks(m, bb, eb, desc).astype(np.int64)
    return oracle.lsb_reference_ranks_u64(m, U64, bb, eb, desc).astype(np.int64)


def gen_keys(kb, kt, kind, n, seed):
    ut = UINT[kb]
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    if kb == 4:
        k = (k >> np.uint64(32)).astype(np.uint32)
    if kind == "equal":
        k[:] = k[0]
    elif kind == "few":                        # 5 distinct values
        k = k[:5][rng.integers(0, 5, size=n)]
    elif kind == "zipf":
        k = (rng.zipf(1.3, size=n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(ut)
    elif kind == "special":
        if kt in (F32, F64):
            ft = np.float32 if kb == 4 else np.float64
            tiny = np.finfo(ft).smallest_subnormal
            sp = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 1.5, -1.5, np.nan, -np.nan], ft).view(ut)
            sp = np.concatenate([sp, np.array([0x7FC00001 if kb == 4 else 0x7FF8000000000001], ut)])   # a NaN payload
        else:
            mx = np.iinfo(ut).max
            sp = np.array([0, 1, mx, mx - 1, mx >> 1, (mx >> 1) + 1], ut)        # MIN, MAX, -1, 0 of the signed types
        idx = rng.random(n) < 0.6
        k[idx] = sp[rng.integers(0, sp.size, size=int(idx.sum()))]
    return k


# ----------------------------------------------------------------------------------------------------------- sort --
def _tensor(a, dev):
    return torch.from_numpy(a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).copy()).to(dev)


def sort_large(gs, dev, keys, kt, vb, bb, eb, desc, sel0=0, fn=None):
    """gs_lsb_sort_large (or `fn` with the same arguments) on keys with enumerated values of vb bytes: (keys, values, selector)."""
    n, kb = keys.size, keys.dtype.itemsize
    kbuf = [_tensor(keys, dev), torch.full((max(n, 1),), -1, dtype=TDT[kb], device=dev)]
    if sel0:
        kbuf.reverse()
    vbuf = None
    if vb:
        vbuf = [torch.arange(n, dtype=TDT[vb], device=dev), torch.full((max(n, 1),), -1, dtype=TDT[vb], device=dev)]
        if sel0:
            vbuf.reverse()
    fn = fn or gs.lib.gs_lsb_sort_large
    nbytes = gs.lib.gs_lsb_large_temp_bytes(n, kb, vb)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    sel = C.c_int(sel0)
    kk = (C.c_void_p * 2)(kbuf[0].data_ptr(), kbuf[1].data_ptr())
    vv = (C.c_void_p * 2)(vbuf[0].data_ptr(), vbuf[1].data_ptr()) if vb else None
    rc = fn(ws.data_ptr(), nbytes, kk, vv, C.byref(sel), n, kb, vb, bb, eb, int(desc), kt, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out_k = kbuf[sel.value].cpu().numpy().view(keys.dtype)[:n]
    out_v = vbuf[sel.value].cpu().numpy()[:n].astype(np.int64) if vb else None
    return out_k, out_v, sel.value


def check(gs, oracle, dev, keys, kt, vb, bb=0, eb=None, desc=False):
    eb = 8 * keys.dtype.itemsize if eb is None else eb
    got_k, got_v, sel = sort_large(gs, dev, keys, kt, vb, bb, eb, desc)
    r = ranks(oracle, keys, kt, bb, eb, desc)
    assert np.array_equal(got_k, keys[r]), "keys"
    if vb:
        assert np.array_equal(got_v, r), "values"
    passes = (eb - bb + 7) // 8
    assert sel == passes % 2, "selector"


# -------------------------------------------------------------------------------------------------------- tests --
LIMITS = [256, 4096, 8191, 8192, 8193, 1 << 15]


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_every_combination_both_orders(gs, oracle, cuda, monkeypatch, kb, vb, kt, limit):
    """n = q * k + 1: q full slices and a last slice of one element; k = 256 gives slices of one partial tile, 4096 and 8192
    the edges of the wide and u32 tiles."""
    monkeypatch.setenv(LIMIT_ENV, str(limit))
    q = 40 if limit < 4096 else (25 if limit < 1 << 15 else 20)
    n = q * limit + 1
    keys = gen_keys(kb, kt, "uniform", n, limit + kb + vb)
    for desc in (False, True):
        check(gs, oracle, cuda, keys, kt, vb, desc=desc)


RANGES = [(kb, vb, kt, bb, eb) for kb, vb, kt in COMBOS for bb, eb in [(0, 8), (3, 29), (20, 21), (5, 61), (0, 64), (31, 33)]
          if eb <= 8 * kb]


@pytest.mark.parametrize("kb,vb,kt,bb,eb", RANGES)
def test_bit_ranges(gs, oracle, cuda, monkeypatch, kb, vb, kt, bb, eb):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    keys = gen_keys(kb, kt, "uniform", 61_441, bb * 100 + eb)
    check(gs, oracle, cuda, keys, kt, vb, bb, eb, desc=bool(bb % 2))


@pytest.mark.parametrize("kind", ["equal", "few", "zipf"])
@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_skewed_inputs(gs, oracle, cuda, monkeypatch, kb, vb, kt, kind):
    monkeypatch.setenv(LIMIT_ENV, "8192")
    keys = gen_keys(kb, kt, kind, 200_003, kb * 10 + vb)
    for desc in (False, True):
        check(gs, oracle, cuda, keys, kt, vb, desc=desc)


@pytest.mark.parametrize("kb,vb,kt", [(4, 0, I32), (4, 4, F32), (4, 8, I32), (8, 0, F64), (8, 4, I64), (8, 8, F64), (8, 8, I64),
                                      (4, 0, F32)])
def test_special_keys(gs, oracle, cuda, monkeypatch, kb, vb, kt):
    """MIN / MAX of the signed types; +-0.0, +-inf, subnormals and NaNs of the floats, in the order the existing sorts give."""
    monkeypatch.setenv(LIMIT_ENV, "4096")
    keys = gen_keys(kb, kt, "special", 100_001, kt * 7 + vb)
    for desc in (False, True):
        check(gs, oracle, cuda, keys, kt, vb, desc=desc)
        check(gs, oracle, cuda, keys, kt, vb, 4, 8 * kb - 3, desc=desc)


@pytest.mark.parametrize("kb,vb,kt", [(4, 4, U32), (8, 8, U64)])
def test_selector_flips_once_per_pass(gs, cuda, monkeypatch, kb, vb, kt):
    """Start on either half; after ceil((end - begin) / 8) passes the result (keys and values) is in the half *selector names."""
    monkeypatch.setenv(LIMIT_ENV, "4096")
    n = 30_011
    keys = gen_keys(kb, kt, "uniform", n, 5)
    for bits in range(1, 8 * kb + 1, 5):
        for sel0 in (0, 1):
            k, v, sel = sort_large(gs, cuda, keys, kt, vb, 0, bits, False, sel0=sel0)
            assert sel == sel0 ^ (((bits + 7) // 8) % 2), (bits, sel0)
            m = keys & UINT[kb]((1 << bits) - 1) if bits < 64 else keys
            order = np.argsort(m, kind="stable")
            assert np.array_equal(k, keys[order]) and np.array_equal(v, order), (bits, sel0)


@pytest.mark.parametrize("kb,vb,kt", COMBOS)
def test_without_the_hook_same_result_as_the_plain_sort(gs, cuda, monkeypatch, kb, vb, kt):
    """Arrays of one slice take gs_lsb_sort_u32 / gs_lsb_sort_wide: keys, values and selector bit-identical to a direct call."""
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    keys = gen_keys(kb, kt, "special" if kt != U32 else "few", 300_007, 77 + kb + vb)
    plain = gs.lib.gs_lsb_sort_u32 if kb == 4 and vb != 8 else gs.lib.gs_lsb_sort_wide
    for bb, eb, desc in [(0, 8 * kb, False), (0, 8 * kb, True), (3, 8 * kb - 5, True)]:
        a = sort_large(gs, cuda, keys, kt, vb, bb, eb, desc)
        if plain is gs.lib.gs_lsb_sort_u32:
            def direct(ws, nb, kk, vv, sel, n, kb_, vb_, bb_, eb_, d, kt_, s):
                return plain(ws, nb, kk, vv, sel, n, bb_, eb_, d, kt_, s)
        else:
            direct = plain
        b = sort_large(gs, cuda, keys, kt, vb, bb, eb, desc, fn=direct)
        assert a[2] == b[2] and np.array_equal(a[0], b[0])
        if vb:
            assert np.array_equal(a[1], b[1])


def test_check_sorted_stable_counts_what_it_should(gs, cuda):
    """The device check counts order breaks on the bit range and, with row ids, equal sort keys out of row-id order."""
    lib = gs.lib
    res = torch.zeros(1, dtype=torch.int64, device=cuda)

    def run(keys, rowids, kt, bb, eb, desc):
        k = _tensor(keys, cuda)
        r = torch.from_numpy(rowids.astype(np.int64)).to(cuda) if rowids is not None else None
        assert lib.gs_check_sorted_stable(k.data_ptr(), r.data_ptr() if r is not None else None, keys.size, keys.dtype.itemsize, kt,
                                          bb, eb, int(desc), res.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return int(res.item())

    k = np.array([1, 2, 2, 3, 0x80000000], np.uint32)
    assert run(k, None, U32, 0, 32, False) == 0
    assert run(k, None, I32, 0, 32, False) == 1                        # 0x80000000 is INT_MIN: first, not last
    assert run(k[::-1].copy(), None, U32, 0, 32, True) == 0
    assert run(k, np.array([0, 5, 4, 1, 2]), U32, 0, 32, False) == 1   # the tie (2, 2) has row ids 5, 4
    assert run(k, np.array([0, 4, 4, 1, 2]), U32, 0, 32, False) == 1   # ... or a repeated one
    assert run(k, np.array([0, 4, 5, 1, 2]), U32, 1, 2, False) == 2    # bit 1 only (0 1 1 1 0): one break, and the tie 2, 3
                                                                       # has row ids 5, 1
    f = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], np.float64).view(np.uint64)
    assert run(f, None, F64, 0, 64, False) == 0
    assert run(f[::-1].copy(), None, F64, 0, 64, True) == 0
    assert run(f[::-1].copy(), None, F64, 0, 64, False) == f.size - 1
    assert run(np.zeros(3, np.uint64), np.array([2, 1, 0]), U64, 0, 0, False) == 2


# ------------------------------------------------------------------------------------------------ buffer contract --
PLACEMENTS = {"P0": (0, 0), "P1": (1, 1), "P2+255": (0, 255)}     # name -> (data offset in elements, workspace offset in bytes)


def _arena_call(gs, cuda, calls, pl, fill, seed, short=False):
    """Place every call's buffers and ONE workspace (the largest query; `short`: one byte less) in a guarded arena, enqueue the
    calls one behind the other, check guards and (unless refused) every result against numpy's stable order."""
    doff, woff = PLACEMENTS[pl]
    A = Arena(cuda, seed=seed, all_const=short)
    prepared = []
    for i, (n, kb, vb, kt, bb, eb, desc, kind) in enumerate(calls):
        t = "c%d_" % i
        keys = gen_keys(kb, kt, kind, n, seed + i)
        A.add(t + "k0", kb * n, doff * kb, data=keys).add(t + "k1", kb * n, doff * kb, fill)
        vals = np.arange(n, dtype=UINT[vb]) if vb else None
        if vb:
            A.add(t + "v0", vb * n, doff * vb, data=vals).add(t + "v1", vb * n, doff * vb, fill)
        prepared.append((t, n, kb, vb, kt, bb, eb, desc, keys, vals, gs.lib.gs_lsb_large_temp_bytes(n, kb, vb)))
    wsz = max(p[-1] for p in prepared)
    A.add("ws", wsz - 1 if short else wsz, woff, fill)
    A.build()
    sels = []
    for t, n, kb, vb, kt, bb, eb, desc, keys, vals, q in prepared:
        sel = C.c_int(0)
        kk = (C.c_void_p * 2)(A.ptr(t + "k0"), A.ptr(t + "k1"))
        vv = (C.c_void_p * 2)(A.ptr(t + "v0"), A.ptr(t + "v1")) if vb else None
        rc = gs.lib.gs_lsb_sort_large(A.ptr("ws"), q - 1 if short else q, kk, vv, C.byref(sel), n, kb, vb, bb, eb, int(desc), kt, None)
        assert rc == (INVALID if short else 0), rc
        sels.append(sel.value)
    A.check()
    if short:
        return
    for (t, n, kb, vb, kt, bb, eb, desc, keys, vals, q), sel in zip(prepared, sels):
        m = (ordmap(keys, kt).astype(np.uint64) >> np.uint64(bb)) & np.uint64((1 << (eb - bb)) - 1)
        order = np.argsort(~m if desc else m, kind="stable")
        assert np.array_equal(A.read(t + "k%d" % sel, UINT[kb]), keys[order]), (t, "keys")
        if vb:
            assert np.array_equal(A.read(t + "v%d" % sel, UINT[vb]), vals[order]), (t, "values")


@pytest.mark.parametrize("pl,fill", [("P0", "00"), ("P1", "random"), ("P1", "ff"), ("P2+255", "random"), ("P2+255", "ff")])
def test_buffer_contract_placements(gs, cuda, monkeypatch, pl, fill):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    for i, (kb, vb, kt) in enumerate(COMBOS):
        _arena_call(gs, cuda, [(50_001, kb, vb, kt, 0, 8 * kb, bool(i % 2), "special" if kt != U32 else "few")], pl, fill, seed=i)


@pytest.mark.parametrize("pl", ["P1", "P2+255"])
def test_dirty_workspace_reused(gs, cuda, monkeypatch, pl):
    """Two calls through one workspace on one stream, the second with another size, type and bit range."""
    monkeypatch.setenv(LIMIT_ENV, "4096")
    _arena_call(gs, cuda, [(100_003, 8, 8, F64, 0, 64, True, "special"), (9_217, 4, 4, I32, 3, 29, False, "zipf")], pl, "random", seed=9)
    _arena_call(gs, cuda, [(70_001, 4, 8, U32, 0, 32, False, "few"), (4_097, 8, 0, I64, 5, 61, True, "uniform")], pl, "ff", seed=10)


@pytest.mark.parametrize("pl", ["P0", "P1"])
def test_short_workspace_is_refused_and_touches_nothing(gs, cuda, monkeypatch, pl):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    for kb, vb, kt in COMBOS:
        _arena_call(gs, cuda, [(40_001, kb, vb, kt, 0, 8 * kb, False, "uniform")], pl, "random", seed=kb + vb, short=True)
        _arena_call(gs, cuda, [(1_000, kb, vb, kt, 0, 8 * kb, False, "uniform")], pl, "random", seed=kb + vb, short=True)


# ------------------------------------------------------------------------------------------------------- capture --
@pytest.mark.parametrize("kb,vb,kt", [(4, 4, F32), (8, 8, I64)])
def test_capture_and_replay(gs, cuda, monkeypatch, kb, vb, kt):
    """One multi-slice call captured into a graph on a side stream (a linear chain of kernels); replayed on fresh input copied
    into the same buffers, it gives what an eager call gives."""
    monkeypatch.setenv(LIMIT_ENV, "8192")
    n = 100_003
    k0, k1 = torch.empty(n, dtype=TDT[kb], device=cuda), torch.empty(n, dtype=TDT[kb], device=cuda)
    v0, v1 = torch.empty(n, dtype=TDT[vb], device=cuda), torch.empty(n, dtype=TDT[vb], device=cuda)
    nbytes = gs.lib.gs_lsb_large_temp_bytes(n, kb, vb)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    kk = (C.c_void_p * 2)(k0.data_ptr(), k1.data_ptr())
    vv = (C.c_void_p * 2)(v0.data_ptr(), v1.data_ptr())
    sel = C.c_int(0)
    first = gen_keys(kb, kt, "special", n, 1)
    k0.copy_(_tensor(first, cuda))
    v0.copy_(torch.arange(n, dtype=TDT[vb], device=cuda))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            rc = gs.lib.gs_lsb_sort_large(ws.data_ptr(), nbytes, kk, vv, C.byref(sel), n, kb, vb, 0, 8 * kb, 1, kt, s.cuda_stream)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert rc == 0 and sel.value == 0                                # 4 or 8 passes: the result is in half 0
    for rep in range(3):
        keys = gen_keys(kb, kt, "special" if rep % 2 else "few", n, 10 + rep)
        k0.copy_(_tensor(keys, cuda))
        v0.copy_(torch.arange(n, dtype=TDT[vb], device=cuda))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = sort_large(gs, cuda, keys, kt, vb, 0, 8 * kb, True)
        assert np.array_equal(k0.cpu().numpy().view(UINT[kb]), eager[0]), rep
        assert np.array_equal(v0.cpu().numpy().astype(np.int64), eager[1]), rep
    del g


# ---------------------------------------------------------------------------------------- public surfaces, driver --
def test_python_device_radix_sort_large(gs, cuda, monkeypatch):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    n = 50_001
    rng = np.random.default_rng(3)
    x = rng.integers(-1000, 1000, size=n).astype(np.int64)
    L = gs.DeviceRadixSortLarge
    for desc in (False, True):
        dk = gs.DoubleBuffer(torch.from_numpy(x.copy()).to(cuda), torch.empty(n, dtype=torch.int64, device=cuda))
        dv = gs.DoubleBuffer(torch.arange(n, dtype=torch.int64, device=cuda), torch.empty(n, dtype=torch.int64, device=cuda))
        nbytes = (L.SortPairsDescending if desc else L.SortPairs)(None, 0, dk, dv, n)
        temp = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        (L.SortPairsDescending if desc else L.SortPairs)(temp, nbytes, dk, dv, n)          # key type from the dtype: GS_KEY_I64
        order = np.argsort(-x if desc else x, kind="stable")
        assert dk.selector == 0 and dv.selector == 0
        assert np.array_equal(dk.Current().cpu().numpy(), x[order]) and np.array_equal(dv.Current().cpu().numpy(), order)
    f = rng.standard_normal(n).astype(np.float32)
    dk = gs.DoubleBuffer(torch.from_numpy(f.copy()).to(cuda), torch.empty(n, dtype=torch.float32, device=cuda))
    nbytes = L.SortKeysDescending(None, 0, dk, n)
    L.SortKeysDescending(torch.empty(nbytes, dtype=torch.uint8, device=cuda), nbytes, dk, n)
    assert np.array_equal(dk.Current().cpu().numpy(), np.sort(f)[::-1])
    dk = gs.DoubleBuffer(torch.from_numpy(f.copy()).to(cuda), torch.empty(n, dtype=torch.float32, device=cuda))
    nbytes = L.SortKeys(None, 0, dk, n, 24, 32)
    L.SortKeys(torch.empty(nbytes, dtype=torch.uint8, device=cuda), nbytes, dk, n, 24, 32)   # the top byte: one pass
    assert dk.selector == 1
    m = ordmap(f.view(np.uint32), F32) >> np.uint32(24)
    assert np.array_equal(dk.Current().cpu().numpy(), f[np.argsort(m, kind="stable")])


@pytest.mark.parametrize("args", [["keys"], ["keys", "desc"], ["pairs", "3:29"], ["u64", "desc"], ["u64", "5:61"], ["rowid"],
                                  ["rowid", "desc"], ["rowid", "desc", "20:32"]])
def test_lsb_large_driver(args):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "lsb_large")
    out = subprocess.run([exe, str((1 << 22) + 77)] + args, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **{LIMIT_ENV: str(1 << 20)}))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "verified=1" in out.stdout and "disorder=0" in out.stdout


# ------------------------------------------------------------------------------------------------------ above 2^32 --
def test_above_2p32(cuda):
    """2^33 u32 keys; u32 keys with u64 row ids at 2^32 + 2^21 + 7 over few distinct values, both orders; i64 keys with row ids
    on a bit range; (u32, u32) pairs against the row-id run -- checked on the device (tools/lsb_large_check.py), in a child
    process.  The i64 case holds about 160 GiB."""
    free, _ = torch.cuda.mem_get_info()
    if free < 170 * (1 << 30):
        pytest.skip("needs 170 GiB of free device memory, %.0f GiB free" % (free / (1 << 30)))
    tool = os.path.join(ROOT, "tools", "lsb_large_check.py")
    cases = ["keys_2p33", "rowid", "pairs32", "rowid_desc", "i64_bits"]   # (pairs32 compares with the rowid run)
    out = subprocess.run([sys.executable, tool] + cases, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("-> OK") == len(cases), out.stdout[-3000:]
