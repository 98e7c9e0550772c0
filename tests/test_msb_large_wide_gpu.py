"""GPU tests of the wide MSB sort above 2^32 elements (gs_msb_sort_large_wide / rdxsrt_unstable_sort_large_wide): 64-bit
keys with no, 32-bit or 64-bit values, and 32-bit keys with 64-bit values (row ids).

Small arrays reach every path of the planner through the test hook GS_MSB_LARGE_TEST_LIMIT=k (read on every call), which
lowers the group size and the slice size of the 64-bit pass to k elements: multi-slice passes, multi-group finishes, splits
of oversized buckets at every depth, and ranges that stay oversized down to the last byte.  Keys must equal, bit for bit,
numpy's order of the key type's order-preserving map; values are enumerated and every one must be a position whose input
key equals the sorted key next to it.  Sizes above 2^32 run in a child process (tools/large_check.py, the msb_large driver)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_ENV = "GS_MSB_LARGE_TEST_LIMIT"
U32, I32, F32, U64, I64, F64 = 0, 1, 2, 3, 4, 5
COMBOS = [(8, 0), (8, 4), (8, 8), (4, 8)]      # (key bytes, value bytes)


def _ord(keys, kt):
    """The key type's order-preserving unsigned map (-0.0 before +0.0, NaNs by their bits)."""
    bits = 64 if keys.dtype == np.uint64 else 32
    t = keys.dtype.type
    sign = t(1 << (bits - 1))
    if kt in (I32, I64):
        return keys ^ sign
    if kt in (F32, F64):
        return np.where(keys >> t(bits - 1) == 1, ~keys, keys | sign).astype(keys.dtype)
    return keys


def _sort(gs, cuda, keys, kt, vb):
    """Sort `keys` (uint64 or uint32 numpy) with enumerated values of vb bytes (0: none); -> (sorted keys, values)."""
    n = keys.size
    kdt = torch.int64 if keys.dtype == np.uint64 else torch.int32
    dk = torch.from_numpy(keys.view(np.int64 if kdt == torch.int64 else np.int32).copy()).to(cuda)
    ka = torch.empty(max(n, 1), dtype=kdt, device=cuda)
    dv = va = None
    if vb:
        vdt = torch.int64 if vb == 8 else torch.int32
        dv = torch.arange(n, dtype=vdt, device=cuda)
        va = torch.empty(max(n, 1), dtype=vdt, device=cuda)
    seq = gs.rdxsrt_unstable_sort_large_wide(dk, dv, n, ka, va, key_type=kt)
    assert seq.sorted_keys is dk and seq.sorted_values is dv
    out_k = dk.cpu().numpy().view(keys.dtype)[:n]
    return out_k, (dv.cpu().numpy()[:n].astype(np.int64) if vb else None)


def _check(gs, cuda, keys, kt, vb):
    got, vals = _sort(gs, cuda, keys, kt, vb)
    exp = keys[np.argsort(_ord(keys, kt), kind="stable")]
    assert np.array_equal(got, exp)
    if vb:
        assert np.array_equal(np.sort(vals), np.arange(keys.size))       # a permutation of the positions
        assert np.array_equal(keys[vals], got)                           # each pointing at an equal input key


def _keys(kb, kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        k = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    elif kind == "few":
        k = rng.integers(0, 2**64, size=5, dtype=np.uint64)[rng.integers(0, 5, size=n)]
    elif kind == "zipf":
        k = rng.zipf(1.3, size=n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    else:
        raise ValueError(kind)
    return k if kb == 8 else (k >> np.uint64(32)).astype(np.uint32)


@pytest.mark.parametrize("limit", [256, 1000, 4096, 65536])
@pytest.mark.parametrize("kb,vb", COMBOS)
def test_uniform_every_combination_and_limit(gs, cuda, monkeypatch, kb, vb, limit):
    monkeypatch.setenv(LIMIT_ENV, str(limit))
    _check(gs, cuda, _keys(kb, "uniform", 100_003 if limit < 4096 else 400_001, limit + kb + vb), U64 if kb == 8 else U32, vb)


@pytest.mark.parametrize("kb,vb", COMBOS)
@pytest.mark.parametrize("kind", ["few", "zipf"])
def test_skewed_keys(gs, cuda, monkeypatch, kind, kb, vb):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    _check(gs, cuda, _keys(kb, kind, 300_000, 7), U64 if kb == 8 else U32, vb)


def _signed(kb, n, rng):
    if kb == 8:
        k = rng.integers(-2**63, 2**63, size=n, dtype=np.int64)
        k[:500], k[500:1000], k[1000:1500], k[1500:2000] = -2**63, 2**63 - 1, 0, -1
        return k.view(np.uint64)
    k = rng.integers(-2**31, 2**31, size=n, dtype=np.int64).astype(np.int32)
    k[:500], k[500:1000], k[1000:1500], k[1500:2000] = -2**31, 2**31 - 1, 0, -1
    return k.view(np.uint32)


def _floats(kb, n, rng):
    ft = np.float64 if kb == 8 else np.float32
    x = (rng.standard_normal(n) * 1e3).astype(ft)
    tiny = np.finfo(ft).smallest_subnormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, -5 * tiny, np.nan, -np.nan], dtype=ft)
    x[:special.size * 300] = np.repeat(special, 300)
    rng.shuffle(x)
    return x.view(np.uint64 if kb == 8 else np.uint32)


@pytest.mark.parametrize("kb,vb", COMBOS)
@pytest.mark.parametrize("kind", ["signed", "float"])
def test_signed_and_float_keys(gs, cuda, monkeypatch, kind, kb, vb):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    rng = np.random.default_rng(kb * 10 + vb)
    keys = _signed(kb, 250_000, rng) if kind == "signed" else _floats(kb, 250_000, rng)
    kt = {("signed", 8): I64, ("float", 8): F64, ("signed", 4): I32, ("float", 4): F32}[(kind, kb)]
    _check(gs, cuda, keys, kt, vb)


@pytest.mark.parametrize("const_bytes", [1, 2, 3, 4, 5, 6, 7])
def test_constant_top_bytes_64(gs, cuda, monkeypatch, const_bytes):
    """The top `const_bytes` bytes are one value: the range is split that many times (odd and even depth) before its
    buckets fit a group; 7: the split on byte 0 leaves it sorted."""
    monkeypatch.setenv(LIMIT_ENV, "4096")
    low = 64 - 8 * const_bytes
    keys = _keys(8, "uniform", 200_001, const_bytes)
    keys = (np.uint64(0xA55A3C7E96E1F00D) >> np.uint64(low) << np.uint64(low)) | (keys >> np.uint64(8 * const_bytes))
    _check(gs, cuda, keys, U64, 8 if const_bytes % 2 else 0)


@pytest.mark.parametrize("const_bytes", [1, 2, 3])
def test_constant_top_bytes_32_rowid(gs, cuda, monkeypatch, const_bytes):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    low = 32 - 8 * const_bytes
    keys = _keys(4, "uniform", 200_001, const_bytes)
    keys = (np.uint32(0x5A3C7E00 >> low << low) | (keys >> np.uint32(8 * const_bytes))).astype(np.uint32)
    _check(gs, cuda, keys, U32, 8)


@pytest.mark.parametrize("kb,vb,kt,value", [(8, 0, U64, 0x0123456789ABCDEF), (8, 8, I64, 2**64 - 5),
                                            (8, 4, F64, int(np.float64(-0.0).view(np.uint64))),
                                            (4, 8, F32, int(np.float32(-1.5).view(np.uint32))), (4, 8, I32, 7)])
def test_all_keys_equal(gs, cuda, monkeypatch, kb, vb, kt, value):
    """Oversized down to the last byte: every byte is split, then the range is only moved back to the caller's arrays."""
    monkeypatch.setenv(LIMIT_ENV, "1000")
    keys = np.full(100_003, value, dtype=np.uint64 if kb == 8 else np.uint32)
    _check(gs, cuda, keys, kt, vb)


@pytest.mark.parametrize("n", [100, 3000, 4095, 4096, 4097, 8191, 8193])
@pytest.mark.parametrize("kb,vb", [(8, 8), (4, 8)])
def test_sizes_around_the_limit(gs, cuda, monkeypatch, kb, vb, n):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    _check(gs, cuda, _keys(kb, "uniform", n, n), U64 if kb == 8 else U32, vb)
    _check(gs, cuda, np.full(n, 0x01020304, dtype=np.uint64 if kb == 8 else np.uint32), U64 if kb == 8 else U32, vb)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_sizes(gs, cuda, monkeypatch, n):
    monkeypatch.setenv(LIMIT_ENV, "256")
    _check(gs, cuda, _keys(8, "uniform", n, 3), U64, 8)


@pytest.mark.parametrize("kb,vb", COMBOS)
def test_without_test_limit_matches_the_wide_sort(gs, cuda, monkeypatch, kb, vb):
    from gpu_sort_amd.msb import rdxsrt_unstable_sort_wide
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    n = 300_000
    keys = _keys(kb, "uniform", n, 41)
    kdt, npdt = (torch.int64, np.int64) if kb == 8 else (torch.int32, np.int32)
    kt = U64 if kb == 8 else U32
    got, _ = _sort(gs, cuda, keys, kt, vb)
    dk = torch.from_numpy(keys.view(npdt).copy()).to(cuda)
    dv = torch.arange(n, dtype=torch.int64 if vb == 8 else torch.int32, device=cuda) if vb else None
    rdxsrt_unstable_sort_wide(dk, dv, n, torch.empty_like(dk), torch.empty_like(dv) if vb else None, key_type=kt)
    assert np.array_equal(got, dk.cpu().numpy().view(keys.dtype))


def test_result_in_input_tensors_alternates_are_scratch(gs, cuda, monkeypatch):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    n = 200_000
    keys = _keys(8, "uniform", n, 31)
    dk = torch.from_numpy(keys.view(np.int64).copy()).to(cuda)
    dv = torch.arange(n, dtype=torch.int64, device=cuda)
    ka = torch.full((n,), -7, dtype=torch.int64, device=cuda)
    va = torch.full((n,), -7, dtype=torch.int64, device=cuda)
    seq = gs.rdxsrt_unstable_sort_large_wide(dk, dv, n, ka, va)        # key type from the dtype: GS_KEY_I64
    assert seq.sorted_keys is dk and seq.sorted_values is dv
    assert isinstance(seq, gs.RDXSRT_SortedSequence)
    exp = np.sort(keys.view(np.int64))
    assert np.array_equal(dk.cpu().numpy(), exp)
    assert np.array_equal(keys.view(np.int64)[dv.cpu().numpy()], exp)
    assert not torch.equal(ka, torch.full_like(ka, -7))               # the alternates served as scratch
    assert not torch.equal(va, torch.full_like(va, -7))


def test_list_overflow_is_reported(gs, cuda, monkeypatch):
    """A finish whose device-side list overflowed makes the synchronous call fail (GS_MSB_TEST_MAX_TASKS shrinks the task
    lists of every finish); without the hook the same sort is clean."""
    monkeypatch.setenv(LIMIT_ENV, str(1 << 16))
    n = 1 << 20
    keys = _keys(8, "uniform", n, 2)
    alt = torch.empty(n, dtype=torch.int64, device=cuda)
    monkeypatch.setenv("GS_MSB_TEST_MAX_TASKS", "3")
    dk = torch.from_numpy(keys.view(np.int64).copy()).to(cuda)
    with pytest.raises(gs.GpuSortError) as ei:
        gs.rdxsrt_unstable_sort_large_wide(dk, None, n, alt, None, key_type=U64)
    assert ei.value.code == 999                                       # hipErrorUnknown
    monkeypatch.delenv("GS_MSB_TEST_MAX_TASKS")
    dk = torch.from_numpy(keys.view(np.int64).copy()).to(cuda)
    gs.rdxsrt_unstable_sort_large_wide(dk, None, n, alt, None, key_type=U64)
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), np.sort(keys))


def test_list_overflow_is_reported_for_one_group(gs, cuda, monkeypatch):
    """Arrays of one group take gs_msb_sort_wide; the large entry point still checks the overflow word it left."""
    monkeypatch.delenv(LIMIT_ENV, raising=False)
    n = 1 << 20
    keys = _keys(8, "uniform", n, 4)
    monkeypatch.setenv("GS_MSB_TEST_MAX_TASKS", "3")
    dk = torch.from_numpy(keys.view(np.int64).copy()).to(cuda)
    with pytest.raises(gs.GpuSortError) as ei:
        gs.rdxsrt_unstable_sort_large_wide(dk, None, n, torch.empty_like(dk), None, key_type=U64)
    assert ei.value.code == 999


def test_capture_is_refused_and_enqueues_nothing(gs, cuda, monkeypatch):
    monkeypatch.setenv(LIMIT_ENV, "4096")
    n = 100_000
    keys = _keys(8, "uniform", n, 5)
    dk = torch.from_numpy(keys.view(np.int64).copy()).to(cuda)
    alt = torch.empty_like(dk)
    dm = torch.empty(gs.lib.gs_msb_large_wide_temp_bytes(n, 8, 0), dtype=torch.uint8, device=cuda)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            err = gs.lib.gs_msb_sort_large_wide(dm.data_ptr(), dm.numel(), dk.data_ptr(), None, n, alt.data_ptr(), None, 8, 0, U64,
                                                s.cuda_stream, 1)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert err == 900                                                 # hipErrorStreamCaptureUnsupported
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), keys)     # nothing ran


def _driver(args, env_extra, timeout=300):
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "msb_large")
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env_extra))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "verified=1" in out.stdout and "inversions=0" in out.stdout


@pytest.mark.parametrize("mode", ["u64", "rowid", "host"])
def test_msb_large_driver_modes(mode):
    _driver([str(1 << 24), mode], {LIMIT_ENV: str(1 << 20)})


def _mem_available_gib():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / (1 << 20)
    return 0.0


def test_above_2p32(cuda):
    """2^32 + 2^21 + 7 uniform u64 keys, as many equal u64 keys and as many u32 keys with u64 row ids, checked on the device
    (tools/large_check.py), in a child process."""
    free, _ = torch.cuda.mem_get_info()
    if free < 120 * (1 << 30):
        pytest.skip("needs 120 GiB of free device memory (the rowid case holds about 112 GiB), %.0f GiB free" % (free / (1 << 30)))
    tool = os.path.join(ROOT, "tools", "large_check.py")
    cases = ["u64", "u64_equal", "rowid"]
    out = subprocess.run([sys.executable, tool] + cases, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("-> OK") == len(cases), out.stdout[-3000:]


def test_host_convenience_above_2p32(cuda):
    """rdxsrt_unstable_sort_keys with 2^32 + 2^20 keys: the count no longer truncates to 32 bits (the large sort runs)."""
    avail = _mem_available_gib()
    if avail < 48:
        pytest.skip("needs 48 GiB of available host memory, %.0f GiB available" % avail)
    free, _ = torch.cuda.mem_get_info()
    if free < 64 * (1 << 30):
        pytest.skip("needs 64 GiB of free device memory, %.0f GiB free" % (free / (1 << 30)))
    _driver([str((1 << 32) + (1 << 20)), "host"], {}, timeout=900)
