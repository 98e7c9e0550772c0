"""gs_lsb_sort_narrow_large on the float key categories at 2^31 + 12345 elements, the smallest size that takes the sliced
64-bit passes (two slices): 8-bit float keys alone (the 64-bit histogram and fill) descending, bfloat16 keys alone (two passes
through narrow_slice_params) ascending.  Checked on the device in chunks of 2^28 elements with torch integer operations: the
image np.where(b & S, b ^ ALL, b ^ S) of the output is monotone, and the 256- / 65536-bin counts equal the input's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 1 << 28
N = (1 << 31) + 12345


def _chunks(n):
    return [(lo, min(lo + CHUNK, n)) for lo in range(0, n, CHUNK)]


def _fill_random(t, card, seed):
    g = torch.Generator(device=t.device)
    g.manual_seed(seed)
    for lo, hi in _chunks(t.numel()):
        t[lo:hi] = torch.randint(0, card, (hi - lo,), device=t.device, generator=g, dtype=torch.int32).to(t.dtype)   # (wraps: every pattern)


def _bits(t, bits):
    """the unsigned bit patterns of a chunk of an int8 / int16 tensor, as int32"""
    return t.to(torch.int32) & ((1 << bits) - 1)


def _image(b, bits):
    S, ALL = 1 << (bits - 1), (1 << bits) - 1
    return torch.where((b & S) != 0, b ^ ALL, b ^ S)


def _counts(t, bits):
    c = torch.zeros(1 << bits, dtype=torch.int64, device=t.device)
    for lo, hi in _chunks(t.numel()):
        c += torch.bincount(_bits(t[lo:hi], bits), minlength=1 << bits)
    return c


def _run(gs, cuda, kt, dtype, bits, desc, seed):
    need = gs.lib.gs_lsb_narrow_large_temp_bytes(N, kt, 0)
    assert need > 0
    free, _ = torch.cuda.mem_get_info()
    want = need + 2 * N * (bits // 8) + (6 << 30)           # the arrays, the workspace and the chunk temporaries of the checks
    if free < want:
        pytest.skip("needs %.0f GiB of free device memory, %.0f GiB free" % (want / (1 << 30), free / (1 << 30)))
    kin = torch.empty(N, dtype=dtype, device=cuda)
    _fill_random(kin, 1 << bits, seed)
    kout = torch.empty_like(kin)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=cuda)
    keep = kin[-(1 << 20):].clone()
    err = gs.lib.gs_lsb_sort_narrow_large(ws.data_ptr(), need, kin.data_ptr(), kout.data_ptr(), None, None, N, kt, 0, 0, bits,
                                          int(desc), None)
    assert err == 0
    torch.cuda.synchronize()
    del ws
    assert torch.equal(keep, kin[-(1 << 20):])
    assert torch.equal(_counts(kin, bits), _counts(kout, bits)), "the counts of the bit patterns differ from the input's"
    for lo, hi in _chunks(N):
        im = _image(_bits(kout[max(lo - 1, 0):hi], bits), bits)
        ok = (im[1:] <= im[:-1]) if desc else (im[1:] >= im[:-1])
        assert bool(ok.all()), "the image is not monotone in the chunk at %d" % lo


def test_f8_keys_descending_2p31_plus_12345(gs, cuda):
    _run(gs, cuda, gs.GS_KEY_F8, torch.int8, 8, True, 1)


def test_bf16_keys_ascending_2p31_plus_12345(gs, cuda):
    _run(gs, cuda, gs.GS_KEY_BF16, torch.int16, 16, False, 2)
