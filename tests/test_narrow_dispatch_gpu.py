"""The Python front end routes 8- and 16-bit keys to gs_lsb_sort_narrow: the DoubleBuffer size query returns that function's
bytes, a workspace of exactly that size is accepted, and the DoubleBuffer behaviour is the one gs_lsb_sort_any gave (result
in the alternate buffer, selector flipped once, current buffer untouched)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tdt,ktname,vdt", [(torch.uint8, "GS_KEY_U8", None), (torch.int8, "GS_KEY_I8", torch.int32),
                                            (torch.bool, "GS_KEY_U8", torch.uint8), (torch.int16, "GS_KEY_I16", None),
                                            (torch.int16, "GS_KEY_I16", torch.int64), (torch.uint8, "GS_KEY_U8", "rows16")])
def test_shim_routes_narrow_keys(gs, cuda, tdt, ktname, vdt):
    n = 70001
    kt = getattr(gs, ktname)
    g = torch.Generator().manual_seed(5)
    if tdt == torch.bool:
        keys = torch.randint(0, 2, (n,), generator=g).to(torch.bool)
    elif tdt == torch.int16:
        keys = torch.randint(-2**15, 2**15, (n,), generator=g).to(torch.int16)
    else:
        keys = torch.randint(0, 256, (n,), generator=g).to(torch.uint8).view(tdt)
    if vdt is None:
        vals, vb = None, 0
    elif vdt == "rows16":
        vals, vb = torch.randint(-2**31, 2**31 - 1, (n, 4), generator=g).to(torch.int32), 16
    else:
        vals = torch.arange(n).to(vdt)
        vb = vals.element_size()
    dk = gs.DoubleBuffer(keys.to(cuda), torch.zeros(n, dtype=tdt, device=cuda))
    dv = gs.DoubleBuffer(vals.to(cuda), torch.zeros_like(vals, device=cuda)) if vals is not None else None
    fn = gs.DeviceRadixSort.SortPairs if dv is not None else gs.DeviceRadixSort.SortKeys
    args = (dk, dv, n) if dv is not None else (dk, n)
    nb = fn(None, 0, *args)
    assert nb == gs.lib.gs_lsb_narrow_temp_bytes(n, kt, vb) and nb > 0
    assert nb != gs.lib.gs_lsb_any_temp_bytes(n, kt, vb)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    assert fn(temp, nb, *args) == nb
    torch.cuda.synchronize()
    assert dk.selector == 1 and (dv is None or dv.selector == 1)
    assert torch.equal(dk.Alternate().cpu(), keys)                      # the buffer that was current is untouched
    order = torch.sort(keys.to(torch.int32), stable=True)[1]
    assert torch.equal(dk.Current().cpu(), keys[order])
    if dv is not None:
        assert torch.equal(dv.Alternate().cpu(), vals)
        assert torch.equal(dv.Current().cpu(), vals[order])
    with pytest.raises(gs.GpuSortError):                                # one byte less is refused
        fn(temp[:nb - 1], nb - 1, *args)
