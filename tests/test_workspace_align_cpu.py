"""CPU test of the workspace alignment contract (include/gpusort.h): d_temp may have any alignment.  Every entry point carves
its workspace from d_temp rounded up to 256 bytes, and every size query includes the slack that rounding takes.
gs_lsb_workspace_layout is pure pointer arithmetic, so fake bases show the carve without a device."""
import ctypes as C

import pytest


@pytest.mark.parametrize("n", [1, 8191, 8193, 100003, (1 << 21) + 77, (1 << 30) + 5])
def test_lsb_layout_is_aligned_and_inside_the_query_at_any_base(gs, n):
    lib = gs.lib
    need = lib.gs_lsb_temp_bytes(n, 0)
    assert need % 256 == 0
    g, t, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib.gs_lsb_geometry(n, 0, C.byref(g), C.byref(t), C.byref(c))
    tiles = (n + t.value - 1) // t.value
    sizes = {"spine": 256 * g.value * 4, "totals": 256 * 4, "prefix16": tiles * 256 * 2}
    for k in range(256):
        base = 0x100000 + k
        sp, tot, pf = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert lib.gs_lsb_workspace_layout(base, n, C.byref(sp), C.byref(tot), C.byref(pf)) == 0
        for name, p in (("spine", sp), ("totals", tot), ("prefix16", pf)):
            assert p.value % 256 == 0, (k, name, hex(p.value))
            assert base <= p.value and p.value + sizes[name] <= base + need, (k, name, hex(p.value), need)
        assert sp.value + sizes["spine"] <= tot.value and tot.value + sizes["totals"] <= pf.value


def test_every_size_query_is_a_multiple_of_256_with_room_for_the_rounding(gs):
    """Each query is its parent-commit layout plus 256 bytes: the carve from a base rounded up by up to 255 bytes fits."""
    lib = gs.lib
    for n in (1, 4097, 8193, 100003, 1 << 21):
        qs = [lib.gs_lsb_temp_bytes(n, 1), lib.gs_lsb_copy_temp_bytes(n, 1), lib.gs_lsb_wide_temp_bytes(n, 8, 8),
              lib.gs_lsb_any_temp_bytes(n, 6, 16), lib.gs_lsb_any_temp_bytes(n, 3, 4), lib.gs_msb_temp_bytes(n, 1),
              lib.gs_msb_wide_temp_bytes(n, 8, 8), lib.gs_msb_large_temp_bytes(n, 1), lib.gs_msb_large_wide_temp_bytes(n, 8, 8),
              lib.gs_segmented_temp_bytes(n, 1, 100), lib.gs_segmented_wide_temp_bytes(n, 8, 8, 100),
              lib.gs_msb_finish_temp_bytes(n, 1, 1)]
        assert all(q % 256 == 0 and q >= 512 for q in qs), (n, qs)
        # the plain MSB sort of a small large-sort call runs in the large sort's workspace
        assert lib.gs_msb_large_temp_bytes(n, 1) >= lib.gs_msb_temp_bytes(n, 1)
        assert lib.gs_msb_large_wide_temp_bytes(n, 8, 8) >= lib.gs_msb_wide_temp_bytes(n, 8, 8)

