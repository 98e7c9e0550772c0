"""The fused look's host side (gs_lsb_plan.hip): no GPU needed.

The test hooks exist in the built library and refuse what gs_lsb_plan_status refuses (null pointers, sizes outside the
plan's window); the plan block still fits the words it had, so gs_lsb_temp_bytes gives what the build before the fused look
gave (the values below were taken from that build)."""
import ctypes as C

TEMP_BYTES = {(1 << 28) - 1: 20978176, 1 << 28: 21247232, 1 << 30: 84161792, 1089208320: 85370112}
INVALID_VALUE = 1       # hipErrorInvalidValue
N_MAX = 1089208320      # the upper end of the plan's window


def test_hooks_are_exported(gs):
    for name in ("gs_lsb_plan_look_only", "gs_lsb_plan_layout", "gs_lsb_plan_status"):
        assert hasattr(gs.lib, name), name


def test_temp_bytes_unchanged(gs):
    for n, b in TEMP_BYTES.items():
        assert gs.lib.gs_lsb_temp_bytes(n, 0) == b, n
        assert gs.lib.gs_lsb_temp_bytes(n, 1) == b, n


def test_layout_inside_the_window(gs):
    """spine first, prefix16 behind the spine and the digit totals, the plan block behind the four passes' workspace."""
    out = (C.c_uint64 * 4)()
    for n in (1 << 28, 1 << 30, N_MAX):
        assert gs.lib.gs_lsb_plan_layout(n, out) == 0
        spine, prefix16, plan, grid = (int(x) for x in out)
        tiles = (n + 8191) // 8192
        assert grid == (tiles + 7) // 8
        assert spine == 0 and prefix16 == 256 * grid * 4 + 1024 and prefix16 + tiles * 512 <= plan
        assert plan + 64 <= gs.lib.gs_lsb_temp_bytes(n, 0) - 256


def test_hooks_refuse_sizes_outside_the_window_and_null_pointers(gs):
    out = (C.c_uint64 * 4)()
    fake = C.c_void_p(1 << 20)     # never dereferenced: every call below is refused on the host
    for n in (0, 65536, (1 << 28) - 1, N_MAX + 1, 1 << 32, (1 << 32) + 5):
        assert gs.lib.gs_lsb_plan_layout(n, out) == INVALID_VALUE, n
        assert gs.lib.gs_lsb_plan_look_only(fake, fake, fake, n, 0, 0, None) == INVALID_VALUE, n
    n = 1 << 28
    assert gs.lib.gs_lsb_plan_layout(n, None) == INVALID_VALUE
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert gs.lib.gs_lsb_plan_look_only(*args, n, 0, 0, None) == INVALID_VALUE
