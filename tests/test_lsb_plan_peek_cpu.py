"""The host's look at the keys-only plan's decision (gs_lsb_plan.hip), host side: no GPU needed.

gs_lsb_plan_peek_status exists, refuses a null pointer, reports zeros on a thread that has not run a planned sort, and keeps
its record per thread; the workspace has the size it had (the mailbox is pinned host memory of the library's own)."""
import ctypes as C
import threading

INVALID_VALUE = 1       # hipErrorInvalidValue
TEMP_BYTES = {1 << 28: 21247232, 1 << 30: 84161792, 1089208320: 85370112}      # as tests/test_lsb_plan_fused_cpu.py


def test_peek_status_refuses_null_and_fills_four_words(gs):
    assert gs.lib.gs_lsb_plan_peek_status(None) == INVALID_VALUE
    out = (C.c_uint32 * 5)(7, 7, 7, 7, 7)
    assert gs.lib.gs_lsb_plan_peek_status(out) == 0
    assert out[0] in (0, 1) and out[1] in (0, 1, 2) and out[2] in (0, 2, 4) and out[3] < 16 and out[4] == 7


def test_peek_status_on_a_fresh_thread(gs):
    got = []

    def worker():
        out = (C.c_uint32 * 4)(9, 9, 9, 9)
        got.append((gs.lib.gs_lsb_plan_peek_status(out), list(out)))

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert got == [(0, [0, 0, 0, 0])]


def test_workspace_size_unchanged(gs):
    for n, b in TEMP_BYTES.items():
        assert gs.lib.gs_lsb_temp_bytes(n, 0) == b, n
