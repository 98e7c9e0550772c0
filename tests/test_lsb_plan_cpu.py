"""gs_lsb_temp_bytes with the keys-only plan's block (gs_lsb_plan.hip): no GPU needed.

Over the size ladder of tests/test_lsb_large_cpu.py (sizes below 2^32, the limit of gs_lsb_sort_u32): a multiple of 256,
monotone in n, below n * 4 / 50 at 2^30 keys, and below the plan's size window exactly what the four passes alone need
(restated here from the layout: spine, digit totals, prefix16, pass totals, alignment slack).  The window's lower end is a
process-wide switch, so the same checks run once more in a child process that lowers it to its floor."""
import os
import subprocess
import sys

from test_lsb_large_cpu import _sizes

TILE, CHUNK = 8192, 8
PLAN_BLOCK_MAX = 512 << 10          # the plan block is about 0.27 MB
LISTS_MAX = 4 * 65536 * 16          # task lists of arrays too small to hold them in the four passes' region


def _align256(x):
    return (x + 255) & ~255


def four_pass_bytes(n):
    tiles = (n + TILE - 1) // TILE
    grid = max((tiles + CHUNK - 1) // CHUNK, 1)
    return _align256(256 * grid * 4) + 1024 + _align256(tiles * 256 * 2) + _align256(5 * 256 * 4) + 256 + 256


def check_ladder(lib, window_lo):
    prev = 0
    for n in [x for x in _sizes() if x < (1 << 32)]:
        b = lib.gs_lsb_temp_bytes(n, 0)
        assert b % 256 == 0 and b >= prev, (n, b, prev)
        assert lib.gs_lsb_temp_bytes(n, 1) == b
        if n < window_lo:
            assert b == four_pass_bytes(n), (n, b, four_pass_bytes(n))
        else:
            assert four_pass_bytes(n) < b <= max(four_pass_bytes(n), LISTS_MAX) + PLAN_BLOCK_MAX, (n, b)
        prev = b
    assert lib.gs_lsb_temp_bytes(1 << 30, 0) < (1 << 32) // 50


def test_temp_bytes_default_window(gs):
    """The shipped window starts at 2^28 keys or above (DESIGN.md section 9 has the measured crossover)."""
    lo = min(n for n in _sizes() if gs.lib.gs_lsb_temp_bytes(n, 0) != four_pass_bytes(n))
    assert (1 << 27) < lo <= (1 << 30)
    check_ladder(gs.lib, lo)
    assert gs.lib.gs_lsb_temp_bytes(1 << 30, 0) - four_pass_bytes(1 << 30) < PLAN_BLOCK_MAX   # the lists reuse the passes' region


def test_temp_bytes_lowered_window():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gpu_sort_amd as gs\nfrom test_lsb_plan_cpu import check_ladder\ncheck_ladder(gs.lib, 65536)\nprint('ladder ok')\n"
            % (root, os.path.join(root, "tests")))
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    env.pop("GS_LSB_MODE", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ladder ok" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
