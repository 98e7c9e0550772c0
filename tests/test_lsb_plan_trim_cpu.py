"""What trimming the small launches of the keys-only plan (gs_lsb_plan.hip) must leave alone on the host: no GPU needed.

gs_lsb_plan_finish_cap is exported and returns one of the three grids it may be (512, 1024, 2048); gs_lsb_temp_bytes is what
it was before the change, for every size that tests/test_lsb_plan_cpu.py walks, with the default size window and -- in a
child process, the window being a process-wide switch -- with the window lowered to its floor.  The sizes of the build before
are recorded in tests/golden/lsb_plan_trim_temp_bytes.json."""
import json
import os
import subprocess
import sys

from test_lsb_large_cpu import _sizes

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lsb_plan_trim_temp_bytes.json")


def check_sizes(lib, table):
    with open(GOLDEN) as f:
        want = json.load(f)[table]
    ns = [n for n in _sizes() if n < (1 << 32)]
    assert sorted(int(k) for k in want) == sorted(ns), "the size ladder changed: record the sizes again"
    for n in ns:
        assert [lib.gs_lsb_temp_bytes(n, 0), lib.gs_lsb_temp_bytes(n, 1)] == want[str(n)], n


def test_finish_cap_exported(gs):
    assert gs.lib.gs_lsb_plan_finish_cap() in (512, 1024, 2048)


def test_temp_bytes_unchanged_default_window(gs):
    check_sizes(gs.lib, "default_window")


def test_temp_bytes_unchanged_lowered_window():
    root = os.path.dirname(HERE)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import gpu_sort_amd as gs\nfrom test_lsb_plan_trim_cpu import check_sizes\ncheck_sizes(gs.lib, 'window_from_65536')\n"
            "print('sizes ok')\n" % (root, HERE))
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    env.pop("GS_LSB_MODE", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "sizes ok" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
