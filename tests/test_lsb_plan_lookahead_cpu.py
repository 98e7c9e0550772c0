"""The grid of the keys-only plan's one-pass local-sort launch on the host (gs_lsb_plan.hip): no GPU needed.

gs_lsb_plan_onepass_grid is exported and returns a power of two from 512 to 65536.  GS_LSB_PLAN_ONEPASS_GRID, read once per
process, overrides it with one of these eight values and is ignored with any other: one child process per value.  The
workspace does not depend on it: tests/test_lsb_plan_trim_cpu.py pins gs_lsb_temp_bytes against
tests/golden/lsb_plan_trim_temp_bytes.json, and one size of that table is checked here under the override."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GRIDS = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
N = 1 << 30


def _child(value):
    code = ("import sys; sys.path.insert(0, %r)\nimport gpu_sort_amd as gs\n"
            "print('grid', gs.lib.gs_lsb_plan_onepass_grid(), gs.lib.gs_lsb_temp_bytes(%d, 0), gs.lib.gs_lsb_temp_bytes(%d, 1))\n"
            % (os.path.dirname(HERE), N, N))
    env = dict(os.environ)
    env.pop("GS_LSB_PLAN_ONEPASS_GRID", None)
    if value is not None:
        env["GS_LSB_PLAN_ONEPASS_GRID"] = value
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "grid " in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
    return [int(x) for x in out.stdout.split("grid ")[1].split()]


@pytest.fixture(scope="module")
def default():
    return _child(None)


def test_onepass_grid_exported(gs, default):
    assert gs.lib.gs_lsb_plan_onepass_grid() in GRIDS
    assert default[0] in GRIDS


@pytest.mark.parametrize("value", ["512", "16384", "65536"])
def test_override_taken(default, value):
    got = _child(value)
    assert got[0] == int(value)
    assert got[1:] == default[1:], "the workspace depends on the one-pass grid"


@pytest.mark.parametrize("value", ["0", "256", "1000", "131072", "many", ""])
def test_other_values_ignored(default, value):
    assert _child(value) == default


def test_workspace_is_the_recorded_one(default):
    with open(os.path.join(HERE, "golden", "lsb_plan_trim_temp_bytes.json")) as f:
        want = json.load(f)["default_window"]
    assert default[1:] == want[str(N)]
