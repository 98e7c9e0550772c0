"""drivers/lsb_halfs (built by build()): __half keys and (__hip_bfloat16, int) pairs descending through gpusort.hpp's
DeviceRadixSort, checked on the host by the driver itself.  Nothing is built here."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lsb_halfs_driver_passes():
    exe = os.path.join(ROOT, "gpu-sort_amd", "drivers", "lsb_halfs")
    assert os.path.exists(exe), "%s is missing: build() builds the drivers" % exe
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "PASS" and sum("CORRECT" in l for l in lines) == 2, out.stdout
