"""bench.py must start its own ranks when it is called plainly with --gpus N > 1: the driver runs
`python bench.py --gpus N ...` the way it runs `--gpus 1`.  Exercised here without a GPU through --dry-run-launch
(gloo, world size 2): spawn, rendezvous on 127.0.0.1, one collective, ONE JSON line from rank 0, exit code passed on."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=600)


def test_plain_call_with_two_gpus_launches_its_ranks():
    out = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run-launch"])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["dry_run"] is True and rec["rank_sum"] == 3.0 and rec["steps"] == 3


def test_world_size_mismatch_is_an_error():
    out = _run(["--gpus", "2", "--dry-run-launch"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode == 2 and "WORLD_SIZE" in out.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_positions_are_fixed_and_in_range():
    import numpy as np
    b = _bench_module()
    assert np.array_equal(b.dump_sample_index(1000), np.arange(1000))
    n = 1 << 30
    idx = b.dump_sample_index(n)
    assert idx.size == b.DUMP_MAX and idx.size * 8 <= 32 << 20
    assert idx[0] >= 0 and idx[-1] < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, b.dump_sample_index(n))


def _json_line(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_every_step_and_dumps_the_last_output(tmp_path, oracle):
    """More steps than the input ring (inputs refilled between chunks), headline fields only, and the dumped sample of the
    last timed step's output equals the CPU oracle's sort of that step's input (seed = step index)."""
    import numpy as np
    b = _bench_module()
    log2n, steps, warmup = 22, b.INPUT_RING + 3, 1
    rec = _json_line(_run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--log2n", str(log2n),
                           "--dump-outputs", str(tmp_path)]))
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["value"] > 0 and rec["unit"] == "Gkeys/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u32" and rec["full"] is False
    assert rec["also"] is None and rec["cpu_baseline"] is None and rec["roofline"] is None
    got = np.load(tmp_path / "sorted_keys.npy")
    assert got.dtype == np.float64
    n = 1 << log2n
    want = np.sort(oracle.gen_uniform(n, seed=steps + warmup - 1))[b.dump_sample_index(n)]
    assert np.array_equal(got, want.astype(np.float64))


@pytest.mark.gpu
def test_full_run_reports_the_extra_figures():
    rec = _json_line(_run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--log2n", "20", "--full", "--also-steps", "2"]))
    assert rec["full"] is True and rec["verified"] is True
    assert rec["kernels_ms_total"] and rec["whole_sort"] and rec["box"] and rec["cpu_baseline"]["value"] > 0
    assert rec["also"] and all(v["verified"] for v in rec["also"].values())
