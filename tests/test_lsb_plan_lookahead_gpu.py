"""The keys-only plan at the edges of what a look workgroup and a one-pass local-sort workgroup walk (gs_lsb_plan.hip,
gs_msb.hip): the look takes units of 131072 keys, slot, slot + grid, ..., and the one-pass local sort
runs on the grid that gs_lsb_plan_onepass_grid() reports -- a workgroup per task as built, fewer under
GS_LSB_PLAN_ONEPASS_GRID, which then stride over the task list and pass over the records the one-pass sort cannot take.  No
grid and no walk may change a byte of any result.  (Written with a look that kept loads in flight across its unit epilogue and
a one-pass sort that requested its records two tasks ahead; neither was kept, the cases are those that would catch them.)

GS_LSB_KEYS_PLAN, GS_LSB_PLAN_MIN_ITEMS and GS_LSB_PLAN_ONEPASS_GRID are read once per process, so the cases run in child
processes (tests/lsb_plan_lookahead_child.py), each once per session, all with the plan reachable from 65536 keys.

Look: gs_lsb_plan_look_only against the numpy reference of tests/lsb_plan_fused_child.py and gs_lsb_plan_status against the plan
rule, at sizes where a look workgroup has one unit of 131072 keys, where some have two and others one, where all have three,
where the next unit exists but some waves' tiles in it are ragged or past the end, where the last unit is one chunk and the last
tile holds 1, 63, 64 or 8191 keys, and at the smallest size; uniform, constant, half all-ones and wrapped-counter keys; u32, i32
and f32 keys in both directions.  On every case the whole sort equals the four passes' (GS_LSB_KEYS_PLAN=classic) byte for byte,
with intact guard bands around both buffers and the workspace.

Finish: with the one-pass grid at 512, lists of grid - 1, grid, grid + 1 and 2 grid + 1 class-3 groups (a workgroup takes no,
one, two or three tasks), in which every second group, or the last alone, cannot be sorted in one pass (one value 300 times:
a byte counter overflows; 20 times: a packed count does; a third of the group: the sample look flags the record beforehand and
the one-pass sort passes it over), and a list with all four classes: checked on the device and against the four passes.

MSB: rdxsrt_unstable_sort shares the one-pass kernel; uniform and Zipf keys, keys and pairs, at a size with more class-3 tasks
than its grid of 16384."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from lsb_plan_lookahead_child import HEAVY, KEY_SIZES, finish_cases, look_cases  # noqa: E402

PLANNED, CLASSIC = 1, 2
FINISH_GRID = 512
LOOK = sorted(look_cases())
FINISH = sorted(finish_cases(FINISH_GRID))


def _child(tmp, part, tag, extra_env):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    for k in ("GS_LSB_MODE", "GS_LSB_KEYS_PLAN", "GS_LSB_PLAN_SCATTER2", "GS_LSB_PLAN_PEEK", "GS_LSB_PLAN_FINISH_CAP", "GS_LSB_PLAN_ONEPASS_GRID",
              "GS_MSB_DEDUPE"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_lookahead_child.py"), part, out], env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0 and "lookahead child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def look_runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_lookahead_look")
    return _child(tmp, "look", "plan", {}), _child(tmp, "look", "classic", {"GS_LSB_KEYS_PLAN": "classic"})


@pytest.fixture(scope="module")
def finish_runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_lookahead_finish")
    grid = {"GS_LSB_PLAN_ONEPASS_GRID": str(FINISH_GRID)}
    return _child(tmp, "finish", "plan", grid), _child(tmp, "finish", "classic", dict(grid, GS_LSB_KEYS_PLAN="classic"))


def test_every_case_ran(look_runs, finish_runs):
    for r in look_runs:
        assert sorted(r) == LOOK
    for r in finish_runs:
        assert sorted(k for k in r if k != "grid") == FINISH
        assert r["grid"] == FINISH_GRID, "GS_LSB_PLAN_ONEPASS_GRID=%d was not taken" % FINISH_GRID


@pytest.mark.parametrize("case", LOOK)
def test_look(look_runs, case):
    plan, classic = (r[case] for r in look_runs)
    assert plan["look_guards"] and plan["guards"] and classic["guards"], "a guard band changed"
    assert plan["grid"] == plan["grid_expected"]
    assert plan["spine_bad"] == 0, "%d spine words differ from numpy" % plan["spine_bad"]
    assert plan["prefix_bad"] == 0, "%d prefix16 words differ from numpy" % plan["prefix_bad"]
    rule = plan["rule"]
    if rule[0] == CLASSIC:
        # nearly every CLASSIC case here has a group of 65536 keys or more inside one look workgroup: a 16-bit counter wrapped,
        # and the other words of the head are then those of the wrapped counters
        assert plan["head"][0] == CLASSIC and plan["status"][0] == CLASSIC
        assert plan["status"][3:7] == [0, 0, 0, 0] and plan["status"][7] <= plan["n"]
    else:
        assert plan["head"][:8] == rule, "the look decided %s, the plan rule says %s" % (plan["head"][:8], rule)
        assert plan["status"] == rule, "device plan %s, plan rule %s" % (plan["status"], rule)
    assert plan["head"][0] == plan["status"][0]
    if plan["head"][0] == PLANNED:
        assert plan["head"][8:12] == [16, 24, 0xFFFFFFFF, 0xFFFFFFFF] and plan["head"][12:16] == [1, 0, 1, 1]
    else:
        assert plan["head"][8:12] == [0, 8, 16, 24] and plan["head"][12:16] == [0, 0, 0, 0]
    assert classic["status"] == [0] * 8, "GS_LSB_KEYS_PLAN=classic must not look"
    assert plan["sha"] == classic["sha"], "the plan's result differs from the four passes'"
    assert plan["sel"] == classic["sel"], "the selector depends on the route"
    if plan["inversions"] is not None:
        assert plan["inversions"] == 0 and classic["inversions"] == 0


def test_look_cases_take_both_routes(look_runs):
    routes = {case: look_runs[0][case]["status"][0] for case in LOOK}
    for n in KEY_SIZES:
        assert routes["uniform_%d" % n] == PLANNED
        assert routes["constant_%d" % n] == CLASSIC and routes["half_ones_%d" % n] == CLASSIC and routes["wrapped_%d" % n] == CLASSIC


@pytest.mark.parametrize("case", FINISH)
def test_finish(finish_runs, case):
    plan, classic = (r[case] for r in finish_runs)
    assert plan["guards"] and classic["guards"], "a guard band changed"
    for tag, r in (("plan", plan), ("classic", classic)):
        assert r["inversions"] == 0 and r["multiset"], "%s: %d inversions, multiset kept: %s" % (tag, r["inversions"], r["multiset"])
    assert plan["sha"] == classic["sha"], "the plan's result differs from the four passes'"
    assert plan["sel"] == classic["sel"]
    st, classes = plan["status"], plan["classes"]
    assert st[0] == PLANNED and st[3:7] == classes and st[2] == sum(classes) and st[7] == plan["n"]
    assert plan["peek"] == [1, PLANNED, 2, sum(1 << c for c in range(4) if classes[c])]
    assert classic["status"] == [0] * 8
    groups3 = classes[3]
    if case == "four_classes":
        assert all(classes) and groups3 == FINISH_GRID + 3 > FINISH_GRID
        assert plan["heavy"] == (groups3 + 1) // 2
    else:
        kind, groups = case.rsplit("_", 1)
        assert kind in HEAVY and groups3 == int(groups) and classes[:3] == [0, 0, 0]
        assert plan["heavy"] == ((groups3 + 1) // 2 if HEAVY[kind][0] == 2 else 1)


def test_built_in_grid_above_the_local_sorts_limit(gs, cuda):
    """More class-3 groups than the 16384 workgroups the local sorts give themselves: as built, the plan's one-pass launch has
    a workgroup for each (this process's switches are the defaults: the plan takes 2^28 keys and more)."""
    import ctypes as C

    import numpy as np
    import torch
    from lsb_plan_lookahead_child import finish_keys
    groups = 20500
    assert gs.lib.gs_lsb_plan_onepass_grid() >= groups > 16384
    sizes = np.random.default_rng(5).integers(13000, 13401, size=groups)
    keys, _ = finish_keys(torch, cuda, sizes, 31, "last_20")
    n = int(keys.numel())
    assert n >= 1 << 28
    _, want_sum, want_xor = gs.check_sorted(keys)
    alt = torch.empty_like(keys)
    nb = gs.lib.gs_lsb_temp_bytes(n, 0)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    dk = gs.DoubleBuffer(keys, alt)
    gs.DeviceRadixSort.SortKeys(temp, nb, dk, n, key_type=gs.GS_KEY_U32)
    st = (C.c_uint32 * 8)()
    assert gs.lib.gs_lsb_plan_status(temp.data_ptr(), n, st, None) == 0
    assert list(st)[0] == PLANNED and list(st)[3:7] == [0, 0, 0, groups] and st[7] == n
    inv, got_sum, got_xor = gs.check_sorted(dk.Current())
    assert inv == 0 and got_sum == want_sum and got_xor == want_xor


@pytest.mark.parametrize("dist", ["uniform", "zipf"])
@pytest.mark.parametrize("pairs", [False, True], ids=["keys", "pairs"])
def test_msb_more_tasks_than_the_grid(gs, cuda, dist, pairs):
    import torch
    n = (1 << 28) + 12345
    src = (gs.generate_zipf_keys if dist == "zipf" else gs.generate_uniform_keys)(n, device=cuda)
    _, want_sum, want_xor = gs.check_sorted(src)
    keys = src.clone()
    vals = gs.generate_enumerated_values(n, device=cuda) if pairs else None
    seq = gs.rdxsrt_unstable_sort(keys, vals, n, torch.empty_like(keys), torch.empty_like(keys) if pairs else None)
    inv, got_sum, got_xor = gs.check_sorted(seq.sorted_keys)
    assert inv == 0 and got_sum == want_sum and got_xor == want_xor
    if pairs:
        bad, vsum = gs.check_pairs_enumerated(src, seq.sorted_keys, seq.sorted_values, n)
        assert bad == 0 and vsum == n * (n - 1) // 2
