"""The keys-only plan of gs_lsb_sort_u32 (gs_lsb_plan.hip): full-width keys without values are sorted
by two scatters and one local sort per group of equal top 16 bits when every group fits the largest local sort (PLANNED),
and by the four passes otherwise (CLASSIC), decided on the device.

GS_LSB_KEYS_PLAN and GS_LSB_PLAN_MIN_ITEMS are read once per process, so the cases run in two child processes
(tests/lsb_plan_child.py), one with the plan reachable from 65536 keys and one with GS_LSB_KEYS_PLAN=classic; both run once
per session.  For every case: the result equals numpy's, byte for byte, in both modes; the two modes agree on the result
bytes and on the selector; the guard bands around the key buffers and the workspace are intact; and what
gs_lsb_plan_status reports equals the plan rule restated in numpy (route, largest group, non-empty groups, tasks per class)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANNED, CLASSIC = 1, 2

# case -> the route the plan must take (the child computes the same from the keys; this table pins the intent of each case)
ROUTES = {
    "cap_edge_planned": PLANNED, "cap_edge_classic": CLASSIC,
    "size_131072": PLANNED, "size_131073": PLANNED, "size_139263": PLANNED, "size_143363": PLANNED,
    "tiny_groups": PLANNED,
    "type_u32_asc": PLANNED, "type_u32_desc": PLANNED, "type_i32_asc": PLANNED, "type_i32_desc": PLANNED,
    "type_f32_asc": PLANNED, "type_f32_desc": PLANNED,
    "all_equal": CLASSIC, "sorted": PLANNED, "reversed": PLANNED, "low16_constant": PLANNED, "low16_few_values": PLANNED,
    "top16_constant": CLASSIC,
    "ws_offset_4": PLANNED, "ws_offset_255_data_offset": PLANNED,
    "reuse_0": PLANNED, "reuse_1": CLASSIC, "reuse_2": PLANNED, "reuse_3": CLASSIC,
    "graph_0": PLANNED, "graph_1": CLASSIC, "graph_2": CLASSIC, "graph_3": PLANNED,
}


def _child(tmp, tag, extra_env):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536", **extra_env)
    env.pop("GS_LSB_MODE", None)
    if "GS_LSB_KEYS_PLAN" not in extra_env:
        env.pop("GS_LSB_KEYS_PLAN", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_child.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "plan child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan")
    return _child(tmp, "plan", {}), _child(tmp, "classic", {"GS_LSB_KEYS_PLAN": "classic"})


def test_every_case_ran(runs):
    plan, classic = runs
    assert set(plan) == set(ROUTES) and set(classic) == set(ROUTES)


@pytest.mark.parametrize("case", sorted(ROUTES))
def test_plan_case(runs, case):
    plan, classic = runs
    p, c = plan[case], classic[case]
    assert p["guards"] and c["guards"], "a guard band changed"
    assert c["ok_numpy"], "the four passes differ from numpy"
    assert p["ok_numpy"], "the planned sort differs from numpy (route %d)" % p["status"][0]
    assert p["sha"] == c["sha"], "the two modes differ"
    assert p["sel"] == c["sel"], "the selector depends on the route"
    if p["rule"][1] < 65536:
        assert p["status"] == p["rule"], "device plan %s, plan rule %s" % (p["status"], p["rule"])
    else:
        # a group of 65536 keys or more can wrap a 16-bit counter of the look: the sort then only knows that the group is
        # too large (CLASSIC), and the sizes it reports are those of the wrapped counters
        assert p["status"][0] == CLASSIC and p["status"][3:7] == [0, 0, 0, 0]
    assert p["status"][0] == ROUTES[case]
    assert c["status"] == [0] * 8, "GS_LSB_KEYS_PLAN=classic must not look"


def test_cap_edge_classes(runs):
    """The cap-edge case holds groups of 1, 2, 63, 64, 2048 | 2049, 4608 | 4609, 5000, 9216 | 9217, 12000, 17407, 17408 x 2
    keys: 5, 2, 3 and 5 tasks in the classes of 2048, 4608, 9216 and 17408 keys, 15 non-empty groups."""
    st = runs[0]["cap_edge_planned"]["status"]
    assert st[:7] == [PLANNED, 17408, 15, 5, 2, 3, 5]
    st = runs[0]["cap_edge_classic"]["status"]
    assert st[:7] == [CLASSIC, 17409, 15, 0, 0, 0, 0]
