"""The second scatter of the keys-only plan in cursor mode (gs_lsb_plan.hip): when the plan is PLANNED the
scatter on bits 24-31 has no upsweep -- a tile claims its places in every group with one returning add on the group's cursor,
and the tiles that hold more than one value of bits 16-23, and the partial last tile, are placed key by key by a follow-up
kernel.  The finish sorts every group, so the result is byte for byte what the stable scatter gives.

GS_LSB_KEYS_PLAN, GS_LSB_PLAN_SCATTER2 and GS_LSB_PLAN_MIN_ITEMS are read once per process, so the cases run in three child
processes (tests/lsb_plan_cursor_child.py), each once per session: the four passes (GS_LSB_KEYS_PLAN=classic), the plan with
GS_LSB_PLAN_SCATTER2=stable and the plan with GS_LSB_PLAN_SCATTER2=cursor, all with the plan reachable from 65536 keys.  For
every case and mode: the result equals numpy's sort of the order-mapped keys; the three modes agree on the result bytes and
on the selector; the two plan modes agree on gs_lsb_plan_status, which equals the plan rule restated in numpy; the guard bands
around both key buffers and the workspace are intact.  In cursor mode gs_lsb_plan_cursor_status reports cursor mode exactly
when the route is PLANNED, and then as many follow-up tiles as numpy counts; in the other modes it reports zeros."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANNED, CLASSIC = 1, 2
N_CAMPAIGN = 40

# case -> the route the plan must take (this table pins the intent of each case; the child restates the rule from the keys)
ROUTES = {
    "uniform_65536": PLANNED, "uniform_65537": PLANNED, "uniform_139263": PLANNED, "uniform_1052675": PLANNED,
    "regions_aligned": PLANNED, "region0_8191": PLANNED, "region0_8193": PLANNED, "many_boundaries": PLANNED,
    "empty_regions": PLANNED, "hot_row": PLANNED, "one_d2": PLANNED,
    "cap_edge_planned": PLANNED, "cap_edge_classic": CLASSIC,
    "type_u32_asc": PLANNED, "type_u32_desc": PLANNED, "type_i32_asc": PLANNED, "type_i32_desc": PLANNED,
    "type_f32_asc": PLANNED, "type_f32_desc": PLANNED,
    "sorted": PLANNED, "reversed": PLANNED,
    "reuse_0": CLASSIC, "reuse_1": PLANNED, "reuse_2": PLANNED,
    "graph_0": PLANNED, "graph_1": PLANNED,
}
ROUTES.update({"campaign_%02d" % i: CLASSIC if i % 8 == 7 else PLANNED for i in range(N_CAMPAIGN)})

# follow-up tiles that the layout of a case fixes by construction: the straddling full tiles plus the partial tile
IRREGULAR = {"uniform_65536": 8, "uniform_65537": 8 + 1, "regions_aligned": 0, "region0_8191": 255 + 1, "region0_8193": 255 + 1,
             "many_boundaries": 1 + 1}


def _child(tmp, tag, extra_env):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    for k in ("GS_LSB_MODE", "GS_LSB_KEYS_PLAN", "GS_LSB_PLAN_SCATTER2"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_cursor_child.py"), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "cursor child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_cursor")
    return (_child(tmp, "classic", {"GS_LSB_KEYS_PLAN": "classic"}), _child(tmp, "stable", {"GS_LSB_PLAN_SCATTER2": "stable"}),
            _child(tmp, "cursor", {"GS_LSB_PLAN_SCATTER2": "cursor"}))


def test_every_case_ran(runs):
    for r in runs:
        assert set(r) == set(ROUTES)


@pytest.mark.parametrize("case", sorted(ROUTES))
def test_cursor_case(runs, case):
    c, s, k = (r[case] for r in runs)
    for tag, r in (("classic", c), ("stable", s), ("cursor", k)):
        assert r["guards"], "a guard band changed (%s)" % tag
        assert r["ok_numpy"], "the sort differs from numpy (%s, route %d)" % (tag, r["status"][0])
    assert c["sha"] == s["sha"] == k["sha"], "the modes differ"
    assert c["sel"] == s["sel"] == k["sel"], "the selector depends on the mode"
    assert s["status"] == k["status"], "the plan depends on the scatter"
    if k["rule"][1] < 65536:
        assert k["status"] == k["rule"], "device plan %s, plan rule %s" % (k["status"], k["rule"])
    else:
        # a group of 65536 keys or more can wrap a 16-bit counter of the look: the sort then only knows that the group is too
        # large (CLASSIC), and the sizes it reports are those of the wrapped counters
        assert k["status"][0] == CLASSIC and k["status"][3:7] == [0, 0, 0, 0]
    assert k["status"][0] == ROUTES[case]
    assert c["status"] == [0] * 8 and c["cursor"] == [0] * 4, "GS_LSB_KEYS_PLAN=classic must not look"
    assert s["cursor"] == [0] * 4, "GS_LSB_PLAN_SCATTER2=stable ran in cursor mode"
    if k["status"][0] == PLANNED:
        tail = 1 if k["n"] % 8192 else 0
        assert k["cursor"] == [1, k["irregular"], k["irregular"] - tail, 0], "follow-up tiles: device %s, numpy %d" % (k["cursor"], k["irregular"])
    else:
        assert k["cursor"] == [0] * 4, "a CLASSIC sort reports cursor mode"
    if case in IRREGULAR:
        assert k["irregular"] == IRREGULAR[case]
