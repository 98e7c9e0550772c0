"""The small launches of the keys-only plan (gs_lsb_plan.hip): the follow-up kernel of the cursor scatter
with all its memory operations in flight, the cursor set-up and the cursor scatter of a host that has seen the route, the
decision written to the host's mailbox by the decide kernel, and the finish's two leftover local-sort launches on a capped
grid, reading 64 task records at a time.  None of them may change a byte of the result.

GS_LSB_PLAN_PEEK, GS_LSB_KEYS_PLAN and GS_LSB_PLAN_MIN_ITEMS are read once per process, so the cases run in three child
processes (tests/lsb_plan_trim_child.py), each once per session, all with the plan reachable from 65536 keys: the default
(the host looks: the new set-up kernel and scatter), GS_LSB_PLAN_PEEK=0 (the fixed sequence with the slot kernels and their
set-up) and GS_LSB_KEYS_PLAN=classic (the four passes).  For every case the three agree on the result bytes and the
selector, the first two also on gs_lsb_plan_status and gs_lsb_plan_cursor_status, and the guard bands around both key
buffers and the workspace are intact.  The small cases are compared with numpy's sort and the plan rule restated in numpy,
and gs_lsb_plan_cursor_status must report the follow-up tiles that numpy counts from the layout; the capped cases (more
class-3 groups than the leftover launches have workgroups) are checked on the device."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANNED, CLASSIC = 1, 2
TAILS = (1, 63, 64, 65, 4097, 8191)

SMALL = {"straddle_hot_then_one": PLANNED, "straddle_one_then_hot": PLANNED, "three_groups_in_a_wave": PLANNED,
         "every_lane_its_group": PLANNED, "tail_alone_in_its_d1": PLANNED,
         "reuse_0": PLANNED, "reuse_1": CLASSIC, "reuse_2": CLASSIC, "reuse_3": PLANNED, "graph_0": PLANNED, "graph_1": CLASSIC}
SMALL.update({"tail_%d" % r: PLANNED for r in TAILS})
CAPPED = ("capped_few", "capped_heavy")
# follow-up tiles that the layout fixes by construction (straddling full tiles + the partial tile)
IRREGULAR = {"straddle_hot_then_one": 1, "straddle_one_then_hot": 1, "three_groups_in_a_wave": 1, "every_lane_its_group": 1,
             "tail_alone_in_its_d1": 1}


def _child(tmp, tag, extra_env):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    for k in ("GS_LSB_MODE", "GS_LSB_KEYS_PLAN", "GS_LSB_PLAN_SCATTER2", "GS_LSB_PLAN_PEEK", "GS_LSB_PLAN_FINISH_CAP", "GS_MSB_DEDUPE"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_trim_child.py"), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0 and "trim child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_trim")
    return (_child(tmp, "look", {}), _child(tmp, "nolook", {"GS_LSB_PLAN_PEEK": "0"}), _child(tmp, "classic", {"GS_LSB_KEYS_PLAN": "classic"}))


def test_every_case_ran(runs):
    for r in runs:
        assert set(r) == set(SMALL) | set(CAPPED)


def _agree(case, look, nolook, classic):
    for tag, r in (("look", look), ("no look", nolook), ("classic", classic)):
        assert r["guards"], "a guard band changed (%s)" % tag
    assert look["sha"] == nolook["sha"] == classic["sha"], "the modes differ"
    assert look["sel"] == nolook["sel"] == classic["sel"], "the selector depends on the mode"
    assert look["status"] == nolook["status"], "the plan depends on the host's look"
    assert look["cursor"] == nolook["cursor"], "the follow-up tiles depend on the host's look"
    assert classic["status"] == [0] * 8 and classic["cursor"] == [0] * 4, "GS_LSB_KEYS_PLAN=classic must not look"


@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_case(runs, case):
    look, nolook, classic = (r[case] for r in runs)
    _agree(case, look, nolook, classic)
    for tag, r in (("look", look), ("no look", nolook), ("classic", classic)):
        assert r["ok_numpy"], "the sort differs from numpy (%s, route %d)" % (tag, r["status"][0])
    assert look["status"] == look["rule"], "device plan %s, plan rule %s" % (look["status"], look["rule"])
    assert look["status"][0] == SMALL[case]
    if SMALL[case] == PLANNED:
        tail = 1 if look["n"] % 8192 else 0
        assert look["cursor"] == [1, look["irregular"], look["irregular"] - tail, 0], \
            "follow-up tiles: device %s, numpy %d" % (look["cursor"], look["irregular"])
    else:
        assert look["cursor"] == [0] * 4, "a CLASSIC sort reports cursor mode"
    if case in IRREGULAR:
        assert look["irregular"] == IRREGULAR[case]
    if case.startswith("graph_"):
        assert look["peek"] == [0, 0, 4, 15], "a captured sort has no mailbox: the fixed sequence"
    else:
        classes = sum(1 << c for c in range(4) if look["status"][3 + c])
        assert look["peek"] == ([1, PLANNED, 2, classes] if SMALL[case] == PLANNED else [1, CLASSIC, 4, 0])
        assert nolook["peek"] == [0, 0, 4, 15]


@pytest.mark.parametrize("case", CAPPED)
def test_capped_leftover_launches(runs, gs, case):
    look, nolook, classic = (r[case] for r in runs)
    _agree(case, look, nolook, classic)
    cap = gs.lib.gs_lsb_plan_finish_cap()
    assert look["groups"] == cap + cap // 2 > cap, "the leftover launches must stride"
    for tag, r in (("look", look), ("no look", nolook), ("classic", classic)):
        assert r["inversions"] == 0 and r["multiset"], "%s: %d inversions, multiset kept: %s" % (tag, r["inversions"], r["multiset"])
    st = look["status"]
    assert st[0] == PLANNED and st[3:7] == [0, 0, 0, look["groups"]] and st[2] == look["groups"] and st[7] == look["n"]
    assert 9217 <= st[1] <= 17408
    assert look["peek"] == [1, 1, 2, 8]
    assert nolook["peek"] == [0, 0, 4, 15]
