"""The host's look at the keys-only plan's decision (gs_lsb_plan.hip): unless the stream is being captured
or GS_LSB_PLAN_PEEK=0 is set, gs_lsb_sort_u32 reads the decision on the host once the first pass slot is enqueued and
launches only what the route needs -- two pass slots, the task builder and the local sorts of the classes that have tasks
when PLANNED; four real passes and no finish when CLASSIC.  Without the look one fixed sequence serves both routes.  The
result, the selector, the workspace and what gs_lsb_plan_status / gs_lsb_plan_cursor_status report must not depend on it.

The switches are read once per process, so the cases run in child processes (tests/lsb_plan_peek_child.py), each once per
session and all with the plan reachable from 65536 keys: the default, GS_LSB_PLAN_PEEK=0, GS_LSB_KEYS_PLAN=classic (the four
passes, no plan), and GS_LSB_PLAN_SCATTER2=stable with the look on the class-mix case alone.  For every sort: the result
equals numpy's sort of the order-mapped keys and the guard bands are intact in every mode; the modes agree on the result
bytes and the selector; the default and GS_LSB_PLAN_PEEK=0 agree on both status reports, which equal the plan rule restated in
numpy; GS_LSB_KEYS_PLAN=classic reports zeros; and gs_lsb_plan_peek_status reports what EXPECT states for the default, "no
look, four slots, every class" for GS_LSB_PLAN_PEEK=0 and for a captured call, and zeros where no planned sort ran."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANNED, CLASSIC = 1, 2
P0 = [1, PLANNED, 2, 0b0001]        # uniform keys of these sizes: every group is tiny, class 0 only
C4 = [1, CLASSIC, 4, 0]
NO_LOOK = [0, 0, 4, 0b1111]

# sort -> what gs_lsb_plan_peek_status must report in the default mode
EXPECT = {
    "ragged_planned": P0,
    "class_mix": [1, PLANNED, 2, 0b1111],
    "class_mix_classic": C4,
    "wrapped_classic": C4,                              # a wrapped counter of the look: fewer than n keys counted
    "tiles_24": P0, "tiles_24_plus_1": P0,
    "f32_desc_planned": [1, PLANNED, 2, 0b1101],        # the special values' groups: 3 of class 2, 4 of class 3 (numpy's count)
    "f32_desc_classic": C4,
    "i32_asc_planned": P0, "i32_asc_classic": C4,
    "reuse_0": P0, "reuse_1": C4, "reuse_2": C4, "reuse_3": P0,
    "thread_a_0": P0, "thread_a_1": C4, "thread_a_2": P0, "thread_a_3": C4,
    "thread_b_0": C4, "thread_b_1": P0, "thread_b_2": P0, "thread_b_3": C4,
    "graph_0": NO_LOOK, "graph_1": NO_LOOK,
    "eager_after_graph": C4,
}
# the route of the sorts whose report does not name it
ROUTES = {"graph_0": PLANNED, "graph_1": CLASSIC}
# follow-up tiles that n alone fixes: the partial tile is the follow-up kernel's in cursor mode
HAS_TAIL = {"tiles_24": 0, "tiles_24_plus_1": 1, "ragged_planned": 1}


def _child(tmp, tag, extra_env, only=None):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536")
    for k in ("GS_LSB_MODE", "GS_LSB_KEYS_PLAN", "GS_LSB_PLAN_SCATTER2", "GS_LSB_PLAN_PEEK"):
        env.pop(k, None)
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_peek_child.py"), out] + ([only] if only else []), env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "peek child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_peek")
    return {"peek": _child(tmp, "peek", {}), "nopeek": _child(tmp, "nopeek", {"GS_LSB_PLAN_PEEK": "0"}),
            "classic": _child(tmp, "classic", {"GS_LSB_KEYS_PLAN": "classic"}),
            "stable": _child(tmp, "stable", {"GS_LSB_PLAN_SCATTER2": "stable"}, only="class_mix")}


def test_every_sort_ran(runs):
    for tag in ("peek", "nopeek", "classic"):
        assert set(runs[tag]) == set(EXPECT), tag
    assert set(runs["stable"]) == {"class_mix"}


@pytest.mark.parametrize("case", sorted(EXPECT))
def test_peek_case(runs, case):
    k, o, c = runs["peek"][case], runs["nopeek"][case], runs["classic"][case]
    for tag, r in (("peek", k), ("nopeek", o), ("classic", c)):
        assert r["guards"], "a guard band changed (%s)" % tag
        assert r["ok_numpy"], "the sort differs from numpy (%s, route %d)" % (tag, r["status"][0])
    assert k["sha"] == o["sha"] == c["sha"], "the modes differ"
    assert k["sel"] == o["sel"] == c["sel"], "the selector depends on the mode"
    assert k["status"] == o["status"], "gs_lsb_plan_status depends on the look"
    assert k["cursor"] == o["cursor"], "gs_lsb_plan_cursor_status depends on the look"
    if k["rule"][1] < 65536:
        assert k["status"] == k["rule"], "device plan %s, plan rule %s" % (k["status"], k["rule"])
    else:
        # a group of 65536 keys or more can wrap a 16-bit counter of the look: the sort then only knows that the group is too
        # large (CLASSIC), and the sizes it reports are those of the wrapped counters
        assert k["status"][0] == CLASSIC and k["status"][3:7] == [0, 0, 0, 0] and k["status"][7] <= k["n"]
    assert c["status"] == [0] * 8 and c["cursor"] == [0] * 4 and c["peek"] == [0] * 4, "GS_LSB_KEYS_PLAN=classic must not plan"
    assert k["peek"] == EXPECT[case], "the look: reported %s, expected %s" % (k["peek"], EXPECT[case])
    assert o["peek"] == NO_LOOK, "GS_LSB_PLAN_PEEK=0 looked: %s" % o["peek"]
    route = ROUTES.get(case, EXPECT[case][1])
    assert k["status"][0] == route
    if route == PLANNED:
        assert k["cursor"][0] == 1 and k["cursor"][3] == 0
        tail = 1 if k["n"] % 8192 else 0
        assert k["cursor"][1] == k["cursor"][2] + tail, "the follow-up kernel owns the partial tile"
        if k["peek"][0]:
            # the class bits are those of the classes with tasks
            assert k["peek"][3] == sum(1 << i for i in range(4) if k["status"][3 + i])
    else:
        assert k["cursor"] == [0] * 4, "a CLASSIC sort reports cursor mode"
    if case in HAS_TAIL:
        assert (1 if k["n"] % 8192 else 0) == HAS_TAIL[case]


def test_stable_scatter_with_the_look(runs):
    """GS_LSB_PLAN_SCATTER2=stable: the host reads "no cursor mode" and enqueues the whole stable slot"""
    s, k = runs["stable"]["class_mix"], runs["peek"]["class_mix"]
    assert s["guards"] and s["ok_numpy"]
    assert s["sha"] == k["sha"] and s["sel"] == k["sel"]
    assert s["status"] == k["status"] == s["rule"]
    assert s["cursor"] == [0] * 4, "GS_LSB_PLAN_SCATTER2=stable ran in cursor mode"
    assert s["peek"] == EXPECT["class_mix"]
