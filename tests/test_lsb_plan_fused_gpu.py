"""The fused look of the keys-only plan (gs_lsb_plan.hip): the look's one read of the input also counts
bits 16-23 per tile and leaves the spine and prefix16 of the first PLANNED scatter, so that slot 1's upsweep returns at once
when the plan is PLANNED and runs, at shift 0, over the look's counts when it is CLASSIC.

GS_LSB_KEYS_PLAN and GS_LSB_PLAN_MIN_ITEMS are read once per process, so the cases run in two child processes
(tests/lsb_plan_fused_child.py), one with the plan reachable from 65536 keys and one with GS_LSB_KEYS_PLAN=classic; both run
once per session.  The look-only tests stand first: wrong counts are seen before a scatter uses them.

The sizes stand in a fixed relation to the geometry (tile 8192 keys, chunk 65536 keys, look grid min(n / 32768, 256), a look
workgroup takes one unit of two chunks at a time and walks the units slot, slot + grid, ...): one chunk; a second chunk of two
tiles, the last of one key; one chunk fewer than, as many as and more chunks than look workgroups, with a ragged last chunk
and tile; 385 chunks = 193 units, which is still at most one unit per workgroup; and 1030 chunks = 515 units on 256
workgroups, where every workgroup walks two units and some walk three, so the wave counters are cleared between units and
the results of a unit are written while the next one waits: the production sizes (2^28 keys and more) walk 8 units and more."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLANNED, CLASSIC = 1, 2
SKIP = 0xFFFFFFFF
TILE, CHUNK = 8192, 65536
N_257 = 257 * CHUNK + 3 * TILE + 5
N_WALK = 3 * (1 << 23) + 3 * TILE + 5
LOOK_GRID, LOOK_UNIT_CHUNKS = 256, 2
N_THREE_UNITS = (2 * LOOK_GRID * LOOK_UNIT_CHUNKS + 5) * CHUNK + 3 * TILE + 5

# look-only case -> the route the decision must take (the spine and prefix16 are those of bits 16-23 on either route)
LOOKS = {
    "look_uniform_%d" % CHUNK: PLANNED, "look_uniform_%d" % (9 * TILE + 1): PLANNED,
    "look_uniform_%d" % (255 * CHUNK): PLANNED, "look_uniform_%d" % (256 * CHUNK): PLANNED,
    "look_uniform_%d" % N_257: PLANNED, "look_uniform_%d" % N_WALK: PLANNED,
    "look_uniform_%d" % N_THREE_UNITS: PLANNED,
    "look_sorted": PLANNED, "look_runs_of_16": PLANNED, "look_i32_desc": PLANNED, "look_f32_specials": CLASSIC,
}
SORTS = {
    "sort_uniform_257": PLANNED, "sort_uniform_walk": PLANNED, "sort_planted_walk": CLASSIC, "sort_i32_desc": PLANNED,
    "sort_f32_asc": CLASSIC, "sort_uniform_three_units": PLANNED, "sort_planted_three_units": CLASSIC,
    "reuse_0": PLANNED, "reuse_1": CLASSIC, "reuse_2": PLANNED, "reuse_3": CLASSIC,
    "graph_0": PLANNED, "graph_1": CLASSIC, "graph_2": CLASSIC, "graph_3": PLANNED,
    "reuse_three_units_0": PLANNED, "reuse_three_units_1": CLASSIC, "reuse_three_units_2": PLANNED, "reuse_three_units_3": CLASSIC,
    "graph_three_units_0": PLANNED, "graph_three_units_1": CLASSIC, "graph_three_units_2": CLASSIC, "graph_three_units_3": PLANNED,
}


def _child(tmp, tag, extra_env):
    out = os.path.join(str(tmp), tag + ".json")
    env = dict(os.environ, GS_LSB_PLAN_MIN_ITEMS="65536", **extra_env)
    env.pop("GS_LSB_MODE", None)
    if "GS_LSB_KEYS_PLAN" not in extra_env:
        env.pop("GS_LSB_KEYS_PLAN", None)
    p = subprocess.run([sys.executable, os.path.join(HERE, "lsb_plan_fused_child.py"), out], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fused child ok" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, cuda):
    tmp = tmp_path_factory.mktemp("lsb_plan_fused")
    return _child(tmp, "plan", {}), _child(tmp, "classic", {"GS_LSB_KEYS_PLAN": "classic"})


def _status_matches(status, rule, route):
    if rule[1] < 65536:
        assert status == rule, "device plan %s, plan rule %s" % (status, rule)
    else:
        # a group of 65536 keys or more can wrap a 16-bit counter of the look: the sort then only knows that the group is
        # too large (CLASSIC), and the sizes it reports are those of the wrapped counters
        assert status[0] == CLASSIC and status[3:7] == [0, 0, 0, 0]
    assert status[0] == route


# ---- the look alone

def test_every_case_ran(runs):
    plan, classic = runs
    assert set(plan) == set(LOOKS) | set(SORTS)
    assert set(classic) == {"look_refused"} | set(SORTS)


@pytest.mark.parametrize("case", sorted(LOOKS))
def test_look_leaves_the_first_scatters_counts(runs, case):
    """spine and prefix16 after gs_lsb_plan_look_only equal numpy's word for word, and the plan block's head holds the
    decision: status, digit positions of the slots, and the upsweep flags (PLANNED: only slot 2's upsweep counts)."""
    r = runs[0][case]
    assert r["guards"], "a guard band or the input changed"
    assert r["grid"] == r["grid_expected"]
    assert r["spine_bad"] == 0, "%d spine words differ" % r["spine_bad"]
    assert r["prefix_bad"] == 0, "%d prefix16 words differ" % r["prefix_bad"]
    head = r["head"]
    _status_matches(head[:8], r["rule"], LOOKS[case])
    if head[0] == PLANNED:
        assert head[8:16] == [16, 24, SKIP, SKIP, 1, 0, 1, 1]
    else:
        assert head[8:16] == [0, 8, 16, 24, 0, 0, 0, 0]


def test_look_only_needs_the_plan(runs):
    """With GS_LSB_KEYS_PLAN=classic no sort looks: the hook and the layout query refuse, and nothing is written."""
    r = runs[1]["look_refused"]
    assert r["refused"] and r["guards"]


# ---- whole sorts

@pytest.mark.parametrize("case", sorted(SORTS))
def test_sort_case(runs, case):
    plan, classic = runs
    p, c = plan[case], classic[case]
    assert p["guards"] and c["guards"], "a guard band changed"
    assert c["ok_numpy"], "the four passes differ from numpy"
    assert p["ok_numpy"], "the planned sort differs from numpy (route %d)" % p["status"][0]
    assert p["sha"] == c["sha"], "the two modes differ"
    assert p["sel"] == c["sel"], "the selector depends on the route"
    _status_matches(p["status"], p["rule"], SORTS[case])
    assert c["status"] == [0] * 8, "GS_LSB_KEYS_PLAN=classic must not look"


def test_planted_group_is_one_key_above_the_cap(runs):
    assert runs[0]["sort_planted_walk"]["status"][:2] == [CLASSIC, 17409]
    assert runs[0]["sort_planted_three_units"]["status"][:2] == [CLASSIC, 17409]


def test_the_largest_size_walks_three_units():
    """The size that stands for "workgroups walk several units" does so under the look's geometry."""
    chunks = (N_THREE_UNITS + CHUNK - 1) // CHUNK
    units = (chunks + LOOK_UNIT_CHUNKS - 1) // LOOK_UNIT_CHUNKS
    assert min(N_THREE_UNITS // 32768, 256) == LOOK_GRID and units > 2 * LOOK_GRID
    assert N_THREE_UNITS % CHUNK and N_THREE_UNITS % TILE
