"""gs_msb_sort_u32 path by path, on inputs BUILT for it (tests/msb_cases.py): every classification edge at every level, the
heavy-hitter decision and scatter on both sides of every limit, and the local-sort plans of every class on both sides of theirs.

What is compared: the lists gs_msb_classify_upto reads back against oracle.msb_level_lists (keys), the census of the full sort
against the restatement built on oracle.msb_classify_counts and oracle.msb_heavy_hitter (keys and pairs; level by level:
buckets, keys, tasks per class, task_keys, pivot_buckets, pivot_keys, overflow == 0), the census word `flagged` against the rule
in msb_cases' docstring, and the result bit for bit against numpy's sort of the images, mapped back to uint32 / int32 / float32.
Nothing has a tolerance.

What can only be inferred, not observed (no census word tells, and the task records' `pad` word is not read back):
  * which of the one-pass plan's two abandon conditions fired (16 keys in a bin, 255 in a byte counter, `old + cnt > 255` in the
    wave-uniform branch): every one of them sets `flagged`, and a bin of 255 keys has passed 16 before;
  * that LS_DD was set by the sample look, and that the few-distinct-values plan (LS_DEDUPE / LS_DEDUPE_ALL) rather than the
    general plan sorted a task: the result is exact with the plan on, and the same bytes with GS_MSB_DEDUPE=0;
  * the replica count the few-distinct plan chose (256 / 512 / 1024 distinct values)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import msb_cases as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------- running --
def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(dev)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def run_sort(dev, keys, kt, vals=None, stream=None, synchronize=True):
    """rdxsrt_unstable_sort on uint32 bit patterns of key type kt: (sorted keys, sorted values or None, census)."""
    import gpu_sort_amd as gs
    from gpu_sort_amd.msb import msb_census
    n = keys.size
    dk, ka = _dev(keys, dev), torch.empty(n, dtype=torch.int32, device=dev)
    dv, va = (_dev(vals, dev), torch.empty(n, dtype=torch.int32, device=dev)) if vals is not None else (None, None)
    dm = torch.empty(gs.lib.gs_msb_temp_bytes(n, int(vals is not None)), dtype=torch.uint8, device=dev)
    if stream is None:
        seq = gs.rdxsrt_unstable_sort(dk, dv, n, ka, va, pre_allocated_dm=dm, key_type=kt)
    else:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            seq = gs.rdxsrt_unstable_sort(dk, dv, n, ka, va, pre_allocated_dm=dm, key_type=kt, stream=stream, synchronize=synchronize)
        torch.cuda.synchronize()
    assert seq.sorted_keys is dk
    return _host(dk), (_host(dv) if vals is not None else None), msb_census(dm, n, vals is not None)


def assert_census(got, r, pairs, what):
    """Level by level against the restatement; `flagged` by the rule (predict_flagged), where the rule can tell."""
    for L in range(4):
        for f in M.CENSUS_FIELDS:
            assert got[L][f] == r.census[L][f], f"{what}: level {L} {f}: census {got[L][f]}, restatement {r.census[L][f]}"
        assert got[L]["overflow"] == 0, f"{what}: level {L} overflow"
        want = M.predict_flagged(r, L, pairs)
        if want is not None:
            assert (got[L]["flagged"] != 0) == want, f"{what}: level {L} flagged {got[L]['flagged']}, the rule says {want}"


def assert_keys(img, kt, got, what):
    exp = M.from_image(np.sort(img), kt)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} keys differ from the reference, the first at {bad[:4]}"


def assert_pairs(img, kt, keys, vals, ks, vs, enumerated, what):
    assert_keys(img, kt, ks, what)
    pin = np.sort(keys.astype(np.uint64) << np.uint64(32) | vals.astype(np.uint64))
    pout = np.sort(ks.astype(np.uint64) << np.uint64(32) | vs.astype(np.uint64))
    assert np.array_equal(pin, pout), what + ": the (key, value) pairs are not the input's"
    if enumerated:                                    # on the images: the checker compares keys as unsigned
        assert O.msb_check_pairs_enumerated(np.asarray(img), M.to_image(ks, kt), vs) == 0, what + ": a value names a different key"


def check_lists(dev, img, what, stops=(0, 1, 2)):
    """gs_msb_classify_upto's bucket and task lists against oracle.msb_level_lists, heavy hitters off and on."""
    from gpu_sort_amd.msb import msb_classify_upto
    n = img.size
    for pivot in (False, True):
        for stop in stops:
            exp_b, exp_t = O.msb_level_lists(np.asarray(img), stop, pivot=pivot)
            got_b, got_t, _ = msb_classify_upto(_dev(img, dev), torch.empty(n, dtype=torch.int32, device=dev), n, stop, pivot=pivot)
            assert got_b == exp_b, f"{what}: pivot={pivot} stop={stop}: buckets differ: {sorted(got_b ^ exp_b)[:4]}"
            for c in range(4):
                assert got_t[c] == exp_t[c], f"{what}: pivot={pivot} stop={stop} class {c}: {sorted(got_t[c] ^ exp_t[c])[:4]}"
            assert (exp_b, exp_t) == M.task_lists(M.restate_cached(img, pivot), stop)


def check_sorts(dev, img, what, key_types=M.KEY_TYPES, pairs_types=M.KEY_TYPES, random_values=True):
    """Keys and pairs of every key type: exact result and the census of the restatement."""
    r = M.restate_cached(img)
    n = img.size
    for kt in key_types:
        keys = M.from_image(img, kt)
        got, _, cen = run_sort(dev, keys, kt)
        assert_keys(img, kt, got, f"{what} keys kt={kt}")
        assert_census(cen, r, False, f"{what} keys kt={kt}")
    for kt in pairs_types:
        keys = M.from_image(img, kt)
        modes = [("enumerated", np.arange(n, dtype=np.uint32))]
        if random_values and kt == pairs_types[0]:
            modes.append(("random", np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)))
        for mode, vals in modes:
            ks, vs, cen = run_sort(dev, keys, kt, vals)
            assert_pairs(img, kt, keys, vals, ks, vs, mode == "enumerated", f"{what} pairs kt={kt} {mode}")
            assert_census(cen, r, True, f"{what} pairs kt={kt} {mode}")


# ----------------------------------------------------------------------------------- 1. classification edges --
@pytest.mark.parametrize("label,level,img", M.classify_inputs(), ids=[x[0] for x in M.classify_inputs()])
def test_classification_edges(gs, cuda, label, level, img):
    """Merge sums of 2999 / 3000 from 2, 3 and 255 sub-buckets, run boundaries, the any_small shortcut and its neighbour, every
    class cap -- as the bucket of level 0, and as buckets of level 1 and of level 2."""
    r = M.restate_cached(img)
    at = [t for t in r.tasks if t.level == level]
    assert all(t.bits == (32 if t.merged else 24) - 8 * level for t in at)
    check_lists(cuda, img, label)
    check_sorts(cuda, img, label)


@pytest.mark.parametrize("which", ["one", "three"])
def test_level3_scatter(gs, cuda, which):
    """Buckets of 17409 keys and more that share three bytes: the last-byte scatter finishes them (no value dominant)."""
    img = M.level3_input(which)
    r = M.restate_cached(img)
    assert r.census[3]["buckets"] == {"one": 1, "three": 3}[which] and sum(c["pivot_buckets"] for c in r.census) == 0
    check_lists(cuda, img, f"level3-{which}")
    check_sorts(cuda, img, f"level3-{which}")


def test_many_buckets(gs, cuda):
    """250 buckets at level 1 and 250 at level 2 (a level-1 bucket is a top byte: 256 at most)."""
    img = M.many_buckets_input()
    check_lists(cuda, img, "many buckets", stops=(1, 2))
    check_sorts(cuda, img, "many buckets", key_types=(M.U32,), pairs_types=(M.F32,), random_values=False)


# ------------------------------------------------------------------------------------------- 2. heavy hitters --
@pytest.mark.parametrize("level", [1, 2])
def test_heavy_hitter_decision_and_scatter(gs, cuda, level):
    """Every case of msb_cases.HH_CASES as a bucket of `level`: eq at and one below half, less / greater at and over the largest
    class, strangers in every class and none at all, a dominant value the probes miss or that 2 / 3 of the 16 samples show, full
    and ragged last tiles, buckets behind odd-sized neighbours.  The exact census says which buckets took the path; the strangers' tasks carry rb + 8 bits."""
    img, info = M.hh_input(level)
    r = M.restate_cached(img)
    taken = [c for c, _, _ in info if c.taken]
    assert r.census[level]["pivot_buckets"] == len(taken) and r.census[level]["pivot_keys"] == sum(c.less + c.eq + c.greater for c in taken)
    strangers = [t for t in r.tasks if t.level == level and t.stranger]
    assert strangers and all(t.bits == 32 - 8 * level for t in strangers)
    check_lists(cuda, img, f"heavy hitters L{level}")
    check_sorts(cuda, img, f"heavy hitters L{level}")
    # with the path switched off for the call, no bucket takes it
    assert M.restate_cached(img, False).census[level]["pivot_buckets"] == 0


def test_heavy_hitter_bucket_of_256_tiles_at_an_odd_offset(gs, cuda):
    img, [(case, pre, dom)] = M.hh_big_input()
    r = M.restate_cached(img)
    assert r.census[1]["pivot_buckets"] == 1 and r.buckets[1][-1][0] % 64 != 0
    check_lists(cuda, img, "heavy hitter, 256 tiles", stops=(1,))
    check_sorts(cuda, img, "heavy hitter, 256 tiles", key_types=(M.U32, M.F32), pairs_types=(M.I32,), random_values=False)


def test_whole_array_dominated(gs, cuda):
    """One value in 30000 of 30100 keys: level 0 has no heavy-hitter rule, the path is taken at level 1 and not before."""
    img, dom = M.hh_whole_array_input()
    r = M.restate_cached(img)
    assert r.census[0]["pivot_buckets"] == 0 and r.census[1]["pivot_buckets"] == 1 and r.census[1]["pivot_keys"] == 30000
    check_lists(cuda, img, "whole array dominated", stops=(0, 1))
    check_sorts(cuda, img, "whole array dominated")


# ----------------------------------------------------------------------------------------- 3. local-sort plans --
def test_single_task_sizes(gs, cuda):
    """Arrays of one task on all 32 bits: 1, 63, 64 keys and every class at and below its cap, one key in 8 all ones."""
    for n in M.SINGLE_SIZES:
        check_sorts(cuda, M.single_task_input(n), f"single task n={n}", random_values=False)


@pytest.mark.parametrize("case", M.OP_CASES, ids=[c.name for c in M.OP_CASES])
def test_onepass_plan_limits(gs, cuda, case):
    """The one-pass plan on both sides of its limits.  The rule for the census word `flagged` of the level (msb_cases'
    docstring): with no skew in the level and only 16-bit tasks in the one-pass classes it is 0 exactly when no value of a task
    occurs 16 times; with skew, 3 equal keys among the 64 sampled set it as well."""
    for pairs in (False, True):
        for cls in M.onepass_classes(pairs):
            img = M.onepass_input(case.name, cls)
            r = M.restate_cached(img)
            what = f"one-pass {case.name} class {cls} pairs={pairs}"
            assert M.predict_flagged(r, 1, pairs) is case.flagged, what
            for kt in M.KEY_TYPES:
                keys = M.from_image(img, kt)
                vals = np.arange(img.size, dtype=np.uint32) if pairs else None
                ks, vs, cen = run_sort(cuda, keys, kt, vals)
                if pairs:
                    assert_pairs(img, kt, keys, vals, ks, vs, True, what)
                else:
                    assert_keys(img, kt, ks, what)
                assert_census(cen, r, pairs, what)
                assert (cen[1]["flagged"] != 0) == case.flagged, what


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()


def few_distinct_report(dev):
    """Sorted-key digests of the few-distinct inputs, keys and pairs, for every key type: {name: sha256}."""
    out = {}
    for pairs in (False, True):
        img, _ = M.few_distinct_input(pairs)
        for kt in M.KEY_TYPES:
            keys = M.from_image(img, kt)
            ks, _, _ = run_sort(dev, keys, kt, np.arange(img.size, dtype=np.uint32) if pairs else None)
            out[f"pairs={int(pairs)} kt={kt}"] = _digest(ks)
    return out


@pytest.mark.parametrize("pairs", [False, True])
def test_few_distinct_values_plan_edges(gs, cuda, pairs):
    """16-bit tasks with exactly 1 ... 2049 distinct values (the replica steps at 256 / 512 / 1024, DD_MAX = 2048) in every
    class that compiles the plan, through LS_DEDUPE (after a flagged one-pass) and LS_DEDUPE_ALL."""
    img, info = M.few_distinct_input(pairs)
    assert {cls for cls, _, _, _ in info} == set(M.dedupe_classes(pairs))
    if pairs:
        check_sorts(cuda, img, "few distinct", key_types=())
    else:
        check_lists(cuda, img, "few distinct", stops=(1,))
        check_sorts(cuda, img, "few distinct", pairs_types=())


def test_few_distinct_values_plan_switched_off_gives_the_same_bytes(gs, cuda):
    """GS_MSB_DEDUPE=0 is read once per process: one child sorts every few-distinct input with the plan off."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys, json, torch\nsys.path[:0] = [%r, %r]\nimport test_msb_paths_gpu as P\n"
              "print(json.dumps(P.few_distinct_report(torch.device('cuda:0'))))\n") % (root, os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300, env=dict(os.environ, GS_MSB_DEDUPE="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    off = json.loads(r.stdout.strip().splitlines()[-1])
    on = few_distinct_report(cuda)
    assert off == on
    for pairs in (False, True):
        img = M.few_distinct_input(pairs)[0]
        for kt in M.KEY_TYPES:
            assert on[f"pairs={int(pairs)} kt={kt}"] == _digest(M.from_image(np.sort(img), kt))


# ------------------------------------------------------------------------------- 4. without the host's look --
def async_inputs():
    return [("L0-caps", M.classify_input(0, "caps")), ("L2-tables", M.classify_input(2)), ("level3-three", M.level3_input("three")),
            ("heavy hitters L2", M.hh_input(2)[0]), ("one-pass k16", M.onepass_input("k16", 3)),
            ("one-pass look_flag", M.onepass_input("look_flag", 3)), ("few distinct", M.few_distinct_input(True)[0])]


@pytest.mark.parametrize("pairs", [False, True])
def test_same_cases_without_the_host_look(gs, cuda, pairs):
    """synchronize=False on a side stream: no look at the next level, worst-case grids, blocks that find no task exit.  The same
    sorted bytes and the same census, word for word, as the synchronous run."""
    side = torch.cuda.Stream()
    for name, img in async_inputs():
        kt = M.F32 if pairs else M.I32
        keys = M.from_image(img, kt)
        vals = np.arange(img.size, dtype=np.uint32) if pairs else None
        ks0, vs0, cen0 = run_sort(cuda, keys, kt, vals)
        ks1, vs1, cen1 = run_sort(cuda, keys, kt, vals, stream=side, synchronize=False)
        assert_keys(img, kt, ks1, f"async {name}")
        assert np.array_equal(ks0, ks1) and cen0 == cen1, f"async {name}: {cen0} / {cen1}"
        if pairs:
            assert_pairs(img, kt, keys, vals, ks1, vs1, True, f"async {name}")
        assert_census(cen1, M.restate_cached(img), pairs, f"async {name}")


def test_heavy_hitter_case_captured_in_a_graph(gs, cuda):
    """The level-2 heavy-hitter input captured once and replayed twice."""
    from gpu_sort_amd.msb import msb_census
    img = M.hh_input(2)[0]
    n = img.size
    keys = M.from_image(img, M.U32)
    src = _dev(keys, cuda)
    a, b = src.clone(), torch.empty_like(src)
    temp = torch.empty(gs.lib.gs_msb_temp_bytes(n, 0), dtype=torch.uint8, device=cuda)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gs.rdxsrt_unstable_sort(a, None, n, b, None, pre_allocated_dm=temp, stream=side, synchronize=False)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        a.copy_(src)
        seq = gs.rdxsrt_unstable_sort(a, None, n, b, None, pre_allocated_dm=temp, synchronize=False)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert_keys(img, M.U32, _host(seq.sorted_keys), "graph replay")
        assert_census(msb_census(temp, n), M.restate_cached(img), False, "graph replay")
