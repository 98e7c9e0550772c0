"""The CPU half of tests/test_msb_paths_gpu.py: every builder of tests/msb_cases.py is held to its intent without a device --
the 256 counts of every built bucket, the class and sort bits oracle.msb_classify_counts gives every named run, the decision of
oracle.msb_heavy_hitter, the fullest bin of every one-pass task, the distinct values of every few-distinct task, what the 64
sampled positions show, the key images of the three key types, and that every row of the plan table is reached."""
import numpy as np
import pytest

import msb_cases as M
from oracle import oracle as O


def _special_patterns():
    return np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
                     0x3F800000, 0xBF800000, 0x00800000, 0x007FFFFF], np.uint32)


@pytest.mark.parametrize("kt", M.KEY_TYPES)
def test_images_map_back_and_forth(kt):
    from test_buffer_contracts_gpu import ordmap
    keys = np.concatenate((_special_patterns(), np.random.default_rng(kt).integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)))
    img = M.to_image(keys, kt)
    assert np.array_equal(img.astype(np.uint64), ordmap(keys, kt))
    assert np.array_equal(M.from_image(img, kt), keys)
    built = M.classify_input(1)
    assert np.array_equal(M.to_image(M.from_image(built, kt), kt), built)
    if kt == M.I32:                                   # the order of the images is the order of the keys
        assert np.array_equal(np.argsort(img, kind="stable"), np.argsort(keys.view(np.int32), kind="stable"))
    if kt != M.U32:                                   # negative keys, and for floats -0.0 and NaN patterns, are in the built inputs
        back = M.from_image(M.hh_input(1)[0], kt)
        assert (back & np.uint32(0x80000000)).any() and (~back & np.uint32(0x80000000)).any()
    assert M.from_image(np.array([0x7FFFFFFF], np.uint32), M.F32)[0] == 0x80000000      # -0.0 is an ordinary key


def test_plan_table_is_the_code_rule():
    for (mb, cls, pairs), seq in M.PLAN_TABLE.items():
        assert M.plan_from_code(mb, cls, pairs) == seq, (mb, cls, pairs)
    assert {c for c in range(4) if M.ONEPASS in M.PLAN_TABLE[(16, c, False)]} == set(M.onepass_classes(False))
    assert {c for c in range(4) if M.ONEPASS in M.PLAN_TABLE[(16, c, True)]} == set(M.onepass_classes(True))
    for pairs in (False, True):
        assert {c for c in range(4) if any(isinstance(x, tuple) for x in M.PLAN_TABLE[(16, c, pairs)])} == set(M.dedupe_classes(pairs))


@pytest.mark.parametrize("name", M.TABLE_NAMES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_tables_classify_as_named(name, level):
    """oracle.msb_classify_counts puts every named run / single / bucket where the table says, with the bits of the level."""
    counts, expect = M.table_counts(name)
    assert counts.sum() > M.CAP_MAX                   # it is a bucket of its level at all
    rb = 24 - 8 * level
    b, t = O.msb_classify_counts(counts, 1000, level)
    starts = 1000 + np.concatenate(([0], np.cumsum(counts[:-1])))
    exp_b = [(int(starts[d]), s) for kind, d, s, _ in expect if kind == "bucket"]
    exp_t = [(O.msb_class_of(s), int(starts[d]), s, rb + (8 if kind == "run" else 0)) for kind, d, s, _ in expect if kind != "bucket"]
    assert b == exp_b and t == exp_t
    for kind, d, s, nsub in expect:
        assert (kind == "run") == (nsub > 1) and (kind != "bucket" or s > M.CAP_MAX) and (kind == "bucket" or s <= M.CAP_MAX)
        assert kind != "run" or s < M.MERGE


def test_tables_hold_the_edges_the_issue_names():
    runs = {(s, n) for name in M.TABLE_NAMES for kind, d, s, n in M.table_counts(name)[1] if kind == "run"}
    assert {(2999, 2), (2999, 3), (2999, 255), (2794, 254), (2000, 2), (2047, 2), (2048, 2), (2049, 2), (2, 2)} <= runs
    singles = {s for name in M.TABLE_NAMES for kind, d, s, n in M.table_counts(name)[1] if kind == "single"}
    assert {1, 63, 64, 2047, 2048, 2049, 4607, 4608, 4609, 9215, 9216, 9217, 17407, 17408, 2999, 3000, 3001} <= singles
    first = {d for name in M.TABLE_NAMES for kind, d, s, n in M.table_counts(name)[1] if kind == "run"}
    assert 0 in first and 254 in first                # a run from digit 0, a run up to digit 255
    small = lambda name: int(((M.table_counts(name)[0] > 0) & (M.table_counts(name)[0] < M.MERGE)).sum())
    assert small("no_small") == 0 and small("one_small") == 1
    # a threshold of 3001 or 2999, or a cap off by one, changes what the oracle says about these tables
    c = M.table_counts("merge_sums")[0]
    assert [x[2] for x in O.msb_classify_counts(c, 0, 1)[1]] == [2999, 3000, 2000, 1000, 3000, 2999, 3000, 2000, 1000, 3000]


@pytest.mark.parametrize("label,level,img", M.classify_inputs(), ids=[x[0] for x in M.classify_inputs()])
def test_classify_inputs_hold_their_tables(label, level, img):
    """The built arrays hold the tables' counts under the right prefixes, and the restatement is oracle.msb_level_lists."""
    names = [label[3:]] if level == 0 else M.TABLE_NAMES
    for top, name in zip(M.TABLE_TOPS, names):
        pre = () if level == 0 else (top,) if level == 1 else (top, 0x33)
        sub = img if level == 0 else img[M.positions_of(img, pre)]
        digit = (sub >> np.uint32(24 - 8 * level)) & np.uint32(0xff)
        assert np.array_equal(np.bincount(digit, minlength=256), M.table_counts(name)[0]), (label, name)
    for pivot in (False, True):
        r = M.restate(img, pivot)
        for stop in range(3):
            eb, et = O.msb_level_lists(img, stop, pivot=pivot)
            gb, gt = M.task_lists(r, stop)
            assert gb == eb and gt == et, (label, pivot, stop)
    r = M.restate_cached(img)
    at = [t for t in r.tasks if t.level == level]
    assert {t.bits for t in at if t.merged} <= {32 - 8 * level} and {t.bits for t in at if not t.merged} <= {24 - 8 * level}
    assert level == 0 or any(not t.merged for t in at)
    assert r.census[0]["pivot_buckets"] == 0 and sum(c["task_keys"] for c in r.census) + r.census[3]["keys"] == img.size


def test_level3_and_many_buckets_inputs():
    one = M.restate(M.level3_input("one"))
    assert [c["buckets"] for c in one.census] == [1, 1, 1, 1] and one.census[3]["keys"] == M.CAP_MAX + 1 and not one.tasks
    assert sum(c["pivot_buckets"] for c in one.census) == 0
    assert np.unique(M.level3_input("one") & np.uint32(0xff)).size == 256
    three = M.restate(M.level3_input("three"))
    assert three.census[3]["buckets"] == 3 and sorted(s for _, s in three.buckets[3]) == [17409, 17411, 20001]
    assert all(o % 2 == 1 for o, _ in three.buckets[3]) and sum(c["pivot_buckets"] for c in three.census) == 0
    many = M.restate_cached(M.many_buckets_input())
    assert many.census[1]["buckets"] == M.MANY and many.census[2]["buckets"] == M.MANY and many.census[3]["buckets"] == 0
    assert {t.bits for t in many.tasks} == {16} and all(t.merged for t in many.tasks)


@pytest.mark.parametrize("level", [1, 2])
def test_heavy_hitter_cases_decide_as_intended(level):
    img, info = M.hh_input(level)
    r = M.restate_cached(img)
    assert len(info) == len(M.HH_CASES)
    by_off = {o: s for o, s in r.buckets[level]}
    S = np.sort(img)
    taken = 0
    for case, pre, dom in info:
        idx = M.positions_of(img, pre)
        content = img[idx]
        size = case.less + case.eq + case.greater
        assert content.size == size and int((content == dom).sum()) == case.eq and int((content < dom).sum()) == case.less
        off = int(np.searchsorted(S, content.min()))
        assert by_off.get(off) == size, case.name                        # it is a bucket of this level ...
        hh = O.msb_heavy_hitter(content)                                # ... and the rule decides as the case says
        assert (hh is not None) == case.taken, case.name
        probes, samples = content[M.hh_probes(size)] == dom, content[M.hh_samples(size)] == dom
        if case.seen is True or case.seen is False:
            assert probes.all() == samples.all() == case.seen and probes.any() == samples.any() == case.seen, case.name
        else:                                         # at the probes, and in exactly case.seen of the 16 samples
            assert probes.all() and int(samples.sum()) == case.seen, case.name
        if case.taken:
            taken += 1
            assert hh == (dom, case.less, case.eq)
            for o, s in ((off, case.less), (off + case.less + case.eq, case.greater)):
                got = [t for t in r.tasks if t.level == level and t.offset == o and t.stranger]
                assert (len(got) == 1 and got[0].size == s and got[0].bits == 32 - 8 * level and got[0].cls == O.msb_class_of(s)) if s else not got
    assert r.census[level]["pivot_buckets"] == taken == sum(c.taken for c in M.HH_CASES)
    assert r.census[level]["pivot_keys"] == sum(c.less + c.eq + c.greater for c in M.HH_CASES if c.taken)
    if level == 2:                                                       # no level-1 bucket is dominated
        assert r.census[1]["pivot_buckets"] == 0
    # the sizes and offsets the issue names
    sizes = {c.name: c.less + c.eq + c.greater for c in M.HH_CASES}
    assert sizes["tiles_full"] == 3 * M.TILE and sizes["tiles_ragged"] == 3 * M.TILE + 1 and sizes["below_half_odd"] % 2 == 1
    assert sizes["half_even"] == 2 * 20000 and any(o % 64 for o in by_off)
    classes = {(O.msb_class_of(c.less) if c.less else None, O.msb_class_of(c.greater) if c.greater else None) for c in M.HH_CASES if c.taken}
    assert {x for p in classes for x in p} == {None, 0, 1, 2, 3}
    # both signs: images below 0x80000000 are negative int32 / float32 keys
    assert any(dom < 0x80000000 for c, _, dom in info if c.taken) and any(dom >= 0x80000000 for c, _, dom in info if c.taken)


def test_heavy_hitter_big_and_whole_array_inputs():
    img, [(case, pre, dom)] = M.hh_big_input()
    r = M.restate(img)
    (off, size), = r.buckets[1][-1:]
    assert size >= M.ALIGN_MIN_TILES * M.TILE and off % 64 != 0 and size == case.less + case.eq + case.greater
    assert r.census[1]["pivot_buckets"] == 1 and r.census[1]["pivot_keys"] == size
    img, dom = M.hh_whole_array_input()
    r = M.restate(img)
    assert int((img == dom).sum()) * 2 > img.size
    assert r.census[0]["pivot_buckets"] == 0 and r.census[1]["pivot_buckets"] == 1 and r.census[1]["pivot_keys"] == 30000
    assert r.census[1]["task_keys"] == 0 and r.census[0]["task_keys"] == 100


@pytest.mark.parametrize("pairs", [False, True])
def test_onepass_tasks_hold_the_stated_bin(pairs):
    for cls in M.onepass_classes(pairs):
        for case in M.OP_CASES:
            img = M.onepass_input(case.name, cls)
            r = M.restate_cached(img)
            at = [t for t in r.tasks if t.level == 1]
            task = next(t for t in at if t.size == M.OP_TASK_SIZE[cls])
            assert task.cls == cls and task.bits == 16 and not task.merged and M.fullest_bin(task.content, 16) == case.k
            others = [t for t in at if t is not task]
            assert len(others) == 1 and others[0].bits == 16 and M.fullest_bin(others[0].content, 16) == 1
            assert bool(r.buckets.get(2)) == bool(case.look) and r.census[1]["pivot_buckets"] == 0
            v = (img[M.positions_of(img, (M.OP_TOP, M.OP_TASK))] & np.uint32(0xffff))
            if case.front:                            # the bin's keys are the first k of the task on the device
                assert (task.content[:case.k] & np.uint32(0xffff) == case.value).all() and (v[:case.k] == case.value).all()
                assert case.k >= 64
            triples, twins = M.sample_counts(task.content, 16)
            if case.look == "triple":
                assert triples == 3 and case.k == 3
            elif case.look == "twins":
                assert triples == 0 and twins == 8
            elif case.look == "distinct":
                assert triples == 0 and twins == 0
            # the rule: flagged exactly when a bin reaches 16 keys or the look sees a triple
            assert M.predict_flagged(r, 1, pairs) is case.flagged, (case.name, cls)
            assert M.predict_flagged(r, 2, pairs) is False and M.predict_flagged(r, 0, pairs) is False


@pytest.mark.parametrize("pairs", [False, True])
def test_few_distinct_tasks_hold_the_stated_values(pairs):
    img, info = M.few_distinct_input(pairs)
    r = M.restate_cached(img)
    assert {(cls, D) for cls, D, _, _ in info} == {(c, D) for c in M.dedupe_classes(pairs) for D in M.FD_DISTINCT}
    S = np.sort(img)
    tasks = {t.offset: t for t in r.tasks if t.level == 1}
    for cls, D, pre, size in info:
        t = tasks[int(np.searchsorted(S, np.uint32(M._prefix(pre) << 16)))]
        assert (t.cls, t.size, t.bits, t.merged) == (cls, size, 16, False)
        low = t.content & np.uint32(0xffff)
        assert np.unique(low).size == D and (low == 0xffff).any()
        triples, twins = M.sample_counts(t.content, 16)
        assert triples >= 3 and twins >= min(64, 11)      # LS_FLAG and LS_DD
    assert len(r.buckets[2]) == len(M.dedupe_classes(pairs)) and r.census[1]["pivot_buckets"] == 0
    assert M.predict_flagged(r, 1, pairs) is True


@pytest.mark.parametrize("pairs", [False, True])
def test_every_row_of_the_plan_table_is_reached(pairs):
    """Every (level, class) gets a task of the level's bits; merged tasks (8 more bits) reach the classes they can (0 and 1); the
    single task reaches every class; and every class whose plan differs for 16-bit tasks gets 16-bit tasks at levels 1 and 2."""
    seen = M.coverage(pairs)
    for (mb, cls, p), seq in M.PLAN_TABLE.items():
        if p != pairs:
            continue
        level = {32: 0, 24: 0, 16: 1, 8: 2}[mb]
        assert (level, cls, mb) in seen, (mb, cls)
        if mb != 32 and cls < 2:
            assert (level, cls, mb + 8) in seen, (mb, cls, "merged")
        if mb in (16, 8) and len(seq) > 1:
            assert (1, cls, 16) in seen and (2, cls, 16) in seen, (cls, "16-bit tasks")
    assert {n for n in M.SINGLE_SIZES} >= {1, 63, 64} | {c - 1 for c in M.CAPS} | set(M.CAPS)
