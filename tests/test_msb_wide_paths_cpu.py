"""The CPU half of tests/test_msb_wide_paths_gpu.py: its input builders, its restatement of the wide classification and the
assertions about the inputs themselves (every level gets tasks of both classes and a merged task; the fullest bin of a task
is exactly k).  Also shows that the census the GPU tests compare against tells the caps 2048 / 8192 and the merge threshold
3000 from their neighbours."""
import numpy as np
import pytest

import test_msb_wide_paths_gpu as P
from test_buffer_contracts_gpu import F32, F64, I64, KEY_BYTES, U32, U64, gen_keys, ordmap

CENSUS_FIELDS = ("buckets", "tiles", "keys", "task_keys", "tasks")


@pytest.mark.parametrize("kt", [U64, I64, F64, U32, F32])
def test_from_image_inverts_the_order_map(kt):
    keys = np.concatenate([gen_keys(kt, kind, 4000, 3) for kind in ("uniform", "special", "pad")])
    assert np.array_equal(P.from_image(ordmap(keys, kt), kt), keys)
    img = P.build_ladder(8 * KEY_BYTES[kt])
    assert np.array_equal(ordmap(P.from_image(img, kt), kt), img)


def test_restatement_is_the_oracle_rule_with_other_constants(oracle):
    """With the 32-bit sort's caps the generalised rule is oracle.msb_classify_counts, bucket by bucket."""
    rng = np.random.default_rng(2)
    for trial in range(40):
        counts = rng.integers(0, (5, 200, 4000, 30000)[trial % 4], size=256)
        counts[rng.random(256) < 0.3] = 0
        counts[rng.integers(0, 256, 6)] = (2999, 3000, 4608, 4609, 17408, 17409)
        for level in range(3):
            eb, et = oracle.msb_classify_counts(counts, 77, level)
            b, t = P.wide_classify_counts(counts, 77, 24 - 8 * level, caps=oracle.MSB_CLASS_CAPS, merge=oracle.MSB_MERGE)
            assert b == eb and [x[:4] for x in t] == et


@pytest.mark.parametrize("key_bits", [64, 32])
def test_ladder_reaches_every_level(key_bits):
    img = P.build_ladder(key_bits)
    levels = key_bits // 8
    assert img.size == (levels - 1) * sum(P.LADDER_COUNTS + P.LADDER_PAIR) + P.LADDER_DEEP + P.LADDER_EQUAL
    cen, tasks = P.ladder_restatement(key_bits)
    P.assert_ladder_reaches_every_level(key_bits, tasks)
    assert all(cen[L]["buckets"] >= 1 for L in range(levels)) and all(cen[L]["buckets"] == 0 for L in range(levels, 8))
    assert cen[levels - 1]["tasks"] == [0, 0, 0, 0] and cen[levels - 1]["keys"] >= P.LADDER_DEEP + P.LADDER_EQUAL + 8193
    # every key is finished exactly once: by a task or by the last scatter
    assert sum(c["task_keys"] for c in cen) + cen[levels - 1]["keys"] == img.size
    # digits 0 and 255 occur below the top byte, and (as doubles / floats) negative keys, -0.0 and NaN patterns
    below = (img >> np.uint64(key_bits - 16)) & np.uint64(0xff)
    assert (below == 0).any() and (below == 255).any()
    kt = F64 if key_bits == 64 else F32
    k = P.from_image(img, kt)
    sign = np.uint64(1 << (key_bits - 1))
    assert np.count_nonzero(k == sign) == P.LADDER_EQUAL and (k & sign != 0).any() and (k & sign == 0).any()
    f = k.view(np.float64 if key_bits == 64 else np.float32)
    assert np.isnan(f).any()


def test_ladder_has_crowded_and_uncrowded_tasks_at_every_bin_shift():
    """Tasks with 24, 32, 40, 48 and 56 bits left, each with some whose fullest bin stays below 24 keys (the order-free plan
    finishes them) and some with 24 or more (abandoned for the LSD passes)."""
    full = P.task_fullest_bins(P.build_ladder(64), P.ladder_restatement(64)[1])
    for bits in (24, 32, 40, 48, 56):
        mine = [k for t, k in full if t["sort_bits"] == bits]
        assert any(k < P.BIN_LIMIT for k in mine) and any(k >= P.BIN_LIMIT for k in mine), (bits, sorted(mine))


@pytest.mark.parametrize("key_bits", [64, 32])
def test_census_tells_the_caps_and_the_merge_threshold(key_bits):
    """The expected census of the ladder changes at every level 0 .. levels-2 when the largest cap is 8191 or 8193, the small
    cap 2047 or 2049, or the merge threshold 2999 or 3001: the census assertions cannot pass with any of those."""
    img = P.build_ladder(key_bits)
    base = P.ladder_restatement(key_bits)[0]
    for caps, merge in (((2048, 8191), 3000), ((2048, 8193), 3000), ((2047, 8192), 3000), ((2049, 8192), 3000),
                        ((2048, 8192), 2999), ((2048, 8192), 3001)):
        other = P.wide_restatement(img, key_bits, caps, merge)[0]
        for L in range(key_bits // 8 - 1):
            here = any(other[L][f] != base[L][f] for f in CENSUS_FIELDS)
            below = any(other[L + 1][f] != base[L + 1][f] for f in CENSUS_FIELDS)
            assert here or below, (caps, merge, L)
            if caps[0] != 2048 or merge != 3000:
                assert other[L]["tasks"] != base[L]["tasks"], (caps, merge, L)
            else:
                assert other[L + 1]["buckets"] != base[L + 1]["buckets"], (caps, merge, L)


@pytest.mark.parametrize("k", P.FULLEST)
@pytest.mark.parametrize("key_bits", [64, 32])
def test_boundary_inputs_hold_the_tasks_they_name(key_bits, k):
    """Level-1 cases: each is an unmerged task of level 1 with all bits below its byte to sort, and its fullest bin -- by the
    kernel's rule, the top 11 of the task's sort bits -- is exactly min(k, size).  Single-task arrays: the same on all bits."""
    img, info, fullest, (cen, tasks) = P.level1_input(key_bits, k)
    assert len(info) == len(P.SIZES) * 9
    P.assert_embedded(key_bits, img, info, tasks, fullest)
    assert cen[0]["tasks"] == [0, 0, 0, 0] and cen[1]["buckets"] == len(info) and cen[2]["buckets"] == 0
    singles = P.single_task_inputs(key_bits, k)
    for label, simg, full in singles:
        assert simg.size <= 8192 and (full is None or P.fullest_bin(simg, key_bits) == full), label
        if " distinct" in label:
            assert np.unique(simg).size == simg.size, label
        if " equal" in label and full is not None and full > 1:
            assert np.unique(simg).size == simg.size - full + 1, label
    assert {s.size for _, s, _ in singles} == set(P.SIZES) | {5000}
    assert P.fullest_bin(singles[-1][1], key_bits) >= 4000 and np.count_nonzero(singles[-1][1] == np.uint64((1 << key_bits) - 1)) >= 4000


@pytest.mark.parametrize("key_bits", [64, 32])
def test_deep_inputs_hold_the_tasks_they_name(key_bits):
    img, info, fullest, (cen, tasks) = P.deep_input(key_bits)
    P.assert_embedded(key_bits, img, info, tasks, fullest)
    bits = {sb for _, _, sb, _, _, _ in info}
    assert bits == ({56, 48, 40, 32, 24} if key_bits == 64 else {24, 16})
    # the task of all ones: abandoned (its bin holds everything), and under a 64-bit float key it is full of -0.0
    label, d, sb, tp, _, _ = info[-1]
    S = np.sort(img)
    lo = int(np.searchsorted(S, np.uint64(tp << sb)))
    assert label.startswith("L1 all ones") and P.fullest_bin(S[lo:lo + 5000], sb) == 5000
    ones = np.uint64((tp << sb) | ((1 << sb) - 1))
    assert np.count_nonzero(img == ones) >= 4000
    if key_bits == 64:
        assert P.from_image(np.array([ones]), F64).view(np.float64)[0] == 0.0 and P.from_image(np.array([ones]), F64)[0] >> np.uint64(63) == 1


def test_failing_cases_names_the_case():
    img, info, _, _ = P.level1_input(64, 23)
    exp = np.sort(img)
    assert P.failing_cases(exp, exp, info, 64) == []
    label, d, sb, tp, _, _ = info[17]
    lo = int(np.searchsorted(exp, np.uint64(tp << sb)))
    got = exp.copy()
    got[lo] ^= np.uint64(1)
    assert P.failing_cases(got, exp, info, 64) == [label]


def test_wide_census_refuses_what_the_sort_refuses(gs):
    """hipErrorInvalidValue before the device is touched; num_items == 0 is all zeros."""
    import ctypes as C
    from gpu_sort_amd.msb import _LevelCensus
    lib = gs.lib
    out = (_LevelCensus * 8)()
    po, ws = C.cast(out, C.c_void_p), C.c_void_p(256)
    assert lib.gs_msb_wide_census(None, 10, 8, 0, po, None) == 1
    assert lib.gs_msb_wide_census(ws, 10, 8, 0, None, None) == 1
    assert lib.gs_msb_wide_census(ws, 1 << 32, 8, 0, po, None) == 1
    for kb, vb in ((4, 0), (4, 4), (2, 8), (8, 2), (16, 8)):
        assert lib.gs_msb_wide_census(ws, 10, kb, vb, po, None) == 1, (kb, vb)
    out[3].keys = 5
    assert lib.gs_msb_wide_census(ws, 0, 8, 4, po, None) == 0
    assert all(c.buckets == 0 and c.keys == 0 and c.tasks[0] == 0 and c.overflow == 0 for c in out)
