"""The inputs of tests/test_topk_rows_edges_gpu.py without a device: the plan and the workspace size of every shape against
tests/topk_rows_ref.py, every builder of tests/topk_rows_cases.py held to its intent with the images alone (the k-th image
and its bytes, LESS and TAKE, the wave, ballot row and lane of the cut, the wave or chunk of the winners), the numpy model
of the chunked scheme against the per-row reference on every path-3 case, and, for the compaction and chunk cases, three
deliberately wrong numpy variants that must differ from the reference on those inputs: a case that cannot tell them from
the right answer fails here."""
import ctypes as C

import numpy as np
import pytest

import topk_cases as T
import topk_ref as R
import topk_rows_cases as TC
import topk_rows_ref as RR

CH = TC.CH
U32, I32, F32 = R.U32, R.I32, R.F32


def _plan(gs, rows, cols, k, hv=0):
    out = (C.c_uint32 * 8)(*([9] * 8))
    assert gs.lib.gs_topk_rows_plan(rows, cols, k, hv, out) == 0, (rows, cols, k)
    return list(out)


def shape_is(gs, rows, cols, k, path, levels):
    """The host plan is the reference plan with the stated path and levels, and the size query is the header's formula."""
    p = _plan(gs, rows, cols, k)
    assert p == RR.plan(rows, cols, k) and p[:2] == [path, levels], (rows, cols, k, p)
    for hv in (0, 1):
        assert gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, hv) == RR.temp_bytes(rows, cols, k, hv) > 0, (rows, cols, k, hv)


def model_is_reference(keys, k, kt, desc):
    ek, ec, _ = R.topk(keys, k, kt, desc)
    mk, mc, levels = RR.chunk_model(keys, k, kt, desc)
    assert np.array_equal(mk, ek) and np.array_equal(mc, ec), (keys.size, k, kt, desc)
    assert levels == len(RR.level_sizes(keys.size, k))


# -------------------------------------------------------------------------------------- the wrong variants --
def wrong_model(keys, k, kt, desc, fault, ch=CH):
    """topk_rows_ref.chunk_model with one fault.  "unstable": ties inside a chunk in reverse position order, at every level.
    "by_key": the same from level 1 on only, candidates ranked by key without their position.  "early" / "late", at the
    last level: the cut one element early (the k-th element dropped, the next one in its place) or late (the first element
    of the k-th image's run dropped).  -> (keys, columns)."""
    img = R.image(keys, kt, desc)
    col = np.arange(img.size, dtype=np.uint32)
    level = 0
    while True:
        single = img.size <= ch
        out_i, out_c = [], []
        for lo in range(0, img.size, ch):
            seg = img[lo:lo + ch]
            m = min(k, seg.size)
            if fault == "unstable" or (fault == "by_key" and level > 0):
                order = (seg.size - 1 - np.argsort(seg[::-1], kind="stable"))[:m]
            else:
                order = np.argsort(seg, kind="stable")
                if single and fault == "early" and m < seg.size:
                    order = np.concatenate([order[:m - 1], order[m:m + 1]])
                elif single and fault == "late" and m < seg.size:
                    less = int(np.searchsorted(seg[order], seg[order[m - 1]], side="left"))
                    order = np.concatenate([order[:less], order[less + 1:m + 1]])
                else:
                    order = order[:m]
            out_i.append(seg[order])
            out_c.append(col[lo:lo + ch][order])
        img, col = np.concatenate(out_i), np.concatenate(out_c)
        level += 1
        if single:
            return R.preimage(img, kt, desc), col


def tells_right_from_wrong(keys, k, kt, desc, faults):
    """The reference is the model's answer, and every fault changes the columns."""
    _, ec, _ = R.topk(keys, k, kt, desc)
    model_is_reference(keys, k, kt, desc)
    for fault in faults:
        wk, wc = wrong_model(keys, k, kt, desc, fault)
        assert wc.size == k and not np.array_equal(wc, ec), (fault, keys.size, k)


def test_wrong_model_without_a_fault_is_the_model():
    keys = T.gen("five", 3 * CH + 5, seed=3)
    for k in (1, 100, 1024):
        mk, mc, _ = RR.chunk_model(keys, k, U32, True)
        wk, wc = wrong_model(keys, k, U32, True, None)
        assert np.array_equal(wk, mk) and np.array_equal(wc, mc)


# ---------------------------------------------------------------------------- 1. deep levels and workspace reuse --
def test_deep_shapes_levels_come_from_level_sizes(gs):
    want = {(65536, 1024): 2, (524288, 1024): 3, (524289, 1024): 4, (4194304, 1024): 4, (4194305, 1024): 5, (2097153, 512): 4,
            (262145, 256): 3, (262145, 257): 3}
    assert {(c, k): lv for _, c, k, lv in TC.DEEP_SHAPES} == want
    for rows, cols, k, levels in TC.DEEP_SHAPES + TC.DEEP_EQUAL + [TC.DEEP_ARENA]:
        ns = RR.level_sizes(cols, k)
        assert len(ns) == levels and ns[-1] <= CH < ns[-2]
        shape_is(gs, rows, cols, k, 3, levels)
        # the areas: level i writes n[i + 1] per row into area i & 1, sized for n[1] and n[2]
        for i in range(2, levels - 1):
            assert ns[i + 1] <= ns[1 + (i & 1)]
    assert RR.level_sizes(65536, 1024) == [65536, 8192]                      # level 1 reads exactly one full chunk
    assert RR.level_sizes(524288, 1024)[1:] == [65536, 8192] and RR.level_sizes(524289, 1024)[1:] == [65537, 8193, 1025]     # a tail of one gives one
    assert RR.level_sizes(4194304, 1024)[1:] == [524288, 65536, 8192] and len(RR.level_sizes(4194305, 1024)) == 5
    assert len(RR.level_sizes(2097152, 512)) == 3 and len(RR.level_sizes(262144, 256)) == 2
    assert {lv for _, _, _, lv in TC.DEEP_SHAPES} == {2, 3, 4, 5}
    assert len(RR.level_sizes(33554432, 1024)) == 5 and len(RR.level_sizes(33554433, 1024)) == 6    # six levels: out of reach


def test_deep_runs_see_every_distribution_type_and_direction():
    seen = set()
    for shape in TC.DEEP_SHAPES:
        runs = TC.deep_runs(shape)
        assert len(runs) == (1 if shape[1] in TC.DEEP_SINGLE else 4)
        for kt, desc, kinds in runs:
            assert "special" not in kinds or kt == F32
            seen |= {(kt, desc, kind) for kind in TC.deep_row_kinds(shape, (kt, desc, kinds))}
    assert {k for _, _, k in seen} == set(TC.DEEP_KINDS) and {(kt, d) for kt, d, _ in seen} == set(TC.TYPES_DIRS)
    deep = [s for s in TC.DEEP_SHAPES if s[3] >= 4]
    assert {kind for s in deep for run in TC.deep_runs(s) for kind in TC.deep_row_kinds(s, run)} == set(TC.DEEP_KINDS)


@pytest.mark.parametrize("shape", TC.DEEP_SHAPES)
def test_deep_chunk_model_is_the_reference(shape):
    """Row 0 of the shape's last run (an f32 run: NaNs and -0.0 travel through the candidate rows); the 16 MiB rows once each."""
    rows, cols, k, levels = shape
    kt, desc, kinds = TC.deep_runs(shape)[-1]
    mat = TC.deep_matrix(shape, (kt, desc, kinds))
    assert mat.shape == (rows, cols)
    model_is_reference(mat[0], k, kt, desc)
    if "special" in TC.deep_row_kinds(shape, (kt, desc, kinds)):
        assert kt == F32 and np.isnan(mat.view(np.float32)).any() and (mat == 0x80000000).any()      # NaNs and -0.0


def test_deep_equal_rows_give_the_first_columns():
    for rows, cols, k, levels in TC.DEEP_EQUAL:
        for kt, desc in ((I32, False), (F32, True)):
            mat = TC.equal_matrix(rows, cols, kt, desc)
            assert mat.shape == (rows, cols) and np.unique(mat).size == 1
            ek, ec = RR.rows_topk(mat[:1], cols, k, kt, desc)
            assert np.array_equal(ec[0], np.arange(k, dtype=np.uint32))
        model_is_reference(mat[0], k, kt, desc)


# ------------------------------------------------------------------------------ 2. finishing-wave classes in k --
def test_class_ks_sit_on_every_class_edge(gs):
    assert [TC.k_class(k) for k in TC.CLASS_KS] == [1, 1, 4, 4, 4, 8, 8, 8, 16, 16, 16]
    for wkpt in (1, 4, 8):                                                      # one short, exactly full, the first k of the next class
        assert {wkpt * 64 - 1, wkpt * 64, wkpt * 64 + 1} <= set(TC.CLASS_KS) and TC.k_class(wkpt * 64 + 1) > TC.k_class(wkpt * 64) == wkpt
    assert {1023, 1024} <= set(TC.CLASS_KS) and max(TC.CLASS_KS) == RR.MAX_K == 16 * 64
    for rows, cols, path, levels in TC.CLASS_SHAPES:
        for k in TC.CLASS_KS:
            shape_is(gs, rows, cols, k, path, levels)
    # a full chunk: keff = k, so k = 64 * WKPT leaves no pad in the finishing wave
    assert TC.CLASS_SHAPES[0][1] == CH and TC.CLASS_SHAPES[1][1] == 2 * CH + 1


@pytest.mark.parametrize("rows,cols,path,levels", TC.CLASS_SHAPES)
def test_class_rows_of_five_cut_inside_a_long_tie_run(rows, cols, path, levels):
    for kt, desc in ((U32, False), (F32, True)):
        if path == 3:
            for k in TC.CLASS_KS:
                model_is_reference(TC.dist_matrix(rows, cols, kt, 1, ["uniform"])[0], k, kt, desc)
        mat = TC.dist_matrix(rows, cols, kt, 1, ["five"])
        for r in range(rows):
            ref = R.Ref(mat[r], kt, desc)
            for k in TC.CLASS_KS:
                kth, less, take, _ = ref.topk(k)[2]
                assert take >= 1 and int(np.count_nonzero(ref.img == kth)) > take + 100, (k, less, take)
                if path == 3:
                    model_is_reference(mat[r], k, kt, desc)


# --------------------------------------------------------------------------- 3. row lengths of the block kernel --
def test_length_cols_decide_the_empty_waves_and_the_last_ballot_row(gs):
    last = [TC.where(cols - 1) for cols in TC.LENGTH_COLS]
    assert {w for w, _, _ in last} == {1, 2, 3, 4, 6, 7}                      # the last wave with an element
    assert {lane for _, _, lane in last} >= {0, 62, 63} and {row for _, row, _ in last} >= {0, 1, 15}
    for m in (2, 4, 7):
        assert {1024 * m - 1, 1024 * m, 1024 * m + 1} <= set(TC.LENGTH_COLS)
    assert {1025, 8 * 1024 - 1, 8 * 1024} <= set(TC.LENGTH_COLS)                # (1024 and below, and CH + 1, are other paths)
    assert {1088 - 1, 1088, 1088 + 1} <= set(TC.LENGTH_COLS) and 1088 % 64 == 0 and 1088 % 1024 != 0   # a ballot row's edge inside a wave
    for cols in TC.LENGTH_COLS:
        assert TC.length_ks(cols) == [1, 64, 1024]
        for k in TC.length_ks(cols):
            shape_is(gs, TC.LENGTH_ROWS, cols, k, 2, 1)


def test_tail_lengths_of_path_three(gs):
    for k in TC.TAIL_KS:
        ts = TC.tail_lengths(k)
        assert ts == [1, 63, 64, 65, k - 1, k, k + 1]
        for t in ts:
            shape_is(gs, 2, CH + t, k, 3, 2)
            assert RR.level_sizes(CH + t, k) == [CH + t, k + min(k, t)]
            mat = TC.dist_matrix(1, CH + t, F32, t, ["special"])
            model_is_reference(mat[0], k, F32, bool(t % 2))


# ------------------------------------------------------------------------------ 4. select-digit edges and pads --
def test_digit_base_row():
    runs = TC.digit_runs()
    assert [i for i, _ in runs] == T.IMAGES20 and sum(ln for _, ln in runs) == TC.DIGIT_BASE == 780
    assert {ln for _, ln in runs} == {1, 2, 63, 64, 65} and [ln for _, ln in runs[:6]] == [1, 2, 63, 64, 65, 1]
    assert TC.cols_class(TC.DIGIT_BASE) == 16


@pytest.mark.parametrize("variant,cols", TC.DIGIT_VARIANTS)
def test_digit_variants_meet_every_digit_edge(gs, variant, cols):
    runs = TC.digit_runs()
    path, levels = (1, 1) if cols <= 1024 else (2, 1) if cols <= CH else (3, 2)
    lim = min(cols, 1024)
    for kt, desc in TC.TYPES_DIRS:
        mat = TC.digit_matrix(variant, cols, kt, desc)
        assert mat.shape == (TC.DIGIT_ROWS, cols) and not np.array_equal(mat[0], mat[1])
        refs = [R.Ref(mat[r], kt, desc) for r in range(TC.DIGIT_ROWS)]
        assert np.array_equal(refs[0].sorted_img, refs[1].sorted_img)          # the same images in another shuffle
        ref = refs[0]
        assert np.array_equal(np.unique(ref.img), np.array(T.IMAGES20, np.uint32))
        counts = dict(zip(*[x.tolist() for x in np.unique(ref.img, return_counts=True)]))
        filled = {"a": None, "b": TC.PAD, "c": 0}[variant]                     # the image that fills the row up to cols
        for img, ln in runs:
            assert counts[img] == ln + (cols - TC.DIGIT_BASE if img == filled else 0)
        ks = TC.digit_ks(variant, cols, ref)
        assert all(1 <= k <= lim and m in TC.MODES for k, m in ks) and {m for _, m in ks} == set(TC.MODES)
        assert {1, lim} <= {k for k, _ in ks}
        kths = set()
        for k, mode in ks:
            shape_is(gs, TC.DIGIT_ROWS, cols, k, path, levels)
            kth, less, take, _ = ref.topk(k)[2]
            kths.add(kth)
            if variant == "c":
                assert (kth, less, take) == (0, 0, k) and counts[0] > 1024
            if path == 3 and (kt, desc) in ((U32, False), (F32, True)):
                model_is_reference(mat[0], k, kt, desc)
        if variant != "c":
            # k on the last element of every run, the first of the next, and one before the last
            C_ = 0
            for img, _ in runs:
                ln = counts[img]
                start, C_ = C_, C_ + ln
                have = {k: m for k, m in ks}
                if C_ <= lim:
                    assert have[C_] == TC.ARGS and ref.topk(C_)[2][:3] == [img, start, ln]
                if C_ + 1 <= lim:
                    assert C_ + 1 in have and ref.topk(C_ + 1)[2][1:3] == [C_, 1]
                if ln > 1 and C_ - 1 <= lim:
                    assert C_ - 1 in have and ref.topk(C_ - 1)[2][:3] == [img, start, ln - 1]
            assert kths == set(T.IMAGES20)
            for shift in (0, 8, 16, 24):                                       # a k-th image with 0x00 and with 0xFF in every round
                assert {0x00, 0xFF} <= {(kth >> shift) & 255 for kth in kths}


def test_pad_rows_hold_the_words_whose_image_is_a_pads(gs):
    words = {(U32, False): 0xFFFFFFFF, (U32, True): 0, (I32, False): 0x7FFFFFFF, (F32, False): 0x7FFFFFFF, (F32, True): 0xFFFFFFFF,
             (I32, True): 0x80000000}
    assert np.isnan(np.array([0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)).all()
    assert any(c % 64 for c in TC.PAD_COLS) and max(TC.PAD_COLS) <= RR.WAVE_COLS
    assert {TC.cols_class(c) for c in TC.PAD_COLS} == {1, 4, 8, 16}
    for cols in TC.PAD_COLS:
        for (kt, desc), word in words.items():
            mat = TC.pad_matrix(cols, kt, desc)
            assert mat.shape == (TC.PAD_ROWS, cols) and (mat == word).all() and (R.image(mat, kt, desc) == TC.PAD).all()
            for k in TC.pad_ks(cols):
                shape_is(gs, TC.PAD_ROWS, cols, k, 1, 1)
                assert np.array_equal(RR.rows_topk(mat, cols, k, kt, desc)[1], np.tile(np.arange(k, dtype=np.uint32), (TC.PAD_ROWS, 1)))
        assert cols in TC.pad_ks(cols)


# ---------------------------------------------------------------------------------------- 5. compaction edges --
CUT_AT = {1: (-1, 15, 34), 29: (-1, 15, 62), 30: (-1, 15, 63), 31: (0, 0, 0), 94: (0, 0, 63), 95: (0, 1, 0)}   # t -> (wave - w, row, lane)


@pytest.mark.parametrize("chunks,path,levels", TC.COMPACT_FORMS)
def test_cut_rows_put_the_cut_around_every_wave_boundary(gs, chunks, path, levels):
    lo = (chunks - 1) * CH
    assert sorted(CUT_AT) == TC.CUT_TS and TC.CUT_WAVES == [1, 2, 3, 4, 5, 6, 7]
    for kt, desc in TC.TYPES_DIRS:
        mat = TC.cut_matrix(chunks, kt, desc)
        assert mat.shape == (7, chunks * CH)
        for w, row in zip(TC.CUT_WAVES, mat):
            ref = R.Ref(row, kt, desc)
            assert (ref.img[:lo] > TC.CUT_T).all()                             # chunk 0 of the two-chunk form: only losers
            img = ref.img[lo:]
            start = 1024 * w - TC.CUT_LEAD
            below = np.flatnonzero(img < TC.CUT_T)
            assert below.size == TC.CUT_BELOW and [TC.where(j)[0] for j in below] == [0, 0, 7, 7, 7]
            assert np.count_nonzero(img[:start] == TC.CUT_T) == 0 and np.count_nonzero(img[:start] < TC.CUT_T) == 2
            assert (img[start:] <= TC.CUT_T).all() and np.unique(img[below]).size == TC.CUT_BELOW
            assert (below[2:] >= 7 * 1024 + 128).all() and img[7 * 1024] == TC.CUT_T        # behind elements equal to T, in wave 7
            for t in TC.CUT_TS:
                k = TC.CUT_BELOW + t
                shape_is(gs, 7, chunks * CH, k, path, levels)
                ek, ec, (kth, less, take, _) = ref.topk(k)
                assert (kth, less, take) == (TC.CUT_T, TC.CUT_BELOW, t)
                cut = int(ec[-1]) - lo                                         # the last element of the run that is taken
                dw, brow, lane = CUT_AT[t]
                assert cut == start + t - 1 and TC.where(cut) == (w + dw, brow, lane)
                assert np.count_nonzero(img[cut + 1:] == TC.CUT_T) > 800       # group B behind the cut: dropped
                assert (below[2:] > cut).all()                                 # group A behind it: kept
                if (kt, desc) in ((U32, False), (F32, True)):
                    faults = ["unstable", "early", "late"] + (["by_key"] if chunks > 1 and t > 1 else [])
                    tells_right_from_wrong(row, k, kt, desc, faults)


@pytest.mark.parametrize("chunks,path,levels", TC.COMPACT_FORMS)
def test_one_wave_rows_hold_their_winners_in_one_wave(gs, chunks, path, levels):
    lo = (chunks - 1) * CH
    for kt, desc in TC.TYPES_DIRS:
        mat = TC.one_wave_matrix(chunks, kt, desc)
        assert mat.shape == (8, chunks * CH)
        for w, row in enumerate(mat):
            for k in TC.ONE_WAVE_KS:
                shape_is(gs, 8, chunks * CH, k, path, levels)
                ek, ec, (kth, less, take, _) = R.topk(row, k, kt, desc)
                assert kth < TC.CUT_T and ((ec - lo) // 1024 == w).all() and (ec >= lo).all()
            assert np.count_nonzero(R.image(row, kt, desc) < TC.CUT_T) == 64
            if (kt, desc) == (I32, True):
                tells_right_from_wrong(row, 63, kt, desc, ["early", "late"])


# ------------------------------------------------------------------------------- 6. where the winners lie --
def test_spread_rows(gs):
    cols, k = TC.SPREAD_COLS, TC.SPREAD_K
    assert cols - 3 * CH == 77 >= k
    for kt, desc in TC.TYPES_DIRS:
        mat = TC.one_chunk_matrix(kt, desc)
        assert mat.shape == (4, cols)
        shape_is(gs, 4, cols, k, 3, 2)
        for c, row in enumerate(mat):
            ek, ec, (kth, _, _, _) = R.topk(row, k, kt, desc)
            assert (ec // CH == c).all() and kth < TC.CUT_T and np.count_nonzero(R.image(row, kt, desc) < TC.CUT_T) == k
            model_is_reference(row, k, kt, desc)
        tells_right_from_wrong(mat[3], k, kt, desc, ["early", "late"])
        row = R.preimage(TC.one_per_chunk_images().astype(np.uint32), kt, desc)
        shape_is(gs, 1, cols, 4, 3, 2)
        assert sorted((R.topk(row, 4, kt, desc)[1] // CH).tolist()) == [0, 1, 2, 3]
        model_is_reference(row, 4, kt, desc)


def test_thin_tie_run_over_three_chunks(gs):
    cols = TC.SPREAD_COLS
    img = TC.thin_tie_images()
    at = np.flatnonzero(img == TC.CUT_T)
    assert [int(np.count_nonzero(at // CH == c)) for c in range(4)] == [10, 10, 10, 0]
    assert np.count_nonzero(img < TC.CUT_T) == TC.CUT_BELOW
    want = {10: (0, 5), 15: (0, 10), 16: (1, 11), 25: (1, 20), 26: (2, 21), 35: (2, 30)}       # k -> (chunk of the cut, take)
    assert sorted(want) == TC.SPREAD_TIE_KS
    for kt, desc in TC.TYPES_DIRS:
        row = R.preimage(img.astype(np.uint32), kt, desc)
        for k in TC.SPREAD_TIE_KS:
            shape_is(gs, 1, cols, k, 3, 2)
            ek, ec, (kth, less, take, _) = R.topk(row, k, kt, desc)
            assert (kth, less, take) == (TC.CUT_T, TC.CUT_BELOW, want[k][1]) and int(ec[-1]) // CH == want[k][0]
            assert np.array_equal(ec[less:], at[:take])
            faults = ["by_key"] + (["unstable", "early", "late"] if k < 35 else [])
            tells_right_from_wrong(row, k, kt, desc, faults)


def test_level_one_chunk_boundary_rows(gs):
    cols, k = TC.L1_COLS, TC.L1_K
    assert RR.level_sizes(cols, k) == [cols, TC.L1_N1, 2 * k] and TC.L1_N1 - CH == 2 * k
    for kt, desc in ((U32, True), (I32, False), (F32, True)):
        mat = TC.level1_matrix(kt, desc)
        assert mat.shape == (TC.L1_ROWS, cols)
        for row in mat:
            img = R.image(row, kt, desc)
            assert np.count_nonzero(img[:8 * CH] == TC.CUT_T) == 1000 and np.count_nonzero(img[8 * CH:] == TC.CUT_T) == 50
            assert img.min() == TC.CUT_T
            for kk in TC.L1_KS:
                shape_is(gs, TC.L1_ROWS, cols, kk, 3, 3)
                ek, ec, (kth, less, take, _) = R.topk(row, kk, kt, desc)
                assert (kth, less, take) == (TC.CUT_T, 0, kk)
                assert (ec[:1000] < 8 * CH).all() and (ec[1000:] >= 8 * CH).all()          # 0, 1 and 24 of the second level-1 chunk
                tells_right_from_wrong(row, kk, kt, desc, ["unstable", "by_key", "early", "late"])
            assert (R.topk(row, k, kt, desc)[1][-24:] >= 8 * CH).all()


# --------------------------------------------------------------------------------------------- 7. many rows --
def test_many_rows_shapes(gs):
    for rows, cols, k, path, levels in TC.MANY_ROWS:
        shape_is(gs, rows, cols, k, path, levels)
    rows, cols, k, _, _ = TC.MANY_ROWS[2]
    assert _plan(gs, rows, cols, k)[3] == 3                                     # chunks per row: no power of two
    wide = TC.many_rows_matrix(rows, cols, F32, False)
    for r in (0, 1, 50, 96):
        model_is_reference(wide[r], k, F32, False)
    mat = TC.many_rows_matrix(1000, 7, I32, True)
    img = R.image(mat, I32, True)
    assert mat.shape == (1000, 7) and (img[::3] <= 3).all() and np.unique(img[1::3]).size > 1990
    assert np.unique(mat[1::3], axis=0).shape[0] == mat[1::3].shape[0]          # every row has data of its own
    assert np.array_equal(TC.many_rows_matrix(1000, 7, I32, True), mat)


# ----------------------------------------------------------------------------------------------- 8. campaign --
@pytest.mark.parametrize("seed", TC.CAMPAIGN_SEEDS)
def test_campaign_cases_are_well_formed(gs, seed):
    for i in range(TC.CAMPAIGN_CASES):
        what, mat, cols, kt, desc, kinds, rng = TC.campaign_case(seed, i)
        rows, stride = mat.shape
        assert 1 <= rows <= 9 and stride - cols in TC.CAMPAIGN_GAPS and len(kinds) == rows and mat.dtype == np.uint32, what
        assert cols >= 1 and min(abs(cols - a) for a in TC.CAMPAIGN_ANCHORS) <= 40, what
        assert np.isin(mat[:, cols:], [0, 0xFFFFFFFF]).all() and set(kinds) <= set(TC.CAMPAIGN_DISTS), what
        ks = TC.campaign_ks(R.Ref(mat[0, :cols], kt, desc), cols, rng)
        assert len(ks) == 4 and all(1 <= k <= min(cols, 1024) and m in TC.MODES for k, m in ks), what
        for j, (k, _) in enumerate(ks):
            p = RR.plan(rows, cols, k)
            shape_is(gs, rows, cols, k, p[0], p[1])
            if p[0] == 3:
                model_is_reference(mat[j % rows, :cols], k, kt, desc)
        if i % 10 == 0:
            what2, mat2, _, _, _, _, rng2 = TC.campaign_case(seed, i)           # a case is a function of (seed, index) alone
            assert what2 == what and np.array_equal(mat2, mat) and TC.campaign_ks(R.Ref(mat[0, :cols], kt, desc), cols, rng2) == ks


def test_campaign_reaches_every_path_level_class_type_and_form():
    plans, wave_classes, block_classes, types, forms, dists = set(), set(), set(), set(), set(), set()
    for seed in TC.CAMPAIGN_SEEDS:
        for i in range(TC.CAMPAIGN_CASES):
            what, mat, cols, kt, desc, kinds, rng = TC.campaign_case(seed, i)
            types.add((kt, desc))
            dists |= set(kinds)
            for k, mode in TC.campaign_ks(R.Ref(mat[0, :cols], kt, desc), cols, rng):
                p = RR.plan(mat.shape[0], cols, k)
                plans.add((p[0], p[1]))
                forms.add(mode)
                if p[0] == 1:
                    wave_classes.add(TC.cols_class(cols))
                else:
                    block_classes.add(TC.k_class(k))
    assert plans == {(1, 1), (2, 1), (3, 2), (3, 3)}
    assert wave_classes == {1, 4, 8, 16} and block_classes == {1, 4, 8, 16}
    assert types == set(TC.TYPES_DIRS) and forms == set(TC.MODES) and dists == set(TC.CAMPAIGN_DISTS)


# ---------------------------------------------------------------------------------------------- 9. front end --
def test_front_end_shapes(gs):
    assert TC.FRONT_SHAPES == [(5, 300), (1, 5000), (4, 1)]
    for (rows, cols), path in zip(TC.FRONT_SHAPES, (1, 2, 1)):
        for k in TC.front_ks(cols):
            shape_is(gs, rows, cols, k, path, 1)
        m = TC.distinct_int32(rows, cols, cols)
        assert m.dtype == np.int32 and all(np.unique(r).size == cols for r in m) and (cols == 1 or (m.min() < 0 < m.max()))
