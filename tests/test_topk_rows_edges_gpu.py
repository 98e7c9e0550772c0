"""gs_topk_rows_u32 at the edges of its own decisions, every row bit for bit against the numpy reference (keys, then values or
columns) through the Case of tests/test_topk_rows_gpu.py: a sentinel tail behind the outputs, a workspace of exactly
gs_topk_rows_temp_bytes filled with 0xA5, and the expected (path, levels) asserted through DeviceTopKRows.Plan in every
check.  The inputs come from tests/topk_rows_cases.py; tests/test_topk_rows_edges_cpu.py holds each of them to its intent.

Reached: 4 and 5 select levels, where the candidate rows go back into the first and the second workspace area (with the full
boundaries below them, a level 1 that reads exactly one full chunk, all keys equal, f32 NaNs and -0.0 through every candidate
row, and guard zones around a workspace of exactly the queried size); the finishing wave's classes WKPT = 1, 4, 8, 16 at
k = 64 * WKPT - 1, exactly full and one past, on paths 2 and 3; row lengths of the block kernel at 1024 m - 1 / + 0 / + 1
and off the multiples of 64, and short last chunks around 64 and around k; k-th images with 0x00 and 0xFF in every select
round and the three cuts around every tie run; rows of keys whose image is a pad's; the tie run's cut on each of the seven
wave boundaries and on a ballot-row boundary, with group-B elements behind the cut and group-A elements behind those;
winners in one wave, in one chunk, one per chunk, a tie run thin over three chunks and across a level-1 chunk boundary;
100003, 600 and 97 rows; a seeded campaign over shapes, strides, types, directions, forms and distributions; `topk_rows` on
int32, on a one-row slice and on one column.

Not reached: six levels need cols >= 33,554,433 at k = 1024, whose reference is too slow for a test of seconds;
num_rows * num_cols near 2^32; what a kernel does with its pads beyond what the outputs show (path 1 clamps the column of a
misplaced pad into the row)."""
import numpy as np
import pytest
import torch

import topk_ref as R
import topk_rows_cases as TC
import topk_rows_ref as RR
from guarded import Arena
from test_topk_rows_gpu import Case, values_for

pytestmark = pytest.mark.gpu

U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS, MODES = TC.KEYS, TC.PAIRS, TC.ARGS, TC.MODES
CH = TC.CH


class WideCase(Case):
    """Case for many short rows: the stable order of all rows in one numpy call."""

    def expect(self, rows, k, mode):
        if "all" not in self.order:
            self.order["all"] = np.argsort(R.image(self.mat[:, :self.cols], self.kt, self.desc), axis=1, kind="stable").astype(np.uint32)
        o = self.order["all"][:rows, :k]
        return np.take_along_axis(self.mat[:rows], o, 1), (np.take_along_axis(self.vals[:rows], o, 1) if mode == PAIRS else o)


def first_columns(rows, k):
    return np.tile(np.arange(k, dtype=np.uint32), (rows, 1))


# ---------------------------------------------------------------------------- 1. deep levels and workspace reuse --
@pytest.mark.parametrize("shape", TC.DEEP_SHAPES)
def test_deep_levels_alternate_the_workspace_areas(gs, cuda, shape):
    """Up to five levels: level i writes its candidate rows into area i & 1, so levels 2 and 3 go back into the areas sized for
    n[1] and n[2].  Uniform keys, five values (ties through every level) and the f32 specials; all three forms."""
    rows, cols, k, levels = shape
    for run in TC.deep_runs(shape):
        kt, desc, _ = run
        c = Case(gs, cuda, TC.deep_matrix(shape, run), cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


def test_three_levels_with_a_finishing_wave_of_one_per_lane(gs, cuda):
    """k = 64: the middle level (carried columns in, a candidate row out) in the one class DEEP_SHAPES leaves out -- its three
    and more levels are at k = 256 and above."""
    rows, cols, k, levels = RR.MIDDLE_SHAPES[0]
    assert k == 64 and not any(kk <= 64 for _, _, kk, _ in TC.DEEP_SHAPES)
    for kt, desc, kinds in ((F32, True, ["special"]), (I32, False, ["five"])):
        c = Case(gs, cuda, TC.dist_matrix(rows, cols, kt, 11, kinds), cols, kt, desc)
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


@pytest.mark.parametrize("rows,cols,k,levels", TC.DEEP_EQUAL)
def test_deep_all_keys_equal_gives_the_first_columns(gs, cuda, rows, cols, k, levels):
    for kt, desc in ((I32, False), (F32, True)):
        c = Case(gs, cuda, TC.equal_matrix(rows, cols, kt, desc), cols, kt, desc)
        assert np.array_equal(c.expect(rows, k, ARGS)[1], first_columns(rows, k))
        for mode in MODES:
            c.check(rows, k, mode, plan=(3, levels))


def test_four_levels_stay_inside_a_guarded_workspace_of_the_queried_size(gs, cuda):
    """The pairs form at 4 levels with guard zones around every array; the workspace is exactly the queried size, at an odd
    offset, filled at random: the third candidate write stays inside the area it reuses."""
    rows, cols, k, levels = TC.DEEP_ARENA
    kt, desc = F32, True
    mat = TC.dist_matrix(rows, cols, kt, 3, ["five", "special"])
    vals = values_for(mat.shape, seed=9)
    nb = gs.lib.gs_topk_rows_temp_bytes(rows, cols, k, 1)
    assert nb == RR.temp_bytes(rows, cols, k, 1) and gs.DeviceTopKRows.Plan(rows, cols, k, 1)[:2] == [3, levels]
    a = Arena(cuda, seed=4)
    a.add("keys_in", 4 * rows * cols, offset=4, data=mat, const=True)
    a.add("vals_in", 4 * rows * cols, offset=12, data=vals, const=True)
    a.add("keys_out", 4 * rows * k, offset=8, fill="random")
    a.add("vals_out", 4 * rows * k, offset=20, fill="random")
    a.add("temp", nb, offset=7, fill="random")
    a.build()
    rc = gs.lib.gs_topk_rows_u32(a.ptr("temp"), nb, a.ptr("keys_in"), a.ptr("vals_in"), a.ptr("keys_out"), a.ptr("vals_out"), rows, cols,
                                 cols, k, int(desc), kt, None)
    assert rc == 0
    a.check()
    ek, ev = RR.rows_topk(mat, cols, k, kt, desc, vals)
    assert np.array_equal(a.read("keys_out", np.uint32).reshape(rows, k), ek)
    assert np.array_equal(a.read("vals_out", np.uint32).reshape(rows, k), ev)


# ------------------------------------------------------------------------------ 2. finishing-wave classes in k --
@pytest.mark.parametrize("rows,cols,path,levels", TC.CLASS_SHAPES)
@pytest.mark.parametrize("kind", TC.CLASS_KINDS)
def test_finishing_wave_classes_at_and_past_capacity(gs, cuda, rows, cols, path, levels, kind):
    """k = 64 * WKPT - 1, 64 * WKPT (no pad in the finishing wave) and one more (the next class), on full chunks; rows of five
    values put the cut inside a long tie run, where a dropped winner shows as a wrong column."""
    cases = {}
    for j, k in enumerate(TC.CLASS_KS):
        kt, desc, _ = TC.rotate(j)
        if (kt, desc) not in cases:
            cases[(kt, desc)] = Case(gs, cuda, TC.dist_matrix(rows, cols, kt, 1, [kind]), cols, kt, desc)
        for mode in MODES:
            cases[(kt, desc)].check(rows, k, mode, plan=(path, levels))


# --------------------------------------------------------------------------- 3. row lengths of the block kernel --
@pytest.mark.parametrize("cols", TC.LENGTH_COLS)
def test_row_lengths_of_one_workgroup_per_row(gs, cuda, cols):
    """Which waves are empty and which lanes vote in the last ballot row."""
    ci = TC.LENGTH_COLS.index(cols)
    for j, k in enumerate(TC.length_ks(cols)):
        kt, desc, mode = TC.rotate(ci + 2 * j)
        c = Case(gs, cuda, TC.dist_matrix(TC.LENGTH_ROWS, cols, kt, 30 + ci, TC.LENGTH_KINDS), cols, kt, desc)
        for m in (mode, MODES[(MODES.index(mode) + 1) % 3]):
            c.check(TC.LENGTH_ROWS, k, m, plan=(2, 1))


@pytest.mark.parametrize("k", TC.TAIL_KS)
def test_short_last_chunks_of_the_chunked_path(gs, cuda, k):
    for i, t in enumerate(TC.tail_lengths(k)):
        kt, desc, _ = TC.rotate(i + k)
        c = Case(gs, cuda, TC.dist_matrix(2, CH + t, kt, 50 + i, TC.LENGTH_KINDS), CH + t, kt, desc)
        for mode in MODES:
            c.check(2, k, mode, plan=(3, 2))


# ------------------------------------------------------------------------------ 4. select-digit edges and pads --
@pytest.mark.parametrize("variant,cols", TC.DIGIT_VARIANTS)
@pytest.mark.parametrize("kt", TC.KEY_TYPES)
def test_extreme_digits_and_the_cuts_around_every_tie_run(gs, cuda, variant, cols, kt):
    """The twenty images in runs of 1, 2, 63, 64 and 65: every pick round meets digit 0 and digit 255; k is the last of each
    run, the first of the next, and one before.  b: thousands of real keys with a pad's image behind them.  c: a first run
    longer than 1024, which every k cuts."""
    plan = (1, 1) if cols <= RR.WAVE_COLS else (2, 1) if cols <= CH else (3, 2)
    for desc in (False, True):
        c = Case(gs, cuda, TC.digit_matrix(variant, cols, kt, desc), cols, kt, desc)
        for k, mode in TC.digit_ks(variant, cols, R.Ref(c.mat[0], kt, desc)):
            c.check(TC.DIGIT_ROWS, k, mode, plan=plan)


@pytest.mark.parametrize("cols", TC.PAD_COLS)
def test_rows_of_keys_with_a_pads_image(gs, cuda, cols):
    """u32 max ascending, 0 descending, i32 max and min, the f32 NaNs 0x7FFFFFFF ascending and 0xFFFFFFFF descending: real keys
    that only position keeps in front of the pads.  The columns are 0 .. k - 1 and the values those columns' values."""
    for kt, desc in TC.TYPES_DIRS:
        c = Case(gs, cuda, TC.pad_matrix(cols, kt, desc), cols, kt, desc)
        for k in TC.pad_ks(cols):
            ek, ev = c.expect(TC.PAD_ROWS, k, ARGS)
            assert np.array_equal(ev, first_columns(TC.PAD_ROWS, k)) and (R.image(ek, kt, desc) == TC.PAD).all()
            assert np.array_equal(c.expect(TC.PAD_ROWS, k, PAIRS)[1], c.vals[:, :k])
            for mode in (ARGS, PAIRS):
                c.check(TC.PAD_ROWS, k, mode, plan=(1, 1))


# ---------------------------------------------------------------------------------------- 5. compaction edges --
@pytest.mark.parametrize("chunks,path,levels", TC.COMPACT_FORMS)
def test_tie_run_cut_on_every_wave_boundary(gs, cuda, chunks, path, levels):
    """Seven rows, the run of row w starting 30 elements before wave w: the cut falls just before, on and after the wave
    boundary and on a ballot-row boundary; the rest of the run is dropped, three smaller keys behind it in wave 7 are kept."""
    for kt, desc in TC.TYPES_DIRS:
        c = Case(gs, cuda, TC.cut_matrix(chunks, kt, desc), chunks * CH, kt, desc)
        for t in TC.CUT_TS:
            for mode in MODES:
                c.check(len(TC.CUT_WAVES), TC.CUT_BELOW + t, mode, plan=(path, levels))


@pytest.mark.parametrize("chunks,path,levels", TC.COMPACT_FORMS)
def test_winners_all_in_one_wave(gs, cuda, chunks, path, levels):
    for kt, desc in TC.TYPES_DIRS:
        c = Case(gs, cuda, TC.one_wave_matrix(chunks, kt, desc), chunks * CH, kt, desc)
        for k in TC.ONE_WAVE_KS:
            for mode in MODES:
                c.check(8, k, mode, plan=(path, levels))


# ------------------------------------------------------------------------------- 6. where the winners lie --
def test_winners_in_one_chunk_and_one_per_chunk(gs, cuda):
    cols = TC.SPREAD_COLS
    for kt, desc in TC.TYPES_DIRS:
        c = Case(gs, cuda, TC.one_chunk_matrix(kt, desc), cols, kt, desc)
        for mode in MODES:
            c.check(4, TC.SPREAD_K, mode, plan=(3, 2))
        row = R.preimage(TC.one_per_chunk_images().astype(np.uint32), kt, desc)
        c = Case(gs, cuda, row.reshape(1, cols), cols, kt, desc)
        for mode in MODES:
            c.check(1, 4, mode, plan=(3, 2))


def test_tie_run_thin_over_three_chunks(gs, cuda):
    cols = TC.SPREAD_COLS
    for kt, desc in TC.TYPES_DIRS:
        row = R.preimage(TC.thin_tie_images().astype(np.uint32), kt, desc)
        c = Case(gs, cuda, row.reshape(1, cols), cols, kt, desc)
        for k in TC.SPREAD_TIE_KS:
            for mode in MODES:
                c.check(1, k, mode, plan=(3, 2))


def test_tie_run_across_a_level_one_chunk_boundary(gs, cuda):
    """1000 ties in the first level-1 chunk and 50 in the second: at k = 1024 the last 24 columns come from the second, ordered
    by candidate position with carried columns."""
    for kt, desc in TC.TYPES_DIRS:
        c = Case(gs, cuda, TC.level1_matrix(kt, desc), TC.L1_COLS, kt, desc)
        assert (c.expect(TC.L1_ROWS, TC.L1_K, ARGS)[1][:, -24:] >= 8 * CH).all()
        for k in TC.L1_KS:
            for mode in MODES:
                c.check(TC.L1_ROWS, k, mode, plan=(3, 3))


# --------------------------------------------------------------------------------------------- 7. many rows --
@pytest.mark.parametrize("rows,cols,k,path,levels", TC.MANY_ROWS)
def test_many_rows(gs, cuda, rows, cols, k, path, levels):
    """A ragged last workgroup of path 1 at 100003 rows; the block map r = block / chunks with three chunks and 97 rows."""
    i = TC.MANY_ROWS.index((rows, cols, k, path, levels))
    for j, mode in enumerate((KEYS, ARGS)):
        kt, desc, _ = TC.rotate(2 * i + j + 1)
        c = WideCase(gs, cuda, TC.many_rows_matrix(rows, cols, kt, desc), cols, kt, desc)
        c.check(rows, k, mode, plan=(path, levels))


# ----------------------------------------------------------------------------------------------- 8. campaign --
@pytest.mark.parametrize("seed", TC.CAMPAIGN_SEEDS)
@pytest.mark.parametrize("part", range(TC.CAMPAIGN_PARTS))
def test_seeded_campaign(gs, cuda, seed, part):
    """Column counts around every path and class edge, 1 to 9 rows at strides with a gap of extremes, every distribution and
    the digit-edge row, cuts around tie runs and random k; a failure prints the case
    (topk_rows_cases.campaign_case(seed, index) rebuilds it).  Nothing is skipped."""
    for index in range(part, TC.CAMPAIGN_CASES, TC.CAMPAIGN_PARTS):
        what, mat, cols, kt, desc, _, rng = TC.campaign_case(seed, index)
        rows = mat.shape[0]
        c = Case(gs, cuda, mat, cols, kt, desc)
        for k, mode in TC.campaign_ks(R.Ref(mat[0, :cols], kt, desc), cols, rng):
            try:
                c.check(rows, k, mode, plan=RR.plan(rows, cols, k)[:2])
            except AssertionError as e:
                raise AssertionError("%s k=%d %s: %s" % (what, k, mode, e)) from e


# ---------------------------------------------------------------------------------------------- 9. front end --
@pytest.mark.parametrize("rows,cols", TC.FRONT_SHAPES)
def test_topk_rows_on_int32_slices_and_one_column(gs, cuda, rows, cols):
    """int32 keys of both signs against torch.topk: contiguous, and as a slice of a wider matrix (for one row, [1:2, 3:3 + cols],
    whose stride is taken as cols)."""
    wide = torch.from_numpy(TC.distinct_int32(rows + 2, cols + 8, seed=cols)).to(cuda)
    view = wide[1:1 + rows, 3:3 + cols]
    assert view.shape == (rows, cols) and view.stride(0) == cols + 8 and view.data_ptr() != wide.data_ptr()
    for x in (view.clone(memory_format=torch.contiguous_format), view):
        for k in TC.front_ks(cols):
            for largest in (False, True):
                want = torch.topk(x, k, dim=1, largest=largest, sorted=True)
                ko, io = gs.topk_rows(x, k, largest=largest, indices=True)
                assert tuple(ko.shape) == (rows, k) and ko.dtype == torch.int32 and io.dtype == torch.int32
                assert torch.equal(ko, want.values) and torch.equal(io.long(), want.indices), (rows, cols, k, largest)
