"""The top-k campaign on the device (tests/topk_campaign.py): all eleven entry points through the C ABI, 96 cases per entry
point and seed.  Per case: inputs, pre-filled outputs and a workspace of exactly the queried size (0xA5) in one guarded Arena
at the case's offsets, one call, check() against reference() -- keys, values, counts, the pre-fill behind kept, the inputs
and every guard band, bit for bit -- then the status call of the shape held to what the reference derives without modelling
a kernel (the k-th image, less, take, the six list counts, nothing dropped), then at most two of the header's equalities on
the same device data, and every eighth case the same call again on the same workspace.  A failure names
(entry point, seed, index), which rebuilds the case, and the first difference."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_campaign as T
from guarded import Arena

pytestmark = pytest.mark.gpu

PARTS = 4                   # items per (entry point, seed): chosen so that the slowest item stays under 10 s
PER_PART = T.CASES // PARTS
assert PER_PART * PARTS == T.CASES


# ---------------------------------------------------------------------------------------------------- the calls --
def dims_of(c, arena=None):
    if c.shape == T.FLAT:
        return {"n": c.n}
    if c.shape == T.SEG:
        return {"n": c.n, "S": c.S, "begin": arena.ptr("begin") if arena else None, "end": arena.ptr("end") if arena else None}
    return {"rows": c.rows, "cols": c.cols, "stride": c.stride}


def shape_args(family, d):
    shape = T.FAMILIES[family][0]
    if shape == T.FLAT:
        return (d["n"],)
    if shape == T.SEG:
        return (d["n"], d["S"])
    return (d["rows"], d["cols"])


def temp_query(gs, family, d, k, hv):
    nb = getattr(gs.lib, T.FAMILIES[family][2])(*shape_args(family, d), k, hv)
    assert nb > 0, (family, d, k, hv)
    return nb


def invoke(gs, family, temp, nb, kin, vin, kout, vout, counts, d, k, desc, kt):
    shape = T.FAMILIES[family][0]
    fn = getattr(gs.lib, family)
    if shape == T.FLAT:
        return fn(temp, nb, kin, vin, kout, vout, d["n"], k, int(desc), kt, None)
    if shape == T.SEG:
        return fn(temp, nb, kin, vin, kout, vout, counts, d["n"], d["S"], d["begin"], d["end"], k, int(desc), kt, None)
    return fn(temp, nb, kin, vin, kout, vout, d["rows"], d["cols"], d["stride"], k, int(desc), kt, None)


def status(gs, family, temp, d, k, hv, row=None):
    out = (C.c_uint32 * 8)()
    fn = getattr(gs.lib, T.FAMILIES[family][3])
    args = shape_args(family, d) + (k, hv) + (() if row is None else (row,))
    assert fn(temp, *args, out, None) == 0
    return list(out)


def plain(gs, cuda, family, kt, desc, form, k, kin, vin, d, S):
    """One call of `family` with outputs and workspace of its own: (keys [S, k], values [S, k] or None, counts or None).
    The slots a segmented call leaves unwritten read as zero."""
    width = T.FAMILIES[family][1]
    hv = int(form != T.KEYS)
    nb = temp_query(gs, family, d, k, hv)
    temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=cuda)
    ko = torch.zeros(S * k * width // 8, dtype=torch.uint8, device=cuda)
    vo = torch.zeros(S * k * 4, dtype=torch.uint8, device=cuda) if hv else None
    co = torch.zeros(S * 4, dtype=torch.uint8, device=cuda) if T.FAMILIES[family][0] == T.SEG else None
    rc = invoke(gs, family, temp.data_ptr(), nb, kin, vin if form == T.PAIRS else None, ko.data_ptr(),
                vo.data_ptr() if hv else None, co.data_ptr() if co is not None else None, d, k, desc, kt)
    assert rc == 0, (family, rc)
    torch.cuda.synchronize()
    return (ko.cpu().numpy().view(T.UINT[width]).reshape(S, k), vo.cpu().numpy().view(np.uint32).reshape(S, k) if hv else None,
            co.cpu().numpy().view(np.uint32) if co is not None else None)


def upload(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(cuda)


# ------------------------------------------------------------------------------------------------- one case --
class Run:
    """A case on the device: the arena, the one call, and the outputs as check() reads them."""

    def __init__(self, gs, cuda, c):
        self.gs, self.cuda, self.c = gs, cuda, c
        self.r = T.reference(c)
        self.hv = int(c.form != T.KEYS)
        self.S = self.r.counts.size
        self.nb = temp_query(gs, c.family, dims_of(c), c.k, self.hv)
        self.arena = Arena(cuda)
        for name, nbytes, off, data, _ in T.layout(c, self.nb):
            self.arena.add(name, nbytes, offset=off, data=data)      # check() compares the inputs itself
        self.arena.build()
        self.d = dims_of(c, self.arena)

    def ptr(self, name):
        return self.arena.ptr(name) if name in self.arena.slots else None

    def call(self):
        c = self.c
        rc = invoke(self.gs, c.family, self.ptr("temp"), self.nb, self.ptr("keys_in"), self.ptr("vals_in"), self.ptr("keys_out"),
                    self.ptr("vals_out"), self.ptr("counts"), self.d, c.k, c.descending, c.key_type)
        assert rc == 0, (c.describe(), "returned", rc)
        torch.cuda.synchronize()

    def snapshot(self):
        return {"mem": self.arena.mem.cpu().numpy(), "pattern": self.arena.pattern.cpu().numpy(), "slots": self.arena.slots}

    def outputs(self, snap):
        def buf(name, t):
            start, nbytes = snap["slots"][name][:2]
            return snap["mem"][start:start + nbytes].view(t).reshape(self.S, -1)
        return (buf("keys_out", T.UINT[self.c.width]), buf("vals_out", np.uint32) if self.hv else None,
                buf("counts", np.uint32).reshape(-1) if self.c.shape == T.SEG else None)


def sampled(c, index_space, salt):
    """First, last and one random element of index_space."""
    if len(index_space) == 0:
        return []
    rng = np.random.default_rng([c.seed, c.index, salt])
    return sorted({int(index_space[0]), int(index_space[-1]), int(index_space[int(rng.integers(0, len(index_space)))])})


def check_status(run):
    """Only what the reference derives without modelling a kernel."""
    c, r, gs = run.c, run.r, run.gs
    temp = run.ptr("temp")
    if c.shape == T.FLAT:
        st = status(gs, c.family, temp, run.d, c.k, run.hv)
        kth, less, take = int(r.kth[0]), int(r.less[0]), int(r.take[0])
        want = [kth & 0xFFFFFFFF, kth >> 32, less, take] if c.width == 64 else [kth, less, take]
        assert st[1:1 + len(want)] == want, (c.describe(), "status", st, "expected k-th image, less, take", want)
    elif c.shape == T.ANYK:
        for row in sampled(c, range(c.rows), 11):
            st = status(gs, c.family, temp, run.d, c.k, run.hv, row)
            want = [int(r.kth[row]), int(r.less[row]), int(r.take[row])]
            assert st[1:4] == want, (c.describe(), "status of row", row, st, "expected k-th image, less, take", want)
    elif c.shape == T.SEG:
        st = status(gs, c.family, temp, run.d, c.k, run.hv)
        lists, _ = T.seg_lists(c)
        assert st[:6] == lists and st[7] == 0, (c.describe(), "status", st, "expected lists", lists, "and nothing dropped")


# ------------------------------------------------------------------------------------------ the header's equalities --
def _same(c, what, got, want, mask=None):
    bad = (got != want) if mask is None else ((got != want) & mask)
    if bad.any():
        s, j = divmod(int(np.flatnonzero(bad.reshape(-1))[0]), bad.shape[-1])
        pytest.fail("%s: %s differs at row or segment %d, slot %d: 0x%x against 0x%x of the call under test"
                    % (c.describe(), what, s, j, got.reshape(bad.shape[0], -1)[s, j], want.reshape(bad.shape[0], -1)[s, j]))


def eq_sub_flat(run, gk, gv):
    """Row r, or clamped segment s with k = kept, equals the flat call of the same width on that sub-array."""
    c, r = run.c, run.r
    flat = T.FAMILY_OF[(T.FLAT, c.width)]
    base, length = T.subarrays(c)
    for s in sampled(c, np.flatnonzero(r.counts), 12):
        kept, isz = int(r.counts[s]), c.width // 8
        vin = run.ptr("vals_in") + int(base[s]) * 4 if c.form == T.PAIRS else None
        fk, fv, _ = plain(run.gs, run.cuda, flat, c.key_type, c.descending, c.form, kept,
                          run.ptr("keys_in") + int(base[s]) * isz, vin, {"n": int(length[s])}, 1)
        _same(c, "%s on sub-array %d, keys" % (flat, s), fk, gk[s:s + 1, :kept])
        if run.hv:
            _same(c, "%s on sub-array %d, values" % (flat, s), fv, gv[s:s + 1, :kept])


def eq_wide16(run, gk, gv):
    """The 16-bit call equals the 32-bit sibling on (uint32_t)key << 16 with the type widened, keys shifted back."""
    c, r = run.c, run.r
    sib = T.FAMILY_OF[(c.shape, 32)]
    wide = upload(c.keys.astype(np.uint32) << np.uint32(16), run.cuda)
    sk, sv, sc = plain(run.gs, run.cuda, sib, T.WIDEN[c.key_type], c.descending, c.form, c.k, wide.data_ptr(), run.ptr("vals_in"),
                       run.d, run.S)
    assert not ((sk & np.uint32(0xFFFF)) != 0)[r.written].any(), (c.describe(), sib, "returned a key that was not in its input")
    _same(c, sib + " on key << 16, keys", (sk >> np.uint32(16)).astype(np.uint16), gk, r.written)
    if run.hv:
        _same(c, sib + " on key << 16, values", sv, gv, r.written)
    if sc is not None:
        assert np.array_equal(sc, r.counts), (c.describe(), sib, "counts")


def eq_half(run, gk, gv):
    """On patterns of half the width shifted up, the call equals its sibling of half the width on the patterns themselves."""
    c, r = run.c, run.r
    half = c.width // 2
    sib = T.FAMILY_OF[(c.shape, half)]
    dt, nt = T.UINT[c.width], T.UINT[half]
    assert not (c.keys[: c.cols if c.shape in (T.ROWS, T.ANYK) else c.alloc] & dt((1 << half) - 1)).any()
    narrow = upload((c.keys >> dt(half)).astype(nt), run.cuda)
    kt = (T.NARROW32 if c.width == 64 else T.NARROW16)[c.key_type]
    sk, sv, sc = plain(run.gs, run.cuda, sib, kt, c.descending, c.form, c.k, narrow.data_ptr(), run.ptr("vals_in"), run.d, run.S)
    _same(c, sib + " on the narrow patterns, keys", sk.astype(dt) << dt(half), gk, r.written)
    if run.hv:
        _same(c, sib + " on the narrow patterns, values", sv, gv, r.written)
    if sc is not None:
        assert np.array_equal(sc, r.counts), (c.describe(), sib, "counts")


def eq_anyk_rows(run, gk, gv):
    """Any-k with k <= 1024 gives the rows call's bytes."""
    c = run.c
    sib = T.FAMILY_OF[(T.ROWS, c.width)]
    sk, sv, _ = plain(run.gs, run.cuda, sib, c.key_type, c.descending, c.form, c.k, run.ptr("keys_in"), run.ptr("vals_in"), run.d, run.S)
    _same(c, sib + ", keys", sk, gk)
    if run.hv:
        _same(c, sib + ", values", sv, gv)


def eq_rows_segmented(run, gk, gv):
    """The segmented call with the regular offsets r * stride equals the rows call."""
    c = run.c
    sib = T.FAMILY_OF[(T.SEG, c.width)]
    begin = (np.arange(c.rows, dtype=np.int64) * c.stride).astype(np.int32)
    d_begin, d_end = upload(begin, run.cuda), upload(begin + np.int32(c.cols), run.cuda)
    d = {"n": c.alloc, "S": c.rows, "begin": d_begin.data_ptr(), "end": d_end.data_ptr()}
    sk, sv, sc = plain(run.gs, run.cuda, sib, c.key_type, c.descending, c.form, c.k, run.ptr("keys_in"), run.ptr("vals_in"), d, run.S)
    _same(c, sib + " with regular offsets, keys", sk, gk)
    if run.hv:
        _same(c, sib + " with regular offsets, values", sv, gv)
    assert (sc == c.k).all(), (c.describe(), sib, "counts")


def equalities(c):
    """The equalities of include/gpusort.h that apply to a case; a case runs at most two of them, chosen by its index."""
    halves = c.dist == "widened" and c.width > 16
    eqs = []
    if c.shape != T.FLAT:
        eqs.append(eq_sub_flat)
    if c.width == 16:
        eqs.append(eq_wide16)
    if halves:
        eqs.append(eq_half)
    if c.shape == T.ANYK and c.k <= T.MAX_K:
        eqs.append(eq_anyk_rows)
    if c.shape == T.ROWS:
        eqs.append(eq_rows_segmented)
    if not eqs:
        return []
    return list(dict.fromkeys([eqs[c.index % len(eqs)], eqs[(c.index + 1) % len(eqs)]]))


def run_case(gs, cuda, family, seed, index):
    c = T.case(family, seed, index)
    run = Run(gs, cuda, c)
    run.call()
    snap = run.snapshot()
    diff = T.check(c, snap, run.r)
    assert diff is None, "%s: %s [%s]" % (c.name(), diff, c.describe())
    check_status(run)
    gk, gv, gc = run.outputs(snap)
    for eq in equalities(c):
        eq(run, gk, gv)
    if index % 8 == 0:                                # the same call again on the same workspace: identical output bytes
        run.call()
        again = run.outputs(run.snapshot())
        for name, a, b in zip(("keys", "values", "counts"), (gk, gv, gc), again):
            assert a is None or np.array_equal(a, b), "%s: %s differ between two runs on one workspace" % (c.name(), name)
    return run


# ---------------------------------------------------------------------------------------------------- the tests --
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("seed", T.SEEDS)
@pytest.mark.parametrize("family", tuple(T.FAMILIES))
def test_campaign(gs, cuda, family, seed, part):
    for index in range(part * PER_PART, (part + 1) * PER_PART):
        run_case(gs, cuda, family, seed, index)


@pytest.mark.parametrize("family,index", [("gs_topk_u16", 9), ("gs_topk_rows_u64", 3), ("gs_topk_rows_anyk_u32", 5),
                                          ("gs_topk_segmented_u16", 2)])
def test_check_reports_one_corrupted_output_element_of_a_correct_run(gs, cuda, family, index):
    """One bit of one output element flipped in place on the device, in the last slot a row or segment keeps."""
    run = run_case(gs, cuda, family, 1, index)
    c, r = run.c, run.r
    name = "keys_out" if c.form == T.KEYS or index % 2 else "vals_out"
    isz = c.width // 8 if name == "keys_out" else 4
    s = int(np.flatnonzero(r.counts)[-1])
    at = run.arena.slots[name][0] + (s * c.k + int(r.counts[s]) - 1) * isz
    run.arena.mem[at] ^= 0x04
    torch.cuda.synchronize()
    diff = T.check(c, run.snapshot(), r)
    assert diff is not None and ("row %d" % s in diff or "segment %d" % s in diff), (c.describe(), diff)
