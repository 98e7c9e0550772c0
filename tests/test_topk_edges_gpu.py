"""gs_topk_u32 at the edges of its own decisions and loops, bit for bit against tests/topk_ref.py (keys, values or indices, and
status words 0..7): the candidate list exactly full and one too many, at its smallest capacity and where n / 32 sets it; the
scan kernel's carry over two and three batches of 1024 tiles; the filter's bases with whole tiles and chunks of one digit in
front of the bucket, at 8k - 1 / 8k / 8k + 1 tiles and through a permuted group of chunks; d0 = 0 and 255 and k-th images
whose lower bytes are 0x00 or 0xFF, with the three cuts around every tie run; the local sort's classes in n and in k; a seeded
campaign; the Python front end's refusals.  The inputs come from tests/topk_cases.py, and tests/test_topk_edges_cpu.py holds
every one of them to its intent without a device.

Not reached here: a candidate list of more than 1024 tiles (route 1 with a second scan batch) needs n >= 268,697,600, and the
`i >= lo` wrap guards need n >= 2^31; neither reference fits a test of seconds.  The scan kernel is the same on both routes."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_cases as T
import topk_ref as R

pytestmark = pytest.mark.gpu

U32, I32, F32 = R.U32, R.I32, R.F32
KEYS, PAIRS, ARGS, MODES = T.KEYS, T.PAIRS, T.ARGS, T.MODES
ROUTES_SEEN = set()


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(cuda)


def host(t):
    return t.cpu().numpy().view(np.uint32)


class Case:
    """One input on the device with its reference (one stable argsort); .check(k, mode) runs the C entry point on a workspace
    filled with 0xA5 and outputs filled with -1, and compares keys, values or indices and the eight status words."""

    def __init__(self, gs, cuda, keys, kt, desc, what=""):
        self.gs, self.cuda, self.kt, self.desc, self.n, self.what = gs, cuda, kt, desc, keys.size, what
        self.vals = np.random.default_rng(3).integers(0, 1 << 32, keys.size, dtype=np.uint64).astype(np.uint32)
        self.ref = R.Ref(keys, kt, desc)
        self.d_keys, self.d_vals = dev(keys, cuda), dev(self.vals, cuda)

    def check(self, k, mode, expect_route=None, expect_top=None):
        gs, n = self.gs, self.n
        hv = int(mode != KEYS)
        nb = gs.lib.gs_topk_temp_bytes(n, k, hv)
        temp = torch.full((nb,), 0xA5, dtype=torch.uint8, device=self.cuda)
        ko = torch.full((k,), -1, dtype=torch.int32, device=self.cuda)
        vo = torch.full((k,), -1, dtype=torch.int32, device=self.cuda) if hv else None
        rc = gs.lib.gs_topk_u32(temp.data_ptr(), nb, self.d_keys.data_ptr(), self.d_vals.data_ptr() if mode == PAIRS else None,
                                ko.data_ptr(), vo.data_ptr() if hv else None, n, k, int(self.desc), self.kt, None)
        what = "%s n=%d k=%d %s kt=%d desc=%d" % (self.what, n, k, mode, self.kt, self.desc)
        assert rc == 0, (rc, what)
        st = (C.c_uint32 * 8)()
        assert gs.lib.gs_topk_status(temp.data_ptr(), n, k, hv, st, None) == 0, what
        ek, idx, est = self.ref.topk(k)
        route = self.ref.route(k)
        if expect_route is not None:
            assert route == expect_route, (what, route)
        if expect_top is not None:
            assert est[3] == expect_top, (what, est)
        assert list(st) == [route] + est + [0, 0, 0], (what, list(st), [route] + est)
        ROUTES_SEEN.add(int(st[0]))
        assert np.array_equal(host(ko), ek), what
        if hv:
            assert np.array_equal(host(vo), self.vals[idx] if mode == PAIRS else idx), what
        return int(st[0])


# ---------------------------------------------------------------------------------------------- capacity boundary --
@pytest.mark.parametrize("n,cap", T.CAPACITY)
@pytest.mark.parametrize("dc", [-1, 0, 1])
@pytest.mark.parametrize("desc", [False, True])
def test_candidate_list_one_short_exactly_full_and_one_too_many(gs, cuda, n, cap, dc, desc):
    """A top-byte bucket of cap - 1, cap and cap + 1 elements behind 20000 smaller ones: the list takes cap of them (route 1,
    the last at cand[cap - 1]) and not one more (route 2), at the smallest capacity, with n / 32 one above it and well above it.
    (One direction per item: at 3M elements an item is then one reference.)"""
    c, below = cap + dc, T.CAP_BELOW
    for kt in T.KEY_TYPES if n == T.CAPACITY[0][0] else (U32,):
        case = Case(gs, cuda, T.bucket_case(n, c, below, T.CAP_D0, n + dc, kt, desc), kt, desc, "bucket c=%d" % c)
        for j, (k, inside) in enumerate(T.capacity_ks(below, c)):
            for mode in MODES if j == 3 else (MODES[(j + kt + desc) % 3],):
                case.check(k, mode, expect_route=2 if inside and dc == 1 else 1, expect_top=c if inside else None)


# ------------------------------------------------------------------------------------------------- scan batches --
@pytest.mark.parametrize("n", T.SCAN_SIZES)
@pytest.mark.parametrize("kind", ["equal", "low24"])
def test_scan_carry_over_batches_of_1024_tiles(gs, cuda, n, kind):
    """Keys sharing one top byte, read from the input itself (route 2): 1024 tiles are one batch of the scan kernel, 1025 and
    1026 two, 2050 three.  All keys equal, indices form: the cut just before, at and behind the first batch's end (and the
    second's), where a wrong carry of the tie counts shows as wrong indices.  Random low 24 bits, pairs form: the carry of
    the counts before the k-th image.  One reference per item: its stable argsort of 8M or 16M keys is most of the item's
    time, which is why the two inputs of a size are two items."""
    i = T.SCAN_SIZES.index(n)
    kt, desc = T.KEY_TYPES[i % 3], bool(i % 2)
    if kind == "equal":
        case = Case(gs, cuda, T.equal_case(n, kt, desc), kt, desc, kind)
        for k in T.scan_equal_ks(n):
            case.check(k, ARGS, expect_route=2, expect_top=n)
    else:
        case = Case(gs, cuda, T.topbyte_case(n, 3 + i, kt, desc), kt, desc, kind)
        for k in T.scan_random_ks(n):
            case.check(k, PAIRS, expect_route=2, expect_top=n)


def test_route_one_through_a_permuted_group_of_chunks(gs, cuda):
    """Uniform keys at 2050 tiles = 257 chunks: the upsweep's first 256 workgroups take permuted chunks, and the filter's bases
    sum spine columns of all of them.  An item of its own: one reference, the argsort of 16.8M keys."""
    n = T.SCAN_SIZES[-1]
    case = Case(gs, cuda, T.uniform_case(n, 8, I32, True), I32, True, "uniform")
    case.check(T.SPINE_K, PAIRS, expect_route=1)
    case.check(T.SPINE_K, KEYS, expect_route=1)


# ------------------------------------------------------------------------------------------------------ layout --
@pytest.mark.parametrize("n,c,route", T.LAYERED)
def test_filter_bases_with_whole_tiles_and_chunks_in_front_of_the_bucket(gs, cuda, n, c, route):
    """A chunk of one digit below d0, then seven tiles of it and a tile of the bucket (that tile's prefix16 is 57344), then
    mixed tiles; 23, 24 and 25 tiles.  The staged group must start where spine + prefix16 of every lower digit say."""
    for j, (kt, desc) in enumerate([(U32, False), (F32, True), (I32, True)]):
        keys, below = T.layered_case(n, c, n + c, kt, desc)
        case = Case(gs, cuda, keys, kt, desc, "layered c=%d" % c)
        for k in T.layered_ks(below, c):
            for mode in MODES:
                case.check(k, mode, expect_route=route, expect_top=c)
        case.check(below, MODES[j])                                    # the last element in front of the bucket


# -------------------------------------------------------------------------------------------------- digit edges --
@pytest.mark.parametrize("route,top", T.DIGIT_EDGES)
@pytest.mark.parametrize("kt", T.KEY_TYPES)
def test_extreme_digits_and_the_three_cuts_around_every_tie_run(gs, cuda, route, top, kt):
    """Runs of twenty images whose bytes are 0x00, 0x01, 0x7F, 0x80, 0xFE and 0xFF: every pick round meets digit 0 and digit
    255, on the candidate list and (route 2) on the input; k is the last of each run, the first of the next, and one before."""
    for desc in (False, True):
        case = Case(gs, cuda, T.digit_edge_case(route, top, kt, desc), kt, desc, "digits route=%d top=%#x" % (route, top))
        routes = {case.check(k, MODES[j % 3]) for j, k in enumerate(T.run_cuts(case.ref))}
        assert routes == ({1, 2} if route == 2 else {1})


# -------------------------------------------------------------------------------------------------- class edges --
@pytest.mark.parametrize("n", T.CLASS_EDGES)
def test_local_sort_classes_in_n(gs, cuda, n):
    """Route 3 sorts the whole array in one workgroup: both sides of each class edge of that sort."""
    i = T.CLASS_EDGES.index(n)
    kt, desc = T.KEY_TYPES[i % 3], bool((i // 2) % 2)
    case = Case(gs, cuda, T.uniform_case(n, n, kt, desc), kt, desc, "uniform")
    for j, k in enumerate((1, n // 2, n)):
        for mode in MODES if j == 2 else (MODES[(i + j) % 3],):
            case.check(k, mode, expect_route=3)


@pytest.mark.parametrize("kind,route", [("uniform", 1), ("topbyte", 2)])
def test_local_sort_classes_in_k(gs, cuda, kind, route):
    """Routes 1 and 2 finish with the library's sort of the k staged pairs: k on both sides of each of its class edges."""
    build = T.uniform_case if kind == "uniform" else T.topbyte_case
    for kt, desc in [(U32, False), (F32, True)]:
        case = Case(gs, cuda, build(T.CLASS_N, 1 + route, kt, desc), kt, desc, kind)
        for k in T.CLASS_KS:
            for mode in (KEYS, PAIRS):
                case.check(k, mode, expect_route=route)


# ----------------------------------------------------------------------------------------------------- campaign --
CAMPAIGN_PARTS = 4


@pytest.mark.parametrize("seed", T.CAMPAIGN_SEEDS)
@pytest.mark.parametrize("part", range(CAMPAIGN_PARTS))
def test_seeded_campaign(gs, cuda, seed, part):
    """Sizes around 17408, 65536 and 100003 and 300007, five distributions, cuts around tie runs and random k, random key type,
    direction and form; a failure prints the case (topk_cases.campaign_case(seed, index) rebuilds it)."""
    for index in range(part, T.CAMPAIGN_CASES, CAMPAIGN_PARTS):
        what, keys, kt, desc, rng = T.campaign_case(seed, index)
        case = Case(gs, cuda, keys, kt, desc, what)
        for k, mode in T.campaign_ks(case.ref, rng):
            case.check(k, mode)


def test_every_route_is_taken_in_this_file(gs, cuda):
    n, cap = T.CAPACITY[0]
    for c, route in ((cap, 1), (cap + 1, 2)):
        case = Case(gs, cuda, T.bucket_case(n, c, T.CAP_BELOW, T.CAP_D0, 77), U32, False, "bucket c=%d" % c)
        assert case.check(T.CAP_BELOW + c, ARGS, expect_top=c) == route
    assert Case(gs, cuda, T.uniform_case(9217, 1), U32, False).check(4609, PAIRS) == 3
    assert {1, 2, 3} <= ROUTES_SEEN


# ---------------------------------------------------------------------------------------------------- front end --
def _buffers(cuda, n, k, dtype=torch.int32):
    keys = torch.arange(n, dtype=torch.int32, device=cuda).to(dtype)
    return keys, torch.empty(k, dtype=dtype, device=cuda), torch.empty(k, dtype=torch.int32, device=cuda)


def test_device_topk_refuses_16_bit_keys(gs, cuda):
    n, k = 1000, 10
    nb = gs.DeviceTopK.MinPairs(None, 0, None, None, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    for dtype in (torch.int16, torch.float16, torch.bfloat16):
        keys, ko, vo = _buffers(cuda, n, k, dtype)
        with pytest.raises(TypeError):
            gs.DeviceTopK.MinKeys(temp, nb, keys, ko, n, k)
        with pytest.raises(TypeError):
            gs.DeviceTopK.MaxPairs(temp, nb, keys, ko, None, vo, n, k)


def test_device_topk_refuses_short_outputs_and_writes_nothing(gs, cuda):
    n, k = 1000, 10
    nb = gs.DeviceTopK.MinPairs(None, 0, None, None, None, None, n, k)
    temp = torch.empty(nb, dtype=torch.uint8, device=cuda)
    keys, ko, vo = _buffers(cuda, n, k)
    short = torch.full((k - 1,), -1, dtype=torch.int32, device=cuda)
    ko.fill_(-1)
    vo.fill_(-1)
    with pytest.raises(ValueError, match="d_keys_out"):
        gs.DeviceTopK.MinKeys(temp, nb, keys, short, n, k)
    with pytest.raises(ValueError, match="d_keys_out"):
        gs.DeviceTopK.MaxPairs(temp, nb, keys, short, None, vo, n, k)
    with pytest.raises(ValueError, match="d_values_out"):
        gs.DeviceTopK.MinPairs(temp, nb, keys, ko, None, short, n, k)
    with pytest.raises(ValueError, match="d_values_out"):
        gs.DeviceTopK.MinPairs(temp, nb, keys, ko, keys.clone(), short, n, k)
    torch.cuda.synchronize()
    assert bool((short == -1).all()) and bool((ko == -1).all()) and bool((vo == -1).all())
    gs.DeviceTopK.MinPairs(temp, nb, keys, ko, None, vo, n, k)          # the same buffers at full length are accepted
    torch.cuda.synchronize()
    assert ko.tolist() == list(range(k)) and vo.tolist() == list(range(k))


def test_topk_refuses_values_with_indices_and_k_out_of_range(gs, cuda):
    keys, _, _ = _buffers(cuda, 100, 1)
    with pytest.raises(ValueError):
        gs.topk(keys, 5, values=keys.clone(), indices=True)
    with pytest.raises(ValueError):
        gs.topk(keys, 101)
    with pytest.raises(ValueError):
        gs.topk(keys, -1)
    ko, vo = gs.topk(keys, 100, largest=True, indices=True)             # k = n is in range
    assert ko.tolist() == list(range(99, -1, -1)) and vo.tolist() == list(range(99, -1, -1))


def test_topk_of_zero_returns_empty_tensors_and_launches_nothing(gs, cuda, monkeypatch):
    def launched(*a, **kw):
        raise AssertionError("topk(k=0) reached DeviceTopK")
    monkeypatch.setattr(gs.DeviceTopK, "_run", staticmethod(launched))
    keys = torch.arange(100, dtype=torch.float32, device=cuda)
    ko, vo = gs.topk(keys, 0)
    assert ko.numel() == 0 and ko.dtype == torch.float32 and ko.device == keys.device and vo is None
    ko, vo = gs.topk(keys, 0, indices=True)
    assert ko.numel() == 0 and vo.numel() == 0 and vo.dtype == torch.int32
    ko, vo = gs.topk(keys, 0, values=keys.clone())
    assert ko.numel() == 0 and vo.numel() == 0 and vo.dtype == torch.float32
