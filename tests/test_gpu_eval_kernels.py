"""The five kernels of csrc/census.hip -- segment sum, dasymetric rescale, window stitcher, its finalize, batched visit count -- against the
float64 / int64 yardsticks of tests/eval_kernels_oracle.py: known answers by equality wherever the arithmetic is exact, derived bars (that
module's docstring) where it is not, at the shapes where these kernels take another path.  Every operand, accumulator, count map, sum and
workspace is created inside ``Footprint(..., POISON)`` (tests/footprint.py): it sits between guard bands, and a store outside it fails
the exit check.  tests/test_eval_kernels_cpu.py runs the same verdicts on fp32 restatements: the honest ones pass, the planted defects
fail.  The test bodies (``.body``) are reused by tests/test_gpu_footprint_ops.py."""
import functools

import numpy as np
import pytest
import torch

from tests import census_oracle as CO
from tests import eval_kernels_oracle as K
from tests import footprint as FP

pytestmark = pytest.mark.gpu


def guarded(fn):
    """run the test between guard bands; ``.body`` is the test without them (for a caller that brings its own harness)"""
    @functools.wraps(fn)
    def run(*a, **k):
        with FP.Footprint("cuda", fill=FP.POISON) as fp:
            fn(*a, **k)
        assert fp.guarded > 0
    run.body = fn
    return run


def _planes(st):
    torch.cuda.synchronize()
    get = lambda t: None if t is None else t.cpu().numpy().copy()  # noqa: E731
    return {"out": get(st.out), "out_sq": get(st.out_sq), "scale": get(st.scale), "scale_sq": get(st.scale_sq), "count": get(st.count)}


def _feed(st, wins):
    for xl, yl, pd, sc, ov in wins:
        st.add_window(xl, yl, torch.from_numpy(pd).cuda(), None if sc is None else torch.from_numpy(sc).cuda(), ov)


# ---- stitcher, exact -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,scale", [(1, "all"), (2, "all"), (4, "all"), (2, "some"), (2, "none")])
@guarded
def test_stitcher_exact_known_answer(M, scale):
    """Integer values 0 .. 7, rectangular windows of both orientations that stick out on every side, overlap 0 and ps <= 2 overlap, windows
    outside (eval_kernels_oracle.exact_windows).  ``some``: every third window passes scale=None into a stitcher that has scale planes;
    ``none``: Stitcher(with_scale=False).  Verdict: exact_verdict -- equality before finalize, equality after it where c is 2, 4 or 8."""
    from popcorn_amd import eval as E
    wins = K.exact_windows(M, scale=scale)
    K.exact_conditions(K.stitch64(K.H, K.W, wins, K.OV), M)
    st = E.Stitcher(K.H, K.W, "cuda", with_scale=scale != "none")
    _feed(st, wins[:3])
    part = _planes(st)
    noop = [w for w in wins if w[2].shape[1] <= 2 * w[4]]
    assert len(noop) == 1
    _feed(st, noop)                                                      # ps <= 2 overlap: planes and count unchanged, bit for bit
    again = _planes(st)
    assert all(part[k] is None or np.array_equal(part[k].view(np.int32 if part[k].dtype == np.float32 else np.int16),
                                                 again[k].view(np.int32 if again[k].dtype == np.float32 else np.int16)) for k in part)
    _feed(st, wins[3:])
    before = _planes(st)
    st.finalize()
    fails = K.exact_verdict(before, _planes(st), wins, with_scale=scale != "none")
    assert fails == [], fails


@guarded
def test_stitcher_finalize_on_a_band_leaves_the_other_rows_alone():
    """``st.band = K.BAND`` = (7, 30): the band starts at an odd row of the odd-width raster (byte offset 7 * 45 * 4: 4-byte phase); rows outside
    it keep their sums bit for bit, rows inside follow the exact verdict"""
    from popcorn_amd import eval as E
    band = K.BAND
    wins = K.exact_windows(2)
    st = E.Stitcher(K.H, K.W, "cuda")
    _feed(st, wins)
    before = _planes(st)
    st.band = band
    st.finalize()
    assert (st.out[band[0]:].data_ptr() - st.out.data_ptr()) % 16 != 0
    fails = K.exact_verdict(before, _planes(st), wins, band=band)
    assert fails == [], fails


# ---- stitcher, full mantissa ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spread", "near"])
@guarded
def test_stitcher_full_mantissa_within_derived_bars(kind):
    """M = 3, c = 3, 6, 12, non-negative full-mantissa values, against stitch64.  With u = 2^-24 (derivation: tests/eval_kernels_oracle.py)

        |mean - mean64| <= (c + 1) u sum|v| / c            |(c - 1) std^2 - (c - 1) var64| <= (3c + 10) u sum v^2

    and a NaN only where (c - 1) var64 <= that second bar.  ``spread``: >= 90 % of the pixels have (c - 1) var64 > 100 x the bar and no NaN
    is permitted; ``near`` (the ensemble differs in the last ulps): >= 1 % of the pixels lie inside the cancellation zone."""
    from popcorn_amd import eval as E
    wins = K.mantissa_windows(kind)
    K.mantissa_conditions(K.stitch64(K.H, K.W, wins, K.OV), kind)
    st = E.Stitcher(K.H, K.W, "cuda")
    _feed(st, wins)
    st.finalize()
    fails, reports = K.mantissa_verdict(_planes(st), wins, kind)
    print("\n" + "\n".join(reports))
    assert fails == [], fails


def test_stitch_accumulate_refuses_what_it_cannot_clip():
    """pc_stitch_accumulate: PC_EINVAL for a negative overlap and for H or W below 1, with nothing launched (the planes keep their
    bits); the same call with overlap 0 goes through"""
    from popcorn_amd import _lib as L
    from popcorn_amd import eval as E
    st = E.Stitcher(5, 6, "cuda")
    pd = torch.ones(2, 4, 4, device="cuda")
    fn = L.lib().pc_stitch_accumulate

    def call(overlap, h, w):
        return fn(L.ptr(pd), None, 2, 4, 4, overlap, 0, 0, L.ptr(st.out), L.ptr(st.out_sq), None, None, L.ptr(st.count), h, w, L.stream_ptr())

    assert call(-1, 5, 6) == L.PC_EINVAL and call(0, 0, 6) == L.PC_EINVAL and call(0, 5, 0) == L.PC_EINVAL
    with pytest.raises(L.PopcornHipError):
        st.add_window(0, 0, pd, None, -1)
    torch.cuda.synchronize()
    assert not st.out.any() and not st.out_sq.any() and not st.count.any()
    assert call(0, 5, 6) == 0
    torch.cuda.synchronize()
    assert float(st.out.sum()) == 2 * 16 and int(st.count.sum()) == 2 * 16


def test_every_consumer_of_the_window_list_refuses_a_raster_below_the_patch():
    """ProductGrid.set_windows, CensusTable.set_windows and ResidentWindows (evaluate_raster and run_eval: tests/test_eval_kernels_cpu.py)
    raise the ValueError of eval.require_raster_fits, naming h, w and patchsize, and leave their state alone"""
    from popcorn_amd import eval as E
    from popcorn_amd.data.region import ResidentRegion, ResidentWindows
    from popcorn_amd.data.dataset import SyntheticTestRaster
    h, w, ps = 40, 30, 32
    pg = E.ProductGrid(h, w, 1, 2, "cuda")
    ct = E.CensusTable(h, w, [torch.zeros(h, w, dtype=torch.int32)], [1], 2, "cuda")
    pg.cells.fill_(1.0)
    ct.table.fill_(1)
    for what in (pg, ct):
        with pytest.raises(ValueError) as e:
            what.set_windows([(0, 0, 0)], ps, 4)
        assert all(s in str(e.value) for s in (f"h {h}", f"w {w}", f"patchsize {ps}", type(what).__name__))
    assert bool((pg.cells == 1).all()) and bool((ct.table == 1).all())
    pg.set_windows([(0, 0, 0)], 30, 4)                                   # a side of exactly one patch is defined
    data = SyntheticTestRaster(h, w, seasons=1, n_regions=9, seed=3, device="cuda", raw=True)
    with pytest.raises(ValueError) as e:
        ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=True), ps, 4)
    assert all(s in str(e.value) for s in (f"h {h}", f"w {w}", f"patchsize {ps}", "ResidentWindows"))


# ---- the three accumulators of one evaluation ----------------------------------------------------------------------------------------------
@guarded
def test_three_accumulators_agree_on_out_sticking_windows():
    """Stitcher, ProductGrid(cell=1) and CensusTable over one id raster and one window list with negative origins, integer values and visit
    counts 1, 2, 4: all three follow from stitch64 by equality (every division by a visit count is exact; the table's 2^-30 fixed point
    holds multiples of 1/4 exactly)."""
    from popcorn_amd import eval as E
    wins, boundary, num_ids = K.accumulators_case()
    M = K.ACC_M
    ref = K.stitch64(K.H, K.W, wins, K.OV)
    per = [K.stitch64(K.H, K.W, [(x, y, pd[m:m + 1], None, ov) for x, y, pd, _, ov in wins], K.OV) for m in range(M)]
    visits = per[0]["count"]
    assert np.array_equal(ref["count"], M * visits) and set(np.unique(visits)) == {1, 2, 4} and min(x for x, *_ in wins) < 0
    assert np.array_equal(sum(p["pd"]["sum"] for p in per), ref["pd"]["sum"])
    maps = np.stack([p["pd"]["sum"] / visits for p in per])             # every member's stitched map: exact quarters
    idx = [(x, y, 0) for x, y, *_ in wins]
    st = E.Stitcher(K.H, K.W, "cuda", with_scale=False)
    pg = E.ProductGrid(K.H, K.W, 1, M, "cuda")
    ct = E.CensusTable(K.H, K.W, [torch.from_numpy(boundary)], [num_ids], M, "cuda")
    pg.set_windows(idx, K.ACC_PS, K.OV)
    ct.set_windows(idx, K.ACC_PS, K.OV)
    for x, y, pd, _, ov in wins:
        d = torch.from_numpy(pd).cuda()
        st.add_window(x, y, d, None, ov)
        pg.add_window(x, y, d, ov)
        ct.add_window(x, y, d, ov)
    totals, _, _ = ct.finalize()
    torch.cuda.synchronize()
    assert np.array_equal(pg.visits.cpu().numpy(), visits) and np.array_equal(ct.visits.cpu().numpy(), visits)
    assert np.array_equal(st.count.cpu().numpy(), ref["count"])
    assert np.array_equal(st.out.cpu().numpy().astype(np.float64), ref["pd"]["sum"])
    assert np.array_equal(st.out_sq.cpu().numpy().astype(np.float64), ref["pd"]["sq"])
    assert np.array_equal(pg.cells.cpu().numpy().astype(np.float64), maps)
    want = np.stack([CO.unit_sums(maps[m], boundary, num_ids) for m in range(M)])
    assert (want > 0).all() and np.array_equal(totals.cpu().numpy(), want)


# ---- visit count ---------------------------------------------------------------------------------------------------------------------------
class _AbiSpy:
    """the loaded library with the window count of every pc_stitch_count_windows call written down"""

    def __init__(self, lib):
        self._lib, self.nwin = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != "pc_stitch_count_windows":
            return f

        def call(win, nwin, *rest):
            self.nwin.append(int(nwin))
            return f(win, nwin, *rest)
        return call


def _count_both_ways(h, w, wins, M):
    """add_counts_only == count64 == add_count_only per window; returns (count64, the nwin the kernel was launched with)"""
    from popcorn_amd import eval as E
    want = K.count64(h, w, wins, M, K.COUNT_PS, K.COUNT_OV)
    assert want.max() <= 32767                                           # the int16 range of the map (a condition, not a measurement)
    a, b = E.Stitcher(h, w, "cuda", with_scale=False), E.Stitcher(h, w, "cuda", with_scale=False)
    spy = _AbiSpy(E.L.lib())
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(E.L, "lib", lambda: spy)
        a.add_counts_only(wins, M, K.COUNT_PS, K.COUNT_OV)
    for x, y in wins:
        b.add_count_only(x, y, M, K.COUNT_PS, K.COUNT_OV)
    torch.cuda.synchronize()
    assert torch.equal(a.count.cpu(), torch.from_numpy(want).to(torch.int16))
    assert torch.equal(a.count, b.count)
    assert len(spy.nwin) == 1
    return want, spy.nwin[0]


@pytest.mark.parametrize("w", [5, 1023, 1024, 1025, 1030])
@pytest.mark.parametrize("nwin", [1, 1024, 1025, 2049])
@guarded
def test_visit_count_batches_and_column_blocks(nwin, w):
    """``CW_CAP`` = 1024 windows per LDS batch and ``nwin`` is what the KERNEL is launched with (observed at the ABI call): 1024 fills one
    batch to its last slot, 1025 puts one window into a second batch, 2049 one window into a third (the host drops the windows that begin
    at or beyond the last row / column, so the list is longer than nwin: eval_kernels_oracle.count_case).  Kernel row 1023 alone covers
    pixel (8, 0) and kernel row 1024 alone covers (8, w - 1): losing either, or counting it twice, shows there.  1024 columns per block
    (1025 and 1030: a second block, ragged four-column tail), H = 9; origins from wholly above / left of the raster (they reach the kernel)
    to partly below / right of it."""
    M = 3 if (nwin + w) % 2 else 1
    wins = K.count_case(nwin, 9, w)
    rows = K.kernel_rows(wins, 9, w)
    assert len(rows) == nwin < len(wins)
    want, launched = _count_both_ways(9, w, wins, M)
    assert launched == nwin
    if nwin >= K.CW_CAP:
        others = rows[:K.CW_CAP - 1] + rows[K.CW_CAP + 1:]
        assert not K.count64(9, w, others, 1, K.COUNT_PS, K.COUNT_OV)[8].any()
        assert want[8, 0] == M and want[8, w - 1] == (M if nwin > K.CW_CAP else 0) and not want[8, 1:w - 1].any()
        assert any(x + K.COUNT_PS - K.COUNT_OV <= 0 for x, _ in rows) and any(y + K.COUNT_PS - K.COUNT_OV <= 0 for _, y in rows)
        assert any(-K.COUNT_OV > x > K.COUNT_OV - K.COUNT_PS for x, _ in rows) and any(y + K.COUNT_PS - K.COUNT_OV > w for _, y in rows)


@guarded
def test_visit_count_rows_beyond_the_grid():
    """H = 65540 > 65535 rows of the launch grid: the rows at and beyond 65535 are reached by the row loop's second trip"""
    h, w, wins = K.TALL
    want, launched = _count_both_ways(h, w, wins, 3)
    assert launched == len(K.kernel_rows(wins, h, w)) == len(wins)
    assert (want[65535:] > 0).any() and (want[:5] > 0).any() and (want[65534] > 0).any()


# ---- segment sum ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 4099, 20001])
@pytest.mark.parametrize("num_ids", [1, 4096, 4097])
@guarded
def test_segment_sum_exact_at_every_alignment_phase(num_ids, n):
    """Integer-valued pred (|v| < 2^20): the float64 sums and int32 counts ARE segment64's, for all 16 start phases of pred x boundary
    (views offset by 0 .. 3 elements), num_ids at and beyond the LDS-private limit of 4096, n below the scalar head, n % 4 != 0, more than
    one workgroup (20001), with the ids -1, INT_MIN, INT_MAX and num_ids present and ignored; with and without counts."""
    from popcorn_amd import eval as E
    pred, ids = K.segment_case(num_ids, n)
    dp, di = torch.from_numpy(pred).cuda(), torch.from_numpy(ids).cuda()
    assert dp.data_ptr() % 16 == 0 and di.data_ptr() % 16 == 0
    for pp in range(4):
        for bp in range(4):
            want, wc = K.segment64(pred[pp:pp + n], ids[bp:bp + n], num_ids)
            sums, counts = E.census_sums(dp[pp:pp + n], di[bp:bp + n], num_ids, want_counts=True)
            only = E.census_sums(dp[pp:pp + n], di[bp:bp + n], num_ids)
            assert sums.dtype == torch.float64 and counts.dtype == torch.int32
            assert np.array_equal(sums.cpu().numpy(), want), (pp, bp)
            assert np.array_equal(counts.cpu().numpy().astype(np.int64), wc), (pp, bp)
            assert np.array_equal(only.cpu().numpy(), want), (pp, bp)


@pytest.mark.parametrize("num_ids", [7, 4097])
@guarded
def test_segment_sum_full_mantissa_and_reproducible(num_ids):
    """fp64 accumulation of fp32 terms in any order: per id |sum - exact| <= n_id 2^-53 sum|v| (n_id - 1 additions of at most that
    partial sum each, the conversion of a term is exact); two runs give the same bits once rounded to fp32."""
    from popcorn_amd import eval as E
    n = 20001
    rng = np.random.default_rng(6000 + num_ids)
    pred = ((rng.random(n) - 0.25) * 1000).astype(np.float32)
    ids = rng.integers(-1, num_ids + 1, size=n).astype(np.int32)
    want, wc = K.segment64(pred, ids, num_ids)
    mag, _ = K.segment64(np.abs(pred), ids, num_ids)
    dp, di = torch.from_numpy(pred).cuda(), torch.from_numpy(ids).cuda()
    s1, c1 = E.census_sums(dp, di, num_ids, want_counts=True)
    s2 = E.census_sums(dp, di, num_ids)
    err, bar = np.abs(s1.cpu().numpy() - want), wc * 2.0 ** -53 * mag
    print(f"\n[segment sum] num_ids {num_ids}: worst error / bar {np.max(err[bar > 0] / bar[bar > 0]):.3f}")
    assert (err <= bar).all() and np.array_equal(c1.cpu().numpy().astype(np.int64), wc)
    assert FP.bit_equal(s1.float(), s2.float())


@guarded
def test_segment_sum_nan_stays_in_its_unit():
    from popcorn_amd import eval as E
    num_ids, n = 4097, 4099
    pred, ids = K.segment_case(num_ids, n)
    pred, ids = pred[:n].copy(), ids[:n].copy()
    at = int(np.flatnonzero((ids >= 0) & (ids < num_ids))[17])
    clean = E.census_sums(torch.from_numpy(pred).cuda(), torch.from_numpy(ids).cuda(), num_ids).cpu()
    pred[at] = np.nan
    dirty = E.census_sums(torch.from_numpy(pred).cuda(), torch.from_numpy(ids).cuda(), num_ids).cpu()
    other = torch.ones(num_ids, dtype=torch.bool)
    other[int(ids[at])] = False
    assert bool(torch.isnan(dirty[int(ids[at])])) and FP.bit_equal(dirty[other], clean[other]) and not bool(torch.isnan(clean).any())


# ---- rescale -------------------------------------------------------------------------------------------------------------------------------
@guarded
def test_rescale_is_the_fp32_restatement_bit_for_bit():
    """adjust_map_to_census == adjust32 (s = f32(sum), q = f32(pop / s), f32(pred q): two correctly rounded fp32 operations).  pred holds
    multiples of 2^-10 below 2^6, so the fp64 sums are exact in any order and f32(sum) is not in doubt; pop is full-mantissa.  A unit
    without a census row, a unit whose sum is exactly 0, ids beyond num_ids, outside pixels (-1), unsorted census rows, num_ids larger
    than the largest id in the raster, and pred a view at a 4-byte phase."""
    from popcorn_amd import eval as E
    h, w = 29, 23
    rng = np.random.default_rng(7000)
    b = ((np.arange(h)[:, None] // 5) * 4 + np.arange(w)[None, :] // 6).astype(np.int32)       # ids 0 .. 23
    b[:2] = -1
    b[b == 23] = 40                                                      # beyond num_ids = 31
    pred = (rng.integers(1, 2 ** 16, size=(h, w)) * 2.0 ** -10).astype(np.float32)
    pred[b == 6] = 0.0                                                   # a unit whose sum is exactly 0
    census_idx = [i for i in rng.permutation(23).tolist() if i != 9] + [30]      # unsorted; unit 9 has no row; 30 is not in the raster
    pop = (rng.random(len(census_idx)) * 5000 + 1).astype(np.float32)
    num_ids = 31
    sums, _ = K.segment64(pred, b, num_ids)
    assert sums[6] == 0 and sums[9] > 0 and (b == 40).any() and (b == -1).any() and census_idx != sorted(census_idx)
    table, has = np.zeros(num_ids, np.float32), np.zeros(num_ids, np.uint8)
    table[census_idx], has[census_idx] = pop, 1
    want = K.adjust32(pred, b, sums, table, has)
    buf = torch.zeros(h * w + 4)
    buf[1:1 + h * w] = torch.from_numpy(pred).reshape(-1)
    dpred = buf.cuda()[1:1 + h * w].view(h, w)
    assert dpred.data_ptr() % 16 == 4 and dpred.is_contiguous()
    got = E.adjust_map_to_census(dpred, torch.from_numpy(b).cuda(), census_idx, pop)
    assert got.data_ptr() == dpred.data_ptr()
    untouched = (b < 0) | (b == 40) | (b == 9) | (b == 6)
    assert np.array_equal(want[untouched], pred[untouched]) and not np.array_equal(want[~untouched], pred[~untouched])
    assert FP.bit_equal(got.cpu(), torch.from_numpy(want))
