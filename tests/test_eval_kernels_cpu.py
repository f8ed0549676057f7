"""The yardsticks of tests/test_gpu_eval_kernels.py judged without a device (tests/eval_kernels_oracle.py):

  * the float64 oracle agrees with the pinned restatement of the reference's loops (oracle.popcorn_oracle.stitch_loop / census_sums);
  * an honest fp32 evaluation of the stitcher -- every product rounded, or the compiler's two contractions emulated, members in either
    order -- passes every equality, bar and NaN rule on every input the GPU file uses (a bar the honest formula breaks would be wrong);
  * every planted defect is rejected by the same verdicts on the same inputs;
  * a raster smaller than the patch is refused before anything touches a device."""
import types

import numpy as np
import pytest
import torch

from oracle import popcorn_oracle as O
from tests import eval_kernels_oracle as K

EXACT_INPUTS = [(1, "all"), (2, "all"), (4, "all"), (2, "some"), (2, "none")]
HONEST = [(False, False), (False, True), (True, False), (True, True)]              # (contract, members reversed)


# ---- the oracle against the pinned restatement of the reference ----------------------------------------------------------------------------
def test_stitch64_agrees_with_the_reference_loop_on_square_windows():
    """stitch_loop is the reference's loop in fp32 torch: an honest fp32 evaluation.  Counts are equal; its maps lie within the derived
    bars of stitch64 (its own precision: the bars are a few fp32 roundings wide) and its plain sums where c = 1 are the oracle's."""
    from popcorn_amd.eval import get_patch_indices
    h, w, ps, ov, M = 150, 170, 64, 8, 3
    g = torch.Generator().manual_seed(4)
    wins = [(x, y, torch.rand(M, ps, ps, generator=g), torch.rand(M, ps, ps, generator=g))
            for x, y, s in get_patch_indices(h, w, ps, ov, False).tolist()]
    out, out_sq, sc, sc_sq, cnt = O.stitch_loop(h, w, wins, ps, ov)
    ref = K.stitch64(h, w, [(x, y, pd.numpy(), s.numpy()) for x, y, pd, s in wins], ov)
    assert np.array_equal(cnt.numpy().astype(np.int64), ref["count"]) and ref["count"].max() == 12 and (ref["count"] == 0).any()
    for name, m, s in (("pd", out, out_sq), ("sc", sc, sc_sq)):
        ok, rep = K.judge(name, m.numpy(), s.numpy(), ref["count"], ref[name])
        print(rep)
        assert ok, rep
    assert np.array_equal(K.count64(h, w, [(x, y) for x, y, *_ in wins], M, ps, ov), ref["count"])


def test_segment64_agrees_with_the_reference_sums():
    rng = np.random.default_rng(0)
    b = rng.integers(-1, 40, size=(61, 53)).astype(np.int32)
    full = (rng.random((61, 53)) * 3).astype(np.float32)
    want = O.census_sums(full, b, 37)                                   # float64 running sums: n 2^-53 relative at the worst
    got, counts = K.segment64(full, b, 37)
    assert np.allclose(got, want, rtol=61 * 53 * 2.0 ** -53, atol=0) and np.array_equal(counts, np.bincount(b[(b >= 0) & (b < 37)], minlength=37))
    ints = rng.integers(-1000, 1000, size=(61, 53)).astype(np.float32)
    assert np.array_equal(K.segment64(ints, b, 37)[0], O.census_sums(ints, b, 37))
    # the rescale's restatement against the reference's loop where that is exact: power-of-two factors
    pred = rng.integers(1, 9, size=(8, 8)).astype(np.float32)
    bb = np.repeat(np.arange(4), 16).reshape(8, 8).astype(np.int32)
    sums, _ = K.segment64(pred, bb, 4)
    pop = (sums * np.array([2.0, 0.5, 4.0, 1.0])).astype(np.float32)
    adj = K.adjust32(pred, bb, sums, pop, np.ones(4, np.uint8))
    bbox = [(2 * i, 2 * i + 2, 0, 8) for i in range(4)]
    want = O.adjust_map_to_census_loop(torch.from_numpy(pred), torch.from_numpy(bb.astype(np.float32)), list(range(4)), bbox, torch.from_numpy(pop))
    assert np.array_equal(adj, want.numpy())


# ---- the honest fp32 evaluation passes on the GPU file's own inputs ------------------------------------------------------------------------
@pytest.mark.parametrize("M,scale", EXACT_INPUTS)
def test_honest_fp32_passes_the_exact_verdict(M, scale):
    wins = K.exact_windows(M, scale=scale)
    K.exact_conditions(K.stitch64(K.H, K.W, wins, K.OV), M)
    results = []
    for contract, reverse in HONEST:
        before, after = K.stitch32(K.H, K.W, wins, K.OV, with_scale=scale != "none", contract=contract, reverse=reverse)
        assert K.exact_verdict(before, after, wins, with_scale=scale != "none") == []
        results.append(after)
    # on the pixels held to equality the contracted and the uncontracted form coincide (the claim the equality rests on)
    c = K.stitch64(K.H, K.W, wins, K.OV)["count"]
    sel = np.isin(c, K.EXACT_C)
    for k in ("out", "out_sq"):
        assert np.array_equal(results[0][k][sel].view(np.int32), results[2][k][sel].view(np.int32))


def test_honest_fp32_passes_the_exact_verdict_on_a_band():
    wins = K.exact_windows(2)
    ref = K.stitch64(K.H, K.W, wins, K.OV)
    for contract in (False, True):
        before, _ = K.stitch32(K.H, K.W, wins, K.OV, contract=contract)
        after = dict(before)
        for k, k2 in (("out", "out_sq"), ("scale", "scale_sq")):
            after[k], after[k2] = K.finalize32(before[k], before[k2], before["count"], contract, rows=K.BAND)
        assert K.exact_verdict(before, after, wins, band=K.BAND) == []
    assert (ref["count"][K.BAND[0]:K.BAND[1]] > 1).any()


@pytest.mark.parametrize("kind", ["spread", "near"])
def test_honest_fp32_passes_the_mantissa_verdict(kind):
    wins = K.mantissa_windows(kind)
    K.mantissa_conditions(K.stitch64(K.H, K.W, wins, K.OV), kind)
    for contract, reverse in HONEST:
        _, after = K.stitch32(K.H, K.W, wins, K.OV, contract=contract, reverse=reverse)
        fails, reports = K.mantissa_verdict(after, wins, kind)
        print(f"contract {contract} reverse {reverse}:", *reports, sep="\n  ")
        assert fails == []


# ---- planted defects ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect,M", [("extents_swapped", 2), ("no_top_left_clip", 2), ("bottom_off_by_one", 2), ("count_plus_one", 2),
                                      ("c_ge_1", 1), ("n_for_n_minus_1", 2), ("member_dropped", 2), ("member_dropped", 4)])
def test_planted_stitcher_defects_fail_the_exact_verdict(defect, M):
    wins = K.exact_windows(M)
    for contract in (False, True):
        before, after = K.stitch32(K.H, K.W, wins, K.OV, contract=contract, defects=(defect,))
        fails = K.exact_verdict(before, after, wins)
        print(defect, fails)
        assert fails


@pytest.mark.parametrize("kind", ["spread", "near"])
@pytest.mark.parametrize("defect", ["extents_swapped", "no_top_left_clip", "bottom_off_by_one", "count_plus_one", "member_dropped"])
def test_planted_stitcher_defects_fail_the_mantissa_verdict(defect, kind):
    wins = K.mantissa_windows(kind)
    _, after = K.stitch32(K.H, K.W, wins, K.OV, contract=True, defects=(defect,))
    assert K.mantissa_verdict(after, wins, kind)[0]


def test_planted_divisor_defect_fails_the_spread_verdict():
    """``n`` for ``n - 1`` moves (c - 1) std^2 by a factor (c - 1) / c: visible wherever the variance stands clear of the bar (the spread
    input: 90 % of the pixels by its condition); on the near-constant input the variance is noise and only the exact input sees it."""
    wins = K.mantissa_windows("spread")
    _, after = K.stitch32(K.H, K.W, wins, K.OV, contract=True, defects=("n_for_n_minus_1",))
    assert K.mantissa_verdict(after, wins, "spread")[0]


@pytest.mark.parametrize("num_ids", [1, 4096, 4097])
def test_planted_segment_defects_change_the_exact_sums(num_ids):
    for n in (1, 2, 3, 5, 4099, 20001):
        pred, ids = K.segment_case(num_ids, n)
        assert all((ids == v).any() for v in (-1, num_ids)) or n < 5
        # (what is shown: the sums of the GPU file's inputs CHANGE when the last n % 4 elements of the view, or the id num_ids, are
        # mishandled, so an equality test cannot pass such a result.  This does not model the kernel's own split into a scalar head
        # up to pred's 16-byte boundary, 16-byte body and scalar tail, which depends on the address.  The GPU file runs every phase:
        # one phase that sees the loss rejects it.)
        seen = []
        for p in range(4):
            want = K.segment64(pred[p:p + n], ids[p:p + n], num_ids)
            lost = K.segment64(pred[p:p + n], ids[p:p + n], num_ids, defects=("tail_lost",))
            seen.append(not np.array_equal(want[1], lost[1]))
        assert any(seen) or n % 4 == 0, (n, seen)
        if n >= 64:
            assert all((ids[:n] == v).any() for v in (-1, K.INT_MIN, K.INT_MAX, num_ids))
            want = K.segment64(pred[:n], ids[:n], num_ids)
            more = K.segment64(pred[:n], ids[:n], num_ids, defects=("id_num_ids_counted",))
            assert not np.array_equal(want[1], more[1]) and not np.array_equal(want[0], more[0])


@pytest.mark.parametrize("nwin,w", [(1024, 5), (1025, 5), (1025, 1030), (2049, 1023)])
def test_dropping_a_window_at_the_batch_edge_changes_the_visit_count(nwin, w):
    """the rows the KERNEL receives (kernel_rows: the host drops windows that begin at or beyond the last row / column) are exactly nwin;
    losing row 1023 (last slot of the first LDS batch), row 1024 (the window 1025 of the issue: first of the second batch) or row 2048
    (the third batch) changes the count, rows 1023 / 1024 at a pixel nothing else covers"""
    wins = K.count_case(nwin, 9, w)
    rows = K.kernel_rows(wins, 9, w)
    assert len(rows) == nwin < len(wins)
    full = K.count64(9, w, wins, 3, K.COUNT_PS, K.COUNT_OV)
    assert np.array_equal(full, K.count64(9, w, rows, 3, K.COUNT_PS, K.COUNT_OV))
    for k, pixel in ((K.CW_CAP - 1, (8, 0)), (K.CW_CAP, (8, w - 1)), (2 * K.CW_CAP, None)):
        if k < nwin:
            less = K.count64(9, w, rows[:k] + rows[k + 1:], 3, K.COUNT_PS, K.COUNT_OV)
            assert not np.array_equal(full, less)
            assert pixel is None or (full[pixel] == 3 and less[pixel] == 0)
    assert full.max() <= 32767


# ---- the Python form of the visit count and the refusal -------------------------------------------------------------------------------------
def test_add_count_only_clamps_a_negative_origin():
    """Stitcher.add_count_only on a host count map (the method touches nothing but ``count``, ``h``, ``w``): windows above / left of the
    raster used to wrap through a negative slice start"""
    from popcorn_amd.eval import Stitcher
    h, w = 9, 11
    wins = K.count_case(300, h, w)
    assert any(x + K.COUNT_OV < 0 < x + K.COUNT_PS - K.COUNT_OV for x, _ in wins) and any(y + K.COUNT_OV < 0 < y + K.COUNT_PS - K.COUNT_OV for _, y in wins)
    st = types.SimpleNamespace(count=torch.zeros(h, w, dtype=torch.int16), h=h, w=w)
    for x, y in wins:
        Stitcher.add_count_only(st, x, y, 3, K.COUNT_PS, K.COUNT_OV)
    assert np.array_equal(st.count.numpy().astype(np.int64), K.count64(h, w, wins, 3, K.COUNT_PS, K.COUNT_OV))


class _NeverRun(torch.nn.Module):
    def parameters(self, recurse=True):
        raise AssertionError("evaluate_raster looked for a device before it refused the raster")

    def forward(self, *a, **k):
        raise AssertionError("evaluate_raster ran the model before it refused the raster")


@pytest.mark.parametrize("hw", [(30, 50), (50, 30), (31, 31)])
def test_raster_smaller_than_the_patch_is_refused_before_any_device_call(hw):
    from popcorn_amd import eval as E
    h, w = hw
    with pytest.raises(ValueError) as e:
        E.evaluate_raster([_NeverRun()], torch.zeros(1, 6, h, w), patchsize=32, overlap=4)
    assert all(s in str(e.value) for s in (f"h {h}", f"w {w}", "patchsize 32"))
    raster = types.SimpleNamespace(shape=(h, w))
    with pytest.raises(ValueError):
        E.evaluate_raster([_NeverRun()], raster, patchsize=32, overlap=4)
    E.require_raster_fits(32, 32, 32, "ok")                             # a raster of exactly one patch is defined


def test_run_eval_refuses_a_raster_smaller_than_the_patch():
    from popcorn_amd.cli import check_eval_args, eval_parser
    check_eval_args(eval_parser().parse_args("--raster_hw 300 420 --patchsize 128".split()))
    with pytest.raises(SystemExit) as e:
        check_eval_args(eval_parser().parse_args("--raster_hw 300 100 --patchsize 128".split()))
    assert "patchsize 128" in str(e.value) and "300 100" in str(e.value)
