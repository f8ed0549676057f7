"""Census table, the parts that need no GPU: the run_eval flags, the float64 yardstick of tests/census_oracle.py against a brute-force
per-unit loop and against the reference's own census sums (fixture g9), and the fixed-point error bar restated in numpy."""
import os

import numpy as np
import torch

from tests import census_oracle as CO

G = os.path.join(os.path.dirname(__file__), "golden")


def test_eval_parser_census_flags():
    from popcorn_amd.cli import eval_parser
    a = eval_parser().parse_args([])
    assert a.census_table is False and a.census_out is None and a.census_details is False
    a = eval_parser().parse_args("--census_table --census_out c.pt --census_details".split())
    assert a.census_table is True and a.census_out == "c.pt" and a.census_details is True


def test_binding_constants_follow_the_header():
    import re
    from popcorn_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "popcorn_hip.h")).read()
    for name in ("PC_CENSUS_MAX_LEVELS", "PC_CENSUS_FIX_SHIFT", "PC_CENSUS_MAX_PLANES"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(L, name)
    assert 2.0 ** L.PC_CENSUS_FIX_SHIFT == CO.FIX
    lib = L.lib()
    assert all(hasattr(lib, n) for n in ("pc_census_accumulate", "pc_census_finalize", "pc_census_paint"))


def test_oracle_equals_brute_force_per_unit_loop():
    from popcorn_amd.eval import get_patch_indices
    h, w, ps, ov, M = 23, 31, 12, 2, 3
    g = torch.Generator().manual_seed(1)
    wins = [(x, y, torch.rand(M, ps, ps, generator=g).numpy()) for x, y, s in get_patch_indices(h, w, ps, ov, True).tolist()]
    yy, xx = np.mgrid[0:h, 0:w]
    blocky = ((yy // 6) * 4 + xx // 9).astype(np.int32)           # 4 x 4 units
    blocky[:3, :5] = -1
    blocky[20:, 28:] = 99                                         # out of range
    salt = ((yy * w + xx) % 7).astype(np.int32)
    num_ids = [17, 7]                                             # id 16 never occurs
    (lv, visits) = CO.table_reference(h, w, wins, ov, [blocky, salt], num_ids)
    inside = lambda x, y, r, c: x + ov <= r < x + ps - ov and y + ov <= c < y + ps - ov  # noqa: E731
    for (totals, n_terms), b, n in zip(lv, (blocky, salt), num_ids):
        want, terms = np.zeros((M, n)), np.zeros(n)
        for r in range(h):
            for c in range(w):
                hits = [(x, y, pd) for x, y, pd in wins if inside(x, y, r, c)]
                assert int(visits[r, c]) == len(hits)
                if 0 <= b[r, c] < n:
                    terms[b[r, c]] += len(hits)
                    for x, y, pd in hits:
                        want[:, b[r, c]] += pd[:, r - x, c - y].astype(np.float64) / len(hits)
        assert totals.shape == (M, n) and totals.dtype == np.float64
        np.testing.assert_allclose(totals, want, rtol=1e-13, atol=0)
        assert np.array_equal(n_terms, terms)
    assert int(visits.max()) == 16 and int(visits.min()) == 0
    assert not lv[0][0][:, 16].any() and lv[0][1][16] == 0
    mean, std = CO.members_mean_std(lv[0][0])
    t = lv[0][0][:, 5]
    m = sum(t.tolist()) / M
    assert abs(mean[5] - m) <= 1e-13 * m
    assert abs(std[5] - (sum((v - m) ** 2 for v in t.tolist()) / (M - 1)) ** 0.5) <= 1e-9 * m


def test_oracle_vs_the_references_census_sums_g9():
    """One window covering the raster, overlap 0: the oracle's unit totals against the reference's own convert_popmap_to_census
    (fixture g9, data/PopulationDataset.py:675-729), which sums each unit in fp32: within n * u * T, n = pixels of the unit."""
    g = np.load(os.path.join(G, "g9_census.npz"))
    for name in ("a", "b"):
        pred, boundary = g[f"{name}/pred"], g[f"{name}/boundary"]
        idx = g[f"{name}/census_idx"]
        assert (pred >= 0).all()
        n = int(max(boundary.max(), idx.max())) + 1
        h, w = pred.shape
        lv, visits = CO.table_reference(h, w, [(0, 0, pred[None])], 0, [boundary], [n])
        assert (visits == 1).all()
        totals, n_terms = lv[0]
        assert np.array_equal(n_terms, CO.pixel_counts(boundary, n))
        ref = g[f"{name}/census_pred"].astype(np.float64)
        got = totals[0][idx]
        assert (np.abs(got - ref) <= n_terms[idx] * CO.U * got + 1e-300).all(), name
        assert np.array_equal(got == 0, ref == 0)


def test_fixed_point_bound():
    """The error bar of tests/census_oracle.py holds for the kernel's arithmetic restated in numpy: 200 random units of 1 .. 2e5 terms,
    scales 1e-6 .. 1e3, visit counts 1 .. 16."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        n = int(10 ** rng.uniform(0, 5.3))
        scale = 10 ** rng.uniform(-6, 3)
        p = (rng.random(n) * scale).astype(np.float32)
        v = rng.choice([1, 2, 4, 8, 16, 3, 5, 7, 9, 11, 13], n)
        t_ref = float((p.astype(np.float64) / v).sum())
        err, b = abs(CO.fixed_point_total(p, v) - t_ref), CO.bar(t_ref, n)
        assert err <= b, (n, scale, err, b)
        worst = max(worst, err / b)
    print(f"worst |T - T_ref| / bar = {worst:.3f}")
    # exact inputs are exact
    p = (16 * rng.integers(0, 16, 1000)).astype(np.float32)
    v = rng.choice([1, 2, 4, 8, 16], 1000)
    assert CO.fixed_point_total(p, v) == float((p.astype(np.float64) / v).sum())


def test_detail_maps_oracle_properties():
    """The restated detail maps on a tiny case by hand: a unit without a census row stays 0, a census row absent from the raster paints
    nothing, POP20 = 0 gives densities_gt = 0 and residuals = pred."""
    b = np.array([[0, 0, 1], [2, 2, 1], [2, 5, -1]], dtype=np.int32)
    pred = np.array([3.0, 4.0, 9.0, 7.0, 1.0, 2.0])
    m = CO.detail_maps(pred, b, [0, 2, 3], [1.0, 0.0, 5.0], pred_std=pred / 2)
    assert m["totals"].tolist() == [[3, 3, 0], [9, 9, 0], [9, 0, 0]]
    assert m["densities"].tolist() == [[1.5, 1.5, 0], [3, 3, 0], [3, 0, 0]]
    assert m["densities_gt"].tolist() == [[0.5, 0.5, 0], [0, 0, 0], [0, 0, 0]]
    assert m["residuals"].tolist() == [[2, 2, 0], [9, 9, 0], [9, 0, 0]]
    assert m["residuals_rel"].tolist() == [[1, 1, 0], [3, 3, 0], [3, 0, 0]]
    assert m["totals_std"].tolist() == [[1.5, 1.5, 0], [4.5, 4.5, 0], [4.5, 0, 0]]
