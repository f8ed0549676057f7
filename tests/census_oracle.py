"""Float64 numpy yardsticks of the census table (csrc/census_table.hip, eval.CensusTable) and of the per-unit detail maps
(eval.census_detail_maps), shared by tests/test_census_table_cpu.py and tests/test_gpu_census_table.py.

The detail maps have NO recorded fixture: the reference's own ``details_to`` branch (data/PopulationDataset.py:731-814) cannot be run to
record one -- it raises inside pandas at :749 (a torch tensor divided by a Series) -- so ``detail_maps`` below is a restatement of
:747-804 in float64 numpy, loop over the census rows included, and the tests compare against it.

Derived error bars of the table (nothing here is measured).  u = 2^-24.  Every term is rounded once by the fp32 division by the visit
count and once to the 2^-30 grid (half a grid step: 2^-31); the integer sum is exact and the conversion of the sum to float64 rounds
once.  Per (member, unit), with n_terms the number of (pixel, window) contributions of the unit:

    |T - T_ref| <= u * T_ref + n_terms * 2^-31 + 2^-52 * T_ref

Mean over members: the same bar taken at the largest member.  (n - 1) standard deviation: 2 x the largest member's bar (it is
sqrt(2)-Lipschitz in a sup-norm perturbation of the member totals; the slack covers its own final rounding)."""
import numpy as np

U = 2.0 ** -24
FIX = 2.0 ** 30


def interior(xl, yl, psx, psy, ov, h, w):
    """rows [x0, x1) x columns [y0, y1) of the interior of the window at row xl, column yl, clipped to the raster"""
    return max(xl + ov, 0), min(xl + psx - ov, h), max(yl + ov, 0), min(yl + psy - ov, w)


def member_maps(h, w, wins, ov):
    """wins: list of (row origin, column origin, popdense (M, psx, psy) array).  The reference's loop (run_eval.py:108-154: interior
    ``+=``, then divide by the visit count) per member in float64.  Returns (maps (M, h, w) float64, visits (h, w) int64)."""
    M = wins[0][2].shape[0]
    maps = np.zeros((M, h, w), dtype=np.float64)
    visits = np.zeros((h, w), dtype=np.int64)
    for xl, yl, pd in wins:
        pd = np.asarray(pd, dtype=np.float64)
        x0, x1, y0, y1 = interior(xl, yl, pd.shape[1], pd.shape[2], ov, h, w)
        if x1 > x0 and y1 > y0:
            maps[:, x0:x1, y0:y1] += pd[:, x0 - xl:x1 - xl, y0 - yl:y1 - yl]
            visits[x0:x1, y0:y1] += 1
    seen = visits > 0
    maps[:, seen] /= visits[seen]
    return maps, visits


def unit_sums(values, boundary, num_ids):
    """sums[id] of ``values`` (h, w) over the pixels with boundary == id, id in [0, num_ids); other ids are ignored"""
    b = np.asarray(boundary).astype(np.int64).ravel()
    ok = (b >= 0) & (b < num_ids)
    return np.bincount(b[ok], weights=np.asarray(values, dtype=np.float64).ravel()[ok], minlength=num_ids)


def table_reference(h, w, wins, ov, boundaries, num_ids):
    """Per level l: (totals (M, num_ids[l]) float64, n_terms (num_ids[l],) = (pixel, window) contributions of each unit); and the visit
    map.  Returns ([(totals, n_terms), ...], visits)."""
    maps, visits = member_maps(h, w, wins, ov)
    out = []
    for b, n in zip(boundaries, num_ids):
        totals = np.stack([unit_sums(maps[m], b, n) for m in range(maps.shape[0])])
        out.append((totals, unit_sums(visits, b, n)))
    return out, visits


def members_mean_std(totals):
    """mean and (n - 1) standard deviation over axis 0 (std 0 for one member)"""
    M = totals.shape[0]
    mean = totals.sum(0) / M
    std = np.sqrt(((totals - mean) ** 2).sum(0) / (M - 1)) if M > 1 else np.zeros_like(mean)
    return mean, std


def bar(t_ref, n_terms):
    """the derived bound on |T - T_ref| of the module docstring"""
    return U * t_ref + n_terms * 2.0 ** -31 + 2.0 ** -52 * t_ref


def fixed_point_total(p, v):
    """The kernel's arithmetic for the terms p (fp32 values) / v (visit counts) of ONE unit: fp32 division, llrint onto the 2^-30 grid,
    exact integer sum, one conversion to float64."""
    q = (np.asarray(p, dtype=np.float32) / np.asarray(v).astype(np.float32)).astype(np.float32)
    return float(np.rint(q.astype(np.float64) * FIX).astype(np.int64).sum()) / FIX


def pixel_counts(boundary, num_ids):
    return unit_sums(np.ones(np.asarray(boundary).shape), boundary, num_ids)


def detail_maps(pred_totals, boundary, census_idx, census_pop, pred_std=None):
    """data/PopulationDataset.py:747-804 restated: pred_totals (num_ids,) predicted total per unit id; the census rows are (census_idx[i],
    census_pop[i]); ``count`` is the pixel count of the unit.  Loop over the census rows as the reference does; values are computed in
    float64 from the fp32 totals / POP20 and stored in fp32 maps.  Pixels of units without a census row stay 0."""
    boundary = np.asarray(boundary)
    num_ids = len(pred_totals)
    count = pixel_counts(boundary, num_ids)
    names = ["densities", "totals", "densities_gt", "totals_gt", "residuals", "residuals_rel"] + (["totals_std"] if pred_std is not None else [])
    maps = {k: np.zeros(boundary.shape, dtype=np.float32) for k in names}
    for i, cidx in enumerate(census_idx):
        pred = np.float64(np.float32(pred_totals[cidx]))                 # census_pred_i[i] (fp32)
        pop = np.float64(np.float32(census_pop[i]))                      # torch.tensor(census["POP20"]).to(torch.float32)
        mask = boundary == cidx
        with np.errstate(divide="ignore", invalid="ignore"):
            maps["densities"][mask] = np.float32(pred / count[cidx])                        # :748-753
            maps["totals"][mask] = np.float32(pred)                                         # :756-761
            maps["densities_gt"][mask] = np.float32(pop / count[cidx])                      # :764-769
            maps["totals_gt"][mask] = np.float32(pop)                                       # :772-777
            res = np.float64(np.float32(pred - pop))
            maps["residuals"][mask] = np.float32(res)                                       # :780-785
            rel = res / count[cidx]                                                         # :798
            maps["residuals_rel"][mask] = np.float32(0.0 if np.isinf(rel) or np.isnan(rel) else rel)   # :799-803
        if pred_std is not None:
            maps["totals_std"][mask] = np.float32(pred_std[cidx])
    return maps
