"""Float64 / int64 numpy yardsticks of the adjusted census table (csrc/census_adjust.hip, eval.CensusTable(adjust=...)), shared by
tests/test_census_adjust_cpu.py and tests/test_gpu_census_adjust.py.

  pair_plan             the (unit of l, unit of a) pairs of two id rasters via np.unique over f * num_a + c
  adjusted_from_table   the arithmetic of pc_census_adjust_finalize (include/popcorn_hip.h) restated on an integer table
  adjusted_reference    adjust_map_to_census (data/PopulationDataset.py:843-850) restated as a loop over the census rows on float64 member
                        maps (tests/census_oracle.member_maps), then float64 unit sums at level l

Derived error bars (nothing here is measured).  ``bar`` is tests/census_oracle.bar: |T - T_ref| <= u T_ref + n_terms 2^-31 + 2^-52 T_ref.

(a) Pair columns of the table: BIT-EQUAL to the integer restatement (fp32 quotient, rint onto the 2^-30 grid, int64 sum): the pair plane
    is one more level of pc_census_accumulate, whose sums are integers.

(b) adj against adjusted_from_table, same integer table: relative error <= 2^-50.  All terms are non-negative, so relative errors do not
    grow in the sum.  A term pair_k * factor carries at most three roundings of 2^-53 (the conversion of P or of pair_k where an integer
    exceeds 2^53 -- both cannot matter at once below 2^-106 --, the division, the product; the scalings by 2^-30 are exact, and so is
    pop * M: 24 bits times a small integer), the sum of <= 5 terms at most four more, the division by M of row M one more:
    (1 + 2^-53)^8 - 1 < 2^-50.

(c) adj against adjusted_reference, to first order.  With s_c the float64 factor POP_c / P_c (1 where the unit is not scaled), S_fc the
    joint sum of (f, c) with n_fc terms, P_c with n_c terms and rem with n_rem terms:
        |A_f - A_ref_f| <= bar(rem, n_rem) + sum_c s_c bar(S_fc, n_fc) + sum_c s_c S_fc bar(P_c, n_c) / P_c + 2^-49 A_f
    (the table's error in rem, in each joint sum, in each factor's denominator -- d(1 / P) = dP / P^2 --, and the float64 roundings of
    both sides: (b) and the reference's own sums).  Second order: the relative error of a factor is e_c = bar(P_c) / P_c <= u + 2^-52 +
    n_c 2^-31 / P_c, and what first order leaves out is below e_c times the first-order term.  The tests check ``second_order_ok``,
    e_c <= 2^-11, for every scaled unit (inputs chosen with P_c >= 1 and n_c < 2^16 give e_c < 2^-15), and the bound is multiplied by
    1 + 2^-10.
    The ensemble row is the same bound on the mean map: the bar is linear in T, so the mean over members of the members' bars is the bar
    of the mean total with the same n_terms."""
import numpy as np

from tests import census_oracle as CO

SLOTS = 4
FIX = CO.FIX
REL_B = 2.0 ** -50


def second_order_ok(P, n_terms):
    """the condition of bar (c): the relative error bar of every scaled unit's total is at most 2^-11"""
    P, n_terms = np.asarray(P, dtype=np.float64), np.asarray(n_terms, dtype=np.float64)
    return bool((P > 0).all() and (CO.bar(P, n_terms) / P <= 2.0 ** -11).all())


def _valid(b, n):
    b = np.asarray(b).astype(np.int64)
    return b, (b >= 0) & (b < n)


def pair_plan(b_l, b_a, num_l, num_a):
    """Returns (pair_plane int32 like b_l, pair_f (NP,), pair_c (NP,), base (num_l + 1,), partners (num_l, max(SLOTS, most partners)) padded
    with -1, count (num_l,)).  Pairs ordered by (f, c); nothing is capped (a unit with more than SLOTS partners shows in count)."""
    f, okf = _valid(b_l, num_l)
    c, okc = _valid(b_a, num_a)
    ok = okf & okc
    keys, inv = np.unique(f[ok] * num_a + c[ok], return_inverse=True)
    pair_f, pair_c = (keys // num_a).astype(np.int32), (keys % num_a).astype(np.int32)
    plane = np.full(f.shape, -1, dtype=np.int32)
    plane[ok] = inv.astype(np.int32)
    count = np.bincount(pair_f, minlength=num_l).astype(np.int32)
    base = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    partners = np.full((num_l, max(SLOTS, int(count.max()) if count.size else 0)), -1, dtype=np.int32)
    for j, (pf, pc) in enumerate(zip(pair_f, pair_c)):
        partners[pf, j - base[pf]] = pc
    return plane, pair_f, pair_c, base, partners, count


def _factor(pop, has, P, scale):
    """factor of every unit of level a from its integer totals P (num_a,): pop * scale / (P * 2^-30) where has and P > 0, else 1"""
    P = np.asarray(P, dtype=np.int64)
    out = np.ones(P.shape, dtype=np.float64)
    go = (np.asarray(has) != 0) & (P > 0)
    out[go] = (np.asarray(pop, dtype=np.float32).astype(np.float64)[go] * np.float64(scale)) / (P[go].astype(np.float64) / FIX)
    return out


def _adjust_rows(Tl, Tp, Pa, base, pair_c, pop, has, scale):
    """one row: Tl (num_l,), Tp (NP,), Pa (num_a,) int64 -> 2^-30 * (rem + sum_k pair_k * factor[c_k]), k ascending"""
    num_l = Tl.shape[0]
    fac = _factor(pop, has, Pa, scale)
    cnt = np.diff(base)
    rem = Tl.copy()
    for k in range(SLOTS):
        m = cnt > k
        rem[m] -= Tp[base[:-1][m] + k]
    s = rem.astype(np.float64)
    for k in range(SLOTS):
        m = cnt > k
        j = base[:-1][m] + k
        s[m] = s[m] + Tp[j].astype(np.float64) * fac[pair_c[j]]
    assert num_l == s.shape[0]
    return s / FIX


def adjusted_from_table(table, off_l, num_l, off_a, num_a, off_p, base, pair_c, pop, has):
    """table (M, T) int64 -> adj (M + 1, num_l) float64 by the arithmetic of pc_census_adjust_finalize; row M: the ensemble-mean map"""
    table = np.asarray(table, dtype=np.int64)
    M = table.shape[0]
    base, pair_c = np.asarray(base, dtype=np.int64), np.asarray(pair_c, dtype=np.int64)
    npairs = int(base[-1])
    rows = [_adjust_rows(t[off_l:off_l + num_l], t[off_p:off_p + npairs], t[off_a:off_a + num_a], base, pair_c, pop, has, 1.0)
            for t in table]
    t = table.sum(0)
    rows.append(_adjust_rows(t[off_l:off_l + num_l], t[off_p:off_p + npairs], t[off_a:off_a + num_a], base, pair_c, pop, has, float(M))
                / np.float64(M))
    return np.stack(rows)


def adjusted_self_from_table(table, off_a, num_a, pop, has):
    """level a judged on itself: pop where the unit is scaled, P * 2^-30 where not; row M with the sums over members (/ M where unscaled)"""
    table = np.asarray(table, dtype=np.int64)
    M = table.shape[0]
    popd = np.asarray(pop, dtype=np.float32).astype(np.float64)
    rows = []
    for t, div in [(r, 1.0) for r in table] + [(table.sum(0), float(M))]:
        P = t[off_a:off_a + num_a]
        rows.append(np.where((np.asarray(has) != 0) & (P > 0), popd, P.astype(np.float64) / FIX / div))
    return np.stack(rows)


def adjust_map(pred, b_a, census_idx, census_pop):
    """data/PopulationDataset.py:843-850 on a float64 map: for every census row, scale the pixels of its unit by POP / their sum, unless
    the sum is 0.  Returns (adjusted copy, {cidx: factor})."""
    pred = np.array(pred, dtype=np.float64)
    b_a = np.asarray(b_a)
    fac = {}
    for cidx, pop in zip(census_idx, census_pop):
        mask = b_a == cidx
        s = pred[mask].sum()
        if s == 0:
            continue
        fac[int(cidx)] = np.float64(np.float32(pop)) / s
        pred[mask] *= fac[int(cidx)]
    return pred, fac


def adjusted_reference(maps, b_l, num_l, b_a, census_idx, census_pop):
    """maps (M, h, w) float64 member maps -> (M + 1, num_l): every member's map adjusted on its own and summed over the units of level l;
    row M: the mean map adjusted (what the reference does)."""
    maps = np.asarray(maps, dtype=np.float64)
    rows = [CO.unit_sums(adjust_map(m, b_a, census_idx, census_pop)[0], b_l, num_l) for m in maps]
    rows.append(CO.unit_sums(adjust_map(maps.sum(0) / maps.shape[0], b_a, census_idx, census_pop)[0], b_l, num_l))
    return np.stack(rows)


def bound_c(pred, visits, b_l, num_l, b_a, num_a, census_idx, census_pop):
    """bar (c) of the module docstring for ONE float64 map (a member's, or the mean map): (num_l,) bound on |A - A_ref|"""
    pred = np.asarray(pred, dtype=np.float64)
    plane, pair_f, pair_c, base, _, _ = pair_plan(b_l, b_a, num_l, num_a)
    npairs = max(1, len(pair_f))
    S, nS = CO.unit_sums(pred, plane, npairs), CO.unit_sums(visits, plane, npairs)
    P, nP = CO.unit_sums(pred, b_a, num_a), CO.unit_sums(visits, b_a, num_a)
    outside = (plane < 0)
    rem, nrem = CO.unit_sums(pred * outside, b_l, num_l), CO.unit_sums(np.asarray(visits) * outside, b_l, num_l)
    s, scaled = np.ones(num_a), np.zeros(num_a, dtype=bool)
    for cidx, pop in zip(census_idx, census_pop):
        if 0 <= cidx < num_a and P[cidx] > 0:
            s[cidx], scaled[cidx] = np.float64(np.float32(pop)) / P[cidx], True
    out = CO.bar(rem, nrem)
    A = rem.copy()
    for j, (f, c) in enumerate(zip(pair_f, pair_c)):
        out[f] += s[c] * CO.bar(S[j], nS[j])
        if scaled[c]:
            out[f] += s[c] * S[j] * CO.bar(P[c], nP[c]) / P[c]
        A[f] += s[c] * S[j]
    return (out + 2.0 ** -49 * A) * (1 + 2.0 ** -10)
