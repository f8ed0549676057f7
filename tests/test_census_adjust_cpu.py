"""The adjusted census table, the parts that need no GPU: the numpy yardsticks of tests/census_adjust_oracle.py against answers worked
out by hand, the two-level SyntheticTestRaster, the two C entry points (exported, refusing bad arguments) and the run_eval flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import census_adjust_oracle as AO
from tests import census_oracle as CO

FIX = 1 << 30


# ---- the hand-computed case ------------------------------------------------------------------------------------------------------------
# 4 x 6 raster.  Level a (coarse): unit 0 = columns 0-1, unit 1 = columns 2-3, unit 2 = column 4, unit 3 = rows 0-1 of column 5, unit 4
# nowhere (P = 0); rows 2-3 of column 5: -1.  Level l (fine): unit 0 = columns 0-1 (nested in coarse 0), unit 1 = columns 2-4 of rows
# 0-1 (STRADDLES coarse 1 and 2), unit 2 = columns 2-3 of rows 2-3 (nested in coarse 1), unit 3 = column 5 (coarse 3 and no unit), unit 4
# nowhere; column 4 of rows 2-3: fine -1.
B_A = np.array([[0, 0, 1, 1, 2, 3],
                [0, 0, 1, 1, 2, 3],
                [0, 0, 1, 1, 2, -1],
                [0, 0, 1, 1, 2, -1]], dtype=np.int32)
B_L = np.array([[0, 0, 1, 1, 1, 3],
                [0, 0, 1, 1, 1, 3],
                [0, 0, 2, 2, -1, 3],
                [0, 0, 2, 2, -1, 3]], dtype=np.int32)
# the map: 1 everywhere, 3 in column 4, 2 in column 5
PRED = np.ones((4, 6))
PRED[:, 4] = 3
PRED[:, 5] = 2
# census of level a: unit 0 -> 16 (P = 8, factor 2); unit 1 -> 0 (POP = 0: factor 0); unit 2 -> 6 (P = 12, factor 1/2); unit 3: NO row
# (never scaled); unit 4 -> 5 (P = 0: skipped)
C_IDX, C_POP = [0, 1, 2, 4], [16.0, 0.0, 6.0, 5.0]
# fine unit 0: 8 * 2 = 16; unit 1: 4 pixels of coarse 1 * 0 + 2 pixels (value 3) of coarse 2 * 1/2 = 3; unit 2: 4 * 0 = 0;
# unit 3: rows 0-1 in coarse 3 unscaled (2 + 2) + rows 2-3 in no coarse unit (2 + 2) = 8; unit 4: 0
WANT = [16.0, 3.0, 0.0, 8.0, 0.0]


def test_pair_plan_by_hand():
    plane, pf, pc, base, partners, count = AO.pair_plan(B_L, B_A, 5, 5)
    assert pf.tolist() == [0, 1, 1, 2, 3] and pc.tolist() == [0, 1, 2, 1, 3]
    assert base.tolist() == [0, 1, 3, 4, 5, 5] and count.tolist() == [1, 2, 1, 1, 0]
    assert partners.tolist() == [[0, -1, -1, -1], [1, 2, -1, -1], [1, -1, -1, -1], [3, -1, -1, -1], [-1, -1, -1, -1]]
    assert plane.tolist() == [[0, 0, 1, 1, 2, 4], [0, 0, 1, 1, 2, 4], [0, 0, 3, 3, -1, -1], [0, 0, 3, 3, -1, -1]]
    # ids outside [0, num): no unit
    plane2 = AO.pair_plan(B_L, B_A, 3, 2)[0]
    assert plane2.tolist() == [[0, 0, 1, 1, -1, -1], [0, 0, 1, 1, -1, -1], [0, 0, 2, 2, -1, -1], [0, 0, 2, 2, -1, -1]]


def _table_of(maps):
    """the integer table [fine | coarse | pairs] of exact maps (visit count 1)"""
    plane, pf, pc, base, _, _ = AO.pair_plan(B_L, B_A, 5, 5)
    rows = []
    for m in maps:
        fix = np.rint(m * FIX).astype(np.int64)
        rows.append(np.array([fix[b == i].sum() for b in (B_L, B_A, plane) for i in range(5)], dtype=np.int64))
    return np.stack(rows), base, pc


def test_adjusted_reference_and_from_table_by_hand():
    """The straddling unit, POP = 0, a unit without a census row, a unit with P = 0: both yardsticks give the hand-computed totals, for
    a member and for the ensemble row."""
    ref = AO.adjusted_reference(PRED[None], B_L, 5, B_A, C_IDX, C_POP)
    assert ref.shape == (2, 5) and ref[0].tolist() == WANT and ref[1].tolist() == WANT
    table, base, pc = _table_of([PRED])
    assert table[0].tolist()[:10] == [8 * FIX, 10 * FIX, 4 * FIX, 8 * FIX, 0, 8 * FIX, 8 * FIX, 12 * FIX, 4 * FIX, 0]
    pop, has = np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.uint8)
    pop[C_IDX], has[C_IDX] = C_POP, 1
    adj = AO.adjusted_from_table(table, 0, 5, 5, 5, 10, base, pc, pop, has)
    assert adj.tolist() == [WANT, WANT]
    self_adj = AO.adjusted_self_from_table(table, 5, 5, pop, has)
    assert self_adj.tolist() == [[16.0, 0.0, 6.0, 4.0, 0.0]] * 2            # pop where scaled; P where not (no row; P = 0)
    # the level sums are kept where every unit is nested and scaled: fine unit 0 <-> coarse unit 0
    assert adj[0][0] == pop[0]


def test_ensemble_row_is_the_adjusted_mean_map_not_the_members_mean():
    """Two members, the second 3 x the first on coarse unit 0 only: the factors differ, so the adjusted mean map is not the mean of the
    adjusted member maps on the straddling unit; both yardsticks agree on each."""
    second = PRED.copy()
    second[:, 4] *= 5                                                  # coarse 2: P = 12 and 60 -> factors 1/2 and 1/10; mean map: 36 -> 1/6
    maps = np.stack([PRED, second])
    ref = AO.adjusted_reference(maps, B_L, 5, B_A, C_IDX, C_POP)
    assert ref[0][1] == 3.0 and ref[1][1] == 3.0 and ref[2][1] == 3.0   # unit 1 holds half of coarse 2 whatever the member: POP / 2
    third = PRED.copy()
    third[:2, 4] *= 5                                                  # only the half INSIDE fine unit 1: shares 1/2 and 5/6
    maps = np.stack([PRED, third])
    ref = AO.adjusted_reference(maps, B_L, 5, B_A, C_IDX, C_POP)
    np.testing.assert_allclose(ref[:, 1], [3.0, 5.0, 6 * 18 / 24], rtol=1e-15)        # mean map: (3 + 15) / 2 * 2 of 24 -> 6 * 18 / 24 = 4.5
    assert ref[2][1] != ref[:2, 1].mean()
    table, base, pc = _table_of(maps)
    pop, has = np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.uint8)
    pop[C_IDX], has[C_IDX] = C_POP, 1
    adj = AO.adjusted_from_table(table, 0, 5, 5, 5, 10, base, pc, pop, has)
    np.testing.assert_allclose(adj, ref, rtol=AO.REL_B + 2.0 ** -50, atol=0)


def test_bound_c_terms_by_hand():
    """bar (c) on the hand case: unit 0 (nested, factor 2, 8 terms): 2 * bar(8, 8) + 2 * 8 * bar(8, 8) / 8 + 2^-49 * 16."""
    b = AO.bound_c(PRED, np.ones((4, 6)), B_L, 5, B_A, 5, C_IDX, C_POP)
    want = (4 * CO.bar(8.0, 8) + 2.0 ** -49 * 16) * (1 + 2.0 ** -10)
    assert abs(b[0] - want) <= 1e-15 * want
    # unit 3: 4 in coarse 3 (no row: s = 1, no denominator term), 4 outside every coarse unit
    want3 = (CO.bar(4.0, 2) + CO.bar(4.0, 2) + 2.0 ** -49 * 8) * (1 + 2.0 ** -10)
    assert abs(b[3] - want3) <= 1e-15 * want3


# ---- the two-level synthetic raster -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,n,coarse", [((200, 232), 400, 16), ((96, 80), 30, 4), ((64, 64), 400, 7)])
def test_synthetic_raster_coarse_level(hw, n, coarse):
    from popcorn_amd.data.dataset import SyntheticTestRaster
    old = SyntheticTestRaster(hw[0], hw[1], n_regions=n)
    new = SyntheticTestRaster(hw[0], hw[1], n_regions=n, coarse_regions=coarse)
    for k, v in vars(old).items():                     # every old attribute keeps its bits: nothing is drawn from the generator
        w = getattr(new, k)
        assert torch.equal(v, w) if torch.is_tensor(v) else v == w, k
    assert not hasattr(old, "boundary_coarse")
    nc = int(new.census_idx_coarse.max())
    assert new.census_idx_coarse.tolist() == list(range(1, nc + 1)) and 2 <= nc <= 2 * coarse
    assert new.boundary_coarse.dtype == torch.int32 and new.boundary_coarse.shape == new.boundary.shape
    # nesting: every fine unit lies in exactly one coarse unit, 0 exactly where the fine raster is 0
    fine, crs = new.boundary.long().flatten(), new.boundary_coarse.long().flatten()
    assert torch.equal(fine == 0, crs == 0)
    assert torch.equal(new.coarse_of_fine[fine], crs)
    pairs = torch.unique(torch.stack([fine, crs]), dim=1)
    assert pairs.shape[1] == torch.unique(fine).numel()
    # coarse counts: the sums of the member fine counts (float64 sum, rounded once)
    want = torch.zeros(nc + 1, dtype=torch.float64).index_add_(0, new.coarse_of_fine[1:], new.census_pop.double())[1:]
    assert torch.equal(new.census_pop_coarse, want.float()) and new.census_pop_coarse.dtype == torch.float32
    assert abs(float(new.census_pop_coarse.double().sum()) - float(new.census_pop.double().sum())) <= 1e-6 * float(new.census_pop.sum())


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_refuse_bad_arguments():
    """Both entry points are exported, the binding's slot count follows the header, and null or out-of-range arguments are refused with
    PC_EINVAL before anything is launched (the library loads without a GPU)."""
    from popcorn_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "popcorn_hip.h")).read()
    assert int(re.search(r"#define PC_CENSUS_PAIR_SLOTS (\d+)", hdr).group(1)) == L.PC_CENSUS_PAIR_SLOTS == AO.SLOTS
    assert int(re.search(r"#define PC_ABI_VERSION (\d+)", hdr).group(1)) == L.PC_ABI_VERSION == 10
    lib = L.lib()
    assert hasattr(lib, "pc_census_pair_plan") and hasattr(lib, "pc_census_adjust_finalize")
    EINVAL = -1
    buf = (C.c_int32 * 64)()                                  # host memory: never dereferenced, every call below is refused
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    n = C.c_int64(16)
    plan = lib.pc_census_pair_plan
    assert plan(None, p, n, 4, 4, p, p, p, p, None, None, None) == EINVAL
    assert plan(p, None, n, 4, 4, p, p, p, p, None, None, None) == EINVAL
    assert plan(p, p, n, 4, 4, None, p, p, p, None, None, None) == EINVAL
    assert plan(p, p, n, 0, 4, p, p, p, p, None, None, None) == EINVAL
    assert plan(p, p, n, 4, 0, p, p, p, p, None, None, None) == EINVAL
    assert plan(p, p, C.c_int64(-1), 4, 4, p, p, p, p, None, None, None) == EINVAL
    assert plan(p, p, n, 4, 4, p, None, p, p, None, None, None) == EINVAL          # the rounds need count, flags and scratch
    assert plan(p, p, n, 4, 4, p, p, None, p, None, None, None) == EINVAL
    assert plan(p, p, n, 4, 4, p, p, p, None, None, None, None) == EINVAL
    assert plan(p, p, n, 4, 4, p, None, None, None, None, p, None) == EINVAL       # the write pass needs base
    assert plan(odd, p, n, 4, 4, p, p, p, p, None, None, None) == EINVAL           # 4-byte alignment of the planes
    fin = lib.pc_census_adjust_finalize
    ok = dict(table=p, M=2, T=C.c_int64(30), off_l=C.c_int64(0), off_a=C.c_int64(10), off_p=C.c_int64(15), num_l=10, num_a=5,
              num_p=C.c_int64(15), base=p, pair_c=p, pop=p, has=p, adj=p, mean=p, std=p, stream=None)
    for bad in (dict(table=None), dict(pop=None), dict(has=None), dict(adj=None), dict(mean=None), dict(std=None), dict(pair_c=None),
                dict(M=0), dict(T=C.c_int64(0)), dict(num_l=0), dict(num_a=0), dict(off_l=C.c_int64(-1)), dict(off_l=C.c_int64(21)),
                dict(off_a=C.c_int64(26)), dict(off_p=C.c_int64(16)), dict(num_p=C.c_int64(-1)), dict(off_p=C.c_int64(-1)),
                dict(base=None), dict(base=None, num_l=5, off_l=C.c_int64(0))):
        assert fin(*{**ok, **bad}.values()) == EINVAL, bad


# ---- run_eval ------------------------------------------------------------------------------------------------------------------------------
def test_check_eval_args_coarse_regions():
    from popcorn_amd.cli import check_eval_args, eval_parser
    a = eval_parser().parse_args([])
    assert a.coarse_regions == 0
    check_eval_args(a)
    check_eval_args(eval_parser().parse_args("--coarse_regions 2".split()))
    check_eval_args(eval_parser().parse_args("--coarse_regions 399 --census_table".split()))
    for bad in ("1", "-3", "400", "5000"):
        with pytest.raises(SystemExit, match="coarse_regions"):
            check_eval_args(eval_parser().parse_args(["--coarse_regions", bad]))
