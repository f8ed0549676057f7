"""The adjusted census table (csrc/census_adjust.hip, ops.census_pair_plan, eval.CensusTable(adjust=...)): the dasymetric adjustment to
the census of one level judged on another, per member, from one pass over the windows -- against the numpy yardsticks of
tests/census_adjust_oracle.py, whose docstring derives the bars (a) bit-equal pair columns, (b) 2^-50 against the arithmetic restated on
the same integer table, (c) first-order against adjust_map_to_census restated on float64 member maps."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import census_adjust_oracle as AO
from tests import census_oracle as CO

pytestmark = pytest.mark.gpu
U = CO.U
INT32_MAX = 2 ** 31 - 1
SH, SW = 37, 53                 # the small raster
TH, TW = 70, 300                # the table's raster: more than 256 columns and more than 32 rows give several accumulate tiles


# ---- 1. the plan ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plan_case():
    """(b_l, b_a, num_l, num_a) on 37 x 53.  Level a: a 3 x 3 grid of 13 x 18 blocks, ids 1 .. 9 (1-based as the rasters on disk: id 0 is
    a valid unit that never has a census row), with patches of 0, -1, num_a and INT32_MAX.  Level l, -1 where nothing is said:
      unit 0  nested in one block                                 1 partner
      unit 1  across a vertical block edge                        2 partners
      unit 2  around a block corner                               4 partners
      unit 3  an L across a horizontal edge and a vertical one    3 partners
      unit 4  two separate blobs inside the same block            1 partner, met twice
      units 5, 6, 8  partly over the -1 patch, the num_a patch and the INT32_MAX patch: pixels of a fine unit in no coarse unit, 1 partner
      unit 7  over the 0 patch and a block                        2 partners, one of them unit 0
      unit 9  wholly inside the -1 patch                          no partner
      unit 13 has no pixel; a patch of num_l and one of INT32_MAX: no fine unit (over valid coarse pixels, and over invalid ones)."""
    yy, xx = np.mgrid[0:SH, 0:SW]
    b_a = (1 + (yy // 13) * 3 + xx // 18).astype(np.int32)
    b_a[0:4, 0:6] = -1
    b_a[5:8, 20:30] = 0
    b_a[30:37, 45:53] = 10
    b_a[20:23, 0:5] = INT32_MAX
    b_l = np.full((SH, SW), -1, dtype=np.int32)
    b_l[4:7, 8:17] = 0
    b_l[10:16, 15:21] = 2
    b_l[8:12, 14:22] = 1
    b_l[24:29, 30:36] = 3
    b_l[24:26, 36:39] = 3
    b_l[0:4, 40:45] = 4
    b_l[8:12, 46:51] = 4
    b_l[0:7, 0:8] = 5
    b_l[31:37, 40:53] = 6
    b_l[4:10, 24:29] = 7
    b_l[19:24, 0:9] = 8
    b_l[0:3, 0:3] = 9
    b_l[15:18, 30:34] = 14                     # num_l: no unit, over block pixels
    b_l[32:35, 47:50] = INT32_MAX              # no fine unit over no coarse unit
    b_l[21:22, 1:3] = -1                       # both invalid (coarse INT32_MAX)
    return b_l, b_a, 14, 10


def _gpu_plan(b_l, b_a, num_l, num_a):
    from popcorn_amd import ops
    return ops.census_pair_plan(torch.from_numpy(b_l).cuda(), torch.from_numpy(b_a).cuda(), num_l, num_a)


def _same_plan(got, want):
    plane, pf, pc, base = (t.cpu().numpy() for t in got)
    assert plane.dtype == pf.dtype == pc.dtype == base.dtype == np.int32
    assert np.array_equal(plane, want[0]) and np.array_equal(pf, want[1]) and np.array_equal(pc, want[2]) and np.array_equal(base, want[3])


def test_plan_equals_the_oracle_bit_for_bit():
    b_l, b_a, num_l, num_a = _plan_case()
    want = AO.pair_plan(b_l, b_a, num_l, num_a)
    # the designed cases are there (numpy, no device): partner counts per unit, nothing above four
    assert want[5].tolist() == [1, 2, 4, 3, 1, 1, 1, 2, 1, 0, 0, 0, 0, 0]
    assert want[4][7].tolist() == [0, 2, -1, -1] and want[4][2].tolist() == [1, 2, 4, 5] and int(want[5].max()) == AO.SLOTS
    okl, oka = (b_l >= 0) & (b_l < num_l), (b_a >= 0) & (b_a < num_a)
    assert (okl & ~oka).any() and (~okl & oka).any() and (~okl & ~oka).any() and (want[0][okl & oka] >= 0).all()
    got = _gpu_plan(b_l, b_a, num_l, num_a)
    _same_plan(got, want)
    again = _gpu_plan(b_l, b_a, num_l, num_a)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    # the roles swapped (level a judged, adjusted to level l): another plan of the same rasters
    _same_plan(_gpu_plan(b_a, b_l, num_a, num_l), AO.pair_plan(b_a, b_l, num_a, num_l))


def test_plan_of_a_row_band_at_a_4_byte_aligned_offset():
    """The planes as a row band of a larger raster: 53 columns, so rows 1, 2 and 3 start on 4-byte boundaries only, and the two planes and
    the pair plane get different 16-byte phases (the second raster starts one element later)."""
    from popcorn_amd import ops
    b_l, b_a, num_l, num_a = _plan_case()
    big_l = torch.full((SH + 4, SW), -1, dtype=torch.int32, device="cuda")
    big_a = torch.full(((SH + 4) * SW + 1,), -1, dtype=torch.int32, device="cuda")[1:].view(SH + 4, SW)
    for r0 in (1, 2, 3):
        big_l[r0:r0 + SH] = torch.from_numpy(b_l).cuda()
        big_a[r0:r0 + SH] = torch.from_numpy(b_a).cuda()
        assert big_l[r0:].data_ptr() % 16 != 0 and big_l[r0:].data_ptr() % 16 != big_a[r0:].data_ptr() % 16
        for rows in (SH, 1, 2):
            want = AO.pair_plan(b_l[:rows], b_a[:rows], num_l, num_a)
            _same_plan(ops.census_pair_plan(big_l[r0:r0 + rows], big_a[r0:r0 + rows], num_l, num_a), want)


def test_plan_of_a_level_with_more_ids_than_the_lds_table():
    """9000 ids of level l (the round kernel's LDS table holds 8192): the minima go to the global table directly.  70 x 300, units of 1 x 3
    pixels numbered with a stride, against blocks of 7 x 11: up to two partners."""
    yy, xx = np.mgrid[0:TH, 0:TW]
    b_l = (((yy * 100 + xx // 3) * 7919) % 9000).astype(np.int32)
    b_a = ((yy // 7) * 28 + xx // 11).astype(np.int32)
    want = AO.pair_plan(b_l, b_a, 9000, 280)
    assert 2 <= int(want[5].max()) <= AO.SLOTS and int((want[5] > 0).sum()) > 6000
    _same_plan(_gpu_plan(b_l, b_a, 9000, 280), want)
    # and the small-id path on the same coarse raster, the levels swapped: 280 units of level l with many partners each is refused
    with pytest.raises(ValueError, match="unit 0 "):
        _gpu_plan(b_a, b_l, 280, 9000)


def test_a_unit_with_five_partners_raises_and_names_the_smallest():
    """Units 2 and 8 stretched over five and six blocks: the plan is refused and names unit 2; every output of the call stays inside its
    guard bands."""
    from popcorn_amd import ops
    from tests.footprint import Footprint, POISON
    b_l, b_a, num_l, num_a = _plan_case()
    b_l = b_l.copy()
    b_l[16:28, 15:21] = 2                       # unit 2: blocks 1, 2, 4, 5 and now 7, 8
    b_l[24:30, 0:40][b_l[24:30, 0:40] == -1] = 8
    count = AO.pair_plan(b_l, b_a, num_l, num_a)[5]
    assert [i for i, n in enumerate(count.tolist()) if n > AO.SLOTS] == [2, 8]
    with Footprint("cuda", fill=POISON) as fp:
        tl, ta = fp.place(torch.from_numpy(b_l)), fp.place(torch.from_numpy(b_a))
        with pytest.raises(ValueError, match=r"unit 2 .*more than 4"):
            ops.census_pair_plan(tl, ta, num_l, num_a)
        assert fp.guarded >= 5
    # a plan that succeeds, guarded as well: the write pass and the pair lists
    b_l, b_a, num_l, num_a = _plan_case()
    with Footprint("cuda", fill=POISON) as fp:
        got = ops.census_pair_plan(fp.place(torch.from_numpy(b_l)), fp.place(torch.from_numpy(b_a)), num_l, num_a)
    _same_plan(got, AO.pair_plan(b_l, b_a, num_l, num_a))


# ---- 2. the table with pair columns ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table_levels():
    """70 x 300.  Level a: 35 x 100 blocks, ids 1 .. 6, a strip of 0 (a unit without a census row) and one of -1.  Level l: 8 x 15 blocks
    (9 x 20 = 180 units, ids 0 .. 179): row block 4 straddles the coarse edge at row 35, column blocks 6 and 13 those at columns 100 and
    200, column block 19 the strip of 0 -- units with 0, 1, 2, 3 and 4 partners -- and a strip of -1.  Census of level a: rows for 1, 2, 3, 4, 6 (unit 5: none; unit 3: POP 0)."""
    yy, xx = np.mgrid[0:TH, 0:TW]
    b_a = (1 + (yy // 35) * 3 + xx // 100).astype(np.int32)
    b_a[:, 290:] = 0
    b_a[60:, :20] = -1
    b_l = ((yy // 8) * 20 + xx // 15).astype(np.int32)
    b_l[20:24, 120:170] = -1
    idx = [1, 2, 3, 4, 6]
    pop = np.array([5000.0, 123.456, 0.0, 77777.0, 0.015625], dtype=np.float32)
    return b_l, 180, b_a, 7, idx, pop


@functools.lru_cache(maxsize=None)
def _table_windows(M):
    """Windows over 70 x 300, overlap 4, in the style of test_gpu_census_table._windows (uniform random values): the whole raster once, its
    left half a second time, and two windows over the same 50 x 100 patch inside it: visit counts 0 (the frame), 1, 2 and 4."""
    g = torch.Generator().manual_seed(31)
    geo = [(0, 0, TH, TW), (0, 0, TH, 160), (10, 50, 50, 100), (10, 50, 50, 100)]
    return [(x, y, torch.rand(M, px, py, generator=g)) for x, y, px, py in geo]


@functools.lru_cache(maxsize=None)
def _table_reference(M):
    maps, visits = CO.member_maps(TH, TW, [(x, y, pd.numpy()) for x, y, pd in _table_windows(M)], 4)
    assert set(np.unique(visits).tolist()) == {0, 1, 2, 4}
    return maps, visits


def _adjusted_table(M, order=None, adjust=True, levels=None, wins=None, visits=None, h=TH, w=TW, ov=4):
    from popcorn_amd import eval as E
    b_l, num_l, b_a, num_a, idx, pop = levels or _table_levels()
    wins = wins if wins is not None else _table_windows(M)
    visits = visits if visits is not None else _table_reference(M)[1]
    vis = torch.from_numpy(visits.astype(np.int16)).cuda()
    ct = E.CensusTable(h, w, [torch.from_numpy(b_l), torch.from_numpy(b_a)], [num_l, num_a], M, "cuda", visits=vis,
                       adjust={"level": 1, "census_idx": idx, "census_pop": pop} if adjust else None)
    ct.set_windows([(x, y, 0) for x, y, _ in wins], 0, ov)
    for i in (order if order is not None else range(len(wins))):
        x, y, pd = wins[i]
        ct.add_window(x, y, pd.cuda(), ov)
    ct.finalize()
    return ct


def _integer_table(wins, visits, planes, nums, ov, h, w):
    """the table's arithmetic restated (fp32 quotient, rint onto the 2^-30 grid, int64 sum) for the given planes"""
    M = wins[0][2].shape[0]
    want = np.zeros((M, sum(nums)), dtype=np.int64)
    for x, y, pd in wins:
        x0, x1, y0, y1 = CO.interior(x, y, pd.shape[1], pd.shape[2], ov, h, w)
        q = pd.numpy()[:, x0 - x:x1 - x, y0 - y:y1 - y] / visits[x0:x1, y0:y1].astype(np.float32)
        assert q.dtype == np.float32
        fix = np.rint(q.astype(np.float64) * CO.FIX).astype(np.int64)
        off = 0
        for b, n in zip(planes, nums):
            ids = b[x0:x1, y0:y1].astype(np.int64)
            ok = (ids >= 0) & (ids < n)
            for m in range(M):
                np.add.at(want[m], off + ids[ok], fix[m][ok])
            off += n
    return want


def _check_bars(ct, maps, visits, levels):
    """bars (b) and (c) of every member row and the ensemble row, mean and std of level 0; returns the adjusted rows (M + 1, n)"""
    b_l, num_l, b_a, num_a, idx, pop = levels
    M = ct.members
    members, ens, mean, std = ct.adjusted(0)
    assert members.shape == (M, num_l) and ens.shape == mean.shape == std.shape == (num_l,)
    assert members.dtype == ens.dtype == torch.float64 and mean.dtype == std.dtype == torch.float32
    got = np.concatenate([members.cpu().numpy(), ens.cpu().numpy()[None]])
    pf, pc, _ = ct.pairs(0)
    popt, has = np.zeros(num_a, dtype=np.float32), np.zeros(num_a, dtype=np.uint8)
    popt[idx], has[idx] = pop, 1
    base = ct._pairs[0]["base"].cpu().numpy()
    restated = AO.adjusted_from_table(ct.table.cpu().numpy(), 0, num_l, num_l, num_a, num_l + num_a, base, pc.cpu().numpy(), popt, has)
    rel = np.abs(got - restated) / np.maximum(restated, 1e-300)
    print(f"(b) worst relative error {rel.max():.3e} (bar {AO.REL_B:.3e})")
    assert (np.abs(got - restated) <= AO.REL_B * restated).all()
    ref = AO.adjusted_reference(maps, b_l, num_l, b_a, idx, pop)
    every = list(maps) + [maps.sum(0) / M]
    bounds = np.stack([AO.bound_c(m, visits, b_l, num_l, b_a, num_a, idx, pop) for m in every])
    err = np.abs(got - ref)
    print(f"(c) worst |A - A_ref| / bar = {(err / np.maximum(bounds, 1e-300)).max():.3f}")
    assert (err <= bounds).all() and float(ref.max()) > 0
    rm, rs = CO.members_mean_std(ref[:M])
    top = bounds[:M].max(0)
    assert (np.abs(mean.cpu().numpy() - rm) <= top + U * rm).all()                 # (+ the fp32 rounding of the stored mean)
    assert (np.abs(std.cpu().numpy() - rs) <= 2 * top + U * rs).all()
    return got, ref, bounds


@pytest.mark.parametrize("M", [3, 5])
def test_table_with_pair_columns(M):
    """Bars (a), (b) and (c); the level columns are the bits of a table built without ``adjust``; any window order gives the same table.
    M = 5: a full member pass and a pass of one."""
    levels = _table_levels()
    b_l, num_l, b_a, num_a, idx, pop = levels
    maps, visits = _table_reference(M)
    wins = _table_windows(M)
    ct = _adjusted_table(M)
    plane, pf, pc, base, _, count = AO.pair_plan(b_l, b_a, num_l, num_a)
    assert sorted(set(count.tolist())) == [0, 1, 2, 3, 4] and int(count[0]) == 1
    NP = len(pf)
    assert ct.T == num_l + num_a + NP and ct.table.shape == (M, ct.T) and ct.num_ids == [num_l, num_a] and ct.offsets == [0, num_l]
    # (a) the whole table, pair columns included, bit for bit
    want = _integer_table(wins, visits, [b_l, b_a, plane], [num_l, num_a, NP], 4, TH, TW)
    assert np.array_equal(ct.table.cpu().numpy(), want)
    gf, gc, totals = ct.pairs(0)
    assert np.array_equal(gf.cpu().numpy(), pf) and np.array_equal(gc.cpu().numpy(), pc)
    assert np.array_equal(totals.cpu().numpy(), want[:, num_l + num_a:] / CO.FIX)
    # the levels' columns: the bits of a table without the feature
    plain = _adjusted_table(M, adjust=False)
    assert plain.T == num_l + num_a and torch.equal(plain.table, ct.table[:, :plain.T])
    for l in (0, 1):
        for a, b in zip(plain.level(l), ct.level(l)):
            assert torch.equal(a, b)
    # (b), (c)
    P = CO.unit_sums(maps.min(0), b_a, num_a)[idx]
    assert float(P.min()) >= 1.0 and AO.second_order_ok(P, CO.unit_sums(visits, b_a, num_a)[idx])            # every scaled P_c >= 1
    _check_bars(ct, maps, visits, levels)
    # order
    n = len(wins)
    rev = _adjusted_table(M, order=list(reversed(range(n))))
    shuf = _adjusted_table(M, order=torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist())
    assert torch.equal(ct.table, rev.table) and torch.equal(ct.table, shuf.table)
    for a, b in zip(ct.adjusted(0), rev.adjusted(0)):
        assert torch.equal(a, b)


def test_levels_plus_pair_planes_must_fit_one_pass():
    from popcorn_amd import eval as E
    b_l, num_l, b_a, num_a, idx, pop = _table_levels()
    tb = [torch.from_numpy(b_l), torch.from_numpy(b_a), torch.from_numpy(b_a)]
    with pytest.raises(ValueError, match="pair planes"):
        E.CensusTable(TH, TW, tb, [num_l, num_a, num_a], 1, "cuda", adjust={"level": 1, "census_idx": idx, "census_pop": pop})
    with pytest.raises(ValueError):
        E.CensusTable(TH, TW, tb[:2], [num_l, num_a], 1, "cuda", adjust={"level": 2, "census_idx": idx, "census_pop": pop})
    with pytest.raises(ValueError):
        E.CensusTable(TH, TW, tb[:2], [num_l, num_a], 1, "cuda", adjust={"level": 1, "census_idx": [7], "census_pop": [1.0]})
    with pytest.raises(ValueError):
        E.CensusTable(TH, TW, tb[:2], [num_l, num_a], 1, "cuda").adjusted(0)


# ---- 3. semantics --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nested_case():
    """37 x 53, one window, overlap 0, M = 3.  Level a: the 3 x 3 grid of 13 x 18 blocks, ids 1 .. 9; level l: every block cut into 2 x 2
    nested units, id 4 * c + {0 .. 3}.  Census: unit 1 POP 0; unit 2 no row; unit 3: every member's map is 0 there (P = 0); unit 4: member
    1's map is 0 there (P = 0 for one member only); members are scaled differently from block to block, so their factors differ."""
    yy, xx = np.mgrid[0:SH, 0:SW]
    blk = (yy // 13) * 3 + xx // 18
    b_a = (1 + blk).astype(np.int32)
    b_l = (4 * b_a + ((yy % 13) // 7) * 2 + (xx % 18) // 9).astype(np.int32)
    g = torch.Generator().manual_seed(37)
    pd = torch.rand(3, SH, SW, generator=g) + 0.5
    gain = torch.tensor([[1.0, 2.0, 0.5, 3.0, 1.5, 0.25, 4.0, 1.0, 2.5], [2.0, 0.5, 3.0, 1.0, 0.25, 4.0, 1.0, 2.5, 1.5],
                         [0.5, 3.0, 1.0, 2.0, 4.0, 1.5, 2.5, 0.25, 1.0]])
    pd = pd * gain[:, torch.from_numpy(blk)]
    pd[:, torch.from_numpy(b_a == 3)] = 0.0
    pd[1][torch.from_numpy(b_a == 4)] = 0.0
    idx = [1, 3, 4, 5, 6, 7, 8, 9]
    pop = np.array([0.0, 50.0, 600.0, 1000.0, 12.5, 3333.0, 800.0, 99.0], dtype=np.float32)
    return (b_l, 40, b_a, 10, idx, pop), [(0, 0, pd)]


def test_semantics_of_the_adjustment():
    levels, wins = _nested_case()
    b_l, num_l, b_a, num_a, idx, pop = levels
    maps, visits = CO.member_maps(SH, SW, [(0, 0, wins[0][2].numpy())], 0)
    ct = _adjusted_table(3, levels=levels, wins=wins, visits=visits, h=SH, w=SW, ov=0)
    got, ref, bounds = _check_bars(ct, maps, visits, levels)
    fine_of = lambda c: [4 * c + k for k in range(4)]  # noqa: E731
    popt = dict(zip(idx, pop.tolist()))
    level0 = ct.level(0)[0].cpu().numpy()
    # POP = 0: the unit's fine totals are 0 exactly
    assert not got[:, fine_of(1)].any()
    # no census row: never scaled -- the plain totals
    assert np.array_equal(got[:3, fine_of(2)], level0[:, fine_of(2)]) and float(got[3, fine_of(2)].min()) > 0
    # P = 0 for every member: skipped, the totals stay 0
    assert not got[:, fine_of(3)].any() and not level0[:, fine_of(3)].any()
    # P = 0 for member 1 only: its totals stay 0; the other members and the mean map are scaled to POP
    assert not got[1, fine_of(4)].any() and float(got[0, fine_of(4)].min()) > 0
    # nested and scaled: the fine units of a coarse unit sum to its POP within the sum of their bars
    for c in (4, 5, 6, 7, 8, 9):
        for m in range(4):
            if c == 4 and m == 1:
                continue
            assert abs(got[m, fine_of(c)].sum() - popt[c]) <= bounds[m, fine_of(c)].sum(), (c, m)
    # the ensemble row is the adjusted MEAN MAP, not the mean of the adjusted members: they differ where the factors differ
    members, ens, mean, std = ct.adjusted(0)
    gap = (ens - members.mean(0)).abs().cpu().numpy()
    assert float(gap[fine_of(5)].min()) > 1e-3 * popt[5] / 4 and float(std[fine_of(5)[0]]) > 0
    assert float(np.abs(got[3] - ref[3]).max()) < float(gap.max()) / 1e6            # (and the oracle tells them apart)
    # level a judged on itself: POP where scaled, P where not
    sm, se, smean, sstd = ct.adjusted(1)
    popv, has = np.zeros(num_a, dtype=np.float32), np.zeros(num_a, dtype=np.uint8)
    popv[idx], has[idx] = pop, 1
    want = AO.adjusted_self_from_table(ct.table.cpu().numpy(), num_l, num_a, popv, has)
    assert np.array_equal(np.concatenate([sm.cpu().numpy(), se.cpu().numpy()[None]]), want)
    assert want[0][5] == 1000.0 and want[1][4] == 0.0 and want[3][4] == 600.0 and want[0][2] == ct.level(1)[0][0][2].item()
    assert float(sstd[5]) == 0.0 and float(sstd[4]) > 0 and float(smean[5]) == 1000.0
    # census rows and metrics
    fidx = list(range(4, 40))
    fpop = np.linspace(1.0, 900.0, len(fidx)).astype(np.float32)
    pe, ps, pm, gt = ct.adjusted_census(0, fidx, fpop)
    assert pe.dtype == torch.float32 and pm.shape == (3, 36) and torch.equal(pe, ens[fidx].float()) and torch.equal(ps, std[fidx])
    met = ct.adjusted_metrics(0, fidx, fpop, tag="T")
    plain = ct.metrics(0, fidx, fpop, tag="T")
    assert set(met) == set(plain) and any(met[k] != plain[k] for k in met)
    assert all(k + "_members_mean" in met and met[k + "_members_std"] >= 0 for k in met if "_members_" not in k)


def test_single_member_has_zero_std_and_equals_the_ensemble_row():
    levels, wins = _nested_case()
    one = [(0, 0, wins[0][2][:1].contiguous())]
    visits = np.ones((SH, SW), dtype=np.int64)
    ct = _adjusted_table(1, levels=levels, wins=one, visits=visits, h=SH, w=SW, ov=0)
    members, ens, mean, std = ct.adjusted(0)
    assert torch.equal(members[0], ens) and not bool(std.any()) and torch.equal(mean, ens.float())


@pytest.mark.parametrize("value", [float("nan"), -1.0])
def test_a_bad_value_inside_a_pair_still_raises(value):
    from popcorn_amd._lib import PopcornHipError
    from popcorn_amd import eval as E
    levels, wins = _nested_case()
    b_l, num_l, b_a, num_a, idx, pop = levels
    pd = wins[0][2].clone()
    pd[2, 20, 30] = value
    assert 0 <= b_l[20, 30] < num_l and 0 <= b_a[20, 30] < num_a
    vis = torch.ones(SH, SW, dtype=torch.int16, device="cuda")
    ct = E.CensusTable(SH, SW, [torch.from_numpy(b_l), torch.from_numpy(b_a)], [num_l, num_a], 3, "cuda", visits=vis,
                       adjust={"level": 1, "census_idx": idx, "census_pop": pop})
    ct.set_windows([(0, 0, 0)], SH, 0)
    ct.add_window(0, 0, pd.cuda(), 0)
    with pytest.raises(PopcornHipError):
        ct.finalize()
    with pytest.raises(PopcornHipError):
        ct.adjusted(0)


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------------
def _two_level_raster():
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from tests.test_gpu_product import MH, MW
    return SyntheticTestRaster(MH, MW, n_regions=30, coarse_regions=4)


def _two_level_table(data, M):
    from popcorn_amd import eval as E
    from tests.test_gpu_product import MH, MW
    return E.CensusTable(MH, MW, [data.boundary, data.boundary_coarse], [31, int(data.census_idx_coarse.max()) + 1], M, "cuda",
                         adjust={"level": 1, "census_idx": data.census_idx_coarse, "census_pop": data.census_pop_coarse})


def test_evaluate_raster_adjusted_vs_the_adjusted_mean_map():
    """evaluate_raster(models, raster, census=ct) on a two-level synthetic raster: the ensemble row of ``adjusted(0)`` against
    adjust_map_to_census(stitched mean map, coarse census) followed by census_sums at the fine level.  Bar: (c) on the stitched map, plus
    the map path's own fp32 roundings, relative to A: a pixel of the stitched mean map carries M * V roundings (M * V - 1 accumulations and
    the division, V = the largest visit count), once in the pixel and once more through the factor's denominator; the factor itself three
    (the fp32 total, the division, the product): (2 * M * V + 3) * u * A."""
    from popcorn_amd import eval as E
    from tests.test_gpu_product import MOV, MPS, _members, _raster
    ms, raster, data = _members(), _raster(), _two_level_raster()
    ct = _two_level_table(data, len(ms))
    maps = E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV, census=ct)
    b_l, b_a = data.boundary.numpy(), data.boundary_coarse.numpy()
    num_a = int(data.census_idx_coarse.max()) + 1
    adj = E.adjust_map_to_census(maps[0].clone(), data.boundary_coarse.cuda(), data.census_idx_coarse, data.census_pop_coarse)
    ref = E.census_sums(adj.contiguous(), data.boundary.cuda().contiguous(), 31).cpu().numpy()
    got = ct.adjusted(0)[1].cpu().numpy()
    visits = ct.visits.cpu().numpy()
    mean_map = maps[0].cpu().numpy().astype(np.float64)
    assert AO.second_order_ok(CO.unit_sums(mean_map, b_a, num_a)[1:], CO.unit_sums(visits, b_a, num_a)[1:])
    bars = AO.bound_c(mean_map, visits, b_l, 31, b_a, num_a, data.census_idx_coarse.tolist(), data.census_pop_coarse.tolist())
    bars = bars + (2 * len(ms) * int(visits.max()) + 3) * U * ref
    err = np.abs(got - ref)
    print(f"worst |A(table) - A(map)| / bar = {(err / np.maximum(bars, 1e-300)).max():.3f}")
    assert float(ref[1:].min()) > 0 and (err <= bars).all()
    # the coarse totals of the adjusted fine units are the coarse census
    sums = np.zeros(num_a)
    np.add.at(sums, data.coarse_of_fine.numpy()[1:], got[1:])
    np.testing.assert_allclose(sums[1:], data.census_pop_coarse.numpy(), rtol=1e-5)


def test_run_eval_cli_coarse_regions(capsys, tmp_path):
    """run_eval --coarse_regions: without the flag the printed keys are today's (Main / Adj / Table census of the fine level, nothing
    else); with it the coarse level's Main and Adj keys, a fine Adj number that no longer is exact by construction, and with
    --census_table the table's adjusted fine metrics, within 1e-4 * max(1, |.|) of the map path's (the tolerance
    test_run_eval_cli_census_keys uses between table and map); --census_out gains the adjusted totals and their detail maps."""
    import json
    from popcorn_amd import cli
    base = ("-S2 -NIR -S1 -occmodel -senbuilds -pret --biasinit 0.9407 --raster_hw 200 232 --patchsize 96 --overlap 8 --seed 1600 "
            "--ensemble 2 --census_table")
    off = cli.run_eval(base.split())
    capsys.readouterr()
    tags = lambda res: {k.split("/")[0] for k in res if k != "seconds"}  # noqa: E731
    assert tags(off) == {"Population_MainCensus_synthetic_fine", "Population_AdjCensus_synthetic_fine", "Population_TableCensus_synthetic_fine"}
    path = tmp_path / "census.pt"
    on = cli.run_eval((base + f" --coarse_regions 16 --census_out {path} --census_details").split())
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(printed) == set(on)
    assert tags(on) == tags(off) | {"Population_MainCensus_synthetic_coarse", "Population_AdjCensus_synthetic_coarse",
                                    "Population_TableAdjCensus_synthetic_fine"}
    same = [k for k in off if k != "seconds" and "AdjCensus" not in k]
    assert len(same) > 0 and all(on[k] == off[k] for k in same)
    adj = [k for k in off if k.startswith("Population_AdjCensus_synthetic_fine/")]
    assert len(adj) > 0 and any(on[k] != off[k] for k in adj)
    names = {k.split("/", 1)[1] for k in adj}
    for lvl in ("MainCensus_synthetic_coarse", "AdjCensus_synthetic_coarse"):
        assert {k.split("/", 1)[1] for k in on if k.startswith(f"Population_{lvl}/")} == names
    for k in adj:
        t = k.replace("AdjCensus", "TableAdjCensus")
        assert {t, t + "_members_mean", t + "_members_std"} <= set(on)
        assert abs(on[t] - on[k]) <= 1e-4 * max(1.0, abs(on[k])), (k, on[t], on[k])
        assert on[t + "_members_std"] >= 0
    assert len([k for k in on if k.startswith("Population_TableAdjCensus_synthetic_fine/")]) == 3 * len(adj)
    saved = torch.load(path, weights_only=False)
    assert saved["num_ids"] == [401, 17] and saved["totals"].shape[0] == 2 and saved["totals"].shape[1] == 401 + 17 + 400
    assert saved["adjusted"].shape == saved["adjusted_std"].shape == (401,) and saved["adjusted"].dtype == torch.float64
    assert float(saved["adjusted_std"].max()) > 0
    want = {"densities", "totals", "densities_gt", "totals_gt", "residuals", "residuals_rel", "totals_std"}
    assert set(saved["details"]) == set(saved["details_adj"]) == want
    assert all(v.shape == (200, 232) for v in saved["details_adj"].values())
    assert not torch.equal(saved["details"]["totals"], saved["details_adj"]["totals"])


# ---- 5. two ranks -------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, q):
    import torch.distributed as dist
    from popcorn_amd import eval as E
    from popcorn_amd.distributed import FlatReducer
    from tests.test_gpu_product import MOV, MPS, _members, _raster
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ms = _members()
    ct = _two_level_table(_two_level_raster(), len(ms))
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, reducer=FlatReducer(), rank=rank, census=ct)
    torch.cuda.synchronize()
    q.put((rank, [t.cpu().numpy() for t in (ct.table,) + tuple(ct.adjusted(0)) + tuple(ct.adjusted(1))]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_adjusted_totals_equal_single_process():
    """Two gloo ranks on the one GPU (the process pattern of test_two_ranks_table_equals_single_process): the pair columns ride in the
    table's exact int64 all-reduce, so EVERY rank's table and adjusted totals equal the single-process ones bit for bit."""
    from popcorn_amd import eval as E
    from tests.test_gpu_dp import _free_port, _get
    from tests.test_gpu_product import MOV, MPS, _members, _raster
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ms = _members()
    one = _two_level_table(_two_level_raster(), len(ms))
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, census=one)
    ref = [t.cpu() for t in (one.table,) + tuple(one.adjusted(0)) + tuple(one.adjusted(1))]
    got = dict(_get(q, procs) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(got) == [0, 1] and int(ref[0].sum()) > 0 and float(ref[2].sum()) > 0
    for r in (0, 1):
        for a, want in zip(got[r], ref):
            assert torch.equal(torch.from_numpy(a), want), r
