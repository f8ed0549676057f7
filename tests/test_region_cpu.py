"""The planners of popcorn_amd/data/region.py against the reference's rule (tests/region_oracle.py) and against their stated invariants, on
the host: a blocky 96 x 128 raster of 12 units that touches every raster edge, and an irregular nearest-seed tiling of 24 units plus the
background 0 on 120 x 150 whose bounding boxes overlap.  admin_overlap = 4, K = 4, a budget of 5,200 px: a 2 x 2 group of 32 x 32 blocks
grown by 4 px (at most 72 x 72 = 5,184) fits, a 2 x 3 group (72 x 104) does not."""
import pytest
import torch

from popcorn_amd.data.region import RegionPlan, plan_multi_unit, plan_one_unit
from tests import region_oracle as R

OVERLAP, K, BUDGET = 4, 4, 5200


def _census(n, absent=()):
    ids = torch.tensor(list(range(1, n + 1)) + list(absent))
    pop = torch.rand(ids.numel(), generator=torch.Generator().manual_seed(3)) * 2000
    return ids, pop


RASTERS = {"blocky": (R.blocky_raster, 12), "irregular": (R.irregular_raster, 24)}


@pytest.fixture(scope="module", params=sorted(RASTERS))
def case(request):
    make, n = RASTERS[request.param]
    boundary = make()
    ids, pop = _census(n, absent=(n + 1,))                         # one census row without a pixel in the raster
    table, stray = R.unit_table(boundary, n + 2)
    assert stray == 0
    return request.param, boundary, ids, pop, table


def test_rasters_are_what_the_tests_need():
    t, _ = R.unit_table(R.irregular_raster(), 25)
    assert bool((t[1:, 4] > 0).all()) and int(t[0, 4]) > 0          # 24 units and the background
    over = 0
    for i in range(1, 25):
        for j in range(i + 1, 25):
            a, b = t[i], t[j]
            over += int(a[0] < b[1] and b[0] < a[1] and a[2] < b[3] and b[2] < a[3])
    assert over >= 10                                               # bounding boxes overlap each other
    b = R.blocky_raster()
    tb, _ = R.unit_table(b, 13)
    assert int(tb[:, 0].min()) == 0 and int(tb[:, 1].max()) == 96 and int(tb[:, 3].max()) == 128 and bool((tb[1:, 4] == 1024).all())


def test_one_unit_plan_is_the_reference_rule(case):
    name, boundary, ids, pop, table = case
    shape = tuple(boundary.shape)
    counts = table[ids, 4].sort().values
    areas = ((table[ids, 1] - table[ids, 0]) * (table[ids, 3] - table[ids, 2])).sort().values
    # no filter, a count filter that drops the largest units, a box filter that drops the largest boxes, both
    settings = [(10_000_000, 12_000_000), (int(counts[-3]), 12_000_000), (10_000_000, int(areas[-4])),
                (int(counts[-2]), int(areas[-3]))]
    dropped = set()
    for max_pix, max_pix_box in settings:
        want = R.one_unit_rule(table, ids, pop, shape, OVERLAP, max_pix, max_pix_box)
        plan = plan_one_unit(table, ids, pop, shape, admin_overlap=OVERLAP, max_pix=max_pix, max_pix_box=max_pix_box)
        assert not plan.multi and len(plan) == len(want) and plan.census_n == [1] * len(want)
        assert plan.census_idx[:, 0].tolist() == [r[0] for r in want]
        assert plan.y[:, 0].tolist() == [torch.tensor(r[1]).item() for r in want]
        assert plan.bbox.tolist() == [list(r[2]) for r in want]
        assert plan.crops.tolist() == [list(r[3]) for r in want]
        dropped.add(len(ids) - len(want))
    # the filters bite (equal blocks go all at once, irregular units a few at a time); the unit without pixels is always dropped
    assert min(dropped) == 1 and (dropped == {1, 13} if name == "blocky" else len(dropped) >= 3 and max(dropped) < 13)
    if name == "blocky":
        # clipping at all four raster edges, growth by the overlap inside
        plan = plan_one_unit(table, ids, pop, shape, admin_overlap=OVERLAP)
        c = {int(i): r for i, r in zip(plan.census_idx[:, 0], plan.crops.tolist())}
        assert c[1] == [0, 36, 0, 36] and c[12] == [60, 96, 92, 128] and c[6] == [28, 68, 28, 68]
        assert c[4] == [0, 36, 92, 128] and c[9] == [60, 96, 0, 36]


def test_multi_unit_plan_invariants(case):
    name, boundary, ids, pop, table = case
    shape = tuple(boundary.shape)
    one = plan_one_unit(table, ids, pop, shape, admin_overlap=OVERLAP, max_pix_box=BUDGET)
    plan = plan_multi_unit(table, ids, pop, shape, units_per_crop=K, admin_overlap=OVERLAP, max_pix_box=BUDGET)
    eligible = one.census_idx[:, 0].tolist()
    assert plan.multi and len(eligible) >= 12
    listed = []
    for i in range(len(plan)):
        n = plan.census_n[i]
        row = plan.census_idx[i].tolist()
        x0, x1, y0, y1 = plan.crops[i].tolist()
        # (d) at most K units, distinct, non-negative, padded with -1 / 0 behind census_n
        assert 1 <= n <= K and len(set(row[:n])) == n and min(row[:n]) >= 0
        assert row[n:] == [-1] * (K - n) and plan.y[i, n:].tolist() == [0.0] * (K - n)
        # (e) non-empty, inside the raster
        assert 0 <= x0 < x1 <= shape[0] and 0 <= y0 < y1 <= shape[1]
        # (c) over the budget only with a single unit
        assert (x1 - x0) * (y1 - y0) < BUDGET or n == 1
        win = boundary[x0:x1, y0:y1]
        for k in range(n):
            u = row[k]
            xmin, xmax, ymin, ymax, count = table[u].tolist()
            # (b) the bounding box inside the crop; complete by pixel count; y is the unit's whole count
            assert x0 <= xmin and xmax <= x1 and y0 <= ymin and ymax <= y1
            assert int((win == u).sum()) == count > 0
            assert plan.y[i, k].item() == pop[ids.tolist().index(u)].item()
        listed += row[:n]
    # (a) every eligible unit exactly once
    assert sorted(listed) == sorted(eligible)
    assert len(plan) < len(eligible)                                # strictly fewer crops than units
    assert max(plan.census_n) > 1
    if name == "blocky":
        assert len(plan) <= 6 and max(plan.census_n) == 4           # 2 x 2 groups fit the budget


def test_plans_are_deterministic(case):
    _, boundary, ids, pop, table = case
    shape = tuple(boundary.shape)
    for make in (lambda: plan_one_unit(table, ids, pop, shape, admin_overlap=OVERLAP, max_pix_box=BUDGET),
                 lambda: plan_multi_unit(table, ids, pop, shape, units_per_crop=K, admin_overlap=OVERLAP, max_pix_box=BUDGET)):
        a, b = make(), make()
        assert isinstance(a, RegionPlan) and a == b
    # K = 1: the multi-unit planner lists the one-unit plan's units, one per crop, with the same crops
    one = plan_one_unit(table, ids, pop, shape, admin_overlap=OVERLAP, max_pix_box=BUDGET)
    k1 = plan_multi_unit(table, ids, pop, shape, units_per_crop=1, admin_overlap=OVERLAP, max_pix_box=BUDGET)
    by_id = {int(i): c for i, c in zip(one.census_idx[:, 0], one.crops.tolist())}
    assert sorted(k1.census_idx[:, 0].tolist()) == sorted(by_id) and all(by_id[int(i)] == c for i, c in zip(k1.census_idx[:, 0], k1.crops.tolist()))


def test_planner_rejects_bad_census():
    table, _ = R.unit_table(R.blocky_raster(), 13)
    with pytest.raises(ValueError):
        plan_one_unit(table, torch.tensor([1, 1]), torch.tensor([1.0, 2.0]), (96, 128))
    with pytest.raises(ValueError):
        plan_one_unit(table, torch.tensor([13]), torch.tensor([1.0]), (96, 128))
    with pytest.raises(ValueError):
        plan_multi_unit(table, torch.tensor([1]), torch.tensor([1.0]), (96, 128), units_per_crop=0)


def test_oracle_items_collate_like_the_loader():
    """The oracle's items go through the existing collates: padding 0 / 0 / -1 at the bottom and right, data_hw the items' extents."""
    g = torch.Generator().manual_seed(1)
    boundary = R.blocky_raster()
    s2 = torch.randint(0, 10000, (1, 4, 96, 128), generator=g).to(torch.uint16)
    s1 = torch.randn(1, 2, 96, 128, generator=g)
    table, _ = R.unit_table(boundary, 13)
    ids, pop = _census(12)
    plan = plan_one_unit(table, ids, pop, (96, 128), admin_overlap=OVERLAP)
    items = R.plan_items(s2, s1, boundary, (2, 1, 0, 3, 1, 0), plan, [0, 5], [0, 0])
    batch = R.host_batch(items, False)
    assert tuple(batch["S2"].shape) == (2, 4, 40, 40) and batch["data_hw"].tolist() == [[36, 36], [40, 40]]
    assert torch.equal(batch["S2"][0, 0, :36, :36], s2[0, 2, 0:36, 0:36].float()) and bool((batch["S2"][0, :, 36:] == 0).all())
    assert torch.equal(batch["S1"][1, 0], s1[0, 1, 28:68, 28:68]) and bool((batch["admin_mask"][0, :, 36:] == -1).all())
    assert batch["census_idx"].tolist() == [1, 6] and batch["valid_coords"][1] == (32, 64, 32, 64)


def test_train_parser_region_flags():
    from popcorn_amd.cli import train_parser
    a = train_parser().parse_args([])
    assert a.resident_region is None and a.resident_units == 400 and a.max_weak_pix == 10_000_000 and a.max_pix_box == 12_000_000
    a = train_parser().parse_args("--resident_region 192 256 --resident_units 24 --units_per_crop 4".split())
    assert a.resident_region == [192, 256] and a.resident_units == 24
