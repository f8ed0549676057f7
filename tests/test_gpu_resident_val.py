"""Resident validation (data/region.py: ResidentItems, split_census; cli.py: --resident_val, --resident_seasons) against the per-item host
path it replaces, fp32 compared as integers:

    ResidentItems item == normalize_sample(region.gather([crop + season], orbit=[orbit]), transform=None, nan_fill=True)

with the orbit decided independently from torch's own NaN counts of the crop, and through the trainer: ``validate_weak`` under
--resident_val returns the metrics of the model run on those host-path items."""
import pytest
import torch

from tests.footprint import bit_equal

pytestmark = pytest.mark.gpu

RH, RW, UNITS, SEASONS = 96, 128, 24, 2
_CACHE = {}


def _region(kind):
    """96 x 128, 24 units, two seasons: cloud discs in S2 (fp32) and gap rows in the descending S1; the ascending S1 holds NO NaN, so the
    orbit rule cannot drop an item.  "u16": S2 as digital numbers (its NaN sites zeroed); "clean": no NaN anywhere."""
    if kind not in _CACHE:
        from popcorn_amd.data.dataset import SyntheticTestRaster
        from popcorn_amd.data.region import ResidentRegion
        dirty = kind != "clean"
        data = SyntheticTestRaster(RH, RW, seasons=SEASONS, n_regions=UNITS, seed=1614, device="cuda", raw=True,
                                   nan_clouds=0.05 if dirty else 0.0, s1_gap=0.05 if dirty else 0.0)
        assert not bool(torch.isnan(data.s1_asc).any())
        assert bool(torch.isnan(data.s1).any()) == dirty and bool(torch.isnan(data.s2).any()) == dirty
        if kind == "u16":
            data.s2 = torch.nan_to_num(data.s2.cpu(), nan=0.0).to(torch.int32).to(torch.uint16).cuda()
        _CACHE[kind] = ResidentRegion.from_synthetic(data, with_asc=True)
    return _CACHE[kind]


def _plan(region, units_per_crop):
    from popcorn_amd.data.region import plan_multi_unit, plan_one_unit
    if units_per_crop:
        return plan_multi_unit(region.table, region.census_idx, region.census_pop, region.shape, units_per_crop=units_per_crop)
    return plan_one_unit(region.table, region.census_idx, region.census_pop, region.shape)


def _host_orbit(region, crop, season, ascfill=False):
    """The orbit of one item from torch's own NaN counts (nanfill's rule through ``item_orbit``)."""
    from popcorn_amd.data.region import item_orbit
    x0, x1, y0, y1 = crop
    sel = list(region.band_sel[4:])
    n_desc = int(torch.isnan(region.s1[season, sel, x0:x1, y0:y1]).sum())
    n_asc = int(torch.isnan(region.s1_asc[season, sel, x0:x1, y0:y1]).sum())
    orbit, ok = item_orbit(n_desc, n_asc, 2 * (x1 - x0) * (y1 - y0), ascfill, True)
    assert ok
    return orbit


def _host_item(region, plan, k, season, orbit):
    """The per-item host path: gather, fill, concatenate, normalise (cli.normalize_sample with nan_fill)."""
    from popcorn_amd import cli
    crop = tuple(plan.crops[k].tolist()) + (season,)
    g = region.gather([crop], orbit=[orbit])
    K = plan.census_n[k]
    g["census_idx"] = plan.census_idx[k:k + 1, :K] if plan.multi else plan.census_idx[k, :1]
    g["y"] = plan.y[k:k + 1, :K] if plan.multi else plan.y[k, :1]
    return cli.normalize_sample(g, region.device, None, nan_fill=True)


def _assert_item(got, want, multi, K):
    assert bit_equal(got["input"], want["input"]) and not bool(torch.isnan(got["input"]).any())
    assert bit_equal(got["admin_mask"], want["admin_mask"])
    assert torch.equal(got["census_idx"], want["census_idx"]) and bit_equal(got["y"], want["y"])
    assert got["census_idx"].dtype == torch.int64 and got["census_idx"].is_cuda
    assert tuple(got["y"].shape) == ((1, K) if multi else (1,))
    assert (got.get("census_n") == [K]) if multi else ("census_n" not in got)


@pytest.mark.parametrize("units_per_crop", [0, 3])
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_every_item_equals_the_per_item_host_path(kind, units_per_crop, monkeypatch):
    from popcorn_amd import ops
    from popcorn_amd.data.region import ResidentItems
    region = _region(kind)
    plan = _plan(region, units_per_crop)
    n = len(plan)
    assert n == (UNITS if not units_per_crop else len(plan.census_n)) and sum(plan.census_n) == UNITS
    items = ResidentItems(region, plan, seasons=SEASONS, generator=torch.Generator().manual_seed(5))
    assert items.dropped == [] and len(items) == n and items.plan == plan
    season = torch.randint(0, SEASONS, (n,), generator=torch.Generator().manual_seed(5))
    assert torch.equal(items.season, season) and set(season.tolist()) == {0, 1}
    # the orbit column, decided here from torch's own NaN counts; both orbits and repaired items occur before anything is compared
    orbits = [_host_orbit(region, plan.crops[k].tolist(), int(season[k])) for k in range(n)]
    assert items.orbit.tolist() == orbits and set(orbits) == {0, 1} and items.ascending == sum(orbits)
    assert tuple(items.counts.shape) == (n, 3) and tuple(items.off.shape) == (n + 1,)
    assert items.entries == int(items.off[-1]) == items.table_idx.numel() > 0 and items.nbytes == 8 * items.entries and items.build_ms > 0
    want = [_host_item(region, plan, k, int(season[k]), orbits[k]) for k in range(n)]
    # ascfill: every item whose descending S1 holds a NaN switches
    filled = ResidentItems(region, plan, seasons=SEASONS, generator=torch.Generator().manual_seed(5), ascfill=True)
    assert filled.orbit.tolist() == [int(c > 0) for c in filled.counts[:, 1].tolist()] and filled.ascending > items.ascending

    def no_fill(*a, **k):
        raise AssertionError("the resident validation ran a per-item fill")
    monkeypatch.setattr(ops, "nan_fill_", no_fill)
    first = []
    for k, got in enumerate(items):
        _assert_item(got, want[k], plan.multi, plan.census_n[k])
        first.append((got["input"].clone(), got["admin_mask"].clone()))
    assert len(first) == n
    for k, got in enumerate(items):                                      # a second iteration: the same bits
        assert bit_equal(got["input"], first[k][0]) and bit_equal(got["admin_mask"], first[k][1])


def test_region_without_nan_needs_no_table():
    from popcorn_amd.data.region import ResidentItems
    region = _region("clean")
    plan = _plan(region, 0)
    items = ResidentItems(region, plan, seasons=SEASONS, generator=torch.Generator().manual_seed(5))
    assert items.entries == 0 and items.table_idx.numel() == 0 and items.nbytes == 0 and items.ascending == 0 and items.dropped == []
    assert int(items.counts.sum()) == 0
    for k, got in enumerate(items):
        _assert_item(got, _host_item(region, plan, k, int(items.season[k]), 0), False, 1)
    one = ResidentItems(region, plan)                                    # seasons == 1: every item in season 0, no draw
    assert one.season.tolist() == [0] * len(plan)
    with pytest.raises(ValueError, match="seasons"):
        ResidentItems(region, plan, seasons=SEASONS + 1)


ARGV = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --resident_region 96 128 --resident_units 24 "
        "--resident_seasons 2 -wv --nan_clouds 0.05 --resident_repair --resident_s1_gap 0.05 --max_steps 2 --save-model no")


def test_trainer_trains_on_the_train_split_and_validates_on_the_held_out_units(tmp_path, capsys):
    from popcorn_amd import cli
    from popcorn_amd.data.region import plan_one_unit
    from popcorn_amd.utils.metrics import get_test_metrics
    a = cli.train_parser().parse_args((ARGV + f" --resident_val --save_dir {tmp_path}").split())
    t = cli.Trainer(a)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("resident validation:")]
    assert len(line) == 1 and all(w in line[0] for w in ("items", "dropped", "ascending", "entries", "bytes", "ms"))
    region, items = t.region, t.val_items
    assert region.seasons == 2 and region.s1_asc is not None and items.seasons == 2 and items.dropped == []
    # the two plans share no listed unit and together list every eligible unit
    everything = plan_one_unit(region.table, region.census_idx, region.census_pop, region.shape, max_pix=a.max_weak_pix,
                               max_pix_box=a.max_pix_box)
    train_units, val_units = t.region_plan.census_idx[:, 0].tolist(), items.plan.census_idx[:, 0].tolist()
    assert not set(train_units) & set(val_units)
    assert sorted(train_units + val_units) == sorted(everything.census_idx[:, 0].tolist()) and len(everything) == UNITS
    assert len(val_units) == UNITS - int(UNITS * 0.8) and len(train_units) == int(UNITS * 0.8)
    # validate_weak: the metrics of the model run on the host-path items
    listed = (items.plan.crops.clone(), items.season.clone(), items.orbit.clone())
    first = dict(t.validate_weak())
    pred, gt = [], []
    t.model.eval()
    with torch.no_grad():
        for k in range(len(items)):
            season = int(items.season[k])
            orbit = _host_orbit(region, items.plan.crops[k].tolist(), season, a.ascfill)
            s = _host_item(region, items.plan, k, season, orbit)
            pred.append(t.model(s, padding=False)["popcount"])
            gt.append(s["y"])
    want = {k + "/val": float(v) for k, v in get_test_metrics(torch.cat(pred), torch.cat(gt).float(), tag="MainCensus_synthetic_fine").items()}
    assert first == want and len(first) > 2 and all(v == v for v in first.values())
    # two training steps, then a second validation over the same item list
    t.train()
    assert t.info["iter"] == 2
    second = t.validate_weak()
    assert set(second) == set(first) and all(v == v for v in second.values())
    assert torch.equal(items.plan.crops, listed[0]) and torch.equal(items.season, listed[1]) and torch.equal(items.orbit, listed[2])
    assert t.val_items is items


def test_trainer_without_resident_val_plans_every_unit(tmp_path):
    from popcorn_amd import cli
    from popcorn_amd.data.region import plan_one_unit
    a = cli.train_parser().parse_args((ARGV + f" --save_dir {tmp_path}").split())
    t = cli.Trainer(a)
    assert t.val_items is None
    everything = plan_one_unit(t.region.table, t.region.census_idx, t.region.census_pop, t.region.shape, max_pix=a.max_weak_pix,
                               max_pix_box=a.max_pix_box)
    assert t.region_plan == everything and len(everything) == UNITS
