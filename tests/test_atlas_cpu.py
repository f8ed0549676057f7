"""The resident atlas without a GPU: the exported symbols and the struct size, the ABI version, ``AtlasPlan``, the joined patch tables on
a hand-made table, the epoch draws of a feed over an atlas of one region against the region feed, and the command line."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def test_library_exports_the_atlas_entry_points_and_the_struct_size():
    from popcorn_amd import _lib as L
    lib = L.lib()
    for name in ("pc_atlas_create", "pc_atlas_destroy", "pc_atlas_gather", "pc_atlas_batch", "pc_sizeof_atlas_region"):
        assert hasattr(lib, name), name
    assert lib.pc_sizeof_atlas_region() == C.sizeof(L.PcAtlasRegion) == 88
    f = L.PcAtlasRegion
    assert (f.s2.offset, f.s1.offset, f.s1_asc.offset, f.boundary.offset, f.layer.offset, f.S.offset, f.w.offset, f.band_sel.offset) == \
        (0, 8, 16, 24, 32, 40, 56, 60)
    assert L.PC_ATLAS_MAX_REGIONS >= 8
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10
    assert lib.pc_sizeof(9) == -1                                    # the new struct has no index of pc_sizeof
    with open(__file__.rsplit("tests", 1)[0] + "include/popcorn_hip.h") as fh:
        header = fh.read()
    for name in ("pc_atlas_create(", "pc_atlas_destroy(", "pc_atlas_gather(", "pc_atlas_batch(", "pc_sizeof_atlas_region(",
                 f"#define PC_ATLAS_MAX_REGIONS {L.PC_ATLAS_MAX_REGIONS}", "#define PC_ABI_VERSION 10"):
        assert name in header, name


def test_create_refuses_bad_arguments_before_touching_a_device():
    from popcorn_amd import _lib as L
    lib = L.lib()
    h = C.c_void_p()
    d = (L.PcAtlasRegion * 2)()
    assert lib.pc_atlas_create(d, 0, 0, C.byref(h)) == L.PC_EINVAL
    assert lib.pc_atlas_create(d, L.PC_ATLAS_MAX_REGIONS + 1, 0, C.byref(h)) == L.PC_EINVAL
    assert lib.pc_atlas_create(d, 2, 0, C.byref(h)) == L.PC_EINVAL   # NULL sources
    assert lib.pc_atlas_create(None, 1, 0, C.byref(h)) == L.PC_EINVAL
    assert h.value is None
    lib.pc_atlas_destroy(None)


def _plan(n, K, base, multi):
    from popcorn_amd.data.region import RegionPlan
    crops = torch.tensor([[i, i + 3 + base, 2 * i, 2 * i + 5] for i in range(n)], dtype=torch.int64)
    cidx = torch.full((n, K), -1, dtype=torch.int64)
    y = torch.zeros(n, K)
    cn = []
    for i in range(n):
        k = 1 + (i + base) % K
        cidx[i, :k] = torch.arange(k) + 10 * i + base
        y[i, :k] = torch.arange(k).float() + 0.5 + base
        cn.append(k)
    return RegionPlan(crops, cidx, y, cn, crops.clone() + 1, multi)


def test_atlas_plan_concat_subset_and_equality():
    from popcorn_amd.data.atlas import AtlasPlan
    a, b, c = _plan(3, 2, 0, True), _plan(2, 4, 100, True), _plan(4, 1, 200, True)
    plan = AtlasPlan.concat([a, b, c])
    assert len(plan) == 9 and plan.multi and plan.region.tolist() == [0] * 3 + [1] * 2 + [2] * 4
    assert tuple(plan.census_idx.shape) == (9, 4) and plan.census_n == a.census_n + b.census_n + c.census_n
    assert torch.equal(plan.crops[3:5], b.crops) and torch.equal(plan.bbox[5:], c.bbox)          # each region's own coordinates
    assert torch.equal(plan.census_idx[:3, :2], a.census_idx) and bool((plan.census_idx[:3, 2:] == -1).all())
    assert torch.equal(plan.y[:3, :2], a.y) and bool((plan.y[:3, 2:] == 0).all())
    sub = plan.subset([8, 0, 4])
    assert isinstance(sub, AtlasPlan) and sub.region.tolist() == [2, 0, 1] and sub.census_n == [plan.census_n[i] for i in (8, 0, 4)]
    assert torch.equal(sub.crops, plan.crops[[8, 0, 4]])
    rows, mem = plan.member(1)
    assert rows == [3, 4] and type(mem).__name__ == "RegionPlan" and torch.equal(mem.crops, b.crops)
    assert plan == AtlasPlan.concat([a, b, c]) and plan.subset(range(9)) == plan
    other = AtlasPlan.concat([a, b, c])
    other.region[0] = 1
    assert plan != other and plan != plan.subset(range(8))
    with pytest.raises(ValueError):
        AtlasPlan.concat([a, _plan(2, 1, 0, False)])                 # all multi or none
    with pytest.raises(ValueError):
        AtlasPlan(a.crops, a.census_idx, a.y, a.census_n, a.bbox, True, [0, 1])
    one = AtlasPlan.concat([_plan(3, 1, 0, False)])
    assert one.region.tolist() == [0, 0, 0] and not one.multi


def test_joined_patch_tables_shift_the_offsets():
    from popcorn_amd.data.atlas import join_patch_tables
    # region 0: 2 items x 2 seasons with 3, 0, 1, 2 entries; region 1: 1 item x 2 seasons with 0, 4; region 2: no entries at all
    offs = [torch.tensor([0, 3, 3, 4, 6]), torch.tensor([0, 0, 4]), torch.tensor([0, 0, 0])]
    idxs = [torch.arange(6, dtype=torch.int32), torch.arange(100, 104, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)]
    vals = [torch.arange(6).float(), torch.arange(4).float() + 0.5, torch.zeros(0)]
    off, idx, val = join_patch_tables(offs, idxs, vals)
    assert off.tolist() == [0, 3, 3, 4, 6, 6, 10, 10, 10] and off.dtype == torch.int64
    assert idx.tolist() == [0, 1, 2, 3, 4, 5, 100, 101, 102, 103] and val.tolist()[6:] == [0.5, 1.5, 2.5, 3.5]
    # slot k of the joined table is the slot of its own plan: region 1's (item 0, season 1) is slot 4 + 1
    assert idx[off[5]:off[6]].tolist() == [100, 101, 102, 103]


def _fake_atlas():
    from popcorn_amd.data.atlas import ResidentAtlas
    atlas = object.__new__(ResidentAtlas)
    atlas.regions, atlas.names, atlas.device, atlas.seasons, atlas.layered, atlas.handle = [None], ["0"], torch.device("cpu"), 2, False, None
    return atlas


@pytest.mark.parametrize("budget", [0, 700])
def test_an_atlas_feed_of_one_region_takes_the_region_feeds_draws(budget, monkeypatch):
    """The same generator gives the same permutation, seasons, plan_batches inputs and batches; the launch sees the region column."""
    from popcorn_amd.data import region as RG
    from popcorn_amd.data.atlas import AtlasBatchFeed, AtlasPlan, AtlasRegionFeed
    base = _plan(11, 1, 0, False)
    plan = AtlasPlan.concat([base])
    region = SimpleNamespace(device=torch.device("cpu"), seasons=2, buildings=None)
    seen = {"region": [], "atlas": [], "pb_region": [], "pb_atlas": []}

    def launch(tag):
        def f(self, idx, crops, *a):
            seen[tag].append((np.asarray(idx).tolist(), np.asarray(crops).tolist(), None if tag == "region" else self._region[idx].tolist()))
            n = len(idx)
            return {"admin_mask": torch.zeros(n, 1, 1), "raw": torch.zeros(n, 6, 1, 1), "census_idx": torch.zeros(n, 1, dtype=torch.int64),
                    "y": torch.zeros(n, 1)}
        return f

    real = RG.plan_batches
    tag = ["pb_region"]

    def recording(hw, order, *a):
        seen[tag[0]].append(([tuple(v) for v in hw], [int(i) for i in order], a[:3]))
        return real(hw, order, *a)

    monkeypatch.setattr(RG, "plan_batches", recording)
    monkeypatch.setattr(RG.ResidentRegionFeed, "_gather", launch("region"))
    monkeypatch.setattr(RG.ResidentBatchFeed, "_assemble", launch("region"))
    monkeypatch.setattr(AtlasRegionFeed, "_gather", launch("atlas"))
    monkeypatch.setattr(AtlasBatchFeed, "_assemble", launch("atlas"))
    gen = lambda: torch.Generator().manual_seed(9)
    if budget:
        old = RG.ResidentBatchFeed(region, base, 2, generator=gen(), seasons=2, pixel_budget=budget, max_batch=4)
        new = AtlasBatchFeed(_fake_atlas(), plan, 2, generator=gen(), seasons=2, pixel_budget=budget, max_batch=4)
    else:
        old = RG.ResidentRegionFeed(region, base, 2, generator=gen(), seasons=2)
        new = AtlasRegionFeed(_fake_atlas(), plan, 2, generator=gen(), seasons=2)
    for epoch in range(2):
        tag[0] = "pb_region"
        a = list(old)
        tag[0] = "pb_atlas"
        b = list(new)
        assert torch.equal(old.last_order, new.last_order) and torch.equal(old.last_season, new.last_season)
        assert torch.equal(old.generator.get_state(), new.generator.get_state())
        assert len(a) == len(b) >= 2
        for x, y in zip(a, b):
            assert x["img_coords"] == y["img_coords"] and x["valid_coords"] == y["valid_coords"] and torch.equal(x["season"], y["season"])
    assert [s[:2] for s in seen["region"]] == [s[:2] for s in seen["atlas"]] and len(seen["atlas"]) >= 4
    assert all(s[2] == [0] * len(s[0]) for s in seen["atlas"])
    assert seen["pb_region"] == seen["pb_atlas"] and len(seen["pb_atlas"]) == (2 if budget else 0)


def test_feeds_refuse_what_is_not_an_atlas():
    from popcorn_amd.data.atlas import AtlasPlan, AtlasRegionFeed
    base = _plan(4, 1, 0, False)
    with pytest.raises(ValueError):
        AtlasRegionFeed(_fake_atlas(), base, 2)                      # a RegionPlan
    two = AtlasPlan.concat([base, base])
    with pytest.raises(ValueError):
        AtlasRegionFeed(_fake_atlas(), two, 2)                       # region 1 of an atlas of one
    with pytest.raises(ValueError):
        AtlasRegionFeed(_fake_atlas(), AtlasPlan.concat([base]), 2, seasons=3)     # more than the smallest S of the atlas


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _parse(*argv):
    from popcorn_amd.cli import check_repair_args, train_parser
    args = train_parser().parse_args(list(argv))
    check_repair_args(args)
    return args


def test_resident_region_takes_two_integers_per_region():
    from popcorn_amd.cli import resident_shapes
    assert _parse().resident_region is None
    a = _parse("--resident_region", "96", "128")
    assert a.resident_region == [96, 128] and resident_shapes(a) == ([(96, 128)], [400])
    a = _parse("--resident_region", "96", "128", "120", "150", "64", "80", "--resident_assemble")
    assert resident_shapes(a) == ([(96, 128), (120, 150), (64, 80)], [400, 400, 400])
    a = _parse("--resident_region", "96", "128", "120", "150", "--resident_units", "24", "30")
    assert resident_shapes(a)[1] == [24, 30]
    a = _parse("--resident_region", "96", "128", "120", "150", "--resident_units", "24")
    assert resident_shapes(a)[1] == [24, 24]
    with pytest.raises(SystemExit):
        _parse("--resident_region", "96", "128", "120", "150", "64")             # five integers
    with pytest.raises(SystemExit):
        _parse("--resident_region", "96")
    with pytest.raises(SystemExit):
        _parse("--resident_region", "96", "128", "120", "150", "--resident_units", "24", "30", "40")
    with pytest.raises(SystemExit):
        _parse("--resident_region", *(["64", "64"] * 17))                          # more regions than an atlas holds


def test_resident_ascfill_needs_a_plan_that_takes_it():
    two = ("--resident_region", "96", "128", "120", "150")
    with pytest.raises(SystemExit) as e:
        _parse(*two, "--resident_ascfill", "1")
    assert "no plan takes it" in str(e.value)
    with pytest.raises(SystemExit):
        _parse(*two, "--resident_assemble", "--resident_ascfill", "1")
    with pytest.raises(SystemExit):
        _parse("--resident_ascfill", "0")                                          # no resident region at all
    for plan in ("--resident_repair", "--resident_val", "--resident_test"):
        assert _parse(*two, plan, "--resident_ascfill", "1").resident_ascfill == [1]
    with pytest.raises(SystemExit):
        _parse(*two, "--resident_repair", "--resident_ascfill", "2")               # outside [0, R)
    assert _parse(*two, "--resident_repair", "--ascfill").resident_ascfill is None # --ascfill keeps meaning all regions
