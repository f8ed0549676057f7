"""The resident atlas on the GPU (csrc/region_atlas.hip and everything above it): several resident regions, one launch per batch.

Three regions chosen so that a wrong region's stride, extent, band map or season count shows up (tests/atlas_oracle.py: 37 x 53 with one
season and the reference's band order, 64 x 48 and 96 x 128 with two seasons), values distinct per (region, season, band, pixel), NaNs with
payloads.  Every comparison is an equality of bits (fp32 compared as int32):

    row b of ops.atlas_gather     ==  the host item of crop b cut from its OWN region, padded by the collate
                                  ==  row 0 of ops.region_gather on that region alone at the same tile
    ops.atlas_batch               ==  ops.augment_raw(ops.atlas_gather(...), coins), plus the label rows of the concatenated plan table
    R = 1                         ==  ops.region_gather / ops.region_batch on every output

Outputs sit in poisoned memory between the guard bands of tests/footprint.py.  Above the ops: the refusals (no kernel is reached), the
feeds against the host path, the planned repair, and the trainer over two regions."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest
import torch

from tests import atlas_oracle as A
from tests import region_oracle as R
from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

REGION_OF = (1, 0, 2, 0, 1)
# {x0, x1, y0, y1, season}: a crop that ends at its raster's bottom-right pixel in season 1 (64 x 48), a 1 x 1 crop of the S = 1 region next to
# it, rows 70 .. 96 that exist only in the 96-row region (again ending at the bottom-right pixel), a crop whose width 23 straddles the
# four-pixel groups, and one at an odd column origin
CROPS = {
    "wm28": [(40, 64, 20, 48, 1), (5, 6, 7, 8, 0), (70, 96, 100, 128, 1), (3, 37, 30, 53, 0), (0, 10, 1, 27, 0)],       # 34 x 28: four pixels
    "wm29": [(40, 64, 20, 48, 1), (5, 6, 7, 8, 0), (70, 96, 99, 128, 0), (3, 37, 30, 53, 0), (0, 10, 1, 27, 1)],        # 34 x 29: one pixel
}
ORBIT = (1, 0, 1, 0, 0)                                             # region 0 holds no s1_asc and sits next to ascending crops
GEOMETRY = list(itertools.product((False, True), (False, True), (0, 1, 2, 3)))
VALUES = [(None, None), (1.3, None), (None, 0.8), (0.7, 1.4)]
VARIANTS = [("f32", False), ("u16", False), ("f32", True), ("u16", True)]
_HOST = {}


def _host(kind, layer):
    """the three regions on the host; regions 1 and 2 hold an ascending S1, region 0 does not"""
    if (kind, layer) not in _HOST:
        _HOST[(kind, layer)] = [A.make_region(k, kind, layer, asc=k > 0) for k in range(3)]
    return _HOST[(kind, layer)]


def _place(fp, regions):
    from popcorn_amd import ops
    dev = [{k: (fp.place(v) if torch.is_tensor(v) and k not in ("census_idx", "census_pop") else v) for k, v in r.items()} for r in regions]
    return dev, ops.AtlasHandle(dev)


def _single(r, crops, orbit=None, out=None):
    from popcorn_amd import ops
    return ops.region_gather(r["s2"], r["s1"], r["boundary"], r["band_sel"], crops, out=out, s1_asc=r.get("s1_asc"), orbit=orbit,
                             buildings=r.get("buildings"))


def _tile(B, hw, layer, fp=None, shift=0):
    """an ``out`` dict of tile hw; shift = 1: every output starts 4 bytes behind a 512-byte boundary"""
    def mk(shape, dtype=torch.float32):
        n = int(np.prod(shape))
        if fp is None:
            return torch.empty(n + shift, dtype=dtype, device="cuda")[shift:].view(shape)
        return fp.alloc((n + shift,), dtype)[shift:].view(shape)
    out = {"S2": mk((B, 4) + hw), "S1": mk((B, 2) + hw), "admin_mask": mk((B,) + hw), "data_hw": mk((B, 2), torch.int32)}
    if layer:
        out["building_counts"] = mk((B, 1) + hw)
    return out


KEYS = ("S2", "S1", "admin_mask", "data_hw")


# ---- the gather -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layer", VARIANTS)
def test_atlas_gather_equals_the_host_items_and_the_single_region_gather(kind, layer):
    from popcorn_amd import ops
    regions = _host(kind, layer)
    keys = KEYS + (("building_counts",) if layer else ())
    checked = 0
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, regions)
        for (name, crops), orbit, shift in itertools.product(CROPS.items(), (None, ORBIT), (0, 1)):
            Hm, Wm = max(c[1] - c[0] for c in crops), max(c[3] - c[2] for c in crops)
            assert (Hm, Wm) == (34, 28 if name == "wm28" else 29)
            want = A.host_atlas_batch(regions, REGION_OF, crops, orbit)
            n0 = fp.guarded
            if shift:
                got = ops.atlas_gather(atlas, REGION_OF, crops, out=_tile(5, (Hm, Wm), layer, fp, 1), orbit=orbit)
                assert got["S2"].data_ptr() % 16 == 4
            else:
                got = ops.atlas_gather(atlas, REGION_OF, crops, orbit=orbit)
                assert fp.guarded == n0 + len(keys)                   # the outputs and nothing else
            assert got["region"] == list(REGION_OF)
            for key in keys:
                assert bit_equal(got[key].cpu(), want[key]), (name, orbit, shift, key)
            # row b == row 0 of the single-region gather of crop b at the same tile
            for b, (k, c) in enumerate(zip(REGION_OF, crops)):
                one = _single(dev[k], [c], None if orbit is None else [orbit[b]], out=_tile(1, (Hm, Wm), layer))
                for key in keys:
                    assert bit_equal(got[key][b:b + 1].contiguous(), one[key]), (name, orbit, shift, b, key)
            checked += 1
            if kind == "f32" and orbit is None:
                seen = torch.cat([got["S2"].reshape(-1), got["S1"].reshape(-1)]).view(torch.int32)
                assert all(bool((seen == p).any()) for p in A.PAYLOADS)  # NaN payloads arrive bit for bit
    assert checked == 8


def test_a_larger_tile_pads_like_the_collate():
    from popcorn_amd import ops
    regions = _host("f32", True)
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, regions)
        got = ops.atlas_gather(atlas, REGION_OF, CROPS["wm28"], out=_tile(5, (36, 32), True, fp))
        want = A.host_atlas_batch(regions, REGION_OF, CROPS["wm28"], hw=(36, 32))
    for key in KEYS + ("building_counts",):
        assert bit_equal(got[key].cpu(), want[key]), key


# ---- the one-launch assembly ------------------------------------------------------------------------------------------------------------
def _augment(tile, params):
    from popcorn_amd import ops
    if "building_counts" in tile:
        return ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params, buildings=tile["building_counts"])
    return ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params)


def _same_batch(got, want, layer, what):
    assert bit_equal(got["raw"], want[0]) and bit_equal(got["admin_mask"], want[1]), what
    if layer:
        assert bit_equal(got["building_counts"], want[2]), what


@pytest.mark.parametrize("kind,layer", VARIANTS)
def test_atlas_batch_equals_gather_then_augment(kind, layer):
    from popcorn_amd import ops
    regions = _host(kind, layer)
    checked = 0
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, regions)
        for (name, crops), orbit in itertools.product(CROPS.items(), (None, ORBIT)):
            tile = ops.atlas_gather(atlas, REGION_OF, crops, orbit=orbit)
            for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES):
                params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
                want = _augment(tile, params)
                n0 = fp.guarded
                got = ops.atlas_batch(atlas, REGION_OF, crops, params, orbit=orbit)
                assert fp.guarded == n0 + 2 + int(layer) and got["region"] == list(REGION_OF)
                _same_batch(got, want, layer, (name, orbit, params))
                checked += 1
    assert checked == 4 * 64


def _label_tables(n, Kp):
    cidx = (torch.arange(n * Kp, dtype=torch.int64).reshape(n, Kp) * 3 + 1)
    y = torch.arange(n * Kp, dtype=torch.float32).reshape(n, Kp) * 0.5 + 0.25
    return cidx, y


@pytest.mark.parametrize("K", [1, 3])
def test_atlas_batch_labels_index_the_concatenated_plan_table(K):
    """items index ONE table, the regions' rows one after another; K = 3 with ragged lists (the padding columns are copied as they are)."""
    from popcorn_amd import ops
    regions = _host("f32", False)
    cidx, y = _label_tables(30, 4)
    cidx[[4, 17], 1:] = -1                                           # ragged: one listed unit
    cidx[22, 2:] = -1
    items = [17, 4, 29, 0, 22]
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, regions)
        dc, dy = fp.place(cidx), fp.place(y)
        for rot in (0, 1):
            params = {"vflip": True, "hflip": False, "rot": rot, "beta": None, "gamma": None}
            got = ops.atlas_batch(atlas, REGION_OF, CROPS["wm28"], params, labels=(dc, dy, items, K), orbit=ORBIT)
            want = _augment(ops.atlas_gather(atlas, REGION_OF, CROPS["wm28"], orbit=ORBIT), params)
            _same_batch(got, want, False, rot)
            assert torch.equal(got["census_idx"].cpu(), cidx[items, :K]) and bit_equal(got["y"].cpu(), y[items, :K])


def test_more_crops_than_one_launch_change_region_across_the_boundary():
    """130 crops of 8 x 8 alternating over the three regions: two launches, crop 127 and crop 128 come from different regions."""
    from popcorn_amd import _lib as L, ops
    assert L.PC_REGION_GATHER_MAX_B == 128
    regions = _host("f32", False)
    g = torch.Generator().manual_seed(4)
    region_of = [i % 3 for i in range(130)]
    crops = []
    for k in region_of:
        (h, w), S = A.SPECS[k][0], A.SPECS[k][1]
        x0, y0 = int(torch.randint(0, h - 7, (1,), generator=g)), int(torch.randint(0, w - 7, (1,), generator=g))
        crops.append((x0, x0 + 8, y0, y0 + 8, int(torch.randint(0, S, (1,), generator=g))))
    assert region_of[127] != region_of[128]
    cidx, y = _label_tables(130, 2)
    items = list(range(129, -1, -1))
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, regions)
        dc, dy = fp.place(cidx), fp.place(y)
        tile = ops.atlas_gather(atlas, region_of, crops)
        want = A.host_atlas_batch(regions, region_of, crops)
        for key in KEYS:
            assert bit_equal(tile[key].cpu(), want[key]), key
        for rot in (0, 3):
            params = {"vflip": False, "hflip": True, "rot": rot, "beta": 1.2, "gamma": None}
            got = ops.atlas_batch(atlas, region_of, crops, params, labels=(dc, dy, items, 2))
            _same_batch(got, _augment(tile, params), False, rot)
            assert torch.equal(got["census_idx"].cpu(), cidx[items]) and bit_equal(got["y"].cpu(), y[items])


@pytest.mark.parametrize("kind,layer", [("f32", True), ("u16", False)])
def test_an_atlas_of_one_region_equals_the_single_region_entry_points(kind, layer):
    from popcorn_amd import ops
    r = _host(kind, layer)[2]
    crops = [(70, 96, 100, 128, 1), (3, 60, 5, 70, 0), (95, 96, 127, 128, 0), (0, 96, 0, 128, 1)]
    orbit = (1, 0, 0, 1)
    cidx, y = _label_tables(7, 3)
    with Footprint("cuda", fill=POISON) as fp:
        dev, atlas = _place(fp, [r])
        d = dev[0]
        dc, dy = fp.place(cidx), fp.place(y)
        one, many = _single(d, crops, orbit), ops.atlas_gather(atlas, [0] * 4, crops, orbit=orbit)
        assert set(many) == set(one) | {"region"}
        for key in one:
            assert bit_equal(many[key], one[key]), key
        for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES[::3]):
            params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
            kw = {"buildings": d["buildings"]} if layer else {}
            one = ops.region_batch(d["s2"], d["s1"], d["boundary"], d["band_sel"], crops, params, labels=(dc, dy, [6, 0, 3, 3], 2),
                                   s1_asc=d["s1_asc"], orbit=orbit, **kw)
            many = ops.atlas_batch(atlas, [0] * 4, crops, params, labels=(dc, dy, [6, 0, 3, 3], 2), orbit=orbit)
            assert set(many) == set(one) | {"region"}
            for key in one:
                assert bit_equal(many[key], one[key]), (key, params)


# ---- refusals: PC_EINVAL and no kernel -----------------------------------------------------------------------------------------------------
def test_refusals_reach_no_kernel():
    from popcorn_amd import _lib as L, ops
    lib = L.lib()
    plain = ops.AtlasHandle([{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in _host("f32", False)])
    layered = ops.AtlasHandle([{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in _host("f32", True)])
    Hm, Wm = 34, 28

    def outs(layer):
        out = {"raw": torch.full((5, 6, Hm, Wm), 7.0, device="cuda"), "S2": torch.full((5, 4, Hm, Wm), 7.0, device="cuda"),
               "S1": torch.full((5, 2, Hm, Wm), 7.0, device="cuda"), "admin_mask": torch.full((5, Hm, Wm), 7.0, device="cuda"),
               "data_hw": torch.full((5, 2), 7, dtype=torch.int32, device="cuda")}
        if layer:
            out["building_counts"] = torch.full((5, 1, Hm, Wm), 7.0, device="cuda")
        return out

    def call(atlas, region_of, crops, orbit, out, layer_out, which, Ho=Hm, Wo=Wm, rot=0):
        ro = np.asarray(region_of, dtype=np.uint8)
        cr = np.ascontiguousarray(np.asarray(crops, dtype=np.int32))
        ob = None if orbit is None else np.asarray(orbit, dtype=np.uint8)
        head = (atlas._h, ro.ctypes.data_as(C.POINTER(C.c_uint8)), cr.ctypes.data_as(C.POINTER(C.c_int32)),
                None if ob is None else ob.ctypes.data_as(C.POINTER(C.c_uint8)), len(crops), Hm, Wm)
        lo = None if layer_out is None else L.ptr(layer_out)
        if which == "gather":
            return lib.pc_atlas_gather(*head, L.ptr(out["S2"]), L.ptr(out["S1"]), L.ptr(out["admin_mask"]), lo, L.ptr(out["data_hw"]),
                                       L.stream_ptr())
        return lib.pc_atlas_batch(*head, 0, 0, rot, 0, C.c_float(1.0), 0, C.c_float(1.0), L.ptr(out["raw"]), L.ptr(out["admin_mask"]), lo, Ho,
                                  Wo, None, L.stream_ptr())

    good = list(CROPS["wm28"])
    swap = lambda b, c: good[:b] + [c] + good[b + 1:]
    cases = {
        "region_of >= R": dict(region_of=(1, 0, 3, 0, 1)),
        "rows 70 .. 96 exist in region 2, not in region 0": dict(crops=swap(1, (70, 96, 20, 48, 0))),
        "columns up to 128 exist in region 2, not in region 1": dict(crops=swap(0, (40, 64, 100, 128, 1))),
        "season 1 in the region of one season": dict(crops=swap(3, (3, 37, 30, 53, 1))),
        "an empty crop": dict(crops=swap(4, (5, 5, 1, 27, 0))),
        "a crop larger than the tile": dict(crops=swap(4, (0, 40, 1, 27, 0))),
        "ascending orbit in the region without s1_asc": dict(orbit=(1, 1, 1, 0, 0)),
        "an orbit byte above 1": dict(orbit=(2, 0, 0, 0, 0)),
    }
    for which in ("gather", "batch"):
        fn = ops.atlas_gather if which == "gather" else ops.atlas_batch
        for what, kw in cases.items():
            region_of, crops, orbit = kw.get("region_of", REGION_OF), kw.get("crops", good), kw.get("orbit")
            out = outs(False)
            assert call(plain, region_of, crops, orbit, out, None, which) == L.PC_EINVAL, (which, what)
            torch.cuda.synchronize()
            assert all(bool((out[k] == 7).all()) for k in out), (which, what)
            if what not in ("a crop larger than the tile",):
                with pytest.raises(ValueError):
                    fn(plain, region_of, crops, orbit=orbit)
        # layer_out for an atlas without a layer, and none for an atlas with one
        out = outs(True)
        assert call(plain, REGION_OF, good, None, out, out["building_counts"], which) == L.PC_EINVAL
        assert call(layered, REGION_OF, good, None, out, None, which) == L.PC_EINVAL
        assert call(plain, REGION_OF, good, None, out, None, which, Ho=Wm, Wo=Hm) == (0 if which == "gather" else L.PC_EINVAL)
        torch.cuda.synchronize()
        touched = {k for k in out if not bool((out[k] == 7).all())}
        assert touched == ({"S2", "S1", "admin_mask", "data_hw"} if which == "gather" else set()), (which, touched)
    out = outs(False)
    assert call(plain, REGION_OF, good, None, out, None, "batch", rot=4) == L.PC_EINVAL
    torch.cuda.synchronize()
    assert all(bool((out[k] == 7).all()) for k in out)
    # the accepted calls next to them do write
    out = outs(True)
    assert call(layered, REGION_OF, good, ORBIT, out, out["building_counts"], "batch") == 0
    torch.cuda.synchronize()
    assert not bool((out["raw"] == 7).all()) and not bool((out["building_counts"] == 7).all())
    # what the handle refuses at creation: a layer on some regions only, two S2 types, a region on the host
    mixed = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in _host("f32", True)]
    mixed[1] = dict(mixed[1], buildings=None)
    with pytest.raises(ValueError):
        ops.AtlasHandle(mixed)
    two = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in r.items()} for r in (_host("f32", False)[0], _host("u16", False)[1])]
    with pytest.raises(ValueError):
        ops.AtlasHandle(two)
    with pytest.raises(L.PopcornHipError):
        ops.AtlasHandle([_host("f32", False)[0]])
    with pytest.raises(ValueError):
        ops.AtlasHandle([])


# ---- the feeds ----------------------------------------------------------------------------------------------------------------------------
def _atlas_and_plan(multi=False, layer=False, kind="f32"):
    from popcorn_amd.data.atlas import AtlasPlan, ResidentAtlas
    from popcorn_amd.data.region import ResidentRegion, plan_multi_unit, plan_one_unit
    host = [A.make_region(k, kind, layer, asc=True) for k in range(3)]
    regions = [ResidentRegion(r["s2"], r["s1"], r["boundary"], r["census_idx"], r["census_pop"], band_sel=r["band_sel"], device="cuda",
                              s1_asc=r["s1_asc"], buildings=r.get("buildings")) for r in host]
    if multi:
        plans = [plan_multi_unit(g.table, r["census_idx"], r["census_pop"], g.shape, units_per_crop=3, admin_overlap=4, max_pix_box=3000)
                 for g, r in zip(regions, host)]
    else:
        plans = [plan_one_unit(g.table, r["census_idx"], r["census_pop"], g.shape, admin_overlap=4) for g, r in zip(regions, host)]
    return host, ResidentAtlas(regions, names=["a", "b", "c"]), AtlasPlan.concat(plans), plans


def _epoch(feed, prepare):
    torch.manual_seed(11)
    random.seed(11)
    out = []
    for sample in feed:
        s = prepare(sample)
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()})
        torch.rand(1)
    return out, torch.get_rng_state(), random.getstate()


@pytest.mark.parametrize("multi", [False, True])
def test_atlas_region_feed_equals_the_host_path(multi):
    """Every batch: the per-region items of the host, then the collate."""
    from popcorn_amd.data.atlas import AtlasRegionFeed
    host, atlas, plan, plans = _atlas_and_plan(multi)
    assert atlas.seasons == 1 and len(atlas) == 3 and plan.multi == multi
    if multi:
        assert len(set(plan.census_n)) > 1                            # ragged lists
    start = np.cumsum([0] + [len(p) for p in plans])
    feed = AtlasRegionFeed(atlas, plan, 3, generator=torch.Generator().manual_seed(5))
    seen = set()
    batches = list(feed)
    assert len(batches) == len(plan) // 3 >= 2
    for k, s in enumerate(batches):
        idx = feed.last_order[3 * k:3 * k + 3].tolist()
        reg = [int(plan.region[i]) for i in idx]
        assert s["region"] == reg
        seen.add(tuple(sorted(set(reg))))
        items = []
        for i, r in zip(idx, reg):
            h = host[r]
            items += R.plan_items(h["s2"], h["s1"], h["boundary"], h["band_sel"], plans[r], [i - int(start[r])], [0])
        want = R.host_batch(items, multi)
        for key in ("S2", "S1", "admin_mask", "y", "census_idx"):
            assert bit_equal(s[key].cpu(), want[key].to(s[key].dtype)), (k, key)
        assert s["img_coords"] == [it["img_coords"] for it in items] and s["valid_coords"] == [it["valid_coords"] for it in items]
        assert s.get("census_n") == (want["census_n"] if multi else None)
    assert any(len(r) > 1 for r in seen)                              # batches did mix regions
    with pytest.raises(ValueError, match="seasons"):
        AtlasRegionFeed(atlas, plan, 3, seasons=2)                    # the smallest S of the atlas is 1


@pytest.mark.parametrize("layer", [False, True])
def test_atlas_batch_feed_equals_region_feed_then_prepare(layer):
    from popcorn_amd.cli import prepare_sample_fused
    from popcorn_amd.data.atlas import AtlasBatchFeed, AtlasRegionFeed
    from popcorn_amd.utils.transform import default_train_transform
    _, atlas, plan, _ = _atlas_and_plan(False, layer)
    transform = default_train_transform()
    old = AtlasRegionFeed(atlas, plan, 2, generator=torch.Generator().manual_seed(5))
    new = AtlasBatchFeed(atlas, plan, 2, transform=transform, generator=torch.Generator().manual_seed(5))
    want, rng_w, py_w = _epoch(old, lambda s: dict(prepare_sample_fused(s, transform), region=s["region"]))
    got, rng_g, py_g = _epoch(new, lambda s: s)
    assert torch.equal(new.last_order, old.last_order) and torch.equal(rng_w, rng_g) and py_w == py_g
    assert len(got) == len(want) >= 4
    for g, w in zip(got, want):
        for key in ("raw", "admin_mask", "y", "census_idx") + (("building_counts",) if layer else ()):
            assert g[key].is_cuda and bit_equal(g[key], w[key]), key
        assert g["region"] == w["region"] and ("building_counts" in g) == layer
    # under a pixel budget: every item once, each batch one launch
    feed = AtlasBatchFeed(atlas, plan, 2, generator=torch.Generator().manual_seed(5), pixel_budget=6000, max_batch=8)
    batches = list(feed)
    assert sorted(i for b in feed.last_batches for i in b) == list(range(len(plan)))
    for items, s in zip(feed.last_batches, batches):
        assert s["region"] == plan.region[items].tolist() and torch.equal(s["census_idx"].cpu(), plan.census_idx[items, 0])


def test_planned_repair_over_an_atlas():
    """plan_repair per region with its own ascfill, the tables joined; each batch == augment_raw(fill_sample_(gather with the orbits))."""
    from popcorn_amd.cli import fill_sample_, prepare_sample_fused
    from popcorn_amd.data.atlas import AtlasBatchFeed, AtlasRegionFeed, plan_repair_atlas
    from popcorn_amd.data.region import plan_repair
    from popcorn_amd.utils.transform import default_train_transform
    _, atlas, plan, plans = _atlas_and_plan(False)
    new_plan, rep = plan_repair_atlas(atlas, plan, seasons=1, ascfill=[1])
    alone = [plan_repair(atlas.regions[k], plans[k], seasons=1, ascfill=(k == 1)) for k in range(3)]
    assert set(rep.dropped_by_region) == {0, 1, 2}
    start = np.cumsum([0] + [len(p) for p in plans])
    for k, (p, r) in enumerate(alone):
        assert rep.dropped_by_region[k] == [int(start[k]) + i for i in r.dropped]
    assert torch.equal(rep.orbit, torch.cat([r.orbit for _, r in alone])) and rep.entries == sum(r.entries for _, r in alone) > 0
    assert rep.ascending > 0 and bool(alone[1][1].orbit.any())
    assert torch.equal(new_plan.crops, torch.cat([p.crops for p, _ in alone])) and len(new_plan) == rep.n
    with pytest.raises(ValueError):
        plan_repair_atlas(atlas, plan, ascfill=[3])
    transform = default_train_transform()
    unfused = AtlasRegionFeed(atlas, new_plan, 2, generator=torch.Generator().manual_seed(5), repair=rep)
    fused = AtlasBatchFeed(atlas, new_plan, 2, transform=transform, generator=torch.Generator().manual_seed(5), repair=rep)
    want, _, _ = _epoch(unfused, lambda s: dict(prepare_sample_fused(s, transform), S2=s["S2"], S1=s["S1"], orbit=s["orbit"], region=s["region"]))
    got, _, _ = _epoch(fused, lambda s: s)
    assert len(got) == len(want) >= 4
    patched = 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert bit_equal(g["raw"], w["raw"]) and bit_equal(g["admin_mask"], w["admin_mask"]) and g["orbit"] == w["orbit"]
        assert not bool(torch.isnan(g["raw"]).any())
        # the unfused batch itself: the gather with the planned orbits, filled over each item's own extent
        idx = unfused.last_order[2 * k:2 * k + 2].tolist()
        crops = [new_plan.crops[i].tolist() + [0] for i in idx]
        ref = atlas.gather(w["region"], crops, orbit=w["orbit"])
        patched += int(torch.isnan(ref["S2"]).any() or torch.isnan(ref["S1"]).any())
        fill_sample_(ref["S2"], ref["S1"], ref)
        assert bit_equal(w["S2"], ref["S2"]) and bit_equal(w["S1"], ref["S1"]), k
    assert patched > 0


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
BASE = "-S2 -NIR -S1 -occmodel -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --resident_units 24 --max_steps 3 --save-model no"
TWO = "--resident_region 96 128 120 150"


def _run(tmp_path, tag, extra):
    from popcorn_amd.cli import run_train
    t = run_train((BASE + " " + extra).split() + ["--save_dir", str(tmp_path / tag)])
    torch.cuda.synchronize()
    assert t.info["iter"] == 3 and bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
    return t


@pytest.mark.parametrize("units", [0, 3])
def test_run_train_over_two_regions_with_and_without_the_one_launch_assembly(tmp_path, units):
    from popcorn_amd.data.atlas import AtlasBatchFeed, AtlasPlan, AtlasRegionFeed
    extra = f"-senbuilds {TWO}" + (f" --units_per_crop {units}" if units else "")
    a, b = _run(tmp_path, "plain", extra), _run(tmp_path, "assemble", extra + " --resident_assemble")
    assert type(a._resident_feed) is AtlasRegionFeed and type(b._resident_feed) is AtlasBatchFeed
    assert isinstance(a.region_plan, AtlasPlan) and set(a.region_plan.region.tolist()) == {0, 1} and len(a.regions) == 2
    assert [r.shape for r in a.regions] == [(96, 128), (120, 150)]
    assert torch.equal(a._resident_feed.last_order, b._resident_feed.last_order)
    assert bit_equal(a.fused.loss_out, b.fused.loss_out) and bit_equal(a.fused.flat_p, b.fused.flat_p)


def test_run_train_native_layer_over_two_regions_equals_the_per_launch_step(tmp_path):
    extra = f"{TWO} --resident_assemble --building_layer"
    a, b = _run(tmp_path, "launches", extra), _run(tmp_path, "native", extra + " --native_layer")
    assert a.atlas.layered and b.atlas.layered
    assert bit_equal(a.fused.loss_out, b.fused.loss_out) and bit_equal(a.fused.flat_p, b.fused.flat_p)


@pytest.mark.parametrize("assemble", [False, True])
def test_an_atlas_run_of_one_region_equals_the_single_region_run(tmp_path, assemble):
    from popcorn_amd import cli
    from popcorn_amd.data.atlas import AtlasBatchFeed, AtlasPlan, AtlasRegionFeed, ResidentAtlas
    extra = "-senbuilds --resident_region 96 128" + (" --resident_assemble" if assemble else "")
    a = _run(tmp_path, "region", extra)
    args = cli.train_parser().parse_args((BASE + " " + extra).split() + ["--save_dir", str(tmp_path / "atlas")])
    t = cli.Trainer(args)
    assert t.atlas is None and not isinstance(t.region_plan, AtlasPlan)      # two integers are the single-region run as it was
    atlas, plan, gen = ResidentAtlas([t.region]), AtlasPlan.concat([t.region_plan]), torch.Generator().manual_seed(args.seed)
    if assemble:
        t._resident_feed = AtlasBatchFeed(atlas, plan, 2, transform=t.data_transform, generator=gen)
    else:
        t._resident_feed = AtlasRegionFeed(atlas, plan, 2, generator=gen)
    t.train()
    torch.cuda.synchronize()
    assert t.info["iter"] == 3 and torch.equal(t._resident_feed.last_order, a._resident_feed.last_order)
    assert bit_equal(a.fused.loss_out, t.fused.loss_out) and bit_equal(a.fused.flat_p, t.fused.flat_p)


def test_resident_val_and_test_over_two_regions_report_every_region(tmp_path, capsys):
    """Both regions' keys; region k's metrics are those of a single-region trainer over region k with the same weights."""
    from popcorn_amd import cli
    common = ("-senbuilds --resident_val --resident_test --resident_repair --nan_clouds 0.05 --resident_s1_gap 0.05 --test_patchsize 64 "
              "--test_overlap 8")
    parse = lambda extra, tag: cli.train_parser().parse_args((BASE + " " + common + " " + extra).split() + ["--save_dir", str(tmp_path / tag)])
    t = cli.Trainer(parse(TWO + " --resident_ascfill 1", "two"))
    out = capsys.readouterr().out
    assert "resident validation (region 0):" in out and "resident validation (region 1):" in out and "per region: 0:" in out
    assert t.region_ascfill == [False, True] and len(t.val_sets) == 2 and t.val_sets[1].ascfill and not t.val_sets[0].ascfill
    val, test = dict(t.validate_weak()), dict(t.test_target())
    assert t.valweak_stats == val and t.target_test_stats == test
    assert [w.ascfill for w in t._resident_window_sets] == [False, True]
    for stats_, suffix in ((val, "/val"), (test, "/targettest")):
        assert all(k.endswith(suffix) and v == v for k, v in stats_.items())
        assert {k.split("/")[0] for k in stats_} == {"Population_MainCensus_synthetic0_fine", "Population_MainCensus_synthetic1_fine"}
    for k, (hw, asc) in enumerate((("96 128", ""), ("120 150", " --ascfill"))):
        args = parse(f"--resident_region {hw}{asc}", f"one{k}")
        args.seed += k                                               # region k of the atlas is the raster of seed + 20 + k
        one = cli.Trainer(args)
        assert torch.equal(one.region.boundary, t.regions[k].boundary) and bit_equal(one.region.s1, t.regions[k].s1)
        one.model.load_state_dict(t.model.state_dict())
        v, w = one.validate_weak(), one.test_target()
        assert {key.replace("synthetic_", f"synthetic{k}_"): x for key, x in v.items()} == {key: x for key, x in val.items() if f"synthetic{k}_" in key}
        assert {key.replace("synthetic_", f"synthetic{k}_"): x for key, x in w.items()} == {key: x for key, x in test.items() if f"synthetic{k}_" in key}
    t.train()                                                        # and the run trains on the concatenated train plans
    assert t.info["iter"] == 3 and set(t.region_plan.region.tolist()) == {0, 1}


def test_what_stays_refused(tmp_path):
    from popcorn_amd.cli import run_train
    for extra, word in ((" --fixed_hw 64 64", "--fixed_hw"), (" --torch_optimizer", "--torch_optimizer")):
        with pytest.raises(SystemExit) as e:
            run_train((BASE + " -senbuilds " + TWO + extra).split() + ["--save_dir", str(tmp_path)])
        assert word in str(e.value)
