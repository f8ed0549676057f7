"""The building layer a dataset ships, on the GPU: the `_layer` forms of the five data-movement launches (csrc/train_ops.hip, region.hip,
region_batch.hip, region_crop.hip), the resident feeds and plans, the trainer and the evaluator.

All comparisons are bit for bit (fp32 compared as int32, NaN payloads included).  The sources are those of test_gpu_region_batch.py --
rasters of 37 x 53 (odd width: no source row is 16-byte aligned, the one-pixel form) and 96 x 128 with two seasons, five S2 and three S1
bands and a band selection that is not the identity, uint16 and fp32 S2 -- plus a layer (h, w) holding zeros, whole-numbered counts and
two NaN payloads.  Tiles (40, 56) and 96 x 128 take the four-pixel form with a group straddling the crop's edge; odd rotations at
96 x 128 take twelve LDS tiles per crop; a one-pixel crop sits in the raster's last corner; 130 small crops carry across
PC_REGION_GATHER_MAX_B.  Outputs sit in poisoned memory between the guard bands of tests/footprint.py, and the number of guarded
allocations grows by exactly one more than without the layer."""
import itertools
import random

import numpy as np
import pytest
import torch

from tests import region_oracle as R
from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

S, C2, C1 = 2, 5, 3
BANDS = (4, 0, 2, 1, 2, 0)                                          # not the identity
RASTERS = {"37x53": (37, 53), "96x128": (96, 128)}
PAYLOADS = (0x7FC0ABCD, -0x3FFF55)                                  # quiet NaNs with payloads, the second with the sign bit set
_SRC = {}


def _sources(name, kind):
    """S2 / S1 / boundary as test_gpu_region_batch.py makes them, an ascending S1, and the layer (h, w): about 60 % zeros, counts 1 .. 12,
    two NaN payloads (never the poison's all-ones)."""
    if (name, kind) not in _SRC:
        h, w = RASTERS[name]
        g = torch.Generator().manual_seed(21)
        s2 = torch.randint(0, 10000, (S, C2, h, w), generator=g)
        s2 = s2.to(torch.uint16) if kind == "u16" else s2.float()
        s1 = torch.randn(S, C1, h, w, generator=g) * 5 - 12
        bits = s1.view(torch.int32)
        bits[0, 2, 3:9, 4:40] = 0x7FC12345
        bits[1, 0, h - 7:h, w - 7:w] = -0x3FFFFF
        if kind == "f32":
            s2.view(torch.int32)[1, 4, 10:20, 0:33] = 0x7FC00777
            s2.view(torch.int32)[0, 0, h - 1, w - 1] = 0x7FC00001
        boundary = R.irregular_raster(h, w, units=9, seed=2)
        asc = torch.randn(S, C1, h, w, generator=g) * 5 - 12
        layer = torch.randint(1, 13, (h, w), generator=g).float() * (torch.rand(h, w, generator=g) < 0.4)
        lb = layer.view(torch.int32)
        lb[5, 6:11] = PAYLOADS[0]
        lb[h - 1, w - 1] = PAYLOADS[1]                                # the one-pixel crop in the last corner holds it
        _SRC[(name, kind)] = (s2, s1, boundary, asc, layer)
    return _SRC[(name, kind)]


CASES = {
    "37x53": {
        "crops": {
            "three_odd_origins": [(3, 20, 5, 32, 0), (7, 30, 11, 27, 1), (1, 12, 3, 25, 1)],
            "corners": [(0, 10, 0, 12, 0), (0, 10, 41, 53, 1), (27, 37, 0, 12, 1), (27, 37, 41, 53, 0)],
            "whole_and_one_pixel": [(0, 37, 0, 53, 0), (36, 37, 52, 53, 1), (0, 37, 0, 53, 1)],
        },
        "tiles": [None, (40, 56), (37, 53)],
    },
    "96x128": {
        "crops": {
            "three_odd_origins": [(3, 60, 5, 70, 0), (17, 50, 31, 127, 1), (41, 96, 1, 40, 1)],
            "corners": [(0, 33, 0, 35, 0), (0, 33, 93, 128, 1), (63, 96, 0, 35, 1), (63, 96, 93, 128, 0)],
            "whole_and_one_pixel": [(0, 96, 0, 128, 1), (95, 96, 127, 128, 0), (0, 96, 0, 128, 0)],
        },
        "tiles": [None, (97, 129)],
    },
}
GEOMETRY = list(itertools.product((False, True), (False, True), (0, 1, 2, 3)))        # 16 x (vflip, hflip, rot)
VALUES = [(None, None), (1.3, None), (None, 0.8), (0.7, 1.4)]


def _moved(t, vflip, hflip, rot):
    """out = rot90^rot(hflip(vflip(t))) over the last two axes, with torch on the host"""
    t = t.cpu()
    if vflip:
        t = torch.flip(t, dims=(-2,))
    if hflip:
        t = torch.flip(t, dims=(-1,))
    return torch.rot90(t, rot, dims=(-2, -1)).contiguous()


def _host_layer_tile(layer, crops, Hm, Wm):
    """host slicing plus zero padding to the tile"""
    out = torch.zeros(len(crops), 1, Hm, Wm)
    for b, (x0, x1, y0, y1, _) in enumerate(crops):
        out[b, 0, :x1 - x0, :y1 - y0] = layer[x0:x1, y0:y1]
    return out


# ---- augment_raw ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 37, 53), (2, 40, 56), (3, 96, 128)])
def test_augment_raw_moves_the_layer_like_the_admin_mask(shape):
    from popcorn_amd import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(B * H + W)
    s2 = torch.randint(0, 10000, (B, 4, H, W), generator=g).float()
    s1 = torch.randn(B, 2, H, W, generator=g) * 5 - 12
    admin = torch.randint(0, 9, (B, H, W), generator=g).float()
    layer = torch.randint(1, 13, (B, 1, H, W), generator=g).float() * (torch.rand(B, 1, H, W, generator=g) < 0.4)
    layer.view(torch.int32)[0, 0, 2, 3:8] = PAYLOADS[0]
    layer.view(torch.int32)[B - 1, 0, H - 1, W - 1] = PAYLOADS[1]
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, da, dl = fp.place(s2), fp.place(s1), fp.place(admin), fp.place(layer)
        for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES[:1] + VALUES[3:]):
            params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
            n0 = fp.guarded
            raw0, adm0 = ops.augment_raw(d2, d1, da, params)
            n1 = fp.guarded
            got = ops.augment_raw(d2, d1, da, params, buildings=dl)
            assert fp.guarded - n1 == (n1 - n0) + 1 == 3             # exactly one more than without the layer
            assert len(got) == 3 and tuple(got[2].shape) == (B, 1) + ((W, H) if rot & 1 else (H, W))
            assert bit_equal(got[2].cpu(), _moved(layer, vflip, hflip, rot)), params
            assert bit_equal(got[0], raw0) and bit_equal(got[1], adm0), params          # unchanged by the layer's presence
            for payload in PAYLOADS:
                assert bool((got[2].view(torch.int32) == payload).any())
        out = fp.alloc((B, 1, W, H))
        assert ops.augment_raw(d2, d1, da, {"rot": 1}, buildings=dl, buildings_out=out)[2] is out
        assert bit_equal(out.cpu(), _moved(layer, False, False, 1))
    with pytest.raises(ValueError):
        ops.augment_raw(d2, d1, da, None, buildings=dl[:, 0])
    with pytest.raises(ValueError):
        ops.augment_raw(d2, d1, da, None, buildings_out=out)


# ---- region_gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_region_gather_layer_equals_host_slicing(name, kind):
    from popcorn_amd import ops
    s2, s1, boundary, asc, layer = _sources(name, kind)
    for case, crops in CASES[name]["crops"].items():
        orbit = [b & 1 for b in range(len(crops))]
        for hw in CASES[name]["tiles"]:
            with Footprint("cuda", fill=POISON) as fp:
                d2, d1, db, da, dl = fp.place(s2), fp.place(s1), fp.place(boundary), fp.place(asc), fp.place(layer)
                for kw in ({}, {"s1_asc": da, "orbit": orbit}):
                    B = len(crops)
                    outs = [None, None]
                    if hw is not None:
                        for k in (0, 1):
                            outs[k] = {"S2": fp.alloc((B, 4) + hw), "S1": fp.alloc((B, 2) + hw), "admin_mask": fp.alloc((B,) + hw),
                                       "data_hw": fp.alloc((B, 2), torch.int32)}
                        outs[1]["building_counts"] = fp.alloc((B, 1) + hw)
                    n0 = fp.guarded
                    plain = ops.region_gather(d2, d1, db, BANDS, crops, out=outs[0], **kw)
                    n1 = fp.guarded
                    got = ops.region_gather(d2, d1, db, BANDS, crops, out=outs[1], buildings=dl, **kw)
                    if hw is None:
                        assert fp.guarded - n1 == (n1 - n0) + 1 == 5
                    Hm, Wm = got["admin_mask"].shape[1:]
                    what = (case, hw, bool(kw))
                    assert bit_equal(got["building_counts"].cpu(), _host_layer_tile(layer, crops, Hm, Wm)), what
                    for key in ("S2", "S1", "admin_mask", "data_hw"):
                        assert bit_equal(got[key], plain[key]) if key != "data_hw" else torch.equal(got[key], plain[key]), (key, what)
                    assert "building_counts" not in plain


@pytest.mark.parametrize("rot", [0, 3])
def test_more_crops_than_one_launch_carry_the_layer(rot):
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    assert L.PC_REGION_GATHER_MAX_B == 128
    g = torch.Generator().manual_seed(4)
    crops = []
    for _ in range(130):
        x0, y0 = int(torch.randint(0, 29, (1,), generator=g)), int(torch.randint(0, 45, (1,), generator=g))
        crops.append((x0, x0 + 1 + int(torch.randint(0, 8, (1,), generator=g)), y0, y0 + 1 + int(torch.randint(0, 8, (1,), generator=g)),
                      int(torch.randint(0, S, (1,), generator=g))))
    s2, s1, boundary, asc, layer = _sources("37x53", "u16")
    params = {"vflip": True, "hflip": False, "rot": rot, "beta": 1.2, "gamma": None}
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db, dl = fp.place(s2), fp.place(s1), fp.place(boundary), fp.place(layer)
        tile = ops.region_gather(d2, d1, db, BANDS, crops, buildings=dl)
        Hm, Wm = tile["admin_mask"].shape[1:]
        assert bit_equal(tile["building_counts"].cpu(), _host_layer_tile(layer, crops, Hm, Wm))
        raw, adm, bc = ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params, buildings=tile["building_counts"])
        got = ops.region_batch(d2, d1, db, BANDS, crops, params, buildings=dl)
    # (the crops of the second launch land behind the first's: the host tile above and the composite below cover all 130)
    assert bit_equal(got["raw"], raw) and bit_equal(got["admin_mask"], adm) and bit_equal(got["building_counts"], bc)


# ---- region_batch -----------------------------------------------------------------------------------------------------------------------
def _composite(d2, d1, db, dl, crops, params, hw, kw):
    from popcorn_amd import ops
    if hw is None:
        tile = ops.region_gather(d2, d1, db, BANDS, crops, buildings=dl, **kw)
    else:
        B = len(crops)
        tile = {"S2": torch.empty(B, 4, *hw, device="cuda"), "S1": torch.empty(B, 2, *hw, device="cuda"),
                "admin_mask": torch.empty(B, *hw, device="cuda"), "data_hw": torch.empty(B, 2, dtype=torch.int32, device="cuda"),
                "building_counts": torch.empty(B, 1, *hw, device="cuda")}
        ops.region_gather(d2, d1, db, BANDS, crops, out=tile, buildings=dl, **kw)
    return tile, ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params, buildings=tile["building_counts"])


@pytest.mark.parametrize("orbits", [False, True])
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_region_batch_layer_equals_gather_then_augment(name, kind, orbits):
    from popcorn_amd import ops
    s2, s1, boundary, asc, layer = _sources(name, kind)
    checked = 0
    for case, crops in CASES[name]["crops"].items():
        for hw in CASES[name]["tiles"]:
            with Footprint("cuda", fill=POISON) as fp:
                d2, d1, db, da, dl = fp.place(s2), fp.place(s1), fp.place(boundary), fp.place(asc), fp.place(layer)
                kw = {"s1_asc": da, "orbit": [(b + 1) & 1 for b in range(len(crops))]} if orbits else {}
                for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES):
                    params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
                    tile, (raw, adm, bc) = _composite(d2, d1, db, dl, crops, params, hw, kw)
                    n0 = fp.guarded
                    got = ops.region_batch(d2, d1, db, BANDS, crops, params, hw=hw, buildings=dl, **kw)
                    assert fp.guarded == n0 + 3                                   # raw, admin_mask and one more: the layer
                    Hm, Wm = tile["admin_mask"].shape[1:]
                    assert tuple(got["building_counts"].shape) == (len(crops), 1) + ((Wm, Hm) if rot & 1 else (Hm, Wm))
                    what = (case, hw, params)
                    assert bit_equal(got["raw"], raw) and bit_equal(got["admin_mask"], adm), what
                    assert bit_equal(got["building_counts"], bc), what
                    checked += 1
                    if beta is None and gamma is None:
                        # against torch on the host as well, and the call without a layer keeps its bits
                        assert bit_equal(got["building_counts"].cpu(), _moved(_host_layer_tile(layer, crops, Hm, Wm), vflip, hflip, rot)), what
                        plain = ops.region_batch(d2, d1, db, BANDS, crops, params, hw=hw, **kw)
                        assert "building_counts" not in plain and bit_equal(plain["raw"], raw) and bit_equal(plain["admin_mask"], adm)
                        if case == "whole_and_one_pixel":
                            for payload in PAYLOADS:                              # NaN payloads arrive bit for bit
                                assert bool((got["building_counts"].view(torch.int32) == payload).any()), (payload, what)
    assert checked == 64 * len(CASES[name]["crops"]) * len(CASES[name]["tiles"])


def test_layer_refusals_of_the_wrappers():
    from popcorn_amd import ops
    s2, s1, boundary, asc, layer = (t.cuda() for t in _sources("37x53", "f32"))
    good = [(3, 20, 5, 32, 0)]
    for bad in (layer[:, :52], layer.double(), layer.t(), layer.cpu()):
        with pytest.raises((ValueError, RuntimeError)):
            ops.region_gather(s2, s1, boundary, BANDS, good, buildings=bad)
        with pytest.raises((ValueError, RuntimeError)):
            ops.region_batch(s2, s1, boundary, BANDS, good, buildings=bad)
    out = ops.region_batch(s2, s1, boundary, BANDS, good)
    with pytest.raises(ValueError):                                  # an ``out`` without the layer's slot
        ops.region_batch(s2, s1, boundary, BANDS, good, out=out, buildings=layer)
    with pytest.raises(ValueError):
        ops.region_window(s2, s1, BANDS, (0, 0, 0), 8, [0.0] * 6, [1.0] * 6, buildings_out=torch.empty(8, 8, device="cuda"))


# ---- region_window / region_item --------------------------------------------------------------------------------------------------------
def _stats():
    from popcorn_amd.data import stats
    return stats.MEAN6, stats.STD6


def _crop_table(d2, d1, da, db, crop, orbit):
    """The patch table of one crop as the plans build it: gather, fill on a clone, extract."""
    from popcorn_amd import ops
    t = ops.region_gather(d2, d1, db, BANDS, [crop], s1_asc=da, orbit=[orbit])
    f2, f1 = t["S2"].clone(), t["S1"].clone()
    ops.nan_fill_(f2, t["data_hw"])
    ops.nan_fill_(f1, t["data_hw"])
    idx, val, _ = ops.region_patch_extract(t, {"S2": f2, "S1": f1})
    return idx, val


def _eq_nan(a, b):
    """bit-equal where neither is NaN, NaN at the same sites (a normalised NaN's payload is the division's)"""
    an, bn = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and bool(torch.equal(an, bn)) and bool((a.view(torch.int32)[~an] == b.view(torch.int32)[~bn]).all())


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("ps", [32, 33, 36])
def test_region_window_layer_is_the_raster_slice(ps, with_table):
    from popcorn_amd import ops
    s2, s1, boundary, asc, layer = _sources("96x128", "f32")
    H, W = RASTERS["96x128"]
    mean6, std6 = _stats()
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db, da, dl = fp.place(s2), fp.place(s1), fp.place(boundary), fp.place(asc), fp.place(layer)
        for (x, y), orbit, season in [(o, b, s) for o in ((0, 0), (1, 3), (H - ps, W - ps)) for b in (0, 1) for s in (0, 1)]:
            table = None
            if with_table:
                idx, val = _crop_table(d2, d1, da, db, (x, x + ps, y, y + ps, season), orbit)
                table = (idx, val, 0, idx.numel())
            kw = dict(s1_asc=da, orbit=orbit, table=table)
            n0 = fp.guarded
            plain = ops.region_window(d2, d1, BANDS, (x, y, season), ps, mean6, std6, **kw)
            n1 = fp.guarded
            got, bc = ops.region_window(d2, d1, BANDS, (x, y, season), ps, mean6, std6, buildings=dl, **kw)
            assert fp.guarded - n1 == (n1 - n0) + 1 == 2
            want = layer[x:x + ps, y:y + ps].reshape(1, 1, ps, ps).contiguous()
            assert tuple(bc.shape) == (1, 1, ps, ps) and bit_equal(bc.cpu(), want), (x, y, orbit, season)
            assert _eq_nan(got, plain), (x, y, orbit, season)
            # 4-byte aligned layer output only: the element-by-element path at any ps, the same bits
            shifted = torch.full((ps * ps + 1,), 123.0, device="cuda")[1:].view(ps, ps)
            got2, bc2 = ops.region_window(d2, d1, BANDS, (x, y, season), ps, mean6, std6, buildings=dl, buildings_out=shifted, **kw)
            assert bit_equal(shifted.cpu(), want[0, 0]) and _eq_nan(got2, plain) and bc2.data_ptr() == shifted.data_ptr()


ITEM_CROPS = {"odd_y0_wc31": (3, 20, 5, 36), "odd_y0_wc28": (2, 30, 7, 35), "corner_top_left": (0, 10, 0, 12),
              "corner_top_right": (0, 10, 53 - 12, 53), "corner_bottom_left": (37 - 10, 37, 0, 12),
              "corner_bottom_right": (37 - 9, 37, 53 - 13, 53), "whole_raster": (0, 37, 0, 53), "one_pixel": (17, 18, 23, 24),
              "last_corner_pixel": (36, 37, 52, 53)}


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_region_item_layer_is_the_raster_slice(kind, with_table):
    from popcorn_amd import ops
    s2, s1, boundary, asc, layer = _sources("37x53", kind)
    mean6, std6 = _stats()
    seen = set()
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db, da, dl = fp.place(s2), fp.place(s1), fp.place(boundary), fp.place(asc), fp.place(layer)
        for k, (name, (x0, x1, y0, y1)) in enumerate(ITEM_CROPS.items()):
            crop, orbit = (x0, x1, y0, y1, k & 1), (k >> 1) & 1
            table = None
            if with_table:
                idx, val = _crop_table(d2, d1, da, db, crop, orbit)
                table = (idx, val, 0, idx.numel())
            kw = dict(s1_asc=da, orbit=orbit, table=table)
            n0 = fp.guarded
            plain = ops.region_item(d2, d1, db, BANDS, crop, mean6, std6, **kw)
            n1 = fp.guarded
            got = ops.region_item(d2, d1, db, BANDS, crop, mean6, std6, buildings=dl, **kw)
            assert fp.guarded - n1 == (n1 - n0) + 1 == 3
            hc, wc = x1 - x0, y1 - y0
            want = layer[x0:x1, y0:y1].reshape(1, 1, hc, wc).contiguous()
            assert len(plain) == 2 and len(got) == 3 and tuple(got[2].shape) == (1, 1, hc, wc)
            assert bit_equal(got[2].cpu(), want), name
            assert _eq_nan(got[0], plain[0]) and bit_equal(got[1], plain[1]), name
            seen |= {p for p in PAYLOADS if bool((got[2].view(torch.int32) == p).any())}
            shifted = torch.full((hc * wc + 1,), 123.0, device="cuda")[1:].view(hc, wc)
            got2 = ops.region_item(d2, d1, db, BANDS, crop, mean6, std6, buildings=dl, buildings_out=shifted, **kw)
            assert bit_equal(shifted.cpu(), want[0, 0]) and _eq_nan(got2[0], plain[0]) and bit_equal(got2[1], plain[1]), name
    assert seen == set(PAYLOADS)


# ---- the resident feeds -----------------------------------------------------------------------------------------------------------------
def _region_and_plan():
    from popcorn_amd.data.region import ResidentRegion, plan_one_unit
    if "region" not in _SRC:
        s2, s1, boundary, asc, layer = _sources("96x128", "f32")
        ids, pop = torch.arange(1, 10), torch.rand(9, generator=torch.Generator().manual_seed(3)) * 2000
        region = ResidentRegion(s2, s1, boundary, ids, pop, band_sel=BANDS, device="cuda", buildings=layer)
        assert region.buildings.is_cuda and region.buildings.dtype == torch.float32 and bit_equal(region.buildings.cpu(), layer)
        with pytest.raises(ValueError):
            ResidentRegion(s2, s1, boundary, ids, pop, band_sel=BANDS, device="cuda", buildings=layer[:, :100])
        _SRC["region"] = (region, plan_one_unit(region.table, ids, pop, region.shape, admin_overlap=4))
    return _SRC["region"]


def _host_sample(plan, items, seasons):
    """dataset item -> collate, from host slicing of the sources on the plan's crops"""
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    s2, s1, boundary, asc, layer = _sources("96x128", "f32")
    batch = []
    for i, s in zip(items, seasons):
        x0, x1, y0, y1 = (int(v) for v in plan.crops[i])
        batch.append({"S2": s2[s, list(BANDS[:4]), x0:x1, y0:y1], "S1": s1[s, list(BANDS[4:]), x0:x1, y0:y1],
                      "admin_mask": boundary[x0:x1, y0:y1].float(), "building_counts": layer[None, x0:x1, y0:y1],
                      "y": plan.y[i, 0], "census_idx": plan.census_idx[i, :1], "img_coords": (0, 0), "valid_coords": (0, 0), "season": int(s)})
    host = Population_Dataset_collate_fn(batch)
    # the collate's zeros() * NaN-free copy keeps payloads: a slice assignment copies bits
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}


def _epoch(feed, prepare):
    torch.manual_seed(11)
    random.seed(11)
    out = []
    for sample in feed:
        s = prepare(sample)
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()})
        torch.rand(1)
    return out


def _step_model():
    from popcorn_amd.model.popcorn import POPCORN
    from popcorn_amd.train import FusedTrainStep
    from popcorn_amd.data import stats
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=False).cuda()
    return FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, scale_regularization=0.01,
                          raw_norm=(tuple(range(6)), stats.MEAN6, stats.STD6))


@pytest.mark.parametrize("feed_name", ["ResidentRegionFeed", "ResidentBatchFeed"])
def test_resident_feed_layer_equals_the_host_path(feed_name):
    from popcorn_amd.cli import prepare_sample_fused
    from popcorn_amd.data import region as DR
    from popcorn_amd.utils.transform import default_train_transform
    region, plan = _region_and_plan()
    transform = default_train_transform()
    B = 2
    if feed_name == "ResidentRegionFeed":
        feed = DR.ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2)
        got = _epoch(feed, lambda s: prepare_sample_fused(s, transform))
    else:
        feed = DR.ResidentBatchFeed(region, plan, B, transform=transform, generator=torch.Generator().manual_seed(5), seasons=2)
        got = _epoch(feed, lambda s: s)
    order, season = feed.last_order.tolist(), feed.last_season.tolist()
    host = [_host_sample(plan, order[k * B:(k + 1) * B], season[k * B:(k + 1) * B]) for k in range(len(got))]
    want = _epoch(host, lambda s: prepare_sample_fused(s, transform))
    assert len(got) == len(want) >= 2
    shapes = set()
    for g, w in zip(got, want):
        for key in ("raw", "admin_mask", "building_counts", "y"):
            assert g[key].is_cuda and bit_equal(g[key].contiguous(), w[key].contiguous()), key
        assert torch.equal(g["census_idx"].view(-1), w["census_idx"].view(-1))
        assert tuple(g["building_counts"].shape) == (B, 1) + tuple(g["raw"].shape[2:])
        shapes.add(tuple(g["raw"].shape[2:]))
    assert len(shapes) > 1                                           # the coins and sizes did vary over the epoch
    # a fused step on either: equal bits in loss and parameters, and the layer that reached the step is the one that was fed
    res = []
    for s in (got[0], want[0]):
        tr = _step_model()
        fed = s["building_counts"].clone()
        torch.manual_seed(5)
        loss = tr.step({k: s[k] for k in ("raw", "admin_mask", "census_idx", "y", "building_counts")}).clone()
        torch.cuda.synchronize()
        assert tr.native_steps == 0                                  # a given layer goes to the per-launch engine
        assert bit_equal(tr.last["building_counts"].reshape(fed.shape).contiguous(), fed)      # not the extractor's score
        res.append((loss, tr.flat_p.clone()))
    assert bool(torch.isfinite(res[0][0]).all()) and bit_equal(res[0][0], res[1][0]) and bit_equal(res[0][1], res[1][1])


def test_normalize_sample_turns_the_layer_with_the_admin_mask():
    """The general transform on the stacked {admin mask, layer} (utils/utils.py:182-209) against the one-launch form under the same coins."""
    from popcorn_amd.cli import normalize_sample, prepare_sample_fused
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.dataset import SyntheticWeaksupDataset
    from popcorn_amd.utils.transform import default_train_transform
    ds = SyntheticWeaksupDataset(6, min_hw=24, max_hw=48, seed=5, buildings=True)
    transform = default_train_transform()
    turned = 0
    for k in range(6):
        host = Population_Dataset_collate_fn([ds[k], ds[(k + 1) % 6]])
        dev = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in host.items()}
        torch.manual_seed(30 + k)
        random.seed(30 + k)
        a = normalize_sample(host, torch.device("cuda"), transform)
        torch.manual_seed(30 + k)
        random.seed(30 + k)
        b = prepare_sample_fused(dev, transform)
        assert tuple(a["building_counts"].shape) == (2, 1) + tuple(a["input"].shape[2:])
        assert bit_equal(a["building_counts"], b["building_counts"]) and bit_equal(a["admin_mask"], b["admin_mask"]), k
        turned += int(not (a["building_counts"].shape == host["building_counts"].shape and
                           bit_equal(a["building_counts"].cpu(), host["building_counts"])))
        plain = normalize_sample({key: v for key, v in host.items() if key != "building_counts"}, torch.device("cuda"), None)
        assert "building_counts" not in plain
    assert turned >= 2                                               # the coins did move the layer


def test_resident_items_carry_the_layer():
    from popcorn_amd.data.region import ResidentItems
    region, plan = _region_and_plan()
    layer = _sources("96x128", "f32")[4]
    items = ResidentItems(region, plan, seasons=2, generator=torch.Generator().manual_seed(2))
    n = 0
    for k, s in enumerate(items):
        x0, x1, y0, y1 = (int(v) for v in items.plan.crops[k])
        assert tuple(s["building_counts"].shape) == (1, 1, x1 - x0, y1 - y0)
        assert bit_equal(s["building_counts"].cpu(), layer[x0:x1, y0:y1].reshape(1, 1, x1 - x0, y1 - y0).contiguous())
        n += 1
    assert n == len(items) >= 2


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
TRAIN = "-S2 -NIR -S1 -occmodel -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --max_steps 3 --save-model no"
RESIDENT = "--resident_region 192 256 --resident_units 24"


def _train(tmp_path, tag, extra):
    from popcorn_amd.cli import run_train
    t = run_train(TRAIN.split() + ["--save_dir", str(tmp_path / tag)] + extra.split())
    torch.cuda.synchronize()
    assert t.info["iter"] == 3
    return t, t.fused.loss_out.clone(), t.fused.flat_p.clone()


def test_run_train_building_layer_on_the_resident_feeds(tmp_path):
    """--building_layer on --resident_region and on --resident_assemble: equal bits in loss and parameters, other bits than without the
    flag, and no step through the native executor."""
    runs = {}
    for tag, extra in (("region", RESIDENT + " --building_layer"), ("assemble", RESIDENT + " --resident_assemble --building_layer"),
                       ("plain", RESIDENT)):
        runs[tag] = _train(tmp_path, tag, extra)
    for tag in ("region", "assemble"):
        t, loss, p = runs[tag]
        assert t.region.buildings is not None and t.fused.native_steps == 0
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all())
    assert runs["plain"][0].region.buildings is None and runs["plain"][0].fused.native_steps == 3
    assert bit_equal(runs["region"][1], runs["assemble"][1]) and bit_equal(runs["region"][2], runs["assemble"][2])
    assert not bit_equal(runs["region"][1], runs["plain"][1]) and not bit_equal(runs["region"][2], runs["plain"][2])


def test_run_train_building_layer_on_the_host_feed_with_validation_and_test(tmp_path):
    """The host feed (dataset item -> collate -> staged batch -> prepare_sample_fused) with -wv validation and the in-training target
    test: the layer reaches every one of them."""
    common = " --synthetic_regions 8 --synthetic_val_regions 3 --synthetic_hw_range 48 80 -wv -vi 2 -testi 3 --test_raster_hw 96 128 " \
             "--test_patchsize 64 --test_overlap 8"
    t, loss, p = _train(tmp_path, "layer", "--building_layer" + common)
    assert t.fused.native_steps == 0 and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all())
    assert t._test_raster.buildings is not None and t.valweak_stats and t.target_test_stats
    assert all(np.isfinite(v) for v in t.valweak_stats.values()) and all(np.isfinite(v) for v in t.target_test_stats.values())
    t0, loss0, p0 = _train(tmp_path, "plain", common.strip())
    assert t0.fused.native_steps == 3 and t0._test_raster.buildings is None
    assert not bit_equal(loss, loss0) and not bit_equal(p, p0)
    assert t.target_test_stats != t0.target_test_stats and t.valweak_stats != t0.valweak_stats


def test_run_train_building_layer_resident_val_and_test(tmp_path):
    """--resident_val and --resident_test over a region with a layer: items and windows hand it to the model."""
    t, loss, p = _train(tmp_path, "resident", RESIDENT + " --building_layer --resident_val --resident_test -wv -vi 2 -testi 3 "
                        "--test_patchsize 64 --test_overlap 8")
    assert t.fused.native_steps == 0 and bool(torch.isfinite(loss).all())
    assert t._resident_windows.window_buildings is not None and tuple(t._resident_windows.window_buildings.shape) == (1, 1, 64, 64)
    assert all(np.isfinite(v) for v in t.valweak_stats.values()) and all(np.isfinite(v) for v in t.target_test_stats.values())


@pytest.mark.parametrize("where", ["host", "resident"])
def test_run_train_building_layer_with_multi_unit_crops(tmp_path, where):
    """--units_per_crop with a layer, on the synthetic multi-unit host dataset and on the resident region's multi-unit plan."""
    extra = "--units_per_crop 3 " + ("--synthetic_regions 8 --synthetic_hw_range 48 80" if where == "host" else RESIDENT)
    t, loss, p = _train(tmp_path, "layer", extra + " --building_layer")
    t0, loss0, p0 = _train(tmp_path, "plain", extra)
    assert t.fused.native_steps == 0 and t.fused.native_unit_steps == 0
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all())
    assert not bit_equal(loss, loss0) and not bit_equal(p, p0)


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------
EH, EW, EPS, EOV = 96, 128, 64, 8


def _members(senbuilds, n=2):
    from popcorn_amd.model.popcorn import POPCORN
    out = []
    for k in range(n):
        torch.manual_seed(40 + k)
        out.append(POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=senbuilds).cuda().eval())
    return out


def _eval_data():
    if "eval" not in _SRC:
        from popcorn_amd.data.dataset import SyntheticTestRaster
        _SRC["eval"] = SyntheticTestRaster(EH, EW, seasons=1, n_regions=16, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.05,
                                           buildings=True)
    return _SRC["eval"]


def test_evaluate_raster_with_a_layer_equals_the_hand_loop():
    from popcorn_amd import _lib as L
    from popcorn_amd import eval as E
    data = _eval_data()
    layer = data.buildings
    models = _members(False)
    raster = torch.randn(1, 6, EH, EW, generator=torch.Generator().manual_seed(7)).cuda()
    got = E.evaluate_raster(models, raster, EPS, EOV, False, buildings=layer)
    plain = E.evaluate_raster(models, raster, EPS, EOV, False)
    st = E.Stitcher(EH, EW, raster.device)
    for x, y, s in E.get_patch_indices(EH, EW, EPS, EOV, False).tolist():
        sample_layer = layer[x:x + EPS, y:y + EPS].reshape(1, 1, EPS, EPS).contiguous()
        pds, scs = [], []
        with torch.no_grad(), L.padded_rows():
            for m in models:
                o = m({"input": raster[s:s + 1, :, x:x + EPS, y:y + EPS].contiguous(), "building_counts": sample_layer}, padding=False)
                pds.append(o["popdensemap"][0])
                scs.append(o["scale"][0])
        st.add_window(x, y, torch.stack(pds), torch.stack(scs), EOV)
    want = st.finalize()
    for a, b in zip(got, want):
        assert bit_equal(a, b)
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().sum()) > 0
    assert not bit_equal(got[0], plain[0])
    # the layer zeroes the occupancy product wherever it is zero
    assert bool((got[0][layer == 0] == 0).all()) and bool((plain[0][layer == 0] != 0).any())
    with pytest.raises(ValueError):
        E.evaluate_raster(models, raster, EPS, EOV, False, buildings=layer[:, :100])


def test_members_built_with_sentinelbuildings_ignore_the_layer():
    from popcorn_amd import eval as E
    data = _eval_data()
    models = _members(True)
    raster = torch.randn(1, 6, EH, EW, generator=torch.Generator().manual_seed(7)).cuda()
    a = E.evaluate_raster(models, raster, EPS, EOV, False, buildings=data.buildings)
    b = E.evaluate_raster(models, raster, EPS, EOV, False)
    for u, v in zip(a, b):
        assert bit_equal(u, v)


def test_resident_windows_hand_over_the_layer_from_the_windows_own_launch(monkeypatch):
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd.data.region import ResidentRegion, ResidentWindows
    data = _eval_data()
    models = _members(False)
    region = ResidentRegion.from_synthetic(data, with_asc=True)
    assert region.buildings is not None and bit_equal(region.buildings, data.buildings)
    want = E.evaluate_raster(models, data.raster, EPS, EOV, False, raw=True, buildings=data.buildings,
                             product=(p_raw := E.ProductGrid(EH, EW, 10, 2, "cuda")),
                             census=(c_raw := E.CensusTable(EH, EW, [data.boundary], [17], 2, "cuda")))
    feed = ResidentWindows(region, EPS, EOV)
    calls = []
    real = ops.region_window

    def counted(*a, **k):
        calls.append(k.get("buildings") is not None)
        return real(*a, **k)

    monkeypatch.setattr(ops, "region_window", counted)
    got = E.evaluate_raster(models, feed, EPS, EOV, False, product=(p_res := E.ProductGrid(EH, EW, 10, 2, "cuda")),
                            census=(c_res := E.CensusTable(EH, EW, [data.boundary], [17], 2, "cuda")))
    n = E.get_patch_indices(EH, EW, EPS, EOV, False).shape[0]
    assert len(calls) == n and all(calls)                            # one launch per window, the layer in it
    for a, b in zip(got, want):
        assert bit_equal(a, b)
    assert bit_equal(p_raw.mean, p_res.mean) and bit_equal(p_raw.std, p_res.std) and bit_equal(p_raw.cells, p_res.cells)
    assert torch.equal(c_raw.table, c_res.table) and bit_equal(c_raw.mean, c_res.mean) and bit_equal(c_raw.std, c_res.std)
    no_layer = E.evaluate_raster(models, ResidentWindows(ResidentRegion(data.s2, data.s1, data.boundary, data.census_idx, data.census_pop,
                                                                        band_sel=(0, 1, 2, 3, 0, 1), s1_asc=data.s1_asc), EPS, EOV),
                                 EPS, EOV, False)
    assert not bit_equal(no_layer[0], got[0])


def test_layer_fed_member_agrees_with_the_oracle():
    """One forward on a given layer against the oracle's on the same building_counts, at the bar of test_gpu_model.py's given-layer case:
    1e-5 * max(1, |reference|) on the scalar it compares (there the loss, here every popcount)."""
    from oracle import popcorn_oracle as O
    from popcorn_amd.data.synthetic import make_raw_batch
    m = _members(False, 1)[0]
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    b = make_raw_batch(2, 100, 100, seed=3, region="disc")
    layer = torch.randint(0, 13, (2, 1, 100, 100), generator=torch.Generator().manual_seed(4)).float() * \
        (torch.rand(2, 1, 100, 100, generator=torch.Generator().manual_seed(5)) < 0.4)
    cpu = {"input": O.select_normalize(b["raw"]), "admin_mask": b["admin_mask"], "census_idx": b["census_idx"], "building_counts": layer}
    with torch.no_grad():
        got = m({k: v.cuda() for k, v in cpu.items()}, padding=False)
        ref = O.popcorn_forward(sd, {k: v.clone() for k, v in cpu.items()}, padding=False, sparse=False, occupancymodel=True,
                                sentinelbuildings=False)
    for g, r in zip(got["popcount"].cpu().tolist(), ref["popcount"].tolist()):
        print("popcount", g, r)
        assert abs(g - r) < 1e-5 * max(1.0, abs(r)), (g, r)
