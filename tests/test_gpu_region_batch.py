"""One-launch batch assembly on the GPU (csrc/region_batch.hip and everything above it).

The oracle of ``ops.region_batch`` is the pair it replaces, bit for bit (fp32 compared as int32, NaN payloads included):

    raw, admin_mask  ==  ops.augment_raw(*ops.region_gather(..., out=tile of (Hm, Wm)), params)

on rasters of 37 x 53 (odd width: no source row is 16-byte aligned) and 96 x 128 with two seasons, five S2 and three S1 bands and a band
selection that is not the identity.  A tile width that is a multiple of four takes the four-pixel form (16-byte stores, a group that
straddles the crop's edge element by element), any other the one-pixel form; an odd rotation takes 32 x 32 tiles through LDS, of which a
96 x 128 tile has twelve per crop.  The outputs sit in poisoned memory between the guard bands of tests/footprint.py: every element is
proven written, nothing outside is touched.  Above the op: the labels against torch indexing, the refusals, ``ResidentBatchFeed`` against
``ResidentRegionFeed`` + ``prepare_sample_fused``, and the trainer flags against the unfused resident feed."""
import ctypes as C
import itertools
import random

import pytest
import torch

from tests import region_oracle as R
from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

S, C2, C1 = 2, 5, 3
BANDS = (4, 0, 2, 1, 2, 0)                                          # not the identity
RASTERS = {"37x53": (37, 53), "96x128": (96, 128)}
_SRC = {}


def _sources(name, kind):
    """S2 (S, C2, h, w) as uint16 or fp32, S1 fp32, boundary int32; the fp32 sources hold NaNs with payloads (never the poison's all-ones)."""
    if (name, kind) not in _SRC:
        h, w = RASTERS[name]
        g = torch.Generator().manual_seed(21)
        s2 = torch.randint(0, 10000, (S, C2, h, w), generator=g)
        s2 = s2.to(torch.uint16) if kind == "u16" else s2.float()
        s1 = torch.randn(S, C1, h, w, generator=g) * 5 - 12
        bits = s1.view(torch.int32)
        bits[0, 2, 3:9, 4:40] = 0x7FC12345                          # quiet NaN, payload
        bits[1, 0, h - 7:h, w - 7:w] = -0x3FFFFF                    # 0xFFC00001: negative quiet NaN, payload
        if kind == "f32":
            s2.view(torch.int32)[1, 4, 10:20, 0:33] = 0x7FC00777
            s2.view(torch.int32)[0, 0, h - 1, w - 1] = 0x7FC00001
        boundary = R.irregular_raster(h, w, units=9, seed=2)
        _SRC[(name, kind)] = (s2, s1, boundary)
    return _SRC[(name, kind)]


# crops {x0, x1, y0, y1, season} and the tiles (Hm, Wm) they are gathered at (None: the batch maximum)
CASES = {
    "37x53": {
        "crops": {
            "three_odd_origins": [(3, 20, 5, 32, 0), (7, 30, 11, 27, 1), (1, 12, 3, 25, 1)],                     # maximum 23 x 27: one pixel
            "corners": [(0, 10, 0, 12, 0), (0, 10, 41, 53, 1), (27, 37, 0, 12, 1), (27, 37, 41, 53, 0)],        # 10 x 12: four pixels
            "whole_and_one_pixel": [(0, 37, 0, 53, 0), (36, 37, 52, 53, 1), (0, 37, 0, 53, 1)],         # both seasons whole
        },
        "tiles": [None, (40, 56), (37, 53)],                        # larger than every crop: four pixels; one pixel
    },
    "96x128": {
        "crops": {
            "three_odd_origins": [(3, 60, 5, 70, 0), (17, 50, 31, 127, 1), (41, 96, 1, 40, 1)],                # maximum 57 x 96
            "corners": [(0, 33, 0, 35, 0), (0, 33, 93, 128, 1), (63, 96, 0, 35, 1), (63, 96, 93, 128, 0)],    # 33 x 35
            "whole_and_one_pixel": [(0, 96, 0, 128, 1), (95, 96, 127, 128, 0), (0, 96, 0, 128, 0)],
        },
        "tiles": [None, (97, 129)],
    },
}
GEOMETRY = list(itertools.product((False, True), (False, True), (0, 1, 2, 3)))        # 16 x (vflip, hflip, rot)
VALUES = [(None, None), (1.3, None), (None, 0.8), (0.7, 1.4)]                          # no change, beta, gamma, both


def _composite(d2, d1, db, crops, params, hw):
    from popcorn_amd import ops
    if hw is None:
        tile = ops.region_gather(d2, d1, db, BANDS, crops)
    else:
        B = len(crops)
        tile = {"S2": torch.empty(B, 4, *hw, device="cuda"), "S1": torch.empty(B, 2, *hw, device="cuda"),
                "admin_mask": torch.empty(B, *hw, device="cuda"), "data_hw": torch.empty(B, 2, dtype=torch.int32, device="cuda")}
        ops.region_gather(d2, d1, db, BANDS, crops, out=tile)
    return tile, ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params)


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("name", sorted(RASTERS))
def test_region_batch_equals_gather_then_augment(name, kind):
    from popcorn_amd import ops
    s2, s1, boundary = _sources(name, kind)
    checked = 0
    for case, crops in CASES[name]["crops"].items():
        for hw in CASES[name]["tiles"]:
            with Footprint("cuda", fill=POISON) as fp:
                d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
                for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES):
                    params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
                    tile, (raw, adm) = _composite(d2, d1, db, crops, params, hw)
                    n0 = fp.guarded
                    got = ops.region_batch(d2, d1, db, BANDS, crops, params, hw=hw)
                    assert fp.guarded == n0 + 2                                   # the two outputs and nothing else
                    Hm, Wm = tile["admin_mask"].shape[1:]
                    assert tuple(got["raw"].shape) == (len(crops), 6) + ((Wm, Hm) if rot & 1 else (Hm, Wm))
                    what = (case, hw, params)
                    assert bit_equal(got["raw"], raw), what
                    assert bit_equal(got["admin_mask"], adm), what
                    checked += 1
                    if beta is None and gamma is None and kind == "f32" and case == "whole_and_one_pixel":
                        keep = got["raw"].view(torch.int32)
                        for payload in (0x7FC12345, -0x3FFFFF, 0x7FC00777, 0x7FC00001):      # NaN payloads arrive bit for bit
                            assert bool((keep == payload).any()), (payload, what)
    assert checked == 64 * len(CASES[name]["crops"]) * len(CASES[name]["tiles"])


def test_region_batch_identity_params_and_out():
    """params=None is the plain gather as a raw tile; ``out=`` is written in place and returned."""
    from popcorn_amd import ops
    s2, s1, boundary = _sources("37x53", "f32")
    crops = CASES["37x53"]["crops"]["three_odd_origins"]
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
        tile = ops.region_gather(d2, d1, db, BANDS, crops)
        out = {"raw": fp.alloc((3, 6, 23, 27)), "admin_mask": fp.alloc((3, 23, 27))}
        got = ops.region_batch(d2, d1, db, BANDS, torch.tensor(crops), out=out)
    assert got is out
    assert bit_equal(out["raw"][:, :4].contiguous(), tile["S2"]) and bit_equal(out["raw"][:, 4:].contiguous(), tile["S1"])
    assert bit_equal(out["admin_mask"], tile["admin_mask"])
    assert bool(torch.isnan(out["raw"]).any())


def _random_crops(n, h, w, side, seed):
    g = torch.Generator().manual_seed(seed)
    crops = []
    for _ in range(n):
        x0, y0 = int(torch.randint(0, h - side, (1,), generator=g)), int(torch.randint(0, w - side, (1,), generator=g))
        crops.append((x0, x0 + 1 + int(torch.randint(0, side, (1,), generator=g)), y0, y0 + 1 + int(torch.randint(0, side, (1,), generator=g)),
                      int(torch.randint(0, S, (1,), generator=g))))
    return crops


@pytest.mark.parametrize("rot", [0, 3])
def test_region_batch_more_crops_than_one_launch_carries(rot):
    """B = 130 > PC_REGION_GATHER_MAX_B: two launches; the crops and the label rows of the second land behind the first's."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    assert L.PC_REGION_GATHER_MAX_B == 128
    crops = _random_crops(130, 37, 53, 8, seed=4)
    s2, s1, boundary = _sources("37x53", "u16")
    g = torch.Generator().manual_seed(8)
    plan_cidx = torch.randint(0, 1000, (40, 3), generator=g)
    plan_y = torch.rand(40, 3, generator=g) * 500
    items = torch.randint(0, 40, (130,), generator=g)
    params = {"vflip": True, "hflip": False, "rot": rot, "beta": 1.2, "gamma": None}
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
        pc, py = fp.place(plan_cidx), fp.place(plan_y)
        _, (raw, adm) = _composite(d2, d1, db, crops, params, None)
        got = ops.region_batch(d2, d1, db, BANDS, crops, params, labels=(pc, py, items.tolist(), 2))
    assert bit_equal(got["raw"], raw) and bit_equal(got["admin_mask"], adm)
    assert torch.equal(got["census_idx"].cpu(), plan_cidx[items][:, :2]) and bit_equal(got["y"].cpu(), plan_y[items][:, :2].contiguous())


@pytest.mark.parametrize("form", ["one_unit", "ragged_multi_unit"])
def test_region_batch_labels_equal_torch_indexing(form):
    from popcorn_amd import ops
    from popcorn_amd.data.region import plan_multi_unit, plan_one_unit
    s2, s1, boundary = _sources("96x128", "u16")
    table, _ = R.unit_table(boundary, 10)
    ids, pop = torch.arange(1, 10), torch.rand(9, generator=torch.Generator().manual_seed(3)) * 2000
    if form == "one_unit":
        plan = plan_one_unit(table, ids, pop, (96, 128), admin_overlap=4)
    else:
        plan = plan_multi_unit(table, ids, pop, (96, 128), units_per_crop=4, admin_overlap=4, max_pix_box=6000)
        assert len(set(plan.census_n)) > 1                          # ragged rows
    n, Kp = plan.census_idx.shape
    items = [n - 1, 0, n // 2, 0]                                    # a row twice
    crops = [plan.crops[i].tolist() + [k % S] for k, i in enumerate(items)]
    K = max(plan.census_n[i] for i in items)
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
        pc, py = fp.place(plan.census_idx), fp.place(plan.y)
        n0 = fp.guarded
        got = ops.region_batch(d2, d1, db, BANDS, crops, labels=(pc, py, items, K))
        assert fp.guarded == n0 + 4
        first = ops.region_batch(d2, d1, db, BANDS, crops, labels=(pc, py, items, 1))
    assert got["census_idx"].dtype == torch.int64 and got["y"].dtype == torch.float32
    assert torch.equal(got["census_idx"].cpu(), plan.census_idx[items][:, :K])
    assert bit_equal(got["y"].cpu(), plan.y[items][:, :K].contiguous())
    assert torch.equal(first["census_idx"].cpu(), plan.census_idx[items][:, :1]) and tuple(first["y"].shape) == (4, 1)
    if form == "ragged_multi_unit":
        assert K > 1 and bool((got["census_idx"] == -1).any())       # the plan's own padding behind census_n travels as it is


def test_region_batch_refuses_before_any_launch():
    """Every refusal raises ValueError in the wrapper; the library's own check returns PC_EINVAL with nothing enqueued: outputs keep their fill."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    h, w = RASTERS["37x53"]
    s2, s1, boundary = (t.cuda() for t in _sources("37x53", "f32"))
    plan_cidx = torch.arange(12, dtype=torch.int64, device="cuda").reshape(6, 2)
    plan_y = torch.ones(6, 2, device="cuda")
    good = (3, 20, 5, 32, 0)                                        # 17 x 27
    ident = {"vflip": False, "hflip": False, "rot": 0, "beta": None, "gamma": None}

    def outs(shape=(17, 27), K=2):
        return {"raw": torch.full((2, 6) + shape, 7.0, device="cuda"), "admin_mask": torch.full((2,) + shape, 7.0, device="cuda"),
                "census_idx": torch.full((2, K), 7, dtype=torch.int64, device="cuda"), "y": torch.full((2, K), 7.0, device="cuda")}

    def call_lib(crops, rot, items, K, out, Ho=17, Wo=27):
        flat = [int(v) for c in crops for v in c]
        lab = L.PcRegionLabels(plan_cidx.data_ptr(), plan_y.data_ptr(), (C.c_int32 * 2)(*items), out["census_idx"].data_ptr(),
                               out["y"].data_ptr(), 6, 2, K, 0)
        return L.lib().pc_region_batch(L.ptr(s2), 0, L.ptr(s1), L.ptr(boundary), S, C2, C1, h, w, (C.c_int32 * 6)(*BANDS),
                                       (C.c_int32 * 10)(*flat), 2, 17, 27, 0, 0, rot, 0, C.c_float(1.0), 0, C.c_float(1.0),
                                       L.ptr(out["raw"]), L.ptr(out["admin_mask"]), Ho, Wo, C.byref(lab), L.stream_ptr())

    refusals = [
        ("empty crop", dict(crops=[good, (3, 3, 5, 32, 0)])),
        ("crop leaves the raster", dict(crops=[good, (3, 20, 30, 54, 0)])),
        ("season >= S", dict(crops=[good, (3, 20, 5, 32, 2)])),
        ("rot = 4", dict(rot=4)),
        ("item >= n", dict(items=[0, 6])),
        ("K > Kp", dict(K=3)),
    ]
    for what, kw in refusals:
        crops, rot, items, K = kw.get("crops", [good, good]), kw.get("rot", 0), kw.get("items", [0, 5]), kw.get("K", 2)
        out = outs(K=K)
        with pytest.raises(ValueError):
            ops.region_batch(s2, s1, boundary, BANDS, crops, dict(ident, rot=rot), labels=(plan_cidx, plan_y, items, K), out=out)
        code = call_lib(crops, rot, items, K, out)
        torch.cuda.synchronize()
        assert code == L.PC_EINVAL, what
        assert all(bool((out[k] == 7).all()) for k in out), what
    # a wrong output shape: the tile of an odd rotation handed in unrotated, a tile smaller than a crop, labels of another K
    for out, params, hw in ((outs(), dict(ident, rot=1), None), (outs((16, 27)), ident, None), (outs(K=1), ident, None),
                            (outs(), ident, (16, 27))):
        with pytest.raises(ValueError):
            ops.region_batch(s2, s1, boundary, BANDS, [good, good], params, hw=hw, labels=(plan_cidx, plan_y, [0, 5], 2), out=out)
        assert all(bool((out[k] == 7).all()) for k in out)
    out = outs()
    assert call_lib([good, good], 1, [0, 5], 2, out) == L.PC_EINVAL                    # (Ho, Wo) of rot = 1 is (27, 17)
    torch.cuda.synchronize()
    assert all(bool((out[k] == 7).all()) for k in out)
    with pytest.raises(L.PopcornHipError):
        ops.region_batch(s2.cpu(), s1, boundary, BANDS, [good])
    with pytest.raises(ValueError):
        ops.region_batch(s2, s1, boundary, (5, 0, 2, 1, 2, 0), [good])
    with pytest.raises(ValueError):
        ops.region_batch(s2, s1, boundary, BANDS, [good], labels=(plan_cidx.cpu().int().cuda(), plan_y, [0], 1))
    # and the accepted call next to them does write
    out = outs()
    assert call_lib([good, good], 0, [0, 5], 2, out) == 0
    torch.cuda.synchronize()
    assert not bool((out["raw"] == 7).all()) and out["census_idx"].tolist() == [[0, 1], [10, 11]]


# ---- the feed ---------------------------------------------------------------------------------------------------------------------------
def _region_and_plan(multi):
    from popcorn_amd.data.region import ResidentRegion, plan_multi_unit, plan_one_unit
    s2, s1, boundary = _sources("96x128", "f32")
    ids, pop = torch.arange(1, 10), torch.rand(9, generator=torch.Generator().manual_seed(3)) * 2000
    region = ResidentRegion(s2, s1, boundary, ids, pop, band_sel=BANDS, device="cuda")
    if multi:
        plan = plan_multi_unit(region.table, ids, pop, region.shape, units_per_crop=4, admin_overlap=4, max_pix_box=6000)
        assert len(set(plan.census_n)) > 1
    else:
        plan = plan_one_unit(region.table, ids, pop, region.shape, admin_overlap=4)
    return region, plan


def _epoch(feed, prepare):
    """the batches of one epoch from fixed global generator states, with one global draw per batch where the step would draw"""
    torch.manual_seed(11)
    random.seed(11)
    out = []
    for sample in feed:
        s = prepare(sample)
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()})
        torch.rand(1)
    return out, torch.get_rng_state(), random.getstate()


@pytest.mark.parametrize("multi", [False, True])
def test_batch_feed_equals_region_feed_then_prepare(multi):
    from popcorn_amd.cli import prepare_sample_fused
    from popcorn_amd.data.region import ResidentBatchFeed, ResidentRegionFeed
    from popcorn_amd.utils.transform import Compose, RandomVerticalFlip, default_train_transform
    region, plan = _region_and_plan(multi)
    transform = default_train_transform()
    B = 2

    def unfused(sample):
        s = prepare_sample_fused(sample, transform)
        if sample.get("census_n") is not None:
            s["census_n"] = sample["census_n"]
        return s

    old = ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2)
    new = ResidentBatchFeed(region, plan, B, transform=transform, generator=torch.Generator().manual_seed(5), seasons=2)
    assert type(new.pause()).__name__ == "nullcontext" and len(new) == len(old) == len(plan) // B
    want, rng_w, py_w = _epoch(old, unfused)
    got, rng_g, py_g = _epoch(new, lambda s: s)
    assert torch.equal(new.last_order, old.last_order) and torch.equal(new.last_season, old.last_season)
    assert torch.equal(rng_w, rng_g) and py_w == py_g                # the same global draws, in the same order
    assert len(got) == len(want) == len(old) and len(got) >= 2
    shapes = set()
    for g, w in zip(got, want):
        for key in ("raw", "admin_mask", "y", "census_idx"):
            assert g[key].is_cuda and bit_equal(g[key], w[key]), key
        assert g.get("census_n") == w.get("census_n") and (g.get("census_n") is not None) == multi
        assert {"img_coords", "valid_coords", "season"} <= set(g) and tuple(g["season"].shape) == (B,)
        shapes.add(tuple(g["raw"].shape[2:]))
    assert len(shapes) > 1                                           # the coins and sizes did vary over the epoch
    second, _, _ = _epoch(new, lambda s: s)                         # the next epoch: another permutation from the same generator
    assert not torch.equal(new.last_order, old.last_order) and len(second) == len(got)
    # a transform draw_fused_params cannot express: refused at construction, the global generators untouched
    state = torch.get_rng_state()
    with pytest.raises(ValueError):
        ResidentBatchFeed(region, plan, B, transform={"general": Compose([RandomVerticalFlip(p=0.5, allsame=True)])})
    assert torch.equal(torch.get_rng_state(), state)


def test_batch_feed_under_a_pixel_budget():
    """Every item once per epoch, each batch one launch under the budget; the labels follow the composed batches."""
    from popcorn_amd.data.region import ResidentBatchFeed
    region, plan = _region_and_plan(False)
    budget = 3 * max(int(c[1] - c[0]) * int(c[3] - c[2]) for c in plan.crops.tolist())
    feed = ResidentBatchFeed(region, plan, 2, generator=torch.Generator().manual_seed(5), seasons=2, pixel_budget=budget, max_batch=8)
    with pytest.raises(TypeError):
        len(feed)
    batches = list(feed)
    assert len(feed) == len(batches) == len(feed.last_batches)
    assert sorted(i for b in feed.last_batches for i in b) == list(range(len(plan)))
    assert max(len(b) for b in feed.last_batches) > 2
    for items, s in zip(feed.last_batches, batches):
        Bn, _, Ho, Wo = s["raw"].shape
        assert Bn == len(items) and (Bn == 1 or Bn * Ho * Wo <= budget) and tuple(s["season"].shape) == (Bn,)
        assert torch.equal(s["census_idx"].cpu(), plan.census_idx[items, 0]) and torch.equal(s["y"].cpu(), plan.y[items, 0])
        assert s["valid_coords"] == [tuple(plan.bbox[i].tolist()) for i in items]
        assert torch.equal(s["season"].cpu(), feed.last_season[[feed.last_order.tolist().index(i) for i in items]])


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
BASE = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --resident_region 192 256 --resident_units 24 "
        "--max_steps 3 --save-model no")


@pytest.mark.parametrize("units", [0, 4])
def test_run_train_resident_assemble_equals_the_unfused_feed(tmp_path, units):
    """Three steps with and without --resident_assemble: equal bits in the loss and in every parameter."""
    from popcorn_amd.cli import run_train
    from popcorn_amd.data.region import ResidentBatchFeed, ResidentRegionFeed
    res = []
    for flag, cls in (([], ResidentRegionFeed), (["--resident_assemble"], ResidentBatchFeed)):
        argv = BASE.split() + ["--save_dir", str(tmp_path / (flag[0][2:] if flag else "plain"))] + flag
        if units:
            argv += ["--units_per_crop", str(units)]
        t = run_train(argv)
        assert t.info["iter"] == 3 and type(t._resident_feed) is cls and t.region_plan.multi == bool(units)
        torch.cuda.synchronize()
        res.append((t.fused.loss_out.clone(), t.fused.flat_p.clone(), t._resident_feed.last_order.clone()))
    assert torch.equal(res[0][2], res[1][2])
    assert bool(torch.isfinite(res[0][0]).all()) and bool(torch.isfinite(res[0][1]).all())
    assert bit_equal(res[0][0], res[1][0]) and bit_equal(res[0][1], res[1][1])


def test_run_train_resident_pixel_budget(tmp_path):
    from popcorn_amd.cli import run_train
    from popcorn_amd.data.region import ResidentBatchFeed
    t = run_train(BASE.split() + ["--save_dir", str(tmp_path), "--resident_pixel_budget", "60000"])
    assert t.info["iter"] == 3 and isinstance(t._resident_feed, ResidentBatchFeed) and t._resident_feed.pixel_budget == 60000
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
    taken = t._resident_feed.last_batches[:3]
    assert max(len(b) for b in taken) > 2, taken                     # at least one step on more than two crops
    hw = t._resident_feed._hw
    for b in taken:
        assert len(b) == 1 or len(b) * max(hw[i][0] for i in b) * max(hw[i][1] for i in b) <= 60000


def test_run_train_resident_assemble_refusals(tmp_path):
    from popcorn_amd import cli
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path}".split()
    region = "--resident_region 192 256 --resident_units 24".split()
    for flag in (["--resident_assemble"], ["--resident_pixel_budget", "60000"]):
        with pytest.raises(SystemExit) as e:
            cli.run_train(base + flag)
        assert "--resident_region" in str(e.value)
        with pytest.raises(SystemExit) as e:
            cli.run_train(base + region + flag + ["--nan_fill"])
        assert "--nan_fill" in str(e.value)
    for extra, word in ((["--torch_optimizer"], "--torch_optimizer"), (["--fixed_hw", "64", "64"], "--fixed_hw")):
        with pytest.raises(SystemExit) as e:
            cli.run_train(base + region + ["--resident_assemble"] + extra)
        assert word in str(e.value)
