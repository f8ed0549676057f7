"""Region-resident training data on the GPU (csrc/region.hip and everything above it): the unit table and the gather bit for bit against
the reference's rule restated in tests/region_oracle.py, a feed batch against the host path on the same items, a fused step on either,
and the trainer flag.

Launch geometry of the table pass (csrc/region.hip): a workgroup takes tiles of 32 rows x 1,024 columns when w % 4 == 0 and the raster
is 16-byte aligned (four columns per lane), 32 rows x 256 columns otherwise; tiles are dealt round-robin over min(tiles, 1,024)
workgroups, so a raster of 70 x 1,100 is 3 x 2 tiles = 6 workgroups, 70 x 1,101 is 3 x 5 = 15, and a unit over rows 10 .. 60 and columns
200 .. 1,090 spans workgroups in both directions.  A workgroup has 1,024 LDS bins: 5,000 ids overflow them."""
import ctypes as C

import pytest
import torch

from tests import region_oracle as R
from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu


# ---- the unit table ---------------------------------------------------------------------------------------------------------------------
def _small_raster():
    """37 x 53 (odd width: rows are not 16-byte aligned): background 0, unit 1 = one pixel, id 2 absent, units 3 .. 6 touch the four edges,
    unit 7 in two separate pieces."""
    b = torch.zeros(37, 53, dtype=torch.int32)
    b[20, 31] = 1
    b[0:5, 3:30] = 3            # top edge
    b[30:37, 10:20] = 4         # bottom edge
    b[8:25, 0:4] = 5            # left edge
    b[6:33, 50:53] = 6          # right edge
    b[10:12, 10:12] = 7
    b[26:29, 40:47] = 7
    return b, 8


def _wide_raster(w):
    b = torch.zeros(70, w, dtype=torch.int32)
    b[10:61, 200:1091] = 1                                         # spans the tiles in both directions
    b[0:40, 0:150] = 2
    b[33:70, 1095:w] = 3
    b[31:33, 255:258] = 4                                          # across a tile corner of either geometry
    return b, 6


def _many_ids_raster():
    g = torch.Generator().manual_seed(9)
    cells = torch.randint(0, 5000, (32, 64), generator=g, dtype=torch.int32)
    return cells.repeat_interleave(2, 0).repeat_interleave(2, 1).contiguous(), 5000


def _stray_raster():
    b, n = _small_raster()
    b = b.clone()
    b[1, 1] = -4
    b[15:17, 20:23] = 11                                           # >= num_ids
    b[36, 52] = 8                                                  # == num_ids
    return b, n


TABLE_CASES = {"37x53": _small_raster, "70x1100": lambda: _wide_raster(1100), "70x1101": lambda: _wide_raster(1101),
               "64x128_5000ids": _many_ids_raster, "stray": _stray_raster}
_TABLE_REF = {}


def _table_ref(name):
    """the oracle's table, computed once per case"""
    if name not in _TABLE_REF:
        b, n = TABLE_CASES[name]()
        _TABLE_REF[name] = (b, n) + R.unit_table(b, n)
    return _TABLE_REF[name]


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_region_units_equals_the_per_unit_loop(name):
    from popcorn_amd import ops
    b, n, want, want_stray = _table_ref(name)
    with Footprint("cuda", fill=POISON) as fp:
        bd = fp.place(b)
        table, stray = ops.region_units(bd, n)
        again, stray2 = ops.region_units(bd, n)
        shapes = [ops.region_units(bd, n, max_blocks=k) for k in (1, 3)]
    assert table.dtype == torch.int32 and tuple(table.shape) == (n, 5)
    assert torch.equal(table.cpu(), want), (table.cpu() - want).abs().sum()
    assert int(stray) == want_stray == {"stray": 8}.get(name, 0)
    assert bit_equal(table, again) and int(stray2) == want_stray                     # two runs
    for t, s in shapes:                                                              # two more launch shapes
        assert bit_equal(table, t) and int(s) == want_stray
    if name == "37x53":
        assert want[1].tolist() == [20, 21, 31, 32, 1] and want[2].tolist() == [0] * 5 and want[7].tolist() == [10, 29, 10, 47, 25]


def test_region_units_unaligned_base_and_arguments():
    """A raster with w % 4 == 0 whose base is only 4-byte aligned takes the scalar loads; bad arguments raise before a launch."""
    from popcorn_amd import ops
    from popcorn_amd._lib import PopcornHipError
    b, n, want, _ = _table_ref("70x1100")
    buf = torch.empty(b.numel() + 1, dtype=torch.int32, device="cuda")
    view = buf[1:].view(70, 1100)
    view.copy_(b)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    table, stray = ops.region_units(view, n)
    assert torch.equal(table.cpu(), want) and int(stray) == 0
    with pytest.raises(PopcornHipError):
        ops.region_units(b, n)                                     # a host tensor
    for bad in (view.long(), view[:, :50], view[None]):
        with pytest.raises(ValueError):
            ops.region_units(bad, n)
    with pytest.raises(ValueError):
        ops.region_units(view, 0)


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
H, W, S, C2, C1 = 50, 67, 2, 5, 3
BANDS = (4, 0, 2, 1, 2, 0)                                          # not the identity
_SRC = {}


def _sources(kind):
    """S2 (S, C2, H, W) as uint16 or fp32, S1 fp32, boundary; the fp32 sources hold NaNs with payloads (never the poison's all-ones)."""
    if kind not in _SRC:
        g = torch.Generator().manual_seed(21)
        s2 = torch.randint(0, 10000, (S, C2, H, W), generator=g)
        s2 = s2.to(torch.uint16) if kind == "u16" else s2.float()
        s1 = torch.randn(S, C1, H, W, generator=g) * 5 - 12
        bits = s1.view(torch.int32)
        bits[0, 2, 3:9, 4:40] = 0x7FC12345                          # quiet NaN, payload
        bits[1, 0, 30:50, 60:67] = -0x3FFFFF                        # 0xFFC00001: negative quiet NaN, payload
        if kind == "f32":
            s2.view(torch.int32)[1, 4, 10:20, 0:33] = 0x7FC00777
            s2.view(torch.int32)[0, 0, 49, 66] = 0x7FC00001
        boundary = R.irregular_raster(H, W, units=9, seed=2)
        _SRC[kind] = (s2, s1, boundary)
    return _SRC[kind]


GATHER_CASES = {
    # different sizes, odd y0, Wm = 31: the element-by-element form
    "three_sizes_scalar": [(3, 20, 5, 32, 0), (10, 45, 1, 20, 1), (0, 9, 33, 64, 0)],
    # Wm = 28: vector stores from odd columns, a crop whose right edge cuts a group of four (22 wide), one that ends on one (16 wide)
    "three_sizes_vector": [(3, 20, 5, 33, 1), (7, 30, 11, 27, 0), (1, 12, 3, 25, 1)],
    "corners": [(0, 10, 0, 12, 0), (0, 10, 55, 67, 1), (40, 50, 0, 12, 1), (40, 50, 55, 67, 0)],
    "whole_raster": [(0, 50, 0, 67, 1)],
    "whole_and_one_pixel": [(0, 50, 0, 67, 0), (49, 50, 66, 67, 1)],
}


def _oracle_batch(kind, crops):
    s2, s1, boundary = _sources(kind)
    items = [R.weaksup_item(s2, s1, boundary, BANDS, c[:4], c[4], 1.0, [1], c[:4]) for c in crops]
    return R.host_batch(items, False)


def _assert_batch(out, want):
    for key in ("S2", "S1", "admin_mask", "data_hw"):
        got = out[key].cpu()
        assert got.shape == want[key].shape and got.dtype == want[key].dtype, key
        assert bit_equal(got, want[key]), (key, int((got.contiguous().view(torch.int32) != want[key].contiguous().view(torch.int32)).sum()))


@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("case", sorted(GATHER_CASES))
def test_region_gather_equals_slices_and_collate(case, kind):
    """fp32 compared as int32: NaN payloads count.  The outputs come from intercepted ``torch.empty`` calls: poisoned payloads between
    guard bands, so every element is proven written and nothing outside is touched."""
    from popcorn_amd import ops
    crops = GATHER_CASES[case]
    want = _oracle_batch(kind, crops)
    s2, s1, boundary = _sources(kind)
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
        n0 = fp.guarded
        out = ops.region_gather(d2, d1, db, BANDS, crops)
        assert fp.guarded == n0 + 4
        again = ops.region_gather(d2, d1, db, BANDS, torch.tensor(crops))
    assert all(out[k].is_cuda for k in ("S2", "S1", "admin_mask", "data_hw"))
    _assert_batch(out, want)
    _assert_batch(again, want)
    if kind == "f32":
        assert bool(torch.isnan(want["S1"]).any())                  # the case does carry NaNs


def test_region_gather_into_a_larger_poisoned_out():
    """``out=`` of (Hm + 3, Wm + 1): the padding extends to it; the poison is gone everywhere, the bands are intact."""
    from popcorn_amd import ops
    crops = GATHER_CASES["three_sizes_vector"]
    s2, s1, boundary = _sources("f32")
    want = _oracle_batch("f32", crops)
    Hm, Wm = want["admin_mask"].shape[1:]
    for dh, dw in ((3, 1), (1, 4)):                                 # Wm + 1: element by element; Wm + 4: vector stores
        with Footprint("cuda", fill=POISON) as fp:
            out = {"S2": fp.alloc((3, 4, Hm + dh, Wm + dw)), "S1": fp.alloc((3, 2, Hm + dh, Wm + dw)),
                   "admin_mask": fp.alloc((3, Hm + dh, Wm + dw)), "data_hw": fp.alloc((3, 2), torch.int32)}
            res = ops.region_gather(fp.place(s2), fp.place(s1), fp.place(boundary), BANDS, crops, out=out)
        assert res is out
        for key, pad in (("S2", 0.0), ("S1", 0.0), ("admin_mask", -1.0)):
            got = out[key].cpu()
            assert bit_equal(got[..., :Hm, :Wm].contiguous(), want[key])
            assert bool((got[..., Hm:, :] == pad).all()) and bool((got[..., :, Wm:] == pad).all())
        assert torch.equal(out["data_hw"].cpu(), want["data_hw"])


def test_region_gather_refuses_before_any_launch():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    s2, s1, boundary = (t.cuda() for t in _sources("f32"))
    good = (3, 20, 5, 32, 0)
    for bad in ((3, 20, 5, 68, 0), (-1, 20, 5, 32, 0), (3, 51, 5, 32, 0),          # leaves the raster
                (3, 3, 5, 32, 0), (3, 20, 32, 5, 0),                                # empty
                (3, 20, 5, 32, 2), (3, 20, 5, 32, -1)):                             # season >= S
        out = {"S2": torch.full((2, 4, 17, 27), 7.0, device="cuda"), "S1": torch.full((2, 2, 17, 27), 7.0, device="cuda"),
               "admin_mask": torch.full((2, 17, 27), 7.0, device="cuda"), "data_hw": torch.full((2, 2), 7, dtype=torch.int32, device="cuda")}
        with pytest.raises(ValueError):
            ops.region_gather(s2, s1, boundary, BANDS, [good, bad], out=out)
        # the library's own check, behind the wrapper's: PC_EINVAL, nothing enqueued -- the good crop in front of the bad one is not written
        flat = [int(v) for c in (good, bad) for v in c]
        code = L.lib().pc_region_gather(L.ptr(s2), 0, L.ptr(s1), L.ptr(boundary), S, C2, C1, H, W, (C.c_int32 * 6)(*BANDS),
                                        (C.c_int32 * 10)(*flat), 2, 17, 27, L.ptr(out["S2"]), L.ptr(out["S1"]), L.ptr(out["admin_mask"]),
                                        L.ptr(out["data_hw"]), L.stream_ptr())
        torch.cuda.synchronize()
        assert code == L.PC_EINVAL
        assert all(bool((out[k] == 7).all()) for k in out)
    with pytest.raises(L.PopcornHipError):
        ops.region_gather(s2.cpu(), s1, boundary, BANDS, [good])
    for bands in ((5, 0, 2, 1, 2, 0), (4, 0, 2, 1, 3, 0), (0, 1, 2, 3)):
        with pytest.raises(ValueError):
            ops.region_gather(s2, s1, boundary, bands, [good])
    with pytest.raises(ValueError):
        ops.region_gather(s2, s1, boundary, BANDS, torch.tensor([good]).cuda())


def test_region_gather_more_crops_than_one_launch_carries():
    """B = 130 > PC_REGION_GATHER_MAX_B: two launches, one result."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    assert L.PC_REGION_GATHER_MAX_B == 128
    g = torch.Generator().manual_seed(4)
    crops = []
    for _ in range(130):
        x0, y0 = int(torch.randint(0, H - 8, (1,), generator=g)), int(torch.randint(0, W - 8, (1,), generator=g))
        crops.append((x0, x0 + 1 + int(torch.randint(0, 8, (1,), generator=g)), y0, y0 + 1 + int(torch.randint(0, 8, (1,), generator=g)),
                      int(torch.randint(0, S, (1,), generator=g))))
    s2, s1, boundary = _sources("u16")
    with Footprint("cuda", fill=POISON) as fp:
        out = ops.region_gather(fp.place(s2), fp.place(s1), fp.place(boundary), BANDS, crops)
    _assert_batch(out, _oracle_batch("u16", crops))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _region(nan_clouds, seasons=2):
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import ResidentRegion
    data = SyntheticTestRaster(192, 256, seasons=seasons, n_regions=24, seed=31, device="cuda", raw=True, nan_clouds=nan_clouds)
    return data, ResidentRegion.from_synthetic(data)


def _plan(region, multi):
    from popcorn_amd.data.region import plan_multi_unit, plan_one_unit
    if multi:                                                       # a budget under which the greedy groups come out ragged
        return plan_multi_unit(region.table, region.census_idx, region.census_pop, region.shape, units_per_crop=4, max_pix_box=16000)
    return plan_one_unit(region.table, region.census_idx, region.census_pop, region.shape)


def _host_batches(data, region, plan, feed, B):
    """the host path over the order and seasons the feed drew: slices of the same rasters, the existing collates"""
    s2, s1, boundary = data.s2.cpu(), data.s1.cpu(), data.boundary.cpu()
    order, season = feed.last_order.tolist(), feed.last_season.tolist()
    for k in range(len(feed)):
        items = R.plan_items(s2, s1, boundary, region.band_sel, plan, order[k * B:(k + 1) * B], season[k * B:(k + 1) * B])
        yield R.host_batch(items, plan.multi)


def test_resident_region_refuses_stray_ids_and_a_full_device(monkeypatch):
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import ResidentRegion
    data = SyntheticTestRaster(64, 96, n_regions=6, seed=3, raw=True)               # host tensors: they still have to move
    region = ResidentRegion.from_synthetic(data, device="cuda")
    assert region.s2.is_cuda and region.shape == (64, 96) and tuple(region.table.shape) == (7, 5) and not region.table.is_cuda
    bad = data.boundary.clone()
    bad[5, 7], bad[6, 7] = 9, -2
    with pytest.raises(ValueError, match="2 pixels"):
        ResidentRegion(data.s2, data.s1, bad, data.census_idx, data.census_pop, device="cuda")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (4096, 8192))
    with pytest.raises(MemoryError, match="GiB free"):
        ResidentRegion(data.s2, data.s1, data.boundary, data.census_idx, data.census_pop, device="cuda")
    ResidentRegion(region.s2, region.s1, region.boundary, data.census_idx, data.census_pop, device=region.device)   # nothing left to move


@pytest.mark.parametrize("multi", [False, True])
def test_feed_batches_equal_the_host_path(multi):
    from popcorn_amd.data.region import ResidentRegionFeed
    data, region = _region(nan_clouds=0.03)
    assert torch.equal(region.table, R.unit_table(data.boundary.cpu(), 25)[0])
    plan = _plan(region, multi)
    if multi:
        assert len(set(plan.census_n)) > 1 and len(plan) < 24       # ragged K
    B = 3
    feed = ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2)
    assert len(feed) == len(plan) // B and type(feed.pause()).__name__ == "nullcontext"
    batches = list(feed)
    assert len(batches) == len(feed) and len(set(feed.last_season.tolist())) == 2
    first_order = feed.last_order.clone()
    n, nans = 0, 0
    for got, want in zip(batches, _host_batches(data, region, plan, feed, B)):
        _assert_batch(got, want)
        nans += int(torch.isnan(want["S2"]).sum())
        assert got["y"].is_cuda and got["census_idx"].is_cuda and got["y"].dtype == torch.float32 and got["census_idx"].dtype == torch.int64
        assert torch.equal(got["y"].cpu(), want["y"]) and torch.equal(got["census_idx"].cpu(), want["census_idx"])
        assert got["img_coords"] == want["img_coords"] and got["valid_coords"] == want["valid_coords"]
        assert torch.equal(got["season"].cpu(), want["season"])
        assert got.get("census_n") == want.get("census_n")
        assert set(want) <= set(got)
        n += 1
    assert n == len(feed) and nans > 0                              # the cloud NaNs travel through the gather
    list(feed)                                                     # the next epoch: another permutation from the same generator
    assert not torch.equal(feed.last_order, first_order)


def _new_model():
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    return POPCORN(input_channels=6, feature_extractor="DDA", occupancymodel=True, pretrained=True, biasinit=0.9407,
                   sentinelbuildings=True).cuda()


def _step_sample(batch):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    raw = torch.cat([batch["S2"].cuda(), batch["S1"].cuda()], 1).contiguous()
    s = {"input": ops.select_normalize(raw, (0, 1, 2, 3, 4, 5), stats.MEAN6, stats.STD6), "admin_mask": batch["admin_mask"].cuda().contiguous(),
         "census_idx": batch["census_idx"].cuda().contiguous(), "y": batch["y"].cuda().float().contiguous()}
    if batch.get("census_n") is not None:
        s["census_n"] = batch["census_n"]
    return s


@pytest.mark.parametrize("multi", [False, True])
def test_fused_step_on_a_feed_batch_equals_the_host_batch(multi):
    """One FusedTrainStep.step on the feed's batch and one on the host-collated batch, from equal model and generator state: equal bits in
    the loss and in every parameter."""
    from popcorn_amd.data.region import ResidentRegionFeed
    from popcorn_amd.train import FusedTrainStep
    data, region = _region(nan_clouds=0.0, seasons=1)
    plan = _plan(region, multi)
    feed = ResidentRegionFeed(region, plan, 2, generator=torch.Generator().manual_seed(6))
    got = next(iter(feed))
    want = next(_host_batches(data, region, plan, feed, 2))
    res = []
    for batch in (got, want):
        tr = FusedTrainStep(_new_model(), lr=1e-4, weight_decay=1e-5, gradient_clip=0.01)
        torch.manual_seed(33)
        loss = tr.step(_step_sample(batch))
        torch.cuda.synchronize()
        res.append((loss[0].clone(), tr.flat_p.clone(), tr.last["popcount"].clone()))
    assert bool(torch.isfinite(res[0][0])) and bool(torch.isfinite(res[0][1]).all())
    assert bit_equal(res[0][0], res[1][0]) and bit_equal(res[0][1], res[1][1]) and bit_equal(res[0][2], res[1][2])
    assert res[0][2].numel() == (sum(got["census_n"]) if multi else 2)


@pytest.mark.parametrize("units", [0, 4])
def test_run_train_resident_region(tmp_path, units):
    """run_train.py --resident_region 192 256 --resident_units 24 --max_steps 3 [--units_per_crop 4]: finishes with finite losses."""
    from popcorn_amd.cli import run_train
    from popcorn_amd.data.region import ResidentRegionFeed
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --resident_region 192 256 "
            f"--resident_units 24 --max_steps 3 --save-model no --save_dir {tmp_path}").split()
    if units:
        argv += ["--units_per_crop", str(units)]
    t = run_train(argv)
    assert t.info["iter"] == 3 and isinstance(t._resident_feed, ResidentRegionFeed) and t.region_plan.multi == bool(units)
    assert t._resident_feed.last_order is not None                 # the batches came from the resident feed
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
    if units:
        assert max(t.region_plan.census_n) == 4 and tuple(t.fused.last["popcount"].shape)[0] > 2


def test_run_train_resident_region_refusals(tmp_path, monkeypatch):
    from popcorn_amd import cli
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --resident_region 192 256 --resident_units 24 --save-model no --save_dir {tmp_path}".split()
    for extra, word in ((["--torch_optimizer"], "--torch_optimizer"), (["--fixed_hw", "64", "64"], "--fixed_hw")):
        with pytest.raises(SystemExit) as e:
            cli.run_train(base + extra)
        assert "--resident_region" in str(e.value) and word in str(e.value)
    monkeypatch.setattr(cli, "init_from_env", lambda: (0, 0, 2))
    with pytest.raises(SystemExit) as e:
        cli.run_train(base)
    assert "--resident_region" in str(e.value) and "single process" in str(e.value)
