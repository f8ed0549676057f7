"""The building layer a dataset ships, without a GPU: the additive C ABI (every `_layer` entry point refuses a half-given or misaligned
layer before anything is enqueued, the plain entry points stay exported, the ABI version stays 10), the synthetic layer of the host
datasets and the test raster, the collate's zero padding, and the refusal of ``--building_layer -senbuilds`` in both command lines."""
import ctypes as C
import os
import re

import pytest
import torch

# pointer values that are never dereferenced: every call below is refused by the host checks, which run before anything is enqueued
P = [0x100000 + 0x10000 * k for k in range(16)]
BANDS = (0, 1, 2, 3, 0, 1)


def _calls(L):
    """name -> f(layer, layer_out): one otherwise valid call of every `_layer` entry point with the two layer pointers as given."""
    lib = L.lib()
    band = (C.c_int32 * 6)(*BANDS)
    crops = (C.c_int32 * 5)(1, 9, 2, 14, 0)
    mean, std = (C.c_float * 6)(*[0.0] * 6), (C.c_float * 6)(*[1.0] * 6)
    one = C.c_float(1.0)
    return {
        "pc_augment_raw_layer": lambda a, b: lib.pc_augment_raw_layer(P[0], P[1], P[2], a, P[3], P[4], b, 1, 8, 12, 0, 0, 0, 0, one, 0, one,
                                                                      None),
        "pc_region_gather_layer": lambda a, b: lib.pc_region_gather_layer(P[0], 0, P[1], None, None, P[2], a, 1, 4, 2, 16, 16, band, crops, 1,
                                                                          8, 12, P[3], P[4], P[5], b, P[6], None),
        "pc_region_batch_layer": lambda a, b: lib.pc_region_batch_layer(P[0], 0, P[1], None, None, P[2], a, 1, 4, 2, 16, 16, band, crops, 1, 8,
                                                                        12, 0, 0, 0, 0, one, 0, one, P[3], P[4], b, 8, 12, None, None),
        "pc_region_window_layer": lambda a, b: lib.pc_region_window_layer(P[0], 0, P[1], None, 0, a, 1, 4, 2, 16, 16, band, 2, 3, 0, 8, mean,
                                                                          std, None, None, 0, 0, 0, P[3], b, None),
        "pc_region_item_layer": lambda a, b: lib.pc_region_item_layer(P[0], 0, P[1], None, 0, P[2], a, 1, 4, 2, 16, 16, band, 1, 9, 2, 14, 0,
                                                                      mean, std, None, None, 0, 0, 0, P[3], P[4], b, None),
    }


def test_every_layer_entry_point_refuses_before_any_launch():
    from popcorn_amd import _lib as L
    for name, call in _calls(L).items():
        assert call(None, P[8]) == L.PC_EINVAL, f"{name}: a NULL layer with a layer output"
        assert call(P[7], None) == L.PC_EINVAL, f"{name}: a layer without a layer output"
        assert call(P[7] + 1, P[8]) == L.PC_EINVAL, f"{name}: a layer misaligned for fp32"
        assert call(P[7], P[8] + 2) == L.PC_EINVAL, f"{name}: a layer output misaligned for fp32"


def test_abi_is_additive_and_the_header_is_exported():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10            # additive: no version bump
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "popcorn_hip.h")).read()
    old = ("pc_augment_raw", "pc_region_gather", "pc_region_gather_orbit", "pc_region_batch", "pc_region_batch_orbit", "pc_region_window",
           "pc_region_item")
    new = ("pc_augment_raw_layer", "pc_region_gather_layer", "pc_region_batch_layer", "pc_region_window_layer", "pc_region_item_layer")
    for name in old + new:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(rf"\bint {name}\(", hdr), f"{name} is not declared in popcorn_hip.h"
    for name in new:
        assert getattr(lib, name).argtypes is not None, f"{name} has no binding in _lib.py"
    declared = set(re.findall(r"^[A-Za-z_][A-Za-z0-9_ \*]*?\b(pc_[a-z0-9_]+)\(", hdr, flags=re.M))
    assert len(declared) > 60 and set(new) <= declared
    missing = sorted(n for n in declared if not hasattr(lib, n))
    assert not missing, f"declared in popcorn_hip.h but not exported: {missing}"


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_synthetic_weaksup_layer():
    from popcorn_amd.data.dataset import SyntheticWeaksupDataset
    plain = SyntheticWeaksupDataset(6, min_hw=20, max_hw=40, seed=5)
    a = SyntheticWeaksupDataset(6, min_hw=20, max_hw=40, seed=5, buildings=True)
    b = SyntheticWeaksupDataset(6, min_hw=20, max_hw=40, seed=5, buildings=True)
    other = SyntheticWeaksupDataset(6, min_hw=20, max_hw=40, seed=6, buildings=True)
    for i in range(6):
        p, x, y = plain[i], a[i], b[i]
        assert "building_counts" not in p
        layer = x["building_counts"]
        h, w = x["S2"].shape[1:]
        assert layer.dtype == torch.float32 and tuple(layer.shape) == (1, h, w)
        assert _same(layer, y["building_counts"])                                      # deterministic per seed
        assert bool((layer >= 0).all()) and bool((layer == layer.round()).all())       # non-negative whole numbers
        zero = float((layer == 0).float().mean())
        assert 0.5 < zero < 0.9 and float(layer.max()) >= 1                            # the occupancy model's > 0 mask matters
        for key in ("S2", "S1", "admin_mask", "y", "census_idx"):                     # switching it on changes no other tensor
            assert _same(p[key], x[key]), key
        assert p["season"] == x["season"]
    assert other.hw != a.hw or not _same(other[0]["building_counts"], a[0]["building_counts"])


def test_synthetic_test_raster_layer():
    from popcorn_amd.data.dataset import SyntheticTestRaster
    for raw in (False, True):
        kw = dict(h=48, w=64, seasons=2, n_regions=12, seed=3, raw=raw, nan_clouds=0.05 if raw else 0.0, s1_gap=0.05 if raw else 0.0,
                  coarse_regions=4)
        plain, a, b = SyntheticTestRaster(**kw), SyntheticTestRaster(buildings=True, **kw), SyntheticTestRaster(buildings=True, **kw)
        assert plain.buildings is None
        layer = a.buildings
        assert layer.dtype == torch.float32 and tuple(layer.shape) == (48, 64) and _same(layer, b.buildings)
        assert bool((layer >= 0).all()) and bool((layer == layer.round()).all()) and 0.5 < float((layer == 0).float().mean()) < 0.9
        names = ("s2", "s1", "s1_asc") if raw else ("raster",)
        for key in names + ("boundary", "census_pop", "census_idx", "boundary_coarse", "census_pop_coarse"):
            assert _same(getattr(plain, key), getattr(a, key)), key
    assert not _same(SyntheticTestRaster(h=48, w=64, n_regions=12, seed=4, buildings=True).buildings, layer)


def test_collate_pads_the_layer_with_zeros():
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.dataset import SyntheticWeaksupDataset
    ds = SyntheticWeaksupDataset(4, min_hw=20, max_hw=40, seed=9, buildings=True)
    items = [ds[0], ds[1], ds[2]]
    assert len({tuple(it["S2"].shape[1:]) for it in items}) > 1
    batch = Population_Dataset_collate_fn(items)
    bc = batch["building_counts"]
    Hm, Wm = max(it["S2"].shape[1] for it in items), max(it["S2"].shape[2] for it in items)
    assert tuple(bc.shape) == (3, 1, Hm, Wm) and bc.dtype == torch.float32
    for k, it in enumerate(items):
        h, w = it["S2"].shape[1:]
        assert _same(bc[k, :, :h, :w].contiguous(), it["building_counts"])
        assert bool((bc[k, :, h:, :] == 0).all()) and bool((bc[k, :, :, w:] == 0).all())
        assert not bool(torch.signbit(bc[k, :, h:, :]).any()) and not bool(torch.signbit(bc[k, :, :, w:]).any())      # +0.0


def test_multi_unit_items_and_their_collate_carry_the_layer():
    from popcorn_amd.data.units import SyntheticMultiUnitDataset, collate_units
    kw = dict(n_regions=4, units=3, min_hw=20, max_hw=40, seed=7, ragged=True)
    plain, a, b = SyntheticMultiUnitDataset(**kw), SyntheticMultiUnitDataset(buildings=True, **kw), SyntheticMultiUnitDataset(buildings=True, **kw)
    for i in range(4):
        p, x = plain[i], a[i]
        layer = x["building_counts"]
        assert "building_counts" not in p and tuple(layer.shape) == (1,) + tuple(x["S2"].shape[1:]) and _same(layer, b[i]["building_counts"])
        assert bool((layer >= 0).all()) and bool((layer == layer.round()).all()) and 0.5 < float((layer == 0).float().mean()) < 0.9
        for key in ("S2", "S1", "admin_mask", "y", "census_idx"):
            assert _same(p[key], x[key]), key
    batch = collate_units([a[0], a[1], a[2]])
    Hm, Wm = batch["S2"].shape[2:]
    assert tuple(batch["building_counts"].shape) == (3, 1, Hm, Wm) and batch["census_n"] == [a[k]["census_idx"].numel() for k in range(3)]
    for k in range(3):
        h, w = a[k]["S2"].shape[1:]
        assert _same(batch["building_counts"][k, :, :h, :w].contiguous(), a[k]["building_counts"])
        assert bool((batch["building_counts"][k, :, h:, :] == 0).all()) and bool((batch["building_counts"][k, :, :, w:] == 0).all())


def test_building_layer_with_senbuilds_is_refused_by_name(tmp_path):
    from popcorn_amd import cli
    assert cli.train_parser().parse_args([]).building_layer is False and cli.eval_parser().parse_args([]).building_layer is False
    assert cli.train_parser().parse_args(["--building_layer"]).building_layer
    assert cli.eval_parser().parse_args(["--building_layer"]).building_layer
    cli.check_building_layer(cli.train_parser().parse_args(["--building_layer"]))
    cli.check_building_layer(cli.eval_parser().parse_args(["-senbuilds"]))
    with pytest.raises(SystemExit) as e:
        cli.run_train(f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path} --building_layer".split())
    assert "--building_layer" in str(e.value) and "-senbuilds" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.run_eval("-S2 -NIR -S1 -occmodel -senbuilds --building_layer".split())
    assert "--building_layer" in str(e.value) and "-senbuilds" in str(e.value)
