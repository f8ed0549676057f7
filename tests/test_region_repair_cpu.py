"""The host side of the resident repair (popcorn_amd/data/region.py: plan_repair and what it is made of) against the plain-torch
statements of tests/region_repair_oracle.py, the library's new exports, and the command-line refusals that need no device."""
import itertools
import os
import re

import pytest
import torch

from popcorn_amd.data import nanfill
from popcorn_amd.data.region import RegionPlan, item_orbit, plan_multi_unit
from tests import region_oracle as R
from tests import region_repair_oracle as O

NEW_SYMBOLS = ("pc_region_nan_census", "pc_region_gather_orbit", "pc_region_batch_orbit", "pc_region_patch_count", "pc_region_patch_write",
               "pc_region_patch_apply")


def test_library_exports_the_repair_at_abi_10():
    from popcorn_amd import _lib as L
    lib = L.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "popcorn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", hdr), f"{name} is not declared in popcorn_hip.h"
        assert getattr(lib, name).argtypes is not None, f"{name} has no binding in _lib.py"
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10            # additive: no version bump
    assert int(re.search(r"#define PC_REGION_PATCH_CHUNK (\d+)", hdr).group(1)) == L.PC_REGION_PATCH_CHUNK


@pytest.mark.parametrize("ascfill", [False, True])
def test_orbit_rule_equals_the_restated_reference(ascfill):
    """``item_orbit`` (nanfill.s1_orbit / asc_fill) against PopulationDataset.py:423-441 over counts around every threshold, the boundary
    count == 0.05 * numel included: 0.05 is not below 0.05."""
    seen = set()
    for h, w in ((10, 10), (36, 36), (40, 50), (1, 1), (3, 7)):
        numel = 2 * h * w
        edge = numel // 20                                            # 0.05 * numel where numel is a multiple of 20
        grid = sorted({0, 1, edge - 1, edge, edge + 1, numel - 1, numel} & set(range(numel + 1)))
        for nd, na in itertools.product(grid, grid):
            try:
                want = (O.orbit_rule(nd, na, numel, ascfill)[0], True)
            except O.NoData:
                want = (1, False)
            got = item_orbit(nd, na, numel, ascfill, True)
            assert (int(got[0]), got[1]) == want, (nd, na, numel, ascfill)
            seen.add(want)
            # without an ascending raster: descending at any fraction, never dropped
            assert item_orbit(nd, na, numel, False, False) == (0, True)
            assert O.orbit_rule(nd, na, numel, False, has_asc=False)[0] == 0
    assert seen == {(0, True), (1, True), (1, False)}
    # the boundary itself, by name: 200 entries, 10 NaNs -> the quotient is 0.05, not below it
    assert not nanfill.nan_fraction_ok(10, 200) and nanfill.nan_fraction_ok(9, 200)
    assert item_orbit(10, 0, 200, False, True) == (1, True) and item_orbit(9, 0, 200, False, True) == (0, True)
    assert item_orbit(10, 10, 200, False, True) == (1, False) and item_orbit(10, 9, 200, False, True) == (1, True)
    assert item_orbit(1, 0, 200, True, True) == (1, True) and item_orbit(0, 200, 200, True, True) == (0, True)     # ascfill; no NaN: kept


def test_patch_position_for_all_flips_and_turns():
    """The oracle's position map on a non-square tile against torch.flip / torch.rot90 of an index image."""
    Hm, Wm = 5, 7
    index = torch.arange(Hm * Wm).reshape(Hm, Wm)
    for vflip, hflip, rot in itertools.product((False, True), (False, True), range(4)):
        out = O.transform_tile(index, vflip, hflip, rot)
        assert tuple(out.shape) == ((Wm, Hm) if rot & 1 else (Hm, Wm))
        for i, j in itertools.product(range(Hm), range(Wm)):
            a, b = O.patch_position(i, j, Hm, Wm, vflip, hflip, rot)
            assert int(out[a, b]) == i * Wm + j, (vflip, hflip, rot, i, j)


def test_plan_subset_keeps_every_row():
    boundary = R.irregular_raster()
    ids = torch.arange(1, 25)
    pop = torch.rand(24, generator=torch.Generator().manual_seed(3)) * 2000
    table, _ = R.unit_table(boundary, 25)
    plan = plan_multi_unit(table, ids, pop, tuple(boundary.shape), units_per_crop=3, admin_overlap=4, max_pix_box=3000)
    n = len(plan)
    kept = [i for i in range(n) if i not in (0, 3, n - 1)]
    sub = plan.subset(kept)
    assert isinstance(sub, RegionPlan) and len(sub) == n - 3 and sub.multi == plan.multi
    for k, i in enumerate(kept):
        for name in ("crops", "census_idx", "y", "bbox"):
            assert torch.equal(getattr(sub, name)[k], getattr(plan, name)[i]), (name, k, i)
        assert sub.census_n[k] == plan.census_n[i]
    assert plan.subset(range(n)) == plan


def test_train_parser_repair_flags_and_refusals(tmp_path):
    from popcorn_amd import cli
    a = cli.train_parser().parse_args([])
    assert a.resident_repair is False and a.resident_s1_gap == 0.0
    a = cli.train_parser().parse_args("--resident_region 192 256 --resident_repair --ascfill --resident_s1_gap 0.1 --nan_clouds 0.05 "
                                      "--resident_assemble".split())
    assert a.resident_repair and a.ascfill and a.resident_s1_gap == 0.1 and a.nan_clouds == 0.05 and a.resident_assemble
    cli.check_repair_args(a)
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path}".split()
    with pytest.raises(SystemExit) as e:
        cli.run_train(base + ["--resident_repair"])
    assert "--resident_region" in str(e.value) and "--resident_repair" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.run_train(base + "--resident_region 192 256 --resident_s1_gap 0.1".split())
    assert "--resident_repair" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.run_train(base + "--resident_region 192 256 --resident_repair --resident_s1_gap 1.5".split())
    assert "[0, 1]" in str(e.value)
