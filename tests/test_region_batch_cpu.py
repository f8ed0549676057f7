"""The pixel-budget batcher of popcorn_amd/data/region.py (``plan_batches``) against its stated invariants, on the host, and the library's
new export.  Plans: the one-unit plan of the irregular 120 x 150 raster of tests/region_oracle.py with admin_overlap = 4 (24 crops between
11 x 21 = 231 px and 44 x 56 = 2,464 px) and a multi-unit plan of the same raster (units_per_crop = 3, a box budget of 3,000 px)."""
import math

import pytest
import torch

from popcorn_amd.data.region import plan_batches, plan_multi_unit, plan_one_unit
from tests import region_oracle as R

MAX_BATCH, MIN_FILL = 8, 0.6


def _plan(multi):
    boundary = R.irregular_raster()
    ids = torch.arange(1, 25)
    pop = torch.rand(24, generator=torch.Generator().manual_seed(3)) * 2000
    table, stray = R.unit_table(boundary, 25)
    assert stray == 0
    if multi:
        return plan_multi_unit(table, ids, pop, tuple(boundary.shape), units_per_crop=3, admin_overlap=4, max_pix_box=3000)
    return plan_one_unit(table, ids, pop, tuple(boundary.shape), admin_overlap=4)


@pytest.fixture(scope="module", params=[False, True], ids=["one_unit", "multi_unit"])
def hw(request):
    plan = _plan(request.param)
    return [(int(c[1] - c[0]), int(c[3] - c[2])) for c in plan.crops.tolist()]


def _epochs(hw, budget, max_batch=MAX_BATCH, min_fill=MIN_FILL, seed=0, epochs=2):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(epochs):
        order = torch.randperm(len(hw), generator=g)
        out.append(plan_batches(hw, order, budget, max_batch, min_fill, g))
    return out


def _check(hw, batches, budget, max_batch, min_fill):
    assert sorted(i for b in batches for i in b) == list(range(len(hw)))                       # (a) every item exactly once
    for b in batches:
        Hm, Wm = max(hw[i][0] for i in b), max(hw[i][1] for i in b)
        assert 1 <= len(b) <= max_batch                                                         # (c)
        if len(b) > 1:
            assert len(b) * Hm * Wm <= budget                                                   # (b)
            assert sum(hw[i][0] * hw[i][1] for i in b) >= min_fill * len(b) * Hm * Wm           # (d)


def test_library_exports_region_batch_and_keeps_the_abi():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert hasattr(lib, "pc_region_batch")
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10            # additive: no version bump
    assert L.PcRegionLabels.n.offset == 40 and L.PcRegionLabels.K.offset == 48      # five pointers, then n, Kp, K, pad


def test_plan_is_what_the_tests_need():
    plan = _plan(False)
    area = sorted((int(c[1] - c[0]) * int(c[3] - c[2]), int(c[1] - c[0]), int(c[3] - c[2])) for c in plan.crops.tolist())
    assert len(plan) == 24 and area[0] == (231, 11, 21) and area[-1] == (2464, 44, 56)
    classes = [math.floor(8 * math.log2(a)) for a, _, _ in area]
    assert len(set(classes)) < len(classes)                           # some size class holds two items: (f) applies
    multi = _plan(True)
    assert multi.multi and len(set(multi.census_n)) > 1 and len(multi) < 24


@pytest.mark.parametrize("budget", [4000, 8000])
def test_plan_batches_invariants(hw, budget):
    first, second = _epochs(hw, budget)
    for batches in (first, second):
        _check(hw, batches, budget, MAX_BATCH, MIN_FILL)
    # (e) a function of the generator state alone
    assert _epochs(hw, budget) == [first, second]
    assert _epochs(hw, budget, seed=1)[0] != first
    # (f) the next epoch composes other batches -- wherever two crops can share a batch at all.  No two of the multi-unit crops fit
    # 4,000 px padded to their common size with a fill of 0.6, so (b) and (d) leave any rule only batches of one there, in every epoch
    def pairs(a, b):
        padded = 2 * max(a[0], b[0]) * max(a[1], b[1])
        return padded <= budget and a[0] * a[1] + b[0] * b[1] >= MIN_FILL * padded
    if not any(pairs(a, b) for k, a in enumerate(hw) for b in hw[k + 1:]):
        assert all(len(b) == 1 for b in first + second)
    else:
        assert {frozenset(b) for b in first} != {frozenset(b) for b in second}
        assert max(len(b) for b in first) > 1 and len(first) < len(hw)


def test_plan_batches_packs_the_one_unit_plan():
    plan = _plan(False)
    hw = [(int(c[1] - c[0]), int(c[3] - c[2])) for c in plan.crops.tolist()]
    for seed in range(4):
        for batches in _epochs(hw, 8000, seed=seed):
            assert len(batches) < 12 and max(len(b) for b in batches) >= 3
    # the epoch's real pixels over its padded ones: every batch keeps min_fill (a batch of one is full), so the epoch does
    batches = _epochs(hw, 8000)[0]
    padded = sum(len(b) * max(hw[i][0] for i in b) * max(hw[i][1] for i in b) for b in batches)
    assert sum(h * w for h, w in hw) / padded >= MIN_FILL


def test_plan_batches_degenerates_to_batches_of_one(hw):
    smallest = min(h * w for h, w in hw)
    for budget, max_batch in ((smallest - 1, MAX_BATCH), (8000, 1)):
        batches = _epochs(hw, budget, max_batch=max_batch)[0]
        assert len(batches) == len(hw) and all(len(b) == 1 for b in batches)
        _check(hw, batches, budget, max_batch, MIN_FILL)


def test_plan_batches_max_batch_and_fill_bite(hw):
    # a budget that never binds: max_batch does; min_fill = 1 only joins crops of one size
    batches = _epochs(hw, 10 ** 9, max_batch=3, min_fill=0.0)[0]
    _check(hw, batches, 10 ** 9, 3, 0.0)
    assert max(len(b) for b in batches) == 3 and len(batches) == -(-len(hw) // 3)
    batches = _epochs(hw, 10 ** 9, min_fill=1.0)[0]
    _check(hw, batches, 10 ** 9, MAX_BATCH, 1.0)
    assert all(len({hw[i] for i in b}) == 1 for b in batches)


def test_plan_batches_rejects_bad_arguments(hw):
    g = torch.Generator().manual_seed(0)
    order = torch.randperm(len(hw), generator=g)
    for kw in (dict(pixel_budget=0), dict(max_batch=0), dict(min_fill=1.5)):
        args = dict(pixel_budget=8000, max_batch=8, min_fill=0.6)
        args.update(kw)
        with pytest.raises(ValueError):
            plan_batches(hw, order, generator=g, **args)
    with pytest.raises(ValueError):
        plan_batches(hw, order[:-1], 8000, 8, 0.6, g)               # not a permutation of the items


def test_train_parser_assemble_flags():
    from popcorn_amd.cli import train_parser
    a = train_parser().parse_args([])
    assert a.resident_assemble is False and a.resident_pixel_budget == 0 and a.resident_max_batch == 128 and a.resident_min_fill == 0.6
    a = train_parser().parse_args("--resident_region 192 256 --resident_pixel_budget 60000 --resident_max_batch 16".split())
    assert a.resident_pixel_budget == 60000 and a.resident_max_batch == 16 and not a.resident_assemble
