"""The host side of the resident validation (popcorn_amd/data/region.py: split_census, ResidentItems; cli.py: --resident_val,
--resident_seasons): the reference's 80 / 20 split against a fixture pandas wrote (tests/golden/g14_split.npz,
tests/golden/make_golden_split.py), its placement in front of the planner's size filters, the command-line refusals that need no device,
and the library's new export."""
import os
import re

import numpy as np
import pytest
import torch

from popcorn_amd.data.region import plan_one_unit, split_census

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_split.npz")
SIZES = (1, 2, 5, 37, 400)


def _table(n):
    """The fixture's census table: idx = 7 * row + 3, POP20 = 1.5 * row."""
    return 7 * torch.arange(n, dtype=torch.int64) + 3, torch.arange(n, dtype=torch.float32) * 1.5


@pytest.mark.parametrize("n", SIZES)
def test_split_equals_the_pandas_fixture(n):
    g = np.load(GOLDEN)
    ids, pop = _table(n)
    order = g[f"n{n}/order"]
    assert sorted(order.tolist()) == list(range(n))
    cut = int(n * 0.8)
    for split, rows in (("train", order[:cut]), ("val", order[cut:])):
        got_ids, got_pop = split_census(ids, pop, split)
        want = g[f"n{n}/{split}"]
        assert got_ids.dtype == torch.int64 and got_pop.dtype == torch.float32
        assert got_ids.tolist() == want.tolist() == (7 * rows + 3).tolist(), (n, split)       # the permuted order is kept
        assert got_pop.tolist() == (rows * 1.5).tolist()                                     # every row keeps its count


@pytest.mark.parametrize("n", SIZES)
def test_train_and_val_are_disjoint_and_cover_all_rows(n):
    ids, pop = _table(n)
    tr, _ = split_census(ids, pop, "train")
    va, _ = split_census(ids, pop, "val")
    assert tr.numel() == int(n * 0.8) and tr.numel() + va.numel() == n
    assert not set(tr.tolist()) & set(va.tolist())
    assert sorted(tr.tolist() + va.tolist()) == ids.tolist()


def test_all_is_the_identity_and_one_row_trains_on_nothing():
    ids, pop = _table(37)
    a_ids, a_pop = split_census(ids, pop, "all")
    assert torch.equal(a_ids, ids) and torch.equal(a_pop, pop)
    one = split_census(*_table(1), "train")
    assert one[0].numel() == 0 and one[1].numel() == 0                   # int(1 * 0.8) == 0: the caller refuses it
    assert split_census(*_table(1), "val")[0].tolist() == [3]
    with pytest.raises(ValueError, match="split"):
        split_census(ids, pop, "test")
    with pytest.raises(ValueError, match="length"):
        split_census(ids, pop[:-1], "train")


def test_split_feeds_the_planner_in_permuted_order_filters_afterwards():
    """The split comes first and the planner's filters second (PopulationDataset.py:105-131): the items are the split's rows in the
    permuted order, without the rows either size filter (or the empty-unit rule) takes out."""
    n, h, w = 37, 200, 300
    ids = torch.arange(1, n + 1, dtype=torch.int64)
    pop = torch.arange(n, dtype=torch.float32) + 0.5
    table = torch.zeros(n + 1, 5, dtype=torch.int64)                     # {xmin, xmax, ymin, ymax, count} per id
    for i in range(1, n + 1):
        x, y = 5 * (i % 20), 7 * (i % 30)
        table[i] = torch.tensor([x, x + 4, y, y + 6, 20])
    table[5, 4] = 1000                                                   # count >= max_pix
    table[9] = torch.tensor([0, 150, 0, 200, 30])                        # bounding box >= max_pix_box
    table[11] = torch.tensor([0, 0, 0, 0, 0])                            # no pixel
    g = np.load(GOLDEN)
    order = g["n37/order"]
    seen = []
    for split, rows in (("train", order[:29]), ("val", order[29:])):
        s_ids, s_pop = split_census(ids, pop, split)
        plan = plan_one_unit(table, s_ids, s_pop, (h, w), max_pix=500, max_pix_box=10_000)
        want = [int(r) + 1 for r in rows if int(r) + 1 not in (5, 9, 11)]
        assert plan.census_idx[:, 0].tolist() == want, split
        assert plan.y[:, 0].tolist() == [i - 0.5 for i in want]
        seen += want
    assert sorted(seen) == [i for i in range(1, n + 1) if i not in (5, 9, 11)]       # every eligible unit, in exactly one plan
    assert {5, 9, 11} & set((order[:29] + 1).tolist()) and len(seen) == n - 3


def test_command_line_refusals(tmp_path):
    from popcorn_amd import cli
    t = cli.train_parser().parse_args([])
    assert t.resident_val is False and t.resident_seasons == 1
    cli.check_repair_args(t)
    t = cli.train_parser().parse_args("--resident_region 96 128 --resident_val -wv --resident_seasons 2".split())
    assert t.resident_val and t.weak_validation and t.resident_seasons == 2 and t.weak_val_batch_size == 1
    cli.check_repair_args(t)
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path}".split()
    before = set(os.listdir(tmp_path))
    for extra, words in ((["--resident_val"], ("--resident_val", "--resident_region")),
                         (["--resident_region", "96", "128", "--resident_val", "-wvb", "2"], ("--resident_val", "-wvb")),
                         (["--resident_seasons", "2"], ("--resident_seasons", "--resident_region")),
                         (["--resident_region", "96", "128", "--resident_seasons", "0"], ("--resident_seasons",))):
        with pytest.raises(SystemExit) as e:
            cli.run_train(base + extra)
        assert all(wd in str(e.value) for wd in words), (extra, str(e.value))
    assert set(os.listdir(tmp_path)) == before                           # refused before anything was set up


def test_library_exports_the_item_kernel_at_abi_10():
    import ctypes as C
    from popcorn_amd import _lib as L
    lib = L.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "popcorn_hip.h")).read()
    assert hasattr(lib, "pc_region_item")
    assert re.search(r"\bint pc_region_item\(", hdr), "pc_region_item is not declared in popcorn_hip.h"
    assert lib.pc_region_item.argtypes is not None and len(lib.pc_region_item.argtypes) == 27
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10                # additive: no version bump
    tile = int(re.search(r"#define PC_REGION_ITEM_TILE (\d+)", hdr).group(1))
    assert tile == L.PC_REGION_ITEM_TILE and tile % 4 == 0
    # a NULL pointer is refused before the device is touched
    z = C.c_int64(0)
    assert lib.pc_region_item(None, 0, None, None, 0, None, 1, 4, 2, 8, 8, None, 0, 1, 0, 1, 0, None, None, None, None, z, z, z, None, None,
                              None) == L.PC_EINVAL
