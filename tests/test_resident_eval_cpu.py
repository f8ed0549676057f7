"""The host side of the resident evaluation (popcorn_amd/data/region.py: ResidentWindows and what it is made of): the library's new
export, the orbit column of a window list as a pure function of its census, the sharding of the window list over ranks, and the
command-line refusals that need no device."""
import itertools
import os
import re

import pytest
import torch

from popcorn_amd import eval as E
from popcorn_amd.data.region import item_orbit, orbit_column, window_orbits
from popcorn_amd.distributed import shard_indices


def test_library_exports_the_window_kernel_at_abi_10():
    from popcorn_amd import _lib as L
    lib = L.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(L.__file__)), "include", "popcorn_hip.h")).read()
    for name in ("pc_region_window", "pc_region_window_rows"):
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\(", hdr), f"{name} is not declared in popcorn_hip.h"
        assert getattr(lib, name).argtypes is not None, f"{name} has no binding in _lib.py"
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10            # additive: no version bump
    cap = int(re.search(r"#define PC_REGION_WINDOW_MAX_PS (\d+)", hdr).group(1))
    assert cap == L.PC_REGION_WINDOW_MAX_PS and 6 * cap * cap < 2 ** 31
    # the rows a workgroup owns: a tile of at most 32 KB, at least one row, no more rows than the window has; 0 for a refused side
    for ps in (1, 2, 3, 32, 33, 36, 255, 256, 1024, 2048, 4096, 4097, cap):
        R = lib.pc_region_window_rows(ps)
        assert 1 <= R <= ps and R * ps * 4 <= 32 * 1024, (ps, R)
    assert lib.pc_region_window_rows(0) == 0 and lib.pc_region_window_rows(cap + 1) == 0
    assert lib.pc_region_window_rows(36) < 36                         # the ps = 36 tests of the GPU file cross a row-block boundary


def test_window_rows_make_ranges_the_crop_kernel_takes():
    """A window is launched as a square item whose range argument is R * ps, R = pc_region_window_rows(ps).  For every side the launch
    accepts: at least one row and no more than 16 or than the window has; a range of at most 4,096 elements unless it is a single row;
    and a range that is a multiple of the vector width whenever the rows are -- the conditions under which the contiguous ranges of
    region_crop.hip are blocks of whole rows and a group of four never leaves its row."""
    from popcorn_amd import _lib as L
    rows = L.lib().pc_region_window_rows
    for ps in range(1, L.PC_REGION_WINDOW_MAX_PS + 1):
        R = rows(ps)
        assert 1 <= R <= min(16, ps), (ps, R)
        assert R * ps <= 4096 or R == 1, (ps, R)
        assert ps % 4 != 0 or (R * ps) % 4 == 0, (ps, R)


@pytest.mark.parametrize("ascfill", [False, True])
@pytest.mark.parametrize("ps", [10, 20, 36])
def test_window_orbits_against_item_orbit_around_five_percent(ps, ascfill):
    """``window_orbits`` maps (counts, window list, ps, ascfill, has_asc) to the orbit column or to the ValueError naming the window;
    the rule is ``item_orbit`` at numel = 2 * ps * ps.  Counts sit around the boundary count = 0.05 * 2 * ps * ps: 0.05 is not below 0.05."""
    numel = 2 * ps * ps
    hi = -(-numel // 20)                                               # the first count at or above 0.05 * numel, in integers
    lo = hi - 1                                                        # the last one below
    assert lo / numel < 0.05 <= hi / numel and hi == lo + 1
    grid = [0, 1, lo, hi, hi + 1, numel]
    windows = [(3 * k, 5 * k + 1, k % 4) for k in range(len(grid) ** 2)]
    pairs = list(itertools.product(grid, grid))
    seen = set()
    for has_asc in (True, False):
        if ascfill and not has_asc:
            continue
        want = [item_orbit(nd, na, numel, ascfill, has_asc) for nd, na in pairs]
        good = [k for k, (_, ok) in enumerate(want) if ok]
        counts = torch.tensor([[7, nd, na] for nd, na in pairs], dtype=torch.int64)
        got = window_orbits(counts[good], [windows[k] for k in good], ps, ascfill, has_asc)
        assert got.dtype == torch.int8 and got.tolist() == [int(want[k][0]) for k in good]
        seen.update(int(want[k][0]) for k in good)
        # the column of orbit_column is the same rule, item by item
        o, ok = orbit_column([[c] for c in counts.tolist()], [numel] * len(pairs), ascfill, has_asc)
        assert [(int(a), bool(b)) for a, b in zip(o[:, 0], ok[:, 0])] == [(int(a), b) for a, b in want]
        bad = [k for k, (_, ok_) in enumerate(want) if not ok_]
        assert bool(bad) == has_asc                                    # without an ascending raster nothing is refused
        if bad:
            # the FIRST window of the list without data is the one named
            with pytest.raises(ValueError) as e:
                window_orbits(counts, windows, ps, ascfill, has_asc)
            x, y, s = windows[bad[0]]
            assert f"({x}, {y}, {s})" in str(e.value) and "No data here!" in str(e.value)
    assert seen == {0, 1}
    # the boundary by name
    assert window_orbits([[0, lo, 0]], [(0, 0, 0)], ps, False, True).tolist() == [0]
    assert window_orbits([[0, hi, 0]], [(0, 0, 0)], ps, False, True).tolist() == [1]
    assert window_orbits([[0, hi, lo]], [(0, 0, 0)], ps, False, True).tolist() == [1]
    with pytest.raises(ValueError, match=r"\(4, 9, 2\)"):
        window_orbits([[0, 0, 0], [0, hi, hi]], [(0, 0, 0), (4, 9, 2)], ps, False, True)
    assert window_orbits([[0, 1, 0]], [(0, 0, 0)], ps, True, True).tolist() == [1]           # ascfill: any NaN switches
    assert window_orbits([[0, 0, numel]], [(0, 0, 0)], ps, True, True).tolist() == [0]       # no NaN: kept, the ascending orbit is not looked at
    assert window_orbits([[0, numel, numel]], [(0, 0, 0)], ps, False, False).tolist() == [0]  # no ascending raster: descending at any fraction
    with pytest.raises(ValueError, match="one census triple per window"):
        window_orbits([[0, 0, 0]], [(0, 0, 0), (1, 1, 0)], ps)


@pytest.mark.parametrize("h,w,ps,overlap,four", [(150, 170, 64, 8, True), (70, 90, 36, 4, False), (64, 64, 64, 8, False), (300, 200, 64, 16, True)])
def test_rank_sharding_covers_every_window_exactly_once(h, w, ps, overlap, four):
    n = E.get_patch_indices(h, w, ps, overlap, four).shape[0]
    assert n >= 1
    for world in (1, 2, 3, 5, n, n + 3):
        shards = [list(shard_indices(n, r, world)) for r in range(world)]
        flat = sorted(k for s in shards for k in s)
        assert flat == list(range(n)), (world, flat)                   # every window once, none twice
        assert all(k % world == r for r, s in enumerate(shards) for k in s)


def test_command_line_refusals(tmp_path):
    from popcorn_amd import cli
    a = cli.eval_parser().parse_args([])
    assert a.resident_windows is False
    a = cli.eval_parser().parse_args("--resident_windows --nan_clouds 0.05 --s1_gap 0.05 --ascfill --fourseasons --product_cell 10 "
                                     "--census_table".split())
    assert a.resident_windows and not a.raw_input and a.ascfill and a.fourseasons and a.product_cell == 10 and a.census_table
    cli.check_eval_args(a)
    with pytest.raises(SystemExit) as e:
        cli.run_eval("-S2 -NIR -S1 -occmodel -senbuilds --resident_windows --raw_input".split())
    assert "--resident_windows" in str(e.value) and "--raw_input" in str(e.value)
    t = cli.train_parser().parse_args([])
    assert t.resident_test is False
    t = cli.train_parser().parse_args("--resident_region 150 170 --resident_test".split())
    assert t.resident_test
    cli.check_repair_args(t)
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path}".split()
    with pytest.raises(SystemExit) as e:
        cli.run_train(base + ["--resident_test"])
    assert "--resident_test" in str(e.value) and "--resident_region" in str(e.value)
