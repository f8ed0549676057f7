"""The NaN-fill oracle (tests/nanfill_oracle.py) against the reference's interpolate_nan (data/PopulationDataset.py:526-551, scipy
griddata "nearest"), recorded in tests/golden/g13_nan_fill.npz by tests/golden/make_golden_nanfill.py: exact wherever the nearest known
entry is unique, and the reference's value one of the tie set's values where it is not (scipy's k-d tree breaks ties its own way)."""
import os

import numpy as np
import pytest

from tests import nanfill_oracle as NO

G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_nan_fill.npz")
CASES = ["clouds", "scattered_one_channel", "row_col", "s1_plane", "tie_free", "few_known", "nan_free"]


def check_against_reference(inp, ref, got):
    """got (the oracle's or the device's fill) vs the reference: bit-equal at unique-nearest sites, in the tie set elsewhere; known
    entries unchanged.  Returns (unique sites, tie sites)."""
    nan = np.isnan(inp)
    assert not np.isnan(got).any() and not np.isnan(ref).any()
    assert np.array_equal(got[~nan].view(np.uint32), inp[~nan].view(np.uint32))
    miss, sets = NO.tie_sets(inp)
    uniq = ties = 0
    for m, s in zip(miss, sets):
        r, g = ref[tuple(m)], got[tuple(m)]
        if len(s) == 1:
            uniq += 1
            assert np.float32(r).view(np.uint32) == np.float32(g).view(np.uint32), (m, r, g)
        else:
            ties += 1
            vals = inp[tuple(s.T)]
            assert np.any(vals.view(np.uint32) == np.float32(r).view(np.uint32)), (m, r, vals)
            assert np.any(vals.view(np.uint32) == np.float32(g).view(np.uint32)), (m, g, vals)
    return uniq, ties


@pytest.fixture(scope="module")
def g13():
    return np.load(G13)


@pytest.mark.parametrize("case", [c for c in CASES if c not in ("few_known", "nan_free")])
def test_oracle_matches_reference_up_to_ties(g13, case):
    inp, ref = g13[f"{case}/input"], g13[f"{case}/output"]
    assert np.isnan(inp).any()
    uniq, ties = check_against_reference(inp, ref, NO.nan_fill(inp))
    assert uniq + ties == int(np.isnan(inp).sum())


def test_oracle_tie_free_case_is_bit_equal(g13):
    inp, ref = g13["tie_free/input"], g13["tie_free/output"]
    _, sets = NO.tie_sets(inp)
    assert all(len(s) == 1 for s in sets)
    assert np.array_equal(NO.nan_fill(inp).view(np.uint32), ref.view(np.uint32))


def test_oracle_few_known_zeroes_everything(g13):
    inp, ref = g13["few_known/input"], g13["few_known/output"]
    assert (~np.isnan(inp)).sum() < 4
    got = NO.nan_fill(inp)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert not got.any()


def test_oracle_nan_free_is_untouched(g13):
    inp, ref = g13["nan_free/input"], g13["nan_free/output"]
    assert np.array_equal(NO.nan_fill(inp).view(np.uint32), inp.view(np.uint32))
    assert np.array_equal(ref.view(np.uint32), inp.view(np.uint32))


def test_oracle_fills_across_channels():
    """The distance is 3-D: a NaN takes the other channel's value at the same pixel (distance 1) before a farther in-plane entry."""
    a = np.arange(2 * 3 * 3, dtype=np.float32).reshape(2, 3, 3)
    a[0, :, :] = np.nan
    a[0, 0, 0] = 100.0
    got = NO.nan_fill(a)
    assert got[0, 2, 2] == a[1, 2, 2]
    assert got[0, 0, 1] == 100.0                        # in-plane distance 1 beats the other channel (also 1) by channel order


def test_box_search_equals_brute_force():
    rng = np.random.default_rng(5)
    a = rng.normal(size=(3, 40, 60)).astype(np.float32)
    a[rng.random(a.shape) < 0.6] = np.nan
    a[:, 10:30, 20:50] = np.nan
    full = NO.nan_fill(a)
    for site in np.argwhere(np.isnan(a))[::37]:
        assert NO.nearest_value_box(a, site, start=1) == full[tuple(site)]


def test_decision_rule_of_the_orbits():
    """The 5 % rule of data/PopulationDataset.py:426,486 (host helper, no device needed)."""
    from popcorn_amd.data.nanfill import s1_orbit
    assert s1_orbit(0, 100, False) == ("desc", False)
    assert s1_orbit(4, 100, False) == ("desc", True)
    assert s1_orbit(5, 100, False) == ("asc", None)      # 5 / 100 is not < 0.05
    assert s1_orbit(1, 100, True) == ("asc", None)
    assert s1_orbit(0, 100, True) == ("desc", False)     # no NaN: the descending orbit stays, ascfill or not


def test_offset_walk_equals_brute_force():
    rng = np.random.default_rng(11)
    for shape, p in (((4, 50, 70), 0.3), ((2, 33, 41), 0.8), ((3, 20, 25), 0.97)):
        a = rng.integers(0, 4, shape).astype(np.float32)          # few distinct values: ties everywhere, the source decides
        a[rng.random(shape) < p] = np.nan
        a[:, 5:15, 10:30] = np.nan
        m = ~np.isnan(a)
        a[m] = np.arange(m.sum(), dtype=np.float32)               # unique values: equal values mean the same source
        assert np.array_equal(NO.nan_fill_offsets(a, radius=6), NO.nan_fill(a))
