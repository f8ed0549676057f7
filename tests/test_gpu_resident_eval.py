"""Resident evaluation (csrc/region_window.hip, ops.region_window, data/region.py: ResidentWindows, run_eval --resident_windows, run_train
--resident_test) against the paths it replaces, fp32 compared as integers:

  1. without a table   region_window(window, orbit) == select_normalize(cat(S2, S1 of region_gather(window, orbit))) on every non-NaN
                       element, NaN at exactly the same sites;
  2. with the table    ResidentWindows(...)(x, y, s, ps) == eval.raw_window_input(data(x, y, s, ps), ascfill)[0] bit for bit, and its orbit
                       is that function's second return, for every window of the list;
  3. through eval      evaluate_raster(models, ResidentWindows(...)) returns the four maps of evaluate_raster(models, data.raster,
                       raw=True, ascfill=...) bit for bit, likewise the product grid and the census table."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

H, W, SEASONS = 70, 90, 2
DUP_BANDS = (2, 0, 2, 4, 1, 0)             # S2 band 2 twice, out of 5; S1 bands out of 3
MODEL_BANDS = (0, 1, 2, 3, 0, 1)
NAN = float("nan")
_CACHE = {}


def _stats():
    from popcorn_amd.data import stats
    return stats.MEAN6, stats.STD6


def _sources(kind):
    """(s2 (2, 5, 70, 90) fp32 or uint16, s1 (2, 3, 70, 90), s1_asc likewise, boundary) on the device, NaNs at stated coordinates."""
    if kind not in _CACHE:
        g = torch.Generator().manual_seed(11)
        s2 = torch.randint(0, 10000, (SEASONS, 5, H, W), generator=g).float()
        s1 = torch.randn(SEASONS, 3, H, W, generator=g) * 4 - 12
        asc = torch.randn(SEASONS, 3, H, W, generator=g) * 4 - 12
        if kind == "f32":
            s2[0, 2, 0, 0] = NAN; s2[0, 2, 1, 3] = NAN; s2[1, 0, H - 1, W - 1] = NAN; s2[0, 4, 10:14, 20:31] = NAN; s2[1, 2, 33, :] = NAN
        s1[0, 1, 0, 0] = NAN; s1[0, 0, 2, 5] = NAN; s1[1, 1, H - 1, W - 1] = NAN; s1[0, 0, 40:43, :] = NAN; s1[1, 0, :, 7] = NAN
        asc[0, 0, 0, 1] = NAN; asc[1, 1, H - 2, W - 1] = NAN; asc[0, 1, 36, 30:50] = NAN
        if kind == "u16":
            s2 = s2.to(torch.int32).to(torch.uint16)
        boundary = (torch.arange(H * W, dtype=torch.int32).reshape(H, W) % 7)
        _CACHE[kind] = tuple(t.cuda() for t in (s2, s1, asc, boundary))
    return _CACHE[kind]


def _by_gather(s2, s1, asc, boundary, bands, x, y, season, ps, orbit):
    """Definition 1's right-hand side"""
    from popcorn_amd import ops
    mean6, std6 = _stats()
    t = ops.region_gather(s2, s1, boundary, bands, [(x, x + ps, y, y + ps, season)], s1_asc=asc, orbit=[orbit])
    return ops.select_normalize(torch.cat([t["S2"], t["S1"]], 1).contiguous(), tuple(range(6)), mean6, std6)


def _same_where_not_nan(got, want):
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool((got.view(torch.int32)[~gn] == want.view(torch.int32)[~wn]).all())


# ---- definition 1 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [32, 33, 36])
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_window_without_table_equals_gather_then_normalize(kind, ps):
    from popcorn_amd import ops
    s2, s1, asc, boundary = _sources(kind)
    mean6, std6 = _stats()
    out = torch.full((1, 6, ps, ps), 123.0, device="cuda")              # reused between the calls: a site nobody stores keeps a stale window
    shifted = torch.full((6 * ps * ps + 1,), 123.0, device="cuda")[1:].view(1, 6, ps, ps)      # 4-byte aligned only: the scalar path at any ps
    nans = 0
    for (x, y), orbit, season in [(o, b, s) for o in ((0, 0), (1, 3), (H - ps, W - ps)) for b in (0, 1) for s in (0, 1)]:
        want = _by_gather(s2, s1, asc, boundary, DUP_BANDS, x, y, season, ps, orbit)
        got = ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6, out=out, s1_asc=asc, orbit=orbit)
        assert got is out and _same_where_not_nan(got, want), (kind, ps, x, y, orbit, season)
        fresh = ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6, s1_asc=asc, orbit=orbit)
        assert tuple(fresh.shape) == (1, 6, ps, ps) and _same_where_not_nan(fresh, want)
        ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6, out=shifted, s1_asc=asc, orbit=orbit)
        assert _same_where_not_nan(shifted, want), ("unaligned out", kind, ps, x, y, orbit, season)
        nans += int(torch.isnan(want).sum())
        if orbit == 0:                                                   # without s1_asc / orbit: the descending raster
            plain = ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6)
            assert _same_where_not_nan(plain, want)
    assert nans > 0                                                      # the NaN sites were part of the comparison


# ---- definition 2 at the op level -------------------------------------------------------------------------------------------------------
PS2, X0, Y0 = 36, 5, 7


def _clean():
    g = torch.Generator().manual_seed(23)
    s2 = torch.randint(1, 10000, (1, 4, H, W), generator=g).float()
    s1 = torch.randn(1, 2, H, W, generator=g) * 4 - 12
    asc = torch.randn(1, 2, H, W, generator=g) * 4 - 12
    return s2, s1, asc


def _disc(t, band, cx, cy, r):
    ii, jj = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    t[0, band][(ii - cx) ** 2 + (jj - cy) ** 2 <= r * r] = NAN


def _hand_cases():
    """name -> (s2, s1, asc, [windows (x, y)], expected orbit name per window)"""
    from popcorn_amd import ops
    R = ops.region_window_rows(PS2)
    assert 1 <= R < PS2
    numel = 2 * PS2 * PS2
    hi = -(-numel // 20)                                                 # the first count at or above 5 %
    cases = {}
    s2, s1, asc = _clean()
    s2[0, 0, X0, Y0] = NAN
    s1[0, 1, X0 + PS2 - 1, Y0 + PS2 - 1] = NAN
    cases["first_and_last_element"] = (s2, s1, asc, [(X0, Y0)], ["desc"])
    s2, s1, asc = _clean()
    s2[0, 1, X0 + 17, Y0:Y0 + PS2] = NAN
    cases["whole_row"] = (s2, s1, asc, [(X0, Y0)], ["desc"])
    s2, s1, asc = _clean()
    for b in range(4):
        _disc(s2, b, X0 + R, Y0 + 18, 5)                                 # rows R - 5 .. R + 5 of the window: two row blocks of the kernel
    _disc(s2, 2, X0 + 2 * R + 1, Y0 + 30, 3)
    cases["disc_across_row_blocks"] = (s2, s1, asc, [(X0, Y0)], ["desc"])
    s2, s1, asc = _clean()
    s2[0, :, 22:30, Y0:Y0 + PS2] = NAN                                   # rows 22 .. 29 over the whole width: window (25, 7) starts inside the block
    cases["overlap_of_two_windows"] = (s2, s1, asc, [(X0, Y0), (25, Y0)], ["desc", "desc"])
    s2, s1, asc = _clean()
    keep = [(0, X0 + 3, Y0 + 4), (2, X0 + 20, Y0 + 9), (3, X0 + 35, Y0 + 35)]
    vals = [float(s2[0, c, i, j]) for c, i, j in keep]
    s2[0, :, X0:X0 + PS2, Y0:Y0 + PS2] = NAN
    for (c, i, j), v in zip(keep, vals):
        s2[0, c, i, j] = v
    cases["s2_three_known"] = (s2, s1, asc, [(X0, Y0)], ["desc"])

    def holes(t, n):                                                     # the first n entries of the window's band 0, row-major
        win = t[0, 0, X0:X0 + PS2, Y0:Y0 + PS2].clone().reshape(-1)
        win[:n] = NAN
        t[0, 0, X0:X0 + PS2, Y0:Y0 + PS2] = win.reshape(PS2, PS2)

    s2, s1, asc = _clean()
    holes(s1, hi - 1)
    cases["s1_just_below_5_percent"] = (s2, s1, asc, [(X0, Y0)], ["desc"])
    s2, s1, asc = _clean()
    holes(s1, hi)
    cases["s1_at_5_percent"] = (s2, s1, asc, [(X0, Y0)], ["asc"])
    s2, s1, asc = _clean()
    holes(s1, hi)
    holes(asc, hi - 1)
    cases["asc_below_5_percent"] = (s2, s1, asc, [(X0, Y0)], ["asc"])
    return cases


def _window_table(d2, d1, da, db, x, y, orbit):
    """The patch table of one window as the plan builds it: gather, fill on a clone, extract."""
    from popcorn_amd import ops
    t = ops.region_gather(d2, d1, db, MODEL_BANDS, [(x, x + PS2, y, y + PS2, 0)], s1_asc=da, orbit=[orbit])
    f2, f1 = t["S2"].clone(), t["S1"].clone()
    ops.nan_fill_(f2, t["data_hw"])
    ops.nan_fill_(f1, t["data_hw"])
    idx, val, per_item = ops.region_patch_extract(t, {"S2": f2, "S1": f1})
    assert int(per_item.sum()) == idx.numel()
    return idx, val


def _reference_input(s2, s1, asc, x, y, ascfill=False):
    """eval.raw_window_input on the window, the per-window path of evaluate_raster(raw=True)"""
    from popcorn_amd import eval as E
    cut = lambda t: t[:, :, x:x + PS2, y:y + PS2].clone(memory_format=torch.contiguous_format)      # noqa: E731
    return E.raw_window_input({"S2": cut(s2), "S1": cut(s1), "S1_asc": lambda: cut(asc)}, ascfill)


@pytest.mark.parametrize("name", ["first_and_last_element", "whole_row", "disc_across_row_blocks", "overlap_of_two_windows",
                                  "s2_three_known", "s1_just_below_5_percent", "s1_at_5_percent", "asc_below_5_percent"])
def test_window_with_table_equals_the_per_window_fill(name):
    from popcorn_amd import ops
    from popcorn_amd.data.region import window_orbits
    mean6, std6 = _stats()
    s2, s1, asc, windows, want_orbit = _hand_cases()[name]
    d2, d1, da = s2.cuda(), s1.cuda(), asc.cuda()
    db = torch.zeros(H, W, dtype=torch.int32, device="cuda")
    counts = ops.region_nan_census(d2, d1, db, MODEL_BANDS, [(x, x + PS2, y, y + PS2, 0) for x, y in windows], s1_asc=da).cpu()
    orbits = window_orbits(counts, [(x, y, 0) for x, y in windows], PS2, False, True).tolist()
    outs = []
    for (x, y), orbit, name_o in zip(windows, orbits, want_orbit):
        want, ref_orbit = _reference_input(d2, d1, da, x, y)
        assert ref_orbit == name_o == ("asc" if orbit else "desc")
        assert not bool(torch.isnan(want).any())
        idx, val = _window_table(d2, d1, da, db, x, y, orbit)
        # (the descending S1 at 5 % switches to a NaN-free ascending orbit over a NaN-free S2: the one case with nothing to patch)
        assert (idx.numel() > 0) == (name != "s1_at_5_percent") and bool((idx[1:] > idx[:-1]).all())
        # the slice sits in the middle of a longer table whose other entries would damage the window if they were read
        junk_i = torch.tensor([0, 5, 6 * PS2 * PS2 - 1], dtype=torch.int32, device="cuda")
        junk_v = torch.full((3,), 1e30, device="cuda")
        tab_i, tab_v = torch.cat([junk_i, idx, junk_i]), torch.cat([junk_v, val, junk_v])
        out = torch.full((1, 6, PS2, PS2), NAN, device="cuda")
        got = ops.region_window(d2, d1, MODEL_BANDS, (x, y, 0), PS2, mean6, std6, out=out, s1_asc=da, orbit=orbit,
                                table=(tab_i, tab_v, 3, idx.numel()))
        assert bit_equal(got, want), (name, x, y)
        outs.append((got.clone(), idx, val))
    if name == "s2_three_known":
        # fewer than 4 known entries -> zeros: the table holds entries at sites that were NOT NaN (the three known values)
        idx = outs[0][1]
        assert int((idx < 4 * PS2 * PS2).sum()) == 4 * PS2 * PS2 and bool((outs[0][2][idx < 4 * PS2 * PS2] == 0).all())
    if name == "overlap_of_two_windows":
        # global rows 25 .. 29 lie in both windows (rows 20 .. 24 of the first, 0 .. 4 of the second) and inside the NaN block: each window
        # equals its own fill (above).  Row 25 is 4 rows below known row 21, which only the first window holds, and 5 above row 30: the first
        # window fills it from above, the second from below, so the two fills differ there
        a, b = outs[0][0][0, :4, 25 - X0:30 - X0, :], outs[1][0][0, :4, 0:5, :]
        assert a.shape == b.shape and not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any())
        assert a[0, 0, 4].item() != b[0, 0, 4].item() and bool((a != b).any())


def test_window_table_case_without_entries_needs_no_tables():
    """The descending S1 at 5 % switches to a NaN-free ascending orbit: nothing to patch, count = 0 with or without the tables."""
    from popcorn_amd import ops
    mean6, std6 = _stats()
    s2, s1, asc, _, _ = _hand_cases()["s1_at_5_percent"]
    d2, d1, da = s2.cuda(), s1.cuda(), asc.cuda()
    db = torch.zeros(H, W, dtype=torch.int32, device="cuda")
    want, orbit = _reference_input(d2, d1, da, X0, Y0)
    assert orbit == "asc"
    idx, val = _window_table(d2, d1, da, db, X0, Y0, 1)
    assert idx.numel() == 0
    for table in (None, (None, None, 0, 0), (idx, val, 0, 0)):
        assert bit_equal(ops.region_window(d2, d1, MODEL_BANDS, (X0, Y0, 0), PS2, mean6, std6, s1_asc=da, orbit=1, table=table), want)


# ---- footprint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [33, 36])
def test_window_footprint_every_element_written_nothing_outside(ps):
    from popcorn_amd import ops
    mean6, std6 = _stats()
    s2, s1, asc = _clean()
    for b in range(4):
        _disc(s2, b, 20, 25, 6)
    s1[0, 0, 12, :] = NAN
    x, y = H - ps, W - ps                                                # the window ends at the raster's last element
    _disc(s2, 1, H - 3, W - 4, 4)
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, da = fp.place(s2), fp.place(s1), fp.place(asc)
        db = fp.place(torch.zeros(H, W, dtype=torch.int32))
        t = ops.region_gather(d2, d1, db, MODEL_BANDS, [(x, x + ps, y, y + ps, 0)])
        f2, f1 = t["S2"].clone(), t["S1"].clone()
        ops.nan_fill_(f2, t["data_hw"])
        ops.nan_fill_(f1, t["data_hw"])
        idx, val, _ = ops.region_patch_extract(t, {"S2": f2, "S1": f1})
        want = ops.select_normalize(torch.cat([f2, f1], 1).contiguous(), tuple(range(6)), mean6, std6)
        out = fp.alloc((1, 6, ps, ps), torch.float32)                    # poisoned: 0xFF bytes = NaN
        assert bool(torch.isnan(out).all())
        got = ops.region_window(d2, d1, MODEL_BANDS, (x, y, 0), ps, mean6, std6, out=out, table=(idx, val, 0, idx.numel()))
        fresh = ops.region_window(d2, d1, MODEL_BANDS, (x, y, 0), ps, mean6, std6, table=(idx, val, 0, idx.numel()))      # its own empty()
    assert idx.numel() > 0
    assert not bool(torch.isnan(got).any()) and bit_equal(got, want) and bit_equal(fresh, want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_window_refusals_enqueue_nothing():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    s2, s1, asc, _ = _sources("f32")
    mean6, std6 = _stats()
    ps = 32
    out = torch.full((1, 6, ps, ps), 7.0, device="cuda")
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    val = torch.ones(4, device="cuda")
    ok = dict(s2=s2, s1=s1, band_sel=DUP_BANDS, window=(1, 3, 0), ps=ps, mean6=mean6, std6=std6, out=out, s1_asc=asc, orbit=1,
              table=(idx, val, 0, 4))
    bad = [dict(ps=0), dict(ps=L.PC_REGION_WINDOW_MAX_PS + 1), dict(window=(H - ps + 1, 0, 0)), dict(window=(0, W - ps + 1, 0)),
           dict(window=(-1, 0, 0)), dict(window=(0, -1, 0)), dict(window=(0, 0, SEASONS)), dict(window=(0, 0, -1)), dict(window=(0, 0)),
           dict(band_sel=(5, 0, 2, 4, 1, 0)), dict(band_sel=(2, 0, 2, 4, 3, 0)), dict(band_sel=(2, 0, 2, 4, 1)),
           dict(s1_asc=None), dict(orbit=2), dict(orbit=-1), dict(s1_asc=asc[:1].contiguous()),
           dict(table=(None, None, 0, 4)), dict(table=(idx, None, 0, 4)), dict(table=(idx, val, 2, 3)), dict(table=(idx, val, -1, 2)),
           dict(table=(idx, val, 0, -1)), dict(table=(idx.long(), val, 0, 4)), dict(table=(idx.cpu(), val.cpu(), 0, 4)),
           dict(out=torch.full((1, 6, ps, ps + 1), 7.0, device="cuda")), dict(out=out.double()), dict(mean6=mean6[:5]),
           dict(s2=s2[:, :, :, ::2]), dict(s1=s1[:1].contiguous()), dict(s2=s2.half())]
    for kw in bad:
        with pytest.raises((ValueError, L.PopcornHipError)) as e:
            ops.region_window(**{**ok, **kw})
        assert e.type is ValueError or "cpu" in str(e.value), kw
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), kw
    # the library's own checks: PC_EINVAL with nothing enqueued -- out keeps its fill
    def call(s2_=s2, s1_=s1, asc_=asc, orbit=1, bands=DUP_BANDS, x=1, y=3, season=0, ps_=ps, mean_=True, idx_=idx, val_=val, cap=4,
             start=0, count=4, out_=out):
        return L.lib().pc_region_window(L.ptr(s2_), 0, L.ptr(s1_), L.ptr(asc_), orbit, SEASONS, 5, 3, H, W, (C.c_int32 * 6)(*bands), x, y,
                                        season, ps_, (C.c_float * 6)(*mean6) if mean_ else None, (C.c_float * 6)(*std6), L.ptr(idx_),
                                        L.ptr(val_), C.c_int64(cap), C.c_int64(start), C.c_int64(count), L.ptr(out_), L.stream_ptr())
    for kw in (dict(s2_=None), dict(s1_=None), dict(out_=None), dict(mean_=False), dict(ps_=0), dict(ps_=L.PC_REGION_WINDOW_MAX_PS + 1),
               dict(x=H - ps + 1), dict(y=W - ps + 1), dict(x=-1), dict(y=-1), dict(season=SEASONS), dict(season=-1),
               dict(bands=(5, 0, 2, 4, 1, 0)), dict(bands=(2, 0, 2, 4, 1, 3)), dict(asc_=None), dict(orbit=2), dict(idx_=None),
               dict(val_=None), dict(start=1), dict(cap=3), dict(count=-1), dict(start=-1, count=1), dict(count=6 * ps * ps + 1, cap=1 << 20)):
        assert call(**kw) == L.PC_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), kw
    assert call() == 0 and call(asc_=None, orbit=0, idx_=None, val_=None, cap=0, count=0) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())


# ---- definitions 2 and 3, end to end ----------------------------------------------------------------------------------------------------
EH, EW, EPS, EOV = 150, 170, 64, 8


def _e2e():
    """The raster, the region, two models and -- computed ONCE and left unchanged -- the per-window reference inputs and orbits."""
    if "e2e" not in _CACHE:
        from popcorn_amd import eval as E
        from popcorn_amd.data.dataset import SyntheticTestRaster
        from popcorn_amd.data.region import ResidentRegion
        from popcorn_amd.model.popcorn import POPCORN
        data = SyntheticTestRaster(EH, EW, seasons=4, n_regions=16, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.05)
        region = ResidentRegion.from_synthetic(data, with_asc=True)
        models = []
        for k in range(2):
            torch.manual_seed(40 + k)
            models.append(POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval())
        idx = E.get_patch_indices(EH, EW, EPS, EOV, True)
        ref = {}
        for ascfill in (False, True):
            ref[ascfill] = [E.raw_window_input(data(x, y, s, EPS), ascfill) for x, y, s in idx.tolist()]
        _CACHE["e2e"] = (data, region, models, idx, ref)
    return _CACHE["e2e"]


@pytest.mark.parametrize("ascfill", [False, True])
def test_resident_windows_equal_the_per_window_path_end_to_end(ascfill, monkeypatch):
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd.data.region import ResidentWindows
    data, region, models, idx, ref = _e2e()
    n = idx.shape[0]
    assert n == 48
    feed = ResidentWindows(region, EPS, EOV, fourseasons=True, ascfill=ascfill)
    assert feed.shape == (EH, EW) and torch.equal(feed.idx, idx) and tuple(feed.orbit.shape) == (n,) and tuple(feed.counts.shape) == (n, 3)
    # all three outcomes occur, before anything is compared: S1 without NaN, filled on the descending orbit, switched to the ascending one
    s1_nan = feed.counts[:, 1] > 0
    clean, filled, switched = int((~s1_nan).sum()), int((s1_nan & (feed.orbit == 0)).sum()), int((feed.orbit == 1).sum())
    if not ascfill:
        assert (clean, filled, switched) == (12, 20, 16) and int((feed.counts[:, 0] > 0).sum()) == 27
    else:
        assert (clean, filled, switched) == (12, 0, 36)
    assert feed.ascending == switched and feed.entries > 0 and feed.nbytes == 8 * feed.entries and feed.build_ms > 0
    # the census itself, against torch on the windows
    for k in (0, 7, n - 1):
        x, y, s = idx[k].tolist()
        cut = lambda t: int(torch.isnan(t[s, :, x:x + EPS, y:y + EPS]).sum())      # noqa: E731
        assert feed.counts[k].tolist() == [cut(data.s2), cut(data.s1), cut(data.s1_asc)]
    # definition 2: every window, bit for bit, and its orbit -- with the per-window fill taken away
    raster_raw = E.evaluate_raster(models, data.raster, EPS, EOV, True, raw=True, ascfill=ascfill,
                                   product=(p_raw := E.ProductGrid(EH, EW, 10, 2, "cuda")),
                                   census=(c_raw := E.CensusTable(EH, EW, [data.boundary], [17], 2, "cuda")))
    def no_fill(*a, **k):
        raise AssertionError("the resident evaluation ran a per-window fill")
    monkeypatch.setattr(ops, "nan_fill_", no_fill)
    for k, (x, y, s) in enumerate(idx.tolist()):
        want, orbit = ref[ascfill][k]
        got = feed(x, y, s, EPS)
        assert tuple(got.shape) == (1, 6, EPS, EPS) and bit_equal(got, want), (k, x, y, s)
        assert ("asc" if int(feed.orbit[k]) else "desc") == orbit, k
    # definition 3: the four maps, the product and the census table
    raster_res = E.evaluate_raster(models, feed, EPS, EOV, True, product=(p_res := E.ProductGrid(EH, EW, 10, 2, "cuda")),
                                   census=(c_res := E.CensusTable(EH, EW, [data.boundary], [17], 2, "cuda")))
    for a, b in zip(raster_raw, raster_res):
        assert bit_equal(a, b)
    assert bool(torch.isfinite(raster_res[0]).all()) and float(raster_res[0].abs().sum()) > 0
    assert bit_equal(p_raw.mean, p_res.mean) and bit_equal(p_raw.std, p_res.std) and bit_equal(p_raw.cells, p_res.cells)
    assert torch.equal(c_raw.table, c_res.table) and bit_equal(c_raw.mean, c_res.mean) and bit_equal(c_raw.std, c_res.std)
    # what is not planned raises
    for args in ((1, 0, 0, EPS), (0, 0, 4, EPS), (0, 0, 0, EPS - 1)):
        with pytest.raises(ValueError, match="not planned"):
            feed(*args)


def test_no_data_window_is_named_at_construction():
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import ResidentRegion, ResidentWindows
    data = SyntheticTestRaster(100, 120, seasons=1, n_regions=9, seed=3, device="cuda", raw=True)
    from popcorn_amd import eval as E
    idx = E.get_patch_indices(100, 120, 64, 8, False).tolist()
    x, y, s = idx[2]
    numel = 2 * 64 * 64
    hi = -(-numel // 20)
    rows = -(-hi // 64)                                                  # whole rows of one band: at or above 5 % of the window
    data.s1[0, 0, x + 20:x + 20 + rows, y:y + 64] = NAN
    data.s1_asc[0, 1, x + 30:x + 30 + rows, y:y + 64] = NAN
    region = ResidentRegion.from_synthetic(data, with_asc=True)
    with pytest.raises(ValueError) as e:
        ResidentWindows(region, 64, 8)
    assert "No data here!" in str(e.value) and "ResidentWindows" in str(e.value)
    m = re.search(r"\((\d+), (\d+), (\d+)\)", str(e.value))
    named = tuple(int(v) for v in m.groups())
    assert list(named) in idx
    # the named window is the first of the list both of whose orbits are at or above 5 %
    def frac(t, w):
        return int(torch.isnan(t[w[2], :, w[0]:w[0] + 64, w[1]:w[1] + 64]).sum()) * 20 >= numel
    lacking = [w for w in idx if frac(data.s1, w) and frac(data.s1_asc, w)]
    assert list(idx[2]) in lacking and list(named) == lacking[0]
    # without the ascending raster the descending orbit is filled at any fraction: the plan builds
    feed = ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=False), 64, 8)
    assert feed.ascending == 0 and feed.entries > 0
    with pytest.raises(ValueError, match="ascfill"):
        ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=False), 64, 8, ascfill=True)


def test_ranks_share_the_orbit_column_and_split_the_table():
    from popcorn_amd.data.region import ResidentWindows
    data, region, models, idx, ref = _e2e()
    one = ResidentWindows(region, EPS, EOV, fourseasons=True)
    parts = [ResidentWindows(region, EPS, EOV, fourseasons=True, rank=r, world=2) for r in range(2)]
    assert torch.equal(parts[0].orbit, one.orbit) and torch.equal(parts[1].orbit, one.orbit)
    assert torch.equal(parts[0].counts, one.counts) and torch.equal(parts[1].counts, one.counts)
    assert parts[0].entries > 0 and parts[1].entries > 0 and parts[0].entries + parts[1].entries == one.entries
    assert sorted(parts[0].mine + parts[1].mine) == list(range(idx.shape[0])) and not set(parts[0].mine) & set(parts[1].mine)
    for k, (x, y, s) in enumerate(idx.tolist()):
        r = k % 2
        assert bit_equal(parts[r](x, y, s, EPS), one(x, y, s, EPS)), k
        with pytest.raises(ValueError, match="rank"):
            parts[1 - r](x, y, s, EPS)
    with pytest.raises(ValueError):
        ResidentWindows(region, EPS, EOV, rank=2, world=2)


# ---- the front ends ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", ["", "--product_cell 10 --census_table", "--ascfill --fourseasons"])
def test_run_eval_resident_windows_prints_the_metrics_of_raw_input(extra, capsys):
    from popcorn_amd import cli
    base = ("-S2 -NIR -S1 -occmodel -senbuilds -pret --biasinit 0.9407 --raster_hw 150 170 --patchsize 64 --overlap 8 --ensemble 2 "
            "--nan_clouds 0.05 --s1_gap 0.05 " + extra).split()
    raw = cli.run_eval(base + ["--raw_input"])
    printed_raw = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    res = cli.run_eval(base + ["--resident_windows"])
    lines = capsys.readouterr().out.strip().splitlines()
    printed_res = json.loads(lines[-1])
    build = [ln for ln in lines if ln.startswith("resident windows:")]
    assert len(build) == 1 and all(w in build[0] for w in ("windows", "ascending", "entries", "bytes", "ms"))
    for a, b in ((raw, res), (printed_raw, printed_res)):
        a, b = dict(a), dict(b)
        a.pop("seconds"), b.pop("seconds")
        assert a == b and len(a) > 4
    if "--census_table" in extra:
        assert "product_total" in res and any(k.endswith("_members_std") for k in res)


def test_run_train_resident_test_plans_once_and_equals_the_raw_evaluation(tmp_path, capsys):
    from popcorn_amd import cli
    from popcorn_amd import eval as E
    from popcorn_amd.utils.metrics import get_test_metrics
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 2 -wb 2 -lt 1 --resident_region 150 170 --resident_units 24 "
            "--resident_test --test_patchsize 64 --test_overlap 8 --val_every_n_epochs 1 --save-model no --nan_clouds 0.05 "
            f"--save_dir {tmp_path}").split()
    a = cli.train_parser().parse_args(argv)
    t = cli.Trainer(a)
    assert t.region.s1_asc is not None and t._resident_windows is None
    # the first test, before any step: the same weights through the per-window path over the same data
    first = dict(t.test_target())
    feed = t._resident_windows
    assert feed is not None and feed.entries > 0
    out, _, _, _ = E.evaluate_raster([t.model], t.region_data.raster, 64, 8, False, raw=True, ascfill=False)
    cp, cg = E.convert_popmap_to_census(out, t.region.boundary, t.region.census_idx, t.region.census_pop)
    want = {k + "/targettest": float(v) for k, v in get_test_metrics(cp, cg, tag="MainCensus_synthetic_fine").items()}
    assert first == want and len(first) > 2
    t.train()
    assert t._resident_windows is feed                                   # planned once, reused
    lines = capsys.readouterr().out.splitlines()
    assert len([ln for ln in lines if ln.startswith("resident windows:")]) == 1
    log = [json.loads(ln) for ln in open(os.path.join(t.exp, "train_log.jsonl"))]
    tests = [r for r in log if any(k.endswith("/targettest") for k in r)]
    assert len(tests) == 3 and [r["epoch"] for r in tests] == [0, 1, 2]        # the one above, then one per epoch
    assert {k: v for k, v in tests[0].items() if k.endswith("/targettest")} == want
    assert all(all(v == v for k, v in r.items() if k.endswith("/targettest")) for r in tests)
