"""The resident repair on the GPU (csrc/region_repair.hip and everything above it): the census, the orbit-aware gathers, the patch table
and its application, the orbit column, the feeds and the trainer flags.

The oracle of the application is the chain it replaces, bit for bit (fp32 compared as int32):

    patch_apply(region_batch(crops, orbit, coins))  ==  augment_raw(fill_sample_(region_gather(crops, orbit)), coins)

Inputs are the rasters of tests/region_repair_oracle.py (37 x 53 and 96 x 128, two seasons, five S2 and three S1 bands, a band selection
that is not the identity) with NaNs at stated coordinates; every class of item a test relies on is asserted present.  Outputs sit in poisoned
memory between the guard bands of tests/footprint.py."""
import itertools
import random

import pytest
import torch

from tests import region_oracle as R
from tests import region_repair_oracle as O
from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

S, BANDS = O.S, O.BANDS
GEOMETRY = list(itertools.product((False, True), (False, True), (0, 1, 2, 3)))        # 16 x (vflip, hflip, rot)
VALUES = [(None, None), (1.3, None), (None, 0.8), (0.7, 1.4)]                          # no change, beta, gamma, both
_SRC = {}


def _host(name, kind="f32"):
    if (name, kind) not in _SRC:
        h, w = O.RASTERS[name]
        boundary = R.blocky_raster(h, w) if name == "96x128" else R.irregular_raster(h, w, units=9, seed=2)
        _SRC[(name, kind)] = O.sources(name, kind) + (boundary.to(torch.int32),)
    return _SRC[(name, kind)]


def _fill(tile):
    """fill_sample_ on a clone of a gathered batch"""
    from popcorn_amd.cli import fill_sample_
    f2, f1 = tile["S2"].clone(), tile["S1"].clone()
    fill_sample_(f2, f1, tile)
    return f2, f1


def _composite(d2, d1, da, db, crops, orbit, params, hw=None):
    """augment_raw(fill_sample_(region_gather(crops, orbit)), coins)"""
    from popcorn_amd import ops
    out = None
    if hw is not None:
        B = len(crops)
        out = {"S2": torch.empty(B, 4, *hw, device="cuda"), "S1": torch.empty(B, 2, *hw, device="cuda"),
               "admin_mask": torch.empty(B, *hw, device="cuda"), "data_hw": torch.empty(B, 2, dtype=torch.int32, device="cuda")}
    tile = ops.region_gather(d2, d1, db, BANDS, crops, out=out, s1_asc=da, orbit=orbit)
    f2, f1 = _fill(tile)
    return tile, (f2, f1), ops.augment_raw(f2, f1, tile["admin_mask"], params)


def _table(d2, d1, da, db, crops, orbit):
    """The patch table of a crop list: (idx, val, off host int64 (B + 1,), item_hw)"""
    from popcorn_amd import ops
    tile = ops.region_gather(d2, d1, db, BANDS, crops, s1_asc=da, orbit=orbit)
    f2, f1 = _fill(tile)
    idx, val, per_item = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per_item, 0)])
    return idx, val, off, [(c[1] - c[0], c[3] - c[2]) for c in crops]


# ---- census -----------------------------------------------------------------------------------------------------------------------------
def _boxes(name):
    h, w = O.RASTERS[name]
    g = torch.Generator().manual_seed(7)
    boxes = [(0, h, 0, w, 0), (0, h, 0, w, 1),                                                  # the whole raster
             (10, 11, 5, 6, 0), (h - 1, h, w - 1, w, 1),                                        # one pixel
             (0, 9, 0, 11, 0), (0, 9, w - 11, w, 1), (h - 9, h, 0, 11, 1), (h - 9, h, w - 11, w, 0),      # the four corners
             (3, 24, 5, 32, 0), (7, 30, 11, 27, 1), (1, 12, 3, 26, 0)]                          # odd origins, widths 27, 16, 23
    for _ in range(300):
        x0, y0 = int(torch.randint(0, h - 1, (1,), generator=g)), int(torch.randint(0, w - 1, (1,), generator=g))
        boxes.append((x0, x0 + 1 + int(torch.randint(0, h - x0, (1,), generator=g)), y0, y0 + 1 + int(torch.randint(0, w - y0, (1,), generator=g)),
                      int(torch.randint(0, S, (1,), generator=g))))
    return boxes


@pytest.mark.parametrize("case", ["f32", "dup_bands", "u16", "no_asc"])
@pytest.mark.parametrize("name", sorted(O.RASTERS))
def test_census_equals_isnan_sums(name, case):
    from popcorn_amd import ops
    s2, s1, asc, boundary = _host(name, "u16" if case == "u16" else "f32")
    bands = O.DUP_BANDS if case == "dup_bands" else BANDS
    if case == "no_asc":
        asc = None
    boxes = _boxes(name)
    want = torch.tensor([O.census(s2, s1, asc, bands, b) for b in boxes])
    assert int((want[:, 1] > 0).sum()) > 10 and (case in ("u16",) or int((want[:, 0] > 0).sum()) > 10)
    assert (case == "no_asc") == (int(want[:, 2].sum()) == 0) and (case == "u16") == (int(want[:, 0].sum()) == 0)
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, db = fp.place(s2), fp.place(s1), fp.place(boundary)
        da = None if asc is None else fp.place(asc)
        got = ops.region_nan_census(d2, d1, db, bands, boxes, s1_asc=da)
        again = ops.region_nan_census(d2, d1, db, bands, boxes, s1_asc=da)
        one = ops.region_nan_census(d2, d1, db, bands, boxes, s1_asc=da, max_blocks=1)
        three = ops.region_nan_census(d2, d1, db, bands, boxes, s1_asc=da, max_blocks=3)
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(boxes), 3)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, again) and torch.equal(got, one) and torch.equal(got, three)


def test_census_refusals():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    s2, s1, asc, boundary = (t.cuda() for t in _host("37x53"))
    good = (3, 20, 5, 32, 0)
    for bad in ((3, 3, 5, 32, 0), (3, 20, 30, 54, 0), (3, 20, 5, 32, 2), (-1, 20, 5, 32, 0)):
        with pytest.raises(ValueError):
            ops.region_nan_census(s2, s1, boundary, BANDS, [good, bad], s1_asc=asc)
    with pytest.raises(ValueError):
        ops.region_nan_census(s2, s1, boundary, (5, 0, 2, 1, 2, 0), [good])
    with pytest.raises(ValueError):
        ops.region_nan_census(s2, s1, boundary, BANDS, [good], s1_asc=asc[:1].contiguous())
    # the library's own checks: PC_EINVAL with nothing enqueued -- the counts keep their fill
    import ctypes as C
    counts = torch.full((1, 3), 7, dtype=torch.int64, device="cuda")
    boxes = torch.tensor([good], dtype=torch.int32, device="cuda")

    def call(bands=BANDS, n=1, rows=17, s1_=s1):
        return L.lib().pc_region_nan_census(L.ptr(s2), 0, L.ptr(s1_), L.ptr(asc), S, O.C2, O.C1, 37, 53, (C.c_int32 * 6)(*bands),
                                            L.ptr(boxes), n, rows, L.ptr(counts), 0, L.stream_ptr())
    for kw in (dict(bands=(5, 0, 2, 1, 2, 0)), dict(n=0), dict(rows=0), dict(rows=38), dict(s1_=None)):
        assert call(**kw) == L.PC_EINVAL, kw
        torch.cuda.synchronize()
        assert bool((counts == 7).all()), kw
    assert call() == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [O.census(*_host("37x53")[:3], BANDS, good)]


# ---- orbit gathers ----------------------------------------------------------------------------------------------------------------------
def _random_crops(n, h, w, side, seed):
    g = torch.Generator().manual_seed(seed)
    crops = []
    for _ in range(n):
        x0, y0 = int(torch.randint(0, h - side, (1,), generator=g)), int(torch.randint(0, w - side, (1,), generator=g))
        crops.append((x0, x0 + 1 + int(torch.randint(0, side, (1,), generator=g)), y0, y0 + 1 + int(torch.randint(0, side, (1,), generator=g)),
                      int(torch.randint(0, S, (1,), generator=g))))
    return crops


@pytest.mark.parametrize("n", [3, 130])
def test_orbit_gathers_swap_the_s1_source_per_item(n):
    """A mixed mask over 3 crops and over 130 (two launches: the mask restarts with the second) equals the plain gather with the S1 source
    swapped per item, for the gather and for the assembly; mask zero equals the existing entry points, NaN payloads included."""
    from popcorn_amd import ops
    s2, s1, asc, boundary = _host("37x53")
    s1 = s1.clone()
    s1.view(torch.int32)[1, 2, 20:24, 12:20] = 0x7FC12345               # a NaN with a payload in each orbit
    asc = asc.clone()
    asc.view(torch.int32)[1, 0, 5:9, 0:20] = -0x3FFFFF
    crops = [(3, 24, 2, 30, 0), (7, 30, 11, 27, 1), (1, 12, 3, 25, 1)] if n == 3 else _random_crops(130, 37, 53, 8, seed=4)
    orbit = [1, 0, 1] if n == 3 else torch.randint(0, 2, (130,), generator=torch.Generator().manual_seed(9)).tolist()
    if n == 130:
        orbit[0], orbit[1], orbit[128], orbit[129] = 0, 1, 1, 0      # bit 0 of the first launch is clear, bit 0 of the second is set
    assert 0 < sum(orbit[:128]) < min(n, 128)
    params = {"vflip": True, "hflip": False, "rot": 3, "beta": 1.2, "gamma": None}
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, da, db = fp.place(s2), fp.place(s1), fp.place(asc), fp.place(boundary)
        desc, ascg = ops.region_gather(d2, d1, db, BANDS, crops), ops.region_gather(d2, da, db, BANDS, crops)
        got = ops.region_gather(d2, d1, db, BANDS, crops, s1_asc=da, orbit=orbit)
        zero = ops.region_gather(d2, d1, db, BANDS, crops, s1_asc=da, orbit=[0] * n)
        bd, ba = ops.region_batch(d2, d1, db, BANDS, crops, params), ops.region_batch(d2, da, db, BANDS, crops, params)
        bgot = ops.region_batch(d2, d1, db, BANDS, crops, params, s1_asc=da, orbit=orbit)
        bzero = ops.region_batch(d2, d1, db, BANDS, crops, params, s1_asc=da, orbit=None)
    pick = torch.tensor(orbit, dtype=torch.bool, device="cuda")
    want_s1 = torch.where(pick[:, None, None, None].expand_as(desc["S1"]), ascg["S1"].view(torch.int32), desc["S1"].view(torch.int32))
    assert torch.equal(got["S1"].view(torch.int32), want_s1)
    for key in ("S2", "admin_mask", "data_hw"):
        assert bit_equal(got[key], desc[key]), key
    for key in ("S2", "S1", "admin_mask", "data_hw"):
        assert bit_equal(zero[key], desc[key]), key
    want_raw = torch.where(pick[:, None, None, None].expand_as(bd["raw"]), ba["raw"].view(torch.int32), bd["raw"].view(torch.int32))
    assert torch.equal(bgot["raw"].view(torch.int32), want_raw) and bit_equal(bgot["admin_mask"], bd["admin_mask"])
    assert bit_equal(bzero["raw"], bd["raw"]) and bit_equal(bzero["admin_mask"], bd["admin_mask"])
    if n == 3:
        bits = got["S1"].view(torch.int32)
        assert bool((bits == -0x3FFFFF).any()) and bool((zero["S1"].view(torch.int32) == 0x7FC12345).any())
    # an ascending crop without the ascending raster, a value outside {0, 1}, a list of another length
    d2, d1, da, db = s2.cuda(), s1.cuda(), asc.cuda(), boundary.cuda()
    for kw in (dict(orbit=orbit), dict(s1_asc=da, orbit=[2] + orbit[1:]), dict(s1_asc=da, orbit=orbit[:-1])):
        with pytest.raises(ValueError):
            ops.region_gather(d2, d1, db, BANDS, crops, **kw)
        with pytest.raises(ValueError):
            ops.region_batch(d2, d1, db, BANDS, crops, params, **kw)


# ---- extraction -------------------------------------------------------------------------------------------------------------------------
def test_patch_extract_equals_nonzero_of_the_bit_difference():
    """Three items at a 40 x 44 tile (6 * 1,760 entries: three chunks): one without NaN (no entry), one whose S1 keeps three known entries
    (the fill zeroes it: its S1 differs wherever it was not zero), one where everything differs.  The padding outside the extents differs
    everywhere and yields nothing."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    Hm, Wm = 40, 44
    assert 6 * Hm * Wm > 2 * L.PC_REGION_PATCH_CHUNK
    hw = [(40, 44), (33, 37), (40, 41)]
    g = torch.Generator().manual_seed(12)
    g2 = torch.randint(1, 10000, (3, 4, Hm, Wm), generator=g).float()
    g1 = torch.randn(3, 2, Hm, Wm, generator=g) * 5 - 12
    g1[1] = O.NAN
    g1[1, 0, 4, 5], g1[1, 1, 0, 0], g1[1, 1, 32, 36] = -3.0, -4.0, -5.0          # three known entries
    g2[2], g1[2] = O.NAN, O.NAN
    with Footprint("cuda", fill=POISON) as fp:
        tile = {"S2": fp.place(g2), "S1": fp.place(g1), "data_hw": fp.place(torch.tensor(hw, dtype=torch.int32))}
        f2, f1 = _fill(tile)
        for b, (hb, wb) in enumerate(hw):                              # the padding: other bits in the filled copy
            f2[b, :, hb:, :] += 1.0
            f2[b, :, :, wb:] += 1.0
            f1[b, :, hb:, :] = 1.0
            f1[b, :, :, wb:] = 1.0
        n0 = fp.guarded
        idx, val, per_item = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
        grew = fp.guarded - n0
        again = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
    assert grew >= 3                                                  # counts, idx and val were allocated between guard bands
    assert idx.dtype == torch.int32 and val.dtype == torch.float32 and per_item.tolist() == [0, 2 * 33 * 37, 6 * 40 * 41]
    at = 0
    for b, (hb, wb) in enumerate(hw):
        want_idx, want_val = O.patch_entries(g2[b], g1[b], f2[b].cpu(), f1[b].cpu(), hb, wb)
        n = int(per_item[b])
        got_idx = idx[at:at + n].cpu().to(torch.int64)
        assert torch.equal(got_idx, want_idx), b
        assert bool((got_idx[1:] > got_idx[:-1]).all())              # ascending
        assert bit_equal(val[at:at + n].cpu(), want_val.contiguous()), b
        at += n
    assert at == idx.numel()
    assert bool((val[per_item[0]:per_item[0] + per_item[1]] == 0).all())         # fewer than 4 known entries -> zeros
    assert torch.equal(again[0], idx) and bit_equal(again[1], val) and torch.equal(again[2], per_item)


# ---- application ------------------------------------------------------------------------------------------------------------------------
# S2 and ascending-S1 patches; a NaN-free crop; S2 and descending-S1 patches; a corner crop whose S2 is NaN in every band
APPLY_CROPS = [(3, 24, 2, 30, 0), (7, 30, 11, 27, 1), (1, 12, 3, 25, 0), (28, 37, 38, 53, 1)]
APPLY_ORBIT = [1, 0, 0, 0]


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_patch_apply_equals_gather_fill_augment(kind):
    from popcorn_amd import ops
    s2, s1, asc, boundary = _host("37x53", kind)
    checked = 0
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, da, db = fp.place(s2), fp.place(s1), fp.place(asc), fp.place(boundary)
        idx, val, off, item_hw = _table(d2, d1, da, db, APPLY_CROPS, APPLY_ORBIT)
        count = (off[1:] - off[:-1]).tolist()
        assert count[1] == 0 and min(count[0], count[2]) > 0 and (count[3] > 0) == (kind == "f32")
        c_of = lambda b: (idx[off[b]:off[b + 1]].cpu().to(torch.int64) // (item_hw[b][0] * item_hw[b][1]))       # noqa: E731
        assert bool((c_of(0) == 5).any()) and bool((c_of(2) >= 4).any())                  # S1 patches, ascending and descending
        assert (kind == "u16") == (not bool((c_of(0) < 4).any()))                        # S2 patches where S2 can hold NaN
        for hw in (None, (25, 31)):                                   # the batch maximum 23 x 28 (four-pixel form) and beyond it (one-pixel)
            for (vflip, hflip, rot), (beta, gamma) in itertools.product(GEOMETRY, VALUES):
                params = {"vflip": vflip, "hflip": hflip, "rot": rot, "beta": beta, "gamma": gamma}
                tile, _, (raw, adm) = _composite(d2, d1, da, db, APPLY_CROPS, APPLY_ORBIT, params, hw)
                n0 = fp.guarded
                got = ops.region_batch(d2, d1, db, BANDS, APPLY_CROPS, params, hw=hw, s1_asc=da, orbit=APPLY_ORBIT)
                before = got["raw"][1].clone()
                n = ops.region_patch_apply(idx, val, off[:-1], count, item_hw, got["raw"][:, :4], got["raw"][:, 4:],
                                           tuple(tile["admin_mask"].shape[1:]), params)
                assert n == sum(count) and fp.guarded <= n0 + 3        # the two outputs, the clone, and nothing else
                assert bit_equal(got["raw"], raw), (hw, params)
                assert bit_equal(got["admin_mask"], adm) and bit_equal(got["raw"][1], before)       # an item without entries: untouched
                assert not bool(torch.isnan(got["raw"]).any())
                checked += 1
        # the unfused feed's form: separate S2 / S1 tensors, identity coins
        tile, (f2, f1), _ = _composite(d2, d1, da, db, APPLY_CROPS, APPLY_ORBIT, None)
        ops.region_patch_apply(idx, val, off[:-1], count, item_hw, tile["S2"], tile["S1"], tuple(tile["admin_mask"].shape[1:]))
        assert bit_equal(tile["S2"], f2) and bit_equal(tile["S1"], f1)
    assert checked == 2 * 64


@pytest.mark.parametrize("rot", [0, 1])
def test_patch_apply_more_items_than_one_launch_carries(rot):
    from popcorn_amd import ops
    s2, s1, asc, boundary = _host("37x53")
    crops = _random_crops(130, 37, 53, 12, seed=6)
    orbit = torch.randint(0, 2, (130,), generator=torch.Generator().manual_seed(2)).tolist()
    params = {"vflip": False, "hflip": True, "rot": rot, "beta": None, "gamma": 0.9}
    with Footprint("cuda", fill=POISON) as fp:
        d2, d1, da, db = fp.place(s2), fp.place(s1), fp.place(asc), fp.place(boundary)
        idx, val, off, item_hw = _table(d2, d1, da, db, crops, orbit)
        count = (off[1:] - off[:-1]).tolist()
        assert sum(1 for c in count[:128] if c) > 5 and sum(count[128:]) > 0 and count.count(0) > 5
        tile, _, (raw, _) = _composite(d2, d1, da, db, crops, orbit, params)
        got = ops.region_batch(d2, d1, db, BANDS, crops, params, s1_asc=da, orbit=orbit)
        ops.region_patch_apply(idx, val, off[:-1], count, item_hw, got["raw"][:, :4], got["raw"][:, 4:], tuple(tile["admin_mask"].shape[1:]),
                               params)
    assert bit_equal(got["raw"], raw)


def test_patch_apply_refuses_before_any_launch():
    from popcorn_amd import ops
    s2, s1, asc, boundary = (t.cuda() for t in _host("37x53"))
    idx, val, off, item_hw = _table(s2, s1, asc, boundary, APPLY_CROPS, APPLY_ORBIT)
    count = (off[1:] - off[:-1]).tolist()
    raw = torch.full((4, 6, 23, 28), 7.5, device="cuda")
    args = dict(off=off[:-1], count=count, item_hw=item_hw, hw=(23, 28), params=None)
    for kw in (dict(off=off[:-1] + 1), dict(count=[c + 1 for c in count]), dict(item_hw=[(24, 28)] + item_hw[1:]), dict(hw=(22, 28)),
               dict(params={"rot": 4}), dict(params={"rot": 1})):
        a = dict(args, **kw)
        with pytest.raises(ValueError):
            ops.region_patch_apply(idx, val, a["off"], a["count"], a["item_hw"], raw[:, :4], raw[:, 4:], a["hw"], a["params"])
    torch.cuda.synchronize()
    assert bool((raw == 7.5).all())
    assert ops.region_patch_apply(idx, val, off[:-1], [0, 0, 0, 0], item_hw, raw[:, :4], raw[:, 4:], (23, 28)) == 0      # no entry: no launch
    assert ops.region_patch_apply(idx, val, off[:-1], count, item_hw, raw[:, :4], raw[:, 4:], (23, 28)) == sum(count)
    torch.cuda.synchronize()
    assert int((raw != 7.5).sum()) == sum(count)


# ---- the orbit column and the plan ------------------------------------------------------------------------------------------------------
def _region(name, with_asc=True, kind="f32"):
    from popcorn_amd.data.region import ResidentRegion
    s2, s1, asc, boundary = _host(name, kind)
    n = int(boundary.max())
    ids, pop = torch.arange(1, n + 1), torch.rand(n, generator=torch.Generator().manual_seed(3)) * 2000
    return ResidentRegion(s2, s1, boundary, ids, pop, band_sel=BANDS, device="cuda", s1_asc=asc if with_asc else None)


def _plan(region, multi):
    from popcorn_amd.data.region import plan_multi_unit, plan_one_unit
    if multi:
        return plan_multi_unit(region.table, region.census_idx, region.census_pop, region.shape, units_per_crop=2, admin_overlap=4,
                               max_pix_box=6000)
    return plan_one_unit(region.table, region.census_idx, region.census_pop, region.shape, admin_overlap=4)


@pytest.mark.parametrize("ascfill", [False, True])
def test_orbit_column_equals_the_host_path_item_by_item(ascfill):
    """``nanfill.select_s1_host`` on every item's own slices gives the orbit of the column and raises for exactly the dropped items; every
    class of item the other tests rely on is present in this plan."""
    from popcorn_amd.data import nanfill
    from popcorn_amd.data.region import plan_repair
    s2, s1, asc, _ = _host("96x128")
    region = _region("96x128")
    plan = _plan(region, False)
    new, rep = plan_repair(region, plan, seasons=2, ascfill=ascfill)
    assert len(plan) == 12 and sorted(rep.kept + rep.dropped) == list(range(12)) and new == plan.subset(rep.kept)
    s1b, ab = s1[:, list(BANDS[4:])], asc[:, list(BANDS[4:])]
    raised = set()
    for i, c in enumerate(plan.crops.tolist()):
        orbits = []
        for s in range(2):
            desc, a = s1b[s, :, c[0]:c[1], c[2]:c[3]], ab[s, :, c[0]:c[1], c[2]:c[3]]
            try:
                orbits.append({"desc": 0, "asc": 1}[nanfill.select_s1_host(desc, lambda: a, ascfill)[1]])
            except Exception as e:
                assert str(e) == "No data here!"
                raised.add(i)
        if i not in raised:
            assert rep.orbit[rep.kept.index(i)].tolist() == orbits, i
    assert raised == set(rep.dropped) and len(raised) >= 1                             # >= 1 item dropped
    if ascfill:
        return
    assert sorted(plan.census_idx[rep.dropped, 0].tolist()) == [8, 11, 12]             # the units around the ascending corner block
    cnt, orb = rep.counts, rep.orbit
    per = (rep.off[1:] - rep.off[:-1]).reshape(rep.n, 2)
    assert bool(((orb == 0) & (cnt[:, :, 1] > 0)).any())                               # >= 1 item kept descending and filled
    assert bool((orb == 1).any()) and rep.ascending == int((orb == 1).sum())           # >= 1 item switched to ascending
    assert bool(((cnt[:, :, 0] == 0) & (cnt[:, :, 1] == 0)).all(1).any())              # >= 1 NaN-free item
    assert bool(((cnt[:, :, 0] > 0) & (per > 0)).any())                                # >= 1 item with S2 patches
    assert bool(((orb == 1) & (cnt[:, :, 2] > 0) & (per > 0)).any())                   # >= 1 item with (ascending) S1 patches
    chosen = torch.where(orb == 1, cnt[:, :, 2], cnt[:, :, 1])
    assert bool(((per > 0) == ((cnt[:, :, 0] > 0) | (chosen > 0))).all())              # entries exactly where the chosen inputs hold NaN
    assert rep.entries == int(rep.off[-1]) == rep.idx.numel() == rep.val.numel() and rep.entries > 0 and rep.build_ms > 0
    # without the ascending raster: descending at any fraction, nothing dropped, and the item with fewer than 4 known S1 entries is zeroed
    bare = _region("96x128", with_asc=False)
    with pytest.raises(ValueError):
        plan_repair(bare, plan, seasons=2, ascfill=True)
    same, rb = plan_repair(bare, plan, seasons=2)
    assert same == plan and rb.dropped == [] and rb.ascending == 0 and bool((rb.counts[:, :, 2] == 0).all())
    numel = torch.tensor([2 * h * w for h, w in rb.hw])
    known = numel[:, None] - rb.counts[:, :, 1]
    few = torch.nonzero((known > 0) & (known < 4)).tolist()
    assert few == [[8, 0]]                                                              # one item with fewer than 4 (three) known S1 entries
    lo, hi = int(rb.off[8 * 2]), int(rb.off[8 * 2 + 1])
    h9, w9 = rb.hw[8]
    s1_entries = rb.idx[lo:hi] >= 4 * h9 * w9
    assert int(s1_entries.sum()) == 2 * h9 * w9 and bool((rb.val[lo:hi][s1_entries] == 0).all())


# ---- the feeds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("multi", [False, True])
def test_region_feed_with_repair_equals_gather_then_fill(multi):
    from popcorn_amd import ops
    from popcorn_amd.data.region import ResidentRegionFeed, plan_repair
    region = _region("96x128")
    plan, rep = plan_repair(region, _plan(region, multi), seasons=2)
    assert rep.entries > 0 and rep.ascending > 0 and len(plan) >= 4
    B = 2
    feed = ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2, repair=rep)
    bare = ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2)
    state = torch.get_rng_state()
    got = list(feed)
    plain = list(bare)
    assert torch.equal(torch.get_rng_state(), state)                                   # no draw from the global generator
    assert torch.equal(feed.generator.get_state(), bare.generator.get_state()) and torch.equal(feed.last_order, bare.last_order)
    assert len(got) == len(plan) // B
    patched = 0
    for k, (s, p) in enumerate(zip(got, plain)):
        idx = feed.last_order[k * B:(k + 1) * B].tolist()
        sea = feed.last_season[k * B:(k + 1) * B].tolist()
        crops = [plan.crops[i].tolist() + [q] for i, q in zip(idx, sea)]
        orbit = [int(rep.orbit[i, q]) for i, q in zip(idx, sea)]
        assert s["orbit"] == orbit and "orbit" not in p
        tile = ops.region_gather(region.s2, region.s1, region.boundary, BANDS, crops, s1_asc=region.s1_asc, orbit=orbit)
        f2, f1 = _fill(tile)
        assert bit_equal(s["S2"], f2) and bit_equal(s["S1"], f1) and bit_equal(s["admin_mask"], tile["admin_mask"])
        assert not bool(torch.isnan(s["S2"]).any()) and not bool(torch.isnan(s["S1"]).any())
        patched += int(not bit_equal(s["S2"], tile["S2"]) or not bit_equal(s["S1"], tile["S1"]))
        for key in ("y", "census_idx", "data_hw", "season"):
            assert torch.equal(s[key], p[key]), key
        assert s.get("census_n") == p.get("census_n") and s["valid_coords"] == p["valid_coords"]
    assert patched >= 1
    with pytest.raises(ValueError):                                                    # a repair of another plan
        ResidentRegionFeed(region, plan.subset(range(len(plan) - 1)), B, repair=rep)


def _epoch(feed, prepare):
    torch.manual_seed(11)
    random.seed(11)
    out = []
    for sample in feed:
        s = prepare(sample)
        out.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in s.items()})
        torch.rand(1)
    return out, torch.get_rng_state(), random.getstate()


@pytest.mark.parametrize("multi", [False, True])
def test_batch_feed_with_repair_equals_region_feed_then_prepare(multi):
    from popcorn_amd.cli import prepare_sample_fused
    from popcorn_amd.data.region import ResidentBatchFeed, ResidentRegionFeed, plan_repair
    from popcorn_amd.utils.transform import default_train_transform
    region = _region("96x128")
    plan, rep = plan_repair(region, _plan(region, multi), seasons=2)
    transform = default_train_transform()
    B = 2

    def unfused(sample):
        s = prepare_sample_fused(sample, transform)                    # no per-step fill: the repair is in the batch
        s["orbit"] = sample["orbit"]
        if sample.get("census_n") is not None:
            s["census_n"] = sample["census_n"]
        return s

    old = ResidentRegionFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2, repair=rep)
    new = ResidentBatchFeed(region, plan, B, transform=transform, generator=torch.Generator().manual_seed(5), seasons=2, repair=rep)
    want, rng_w, py_w = _epoch(old, unfused)
    got, rng_g, py_g = _epoch(new, lambda s: s)
    assert torch.equal(new.last_order, old.last_order) and torch.equal(new.last_season, old.last_season)
    assert torch.equal(rng_w, rng_g) and py_w == py_g and torch.equal(old.generator.get_state(), new.generator.get_state())
    assert len(got) == len(want) >= 2
    shapes = set()
    for g, w in zip(got, want):
        for key in ("raw", "admin_mask", "y", "census_idx"):
            assert bit_equal(g[key], w[key]), key
        assert g["orbit"] == w["orbit"] and g.get("census_n") == w.get("census_n")
        assert not bool(torch.isnan(g["raw"]).any())
        shapes.add(tuple(g["raw"].shape[2:]))
    assert len(shapes) > 1 and sum(sum(g["orbit"]) for g in got) > 0
    # under a pixel budget: every item once, repaired
    budget = 3 * max(h * w for h, w in rep.hw)
    feed = ResidentBatchFeed(region, plan, B, generator=torch.Generator().manual_seed(5), seasons=2, pixel_budget=budget, max_batch=8,
                             repair=rep)
    batches = list(feed)
    assert sorted(i for b in feed.last_batches for i in b) == list(range(len(plan)))
    assert all(not bool(torch.isnan(s["raw"]).any()) and len(s["orbit"]) == s["raw"].shape[0] for s in batches)


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
BASE = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --resident_region 192 256 --resident_units 24 "
        "--max_steps 3 --save-model no --nan_clouds 0.05")


def _train(tmp_path, name, flags):
    from popcorn_amd.cli import run_train
    t = run_train(BASE.split() + ["--save_dir", str(tmp_path / name)] + flags)
    assert t.info["iter"] == 3
    torch.cuda.synchronize()
    return t, t.fused.loss_out.clone(), t.fused.flat_p.clone()


def test_run_train_resident_repair_equals_nan_fill(tmp_path, capsys):
    """S2 clouds, no S1 gap: the per-step fill and the planned repair give equal bits in the loss and in every parameter after three steps."""
    a, loss_a, p_a = _train(tmp_path, "fill", ["--nan_fill"])
    b, loss_b, p_b = _train(tmp_path, "repair", ["--resident_repair"])
    assert a.region_repair is None and a._step_nan_fill and b.region_repair is not None and not b._step_nan_fill
    assert b.region_repair.entries > 0 and b.region_repair.ascending == 0 and b.region_repair.dropped == []
    assert bool(torch.isnan(b.region.s2).any())
    assert torch.equal(a._resident_feed.last_order, b._resident_feed.last_order)
    assert bool(torch.isfinite(loss_a).all()) and bool(torch.isfinite(p_a).all())
    assert bit_equal(loss_a, loss_b) and bit_equal(p_a, p_b)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("resident repair:")]
    assert len(line) == 1 and all(w in line[0] for w in ("items", "dropped", "ascending", "entries", "bytes", "ms"))


def test_run_train_resident_repair_assembled_equals_unfused(tmp_path):
    from popcorn_amd.data.region import ResidentBatchFeed, ResidentRegionFeed
    gaps = ["--resident_repair", "--resident_s1_gap", "0.1"]
    a, loss_a, p_a = _train(tmp_path, "unfused", gaps)
    b, loss_b, p_b = _train(tmp_path, "assembled", gaps + ["--resident_assemble"])
    assert type(a._resident_feed) is ResidentRegionFeed and type(b._resident_feed) is ResidentBatchFeed
    assert a.region_repair.ascending > 0 and a.region_repair.entries > 0 and bool(torch.isnan(a.region.s1).any())
    assert torch.equal(a.region_repair.orbit, b.region_repair.orbit) and torch.equal(a.region_repair.idx, b.region_repair.idx)
    assert bool(torch.isfinite(loss_a).all()) and bool(torch.isfinite(p_a).all())
    assert bit_equal(loss_a, loss_b) and bit_equal(p_a, p_b)


def test_run_train_resident_repair_pixel_budget_and_refusals(tmp_path):
    from popcorn_amd import cli
    t, loss, p = _train(tmp_path, "budget", ["--resident_repair", "--resident_s1_gap", "0.1", "--resident_pixel_budget", "60000"])
    assert t._resident_feed.pixel_budget == 60000 and t._resident_feed.repair is t.region_repair
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(p).all())
    base = f"-S2 -NIR -S1 -occmodel -senbuilds -pret --save-model no --save_dir {tmp_path}".split()
    with pytest.raises(SystemExit) as e:                               # without the new flag: today's words
        cli.run_train(base + "--resident_region 192 256 --resident_units 24 --resident_assemble --nan_fill".split())
    assert "cannot be combined with --nan_fill" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.run_train(base + ["--resident_repair"])
    assert "--resident_region" in str(e.value)
