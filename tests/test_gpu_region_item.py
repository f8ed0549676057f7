"""pc_region_item (csrc/region_crop.hip, ops.region_item): the normalised model input and the admin mask of ONE rectangular crop of the
resident rasters in one launch, against the composition of the existing ops it replaces, fp32 compared as integers:

    out       == select_normalize(cat(S2, S1 of patch_apply(region_gather({crop}, orbit))), 0 .. 5, mean6, std6)
                 on every non-NaN element, NaN at exactly the same sites
    admin_out == admin_mask of that gather

Outputs sit between guard bands in poisoned memory (tests/footprint.py): an element nobody stores stays NaN, a store outside an output
damages a band."""
import ctypes as C

import pytest
import torch

from tests.footprint import POISON, Footprint, bit_equal

pytestmark = pytest.mark.gpu

H, W, SEASONS = 37, 53, 2
DUP_BANDS = (2, 0, 2, 4, 1, 0)             # S2 band 2 twice, out of 5; S1 bands out of 3
MODEL_BANDS = (0, 1, 2, 3, 0, 1)
WIDE_H, WIDE_W = 3, 9001                   # wider than two workgroup ranges per row: the crop region_window (square, capped) cannot take
NAN = float("nan")
_CACHE = {}


def _stats():
    from popcorn_amd.data import stats
    return stats.MEAN6, stats.STD6


def _payload_nan(bits):
    return torch.tensor([bits], dtype=torch.int32).view(torch.float32)[0]


def _sources(kind):
    """(s2 (2, 5, 37, 53) fp32 or uint16, s1 (2, 3, 37, 53), s1_asc likewise, boundary) on the device; NaNs -- with payloads in S1 -- at
    stated coordinates."""
    if kind not in _CACHE:
        g = torch.Generator().manual_seed(14)
        s2 = torch.randint(0, 10000, (SEASONS, 5, H, W), generator=g).float()
        s1 = torch.randn(SEASONS, 3, H, W, generator=g) * 4 - 12
        asc = torch.randn(SEASONS, 3, H, W, generator=g) * 4 - 12
        if kind == "f32":
            s2[0, 2, 0, 0] = NAN; s2[0, 2, 1, 3] = NAN; s2[1, 0, H - 1, W - 1] = NAN; s2[0, 4, 10:14, 20:31] = NAN; s2[1, 2, 33, :] = NAN
        s1[0, 1, 0, 0] = _payload_nan(0x7FC12345); s1[0, 0, 2, 5] = _payload_nan(-0x3F0001)      # (0xFFC0FFFF: sign bit set)
        s1[1, 1, H - 1, W - 1] = _payload_nan(0x7FA00001); s1[0, 0, 20:23, :] = NAN; s1[1, 0, :, 7] = _payload_nan(0x7FC00077)
        asc[0, 0, 0, 1] = _payload_nan(0x7FC0BEEF); asc[1, 1, H - 2, W - 1] = NAN; asc[0, 1, 16, 30:50] = NAN
        if kind == "u16":
            s2 = s2.to(torch.int32).to(torch.uint16)
        boundary = ((torch.arange(H * W, dtype=torch.int32).reshape(H, W) * 37) % 1009)
        _CACHE[kind] = tuple(t.cuda() for t in (s2, s1, asc, boundary))
    return _CACHE[kind]


def _wide(kind):
    if ("wide", kind) not in _CACHE:
        g = torch.Generator().manual_seed(15)
        s2 = torch.randint(0, 10000, (1, 4, WIDE_H, WIDE_W), generator=g).float()
        s1 = torch.randn(1, 2, WIDE_H, WIDE_W, generator=g) * 4 - 12
        asc = torch.randn(1, 2, WIDE_H, WIDE_W, generator=g) * 4 - 12
        s1[0, 1, 1, 4000:4200] = NAN
        if kind == "f32":
            s2[0, 3, 2, 8990:] = NAN
        else:
            s2 = s2.to(torch.int32).to(torch.uint16)
        boundary = torch.arange(WIDE_H * WIDE_W, dtype=torch.int32).reshape(WIDE_H, WIDE_W) % 911
        _CACHE[("wide", kind)] = tuple(t.cuda() for t in (s2, s1, asc, boundary))
    return _CACHE[("wide", kind)]


def _compose(s2, s1, asc, boundary, bands, crop, orbit, entries=None):
    """The right-hand side: gather with the orbit, the patches laid over it, concatenation, normalisation; and the gather's admin mask."""
    from popcorn_amd import ops
    mean6, std6 = _stats()
    t = ops.region_gather(s2, s1, boundary, bands, [crop], s1_asc=asc, orbit=[orbit])
    if entries is not None:
        idx, val = entries
        hc, wc = crop[1] - crop[0], crop[3] - crop[2]
        assert ops.region_patch_apply(idx, val, [0], [idx.numel()], [(hc, wc)], t["S2"], t["S1"], (hc, wc)) == idx.numel()
    return ops.select_normalize(torch.cat([t["S2"], t["S1"]], 1).contiguous(), tuple(range(6)), mean6, std6), t["admin_mask"]


def _same_where_not_nan(got, want):
    gn, wn = torch.isnan(got), torch.isnan(want)
    return got.shape == want.shape and bool(torch.equal(gn, wn)) and bool((got.view(torch.int32)[~gn] == want.view(torch.int32)[~wn]).all())


def _check(src, bands, crop, orbit, table=None, entries=None):
    """One crop through the kernel into poisoned, guarded outputs -- and into its own allocations -- against the composition."""
    from popcorn_amd import ops
    s2, s1, asc, boundary = src
    mean6, std6 = _stats()
    hc, wc = crop[1] - crop[0], crop[3] - crop[2]
    want, want_admin = _compose(s2, s1, asc, boundary, bands, crop, orbit, entries)
    with Footprint("cuda", fill=POISON) as fp:
        out = fp.alloc((1, 6, hc, wc), torch.float32)
        admin = fp.alloc((1, hc, wc), torch.float32)
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(admin).all())
        got, got_admin = ops.region_item(s2, s1, boundary, bands, crop, mean6, std6, out=out, admin_out=admin, s1_asc=asc, orbit=orbit,
                                         table=table)
        fresh, fresh_admin = ops.region_item(s2, s1, boundary, bands, crop, mean6, std6, s1_asc=asc, orbit=orbit, table=table)
    assert got is out and got_admin is admin
    assert _same_where_not_nan(got, want), ("input", crop, orbit)
    assert bit_equal(got_admin, want_admin) and not bool(torch.isnan(got_admin).any()), ("admin_mask", crop, orbit)
    assert tuple(fresh.shape) == (1, 6, hc, wc) and tuple(fresh_admin.shape) == (1, hc, wc)
    assert _same_where_not_nan(fresh, want) and bit_equal(fresh_admin, want_admin)
    # 4-byte aligned outputs only: the element-by-element path at any width
    sh_out = torch.full((6 * hc * wc + 1,), 123.0, device="cuda")[1:].view(1, 6, hc, wc)
    sh_admin = torch.full((hc * wc + 1,), 123.0, device="cuda")[1:].view(1, hc, wc)
    ops.region_item(s2, s1, boundary, bands, crop, mean6, std6, out=sh_out, admin_out=sh_admin, s1_asc=asc, orbit=orbit, table=table)
    assert _same_where_not_nan(sh_out, want) and bit_equal(sh_admin, want_admin), ("unaligned outputs", crop, orbit)
    return want


CROPS = {
    "odd_y0_wc31": (3, 20, 5, 36),
    "odd_y0_wc28": (2, 30, 7, 35),
    "corner_top_left": (0, 10, 0, 12),
    "corner_top_right": (0, 10, W - 12, W),
    "corner_bottom_left": (H - 10, H, 0, 12),
    "corner_bottom_right": (H - 9, H, W - 13, W),
    "whole_raster": (0, H, 0, W),
    "one_pixel": (17, 18, 23, 24),
    "nan_pixel": (0, 1, 0, 1),
}


@pytest.mark.parametrize("name", list(CROPS))
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_item_without_table_equals_gather_then_normalize(kind, name):
    src = _sources(kind)
    nans = 0
    for season in range(SEASONS):
        for orbit in (0, 1):
            want = _check(src, DUP_BANDS, CROPS[name] + (season,), orbit)
            nans += int(torch.isnan(want).sum())
    if name in ("whole_raster", "nan_pixel", "odd_y0_wc31", "odd_y0_wc28"):
        assert nans > 0                                                  # the NaN sites were part of the comparison


def test_item_without_orbit_arguments_reads_the_descending_raster():
    from popcorn_amd import ops
    s2, s1, asc, boundary = _sources("f32")
    mean6, std6 = _stats()
    crop = CROPS["odd_y0_wc28"] + (1,)
    want, want_admin = _compose(s2, s1, asc, boundary, DUP_BANDS, crop, 0)
    got, got_admin = ops.region_item(s2, s1, boundary, DUP_BANDS, crop, mean6, std6)
    assert _same_where_not_nan(got, want) and bit_equal(got_admin, want_admin)
    flat = torch.full((6, 28, 28), 5.0, device="cuda")                  # the (6, hc, wc) / (hc, wc) forms of the outputs
    flat_admin = torch.full((28, 28), 5.0, device="cuda")
    a, b = ops.region_item(s2, s1, boundary, DUP_BANDS, crop, mean6, std6, out=flat, admin_out=flat_admin)
    assert tuple(a.shape) == (1, 6, 28, 28) and tuple(b.shape) == (1, 28, 28) and a.data_ptr() == flat.data_ptr()
    assert _same_where_not_nan(a, want) and bit_equal(b, want_admin)


@pytest.mark.parametrize("y0", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_wide_crop_spans_workgroup_ranges_that_end_inside_a_row(kind, y0):
    """3 x 9,001 at full width (element by element) and 3 x 9,000 from column 1 (16-byte accesses at an odd origin): seven ranges of
    4,096 elements per plane, none of which ends on a row boundary."""
    from popcorn_amd import _lib as L
    plane = WIDE_H * (WIDE_W - y0)
    assert plane > 6 * L.PC_REGION_ITEM_TILE and (WIDE_W - y0) % L.PC_REGION_ITEM_TILE != 0 and ((WIDE_W - y0) % 4 == 0) == (y0 == 1)
    for orbit in (0, 1):
        want = _check(_wide(kind), MODEL_BANDS, (0, WIDE_H, y0, WIDE_W, 0), orbit)
        assert int(torch.isnan(want).sum()) > 0 or orbit == 1 and kind == "u16"


@pytest.mark.parametrize("y0", [0, 1])
def test_hand_made_table_at_range_and_channel_boundaries(y0):
    """Entries at the first and the last element of a workgroup's range, on both sides of a channel boundary and in the last element of
    channel 5; one stray entry beyond the item's space, inside the slice, is ignored.  The slice sits inside a longer table whose other
    entries would damage the item if they were read."""
    from popcorn_amd import _lib as L
    src = _wide("f32")
    wc = WIDE_W - y0
    plane, T = WIDE_H * wc, L.PC_REGION_ITEM_TILE
    sites = [0, T - 1, T, 3 * T - 1, 3 * T, plane - 1, plane, 4 * plane + T, 5 * plane + 6 * T, 6 * plane - 1]
    assert sites == sorted(sites) and 6 * T < plane < 7 * T
    idx = torch.tensor(sites, dtype=torch.int32, device="cuda")
    val = torch.arange(len(sites), dtype=torch.float32, device="cuda") * 17.0 + 1000.0
    stray = torch.tensor([6 * plane + 5], dtype=torch.int32, device="cuda")
    junk_i = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
    junk_v = torch.full((2,), 1e30, device="cuda")
    tab_i = torch.cat([junk_i, idx, stray, junk_i])
    tab_v = torch.cat([junk_v, val, torch.full((1,), -1e30, device="cuda"), junk_v])
    crop = (0, WIDE_H, y0, WIDE_W, 0)
    want = _check(src, MODEL_BANDS, crop, 1, table=(tab_i, tab_v, 2, len(sites) + 1), entries=(idx, val))
    plain, _ = _compose(*src, MODEL_BANDS, crop, 1)
    changed = (want.view(torch.int32) != plain.view(torch.int32)).reshape(-1).nonzero().reshape(-1).tolist()
    assert changed == sites                                              # the composition itself moved exactly the listed sites


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("orbit", [0, 1])
@pytest.mark.parametrize("ps", [32, 33, 36])
@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_a_window_is_a_square_item_bit_for_bit(kind, ps, orbit, with_table):
    """``region_window`` and ``region_item`` are two launches of one kernel: a window of side ps is the item [x, x + ps) x [y, y + ps)
    whose workgroup ranges are blocks of ``region_window_rows(ps)`` whole rows.  ps = 32: 16-byte accesses; 33: element by element; 36:
    16-byte accesses and a short last range (R = 16 < ps).  The origin is odd (source rows are not 16-byte aligned), the season is 1.  The
    hand-made table has entries at the first and the last site of channel 0, on both sides of a boundary between two of the window's
    ranges and at the first site of channel 4, inside a longer table whose other entries would damage the output if they were read."""
    from popcorn_amd import ops
    s2, s1, asc, boundary = _sources(kind)
    mean6, std6 = _stats()
    x, y, season = 1, 5, 1
    plane, T = ps * ps, ops.region_window_rows(ps) * ps
    assert x + ps <= H and y + ps <= W and 0 < T < plane and (ps % 4 == 0) == (ps != 33) and (plane % T != 0) == (ps != 32)
    table = None
    if with_table:
        sites = [0, T - 1, T, plane - 1, 4 * plane]
        assert sites == sorted(set(sites))
        idx = torch.tensor(sites, dtype=torch.int32, device="cuda")
        val = torch.arange(len(sites), dtype=torch.float32, device="cuda") * 17.0 + 1000.5      # (no S2 digital number has a fraction)
        stray = torch.tensor([6 * plane + 5], dtype=torch.int32, device="cuda")
        junk_i = torch.tensor([0, 5], dtype=torch.int32, device="cuda")
        junk_v = torch.full((2,), 1e30, device="cuda")
        table = (torch.cat([junk_i, idx, stray, junk_i]), torch.cat([junk_v, val, torch.full((1,), -1e30, device="cuda"), junk_v]), 2,
                 len(sites) + 1)
    win = torch.full((1, 6, ps, ps), NAN, device="cuda")
    item = torch.full((1, 6, ps, ps), NAN, device="cuda")
    admin = torch.full((1, ps, ps), NAN, device="cuda")
    ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6, out=win, s1_asc=asc, orbit=orbit, table=table)
    ops.region_item(s2, s1, boundary, DUP_BANDS, (x, x + ps, y, y + ps, season), mean6, std6, out=item, admin_out=admin, s1_asc=asc,
                    orbit=orbit, table=table)
    assert torch.equal(win.view(torch.int32), item.view(torch.int32)), (kind, ps, orbit, with_table)
    assert not bool(torch.isnan(admin).any())
    if with_table:
        plain = ops.region_window(s2, s1, DUP_BANDS, (x, y, season), ps, mean6, std6, s1_asc=asc, orbit=orbit)
        changed = (win.view(torch.int32) != plain.view(torch.int32)).reshape(-1).nonzero().reshape(-1).tolist()
        assert changed == sites                                          # the table moved exactly the listed sites


def test_refusals_enqueue_nothing():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    s2, s1, asc, boundary = _sources("f32")
    mean6, std6 = _stats()
    crop = (1, 21, 3, 35, 0)
    hc, wc = 20, 32
    out = torch.full((1, 6, hc, wc), 7.0, device="cuda")
    admin = torch.full((1, hc, wc), -3.0, device="cuda")               # (ids are non-negative: no admin value equals the fill)
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    val = torch.ones(4, device="cuda")

    def untouched(kw):
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((admin == -3.0).all()), kw

    ok = dict(s2=s2, s1=s1, boundary=boundary, band_sel=DUP_BANDS, crop=crop, mean6=mean6, std6=std6, out=out, admin_out=admin, s1_asc=asc,
              orbit=1, table=(idx, val, 0, 4))
    bad = [dict(crop=(5, 5, 3, 35, 0)), dict(crop=(1, 21, 9, 9, 0)), dict(crop=(1, H + 1, 3, 35, 0)), dict(crop=(1, 21, 3, W + 1, 0)),
           dict(crop=(-1, 19, 3, 35, 0)), dict(crop=(1, 21, -1, 31, 0)), dict(crop=(1, 21, 3, 35, SEASONS)), dict(crop=(1, 21, 3, 35, -1)),
           dict(crop=(1, 21, 3, 35)), dict(band_sel=(5, 0, 2, 4, 1, 0)), dict(band_sel=(2, 0, 2, 4, 3, 0)), dict(band_sel=(2, 0, 2, 4, 1)),
           dict(s1_asc=None), dict(orbit=2), dict(orbit=-1), dict(s1_asc=asc[:1].contiguous()), dict(boundary=boundary.long()),
           dict(table=(None, None, 0, 4)), dict(table=(idx, None, 0, 4)), dict(table=(idx, val, 2, 3)), dict(table=(idx, val, -1, 2)),
           dict(table=(idx, val, 0, -1)), dict(table=(idx.long(), val, 0, 4)), dict(table=(idx.cpu(), val.cpu(), 0, 4)),
           dict(out=torch.full((1, 6, hc, wc + 1), 7.0, device="cuda")), dict(out=out.double()), dict(admin_out=admin.double()),
           dict(admin_out=torch.full((1, hc + 1, wc), -3.0, device="cuda")), dict(mean6=mean6[:5]), dict(s2=s2[:, :, :, ::2]),
           dict(s1=s1[:1].contiguous()), dict(s2=s2.half())]
    for kw in bad:
        with pytest.raises((ValueError, L.PopcornHipError)) as e:
            ops.region_item(**{**ok, **kw})
        assert e.type is ValueError or "cpu" in str(e.value), kw
        untouched(kw)

    # the library's own checks: PC_EINVAL with nothing enqueued -- both outputs keep their fill
    def p(t, off=0):
        return C.c_void_p(0 if t is None else t.data_ptr() + off)

    def call(s2_=p(s2), s1_=p(s1), asc_=p(asc), orbit=1, bnd_=p(boundary), h=H, w=W, bands=DUP_BANDS, x0=1, x1=21, y0=3, y1=35, season=0,
             mean_=True, std_=True, idx_=p(idx), val_=p(val), cap=4, start=0, count=4, out_=p(out), admin_=p(admin)):
        return L.lib().pc_region_item(s2_, 0, s1_, asc_, orbit, bnd_, SEASONS, 5, 3, h, w, (C.c_int32 * 6)(*bands) if bands else None, x0,
                                      x1, y0, y1, season, (C.c_float * 6)(*mean6) if mean_ else None,
                                      (C.c_float * 6)(*std6) if std_ else None, idx_, val_, C.c_int64(cap), C.c_int64(start),
                                      C.c_int64(count), out_, admin_, L.stream_ptr())

    cases = [
        # a NULL pointer
        dict(s2_=p(None)), dict(s1_=p(None)), dict(bnd_=p(None)), dict(bands=None), dict(mean_=False), dict(std_=False), dict(out_=p(None)),
        dict(admin_=p(None)),
        # an empty crop, a crop that leaves the raster
        dict(x1=1), dict(y1=3), dict(x1=0), dict(x1=H + 1), dict(y1=W + 1), dict(x0=-1), dict(y0=-1),
        # 6 * hc * wc >= 2^31 (a raster of 20,000 x 20,000 is claimed; the refusal comes before anything is read)
        dict(h=20000, w=20000, x0=0, x1=20000, y0=0, y1=20000),
        # a season outside [0, S), a band outside its source
        dict(season=SEASONS), dict(season=-1), dict(bands=(5, 0, 2, 4, 1, 0)), dict(bands=(2, 0, 2, 4, 1, 3)), dict(bands=(2, 0, -1, 4, 1, 0)),
        # an orbit outside {0, 1}, orbit 1 without s1_asc
        dict(orbit=2), dict(orbit=-1), dict(asc_=p(None)),
        # count > 0 without tables
        dict(idx_=p(None)), dict(val_=p(None)),
        # a slice outside [0, cap] or longer than 6 * hc * wc
        dict(start=1), dict(cap=3), dict(count=-1), dict(start=-1, count=1), dict(cap=-1),
        dict(count=6 * hc * wc + 1, cap=1 << 20), dict(start=1 << 62, cap=1 << 20),
        # misaligned pointers
        dict(s2_=p(s2, 2)), dict(s1_=p(s1, 2)), dict(asc_=p(asc, 1)), dict(bnd_=p(boundary, 2)), dict(out_=p(out, 2)), dict(admin_=p(admin, 1)),
        dict(idx_=p(idx, 2)), dict(val_=p(val, 2)),
    ]
    for kw in cases:
        assert call(**kw) == L.PC_EINVAL, kw
        untouched(kw)
    assert call() == 0 and call(asc_=p(None), orbit=0, idx_=p(None), val_=p(None), cap=0, count=0) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any()) and not bool((admin == -3.0).any())
