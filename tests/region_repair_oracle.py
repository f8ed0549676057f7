"""Plain-torch statements of what the resident repair (popcorn_amd/data/region.py: plan_repair; csrc/region_repair.hip) has to compute, and
the inputs its tests share.  Nothing here calls the library.

  ``orbit_rule``       data/PopulationDataset.py:423-441, restated operation by operation on NaN counts
  ``patch_position``   where tile position (i, j) of a gathered (Hm, Wm) tile lands under vflip, then hflip, then ``rot`` quarter turns
  ``census``           torch.isnan(slice[bands]).sum() of a box
  ``patch_entries``    torch.nonzero of the bit difference of a gathered item and its filled copy, in the table's index space
  ``sources``          rasters of 37 x 53 and 96 x 128 (two seasons, five S2 and three S1 bands) with NaNs at STATED coordinates"""
import torch

MAX_NAN_FRACTION = 0.05


class NoData(Exception):
    pass


def orbit_rule(n_desc, n_asc, numel, ascfill, has_asc=True):
    """(orbit, filled?) of an item whose descending S1 holds n_desc NaNs among numel entries and whose ascending S1 holds n_asc; raises
    NoData where the reference raises "No data here!".  has_asc False: the project's resident feed without an ascending raster keeps the
    descending orbit and fills it at any fraction."""
    if n_desc == 0:                                                                   # :424 np.any(np.isnan(S1)) is False
        return 0, False
    if not has_asc:
        return 0, True
    if bool(torch.tensor(n_desc) / numel < MAX_NAN_FRACTION) and not ascfill:        # :428, a float32 quotient
        return 0, True
    if bool(torch.tensor(n_asc) / numel < MAX_NAN_FRACTION):                         # :436
        return 1, n_asc > 0
    raise NoData("No data here!")                                                     # :441


def patch_position(i, j, Hm, Wm, vflip, hflip, rot):
    """Output position (i', j') of tile position (i, j): out = rot90^rot(hflip(vflip(T))), stated forwards, one step at a time."""
    H, W = Hm, Wm
    if vflip:
        i = H - 1 - i
    if hflip:
        j = W - 1 - j
    for _ in range(rot & 3):                                                          # torch.rot90(k=1): out[a][b] = in[b][W - 1 - a]
        i, j = W - 1 - j, i
        H, W = W, H
    return i, j


def transform_tile(t, vflip, hflip, rot):
    """The same transform on a (.., H, W) tensor with torch's own ops (what utils/transform.py applies)."""
    if vflip:
        t = torch.flip(t, [-2])
    if hflip:
        t = torch.flip(t, [-1])
    return torch.rot90(t, rot & 3, [-2, -1])


def census(s2, s1, s1_asc, bands, box):
    """[NaN entries of S2 over bands[:4], of s1 over bands[4:], of s1_asc likewise] of box = (x0, x1, y0, y1, season); host tensors."""
    x0, x1, y0, y1, s = box
    out = [0, 0, 0]
    if s2.dtype == torch.float32:
        out[0] = int(torch.isnan(s2[s, list(bands[:4]), x0:x1, y0:y1]).sum())
    out[1] = int(torch.isnan(s1[s, list(bands[4:]), x0:x1, y0:y1]).sum())
    if s1_asc is not None:
        out[2] = int(torch.isnan(s1_asc[s, list(bands[4:]), x0:x1, y0:y1]).sum())
    return out


def patch_entries(g2, g1, f2, f1, hb, wb):
    """(idx int64, val fp32) of ONE item: gathered (4, Hm, Wm) / (2, Hm, Wm) and filled copies, extent (hb, wb); ascending idx =
    (c * hb + i) * wb + j over the entries whose 32-bit pattern differs, with the filled bits."""
    g = torch.cat([g2[:, :hb, :wb], g1[:, :hb, :wb]]).contiguous()
    f = torch.cat([f2[:, :hb, :wb], f1[:, :hb, :wb]]).contiguous()
    diff = (g.view(torch.int32) != f.view(torch.int32)).reshape(-1)
    idx = torch.nonzero(diff).reshape(-1)
    return idx, f.reshape(-1)[idx]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
S, C2, C1 = 2, 5, 3
BANDS = (4, 0, 2, 1, 2, 0)                                          # not the identity
DUP_BANDS = (4, 4, 2, 1, 0, 0)                                      # a band listed twice counts twice
RASTERS = {"37x53": (37, 53), "96x128": (96, 128)}
NAN = float("nan")


def sources(name, kind="f32"):
    """(s2, s1, s1_asc) on the host.  Every NaN sits at a stated place:
    37x53   S2 season 0, source band 4 (output channel 0): rows 2..8, columns 3..16; season 1 all S2 bands: rows 30..36, columns 40..52
            descending S1 season 0, all bands: rows 10, 11 (whole width); season 1, source band 2: row 0, columns 0..4
            ascending S1 season 0, source band 0: rows 20..24, columns 0..9
    96x128  S2 season 0 all bands: rows 40..55, columns 50..89; descending S1 both seasons: row 0, columns 0..59 (a thin gap) and rows
            60..95 (a wide one) -- of which season 0, source band 2, row 95, columns 0..2 are known again: three known entries in the crop
            of the bottom-left unit; ascending S1 season 0: rows 64..95, columns 96..127 all bands (one corner block: the units around
            it have no data); ascending S1 season 1, source band 0: rows 70, 71, columns 0..31"""
    h, w = RASTERS[name]
    g = torch.Generator().manual_seed(31)
    s2 = torch.randint(0, 10000, (S, C2, h, w), generator=g)
    s2 = s2.to(torch.uint16) if kind == "u16" else s2.float()
    s1 = torch.randn(S, C1, h, w, generator=g) * 5 - 12
    asc = torch.randn(S, C1, h, w, generator=g) * 5 - 12
    if name == "37x53":
        if kind == "f32":
            s2[0, 4, 2:9, 3:17] = NAN
            s2[1, :, 30:37, 40:53] = NAN
        s1[0, :, 10:12, :] = NAN
        s1[1, 2, 0, 0:5] = NAN
        asc[0, 0, 20:25, 0:10] = NAN
    else:
        if kind == "f32":
            s2[0, :, 40:56, 50:90] = NAN
        s1[:, :, 0, 0:60] = NAN
        s1[:, :, 60:96, :] = NAN
        s1[0, 2, 95, 0:3] = -7.0
        asc[0, :, 64:96, 96:128] = NAN
        asc[1, 0, 70:72, 0:32] = NAN
    return s2, s1, asc
