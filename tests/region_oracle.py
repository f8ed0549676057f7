"""The reference's region bookkeeping and weaksup items restated in the project's own words (plain torch on the host), for the tests of
csrc/region.hip and popcorn_amd/data/region.py.

  unit_table      utils/02_preprocess_rwa_shapefile.py:142-161: per census unit, the rows / columns that hold any of its pixels
                  (torch.where(torch.any(mask, dim))), first and last + 1 of each, the pixel count; zeros for a unit without pixels
  one_unit_rule   data/PopulationDataset.py:124-131 (the two size filters) and :644-649 (the crop: the bounding box grown by admin_overlap,
                  clipped to the raster), as a loop over the census rows
  weaksup_item    data/PopulationDataset.py:403-458, :566-568, :594-604: the selected bands of the window as fp32, the boundary window as
                  fp32, y, census_idx, img_coords, valid_coords, season
  host_batch      the items through the existing collates (``Population_Dataset_collate_fn`` / ``collate_units``)
and the two test rasters of tests/test_region_cpu.py."""
import torch

from popcorn_amd.data.collate import Population_Dataset_collate_fn
from popcorn_amd.data.units import collate_units


def unit_table(boundary, num_ids):
    """(table int32 (num_ids, 5) = {xmin, xmax, ymin, ymax, count}, stray): x indexes rows, y columns, maxima exclusive."""
    b = boundary.cpu()
    table = torch.zeros(num_ids, 5, dtype=torch.int32)
    for i in range(num_ids):
        mask = b == i
        count = int(mask.sum())
        if count == 0:
            continue
        vertical = torch.where(torch.any(mask, dim=1))[0]
        horizontal = torch.where(torch.any(mask, dim=0))[0]
        table[i] = torch.tensor([int(vertical[0]), int(vertical[-1]) + 1, int(horizontal[0]), int(horizontal[-1]) + 1, count])
    stray = int(((b < 0) | (b >= num_ids)).sum())
    return table, stray


def one_unit_rule(table, census_idx, census_pop, shape, admin_overlap, max_pix, max_pix_box):
    """[(idx, pop, (xmin, xmax, ymin, ymax), (x0, x1, y0, y1))] in census order: the rows the reference keeps and the window it reads; rows
    without pixels left out (the project's stated deviation)."""
    rows = [(int(i), float(p), [int(v) for v in table[int(i)]]) for i, p in zip(census_idx, census_pop)]
    rows = [r for r in rows if r[2][4] < max_pix]
    rows = [r for r in rows if (r[2][1] - r[2][0]) * (r[2][3] - r[2][2]) < max_pix_box]
    out = []
    for idx, pop, (xmin, xmax, ymin, ymax, count) in rows:
        if count == 0:
            continue
        px, py = xmax - xmin, ymax - ymin
        window = (max(xmin - admin_overlap, 0), min(xmin + px + admin_overlap, shape[0]),
                  max(ymin - admin_overlap, 0), min(ymin + py + admin_overlap, shape[1]))
        out.append((idx, pop, (xmin, xmax, ymin, ymax), window))
    return out


def weaksup_item(s2, s1, boundary, band_sel, crop, season, y, census_idx, bbox):
    """One item: host tensors.  s2 (S, C2, h, w) fp32 or uint16, s1 (S, C1, h, w), boundary int32 (h, w); crop = (x0, x1, y0, y1);
    y / census_idx: a scalar and one id (one-unit item) or K of each (multi-unit item)."""
    x0, x1, y0, y1 = (int(v) for v in crop)
    sel2, sel1 = [int(v) for v in band_sel[:4]], [int(v) for v in band_sel[4:]]
    win2 = torch.stack([s2[season, c, x0:x1, y0:y1] for c in sel2]).float()
    win1 = torch.stack([s1[season, c, x0:x1, y0:y1] for c in sel1]).float()
    ids = torch.as_tensor(census_idx, dtype=torch.int64).reshape(-1)
    yy = torch.as_tensor(y, dtype=torch.float32).reshape(-1)
    return {"S2": win2, "S1": win1, "admin_mask": boundary[x0:x1, y0:y1].float(), "y": yy[0] if yy.numel() == 1 else yy,
            "census_idx": ids, "img_coords": (int(bbox[0]), int(bbox[2])), "valid_coords": tuple(int(v) for v in bbox),
            "season": int(season)}


def host_batch(items, multi):
    return collate_units(items) if multi else Population_Dataset_collate_fn(items)


def plan_items(s2, s1, boundary, band_sel, plan, indices, seasons):
    """The items of plan rows ``indices`` (with their seasons) as the host would cut them."""
    out = []
    for i, s in zip(indices, seasons):
        n = plan.census_n[i]
        out.append(weaksup_item(s2, s1, boundary, band_sel, plan.crops[i].tolist(), int(s), plan.y[i, :n], plan.census_idx[i, :n],
                                plan.bbox[i].tolist()))
    return out


# ---- test rasters -------------------------------------------------------------------------------------------------------------------
def blocky_raster(h=96, w=128, gy=3, gx=4):
    """ids 1 .. gy * gx in equal blocks: every edge of the raster is touched by some unit."""
    ys = (torch.arange(h) * gy) // h
    xs = (torch.arange(w) * gx) // w
    return (ys[:, None] * gx + xs[None, :] + 1).to(torch.int32)


def irregular_raster(h=120, w=150, units=24, seed=5):
    """A nearest-seed tiling (unequal metrics, as SyntheticMultiUnitDataset._make) of ids 1 .. units; pixels far from every seed are the
    background 0.  The units' bounding boxes overlap each other."""
    g = torch.Generator().manual_seed(seed)
    sy, sx = torch.rand(units, generator=g) * h, torch.rand(units, generator=g) * w
    wgt = 0.75 + 0.5 * torch.rand(units, generator=g)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    d = ((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2) * wgt[:, None, None]
    best, owner = d.min(0)
    ids = owner + 1
    ids[best > 24.0 ** 2] = 0
    return ids.to(torch.int32)
