"""Synthetic stand-in for the reference's ``Population_Dataset`` (data/PopulationDataset.py:30-37), shaped like its
two modes, for environments without the GeoTIFF archive (no rasterio / no data here):

  * mode="weaksup": one census region per item -- a variable-size crop with S2 (4,h,w) raw reflectances, S1 (2,h,w)
    backscatter in dB, ``admin_mask`` (h,w) of region ids, the census count ``y`` and ``census_idx`` (:425-470);
  * mode="test": a raster (seasons, 6, H, W) walked with 2048-px windows (:336-420) plus a census table / boundary map
    in the on-disk format written by utils/02_preprocess_rwa_shapefile.py:142-164 (idx, POP20, bbox, count).
"""
from __future__ import annotations

import torch
from torch.utils.data import Dataset

from . import stats


def cloud_mask(h, w, fraction, g):
    """Seeded cloud discs (radii 4 - 40 px) over an h x w raster until about ``fraction`` of it is covered (a bool (h, w) mask)."""
    m = torch.zeros(h, w, dtype=torch.bool)
    if fraction <= 0:
        return m
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    target = fraction * h * w
    for _ in range(10000):
        if m.sum() >= target:
            break
        cy, cx = torch.rand(2, generator=g) * torch.tensor([h, w])
        r = 4 + torch.rand(1, generator=g).item() * min(36.0, max(h, w) / 4)
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
    return m


def gap_rows(h, fraction, g):
    """Seeded orbit-gap stripes: a bool (h,) mask of about ``fraction`` of the rows, in up to three bands."""
    m = torch.zeros(h, dtype=torch.bool)
    n = int(round(fraction * h))
    if n <= 0:
        return m
    bands = min(3, n)
    for k in range(bands):
        ln = n // bands + (1 if k < n % bands else 0)
        r0 = int(torch.randint(0, max(1, h - ln + 1), (1,), generator=g))
        m[r0:r0 + ln] = True
    return m


def building_layer(h, w, g):
    """A synthetic building layer as a dataset ships it (Google Open Buildings / swissTLM3D counts; data/PopulationDataset.py:606-612): fp32
    (h, w), whole-numbered counts 0 .. 12, exactly 0.0 on about 70 % of the pixels so that the occupancy model's ``building_counts > 0``
    mask matters.  Drawn from ``g`` alone."""
    counts = torch.randint(1, 13, (h, w), generator=g).float()
    built = torch.rand(h, w, generator=g) < 0.3
    return torch.where(built, counts, torch.zeros(()))


class SyntheticWeaksupDataset(Dataset):
    def __init__(self, n_regions=256, min_hw=64, max_hw=144, seed=1600, fixed_hw=None, nan_clouds=0.0, ascfill=False, buildings=False):
        """nan_clouds > 0 (opt-in): real-raster NaNs -- cloud discs over about that fraction of every item's S2 (all bands), orbit-gap rows in
        its descending S1 (every third item over 5 % of the rows) and a NaN-free ascending S1; the item carries the S1 of the orbit the
        reference's rule picks (data.nanfill.select_s1_host; ``ascfill``: always the ascending one where the descending has a gap).  The
        NaN-free data underneath is the same as with nan_clouds = 0.  The fill runs on the device (Trainer ``--nan_fill``).
        buildings (opt-in): every item carries ``building_counts`` (1, h, w), a ``building_layer`` from a generator of its own -- every
        other tensor of the item keeps its bits."""
        self.nan_clouds, self.ascfill, self.buildings = float(nan_clouds), bool(ascfill), bool(buildings)
        self.n = n_regions
        g = torch.Generator().manual_seed(seed)
        if fixed_hw is not None:
            self.hw = [tuple(fixed_hw)] * n_regions
        else:
            hw = torch.randint(min_hw, max_hw + 1, (n_regions, 2), generator=g)
            self.hw = [tuple(int(v) for v in r) for r in hw]
        self.seed = seed
        self._cache = {}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        # deterministic per index: generated once, then served from memory (the reference reads tiles from disk)
        if i not in self._cache:
            self._cache[i] = self._make(i)
        return dict(self._cache[i])

    def _make(self, i):
        h, w = self.hw[i]
        g = torch.Generator().manual_seed(self.seed * 7919 + i)
        s2 = torch.randint(0, 10000, (4, h, w), generator=g).float()
        s1 = torch.randn(2, h, w, generator=g) * torch.tensor(stats.S1_STD).view(2, 1, 1) + torch.tensor(stats.S1_MEAN).view(2, 1, 1)
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        cy, cx = h / 2 + (i % 5) - 2, w / 2 - (i % 3) + 1
        r = 0.35 * min(h, w)
        inside = ((yy - cy) ** 2 + (xx - cx) ** 2) < r * r
        cid = i + 1
        admin = torch.where(inside, float(cid), float(cid + self.n))
        y = torch.rand(1, generator=g).item() * 500.0
        if self.nan_clouds > 0:
            s2, s1 = self._holes(i, s2, s1)
        item = {"S2": s2, "S1": s1, "admin_mask": admin, "y": torch.tensor(y), "census_idx": torch.tensor([cid]),
                "img_coords": (0, 0), "valid_coords": (0, 0), "season": i % 4}
        if self.buildings:
            item["building_counts"] = building_layer(h, w, torch.Generator().manual_seed(self.seed * 15485863 + i)).unsqueeze(0)
        return item


    def _holes(self, i, s2, s1):
        from .nanfill import select_s1_host
        h, w = s2.shape[1:]
        g = torch.Generator().manual_seed(self.seed * 104729 + i)       # a generator of its own: the data underneath does not change
        s2 = s2.clone()
        s2[:, cloud_mask(h, w, self.nan_clouds, g)] = float("nan")
        desc = s1.clone()
        desc[:, gap_rows(h, 0.08 if i % 3 == 0 else 0.02, g)] = float("nan")
        asc = s1.flip(-1).contiguous()                                   # the other orbit: same statistics, other values
        s1, _ = select_s1_host(desc, lambda: asc, self.ascfill)
        return s2, s1


TEST_RASTER_REGIONS = 400          # census units of a SyntheticTestRaster unless told otherwise


class SyntheticTestRaster:
    """A normalised (seasons,6,H,W) raster with a blocky census map (ids 1..n, 0 = outside) and a census table.

    raw=True: the loader's un-normalised bands instead -- S2 (seasons, 4, H, W) digital numbers, S1 (seasons, 2, H, W) descending-orbit
    backscatter and its ascending companion ``s1_asc`` -- with seeded NaNs: cloud discs over about ``nan_clouds`` of S2 (all bands) and
    orbit-gap rows over ``s1_gap`` of the descending S1.  The object is then the raster callable of ``eval.evaluate_raster(raw=True)``:
    ``self(x, y, season, ps)`` -> {"S2": (1,4,ps,ps), "S1": (1,2,ps,ps), "S1_asc": callable} (copies; ``self.raster`` is the object).

    coarse_regions = N > 0: a second, coarser census level (the reference's training level next to the fine one it is judged on) --
    ``boundary_coarse``: rectangular blocks of fine units grouped into about N coarse ones (ids 1 .. n_coarse, 0 outside; every fine unit
    lies in exactly one), ``census_idx_coarse`` and ``census_pop_coarse``: the sums of the member fine counts.  Nothing is drawn from the
    generator for it: every other attribute keeps its bits.

    buildings=True: ``.buildings`` (h, w), a ``building_layer`` without a season axis from a generator of its own (every other attribute
    keeps its bits); None otherwise.  ``eval.evaluate_raster`` picks it up from the raster object."""

    def __init__(self, h=2304, w=2560, seasons=1, n_regions=TEST_RASTER_REGIONS, seed=1610, device="cpu", raw=False, nan_clouds=0.0, s1_gap=0.0,
                 coarse_regions=0, buildings=False):
        g = torch.Generator().manual_seed(seed)
        self.raw = raw
        self.buildings = building_layer(h, w, torch.Generator().manual_seed(seed + 2)).to(device) if buildings else None
        if raw:
            self.s2 = torch.randint(0, 10000, (seasons, 4, h, w), generator=g).float()
            sd, mu = torch.tensor(stats.S1_STD).view(1, 2, 1, 1), torch.tensor(stats.S1_MEAN).view(1, 2, 1, 1)
            self.s1 = torch.randn(seasons, 2, h, w, generator=g) * sd + mu
            self.s1_asc = torch.randn(seasons, 2, h, w, generator=g) * sd + mu
            gh = torch.Generator().manual_seed(seed + 1)
            for s in range(seasons):
                self.s2[s][:, cloud_mask(h, w, nan_clouds, gh)] = float("nan")
                self.s1[s][:, gap_rows(h, s1_gap, gh)] = float("nan")
            self.s2, self.s1, self.s1_asc = self.s2.to(device), self.s1.to(device), self.s1_asc.to(device)
            self.raster = self
        else:
            self.raster = torch.randn(seasons, 6, h, w, generator=g).to(device)
        gy = int(n_regions ** 0.5)
        gx = (n_regions + gy - 1) // gy
        ys = torch.clamp((torch.arange(h) * gy) // h, max=gy - 1)
        xs = torch.clamp((torch.arange(w) * gx) // w, max=gx - 1)
        b = ys[:, None] * gx + xs[None, :] + 1
        b[b > n_regions] = 0
        self.boundary = b.to(torch.int32).to(device)
        self.census_idx = torch.arange(1, n_regions + 1)
        self.census_pop = torch.rand(n_regions, generator=g) * 2000
        self.shape = (h, w)
        if coarse_regions > 0:
            cy = max(1, min(gy, int(coarse_regions ** 0.5)))
            cx = max(1, min(gx, (coarse_regions + cy - 1) // cy))
            fid = torch.arange(n_regions)                                   # fine unit id - 1 -> its grid cell -> its coarse block
            block = ((fid // gx) * cy // gy) * cx + (fid % gx) * cx // gx
            _, member = torch.unique(block, return_inverse=True)            # compact ids in block order
            coarse_of = torch.cat([torch.zeros(1, dtype=torch.int64), member + 1])
            self.boundary_coarse = coarse_of[b.long()].to(torch.int32).to(device)
            n_coarse = int(member.max()) + 1
            self.census_idx_coarse = torch.arange(1, n_coarse + 1)
            self.census_pop_coarse = torch.zeros(n_coarse, dtype=torch.float64).index_add_(0, member, self.census_pop.double()).float()
            self.coarse_of_fine = coarse_of                                 # [fine id] -> coarse id (0 -> 0)

    def __call__(self, x, y, season, ps):
        """One raw window (raw=True): copies of the bands, so that the fill can work in place."""
        win = lambda t: t[season:season + 1, :, x:x + ps, y:y + ps].clone(memory_format=torch.contiguous_format)  # noqa: E731
        return {"S2": win(self.s2), "S1": win(self.s1), "S1_asc": lambda: win(self.s1_asc)}
