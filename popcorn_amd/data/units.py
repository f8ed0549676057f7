"""Multi-unit census supervision on the data side: items that list SEVERAL census units of one crop, and their collate.

The reference's weaksup items are the bounding-box crop of ONE unit (data/PopulationDataset.py:425-470); ``admin_mask`` already carries the
ids of all its neighbours.  A multi-unit item lists K of them: ``census_idx`` (K,) int64 and ``y`` (K,) -- the model and the fused step
then supervise all K in one pass (popcorn_amd/model/popcorn.py, popcorn_amd/train.py, csrc/units.hip).  ``collate.py`` / ``dataset.py`` and
their one-unit behaviour are untouched.  Host-side glue, plain torch."""
from __future__ import annotations

import torch
from torch.utils.data import Dataset

from . import stats
from .collate import Population_Dataset_collate_fn

PAD_ID = -1          # census_idx padding (ids are non-negative); census_n says how many slots of a row count


class SyntheticMultiUnitDataset(Dataset):
    """Crops tiled by K irregular census units (listed, each with its own count ``y``) plus unlisted neighbours: the nearest-seed
    tiling of K + ``neighbours`` jittered seed points, the neighbours' seeds near the crop's border.  Item keys as
    ``SyntheticWeaksupDataset`` except ``census_idx`` (K_i,) int64 and ``y`` (K_i,).  ragged: every third item lists one unit fewer and
    every fifth two fewer (at least one), so that batches are ragged; the dropped units stay in ``admin_mask`` as neighbours.
    buildings (opt-in): every item carries ``building_counts`` (1, h, w), ``dataset.building_layer`` from a generator of its own -- every
    other tensor of the item keeps its bits; ``collate_units`` pads it with zeros as the plain collate does."""

    def __init__(self, n_regions=64, units=4, neighbours=3, min_hw=64, max_hw=144, seed=1600, fixed_hw=None, ragged=False, buildings=False):
        self.buildings = bool(buildings)
        if units < 1:
            raise ValueError("units >= 1")
        self.n, self.units, self.neighbours, self.ragged = n_regions, int(units), int(neighbours), bool(ragged)
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
        if i not in self._cache:
            self._cache[i] = self._make(i)
        return dict(self._cache[i])

    def _make(self, i):
        h, w = self.hw[i]
        K, M = self.units, self.neighbours
        g = torch.Generator().manual_seed(self.seed * 7919 + i)
        s2 = torch.randint(0, 10000, (4, h, w), generator=g).float()
        s1 = torch.randn(2, h, w, generator=g) * torch.tensor(stats.S1_STD).view(2, 1, 1) + torch.tensor(stats.S1_MEAN).view(2, 1, 1)
        # listed units: seeds inside the central 70 % of the crop; neighbours: seeds in the outer 10 % frame
        sy = torch.cat([(0.15 + 0.7 * torch.rand(K, generator=g)) * h, torch.where(torch.rand(M, generator=g) < 0.5, torch.tensor(0.05), torch.tensor(0.95)) * h])
        sx = torch.cat([(0.15 + 0.7 * torch.rand(K, generator=g)) * w, torch.rand(M, generator=g) * w])
        wgt = 0.75 + 0.5 * torch.rand(K + M, generator=g)                 # unequal metrics: irregular, unequal units
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        d = ((yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2) * wgt[:, None, None]
        owner = d.argmin(0)
        # ids: the item's K units are consecutive (adjacent ids), neighbours far above them; 0 is never used
        base = 1 + i * K
        ids = torch.cat([base + torch.arange(K), 1_000_000 + i * M + torch.arange(M)])
        admin = ids[owner].float()
        k_i = K
        if self.ragged:
            k_i = max(1, K - (1 if i % 3 == 0 else 0) - (2 if i % 5 == 0 else 0))
        y = torch.rand(K, generator=g) * 500.0
        item = {"S2": s2, "S1": s1, "admin_mask": admin, "y": y[:k_i].clone(), "census_idx": ids[:k_i].to(torch.int64).clone(),
                "img_coords": (0, 0), "valid_coords": (0, 0), "season": i % 4}
        if self.buildings:
            from .dataset import building_layer
            item["building_counts"] = building_layer(h, w, torch.Generator().manual_seed(self.seed * 15485863 + i)).unsqueeze(0)
        return item


def collate_units(batch):
    """``Population_Dataset_collate_fn`` for multi-unit items: ``census_idx`` (K_i,) / ``y`` (K_i,) are padded to the batch maximum K --
    ``census_idx`` (n, K) int64 with PAD_ID = -1, ``y`` (n, K) fp32 with 0 -- and ``census_n`` (a list of n ints, host data: it sizes the
    step's N) says how many slots of each row count.  Every other key is the plain collate's.  A batch of 1-unit items carries the plain
    collate's tensors with a trailing K = 1 axis on ``census_idx`` / ``y``."""
    counts = [int(item["census_idx"].numel()) for item in batch]
    if min(counts) < 1 or any(int(item["y"].numel()) != c for item, c in zip(batch, counts)):
        raise ValueError("collate_units: every item lists >= 1 units and as many y values as census_idx entries")
    K = max(counts)
    # the plain collate does all the rest; it wants a scalar y and a (1,) census_idx per item
    out = Population_Dataset_collate_fn([{**item, "y": item["y"].reshape(-1)[0], "census_idx": item["census_idx"].reshape(-1)[:1]}
                                         for item in batch])
    cidx = torch.full((len(batch), K), PAD_ID, dtype=torch.int64)
    y = torch.zeros(len(batch), K)
    for i, (item, c) in enumerate(zip(batch, counts)):
        cidx[i, :c] = item["census_idx"].reshape(-1).to(torch.int64)
        y[i, :c] = item["y"].reshape(-1).float()
    out.update({"census_idx": cidx, "y": y, "census_n": counts})
    return out


def flat_valid(t, census_n):
    """(B, K) per-slot values -> the flat (N,) vector over the valid slots in (b, k) order (the order of the model's ``popcount``)."""
    return torch.cat([t[b, :int(c)] for b, c in enumerate(census_n)])
