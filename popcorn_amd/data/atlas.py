"""The resident atlas: several resident regions trained on at once, one launch per batch whichever regions its crops come from.

The reference trains on several countries: one ``Population_Dataset`` per entry of ``-tregtrain``, each with its own ``ascfill = region in
need_asc``, concatenated and shuffled with ``weak_batch_size = 2`` (run_train.py:423-431), so the crops of a step usually come from
different rasters.  data/region.py holds one region per feed.  Here:

  ``ResidentAtlas``      R ``ResidentRegion``s on one device (one S2 type, a building layer on all or on none) behind one C handle
                         (``ops.AtlasHandle``): the descriptors are uploaded once
  ``AtlasPlan``          the regions' ``RegionPlan``s concatenated in region order plus a ``region`` column; ``crops`` and ``bbox`` stay in
                         each region's own coordinates
  ``plan_repair_atlas``  ``plan_repair`` per region with that region's ``ascfill``, the patch tables joined into one (``idx`` / ``val``
                         concatenated, ``off`` shifted: ``ops.region_patch_apply`` takes an item's range per item, so it needs no change)
  ``AtlasRegionFeed``    ``ResidentRegionFeed`` with ``ops.atlas_gather`` as its launch
  ``AtlasBatchFeed``     ``ResidentBatchFeed`` with ``ops.atlas_batch`` as its launch

An epoch takes the same draws from the generator as the region feeds over the concatenated plan (one ``randperm``, the seasons'
``randint``, ``plan_batches``' ``randperm`` under a pixel budget), so a feed over an atlas of ONE region yields the bits of the region
feed with the same generator.  ``img_coords`` / ``valid_coords`` are in the item's own region and every sample carries ``"region"``, the
host list of region indices.  Not part of this module: sharding a plan over data-parallel ranks, graph capture of the gather, the
reference's ``-ascAug``, mixed S2 types in one atlas, per-region normalisation statistics."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .region import RegionPlan, RegionRepair, ResidentBatchFeed, ResidentRegion, ResidentRegionFeed, plan_repair


class ResidentAtlas:
    """R ``ResidentRegion``s on one device behind one handle.  regions: a list of 1 .. PC_ATLAS_MAX_REGIONS regions, all with the same S2
    dtype and all or none with a building layer (ValueError otherwise); names: one label per region (default "0", "1", ...).
    ``seasons`` is the smallest season count of the atlas: what a feed may draw from.  Owns the handle (``ops.AtlasHandle``), which keeps
    the rasters alive."""

    def __init__(self, regions, names=None):
        self.regions = list(regions)
        if not self.regions or any(not isinstance(r, ResidentRegion) for r in self.regions):
            raise ValueError("ResidentAtlas: a non-empty list of ResidentRegion")
        self.names = [str(k) for k in range(len(self.regions))] if names is None else [str(v) for v in names]
        if len(self.names) != len(self.regions):
            raise ValueError(f"ResidentAtlas: one name per region ({len(self.regions)}), got {len(self.names)}")
        self.handle = ops.AtlasHandle([{"s2": r.s2, "s1": r.s1, "s1_asc": r.s1_asc, "boundary": r.boundary, "buildings": r.buildings,
                                        "band_sel": r.band_sel} for r in self.regions])
        self.device = self.regions[0].device
        self.seasons = min(r.seasons for r in self.regions)
        self.layered = self.handle.layered

    def __len__(self):
        return len(self.regions)

    def gather(self, region_of, crops, out=None, orbit=None):
        """``ops.atlas_gather``: crop b = crops[b] = {x0, x1, y0, y1, season} of region region_of[b]."""
        return ops.atlas_gather(self.handle, region_of, crops, out=out, orbit=orbit)


class AtlasPlan(RegionPlan):
    """The concatenation of per-region ``RegionPlan``s plus ``region`` int64 (n,): the region of every row.  ``crops`` and ``bbox`` stay in
    each region's own coordinates; census_idx / y are padded to the widest member with -1 / 0.  All members are ``multi`` or none."""

    def __init__(self, crops, census_idx, y, census_n, bbox, multi, region):
        super().__init__(crops, census_idx, y, census_n, bbox, multi)
        self.region = torch.as_tensor(region, dtype=torch.int64).reshape(-1)
        if self.region.numel() != len(self):
            raise ValueError(f"AtlasPlan: one region per row ({len(self)}), got {self.region.numel()}")

    @classmethod
    def concat(cls, plans):
        """From one ``RegionPlan`` per region, in region order (a region without rows contributes an empty plan)."""
        plans = list(plans)
        if not plans:
            raise ValueError("AtlasPlan.concat: at least one plan")
        if len({bool(p.multi) for p in plans}) != 1:
            raise ValueError("AtlasPlan.concat: all member plans are multi-unit plans or none of them is")
        K = max(int(p.census_idx.shape[1]) for p in plans)

        def wide(t, fill):
            return torch.nn.functional.pad(t, (0, K - t.shape[1]), value=fill)

        return cls(torch.cat([p.crops for p in plans]), torch.cat([wide(p.census_idx, -1) for p in plans]),
                   torch.cat([wide(p.y, 0.0) for p in plans]), [n for p in plans for n in p.census_n], torch.cat([p.bbox for p in plans]),
                   plans[0].multi, torch.cat([torch.full((len(p),), k, dtype=torch.int64) for k, p in enumerate(plans)]))

    def subset(self, rows):
        sel = torch.as_tensor(list(rows), dtype=torch.int64)
        return AtlasPlan(self.crops[sel], self.census_idx[sel], self.y[sel], [self.census_n[int(i)] for i in sel], self.bbox[sel], self.multi,
                         self.region[sel])

    def member(self, k):
        """(rows, plan): the rows of region k in this plan's order and their ``RegionPlan``."""
        rows = torch.nonzero(self.region == int(k)).reshape(-1).tolist()
        return rows, RegionPlan.subset(self, rows)

    def __eq__(self, other):
        return isinstance(other, AtlasPlan) and torch.equal(self.region, other.region) and self._as_region() == other._as_region()

    def _as_region(self):
        return RegionPlan(self.crops, self.census_idx, self.y, self.census_n, self.bbox, self.multi)


class AtlasRepair(RegionRepair):
    """The joined ``RegionRepair`` of an ``AtlasPlan``: ``dropped`` / ``kept`` are rows of the ORIGINAL atlas plan, ``dropped_by_region``
    {region: rows of that plan} reports them per region."""

    def __init__(self, *args, dropped_by_region=None, **kw):
        super().__init__(*args, **kw)
        self.dropped_by_region = dict(dropped_by_region or {})


def join_patch_tables(offs, idxs, vals):
    """The patch tables of several plans as one (pure torch): offs = their ``off`` (n_k * S + 1 each, host), idxs / vals their entries.
    Returns (off, idx, val): idx and val concatenated, every ``off`` shifted by the entries in front of it."""
    base, parts = 0, []
    for off in offs:
        parts.append(off[:-1] + base)
        base += int(off[-1])
    off = torch.cat(parts + [torch.tensor([base], dtype=torch.int64)])
    return off, torch.cat(list(idxs)), torch.cat(list(vals))


def plan_repair_atlas(atlas, plan, seasons=1, ascfill=(), pixel_budget=1 << 22):
    """``plan_repair`` of an ``AtlasPlan``, region by region: returns (plan', AtlasRepair).  ascfill: the region indices that take the
    ascending orbit wherever the descending one holds NaN (the reference's ``need_asc``), or True / False for all / none.  Every region
    with rows gets one ``plan_repair`` (its own census pass, its own dropped rows); plan' lists the surviving rows in region order and the
    patch tables are joined (``join_patch_tables``).  Whatever ``plan_repair`` raises for a region is raised here."""
    if not isinstance(plan, AtlasPlan):
        raise ValueError("plan_repair_atlas: an AtlasPlan")
    R = len(atlas)
    asc = set(range(R)) if ascfill is True else set() if ascfill in (False, None) else {int(k) for k in ascfill}
    if any(not 0 <= k < R for k in asc):
        raise ValueError(f"plan_repair_atlas: ascfill names regions in [0, {R}), got {sorted(asc)}")
    if len(plan) < 1 or int(plan.region.min()) < 0 or int(plan.region.max()) >= R:
        raise ValueError(f"plan_repair_atlas: a plan with at least one crop whose regions lie in [0, {R})")
    plans, reps, kept, dropped, by_region = [], [], [], [], {}
    for k in range(R):
        rows, sub = plan.member(k)
        if not rows:
            plans.append(sub)
            continue
        new, rep = plan_repair(atlas.regions[k], sub, seasons=seasons, ascfill=k in asc, pixel_budget=pixel_budget)
        plans.append(new)
        reps.append(rep)
        kept += [rows[i] for i in rep.kept]
        by_region[k] = [rows[i] for i in rep.dropped]
        dropped += by_region[k]
    off, idx, val = join_patch_tables([r.off for r in reps], [r.idx for r in reps], [r.val for r in reps])
    joined = AtlasRepair(torch.cat([r.orbit for r in reps]), dropped, kept, torch.cat([r.counts for r in reps]), idx, val, off,
                         [hw for r in reps for hw in r.hw], build_ms=sum(r.build_ms for r in reps), dropped_by_region=by_region)
    return AtlasPlan.concat(plans), joined


def _check_atlas(what, atlas, plan):
    if not isinstance(atlas, ResidentAtlas) or not isinstance(plan, AtlasPlan):
        raise ValueError(f"{what}: a ResidentAtlas and an AtlasPlan")
    if len(plan) and (int(plan.region.min()) < 0 or int(plan.region.max()) >= len(atlas)):
        raise ValueError(f"{what}: the plan names regions outside [0, {len(atlas)})")


class AtlasRegionFeed(ResidentRegionFeed):
    """``ResidentRegionFeed`` over a ``ResidentAtlas`` and an ``AtlasPlan``: the same epoch draws, keys and label indexing; each batch is one
    ``ops.atlas_gather`` launch and carries ``"region"``.  seasons must not exceed the smallest season count of the atlas."""

    def __init__(self, atlas, plan, batch_size, generator=None, drop_last=True, seasons=1, repair=None):
        _check_atlas("AtlasRegionFeed", atlas, plan)
        super().__init__(atlas, plan, batch_size, generator=generator, drop_last=drop_last, seasons=seasons, repair=repair)
        self._region = plan.region.numpy()

    def _gather(self, idx, crops, orbit=None):
        return self.region.gather(self._region[idx], crops, orbit=orbit)


class AtlasBatchFeed(ResidentBatchFeed):
    """``ResidentBatchFeed`` over a ``ResidentAtlas`` and an ``AtlasPlan``: the same epoch draws, coins, keys and batch composition; each
    batch is one ``ops.atlas_batch`` launch and carries ``"region"``."""

    def __init__(self, atlas, plan, batch_size, **kw):
        _check_atlas("AtlasBatchFeed", atlas, plan)
        super().__init__(atlas, plan, batch_size, **kw)
        self._region = plan.region.numpy()

    def _assemble(self, idx, crops, params, labels, orbit=None):
        return ops.atlas_batch(self.region.handle, self._region[np.asarray(idx, dtype=np.int64)], crops, params, labels=labels, orbit=orbit)
