"""Region-resident training data: a country's rasters stay in HBM and a batch of census-unit crops is ONE gather launch.

The reference trains from a region: ``Population_Dataset(mode="weaksup")`` holds the S1 / S2 rasters, the boundary raster and the census
table of a country; item i is the bounding box of census unit i grown by 32 px and clipped to the raster, cut out of those rasters
(data/PopulationDataset.py:403-458, :624-649), and the collate pads the items of a batch to the largest (:885-958).  The bounding boxes
and pixel counts are made at preprocessing time with one pass per unit (utils/02_preprocess_rwa_shapefile.py:142-161).  Here:

  ``ResidentRegion``      the device tensors + the unit table from one device pass (``ops.region_units``)
  ``plan_one_unit``       the reference's items: one crop per census unit, both size filters
  ``plan_multi_unit``     crops that list up to K complete units each (multi-unit census supervision, data/units.py), greedy and deterministic
  ``ResidentRegionFeed``  iterates like ``feed.RegionFeed``: per batch one ``ops.region_gather`` launch, no loader / collate / pinned
                          staging / copy stream and no producer thread
  ``ResidentBatchFeed``   the same batches in the form the fused step takes -- gather, augmentation, raw tile and labels in ONE
                          ``ops.region_batch`` launch --, cut at a fixed count or composed by size under a pixel budget (``plan_batches``)
  ``plan_repair``         the reference's per-item NaN repair (:419-441), decided ONCE for a plan: the S1 orbit of every (item, season) from
                          one census pass, the repaired sites as a sparse patch table in HBM (``RegionRepair``); a feed built with
                          ``repair=`` gathers with orbits and lays each batch's patches over it with one small launch
  ``ResidentWindows``     the same region EVALUATED: the sliding windows of ``eval.evaluate_raster`` planned once -- orbit per window from
                          one census pass, repaired sites as a patch table (``repair_core``, shared with ``plan_repair``), sharded over
                          ranks like the windows --, each window's normalised model input then ONE ``ops.region_window`` launch with no
                          fill and no synchronisation; it is the raster callable ``evaluate_raster`` already takes
  ``split_census``        the reference's 80 / 20 split of the census rows (one shuffle with random_state 1610), before the size filters
  ``ResidentItems``       the same region VALIDATED: the items of a (validation) plan with season, orbit and repaired sites planned once,
                          each item's normalised input and admin mask then ONE ``ops.region_item`` launch

Several regions at once (the reference's multi-country -tregtrain): data/atlas.py, whose feeds are these with the launch replaced.
Host glue, plain torch; the kernels are csrc/region.hip, csrc/region_batch.hip, csrc/region_repair.hip and csrc/region_crop.hip.
Deviations from the reference, all named where they happen: units without pixels are dropped (``plan_one_unit``); the per-epoch order and the season per item come from a torch generator, not Python's ``random`` stream
(``ResidentRegionFeed``); without ``plan_repair`` the resident S1 is the orbit already chosen per season (``--nan_fill`` fills what is
left), with it an item the reference would end on ("No data here!") is dropped from the plan.  Sharding a plan over data-parallel ranks and graph capture of the gather are not part of this module."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from .. import ops
from . import stats

REFERENCE_BANDS = (2, 1, 0, 3, 0, 1)      # file bands (3, 2, 1, 4) of S2 and (1, 2) of S1, 1-based (PopulationDataset.py:566-568), 0-based
MODEL_ORDER_BANDS = (0, 1, 2, 3, 0, 1)    # rasters whose bands are stored in the model's order already (SyntheticTestRaster)
MAX_PIX, MAX_PIX_BOX = 10_000_000, 12_000_000      # the reference's defaults (PopulationDataset.py:124-131)
PC_GATHER_MAX_B = 128                               # crops of one gather launch (popcorn_hip.h: PC_REGION_GATHER_MAX_B)


class ResidentRegion:
    """The rasters of one region on the device: s2 (S, C2, h, w) fp32 or uint16 digital numbers, s1 fp32 (S, C1, h, w), boundary int32
    (h, w) of census-unit ids, optionally s1_asc (the ascending-orbit S1, shaped and checked like s1), and the census table (census_idx (n,) ids, census_pop (n,) counts; host).  ``table`` (host int32
    (num_ids, 5) = {xmin, xmax, ymin, ymax, count}, the reference's convention) is computed once on the device.  Raises when the boundary
    holds ids outside [0, num_ids) (num_ids defaults to the largest census id + 1) and when the tensors that still have to move do not
    fit the device's free memory.
    buildings: the building layer a dataset ships (PopulationDataset.py:606-612), an (h, w) raster without a season axis, kept resident as
    fp32, shape-checked against the boundary and counted in the free-memory check.  Every feed / plan over the region then emits
    ``building_counts`` from the launch that produces the rest (``plan_repair`` / ``RegionRepair`` never touch it: the reference repairs
    S2 / S1 only)."""

    def __init__(self, s2, s1, boundary, census_idx, census_pop, band_sel=REFERENCE_BANDS, device=None, num_ids=None, s1_asc=None,
                 buildings=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"ResidentRegion: the region lives on a HIP device, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if s1_asc is not None and tuple(s1_asc.shape) != tuple(s1.shape):
            raise ValueError(f"ResidentRegion: s1_asc is shaped like s1 {tuple(s1.shape)}, got {tuple(s1_asc.shape)}")
        if buildings is not None and tuple(buildings.shape) != tuple(boundary.shape):
            raise ValueError(f"ResidentRegion: buildings is an (h, w) raster shaped like the boundary {tuple(boundary.shape)}, got "
                             f"{tuple(buildings.shape)}")
        need = sum(t.numel() * t.element_size() for t in (s2, s1, boundary, s1_asc) if t is not None and t.device != dev)
        if buildings is not None and (buildings.device != dev or buildings.dtype != torch.float32):
            need += buildings.numel() * 4                              # resident as fp32 whatever it arrives as
        if need:
            free, total = torch.cuda.mem_get_info(dev)
            if need > free:
                raise MemoryError(f"ResidentRegion: the rasters take {need / 2 ** 30:.2f} GiB, device {dev} has {free / 2 ** 30:.2f} GiB free "
                                  f"of {total / 2 ** 30:.2f}: keep fewer seasons resident or store S2 as uint16")
        self.s2 = s2.to(dev).contiguous()
        self.s1 = s1.to(dev).float().contiguous()
        self.s1_asc = None if s1_asc is None else s1_asc.to(dev).float().contiguous()
        self.boundary = boundary.to(dev).to(torch.int32).contiguous()
        self.buildings = None if buildings is None else buildings.to(dev).float().contiguous()
        if self.s2.dtype not in (torch.float32, torch.uint16):
            raise ValueError(f"ResidentRegion: S2 as fp32 or uint16, got {self.s2.dtype}")
        self.device = dev
        self.seasons = int(self.s2.shape[0])
        self.shape = tuple(int(v) for v in self.boundary.shape)
        self.band_sel = tuple(int(v) for v in band_sel)
        self.census_idx = torch.as_tensor(census_idx, dtype=torch.int64).cpu().reshape(-1)
        self.census_pop = torch.as_tensor(census_pop, dtype=torch.float32).cpu().reshape(-1)
        if self.census_idx.numel() != self.census_pop.numel() or self.census_idx.numel() < 1 or int(self.census_idx.min()) < 0:
            raise ValueError("ResidentRegion: census_idx (n >= 1 non-negative ids) and census_pop (n counts)")
        self.num_ids = int(self.census_idx.max()) + 1 if num_ids is None else int(num_ids)
        table, stray = ops.region_units(self.boundary, self.num_ids)
        stray = int(stray.item())                                  # the one synchronisation, at construction
        if stray > 0:
            raise ValueError(f"ResidentRegion: {stray} pixels of the boundary raster hold ids outside [0, {self.num_ids}): the census table "
                             "does not cover the raster")
        self.table = table.cpu()

    @classmethod
    def from_synthetic(cls, data, device=None, with_asc=False):
        """From a ``SyntheticTestRaster(raw=True, ...)``: its S2 / S1 / boundary / census table, bands in the model's order.  with_asc: its
        ascending-orbit S1 stays resident as well (a third more S1 memory; off by default).  Its building layer (``buildings=True``) is
        taken over."""
        if not getattr(data, "raw", False):
            raise ValueError("ResidentRegion.from_synthetic: a SyntheticTestRaster(raw=True)")
        return cls(data.s2, data.s1, data.boundary, data.census_idx, data.census_pop, band_sel=MODEL_ORDER_BANDS,
                   device=data.s2.device if data.s2.is_cuda and device is None else device, s1_asc=data.s1_asc if with_asc else None,
                   buildings=getattr(data, "buildings", None))

    def gather(self, crops, out=None, orbit=None):
        """``ops.region_gather`` of host crops (B, 5) = {x0, x1, y0, y1, season} on this region; orbit: per crop 0 = descending S1,
        1 = ascending (None: the plain gather).  A region with a building layer gathers it in the same launch ("building_counts")."""
        kw = {} if self.buildings is None else {"buildings": self.buildings}
        if orbit is None:
            return ops.region_gather(self.s2, self.s1, self.boundary, self.band_sel, crops, out=out, **kw)
        return ops.region_gather(self.s2, self.s1, self.boundary, self.band_sel, crops, out=out, s1_asc=self.s1_asc, orbit=orbit, **kw)


class RegionPlan:
    """n crops over a region: crops int64 (n, 4) = {x0, x1, y0, y1} (rows [x0, x1), columns [y0, y1)), the listed units census_idx int64
    (n, K) padded with -1, their counts y fp32 (n, K) padded with 0, census_n (n ints: listed units per crop), bbox int64 (n, 4): the union
    bounding box of the listed units (the item's ``valid_coords``), multi: the batch form (``collate_units``' or the plain collate's)."""

    def __init__(self, crops, census_idx, y, census_n, bbox, multi):
        self.crops, self.census_idx, self.y, self.census_n, self.bbox, self.multi = crops, census_idx, y, list(census_n), bbox, bool(multi)

    def __len__(self):
        return int(self.crops.shape[0])

    def subset(self, rows):
        """The plan of the listed rows, in the listed order: every table keeps its row."""
        sel = torch.as_tensor(list(rows), dtype=torch.int64)
        return RegionPlan(self.crops[sel], self.census_idx[sel], self.y[sel], [self.census_n[int(i)] for i in sel], self.bbox[sel], self.multi)

    def __eq__(self, other):
        return (isinstance(other, RegionPlan) and self.multi == other.multi and self.census_n == other.census_n and
                all(torch.equal(getattr(self, k), getattr(other, k)) for k in ("crops", "census_idx", "y", "bbox")))


def _grow(bbox, shape, admin_overlap):
    """bbox (.., 4) = {xmin, xmax, ymin, ymax} grown by admin_overlap and clipped to the raster (PopulationDataset.py:644-649)."""
    out = bbox.clone()
    out[..., 0] = (bbox[..., 0] - admin_overlap).clamp(min=0)
    out[..., 1] = (bbox[..., 1] + admin_overlap).clamp(max=int(shape[0]))
    out[..., 2] = (bbox[..., 2] - admin_overlap).clamp(min=0)
    out[..., 3] = (bbox[..., 3] + admin_overlap).clamp(max=int(shape[1]))
    return out


def _eligible(table, census_idx, census_pop, max_pix, max_pix_box):
    """Rows of the census table that survive the reference's two filters, in census order, without the units that have no pixel:
    (ids, pops, bbox int64 (m, 4), count int64 (m,))."""
    table = torch.as_tensor(table).cpu().to(torch.int64)
    ids = torch.as_tensor(census_idx, dtype=torch.int64).cpu().reshape(-1)
    pop = torch.as_tensor(census_pop, dtype=torch.float32).cpu().reshape(-1)
    if ids.numel() != pop.numel():
        raise ValueError("census_idx and census_pop differ in length")
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= table.shape[0] or ids.unique().numel() != ids.numel()):
        raise ValueError(f"census ids must be distinct and lie in [0, {table.shape[0]})")
    rows = table[ids]
    bbox, count = rows[:, :4], rows[:, 4]
    keep = count < max_pix                                                      # PopulationDataset.py:124-125
    area = (bbox[:, 1] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 2])               # calculate_pixel_count, :348-357
    keep &= area < max_pix_box                                                  # :128-131
    keep &= count > 0
    return ids[keep], pop[keep], bbox[keep], count[keep]


SPLIT_SEED = 1610                                   # the reference's random_state (PopulationDataset.py:112, :117)


def split_census(census_idx, census_pop, split, frac=0.8, seed=SPLIT_SEED):
    """The reference's 80 / 20 split of a census table (data/PopulationDataset.py:105-121; run_train.py:425-440 builds the training set
    with split="train" and the validation set with split="val" under ``-wv``): returns (census_idx', census_pop').
    Rule: the n rows are permuted as ``DataFrame.sample(frac=1, random_state=1610)`` permutes them, which is
    ``numpy.random.RandomState(1610).permutation(n)`` (pinned by tests/golden/g14_split.npz, written with pandas itself); "train" is the
    first int(n * frac) rows of that order, "val" the rest, and both KEEP the permuted order, as the reference's items do after its
    ``reset_index``.  "all" returns the rows untouched.  Both cuts come from one permutation, so they are disjoint and cover the table.
    Placement: before the two size filters, as in the reference -- hand the result to ``plan_one_unit`` / ``plan_multi_unit`` as it is.
    Multi-unit plans: the units are split first and a crop is composed from one split's units only; a validation unit may still lie inside
    a training crop, where it shows up in ``admin_mask`` as an unlisted neighbour, which the step ignores (its pixels reach no loss term).
    int(n * frac) == 0 (n = 1) gives an empty training split: the caller refuses it, naming n.  Pure host code; no pandas."""
    ids = torch.as_tensor(census_idx, dtype=torch.int64).cpu().reshape(-1)
    pop = torch.as_tensor(census_pop, dtype=torch.float32).cpu().reshape(-1)
    if ids.numel() != pop.numel():
        raise ValueError("split_census: census_idx and census_pop differ in length")
    if split == "all":
        return ids, pop
    if split not in ("train", "val"):
        raise ValueError(f"split_census: split is \"all\", \"train\" or \"val\", got {split!r}")
    n = ids.numel()
    order = torch.from_numpy(np.random.RandomState(int(seed)).permutation(n).astype(np.int64))
    cut = int(n * frac)
    rows = order[:cut] if split == "train" else order[cut:]
    return ids[rows], pop[rows]


def plan_one_unit(table, census_idx, census_pop, shape, admin_overlap=32, max_pix=MAX_PIX, max_pix_box=MAX_PIX_BOX):
    """The reference's weaksup items over a unit table: rows with count >= max_pix are dropped, then rows whose bounding box has
    >= max_pix_box pixels (PopulationDataset.py:124-131); the crop is the bounding box grown by admin_overlap and clipped to the raster
    (:413, :644-649); ``y`` = POP20 and ``census_idx`` = idx of the row (:453-457).  Items keep the census table's order.
    Deviation: units with count == 0 are dropped -- the reference would emit the crop [0, admin_overlap) x [0, admin_overlap) at the
    raster's origin for their all-zero bounding box, without a pixel of the unit in it."""
    ids, pop, bbox, _ = _eligible(table, census_idx, census_pop, max_pix, max_pix_box)
    n = ids.numel()
    return RegionPlan(_grow(bbox, shape, admin_overlap), ids.reshape(n, 1), pop.reshape(n, 1), [1] * n, bbox.clone(), multi=False)


def plan_multi_unit(table, census_idx, census_pop, shape, units_per_crop=4, admin_overlap=32, max_pix=MAX_PIX, max_pix_box=MAX_PIX_BOX):
    """Crops that list up to ``units_per_crop`` units which lie COMPLETELY inside them, every eligible unit (``plan_one_unit``'s filters)
    in exactly one crop.  Greedy and deterministic given the table: the seed is the first unassigned unit in row-major order of its
    bounding box's origin; then the nearest unassigned unit (squared distance of the bounding-box centre to the centre of the crop's
    current union box, in integers; ties to the earlier unit in that order) joins while the union box grown by admin_overlap and clipped
    stays under max_pix_box pixels and fewer than units_per_crop are listed; the first candidate that does not fit closes the crop.
    Invariants: (a) every eligible unit is listed exactly once; (b) every listed unit's bounding box lies inside its crop, so the unit
    is complete there and ``y`` is its whole count; (c) a crop reaches the budget only when it lists a single unit; (d) at most
    units_per_crop distinct non-negative ids per crop; (e) crops are non-empty and inside the raster.  Unlisted units inside a crop stay
    in ``admin_mask`` as neighbours, which the step ignores."""
    K = int(units_per_crop)
    if K < 1:
        raise ValueError("plan_multi_unit: units_per_crop >= 1")
    ids, pop, bbox, _ = _eligible(table, census_idx, census_pop, max_pix, max_pix_box)
    m = ids.numel()
    order = sorted(range(m), key=lambda i: (int(bbox[i, 0]), int(bbox[i, 2]), int(ids[i])))
    rank = torch.empty(m, dtype=torch.int64)
    rank[torch.tensor(order, dtype=torch.int64)] = torch.arange(m)
    cx2, cy2 = bbox[:, 0] + bbox[:, 1], bbox[:, 2] + bbox[:, 3]               # twice the centres: integers
    free = torch.ones(m, dtype=torch.bool)
    FAR = torch.iinfo(torch.int64).max
    lists, unions = [], []
    for seed in order:
        if not bool(free[seed]):
            continue
        free[seed] = False
        members, union = [seed], bbox[seed].clone()
        while len(members) < K and bool(free.any()):
            ux2, uy2 = union[0] + union[1], union[2] + union[3]
            key = ((cx2 - ux2) ** 2 + (cy2 - uy2) ** 2) * m + rank            # distinct keys: the arg-min is unique
            cand = int(torch.where(free, key, torch.full_like(key, FAR)).argmin())
            grown = torch.stack([torch.minimum(union[0], bbox[cand, 0]), torch.maximum(union[1], bbox[cand, 1]),
                                 torch.minimum(union[2], bbox[cand, 2]), torch.maximum(union[3], bbox[cand, 3])])
            g = _grow(grown, shape, admin_overlap)
            if int((g[1] - g[0]) * (g[3] - g[2])) >= max_pix_box:
                break
            free[cand] = False
            members.append(cand)
            union = grown
        lists.append(members)
        unions.append(union)
    n = len(lists)
    cidx = torch.full((n, K), -1, dtype=torch.int64)
    y = torch.zeros(n, K, dtype=torch.float32)
    for i, mem in enumerate(lists):
        cidx[i, :len(mem)] = ids[mem]
        y[i, :len(mem)] = pop[mem]
    union = torch.stack(unions) if n else torch.zeros(0, 4, dtype=torch.int64)
    return RegionPlan(_grow(union, shape, admin_overlap), cidx, y, [len(mem) for mem in lists], union, multi=True)


class RegionRepair:
    """What ``plan_repair`` decided for a plan of n items over S seasons, all of it fixed before the first step:
    orbit int8 (n, S): 0 = the descending S1, 1 = the ascending one; dropped: the rows of the ORIGINAL plan that were taken out, kept: the
    rows that stayed (row k of the new plan is row kept[k] of the original); counts int64 (n, S, 3): the census of every kept (item,
    season) = NaN entries of {S2, descending S1, ascending S1}; the patch table idx int32 / val fp32 (device) with off int64 (n * S + 1)
    on the host and the device (``off_dev``): the entries of (item i, season s) are [off[i * S + s], off[i * S + s + 1]), ascending, idx =
    (c * h + i) * w + j in the item's own (6, h, w) space; hw: the items' extents; entries, nbytes (table bytes on the device),
    ascending (how many (item, season) pairs switched orbit), build_ms."""

    def __init__(self, orbit, dropped, kept, counts, idx, val, off, hw, build_ms=0.0):
        self.orbit, self.dropped, self.kept, self.counts, self.idx, self.val, self.off = orbit, list(dropped), list(kept), counts, idx, val, off
        self.hw = [(int(h), int(w)) for h, w in hw]
        self.n, self.seasons = int(orbit.shape[0]), int(orbit.shape[1])
        self.off_dev = off.to(idx.device)
        self.entries = int(off[-1])
        self.nbytes = 8 * self.entries + 8 * off.numel()
        self.ascending = int(orbit.sum())
        self.build_ms = float(build_ms)
        self._orbit = orbit.numpy()
        self._off = off.numpy()
        self._hw = np.asarray(self.hw, dtype=np.int64).reshape(-1, 2)

    def orbit_of(self, items, seasons):
        """The orbit of every (item, season) of a batch: a host uint8 array."""
        return self._orbit[np.asarray(items, dtype=np.int64), np.asarray(seasons, dtype=np.int64)].astype(np.uint8)

    def ranges(self, items, seasons):
        """(off, count, item_hw) of a batch's items: host arrays for ``ops.region_patch_apply``."""
        k = np.asarray(items, dtype=np.int64) * self.seasons + np.asarray(seasons, dtype=np.int64)
        return self._off[k], self._off[k + 1] - self._off[k], self._hw[np.asarray(items, dtype=np.int64)]

    def apply(self, items, seasons, s2, s1, hw, params=None):
        """Lay the batch's patches over s2 / s1 (``ops.region_patch_apply``); no launch when the host table shows no entry for the batch."""
        off, count, item_hw = self.ranges(items, seasons)
        if not count.any():
            return 0
        return ops.region_patch_apply(self.idx, self.val, off, count, item_hw, s2, s1, hw, params)


def item_orbit(n_desc, n_asc, numel, ascfill=False, has_asc=True):
    """The orbit of one (item, season) from its census: (0 | 1, ok).  With an ascending raster the rule is ``nanfill.s1_orbit`` /
    ``nanfill.asc_fill`` unchanged (numel = 2 * h * w of the item); ok False where the reference raises "No data here!".  Without one the
    descending orbit is kept and filled at any fraction."""
    from . import nanfill
    if not has_asc or nanfill.s1_orbit(n_desc, numel, ascfill)[0] == "desc":
        return 0, True
    try:
        nanfill.asc_fill(n_asc, numel)
    except Exception as e:                                             # the reference's exception type: told apart by its words
        if str(e) != "No data here!":
            raise
        return 1, False
    return 1, True


def _check_repair(what, repair, plan, seasons):
    if repair is None:
        return
    if repair.n != len(plan) or repair.seasons < int(seasons) or repair.hw != [(int(c[1] - c[0]), int(c[3] - c[2])) for c in plan.crops.tolist()]:
        raise ValueError(f"{what}: repair was planned for another plan (it holds {repair.n} items over {repair.seasons} seasons; the plan "
                         f"has {len(plan)}, the feed draws from {seasons} seasons): pass the plan plan_repair returned")


def plan_repair(region, plan, seasons=1, ascfill=False, pixel_budget=1 << 22):
    """The reference's repair of every weaksup item (data/PopulationDataset.py:419-441), decided once for ``plan`` over seasons [0, seasons):
    returns (plan', RegionRepair).

    Orbit column: ONE census call over all items x seasons (``ops.region_nan_census``) and one synchronisation.  A region with ``s1_asc``
    follows ``nanfill.s1_orbit`` / ``nanfill.asc_fill`` unchanged -- the descending S1 is kept (and filled) below 5 % NaN, in the
    reference's float32 quotient count / numel < 0.05 with numel = 2 * h * w of the item, otherwise (or always where it holds NaN, with
    ``ascfill``) the ascending orbit replaces it under the same rule.  A region without ``s1_asc`` keeps the descending orbit and fills it at
    any fraction, which is what ``--nan_fill`` does on the resident feed; ``ascfill`` then raises ValueError.
    Named deviation: an item for which the reference would raise "No data here!" in ANY of the seasons is dropped -- the reference's run
    would end on that exception; its row of ``plan`` is recorded in ``RegionRepair.dropped``.  plan' keeps the order and the rows of crops,
    census_idx, y, census_n and bbox of the surviving items.

    Patch table: the (item, season) pairs whose census shows a NaN in S2 or in the chosen S1 are grouped by size (``plan_batches`` under
    ``pixel_budget`` pixels per group, a generator of its own), gathered with their orbits, filled on a clone (what ``fill_sample_`` does to
    a batch) and reduced to the entries whose bit pattern changed (``ops.region_patch_extract``: one synchronisation per group, build time
    only).  Items without NaN never reach that pass.  MemoryError, with the byte count, before a table that does not fit is allocated."""
    import time
    S = int(seasons)
    if not 1 <= S <= region.seasons:
        raise ValueError(f"plan_repair: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
    if len(plan) < 1:
        raise ValueError("plan_repair: a plan with at least one crop")
    has_asc = region.s1_asc is not None
    if ascfill and not has_asc:
        raise ValueError("plan_repair: ascfill takes the ascending orbit wherever the descending one holds NaN: the region holds no s1_asc")
    t0 = time.perf_counter()
    n = len(plan)
    orbit, counts, ok, pieces = repair_core(region, plan.crops.numpy(), S, ascfill, pixel_budget)
    alive = ok.all(1).tolist()
    kept = [i for i in range(n) if alive[i]]
    dropped = [i for i in range(n) if not alive[i]]
    if not kept:
        raise ValueError("plan_repair: every item of the plan lacks S1 data in some season (the reference's \"No data here!\")")
    new = plan.subset(kept)
    sel = torch.tensor(kept, dtype=torch.int64)
    orbit, counts = orbit[sel].contiguous(), counts[sel].contiguous()
    m = len(kept)
    hw = [(int(c[1] - c[0]), int(c[3] - c[2])) for c in new.crops.numpy()]
    row = {i: k for k, i in enumerate(kept)}                           # row of the original plan -> row of plan'
    off, idx, val = _assemble_table({row[i] * S + s: pc for (i, s), pc in pieces.items()}, m * S, region.device, "plan_repair",
                                    "plan fewer seasons")
    torch.cuda.synchronize(region.device)
    return new, RegionRepair(orbit, dropped, kept, counts, idx, val, off, hw, build_ms=(time.perf_counter() - t0) * 1e3)


def orbit_column(counts, numel, ascfill=False, has_asc=True):
    """The orbit rule over a census (pure host code): counts = n rows of S triples {S2, descending S1, ascending S1} NaN entries (nested
    lists or a tensor (n, S, 3)), numel = n values 2 * h * w.  Returns (orbit int8 (n, S), ok bool (n, S)): ``item_orbit`` of every pair."""
    cl = counts.tolist() if torch.is_tensor(counts) else counts
    n, S = len(cl), len(cl[0]) if len(cl) else 0
    orbit, ok = torch.zeros(n, S, dtype=torch.int8), torch.ones(n, S, dtype=torch.bool)
    for i in range(n):
        for s in range(S):
            o, good = item_orbit(cl[i][s][1], cl[i][s][2], int(numel[i]), ascfill, has_asc)
            orbit[i, s], ok[i, s] = o, good
    return orbit, ok


def repair_core(region, crops, seasons, ascfill=False, pixel_budget=1 << 22, select=None, no_data=None):
    """What ``plan_repair`` and ``ResidentWindows`` share: over items crops (n, 4) = {x0, x1, y0, y1} (host integers) x seasons [0, seasons)
    ONE census call and one synchronisation, the orbit rule (``orbit_column``), and the patch-table pieces of the pairs that need them.
    Returns (orbit int8 (n, S), counts int64 (n, S, 3), ok bool (n, S), pieces {(i, s): (idx, val)}).
    ok is False where the reference raises "No data here!"; ``no_data`` (a callable) is handed the list of those (i, s) and the counts
    before any table work -- what it raises ends the call --, and an item with such a season gets no pieces (under ``select``: a pair without data gets none, the item's other seasons keep theirs).  Pieces: the (i, s) whose census shows a NaN in S2
    or in the chosen S1, and for which ``select(i, s)`` holds where it is given, are grouped by size (``plan_batches`` under ``pixel_budget``
    pixels per group, a generator of its own; an item at or above the budget is a group of one), gathered with their orbits, filled on a
    clone and reduced to the entries whose bit pattern changed (``ops.region_patch_extract``: one synchronisation per group)."""
    S = int(seasons)
    has_asc = region.s1_asc is not None
    crops = np.asarray(crops, dtype=np.int64).reshape(-1, 4)
    n = crops.shape[0]
    boxes = np.empty((n, S, 5), dtype=np.int64)
    boxes[:, :, :4] = crops[:, None, :]
    boxes[:, :, 4] = np.arange(S)[None, :]
    counts = ops.region_nan_census(region.s2, region.s1, region.boundary, region.band_sel, boxes.reshape(-1, 5),
                                   s1_asc=region.s1_asc).cpu().reshape(n, S, 3)         # the one synchronisation of the orbit column
    hw = [(int(c[1] - c[0]), int(c[3] - c[2])) for c in crops]
    orbit, ok = orbit_column(counts, [2 * h * w for h, w in hw], ascfill, has_asc)
    if no_data is not None and not bool(ok.all()):
        no_data([(int(i), int(s)) for i, s in torch.nonzero(~ok).tolist()], counts)
    # an item lacking data in ANY season gets no pieces; under ``select`` only the selected pairs count, each on its own season
    alive = ok.all(1)[:, None] if select is None else ok
    # the (item, season) pairs that need patches: a NaN in S2 or in the chosen S1
    chosen = torch.where(orbit == 1, counts[:, :, 2], counts[:, :, 1])
    pairs = [(i, s) for i, s in torch.nonzero(((counts[:, :, 0] > 0) | (chosen > 0)) & alive).tolist()
             if select is None or select(i, s)]
    pieces = {}
    if pairs:
        groups = plan_batches([hw[i] for i, _ in pairs], list(range(len(pairs))), int(pixel_budget), PC_GATHER_MAX_B, 0.6,
                              torch.Generator().manual_seed(0))
        for grp in groups:
            gc = np.array([list(crops[pairs[p][0]]) + [pairs[p][1]] for p in grp], dtype=np.int64)
            go = np.array([int(orbit[pairs[p][0], pairs[p][1]]) for p in grp], dtype=np.uint8)
            gathered = region.gather(gc, orbit=go) if has_asc else region.gather(gc)
            filled = {"S2": gathered["S2"].clone(), "S1": gathered["S1"].clone()}
            ops.nan_fill_(filled["S2"], gathered["data_hw"])           # cli.fill_sample_ on the clone
            ops.nan_fill_(filled["S1"], gathered["data_hw"])
            idx, val, per_item = ops.region_patch_extract(gathered, filled)
            sizes = per_item.tolist()
            for p, pi, pv in zip(grp, idx.split(sizes), val.split(sizes)):
                pieces[tuple(pairs[p])] = (pi, pv)
    return orbit, counts, ok, pieces


def _assemble_table(pieces, slots, dev, who, hint):
    """pieces {slot: (idx, val)} -> (off int64 (slots + 1) on the host, idx int32, val fp32 on the device): the pieces in slot order.
    MemoryError, with the byte count, before a table that does not fit is allocated."""
    off = torch.zeros(slots + 1, dtype=torch.int64)
    order = sorted(pieces)
    for k in order:
        off[k + 1] = pieces[k][0].numel()
    off = torch.cumsum(off, 0)
    total = int(off[-1])
    if total:
        free, _ = torch.cuda.mem_get_info(dev)
        if 8 * total > free:
            raise MemoryError(f"{who}: the patch table takes {8 * total} bytes ({total} entries), device {dev} has {free} free: {hint}")
        idx = torch.cat([pieces[k][0] for k in order])
        val = torch.cat([pieces[k][1] for k in order])
    else:
        idx = torch.empty(0, dtype=torch.int32, device=dev)
        val = torch.empty(0, dtype=torch.float32, device=dev)
    return off, idx, val


def window_orbits(counts, windows, ps, ascfill=False, has_asc=True):
    """The orbit column of an evaluation's window list from its census (pure host code): counts = per window its triple {S2, descending
    S1, ascending S1} NaN entries, windows = rows (x, y, season), ps the window side.  Returns int8 (n,): ``item_orbit`` with numel =
    2 * ps * ps.  A window for which the reference raises "No data here!" (PopulationDataset.py:498-500) raises ValueError naming it."""
    cl = counts.tolist() if torch.is_tensor(counts) else list(counts)
    wl = windows.tolist() if torch.is_tensor(windows) else [list(v) for v in windows]
    if len(cl) != len(wl):
        raise ValueError(f"window_orbits: one census triple per window, got {len(cl)} for {len(wl)} windows")
    orbit, ok = orbit_column([[c] for c in cl], [2 * int(ps) * int(ps)] * len(cl), ascfill, has_asc)
    bad = torch.nonzero(~ok[:, 0]).reshape(-1).tolist() if len(cl) else []
    if bad:
        raise _no_data_error(wl[bad[0]], cl[bad[0]], ps, len(bad))
    return orbit[:, 0].contiguous() if len(cl) else torch.zeros(0, dtype=torch.int8)


def _no_data_error(window, triple, ps, how_many):
    x, y, s = (int(v) for v in window)
    return ValueError(f"ResidentWindows: no S1 data in window (x, y, season) = ({x}, {y}, {s}) of side {ps}: {int(triple[1])} NaN entries in "
                      f"the descending and {int(triple[2])} in the ascending orbit of {2 * int(ps) * int(ps)}, both at or above 5 % (the "
                      f"reference's \"No data here!\"; {how_many} such window(s))")


def _finish_plan(plan, pieces, n, what, hint):
    """The tail of ``ResidentWindows``' and ``ResidentItems``' constructors, once ``plan.orbit`` stands: the patch table of its n crops
    from the pieces (``_assemble_table``), the host copies ``_off`` / ``_orbit`` its launches index, and the figures it reports."""
    dev = plan.region.device
    plan.off, plan.table_idx, plan.table_val = _assemble_table(pieces, n, dev, what, hint)
    torch.cuda.synchronize(dev)
    plan._off = plan.off.tolist()
    plan._orbit = plan.orbit.tolist()
    plan.entries = int(plan.off[-1])
    plan.nbytes = 8 * plan.entries
    plan.ascending = int(plan.orbit.sum())


class ResidentWindows:
    """The sliding windows of an evaluation over a ``ResidentRegion``, planned ONCE: the raster callable ``eval.evaluate_raster`` takes
    (``.shape`` = (h, w), ``self(x, y, season, ps)`` -> the normalised model input (1, 6, ps, ps) on the device), so that
    ``evaluate_raster(models, ResidentWindows(region, ps, overlap, ...), ps, overlap, fourseasons, ...)`` returns the bits of
    ``evaluate_raster(models, raster, ..., raw=True, ascfill=...)`` without a per-window fill, clone, concatenation or synchronisation.

    Construction: the window list is ``eval.get_patch_indices(h, w, patchsize, overlap, fourseasons)``; ONE ``region_nan_census`` over all
    windows on every rank (the one synchronisation of the orbit column) decides each window's S1 orbit by the reference's rule for test
    windows (PopulationDataset.py:479-500 = ``nanfill.fill_item_``; ``window_orbits``).  A window for which the reference raises "No data
    here!" raises ValueError naming (x, y, season) -- on every rank alike, since every rank sees the same census, so no rank enters a
    collective another never reaches.  A region without ``s1_asc`` keeps the descending orbit and fills it at any fraction; ``ascfill`` then
    raises.  The patch table (``repair_core``) is built only for the windows of ``shard_indices(n, rank, world)``; MemoryError with the byte
    count before a table that does not fit is allocated.
    Attributes: idx int64 (n, 3) the window list, orbit int8 (n,) (0 descending, 1 ascending), counts int64 (n, 3) the census, mine (the
    window numbers of this rank), off int64 (n + 1) / table_idx int32 / table_val fp32 the patch table (window k: [off[k], off[k + 1])),
    entries, nbytes (table bytes on the device), ascending (windows on the ascending orbit), build_ms.
    ``__call__``: one ``ops.region_window`` launch, no synchronisation; a window that is not planned, another ps or a window of another
    rank raises ValueError."""

    def __init__(self, region, patchsize, overlap, fourseasons=False, ascfill=False, rank=0, world=1, mean6=stats.MEAN6, std6=stats.STD6):
        import time
        from .. import eval as E
        from ..distributed import shard_indices
        self.region, self.patchsize, self.overlap = region, int(patchsize), int(overlap)
        self.fourseasons, self.ascfill, self.rank, self.world = bool(fourseasons), bool(ascfill), int(rank), max(1, int(world))
        self.mean6, self.std6 = tuple(float(v) for v in mean6), tuple(float(v) for v in std6)
        self.shape = tuple(region.shape)
        h, w = self.shape
        ps = self.patchsize
        S = 4 if self.fourseasons else 1
        E.require_raster_fits(h, w, ps, "ResidentWindows")
        if not 1 <= ps or not 0 <= self.overlap or 2 * self.overlap >= ps:
            raise ValueError(f"ResidentWindows: 1 <= patchsize and 0 <= 2 * overlap < patchsize, got patchsize {patchsize}, overlap "
                             f"{overlap}")
        if region.seasons < S:
            raise ValueError(f"ResidentWindows: fourseasons evaluates seasons 0 .. 3, the region holds {region.seasons}")
        if not 0 <= self.rank < self.world:
            raise ValueError(f"ResidentWindows: rank in [0, {self.world}), got {rank}")
        has_asc = region.s1_asc is not None
        if self.ascfill and not has_asc:
            raise ValueError("ResidentWindows: ascfill takes the ascending orbit wherever the descending one holds NaN: the region holds no "
                             "s1_asc")
        t0 = time.perf_counter()
        self.idx = E.get_patch_indices(h, w, ps, self.overlap, self.fourseasons)
        wl = self.idx.tolist()
        n = len(wl)
        # the list is origins x seasons: the census runs over the distinct origins and all S seasons at once
        item = {}
        for x, y, _ in wl:
            item.setdefault((x, y), len(item))
        crops = np.array([[x, x + ps, y, y + ps] for x, y in item], dtype=np.int64).reshape(-1, 4)
        self._at = {}
        for k, (x, y, s) in enumerate(wl):
            self._at.setdefault((x, y, s), k)
        self.mine = list(shard_indices(n, self.rank, self.world))
        rows = [(item[(x, y)], s) for x, y, s in wl]                      # window k -> (origin, season) of the census
        mine = {rows[k] for k in self.mine}

        def no_data(bad, counts):
            lacking = set(bad)
            first = min(k for k in range(n) if rows[k] in lacking)
            raise _no_data_error(wl[first], counts[rows[first][0], rows[first][1]].tolist(), ps, len(bad))

        orbit, counts, ok, pieces = repair_core(region, crops, S, self.ascfill, select=lambda i, s: (i, s) in mine, no_data=no_data)
        self.orbit = torch.tensor([int(orbit[i, s]) for i, s in rows], dtype=torch.int8)
        self.counts = torch.stack([counts[i, s] for i, s in rows]) if n else torch.zeros(0, 3, dtype=torch.int64)
        slot = {}
        for k in self.mine:
            slot.setdefault(rows[k], k)
        self._mine = set(self.mine)
        _finish_plan(self, {slot[key]: pc for key, pc in pieces.items()}, n, "ResidentWindows",
                     "evaluate fewer seasons or shard over more ranks")
        self.window_buildings = None                                     # building_counts (1, 1, ps, ps) of the last window (a region with a layer)
        self.build_ms = (time.perf_counter() - t0) * 1e3

    def __call__(self, x, y, season, ps):
        k = self._at.get((int(x), int(y), int(season)))
        if int(ps) != self.patchsize or k is None:
            raise ValueError(f"ResidentWindows: window (x, y, season) = ({x}, {y}, {season}) of side {ps} is not planned: the plan holds "
                             f"{len(self._at)} windows of side {self.patchsize}, overlap {self.overlap}")
        if k not in self._mine:
            raise ValueError(f"ResidentWindows: window {k} = ({x}, {y}, {season}) belongs to rank {k % self.world}, this feed was planned "
                             f"for rank {self.rank} of {self.world} and holds no patches for it")
        r = self.region
        start = self._off[k]
        kw = {} if r.buildings is None else {"buildings": r.buildings}
        got = ops.region_window(r.s2, r.s1, r.band_sel, (x, y, season), self.patchsize, self.mean6, self.std6, s1_asc=r.s1_asc,
                                orbit=self._orbit[k], table=(self.table_idx, self.table_val, start, self._off[k + 1] - start), **kw)
        if r.buildings is None:
            return got
        # the plane of the window just produced, from the same launch: ``evaluate_raster`` reads it through ``window_buildings``
        self.window_buildings = got[1]
        return got[0]


class ResidentItems:
    """The validation set of a ``RegionPlan`` over a ``ResidentRegion``, planned ONCE: iterating yields one item at a time in the form
    ``model(sample, padding=False)`` takes -- {"input" (1, 6, hc, wc), "admin_mask" (1, hc, wc), "census_idx", "y"} ((1,) each for a one-unit
    plan; (1, K) plus the host list ``census_n`` = [K] for a multi-unit plan, K = the item's listed units) --, each item ONE
    ``ops.region_item`` launch: no clone, no concatenation, no fill and no synchronisation after construction.  By definition, bit for bit:

        item == normalize_sample(region.gather([crop + season], orbit=[orbit]), transform=None, nan_fill=True)

    Construction: the season of every item is drawn ONCE -- ``torch.randint(0, seasons, (n,))`` from ``generator``, all zero for seasons ==
    1.  Named deviation: the reference draws a fresh season from Python's ``random`` at every validation (PopulationDataset.py:409), so its
    validation sets differ from epoch to epoch; here every validation sees the same (item, season) list and its metrics are comparable.
    ``repair_core`` over the plan's crops, restricted to each item's own season, gives the orbit (one census call, one synchronisation; the
    rule of ``plan_repair``) and the patch pieces.  An item whose own season would make the reference raise "No data here!" is dropped and
    its row of the ORIGINAL plan recorded in ``dropped`` -- the named deviation of ``plan_repair``.  MemoryError with the byte count before a
    table that does not fit is allocated.
    Attributes: plan (the surviving items, in order), season int64 (m,) and orbit int8 (m,) of the surviving items, counts int64 (m, 3)
    their census, off int64 (m + 1) / table_idx int32 / table_val fp32 the patch table (item k: [off[k], off[k + 1])), entries, nbytes
    (table bytes on the device), ascending (items on the ascending orbit), build_ms, dropped."""

    def __init__(self, region, plan, seasons=1, generator=None, ascfill=False, mean6=stats.MEAN6, std6=stats.STD6):
        import time
        S = int(seasons)
        if not 1 <= S <= region.seasons:
            raise ValueError(f"ResidentItems: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
        if len(plan) < 1:
            raise ValueError("ResidentItems: a plan with at least one crop")
        if ascfill and region.s1_asc is None:
            raise ValueError("ResidentItems: ascfill takes the ascending orbit wherever the descending one holds NaN: the region holds no "
                             "s1_asc")
        t0 = time.perf_counter()
        self.region, self.seasons, self.ascfill = region, S, bool(ascfill)
        self.mean6, self.std6 = tuple(float(v) for v in mean6), tuple(float(v) for v in std6)
        n = len(plan)
        gen = generator if generator is not None else torch.Generator().manual_seed(0)
        drawn = torch.randint(0, S, (n,), generator=gen) if S > 1 else torch.zeros(n, dtype=torch.int64)
        own = drawn.tolist()
        orbit, counts, ok, pieces = repair_core(region, plan.crops.numpy(), S, self.ascfill, select=lambda i, s: s == own[i])
        kept = [i for i in range(n) if bool(ok[i, own[i]])]
        self.dropped = [i for i in range(n) if not bool(ok[i, own[i]])]
        if not kept:
            raise ValueError("ResidentItems: every item of the plan lacks S1 data in its season (the reference's \"No data here!\")")
        self.plan = plan.subset(kept)
        m = len(kept)
        self.season = drawn[torch.tensor(kept, dtype=torch.int64)].contiguous()
        self.orbit = torch.tensor([int(orbit[i, own[i]]) for i in kept], dtype=torch.int8)
        self.counts = torch.stack([counts[i, own[i]] for i in kept])
        row = {i: k for k, i in enumerate(kept)}
        # the plan tables, uploaded once: an item's labels are views of them
        self._cidx = self.plan.census_idx.to(region.device).contiguous()
        self._y = self.plan.y.to(region.device).float().contiguous()
        self._crops = [tuple(int(v) for v in c) + (int(s),) for c, s in zip(self.plan.crops.tolist(), self.season.tolist())]
        _finish_plan(self, {row[i]: pc for (i, s), pc in pieces.items() if i in row}, m, "ResidentItems", "validate fewer items")
        self.build_ms = (time.perf_counter() - t0) * 1e3

    def __len__(self):
        return len(self.plan)

    def item(self, k):
        """Item k: one ``ops.region_item`` launch."""
        r, plan = self.region, self.plan
        start = self._off[k]
        kw = {} if r.buildings is None else {"buildings": r.buildings}
        got = ops.region_item(r.s2, r.s1, r.boundary, r.band_sel, self._crops[k], self.mean6, self.std6, s1_asc=r.s1_asc,
                              orbit=self._orbit[k], table=(self.table_idx, self.table_val, start, self._off[k + 1] - start), **kw)
        x, admin = got[0], got[1]
        layer = {} if r.buildings is None else {"building_counts": got[2]}     # (1, 1, hc, wc), from the same launch
        if plan.multi:
            K = plan.census_n[k]
            return {"input": x, "admin_mask": admin, "census_idx": self._cidx[k:k + 1, :K], "y": self._y[k:k + 1, :K], "census_n": [K],
                    **layer}
        return {"input": x, "admin_mask": admin, "census_idx": self._cidx[k, :1], "y": self._y[k, :1], **layer}

    def __iter__(self):
        for k in range(len(self.plan)):
            yield self.item(k)


class ResidentRegionFeed:
    """Batches of a ``RegionPlan`` over a ``ResidentRegion``, iterated like ``feed.RegionFeed``:

        for sample in ResidentRegionFeed(region, plan, batch_size, generator):
            trainer.train_step(sample)

    Each batch is one ``ops.region_gather`` launch; the crop list travels in its kernel arguments and ``y`` / ``census_idx`` are indexed on
    the device from tables uploaded once, so a batch costs no host-to-device copy and no synchronisation.  The dicts carry the plain
    collate's keys -- S2 (B, 4, Hm, Wm) and S1 (B, 2, Hm, Wm) fp32, admin_mask, y, census_idx, data_hw, img_coords, valid_coords, season --
    and for a multi-unit plan ``collate_units``' form: census_idx / y as (B, K) padded with -1 / 0 (K = the batch maximum) plus the host
    list census_n.  All tensors are on the device, so ``Trainer.train_step`` -> ``prepare_sample_fused`` takes them as they are.
    Order: each epoch (each ``__iter__``) takes ONE ``torch.randperm`` from ``generator``, then (seasons > 1) one ``torch.randint`` for the
    season of every item of the epoch; ``last_order`` / ``last_season`` (host) record them.  Parity with the reference's shuffling sampler
    and its Python ``random.choice`` of the season (PopulationDataset.py:409) is not claimed.
    There is no producer thread: ``pause()`` returns a null context, so ``FusedTrainStep.capture_guard`` keeps working."""

    def __init__(self, region, plan, batch_size, generator=None, drop_last=True, seasons=1, repair=None):
        if len(plan) < 1 or int(batch_size) < 1:
            raise ValueError("ResidentRegionFeed: a plan with at least one crop and batch_size >= 1")
        if not 1 <= int(seasons) <= region.seasons:
            raise ValueError(f"ResidentRegionFeed: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
        _check_repair("ResidentRegionFeed", repair, plan, seasons)
        self.repair = repair
        self.region, self.plan, self.batch_size, self.drop_last, self.seasons = region, plan, int(batch_size), bool(drop_last), int(seasons)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)
        self.device = region.device
        self._cidx = plan.census_idx.to(self.device)
        self._y = plan.y.to(self.device)
        self._crops = plan.crops.numpy()
        self._bbox = plan.bbox.tolist()
        self.last_order = self.last_season = None

    def pause(self):
        return contextlib.nullcontext()

    def __len__(self):
        n, B = len(self.plan), self.batch_size
        return n // B if self.drop_last else -(-n // B)

    def _gather(self, idx, crops, orbit=None):
        """The gather launch of plan rows ``idx`` (what a feed over several regions, data/atlas.py, replaces)."""
        return self.region.gather(crops) if orbit is None else self.region.gather(crops, orbit=orbit)

    def __iter__(self):
        plan, B, n = self.plan, self.batch_size, len(self.plan)
        order = torch.randperm(n, generator=self.generator)
        season = (torch.randint(0, self.seasons, (n,), generator=self.generator) if self.seasons > 1
                  else torch.zeros(n, dtype=torch.int64))
        self.last_order, self.last_season = order, season
        order_dev, season_dev = order.to(self.device), season.to(self.device)      # one upload per epoch
        order_np, season_np = order.numpy(), season.numpy()
        for k in range(len(self)):
            idx = order_np[k * B:(k + 1) * B]
            sel = order_dev[k * B:(k + 1) * B]
            crops = np.empty((idx.size, 5), dtype=np.int64)
            crops[:, :4] = self._crops[idx]
            crops[:, 4] = season_np[k * B:(k + 1) * B]
            if self.repair is None:
                out = self._gather(idx, crops)
            else:
                # the plan's orbit column, then the batch's patches: one small launch behind the gather, none for a batch without entries
                orbit = self.repair.orbit_of(idx, crops[:, 4])
                out = self._gather(idx, crops, orbit)
                self.repair.apply(idx, crops[:, 4], out["S2"], out["S1"], tuple(out["admin_mask"].shape[1:]))
                out["orbit"] = orbit.tolist()
            if plan.multi:
                cn = [plan.census_n[i] for i in idx]
                K = max(cn)
                out["census_idx"] = self._cidx[sel][:, :K].contiguous()
                out["y"] = self._y[sel][:, :K].contiguous()
                out["census_n"] = cn
            else:
                out["census_idx"] = self._cidx[sel, 0]
                out["y"] = self._y[sel, 0]
            boxes = [self._bbox[i] for i in idx]
            out["img_coords"] = [(b[0], b[2]) for b in boxes]
            out["valid_coords"] = [tuple(b) for b in boxes]
            out["season"] = season_dev[k * B:(k + 1) * B]
            yield out


def plan_batches(hw_list, order, pixel_budget, max_batch, min_fill, generator):
    """The batches of one epoch under a pixel budget (pure host code): ``hw_list[i]`` = (h, w) of plan item i, ``order`` = the epoch's
    permutation of the items.  Returns a list of lists of item indices.
    Rule: the permuted items are sorted by the size class floor(8 * log2(h * w)), ties by their position in the permutation (so batches of
    similar items differ from epoch to epoch); a sweep over the sorted list lets an item join the open batch of B items while B + 1 <=
    max_batch, (B + 1) * Hm' * Wm' <= pixel_budget and the real pixels are >= min_fill * the padded ones -- (Hm', Wm') the maximum with
    the item included --, and otherwise opens a new batch with it; one ``torch.randperm`` from ``generator`` then shuffles the batches.
    Invariants: (a) every item is in exactly one batch, nothing is dropped; (b) a batch with B > 1 has B * Hm * Wm <= pixel_budget (an
    item that alone exceeds the budget is a batch of one); (c) B <= max_batch; (d) a batch with B > 1 has fill >= min_fill; (e) the
    result is a function of the arguments and the generator's state alone; (f) two epochs (two permutations) give different
    compositions when a size class holds at least two items that do not share a batch."""
    import math
    if int(max_batch) < 1 or int(pixel_budget) < 1 or not 0.0 <= float(min_fill) <= 1.0:
        raise ValueError(f"plan_batches: pixel_budget >= 1, max_batch >= 1 and min_fill in [0, 1], got {pixel_budget}, {max_batch}, {min_fill}")
    order = [int(i) for i in (order.tolist() if torch.is_tensor(order) else order)]
    hw = [(int(h), int(w)) for h, w in hw_list]
    if sorted(order) != list(range(len(hw))) or any(h < 1 or w < 1 for h, w in hw):
        raise ValueError("plan_batches: order is a permutation of the items of hw_list, every item non-empty")
    keyed = sorted(range(len(order)), key=lambda p: (math.floor(8.0 * math.log2(hw[order[p]][0] * hw[order[p]][1])), p))
    batches, cur, Hm, Wm, real = [], [], 0, 0, 0
    for p in keyed:
        i = order[p]
        h, w = hw[i]
        if cur:
            H2, W2, n2 = max(Hm, h), max(Wm, w), len(cur) + 1
            padded = n2 * H2 * W2
            if n2 <= max_batch and padded <= pixel_budget and real + h * w >= min_fill * padded:
                cur.append(i)
                Hm, Wm, real = H2, W2, real + h * w
                continue
            batches.append(cur)
        cur, Hm, Wm, real = [i], h, w, h * w
    if cur:
        batches.append(cur)
    shuffle = torch.randperm(len(batches), generator=generator).tolist()
    return [batches[k] for k in shuffle]


class ResidentBatchFeed:
    """``ResidentRegionFeed`` with the whole batch assembled in ONE launch: per batch one ``ops.region_batch`` call -- gather, augmentation,
    raw-tile assembly and the y / census_idx rows of the plan tables -- and no other device work.  Yields what the fused step takes:
    {"raw" (B, 6, Ho, Wo), "admin_mask" (B, Ho, Wo), "census_idx", "y", ["census_n"], "img_coords", "valid_coords", "season"}; census_idx / y
    are (B,) for a one-unit plan and (B, K) padded with -1 / 0 (K = the batch maximum) plus host ``census_n`` for a multi-unit plan.
    Order: the epoch's ``randperm`` / ``randint`` come from ``generator`` as in ``ResidentRegionFeed``; the augmentation coins are drawn with
    ``draw_fused_params(transform)`` once per batch, immediately before the batch is yielded, so the global generators see the sequence
    ``Trainer.train_step`` consumes with the unfused feed: coins, then the step's selection draw.  A transform that ``draw_fused_params``
    cannot express raises ValueError here (the global generators are left as they were).
    pixel_budget > 0: batches are composed by size with ``plan_batches`` (one more ``randperm`` per epoch, after the two above) instead of
    cut at ``batch_size``; nothing is dropped.  Variable batch sizes change the optimisation schedule: this is not the reference recipe."""

    def __init__(self, region, plan, batch_size, transform=None, generator=None, drop_last=True, seasons=1, pixel_budget=0, max_batch=128,
                 min_fill=0.6, repair=None):
        import random
        from ..utils.transform import draw_fused_params
        if len(plan) < 1 or int(batch_size) < 1:
            raise ValueError("ResidentBatchFeed: a plan with at least one crop and batch_size >= 1")
        if not 1 <= int(seasons) <= region.seasons:
            raise ValueError(f"ResidentBatchFeed: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
        if int(pixel_budget) < 0 or int(max_batch) < 1 or not 0.0 <= float(min_fill) <= 1.0:
            raise ValueError(f"ResidentBatchFeed: pixel_budget >= 0, max_batch >= 1, min_fill in [0, 1]; got {pixel_budget}, {max_batch}, "
                             f"{min_fill}")
        _check_repair("ResidentBatchFeed", repair, plan, seasons)
        self.repair = repair
        state = torch.get_rng_state(), random.getstate()
        expressible = draw_fused_params(transform) is not None
        torch.set_rng_state(state[0])
        random.setstate(state[1])
        if not expressible:
            raise ValueError("ResidentBatchFeed: the transform is not one draw_fused_params can express (one coin per batch, the reference "
                             "trainer's brightness / gamma / flips / quarter turns); use ResidentRegionFeed with it")
        self._draw = draw_fused_params
        self.region, self.plan, self.batch_size, self.drop_last, self.seasons = region, plan, int(batch_size), bool(drop_last), int(seasons)
        self.transform = transform
        self.pixel_budget, self.max_batch, self.min_fill = int(pixel_budget), int(max_batch), float(min_fill)
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)
        self.device = region.device
        self._cidx = plan.census_idx.to(self.device).contiguous()       # the plan tables, uploaded once
        self._y = plan.y.to(self.device).float().contiguous()
        self._crops = plan.crops.numpy()
        self._hw = [(int(c[1] - c[0]), int(c[3] - c[2])) for c in self._crops]
        self._bbox = plan.bbox.tolist()
        self.last_order = self.last_season = self.last_batches = None

    def pause(self):
        return contextlib.nullcontext()

    def __len__(self):
        if self.pixel_budget > 0:
            if self.last_batches is None:
                raise TypeError("ResidentBatchFeed: under a pixel budget the number of batches is known once an epoch is planned")
            return len(self.last_batches)
        n, B = len(self.plan), self.batch_size
        return n // B if self.drop_last else -(-n // B)

    def _assemble(self, idx, crops, params, labels, orbit=None):
        """The assembly launch of plan rows ``idx`` (what a feed over several regions, data/atlas.py, replaces)."""
        r = self.region
        kw = {} if r.buildings is None else {"buildings": r.buildings}     # "building_counts", same launch
        if orbit is None:
            return ops.region_batch(r.s2, r.s1, r.boundary, r.band_sel, crops, params, labels=labels, **kw)
        return ops.region_batch(r.s2, r.s1, r.boundary, r.band_sel, crops, params, labels=labels, s1_asc=r.s1_asc, orbit=orbit, **kw)

    def __iter__(self):
        plan, B, n = self.plan, self.batch_size, len(self.plan)
        order = torch.randperm(n, generator=self.generator)
        season = (torch.randint(0, self.seasons, (n,), generator=self.generator) if self.seasons > 1
                  else torch.zeros(n, dtype=torch.int64))
        self.last_order, self.last_season = order, season
        order_np, season_np = order.numpy(), season.numpy()
        if self.pixel_budget > 0:
            pos = np.empty(n, dtype=np.int64)
            pos[order_np] = np.arange(n)                               # the season of an item is drawn at its place in the permutation
            batches = [np.asarray(b, dtype=np.int64) for b in
                       plan_batches(self._hw, order_np, self.pixel_budget, self.max_batch, self.min_fill, self.generator)]
            seasons = [season_np[pos[b]] for b in batches]
        else:
            batches = [order_np[k * B:(k + 1) * B] for k in range(len(self))]
            seasons = [season_np[k * B:(k + 1) * B] for k in range(len(self))]
        self.last_batches = [b.tolist() for b in batches]
        season_dev = torch.from_numpy(np.concatenate(seasons)).to(self.device) if batches else None      # one upload per epoch
        at = 0
        for idx, sea in zip(batches, seasons):
            crops = np.empty((idx.size, 5), dtype=np.int64)
            crops[:, :4] = self._crops[idx]
            crops[:, 4] = sea
            cn = [plan.census_n[i] for i in idx] if plan.multi else None
            params = self._draw(self.transform)                        # the coins, immediately before the batch goes out
            labels = (self._cidx, self._y, idx, max(cn) if plan.multi else 1)
            if self.repair is None:
                out = self._assemble(idx, crops, params, labels)
            else:
                # the plan's orbit column, then the batch's patches through the same coins: one small launch behind the assembly
                orbit = self.repair.orbit_of(idx, sea)
                out = self._assemble(idx, crops, params, labels, orbit)
                tile = (max(self._hw[i][0] for i in idx), max(self._hw[i][1] for i in idx))
                self.repair.apply(idx, sea, out["raw"][:, :4], out["raw"][:, 4:], tile, params)
                out["orbit"] = orbit.tolist()
            if plan.multi:
                out["census_n"] = cn
            else:
                out["census_idx"], out["y"] = out["census_idx"].view(-1), out["y"].view(-1)
            boxes = [self._bbox[i] for i in idx]
            out["img_coords"] = [(b[0], b[2]) for b in boxes]
            out["valid_coords"] = [tuple(b) for b in boxes]
            out["season"] = season_dev[at:at + idx.size]
            at += idx.size
            yield out
