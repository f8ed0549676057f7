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

Host glue, plain torch; the kernels are csrc/region.hip and csrc/region_batch.hip.  Deviations from the reference, all named where they happen: units without pixels
are dropped (``plan_one_unit``); the per-epoch order and the season per item come from a torch generator, not Python's ``random`` stream
(``ResidentRegionFeed``); the resident S1 is the orbit already chosen per season (no switch by NaN fraction: ``--nan_fill`` fills what is
left).  Sharding a plan over data-parallel ranks and graph capture of the gather are not part of this module."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from .. import ops

REFERENCE_BANDS = (2, 1, 0, 3, 0, 1)      # file bands (3, 2, 1, 4) of S2 and (1, 2) of S1, 1-based (PopulationDataset.py:566-568), 0-based
MODEL_ORDER_BANDS = (0, 1, 2, 3, 0, 1)    # rasters whose bands are stored in the model's order already (SyntheticTestRaster)
MAX_PIX, MAX_PIX_BOX = 10_000_000, 12_000_000      # the reference's defaults (PopulationDataset.py:124-131)


class ResidentRegion:
    """The rasters of one region on the device: s2 (S, C2, h, w) fp32 or uint16 digital numbers, s1 fp32 (S, C1, h, w), boundary int32
    (h, w) of census-unit ids, and the census table (census_idx (n,) ids, census_pop (n,) counts; host).  ``table`` (host int32
    (num_ids, 5) = {xmin, xmax, ymin, ymax, count}, the reference's convention) is computed once on the device.  Raises when the boundary
    holds ids outside [0, num_ids) (num_ids defaults to the largest census id + 1) and when the tensors that still have to move do not
    fit the device's free memory."""

    def __init__(self, s2, s1, boundary, census_idx, census_pop, band_sel=REFERENCE_BANDS, device=None, num_ids=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"ResidentRegion: the region lives on a HIP device, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        need = sum(t.numel() * t.element_size() for t in (s2, s1, boundary) if t.device != dev)
        if need:
            free, total = torch.cuda.mem_get_info(dev)
            if need > free:
                raise MemoryError(f"ResidentRegion: the rasters take {need / 2 ** 30:.2f} GiB, device {dev} has {free / 2 ** 30:.2f} GiB free "
                                  f"of {total / 2 ** 30:.2f}: keep fewer seasons resident or store S2 as uint16")
        self.s2 = s2.to(dev).contiguous()
        self.s1 = s1.to(dev).float().contiguous()
        self.boundary = boundary.to(dev).to(torch.int32).contiguous()
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
    def from_synthetic(cls, data, device=None):
        """From a ``SyntheticTestRaster(raw=True, ...)``: its S2 / S1 / boundary / census table, bands in the model's order."""
        if not getattr(data, "raw", False):
            raise ValueError("ResidentRegion.from_synthetic: a SyntheticTestRaster(raw=True)")
        return cls(data.s2, data.s1, data.boundary, data.census_idx, data.census_pop, band_sel=MODEL_ORDER_BANDS,
                   device=data.s2.device if data.s2.is_cuda and device is None else device)

    def gather(self, crops, out=None):
        """``ops.region_gather`` of host crops (B, 5) = {x0, x1, y0, y1, season} on this region."""
        return ops.region_gather(self.s2, self.s1, self.boundary, self.band_sel, crops, out=out)


class RegionPlan:
    """n crops over a region: crops int64 (n, 4) = {x0, x1, y0, y1} (rows [x0, x1), columns [y0, y1)), the listed units census_idx int64
    (n, K) padded with -1, their counts y fp32 (n, K) padded with 0, census_n (n ints: listed units per crop), bbox int64 (n, 4): the union
    bounding box of the listed units (the item's ``valid_coords``), multi: the batch form (``collate_units``' or the plain collate's)."""

    def __init__(self, crops, census_idx, y, census_n, bbox, multi):
        self.crops, self.census_idx, self.y, self.census_n, self.bbox, self.multi = crops, census_idx, y, list(census_n), bbox, bool(multi)

    def __len__(self):
        return int(self.crops.shape[0])

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

    def __init__(self, region, plan, batch_size, generator=None, drop_last=True, seasons=1):
        if len(plan) < 1 or int(batch_size) < 1:
            raise ValueError("ResidentRegionFeed: a plan with at least one crop and batch_size >= 1")
        if not 1 <= int(seasons) <= region.seasons:
            raise ValueError(f"ResidentRegionFeed: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
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
            out = self.region.gather(crops)
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
                 min_fill=0.6):
        import random
        from ..utils.transform import draw_fused_params
        if len(plan) < 1 or int(batch_size) < 1:
            raise ValueError("ResidentBatchFeed: a plan with at least one crop and batch_size >= 1")
        if not 1 <= int(seasons) <= region.seasons:
            raise ValueError(f"ResidentBatchFeed: seasons in [1, {region.seasons}] (what the region holds), got {seasons}")
        if int(pixel_budget) < 0 or int(max_batch) < 1 or not 0.0 <= float(min_fill) <= 1.0:
            raise ValueError(f"ResidentBatchFeed: pixel_budget >= 0, max_batch >= 1, min_fill in [0, 1]; got {pixel_budget}, {max_batch}, "
                             f"{min_fill}")
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
            out = ops.region_batch(self.region.s2, self.region.s1, self.region.boundary, self.region.band_sel, crops, params,
                                   labels=(self._cidx, self._y, idx, max(cn) if plan.multi else 1))
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
