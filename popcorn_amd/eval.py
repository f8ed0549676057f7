"""Evaluation counterpart of the reference's ``run_eval.py`` Trainer.test_target (run_eval.py:71-203) and the census
helpers of ``Population_Dataset`` (data/PopulationDataset.py:294-334, 656-672, 675-852):

  sliding windows (2048 px, 128 px overlap, interior-only write-back) over a raster  ->  ensemble forward (HIP)  ->
  device-resident (h,w) accumulators {sum, sum^2, scale sum, scale sum^2, count}  ->  mean / std  ->
  one-pass census aggregation (segment sum)  ->  metrics  ->  dasymetric adjustment  ->  metrics again.

Relative to the reference: the frozen building extractor (identical in every ensemble member, popcorn.py:96) runs ONCE
per window instead of once per member; accumulators never leave the device; the per-census-row Python loop is one
kernel.  Windows are independent, so multi-GPU evaluation shards them round-robin and sum-reduces the accumulators.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .distributed import FlatReducer, shard_indices

INFERENCE_PATCH_SIZE = 2048      # utils/constants.py:12
OVERLAP = 128                    # utils/constants.py:13


def get_patch_indices(h, w, patchsize=INFERENCE_PATCH_SIZE, overlap=OVERLAP, fourseasons=False):
    """(x, y, season) window origins: regular grid of stride patchsize - 2*overlap plus a bottom row, a right column and
    the bottom-right corner, repeated per season.  data/PopulationDataset.py:294-334."""
    stride = patchsize - 2 * overlap
    x = torch.arange(0, h - patchsize, stride, dtype=int)
    y = torch.arange(0, w - patchsize, stride, dtype=int)
    main = torch.cartesian_prod(x, y).reshape(-1, 2)
    max_x, max_y = h - patchsize, w - patchsize
    bottom = torch.stack([torch.full((len(y),), max_x, dtype=int), y]).T
    right = torch.stack([x, torch.full((len(x),), max_y, dtype=int)]).T
    corner = torch.tensor([[max_x, max_y]])
    main = torch.cat([main, bottom, right, corner])
    seasons = range(4) if fourseasons else range(1)
    return torch.cat([torch.cat([main, torch.full((main.shape[0], 1), s, dtype=int)], dim=1) for s in seasons], dim=0)


def require_raster_fits(h, w, patchsize, who):
    """A raster with a side below the patch size is not defined by the reference: its window list (``get_patch_indices``) needs
    ``torch.arange(0, h - patchsize, stride)`` with a negative end -- a RuntimeError in current torch builds, a negative origin (which
    tensor slices wrap silently) where arange tolerates it -- and its loader would read a window at a negative offset
    (data/PopulationDataset.py:294-334, 624-653).  Every consumer of the window list refuses it here by name, before anything is
    allocated or launched."""
    if min(int(h), int(w)) < int(patchsize):
        raise ValueError(f"{who}: a raster of h {int(h)} x w {int(w)} is smaller than patchsize {int(patchsize)}; the sliding windows of "
                         f"the reference are not defined for it (evaluate with a patchsize <= min(h, w))")


def create_mask(patchsize_x, patchsize_y, overlap):
    """Interior of a window (data/PopulationDataset.py:656-672)."""
    m = torch.zeros(patchsize_x, patchsize_y, dtype=torch.bool)
    m[overlap:patchsize_x - overlap, overlap:patchsize_y - overlap] = True
    return m


def count_windows(count, windows, M, ps, overlap=OVERLAP):
    """count[r][c] += M for every window of ``windows`` (iterable of (row origin, column origin)) whose interior covers (r, c), in ONE
    launch of ``census.hip`` (pc_stitch_count_windows).  count: (h, w) int16 device map, rows contiguous."""
    h, w = count.shape
    # interiors {x0, x1, y0, y1} of all windows as ONE small device array; census.hip counts them into the map in one launch.  Clipped at
    # the bottom / right here; a negative origin needs no clamp: the kernel compares every pixel (r, c) of the raster with x0 <= r < x1,
    # y0 <= c < y1, so the part of an interior above / left of the raster matches no pixel (all four sides clip through the comparisons)
    rows = []
    for x, y in windows:
        x, y = int(x), int(y)
        x0, x1 = min(x + overlap, h), min(x + ps - overlap, h)
        y0, y1 = min(y + overlap, w), min(y + ps - overlap, w)
        if x1 > x0 and y1 > y0:
            rows.append((x0, x1, y0, y1))
    if not rows:
        return
    win = torch.tensor(rows, dtype=torch.int32).to(count.device)
    L.check(L.lib().pc_stitch_count_windows(L.ptr(win), len(rows), int(M), L.ptr(count), h, w, L.stream_ptr()),
            "pc_stitch_count_windows")


class Stitcher:
    """Device-resident accumulators of run_eval.py:84-90 and the write-back / averaging of :127-154.

    Multi-GPU (windows sharded over ranks): ``world`` pads the row count to a multiple of the world size so that
    ``reduce_scatter`` can hand every rank the SUM of one equal row band (one ring pass over the four fp32 planes -- half the
    bytes of an all-reduce); the visit-count map is not communicated at all: it depends only on the window list, so every
    rank adds the windows of the OTHER ranks to its own count map (``add_count_only``).  Each rank then finalises its band;
    ``gather_bands`` assembles the full maps where a caller wants them (the census sums do not: ``census_sums`` on the band
    plus one tiny all-reduce of the per-region sums)."""

    def __init__(self, h, w, device, with_scale=True, world=1):
        if torch.device(device).type != "cuda":
            raise L.PopcornHipError("Stitcher accumulates on a HIP device only")
        self.h, self.w, self.world = h, w, max(1, int(world))
        self.hb = -(-h // self.world)                      # rows per rank band
        self.hp = self.hb * self.world                     # padded row count (rows >= h are never written)
        # the fp32 accumulators are planes of ONE allocation
        self.acc = torch.zeros(4 if with_scale else 2, self.hp, w, dtype=torch.float32, device=device)
        self.out, self.out_sq = self.acc[0][:h], self.acc[1][:h]
        self.scale, self.scale_sq = (self.acc[2][:h], self.acc[3][:h]) if with_scale else (None, None)
        self.count = torch.zeros(self.hp, w, dtype=torch.int16, device=device)[:h]
        self.band = None                                   # (row0, row1) once the accumulators hold only this rank's band

    def add_window(self, xl, yl, popdense, scale=None, overlap=OVERLAP):
        """popdense / scale: (M, psx, psy) member outputs of the window whose origin is row xl, column yl (the reference's
        ``img_coords``); psx rows, psy columns.  The interior is clipped to the raster on all four sides: the origin may be negative."""
        L.require_device(popdense)
        M, psx, psy = popdense.shape
        popdense = popdense.contiguous().float()
        scale = scale.contiguous().float() if scale is not None and self.scale is not None else None
        L.check(L.lib().pc_stitch_accumulate(L.ptr(popdense), L.ptr(scale), M, psx, psy, overlap, int(xl), int(yl),
                                             L.ptr(self.out), L.ptr(self.out_sq), L.ptr(self.scale), L.ptr(self.scale_sq),
                                             L.ptr(self.count), self.h, self.w, L.stream_ptr()), "pc_stitch_accumulate")

    def add_count_only(self, xl, yl, M, ps, overlap=OVERLAP):
        """A window another rank computed: only its visit count (interior += M), no data."""
        x0, x1 = max(xl + overlap, 0), min(xl + ps - overlap, self.h)       # (a negative slice start would wrap)
        y0, y1 = max(yl + overlap, 0), min(yl + ps - overlap, self.w)
        if x1 > x0 and y1 > y0:
            self.count[x0:x1, y0:y1] += M

    def add_counts_only(self, windows, M, ps, overlap=OVERLAP):
        """The visit counts of MANY windows other ranks computed, in ONE launch of ``census.hip`` (pc_stitch_count_windows) instead of one
        slice-add per window from the host loop.  windows: iterable of (row origin, column origin)."""
        # (round 6: the difference-array form did this bookkeeping with stock torch ops -- index_put_, two cumsum_, a banded int16
        # conversion -- and a transient int32 plane of the raster's size)
        count_windows(self.count, windows, M, ps, overlap)

    def all_reduce(self, reducer: FlatReducer):
        """Multi-GPU, simple form: sum the full accumulators on every rank (interiors of regular windows are disjoint, the
        bottom/right catch-up windows overlap them -- the count map handles both)."""
        if reducer.active:
            import torch.distributed as dist
            dist.all_reduce(self.acc, group=reducer.group)            # all fp32 planes in one ring pass
            c = self.count.to(torch.int32)                            # RCCL has no 16-bit integer sum
            dist.all_reduce(c, group=reducer.group)
            self.count.copy_(c)

    def reduce_scatter(self, reducer: FlatReducer, rank):
        """Multi-GPU, band form: this rank ends up with the summed accumulators of rows [rank * hb, (rank + 1) * hb) (clipped
        to h) in place; the other rows of its planes are stale afterwards.  The count map must already be complete
        (``add_count_only`` for the other ranks' windows).  Returns (row0, row1)."""
        r0, r1 = min(rank * self.hb, self.h), min((rank + 1) * self.hb, self.h)
        if reducer.active:
            import torch.distributed as dist
            assert reducer.world == self.world, "Stitcher(world=...) must equal the reducer's world size"
            if reducer.backend == "nccl":
                for p in range(self.acc.shape[0]):
                    plane = self.acc[p]                                # (hp, w) contiguous: chunk r = band r
                    dist.reduce_scatter_tensor(plane[rank * self.hb:(rank + 1) * self.hb], plane, group=reducer.group)
            else:
                # gloo (functional runs) has no reduce-scatter on device tensors: all-reduce, then make the result look like one --
                # the rows of the OTHER ranks' bands are poisoned, so anything that reads a stale row after this call (which the
                # RCCL branch leaves unsummed) shows up as NaN in the functional tests instead of passing by accident
                dist.all_reduce(self.acc, group=reducer.group)
                self.acc[:, :rank * self.hb] = float("nan")
                self.acc[:, (rank + 1) * self.hb:] = float("nan")
        self.band = (r0, r1)
        return self.band

    def finalize(self):
        """mean / std where count > 1 (run_eval.py:140-154) over the whole raster, or over this rank's band after
        ``reduce_scatter``.  Returns the four maps (full-raster views; after a reduce_scatter only the band rows are valid)."""
        r0, r1 = self.band if self.band is not None else (0, self.h)
        n = (r1 - r0) * self.w
        if n > 0:
            sl = lambda t: None if t is None else t[r0:r1]  # noqa: E731
            L.check(L.lib().pc_stitch_finalize(L.ptr(sl(self.out)), L.ptr(sl(self.out_sq)), L.ptr(sl(self.scale)),
                                               L.ptr(sl(self.scale_sq)), L.ptr(sl(self.count)), C.c_int64(n), L.stream_ptr()),
                    "pc_stitch_finalize")
        return self.out, self.out_sq, self.scale, self.scale_sq

    def gather_bands(self, reducer: FlatReducer):
        """After reduce_scatter + finalize: every rank receives every band (the full finalised maps)."""
        if reducer.active and self.band is not None:
            import torch.distributed as dist
            for p in range(self.acc.shape[0]):
                plane = self.acc[p]
                if reducer.backend == "nccl":
                    r = dist.get_rank(reducer.group)
                    dist.all_gather_into_tensor(plane, plane[r * self.hb:(r + 1) * self.hb].clone(), group=reducer.group)
                else:
                    parts = [torch.empty(self.hb, self.w, device=plane.device) for _ in range(self.world)]
                    r = dist.get_rank(reducer.group)
                    dist.all_gather(parts, plane[r * self.hb:(r + 1) * self.hb].contiguous(), group=reducer.group)
                    plane.copy_(torch.cat(parts, 0))
        self.band = None
        return self.out, self.out_sq, self.scale, self.scale_sq


def product_shape(h, w, cell):
    """(Hc, Wc) of the product grid: cells of ``cell`` x ``cell`` pixels anchored at pixel (0, 0), partial cells at the bottom / right."""
    return -(-h // cell), -(-w // cell)


class ProductGrid:
    """The product the reference's README recommends for the final maps and for evaluation: the 10 m output aggregated to a grid of
    ``cell`` x ``cell`` pixels (cell = 10: one hectare), stitched on the device (``csrc/product.hip``).

    The product mean is the block sum of the 10 m mean map.  The product's ensemble spread is NOT a function of the 10 m std map: it is
    the standard deviation over members of each member's own cell total, and a cell total is complete only once every window that
    touches the cell has been added (cells are not aligned with window interiors; catch-up windows and seasons revisit pixels).  So the
    grid keeps one small plane per member, ``cells`` (M, Hc, Wc), to which every window adds its interior pixels weighted by
    1 / visit count; ``visits`` (h, w) int16 is that count for one member over the WHOLE window list and must be set (``set_windows``)
    before the first ``add_window``.  ``finalize`` reduces the planes to ``mean`` / ``std`` (Hc, Wc).  No atomics: bit-reproducible.

    Multi-GPU (windows sharded over ranks): every rank sets the complete window list, adds its own windows, and ``all_reduce`` sums the
    small planes; the visit map depends on the window list alone and needs no collective."""

    def __init__(self, h, w, cell, members, device):
        if torch.device(device).type != "cuda":
            raise L.PopcornHipError("ProductGrid accumulates on a HIP device only")
        if int(cell) < 1 or int(members) < 1:
            raise ValueError(f"ProductGrid: cell and members must be >= 1, got cell {cell}, members {members}")
        self.h, self.w, self.cell, self.members = int(h), int(w), int(cell), int(members)
        self.cells = torch.zeros(self.members, *product_shape(self.h, self.w, self.cell), dtype=torch.float32, device=device)
        self.visits = torch.zeros(self.h, self.w, dtype=torch.int16, device=device)
        self.mean = self.std = None

    def set_windows(self, idx, patchsize=INFERENCE_PATCH_SIZE, overlap=OVERLAP):
        """The complete window list of the evaluation (``get_patch_indices``: rows of (row origin, column origin[, season]); every
        season's windows count) -> the visit map.  Starts a new accumulation: the planes are zeroed."""
        require_raster_fits(self.h, self.w, patchsize, "ProductGrid.set_windows")
        self.cells.zero_()
        self.visits.zero_()
        self.mean = self.std = None
        count_windows(self.visits, [(r[0], r[1]) for r in idx], 1, patchsize, overlap)

    def add_window(self, xl, yl, popdense, overlap=OVERLAP):
        """popdense: (M, ps, ps) member outputs of the window whose origin is row xl, column yl, as for ``Stitcher.add_window``."""
        L.require_device(popdense)
        M, psx, psy = popdense.shape
        if M != self.members:
            raise ValueError(f"ProductGrid of {self.members} members got a window of {M}")
        popdense = popdense.contiguous().float()
        L.check(L.lib().pc_product_accumulate(L.ptr(popdense), M, psx, psy, int(overlap), int(xl), int(yl), L.ptr(self.visits), self.h,
                                              self.w, self.cell, L.ptr(self.cells), L.stream_ptr()), "pc_product_accumulate")

    def all_reduce(self, reducer: FlatReducer):
        """Multi-GPU: the sum of every rank's planes on every rank (M * Hc * Wc floats, one collective)."""
        if reducer.active:
            import torch.distributed as dist
            dist.all_reduce(self.cells, group=reducer.group)

    def finalize(self):
        """(mean, std) over the members of every cell, (Hc, Wc) each; std is the n - 1 form, 0 for a single member."""
        if self.mean is None:
            self.mean, self.std = torch.empty_like(self.cells[0]), torch.empty_like(self.cells[0])
        L.check(L.lib().pc_product_finalize(L.ptr(self.cells), self.members, self.mean.numel(), L.ptr(self.mean), L.ptr(self.std),
                                            L.stream_ptr()), "pc_product_finalize")
        return self.mean, self.std


class CensusTable:
    """Census-unit totals of every ensemble member, accumulated on the device as the windows go by (``csrc/census_table.hip``): what the
    evaluation is judged on (``convert_popmap_to_census`` -> ``get_test_metrics``), with the ensemble spread per unit.

    As for ``ProductGrid``, the spread of a unit total is the standard deviation over members of each member's own total, which is no
    function of the 10 m std map and is complete only once every window that touches the unit has been added, each pixel weighted by
    1 / its visit count.  ``boundaries``: one (h, w) id raster per census level (the reference's ``testlevels_eval``, e.g. fine and
    coarse), at most ``PC_CENSUS_MAX_LEVELS``; ``num_ids[l]``: ids of level l are [0, num_ids[l]), anything else is ignored.  The table is
    ``table`` (M, T) int64, T = sum(num_ids), level l in columns ``offsets[l] : offsets[l] + num_ids[l]``: 64-bit fixed point with 30
    fractional bits, so it holds the same bits for any window order and rank sharding (a unit total must stay below 2^33 per member).
    ``visits`` (h, w) int16 is the visit count of one member over the whole window list; pass a ``ProductGrid``'s to share it.

    Multi-GPU: every rank sets the complete window list and adds its own windows; ``all_reduce`` is an exact int64 sum.

    ``adjust`` (opt-in) = {"level": a, "census_idx": ..., "census_pop": ...}: the dasymetric adjustment of every member's map to the census
    of level a (``adjust_map_to_census``), judged on every level, without the maps (``csrc/census_adjust.hip``).  The adjustment scales
    every pixel of a unit c of level a by one factor, so the adjusted total of a unit f of level l follows from the joint sums over the
    (f, c) pairs that share a pixel: one pair plane per other level is planned once at construction (``ops.census_pair_plan``; boundaries
    are fixed, every ``set_windows`` reuses it) and accumulated as one more level, its columns behind the levels' (``offsets``,
    ``level(l)`` and ``metrics`` keep their meaning; ``T`` grows).  Levels plus pair planes must not exceed ``PC_CENSUS_MAX_LEVELS``.  Read
    ``pairs(l)``, ``adjusted(l)``, ``adjusted_census(...)``, ``adjusted_metrics(...)``."""

    def __init__(self, h, w, boundaries, num_ids, members, device, visits=None, adjust=None):
        if torch.device(device).type != "cuda":
            raise L.PopcornHipError("CensusTable accumulates on a HIP device only")
        boundaries, num_ids = list(boundaries), [int(n) for n in num_ids]
        if int(members) < 1 or not boundaries or len(boundaries) != len(num_ids) or min(num_ids) < 1:
            raise ValueError(f"CensusTable: members >= 1 and one num_ids >= 1 per boundary, got members {members}, {len(boundaries)} "
                             f"boundaries, num_ids {num_ids}")
        if len(boundaries) > L.PC_CENSUS_MAX_LEVELS:
            raise ValueError(f"CensusTable: at most {L.PC_CENSUS_MAX_LEVELS} census levels, got {len(boundaries)}")
        self.h, self.w, self.members, self.num_ids = int(h), int(w), int(members), num_ids
        for b in boundaries:
            if tuple(b.shape) != (self.h, self.w):
                raise ValueError(f"CensusTable: boundary of shape {tuple(b.shape)} for a raster of {self.h} x {self.w}")
        self.boundaries = [b.to(device=device, dtype=torch.int32).contiguous() for b in boundaries]     # converted once
        self.offsets = [sum(num_ids[:l]) for l in range(len(num_ids))]
        self.T = sum(num_ids)
        self.adjust_level, self._pairs, self._adjusted = None, {}, {}
        planes, plane_ids = [], []
        if adjust is not None:
            planes, plane_ids = self._plan_adjust(adjust, device)
        self.table = torch.zeros(self.members, self.T, dtype=torch.int64, device=device)
        self.flags = torch.zeros(1, dtype=torch.int32, device=device)
        if visits is not None and (tuple(visits.shape) != (self.h, self.w) or visits.dtype != torch.int16 or not visits.is_cuda
                                   or not visits.is_contiguous()):
            raise ValueError("CensusTable: visits must be a contiguous (h, w) int16 device map")
        self.shared_visits = visits is not None
        self.visits = visits if visits is not None else torch.zeros(self.h, self.w, dtype=torch.int16, device=device)
        # what one accumulate launch takes: the levels, then the pair planes (ids of a plane: its pairs, at least 1)
        self._planes = self.boundaries + planes
        all_ids = num_ids + plane_ids
        nl = len(all_ids)
        self._bptr = (C.c_void_p * nl)(*[b.data_ptr() for b in self._planes])
        self._nids, self._off = (C.c_int32 * nl)(*all_ids), (C.c_int32 * nl)(*[sum(all_ids[:l]) for l in range(nl)])
        self.totals = self.mean = self.std = None

    def _plan_adjust(self, adjust, device):
        """The pair plane of every level but ``adjust["level"]`` (one plan per region) and the census of that level as per-unit tables."""
        from . import ops
        a = int(adjust["level"])
        nl = len(self.num_ids)
        if not 0 <= a < nl:
            raise ValueError(f"CensusTable: adjust level {a} of {nl} levels")
        if 2 * nl - 1 > L.PC_CENSUS_MAX_LEVELS:
            raise ValueError(f"CensusTable: {nl} census levels plus {nl - 1} pair planes (one per level judged after the adjustment to "
                             f"level {a}) exceed the {L.PC_CENSUS_MAX_LEVELS} levels one accumulate pass takes")
        idx = torch.as_tensor(adjust["census_idx"], dtype=torch.int64).reshape(-1)
        pop = torch.as_tensor(adjust["census_pop"], dtype=torch.float32).reshape(-1)
        if idx.numel() != pop.numel() or (idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.num_ids[a])):
            raise ValueError(f"CensusTable: adjust needs one census_pop per census_idx, ids in [0, {self.num_ids[a]})")
        self.adjust_level = a
        self._pop = torch.zeros(self.num_ids[a], dtype=torch.float32, device=device)
        self._has = torch.zeros(self.num_ids[a], dtype=torch.uint8, device=device)
        self._pop[idx.to(device)] = pop.to(device)
        self._has[idx.to(device)] = 1
        planes, plane_ids = [], []
        for l in range(nl):
            if l == a:
                continue
            plane, pair_f, pair_c, base = ops.census_pair_plan(self.boundaries[l], self.boundaries[a], self.num_ids[l], self.num_ids[a])
            self._pairs[l] = {"f": pair_f, "c": pair_c, "base": base, "np": int(pair_c.numel()), "off": self.T}
            planes.append(plane)
            plane_ids.append(max(1, int(pair_c.numel())))
            self.T += plane_ids[-1]
        return planes, plane_ids

    def set_windows(self, idx, patchsize=INFERENCE_PATCH_SIZE, overlap=OVERLAP):
        """The complete window list of the evaluation (as ``ProductGrid.set_windows``) -> the visit map.  Starts a new accumulation: the
        table and the flags are zeroed.  A shared visit map is left to its owner, whose ``set_windows`` must have run."""
        require_raster_fits(self.h, self.w, patchsize, "CensusTable.set_windows")
        self.table.zero_()
        self.flags.zero_()
        self.totals = self.mean = self.std = None
        self._adjusted = {}
        if not self.shared_visits:
            self.visits.zero_()
            count_windows(self.visits, [(r[0], r[1]) for r in idx], 1, patchsize, overlap)

    def add_window(self, xl, yl, popdense, overlap=OVERLAP):
        """popdense: (M, ps, ps) member outputs of the window whose origin is row xl, column yl, as for ``Stitcher.add_window``."""
        L.require_device(popdense)
        M, psx, psy = popdense.shape
        if M != self.members:
            raise ValueError(f"CensusTable of {self.members} members got a window of {M}")
        popdense = popdense.contiguous().float()
        L.check(L.lib().pc_census_accumulate(L.ptr(popdense), M, psx, psy, int(overlap), int(xl), int(yl), L.ptr(self.visits), self.h,
                                             self.w, len(self._planes), self._bptr, self._nids, self._off, L.ptr(self.table),
                                             C.c_int64(self.T), L.ptr(self.flags), L.stream_ptr()), "pc_census_accumulate")

    def all_reduce(self, reducer: FlatReducer):
        """Multi-GPU: the exact int64 sum of every rank's table (and the OR of the flags) on every rank."""
        if reducer.active:
            import torch.distributed as dist
            dist.all_reduce(self.table, group=reducer.group)
            dist.all_reduce(self.flags, op=dist.ReduceOp.MAX, group=reducer.group)

    def finalize(self):
        """(totals (M, T) float64, mean (T,), std (T,)) over the members; std is the n - 1 form, 0 for a single member.  Raises when a
        window held a value the table cannot take (NaN, +-Inf, negative or >= 2^32 after the division by the visit count)."""
        if int(self.flags.item()) != 0:
            raise L.PopcornHipError("CensusTable: a window held a NaN, infinite, negative or >= 2^32 value inside a census unit; "
                                    "the table is incomplete")
        if self.totals is None:
            dev = self.table.device
            self.totals = torch.empty(self.members, self.T, dtype=torch.float64, device=dev)
            self.mean, self.std = torch.empty(self.T, dtype=torch.float32, device=dev), torch.empty(self.T, dtype=torch.float32, device=dev)
        L.check(L.lib().pc_census_finalize(L.ptr(self.table), self.members, C.c_int64(self.T), L.ptr(self.totals), L.ptr(self.mean),
                                           L.ptr(self.std), L.stream_ptr()), "pc_census_finalize")
        self._adjusted = {}
        return self.totals, self.mean, self.std

    def level(self, l):
        """(totals (M, num_ids[l]), mean, std) of census level l: views of the finalised table."""
        if self.totals is None:
            self.finalize()
        a, b = self.offsets[l], self.offsets[l] + self.num_ids[l]
        return self.totals[:, a:b], self.mean[a:b], self.std[a:b]

    def census(self, l, census_idx, census_pop):
        """(pred_mean (n,), pred_std (n,), pred_members (M, n), gt (n,)) for the census rows ``census_idx`` (unit ids of level l) /
        ``census_pop`` (POP20): the per-unit counterpart of ``convert_popmap_to_census`` with the ensemble spread."""
        totals, mean, std = self.level(l)
        census_idx = torch.as_tensor(census_idx, dtype=torch.int64, device=mean.device)
        gt = torch.as_tensor(census_pop, dtype=torch.float32, device=mean.device)
        return mean[census_idx], std[census_idx], totals[:, census_idx].to(torch.float32), gt

    def metrics(self, l, census_idx, census_pop, tag=""):
        """``get_test_metrics`` of the ensemble mean under its usual keys, plus ``<key>_members_mean`` / ``<key>_members_std``: the mean
        and the n - 1 standard deviation (0 for one member) over members of the metric computed for each member's own totals."""
        pm, _, members, gt = self.census(l, census_idx, census_pop)
        return self._metrics_with_spread(pm, members, gt, tag)

    def _metrics_with_spread(self, pred, members, gt, tag):
        from .utils.metrics import get_test_metrics
        res = {k: float(v) for k, v in get_test_metrics(pred, gt, tag=tag).items()}
        per = [get_test_metrics(members[m], gt, tag=tag) for m in range(self.members)]
        for k in list(res):
            v = torch.tensor([float(p[k]) for p in per], dtype=torch.float64)
            res[k + "_members_mean"] = v.mean().item()
            res[k + "_members_std"] = v.std(unbiased=True).item() if self.members > 1 else 0.0
        return res


    # ---- the adjustment to the census of level ``adjust["level"]`` ------------------------------------------------------------------
    def pairs(self, l):
        """(pair_f (NP,), pair_c (NP,), totals (M, NP)) of level l: the (unit of l, unit of the adjust level) pairs that share a pixel,
        ordered by (f, c), and every member's joint sums (views of the finalised table)."""
        if self.adjust_level is None or l not in self._pairs:
            raise ValueError(f"CensusTable: no pair plane for level {l} (adjust level: {self.adjust_level})")
        if self.totals is None:
            self.finalize()
        p = self._pairs[l]
        return p["f"], p["c"], self.totals[:, p["off"]:p["off"] + p["np"]]

    def adjusted(self, l):
        """(adj_members (M, n) float64, adj_ensemble (n,) float64, mean (n,), std (n,)) of level l after the adjustment: every member's
        own map adjusted to the census of the adjust level, the adjustment of the ENSEMBLE-MEAN map (what the reference adjusts; it is
        not the mean of the members' where their factors differ), and the mean / (n - 1) standard deviation over the members.  The
        arithmetic: ``include/popcorn_hip.h``, pc_census_adjust_finalize."""
        if self.adjust_level is None:
            raise ValueError("CensusTable was built without adjust=")
        if self.totals is None:
            self.finalize()
        if l not in self._adjusted:
            a, n, dev = self.adjust_level, self.num_ids[l], self.table.device
            adj = torch.empty(self.members + 1, n, dtype=torch.float64, device=dev)
            mean, std = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            p = self._pairs.get(l)
            if l != a and p is None:
                raise ValueError(f"CensusTable: level {l} of {len(self.num_ids)} levels")
            L.check(L.lib().pc_census_adjust_finalize(
                L.ptr(self.table), self.members, C.c_int64(self.T), C.c_int64(self.offsets[l]), C.c_int64(self.offsets[a]),
                C.c_int64(p["off"] if p else 0), n, self.num_ids[a], C.c_int64(p["np"] if p else 0), L.ptr(p["base"] if p else None),
                L.ptr(p["c"] if p else None), L.ptr(self._pop), L.ptr(self._has), L.ptr(adj), L.ptr(mean), L.ptr(std), L.stream_ptr()),
                "pc_census_adjust_finalize")
            self._adjusted[l] = (adj[:self.members], adj[self.members], mean, std)
        return self._adjusted[l]

    def adjusted_census(self, l, census_idx, census_pop):
        """(pred_ensemble (n,), pred_std (n,), pred_members (M, n), gt (n,)) in fp32 for the census rows of level l, after the adjustment:
        the counterpart of ``census``; pred_ensemble is the adjusted ensemble-mean map's total."""
        members, ens, _, std = self.adjusted(l)
        census_idx = torch.as_tensor(census_idx, dtype=torch.int64, device=ens.device)
        gt = torch.as_tensor(census_pop, dtype=torch.float32, device=ens.device)
        return ens[census_idx].to(torch.float32), std[census_idx], members[:, census_idx].to(torch.float32), gt

    def adjusted_metrics(self, l, census_idx, census_pop, tag=""):
        """``get_test_metrics`` of the adjusted ensemble-mean map under its usual keys, plus ``<key>_members_mean`` /
        ``<key>_members_std`` over the members' own adjusted totals, as ``metrics``."""
        ens, _, members, gt = self.adjusted_census(l, census_idx, census_pop)
        return self._metrics_with_spread(ens, members, gt, tag)


def census_detail_maps(pred_totals, boundary, census_idx, census_pop, pred_std=None):
    """The six per-unit detail maps of the reference's ``full`` evaluation mode (``details_to=``, data/PopulationDataset.py:747-804) as
    one gather launch instead of six Python loops over the census rows.  pred_totals: (num_ids,) predicted total per unit id (a level of
    a ``CensusTable``, or ``census_sums``); boundary: (h, w) id raster; census_idx / census_pop: the census rows (unit id, POP20).
    With ``count`` the pixel count of the unit (``pc_census_sum``'s counts) the maps hold, on every pixel of a unit with a census row:

      densities      pred / count                          (:748-753)
      totals         pred                                  (:756-761)
      densities_gt   POP20 / count                         (:764-769)
      totals_gt      POP20                                 (:772-777)
      residuals      pred - POP20 in fp32                  (:780-785)
      residuals_rel  (pred - POP20) / count, inf / NaN -> 0  (:788-804)
      totals_std     pred_std (only when given; no counterpart in the reference)

    and 0 on pixels of units without a census row and of ids outside [0, num_ids).  The per-unit values are computed once in float64
    from the fp32 totals and rounded to fp32, then painted by ``ops.census_paint``.  Returns a dict of (h, w) fp32 device maps."""
    from . import ops
    L.require_device(pred_totals, boundary)
    dev = pred_totals.device
    num_ids = pred_totals.numel()
    b32 = boundary.to(torch.int32).contiguous()
    census_idx = torch.as_tensor(census_idx, dtype=torch.int64, device=dev)
    # the pixel counts: pc_census_sum over the boundary plane itself (its bits read as fp32; the sums are not used)
    _, counts = census_sums(b32.view(torch.float32), b32, num_ids, want_counts=True)
    count = counts.double()
    has = torch.zeros(num_ids, dtype=torch.bool, device=dev)
    has[census_idx] = True
    pred = pred_totals.to(torch.float32).double()
    pop = torch.zeros(num_ids, dtype=torch.float64, device=dev)
    pop[census_idx] = torch.as_tensor(census_pop, dtype=torch.float32, device=dev).double()
    res = (pred - pop).to(torch.float32).double()
    rel = res / count
    rel[torch.isinf(rel) | torch.isnan(rel)] = 0
    tabs = {"densities": pred / count, "totals": pred, "densities_gt": pop / count, "totals_gt": pop, "residuals": res,
            "residuals_rel": rel}
    if pred_std is not None:
        tabs["totals_std"] = pred_std.to(device=dev, dtype=torch.float32).double()
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    names = list(tabs)
    maps = ops.census_paint(b32, [torch.where(has, tabs[k], zero).to(torch.float32) for k in names])
    return {k: maps[i] for i, k in enumerate(names)}


def census_sums(pred, boundary, num_ids, want_counts=False):
    """sums[id] = sum(pred[boundary == id]) for id in [0, num_ids) -- one pass (segment sum).  pred: (h,w) f32,
    boundary: (h,w) int32.  Returns float64 sums (and int32 counts)."""
    L.require_device(pred, boundary)
    assert pred.dtype == torch.float32 and boundary.dtype == torch.int32 and pred.is_contiguous() and boundary.is_contiguous()
    sums = torch.empty(num_ids, dtype=torch.float64, device=pred.device)
    counts = torch.empty(num_ids, dtype=torch.int32, device=pred.device) if want_counts else None
    L.check(L.lib().pc_census_sum(L.ptr(pred), L.ptr(boundary), C.c_int64(pred.numel()), num_ids, L.ptr(sums),
                                  L.ptr(counts), L.stream_ptr()), "pc_census_sum")
    return (sums, counts) if want_counts else sums


def census_sums_sharded(st: "Stitcher", boundary, num_ids, reducer: FlatReducer):
    """Region sums of a map that is distributed by row band (``evaluate_raster(..., gather=False)``): each rank sums its own
    band, then ONE all-reduce of the float64 per-region sums (num_ids * 8 bytes) -- the full map never travels."""
    r0, r1 = st.band if st.band is not None else (0, st.h)
    if r1 > r0:
        # (a band starts at byte r0 * w * 4 of the plane: any 4-byte alignment -- pc_census_sum takes a scalar head)
        sums = census_sums(st.out[r0:r1], boundary[r0:r1].contiguous().to(torch.int32), num_ids)
    else:
        sums = torch.zeros(num_ids, dtype=torch.float64, device=st.out.device)
    if reducer.active:
        import torch.distributed as dist
        dist.all_reduce(sums, group=reducer.group)
    return sums


def convert_popmap_to_census(pred, boundary, census_idx, census_pop):
    """data/PopulationDataset.py:675-820 without the GeoTIFF/CSV I/O: returns (census_pred, census_gt) for the census
    rows ``census_idx`` (region ids) / ``census_pop`` (POP20)."""
    census_idx = torch.as_tensor(census_idx, dtype=torch.int64, device=pred.device)
    num_ids = int(census_idx.max().item()) + 1 if census_idx.numel() else 1
    sums = census_sums(pred.contiguous().float(), boundary.contiguous().to(torch.int32), num_ids)
    census_pred = sums[census_idx].to(torch.float32)
    census_gt = torch.as_tensor(census_pop, dtype=torch.float32, device=pred.device)
    return census_pred, census_gt


def adjust_map_to_census(pred, boundary, census_idx, census_pop):
    """Dasymetric rescale so that every census region sums to its census count (data/PopulationDataset.py:823-852).
    In place on ``pred`` like the reference; returns it."""
    L.require_device(pred, boundary)
    census_idx = torch.as_tensor(census_idx, dtype=torch.int64, device=pred.device)
    num_ids = int(census_idx.max().item()) + 1 if census_idx.numel() else 1
    b32 = boundary.contiguous().to(torch.int32)
    sums = census_sums(pred, b32, num_ids)
    pop = torch.zeros(num_ids, dtype=torch.float32, device=pred.device)
    has = torch.zeros(num_ids, dtype=torch.uint8, device=pred.device)
    pop[census_idx] = torch.as_tensor(census_pop, dtype=torch.float32, device=pred.device)
    has[census_idx] = 1
    L.check(L.lib().pc_census_adjust(L.ptr(pred), L.ptr(b32), C.c_int64(pred.numel()), num_ids, L.ptr(sums), L.ptr(pop),
                                     L.ptr(has), L.stream_ptr()), "pc_census_adjust")
    return pred


def raw_window_input(win, ascfill=False):
    """One raw window of ``evaluate_raster(raw=True)`` -> the normalised model input (1, 6, ps, ps): the window's S2 / S1 NaN-filled on
    their own (data/PopulationDataset.py:479-500 via ``data.nanfill.fill_item_``; S1 may switch to ``win["S1_asc"]()``), THEN normalised
    -- the fill copies values across channels, so it must see the loader's raw bands, not normalised ones.  Returns (input, orbit)."""
    from .data import stats
    from .data.nanfill import fill_item_
    from . import ops
    s2, s1 = win["S2"], win["S1"]
    L.require_device(s2, s1)
    raw = torch.cat([s2.float(), s1.float()], 1).contiguous()                # (1, 6, ps, ps); the two views below are contiguous
    orbit = fill_item_(raw[:, :4], raw[:, 4:], win.get("S1_asc"), ascfill)
    return ops.select_normalize(raw, tuple(range(6)), stats.MEAN6, stats.STD6), orbit


def evaluate_raster(models, raster, patchsize=INFERENCE_PATCH_SIZE, overlap=OVERLAP, fourseasons=False,
                    reducer: FlatReducer | None = None, rank=0, band_reduce=True, gather=True, return_stitcher=False, raw=False,
                    ascfill=False, product: ProductGrid | None = None, census: CensusTable | None = None, buildings=None):
    """Ensemble sliding-window inference over ``raster`` = callable (x, y, season, ps) -> normalised model input
    (1,6,ps,ps) on the device (the reference's Population_Dataset(mode="test") item, PopulationDataset.py:336-420), or a
    (S,6,h,w) device tensor of pre-normalised seasons.  Returns the finalised (mean map, std map, scale mean, scale std).

    Windows are assigned round-robin to ranks (no data-path collective).  Multi-GPU: ``band_reduce`` (default) sums the
    accumulators with one reduce-scatter by row band, every rank finalises its own band, and ``gather`` decides whether the
    bands are then all-gathered into full maps on every rank (True: the four maps are returned, as in the single-process
    case) or stay distributed (False: the ``Stitcher`` is returned; ``census_sums_sharded`` works on the band).
    ``band_reduce=False``: the round-2 form, an all-reduce of the full planes and of the count map.
    ``return_stitcher``: also return the ``Stitcher`` (its visit-count map).
    ``raw``: real rasters -- the callable returns the loader's UN-normalised bands {"S2": (1,4,ps,ps), "S1": (1,2,ps,ps)} plus an optional
    "S1_asc" callable (the ascending orbit); every window is NaN-filled on the device and then normalised (``raw_window_input``; one
    host synchronisation per window for the 5 % orbit rule).  ``ascfill``: the reference's per-region switch to the ascending orbit.
    ``product``: a ``ProductGrid`` of this raster and ensemble; it is given the window list, fed every window this rank computes,
    all-reduced and finalised on every rank (read ``product.mean`` / ``.std`` / ``.cells``); what is returned does not change.
    ``census``: a ``CensusTable`` of this raster and ensemble, handled exactly like ``product`` (read ``census.totals`` / ``.mean`` /
    ``.std``, ``census.level(l)``, ``census.metrics(...)``).
    ``buildings``: the building layer the dataset ships for test windows as well (PopulationDataset.py:475,520-523) -- an (h, w) device
    tensor without a season axis; None takes what the raster object provides (``raster.buildings``, e.g. a ``SyntheticTestRaster(
    buildings=True)``).  A ``raw=True`` callable may instead add "building_counts" (1, 1, ps, ps) to its dict, and a ``ResidentWindows``
    over a region with a layer hands over the plane of the window it just produced (``window_buildings``); both take precedence over the
    tensor.  Every window's sample of a member built WITHOUT ``sentinelbuildings`` then carries ``building_counts`` (1, 1, ps, ps) and the
    member never runs its extractor; members built with it ignore the layer, as the reference's model does (popcorn.py:112-114).  Stitcher,
    product grid, census table and the rank sharding are unchanged."""
    reducer = reducer or FlatReducer()
    source = raster
    if torch.is_tensor(raster):
        h, w = raster.shape[-2:]
        tensor = raster
        raster = lambda x, y, s, ps: tensor[s:s + 1, :, x:x + ps, y:y + ps]  # noqa: E731
    else:
        h, w = raster.shape
        if buildings is None:
            buildings = getattr(raster, "buildings", None)
    if buildings is not None:
        L.require_device(buildings)
        if tuple(buildings.shape) != (h, w):
            raise ValueError(f"evaluate_raster: buildings is an (h, w) = ({h}, {w}) layer without a season axis, got {tuple(buildings.shape)}")
        buildings = buildings.float()
    require_raster_fits(h, w, patchsize, "evaluate_raster")            # before anything is allocated or launched
    dev = next(models[0].parameters()).device
    st = Stitcher(h, w, dev, world=reducer.world)
    idx = get_patch_indices(h, w, patchsize, overlap, fourseasons)
    mine = set(shard_indices(idx.shape[0], rank, reducer.world))
    if product is not None:
        if (product.h, product.w, product.members) != (h, w, len(models)):
            raise ValueError(f"product grid of {product.h} x {product.w} x {product.members} members for a raster of {h} x {w} and "
                             f"{len(models)} models")
        product.set_windows(idx, patchsize, overlap)
    if census is not None:
        if (census.h, census.w, census.members) != (h, w, len(models)):
            raise ValueError(f"census table of {census.h} x {census.w} x {census.members} members for a raster of {h} x {w} and "
                             f"{len(models)} models")
        census.set_windows(idx, patchsize, overlap)
    if band_reduce and reducer.world > 1:
        # the visit count needs no collective: the windows of the OTHER ranks enter this rank's count map analytically, all at once
        st.add_counts_only([(int(idx[i][0]), int(idx[i][1])) for i in range(idx.shape[0]) if i not in mine], len(models), patchsize, overlap)
    for i in range(idx.shape[0]):
        x, y, season = (int(v) for v in idx[i])
        if i not in mine:
            continue
        layer = None
        if raw:
            win = raster(x, y, season, patchsize)
            inp, _ = raw_window_input(win, ascfill)
            layer = win.get("building_counts")
        else:
            inp = raster(x, y, season, patchsize).contiguous()
        if layer is None:
            layer = getattr(source, "window_buildings", None)           # ResidentWindows: the plane of the window it just produced
        if layer is None and buildings is not None:
            layer = buildings[x:x + patchsize, y:y + patchsize]
        if layer is not None:
            layer = layer.reshape(1, 1, patchsize, patchsize).contiguous()
        sample = {"input": inp}
        pds, scs = [], []
        with torch.no_grad(), L.padded_rows():      # (16-byte aligned rows for the levels whose width is not a multiple of 4)
            for j, m in enumerate(models):
                m.eval()
                if layer is not None and not m.sentinelbuildings:
                    # a shipped layer: the member multiplies its occupancy head by it and never runs the extractor (a dict of its own,
                    # so that no member's extractor score stands in for the layer)
                    o = m({"input": inp, "building_counts": layer}, padding=False)
                elif j > 0 and m.sentinelbuildings and "building_counts" in sample:
                    # identical frozen extractor in every member: reuse the score of member 0
                    keep = m.sentinelbuildings
                    m.sentinelbuildings = False
                    o = m(sample, padding=False)
                    m.sentinelbuildings = keep
                else:
                    o = m(sample, padding=False)
                pds.append(o["popdensemap"][0])
                if o.get("scale") is not None:
                    scs.append(o["scale"][0])
        pd = torch.stack(pds)
        st.add_window(x, y, pd, torch.stack(scs) if scs else None, overlap)
        if product is not None:
            product.add_window(x, y, pd, overlap)
        if census is not None:
            census.add_window(x, y, pd, overlap)
    if product is not None:
        product.all_reduce(reducer)
        product.finalize()
    if census is not None:
        census.all_reduce(reducer)
        census.finalize()
    if band_reduce and reducer.world > 1:
        # one reduce-scatter by row band (half the bytes of an all-reduce, no count collective), every rank finalises its band
        st.reduce_scatter(reducer, rank)
        st.finalize()
        if not gather:
            return st
        maps = st.gather_bands(reducer)
        return (maps, st) if return_stitcher else maps
    st.all_reduce(reducer)
    maps = st.finalize()
    return (maps, st) if return_stitcher else maps
