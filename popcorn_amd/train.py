"""Fused training step: the build's counterpart of the reference's inner training loop
(run_train.py:186-238: forward(train, padding=False, sparse=True) -> get_loss -> x lam_weak -> backward ->
clip_grad_norm_(0.01) -> Adam step -> zero_grad), with everything on the device and nothing synchronising:

    building score (frozen U-Net) -> sparsity mask -> U-Net forward -> sparse head (+ {Nsel, sum scale})
    -> [DP: all-reduce 2 scalars] -> loss fwd+bwd kernel -> head backward -> U-Net backward into ONE flat gradient
    buffer -> [DP: one all-reduce] -> gradient norm -> fused clip + Adam over the flat parameter buffer.

The 56 trainable tensors (39,298 elements) are re-homed as views of one flat buffer, so the optimiser and the
all-reduce are single kernels / a single collective.  The static-shape step can be captured into HIP graphs
(``use_graph=True``) and replayed with no per-launch host cost.

Multi-unit census supervision (opt-in; csrc/units.hip): a sample whose ``census_idx`` is 2-D (B, K) -- with ``y`` (B, K) and the optional
host-side ``census_n`` -- supervises every listed unit of each crop in one step: one crop, K popcounts, one loss over the N = sum(census_n)
(b, k) pairs, one backward.  It computes what the one-unit step computes on the replicated batch.  Such a step runs eagerly through the
per-launch engine -- or, with ``native_units=True``, through the native executor (pc_train_step_units: one C-ABI call, the same bits);
graph mode and data parallelism raise for it (``FusedTrainStep.step``) -- unless the trainer was built with ``device_units=True``: the
device-N step (pc_unit_layout_dev, pc_unit_popcount_loss_dev) runs every launch at the capacity B * K and reads the counts, N and 1 / N
from device memory, so that one captured graph serves every N and the global N of a data-parallel step rides in the stats all-reduce.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import os
from types import SimpleNamespace

import torch

from . import _lib as L
from . import engine as E
from . import ops
from .distributed import FlatReducer
from .model.popcorn import draw_selection, pad_geometry

# The head backward hands its weight-gradient partials to the U-Net backward's batched reduction (False: it reduces them itself, one launch
# more per step -- what the head-only regime does anyway).  A test hook, not an environment switch any more (round 6).
DEFER_HEAD_REDUCE = True

# Eager steps (no captured graph: the reference's variable-size census regions, run_train.py:186-202) go through the native executor --
# ONE C-ABI call per step (pc_train_step: geometry, arena, descriptors and all launches in C++) instead of ~45 ctypes calls.
# POPCORN_NATIVE_STEP=0: the per-launch Python engine (same kernels; A/B switch and the bit-equality reference of the tests)
NATIVE_STEP = os.environ.get("POPCORN_NATIVE_STEP", "1") != "0"
_LAYER_TAGS = ("inc1", "inc2", "d1a", "d1b", "d2a", "d2b", "up2a", "up2b", "up1a", "up1b")      # pc_step_stream's layer order
_CONVT_TAGS = ("up2t", "up1t")


def fill_step_net(net, eng, grads, prefix, keep):
    """One network of a pc_step_plan (``net``: a PcStepNet) from its engine.  A stream keeps its slot -- 0: sar, 1: optical -- whichever
    streams the model has: the table of an absent one stays all zero (a one-stream plan, include/popcorn_hip.h).  ``fusion_w`` /
    ``fusion_b``: fusion_out_conv (16 + 1), or the only stream's own out conv (8 + 1).  ``grads`` / ``prefix``: the gradient targets of
    the trainable network (None: the frozen extractor).  ``keep`` collects what the raw pointers refer to."""
    slots = [n for n, _, _, _ in E.STREAMS]
    for sname, chmap, cin, f0 in eng.streams:
        st = net.s[slots.index(sname)]
        for li, tag in enumerate(_LAYER_TAGS):
            lay = eng.layers[(sname, tag)]
            st.w[li] = lay.w.data_ptr()
            st.bn[li] = lay.bn
            if prefix is not None:
                st.dw[li] = grads[prefix + lay.wname].data_ptr()
                st.db[li] = grads[prefix + lay.bname].data_ptr()
            keep.append(lay)
        for ti, tag in enumerate(_CONVT_TAGS):
            lay = eng.layers[(sname, tag)]
            st.wt[ti], st.bt[ti] = lay.w.data_ptr(), lay.b.data_ptr()
            if prefix is not None:
                st.dwt[ti] = grads[prefix + lay.wname].data_ptr()
                st.dbt[ti] = grads[prefix + lay.bname].data_ptr()
            keep.append(lay)
        for c in range(4):
            st.chan[c] = chmap[c]
        st.cin, st.feat_c0 = cin, f0
    ow, ob = (eng.fusion_w, eng.fusion_b) if eng.single_out is None else eng.single_out
    net.fusion_w, net.fusion_b = ow.data_ptr(), ob.data_ptr()
    keep.append((ow, ob))


class _ArenaOutputs:
    """The outputs of a native step -- views into the step's arena, built on first access (``popcount``, ``popdensemap``, ``scale_map``,
    ``mask``, ``building_counts``).  Valid until the trainer's next step (the arena is reused), like the static outputs of a replayed graph."""

    def __init__(self, arena, io, units=None, layer=None):
        B, H, W = io.B, io.H, io.W
        self._arena = arena
        self._layer = layer             # a step on a given building layer: the sample's own tensor is the output (io.off_building = -1)
        self._spec = {"popcount": (io.off_popcount, torch.float32, (B,)), "popdensemap": (io.off_popdense, torch.float32, (B, H, W)),
                      "scale_map": (io.off_scale, torch.float32, (B, H, W)), "mask": (io.off_mask, torch.uint8, (B, H, W)),
                      "building_counts": (io.off_building, torch.float32, (B, 1, H, W))}
        if units is not None:           # a multi-unit step (pc_step_units): popcount (N,) in (b, k) order, and the slot map
            self._spec.update(popcount=(units.off_popcount, torch.float32, (units.N,)), slot=(units.off_slot, torch.int32, (B, H, W)))
        self._views = {}

    def __getitem__(self, k):
        v = self._views.get(k)
        if v is None:
            off, dt, shape = self._spec[k]
            if off < 0:
                return self._layer
            n = 1
            for d in shape:
                n *= d
            nbytes = n * (1 if dt == torch.uint8 else 4)
            v = self._views[k] = self._arena[off:off + nbytes].view(dt).view(shape)
        return v

    def __contains__(self, k):
        return k in self._spec

    def get(self, k, default=None):
        return self[k] if k in self._spec else default

    def keys(self):
        return self._spec.keys()


@contextlib.contextmanager
def _capturing(g, **kw):
    """``torch.cuda.graph(g, **kw)`` with Python's cyclic garbage collector switched off for the duration of the capture.
    ``torch.cuda.graph.__enter__`` collects once before the capture begins; a collection that the ~40 launches' Python allocations
    trigger DURING it runs arbitrary finalisers of whatever became unreachable earlier in the process with a capture open -- and
    anything in them that synchronises, frees or touches another context (CUDA-IPC handles of tensors shared with worker processes,
    process-group objects, ...) is illegal then.  Observed once, deterministically for one state of the test suite: `Fatal Python
    error: Aborted` with the main thread `Garbage-collecting` inside ``_backward`` of a re-capture, after the multi-process tests
    had run in the same interpreter.  (Destroying an older captured step in the middle of a capture is NOT the trigger:
    tools/diag_gc_graph_destroy.py.)  Finalisers simply run after the capture instead."""
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):           # (__enter__ collects explicitly before the capture begins, whatever the collector's state)
            yield
    finally:
        # re-enabled only AFTER ``__exit__`` -> ``capture_end`` has run (round 4 re-enabled it inside the ``with``, i.e. with the capture
        # still open: ADVICE / VERDICT round 4)
        if was:
            gc.enable()


def _is_oom(exc):
    """An allocation failure, also when it surfaces as the RuntimeError of a failed ``capture_end`` with the OutOfMemoryError as its
    context (an exception inside ``with torch.cuda.graph(g)`` leaves through ``__exit__`` -> ``capture_end``, which raises on the
    invalidated capture and masks the original)."""
    seen = set()
    while exc is not None and id(exc) not in seen:
        seen.add(id(exc))
        if isinstance(exc, torch.OutOfMemoryError) or "out of memory" in str(exc).lower():
            return True
        exc = exc.__cause__ or exc.__context__
    return False


def data_keys(sample):
    """The keys of a sample that carry the image: the normalised model input, the raw fp32 tile, or the loader's pair {uint16 S2
    digital numbers, fp32 S1} (ingested by pc_ingest_split)."""
    if sample.get("input") is not None:
        return ("input",)
    if sample.get("raw") is not None:
        return ("raw",)
    if sample.get("raw_s2") is not None:
        return ("raw_s2", "raw_s1")
    raise KeyError("sample needs 'input', 'raw' or 'raw_s2' + 'raw_s1'")


def _is_multi_unit(sample):
    """A sample with a 2-D ``census_idx`` (B, K): multi-unit census supervision."""
    c = sample.get("census_idx")
    return torch.is_tensor(c) and c.dim() == 2


def _data_form(sample, u16=False):
    """(form, tensors) of a sample's image: ("input", (x,)), ("raw", (raw,)) or ("split", (s2, s1)).  The one copy of the split form's
    channel check; u16: the dtype too (the native executor reads the bytes through a raw pointer, the engine's ops check their own)."""
    dk = data_keys(sample)
    if len(dk) == 1:
        return dk[0], (sample[dk[0]],)
    s2, s1 = sample["raw_s2"], sample["raw_s1"]
    if s2.shape[1] != 4 or s1.shape[1] != 2 or (u16 and s2.dtype != torch.uint16):
        raise ValueError("raw_s2 / raw_s1: the 4 selected S2 bands [R, G, B, NIR] as uint16 and the 2 S1 bands [VV, VH] as fp32")
    return "split", (s2, s1)


# The one-launch ingest of a raw form -- band selection + normalisation + reflect padding + stream order, the unpadded input never
# written -- per (form, bf16 mode): (op, looked up in ``ops`` when called; needs real padding; needs 16-byte fp32 rows).  fp32 writes the
# padded planar input; bf16 ONE channels-last bf16 tensor (8-channel slots) that both networks' first convolutions and the first-layer
# weight gradients read through the standard 8-channel kernels.  The four rules differ; each is what its kernel takes.
_PADDED_INGEST = {("split", False): ("ingest_split", True, True), ("split", True): ("ingest_split", True, False),
                  ("raw", False): ("select_normalize_pad", False, True), ("raw", True): ("ingest_cl8", True, False)}


LOSS_INDEX = {"l1_loss": 0, "log_l1_loss": 1, "mse_loss": 2, "log_mse_loss": 3}
HEAD_NO_DECAY = ("head.6.weight", "head.6.bias")        # run_train.py:82


class FusedTrainStep:
    def __init__(self, model, lr=1e-4, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, gradient_clip=0.01,
                 loss=("log_l1_loss",), lam=(1.0,), scale_regularization=0.01, lam_weak=100.0,
                 reducer: FlatReducer | None = None, use_graph=False, raw_norm=None, graph_cache_max=None, native_units=False,
                 device_units=False, native_layer=False, native_single=False):
        """raw_norm = (band6, mean6, std6): how a RAW tile (sample key "raw" instead of "input": (B, Craw, H, W) reflectances /
        backscatter) becomes the model input -- band selection (data/PopulationDataset.py:566-568) + apply_normalize
        (utils/utils.py:105-127); default: the reference's dataset statistics (popcorn_amd.data.stats).  With a raw sample the
        step's first launch does select + normalise + reflect padding in one pass (pc_select_normalize_pad).
        graph_cache_max: how many captured steps (one per (tile shape, truncation regime, precision)) stay alive -- each owns a
        private memory pool with every activation and gradient of its step; default 6 or POPCORN_GRAPH_CACHE_MAX.  A capture that
        runs out of memory drops ALL cached graphs (and their pools) and is retried once.
        native_units: multi-unit samples (2-D census_idx) go through the native executor (pc_train_step_units) where it takes them --
        opt-in, experimental; off: the per-launch engine, as before.  The two compute the same bits.
        device_units: multi-unit samples take the device-N step (``step``): eager, captured (``use_graph=True``) and with an active
        data-parallel reducer; the native executor is not asked.  Off: as before, refusals included.  One-unit samples are unaffected.
        native_layer: eager steps on a given building layer (``sentinelbuildings=False`` models fed ``building_counts``) and of models without
        the occupancy product go through the native executor too (pc_train_step_layer / pc_train_step_units_layer) -- opt-in; off: the
        per-launch engine, as before.  The two compute the same bits.  Multi-unit samples on a layer need ``native_units`` as well.
        native_single: eager fp32 steps of a single-modality model (S1-only / S2-only: ``input_channels`` 2 / 4) go through the native
        executor too, as a one-stream plan (include/popcorn_hip.h) -- opt-in; off: the per-launch engine, as before.  The two compute the
        same bits; no torch op stays on that path (the 64 x 16 images of the head's first layer are made inside the call).  Multi-unit
        samples and shipped layers of such a model need ``native_units`` / ``native_layer`` as well."""
        from .data import stats as _stats
        self.raw_norm = raw_norm or (_stats.BAND6, _stats.MEAN6, _stats.STD6)
        self.model = model
        self.names, params = model.trainable()
        dev = params[0].device
        if dev.type != "cuda":
            raise L.PopcornHipError("FusedTrainStep needs the model on a HIP device (no CPU path)")
        self.device = dev
        assert self.names[-2:] == list(HEAD_NO_DECAY)
        sizes = [p.numel() for p in params]
        self.n = sum(sizes)
        self.n_decay = self.n - sizes[-1] - sizes[-2]
        self.flat_p = torch.empty(self.n, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(self.n, device=dev, dtype=torch.float32)
        self.grads = {}
        off = 0
        for n_, p in zip(self.names, params):
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + k].view_as(p)          # parameters become views of the flat buffer
            self.grads[n_] = self.flat_g[off:off + k].view_as(p)
            off += k
        model.invalidate_cache()
        self.m = torch.zeros_like(self.flat_p)
        self.v = torch.zeros_like(self.flat_p)
        # Adam parameter groups: 0 = U-Net encoder, 1 = U-Net decoder, 2 = head.  limit1 / limit2 samples give the
        # encoder / the whole U-Net no gradient (run_train.py:191-198) and torch.optim.Adam then skips those parameters
        # (state and per-parameter step untouched): one step counter per group, inactive groups are not updated.
        segs, off = [], 0
        for n_, k in zip(self.names, sizes):
            if n_.startswith("head."):
                grp = 2
            else:
                grp = 0 if any(("." + E.CONVS[t][0] + ".") in n_ for t in E.ENCODER) else 1
            off += k
            if segs and segs[-1][1] == grp:
                segs[-1] = (off, grp)
            else:
                segs.append((off, grp))
        self.segments = segs
        self.step_count = torch.zeros(L.PC_ADAM_GROUPS, device=dev, dtype=torch.int32)
        self.hyper = torch.tensor([lr], device=dev, dtype=torch.float32)
        self.lr = lr
        self.wd, self.betas, self.eps, self.clip = weight_decay, betas, eps, gradient_clip
        self.lam4 = [0.0] * 4
        for lo, la in zip(loss, lam):
            if lo in LOSS_INDEX:
                self.lam4[LOSS_INDEX[lo]] += la
        # popcorn.py:177-181 + utils/losses.py:63-76: without the occupancy model forward() returns scale = None and get_loss adds NO
        # scale regulariser, whatever --scale_regularization says (round 4: the fused step used to add it)
        self.sreg, self.lam_weak = (scale_regularization if model.occupancymodel else 0.0), lam_weak
        self.reducer = reducer or FlatReducer()
        # {Nsel, sum scale, N, reserved}: the first two as ever (the head / the loss launch write them); N = the pairs of a device-N multi-unit
        # step (pc_unit_layout_dev writes the local count).  ONE tensor: the global N rides in the stats all-reduce the step already has
        self.stats = torch.zeros(4, device=dev, dtype=torch.float64)
        self.loss_out = torch.zeros(2, device=dev, dtype=torch.float32)
        self.g_scale_const = torch.zeros(1, device=dev, dtype=torch.float32)
        self.norm = torch.zeros(1, device=dev, dtype=torch.float32)
        self.use_graph = use_graph
        self._graphs = None
        self._graph_cache = {}          # key -> captured step; a few recurring shapes (e.g. the smaller last batch of an epoch,
        self._graph_cache_max = max(1, int(graph_cache_max if graph_cache_max is not None      # alternating truncation regimes)
                                           else os.environ.get("POPCORN_GRAPH_CACHE_MAX", "6")))  # replay instead of being re-captured
        self._static = None
        self._ctx = None                # what _forward leaves for _backward (a record; None between steps)
        self._sel_ring, self._sel_next = [], 0          # pinned host slots for the per-step selection grid (H2D without a host sync)
        self.last = {}
        self._native = None             # (handle, plan, the engine objects it was built from) of pc_train_step
        self._arena = None
        self.native_steps = 0           # eager steps that went through pc_train_step (tests / tools read it)
        self.native_units = bool(native_units)
        self.native_unit_steps = 0      # multi-unit steps that went through pc_train_step_units (native_steps counts one-unit steps only)
        self.device_units = bool(device_units)
        self.native_layer = bool(native_layer)
        self.native_single = bool(native_single)
        self.device_unit_steps = 0      # multi-unit steps that took the device-N form (eager or replayed)
        self.captures = 0               # graph captures so far (tests / tools read it)
        self._cn_ring, self._cn_next = [], 0            # pinned host slots for census_n (as the selection's ring)
        # a callable returning a context manager that a capture runs inside (None: nothing): a loader whose producer thread allocates
        # pinned or device memory hands in its pause here (data/feed.py: RegionFeed.pause) -- such a call invalidates an open capture
        self.capture_guard = None

    def __del__(self):
        nat = getattr(self, "_native", None)
        if nat is not None:
            try:
                L.lib().pc_step_destroy(nat[0])
            except Exception:
                pass

    # ------------------------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        """StepLR-style schedule hook (run_train.py:93,141): takes effect on the next step, also under graph replay."""
        self.lr = lr
        self.hyper.fill_(lr)

    # ---- optimizer state <-> checkpoints ----------------------------------------------------------------------------
    def sync_from_model(self):
        """After ``model.load_state_dict``: the parameters must still be views of the flat buffer (load_state_dict copies
        in place, so they are); re-home any that were replaced."""
        table = dict(self.model.named_parameters())
        off = 0
        for n_ in self.names:
            p = table[n_]
            k = p.numel()
            view = self.flat_p[off:off + k].view_as(p)
            if p.data.data_ptr() != view.data_ptr():
                view.copy_(p.data)
                p.data = view
            off += k
        self.model.invalidate_cache()

    def optimizer_state(self):
        return {"m": self.m.cpu(), "v": self.v.cpu(), "step": self.step_count.cpu(), "lr": self.lr,
                "names": list(self.names), "segments": list(self.segments)}

    def load_optimizer_state(self, fa):
        self.m.copy_(fa["m"])
        self.v.copy_(fa["v"])
        st = fa["step"].to(torch.int32).reshape(-1)
        if st.numel() == 1:                    # checkpoints written before the per-group counters: one shared step
            st = st.expand(3)
        self.step_count.zero_()
        self.step_count[: min(st.numel(), self.step_count.numel())].copy_(st[: self.step_count.numel()])

    def _torch_adam_index(self, param_names):
        """name -> index in torch.optim.Adam's state dict for the reference's three parameter groups
        (run_train.py:82-90): [not head.6 and not unetmodel], [unetmodel], [head.6]."""
        groups = [[n for n in param_names if n not in HEAD_NO_DECAY and "unetmodel" not in n],
                  [n for n in param_names if n not in HEAD_NO_DECAY and "unetmodel" in n],
                  [n for n in param_names if n in HEAD_NO_DECAY and "unetmodel" not in n]]
        index, i = {}, 0
        for g in groups:
            for n in g:
                index[n] = i
                i += 1
        return index, [len(g) for g in groups]

    def load_torch_adam_state(self, opt_sd, param_names):
        """Moments / steps of a ``torch.optim.Adam.state_dict()`` (the reference's checkpoint format) -> flat buffers."""
        index, _ = self._torch_adam_index(param_names)
        state = opt_sd["state"]
        steps = {0: 0, 1: 0, 2: 0}
        off = 0
        table = dict(self.model.named_parameters())
        seg_of = list(self.segments)
        for n_ in self.names:
            k = table[n_].numel()
            st = state.get(index[n_])
            if st is not None:
                self.m[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                grp = next(g for e, g in seg_of if off < e)
                steps[grp] = max(steps[grp], int(st["step"]))
            off += k
        self.step_count.zero_()
        for g, t in steps.items():
            self.step_count[g] = t

    def torch_adam_state_dict(self, param_names):
        """The flat optimizer state in ``torch.optim.Adam.state_dict()`` form for the reference's parameter groups, so a
        checkpoint written by the fused step loads into the reference trainer's optimizer (run_train.py:458-472)."""
        index, sizes = self._torch_adam_index(param_names)
        table = dict(self.model.named_parameters())
        steps = self.step_count.cpu().tolist()
        state, off = {}, 0
        seg_of = list(self.segments)
        m, v = self.m.cpu(), self.v.cpu()
        for n_ in self.names:
            p = table[n_]
            k = p.numel()
            grp = next(g for e, g in seg_of if off < e)
            if steps[grp] > 0:
                state[index[n_]] = {"step": torch.tensor(float(steps[grp])), "exp_avg": m[off:off + k].view_as(p).clone(),
                                    "exp_avg_sq": v[off:off + k].view_as(p).clone()}
            off += k
        groups, start = [], 0
        for gi, cnt in enumerate(sizes):
            groups.append({"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps,
                           "weight_decay": 0.0 if gi == 2 else self.wd, "amsgrad": False, "maximize": False, "foreach": None,
                           "capturable": False, "differentiable": False, "fused": None,
                           "params": list(range(start, start + cnt))})
            start += cnt
        return {"state": state, "param_groups": groups}

    def attach_grads(self):
        """Expose the flat gradient views as ``param.grad`` (for logging / wandb.watch-style consumers)."""
        table = dict(self.model.named_parameters())
        for n_ in self.names:
            table[n_].grad = self.grads[n_]

    # ---- native executor (one C-ABI call per eager step) ------------------------------------------------------------
    def _native_ok(self, sample):
        """Which steps pc_train_step covers (include/popcorn_hip.h): fp32, dual-stream models whose building score comes from the frozen
        extractor, with the occupancy product -- and, with ``native_layer``, a given building layer and models without the product; with
        ``native_single``, single-modality models (a one-stream plan).  Everything else keeps the per-launch engine (same kernels)."""
        m = self.model
        if not NATIVE_STEP or m.precision != "fp32" or not (m.occupancymodel or self.native_layer):
            return False
        if not (m.S1 and m.S2) and not self.native_single:
            return False               # opt-in (one-stream plan)
        if _is_multi_unit(sample) and (self.device_units or not self.native_units):
            return False               # opt-in (pc_train_step_units); pc_train_step supervises one unit per sample.  device_units: not asked
        if not (E.PADDED_INPUT and E.COMPOSED_UP and E.FUSED_LEVEL2 and E.FUSED_CONV_BWD and DEFER_HEAD_REDUCE):
            return False               # an A/B switch of the per-launch engine is off its default: that engine is what is being asked for
        if (not m.sentinelbuildings) and sample.get("building_counts") is not None and not self.native_layer:
            return False               # opt-in (pc_train_step_layer)
        return True

    def _native_handle(self):
        m = self.model
        engs = m.engines()
        # everything the C plan bakes in besides pointers: a trainer whose public attributes are reassigned after construction
        # (raw_norm by bench.py / tools / tests, the loss weights by a schedule) must not keep stepping with the stale copy
        band, mean, std = self.raw_norm
        baked = (tuple(int(b) for b in band[:6]), tuple(float(v) for v in mean[:6]), tuple(float(v) for v in std[:6]),
                 tuple(float(v) for v in self.lam4), float(self.lam_weak), float(self.sreg), float(self.clip or 0.0), float(self.wd),
                 tuple(float(b) for b in self.betas), float(self.eps), int(m.p), int(bool(m.occupancymodel)), bool(self.native_single))
        if self._native is not None and self._native[2] is engs and self._native[6] == baked:
            return self._native[0]
        if self._native is not None:
            L.lib().pc_step_destroy(self._native[0])
            self._native = None
        eng_u, eng_b = engs
        plan = L.PcStepPlan()
        keep = []
        fill_step_net(plan.unet, eng_u, self.grads, "unetmodel.", keep)
        fill_step_net(plan.extractor, eng_b, None, None, keep)
        # (one-stream plan: head_w[0] is the 64 x 8 parameter itself, not the padded image of head_tensors(): the executor embeds it)
        ht = m.head_tensors() if (m.S1 and m.S2) else [getattr(m.head[i], n_) for i in (0, 2, 4, 6) for n_ in ("weight", "bias")]
        hg = [self.grads[n_] for n_ in self.names[-8:]]
        for i in range(8):
            plan.head_w[i], plan.head_dw[i] = ht[i].data_ptr(), hg[i].data_ptr()
        plan.flat_p, plan.flat_g, plan.adam_m, plan.adam_v = (t.data_ptr() for t in (self.flat_p, self.flat_g, self.m, self.v))
        plan.n, plan.n_decay, plan.n_head = self.n, self.n_decay, sum(g.numel() for g in hg)
        plan.occupancymodel = int(bool(m.occupancymodel))
        plan.hyper_dev, plan.step_dev, plan.norm_dev = self.hyper.data_ptr(), self.step_count.data_ptr(), self.norm.data_ptr()
        plan.stats_dev, plan.loss_dev, plan.g_scale_const_dev = self.stats.data_ptr(), self.loss_out.data_ptr(), self.g_scale_const.data_ptr()
        plan.groups = ops.adam_groups(self.segments, {0, 1, 2})
        plan.weight_decay, plan.beta1, plan.beta2, plan.eps = self.wd, self.betas[0], self.betas[1], self.eps
        plan.max_norm, plan.scale_regularization, plan.lam_weak = (self.clip or 0.0), self.sreg, self.lam_weak
        for i in range(4):
            plan.lam4[i] = self.lam4[i]
        plan.extractor_pad = m.p
        band, mean, std = self.raw_norm
        for c in range(6):
            plan.band[c], plan.mean[c], plan.stdv[c] = int(band[c]), float(mean[c]), float(std[c])
        h = L.lib().pc_step_create(C.byref(plan))
        if not h:
            raise L.PopcornHipError("pc_step_create failed")
        self._native = (h, plan, engs, keep, ht, hg, baked)
        return h

    def _native_io(self, s, sel, encoder_no_grad, unet_no_grad):
        dk = data_keys(s)
        B, _, H, W = s[dk[0]].shape
        io = L.PcStepIo()
        io.B, io.H, io.W = B, H, W
        # the executor takes raw device pointers: everything the per-launch engine checks tensor by tensor (device, dtype, layout) is
        # checked here, so that a CPU tensor or a wrong dtype raises instead of faulting on the GPU / training on reinterpreted bytes
        L.require_device(*(s[k] for k in dk), s["admin_mask"], s["census_idx"], s["y"])
        units = None

        def want(key, dtype, shape=None):
            t = s[key]
            if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
                raise ValueError(f"{key}: expected a contiguous {dtype} tensor" + (f" of shape {shape}" if shape else "") +
                                 f", got {t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else " (non-contiguous)"))
        form, _ = _data_form(s, u16=True)
        if form == "split":
            want("raw_s2", torch.uint16, (B, 4, H, W))
            want("raw_s1", torch.float32, (B, 2, H, W))
            io.data_kind, io.data, io.data2 = L.PC_DATA_SPLIT, s["raw_s2"].data_ptr(), s["raw_s1"].data_ptr()
        elif form == "raw":
            want("raw", torch.float32)
            io.data_kind, io.data, io.craw = L.PC_DATA_RAW, s["raw"].data_ptr(), s["raw"].shape[1]
        elif self.model.S1 and self.model.S2:
            if s["input"].shape[1] != 6 or s["input"].dtype != torch.float32:
                raise ValueError("input must be a (B, 6, H, W) fp32 tensor")
            want("input", torch.float32, (B, 6, H, W))
            io.data_kind, io.data = L.PC_DATA_INPUT, s["input"].data_ptr()
        else:
            # one-stream plan: the model's own input (B, input_channels, H, W) -- or any tensor that holds the channels the stream picks
            # (a 6-channel tile: what the per-launch step reads of it); io.craw carries its channel count
            Cx = s["input"].shape[1]
            stream = self.model.engines()[0].streams[0]
            if Cx <= max(stream[1][:stream[2]]):
                raise ValueError(f"input: {Cx} channels, the model's stream reads channels {stream[1][:stream[2]]}")
            want("input", torch.float32, (B, Cx, H, W))
            io.data_kind, io.data, io.craw = L.PC_DATA_INPUT, s["input"].data_ptr(), Cx
        want("admin_mask", torch.float32, (B, H, W))
        io.admin_mask = s["admin_mask"].data_ptr()
        io._layer = None
        if (not self.model.sentinelbuildings) and s.get("building_counts") is not None:
            # the given building layer (pc_train_step_layer reads it where it read the extractor's score)
            if not s["building_counts"].is_cuda:
                raise ValueError(f"building_counts: expected a tensor on {self.device}, got one on {s['building_counts'].device}")
            want("building_counts", torch.float32, (B, 1, H, W))
            io._layer = s["building_counts"]            # (kept alive with the struct)
        if _is_multi_unit(s):
            # the unit lists travel in their own struct (pc_step_units); census_n is host data, default K per row
            K = s["census_idx"].shape[1]
            want("census_idx", torch.int64, (B, K))
            want("y", torch.float32, (B, K))
            counts = ops._unit_counts(s.get("census_n"), B, K)
            units = L.PcStepUnits()
            units._counts = (C.c_int32 * B)(*counts)             # (kept alive with the struct)
            units.census_idx, units.y, units.census_n = s["census_idx"].data_ptr(), s["y"].data_ptr(), units._counts
            units.K, units.N = K, sum(counts)
        else:
            want("census_idx", torch.int64, (B,))
            want("y", torch.float32, (B,))
            io.census_idx, io.y = s["census_idx"].data_ptr(), s["y"].data_ptr()
        if sel.is_cuda:
            io.sel = sel.data_ptr()
        else:                       # host flags: they travel in the kernel arguments of the executor's first launch (no H2D copy command)
            io.sel_host = sel.data_ptr()
        io.encoder_no_grad, io.unet_no_grad = int(bool(encoder_no_grad)), int(bool(unet_no_grad))
        io.inv_B = 1.0 / self.reducer.global_batch(B)
        io.dp = int(bool(self.reducer.active))
        return io if units is None else (io, units)

    def _native_call(self, h, io, phases, stream, units=None):
        """pc_train_step_layer (``units``: pc_train_step_units_layer; without a layer they are pc_train_step / pc_train_step_units) with the
        arena grown to what the geometry takes.  With ``units`` a PC_ENOTSUP is returned instead of raised: nothing was enqueued, the caller
        takes the per-launch engine."""
        lib = L.lib()
        for _ in range(2):
            if self._arena is not None:
                io.arena, io.arena_bytes = self._arena.data_ptr(), self._arena.numel()
            layer = io._layer.data_ptr() if getattr(io, "_layer", None) is not None else None      # (every phase names the same layer)
            if units is None:
                rc = lib.pc_train_step_layer(h, C.byref(io), layer, phases, stream)
            else:
                rc = lib.pc_train_step_units_layer(h, C.byref(io), C.byref(units), layer, phases, stream)
            if rc != L.PC_ENOMEM or not (phases & L.PC_STEP_FWD):
                break               # (a backward / update phase never grows the arena: the forward's activations live in it)
            # the arena grows to what this geometry takes (+ 1/8: the next region is a little larger more often than not); the old one is
            # released to torch's stream-ordered allocator, so work still in flight on it finishes first
            self._arena = None
            self._arena = torch.empty(int(io.arena_needed * 9 // 8), dtype=torch.uint8, device=self.device)
        if units is not None and rc == L.PC_ENOTSUP:
            return rc
        L.check(rc, "pc_train_step" if units is None else "pc_train_step_units")
        return rc

    def _native_step(self, s, sel, encoder_no_grad, unet_no_grad):
        """One executor step; False: a multi-unit batch the executor declines (nothing enqueued, nothing updated)."""
        h = self._native_handle()
        io = self._native_io(s, sel, encoder_no_grad, unet_no_grad)
        stream = L.stream_ptr()
        if isinstance(io, tuple):
            io, units = io
            if self._native_call(h, io, L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, stream, units) == L.PC_ENOTSUP:
                return False
            self.last = _ArenaOutputs(self._arena, io, units, layer=io._layer)
            self.native_unit_steps += 1
            return True
        if not self.reducer.active:
            self._native_call(h, io, L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, stream)
        else:
            self._native_call(h, io, L.PC_STEP_FWD, stream)
            self.reducer.reduce_stats(self.stats)
            self._native_call(h, io, L.PC_STEP_BWD, stream)
            self.reducer.reduce_grads(self.flat_g)
            self._native_call(h, io, L.PC_STEP_UPD, stream)
        self.last = _ArenaOutputs(self._arena, io, layer=io._layer)
        self.native_steps += 1
        return True

    # ---- the three stream-ordered sections -------------------------------------------------------------------------
    def _forward(self, s, sel, encoder_no_grad, unet_no_grad):
        """ingest -> building score, mask and U-Net features, in the launch order of the building source -> head -> context.  Each decision
        is taken once: the input form and the one-launch ingest (``_ingest``), the domain (``same``), the building source (below), the mask
        kind (``_mask``: one unit / multi-unit) and the head's form (``_head``)."""
        m = self.model
        eng_u, eng_b = m.engines()
        # multi-unit supervision: the flattened unit lists; the mask is then ops.unit_mask on the building score and the head runs on the
        # union mask without a region (the N region sums follow it: ops.unit_popcount)
        lay = None
        if _is_multi_unit(s):
            lay = self._layout_dev(s) if self._device_n(s) else ops.unit_layout(s["census_idx"], s.get("census_n"))
        form, data = _data_form(s)
        B, _, H, W = data[0].shape
        pads = pt, pb, pl, pr = pad_geometry(H, W, False)
        same = pads == (m.p, m.p, m.p, m.p)      # e.g. 100x100 tiles: both networks see the same 128x128 domain
        X, Xp_all = self._ingest(form, data, pads, same)
        dom = (X, pt, pl, H + pt + pb, W + pl + pr)
        rowcol = (sel[:H], sel[H:])
        # popcorn.py:113-114: the building score comes from the frozen extractor unless the model was built with sentinelbuildings =
        # False AND the sample brings its own "building_counts" (a dataset that ships a building layer)
        given = (not m.sentinelbuildings) and s.get("building_counts") is not None
        if same and not given:
            # both networks layer by layer in shared launches; score (+ mask) from the extractor's partial logits
            (f_b, feats), (_, saved) = E.forward_multi([eng_b, eng_u], *dom, [False, not unet_no_grad], logit_only=[True, False],
                                                       Xp_all=Xp_all)
            building, mask, counts, slot = self._mask(f_b, s, rowcol, lay, window=(H, W, pt, pl))
        else:
            # the score first (given, or the extractor on its own 14-px domain), then the mask, then the trainable U-Net
            if given:
                building = s["building_counts"].contiguous().float()
                if tuple(building.shape) != (B, 1, H, W):
                    raise ValueError(f"building_counts must be (B, 1, H, W) = {(B, 1, H, W)}, got {tuple(building.shape)}")
            else:
                building = eng_b.building_score(X, m.p)
            building, mask, counts, slot = self._mask(building, s, rowcol, lay)
            if given:
                (feats,), (saved,) = E.forward_multi([eng_u], *dom, [not unet_no_grad], Xp_all=Xp_all)
            else:
                feats, saved = eng_u.forward(*dom, save=not unet_no_grad)
        s["building_counts"] = building
        if not m.occupancymodel:
            building = torch.ones_like(building)
        ctx = SimpleNamespace(feats=feats, saved=saved, building=building, mask=mask, pads=(pt, pl), shape=(B, H, W), counts=counts,
                              slot=slot, lay=lay, pc_sorted=None)          # (slot, lay, pc_sorted: multi-unit steps only)
        self._head(s, ctx)
        self._ctx = ctx

    def _ingest(self, form, data, pads, same):
        """(X, Xp_all): the normalised model input -- or, where the one-launch padded ingest applies (``_PADDED_INGEST``; both networks on
        the same padded domain, two streams), (None, the padded, normalised, stream-ordered input of both networks)."""
        if form == "input":
            return data[0], None
        band, mean, std = self.raw_norm
        if form == "split":
            # the loader's own tensors: S2 as uint16 digital numbers [R, G, B, NIR] (two thirds of the PCIe bytes of fp32), S1 fp32
            # [VV, VH]; their concatenation IS the model's channel order, so band index = model channel
            band = tuple(range(6))
        streams = self.model.engines()[0].streams
        if same and E.PADDED_INPUT and len(streams) == 2:
            pt, pb, pl, pr = pads
            op, need_pad, need_rows16 = _PADDED_INGEST[form, L.act_dtype() == torch.bfloat16]
            if (not need_pad or pt or pb or pl or pr) and (not need_rows16 or (data[0].shape[3] + pl + pr) % 4 == 0):
                order = E.stream_channel_order(streams)
                return None, getattr(ops, op)(*data, [band[c] for c in order], [mean[c] for c in order], [std[c] for c in order],
                                              pt, pb, pl, pr)
        raw = data[0] if form == "raw" else torch.cat([data[0].to(torch.float32), data[1]], 1).contiguous()
        return ops.select_normalize(raw, band, mean, std), None

    def _mask(self, src, s, rowcol, lay, window=None):
        """(building, mask, counts, slot) from the building score ``src`` -- or, with ``window`` = (H, W, pt, pl), from the extractor's
        features on the shared domain, where the one-unit form is ONE launch (``score_and_mask``).  One unit per sample (``lay`` None,
        ``slot`` None): ops.sparsity_mask; multi-unit: ops.unit_mask."""
        occ = self.model.occupancymodel
        if window is not None:
            eng_b = self.model.engines()[1]
            if lay is None:
                return (*eng_b.score_and_mask(src, *window, s["admin_mask"], s["census_idx"], *rowcol, occ), None)
            src = eng_b.score_from_features(src, *window)
        if lay is None:
            return (src, *ops.sparsity_mask(src, s["admin_mask"], s["census_idx"], *rowcol, occ), None)
        slot, mask, counts = ops.unit_mask(src, s["admin_mask"], lay["units"], lay["unit_off"], *rowcol, occ)
        return src, mask, counts, slot

    def _head(self, s, c):
        """The sparse head on the step's mask; fills ``last``.  One unit: the head reduces each sample's region (single process: popcount /
        stats are finished by the loss launch of ``_backward``; data parallel: here, for the stats all-reduce).  Multi-unit: the union
        mask, no region, stats {Nsel, sum scale} finished by the call; then the N region sums."""
        (pt, pl), (B, H, W) = c.pads, c.shape
        one = c.lay is None
        scale_map, popdense, popcount = ops.head_fwd(c.feats, pt, pl, H, W, self.model.head_tensors(), c.building, mask=c.mask,
                                                     admin_mask=s["admin_mask"] if one else None,
                                                     census_idx=s["census_idx"] if one else None, stats=self.stats,
                                                     nsel_counts=c.counts, pack_both=True,
                                                     defer_reduce=one and not self.reducer.active)
        # (building_counts: the layer the step multiplied by -- the extractor's score or the sample's own --, as the native step's outputs name it)
        self.last = {"popcount": popcount, "popdensemap": popdense, "scale_map": scale_map, "mask": c.mask,
                     "building_counts": s["building_counts"]}
        if not one and "n_dev" in c.lay:
            # device-N: the sums belong to the loss launch pair of ``_backward`` (after the stats all-reduce); their outputs exist from here
            # on, so that ``last`` names the tensors a replayed graph writes
            n = c.lay["Ncap"]
            c.popdense = popdense
            c.pc_sorted = torch.empty(n, device=self.device, dtype=torch.float32)
            self.last.update(popcount=torch.empty(n, device=self.device, dtype=torch.float32), slot=c.slot, unit_n=c.lay["n_dev"])
        elif not one:
            c.pc_sorted = ops.unit_popcount(popdense, c.slot, c.lay["N"], c.lay["unit_off"])
            self.last.update(popcount=c.pc_sorted.index_select(0, c.lay["to_caller"]), slot=c.slot)

    def _backward(self, s, encoder_no_grad, unet_no_grad):
        m, c = self.model, self._ctx
        (pt, pl), (B, H, W) = c.pads, c.shape
        g_pc = g_pd = admin = census = None
        if c.lay is not None:
            g_pd = self._unit_loss_dev(c) if "n_dev" in c.lay else self._unit_loss(s, c)
        else:
            admin, census = s["admin_mask"], s["census_idx"]
            g_pc = torch.empty(B, device=self.device, dtype=torch.float32)
            inv_B = 1.0 / self.reducer.global_batch(B)
            if self.reducer.active:
                ops.loss_fwd_bwd(self.last["popcount"], s["y"], self.stats, self.lam4, self.sreg, self.lam_weak, inv_B,
                                 self.loss_out, g_pc, self.g_scale_const)
            else:
                ops.head_popcount_loss(B, H, W, c.counts, s["y"], self.lam4, self.sreg, self.lam_weak, inv_B, self.last["popcount"], self.stats,
                                       self.loss_out, g_pc, self.g_scale_const)
        eng_u = m.engines()[0]
        hgrads = [self.grads[n_] for n_ in self.names[-8:]]
        khgrads, fix = m.head_grad_targets(hgrads)
        # the head's weight-gradient partials are finished by the U-Net backward's batched reduction launch when there is one
        hp, G = ops.head_bwd(c.feats, pt, pl, H, W, m.head_tensors(), c.building, mask=c.mask, admin_mask=admin,
                             census_idx=census, g_popcount=g_pc, g_popdense=g_pd, g_scale_const=self.g_scale_const, grads=khgrads,
                             feat_bn=None if unet_no_grad else eng_u.feat_bn(), packed=True, defer_reduce=DEFER_HEAD_REDUCE and not unet_no_grad)
        if unet_no_grad:
            self.flat_g[: self.n - sum(g.numel() for g in hgrads)].zero_()
        else:
            if encoder_no_grad:
                self.flat_g[: self.n - sum(g.numel() for g in hgrads)].zero_()
            eng_u.backward(c.saved, G, self.grads, accumulate=False, encoder_no_grad=encoder_no_grad, prefix="unetmodel.",
                           head_reduce=hp if isinstance(hp, ops.HeadPartials) else None)
        fix()                    # (single modality: the padded first-layer gradient -> the parameter's shape; after the reduction)
        self._ctx = None

    def _unit_loss(self, s, c):
        """Multi-unit step: the population loss is the mean over the N (b, k) pairs (pc_loss_fwd_bwd with B := N, inv_B = 1 / N); its
        gradient g_popcount[N] painted onto the units' pixels is the head backward's g_popdense."""
        lay, y = c.lay, s["y"].float()
        N = lay["N"]
        if tuple(y.shape) != tuple(s["census_idx"].shape):
            raise ValueError(f"y must be (B, K) like census_idx {tuple(s['census_idx'].shape)}, got {tuple(y.shape)}")
        y_sorted = y.reshape(-1)[lay["to_sorted"]]
        g_pc = torch.empty(N, device=self.device, dtype=torch.float32)
        ops.loss_fwd_bwd(c.pc_sorted, y_sorted, self.stats, self.lam4, self.sreg, self.lam_weak, 1.0 / N, self.loss_out, g_pc,
                         self.g_scale_const)
        return ops.unit_paint(g_pc, c.slot)

    def _device_n(self, s):
        """A multi-unit sample takes the device-N form: the trainer's switch, and ``census_n`` already on the device (``step`` /
        ``_graph_step`` put it there after the host's validation)."""
        return self.device_units and torch.is_tensor(s.get("census_n")) and s["census_n"].is_cuda

    def _layout_dev(self, s):
        """The device-N layout (ops.unit_layout_dev): capacity B * K, the counts read from the device tensor ``census_n``, the local N
        left in stats[2] for the stats all-reduce."""
        cidx, y = s["census_idx"], s["y"]
        if tuple(y.shape) != tuple(cidx.shape):
            raise ValueError(f"y must be (B, K) like census_idx {tuple(cidx.shape)}, got {tuple(y.shape)}")
        return ops.unit_layout_dev(cidx, y.float(), s["census_n"], stats=self.stats)

    def _unit_loss_dev(self, c):
        """``_unit_loss`` at capacity: sums, finish, scatter and loss in two launches with N and 1 / N (global, after the stats
        all-reduce) read on the device; g_popcount's tail is 0, so the paint runs with N := Ncap."""
        g_pc = torch.empty(c.lay["Ncap"], device=self.device, dtype=torch.float32)
        ops.unit_popcount_loss_dev(c.popdense, c.slot, c.lay, self.stats, self.lam4, self.sreg, self.lam_weak, self.loss_out, g_pc,
                                   self.g_scale_const, out=(c.pc_sorted, self.last["popcount"]))
        return ops.unit_paint(g_pc, c.slot)

    def _counts_to_device(self, counts, dst=None):
        """The host's valid counts -> a device int32 [B] tensor through a ring of pinned slots (``_sel_to_device``'s scheme: no pageable
        copy, no host synchronisation)."""
        n = len(counts)
        if not self._cn_ring or self._cn_ring[0][0].numel() < n:
            self._cn_ring = [(torch.empty(max(n, L.PC_UNIT_LAYOUT_MAX_B), dtype=torch.int32).pin_memory(), torch.cuda.Event())
                             for _ in range(8)]
            self._cn_next = 0
            for _, ev in self._cn_ring:
                ev.record()
        buf, ev = self._cn_ring[self._cn_next]
        self._cn_next = (self._cn_next + 1) % len(self._cn_ring)
        ev.synchronize()
        buf[:n].copy_(torch.tensor(counts, dtype=torch.int32))
        if dst is None:
            dst = torch.empty(n, dtype=torch.int32, device=self.device)
        dst.copy_(buf[:n], non_blocking=True)
        ev.record()
        return dst

    @staticmethod
    def _units_capped(B, K):
        return K > L.PC_UNIT_LAYOUT_MAX_K or B > L.PC_UNIT_LAYOUT_MAX_B

    def _sections(self, st, sel, enc_ng, unet_ng, collectives=True):
        """The step: forward -> [all-reduce {Nsel, sum scale}] -> backward -> [all-reduce the flat gradient] -> update.  The reducer's calls
        return at once in a single process; ``collectives=False``: the capture's warm-up, which must not pair with the peers' collectives."""
        self._forward(st, sel, enc_ng, unet_ng)
        if collectives:
            self.reducer.reduce_stats(self.stats)
        self._backward(st, enc_ng, unet_ng)
        if collectives:
            self.reducer.reduce_grads(self.flat_g)
        self._update(enc_ng, unet_ng)

    def _update(self, encoder_no_grad=False, unet_no_grad=False):
        active = {2} if unet_no_grad else ({1, 2} if encoder_no_grad else {0, 1, 2})
        ops.adam_clip_step_fused(self.flat_p, self.flat_g, self.m, self.v, self.n_decay, self.hyper, self.wd, self.betas[0],
                                 self.betas[1], self.eps, self.clip or 0.0, self.norm, self.step_count,
                                 groups=ops.adam_groups(self.segments, active))

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _draw_selection(H, W):
        """The two CPU-generator multinomial draws of get_sparsity_mask (popcorn.py:366-369): ``draw_selection``, the model API's draw."""
        return draw_selection(H, W)

    def _sel_to_device(self, sel_host, dst=None):
        """The per-step row / column selection (H + W bytes drawn on the CPU generator, like the reference) goes to the device
        through a ring of PINNED host slots: a ``copy_`` from pageable memory is a host synchronisation per step on every rank
        (round-2 review).  A slot is reused only after the copy that read it has completed (its event)."""
        n = sel_host.numel()
        if not self._sel_ring or self._sel_ring[0][0].numel() < n:
            self._sel_ring = [(torch.empty(max(n, 256), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(8)]
            self._sel_next = 0
            for _, ev in self._sel_ring:
                ev.record()
        buf, ev = self._sel_ring[self._sel_next]
        self._sel_next = (self._sel_next + 1) % len(self._sel_ring)
        ev.synchronize()                                  # eight steps back: complete unless the host runs far ahead
        buf[:n].copy_(sel_host)
        if dst is None:
            dst = torch.empty(n, dtype=torch.uint8, device=self.device)
        dst.copy_(buf[:n], non_blocking=True)
        ev.record()
        return dst

    def _throttle(self, depth=8):
        """Bound how far the host runs ahead of the device (what the pinned selection ring did as a side effect): at most ``depth`` steps."""
        ring = getattr(self, "_run_ahead", None)
        if ring is None:
            ring = self._run_ahead = [[torch.cuda.Event() for _ in range(depth)], 0]
            for ev in ring[0]:
                ev.record()
        ev = ring[0][ring[1]]
        ring[1] = (ring[1] + 1) % len(ring[0])
        ev.synchronize()
        ev.record()

    def step(self, sample, encoder_no_grad=False, unet_no_grad=False):
        """One optimisation step on ``sample`` = {input (B,6,H,W) normalised -- or raw (B,Craw,H,W), see ``raw_norm`` --,
        admin_mask, census_idx, y}.  Returns the device tensor loss_out[2] = {loss, regulariser} (no host sync).

        Multi-unit supervision: ``census_idx`` (B, K) int64 on the device (ids non-negative, distinct within a row), ``y`` (B, K) and optionally ``census_n`` (HOST list / CPU tensor: valid units per row, default K).  The step is the
        one-unit step on the replicated batch of N = sum(census_n) samples; ``last["popcount"]`` is (N,) in (b, k) order.  It runs
        eagerly through the per-launch engine (``native_steps`` does not count it) or, with ``native_units=True``, through
        pc_train_step_units (counted in ``native_unit_steps``; what that entry declines -- K or B beyond its caps -- falls back to the
        per-launch engine within the step).  Out of scope, and refused: ``use_graph=True`` raises ValueError, an active data-parallel
        reducer raises NotImplementedError.

        With ``device_units=True`` a multi-unit sample takes the device-N step instead -- eagerly, under ``use_graph=True`` (one capture per
        (B, K, H, W) serves every N, id list and y) and with an active reducer (the global N rides in the stats all-reduce; each rank's
        loss_out[0] is its part of the global mean plus the regulariser).  ``census_n`` stays host data and is validated here (a count
        outside [1, K] raises ValueError before anything is enqueued); it reaches the device through a pinned ring and sizes nothing:
        ``last["popcount"]`` has B * K elements, the first N in (b, k) order, the rest 0, and ``last["unit_n"]`` is N as a device int32.
        K or B beyond pc_unit_layout's caps: ValueError under a graph or a reducer (no fallback there), the host-N step otherwise."""
        dkey = data_keys(sample)[0]
        B, _, H, W = sample[dkey].shape
        counts = None
        if _is_multi_unit(sample):
            K = sample["census_idx"].shape[1]
            dev_n = self.device_units
            if dev_n and self._units_capped(B, K):
                if self.use_graph or self.reducer.active:
                    raise ValueError(f"device_units: (B, K) = {(B, K)} is beyond the layout kernel's caps ({L.PC_UNIT_LAYOUT_MAX_B}, "
                                     f"{L.PC_UNIT_LAYOUT_MAX_K}); a captured or data-parallel step has no fallback")
                dev_n = False                                      # eager, single process: the host-N step takes any K
            if not dev_n:
                if self.use_graph:
                    raise ValueError("multi-unit samples (2-D census_idx) run eagerly: build the FusedTrainStep with use_graph=False")
                if self.reducer.active:
                    raise NotImplementedError("multi-unit samples (2-D census_idx) are not supported with a data-parallel reducer")
            elif not (self.use_graph and self._static_counts(sample)):
                counts = ops._unit_counts(sample.get("census_n"), B, K)      # (raises before anything is enqueued)
        sel_host = self._draw_selection(H, W)
        if self.use_graph:
            return self._graph_step(sample, sel_host, encoder_no_grad, unet_no_grad, counts)
        s = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in sample.items() if not k.startswith("_")}
        s["admin_mask"] = s["admin_mask"].float()
        if counts is not None:
            s["census_n"] = self._counts_to_device(counts)         # from here on the step reads the counts on the device only
            self.device_unit_steps += 1
        with L.precision(self.model.precision), L.stream_scope():      # (one stream lookup for the step's ~40 launches)
            done = False
            if self._native_ok(s):
                if H + W <= L.PC_STEP_SEL_MAX:
                    self._throttle()
                    sel = sel_host                                 # (consumed during the call: no ring slot)
                else:
                    sel = self._sel_to_device(sel_host)
                done = self._native_step(s, sel, encoder_no_grad, unet_no_grad)
            if not done:                                           # (not covered, or a multi-unit batch the executor declined)
                self._sections(s, self._sel_to_device(sel_host), encoder_no_grad, unet_no_grad)
        return self.loss_out

    def _static_counts(self, sample):
        """``census_n`` of the sample IS the device tensor of one of the loader's static sets (``static_buffers(units=K)``), filled in
        place: nothing to validate on the host (the layout kernel clamps), nothing to copy."""
        cn = sample.get("census_n")
        return torch.is_tensor(cn) and cn.is_cuda and any(d.get("census_n") is cn for d in (self._static or {}).values())

    def _graph_step(self, sample, sel_host, encoder_no_grad, unet_no_grad, counts=None):
        dks = data_keys(sample)
        dkey = dks[0]
        # "_slot": which of the loader's static sets this is (static_buffers(slot=...)): every set has its own captured graph, so
        # a double-buffering loader replays graph A on set A while the copy stream fills set B -- no device-to-device copies.
        # K: the units per crop of a device-N multi-unit step (0: one unit per sample) -- the capacity B * K shapes the launches
        multi = _is_multi_unit(sample)
        key = (dkey, tuple(sample[dkey].shape), encoder_no_grad, unet_no_grad, self.model.precision, sample.get("_slot", 0),
               sample["census_idx"].shape[1] if multi else 0,
               (not self.model.sentinelbuildings) and sample.get("building_counts") is not None)
        if self._graphs is None or self._graphs[0] != key:
            if key in self._graph_cache:
                self._graphs, self.last = self._graph_cache.pop(key)      # (re-inserted below: most recently used last)
            else:
                guard = self.capture_guard() if self.capture_guard is not None else contextlib.nullcontext()
                with guard, L.precision(self.model.precision):      # the mode is read when a launch is enqueued = captured
                    try:
                        self._capture(sample, sel_host, key, counts)
                    except RuntimeError as e:
                        if not _is_oom(e):
                            raise
                        # every cached step keeps its own pool alive: let them all go and try once more with the memory back.  The
                        # loader-facing static sets are NOT part of those pools and stay (a loader keeps writing into them)
                        self._graphs = None
                        self._graph_cache.clear()
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        self._capture(sample, sel_host, key, counts)
            self._graph_cache[key] = (self._graphs, self.last)
            while len(self._graph_cache) > self._graph_cache_max:
                self._graph_cache.pop(next(iter(self._graph_cache)))
        _, st, sel, graphs = self._graphs
        extra = ("building_counts",) if key[-1] else ()          # (an input only for sentinelbuildings = False models fed a building layer)
        for k in dks + ("admin_mask", "census_idx", "y") + extra:
            if sample[k] is not st[k]:            # a loader that fills static_buffers() in place skips the copy
                st[k].copy_(sample[k], non_blocking=True)
        if multi:
            if counts is not None:                # (None: the loader filled the static set's census_n in place)
                self._counts_to_device(counts, st["census_n"])
            self.device_unit_steps += 1
        self._sel_to_device(sel_host, sel)
        graphs[0].replay()
        if len(graphs) > 1:                       # (one graph: single process, or both collectives captured inside it (RCCL))
            self.reducer.reduce_stats(self.stats)
            graphs[1].replay()
            self.reducer.reduce_grads(self.flat_g)
            graphs[2].replay()
        return self.loss_out

    @staticmethod
    def packed_layout(B, H, W, units=0):
        """The ``_packed`` byte buffer of ``static_buffers``: ({name: (byte offset, dtype, shape)}, total bytes).  units = 0: admin_mask
        f32 (B, H, W) | y f32 [B] | census_idx i64 [B], each 16-byte aligned -- the layout of every one-unit set so far.  units = K >= 1
        (multi-unit, device-N): y f32 (B, K) and census_idx i64 (B, K) in their places, then census_n i32 [B] behind them."""
        K = int(units)
        if K < 0:
            raise ValueError("units >= 0")
        al = lambda n: -(-n // 16) * 16                            # noqa: E731
        per = max(K, 1)
        shape = (B, K) if K else (B,)
        o_y = al(B * H * W * 4) if K else B * H * W * 4            # (units = 0: byte for byte the layout ``pack_small`` has always written)
        o_ci = o_y + al(B * per * 4)
        lay = {"admin_mask": (0, torch.float32, (B, H, W)), "y": (o_y, torch.float32, shape), "census_idx": (o_ci, torch.int64, shape)}
        total = o_ci + B * per * 8
        if K:
            o_cn = o_ci + al(B * K * 8)
            lay["census_n"] = (o_cn, torch.int32, (B,))
            total = o_cn + B * 4
        return lay, total

    @staticmethod
    def _packed_views(packed, lay):
        out = {}
        for name, (off, dt, shape) in lay.items():
            n = 1
            for d in shape:
                n *= d
            out[name] = packed[off:off + n * torch.empty((), dtype=dt).element_size()].view(dt).view(shape)
        return out

    def static_buffers(self, B, H, W, C=6, raw_channels=None, slot=0, split=False, building=False, units=0):
        """The device tensors the captured graph reads {input, admin_mask (float ids), census_idx, y}.  A data pipeline
        that writes its batch straight into them (e.g. ``ops.select_normalize(raw, ..., out=buf["input"])``) and passes
        this very dict to ``step`` saves the per-step input copies.  raw_channels: the data tensor is the RAW tile
        {raw (B, raw_channels, H, W)} instead of the normalised input (the graph then starts with the one-pass ingest).
        slot: independent sets for a double-buffering loader (each is captured into its own graph: H2D copies go straight into the
        idle set on a copy stream, guarded by two events, and `step(set)` replays that set's graph).
        units = K >= 1: the set of a multi-unit step (``device_units=True``): census_idx (B, K) int64, y (B, K) and census_n int32 [B]
        (1 everywhere until the loader writes it), all in the packed buffer (``packed_layout``).  K or B beyond the layout kernel's caps
        raises ValueError (a graph has no fallback)."""
        if units and self._units_capped(B, int(units)):
            raise ValueError(f"static_buffers: (B, units) = {(B, units)} is beyond the layout kernel's caps ({L.PC_UNIT_LAYOUT_MAX_B}, "
                             f"{L.PC_UNIT_LAYOUT_MAX_K})")
        dkey = "raw_s2" if split else ("input" if raw_channels is None else "raw")      # split: {raw_s2 uint16 (B,4,H,W), raw_s1 (B,2,H,W)}
        C = 4 if split else (C if raw_channels is None else raw_channels)
        if self._static is None:
            self._static = {}
        skey = (dkey, C, slot, bool(building)) + ((int(units),) if units else ())     # (a new B / H / W replaces the set of that kind: bounded memory with varying tile sizes)
        cur = self._static.get(skey)
        if cur is None or tuple(cur[dkey].shape) != (B, C, H, W):
            dev = self.device
            # the small tensors are views of ONE packed byte buffer ("_packed": admin_mask f32 | y f32 | census_idx i64 [| census_n i32],
            # each 16-byte aligned): a loader that stages a batch elsewhere moves them with a single device copy
            lay, total = self.packed_layout(B, H, W, units)
            packed = torch.zeros(total, dtype=torch.uint8, device=dev)
            small = self._packed_views(packed, lay)
            if units:
                small["census_n"].fill_(1)
            if split:
                # both tensors are views of ONE byte buffer ("_rawpacked": uint16 S2 | fp32 S1, 16-byte aligned): one H2D copy per batch
                n2 = -(-B * 4 * H * W * 2 // 16) * 16
                rp = torch.zeros(n2 + B * 2 * H * W * 4, dtype=torch.uint8, device=dev)
                data = {"raw_s2": rp[:B * 4 * H * W * 2].view(torch.uint16).view(B, 4, H, W),
                        "raw_s1": rp[n2:].view(torch.float32).view(B, 2, H, W), "_rawpacked": rp}
            else:
                data = {dkey: torch.zeros(B, C, H, W, device=dev)}
            if building:
                data["building_counts"] = torch.zeros(B, 1, H, W, device=dev)
            cur = self._static[skey] = {**data, "_slot": slot, **small, "_packed": packed}
        return cur

    @staticmethod
    def pack_split(s2_u16, s1):
        """Host-side counterpart of the ``_rawpacked`` layout of ``static_buffers(split=True)`` (one byte tensor)."""
        n2 = -(-s2_u16.numel() * 2 // 16) * 16
        out = torch.zeros(n2 + s1.numel() * 4, dtype=torch.uint8)
        out[:s2_u16.numel() * 2].view(torch.uint16).copy_(s2_u16.reshape(-1))
        out[n2:].view(torch.float32).copy_(s1.float().reshape(-1))
        return out

    @staticmethod
    def pack_small(admin_mask, y, census_idx, census_n=None):
        """Host-side counterpart of the ``_packed`` layout of ``static_buffers`` (one byte tensor).  A 2-D census_idx (B, K) with
        ``census_n`` (B counts): the ``units=K`` layout."""
        if census_idx.dim() == 2:
            B, K = census_idx.shape
            lay, total = FusedTrainStep.packed_layout(B, admin_mask.shape[-2], admin_mask.shape[-1], K)
            out = torch.zeros(total, dtype=torch.uint8)
            v = FusedTrainStep._packed_views(out, lay)
            v["admin_mask"].copy_(admin_mask.float().reshape(v["admin_mask"].shape))
            v["y"].copy_(y.float().reshape(B, K))
            v["census_idx"].copy_(census_idx.to(torch.int64))
            v["census_n"].copy_(torch.as_tensor([K] * B if census_n is None else census_n, dtype=torch.int32).reshape(B))
            return out
        B = y.numel()
        n_am, n_y = admin_mask.numel() * 4, -(-B * 4 // 16) * 16
        out = torch.zeros(n_am + n_y + B * 8, dtype=torch.uint8)
        out[:n_am].view(torch.float32).copy_(admin_mask.float().reshape(-1))
        out[n_am:n_am + B * 4].view(torch.float32).copy_(y.float().reshape(-1))
        out[n_am + n_y:].view(torch.int64).copy_(census_idx.to(torch.int64).reshape(-1))
        return out

    def _capture(self, sample, sel_host, key, counts=None):
        dkey, _, enc_ng, unet_ng = key[:4]
        # (census_n: host data in the public interface -- a loader may fill a static set in place and still pass its counts as a list)
        mine = [d for d in (self._static or {}).values() if all(sample.get(k) is d[k] for k in d if k != "census_n")]
        if mine:
            st = dict(mine[0])
        else:
            st = {k: sample[k].detach().clone().contiguous() for k in data_keys(sample) + ("admin_mask", "census_idx", "y")}
            st["admin_mask"] = st["admin_mask"].float()
        if _is_multi_unit(sample):
            # the device-N step: y as fp32 (B, K); the counts in a static int32 [B] tensor that ``_graph_step`` rewrites before every replay
            st["y"] = st["y"].float()
            if tuple(st["y"].shape) != tuple(st["census_idx"].shape) or st["census_idx"].dtype != torch.int64:
                raise ValueError(f"census_idx must be int64 (B, K) and y (B, K) alike, got {st['census_idx'].dtype} "
                                 f"{tuple(st['census_idx'].shape)} and {tuple(st['y'].shape)}")
            if st.get("census_n") is None or not (torch.is_tensor(st["census_n"]) and st["census_n"].is_cuda):
                st["census_n"] = torch.ones(st["census_idx"].shape[0], dtype=torch.int32, device=self.device)
            if counts is not None:
                self._counts_to_device(counts, st["census_n"])
        if key[-1] and "building_counts" not in st:
            # a sample that brings its own building layer (sentinelbuildings = False models, popcorn.py:113-114; key[-1]) -- also with a
            # static set built without ``building=True``: the layer is an INPUT of the captured step -- it gets its own static tensor, which
            # ``_graph_step`` refreshes from the sample before every replay (round 4 dropped it for static sets: the capture then recorded
            # the frozen-extractor path and training ran on the extractor's score without an error)
            st["building_counts"] = sample["building_counts"].detach().clone().contiguous().float()
        if key[-1] and st.get("building_counts") is None:
            raise L.PopcornHipError("graph capture of a step with a given building layer needs 'building_counts' among its static inputs")
        sel = sel_host.to(self.device)
        # warm-up on a side stream (first-launch attribute calls, workspace allocation), state restored afterwards
        snap = (self.flat_p.clone(), self.m.clone(), self.v.clone(), self.step_count.clone())
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._sections(st, sel, enc_ng, unet_ng, collectives=False)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.flat_p.copy_(snap[0]); self.m.copy_(snap[1]); self.v.copy_(snap[2]); self.step_count.copy_(snap[3])
        graphs = []
        if not self.reducer.active or self.reducer.capturable():
            # ONE graph for the whole step.  Data parallel on RCCL: the two collectives ({Nsel, sum scale}: 16 bytes; the flat
            # gradient: 157 KB) are captured as nodes of the same graph -- no graph boundary and no eager collective launch
            # between the three sections (POPCORN_DP_ONE_GRAPH=0 or a backend that cannot be captured: the split form below)
            ok = True
            try:
                g = torch.cuda.CUDAGraph()
                with _capturing(g):
                    self._sections(st, sel, enc_ng, unet_ng)
                graphs = [g]
            except RuntimeError as e:
                # only a failed CAPTURE of the collectives falls back; programming errors propagate.  An allocation failure of a
                # single-process step propagates too (``_graph_step`` frees the cached steps and retries); with peers it counts as
                # "not ok" in the handshake below instead -- a rank that re-raised here would leave its peers blocked in that
                # all-reduce, and its own retry would then issue a second one that pairs with nothing
                if not self.reducer.active:
                    raise
                torch.cuda.synchronize()
                if _is_oom(e):
                    torch.cuda.empty_cache()
                ok, graphs = False, []
            if self.reducer.active:
                # every rank must replay the same structure (one graph with captured collectives vs three graphs with eager
                # collectives between them issue different collective sequences): agree, and fall back TOGETHER
                if not self.reducer.all_agree(ok):
                    self.reducer.capture_failed = True
                    graphs = []
        if not graphs:
            g0, g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with _capturing(g0):
                self._forward(st, sel, enc_ng, unet_ng)
            pool = g0.pool()
            with _capturing(g1, pool=pool):
                self._backward(st, enc_ng, unet_ng)
            with _capturing(g2, pool=pool):
                self._update(enc_ng, unet_ng)
            graphs = [g0, g1, g2]
        self._graphs = (key, st, sel, graphs)
        self.captures += 1
