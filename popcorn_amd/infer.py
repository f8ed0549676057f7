"""Native forward executor: ``model(sample, padding=False)`` in eval mode under ``no_grad`` -- frozen extractor, trainable U-Net, dense
head -- as ONE C-ABI call (``pc_forward``, include/popcorn_hip.h) instead of one ctypes launch at a time.  Opt-in per model:

    model.native_forward = True        # default False; model.native_forwards counts the calls that took the executor

``POPCORN.forward`` routes a call here only when ``route_ok`` holds; every other call takes the per-launch engine unchanged (same
kernels) and leaves the counter alone.  Still declined: bf16 precision, single-modality (S1-only / S2-only) models, ``sparse=True``,
``padding=True``, a 2-D ``census_idx``, calls that build an autograd graph, an ``input`` that is not a contiguous fp32 (B, 6, H, W)
tensor, and an engine whose A/B switches are off their defaults.  (The TRAINING executor takes a single-modality model as a one-stream
plan -- ``FusedTrainStep(native_single=True)`` --; ``pc_forward`` keeps refusing such a plan with PC_ENOTSUP and this module keeps
declining the model: tests/test_gpu_native_forward.py pins both.)

The outputs (``popcount``, ``popdensemap``, ``scale`` and the extractor's ``building_counts``) are VIEWS into the model's own arena:
valid until that model's next native forward.  ``evaluate_raster`` and ``validate_weak`` copy what they keep.  Every model has an arena
of its own, so the score of ensemble member 0, handed to member j as its layer, is never in memory that member j's call writes.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import engine as E

_LAYER_TAGS = ("inc1", "inc2", "d1a", "d1b", "d2a", "d2b", "up2a", "up2b", "up1a", "up1b")      # pc_step_stream's layer order
_CONVT_TAGS = ("up2t", "up1t")


def engine_switches_default():
    """The A/B switches of the per-launch engine at their defaults (train.py: FusedTrainStep._native_ok asks the same): with one of them
    off, that engine is what is being asked for."""
    from . import train as T
    return bool(E.PADDED_INPUT and E.COMPOSED_UP and E.FUSED_LEVEL2 and E.FUSED_CONV_BWD and T.DEFER_HEAD_REDUCE)


def route_ok(model, inputs, need_grad, sparse, padding, switches_default=None):
    """May this ``POPCORN.forward`` call take the executor?  Attributes only -- nothing here touches a device; tensors are validated
    (device, dtype, shape: ``NativeForward._io``) after the decision."""
    if not getattr(model, "native_forward", False) or need_grad or sparse or padding:
        return False
    if model.precision != "fp32" or not (model.S1 and model.S2):
        return False
    X = inputs.get("input")
    if not torch.is_tensor(X) or X.dim() != 4 or X.shape[1] != 6 or X.dtype != torch.float32 or not X.is_contiguous():
        return False
    cidx = inputs.get("census_idx")
    if cidx is not None and not (torch.is_tensor(cidx) and cidx.dim() == 1):
        return False               # (a 2-D census_idx is the multi-unit entry form: units.hip behind the per-launch engine)
    return engine_switches_default() if switches_default is None else bool(switches_default)


class ForwardOutputs(dict):
    """The result dict of a native forward, with the call's numbers: ``launches``, ``arena_needed``."""
    launches = 0
    arena_needed = 0


class NativeForward:
    """Per model: the inference handle (a ``pc_step_plan`` without gradient / optimiser / loss pointers), the arena and the tensors whose
    pointers the plan holds.  The handle holds pointers, not copies: a forward after an optimiser step sees the new weights.  It is
    rebuilt when ``model.engines()`` is a new object (``load_state_dict``, ``.to``, ``invalidate_cache``) or a baked constant changes."""

    def __init__(self, model):
        from .data import stats
        self.model = model
        self.raw_norm = (stats.BAND6, stats.MEAN6, stats.STD6)      # the raw-tile ingest of PC_DATA_RAW / PC_DATA_SPLIT callers
        self._native = None
        self._arena = None
        self.last_io = None

    def close(self):
        if self._native is not None:
            L.lib().pc_step_destroy(self._native[0])
            self._native = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # a copied or pickled model gets an executor of its own: the handle and the arena belong to this one
    def __getstate__(self):
        return {"model": self.model, "raw_norm": self.raw_norm}

    def __setstate__(self, state):
        self.model, self.raw_norm = state["model"], state["raw_norm"]
        self._native = self._arena = self.last_io = None

    def handle(self):
        m = self.model
        engs = m.engines()
        band, mean, std = self.raw_norm
        baked = (tuple(int(b) for b in band[:6]), tuple(float(v) for v in mean[:6]), tuple(float(v) for v in std[:6]), int(m.p),
                 int(bool(m.occupancymodel)))
        if self._native is not None and self._native[2] is engs and self._native[5] == baked:
            return self._native[0]
        self.close()
        if not (m.S1 and m.S2):
            raise L.PopcornHipError("pc_forward takes dual-stream (S1 + S2) models only")
        eng_u, eng_b = engs
        plan = L.PcStepPlan()              # (zeroed: every gradient / optimiser / loss / statistics pointer stays NULL)
        keep = []

        def fill(net, eng):
            for si, (sname, chmap, cin, f0) in enumerate(eng.streams):
                st = net.s[si]
                for li, tag in enumerate(_LAYER_TAGS):
                    lay = eng.layers[(sname, tag)]
                    st.w[li] = lay.w.data_ptr()
                    st.bn[li] = lay.bn
                    keep.append(lay)
                for ti, tag in enumerate(_CONVT_TAGS):
                    lay = eng.layers[(sname, tag)]
                    st.wt[ti], st.bt[ti] = lay.w.data_ptr(), lay.b.data_ptr()
                    keep.append(lay)
                for c in range(4):
                    st.chan[c] = chmap[c]
                st.cin, st.feat_c0 = cin, f0
            net.fusion_w = eng.fusion_w.data_ptr()
            net.fusion_b = eng.fusion_b.data_ptr()

        fill(plan.unet, eng_u)
        fill(plan.extractor, eng_b)
        ht = m.head_tensors()
        for i in range(8):
            plan.head_w[i] = ht[i].data_ptr()
        plan.occupancymodel = int(bool(m.occupancymodel))
        plan.extractor_pad = m.p
        for c in range(6):
            plan.band[c], plan.mean[c], plan.stdv[c] = int(band[c]), float(mean[c]), float(std[c])
        h = L.lib().pc_step_create(C.byref(plan))
        if not h:
            raise L.PopcornHipError("pc_step_create failed")
        self._native = (h, plan, engs, keep, ht, baked)
        return h

    # ---- one call ---------------------------------------------------------------------------------------------------------------------
    def _io(self, s):
        """The call's descriptor from a sample dict: ``input`` (B, 6, H, W) fp32, or ``raw`` (B, C, H, W) fp32, or ``raw_s2`` uint16 +
        ``raw_s1`` fp32; optional ``admin_mask`` + 1-D ``census_idx``; optional ``building_counts`` for a model without
        ``sentinelbuildings``.  Everything the per-launch engine checks tensor by tensor is checked here: a CPU tensor or a wrong dtype
        raises, naming the key, instead of faulting on the GPU."""
        dev = self.model.engines()[0].device
        io = L.PcFwdIo()
        keep = []

        def want(key, dtype, shape=None):
            t = s[key]
            if not torch.is_tensor(t) or t.device != dev:
                raise ValueError(f"{key}: expected a tensor on {dev}, got " + (f"one on {t.device}" if torch.is_tensor(t) else type(t).__name__))
            if t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
                raise ValueError(f"{key}: expected a contiguous {dtype} tensor" + (f" of shape {shape}" if shape else "") +
                                 f", got {t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else " (non-contiguous)"))
            keep.append(t)
            return t.data_ptr()

        if s.get("raw_s2") is not None:
            B, _, H, W = s["raw_s2"].shape
            io.data_kind, io.data, io.data2 = L.PC_DATA_SPLIT, want("raw_s2", torch.uint16, (B, 4, H, W)), want("raw_s1", torch.float32, (B, 2, H, W))
        elif s.get("raw") is not None:
            B, craw, H, W = s["raw"].shape
            io.data_kind, io.data, io.craw = L.PC_DATA_RAW, want("raw", torch.float32), craw
        else:
            if s["input"].dim() != 4 or s["input"].shape[1] != 6:
                raise ValueError(f"input: expected a (B, 6, H, W) fp32 tensor, got {tuple(s['input'].shape)}")
            B, _, H, W = s["input"].shape
            io.data_kind, io.data = L.PC_DATA_INPUT, want("input", torch.float32, (B, 6, H, W))
        io.B, io.H, io.W = B, H, W
        # the per-launch engine composes an Up block only where ITS tensors have aligned rows: every even width under padded_rows()
        # (eval.py), multiples of 4 otherwise.  Composed and plain blocks round differently; the executor takes the form that engine takes
        io.flags = 0 if L._PAD_ROWS[0] else L.PC_FWD_DENSE_ROW_RULE
        if s.get("admin_mask") is not None:
            io.admin_mask = want("admin_mask", torch.float32, (B, H, W))
            if s.get("census_idx") is None:
                raise ValueError("census_idx: admin_mask comes with a 1-D int64 census_idx")
            io.census_idx = want("census_idx", torch.int64, (B,))
        layer = None
        if (not self.model.sentinelbuildings) and s.get("building_counts") is not None:
            want("building_counts", torch.float32, (B, 1, H, W))
            layer = s["building_counts"]
        io._keep = keep
        return io, layer

    def call(self, io, layer=None):
        """``pc_forward`` with the arena grown to what the geometry takes (train.py: ``_native_call``)."""
        lib = L.lib()
        h = self.handle()
        stream = L.stream_ptr()
        lp = layer.data_ptr() if layer is not None else None
        rc = 0
        for _ in range(2):
            if self._arena is not None:
                io.arena, io.arena_bytes = self._arena.data_ptr(), self._arena.numel()
            rc = lib.pc_forward(h, C.byref(io), lp, stream)
            if rc != L.PC_ENOMEM:
                break
            # (+ 1/8: the next window or region is a little larger more often than not; the old arena goes back to torch's stream-ordered
            # allocator, so work still in flight on it finishes first)
            self._arena = None
            self._arena = torch.empty(int(io.arena_needed * 9 // 8), dtype=torch.uint8, device=self.model.engines()[0].device)
        L.check(rc, "pc_forward")
        self.last_io = io
        return rc

    def view(self, io, off, shape):
        n = 4
        for d in shape:
            n *= d
        return self._arena[off:off + n].view(torch.float32).view(shape)

    def forward(self, s):
        """The model's output dict (+ ``building_counts``: the extractor's score, or the sample's layer)."""
        io, layer = self._io(s)
        with L.precision(self.model.precision):
            self.call(io, layer)
        B, H, W = io.B, io.H, io.W
        out = ForwardOutputs(popcount=self.view(io, io.off_popcount, (B,)), popdensemap=self.view(io, io.off_popdense, (B, H, W)),
                             scale=self.view(io, io.off_scale, (B, H, W)) if self.model.occupancymodel else None)
        out["building_counts"] = layer if io.off_building < 0 else self.view(io, io.off_building, (B, 1, H, W))
        out.launches, out.arena_needed = int(io.launches), int(io.arena_needed)
        return out


def native_forward(model, inputs):
    """``POPCORN.forward``'s executor leg (``route_ok`` held): the reference's output dict, with ``inputs["building_counts"]`` set to the
    score the pass used, as ``create_building_score`` leaves it."""
    nf = getattr(model, "_native_fwd", None)
    if nf is None:
        nf = NativeForward(model)
        object.__setattr__(model, "_native_fwd", nf)
    model.building_extractor.eval()
    model.unetmodel.freeze_bn_layers()
    out = nf.forward(inputs)
    inputs["building_counts"] = out.pop("building_counts")
    model.native_forwards += 1
    return out
