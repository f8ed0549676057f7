"""HIP execution engine for the dual-stream U-Net (forward, building score, backward).

Orchestrates the kernels of libpopcorn_hip.so for the computation the reference expresses as
``DualStreamUNet.forward`` / ``UNet.forward`` / ``DoubleConv`` / ``Down`` / ``Up``
(model/DDA_model/utils/networks.py:121-151,192-237,253-320) and its autograd backward.  Fusions relative to the
reference's op list:

  * reflect padding + channel reorder (popcorn.py:231-258,130-134) -> loader of the first conv
  * Conv2d + BatchNorm2d(eval) + ReLU -> one kernel (BN folded in the epilogue; BN is frozen, networks.py:184-189)
  * MaxPool2d(2) -> loader of the next conv;  its backward -> epilogue of that conv's data-gradient
  * torch.cat([skip, up]) + Up's zero F.pad -> two-source loader (no concat buffer)
  * ReLU/BN backward -> epilogue of the kernel that produces the gradient (no elementwise passes)
  * the two streams write straight into the 16-channel feature map (no final cat)

All launches go to the current torch stream, so a whole step can be captured into one HIP graph
(``torch.cuda.graph``) and replayed.  There is no non-HIP path.
"""
from __future__ import annotations

import collections
import os

import torch

from . import _lib as L
from . import ops

BN_EPS = 1e-5
STREAMS = (("sar_stream", (4, 5, 0, 0), 2, 0), ("optical_stream", (2, 1, 0, 3), 4, 8))   # name, chmap, Cin, feat ch0

# (tag, conv key, bn key) per stream, relative to the stream prefix
CONVS = {
    "inc1": ("inc.conv.conv.0", "inc.conv.conv.1"),
    "inc2": ("inc.conv.conv.3", "inc.conv.conv.4"),
    "d1a": ("down_seq.down1.mpconv.1.conv.0", "down_seq.down1.mpconv.1.conv.1"),
    "d1b": ("down_seq.down1.mpconv.1.conv.3", "down_seq.down1.mpconv.1.conv.4"),
    "d2a": ("down_seq.down2.mpconv.1.conv.0", "down_seq.down2.mpconv.1.conv.1"),
    "d2b": ("down_seq.down2.mpconv.1.conv.3", "down_seq.down2.mpconv.1.conv.4"),
    "up2a": ("up_seq.up2.conv.conv.0", "up_seq.up2.conv.conv.1"),
    "up2b": ("up_seq.up2.conv.conv.3", "up_seq.up2.conv.conv.4"),
    "up1a": ("up_seq.up1.conv.conv.0", "up_seq.up1.conv.conv.1"),
    "up1b": ("up_seq.up1.conv.conv.3", "up_seq.up1.conv.conv.4"),
}
CONVTS = {"up2t": "up_seq.up2.up", "up1t": "up_seq.up1.up"}
ENCODER = ("inc1", "inc2", "d1a", "d1b", "d2a", "d2b")


def trainable_names(prefix="unetmodel.", streams=("sar_stream", "optical_stream")):
    """The 48 U-Net tensors that receive a gradient in the reference train step (conv / convT weights + biases of
    both streams; BN affine frozen, out-convs unused).  SURVEY.md section 8a row 18."""
    names = []
    for s, _, _, _ in STREAMS:
        if s not in streams:
            continue
        for tag in ("inc1", "inc2", "d1a", "d1b", "d2a", "d2b"):
            names += [f"{prefix}{s}.{CONVS[tag][0]}.weight", f"{prefix}{s}.{CONVS[tag][0]}.bias"]
        names += [f"{prefix}{s}.{CONVTS['up2t']}.weight", f"{prefix}{s}.{CONVTS['up2t']}.bias"]
        for tag in ("up2a", "up2b"):
            names += [f"{prefix}{s}.{CONVS[tag][0]}.weight", f"{prefix}{s}.{CONVS[tag][0]}.bias"]
        names += [f"{prefix}{s}.{CONVTS['up1t']}.weight", f"{prefix}{s}.{CONVTS['up1t']}.bias"]
        for tag in ("up1a", "up1b"):
            names += [f"{prefix}{s}.{CONVS[tag][0]}.weight", f"{prefix}{s}.{CONVS[tag][0]}.bias"]
    return names


# data gradient + weight gradient of a conv layer in one launch (bf16 mode: every layer; fp32 mode: the 8 -> 8 layers);
# POPCORN_FUSED_CONV_BWD=0: separate launches (A/B switch)
FUSED_CONV_BWD = os.environ.get("POPCORN_FUSED_CONV_BWD", "1") != "0"
# fp32: the whole 32 x 32 level (down2's DoubleConv + up2's transposed conv) in one launch (POPCORN_FUSED_LEVEL2=0: three launches)
FUSED_LEVEL2 = os.environ.get("POPCORN_FUSED_LEVEL2", "1") != "0"
FUSED_LEVEL2_BWD = os.environ.get("POPCORN_FUSED_LEVEL2_BWD", "1") != "0"      # (A/B of the backward launch alone)
# fp32: the first conv of an Up block reads the LOW-resolution map through composed (transposed conv o conv) weights instead of an
# up-sampled tensor (POPCORN_COMPOSED_UP=0: transposed-conv launch + two-source conv)
COMPOSED_UP = os.environ.get("POPCORN_COMPOSED_UP", "1") != "0"
# Not environment switches any more (round 6: their losing sides were rejected with numbers in rounds 2-4, DESIGN_HISTORY.md): module
# constants that tests monkeypatch to reach the launches the geometry conditions fall back to anyway --
# bf16: up1's transposed conv in the epilogue of up2's second conv (False: the separate launch an odd-sized map takes)
FUSED_UPT = True
# padded + channel-gathered input materialised once per forward pass (False: the reflect loaders a row width not divisible by 4 takes)
PADDED_INPUT = True


class _Layer:
    __slots__ = ("w", "b", "bn", "bn_nobias", "wname", "bname", "_keep", "_slices")

    def __init__(self, T, conv_key, bn_key):
        self.wname, self.bname = conv_key + ".weight", conv_key + ".bias"
        self.w, self.b = T[self.wname], T[self.bname]
        if bn_key is not None:
            g, be, m, v = (T[bn_key + "." + n] for n in ("weight", "bias", "running_mean", "running_var"))
            self.bn = L.bn(self.b, g, be, m, v, BN_EPS)
            self.bn_nobias = L.bn(None, g, be, m, v, BN_EPS)
            self._keep = (g, be, m, v)
        else:
            self.bn = self.bn_nobias = None
            self._keep = ()
        self._slices = {}

    def bn_slice(self, c0, n):
        """The ReLU / BN factor descriptor (no conv bias) of channels [c0, c0 + n) of this layer's output -- for launches that take one
        8-channel column block of it as a problem of its own."""
        key = (c0, n)
        if key not in self._slices:
            g, be, m, v = self._keep
            self._slices[key] = L.bn(None, g[c0:c0 + n], be[c0:c0 + n], m[c0:c0 + n], v[c0:c0 + n], BN_EPS)
        return self._slices[key]


class UNetEngine:
    """Executes one DualStreamUNet on the HIP kernels.  ``tensors``: name -> tensor, names relative to the
    DualStreamUNet module (e.g. 'sar_stream.inc.conv.conv.0.weight').  Tensors are referenced, not copied."""

    def __init__(self, tensors, streams=("sar_stream", "optical_stream"), chmaps=None):
        """streams: which U-Net streams run (single-modality variants of popcorn.py:136-145 run one); chmaps: optional
        {stream: source-channel map} overriding the 6-channel default (a 2-channel S1 or 4-channel S2 input)."""
        self.streams = [st for st in STREAMS if st[0] in streams]
        if chmaps:
            self.streams = [(n, tuple(chmaps.get(n, cm)), ci, f0) for n, cm, ci, f0 in self.streams]
        self.layers = {}
        for s, _, _, _ in self.streams:
            for tag, (ck, bk) in CONVS.items():
                self.layers[(s, tag)] = _Layer(tensors, f"{s}.{ck}", f"{s}.{bk}")
            for tag, ck in CONVTS.items():
                self.layers[(s, tag)] = _Layer(tensors, f"{s}.{ck}", None)
        self.fusion_w = tensors.get("fusion_out_conv.conv.weight")
        self.fusion_b = tensors.get("fusion_out_conv.conv.bias")
        self.single_out = None
        if len(self.streams) == 1:        # logits of the only stream: sar_out_conv / optical_out_conv (networks.py:217-228)
            pre = "sar_out_conv" if self.streams[0][0] == "sar_stream" else "optical_out_conv"
            self.single_out = (tensors[pre + ".conv.weight"], tensors[pre + ".conv.bias"])
        dev = self.layers[(self.streams[0][0], "inc1")].w.device
        if dev.type != "cuda":
            raise L.PopcornHipError(f"popcorn_amd engine needs parameters on a HIP device, got {dev}; there is no CPU path")
        self.device = dev


    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, X, pad_top, pad_left, Hp, Wp, save=False, feats=None):
        """X: (B,6,H,W) in the dataset's channel order [R,G,B,NIR,VV,VH]; the conv domain is the reflect-padded
        (Hp,Wp) image.  Returns (features (B,16,Hp,Wp), saved activations or None)."""
        f, s = forward_multi([self], X, pad_top, pad_left, Hp, Wp, [save], [feats])
        return f[0], s[0]

    def building_score(self, X, pad=14):
        """create_building_score (popcorn.py:279-322): reflect-pad 14, frozen U-Net, fusion_out_conv, sigmoid, crop."""
        B, _, H, W = X.shape
        if self.single_out is None:
            f, _ = forward_multi([self], X, pad, pad, H + 2 * pad, W + 2 * pad, [False], logit_only=[True])
            return self.score_from_features(f[0], H, W, pad, pad)
        feats, _ = self.forward(X, pad, pad, H + 2 * pad, W + 2 * pad, save=False)
        f0 = self.streams[0][3]
        return ops.outconv_sigmoid_crop(feats[:, f0:f0 + 8], self.single_out[0], self.single_out[1], H, W, pad, pad)

    def _logit_weights(self, f):
        """fusion_out_conv's weights for the 16-channel feature map, or ones for the (B,2,.,.) partial logits that
        ``forward_multi(logit_only=...)`` returns (they only remain to be added)."""
        if f.shape[1] != 2:
            return self.fusion_w
        if getattr(self, "_ones2", None) is None or self._ones2.device != f.device:
            self._ones2 = torch.ones(2, device=f.device, dtype=torch.float32)
        return self._ones2

    def _logit_operands(self, f):
        """(source, weights, bias) of the building logit over the feature map ``f``.  Two streams: ``fusion_out_conv`` over the 16
        channels (or ones over the partial logits).  One stream: that stream's OWN out conv over its 8 channels (networks.py:217-228;
        fixture g13) -- the matching half of ``fusion_out_conv`` is another set of weights and another bias."""
        if self.single_out is None:
            return f, self._logit_weights(f), self.fusion_b
        f0 = self.streams[0][3]
        return f[:, f0:f0 + 8], self.single_out[0], self.single_out[1]

    def score_from_features(self, f, H, W, py, px):
        """out conv + sigmoid + crop from either the 16-channel feature map or the partial logits."""
        return ops.outconv_sigmoid_crop(*self._logit_operands(f), H, W, py, px)

    def score_and_mask(self, f, H, W, py, px, admin_mask, census_idx, rowsel, colsel, occupancymodel=True):
        """score_from_features + get_sparsity_mask (popcorn.py:361-377) in one launch: (building, mask, counts)."""
        return ops.building_score_mask(*self._logit_operands(f), H, W, py, px, admin_mask, census_idx, rowsel, colsel, occupancymodel)

    def feat_bn(self):
        """BN descriptors of the two layers that produce the feature map (for the head-backward epilogue)."""
        plain = L.bn()       # missing stream: its feature channels are identically zero, any scale will do
        names = [st[0] for st in self.streams]
        return (self.layers[("sar_stream", "up1b")].bn_nobias if "sar_stream" in names else plain,
                self.layers[("optical_stream", "up1b")].bn_nobias if "optical_stream" in names else plain)

    # ----------------------------------------------------------------------------------------------- backward
    def backward(self, saved, G, grads, accumulate=False, encoder_no_grad=False, prefix="", head_reduce=None, input_grad=None):
        """G: (B,16,Hp,Wp) gradient w.r.t. the conv outputs of the two up1b layers (i.e. already multiplied by
        relu-mask * bn-scale -- the head-backward epilogue does that).  Writes dW/db into ``grads[prefix+name]``
        (= or += per ``accumulate``).  encoder_no_grad: networks.py:124-132 semantics.  head_reduce: the ``ops.HeadPartials`` of the
        pass's ``head_bwd(defer_reduce=True)`` -- finished by this pass's batched reduction launch.  input_grad: a contiguous fp32
        tensor of the model input's shape to fill with the gradient w.r.t. that input (one more launch, csrc/input_grad.hip); None: the
        pass is what it was.  Under encoder_no_grad the pass ends before the encoder and the tensor is left untouched: no such gradient
        exists (networks.py:124-132 runs ``inc`` under no_grad).
        Data-gradient launches are grouped over the two streams (same shapes); weight-gradient launches are per
        stream (each owns its partial-sum workspace).  The network in reverse, one call per block (``_Backward`` below; the native
        executor's counterpart, same calls in the same order: csrc/step.hip: backward)."""
        p = _Backward(self, saved, G, grads, accumulate, encoder_no_grad, prefix, head_reduce)
        _, _, Hp, Wp = saved["geom"]
        H1, W1 = Hp // 2, Wp // 2
        H2, W2 = H1 // 2, W1 // 2
        G_f2 = {s: G[:, f0:f0 + 8] for s, _, _, f0 in self.streams}
        G_f1 = p.conv8("up1b", G_f2, "f1", "up1a", Hp, Wp)
        G_a2, G_e2 = p.up(UP1, G_f1, Hp, Wp, H1, W1, want_gz=True)
        G_e1 = p.conv8("up2b", G_e2, "e1", "up2a", H1, W1)
        G_b2, G_c2 = p.up(UP2, G_e1, H1, W1, H2, W2, want_gz=not encoder_no_grad)
        if encoder_no_grad:
            p.wb.finish()
            return
        if not p.level2(G_c2, G_b2):
            p.down(DOWN2, G_c2, G_b2, H2, W2)
        p.down(DOWN1, G_b2, G_a2, H1, W1)
        G_a1 = p.conv8("inc2", G_a2, "a1", "inc1", Hp, Wp)
        p.first_layer(G_a1, input_grad)
        p.wb.finish()


def _rows16(t):
    """planar fp32 tensor with unit column stride and every row on a 16-byte boundary"""
    return t.stride(3) == 1 and t.stride(2) % 4 == 0 and t.stride(1) % 4 == 0 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


# The blocks of the network as the backward pass walks them: layer tags and saved-activation keys.
# Up: first conv (over cat[skip | up-sampled z]) and transposed conv; c = channels of the skip tensor = of z = of the up-sampled block
_Up = collections.namedtuple("_Up", "conv convt skip skip_act up off z z_act ws c")
UP1 = _Up("up1a", "up1t", "a2", "inc2", "u1", "o1", "e2", "up2b", "ws_up1", 8)
UP2 = _Up("up2a", "up2t", "b2", "d1b", "u2", "o2", "c2", "d2b", "ws_up2", 16)
# Down: the DoubleConv behind a MaxPool2d(2); cin = channels of the pooled map (`pooled`: its saved copy, `full`: what it was pooled from)
_Down = collections.namedtuple("_Down", "conv1 conv2 mid pooled full full_act cin")
DOWN1 = _Down("d1a", "d1b", "b1", "pa2", "a2", "inc2", 8)
DOWN2 = _Down("d2a", "d2b", "c1", "pb2", "b2", "d1b", 16)


class _Backward:
    """One backward pass of a UNetEngine: its context, the launch helpers (``wgrad`` ... ``up_bwd``: one ops / WgradBatch call each, both
    streams grouped) and one function per block of the network (``conv8``, ``up``, ``level2``, ``down``, ``first_layer``), each of which
    decides its launch form where it stands.  Everything stays on the caller's stream: running the weight-gradient branch on a second
    stream next to the data-gradient chain was measured three times and lost every time (both branches are bound
    by the same memory pipe); the first stages are enqueued as the pass goes, ONE batched reduction ends it (``wb.finish``).

    Which launch a conv layer gets -- two notions, never mixed:
      ``fuse_bf16``  this run is bf16 with FUSED_CONV_BWD on: data + weight gradient of ANY layer (or column block of a concat layer, or
                     Down block's first layer with its pooling scatter) read the same two tensors -- one launch (conv3x3_bwd_group)
      ``f32_ok()``   fp32: the launcher's own predicate (pc_conv3x3_bwd_ok) takes these problems -- 8-channel input blocks, planar
                     16-byte aligned rows, the input placed at (0, 0) with the gradient's extent"""

    def __init__(self, eng, saved, G, grads, accumulate, encoder_no_grad, prefix, head_reduce):
        self.eng, self.saved, self.grads, self.prefix, self.enc_ng = eng, saved, grads, prefix, encoder_no_grad
        self.S = [s for s, _, _, _ in eng.streams]
        assert len(self.S) <= 2             # at most two problems per stream in a launch: a group takes four
        self.A = {s: saved[s] for s in self.S}
        self.B, self.dev = G.shape[0], G.device
        self.bf = L.act_dtype() == torch.bfloat16
        self.fuse_bf16 = FUSED_CONV_BWD and self.bf
        self.wb = ops.WgradBatch(self.dev, accumulate)
        self.deferred = None                # up(UP1)'s skip launch, handed to down(DOWN1): (lv, gs, g_skip, g_mid, g_pooled) -- see pool_add_plan
        self.deferred2 = None               # up(UP2)'s skip-halves launch, handed to level2(): (lv, gs, hv, g_pooled) -- see pool_add_plan2
        if head_reduce is not None:
            self.wb.head_reduce(head_reduce)

    def new(self, c, h, w):
        return {s: L.empty_act(self.B, c, h, w, self.dev) for s in self.S}

    def ly(self, s, tag):
        return self.eng.layers[(s, tag)]

    def dw(self, s, tag):
        return self.grads[self.prefix + self.ly(s, tag).wname]

    def db(self, s, tag):
        return self.grads[self.prefix + self.ly(s, tag).bname]

    def f32_ok(self, gs, xs, outs, pool_acts=None):
        return FUSED_CONV_BWD and not self.bf and all(
            ops.conv3x3_bwd_ok(gs[s], xs[s], outs[s], None if pool_acts is None else pool_acts[s]) for s in self.S)

    # ---- launch helpers
    def wgrad(self, tag, a_key, gs, b_key=None, off_key=None, **kw):
        """weight gradient of layer `tag` (b_key / off_key: the second source of a concat layer and its offset)"""
        probs = []
        for s in self.S:
            pr = {"a": self.A[s][a_key], "g": gs[s], "dw": self.dw(s, tag), "db": self.db(s, tag)}
            if b_key is not None:
                pr["b"], pr["b_offset"] = self.A[s][b_key], self.A[s][off_key]
            probs.append(pr)
        self.wb.conv3x3_group(probs, self.ly(self.S[0], tag).w.shape[0], **kw)

    def dgrad(self, tag, gs, outs, c0, cn, acts=None, act_tag=None, pool=False, acc=False):
        """data gradient of layer `tag` w.r.t. its input channels [c0, c0 + cn), masked by the producer `act_tag` of `acts`"""
        probs = []
        for s in self.S:
            pr = {"g": gs[s], "w": self.ly(s, tag).w, "out": outs[s]}
            if acts is not None:
                pr["act"] = acts[s]
                pr["act_bn"] = self.ly(s, act_tag).bn_nobias
            probs.append(pr)
        ops.conv3x3_dgrad_group(probs, c0, cn, pool=pool, accumulate=acc)
        return outs

    def bwd8(self, tag, gs, x_key, act_tag, outs, cin_total=8, pool_key=None, accumulate=False, pool_grads=None):
        """data + weight gradient of layer `tag` in one launch.  pool_key: a Down block's first layer -- x is the saved pooled map,
        outs the (accumulated) gradient of the full-resolution map it was pooled from.  act_tag None: the raw data gradient (no ReLU / BN
        factor).  pool_grads: the pool-add form -- x also went through a max-pool, outs receives the scatter of these raw gradients of
        its pooled copy in the same pass"""
        probs = []
        for s in self.S:
            pr = {"g": gs[s], "x": self.A[s][x_key], "w": self.ly(s, tag).w, "out": outs[s], "dw": self.dw(s, tag), "db": self.db(s, tag),
                  "x_bn": None if act_tag is None else self.ly(s, act_tag).bn_nobias}
            if pool_key is not None:
                pr["pool_act"] = self.A[s][pool_key]
            if pool_grads is not None:
                pr["pool_grad"] = pool_grads[s]
            probs.append(pr)
        self.wb.conv3x3_bwd_group(probs, cin_total, 0, accumulate=accumulate)
        return outs

    def halves(self, gs, x_key, outs):
        """fp32: the two 8-channel halves of a layer's 16-channel input and of its gradient, per stream: [(x half, out half)] * 2 -- or
        None where the fused backward does not take them as problems (asked of the second half: the first is aligned wherever it is)"""
        hv = {s: [(self.A[s][x_key][:, c:c + 8], outs[s][:, c:c + 8]) for c in (0, 8)] for s in self.S}
        return hv if self.f32_ok(gs, {s: hv[s][1][0] for s in self.S}, {s: hv[s][1][1] for s in self.S}) else None

    def bwd_halves(self, tag, gs, hv, act_tag, cin_total, pool_grads=None):
        """fp32: a layer with a 16-channel input as ONE launch of the fused 8-channel backward (round 4) -- the two halves are two
        problems per stream over the same gradient (it comes out of L2 once), each writing its half of the data gradient and its
        column block of the weight gradient.  pool_grads: the pool-add form, each half with its 8-channel slice of the pooled gradient"""
        probs = []
        for s in self.S:
            for i, (x, out) in enumerate(hv[s]):
                probs.append({"g": gs[s], "x": x, "w": self.ly(s, tag).w, "out": out, "dw": self.dw(s, tag),
                              "db": self.db(s, tag) if i == 0 else None, "x_bn": self.ly(s, act_tag).bn_slice(8 * i, 8), "c0_add": 8 * i})
                if pool_grads is not None:
                    probs[-1]["pool_grad"] = pool_grads[s][:, 8 * i:8 * i + 8]
        self.wb.conv3x3_bwd_group(probs, cin_total, 0)

    def bwd_cat(self, lv, gs, g_skip, g_up):
        """both column blocks of a concat layer (networks.py:318: [skip | up]) in ONE launch: same g, the skip block masked by
        its producer, the up-sampled block placed at its offset, unmasked and without a second bias gradient"""
        probs = []
        for s in self.S:
            probs.append({"g": gs[s], "x": self.A[s][lv.skip], "w": self.ly(s, lv.conv).w, "out": g_skip[s], "dw": self.dw(s, lv.conv),
                          "db": self.db(s, lv.conv), "x_bn": self.ly(s, lv.skip_act).bn_nobias})
        for s in self.S:
            probs.append({"g": gs[s], "x": self.A[s][lv.up], "w": self.ly(s, lv.conv).w, "out": g_up[s], "dw": self.dw(s, lv.conv),
                          "db": None, "x_offset": self.A[s][lv.off], "c0_add": lv.c})
        self.wb.conv3x3_bwd_group(probs, 2 * lv.c, 0)

    def convt_bwd(self, tag, x_key, act_tag, gs, outs):
        """transposed conv `tag`: weight gradient + (outs not None) data gradient masked by x's producer `act_tag` -- one launch when the
        fused form applies (bf16: always; fp32: aligned tensors, W % 16 == 0), else the two grouped launches"""
        S, ly = self.S, self.ly
        xs = {s: self.A[s][x_key] for s in S}
        if outs is not None and FUSED_CONV_BWD and (self.bf or all(
                xs[s].shape[3] % 16 == 0 and _rows16(xs[s]) and _rows16(gs[s]) and _rows16(outs[s]) for s in S)):
            self.wb.convt2x2_bwd_group([{"x": xs[s], "g": gs[s], "w": ly(s, tag).w, "out": outs[s], "x_bn": ly(s, act_tag).bn_nobias,
                                         "dw": self.dw(s, tag), "db": self.db(s, tag)} for s in S])
            return
        self.wb.convt2x2_group([{"x": xs[s], "g": gs[s], "dw": self.dw(s, tag), "db": self.db(s, tag)} for s in S])
        if outs is not None:
            ops.convt2x2_dgrad_group([{"g": gs[s], "w": ly(s, tag).w, "out": outs[s], "act": xs[s], "act_bn": ly(s, act_tag).bn_nobias}
                                      for s in S])

    def up_bwd(self, lv, gs, gz):
        """composed Up block (the forward never made the up-sampled tensor): gradient of the conv's up-sampled weight half, of the
        transposed conv's weight / bias, and (gz) of the low-resolution map, from one pass over gs"""
        ly = self.ly
        self.wb.up_bwd_group([{"g": gs[s], "z": self.A[s][lv.z], "z_bn": ly(s, lv.z_act).bn_nobias, "gz": None if gz is None else gz[s],
                               "w": ly(s, lv.conv).w, "wt": ly(s, lv.convt).w, "bt": ly(s, lv.convt).b, "fwd_ws": self.A[s][lv.ws],
                               "dw": self.dw(s, lv.conv), "dwt": self.dw(s, lv.convt), "dbt": self.db(s, lv.convt)} for s in self.S])

    def pool_add_plan(self, lv, gs, g_skip, h, w):
        """fp32, level 1, encoder trained: may the skip launch of the Up block wait for the Down block that pooled the same map, and add
        that block's max-pool scatter in its own epilogue (one write of the map's gradient instead of a write and a read-modify-write)?
        Yes where today's fused pair of the Down block applies (asked of tensors allocated as the pass allocates them), its first layer
        runs as a plain launch into a pooled-resolution gradient, and the launcher takes the skip launch with that operand.  Returns
        (g_mid, g_pooled) -- the Down block's two gradient maps, allocated here -- or None.  csrc/step.hip: Backward::pool_add_plan asks
        the same predicates."""
        S, A, dn = self.S, self.A, DOWN1
        if self.enc_ng or self.bf or lv is not UP1 or not all(A[s].get(dn.pooled) is not None for s in S):
            return None
        h1, w1 = h // 2, w // 2
        g_out, g_mid, g_pooled = self.new(16, h1, w1), self.new(16, h1, w1), self.new(dn.cin, h1, w1)
        pooled, fulls = {s: A[s][dn.pooled] for s in S}, {s: A[s][dn.full] for s in S}
        if not (self.f32_ok(g_mid, pooled, g_skip, fulls) and self.halves(g_out, dn.mid, g_mid) and self.f32_ok(g_mid, pooled, g_pooled)):
            return None
        if not all(ops.conv3x3_bwd_pool_add_ok(gs[s], A[s][lv.skip], g_skip[s], g_pooled[s]) for s in S):
            return None
        return g_mid, g_pooled

    def level2_ok(self, g_out, g_in):
        S, A = self.S, self.A
        return FUSED_LEVEL2 and FUSED_LEVEL2_BWD and all(
            A[s].get("pb2") is not None and ops.level2_bwd_ok(g_out[s], A[s]["c1"], A[s]["pb2"], A[s]["b2"], g_in[s]) for s in S)

    def pool_add_plan2(self, gs, hv, g_skip, gz):
        """fp32, level 2, encoder trained: the same exchange one level down -- where the whole-level kernel will take the 32 x 32 level
        (level2_ok, asked of the tensors it will get) and the launcher takes both skip halves with their slices of the pooled gradient,
        that kernel writes its data gradient raw (pool_grad_out) and the skip-halves launch, issued after it, adds the scatter.
        Returns the pooled gradient, or None.  csrc/step.hip: Backward::pool_add_plan2"""
        if self.bf or gz is None or not self.level2_ok(gz, g_skip):
            return None
        g_pooled = self.new(16, 32, 32)
        if not all(ops.conv3x3_bwd_pool_add_ok(gs[s], x, out, g_pooled[s][:, 8 * i:8 * i + 8])
                   for s in self.S for i, (x, out) in enumerate(hv[s])):
            return None
        return g_pooled

    # ---- the blocks (csrc/step.hip: struct Backward has the same five, over its bwd8 / bwd_halves / wgrad / dgrad / up_bwd; it has no
    # non-composed Up block -- bwd_cat / convt_bwd -- because its trainable network always runs on a domain whose levels compose)
    def conv8(self, tag, gs, x_key, act_tag, h, w):
        """an 8 -> 8 layer (second conv of a DoubleConv at full or half resolution): returns the gradient of its input"""
        outs, xs = self.new(8, h, w), {s: self.A[s][x_key] for s in self.S}
        if self.fuse_bf16 or self.f32_ok(gs, xs, outs):
            return self.bwd8(tag, gs, x_key, act_tag, outs)
        self.wgrad(tag, x_key, gs)
        return self.dgrad(tag, gs, outs, 0, 8, xs, act_tag)

    def up(self, lv, gs, h, w, hz, wz, want_gz):
        """An Up block from the gradient gs of its first conv's output at (h, w): that conv over cat[skip | up-sampled z] and the
        transposed conv that up-samples z (hz, wz).  Returns (gradient of the skip tensor, gradient of z); the first only where the
        encoder's backward will read it or the launch writes it anyway, the second only if want_gz."""
        S, A, c, enc_ng = self.S, self.A, lv.c, self.enc_ng
        composed = all(A[s].get(lv.ws) is not None for s in S)
        # (encoder_no_grad: nobody reads the skip tensor's gradient -- the composed level-1 launch writes it anyway)
        g_skip = self.new(c, h, w) if not enc_ng or (composed and c == 8) else None
        gz = self.new(c, hz, wz) if want_gz else None
        skips = {s: A[s][lv.skip] for s in S}
        if composed:
            # the skip column block: weight gradient into the first c input columns, data gradient masked by its producer
            if c == 8:          # (one launch whatever the regime: the composed forward's geometry implies the fused backward's)
                plan = self.pool_add_plan(lv, gs, g_skip, h, w)
                if plan is not None:
                    self.deferred = (lv, gs, g_skip) + plan           # down(DOWN1) issues it, behind its own first layer
                else:
                    self.bwd8(lv.conv, gs, lv.skip, lv.skip_act, g_skip, cin_total=2 * c)
            elif not enc_ng and (hv := self.halves(gs, lv.skip, g_skip)):
                g_pooled = self.pool_add_plan2(gs, hv, g_skip, gz)
                if g_pooled is not None:
                    self.deferred2 = (lv, gs, hv, g_pooled)           # level2() issues it, behind its own launch
                else:
                    self.bwd_halves(lv.conv, gs, hv, lv.skip_act, 2 * c)
            else:
                self.wgrad(lv.conv, lv.skip, gs, cin_total=2 * c)
                if not enc_ng:
                    self.dgrad(lv.conv, gs, g_skip, 0, c, skips, lv.skip_act)
            self.up_bwd(lv, gs, gz)
            return g_skip, gz
        ups, g_up = {s: A[s][lv.up] for s in S}, self.new(c, h, w)
        # (fp32: the launcher declines 16-channel input blocks, so level 2 keeps the separate launches)
        if not enc_ng and (self.fuse_bf16 or (self.f32_ok(gs, skips, g_skip) and self.f32_ok(gs, ups, g_up))):
            self.bwd_cat(lv, gs, g_skip, g_up)
        else:
            self.wgrad(lv.conv, lv.skip, gs, b_key=lv.up, off_key=lv.off)
            if enc_ng:
                self.dgrad(lv.conv, gs, g_up, c, c)
            elif c == 16:
                # both column blocks in one launch: the four problems read the same gradient
                ops.conv3x3_dgrad_group(
                    [{"g": gs[s], "w": self.ly(s, lv.conv).w, "out": g_skip[s], "act": skips[s], "act_bn": self.ly(s, lv.skip_act).bn_nobias}
                     for s in S] + [{"g": gs[s], "w": self.ly(s, lv.conv).w, "out": g_up[s], "c0_add": c} for s in S], 0, c)
            else:
                self.dgrad(lv.conv, gs, g_skip, 0, c, skips, lv.skip_act)
                self.dgrad(lv.conv, gs, g_up, c, c)
        views = {}
        for s in S:
            oy, ox = A[s][lv.off]
            views[s] = g_up[s][:, :, oy:oy + 2 * hz, ox:ox + 2 * wz]
        self.convt_bwd(lv.convt, lv.z, lv.z_act, views, gz)
        return g_skip, gz

    def level2(self, g_out, g_in):
        """the 32 x 32 level: both weight gradients, the data gradient chain d2b -> d2a and the pooling scatter in one launch (both
        arithmetic modes: level2.hip / level2_cl.hip).  False: the geometry does not qualify, nothing was enqueued"""
        S, A, ly = self.S, self.A, self.ly
        deferred, self.deferred2 = self.deferred2, None
        if not self.level2_ok(g_out, g_in):
            if deferred is not None:
                raise RuntimeError("pool-add backward: the whole-level kernel declines the level it was planned for")
            return False
        g_pooled = None if deferred is None else deferred[3]
        self.wb.level2_bwd_group([{"g2": g_out[s], "c1": A[s]["c1"], "x": A[s]["pb2"], "w1": ly(s, "d2a").w, "w2": ly(s, "d2b").w,
                                   "bn1": ly(s, "d2a").bn_nobias, "act": A[s]["b2"], "act_bn": ly(s, "d1b").bn_nobias, "out": g_in[s],
                                   "dw1": self.dw(s, "d2a"), "db1": self.db(s, "d2a"), "dw2": self.dw(s, "d2b"), "db2": self.db(s, "d2b"),
                                   "pool_grad_out": None if g_pooled is None else g_pooled[s]}
                                  for s in S])
        if deferred is not None:
            # pool-add order (pool_add_plan2): the Up block's skip-halves launch scatters the level's raw data gradient while it writes g_in
            lv, gs, hv, _ = deferred
            self.bwd_halves(lv.conv, gs, hv, lv.skip_act, 2 * lv.c, pool_grads=g_pooled)
        return True

    def down(self, lv, g_out, g_in, h, w):
        """A Down block's DoubleConv at (h, w), 16 channels: the second conv, then the first conv with the max-pool scatter (+=) into
        g_in, the gradient of the full-resolution map.  fp32 (round 6, down1): both through the split-operand fused backward -- the
        second as the two halves of its input, the first with the scatter -- instead of four launches; the launcher declines a
        16-channel pooled map (down2)"""
        S, A = self.S, self.A
        if self.deferred is not None and lv is DOWN1:
            # pool-add order (pool_add_plan): the first layer's raw data gradient stays at the pooled resolution; the Up block's deferred
            # skip launch scatters it into g_in while it writes that map -- once
            up_lv, up_gs, g_skip, g_mid, g_pooled = self.deferred
            self.deferred = None
            assert all(g_skip[s] is g_in[s] for s in S)
            hv = self.halves(g_out, lv.mid, g_mid)
            if hv is None:
                raise RuntimeError("pool-add backward: the fused backward declines the Down block it was planned for")
            self.bwd_halves(lv.conv2, g_out, hv, lv.conv1, 16)
            self.bwd8(lv.conv1, g_mid, lv.pooled, None, g_pooled, cin_total=lv.cin)
            self.bwd8(up_lv.conv, up_gs, up_lv.skip, up_lv.skip_act, g_in, cin_total=2 * up_lv.c, pool_grads=g_pooled)
            return
        pooled = all(A[s].get(lv.pooled) is not None for s in S)              # the forward pass saved the pooled map
        fulls = {s: A[s][lv.full] for s in S}
        g_mid = self.new(16, h, w)
        # hv: both layers take the fp32 fused form, or neither (the pooled map is asked first: one call settles down2)
        hv = None
        if not self.fuse_bf16 and pooled and self.f32_ok(g_mid, {s: A[s][lv.pooled] for s in S}, g_in, fulls):
            hv = self.halves(g_out, lv.mid, g_mid)
        if self.fuse_bf16:
            self.bwd8(lv.conv2, g_out, lv.mid, lv.conv1, g_mid, cin_total=16)
        elif hv:
            self.bwd_halves(lv.conv2, g_out, hv, lv.conv1, 16)
        else:
            self.wgrad(lv.conv2, lv.mid, g_out)
            self.dgrad(lv.conv2, g_out, g_mid, 0, 16, {s: A[s][lv.mid] for s in S}, lv.conv1)
        if hv:
            self.bwd8(lv.conv1, g_mid, lv.pooled, lv.full_act, g_in, cin_total=lv.cin, pool_key=lv.full, accumulate=True)
        elif self.fuse_bf16 and pooled:
            self.bwd8(lv.conv1, g_mid, lv.pooled, lv.full_act, g_in, cin_total=lv.cin, pool_key=lv.full)
        else:
            if pooled:
                self.wgrad(lv.conv1, lv.pooled, g_mid)
            else:
                self.wgrad(lv.conv1, lv.full, g_mid, a_mode=L.PC_SRC_POOL2)
            self.dgrad(lv.conv1, g_mid, g_in, 0, lv.cin, fulls, lv.full_act, pool=True, acc=True)

    def first_layer(self, G_a1, input_grad=None):
        """inc1: weight gradients over whichever form of the input the forward pass saved; then, when asked for, the gradient of the
        model input itself"""
        self.first_layer_wgrad(G_a1)
        if input_grad is not None:
            # data gradient of inc1 + the adjoint of its loader (reflect padding, channel gather), all streams in one launch
            pt, pl, Hp, Wp = self.saved["geom"]
            H, W = input_grad.shape[2:]
            ops.input_grad([{"g": G_a1[s], "w": self.ly(s, "inc1").w, "chmap": chmap[:cin]} for s, chmap, cin, _ in self.eng.streams],
                           input_grad, (pt, Hp - H - pt, pl, Wp - W - pl))

    def first_layer_wgrad(self, G_a1):
        saved, wb = self.saved, self.wb
        if saved.get("Xp8") is not None:
            # both streams' first-layer weight gradients in ONE launch of the standard 8-channel kernel over the shared input; the
            # batched reduce writes each stream's channel window
            xp8, win = saved["Xp8"]
            wb.conv3x3_group([{"a": xp8, "g": G_a1[s], "dw": self.dw(s, "inc1"), "db": self.db(s, "inc1"), "src_window": win[s]}
                              for s in self.S], 8)
            return
        pad_top, pad_left, _, _ = saved["geom"]
        for s, chmap, cin, _ in self.eng.streams:
            cout = self.ly(s, "inc1").w.shape[0]
            if saved.get("Xp") is not None:
                wb.conv3x3(saved["Xp"][s], G_a1[s], cout, self.dw(s, "inc1"), self.db(s, "inc1"))
            else:           # (saved["X"] is None only when the forward pass was fed the padded input directly: Xp_all)
                wb.conv3x3(saved["X"], G_a1[s], cout, self.dw(s, "inc1"), self.db(s, "inc1"), a_mode=L.PC_SRC_REFLECT,
                           a_pad=(pad_top, pad_left), chmap=chmap, a_channels=cin)


def up_bwd_w_ok(w):
    """Widths the composed Up block's backward kernel takes (pc_conv3x3_up_bwd_ok: column tiles of 64 / 128, ragged in multiples of 8)."""
    return w >= 16 and w % 8 == 0


def compose_ok(h, w, hz, wz, fwd_only):
    """May the first conv of an Up block at (h, w) read the low-resolution map (hz, wz) through composed weights?  fp32, exact 2x
    geometry; the composed BACKWARD kernel takes widths that are multiples of 8 (round 5: column tiles), a forward-only pass takes any
    geometry the forward kernel accepts, e.g. the 2076 / 1038-wide levels of an inference window."""
    return COMPOSED_UP and FUSED_CONV_BWD and L.act_dtype() == torch.float32 and (h, w) == (2 * hz, 2 * wz) and h % 4 == 0 and \
        (up_bwd_w_ok(w) or fwd_only)


def stream_channel_order(streams):
    """Input channels (indices into the model input [R,G,B,NIR,VV,VH]) in the order the padded per-stream input holds them."""
    return [c for _, chmap, cin, _ in streams for c in chmap[:cin]]


def forward_multi(engines, X, pad_top, pad_left, Hp, Wp, saves, feats_list=None, logit_only=None, Xp_all=None):
    """Forward of several DualStreamUNets (e.g. the frozen building extractor and the trainable U-Net) on the same
    input and geometry, layer by layer, with ONE launch per layer for all (network, stream) pairs: 4x fewer
    launches than per-stream execution and 4x more workgroups per launch on the 32x32 layers.
    Returns ([features], [saved-or-None]).

    logit_only[e] = True (dual-stream engines that are not saved, i.e. the frozen building extractor): the network's
    feature map is only ever consumed by its 1x1 ``fusion_out_conv`` (popcorn.py:301), so the last conv of each stream
    writes that layer's partial sum over its own 8 channels instead of the features; ``features[e]`` is then the
    (B, 2, Hp, Wp) tensor of the two partial logits (add them and the bias: ``partial_logit_weights``), or the ordinary
    16-channel map when the geometry does not qualify.

    Xp_all (fp32 mode): the already padded, normalised, channel-gathered input (B, sum of stream channels in stream order, Hp, Wp)
    as ``ops.select_normalize_pad`` writes it from a raw tile -- X may then be None (nothing reads the unpadded input)."""
    bf = L.act_dtype() == torch.bfloat16
    if Xp_all is not None:
        L.require_device(Xp_all)
        if bf:
            # bf16 mode: ONE channels-last bf16 tensor (B, 8, Hp, Wp) as ops.ingest_cl8 writes it (stream channels in stream order,
            # the rest zero)
            if tuple(Xp_all.shape[1:]) != (8, Hp, Wp) or Xp_all.dtype != torch.bfloat16 or Xp_all.stride(1) != 1 or Xp_all.stride(3) != 8:
                raise ValueError("bf16 mode: Xp_all must be a channels-last bf16 (B, 8, Hp, Wp) tensor (ops.ingest_cl8)")
        elif tuple(Xp_all.shape[2:]) != (Hp, Wp) or Wp % 4 or Xp_all.dtype != torch.float32:
            raise ValueError("Xp_all needs a (B, C, Hp, Wp) fp32 tensor with Wp % 4 == 0 (fp32 mode)")
        B, dev = Xp_all.shape[0], Xp_all.device
    else:
        L.require_device(X)
        B = X.shape[0]
        if pad_top >= X.shape[2] or pad_left >= X.shape[3] or Hp - X.shape[2] - pad_top >= X.shape[2] \
                or Wp - X.shape[3] - pad_left >= X.shape[3]:
            raise ValueError("reflect padding must be smaller than the input (same restriction as F.pad reflect)")
        dev = X.device
    if Hp < 4 or Wp < 4:
        raise ValueError("input too small for two 2x2 poolings")
    H1, W1 = Hp // 2, Wp // 2
    H2, W2 = H1 // 2, W1 // 2
    nE = len(engines)
    if feats_list is None:
        feats_list = [None] * nE
    # single-stream engines leave the other 8 feature channels at zero
    mk = torch.empty if len(engines[0].streams) == 2 else torch.zeros
    if logit_only is None:
        logit_only = [False] * nE
    # (fp32: any geometry -- partial strips take the per-element form of the epilogue; the bf16 kernels' form needs whole strips)
    dot_ok = len(engines[0].streams) == 2 and (not bf or (Wp % 32 == 0 and Hp % 4 == 0))
    logit_only = [bool(lo) and dot_ok and not saves[e] and feats_list[e] is None and engines[e].fusion_w is not None
                  for e, lo in enumerate(logit_only)]
    feats = [f if f is not None else
             (torch.empty(B, 2, Hp, Wp, device=dev, dtype=torch.float32) if logit_only[e] else
              L.empty_act(B, 16, Hp, Wp, dev, zero=mk is torch.zeros)) for e, f in enumerate(feats_list)]
    E = lambda c, h, w: L.empty_act(B, c, h, w, dev)  # noqa: E731
    streams = engines[0].streams
    assert all([st[0] for st in e.streams] == [st[0] for st in streams] for e in engines)
    if Xp_all is not None:
        # the padded input is sliced by engines[0]'s stream table: every engine must read the same channels in the same order
        order = stream_channel_order(streams)
        if any(stream_channel_order(e.streams) != order for e in engines) or (not bf and Xp_all.shape[1] != sum(st[2] for st in streams)):
            raise ValueError(f"Xp_all holds {Xp_all.shape[1]} channels; the engines expect {order} (identical for all engines)")
    keys = [(e, s) for e in range(nE) for s, _, _, _ in streams]
    ly = lambda k, t: engines[k[0]].layers[(k[1], t)]  # noqa: E731
    fwd_only = not any(saves)          # (forward-only passes -- inference windows -- take any width the composed forward kernel accepts)

    def first_layer(Xp_all):
        """inc1.  Cin differs per stream -> one launch per stream kind, over one of three forms of the input.  With real padding the
        padded, channel-gathered input is written ONCE and every consumer -- the first conv of each (network, stream) pair and, in
        training, its weight gradient -- reads that: fp32 with 16-byte rows as planar channel blocks through the aligned DIRECT
        loader (pc_reflect_pad_select), bf16 as ONE channels-last tensor with a 16-byte slot per pixel, of which every first conv
        reads a channel window (one launch for all pairs).  Otherwise the reflect padding + channel gather stay fused in the loaders
        (bf16 mode rounds the planar fp32 input there; unpadded inference windows need no copy).
        Returns (a1, Xp, Xp8): the outputs and the saved form -- Xp {stream: padded gathered input} (fp32), Xp8 (shared input,
        {stream: (first channel, channels)}) (bf16), or neither."""
        a1 = {k: E(8, Hp, Wp) for k in keys}
        if Xp_all is None and PADDED_INPUT and Wp <= 1024 and (Hp, Wp) != tuple(X.shape[2:]) and X.dtype == torch.float32:
            pads = (pad_top, Hp - X.shape[2] - pad_top, pad_left, Wp - X.shape[3] - pad_left)
            if not bf and Wp % 4 == 0:
                Xp_all = ops.reflect_pad_select(X, stream_channel_order(streams), *pads)
            elif bf and len(streams) == 2 and len(keys) <= L.PC_MAX_GROUP and X.is_contiguous():
                Xp_all = ops.ingest_cl8(X, stream_channel_order(streams), None, None, *pads)
        win, off = {}, 0
        for s, _, cin, _ in streams:
            win[s] = (off, cin)
            off += cin
        if Xp_all is not None and bf:
            if len(keys) > L.PC_MAX_GROUP:
                raise ValueError("bf16 shared-input first layer: at most PC_MAX_GROUP (network, stream) pairs")
            ops.conv3x3_fwd_group([{"a": Xp_all, "w": ly(k, "inc1").w, "bn": ly(k, "inc1").bn, "out": a1[k], "w_window": win[k[1]]}
                                   for k in keys])
            return a1, None, (Xp_all, win)
        Xp = None if Xp_all is None else {s: Xp_all[:, c0:c0 + cin] for s, (c0, cin) in win.items()}
        for s, chmap, cin, _ in streams:
            probs = [{"a": X if Xp is None else Xp[s], "w": ly(k, "inc1").w, "bn": ly(k, "inc1").bn, "out": a1[k]} for k in keys if k[1] == s]
            if Xp is not None:
                ops.conv3x3_fwd_group(probs)
            else:
                for pr in probs:
                    pr["chmap"] = chmap
                ops.conv3x3_fwd_group(probs, a_mode=L.PC_SRC_REFLECT, a_pad=(pad_top, pad_left), out_hw=(Hp, Wp), a_channels=cin)
        return a1, Xp, None

    def conv(tag, ins, c, h, w, outs=None, bs=None, pooled=None, **kw):
        """pooled: dict to receive the MaxPool2d(2) copy of every output (written by the same epilogue) -- left empty when
        the geometry does not qualify, in which case the Down block pools on the fly (PC_SRC_POOL2 loader)."""
        outs = outs or {k: E(c, h, w) for k in keys}
        probs = []
        for k in keys:
            pr = {"a": ins[k], "w": ly(k, tag).w, "bn": ly(k, tag).bn, "out": outs[k]}
            if bs is not None:
                pr["b"] = bs[k]
            if pooled is not None:
                po = ops.pool_out_like(outs[k])
                if po is not None:
                    pooled[k] = pr["pool_out"] = po
            probs.append(pr)
        ops.conv3x3_fwd_group(probs, **kw)
        if pooled is not None and len(pooled) != len(keys):
            pooled.clear()
        return outs

    def down(tag, full, pooled, c, h, w):
        if pooled:
            return conv(tag, pooled, c, h, w)
        return conv(tag, full, c, h, w, a_mode=L.PC_SRC_POOL2)

    def convt(tag, ins, c, h, w):
        outs = {k: E(c, h, w) for k in keys}
        ops.convt2x2_group([{"x": ins[k], "w": ly(k, tag).w, "bias": ly(k, tag).b, "out": outs[k]} for k in keys])
        return outs

    def up_conv(tag, ttag, skip, z, c, h, w):
        """first conv of an Up block straight from the low-resolution map z (composed weights): (outs, workspaces), or None"""
        if not compose_ok(h, w, z[keys[0]].shape[2], z[keys[0]].shape[3], fwd_only):
            return None
        outs = {k: E(c, h, w) for k in keys}
        if not all(ops.conv3x3_up_fwd_ok(skip[k], z[k], outs[k]) for k in keys):
            return None
        ws = ops.conv3x3_up_fwd_group([{"skip": skip[k], "z": z[k], "w": ly(k, tag).w, "wt": ly(k, ttag).w, "bt": ly(k, ttag).b,
                                        "bn": ly(k, tag).bn, "out": outs[k], "ws": precomp.get((tag, k))} for k in keys])
        return outs, dict(zip(keys, ws))

    def compose_weights():
        """the composed operand images of both Up levels of all (network, stream) pairs: one launch (they only depend on the weights)"""
        lst = [("up2a", "up2t", k) for k in keys] + [("up1a", "up1t", k) for k in keys]
        wss = ops.conv3x3_up_compose([{"w": ly(k, t).w, "wt": ly(k, tt).w, "bt": ly(k, tt).b} for t, tt, k in lst])
        return {(t, k): w_ for (t, tt, k), w_ in zip(lst, wss)}

    def level2(pb2, compose2):
        """fp32 / bf16 (level2.hip / level2_cl.hip): whole-tile residency at 32 x 32 -- one workgroup per (tile, network-stream) runs
        down2's two convs and up2's transposed conv with the 16 x 32 x 32 maps in LDS; c1 / c2 / u2 go to HBM only for whoever reads
        them.  Returns (c1, c2, u2), or None when the geometry does not qualify"""
        if not (FUSED_LEVEL2 and pb2 and (H2, W2) == (32, 32)):
            return None
        u2 = {k: (None if compose2 else E(16, 2 * H2, 2 * W2)) for k in keys}
        if not all(ops.level2_fwd_ok(pb2[k], u2[k]) for k in keys):
            return None
        c1 = {k: (E(16, H2, W2) if saves[k[0]] else None) for k in keys}
        c2 = {k: (E(16, H2, W2) if (saves[k[0]] or compose2) else None) for k in keys}
        ops.level2_fwd_group([{"x": pb2[k], "w1": ly(k, "d2a").w, "bn1": ly(k, "d2a").bn, "w2": ly(k, "d2b").w,
                               "bn2": ly(k, "d2b").bn, "wt": ly(k, "up2t").w, "bt": ly(k, "up2t").b, "c1": c1[k], "c2": c2[k],
                               "u2": u2[k]} for k in keys])
        return c1, c2, u2

    # with the composed first conv nobody reads the up-sampled tensors u2 / u1 -- not even the backward pass (up_bwd.hip)
    compose2 = compose_ok(H1, W1, H2, W2, fwd_only)
    compose1 = compose_ok(Hp, Wp, H1, W1, fwd_only)
    precomp, pa2, pb2 = {}, {}, {}
    a1, Xp, Xp8 = first_layer(Xp_all)
    a2 = conv("inc2", a1, 8, Hp, Wp, pooled=pa2)
    b1 = down("d1a", a2, pa2, 16, H1, W1)
    b2 = conv("d1b", b1, 16, H1, W1, pooled=pb2)
    if compose1 and compose2 and 2 * len(keys) <= 2 * L.PC_MAX_GROUP:
        precomp = compose_weights()
    r = level2(pb2, compose2)
    if r is None:
        c1 = down("d2a", b2, pb2, 16, H2, W2)
        c2 = conv("d2b", c1, 16, H2, W2)
        u2 = {k: None for k in keys}
    else:
        c1, c2, u2 = r
    o2 = ((H1 - 2 * H2) // 2, (W1 - 2 * W2) // 2)
    r = up_conv("up2a", "up2t", b2, c2, 8, H1, W1) if compose2 else None
    ws_up2 = {}
    if r is None:
        if any(u2[k] is None for k in keys):
            u2 = convt("up2t", c2, 16, 2 * H2, 2 * W2)
        e1 = conv("up2a", b2, 8, H1, W1, bs=u2, b_offset=o2)
    else:
        e1, ws_up2 = r
    u1_fused = None
    if bf and FUSED_UPT and (Hp, Wp) == (2 * H1, 2 * W1):
        # bf16 mode: up1's transposed conv in the epilogue of the conv that produces its input (one launch instead of two; e2 is still
        # written for the backward pass)
        e2 = {k: E(8, H1, W1) for k in keys}
        u1_fused = {k: E(8, 2 * H1, 2 * W1) for k in keys}
        ops.conv3x3_fwd_group([{"a": e1[k], "w": ly(k, "up2b").w, "bn": ly(k, "up2b").bn, "out": e2[k], "upt_w": ly(k, "up1t").w,
                                "upt_b": ly(k, "up1t").b, "upt_out": u1_fused[k]} for k in keys])
    else:
        e2 = conv("up2b", e1, 8, H1, W1)
    o1 = ((Hp - 2 * H1) // 2, (Wp - 2 * W1) // 2)
    r = up_conv("up1a", "up1t", a2, e2, 8, Hp, Wp) if compose1 else None
    ws_up1 = {}
    if r is None:
        u1 = u1_fused if u1_fused is not None else convt("up1t", e2, 8, 2 * H1, 2 * W1)
        f1 = conv("up1a", a2, 8, Hp, Wp, bs=u1, b_offset=o1)
    else:
        f1, ws_up1 = r
        u1 = {k: None for k in keys}
    f0s = {s: f0 for s, _, _, f0 in streams}
    probs = []
    for k in keys:
        pr = {"a": f1[k], "w": ly(k, "up1b").w, "bn": ly(k, "up1b").bn}
        f0 = f0s[k[1]]
        if logit_only[k[0]]:
            si = f0 // 8                                   # stream index = channel of the partial-logit tensor
            pr["dot_w"] = engines[k[0]].fusion_w.reshape(-1)[f0:f0 + 8].contiguous()
            pr["dot_out"] = feats[k[0]][:, si:si + 1]
        else:
            pr["out"] = feats[k[0]][:, f0:f0 + 8]
        probs.append(pr)
    ops.conv3x3_fwd_group(probs)
    saved = []
    for e in range(nE):
        if not saves[e]:
            saved.append(None)
            continue
        sv = {}
        for s, _, _, _ in streams:
            k = (e, s)
            sv[s] = dict(a1=a1[k], a2=a2[k], b1=b1[k], b2=b2[k], c1=c1[k], c2=c2[k], u2=u2[k], e1=e1[k], e2=e2[k],
                         u1=u1[k], f1=f1[k], o1=o1, o2=o2, pa2=pa2.get(k), pb2=pb2.get(k), ws_up1=ws_up1.get(k), ws_up2=ws_up2.get(k))
        sv["X"] = X
        sv["Xp"] = Xp                       # per stream: the padded, gathered input (fp32 path) or None
        sv["Xp8"] = Xp8                     # bf16 path: (shared channels-last input, channel window per stream) or None
        sv["geom"] = (pad_top, pad_left, Hp, Wp)
        sv["feats"] = feats[e]
        saved.append(sv)
    return feats, saved
