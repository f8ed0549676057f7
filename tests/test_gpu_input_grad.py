"""Gradient w.r.t. the model input on the GPU (csrc/input_grad.hip, ops.input_grad, UNetEngine.backward(input_grad=...),
POPCORN.forward with ``inputs["input"].requires_grad``).

  1 / 2  the op against torch autograd in float64 on the CPU (fp32 mode, and PC_PREC_BF16 with the roundings shared): the operation is
         linear, so the bar is the project's fp32 bar, 1e-4 of the largest reference element, with no ReLU decision involved;
  3      the model's ``X.grad`` against the fp64 oracle evaluated on the HIP side of every ReLU / arg-max decision (tests/tie_adjudication.py
         helpers, unchanged), bar 1e-4 -- and the parameter gradients bit-equal to a run whose input does not require grad;
  4      a decision-free identity: the first conv is linear in both operands, so per stream sum(X.grad * X) = sum(dW * W) of its weight;
         bar 1e-5 of sum|dW * W| (about 300 x the oracle's own fp32 residual, 9 x below the smaller of the two seeded mistakes the issue
         measured: cropping instead of folding 1.6e-4, a mirror off by one row 8.7e-5);
  5      semantics: where the reference leaves ``X.grad`` at None, frozen parameters, a non-contiguous leaf, the 2- / 4-channel models;
  6      bf16 mode: finite, non-zero, its distance from the fp32-mode gradient printed (no bar: the mode is parity-unpinned).

Every test prints the figure it asserts on."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")

SAR6, OPT6 = (4, 5), (2, 1, 0, 3)
KINDS = {6: [(2, SAR6), (4, OPT6)], 2: [(2, (0, 1))], 4: [(4, OPT6)]}          # model kind -> [(Cin, chmap)] of its streams
CASES = {                                                                       # (H, W), (pt, pb, pl, pr)
    "no_fold_32x32": ((32, 32), (0, 0, 0, 0)),
    "forced_33x20_pad14": ((33, 20), (14, 14, 14, 14)),                         # all three preimages of a column at once
    "unforced_131x77": ((131, 77), (30, 31, 25, 26)),                           # asymmetric pads, ragged against the tile
    "edge_16x130": ((16, 130), (15, 3, 0, 7)),                                  # pad = extent - 1, one axis unpadded, > 1 column tile
}
B = 2


@functools.lru_cache(maxsize=None)
def operands(case, cx, bf16=False):
    """(G per stream (B, 8, Hp, Wp) fp32 CPU, w per stream, float64 reference (B, cx, H, W)) -- made once per case, never modified.
    bf16: G and w are bf16 values (what the kernel's operands are in that mode); the reference is their exact float64 result."""
    (H, W), (pt, pb, pl, pr) = CASES[case]
    g = torch.Generator().manual_seed(1000 + 7 * sorted(CASES).index(case) + cx)
    gs, ws = [], []
    x64 = torch.zeros(B, cx, H, W, dtype=torch.float64, requires_grad=True)
    for cin, chmap in KINDS[cx]:
        gg = torch.randn(B, 8, H + pt + pb, W + pl + pr, generator=g)
        w = torch.randn(8, cin, 3, 3, generator=g) * 0.3
        gq, wq = (gg.bfloat16().float(), w.bfloat16().float()) if bf16 else (gg, w)
        xp = F.pad(x64[:, list(chmap)], (pl, pr, pt, pb), mode="reflect") if (pt or pb or pl or pr) else x64[:, list(chmap)]
        F.conv2d(xp, wq.double(), padding=1).backward(gq.double())
        gs.append(gq)
        ws.append(w)
    return gs, ws, x64.grad.detach().clone()


def run_op(case, cx, gs_dev, ws, out=None):
    from popcorn_amd import ops
    (H, W), pads = CASES[case]
    if out is None:
        out = torch.empty(B, cx, H, W, device="cuda")
    probs = [{"g": g_, "w": w.cuda(), "chmap": chmap} for g_, w, (_, chmap) in zip(gs_dev, ws, KINDS[cx])]
    ops.input_grad(probs, out, pads)
    torch.cuda.synchronize()
    return out


def worst(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


# ---- 1. the op against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [6, 2, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_op_vs_float64(case, cx):
    gs, ws, ref = operands(case, cx)
    got = run_op(case, cx, [g_.cuda() for g_ in gs], ws)
    e = worst(got, ref)
    print(f"\n[input_grad op fp32] {case} Cx={cx}: max|HIP - fp64| / max|fp64| = {e:.2e}")
    assert e <= 1e-4


def test_op_row_strided_gradient():
    """G as a [:, :, :, :Wp] slice of a wider tensor (what L.padded_rows() activations are)"""
    case, cx = "unforced_131x77", 6
    gs, ws, ref = operands(case, cx)
    views = []
    for g_ in gs:
        wide = torch.full((B, 8, g_.shape[2], g_.shape[3] + 3), float("nan"), device="cuda")
        wide[..., :g_.shape[3]] = g_.cuda()
        views.append(wide[..., :g_.shape[3]])
        assert not views[-1].is_contiguous()
    e = worst(run_op(case, cx, views, ws), ref)
    print(f"\n[input_grad op fp32] row-strided G: {e:.2e}")
    assert e <= 1e-4


@pytest.mark.parametrize("case", ["forced_33x20_pad14", "edge_16x130"])
def test_op_writes_every_element_and_is_reproducible(case):
    cx = 6
    gs, ws, ref = operands(case, cx)
    gd = [g_.cuda() for g_ in gs]
    (H, W), _ = CASES[case]
    a = run_op(case, cx, gd, ws, out=torch.full((B, cx, H, W), float("nan"), device="cuda"))
    assert bool(torch.isfinite(a).all())                   # every element written, with `=` (NaN + x stays NaN)
    assert worst(a, ref) <= 1e-4
    b = run_op(case, cx, gd, ws, out=torch.zeros(B, cx, H, W, device="cuda"))
    assert torch.equal(a, b)                               # fixed summation order: the same bits from run to run


# ---- 2. the same in PC_PREC_BF16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cx", [6, 2, 4])
@pytest.mark.parametrize("case", ["forced_33x20_pad14", "unforced_131x77"])
def test_op_bf16_vs_float64(case, cx):
    from popcorn_amd import _lib as L
    gs, ws, ref = operands(case, cx, True)
    with L.precision("bf16"):
        gd = []
        for g_ in gs:
            t = L.empty_act(B, 8, g_.shape[2], g_.shape[3], "cuda")
            assert t.dtype == torch.bfloat16 and t.stride(1) == 1
            t.copy_(g_.cuda())                             # exact: the values are bf16 numbers already
            gd.append(t)
        got = run_op(case, cx, gd, ws)                     # (the fp32 weights go in unrounded: the kernel rounds them)
    e = worst(got, ref)
    print(f"\n[input_grad op bf16] {case} Cx={cx}: max|HIP - fp64 of the bf16 operands| / max = {e:.2e}")
    assert got.dtype == torch.float32 and e <= 1e-4


# ---- model level --------------------------------------------------------------------------------------------------------------------------
def new_model(ic=6):
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    return POPCORN(input_channels=ic, feature_extractor="DDA", occupancymodel=True, pretrained=True, biasinit=0.9407,
                   sentinelbuildings=True).cuda()


@pytest.fixture(scope="module")
def model():
    return new_model()


@pytest.fixture(scope="module")
def g5():
    g = np.load(os.path.join(G, "g5_train.npz"))
    return {k: torch.from_numpy(g[k]) for k in ("input", "admin_mask", "census_idx", "y")}


def hip_step(model, sample, x_requires_grad, seed=5, x=None, **kw):
    """forward + get_loss + (loss * 100).backward() as tests/test_gpu_model.py: test_grad_truncation_modes_vs_oracle sets it up.
    Returns (X, {name: parameter gradient}, outputs)."""
    from popcorn_amd.utils.losses import get_loss
    s = {k: v.cuda() for k, v in sample.items()}
    if x is not None:
        s["input"] = x
    elif x_requires_grad:
        s["input"] = s["input"].clone().requires_grad_(True)
    kw.setdefault("padding", False)
    kw.setdefault("sparse", True)
    model.train()
    model.zero_grad()
    torch.manual_seed(seed)
    o = model(s, train=True, **kw)
    loss, _ = get_loss(o, s, scale=o["scale"], loss=["log_l1_loss"], lam=[1.0], scale_regularization=0.01, tag="weak")
    (loss * 100.0).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    return s["input"], grads, o


def forced_oracle_input_grad(sd, cpu_sample, acts, pools, head_masks, seed, **kw):
    """X.grad of the fp64 oracle evaluated with the given decisions (O.ForceDecisions), under the guards of
    tests/tie_adjudication.py: forced_decision_distance -- overridden sites <= max(8, 2e-5 * sites) per kind, each a near-tie (1e-4)."""
    from oracle import popcorn_oracle as O
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    s64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in cpu_sample.items()}
    s64["input"] = s64["input"].clone().requires_grad_(True)
    torch.manual_seed(seed)
    with O.ForceDecisions(acts, pools, (), head_masks=head_masks) as f:
        out = O.popcorn_forward(sd64, s64, **kw)
        loss, _ = O.get_loss(out, s64, scale=out["scale"], loss=("log_l1_loss",), lam=(1.0,), scale_regularization=0.01, tag="weak")
        (loss * 100.0).backward()
    assert f.i == len(acts) and f.j == len(pools), (f.i, len(acts), f.j, len(pools))
    assert f.sites["head"] == head_masks[0].numel() + head_masks[1].numel()
    for kind in ("relu", "pool", "head"):
        nf = len(f.flips[kind]) if isinstance(f.flips[kind], list) else f.flips[kind]
        assert nf <= max(8, 2e-5 * f.sites[kind]), (kind, "overridden decisions", nf, "of", f.sites[kind])
        assert f.margin[kind] <= 1e-4, (kind, "an overridden decision is not a near-tie in the oracle's own values", f.margin[kind])
    return s64["input"].grad, out


def stream_channels(ic):
    return {"sar_stream": {6: SAR6, 2: (0, 1)}.get(ic), "optical_stream": {6: OPT6, 4: OPT6}.get(ic)}


def identity_residuals(model, X, grads, ic=6):
    """per stream: |sum(X.grad * X) - sum(dW * W)| / sum|dW * W| over the first conv's weight, both sides in float64 on the host"""
    res = {}
    xg, x = X.grad.detach().double().cpu(), X.detach().double().cpu()
    for s, ch in stream_channels(ic).items():
        if ch is None:
            continue
        n = f"unetmodel.{s}.inc.conv.conv.0.weight"
        w, dw = dict(model.named_parameters())[n].detach().double().cpu(), grads[n].double().cpu()
        lhs = (xg[:, list(ch)] * x[:, list(ch)]).sum().item()
        res[s] = abs(lhs - (dw * w).sum().item()) / (dw * w).abs().sum().item()
    return res


# ---- 3. model against the oracle under shared decisions --------------------------------------------------------------------------------
def test_model_input_grad_vs_forced_oracle(model, g5):
    from tests.tie_adjudication import hip_decision_sites, hip_head_decisions, oracle_head_decisions, rel
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    X, grads, _ = hip_step(model, g5, True)
    assert X.grad is not None and X.grad.shape == X.shape and bool(torch.isfinite(X.grad).all())
    # a training step whose input does not require grad: the same 56 parameter gradients, bit for bit
    X0, grads0, _ = hip_step(model, g5, False)
    assert X0.grad is None and len(grads) == len(grads0) == 56
    for n in grads0:
        assert torch.equal(grads[n], grads0[n]), n
    H, W = X.shape[2:]
    acts, pools, (feats_dev, pt, pl) = hip_decision_sites(sd, X.detach(), padded=True)
    _, mask = oracle_head_decisions(sd, dict(g5), 5)
    head_masks = hip_head_decisions(sd, feats_dev, pt, pl, H, W, mask)
    ref, _ = forced_oracle_input_grad(sd, dict(g5), acts, pools, head_masks, 5, padding=False, sparse=True)
    e = rel(X.grad.cpu(), ref)
    print(f"\n[input_grad model] g5, shared decisions: rel(X.grad, fp64 oracle) = {e:.2e}")
    assert e < 1e-4


# ---- 4. the decision-free identity ---------------------------------------------------------------------------------------------------------
def test_identity_with_first_layer_weight_gradient(model, g5):
    X, grads, _ = hip_step(model, g5, True)
    res = identity_residuals(model, X, grads)
    print(f"\n[input_grad identity] g5 sparse: residual / sum|dW W| = { {k: f'{v:.2e}' for k, v in res.items()} }")
    assert all(v <= 1e-5 for v in res.values()), res


def test_identity_dense_padded_no_admin(model):
    """sparse=False, no admin_mask, padding=True on 1 x 6 x 33 x 36: the gradient reaches the border and every fold is exercised"""
    g = torch.Generator().manual_seed(41)
    sample = {"input": torch.randn(1, 6, 33, 36, generator=g), "y": torch.rand(1, generator=g) * 50 + 5}
    X, grads, _ = hip_step(model, sample, True, padding=True, sparse=False)
    assert bool((X.grad[:, :, 0].abs().sum() > 0) & (X.grad[:, :, :, -1].abs().sum() > 0))
    res = identity_residuals(model, X, grads)
    print(f"\n[input_grad identity] 1x6x33x36 dense padded: residual / sum|dW W| = { {k: f'{v:.2e}' for k, v in res.items()} }")
    assert all(v <= 1e-5 for v in res.values()), res


# ---- 5. semantics ------------------------------------------------------------------------------------------------------------------------------
def test_unet_no_grad_leaves_input_grad_none(model, g5):
    X, grads, _ = hip_step(model, g5, True, unet_no_grad=True, encoder_no_grad=True)
    assert X.grad is None
    assert sorted(grads) == sorted(f"head.{i}.{n}" for i in (0, 2, 4, 6) for n in ("weight", "bias"))


def test_encoder_no_grad_leaves_input_grad_none(model, g5):
    X, grads, _ = hip_step(model, g5, True, encoder_no_grad=True)
    assert X.grad is None
    assert any("up_seq" in n for n in grads) and not any(".inc." in n for n in grads)


def test_frozen_parameters_differentiable_input(g5):
    m = new_model()
    for p in m.parameters():
        p.requires_grad_(False)
    X, grads, o = hip_step(m, g5, True)
    assert o["popcount"].requires_grad and not grads
    assert X.grad is not None and X.grad.shape == X.shape
    assert bool(torch.isfinite(X.grad).all()) and float(X.grad.abs().max()) > 0


def test_snippet_of_the_issue(model, g5):
    s = {k: v.cuda() for k, v in g5.items()}
    x = s["input"].requires_grad_(True)
    model(s, padding=False)["popcount"].sum().backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    model.zero_grad()


def test_non_contiguous_leaf(model, g5):
    """a channel-sliced view of a 7-channel tensor as the leaf: the gradient arrives at the leaf's shape through .contiguous()"""
    base = torch.zeros(3, 7, 100, 100, device="cuda")
    base[:, :6] = g5["input"].cuda()
    leaf = base[:, :6].requires_grad_(True)
    assert leaf.is_leaf and not leaf.is_contiguous()
    Xv, _, _ = hip_step(model, g5, True, x=leaf)
    Xc, _, _ = hip_step(model, g5, True)
    assert Xv is leaf and leaf.grad is not None and leaf.grad.shape == leaf.shape
    assert torch.equal(leaf.grad, Xc.grad)


@pytest.mark.parametrize("ic", [2, 4])
def test_single_modality_vs_forced_oracle(ic):
    """input_channels = 2 / 4, dense (sparse=False) on 2 x Cx x 64 x 64, input seed 77, against the fp64 oracle under shared decisions.
    The oracle forces head masks only through its sparse head, so it runs sparse=True on a region that covers the whole tile, where
    its selection is every pixel (asserted) and the sparse head IS the dense one, pixel for pixel in the same order."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    from tests.tie_adjudication import rel
    m = new_model(ic)
    g = torch.Generator().manual_seed(77)
    sample = {"input": torch.randn(2, ic, 64, 64, generator=g), "admin_mask": torch.ones(2, 64, 64),
              "census_idx": torch.ones(2, dtype=torch.int64), "y": torch.rand(2, generator=g) * 200 + 20}
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    X, grads, _ = hip_step(m, sample, True, sparse=False)
    assert X.grad is not None and X.grad.shape == (2, ic, 64, 64) and len(grads) == 32
    # the HIP side's decisions: saved activations of its forward, and the head backward kernel's exported masks on every pixel
    feats, saved = m.engines()[0].forward(X.detach(), 0, 0, 64, 64, save=True)
    acts, pools = [], []
    for s in m._streams:
        sv = saved[s]
        acts += [sv[k].cpu() for k in ("a1", "a2", "b1", "b2", "c1", "c2", "e1", "e2", "f1")]
        acts.append(saved["feats"][:, m.feat_offset:m.feat_offset + 8].cpu())
        pools += [sv["a2"].cpu(), sv["b2"].cpu()]
    buf = ops.head_decision_buffer(2, 64, 64, X.device)
    ops.head_bwd(feats.float().contiguous(), 0, 0, 64, 64, [t.detach() for t in m.head_tensors()], torch.ones(2, 1, 64, 64, device=X.device),
                 g_scale_const=torch.ones(1, device=X.device), decisions=buf)
    torch.cuda.synchronize()
    head_masks = ops.decode_head_decisions(buf, None)
    ref, out = forced_oracle_input_grad(sd, dict(sample), acts, pools, head_masks, 5, padding=False, sparse=True)
    assert out["scale"].numel() == 2 * 64 * 64               # the oracle selected every pixel: its sparse head is the dense head
    e = rel(X.grad.cpu(), ref)
    res = identity_residuals(m, X, grads, ic)
    print(f"\n[input_grad model] input_channels={ic} dense 2x{ic}x64x64: rel(X.grad, fp64 oracle) = {e:.2e}; identity {res}")
    assert e < 1e-4
    assert all(v <= 1e-5 for v in res.values()), res


# ---- 6. bf16 model smoke ---------------------------------------------------------------------------------------------------------------------
def test_bf16_mode_input_grad(model, g5):
    X32, _, _ = hip_step(model, g5, True)
    m16 = new_model()
    m16.load_state_dict(model.state_dict())
    m16.set_precision("bf16")
    X16, _, _ = hip_step(m16, g5, True)
    assert X16.grad is not None and X16.grad.dtype == torch.float32 and bool(torch.isfinite(X16.grad).all())
    assert float(X16.grad.abs().max()) > 0
    d = ((X16.grad - X32.grad).double().norm() / X32.grad.double().norm()).item()
    print(f"\n[input_grad model] bf16 mode vs fp32 mode on g5: relative L2 distance of X.grad = {d:.3e} (no bar: parity-unpinned mode)")
