"""Adjudication of a gradient mismatch between the HIP path and an fp32 reference (DESIGN.md section 0 "Ties"; DESIGN_HISTORY.md "Gradient parity and ties").

The backward pass contains discrete decisions -- the ReLU mask of every layer and the arg-max of every 2 x 2 pooling window -- and an
activation within fp32 rounding of a tie flips one of them in one of two fp32 evaluations; the affected gradients then move by
~1e-3 relative in ALL layers below.  EVERY decision of the HIP side is OBSERVED, none is searched for:

  * the ReLU masks and pooling arg-maxes of the trainable U-Net come from the HIP forward's saved activations (``hip_decision_sites``);
  * the ReLU masks of the head's three hidden layers and of the final ``relu(out[:, 0])`` on the selected pixels come from the head
    backward kernel itself: its hidden activations live in registers, so one ``ops.head_bwd`` call on the saved features runs the
    decision-exporting instantiation of the kernel (``pc_debug_head_decisions``, popcorn_hip.h) in the multiplication form in force
    (``hip_head_decisions``).  The exported masks are the values the kernel's own backward chain multiplies with.

A mismatch above the 2e-4 bar is accepted ONLY when it is proven to be a tie flip (``assert_tie_flip``):

  1. at least one of those decisions differs between the HIP side and the fp32 CPU oracle (``O.TieProbe``), compared site by site;
  2. ONE of the two fp32 gradient sets is the neighbour of the exact (fp64 oracle) gradients (<= 2e-4) and the other is no further
     than one flipped decision explains (< 5e-3);
  3. (checked by the callers) the forward results / losses agree to rounding.

A mismatch with no differing site anywhere is a failure: there is no fallback.

Used by tests/test_gpu_fuzz.py (random geometries) and by the golden-fixture gradient tests of tests/test_gpu_model.py.

``forced_decision_distance`` is the stronger statement and needs no tolerance for ties at all: the oracle is evaluated with the
HIP side's decisions (``O.ForceDecisions``: U-Net sites and full head masks) and the two gradient sets must then agree to rounding.  The
oracle cannot adopt a WRONG mask that way: the overridden sites are bounded in number and each must be a near-tie in the oracle's own
values, for the head exactly as for the U-Net."""
import torch

from oracle import popcorn_oracle as O

ADJUDICATED = []       # one record per mismatch that passed through assert_tie_flip (printed in the session summary, conftest.py)
SHARED = []            # one record per forced_decision_distance comparison (residual under shared decisions, sites that differed)


def rel(a, r):
    return ((a.double() - r.double()).abs().max() / max(r.abs().max().item(), 1e-3)).item()


def hip_decision_sites(sd, x_dev, encoder_no_grad=False, padded=False):
    """Saved activations of the trainable U-Net's HIP forward (a fresh model with the given parameters), in the order the probe
    records the oracle's: per stream the conv+BN+ReLU layers that carry gradient (encoder_no_grad: the decoder only) and the
    inputs of the two poolings (none under encoder_no_grad).  Third result: the head's input, the (B, 16, H, W) crop of the feature map
    (padded: the device feature map itself with its crop origin, (feats (B, 16, Hp, Wp), pt, pl), for ``hip_head_decisions``)."""
    from popcorn_amd.model import POPCORN
    from popcorn_amd.model.popcorn import pad_geometry
    model2 = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    model2.load_state_dict(sd)
    H, W = x_dev.shape[2:]
    pt, pb, pl, pr = pad_geometry(H, W, False)
    _, saved = model2.engines()[0].forward(x_dev, pt, pl, H + pt + pb, W + pl + pr, save=True)
    acts, pools = [], []
    for s in ("sar_stream", "optical_stream"):
        sv = saved[s]
        acts += [sv[k].cpu() for k in (("e1", "e2", "f1") if encoder_no_grad else ("a1", "a2", "b1", "b2", "c1", "c2", "e1", "e2", "f1"))]
        f0 = 0 if s == "sar_stream" else 8
        acts.append(saved["feats"][:, f0:f0 + 8].cpu())
        if not encoder_no_grad:
            pools += [sv["a2"].cpu(), sv["b2"].cpu()]
    if padded:
        return acts, pools, (saved["feats"], pt, pl)
    feats = saved["feats"][:, :, pt:pt + H, pl:pl + W].cpu()
    return acts, pools, feats


def hip_head_decisions(sd, feats_dev, pt, pl, H, W, mask):
    """The head's ReLU decisions as the head backward KERNEL takes them on the selected pixels: one ``ops.head_bwd`` on the HIP forward's
    padded feature map with the decision-exporting instantiation (in the head form in force: split operands or fp32 MFMA) -> (hidden
    (3, 64, Nsel) bool, out (Nsel,) bool), columns in the oracle's order.  ``mask``: the oracle's selection (B, H, W), bit-equal to the
    HIP side's (tests/test_gpu_convt_head.py, test_gpu_model.py); the decisions do not depend on the upstream gradient (a constant 1)."""
    from popcorn_amd import ops
    dev = feats_dev.device
    B = feats_dev.shape[0]
    ht = [sd[f"head.{i}.{n}"].float().to(dev) for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    buf = ops.head_decision_buffer(B, H, W, dev)
    ops.head_bwd(feats_dev.float().contiguous(), pt, pl, H, W, ht, torch.ones(B, 1, H, W, device=dev),
                 mask=mask.to(torch.uint8).to(dev), g_scale_const=torch.ones(1, device=dev), decisions=buf)
    torch.cuda.synchronize()
    return ops.decode_head_decisions(buf, mask)


def oracle_head_decisions(sd, cpu_sample, seed, **flags):
    """The fp32 oracle's own head decisions on its selected pixels, its selection mask, and its features: (hidden (3, 64, Nsel) bool,
    out (Nsel,) bool), mask (B, H, W).  ``seed``: the torch seed in front of the forward (selection grid)."""
    import torch.nn.functional as F
    torch.manual_seed(seed)
    with torch.no_grad():
        fo = O.popcorn_forward(sd, {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in cpu_sample.items()},
                               padding=False, sparse=True, return_features=True,
                               **{k: v for k, v in flags.items() if k in ("encoder_no_grad", "unet_no_grad")})
        mask = fo["mask"]
        B, H, W = mask.shape
        from popcorn_amd.model.popcorn import pad_geometry
        pt, _, pl, _ = pad_geometry(H, W, False)
        feats = fo["features"][:, :, pt:pt + H, pl:pl + W]
        x = feats.permute(1, 0, 2, 3).reshape(feats.shape[1], -1, 1)[:, mask.reshape(-1)]
        hidden = []
        for i in (0, 2, 4):
            x = F.conv2d(x, sd[f"head.{i}.weight"], sd[f"head.{i}.bias"])
            hidden.append(x[:, :, 0] > 0)
            x = F.relu(x)
        out = F.conv2d(x, sd["head.6.weight"], sd["head.6.bias"])[0, :, 0] > 0
    return (torch.stack(hidden), out), mask


def assert_tie_flip(sd, cpu_sample, x_dev, hip_grads, ref_grads, seed, worst, **flags):
    """Raises unless the mismatch ``worst`` between ``hip_grads`` and ``ref_grads`` (both {name: cpu tensor}) is a proven
    decision flip (see the module docstring).  ``sd``: CPU state dict; ``cpu_sample``: the oracle's inputs; ``seed``: the torch
    seed in front of the forward (selection grid)."""
    torch.manual_seed(seed)
    with O.TieProbe() as probe32:
        O.train_step_grads(sd, dict(cpu_sample), **flags)
    acts, pools, (feats_dev, pt, pl) = hip_decision_sites(sd, x_dev, bool(flags.get("encoder_no_grad")), padded=True)
    if flags.get("unet_no_grad"):
        flips = 0                                 # nothing in the U-Net carries gradient: only the head has decisions
    else:
        assert len(acts) == len(probe32.acts) and len(pools) == len(probe32.pools), (len(acts), len(probe32.acts), len(pools), len(probe32.pools))
        flips = probe32.decisions_differ(acts, pools)
    # the head's decisions on the selected pixels: the kernel's own (exported) against the fp32 oracle's own
    H, W = x_dev.shape[2:]
    (re_hidden, re_out), mask = oracle_head_decisions(sd, cpu_sample, seed, **flags)
    ref_hidden, ref_out = probe32.head_masks()            # (what the oracle's backward pass above actually used)
    assert torch.equal(ref_hidden, re_hidden) and torch.equal(ref_out, re_out)
    hip_hidden, hip_out = hip_head_decisions(sd, feats_dev, pt, pl, H, W, mask)
    flips += int((ref_hidden != hip_hidden).sum()) + int((ref_out != hip_out).sum())
    proof = "site by site"
    assert flips > 0, ("no differing decision between the HIP side and the oracle explains the mismatch", worst)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    cpu64 = {k: (v.double() if v.is_floating_point() else v) for k, v in cpu_sample.items()}
    torch.manual_seed(seed)
    l64, _, g64, _ = O.train_step_grads(sd64, cpu64, **flags)
    w_hip = max(rel(hip_grads[n], g64[n]) for n in g64)
    w_ref = max(rel(ref_grads[n], g64[n]) for n in g64)
    import os
    rec = {"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "worst": worst, "flips": flips, "w_hip": w_hip, "w_ref": w_ref, "proof": proof}
    print(f"\n[tie adjudication] {rec['test']}: HIP-vs-fp32-reference {worst:.2e} above the 2e-4 bar; differing decisions (flips) = {flips}; "
          f"vs the fp64 oracle: w_hip = {w_hip:.2e}, w_ref = {w_ref:.2e}")
    assert min(w_hip, w_ref) < 2e-4 and max(w_hip, w_ref) < 5e-3, (worst, flips, w_hip, w_ref)
    ADJUDICATED.append(rec)
    return l64, flips, w_hip, w_ref


def forced_decision_distance(sd, cpu_sample, x_dev, hip_grads, seed, fp64=True, head_flips=(), observe_head=True, bar=1e-4,
                             max_flip_rate=2e-5, margin_bar=1e-4, **flags):
    """Worst relative distance between the HIP gradients and the CPU oracle's when the oracle takes the HIP side's decisions
    (``O.ForceDecisions``): at EVERY ReLU mask and pooling arg-max of the trainable U-Net they come from the HIP forward's saved
    activations, at every hidden unit and output of the head on the selected pixels from the head backward kernel's exported masks
    (``hip_head_decisions``).  No tie is then left to flip between the two sides and the distance is rounding only -- whatever the
    unforced comparison showed.  ``fp64``: the oracle in double precision (the exact gradients of that decision set).  Returns (worst,
    name of the worst tensor, {"relu", "pool": number of sites where the oracle alone decides differently, "head": list of those sites
    (layer 0 / 2 / 4 / 6, unit, column)}, loss).  (``observe_head=False, head_flips=[...]``: the head left to the oracle's own decisions
    with the listed units inverted -- tools/diag_shared_decisions.py only; ``bar`` is the callers' bound, kept for them.)

    The forced oracle takes its decisions from the implementation under test, so it must not be able to adopt a WRONG mask: per kind
    (relu, pool, head) the number of overridden sites is bounded (``max_flip_rate`` of all decision sites, at least 8) and every overridden
    site must be within rounding of a tie in the oracle's own values (``margin_bar``: |pre-activation| or top-2 gap relative to the
    layer's mean magnitude) -- a kernel regression that corrupts masks or arg-maxes fails here instead of being adopted."""
    acts, pools, (feats_dev, pt, pl) = hip_decision_sites(sd, x_dev, bool(flags.get("encoder_no_grad")), padded=True)
    if flags.get("unet_no_grad"):
        acts, pools = [], []                      # nothing in the U-Net carries gradient: only the head has decisions
    head_masks = None
    if observe_head:
        _, mask = oracle_head_decisions(sd, cpu_sample, seed, **flags)
        H, W = x_dev.shape[2:]
        head_masks = hip_head_decisions(sd, feats_dev, pt, pl, H, W, mask)
    if fp64:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
        cpu_sample = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in cpu_sample.items()}
    torch.manual_seed(seed)
    with O.ForceDecisions(acts, pools, head_flips, head_masks=head_masks) as f:
        loss, out, g, _ = O.train_step_grads(sd, dict(cpu_sample), **flags)
    assert f.i == len(acts) and f.j == len(pools), (f.i, len(acts), f.j, len(pools))
    if observe_head:
        assert f.sites["head"] == head_masks[0].numel() + head_masks[1].numel(), (f.sites["head"], head_masks[0].shape)
    for kind in ("relu", "pool", "head") if observe_head else ("relu", "pool"):
        nf = len(f.flips[kind]) if isinstance(f.flips[kind], list) else f.flips[kind]
        assert nf <= max(8, max_flip_rate * f.sites[kind]), \
            (kind, "overridden decisions", nf, "of", f.sites[kind], ": more than rounding explains")
        assert f.margin[kind] <= margin_bar, (kind, "an overridden decision is not a near-tie in the oracle's own values", f.margin[kind])
    errs = {n: rel(hip_grads[n], g[n]) for n in g}
    worst = max(errs, key=errs.get)
    flips = dict(f.flips)
    flips["head"] = list(f.flips["head"]) if observe_head else list(head_flips)
    import os
    SHARED.append({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "residual": errs[worst], "tensor": worst, "flips": flips,
                   "sites": dict(f.sites)})
    return errs[worst], worst, flips, loss
