"""Multi-unit census supervision on the GPU (csrc/units.hip and everything above it): the three kernels against the torch restatement
of tests/units_oracle.py, the model / autograd / fused-step paths against the EXISTING one-unit path on the replicated batch -- the
definition of the feature -- and the trainer flag.

Shapes at which the kernels can go wrong: (1, 37, 53) the scalar tail, (3, 64, 64) the 4-pixel path, (2, 100, 100) the model's padded
size; ragged K (census_n = [1, 4, 2]); one sample with K = 300 (beyond the 256 LDS bins); adjacent ids (5, 6, 7), the first and the
last of a list, an id above 65,536; a listed unit absent from the crop, unlisted neighbours, -1 padding."""
import numpy as np
import pytest
import torch

from tests import units_oracle as U

pytestmark = pytest.mark.gpu

BIG = 70001                 # an id above 65,536 (exact in fp32)
ABSENT = 99                 # listed, but not in any crop


def _tiling(H, W, ids, g, cell=5):
    """(H, W) float ids: wavy cells cycling through ``ids``, a -1 frame of 3 rows / 2 columns at the bottom / right (the collate's padding)."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    k = ((yy + (xx // 7) % 3) // cell) * ((W + cell - 1) // cell) + (xx + (yy // 9) % 2) // cell
    a = torch.tensor(ids, dtype=torch.float32)[k % len(ids)]
    a[H - 3:, :] = -1.0
    a[:, W - 2:] = -1.0
    return a


def _case(B, H, W, seed=0):
    """(admin (B,H,W), census_idx (B,K) int64, census_n) of the module docstring, per shape."""
    g = torch.Generator().manual_seed(seed)
    if B == 1:
        rows, pool = [[6, BIG, 5, 7, ABSENT]], [[5, 6, 7, BIG, 40, 41]]
    elif B == 3:
        # ragged: slots past census_n hold ids that ARE in the crop (5) or garbage -- ignored whatever they hold
        rows = [[6, 5, 123456, -7], [7, 5, BIG, 6], [12, 3, 5, 5]]
        pool = [[5, 6, 7, 40], [5, 6, 7, BIG, 41, 8], [3, 12, 5, 42]]
    else:
        many = (1000 + torch.randperm(300, generator=g)).tolist()          # K = 300, unsorted; 1000 .. 1288 present, the rest absent
        rows = [[7, 6, BIG, 5] + [-1] * 296, many]
        pool = [[5, 6, 7, BIG, 40, 41], list(range(1000, 1289)) + [43, 44]]
    cn = {1: [5], 3: [1, 4, 2], 2: [4, 300]}[B]
    admin = torch.stack([_tiling(H, W, pool[b], g) for b in range(B)])
    return admin, torch.tensor(rows, dtype=torch.int64), cn


SHAPES = [(1, 37, 53), (3, 64, 64), (2, 100, 100)]


def _kernel_slots(admin, cidx, cn):
    """The restatement's slot map in the kernels' numbering (ascending ids within a sample) + N."""
    slot, N = U.unit_slots(admin, cidx, cn)
    order = U.sorted_order(cidx, cn)
    ks = torch.where(slot >= 0, order[slot.clamp(min=0)], slot)
    return ks, order, N


@pytest.mark.parametrize("occ", [True, False])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_unit_mask_bit_exact(B, H, W, occ):
    from popcorn_amd import ops
    admin, cidx, cn = _case(B, H, W)
    g = torch.Generator().manual_seed(B * 1000 + H)
    building = torch.rand(B, 1, H, W, generator=g)
    building[building < 0.6] = 0.0
    rs = (torch.rand(H, generator=g) < 0.3).to(torch.uint8)
    cs = (torch.rand(W, generator=g) < 0.3).to(torch.uint8)
    ks, order, N = _kernel_slots(admin, cidx, cn)
    lay = ops.unit_layout(cidx.cuda(), cn)
    assert lay["N"] == N == sum(cn)
    assert torch.equal(lay["to_caller"].cpu(), order)
    units = lay["units"].cpu()
    off = lay["unit_off"].cpu().tolist()
    assert off == np.concatenate([[0], np.cumsum(cn)]).tolist()
    for b, c in enumerate(cn):
        assert units[off[b]:off[b + 1]].tolist() == sorted(cidx[b, :c].tolist())
    slot, mask, counts, pixels = ops.unit_mask(building.cuda(), admin.cuda(), lay["units"], lay["unit_off"], rs.cuda(), cs.cuda(), occ,
                                               want_pixels=True)
    want_mask, nsel, nreg = U.unit_mask(building, ks, rs, cs, occ)
    assert slot.dtype == torch.int32 and torch.equal(slot.cpu().long(), ks)
    assert torch.equal(mask.cpu().bool(), want_mask)
    assert counts.cpu().tolist() == [nsel, nreg]
    assert torch.equal(pixels.cpu().long(), torch.bincount(ks[ks >= 0], minlength=N))
    assert 0 < nsel < nreg or not occ
    # the same without the pixel counts (one launch)
    slot2, mask2, counts2 = ops.unit_mask(building.cuda(), admin.cuda(), lay["units"], lay["unit_off"], rs.cuda(), cs.cuda(), occ)
    assert torch.equal(slot2, slot) and torch.equal(mask2, mask) and torch.equal(counts2, counts)
    # the batch-wide empty-selection fallback: nothing built, nothing drawn
    zb, zr, zc = torch.zeros_like(building).cuda(), torch.zeros_like(rs).cuda(), torch.zeros_like(cs).cuda()
    slot3, mask3, counts3 = ops.unit_mask(zb, admin.cuda(), lay["units"], lay["unit_off"], zr, zc, occ)
    assert torch.equal(slot3, slot) and torch.equal(mask3.bool().cpu(), ks >= 0) and counts3.cpu().tolist() == [nreg, nreg]
    # and the call after it starts from clean accumulators
    _, _, counts4 = ops.unit_mask(building.cuda(), admin.cuda(), lay["units"], lay["unit_off"], rs.cuda(), cs.cuda(), occ)
    assert counts4.cpu().tolist() == [nsel, nreg]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_unit_popcount_reproducible_and_bounded(B, H, W):
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    admin, cidx, cn = _case(B, H, W)
    ks, order, N = _kernel_slots(admin, cidx, cn)
    g = torch.Generator().manual_seed(7 + H)
    # population densities over six decades, a quarter exact zeros (unselected pixels), one sample with both signs
    pd = torch.rand(B, H, W, generator=g) * 10.0 ** torch.randint(-4, 3, (B, H, W), generator=g).float()
    pd[torch.rand(B, H, W, generator=g) < 0.25] = 0.0
    pd[0] *= torch.where(torch.rand(H, W, generator=g) < 0.3, -1.0, 1.0)
    lay = ops.unit_layout(cidx.cuda(), cn)
    slot = ks.to(torch.int32).cuda()
    got = ops.unit_popcount(pd.cuda(), slot, N, lay["unit_off"])
    ref = U.unit_sums(pd, ks, N)                                          # float64
    n_px = torch.bincount(ks[ks >= 0], minlength=N).double()
    q = L.PC_UNIT_QUANTUM
    assert q == 2.0 ** -30
    err = (got.cpu().double() - ref).abs()
    bar = 2.0 ** -23 * ref.abs() + n_px * q
    print(f"\n[unit_popcount] {B}x{H}x{W}: worst err / bar {float((err / bar.clamp(min=1e-300)).max()):.3f}")
    assert bool((err <= bar).all()), float((err / bar.clamp(min=1e-300)).max())
    assert bool((got.cpu()[n_px == 0] == 0).all())                         # a listed unit absent from the crop sums to exactly 0
    # identical bits: a second run; without the sample ranges (global atomics only: another launch shape of the adds)
    assert torch.equal(_bits(ops.unit_popcount(pd.cuda(), slot, N, lay["unit_off"])), _bits(got))
    assert torch.equal(_bits(ops.unit_popcount(pd.cuda(), slot, N, None)), _bits(got))
    # identical bits with the samples in reversed batch order
    rev = list(range(B - 1, -1, -1))
    ks_r, order_r, _ = _kernel_slots(admin[rev], cidx[rev], [cn[b] for b in rev])
    lay_r = ops.unit_layout(cidx[rev].cuda(), [cn[b] for b in rev])
    got_r = ops.unit_popcount(pd[rev].cuda(), ks_r.to(torch.int32).cuda(), N, lay_r["unit_off"])
    per_sample = lambda v, counts: list(torch.split(v.cpu(), counts))  # noqa: E731
    a = per_sample(got, cn)
    b = per_sample(got_r, [cn[i] for i in rev])[::-1]
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    # a NaN / Inf / out-of-range term is reported as NaN on ITS unit; nothing wraps, the other units keep their bits
    tgt = int(ks[ks >= 0][0])
    where = (ks == tgt).nonzero()[0]
    for bad in (float("nan"), float("inf"), -float("inf"), 1e10):
        pd2 = pd.clone()
        pd2[tuple(where)] = bad
        out = ops.unit_popcount(pd2.cuda(), slot, N, lay["unit_off"]).cpu()
        assert bool(torch.isnan(out[tgt])), bad
        keep = torch.arange(N) != tgt
        assert torch.equal(_bits(out[keep]), _bits(got.cpu()[keep]))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_unit_paint_and_autograd(B, H, W):
    from popcorn_amd import ops
    admin, cidx, cn = _case(B, H, W)
    ks, order, N = _kernel_slots(admin, cidx, cn)
    g = torch.Generator().manual_seed(3)
    gp = torch.randn(N, generator=g)
    slot = ks.to(torch.int32).cuda()
    out = ops.unit_paint(gp.cuda(), slot)
    want = U.unit_paint(gp, ks)
    assert torch.equal(_bits(out), _bits(want))
    # a stale output buffer is overwritten everywhere
    buf = torch.full((B, H, W), 7.0, device="cuda")
    assert torch.equal(_bits(ops.unit_paint(gp.cuda(), slot, out=buf)), _bits(want))
    lay = ops.unit_layout(cidx.cuda(), cn)
    pd = torch.rand(B, H, W, generator=g).cuda().requires_grad_(True)
    pc = ops.UnitPopcount.apply(pd, slot, N, lay["unit_off"])
    (pc * gp.cuda()).sum().backward()
    assert torch.equal(_bits(pd.grad), _bits(want))
    assert torch.equal(_bits(pc), _bits(ops.unit_popcount(pd.detach(), slot, N, lay["unit_off"])))


# ---- the model, autograd and the fused step against the one-unit path on the replicated batch ---------------------------------------
def _new_model(precision="fp32"):
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, feature_extractor="DDA", occupancymodel=True, pretrained=True, biasinit=0.9407,
                sentinelbuildings=True).cuda()
    return m.set_precision(precision)


@pytest.fixture(scope="module")
def model():
    return _new_model()


@pytest.fixture(scope="module")
def case():
    """B = 2, 96 x 80, units [[12, 3, 7], [9, 5]] (unsorted) next to unlisted neighbours and -1 padding; K padded to 3."""
    inputs, y = U.make_case(B=2, H=96, W=80, units=((12, 3, 7), (9, 5)), channels=6, seed=11)
    return inputs, y


def _cuda(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module")
def oracle_forward(model, case):
    """tests/units_oracle.py on the CPU with the model's state, sparse and dense, computed once."""
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    out = {}
    for sparse in (True, False):
        torch.manual_seed(21)
        with torch.no_grad():
            out[sparse] = U.units_forward(sd, dict(case[0]), padding=False, sparse=sparse)
    return out


@pytest.mark.parametrize("sparse", [True, False])
def test_model_forward_vs_replicated_batch(model, case, oracle_forward, sparse):
    inputs, _ = case
    rep, _, rows = U.replicate(inputs)
    model.eval()
    with torch.no_grad():
        torch.manual_seed(21)
        o = model(_cuda(inputs), train=False, padding=False, sparse=sparse)
        torch.manual_seed(21)
        r = model(_cuda(rep), train=False, padding=False, sparse=sparse)
    N = sum(inputs["census_n"])
    assert tuple(o["popcount"].shape) == (N,) and tuple(o["popdensemap"].shape) == (2, 96, 80)
    if sparse:
        assert o["scale"].numel() == r["scale"].numel()                         # Nsel, exact
        total = torch.zeros_like(o["popdensemap"])
        for n, b in enumerate(rows):
            total[b] += r["popdensemap"][n]
        assert rel(o["popdensemap"], total) <= 1e-4                             # disjoint supports: the replicas add up to the map
        assert rel(o["scale"].sum(), r["scale"].sum()) <= 1e-4
    else:
        # the dense path masks nothing: every replica of a sample carries the same full map, and the multi-unit map is that map (their
        # literal sum would count it K_b times)
        assert tuple(o["scale"].shape) == (2, 96, 80)
        for n, b in enumerate(rows):
            assert rel(o["popdensemap"][b], r["popdensemap"][n]) <= 1e-4
    assert rel(o["popcount"], r["popcount"]) <= 1e-4
    ref = oracle_forward[sparse]
    assert rel(o["popcount"], ref["popcount"]) <= 1e-4 and rel(o["popdensemap"], ref["popdensemap"]) <= 1e-4
    if sparse:
        assert o["scale"].numel() == ref["scale"].numel() and rel(o["scale"], ref["scale"]) <= 1e-4
    # a 1-D census_idx is the one-unit path, untouched: (B,) popcounts
    assert tuple(r["popcount"].shape) == (N,) and r["popcount"].dim() == 1


def test_model_forward_bf16_vs_replicated_batch(case):
    inputs, _ = case
    rep, _, rows = U.replicate(inputs)
    m = _new_model("bf16").eval()
    with torch.no_grad():
        torch.manual_seed(21)
        o = m(_cuda(inputs), train=False, padding=False, sparse=True)
        torch.manual_seed(21)
        r = m(_cuda(rep), train=False, padding=False, sparse=True)
    assert o["scale"].numel() == r["scale"].numel()
    assert rel(o["popcount"], r["popcount"]) <= 1e-4
    total = torch.zeros_like(o["popdensemap"])
    for n, b in enumerate(rows):
        total[b] += r["popdensemap"][n]
    assert rel(o["popdensemap"], total) <= 1e-4


def _autograd_step(m, sample, y_flat, seed):
    """forward(train, padding=False, sparse=True) -> get_loss -> (100 loss).backward() through the drop-in module: (loss, grads by name,
    input gradient)."""
    from popcorn_amd.utils.losses import get_loss
    m.train()
    m.zero_grad()
    s = _cuda(sample)
    s["input"] = s["input"].clone().requires_grad_(True)
    torch.manual_seed(seed)
    o = m(s, train=True, padding=False, sparse=True)
    loss, _ = get_loss(o, {"y": y_flat.cuda()}, scale=o["scale"], loss=["log_l1_loss"], lam=[1.0], scale_regularization=0.01, tag="weak")
    (loss * 100.0).backward()
    grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    return loss.detach().cpu(), grads, s["input"].grad.detach().cpu().clone(), o


def grad_err(got, ref):
    """The project's gradient bar: max-abs difference over max(max-abs, 1e-3)."""
    return float((got.double() - ref.double()).abs().max() / max(float(ref.abs().max()), 1e-3))


@pytest.fixture(scope="module")
def autograd_pair(model, case):
    inputs, y = case
    rep, y_flat, rows = U.replicate(inputs, y)
    one = _autograd_step(model, inputs, y_flat, 33)
    ref = _autograd_step(model, rep, y_flat, 33)
    model.zero_grad()
    return one, ref, rows


def test_autograd_vs_replicated_batch(autograd_pair):
    (l1, g1, gx1, o1), (l0, g0, gx0, o0), rows = autograd_pair
    assert abs(l1.item() - l0.item()) <= 1e-4 * max(1.0, abs(l0.item()))
    assert set(g1) == set(g0) and len(g1) == 56
    worst = max(grad_err(g1[n], g0[n]) for n in g0)
    total = torch.zeros_like(gx1)
    for n, b in enumerate(rows):
        total[b] += gx0[n]
    ex = grad_err(gx1, total)
    print(f"\n[multi-unit autograd] loss {l1.item():.6f} vs {l0.item():.6f}; worst parameter gradient {worst:.2e}; input gradient {ex:.2e}")
    assert worst <= 2e-4 and ex <= 2e-4
    assert float(gx1.abs().max()) > 0


def test_fused_step_multi_unit(case, autograd_pair):
    from popcorn_amd.train import FusedTrainStep
    from tests import train_tail_oracle as TO
    (l1, g1, _, o1), _, _ = autograd_pair
    inputs, y = case
    hyp = dict(lr=1e-4, wd=1e-5, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.01)
    tr = FusedTrainStep(_new_model(), lr=hyp["lr"], weight_decay=hyp["wd"], gradient_clip=hyp["max_norm"])
    p0 = tr.flat_p.detach().cpu().numpy().copy()
    s = _cuda(inputs)
    s["y"] = y.cuda()
    torch.manual_seed(33)
    loss = tr.step(s)
    assert tr.native_steps == 0                                    # the eager per-launch engine, not pc_train_step
    assert abs(loss[0].item() - l1.item()) <= 1e-4 * max(1.0, abs(l1.item()))
    worst = max(grad_err(tr.grads[n].cpu(), g1[n]) for n in g1)
    print(f"\n[multi-unit fused step] loss {loss[0].item():.6f} vs autograd {l1.item():.6f}; worst gradient vs autograd {worst:.2e}")
    assert worst <= 2e-4
    assert rel(tr.last["popcount"], o1["popcount"]) <= 1e-4 and tuple(tr.last["popcount"].shape) == (5,)
    # parameters after the step: Adam + clip on THOSE gradients in float64, the bars of tests/test_gpu_train_tail.py
    gflat = tr.flat_g.detach().cpu().numpy()
    zeros = np.zeros_like(p0)
    ref = TO.adam_clip_ref(p0, gflat, zeros, zeros, [0, 0, 0, 0], n_decay=tr.n_decay, segments=list(tr.segments), active={0, 1, 2},
                           with_coef=True, **hyp)
    bars = TO.adam_bars(p0, ref)
    err = np.abs(tr.flat_p.detach().cpu().numpy().astype(np.float64) - ref[0])
    assert (err <= bars[0]).all(), float(np.max(err / np.maximum(bars[0], 1e-300)))
    assert tr.step_count.cpu().tolist()[:3] == [1, 1, 1]
    # a following one-unit sample still goes through the native executor
    rep, y_flat, _ = U.replicate(inputs, y)
    s1 = _cuda(rep)
    s1["y"] = y_flat.cuda()
    tr.step(s1)
    assert tr.native_steps == 1
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.loss_out).all())
    # graph mode refuses a multi-unit sample
    trg = FusedTrainStep(_new_model(), use_graph=True)
    with pytest.raises(ValueError):
        trg.step(dict(s))


def _fused_pair(H, W, given, seed=33):
    """One multi-unit fused step (B = 2, the ``case`` fixture's units at H x W) and the one-unit fused step on the replicated batch: fresh
    trainers on the same model state, the same seed in front of both (the same selection grid).  given: a sentinelbuildings = False model
    and a fixed building layer in the sample, which ``U.replicate`` carries along.  Returns (multi-unit trainer, loss, one-unit trainer,
    loss)."""
    from popcorn_amd.train import FusedTrainStep
    inputs, y = U.make_case(B=2, H=H, W=W, units=((12, 3, 7), (9, 5)), channels=6, seed=11)
    if given:
        inputs["building_counts"] = torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(4))
    rep, y_flat, _ = U.replicate(inputs, y)
    out = []
    for smp, yy in ((inputs, y), (rep, y_flat)):
        m = _new_model()
        m.sentinelbuildings = not given
        tr = FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01)
        s = _cuda(smp)
        s["y"] = yy.cuda()
        torch.manual_seed(seed)
        loss = tr.step(s)
        out += [tr, loss[0].item()]
    return out


def _assert_fused_pair(tag, tr, loss, tr1, loss1):
    """The bars of ``test_fused_step_multi_unit``: loss 1e-4 relative, the 56 gradients 2e-4, popcount 1e-4."""
    worst = max(grad_err(tr.grads[n].cpu(), tr1.grads[n].cpu()) for n in tr.names)
    pc = rel(tr.last["popcount"], tr1.last["popcount"])
    print(f"\n[{tag}] loss {loss:.6f} vs one-unit {loss1:.6f}; worst gradient {worst:.2e}; popcount {pc:.2e}")
    assert len(tr.names) == 56 and tuple(tr.last["popcount"].shape) == (5,)
    assert abs(loss - loss1) <= 1e-4 * max(1.0, abs(loss1))
    assert worst <= 2e-4
    assert pc <= 1e-4
    assert "slot" in tr.last and tr._ctx is None                   # the step's context does not outlive the step


def test_fused_step_multi_unit_same_domain():
    """2 x 100 x 100: pads of 14 on every side = the extractor's pad, so both networks run on ONE padded domain and the multi-unit step
    takes score_from_features + unit_mask behind the shared forward (the one-unit step there: the fused score_and_mask).  Seed 33, the
    first tried."""
    tr, loss, tr1, loss1 = _fused_pair(100, 100, given=False)
    assert tr.native_steps == 0 and tr1.native_steps == 1          # the replicated one-unit step goes through the native executor
    assert getattr(tr1, "_ctx", None) is None
    _assert_fused_pair("multi-unit fused step, same domain", tr, loss, tr1, loss1)


@pytest.mark.parametrize("H,W", [(96, 80), (100, 100)])
def test_fused_step_multi_unit_given_buildings(H, W):
    """A given building layer (sentinelbuildings = False + ``building_counts`` in the sample) x multi-unit, on separate domains (96 x 80)
    and on the shared one (100 x 100): unit_mask on the given layer, then the trainable U-Net alone.  Both sides run the per-launch
    engine (the executor declines a given layer).  Seed 33, the first tried."""
    tr, loss, tr1, loss1 = _fused_pair(H, W, given=True)
    assert tr.native_steps == 0 and tr1.native_steps == 0
    assert tr1._ctx is None
    _assert_fused_pair(f"multi-unit fused step, given buildings {H}x{W}", tr, loss, tr1, loss1)


def test_run_train_units_per_crop(tmp_path):
    """run_train.py --units_per_crop 4 --max_steps 4 on the synthetic multi-unit dataset: finishes with finite losses."""
    from popcorn_amd.cli import run_train
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 --synthetic_regions 16 -wb 2 -lt 2 "
            f"--units_per_crop 4 --max_steps 4 --synthetic_hw_range 48 80 --save-model no --save_dir {tmp_path}").split()
    t = run_train(argv)
    assert t.info["iter"] == 4 and t.fused.native_steps == 0
    assert tuple(t.fused.last["popcount"].shape)[0] >= 2
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
    pr = torch.cat([p for p, _ in t._r2buf])
    yy = torch.cat([y_ for _, y_ in t._r2buf])
    assert pr.shape == yy.shape and pr.dim() == 1                  # the rolling R2 buffer holds the flat N
