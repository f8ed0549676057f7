"""Single-modality models (S1-only: ``input_channels = 2``, S2-only: 4; popcorn.py:48-54,135-145,302-314) in the native step executor: a
ONE-STREAM plan of pc_train_step / _layer / _units / _units_layer (include/popcorn_hip.h), opt-in through ``FusedTrainStep(native_single=
True)``.

  * fixture g13 (tests/golden/make_golden_g13.py): g8 on the SHARED padded domain, 2 x ic x 36 x 36 -- the per-launch step, the model
    forward and the native step against the reference's loss, density map, building score and 32 gradients, at the bars of
    tests/test_gpu_model.py::test_single_modality_vs_reference_golden; the native step against g8 (48 x 40: two domains) as well.  The
    building score on the shared domain is the stream's own out conv (networks.py:217-228), not a half of fusion_out_conv: before this
    fixture the per-launch step took the latter there and nothing noticed;
  * equal bits, native against per-launch, two consecutive steps: loss, flat_p, flat_g, Adam state and every entry of ``last`` over
    geometries, regimes, data forms, the occupancy product, multi-unit batches and a shipped layer; the three phases issued separately;
  * footprint: an arena of exactly ``arena_needed`` bytes, equal bits whatever it held (the zero fill of the dead feature half and of the
    64 x 16 head images is what this catches);
  * opt-in: without the switch nothing moves, with it a dual-stream trainer issues its old launches;
  * the C entry's refusals: their codes, a 0x5A-filled arena untouched, a good call afterwards."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_native_step as t_native
from tests import footprint as FP
from tests import units_oracle as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGIMES = t_native.REGIMES
# (2, 36, 36): shared domain (pads 14 = the extractor's); (2, 48, 40): g8's; (2, 37, 53): odd sides, two different pads; (1, 70, 90)
GEOMS = [(2, 36, 36), (2, 48, 40), (2, 37, 53), (1, 70, 90)]
LAST = ("popcount", "popdensemap", "scale_map", "mask", "building_counts")


def rel_err(a, b):          # (tests/test_gpu_model.py)
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _same(a, b):
    return FP.bit_equal(a.detach().contiguous(), b.detach().contiguous())


def _model(ic, occ=True, given=False):
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    return POPCORN(input_channels=ic, feature_extractor="DDA", occupancymodel=occ, pretrained=True, biasinit=0.9407,
                   sentinelbuildings=not given).cuda()


def _trainer(ic, single, occ=True, given=False, **kw):
    from popcorn_amd.train import FusedTrainStep
    if single:
        kw["native_single"] = True
    return FusedTrainStep(_model(ic, occ, given), lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, **kw)


def _batch(ic, B, H, W, kind="input"):
    """The batch of tests/test_gpu_native_step.py.  "input": the model's own (B, ic, H, W); "input6": a 6-channel normalised tile, of which
    the stream picks its channels (what the trainer's host loader hands a one-stream model); "raw" / "split": as there."""
    smp = t_native._batch(B, H, W, "input" if kind == "input6" else kind)
    if kind == "input":
        smp["input"] = smp["input"][:, :ic].contiguous()
    return smp


def _two_steps(tr, smp, flags=(False, False)):
    out = []
    for it in range(2):
        torch.manual_seed(3 + it)
        loss = tr.step(dict(smp), encoder_no_grad=flags[0], unet_no_grad=flags[1])
        torch.cuda.synchronize()
        assert len(tr.grads) == 32
        o = {"loss": loss.clone(), "flat_g": tr.flat_g.clone(), "flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
             "step": tr.step_count.clone()}
        o.update({k: tr.last[k].clone() for k in LAST})
        if "slot" in tr.last:
            o["slot"] = tr.last["slot"].clone()
        out.append(o)
    return out


def _assert_same_steps(got, want, multi=False):
    assert len(got) == len(want) == 2
    for it, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        sel = b["mask"].bool()
        assert int(sel.sum()) > 0 and bool(torch.isfinite(b["loss"]).all()) and float(b["flat_g"].abs().max()) > 0
        for n in a:
            if n == "scale_map" or (n == "popdensemap" and not multi):
                # outside the selection the per-launch one-unit path leaves torch.empty memory (tests/test_gpu_native_step.py)
                assert _same(a[n][sel], b[n][sel]), (n, it)
            else:
                assert _same(a[n], b[n]), (n, it, (a[n].float() - b[n].float()).abs().nan_to_num(0).max().item())


def _check(ic, smp, flags=(False, False), multi=False, **kw):
    tr_n, tr_p = _trainer(ic, True, **kw), _trainer(ic, False, **kw)
    got, want = _two_steps(tr_n, smp, flags), _two_steps(tr_p, smp, flags)
    assert (tr_n.native_unit_steps, tr_n.native_steps) == ((2, 0) if multi else (0, 2))
    assert tr_p.native_steps == 0 and tr_p.native_unit_steps == 0
    _assert_same_steps(got, want, multi)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------------------
def _fixture_sample(g, ic):
    return {k: torch.from_numpy(g[f"ic{ic}/{k}"]).cuda() for k in ("input", "admin_mask", "census_idx", "y")}


def _assert_step_vs_fixture(tr, g, ic, native):
    """One fused step on the fixture's sample under the reference's draws (seed 5): loss, the 32 gradients, and the building score the
    step multiplied by -- the bars of test_single_modality_vs_reference_golden (1e-4 on the loss, 2e-4 of the tensor's largest magnitude
    on a gradient); the score at the density map's bar (rel_err 1e-4: a sigmoid of a 13-layer fp32 logit, ~1e-6 in practice)."""
    s = _fixture_sample(g, ic)
    torch.manual_seed(5)
    loss = tr.step(dict(s))
    torch.cuda.synchronize()
    assert tr.native_steps == (1 if native else 0)
    names = set(g[f"ic{ic}/grad_names"].tolist())
    assert set(tr.grads) == names and len(names) == 32
    err_b = rel_err(tr.last["building_counts"].cpu().numpy(), g[f"ic{ic}/building_counts"])
    err_l = abs(loss[0].item() - float(g[f"ic{ic}/loss"]))
    worst = max(np.abs(tr.grads[n].cpu().numpy() - g[f"ic{ic}/grad/{n}"]).max() / max(np.abs(g[f"ic{ic}/grad/{n}"]).max(), 1e-3) for n in names)
    print(f"\n[ic{ic} {'native' if native else 'per-launch'}] building_counts rel_err {err_b:.2e}, loss error {err_l:.2e}, "
          f"worst gradient error {worst:.2e} (bar 2e-4)")
    assert err_b < 1e-4
    assert err_l < 1e-4
    sel = tr.last["mask"].bool().cpu().numpy()
    assert int(sel.sum()) == g[f"ic{ic}/scale"].shape[0]
    assert rel_err(tr.last["popdensemap"].cpu().numpy()[sel], g[f"ic{ic}/popdensemap"][sel]) < 1e-4
    for n in names:
        r = g[f"ic{ic}/grad/{n}"]
        assert np.abs(tr.grads[n].cpu().numpy() - r).max() <= 2e-4 * max(np.abs(r).max(), 1e-3), n


@pytest.mark.parametrize("ic", [2, 4])
def test_per_launch_step_on_the_shared_domain_vs_reference_golden(ic):
    g = np.load(os.path.join(G, "g13_single_modality_shared.npz"))
    _assert_step_vs_fixture(_trainer(ic, False), g, ic, native=False)


@pytest.mark.parametrize("ic", [2, 4])
def test_model_on_the_shared_domain_vs_reference_golden(ic):
    """test_single_modality_vs_reference_golden on g13, plus the eval-mode dense ``model(sample, padding=False)``."""
    from popcorn_amd.utils.losses import get_loss
    g = np.load(os.path.join(G, "g13_single_modality_shared.npz"))
    m = _model(ic)
    for k in g.files:
        if k.startswith(f"ic{ic}/head."):
            assert np.array_equal(m.state_dict()[k[len(f"ic{ic}/"):]].cpu().numpy(), g[k])     # same seeded init
    m.train()
    s = _fixture_sample(g, ic)
    torch.manual_seed(5)
    smp = dict(s)
    o = m(smp, train=True, padding=False, sparse=True)
    loss, _ = get_loss(o, s, scale=o["scale"], loss=["log_l1_loss"], lam=[1.0], scale_regularization=0.01, tag="weak")
    (loss * 100.0).backward()
    assert abs(loss.item() - float(g[f"ic{ic}/loss"])) < 1e-4
    assert rel_err(o["popdensemap"].detach().cpu().numpy(), g[f"ic{ic}/popdensemap"]) < 1e-4
    assert rel_err(smp["building_counts"].cpu().numpy(), g[f"ic{ic}/building_counts"]) < 1e-4
    assert o["scale"].shape == g[f"ic{ic}/scale"].shape
    got = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(g[f"ic{ic}/grad_names"].tolist())
    for n, gr in got.items():
        r = g[f"ic{ic}/grad/{n}"]
        assert np.abs(gr.cpu().numpy() - r).max() <= 2e-4 * max(np.abs(r).max(), 1e-3), n
    with torch.no_grad():
        o2 = m({"input": s["input"]}, padding=True)
    assert rel_err(o2["popdensemap"].cpu().numpy(), g[f"ic{ic}/dense_pad1/popdensemap"]) < 1e-4
    m.eval()
    with torch.no_grad():
        s3 = {k: s[k] for k in ("input", "admin_mask", "census_idx")}
        o3 = m(s3, padding=False)
    for k, v in (("popdensemap", o3["popdensemap"]), ("scale", o3["scale"]), ("building_counts", s3["building_counts"])):
        assert rel_err(v.cpu().numpy(), g[f"ic{ic}/dense_pad0/{k}"]) < 1e-4, k


@pytest.mark.parametrize("fixture", ["g13_single_modality_shared", "g8_single_modality"])
@pytest.mark.parametrize("ic", [2, 4])
def test_native_step_vs_reference_golden(ic, fixture):
    g = np.load(os.path.join(G, fixture + ".npz"))
    _assert_step_vs_fixture(_trainer(ic, True), g, ic, native=True)


# ---- equal bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("B,H,W", GEOMS)
@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_is_bit_equal_to_the_per_launch_engine(ic, B, H, W, regime):
    _check(ic, _batch(ic, B, H, W), REGIMES[regime])


@pytest.mark.parametrize("kind", ["input6", "raw", "split"])
@pytest.mark.parametrize("B,H,W", [(2, 36, 36), (2, 37, 53)])
@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_data_forms(ic, B, H, W, kind):
    _check(ic, _batch(ic, B, H, W, kind))


@pytest.mark.parametrize("B,H,W", [(2, 36, 36), (2, 37, 53)])
@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_without_the_occupancy_product(ic, B, H, W):
    _check(ic, _batch(ic, B, H, W), occ=False, native_layer=True)


def _units_sample(ic, layer=False):
    """(2, 70, 90), K = 3, ragged: census_n = [3, 1] (tests/test_gpu_native_layer.py: _units_sample)"""
    inputs, y = U.make_case(B=2, H=70, W=90, units=((12, 3, 7), (9,)), channels=ic, seed=11)
    assert inputs["census_n"] == [3, 1] and tuple(inputs["census_idx"].shape) == (2, 3)
    s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    s["y"] = y.cuda()
    if layer:
        from tests.test_gpu_native_layer import _layer
        s["building_counts"] = _layer(2, 70, 90).cuda()
    return s


@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_multi_unit(ic):
    _check(ic, _units_sample(ic), multi=True, native_units=True)


@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_on_a_shipped_layer(ic):
    from tests.test_gpu_native_layer import _layer
    smp = _batch(ic, 2, 37, 53)
    smp["building_counts"] = _layer(2, 37, 53).cuda()
    _check(ic, smp, given=True, native_layer=True)


def _io(tr, smp, flags=(False, False), seed=3):
    from popcorn_amd.train import data_keys
    H, W = smp[data_keys(smp)[0]].shape[-2:]
    torch.manual_seed(seed)
    sel = tr._draw_selection(H, W)
    s = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in smp.items()}
    s["admin_mask"] = s["admin_mask"].float()
    return tr._native_io(s, sel, *flags), (s, sel)


@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_phases_issued_separately_equal_the_one_call_step(ic):
    from popcorn_amd import _lib as L
    from popcorn_amd.train import _ArenaOutputs
    smp = _batch(ic, 2, 37, 53)
    tr1, tr2 = _trainer(ic, True), _trainer(ic, True)
    torch.manual_seed(3)
    tr1.step(dict(smp))
    io, keep = _io(tr2, smp)
    with L.precision("fp32"), L.stream_scope():
        for ph in (L.PC_STEP_FWD, L.PC_STEP_BWD, L.PC_STEP_UPD):
            tr2._native_call(tr2._native_handle(), io, ph, L.stream_ptr())
    torch.cuda.synchronize()
    last2 = _ArenaOutputs(tr2._arena, io)
    for n in ("loss_out", "flat_g", "flat_p", "m", "v", "step_count"):
        assert _same(getattr(tr1, n), getattr(tr2, n)), n
    for k in LAST:
        assert _same(tr1.last[k], last2[k]), k


# ---- footprint ---------------------------------------------------------------------------------------------------------------------------
def _arena_needed(tr, smp, flags):
    from popcorn_amd import _lib as L
    io, keep = _io(tr, smp, flags)
    rc = L.lib().pc_train_step(tr._native_handle(), C.byref(io), L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.PC_ENOMEM and io.arena_needed > 0, rc
    return int(io.arena_needed)


def _fwd_bwd(tr, smp, flags):
    from popcorn_amd import _lib as L
    from popcorn_amd.train import _ArenaOutputs
    io, keep = _io(tr, smp, flags)
    arena = tr._arena
    with L.precision("fp32"), L.stream_scope():
        rc = tr._native_call(tr._native_handle(), io, L.PC_STEP_FWD | L.PC_STEP_BWD, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and tr._arena is arena, "the executor outgrew the size it reported"
    last = _ArenaOutputs(tr._arena, io)
    out = {"loss": tr.loss_out.clone(), "flat_g": tr.flat_g.clone()}
    out.update({k: last[k].clone() for k in LAST})
    return out


@pytest.mark.parametrize("regime", ["all", "limit2"])
@pytest.mark.parametrize("ic", [2, 4])
def test_native_single_exact_arena_whatever_it_held(ic, regime):
    """(2, 37, 53) in an arena of exactly ``arena_needed`` bytes between guard bands, filled with NaN bytes and then with 0x5A: loss, every
    gradient and every output bit-identical (density and scale maps where the mask selects: elsewhere nobody writes them), bands intact."""
    flags = REGIMES[regime]
    tr = _trainer(ic, True)
    with FP.Footprint("cuda", fill=FP.POISON) as fp:
        smp = _batch(ic, 2, 37, 53)
        need = _arena_needed(tr, smp, flags)
        assert tr._arena is None
        tr._arena = fp.alloc(need, torch.uint8, fill=FP.POISON, what="arena")
        assert tr._arena.numel() == need
        p0 = tr.flat_p.clone()
        runs = {}
        for name, byte in (("0xFF", 0xFF), ("0x5A", 0x5A)):
            tr._arena.fill_(byte)
            runs[name] = _fwd_bwd(tr, smp, flags)
        assert FP.bit_equal(tr.flat_p, p0)
    ref = runs["0xFF"]
    sel = ref["mask"].bool()
    assert bool(torch.isfinite(ref["loss"]).all()) and bool(torch.isfinite(ref["flat_g"]).all()) and int(sel.sum()) > 0
    assert float(ref["flat_g"][-600:].abs().max()) > 0
    for k, a in runs["0x5A"].items():
        if k in ("popdensemap", "scale_map"):
            assert FP.bit_equal(a[sel], ref[k][sel]), k
        else:
            bad = FP.differing(a, ref[k])
            assert not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].tolist())


# ---- opt-in ------------------------------------------------------------------------------------------------------------------------------
def test_native_single_is_opt_in():
    """Without the switch a one-stream trainer stays on the per-launch engine; the switch itself is new."""
    smp = _batch(2, 2, 48, 40)
    tr = _trainer(2, False)
    torch.manual_seed(3)
    tr.step(dict(smp))
    assert tr.native_steps == 0 and tr.native_single is False
    tr2 = _trainer(2, True)
    torch.manual_seed(3)
    tr2.step(dict(smp))
    assert tr2.native_steps == 1 and tr2.native_single is True


def test_the_switch_leaves_a_dual_stream_trainer_its_launches():
    from popcorn_amd import _lib as L
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    smp = t_native._batch(2, 37, 53)
    res = []
    for kw in ({}, {"native_single": True}):
        torch.manual_seed(1600)
        m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
        tr = FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, **kw)
        io, keep = _io(tr, smp)
        with L.precision("fp32"), L.stream_scope():
            tr._native_call(tr._native_handle(), io, L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, L.stream_ptr())
        torch.cuda.synchronize()
        res.append((int(io.launches), int(io.arena_needed), tr.loss_out.clone(), tr.flat_g.clone(), tr.flat_p.clone()))
    assert res[0][:2] == res[1][:2] and res[0][0] > 20
    for a, b in zip(res[0][2:], res[1][2:]):
        assert _same(a, b)


# ---- the C entry's refusals ----------------------------------------------------------------------------------------------------------------
def _plan_copy(tr):
    from popcorn_amd import _lib as L
    tr._native_handle()
    plan = L.PcStepPlan()
    C.memmove(C.byref(plan), C.byref(tr._native[1]), C.sizeof(L.PcStepPlan))
    return plan


@pytest.mark.parametrize("case", ["one_net_only", "no_stream", "bf16"])
def test_one_stream_plan_refusals_leave_the_arena_untouched(case):
    from popcorn_amd import _lib as L
    lib = L.lib()
    tr = _trainer(2, True)
    smp = _batch(2, 2, 37, 53)
    need = _arena_needed(tr, smp, (False, False))
    arena = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    io, keep = _io(tr, smp)
    io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    p0, g0 = tr.flat_p.clone(), tr.flat_g.clone()
    good = tr._native_handle()
    h = good
    if case != "bf16":
        plan = _plan_copy(tr)
        empty = L.PcStepStream()
        # the sar stream taken out of the extractor alone / out of both networks
        C.memmove(C.byref(plan.extractor.s[0]), C.byref(empty), C.sizeof(L.PcStepStream))
        if case == "no_stream":
            C.memmove(C.byref(plan.unet.s[0]), C.byref(empty), C.sizeof(L.PcStepStream))
        h = lib.pc_step_create(C.byref(plan))
        assert h
    try:
        with L.precision("bf16" if case == "bf16" else "fp32"):
            for call in ("step", "units"):
                if call == "step":
                    rc = lib.pc_train_step(h, C.byref(io), full, stream)
                else:
                    us, _ = _io(tr, {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in _units_sample(2).items()})
                    uio, units = us
                    uio.arena, uio.arena_bytes = arena.data_ptr(), arena.numel()
                    rc = lib.pc_train_step_units(h, C.byref(uio), C.byref(units), full, stream)
                assert rc == (L.PC_ENOTSUP if case == "bf16" else L.PC_EINVAL), (call, rc)
        torch.cuda.synchronize()
        assert bool((arena == 0x5A).all()) and _same(tr.flat_p, p0) and _same(tr.flat_g, g0)
    finally:
        if h != good:
            lib.pc_step_destroy(h)
    # the trainer's handle -- the refused one under bf16 -- then runs a good call in that arena
    with L.precision("fp32"):
        rc = lib.pc_train_step(good, C.byref(io), full, stream)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((arena == 0x5A).all()) and not _same(tr.flat_p, p0)
    assert bool(torch.isfinite(tr.loss_out).all())


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["-S1"], ["-S2", "-NIR"]], ids=["S1", "S2_NIR"])
def test_trainer_with_and_without_native_single(flags, tmp_path):
    """run_train.py <flags> -occmodel -pret --resident_region 320 352 --resident_units 40 --max_steps 3: equal loss and parameter bits with
    and without --native_single; the executor took every step of the run that asked for it."""
    from popcorn_amd.cli import run_train
    res = []
    for extra in ([], ["--native_single"]):
        argv = flags + ["-occmodel", "-pret", "--resident_region", "320", "352", "--resident_units", "40", "--max_steps", "3",
                        "-e", "1", "--save-model", "no", "--save_dir", str(tmp_path / ("b" if extra else "a"))] + extra
        t = run_train(argv)
        torch.cuda.synchronize()
        assert t.info["iter"] == 3
        res.append((t.fused.native_steps, t.fused.loss_out.clone(), t.fused.flat_p.clone(), t.fused.m.clone()))
    assert res[0][0] == 0 and res[1][0] == 3
    for a, b in zip(res[0][1:], res[1][1:]):
        assert _same(a, b)
