"""Whole steps under the memory-footprint harness (tests/footprint.py).

  * the native step executor in an arena of EXACTLY the size it reports (``arena_needed``), between two guard bands: the step must take
    it as it is (no regrowth), and leave the bands intact;
  * the executor's results must not depend on what the arena held before: zeros, 0xFF (NaN), or the remains of a larger region's step;
  * the per-launch engine and the inference forward with every ``torch.empty`` payload 0x00 and then 0xFF: same bits, bands intact.

Only two regions may differ between fills, and they are excluded by name below (EXCLUDED): ``popdensemap`` / ``scale_map`` outside the
selection on the per-launch ONE-UNIT path (tests/test_gpu_native_step.py documents it), and the pad columns of padded rows, which no
result tensor of these tests contains.  Everything else is compared bit for bit."""
import ctypes as C
import os

import pytest
import torch

import tests.test_gpu_native_step as t_native
import tests.test_gpu_units_native as t_un
from tests import footprint as FP
from tests.test_gpu_footprint_ops import _pair, fresh_workspaces

pytestmark = pytest.mark.gpu

REGIMES = t_native.REGIMES
EXCLUDED = ("popdensemap", "scale_map")          # outside the selection, per-launch one-unit path only
BIGGER = (2, 150, 90)                            # the region whose step leaves the arena dirty: larger than every geometry below
BIGGER_UNITS = "2x100x100"


def _native_io(tr, smp, flags, seed=3):
    """the arguments of one executor call, as FusedTrainStep.step prepares them"""
    from popcorn_amd import _lib as L
    from popcorn_amd.train import data_keys
    H, W = smp[data_keys(smp)[0]].shape[-2:]
    torch.manual_seed(seed)
    sel = tr._draw_selection(H, W)
    if H + W > L.PC_STEP_SEL_MAX:
        sel = sel.cuda()
    s = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in smp.items()}
    s["admin_mask"] = s["admin_mask"].float()
    io = tr._native_io(s, sel, *flags)
    io, units = io if isinstance(io, tuple) else (io, None)
    return io, units, (s, sel)


def _arena_needed(tr, smp, flags):
    """an arena-less call: PC_ENOMEM and the size the geometry takes (as test_pc_train_step_through_ctypes_vs_the_oracles_56_gradients)"""
    from popcorn_amd import _lib as L
    lib = L.lib()
    io, units, keep = _native_io(tr, smp, flags)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    phases = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    if units is None:
        rc = lib.pc_train_step(tr._native_handle(), C.byref(io), phases, stream)
    else:
        rc = lib.pc_train_step_units(tr._native_handle(), C.byref(io), C.byref(units), phases, stream)
    assert rc == L.PC_ENOMEM and io.arena_needed > 0, rc
    return int(io.arena_needed)


def _exact_arena_step(tr, make_sample, flags):
    with FP.Footprint("cuda", fill=FP.POISON) as fp:
        smp = make_sample()
        need = _arena_needed(tr, smp, flags)
        assert tr._arena is None
        arena = fp.alloc(need, torch.uint8, fill=FP.POISON, what="arena")
        assert arena.numel() == need and arena.data_ptr() % 512 == 0
        tr._arena = arena
        before = (tr.native_steps, tr.native_unit_steps)
        torch.manual_seed(3)
        loss = t_native._step(tr, smp, flags) if hasattr(tr, "_force_native") else tr.step(dict(smp), encoder_no_grad=flags[0],
                                                                                           unet_no_grad=flags[1])
        torch.cuda.synchronize()
        assert tr._arena is arena, ("the executor outgrew the size it reported", need, tr._arena.numel())
        assert (tr.native_steps, tr.native_unit_steps) != before
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(tr.flat_g).all()) and bool(torch.isfinite(tr.flat_p).all())
        assert bool(torch.isfinite(tr.last["popcount"]).all())
        assert fp.guarded >= 1 + len(smp) - ("census_n" in smp)
    return need


@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 64, 48), (1, 131, 77)])
def test_native_step_runs_in_an_arena_of_exactly_the_reported_size(B, H, W):
    """(1, 131, 77): W + 28 = 105 is odd, so the arena's rows carry pad columns on the building extractor's domain"""
    tr = t_native._fresh(True)
    _exact_arena_step(tr, lambda: t_native._batch(B, H, W), (False, False))
    assert tr.native_steps == 1


@pytest.mark.parametrize("regime", ["limit1", "limit2"])           # ("all" at this geometry: the test above)
def test_native_step_exact_arena_truncation_regimes(regime):
    tr = t_native._fresh(True)
    _exact_arena_step(tr, lambda: t_native._batch(2, 64, 48), REGIMES[regime])
    assert tr.native_steps == 1


@pytest.mark.parametrize("kind", ["raw", "split"])                 # ("input" at this geometry: the first test)
def test_native_step_exact_arena_input_forms(kind):
    tr = t_native._fresh(True)
    _exact_arena_step(tr, lambda: t_native._batch(1, 131, 77, kind), (False, False))
    assert tr.native_steps == 1


@pytest.mark.parametrize("name", ["2x32x32", "1x131x77"])
def test_native_units_step_exact_arena(name):
    tr = t_un._trainer(True)
    _exact_arena_step(tr, lambda: t_un._sample(name), (False, False))
    assert tr.native_unit_steps == 1 and tr.native_steps == 0


# ---- what the arena held before ----------------------------------------------------------------------------------------------------------
def _fwd_bwd(tr, smp, flags):
    """PC_STEP_FWD | PC_STEP_BWD in tr._arena (no parameter update: one trainer serves every run); clones of what the step leaves"""
    from popcorn_amd import _lib as L
    from popcorn_amd.train import _ArenaOutputs
    io, units, keep = _native_io(tr, smp, flags)
    arena = tr._arena
    with L.precision("fp32"), L.stream_scope():
        rc = tr._native_call(tr._native_handle(), io, L.PC_STEP_FWD | L.PC_STEP_BWD, L.stream_ptr(), units)
    torch.cuda.synchronize()
    assert rc == 0 and tr._arena is arena
    last = _ArenaOutputs(tr._arena, io, units)
    out = {"loss": tr.loss_out.clone(), "flat_g": tr.flat_g.clone()}
    out.update({k: last[k].clone() for k in ("popcount", "mask", "popdensemap", "scale_map")})
    return out


def _prefill_runs(tr, make_sample, make_bigger, flags):
    with FP.Footprint("cuda", fill=FP.POISON) as fp:
        smp, big = make_sample(), make_bigger()
        size = max(_arena_needed(tr, smp, flags), _arena_needed(tr, big, flags))
        tr._arena = fp.alloc(size, torch.uint8, what="arena")
        p0 = tr.flat_p.clone()
        runs = {}
        tr._arena.fill_(0x00)
        runs["zeros"] = _fwd_bwd(tr, smp, flags)
        tr._arena.fill_(0xFF)
        runs["0xFF"] = _fwd_bwd(tr, smp, flags)
        _fwd_bwd(tr, big, flags)
        runs["after a larger region"] = _fwd_bwd(tr, smp, flags)
        assert FP.bit_equal(tr.flat_p, p0) and fp.guarded >= 3
    return runs


def _assert_prefill_independent(runs, everywhere):
    ref = runs["zeros"]
    assert bool(torch.isfinite(ref["loss"]).all()) and int(ref["mask"].sum()) > 0
    sel = ref["mask"].bool()
    for name, got in runs.items():
        for k, a in got.items():
            if k in EXCLUDED and k not in everywhere:
                assert FP.bit_equal(a[sel], ref[k][sel]), (name, k, "inside the selection")
            else:
                bad = FP.differing(a, ref[k])
                assert not bool(bad.any()), (name, k, int(bad.sum()), bad.nonzero()[:4].tolist())


_one_trainer = []


def _shared_trainer():
    if not _one_trainer:
        _one_trainer.append(t_native._fresh(True))
    return _one_trainer[0]


@pytest.mark.parametrize("regime", ["all", "limit2"])
@pytest.mark.parametrize("B,H,W", [(2, 32, 32), (2, 64, 48), (1, 131, 77)])
def test_native_step_does_not_depend_on_what_the_arena_held(B, H, W, regime):
    """loss, every gradient, popcount and mask bit-identical whether the arena was zeros, NaN bytes or the remains of a (2, 150, 90) step;
    popdensemap / scale_map where the mask selects"""
    tr = _shared_trainer()
    runs = _prefill_runs(tr, lambda: t_native._batch(B, H, W), lambda: t_native._batch(*BIGGER), REGIMES[regime])
    tr._arena = None
    _assert_prefill_independent(runs, everywhere=())


_units_trainer = []


@pytest.mark.parametrize("name", ["2x32x32", "1x131x77"])
def test_native_units_step_does_not_depend_on_what_the_arena_held(name):
    """the multi-unit path: the same, and popdensemap at EVERY pixel (the head forward writes them all: the arena's map needs no zero fill)"""
    if not _units_trainer:
        _units_trainer.append(t_un._trainer(True))
    tr = _units_trainer[0]
    runs = _prefill_runs(tr, lambda: t_un._sample(name), lambda: t_un._sample(BIGGER_UNITS), (False, False))
    tr._arena = None
    _assert_prefill_independent(runs, everywhere=("popdensemap",))


def _made_by_the_package(fp):
    """guarded allocations whose creating call site is inside popcorn_amd/ (activations, outputs, workspaces), not the test's own"""
    import popcorn_amd
    return sum(r.site.startswith(os.path.dirname(os.path.abspath(popcorn_amd.__file__)) + os.sep) for r in fp.records)


# ---- per-launch engine -------------------------------------------------------------------------------------------------------------------
def _per_launch_trainer(precision):
    """the trainer of t_native._fresh / t_un._trainer(False), in the given arithmetic mode"""
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    m.set_precision(precision)
    return FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01)


def _per_launch_step(fill, precision, make_sample):
    from popcorn_amd import train as T
    with fresh_workspaces():
        with FP.Footprint("cuda", fill=fill) as fp:
            tr = _per_launch_trainer(precision)          # (flat parameters, gradients, Adam state: guarded too)
            smp = make_sample()
            prev, T.NATIVE_STEP = T.NATIVE_STEP, False
            try:
                torch.manual_seed(3)
                loss = tr.step(dict(smp))
            finally:
                T.NATIVE_STEP = prev
            torch.cuda.synchronize()
            assert tr.native_steps == 0 and tr.native_unit_steps == 0 and _made_by_the_package(fp) >= 30
            out = {"loss": loss.clone(), "flat_g": tr.flat_g.clone(), "flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
                   "step": tr.step_count.clone()}
            out.update({k: tr.last[k].clone() for k in ("popcount", "mask", "popdensemap", "scale_map")})
    return out


def _assert_same_step(clean, poison, one_unit):
    assert bool(torch.isfinite(clean["loss"]).all()) and int(clean["mask"].sum()) > 0 and bool((clean["step"] >= 0).all())
    sel = clean["mask"].bool()
    for k, a in poison.items():
        if one_unit and k in EXCLUDED:
            assert FP.bit_equal(a[sel], clean[k][sel]), (k, "inside the selection")
        else:
            bad = FP.differing(a, clean[k])
            assert not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,H,W,region", [(2, 32, 32, "disc"), (1, 37, 53, "disc"), (2, 64, 48, "disc")])
def test_per_launch_step_does_not_depend_on_what_torch_empty_returns(B, H, W, region, precision):
    """an eager step of the per-launch engine with every torch.empty payload (activations, gradients, workspaces) 0x00, then 0xFF:
    loss, gradients, parameters and Adam state after the update, popcount and mask bit-identical, bands intact"""
    make = lambda: t_native._batch(B, H, W, region=region)  # noqa: E731
    clean = _per_launch_step(FP.CLEAN, precision, make)
    poison = _per_launch_step(FP.POISON, precision, make)
    _assert_same_step(clean, poison, one_unit=True)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["2x32x32", "1x131x77"])
def test_per_launch_multi_unit_step_does_not_depend_on_what_torch_empty_returns(name, precision):
    clean = _per_launch_step(FP.CLEAN, precision, lambda: t_un._sample(name))
    poison = _per_launch_step(FP.POISON, precision, lambda: t_un._sample(name))
    _assert_same_step(clean, poison, one_unit=False)


# ---- inference ---------------------------------------------------------------------------------------------------------------------------
_pair_cache = []


@pytest.mark.parametrize("padding", [True, False])
@pytest.mark.parametrize("shape", [(1, 29, 31), (2, 33, 47)])
def test_inference_forward_does_not_depend_on_what_torch_empty_returns(shape, padding):
    """the forward of test_ragged_and_aligned_shapes (its oracle comparison included, under poison); padding = False takes the
    L.padded_rows path, whose pad columns are 0xFF in the poisoned run"""
    import tests.test_gpu_sizes as t_sizes
    if not _pair_cache:
        _pair_cache.append(_pair())
    pair = _pair_cache[0]
    B, H, W = shape
    x = torch.randn(B, 6, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    outs = {}
    for fill in (FP.CLEAN, FP.POISON):
        with fresh_workspaces():
            with FP.Footprint("cuda", fill=fill) as fp:
                if fill == FP.POISON:
                    t_sizes.test_ragged_and_aligned_shapes(pair, shape, padding)
                with torch.no_grad():
                    out = pair[0]({"input": fp.place(x)}, padding=padding)
                torch.cuda.synchronize()
                assert _made_by_the_package(fp) >= 20
                outs[fill] = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
    assert {"popdensemap", "scale", "popcount"} <= set(outs[FP.CLEAN])
    for k, a in outs[FP.CLEAN].items():
        bad = FP.differing(a, outs[FP.POISON][k])
        assert bool(torch.isfinite(a.float()).all()) and not bool(bad.any()), (k, int(bad.sum()), bad.nonzero()[:4].tolist())
