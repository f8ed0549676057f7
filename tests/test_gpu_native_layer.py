"""The native step executor on a shipped building layer (pc_train_step_layer / pc_train_step_units_layer, opt-in through
``FusedTrainStep(native_layer=True)``) and for models without the occupancy product.

What is compared: two trainers built from the same seed and the same model copy; the subject has ``native_layer=True``, the reference is
a default trainer, which takes the per-launch engine by itself for a given layer (and for ``occupancymodel=False``).  Both step on the
same batch with the same selection draw.  The comparison is equality of the int32 views -- both sides launch the same kernels with the
same arguments, anything else is a bug in the executor's geometry -- over loss, popcount, mask and building_counts of ``last``, all 56
gradients, and after two steps every parameter and both Adam moments.  ``popdensemap`` and ``scale_map`` are compared where the mask
selects on the one-unit path: outside the selection neither side writes them (the per-launch path returns ``torch.empty`` memory, the
executor arena bytes; tests/test_gpu_native_step.py documents it), so there is nothing to compare there; the multi-unit head writes
``popdensemap`` at every pixel and it is compared whole.

Layer: ``data.dataset.building_layer`` values (zeros on about 70 % of the pixels, counts 1 - 12); in the one-unit cases one NaN payload at
a pixel outside the supervised unit.  Shapes: (2, 100, 100) both networks' shared 128 x 128 domain (the layer must still switch the
extractor off there), (2, 70, 90) separate domains and rows that are no 16-byte multiples, (2, 131, 77) the odd golden geometry with
Up's zero pad, (1, 64, 96) where add_padding adds nothing."""
import ctypes as C

import pytest
import torch

import tests.test_gpu_native_step as t_native
from tests import footprint as FP
from tests import units_oracle as U

pytestmark = pytest.mark.gpu

REGIMES = t_native.REGIMES
I64_MAX = torch.iinfo(torch.int64).max


def _same(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _trainer(native_layer, given=True, occ=True, native_units=False):
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=occ, pretrained=True, biasinit=0.9407, sentinelbuildings=not given).cuda()
    kw = {"native_layer": True} if native_layer else {}
    return FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, native_units=native_units, **kw)


def _layer(B, H, W, seed=9):
    from popcorn_amd.data.dataset import building_layer
    g = torch.Generator().manual_seed(seed + H * 1000 + W)
    return torch.stack([building_layer(H, W, g) for _ in range(B)]).reshape(B, 1, H, W).contiguous()


def _sample(B, H, W, kind="input", layer=True):
    """The one-unit batch of tests/test_gpu_native_step.py, with a building layer that holds one NaN outside sample 0's unit."""
    smp = t_native._batch(B, H, W, kind)
    if layer:
        lay = _layer(B, H, W)
        outside = (smp["admin_mask"][0].cpu() != float(smp["census_idx"][0])).nonzero()
        assert outside.numel() > 0
        y, x = outside[len(outside) // 2].tolist()
        lay[0, 0, y, x] = float("nan")
        smp["building_counts"] = lay.cuda()
    return smp


def _units_sample(layer=True):
    """(2, 70, 90), K = 3, census_n = [3, 1]: the padding slots of the second row hold a duplicate of its valid id and INT64_MAX."""
    inputs, y = U.make_case(B=2, H=70, W=90, units=((12, 3, 7), (9,)), channels=6, seed=11)
    assert inputs["census_n"] == [3, 1] and tuple(inputs["census_idx"].shape) == (2, 3)
    inputs["census_idx"][1, 1], inputs["census_idx"][1, 2] = 9, I64_MAX
    s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    s["y"] = y.cuda()
    if layer:
        s["building_counts"] = _layer(2, 70, 90).cuda()
    return s


def _two_steps(tr, smp, flags=(False, False)):
    out = []
    for it in range(2):
        torch.manual_seed(3 + it)
        loss = tr.step(dict(smp), encoder_no_grad=flags[0], unet_no_grad=flags[1])
        torch.cuda.synchronize()
        assert len(tr.grads) == 56
        o = {"loss": loss.clone(), "flat_g": tr.flat_g.clone(), "flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
             "step": tr.step_count.clone()}
        o.update({"grad " + n: g.clone() for n, g in tr.grads.items()})
        o.update({k: tr.last[k].clone() for k in ("popcount", "popdensemap", "scale_map", "mask", "building_counts")})
        if "slot" in tr.last:
            o["slot"] = tr.last["slot"].clone()
        out.append(o)
    return out


def _assert_same_steps(got, want, multi=False):
    assert len(got) == len(want) == 2
    for it, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(b)
        sel = b["mask"].bool()
        assert int(sel.sum()) > 0 and bool(torch.isfinite(b["loss"]).all())
        for n in a:
            if n == "scale_map" or (n == "popdensemap" and not multi):
                print(f"[{it}] {n}: {int((a[n][sel].view(torch.int32) != b[n][sel].view(torch.int32)).sum())} differing selected pixels")
                assert _same(a[n][sel], b[n][sel]), (n, it)
            else:
                assert _same(a[n], b[n]), (n, it, (a[n].float() - b[n].float()).abs().nan_to_num(0).max().item())


_reference = {}


def _per_launch_steps(key, make_sample, flags=(False, False), **model):
    """Two steps of a default trainer (no opt-in: the per-launch engine for a given layer / a model without the product), once per case."""
    if key not in _reference:
        tr = _trainer(False, **model)
        _reference[key] = _two_steps(tr, make_sample(), flags)
        assert tr.native_steps == 0 and tr.native_unit_steps == 0
    return _reference[key]


def _check_case(B, H, W, kind="input", regime="all"):
    smp = _sample(B, H, W, kind)
    fed = smp["building_counts"].clone()
    tr = _trainer(True)
    got = _two_steps(tr, smp, REGIMES[regime])
    assert tr.native_steps == 2 and tr.native_unit_steps == 0
    assert _same(got[1]["building_counts"], fed) and _same(smp["building_counts"], fed)        # the layer is the output, and untouched
    assert tr.last["building_counts"].data_ptr() == smp["building_counts"].data_ptr()          # the caller's own tensor, no plane
    _assert_same_steps(got, _per_launch_steps((B, H, W, kind, regime), lambda: _sample(B, H, W, kind), REGIMES[regime]))


@pytest.mark.parametrize("regime", list(REGIMES))
def test_regimes_equal_the_per_launch_engine(regime):
    _check_case(2, 70, 90, "input", regime)


@pytest.mark.parametrize("kind", ["input", "raw", "split"])
@pytest.mark.parametrize("B,H,W", [(2, 100, 100), (2, 70, 90)])
def test_input_forms_equal_the_per_launch_engine(B, H, W, kind):
    _check_case(B, H, W, kind)


@pytest.mark.parametrize("B,H,W", [(2, 131, 77), (1, 64, 96)])
def test_odd_and_unpadded_geometries_equal_the_per_launch_engine(B, H, W):
    _check_case(B, H, W)


def test_multi_unit_step_equals_the_per_launch_engine():
    smp = _units_sample()
    fed = smp["building_counts"].clone()
    tr = _trainer(True, native_units=True)
    torch.manual_seed(3)
    tr.step(dict(smp))
    assert tr.native_unit_steps == 1 and tr.native_steps == 0
    tr2 = _trainer(True, native_units=True)
    got = _two_steps(tr2, smp)
    assert tr2.native_unit_steps == 2 and tr2.native_steps == 0
    assert tuple(got[0]["popcount"].shape) == (4,) and _same(smp["building_counts"], fed)
    _assert_same_steps(got, _per_launch_steps("units", _units_sample), multi=True)
    # without native_units the layer flag alone keeps multi-unit samples on the per-launch engine
    tr3 = _trainer(True)
    tr3.step(dict(smp))
    assert tr3.native_unit_steps == 0 and tr3.native_steps == 0


def _io(tr, smp, flags=(False, False), seed=3):
    """the arguments of one executor call, as FusedTrainStep.step prepares them"""
    from popcorn_amd.train import data_keys
    H, W = smp[data_keys(smp)[0]].shape[-2:]
    torch.manual_seed(seed)
    sel = tr._draw_selection(H, W)
    s = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in smp.items()}
    s["admin_mask"] = s["admin_mask"].float()
    return tr._native_io(s, sel, *flags), (s, sel)


def _layer_ptr(io):
    return None if io._layer is None else C.c_void_p(io._layer.data_ptr())


def _sized(tr, smp):
    """an arena-less call: PC_ENOMEM and the size the geometry takes; nothing is enqueued"""
    from popcorn_amd import _lib as L
    io, keep = _io(tr, smp)
    with L.precision("fp32"):
        rc = L.lib().pc_train_step_layer(tr._native_handle(), C.byref(io), _layer_ptr(io), L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.PC_ENOMEM and io.arena_needed > 0, rc
    return int(io.arena_needed)


def test_data_parallel_phases_equal_the_single_call():
    """FWD | BWD | UPD as three calls under io.dp = 1 (the forced one-rank reducer's identity collectives in between) = the one-call step,
    bit for bit; the layer named with FWD is the one BWD reads: another pointer is PC_EINVAL, NULL and the same pointer are accepted."""
    from popcorn_amd import _lib as L
    smp = _sample(2, 70, 90)
    tr1, tr2 = _trainer(True), _trainer(True)
    torch.manual_seed(3)
    tr1.step(dict(smp))
    torch.cuda.synchronize()
    assert tr1.native_steps == 1
    io, keep = _io(tr2, smp)
    io.dp = 1
    h = tr2._native_handle()
    other = torch.zeros_like(smp["building_counts"])
    with L.precision("fp32"), L.stream_scope():
        stream = L.stream_ptr()
        tr2._native_call(h, io, L.PC_STEP_FWD, stream)
        assert io.off_building == -1
        g0 = tr2.flat_g.clone()
        assert L.lib().pc_train_step_layer(h, C.byref(io), C.c_void_p(other.data_ptr()), L.PC_STEP_BWD, stream) == L.PC_EINVAL
        assert L.lib().pc_train_step_layer(h, C.byref(io), C.c_void_p(other.data_ptr()), L.PC_STEP_UPD, stream) == L.PC_EINVAL
        torch.cuda.synchronize()
        assert _same(tr2.flat_g, g0)                                                  # nothing was enqueued
        assert L.lib().pc_train_step_layer(h, C.byref(io), None, L.PC_STEP_BWD, stream) == 0
        tr2._native_call(h, io, L.PC_STEP_UPD, stream)                                # (the same pointer again)
    torch.cuda.synchronize()
    for n in ("loss_out", "flat_g", "flat_p", "m", "v", "step_count"):
        a, b = getattr(tr1, n), getattr(tr2, n)
        print(n, "max abs difference", (a.float() - b.float()).abs().max().item())
    for n in ("loss_out", "flat_g", "flat_p", "m", "v", "step_count"):
        assert _same(getattr(tr1, n), getattr(tr2, n)), n


@pytest.mark.parametrize("layer", [True, False], ids=["layer", "extractor"])
@pytest.mark.parametrize("B,H,W", [(2, 70, 90), (2, 100, 100)])
def test_model_without_the_occupancy_product(B, H, W, layer):
    """occupancymodel = False: the mask is the region only, the head multiplies by ones, building_counts stays the layer / the score."""
    smp = _sample(B, H, W, layer=layer)
    tr = _trainer(True, given=layer, occ=False)
    got = _two_steps(tr, smp)
    assert tr.native_steps == 2
    sel = got[0]["mask"].bool()
    assert _same(got[0]["popdensemap"][sel], got[0]["scale_map"][sel])                # (x 1.0)
    if layer:
        assert _same(got[0]["building_counts"], smp["building_counts"])
    _assert_same_steps(got, _per_launch_steps((B, H, W, "nonocc", layer), lambda: _sample(B, H, W, layer=layer), given=layer, occ=False))


def test_fewer_launches_and_a_smaller_arena_than_the_extractor_step():
    """io.launches and io.arena_needed of the step on a layer against the extractor step of the same geometry."""
    from popcorn_amd import _lib as L
    full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    res = {}
    for B, H, W in ((2, 70, 90), (2, 100, 100)):
        for given in (True, False):
            tr = _trainer(True, given=given)
            io, keep = _io(tr, _sample(B, H, W, layer=given))
            with L.precision("fp32"), L.stream_scope():
                tr._native_call(tr._native_handle(), io, full, L.stream_ptr())
            torch.cuda.synchronize()
            assert (io.off_building == -1) == given
            res[B, H, W, given] = (io.launches, int(io.arena_needed))
        print(f"{B}x{H}x{W}: layer {res[B, H, W, True]}, extractor {res[B, H, W, False]} (launches, arena bytes)")
        assert res[B, H, W, True][1] < res[B, H, W, False][1]
    # separate domains: the extractor's whole launch chain is gone.  On the shared 128 x 128 domain the extractor never had launches of
    # its own -- it rode in the trainable network's grouped launches, and score + mask were one launch where the mask now is one -- so
    # the count is the same there and every grouped launch carries two (network, stream) pairs instead of four
    assert res[2, 70, 90, True][0] < res[2, 70, 90, False][0]
    assert res[2, 100, 100, True][0] <= res[2, 100, 100, False][0]


def test_exact_arena_under_both_fills_and_the_layer_is_not_written():
    """The step in an arena of exactly ``arena_needed`` bytes between guard bands, the arena and every ``torch.empty`` payload 0x00 and then
    0xFF: equal bits, the bands intact, and the caller's layer -- between bands of its own -- bit-identical before and after."""
    cpu = {k: v.cpu() for k, v in _sample(2, 70, 90).items()}
    runs = {}
    for fill in (FP.CLEAN, FP.POISON):
        tr = _trainer(True)
        with FP.Footprint("cuda", fill=fill) as fp:
            smp = {k: fp.place(v) for k, v in cpu.items()}
            need = _sized(tr, smp)
            assert tr._arena is None
            arena = fp.alloc(need, torch.uint8, fill=fill, what="arena")
            assert arena.numel() == need
            tr._arena = arena
            torch.manual_seed(3)
            loss = tr.step(dict(smp))
            torch.cuda.synchronize()
            assert tr._arena is arena, ("the executor outgrew the size it reported", need, tr._arena.numel())
            assert tr.native_steps == 1 and fp.guarded >= 1 + len(smp)
            assert _same(smp["building_counts"], cpu["building_counts"])
            assert tr.last["building_counts"].data_ptr() == smp["building_counts"].data_ptr()
            runs[fill] = {"loss": loss.clone(), "flat_g": tr.flat_g.clone(), "flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone()}
            runs[fill].update({k: tr.last[k].clone() for k in ("popcount", "mask", "popdensemap", "scale_map")})
    a, b = runs[FP.CLEAN], runs[FP.POISON]
    sel = a["mask"].bool()
    assert bool(torch.isfinite(a["loss"]).all()) and int(sel.sum()) > 0
    for k in a:
        if k in ("popdensemap", "scale_map"):
            assert _same(a[k][sel], b[k][sel]), k
        else:
            assert _same(a[k], b[k]), k


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_cpu_layer_raises_naming_the_key():
    smp = _sample(2, 70, 90)
    smp["building_counts"] = smp["building_counts"].cpu()
    tr = _trainer(True)
    p0 = tr.flat_p.clone()
    with pytest.raises(ValueError, match="building_counts"):
        tr.step(dict(smp))
    torch.cuda.synchronize()
    assert tr.native_steps == 0 and _same(tr.flat_p, p0)


def test_a_three_dimensional_layer_raises_naming_the_key():
    smp = _sample(2, 70, 90)
    smp["building_counts"] = smp["building_counts"][:, 0].contiguous()
    tr = _trainer(True)
    with pytest.raises(ValueError, match="building_counts"):
        tr.step(dict(smp))
    assert tr.native_steps == 0


def test_a_sentinelbuildings_model_ignores_the_layer():
    res = []
    for with_key in (True, False):
        tr = _trainer(True, given=False)
        smp = _sample(2, 70, 90, layer=with_key)
        got = _two_steps(tr, smp)
        assert tr.native_steps == 2
        res.append(got)
    assert not _same(res[0][0]["building_counts"], _sample(2, 70, 90)["building_counts"])      # the extractor's score
    _assert_same_steps(*res)


def test_a_stream_under_capture_is_still_refused():
    from popcorn_amd import _lib as L
    smp = _sample(2, 70, 90)
    tr = _trainer(True)
    io, keep = _io(tr, smp)
    arena = torch.empty(_sized(tr, smp), dtype=torch.uint8, device="cuda")
    io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
    h = tr._native_handle()
    p0, x = tr.flat_p.clone(), torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with L.precision("fp32"), torch.cuda.graph(g):
        x += 1                                                                        # (a kernel node: the capture is not empty)
        rc = L.lib().pc_train_step_layer(h, C.byref(io), _layer_ptr(io), L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.PC_ENOTSUP
    torch.cuda.synchronize()
    assert _same(tr.flat_p, p0)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------------
TRAIN = "-S2 -NIR -S1 -occmodel -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --max_steps 3 --save-model no"
RESIDENT = "--resident_region 320 352 --resident_units 40 --building_layer"


@pytest.mark.parametrize("feed", ["", " --resident_assemble"], ids=["region", "assemble"])
def test_run_train_native_layer_on_the_resident_feeds(tmp_path, feed):
    from popcorn_amd.cli import run_train
    runs = []
    for tag, flag in (("native", " --native_layer"), ("per_launch", "")):
        t = run_train(TRAIN.split() + ["--save_dir", str(tmp_path / tag)] + (RESIDENT + feed + flag).split())
        torch.cuda.synchronize()
        assert t.info["iter"] == 3 and t.region.buildings is not None
        assert t.fused.native_steps == (3 if flag else 0)
        runs.append((t.fused.loss_out.clone(), t.fused.flat_p.clone(), t.fused.m.clone(), t.fused.v.clone()))
    assert bool(torch.isfinite(runs[0][0]).all())
    for a, b in zip(*runs):
        assert _same(a, b)
