"""The native forward executor (pc_forward, include/popcorn_hip.h; popcorn_amd/infer.py): ``model(sample, padding=False)`` in eval mode
under ``no_grad`` with the dense head as ONE C-ABI call, opt-in through ``model.native_forward = True``.

What is compared: the SAME model and the SAME sample through the executor and through the per-launch engine (the flag off).  Both sides
launch the same kernels with the same arguments -- only the host side differs -- so every comparison is equality of the int32 views of
popcount, popdensemap, scale and building_counts; anything else is a bug in the executor's geometry.  The dense head writes every pixel
of its maps, so they are compared whole.

Geometries: (2, 100, 100) both networks on the shared 128 x 128 domain (grouped launches), (2, 37, 53) odd sides with rows that are no
multiple of 4 floats on both domains, (1, 64, 96) no U-Net padding, (3, 131, 77) the odd golden geometry, (1, 22, 22) the smallest side
the reflect rule admits (pads 21 / 21)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_native_layer as t_layer
import tests.test_gpu_native_step as t_native
from tests import footprint as FP

pytestmark = pytest.mark.gpu

GEOMS = [(2, 100, 100), (2, 37, 53), (1, 64, 96), (3, 131, 77), (1, 22, 22)]
KEYS = ("popcount", "popdensemap", "scale", "building_counts")
G = os.path.join(os.path.dirname(__file__), "golden")
_same = t_layer._same
_models = {}


def _model(occ=True, senb=True, seed=1600, fresh=False):
    from popcorn_amd.model import POPCORN
    key = (occ, senb, seed)
    if fresh or key not in _models:
        torch.manual_seed(seed)
        m = POPCORN(input_channels=6, occupancymodel=occ, pretrained=True, biasinit=0.9407, sentinelbuildings=senb).cuda().eval()
        if fresh:
            return m
        _models[key] = m
    return _models[key]


def _sample(B, H, W, admin=True, layer=False):
    s = t_native._batch(B, H, W)
    s.pop("y")
    if not admin:
        s.pop("admin_mask"), s.pop("census_idx")
    if layer:
        s["building_counts"] = t_layer._layer(B, H, W).cuda()
    return s


def _run(model, sample, native):
    """One forward of ``model`` (flag = ``native``) on a copy of the sample dict: clones of the four results."""
    model.native_forward = bool(native)
    n0 = model.native_forwards
    s = dict(sample)
    try:
        with torch.no_grad():
            o = model(s, padding=False)
        torch.cuda.synchronize()
        assert model.native_forwards == n0 + (1 if native else 0)
        out = {k: (None if o[k] is None else o[k].clone()) for k in ("popcount", "popdensemap", "scale")}
        out["building_counts"] = s["building_counts"].clone()
        out["launches"], out["arena_needed"] = getattr(o, "launches", None), getattr(o, "arena_needed", None)
    finally:
        model.native_forward = False
    return out


def _assert_equal(got, want, where=""):
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (k, where)
            continue
        diff = int(FP.differing(got[k], want[k]).sum()) if got[k].shape == want[k].shape else -1
        print(f"{where} {k}: {diff} differing elements of {want[k].numel()}")
        assert _same(got[k], want[k]), (k, where)
    assert bool(torch.isfinite(want["popcount"]).all()) and float(want["popdensemap"].nan_to_num(0).abs().sum()) > 0


# ---- 1. the entry point against the per-launch forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("admin", [True, False], ids=["region", "plain_sum"])
@pytest.mark.parametrize("B,H,W", GEOMS)
def test_native_forward_equals_the_per_launch_forward(B, H, W, admin):
    m = _model()
    s = _sample(B, H, W, admin)
    want = _run(m, s, False)
    got = _run(m, s, True)
    assert tuple(got["popdensemap"].shape) == (B, H, W) and tuple(got["building_counts"].shape) == (B, 1, H, W)
    _assert_equal(got, want, f"{B}x{H}x{W}")


@pytest.mark.parametrize("padded", [False, True], ids=["dense_rows", "padded_rows"])
@pytest.mark.parametrize("B,H,W", [(1, 36, 38), (1, 100, 70), (1, 36, 96)])
def test_widths_where_the_row_layout_decides_the_up_block_form(B, H, W, padded):
    """Extractor domains 64 x 66 and 128 x 98 (level 1: rows of 66 / 98 floats are no 16-byte multiples) and 64 x 124 (level 2: rows of
    62 floats): the
    per-launch engine composes the Up block there under ``L.padded_rows()`` (eval.py) and not outside it, and the two forms round
    differently.  The executor returns the bits of the engine in the same context, both times."""
    from popcorn_amd import _lib as L
    m = _model()
    s = _sample(B, H, W)
    with L.padded_rows(padded):
        want = _run(m, s, False)
        got = _run(m, s, True)
    assert m._native_fwd.last_io.flags == (0 if padded else L.PC_FWD_DENSE_ROW_RULE)
    _assert_equal(got, want, f"{B}x{H}x{W} padded_rows={padded}")


def _nf(model):
    from popcorn_amd import infer
    return infer.NativeForward(model)


def _call(nf, io, layer=None):
    from popcorn_amd import _lib as L
    with L.precision("fp32"):
        return L.lib().pc_forward(nf.handle(), C.byref(io), None if layer is None else C.c_void_p(layer),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_22_is_the_smallest_side_and_21_is_refused_with_nothing_enqueued():
    from popcorn_amd import _lib as L
    from popcorn_amd.model.popcorn import pad_geometry
    assert pad_geometry(22, 22, False) == (21, 21, 21, 21) and pad_geometry(21, 21, False) == (21, 22, 21, 22)
    m = _model()
    nf = _nf(m)
    io, _ = nf._io({"input": torch.zeros(1, 6, 22, 22, device="cuda")})
    assert _call(nf, io) == L.PC_ENOMEM                                  # (an arena-less call: the size of the smallest geometry)
    arena = torch.full((int(io.arena_needed),), 0x5A, dtype=torch.uint8, device="cuda")
    for side in range(1, 22):
        for hw in ((side, 64), (64, side), (side, side)):
            io, _ = nf._io({"input": torch.zeros(1, 6, *hw, device="cuda")})
            io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
            assert _call(nf, io) == L.PC_EINVAL, hw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())                                   # nothing was enqueued
    io, _ = nf._io({"input": torch.zeros(1, 6, 22, 22, device="cuda")})
    io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
    assert _call(nf, io) == 0 and io.launches > 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):                                      # the per-launch engine's own rule agrees
        with torch.no_grad():
            m({"input": torch.zeros(1, 6, 21, 21, device="cuda")}, padding=False)


def test_side_stream_disabled_equals_the_forked_form(monkeypatch):
    """POPCORN_STEP_SIDE_PX=0 at handle creation: the extractor's chain stays on the caller's stream and its activations are released
    before the U-Net's are carved."""
    m = _model()
    s = _sample(2, 37, 53)
    forked = _run(m, s, True)
    monkeypatch.setenv("POPCORN_STEP_SIDE_PX", "0")
    m2 = _model(fresh=True)
    m2.load_state_dict(m.state_dict())
    plain = _run(m2, s, True)
    monkeypatch.delenv("POPCORN_STEP_SIDE_PX")
    _assert_equal(plain, forked, "sequential against forked")
    print("sequential (launches, arena)", plain["launches"], plain["arena_needed"], "forked", forked["launches"], forked["arena_needed"])
    assert plain["launches"] < forked["launches"]                        # (the fork's and the join's event operations are counted)
    assert plain["arena_needed"] <= forked["arena_needed"]               # (its activations are released before the U-Net's are carved)


@pytest.mark.parametrize("name", ["b2_100", "b1_131x77", "b2_64"])
def test_native_forward_meets_the_reference_fixture(name):
    """tests/golden g2, the dense padding=False cases, at the bar of tests/test_gpu_model.py (1e-4 relative; the score 1e-5 absolute)."""
    from tests.test_gpu_model import rel_err
    g = np.load(os.path.join(G, "g2_forward.npz"))
    m = _model()
    inp = {"input": torch.from_numpy(g[f"{name}/input"]).cuda(), "admin_mask": torch.from_numpy(g[f"{name}/admin_mask"]).cuda(),
           "census_idx": torch.from_numpy(g[f"{name}/census_idx"]).cuda()}
    o = _run(m, inp, True)
    tag = f"{name}/pad0_sp0"
    np.testing.assert_allclose(o["building_counts"].cpu().numpy(), g[f"{name}/building_counts"], rtol=0, atol=1e-5)
    for k in ("popdensemap", "popcount", "scale"):
        e = rel_err(o[k].cpu().numpy(), g[f"{tag}/{k}"])
        print(name, k, "relative error", e)
        assert o[k].shape == g[f"{tag}/{k}"].shape and e < 1e-4, (k, e)
    if f"{name}/noadmin/popcount" in g.files:
        o = _run(m, {"input": inp["input"]}, True)
        assert rel_err(o["popcount"].cpu().numpy(), g[f"{name}/noadmin/popcount"]) < 1e-4
        assert rel_err(o["popdensemap"].cpu().numpy(), g[f"{name}/noadmin/popdensemap"]) < 1e-4


# ---- the building layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (2, 100, 100)])
def test_layer_replaces_the_extractor(B, H, W):
    m = _model(senb=False)
    s = t_layer._sample(B, H, W)                                         # (one NaN payload outside sample 0's unit: used bit for bit)
    s.pop("y")
    assert int(torch.isnan(s["building_counts"]).sum()) == 1
    want = _run(m, s, False)
    assert int(torch.isnan(want["popdensemap"]).sum()) == 1
    cpu = {k: v.cpu() for k, v in s.items()}
    with FP.Footprint("cuda", fill=FP.POISON) as fp:
        placed = {k: fp.place(v) for k, v in cpu.items()}
        got = _run(m, placed, True)
        assert _same(placed["building_counts"], cpu["building_counts"])  # only read (the bands are checked on leaving the block)
        nf = m._native_fwd
        assert nf.last_io.off_building == -1
    _assert_equal(got, want, "layer")
    assert _same(got["building_counts"], cpu["building_counts"].cuda())
    # against the extractor on the same geometry: no plane, a smaller arena, fewer launches (on separate domains the extractor's chain is
    # gone; on the shared domain it rode in the grouped launches and its score's launch goes)
    ext = _run(_model(), _sample(B, H, W), True)
    print(f"{B}x{H}x{W}: layer (launches, arena) {got['launches'], got['arena_needed']}, extractor {ext['launches'], ext['arena_needed']}")
    assert got["arena_needed"] < ext["arena_needed"]
    assert got["launches"] < ext["launches"]


def test_a_sentinelbuildings_model_ignores_the_layer():
    m = _model()
    with_key, without = _run(m, _sample(2, 37, 53, layer=True), True), _run(m, _sample(2, 37, 53), True)
    _assert_equal(with_key, without, "sentinelbuildings")
    assert not _same(with_key["building_counts"], _sample(2, 37, 53, layer=True)["building_counts"])      # the extractor's score


@pytest.mark.parametrize("layer", [True, False], ids=["layer", "extractor"])
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (2, 100, 100)])
def test_model_without_the_occupancy_product(B, H, W, layer):
    m = _model(occ=False, senb=not layer)
    s = _sample(B, H, W, layer=layer)
    want, got = _run(m, s, False), _run(m, s, True)
    assert got["scale"] is None and want["scale"] is None
    _assert_equal(got, want, "no product")


# ---- input forms through ctypes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["raw", "split"])
def test_raw_and_split_inputs_equal_the_normalised_input(kind):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    B, H, W = 2, 37, 53
    m = _model()
    nf = _nf(m)
    s = t_native._batch(B, H, W, kind)
    if kind == "raw":
        x = ops.select_normalize(s["raw"], stats.BAND6, stats.MEAN6, stats.STD6)
    else:
        x = ops.ingest_split(s["raw_s2"], s["raw_s1"], tuple(range(6)), stats.MEAN6, stats.STD6, 0, 0, 0, 0, cl8=False)
    assert tuple(x.shape) == (B, 6, H, W)
    res = []
    for smp in ({"input": x.contiguous(), "admin_mask": s["admin_mask"], "census_idx": s["census_idx"]}, {k: v for k, v in s.items() if k != "y"}):
        o = nf.forward(smp)
        torch.cuda.synchronize()
        res.append({k: (o[k].clone()) for k in KEYS})
    assert nf.last_io.data_kind == {"raw": 1, "split": 2}[kind]
    _assert_equal(res[1], res[0], kind)


# ---- footprint ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (2, 100, 100)])
def test_exact_arena_between_guard_bands_under_both_fills(B, H, W):
    from popcorn_amd import _lib as L
    m = _model()
    cpu = {k: v.cpu() for k, v in _sample(B, H, W).items()}
    runs = {}
    for fill in (FP.CLEAN, FP.POISON):
        nf = _nf(m)
        with FP.Footprint("cuda", fill=fill) as fp:
            smp = {k: fp.place(v) for k, v in cpu.items()}
            io, _ = nf._io(smp)
            assert _call(nf, io) == L.PC_ENOMEM and io.arena_needed > 0   # an arena-less call: the size, nothing enqueued
            need = int(io.arena_needed)
            arena = fp.alloc(need, torch.uint8, fill=fill, what="arena")
            before = arena.clone()
            io.arena, io.arena_bytes = arena.data_ptr(), need - 1
            assert _call(nf, io) == L.PC_ENOMEM and int(io.arena_needed) == need
            torch.cuda.synchronize()
            assert torch.equal(arena, before)                            # one byte less: nothing was enqueued
            nf._arena = arena
            o = nf.forward(smp)
            torch.cuda.synchronize()
            assert nf._arena is arena, ("the executor outgrew the size it reported", need)
            assert int(nf.last_io.arena_needed) == need and fp.guarded >= 1 + len(smp)
            runs[fill] = {k: o[k].clone() for k in KEYS}
    _assert_equal(runs[FP.POISON], runs[FP.CLEAN], "0xFF against 0x00")


def test_arena_next_to_a_training_forward_under_unet_no_grad():
    """What the issue asks to be recorded: arena_needed of pc_forward next to a training FWD (sized with its BWD / UPD) under unet_no_grad."""
    from popcorn_amd import _lib as L
    for B, H, W in ((2, 37, 53), (2, 100, 100)):
        tr = t_native._fresh(True)
        smp = t_native._batch(B, H, W)
        io, keep = t_layer._io(tr, smp, flags=(True, True))
        with L.precision("fp32"):
            rc = L.lib().pc_train_step_layer(tr._native_handle(), C.byref(io), None, L.PC_STEP_FWD, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == L.PC_ENOMEM
        o = _run(_model(), _sample(B, H, W), True)
        print(f"{B}x{H}x{W}: pc_forward arena {o['arena_needed']} bytes, training FWD (unet_no_grad) {int(io.arena_needed)} bytes")
        assert o["arena_needed"] <= int(io.arena_needed)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_excluding_condition_falls_back_and_leaves_the_counter(monkeypatch):
    from popcorn_amd import engine as E
    from popcorn_amd.model import POPCORN
    m = _model()
    s = _sample(1, 64, 96)
    want = _run(m, s, False)
    m.native_forward = True
    try:
        n0 = m.native_forwards
        with torch.no_grad():
            torch.manual_seed(5)
            m(dict(s), padding=False, sparse=True)
            m(dict(s), padding=True)
            m.set_precision("bf16")
            m(dict(s), padding=False)
            m.set_precision("fp32")
            with pytest.raises(AssertionError):                          # today's path, which takes no fp64 input either (L.src)
                m({**s, "input": s["input"].double()}, padding=False)
            wide = torch.zeros(1, 6, 64, 192, device="cuda")
            wide[..., ::2] = s["input"]
            o = m({**s, "input": wide[..., ::2]}, padding=False)
            assert _same(o["popdensemap"], want["popdensemap"])
            m({"input": s["input"], "admin_mask": s["admin_mask"], "census_idx": s["census_idx"].reshape(1, 1)}, padding=False)
            monkeypatch.setattr(E, "FUSED_LEVEL2", False)
            m(dict(s), padding=False)
            monkeypatch.setattr(E, "FUSED_LEVEL2", True)
        m(dict(s), padding=False, unet_no_grad=False)                    # grad enabled, trainable parameters: a graph is built
        torch.manual_seed(1600)
        single = POPCORN(input_channels=2, occupancymodel=True, pretrained=True, sentinelbuildings=True).cuda().eval()
        single.native_forward = True
        with torch.no_grad():
            single({"input": s["input"][:, 4:6].contiguous()}, padding=False)
        torch.cuda.synchronize()
        assert m.native_forwards == n0 and single.native_forwards == 0
        with torch.no_grad():
            m(dict(s), padding=False)
        assert m.native_forwards == n0 + 1
    finally:
        m.native_forward = False
        m.set_precision("fp32")


@pytest.mark.parametrize("key", ["input", "admin_mask", "building_counts"])
def test_a_cpu_tensor_raises_naming_the_key(key):
    m = _model(senb=False)
    s = _sample(2, 37, 53, layer=True)
    s[key] = s[key].cpu()
    m.native_forward = True
    n0 = m.native_forwards
    try:
        with pytest.raises(ValueError, match=key), torch.no_grad():
            m(s, padding=False)
        assert m.native_forwards == n0
    finally:
        m.native_forward = False


def test_a_wrong_dtype_raises_naming_the_key():
    m = _model()
    m.native_forward = True
    try:
        for key, bad in (("admin_mask", lambda t: t.double()), ("census_idx", lambda t: t.int())):
            s = _sample(2, 37, 53)
            s[key] = bad(s[key])
            with pytest.raises(ValueError, match=key), torch.no_grad():
                m(s, padding=False)
    finally:
        m.native_forward = False


def test_c_level_refusals_enqueue_nothing():
    from popcorn_amd import _lib as L
    m = _model(senb=False)
    nf = _nf(m)
    nf.handle()
    s = _sample(2, 37, 53, layer=True)
    io, layer = nf._io(s)
    assert _call(nf, io, layer.data_ptr()) == L.PC_ENOMEM                # (an arena-less call: the size)
    arena = torch.full((int(io.arena_needed),), 0x5A, dtype=torch.uint8, device="cuda")

    def io_of(smp=s):
        io, layer = nf._io(smp)
        io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
        return io, layer.data_ptr()

    io, lp = io_of()
    with L.precision("bf16"):
        rc = L.lib().pc_forward(nf.handle(), C.byref(io), C.c_void_p(lp), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.PC_ENOTSUP
    io, lp = io_of(); io.B, io.H, io.W = 32768, 256, 256
    assert _call(nf, io, lp) == L.PC_ENOTSUP                             # B * H * W = 2^31
    io, lp = io_of(); io.data = None
    assert _call(nf, io, lp) == L.PC_EINVAL
    io, lp = io_of(); io.data_kind, io.data2 = L.PC_DATA_SPLIT, None
    assert _call(nf, io, lp) == L.PC_EINVAL
    io, lp = io_of(); io.admin_mask = None
    assert _call(nf, io, lp) == L.PC_EINVAL
    io, lp = io_of(); io.census_idx = None
    assert _call(nf, io, lp) == L.PC_EINVAL
    io, lp = io_of()
    assert _call(nf, io, lp + 2) == L.PC_EINVAL                          # a misaligned layer
    io, lp = io_of(); io.arena_bytes = 4096
    assert _call(nf, io, lp) == L.PC_ENOMEM and io.arena_needed > 4096
    # a single-modality plan: the second stream's table is empty
    plan = L.PcStepPlan.from_buffer_copy(nf._native[1])
    for net in (plan.unet, plan.extractor):
        C.memset(C.addressof(net.s[1]), 0, C.sizeof(L.PcStepStream))
    h1 = L.lib().pc_step_create(C.byref(plan))
    assert h1
    io, lp = io_of()
    with L.precision("fp32"):
        rc = L.lib().pc_forward(h1, C.byref(io), C.c_void_p(lp), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.lib().pc_step_destroy(h1)
    assert rc == L.PC_ENOTSUP
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    io, lp = io_of()
    assert _call(nf, io, lp) == 0                                        # ... and the same call goes through untouched
    torch.cuda.synchronize()


def test_a_stream_under_capture_is_refused():
    from popcorn_amd import _lib as L
    m = _model()
    nf = _nf(m)
    io, _ = nf._io(_sample(2, 37, 53))
    assert _call(nf, io) == L.PC_ENOMEM
    arena = torch.full((int(io.arena_needed),), 0x5A, dtype=torch.uint8, device="cuda")
    io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
    h = nf.handle()
    x = torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with L.precision("fp32"), torch.cuda.graph(g):
        x += 1                                                           # (a kernel node: the capture is not empty)
        rc = L.lib().pc_forward(h, C.byref(io), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.PC_ENOTSUP
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())


def test_a_training_call_on_an_inference_plan_is_refused():
    from popcorn_amd import _lib as L
    tr = t_native._fresh(True)
    nf = _nf(tr.model)
    io, keep = t_layer._io(tr, t_native._batch(2, 37, 53))
    arena = torch.full((1 << 26,), 0x5A, dtype=torch.uint8, device="cuda")
    io.arena, io.arena_bytes = arena.data_ptr(), arena.numel()
    p0 = tr.flat_p.clone()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with L.precision("fp32"):
        for phases in (L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, L.PC_STEP_FWD, L.PC_STEP_UPD):
            assert L.lib().pc_train_step(nf.handle(), C.byref(io), phases, stream) == L.PC_EINVAL
            assert L.lib().pc_train_step_layer(nf.handle(), C.byref(io), None, phases, stream) == L.PC_EINVAL
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all()) and _same(tr.flat_p, p0)


# ---- with training -----------------------------------------------------------------------------------------------------------------------
def test_forwards_between_training_steps():
    smp = t_native._batch(2, 37, 53)
    fwd = {k: v for k, v in smp.items() if k != "y"}
    res = []
    for with_forward in (True, False):
        tr = t_native._fresh(True)
        m = tr.model
        torch.manual_seed(3)
        tr.step(dict(smp))
        if with_forward:
            after_one = _run(m, fwd, True)
            _assert_equal(after_one, _run(m, fwd, False), "after one step")
        torch.manual_seed(4)
        tr.step(dict(smp))
        torch.cuda.synchronize()
        assert tr.native_steps == 2
        res.append((tr.flat_p.clone(), tr.m.clone(), tr.v.clone(), tr.loss_out.clone()))
    for a, b in zip(*res):
        assert _same(a, b)


def test_forward_sees_new_weights_after_a_step_and_after_load_state_dict():
    smp = t_native._batch(2, 37, 53)
    fwd = {k: v for k, v in smp.items() if k != "y"}
    tr = t_native._fresh(True)
    m = tr.model
    before = _run(m, fwd, True)
    h0 = m._native_fwd.handle()
    torch.manual_seed(3)
    tr.step(dict(smp))
    after = _run(m, fwd, True)
    assert m._native_fwd.handle() == h0                                  # the same handle: pointers, not copies
    assert not _same(after["popdensemap"], before["popdensemap"])
    _assert_equal(after, _run(m, fwd, False), "after the step")
    other = _model(seed=77, fresh=True)
    m.load_state_dict(other.state_dict())
    loaded = _run(m, fwd, True)
    _assert_equal(loaded, _run(other, fwd, False), "after load_state_dict")
    assert not _same(loaded["popdensemap"], after["popdensemap"])


def test_data_parallel_phases_survive_a_forward_in_between():
    """FWD | (pc_forward on the model's own inference handle) | BWD | UPD under io.dp = 1 = the one-call step, bit for bit."""
    from popcorn_amd import _lib as L
    smp = t_native._batch(2, 37, 53)
    fwd = {k: v for k, v in smp.items() if k != "y"}
    tr1, tr2 = t_native._fresh(True), t_native._fresh(True)
    torch.manual_seed(3)
    tr1.step(dict(smp))
    torch.cuda.synchronize()
    assert tr1.native_steps == 1
    io, keep = t_layer._io(tr2, smp)
    io.dp = 1
    h = tr2._native_handle()
    with L.precision("fp32"), L.stream_scope():
        stream = L.stream_ptr()
        tr2._native_call(h, io, L.PC_STEP_FWD, stream)
    mid = _run(tr2.model, fwd, True)
    assert tr2.model._native_fwd.handle() != h
    with L.precision("fp32"), L.stream_scope():
        stream = L.stream_ptr()
        tr2._native_call(h, io, L.PC_STEP_BWD, stream)
        tr2._native_call(h, io, L.PC_STEP_UPD, stream)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(mid["popcount"]).all())
    for n in ("loss_out", "flat_g", "flat_p", "m", "v", "step_count"):
        assert _same(getattr(tr1, n), getattr(tr2, n)), n


# ---- consumers ---------------------------------------------------------------------------------------------------------------------------
RH, RW, PS, OV = 160, 192, 96, 16


def _members():
    return [_model(seed=40), _model(seed=41)]


def _evaluate(models, source, data, native, **kw):
    from popcorn_amd import eval as E
    for m in models:
        m.native_forward = native
    n0 = sum(m.native_forwards for m in models)
    num_ids = int(data.census_idx.max()) + 1
    try:
        maps = E.evaluate_raster(models, source, PS, OV, False, product=(p := E.ProductGrid(RH, RW, 8, 2, "cuda")),
                                 census=(c := E.CensusTable(RH, RW, [data.boundary], [num_ids], 2, "cuda")), **kw)
        torch.cuda.synchronize()
    finally:
        for m in models:
            m.native_forward = False
    return maps, p, c, sum(m.native_forwards for m in models) - n0


def _assert_same_evaluation(a, b):
    for x, y in zip(a[0], b[0]):
        assert FP.bit_equal(x, y)
    assert bool(torch.isfinite(a[0][0]).all()) and float(a[0][0].abs().sum()) > 0
    assert FP.bit_equal(a[1].mean, b[1].mean) and FP.bit_equal(a[1].std, b[1].std) and FP.bit_equal(a[1].cells, b[1].cells)
    assert torch.equal(a[2].table, b[2].table) and FP.bit_equal(a[2].mean, b[2].mean) and FP.bit_equal(a[2].std, b[2].std)


def test_evaluate_raster_two_members_equal_maps_product_and_census():
    from popcorn_amd import eval as E
    from popcorn_amd.data.dataset import SyntheticTestRaster
    data = SyntheticTestRaster(RH, RW, seasons=1, n_regions=16, seed=1610, device="cuda")
    models = _members()
    nwin = E.get_patch_indices(RH, RW, PS, OV, False).shape[0]
    off = _evaluate(models, data.raster, data, False)
    on = _evaluate(models, data.raster, data, True)
    assert off[3] == 0 and on[3] == 2 * nwin                             # member 1 reuses member 0's score as its layer
    _assert_same_evaluation(on, off)


def test_evaluate_raster_through_resident_windows():
    from popcorn_amd import eval as E
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import ResidentRegion, ResidentWindows
    data = SyntheticTestRaster(RH, RW, seasons=1, n_regions=16, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.05)
    feed = ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=True), PS, OV, fourseasons=False)
    models = _members()
    off = _evaluate(models, feed, data, False)
    on = _evaluate(models, feed, data, True)
    assert off[3] == 0 and on[3] == 2 * len(feed.idx)
    _assert_same_evaluation(on, off)


TRAIN = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 -wb 2 -lt 1 --max_steps 2 --save-model no -wv "
         "--val_every_n_epochs 1 --synthetic_regions 8 --synthetic_val_regions 4 --test_raster_hw 160 192 --test_patchsize 96 --test_overlap 16")


def test_validate_weak_gives_the_same_metrics(tmp_path):
    from popcorn_amd import cli
    t = cli.Trainer(cli.train_parser().parse_args(TRAIN.split() + ["--save_dir", str(tmp_path)]))
    off = dict(t.validate_weak())
    t.model.native_forward = True
    on = dict(t.validate_weak())
    assert t.model.native_forwards == 4 and on == off and len(on) > 2
    assert all(v == v for v in on.values())


def test_run_train_and_run_eval_print_a_non_zero_count(tmp_path, capsys):
    from popcorn_amd import cli
    t = cli.run_train(TRAIN.split() + ["--save_dir", str(tmp_path), "--native_forward"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("native forwards:")]
    assert len(lines) == 1 and int(lines[0].split(":")[1]) == t.model.native_forwards > 4      # validation items + test windows
    base = ("-S2 -NIR -S1 -occmodel -senbuilds -pret --biasinit 0.9407 --raster_hw 160 192 --patchsize 96 --overlap 16 --ensemble 2").split()
    off = cli.run_eval(base)
    capsys.readouterr()
    on = cli.run_eval(base + ["--native_forward"])
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1])["native_forwards"] == on["native_forwards"] > 0
    assert [ln for ln in out if ln.startswith("native forwards:")] == [f"native forwards: {on['native_forwards']}"]
    a, b = dict(off), dict(on)
    a.pop("seconds"), b.pop("seconds"), b.pop("native_forwards")
    assert a == b and len(a) > 4
    # what the executor declines is accepted and simply never takes it
    res = cli.run_eval(base + ["--native_forward", "--precision", "bf16"])
    assert res["native_forwards"] == 0
