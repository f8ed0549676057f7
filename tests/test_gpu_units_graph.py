"""The device-N multi-unit step (``FusedTrainStep(device_units=True)``) against the plain eager multi-unit step, bit for bit: replayed
from ONE captured graph while N, the id lists and y change from step to step, and eagerly.  Both trainers start from the same model state
and see the same seed in front of each step (the same selection grid).

(2, 32, 32) with K = 3: separate padded domains of the two networks; (2, 100, 100) with K = 4: the shared 128 x 128 domain.  census_n goes
[3, 2] -> [1, 3] -> [3, 3]: ragged, a one-unit row, then the full capacity of K = 3 (no tail at all)."""
import pytest
import torch

from tests import units_oracle as U

pytestmark = pytest.mark.gpu

# the listed units of the two crops, step by step: counts [3, 2], [1, 3], [3, 3]; unsorted, different ids every step
STEP_UNITS = [((12, 3, 7), (9, 5)), ((4,), (8, 2, 6)), ((7, 1, 3), (11, 5, 2))]
GEOMS = [(32, 32, 3), (100, 100, 4)]


def _trainer(**kw):
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    return FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, gradient_clip=0.01, **kw)


def _samples(H, W, K):
    out = []
    for it, units in enumerate(STEP_UNITS):
        inputs, y = U.make_case(B=2, H=H, W=W, units=units, channels=6, seed=11 + it, pad_to=K)
        s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
        s["y"] = y.cuda()
        assert tuple(s["census_idx"].shape) == (2, K) and s["census_n"] == [len(u) for u in units]
        out.append(s)
    return out


def _run(tr, samples):
    out = []
    for it, s in enumerate(samples):
        torch.manual_seed(50 + it)
        loss = tr.step(dict(s))
        torch.cuda.synchronize()
        out.append({"loss": loss.clone(), "flat_p": tr.flat_p.clone(), "popcount": tr.last["popcount"].clone(),
                    "unit_n": tr.last["unit_n"].clone() if "unit_n" in tr.last else None})
    return out


_eager = {}


def _reference(H, W, K):
    """three steps of the plain eager multi-unit trainer (the parent commit's only form), once per geometry"""
    if (H, W, K) not in _eager:
        tr = _trainer()
        _eager[H, W, K] = _run(tr, _samples(H, W, K))
        assert tr.device_unit_steps == 0 and tr.captures == 0
    return _eager[H, W, K]


def _assert_equal_steps(got, want, samples, K):
    for it, (a, b, s) in enumerate(zip(got, want, samples)):
        N = sum(s["census_n"])
        assert torch.equal(a["flat_p"], b["flat_p"]), (it, (a["flat_p"] - b["flat_p"]).abs().max().item())
        assert torch.equal(a["loss"], b["loss"]), (it, a["loss"].tolist(), b["loss"].tolist())
        assert tuple(a["popcount"].shape) == (2 * K,) and tuple(b["popcount"].shape) == (N,)
        assert torch.equal(a["popcount"][:N], b["popcount"]), it
        assert not bool(a["popcount"][N:].any()), it                               # the tail is exactly 0
        assert a["unit_n"].dtype == torch.int32 and a["unit_n"].tolist() == [N]
    assert bool(torch.isfinite(got[-1]["loss"]).all()) and float(got[-1]["popcount"].abs().max()) > 0


@pytest.mark.parametrize("H,W,K", GEOMS)
def test_one_captured_graph_serves_every_n(H, W, K):
    samples = _samples(H, W, K)
    tr = _trainer(device_units=True, use_graph=True)
    got = _run(tr, samples)
    _assert_equal_steps(got, _reference(H, W, K), samples, K)
    assert tr.captures == 1 and tr.device_unit_steps == 3                          # exactly one capture took place
    assert tr.native_unit_steps == 0 and tr.native_steps == 0


@pytest.mark.parametrize("H,W,K", GEOMS)
def test_eager_device_n_step_equals_the_host_n_step(H, W, K):
    samples = _samples(H, W, K)
    tr = _trainer(device_units=True)
    got = _run(tr, samples)
    _assert_equal_steps(got, _reference(H, W, K), samples, K)
    assert tr.captures == 0 and tr.device_unit_steps == 3 and tr.native_unit_steps == 0


def test_static_set_filled_in_place():
    """A loader writes its batch into ``static_buffers(units=K)`` -- the counts too -- and passes the very dict: no copies, one capture."""
    H, W, K = 32, 32, 3
    samples = _samples(H, W, K)
    tr = _trainer(device_units=True, use_graph=True)
    buf = tr.static_buffers(2, H, W, units=K)
    assert tuple(buf["census_idx"].shape) == (2, K) and tuple(buf["y"].shape) == (2, K) and buf["census_n"].dtype == torch.int32
    got = []
    for it, s in enumerate(samples):
        for k in ("input", "admin_mask", "census_idx", "y"):
            buf[k].copy_(s[k])
        buf["census_n"].copy_(torch.tensor(s["census_n"], dtype=torch.int32))
        torch.manual_seed(50 + it)
        loss = tr.step(buf)
        torch.cuda.synchronize()
        got.append({"loss": loss.clone(), "flat_p": tr.flat_p.clone(), "popcount": tr.last["popcount"].clone(),
                    "unit_n": tr.last["unit_n"].clone()})
    _assert_equal_steps(got, _reference(H, W, K), samples, K)
    assert tr.captures == 1


def test_run_train_device_units_with_fixed_hw(tmp_path):
    """run_train.py --units_per_crop 4 --device_units --fixed_hw 64 64: ``collate_units`` output as it comes (ragged rows, K = the batch's
    maximum, padded on to 4 by the trainer), every step a replay of ONE captured graph, finite losses."""
    from popcorn_amd.cli import run_train
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 --synthetic_regions 16 -wb 2 -lt 2 "
            f"--units_per_crop 4 --device_units --fixed_hw 64 64 --max_steps 4 --save-model no --save_dir {tmp_path}").split()
    t = run_train(argv)
    assert t.fused.use_graph and t.fused.device_units
    assert t.info["iter"] == 4 and t.fused.device_unit_steps == 4 and t.fused.captures == 1
    assert t.fused.native_steps == 0 and t.fused.native_unit_steps == 0
    assert tuple(t.fused.last["popcount"].shape) == (8,)                           # the capacity B K
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
    pr = torch.cat([p for p, _ in t._r2buf])
    yy = torch.cat([y_ for _, y_ in t._r2buf])
    assert pr.shape == yy.shape and pr.dim() == 1                                  # the rolling R2 buffer holds the flat N, not the capacity


def test_beyond_the_caps_a_graph_raises_and_an_eager_step_falls_back():
    """K = 1025: ValueError at capture (a graph has no fallback), from ``static_buffers`` too; eager in one process, the host-N step."""
    inputs, y = U.make_case(B=2, H=32, W=32, units=((3, 7), (5,)), channels=6, seed=11, pad_to=1025)
    s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    s["y"] = y.cuda()
    trg = _trainer(device_units=True, use_graph=True)
    with pytest.raises(ValueError):
        trg.step(dict(s))
    with pytest.raises(ValueError):
        trg.static_buffers(2, 32, 32, units=1025)
    assert trg.captures == 0
    res = []
    for kw in ({"device_units": True}, {}):
        tr = _trainer(**kw)
        torch.manual_seed(50)
        loss = tr.step(dict(s))
        torch.cuda.synchronize()
        res.append((loss.clone(), tr.flat_p.clone(), tr.last["popcount"].clone()))
        assert tr.device_unit_steps == 0
    assert all(torch.equal(a, b) for a, b in zip(*res)) and tuple(res[0][2].shape) == (3,)


def test_switch_off_keeps_the_refusal_and_bad_counts_raise_on_the_host():
    s = _samples(32, 32, 3)[0]
    with pytest.raises(ValueError):
        _trainer(use_graph=True).step(dict(s))
    tr = _trainer(device_units=True, use_graph=True)
    p0 = tr.flat_p.clone()
    for bad in ([0, 2], [3, 4], [3]):
        with pytest.raises(ValueError):
            tr.step({**s, "census_n": bad})
    assert tr.captures == 0 and torch.equal(tr.flat_p, p0)                         # nothing was enqueued
    # a 1-D census_idx takes the one-unit path whatever the switch says
    rep, y_flat, _ = U.replicate({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in s.items() if k != "y"}, s["y"].cpu())
    one = {k: v.cuda() for k, v in rep.items()}
    one["y"] = y_flat.cuda()
    tr2 = _trainer(device_units=True)
    tr2.step(one)
    assert tr2.native_steps == 1 and tr2.device_unit_steps == 0
