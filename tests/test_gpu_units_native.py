"""Multi-unit census supervision through the native step executor (pc_train_step_units) and its two kernels (csrc/units.hip):

  * pc_unit_layout against ``ops.unit_layout`` (torch.sort + gathers), exact;
  * pc_unit_popcount_loss against ``ops.unit_popcount`` + ``ops.loss_fwd_bwd``, bit for bit;
  * the executor's multi-unit step against the per-launch engine's (``native_units=False``: the path of tests/test_gpu_units.py), bit for
    bit over two steps -- parameters, gradients, Adam state, outputs;
  * the routing: opt-in, fallbacks, counters, and that the one-unit executor issues the launches it always issued.

Shapes: K = 1 (no sort round at all), K = 5 ragged with junk in the padding, K = 300 (not a power of two, above the 256 LDS bins of the
sums), K = 1024 (the cap), K = 1025 (declined); N = 1, 257 (crosses the 256-thread stride of the one-block tail) and 1000."""
import ctypes as C

import pytest
import torch

from tests import units_oracle as U

pytestmark = pytest.mark.gpu

I64_MAX = torch.iinfo(torch.int64).max
BIG = (1 << 24) + 2                      # an id above 2^24 that fp32 still holds exactly


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- pc_unit_layout ------------------------------------------------------------------------------------------------------------------
def _layout_case(name):
    """(census_idx (B, K) int64, y (B, K) fp32, census_n) on the CPU."""
    g = torch.Generator().manual_seed(5)
    if name == "1x1":
        cidx, cn = torch.tensor([[42]]), [1]
    elif name == "3x5_junk_padding":
        # slots past census_n hold -1, a duplicate of a valid id, and INT64_MAX: ignored whatever they hold
        cidx = torch.tensor([[9, 3, BIG, 7, 5], [8, 8, -1, I64_MAX, 8], [12, 4, 6, 4, I64_MAX]])
        cn = [5, 1, 3]
    elif name == "2x300_ragged":
        cidx = torch.stack([1000 + torch.randperm(300, generator=g), 5000 + 3 * torch.randperm(300, generator=g)])
        cidx[1, 123:] = -1
        cn = [300, 123]
    elif name == "1x1024_cap":
        cidx, cn = (7 + 5 * torch.randperm(1024, generator=g)).reshape(1, 1024), [1024]
    else:
        raise KeyError(name)
    cidx = cidx.to(torch.int64)
    return cidx, torch.rand(cidx.shape, generator=g) * 300.0, cn


@pytest.mark.parametrize("name", ["1x1", "3x5_junk_padding", "2x300_ragged", "1x1024_cap"])
def test_unit_layout_equals_the_torch_plumbing(name):
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    cidx, y, cn = _layout_case(name)
    cidx, y = cidx.cuda(), y.cuda()
    ref = ops.unit_layout(cidx, cn)
    N = ref["N"]
    need = L.lib().pc_unit_ws_bytes(N)
    assert need >= 20 * N and need % 16 == 0
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")          # 64 guard bytes behind the workspace
    lay = ops.unit_layout_device(cidx, y, cn, ws=ws)
    assert lay["N"] == N == sum(cn) and lay["counts"] == cn
    assert lay["units"].dtype == torch.int64 and torch.equal(lay["units"], ref["units"])
    assert lay["unit_off"].dtype == torch.int32 and torch.equal(lay["unit_off"], ref["unit_off"])
    assert torch.equal(_bits(lay["y_sorted"]), _bits(y.reshape(-1)[ref["to_sorted"]]))
    # dest[n] = the (b, k) position of sorted slot n: its inverse is to_caller
    dest = lay["dest"].long()
    assert lay["dest"].dtype == torch.int32 and sorted(dest.tolist()) == list(range(N))
    to_caller = torch.empty(N, dtype=torch.int64, device="cuda")
    to_caller[dest] = torch.arange(N, device="cuda")
    assert torch.equal(to_caller, ref["to_caller"])
    # the workspace: zero over exactly 20 N bytes, everything behind untouched
    assert int(ws[:20 * N].count_nonzero()) == 0
    assert bool((ws[20 * N:] == 0xFF).all())
    if name == "3x5_junk_padding":
        assert lay["units"].tolist() == [3, 5, 7, 9, BIG, 8, 4, 6, 12]


def test_unit_layout_declines_k_above_the_cap():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    B, K = 1, L.PC_UNIT_LAYOUT_MAX_K + 1
    cidx = torch.arange(K, dtype=torch.int64, device="cuda").reshape(B, K)
    y = torch.zeros(B, K, device="cuda")
    out = [torch.full((K + 8,), -7, dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.float32, torch.int32)]
    rc = L.lib().pc_unit_layout(L.ptr(cidx), L.ptr(y), (C.c_int32 * 1)(K), B, K, *[L.ptr(t) for t in out], None, L.stream_ptr())
    assert rc == L.PC_ENOTSUP
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out)                                # nothing was launched
    with pytest.raises(L.PopcornHipError):
        ops.unit_layout_device(cidx, y)
    assert ops.unit_layout(cidx)["N"] == K                                        # the torch plumbing has no cap


# ---- pc_unit_popcount_loss -----------------------------------------------------------------------------------------------------------
LAM4, SREG, LAM_WEAK = [0.5, 1.0, 0.25, 0.125], 0.01, 100.0
TAIL_CASES = [(1, (1, 37, 53)), (257, (1, 37, 53)), (257, (2, 64, 64)), (1000, (2, 64, 64)), (1000, (1, 37, 53))]


def _tail_case(N, shape):
    """cidx, y, census_n with sum = N, a slot map in the kernels' numbering (a fifth of the pixels unowned) and a density map."""
    B, H, W = shape
    g = torch.Generator().manual_seed(N * 7 + H)
    cn = [N] if B == 1 else [N - N // 4, N // 4]
    K = max(cn)
    cidx = torch.full((B, K), -1, dtype=torch.int64)
    for b, c in enumerate(cn):
        cidx[b, :c] = 100 + torch.randperm(3 * K, generator=g)[:c]
    y = torch.rand(B, K, generator=g) * 300.0
    slot = torch.empty(B, H, W, dtype=torch.int32)
    off = 0
    for b, c in enumerate(cn):
        s = torch.randint(0, c, (H, W), generator=g) + off
        s[torch.rand(H, W, generator=g) < 0.2] = -1
        slot[b] = s.to(torch.int32)
        off += c
    pd = torch.rand(B, H, W, generator=g) * 10.0 ** torch.randint(-4, 2, (B, H, W), generator=g).float()
    pd[torch.rand(B, H, W, generator=g) < 0.25] = 0.0
    return cidx.cuda(), y.cuda(), cn, slot.cuda(), pd.cuda()


def _tail_outputs():
    return (torch.full((2,), -1.0, device="cuda"), torch.full((1,), -1.0, device="cuda"))


def _reference_tail(cidx, y, cn, slot, pd, stats):
    """ops.unit_layout + ops.unit_popcount + ops.loss_fwd_bwd: the per-launch trainer's tail."""
    from popcorn_amd import ops
    ref = ops.unit_layout(cidx, cn)
    N = ref["N"]
    pc = ops.unit_popcount(pd, slot, N, ref["unit_off"])
    loss, gsc = _tail_outputs()
    g = torch.empty(N, device="cuda")
    ops.loss_fwd_bwd(pc, y.reshape(-1)[ref["to_sorted"]], stats, LAM4, SREG, LAM_WEAK, 1.0 / N, loss, g, gsc)
    return pc, pc.index_select(0, ref["to_caller"]), loss, g, gsc


def _fused_tail(cidx, y, cn, slot, pd, stats, ws=None):
    from popcorn_amd import ops
    lay = ops.unit_layout_device(cidx, y, cn, ws=ws)
    loss, gsc = _tail_outputs()
    g = torch.empty(lay["N"], device="cuda")
    pcs, pcc = ops.unit_popcount_loss(pd, slot, lay, stats, LAM4, SREG, LAM_WEAK, loss, g, gsc)
    return pcs, pcc, loss, g, gsc


@pytest.mark.parametrize("N,shape", TAIL_CASES)
def test_unit_popcount_loss_is_bitwise_the_two_calls(N, shape):
    from popcorn_amd import _lib as L
    cidx, y, cn, slot, pd = _tail_case(N, shape)
    stats = torch.tensor([float((slot >= 0).sum()), 1234.5], dtype=torch.float64, device="cuda")
    want = _reference_tail(cidx, y, cn, slot, pd, stats)
    ws = torch.full((L.lib().pc_unit_ws_bytes(N),), 0xFF, dtype=torch.uint8, device="cuda")
    got = _fused_tail(cidx, y, cn, slot, pd, stats, ws)
    names = ("popcount sorted", "popcount caller", "loss_out", "g_popcount", "g_scale_const")
    for n, a, b in zip(names, got, want):
        assert torch.equal(_bits(a), _bits(b)), n
    assert bool(torch.isfinite(got[2]).all()) and float(got[0].max()) > 0
    # twice in a row on the same workspace: the layout launch re-zeroes it
    again = _fused_tail(cidx, y, cn, slot, pd, stats, ws)
    for n, a, b in zip(names, again, got):
        assert torch.equal(_bits(a), _bits(b)), ("second call", n)
    # an Inf term makes ITS unit NaN, bitwise as the two calls do; the other units keep their bits
    tgt = int(slot[slot >= 0][0])
    pd2 = pd.clone()
    pd2.view(-1)[int((slot.view(-1) == tgt).nonzero()[0])] = float("inf")
    bad = _fused_tail(cidx, y, cn, slot, pd2, stats, ws)
    want_bad = _reference_tail(cidx, y, cn, slot, pd2, stats)
    assert bool(torch.isnan(bad[0][tgt]))
    for n, a, b in zip(names, bad, want_bad):
        assert torch.equal(_bits(a), _bits(b)), ("inf", n)
    keep = torch.arange(N, device="cuda") != tgt
    assert torch.equal(_bits(bad[0][keep]), _bits(got[0][keep]))


# ---- the step ------------------------------------------------------------------------------------------------------------------------
REGIMES = {"all": (False, False), "limit1": (True, False), "limit2": (True, True)}


def _trainer(native_units, given=False):
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=not given).cuda()
    return FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, native_units=native_units)


def _cells_case(H=131, W=77, cell=5, listed=300, seed=2):
    """(1, 131, 77): a 5 x 5 tiling of 27 x 16 cells with ids 1000 + cell, `listed` of them listed in shuffled order, the rest unlisted
    neighbours; the collate's -1 frame at the bottom / right."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    ncol = (W + cell - 1) // cell
    admin = (1000 + (yy // cell) * ncol + xx // cell).float()
    admin[H - 3:, :] = -1.0
    admin[:, W - 2:] = -1.0
    present = admin[admin >= 0].unique().long()
    ids = present[torch.randperm(present.numel(), generator=g)[:listed]]
    return {"input": torch.randn(1, 6, H, W, generator=g), "admin_mask": admin[None], "census_idx": ids[None].contiguous(),
            "census_n": [listed]}, (torch.rand(1, listed, generator=g) * 50.0)


def _geometry(name):
    if name == "2x32x32":
        return U.make_case(B=2, H=32, W=32, units=((3, 7), (5,)), channels=6, seed=11)
    if name == "2x100x100":
        return U.make_case(B=2, H=100, W=100, units=((12, 3, 7), (9, 5)), channels=6, seed=11)
    if name == "3x96x160":
        return U.make_case(B=3, H=96, W=160, units=((12, 3, 7), (9, 5), (4,)), channels=6, seed=11)
    if name == "1x131x77":
        return _cells_case()
    raise KeyError(name)


def _sample(name, form="input"):
    """The multi-unit batch of a geometry on the device; form: the normalised input, or the same units on a raw / split tile."""
    inputs, y = _geometry(name)
    s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
    s["y"] = y.cuda()
    if form != "input":
        from popcorn_amd.data import stats
        from popcorn_amd.data.synthetic import make_raw_batch
        B, _, H, W = s.pop("input").shape
        raw = make_raw_batch(B, H, W, seed=H * 1000 + W)["raw"].cuda()
        if form == "raw":
            s["raw"] = raw
        else:
            sel = raw[:, list(stats.BAND6)]
            s["raw_s2"] = sel[:, :4].round().clamp(0, 65535).to(torch.int32).cpu().to(torch.uint16).cuda().contiguous()
            s["raw_s1"] = sel[:, 4:6].contiguous()
    return s


def _two_steps(tr, smp, flags=(False, False)):
    out = []
    for it in range(2):
        torch.manual_seed(3 + it)
        loss = tr.step(dict(smp), encoder_no_grad=flags[0], unet_no_grad=flags[1])
        torch.cuda.synchronize()
        out.append({"loss": loss.clone(), "flat_g": tr.flat_g.clone(), "flat_p": tr.flat_p.clone(), "m": tr.m.clone(), "v": tr.v.clone(),
                    "step": tr.step_count.clone(), "popcount": tr.last["popcount"].clone(), "slot": tr.last["slot"].clone(),
                    "mask": tr.last["mask"].clone(), "popdensemap": tr.last["popdensemap"].clone(),
                    "scale_map": tr.last["scale_map"].clone()})
    return out


def _assert_same_steps(got, want):
    for it, (a, b) in enumerate(zip(got, want)):
        sel = b["mask"].bool()
        for n in a:
            if n in ("popdensemap", "scale_map"):
                assert torch.equal(a[n][sel], b[n][sel]), (n, it)
            else:
                assert a[n].shape == b[n].shape and torch.equal(a[n], b[n]), (n, it, (a[n].float() - b[n].float()).abs().max().item())


_per_launch = {}


def _per_launch_steps(name, regime="all", form="input"):
    """Two steps of a trainer that never opted in (the parent's multi-unit path), once per case."""
    key = (name, regime, form)
    if key not in _per_launch:
        tr = _trainer(False)
        _per_launch[key] = _two_steps(tr, _sample(name, form), REGIMES[regime])
        assert tr.native_unit_steps == 0 and tr.native_steps == 0
    return _per_launch[key]


STEP_CASES = [("2x32x32", "all", "input"), ("2x100x100", "all", "input"), ("2x100x100", "limit1", "input"), ("2x100x100", "limit2", "input"),
              ("3x96x160", "all", "input"), ("1x131x77", "all", "input"), ("2x100x100", "all", "raw"), ("2x100x100", "all", "split")]


@pytest.mark.parametrize("name,regime,form", STEP_CASES, ids=["-".join(c) for c in STEP_CASES])
def test_native_units_step_is_bit_equal_to_the_per_launch_step(name, regime, form):
    smp = _sample(name, form)
    tr = _trainer(True)
    got = _two_steps(tr, smp, REGIMES[regime])
    assert tr.native_unit_steps == 2              # (0 without the feature: the executor declined every multi-unit sample)
    assert tr.native_steps == 0                   # ... which counts one-unit executor steps only
    N = sum(smp["census_n"])
    assert tuple(got[0]["popcount"].shape) == (N,) and got[0]["slot"].dtype == torch.int32
    assert tuple(tr.last["building_counts"].shape) == (smp["admin_mask"].shape[0], 1, *smp["admin_mask"].shape[1:])
    assert bool(torch.isfinite(got[1]["loss"]).all()) and int(got[0]["mask"].sum()) > 0
    _assert_same_steps(got, _per_launch_steps(name, regime, form))


# ---- routing -------------------------------------------------------------------------------------------------------------------------
def test_default_keeps_the_per_launch_engine():
    tr = _trainer(False)
    assert tr.native_units is False
    tr.step(_sample("2x32x32"))
    assert tr.native_unit_steps == 0 and tr.native_steps == 0


@pytest.mark.parametrize("why", ["given_buildings", "k_above_cap"])
def test_opt_in_falls_back_where_the_executor_declines(why):
    """A given building layer (declined by ``_native_ok``) and K = 1025 (declined by the entry: PC_ENOTSUP, nothing enqueued): the
    per-launch engine within the same step, bit-equal to a trainer that never opted in, and not counted."""
    given = why == "given_buildings"
    if given:
        smp = _sample("2x100x100")
        smp["building_counts"] = torch.rand(2, 1, 100, 100, generator=torch.Generator().manual_seed(4)).cuda()
    else:
        inputs, y = U.make_case(B=2, H=32, W=32, units=((3, 7), (5,)), channels=6, seed=11, pad_to=1025)
        smp = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inputs.items()}
        smp["y"] = y.cuda()
        assert tuple(smp["census_idx"].shape) == tuple(smp["y"].shape) == (2, 1025) and smp["census_n"] == [2, 1]
    res = []
    for native_units in (True, False):
        tr = _trainer(native_units, given=given)
        res.append(_two_steps(tr, smp))
        assert tr.native_unit_steps == 0 and tr.native_steps == 0
    _assert_same_steps(*res)


def test_one_unit_sample_after_a_multi_unit_one_counts_in_native_steps():
    inputs, y = _geometry("2x100x100")
    rep, y_flat, _ = U.replicate(inputs, y)
    tr = _trainer(True)
    tr.step(_sample("2x100x100"))
    one = {k: v.cuda() for k, v in rep.items()}
    one["y"] = y_flat.cuda()
    tr.step(one)
    tr.step(_sample("2x100x100"))
    assert (tr.native_unit_steps, tr.native_steps) == (2, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.loss_out).all()) and tuple(tr.last["popcount"].shape) == (5,)


# launches of one pc_train_step call, FWD | BWD | UPD, 2 x 100 x 100, regime `all`, host selection flags -- measured on the parent commit
# of this feature (io.launches of the same batch and call, parent's library): 37
ONE_UNIT_LAUNCHES_2x100x100 = 37


def test_one_unit_executor_issues_the_launches_it_issued_before():
    from popcorn_amd import _lib as L
    inputs, y = _geometry("2x100x100")
    one = {"input": inputs["input"].cuda(), "admin_mask": inputs["admin_mask"].cuda(), "census_idx": inputs["census_idx"][:, 0].cuda().contiguous(),
           "y": y[:, 0].cuda().contiguous()}            # the first listed unit of each crop
    tr = _trainer(True)
    torch.manual_seed(3)
    sel = tr._draw_selection(100, 100)
    with L.precision("fp32"):
        io = tr._native_io(one, sel, False, False)
        tr._native_call(tr._native_handle(), io, L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, L.stream_ptr())
    torch.cuda.synchronize()
    print(f"\n[one-unit pc_train_step 2x100x100] launches {io.launches}")
    assert io.launches == ONE_UNIT_LAUNCHES_2x100x100
    # and the multi-unit step of the same crop: the count the design document states
    smp = _sample("2x100x100")
    smp = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in smp.items()}
    with L.precision("fp32"):
        io2, units = tr._native_io(smp, sel, False, False)
        rc = tr._native_call(tr._native_handle(), io2, L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD, L.stream_ptr(), units)
    torch.cuda.synchronize()
    print(f"[multi-unit pc_train_step_units 2x100x100] launches {io2.launches}")
    assert rc == 0 and io2.launches == io.launches + 5


def test_run_train_native_units(tmp_path):
    """run_train.py --units_per_crop 4 --native_units --max_steps 4: every step through the executor, finite losses."""
    from popcorn_amd.cli import run_train
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 --synthetic_regions 16 -wb 2 -lt 2 "
            f"--units_per_crop 4 --native_units --max_steps 4 --synthetic_hw_range 48 80 --save-model no --save_dir {tmp_path}").split()
    t = run_train(argv)
    assert t.info["iter"] == 4 and t.fused.native_unit_steps == 4 and t.fused.native_steps == 0
    assert tuple(t.fused.last["popcount"].shape)[0] >= 2
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all())
