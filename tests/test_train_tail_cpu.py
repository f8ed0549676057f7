"""The references and bars of tests/train_tail_oracle.py, checked without a GPU: the float64 references against torch (clip_grad_norm_ +
optim.Adam, autograd through the oracle's get_loss), the fp32 emulations of the kernels against the references (they must sit within HALF
of every bar: the bars are attainable by fp32 arithmetic), and the bars' power to tell wrong Adam formulas from the right one."""
import numpy as np
import pytest
import torch

from tests import train_tail_oracle as TO

U = TO.U
HYP = TO.HYP


# ---- a. the float64 reference against torch -------------------------------------------------------------------------------------------
# flat layout of the project's trainer in miniature: encoder | decoder | head (decayed part) | head.6.weight | head.6.bias; groups 0 / 1 / 2;
# the last two tensors take no weight decay (run_train.py:82-90)
SIZES = (1000, 800, 300, 64, 3)
SEGMENTS = [(1000, 0), (1800, 1), (2167, 2)]
N_DECAY = 2100
REGIMES = [{0, 1, 2}, {1, 2}, {2}, {0, 1, 2}, {1, 2}, {2}, {2}, {0, 1, 2}, {1, 2}, {0, 1, 2}, {2}, {1, 2}]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_adam_ref_equals_torch_adam_with_frozen_groups():
    """adam_clip_ref (nominal double hyperparameters) against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on float64 parameters: three
    groups, the project's decay split, 12 steps in which the encoder or the whole U-Net has ``grad = None`` (as in
    test_fused_step_skips_frozen_groups_like_torch_adam); parameters, exp_avg, exp_avg_sq and the per-parameter steps to 1e-12 relative."""
    rng = np.random.default_rng(1)
    n = sum(SIZES)
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    grp_of_tensor = (0, 1, 2, 2, 2)
    p = rng.normal(size=n) * 0.1
    params = [torch.tensor(p[offs[i]:offs[i + 1]].copy(), dtype=torch.float64, requires_grad=True) for i in range(5)]
    opt = torch.optim.Adam([{"params": params[:3], "weight_decay": HYP["wd"]}, {"params": params[3:], "weight_decay": 0.0}],
                           lr=HYP["lr"], betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"])
    m, v, steps = np.zeros(n), np.zeros(n), np.zeros(4, dtype=np.int64)
    for it, active in enumerate(REGIMES):
        g = TO.adam_grad(rng, n, below=HYP["max_norm"] if it % 5 == 4 else None).astype(np.float64)
        for i, t in enumerate(params):
            if grp_of_tensor[i] in active:
                t.grad = torch.tensor(g[offs[i]:offs[i + 1]].copy(), dtype=torch.float64)
            else:
                t.grad = None
                g[offs[i]:offs[i + 1]] = 0.0            # the trainer's contract: an inactive group's gradient is zero in the flat buffer
        total = torch.nn.utils.clip_grad_norm_(params, HYP["max_norm"])
        opt.step()
        p, m, v, steps, norm = TO.adam_clip_ref(p, g, m, v, steps, n_decay=N_DECAY, segments=SEGMENTS, active=active, f32_hyper=False, **HYP)
        assert abs(norm - total.item()) <= 1e-12 * norm
    assert steps.tolist() == [sum(0 in r for r in REGIMES), sum(1 in r for r in REGIMES), len(REGIMES), 0]
    st = opt.state_dict()["state"]
    for i, t in enumerate(params):
        sl = slice(offs[i], offs[i + 1])
        assert _rel(t.detach().numpy(), p[sl]) <= 1e-12
        assert _rel(st[i]["exp_avg"].numpy(), m[sl]) <= 1e-12 and _rel(st[i]["exp_avg_sq"].numpy(), v[sl]) <= 1e-12
        assert int(st[i]["step"]) == steps[grp_of_tensor[i]]


def test_adam_ref_equals_the_oracle_train_step():
    """All groups active: adam_clip_ref against oracle.popcorn_oracle.clip_grad_norm + adam_step (float64), 12 steps."""
    from oracle import popcorn_oracle as O
    rng = np.random.default_rng(2)
    names = ["enc.w", "dec.w", "head.0.weight", "head.6.weight", "head.6.bias"]
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    n = sum(SIZES)
    p = rng.normal(size=n) * 0.1
    params = {k: torch.tensor(p[offs[i]:offs[i + 1]].copy()) for i, k in enumerate(names)}
    state = {}
    m, v, steps = np.zeros(n), np.zeros(n), np.zeros(1, dtype=np.int64)
    for it in range(12):
        g = TO.adam_grad(rng, n, below=HYP["max_norm"] if it % 5 == 4 else None).astype(np.float64)
        total, clipped = O.clip_grad_norm({k: torch.tensor(g[offs[i]:offs[i + 1]].copy()) for i, k in enumerate(names)}, HYP["max_norm"])
        params = O.adam_step(params, clipped, state, lr=HYP["lr"], betas=(HYP["beta1"], HYP["beta2"]), eps=HYP["eps"], weight_decay=HYP["wd"])
        p, m, v, steps, norm = TO.adam_clip_ref(p, g, m, v, steps, n_decay=N_DECAY, f32_hyper=False, **HYP)
        assert abs(norm - total.item()) <= 1e-12 * norm
    assert steps.tolist() == [12]
    for i, k in enumerate(names):
        sl = slice(offs[i], offs[i + 1])
        t, em, ev = state[k]
        assert t == 12
        assert _rel(params[k].numpy(), p[sl]) <= 1e-12 and _rel(em.numpy(), m[sl]) <= 1e-12 and _rel(ev.numpy(), v[sl]) <= 1e-12


# ---- b. the fp32 emulation against the reference, c. discrimination ----------------------------------------------------------------------
TRAJ_N, TRAJ_STEPS, TRAJ_DECAY = TO.TRAJ_N, TO.TRAJ_STEPS, TO.TRAJ_DECAY


def trajectory(seed=3):
    """The 40-step recipe shared with the GPU test: yields (t, p, g, m, v) -- fp32 state BEFORE step t (t = 1 ..), the emulation's own, and
    the gradient of the step; every fifth gradient has its norm under max_norm."""
    rng = np.random.default_rng(seed)
    p, _, m, v = TO.adam_inputs(rng, TRAJ_N)
    steps = np.zeros(1, dtype=np.int64)
    for t in range(1, TRAJ_STEPS + 1):
        g = TO.adam_grad(rng, TRAJ_N, below=HYP["max_norm"] if t % 5 == 0 else None)
        yield t, p, g, m, v
        p, m, v, steps, _ = TO.adam_clip_f32(p, g, m, v, steps, n_decay=TRAJ_DECAY, **HYP)


def test_adam_f32_emulation_stays_within_half_of_every_bar():
    """adam_clip_f32 against adam_clip_ref, single steps from identical fp32 state (teacher forcing: the reference starts every step from
    the emulation's stored p, m, v), 40 steps at n = 5000, lr = wd = 1e-3, max_norm = 0.01, gradients log-uniform over [1e-10, 1e-1] with
    2 % exact zeros, every fifth gradient under max_norm.  Every element of every step within HALF of its bar (train_tail_oracle.adam_bars
    with frac = 0.5: half of each counted part; the u |p0| of the parameter's own final rounding is one hard-bounded operation and stays).
    Worst errors measured with this recipe, in u of each bar's scale: m 3.91 u of M (bar 8 u), v 6.78 u of V (bar 16 u), p 4.34 u of D beyond
    u |p0| (bar 16 u), norm 0.88 u (bar 2 u)."""
    worst = dict(p=0.0, m=0.0, v=0.0, norm=0.0)
    for t, p, g, m, v in trajectory():
        steps = np.array([t - 1])
        ref = TO.adam_clip_ref(p, g, m, v, steps, n_decay=TRAJ_DECAY, with_coef=True, **HYP)
        emu = TO.adam_clip_f32(p, g, m, v, steps, n_decay=TRAJ_DECAY, **HYP)
        if t % 5 == 0:
            assert ref[5]["coef"] == 1.0
        half = TO.adam_bars(p, ref, frac=0.5)
        for k, i in (("p", 0), ("m", 1), ("v", 2)):
            err = np.abs(emu[i].astype(np.float64) - ref[i])
            ok = err <= half[i]
            assert ok.all(), (t, k, int((~ok).sum()), float(np.max(err[~ok] / half[i][~ok])))
        # the figures of the docstring: m, v in u of M, V; p as (error - u |p0|) in u of D (train_tail_oracle: the bars' scales)
        scale_m, scale_v, scale_p = ref[5]["m_abs"], ref[5]["v_abs"], ref[5]["upd_abs"]
        for k, i, sc, off in (("m", 1, scale_m, 0.0), ("v", 2, scale_v, 0.0), ("p", 0, scale_p, U * np.abs(p.astype(np.float64)))):
            nz = sc > 0
            e = np.abs(emu[i].astype(np.float64) - ref[i]) - off
            worst[k] = max(worst[k], float(np.max(e[nz] / sc[nz])) / U)
        en = abs(float(emu[4]) - ref[4])
        assert en <= half[3]
        worst["norm"] = max(worst["norm"], en / ref[4] / U)
        assert emu[3].tolist() == ref[3].tolist() == [t]
    print(f"\n[adam fp32 emulation] worst errors in u of each bar's scale: {worst}")


@pytest.mark.parametrize("variant", [v for v in TO.VARIANTS if v != "shared_counter"])
def test_bars_tell_wrong_adam_formulas_apart(variant):
    """On the trajectory's inputs at t = 1, 2, 7 and 40, a reference with one deliberately wrong formula lies at least 1000 bars from the
    right one in p (decay on the tail: in m as well) -- the inputs of the GPU test can tell the formulas apart."""
    seen = set()
    for t, p, g, m, v in trajectory():
        if t not in (1, 2, 7, 40):
            continue
        seen.add(t)
        kw = dict(n_decay=TRAJ_DECAY, **HYP)
        ref = TO.adam_clip_ref(p, g, m, v, [t - 1], with_coef=True, **kw)
        bad = TO.adam_clip_ref(p, g, m, v, [t - 1], variant=variant, **kw)
        bars = TO.adam_bars(p, ref)
        dist_p = float(np.max(np.abs(bad[0] - ref[0]) / bars[0]))
        print(f"\n[{variant}] t = {t}: {dist_p:.3g} bars in p")
        assert dist_p >= 1000, (variant, t, dist_p)
        if variant == "decay_tail":
            tail = slice(TRAJ_DECAY, None)
            assert float(np.max(np.abs(bad[1] - ref[1])[tail] / bars[1][tail])) >= 1000
    assert seen == {1, 2, 7, 40}


GROUP_SEGMENTS, GROUP_COUNTERS = TO.GROUP_SEGMENTS, TO.GROUP_COUNTERS


def test_bars_tell_a_shared_step_counter_apart():
    """Groups whose counters differ (0, 9, 999, 123456): bias corrections read from counter 0 for every group lie >= 1000 bars away in p."""
    rng = np.random.default_rng(4)
    p, g, m, v = TO.adam_inputs(rng, 6000)
    kw = dict(n_decay=4321, segments=GROUP_SEGMENTS, active={0, 1, 2, 3}, **HYP)
    ref = TO.adam_clip_ref(p, g, m, v, GROUP_COUNTERS, with_coef=True, **kw)
    bad = TO.adam_clip_ref(p, g, m, v, GROUP_COUNTERS, variant="shared_counter", **kw)
    bars = TO.adam_bars(p, ref)
    grp = TO.group_of(6000, GROUP_SEGMENTS)
    for gid in (1, 2, 3):
        assert float(np.max((np.abs(bad[0] - ref[0]) / bars[0])[grp == gid])) >= 1000, gid
    assert np.array_equal(bad[0][grp == 0], ref[0][grp == 0])
    emu = TO.adam_clip_f32(p, g, m, v, GROUP_COUNTERS, **{k: kw[k] for k in kw})
    half = TO.adam_bars(p, ref, frac=0.5)
    for i in range(3):
        assert (np.abs(emu[i].astype(np.float64) - ref[i]) <= half[i]).all()
    assert emu[3].tolist() == ref[3].tolist() == [1, 10, 1000, 123457]


# ---- d. the distance between the kernel's hyperparameters and torch's -------------------------------------------------------------------
def test_rounded_hyperparameters_deviation_is_small_and_known():
    """v after one step with nominal double hyperparameters against fp32-rounded ones: 1 - fl(0.999) is not fl(0.001).  Measured 1.3e-5
    relative (the known distance to torch's fp32 Adam, which multiplies by fl(1 - beta2)); asserted below 1e-4."""
    rng = np.random.default_rng(5)
    p, g, m, v = TO.adam_inputs(rng, 5000)
    v[:] = 0                                                # from zero moments v' = (1 - beta2) g^2: the whole deviation shows
    kw = dict(n_decay=4321, **HYP)
    a = TO.adam_clip_ref(p, g, m, v, [0], f32_hyper=False, **kw)[2]
    rb = TO.adam_clip_ref(p, g, m, v, [0], f32_hyper=True, with_coef=True, **kw)
    b, scale = rb[2], rb[5]["v_abs"]                        # relative to V: no credit for the decay term cancelling the gradient
    nz = scale > 0
    dev = float(np.max(np.abs(a[nz] - b[nz]) / scale[nz]))
    print(f"\n[1 - beta] relative deviation of v, nominal against fp32-rounded hyperparameters: {dev:.3e}")
    assert 0 < dev < 1e-4


# ---- e. the loss reference -------------------------------------------------------------------------------------------------------------
LOSS_SETTINGS = [(("l1_loss",), (1.0,)), (("log_l1_loss",), (1.0,)), (("mse_loss",), (1.0,)), (("log_mse_loss",), (1.0,)),
                 (("l1_loss", "log_mse_loss", "mse_loss"), (0.5, 2.0, 0.01))]
LOSS_INDEX = {"l1_loss": 0, "log_l1_loss": 1, "mse_loss": 2, "log_mse_loss": 3}       # popcorn_amd.train.LOSS_INDEX


def lam4_of(losses, lams):
    lam4 = [0.0] * 4
    for lo, la in zip(losses, lams):
        lam4[LOSS_INDEX[lo]] += la
    return lam4


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("losses,lams", LOSS_SETTINGS)
def test_loss_ref_equals_float64_autograd_through_the_oracle(losses, lams, world):
    """loss_ref against float64 autograd through oracle.popcorn_oracle.get_loss: each loss, the mix, world 1 and 2 (a rank's share of a
    global batch mean: the rank's loss part and gradients are 1 / world of the single-process ones), 1e-12 relative."""
    from oracle import popcorn_oracle as O
    rng = np.random.default_rng(6)
    B = 37
    pc, y, _ = TO.loss_inputs(rng, B)
    scale = rng.random(500)
    lam_weak, sreg = 100.0, 0.0078125                      # (exact in fp32: the reference takes its scalars as fp32 values)
    lams = tuple(float(np.float32(x)) for x in lams)
    p = torch.tensor(pc.astype(np.float64), requires_grad=True)
    sc = torch.tensor(scale, requires_grad=True)
    ref, _ = O.get_loss({"popcount": p}, {"y": torch.tensor(y.astype(np.float64))}, scale=sc, loss=list(losses), lam=list(lams),
                        scale_regularization=sreg, tag="weak")
    # get_loss casts the scale to float for its mean; add the regulariser in double instead so the bar can be 1e-12
    ref = ref - sreg * sc.float().abs().mean() + sreg * sc.abs().mean()
    (ref * lam_weak).backward()
    inv_B = 1.0 / (world * B)
    stats = (float(scale.size), float(scale.sum()))
    loss, reg, g, gsc = TO.loss_ref(pc, y, lam4_of(losses, lams), sreg, lam_weak, np.float64(inv_B), stats)
    # loss_ref rounds inv_B to fp32 as the kernel's argument is: undo that factor exactly for the comparison
    r = inv_B / float(np.float32(inv_B))
    assert abs(reg - sreg * scale.mean()) <= 1e-12 * reg
    assert abs((loss - reg) * r * world + reg - ref.item()) <= 1e-12 * abs(ref.item())
    assert _rel(g * r * world, p.grad.numpy()) <= 1e-12
    assert abs(gsc - sc.grad[0].item()) <= 1e-12 * abs(gsc)


def test_loss_ref_regulariser_off():
    pc, y, _ = TO.loss_inputs(np.random.default_rng(7), 20)
    for sreg, stats in ((0.0, (10.0, 5.0)), (0.01, None), (0.01, (0.0, 0.0))):
        loss, reg, g, gsc = TO.loss_ref(pc, y, [0, 1, 0, 0], sreg, 100.0, 0.05, stats)
        assert reg == 0.0 and gsc == 0.0 and np.isfinite(loss) and np.isfinite(g).all()


@pytest.mark.parametrize("losses,lams", LOSS_SETTINGS)
def test_loss_f32_emulation_stays_within_half_of_the_bars(losses, lams):
    """loss_f32 (pc_loss_block in numpy fp32, numpy's float log for logf) against loss_ref at B = 600 with planted ties and zeros: loss,
    regulariser, every g_popcount[b], g_scale_const within half of their bars; ties give exactly 0.  Half bars: loss_bars with frac = 0.5 (half of the doubled
    counts; the delta terms are worst cases of their own).  Worst measured over the five settings: g_popcount 0.58 of its half bar (log_mse,
    where the two roundings of pc + 1 and y + 1 dominate), loss 0.10."""
    rng = np.random.default_rng(8)
    pc, y, ties = TO.loss_inputs(rng, 600)
    assert len(ties) == 10 and (y == 0).sum() == 5 and (pc == 0).sum() == 3
    lam4 = lam4_of(losses, lams)
    args = (pc, y, lam4, 0.01, 100.0, 1.0 / 600, (12345.0, 4321.5))
    loss, reg, g, gsc = TO.loss_ref(*args)
    eloss, ereg, eg, egsc = TO.loss_f32(*args)
    b_loss, b_reg, b_g, b_gsc = TO.loss_bars(*args, frac=0.5)
    err = np.abs(eg.astype(np.float64) - g)
    assert (err <= b_g).all(), float(np.max(err / np.maximum(b_g, 1e-300)))
    assert (eg[ties] == 0).all() and (g[ties] == 0).all()
    assert abs(float(eloss) - loss) <= b_loss and abs(float(ereg) - reg) <= b_reg and abs(float(egsc) - gsc) <= b_gsc
    nz = b_g > 0
    print(f"\n[loss fp32 emulation] {losses}: worst g error / half bar {float(np.max(err[nz] / b_g[nz])):.3f}, loss error / half bar "
          f"{abs(float(eloss) - loss) / b_loss:.3f}")
