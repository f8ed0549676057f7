"""The kernels that end every training step, each on its own against the float64 references and bars of tests/train_tail_oracle.py:
pc_adam_clip_step_fused (csrc/train_ops.hip), pc_loss_fwd_bwd / pc_loss_block (csrc/common.h), pc_head_popcount_loss over
pc_popcount_sums_block (csrc/head.hip) and pc_zero_fill (csrc/mask.hip).  tests/test_train_tail_cpu.py shows that the references equal
torch's and that fp32 arithmetic attains half of every bar.

The Adam kernel's last-workgroup ticket is ONE static device word per process: the optimiser is launched on one stream at a time (the
trainer's only use), and nothing here launches it on two streams at once."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_tail_oracle as TO

pytestmark = pytest.mark.gpu
HYP = TO.HYP
REAL_N = 39298            # the product model's flat parameter count (56 tensors: oracle.popcorn_oracle.trainable_names)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def adam_warm_up():
    """One eager launch before anything else: the first call allocates and clears the kernel's static ticket with a device synchronise,
    which must not fall inside a graph capture."""
    st = _State(*TO.adam_inputs(np.random.default_rng(0), 8), [0])
    st.launch(n_decay=8)
    torch.cuda.synchronize()


class _State:
    """Flat fp32 optimiser state on the device."""

    def __init__(self, p, g, m, v, steps, lr=HYP["lr"], norm_fill=-7.25):
        dev = "cuda"
        self.p, self.g, self.m, self.v = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (p, g, m, v))
        st = np.zeros(4, dtype=np.int32)
        st[:len(steps)] = steps
        self.step = torch.from_numpy(st).to(dev)
        self.hyper = torch.tensor([lr], dtype=torch.float32, device=dev)
        self.norm = torch.full((1,), norm_fill, dtype=torch.float32, device=dev)

    def launch(self, n_decay, wd=HYP["wd"], max_norm=HYP["max_norm"], groups=None, g=None):
        from popcorn_amd import ops
        ops.adam_clip_step_fused(self.p, self.g if g is None else g, self.m, self.v, n_decay, self.hyper, wd, HYP["beta1"], HYP["beta2"],
                                 HYP["eps"], max_norm, self.norm, self.step, groups=groups)

    def host(self):
        torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.p, self.m, self.v, self.step)) + (float(self.norm.item()),)

    def clone(self):
        c = object.__new__(_State)
        for k, t in self.__dict__.items():
            setattr(c, k, t.clone())
        return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# largest error / bar any Adam comparison of this module met, printed at the end.  On an MI355X: m 0.50 (4.0 u of M), v 0.45 (7.1 u of V),
# norm 0.44, p 0.99 -- the u |p0| of p's own final rounding, which is reached whenever the update is small next to the parameter.
WORST = {"p": 0.0, "m": 0.0, "v": 0.0, "norm": 0.0}


@pytest.fixture(scope="module", autouse=True)
def adam_worst_report():
    yield
    print(f"\n[adam kernel] worst error / bar over every comparison of this module: {WORST}")


def _check(tag, got, p0, ref, norm_expected=True):
    """p, m, v of one launch under the bars, element by element (no element excluded); norm_out under its bar."""
    bars = TO.adam_bars(p0, ref)
    for name, i in (("p", 0), ("m", 1), ("v", 2)):
        err = np.abs(got[i].astype(np.float64) - ref[i])
        bad = ~(err <= bars[i])
        assert not bad.any(), (tag, name, int(bad.sum()), int(np.argmax(bad)), float(np.max(err[bad] / np.maximum(bars[i][bad], 1e-300))))
        nz = bars[i] > 0
        if nz.any():
            WORST[name] = max(WORST[name], float(np.max(err[nz] / bars[i][nz])))
    if norm_expected:
        assert abs(got[4] - ref[4]) <= bars[3], (tag, got[4], ref[4])
        if bars[3] > 0:
            WORST["norm"] = max(WORST["norm"], abs(got[4] - ref[4]) / bars[3])


def _odd_decay(n):
    k = max(1, (2 * n) // 3)
    while k % 4 == 0 or k % 1024 == 0:
        k += 1
    return min(k, n)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 4099, 28671, 28672, 28676, 32767, 32768, 32771, REAL_N, 65541])
def test_adam_size_sweep(n):
    """One teacher-forced step from non-zero random m, v > 0 at the sizes where the kernel changes path: the norm's 8-deep main loop first
    runs at n / 4 > 7 * 1024 (28672 / 4 = 7168 is the last size without it, 28676 the first with), its tail batch is guarded per float4, its
    scalar tail takes n % 4 elements, and the update grid is ceil(n / 1024) workgroups.  n_decay in {0, n, a value that is neither a
    multiple of 4 nor of 1024}, weight decay on and off, max_norm 0.01 and 0 (then norm_out, pre-filled with a sentinel, is left alone).
    p, m, v under the bars against adam_clip_ref, norm_out under its bar, the step counter + 1."""
    rng = np.random.default_rng(100 + n)
    p, g, m, v = TO.adam_inputs(rng, n)
    t0 = 3
    for n_decay in sorted({0, n, _odd_decay(n)}):
        for wd in (0.0, HYP["wd"]):
            for max_norm in (HYP["max_norm"], 0.0):
                st = _State(p, g, m, v, [t0])
                st.launch(n_decay, wd=wd, max_norm=max_norm)
                got = st.host()
                kw = dict(HYP, wd=wd, max_norm=max_norm)
                ref = TO.adam_clip_ref(p, g, m, v, [t0], n_decay=n_decay, with_coef=True, **kw)
                tag = (n, n_decay, wd, max_norm)
                _check(tag, got, p, ref, norm_expected=max_norm > 0)
                if max_norm == 0:
                    assert got[4] == -7.25, tag                       # the sentinel: no norm is computed, none is written
                    assert ref[5]["coef"] == 1.0
                assert got[3].tolist() == [t0 + 1, 0, 0, 0], tag


def test_adam_trajectory_teacher_forced():
    """The 40-step recipe of tests/test_train_tail_cpu.py on the device, each step checked against adam_clip_ref started from the kernel's
    own stored state (teacher forcing).  Every fifth gradient has its norm under max_norm: coef must be exactly 1 there -- the result equals
    the max_norm = 0 launch from the same state bit for bit.  lr is changed on the device between launches (the scheduler's route), and
    one step runs at lr = 0: p bit-identical, m and v advanced."""
    rng = np.random.default_rng(3)
    p, _, m, v = TO.adam_inputs(rng, TO.TRAJ_N)
    st = _State(p, np.zeros_like(p), m, v, [0])
    lr = HYP["lr"]
    for t in range(1, TO.TRAJ_STEPS + 1):
        g = TO.adam_grad(rng, TO.TRAJ_N, below=HYP["max_norm"] if t % 5 == 0 else None)
        if t == 11:
            lr = 5e-4
        if t == 23:
            lr = 0.0
        if t == 24:
            lr = 2e-3
        st.hyper.fill_(lr)
        st.g.copy_(torch.from_numpy(g))
        p0, m0, v0, s0, _ = st.host()
        assert s0[0] == t - 1
        twin = st.clone() if t % 5 == 0 else None
        st.launch(TO.TRAJ_DECAY)
        got = st.host()
        ref = TO.adam_clip_ref(p0, g, m0, v0, [t - 1], n_decay=TO.TRAJ_DECAY, with_coef=True, **dict(HYP, lr=lr))
        _check(("trajectory", t), got, p0, ref)
        if twin is not None:
            assert ref[5]["coef"] == 1.0
            twin.launch(TO.TRAJ_DECAY, max_norm=0.0)
            tw = twin.host()
            for i in range(3):
                assert np.array_equal(_bits(got[i]), _bits(tw[i])), ("coef == 1", t, i)
        if lr == 0.0:
            assert np.array_equal(_bits(got[0]), _bits(p0))
            assert not np.array_equal(got[1], m0) and not np.array_equal(got[2], v0)
    assert st.host()[3].tolist() == [TO.TRAJ_STEPS, 0, 0, 0]


GROUP_ACTIVE = [set(), {0}, {1}, {2}, {3}, {0, 2}, {0, 1, 2, 3}]


@pytest.mark.parametrize("active", GROUP_ACTIVE, ids=lambda a: "active_" + ("".join(map(str, sorted(a))) or "none"))
def test_adam_groups(active):
    """Parameter groups: segment ends (7, 1030, 2049, 5001, 6000) inside float4s and workgroups, mapped to groups (2, 0, 1, 0, 3) -- not
    monotone -- with n_decay = 4321 inside a segment and counters preset to 0, 9, 999, 123456.  The gradients of inactive groups are exactly
    zero: that is the contract of the callers (csrc/step.hip zero-fills the U-Net part of the flat gradient on limit1 / limit2 steps,
    train.py does the same), because the kernel takes the norm over the whole buffer.  Active elements under the bars with their own
    group's step count; inactive elements of p, m, v bit-identical; counters + 1 on active groups only."""
    from popcorn_amd import ops
    rng = np.random.default_rng(200 + sum(1 << a for a in active))
    n = TO.GROUP_N
    p, g, m, v = TO.adam_inputs(rng, n)
    grp = TO.group_of(n, TO.GROUP_SEGMENTS)
    on = np.isin(grp, sorted(active))
    g[~on] = 0.0
    st = _State(p, g, m, v, TO.GROUP_COUNTERS)
    st.launch(TO.GROUP_DECAY, groups=ops.adam_groups(TO.GROUP_SEGMENTS, active))
    got = st.host()
    ref = TO.adam_clip_ref(p, g, m, v, TO.GROUP_COUNTERS, n_decay=TO.GROUP_DECAY, segments=TO.GROUP_SEGMENTS, active=active,
                           with_coef=True, **HYP)
    _check(("groups", sorted(active)), got, p, ref)
    for a, b in ((got[0], p), (got[1], m), (got[2], v)):
        assert np.array_equal(_bits(a)[~on], _bits(b)[~on])
        if on.any():
            assert not np.array_equal(a[on], b[on])
    assert got[3].tolist() == [c + (i in active) for i, c in enumerate(TO.GROUP_COUNTERS)] == ref[3].tolist()


def test_adam_norm_counts_inactive_gradients():
    """The contract itself: the norm (and so the clip coefficient of the active groups) is taken over the WHOLE gradient buffer; a non-zero
    gradient left in an inactive group is counted in norm_out.  Callers zero it."""
    from popcorn_amd import ops
    rng = np.random.default_rng(300)
    n = TO.GROUP_N
    p, g, m, v = TO.adam_inputs(rng, n)
    grp = TO.group_of(n, TO.GROUP_SEGMENTS)
    st = _State(p, g, m, v, TO.GROUP_COUNTERS)
    st.launch(TO.GROUP_DECAY, groups=ops.adam_groups(TO.GROUP_SEGMENTS, {0}))
    got = st.host()
    whole = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    own = float(np.sqrt(np.sum(g[grp == 0].astype(np.float64) ** 2)))
    assert abs(got[4] - whole) <= 2 * TO.U * whole and abs(whole - own) > 1e3 * TO.U * whole
    ref = TO.adam_clip_ref(p, g, m, v, TO.GROUP_COUNTERS, n_decay=TO.GROUP_DECAY, segments=TO.GROUP_SEGMENTS, active={0}, with_coef=True, **HYP)
    _check("contract", got, p, ref)


def test_adam_ticket_across_grid_sizes():
    """Back-to-back launches of 1, 65, 1 and 1 workgroups on one stream without a host synchronisation in between: the ticket returns to
    zero after every launch whatever the grid, so every launch advances its counter once and computes the right step."""
    rng = np.random.default_rng(400)
    runs = []
    for n in (5, 65541, 1024, 5):
        p, g, m, v = TO.adam_inputs(rng, n)
        runs.append((n, (p, g, m, v), _State(p, g, m, v, [6])))
    for n, _, st in runs:
        st.launch(_odd_decay(n))
    for n, (p, g, m, v), st in runs:
        got = st.host()
        ref = TO.adam_clip_ref(p, g, m, v, [6], n_decay=_odd_decay(n), with_coef=True, **HYP)
        _check(("ticket", n), got, p, ref)
        assert got[3].tolist() == [7, 0, 0, 0], n


def test_adam_graph_replay_equals_eager():
    """One launch captured with torch.cuda.graph (a single kernel node, no parallel branch) and replayed three times: the device counter
    advances by 3 and p, m, v equal three eager launches bit for bit."""
    rng = np.random.default_rng(500)
    n = 4099
    p, g, m, v = TO.adam_inputs(rng, n)
    eager, graphed = _State(p, g, m, v, [2]), _State(p, g, m, v, [2])
    for _ in range(3):
        eager.launch(_odd_decay(n))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.launch(_odd_decay(n))
    torch.cuda.synchronize()
    assert graphed.host()[3].tolist() == [2, 0, 0, 0]                  # capture enqueues nothing
    for _ in range(3):
        graph.replay()
    a, b = eager.host(), graphed.host()
    assert a[3].tolist() == b[3].tolist() == [5, 0, 0, 0]
    for i in range(3):
        assert np.array_equal(_bits(a[i]), _bits(b[i])), i
    assert a[4] == b[4]
    # and the three steps are the right ones: the last of them against the reference from the state two eager launches leave
    two = _State(p, g, m, v, [2])
    two.launch(_odd_decay(n))
    two.launch(_odd_decay(n))
    s2 = two.host()
    ref = TO.adam_clip_ref(s2[0], g, s2[1], s2[2], [4], n_decay=_odd_decay(n), with_coef=True, **HYP)
    _check("replay", b, s2[0], ref)


def _raw_groups(nseg, ends, gids, mask):
    from popcorn_amd import _lib as L
    g = L.PcAdamGroups()
    g.nseg = nseg
    for i, (e, k) in enumerate(zip(ends, gids)):
        g.seg_end[i], g.seg_group[i] = e, k
    g.active_mask = mask
    return g


@pytest.mark.parametrize("case", ["misaligned_gradient", "last_end_not_n", "decreasing_ends", "group_id_4"])
def test_adam_refusals_change_nothing(case):
    """Arguments the launcher refuses with PC_EINVAL before anything is enqueued: a gradient pointer that is not 16-byte aligned (a view
    offset by one element), a segment table that does not end at n, decreasing segment ends, a group id outside [0, 4)."""
    from popcorn_amd import _lib as L
    rng = np.random.default_rng(600)
    n = 1025
    p, g, m, v = TO.adam_inputs(rng, n)
    st = _State(p, g, m, v, [1, 2, 3, 4])
    before = st.host()
    kw = {}
    if case == "misaligned_gradient":
        wide = torch.zeros(n + 4, dtype=torch.float32, device="cuda")
        wide[1:n + 1].copy_(st.g)
        kw["g"] = wide[1:n + 1]
        assert kw["g"].data_ptr() % 16 == 4
    elif case == "last_end_not_n":
        kw["groups"] = _raw_groups(2, (500, n - 1), (0, 1), 3)
    elif case == "decreasing_ends":
        kw["groups"] = _raw_groups(3, (500, 400, n), (0, 1, 2), 7)
    else:
        kw["groups"] = _raw_groups(2, (500, n), (0, 4), 3)
    with pytest.raises(L.PopcornHipError, match=rf"error {L.PC_EINVAL}:"):
        st.launch(_odd_decay(n), **kw)
    after = st.host()
    for a, b in zip(before[:4], after[:4]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert before[4] == after[4]


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
LOSS_LAM4 = {"l1": [1, 0, 0, 0], "log_l1": [0, 1, 0, 0], "mse": [0, 0, 1, 0], "log_mse": [0, 0, 0, 1], "mix": [0.5, 0, 0.01, 2.0]}


def _loss_dev(pc, y, stats, lam4, sreg, lam_weak, inv_B):
    from popcorn_amd import ops
    B = pc.size
    st = None if stats is None else torch.tensor(stats, dtype=torch.float64, device="cuda")
    loss_out = torch.full((2,), float("nan"), device="cuda")
    g_pc = torch.full((B,), float("nan"), device="cuda")
    g_sc = torch.full((1,), float("nan"), device="cuda")
    ops.loss_fwd_bwd(torch.from_numpy(pc).cuda(), torch.from_numpy(y).cuda(), st, lam4, sreg, lam_weak, inv_B, loss_out, g_pc, g_sc)
    torch.cuda.synchronize()
    return loss_out.cpu().numpy(), g_pc.cpu().numpy(), float(g_sc.item())


@pytest.mark.parametrize("setting", list(LOSS_LAM4))
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 600])
def test_loss_kernel_vs_float64(B, setting):
    """pc_loss_fwd_bwd at batch sizes on both sides of its 256-thread stride (the ``b += 256`` loop iterates from B = 257 on; 600 takes it
    three times) against loss_ref under loss_bars: pc and y log-uniform over [1e-2, 1e5] with |pc - y| >= 1e-2 max(y, 1) on every non-tie
    sample, ten bit-equal ties, five y = 0, three pc = 0 (as many as B holds); the four losses and the l1 / log_mse / mse mix, world 1 and
    2, the regulariser with stats, without stats (sreg = 0) and with Nsel = 0 at sreg > 0 (reg = 0 and g_scale_const = 0).  Loss,
    regulariser, every g_popcount[b] and g_scale_const under the bars; no NaN anywhere; tie samples get a gradient of exactly 0.
    logf: the bars take TO.LOGF_ULP, twice what test_logf_error_observed measures."""
    rng = np.random.default_rng(700 + B)
    pc, y, ties = TO.loss_inputs(rng, B)
    lam4 = LOSS_LAM4[setting]
    lam_weak = 100.0
    for world in (1, 2):
        inv_B = 1.0 / (world * B)
        for sreg, stats in ((0.01, (12345.0, 4321.5)), (0.0, None), (0.01, (0.0, 0.0))):
            args = (pc, y, lam4, sreg, lam_weak, inv_B, stats)
            loss_out, g_pc, g_sc = _loss_dev(pc, y, stats, lam4, sreg, lam_weak, inv_B)
            loss, reg, g, gsc = TO.loss_ref(*args)
            b_loss, b_reg, b_g, b_gsc = TO.loss_bars(*args)
            tag = (B, setting, world, sreg, stats)
            assert np.isfinite(loss_out).all() and np.isfinite(g_pc).all() and np.isfinite(g_sc), tag
            err = np.abs(g_pc.astype(np.float64) - g)
            bad = ~(err <= b_g)
            assert not bad.any(), (tag, int(bad.sum()), int(np.argmax(bad)), float(np.max(err[bad] / np.maximum(b_g[bad], 1e-300))))
            assert abs(float(loss_out[0]) - loss) <= b_loss, (tag, float(loss_out[0]), loss, b_loss)
            assert abs(float(loss_out[1]) - reg) <= b_reg and abs(g_sc - gsc) <= b_gsc, tag
            if stats is None or stats[0] == 0:
                assert loss_out[1] == 0.0 and g_sc == 0.0, tag
            assert (g_pc[ties] == 0).all() and (g[ties] == 0).all(), tag


@pytest.mark.parametrize("setting", ["l1", "log_l1", "mix"])
def test_loss_of_exact_ties_is_exactly_zero(setting):
    """A batch of bit-equal pc == y (zeros included): d and dl are exactly 0 in the kernel, so the l1 and log-l1 contributions, every other
    term, the loss and every gradient are exactly 0."""
    rng = np.random.default_rng(800)
    pc = (10.0 ** rng.uniform(-2, 5, size=300)).astype(np.float32)
    pc[::50] = 0.0
    loss_out, g_pc, g_sc = _loss_dev(pc, pc.copy(), None, LOSS_LAM4[setting], 0.0, 100.0, 1.0 / 300)
    assert loss_out.tolist() == [0.0, 0.0] and (g_pc == 0).all() and g_sc == 0.0


def test_logf_error_observed():
    """The device logf as pc_loss_block calls it, observed through the kernel: B = 1, log-l1 only, y = 0, lam_weak = inv_B = 1 make
    loss_out[0] = |logf(pc + 1) - logf(1)| = logf(pc + 1) with no further rounding.  Against the float64 log of the fp32 sum pc + 1, in
    units of the fp32 result's last place, over 2300 arguments from 1e-7 to 1e5 and the sums next to powers of two.  Observed on an
    MI355X: 2.118 ulp (TO.OBSERVED_LOGF_ULP; the hardware log2 of 1 ulp times ln 2, see there), above the 2 ulp first assumed, so the loss
    bars take TO.LOGF_ULP = twice the observed figure; the assertion holds the device to that."""
    from popcorn_amd import ops
    rng = np.random.default_rng(900)
    near = np.array([2.0 ** k + s * 2.0 ** (k - 23) for k in range(1, 17) for s in (-2, -1, 0, 1, 2)]) - 1.0
    pc = np.concatenate([10.0 ** rng.uniform(-2, 5, size=1800), 10.0 ** rng.uniform(-7, -2, size=420), near]).astype(np.float32)
    N = pc.size
    pcd, y = torch.from_numpy(pc).cuda(), torch.zeros(N, device="cuda")
    loss_out, g_pc, g_sc = torch.zeros(N, 2, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(1, device="cuda")
    for i in range(N):
        ops.loss_fwd_bwd(pcd[i:i + 1], y[i:i + 1], None, [0, 1, 0, 0], 0.0, 1.0, 1.0, loss_out[i], g_pc[i:i + 1], g_sc)
    torch.cuda.synchronize()
    got = loss_out[:, 0].cpu().numpy().astype(np.float64)
    arg = (pc + np.float32(1)).astype(np.float64)
    ref = np.log(arg)
    nz = ref > 0
    ulps = np.abs(got[nz] - ref[nz]) / np.spacing(ref[nz].astype(np.float32)).astype(np.float64)
    assert (got[~nz] == 0).all()
    worst = float(ulps.max())
    print(f"\n[logf] worst error of the device logf through pc_loss_block: {worst:.3f} ulp at pc = {pc[nz][int(ulps.argmax())]!r} "
          f"(assumed {TO.LOGF_ULP}, recorded {TO.OBSERVED_LOGF_ULP})")
    assert worst <= TO.LOGF_ULP


# ---- popcount reduce ------------------------------------------------------------------------------------------------------------------
def _head_case(B, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    pad = 8
    feat = torch.randn(B, 16, H + 2 * pad, W + 2 * pad, generator=gen)
    shapes = [(64, 16, 1, 1), (64,), (64, 64, 1, 1), (64,), (64, 64, 1, 1), (64,), (2, 64, 1, 1), (2,)]
    ht = []
    for s in shapes:
        fan = s[1] if len(s) == 4 else 1
        ht.append(torch.randn(*s, generator=gen) * (1.0 / fan ** 0.5 if len(s) == 4 else 0.1))
    building = torch.rand(B, 1, H, W, generator=gen)
    admin = (torch.rand(B, H, W, generator=gen) < 0.6).float() * 5.0
    census = torch.full((B,), 5, dtype=torch.int64)
    mask = ((torch.rand(B, H, W, generator=gen) < 0.5) & (admin == 5.0)).to(torch.uint8)
    y = (10.0 ** (torch.rand(B, generator=gen) * 3)).float()
    counts = torch.tensor([int(mask.sum()), int((admin == 5.0).sum())], dtype=torch.int32)
    return pad, feat, ht, building, admin, census, mask, y, counts


@pytest.mark.parametrize("split", [1, 0], ids=["split", "mfma"])
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (3, 16, 16), (5, 16, 16), (40, 16, 16), (64, 16, 16), (65, 16, 16), (129, 16, 16),
                                   (257, 16, 16), (3, 100, 100), (40, 64, 64), (129, 48, 48)])
def test_popcount_reduce_deferred_equals_two_launch(B, H, W, split):
    """pc_popcount_sums_block at the batch sizes where its threads-per-sample changes (tpb = 256, 64, 32, 4, 4, 2, 1, 1) and, by the formula
    of head_fwd_chunks, at chunk counts below (3 x 100 x 100: up to 10 chunks, tpb 64), at and above tpb (40 x 64 x 64: up to 4 / 8 chunks in the
    two forms, tpb 4; 129 x 48 x 48: up to 3 / 5 chunks, tpb 1: the strided chunk loop iterates), in both multiplication forms of the head (pc_set_head_split).
    The two-launch path head_fwd + loss_fwd_bwd and the deferred path head_fwd(defer_reduce=True) + head_popcount_loss must give popcount,
    stats, loss_out, g_popcount and g_scale_const bit for bit (the source promises the same summation orders); popcount[b] equals the
    float64 sum of the returned popdensemap over the sample's census region within popcount_depth(...) * u relative (non-negative terms:
    train_tail_oracle.popcount_depth states how the depth follows from the chunk geometry)."""
    from popcorn_amd import ops, _lib as L
    pad, feat, ht, building, admin, census, mask, y, counts = _head_case(B, H, W, seed=1000 + B + H)
    dev = "cuda"
    feat, building, admin, census, mask, y, counts = (t.to(dev) for t in (feat, building, admin, census, mask, y, counts))
    ht = [t.to(dev) for t in ht]
    lam4, sreg, lam_weak, inv_B = [0.5, 1.0, 0.01, 2.0], 0.01, 100.0, 1.0 / B
    prev = L.lib().pc_set_head_split(split)
    try:
        out = []
        for deferred in (False, True):
            stats = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
            loss_out, g_pc, g_sc = (torch.full((k,), float("nan"), device=dev) for k in (2, B, 1))
            _, popdense, popcount = ops.head_fwd(feat, pad, pad, H, W, ht, building, mask=mask, admin_mask=admin, census_idx=census,
                                                 stats=stats, nsel_counts=counts, defer_reduce=deferred)
            if deferred:
                popcount.fill_(float("nan"))
                ops.head_popcount_loss(B, H, W, counts, y, lam4, sreg, lam_weak, inv_B, popcount, stats, loss_out, g_pc, g_sc)
            else:
                ops.loss_fwd_bwd(popcount, y, stats, lam4, sreg, lam_weak, inv_B, loss_out, g_pc, g_sc)
            torch.cuda.synchronize()
            out.append([t.cpu().numpy() for t in (popcount, stats, loss_out, g_pc, g_sc, popdense)])
    finally:
        L.lib().pc_set_head_split(prev)
    for name, a, b in zip(("popcount", "stats", "loss_out", "g_popcount", "g_scale_const", "popdensemap"), *out):
        assert np.isfinite(a).all(), name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    popcount, stats, _, _, _, popdense = out[1]
    region = (admin == 5.0).cpu().numpy()
    assert (popdense >= 0).all() and stats[0] == float(counts[0].item())
    ref = np.array([popdense[b].astype(np.float64)[region[b]].sum() for b in range(B)])
    assert (ref > 0).sum() >= (B + 1) // 2                           # the random head leaves most samples a non-trivial sum
    bar = TO.popcount_depth(B, H, W, 8 if split else 4) * TO.U * ref
    err = np.abs(popcount.astype(np.float64) - ref)
    assert (err <= bar).all(), (float(np.max(err / np.maximum(bar, 1e-300))), TO.popcount_depth(B, H, W, 8 if split else 4))


# ---- zero fill ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027, 2048 * 256 * 4 + 7])
def test_zero_fill(n):
    """pc_zero_fill (the step executor's clip norm on limit1 / limit2 steps relies on it): exactly [0, n) becomes zero, the next 8 elements
    keep their sentinel; the last length is past 2048 workgroups x 256 threads x 4, so the grid-stride loop iterates; a pointer offset by one
    element is refused with PC_EINVAL and nothing is written."""
    from popcorn_amd import _lib as L
    buf = torch.full((n + 16,), 7.25, dtype=torch.float32, device="cuda")
    stream = L.stream_ptr()
    assert buf.data_ptr() % 16 == 0
    rc = L.lib().pc_zero_fill(C.c_void_p(buf.data_ptr() + 4), C.c_int64(n), stream)
    torch.cuda.synchronize()
    assert rc == L.PC_EINVAL and bool((buf == 7.25).all())
    rc = L.lib().pc_zero_fill(C.c_void_p(buf.data_ptr()), C.c_int64(n), stream)
    torch.cuda.synchronize()
    assert rc == 0
    host = buf.cpu().numpy()
    assert not host[:n].view(np.uint32).any() and (host[n:] == 7.25).all()
