"""Float64 references, fp32 emulations and error bars for the kernels that end every training step (csrc/train_ops.hip:
adam_clip_fused_kernel, loss_fwd_bwd_kernel; csrc/common.h: pc_loss_block; csrc/head.hip: pc_popcount_sums_block).  Plain numpy: no torch,
no GPU.  tests/test_train_tail_cpu.py checks the references against torch and the emulations against the bars;
tests/test_gpu_train_tail.py holds the kernels to the same bars.

u = 2^-24 is the unit roundoff of fp32: one correctly rounded operation has a relative error of at most u.

Hyperparameters as the kernel receives them.  The C ABI passes lr (through the device word ``hyper[0]``), weight decay, beta1, beta2, eps
and max_norm as ``float``.  With ``f32_hyper=True`` (the default) the references take ``np.float32(x)`` widened to double, and their
``1 - beta`` is the exact double difference of the rounded beta -- bit for bit the kernel's ``1.f - beta`` (Sterbenz: the fp32 subtraction
is exact for beta in [0.5, 1]).  ``1 - fl(0.999)`` differs from ``fl(0.001)`` by 1.3e-5 relative, so with nominal double hyperparameters
the reference's ``v`` sits ~200 u from the kernel instead of a few u; ``f32_hyper=False`` is the nominal form that is compared with torch
(tests/test_train_tail_cpu.py measures the distance).

Bars (functions below; each is a first-order worst-case count of the kernel's roundings, written next to it):

  G = |g coef| + wd |p0| is the magnitude of the gradient after decay with no credit for cancellation between its two parts.

  norm   2 u * norm                        one rounding of the double sqrt to float (the double accumulation adds ~n * 2^-53), doubled.
  m      8 u * M,  M = beta1 |m0| + (1 - beta1) G
         coef = max_norm / (norm + 1e-6f): float norm, add, divide = 3 roundings; g * coef 1; fmaf(wd, p, g) 1; (1 - beta1) * g 1; the
         final sum 1: 7 on the gradient path; beta1 * m0 and the sum: 2 on the m0 path -> 8 u M bounds the worst case.
  v      16 u * V,  V = beta2 v0 + (1 - beta2) G^2   (= v_ref wherever g coef and wd p0 have one sign or one of them is negligible)
         the gradient after decay carries 5 u G (above), its square 10 u, (1 - beta2) * g 1, * g 1, the sum 1: 13 u on the gradient path,
         2 u on beta2 * v0.  Written against v_ref itself the bar would not be a bound where the decay term cancels the gradient.
  p      u |p0| + 16 u * D,  D = (lr / bc1) M / (sqrt(v_ref) / sqrt(bc2) + eps)
         D = |p_ref - p0| wherever beta1 m0 and the gradient term have one sign; it is larger only where they cancel, and there the
         error of m is 8 u M, not 8 u |m| (a draft of the trajectory recipe met a cancellation by a factor of 12 in m among its 200 000
         element steps: 25 u |p_ref - p0| in the emulation, 2 u of D).
         The final subtraction rounds once at the magnitude of p (u |p0| to first order); the update carries m (7 u M), the denominator
         (13 / 2 + sqrtf 1 + the float sqrt(bc2) 1 + divide 1 + add 1 = 10.5 u), the divide 1, the float step size 1 and the product 1:
         21 u if every rounding pulled the same way.  The bar is held at 16 u, under that count, because a tighter bar checks more: the
         fp32 emulation below, which makes every one of these roundings, stays under 8 u of D (measured 4.34 u) on 200 000 element steps
         with magnitudes over nine decades.  Where v itself cancelled (V > v_ref) the denominator's share grows by
         8 u (V / v_ref - 1) |p_ref - p0|, which is added.
  loss   see loss_bars: per-term counts, and the absolute error ``delta`` of logf(pc + 1) - logf(y + 1) for a logf of LOGF_ULP ulp.
"""
import numpy as np

U = 2.0 ** -24
# Accuracy of the device logf in units of the result's last place.  The first assumption was 2 ulp.  tests/test_gpu_train_tail.py::
# test_logf_error_observed measures it through the loss kernel against float64: worst 2.118 ulp on an MI355X (at pc = 582.3628, over 2300
# arguments).  Why: the device logf is the hardware base-2 logarithm (v_log_f32, 1 ulp of log2 x) times ln 2 in split precision; where
# log2 x sits one binade above ln x (here 9.19 against 6.37) one ulp of the former is 2 ln 2 = 1.39 ulp of the latter, and the product
# rounds on top of it.  Since the observation exceeds the assumption, the bars take twice the observed figure.
OBSERVED_LOGF_ULP = 2.118
LOGF_ULP = 2 * OBSERVED_LOGF_ULP

# the recipes the CPU and the GPU tests share
HYP = dict(lr=1e-3, wd=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.01)
TRAJ_N, TRAJ_STEPS, TRAJ_DECAY = 5000, 40, 4321
GROUP_N, GROUP_DECAY = 6000, 4321
GROUP_SEGMENTS = [(7, 2), (1030, 0), (2049, 1), (5001, 0), (6000, 3)]        # a non-monotone segment -> group map, ends inside float4s
GROUP_COUNTERS = [0, 9, 999, 123456]

VARIANTS = ("decay_tail", "step_off_by_one", "no_bc2", "eps_in_root", "eps_before_bc2", "decoupled_wd", "shared_counter")


def _hyper(x, f32):
    return float(np.float32(x)) if f32 else float(x)


def group_of(n, segments):
    """Group id of every element: segments = [(end offset, group id), ...], consecutive; element i belongs to the first segment whose end
    is above i (adam_group_of)."""
    grp = np.zeros(n, dtype=np.int64)
    if segments:
        lo = 0
        for end, gid in segments:
            grp[lo:end] = gid
            lo = max(lo, end)
    return grp


def _active_mask(n, grp, segments, active):
    if not segments:
        return np.ones(n, dtype=bool)
    act = np.zeros(n, dtype=bool)
    for a in set(active):
        act |= grp == a
    return act


def adam_clip_ref(p, g, m, v, steps, *, n_decay, lr, wd, beta1, beta2, eps, max_norm, segments=None, active=None, f32_hyper=True,
                  variant=None, with_coef=False):
    """One launch of pc_adam_clip_step_fused in float64: the gradient norm over the WHOLE buffer (inactive groups included: the trainer
    zeroes their gradients), coef = min(1, max_norm / (norm + 1e-6)) when max_norm > 0 else 1, L2 decay folded into the gradient on
    [0, n_decay), torch.optim.Adam's update with eps outside the square root, one step counter per group (segments given: 4 counters;
    else one) with each group's bias corrections from its own counter, inactive groups untouched, counter included.
    Returns (p', m', v', steps', norm) -- and, with ``with_coef``, a sixth value: a dict with coef and the non-cancelling magnitudes the
    bars are written in (adam_bars).  ``variant``: one of VARIANTS, a deliberately wrong
    formula for the discrimination test."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    steps = np.array(steps, dtype=np.int64).reshape(-1).copy()
    n = p.size
    lr, wd, beta1, beta2, eps, max_norm = (_hyper(x, f32_hyper) for x in (lr, wd, beta1, beta2, eps, max_norm))
    tiny = _hyper(1e-6, f32_hyper)
    norm = float(np.sqrt(np.sum(g * g)))
    coef = min(1.0, max_norm / (norm + tiny)) if max_norm > 0 else 1.0
    grp = group_of(n, segments)
    act = _active_mask(n, grp, segments, active)
    idx = np.arange(n)
    decay = idx < n_decay if variant != "decay_tail" else np.ones(n, dtype=bool)
    ge = g * coef
    if variant != "decoupled_wd":
        ge = ge + np.where(decay, wd, 0.0) * p
    m1 = beta1 * m + (1.0 - beta1) * ge
    v1 = beta2 * v + (1.0 - beta2) * ge * ge
    cnt = steps[grp] if segments else np.full(n, steps[0])
    if variant == "shared_counter":
        cnt = np.full(n, steps[0])
    t = (cnt + 1 + (1 if variant == "step_off_by_one" else 0)).astype(np.float64)
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    if variant == "no_bc2":
        denom = np.sqrt(v1) + eps
    elif variant == "eps_in_root":
        denom = np.sqrt(v1 / bc2 + eps)
    elif variant == "eps_before_bc2":
        denom = (np.sqrt(v1) + eps) / np.sqrt(bc2)
    else:
        denom = np.sqrt(v1) / np.sqrt(bc2) + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    if variant == "decoupled_wd":
        p1 = p1 - lr * np.where(decay, wd, 0.0) * p
    p1, m1, v1 = np.where(act, p1, p), np.where(act, m1, m), np.where(act, v1, v)
    if segments:
        for a in set(active):
            steps[a] += 1
    else:
        steps[0] += 1
    out = (p1, m1, v1, steps, norm)
    if not with_coef:
        return out
    G = np.abs(g * coef) + np.where(decay, wd, 0.0) * np.abs(p)
    m_abs = beta1 * np.abs(m) + (1.0 - beta1) * G
    v_abs = beta2 * v + (1.0 - beta2) * G * G
    return out + (dict(coef=coef, m_abs=m_abs, v_abs=v_abs, upd_abs=(lr / bc1) * m_abs / denom, act=act),)


def adam_clip_f32(p, g, m, v, steps, *, n_decay, lr, wd, beta1, beta2, eps, max_norm, segments=None, active=None):
    """The same launch in numpy float32, operation for operation as adam_clip_fused_kernel: double accumulation of the squared gradients
    and a double sqrt rounded to float, coef in float, fmaf for the decay (evaluated in double and rounded once: the product of two floats
    is exact in double), float m and v in the kernel's association, step size (float)(lr / bc1) and (float)sqrt(bc2) from double pow,
    sqrtf(v) / sqrt_bc2 + eps, p - step * (m / denom).  CPU only: it shows that the bars are attainable by fp32 arithmetic."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    steps = np.array(steps, dtype=np.int64).reshape(-1).copy()
    n = p.size
    lr, wd, beta1, beta2, eps, max_norm = (f(x) for x in (lr, wd, beta1, beta2, eps, max_norm))
    gd = g.astype(np.float64)
    norm = f(np.sqrt(np.sum(gd * gd)))
    coef = f(1.0)
    if max_norm > 0:
        coef = f(max_norm / f(norm + f(1e-6)))
        coef = f(1.0) if coef > 1 else coef
    grp = group_of(n, segments)
    act = _active_mask(n, grp, segments, active)
    ge = (g * coef).astype(f)
    if wd != 0:
        dec = (np.float64(wd) * p.astype(np.float64) + ge.astype(np.float64)).astype(f)
        ge = np.where(np.arange(n) < n_decay, dec, ge)
    omb1, omb2 = f(f(1.0) - beta1), f(f(1.0) - beta2)
    m1 = (beta1 * m).astype(f) + (omb1 * ge).astype(f)
    v1 = (beta2 * v).astype(f) + ((omb2 * ge).astype(f) * ge).astype(f)
    ng = 4 if segments else 1
    t = steps[:ng].astype(np.float64) + 1.0
    step_size = (np.float64(lr) / (1.0 - np.float64(beta1) ** t)).astype(f)
    sq_bc2 = np.sqrt(1.0 - np.float64(beta2) ** t).astype(f)
    gi = grp if segments else np.zeros(n, dtype=np.int64)
    denom = (np.sqrt(v1).astype(f) / sq_bc2[gi]).astype(f) + eps
    p1 = p - (step_size[gi] * (m1 / denom).astype(f)).astype(f)
    p1, m1, v1 = np.where(act, p1, p).astype(f), np.where(act, m1, m).astype(f), np.where(act, v1, v).astype(f)
    if segments:
        for a in set(active):
            steps[a] += 1
    else:
        steps[0] += 1
    return p1, m1, v1, steps, (norm if max_norm > 0 else None)


def adam_bars(p0, ref, frac=1.0):
    """(bar_p, bar_m, bar_v, bar_norm) for one launch from fp32 parameters p0, with ``ref`` = adam_clip_ref(..., with_coef=True); the
    derivations are in the module docstring.  ``frac`` scales the counted parts (0.5: the half bars the fp32 emulation has to meet); the
    u |p0| of the parameter's own final rounding is a hard bound of one operation, reached whenever the update is small next to p, and is
    not scaled."""
    p0 = np.asarray(p0, dtype=np.float64)
    p_ref, _, v_ref, _, norm, aux = ref
    bar_m = frac * 8 * U * aux["m_abs"]
    bar_v = frac * 16 * U * aux["v_abs"]
    amp = np.where(v_ref > 0, aux["v_abs"] / np.where(v_ref > 0, v_ref, 1.0), 1.0) - 1.0
    bar_p = U * np.abs(p0) + frac * (16 * U * aux["upd_abs"] + 8 * U * amp * np.abs(p_ref - p0))
    act = aux["act"]                                       # inactive elements: untouched, bit for bit
    return np.where(act, bar_p, 0.0), np.where(act, bar_m, 0.0), np.where(act, bar_v, 0.0), frac * 2 * U * norm


def adam_inputs(rng, n, *, scale_p=0.1):
    """Teacher-forcing start state and one gradient: p ~ N(0, scale_p); moments as a history of clipped gradients of the recipe below leaves
    them: per element a magnitude a, log-uniform over [1e-12, 1e-3], m = +-a * U(0.1, 1), v = a^2 * U(0.5, 2) -- non-zero m, v > 0,
    |m| / sqrt(v) of order one, and sqrt(v) on both sides of eps, where the placement of eps and of the second bias correction shows."""
    p = (rng.normal(size=n) * scale_p).astype(np.float32)
    a = 10.0 ** rng.uniform(-12, -3, size=n)
    m = (a * rng.uniform(0.1, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    v = (a * a * rng.uniform(0.5, 2.0, size=n)).astype(np.float32)
    return p, adam_grad(rng, n), m, v


def adam_grad(rng, n, below=None):
    """Gradient of the trajectory recipe: magnitudes log-uniform over [1e-10, 1e-1], random signs, 2 % exact zeros; ``below``: scaled (in
    fp32) so that its norm is half of that value -- coef is then exactly 1."""
    g = 10.0 ** rng.uniform(-10, -1, size=n) * rng.choice([-1.0, 1.0], size=n)
    g[rng.random(n) < 0.02] = 0.0
    g = g.astype(np.float32)
    if below is not None:
        nrm = np.sqrt(np.sum(g.astype(np.float64) ** 2))
        if nrm > 0:
            g = (g * np.float32(0.5 * below / nrm)).astype(np.float32)
    return g


# ---- loss ---------------------------------------------------------------------------------------------------------------------------
def loss_ref(popcount, y, lam4, sreg, lam_weak, inv_B, stats):
    """pc_loss_block in float64 (the comment over it in csrc/common.h): l_b = lam0 |d| + lam1 |dl| + lam2 d^2 + lam3 dl^2 with d = pc - y,
    dl = log(pc + 1) - log(y + 1); loss = inv_B * sum l_b + reg; g_popcount[b] = lam_weak inv_B (lam0 sign(d) + lam1 sign(dl) / (pc + 1) +
    2 lam2 d + 2 lam3 dl / (pc + 1)), sign(0) = 0; reg = sreg * stats[1] / stats[0] and g_scale_const = lam_weak sreg / stats[0], both 0
    when sreg <= 0, stats is None or stats[0] == 0.  lam4 and the scalars are taken as fp32 values widened (the C ABI passes floats).
    Returns (loss, reg, g_popcount, g_scale_const)."""
    pc, y = np.asarray(popcount, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lam = [float(np.float32(x)) for x in lam4]
    sreg, lam_weak, inv_B = (float(np.float32(x)) for x in (sreg, lam_weak, inv_B))
    d = pc - y
    dl = np.log1p(pc) - np.log1p(y)
    l = lam[0] * np.abs(d) + lam[1] * np.abs(dl) + lam[2] * d * d + lam[3] * dl * dl
    g = lam[0] * np.sign(d) + lam[1] * np.sign(dl) / (pc + 1) + lam[2] * 2 * d + lam[3] * 2 * dl / (pc + 1)
    reg, gsc = 0.0, 0.0
    if stats is not None and sreg > 0 and float(stats[0]) > 0:
        reg = sreg * float(stats[1]) / float(stats[0])
        gsc = lam_weak * sreg / float(stats[0])
    return float(np.sum(l) * inv_B + reg), reg, lam_weak * inv_B * g, gsc


def loss_f32(popcount, y, lam4, sreg, lam_weak, inv_B, stats):
    """pc_loss_block in numpy float32, operation for operation (numpy's float32 log stands in for logf), double accumulation of the
    per-sample losses in the kernel's order: 256 strided partial sums, then the halving tree."""
    f = np.float32
    pc, y = np.asarray(popcount, dtype=f), np.asarray(y, dtype=f)
    lam = [f(x) for x in lam4]
    sreg, lam_weak, inv_B = f(sreg), f(lam_weak), f(inv_B)
    one, two = f(1), f(2)
    d = pc - y
    dl = np.log(pc + one).astype(f) - np.log(y + one).astype(f)
    sg, sgl = np.sign(d).astype(f), np.sign(dl).astype(f)
    l = ((lam[0] * np.abs(d) + lam[1] * np.abs(dl)).astype(f) + ((lam[2] * d).astype(f) * d).astype(f)).astype(f) \
        + ((lam[3] * dl).astype(f) * dl).astype(f)
    g = ((lam[0] * sg + (lam[1] * sgl / (pc + one)).astype(f)).astype(f) + ((lam[2] * two).astype(f) * d).astype(f)).astype(f) \
        + (((lam[3] * two).astype(f) * dl).astype(f) / (pc + one)).astype(f)
    gpc = (f(lam_weak * inv_B) * g).astype(f)
    red = np.zeros(256, dtype=np.float64)
    for t in range(256):
        red[t] = sum(float(x) for x in l[t::256])
    off = 128
    while off:
        red[:off] += red[off:2 * off]
        off >>= 1
    reg, gsc = 0.0, f(0)
    if stats is not None and sreg > 0 and float(stats[0]) > 0:
        reg = float(sreg) * float(stats[1]) / float(stats[0])
        gsc = f(float(lam_weak) * float(sreg) / float(stats[0]))
    return f(red[0] * float(inv_B) + reg), f(reg), gpc, gsc


def log_delta(popcount, y, ulp=LOGF_ULP):
    """Absolute error bound of the kernel's dl = logf(pc + 1) - logf(y + 1): each fp32 sum x + 1 carries u relative, which moves its log by
    u absolute; a logf of ``ulp`` units in the last place adds ulp * 2u |log|; the subtraction rounds once."""
    pc, y = np.asarray(popcount, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lp, ly = np.log1p(pc), np.log1p(y)
    return 2 * ulp * U * (np.abs(lp) + np.abs(ly)) + 2 * U + U * np.abs(lp - ly)


def loss_bars(popcount, y, lam4, sreg, lam_weak, inv_B, stats, ulp=LOGF_ULP, frac=1.0):
    """(bar_loss, bar_reg, bar_g_popcount[B], bar_g_scale_const) for pc_loss_block against loss_ref.

    Gradient: lam_weak inv_B (16 u sum_k |term_k| + lam3 * 2 delta / (pc + 1) + lam1 * [flip term]).  Count: term0 = lam0 sign(d) is exact;
    term1 = lam1 sign / (pc + 1): the sum pc + 1 and the divide, 2; term2 = lam2 * 2 * d: d and the product, 2 (lam2 * 2 is exact); term3
    = lam3 * 2 * dl / (pc + 1): the product, pc + 1, the divide, 3 (the error of dl itself is the delta term); three additions, each u on
    a partial sum that sum_k |term_k| bounds; lam_weak * inv_B and the final product, 2: 3 + 3 + 2 = 8, doubled 16.  The delta term is
    the worst case under the logf assumption and is not doubled.  The flip term 2 / (pc + 1) applies where 0 < |dl| <= delta, i.e. where
    fp32 could take the other sign; the test inputs keep |pc - y| >= 1e-2 max(y, 1), which puts |dl| three orders above delta, and plant
    ties as bit-equal values, where the kernel's d and dl are exactly 0.

    Loss value: 2 (inv_B sum_b e_b + u S) + inv_B sum_b (lam1 + 2 lam3 |dl|) delta with S = inv_B sum |l_b| + reg (the final rounding to float) and the per-sample count
    e_b = 2 u lam0 |d| (d, the product) + 4 u lam2 d^2 (d twice, two products) + u lam1 |dl| + 2 u lam3 dl^2 (the products)
    + 3 u l_b (three additions); the double accumulation adds nothing at this scale.
    Regulariser and g_scale_const: double arithmetic rounded once to float, u, doubled.
    ``frac`` scales the doubled counts (0.5: the half bars of the fp32 emulation); the delta terms are worst cases of their own -- 2 u of
    delta are the two roundings of pc + 1 and y + 1, which any fp32 evaluation makes -- and are not scaled."""
    pc, y = np.asarray(popcount, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lam = [abs(float(np.float32(x))) for x in lam4]
    lam_weak, inv_B = abs(float(np.float32(lam_weak))), float(np.float32(inv_B))
    loss, reg, _, gsc = loss_ref(popcount, y, lam4, sreg, lam_weak, inv_B, stats)
    d = np.abs(pc - y)
    dl = np.abs(np.log1p(pc) - np.log1p(y))
    delta = log_delta(pc, y, ulp)
    terms = lam[0] * np.sign(d) + lam[1] * np.sign(dl) / (pc + 1) + lam[2] * 2 * d + lam[3] * 2 * dl / (pc + 1)
    flip = np.where((dl > 0) & (dl <= delta), 2.0 / (pc + 1), 0.0)
    bar_g = lam_weak * inv_B * (frac * 16 * U * terms + lam[3] * 2 * delta / (pc + 1) + lam[1] * flip)
    l_abs = lam[0] * d + lam[1] * dl + lam[2] * d * d + lam[3] * dl * dl
    e = 2 * U * lam[0] * d + 4 * U * lam[2] * d * d + lam[1] * U * dl + lam[3] * 2 * U * dl * dl + 3 * U * l_abs
    e_delta = lam[1] * delta + lam[3] * 2 * dl * delta
    S = inv_B * float(np.sum(l_abs)) + abs(reg)
    bar_loss = frac * 2 * (inv_B * float(np.sum(e)) + U * S) + inv_B * float(np.sum(e_delta))
    return bar_loss, frac * 2 * U * abs(reg), bar_g, frac * 2 * U * abs(gsc)


def loss_inputs(rng, B, ties=10, y_zero=5, pc_zero=3):
    """pc and y log-uniform over [1e-2, 1e5] with every non-tie sample at |pc - y| >= 1e-2 max(y, 1) (redrawn until it holds, in fp32);
    then, as far as B allows, ``ties`` bit-equal pairs, ``y_zero`` samples with y = 0 and ``pc_zero`` with pc = 0 at distinct positions.
    Returns (pc, y, tie index array)."""
    def draw(k):
        return (10.0 ** rng.uniform(-2, 5, size=k)).astype(np.float32)
    pc, y = draw(B), draw(B)
    for _ in range(200):
        bad = np.abs(pc.astype(np.float64) - y) < 1e-2 * np.maximum(y.astype(np.float64), 1.0)
        if not bad.any():
            break
        pc[bad] = draw(int(bad.sum()))
    assert not (np.abs(pc.astype(np.float64) - y) < 1e-2 * np.maximum(y.astype(np.float64), 1.0)).any()
    order = rng.permutation(B)
    if B >= 256:
        first = list(dict.fromkeys([B - 1, 255, 0]))                                 # ties at the ends of the 256-thread stride
        order = np.concatenate([first, order[~np.isin(order, first)]]).astype(np.int64)
    k_t = min(ties, max(B - 1, 0)) if B > 1 else 0
    k_y = min(y_zero, max(B - k_t - 1, 0))
    k_p = min(pc_zero, max(B - k_t - k_y - 1, 0))
    ti, yi, pi = order[:k_t], order[k_t:k_t + k_y], order[k_t + k_y:k_t + k_y + k_p]
    y[ti] = pc[ti]
    y[yi] = 0.0
    pc[yi] = np.maximum(pc[yi], np.float32(1e-2))
    pc[pi] = 0.0
    y[pi] = np.maximum(y[pi], np.float32(1.0))           # |0 - y| >= 1e-2 max(y, 1) holds for every y > 0; keep y away from the tie with 0
    return pc, y, np.sort(ti)


# ---- popcount reduction -------------------------------------------------------------------------------------------------------------
def popcount_tpb(B):
    """Threads per sample of pc_popcount_sums_block: the largest power of two with tpb * B <= 256 (1 when B > 128)."""
    tpb = 1
    while 2 * tpb * B <= 256:
        tpb *= 2
    return tpb


def popcount_depth(B, H, W, nw):
    """Upper bound of the number of fp32 additions any pixel's term passes through on its way into popcount[b], from the chunk geometry of
    head_fwd_chunks (csrc/head.hip): a chunk is one workgroup of ``nw`` waves (8 in the split form, 4 in the fp32-MFMA form), a wave walks
    ``gpw`` groups of 16 pixels, lane i adding pixel i of each group in sequence (gpw additions), then one thread adds the 16 * nw lane
    sums of the workgroup in sequence; pc_popcount_sums_block adds every tpb-th chunk partial in sequence (at most nchunk) and finishes
    with a tree of log2(tpb) <= tpb levels.  gpw = max(8, ceil(groups / (nw * chunks))) depends on how many workgroups are resident, which
    the host decides; the bound takes its largest value (one chunk) and the largest nchunk = ceil(groups / (8 nw)).  The terms are
    non-negative, so the relative error of the sum is at most depth * u.  This is never above the plain sequential count
    (16 nw gpw + nchunk + tpb) for maps of up to 100 000 pixels."""
    groups = (H * W + 15) // 16
    gpw_max = max(8, -(-groups // nw))
    max_chunks = -(-groups // (8 * nw))
    return gpw_max + 16 * nw + max_chunks + popcount_tpb(B)
