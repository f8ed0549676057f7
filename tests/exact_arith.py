"""Exact-arithmetic known answers (CPU-only helper).

Every operand of a launch is a small dyadic number (an integer times a power of two), small enough that every partial sum a kernel
can form, in ANY order, is exactly representable in fp32.  Then the torch float64 reference is exact, every summation order gives the
same bits, ReLU decisions at exactly 0 are decided, and the bar is ``torch.equal`` on the whole tensor.  In bf16 mode the expected
value is the exact value rounded to nearest even at each rounding point of include/popcorn_hip.h (PC_PREC_BF16), again bit for bit.

The budget (``assert_budget``) is a condition, not a measurement: for every sum a kernel forms,
    sum |a_i * b_i| + |bias| + |prev|   (float64, on the operands' absolute values)
divided by the common quantum of its terms must be <= 2^22.  fp32 holds 2^24; the two bits of headroom are for the bf16 matrix
unit, whose internal summation width is not documented.  The budget is never raised to make a case fit: shrink the values.

Coverage conditions (``assert_bf16_coverage`` / ``assert_relu_coverage``), checked on the reference alone:
  bf16 activation output: >= 10 % of the non-zero expected elements differ from their unrounded value, >= 2 % are exact ties with
      an odd retained mantissa (RNE rounds them up) and >= 2 % exact ties with an even one (RNE rounds them down);
  ReLU: >= 0.5 % of the pre-activations are exactly 0."""
import torch
import torch.nn.functional as F

BUDGET = 2.0 ** 22
ODDS = (1, 3, 5, -1, -3)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- values -----------------------------------------------------------------------------------------------------------------------------

def ints(shape, lo, hi, g, density=1.0):
    """fp32 tensor of integers uniform in [lo, hi]; with density < 1 each element is kept with that probability, else 0"""
    v = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=g) < density).float()
    return v


def bn_odd(c, g, kmin=-2, kmax=1, shift=4, bias=2):
    """BN parameters whose folded scale is exactly odd * 2^k with (odd, k) distinct per channel: gamma = odd * 2^k, var = 1, eps = 0.0;
    mean, beta and the conv bias are integers in [-shift, shift] / [-bias, bias].  An odd factor does not commute with rounding, a
    power of two does: only the former can locate a rounding point.  Returns a dict of fp32 tensors + eps + the folded scale / shift
    (float64): y = conv * scale + shift."""
    pairs = [(o, k) for k in range(kmin, kmax + 1) for o in ODDS]
    assert c <= len(pairs)
    pick = torch.randperm(len(pairs), generator=g)[:c].tolist()
    odd = torch.tensor([pairs[i][0] for i in pick], dtype=torch.float32)
    k = torch.tensor([pairs[i][1] for i in pick], dtype=torch.float32)
    gamma = odd * torch.pow(torch.tensor(2.0), k)
    assert len({(float(o), float(e)) for o, e in zip(odd, k)}) == c
    d = dict(gamma=gamma, beta=ints((c,), -shift, shift, g), mean=ints((c,), -shift, shift, g), var=torch.ones(c), eps=0.0,
             bias=ints((c,), -bias, bias, g))
    d["scale"] = gamma.double()
    d["shift"] = (d["bias"].double() - d["mean"].double()) * d["scale"] + d["beta"].double()
    return d


def bn_apply(y, bn):
    """float64: the folded BN of common.h (pc_bn_fold) on a conv result WITHOUT its bias: y * scale + shift"""
    c = bn["scale"].numel()
    return y * bn["scale"].view(1, c, 1, 1) + bn["shift"].view(1, c, 1, 1)


def sig_bits(t):
    """number of significant bits of every element (0 for 0): position of the highest minus the lowest set bit + 1"""
    a = t.double().abs()
    q = _elem_quantum(a)
    n = torch.where(a > 0, torch.floor(torch.log2((a / q).clamp_min(1.0))) + 1, torch.zeros_like(a))
    return n


def _elem_quantum(a):
    """per element: the largest power of two that divides it (1.0 for 0)"""
    m, e = torch.frexp(a.double().abs())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return torch.where(mi != 0, low * torch.pow(torch.tensor(2.0, dtype=torch.double), (e - 53).double()), torch.ones_like(low))


def quantum(*tensors):
    """the common quantum of the tensors' non-zero elements: the largest power of two that divides every one of them"""
    q = float("inf")
    for t in tensors:
        t = torch.as_tensor(t).double()
        nz = t[t != 0]
        if nz.numel():
            q = min(q, float(_elem_quantum(nz).min()))
    return 1.0 if q == float("inf") else q


# ---- the budget -------------------------------------------------------------------------------------------------------------------------

def assert_budget(abs_sum, q, what=""):
    """abs_sum: float64 tensor, per output element the sum of the absolute values of every term behind it (products, bias, previous
    content of a += target); q: the common quantum of those terms.  sum / q <= 2^22, or the case is not exact by construction."""
    worst = float(torch.as_tensor(abs_sum).double().max()) / q
    assert worst <= BUDGET, "%s: %.4g quanta (2^%.2f) behind one element, the budget is 2^22" % (what, worst, torch.log2(torch.tensor(worst)).item())
    return worst


def _per_channel(s, q, scale, what):
    """s [B][C][H][W] absolute sums before the scale, q their quantum: each channel against the quantum of ITS scale"""
    qs = _elem_quantum(scale.double())
    worst = (s * scale.double().abs().view(1, -1, 1, 1)).amax((0, 2, 3)) / (q * qs)
    return assert_budget(worst, 1.0, what)


def budget_conv_fwd(x, w, bn=None, what="conv forward"):
    """x: the conv's input as torch sees it (after pooling / concat / reflect); returns the worst quanta count"""
    s = F.conv2d(x.double().abs(), w.double().abs(), padding=1)
    q = quantum(x) * quantum(w)
    if bn is None:
        return assert_budget(s, q, what)
    c = s.shape[1]
    qs = _elem_quantum(bn["scale"])
    s = (s + (bn["bias"].abs() + bn["mean"].abs()).double().view(1, c, 1, 1)) * bn["scale"].abs().view(1, c, 1, 1) + bn["beta"].abs().double().view(1, c, 1, 1)
    return assert_budget(s.amax((0, 2, 3)) / (min(q, 1.0) * torch.minimum(qs, torch.ones_like(qs))), 1.0, what)


def budget_dgrad(g, w, scale=None, prev=None, what="data gradient"):
    """w: the column block [cg][cn][3][3] of the weight; prev at the resolution of the product"""
    s = F.conv_transpose2d(g.double().abs(), w.double().abs(), padding=1)
    q = quantum(g) * quantum(w)
    qs = torch.ones(s.shape[1], dtype=torch.double)
    if scale is not None:
        s = s * scale.double().abs().view(1, -1, 1, 1)
        qs = _elem_quantum(scale.double())
    if prev is not None:
        s = s + prev.double().abs()
        q = min(q, quantum(prev))
    return assert_budget(s.amax((0, 2, 3)) / (q * torch.minimum(qs, torch.ones_like(qs))), 1.0, what)


def budget_wgrad(x, g, prev_w=None, prev_b=None, what="weight gradient"):
    co, ci = g.shape[1], x.shape[1]
    s = torch.nn.grad.conv2d_weight(x.double().abs(), (co, ci, 3, 3), g.double().abs(), padding=1)
    q = quantum(x) * quantum(g)
    sb = g.double().abs().sum((0, 2, 3))
    qb = quantum(g)
    if prev_w is not None:
        s, q = s + prev_w.double().abs(), min(q, quantum(prev_w))
    if prev_b is not None:
        sb, qb = sb + prev_b.double().abs(), min(qb, quantum(prev_b))
    return max(assert_budget(s, q, what + " dw"), assert_budget(sb, qb, what + " db"))


def budget_convt(x, w, bias, g=None, scale=None, what="transposed conv"):
    """forward, and with g the three gradients"""
    s = F.conv_transpose2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=2)
    worst = assert_budget(s, min(quantum(x) * quantum(w), quantum(bias)), what + " forward")
    if g is not None:
        sx = F.conv2d(g.double().abs(), w.double().abs(), stride=2)
        qx = quantum(g) * quantum(w)
        if scale is not None:
            sx, qx = sx * scale.abs().view(1, -1, 1, 1), qx * quantum(scale)
        worst = max(worst, assert_budget(sx, qx, what + " gx"))
        c = x.shape[1]
        sw = torch.einsum("bihw,bohpwq->iopq", x.double().abs(), g.double().abs().view(g.shape[0], c, x.shape[2], 2, x.shape[3], 2))
        worst = max(worst, assert_budget(sw, quantum(x) * quantum(g), what + " dw"))
        worst = max(worst, assert_budget(g.double().abs().sum((0, 2, 3)), quantum(g), what + " db"))
    return worst


# ---- bf16 rounding ----------------------------------------------------------------------------------------------------------------------

def rbf(x):
    """round to nearest even to bf16, returned in the dtype of x (the rounding of oracle/popcorn_oracle.py: _round_bf16)"""
    return x.to(torch.bfloat16).to(x.dtype)


def _bits(x):
    x32 = x.float()
    assert torch.equal(x32.double(), x.double()), "value is not an fp32 number"
    return x32.contiguous().view(torch.int32)


def rbf_trunc(x):
    """planted defect: truncation (the low 16 bits dropped) in place of RNE"""
    return (_bits(x) & -65536).view(torch.float32).to(x.dtype)


def rbf_half_up(x):
    """planted defect: round half away from zero (add 0x8000, truncate) in place of RNE"""
    return ((_bits(x) + 0x8000) & -65536).view(torch.float32).to(x.dtype)


def bf16_coverage(exact):
    """exact: the unrounded expected values (float64, each an fp32 number).  Shares among the elements whose ROUNDED value is non-zero:
    (rounded: differs from its unrounded value, tie_odd: exact tie with an odd retained mantissa, tie_even: with an even one)"""
    b = _bits(exact)
    nz = rbf(exact.float()) != 0
    n = max(int(nz.sum()), 1)
    low = b & 0xFFFF
    tie = low == 0x8000
    odd = ((b >> 16) & 1) == 1
    return (int(((low != 0) & nz).sum()) / n, int((tie & odd & nz).sum()) / n, int((tie & ~odd & nz).sum()) / n)


def assert_bf16_coverage(exact, what=""):
    r, to, te = bf16_coverage(exact)
    assert r >= 0.10 and to >= 0.02 and te >= 0.02, "%s: rounded %.3f (>= 0.10), odd ties %.3f, even ties %.3f (>= 0.02 each)" % (what, r, to, te)
    return r, to, te


def relu_coverage(pre):
    return float((pre == 0).double().mean())


def assert_relu_coverage(pre, what=""):
    z = relu_coverage(pre)
    assert z >= 0.005, "%s: %.4f of the pre-activations are exactly 0 (>= 0.005)" % (what, z)
    return z


# ---- references (torch float64 on the CPU) ----------------------------------------------------------------------------------------------

def ref_conv_fwd(x, w, bn=None, relu=True, bf16=False, pre=False):
    """x: the conv's input as torch sees it.  bf16: operands rounded where they are used (x, w), the output after the fp32 epilogue.
    pre: return the pre-activation (unrounded) too"""
    xd, wd = x.double(), w.double()
    if bf16:
        xd, wd = rbf(xd), rbf(wd)
    y = F.conv2d(xd, wd, padding=1)
    if bn is not None:
        y = bn_apply(y, bn)
    p = y
    if relu:
        y = torch.relu(y)
    out = rbf(y) if bf16 else y
    return (out, p) if pre else out


def ref_dgrad(g, w, c0, cn, act=None, scale=None, prev=None, bf16=False, ge=False):
    """data gradient of conv3x3 pad 1 for input channels [c0, c0 + cn), times relu'(act) * scale of the producing layer, (+ prev);
    bf16: ONE rounding, of the final value.  ge: the planted defect act >= 0"""
    wd = rbf(w.double()) if bf16 else w.double()
    gx = F.conv_transpose2d(g.double(), wd, padding=1)[:, c0:c0 + cn]
    if act is not None:
        gx = gx * ((act >= 0) if ge else (act > 0)).double()
    if scale is not None:
        gx = gx * scale.double().view(1, -1, 1, 1)
    if prev is not None:
        gx = gx + prev.double()
    return rbf(gx) if bf16 else gx


def ref_wgrad(x, g):
    """(dw, db) of conv3x3 pad 1; fp32 sums in either mode (no rounding point)"""
    co, ci = g.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), g.double(), padding=1), g.double().sum((0, 2, 3))


def ref_convt(x, w, bias, bf16=False):
    y = F.conv_transpose2d(x.double(), rbf(w.double()) if bf16 else w.double(), bias.double(), stride=2)
    return rbf(y) if bf16 else y


def ref_convt_bwd(x, w, g, act=None, scale=None, bf16=False):
    """(gx [masked and scaled with act / scale], dw, db) of ConvTranspose2d(2, stride 2)"""
    wd = rbf(w.double()) if bf16 else w.double()
    gx = F.conv2d(g.double(), wd, stride=2)
    if act is not None:
        gx = gx * (act > 0).double() * scale.double().view(1, -1, 1, 1)
    B, c, H, W = x.shape
    dw = torch.einsum("bihw,bohpwq->iopq", x.double(), g.double().view(B, c, H, 2, W, 2))
    return (rbf(gx) if bf16 else gx), dw, g.double().sum((0, 2, 3))


# ---- the head: Conv1x1(16, 64) ReLU Conv1x1(64, 64) ReLU Conv1x1(64, 64) ReLU Conv1x1(64, 2), relu, occupancy product -----------------

HEAD_NAMES = ["head.%d.%s" % (i, n) for i in (0, 2, 4, 6) for n in ("weight", "bias")]


def head_weights(g, density=(0.5, 0.25, 0.25, 0.5), wmax=(2, 1, 1, 1), bmax=(4, 8, 8, 8)):
    """integer head weights of the given density per layer; biases integers"""
    dims = [(64, 16), (64, 64), (64, 64), (2, 64)]
    out = []
    for (co, ci), d, wm, bm in zip(dims, density, wmax, bmax):
        out.append(ints((co, ci, 1, 1), -wm, wm, g, d))
        out.append(ints((co,), -bm, bm, g))
    return out


def head_chain(x, ht, bf16=False):
    """float64 forward of the head on pixel columns x [16][N]: returns (pre-activations of the three hidden layers and of output
    channel 0, hidden activations as the next layer reads them, scale = relu(out0)).  bf16: weights and the input are rounded where
    they are used, hidden layers after their ReLU (popcorn_hip.h)."""
    q = (lambda t: rbf(t)) if bf16 else (lambda t: t)
    h = q(x.double())
    pres, acts = [], [h]
    for l in range(3):
        p = q(ht[2 * l].double().view(ht[2 * l].shape[0], -1)) @ h + ht[2 * l + 1].double().view(-1, 1)
        pres.append(p)
        h = q(torch.relu(p))
        acts.append(h)
    p = (q(ht[6].double().view(2, -1)) @ h + ht[7].double().view(-1, 1))[0:1]
    pres.append(p)
    return pres, acts, torch.relu(p[0])


def head_backward(x, ht, g_out, bf16=False, ge=False, parts=False):
    """float64 backward of the chain for dL/d(scale) = g_out [N]: returns (8 gradients in HEAD_NAMES order, g_x [16][N]).  bf16: every
    gradient w.r.t. a product output is rounded after its ReLU mask, before it is used (oracle: _rb); the weight gradients are fp32
    sums of products of those rounded operands.  ge: the planted defect >= in the masks.  parts: also the masked gradient of each
    layer's pre-activation [g0, g1, g2, g3] as the products read them."""
    q = (lambda t: rbf(t)) if bf16 else (lambda t: t)
    pres, acts, _ = head_chain(x, ht, bf16)
    on = (lambda p: (p >= 0) if ge else (p > 0))
    grads, gs = [None] * 8, [None] * 4
    g = (g_out.double() * on(pres[3][0]).double()).view(1, -1)         # fp32 (the logits are not a bf16 tensor)
    gs[3] = g
    w6 = q(ht[6].double().view(2, -1))
    dw6 = torch.zeros(2, 64, dtype=torch.double)
    dw6[0] = (g @ acts[3].t())[0]
    grads[6], grads[7] = dw6.view(2, 64, 1, 1), torch.stack([g.sum(), torch.zeros((), dtype=torch.double)])
    g = w6[0:1].t() @ g
    for l in (2, 1, 0):
        g = q(g * on(pres[l]).double())
        gs[l] = g
        grads[2 * l] = (g @ acts[l].t()).view(ht[2 * l].shape)
        grads[2 * l + 1] = g.sum(1)
        g = q(ht[2 * l].double().view(ht[2 * l].shape[0], -1)).t() @ g
    return (grads, q(g), gs) if parts else (grads, q(g))


def budget_head(x, ht, g_out, bf16=False, what="head"):
    """every sum of the chain on the absolute values of ITS operands (a term that a ReLU has set to exactly 0 adds nothing): the four
    forward products + bias, the three backward products, the eight weight / bias gradient sums over the pixels"""
    _, acts, _ = head_chain(x, ht, bf16)
    _, _, gs = head_backward(x, ht, g_out, bf16, parts=True)
    qg = quantum(g_out)
    worst = 0.0
    for l in range(4):
        wl = ht[2 * l].double().abs().view(ht[2 * l].shape[0], -1)
        worst = max(worst, assert_budget(wl @ acts[l].abs() + ht[2 * l + 1].double().abs().view(-1, 1), 1.0, "%s layer %d" % (what, l)))
        worst = max(worst, assert_budget(gs[l].abs() @ acts[l].abs().t(), qg, "%s dW%d" % (what, 2 * l)))
        worst = max(worst, assert_budget(gs[l].abs().sum(1), qg, "%s db%d" % (what, 2 * l)))
        worst = max(worst, assert_budget((wl[0:1] if l == 3 else wl).t() @ gs[l].abs(), qg, "%s data gradient below layer %d" % (what, l)))
    return worst


# ---- the equality bar -------------------------------------------------------------------------------------------------------------------

def mismatch(got, expected):
    """None if equal bit for bit as values (NaN in got counts as different, -0 == +0), else 'count, first index, got, expected'"""
    g = got.detach().cpu()
    assert g.shape == expected.shape, (g.shape, expected.shape)
    e = expected.to(torch.float64)
    d = ~(g.to(torch.float64) == e)
    n = int(d.sum())
    if n == 0:
        return None
    idx = tuple(int(i) for i in torch.nonzero(d)[0])
    return "%d of %d elements differ, first at %s: got %r, expected %r" % (n, d.numel(), idx, float(g[idx]), float(e[idx]))


def assert_equal(got, expected, what=""):
    """whole-tensor equality with the exact reference: the reference must be an fp32 (bf16 container: bf16) number everywhere"""
    e = expected.to(torch.float64)
    assert torch.equal(e.to(got.dtype).to(torch.float64), e), what + ": the reference is not representable in the output's type"
    m = mismatch(got, e)
    assert torch.equal(got.detach().cpu().to(torch.float64), e) == (m is None)
    assert m is None, "%s: %s" % (what, m)
    print("[exact] %s: %d elements equal" % (what, e.numel()))


# ---- operand builders of the families (shared by the CPU self-tests and the GPU tests) --------------------------------------------------

X_RANGE, W_RANGE, G_RANGE = 8, 4, 32          # (gradients of the data-gradient families in [-32, 32]: the unscaled sums need rounding too)
# activations / gradients in [-8, 8], weights in [-4, 4]: bf16 numbers, sums far below the budget
WIDE = 2047                       # "wide" operand of the split forms: 9-12 significant bits (second / third piece non-empty)


def _xw(shape_x, shape_w, g, wide=None, xr=X_RANGE, wr=W_RANGE):
    if wide == "x":
        return ints(shape_x, -WIDE - 1, WIDE, g), ints(shape_w, -2, 2, g)
    if wide == "w":
        return ints(shape_x, -2, 2, g), ints(shape_w, -WIDE - 1, WIDE, g)
    return ints(shape_x, -xr, xr, g), ints(shape_w, -wr, wr, g)


def conv_fwd_case(loader, cin, cout, B, hw, seed, wide=None, bf16=False):
    """operands of one forward launch: {src: tensors the op takes, ref_in: the conv's input as torch sees it, w, bn, expected, pre}.
    loaders: plain | pool2 (source at 2H x 2W) | concat (16 + 16, the second smaller by one and placed at offset (1, 1)) | reflect
    (6-channel source, reflect pad 14, channel gather; integers of up to 9 bits, a fifth of which bf16 mode has to round)."""
    g = gen(seed)
    H, W = hw
    src = {}
    if loader == "plain":
        x, w = _xw((B, cin, H, W), (cout, cin, 3, 3), g, wide, xr=32 if cin < 8 else X_RANGE)
        src["a"] = x
    elif loader == "pool2":
        xs, w = _xw((B, cin, 2 * H, 2 * W), (cout, cin, 3, 3), g, wide)
        src["a"], x = xs, F.max_pool2d(xs, 2)
    elif loader == "concat":
        assert cin == 32
        skip, w = _xw((B, 16, H, W), (cout, 32, 3, 3), g, wide)
        up = ints((B, 16, H - 1, W - 1), -X_RANGE, X_RANGE, g)
        src["a"], src["b"], x = skip, up, torch.cat([skip, F.pad(up, (1, 0, 1, 0))], 1)
    else:
        assert loader == "reflect" and cin in (2, 4)
        X = ints((B, 6, H - 28, W - 28), -400, 400, g)
        w = ints((cout, cin, 3, 3), -2, 2, g)
        chmap = (4, 5, 0, 0) if cin == 2 else (2, 1, 0, 3)
        src["a"], src["chmap"] = X, chmap
        x = F.pad(X[:, list(chmap[:cin])], (14, 14, 14, 14), mode="reflect")
    bn = bn_odd(cout, g)
    if bf16:
        x = rbf(x)
    budget_conv_fwd(x, w, bn, "A %s %d->%d %s" % (loader, cin, cout, hw))
    exact, pre = ref_conv_fwd(x, w, bn, relu=True, pre=True)
    return dict(src=src, ref_in=x, w=w, bn=bn, exact=exact, pre=pre, expected=rbf(exact) if bf16 else exact)


def pooled_act(shape, g):
    """full-resolution activation whose 2 x 2 windows hold four DISTINCT values (4 v + position), mixed sign with exact zeros: the
    arg-max of a window is unique, and a window whose maximum is exactly 0 exists"""
    B, c, H2, W2 = shape
    v = ints(shape, -2, 1, g)
    bump = torch.tensor([[0.0, 1.0], [2.0, 3.0]]).repeat((H2 + 1) // 2, (W2 + 1) // 2)[:H2, :W2]
    return 4 * v + bump


def dgrad_case(cg, cin_total, c0, cn, B, hw, seed, pool=False, bf16=False, wide=None):
    """operands of the data gradient: g, w [cg][cin_total][3][3], act (mixed sign, exact zeros; pool: at twice the resolution with
    unique window maxima), bn (odd scales) of the producing layer, prev for the += form"""
    gg = gen(seed)
    H, W = hw
    g, w = _xw((B, cg, H, W), (cg, cin_total, 3, 3), gg, wide, xr=G_RANGE)
    bn = bn_odd(cn, gg)
    if pool:
        act = pooled_act((B, cn, 2 * H, 2 * W), gg)
        prev = ints((B, cn, 2 * H, 2 * W), -64, 64, gg)
    else:
        act = ints((B, cn, H, W), -3, 3, gg)
        prev = ints((B, cn, H, W), -64, 64, gg)
    assert_relu_coverage(act, "dgrad act")
    return dict(g=g, w=w, act=act, bn=bn, prev=prev)


def ref_dgrad_pool(g, w, c0, cn, act, scale, prev, bf16=False, ge=False):
    """gradient of conv(maxpool2(act)) scattered to the arg-max of every window, times relu'(act) * scale, + prev"""
    wd = rbf(w.double()) if bf16 else w.double()
    gx = F.conv_transpose2d(g.double(), wd, padding=1)[:, c0:c0 + cn].contiguous()
    H2, W2 = act.shape[2:]
    Hc, Wc = 2 * gx.shape[2], 2 * gx.shape[3]
    _, idx = F.max_pool2d(act[:, :, :Hc, :Wc].double(), 2, return_indices=True)
    full = torch.zeros(act.shape, dtype=torch.double)
    full[:, :, :Hc, :Wc] = F.max_unpool2d(gx, idx, 2, output_size=(Hc, Wc))
    full = full * ((act >= 0) if ge else (act > 0)).double() * scale.double().view(1, -1, 1, 1) + prev.double()
    return rbf(full) if bf16 else full


def wgrad_case(cin, cout, B, hw, seed):
    gg = gen(seed)
    H, W = hw
    return dict(x=ints((B, cin, H, W), -X_RANGE, X_RANGE, gg), g=ints((B, cout, H, W), -X_RANGE, X_RANGE, gg),
                prev_w=ints((cout, cin, 3, 3), -1000, 1000, gg), prev_b=ints((cout,), -1000, 1000, gg))


def convt_case(c, B, hw, seed):
    gg = gen(seed)
    H, W = hw
    d = dict(x=ints((B, c, H, W), -128, 127, gg), w=ints((c, c, 2, 2), -W_RANGE, W_RANGE, gg), bias=ints((c,), -4, 4, gg),
             g=ints((B, c, 2 * H, 2 * W), -G_RANGE, G_RANGE, gg), bn=bn_odd(c, gg))
    d["x"] = d["x"] * (torch.rand(d["x"].shape, generator=gg) < 0.95).float()          # exact zeros: x is the mask source of its data gradient
    budget_convt(d["x"], d["w"], d["bias"], d["g"], d["bn"]["scale"], "D convt C=%d %s" % (c, hw))
    assert_relu_coverage(d["x"], "convt x")
    return d


def head_case(shape, seed, wide=False, sparse=False, few_census=None):
    """operands of the head at (B, H, W, Hp, Wp, py, px): feat (B, 16, Hp, Wp) integers, the eight head tensors (integer weights of
    density 1/4 - 1/2), building in {0, 1, 2, 3}, admin mask / census index, the selection mask of the sparse form, and small integer
    upstream gradients on all four routes.  wide: features of 8 bits and very sparse deeper layers, so that the hidden units carry
    more than 8 significant bits (non-empty second pieces in the split form, roundings in bf16 mode)."""
    B, H, W, Hp, Wp, py, px = shape
    g = gen(seed)
    if wide is True:
        feat = ints((B, 16, Hp, Wp), -1024, 1023, g)
        ht = head_weights(g, density=(0.125, 2 / 64, 2 / 64, 4 / 64), wmax=(1, 1, 1, 1))
        for l in range(3):
            ht[2 * l + 1] = ints((64,), 256, 1024, g)
        ht[6].zero_()
        pick = torch.randperm(64, generator=g)[:4]
        ht[6][0, pick, 0, 0] = torch.tensor([1.0, 1.0, -1.0, -1.0])
    else:
        feat = ints((B, 16, Hp, Wp), -4, 4, g)
        ht = head_weights(g, density=(0.5, 0.25, 0.25, 0.25))
    building = ints((B, 1, H, W), 0, 3, g)
    admin = (torch.rand(B, H, W, generator=g) < (0.03 if wide is True else 0.6)).float() * 5.0
    census = torch.full((B,), 5, dtype=torch.int64)
    mask = (torch.rand(B, H, W, generator=g) < 0.5) if sparse else torch.ones(B, H, W, dtype=torch.bool)
    gd = 0.1 if wide is True else 0.25
    d = dict(feat=feat, ht=ht, building=building, admin=admin, census=census, mask=mask, sparse=sparse,
             g_pc=ints((B,), -2, 2, g), g_pd=ints((B, H, W), -1, 1, g, gd), g_sm=ints((B, H, W), -1, 1, g, gd), g_const=1.0)
    d["g_pc"][d["g_pc"] == 0] = 1.0
    if wide == "g":               # upstream gradients of 10 bits: the hidden gradients and g_feat need rounding in bf16 mode
        d["g_sm"] = ints((B, H, W), -300, 300, g, 0.35)
    # head.6.bias[0] centres the output on its median: the output decision takes both signs, and exact zeros where the values allow
    x = feat[:, :, py:py + H, px:px + W].permute(1, 0, 2, 3).reshape(16, -1)[:, mask.reshape(-1)]
    ht[7] = torch.zeros(2)
    ht[7][0] = -float(head_chain(x, ht)[0][3].median().round())
    return d


def head_reference(d, shape, bf16=False, ge=False):
    """float64 reference of ops.head_fwd / ops.head_bwd on a head_case: dict(scale_map, popdense, popcount, grads [8], g_feat (B, 16,
    Hp, Wp), pres: the pre-activations of the selected pixels [3 x (64, N), (1, N)], g_out)"""
    B, H, W, Hp, Wp, py, px = shape
    sel = d["mask"].reshape(-1)
    x = d["feat"][:, :, py:py + H, px:px + W].permute(1, 0, 2, 3).reshape(16, -1)[:, sel]
    pres, acts, scale = head_chain(x, d["ht"], bf16)
    smap = torch.zeros(B * H * W, dtype=torch.double)
    smap[sel] = scale
    smap = smap.view(B, H, W)
    bld = d["building"][:, 0].double()
    pd = smap * bld
    inunit = (d["admin"] == d["census"].view(-1, 1, 1).float()).double()
    pc = (pd * inunit).sum((1, 2))
    g_out = (d["g_pc"].double().view(B, 1, 1) * inunit * bld + d["g_pd"].double() * bld + d["g_sm"].double() + d["g_const"]).reshape(-1)[sel]
    grads, gx = head_backward(x, d["ht"], g_out, bf16, ge)
    gf = torch.zeros(16, B * H * W, dtype=torch.double)
    gf[:, sel] = gx
    g_feat = torch.zeros(B, 16, Hp, Wp, dtype=torch.double)
    g_feat[:, :, py:py + H, px:px + W] = gf.view(16, B, H, W).permute(1, 0, 2, 3)
    worst = budget_head(x, d["ht"], g_out, bf16)
    worst = max(worst, assert_budget((pd * inunit).abs().sum((1, 2)), 1.0, "head popcount"))
    return dict(scale_map=smap, popdense=pd, popcount=pc, grads=grads, g_feat=g_feat, pres=pres, acts=acts, g_out=g_out, worst=worst)


# ---- the cases the GPU tests run (tests/test_gpu_exact_arith.py); tests/test_exact_arith_cpu.py checks budget and coverage of each -------

PAIRS = [(8, 8), (8, 16), (16, 16), (16, 8)]
# family A, bf16 mode: (loader, cin, cout, B, (H, W))
A_BF16 = ([("plain", ci, co, 1, (37, 53)) for ci, co in PAIRS] + [("plain", ci, co, 3, (16, 32)) for ci, co in PAIRS] +
          [("plain", 8, 8, 2, (19, 35)), ("plain", 16, 16, 2, (20, 36)), ("pool2", 8, 16, 2, (20, 36)), ("concat", 32, 8, 2, (23, 35)),
           ("concat", 32, 8, 1, (37, 53)), ("reflect", 2, 8, 2, (58, 69)), ("reflect", 4, 8, 2, (58, 69))])
# family B, bf16 mode, the five cases of test_bf16_conv_backward_fused_op: name -> (gradient channels, x channels, cin_total, c0)
B_BF16_FUSED = {"plain_masked": (8, 8, 8, 0), "concat_up_half": (8, 8, 16, 8), "concat_skip_half_accumulate": (8, 8, 16, 0),
                "g8_x16_up_half_of_32": (8, 16, 32, 16), "g16_x16_masked": (16, 16, 16, 0)}
BF16_SHAPES = [(1, (37, 53)), (3, (16, 32)), (2, (20, 36))]
BF16_POOL_SHAPES = [(1, (37, 53)), (2, (40, 72))]                 # full resolution of the pool form
HEAD_SHAPES = [(1, 37, 29, 64, 64, 13, 17), (2, 100, 100, 128, 128, 14, 14)]
HEAD_SEED = 10
# (shape index, variant, sparse): the wide variants at the small geometry only (the budget of the weight-gradient sums over the pixels)
HEAD_CASES = [(0, False, False), (0, False, True), (0, True, False), (0, True, True), (0, "g", False), (0, "g", True), (1, False, False),
              (1, False, True)]


def fused_bwd_case(gc, xc, cin_total, c0, B, hw, seed, up_half=False, pool=False, wide=None):
    """operands of the fused backward of one conv layer for the column block [c0, c0 + xc): g, x (the mask source: mixed sign with
    exact zeros; up_half: smaller by one row and column, zero-padded at the end), w, bn of x's producer, prev; pool: hw is the FULL
    resolution (odd sizes: the last row / column is not pooled), x the pooled copy of ``act`` (unique window maxima)"""
    gg = gen(seed)
    H, W = (hw[0] // 2, hw[1] // 2) if pool else hw
    g, w = _xw((B, gc, H, W), (gc, cin_total, 3, 3), gg, wide, xr=G_RANGE)
    d = dict(g=g, w=w, bn=bn_odd(xc, gg))
    if pool:
        d["act"] = pooled_act((B, xc, hw[0], hw[1]), gg)
        d["x"] = F.max_pool2d(d["act"], 2)
        d["prev"] = ints((B, xc, hw[0], hw[1]), -64, 64, gg)
        d["xfull"] = d["x"]
    else:
        hx, wx = (H - 1, W - 1) if up_half else (H, W)
        d["x"] = ints((B, xc, hx, wx), -X_RANGE, X_RANGE, gg) if wide != "w" else ints((B, xc, hx, wx), -2, 2, gg)
        d["xfull"] = F.pad(d["x"], (0, W - wx, 0, H - hx))
        d["prev"] = ints((B, xc, H, W), -64, 64, gg)
    assert_relu_coverage(d["act"] if pool else d["x"], "fused backward mask source")
    return d


def fused_bwd_reference(d, c0, masked=True, acc=False, bf16=False, pool=False):
    """(gx, dw[:, c0:c0 + xc], db) float64; gx with the mask / scale of x's producer and (+ prev) as the flags say"""
    xc = d["x"].shape[1]
    scale = d["bn"]["scale"] if masked else None
    if pool:
        gx = ref_dgrad_pool(d["g"], d["w"], c0, xc, d["act"], d["bn"]["scale"], d["prev"], bf16)
        budget_dgrad(d["g"], d["w"][:, c0:c0 + xc], d["bn"]["scale"], F.max_pool2d(d["prev"].abs(), 2), "fused backward gx (pool)")      # (the largest |prev| of a window)
    else:
        gx = ref_dgrad(d["g"], d["w"], c0, xc, d["xfull"] if masked else None, scale, d["prev"] if acc else None, bf16)
        budget_dgrad(d["g"], d["w"][:, c0:c0 + xc], scale, d["prev"] if acc else None, "fused backward gx")
    dw, db = ref_wgrad(d["xfull"], d["g"])
    budget_wgrad(d["xfull"], d["g"], what="fused backward")
    return gx, dw, db


# ---- family E: the composed Up (conv3x3 over cat[skip, ConvTranspose2d(z)] computed from the low-resolution map) --------------------------

UP_GEOMS = [(8, (12, 16)), (16, (12, 16)), (8, (20, 72)), (16, (24, 136)), (8, (16, 64))]
UP_BWD = UP_GEOMS + [(8, (20, 136))]


def up_case(Cs, hw, seed, B=2, wide=None):
    """skip (B, Cs, H, W), z (B, Cs, H/2, W/2), w [8][2 Cs][3][3], wt [Cs][Cs][2][2], bt, bn of the output, z_bn (z's producer), G.
    The kernels compose w and wt first, so the budget is taken on the whole chain of absolute values: it bounds every regrouping.
    wide "x": z and skip of 12 bits; "w": w of 12 bits; the other operands in {-1, 0, 1}."""
    g = gen(seed)
    H, W = hw
    C = Cs
    if wide:
        big, one = (lambda s: ints(s, -WIDE - 1, WIDE, g)), (lambda s: ints(s, -1, 1, g, 4.0 / Cs))
        skip, z = (big if wide == "x" else one)((B, Cs, H, W)), (big if wide == "x" else one)((B, C, H // 2, W // 2))
        w, wt, bt = (big if wide == "w" else one)((8, Cs + C, 3, 3)), one((C, C, 2, 2)), ints((C,), -1, 1, g)
    else:
        skip, z = ints((B, Cs, H, W), -4, 4, g), ints((B, C, H // 2, W // 2), -4, 4, g)
        w, wt, bt = ints((8, Cs + C, 3, 3), -2, 2, g), ints((C, C, 2, 2), -2, 2, g), ints((C,), -2, 2, g)
    d = dict(skip=skip, z=z, w=w, wt=wt, bt=bt, bn=bn_odd(8, g), z_bn=bn_odd(C, g), G=ints((B, 8, H, W), -4, 4, g))
    up = F.conv_transpose2d(z.double().abs(), wt.double().abs(), bt.double().abs(), stride=2)
    budget_conv_fwd(torch.cat([skip.double().abs(), up], 1), w, d["bn"], "E up forward Cs=%d %s" % (Cs, hw))
    return d


def up_forward_reference(d, relu=True):
    up = F.conv_transpose2d(d["z"].double(), d["wt"].double(), d["bt"].double(), stride=2)
    y = bn_apply(F.conv2d(torch.cat([d["skip"].double(), up], 1), d["w"].double(), padding=1), d["bn"])
    return torch.relu(y) if relu else y


def _up_chain(z, w_up, wt, bt, G):
    zd, wd, wtd, btd = (t.double().clone().requires_grad_(True) for t in (z, w_up, wt, bt))
    F.conv2d(F.conv_transpose2d(zd, wtd, btd, stride=2), wd, padding=1).backward(G.double())
    return zd.grad, wd.grad, wtd.grad, btd.grad


def up_backward_reference(d):
    """(gz masked and scaled by z's producer, dw[:, Cs:], dwt, dbt) of the up-sampled half, float64 autograd; asserts the budget on
    the chain of absolute values"""
    Cs = d["skip"].shape[1]
    gz, dw, dwt, dbt = _up_chain(d["z"], d["w"][:, Cs:], d["wt"], d["bt"], d["G"])
    a = _up_chain(d["z"].abs(), d["w"][:, Cs:].abs(), d["wt"].abs(), d["bt"].abs(), d["G"].abs())
    _per_channel(a[0], 1.0, d["z_bn"]["scale"], "E up backward gz")
    for t, n in zip(a[1:], ("dw", "dwt", "dbt")):
        assert_budget(t, 1.0, "E up backward " + n)
    assert_relu_coverage(d["z"], "E up backward z")
    return gz * (d["z"] > 0).double() * d["z_bn"]["scale"].view(1, -1, 1, 1), dw, dwt, dbt


# ---- family F: the whole 32 x 32 level --------------------------------------------------------------------------------------------------

def level2_case(seed, B=2):
    """forward: x (B, 16, 32, 32) >= 0, two 16 -> 16 convs with BN + ReLU and the transposed conv; weights of density 1/4 in {-1, 0, 1}
    keep the three-stage chain inside the budget.  backward: g2, c1 (its sign is conv1's mask), act (B, 16, 64, 64) with unique window
    maxima, x = maxpool(act), prev"""
    g = gen(seed)
    d = dict(w1=ints((16, 16, 3, 3), -1, 1, g, 0.25), w2=ints((16, 16, 3, 3), -1, 1, g, 0.25), wt=ints((16, 16, 2, 2), -1, 1, g, 0.5),
             bt=ints((16,), -2, 2, g), bn1=bn_odd(16, g), bn2=bn_odd(16, g), abn=bn_odd(16, g),
             act=pooled_act((B, 16, 64, 64), g), g2=ints((B, 16, 32, 32), -4, 4, g), c1b=ints((B, 16, 32, 32), -3, 3, g),
             prev=ints((B, 16, 64, 64), -64, 64, g))
    d["x"] = F.max_pool2d(d["act"], 2)
    d["xf"] = ints((B, 16, 32, 32), 0, 32, g)
    return d


def level2_forward_reference(d, bf16=False):
    """(c1, c2, u2); bf16: every stage rounded once after its epilogue, the next stage reads the rounded value"""
    q = (lambda t: rbf(t)) if bf16 else (lambda t: t)
    x = d["xf"].double()
    budget_conv_fwd(x, d["w1"], d["bn1"], "F c1")
    c1 = q(torch.relu(bn_apply(F.conv2d(x, d["w1"].double(), padding=1), d["bn1"])))
    budget_conv_fwd(c1, d["w2"], d["bn2"], "F c2")
    c2 = q(torch.relu(bn_apply(F.conv2d(c1, d["w2"].double(), padding=1), d["bn2"])))
    assert_budget(F.conv_transpose2d(c2.abs(), d["wt"].double().abs(), d["bt"].double().abs(), stride=2), quantum(c2), "F u2")
    u2 = q(F.conv_transpose2d(c2, d["wt"].double(), d["bt"].double(), stride=2))
    return c1, c2, u2


def level2_backward_reference(d, bf16=False):
    """(out, dw1, db1, dw2, db2); bf16: the intermediate gradient g1 is rounded where the layer-wise launches store it"""
    q = (lambda t: rbf(t)) if bf16 else (lambda t: t)
    s1, sa = d["bn1"]["scale"], d["abn"]["scale"]
    budget_dgrad(d["g2"], d["w2"], s1, what="F g1")
    g1 = q(ref_dgrad(d["g2"], d["w2"], 0, 16, d["c1b"], s1))
    dw2, db2 = ref_wgrad(d["c1b"], d["g2"])
    budget_wgrad(d["c1b"], d["g2"], what="F dw2")
    dw1, db1 = ref_wgrad(d["x"], g1)
    budget_wgrad(d["x"], g1, what="F dw1")
    budget_dgrad(g1, d["w1"], sa, F.max_pool2d(d["prev"].abs(), 2), "F out")
    out = ref_dgrad_pool(g1, d["w1"], 0, 16, d["act"], sa, d["prev"], bf16)
    return out, dw1, db1, dw2, db2
