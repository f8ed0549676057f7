"""Single-product known answers for the fp32 matrix kernels (tests/single_product.py): the operands of every
launch are arranged so that each checked output element is exactly ONE product of two full-mantissa fp32 numbers (times exact
factors +-1 / 2^k), the torch float64 reference is then exact, and the bar is the arithmetic's own, per element:
2^-23 of the element for v_mfma_f32_16x16x4_f32, 2^-20 for the six-term sum of the split form.  Pattern P (permutation weights)
visits every (co, ci, tap) of a layer once over a family of launches; pattern S (sparse gradient) puts one non-zero per gradient
channel on corners, tile / strip seams and ragged last rows and columns, rotating the channels over the positions.
fp32 mode only.  Each test prints the worst |got - ref| / |ref| and the number of elements that differ from float32(ref64)."""
import pytest
import torch
import torch.nn.functional as F

from tests import single_product as SP

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(params=[1, 0], ids=["split", "fp32mfma"])
def conv_form(request):
    """pc_set_conv_split: 1 = split-operand kernels where they exist, 0 = v_mfma_f32_16x16x4_f32 everywhere; restored afterwards"""
    from popcorn_amd import _lib as L
    prev = L.lib().pc_set_conv_split(int(request.param))
    yield int(request.param)
    L.lib().pc_set_conv_split(prev)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn_dev(c):
    """(descriptor with exact 2^k scales, the scales)"""
    from popcorn_amd import _lib as L
    gamma, beta, mean, var, eps, scale = SP.bn_pow2(c)
    return L.bn(None, gamma.cuda(), beta.cuda(), mean.cuda(), var.cuda(), eps), scale.double()


def _fwd_form(split, cin, cout, W, direct=True):
    """conv3x3_fwd_s3.h: fwd_s3_ok -- the split-form forward takes one DIRECT source of 8 / 16 channels, 8 / 16 outputs, W % 4 == 0"""
    return "split" if split and direct and cin in (8, 16) and cout in (8, 16) and W % 4 == 0 else "fp32mfma"


def _finish(r, form, what):
    if form == "split":
        SP.assert_form_witness([r], what)
    return r


# =========================================================================================================================================
# Family A: conv forward
# =========================================================================================================================================

def _fwd_family(cin, cout, ref_in, problem, form, what, group_kw=None, seed=1, every=1):
    """the launches k = 0, every, 2 every, ... of the pattern-P family of a (cin -> cout) layer through ops.conv3x3_fwd_group;
    ref_in: the conv's input as torch sees it (after pooling / concat / reflect), CPU; problem(k): the source keys of launch k.
    2^k BN scales per output channel; ReLU on the even launches."""
    from popcorn_amd import ops
    fam = SP.pattern_p_family(cout, cin, _gen(seed), "forward")[::every]
    K = fam.shape[0]
    B, _, H, W = ref_in.shape
    bnd, scale = _bn_dev(cout)
    fam_d = fam.cuda()
    out = torch.full((K, B, cout, H, W), NAN, device="cuda")
    for k in range(K):
        ops.conv3x3_fwd_group([dict(problem(k), w=fam_d[k], bn=bnd, out=out[k])], relu=(k % 2 == 0), **(group_kw or {}))
    ref = F.conv2d(ref_in.double(), fam.reshape(K * cout, cin, 3, 3).double(), padding=1).view(B, K, cout, H, W).transpose(0, 1)
    ref = ref * scale.view(1, 1, cout, 1, 1)
    ref[0::2] = torch.relu(ref[0::2])
    return _finish(SP.assert_single_product(out, ref.contiguous(), form, what=what), form, what), out


PAIRS = [(8, 8), (8, 16), (16, 16), (16, 8)]


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_a_forward_every_triple_aligned(cin, cout, conv_form):
    """(20, 36): W % 4 == 0 (the split form / the staged loader), 2 x 2 tiles of 32 x 16, ragged last tiles"""
    x = torch.randn(2, cin, 20, 36, generator=_gen(100 + cin + cout))
    xd = x.cuda()
    form = _fwd_form(conv_form, cin, cout, 36)
    assert form == ("split" if conv_form else "fp32mfma")
    _fwd_family(cin, cout, x, lambda k: {"a": xd}, form, "A fwd %d->%d (20,36)" % (cin, cout))


@pytest.mark.parametrize("cin,cout", PAIRS + [(2, 8), (4, 8), (32, 8)])
def test_a_forward_every_triple_generic(cin, cout):
    """(19, 35): W % 4 != 0, the generic loader (fp32 MFMA in either form setting)"""
    x = torch.randn(2, cin, 19, 35, generator=_gen(120 + cin + cout))
    xd = x.cuda()
    _fwd_family(cin, cout, x, lambda k: {"a": xd}, "fp32mfma", "A fwd %d->%d (19,35)" % (cin, cout))


def test_a_forward_pool2_source(conv_form):
    """MaxPool2d(2) fused into the loader: source (40, 72), no ties"""
    from popcorn_amd import _lib as L
    xs = torch.randn(2, 8, 40, 72, generator=_gen(131))
    xd = xs.cuda()
    _fwd_family(8, 16, F.max_pool2d(xs, 2), lambda k: {"a": xd}, "fp32mfma", "A fwd pool2 8->16", {"a_mode": L.PC_SRC_POOL2})


def test_a_forward_concat_with_smaller_offset_b(conv_form):
    """cat[skip (23 x 35), up (22 x 34) placed at offset (1, 1)] (Up's zero F.pad): 16 + 16 -> 8"""
    skip = torch.randn(2, 16, 23, 35, generator=_gen(132))
    up = torch.randn(2, 16, 22, 34, generator=_gen(133))
    sd, ud = skip.cuda(), up.cuda()
    ref_in = torch.cat([skip, F.pad(up, (1, 0, 1, 0))], 1)
    _fwd_family(32, 8, ref_in, lambda k: {"a": sd, "b": ud}, "fp32mfma", "A fwd concat 16+16->8", {"b_offset": (1, 1)})


@pytest.mark.parametrize("lo,hi,chmap", [(0, 2, (4, 5, 0, 0)), (2, 6, (2, 1, 0, 3))])
def test_a_forward_reflect_and_channel_map(lo, hi, chmap, conv_form):
    """reflect padding (14) + channel gather fused into the first conv: source 30 x 41, out 58 x 69, both channel windows"""
    from popcorn_amd import _lib as L
    X = torch.randn(2, 6, 30, 41, generator=_gen(134))
    Xp = F.pad(X, (14, 14, 14, 14), mode="reflect")
    Xr = torch.cat([Xp[:, 4:6], torch.flip(Xp[:, :3], dims=(1,)), Xp[:, 3:4]], 1)
    Xd = X.cuda()
    cin = hi - lo
    _fwd_family(cin, 8, Xr[:, lo:hi].contiguous(), lambda k: {"a": Xd, "chmap": chmap}, "fp32mfma", "A fwd reflect %d->8" % cin,
                {"a_mode": L.PC_SRC_REFLECT, "a_pad": (14, 14), "out_hw": (58, 69), "a_channels": cin})


@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 16), (16, 16)])
def test_a_forward_pooled_second_output(cin, cout, conv_form):
    """(20, 64), the smallest shape pc_conv3x3_pool_out_ok takes: pool_out is bit-equal to max_pool2d of the checked output"""
    from popcorn_amd import ops
    x = torch.randn(2, cin, 20, 64, generator=_gen(140 + cin + cout))
    xd = x.cuda()
    pools = {}

    def problem(k):
        pools[k] = ops.pool_out_like(torch.empty(2, cout, 20, 64, device="cuda"))
        assert pools[k] is not None
        pools[k].fill_(NAN)
        return {"a": xd, "pool_out": pools[k]}

    form = _fwd_form(conv_form, cin, cout, 64)
    _, out = _fwd_family(cin, cout, x, problem, form, "A fwd pooled output %d->%d" % (cin, cout), every=3)
    for k, p in pools.items():
        assert torch.equal(p, F.max_pool2d(out[k], 2)), k


def test_a_forward_dot_epilogue_with_one_hot_dot_w(conv_form):
    """dot_w one-hot 1.0 at channel j: the one-channel map equals channel j of the single-product output; the other map channel stays"""
    from popcorn_amd import ops
    B, H, W = 2, 20, 36
    x = torch.randn(B, 8, H, W, generator=_gen(150))
    xd = x.cuda()
    fam = SP.pattern_p_family(8, 8, _gen(151), "forward")
    K = fam.shape[0]
    bnd, scale = _bn_dev(8)
    fam_d = fam.cuda()
    eye = torch.eye(8, device="cuda")
    maps = torch.full((K, B, 2, H, W), NAN, device="cuda")
    for k in range(K):
        ops.conv3x3_fwd_group([{"a": xd, "w": fam_d[k], "bn": bnd, "dot_w": eye[k % 8], "dot_out": maps[k][:, 1:2]}], relu=True)
    ref = F.conv2d(x.double(), fam.reshape(K * 8, 8, 3, 3).double(), padding=1).view(B, K, 8, H, W).transpose(0, 1)
    ref = torch.relu(ref * scale.view(1, 1, 8, 1, 1))
    ref = torch.stack([ref[k][:, k % 8] for k in range(K)])
    form = _fwd_form(conv_form, 8, 8, W)
    _finish(SP.assert_single_product(maps[:, :, 1], ref, form, what="A fwd dot epilogue"), form, "A fwd dot epilogue")
    assert bool(torch.isnan(maps[:, :, 0]).all())


@pytest.mark.parametrize("cin,cout,hw", [(8, 8, (20, 36)), (16, 16, (20, 36)), (8, 16, (19, 35)), (32, 8, (19, 35))])
def test_a_forward_bias_alone(cin, cout, hw, conv_form):
    """x = 0 with a full-mantissa bias and dense weights: the output is the bias, exactly"""
    from popcorn_amd import ops, _lib as L
    H, W = hw
    bias = SP.full_mantissa((cout,), _gen(160), scale=1.0)
    w = SP.full_mantissa((cout, cin, 3, 3), _gen(161))
    bd = bias.cuda()
    out = torch.full((2, cout, H, W), NAN, device="cuda")
    ops.conv3x3_fwd_group([{"a": torch.zeros(2, cin, H, W, device="cuda"), "w": w.cuda(), "bn": L.bn(bd), "out": out}], relu=False)
    assert torch.equal(out.cpu(), bias.view(1, cout, 1, 1).expand(2, cout, H, W))


# =========================================================================================================================================
# Family B: data gradient and fused backward
# =========================================================================================================================================

def _gx_reference(g, w):
    """float64 data gradient of conv3x3 pad 1: g [N][cg][H][W], w [cg][cin][3][3] -> [N][cin][H][W]"""
    return F.conv_transpose2d(g.double(), w.double(), padding=1)


def _stack_dgrad_family(fam):
    """[K][cg][cin][3][3] -> the weight [cg][K * cin][3][3] whose data gradient is the K launches' side by side"""
    K, cg, cin = fam.shape[:3]
    return fam.permute(1, 0, 2, 3, 4).reshape(cg, K * cin, 3, 3)


@pytest.mark.parametrize("cin_total,c0,cn,cg", [(8, 0, 8, 8), (16, 8, 8, 8), (32, 16, 16, 8), (8, 0, 8, 16), (16, 0, 16, 16)])
@pytest.mark.parametrize("hw", [(20, 36), (19, 35)])
def test_b_dgrad_plain_and_masked_accumulate_every_triple(cin_total, c0, cn, cg, hw):
    """pc_conv3x3_dgrad, pattern P over (co, tap) per input channel: plain into a NaN output, then masked (mixed-sign activation,
    2^k BN scales) += a dense previous value"""
    from popcorn_amd import ops
    B, (H, W) = 2, hw
    fam = SP.pattern_p_family(cg, cin_total, _gen(200 + cg + cin_total), "dgrad")
    K = fam.shape[0]
    g = torch.randn(B, cg, H, W, generator=_gen(201))
    gd, fam_d = g.cuda(), fam.cuda()
    ref = _gx_reference(g, _stack_dgrad_family(fam)).view(B, K, cin_total, H, W).transpose(0, 1)[:, :, c0:c0 + cn].contiguous()
    out = torch.full((K, B, cn, H, W), NAN, device="cuda")
    for k in range(K):
        ops.conv3x3_dgrad(gd, fam_d[k], c0, cn, out[k])
    SP.assert_single_product(out, ref, "fp32mfma", what="B dgrad plain cg=%d cin=%d %s" % (cg, cin_total, hw))
    act = torch.randn(B, cn, H, W, generator=_gen(202))
    bnd, scale = _bn_dev(cn)
    prev = torch.randn(K, B, cn, H, W, generator=_gen(203))
    out = prev.cuda()
    ad = act.cuda()
    for k in range(K):
        ops.conv3x3_dgrad(gd, fam_d[k], c0, cn, out[k], act=ad, act_bn=bnd, accumulate=True)
    ref = ref * (act > 0).double() * scale.view(1, 1, cn, 1, 1)
    SP.assert_single_product(out, ref, "fp32mfma", prev=prev, what="B dgrad masked += cg=%d cin=%d %s" % (cg, cin_total, hw))


@pytest.mark.parametrize("cn", [8, 16])
def test_b_dgrad_pool_scatter(cn):
    """pc_conv3x3_dgrad(pool=True): the gradient of conv(maxpool(act)) scattered (+=) to the arg-max of every 2 x 2 window of a
    (40, 72) activation without ties, times the ReLU / 2^k BN factor of its producer"""
    from popcorn_amd import ops
    B, H, W = 2, 20, 36
    fam = SP.pattern_p_family(16, cn, _gen(210 + cn), "dgrad")[::3]         # (every triple is visited by the plain test above)
    K = fam.shape[0]
    act = torch.randn(B, cn, 2 * H, 2 * W, generator=_gen(211))
    g = torch.randn(B, 16, H, W, generator=_gen(212))
    _, idx = F.max_pool2d(act.double(), 2, return_indices=True)
    gxp = _gx_reference(g, _stack_dgrad_family(fam)).view(B, K, cn, H, W)
    bnd, scale = _bn_dev(cn)
    ref = torch.stack([F.max_unpool2d(gxp[:, k].contiguous(), idx, 2, output_size=(2 * H, 2 * W)) for k in range(K)])
    ref = ref * (act > 0).double() * scale.view(1, 1, cn, 1, 1)
    prev = torch.randn(K, B, cn, 2 * H, 2 * W, generator=_gen(213))
    out = prev.cuda()
    gd, fam_d, ad = g.cuda(), fam.cuda(), act.cuda()
    for k in range(K):
        ops.conv3x3_dgrad(gd, fam_d[k], 0, cn, out[k], act=ad, act_bn=bnd, pool=True, accumulate=True)
    SP.assert_single_product(out, ref, "fp32mfma", prev=prev, what="B dgrad pool scatter cn=%d" % cn)


# the fused backward (WgradBatch.conv3x3_bwd_group): name -> (gradient channels, input channels of the layer, first column c0, column
# blocks as c0_add, masked, accumulate, pool scatter, needs the split form)
FUSED = {
    "8_plain": (8, 8, 0, (0,), False, False, False, False),                 # conv3x3_bwd_s3_kernel<8, false> / the fp32-MFMA kernel
    "8_masked_accumulate": (8, 8, 0, (0,), True, True, False, False),
    "8_concat_up_half": (8, 16, 8, (0,), False, False, False, False),       # c0 = 8 of 16: the other columns of dw stay
    "8_concat_both_blocks": (8, 16, 0, (0, 8), True, False, False, False),  # two problems with c0_add
    "16_both_blocks": (16, 16, 0, (0, 8), True, False, False, True),        # <16, false>
    "8_pool": (8, 8, 0, (0,), True, True, True, True),                      # <8, true>
    "16_pool": (16, 8, 0, (0,), True, True, True, True),                    # <16, true>
}
ROW_SEAMS, COL_SEAMS = (4, 16, 32), (32, 64)


def _fused_cases(geoms):
    out = []
    for form in (1, 0):
        for name, spec in FUSED.items():
            if spec[7] and not form:
                continue                                                    # these instantiations exist in the split form only
            for hw in geoms:
                if hw != (20, 36) and name not in ("8_plain", "16_both_blocks"):
                    continue
                out.append(pytest.param(form, name, hw, id="%s-%s-%dx%d" % ("split" if form else "fp32mfma", name, hw[0], hw[1])))
    return out


def _run_fused(form, name, hw, pattern):
    from popcorn_amd import ops, _lib as L
    cg, cin_total, c0, blocks, masked, acc, pool, _ = FUSED[name]
    B, (H, W) = 2, hw
    fname = "split" if form else "fp32mfma"
    gen = _gen(300 + 7 * cg + cin_total + H)
    if pool:
        act = torch.randn(B, 8, 2 * H, 2 * W, generator=gen)                # mixed sign, no ties
        x_full, idx = F.max_pool2d(act, 2, return_indices=True)
    else:
        x_full = torch.randn(B, cin_total, H, W, generator=gen)
    if pattern == "P":
        ws = SP.pattern_p_family(cg, cin_total, gen, "dgrad")
        n = ws.shape[0]
        gs = torch.randn(1, B, cg, H, W, generator=gen).expand(n, B, cg, H, W)
        places, req = None, None
    else:
        req = SP.required_positions(H, W, ROW_SEAMS, COL_SEAMS)
        gs, places = SP.pattern_s_gradients(B, H, W, cg, SP.pattern_s_groups(B, H, W, cg, req), gen)
        SP.assert_every_channel_visits(places, req, cg)
        n = gs.shape[0]
        ws = SP.full_mantissa((1, cg, cin_total, 3, 3), gen).expand(n, cg, cin_total, 3, 3)
    nb = len(blocks)
    Ho, Wo = (2 * H, 2 * W) if pool else (H, W)
    prev = torch.randn(n, B, 8 * nb, Ho, Wo, generator=gen) if acc else None
    out = prev.cuda() if acc else torch.full((n, B, 8 * nb, Ho, Wo), NAN, device="cuda")
    dw = torch.full((n, cg, cin_total, 3, 3), 7.0, device="cuda")
    db = torch.full((n, cg), NAN, device="cuda")
    bns = [_bn_dev(8) for _ in blocks]
    prev_form = L.lib().pc_set_conv_split(form)
    try:
        gs_d = (gs if pattern == "S" else gs[:1]).contiguous().cuda()          # (the operand that does not vary is uploaded once)
        ws_d = (ws if pattern == "P" else ws[:1]).contiguous().cuda()
        x_d = x_full.cuda()
        act_d = act.cuda() if pool else None
        for l in range(n):
            g_l = gs_d[l] if pattern == "S" else gs_d[0]
            w_l = ws_d[l] if pattern == "P" else ws_d[0]
            probs = []
            for i, blk in enumerate(blocks):
                pr = {"g": g_l, "x": x_d[:, c0 + blk:c0 + blk + 8], "w": w_l, "out": out[l][:, 8 * i:8 * i + 8], "dw": dw[l],
                      "db": db[l] if i == 0 else None, "c0_add": blk, "x_bn": bns[i][0] if masked else None}
                if pool:
                    pr["pool_act"] = act_d
                probs.append(pr)
            wb = ops.WgradBatch(torch.device("cuda"))
            wb.conv3x3_bwd_group(probs, cin_total, c0, accumulate=acc)
            wb.finish()
        torch.cuda.synchronize()
    finally:
        L.lib().pc_set_conv_split(prev_form)
    # ---- data gradient
    if pattern == "P":
        gx = _gx_reference(gs[0], _stack_dgrad_family(ws)).view(B, n, cin_total, H, W).transpose(0, 1)
    else:
        gx = _gx_reference(gs.reshape(n * B, cg, H, W), ws[0]).view(n, B, cin_total, H, W)
        assert float(SP.products_per_output_dgrad(gs[0], ws[0]).max()) <= 1.0
    cols = [c0 + blk + j for blk in blocks for j in range(8)]
    gx = gx[:, :, cols]
    if pool:
        gx = torch.stack([F.max_unpool2d(gx[l].contiguous(), idx, 2, output_size=(Ho, Wo)) for l in range(n)])
        mask_src = act
    else:
        mask_src = x_full[:, cols]
    if masked:
        scale = torch.cat([s for _, s in bns]).view(1, 1, -1, 1, 1)
        gx = gx * (mask_src > 0).double() * scale
    what = "B fused %s pattern %s %s [%s]" % (name, pattern, hw, fname)
    res = [SP.assert_single_product(out, gx.contiguous(), fname, prev=prev, what=what + " gx")]
    # ---- weight and bias gradient (pattern S: one product each)
    if pattern == "S":
        xw = x_full[:, cols].double()
        rdw = torch.stack([torch.nn.grad.conv2d_weight(xw, (cg, len(cols), 3, 3), gs[l].double(), padding=1) for l in range(n)])
        assert float(SP.products_per_output_wgrad(x_full[:, cols], gs[0]).max()) <= 1.0
        lo, hi = min(cols), max(cols) + 1
        res.append(SP.assert_single_product(dw[:, :, lo:hi], rdw, fname, what=what + " dw"))
        rest = [c for c in range(cin_total) if not lo <= c < hi]
        assert bool((dw[:, :, rest] == 7.0).all())
        r = SP.assert_single_product(db, gs.double().sum((1, 3, 4)), "fp32mfma", what=what + " db")
        assert r.differing == 0
    if form:
        SP.assert_form_witness(res, what)
    return places, req


@pytest.mark.parametrize("form,name,hw", _fused_cases([(20, 36)]))
def test_b_fused_backward_every_triple(form, name, hw):
    """pattern P: every (co, ci, tap) of the layer behind one data-gradient element once, over all pixels"""
    _run_fused(form, name, hw, "P")


@pytest.mark.parametrize("form,name,hw", _fused_cases([(20, 36), (36, 68)]))
def test_b_fused_backward_sparse_gradient(form, name, hw):
    """pattern S: gx, dw and db together; the non-zeros sit on the corners, both sides of the strip (3|4), tile (15|16, 31|32) seams,
    their crossings and the ragged last row / column -- (36, 68) is a 3 x 3 grid of tiles -- and every channel visits each of them"""
    places, req = _run_fused(form, name, hw, "S")
    H, W = hw
    for p in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (3, 31), (4, 32), (15, 31), (16, 32), (H - 1, 31), (3, W - 1)]:
        assert p in req
    print("B pattern S positions %s: rows %s x columns %s" % (hw, sorted({y for y, _ in req}), sorted({x for _, x in req})))


# =========================================================================================================================================
# Family C: weight gradient alone
# =========================================================================================================================================

def _wgrad_family(cin, cout, hw, call, x_ref, what, seed=400, accumulate=False):
    """pattern S through ops.conv3x3_wgrad; call(g, dw, db) launches; x_ref: the conv's input as torch sees it"""
    B, (H, W) = 2, hw
    gen = _gen(seed + cin + cout)
    req = SP.required_positions(H, W, ROW_SEAMS, COL_SEAMS)
    gs, places = SP.pattern_s_gradients(B, H, W, cout, SP.pattern_s_groups(B, H, W, cout, req), gen)
    SP.assert_every_channel_visits(places, req, cout)
    n = gs.shape[0]
    prev_w = torch.randn(n, cout, cin, 3, 3, generator=gen) if accumulate else None
    prev_b = torch.randn(n, cout, generator=gen) if accumulate else None
    dw = prev_w.cuda() if accumulate else torch.full((n, cout, cin, 3, 3), NAN, device="cuda")
    db = prev_b.cuda() if accumulate else torch.full((n, cout), NAN, device="cuda")
    gs_d = gs.cuda()
    for l in range(n):
        call(gs_d[l], dw[l], db[l])
    assert float(SP.products_per_output_wgrad(x_ref, gs[0]).max()) <= 1.0
    rdw = torch.stack([torch.nn.grad.conv2d_weight(x_ref.double(), (cout, cin, 3, 3), gs[l].double(), padding=1) for l in range(n)])
    SP.assert_single_product(dw, rdw, "fp32mfma", prev=prev_w, what=what + " dw")
    r = SP.assert_single_product(db, gs.double().sum((1, 3, 4)), "fp32mfma", prev=prev_b, what=what + " db")
    assert accumulate or r.differing == 0
    print(what, "positions: rows %s x columns %s" % (sorted({y for y, _ in req}), sorted({x for _, x in req})))
    return req


@pytest.mark.parametrize("cin,cout", PAIRS + [(2, 8), (4, 8), (32, 8)])
@pytest.mark.parametrize("hw", [(20, 36), (19, 35)], ids=["wave", "generic"])
def test_c_wgrad_sparse_gradient(cin, cout, hw):
    """WgradBatch.conv3x3: (20, 36) the wave kernels, (19, 35) the generic workgroup-tile kernel; every dw element is g[co, p] *
    x[ci, p + tap - 1] (0 outside the image), db[co] = g[co, p]"""
    from popcorn_amd import ops
    x = torch.randn(2, cin, *hw, generator=_gen(410 + cin))
    xd = x.cuda()
    _wgrad_family(cin, cout, hw, lambda g, dw, db: ops.conv3x3_wgrad(xd, g, cout, dw=dw, db=db), x, "C wgrad %d->%d %s" % (cin, cout, hw))


def test_c_wgrad_accumulate():
    from popcorn_amd import ops
    x = torch.randn(2, 8, 20, 36, generator=_gen(420))
    xd = x.cuda()
    _wgrad_family(8, 8, (20, 36), lambda g, dw, db: ops.conv3x3_wgrad(xd, g, 8, dw=dw, db=db, accumulate=True), x, "C wgrad += 8->8",
                  accumulate=True)


def test_c_wgrad_fused_loaders():
    """POOL2 source (40, 72); concat with a smaller, offset b; REFLECT + chmap"""
    from popcorn_amd import ops, _lib as L
    xs = torch.randn(2, 8, 40, 72, generator=_gen(430))
    xd = xs.cuda()
    _wgrad_family(8, 16, (20, 36), lambda g, dw, db: ops.conv3x3_wgrad(xd, g, 16, dw=dw, db=db, a_mode=L.PC_SRC_POOL2),
                  F.max_pool2d(xs, 2), "C wgrad pool2 8->16")
    skip, up = torch.randn(2, 16, 23, 35, generator=_gen(431)), torch.randn(2, 16, 22, 34, generator=_gen(432))
    sd, ud = skip.cuda(), up.cuda()
    _wgrad_family(32, 8, (23, 35), lambda g, dw, db: ops.conv3x3_wgrad(sd, g, 8, dw=dw, db=db, b=ud, b_offset=(1, 1)),
                  torch.cat([skip, F.pad(up, (1, 0, 1, 0))], 1), "C wgrad concat 16+16->8")
    X = torch.randn(2, 6, 30, 41, generator=_gen(433))
    Xp = F.pad(X, (14, 14, 14, 14), mode="reflect")
    Xr = torch.cat([Xp[:, 4:6], torch.flip(Xp[:, :3], dims=(1,)), Xp[:, 3:4]], 1)
    Xd = X.cuda()
    for lo, hi, chmap in [(0, 2, (4, 5, 0, 0)), (2, 6, (2, 1, 0, 3))]:
        cin = hi - lo
        # (dw is sized from a_channels, the source's own channel count is not the conv's)
        _wgrad_family(cin, 8, (58, 69), lambda g, dw, db: ops.conv3x3_wgrad(Xd, g, 8, dw=dw, db=db, a_mode=L.PC_SRC_REFLECT, a_pad=(14, 14),
                                                                            chmap=chmap, a_channels=cin),
                      Xr[:, lo:hi].contiguous(), "C wgrad reflect %d->8" % cin)


# =========================================================================================================================================
# Family D: transposed conv
# =========================================================================================================================================

@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("hw", [(9, 21), (16, 32)])
def test_d_convt_forward_every_weight_and_bias_alone(c, hw):
    """pattern P: one input channel per (co, sub-pixel); c launches visit every (ci, co, sub-pixel).  Then x = 0: out is the bias."""
    from popcorn_amd import ops
    B, (H, W) = 2, hw
    x = torch.randn(B, c, H, W, generator=_gen(500 + c))
    fam = torch.stack([SP.pattern_p_convt(c, k, _gen(501 + k)) for k in range(c)])
    assert bool(((fam != 0).sum(0) == 1).all())
    xd, fam_d, zero = x.cuda(), fam.cuda(), torch.zeros(c, device="cuda")
    out = torch.full((c, B, c, 2 * H, 2 * W), NAN, device="cuda")
    for k in range(c):
        ops.convt2x2(xd, fam_d[k], zero, out=out[k])
    ref = torch.stack([F.conv_transpose2d(x.double(), fam[k].double(), stride=2) for k in range(c)])
    r = SP.assert_single_product(out, ref, "fp32mfma", what="D convt fwd C=%d %s" % (c, hw))
    assert r.n == ref.numel()
    bias = SP.full_mantissa((c,), _gen(502), scale=1.0)
    o = torch.full((B, c, 2 * H, 2 * W), NAN, device="cuda")
    ops.convt2x2(torch.zeros_like(xd), SP.full_mantissa((c, c, 2, 2), _gen(503)).cuda(), bias.cuda(), out=o)
    assert torch.equal(o.cpu(), bias.view(1, c, 1, 1).expand(B, c, 2 * H, 2 * W))


def _convt_sparse(c, hw, seed):
    B, (H, W) = 2, hw
    gen = _gen(seed)
    req = SP.required_positions(2 * H, 2 * W, (2, 8), (32,))           # output rows 1|2 (input rows 0|1), 7|8; a 16-input-pixel column group
    gs, places = SP.pattern_s_gradients(B, 2 * H, 2 * W, c, SP.pattern_s_groups(B, 2 * H, 2 * W, c, req), gen)
    SP.assert_every_channel_visits(places, req, c)
    print("D convt C=%d %s positions (output grid): rows %s x columns %s" % (c, hw, sorted({y for y, _ in req}), sorted({x for _, x in req})))
    x = torch.randn(B, c, H, W, generator=gen)
    w = SP.full_mantissa((c, c, 2, 2), gen)
    refs = [SP.ref_convt_bwd(x, w, gs[l]) for l in range(gs.shape[0])]
    return x, w, gs, [torch.stack([r[i] for r in refs]) for i in range(3)]


@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("hw", [(9, 21), (16, 32)])
def test_d_convt_dgrad_and_wgrad_sparse_gradient(c, hw):
    """pattern S on the (2H, 2W) gradient: gx[ci, y, x] = g[co, p] w[ci, co, sub(p)] (masked: mixed-sign activation, 2^k scales),
    dw[ci, co, sub] = x[ci, p / 2] g[co, p] for the sub-pixel of p and 0 for the others, db[co] = g[co, p]"""
    from popcorn_amd import ops
    B, (H, W) = 2, hw
    x, w, gs, (rgx, rdw, rdb) = _convt_sparse(c, hw, 510 + c)
    n = gs.shape[0]
    xd, wd, gd = x.cuda(), w.cuda(), gs.cuda()
    bnd, scale = _bn_dev(c)
    gx = torch.full((n, B, c, H, W), NAN, device="cuda")
    gxm = torch.full((n, B, c, H, W), NAN, device="cuda")
    dw, db = torch.full((n, c, c, 2, 2), NAN, device="cuda"), torch.full((n, c), NAN, device="cuda")
    for l in range(n):
        ops.convt2x2_dgrad(gd[l], wd, gx[l])
        ops.convt2x2_dgrad(gd[l], wd, gxm[l], act=xd, act_bn=bnd)
        ops.convt2x2_wgrad(xd, gd[l], dw=dw[l], db=db[l])
    what = "D convt C=%d %s" % (c, hw)
    SP.assert_single_product(gx, rgx, "fp32mfma", what=what + " dgrad")
    SP.assert_single_product(gxm, rgx * (x > 0).double() * scale.view(1, 1, c, 1, 1), "fp32mfma", what=what + " dgrad masked")
    SP.assert_single_product(dw, rdw, "fp32mfma", what=what + " dw")
    assert SP.assert_single_product(db, rdb, "fp32mfma", what=what + " db").differing == 0


@pytest.mark.parametrize("c", [8, 16])
def test_d_convt_fused_backward_sparse_gradient(c):
    """WgradBatch.convt2x2_bwd_group at (16, 32), the fused form's aligned rows: gx (masked), dw, db of one launch"""
    from popcorn_amd import ops
    B, H, W = 2, 16, 32
    x, w, gs, (rgx, rdw, rdb) = _convt_sparse(c, (H, W), 520 + c)
    n = gs.shape[0]
    xd, wd, gd = x.cuda(), w.cuda(), gs.cuda()
    bnd, scale = _bn_dev(c)
    gx = torch.full((n, B, c, H, W), NAN, device="cuda")
    dw, db = torch.full((n, c, c, 2, 2), NAN, device="cuda"), torch.full((n, c), NAN, device="cuda")
    for l in range(n):
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.convt2x2_bwd_group([{"x": xd, "g": gd[l], "w": wd, "out": gx[l], "dw": dw[l], "db": db[l], "x_bn": bnd}])
        wb.finish()
    what = "D convt fused C=%d" % c
    SP.assert_single_product(gx, rgx * (x > 0).double() * scale.view(1, 1, c, 1, 1), "fp32mfma", what=what + " gx masked")
    SP.assert_single_product(dw, rdw, "fp32mfma", what=what + " dw")
    assert SP.assert_single_product(db, rdb, "fp32mfma", what=what + " db").differing == 0


# =========================================================================================================================================
# Family E: composed Up (forward)
# =========================================================================================================================================

UP_GEOMS = [(8, (12, 16), 1), (16, (12, 16), 1), (8, (20, 72), 4), (16, (24, 136), 8), (8, (16, 64), 4)]


@pytest.mark.parametrize("Cs,hw,every", UP_GEOMS)
def test_e_up_forward_every_triple(Cs, hw, every, conv_form):
    """conv3x3(cat[skip, ConvTranspose2d(z)]) from the low-resolution map: Wt signed one-hot (+-1.0, one input channel per (c,
    sub-pixel)), W on pattern P over all Cs + C input channels, bt = 0 -- every y element is skip * w or +-z * w, times 2^k.  Every
    triple at (12, 16), the smallest geometry the kernel takes; every ``every``-th launch of the family at the larger ones (two column
    tiles of the 128 template with a ragged last tile; the 64 template)."""
    from popcorn_amd import ops
    B, (H, W), Cz = 2, hw, Cs
    gen = _gen(600 + Cs + H)
    skip = torch.randn(B, Cs, H, W, generator=gen)
    z = torch.randn(B, Cz, H // 2, W // 2, generator=gen)
    fam = SP.pattern_p_family(8, Cs + Cz, gen, "forward")[::every]
    K = fam.shape[0]
    wts = torch.stack([SP.pattern_p_convt(Cz, k, gen, one_hot=True) for k in range(Cz)])
    bnd, scale = _bn_dev(8)
    sd, zd, fam_d, wts_d, bt = skip.cuda(), z.cuda(), fam.cuda(), wts.cuda(), torch.zeros(Cz, device="cuda")
    out = torch.full((K, B, 8, H, W), NAN, device="cuda")
    assert ops.conv3x3_up_fwd_ok(sd, zd, out[0])
    for k in range(K):
        ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd, "w": fam_d[k], "wt": wts_d[k % Cz], "bt": bt, "bn": bnd, "out": out[k]}], relu=(k % 2 == 0))
    us = [F.conv_transpose2d(z.double(), wts[j].double(), stride=2) for j in range(Cz)]
    ref = torch.stack([F.conv2d(torch.cat([skip.double(), us[k % Cz]], 1), fam[k].double(), padding=1) for k in range(K)])
    ref = ref * scale.view(1, 1, 8, 1, 1)
    ref[0::2] = torch.relu(ref[0::2])
    form = "split" if conv_form else "fp32mfma"
    what = "E up fwd Cs=%d %s" % (Cs, hw)
    _finish(SP.assert_single_product(out, ref, form, what=what), form, what)


@pytest.mark.parametrize("Cs,hw", [(8, (12, 16)), (16, (12, 16)), (8, (20, 72))])
def test_e_up_forward_full_mantissa_transposed_weights(Cs, hw, conv_form):
    """the other operand: W one-hot 1.0 (pattern P positions), Wt full-mantissa, z non-zero in ONE channel per image -- every y element
    is z[ci] * wt[ci, c, sub-pixel]"""
    from popcorn_amd import ops
    B, (H, W), Cz = 2, hw, Cs
    gen = _gen(620 + Cs + H)
    skip = torch.randn(B, Cs, H, W, generator=gen)
    wt = SP.full_mantissa((Cz, Cz, 2, 2), gen)
    K = 9 * (Cs + Cz)
    ks = [k for k in range(0, K, 5)]
    zs = torch.zeros(Cz, B, Cz, H // 2, W // 2)
    for j in range(Cz):
        for b in range(B):
            zs[j, b, (j + 3 * b) % Cz] = torch.randn(H // 2, W // 2, generator=gen)
    ws = torch.stack([(SP.pattern_p_forward(8, Cs + Cz, k, gen) != 0).float() for k in ks])
    ws[:, :, :Cs] = 0                                                   # the up-sampled half only: the skip half would add a second term
    bnd, scale = _bn_dev(8)
    sd, zd, ws_d, wtd, bt = skip.cuda(), zs.cuda(), ws.cuda(), wt.cuda(), torch.zeros(Cz, device="cuda")
    out = torch.full((len(ks), B, 8, H, W), NAN, device="cuda")
    for i, k in enumerate(ks):
        ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd[k % Cz], "w": ws_d[i], "wt": wtd, "bt": bt, "bn": bnd, "out": out[i]}], relu=False)
    ref = torch.stack([F.conv2d(torch.cat([skip.double(), F.conv_transpose2d(zs[k % Cz].double(), wt.double(), stride=2)], 1),
                                ws[i].double(), padding=1) for i, k in enumerate(ks)]) * scale.view(1, 1, 8, 1, 1)
    form = "split" if conv_form else "fp32mfma"
    what = "E up fwd (Wt operand) Cs=%d %s" % (Cs, hw)
    _finish(SP.assert_single_product(out, ref, form, what=what), form, what)


@pytest.mark.parametrize("Cs,hw", [(8, (12, 16)), (16, (12, 16)), (8, (20, 72))])
def test_e_up_forward_bias_through_the_taps(Cs, hw, conv_form):
    """z = 0 and skip = 0 with a full-mantissa bt and ONE tap of 1.0 per output channel in the up-sampled half: y is bt[c] where the tap
    lands inside the image and 0 where it does not, exactly, on all four borders and corners and both output parities"""
    from popcorn_amd import ops, _lib as L
    B, (H, W), Cz = 2, hw, Cs
    gen = _gen(640 + Cs + H)
    bt = SP.full_mantissa((Cz,), gen, scale=1.0)
    wt = SP.full_mantissa((Cz, Cz, 2, 2), gen)
    ks = [k for k in range(9 * (Cs + Cz)) if all(i >= 9 * Cs for i in SP.pattern_p_index(8, Cs + Cz, k))]
    assert len(ks) >= 9
    ws = torch.stack([(SP.pattern_p_forward(8, Cs + Cz, k, gen) != 0).float() for k in ks])
    taps = {(i % 9) for k in ks for i in SP.pattern_p_index(8, Cs + Cz, k)}
    assert taps == set(range(9))                                        # every tap, so every border and corner drops a term somewhere
    sd, zd = torch.zeros(B, Cs, H, W, device="cuda"), torch.zeros(B, Cz, H // 2, W // 2, device="cuda")
    ws_d, wtd, btd = ws.cuda(), wt.cuda(), bt.cuda()
    out = torch.full((len(ks), B, 8, H, W), NAN, device="cuda")
    for i in range(len(ks)):
        ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd, "w": ws_d[i], "wt": wtd, "bt": btd, "bn": L.bn(None), "out": out[i]}], relu=False)
    u = bt.double().view(1, Cz, 1, 1).expand(B, Cz, H, W)
    ref = torch.stack([F.conv2d(torch.cat([torch.zeros(B, Cs, H, W, dtype=torch.double), u], 1), ws[i].double(), padding=1) for i in range(len(ks))])
    assert int((ref == 0).sum()) > 0
    assert torch.equal(out.cpu().double(), ref), "bias through the taps: %d elements differ" % int((out.cpu().double() != ref).sum())


# =========================================================================================================================================
# Family F: the whole 32 x 32 level (forward)
# =========================================================================================================================================

@pytest.mark.parametrize("part", [0, 1, 2])
def test_f_level2_forward_every_triple_of_both_convs(part):
    """pattern P in every layer (both 16 -> 16 convs on the same launch index, the transposed conv one-hot over ci with full-mantissa
    values): each stage is one product; the float64 chain, rounded to fp32 after each stage, is the reference of the next.  These
    kernels have the fp32-MFMA form only.  The 144 launches of the family in three parts."""
    from popcorn_amd import ops
    B = 2
    gen = _gen(700)
    x = torch.relu(torch.randn(B, 16, 32, 32, generator=gen)) + 0.25     # a pooled post-ReLU map; strictly positive keeps every product alive
    f1 = SP.pattern_p_family(16, 16, gen, "forward")
    f2 = SP.pattern_p_family(16, 16, gen, "forward")
    wts = torch.stack([SP.pattern_p_convt(16, k, gen) for k in range(16)])
    ks = list(range(part, 144, 3))
    bn1, s1 = _bn_dev(16)
    bn2, s2 = _bn_dev(16)
    xd, f1d, f2d, wtd, bt = x.cuda(), f1.cuda(), f2.cuda(), wts.cuda(), torch.zeros(16, device="cuda")
    n = len(ks)
    c1 = torch.full((n, B, 16, 32, 32), NAN, device="cuda")
    c2 = torch.full((n, B, 16, 32, 32), NAN, device="cuda")
    u2 = torch.full((n, B, 16, 64, 64), NAN, device="cuda")
    assert ops.level2_fwd_ok(xd, u2[0])
    for i, k in enumerate(ks):
        ops.level2_fwd_group([{"x": xd, "w1": f1d[k], "bn1": bn1, "w2": f2d[(k * 5 + 1) % 144], "bn2": bn2, "wt": wtd[k % 16], "bt": bt,
                               "c1": c1[i], "c2": c2[i], "u2": u2[i]}])
    r1 = torch.stack([torch.relu(F.conv2d(x.double(), f1[k].double(), padding=1) * s1.view(1, 16, 1, 1)) for k in ks])
    SP.assert_single_product(c1, r1, "fp32mfma", what="F level2 c1 part %d" % part)
    r1f = r1.float().double()
    r2 = torch.stack([torch.relu(F.conv2d(r1f[i], f2[(k * 5 + 1) % 144].double(), padding=1) * s2.view(1, 16, 1, 1)) for i, k in enumerate(ks)])
    SP.assert_single_product(c2, r2, "fp32mfma", what="F level2 c2 part %d" % part)
    r2f = r2.float().double()
    r3 = torch.stack([F.conv_transpose2d(r2f[i], wts[k % 16].double(), stride=2) for i, k in enumerate(ks)])
    SP.assert_single_product(u2, r3, "fp32mfma", what="F level2 u2 part %d" % part)
    assert int((r3 != 0).sum()) > r3.numel() // 8


# =========================================================================================================================================
# Family E: composed Up (backward)
# =========================================================================================================================================

def _up_chain(z, w_up, wt, G):
    """float64 autograd of  conv3x3(conv_transpose2d(z, Wt, bt = 0), W[:, Cs:])  against G: (gz, dw_up, dwt, dbt)"""
    zd, wd, wtd = (t.double().requires_grad_(True) for t in (z, w_up, wt))
    btd = torch.zeros(wt.shape[1], dtype=torch.double, requires_grad=True)
    F.conv2d(F.conv_transpose2d(zd, wtd, btd, stride=2), wd, padding=1).backward(G.double())
    return zd.grad, wd.grad, wtd.grad, btd.grad


UP_BWD = [(8, (12, 16)), (16, (12, 16)), (8, (20, 72)), (16, (24, 136)), (8, (16, 64)), (8, (20, 136))]


@pytest.mark.parametrize("operand", ["w", "wt"])
@pytest.mark.parametrize("Cs,hw", UP_BWD)
def test_e_up_backward_sparse_gradient(Cs, hw, operand):
    """pc_conv3x3_up_bwd_group (up_bwd_kernel<8|16, 64|128>, reduction, chain rule; fp32 MFMA only): G on pattern S -- corners, both
    sides of the 4-low-res-row block seams (rows 7|8, 15|16) and of the 128-column tile seam (127|128), ragged last tile -- and z dense.
      operand "w":  W[:, Cs:] full-mantissa on pattern P, Wt signed one-hot: gz = +-G w, dw[:, Cs:] = +-G z, dbt = G w;
      operand "wt": W[:, Cs:] signed one-hot, Wt full-mantissa and dense:   gz = +-G wt, dwt = +-G z, dbt = +-G.
    An element is checked where the float64 chain on the operands' non-zero masks counts at most one term behind it.  Even launches go
    through ops.conv3x3_up_bwd_group, odd ones through the deferred WgradBatch.up_bwd_group.  dw[:, :Cs] stays untouched."""
    from popcorn_amd import ops
    B, (H, W), Cz = 2, hw, Cs
    gen = _gen(660 + Cs + H + W)
    req = SP.required_positions(H, W, (8, 16), (128,))
    gs, places = SP.pattern_s_gradients(B, H, W, 8, SP.pattern_s_groups(B, H, W, 8, req), gen)
    SP.assert_every_channel_visits(places, req, 8)
    nS, K = gs.shape[0], 9 * Cz
    n = K if H * W <= 256 else max(nS, 24)
    ks = [l if n == K else (l * (K // n)) % K for l in range(n)]
    z = torch.randn(B, Cz, H // 2, W // 2, generator=gen)
    skip = torch.randn(B, Cs, H, W, generator=gen)
    w_all = torch.randn(n, 8, Cs + Cz, 3, 3, generator=gen) * 0.1
    wt_all = []
    for l, k in enumerate(ks):
        p = SP.pattern_p_forward(8, Cz, k, gen)
        if operand == "w":
            w_all[l][:, Cs:] = p
            wt_all.append(SP.pattern_p_convt(Cz, l % Cz, gen, one_hot=True))
        else:
            w_all[l][:, Cs:] = (p != 0).float() * torch.where(torch.rand(8, 1, 1, 1, generator=gen) < 0.5, -1.0, 1.0)
            wt_all.append(SP.full_mantissa((Cz, Cz, 2, 2), gen))
    wt_all = torch.stack(wt_all)
    bnd, scale = _bn_dev(Cz)
    bn_out, _ = _bn_dev(8)
    zd, sd, gd, wd, wtd, bt = z.cuda(), skip.cuda(), gs.cuda(), w_all.cuda(), wt_all.cuda(), torch.zeros(Cz, device="cuda")
    gz = torch.full((n, B, Cz, H // 2, W // 2), NAN, device="cuda")
    dw = torch.full((n, 8, Cs + Cz, 3, 3), 7.0, device="cuda")
    dwt = torch.full((n, Cz, Cz, 2, 2), NAN, device="cuda")
    dbt = torch.full((n, Cz), NAN, device="cuda")
    y = torch.empty(B, 8, H, W, device="cuda")
    for l in range(n):
        slot = ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd, "w": wd[l], "wt": wtd[l], "bt": bt, "bn": bn_out, "out": y}])[0]
        pr = {"g": gd[l % nS], "z": zd, "z_bn": bnd, "gz": gz[l], "w": wd[l], "wt": wtd[l], "bt": bt, "fwd_ws": slot, "dw": dw[l],
              "dwt": dwt[l], "dbt": dbt[l]}
        assert ops.conv3x3_up_bwd_ok(pr["g"], pr["z"], pr["gz"])
        if l % 2 == 0:
            ops.conv3x3_up_bwd_group([pr])
        else:
            wb = ops.WgradBatch(torch.device("cuda"))
            wb.up_bwd_group([pr])
            wb.finish()
    torch.cuda.synchronize()
    vals = [_up_chain(z, w_all[l][:, Cs:], wt_all[l], gs[l % nS]) for l in range(n)]
    cnts = [_up_chain((z != 0).float(), (w_all[l][:, Cs:] != 0).float(), (wt_all[l] != 0).float(), (gs[l % nS] != 0).float()) for l in range(n)]
    rgz, rdw, rdwt, rdbt = (torch.stack([v[i] for v in vals]) for i in range(4))
    cgz, cdw, cdwt, cdbt = (torch.stack([c[i] for c in cnts]) <= 1.0 for i in range(4))
    rgz = rgz * (z > 0).double() * scale.view(1, 1, Cz, 1, 1)
    what = "E up bwd (%s operand) Cs=%d %s" % (operand, Cs, hw)
    assert bool((dw[:, :, :Cs] == 7.0).all())
    r = SP.assert_single_product(gz, rgz, "fp32mfma", where=cgz, what=what + " gz")
    assert r.n > 0
    if operand == "w":
        r = SP.assert_single_product(dw[:, :, Cs:], rdw, "fp32mfma", where=cdw, what=what + " dw")
    else:
        r = SP.assert_single_product(dwt, rdwt, "fp32mfma", where=cdwt, what=what + " dwt")
    assert r.n > 0
    r = SP.assert_single_product(dbt, rdbt, "fp32mfma", where=cdbt, what=what + " dbt")
    assert r.n > 0
    print(what, "positions: rows %s x columns %s" % (sorted({p[0] for p in req}), sorted({p[1] for p in req})))


# =========================================================================================================================================
# Family F: the whole 32 x 32 level (backward)
# =========================================================================================================================================

@pytest.mark.parametrize("mode", ["S", "P"])
def test_f_level2_backward(mode):
    """WgradBatch.level2_bwd_group with both convs' weights on pattern P (one non-zero per input channel).
      mode S: g2 on pattern S -- dw2 = g2 c1 and db2 = g2 are single products; g1 = g2 w2 (times relu'(c1) and 2^k) has one non-zero
              per channel, so with g1 rounded to fp32 as the kernel holds it dw1 = g1 x, db1 = g1 and the scattered out += g1 w1
              (times relu'(act) and 2^k) are single products too;
      mode P: g2 dense -- every pixel of the data-gradient chain into out is one product g1 w1; the weight / bias gradients are sums
              there and go against float64 at the bar of test_level2_bwd_group_vs_autograd (5e-5 of the largest value)."""
    from popcorn_amd import ops
    B, n = 2, 48
    gen = _gen(720)
    act = torch.randn(B, 16, 64, 64, generator=gen)                        # mixed sign, no ties
    x, idx = F.max_pool2d(act, 2, return_indices=True)
    c1 = torch.randn(B, 16, 32, 32, generator=gen)                         # its sign is conv1's ReLU mask
    fam1 = SP.pattern_p_family(16, 16, gen, "dgrad")
    fam2 = SP.pattern_p_family(16, 16, gen, "dgrad")
    if mode == "S":
        req = SP.required_positions(32, 32, (4, 16), (16,))
        gs, places = SP.pattern_s_gradients(B, 32, 32, 16, SP.pattern_s_groups(B, 32, 32, 16, req), gen)
        SP.assert_every_channel_visits(places, req, 16)
        print("F level2 bwd positions: rows %s x columns %s" % (sorted({y for y, _ in req}), sorted({x for _, x in req})))
    else:
        gs = torch.randn(1, B, 16, 32, 32, generator=gen)
    nS = gs.shape[0]
    bn1, s1 = _bn_dev(16)
    abn, sa = _bn_dev(16)
    prev = torch.randn(n, B, 16, 64, 64, generator=gen)
    out = prev.cuda()
    dws = [torch.full((n, 16, 16, 3, 3), NAN, device="cuda") for _ in range(2)]
    dbs = [torch.full((n, 16), NAN, device="cuda") for _ in range(2)]
    gd, f1d, f2d, xd, c1d, actd = gs.cuda(), fam1.cuda(), fam2.cuda(), x.cuda(), c1.cuda(), act.cuda()
    k1 = [(3 * l + 1) % 144 for l in range(n)]
    k2 = [(3 * l) % 144 for l in range(n)]
    for l in range(n):
        pr = {"g2": gd[l % nS], "c1": c1d, "x": xd, "w1": f1d[k1[l]], "w2": f2d[k2[l]], "bn1": bn1, "act": actd, "act_bn": abn, "out": out[l],
              "dw1": dws[0][l], "db1": dbs[0][l], "dw2": dws[1][l], "db2": dbs[1][l]}
        assert ops.level2_bwd_ok(pr["g2"], pr["c1"], pr["x"], pr["act"], pr["out"])
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.level2_bwd_group([pr])
        wb.finish()
    torch.cuda.synchronize()
    rw1, rb1, rw2, rb2, rout = [], [], [], [], []
    for l in range(n):
        g2 = gs[l % nS].double()
        g1 = _gx_reference(g2, fam2[k2[l]]) * (c1 > 0).double() * s1.view(1, 16, 1, 1)
        g1 = g1.float().double()                                           # the kernel holds g1 in fp32: one rounding per product
        rw2.append(torch.nn.grad.conv2d_weight(c1.double(), (16, 16, 3, 3), g2, padding=1))
        rb2.append(g2.sum((0, 2, 3)))
        rw1.append(torch.nn.grad.conv2d_weight(x.double(), (16, 16, 3, 3), g1, padding=1))
        rb1.append(g1.sum((0, 2, 3)))
        gx = F.max_unpool2d(_gx_reference(g1, fam1[k1[l]]), idx, 2, output_size=(64, 64))
        rout.append(gx * (act > 0).double() * sa.view(1, 16, 1, 1))
    rw1, rb1, rw2, rb2, rout = (torch.stack(t) for t in (rw1, rb1, rw2, rb2, rout))
    what = "F level2 bwd pattern " + mode
    r = SP.assert_single_product(out, rout, "fp32mfma", prev=prev, what=what + " out")
    # (a product survives where c1 > 0, one half, and the window's maximum of act is positive, 15 / 16; mode S: 16 products a launch)
    assert r.n > (n * 16 // 8 if mode == "S" else n * B * 16 * 32 * 32 // 4)
    for name, got, ref in (("dw2", dws[1], rw2), ("db2", dbs[1], rb2), ("dw1", dws[0], rw1), ("db1", dbs[0], rb1)):
        if mode == "S":
            SP.assert_single_product(got, ref, "fp32mfma", what="%s %s" % (what, name))
        else:
            err = (got.cpu().double() - ref).flatten(1).abs().amax(1) / ref.flatten(1).abs().amax(1).clamp_min(1e-6)
            print(what, name, "max error / max|ref| over the launches", float(err.max()))
            assert float(err.max()) < 5e-5, (name, float(err.max()))


# =========================================================================================================================================
# The pooled second output below a ragged last tile (found by family A at H = 20: the split-form and the channels-last kernels stored
# the pooled rows of the strips BELOW the image -- into the next channel / image, and past the end of pool_out for the last one)
# =========================================================================================================================================

@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 16), (16, 16)])
@pytest.mark.parametrize("H", [20, 36])
def test_pooled_second_output_stays_inside_its_buffer(H, cin, cout, prec, conv_form):
    """H % 16 != 0: pool_out is the first B images of a NaN-filled buffer of B + 1; the extra image stays NaN and pool_out equals
    max_pool2d of the output (dense random operands)"""
    from popcorn_amd import ops, _lib as L
    B, W = 2, 64
    gen = _gen(800 + H + cin + cout)
    x, w, b = torch.randn(B, cin, H, W, generator=gen), torch.randn(cout, cin, 3, 3, generator=gen) * 0.2, torch.randn(cout, generator=gen) * 0.1
    with L.precision(prec):
        out = L.empty_act(B, cout, H, W, "cuda")
        out.fill_(NAN)
        big = L.empty_act(B + 1, cout, H // 2, W // 2, "cuda")
        big.fill_(NAN)
        assert ops.pool_out_like(out) is not None and ops.pool_out_like(out).stride() == big[:B].stride()
        bd = b.cuda()
        ops.conv3x3_fwd_group([{"a": L.as_act(x.cuda()), "w": w.cuda(), "bn": L.bn(bd), "out": out, "pool_out": big[:B]}])
        torch.cuda.synchronize()
    assert bool(torch.isnan(big[B]).all()), "%d elements written past the end of pool_out" % int((~torch.isnan(big[B])).sum())
    assert not bool(torch.isnan(out).any())
    assert torch.equal(big[:B].float(), F.max_pool2d(out.float(), 2))
