"""Exact-arithmetic known answers (tests/exact_arith.py): every operand is a small dyadic number, every partial sum
a kernel can form is exactly representable in fp32 (the budget, asserted before each launch), so the float64 reference is exact, every
summation order gives the same bits, and the bar is whole-tensor equality -- dense operands, every element, every arithmetic form a
family has: fp32 MFMA, the split form (pc_set_conv_split / pc_set_head_split), and bf16 mode, where the expected value is the exact
value rounded to nearest even at each rounding point of include/popcorn_hip.h.  Families A-G as in DESIGN.md section 6."""
import pytest
import torch
import torch.nn.functional as F

from tests import exact_arith as E

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(params=[1, 0], ids=["split", "fp32mfma"])
def conv_form(request):
    """pc_set_conv_split: 1 = split-operand kernels where they exist, 0 = v_mfma_f32_16x16x4_f32 everywhere; restored afterwards"""
    from popcorn_amd import _lib as L
    prev = L.lib().pc_set_conv_split(int(request.param))
    yield int(request.param)
    L.lib().pc_set_conv_split(prev)


@pytest.fixture(params=["fp32mfma", "split", "bf16"])
def head_mode(request):
    """the head's three forms: pc_set_head_split 0 / 1 in fp32 mode, and bf16 mode; restored afterwards"""
    from popcorn_amd import _lib as L
    prev = L.lib().pc_set_head_split(1 if request.param == "split" else 0)
    with L.precision("bf16" if request.param == "bf16" else "fp32"):
        yield request.param
    L.lib().pc_set_head_split(prev)


def _bn_dev(bn, with_bias=True):
    from popcorn_amd import _lib as L
    return L.bn(bn["bias"].cuda() if with_bias else None, bn["gamma"].cuda(), bn["beta"].cuda(), bn["mean"].cuda(), bn["var"].cuda(), bn["eps"])


def _act(t):
    """device copy in the container of the current arithmetic mode (planar fp32 / channels-last bf16); the values are bf16 numbers
    wherever the mode is bf16 (asserted)"""
    from popcorn_amd import _lib as L
    d = L.as_act(t.cuda())
    assert torch.equal(d.float().cpu(), t.float())
    return d


def _out(shape, prev=None):
    """output tensor in the mode's container: NaN-filled, or a copy of prev for the += forms"""
    from popcorn_amd import _lib as L
    if prev is not None:
        return _act(prev)
    o = L.empty_act(*shape, "cuda")
    o.fill_(NAN)
    return o


def _mode(bf16):
    from popcorn_amd import _lib as L
    return L.precision("bf16" if bf16 else "fp32")


# =========================================================================================================================================
# Family A: conv forward
# =========================================================================================================================================

def _run_forward(case, loader, hw, bf16, relu=True, extra=None):
    """one launch of ops.conv3x3_fwd_group on a conv_fwd_case; returns the output"""
    from popcorn_amd import ops, _lib as L
    src = case["src"]
    B, cout = src["a"].shape[0], case["w"].shape[0]
    kw = {}
    pr = {"w": case["w"].cuda(), "bn": _bn_dev(case["bn"])}
    if loader == "reflect":
        pr["a"], pr["chmap"] = src["a"].cuda(), src["chmap"]                    # the model input stays planar fp32 in both modes
        kw = {"a_mode": L.PC_SRC_REFLECT, "a_pad": (14, 14), "out_hw": hw, "a_channels": case["w"].shape[1]}
    else:
        pr["a"] = _act(src["a"])
        if loader == "pool2":
            kw = {"a_mode": L.PC_SRC_POOL2}
        if loader == "concat":
            pr["b"] = _act(src["b"])
            kw = {"b_offset": (1, 1)}
    out = _out((B, cout, hw[0], hw[1]))
    pr["out"] = out
    pr.update(extra or {})
    ops.conv3x3_fwd_group([pr], relu=relu, **kw)
    torch.cuda.synchronize()
    return out


def _expected_fwd(case, relu, bf16):
    ex = case["exact"] if relu else case["pre"]
    return E.rbf(ex) if bf16 else ex


@pytest.mark.parametrize("wide", [None, "x", "w"])
@pytest.mark.parametrize("cin,cout", E.PAIRS)
def test_a_forward_aligned(cin, cout, wide, conv_form):
    """(20, 36): W % 4 == 0 -- the split form / the staged loader; 2 x 2 tiles of 32 x 16 with ragged last tiles.  wide: one operand of
    9-12 significant bits (non-empty second and third pieces of the split), the other of <= 2"""
    case = E.conv_fwd_case("plain", cin, cout, 2, (20, 36), 100 + cin + cout, wide=wide)
    for relu in (True, False):
        out = _run_forward(case, "plain", (20, 36), False, relu=relu)
        E.assert_equal(out, _expected_fwd(case, relu, False), "A fwd %d->%d (20,36) wide=%s relu=%s form=%d" % (cin, cout, wide, relu, conv_form))


@pytest.mark.parametrize("cin,cout", E.PAIRS + [(2, 8), (4, 8), (32, 8)])
def test_a_forward_generic(cin, cout):
    """(19, 35): W % 4 != 0, the generic loader"""
    case = E.conv_fwd_case("plain", cin, cout, 2, (19, 35), 100 + cin + cout)
    out = _run_forward(case, "plain", (19, 35), False)
    E.assert_equal(out, case["expected"], "A fwd %d->%d (19,35)" % (cin, cout))


@pytest.mark.parametrize("loader,cin,cout,hw", [("pool2", 8, 16, (20, 36)), ("concat", 32, 8, (23, 35)), ("reflect", 2, 8, (58, 69)),
                                                ("reflect", 4, 8, (58, 69))])
def test_a_forward_fused_loaders(loader, cin, cout, hw, conv_form):
    case = E.conv_fwd_case(loader, cin, cout, 2, hw, 130 + cin)
    out = _run_forward(case, loader, hw, False)
    E.assert_equal(out, case["expected"], "A fwd %s %d->%d" % (loader, cin, cout))


def _pooled_and_dot(cin, cout, bf16, what):
    """(20, 64), the smallest shape pc_conv3x3_pool_out_ok takes: the pooled second output; (8 -> 8) the dot_w epilogue with an integer
    dot_w into channel 1 of a two-channel map whose channel 0 stays"""
    from popcorn_amd import ops
    case = E.conv_fwd_case("plain", cin, cout, 2, (20, 64), 140 + cin + cout, bf16=bf16)
    if bf16:
        E.assert_bf16_coverage(case["exact"], what)
    like = _out((2, cout, 20, 64))
    pool = ops.pool_out_like(like)
    assert pool is not None
    pool.fill_(NAN)
    out = _run_forward(case, "plain", (20, 64), bf16, extra={"pool_out": pool})
    E.assert_equal(out, case["expected"], what + " out")
    E.assert_equal(pool, F.max_pool2d(case["expected"], 2), what + " pooled second output")
    if (cin, cout) == (8, 8):
        dot_w = E.ints((8,), -2, 2, E.gen(150))
        dot_w[0] = 2.0
        want = (case["expected"] * dot_w.double().view(1, 8, 1, 1)).sum(1)
        E.assert_budget((case["expected"].abs() * dot_w.double().abs().view(1, 8, 1, 1)).sum(1), 0.25, what + " dot")
        maps = torch.full((2, 2, 20, 64), NAN, device="cuda")
        _run_forward(case, "plain", (20, 64), bf16, extra={"out": None, "dot_w": dot_w.cuda(), "dot_out": maps[:, 1:2]})
        E.assert_equal(maps[:, 1], want, what + " dot epilogue")
        assert bool(torch.isnan(maps[:, 0]).all())


@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 16), (16, 16)])
def test_a_forward_pooled_second_output_and_dot_epilogue(cin, cout, conv_form):
    _pooled_and_dot(cin, cout, False, "A fwd %d->%d (20,64) form=%d" % (cin, cout, conv_form))


@pytest.mark.parametrize("case", E.A_BF16, ids=lambda c: "%s-%d-%d-%d-%dx%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1]))
def test_a_forward_bf16(case):
    """the channels-last bf16 kernels: expected = RNE(relu(bn(conv))) of the exact sum; the reflect loader rounds its fp32 input"""
    loader, cin, cout, B, hw = case
    c = E.conv_fwd_case(loader, cin, cout, B, hw, 100 + cin + cout, bf16=True)
    E.assert_bf16_coverage(c["exact"], str(case))
    if loader == "reflect":
        assert not torch.equal(E.rbf(c["src"]["a"]), c["src"]["a"])             # the input needs rounding
    with _mode(True):
        out = _run_forward(c, loader, hw, True)
        assert out.dtype == torch.bfloat16
        E.assert_equal(out, c["expected"], "A fwd bf16 %s" % (case,))
        if loader == "plain" and B == 1:
            E.assert_equal(_run_forward(c, loader, hw, True, relu=False), E.rbf(c["pre"]), "A fwd bf16 no relu %s" % (case,))


@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 16), (16, 16)])
def test_a_forward_bf16_pooled_second_output_and_dot_epilogue(cin, cout):
    with _mode(True):
        _pooled_and_dot(cin, cout, True, "A fwd bf16 %d->%d (20,64)" % (cin, cout))


# =========================================================================================================================================
# Family B: data gradient and fused backward
# =========================================================================================================================================

@pytest.mark.parametrize("cin_total,c0,cn,cg", [(8, 0, 8, 8), (16, 8, 8, 8), (32, 16, 16, 8), (8, 0, 8, 16), (16, 0, 16, 16)])
@pytest.mark.parametrize("hw", [(20, 36), (19, 35)])
def test_b_dgrad_plain_and_masked_accumulate(cin_total, c0, cn, cg, hw):
    """pc_conv3x3_dgrad: plain into a NaN output, then masked (act with exact zeros, odd BN scales) += a previous value"""
    from popcorn_amd import ops
    d = E.dgrad_case(cg, cin_total, c0, cn, 2, hw, 200 + cg + cin_total)
    wcol = d["w"][:, c0:c0 + cn]
    E.budget_dgrad(d["g"], wcol, d["bn"]["scale"], d["prev"])
    gd, wd = d["g"].cuda(), d["w"].cuda()
    out = torch.full((2, cn, *hw), NAN, device="cuda")
    ops.conv3x3_dgrad(gd, wd, c0, cn, out)
    E.assert_equal(out, E.ref_dgrad(d["g"], d["w"], c0, cn), "B dgrad plain cg=%d cin=%d %s" % (cg, cin_total, hw))
    out = d["prev"].cuda()
    ops.conv3x3_dgrad(gd, wd, c0, cn, out, act=d["act"].cuda(), act_bn=_bn_dev(d["bn"], False), accumulate=True)
    E.assert_equal(out, E.ref_dgrad(d["g"], d["w"], c0, cn, d["act"], d["bn"]["scale"], d["prev"]), "B dgrad masked += cg=%d cin=%d %s" % (cg, cin_total, hw))


@pytest.mark.parametrize("cn", [8, 16])
def test_b_dgrad_pool_scatter(cn):
    """pc_conv3x3_dgrad(pool=True) at (20, 36) from a (40, 72) activation with unique window maxima and windows whose maximum is 0"""
    from popcorn_amd import ops
    d = E.dgrad_case(16, cn, 0, cn, 2, (20, 36), 210 + cn, pool=True)
    E.budget_dgrad(d["g"], d["w"], d["bn"]["scale"], F.max_pool2d(d["prev"].abs(), 2))
    out = d["prev"].cuda()
    ops.conv3x3_dgrad(d["g"].cuda(), d["w"].cuda(), 0, cn, out, act=d["act"].cuda(), act_bn=_bn_dev(d["bn"], False), pool=True, accumulate=True)
    E.assert_equal(out, E.ref_dgrad_pool(d["g"], d["w"], 0, cn, d["act"], d["bn"]["scale"], d["prev"]), "B dgrad pool scatter cn=%d" % cn)


# the fused backward (WgradBatch.conv3x3_bwd_group), as tests/test_gpu_single_product.py: name -> (gradient channels, input channels of
# the layer, first column c0, column blocks as c0_add, masked, accumulate, pool scatter, needs the split form)
FUSED = {
    "8_plain": (8, 8, 0, (0,), False, False, False, False),
    "8_masked_accumulate": (8, 8, 0, (0,), True, True, False, False),
    "8_concat_up_half": (8, 16, 8, (0,), False, False, False, False),
    "8_concat_both_blocks": (8, 16, 0, (0, 8), True, False, False, False),
    "16_both_blocks": (16, 16, 0, (0, 8), True, False, False, True),
    "8_pool": (8, 8, 0, (0,), True, True, True, True),
    "16_pool": (16, 8, 0, (0,), True, True, True, True),
}


def _fused_cases():
    out = []
    for form in (1, 0):
        for name, spec in FUSED.items():
            if spec[7] and not form:
                continue
            for hw in ((20, 36), (36, 68)):
                if hw != (20, 36) and name not in ("8_plain", "16_both_blocks"):
                    continue
                for wide in ((None, "x", "w") if form and hw == (20, 36) and name in ("8_plain", "16_both_blocks") else (None,)):
                    out.append(pytest.param(form, name, hw, wide, id="%s-%s-%dx%d-%s" % ("split" if form else "fp32mfma", name, hw[0], hw[1], wide)))
    return out


@pytest.mark.parametrize("form,name,hw,wide", _fused_cases())
def test_b_fused_backward(form, name, hw, wide):
    """gx (plain / masked / += / pool scatter), dw and db of one launch, dense operands; the fp32-MFMA kernel and all four
    conv3x3_bwd_s3_kernel<8|16, false|true> instantiations; wide: g (x) or w of 9-12 significant bits"""
    from popcorn_amd import ops, _lib as L
    cg, cin_total, c0, blocks, masked, acc, pool, _ = FUSED[name]
    B, (H, W) = 2, hw
    gg = E.gen(300 + 7 * cg + cin_total + H)
    g, w = E._xw((B, cg, H, W), (cg, cin_total, 3, 3), gg, wide, xr=E.G_RANGE)
    if pool:
        act = E.pooled_act((B, 8, 2 * H, 2 * W), gg)
        x_full = F.max_pool2d(act, 2)
    else:
        xr = 1 if wide else E.X_RANGE                                       # (wide: the weight-gradient sums over the pixels stay in the budget)
        x_full = E.ints((B, cin_total, H, W), -xr, xr, gg)
    cols = [c0 + blk + j for blk in blocks for j in range(8)]
    nb = len(blocks)
    bns = [E.bn_odd(8, gg) for _ in blocks]
    scale = torch.cat([b["scale"] for b in bns])
    Ho, Wo = (2 * H, 2 * W) if pool else (H, W)
    prev = E.ints((B, 8 * nb, Ho, Wo), -64, 64, gg) if acc else None
    mask_src = act if pool else x_full[:, cols]
    E.assert_relu_coverage(mask_src, name)
    # ---- reference and budget
    if pool:
        rgx = E.ref_dgrad_pool(g, w, 0, 8, act, scale, prev)
        E.budget_dgrad(g, w[:, cols], scale, F.max_pool2d(prev.abs(), 2), name)
    else:
        rgx = torch.cat([E.ref_dgrad(g, w, c0 + blk, 8, mask_src[:, 8 * i:8 * i + 8] if masked else None, bns[i]["scale"] if masked else None,
                                     prev[:, 8 * i:8 * i + 8] if acc else None) for i, blk in enumerate(blocks)], 1)
        E.budget_dgrad(g, w[:, cols], scale if masked else None, prev, name)
    rdw, rdb = E.ref_wgrad(x_full[:, cols], g)
    E.budget_wgrad(x_full[:, cols], g, what=name)
    # ---- launch
    out = prev.cuda() if acc else torch.full((B, 8 * nb, Ho, Wo), NAN, device="cuda")
    dw = torch.full((cg, cin_total, 3, 3), 7.0, device="cuda")
    db = torch.full((cg,), NAN, device="cuda")
    prev_form = L.lib().pc_set_conv_split(form)
    try:
        gd, wd, xd = g.cuda(), w.cuda(), x_full.cuda()
        actd = act.cuda() if pool else None
        probs = []
        for i, blk in enumerate(blocks):
            pr = {"g": gd, "x": xd[:, c0 + blk:c0 + blk + 8], "w": wd, "out": out[:, 8 * i:8 * i + 8], "dw": dw, "db": db if i == 0 else None,
                  "c0_add": blk, "x_bn": _bn_dev(bns[i], False) if masked else None}
            if pool:
                pr["pool_act"] = actd
            probs.append(pr)
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.conv3x3_bwd_group(probs, cin_total, c0, accumulate=acc)
        wb.finish()
        torch.cuda.synchronize()
    finally:
        L.lib().pc_set_conv_split(prev_form)
    what = "B fused %s %s wide=%s [%s]" % (name, hw, wide, "split" if form else "fp32mfma")
    E.assert_equal(out, rgx, what + " gx")
    lo, hi = min(cols), max(cols) + 1
    E.assert_equal(dw[:, lo:hi], rdw, what + " dw")
    rest = [c for c in range(cin_total) if not lo <= c < hi]
    assert bool((dw[:, rest] == 7.0).all())
    E.assert_equal(db, rdb, what + " db")


def _fused_bf16(d, gc, xc, cin_total, c0, masked, acc, pool, what):
    from popcorn_amd import ops
    rgx, rdw, rdb = E.fused_bwd_reference(d, c0, masked=masked, acc=acc, bf16=True, pool=pool)
    out = _out(d["prev"].shape, d["prev"] if (acc or pool) else None)
    dw = torch.full((gc, cin_total, 3, 3), 7.0, device="cuda")
    db = torch.full((gc,), NAN, device="cuda")
    pr = {"g": _act(d["g"]), "x": _act(d["x"]), "w": d["w"].cuda(), "out": out, "dw": dw, "db": db,
          "x_bn": _bn_dev(d["bn"], False) if masked else None}
    if pool:
        pr["pool_act"] = _act(d["act"])
    wb = ops.WgradBatch(torch.device("cuda"))
    wb.conv3x3_bwd_group([pr], cin_total, c0, accumulate=acc)
    wb.finish()
    torch.cuda.synchronize()
    E.assert_equal(out, rgx, what + " gx")
    E.assert_equal(dw[:, c0:c0 + xc], rdw, what + " dw")
    other = [c for c in range(cin_total) if not c0 <= c < c0 + xc]
    assert bool((dw[:, other] == 7.0).all())
    E.assert_equal(db, rdb, what + " db")


@pytest.mark.parametrize("B,hw", E.BF16_SHAPES)
@pytest.mark.parametrize("name", list(E.B_BF16_FUSED))
def test_b_fused_backward_bf16(name, B, hw):
    """the five cases of test_bf16_conv_backward_fused_op, dense: the data gradient is rounded ONCE, after mask, scale and accumulate;
    dw / db are fp32 sums (no rounding point)"""
    gc, xc, cin_total, c0 = E.B_BF16_FUSED[name]
    up = "up_half" in name
    d = E.fused_bwd_case(gc, xc, cin_total, c0, B, hw, 300 + gc + cin_total, up_half=up)
    with _mode(True):
        _fused_bf16(d, gc, xc, cin_total, c0, not up, "accumulate" in name, False, "B fused bf16 %s %s" % (name, hw))


@pytest.mark.parametrize("B,hw", E.BF16_POOL_SHAPES)
@pytest.mark.parametrize("xc", [8, 16])
def test_b_fused_backward_pool_bf16(xc, B, hw):
    d = E.fused_bwd_case(16, xc, xc, 0, B, hw, 330 + xc, pool=True)
    with _mode(True):
        _fused_bf16(d, 16, xc, xc, 0, True, False, True, "B fused pool bf16 xc=%d %s" % (xc, hw))


@pytest.mark.parametrize("B,hw", E.BF16_SHAPES)
def test_b_dgrad_bf16(B, hw):
    """pc_conv3x3_dgrad in bf16 mode: plain, and masked += with the producer's odd scales"""
    from popcorn_amd import ops
    d = E.dgrad_case(8, 16, 8, 8, B, hw, 340)
    E.budget_dgrad(d["g"], d["w"][:, 8:16], d["bn"]["scale"], d["prev"])
    with _mode(True):
        out = _out((B, 8, *hw))
        ops.conv3x3_dgrad(_act(d["g"]), d["w"].cuda(), 8, 8, out)
        E.assert_equal(out, E.ref_dgrad(d["g"], d["w"], 8, 8, bf16=True), "B dgrad bf16 plain %s" % (hw,))
        out = _out(None, d["prev"])
        ops.conv3x3_dgrad(_act(d["g"]), d["w"].cuda(), 8, 8, out, act=_act(d["act"]), act_bn=_bn_dev(d["bn"], False), accumulate=True)
        E.assert_equal(out, E.ref_dgrad(d["g"], d["w"], 8, 8, d["act"], d["bn"]["scale"], d["prev"], bf16=True), "B dgrad bf16 masked += %s" % (hw,))


# =========================================================================================================================================
# Family C: weight and bias gradient
# =========================================================================================================================================

@pytest.mark.parametrize("cin,cout", E.PAIRS + [(2, 8), (4, 8), (32, 8)])
@pytest.mark.parametrize("hw", [(20, 36), (19, 35)], ids=["wave", "generic"])
def test_c_wgrad(cin, cout, hw):
    """WgradBatch.conv3x3: (20, 36) the wave kernels, (19, 35) the workgroup-tile kernel; =, a second launch (run-to-run), then +="""
    from popcorn_amd import ops
    d = E.wgrad_case(cin, cout, 2, hw, 400 + cin + cout)
    E.budget_wgrad(d["x"], d["g"], d["prev_w"], d["prev_b"])
    rdw, rdb = E.ref_wgrad(d["x"], d["g"])
    xd, gd = d["x"].cuda(), d["g"].cuda()
    what = "C wgrad %d->%d %s" % (cin, cout, hw)
    for _ in range(2):
        dw, db = torch.full((cout, cin, 3, 3), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
        ops.conv3x3_wgrad(xd, gd, cout, dw=dw, db=db)
        E.assert_equal(dw, rdw, what + " dw")
        E.assert_equal(db, rdb, what + " db")
    dw, db = d["prev_w"].cuda(), d["prev_b"].cuda()
    ops.conv3x3_wgrad(xd, gd, cout, dw=dw, db=db, accumulate=True)
    E.assert_equal(dw, rdw + d["prev_w"].double(), what + " dw +=")
    E.assert_equal(db, rdb + d["prev_b"].double(), what + " db +=")


def test_c_wgrad_fused_loaders():
    """POOL2 source (40, 72); concat with a smaller, offset b; REFLECT + chmap"""
    from popcorn_amd import ops, _lib as L
    for loader, cin, cout, hw in [("pool2", 8, 16, (20, 36)), ("concat", 32, 8, (23, 35)), ("reflect", 2, 8, (58, 69)), ("reflect", 4, 8, (58, 69))]:
        c = E.conv_fwd_case(loader, cin, cout, 2, hw, 430 + cin)
        gr = 1 if loader == "reflect" else E.X_RANGE                        # (8,004 pixels of 9-bit inputs: a gradient in {-1, 0, 1} keeps the budget)
        g = E.ints((2, cout, *hw), -gr, gr, E.gen(431))
        E.budget_wgrad(c["ref_in"], g)
        rdw, rdb = E.ref_wgrad(c["ref_in"], g)
        dw, db = torch.full((cout, cin, 3, 3), NAN, device="cuda"), torch.full((cout,), NAN, device="cuda")
        kw = {"pool2": dict(a_mode=L.PC_SRC_POOL2), "concat": dict(b=c["src"].get("b").cuda() if loader == "concat" else None, b_offset=(1, 1)),
              "reflect": dict(a_mode=L.PC_SRC_REFLECT, a_pad=(14, 14), chmap=c["src"].get("chmap"), a_channels=cin)}[loader]
        ops.conv3x3_wgrad(c["src"]["a"].cuda(), g.cuda(), cout, dw=dw, db=db, **kw)
        E.assert_equal(dw, rdw, "C wgrad %s dw" % loader)
        E.assert_equal(db, rdb, "C wgrad %s db" % loader)


@pytest.mark.parametrize("B,hw", E.BF16_SHAPES)
@pytest.mark.parametrize("cin,cout", E.PAIRS)
def test_c_wgrad_bf16_single_op_and_batched_reduction(cin, cout, B, hw):
    """bf16 mode: fp32 sums of bf16 operands, no rounding point; the single op, a group of one and the first problem of a group of two
    give IDENTICAL bits -- with exact sums "the same up to association order" is "equal" --, = and +="""
    from popcorn_amd import ops
    dev = torch.device("cuda")
    d = E.wgrad_case(cin, cout, B, hw, 400 + cin + cout)
    d2 = E.wgrad_case(cin, cout, B, hw, 450 + cin + cout)
    E.budget_wgrad(d["x"], d["g"], d["prev_w"], d["prev_b"])
    rdw, rdb = E.ref_wgrad(d["x"], d["g"])
    with _mode(True):
        a, g, a2, g2 = _act(d["x"]), _act(d["g"]), _act(d2["x"]), _act(d2["g"])
        for acc in (False, True):
            want_w, want_b = (rdw + d["prev_w"].double(), rdb + d["prev_b"].double()) if acc else (rdw, rdb)

            def fresh():
                return (d["prev_w"].cuda(), d["prev_b"].cuda()) if acc else (torch.full((cout, cin, 3, 3), NAN, device=dev), torch.full((cout,), NAN, device=dev))
            dw, db = fresh()
            ops.conv3x3_wgrad(a, g, cout, dw=dw, db=db, accumulate=acc)
            what = "C wgrad bf16 %d->%d %s acc=%s" % (cin, cout, hw, acc)
            E.assert_equal(dw, want_w, what + " dw")
            E.assert_equal(db, want_b, what + " db")
            for others in ([], [(a2, g2)]):
                wb = ops.WgradBatch(dev, accumulate=acc)
                probs = [{"a": a_, "g": g_, "dw": t[0], "db": t[1]} for (a_, g_), t in zip([(a, g)] + others, [fresh(), fresh()])]
                wb.conv3x3_group(probs, cout)
                wb.finish()
                E.assert_equal(probs[0]["dw"], want_w, what + " dw, group of %d" % len(probs))
                E.assert_equal(probs[0]["db"], want_b, what + " db, group of %d" % len(probs))


# =========================================================================================================================================
# Family D: transposed conv
# =========================================================================================================================================

def _convt_all(c, B, hw, bf16, what):
    from popcorn_amd import ops
    d = E.convt_case(c, B, hw, 500 + c)                                     # (asserts the budget of all four sums)
    H, W = hw
    xd, wd, gd = _act(d["x"]), d["w"].cuda(), _act(d["g"])
    out = _out((B, c, 2 * H, 2 * W))
    ops.convt2x2(xd, wd, d["bias"].cuda(), out=out)
    E.assert_equal(out, E.ref_convt(d["x"], d["w"], d["bias"], bf16), what + " forward")
    rgx, rdw, rdb = E.ref_convt_bwd(d["x"], d["w"], d["g"], bf16=bf16)
    rgxm = E.ref_convt_bwd(d["x"], d["w"], d["g"], d["x"], d["bn"]["scale"], bf16=bf16)[0]
    bnd = _bn_dev(d["bn"], False)
    gx, gxm = _out((B, c, H, W)), _out((B, c, H, W))
    ops.convt2x2_dgrad(gd, wd, gx)
    ops.convt2x2_dgrad(gd, wd, gxm, act=xd, act_bn=bnd)
    E.assert_equal(gx, rgx, what + " dgrad")
    E.assert_equal(gxm, rgxm, what + " dgrad masked")
    for _ in range(2):
        dw, db = torch.full((c, c, 2, 2), NAN, device="cuda"), torch.full((c,), NAN, device="cuda")
        ops.convt2x2_wgrad(xd, gd, dw=dw, db=db)
        E.assert_equal(dw, rdw, what + " dw")
        E.assert_equal(db, rdb, what + " db")
    return d, (xd, wd, gd, bnd), (rgxm, rdw, rdb)


def _convt_fused(c, B, hw, dev_ops, refs, what):
    from popcorn_amd import ops
    xd, wd, gd, bnd = dev_ops
    gx = _out((B, c, *hw))
    dw, db = torch.full((c, c, 2, 2), NAN, device="cuda"), torch.full((c,), NAN, device="cuda")
    wb = ops.WgradBatch(torch.device("cuda"))
    wb.convt2x2_bwd_group([{"x": xd, "g": gd, "w": wd, "out": gx, "dw": dw, "db": db, "x_bn": bnd}])
    wb.finish()
    E.assert_equal(gx, refs[0], what + " fused gx")
    E.assert_equal(dw, refs[1], what + " fused dw")
    E.assert_equal(db, refs[2], what + " fused db")


@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("hw", [(9, 21), (16, 32)])
def test_d_convt(c, hw):
    """forward, dgrad plain and with the producer's epilogue (x holds exact zeros), wgrad twice; at (16, 32) the fused backward"""
    what = "D convt C=%d %s" % (c, hw)
    d, dev_ops, refs = _convt_all(c, 2, hw, False, what)
    if hw == (16, 32):
        _convt_fused(c, 2, hw, dev_ops, refs, what)


@pytest.mark.parametrize("c", [8, 16])
@pytest.mark.parametrize("B,hw", [(3, (9, 21)), (2, (16, 32))])
def test_d_convt_bf16(c, B, hw):
    """bf16 mode: the forward output and the data gradients are rounded once, after bias / mask / scale; the fused backward at any
    geometry"""
    what = "D convt bf16 C=%d %s" % (c, hw)
    d = E.convt_case(c, B, hw, 500 + c)
    E.assert_bf16_coverage(E.ref_convt(d["x"], d["w"], d["bias"]), what + " forward")
    E.assert_bf16_coverage(E.ref_convt_bwd(d["x"], d["w"], d["g"], d["x"], d["bn"]["scale"])[0], what + " gx")
    with _mode(True):
        d, dev_ops, refs = _convt_all(c, B, hw, True, what)
        _convt_fused(c, B, hw, dev_ops, refs, what)


# =========================================================================================================================================
# Family E: composed Up
# =========================================================================================================================================

def _up_cases():
    out = [pytest.param(Cs, hw, None, id="%d-%dx%d" % (Cs, hw[0], hw[1])) for Cs, hw in E.UP_GEOMS]
    return out + [pytest.param(Cs, hw, wd, id="%d-%dx%d-wide_%s" % (Cs, hw[0], hw[1], wd)) for Cs, hw in E.UP_GEOMS[:3] for wd in ("x", "w")]


@pytest.mark.parametrize("Cs,hw,wide", _up_cases())
def test_e_up_forward(Cs, hw, wide, conv_form):
    """conv3x3(cat[skip, ConvTranspose2d(z)]) from the low-resolution map, every operand dense, both forms; with and without ReLU"""
    from popcorn_amd import ops
    d = E.up_case(Cs, hw, 600 + Cs + hw[0], wide=wide)
    sd, zd, out = d["skip"].cuda(), d["z"].cuda(), torch.full((2, 8, *hw), NAN, device="cuda")
    assert ops.conv3x3_up_fwd_ok(sd, zd, out)
    for relu in (True, False):
        out.fill_(NAN)
        ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd, "w": d["w"].cuda(), "wt": d["wt"].cuda(), "bt": d["bt"].cuda(), "bn": _bn_dev(d["bn"]), "out": out}],
                                 relu=relu)
        E.assert_equal(out, E.up_forward_reference(d, relu), "E up fwd Cs=%d %s wide=%s relu=%s form=%d" % (Cs, hw, wide, relu, conv_form))


@pytest.mark.parametrize("deferred", [False, True], ids=["direct", "deferred"])
@pytest.mark.parametrize("Cs,hw", E.UP_BWD)
def test_e_up_backward(Cs, hw, deferred):
    """pc_conv3x3_up_bwd_group (up_bwd_kernel<8|16, 64|128>, reduction, chain rule; fp32 MFMA only), every operand dense: gz with the
    epilogue of z's producer, dw[:, Cs:], dwt, dbt -- all of them sums of many terms -- equal float64 autograd; dw[:, :Cs] stays"""
    from popcorn_amd import ops
    d = E.up_case(Cs, hw, 600 + Cs + hw[0])
    rgz, rdw, rdwt, rdbt = E.up_backward_reference(d)
    B, (H, W), C = 2, hw, Cs
    sd, zd, wd, wtd, btd = (d[k].cuda() for k in ("skip", "z", "w", "wt", "bt"))
    y = torch.empty(B, 8, H, W, device="cuda")
    slot = ops.conv3x3_up_fwd_group([{"skip": sd, "z": zd, "w": wd, "wt": wtd, "bt": btd, "bn": _bn_dev(d["bn"]), "out": y}])[0]
    gz = torch.full((B, C, H // 2, W // 2), NAN, device="cuda")
    dw = torch.full((8, Cs + C, 3, 3), 7.0, device="cuda")
    dwt, dbt = torch.full((C, C, 2, 2), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    pr = {"g": d["G"].cuda(), "z": zd, "z_bn": _bn_dev(d["z_bn"], False), "gz": gz, "w": wd, "wt": wtd, "bt": btd, "fwd_ws": slot, "dw": dw,
          "dwt": dwt, "dbt": dbt}
    assert ops.conv3x3_up_bwd_ok(pr["g"], pr["z"], pr["gz"])
    if deferred:
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.up_bwd_group([pr])
        wb.finish()
    else:
        ops.conv3x3_up_bwd_group([pr])
    torch.cuda.synchronize()
    what = "E up bwd Cs=%d %s %s" % (Cs, hw, "deferred" if deferred else "direct")
    E.assert_equal(gz, rgz, what + " gz")
    E.assert_equal(dw[:, Cs:], rdw, what + " dw[:, Cs:]")
    assert bool((dw[:, :Cs] == 7.0).all())
    E.assert_equal(dwt, rdwt, what + " dwt")
    E.assert_equal(dbt, rdbt, what + " dbt")


# =========================================================================================================================================
# Family F: the whole 32 x 32 level
# =========================================================================================================================================

def _level2_fwd(d):
    from popcorn_amd import ops
    c1, c2, u2 = _out((2, 16, 32, 32)), _out((2, 16, 32, 32)), _out((2, 16, 64, 64))
    xd = _act(d["xf"])
    assert ops.level2_fwd_ok(xd, u2)
    ops.level2_fwd_group([{"x": xd, "w1": d["w1"].cuda(), "bn1": _bn_dev(d["bn1"]), "w2": d["w2"].cuda(), "bn2": _bn_dev(d["bn2"]),
                           "wt": d["wt"].cuda(), "bt": d["bt"].cuda(), "c1": c1, "c2": c2, "u2": u2}])
    torch.cuda.synchronize()
    return c1, c2, u2


def _level2_bwd(d, fused):
    """fused: WgradBatch.level2_bwd_group; else the two conv3x3_bwd_group launches it replaces (bf16 mode)"""
    from popcorn_amd import ops
    t = {k: torch.full(sh, NAN, device="cuda") for k, sh in (("dw1", (16, 16, 3, 3)), ("db1", (16,)), ("dw2", (16, 16, 3, 3)), ("db2", (16,)))}
    out = _out(None, d["prev"])
    g2, c1, x, act = _act(d["g2"]), _act(d["c1b"]), _act(d["x"]), _act(d["act"])
    w1, w2, bn1, abn = d["w1"].cuda(), d["w2"].cuda(), _bn_dev(d["bn1"], False), _bn_dev(d["abn"], False)
    wb = ops.WgradBatch(torch.device("cuda"))
    if fused:
        assert ops.level2_bwd_ok(g2, c1, x, act, out)
        wb.level2_bwd_group([dict(t, g2=g2, c1=c1, x=x, act=act, w1=w1, w2=w2, bn1=bn1, act_bn=abn, out=out)])
    else:
        g1 = _out((2, 16, 32, 32))
        wb.conv3x3_bwd_group([{"g": g2, "x": c1, "w": w2, "out": g1, "dw": t["dw2"], "db": t["db2"], "x_bn": bn1}], 16, 0)
        wb.conv3x3_bwd_group([{"g": g1, "x": x, "w": w1, "out": out, "dw": t["dw1"], "db": t["db1"], "pool_act": act, "x_bn": abn}], 16, 0)
    wb.finish()
    torch.cuda.synchronize()
    return out, t["dw1"], t["db1"], t["dw2"], t["db2"]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_f_level2_forward_and_backward(bf16):
    """both convs of the 32 x 32 level and its transposed conv in one launch, the backward of both convs in one launch: c1, c2, u2, the
    scattered out +=, dw1 / db1 / dw2 / db2 equal the float64 chain (bf16: rounded once per stage / at the intermediate gradient); in
    bf16 mode also the launches level2_bwd_cl_kernel replaces -- with exact sums their weight gradients are EQUAL, not merely close"""
    d = E.level2_case(700)
    rf = E.level2_forward_reference(d, bf16)
    rb = E.level2_backward_reference(d, bf16)
    if bf16:
        E.assert_bf16_coverage(E.level2_forward_reference(d, False)[0], "F c1")
    with _mode(bf16):
        for name, got, want in zip(("c1", "c2", "u2"), _level2_fwd(d), rf):
            E.assert_equal(got, want, "F level2 forward %s bf16=%s" % (name, bf16))
        if bf16:                                                           # the three launches level2_fwd_cl_kernel replaces
            from popcorn_amd import ops
            c1 = ops.conv3x3_raw(_act(d["xf"]), d["w1"].cuda(), _bn_dev(d["bn1"]))
            c2 = ops.conv3x3_raw(c1, d["w2"].cuda(), _bn_dev(d["bn2"]))
            u2 = ops.convt2x2(c2, d["wt"].cuda(), d["bt"].cuda())
            for name, got, want in zip(("c1", "c2", "u2"), (c1, c2, u2), rf):
                E.assert_equal(got, want, "F level2 forward, layer by layer, %s bf16" % name)
        for fused in ((True, False) if bf16 else (True,)):
            for name, got, want in zip(("out", "dw1", "db1", "dw2", "db2"), _level2_bwd(d, fused), rb):
                E.assert_equal(got, want, "F level2 backward %s bf16=%s fused=%s" % (name, bf16, fused))


# =========================================================================================================================================
# Family G: the head
# =========================================================================================================================================

@pytest.mark.parametrize("case", E.HEAD_CASES, ids=lambda c: "%dx%d-%s-%s" % (E.HEAD_SHAPES[c[0]][1], E.HEAD_SHAPES[c[0]][2], c[1], "sparse" if c[2] else "dense"))
def test_g_head(case, head_mode):
    """ops.head_fwd / ops.head_bwd, dense and sparse, admin mask and census index, all four gradient routes, in the three forms: the
    scale map, popdensemap, popcount, g_feat and the eight gradients equal the float64 chain bit for bit; the exported decisions equal
    pre > 0 of the reference, exact zeros included (fp32 forms: the export exists there); a second launch (run-to-run); the deferred
    reduction (= and +=).  Excluded by name: scale map / popdensemap outside the selection of the sparse form (not written)."""
    from popcorn_amd import ops
    si, variant, sparse = case
    shape = E.HEAD_SHAPES[si]
    B, H, W, Hp, Wp, py, px = shape
    bf16 = head_mode == "bf16"
    d = E.head_case(shape, E.HEAD_SEED, wide=variant, sparse=sparse)
    if bf16:
        d["feat"] = E.rbf(d["feat"])                                       # the feature map arrives rounded from its producers
    r = E.head_reference(d, shape, bf16=bf16)                              # (asserts the budget of every sum)
    if variant is True and head_mode == "split":
        h = torch.cat([a.reshape(-1) for a in r["acts"][1:]])
        assert float((E.sig_bits(h) > 8).double().mean()) >= 0.25
    ht = [t.cuda() for t in d["ht"]]
    mask = d["mask"]
    kw = dict(mask=mask.to(torch.uint8).cuda() if sparse else None, admin_mask=d["admin"].cuda(), census_idx=d["census"].cuda())
    gkw = dict(g_popcount=d["g_pc"].cuda(), g_popdense=d["g_pd"].cuda(), g_scale_map=d["g_sm"].cuda(),
               g_scale_const=torch.tensor([d["g_const"]], device="cuda"))
    feat, bld = _act(d["feat"]), d["building"].cuda()
    what = "G head %s %s [%s]" % (case, shape[:3], head_mode)
    s_map, pd, pc = ops.head_fwd(feat, py, px, H, W, ht, bld, **kw)
    E.assert_equal(s_map.cpu()[mask], r["scale_map"][mask], what + " scale map")
    E.assert_equal(pd.cpu()[mask], r["popdense"][mask], what + " popdensemap")
    E.assert_equal(pc, r["popcount"], what + " popcount")
    buf = None if bf16 else ops.head_decision_buffer(B, H, W, "cuda")
    grads, g_feat = ops.head_bwd(feat, py, px, H, W, ht, bld, decisions=buf, **kw, **gkw)
    E.assert_equal(g_feat, r["g_feat"], what + " g_feat")
    for n, got, want in zip(E.HEAD_NAMES, grads, r["grads"]):
        E.assert_equal(got, want.view(got.shape), "%s d(%s)" % (what, n))
    if buf is not None:
        hidden, outd = ops.decode_head_decisions(buf, mask)
        for l in range(3):
            want = r["pres"][l] > 0
            assert torch.equal(hidden[l], want), "%s decisions of layer %d: %d differ" % (what, l, int((hidden[l] != want).sum()))
        assert torch.equal(outd, r["pres"][3][0] > 0), what + " output decision"
    grads2, g_feat2 = ops.head_bwd(feat, py, px, H, W, ht, bld, **kw, **gkw)
    assert torch.equal(g_feat2, g_feat) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    for acc in (False, True):
        tgt = [torch.full_like(t, 4.0) for t in ht]                        # (|prev| = 4: nothing next to sums of 2^10 and more quanta)
        hp, g_feat3 = ops.head_bwd(feat, py, px, H, W, ht, bld, grads=tgt, accumulate=acc, defer_reduce=True, **kw, **gkw)
        assert isinstance(hp, ops.HeadPartials) and torch.equal(g_feat3, g_feat)
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.head_reduce(hp)
        wb.finish()
        for i, (got, want) in enumerate(zip(tgt, r["grads"])):
            want = want.view(got.shape).clone() + (4.0 if acc else 0.0)
            if i in (6, 7) and acc:
                want.view(-1)[want.numel() // 2:] = 4.0                    # (+= leaves the structurally zero second row alone)
            E.assert_equal(got, want, "%s deferred %s d(%s)" % (what, "+=" if acc else "=", E.HEAD_NAMES[i]))
