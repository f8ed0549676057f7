"""Self-tests of tests/exact_arith.py (no GPU): under the budget every accumulation order of fp32 torch equals the float64 reference bit
for bit (and a broken budget shows the orders disagreeing); the equality bar rejects planted defects on the families' own inputs; the
builders' outputs meet the budget and every coverage condition for every family and shape tests/test_gpu_exact_arith.py runs."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import exact_arith as E


def _chunks(c, n=4):
    return [slice(i, min(i + n, c)) for i in range(0, c, n)][::-1]


def _orders(op, a, b, ca, cb, flip):
    """fp32 evaluations of op(a, b) whose reduction runs over axis ca of a / cb of b: a permutation of that axis, its chunks of 4 in
    reversed order summed one by one, and ``flip`` (the spatially flipped operands, flipped back)"""
    n = a.shape[ca]
    perm = torch.randperm(n, generator=E.gen(5))
    o1 = op(a.index_select(ca, perm), b.index_select(cb, perm))
    o2 = None
    for s in _chunks(n):
        idx = torch.arange(n)[s]
        t = op(a.index_select(ca, idx), b.index_select(cb, idx))
        o2 = t if o2 is None else o2 + t
    return [o1, o2, flip(op)]


def _all_equal(outs, ref64):
    return all(torch.equal(o.double(), ref64) for o in outs)


def _conv(x, w):
    return F.conv2d(x, w, padding=1)


def _dconv(g, w):
    return F.conv_transpose2d(g, w, padding=1)


@pytest.mark.parametrize("broken", [False, True])
def test_order_independence_of_the_conv_family(broken):
    """conv forward, data gradient, weight gradient and transposed conv (19 x 35, 16 channels): three accumulation orders in fp32
    equal float64 bit for bit under the budget; with operands of 20 bits (the budget broken on purpose) the orders disagree"""
    g = E.gen(11)
    r = 2 ** 20 if broken else E.X_RANGE
    x, w, gr = E.ints((2, 16, 19, 35), -r, r, g), E.ints((16, 16, 3, 3), -r if broken else -E.W_RANGE, r if broken else E.W_RANGE, g), E.ints((2, 16, 19, 35), -r, r, g)
    wt, xs = E.ints((16, 16, 2, 2), -r if broken else -E.W_RANGE, r if broken else E.W_RANGE, g), E.ints((2, 16, 9, 21), -r, r, g)
    f2 = lambda t: torch.flip(t, (2, 3))  # noqa: E731
    fams = {
        "forward": (_orders(_conv, x, w, 1, 1, lambda op: f2(op(f2(x), f2(w)))), _conv(x.double(), w.double())),
        "dgrad": (_orders(_dconv, gr, w, 1, 0, lambda op: f2(op(f2(gr), f2(w)))), _dconv(gr.double(), w.double())),
        "wgrad": (_orders(lambda a, b: torch.nn.grad.conv2d_weight(a, (16, 16, 3, 3), b, padding=1), x, gr, 0, 0,
                          lambda op: f2(op(f2(x), f2(gr)))), E.ref_wgrad(x, gr)[0]),
        "convt": (_orders(lambda a, b: F.conv_transpose2d(a, b, stride=2), xs, wt, 1, 0,
                          lambda op: f2(op(f2(xs), f2(wt)))), F.conv_transpose2d(xs.double(), wt.double(), stride=2)),
    }
    if not broken:
        E.budget_conv_fwd(x, w)
        E.budget_dgrad(gr, w)
        E.budget_wgrad(x, gr)
        E.budget_convt(xs, wt, torch.zeros(16))
    for name, (outs, ref) in fams.items():
        if broken:
            with pytest.raises(AssertionError):
                E.assert_budget(ref.abs(), 1.0)
            assert not _all_equal(outs, ref), name + ": beyond the budget the orders still agree -- the budget is not what makes them agree"
        else:
            assert _all_equal(outs, ref), name


@pytest.mark.parametrize("broken", [False, True])
def test_order_independence_of_the_head_chain(broken):
    """the head's four 1x1 products and the weight-gradient sums over the pixels, fp32 matmuls in three orders"""
    shape = E.HEAD_SHAPES[0]
    d = E.head_case(shape, E.HEAD_SEED)
    if broken:
        d["feat"] = d["feat"] * 2.0 ** 16 + E.ints(d["feat"].shape, -2 ** 15, 2 ** 15, E.gen(3))
        d["ht"][0] = d["ht"][0] * 2.0 ** 12 + E.ints(d["ht"][0].shape, -2 ** 11, 2 ** 11, E.gen(4))
        with pytest.raises(AssertionError):
            E.head_reference(d, shape)
    else:
        ref = E.head_reference(d, shape)
    B, H, W, Hp, Wp, py, px = shape
    x = d["feat"][:, :, py:py + H, px:px + W].permute(1, 0, 2, 3).reshape(16, -1)
    pres64, acts64, _ = E.head_chain(x, d["ht"])
    h = x
    for l in range(4):
        wl = d["ht"][2 * l].view(d["ht"][2 * l].shape[0], -1)
        mm = lambda a, b: a @ b  # noqa: E731
        outs = _orders(mm, wl, h, 1, 0, lambda op: torch.flip(op(wl, torch.flip(h, (1,))), (1,)))
        outs = [o + d["ht"][2 * l + 1].view(-1, 1) for o in outs]
        want = pres64[l] if l < 3 else (d["ht"][6].double().view(2, -1) @ acts64[3] + d["ht"][7].double().view(-1, 1))
        if broken and l == 0:
            assert not _all_equal(outs, want)
            return
        assert _all_equal(outs, want), l
        h = torch.relu(outs[0])
    grads64, gx64, gs = E.head_backward(x, d["ht"], ref["g_out"], parts=True)
    for l in range(3):                                                    # weight gradients: sums over the pixels
        a, b = gs[l].float(), acts64[l].float()
        outs = _orders(lambda p, q: p @ q.t(), a, b, 1, 1, lambda op: op(torch.flip(a, (1,)), torch.flip(b, (1,))))
        assert _all_equal(outs, grads64[2 * l].view(outs[0].shape)), l


# ---- planted defects --------------------------------------------------------------------------------------------------------------------

def _rejected(got, expected):
    return E.mismatch(got, expected) is not None


def test_equality_rejects_planted_index_defects():
    """on the inputs of family A (8 -> 8 at 19 x 35, two 32-column tiles, the last ragged): a tap dropped at the last column, a halo
    column counted twice at the tile seam, one K-chunk added twice -- in ONE image, ONE output channel each"""
    c = E.conv_fwd_case("plain", 8, 8, 2, (19, 35), 21)
    x, w, bn = c["ref_in"], c["w"], c["bn"]
    good = E.ref_conv_fwd(x, w, bn)
    assert not _rejected(good.float(), c["expected"])
    w_tap = torch.zeros_like(w)
    w_tap[3, :, :, 0] = w[3, :, :, 0]                               # the left taps (they read column W - 2) of output channel 3
    part = F.conv2d(x.double(), w_tap.double(), padding=1)
    dropped = F.conv2d(x.double(), w.double(), padding=1)
    dropped[..., 34] -= part[..., 34]
    assert _rejected(torch.relu(E.bn_apply(dropped, bn)), c["expected"])
    doubled = F.conv2d(x.double(), w.double(), padding=1)
    doubled[..., 32] += part[..., 32]                               # column 31, the halo of the second tile, counted twice
    assert _rejected(torch.relu(E.bn_apply(doubled, bn)), c["expected"])
    wk = torch.zeros_like(w)
    wk[5, 4:8] = w[5, 4:8]
    chunk = F.conv2d(x.double(), w.double(), padding=1) + F.conv2d(x.double(), wk.double(), padding=1)
    assert _rejected(torch.relu(E.bn_apply(chunk, bn)), c["expected"])
    # the same three in the weight gradient (family C) and the data gradient (family B)
    d = E.wgrad_case(8, 8, 2, (19, 35), 22)
    dw, _ = E.ref_wgrad(d["x"], d["g"])
    gcut = d["g"].clone()
    gcut[:, :, :, 34] = 0
    dw_cut, _ = E.ref_wgrad(d["x"], gcut)
    bad = dw.clone()
    bad[:, :, :, 0] = dw_cut[:, :, :, 0]
    assert _rejected(bad, dw)
    b = E.dgrad_case(8, 8, 0, 8, 2, (19, 35), 23)
    gx = E.ref_dgrad(b["g"], b["w"], 0, 8, b["act"], b["bn"]["scale"], b["prev"])
    g2 = b["g"].clone()
    g2[:, :4] *= 2                                                  # the first K-chunk of the gradient channels added twice
    assert _rejected(E.ref_dgrad(g2, b["w"], 0, 8, b["act"], b["bn"]["scale"], b["prev"]), gx)


def test_equality_rejects_planted_rounding_defects():
    """bf16 mode, family A inputs: the rounding point moved across the BN scale, truncation, round-half-up; family B: a gradient rounded
    once too often"""
    c = E.conv_fwd_case("concat", 32, 8, 1, (37, 53), 31, bf16=True)
    x, w, bn = c["ref_in"], c["w"], c["bn"]
    E.assert_bf16_coverage(c["exact"])
    y = F.conv2d(x.double(), w.double(), padding=1)
    moved = E.rbf(torch.relu(E.rbf(y) * bn["scale"].view(1, -1, 1, 1) + bn["shift"].view(1, -1, 1, 1)))
    assert _rejected(moved, c["expected"])
    print("rounding before the scale instead of after changes %.1f %% of the elements" % (100 * float((moved != c["expected"]).double().mean())))
    assert _rejected(E.rbf_trunc(c["exact"]), c["expected"]) and _rejected(E.rbf_half_up(c["exact"]), c["expected"])
    pow2 = dict(bn, scale=torch.pow(torch.tensor(2.0, dtype=torch.double), torch.arange(8).double() - 4))       # 2^k scales cannot see it
    pow2["shift"] = torch.zeros(8, dtype=torch.double)
    assert torch.equal(E.rbf(torch.relu(E.bn_apply(E.rbf(y), pow2))), E.rbf(torch.relu(E.bn_apply(y, pow2))))
    b = E.dgrad_case(8, 8, 0, 8, 1, (37, 53), 32)
    want = E.ref_dgrad(b["g"], b["w"], 0, 8, b["act"], b["bn"]["scale"], None, bf16=True)
    twice = E.rbf(E.rbf(F.conv_transpose2d(b["g"].double(), b["w"].double(), padding=1)) * (b["act"] > 0).double() * b["bn"]["scale"].view(1, -1, 1, 1))
    assert _rejected(twice, want)
    h = E.head_case(E.HEAD_SHAPES[0], E.HEAD_SEED, wide="g")
    r = E.head_reference(h, E.HEAD_SHAPES[0], bf16=True)
    fp = E.head_reference(h, E.HEAD_SHAPES[0], bf16=False)
    assert _rejected(E.rbf(fp["g_feat"]), r["g_feat"]), "rounding g_feat once at the end is not the mode's definition"


def test_equality_rejects_a_wrong_relu_comparison():
    """>= in place of > in a ReLU mask: the data gradient (act holds exact zeros), the pool scatter, the head's decisions"""
    b = E.dgrad_case(8, 8, 0, 8, 2, (19, 35), 41)
    assert _rejected(E.ref_dgrad(b["g"], b["w"], 0, 8, b["act"], b["bn"]["scale"], b["prev"], ge=True),
                     E.ref_dgrad(b["g"], b["w"], 0, 8, b["act"], b["bn"]["scale"], b["prev"]))
    p = E.dgrad_case(16, 8, 0, 8, 2, (20, 36), 42, pool=True)
    assert _rejected(E.ref_dgrad_pool(p["g"], p["w"], 0, 8, p["act"], p["bn"]["scale"], p["prev"], ge=True),
                     E.ref_dgrad_pool(p["g"], p["w"], 0, 8, p["act"], p["bn"]["scale"], p["prev"]))
    shape = E.HEAD_SHAPES[0]
    h = E.head_case(shape, E.HEAD_SEED)
    good, bad = E.head_reference(h, shape), E.head_reference(h, shape, ge=True)
    assert _rejected(bad["g_feat"], good["g_feat"])
    assert any(_rejected(a, b_) for a, b_ in zip(bad["grads"], good["grads"]))


# ---- budget and coverage of every case the GPU file runs --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", E.A_BF16, ids=lambda c: "%s-%d-%d-%d-%dx%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1]))
def test_family_a_bf16_inputs_meet_budget_and_coverage(case):
    loader, cin, cout, B, hw = case
    c = E.conv_fwd_case(loader, cin, cout, B, hw, 100 + cin + cout, bf16=True)
    r, to, te = E.assert_bf16_coverage(c["exact"], str(case))
    print(case, "rounded %.3f, odd ties %.3f, even ties %.3f, exact-zero pre-activations %.4f" % (r, to, te, E.relu_coverage(c["pre"])))


def test_family_a_fp32_and_wide_inputs_meet_the_budget():
    for cin, cout in E.PAIRS + [(2, 8), (4, 8), (32, 8)]:
        E.conv_fwd_case("plain", cin, cout, 2, (19, 35), 100 + cin + cout)
    for cin, cout in E.PAIRS:
        for wide in (None, "x", "w"):
            c = E.conv_fwd_case("plain", cin, cout, 2, (20, 36), 100 + cin + cout, wide=wide)
            if wide:
                op = c["ref_in"] if wide == "x" else c["w"]
                assert float((E.sig_bits(op) > 8).double().mean()) > 0.5 and float(E.sig_bits(op).max()) <= 12
    E.conv_fwd_case("pool2", 8, 16, 2, (20, 36), 131)
    E.conv_fwd_case("concat", 32, 8, 2, (23, 35), 132)
    for cin in (2, 4):
        E.conv_fwd_case("reflect", cin, 8, 2, (58, 69), 134)


@pytest.mark.parametrize("B,hw", E.BF16_SHAPES)
def test_families_b_c_d_inputs_meet_budget_and_coverage(B, hw):
    """the data-gradient outputs of bf16 mode are activation-gradient tensors: the rounding coverage applies to them; ``act`` / ``x``
    (the mask sources) hold exact zeros (asserted by the builders)"""
    for name, (gc, xc, cin_total, c0) in E.B_BF16_FUSED.items():
        up = "up_half" in name
        d = E.fused_bwd_case(gc, xc, cin_total, c0, B, hw, 300 + gc + cin_total, up_half=up)
        gx, _, _ = E.fused_bwd_reference(d, c0, masked=not up, acc="accumulate" in name)
        E.assert_bf16_coverage(gx, "B fused " + name)
    for Bp, hwp in E.BF16_POOL_SHAPES:
        for xc in (8, 16):
            d = E.fused_bwd_case(16, xc, xc, 0, Bp, hwp, 330 + xc, pool=True)
            gx, _, _ = E.fused_bwd_reference(d, 0, pool=True)
            E.assert_bf16_coverage(gx[gx != d["prev"].double()], "B fused pool")       # (three of four positions keep their previous value)
    b = E.dgrad_case(8, 16, 8, 8, B, hw, 340)
    E.budget_dgrad(b["g"], b["w"][:, 8:16], b["bn"]["scale"], b["prev"])
    E.assert_bf16_coverage(E.ref_dgrad(b["g"], b["w"], 8, 8, b["act"], b["bn"]["scale"], b["prev"]), "B dgrad")
    for cin, cout in E.PAIRS:
        w = E.wgrad_case(cin, cout, B, hw, 400 + cin + cout)
        E.budget_wgrad(w["x"], w["g"], w["prev_w"], w["prev_b"])
    for c in (8, 16):
        t = E.convt_case(c, B, (hw[0] // 2, hw[1] // 2), 500 + c)
        E.assert_bf16_coverage(E.ref_convt(t["x"], t["w"], t["bias"]), "D convt forward")
        E.assert_bf16_coverage(E.ref_convt_bwd(t["x"], t["w"], t["g"], t["x"], t["bn"]["scale"])[0], "D convt gx")


@pytest.mark.parametrize("case", E.HEAD_CASES, ids=lambda c: "%dx%d-%s-%s" % (E.HEAD_SHAPES[c[0]][1], E.HEAD_SHAPES[c[0]][2], c[1], "sparse" if c[2] else "dense"))
def test_family_g_inputs_meet_budget_and_coverage(case):
    """base variant: >= 0.5 % of the pre-activations of every layer are exactly 0 and the output decision takes both signs; wide
    variant (split form, bf16): >= 25 % of the hidden units carry more than 8 significant bits and the rounding coverage holds for
    the hidden layers; variant "g": the rounding coverage holds for g_feat"""
    si, variant, sparse = case
    shape = E.HEAD_SHAPES[si]
    d = E.head_case(shape, E.HEAD_SEED, wide=variant, sparse=sparse)
    for bf16 in (False, True):
        r = E.head_reference(d, shape, bf16=bf16)                      # (asserts the budget of every sum)
        assert 0.2 < float((r["pres"][3] > 0).double().mean()) < 0.8 or bf16
    r = E.head_reference(d, shape)
    if variant is True:
        h = torch.cat([a.reshape(-1) for a in r["acts"][1:]])
        assert float((E.sig_bits(h) > 8).double().mean()) >= 0.25
        E.assert_bf16_coverage(torch.cat([torch.relu(p).reshape(-1) for p in r["pres"][:3]]), "hidden layers")
    else:
        for l, p in enumerate(r["pres"]):
            E.assert_relu_coverage(p, "head layer %d" % l)
    if variant == "g":
        E.assert_bf16_coverage(r["g_feat"], "g_feat")
    print(case, "worst sum 2^%.1f quanta" % torch.log2(torch.tensor(r["worst"])).item())


def test_rounding_helpers_and_tie_classes():
    v = torch.tensor([257.0, 259.0, 258.0, 1.0, -257.0, -259.0, 0.0, 256.5])      # 257 = tie, even mantissa (-> 256); 259 = tie, odd (-> 260)
    assert E.rbf(v).tolist() == [256.0, 260.0, 258.0, 1.0, -256.0, -260.0, 0.0, 256.0]
    assert E.rbf_trunc(v).tolist() == [256.0, 258.0, 258.0, 1.0, -256.0, -258.0, 0.0, 256.0]
    assert E.rbf_half_up(v).tolist() == [258.0, 260.0, 258.0, 1.0, -258.0, -260.0, 0.0, 256.0]
    r, to, te = E.bf16_coverage(v.double())
    assert (r, to, te) == (5 / 7, 2 / 7, 2 / 7)
    assert E.quantum(torch.tensor([6.0, 0.0, 20.0])) == 2.0 and E.quantum(torch.tensor([0.75, 3.0])) == 0.25
    assert E.sig_bits(torch.tensor([0.0, 1.0, 6.0, 257.0, 0.375])).tolist() == [0.0, 1.0, 2.0, 9.0, 2.0]
    with pytest.raises(AssertionError):
        E.assert_budget(torch.tensor([2.0 ** 22 + 1]), 1.0)
    E.assert_budget(torch.tensor([2.0 ** 22]), 1.0)
    bn = E.bn_odd(16, E.gen(1))
    odd = bn["gamma"] / E._elem_quantum(bn["gamma"]).float() * torch.sign(bn["gamma"]) * torch.sign(bn["gamma"])
    assert set(odd.abs().tolist()) <= {1.0, 3.0, 5.0} and len({float(x) for x in bn["gamma"]}) == 16
    with pytest.raises(AssertionError):
        E.assert_equal(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0], dtype=torch.double))
    with pytest.raises(AssertionError):
        E.assert_equal(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 0.0], dtype=torch.double))
    E.assert_equal(torch.tensor([1.0, -0.0]), torch.tensor([1.0, 0.0], dtype=torch.double))


def test_families_e_f_inputs_meet_the_budget_and_order_independence():
    """composed Up (forward in both forms incl. the wide variants, backward) and the 32 x 32 level: the builders assert the budget of
    every sum on the chain of absolute values; the composed evaluation (w and wt multiplied first, as the kernels do) gives the same
    bits as the staged one in fp32"""
    for Cs, hw in E.UP_BWD:
        d = E.up_case(Cs, hw, 600 + Cs + hw[0])
        want = E.up_forward_reference(d, relu=False)
        E.up_backward_reference(d)
        up32 = F.conv_transpose2d(d["z"], d["wt"], d["bt"], stride=2)
        y32 = F.conv2d(torch.cat([d["skip"], up32], 1), d["w"], padding=1)
        y32 = y32 * d["bn"]["scale"].float().view(1, -1, 1, 1) + d["bn"]["shift"].float().view(1, -1, 1, 1)
        assert torch.equal(y32.double(), want)
        # composed: one 3x3 conv over the zero-stuffed z per sub-pixel weight = conv(skip) + conv(up without bias) + bias through the taps
        y_split = (F.conv2d(d["skip"], d["w"][:, :Cs], padding=1) + F.conv2d(F.conv_transpose2d(d["z"], d["wt"], stride=2), d["w"][:, Cs:], padding=1)
                   + F.conv2d(d["bt"].view(1, -1, 1, 1).expand(2, Cs, *hw).contiguous(), d["w"][:, Cs:], padding=1))
        y_split = y_split * d["bn"]["scale"].float().view(1, -1, 1, 1) + d["bn"]["shift"].float().view(1, -1, 1, 1)
        assert torch.equal(y_split.double(), want)
    for Cs, hw in E.UP_GEOMS[:3]:
        for wide in ("x", "w"):
            d = E.up_case(Cs, hw, 600 + Cs + hw[0], wide=wide)
            op = torch.cat([d["z"].reshape(-1), d["skip"].reshape(-1)]) if wide == "x" else d["w"]
            assert float((E.sig_bits(op) > 8).double().mean()) > 0.5
    d = E.level2_case(700)
    for bf16 in (False, True):
        E.level2_forward_reference(d, bf16)
        E.level2_backward_reference(d, bf16)
    E.assert_bf16_coverage(E.level2_forward_reference(d, False)[0], "F c1")
    E.assert_relu_coverage(d["c1b"], "F c1 mask")


@pytest.mark.parametrize("variant", [False, True, "g"])
def test_head_reference_is_the_oracle_head_with_its_bf16_rounding_points(variant):
    """the helper's explicit chain against oracle/popcorn_oracle.py (head_forward under bf16_mode, torch autograd through _rf / _rb) in
    float64 on the family's own operands: forward pre-activations' consequences (the scale), all eight gradients and the rounded
    feature gradient are equal bit for bit, in both precisions"""
    from oracle import popcorn_oracle as O
    shape = E.HEAD_SHAPES[0]
    B, H, W, Hp, Wp, py, px = shape
    d = E.head_case(shape, E.HEAD_SEED, wide=variant)
    for bf16 in (False, True):
        r = E.head_reference(d, shape, bf16=bf16)
        sd = {n: t.double().clone().requires_grad_(True) for n, t in zip(E.HEAD_NAMES, d["ht"])}
        feat = (E.rbf(d["feat"]) if bf16 else d["feat"]).double().requires_grad_(True)
        with (O.bf16_mode() if bf16 else contextlib.nullcontext()):
            scale = torch.relu(O.head_forward(sd, feat[:, :, py:py + H, px:px + W])[:, 0])
            (scale * r["g_out"].view(B, H, W)).sum().backward()
        assert torch.equal(scale.detach(), r["scale_map"])
        for n, want in zip(E.HEAD_NAMES, r["grads"]):
            got = sd[n].grad
            if n.startswith("head.6"):
                got, want = got[:1], want.view(got.shape)[:1]           # (autograd gives the unused second logit its zero gradient too)
            assert torch.equal(got, want.view(got.shape)), (n, bf16)
        assert torch.equal(E.rbf(feat.grad) if bf16 else feat.grad, r["g_feat"]), bf16
