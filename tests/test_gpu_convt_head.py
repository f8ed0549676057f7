"""Kernel parity: ConvTranspose2d 2x2/s2 (fwd, dgrad, wgrad), building-score tail, sparsity mask, sparse head
forward and ordered compaction -- HIP vs stock PyTorch-CPU ops / the oracle.  fp32 tolerance 1e-5 rel on O(1) data;
mask / index paths bit-exact."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _mk(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("C_", [8, 16])
@pytest.mark.parametrize("shape", [(2, 32, 32), (3, 9, 21), (1, 40, 16)])
def test_convt_fwd_dgrad_wgrad(C_, shape):
    from popcorn_amd import ops
    from popcorn_amd import _lib as L
    B, H, W = shape
    x = _mk(B, C_, H, W, seed=1).requires_grad_(True)
    w = _mk(C_, C_, 2, 2, seed=2, scale=0.3).requires_grad_(True)
    bias = _mk(C_, seed=3, scale=0.1).requires_grad_(True)
    y = F.conv_transpose2d(x, w, bias, stride=2)
    g = _mk(*y.shape, seed=4)
    y.backward(g)
    out = ops.convt2x2(x.detach().cuda(), w.detach().cuda(), bias.detach().cuda())
    torch.testing.assert_close(out.cpu(), y.detach(), rtol=1e-5, atol=1e-5)
    gx = torch.empty(B, C_, H, W, device="cuda")
    ops.convt2x2_dgrad(g.cuda(), w.detach().cuda(), gx)
    torch.testing.assert_close(gx.cpu(), x.grad, rtol=1e-5, atol=1e-5)
    # fused ReLU/BN backward of the producer
    act = F.relu(_mk(B, C_, H, W, seed=5))
    gen = torch.Generator().manual_seed(6)
    gamma, var = torch.rand(C_, generator=gen) + 0.5, torch.rand(C_, generator=gen) + 0.3
    beta, mean = torch.zeros(C_), torch.zeros(C_)
    keep = [t.cuda() for t in (gamma, beta, mean, var)]
    bnd = L.bn(None, *keep)
    ops.convt2x2_dgrad(g.cuda(), w.detach().cuda(), gx, act=act.cuda(), act_bn=bnd)
    ref = x.grad * (act > 0) * (gamma / torch.sqrt(var + 1e-5)).view(1, -1, 1, 1)
    torch.testing.assert_close(gx.cpu(), ref, rtol=1e-5, atol=1e-5)
    dw, db = ops.convt2x2_wgrad(x.detach().cuda(), g.cuda())
    torch.testing.assert_close(dw.cpu(), w.grad, rtol=1e-5, atol=2e-6 * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(db.cpu(), bias.grad, rtol=1e-5, atol=2e-6 * max(1.0, bias.grad.abs().max().item()))
    dw2, db2 = ops.convt2x2_wgrad(x.detach().cuda(), g.cuda())
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _convt_wgrad_case(C_, shape, seed=1):
    """x, g and the fp64 autograd weight / bias gradient of ConvTranspose2d(C, C, 2, stride=2)"""
    B, H, W = shape
    x = _mk(B, C_, H, W, seed=seed)
    w = _mk(C_, C_, 2, 2, seed=seed + 1, scale=0.3).double().requires_grad_(True)
    bias = torch.zeros(C_, dtype=torch.double, requires_grad=True)
    y = F.conv_transpose2d(x.double(), w, bias, stride=2)
    g = _mk(*y.shape, seed=seed + 3)
    y.backward(g.double())
    return x.cuda(), g.cuda(), w.grad, bias.grad


def _assert_wgrad_close(got, ref):
    """the bar of test_convt_fwd_dgrad_wgrad against the fp64 reference"""
    torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-5, atol=2e-6 * max(ref.abs().max().item(), 1.0))


@pytest.mark.parametrize("C_,shape", [(8, (1, 16, 16)), (16, (2, 16, 32))])
@pytest.mark.parametrize("accumulate", [False, True])
def test_convt_wgrad_single_op_equals_the_batched_path(C_, shape, accumulate):
    """ops.convt2x2_wgrad == a WgradBatch of one group of one == the first problem of a group of two, bit for bit: at these sizes a
    group of two gives each problem as many partials as a lone problem gets (the test checks that it does)."""
    from popcorn_amd import ops
    dev = torch.device("cuda")
    x, g, rw, rb = _convt_wgrad_case(C_, shape)
    x2, g2, _, _ = _convt_wgrad_case(C_, shape, seed=11)
    init_w, init_b = _mk(C_, C_, 2, 2, seed=7).cuda(), _mk(C_, seed=8).cuda()

    def fresh():
        return (init_w.clone(), init_b.clone()) if accumulate else (torch.full_like(init_w, float("nan")), torch.full_like(init_b, float("nan")))

    dw, db = ops.convt2x2_wgrad(x, g, *fresh(), accumulate=accumulate)
    nwgs = []
    for others in ([], [(x2, g2)]):
        wb = ops.WgradBatch(dev, accumulate=accumulate)
        probs = [{"x": x_, "g": g_, "dw": t[0], "db": t[1]} for (x_, g_), t in zip([(x, g)] + others, [fresh(), fresh()])]
        wb.convt2x2_group(probs)
        nwgs.append(wb.entries[0].nwg)
        wb.finish()
        assert torch.equal(probs[0]["dw"], dw) and torch.equal(probs[0]["db"], db), len(probs)
    B, H, W = shape
    assert nwgs == [B * H * ((W + 15) // 16) // 4] * 2              # a workgroup per four 16-pixel row groups, single and group
    base_w, base_b = (init_w.cpu().double(), init_b.cpu().double()) if accumulate else (0.0, 0.0)
    _assert_wgrad_close(dw.cpu().double() - base_w, rw)
    _assert_wgrad_close(db.cpu().double() - base_b, rb)


@pytest.mark.parametrize("C_", [8, 16])
def test_convt_wgrad_through_the_loops_of_the_batched_reduction(C_):
    """The transposed-conv branch (kind 1) of wgrad_reduce_batch_kernel at op level against fp64 autograd with 42 partials: at least
    40 and no multiple of 32, so the bias tail runs its 4-chain loop and its remainder, the weights the 4-chain loop of rb_sum and
    its remainder (8 slices of the partial list per output).  Largest error in units of the bar (test_convt_fwd_dgrad_wgrad's),
    on an MI355X: 0.058 with the per-op reduction kernel this reduction replaced, 0.051 with this one."""
    from popcorn_amd import ops
    dev = torch.device("cuda")
    x, g, rw, rb = _convt_wgrad_case(C_, (1, 24, 112))
    wb = ops.WgradBatch(dev)
    dw, db = torch.full((C_, C_, 2, 2), float("nan"), device=dev), torch.full((C_,), float("nan"), device=dev)
    wb.convt2x2_group([{"x": x, "g": g, "dw": dw, "db": db}])       # = ops.convt2x2_wgrad
    nwg = wb.entries[0].nwg
    wb.finish()
    assert nwg == 42 and nwg >= 40 and nwg % 32 != 0
    _assert_wgrad_close(dw, rw)
    _assert_wgrad_close(db, rb)
    dw2, db2 = ops.convt2x2_wgrad(x, g)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


@pytest.mark.parametrize("C_", [8, 16])
@pytest.mark.parametrize("shape", [(2, 32, 32), (3, 16, 64), (1, 40, 16)])
@pytest.mark.parametrize("masked", [True, False])
def test_convt_backward_fused_fp32(C_, shape, masked):
    """pc_convt2x2_bwd_group (fp32): weight / bias gradient AND data gradient (+ ReLU / BN factor of x's producer) of a transposed
    conv in one launch, against autograd; the fused form is for aligned tensors with W % 16 == 0 and refuses others."""
    from popcorn_amd import ops
    from popcorn_amd import _lib as L
    B, H, W = shape
    x = F.relu(_mk(B, C_, H, W, seed=11)).requires_grad_(True)
    w = _mk(C_, C_, 2, 2, seed=12, scale=0.3).requires_grad_(True)
    bias = _mk(C_, seed=13, scale=0.1).requires_grad_(True)
    y = F.conv_transpose2d(x, w, bias, stride=2)
    g = _mk(*y.shape, seed=14)
    y.backward(g)
    gen = torch.Generator().manual_seed(16)
    gamma, var = torch.rand(C_, generator=gen) + 0.5, torch.rand(C_, generator=gen) + 0.3
    keep = [t.cuda() for t in (gamma, torch.zeros(C_), torch.zeros(C_), var)]
    gx = torch.full((B, C_, H, W), 7.0, device="cuda")
    dw, db = torch.empty(C_, C_, 2, 2, device="cuda"), torch.empty(C_, device="cuda")
    wb = ops.WgradBatch(torch.device("cuda"))
    wb.convt2x2_bwd_group([{"x": x.detach().cuda(), "g": g.cuda(), "w": w.detach().cuda(), "out": gx, "dw": dw, "db": db,
                            "x_bn": L.bn(None, *keep) if masked else None}])
    wb.finish()
    ref = x.grad * (x > 0) * (gamma / torch.sqrt(var + 1e-5)).view(1, -1, 1, 1) if masked else x.grad
    torch.testing.assert_close(gx.cpu(), ref.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dw.cpu(), w.grad, rtol=1e-5, atol=2e-6 * max(1.0, w.grad.abs().max().item()))
    torch.testing.assert_close(db.cpu(), bias.grad, rtol=1e-5, atol=2e-6 * max(1.0, bias.grad.abs().max().item()))


def test_convt_backward_fused_fp32_refuses_ragged_rows():
    from popcorn_amd import ops
    from popcorn_amd import _lib as L
    x, g = torch.zeros(1, 8, 9, 21, device="cuda"), torch.zeros(1, 8, 18, 42, device="cuda")
    wb = ops.WgradBatch(torch.device("cuda"))
    with pytest.raises(L.PopcornHipError):
        wb.convt2x2_bwd_group([{"x": x, "g": g, "w": torch.zeros(8, 8, 2, 2, device="cuda"), "out": torch.empty_like(x),
                                "dw": torch.empty(8, 8, 2, 2, device="cuda"), "db": torch.empty(8, device="cuda")}])


def test_outconv_sigmoid_crop():
    from popcorn_amd import ops
    feat = _mk(2, 16, 58, 69, seed=7)
    w = _mk(1, 16, 1, 1, seed=8, scale=0.4)
    b = _mk(1, seed=9)
    ref = torch.sigmoid(F.conv2d(feat, w, b))[:, :, 14:-14, 14:-14]
    out = ops.outconv_sigmoid_crop(feat.cuda(), w.cuda(), b.cuda(), 30, 41, 14, 14)
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["b2_100", "b1_131x77", "b2_40x52"])
def test_sparsity_mask_bit_exact_vs_golden(name):
    """Mask is an index path: bit-exact against the reference's own output (fixture g4)."""
    from popcorn_amd import ops
    g = np.load(os.path.join(G, "g4_mask.npz"))
    bc = torch.from_numpy(g[f"{name}/building_counts"])
    admin = torch.from_numpy(g[f"{name}/admin_mask"])
    census = torch.from_numpy(g[f"{name}/census_idx"])
    B, H, W = admin.shape
    rowsel = torch.zeros(H, dtype=torch.uint8)
    colsel = torch.zeros(W, dtype=torch.uint8)
    rowsel[torch.from_numpy(g[f"{name}/xindices"])] = 1
    colsel[torch.from_numpy(g[f"{name}/yindices"])] = 1
    mask, counts = ops.sparsity_mask(bc.cuda(), admin.cuda(), census.cuda(), rowsel.cuda(), colsel.cuda())
    ref = g[f"{name}/mask"]
    assert np.array_equal(mask.cpu().numpy().astype(bool), ref)
    assert counts[0].item() == int(ref.sum())
    # empty selection -> falls back to the region (popcorn.py:374-375)
    mask2, counts2 = ops.sparsity_mask(torch.zeros_like(bc).cuda(), admin.cuda(), census.cuda(),
                                       torch.zeros(H, dtype=torch.uint8).cuda(), torch.zeros(W, dtype=torch.uint8).cuda())
    region = (admin == census.view(-1, 1, 1)).numpy()
    assert np.array_equal(mask2.cpu().numpy().astype(bool), region)
    assert counts2[0].item() == int(region.sum())


def test_compact_masked_order():
    from popcorn_amd import ops
    gen = torch.Generator().manual_seed(10)
    for n in (1, 1000, 1024, 5000, 300007):
        src = torch.randn(n, generator=gen)
        mask = (torch.rand(n, generator=gen) < 0.37)
        out, cnt = ops.compact_masked(src.cuda(), mask.to(torch.uint8).cuda())
        k = cnt.item()
        assert k == int(mask.sum())
        assert torch.equal(out[:k].cpu(), src[mask])


@pytest.fixture
def head_form(request):
    """The head kernels' multiplication form (popcorn_hip.h: pc_set_head_split): 1 = exact 3-way bf16 operand splits on the bf16 matrix
    pipe (default), 0 = fp32 MFMA."""
    from popcorn_amd import _lib as L
    prev = L.lib().pc_set_head_split(int(request.param))
    yield int(request.param)
    L.lib().pc_set_head_split(prev)


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("shape", [(2, 100, 100, 128, 128, 14, 14), (1, 37, 29, 64, 64, 13, 17)])
def test_head_fwd_vs_oracle(sparse, shape, head_form):
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    B, H, W, Hp, Wp, py, px = shape
    sd = O.load_golden_state(G)
    feat = _mk(B, 16, Hp, Wp, seed=11)
    gen = torch.Generator().manual_seed(12)
    building = torch.rand(B, 1, H, W, generator=gen)
    admin = (torch.rand(B, H, W, generator=gen) < 0.6).float() * 5.0
    census = torch.full((B,), 5, dtype=torch.int64)
    mask = (torch.rand(B, H, W, generator=gen) < 0.5) & (admin == 5.0)
    headin = feat[:, :, py:py + H, px:px + W]
    with torch.no_grad():
        if sparse:
            out = O.sparse_head_forward(sd, headin, mask)[:, 0]
        else:
            out = O.head_forward(sd, headin)[:, 0]
        scale = F.relu(out)
        pd = scale * building[:, 0]
        pc = (pd * (admin == census.view(-1, 1, 1))).sum((1, 2))
    ht = [sd[f"head.{i}.{n}"].cuda() for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    s_map, pd_gpu, pc_gpu = ops.head_fwd(feat.cuda(), py, px, H, W, ht, building.cuda(),
                                         mask=mask.to(torch.uint8).cuda() if sparse else None,
                                         admin_mask=admin.cuda(), census_idx=census.cuda())
    torch.testing.assert_close(s_map.cpu(), scale, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pd_gpu.cpu(), pd, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pc_gpu.cpu(), pc, rtol=2e-5, atol=1e-4)
    # no admin mask: plain sum (popcorn.py:189-190)
    _, _, pc2 = ops.head_fwd(feat.cuda(), py, px, H, W, ht, building.cuda())
    with torch.no_grad():
        ref2 = (F.relu(O.head_forward(sd, headin)[:, 0]) * building[:, 0]).sum((1, 2))
    torch.testing.assert_close(pc2.cpu(), ref2, rtol=2e-5, atol=1e-4)


def test_head_split_products_have_the_error_of_fp32_arithmetic():
    """The split form (six bf16 x bf16 partial products of exact 3-way operand splits, fp32 accumulation) against the head evaluated in
    FLOAT64, next to the fp32-MFMA form on the same inputs: forward outputs, the feature gradient and the weight gradients of both forms
    sit at the distance of fp32 rounding from the exact values -- the split form is not a reduced-precision mode."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops, _lib as L
    B, H, W, Hp, Wp, py, px = 3, 100, 100, 128, 128, 14, 14
    sd = O.load_golden_state(G)
    names = [f"head.{i}.{n}" for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    work = {n: sd[n].double().clone().requires_grad_(True) for n in names}
    feat = _mk(B, 16, Hp, Wp, seed=31)
    fd = feat.double().requires_grad_(True)
    gen = torch.Generator().manual_seed(32)
    building = torch.rand(B, 1, H, W, generator=gen)
    g_pc = torch.randn(B, generator=gen)
    x = fd[:, :, py:py + H, px:px + W]
    h = x
    for i in (0, 2, 4, 6):
        h = F.conv2d(h, work[f"head.{i}.weight"], work[f"head.{i}.bias"])
        if i != 6:
            h = F.relu(h)
    scale = F.relu(h[:, 0])
    pc = (scale * building[:, 0].double()).sum((1, 2))
    (pc * g_pc.double()).sum().backward()
    ht = [sd[n].cuda() for n in names]
    rel = lambda a, r: ((a.double() - r).abs().max() / r.abs().max()).item()  # noqa: E731
    err = {}
    for form in (1, 0):
        prev = L.lib().pc_set_head_split(form)
        try:
            s_map, _, pc_gpu = ops.head_fwd(feat.cuda(), py, px, H, W, ht, building.cuda())
            grads, g_feat = ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), g_popcount=g_pc.cuda())
        finally:
            L.lib().pc_set_head_split(prev)
        err[form] = {"scale": rel(s_map.cpu(), scale.detach()), "popcount": rel(pc_gpu.cpu(), pc.detach()),
                     "g_feat": rel(g_feat.cpu(), fd.grad), "dW": max(rel(g.cpu()[:1] if n.startswith("head.6") else g.cpu(),
                                                                       work[n].grad[:1] if n.startswith("head.6") else work[n].grad)
                                                                   for n, g in zip(names, grads))}
    print(f"\n[head forms vs float64] split: {err[1]}   fp32 MFMA: {err[0]}")
    for form in (1, 0):
        assert err[form]["scale"] < 3e-6 and err[form]["popcount"] < 3e-6, err          # (fp32 epsilon = 6e-8; four layers of 16 / 64-term sums)
        assert err[form]["g_feat"] < 1e-5 and err[form]["dW"] < 1e-5, err              # (sums over 30,000 pixels)
    for k in err[1]:
        assert err[1][k] < 4 * err[0][k] + 1e-7, (k, err)                                # the same class, not merely inside the bar


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("shape", [(3, 100, 100, 128, 128, 14, 14), (1, 37, 29, 64, 64, 13, 17)])
def test_head_bwd_vs_oracle_autograd(sparse, shape, head_form):
    """All four upstream-gradient routes at once; reference = torch autograd through the oracle head."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    B, H, W, Hp, Wp, py, px = shape
    sd = O.load_golden_state(G)
    names = [f"head.{i}.{n}" for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    work = dict(sd)
    for n in names:
        work[n] = sd[n].clone().requires_grad_(True)
    feat = _mk(B, 16, Hp, Wp, seed=21).requires_grad_(True)
    gen = torch.Generator().manual_seed(22)
    building = torch.rand(B, 1, H, W, generator=gen)
    admin = (torch.rand(B, H, W, generator=gen) < 0.6).float() * 5.0
    census = torch.full((B,), 5, dtype=torch.int64)
    mask = (torch.rand(B, H, W, generator=gen) < 0.5) & (admin == 5.0)
    g_pc = torch.randn(B, generator=gen)
    g_pd = torch.randn(B, H, W, generator=gen) * 0.1
    g_sm = torch.randn(B, H, W, generator=gen) * 0.1
    g_const = 0.37
    headin = feat[:, :, py:py + H, px:px + W]
    if sparse:
        out = O.sparse_head_forward(work, headin, mask)[:, 0]
        selmask = mask
    else:
        out = O.head_forward(work, headin)[:, 0]
        selmask = torch.ones(B, H, W, dtype=torch.bool)
    scale = F.relu(out)
    pd = scale * building[:, 0]
    pc = (pd * (admin == census.view(-1, 1, 1))).sum((1, 2))
    loss = (pc * g_pc).sum() + (pd * g_pd).sum() + (scale * g_sm).sum() + g_const * scale[selmask].sum()
    loss.backward()
    ht = [sd[n].cuda() for n in names]
    grads, g_feat = ops.head_bwd(feat.detach().cuda(), py, px, H, W, ht, building.cuda(),
                                 mask=mask.to(torch.uint8).cuda() if sparse else None,
                                 admin_mask=admin.cuda(), census_idx=census.cuda(), g_popcount=g_pc.cuda(),
                                 g_popdense=g_pd.cuda(), g_scale_map=g_sm.cuda(),
                                 g_scale_const=torch.tensor([g_const], device="cuda"))
    for n, gr in zip(names, grads):
        ref = work[n].grad
        tol = 3e-6 * max(1.0, ref.abs().max().item())
        torch.testing.assert_close(gr.cpu(), ref, rtol=2e-5, atol=tol, msg=lambda m, n=n: f"{n}: {m}")
    torch.testing.assert_close(g_feat.cpu(), feat.grad, rtol=2e-5, atol=1e-6)
    # second output channel of head.6 gets exact zeros; run-to-run determinism
    assert torch.all(grads[6][1] == 0) and grads[7][1].item() == 0.0
    grads2, g_feat2 = ops.head_bwd(feat.detach().cuda(), py, px, H, W, ht, building.cuda(),
                                   mask=mask.to(torch.uint8).cuda() if sparse else None,
                                   admin_mask=admin.cuda(), census_idx=census.cuda(), g_popcount=g_pc.cuda(),
                                   g_popdense=g_pd.cuda(), g_scale_map=g_sm.cuda(),
                                   g_scale_const=torch.tensor([g_const], device="cuda"))
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)) and torch.equal(g_feat, g_feat2)
    # deferred reduction (PC_HEAD_BWD_DEFER_REDUCE + kind 3 of pc_wgrad_reduce_batch: the trainer's path): same sums up to the
    # association order of the partial list; = and += forms; a skipped tensor (NULL) stays untouched
    for acc in (False, True):
        tgt = [torch.full_like(t, 0.25) for t in ht]
        tgt[3] = None
        hp, g_feat3 = ops.head_bwd(feat.detach().cuda(), py, px, H, W, ht, building.cuda(),
                                   mask=mask.to(torch.uint8).cuda() if sparse else None,
                                   admin_mask=admin.cuda(), census_idx=census.cuda(), g_popcount=g_pc.cuda(),
                                   g_popdense=g_pd.cuda(), g_scale_map=g_sm.cuda(),
                                   g_scale_const=torch.tensor([g_const], device="cuda"), grads=tgt, accumulate=acc, defer_reduce=True)
        assert isinstance(hp, ops.HeadPartials) and torch.equal(g_feat3, g_feat)
        assert all(torch.all(t == 0.25) for t in tgt if t is not None)          # nothing written yet
        wb = ops.WgradBatch(torch.device("cuda"))
        wb.head_reduce(hp)
        wb.finish()
        for i, (a, b) in enumerate(zip(tgt, grads)):
            if a is None:
                continue
            want = b + 0.25 if acc else b
            if i in (6, 7) and acc:
                want = want.clone()                     # (+= leaves the structurally-zero second row alone)
                want.view(-1)[want.numel() // 2:] = 0.25
            torch.testing.assert_close(a, want, rtol=1e-5, atol=3e-6 * max(1.0, b.abs().max().item()), msg=lambda m, i=i: f"tensor {i}: {m}")
        if not acc:
            assert torch.all(tgt[6][1] == 0) and tgt[7][1].item() == 0.0


# ---- the decisions the head backward kernel takes (pc_debug_head_decisions): what tests/tie_adjudication.py forces the fp64 oracle to ----
DEC_SHAPES = [(3, 100, 100, 128, 128, 14, 14), (1, 37, 29, 64, 64, 13, 17)]       # (the second: a ragged last group of 16 pixels)


def _dec_inputs(shape, sparse, seed):
    B, H, W, Hp, Wp, py, px = shape
    feat = _mk(B, 16, Hp, Wp, seed=seed)
    gen = torch.Generator().manual_seed(seed + 1)
    building = torch.rand(B, 1, H, W, generator=gen)
    mask = (torch.rand(B, H, W, generator=gen) < 0.5) if sparse else torch.ones(B, H, W, dtype=torch.bool)
    return feat, building, mask


def _unit_pattern(seed):
    """64 values of +1 / -1 / 0 with no symmetry under permutations of the kernel's unit indices (16 m + 4 k + r): a fixed random draw."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (64,), generator=gen).float()


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("shape", DEC_SHAPES)
def test_head_decision_export_known_answer(sparse, shape, head_form):
    """Bit mapping of the exported records: with all head weights zero every pre-activation IS its bias, so every selected pixel must
    export exactly the sign pattern of the biases -- a different irregular pattern of +1 / -1 / 0 per layer, b6 = +1, -1, 0 in turn; a
    bias of exactly 0 exports 0 (the decision is the strict > 0).  Records of unselected pixels stay untouched."""
    from popcorn_amd import ops
    B, H, W, Hp, Wp, py, px = shape
    feat, building, mask = _dec_inputs(shape, sparse, 61)
    pats = [_unit_pattern(70 + i) for i in range(3)]
    assert all(int((p == v).sum()) > 8 for p in pats for v in (-1.0, 0.0, 1.0)) and not any(torch.equal(pats[i], pats[j]) for i in range(3) for j in range(i))
    for b6 in (1.0, -1.0, 0.0):
        ht = [torch.zeros(64, 16, 1, 1), pats[0], torch.zeros(64, 64, 1, 1), pats[1], torch.zeros(64, 64, 1, 1), pats[2],
              torch.zeros(2, 64, 1, 1), torch.tensor([b6, 0.5])]
        ht = [t.cuda() for t in ht]
        buf = ops.head_decision_buffer(B, H, W, "cuda")
        ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), mask=mask.to(torch.uint8).cuda() if sparse else None,
                     g_scale_const=torch.ones(1, device="cuda"), decisions=buf)
        hidden, outd = ops.decode_head_decisions(buf, mask)
        nsel = int(mask.sum())
        assert hidden.shape == (3, 64, nsel) and outd.shape == (nsel,)
        for layer in range(3):
            want = (pats[layer] > 0).view(64, 1).expand(64, nsel)
            assert torch.equal(hidden[layer], want), (layer, b6, int((hidden[layer] != want).sum()))
        assert torch.equal(outd, torch.full((nsel,), b6 > 0)), b6
        assert torch.all(buf.cpu()[~mask.reshape(-1)] == 0)


def _feat_bn(seed):
    from popcorn_amd import _lib as L
    gen = torch.Generator().manual_seed(seed)
    mk = lambda lo, hi: (lo + (hi - lo) * torch.rand(8, generator=gen)).cuda()  # noqa: E731
    return tuple(L.bn(gamma=mk(0.5, 1.5), beta=mk(-0.2, 0.2), mean=mk(-0.2, 0.2), var=mk(0.5, 1.5)) for _ in range(2))


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("shape", DEC_SHAPES)
def test_head_decision_export_does_not_perturb_the_call(sparse, shape, head_form):
    """The exporting instantiation computes what the product kernel computes: g_feat and the 8 weight gradients are torch.equal between
    the two launches on the same inputs, with and without the fused feature-BN epilogue; with g_popcount all zero (every group leaves
    through the kernel's early exit) the gradients are equal too AND the exported records are complete: the same as with gradient."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    B, H, W, Hp, Wp, py, px = shape
    sd = O.load_golden_state(G)
    feat, building, mask = _dec_inputs(shape, sparse, 81)
    gen = torch.Generator().manual_seed(83)
    admin = (torch.rand(B, H, W, generator=gen) < 0.6).float() * 5.0
    census = torch.full((B,), 5, dtype=torch.int64)
    g_pc = torch.randn(B, generator=gen)
    ht = [sd[f"head.{i}.{n}"].cuda() for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    records = []
    for bn in (None, _feat_bn(85)):
        for gp in (g_pc, torch.zeros(B)):
            kw = dict(mask=mask.to(torch.uint8).cuda() if sparse else None, admin_mask=admin.cuda(), census_idx=census.cuda(),
                      g_popcount=gp.cuda(), feat_bn=bn)
            grads0, gf0 = ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), **kw)
            buf = ops.head_decision_buffer(B, H, W, "cuda")
            grads1, gf1 = ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), decisions=buf, **kw)
            assert torch.equal(gf0, gf1) and all(torch.equal(a, b) for a, b in zip(grads0, grads1)), (bn is not None, float(gp.abs().sum()))
            if float(gp.abs().sum()) == 0.0:
                assert not bool(gf0.any()) and not any(bool(g.any()) for g in grads0)
            else:
                assert bool(gf0.any())
            records.append(buf.cpu())
            # (the export is over: the next product launch is the product kernel again)
            grads2, gf2 = ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), **kw)
            assert torch.equal(gf0, gf2) and all(torch.equal(a, b) for a, b in zip(grads0, grads2))
    assert all(torch.equal(records[0], r) for r in records[1:])
    assert bool((records[0][mask.reshape(-1)] < 0).all())           # every selected record written (bit 63)
    assert torch.all(records[0][~mask.reshape(-1)] == 0)


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("shape", DEC_SHAPES)
def test_head_decision_export_vs_float64(sparse, shape, head_form):
    """The exported masks against a FLOAT64 head on the same random features (golden weights; head.6.bias[0] moved by the median of the
    float64 output so that the output decision takes both signs): they may differ only at near-ties -- at most max(8, 2e-5 x sites)
    sites, each with |float64 pre-activation| <= 1e-4 of its layer's mean magnitude (the bounds tests/tie_adjudication.py puts on the
    sites it overrides).  Room under the cap: with generator seed 41 the float32 TORCH head on the CPU differs from the float64 one at
    0 of 5,790,000 sites (3 x 100 x 100 dense) and 0 of 207,089 (1 x 37 x 29 dense) -- counted without a GPU; the sparse cases are
    subsets of those pixels."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    B, H, W, Hp, Wp, py, px = shape
    sd = O.load_golden_state(G)
    feat, building, mask = _dec_inputs(shape, sparse, 41)
    x = feat[:, :, py:py + H, px:px + W].double().permute(1, 0, 2, 3).reshape(16, -1, 1)

    def pre64(b6):
        h, pres = x, []
        for i in (0, 2, 4):
            h = F.conv2d(h, sd[f"head.{i}.weight"].double(), sd[f"head.{i}.bias"].double())
            pres.append(h[:, :, 0])
            h = F.relu(h)
        pres.append(F.conv2d(h, sd["head.6.weight"].double(), b6.double())[0:1, :, 0])
        return pres

    b6 = sd["head.6.bias"].clone()
    b6[0] -= pre64(b6)[3].median().float()
    pres = [p[:, mask.reshape(-1)] for p in pre64(b6)]
    assert 0.3 < float((pres[3] > 0).double().mean()) < 0.7
    ht = [sd[f"head.{i}.{n}"] for i in (0, 2, 4) for n in ("weight", "bias")] + [sd["head.6.weight"], b6]
    buf = ops.head_decision_buffer(B, H, W, "cuda")
    ops.head_bwd(feat.cuda(), py, px, H, W, [t.cuda() for t in ht], building.cuda(), mask=mask.to(torch.uint8).cuda() if sparse else None,
                 g_scale_const=torch.ones(1, device="cuda"), decisions=buf)
    hidden, outd = ops.decode_head_decisions(buf, mask)
    got = [hidden[0], hidden[1], hidden[2], outd.view(1, -1)]
    sites = sum(p.numel() for p in pres)
    ndiff, margin = 0, 0.0
    for g, p in zip(got, pres):
        d = g != (p > 0)
        ndiff += int(d.sum())
        if bool(d.any()):
            margin = max(margin, float(p.abs()[d].max() / p.abs().mean()))
    print(f"\n[head decisions vs float64] form {head_form}, sparse {sparse}, {shape[:3]}: {ndiff} of {sites} sites differ, worst margin {margin:.1e}")
    assert ndiff <= max(8, 2e-5 * sites), (ndiff, sites)
    assert margin <= 1e-4, margin


@pytest.mark.parametrize("head_form", [1, 0], indirect=True)
def test_head_decision_export_refusals_leave_the_buffer_untouched(head_form):
    """PC_EINVAL, with nothing written: a buffer smaller than B x H x W records, and bf16 mode (its kernel has no export).  The
    registration ends with the call either way: the next plain call runs."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops, _lib as L
    B, H, W, Hp, Wp, py, px = DEC_SHAPES[1]
    sd = O.load_golden_state(G)
    feat, building, mask = _dec_inputs(DEC_SHAPES[1], True, 91)
    ht = [sd[f"head.{i}.{n}"].cuda() for i in (0, 2, 4, 6) for n in ("weight", "bias")]
    kw = dict(mask=mask.to(torch.uint8).cuda(), g_scale_const=torch.ones(1, device="cuda"))
    small = torch.full((B * H * W * 4 - 1,), 7, device="cuda", dtype=torch.int64)
    with pytest.raises(L.PopcornHipError):
        ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), decisions=small, **kw)
    torch.cuda.synchronize()
    assert torch.all(small == 7)
    full = torch.full((B * H * W, 4), 7, device="cuda", dtype=torch.int64)
    with L.precision("bf16"):
        with pytest.raises(L.PopcornHipError):
            ops.head_bwd(L.as_act(feat.cuda()), py, px, H, W, ht, building.cuda(), decisions=full, **kw)
    torch.cuda.synchronize()
    assert torch.all(full == 7)
    # a sufficient buffer in fp32 mode: selected records written, the others still as they were
    ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), decisions=full, **kw)
    fc = full.cpu()
    assert bool((fc[mask.reshape(-1)] < 0).all()) and torch.all(fc[~mask.reshape(-1)] == 7)
    grads, _ = ops.head_bwd(feat.cuda(), py, px, H, W, ht, building.cuda(), **kw)
    assert all(bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.parametrize("case", ["regions", "empty_selection", "no_occupancy"])
@pytest.mark.parametrize("C_", [16, 2])
def test_building_score_mask_equals_the_two_separate_ops(case, C_):
    """pc_building_score_mask (one launch) == pc_outconv_sigmoid_crop + pc_sparsity_mask, bit for bit: building score, mask
    and {nsel, nregion}; incl. the batch-wide empty selection (popcorn.py:374-375 fallback) and repeated calls (the
    library-owned accumulator is re-zeroed per call)."""
    from popcorn_amd import ops
    B, H, W, pad = 3, 37, 52, 14
    g = torch.Generator().manual_seed(5)
    feat = torch.randn(B, C_, H + 2 * pad, W + 2 * pad, generator=g).cuda()
    w = torch.randn(C_, generator=g).cuda()
    bias = torch.randn(1, generator=g).cuda()
    admin = torch.randint(1, 4, (B, H, W), generator=g).float().cuda()
    census = torch.tensor([1, 2, 3], dtype=torch.int64).cuda()
    if case == "empty_selection":
        census = torch.tensor([7, 8, 9], dtype=torch.int64).cuda()          # no pixel belongs to the regions asked for
    rowsel = (torch.rand(H, generator=g) < 0.5).to(torch.uint8).cuda()
    colsel = (torch.rand(W, generator=g) < 0.5).to(torch.uint8).cuda()
    occ = case != "no_occupancy"
    rb = ops.outconv_sigmoid_crop(feat, w, bias, H, W, pad, pad)
    rm, rc = ops.sparsity_mask(rb, admin, census, rowsel, colsel, occ)
    for _ in range(3):
        b2, m2, c2 = ops.building_score_mask(feat, w, bias, H, W, pad, pad, admin, census, rowsel, colsel, occ)
        assert torch.equal(b2, rb) and torch.equal(m2, rm) and c2.tolist() == rc.tolist()
    if case == "empty_selection":
        assert rc.tolist() == [0, 0] and int(rm.sum()) == 0
    else:
        assert rc[0].item() == int(rm.sum()) > 0


@pytest.mark.parametrize("losses,lams", [(("l1_loss",), (1.0,)), (("log_l1_loss",), (1.0,)), (("mse_loss",), (1.0,)),
                                         (("log_mse_loss",), (1.0,)), (("l1_loss", "log_mse_loss", "mse_loss"), (0.5, 2.0, 0.01))])
def test_loss_fwd_bwd_kernel_all_losses_vs_oracle(losses, lams):
    """pc_loss_fwd_bwd for every loss the reference offers (utils/losses.py:49-56) and a weighted mix, against the oracle's
    get_loss + autograd: loss value, regulariser, d(lam_weak * loss)/d popcount and the constant regulariser gradient
    (utils/losses.py:74-76), incl. a rank-style global batch (inv_B of twice the local batch)."""
    from oracle import popcorn_oracle as O
    from popcorn_amd import ops
    from popcorn_amd.train import LOSS_INDEX
    g = np.load(os.path.join(G, "g6_loss_metrics.npz"))
    pred, y, scale = (torch.from_numpy(g[k]) for k in ("pred", "y", "scale"))
    lam_weak, sreg = 100.0, 0.01
    p = pred.clone().requires_grad_(True)
    sc = scale.clone().requires_grad_(True)
    ref, _ = O.get_loss({"popcount": p}, {"y": y}, scale=sc, loss=list(losses), lam=list(lams), scale_regularization=sreg, tag="weak")
    (ref * lam_weak).backward()
    lam4 = [0.0] * 4
    for lo, la in zip(losses, lams):
        lam4[LOSS_INDEX[lo]] += la
    B = pred.numel()
    for world in (1, 2):
        stats = torch.tensor([float(scale.numel()), float(scale.double().sum())], dtype=torch.float64, device="cuda")
        loss_out = torch.zeros(2, device="cuda")
        g_pc = torch.zeros(B, device="cuda")
        g_sc = torch.zeros(1, device="cuda")
        ops.loss_fwd_bwd(pred.cuda(), y.cuda(), stats, lam4, sreg, lam_weak, 1.0 / (world * B), loss_out, g_pc, g_sc)
        torch.cuda.synchronize()
        reg = sreg * scale.abs().mean().item()
        assert abs(loss_out[1].item() - reg) <= 1e-6 * max(1.0, reg)
        assert abs((loss_out[0].item() - reg) * world + reg - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
        torch.testing.assert_close(g_pc.cpu() * world, p.grad, rtol=2e-6, atol=1e-7)
        assert abs(g_sc.item() - sc.grad[0].item()) <= 1e-6 * abs(sc.grad[0].item())
