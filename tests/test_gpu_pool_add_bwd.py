"""The pool-add form of the fused fp32 backward (popcorn_hip.h: pc_conv_bwd_desc::pool_grad; csrc/conv3x3_bwd.hip).

A map that feeds both an Up block's skip connection and, through MaxPool2d(2), the Down block below has a gradient with two sources.
The old order: the skip launch writes the map's gradient, then the Down block's first layer scatters (+=) its data gradient into it
through the arg-max of every window (a read-modify-write at full resolution).  The new order: the first layer writes its RAW data
gradient at the pooled resolution, and the skip launch adds the scatter in its epilogue and writes the map's gradient once.

  * op level: both orders through ops.WgradBatch.conv3x3_bwd_group on the same crafted inputs -- the map's gradient and both layers'
    weight / bias gradients bit for bit; the new gradient against a float64 numpy restatement; what the launcher refuses;
  * step level: one native step and one per-launch-engine step, loss and all 56 gradients bit-equal, arena poisoned."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NEG_GAMMA_CH = 3            # this channel's BN scale is negative: a zero data gradient times it is -0.0
ZERO_G = (0, 0, 1)          # (b, y, x) of a pixel around which the skip launch's gradient operand is zero in every channel


def _mk(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(B, H, W, sliced):
    """a2 (the map: post-ReLU values plus crafted windows), its pooled copy, both gradient operands, both layers' weights, a2's BN"""
    a2 = F.relu(_mk(B, 8, H, W, seed=300))
    a2[0, :, 0:2, 0:2] = 0.75                        # a four-way tie: (0, 0) wins
    a2[0, :, 0:2, 2:4] = torch.tensor([[0.1, 0.5], [0.5, 0.5]])       # three-way tie away from the corner: (0, 1) wins
    a2[0, :, 2:4, 0:2] = torch.tensor([[0.2, 0.3], [0.9, 0.9]])       # tie in the second row: (1, 0) wins
    a2[0, :, 0:2, 4:6] = 0.0                         # maximum == 0: no gradient
    a2[0, :, 2:4, 4:6] = -1.0                        # maximum < 0 (not a ReLU output, but the kernel's rule covers it): no gradient
    a2[0, :, 2:4, 30:32] = torch.tensor([[0.0, 0.0], [0.0, 2.0]])     # the arg-max in the strip's last column and second row
    # the -0.0 case: pixel ZERO_G is its window's arg-max (the four-way tie's winner is (0, 0); make (0, 1) win instead in that channel)
    a2[0, NEG_GAMMA_CH, 0, 1] = 1.5
    g_up = _mk(B, 8, H, W, seed=301)
    b, y, x = ZERO_G
    g_up[b, :, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0.0        # every tap of that pixel's data gradient reads a zero
    g_dn = _mk(B, 16, H // 2, W // 2, seed=302)
    w_up = _mk(8, 16, 3, 3, seed=303, scale=0.2)
    w_dn = _mk(16, 8, 3, 3, seed=304, scale=0.2)
    gen = torch.Generator().manual_seed(305)
    gamma, beta = torch.rand(8, generator=gen) + 0.5, torch.randn(8, generator=gen) * 0.1
    mean, var = torch.randn(8, generator=gen) * 0.2, torch.rand(8, generator=gen) + 0.3
    gamma[NEG_GAMMA_CH] = -gamma[NEG_GAMMA_CH]
    t = {"g_up": g_up.cuda(), "g_dn": g_dn.cuda(), "w_up": w_up.cuda(), "w_dn": w_dn.cuda(),
         "bn": tuple(v.cuda() for v in (gamma, beta, mean, var))}
    if sliced:      # level 2's halves: x, out and pool_grad are the channel slices [:, 8:16] of 16-channel tensors
        big = torch.zeros(B, 16, H, W)
        big[:, 8:16] = a2
        t["a2"] = big.cuda()[:, 8:16]
    else:
        t["a2"] = a2.cuda()
    t["pa2"] = F.max_pool2d(a2, 2).cuda()
    cpu = {"a2": a2, "g_up": g_up, "g_dn": g_dn, "w_up": w_up, "w_dn": w_dn, "scale": gamma / torch.sqrt(var + 1e-5)}
    return t, cpu


def _nan_like(B, c, h, w, sliced):
    """a destination whose every byte is 0xFF (a NaN pattern); sliced: the second half of a 16-channel tensor"""
    full = torch.empty(B, 16 if sliced else c, h, w, device="cuda")
    full.view(torch.uint8).fill_(0xFF)
    return full[:, 8:16] if sliced else full


def _grads(cout, cin):
    return torch.full((cout, cin, 3, 3), 7.0, device="cuda"), torch.full((cout,), 7.0, device="cuda")


def _run_pair(t, B, H, W, sliced, new):
    from popcorn_amd import ops, _lib as L
    bn = L.bn(None, *t["bn"])
    G = _nan_like(B, 8, H, W, sliced)
    dw_up, db_up = _grads(8, 16)
    dw_dn, db_dn = _grads(16, 8)
    wb = ops.WgradBatch(torch.device("cuda"))
    skip = {"g": t["g_up"], "x": t["a2"], "w": t["w_up"], "out": G, "dw": dw_up, "db": db_up, "x_bn": bn}
    down = {"g": t["g_dn"], "x": t["pa2"], "w": t["w_dn"], "dw": dw_dn, "db": db_dn}
    G_p = None
    if new:
        G_p = _nan_like(B, 8, H // 2, W // 2, sliced)
        wb.conv3x3_bwd_group([dict(down, out=G_p)], 8, 0)
        wb.conv3x3_bwd_group([dict(skip, pool_grad=G_p)], 16, 0)
    else:
        wb.conv3x3_bwd_group([skip], 16, 0)
        wb.conv3x3_bwd_group([dict(down, out=G, pool_act=t["a2"], x_bn=bn)], 8, 0, accumulate=True)
    wb.finish()
    torch.cuda.synchronize()
    return {"G_a2": G, "dw_up": dw_up, "db_up": db_up, "dw_dn": dw_dn, "db_dn": db_dn, "G_pa2": G_p}


def _dgrad64(g, w):
    """float64 data gradient of a 3x3 conv (padding 1): gx[b, ci, y, x] = sum w[co, ci, dy, dx] * g[b, co, y - dy + 1, x - dx + 1]"""
    B, _, H, W = g.shape
    gp = np.pad(g, ((0, 0), (0, 0), (1, 1), (1, 1)))
    gx = np.zeros((B, w.shape[1], H, W))
    for dy in range(3):
        for dx in range(3):
            gx += np.einsum("oc,bohw->bchw", w[:, :, dy, dx], gp[:, :, 2 - dy:2 - dy + H, 2 - dx:2 - dx + W])
    return gx


def _reference64(cpu):
    """conv dgrad of the skip launch + max-pool backward (first arg-max) of the Down block's first layer, times relu'(a2) * bn scale"""
    a2 = cpu["a2"].double().numpy()
    B, C, H, W = a2.shape
    gx_up = _dgrad64(cpu["g_up"].double().numpy(), cpu["w_up"].double().numpy()[:, :8])
    gx_dn = _dgrad64(cpu["g_dn"].double().numpy(), cpu["w_dn"].double().numpy())
    win = a2.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    am = win.argmax(-1)                                                   # numpy: the first maximum, in the order 00, 01, 10, 11
    scat = np.zeros_like(win)
    np.put_along_axis(scat, am[..., None], gx_dn[..., None], axis=-1)
    scat = scat.reshape(B, C, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)
    return (gx_up + scat) * (a2 > 0) * cpu["scale"].double().numpy().reshape(1, C, 1, 1)


CASES = {"one_strip": (1, 4, 32, False), "strip_boundaries": (2, 12, 64, False), "level2_half_slice": (1, 8, 32, True)}


@pytest.fixture(scope="module", params=list(CASES))
def pairs(request):
    """both orders on one set of inputs (run once per case, shared by the tests below)"""
    B, H, W, sliced = CASES[request.param]
    t, cpu = _inputs(B, H, W, sliced)
    old = _run_pair(t, B, H, W, sliced, new=False)
    new = _run_pair(t, B, H, W, sliced, new=True)
    return old, new, cpu


def test_pool_add_pair_is_bit_identical_to_the_scatter_pair(pairs):
    old, new, cpu = pairs
    for k in ("G_a2", "dw_up", "db_up", "dw_dn", "db_dn"):
        assert torch.equal(_bits(old[k]), _bits(new[k])), (k, (old[k] - new[k]).abs().max().item())
    # both destinations were 0xFF in every byte: fully overwritten
    assert bool(torch.isfinite(new["G_a2"]).all()) and bool(torch.isfinite(new["G_pa2"]).all())
    # the crafted windows did what they were made for
    G = new["G_a2"].cpu()
    assert bool((G[0, :, 0:2, 4:6] == 0).all()) and bool((G[0, :, 2:4, 4:6] == 0).all())          # maximum <= 0: masked, nothing arrives
    # the -0.0 pixel (skip term: a zero data gradient times a negative scale) is its window's arg-max and received that window's gradient
    b, y, x = ZERO_G
    assert G[b, NEG_GAMMA_CH, y, x].item() != 0.0 and new["G_pa2"][b, NEG_GAMMA_CH, y // 2, x // 2].item() != 0.0


def test_pool_add_gradient_against_float64(pairs):
    """Tolerance: the existing split-form test's bound for the data gradient (tests/test_gpu_conv3x3.py:
    test_conv_backward_fused_split_form_has_the_error_of_fp32_arithmetic: max error <= 2e-6 of the largest reference value)."""
    _, new, cpu = pairs
    ref = _reference64(cpu)
    got = new["G_a2"].cpu().double().numpy()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"pool-add G_a2 vs float64: max error / max reference = {err:.3e}")
    assert err <= 2e-6


@pytest.mark.parametrize("bad", ["width_not_32", "height_not_4", "no_mask", "misaligned_pool_grad", "accumulate", "with_pool_act"])
def test_pool_add_launcher_refuses_without_launching(bad):
    from popcorn_amd import ops, _lib as L
    B, H, W = 1, 8, 32
    if bad == "width_not_32":
        W = 48
    if bad == "height_not_4":
        H = 6
    t, _ = _inputs(B, max(H, 4), max(W, 32), False)
    a2 = t["a2"][:, :, :H, :W].contiguous()
    g_up = t["g_up"][:, :, :H, :W].contiguous()
    bn = L.bn(None, *t["bn"])
    G = _nan_like(B, 8, H, W, False)
    G_p = torch.zeros(B * 8 * (H // 2) * (W // 2) + 2, device="cuda")
    off = 1 if bad == "misaligned_pool_grad" else 0            # 4 bytes past an 8-byte boundary
    pg = G_p[off:off + B * 8 * (H // 2) * (W // 2)].view(B, 8, H // 2, W // 2)
    dw, db = _grads(8, 16)
    pr = {"g": g_up, "x": a2, "w": t["w_up"], "out": G, "dw": dw, "db": db, "x_bn": bn, "pool_grad": pg}
    if bad == "no_mask":
        pr["x_bn"] = None
    if bad == "with_pool_act":
        pr["pool_act"] = torch.zeros(B, 8, 2 * H, 2 * W, device="cuda")
    assert ops.conv3x3_bwd_ok(g_up, a2, G)                     # the plain launch would take these tensors
    if bad in ("width_not_32", "height_not_4", "misaligned_pool_grad"):
        assert not ops.conv3x3_bwd_pool_add_ok(g_up, a2, G, pg)
    wb = ops.WgradBatch(torch.device("cuda"))
    with pytest.raises(L.PopcornHipError):
        wb.conv3x3_bwd_group([pr], 16, 0, accumulate=(bad == "accumulate"))
    torch.cuda.synchronize()
    assert bool((G.view(torch.uint8) == 0xFF).all())           # nothing ran
    assert bool((dw == 7.0).all()) and not wb.entries


def test_pool_add_predicate_accepts_what_the_launcher_takes():
    from popcorn_amd import ops
    t, _ = _inputs(1, 8, 32, False)
    G, G_p = _nan_like(1, 8, 8, 32, False), _nan_like(1, 8, 4, 16, False)
    assert ops.conv3x3_bwd_pool_add_ok(t["g_up"], t["a2"], G, G_p)


# ---- step level: the two executors take the new order from the same predicate ---------------------------------------------------------
@pytest.mark.parametrize("regime", ["all", "limit1"])
def test_step_native_and_per_launch_engine_bit_equal_on_a_poisoned_arena(regime):
    """2 x 64 x 48 (the footprint tests' shape: a 64 x 64 domain with a 32 x 32 level): loss and all 56 gradients, default regime (the
    pool-add order) and encoder_no_grad (the old order)."""
    from tests import test_gpu_native_step as tn
    from tests.test_gpu_footprint_step import _arena_needed
    from popcorn_amd import ops
    flags = tn.REGIMES[regime]
    smp = tn._batch(2, 64, 48)
    res, seen = [], []
    orig = ops.WgradBatch.conv3x3_bwd_group

    def spy(self, problems, *a, **kw):
        seen.append((sum(pr.get("pool_grad") is not None for pr in problems), sum(pr.get("pool_act") is not None for pr in problems)))
        return orig(self, problems, *a, **kw)
    for native in (True, False):
        tr = tn._fresh(native)
        if native:          # (the arena-less sizing call, then an arena of exactly that size with 0xFF in every byte)
            need = _arena_needed(tr, smp, flags)
            tr._arena = torch.empty(need, dtype=torch.uint8, device="cuda")
            tr._arena.fill_(0xFF)
        torch.manual_seed(3)
        ops.WgradBatch.conv3x3_bwd_group = spy
        try:
            loss = tn._step(tr, smp, flags)
        finally:
            ops.WgradBatch.conv3x3_bwd_group = orig
        torch.cuda.synchronize()
        assert tr.native_steps == (1 if native else 0)
        res.append((loss.clone(), {n: g.clone() for n, g in tr.grads.items()}))
    # the per-launch engine took the order the regime asks for: one pool-add launch (both streams) and no scatter launch, or neither
    pool_add, scatter = sum(a for a, _ in seen), sum(b for _, b in seen)
    assert (pool_add, scatter) == ((2, 0) if regime == "all" else (0, 0)), seen
    (l_n, g_n), (l_e, g_e) = res
    assert torch.equal(l_n, l_e), (l_n, l_e)
    assert len(g_n) == len(g_e) == 56
    for n in g_e:
        assert torch.equal(_bits(g_n[n]), _bits(g_e[n])), (n, (g_n[n] - g_e[n]).abs().max().item())


# ---- level 2: the whole-level kernel leaves its data gradient raw, the skip-halves launch of the Up block adds the scatter -------------
def test_level2_pool_grad_out_then_pool_add_halves_is_bit_identical_to_todays_contract():
    """B = 2: pc_level2_bwd_group with pool_grad_out followed by the pool-add skip-halves launch, against the skip-halves launch followed
    by pc_level2_bwd_group's scatter (+=) on the same inputs: G_b2 and the four weight / bias gradients of the level (and the halves
    launch's own) bit for bit; with the option the kernel leaves `out` alone."""
    from popcorn_amd import ops, _lib as L
    B = 2
    b2 = F.relu(_mk(B, 16, 64, 64, seed=400))
    b2[0, :, 0:2, 0:2] = 0.5                       # a tie, a window without a positive value, an arg-max in the last column
    b2[0, :, 2:4, 0:2] = 0.0
    b2[1, :, 62:64, 62:64] = torch.tensor([[0.0, 0.0], [0.0, 3.0]])
    g = torch.Generator().manual_seed(401)
    gam, bet = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.1
    mea, var = torch.randn(16, generator=g) * 0.2, torch.rand(16, generator=g) + 0.3
    gam[5] = -gam[5]
    act_p = [v.cuda() for v in (gam, bet, mea, var)]
    bn1_p = [v.cuda() for v in (torch.rand(16, generator=g) + 0.5, torch.zeros(16), torch.zeros(16), torch.rand(16, generator=g) + 0.3)]
    t = {"g2": _mk(B, 16, 32, 32, seed=402).cuda(), "c1": F.relu(_mk(B, 16, 32, 32, seed=403)).cuda(), "x": F.max_pool2d(b2, 2).cuda(),
         "b2": b2.cuda(), "w1": _mk(16, 16, 3, 3, seed=404, scale=0.1).cuda(), "w2": _mk(16, 16, 3, 3, seed=405, scale=0.1).cuda(),
         "g_e1": _mk(B, 8, 64, 64, seed=406).cuda(), "w_up": _mk(8, 32, 3, 3, seed=407, scale=0.2).cuda()}
    act_bn, bn1 = L.bn(None, *act_p, 1e-5), L.bn(None, *bn1_p, 1e-5)
    half_bn = [L.bn(None, *[v[8 * i:8 * i + 8] for v in act_p], 1e-5) for i in (0, 1)]

    def run(new):
        G = torch.empty(B, 16, 64, 64, device="cuda")
        G.view(torch.uint8).fill_(0xFF)
        G_p = torch.empty(B, 16, 32, 32, device="cuda")
        G_p.view(torch.uint8).fill_(0xFF)
        gr = {k: torch.full(s, 7.0, device="cuda") for k, s in (("dw1", (16, 16, 3, 3)), ("db1", (16,)), ("dw2", (16, 16, 3, 3)),
                                                                  ("db2", (16,)), ("dw_up", (8, 32, 3, 3)), ("db_up", (8,)))}
        wb = ops.WgradBatch(torch.device("cuda"))
        level = {"g2": t["g2"], "c1": t["c1"], "x": t["x"], "w1": t["w1"], "w2": t["w2"], "bn1": bn1, "act": t["b2"], "act_bn": act_bn,
                 "out": G, "dw1": gr["dw1"], "db1": gr["db1"], "dw2": gr["dw2"], "db2": gr["db2"]}
        halves = [{"g": t["g_e1"], "x": t["b2"][:, 8 * i:8 * i + 8], "w": t["w_up"], "out": G[:, 8 * i:8 * i + 8], "dw": gr["dw_up"],
                   "db": gr["db_up"] if i == 0 else None, "x_bn": half_bn[i], "c0_add": 8 * i} for i in (0, 1)]
        if new:
            wb.level2_bwd_group([dict(level, pool_grad_out=G_p)])
            torch.cuda.synchronize()
            assert bool((G.view(torch.uint8) == 0xFF).all())             # `out` was not touched
            assert bool(torch.isfinite(G_p).all())                       # ... and the pooled gradient fully written
            wb.conv3x3_bwd_group([dict(h, pool_grad=G_p[:, 8 * i:8 * i + 8]) for i, h in enumerate(halves)], 32, 0)
        else:
            wb.conv3x3_bwd_group(halves, 32, 0)
            wb.level2_bwd_group([level])
        wb.finish()
        torch.cuda.synchronize()
        gr["G_b2"] = G
        return gr

    old, new = run(False), run(True)
    assert bool(torch.isfinite(new["G_b2"]).all())
    for k in ("G_b2", "dw1", "db1", "dw2", "db2", "dw_up", "db_up"):
        assert torch.equal(_bits(old[k]), _bits(new[k])), (k, (old[k] - new[k]).abs().max().item())
