"""Op-level Python wrappers over the C ABI (one call = one kernel launch on the current stream).

Used by the kernel parity tests and by the nn.Module glue; the training hot path goes through the fused
composite entry points instead (popcorn_amd/engine.py).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def conv3x3_raw(a, w, bnd, relu=True, b=None, a_mode=L.PC_SRC_DIRECT, a_pad=(0, 0), chmap=(0, 1, 2, 3), out=None,
                out_hw=None, b_offset=(0, 0), a_channels=None):
    """Conv2d(3x3, pad 1)(cat[a, b]) -> BN(eval) -> ReLU with a prebuilt pc_bn descriptor.  networks.py:259-266,318.

    a_mode POOL2: a is at twice the resolution (MaxPool2d(2) fused).  a_mode REFLECT: a is reflect-padded by
    a_pad=(top,left) up to out_hw and its channels gathered through chmap."""
    L.require_device(a, w)
    B = a.shape[0]
    Ca = a.shape[1] if a_channels is None else a_channels
    Cb = 0 if b is None else b.shape[1]
    Cout = w.shape[0]
    if a_mode == L.PC_SRC_POOL2:
        H, W = a.shape[2] // 2, a.shape[3] // 2
    elif a_mode == L.PC_SRC_REFLECT:
        H, W = out_hw
    else:
        H, W = a.shape[2], a.shape[3]
    sa = L.src(a, C_=Ca, mode=a_mode, oy=a_pad[0], ox=a_pad[1], chmap=chmap)
    sb = L.src(b, oy=b_offset[0], ox=b_offset[1]) if b is not None else None
    if out is None:
        out = L.empty_act(B, Cout, H, W, a.device)
    d = L.dst(out)
    code = L.lib().pc_conv3x3_bn_relu_fwd(C.byref(sa), C.byref(sb) if sb is not None else None, L.ptr(w), C.byref(bnd),
                                          int(relu), C.byref(d), B, H, W, Ca + Cb, Cout, L.stream_ptr())
    L.check(code, "pc_conv3x3_bn_relu_fwd")
    return out


def conv3x3_fwd_group(problems, relu=True, a_mode=L.PC_SRC_DIRECT, a_pad=(0, 0), out_hw=None, a_channels=None,
                      b_offset=(0, 0)):
    """Grouped form of conv3x3_raw: ``problems`` = list (<= 4) of dicts {a, w, bn, out, b (optional), chmap (optional),
    pool_out (optional: MaxPool2d(2) of out, see pool_out_like), dot_w + dot_out (optional, 8 -> 8 layers: write
    sum_co dot_w[co] * out[co] as a one-channel map instead of out)}
    with identical geometry; one launch (blockIdx.y = problem)."""
    n = len(problems)
    assert 1 <= n <= L.PC_MAX_GROUP
    a0, w0 = problems[0]["a"], problems[0]["w"]
    L.require_device(a0, w0)
    B = a0.shape[0]
    Ca = a0.shape[1] if a_channels is None else a_channels
    Cb = 0 if problems[0].get("b") is None else problems[0]["b"].shape[1]
    Cout = w0.shape[0]
    if a_mode == L.PC_SRC_POOL2:
        H, W = a0.shape[2] // 2, a0.shape[3] // 2
    elif a_mode == L.PC_SRC_REFLECT:
        H, W = out_hw
    else:
        H, W = a0.shape[2], a0.shape[3]
    keep = []
    descs = (L.PcConvFwdDesc * n)()
    for i, pr in enumerate(problems):
        sa = L.src(pr["a"], C_=Ca, mode=a_mode, oy=a_pad[0], ox=a_pad[1], chmap=pr.get("chmap", (0, 1, 2, 3)))
        sb = L.src(pr["b"], oy=b_offset[0], ox=b_offset[1]) if pr.get("b") is not None else None
        d = L.dst(pr["out"]) if pr.get("out") is not None else None
        keep += [sa, sb, d]
        descs[i].a = C.pointer(sa)
        descs[i].b = C.pointer(sb) if sb is not None else None
        descs[i].w = pr["w"].data_ptr()
        descs[i].bn = C.pointer(pr["bn"])
        descs[i].out = C.pointer(d) if d is not None else None
        if pr.get("dot_w") is not None:          # 1x1-conv partial sum over the 8 output channels instead of the map
            dd = L.dst(pr["dot_out"])
            keep += [dd, pr["dot_w"]]
            descs[i].dot_w = pr["dot_w"].data_ptr()
            descs[i].dot_out = C.pointer(dd)
        if pr.get("pool_out") is not None:
            dp = L.dst(pr["pool_out"])
            keep.append(dp)
            descs[i].pool_out = C.pointer(dp)
        if pr.get("upt_out") is not None:        # bf16 mode, 8 -> 8: the transposed conv that follows, in this launch's epilogue
            du = L.dst(pr["upt_out"])
            keep.append(du)
            descs[i].upt_w, descs[i].upt_out = pr["upt_w"].data_ptr(), C.pointer(du)
            descs[i].upt_b = pr["upt_b"].data_ptr() if pr.get("upt_b") is not None else None
        if pr.get("w_window") is not None:       # bf16 mode: w covers input channels [ci0, ci0 + cin) of the shared 8-channel input
            descs[i].w_ci0, descs[i].w_cin = int(pr["w_window"][0]), int(pr["w_window"][1])
            assert pr["w"].shape[1] == descs[i].w_cin and Ca + Cb == 8
    L.check(L.lib().pc_conv3x3_bn_relu_fwd_group(n, descs, int(relu), B, H, W, Ca + Cb, Cout, L.stream_ptr()),
            "pc_conv3x3_bn_relu_fwd_group")


def pool_out_like(out):
    """Buffer for the 2x2-max-pooled second output of conv3x3_fwd_group (problem key "pool_out"), or None when the
    geometry of ``out`` (B, C, H, W) does not qualify (pc_conv3x3_pool_out_ok)."""
    B, Cc, H, W = out.shape
    d = L.dst(out)
    if not L.lib().pc_conv3x3_pool_out_ok(C.byref(d), H, W):
        return None
    return L.empty_act(B, Cc, H // 2, W // 2, out.device)


def conv3x3_dgrad_group(problems, c0, cn, pool=False, accumulate=False):
    """Grouped conv3x3_dgrad: problems = list of dicts {g, w, out, act (optional), act_bn (optional), c0_add (optional: this
    problem's input-channel block starts at c0 + c0_add -- both column blocks of a concat layer in one launch)}."""
    n = len(problems)
    assert 1 <= n <= L.PC_MAX_GROUP
    g0, w0 = problems[0]["g"], problems[0]["w"]
    L.require_device(g0, w0)
    B, Cg, H, W = g0.shape
    keep = []
    descs = (L.PcConvDgradDesc * n)()
    for i, pr in enumerate(problems):
        sg, d = L.src(pr["g"]), L.dst(pr["out"])
        sa = L.src(pr["act"]) if pr.get("act") is not None else None
        keep += [sg, d, sa]
        descs[i].g = C.pointer(sg)
        ca = int(pr.get("c0_add", 0))
        assert 0 <= c0 + ca and c0 + ca + cn <= pr["w"].shape[1]
        descs[i].w = pr["w"].data_ptr() + 4 * 9 * ca
        descs[i].act = C.pointer(sa) if sa is not None else None
        descs[i].act_bn = C.pointer(pr["act_bn"]) if pr.get("act_bn") is not None else None
        descs[i].out = C.pointer(d)
    L.check(L.lib().pc_conv3x3_dgrad_group(n, descs, w0.shape[1], c0, cn, int(pool), int(accumulate), B, H, W, Cg,
                                           L.stream_ptr()), "pc_conv3x3_dgrad_group")


def conv3x3_bwd_ok(g, x, out, pool_act=None):
    """fp32 mode: does the one-launch backward of a conv layer (WgradBatch.conv3x3_bwd_group) take this gradient / 8-channel input
    block / output (and, for a Down block's first layer, the full-resolution activation the input was pooled from)?"""
    if g.dtype != torch.float32:
        return False
    B, _, H, W = g.shape
    sg, sx, d = L.src(g), L.src(x), L.dst(out)
    spa = L.src(pool_act) if pool_act is not None else None
    return bool(L.lib().pc_conv3x3_bwd_ok(C.byref(sg), C.byref(sx), C.byref(d), C.byref(spa) if spa is not None else None, B, H, W))


def conv3x3_bwd_pool_add_ok(g, x, out, pool_grad):
    """fp32 mode: does the one-launch backward take this problem with ``pool_grad`` (the pool-add form: whole strips, the split-operand
    kernel, the pooled gradient planar with 8-byte rows)?"""
    if g.dtype != torch.float32 or pool_grad is None:
        return False
    B, _, H, W = g.shape
    sg, sx, d, spg = L.src(g), L.src(x), L.dst(out), L.src(pool_grad)
    return bool(L.lib().pc_conv3x3_bwd_pool_add_ok(C.byref(sg), C.byref(sx), C.byref(d), C.byref(spg), B, H, W))


def conv3x3_bn_relu(a, w, bias, gamma=None, beta=None, mean=None, var=None, eps=1e-5, relu=True, **kw):
    return conv3x3_raw(a, w, L.bn(bias, gamma, beta, mean, var, eps), relu=relu, **kw)


def conv3x3_dgrad(g, w, c0, cn, out, act=None, act_bn=None, pool=False, accumulate=False):
    """Data gradient of the conv above for forward input channels [c0, c0+cn) -> out (see popcorn_hip.h)."""
    L.require_device(g, w, out)
    B, Cg, H, W = g.shape
    sg = L.src(g)
    d = L.dst(out)
    sa = L.src(act) if act is not None else None
    code = L.lib().pc_conv3x3_dgrad(C.byref(sg), L.ptr(w), w.shape[1], c0, cn,
                                    C.byref(sa) if sa is not None else None,
                                    C.byref(act_bn) if act_bn is not None else None,
                                    int(pool), int(accumulate), C.byref(d), B, H, W, Cg, L.stream_ptr())
    L.check(code, "pc_conv3x3_dgrad")
    return out


_ws_cache = {}
_ws_retired = []       # outgrown workspaces stay allocated: a captured HIP graph may hold their device pointers


def _workspace(nbytes: int, device, tag="ws") -> torch.Tensor:
    key = (str(device), tag)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        if t is not None:
            _ws_retired.append(t)
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = t
    return t


def conv3x3_wgrad(a, g, cout, dw=None, db=None, b=None, accumulate=False, a_mode=L.PC_SRC_DIRECT, a_pad=(0, 0),
                  chmap=(0, 1, 2, 3), b_offset=(0, 0), a_channels=None):
    """Weight/bias gradient of conv3x3 over x = cat[a, b] with output gradient g (already ReLU/BN-masked): a WgradBatch of one."""
    L.require_device(a, g)
    cin = (a.shape[1] if a_channels is None else a_channels) + (0 if b is None else b.shape[1])
    if dw is None:
        dw = torch.empty(cout, cin, 3, 3, device=g.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(cout, device=g.device, dtype=torch.float32)
    wb = WgradBatch(g.device, accumulate=accumulate)
    wb.conv3x3(a, g, cout, dw, db, b=b, a_mode=a_mode, a_pad=a_pad, chmap=chmap, b_offset=b_offset, a_channels=a_channels)
    wb.finish()
    return dw, db


def convt2x2(x, w, bias, out=None):
    """ConvTranspose2d(C, C, 2, stride=2).  networks.py:302,306."""
    L.require_device(x, w)
    B, Cc, H, W = x.shape
    if out is None:
        out = L.empty_act(B, Cc, 2 * H, 2 * W, x.device)
    sx, d = L.src(x), L.dst(out)
    L.check(L.lib().pc_convt2x2_fwd(C.byref(sx), L.ptr(w), L.ptr(bias), C.byref(d), B, H, W, Cc, L.stream_ptr()),
            "pc_convt2x2_fwd")
    return out


def convt2x2_group(problems):
    """Grouped ConvTranspose2d: problems = list of {x, w, bias, out}; one launch."""
    n = len(problems)
    x0 = problems[0]["x"]
    B, Cc, H, W = x0.shape
    keep, descs = [], (L.PcConvtFwdDesc * n)()
    for i, pr in enumerate(problems):
        sx, d = L.src(pr["x"]), L.dst(pr["out"])
        keep += [sx, d]
        descs[i].x, descs[i].w, descs[i].bias, descs[i].out = C.pointer(sx), pr["w"].data_ptr(), pr["bias"].data_ptr(), C.pointer(d)
    L.check(L.lib().pc_convt2x2_fwd_group(n, descs, B, H, W, Cc, L.stream_ptr()), "pc_convt2x2_fwd_group")


def level2_fwd_ok(x, u2):
    """Does the one-launch 32 x 32 level (pc_level2_fwd_group) take these tensors?  x: (B,16,32,32) pooled map, u2: (B,16,64,64)."""
    adt = L.act_dtype()                    # fp32 mode: planar fp32; bf16 mode: channels-last bf16 (level2_cl.hip)
    planar = adt == torch.float32
    if x is None or x.dim() != 4 or tuple(x.shape[1:]) != (16, 32, 32) or x.dtype != adt or x.stride(3 if planar else 1) != 1:
        return False
    if u2 is not None and (tuple(u2.shape[1:]) != (16, 64, 64) or u2.dtype != adt or u2.stride(3 if planar else 1) != 1):
        return False
    sx = L.src(x)
    du = L.dst(u2) if u2 is not None else None
    return bool(L.lib().pc_level2_fwd_ok(C.byref(sx), C.byref(du) if du is not None else None))


def conv3x3_up_fwd_ok(skip, z, out):
    """Does pc_conv3x3_up_fwd_group (first conv of an Up block computed from the LOW-resolution map, no up-sampled tensor) take
    these tensors?  skip (B,Cs,H,W), z (B,C,H/2,W/2), out (B,8,H,W)."""
    if skip is None or z is None or skip.dtype != torch.float32 or z.dtype != torch.float32 or out.dtype != torch.float32:
        return False
    if skip.stride(3) != 1 or z.stride(3) != 1 or out.stride(3) != 1:
        return False
    B, Cs, H, W = skip.shape
    ss, sz, do = L.src(skip), L.src(z), L.dst(out)
    return bool(L.lib().pc_conv3x3_up_fwd_ok(C.byref(ss), C.byref(sz), C.byref(do), H, W, Cs, z.shape[1]))


def conv3x3_up_compose(problems):
    """Composed operand images for a list (<= 8) of Up-block convolutions {w, wt, bt} (any mix of the 8 + 8 and 16 + 16 channel
    shapes) in ONE launch.  Returns one workspace tensor per problem (pass it as ``ws`` to conv3x3_up_fwd_group)."""
    n = len(problems)
    assert 1 <= n <= 2 * L.PC_MAX_GROUP
    dev = problems[0]["w"].device
    descs = (L.PcConvUpFwdDesc * n)()
    cs, cz, slots = (C.c_int * n)(), (C.c_int * n)(), []
    for i, pr in enumerate(problems):
        Cz = pr["wt"].shape[0]
        cs[i], cz[i] = pr["w"].shape[1] - Cz, Cz
        slots.append(torch.empty(int(L.lib().pc_conv3x3_up_ws_bytes(Cz)), dtype=torch.uint8, device=dev))
        descs[i].w, descs[i].wt = pr["w"].data_ptr(), pr["wt"].data_ptr()
        descs[i].bt = pr["bt"].data_ptr() if pr.get("bt") is not None else None
        descs[i].ws = slots[i].data_ptr()
    L.check(L.lib().pc_conv3x3_up_compose_group(n, descs, cs, cz, L.stream_ptr()), "pc_conv3x3_up_compose_group")
    return slots


def conv3x3_up_fwd_group(problems, relu=True):
    """conv3x3(cat[skip, ConvTranspose2d(z)]) + BN + ReLU without materialising the up-sampled map (networks.py:302-318):
    problems = list (<= 4) of dicts {skip, z, w ([8][Cs + C][3][3]), wt ([C][C][2][2]), bt ([C]), bn, out, ws (optional: the
    workspace conv3x3_up_compose filled for this problem)}.  Returns the workspaces (the backward pass reads them again)."""
    n = len(problems)
    assert 1 <= n <= L.PC_MAX_GROUP
    skip0, z0 = problems[0]["skip"], problems[0]["z"]
    L.require_device(skip0, z0)
    B, Cs, H, W = skip0.shape
    Cz = z0.shape[1]
    nbytes = int(L.lib().pc_conv3x3_up_ws_bytes(Cz))
    pre = all(pr.get("ws") is not None for pr in problems)
    keep, slots = [], []
    descs = (L.PcConvUpFwdDesc * n)()
    for i, pr in enumerate(problems):
        # composed operand images of this call (forward stages, bias table, the backward's data-gradient image): a fresh tensor
        # per problem -- the backward pass of a saved network reads it again (under graph capture it lives in the graph's pool)
        slots.append(pr["ws"] if pre else torch.empty(nbytes, dtype=torch.uint8, device=skip0.device))
        ss, sz, do = L.src(pr["skip"]), L.src(pr["z"]), L.dst(pr["out"])
        keep += [ss, sz, do]
        descs[i].skip, descs[i].z, descs[i].out = C.pointer(ss), C.pointer(sz), C.pointer(do)
        descs[i].w, descs[i].wt = pr["w"].data_ptr(), pr["wt"].data_ptr()
        descs[i].bt = pr["bt"].data_ptr() if pr.get("bt") is not None else None
        descs[i].bn = C.pointer(pr["bn"])
        descs[i].ws = slots[i].data_ptr()
    L.check(L.lib().pc_conv3x3_up_fwd_group(n, descs, int(relu) | (2 if pre else 0), B, H, W, Cs, Cz, L.stream_ptr()),
            "pc_conv3x3_up_fwd_group")
    return slots


_up_bwd_ws = {}


def conv3x3_up_bwd_ok(g, z, gz):
    if g is None or z is None or g.dtype != torch.float32 or z.dtype != torch.float32 or g.stride(3) != 1 or z.stride(3) != 1:
        return False
    if gz is not None and (gz.dtype != torch.float32 or gz.stride(3) != 1):
        return False
    B, Cg, H, W = g.shape
    sg, sz = L.src(g), L.src(z)
    dz = L.dst(gz) if gz is not None else None
    return bool(L.lib().pc_conv3x3_up_bwd_ok(C.byref(sg), C.byref(sz), C.byref(dz) if dz is not None else None, H, W, z.shape[1], z.shape[1]))


def conv3x3_up_bwd_group(problems, accumulate=False):
    """Backward of the up-sampled half of an Up block's first conv from the low-resolution map (pc_conv3x3_up_bwd_group):
    problems = list of {g (B,8,H,W), z (B,C,H/2,W/2), z_bn, gz (out, optional), w, wt, bt, fwd_ws (slot returned by
    conv3x3_up_fwd_group), dw (full conv weight gradient [8][Cs + C][3][3]), dwt, dbt}."""
    n = len(problems)
    g0, z0 = problems[0]["g"], problems[0]["z"]
    L.require_device(g0, z0)
    B, Cg, H, W = g0.shape
    Cz = z0.shape[1]
    nbytes = int(L.lib().pc_conv3x3_up_bwd_ws_bytes(B, H, Cz))
    key = (str(g0.device), Cz, nbytes)
    slots = _up_bwd_ws.setdefault(key, [])
    keep = []
    descs = (L.PcConvUpBwdDesc * n)()
    for i, pr in enumerate(problems):
        if len(slots) <= i:
            slots.append(torch.empty(nbytes, dtype=torch.uint8, device=g0.device))
        sg, sz = L.src(pr["g"]), L.src(pr["z"])
        dz = L.dst(pr["gz"]) if pr.get("gz") is not None else None
        keep += [sg, sz, dz]
        descs[i].g, descs[i].z = C.pointer(sg), C.pointer(sz)
        descs[i].z_bn = C.pointer(pr["z_bn"])
        descs[i].gz = C.pointer(dz) if dz is not None else None
        descs[i].w, descs[i].wt = pr["w"].data_ptr(), pr["wt"].data_ptr()
        descs[i].bt = pr["bt"].data_ptr() if pr.get("bt") is not None else None
        descs[i].fwd_ws = pr["fwd_ws"].data_ptr()
        descs[i].ws = slots[i].data_ptr()
        descs[i].dw, descs[i].dwt = pr["dw"].data_ptr(), pr["dwt"].data_ptr()
        descs[i].dbt = pr["dbt"].data_ptr() if pr.get("dbt") is not None else None
    L.check(L.lib().pc_conv3x3_up_bwd_group(n, descs, int(accumulate), B, H, W, Cz, Cz, L.stream_ptr()), "pc_conv3x3_up_bwd_group")


def level2_bwd_ok(g2, c1, x, act, out):
    """Does the one-launch backward of the 32 x 32 level (pc_level2_bwd_group) take these tensors?"""
    adt = L.act_dtype()                    # fp32 mode: planar fp32 (level2.hip); bf16 mode: channels-last bf16 (level2_cl.hip)
    unit = 3 if adt == torch.float32 else 1
    for t, shp in ((g2, (16, 32, 32)), (c1, (16, 32, 32)), (x, (16, 32, 32)), (act, (16, 64, 64)), (out, (16, 64, 64))):
        if t is None or t.dim() != 4 or tuple(t.shape[1:]) != shp or t.dtype != adt or t.stride(unit) != 1:
            return False
    sg, sc, sx, sa, do = L.src(g2), L.src(c1), L.src(x), L.src(act), L.dst(out)
    return bool(L.lib().pc_level2_bwd_ok(C.byref(sg), C.byref(sc), C.byref(sx), C.byref(sa), C.byref(do)))


def level2_fwd_group(problems):
    """DoubleConv(16,16) + ConvTranspose2d(16,16,2,2) of the 32 x 32 level in ONE launch (networks.py:253-271,302): problems =
    list (<= 4) of dicts {x (pooled input), w1, bn1, w2, bn2, wt, bt, u2 (out), c1 / c2 (optional outs: saved activations)}."""
    n = len(problems)
    assert 1 <= n <= L.PC_MAX_GROUP
    L.require_device(problems[0]["x"])
    B = problems[0]["x"].shape[0]
    keep = []
    descs = (L.PcLevel2FwdDesc * n)()
    for i, pr in enumerate(problems):
        sx = L.src(pr["x"])
        du = L.dst(pr["u2"]) if pr.get("u2") is not None else None
        d1 = L.dst(pr["c1"]) if pr.get("c1") is not None else None
        d2 = L.dst(pr["c2"]) if pr.get("c2") is not None else None
        keep += [sx, du, d1, d2]
        descs[i].x = C.pointer(sx)
        descs[i].w1, descs[i].w2, descs[i].wt = pr["w1"].data_ptr(), pr["w2"].data_ptr(), pr["wt"].data_ptr()
        descs[i].bt = pr["bt"].data_ptr() if pr.get("bt") is not None else None
        descs[i].bn1, descs[i].bn2 = C.pointer(pr["bn1"]), C.pointer(pr["bn2"])
        descs[i].c1 = C.pointer(d1) if d1 is not None else None
        descs[i].c2 = C.pointer(d2) if d2 is not None else None
        descs[i].u2 = C.pointer(du) if du is not None else None
    L.check(L.lib().pc_level2_fwd_group(n, descs, B, L.stream_ptr()), "pc_level2_fwd_group")


def convt2x2_dgrad_group(problems):
    """Grouped convT data gradient: problems = list of {g, w, out, act, act_bn}."""
    n = len(problems)
    B, Cc, H, W = problems[0]["out"].shape
    keep, descs = [], (L.PcConvtDgradDesc * n)()
    for i, pr in enumerate(problems):
        sg, d = L.src(pr["g"]), L.dst(pr["out"])
        sa = L.src(pr["act"]) if pr.get("act") is not None else None
        keep += [sg, d, sa]
        descs[i].g, descs[i].w, descs[i].out = C.pointer(sg), pr["w"].data_ptr(), C.pointer(d)
        descs[i].act = C.pointer(sa) if sa is not None else None
        descs[i].act_bn = C.pointer(pr["act_bn"]) if pr.get("act_bn") is not None else None
    L.check(L.lib().pc_convt2x2_dgrad_group(n, descs, B, H, W, Cc, L.stream_ptr()), "pc_convt2x2_dgrad_group")


def convt2x2_dgrad(g, w, out, act=None, act_bn=None):
    L.require_device(g, w, out)
    B, Cc, H, W = out.shape
    sg, d = L.src(g), L.dst(out)
    sa = L.src(act) if act is not None else None
    L.check(L.lib().pc_convt2x2_dgrad(C.byref(sg), L.ptr(w), C.byref(sa) if sa is not None else None,
                                      C.byref(act_bn) if act_bn is not None else None, C.byref(d), B, H, W, Cc,
                                      L.stream_ptr()), "pc_convt2x2_dgrad")
    return out


def convt2x2_wgrad(x, g, dw=None, db=None, accumulate=False):
    L.require_device(x, g)
    B, Cc, H, W = x.shape
    if dw is None:
        dw = torch.empty(Cc, Cc, 2, 2, device=x.device, dtype=torch.float32)
    if db is None:
        db = torch.empty(Cc, device=x.device, dtype=torch.float32)
    wb = WgradBatch(x.device, accumulate=accumulate)
    wb.convt2x2_group([{"x": x, "g": g, "dw": dw, "db": db}])
    wb.finish()
    return dw, db


def outconv_sigmoid_crop(feat, w, bias, H, W, py, px, out=None):
    """fusion_out_conv (1x1, 16->1) + sigmoid + crop.  popcorn.py:301,317-320."""
    L.require_device(feat, w, bias)
    B = feat.shape[0]
    if out is None:
        out = torch.empty(B, 1, H, W, device=feat.device, dtype=torch.float32)
    sf, d = L.src(feat), L.dst(out)
    L.check(L.lib().pc_outconv_sigmoid_crop(C.byref(sf), L.ptr(w), L.ptr(bias), C.byref(d), B, H, W, py, px,
                                            L.stream_ptr()), "pc_outconv_sigmoid_crop")
    return out


def sparsity_mask(building, admin_mask, census_idx, rowsel, colsel, occupancymodel=True):
    """popcorn.py:361-377.  rowsel/colsel: uint8 device vectors.  Returns (mask uint8 (B,H,W), counts int32[2])."""
    L.require_device(building, admin_mask, census_idx, rowsel, colsel)
    B, H, W = admin_mask.shape
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=building.device)
    counts = torch.empty(2, dtype=torch.int32, device=building.device)
    L.check(L.lib().pc_sparsity_mask(L.ptr(building), L.ptr(admin_mask), L.ptr(census_idx), L.ptr(rowsel), L.ptr(colsel),
                                     int(occupancymodel), L.ptr(mask), L.ptr(counts), B, H, W, L.stream_ptr()),
            "pc_sparsity_mask")
    return mask, counts


def sparsity_mask_unet(building, admin_mask, census_idx, rowsel, colsel, threshold=0.001):
    """get_sparsity_mask(sparse_unet=True), popcorn.py:336-359.  Returns (mask uint8 (B,H,W), ratio float32 (B,))."""
    L.require_device(building, admin_mask, census_idx, rowsel, colsel)
    B, H, W = admin_mask.shape
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=building.device)
    ratio = torch.empty(B, dtype=torch.float32, device=building.device)
    L.check(L.lib().pc_sparsity_mask_unet(L.ptr(building), L.ptr(admin_mask), L.ptr(census_idx), L.ptr(rowsel), L.ptr(colsel),
                                          C.c_float(threshold), L.ptr(mask), L.ptr(ratio), B, H, W, L.stream_ptr()),
            "pc_sparsity_mask_unet")
    return mask, ratio


def building_score_mask(feat, w, bias, H, W, py, px, admin_mask, census_idx, rowsel, colsel, occupancymodel=True):
    """outconv_sigmoid_crop + sparsity_mask in one launch.  Returns (building (B,1,H,W), mask uint8 (B,H,W), counts)."""
    L.require_device(feat, w, bias, admin_mask, census_idx, rowsel, colsel)
    B = feat.shape[0]
    dev = feat.device
    building = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    sf, d = L.src(feat), L.dst(building)
    L.check(L.lib().pc_building_score_mask(C.byref(sf), L.ptr(w), L.ptr(bias), C.byref(d), L.ptr(admin_mask),
                                           L.ptr(census_idx), L.ptr(rowsel), L.ptr(colsel), int(occupancymodel),
                                           L.ptr(mask), L.ptr(counts), B, H, W, py, px, L.stream_ptr()),
            "pc_building_score_mask")
    return building, mask, counts


def _hw_array(head_tensors):
    arr = (C.c_void_p * 8)(*[t.data_ptr() for t in head_tensors])
    return arr


PC_HEAD_FWD_PACK_BOTH, PC_HEAD_BWD_PACKED, PC_HEAD_FWD_DEFER_REDUCE, PC_HEAD_BWD_DEFER_REDUCE = 1, 1, 2, 2


def head_fwd(feat, py, px, H, W, head_tensors, building, mask=None, admin_mask=None, census_idx=None,
             want_scale=True, stats=None, nsel_counts=None, pack_both=False, defer_reduce=False):
    """Sparse/dense head + occupancy product + census reduction.  popcorn.py:161-190.
    head_tensors = [w0,b0,w2,b2,w4,b4,w6,b6].  Returns (scale_map, popdensemap, popcount)."""
    L.require_device(feat, building, *head_tensors)
    B = feat.shape[0]
    dev = feat.device
    scale_map = torch.empty(B, H, W, device=dev, dtype=torch.float32) if want_scale else None
    popdense = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    popcount = torch.empty(B, device=dev, dtype=torch.float32)
    ws = _workspace(L.lib().pc_head_ws_bytes(B, H, W), dev)
    sf = L.src(feat)
    hw = _hw_array(head_tensors)
    L.check(L.lib().pc_head_fwd(C.byref(sf), py, px, hw, L.ptr(mask), L.ptr(building), L.ptr(admin_mask),
                                L.ptr(census_idx), L.ptr(scale_map), L.ptr(popdense), L.ptr(popcount), L.ptr(stats),
                                L.ptr(nsel_counts), L.ptr(ws), B, H, W,
                                (PC_HEAD_FWD_PACK_BOTH if pack_both else 0) | (PC_HEAD_FWD_DEFER_REDUCE if defer_reduce else 0), L.stream_ptr()),
            "pc_head_fwd")
    return scale_map, popdense, popcount


def compact_masked(src, mask):
    """src[mask] in row-major order (popcorn.py:173).  Returns (buffer of src.numel() floats, device int32 count)."""
    L.require_device(src, mask)
    n = src.numel()
    out = torch.empty(n, device=src.device, dtype=torch.float32)
    cnt = torch.empty(1, device=src.device, dtype=torch.int32)
    ws = _workspace(L.lib().pc_compact_ws_bytes(n), src.device)
    L.check(L.lib().pc_compact_masked(L.ptr(src), L.ptr(mask), L.ptr(out), L.ptr(cnt), L.ptr(ws), C.c_int64(n),
                                      L.stream_ptr()), "pc_compact_masked")
    return out, cnt


def scatter_masked(src, mask):
    """out[mask] = src (row-major), zeros elsewhere: the autograd of compact_masked / of the reference's ``scale[mask]``."""
    L.require_device(src, mask)
    n = mask.numel()
    out = torch.empty(mask.shape, device=mask.device, dtype=torch.float32)
    ws = _workspace(L.lib().pc_compact_ws_bytes(n), mask.device)
    L.check(L.lib().pc_scatter_masked(L.ptr(src), L.ptr(mask), L.ptr(out), L.ptr(ws), C.c_int64(n), L.stream_ptr()),
            "pc_scatter_masked")
    return out


def unit_layout(census_idx, census_n=None):
    """The flattened unit lists of a multi-unit batch (include/popcorn_hip.h, "multi-unit census supervision") from ``census_idx`` (B, K)
    int64 on the device -- ids non-negative and distinct within a row -- and ``census_n``: HOST data (list / CPU tensor; it sizes N), the
    valid count per row, default K; slots past it are ignored whatever they hold.  Rows are sorted on the device; nothing synchronises.
    Returns a dict: units int64 [N] (ascending per sample), unit_off int32 [B + 1], N, counts (the host list), and the two index vectors
    that carry per-slot data between the caller's (b, k) order and the sorted one: ``to_sorted`` (indices into a flattened (B, K) tensor:
    ``y.reshape(-1)[to_sorted]`` is y in sorted order) and ``to_caller`` (``popcount_sorted[to_caller]`` is in (b, k) order)."""
    L.require_device(census_idx)
    if census_idx.dim() != 2 or census_idx.dtype != torch.int64:
        raise ValueError(f"unit_layout: census_idx must be an int64 (B, K) tensor, got {census_idx.dtype} {tuple(census_idx.shape)}")
    B, K = census_idx.shape
    if census_n is None:
        counts = [K] * B
    else:
        if torch.is_tensor(census_n) and census_n.is_cuda:
            raise ValueError("census_n is host data (a list or a CPU tensor): it sizes the result")
        counts = [int(v) for v in (census_n.tolist() if torch.is_tensor(census_n) else census_n)]
    if len(counts) != B or any(c < 1 or c > K for c in counts):
        raise ValueError(f"census_n must hold B = {B} counts in [1, K = {K}], got {counts}")
    N = sum(counts)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    # host-built index plumbing (B + 1 + N + B integers) in one host-to-device copy
    rows = torch.tensor([b for b, c in enumerate(counts) for _ in range(c)], dtype=torch.int64)
    cols = torch.tensor([j for c in counts for j in range(c)], dtype=torch.int64)
    host = torch.cat([torch.tensor(off, dtype=torch.int64), rows * K + cols, torch.tensor(counts, dtype=torch.int64)])
    dev = host.to(census_idx.device, non_blocking=True)
    off_d, flat, cnt_d = dev[:B + 1], dev[B + 1:B + 1 + N], dev[B + 1 + N:]
    valid = torch.arange(K, device=census_idx.device).unsqueeze(0) < cnt_d.unsqueeze(1)
    srt, perm = torch.sort(census_idx.masked_fill(~valid, torch.iinfo(torch.int64).max), dim=1)
    units = srt.reshape(-1)[flat].contiguous()
    # sorted slot (b, j) holds the caller's slot (b, perm[b, j]); the padding sorts behind every valid id, so perm[b, j] < counts[b]
    to_sorted = (perm + torch.arange(B, device=perm.device).unsqueeze(1) * K).reshape(-1)[flat]
    dest = (perm + off_d[:B].unsqueeze(1)).reshape(-1)[flat]          # flat (b, k) position of sorted slot n
    to_caller = torch.empty(N, dtype=torch.int64, device=perm.device).scatter_(0, dest, torch.arange(N, device=perm.device))
    return {"units": units, "unit_off": off_d.to(torch.int32).contiguous(), "N": N, "counts": counts, "to_sorted": to_sorted,
            "to_caller": to_caller}


def unit_mask(building, admin_mask, units, unit_off, rowsel, colsel, occupancymodel=True, want_pixels=False):
    """pc_unit_mask: unit lookup + the multi-unit sparsity mask (popcorn.py:361-377 with the union of the listed units as the region) in
    one launch.  units int64 [N] ascending per sample, unit_off int32 [B + 1] (``unit_layout``).  Returns (slot int32 (B,H,W): the flat
    index of the listed unit that owns the pixel or -1, mask uint8 (B,H,W), counts int32[2] = {nsel, nregion}[, unit_pixels int32 [N]])."""
    L.require_device(building, admin_mask, units, unit_off, rowsel, colsel)
    B, H, W = admin_mask.shape
    N = units.numel()
    if units.dtype != torch.int64 or unit_off.dtype != torch.int32 or unit_off.numel() != B + 1 or N < 1:
        raise ValueError("unit_mask: units int64 [N >= 1], unit_off int32 [B + 1]")
    if admin_mask.dtype != torch.float32 or building.dtype != torch.float32 or building.numel() != B * H * W:
        raise ValueError("unit_mask: fp32 building (B, 1, H, W) and admin_mask (B, H, W)")
    if rowsel.numel() < H or colsel.numel() < W or rowsel.dtype != torch.uint8 or colsel.dtype != torch.uint8:
        raise ValueError("unit_mask: uint8 rowsel [H] / colsel [W]")
    building, admin_mask, units, unit_off = building.contiguous(), admin_mask.contiguous(), units.contiguous(), unit_off.contiguous()
    dev = building.device
    slot = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    pixels = torch.empty(N, dtype=torch.int32, device=dev) if want_pixels else None
    L.check(L.lib().pc_unit_mask(L.ptr(building), L.ptr(admin_mask), L.ptr(units), L.ptr(unit_off), L.ptr(rowsel.contiguous()),
                                 L.ptr(colsel.contiguous()), int(occupancymodel), L.ptr(slot), L.ptr(mask), L.ptr(counts), L.ptr(pixels),
                                 B, H, W, N, L.stream_ptr()), "pc_unit_mask")
    return (slot, mask, counts, pixels) if want_pixels else (slot, mask, counts)


def unit_popcount(popdense, slot, N, unit_off=None, out=None):
    """pc_unit_popcount: popcount[n] = sum of popdense (B,H,W) over slot == n -- bit-reproducible (fixed-point sums, quantum
    ``L.PC_UNIT_QUANTUM`` per term); a NaN / +-Inf / out-of-range term makes its unit's popcount NaN.  unit_off (optional): the sample
    ranges, for the LDS bins.  Returns popcount fp32 [N]."""
    L.require_device(popdense, slot)
    if popdense.dim() != 3 or popdense.dtype != torch.float32 or slot.dtype != torch.int32 or slot.shape != popdense.shape or int(N) < 1:
        raise ValueError(f"unit_popcount: fp32 popdense (B, H, W) and int32 slot of the same shape, N >= 1; got {popdense.dtype} "
                         f"{tuple(popdense.shape)}, {slot.dtype} {tuple(slot.shape)}, N = {N}")
    popdense, slot = popdense.contiguous(), slot.contiguous()
    B, H, W = popdense.shape
    if unit_off is not None and (unit_off.dtype != torch.int32 or unit_off.numel() != B + 1 or not unit_off.is_cuda):
        raise ValueError("unit_popcount: unit_off int32 [B + 1] on the device")
    if out is None:
        out = torch.empty(int(N), dtype=torch.float32, device=popdense.device)
    # a workspace of its own: the head's (packed weight images of a training step) must survive between head_fwd and head_bwd
    ws = _workspace(L.lib().pc_unit_ws_bytes(int(N)), popdense.device, "units")
    L.check(L.lib().pc_unit_popcount(L.ptr(popdense), L.ptr(slot), L.ptr(None if unit_off is None else unit_off.contiguous()), L.ptr(out),
                                     L.ptr(ws), B, H, W, int(N), L.stream_ptr()), "pc_unit_popcount")
    return out


def unit_paint(g_popcount, slot, out=None):
    """pc_unit_paint: out[b,y,x] = g_popcount[slot[b,y,x]] (0 where slot < 0), every element written: the autograd of ``unit_popcount``."""
    L.require_device(g_popcount, slot)
    if g_popcount.dtype != torch.float32 or g_popcount.dim() != 1 or g_popcount.numel() < 1 or slot.dtype != torch.int32:
        raise ValueError("unit_paint: fp32 g_popcount [N >= 1] and an int32 slot map")
    g_popcount, slot = g_popcount.contiguous(), slot.contiguous()
    if out is None:
        out = torch.empty(slot.shape, dtype=torch.float32, device=slot.device)
    if out.shape != slot.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("unit_paint: out must be a contiguous fp32 tensor of the slot map's shape")
    L.check(L.lib().pc_unit_paint(L.ptr(g_popcount), L.ptr(slot), L.ptr(out), C.c_int64(slot.numel()), g_popcount.numel(),
                                  L.stream_ptr()), "pc_unit_paint")
    return out


def _unit_counts(census_n, B, K):
    """The host list of valid counts per row (``unit_layout``'s rules)."""
    if census_n is None:
        return [K] * B
    if torch.is_tensor(census_n) and census_n.is_cuda:
        raise ValueError("census_n is host data (a list or a CPU tensor): it sizes the result")
    counts = [int(v) for v in (census_n.tolist() if torch.is_tensor(census_n) else census_n)]
    if len(counts) != B or any(c < 1 or c > K for c in counts):
        raise ValueError(f"census_n must hold B = {B} counts in [1, K = {K}], got {counts}")
    return counts


def unit_layout_device(census_idx, y, census_n=None, ws=None):
    """pc_unit_layout: ``unit_layout`` as ONE launch (rows sorted in LDS, the host counts in the kernel arguments: no sort, gather or
    host-to-device copy), for the executor-style tail ``unit_popcount_loss``.  census_idx (B, K) int64 and y (B, K) fp32 on the device,
    census_n host data.  Returns a dict: units, unit_off, N, counts as ``unit_layout``; y_sorted fp32 [N]; dest int32 [N], the flat
    (b, k) position over the valid slots of sorted slot n; ws, the workspace of the unit sums, zeroed over its 20 N bytes by the launch
    (``ws``: a uint8 tensor of at least pc_unit_ws_bytes(N) bytes to use instead of a fresh one).  K above L.PC_UNIT_LAYOUT_MAX_K or B
    above L.PC_UNIT_LAYOUT_MAX_B raises (PC_ENOTSUP): ``unit_layout`` takes those."""
    L.require_device(census_idx, y)
    if census_idx.dim() != 2 or census_idx.dtype != torch.int64:
        raise ValueError(f"unit_layout_device: census_idx must be an int64 (B, K) tensor, got {census_idx.dtype} {tuple(census_idx.shape)}")
    if y.dtype != torch.float32 or tuple(y.shape) != tuple(census_idx.shape):
        raise ValueError(f"unit_layout_device: y must be fp32 {tuple(census_idx.shape)} like census_idx, got {y.dtype} {tuple(y.shape)}")
    B, K = census_idx.shape
    counts = _unit_counts(census_n, B, K)
    N = sum(counts)
    dev = census_idx.device
    census_idx, y = census_idx.contiguous(), y.contiguous()
    units = torch.empty(N, dtype=torch.int64, device=dev)
    unit_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    y_sorted = torch.empty(N, dtype=torch.float32, device=dev)
    dest = torch.empty(N, dtype=torch.int32, device=dev)
    need = L.lib().pc_unit_ws_bytes(N)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_cuda or ws.data_ptr() % 16:
        raise ValueError(f"unit_layout_device: ws must be a 16-byte aligned uint8 device tensor of at least {need} bytes")
    L.check(L.lib().pc_unit_layout(L.ptr(census_idx), L.ptr(y), (C.c_int32 * B)(*counts), B, K, L.ptr(units), L.ptr(unit_off),
                                   L.ptr(y_sorted), L.ptr(dest), L.ptr(ws), L.stream_ptr()), "pc_unit_layout")
    return {"units": units, "unit_off": unit_off, "N": N, "counts": counts, "y_sorted": y_sorted, "dest": dest, "ws": ws}


def unit_popcount_loss(popdense, slot, lay, stats, lam4, scale_regularization, lam_weak, loss_out, g_popcount, g_scale_const):
    """pc_unit_popcount_loss on a ``unit_layout_device`` result: ``unit_popcount`` + ``loss_fwd_bwd`` over the N pairs (inv_B = 1 / N)
    in two launches, bit-identical to the two calls.  Consumes the zeroed workspace ``lay["ws"]`` (one call per layout).  g_popcount
    fp32 [N], in the sorted order (``unit_paint``'s).  Returns (popcount in the sorted order, popcount in the caller's (b, k) order)."""
    L.require_device(popdense, slot, g_popcount)
    N = int(lay["N"])
    if popdense.dim() != 3 or popdense.dtype != torch.float32 or slot.dtype != torch.int32 or slot.shape != popdense.shape:
        raise ValueError("unit_popcount_loss: fp32 popdense (B, H, W) and an int32 slot map of the same shape")
    if g_popcount.dtype != torch.float32 or g_popcount.numel() != N or not g_popcount.is_contiguous():
        raise ValueError(f"unit_popcount_loss: g_popcount must be a contiguous fp32 tensor of N = {N} elements")
    popdense, slot = popdense.contiguous(), slot.contiguous()
    B, H, W = popdense.shape
    pc_sorted = torch.empty(N, dtype=torch.float32, device=popdense.device)
    pc_caller = torch.empty(N, dtype=torch.float32, device=popdense.device)
    L.check(L.lib().pc_unit_popcount_loss(L.ptr(popdense), L.ptr(slot), L.ptr(lay["unit_off"]), L.ptr(lay["dest"]), L.ptr(lay["y_sorted"]),
                                          L.ptr(lay["ws"]), L.ptr(pc_sorted), L.ptr(pc_caller), L.ptr(stats), (C.c_float * 4)(*lam4),
                                          C.c_float(scale_regularization), C.c_float(lam_weak), B, H, W, N, L.ptr(loss_out),
                                          L.ptr(g_popcount), L.ptr(g_scale_const), L.stream_ptr()), "pc_unit_popcount_loss")
    return pc_sorted, pc_caller


def unit_layout_dev(census_idx, y, census_n_dev, stats=None, ws=None):
    """pc_unit_layout_dev: ``unit_layout_device`` with the counts on the DEVICE (``census_n_dev`` int32 [B]; a count outside [1, K] is
    clamped into it -- the device cannot raise, callers validate on the host) and nothing sized by them: every result has the capacity
    Ncap = B * K and is written completely by the one launch.  Returns a dict: units int64 [Ncap] (tail INT64_MAX), unit_off int32 [B + 1]
    (unit_off[B] = N), y_sorted fp32 [Ncap] (tail 0), dest int32 [Ncap] (tail -1), ws (20 Ncap bytes zeroed: the sums' workspace laid out
    by Ncap), n_dev int32 [1] = N, Ncap.  stats (optional): a float64 tensor of at least 3 elements, stats[2] := N.  K above
    L.PC_UNIT_LAYOUT_MAX_K or B above L.PC_UNIT_LAYOUT_MAX_B raises (PC_ENOTSUP)."""
    L.require_device(census_idx, y, census_n_dev, stats)
    if census_idx.dim() != 2 or census_idx.dtype != torch.int64:
        raise ValueError(f"unit_layout_dev: census_idx must be an int64 (B, K) tensor, got {census_idx.dtype} {tuple(census_idx.shape)}")
    if y.dtype != torch.float32 or tuple(y.shape) != tuple(census_idx.shape):
        raise ValueError(f"unit_layout_dev: y must be fp32 {tuple(census_idx.shape)} like census_idx, got {y.dtype} {tuple(y.shape)}")
    B, K = census_idx.shape
    if census_n_dev.dtype != torch.int32 or census_n_dev.numel() != B or not census_n_dev.is_contiguous():
        raise ValueError(f"unit_layout_dev: census_n_dev must be a contiguous int32 [B = {B}] device tensor, got {census_n_dev.dtype} "
                         f"{tuple(census_n_dev.shape)}")
    if stats is not None and (stats.dtype != torch.float64 or stats.numel() < 3 or not stats.is_contiguous()):
        raise ValueError("unit_layout_dev: stats must be a contiguous float64 tensor of at least 3 elements")
    Ncap = B * K
    if Ncap < 1:
        raise ValueError("unit_layout_dev: B >= 1 and K >= 1")
    dev = census_idx.device
    census_idx, y = census_idx.contiguous(), y.contiguous()
    units = torch.empty(Ncap, dtype=torch.int64, device=dev)
    unit_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
    y_sorted = torch.empty(Ncap, dtype=torch.float32, device=dev)
    dest = torch.empty(Ncap, dtype=torch.int32, device=dev)
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    need = L.lib().pc_unit_ws_bytes(Ncap)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_cuda or ws.data_ptr() % 16:
        raise ValueError(f"unit_layout_dev: ws must be a 16-byte aligned uint8 device tensor of at least {need} bytes")
    L.check(L.lib().pc_unit_layout_dev(L.ptr(census_idx), L.ptr(y), L.ptr(census_n_dev), B, K, L.ptr(units), L.ptr(unit_off),
                                       L.ptr(y_sorted), L.ptr(dest), L.ptr(ws), L.ptr(n_dev), L.ptr(stats), L.stream_ptr()),
            "pc_unit_layout_dev")
    return {"units": units, "unit_off": unit_off, "Ncap": Ncap, "y_sorted": y_sorted, "dest": dest, "ws": ws, "n_dev": n_dev}


def unit_popcount_loss_dev(popdense, slot, lay, stats, lam4, scale_regularization, lam_weak, loss_out, g_popcount, g_scale_const,
                           out=None):
    """pc_unit_popcount_loss_dev on a ``unit_layout_dev`` result: ``unit_popcount_loss`` at the capacity Ncap, with N read from
    ``lay["n_dev"]`` and 1 / N formed on the device from stats[2] (``unit_layout_dev`` left the local N there; a data-parallel step
    all-reduces ``stats`` in between).  Consumes the zeroed workspace (one call per layout).  g_popcount fp32 [Ncap], sorted order, tail
    0.  out: (popcount_sorted, popcount_caller) to write into.  Returns (popcount in the sorted order, in the caller's (b, k) order),
    Ncap elements each, the first N valid, the rest 0."""
    L.require_device(popdense, slot, g_popcount, stats)
    Ncap = int(lay["Ncap"])
    if popdense.dim() != 3 or popdense.dtype != torch.float32 or slot.dtype != torch.int32 or slot.shape != popdense.shape:
        raise ValueError("unit_popcount_loss_dev: fp32 popdense (B, H, W) and an int32 slot map of the same shape")
    if g_popcount.dtype != torch.float32 or g_popcount.numel() != Ncap or not g_popcount.is_contiguous():
        raise ValueError(f"unit_popcount_loss_dev: g_popcount must be a contiguous fp32 tensor of Ncap = {Ncap} elements")
    if stats.dtype != torch.float64 or stats.numel() < 3 or not stats.is_contiguous():
        raise ValueError("unit_popcount_loss_dev: stats must be a contiguous float64 tensor of at least 3 elements {Nsel, sum scale, N}")
    popdense, slot = popdense.contiguous(), slot.contiguous()
    B, H, W = popdense.shape
    if lay["unit_off"].numel() != B + 1 or lay["ws"].numel() < L.lib().pc_unit_ws_bytes(Ncap):
        raise ValueError("unit_popcount_loss_dev: the layout belongs to another batch")
    if out is None:
        out = (torch.empty(Ncap, dtype=torch.float32, device=popdense.device), torch.empty(Ncap, dtype=torch.float32, device=popdense.device))
    pc_sorted, pc_caller = out
    for t in out:
        if t.dtype != torch.float32 or t.numel() != Ncap or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"unit_popcount_loss_dev: out must be two contiguous fp32 device tensors of Ncap = {Ncap} elements")
    L.check(L.lib().pc_unit_popcount_loss_dev(L.ptr(popdense), L.ptr(slot), L.ptr(lay["unit_off"]), L.ptr(lay["dest"]),
                                              L.ptr(lay["y_sorted"]), L.ptr(lay["ws"]), L.ptr(lay["n_dev"]), L.ptr(pc_sorted),
                                              L.ptr(pc_caller), L.ptr(stats), (C.c_float * 4)(*lam4), C.c_float(scale_regularization),
                                              C.c_float(lam_weak), B, H, W, Ncap, L.ptr(loss_out), L.ptr(g_popcount), L.ptr(g_scale_const),
                                              L.stream_ptr()), "pc_unit_popcount_loss_dev")
    return pc_sorted, pc_caller


class UnitPopcount(torch.autograd.Function):
    """popcount[N] = ``unit_popcount(popdense, slot, N)``; backward: ``unit_paint``.  slot / unit_off get no gradient."""

    @staticmethod
    def forward(ctx, popdense, slot, N, unit_off=None):
        ctx.slot = slot
        return unit_popcount(popdense.detach(), slot, N, unit_off)

    @staticmethod
    def backward(ctx, g):
        return unit_paint(g.contiguous().float(), ctx.slot), None, None, None


def reflect_pad(x, top, bottom, left, right):
    """F.pad(x, (left, right, top, bottom), mode='reflect') for a contiguous (..., H, W) fp32 tensor."""
    L.require_device(x)
    x = x.contiguous()
    H, W = x.shape[-2:]
    out = torch.empty(*x.shape[:-2], H + top + bottom, W + left + right, device=x.device, dtype=torch.float32)
    planes = x.numel() // (H * W)
    L.check(L.lib().pc_reflect_pad(L.ptr(x), L.ptr(out), C.c_int64(planes), H, W, top, bottom, left, right, L.stream_ptr()),
            "pc_reflect_pad")
    return out


def reflect_pad_select(x, sel, top, bottom, left, right):
    """out[b][j] = F.pad(x[b][sel[j]], reflect): the padded, channel-gathered copy of a (B, C, H, W) fp32 input."""
    L.require_device(x)
    x = x.contiguous()
    B, Cin, H, W = x.shape
    out = torch.empty(B, len(sel), H + top + bottom, W + left + right, device=x.device, dtype=torch.float32)
    arr = (C.c_int * len(sel))(*[int(v) for v in sel])
    L.check(L.lib().pc_reflect_pad_select(L.ptr(x), L.ptr(out), B, Cin, len(sel), arr, H, W, top, bottom, left, right, L.stream_ptr()),
            "pc_reflect_pad_select")
    return out


def select_normalize_pad(raw, band, mean, std, top, bottom, left, right, out=None):
    """Band selection + (x - mean) / std + reflect padding in one pass: out[b][j] = pad((raw[b][band[j]] - mean[j]) / std[j])."""
    L.require_device(raw)
    assert raw.is_contiguous() and raw.dtype == torch.float32
    B, Craw, H, W = raw.shape
    n = len(band)
    if out is None:
        out = torch.empty(B, n, H + top + bottom, W + left + right, device=raw.device, dtype=torch.float32)
    L.check(L.lib().pc_select_normalize_pad(L.ptr(raw), L.ptr(out), B, Craw, n, (C.c_int * n)(*[int(v) for v in band]),
                                            (C.c_float * n)(*[float(v) for v in mean]), (C.c_float * n)(*[float(v) for v in std]),
                                            H, W, top, bottom, left, right, L.stream_ptr()), "pc_select_normalize_pad")
    return out


def ingest_cl8(raw, band, mean, std, top, bottom, left, right, out=None):
    """PC_PREC_BF16 ingest (pc_ingest_cl8): band selection + (x - mean) / std (mean / std None: already normalised) + reflect padding
    of a planar fp32 (B, Craw, H, W) tile into ONE channels-last bf16 tensor (B, 8, Hp, Wp): channel j = the j-th selected band,
    channels >= len(band) zero."""
    L.require_device(raw)
    assert raw.is_contiguous() and raw.dtype == torch.float32
    B, Craw, H, W = raw.shape
    n = len(band)
    if out is None:
        out = torch.empty(B, 8, H + top + bottom, W + left + right, device=raw.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    assert out.stride(1) == 1 and out.stride(3) == 8
    fa = lambda v: None if v is None else (C.c_float * n)(*[float(t) for t in v])  # noqa: E731
    L.check(L.lib().pc_ingest_cl8(L.ptr(raw), L.ptr(out), B, Craw, n, (C.c_int * n)(*[int(v) for v in band]), fa(mean), fa(std),
                                  H, W, top, bottom, left, right, L.stream_ptr()), "pc_ingest_cl8")
    return out


def ingest_split(s2_u16, s1, band, mean, std, top, bottom, left, right, cl8=None):
    """pc_ingest_split: the one-pass ingest (band select + normalise + reflect padding + stream order) from the two tensors a loader
    ships -- s2_u16 (B, C2, H, W) uint16 reflectance digital numbers, s1 (B, C1, H, W) fp32 -- into the padded model input of the
    current arithmetic mode (cl8 None): planar fp32 (B, n, Hp, Wp) or the channels-last bf16 slot tensor (B, 8, Hp, Wp).  band indexes
    [s2 | s1]."""
    L.require_device(s2_u16, s1)
    assert s2_u16.dtype == torch.uint16 and s1.dtype == torch.float32 and s2_u16.is_contiguous() and s1.is_contiguous()
    B, C2, H, W = s2_u16.shape
    C1 = s1.shape[1]
    assert tuple(s1.shape) == (B, C1, H, W)
    n = len(band)
    if cl8 is None:
        cl8 = L.act_dtype() == torch.bfloat16
    Hp, Wp = H + top + bottom, W + left + right
    if cl8:
        out = torch.empty(B, 8, Hp, Wp, device=s1.device, dtype=torch.bfloat16, memory_format=torch.channels_last)
    else:
        out = torch.empty(B, n, Hp, Wp, device=s1.device, dtype=torch.float32)
    fa = lambda v: (C.c_float * n)(*[float(t) for t in v])  # noqa: E731
    L.check(L.lib().pc_ingest_split(L.ptr(s2_u16), C2, L.ptr(s1), C1, L.ptr(out), int(bool(cl8)), B, n, (C.c_int * n)(*[int(v) for v in band]),
                                    fa(mean), fa(std), H, W, top, bottom, left, right, L.stream_ptr()), "pc_ingest_split")
    return out


def head_bwd(feat, py, px, H, W, head_tensors, building, mask=None, admin_mask=None, census_idx=None,
             g_popcount=None, g_popdense=None, g_scale_map=None, g_scale_const=None, grads=None, accumulate=False,
             g_feat=None, feat_bn=None, packed=False, defer_reduce=False, decisions=None):
    """Backward of head_fwd.  Returns (list of 8 head grads, g_feat (B,16,Hp,Wp)).  pack_both (head_fwd) / packed (here): a training
    step's forward call assembles the backward's weight image too (same weights, same workspace): one launch less.  defer_reduce:
    the weight gradients stay per-workgroup partials; returns (HeadPartials, g_feat) instead -- hand the first to the
    ``WgradBatch`` of the same backward pass (``head_reduce``), whose batched reduction writes ``grads``: one launch less.
    decisions (debug, fp32 mode): a contiguous int64 device tensor of at least B * H * W * 4 words (``head_decision_buffer``) that
    receives the ReLU decisions the kernel takes (pc_debug_head_decisions; decode with ``decode_head_decisions``); everything else the
    call returns is bit-equal to the call without it."""
    L.require_device(feat, building, *head_tensors)
    B, _, Hp, Wp = feat.shape
    dev = feat.device
    if grads is None:
        grads = [torch.empty_like(t) for t in head_tensors]
    if g_feat is None:
        g_feat = L.empty_act(B, 16, Hp, Wp, dev)
    ws = _workspace(L.lib().pc_head_ws_bytes(B, H, W), dev)
    sf, d = L.src(feat), L.dst(g_feat)
    hw = _hw_array(head_tensors)
    dhw = (C.c_void_p * 8)(*[0 if t is None else t.data_ptr() for t in grads])
    if decisions is not None:
        L.require_device(decisions)
        assert decisions.dtype == torch.int64 and decisions.is_contiguous()
        L.lib().pc_debug_head_decisions(L.ptr(decisions), C.c_int64(decisions.numel() * 8))
    try:
        code = L.lib().pc_head_bwd(C.byref(sf), py, px, hw, L.ptr(mask), L.ptr(building), L.ptr(admin_mask),
                                   L.ptr(census_idx), L.ptr(g_popcount), L.ptr(g_popdense), L.ptr(g_scale_map),
                                   L.ptr(g_scale_const), dhw, int(accumulate), C.byref(d),
                                   C.byref(feat_bn[0]) if feat_bn else None, C.byref(feat_bn[1]) if feat_bn else None,
                                   Hp, Wp, L.ptr(ws), B, H, W,
                                   (PC_HEAD_BWD_PACKED if packed else 0) | (PC_HEAD_BWD_DEFER_REDUCE if defer_reduce else 0),
                                   L.stream_ptr())
    finally:
        if decisions is not None:
            L.lib().pc_debug_head_decisions(None, C.c_int64(0))
    L.check(code, "pc_head_bwd")
    if defer_reduce:
        pp, nwg = C.c_void_p(0), C.c_int(0)
        L.check(L.lib().pc_head_bwd_partials(L.ptr(ws), B, H, W, C.byref(pp), C.byref(nwg)), "pc_head_bwd_partials")
        return HeadPartials(pp.value, nwg.value, list(grads), bool(accumulate)), g_feat
    return grads, g_feat


HEAD_DEC_WORDS = 4          # int64 words per pixel record (PC_HEAD_DEC_BYTES / 8)


def head_decision_buffer(B, H, W, device):
    """Zeroed record buffer for ``head_bwd(decisions=...)``: (B * H * W, 4) int64."""
    return torch.zeros(B * H * W, HEAD_DEC_WORDS, device=device, dtype=torch.int64)


def decode_head_decisions(buf, mask=None):
    """The records of pc_debug_head_decisions (popcorn_hip.h: word k of a pixel's record, bit 16 l + 4 m + r = unit 16 m + 4 k + r of
    hidden layer l is positive; bit 48 = the output decision; bit 63 = written) -> (hidden (3, 64, Nsel) bool, out (Nsel,) bool) on
    the pixels ``mask`` (B, H, W) selects (None: all), in the order of the reference's sparse head: row-major over (b, h, w).  Raises
    when a selected record was not written or its four words disagree on the output decision."""
    w = buf.reshape(-1, HEAD_DEC_WORDS).cpu()
    if mask is not None:
        w = w[mask.reshape(-1).bool().cpu()]
    if not bool((w < 0).all()):
        raise ValueError("decision record of a selected pixel was not written")
    hidden = torch.zeros(3, 64, w.shape[0], dtype=torch.bool)
    for layer in range(3):
        for k in range(HEAD_DEC_WORDS):
            for m in range(4):
                for r in range(4):
                    hidden[layer, 16 * m + 4 * k + r] = ((w[:, k] >> (16 * layer + 4 * m + r)) & 1).bool()
    out = ((w >> 48) & 1).bool()
    if not bool((out == out[:, :1]).all()):
        raise ValueError("the four words of a decision record disagree on the output decision")
    if bool(((w & 0x7FFE000000000000) != 0).any()):
        raise ValueError("reserved bits of a decision record are set")
    return hidden, out[:, 0]


class HeadPartials:
    """The unreduced weight-gradient partials of a ``head_bwd(defer_reduce=True)`` call: (device pointer, workgroups, the 8 gradient
    tensors they are to be summed into -- None = skip --, accumulate)."""

    def __init__(self, ptr_, nwg, grads, accumulate):
        self.ptr, self.nwg, self.grads, self.accumulate = ptr_, nwg, grads, accumulate


def select_normalize(raw, band6, mean6, std6, out=None):
    """Band selection + (x - mean) / std.  PopulationDataset.py:566-568 + utils/utils.py:105-127."""
    L.require_device(raw)
    B, Craw, H, W = raw.shape
    assert raw.is_contiguous() and raw.dtype == torch.float32
    if out is None:
        out = torch.empty(B, 6, H, W, device=raw.device, dtype=torch.float32)
    L.check(L.lib().pc_select_normalize(L.ptr(raw), Craw, (C.c_int * 6)(*band6), (C.c_float * 6)(*mean6),
                                        (C.c_float * 6)(*std6), L.ptr(out), B, H, W, L.stream_ptr()),
            "pc_select_normalize")
    return out


def block_sum(map, cell):
    """``cell`` x ``cell`` sum pooling of a (H, W) fp32 device map onto the product grid (csrc/product.hip: cells anchored at pixel (0, 0),
    partial cells at the bottom / right sum what exists; no atomics, bit-reproducible).  Returns (ceil(H / cell), ceil(W / cell))."""
    L.require_device(map)
    if map.dim() != 2 or map.dtype != torch.float32 or int(cell) < 1 or map.numel() == 0:
        raise ValueError(f"block_sum: a non-empty fp32 (H, W) map and cell >= 1, got {map.dtype} {tuple(map.shape)}, cell {cell}")
    map = map.contiguous()
    H, W = map.shape
    cell = int(cell)
    out = torch.empty(-(-H // cell), -(-W // cell), dtype=torch.float32, device=map.device)
    L.check(L.lib().pc_block_sum(L.ptr(map), H, W, cell, L.ptr(out), L.stream_ptr()), "pc_block_sum")
    return out


def census_paint(boundary, tables, out=None):
    """Per-unit tables painted onto the raster (csrc/census_table.hip, pc_census_paint): out[k][i] = tables[k][boundary[i]] for ids in
    [0, num_ids), 0 elsewhere, for K <= PC_CENSUS_MAX_PLANES tables in ONE pass over the boundary plane.  boundary: int32 device map
    (h, w) with contiguous rows stacked without gaps (a row band of a larger map is fine: any 4-byte aligned start); tables: (K, num_ids)
    fp32 or a list of K (num_ids,) fp32 tensors.  out: optional (K, h, w) fp32 result (or a list of K band views).  Returns (K, h, w)."""
    tables = [t.contiguous() for t in tables]
    L.require_device(boundary, *tables)
    K = len(tables)
    if boundary.dim() != 2 or boundary.dtype != torch.int32 or not boundary.is_contiguous():
        raise ValueError(f"census_paint: a contiguous int32 (h, w) boundary, got {boundary.dtype} {tuple(boundary.shape)}")
    if not 1 <= K <= L.PC_CENSUS_MAX_PLANES or any(t.dtype != torch.float32 or t.dim() != 1 or t.numel() != tables[0].numel() or
                                                   t.numel() < 1 for t in tables):
        raise ValueError(f"census_paint: 1 .. {L.PC_CENSUS_MAX_PLANES} fp32 tables of one length >= 1, got {K}")
    if out is None:
        out = torch.empty(K, *boundary.shape, dtype=torch.float32, device=boundary.device)
    planes = [out[k] for k in range(K)]
    if any(p.shape != boundary.shape or p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda for p in planes):
        raise ValueError("census_paint: out must hold K contiguous fp32 device planes of the boundary's shape")
    tp = (C.c_void_p * K)(*[t.data_ptr() for t in tables])
    op = (C.c_void_p * K)(*[p.data_ptr() for p in planes])
    L.check(L.lib().pc_census_paint(L.ptr(boundary), C.c_int64(boundary.numel()), tables[0].numel(), K, tp, op, L.stream_ptr()),
            "pc_census_paint")
    return out


def census_pair_plan(b_l, b_a, num_l, num_a):
    """The (unit of level l, unit of level a) pairs of two id rasters as one more id raster (csrc/census_adjust.hip,
    pc_census_pair_plan): what ``eval.CensusTable(adjust=...)`` accumulates beside the levels.  b_l / b_a: int32 device maps of one shape,
    rows stacked without gaps (a row band of a larger map is fine: any 4-byte aligned start); a pixel belongs to f = b_l[p] when
    0 <= f < num_l and to c = b_a[p] when 0 <= c < num_a.  Returns (pair_plane (h, w) int32: the compact pair id, -1 where f or c is no
    unit; pair_f (NP,), pair_c (NP,) int32: the pairs, ordered by (f, c); base (num_l + 1,) int32: pairs of unit f are base[f] ..
    base[f + 1]).  A function of the two rasters alone.  Raises ValueError, naming the smallest such unit, when a unit of level l meets
    more than PC_CENSUS_PAIR_SLOTS units of level a (one host synchronisation: NP sizes the table)."""
    L.require_device(b_l, b_a)
    for b in (b_l, b_a):
        if b.dim() != 2 or b.dtype != torch.int32 or not b.is_contiguous() or b.shape != b_l.shape:
            raise ValueError(f"census_pair_plan: two contiguous int32 (h, w) maps of one shape, got {b.dtype} {tuple(b.shape)}")
    num_l, num_a = int(num_l), int(num_a)
    if num_l < 1 or num_a < 1 or num_l * (L.PC_CENSUS_PAIR_SLOTS + 1) >= 1 << 31:
        raise ValueError(f"census_pair_plan: num_l, num_a >= 1 and {L.PC_CENSUS_PAIR_SLOTS + 1} * num_l < 2^31, got {num_l}, {num_a}")
    dev = b_l.device
    partners = torch.empty(num_l, L.PC_CENSUS_PAIR_SLOTS, dtype=torch.int32, device=dev)
    count = torch.empty(num_l, dtype=torch.int32, device=dev)
    scratch = torch.empty(num_l, dtype=torch.int32, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    n = C.c_int64(b_l.numel())
    L.check(L.lib().pc_census_pair_plan(L.ptr(b_l), L.ptr(b_a), n, num_l, num_a, L.ptr(partners), L.ptr(count), L.ptr(flags),
                                        L.ptr(scratch), None, None, L.stream_ptr()), "pc_census_pair_plan")
    over, first = flags.tolist()
    if over:
        raise ValueError(f"census_pair_plan: unit {first} of the judged level shares pixels with more than {L.PC_CENSUS_PAIR_SLOTS} units "
                         f"of the level adjusted to (it is the smallest such unit); the adjusted table holds at most "
                         f"{L.PC_CENSUS_PAIR_SLOTS} partners per unit")
    base = torch.zeros(num_l + 1, dtype=torch.int32, device=dev)
    base[1:] = torch.cumsum(count, 0)
    pair_plane = torch.empty(b_l.shape, dtype=torch.int32, device=dev)
    L.check(L.lib().pc_census_pair_plan(L.ptr(b_l), L.ptr(b_a), n, num_l, num_a, L.ptr(partners), None, None, None, L.ptr(base),
                                        L.ptr(pair_plane), L.stream_ptr()), "pc_census_pair_plan")
    held = partners >= 0
    pair_c = partners[held]                                             # row-major: ordered by (f, c)
    pair_f = torch.arange(num_l, dtype=torch.int32, device=dev).repeat_interleave(count.long())
    return pair_plane, pair_f, pair_c, base


def region_units(boundary, num_ids, max_blocks=0):
    """The census bookkeeping of a boundary raster in one device pass (csrc/region.hip, pc_region_units; the reference: one Python pass per
    unit, utils/02_preprocess_rwa_shapefile.py:142-161).  boundary: contiguous int32 device map (h, w), h * w < 2^31.  Returns (table int32
    (num_ids, 5) = {xmin, xmax, ymin, ymax, count} -- x indexes rows, y columns, maxima exclusive, zeros for a unit without pixels --, stray
    int64 (): the pixels whose id lies outside [0, num_ids), which contribute nothing).  Bit-reproducible for any launch geometry;
    max_blocks > 0 caps the workgroups of the pass (tests)."""
    L.require_device(boundary)
    if boundary.dim() != 2 or boundary.dtype != torch.int32 or not boundary.is_contiguous() or boundary.numel() == 0:
        raise ValueError(f"region_units: a non-empty contiguous int32 (h, w) boundary, got {boundary.dtype} {tuple(boundary.shape)}")
    h, w = boundary.shape
    num_ids = int(num_ids)
    if num_ids < 1 or 5 * num_ids >= 1 << 31 or h * w >= 1 << 31:
        raise ValueError(f"region_units: num_ids >= 1 and h * w < 2^31, got num_ids {num_ids}, raster {h} x {w}")
    table = torch.empty(num_ids, 5, dtype=torch.int32, device=boundary.device)
    stray = torch.empty((), dtype=torch.int64, device=boundary.device)
    L.check(L.lib().pc_region_units(L.ptr(boundary), h, w, num_ids, L.ptr(table), L.ptr(stray), int(max_blocks), L.stream_ptr()),
            "pc_region_units")
    return table, stray


def _region_sources(what, s2, s1, boundary, band_sel):
    """The resident rasters and the band selection every ``region_*`` wrapper takes (boundary None: the entry point reads none).
    Returns (S, C2, C1, h, w, band); raises before anything is enqueued."""
    L.require_device(s2, s1)
    if s2.dim() != 4 or s2.dtype not in (torch.float32, torch.uint16) or not s2.is_contiguous():
        raise ValueError(f"{what}: s2 must be a contiguous fp32 or uint16 (S, C, h, w) tensor, got {s2.dtype} {tuple(s2.shape)}")
    S, C2, h, w = s2.shape
    if s1.dim() != 4 or s1.dtype != torch.float32 or not s1.is_contiguous() or s1.shape[0] != S or tuple(s1.shape[2:]) != (h, w):
        raise ValueError(f"{what}: s1 must be a contiguous fp32 ({S}, C, {h}, {w}) tensor, got {s1.dtype} {tuple(s1.shape)}")
    if boundary is not None:
        L.require_device(boundary)
        if boundary.dtype != torch.int32 or tuple(boundary.shape) != (h, w) or not boundary.is_contiguous():
            raise ValueError(f"{what}: boundary must be a contiguous int32 ({h}, {w}) map, got {boundary.dtype} {tuple(boundary.shape)}")
    if h * w == 0 or h * w >= 1 << 31:
        raise ValueError(f"{what}: 0 < h * w < 2^31, got {h} x {w}")
    C1 = s1.shape[1]
    band = [int(v) for v in band_sel]
    if len(band) != 6 or any(not 0 <= v < C2 for v in band[:4]) or any(not 0 <= v < C1 for v in band[4:]):
        raise ValueError(f"{what}: band_sel names four of {C2} S2 bands and two of {C1} S1 bands (0-based), got {band}")
    return S, C2, C1, h, w, band


def _region_crops(what, crops, S, h, w):
    """The host crop list {x0, x1, y0, y1, season} of a ``region_*`` wrapper over an (h, w) raster of S seasons.  Returns (crops as int32
    (B, 5), the batch maximum (Hm, Wm)); raises before anything is enqueued."""
    if torch.is_tensor(crops):
        if crops.is_cuda:
            raise ValueError(f"{what}: crops is host data (it travels in the kernel arguments)")
        crops = crops.numpy()
    # (numpy: a handful of vectorised checks -- this wrapper runs once per training batch, next to a kernel of a few microseconds)
    cr = np.ascontiguousarray(np.asarray(crops, dtype=np.int64).reshape(-1, 5))
    if cr.shape[0] < 1:
        raise ValueError(f"{what}: at least one crop")
    hb, wb = cr[:, 1] - cr[:, 0], cr[:, 3] - cr[:, 2]
    bad = (cr[:, 0] < 0) | (hb <= 0) | (cr[:, 1] > h) | (cr[:, 2] < 0) | (wb <= 0) | (cr[:, 3] > w) | (cr[:, 4] < 0) | (cr[:, 4] >= S)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{what}: crop {i} = {cr[i].tolist()} is empty, leaves the {h} x {w} raster or names a season outside "
                         f"[0, {S})")
    return cr.astype(np.int32), int(hb.max()), int(wb.max())


def _region_inputs(what, s2, s1, boundary, band_sel, crops):
    """``_region_sources`` and ``_region_crops``: (S, C2, C1, h, w, band, crops as int32 (B, 5), the batch maximum (Hm, Wm))."""
    S, C2, C1, h, w, band = _region_sources(what, s2, s1, boundary, band_sel)
    return (S, C2, C1, h, w, band) + _region_crops(what, crops, S, h, w)


def _region_orbit(what, s1, s1_asc, orbit, B):
    """The orbit arguments ``region_gather`` and ``region_batch`` share: s1_asc shaped like s1 on its device, orbit = B host values in
    {0, 1}, an ascending crop only with s1_asc.  Returns the list as a ctypes uint8 pointer (None: all descending)."""
    if s1_asc is not None:
        L.require_device(s1_asc)
        if s1_asc.dtype != torch.float32 or s1_asc.shape != s1.shape or not s1_asc.is_contiguous() or s1_asc.device != s1.device:
            raise ValueError(f"{what}: s1_asc must be a contiguous fp32 tensor shaped like s1 {tuple(s1.shape)} on its device, got "
                             f"{s1_asc.dtype} {tuple(s1_asc.shape)}")
    if orbit is None:
        return None
    ob = np.ascontiguousarray(np.asarray(orbit.cpu() if torch.is_tensor(orbit) else orbit, dtype=np.int64).reshape(-1))
    if ob.size != B or ((ob != 0) & (ob != 1)).any() or (ob.any() and s1_asc is None):
        raise ValueError(f"{what}: orbit holds one value in {{0, 1}} per crop ({B}), and 1 (ascending) needs s1_asc; got {ob.tolist()}")
    ob8 = ob.astype(np.uint8)
    ptr = ob8.ctypes.data_as(C.POINTER(C.c_uint8))
    ptr._keep = ob8
    return ptr


def _region_crop_orbit(what, s1, s1_asc, orbit):
    """The orbit of ONE crop (``region_window``, ``region_item``): 0 = s1, 1 = s1_asc, which is shaped like s1 on its device."""
    _region_orbit(what, s1, s1_asc, None, 1)
    if isinstance(orbit, bool) or orbit not in (0, 1) or (orbit == 1 and s1_asc is None):
        raise ValueError(f"{what}: orbit is 0 (s1) or 1 (s1_asc, which must then be given), got {orbit!r}")
    return int(orbit)


def _region_norm(what, mean6, std6):
    """The six means and standard deviations of ``region_window`` / ``region_item`` as ctypes float[6] arrays."""
    mean = [float(v) for v in mean6]
    std = [float(v) for v in std6]
    if len(mean) != 6 or len(std) != 6:
        raise ValueError(f"{what}: mean6 and std6 hold six values each, got {len(mean)} and {len(std)}")
    return (C.c_float * 6)(*mean), (C.c_float * 6)(*std)


def _region_table(what, table, sites, device):
    """The slice of a patch table ``region_window`` / ``region_item`` take: table = (idx int32 (N,), val fp32 (N,), start, count) or None,
    sites = the crop's 6 * hc * wc.  Returns (idx, val, cap, start, count), idx and val None for a slice without entries."""
    idx = val = None
    cap = start = count = 0
    if table is not None:
        idx, val, start, count = table
        start, count = int(start), int(count)
        if count > 0 or idx is not None:
            if idx is None or val is None:
                raise ValueError(f"{what}: a slice of {count} entries needs the tables idx and val")
            L.require_device(idx, val)
            if (idx.dtype != torch.int32 or val.dtype != torch.float32 or idx.dim() != 1 or idx.shape != val.shape or
                    not idx.is_contiguous() or not val.is_contiguous() or idx.device != device or val.device != device):
                raise ValueError(f"{what}: idx int32 (N,) and val fp32 (N,), contiguous, on the rasters' device")
            cap = idx.numel()
        if start < 0 or count < 0 or start + count > cap or count > sites:
            raise ValueError(f"{what}: the slice [{start}, {start} + {count}) lies outside the table of {cap} entries or exceeds the "
                             f"{what.rsplit('_', 1)[-1]}'s {sites} sites")
    if count == 0:
        idx = val = None
    return idx, val, cap, start, count


def _region_layer(what, buildings, h, w, device):
    """The building layer of a ``region_*`` wrapper: a contiguous fp32 (h, w) raster on the rasters' device (no season axis), or None."""
    if buildings is None:
        return None
    L.require_device(buildings)
    if (buildings.dtype != torch.float32 or tuple(buildings.shape) != (h, w) or not buildings.is_contiguous() or
            buildings.device != device):
        raise ValueError(f"{what}: buildings must be a contiguous fp32 ({h}, {w}) raster on the rasters' device, got {buildings.dtype} "
                         f"{tuple(buildings.shape)}")
    return buildings


def _layer_out(what, t, shapes, device):
    """An ``out=`` slot for the building layer: a contiguous fp32 device tensor of one of ``shapes``."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) not in shapes or not t.is_contiguous() or \
            t.device != device:
        raise ValueError(f"{what}: the building_counts output must be a contiguous fp32 {shapes[0]} tensor on the rasters' device, got "
                         f"{None if not torch.is_tensor(t) else (t.dtype, tuple(t.shape))}")
    return t


def region_gather(s2, s1, boundary, band_sel, crops, out=None, s1_asc=None, orbit=None, buildings=None):
    """One batch of crops of resident rasters in ONE launch (csrc/region.hip, pc_region_gather): what the reference's weaksup items
    (data/PopulationDataset.py:403-458,566-568,624-649) and ``Population_Dataset_collate_fn`` (:885-958) assemble on the host.
    s2: device (S, C2, h, w) fp32 or uint16; s1: device fp32 (S, C1, h, w); boundary: device int32 (h, w); band_sel: six 0-based source
    bands, four of S2 then two of S1 (the reference's file bands (3, 2, 1, 4) / (1, 2) are (2, 1, 0, 3, 0, 1)); crops: HOST integers (B, 5)
    = {x0, x1, y0, y1, season}, rows [x0, x1) and columns [y0, y1).  Returns {"S2" (B, 4, Hm, Wm), "S1" (B, 2, Hm, Wm), "admin_mask" (B, Hm, Wm)
    = (float)id, "data_hw" int32 (B, 2)} at the batch maximum (Hm, Wm), padded 0 / 0 / -1 at the bottom and right; every element is written
    and fp32 sources are copied bit for bit.  out: such a dict to write into (its (Hm, Wm) may exceed the batch maximum).  An empty crop, one
    that leaves the raster and a season >= S raise before anything is enqueued.
    s1_asc / orbit (pc_region_gather_orbit): the ascending-orbit S1, shaped like s1, and B host values in {0, 1}: crop b takes its S1 from
    s1_asc where orbit[b] == 1.  Without them the same entry point is called with NULL for both, which IS pc_region_gather.
    buildings (pc_region_gather_layer): a resident fp32 (h, w) building layer; the result then carries "building_counts" (B, 1, Hm, Wm),
    the layer over each crop bit for bit, 0.0 outside it -- from the same launch.  An ``out`` dict must then hold that key as well."""
    S, C2, C1, h, w, band, cr32, Hm, Wm = _region_inputs("region_gather", s2, s1, boundary, band_sel, crops)
    B = cr32.shape[0]
    orb = _region_orbit("region_gather", s1, s1_asc, orbit, B)
    dev = s1.device
    buildings = _region_layer("region_gather", buildings, h, w, dev)
    if out is None:
        out = {"S2": torch.empty(B, 4, Hm, Wm, dtype=torch.float32, device=dev),
               "S1": torch.empty(B, 2, Hm, Wm, dtype=torch.float32, device=dev),
               "admin_mask": torch.empty(B, Hm, Wm, dtype=torch.float32, device=dev),
               "data_hw": torch.empty(B, 2, dtype=torch.int32, device=dev)}
        if buildings is not None:
            out["building_counts"] = torch.empty(B, 1, Hm, Wm, dtype=torch.float32, device=dev)
    else:
        L.require_device(out["S2"], out["S1"], out["admin_mask"], out["data_hw"])
        Ho, Wo = out["admin_mask"].shape[-2:]
        if buildings is not None:
            _layer_out("region_gather", out.get("building_counts"), ((B, 1, int(Ho), int(Wo)),), dev)
        if (tuple(out["S2"].shape) != (B, 4, Ho, Wo) or tuple(out["S1"].shape) != (B, 2, Ho, Wo) or
                tuple(out["admin_mask"].shape) != (B, Ho, Wo) or tuple(out["data_hw"].shape) != (B, 2) or Ho < Hm or Wo < Wm or
                any(out[k].dtype != torch.float32 or not out[k].is_contiguous() for k in ("S2", "S1", "admin_mask")) or
                out["data_hw"].dtype != torch.int32 or not out["data_hw"].is_contiguous()):
            raise ValueError(f"region_gather: out must hold contiguous fp32 S2 ({B}, 4, H, W), S1 ({B}, 2, H, W), admin_mask ({B}, H, W) with "
                             f"(H, W) >= ({Hm}, {Wm}) and int32 data_hw ({B}, 2)")
        Hm, Wm = int(Ho), int(Wo)
    if Hm * Wm >= 1 << 31:
        raise ValueError(f"region_gather: Hm * Wm < 2^31, got {Hm} x {Wm}")
    head = (L.ptr(s2), int(s2.dtype == torch.uint16), L.ptr(s1), L.ptr(s1_asc), orb, L.ptr(boundary))
    mid = (S, C2, C1, h, w, (C.c_int32 * 6)(*band), cr32.ctypes.data_as(C.POINTER(C.c_int32)), B, Hm, Wm, L.ptr(out["S2"]),
           L.ptr(out["S1"]), L.ptr(out["admin_mask"]))
    if buildings is None:
        L.check(L.lib().pc_region_gather_orbit(*head, *mid, L.ptr(out["data_hw"]), L.stream_ptr()), "pc_region_gather_orbit")
    else:
        L.check(L.lib().pc_region_gather_layer(*head, L.ptr(buildings), *mid, L.ptr(out["building_counts"]), L.ptr(out["data_hw"]),
                                               L.stream_ptr()), "pc_region_gather_layer")
    return out


def region_batch(s2, s1, boundary, band_sel, crops, params=None, hw=None, labels=None, out=None, s1_asc=None, orbit=None, buildings=None):
    """The batch a fused step takes, assembled from resident rasters in ONE launch (csrc/region_batch.hip, pc_region_batch).  By definition,
    bit for bit: ``augment_raw(*region_gather(...; tile (Hm, Wm)), params)`` -- without the intermediate S2 / S1 / admin_mask.
    s2, s1, boundary, band_sel, crops: as ``region_gather``.  params: ``draw_fused_params``' dict (None = no augmentation).  hw: the gathered
    tile (Hm, Wm), default and at least the batch maximum.  labels = (plan_cidx int64 (n, Kp), plan_y fp32 (n, Kp) -- device tables uploaded
    once --, items: B host integers, K): the same launch also writes census_idx[b] = plan_cidx[items[b], :K] and y likewise.
    Returns {"raw" (B, 6, Ho, Wo), "admin_mask" (B, Ho, Wo), ["census_idx" int64 (B, K), "y" fp32 (B, K)]} with (Ho, Wo) = (Wm, Hm) for an odd
    rotation; out: such a dict to write into.  Everything ``region_gather`` refuses, a rotation outside 0 .. 3, an item outside [0, n), a K
    outside [1, Kp] and an ``out`` of another shape raise ValueError before anything is enqueued.
    s1_asc / orbit: as ``region_gather`` takes them (pc_region_batch_orbit; NULL for both IS pc_region_batch).
    buildings (pc_region_batch_layer): a resident fp32 (h, w) building layer; the result then carries "building_counts" (B, 1, Ho, Wo) --
    by definition and bit for bit the layer of ``augment_raw(region_gather(..., buildings=), buildings=)``, from the same launch."""
    S, C2, C1, h, w, band, cr32, Hm, Wm = _region_inputs("region_batch", s2, s1, boundary, band_sel, crops)
    B = cr32.shape[0]
    orb = _region_orbit("region_batch", s1, s1_asc, orbit, B)
    if hw is not None:
        th, tw = int(hw[0]), int(hw[1])
        if th < Hm or tw < Wm:
            raise ValueError(f"region_batch: the tile hw = ({th}, {tw}) is smaller than the batch maximum ({Hm}, {Wm})")
        Hm, Wm = th, tw
    if Hm * Wm >= 1 << 31:
        raise ValueError(f"region_batch: Hm * Wm < 2^31, got {Hm} x {Wm}")
    pr = params or {}
    k = int(pr.get("rot", 0))
    if not 0 <= k <= 3:
        raise ValueError(f"region_batch: rot is a number of quarter turns in 0 .. 3, got {k}")
    Ho, Wo = (Wm, Hm) if k & 1 else (Hm, Wm)
    dev = s1.device
    buildings = _region_layer("region_batch", buildings, h, w, dev)
    lab = None
    if labels is not None:
        plan_cidx, plan_y, items, K = labels
        L.require_device(plan_cidx, plan_y)
        K = int(K)
        if (plan_cidx.dim() != 2 or plan_cidx.dtype != torch.int64 or plan_y.dtype != torch.float32 or plan_y.shape != plan_cidx.shape or
                not plan_cidx.is_contiguous() or not plan_y.is_contiguous() or plan_cidx.shape[0] < 1):
            raise ValueError("region_batch: labels are contiguous device tables plan_cidx int64 (n, Kp) and plan_y fp32 (n, Kp)")
        n, Kp = plan_cidx.shape
        it = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1))
        if it.size != B or (it < 0).any() or (it >= n).any():
            raise ValueError(f"region_batch: items names one plan row in [0, {n}) per crop ({B}), got {it.tolist()}")
        if not 1 <= K <= Kp:
            raise ValueError(f"region_batch: K in [1, {Kp}], got {K}")
        it32 = it.astype(np.int32)
    if out is None:
        out = {"raw": torch.empty(B, 6, Ho, Wo, dtype=torch.float32, device=dev),
               "admin_mask": torch.empty(B, Ho, Wo, dtype=torch.float32, device=dev)}
        if labels is not None:
            out["census_idx"] = torch.empty(B, K, dtype=torch.int64, device=dev)
            out["y"] = torch.empty(B, K, dtype=torch.float32, device=dev)
        if buildings is not None:
            out["building_counts"] = torch.empty(B, 1, Ho, Wo, dtype=torch.float32, device=dev)
    else:
        want = {"raw": ((B, 6, Ho, Wo), torch.float32), "admin_mask": ((B, Ho, Wo), torch.float32)}
        if buildings is not None:
            want["building_counts"] = ((B, 1, Ho, Wo), torch.float32)
        if labels is not None:
            want.update({"census_idx": ((B, K), torch.int64), "y": ((B, K), torch.float32)})
        for key, (shape, dt) in want.items():
            t = out.get(key)
            if t is None or not t.is_cuda or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"region_batch: out[{key!r}] must be a contiguous device {dt} tensor of shape {shape}, got "
                                 f"{None if t is None else (t.dtype, tuple(t.shape))}")
    if labels is not None:
        lab = L.PcRegionLabels(plan_cidx.data_ptr(), plan_y.data_ptr(), it32.ctypes.data_as(C.POINTER(C.c_int32)),
                               out["census_idx"].data_ptr(), out["y"].data_ptr(), n, Kp, K, 0)
    beta, gamma = pr.get("beta"), pr.get("gamma")
    head = (L.ptr(s2), int(s2.dtype == torch.uint16), L.ptr(s1), L.ptr(s1_asc), orb, L.ptr(boundary))
    mid = (S, C2, C1, h, w, (C.c_int32 * 6)(*band), cr32.ctypes.data_as(C.POINTER(C.c_int32)), B, Hm, Wm,
           int(bool(pr.get("vflip"))), int(bool(pr.get("hflip"))), k, int(beta is not None),
           C.c_float(beta if beta is not None else 1.0), int(gamma is not None),
           C.c_float(gamma if gamma is not None else 1.0), L.ptr(out["raw"]), L.ptr(out["admin_mask"]))
    tail = (Ho, Wo, C.byref(lab) if lab is not None else None, L.stream_ptr())
    if buildings is None:
        L.check(L.lib().pc_region_batch_orbit(*head, *mid, *tail), "pc_region_batch_orbit")
    else:
        L.check(L.lib().pc_region_batch_layer(*head, L.ptr(buildings), *mid, L.ptr(out["building_counts"]), *tail),
                "pc_region_batch_layer")
    return out


class AtlasHandle:
    """The C handle of a resident atlas (csrc/region_atlas.hip, pc_atlas_create): R regions = dicts of the device tensors s2, s1, boundary,
    optionally s1_asc and buildings, and band_sel.  One device, one S2 type, a building layer on all regions or on none: ValueError
    otherwise, before the library is called.  The descriptors are uploaded once, here: the only copy and the only synchronisation.  The
    handle keeps the tensors alive and frees the device table when it is collected."""

    def __init__(self, regions):
        regions = list(regions)
        if not 1 <= len(regions) <= L.PC_ATLAS_MAX_REGIONS:
            raise ValueError(f"atlas: 1 .. {L.PC_ATLAS_MAX_REGIONS} regions, got {len(regions)}")
        self.meta, keep = [], []
        desc = (L.PcAtlasRegion * len(regions))()
        dev, dt = regions[0]["s1"].device, regions[0]["s2"].dtype
        layered = regions[0].get("buildings") is not None
        for k, r in enumerate(regions):
            what = f"atlas region {k}"
            S, C2, C1, h, w, band = _region_sources(what, r["s2"], r["s1"], r["boundary"], r["band_sel"])
            asc, bld = r.get("s1_asc"), r.get("buildings")
            _region_orbit(what, r["s1"], asc, None, 1)
            _region_layer(what, bld, h, w, r["s1"].device)
            if r["s1"].device != dev or r["s2"].device != dev or r["boundary"].device != dev:
                raise ValueError(f"{what}: every region of an atlas lives on one device ({dev}), got {r['s1'].device}")
            if r["s2"].dtype != dt:
                raise ValueError(f"{what}: one S2 type per atlas ({dt}), got {r['s2'].dtype}: mixed S2 types are not part of it")
            if (bld is not None) != layered:
                raise ValueError(f"{what}: a building layer on all regions of an atlas or on none")
            d = desc[k]
            d.s2, d.s1, d.boundary = r["s2"].data_ptr(), r["s1"].data_ptr(), r["boundary"].data_ptr()
            d.s1_asc = 0 if asc is None else asc.data_ptr()
            d.layer = 0 if bld is None else bld.data_ptr()
            d.S, d.C2, d.C1, d.h, d.w = S, C2, C1, h, w
            d.band_sel[:] = band
            self.meta.append((S, h, w, asc is not None))
            keep.append((r["s2"], r["s1"], r["boundary"], asc, bld))
        self._keep = keep
        self.device, self.layered, self.R = dev, layered, len(regions)
        self._h = C.c_void_p()
        self._destroy = L.lib().pc_atlas_destroy
        with torch.cuda.device(dev):
            L.check(L.lib().pc_atlas_create(desc, self.R, int(dt == torch.uint16), C.byref(self._h)), "pc_atlas_create")

    def __del__(self):
        import sys
        h = getattr(self, "_h", None)
        if h is not None and h.value and not sys.is_finalizing():       # (at interpreter exit the runtime frees the table itself)
            self._destroy(h)
            self._h = None


def _atlas_inputs(what, atlas, region_of, crops, orbit):
    """The host lists of an ``atlas_*`` wrapper: region_of = B region indices, crops (B, 5) each checked in its OWN region, orbit = B values
    in {0, 1} with 1 only for a region that holds s1_asc.  Returns (region list, uint8 array, crops int32 (B, 5), (Hm, Wm), orbit pointer)."""
    if not isinstance(atlas, AtlasHandle):
        raise ValueError(f"{what}: an ops.AtlasHandle, got {type(atlas).__name__}")
    ro = np.ascontiguousarray(np.asarray(region_of.cpu() if torch.is_tensor(region_of) else region_of, dtype=np.int64).reshape(-1))
    if torch.is_tensor(crops):
        if crops.is_cuda:
            raise ValueError(f"{what}: crops is host data (it travels in the kernel arguments)")
        crops = crops.numpy()
    cr = np.ascontiguousarray(np.asarray(crops, dtype=np.int64).reshape(-1, 5))
    B = cr.shape[0]
    if B < 1 or ro.size != B or (ro < 0).any() or (ro >= atlas.R).any():
        raise ValueError(f"{what}: region_of names one region in [0, {atlas.R}) per crop ({B}), got {ro.tolist()}")
    ob = None
    if orbit is not None:
        ob = np.ascontiguousarray(np.asarray(orbit.cpu() if torch.is_tensor(orbit) else orbit, dtype=np.int64).reshape(-1))
        if ob.size != B or ((ob != 0) & (ob != 1)).any():
            raise ValueError(f"{what}: orbit holds one value in {{0, 1}} per crop ({B}), got {ob.tolist()}")
    for k in np.unique(ro).tolist():
        S, h, w, has_asc = atlas.meta[k]
        rows = np.flatnonzero(ro == k)
        try:
            _region_crops(what, cr[rows], S, h, w)
        except ValueError as e:
            raise ValueError(f"{e} (region {k} of the atlas; batch rows {rows.tolist()})") from None
        if ob is not None and ob[rows].any() and not has_asc:
            raise ValueError(f"{what}: orbit 1 (ascending) for a crop of region {k}, which holds no s1_asc")
    orb = None
    if ob is not None:
        ob8 = ob.astype(np.uint8)
        orb = ob8.ctypes.data_as(C.POINTER(C.c_uint8))
        orb._keep = ob8
    ro8 = ro.astype(np.uint8)
    return ro.tolist(), ro8, cr.astype(np.int32), (int((cr[:, 1] - cr[:, 0]).max()), int((cr[:, 3] - cr[:, 2]).max())), orb


def atlas_gather(atlas, region_of, crops, out=None, orbit=None):
    """``region_gather`` over a resident atlas in ONE launch (csrc/region_atlas.hip, pc_atlas_gather): crop b is crops[b] = {x0, x1, y0, y1,
    season} of region region_of[b].  By definition, bit for bit: row b equals row 0 of ``region_gather`` on that region alone with crop b,
    orbit[b] and the tile (Hm, Wm).  Returns ``region_gather``'s dict ("building_counts" when the atlas has layers) plus "region", the host
    list of region indices.  A crop or season invalid in its own region, a region outside [0, R) and orbit 1 for a region without s1_asc
    raise ValueError before anything is enqueued."""
    regions, ro8, cr32, (Hm, Wm), orb = _atlas_inputs("atlas_gather", atlas, region_of, crops, orbit)
    B, dev = cr32.shape[0], atlas.device
    if out is None:
        out = {"S2": torch.empty(B, 4, Hm, Wm, dtype=torch.float32, device=dev),
               "S1": torch.empty(B, 2, Hm, Wm, dtype=torch.float32, device=dev),
               "admin_mask": torch.empty(B, Hm, Wm, dtype=torch.float32, device=dev),
               "data_hw": torch.empty(B, 2, dtype=torch.int32, device=dev)}
        if atlas.layered:
            out["building_counts"] = torch.empty(B, 1, Hm, Wm, dtype=torch.float32, device=dev)
    else:
        L.require_device(out["S2"], out["S1"], out["admin_mask"], out["data_hw"])
        Ho, Wo = out["admin_mask"].shape[-2:]
        if atlas.layered:
            _layer_out("atlas_gather", out.get("building_counts"), ((B, 1, int(Ho), int(Wo)),), dev)
        if (tuple(out["S2"].shape) != (B, 4, Ho, Wo) or tuple(out["S1"].shape) != (B, 2, Ho, Wo) or
                tuple(out["admin_mask"].shape) != (B, Ho, Wo) or tuple(out["data_hw"].shape) != (B, 2) or Ho < Hm or Wo < Wm or
                any(out[k].dtype != torch.float32 or not out[k].is_contiguous() for k in ("S2", "S1", "admin_mask")) or
                out["data_hw"].dtype != torch.int32 or not out["data_hw"].is_contiguous()):
            raise ValueError(f"atlas_gather: out must hold contiguous fp32 S2 ({B}, 4, H, W), S1 ({B}, 2, H, W), admin_mask ({B}, H, W) with "
                             f"(H, W) >= ({Hm}, {Wm}) and int32 data_hw ({B}, 2)")
        Hm, Wm = int(Ho), int(Wo)
    if Hm * Wm >= 1 << 31:
        raise ValueError(f"atlas_gather: Hm * Wm < 2^31, got {Hm} x {Wm}")
    L.check(L.lib().pc_atlas_gather(atlas._h, ro8.ctypes.data_as(C.POINTER(C.c_uint8)), cr32.ctypes.data_as(C.POINTER(C.c_int32)), orb, B,
                                    Hm, Wm, L.ptr(out["S2"]), L.ptr(out["S1"]), L.ptr(out["admin_mask"]),
                                    L.ptr(out["building_counts"]) if atlas.layered else None, L.ptr(out["data_hw"]), L.stream_ptr()),
            "pc_atlas_gather")
    out["region"] = regions
    return out


def atlas_batch(atlas, region_of, crops, params=None, hw=None, labels=None, out=None, orbit=None):
    """``region_batch`` over a resident atlas in ONE launch (csrc/region_atlas.hip, pc_atlas_batch).  By definition, bit for bit:
    ``augment_raw(*atlas_gather(...; tile (Hm, Wm)), params)``.  params, hw, labels and out as ``region_batch`` takes them; the items of
    labels index ONE plan table, the regions' tables concatenated.  Returns ``region_batch``'s dict plus "region".  Everything
    ``atlas_gather`` and ``region_batch`` refuse raises ValueError before anything is enqueued."""
    regions, ro8, cr32, (Hm, Wm), orb = _atlas_inputs("atlas_batch", atlas, region_of, crops, orbit)
    B, dev = cr32.shape[0], atlas.device
    if hw is not None:
        th, tw = int(hw[0]), int(hw[1])
        if th < Hm or tw < Wm:
            raise ValueError(f"atlas_batch: the tile hw = ({th}, {tw}) is smaller than the batch maximum ({Hm}, {Wm})")
        Hm, Wm = th, tw
    if Hm * Wm >= 1 << 31:
        raise ValueError(f"atlas_batch: Hm * Wm < 2^31, got {Hm} x {Wm}")
    pr = params or {}
    k = int(pr.get("rot", 0))
    if not 0 <= k <= 3:
        raise ValueError(f"atlas_batch: rot is a number of quarter turns in 0 .. 3, got {k}")
    Ho, Wo = (Wm, Hm) if k & 1 else (Hm, Wm)
    lab = None
    if labels is not None:
        plan_cidx, plan_y, items, K = labels
        L.require_device(plan_cidx, plan_y)
        K = int(K)
        if (plan_cidx.dim() != 2 or plan_cidx.dtype != torch.int64 or plan_y.dtype != torch.float32 or plan_y.shape != plan_cidx.shape or
                not plan_cidx.is_contiguous() or not plan_y.is_contiguous() or plan_cidx.shape[0] < 1):
            raise ValueError("atlas_batch: labels are contiguous device tables plan_cidx int64 (n, Kp) and plan_y fp32 (n, Kp)")
        n, Kp = plan_cidx.shape
        it = np.ascontiguousarray(np.asarray(items, dtype=np.int64).reshape(-1))
        if it.size != B or (it < 0).any() or (it >= n).any():
            raise ValueError(f"atlas_batch: items names one plan row in [0, {n}) per crop ({B}), got {it.tolist()}")
        if not 1 <= K <= Kp:
            raise ValueError(f"atlas_batch: K in [1, {Kp}], got {K}")
        it32 = it.astype(np.int32)
    want = {"raw": ((B, 6, Ho, Wo), torch.float32), "admin_mask": ((B, Ho, Wo), torch.float32)}
    if atlas.layered:
        want["building_counts"] = ((B, 1, Ho, Wo), torch.float32)
    if labels is not None:
        want.update({"census_idx": ((B, K), torch.int64), "y": ((B, K), torch.float32)})
    if out is None:
        out = {key: torch.empty(*shape, dtype=dt, device=dev) for key, (shape, dt) in want.items()}
    else:
        for key, (shape, dt) in want.items():
            t = out.get(key)
            if t is None or not t.is_cuda or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ValueError(f"atlas_batch: out[{key!r}] must be a contiguous device {dt} tensor of shape {shape}, got "
                                 f"{None if t is None else (t.dtype, tuple(t.shape))}")
    if labels is not None:
        lab = L.PcRegionLabels(plan_cidx.data_ptr(), plan_y.data_ptr(), it32.ctypes.data_as(C.POINTER(C.c_int32)),
                               out["census_idx"].data_ptr(), out["y"].data_ptr(), n, Kp, K, 0)
    beta, gamma = pr.get("beta"), pr.get("gamma")
    L.check(L.lib().pc_atlas_batch(atlas._h, ro8.ctypes.data_as(C.POINTER(C.c_uint8)), cr32.ctypes.data_as(C.POINTER(C.c_int32)), orb, B,
                                   Hm, Wm, int(bool(pr.get("vflip"))), int(bool(pr.get("hflip"))), k, int(beta is not None),
                                   C.c_float(beta if beta is not None else 1.0), int(gamma is not None),
                                   C.c_float(gamma if gamma is not None else 1.0), L.ptr(out["raw"]), L.ptr(out["admin_mask"]),
                                   L.ptr(out["building_counts"]) if atlas.layered else None, Ho, Wo,
                                   C.byref(lab) if lab is not None else None, L.stream_ptr()), "pc_atlas_batch")
    out["region"] = regions
    return out


def region_nan_census(s2, s1, boundary, band_sel, boxes, s1_asc=None, max_blocks=0):
    """The NaN entries of many boxes of the resident rasters in ONE pass (csrc/region_repair.hip, pc_region_nan_census): what decides an
    item's S1 orbit (data/PopulationDataset.py:419-441), for a whole plan at once.  Sources and band_sel as ``region_gather``; boxes: HOST
    integers (n, 5) = {x0, x1, y0, y1, season}, validated here and uploaded once.  Returns a device int64 (n, 3) = {S2 over its four
    selected bands (a band listed twice counts twice; 0 for uint16 S2), descending S1 over its two, ascending S1 likewise (0 without
    s1_asc)}.  Integer adds only: the same bits for any launch geometry; max_blocks > 0 caps the workgroups of the pass (tests)."""
    S, C2, C1, h, w, band, bx32, Hm, _ = _region_inputs("region_nan_census", s2, s1, boundary, band_sel, boxes)
    _region_orbit("region_nan_census", s1, s1_asc, None, bx32.shape[0])
    n = bx32.shape[0]
    if 5 * n >= 1 << 31 or w >= 1 << 29:
        raise ValueError(f"region_nan_census: 5 * n < 2^31 and w < 2^29, got n {n}, w {w}")
    dev = s1.device
    boxes_dev = torch.from_numpy(bx32).to(dev)                       # the one upload
    counts = torch.empty(n, 3, dtype=torch.int64, device=dev)
    L.check(L.lib().pc_region_nan_census(L.ptr(s2), int(s2.dtype == torch.uint16), L.ptr(s1), L.ptr(s1_asc), S, C2, C1, h, w,
                                         (C.c_int32 * 6)(*band), L.ptr(boxes_dev), n, Hm, L.ptr(counts), int(max_blocks), L.stream_ptr()),
            "pc_region_nan_census")
    return counts


def region_patch_extract(gathered, filled):
    """The sparse difference of a gathered batch and its filled copy (pc_region_patch_count / pc_region_patch_write): gathered = what
    ``region_gather`` returned, filled = {"S2", "S1"} of the same shapes after ``nan_fill_`` over ``gathered["data_hw"]``.  Returns (idx
    int32 device (N,), val fp32 device (N,), counts: host int64 (B,)): per item b, in order, the entries (c * h_b + i) * w_b + j of its own
    (6, h_b, w_b) space (c = 0 .. 3: S2, 4 .. 5: S1) whose 32-bit pattern differs, ascending, with the filled tile's bits.  Comparing bit
    patterns covers the fill's "fewer than 4 known entries -> zeros" case without a rule of its own.  ONE synchronisation (the counts come to
    the host for the exclusive prefix): this is build-time work.  Raises MemoryError with the byte count before it allocates a table that
    does not fit the device's free memory."""
    g2, g1, hw = gathered["S2"], gathered["S1"], gathered["data_hw"]
    f2, f1 = filled["S2"], filled["S1"]
    L.require_device(g2, g1, f2, f1, hw)
    B, _, Hm, Wm = g2.shape
    if (tuple(g2.shape) != (B, 4, Hm, Wm) or tuple(g1.shape) != (B, 2, Hm, Wm) or f2.shape != g2.shape or f1.shape != g1.shape or
            tuple(hw.shape) != (B, 2) or hw.dtype != torch.int32 or not hw.is_contiguous() or
            any(t.dtype != torch.float32 or not t.is_contiguous() for t in (g2, g1, f2, f1))):
        raise ValueError("region_patch_extract: contiguous fp32 S2 (B, 4, H, W) / S1 (B, 2, H, W) pairs of equal shapes and int32 data_hw (B, 2)")
    if B < 1 or B > 65535 or 6 * Hm * Wm >= 1 << 31:
        raise ValueError(f"region_patch_extract: 1 <= B <= 65535 and 6 * Hm * Wm < 2^31, got B {B}, tile {Hm} x {Wm}")
    dev = g2.device
    nchunk = -(-6 * Hm * Wm // L.PC_REGION_PATCH_CHUNK)
    counts = torch.empty(B, nchunk, dtype=torch.int32, device=dev)
    L.check(L.lib().pc_region_patch_count(L.ptr(g2), L.ptr(f2), L.ptr(g1), L.ptr(f1), L.ptr(hw), B, Hm, Wm, L.ptr(counts), nchunk,
                                          L.stream_ptr()), "pc_region_patch_count")
    host = counts.cpu().to(torch.int64)                              # the one synchronisation
    per_item = host.sum(1)
    total = int(per_item.sum())
    if total == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev), per_item)
    free, _ = torch.cuda.mem_get_info(dev)
    if 8 * total > free:
        raise MemoryError(f"region_patch_extract: the patch table takes {8 * total} bytes ({total} entries), device {dev} has {free} free")
    flat = host.reshape(-1)
    chunk_off = (torch.cumsum(flat, 0) - flat).to(dev)               # the exclusive prefix
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    val = torch.empty(total, dtype=torch.float32, device=dev)
    L.check(L.lib().pc_region_patch_write(L.ptr(g2), L.ptr(f2), L.ptr(g1), L.ptr(f1), L.ptr(hw), B, Hm, Wm, L.ptr(chunk_off), nchunk,
                                          L.ptr(idx), L.ptr(val), C.c_int64(total), L.stream_ptr()), "pc_region_patch_write")
    return idx, val, per_item


def region_patch_apply(idx, val, off, count, item_hw, s2, s1, hw, params=None):
    """Lay the patches of a batch over it (pc_region_patch_apply), on the current stream, without synchronisation.  idx / val: the device
    tables; off / count / item_hw: HOST, per batch item its range in the tables and its extent (h_b, w_b).  Targets: s2 = the batch's S2
    planes and s1 = its S1 planes -- two views of one raw tile (``raw[:, :4]``, ``raw[:, 4:]``) or the separate contiguous S2 / S1 of the
    unfused feed -- whose item stride may exceed the planes they span.  hw = the gathered tile (Hm, Wm) the batch was assembled at; params:
    the coins it was assembled with (None = none): an entry lands at the image of its tile position under the flips and quarter turns and
    S2 values pass through the same brightness / gamma as the pixels they replace.  Returns the number of entries applied (0: no launch)."""
    B = len(count)
    total = int(sum(int(c) for c in count))
    if total == 0:
        return 0
    L.require_device(idx, val, s2, s1)
    Hm, Wm = int(hw[0]), int(hw[1])
    pr = params or {}
    k = int(pr.get("rot", 0))
    if not 0 <= k <= 3:
        raise ValueError(f"region_patch_apply: rot is a number of quarter turns in 0 .. 3, got {k}")
    Ho, Wo = (Wm, Hm) if k & 1 else (Hm, Wm)
    if (idx.dtype != torch.int32 or val.dtype != torch.float32 or idx.dim() != 1 or idx.shape != val.shape or not idx.is_contiguous() or
            not val.is_contiguous()):
        raise ValueError("region_patch_apply: idx int32 (N,) and val fp32 (N,), contiguous")
    for t, ch, name in ((s2, 4, "s2"), (s1, 2, "s1")):
        if (t.dtype != torch.float32 or tuple(t.shape) != (B, ch, Ho, Wo) or t.stride()[1:] != (Ho * Wo, Wo, 1) or
                (B > 1 and t.stride(0) < ch * Ho * Wo)):
            raise ValueError(f"region_patch_apply: {name} must be fp32 ({B}, {ch}, {Ho}, {Wo}) with dense planes, got {t.dtype} "
                             f"{tuple(t.shape)} strides {t.stride()}")
    offs = np.ascontiguousarray(np.asarray(off, dtype=np.int64).reshape(-1))
    cnt = np.ascontiguousarray(np.asarray(count, dtype=np.int64).reshape(-1))
    ihw = np.ascontiguousarray(np.asarray(item_hw, dtype=np.int64).reshape(-1, 2))
    N = idx.numel()
    live = cnt > 0
    if (offs.size != B or ihw.shape[0] != B or (cnt < 0).any() or (offs < 0).any() or (offs + cnt > N).any() or
            (live & ((ihw[:, 0] < 1) | (ihw[:, 1] < 1) | (ihw[:, 0] > Hm) | (ihw[:, 1] > Wm))).any()):
        raise ValueError(f"region_patch_apply: every item's range inside the table of {N} entries and its extent inside the {Hm} x {Wm} tile")
    cnt32, ihw32 = cnt.astype(np.int32), ihw.astype(np.int32)
    beta, gamma = pr.get("beta"), pr.get("gamma")
    st2 = s2.stride(0) if B > 1 else 4 * Ho * Wo
    st1 = s1.stride(0) if B > 1 else 2 * Ho * Wo
    L.check(L.lib().pc_region_patch_apply(L.ptr(idx), L.ptr(val), C.c_int64(N), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                                          cnt32.ctypes.data_as(C.POINTER(C.c_int32)), ihw32.ctypes.data_as(C.POINTER(C.c_int32)), B,
                                          L.ptr(s2), C.c_int64(st2), L.ptr(s1), C.c_int64(st1), Hm, Wm, Ho, Wo,
                                          int(bool(pr.get("vflip"))), int(bool(pr.get("hflip"))), k, int(beta is not None),
                                          C.c_float(beta if beta is not None else 1.0), int(gamma is not None),
                                          C.c_float(gamma if gamma is not None else 1.0), L.stream_ptr()), "pc_region_patch_apply")
    return total


def region_window_rows(ps):
    """Rows of one channel a workgroup of ``region_window`` owns at window side ps (pc_region_window_rows; 0 for a ps it refuses)."""
    return int(L.lib().pc_region_window_rows(int(ps)))


def region_window(s2, s1, band_sel, window, ps, mean6, std6, out=None, s1_asc=None, orbit=0, table=None, buildings=None,
                  buildings_out=None):
    """The normalised model input (1, 6, ps, ps) of ONE evaluation window of resident rasters in ONE launch (csrc/region_crop.hip,
    pc_region_window), channels [S2 R G B NIR | S1 VV VH]: out = (v - mean6[c]) / std6[c] with ``select_normalize``'s fp32 division.
    s2, s1, band_sel: as ``region_gather``; window: HOST integers (x, y, season) = row origin, column origin, season; orbit: 0 = s1,
    1 = s1_asc (shaped like s1).  table = (idx int32 (N,), val fp32 (N,), start, count): the slice [start, start + count) of a patch table as
    ``region_patch_extract`` writes it -- ascending, idx = (c * ps + i) * ps + j in the window's own (6, ps, ps) space, val the raw repaired
    value, which replaces the raster's value BEFORE the normalisation.  Every element of out is stored exactly once; no synchronisation.
    out: a contiguous fp32 device (1, 6, ps, ps) or (6, ps, ps) tensor to write into.  A window that leaves the raster, a season >= S, a ps
    outside [1, PC_REGION_WINDOW_MAX_PS], a band outside its source, an orbit outside {0, 1} or 1 without s1_asc and a slice outside the
    tables raise ValueError before anything is enqueued.
    buildings (pc_region_window_layer): a resident fp32 (h, w) building layer; the same launch then also copies its slice over the window,
    bit for bit, and the result is the tuple (out, building_counts (1, 1, ps, ps)).  buildings_out: such a tensor (or (ps, ps)) to write
    into."""
    what = "region_window"
    S, C2, C1, h, w, band = _region_sources(what, s2, s1, None, band_sel)
    buildings = _region_layer(what, buildings, h, w, s1.device)
    if buildings is None and buildings_out is not None:
        raise ValueError(f"{what}: buildings_out without buildings")
    orbit = _region_crop_orbit(what, s1, s1_asc, orbit)
    ps = int(ps)
    if not 1 <= ps <= L.PC_REGION_WINDOW_MAX_PS:
        raise ValueError(f"{what}: ps in [1, {L.PC_REGION_WINDOW_MAX_PS}], got {ps}")
    win = [int(v) for v in (window.tolist() if torch.is_tensor(window) else window)]
    if len(win) != 3:
        raise ValueError(f"{what}: window = (x, y, season), got {win}")
    x, y, season = win
    if x < 0 or y < 0 or x + ps > h or y + ps > w or not 0 <= season < S:
        raise ValueError(f"{what}: window {tuple(win)} of side {ps} leaves the {h} x {w} raster or names a season outside [0, {S})")
    mean, std = _region_norm(what, mean6, std6)
    idx, val, cap, start, count = _region_table(what, table, 6 * ps * ps, s1.device)
    if out is None:
        out = torch.empty(1, 6, ps, ps, dtype=torch.float32, device=s1.device)
    else:
        L.require_device(out)
        if (out.dtype != torch.float32 or tuple(out.shape) not in ((1, 6, ps, ps), (6, ps, ps)) or not out.is_contiguous() or
                out.device != s1.device):
            raise ValueError(f"{what}: out must be a contiguous fp32 (1, 6, {ps}, {ps}) tensor on the rasters' device, got {out.dtype} "
                             f"{tuple(out.shape)}")
    head = (L.ptr(s2), int(s2.dtype == torch.uint16), L.ptr(s1), L.ptr(s1_asc), orbit)
    mid = (S, C2, C1, h, w, (C.c_int32 * 6)(*band), x, y, season, ps, mean, std, L.ptr(idx), L.ptr(val), C.c_int64(cap), C.c_int64(start),
           C.c_int64(count), L.ptr(out))
    if buildings is None:
        L.check(L.lib().pc_region_window(*head, *mid, L.stream_ptr()), "pc_region_window")
        return out
    if buildings_out is None:
        buildings_out = torch.empty(1, 1, ps, ps, dtype=torch.float32, device=s1.device)
    else:
        _layer_out(what, buildings_out, ((1, 1, ps, ps), (ps, ps)), s1.device)
    L.check(L.lib().pc_region_window_layer(*head, L.ptr(buildings), *mid, L.ptr(buildings_out), L.stream_ptr()), "pc_region_window_layer")
    return out, buildings_out.view(1, 1, ps, ps)


def region_item(s2, s1, boundary, band_sel, crop, mean6, std6, out=None, admin_out=None, s1_asc=None, orbit=0, table=None, buildings=None,
                buildings_out=None):
    """The normalised model input (1, 6, hc, wc) AND the admin mask (1, hc, wc) of ONE rectangular crop of resident rasters in ONE launch
    (csrc/region_crop.hip, pc_region_item) -- a validation item: input = (v - mean6[c]) / std6[c] with ``select_normalize``'s fp32
    division, channels [S2 R G B NIR | S1 VV VH]; admin_mask = (float)boundary over the crop.
    s2, s1, boundary, band_sel: as ``region_gather``; crop: HOST integers (x0, x1, y0, y1, season), rows [x0, x1) and columns [y0, y1);
    orbit: 0 = s1, 1 = s1_asc (shaped like s1).  table = (idx int32 (N,), val fp32 (N,), start, count): the slice [start, start + count) of
    a patch table as ``region_patch_extract`` writes it -- ascending, idx = (c * hc + i) * wc + j in the item's own (6, hc, wc) space, val the
    raw repaired value, which replaces the raster's value BEFORE the normalisation.  Every element of both outputs is stored exactly once;
    no synchronisation; no cap on a side (6 * hc * wc < 2^31).  out / admin_out: contiguous fp32 device tensors (1, 6, hc, wc) or
    (6, hc, wc) / (1, hc, wc) or (hc, wc) to write into.  Returns (input, admin_mask).  An empty crop, one that leaves the raster, a season
    >= S, a band outside its source, an orbit outside {0, 1} or 1 without s1_asc and a slice outside the tables raise ValueError before
    anything is enqueued.
    buildings (pc_region_item_layer): a resident fp32 (h, w) building layer; the same launch then also copies its slice over the crop, bit
    for bit, and the result is (input, admin_mask, building_counts (1, 1, hc, wc)).  buildings_out: such a tensor (or (hc, wc)) to write
    into."""
    what = "region_item"
    cr = [int(v) for v in (crop.tolist() if torch.is_tensor(crop) or isinstance(crop, np.ndarray) else crop)]
    if len(cr) != 5:
        raise ValueError(f"{what}: crop = (x0, x1, y0, y1, season), got {cr}")
    S, C2, C1, h, w, band, _, hc, wc = _region_inputs(what, s2, s1, boundary, band_sel, [cr])
    orbit = _region_crop_orbit(what, s1, s1_asc, orbit)
    if 6 * hc * wc >= 1 << 31:
        raise ValueError(f"{what}: 6 * hc * wc < 2^31, got a crop of {hc} x {wc}")
    mean, std = _region_norm(what, mean6, std6)
    idx, val, cap, start, count = _region_table(what, table, 6 * hc * wc, s1.device)
    dev = s1.device
    buildings = _region_layer(what, buildings, h, w, dev)
    if buildings is None and buildings_out is not None:
        raise ValueError(f"{what}: buildings_out without buildings")
    if out is None:
        out = torch.empty(1, 6, hc, wc, dtype=torch.float32, device=dev)
    if admin_out is None:
        admin_out = torch.empty(1, hc, wc, dtype=torch.float32, device=dev)
    L.require_device(out, admin_out)
    for t, shapes, name in ((out, ((1, 6, hc, wc), (6, hc, wc)), "out"), (admin_out, ((1, hc, wc), (hc, wc)), "admin_out")):
        if t.dtype != torch.float32 or tuple(t.shape) not in shapes or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: {name} must be a contiguous fp32 {shapes[0]} tensor on the rasters' device, got {t.dtype} "
                             f"{tuple(t.shape)}")
    head = (L.ptr(s2), int(s2.dtype == torch.uint16), L.ptr(s1), L.ptr(s1_asc), orbit, L.ptr(boundary))
    mid = (S, C2, C1, h, w, (C.c_int32 * 6)(*band), cr[0], cr[1], cr[2], cr[3], cr[4], mean, std, L.ptr(idx), L.ptr(val), C.c_int64(cap),
           C.c_int64(start), C.c_int64(count), L.ptr(out), L.ptr(admin_out))
    res = (out if out.dim() == 4 else out.view(1, 6, hc, wc), admin_out if admin_out.dim() == 3 else admin_out.view(1, hc, wc))
    if buildings is None:
        L.check(L.lib().pc_region_item(*head, *mid, L.stream_ptr()), "pc_region_item")
        return res
    if buildings_out is None:
        buildings_out = torch.empty(1, 1, hc, wc, dtype=torch.float32, device=dev)
    else:
        _layer_out(what, buildings_out, ((1, 1, hc, wc), (hc, wc)), dev)
    L.check(L.lib().pc_region_item_layer(*head, L.ptr(buildings), *mid, L.ptr(buildings_out), L.stream_ptr()), "pc_region_item_layer")
    return res + (buildings_out.view(1, 1, hc, wc),)


def nan_fill_(x, hw=None, count_only=False):
    """Nearest-value NaN fill in place (data/PopulationDataset.py:526-551 interpolate_nan, pc_nan_fill): x = contiguous fp32 device tensor
    (B, C, H, W) or (C, H, W), each sample's (C, h, w) array filled on its own -- every NaN takes the value of the nearest known entry in
    3-D index space (c, i, j), ties to the smallest channel, then row, then column; fewer than 4 known entries zero the array.
    hw: per-sample extents (h_b, w_b) anchored top-left (the collate's ``data_hw``; entries outside are neither sources nor targets), a
    (B, 2) integer tensor on the host or the device, or a list of pairs; None = the whole H x W.  count_only: count, do not fill.
    Returns the per-sample (nan_count, known_count) as a device int64 tensor, (B, 2) -- or (2,) for a (C, H, W) input."""
    L.require_device(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() not in (3, 4):
        raise ValueError(f"nan_fill_: a contiguous fp32 (B, C, H, W) or (C, H, W) tensor, got {x.dtype} {tuple(x.shape)}")
    xb = x.unsqueeze(0) if x.dim() == 3 else x
    B, Cc, H, W = xb.shape
    if Cc > L.PC_NAN_FILL_MAX_C or H > L.PC_NAN_FILL_MAX_HW or W > L.PC_NAN_FILL_MAX_HW:
        raise ValueError(f"nan_fill_: at most {L.PC_NAN_FILL_MAX_C} channels and {L.PC_NAN_FILL_MAX_HW} rows / columns, got {tuple(x.shape)}")
    counts = torch.empty(B, 2, dtype=torch.int64, device=x.device)
    if xb.numel() == 0:
        counts.zero_()
        return counts if x.dim() == 4 else counts[0]
    hw_dev = None
    if hw is not None:
        if torch.is_tensor(hw) and hw.is_cuda:
            if tuple(hw.shape) != (B, 2):
                raise ValueError(f"nan_fill_: hw must be (B, 2), got {tuple(hw.shape)}")
            hw_dev = hw.to(torch.int32).contiguous()
        else:
            hw_host = torch.as_tensor(hw, dtype=torch.int64).reshape(-1, 2)
            if hw_host.shape[0] != B or bool((hw_host < 0).any()) or bool((hw_host[:, 0] > H).any()) or bool((hw_host[:, 1] > W).any()):
                raise ValueError(f"nan_fill_: extents {hw_host.tolist()} do not fit a batch of {B} x {H} x {W}")
            hw_dev = hw_host.to(torch.int32).to(x.device)
    ws = _workspace(L.lib().pc_nan_fill_ws_bytes(B, Cc, H, W), x.device)
    L.check(L.lib().pc_nan_fill(L.ptr(xb), L.ptr(hw_dev), L.ptr(counts), L.ptr(ws), B, Cc, H, W,
                                L.PC_NAN_FILL_COUNT_ONLY if count_only else 0, L.stream_ptr()), "pc_nan_fill")
    return counts if x.dim() == 4 else counts[0]


def input_grad(problems, out, pads):
    """Gradient w.r.t. the model input from the gradients at the first convolutions' outputs (pc_input_grad, csrc/input_grad.hip): the
    data gradient of each stream's first conv, folded back through the reflect padding and scattered through the channel gather -- ONE
    launch, no atomics, bit-reproducible.  problems = list (1 or 2) of dicts {g: (B, 8, Hp, Wp) gradient w.r.t. the conv output (planar
    fp32 with any strides, or channels-last bf16 in bf16 mode), w: the conv weight (8, Cin, 3, 3) fp32 with Cin = 2 or 4, chmap: the Cin
    channels of ``out`` the conv's input channels were gathered from}; out: contiguous fp32 (B, Cx, H, W), every element written (=);
    pads = (top, bottom, left, right) of the reflect padding, each smaller than the extent it mirrors.  The chmaps must cover the channels
    of ``out`` exactly once.  Returns out."""
    n = len(problems)
    L.require_device(out, *[t for pr in problems for t in (pr["g"], pr["w"])])
    if out.dim() != 4 or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"input_grad: out must be a contiguous fp32 (B, C, H, W) tensor, got {out.dtype} {tuple(out.shape)}")
    B, Cx, H, W = out.shape
    pt, pb, pl, pr_ = (int(v) for v in pads)
    keep = []
    descs = (L.PcInputGradDesc * max(n, 1))()
    for i, pr in enumerate(problems):
        w = pr["w"]
        if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or pr["g"].shape[0] != B:
            raise ValueError(f"input_grad: problem {i}: a contiguous fp32 (8, Cin, 3, 3) weight and a gradient of batch {B}")
        chmap = [int(c) for c in pr["chmap"]][:w.shape[1]]
        if len(chmap) != w.shape[1] or w.shape[1] > 4:
            raise ValueError(f"input_grad: problem {i}: chmap {pr['chmap']} does not name the {w.shape[1]} input channels of the weight")
        sg = L.src(pr["g"])
        keep.append(sg)
        descs[i].g = C.pointer(sg)
        descs[i].w = w.data_ptr()
        descs[i].cin = w.shape[1]
        for c, ch in enumerate(chmap):
            descs[i].chmap[c] = ch
    L.check(L.lib().pc_input_grad(n, descs, L.ptr(out), B, Cx, H, W, pt, pb, pl, pr_, L.stream_ptr()), "pc_input_grad")
    return out


def augment_raw(s2, s1, admin_mask, params, out=None, admin_out=None, buildings=None, buildings_out=None):
    """The trainer's augmentations (run_train.py:386-402) with parameters drawn on the host (utils/transform.py: draw_fused_params), applied
    while the raw 6-channel tile [S2 | S1] is assembled -- ONE launch (pc_augment_raw).  s2 (B, 4, H, W) digital numbers, s1 (B, 2, H, W),
    admin_mask (B, H, W), fp32 device tensors; returns (raw (B, 6, Ho, Wo), admin (B, Ho, Wo)); params None = no augmentation.
    buildings (pc_augment_raw_layer): a building layer (B, 1, H, W) fp32, moved under the admin mask's map in the same launch, bit for bit;
    the result is then (raw, admin, building_counts (B, 1, Ho, Wo)).  buildings_out: such a tensor to write into."""
    L.require_device(s2, s1, admin_mask)
    B, c2, H, W = s2.shape
    if buildings is not None:
        L.require_device(buildings)
        if buildings.dtype != torch.float32 or tuple(buildings.shape) != (B, 1, H, W) or not buildings.is_contiguous():
            raise ValueError(f"augment_raw: buildings must be a contiguous fp32 ({B}, 1, {H}, {W}) tensor, got {buildings.dtype} "
                             f"{tuple(buildings.shape)}")
    elif buildings_out is not None:
        raise ValueError("augment_raw: buildings_out without buildings")
    if c2 != 4 or tuple(s1.shape) != (B, 2, H, W) or tuple(admin_mask.shape) != (B, H, W):
        raise ValueError(f"augment_raw: S2 (B, 4, H, W), S1 (B, 2, H, W), admin_mask (B, H, W); got {tuple(s2.shape)}, {tuple(s1.shape)}, "
                         f"{tuple(admin_mask.shape)}")
    for t in (s2, s1, admin_mask):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("augment_raw: contiguous fp32 tensors")
    pr = params or {}
    k = int(pr.get("rot", 0)) & 3
    Ho, Wo = (W, H) if k & 1 else (H, W)
    if out is None:
        out = torch.empty(B, 6, Ho, Wo, device=s2.device, dtype=torch.float32)
    if admin_out is None:
        admin_out = torch.empty(B, Ho, Wo, device=s2.device, dtype=torch.float32)
    beta, gamma = pr.get("beta"), pr.get("gamma")
    tail = (B, H, W, int(bool(pr.get("vflip"))), int(bool(pr.get("hflip"))), k, int(beta is not None),
            C.c_float(beta if beta is not None else 1.0), int(gamma is not None), C.c_float(gamma if gamma is not None else 1.0),
            L.stream_ptr())
    if buildings is None:
        L.check(L.lib().pc_augment_raw(L.ptr(s2), L.ptr(s1), L.ptr(admin_mask), L.ptr(out), L.ptr(admin_out), *tail), "pc_augment_raw")
        return out, admin_out
    if buildings_out is None:
        buildings_out = torch.empty(B, 1, Ho, Wo, device=s2.device, dtype=torch.float32)
    else:
        _layer_out("augment_raw", buildings_out, ((B, 1, Ho, Wo),), s2.device)
    L.check(L.lib().pc_augment_raw_layer(L.ptr(s2), L.ptr(s1), L.ptr(admin_mask), L.ptr(buildings), L.ptr(out), L.ptr(admin_out),
                                         L.ptr(buildings_out), *tail), "pc_augment_raw_layer")
    return out, admin_out, buildings_out


def loss_fwd_bwd(popcount, y, stats, lam4, scale_regularization, lam_weak, inv_B, loss_out, g_popcount, g_scale_const):
    L.require_device(popcount, y)
    L.check(L.lib().pc_loss_fwd_bwd(L.ptr(popcount), L.ptr(y), L.ptr(stats), (C.c_float * 4)(*lam4),
                                    C.c_float(scale_regularization), C.c_float(lam_weak), C.c_float(inv_B),
                                    popcount.numel(), L.ptr(loss_out), L.ptr(g_popcount), L.ptr(g_scale_const),
                                    L.stream_ptr()), "pc_loss_fwd_bwd")


def head_popcount_loss(B, H, W, nsel_counts, y, lam4, scale_regularization, lam_weak, inv_B, popcount, stats, loss_out, g_popcount,
                       g_scale_const):
    """Finishes a ``head_fwd(..., defer_reduce=True)`` call -- popcount[B] and stats {Nsel, sum scale} from the per-chunk partials in the
    head workspace -- and computes the loss forward + backward (``loss_fwd_bwd``) in the same single-block launch."""
    L.require_device(y, popcount)
    ws = _workspace(L.lib().pc_head_ws_bytes(B, H, W), y.device)
    L.check(L.lib().pc_head_popcount_loss(L.ptr(ws), B, H, W, L.ptr(nsel_counts), L.ptr(y), (C.c_float * 4)(*lam4),
                                          C.c_float(scale_regularization), C.c_float(lam_weak), C.c_float(inv_B), L.ptr(popcount),
                                          L.ptr(stats), L.ptr(loss_out), L.ptr(g_popcount), L.ptr(g_scale_const), L.stream_ptr()),
            "pc_head_popcount_loss")


def adam_groups(segments, active):
    """pc_adam_groups from [(end_offset, group id), ...] (consecutive segments of the flat buffer) and the set of group
    ids that are updated in this call; the others are skipped like parameters whose .grad is None in torch.optim.Adam."""
    g = L.PcAdamGroups()
    assert 1 <= len(segments) <= L.PC_ADAM_MAX_SEG
    g.nseg = len(segments)
    for i, (end, grp) in enumerate(segments):
        assert 0 <= grp < L.PC_ADAM_GROUPS
        g.seg_end[i], g.seg_group[i] = int(end), int(grp)
    g.active_mask = sum(1 << int(a) for a in set(active))
    return g


def adam_clip_step_fused(p, g, m, v, n_decay, hyper, weight_decay, beta1, beta2, eps, max_norm, norm_out, step, groups=None):
    """grad-norm + clip + Adam in one launch (norm_out receives the total norm).  groups: ops.adam_groups(...) or None."""
    L.require_device(p, g, m, v, hyper, step)
    need = L.PC_ADAM_GROUPS if groups is not None else 1
    assert step.dtype == torch.int32 and step.numel() >= need, "step: one int32 counter per Adam group"
    L.check(L.lib().pc_adam_clip_step_fused(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), n_decay, L.ptr(hyper),
                                            C.c_float(weight_decay), C.c_float(beta1), C.c_float(beta2), C.c_float(eps),
                                            C.c_float(max_norm), L.ptr(norm_out), L.ptr(step),
                                            C.byref(groups) if groups is not None else None, L.stream_ptr()),
            "pc_adam_clip_step_fused")


# one reduction of WgradBatch.finish(): the fields of pc_wgrad_reduce_desc (partial: device address of the workspace slot; dw / db: the
# output tensors, db may be None; dw_offset: elements into dw where the entry's first column starts)
ReduceEntry = collections.namedtuple("ReduceEntry", "partial dw db nwg Cin Cout kind dw_co_stride dw_offset src_cin src_ci0",
                                     defaults=(0, 0, 0, 0))


class WgradBatch:
    """Collects the first-stage (per-workgroup partial) weight-gradient launches of a backward pass and finishes them
    with ONE batched reduction launch.  Each layer gets its own slice of a persistent workspace."""

    _ws = {}

    def __init__(self, device, accumulate=False):
        self.device = device
        self.accumulate = accumulate
        self.entries = []
        self.raw_entries = []           # (partials ptr, total ptr, nwg, floats): raw sums (kind 2)
        self.chains = []                # composed Up blocks: chain-rule launches that follow the reduction
        self.head = None                # HeadPartials of the pass's head_bwd(defer_reduce=True): finished by the same launch
        self.slot_bytes = int(max(L.lib().pc_conv3x3_wgrad_ws_bytes(32, 8), L.lib().pc_convt2x2_wgrad_ws_bytes(16)))
        self.slot = 0

    def _slice(self, nbytes=0):
        """One workspace slot (or as many consecutive slots as ``nbytes`` needs)."""
        k = max(1, -(-int(nbytes) // self.slot_bytes))
        key = str(self.device)
        need = (self.slot + k) * self.slot_bytes
        buf = WgradBatch._ws.get(key)
        if buf is None or buf.numel() < need:
            if buf is not None:
                _ws_retired.append(buf)       # earlier entries of this batch / captured graphs still point into it
            nbuf = torch.empty(max(need, 32 * self.slot_bytes), dtype=torch.uint8, device=self.device)
            WgradBatch._ws[key] = buf = nbuf
        ptr_ = buf.data_ptr() + self.slot * self.slot_bytes
        self.slot += k
        return ptr_

    def conv3x3(self, a, g, cout, dw, db, b=None, a_mode=L.PC_SRC_DIRECT, a_pad=(0, 0), chmap=(0, 1, 2, 3),
                b_offset=(0, 0), a_channels=None):
        B, Cg, H, W = g.shape
        Ca = a.shape[1] if a_channels is None else a_channels
        Cb = 0 if b is None else b.shape[1]
        sa = L.src(a, C_=Ca, mode=a_mode, oy=a_pad[0], ox=a_pad[1], chmap=chmap)
        sb = L.src(b, oy=b_offset[0], ox=b_offset[1]) if b is not None else None
        sg = L.src(g)
        ws = self._slice()
        nwg = C.c_int(0)
        L.check(L.lib().pc_conv3x3_wgrad_partial(C.byref(sa), C.byref(sb) if sb is not None else None, C.byref(sg),
                                                 C.c_void_p(ws), B, H, W, Ca + Cb, cout, C.byref(nwg), L.stream_ptr()),
                "pc_conv3x3_wgrad_partial")
        self.entries.append(ReduceEntry(ws, dw, db, nwg.value, Ca + Cb, cout, 0))

    def conv3x3_group(self, problems, cout, a_mode=L.PC_SRC_DIRECT, a_pad=(0, 0), a_channels=None, cin_total=None):
        """problems: list of dicts {a, g, dw, db, b (opt), b_offset (opt), chmap (opt)} of identical geometry -> one launch.
        cin_total: dw is the gradient of a wider weight [cout][cin_total][3][3] whose FIRST Ca (+ Cb) input channels these are"""
        n = len(problems)
        g0, a0 = problems[0]["g"], problems[0]["a"]
        B, Cg, H, W = g0.shape
        Ca = a0.shape[1] if a_channels is None else a_channels
        Cb = 0 if problems[0].get("b") is None else problems[0]["b"].shape[1]
        keep, descs, slots = [], (L.PcConvWgradDesc * n)(), []
        for i, pr in enumerate(problems):
            sa = L.src(pr["a"], C_=Ca, mode=a_mode, oy=a_pad[0], ox=a_pad[1], chmap=pr.get("chmap", (0, 1, 2, 3)))
            bo = pr.get("b_offset", (0, 0))
            sb = L.src(pr["b"], oy=bo[0], ox=bo[1]) if pr.get("b") is not None else None
            sg = L.src(pr["g"])
            ws = self._slice()
            keep += [sa, sb, sg]
            slots.append(ws)
            descs[i].a, descs[i].g, descs[i].ws = C.pointer(sa), C.pointer(sg), ws
            descs[i].b = C.pointer(sb) if sb is not None else None
        nwg = C.c_int(0)
        L.check(L.lib().pc_conv3x3_wgrad_partial_group(n, descs, B, H, W, Ca + Cb, cout, C.byref(nwg), L.stream_ptr()),
                "pc_conv3x3_wgrad_partial_group")
        for ws, pr in zip(slots, problems):
            if pr.get("src_window") is not None:
                # the partials cover all Ca input channels; dw ([cout][cin][3][3]) receives the channels [ci0, ci0 + cin) only
                ci0, cin = pr["src_window"]
                assert pr["dw"].shape[1] == cin and ci0 + cin <= Ca + Cb and cin_total is None
                self.entries.append(ReduceEntry(ws, pr["dw"], pr["db"], nwg.value, cin, cout, 0, src_cin=Ca + Cb, src_ci0=ci0))
            elif cin_total is None:
                self.entries.append(ReduceEntry(ws, pr["dw"], pr["db"], nwg.value, Ca + Cb, cout, 0))
            else:
                self.entries.append(ReduceEntry(ws, pr["dw"], pr["db"], nwg.value, Ca + Cb, cout, 0, dw_co_stride=cin_total * 9))

    def conv3x3_bwd_group(self, problems, cin_total, c0, accumulate=False):
        """bf16 mode: data gradient + weight-gradient partials of a conv layer (g: 8 / 16 channels, x: an 8- or 16-channel column
        block of the layer's input) in ONE launch.  problems: list of dicts {g, x, w, out, dw (the full [Cg][cin_total][3][3]
        gradient), db (or None), x_bn (opt: ReLU / BN factor of x's producer), x_offset (opt), c0_add (opt: this problem's column
        block starts at c0 + c0_add -- the blocks of a concat layer in one launch), pool_act (opt: a Down block's first layer),
        pool_grad (opt, fp32: the pool-add form -- out also receives the max-pool scatter of this pooled-resolution gradient,
        popcorn_hip.h: pc_conv_bwd_desc)}; the partials cover the columns
        [c0 + c0_add, c0 + c0_add + x.shape[1]) of dw."""
        n = len(problems)
        g0 = problems[0]["g"]
        B, Cg, H, W = g0.shape
        keep, descs, slots = [], (L.PcConvBwdDesc * n)(), []
        for i, pr in enumerate(problems):
            xo = pr.get("x_offset", (0, 0))
            sg, sx, d = L.src(pr["g"]), L.src(pr["x"], oy=xo[0], ox=xo[1]), L.dst(pr["out"])
            ws = self._slice()
            keep += [sg, sx, d]
            slots.append(ws)
            descs[i].g, descs[i].x, descs[i].w, descs[i].out, descs[i].ws = C.pointer(sg), C.pointer(sx), pr["w"].data_ptr(), C.pointer(d), ws
            descs[i].x_bn = C.pointer(pr["x_bn"]) if pr.get("x_bn") is not None else None
            descs[i].c0_add = int(pr.get("c0_add", 0))
            if pr.get("pool_act") is not None:        # Down blocks: x is the pooled copy of pool_act; out is at twice the resolution (+=)
                spa = L.src(pr["pool_act"])
                keep.append(spa)
                descs[i].pool_act = C.pointer(spa)
            if pr.get("pool_grad") is not None:       # pool-add form: x also went through a MaxPool2d(2); its pooled copy's raw gradient
                spg = L.src(pr["pool_grad"])
                keep.append(spg)
                descs[i].pool_grad = C.pointer(spg)
        nwg = C.c_int(0)
        L.check(L.lib().pc_conv3x3_bwd_group(n, descs, cin_total, c0, int(accumulate), B, H, W, C.byref(nwg), L.stream_ptr()),
                "pc_conv3x3_bwd_group")
        for ws, pr in zip(slots, problems):
            self.entries.append(ReduceEntry(ws, pr["dw"], pr.get("db"), nwg.value, pr["x"].shape[1], Cg, 0, dw_co_stride=cin_total * 9,
                                            dw_offset=(c0 + int(pr.get("c0_add", 0))) * 9))      # first column of the column block

    def up_bwd_group(self, problems):
        """Composed Up block backward, deferred form: the pass now (data gradient written, partials queued), the reduction inside
        this batch's one reduce launch, the chain rule right after it (``finish``).  problems: as ops.conv3x3_up_bwd_group."""
        n = len(problems)
        g0, z0 = problems[0]["g"], problems[0]["z"]
        B, Cg, H, W = g0.shape
        Cz = z0.shape[1]
        nbytes = int(L.lib().pc_conv3x3_up_bwd_ws_bytes(B, H, Cz))
        descs = (L.PcConvUpBwdDesc * n)()
        keep, slots = [], []
        for i, pr in enumerate(problems):
            sg, sz = L.src(pr["g"]), L.src(pr["z"])
            dz = L.dst(pr["gz"]) if pr.get("gz") is not None else None
            ws = self._slice(nbytes)
            keep += [sg, sz, dz]
            slots.append(ws)
            descs[i].g, descs[i].z = C.pointer(sg), C.pointer(sz)
            descs[i].z_bn = C.pointer(pr["z_bn"])
            descs[i].gz = C.pointer(dz) if dz is not None else None
            descs[i].w, descs[i].wt = pr["w"].data_ptr(), pr["wt"].data_ptr()
            descs[i].bt = pr["bt"].data_ptr() if pr.get("bt") is not None else None
            descs[i].fwd_ws = pr["fwd_ws"].data_ptr()
            descs[i].ws = ws
            descs[i].dw, descs[i].dwt = pr["dw"].data_ptr(), pr["dwt"].data_ptr()
            descs[i].dbt = pr["dbt"].data_ptr() if pr.get("dbt") is not None else None
        nwg, part = C.c_int(0), C.c_int(0)
        L.check(L.lib().pc_conv3x3_up_bwd_partial_group(n, descs, B, H, W, Cz, Cz, C.byref(nwg), C.byref(part), L.stream_ptr()),
                "pc_conv3x3_up_bwd_partial_group")
        for ws in slots:
            self.raw_entries.append((ws, ws + 4 * nwg.value * part.value, nwg.value, part.value))
        self.chains.append((descs, keep, n, nwg.value, Cz, list(problems)))

    def level2_bwd_group(self, problems):
        """Backward of down2's DoubleConv (the 32 x 32 level) in ONE launch: problems = list of {g2 (dL/d conv2 output, masked),
        c1, x (pooled input), w1, w2, bn1 (BN of conv1: relu'(c1) factor), act (b2, full resolution), act_bn, out (G_b2, +=),
        dw1, db1, dw2, db2, pool_grad_out (opt, fp32: the raw gradient of x goes there INSTEAD of the scatter into out)}.  Queues the
        two layers' weight / bias gradient partials; the data gradients never leave the kernel (but for pool_grad_out)."""
        n = len(problems)
        B = problems[0]["g2"].shape[0]
        nbytes = int(L.lib().pc_level2_bwd_ws_bytes(B))
        descs = (L.PcLevel2BwdDesc * n)()
        keep, slices = [], []
        for i, pr in enumerate(problems):
            sg, sc, sx, sa, do = L.src(pr["g2"]), L.src(pr["c1"]), L.src(pr["x"]), L.src(pr["act"]), L.dst(pr["out"])
            ws1, ws2 = self._slice(nbytes), self._slice(nbytes)
            keep += [sg, sc, sx, sa, do]
            slices.append((ws1, ws2))
            descs[i].g2, descs[i].c1, descs[i].x, descs[i].act, descs[i].out = C.pointer(sg), C.pointer(sc), C.pointer(sx), C.pointer(sa), C.pointer(do)
            descs[i].w1, descs[i].w2 = pr["w1"].data_ptr(), pr["w2"].data_ptr()
            descs[i].bn1, descs[i].act_bn = C.pointer(pr["bn1"]), C.pointer(pr["act_bn"])
            descs[i].ws1, descs[i].ws2 = ws1, ws2
            if pr.get("pool_grad_out") is not None:
                dpg = L.dst(pr["pool_grad_out"])
                keep.append(dpg)
                descs[i].pool_grad_out = C.pointer(dpg)
        nwg = C.c_int(0)
        L.check(L.lib().pc_level2_bwd_group(n, descs, B, C.byref(nwg), L.stream_ptr()), "pc_level2_bwd_group")
        for (ws1, ws2), pr in zip(slices, problems):
            self.entries.append(ReduceEntry(ws1, pr["dw1"], pr["db1"], nwg.value, 16, 16, 0))
            self.entries.append(ReduceEntry(ws2, pr["dw2"], pr["db2"], nwg.value, 16, 16, 0))

    def convt2x2_group(self, problems):
        """problems: list (<= 4) of dicts {x, g, dw, db} with identical geometry: one launch."""
        n = len(problems)
        x0 = problems[0]["x"]
        B, Cc, H, W = x0.shape
        descs = (L.PcConvtWgradDesc * n)()
        keep, slices = [], []
        for i, pr in enumerate(problems):
            sx, sg = L.src(pr["x"]), L.src(pr["g"])
            ws = self._slice()
            keep += [sx, sg]
            slices.append(ws)
            descs[i].x, descs[i].g, descs[i].ws = C.pointer(sx), C.pointer(sg), ws
        nwg = C.c_int(0)
        L.check(L.lib().pc_convt2x2_wgrad_partial_group(n, descs, B, H, W, Cc, C.byref(nwg), L.stream_ptr()),
                "pc_convt2x2_wgrad_partial_group")
        for ws, pr in zip(slices, problems):
            self.entries.append(ReduceEntry(ws, pr["dw"], pr["db"], nwg.value, Cc, Cc, 1))

    def convt2x2_bwd_group(self, problems):
        """Whole backward of a transposed conv in one launch: problems = list of {x, g, w, out, dw, db, x_bn (opt: ReLU / BN factor
        of x's producer)}; writes the data gradient into out and queues the weight / bias gradient partials."""
        n = len(problems)
        B, Cc, H, W = problems[0]["x"].shape
        descs = (L.PcConvtBwdDesc * n)()
        keep, slices = [], []
        for i, pr in enumerate(problems):
            sx, sg, d = L.src(pr["x"]), L.src(pr["g"]), L.dst(pr["out"])
            ws = self._slice()
            keep += [sx, sg, d]
            slices.append(ws)
            descs[i].x, descs[i].g, descs[i].w, descs[i].out, descs[i].ws = C.pointer(sx), C.pointer(sg), pr["w"].data_ptr(), C.pointer(d), ws
            descs[i].x_bn = C.pointer(pr["x_bn"]) if pr.get("x_bn") is not None else None
        nwg = C.c_int(0)
        L.check(L.lib().pc_convt2x2_bwd_group(n, descs, B, H, W, Cc, C.byref(nwg), L.stream_ptr()), "pc_convt2x2_bwd_group")
        for ws, pr in zip(slices, problems):
            self.entries.append(ReduceEntry(ws, pr["dw"], pr["db"], nwg.value, Cc, Cc, 1))

    def head_reduce(self, hp):
        assert self.head is None and isinstance(hp, HeadPartials)
        self.head = hp

    def finish(self):
        n = len(self.entries) + len(self.raw_entries) + (1 if self.head is not None else 0)
        if n == 0:
            return
        d = (L.PcWgradReduceDesc * n)()
        if self.head is not None:       # (kind 3: dw = HOST array of the 8 gradient tensors)
            hp, self.head = self.head, None
            dhw = (C.c_void_p * 8)(*[0 if t is None else t.data_ptr() for t in hp.grads])
            i = n - 1
            d[i].partial, d[i].dw, d[i].db = hp.ptr, C.cast(dhw, C.c_void_p).value, 0
            d[i].nwg, d[i].Cin, d[i].Cout, d[i].kind, d[i].accumulate, d[i].dw_co_stride = hp.nwg, 0, 0, 3, int(hp.accumulate), 0
        acc = int(self.accumulate)
        for i, e in enumerate(self.entries):
            d[i].partial, d[i].dw, d[i].db = e.partial, e.dw.data_ptr() + 4 * e.dw_offset, 0 if e.db is None else e.db.data_ptr()
            d[i].nwg, d[i].Cin, d[i].Cout, d[i].kind, d[i].accumulate = e.nwg, e.Cin, e.Cout, e.kind, acc
            d[i].dw_co_stride, d[i].src_cin, d[i].src_ci0 = e.dw_co_stride, e.src_cin, e.src_ci0
        for j, (pp, tot, nwg, part) in enumerate(self.raw_entries):
            i = len(self.entries) + j
            d[i].partial, d[i].dw, d[i].db = pp, tot, 0
            d[i].nwg, d[i].Cin, d[i].Cout, d[i].kind, d[i].accumulate, d[i].dw_co_stride = nwg, part, 0, 2, 0, 0
        L.check(L.lib().pc_wgrad_reduce_batch(n, d, L.stream_ptr()), "pc_wgrad_reduce_batch")
        c8 = [c for c in self.chains if c[4] == 8]
        c16 = [c for c in self.chains if c[4] == 16]
        if len(c8) == 1 and len(c16) == 1 and len(self.chains) == 2:        # the two Up levels of a U-Net backward: one launch
            L.check(L.lib().pc_conv3x3_up_chain_both(c8[0][2], c8[0][0], c8[0][3], c16[0][2], c16[0][0], c16[0][3],
                                                     int(self.accumulate), L.stream_ptr()), "pc_conv3x3_up_chain_both")
        else:
            for descs, keep, cn, nwg, Cz, probs in self.chains:
                L.check(L.lib().pc_conv3x3_up_chain_group(cn, descs, int(self.accumulate), nwg, Cz, Cz, L.stream_ptr()),
                        "pc_conv3x3_up_chain_group")
        self.entries, self.raw_entries, self.chains = [], [], []
        self.slot = 0
