"""The backward pass takes ONE of two orders at level 1 (engine.py: _Backward.pool_add_plan, csrc/step.hip: Backward::pool_add_plan):
today's (skip launch, later the Down block's first layer with the max-pool scatter) or the pool-add order (first layer raw at the
pooled resolution, then the skip launch with pool_grad).  The executors choose the second where today's fused pair of the Down block
applies AND the launcher takes the plain first layer and the pool-add skip launch.  On every add_padding domain (sides multiples of
32), in the executor's arena layout, the second condition follows from the first: a training step never mixes the two orders.
Descriptors only: nothing is dereferenced, no GPU."""
import ctypes


def test_every_training_domain_that_fuses_down1_takes_the_pool_add_order():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert lib.pc_get_precision() == L.PC_PREC_FP32
    base = 1 << 40
    ref = ctypes.byref

    def views(c, h, w, c_of=None, c0=0):
        """a (c_of or c)-channel arena tensor (rows padded to 4 floats), seen as its channels [c0, c0 + c)"""
        sr = (w + 3) & ~3
        sc = h * sr
        bs = (c_of or c) * sc
        ptr = base + 4 * c0 * sc
        src = L.PcSrc(ptr=ptr, C=c, H=h, W=w, bstride=bs, cstride=sc, rstride=sr, mode=L.PC_SRC_DIRECT, oy=0, ox=0,
                      chmap=(ctypes.c_int32 * 4)(0, 1, 2, 3), dtype=L.PC_F32_T, xstride=1)
        dst = L.PcDst(ptr=ptr, bstride=bs, cstride=sc, rstride=sr, dtype=L.PC_F32_T, xstride=1)
        return src, dst

    def check(B, Hp, Wp):
        H1, W1 = Hp // 2, Wp // 2
        g_f1, g_a2 = views(8, Hp, Wp)                       # up1a's output gradient; inc2's output gradient
        a2, _ = views(8, Hp, Wp)
        g_b2, _ = views(16, H1, W1)                         # d1b's output gradient
        g_mid, _ = views(16, H1, W1)
        b1_half, g_mid_half = views(8, H1, W1, c_of=16, c0=8)
        pa2, g_pa2_dst = views(8, H1, W1)
        g_pa2 = pa2
        today = (lib.pc_conv3x3_bwd_ok(ref(g_b2), ref(b1_half), ref(g_mid_half), None, B, H1, W1)
                 and lib.pc_conv3x3_bwd_ok(ref(g_mid), ref(pa2), ref(g_a2), ref(a2), B, H1, W1))
        new = (lib.pc_conv3x3_bwd_ok(ref(g_mid), ref(pa2), ref(g_pa2_dst), None, B, H1, W1)
               and lib.pc_conv3x3_bwd_pool_add_ok(ref(g_f1), ref(a2), ref(g_a2), ref(g_pa2), B, Hp, Wp))
        return bool(today), bool(new)

    mixed, accepted, declined = [], 0, 0
    for B in (1, 3):
        for Hp in range(32, 2049, 32):
            for Wp in range(32, 2049, 32):
                today, new = check(B, Hp, Wp)
                accepted += today
                if today and not new:
                    mixed.append((B, Hp, Wp))
    assert not mixed, mixed[:8]
    assert accepted == 2 * 64 * 64                          # (every such domain fuses down1 today)
    # batches whose tensors outgrow the split-operand kernel's 32-bit offsets: today's pair declines, and so does the new order's plan
    for Hp in range(256, 2049, 256):
        today, new = check(64, Hp, 2048)
        declined += not today
        assert not (today and not new), (64, Hp)
    assert declined > 0


def test_pool_add_predicate_declines_what_the_kernel_cannot_take():
    from popcorn_amd import _lib as L
    lib = L.lib()
    base = 1 << 40

    def src(c, h, w, ptr=base, sr=None):
        sr = sr or (w + 3) & ~3
        return L.PcSrc(ptr=ptr, C=c, H=h, W=w, bstride=c * h * sr, cstride=h * sr, rstride=sr, mode=L.PC_SRC_DIRECT, oy=0, ox=0,
                       chmap=(ctypes.c_int32 * 4)(0, 1, 2, 3), dtype=L.PC_F32_T, xstride=1)

    def ok(H, W, pg):
        g = src(8, H, W)
        out = L.PcDst(ptr=base, bstride=g.bstride, cstride=g.cstride, rstride=g.rstride, dtype=L.PC_F32_T, xstride=1)
        return bool(lib.pc_conv3x3_bwd_pool_add_ok(ctypes.byref(g), ctypes.byref(g), ctypes.byref(out),
                                                   ctypes.byref(pg) if pg is not None else None, 2, H, W))

    assert ok(8, 32, src(8, 4, 16))
    assert not ok(8, 48, src(8, 4, 24))                     # W % 32: a window would straddle two strips
    assert not ok(6, 32, src(8, 3, 16))                     # H % 4
    assert not ok(8, 32, None)
    assert not ok(8, 32, src(8, 4, 16, ptr=base + 4))       # rows off the 8-byte boundary
    assert not ok(8, 32, src(8, 4, 16, sr=17))
    assert not ok(8, 32, src(16, 4, 16))                    # 8 channels, at half the resolution
    assert not ok(8, 32, src(8, 2, 16))
