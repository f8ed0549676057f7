"""Shared by the conv ablation tools: does the loaded library honour pc_debug_conv's phase switches and pc_debug_conv_ts?

The product library compiles them out (run-time ablation switches are not free).  They exist in a
-DPOPCORN_CONV_ABLATE build only:

    tools/build_variant.sh ablate -DPOPCORN_CONV_ABLATE
    POPCORN_HIP_LIB=ab/libpopcorn_ablate.so python3 tools/<tool>.py

Forced grid sizes (the second argument of pc_debug_conv) are host code and work in every build."""
import sys
import torch
from popcorn_amd import ops, _lib as L


def ablation_build():
    """Switch 4 (no epilogue) leaves the output of a conv launch untouched in an ablation build; a product build ignores it."""
    x = L.as_act(torch.randn(1, 8, 16, 32, device="cuda"))
    w, bias = torch.randn(8, 8, 3, 3, device="cuda"), torch.zeros(8, device="cuda")
    out = L.as_act(torch.full((1, 8, 16, 32), 7.0, device="cuda"))
    L.lib().pc_debug_conv(4, 0)
    ops.conv3x3_fwd_group([{"a": x, "w": w, "bn": L.bn(bias), "out": out}])
    L.lib().pc_debug_conv(0, 0)
    torch.cuda.synchronize()
    return bool((out.float() == 7.0).all())


def unablated_only(variants):
    """variants = [(dbg, ...), ...]: all of them in an ablation build, the dbg == 0 rows (with a note) in a product build"""
    if ablation_build():
        return variants
    print("product build: the phase switches need POPCORN_HIP_LIB = a -DPOPCORN_CONV_ABLATE build "
          "(tools/build_variant.sh ablate -DPOPCORN_CONV_ABLATE; POPCORN_HIP_LIB=ab/libpopcorn_ablate.so); unablated rows only", file=sys.stderr)
    return [v for v in variants if v[0] == 0]
