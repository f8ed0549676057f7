"""Input-image gradient (csrc/input_grad.hip), the parts that need no GPU: the entry point and its op exist, and the launcher's argument
validation returns PC_EINVAL before anything is launched -- on a host without a device a call that got as far as the launch would come
back with a HIP error code instead.  The descriptors point at made-up addresses: a validated-away call never reads them."""
import ctypes as C

import pytest

from popcorn_amd import _lib as L

FAKE_G, FAKE_W, FAKE_DX = 0x10000, 0x20000, 0x30000          # 16-byte aligned, never dereferenced
SAR, OPT = (4, 5), (2, 1, 0, 3)


def g_src(Hp, Wp, channels=8, bf16=False):
    s = L.PcSrc()
    s.ptr, s.C, s.H, s.W = FAKE_G, channels, Hp, Wp
    if bf16:                 # channels-last: one 16-byte slot per pixel
        s.bstride, s.cstride, s.rstride, s.xstride, s.dtype = Hp * Wp * 8, 1, Wp * 8, 8, L.PC_BF16_T
    else:
        s.bstride, s.cstride, s.rstride, s.xstride, s.dtype = channels * Hp * Wp, Hp * Wp, Wp, 1, L.PC_F32_T
    s.mode = L.PC_SRC_DIRECT
    return s


def call(streams, Cx=6, H=8, W=8, pads=(2, 2, 2, 2), channels=8, bf16=False, B=2):
    """pc_input_grad for streams = [(cin, chmap)], every operand well-formed unless an argument says otherwise"""
    pt, pb, pl, pr = pads
    keep = [g_src(H + pt + pb, W + pl + pr, channels, bf16) for _ in streams]
    d = (L.PcInputGradDesc * len(streams))()
    for i, (cin, chmap) in enumerate(streams):
        d[i].g, d[i].w, d[i].cin = C.pointer(keep[i]), FAKE_W, cin
        for c, ch in enumerate(chmap):
            d[i].chmap[c] = ch
    return L.lib().pc_input_grad(len(streams), d, FAKE_DX, B, Cx, H, W, pt, pb, pl, pr, None)


def test_entry_point_and_op_exist():
    from popcorn_amd import ops
    assert hasattr(L.lib(), "pc_input_grad")
    assert callable(ops.input_grad)
    assert C.sizeof(L.PcInputGradDesc) == 40


def test_abi_version_is_unchanged():
    assert L.lib().pc_abi_version() == 10 == L.PC_ABI_VERSION


def test_well_formed_call_passes_validation():
    """the baseline every case below spoils in ONE way: it gets past the validation (and fails at the launch: no device here)"""
    if L.lib().pc_device_count() > 0:
        pytest.skip("with a device the well-formed call would launch on made-up addresses (tests/test_gpu_input_grad.py runs it for real)")
    assert call([(2, SAR), (4, OPT)]) != L.PC_EINVAL
    assert call([(2, (0, 1))], Cx=2) != L.PC_EINVAL
    assert call([(4, OPT)], Cx=4) != L.PC_EINVAL
    assert call([(2, SAR), (4, OPT)], pads=(7, 7, 7, 7)) != L.PC_EINVAL          # pad = extent - 1: torch's limit


@pytest.mark.parametrize("pads", [(8, 0, 0, 0), (0, 8, 0, 0), (0, 0, 8, 0), (0, 0, 0, 8), (-1, 0, 0, 0)])
def test_pad_not_smaller_than_extent(pads):
    assert call([(2, SAR), (4, OPT)], H=8, W=8, pads=pads) == L.PC_EINVAL


def test_gradient_with_16_channels():
    assert call([(2, SAR), (4, OPT)], channels=16) == L.PC_EINVAL


def test_three_input_channels():
    assert call([(3, (0, 1, 2))], Cx=4) == L.PC_EINVAL
    assert call([(3, (0, 1, 2)), (3, (3, 4, 5))], Cx=6) == L.PC_EINVAL


def test_uncovered_channel():
    assert call([(4, OPT)], Cx=6) == L.PC_EINVAL                     # channels 4, 5 of dX unwritten
    assert call([(2, SAR)], Cx=6) == L.PC_EINVAL
    assert call([(2, (0, 1))], Cx=4) == L.PC_EINVAL


def test_channel_covered_twice():
    assert call([(2, (4, 4)), (4, OPT)]) == L.PC_EINVAL
    assert call([(2, (0, 1)), (4, OPT)]) == L.PC_EINVAL              # 0 and 1 twice, 4 and 5 never
    assert call([(4, (0, 1, 2, 2))], Cx=4) == L.PC_EINVAL
    assert call([(2, (0, 7))], Cx=2) == L.PC_EINVAL                  # outside dX


def test_descriptor_must_match_the_arithmetic_mode():
    assert L.lib().pc_get_precision() == L.PC_PREC_FP32
    assert call([(2, SAR), (4, OPT)], bf16=True) == L.PC_EINVAL      # a bf16 descriptor in fp32 mode
    with L.precision("bf16"):
        assert call([(2, SAR), (4, OPT)], bf16=False) == L.PC_EINVAL


def test_problem_count_and_null_operands():
    assert call([]) == L.PC_EINVAL
    assert call([(2, SAR), (2, SAR), (4, OPT)]) == L.PC_EINVAL
    assert call([(2, SAR), (4, OPT)], B=0) == L.PC_EINVAL
    assert call([(2, SAR), (4, OPT)], Cx=5) == L.PC_EINVAL
