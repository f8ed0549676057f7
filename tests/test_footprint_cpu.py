"""The footprint harness itself (tests/footprint.py) on host tensors: layout of what it hands out, what it leaves alone, and that
it notices a one-element overrun on either side.  Every deliberate overrun is an ``as_strided`` write into the harness's own band."""
import pytest
import torch

from tests import footprint as FP


def _is_nan_bits(t):
    return bool(torch.isnan(t.float()).all())


def test_planar_padded_row_and_channels_last_keep_strides_and_alignment():
    with FP.Footprint("cpu") as fp:
        planar = torch.empty(2, 3, 5, 7, device="cpu")
        padded = torch.empty(2, 3, 5, 8, device="cpu", dtype=torch.float32)[..., :7]
        cl = torch.empty(2, 8, 5, 7, device="cpu", dtype=torch.bfloat16, memory_format=torch.channels_last)
        strided = torch.empty_strided((3, 4), (1, 3), device="cpu", dtype=torch.int32)
        like = torch.empty_like(cl)
        moved = torch.arange(24.0).view(2, 3, 4).transpose(1, 2).to("cpu")
        assert fp.guarded == 6
    assert planar.shape == (2, 3, 5, 7) and planar.stride() == (105, 35, 7, 1) and planar.dtype == torch.float32
    assert padded.shape == (2, 3, 5, 7) and padded.stride() == (120, 40, 8, 1)
    assert cl.shape == (2, 8, 5, 7) and cl.stride() == (280, 1, 56, 8) and cl.is_contiguous(memory_format=torch.channels_last)
    assert strided.stride() == (1, 3) and like.stride() == cl.stride() and like.dtype == torch.bfloat16
    assert moved.stride() == (12, 1, 4) and torch.equal(moved, torch.arange(24.0).view(2, 3, 4).transpose(1, 2))
    for t in (planar, padded, cl, strided, like, moved):
        assert t.data_ptr() % 512 == 0
    # poison mode: an unwritten empty is NaN, pad columns included
    assert _is_nan_bits(planar) and _is_nan_bits(cl) and _is_nan_bits(padded.as_strided((2, 3, 5, 8), (120, 40, 8, 1)))
    assert bool((strided == -1).all())


def test_band_rule():
    assert FP.band_bytes((2, 3, 5, 7), (105, 35, 7, 1), 4) == 64 * 1024                    # small tensors: the 64 KiB floor
    assert FP.band_bytes((1, 8, 300, 200), (480000, 60000, 200, 1), 4) == 240128           # one plane, rounded up to 512
    assert FP.band_bytes((1, 8, 300, 200), (480000, 1, 1600, 8), 2) == 960000              # channels-last: one image
    assert FP.band_bytes((100000,), (1,), 4) == 400384
    with FP.Footprint("cpu") as fp:
        torch.empty(1, 2, 300, 200, device="cpu")
        r = fp.records[0]
        assert r.lo >= 240128 and r.raw.numel() - r.hi >= 240128 and r.hi - r.lo == 2 * 300 * 200 * 4


def test_defined_contents_survive_and_clean_fill_is_zero():
    with FP.Footprint("cpu", fill=FP.POISON) as fp:
        z = torch.zeros(3, 5, device="cpu")
        zl = torch.zeros_like(z)
        o = torch.ones(4, device="cpu", dtype=torch.int32)
        f = torch.full((2, 3), 7.0, device="cpu")
        n = torch.full((2,), float("nan"), device="cpu")
        c = torch.tensor([1, 2, 3], dtype=torch.uint8).to(torch.device("cpu"), torch.float32)
        assert fp.guarded == 6
    assert bool((z == 0).all()) and bool((zl == 0).all()) and bool((o == 1).all()) and bool((f == 7.0).all())
    assert _is_nan_bits(n) and f.dtype == torch.float32 and o.dtype == torch.int32
    assert torch.equal(c, torch.tensor([1.0, 2.0, 3.0]))
    with FP.Footprint("cpu", fill=FP.CLEAN) as fp:
        e = torch.empty(3, 5, device="cpu")
        p = fp.place(torch.arange(12.0).view(3, 4)[:, :3])
    assert bool((e == 0).all())
    assert torch.equal(p, torch.arange(12.0).view(3, 4)[:, :3]) and p.stride() == (4, 1)
    assert bool((p.as_strided((3, 4), (4, 1))[:2, 3] == 0).all())                          # pad elements hold the fill, not the source's


def test_calls_without_a_device_and_host_tensors_are_left_alone():
    with FP.Footprint("cpu") as fp:
        a = torch.empty(3)
        b = torch.zeros(3)
        assert fp.guarded == 0
        w = torch.ones(2, requires_grad=True)
        assert w.to("cpu") is w                                                            # autograd leaves pass through
    assert a.shape == (3,) and bool((b == 0).all())


def test_torch_tensor_and_copies_made_on_the_device_are_rehomed():
    with FP.Footprint("cpu") as fp:
        a = torch.tensor([1, 2, 3], device="cpu")
        b = a.float()
        c = b.clone()
        d = torch.zeros(2, 8, 3, 4, device="cpu").contiguous(memory_format=torch.channels_last)
        e = b.to(torch.bfloat16)
        assert b.contiguous() is b and b.to(torch.float32) is b and b.view(3, 1).data_ptr() == b.data_ptr()   # nothing new
        assert fp.guarded == 6
    assert a.dtype == torch.int64 and a.tolist() == [1, 2, 3] and b.tolist() == [1.0, 2.0, 3.0] and torch.equal(c, b)
    assert d.stride() == (96, 1, 32, 8) and bool((d == 0).all()) and e.dtype == torch.bfloat16 and e.tolist() == [1.0, 2.0, 3.0]
    for t in (a, b, c, d, e):
        assert t.data_ptr() % 512 == 0


def test_patched_attributes_are_restored_after_an_exception():
    before = {n: getattr(torch, n) for n in FP._CREATORS + FP._LIKES + ("tensor",)}
    before_m = {n: getattr(torch.Tensor, n) for n in FP._COPIES}
    had = ("cuda" in torch.Tensor.__dict__, "to" in torch.Tensor.__dict__)
    cuda, to = torch.Tensor.cuda, torch.Tensor.to
    with pytest.raises(RuntimeError, match="boom"):
        with FP.Footprint("cpu"):
            assert torch.empty is not before["empty"]
            raise RuntimeError("boom")
    for n, f in before.items():
        assert getattr(torch, n) is f, n
    assert torch.Tensor.cuda is cuda and torch.Tensor.to is to
    for n, f in before_m.items():
        assert getattr(torch.Tensor, n) is f and n not in torch.Tensor.__dict__, n
    assert ("cuda" in torch.Tensor.__dict__, "to" in torch.Tensor.__dict__) == had


@pytest.mark.parametrize("side", ["before", "after"])
def test_one_element_overrun_fails_the_exit_check_and_names_the_side(side):
    with pytest.raises(FP.FootprintError) as e:
        with FP.Footprint("cpu") as fp:
            t = torch.zeros(4, 6, device="cpu")
            r = fp.records[0]
            whole = r.raw.view(torch.float32)                                              # the harness's own buffer
            first = r.lo // 4
            whole.as_strided((1,), (1,), first - 1 if side == "before" else first + 24).fill_(1.0)
            assert bool((t == 0).all())                                                    # the payload itself is untouched
    msg = str(e.value)
    assert f"band {side} the payload" in msg and "(4, 6)" in msg and "test_footprint_cpu.py" in msg
    assert ("offset -4 " if side == "before" else "offset +0 ") in msg


def test_intact_bands_pass_and_check_can_run_inside_the_block():
    with FP.Footprint("cpu") as fp:
        t = torch.empty(5, 9, device="cpu")
        t.fill_(3.0)
        t[-1, -1] = 4.0
        fp.check()


def test_read_before_write_of_a_poisoned_empty_is_visible_as_nan():
    def sums(fill):
        with FP.Footprint("cpu", fill=fill):
            acc = torch.empty(8, device="cpu")
            acc[:7] = 1.0                                                                  # the "kernel" forgets the last element
            return acc.sum()
    assert torch.isnan(sums(FP.POISON)) and sums(FP.CLEAN).item() == 7.0
    assert not FP.bit_equal(sums(FP.POISON), sums(FP.CLEAN))
