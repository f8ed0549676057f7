"""The row / column selection draw of get_sparsity_mask (popcorn.py:366-369; the sparse_unet grid of :336-343 with sub = 250) exists once,
``popcorn_amd.model.popcorn.draw_selection``; the model API and the fused step both call it.  It must consume the CPU generator exactly
like the reference formula, written inline here: the same flags and the same generator state afterwards."""
import pytest
import torch

from popcorn_amd.model.popcorn import draw_selection
from popcorn_amd.train import FusedTrainStep

SHAPES = [(100, 100), (7, 250), (300, 61), (40, 1100)]          # sides below, at and above both grid sizes


def reference_flags(H, W, sub):
    xi = torch.ones(H).multinomial(num_samples=min(sub, H), replacement=False)
    yi = torch.ones(W).multinomial(num_samples=min(sub, W), replacement=False)
    sel = torch.zeros(H + W, dtype=torch.uint8)
    sel[xi] = 1
    sel[H + yi] = 1
    return sel


@pytest.mark.parametrize("sub", [60, 250])
@pytest.mark.parametrize("H,W", SHAPES)
def test_draw_selection_is_the_reference_draw(H, W, sub):
    for k in (0, 3, 1600):
        torch.manual_seed(k)
        want = reference_flags(H, W, sub)
        state = torch.get_rng_state()
        torch.manual_seed(k)
        got = draw_selection(H, W, sub)
        assert got.dtype == torch.uint8 and got.device.type == "cpu" and tuple(got.shape) == (H + W,)
        assert torch.equal(got, want)
        assert torch.equal(torch.get_rng_state(), state)
        assert int(got[:H].sum()) == min(sub, H) and int(got[H:].sum()) == min(sub, W)
        # a second draw continues the stream like the formula does (nothing cached but the ones vector)
        again = draw_selection(H, W, sub)
        torch.set_rng_state(state)
        assert torch.equal(again, reference_flags(H, W, sub))


@pytest.mark.parametrize("H,W", SHAPES)
def test_trainer_draw_is_draw_selection(H, W):
    torch.manual_seed(11)
    want = draw_selection(H, W)
    state = torch.get_rng_state()
    torch.manual_seed(11)
    got = FusedTrainStep._draw_selection(H, W)
    assert got.dtype == torch.uint8 and got.device.type == "cpu"
    assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)
