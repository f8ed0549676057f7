"""Every kernel family under the memory-footprint harness (tests/footprint.py).

The existing op tests are run as they are -- same operands, same reference, same tolerance -- inside ``Footprint("cuda", fill=POISON)``:
their inputs (``.cuda()`` / ``.to(device)`` / ``torch.full`` / ...) and the outputs and workspaces ``ops.py`` allocates sit between bands of
bytes 0xFF, every ``torch.empty`` payload is 0xFF (NaN) too, and leaving the block checks every band bit for bit.  A store past a tensor
fails the band check; a load past an input, or of memory nobody wrote, that reaches a result fails the test's own comparison as NaN.
One case per family and arithmetic mode: the family's smallest ragged shape and, where it has one, its smallest aligned shape (the 16-byte
epilogues only run there).  ``ops.ingest_split`` had no op-level test: it gets one here."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.test_gpu_bf16 as t_bf16
import tests.test_gpu_census_table as t_census
import tests.test_gpu_conv3x3 as t_conv
import tests.test_gpu_conv_fwd_split as t_split
import tests.test_gpu_convt_head as t_ch
import tests.test_gpu_eval_kernels as t_ev
import tests.test_gpu_feed as t_feed
import tests.test_gpu_input_grad as t_ig
import tests.test_gpu_level2 as t_l2
import tests.test_gpu_nan_fill as t_nan
import tests.test_gpu_product as t_prod
import tests.test_gpu_sizes as t_sizes
import tests.test_gpu_train_tail as t_tail
import tests.test_gpu_units as t_units
import tests.test_gpu_units_native as t_un
from tests import footprint as FP

pytestmark = pytest.mark.gpu

HEAD = (1, 37, 29, 64, 64, 13, 17)


@contextlib.contextmanager
def _switch(setter, value):
    """pc_set_conv_split / pc_set_head_split for the block (what the conv_form / head_form fixtures of the reused modules do)"""
    from popcorn_amd import _lib as L
    prev = getattr(L.lib(), setter)(int(value))
    try:
        yield int(value)
    finally:
        getattr(L.lib(), setter)(prev)


@contextlib.contextmanager
def fresh_workspaces():
    """ops._workspace and ops.WgradBatch hand out cached buffers: set the caches aside so the block's workspaces are created under the
    harness (and put them back: earlier launches and captured graphs may still hold their addresses)"""
    from popcorn_amd import ops
    caches = (ops._ws_cache, ops.WgradBatch._ws)
    saved = [dict(c) for c in caches]
    for c in caches:
        c.clear()
    try:
        yield
    finally:
        for c, was in zip(caches, saved):
            c.clear()
            c.update(was)


def _pair():
    """what the ``pair`` fixture of test_gpu_sizes builds"""
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval()
    return m, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _conv_form(fn, form):
    def run(*a):
        with _switch("pc_set_conv_split", form) as f:
            fn(*a, f)
    return run


def _head_form(fn, form):
    def run(*a):
        with _switch("pc_set_head_split", form) as f:
            fn(*a, f)
    return run


def _monkeypatched(fn):
    def run(*a):
        with pytest.MonkeyPatch.context() as mp:
            fn(mp, *a)
    return run


# (id, callable, arguments, least number of guarded allocations = the op's outputs + the operands the test puts on the device)
CASES = [
    # ---- conv3x3 forward: plain, split form, pooled second output, partial logit
    ("conv_fwd-8to8-1x37x53", t_conv.test_conv_fwd_direct, (8, 8, (1, 37, 53)), 8),
    ("conv_fwd-2to8-1x37x53", t_conv.test_conv_fwd_direct, (2, 8, (1, 37, 53)), 8),
    ("conv_fwd-32to8-1x37x53", t_conv.test_conv_fwd_direct, (32, 8, (1, 37, 53)), 8),
    ("conv_fwd-16to16-3x16x32", t_conv.test_conv_fwd_direct, (16, 16, (3, 16, 32)), 8),
    ("conv_fwd-pool_concat_loaders", t_conv.test_conv_fwd_pool_and_concat_with_up_pad, (), 16),
    ("conv_fwd-reflect_loader", t_conv.test_conv_fwd_reflect_reorder, (), 16),
    ("conv_fwd_split-8to16-1x5x4", t_split.test_forward_split_form_vs_float64, (8, 16, (1, 5, 4)), 9),
    ("conv_fwd_split-16to16-2x20x8", t_split.test_forward_split_form_vs_float64, (16, 16, (2, 20, 8)), 9),
    ("conv_fwd_split-16to8-3x16x32", t_split.test_forward_split_form_vs_float64, (16, 8, (3, 16, 32)), 9),
    ("conv_fwd_split-8to8-1x36x52", t_split.test_forward_split_form_vs_float64, (8, 8, (1, 36, 52)), 9),
    ("conv_fwd-pooled_output-1x128x32", t_conv.test_conv_fwd_pooled_second_output, (8, 8, (1, 128, 32)), 9),
    ("conv_fwd_split-pooled_output-1x128x32", t_split.test_forward_split_form_pooled_second_output, (8, 8, (1, 128, 32)), 5),
    ("conv_fwd-partial_logit", t_conv.test_conv_fwd_partial_logit_output, (), 13),
    ("conv_fwd_split-partial_logit", t_split.test_forward_split_form_partial_logit_output, (), 5),
    ("conv_fwd-bf16-8to8-1x37x53", t_bf16.test_bf16_conv_fwd_op, (8, 8, (1, 37, 53)), 4),
    ("conv_fwd-bf16-16to16-3x16x32", t_bf16.test_bf16_conv_fwd_op, (16, 16, (3, 16, 32)), 4),
    ("conv_fwd-bf16-loaders", t_bf16.test_bf16_conv_asymmetric_taps_and_loaders, (), 8),
    # ---- conv3x3 dgrad: plain / masked / pool scatter, single and group
    ("conv_dgrad-8of8-2x29x47", t_conv.test_conv_dgrad_plain_and_masked, (8, 0, 8, 8, (2, 29, 47)), 12),
    ("conv_dgrad-16of32-cg8-2x29x47", t_conv.test_conv_dgrad_plain_and_masked, (32, 16, 16, 8, (2, 29, 47)), 12),
    ("conv_dgrad-16of16-cg16-2x32x64", t_conv.test_conv_dgrad_plain_and_masked, (16, 0, 16, 16, (2, 32, 64)), 12),
    ("conv_dgrad-pool_scatter-cn8-2x38x53", t_conv.test_conv_dgrad_pool_scatter_matches_autograd, ((2, 38, 53), 8), 8),
    ("conv_dgrad-pool_scatter-cn16-2x38x53", t_conv.test_conv_dgrad_pool_scatter_matches_autograd, ((2, 38, 53), 16), 8),
    ("conv_dgrad-refusal-single", t_conv.test_conv_dgrad_refuses_gradients_no_layer_produces, (2, False, "fp32"), 3),
    ("conv_dgrad-refusal-group-bf16", t_conv.test_conv_dgrad_refuses_gradients_no_layer_produces, ("pool2", True, "bf16"), 3),
    # ---- conv3x3 wgrad
    ("conv_wgrad-8to8-1x37x53", t_conv.test_conv_wgrad, (8, 8, (1, 37, 53)), 4),
    ("conv_wgrad-2to8-1x37x53", t_conv.test_conv_wgrad, (2, 8, (1, 37, 53)), 4),
    ("conv_wgrad-4to8-1x37x53", t_conv.test_conv_wgrad, (4, 8, (1, 37, 53)), 4),
    ("conv_wgrad-16to16-1x37x53", t_conv.test_conv_wgrad, (16, 16, (1, 37, 53)), 4),
    ("conv_wgrad-pool_concat_loaders", t_conv.test_conv_wgrad_fused_loaders, (), 9),
    ("conv_wgrad-single_vs_batched-1x37x53", t_conv.test_conv_wgrad_single_op_equals_the_batched_path, ((1, 37, 53), False), 6),
    ("conv_wgrad-bf16-8to8-1x37x53", t_bf16.test_bf16_conv_wgrad_op, (8, 8, (1, 37, 53)), 4),
    ("conv_wgrad-bf16-16to16-3x16x32", t_bf16.test_bf16_conv_wgrad_op, (16, 16, (3, 16, 32)), 4),
    ("conv_wgrad-bf16-reflect_loader-cin2", t_bf16.test_bf16_first_layer_wgrad_reflect_loader, (2,), 4),
    ("conv_wgrad-bf16-reflect_loader-cin4", t_bf16.test_bf16_first_layer_wgrad_reflect_loader, (4,), 4),
    ("conv_wgrad-bf16-pool_concat_loaders", t_bf16.test_bf16_conv_wgrad_pool_and_concat_loaders, (), 6),
    # ---- fused conv backward
    ("conv_bwd-split-concat_skip_accumulate-1x36x52", _conv_form(t_conv.test_conv_backward_fused_op_fp32, 1),
     ((1, 36, 52), "concat_skip_half_accumulate"), 11),
    ("conv_bwd-split-plain_masked-2x20x8", _conv_form(t_conv.test_conv_backward_fused_op_fp32, 1), ((2, 20, 8), "plain_masked"), 11),
    ("conv_bwd-fp32mfma-concat_skip_accumulate-1x36x52", _conv_form(t_conv.test_conv_backward_fused_op_fp32, 0),
     ((1, 36, 52), "concat_skip_half_accumulate"), 11),
    ("conv_bwd-fp32mfma-concat_up_half-2x20x8", _conv_form(t_conv.test_conv_backward_fused_op_fp32, 0), ((2, 20, 8), "concat_up_half"), 7),
    ("conv_bwd-16ch-1x36x52", t_conv.test_conv_backward_fused_op_fp32_16_channels, ((1, 36, 52),), 7),
    ("conv_bwd-16ch-2x20x8", t_conv.test_conv_backward_fused_op_fp32_16_channels, ((2, 20, 8),), 7),
    ("conv_bwd-pool_scatter-1x18x28", t_conv.test_conv_backward_fused_op_fp32_pool_scatter, ((1, 18, 28), 16), 12),
    ("conv_bwd-bf16-concat_skip_accumulate-1x37x53", t_bf16.test_bf16_conv_backward_fused_op, ((1, 37, 53), "concat_skip_half_accumulate"), 5),
    ("conv_bwd-bf16-g16_x16_masked-1x37x53", t_bf16.test_bf16_conv_backward_fused_op, ((1, 37, 53), "g16_x16_masked"), 5),
    ("conv_bwd-bf16-plain_masked-2x64x64", t_bf16.test_bf16_conv_backward_fused_op, ((2, 64, 64), "plain_masked"), 5),
    ("conv_bwd-bf16-pool_scatter-1x37x53", t_bf16.test_bf16_conv_backward_fused_pool_op, ((1, 37, 53), 8), 5),
    # ---- convt2x2
    ("convt-8-3x9x21", t_ch.test_convt_fwd_dgrad_wgrad, (8, (3, 9, 21)), 6),
    ("convt-16-1x40x16", t_ch.test_convt_fwd_dgrad_wgrad, (16, (1, 40, 16)), 6),
    ("convt_bwd-8-masked-1x40x16", t_ch.test_convt_backward_fused_fp32, (8, (1, 40, 16), True), 6),
    ("convt_bwd-16-unmasked-1x40x16", t_ch.test_convt_backward_fused_fp32, (16, (1, 40, 16), False), 6),
    ("convt-bf16-8-1x11x19", t_bf16.test_bf16_convt_fwd_dgrad_wgrad_op, (8, (1, 11, 19)), 5),
    ("convt_bwd-bf16-8-3x9x21", t_bf16.test_bf16_convt_backward_fused_op, (8, (3, 9, 21)), 5),
    ("convt_bwd-bf16-16-1x40x16", t_bf16.test_bf16_convt_backward_fused_op, (16, (1, 40, 16)), 5),
    # ---- composed Up
    ("up_fwd-8-12x38-padded_rows", t_l2.test_conv3x3_up_fwd_group_vs_convt_then_conv, (8, (12, 38)), 36),
    ("up_fwd-16-20x76", t_l2.test_conv3x3_up_fwd_group_vs_convt_then_conv, (16, (20, 76)), 33),
    ("up_fwd_split-8-12x40", t_split.test_forward_split_form_composed_up_vs_convt_then_conv, (8, (12, 40)), 11),
    ("up_fwd_split-16-20x72", t_split.test_forward_split_form_composed_up_vs_convt_then_conv, (16, (20, 72)), 11),
    ("up_bwd-16-12x16", t_l2.test_conv3x3_up_bwd_group_vs_autograd, (16, (12, 16)), 40),
    ("up_bwd-8-16x24", t_l2.test_conv3x3_up_bwd_group_vs_autograd, (8, (16, 24)), 40),
    # ---- 32 x 32 level
    ("level2_fwd-one_problem", t_l2.test_level2_fwd_group_vs_torch, (1, True), 18),
    ("level2_bwd", t_l2.test_level2_bwd_group_vs_autograd, (), 36),
    ("level2_fwd-bf16-whole_level", _monkeypatched(t_bf16.test_bf16_whole_level_forward_kernel_is_bit_identical_to_the_three_launches), (), 20),
    ("level2_bwd-bf16-whole_level-B1", t_bf16.test_bf16_whole_level_backward_kernel_against_the_two_launches, (1, 1), 20),
    # ---- head
    ("head_fwd-split-sparse", _head_form(t_ch.test_head_fwd_vs_oracle, 1), (True, HEAD), 16),
    ("head_fwd-split-dense", _head_form(t_ch.test_head_fwd_vs_oracle, 1), (False, HEAD), 15),
    ("head_fwd-fp32mfma-sparse", _head_form(t_ch.test_head_fwd_vs_oracle, 0), (True, HEAD), 16),
    ("head_fwd-fp32mfma-dense", _head_form(t_ch.test_head_fwd_vs_oracle, 0), (False, HEAD), 15),
    ("head_bwd-split-sparse", _head_form(t_ch.test_head_bwd_vs_oracle_autograd, 1), (True, HEAD), 12),
    ("head_bwd-split-dense", _head_form(t_ch.test_head_bwd_vs_oracle_autograd, 1), (False, HEAD), 12),
    ("head_bwd-fp32mfma-sparse", _head_form(t_ch.test_head_bwd_vs_oracle_autograd, 0), (True, HEAD), 12),
    ("head_bwd-fp32mfma-dense", _head_form(t_ch.test_head_bwd_vs_oracle_autograd, 0), (False, HEAD), 12),
    ("head_decisions-split-sparse", _head_form(t_ch.test_head_decision_export_known_answer, 1), (True, HEAD), 4),
    ("head_decisions-fp32mfma-dense", _head_form(t_ch.test_head_decision_export_known_answer, 0), (False, HEAD), 4),
    ("head_decisions_fp64-split-dense", _head_form(t_ch.test_head_decision_export_vs_float64, 1), (False, HEAD), 4),
    ("head_decisions_fp64-fp32mfma-sparse", _head_form(t_ch.test_head_decision_export_vs_float64, 0), (True, HEAD), 4),
    ("head-bf16-sparse", t_bf16.test_bf16_head_fwd_bwd_vs_bf16_oracle_autograd, (True, HEAD), 8),
    ("head-bf16-dense", t_bf16.test_bf16_head_fwd_bwd_vs_bf16_oracle_autograd, (False, HEAD), 8),
    # ---- masks, compact / scatter, units
    ("sparsity_mask-b2_40x52", t_ch.test_sparsity_mask_bit_exact_vs_golden, ("b2_40x52",), 5),
    ("compact_masked", t_ch.test_compact_masked_order, (), 20),
    ("scatter_masked-add_padding", lambda: t_sizes.test_api_extras_add_padding_scatter_and_sparse_unet_mask(_pair()), (), 10),
    ("outconv_sigmoid_crop", t_ch.test_outconv_sigmoid_crop, (), 3),
    ("building_score_mask-regions-16", t_ch.test_building_score_mask_equals_the_two_separate_ops, ("regions", 16), 8),
    ("building_score_mask-empty_selection-2", t_ch.test_building_score_mask_equals_the_two_separate_ops, ("empty_selection", 2), 8),
    ("unit_mask-1x37x53-occupancy", t_units.test_unit_mask_bit_exact, (1, 37, 53, True), 6),
    ("unit_mask-1x37x53-no_occupancy", t_units.test_unit_mask_bit_exact, (1, 37, 53, False), 6),
    ("unit_popcount-1x37x53", t_units.test_unit_popcount_reproducible_and_bounded, (1, 37, 53), 4),
    ("unit_paint-1x37x53", t_units.test_unit_paint_and_autograd, (1, 37, 53), 4),
    ("unit_layout_device-3x5", t_un.test_unit_layout_equals_the_torch_plumbing, ("3x5_junk_padding",), 7),
    ("unit_layout_device-2x300", t_un.test_unit_layout_equals_the_torch_plumbing, ("2x300_ragged",), 7),
    ("unit_popcount_loss-257-1x37x53", t_un.test_unit_popcount_loss_is_bitwise_the_two_calls, (257, (1, 37, 53)), 12),
    # ---- ingest
    ("reflect_pad_select-3x9x12", t_conv.test_reflect_pad_select_matches_torch, ((3, 6, 9, 12, 0, 3, 4, 0),), 2),
    ("reflect_pad_select-2x20x31", t_conv.test_reflect_pad_select_matches_torch, ((2, 6, 20, 31, 3, 5, 2, 4),), 2),
    ("select_normalize_pad-2x37x52", t_l2.test_select_normalize_pad_equals_normalise_then_pad, (), 3),
    ("ingest_cl8-2x37x53-normalised", t_bf16.test_bf16_ingest_cl8_vs_torch, ((2, 37, 53), (5, 6, 2, 9), True), 2),
    ("ingest_cl8-2x37x53-raw", t_bf16.test_bf16_ingest_cl8_vs_torch, ((2, 37, 53), (5, 6, 2, 9), False), 2),
    # ---- input gradient
    ("input_grad-forced_33x20_pad14", t_ig.test_op_vs_float64, ("forced_33x20_pad14", 6), 5),
    ("input_grad-edge_16x130", t_ig.test_op_vs_float64, ("edge_16x130", 6), 5),
    ("input_grad-every_element-forced_33x20_pad14", t_ig.test_op_writes_every_element_and_is_reproducible, ("forced_33x20_pad14",), 6),
    ("input_grad-every_element-edge_16x130", t_ig.test_op_writes_every_element_and_is_reproducible, ("edge_16x130",), 6),
    ("input_grad-row_strided", t_ig.test_op_row_strided_gradient, (), 5),
    ("input_grad-bf16-forced_33x20_pad14", t_ig.test_op_bf16_vs_float64, ("forced_33x20_pad14", 6), 5),
    ("input_grad-bf16-cx2-forced_33x20_pad14", t_ig.test_op_bf16_vs_float64, ("forced_33x20_pad14", 2), 3),
    ("input_grad-bf16-edge_16x130", t_ig.test_op_bf16_vs_float64, ("edge_16x130", 6), 5),
    # ---- train tail
    ("loss-B257-mix", t_tail.test_loss_kernel_vs_float64, (257, "mix"), 30),
    ("loss-B2-log_l1", t_tail.test_loss_kernel_vs_float64, (2, "log_l1"), 30),
    ("head_popcount_loss-split-3x16x16", t_tail.test_popcount_reduce_deferred_equals_two_launch, (3, 16, 16, 1), 20),
    ("head_popcount_loss-fp32mfma-3x16x16", t_tail.test_popcount_reduce_deferred_equals_two_launch, (3, 16, 16, 0), 20),
    ("adam-n28672", t_tail.test_adam_size_sweep, (28672,), 70),
    ("adam-n28676", t_tail.test_adam_size_sweep, (28676,), 70),
    ("adam-n5", t_tail.test_adam_size_sweep, (5,), 70),
    # ---- nan_fill_, block_sum, census_paint, augment_raw
    ("nan_fill-4x37x53", t_nan.test_op_vs_oracle_bit_exact, ((4, 37, 53), 0.3, 3), 1),
    ("nan_fill-ragged_extents", t_nan.test_batched_ragged_extents, (), 1),
    ("block_sum-cell3", t_prod.test_block_sum_exact, (3,), 2),
    ("block_sum-cell10", t_prod.test_block_sum_exact, (10,), 2),
    ("census_paint-K1", t_census.test_paint_equals_gather, (1,), 3),
    ("census_paint-K3", t_census.test_paint_equals_gather, (3,), 3),
    ("augment_raw-rot1_rot3-non_square", t_feed.test_augment_raw_rotation_direction_known_answer, (), 14),
    # ---- census.hip: stitcher (accumulate + finalize, windows that stick out on every side), segment sum (all 16 alignment phases)
    ("stitcher-exact-M2-some_without_scale", t_ev.test_stitcher_exact_known_answer.body, (2, "some"), 20),
    ("segment_sum-4097ids-n4099", t_ev.test_segment_sum_exact_at_every_alignment_phase.body, (4097, 4099), 50),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_family_under_poisoned_guard_bands(case):
    name, fn, args, least = case
    with fresh_workspaces():
        with FP.Footprint("cuda", fill=FP.POISON) as fp:
            fn(*args)
    print(f"\n[footprint] {name}: {fp.guarded} guarded allocations, bands intact")
    assert fp.guarded >= least, (name, fp.guarded, least)


def test_harness_notices_a_one_element_overrun_on_the_device():
    """the self-test of tests/test_footprint_cpu.py with a torch op on the device: ``as_strided`` writes one element into the harness's
    own band on either side of a tensor (nothing leaves memory the harness allocated)"""
    for side in ("before", "after"):
        with pytest.raises(FP.FootprintError) as e:
            with FP.Footprint("cuda") as fp:
                t = torch.zeros(4, 6, device="cuda")
                r = fp.records[0]
                first = r.lo // 4
                r.raw.view(torch.float32).as_strided((1,), (1,), first - 1 if side == "before" else first + 24).fill_(1.0)
                assert t.data_ptr() % 512 == 0 and bool((t == 0).all())
        msg = str(e.value)
        assert f"band {side} the payload" in msg and "(4, 6)" in msg and ("offset -4 " if side == "before" else "offset +0 ") in msg
    with FP.Footprint("cuda") as fp:
        a = torch.empty(3, 8, 5, 7, device="cuda", dtype=torch.bfloat16, memory_format=torch.channels_last)
        b = torch.randn(2, 3, 5, 8)[..., :7].cuda()
        assert fp.guarded == 2
        assert bool(torch.isnan(a.float()).all()) and a.stride() == (280, 1, 56, 8) and b.shape == (2, 3, 5, 7)


# ---- grouped data gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 29, 47), (2, 32, 64)])            # ragged: scalar epilogues; aligned: the 16-byte ones
@pytest.mark.parametrize("mode", ["plain", "masked_accumulate", "pool_scatter"])
def test_conv_dgrad_group_of_two_is_bitwise_two_single_launches(shape, mode):
    """ops.conv3x3_dgrad_group has no op-level case with more than one problem (the single op is its group of one and is held to
    autograd by test_conv_dgrad_plain_and_masked / test_conv_dgrad_pool_scatter_matches_autograd at these shapes): two problems of one
    launch -- the two column blocks of a 16-channel concat layer (c0_add), or two pool-scatter layers -- against one launch each, bit
    for bit, between the bands."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    B, H, W = shape
    pool, acc = mode == "pool_scatter", mode != "plain"
    gh, gw, cg = (H // 2, W // 2, 16) if pool else (H, W, 8)
    with fresh_workspaces():
        with FP.Footprint("cuda", fill=FP.POISON) as fp:
            shared_w = t_conv._mk(cg, 16, 3, 3, seed=1, scale=0.2).cuda()
            single, group, keep = [], [], []
            for i in range(2):
                g = t_conv._mk(B, cg, gh, gw, seed=10 + i).cuda()
                w = t_conv._mk(cg, 8, 3, 3, seed=2 + i, scale=0.2).cuda() if pool else shared_w
                act = bn = None
                if acc:
                    act = F.relu(t_conv._mk(B, 8, H, W, seed=20 + i)).cuda()
                    keep.append([t.cuda() for t in t_conv._bn_params(8, 30 + i)])
                    bn = L.bn(None, *keep[-1])
                outs = [t_conv._mk(B, 8, H, W, seed=40 + i).cuda() if acc else torch.full((B, 8, H, W), float("nan"), device="cuda")
                        for _ in range(2)]
                c0 = 0 if pool else 8 * i
                ops.conv3x3_dgrad(g, w, c0, 8, outs[0], act=act, act_bn=bn, pool=pool, accumulate=acc)
                single.append(outs[0])
                group.append({"g": g, "w": w, "out": outs[1], "act": act, "act_bn": bn, "c0_add": c0})
            ops.conv3x3_dgrad_group(group, 0, 8, pool=pool, accumulate=acc)
            torch.cuda.synchronize()
            # per problem: gradient, two outputs (+ activation and four BN vectors where masked; + its own weight in the pool form)
            assert fp.guarded >= {"plain": 1 + 2 * 3, "masked_accumulate": 1 + 2 * 8, "pool_scatter": 2 * 9}[mode]
    for i in range(2):
        assert bool(torch.isfinite(single[i]).all()) and float(single[i].abs().max()) > 0
        assert FP.bit_equal(group[i]["out"], single[i]), (mode, i)
    assert not FP.bit_equal(single[0], single[1])


# ---- ops.ingest_split ------------------------------------------------------------------------------------------------------------------
C2, C1 = 4, 2
BAND = [4, 1, 5, 0, 3, 2]                      # indexes [s2 | s1]: S1, S2, S1, S2, S2, S2 -- the two sources interleaved
MEAN = [-11.5, 1102.25, -18.75, 987.5, 2890.0, 1314.125]
STD = [4.25, 611.5, 5.125, 587.75, 1203.0, 702.5]
EDGE_DN = (0, 32767, 32768, 65535)             # a signed 16-bit conversion turns the last two negative


def _split_case(shape, seed):
    B, H, W = shape
    rng = np.random.default_rng(seed)
    dn = rng.integers(0, 65536, size=(B, C2, H, W), dtype=np.int64)
    flat = dn.reshape(-1)
    where = rng.choice(flat.size, size=4 * len(EDGE_DN), replace=False)
    flat[where] = np.tile(np.array(EDGE_DN), 4)
    for c in range(C2):                                                  # and every band holds every edge value at the image corners
        dn[0, c, 0, 0], dn[0, c, 0, W - 1], dn[0, c, H - 1, 0], dn[0, c, H - 1, W - 1] = np.roll(np.array(EDGE_DN), c)
    s2 = torch.from_numpy(dn.astype(np.int32)).to(torch.uint16)
    s1 = torch.from_numpy((rng.standard_normal((B, C1, H, W)) * 4 - 12).astype(np.float32))
    return s2, s1, torch.from_numpy(dn).double()


@pytest.mark.parametrize("shape,pads", [((2, 37, 53), (5, 6, 2, 9)), ((3, 9, 12), (0, 3, 4, 0))])
def test_ingest_split_both_forms_vs_float64_and_its_sibling_kernels(shape, pads):
    """pc_ingest_split (uint16 S2 digital numbers + fp32 S1 -> the padded, normalised, stream-ordered model input) against float64
    ((x - mean) / std) of the reflect-padded selection, mean and std being the fp32 numbers the kernel receives.  Bars from the formats:
    planar fp32 (24 significant bits, unit roundoff u = 2^-24) -- one rounding of the difference and one of the quotient:
    (1 + u)^2 - 1 < 2^-23 (1 + 2^-20) relative; channels-last bf16 -- the same fp32 value rounded once more to 8 significant bits
    (unit roundoff 2^-8): 2^-8 + 2^-22 relative; slots 6 and 7 zero.
    Bit-equality with the kernels the step otherwise uses on the same values held as fp32: select_normalize_pad (planar), ingest_cl8."""
    from popcorn_amd import ops
    top, bottom, left, right = pads
    s2, s1, dn64 = _split_case(shape, seed=shape[1])
    assert all(bool((s2.to(torch.int32) == v).any()) for v in EDGE_DN)
    both = torch.cat([dn64, s1.double()], 1)
    mean32 = torch.tensor(MEAN, dtype=torch.float32).double().view(1, -1, 1, 1)
    std32 = torch.tensor(STD, dtype=torch.float32).double().view(1, -1, 1, 1)
    ref = (F.pad(both[:, BAND], (left, right, top, bottom), mode="reflect") - mean32) / std32
    raw32 = torch.cat([dn64.float(), s1], 1)                             # every uint16 is an fp32 number
    with fresh_workspaces():
        with FP.Footprint("cuda", fill=FP.POISON) as fp:
            s2d, s1d, rawd = fp.place(s2), fp.place(s1), fp.place(raw32)
            planar = ops.ingest_split(s2d, s1d, BAND, MEAN, STD, top, bottom, left, right, cl8=False)
            cl8 = ops.ingest_split(s2d, s1d, BAND, MEAN, STD, top, bottom, left, right, cl8=True)
            sib_planar = ops.select_normalize_pad(rawd, BAND, MEAN, STD, top, bottom, left, right)
            sib_cl8 = ops.ingest_cl8(rawd, BAND, MEAN, STD, top, bottom, left, right)
            assert fp.guarded >= 7
    B, H, W = shape
    assert planar.dtype == torch.float32 and tuple(planar.shape) == (B, 6, H + top + bottom, W + left + right) and planar.is_contiguous()
    assert cl8.dtype == torch.bfloat16 and tuple(cl8.shape) == (B, 8, H + top + bottom, W + left + right) and cl8.stride(1) == 1
    e32 = ((planar.cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    e16 = ((cl8[:, :6].cpu().double() - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    bar32, bar16 = 2.0 ** -23 * (1 + 2.0 ** -20), 2.0 ** -8 + 2.0 ** -22
    print(f"\n[ingest_split] {shape} pads {pads}: planar {e32:.3e} (bar {bar32:.3e}), cl8 {e16:.3e} (bar {bar16:.3e})")
    assert bool(torch.isfinite(planar).all()) and e32 <= bar32
    assert bool(torch.isfinite(cl8.float()).all()) and e16 <= bar16
    assert not cl8[:, 6:].any()
    assert FP.bit_equal(planar, sib_planar)
    assert FP.bit_equal(cl8, sib_cl8)
