"""Entry-point counterparts of the reference's ``run_train.py`` / ``run_eval.py`` (same flag names and defaults as
arguments/train.py:10-60 and arguments/eval.py:4-26; argparse instead of configargparse, JSONL instead of wandb).

Order of operations of the training loop is the reference's (run_train.py:146-269):
  to_device -> normalise (+ augment) -> limit1/2/3 gating -> forward(train, padding=False, sparse=True) -> get_loss ->
  x lam_weak -> backward -> clip_grad_norm_(gradient_clip) -> Adam step -> zero_grad; StepLR per epoch; checkpoint dict
  {'model','epoch','iter','optimizer','scheduler'} in ``<save_dir>/experiment_*/last_model.pth`` (:445-456).
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import random
import time

import numpy as np
import torch

from . import ops
from .data import stats
from .data.collate import Population_Dataset_collate_fn
from .data.dataset import TEST_RASTER_REGIONS, SyntheticTestRaster, SyntheticWeaksupDataset
from .data.feed import RegionFeed
from .distributed import FlatReducer, init_from_env
from .model import get_model_kwargs, model_dict
from .utils.transform import default_train_transform


class _OneOrMany(argparse.Action):
    """nargs="+" whose single value stays the scalar it always was (--resident_units 24 -> 24, --resident_units 24 30 -> [24, 30])"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values[0] if len(values) == 1 else list(values))


def train_parser():
    p = argparse.ArgumentParser(description="Training Population Estimation (MI355X)")
    p.add_argument("-r", "--resume", type=str)
    p.add_argument("-treg", "--target_regions", nargs="+", default=["pri2017"])
    p.add_argument("-tregtrain", "--target_regions_train", nargs="+", default=["pri2017"])
    p.add_argument("-S1", "--Sentinel1", action="store_true")
    p.add_argument("-S2", "--Sentinel2", action="store_true")
    p.add_argument("-NIR", "--NIR", action="store_true")
    p.add_argument("-wb", "--weak_batch_size", type=int, default=2)
    p.add_argument("-wvb", "--weak_val_batch_size", type=int, default=1)
    p.add_argument("-pret", "--pretrained", action="store_true")
    p.add_argument("-m", "--model", type=str, default="POPCORN")
    p.add_argument("-binit", "--biasinit", type=float, default=0.75)
    p.add_argument("-occmodel", "--occupancymodel", action="store_true")
    p.add_argument("-binp", "--buildinginput", action="store_true")
    p.add_argument("-sinp", "--segmentationinput", action="store_true")
    p.add_argument("-senbuilds", "--sentinelbuildings", action="store_true")
    p.add_argument("-fe", "--feature_extractor", type=str, default="DDA")
    p.add_argument("-e", "--num_epochs", type=int, default=100)
    p.add_argument("-lr", "--learning_rate", type=float, default=1e-4)
    p.add_argument("-l", "--loss", nargs="+", default=["log_l1_loss"])
    p.add_argument("-sreg", "--scale_regularization", default=0.01, type=float)
    p.add_argument("-la", "--lam", nargs="+", type=float, default=[1.0])
    p.add_argument("-lw", "--lam_weak", type=float, default=100.0)
    p.add_argument("-lim1", "--limit1", type=int, default=9000000)
    p.add_argument("-lim2", "--limit2", type=int, default=9000000)
    p.add_argument("-lim3", "--limit3", type=int, default=13000000)
    p.add_argument("-wd", "--weightdecay", type=float, default=0.0)
    p.add_argument("-lrs", "--lr_step", type=int, default=5)
    p.add_argument("-lrg", "--lr_gamma", type=float, default=0.75)
    p.add_argument("-gc", "--gradient_clip", type=float, default=0.01)
    p.add_argument("--save_dir", default="outputs")
    p.add_argument("-w", "--num_workers", type=int, default=0)
    p.add_argument("-lt", "--logstep_train", type=int, default=25)
    p.add_argument("-val", "--val_every_n_epochs", type=int, default=2)
    p.add_argument("-wv", "--weak_validation", action="store_true")
    p.add_argument("-testi", "--test_every_i_steps", type=int, default=500000)
    p.add_argument("-vi", "--val_every_i_steps", type=int, default=500000)
    p.add_argument("--seed", type=int, default=1600)
    p.add_argument("--save-model", default="both", choices=["last", "best", "no", "both"])
    p.add_argument("-mws", "--max_weak_samples", type=int, default=None)
    # build-specific
    p.add_argument("--synthetic_regions", type=int, default=64, help="size of the synthetic weaksup dataset")
    p.add_argument("--synthetic_hw_range", type=int, nargs=2, default=[64, 144],
                   help="side range (pixels) of the synthetic census-region crops; the reference's regions reach ~3000 px sides (limit1 = 9e6 px per batch)")
    p.add_argument("--fixed_hw", type=int, nargs=2, default=None, help="fixed crop size (enables HIP-graph replay)")
    p.add_argument("--torch_optimizer", action="store_true",
                   help="reference recipe through torch autograd + torch.optim.Adam instead of the fused HIP step")
    p.add_argument("--max_steps", type=int, default=None)
    p.add_argument("--synthetic_val_regions", type=int, default=16, help="size of the synthetic weak-validation set")
    p.add_argument("--test_raster_hw", type=int, nargs=2, default=[384, 448], help="synthetic target-test raster (test_target)")
    p.add_argument("--test_patchsize", type=int, default=256)
    p.add_argument("--test_overlap", type=int, default=32)
    p.add_argument("--precision", choices=["fp32", "bf16"], default="fp32",
                   help="bf16: mixed precision (bf16 MFMA operands + channels-last bf16 activations, fp32 master weights; DESIGN.md 7)")
    p.add_argument("--nan_fill", action="store_true",
                   help="nearest-value NaN fill of S2 / S1 on the device before augmentation and normalisation (on for real rasters: "
                        "cloud masks, orbit gaps; data/PopulationDataset.py:419-441)")
    p.add_argument("--nan_clouds", type=float, default=0.0,
                   help="synthetic datasets: NaN cloud discs over about this fraction of S2, orbit gaps in S1 (pair with --nan_fill)")
    p.add_argument("--ascfill", action="store_true", help="always take the ascending S1 where the descending one holds NaNs")
    p.add_argument("--units_per_crop", type=int, default=0,
                   help="multi-unit census supervision: train on synthetic crops that list this many census units each (all of them "
                        "supervised in one eager step; 0 = off, the reference's one unit per sample)")
    p.add_argument("--native_units", action="store_true",
                   help="--units_per_crop steps through the native step executor (pc_train_step_units: one call per step, the same "
                        "bits as the per-launch engine); experimental, off by default")
    p.add_argument("--native_layer", action="store_true",
                   help="--building_layer steps (and steps of a model without -occmodel) through the native step executor "
                        "(pc_train_step_layer: one call per step, the same bits as the per-launch engine); experimental, off by default; "
                        "no effect on steps the executor takes anyway")
    p.add_argument("--native_single", action="store_true",
                   help="steps of a single-modality model (-S1 alone, or -S2 alone) through the native step executor (a one-stream plan: "
                        "one call per step, the same bits as the per-launch engine); off by default.  Needs exactly one of -S1 / -S2, "
                        "--precision fp32 and the fused step (no --torch_optimizer)")
    p.add_argument("--native_forward", action="store_true",
                   help="validate_weak and the target test (--resident_val / --resident_test included) run model(sample, padding=False) "
                        "through the native forward executor (pc_forward: one call per forward, the same bits as the per-launch engine); "
                        "off by default.  Still declined: --precision bf16, -S1 alone, -S2 alone (--native_single is the training "
                        "executor's switch, not this one's) and multi-unit validation items keep the per-launch engine -- the count "
                        "printed at the end is then 0")
    p.add_argument("--device_units", action="store_true",
                   help="--units_per_crop steps in the device-N form (counts, N and 1 / N read from device memory): allowed with --fixed_hw "
                        "(replayed HIP graph) and under data parallelism; implies nothing without --units_per_crop")
    p.add_argument("--resident_region", type=int, nargs="+", default=None, metavar=("H", "W"),
                   help="region-resident training: a synthetic H x W raw raster stays on the device and every batch of census-unit crops "
                        "is one gather launch (data/region.py); one unit per crop, or --units_per_crop K complete units per crop.  "
                        "2 * R integers: R rasters (region k seeded --seed + 20 + k) form a resident atlas (data/atlas.py) -- the "
                        "reference's multi-country -tregtrain -- and a batch is still one launch whichever regions its crops come from")
    p.add_argument("--resident_units", type=int, nargs="+", default=400, action=_OneOrMany,
                   help="--resident_region: census units of the synthetic raster; one value, or one per region")
    p.add_argument("--resident_ascfill", type=int, nargs="+", default=None, metavar="K",
                   help="--resident_region: the regions (0-based) whose repair, validation and test plans take the ascending S1 wherever "
                        "the descending one holds NaN -- the reference's need_asc; --ascfill keeps meaning all regions; needs "
                        "--resident_repair, --resident_val or --resident_test (a plan that takes it)")
    p.add_argument("--max_weak_pix", type=int, default=10_000_000,
                   help="--resident_region: census units with at least this many pixels are dropped (the reference's max_pix)")
    p.add_argument("--max_pix_box", type=int, default=12_000_000,
                   help="--resident_region: units whose bounding box has at least this many pixels are dropped; the pixel budget of a "
                        "multi-unit crop (the reference's max_pix_box)")
    p.add_argument("--resident_assemble", action="store_true",
                   help="--resident_region: gather, augmentation, raw tile and labels of a batch in ONE launch (data/region.py: "
                        "ResidentBatchFeed) instead of gather + augment_raw + torch indexing; the same batches and bits")
    p.add_argument("--resident_pixel_budget", type=int, default=0, metavar="P",
                   help="--resident_region: implies --resident_assemble and composes batches by crop size so that B * Hm * Wm <= P "
                        "(plan_batches) instead of cutting them at -wb; variable batch size, NOT the reference recipe (0 = off)")
    p.add_argument("--resident_max_batch", type=int, default=128, help="--resident_pixel_budget: at most this many crops per batch")
    p.add_argument("--resident_min_fill", type=float, default=0.6,
                   help="--resident_pixel_budget: a batch of more than one crop keeps real pixels / padded pixels at or above this")
    p.add_argument("--resident_repair", action="store_true",
                   help="--resident_region: the reference's per-item NaN repair planned ONCE (data/region.py: plan_repair) -- the S1 orbit of "
                        "every crop from one census pass (--ascfill as the reference's), the repaired sites as a patch table on the device, "
                        "one small launch per batch and no per-step fill; works with every resident feed (pair with --nan_clouds / "
                        "--resident_s1_gap)")
    p.add_argument("--resident_s1_gap", type=float, default=0.0, metavar="F",
                   help="--resident_repair: orbit-gap rows over this fraction of the synthetic raster's descending S1")
    p.add_argument("--resident_test", action="store_true",
                   help="--resident_region: the in-training target test evaluates the resident region itself (--test_patchsize / "
                        "--test_overlap) through data/region.py: ResidentWindows -- orbit and NaN repair of every window planned at the "
                        "first test and reused by every later one, one launch per window, no per-window fill; keeps the ascending S1 "
                        "resident as --resident_repair does")
    p.add_argument("--resident_seasons", type=int, default=1, metavar="S",
                   help="--resident_region: the synthetic raster holds S seasons and the resident feeds, --resident_repair and "
                        "--resident_val draw every item's season from them (the reference trains and validates across four); "
                        "--resident_test keeps evaluating season 0")
    p.add_argument("--resident_val", action="store_true",
                   help="--resident_region: the reference's -wv split on the resident raster -- the census rows are shuffled once "
                        "(random_state 1610), the run trains on the first 80 %% and validate_weak runs over the other 20 %% through "
                        "data/region.py: ResidentItems (season, orbit and NaN repair of every item planned once, one launch per item, no "
                        "per-item fill or synchronisation); needs -wvb 1; keeps the ascending S1 resident as --resident_repair does")
    p.add_argument("--building_layer", action="store_true",
                   help="the dataset ships a building layer (the reference's path whenever -senbuilds is absent: Google Open Buildings / "
                        "swissTLM3D counts): the synthetic host datasets, the resident region and the test raster carry a seeded layer and "
                        "every step, validation and target test multiplies the occupancy head by it instead of running the frozen "
                        "extractor; refused together with -senbuilds (the reference's dataset loads no layer then)")
    return p


def eval_parser():
    p = argparse.ArgumentParser(description="Ensemble evaluation (MI355X)")
    p.add_argument("-r", "--resume", nargs="+", type=str, default=[])
    p.add_argument("-treg", "--target_regions", nargs="+", default=["pri2017"])
    p.add_argument("-S1", "--Sentinel1", action="store_true")
    p.add_argument("-S2", "--Sentinel2", action="store_true")
    p.add_argument("-NIR", "--NIR", action="store_true")
    p.add_argument("-m", "--model", type=str, default="POPCORN")
    p.add_argument("-binit", "--biasinit", type=float, default=0.75)
    p.add_argument("-occmodel", "--occupancymodel", action="store_true")
    p.add_argument("-senbuilds", "--sentinelbuildings", action="store_true")
    p.add_argument("-pret", "--pretrained", action="store_true")
    p.add_argument("-fe", "--feature_extractor", type=str, default="DDA")
    p.add_argument("--fourseasons", action="store_true")
    p.add_argument("--save_dir", default="outputs")
    p.add_argument("--seed", type=int, default=1610)
    p.add_argument("--raster_hw", type=int, nargs=2, default=[2304, 2560])
    p.add_argument("--patchsize", type=int, default=2048)
    p.add_argument("--overlap", type=int, default=128)
    p.add_argument("--ensemble", type=int, default=1, help="members to instantiate when no --resume checkpoints are given")
    p.add_argument("--precision", choices=["fp32", "bf16"], default="fp32", help="arithmetic mode of the kernels (DESIGN.md 7)")
    p.add_argument("--native_forward", action="store_true",
                   help="every member's window forward through the native forward executor (pc_forward: one call per window and member, "
                        "the same bits as the per-launch engine); off by default.  Still declined, as by the training executor: "
                        "--precision bf16, -S1 alone, -S2 alone keep the per-launch engine -- the count printed at the end is then 0")
    p.add_argument("--raw_input", action="store_true",
                   help="un-normalised S2 / S1 windows, NaN-filled on the device per window before normalisation (real rasters)")
    p.add_argument("--nan_clouds", type=float, default=0.0, help="--raw_input: NaN cloud discs over about this fraction of S2")
    p.add_argument("--s1_gap", type=float, default=0.0, help="--raw_input: orbit-gap rows over this fraction of the descending S1")
    p.add_argument("--ascfill", action="store_true", help="always take the ascending S1 where the descending one holds NaNs")
    p.add_argument("--resident_windows", action="store_true",
                   help="the raw raster stays on the device as a resident region and the sliding windows are planned once "
                        "(data/region.py: ResidentWindows): orbit choice and NaN repair of every window from one census pass and a patch "
                        "table, then one launch per window with no fill and no synchronisation; the same maps and metrics as --raw_input "
                        "(takes --nan_clouds / --s1_gap / --ascfill / --fourseasons; not together with --raw_input)")
    p.add_argument("--product_cell", type=int, default=0,
                   help="side in pixels of the product grid the 10 m maps are aggregated to on the device (0 = off; 10 = the hectare grid "
                        "the reference recommends for the final product and for evaluation)")
    p.add_argument("--product_out", type=str, default=None,
                   help="--product_cell: torch.save the product {mean, std, adjusted, cell} here (rank 0)")
    p.add_argument("--census_table", action="store_true",
                   help="accumulate every member's census-unit totals on the device while stitching and report the census metrics of "
                        "the ensemble mean with their spread over members (<key>_members_mean / <key>_members_std)")
    p.add_argument("--census_out", type=str, default=None,
                   help="--census_table: torch.save {totals, mean, std, num_ids[, details]} here (rank 0)")
    p.add_argument("--census_details", action="store_true",
                   help="--census_table: also paint the reference's six per-unit detail maps (+ totals_std) into --census_out")
    p.add_argument("--coarse_regions", type=int, default=0,
                   help="a second, coarser census level of about N units (blocks of fine units; N >= 2, fewer than the fine units): the map "
                        "is adjusted to the COARSE census and judged on both levels (AdjCensus_synthetic_fine is then the disaggregation "
                        "result); with --census_table the adjusted fine totals come from the table as well, per member "
                        "(TableAdjCensus_synthetic_fine + _members_mean / _members_std; --census_out gains adjusted / adjusted_std)")
    p.add_argument("--building_layer", action="store_true",
                   help="the test raster ships a building layer (the reference's path whenever -senbuilds is absent): every window's sample "
                        "carries building_counts and no member runs its frozen extractor; with --resident_windows the layer stays resident "
                        "and comes out of each window's own launch; refused together with -senbuilds")
    return p


def check_building_layer(args):
    """--building_layer -senbuilds: the reference's dataset loads no layer for a model that scores buildings itself
    (PopulationDataset.py:606-612 under ``not sentinelbuildings``), and its model would ignore one (popcorn.py:112-114)."""
    if args.building_layer and args.sentinelbuildings:
        raise SystemExit("--building_layer ships a building layer for a model built WITHOUT -senbuilds; with -senbuilds the reference's "
                         "dataset loads no layer and the model ignores one: drop --building_layer or -senbuilds")


def check_native_single(args):
    """--native_single: the refusals that need no device, raised before anything else is set up."""
    if not getattr(args, "native_single", False):
        return
    if bool(args.Sentinel1) == bool(args.Sentinel2):
        raise SystemExit("--native_single sends the steps of a single-modality model through the native executor: it needs exactly one of "
                         "-S1 / -S2 (a model with both takes the executor without it)")
    if args.precision == "bf16":
        raise SystemExit("--native_single: the native executor is fp32 only; --precision bf16 keeps the per-launch engine (drop one of the two)")
    if args.torch_optimizer:
        raise SystemExit("--native_single belongs to the fused step: the --torch_optimizer recipe never reaches the native executor")


def seed_all(seed):
    """utils/utils.py:50-59."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


def new_log(folder, args=None):
    """utils/utils.py:62-73."""
    os.makedirs(folder, exist_ok=True)
    n_exp = len(os.listdir(folder))
    randn = round((time.time() * 1000000) % 1000)
    exp = os.path.join(folder, f"experiment_{n_exp}_{randn}")
    os.makedirs(exp, exist_ok=True)
    if args is not None:
        with open(os.path.join(exp, "args.csv"), "w") as fh:
            fh.write("key,value\n")
            for k, v in vars(args).items():
                fh.write(f"{k},{v}\n")
    return exp


def fill_sample_(s2, s1, sample):
    """--nan_fill: the nearest-value fill (data/PopulationDataset.py:526-551) of the batch's device S2 / S1 in place, each item over its
    own extent (the collate's ``data_hw``): the zero padding of a smaller region is never a source."""
    hw = sample.get("data_hw")
    ops.nan_fill_(s2, hw)
    ops.nan_fill_(s1, hw)


def normalize_sample(sample, device, transform=None, nan_fill=False):
    """to_cuda_inplace + apply_transformations_and_normalize (utils/utils.py:22-43,130-214) on the device: S2 augmentations
    on the raw digital numbers, per-band normalisation + concat [S2, S1] (one HIP kernel), then the joint geometric
    transform of input and admin_mask.  nan_fill: ``fill_sample_`` first."""
    s2, s1 = sample["S2"].to(device, non_blocking=True).float(), sample["S1"].to(device, non_blocking=True).float()
    if nan_fill:
        s2, s1 = s2.contiguous(), s1.contiguous()
        fill_sample_(s2, s1, sample)
    if transform is not None and "S2" in transform:
        s2 = transform["S2"](s2)
    raw = torch.cat([s2, s1], 1).contiguous()
    x = ops.select_normalize(raw, (0, 1, 2, 3, 4, 5), stats.MEAN6, stats.STD6)
    admin = sample["admin_mask"].to(device).float()
    # a shipped building layer is stacked with the admin mask and turned / flipped with it (utils/utils.py:182-209); no value transform
    layer = sample.get("building_counts")
    if layer is not None:
        layer = layer.to(device).float()
    if transform is not None and "general" in transform:
        stack = admin.unsqueeze(1) if layer is None else torch.cat([admin.unsqueeze(1), layer], 1)
        x, m = transform["general"]((x, stack))
        admin = m[:, 0]
        if layer is not None:
            layer = m[:, 1:2]
    out = {"input": x.contiguous(), "admin_mask": admin.contiguous(),
           "census_idx": sample["census_idx"].to(device).contiguous(), "y": sample["y"].to(device).float().contiguous()}
    if layer is not None:
        out["building_counts"] = layer.contiguous()
    return out


def prepare_sample_fused(sample, transform=None, nan_fill=False):
    """The fast form of ``normalize_sample`` for the fused step (round 6): ``sample`` holds DEVICE tensors (``data.feed.RegionFeed``); the
    augmentation parameters are drawn on the host with the reference's generator consumption (``draw_fused_params``), ONE launch
    (``ops.augment_raw``) applies them while it assembles the raw [S2 | S1] tile, and the normalisation happens inside the step's ingest
    (the executor's ``raw`` input form) -- no ``.float()`` / ``torch.cat`` / normalise / flip / rot90 launches, no synchronous copy.
    Returns None when ``transform`` is not the reference trainer's set (the caller then takes ``normalize_sample``).
    nan_fill: ``fill_sample_`` on the staged tensors first.  A shipped ``building_counts`` (B, 1, H, W) goes through the same launch under
    the admin mask's map and is returned."""
    from .utils.transform import draw_fused_params
    s2, s1, admin = sample["S2"], sample["S1"], sample["admin_mask"]
    if not (s2.is_cuda and s2.dtype == torch.float32 and s1.dtype == torch.float32 and s2.shape[1] == 4 and s1.shape[1] == 2):
        return None
    params = draw_fused_params(transform)
    if params is None:
        return None
    if nan_fill:
        s2, s1 = s2.contiguous(), s1.contiguous()
        fill_sample_(s2, s1, sample)
    layer = sample.get("building_counts")
    if layer is not None:
        if not (layer.is_cuda and layer.dtype == torch.float32):
            return None
        raw, adm, bc = ops.augment_raw(s2.contiguous(), s1.contiguous(), admin.float().contiguous(), params, buildings=layer.contiguous())
        return {"raw": raw, "admin_mask": adm, "census_idx": sample["census_idx"].contiguous(), "y": sample["y"].float().contiguous(),
                "building_counts": bc}
    raw, adm = ops.augment_raw(s2.contiguous(), s1.contiguous(), admin.float().contiguous(), params)
    return {"raw": raw, "admin_mask": adm, "census_idx": sample["census_idx"].contiguous(), "y": sample["y"].float().contiguous()}


def limit_regime(num_pix, limit1, limit2, limit3):
    """The memory-driven truncation of the backward pass by batch size in pixels (run_train.py:191-198; defaults
    arguments/train.py:34-36: 9e6 / 9e6 / 13e6): (encoder_no_grad, unet_no_grad, skip the batch).  The limits nest like the
    reference's ifs: limit2 / limit3 only apply beyond limit1 / limit2."""
    enc_ng = unet_ng = skip = False
    if num_pix > limit1:
        enc_ng = True
        if num_pix > limit2:
            unet_ng = True
            if num_pix > limit3:
                skip = True
    return enc_ng, unet_ng, skip


def resident_shapes(args):
    """--resident_region as [(H, W)] * R, --resident_units as R values: SystemExit for an odd count or a list of another length."""
    v = list(args.resident_region)
    if len(v) < 2 or len(v) % 2:
        raise SystemExit(f"--resident_region takes H W per region (2 * R integers), got {len(v)}: {v}")
    shapes = [(int(v[2 * k]), int(v[2 * k + 1])) for k in range(len(v) // 2)]
    u = args.resident_units
    units = [int(x) for x in u] if isinstance(u, (list, tuple)) else [int(u)]
    if len(units) == 1:
        units = units * len(shapes)
    if len(units) != len(shapes):
        raise SystemExit(f"--resident_units takes one value or one per region ({len(shapes)}), got {len(units)}")
    return shapes, units


def check_repair_args(args):
    """The refusals of --resident_repair and its companions that need no device: raised before anything else is set up."""
    if args.resident_region is not None:
        shapes, _ = resident_shapes(args)
        from ._lib import PC_ATLAS_MAX_REGIONS
        if len(shapes) > PC_ATLAS_MAX_REGIONS:
            raise SystemExit(f"--resident_region: an atlas holds at most {PC_ATLAS_MAX_REGIONS} regions, got {len(shapes)}")
    if getattr(args, "resident_ascfill", None) is not None:
        if args.resident_region is None:
            raise SystemExit("--resident_ascfill names regions of a resident atlas: it needs --resident_region")
        if not (args.resident_repair or args.resident_val or args.resident_test):
            raise SystemExit("--resident_ascfill chooses the S1 orbit in a region's repair, validation and test plans: without "
                             "--resident_repair, --resident_val or --resident_test no plan takes it")
        bad = [k for k in args.resident_ascfill if not 0 <= k < len(shapes)]
        if bad:
            raise SystemExit(f"--resident_ascfill names regions in [0, {len(shapes)}), got {bad}")
    if args.resident_repair and args.resident_region is None:
        raise SystemExit("--resident_repair plans the NaN repair of a resident crop plan (orbit column and patch table on the device): it "
                         "needs --resident_region")
    if args.resident_s1_gap and not args.resident_repair:
        raise SystemExit("--resident_s1_gap cuts orbit gaps that only the orbit choice of --resident_repair answers: it needs "
                         "--resident_repair")
    if not 0.0 <= args.resident_s1_gap <= 1.0:
        raise SystemExit("--resident_s1_gap is a fraction of the raster's rows in [0, 1]")
    if args.resident_test and args.resident_region is None:
        raise SystemExit("--resident_test evaluates the resident region itself in the in-training target test (windows planned once on "
                         "the device): it needs --resident_region")
    if args.resident_seasons != 1 and args.resident_region is None:
        raise SystemExit("--resident_seasons sets how many seasons the resident raster holds and its feeds draw from: it needs "
                         "--resident_region")
    if args.resident_seasons < 1:
        raise SystemExit("--resident_seasons is a number of seasons >= 1")
    if args.resident_val and args.resident_region is None:
        raise SystemExit("--resident_val splits the census rows of the resident raster into a training and a validation plan (items "
                         "planned once on the device): it needs --resident_region")
    if args.resident_val and args.weak_val_batch_size != 1:
        raise SystemExit(f"--resident_val validates item by item (padding makes an item's result depend on its batch): -wvb must be 1, got "
                         f"{args.weak_val_batch_size}")


def check_eval_args(args):
    """The refusals of run_eval that need no device: raised before anything else is set up."""
    if args.resident_windows and args.raw_input:
        raise SystemExit("--resident_windows and --raw_input name two paths for the same raw raster (windows planned once on the device / "
                         "filled one by one): give one of them")
    if min(args.raster_hw) < args.patchsize:
        raise SystemExit(f"--raster_hw {args.raster_hw[0]} {args.raster_hw[1]} is smaller than --patchsize {args.patchsize}: the reference's "
                         f"sliding windows are not defined for a raster with a side below the patch size (h, w >= patchsize)")
    if args.coarse_regions:
        fine = TEST_RASTER_REGIONS
        if args.coarse_regions < 2 or args.coarse_regions >= fine:
            raise SystemExit(f"--coarse_regions groups the {fine} fine census units into N coarse ones: 2 <= N < {fine}, got "
                             f"{args.coarse_regions}")


class Trainer:
    def __init__(self, args):
        self.args = args
        check_building_layer(args)
        check_repair_args(args)
        check_native_single(args)
        self.rank, self.local_rank, self.world = init_from_env()
        if not torch.cuda.is_available():
            raise SystemExit("popcorn_amd training needs a HIP device (no CPU path)")
        torch.cuda.set_device(self.local_rank)
        self.device = torch.device("cuda", self.local_rank)
        self.exp = new_log(os.path.join(args.save_dir, "So2Sat"), args) if self.rank == 0 else None
        # host-side glue (collate, augmentation draws) is many tiny CPU ops: an OpenMP pool as wide as a 256-core host
        # costs more per op than the op itself
        torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
        if self.world > 1 and args.torch_optimizer:
            raise SystemExit("--torch_optimizer is the single-process reference recipe: it has no gradient all-reduce; "
                             "data-parallel runs use the fused step (drop the flag)")
        seed_all(args.seed)
        collate = Population_Dataset_collate_fn
        self._resident_feed = None
        self._step_nan_fill = args.nan_fill                              # --resident_repair: the repair is in the batch already
        if (args.resident_assemble or args.resident_pixel_budget > 0) and args.resident_region is None:
            raise SystemExit("--resident_assemble / --resident_pixel_budget assemble batches from resident rasters: they need "
                             "--resident_region")
        if args.resident_region is not None:
            self._init_resident_region()
        if args.units_per_crop > 0:
            if args.torch_optimizer or (self.world > 1 and not args.device_units):
                raise SystemExit("--units_per_crop trains with the fused eager step in a single process (no --torch_optimizer, no data "
                                 "parallelism); --device_units lifts the second restriction and the eager one")
            from .data.units import SyntheticMultiUnitDataset, collate_units
            ds = SyntheticMultiUnitDataset(args.synthetic_regions, units=args.units_per_crop, min_hw=args.synthetic_hw_range[0],
                                           max_hw=args.synthetic_hw_range[1], seed=args.seed, fixed_hw=args.fixed_hw, ragged=True,
                                           buildings=args.building_layer)
            collate = collate_units
        else:
            ds = SyntheticWeaksupDataset(args.synthetic_regions, min_hw=args.synthetic_hw_range[0], max_hw=args.synthetic_hw_range[1],
                                         seed=args.seed, fixed_hw=args.fixed_hw, nan_clouds=args.nan_clouds, ascfill=args.ascfill,
                                         buildings=args.building_layer)
        self.sampler = None
        if self.world > 1:
            self.sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=self.world, rank=self.rank,
                                                                           shuffle=True, seed=args.seed, drop_last=True)
        self.loader = torch.utils.data.DataLoader(ds, batch_size=args.weak_batch_size, num_workers=args.num_workers,
                                                  shuffle=self.sampler is None, sampler=self.sampler,
                                                  collate_fn=collate, drop_last=True,
                                                  persistent_workers=args.num_workers > 0)
        # weak validation set (run_train.py:410-414: a second Population_Dataset in weaksup mode, batch size -wvb)
        self.val_loader = torch.utils.data.DataLoader(
            SyntheticWeaksupDataset(args.synthetic_val_regions, min_hw=args.synthetic_hw_range[0], max_hw=args.synthetic_hw_range[1],
                                    seed=args.seed + 77, fixed_hw=args.fixed_hw, nan_clouds=args.nan_clouds, ascfill=args.ascfill,
                                    buildings=args.building_layer),
            batch_size=args.weak_val_batch_size, shuffle=False, collate_fn=Population_Dataset_collate_fn, drop_last=False)
        self._test_raster = None
        self._resident_windows = None                                    # --resident_test: planned at the first test, reused afterwards
        self.model = model_dict[args.model](**get_model_kwargs(args, args.model)).to(self.device)   # same seed: same init on every rank
        self.model.set_precision(args.precision)
        self.model.native_forward = bool(getattr(args, "native_forward", False))     # (validate_weak / test_target; infer.py: route_ok)
        # from here on the CPU generators feed per-rank randomness (augmentation coins, the 60x60 sparsity grid of
        # get_sparsity_mask): every rank gets its own stream, rank 0 keeps the single-process one
        seed_all(args.seed + 2 + 1000 * self.rank)
        self.data_transform = default_train_transform()                    # run_train.py:386-402
        if hasattr(self._resident_feed, "transform"):
            self._resident_feed.transform = self.data_transform            # --resident_assemble: the feed draws the coins of this set
        self.reducer = FlatReducer()
        self.info = {"epoch": 0, "iter": 0, "sampleitr": 0}
        self._r2buf = collections.deque()
        if args.torch_optimizer:
            head_name = ["head.6.weight", "head.6.bias"]                     # run_train.py:82-90
            named = list(self.model.named_parameters())
            self.optimizer = torch.optim.Adam([
                {"params": [p for n, p in named if n not in head_name and "unetmodel" not in n], "weight_decay": args.weightdecay},
                {"params": [p for n, p in named if n not in head_name and "unetmodel" in n], "weight_decay": args.weightdecay},
                {"params": [p for n, p in named if n in head_name and "unetmodel" not in n], "weight_decay": 0.0}],
                lr=args.learning_rate)
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=args.lr_step, gamma=args.lr_gamma)
            self.fused = None
        else:
            from .train import FusedTrainStep
            # raw_norm: the feed hands the step the loader's own 6 bands [S2 R G B NIR | S1 VV VH] un-normalised (prepare_sample_fused);
            # band j of that tile IS model channel j
            self.fused = FusedTrainStep(self.model, lr=args.learning_rate, weight_decay=args.weightdecay,
                                        gradient_clip=args.gradient_clip, loss=args.loss, lam=args.lam,
                                        scale_regularization=args.scale_regularization, lam_weak=args.lam_weak,
                                        reducer=self.reducer,
                                        use_graph=args.fixed_hw is not None and (args.units_per_crop == 0 or args.device_units),
                                        raw_norm=(tuple(range(6)), stats.MEAN6, stats.STD6), native_units=args.native_units,
                                        device_units=args.device_units and args.units_per_crop > 0,
                                        native_layer=getattr(args, "native_layer", False),
                                        native_single=getattr(args, "native_single", False))
        if args.resume:
            self.resume(args.resume)

    def _init_resident_region(self):
        """--resident_region: the training data is a synthetic raw raster kept on the device, planned into census-unit crops and fed by one
        gather launch per batch (data/region.py) in place of loader -> collate -> pinned staging -> copy stream.  2 * R integers: R
        rasters as one resident atlas (data/atlas.py) -- concatenated plans, one launch per batch, validation and test per region.  Two
        integers are the single-region run as it was: same raster, plan, feeds, launches and metric keys."""
        a = self.args
        if a.torch_optimizer:
            raise SystemExit("--resident_region feeds device batches to the fused step: the --torch_optimizer recipe keeps the host loader")
        if a.fixed_hw is not None:
            raise SystemExit("--resident_region cuts census-unit crops of variable size: it cannot be combined with --fixed_hw")
        if self.world > 1:
            raise SystemExit("--resident_region runs in a single process: sharding a crop plan over data-parallel ranks is not part of it")
        assemble = a.resident_assemble or a.resident_pixel_budget > 0
        if assemble and a.nan_fill and not a.resident_repair:
            raise SystemExit("--resident_assemble / --resident_pixel_budget cannot be combined with --nan_fill: the fill sits between the "
                             "gather and the augmentation, which the one-launch assembly fuses; the unfused --resident_region feed takes it")
        if a.resident_pixel_budget < 0 or a.resident_max_batch < 1 or not 0.0 <= a.resident_min_fill <= 1.0:
            raise SystemExit("--resident_pixel_budget >= 0, --resident_max_batch >= 1 and --resident_min_fill in [0, 1]")
        from .data.atlas import AtlasBatchFeed, AtlasPlan, AtlasRegionFeed, ResidentAtlas, plan_repair_atlas
        from .data.region import (ResidentBatchFeed, ResidentItems, ResidentRegion, ResidentRegionFeed, plan_multi_unit, plan_one_unit,
                                  plan_repair, split_census)
        S = a.resident_seasons
        # R rasters: region 0 is the single-region run's (seed + 20), region k is seeded seed + 20 + k
        shapes, units = resident_shapes(a)
        R = len(shapes)
        with_asc = a.resident_repair or a.resident_test or a.resident_val
        self.region_datas = [SyntheticTestRaster(hw[0], hw[1], seasons=S, n_regions=units[k], seed=a.seed + 20 + k, device=self.device,
                                                 raw=True, nan_clouds=a.nan_clouds, s1_gap=a.resident_s1_gap, buildings=a.building_layer)
                             for k, hw in enumerate(shapes)]
        self.regions = [ResidentRegion.from_synthetic(d, with_asc=with_asc) for d in self.region_datas]
        self.region, self.region_data = self.regions[0], self.region_datas[0]     # (R = 1: the raster of evaluate_raster(raw=True) too)
        self.atlas = ResidentAtlas(self.regions) if R > 1 else None
        # the reference's need_asc: --ascfill means every region, --resident_ascfill the listed ones
        self.region_ascfill = [a.ascfill or k in (getattr(a, "resident_ascfill", None) or ()) for k in range(R)]
        kw = dict(max_pix=a.max_weak_pix, max_pix_box=a.max_pix_box)

        def plan_of(split, region):
            # the reference's order: the split, then the two size filters (inside the planner)
            n = region.census_idx.numel()
            ids, pop = split_census(region.census_idx, region.census_pop, split)
            if ids.numel() < 1:
                raise SystemExit(f"--resident_val: the {split} split of {n} census rows is empty (int({n} * 0.8) = {int(n * 0.8)} rows train)")
            if a.units_per_crop > 0:
                return plan_multi_unit(region.table, ids, pop, region.shape, units_per_crop=a.units_per_crop, **kw)
            return plan_one_unit(region.table, ids, pop, region.shape, **kw)

        plans = [plan_of("train" if a.resident_val else "all", r) for r in self.regions]
        self.region_plan = plans[0] if R == 1 else AtlasPlan.concat(plans)
        self.val_sets, self.val_items = None, None
        if a.resident_val:
            # the held-out 20 % of every region: season, orbit and repaired sites of every item planned once; a generator of its own per
            # region, seeded from --seed
            self.val_sets = []
            for k, r in enumerate(self.regions):
                val_plan = plan_of("val", r)
                if len(val_plan) < 1:
                    raise SystemExit("--resident_val: no unit of the validation split survives the size filters")
                v = ResidentItems(r, val_plan, seasons=S, generator=torch.Generator().manual_seed(a.seed), ascfill=self.region_ascfill[k])
                self.val_sets.append(v)
                if self.rank == 0:
                    print(f"resident validation{'' if R == 1 else f' (region {k})'}: {len(val_plan)} items, {len(v.dropped)} dropped, "
                          f"{v.ascending} ascending, {v.entries} table entries ({v.nbytes} bytes), built in {v.build_ms:.1f} ms", flush=True)
            self.val_items = self.val_sets[0]
        self.region_repair = None
        if a.resident_repair:
            n0 = len(self.region_plan)
            if R == 1:
                self.region_plan, self.region_repair = plan_repair(self.region, self.region_plan, seasons=S, ascfill=self.region_ascfill[0])
            else:
                self.region_plan, self.region_repair = plan_repair_atlas(self.atlas, self.region_plan, seasons=S,
                                                                         ascfill=[k for k in range(R) if self.region_ascfill[k]])
            self._step_nan_fill = False
            r = self.region_repair
            if self.rank == 0:
                per = "" if R == 1 else " (per region: " + ", ".join(f"{k}: {len(v)}" for k, v in sorted(r.dropped_by_region.items())) + ")"
                print(f"resident repair: {n0} items, {len(r.dropped)} dropped{per}, {r.ascending} ascending, {r.entries} table entries "
                      f"({r.nbytes} bytes), built in {r.build_ms:.1f} ms", flush=True)
        if len(self.region_plan) < a.weak_batch_size:
            raise SystemExit(f"--resident_region: the plan holds {len(self.region_plan)} crops, fewer than one batch of {a.weak_batch_size}")
        gen = torch.Generator().manual_seed(a.seed)
        source = self.region if R == 1 else self.atlas
        if assemble:
            # the coins are the feed's to draw (once per batch, right before the step).  The feed validates its transform at construction;
            # Trainer.__init__ hands it the trainer's own data_transform, the same set, once that exists
            feed = ResidentBatchFeed if R == 1 else AtlasBatchFeed
            self._resident_feed = feed(source, self.region_plan, a.weak_batch_size, transform=default_train_transform(),
                                       generator=gen, drop_last=True, pixel_budget=a.resident_pixel_budget,
                                       max_batch=a.resident_max_batch, min_fill=a.resident_min_fill, repair=self.region_repair, seasons=S)
        else:
            feed = ResidentRegionFeed if R == 1 else AtlasRegionFeed
            self._resident_feed = feed(source, self.region_plan, a.weak_batch_size, generator=gen, drop_last=True,
                                       repair=self.region_repair, seasons=S)

    def _region_tag(self, k):
        """The metric tag of resident region k: today's for a single region, numbered for an atlas (the reference keys them per region)."""
        return "MainCensus_synthetic_fine" if len(self.regions) == 1 else f"MainCensus_synthetic{k}_fine"

    # ---- checkpoint (run_train.py:445-476) --------------------------------------------------------------------------
    def save_model(self, prefix="last"):
        if self.rank != 0:
            return None
        path = os.path.join(self.exp, f"{prefix}_model.pth")
        if self.fused is not None:
            # torch.optim.Adam / StepLR state-dict layout (what the reference's resume() loads, run_train.py:458-472),
            # plus the flat buffers themselves under an extra key
            a = self.args
            opt = self.fused.torch_adam_state_dict([n for n, _ in self.model.named_parameters()])
            opt["fused_adam"] = self.fused.optimizer_state()
            ep = self.info["epoch"] - 1                       # StepLR.last_epoch at the time the reference saves
            sched = {"step_size": a.lr_step, "gamma": a.lr_gamma, "base_lrs": [a.learning_rate] * 3, "last_epoch": max(ep, 0),
                     "_step_count": max(ep, 0) + 1, "_get_lr_called_within_step": False, "_last_lr": [self.fused.lr] * 3,
                     "lr": self.fused.lr}
        else:
            opt, sched = self.optimizer.state_dict(), self.scheduler.state_dict()
        torch.save({"model": self.model.state_dict(), "epoch": self.info["epoch"], "iter": self.info["iter"],
                    "optimizer": opt, "scheduler": sched}, path)
        return path

    def _lr_at(self, epoch):
        """StepLR(step_size=lr_step, gamma=lr_gamma) stepped once per finished epoch (run_train.py:93,139-141)."""
        a = self.args
        return a.learning_rate * (a.lr_gamma ** (epoch // a.lr_step)) if a.lr_gamma != 1.0 else a.learning_rate

    def resume(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.model.load_state_dict(ck["model"])
        if self.fused is not None:
            self.fused.sync_from_model()
        self.info["epoch"], self.info["iter"] = ck["epoch"], ck["iter"]
        opt = ck.get("optimizer") or {}
        if self.fused is not None:
            if "fused_adam" in opt:
                self.fused.load_optimizer_state(opt["fused_adam"])
            elif "state" in opt and "param_groups" in opt:
                # a torch.optim.Adam state dict (reference checkpoints, --torch_optimizer runs): per-parameter
                # exp_avg / exp_avg_sq / step -> the flat buffers, matched through the parameter order of run_train.py:82-90
                self.fused.load_torch_adam_state(opt, [n for n, _ in self.model.named_parameters()])
            else:
                print("warning: checkpoint holds no usable optimizer state; Adam moments start from zero")
            self.fused.set_lr(self._lr_at(self.info["epoch"]))       # the checkpoint is written BEFORE the epoch's lr update
        else:
            if "state" in opt and "param_groups" in opt:
                self.optimizer.load_state_dict({"state": opt["state"], "param_groups": opt["param_groups"]})
                self.scheduler.load_state_dict({k: v for k, v in ck["scheduler"].items() if k != "lr"})
            else:
                print("warning: checkpoint holds no torch.optim.Adam state; moments start from zero")

    # ---- loop ------------------------------------------------------------------------------------------------------
    def train_step(self, sample):
        a = self.args
        s = None
        if self.fused is not None and torch.is_tensor(sample.get("raw")) and sample["raw"].is_cuda:
            # a batch assembled by ResidentBatchFeed: augmented raw tile and labels are there already, the coins drawn by the feed
            s = {k: sample[k] for k in ("raw", "admin_mask", "census_idx", "y", "building_counts") if k in sample}
        elif self.fused is not None and torch.is_tensor(sample.get("S2")) and sample["S2"].is_cuda:
            # a batch staged by the feed: augmentation + assembly in one launch, normalisation inside the step (raw input form)
            s = prepare_sample_fused(sample, self.data_transform, nan_fill=self._step_nan_fill)
        if s is None:
            s = normalize_sample(sample, self.device, self.data_transform, nan_fill=self._step_nan_fill)
        if sample.get("census_n") is not None:             # multi-unit items (--units_per_crop): the valid units per row, host data
            s["census_n"] = sample["census_n"]
            K = s["census_idx"].shape[1]
            if a.device_units and a.fixed_hw is not None and K < a.units_per_crop:
                # the collate pads to the batch's own maximum; the captured step is keyed by K: pad on to the data set's K, so that every
                # batch (and, data parallel, every rank) replays one capture.  The padding is behind census_n: the step ignores it
                pad = (0, a.units_per_crop - K)
                s["census_idx"] = torch.nn.functional.pad(s["census_idx"], pad, value=-1)
                s["y"] = torch.nn.functional.pad(s["y"], pad, value=0.0)
        dk = "raw" if "raw" in s else "input"
        num_pix = s[dk].shape[0] * s[dk].shape[2] * s[dk].shape[3]
        if self.world > 1 and a.fixed_hw is None:
            # variable tile sizes: ranks must take the same regime (and skip together), or their collective counts
            # diverge and the job hangs.  The largest rank decides.
            import torch.distributed as dist
            t = torch.tensor([num_pix], device=self.device, dtype=torch.int64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            num_pix = int(t.item())
        enc_ng, unet_ng, skip = limit_regime(num_pix, a.limit1, a.limit2, a.limit3)
        if skip:
            return None
        if self.fused is not None:
            # loss_out is one device buffer overwritten by every step: keep a copy for the running log mean
            loss = self.fused.step(s, encoder_no_grad=enc_ng, unet_no_grad=unet_ng)[0].clone()
            # the R2 buffers hold the last 300 samples and are read at log steps only: a step whose samples will have left the window
            # by the next log step does not copy them (two launches per step on the smallest regions)
            to_log = a.logstep_train - (self.info["iter"] % a.logstep_train)
            if to_log * s["y"].numel() <= 300 + s["y"].numel():
                y, pc = s["y"], self.fused.last["popcount"]
                if s.get("census_n") is not None:           # (B, K) padded -> the flat N of the step's popcount, (b, k) order
                    from .data.units import flat_valid
                    y = flat_valid(y, s["census_n"])
                    pc = pc[:y.numel()]                     # (a device-N step's popcount has the capacity B * K: the first N count)
                self._buffer_r2(pc, y)
            return loss
        from torch.nn.utils import clip_grad_norm_
        from .utils.losses import get_loss
        out = self.model(s, train=True, padding=False, sparse=True, encoder_no_grad=enc_ng, unet_no_grad=unet_ng)
        loss, _ = get_loss(out, s, scale=out["scale"], loss=a.loss, lam=a.lam, scale_regularization=a.scale_regularization,
                           tag="weak")
        if torch.isnan(loss) or torch.isinf(loss):
            raise Exception("detected NaN/Inf loss..")
        self.optimizer.zero_grad()
        (loss * a.lam_weak).backward()
        if a.gradient_clip > 0.0:
            clip_grad_norm_(self.model.parameters(), a.gradient_clip)
        self.optimizer.step()
        self._buffer_r2(out["popcount"].detach(), s["y"])
        return loss.detach()

    def _buffer_r2(self, pred, y):
        """The 300-sample prediction / target buffers behind the logged training R2 (run_train.py:107-108,220-221,272);
        kept on the device, read at log steps only."""
        self._r2buf.append((pred.detach().clone(), y.detach().clone()))
        while sum(p.numel() for p, _ in self._r2buf) > 300 and len(self._r2buf) > 1:
            self._r2buf.popleft()

    # ---- validation / in-training target test (run_train.py:289-370) ---------------------------------------------------
    def validate_weak(self):
        """Weak validation: census-level metrics of model(sample, padding=False) over the validation regions.  --resident_val: over the
        held-out units of the resident raster (data/region.py: ResidentItems), one launch per item in front of the model."""
        from .utils.metrics import get_test_metrics
        self.model.eval()
        pred, gt = [], []
        native = bool(self.model.native_forward)         # a native forward's outputs live in the model's arena (infer.py): keep copies
        with torch.no_grad():
            if self.args.resident_val:
                # one ResidentItems per region, metrics per region (run_train.py:295-310)
                from .data.units import flat_valid
                self.valweak_stats = {}
                for k, items in enumerate(self.val_sets):
                    pred, gt = [], []
                    for s in items:
                        out = self.model(s, padding=False)
                        pred.append(out["popcount"].clone() if native else out["popcount"])
                        gt.append(flat_valid(s["y"], s["census_n"]) if s.get("census_n") is not None else s["y"])
                    stats = get_test_metrics(torch.cat(pred), torch.cat(gt).float(), tag=self._region_tag(k))
                    self.valweak_stats.update({key + "/val": float(v) for key, v in stats.items()})
                self._log(self.valweak_stats)
                return self.valweak_stats
            else:
                for sample in self.val_loader:
                    s = normalize_sample(sample, self.device, None, nan_fill=self.args.nan_fill)
                    out = self.model(s, padding=False)
                    pred.append(out["popcount"].clone() if native else out["popcount"])
                    gt.append(s["y"])
        stats = get_test_metrics(torch.cat(pred), torch.cat(gt).float(), tag="MainCensus_synthetic_fine")
        self.valweak_stats = {k + "/val": float(v) for k, v in stats.items()}
        self._log(self.valweak_stats)
        return self.valweak_stats

    def test_target(self, save=False):
        """In-training target test: sliding windows over the test raster -> stitched map -> census aggregation -> metrics
        (run_train.py:314-370).  The reference accumulates in fp16 host maps; here the accumulators are fp32 and stay on
        the device (popcorn_amd.eval.Stitcher)."""
        from . import eval as E
        from .utils.metrics import get_test_metrics
        a = self.args
        if a.resident_test:
            return self._test_resident(save)
        if self._test_raster is None:
            self._test_raster = SyntheticTestRaster(a.test_raster_hw[0], a.test_raster_hw[1], seasons=1, n_regions=64,
                                                    seed=a.seed + 10, device=self.device, buildings=a.building_layer)
        data = self._test_raster
        self.model.eval()
        kw = {} if data.buildings is None else {"buildings": data.buildings}       # --building_layer: the test raster's own layer
        out, _, scale, _ = E.evaluate_raster([self.model], data.raster, a.test_patchsize, a.test_overlap, False,
                                             FlatReducer(), 0, **kw) if self.world == 1 else \
            E.evaluate_raster([self.model], data.raster, a.test_patchsize, a.test_overlap, False, self.reducer, self.rank, **kw)
        cp, cg = E.convert_popmap_to_census(out, data.boundary, data.census_idx, data.census_pop)
        stats = get_test_metrics(cp, cg, tag="MainCensus_synthetic_fine")
        self.target_test_stats = {k + "/targettest": float(v) for k, v in stats.items()}
        if save and self.rank == 0:
            torch.save({"popdensemap": out.cpu(), "scale": None if scale is None else scale.cpu()},
                       os.path.join(self.exp, "synthetic_predictions.pt"))
        self._log(self.target_test_stats)
        return self.target_test_stats

    def _test_resident(self, save=False):
        """--resident_test: the target test over the region the run trains on (the reference's `-treg rwa -tregtrain rwa`), its windows
        planned once (data/region.py: ResidentWindows) -- every later test is one launch per window in front of the model."""
        from . import eval as E
        from .data.region import ResidentWindows
        from .utils.metrics import get_test_metrics
        a, R = self.args, len(self.regions)
        if self._resident_windows is None:
            # one plan per region, each made once (run_train.py:322-366 tests region by region)
            self._resident_window_sets = []
            for k, region in enumerate(self.regions):
                f = ResidentWindows(region, a.test_patchsize, a.test_overlap, fourseasons=False, ascfill=self.region_ascfill[k])
                self._resident_window_sets.append(f)
                if self.rank == 0:
                    print(f"resident windows{'' if R == 1 else f' (region {k})'}: {len(f.idx)} windows, {f.ascending} ascending, "
                          f"{f.entries} table entries ({f.nbytes} bytes), built in {f.build_ms:.1f} ms", flush=True)
            self._resident_windows = self._resident_window_sets[0]
        self.model.eval()
        self.target_test_stats = {}
        for k, (region, windows) in enumerate(zip(self.regions, self._resident_window_sets)):
            out, _, scale, _ = E.evaluate_raster([self.model], windows, a.test_patchsize, a.test_overlap, False, FlatReducer(), 0)
            cp, cg = E.convert_popmap_to_census(out, region.boundary, region.census_idx, region.census_pop)
            stats = get_test_metrics(cp, cg, tag=self._region_tag(k))
            self.target_test_stats.update({key + "/targettest": float(v) for key, v in stats.items()})
            if save and self.rank == 0:
                torch.save({"popdensemap": out.cpu(), "scale": None if scale is None else scale.cpu()},
                           os.path.join(self.exp, "synthetic_predictions.pt" if R == 1 else f"synthetic{k}_predictions.pt"))
        self._log(self.target_test_stats)
        return self.target_test_stats

    def _log(self, record):
        if self.rank == 0:
            with open(os.path.join(self.exp, "train_log.jsonl"), "a") as fh:
                fh.write(json.dumps({**record, **self.info}) + "\n")

    def train(self):
        a = self.args
        log = open(os.path.join(self.exp, "train_log.jsonl"), "a") if self.rank == 0 else None
        lr = self._lr_at(self.info["epoch"])
        t0 = time.time()
        recent = collections.deque(maxlen=a.logstep_train)                  # running window for the log line, across epochs
        losses = []
        for epoch in range(self.info["epoch"], a.num_epochs):
            self.model.train()
            if self.sampler is not None:
                self.sampler.set_epoch(epoch)                              # a fresh shuffle per epoch on every rank
            losses = []
            # the fused step is fed one batch ahead through pinned memory and a copy stream (data/feed.py: RegionFeed); the torch-optimizer
            # recipe keeps the reference's synchronous loop
            if self._resident_feed is not None:
                feed = self._resident_feed                 # --resident_region: one gather launch per batch, no producer thread
            else:
                feed = RegionFeed(self.loader, self.device) if self.fused is not None else self.loader
            if self.fused is not None:
                self.fused.capture_guard = feed.pause              # (the feed's producer thread keeps still while a step is captured)
            for i, sample in enumerate(feed):
                loss = self.train_step(sample)
                if loss is not None:
                    losses.append(loss)
                    recent.append(loss)
                self.info["iter"] += 1
                self.info["sampleitr"] += len(sample["admin_mask"])       # (weak_batch_size, but for pixel-budget batches)
                if (i + 1) % a.val_every_i_steps == 0 and a.weak_validation:          # run_train.py:255-259
                    self.validate_weak()
                    self.model.train()
                if (i + 1) % a.test_every_i_steps == 0:                              # run_train.py:262-265
                    self.test_target(save=True)
                    self.model.train()
                if self.info["iter"] % a.logstep_train == 0 and recent:              # by global iteration (run_train.py:240)
                    window = torch.stack(list(recent))
                    # the fused step never reads the loss back; its NaN/Inf guard (run_train.py:224-227) is this one
                    # device->host read per log step, covering every step of the window
                    finite = torch.isfinite(window).all()
                    if self.fused is not None:
                        # the conv / hidden-layer ReLU epilogues take the IEEE maximum (a NaN activation becomes 0), so a
                        # diverged run shows up in the gradient norm and the parameters before it shows up in the loss
                        finite = finite & torch.isfinite(self.fused.norm).all() & torch.isfinite(self.fused.flat_p.sum())
                    if not bool(finite):
                        raise Exception("detected NaN/Inf loss..")
                    if log:
                        from .utils.losses import r2
                        pr = torch.cat([p_ for p_, _ in self._r2buf])[-300:]
                        yy = torch.cat([y_ for _, y_ in self._r2buf])[-300:]
                        rec = {"iter": self.info["iter"], "epoch": epoch, "loss": window.mean().item(), "lr": lr,
                               "Population_weak/r2": float(r2(pr, yy)) if pr.numel() > 1 else 0.0}
                        log.write(json.dumps(rec) + "\n")
                        log.flush()
                if a.max_steps and self.info["iter"] >= a.max_steps:
                    break
            if losses and not bool(torch.isfinite(torch.stack(losses)).all()):
                raise Exception("detected NaN/Inf loss..")
            self.info["epoch"] = epoch + 1
            if a.save_model in ("last", "both"):
                self.save_model("last")
            if (epoch + 1) % a.val_every_n_epochs == 0:                              # run_train.py:126-137
                if a.weak_validation:
                    self.validate_weak()
                self.test_target(save=True)
                if a.save_model in ("last", "both"):
                    self.save_model("last")
            if a.lr_gamma != 1.0:                                          # StepLR(step_size=lr_step, gamma), run_train.py:93,141
                lr = self._lr_at(epoch + 1)
                if self.fused is not None:
                    self.fused.set_lr(lr)
                else:
                    self.scheduler.step()
            if a.max_steps and self.info["iter"] >= a.max_steps:
                break
        if self.rank == 0:
            print(f"Training finished in {time.time() - t0:.1f} s, {self.info['iter']} iterations; logs in {self.exp}")
            if getattr(a, "native_forward", False):
                print(f"native forwards: {self.model.native_forwards}", flush=True)
        return losses


def run_train(argv=None):
    args = train_parser().parse_args(argv)
    t = Trainer(args)
    t.train()
    return t


def run_eval(argv=None):
    from . import eval as E
    from .utils.metrics import get_test_metrics
    args = eval_parser().parse_args(argv)
    check_building_layer(args)
    check_eval_args(args)
    rank, local_rank, world = init_from_env()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    seed_all(args.seed)
    models = []
    n = max(len(args.resume), args.ensemble)
    for j in range(n):
        m = model_dict[args.model](**get_model_kwargs(args, args.model)).to(dev)
        if j < len(args.resume):
            m.load_state_dict(torch.load(args.resume[j], map_location="cpu", weights_only=False)["model"])   # run_eval.py:243-257
        m.native_forward = bool(args.native_forward)
        models.append(m.eval().set_precision(args.precision))
    data = SyntheticTestRaster(args.raster_hw[0], args.raster_hw[1], seasons=4 if args.fourseasons else 1, device=dev,
                               raw=args.raw_input or args.resident_windows, nan_clouds=args.nan_clouds, s1_gap=args.s1_gap,
                               coarse_regions=args.coarse_regions, buildings=args.building_layer)
    coarse = args.coarse_regions > 0
    reducer = FlatReducer()
    raster = data.raster
    if args.resident_windows:
        from .data.region import ResidentRegion, ResidentWindows
        raster = ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=True), args.patchsize, args.overlap,
                                 fourseasons=args.fourseasons, ascfill=args.ascfill, rank=rank, world=reducer.world)
        if rank == 0:
            print(f"resident windows: {len(raster.idx)} windows, {raster.ascending} ascending, {raster.entries} table entries "
                  f"({raster.nbytes} bytes), built in {raster.build_ms:.1f} ms", flush=True)
    product = E.ProductGrid(args.raster_hw[0], args.raster_hw[1], args.product_cell, n, dev) if args.product_cell > 0 else None
    num_ids = int(data.census_idx.max()) + 1
    census = None
    if args.census_table and coarse:
        # both levels and the pair plane of (fine, coarse): the adjustment to the coarse census judged on the fine one, per member
        census = E.CensusTable(args.raster_hw[0], args.raster_hw[1], [data.boundary, data.boundary_coarse],
                               [num_ids, int(data.census_idx_coarse.max()) + 1], n, dev,
                               adjust={"level": 1, "census_idx": data.census_idx_coarse, "census_pop": data.census_pop_coarse})
    elif args.census_table:
        census = E.CensusTable(args.raster_hw[0], args.raster_hw[1], [data.boundary], [num_ids], n, dev)
    t0 = time.time()
    out, out_std, scale, scale_std = E.evaluate_raster(models, raster, args.patchsize, args.overlap, args.fourseasons,
                                                       reducer, rank, raw=args.raw_input, ascfill=args.ascfill, product=product,
                                                       census=census,
                                                       **({"buildings": data.buildings} if args.building_layer else {}))
    res = {}
    cp, cg = E.convert_popmap_to_census(out, data.boundary, data.census_idx, data.census_pop)
    res.update({k: float(v) for k, v in get_test_metrics(cp, cg, tag="MainCensus_synthetic_fine").items()})
    if coarse:
        # the reference's evaluator: adjusted to the TRAINING (coarse) level, judged on every level (run_eval.py:168-200)
        cp, cg = E.convert_popmap_to_census(out, data.boundary_coarse, data.census_idx_coarse, data.census_pop_coarse)
        res.update({k: float(v) for k, v in get_test_metrics(cp, cg, tag="MainCensus_synthetic_coarse").items()})
        adj = E.adjust_map_to_census(out.clone(), data.boundary_coarse, data.census_idx_coarse, data.census_pop_coarse)
        cp, cg = E.convert_popmap_to_census(adj, data.boundary_coarse, data.census_idx_coarse, data.census_pop_coarse)
        res.update({k: float(v) for k, v in get_test_metrics(cp, cg, tag="AdjCensus_synthetic_coarse").items()})
    else:
        adj = E.adjust_map_to_census(out.clone(), data.boundary, data.census_idx, data.census_pop)
    cp, cg = E.convert_popmap_to_census(adj, data.boundary, data.census_idx, data.census_pop)
    res.update({k: float(v) for k, v in get_test_metrics(cp, cg, tag="AdjCensus_synthetic_fine").items()})
    if product is not None:
        padj = ops.block_sum(adj, product.cell)
        res.update({"product_cell": product.cell, "product_shape": list(product.mean.shape),
                    "product_total": product.mean.double().sum().item(), "product_std_mean": product.std.double().mean().item(),
                    "product_adj_total": padj.double().sum().item()})
        if args.product_out and rank == 0:
            torch.save({"mean": product.mean.cpu(), "std": product.std.cpu(), "adjusted": padj.cpu(), "cell": product.cell},
                       args.product_out)
    if census is not None:
        res.update(census.metrics(0, data.census_idx, data.census_pop, tag="TableCensus_synthetic_fine"))
        if coarse:
            res.update(census.adjusted_metrics(0, data.census_idx, data.census_pop, tag="TableAdjCensus_synthetic_fine"))
        if args.census_out and rank == 0:
            saved = {"totals": census.totals.cpu(), "mean": census.mean.cpu(), "std": census.std.cpu(), "num_ids": census.num_ids}
            if coarse:
                _, ens, _, astd = census.adjusted(0)
                saved["adjusted"], saved["adjusted_std"] = ens.cpu(), astd.cpu()
            if args.census_details:
                mean0, std0 = (census.level(0)[1], census.level(0)[2]) if coarse else (census.mean, census.std)
                maps = E.census_detail_maps(mean0, data.boundary, data.census_idx, data.census_pop, pred_std=std0)
                saved["details"] = {k: v.cpu() for k, v in maps.items()}
                if coarse:      # the reference's <region>_<level>_adj folder: the detail maps of the adjusted ensemble totals
                    maps = E.census_detail_maps(ens.float(), data.boundary, data.census_idx, data.census_pop, pred_std=astd)
                    saved["details_adj"] = {k: v.cpu() for k, v in maps.items()}
            torch.save(saved, args.census_out)
    torch.cuda.synchronize()
    if rank == 0:
        res["seconds"] = time.time() - t0
        if args.native_forward:
            res["native_forwards"] = sum(m.native_forwards for m in models)
            print(f"native forwards: {res['native_forwards']}", flush=True)
        print(json.dumps(res))
    return res
