#!/usr/bin/env python3
"""Device time of the three multi-unit launches (ops.unit_mask / unit_popcount / unit_paint, csrc/units.hip) next to the one-unit sparsity
mask (ops.sparsity_mask) and the head forward on the SAME crop, under a device-event timer: per op, ``--inner`` back-to-back calls
between two events (one call is a few microseconds: a single call measures the event pair), repeated ``--reps`` times, median and minimum
per call.  Bytes per pixel are computed from the shapes, the rate is bytes over the median time.

    python tools/bench_units.py [--shape 2 512 512] [--units 64] [--reps 30] [--inner 20] [--out profiles/units_bench.json]

The expectation written down before the first run: each of the three is a single pass over <= 16 B / pixel and costs less than the head
forward of the same crop.  The tool states per op whether that held."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_crop(B, H, W, K, seed=0):
    """admin (B, H, W): K listed units as irregular nearest-seed cells + 3 unlisted neighbours; census_idx (B, K)."""
    g = torch.Generator().manual_seed(seed)
    admin = torch.empty(B, H, W)
    cidx = torch.empty(B, K, dtype=torch.int64)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    for b in range(B):
        sy, sx = torch.rand(K + 3, generator=g) * H, torch.rand(K + 3, generator=g) * W
        owner = torch.full((H, W), 0, dtype=torch.int64)
        best = torch.full((H, W), float("inf"))
        for j in range(K + 3):                     # (a loop: a (K, H, W) distance tensor at 512 x 512 x 67 is 70 MB)
            d = (yy - sy[j]) ** 2 + (xx - sx[j]) ** 2
            owner = torch.where(d < best, torch.tensor(j), owner)
            best = torch.minimum(d, best)
        ids = torch.cat([1 + b * K + torch.randperm(K, generator=g), 1_000_000 + torch.arange(3)])
        admin[b] = ids[owner].float()
        cidx[b] = ids[:K]
    return admin, cidx


def timed(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[2, 512, 512])
    ap.add_argument("--units", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "units_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_units.py measures on a HIP device; none found")
    from popcorn_amd import ops
    from popcorn_amd.model import POPCORN
    from popcorn_amd.model.popcorn import pad_geometry
    B, H, W = a.shape
    K = a.units
    admin, cidx = make_crop(B, H, W, K)
    admin, cidx = admin.cuda(), cidx.cuda()
    g = torch.Generator().manual_seed(1)
    building = torch.rand(B, 1, H, W, generator=g)
    building[building < 0.5] = 0.0
    building = building.cuda()
    sel = torch.zeros(H + W, dtype=torch.uint8)
    sel[torch.ones(H).multinomial(min(60, H))] = 1
    sel[H + torch.ones(W).multinomial(min(60, W))] = 1
    sel = sel.cuda()
    lay = ops.unit_layout(cidx, None)
    N = lay["N"]
    slot, mask, counts = ops.unit_mask(building, admin, lay["units"], lay["unit_off"], sel[:H], sel[H:], True)
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, feature_extractor="DDA", occupancymodel=True, pretrained=True, biasinit=0.9407,
                sentinelbuildings=True).cuda()
    pt, pb, pl, pr = pad_geometry(H, W, False)
    feats = torch.randn(B, 16, H + pt + pb, W + pl + pr, device="cuda")
    ht = m.head_tensors()
    _, popdense, _ = ops.head_fwd(feats, pt, pl, H, W, ht, building, mask=mask)
    g_pc = torch.randn(N, device="cuda")
    g_pd = torch.empty(B, H, W, device="cuda")
    pc = torch.empty(N, device="cuda")
    one = cidx[:, 0].contiguous()
    n_px = B * H * W
    # bytes per pixel from the shapes: reads + writes of the per-pixel maps (the unit lists, selections and counts are O(K + H + W))
    ops_ = {
        "unit_mask": (lambda: ops.unit_mask(building, admin, lay["units"], lay["unit_off"], sel[:H], sel[H:], True), 4 + 4 + 4 + 1),
        "unit_popcount": (lambda: ops.unit_popcount(popdense, slot, N, lay["unit_off"], out=pc), 4 + 4),
        "unit_paint": (lambda: ops.unit_paint(g_pc, slot, out=g_pd), 4 + 4),
        "sparsity_mask": (lambda: ops.sparsity_mask(building, admin, one, sel[:H], sel[H:], True), 4 + 4 + 1),
        "head_fwd_union_mask": (lambda: ops.head_fwd(feats, pt, pl, H, W, ht, building, mask=mask), None),
    }
    res = {"device": torch.cuda.get_device_name(0), "shape": [B, H, W], "units_per_sample": K, "N": N, "reps": a.reps, "inner": a.inner,
           "selected_fraction": float(mask.float().mean()), "timer": "device events around `inner` back-to-back calls, per call", "ops": {}}
    for name, (fn, bpp) in ops_.items():
        med, mn = timed(fn, a.reps, a.inner)
        rec = {"us_median": round(med, 2), "us_min": round(mn, 2)}
        if bpp is not None:
            rec["bytes_per_pixel"] = bpp
            rec["gb_per_s_at_median"] = round(bpp * n_px / med / 1e3, 1)
        res["ops"][name] = rec
        print(name, json.dumps(rec), flush=True)
    head = res["ops"]["head_fwd_union_mask"]["us_median"]
    res["expectation"] = {n: {"bytes_per_pixel_le_16": res["ops"][n]["bytes_per_pixel"] <= 16,
                              "faster_than_head_fwd": res["ops"][n]["us_median"] < head} for n in ("unit_mask", "unit_popcount", "unit_paint")}
    print(json.dumps(res["expectation"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
