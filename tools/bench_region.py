#!/usr/bin/env python3
"""Device time of the region-resident data path (csrc/region.hip, popcorn_amd/data/region.py), three legs, each in a child process of
its own under ``timeout -k 10`` (a leg that faults or hangs ends the run; the legs behind it do not start):

  gather  ``ops.region_gather`` per batch at 2 x 517 x 389 and 64 x 100 x 100 (uint16 and fp32 S2, arbitrary odd crop origins), next to the
          head forward of the same batch; bytes from the shapes (read 4 x 2 or 4 x 4 + 2 x 4 + 4 per crop pixel, written 28 per output pixel)
  units   ``ops.region_units`` on a 7,200 x 23,100 boundary raster with 4,096 units (4 bytes read per pixel)
  epoch   ``Trainer.train_step`` steps per second over ONE plan, through ``ResidentRegionFeed`` and through the existing ``RegionFeed``
          over a ``Dataset`` that slices the same items out of host copies of the rasters -- same process, same trainer, alternating,
          three repeats each

Timer of the first two legs: device events around ``--inner`` back-to-back calls, ``--reps`` times, median and minimum per call (as
tools/bench_units.py), the calls enqueued behind a spin kernel so that the events see device time although a call is enqueued slower than it
runs; the host's enqueue time per call is reported next to it.  The epoch leg is wall time from the first batch request to a device synchronisation after the last step.

    python tools/bench_region.py [--out profiles/region_bench.json]

The expectation written down before the first run: each kernel is a single pass -- at most 24 B read + 28 B written
per output pixel for the gather, 4 B per raster pixel for the table --, so the gather costs less than the head forward of the same batch;
the resident feed is at least as fast as the host feed within the spread of the repeats.  The tool states whether each held."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LEGS = {"gather": 180, "units": 240, "epoch": 420}          # seconds of time limit per leg


_SPIN = {}


def spin_cycles(seconds):
    """argument of torch's spin kernel for about ``seconds`` of device time (calibrated once)"""
    if "per_cycle" not in _SPIN:
        torch.cuda._sleep(1 << 20)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.cuda._sleep(1 << 24)
        torch.cuda.synchronize()
        _SPIN["per_cycle"] = max((time.perf_counter() - t0) / (1 << 24), 1e-11)
    return int(seconds / _SPIN["per_cycle"])


def timed(fn, reps, inner):
    """(median, minimum device microseconds per call, host microseconds to enqueue one call).  A call of a few microseconds is enqueued
    slower than it runs: the ``inner`` calls are enqueued BEHIND a spin kernel that keeps the stream busy meanwhile, so the two events see
    them run back to back."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    host = (time.perf_counter() - t0) / inner
    torch.cuda.synchronize()
    spin = spin_cycles(1.5 * host * inner + 3e-4)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(spin)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / inner)
    return float(np.median(ts)), float(np.min(ts)), host * 1e6


def blocky(h, w, gy, gx, device):
    ys = torch.clamp((torch.arange(h, device=device) * gy) // h, max=gy - 1)
    xs = torch.clamp((torch.arange(w, device=device) * gx) // w, max=gx - 1)
    return (ys[:, None] * gx + xs[None, :] + 1).to(torch.int32).contiguous()


def leg_gather(a):
    from popcorn_amd import ops
    from popcorn_amd.model import POPCORN
    from popcorn_amd.model.popcorn import pad_geometry
    h, w = 1536, 2048
    g = torch.Generator(device="cuda").manual_seed(1)
    s2f = torch.randint(0, 10000, (1, 4, h, w), generator=g, device="cuda").float()
    s2u = s2f.cpu().to(torch.uint16).cuda()                                    # (the same digital numbers)
    s1 = torch.randn(1, 2, h, w, generator=g, device="cuda") * 5 - 12
    boundary = blocky(h, w, 12, 16, "cuda")
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, feature_extractor="DDA", occupancymodel=True, pretrained=True, biasinit=0.9407,
                sentinelbuildings=True).cuda()
    ht = m.head_tensors()
    out = {}
    hg = torch.Generator().manual_seed(2)
    for B, H, W in ((2, 517, 389), (64, 100, 100)):
        x0 = torch.randint(0, h - H, (B,), generator=hg) | 1                   # odd origins: source rows are not 16-byte aligned
        y0 = torch.randint(0, w - W, (B,), generator=hg) | 1
        crops = [(int(x), int(x) + H, int(y), int(y) + W, 0) for x, y in zip(x0, y0)]
        n_px = B * H * W
        rec = {}
        for name, s2, rd in (("u16", s2u, 4 * 2 + 2 * 4 + 4), ("f32", s2f, 4 * 4 + 2 * 4 + 4)):
            buf = ops.region_gather(s2, s1, boundary, (0, 1, 2, 3, 0, 1), crops)
            for form, fn in (("out=", lambda: ops.region_gather(s2, s1, boundary, (0, 1, 2, 3, 0, 1), crops, out=buf)),
                             ("alloc", lambda: ops.region_gather(s2, s1, boundary, (0, 1, 2, 3, 0, 1), crops))):
                med, mn, host = timed(fn, a.reps, a.inner)
                rec[f"region_gather_{name}_{form}"] = {"us_median": round(med, 2), "us_min": round(mn, 2), "host_enqueue_us": round(host, 1),
                                                       "bytes_per_pixel": rd + 28,
                                                       "gb_per_s_at_median": round((rd + 28) * n_px / med / 1e3, 1)}
        # the head forward of the same batch: one listed unit per crop (the id at its centre), the reference's sparsity mask
        admin = buf["admin_mask"]
        cidx = admin[:, H // 2, W // 2].long().reshape(B, 1).contiguous()
        building = torch.rand(B, 1, H, W, device="cuda")
        building[building < 0.5] = 0.0
        sel = torch.zeros(H + W, dtype=torch.uint8)
        sel[torch.ones(H).multinomial(min(60, H))] = 1
        sel[H + torch.ones(W).multinomial(min(60, W))] = 1
        sel = sel.cuda()
        lay = ops.unit_layout(cidx, None)
        _, mask, _ = ops.unit_mask(building, admin, lay["units"], lay["unit_off"], sel[:H], sel[H:], True)
        pt, pb, pl, pr = pad_geometry(H, W, False)
        feats = torch.randn(B, 16, H + pt + pb, W + pl + pr, device="cuda")
        med, mn, host = timed(lambda: ops.head_fwd(feats, pt, pl, H, W, ht, building, mask=mask), a.reps, a.inner)
        rec["head_fwd"] = {"us_median": round(med, 2), "us_min": round(mn, 2), "host_enqueue_us": round(host, 1), "selected_fraction": round(float(mask.float().mean()), 3)}
        rec["gather_faster_than_head_fwd"] = all(v["us_median"] < med for k, v in rec.items() if k.startswith("region_gather"))
        out[f"{B}x{H}x{W}"] = rec
        print(f"{B}x{H}x{W}", json.dumps(rec), flush=True)
    return out


def leg_units(a):
    from popcorn_amd import ops
    h, w, n = 7200, 23100, 4096
    boundary = blocky(h, w, 64, 64, "cuda")
    table, stray = ops.region_units(boundary, n + 1)
    med, mn, _ = timed(lambda: ops.region_units(boundary, n + 1), max(a.reps // 3, 5), 3)
    t = table.cpu()
    rec = {"raster": [h, w], "units": n, "us_median": round(med, 1), "us_min": round(mn, 1), "bytes_per_pixel": 4,
           "gb_per_s_at_median": round(4 * h * w / med / 1e3, 1), "stray": int(stray), "pixels_counted": int(t[:, 4].sum()),
           "all_units_found": bool((t[1:, 4] > 0).all())}
    rec["counts_add_up"] = rec["pixels_counted"] == h * w
    print("region_units", json.dumps(rec), flush=True)
    return rec


class HostSliceDataset(torch.utils.data.Dataset):
    """The plan's items cut out of HOST copies of the rasters, as the reference's loader would (one-unit items)."""

    def __init__(self, region, plan):
        self.s2, self.s1, self.boundary = region.s2.cpu(), region.s1.cpu(), region.boundary.cpu()
        self.band, self.plan = region.band_sel, plan

    def __len__(self):
        return len(self.plan)

    def __getitem__(self, i):
        x0, x1, y0, y1 = self.plan.crops[i].tolist()
        bb = self.plan.bbox[i].tolist()
        return {"S2": self.s2[0, list(self.band[:4]), x0:x1, y0:y1].float(), "S1": self.s1[0, list(self.band[4:]), x0:x1, y0:y1],
                "admin_mask": self.boundary[x0:x1, y0:y1].float(), "y": self.plan.y[i, 0], "census_idx": self.plan.census_idx[i, :1],
                "img_coords": (bb[0], bb[2]), "valid_coords": tuple(bb), "season": 0}


def leg_epoch(a):
    from popcorn_amd.cli import Trainer, train_parser
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.feed import RegionFeed
    with tempfile.TemporaryDirectory() as tmp:
        argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -wb 2 --resident_region 2304 2560 --resident_units 400 "
                f"--save-model no --save_dir {tmp}").split()
        t = Trainer(train_parser().parse_args(argv))
        t.model.train()
        plan, region = t.region_plan, t.region
        loader = torch.utils.data.DataLoader(HostSliceDataset(region, plan), batch_size=2, shuffle=True, num_workers=0,
                                             collate_fn=Population_Dataset_collate_fn, drop_last=True)
        feeds = {"resident": lambda: t._resident_feed, "host": lambda: RegionFeed(loader, t.device)}

        def epoch(make):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for sample in make():
                t.train_step(sample)
                n += 1
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0), n
        for make in feeds.values():                                 # warm-up: allocator, pinned ring, copy-stream pick
            epoch(make)
        runs = {k: [] for k in feeds}
        for _ in range(3):
            for k, make in feeds.items():
                sps, n = epoch(make)
                runs[k].append(round(sps, 1))
        crops = plan.crops
        rec = {"raster": list(region.shape), "crops": len(plan), "batch": 2, "steps_per_epoch": n,
               "mean_crop_hw": [round(float((crops[:, 1] - crops[:, 0]).float().mean()), 1), round(float((crops[:, 3] - crops[:, 2]).float().mean()), 1)],
               "steps_per_s": runs, "median": {k: float(np.median(v)) for k, v in runs.items()}}
        spread = max(max(v) - min(v) for v in runs.values())
        rec["spread_of_repeats"] = round(spread, 1)
        rec["resident_over_host"] = round(rec["median"]["resident"] / rec["median"]["host"], 3)
        rec["resident_at_least_as_fast_within_spread"] = rec["median"]["resident"] + spread >= rec["median"]["host"]
        print("epoch", json.dumps(rec), flush=True)
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_region.py measures on a HIP device; none found")
        rec = {"gather": leg_gather, "units": leg_units, "epoch": leg_epoch}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, per call (gather, units); wall time per epoch (epoch)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("gather", "units", "epoch"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_region.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
