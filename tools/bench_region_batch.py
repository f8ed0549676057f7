#!/usr/bin/env python3
"""One-launch batch assembly (csrc/region_batch.hip, popcorn_amd/data/region.py: ResidentBatchFeed) against the pair of launches and the
torch indexing it replaces.  Three legs, each in a child process of its own under ``timeout -k 10`` (a leg that faults or hangs ends the
run; the legs behind it do not start):

  device  ``ops.region_batch`` next to ``ops.region_gather`` + ``ops.augment_raw`` on the same crops and coins, all three with ``out=``, in
          one process: 2 x 517 x 389 and 64 x 100 x 100, uint16 and fp32 S2, rot 0 and 1 (vertical flip, brightness and gamma drawn).
          Timer: tools/bench_region.py's -- device events around ``--inner`` back-to-back calls enqueued behind a spin kernel, ``--reps``
          windows, median and minimum per call
  host    the host's time to enqueue one batch: iterating ``ResidentBatchFeed`` against iterating ``ResidentRegionFeed`` and calling
          ``prepare_sample_fused`` on every batch -- same plan, same generator seeds, hence the same batches; wall time from the first batch
          request to the last batch handed over (before the device synchronisation), alternating, three repeats each
  epoch   ``Trainer.train_step`` steps per second over whole epochs with ``--resident_assemble`` against the existing resident feed: two
          trainers of one seed over one plan in one process, alternating, three repeats each (wall time from the first batch request to a
          device synchronisation after the last step); then crops per second with ``--resident_pixel_budget 1000000`` against ``-wb 2``

    python tools/bench_region_batch.py [--out profiles/region_batch_bench.json]

Expectations written down before the first run; the tool states whether each held:
  * device: the assembly moves at most 24 B read + 28 B written per output pixel, the pair at most (24 + 28) + (28 + 28), so its device
    time does not exceed the sum of the pair's two launches measured in the same process (ratio <= 1, recorded per shape)
  * host: one wrapper and two allocations (four with labels) instead of two wrappers, six allocations and the torch indexing ops: the
    new feed's enqueue time per batch is below the unfused feed's
  * epoch: the new feed is not slower than the existing one beyond the spread of the repeats.  For the pixel budget no threshold is set:
    a CPU cost model (t = 0.45 ms + 1.11 ns per padded pixel, fitted to the README's config3_regions rows) put the gain in crops per
    second at 1.3 - 1.65x on log-uniform crop sizes; the measured ratio on this plan is recorded next to that figure"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_region import blocky, timed  # noqa: E402

LEGS = {"device": 240, "host": 240, "epoch": 480}           # seconds of time limit per leg
COST_MODEL_GAIN = [1.3, 1.65]                               # the CPU prototype's modelled gain of the pixel budget, crops per second
TRAIN_ARGV = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -wb 2 --resident_region 2304 2560 --resident_units 400 "
              "--save-model no")


def leg_device(a):
    from popcorn_amd import ops
    h, w = 1536, 2048
    g = torch.Generator(device="cuda").manual_seed(1)
    s2f = torch.randint(0, 10000, (1, 4, h, w), generator=g, device="cuda").float()
    s2u = s2f.cpu().to(torch.uint16).cuda()                                    # (the same digital numbers)
    s1 = torch.randn(1, 2, h, w, generator=g, device="cuda") * 5 - 12
    boundary = blocky(h, w, 12, 16, "cuda")
    band = (0, 1, 2, 3, 0, 1)
    out = {}
    hg = torch.Generator().manual_seed(2)
    for B, H, W in ((2, 517, 389), (64, 100, 100)):
        x0 = torch.randint(0, h - H, (B,), generator=hg) | 1                   # odd origins: source rows are not 16-byte aligned
        y0 = torch.randint(0, w - W, (B,), generator=hg) | 1
        crops = [(int(x), int(x) + H, int(y), int(y) + W, 0) for x, y in zip(x0, y0)]
        n_px = B * H * W
        rec = {}
        for name, s2, rd in (("u16", s2u, 4 * 2 + 2 * 4 + 4), ("f32", s2f, 4 * 4 + 2 * 4 + 4)):
            for rot in (0, 1):
                params = {"vflip": True, "hflip": False, "rot": rot, "beta": 1.2, "gamma": 0.9}
                tile = ops.region_gather(s2, s1, boundary, band, crops)
                raw, adm = ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params)
                res = ops.region_batch(s2, s1, boundary, band, crops, params)
                same = bool((res["raw"].view(torch.int32) == raw.view(torch.int32)).all()) and \
                    bool((res["admin_mask"].view(torch.int32) == adm.view(torch.int32)).all())
                g_med, g_min, g_host = timed(lambda: ops.region_gather(s2, s1, boundary, band, crops, out=tile), a.reps, a.inner)
                a_med, a_min, a_host = timed(lambda: ops.augment_raw(tile["S2"], tile["S1"], tile["admin_mask"], params, out=raw, admin_out=adm),
                                             a.reps, a.inner)
                b_med, b_min, b_host = timed(lambda: ops.region_batch(s2, s1, boundary, band, crops, params, out=res), a.reps, a.inner)
                rec[f"{name}_rot{rot}"] = {
                    "region_gather_us": [round(g_med, 2), round(g_min, 2)], "augment_raw_us": [round(a_med, 2), round(a_min, 2)],
                    "region_batch_us": [round(b_med, 2), round(b_min, 2)], "pair_us_median": round(g_med + a_med, 2),
                    "batch_over_pair": round(b_med / (g_med + a_med), 3), "not_above_pair": b_med <= g_med + a_med,
                    "host_enqueue_us": {"region_gather": round(g_host, 1), "augment_raw": round(a_host, 1), "region_batch": round(b_host, 1)},
                    "bytes_per_pixel": {"region_batch": rd + 28, "pair": (rd + 28) + (28 + 28)},
                    "gb_per_s_at_median": round((rd + 28) * n_px / b_med / 1e3, 1), "bits_equal_the_pair": same}
        out[f"{B}x{H}x{W}"] = rec
        print(f"{B}x{H}x{W}", json.dumps(rec), flush=True)
    out["expectation_held"] = all(v["not_above_pair"] and v["bits_equal_the_pair"] for r in out.values() for v in r.values())
    return out


def _trainer(tmp, name, extra=()):
    from popcorn_amd.cli import Trainer, train_parser
    t = Trainer(train_parser().parse_args(TRAIN_ARGV.split() + ["--save_dir", os.path.join(tmp, name)] + list(extra)))
    t.model.train()
    return t


def leg_host(a):
    import random
    from popcorn_amd.cli import prepare_sample_fused
    from popcorn_amd.data.region import ResidentBatchFeed, ResidentRegionFeed
    from popcorn_amd.utils.transform import default_train_transform
    with tempfile.TemporaryDirectory() as tmp:
        t = _trainer(tmp, "host")
        region, plan, transform = t.region, t.region_plan, default_train_transform()

        def unfused():
            n = 0
            for sample in ResidentRegionFeed(region, plan, 2, generator=torch.Generator().manual_seed(7)):
                prepare_sample_fused(sample, transform)
                n += 1
            return n

        def fused():
            return sum(1 for _ in ResidentBatchFeed(region, plan, 2, transform=transform, generator=torch.Generator().manual_seed(7)))

        def run(fn):
            torch.manual_seed(3)
            random.seed(3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            dt = time.perf_counter() - t0                           # the last batch is handed over: the host's share
            torch.cuda.synchronize()
            return dt / n * 1e6, n
        legs = {"region_feed_then_prepare": unfused, "batch_feed": fused}
        for fn in legs.values():
            run(fn)
        runs = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                us, n = run(fn)
                runs[k].append(round(us, 1))
        rec = {"raster": list(region.shape), "crops": len(plan), "batch": 2, "batches_per_epoch": n, "host_us_per_batch": runs,
               "median": {k: float(np.median(v)) for k, v in runs.items()}}
        rec["batch_feed_over_unfused"] = round(rec["median"]["batch_feed"] / rec["median"]["region_feed_then_prepare"], 3)
        rec["expectation_held"] = rec["median"]["batch_feed"] < rec["median"]["region_feed_then_prepare"]
        print("host", json.dumps(rec), flush=True)
        return rec


def leg_epoch(a):
    with tempfile.TemporaryDirectory() as tmp:
        trainers = {"resident": _trainer(tmp, "resident"), "assemble": _trainer(tmp, "assemble", ["--resident_assemble"]),
                    "pixel_budget": _trainer(tmp, "budget", ["--resident_pixel_budget", "1000000"])}

        def epochs(t):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = crops = 0
            for _ in range(a.epochs):
                for sample in t._resident_feed:
                    t.train_step(sample)
                    steps += 1
                    crops += sample["admin_mask"].shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return steps / dt, crops / dt, steps, crops
        for t in trainers.values():                                 # warm-up: allocator, every batch shape once
            epochs(t)
        sps, cps = {k: [] for k in trainers}, {k: [] for k in trainers}
        count = {}
        for _ in range(3):
            for k, t in trainers.items():
                s, c, steps, crops = epochs(t)
                sps[k].append(round(s, 1))
                cps[k].append(round(c, 1))
                count[k] = {"steps": steps, "crops": crops}
        plan = trainers["resident"].region_plan
        med = {k: float(np.median(v)) for k, v in sps.items()}
        medc = {k: float(np.median(v)) for k, v in cps.items()}
        spread = max(max(sps[k]) - min(sps[k]) for k in ("resident", "assemble"))
        sizes = [len(b) for b in trainers["pixel_budget"]._resident_feed.last_batches]
        rec = {"raster": list(trainers["resident"].region.shape), "crops": len(plan), "epochs_per_repeat": a.epochs, "counts": count,
               "steps_per_s": sps, "crops_per_s": cps, "median_steps_per_s": med, "median_crops_per_s": medc,
               "spread_of_repeats_steps_per_s": round(spread, 1), "assemble_over_resident": round(med["assemble"] / med["resident"], 3),
               "assemble_not_slower_within_spread": med["assemble"] + spread >= med["resident"],
               "pixel_budget": {"budget": 1000000, "batches_last_epoch": len(sizes), "largest_batch": max(sizes),
                                "crops_per_s_over_wb2": round(medc["pixel_budget"] / medc["resident"], 3),
                                "cost_model_gain": COST_MODEL_GAIN}}
        rec["expectation_held"] = rec["assemble_not_slower_within_spread"]
        print("epoch", json.dumps(rec), flush=True)
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=5, help="epochs per repeat of the epoch leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_batch_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_region_batch.py measures on a HIP device; none found")
        rec = {"device": leg_device, "host": leg_host, "epoch": leg_epoch}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (device); wall time per batch handed over (host); wall time per repeat of whole epochs (epoch)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("device", "host", "epoch"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--epochs", str(a.epochs), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_region_batch.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["device_name"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
