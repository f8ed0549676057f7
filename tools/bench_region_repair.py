#!/usr/bin/env python3
"""The resident repair (csrc/region_repair.hip, popcorn_amd/data/region.py: plan_repair) against the per-step fill it replaces.  Two legs,
each in a child process of its own under ``timeout -k 10`` (a leg that faults or hangs ends the run; the leg behind it does not start):

  device  ``ops.region_patch_apply`` next to the ``fill_sample_`` pair (``ops.nan_fill_`` on S2 and on S1) on the same gathered batch, in one
          process: 2 x 1030 x 770 and 2 x 517 x 389, fp32 S2 with 5 % clouds, descending S1 with gap rows.  The fill works in place and a
          filled tile has nothing left to fill, so it is timed as (restore + fill) minus (restore alone), the restore being two
          ``copy_`` calls from the gathered tile.  Timer: tools/bench_region.py's -- device events around ``--inner`` back-to-back calls
          enqueued behind a spin kernel, ``--reps`` windows, median and minimum per call.  The patched tile is compared with the filled
          one bit for bit; table entries, bytes and the build time of the table are recorded
  epoch   ``Trainer.train_step`` steps per second over whole epochs: ``--nan_fill``, ``--resident_repair`` and a NaN-free region of the
          same plan -- three trainers of one seed in one process, alternating, three repeats each (wall time from the first batch request
          to a device synchronisation after the last step); the repair's one-time costs as the trainer prints them

    python tools/bench_region_repair.py [--out profiles/region_repair_bench.json]

Expectations written down before the first run; the tool states whether each held:
  * device: the application moves about 12 B per patched entry against four passes over each tensor of the tile, so it does not exceed
    the pair it replaces (ratio <= 1, recorded per shape; no absolute figure fixed in advance)
  * epoch: the repaired feed is not slower than the per-step fill beyond the spread of the repeats; its distance to the NaN-free leg is
    recorded without a threshold"""
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

LEGS = {"device": 300, "epoch": 540}                        # seconds of time limit per leg
TRAIN_ARGV = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -wb 2 --resident_region 2304 2560 --resident_units 400 "
              "--save-model no")


def leg_device(a):
    from popcorn_amd import ops
    from popcorn_amd.data.dataset import cloud_mask, gap_rows
    h, w = 2304, 2560
    g = torch.Generator(device="cuda").manual_seed(1)
    s2 = torch.randint(0, 10000, (1, 4, h, w), generator=g, device="cuda").float()
    s1 = torch.randn(1, 2, h, w, generator=g, device="cuda") * 5 - 12
    hg = torch.Generator().manual_seed(2)
    s2[0][:, cloud_mask(h, w, 0.05, hg).cuda()] = float("nan")
    s1[0][:, gap_rows(h, 0.03, hg).cuda()] = float("nan")
    boundary = blocky(h, w, 12, 16, "cuda")
    band = (0, 1, 2, 3, 0, 1)
    out = {}
    for B, H, W in ((2, 1030, 770), (2, 517, 389)):
        x0 = torch.randint(0, h - H, (B,), generator=hg) | 1                   # odd origins: source rows are not 16-byte aligned
        y0 = torch.randint(0, w - W, (B,), generator=hg) | 1
        crops = [(int(x), int(x) + H, int(y), int(y) + W, 0) for x, y in zip(x0, y0)]
        tile = ops.region_gather(s2, s1, boundary, band, crops)
        hw = tile["data_hw"]
        f2, f1 = tile["S2"].clone(), tile["S1"].clone()
        ops.nan_fill_(f2, hw)
        ops.nan_fill_(f1, hw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx, val, per_item = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
        torch.cuda.synchronize()
        extract_ms = (time.perf_counter() - t0) * 1e3
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(per_item, 0)])
        count, item_hw = per_item.tolist(), [(H, W)] * B
        w2, w1 = tile["S2"].clone(), tile["S1"].clone()

        def restore():
            w2.copy_(tile["S2"])
            w1.copy_(tile["S1"])

        def restore_fill():
            restore()
            ops.nan_fill_(w2, hw)
            ops.nan_fill_(w1, hw)

        def apply():
            ops.region_patch_apply(idx, val, off[:-1], count, item_hw, w2, w1, (H, W))
        restore()
        apply()
        same = bool((w2.view(torch.int32) == f2.view(torch.int32)).all()) and bool((w1.view(torch.int32) == f1.view(torch.int32)).all())
        r_med, r_min, _ = timed(restore, a.reps, a.inner)
        rf_med, rf_min, rf_host = timed(restore_fill, a.reps, a.inner)
        restore()
        p_med, p_min, p_host = timed(apply, a.reps, a.inner)
        fill_med = rf_med - r_med
        entries = int(off[-1])
        rec = {"nan_entries": {"S2": int(torch.isnan(tile["S2"]).sum()), "S1": int(torch.isnan(tile["S1"]).sum())},
               "table_entries": entries, "table_bytes": 8 * entries, "extract_ms": round(extract_ms, 2),
               "restore_us": [round(r_med, 2), round(r_min, 2)], "restore_plus_fill_us": [round(rf_med, 2), round(rf_min, 2)],
               "fill_pair_us_median": round(fill_med, 2), "patch_apply_us": [round(p_med, 2), round(p_min, 2)],
               "apply_over_fill_pair": round(p_med / fill_med, 4), "not_above_fill_pair": p_med <= fill_med,
               "host_enqueue_us": {"restore_plus_fill": round(rf_host, 1), "patch_apply": round(p_host, 1)},
               "gb_per_s_at_median": round(12 * entries / p_med / 1e3, 1), "bits_equal_the_fill": same}
        out[f"{B}x{H}x{W}"] = rec
        print(f"{B}x{H}x{W}", json.dumps(rec), flush=True)
    out["expectation_held"] = all(v["not_above_fill_pair"] and v["bits_equal_the_fill"] for v in out.values())
    return out


def _trainer(tmp, name, extra=()):
    from popcorn_amd.cli import Trainer, train_parser
    t = Trainer(train_parser().parse_args(TRAIN_ARGV.split() + ["--save_dir", os.path.join(tmp, name)] + list(extra)))
    t.model.train()
    return t


def leg_epoch(a):
    with tempfile.TemporaryDirectory() as tmp:
        clouds = ["--nan_clouds", "0.05"]
        trainers = {"nan_fill": _trainer(tmp, "fill", clouds + ["--nan_fill"]), "resident_repair": _trainer(tmp, "repair", clouds + ["--resident_repair"]),
                    "nan_free": _trainer(tmp, "free")}
        plans = [t.region_plan for t in trainers.values()]
        assert all(p == plans[0] for p in plans), "the three legs do not share a plan"

        def epochs(t):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps = 0
            for _ in range(a.epochs):
                for sample in t._resident_feed:
                    t.train_step(sample)
                    steps += 1
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0), steps
        for t in trainers.values():                                 # warm-up: allocator, every batch shape once
            epochs(t)
        sps = {k: [] for k in trainers}
        for _ in range(3):
            for k, t in trainers.items():
                s, steps = epochs(t)
                sps[k].append(round(s, 1))
        med = {k: float(np.median(v)) for k, v in sps.items()}
        spread = max(max(sps[k]) - min(sps[k]) for k in ("nan_fill", "resident_repair"))
        r = trainers["resident_repair"].region_repair
        rec = {"raster": list(trainers["nan_fill"].region.shape), "crops": len(plans[0]), "epochs_per_repeat": a.epochs,
               "steps_per_repeat": steps, "steps_per_s": sps, "median_steps_per_s": med, "spread_of_repeats_steps_per_s": round(spread, 1),
               "repair_over_nan_fill": round(med["resident_repair"] / med["nan_fill"], 3),
               "repair_over_nan_free": round(med["resident_repair"] / med["nan_free"], 3),
               "repair_not_slower_within_spread": med["resident_repair"] + spread >= med["nan_fill"],
               "one_time": {"items": r.n, "dropped": len(r.dropped), "ascending": r.ascending, "table_entries": r.entries,
                            "table_bytes": r.nbytes, "build_ms": round(r.build_ms, 1)}}
        rec["expectation_held"] = rec["repair_not_slower_within_spread"]
        print("epoch", json.dumps(rec), flush=True)
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3, help="epochs per repeat of the epoch leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_repair_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_region_repair.py measures on a HIP device; none found")
        rec = {"device": leg_device, "epoch": leg_epoch}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (device); wall time per repeat of whole epochs (epoch)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("device", "epoch"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--epochs", str(a.epochs), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_region_repair.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["device_name"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
