#!/usr/bin/env python3
"""The resident atlas (csrc/region_atlas.hip, popcorn_amd/data/atlas.py) against what it replaces.  Three legs, each in a child process of
its own under ``timeout -k 10`` (a leg that faults or hangs ends the run; the legs behind it do not start):

  device  ``ops.atlas_gather`` / ``ops.atlas_batch`` next to ``ops.region_gather`` / ``ops.region_batch`` on the same crops, all crops in
          ONE region of a three-region atlas so that both can run: 2 x 517 x 389 and 64 x 100 x 100, uint16 S2, rot 0 and 1, all with
          ``out=``, in one process.  The single-region code is untouched by the atlas, so its figure is the parent commit's.
          Timer: tools/bench_region.py's -- device events around ``--inner`` back-to-back calls enqueued behind a spin kernel,
          ``--reps`` windows, median and minimum per call.  Spread = the largest (median - minimum) of the two calls compared
  mixed   a batch whose crops come from three regions: ONE ``ops.atlas_batch`` against what a user does today -- one
          ``ops.region_batch`` per region present (at the batch tile), then ``torch.cat`` of the parts and an index to restore the order;
          device time (same timer) and host enqueue time per batch
  epoch   ``Trainer.train()``-style steps per second over three regions with ``--resident_assemble`` against the same three regions
          through ``RegionFeed`` over a host ``ConcatDataset`` of datasets that slice the same items out of host copies of the rasters
          (tools/bench_region.py: HostSliceDataset); same trainer, alternating, three repeats each

    python tools/bench_atlas.py [--out profiles/atlas_bench.json]

Expectations written down before the first run; the tool states whether each held:
  * device: the only added work is one descriptor read per workgroup, so the atlas launch lies within the spread of the repeats of the
    single-region launch (|median difference| <= spread), per shape and rotation
  * mixed: one atlas launch does not exceed the launches it replaces, in device time and in host enqueue time
  * epoch: no threshold; the ratio atlas / host loader is reported next to section 15's single-region ratio (1.19 - 1.21)"""
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

from bench_region import HostSliceDataset, blocky, timed  # noqa: E402

LEGS = {"device": 240, "mixed": 240, "epoch": 480}          # seconds of time limit per leg
SHAPES = ((1536, 2048), (1200, 1500), (1024, 1280))
BAND = (0, 1, 2, 3, 0, 1)
SINGLE_REGION_RATIO = [1.19, 1.21]                          # section 15: resident feed over the host loader, one region
TRAIN_ARGV = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -wb 2 --resident_region 1536 2048 1200 1500 1024 1280 "
              "--resident_units 200 --save-model no")


def _regions():
    g = torch.Generator(device="cuda").manual_seed(1)
    out = []
    for k, (h, w) in enumerate(SHAPES):
        s2 = torch.randint(0, 10000, (1, 4, h, w), generator=g, device="cuda").cpu().to(torch.uint16).cuda()
        s1 = torch.randn(1, 2, h, w, generator=g, device="cuda") * 5 - 12
        out.append({"s2": s2, "s1": s1, "boundary": blocky(h, w, 12, 16, "cuda"), "band_sel": BAND})
    return out


def _crops(hg, shape, B, H, W):
    x0 = torch.randint(0, shape[0] - H, (B,), generator=hg) | 1     # odd origins: source rows are not 16-byte aligned
    y0 = torch.randint(0, shape[1] - W, (B,), generator=hg) | 1
    return [(int(x), int(x) + H, int(y), int(y) + W, 0) for x, y in zip(x0, y0)]


def _same(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


def leg_device(a):
    from popcorn_amd import ops
    regions = _regions()
    atlas = ops.AtlasHandle(regions)
    r = regions[0]
    hg = torch.Generator().manual_seed(2)
    out = {}
    for B, H, W in ((2, 517, 389), (64, 100, 100)):
        crops, ro = _crops(hg, SHAPES[0], B, H, W), [0] * B
        rec = {}
        one, many = ops.region_gather(r["s2"], r["s1"], r["boundary"], BAND, crops), ops.atlas_gather(atlas, ro, crops)
        same = all(_same(one[k], many[k]) for k in one)
        s_med, s_min, _ = timed(lambda: ops.region_gather(r["s2"], r["s1"], r["boundary"], BAND, crops, out=one), a.reps, a.inner)
        m_med, m_min, _ = timed(lambda: ops.atlas_gather(atlas, ro, crops, out=many), a.reps, a.inner)
        spread = max(s_med - s_min, m_med - m_min)
        rec["gather"] = {"region_gather_us": [round(s_med, 2), round(s_min, 2)], "atlas_gather_us": [round(m_med, 2), round(m_min, 2)],
                         "spread_us": round(spread, 2), "within_spread": abs(m_med - s_med) <= spread, "bits_equal": same}
        for rot in (0, 1):
            params = {"vflip": True, "hflip": False, "rot": rot, "beta": 1.2, "gamma": 0.9}
            one = ops.region_batch(r["s2"], r["s1"], r["boundary"], BAND, crops, params)
            many = ops.atlas_batch(atlas, ro, crops, params)
            same = all(_same(one[k], many[k]) for k in one)
            s_med, s_min, _ = timed(lambda: ops.region_batch(r["s2"], r["s1"], r["boundary"], BAND, crops, params, out=one), a.reps, a.inner)
            m_med, m_min, _ = timed(lambda: ops.atlas_batch(atlas, ro, crops, params, out=many), a.reps, a.inner)
            spread = max(s_med - s_min, m_med - m_min)
            rec[f"batch_rot{rot}"] = {"region_batch_us": [round(s_med, 2), round(s_min, 2)], "atlas_batch_us": [round(m_med, 2), round(m_min, 2)],
                                      "spread_us": round(spread, 2), "atlas_over_region": round(m_med / s_med, 3),
                                      "within_spread": abs(m_med - s_med) <= spread, "bits_equal": same}
        out[f"{B}x{H}x{W}"] = rec
        print(f"{B}x{H}x{W}", json.dumps(rec), flush=True)
    out["expectation_held"] = all(v["within_spread"] and v["bits_equal"] for r_ in out.values() for v in r_.values())
    return out


def leg_mixed(a):
    from popcorn_amd import ops
    regions = _regions()
    atlas = ops.AtlasHandle(regions)
    hg = torch.Generator().manual_seed(3)
    out = {}
    for B, H, W in ((6, 389, 301), (63, 100, 100)):
        ro = [i % 3 for i in range(B)]
        crops = [_crops(hg, SHAPES[k], 1, H - 4 * k, W - 8 * k)[0] for k in ro]           # a size per region: the parts need the batch tile
        rows = [[b for b in range(B) if ro[b] == k] for k in range(3)]
        back = torch.argsort(torch.tensor([b for part in rows for b in part])).cuda()
        rec = {}
        for rot in (0, 1):
            params = {"vflip": True, "hflip": False, "rot": rot, "beta": 1.2, "gamma": 0.9}

            def today():
                parts = [ops.region_batch(regions[k]["s2"], regions[k]["s1"], regions[k]["boundary"], BAND, [crops[b] for b in rows[k]], params,
                                          hw=(H, W)) for k in range(3)]
                return {key: torch.cat([p[key] for p in parts])[back] for key in ("raw", "admin_mask")}

            want, got = today(), ops.atlas_batch(atlas, ro, crops, params)
            same = all(_same(want[k], got[k]) for k in want)
            t_med, t_min, t_host = timed(today, a.reps, a.inner)
            m_med, m_min, m_host = timed(lambda: ops.atlas_batch(atlas, ro, crops, params, out=got), a.reps, a.inner)
            rec[f"rot{rot}"] = {"per_region_then_cat_us": [round(t_med, 2), round(t_min, 2)], "atlas_batch_us": [round(m_med, 2), round(m_min, 2)],
                                "atlas_over_today": round(m_med / t_med, 3), "host_enqueue_us": {"today": round(t_host, 1), "atlas": round(m_host, 1)},
                                "not_above_device": m_med <= t_med, "not_above_host": m_host <= t_host, "bits_equal": same}
        out[f"{B}x{H}x{W}"] = rec
        print(f"{B}x{H}x{W}", json.dumps(rec), flush=True)
    out["expectation_held"] = all(v["not_above_device"] and v["not_above_host"] and v["bits_equal"] for r_ in out.values() for v in r_.values())
    return out


def leg_epoch(a):
    from popcorn_amd.cli import Trainer, train_parser
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.feed import RegionFeed
    with tempfile.TemporaryDirectory() as tmp:
        t = Trainer(train_parser().parse_args(TRAIN_ARGV.split() + ["--resident_assemble", "--save_dir", tmp]))
        t.model.train()
        plan = t.region_plan
        host = torch.utils.data.ConcatDataset([HostSliceDataset(r, plan.member(k)[1]) for k, r in enumerate(t.regions)])
        loader = torch.utils.data.DataLoader(host, batch_size=2, shuffle=True, num_workers=0, collate_fn=Population_Dataset_collate_fn,
                                             drop_last=True)
        feeds = {"atlas": lambda: t._resident_feed, "host": lambda: RegionFeed(loader, t.device)}

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
        rec = {"rasters": [list(r.shape) for r in t.regions], "crops": len(plan), "crops_per_region": [len(plan.member(k)[0]) for k in range(3)],
               "batch": 2, "steps_per_epoch": n, "steps_per_s": runs, "median": {k: float(np.median(v)) for k, v in runs.items()}}
        rec["spread_of_repeats"] = round(max(max(v) - min(v) for v in runs.values()), 1)
        rec["atlas_over_host"] = round(rec["median"]["atlas"] / rec["median"]["host"], 3)
        rec["single_region_ratio_section_15"] = SINGLE_REGION_RATIO
        print("epoch", json.dumps(rec), flush=True)
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atlas_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_atlas.py measures on a HIP device; none found")
        rec = {"device": leg_device, "mixed": leg_mixed, "epoch": leg_epoch}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (device, mixed); host seconds per enqueued call (mixed); wall time per epoch (epoch)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("device", "mixed", "epoch"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_atlas.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
