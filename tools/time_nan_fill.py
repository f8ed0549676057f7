#!/usr/bin/env python3
"""Device time of the NaN fill (ops.nan_fill_, csrc/nan_fill.hip) on inference windows and a training region batch, under a graph-free
event timer: every repetition restores the NaN input with a copy OUTSIDE the timed interval, then times the fill alone (count, rows,
columns, combine launches).

  * a 2048 x 2048 window, S2 (4 bands) + S1 (2 bands) filled separately as the loader does: NaN-free, ~1 % scattered NaNs, ~5 % clouds
    (S2 cloud discs across all bands, S1 orbit-gap rows);
  * a B = 2 region batch of 1030 x 770 (ragged extents: the second item 900 x 700), S2 + S1, ~5 % clouds.

    python tools/time_nan_fill.py [--reps 50] [--out profiles/r7_nan_fill.json]
    python tools/time_nan_fill.py --scipy-only --out profiles/r7_nan_fill.json   # CPU host: adds scipy griddata "nearest" seconds
                                                                                 # (the reference's interpolate_nan) for the same arrays

The arrays are seeded, so both runs see the same data."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def cases():
    from popcorn_amd.data.dataset import cloud_mask, gap_rows
    out = {}
    for name, frac in (("window_2048_nan_free", 0.0), ("window_2048_scattered_1pct", 0.01), ("window_2048_clouds_5pct", 0.05)):
        g = torch.Generator().manual_seed(700)
        s2 = torch.randint(0, 10000, (4, 2048, 2048), generator=g).float()
        s1 = torch.randn(2, 2048, 2048, generator=g) * 4 - 12
        if name.endswith("scattered_1pct"):
            s2[torch.rand(4, 2048, 2048, generator=g) < frac] = float("nan")
            s1[torch.rand(2, 2048, 2048, generator=g) < frac] = float("nan")
        elif frac > 0:
            s2[:, cloud_mask(2048, 2048, frac, g)] = float("nan")
            s1[:, gap_rows(2048, 0.04, g)] = float("nan")
        out[name] = {"S2": (s2[None], None), "S1": (s1[None], None)}
    g = torch.Generator().manual_seed(701)
    hw = [(1030, 770), (900, 700)]
    s2 = torch.zeros(2, 4, 1030, 770)
    s1 = torch.zeros(2, 2, 1030, 770)
    for b, (h, w) in enumerate(hw):
        s2[b, :, :h, :w] = torch.randint(0, 10000, (4, h, w), generator=g).float()
        s1[b, :, :h, :w] = torch.randn(2, h, w, generator=g) * 4 - 12
        s2[b, :, :h, :w][:, cloud_mask(h, w, 0.05, g)] = float("nan")
        s1[b, :, :h, :w][:, gap_rows(h, 0.02, g)] = float("nan")
    out["regions_2x1030x770_clouds_5pct"] = {"S2": (s2, hw), "S1": (s1, hw)}
    return out


def time_device(x, hw, reps):
    from popcorn_amd import ops
    src = x.cuda()
    work = torch.empty_like(src)
    hw_dev = None if hw is None else torch.tensor(hw, dtype=torch.int32).cuda()
    ts = []
    for r in range(reps + 3):
        work.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.nan_fill_(work, hw_dev)
        b.record()
        b.synchronize()
        if r >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def time_scipy(x, hw):
    from scipy.interpolate import griddata
    tot = 0.0
    for b in range(x.shape[0]):
        h, w = (x.shape[2], x.shape[3]) if hw is None else hw[b]
        a = x[b, :, :h, :w].numpy().copy()
        nan = np.isnan(a)
        if not nan.any():
            continue
        t0 = time.perf_counter()
        known, missing = np.where(~nan), np.where(nan)            # interpolate_nan (data/PopulationDataset.py:526-551)
        a[missing] = griddata(np.vstack(known).T, a[known], np.vstack(missing).T, method="nearest")
        tot += time.perf_counter() - t0
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scipy-only", action="store_true")
    a = ap.parse_args()
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            res = json.load(fh)
    res.setdefault("cases", {})
    for name, mods in cases().items():
        rec = res["cases"].setdefault(name, {})
        for mod, (x, hw) in mods.items():
            r = rec.setdefault(mod, {"shape": list(x.shape), "nan_fraction": float(torch.isnan(x).float().mean())})
            if a.scipy_only:
                r["scipy_griddata_s"] = round(time_scipy(x, hw), 3)
            else:
                med, mn = time_device(x, hw, a.reps)
                r["device_us_median"], r["device_us_min"] = round(med, 1), round(mn, 1)
            print(name, mod, json.dumps(r), flush=True)
        if not a.scipy_only:
            rec["device_us_total_median"] = round(sum(v["device_us_median"] for k, v in rec.items() if isinstance(v, dict)), 1)
    if not a.scipy_only:
        res["device"] = torch.cuda.get_device_name(0)
        res["reps"] = a.reps
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
