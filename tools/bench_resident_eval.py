#!/usr/bin/env python3
"""The resident evaluation (csrc/region_crop.hip, popcorn_amd/data/region.py: ResidentWindows) against the per-window path it replaces
(eval.raw_window_input: clone + cat + fill pair + orbit synchronisation + normalise).  Two legs, each in a child process of its own under
``timeout -k 10`` (a leg that faults or hangs ends the run; the leg behind it does not start), by the method of tools/bench_region_repair.py:

  device   ``ops.region_window`` on one 2048 x 2048 window of a 2304 x 2560 raster (fp32 S2 with 5 % clouds, 3 % gap rows in the descending
           S1, odd origin) next to (a) the launches it replaces on the same window -- ``region_gather``, ``region_patch_apply``, ``cat``,
           ``select_normalize`` -- and (b) the fill pair (``ops.nan_fill_`` on S2 and on S1, timed as restore + fill minus the restore alone).
           Timer: tools/bench_region.py's -- device events around ``--inner`` back-to-back calls behind a spin kernel, ``--reps`` windows,
           median and minimum per call.  The window is compared with ``raw_window_input`` bit for bit; achieved bytes / s are recorded
  windows  ``evaluate_raster`` windows per second over the same raster (patchsize 2048, overlap 128) for M = 1 and M = 5 members, three
           legs in one process, alternating, three repeats each after a warm-up per leg: the per-window ``raw=True`` path, ``ResidentWindows``,
           and a pre-normalised NaN-free tensor as the floor; the plan's one-time costs (build ms, table entries and bytes)

    python tools/bench_resident_eval.py [--out profiles/resident_eval_bench.json]

Expectations written down before the first run; the tool states whether each held:
  * device: the launch reads 4 * ps^2 * 4 + 2 * ps^2 * 4 bytes and writes 24 * ps^2, once each, so it does not exceed the chain it replaces
    (ratio <= 1; both times, the ratio to the fill pair and the achieved bytes / s recorded; no absolute figure fixed in advance)
  * windows: the resident leg is not slower than the per-window leg beyond the spread of the repeats; its distance to the floor is recorded"""
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

from bench_region import timed  # noqa: E402

LEGS = {"device": 300, "windows": 540}                       # seconds of time limit per leg
H, W, PS, OV = 2304, 2560, 2048, 128


def _data():
    from popcorn_amd.data.dataset import SyntheticTestRaster
    return SyntheticTestRaster(H, W, seasons=1, n_regions=400, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.03)


def leg_device(a):
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.region import MODEL_ORDER_BANDS as BAND
    data = _data()
    s2, s1, asc, boundary = data.s2, data.s1, data.s1_asc, data.boundary
    x, y, ps = 129, 255, PS                                               # odd origin: source rows are not 16-byte aligned
    crop = [(x, x + ps, y, y + ps, 0)]
    want, orbit_name = E.raw_window_input(data(x, y, 0, ps), False)
    orbit = int(orbit_name == "asc")
    tile = ops.region_gather(s2, s1, boundary, BAND, crop, s1_asc=asc, orbit=[orbit])
    hw = tile["data_hw"]
    f2, f1 = tile["S2"].clone(), tile["S1"].clone()
    ops.nan_fill_(f2, hw)
    ops.nan_fill_(f1, hw)
    idx, val, per_item = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
    n = int(per_item.sum())
    out = torch.empty(1, 6, ps, ps, device="cuda")
    w2, w1 = tile["S2"].clone(), tile["S1"].clone()
    norm = torch.empty(1, 6, ps, ps, device="cuda")

    def window():
        ops.region_window(s2, s1, BAND, (x, y, 0), ps, stats.MEAN6, stats.STD6, out=out, s1_asc=asc, orbit=orbit, table=(idx, val, 0, n))

    def window_plain():
        ops.region_window(s2, s1, BAND, (x, y, 0), ps, stats.MEAN6, stats.STD6, out=out, s1_asc=asc, orbit=orbit)

    def chain():
        ops.region_gather(s2, s1, boundary, BAND, crop, out=tile, s1_asc=asc, orbit=[orbit])
        ops.region_patch_apply(idx, val, [0], [n], [(ps, ps)], tile["S2"], tile["S1"], (ps, ps))
        ops.select_normalize(torch.cat([tile["S2"], tile["S1"]], 1), tuple(range(6)), stats.MEAN6, stats.STD6, out=norm)

    def restore():
        w2.copy_(tile_raw[0])                                             # (the gathered, unrepaired window: the fill has work to do again)
        w1.copy_(tile_raw[1])

    def restore_fill():
        restore()
        ops.nan_fill_(w2, hw)
        ops.nan_fill_(w1, hw)

    window()
    chain()
    same = bool((out.view(torch.int32) == want.view(torch.int32)).all()) and bool((norm.view(torch.int32) == want.view(torch.int32)).all())
    tile_raw = ops.region_gather(s2, s1, boundary, BAND, crop, s1_asc=asc, orbit=[orbit])
    tile_raw = (tile_raw["S2"], tile_raw["S1"])
    w_med, w_min, w_host = timed(window, a.reps, a.inner)
    p_med, p_min, _ = timed(window_plain, a.reps, a.inner)
    c_med, c_min, c_host = timed(chain, a.reps, a.inner)
    r_med, r_min, _ = timed(restore, a.reps, a.inner)
    rf_med, rf_min, rf_host = timed(restore_fill, max(3, a.reps // 3), max(1, a.inner // 5))
    fill_med = rf_med - r_med
    moved = (4 * 4 + 2 * 4 + 24) * ps * ps + 8 * n
    rec = {"window": [x, y, 0, ps], "orbit": orbit_name, "nan_entries": {"S2": int(torch.isnan(tile_raw[0]).sum()), "S1": int(torch.isnan(tile_raw[1]).sum())},
           "table_entries": n, "table_bytes": 8 * n,
           "region_window_us": [round(w_med, 2), round(w_min, 2)], "region_window_without_table_us": [round(p_med, 2), round(p_min, 2)],
           "replaced_chain_us": [round(c_med, 2), round(c_min, 2)], "restore_us": [round(r_med, 2), round(r_min, 2)],
           "restore_plus_fill_us": [round(rf_med, 2), round(rf_min, 2)], "fill_pair_us_median": round(fill_med, 2),
           "window_over_chain": round(w_med / c_med, 4), "window_over_fill_pair": round(w_med / fill_med, 5),
           "not_above_chain": w_med <= c_med, "bytes_moved": moved, "gb_per_s_at_median": round(moved / w_med / 1e3, 1),
           "host_enqueue_us": {"region_window": round(w_host, 1), "replaced_chain": round(c_host, 1), "restore_plus_fill": round(rf_host, 1)},
           "bits_equal_raw_window_input": same}
    rec["expectation_held"] = rec["not_above_chain"] and same
    print("device", json.dumps(rec), flush=True)
    return rec


def leg_windows(a):
    from popcorn_amd import eval as E
    from popcorn_amd.data import stats
    from popcorn_amd.data.region import ResidentRegion, ResidentWindows
    from popcorn_amd.model.popcorn import POPCORN
    data = _data()
    region = ResidentRegion.from_synthetic(data, with_asc=True)
    feed = ResidentWindows(region, PS, OV)
    mean = torch.tensor(stats.MEAN6, device="cuda").view(1, 6, 1, 1)
    std = torch.tensor(stats.STD6, device="cuda").view(1, 6, 1, 1)
    floor = ((torch.nan_to_num(torch.cat([data.s2, data.s1], 1), nan=0.0) - mean) / std).contiguous()      # pre-normalised, NaN-free
    nwin = int(feed.idx.shape[0])
    rec = {"raster": [H, W], "patchsize": PS, "overlap": OV, "windows": nwin,
           "one_time": {"ascending": feed.ascending, "table_entries": feed.entries, "table_bytes": feed.nbytes, "build_ms": round(feed.build_ms, 1)}}
    models = []
    for k in range(5):
        torch.manual_seed(40 + k)
        models.append(POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval())
    legs = {"per_window_raw": lambda ms: E.evaluate_raster(ms, data.raster, PS, OV, False, raw=True),
            "resident_windows": lambda ms: E.evaluate_raster(ms, feed, PS, OV, False),
            "prenormalised_floor": lambda ms: E.evaluate_raster(ms, floor, PS, OV, False)}
    held = True
    for M in (1, 5):
        ms = models[:M]

        def run(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            maps = fn(ms)
            torch.cuda.synchronize()
            return nwin / (time.perf_counter() - t0), maps
        outs = {k: run(fn)[1] for k, fn in legs.items()}                 # warm-up per leg and shape
        same = all(bool((a_.view(torch.int32) == b_.view(torch.int32)).all()) for a_, b_ in zip(outs["per_window_raw"], outs["resident_windows"]))
        wps = {k: [] for k in legs}
        for _ in range(3):
            for k, fn in legs.items():
                wps[k].append(round(run(fn)[0], 3))
        med = {k: float(np.median(v)) for k, v in wps.items()}
        spread = max(max(wps[k]) - min(wps[k]) for k in ("per_window_raw", "resident_windows"))
        r = {"windows_per_s": wps, "median_windows_per_s": med, "spread_of_repeats": round(spread, 3),
             "resident_over_per_window": round(med["resident_windows"] / med["per_window_raw"], 3),
             "resident_over_floor": round(med["resident_windows"] / med["prenormalised_floor"], 3),
             "ms_per_window": {k: round(1e3 / v, 2) for k, v in med.items()},
             "resident_not_slower_within_spread": med["resident_windows"] + spread >= med["per_window_raw"], "maps_bit_equal": same}
        held = held and r["resident_not_slower_within_spread"] and same
        rec[f"M{M}"] = r
        print(f"windows M={M}", json.dumps(r), flush=True)
    rec["expectation_held"] = held
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_eval_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_resident_eval.py measures on a HIP device; none found")
        rec = {"device": leg_device, "windows": leg_windows}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (device); wall time per whole evaluate_raster call between device synchronisations (windows)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("device", "windows"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_resident_eval.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["device_name"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
