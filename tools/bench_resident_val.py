#!/usr/bin/env python3
"""The resident validation (csrc/region_crop.hip, popcorn_amd/data/region.py: ResidentItems, split_census) against the per-item path it
replaces (gather, orbit decision with its synchronisation, fill pair, concatenation, normalisation).  Two legs, each in a child process of
its own under ``timeout -k 10`` (a leg that faults or hangs ends the run; the leg behind it does not start), by the method of
tools/bench_resident_eval.py, over a 2304 x 2560 raster with 400 census units, 5 % clouds in S2 and 3 % gap rows in the descending S1:

  device   ``ops.region_item`` on one crop -- 517 x 389 and 100 x 100, odd origin, with its planned patch table -- next to the launches it
           replaces on the same crop: ``region_gather`` with the orbit, ``region_patch_apply``, ``cat``, ``select_normalize``.  Timer:
           tools/bench_region.py's -- device events around ``--inner`` back-to-back calls behind a spin kernel, ``--reps`` windows, median
           and minimum per call.  Both are compared bit for bit with the filled, normalised item; achieved bytes / s are recorded
  pass     one whole weak-validation pass (model in eval mode under no_grad over every item of the one-unit validation split, then
           ``get_test_metrics``) through ``ResidentItems`` and through the per-item path in the same process, alternating, three repeats
           each after a warm-up per leg; the plan's one-time costs (items, build ms, table entries and bytes)

    python tools/bench_resident_val.py [--out profiles/resident_val_bench.json]

Expectations written down before the first run; the tool states whether each held:
  * device: the launch is one pass, at most 28 B read and 28 B written per pixel, so it does not exceed the chain it replaces (ratio <= 1;
    no absolute figure fixed in advance)
  * pass: both paths share the model's forward, which dominates; the planned pass is not slower than the per-item pass by more than the
    spread of the three repeats"""
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

LEGS = {"device": 240, "pass": 420}                          # seconds of time limit per leg
H, W, UNITS = 2304, 2560, 400
CROPS = {"517x389": (129, 129 + 517, 255, 255 + 389, 0), "100x100": (129, 229, 255, 355, 0)}


def _data():
    from popcorn_amd.data.dataset import SyntheticTestRaster
    return SyntheticTestRaster(H, W, seasons=1, n_regions=UNITS, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.03)


def _bits_equal(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


def leg_device(a):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.region import MODEL_ORDER_BANDS as BAND
    from popcorn_amd.data.region import item_orbit
    data = _data()
    s2, s1, asc, boundary = data.s2, data.s1, data.s1_asc, data.boundary
    rec, held = {}, True
    for name, crop in CROPS.items():
        hc, wc = crop[1] - crop[0], crop[3] - crop[2]
        cen = ops.region_nan_census(s2, s1, boundary, BAND, [crop], s1_asc=asc).cpu()[0].tolist()
        orbit, ok = item_orbit(cen[1], cen[2], 2 * hc * wc, False, True)
        assert ok
        tile = ops.region_gather(s2, s1, boundary, BAND, [crop], s1_asc=asc, orbit=[orbit])
        f2, f1 = tile["S2"].clone(), tile["S1"].clone()
        ops.nan_fill_(f2, tile["data_hw"])
        ops.nan_fill_(f1, tile["data_hw"])
        idx, val, per_item = ops.region_patch_extract(tile, {"S2": f2, "S1": f1})
        n = int(per_item.sum())
        want = ops.select_normalize(torch.cat([f2, f1], 1).contiguous(), tuple(range(6)), stats.MEAN6, stats.STD6)
        want_admin = tile["admin_mask"].clone()
        out = torch.empty(1, 6, hc, wc, device="cuda")
        admin = torch.empty(1, hc, wc, device="cuda")
        norm = torch.empty(1, 6, hc, wc, device="cuda")

        def item():
            ops.region_item(s2, s1, boundary, BAND, crop, stats.MEAN6, stats.STD6, out=out, admin_out=admin, s1_asc=asc, orbit=orbit,
                            table=(idx, val, 0, n))

        def item_plain():
            ops.region_item(s2, s1, boundary, BAND, crop, stats.MEAN6, stats.STD6, out=out, admin_out=admin, s1_asc=asc, orbit=orbit)

        def chain():
            ops.region_gather(s2, s1, boundary, BAND, [crop], out=tile, s1_asc=asc, orbit=[orbit])
            ops.region_patch_apply(idx, val, [0], [n], [(hc, wc)], tile["S2"], tile["S1"], (hc, wc))
            ops.select_normalize(torch.cat([tile["S2"], tile["S1"]], 1), tuple(range(6)), stats.MEAN6, stats.STD6, out=norm)

        item()
        chain()
        same = _bits_equal(out, want) and _bits_equal(norm, want) and _bits_equal(admin, want_admin)
        i_med, i_min, i_host = timed(item, a.reps, a.inner)
        p_med, p_min, _ = timed(item_plain, a.reps, a.inner)
        c_med, c_min, c_host = timed(chain, a.reps, a.inner)
        moved = (4 * 4 + 2 * 4 + 4 + 28) * hc * wc + 8 * n
        r = {"crop": list(crop), "orbit": "asc" if orbit else "desc", "census": cen, "table_entries": n, "table_bytes": 8 * n,
             "region_item_us": [round(i_med, 2), round(i_min, 2)], "region_item_without_table_us": [round(p_med, 2), round(p_min, 2)],
             "replaced_chain_us": [round(c_med, 2), round(c_min, 2)], "item_over_chain": round(i_med / c_med, 4),
             "not_above_chain": i_med <= c_med, "bytes_moved": moved, "gb_per_s_at_median": round(moved / i_med / 1e3, 1),
             "host_enqueue_us": {"region_item": round(i_host, 1), "replaced_chain": round(c_host, 1)}, "bits_equal_filled_item": same}
        held = held and r["not_above_chain"] and same
        rec[name] = r
        print("device", name, json.dumps(r), flush=True)
    rec["expectation_held"] = held
    return rec


def leg_pass(a):
    from popcorn_amd import cli
    from popcorn_amd.data.region import ResidentItems, ResidentRegion, item_orbit, plan_one_unit, split_census
    from popcorn_amd.model.popcorn import POPCORN
    from popcorn_amd.utils.metrics import get_test_metrics
    data = _data()
    region = ResidentRegion.from_synthetic(data, with_asc=True)
    ids, pop = split_census(region.census_idx, region.census_pop, "val")
    plan = plan_one_unit(region.table, ids, pop, region.shape)
    items = ResidentItems(region, plan, seasons=1)
    plan = items.plan
    crops = [tuple(c) + (0,) for c in plan.crops.tolist()]
    torch.manual_seed(40)
    model = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval()
    cidx, y = plan.census_idx.to(region.device), plan.y.to(region.device)

    def host_item(k):
        """gather, the orbit decision with its synchronisation, fill, normalise: what a validation item costs without the plan"""
        crop = crops[k]
        numel = 2 * (crop[1] - crop[0]) * (crop[3] - crop[2])
        g = region.gather([crop], orbit=[0])
        n_desc = int(torch.isnan(g["S1"]).sum())                         # the synchronisation of the 5 % rule
        if item_orbit(n_desc, 0, numel, False, True)[0] == 1:
            g = region.gather([crop], orbit=[1])
            assert item_orbit(n_desc, int(torch.isnan(g["S1"]).sum()), numel, False, True)[1]
        g["census_idx"], g["y"] = cidx[k, :1], y[k, :1]
        return cli.normalize_sample(g, region.device, None, nan_fill=True)

    def validate(feed):
        pred, gt = [], []
        with torch.no_grad():
            for s in feed():
                pred.append(model(s, padding=False)["popcount"])
                gt.append(s["y"])
        pred, gt = torch.cat(pred), torch.cat(gt).float()
        return pred, {k: float(v) for k, v in get_test_metrics(pred, gt, tag="MainCensus_synthetic_fine").items()}

    legs = {"per_item": lambda: (host_item(k) for k in range(len(plan))), "resident_items": lambda: iter(items)}

    def run(feed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = validate(feed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    outs = {k: run(fn)[1] for k, fn in legs.items()}                     # warm-up per leg
    same = _bits_equal(outs["per_item"][0], outs["resident_items"][0]) and outs["per_item"][1] == outs["resident_items"][1]
    ms = {k: [] for k in legs}
    for _ in range(3):
        for k, fn in legs.items():
            ms[k].append(round(run(fn)[0], 2))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    hw = [(c[1] - c[0], c[3] - c[2]) for c in crops]
    rec = {"raster": [H, W], "units": UNITS, "items": len(plan), "dropped": len(items.dropped), "item_hw_min_max": [min(hw), max(hw)],
           "one_time": {"ascending": items.ascending, "table_entries": items.entries, "table_bytes": items.nbytes,
                        "build_ms": round(items.build_ms, 1)},
           "pass_ms": ms, "median_pass_ms": med, "spread_of_repeats_ms": round(spread, 2),
           "ms_per_item": {k: round(v / len(plan), 3) for k, v in med.items()},
           "resident_over_per_item": round(med["resident_items"] / med["per_item"], 3),
           "resident_not_slower_within_spread": med["resident_items"] <= med["per_item"] + spread, "popcounts_bit_equal": same}
    rec["expectation_held"] = rec["resident_not_slower_within_spread"] and same
    print("pass", json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_val_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_resident_val.py measures on a HIP device; none found")
        rec = {"device": leg_device, "pass": leg_pass}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (device); wall time per whole validation pass between device synchronisations (pass)",
           "reps": a.reps, "inner": a.inner}
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ("device", "pass"):
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--out", part]).returncode
            if rc != 0:
                raise SystemExit(f"bench_resident_val.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["device_name"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
