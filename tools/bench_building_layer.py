#!/usr/bin/env python3
"""What a shipped building layer costs where it is moved and saves where it replaces the frozen extractor.  Five
legs, each in a child process of its own under ``timeout -k 10`` (a leg that faults or hangs ends the run; the leg behind it does not
start), by the method of tools/bench_resident_eval.py:

  launches  ``ops.region_gather`` and ``ops.region_batch`` (rot 0 and rot 1) with and without ``buildings=`` at 2 x 517 x 389 and
            64 x 100 x 100 crops of a 1536 x 2048 raster, uint16 and fp32 S2, odd origins.  Timer: tools/bench_region.py's -- device events
            around ``--inner`` back-to-back calls behind a spin kernel, ``--reps`` windows, median and minimum per call
  window    one ``ops.region_window`` launch of a 2048 x 2048 window of a 2304 x 2560 raster with and without the layer, same timer
  steps     a per-launch-engine training step (POPCORN_NATIVE_STEP=0 for both sides) of a model built without ``sentinelbuildings`` on a
            given layer against the same step without one (the extractor runs), at 2 x 230 x 220 and 2 x 517 x 389: wall milliseconds per
            step between device synchronisations, median of ``--steps`` after a warm-up
  eval      ``evaluate_raster`` windows per second over ``ResidentWindows`` on the raster of tools/bench_resident_eval.py (patchsize 2048,
            overlap 128) with M = 1 and M = 5 members built without ``sentinelbuildings``: a region with a layer against the same region
            without one, alternating, three repeats each after a warm-up
  kernels   the kernel launches of one such step on either side, counted with torch.profiler (a leg of its own, the last: when the
            profiler is not available the counts are recorded as null with the reason and the other legs stand)

    python tools/bench_building_layer.py [--out profiles/building_layer_bench.json]

EXPECTATIONS, written down before the first run; each is recorded as held or not held, none is a pass / fail bar:
  * launches: with the layer a launch takes no more than the ratio of bytes moved per pixel -- 56 / 48 for uint16 S2 (20 read + 28
    written against 24 + 32) and 64 / 56 for fp32 S2 -- plus the spread of the repeats ((median - minimum) / median of both sides)
  * window: the same rule, 7 planes against 6 (56 / 48 bytes per pixel)
  * steps: the step on a given layer is faster; launches and milliseconds of both sides recorded
  * eval: the given layer is faster, and by no more than 1 / (1 - 0.38) = 1.613: the extractor is 38 % of the forward MACs"""
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

LEGS = {"launches": 240, "window": 180, "steps": 240, "kernels": 180, "eval": 540}      # seconds of time limit per leg
ORDER = ("launches", "window", "steps", "eval", "kernels")      # kernels last: nothing is started behind a profiler that fails
BOUND = {"u16": 56.0 / 48.0, "f32": 64.0 / 56.0}
H, W, PS, OV = 2304, 2560, 2048, 128
EXTRACTOR_SHARE = 0.38


def _layer(h, w, seed):
    from popcorn_amd.data.dataset import building_layer
    return building_layer(h, w, torch.Generator().manual_seed(seed)).cuda()


def _pair(with_fn, without_fn, a, bound):
    w_med, w_min, _ = timed(with_fn, a.reps, a.inner)
    p_med, p_min, _ = timed(without_fn, a.reps, a.inner)
    spread = (w_med - w_min) / w_med + (p_med - p_min) / p_med
    ratio = w_med / p_med
    return {"with_layer_us": [round(w_med, 2), round(w_min, 2)], "without_us": [round(p_med, 2), round(p_min, 2)], "ratio": round(ratio, 4),
            "bytes_ratio": round(bound, 4), "spread_of_repeats": round(spread, 4), "expectation_held": bool(ratio <= bound + spread)}


def leg_launches(a):
    from popcorn_amd import ops
    from bench_region import blocky
    h, w = 1536, 2048
    g = torch.Generator(device="cuda").manual_seed(1)
    s2f = torch.randint(0, 10000, (1, 4, h, w), generator=g, device="cuda").float()
    s2u = s2f.cpu().to(torch.uint16).cuda()
    s1 = torch.randn(1, 2, h, w, generator=g, device="cuda") * 5 - 12
    boundary = blocky(h, w, 12, 16, "cuda")
    layer = _layer(h, w, 3)
    band = (0, 1, 2, 3, 0, 1)
    rec, held = {}, True
    for B, hc, wc in ((2, 517, 389), (64, 100, 100)):
        crops = [(3 + 7 * b, 3 + 7 * b + hc, 5 + 13 * b, 5 + 13 * b + wc, 0) for b in range(B)]
        for kind, s2 in (("u16", s2u), ("f32", s2f)):
            with_l = ops.region_gather(s2, s1, boundary, band, crops, buildings=layer)
            plain = ops.region_gather(s2, s1, boundary, band, crops)
            same = all(bool((with_l[k].view(torch.int32) == plain[k].view(torch.int32)).all()) for k in ("S2", "S1", "admin_mask"))
            r = {"gather": _pair(lambda: ops.region_gather(s2, s1, boundary, band, crops, out=with_l, buildings=layer),
                                 lambda: ops.region_gather(s2, s1, boundary, band, crops, out=plain), a, BOUND[kind]),
                 "other_outputs_bit_equal": same}
            for rot in (0, 1):
                params = {"vflip": True, "hflip": False, "rot": rot, "beta": None, "gamma": None}
                ob = ops.region_batch(s2, s1, boundary, band, crops, params, buildings=layer)
                op = ops.region_batch(s2, s1, boundary, band, crops, params)
                r[f"batch_rot{rot}"] = _pair(lambda: ops.region_batch(s2, s1, boundary, band, crops, params, out=ob, buildings=layer),
                                             lambda: ops.region_batch(s2, s1, boundary, band, crops, params, out=op), a, BOUND[kind])
            held = held and all(v["expectation_held"] for v in r.values() if isinstance(v, dict)) and same
            rec[f"{B}x{hc}x{wc}_{kind}"] = r
            print("launches", B, hc, wc, kind, json.dumps(r), flush=True)
    rec["expectation_held"] = held
    return rec


def leg_window(a):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.dataset import SyntheticTestRaster
    data = SyntheticTestRaster(H, W, seasons=1, n_regions=400, seed=1610, device="cuda", raw=True, buildings=True)
    band = (0, 1, 2, 3, 0, 1)
    x, y = 129, 255                                                       # odd origin: source rows are not 16-byte aligned
    out = torch.empty(1, 6, PS, PS, device="cuda")
    bc = torch.empty(1, 1, PS, PS, device="cuda")
    rec = _pair(lambda: ops.region_window(data.s2, data.s1, band, (x, y, 0), PS, stats.MEAN6, stats.STD6, out=out, buildings=data.buildings,
                                          buildings_out=bc),
                lambda: ops.region_window(data.s2, data.s1, band, (x, y, 0), PS, stats.MEAN6, stats.STD6, out=out), a, 7.0 / 6.0)
    rec["layer_bit_equal"] = bool((bc[0, 0].view(torch.int32) == data.buildings[x:x + PS, y:y + PS].view(torch.int32)).all())
    rec["window"] = [x, y, 0, PS]
    print("window", json.dumps(rec), flush=True)
    return rec


def _step_sides(B, hh, ww):
    """(trainer, sample with a layer, the same sample without one) for a model built without sentinelbuildings"""
    from popcorn_amd.data import stats
    from popcorn_amd.data.synthetic import make_raw_batch
    from popcorn_amd.model.popcorn import POPCORN
    from popcorn_amd.train import FusedTrainStep
    from popcorn_amd import ops
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=False).cuda()
    tr = FusedTrainStep(m, lr=1e-4, weight_decay=1e-5, gradient_clip=0.01, scale_regularization=0.01)
    b = make_raw_batch(B, hh, ww, seed=3, region="disc")
    x = ops.select_normalize(b["raw"].cuda(), stats.BAND6, stats.MEAN6, stats.STD6)
    plain = {"input": x, "admin_mask": b["admin_mask"].cuda(), "census_idx": b["census_idx"].cuda(), "y": b["y"].cuda()}
    layer = torch.stack([_layer(hh, ww, 10 + k) for k in range(B)]).unsqueeze(1).contiguous()
    return tr, dict(plain, building_counts=layer), plain


def leg_steps(a):
    rec, held = {}, True
    for B, hh, ww in ((2, 230, 220), (2, 517, 389)):
        tr, given, plain = _step_sides(B, hh, ww)
        ms = {"given_layer": [], "extractor": []}
        for k in range(a.steps + 3):
            for name, s in (("given_layer", given), ("extractor", plain)):
                torch.manual_seed(5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(s)
                torch.cuda.synchronize()
                if k >= 3:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        assert tr.native_steps == 0, "both sides run the per-launch engine (POPCORN_NATIVE_STEP=0)"
        med = {k: float(np.median(v)) for k, v in ms.items()}
        r = {"ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min": {k: round(min(v), 3) for k, v in ms.items()},
             "given_over_extractor": round(med["given_layer"] / med["extractor"], 4), "expectation_held": med["given_layer"] < med["extractor"]}
        held = held and r["expectation_held"]
        rec[f"{B}x{hh}x{ww}"] = r
        print("steps", B, hh, ww, json.dumps(r), flush=True)
    rec["expectation_held"] = held
    return rec


def leg_kernels(a):
    rec = {}
    try:
        from torch.profiler import ProfilerActivity, profile
    except Exception as e:                                                # noqa: BLE001
        return {"launches": None, "reason": f"torch.profiler is not available: {e}"}
    for B, hh, ww in ((2, 230, 220), (2, 517, 389)):
        tr, given, plain = _step_sides(B, hh, ww)
        r = {}
        for name, s in (("given_layer", given), ("extractor", plain)):
            for _ in range(2):
                torch.manual_seed(5)
                tr.step(s)
            torch.cuda.synchronize()
            try:
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    torch.manual_seed(5)
                    tr.step(s)
                    torch.cuda.synchronize()
                n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                        and "memset" not in e.name.lower())
                r[name] = n if n > 0 else None
            except Exception as e:                                        # noqa: BLE001
                r[name] = None
                r["reason"] = f"the profiler did not record the step: {e}"
        rec[f"{B}x{hh}x{ww}"] = r
        print("kernels", B, hh, ww, json.dumps(r), flush=True)
    return rec


def leg_eval(a):
    from popcorn_amd import eval as E
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import MODEL_ORDER_BANDS, ResidentRegion, ResidentWindows
    from popcorn_amd.model.popcorn import POPCORN
    data = SyntheticTestRaster(H, W, seasons=1, n_regions=400, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.03,
                               buildings=True)
    with_l = ResidentWindows(ResidentRegion.from_synthetic(data, with_asc=True), PS, OV)
    without = ResidentWindows(ResidentRegion(data.s2, data.s1, data.boundary, data.census_idx, data.census_pop, band_sel=MODEL_ORDER_BANDS,
                                             s1_asc=data.s1_asc), PS, OV)
    nwin = int(with_l.idx.shape[0])
    models = []
    for k in range(5):
        torch.manual_seed(40 + k)
        models.append(POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=False).cuda().eval())
    legs = {"given_layer": with_l, "extractor": without}
    rec, held = {"raster": [H, W], "patchsize": PS, "overlap": OV, "windows": nwin, "bound": round(1.0 / (1.0 - EXTRACTOR_SHARE), 4)}, True
    for M in (1, 5):
        ms = models[:M]

        def run(feed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            E.evaluate_raster(ms, feed, PS, OV, False)
            torch.cuda.synchronize()
            return nwin / (time.perf_counter() - t0)
        for feed in legs.values():
            run(feed)                                                     # warm-up per leg and shape
        wps = {k: [] for k in legs}
        for _ in range(3):
            for k, feed in legs.items():
                wps[k].append(round(run(feed), 3))
        med = {k: float(np.median(v)) for k, v in wps.items()}
        speedup = med["given_layer"] / med["extractor"]
        r = {"windows_per_s": wps, "median_windows_per_s": med, "given_over_extractor": round(speedup, 4), "faster": speedup > 1.0,
             "within_bound": speedup <= 1.0 / (1.0 - EXTRACTOR_SHARE)}
        r["expectation_held"] = r["faster"] and r["within_bound"]
        held = held and r["expectation_held"]
        rec[f"M{M}"] = r
        print(f"eval M={M}", json.dumps(r), flush=True)
    rec["expectation_held"] = held
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg in this process (what the parent starts per leg)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "building_layer_bench.json"))
    a = ap.parse_args()
    if a.leg is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench_building_layer.py measures on a HIP device; none found")
        rec = {"launches": leg_launches, "window": leg_window, "steps": leg_steps, "kernels": leg_kernels, "eval": leg_eval}[a.leg](a)
        with open(a.out, "w") as fh:
            json.dump(rec, fh)
        return
    res = {"timer": "device events around `inner` back-to-back calls enqueued behind a spin kernel, median and minimum of `reps` windows per "
                    "call (launches, window); wall time between device synchronisations (steps, eval)",
           "reps": a.reps, "inner": a.inner, "steps": a.steps}
    env = dict(os.environ, POPCORN_NATIVE_STEP="0")                       # steps / kernels: the per-launch engine on both sides
    with tempfile.TemporaryDirectory() as tmp:
        for leg in ORDER:
            part = os.path.join(tmp, leg + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(LEGS[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps",
                                 str(a.reps), "--inner", str(a.inner), "--steps", str(a.steps), "--out", part],
                                env=env if leg in ("steps", "kernels") else None).returncode
            if rc != 0 and leg == "kernels":
                res[leg] = {"launches": None, "reason": f"the leg ended with status {rc}"}
                continue
            if rc != 0:
                raise SystemExit(f"bench_building_layer.py: leg {leg} ended with status {rc}; nothing further was started")
            res[leg] = json.load(open(part))
    res["expectations"] = {leg: ("held" if res[leg].get("expectation_held") else "not held") for leg in ("launches", "window", "steps", "eval")}
    res["device_name"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
