"""Cost of the no-grad forward through the native forward executor (pc_forward, popcorn_amd/infer.py) against the
per-launch engine of the same commit, in ONE process, the legs alternating window by window (the method of tools/bench_native_layer.py):

  per call    model(sample, padding=False) under no_grad at 1 x 230 x 220, 1 x 517 x 389, 1 x 1030 x 770 and 1 x 2048 x 2048, each with
              the frozen extractor and on a shipped building layer, flag off (per-launch) and on (native): device events around
              back-to-back calls, median / minimum / maximum of the windows; io.launches, the executor's own host time
              (pc_debug_step_host_ns: sizing pass, launching pass), arena_needed, the host's enqueue time per call
  validation  one whole weak-validation pass over the held-out units of tools/bench_resident_val.py's setup (2304 x 2560, 400 units, 80
              held out, ResidentItems), flag off and on, alternating, wall time between device synchronisations
  evaluation  resident evaluation (ResidentWindows) of the same raster at patch 2048 / overlap 128 and patch 256 / overlap 32, one
              member, flag off and on, in windows per second

    python tools/bench_native_forward.py [--out profiles/native_forward_bench.json] [--quick]

EXPECTATIONS, written before the first run; each is recorded as held or not held, none is a pass / fail bar and no absolute figure is
fixed.  The spread of a comparison is (median - minimum) of both sides added (per call), or the largest (max - min) of the repeats of
either side (passes).
  1. per call: native is not slower than per-launch beyond the spread at any row.
  2. per call: native is faster by more than the spread at the two rows below 1 Mpx (the per-launch path is host-bound there).
  3. per call: native is within the spread at 1 x 2048 x 2048 (the kernels bound the call and both sides run the same ones).
  4. validation: the pass is faster by more than the spread with the flag on.
  5. evaluation at patch 2048: within the spread.
  6. evaluation at patch 256: not slower (beyond the spread).
The comparison is always against the per-launch path of the same commit in the same process."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch                                                         # noqa: E402
from popcorn_amd import _lib as L                                    # noqa: E402
from popcorn_amd.model import POPCORN                                # noqa: E402

GEOMS = [(1, 230, 220), (1, 517, 389), (1, 1030, 770), (1, 2048, 2048)]
RH, RW, UNITS = 2304, 2560, 400


def layer(B, H, W, seed=10):
    from popcorn_amd.data.dataset import building_layer
    return torch.stack([building_layer(H, W, torch.Generator().manual_seed(seed + k)) for k in range(B)]).unsqueeze(1).contiguous().cuda()


def make_batch(B, H, W):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.synthetic import make_raw_batch
    b = make_raw_batch(B, H, W, seed=3, region="disc")
    x = ops.select_normalize(b["raw"].cuda(), stats.BAND6, stats.MEAN6, stats.STD6)
    return {"input": x, "admin_mask": b["admin_mask"].cuda(), "census_idx": b["census_idx"].cuda()}


def model(given, seed=1600):
    torch.manual_seed(seed)
    return POPCORN(6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=not given).cuda().eval()


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def host_ms(fn, n=7, reps=5):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        d = (time.perf_counter() - t0) / n
        best = d if best is None or d < best else best
    torch.cuda.synchronize()
    return best * 1e3


def timed(fns, steps, windows, warm=4):
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(window_ms(f, steps))
    return t


def summary(t):
    return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in t.items()}


def spread(s, x, y):
    return (s[x]["median"] - s[x]["min"]) + (s[y]["median"] - s[y]["min"])


def forward(m, smp, native):
    def f():
        m.native_forward = native
        with torch.no_grad():
            return m(dict(smp), padding=False)
    return f


def executor_probe(m, smp):
    """(io.launches, arena_needed, sizing-pass us, launching-pass us) of the model's executor on ``smp``, mean of 7 calls"""
    lib = L.lib()
    lib.pc_debug_step_host_ns.argtypes = [C.POINTER(C.c_double)]
    ns, acc = (C.c_double * 2)(), [0.0, 0.0]
    f = forward(m, smp, True)
    f()
    torch.cuda.synchronize()
    for _ in range(7):
        o = f()
        lib.pc_debug_step_host_ns(ns)
        acc[0] += ns[0]
        acc[1] += ns[1]
    torch.cuda.synchronize()
    return int(o.launches), int(o.arena_needed), round(acc[0] / 7e3, 1), round(acc[1] / 7e3, 1)


def same_bits(m, smp):
    a, b = forward(m, smp, False)(), forward(m, smp, True)()
    return all(bool(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))) for k in ("popcount", "popdensemap", "scale"))


def per_call(args):
    m_ext, m_lay = model(False), model(True)
    rows, held = [], {1: True, 2: True, 3: True}
    for (B, H, W) in (GEOMS[:1] if args.quick else GEOMS):
        px = B * H * W
        steps, windows = (5, 3) if args.quick else ((20, 30) if px < 1_000_000 else (5, 20))
        plain = make_batch(B, H, W)
        given = dict(plain, building_counts=layer(B, H, W))
        row = {"B": B, "H": H, "W": W, "pixels": px, "steps_per_window": steps, "windows": windows}
        for tag, m, smp in (("extractor", m_ext, plain), ("layer", m_lay, given)):
            fns = {"per_launch": forward(m, smp, False), "native": forward(m, smp, True)}
            n0 = m.native_forwards
            s = summary(timed(fns, steps, windows))
            assert m.native_forwards > n0
            sp = spread(s, "per_launch", "native")
            launches, arena, size_us, launch_us = executor_probe(m, smp)
            r = {"per_launch_ms": s["per_launch"], "native_ms": s["native"], "spread_ms": round(sp, 4),
                 "native_over_per_launch": round(s["native"]["median"] / s["per_launch"]["median"], 4),
                 "host_enqueue_ms": {k: round(host_ms(f), 4) for k, f in fns.items()}, "launches": launches, "arena_needed": arena,
                 "executor_host_us": [size_us, launch_us], "bitwise_equal": same_bits(m, smp)}
            e1 = s["native"]["median"] <= s["per_launch"]["median"] + sp
            held[1] = held[1] and e1
            r["expectation_1"] = "held" if e1 else "not held"
            if px < 1_000_000:
                e2 = s["per_launch"]["median"] - s["native"]["median"] > sp
                held[2] = held[2] and e2
                r["expectation_2"] = "held" if e2 else "not held"
            if (H, W) == (2048, 2048):
                e3 = abs(s["native"]["median"] - s["per_launch"]["median"]) <= sp
                held[3] = held[3] and e3
                r["expectation_3"] = "held" if e3 else "not held"
            row[tag] = r
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows, held


def passes(legs, repeats):
    """{leg: [ms per pass]}, alternating after a warm-up pass per leg; the warm-up's results are returned for the comparison of bits"""
    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    outs = {k: run(fn)[1] for k, fn in legs.items()}
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            ms[k].append(round(run(fn)[0], 2))
    med = {k: float(statistics.median(v)) for k, v in ms.items()}
    sp = max(max(v) - min(v) for v in ms.values())
    return outs, ms, med, round(sp, 2)


def end_to_end(args):
    from popcorn_amd import eval as E
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.region import ResidentItems, ResidentRegion, ResidentWindows, plan_one_unit, split_census
    data = SyntheticTestRaster(RH, RW, seasons=1, n_regions=UNITS, seed=1610, device="cuda", raw=True, nan_clouds=0.05, s1_gap=0.03)
    region = ResidentRegion.from_synthetic(data, with_asc=True)
    ids, pop = split_census(region.census_idx, region.census_pop, "val")
    items = ResidentItems(region, plan_one_unit(region.table, ids, pop, region.shape), seasons=1)
    m = model(False, seed=40)

    def validate(native):
        def f():
            m.native_forward = native
            pred = []
            with torch.no_grad():
                for s in items:
                    pred.append(m(s, padding=False)["popcount"].clone())
            return torch.cat(pred)
        return f
    outs, ms, med, sp = passes({"per_launch": validate(False), "native": validate(True)}, 3)
    assert m.native_forwards == 4 * len(items.plan)                      # the passes went where the legs say they went
    val = {"raster": [RH, RW], "units": UNITS, "items": len(items.plan), "pass_ms": ms, "median_pass_ms": med, "spread_of_repeats_ms": sp,
           "ms_per_item": {k: round(v / len(items.plan), 3) for k, v in med.items()},
           "native_over_per_launch": round(med["native"] / med["per_launch"], 4),
           "popcounts_bit_equal": bool(torch.equal(outs["per_launch"].view(torch.int32), outs["native"].view(torch.int32))),
           "expectation_4": "held" if med["per_launch"] - med["native"] > sp else "not held"}
    print("validation", json.dumps(val), flush=True)
    ev = {}
    for ps, ov, key in ((2048, 128, 5), (256, 32, 6)):
        feed = ResidentWindows(region, ps, ov, fourseasons=False)

        def evaluate(native):
            def f():
                m.native_forward = native
                return E.evaluate_raster([m], feed, ps, ov, False)[0]
            return f
        outs, ms, med, sp = passes({"per_launch": evaluate(False), "native": evaluate(True)}, 3)
        n = len(feed.idx)
        r = {"patch": ps, "overlap": ov, "windows": n, "pass_ms": ms, "median_pass_ms": med, "spread_of_repeats_ms": sp,
             "windows_per_s": {k: round(n / v * 1e3, 2) for k, v in med.items()},
             "native_over_per_launch": round(med["native"] / med["per_launch"], 4),
             "maps_bit_equal": bool(torch.equal(outs["per_launch"].view(torch.int32), outs["native"].view(torch.int32)))}
        if key == 5:
            r["expectation_5"] = "held" if abs(med["native"] - med["per_launch"]) <= sp else "not held"
        else:
            r["expectation_6"] = "held" if med["native"] <= med["per_launch"] + sp else "not held"
        ev[f"patch_{ps}"] = r
        print("evaluation", json.dumps(r), flush=True)
    return val, ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/native_forward_bench.json")
    ap.add_argument("--quick", action="store_true", help="one geometry, 3 windows of 5 calls, no end-to-end legs (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_native_forward needs a HIP device"
    rows, held = per_call(args)
    val, ev = (None, None) if args.quick else end_to_end(args)
    out = {"tool": "tools/bench_native_forward.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": getattr(torch.version, "hip", None), "statistic": "median of windows", "quick": bool(args.quick),
           "notes": "per call: device-event time per call, eager, one process, per-launch and native alternating window by window; spread = "
                    "(median - minimum) of both sides added; executor_host_us = [sizing pass, launching pass] of pc_debug_step_host_ns, mean "
                    "of 7 calls; host_enqueue_ms = wall time of the call, 7 calls into an idle queue, best of 5.  Passes: wall time between "
                    "device synchronisations, 3 repeats per leg alternating after a warm-up pass each; spread = the largest max - min",
           "rows": rows, "validation": val, "evaluation": ev,
           "expectations": {"1_native_not_slower_beyond_the_spread_every_row": "held" if held[1] else "not held",
                            "2_native_faster_by_more_than_the_spread_below_1Mpx": "held" if held[2] else "not held",
                            "3_within_the_spread_at_2048x2048": None if args.quick else ("held" if held[3] else "not held"),
                            "4_validation_faster_by_more_than_the_spread": None if val is None else val["expectation_4"],
                            "5_evaluation_patch_2048_within_the_spread": None if ev is None else ev["patch_2048"]["expectation_5"],
                            "6_evaluation_patch_256_not_slower": None if ev is None else ev["patch_256"]["expectation_6"]}}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
