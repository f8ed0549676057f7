"""Step-level cost of training on a shipped building layer through the native executor: three steps timed in
ONE process, eagerly, window by window in turn:

  (a) the per-launch engine on a given layer         FusedTrainStep()                   -> the baseline, unchanged by the feature
  (b) the native executor on the layer               FusedTrainStep(native_layer=True)  -> pc_train_step_layer
  (c) the native executor with the frozen extractor  FusedTrainStep(), sentinelbuildings model, no layer -> pc_train_step: the fastest
      step before the feature, of ANOTHER model configuration -- shown for orientation

    python tools/bench_native_layer.py [--out profiles/native_layer_bench.json] [--quick]

Rows 2 x 230 x 220, 2 x 517 x 389, 2 x 1030 x 770 and 64 x 100 x 100.  Device events around 20 back-to-back steps, median of 30 windows
with minimum and maximum recorded; lr = 0: thousands of steps leave the parameters where they are.  Also per row: the host's enqueue
time of a step (7 steps into an idle queue, best of 5), the executor's own host time (pc_debug_step_host_ns: sizing pass + launching
pass) and io.launches of (b) and (c); and the multi-unit step at K = 16 on 2 x 230 x 220, native (pc_train_step_units_layer) against
per-launch, both on the layer.

EXPECTATIONS, written before the first run; each is recorded as held or not held, none is a pass / fail bar and no ratio is fixed.  The
spread of a comparison is (median - minimum) of both sides added, in milliseconds.
  1. (b) <= (c) at every row: (b) issues a subset of (c)'s launches.
  2. (b) < (a) by more than the spread at every row below 1 Mpx (B * H * W): there the host's enqueue bounds the step.
  3. at 2 x 1030 x 770, (b) is within the spread of (a) or better: there the kernels bound the step and both sides run the same ones."""
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
from popcorn_amd.train import FusedTrainStep                         # noqa: E402

GEOMS = [(2, 230, 220), (2, 517, 389), (2, 1030, 770), (64, 100, 100)]
UNITS_GEOM, UNITS_K = (2, 230, 220), 16


def layer(B, H, W, seed=10):
    from popcorn_amd.data.dataset import building_layer
    return torch.stack([building_layer(H, W, torch.Generator().manual_seed(seed + k)) for k in range(B)]).unsqueeze(1).contiguous().cuda()


def make_batch(B, H, W):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.synthetic import make_raw_batch
    b = make_raw_batch(B, H, W, seed=3, region="disc")
    x = ops.select_normalize(b["raw"].cuda(), stats.BAND6, stats.MEAN6, stats.STD6)
    plain = {"input": x, "admin_mask": b["admin_mask"].cuda(), "census_idx": b["census_idx"].cuda(), "y": b["y"].cuda()}
    return dict(plain, building_counts=layer(B, H, W)), plain


def trainer(given, **kw):
    torch.manual_seed(1600)
    m = POPCORN(6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=not given).cuda()
    return FusedTrainStep(m, lr=0.0, weight_decay=1e-5, gradient_clip=0.01, **kw)


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


def executor_probe(tr, smp):
    """(io.launches, sizing-pass us, launching-pass us) of one direct executor call on ``smp``"""
    lib = L.lib()
    lib.pc_debug_step_host_ns.argtypes = [C.POINTER(C.c_double)]
    s = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in smp.items()}
    B, _, H, W = s["input"].shape
    sel = tr._draw_selection(H, W)
    ns = (C.c_double * 2)()
    acc = [0.0, 0.0]
    with L.precision("fp32"), L.stream_scope():
        got = tr._native_io(s, sel, False, False)
        io, units = got if isinstance(got, tuple) else (got, None)
        full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
        torch.cuda.synchronize()
        for _ in range(7):
            rc = tr._native_call(tr._native_handle(), io, full, L.stream_ptr(), units)
            assert rc == 0, rc
            lib.pc_debug_step_host_ns(ns)
            acc[0] += ns[0]
            acc[1] += ns[1]
        torch.cuda.synchronize()
    return int(io.launches), acc[0] / 7e3, acc[1] / 7e3


def timed(fns, steps, windows, warm=6):
    """{name: list of per-step ms, one per window}, the variants alternating window by window after a warm-up of each"""
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


def same_bits(tr_x, tr_y, smp):
    out = []
    for tr in (tr_x, tr_y):
        torch.manual_seed(7)
        tr.step(dict(smp))
        out.append((tr.loss_out.clone(), tr.flat_g.clone(), tr.last["popcount"].clone()))
    return all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(*out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/native_layer_bench.json")
    ap.add_argument("--quick", action="store_true", help="one geometry, 3 windows of 5 steps (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_native_layer needs a HIP device"
    steps, windows = (5, 3) if args.quick else (20, 30)
    geoms = GEOMS[:1] if args.quick else GEOMS
    tr_a, tr_b, tr_c = trainer(True), trainer(True, native_layer=True), trainer(False)
    rows, held = [], {1: True, 2: True, 3: True}
    for (B, H, W) in geoms:
        given, plain = make_batch(B, H, W)
        fns = {"a": lambda: tr_a.step(dict(given)), "b": lambda: tr_b.step(dict(given)), "c": lambda: tr_c.step(dict(plain))}
        n0 = (tr_a.native_steps, tr_b.native_steps, tr_c.native_steps)
        t = timed(fns, steps, windows)
        s = summary(t)
        host = {k: round(host_ms(f), 4) for k, f in fns.items()}
        # the steps went where the row says they went
        assert tr_a.native_steps == n0[0] and tr_b.native_steps > n0[1] and tr_c.native_steps > n0[2]
        lb, sb, eb = executor_probe(tr_b, given)
        lc, sc, ec = executor_probe(tr_c, plain)
        px = B * H * W
        e1 = s["b"]["median"] <= s["c"]["median"]
        held[1] = held[1] and e1
        row = {"B": B, "H": H, "W": W, "pixels": px,
               "a_per_launch_layer_ms": s["a"], "b_native_layer_ms": s["b"], "c_native_extractor_ms": s["c"],
               "b_over_a": round(s["b"]["median"] / s["a"]["median"], 4), "b_over_c": round(s["b"]["median"] / s["c"]["median"], 4),
               "spread_ab_ms": round(spread(s, "a", "b"), 4), "host_enqueue_ms": host,
               "executor_host_us": {"b": [round(sb, 1), round(eb, 1)], "c": [round(sc, 1), round(ec, 1)]},
               "launches": {"b": lb, "c": lc}, "b_equals_a_bitwise": same_bits(tr_b, tr_a, given), "expectation_1": "held" if e1 else "not held"}
        if px < 1_000_000:
            e2 = s["a"]["median"] - s["b"]["median"] > spread(s, "a", "b")
            held[2] = held[2] and e2
            row["expectation_2"] = "held" if e2 else "not held"
        if (B, H, W) == (2, 1030, 770):
            e3 = s["b"]["median"] <= s["a"]["median"] + spread(s, "a", "b")
            held[3] = held[3] and e3
            row["expectation_3"] = "held" if e3 else "not held"
        rows.append(row)
        print(json.dumps(row), flush=True)
    units = None
    if not args.quick:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from bench_units_step import make_batch as make_units
        B, H, W = UNITS_GEOM
        smp = dict(make_units(B, H, W, UNITS_K), building_counts=layer(B, H, W))
        tr_un, tr_up = trainer(True, native_layer=True, native_units=True), trainer(True)
        fns = {"native": lambda: tr_un.step(dict(smp)), "per_launch": lambda: tr_up.step(dict(smp))}
        t = timed(fns, steps, windows)
        s = summary(t)
        assert tr_un.native_unit_steps > 0 and tr_up.native_unit_steps == 0 and tr_up.native_steps == 0
        lu, su, eu = executor_probe(tr_un, smp)
        units = {"B": B, "H": H, "W": W, "K": UNITS_K, "native_layer_ms": s["native"], "per_launch_layer_ms": s["per_launch"],
                 "native_over_per_launch": round(s["native"]["median"] / s["per_launch"]["median"], 4),
                 "spread_ms": round(spread(s, "native", "per_launch"), 4), "host_enqueue_ms": {k: round(host_ms(f), 4) for k, f in fns.items()},
                 "executor_host_us": [round(su, 1), round(eu, 1)], "launches": lu, "bitwise_equal": same_bits(tr_un, tr_up, smp)}
        print(json.dumps(units), flush=True)
    out = {"tool": "tools/bench_native_layer.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": getattr(torch.version, "hip", None), "steps_per_window": steps, "windows": windows, "statistic": "median of windows",
           "quick": bool(args.quick),
           "notes": "device-event time per step, eager, lr = 0, one process, the variants alternating window by window; spread = (median - "
                    "minimum) of both sides added; executor_host_us = [sizing pass, launching pass] of pc_debug_step_host_ns, mean of 7 "
                    "calls; host_enqueue_ms = wall time of step() per call, 7 calls into an idle queue, best of 5",
           "rows": rows, "multi_unit_K16": units,
           "expectations": {"1_b_le_c_every_row": "held" if held[1] else "not held",
                            "2_b_lt_a_by_more_than_the_spread_below_1Mpx": "held" if held[2] else "not held",
                            "3_b_within_spread_of_a_or_better_at_2x1030x770": ("held" if held[3] else "not held") if not args.quick else None}}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
