"""Step-level cost of the device-N multi-unit step under graph replay: three ways to run the same multi-unit step, timed in
ONE process on the same inputs, the variants alternating window by window:

  (a) the replayed device-N graph                         FusedTrainStep(device_units=True, use_graph=True)
  (b) the eager per-launch multi-unit step                FusedTrainStep()                      -> the parent's only form where a graph or a
                                                                                                    reducer is wanted
  (c) the native executor's multi-unit step               FusedTrainStep(native_units=True)     -> pc_train_step_units (eager, one process)

    python tools/bench_units_graph.py [--out profiles/units_graph_bench.json] [--quick]

Geometries 2 x 100 x 100 and 64 x 100 x 100 with K = 4, 2 x 230 x 220 with K = 16.  Device events around 20 back-to-back steps, median of 30
windows; lr = 0: thousands of steps leave the parameters where they are.  Also per row: the host's enqueue time of a step (7 steps into an
idle queue, best of 5) and whether (a) and (b) give the same bits on the same selection draw.

EXPECTATION, written before the first run: (a) < (b) in every row -- a replay has no per-launch host cost, and (b)'s ~50 launches through
ctypes are host-bound at these sizes.  No figure is fixed in advance.  (a) against (c) is reported, not required: (c) pays one C call per
step and no capacity tail, (a) pays the graph's launch and runs its tail kernels at B K."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch                                                         # noqa: E402
from popcorn_amd.model import POPCORN                                # noqa: E402
from popcorn_amd.train import FusedTrainStep                         # noqa: E402
from tools.bench_units_step import host_ms, make_batch, window_ms    # noqa: E402

ROWS = [(2, 100, 100, 4), (64, 100, 100, 4), (2, 230, 220, 16)]


def trainer(**kw):
    torch.manual_seed(1600)
    m = POPCORN(6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    return FusedTrainStep(m, lr=0.0, weight_decay=1e-5, gradient_clip=0.01, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/units_graph_bench.json")
    ap.add_argument("--quick", action="store_true", help="one row, 3 windows of 5 steps (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_units_graph needs a HIP device"
    steps, windows = (5, 3) if args.quick else (20, 30)
    tr_a, tr_b, tr_c = trainer(device_units=True, use_graph=True), trainer(), trainer(native_units=True)
    rows = []
    for (B, H, W, K) in (ROWS[:1] if args.quick else ROWS):
        smp = make_batch(B, H, W, K)
        fa = lambda i: tr_a.step(dict(smp))                         # noqa: E731
        fb = lambda i: tr_b.step(dict(smp))                         # noqa: E731
        fc = lambda i: tr_c.step(dict(smp))                         # noqa: E731
        n0 = (tr_a.captures, tr_a.device_unit_steps, tr_b.native_unit_steps + tr_b.native_steps + tr_b.device_unit_steps, tr_c.native_unit_steps)
        for f in (fa, fb, fc):
            for i in range(6):
                f(i)
        torch.cuda.synchronize()
        t = {"a": [], "b": [], "c": []}
        for _ in range(windows):
            t["a"].append(window_ms(fa, steps))
            t["b"].append(window_ms(fb, steps))
            t["c"].append(window_ms(fc, steps))
        med = {k: statistics.median(v) for k, v in t.items()}
        host = {"a": host_ms(fa), "b": host_ms(fb), "c": host_ms(fc)}
        # the steps went where the row says they went: one capture, every (a) step a replay of it; (b) neither native nor device-N
        assert tr_a.captures == n0[0] + 1 and tr_a.device_unit_steps > n0[1]
        assert tr_b.native_unit_steps + tr_b.native_steps + tr_b.device_unit_steps == n0[2] and tr_c.native_unit_steps > n0[3]
        torch.manual_seed(7)
        tr_a.step(dict(smp))
        pa, loss_a = tr_a.last["popcount"].clone(), tr_a.loss_out.clone()
        torch.manual_seed(7)
        tr_b.step(dict(smp))
        same = bool(torch.equal(pa[:B * K], tr_b.last["popcount"]) and torch.equal(loss_a, tr_b.loss_out))
        row = {"B": B, "H": H, "W": W, "K": K, "N": B * K,
               "a_graph_ms": round(med["a"], 4), "b_per_launch_ms": round(med["b"], 4), "c_executor_ms": round(med["c"], 4),
               "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
               "range_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
               "host_enqueue_ms": {k: round(v, 4) for k, v in host.items()}, "a_equals_b_bitwise": same}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_units_graph.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": getattr(torch.version, "hip", None), "steps_per_window": steps, "windows": windows, "statistic": "median of windows",
           "quick": bool(args.quick),
           "notes": "device-event time per step, variants alternating window by window; host_enqueue_ms = wall time of step() per call, 7 "
                    "calls into an idle queue, best of 5; a_equals_b_bitwise: popcount[:N] and loss_out on the same selection draw",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
