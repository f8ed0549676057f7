"""Step-level cost of training a single-modality model (S1-only: input_channels 2, S2-only: 4) through the native executor (DESIGN.md
section 15.9): three steps timed in ONE process, eagerly, window by window in turn:

  (a) the per-launch engine on the one-stream model   FusedTrainStep()                    -> the baseline, unchanged by the feature
  (b) the native executor on the one-stream model     FusedTrainStep(native_single=True)  -> pc_train_step on a one-stream plan
  (c) the native executor on the dual-stream model    FusedTrainStep(), input_channels 6  -> pc_train_step as it was: twice the U-Net work

    python tools/bench_native_single.py [--out profiles/native_single_bench.json] [--quick]

Rows 2 x 230 x 220, 2 x 517 x 389, 2 x 1030 x 770 and 64 x 100 x 100, for ic 2 and 4.  Device events around 20 back-to-back steps, median
of 30 windows with minimum and maximum recorded; lr = 0: thousands of steps leave the parameters where they are.  Also per row: the host's
enqueue time of a step (7 steps into an idle queue, best of 5), the executor's own host time (pc_debug_step_host_ns: sizing pass +
launching pass) and io.launches of (b) and (c), and whether (b) and (a) leave the same bits.

EXPECTATIONS, written before the first run; each is recorded as held or not held per row, none is a pass / fail bar and no ratio is fixed.
The spread of a comparison is (median - minimum) of both sides added, in milliseconds.
  1. (b) is not slower than (a) at any row beyond the spread: the same kernels, fewer host calls.
  2. (b) < (a) by more than the spread at every row below 1 Mpx (B * H * W): there the host's enqueue bounds the step.
  3. (b) <= (c) beyond the spread at no row: one stream's U-Net launches carry half the work of two."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                                         # noqa: E402
from bench_native_layer import executor_probe, host_ms, same_bits, spread, summary, timed      # noqa: E402
from popcorn_amd.model import POPCORN                                # noqa: E402
from popcorn_amd.train import FusedTrainStep                         # noqa: E402

GEOMS = [(2, 230, 220), (2, 517, 389), (2, 1030, 770), (64, 100, 100)]


def make_batch(B, H, W, ic):
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.synthetic import make_raw_batch
    b = make_raw_batch(B, H, W, seed=3, region="disc")
    x = ops.select_normalize(b["raw"].cuda(), stats.BAND6, stats.MEAN6, stats.STD6)
    small = {"admin_mask": b["admin_mask"].cuda(), "census_idx": b["census_idx"].cuda(), "y": b["y"].cuda()}
    # the one-stream model's own input: its first ic channels, as fixtures g8 / g13 cut it
    return dict(small, input=x[:, :ic].contiguous()), dict(small, input=x)


def trainer(ic, **kw):
    torch.manual_seed(1600)
    m = POPCORN(ic, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    return FusedTrainStep(m, lr=0.0, weight_decay=1e-5, gradient_clip=0.01, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/native_single_bench.json")
    ap.add_argument("--quick", action="store_true", help="one geometry, 3 windows of 5 steps (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_native_single needs a HIP device"
    steps, windows = (5, 3) if args.quick else (20, 30)
    geoms = GEOMS[:1] if args.quick else GEOMS
    tr_c = trainer(6)
    rows, held = [], {1: True, 2: True, 3: True}
    for ic in (2, 4):
        tr_a, tr_b = trainer(ic), trainer(ic, native_single=True)
        for (B, H, W) in geoms:
            one, dual = make_batch(B, H, W, ic)
            fns = {"a": lambda: tr_a.step(dict(one)), "b": lambda: tr_b.step(dict(one)), "c": lambda: tr_c.step(dict(dual))}
            n0 = (tr_a.native_steps, tr_b.native_steps, tr_c.native_steps)
            s = summary(timed(fns, steps, windows))
            host = {k: round(host_ms(f), 4) for k, f in fns.items()}
            # the steps went where the row says they went
            assert tr_a.native_steps == n0[0] and tr_b.native_steps > n0[1] and tr_c.native_steps > n0[2]
            lb, sb, eb = executor_probe(tr_b, one)
            lc, sc, ec = executor_probe(tr_c, dual)
            px = B * H * W
            sp_ab, sp_bc = spread(s, "a", "b"), spread(s, "b", "c")
            e1 = s["b"]["median"] <= s["a"]["median"] + sp_ab
            e3 = s["b"]["median"] <= s["c"]["median"] + sp_bc
            held[1], held[3] = held[1] and e1, held[3] and e3
            row = {"ic": ic, "B": B, "H": H, "W": W, "pixels": px,
                   "a_per_launch_single_ms": s["a"], "b_native_single_ms": s["b"], "c_native_dual_ms": s["c"],
                   "b_over_a": round(s["b"]["median"] / s["a"]["median"], 4), "b_over_c": round(s["b"]["median"] / s["c"]["median"], 4),
                   "spread_ab_ms": round(sp_ab, 4), "spread_bc_ms": round(sp_bc, 4), "host_enqueue_ms": host,
                   "executor_host_us": {"b": [round(sb, 1), round(eb, 1)], "c": [round(sc, 1), round(ec, 1)]},
                   "launches": {"b": lb, "c": lc}, "b_equals_a_bitwise": same_bits(tr_b, tr_a, one),
                   "expectation_1": "held" if e1 else "not held", "expectation_3": "held" if e3 else "not held"}
            if px < 1_000_000:
                e2 = s["a"]["median"] - s["b"]["median"] > sp_ab
                held[2] = held[2] and e2
                row["expectation_2"] = "held" if e2 else "not held"
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_native_single.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": getattr(torch.version, "hip", None), "steps_per_window": steps, "windows": windows, "statistic": "median of windows",
           "quick": bool(args.quick),
           "notes": "device-event time per step, eager, lr = 0, one process, the variants alternating window by window; spread = (median - "
                    "minimum) of both sides added; executor_host_us = [sizing pass, launching pass] of pc_debug_step_host_ns, mean of 7 "
                    "calls; host_enqueue_ms = wall time of step() per call, 7 calls into an idle queue, best of 5",
           "rows": rows,
           "expectations": {"1_b_not_slower_than_a_beyond_the_spread_every_row": "held" if held[1] else "not held",
                            "2_b_lt_a_by_more_than_the_spread_below_1Mpx": "held" if held[2] else "not held",
                            "3_b_not_slower_than_c_beyond_the_spread_every_row": "held" if held[3] else "not held"}}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
