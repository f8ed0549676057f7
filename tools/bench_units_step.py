"""Step-level cost of multi-unit census supervision: three ways to supervise the same K units of each crop of a 2-crop batch, timed in ONE
process on the same inputs (the comparison DESIGN.md 14 had left open):

  (a) the multi-unit step through the native executor       FusedTrainStep(native_units=True)   -> pc_train_step_units
  (b) the multi-unit step through the per-launch engine     FusedTrainStep(native_units=False)  -> the baseline, unchanged by the feature
  (c) K one-unit native steps, step k supervising unit k of each crop (pc_train_step): what a trainer without the feature pays

    python tools/bench_units_step.py [--out profiles/units_step_bench.json] [--quick]

Geometries 2 x 230 x 220 and 2 x 517 x 389 (the two small rows of bench.py's config3_regions), K in {4, 16, 64}.  Device events around 20
back-to-back steps, median of 30 windows, the three variants alternating window by window; (c) is timed per one-unit step (windows that
cycle through the K units) and reported times K.  lr = 0: thousands of steps leave the parameters where they are.  Also per row: the
host's enqueue time of a step inside the trainer's run-ahead window (7 steps into an idle queue, best of 5), the executor's own host time
(pc_debug_step_host_ns: sizing pass + launching pass) and io.launches.

EXPECTATION, written before the first run: (a) < (b) at every row, (a) issues no torch launch, and the issue that asked for this tool
expected (a) to issue FOUR launches more than a one-unit native step of the same geometry (layout, the score as its own launch, the
sums' accumulate launch, the paint).  Reading the executor's stage list gives FIVE: the head forward without a region finishes
{Nsel, sum scale} itself -- its single-block reduction, which the one-unit step folds into its loss launch.  The JSON records what ran."""
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

GEOMS = [(2, 230, 220), (2, 517, 389)]
KS = [4, 16, 64]


def make_batch(B, H, W, K, seed=0):
    """A normalised-input batch whose crops are cut into a grid of K + 8 cells or more: K of them listed (shuffled order), the others
    unlisted neighbours, a -1 frame at the bottom / right like the collate's padding."""
    g = torch.Generator().manual_seed(seed + 131 * K + H)
    gy = 1
    while gy * gy < K + 8:
        gy += 1
    gx = gy
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    cell = (yy * gy // H) * gx + xx * gx // W
    admin = torch.empty(B, H, W)
    cidx = torch.empty(B, K, dtype=torch.int64)
    for b in range(B):
        admin[b] = (100 * (b + 1) + cell).float()
        cidx[b] = 100 * (b + 1) + torch.randperm(gx * gy, generator=g)[:K]
    admin[:, H - 3:, :] = -1.0
    admin[:, :, W - 2:] = -1.0
    dev = "cuda"
    return {"input": torch.randn(B, 6, H, W, generator=g).to(dev), "admin_mask": admin.to(dev), "census_idx": cidx.to(dev),
            "y": (torch.rand(B, K, generator=g) * 300.0).to(dev), "census_n": [K] * B}


def trainer(native_units):
    torch.manual_seed(1600)
    m = POPCORN(6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    return FusedTrainStep(m, lr=0.0, weight_decay=1e-5, gradient_clip=0.01, native_units=native_units)


def one_unit(smp, k):
    return {"input": smp["input"], "admin_mask": smp["admin_mask"], "census_idx": smp["census_idx"][:, k].contiguous(),
            "y": smp["y"][:, k].contiguous()}


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def host_ms(fn, n=7, reps=5):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            fn(i)
        d = (time.perf_counter() - t0) / n
        best = d if best is None or d < best else best
    torch.cuda.synchronize()
    return best * 1e3


def executor_probe(tr, smp):
    """(io.launches, sizing-pass us, launching-pass us) of one direct executor call on ``smp`` (multi-unit or one-unit)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/units_step_bench.json")
    ap.add_argument("--quick", action="store_true", help="one geometry, one K, 3 windows of 5 steps (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_units_step needs a HIP device"
    steps, windows = (5, 3) if args.quick else (20, 30)
    geoms, ks = (GEOMS[:1], KS[:1]) if args.quick else (GEOMS, KS)
    tr_a, tr_b, tr_c = trainer(True), trainer(False), trainer(False)
    rows = []
    for (B, H, W) in geoms:
        for K in ks:
            smp = make_batch(B, H, W, K)
            ones = [one_unit(smp, k) for k in range(K)]
            fa = lambda i: tr_a.step(dict(smp))                         # noqa: E731
            fb = lambda i: tr_b.step(dict(smp))                         # noqa: E731
            fc = lambda i: tr_c.step(dict(ones[i % K]))                 # noqa: E731
            n0 = (tr_a.native_unit_steps, tr_b.native_unit_steps + tr_b.native_steps, tr_c.native_steps)
            for f in (fa, fb, fc):                                      # warm-up: every shape of the timed windows
                for i in range(max(6, min(K, 16))):
                    f(i)
            torch.cuda.synchronize()
            t = {"a": [], "b": [], "c": []}
            for _ in range(windows):
                t["a"].append(window_ms(fa, steps))
                t["b"].append(window_ms(fb, steps))
                t["c"].append(window_ms(fc, steps))
            med = {k: statistics.median(v) for k, v in t.items()}
            lo = {k: min(v) for k, v in t.items()}
            hi = {k: max(v) for k, v in t.items()}
            host = {"a": host_ms(fa), "b": host_ms(fb), "c": host_ms(fc)}
            # the steps went where the row says they went
            assert tr_a.native_unit_steps > n0[0] and tr_b.native_unit_steps + tr_b.native_steps == n0[1] and tr_c.native_steps > n0[2]
            la, sa, ea = executor_probe(tr_a, smp)
            lc, sc, ec = executor_probe(tr_c, ones[0])
            # same computation: the two multi-unit paths give the same bits on the same selection draw
            torch.manual_seed(7)
            tr_a.step(dict(smp))
            pa = tr_a.last["popcount"].clone()
            loss_a = tr_a.loss_out.clone()
            torch.manual_seed(7)
            tr_b.step(dict(smp))
            same = bool(torch.equal(pa, tr_b.last["popcount"]) and torch.equal(loss_a, tr_b.loss_out))
            row = {"B": B, "H": H, "W": W, "K": K, "N": B * K,
                   "a_executor_ms": round(med["a"], 4), "b_per_launch_ms": round(med["b"], 4),
                   "c_one_unit_step_ms": round(med["c"], 4), "c_K_one_unit_steps_ms": round(K * med["c"], 4),
                   "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / (K * med["c"]), 4),
                   "range_ms": {k: [round(lo[k], 4), round(hi[k], 4)] for k in t},
                   "host_enqueue_ms": {k: round(v, 4) for k, v in host.items()},
                   "executor_host_us": {"a": [round(sa, 1), round(ea, 1)], "c": [round(sc, 1), round(ec, 1)]},
                   "launches": {"a": la, "c_one_unit": lc}, "a_equals_b_bitwise": same}
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_units_step.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "hip": getattr(torch.version, "hip", None), "steps_per_window": steps, "windows": windows, "statistic": "median of windows",
           "quick": bool(args.quick),
           "notes": "device-event time per step; c_K_one_unit_steps_ms = K x the per-step median of one-unit native steps cycling through "
                    "the K units; executor_host_us = [sizing pass, launching pass] of pc_debug_step_host_ns, mean of 7 calls; "
                    "host_enqueue_ms = wall time of step() per call, 7 calls into an idle queue, best of 5",
           "rows": rows}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
