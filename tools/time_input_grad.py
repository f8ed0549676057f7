#!/usr/bin/env python3
"""Device time of the input-gradient launch (ops.input_grad, csrc/input_grad.hip) under an event timer, and the achieved rate of its
ALGORITHMIC bytes -- G read once plus dX written once:

  * a training batch: B = 64 tiles of 100 x 100 with the forced 14-pixel reflect padding (128 x 128 padded), both streams
    (2 x 64 x 8 x 128 x 128 gradient elements in, 64 x 6 x 100 x 100 out: ~82 MB in fp32);
  * an inference window: 1 x 2048 x 2048 without padding, both streams.

    python tools/time_input_grad.py [--reps 50] [--precision fp32|bf16] [--out profiles/input_grad.json]

For context: the strip-pattern conv kernels of this project measure ~3.7 TB/s on this device."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

STREAMS = ((2, (4, 5)), (4, (2, 1, 0, 3)))          # (Cin, chmap) of the SAR and optical streams of the 6-channel model
CASES = {"train_64x100x100_pad14": (64, 100, 100, (14, 14, 14, 14)), "window_1x2048x2048_nopad": (1, 2048, 2048, (0, 0, 0, 0))}


def time_case(B, H, W, pads, reps):
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    pt, pb, pl, pr = pads
    g = torch.Generator().manual_seed(900)
    probs = []
    for cin, chmap in STREAMS:
        G = L.empty_act(B, 8, H + pt + pb, W + pl + pr, "cuda")
        G.copy_(torch.randn(G.shape, generator=g).cuda())
        probs.append({"g": G, "w": (torch.randn(8, cin, 3, 3, generator=g) * 0.3).cuda(), "chmap": chmap})
    out = torch.empty(B, 6, H, W, device="cuda")
    ts = []
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.input_grad(probs, out, pads)
        b.record()
        b.synchronize()
        if r >= 3:
            ts.append(a.elapsed_time(b) * 1e3)
    nbytes = sum(p["g"].numel() * p["g"].element_size() for p in probs) + out.numel() * 4
    med = float(np.median(ts))
    return {"shape": [B, 6, H, W], "pads": list(pads), "algorithmic_MB": round(nbytes / 1e6, 1), "device_us_median": round(med, 1),
            "device_us_min": round(float(np.min(ts)), 1), "GBps_median": round(nbytes / med / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from popcorn_amd import _lib as L
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "precision": a.precision, "cases": {}}
    with L.precision(a.precision):
        for name, (B, H, W, pads) in CASES.items():
            res["cases"][name] = time_case(B, H, W, pads, a.reps)
            print(name, json.dumps(res["cases"][name]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
