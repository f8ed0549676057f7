#!/usr/bin/env python3
"""Device time of the product-grid accumulation (pc_product_accumulate, csrc/product.hip) next to its sibling on the same window, the
stitcher's pc_stitch_accumulate (csrc/census.hip, with the scale planes, as evaluate_raster calls it): one 2048 x 2048 window, overlap
128, M = 1 and M = 5 members, cell = 10.  Per pixel the product launch reads 4 M + 2 bytes, the sibling moves at least 8 M + 36, so the
product launch must not be the slower one.

Both are timed in this one process with HIP events, alternating; a sample is one event pair around ``--batch`` back-to-back launches
(the device never waits for the host inside a sample) divided by the batch, and the figure is the median of ``--reps`` samples after
warm-up.  ``share`` is the product launch over the time of one ``config5`` window (``--windows_per_s``: the bench line of DESIGN.md 5,
one member).

    python tools/bench_product.py [--reps 30] [--batch 8] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def sample(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / batch


def main():
    from popcorn_amd import _lib as L
    from popcorn_amd.eval import ProductGrid, Stitcher
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ps", type=int, default=2048)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--cell", type=int, default=10)
    ap.add_argument("--windows_per_s", type=float, default=345.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    ps, ov = a.ps, a.overlap
    res = {"device": torch.cuda.get_device_name(0), "window": ps, "overlap": ov, "cell": a.cell, "reps": a.reps, "batch": a.batch, "members": {}}
    for M in (1, 5):
        g = torch.Generator(device="cuda").manual_seed(M)
        pd = torch.rand(M, ps, ps, generator=g, device="cuda")
        sc = torch.rand(M, ps, ps, generator=g, device="cuda")
        pg = ProductGrid(ps, ps, a.cell, M, "cuda")
        pg.set_windows([(0, 0)], ps, ov)
        ts = {"stitch": [], "product": []}
        for r in range(a.reps + 3):
            # fresh accumulators per sample: the int16 count of the stitcher must not run over
            st = Stitcher(ps, ps, "cuda")
            pg.cells.zero_()
            for name, fn in (("stitch", lambda: st.add_window(0, 0, pd, sc, ov)), ("product", lambda: pg.add_window(0, 0, pd, ov))):
                with L.stream_scope():
                    t = sample(fn, a.batch)
                if r >= 3:
                    ts[name].append(t)
        s_us, p_us = float(np.median(ts["stitch"])), float(np.median(ts["product"]))
        px = (ps - 2 * ov) ** 2
        res["members"][str(M)] = {
            "stitch_accumulate_us": round(s_us, 2), "product_accumulate_us": round(p_us, 2), "product_over_stitch": round(p_us / s_us, 3),
            "stitch_min_us": round(min(ts["stitch"]), 2), "product_min_us": round(min(ts["product"]), 2),
            "product_read_GBps": round(px * (4 * M + 2) / p_us * 1e-3, 1), "stitch_moved_GBps": round(px * (8 * M + 36) / s_us * 1e-3, 1),
            "share_of_config5_window": round(p_us * 1e-6 * a.windows_per_s, 5)}
        print(f"M={M}", json.dumps(res["members"][str(M)]), flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
