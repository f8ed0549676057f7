#!/usr/bin/env python3
"""Device time of the census-table accumulation (pc_census_accumulate, csrc/census_table.hip) next to the stitcher's
pc_stitch_accumulate (csrc/census.hip, with the scale planes, as evaluate_raster calls it) on the same window: one 2048 x 2048 window,
overlap 128, M = 5 members, L = 2 census levels (a fine level of 4,096 units as 32 x 32-pixel blocks, a coarse level of 64 units as
256 x 256-pixel blocks).  Per pixel the census launch reads 4 M + 2 + 4 L = 30 bytes (40 with the second member pass of M = 5), the
stitcher moves about 8 M + 36 = 76; the allowance for the census launch is 2 x the stitcher's time.

Both are timed in this one process with HIP events, alternating; a sample is one event pair around ``--batch`` back-to-back launches
(the device never waits for the host inside a sample) divided by the batch, and the figure is the median of ``--reps`` samples after
warm-up.  ``--levels salt`` times the worst case for the on-chip stages instead: a new id every pixel on both levels.

    python tools/bench_census.py [--reps 30] [--batch 8] [--levels blocks|salt] [--out FILE.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_product import sample  # noqa: E402


def main():
    from popcorn_amd import _lib as L
    from popcorn_amd.eval import CensusTable, Stitcher
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ps", type=int, default=2048)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--levels", choices=("blocks", "salt"), default="blocks")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    ps, ov, M = a.ps, a.overlap, a.members
    yy, xx = torch.meshgrid(torch.arange(ps), torch.arange(ps), indexing="ij")
    if a.levels == "blocks":
        fine, coarse = (yy // 32) * (ps // 32) + xx // 32, (yy // 256) * (ps // 256) + xx // 256
    else:
        fine, coarse = (yy * ps + xx) % 4093, (yy * ps + xx) % 61
    num_ids = [int(fine.max()) + 1, int(coarse.max()) + 1]
    g = torch.Generator(device="cuda").manual_seed(M)
    pd = torch.rand(M, ps, ps, generator=g, device="cuda")
    sc = torch.rand(M, ps, ps, generator=g, device="cuda")
    ct = CensusTable(ps, ps, [fine, coarse], num_ids, M, "cuda")
    ct.set_windows([(0, 0)], ps, ov)
    ts = {"stitch": [], "census": []}
    for r in range(a.reps + 3):
        # fresh accumulators per sample: the int16 count of the stitcher must not run over, the table stays far below 2^63
        st = Stitcher(ps, ps, "cuda")
        ct.table.zero_()
        for name, fn in (("stitch", lambda: st.add_window(0, 0, pd, sc, ov)), ("census", lambda: ct.add_window(0, 0, pd, ov))):
            with L.stream_scope():
                t = sample(fn, a.batch)
            if r >= 3:
                ts[name].append(t)
    ct.finalize()
    s_us, c_us = float(np.median(ts["stitch"])), float(np.median(ts["census"]))
    px = (ps - 2 * ov) ** 2
    res = {"device": torch.cuda.get_device_name(0), "window": ps, "overlap": ov, "members": M, "levels": a.levels, "num_ids": num_ids,
           "reps": a.reps, "batch": a.batch, "stitch_accumulate_us": round(s_us, 2), "census_accumulate_us": round(c_us, 2),
           "census_over_stitch": round(c_us / s_us, 3), "allowance": 2.0, "stitch_min_us": round(min(ts["stitch"]), 2),
           "census_min_us": round(min(ts["census"]), 2), "census_read_GBps": round(px * (4 * M + 2 + 8) / c_us * 1e-3, 1),
           "stitch_moved_GBps": round(px * (8 * M + 36) / s_us * 1e-3, 1)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
