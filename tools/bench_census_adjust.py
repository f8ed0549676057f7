#!/usr/bin/env python3
"""Device time of the adjusted census table (csrc/census_adjust.hip, eval.CensusTable(adjust=...)) next to what it replaces: one
2048 x 2048 window, overlap 128, M = 1 and M = 5 members, a fine level of 4,096 units (32 x 32-pixel blocks) adjusted to a coarse level of
64 units (256 x 256-pixel blocks; nested, so 4,096 pairs).

  plan        ops.census_pair_plan: host time around the call, synchronised (five rounds over the two planes, a count pass, one host
              synchronisation for the flag word, the write pass), and the bytes the plan keeps (the pair plane and the pair lists)
  accumulate  pc_census_accumulate for the two levels, and for the two levels plus the pair plane.  4,096 + 64 ids fill the launch's LDS
              table (4,864 ids); the pair plane's 4,096 do not fit beside them and add to the global table directly
  finalize    pc_census_finalize + pc_census_adjust_finalize of the fine level (with the buffers' allocation)
  map path    what gives the same numbers without the table: M x (adjust_map_to_census + pc_census_sum at the fine level) on M
              full-resolution member maps, and the bytes of those M maps

EXPECTED, written before the first run: the pair plane is one more level for stages 1 and 2 of the accumulate (the launch is bound by
that on-chip work, not by its reads: 0.94 TB/s in profiles/r8_bench_census_blocks.json) and, outside the LDS table, one global 64-bit
atomic per (lane, member, tile) instead of an LDS one: 392 tiles x 256 lanes x M = 0.5 M atomics on 4,096 x M addresses at M = 5.  From
102.6 us for two levels at M = 5: +35 % to +60 % (140 - 165 us); at M = 1 the same share.  The finalize and the plan are small: a few
microseconds, and well under a millisecond of device work for the plan.  No number here is a pass bar.

Timing as tools/bench_census.py: HIP events around ``--batch`` back-to-back launches, alternating the variants, the median of ``--reps``
samples after warm-up.

    python tools/bench_census_adjust.py [--reps 30] [--batch 8] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_product import sample  # noqa: E402

EXPECTED = {"accumulate_extra_share_M5": [0.35, 0.60], "accumulate_with_pairs_us_M5": [140, 165],
            "finalize_us": "a few microseconds", "plan_device_ms": "well under 1"}


def bench_members(M, a, fine, coarse, num_ids, pop):
    from popcorn_amd import _lib as L
    from popcorn_amd import eval as E
    ps, ov = a.ps, a.overlap
    g = torch.Generator(device="cuda").manual_seed(M)
    pd = torch.rand(M, ps, ps, generator=g, device="cuda")
    idx = list(range(num_ids[1]))
    idx_d, pop_d = torch.tensor(idx, device="cuda"), torch.tensor(pop, dtype=torch.float32, device="cuda")
    plain = E.CensusTable(ps, ps, [fine, coarse], num_ids, M, "cuda")
    adj = E.CensusTable(ps, ps, [fine, coarse], num_ids, M, "cuda", adjust={"level": 1, "census_idx": idx, "census_pop": pop})
    for ct in (plain, adj):
        ct.set_windows([(0, 0)], ps, ov)

    def finalize():
        adj.totals = None
        adj.finalize()
        adj.adjusted(0)

    def map_path():
        for m in range(M):
            mp = E.adjust_map_to_census(maps[m], coarse_d, idx_d, pop_d)        # (one host synchronisation per call: num_ids)
            E.census_sums(mp, fine_d, num_ids[0])

    fine_d, coarse_d = adj.boundaries
    maps = pd.clone()
    ts = {"levels": [], "levels_pairs": [], "finalize": [], "map_path": []}
    for r in range(a.reps + 3):
        plain.table.zero_()
        adj.table.zero_()
        maps.copy_(pd)                          # (the adjustment works in place)
        for name, fn, batch in (("levels", lambda: plain.add_window(0, 0, pd, ov), a.batch),
                                ("levels_pairs", lambda: adj.add_window(0, 0, pd, ov), a.batch), ("finalize", finalize, a.batch),
                                ("map_path", map_path, 1)):
            with L.stream_scope():
                t = sample(fn, batch)
            if r >= 3:
                ts[name].append(t)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    return {"members": M, "accumulate_levels_us": round(med["levels"], 2), "accumulate_levels_pairs_us": round(med["levels_pairs"], 2),
            "accumulate_extra_us": round(med["levels_pairs"] - med["levels"], 2),
            "accumulate_extra_share": round(med["levels_pairs"] / med["levels"] - 1.0, 3),
            "accumulate_levels_min_us": round(min(ts["levels"]), 2), "accumulate_levels_pairs_min_us": round(min(ts["levels_pairs"]), 2),
            "finalize_us": round(med["finalize"], 2), "map_path_us": round(med["map_path"], 2),
            "map_path_min_us": round(min(ts["map_path"]), 2), "member_maps_bytes": M * ps * ps * 4,
            "table_bytes": adj.table.numel() * 8, "pairs": adj._pairs[0]["np"]}


def main():
    from popcorn_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ps", type=int, default=2048)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    ps = a.ps
    yy, xx = torch.meshgrid(torch.arange(ps), torch.arange(ps), indexing="ij")
    fine, coarse = ((yy // 32) * (ps // 32) + xx // 32).to(torch.int32), ((yy // 256) * (ps // 256) + xx // 256).to(torch.int32)
    num_ids = [int(fine.max()) + 1, int(coarse.max()) + 1]
    pop = (torch.rand(num_ids[1], generator=torch.Generator().manual_seed(7)) * 50000).tolist()
    fd, cd = fine.cuda(), coarse.cuda()
    plan_ms = []
    for r in range(a.reps + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plane, pair_f, pair_c, base = ops.census_pair_plan(fd, cd, num_ids[0], num_ids[1])
        torch.cuda.synchronize()
        if r >= 3:
            plan_ms.append((time.perf_counter() - t0) * 1e3)
    plan_bytes = sum(t.numel() * t.element_size() for t in (plane, pair_f, pair_c, base))
    res = {"device": torch.cuda.get_device_name(0), "window": ps, "overlap": a.overlap, "num_ids": num_ids, "reps": a.reps,
           "batch": a.batch, "expected": EXPECTED, "plan_build_ms": round(float(np.median(plan_ms)), 3),
           "plan_build_min_ms": round(min(plan_ms), 3), "plan_bytes": plan_bytes,
           "runs": [bench_members(M, a, fine, coarse, num_ids, pop) for M in (1, 5)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
