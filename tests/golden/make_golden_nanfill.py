#!/usr/bin/env python3
"""Generate tests/golden/g13_nan_fill.npz: the REFERENCE ``Population_Dataset.interpolate_nan`` (data/PopulationDataset.py:526-551,
scipy griddata "nearest") on seeded NaN patterns.  Like make_golden.py it runs in the build container only, imports the reference
through ``make_golden.import_reference()`` and the rasterio stub of g9, and copies no reference source: it records inputs and outputs.

    python tests/golden/make_golden_nanfill.py

Per case ``<name>/input`` and ``<name>/output`` (float32, (C, h, w)).  ``interpolate_nan`` uses no instance state, so it is called
unbound."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden  # noqa: E402


def discs(rng, a, n, rmin, rmax, channels=None):
    C, h, w = a.shape
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(rmin, rmax)
        m = (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        for c in (range(C) if channels is None else channels):
            a[c][m] = np.nan


def cases():
    rng = np.random.default_rng(1313)
    out = {}
    a = rng.normal(1000.0, 300.0, (4, 96, 128)).astype(np.float32)
    discs(rng, a, 9, 3, 14)
    discs(rng, a, 4, 2, 6, channels=[1])
    out["clouds"] = a
    a = rng.normal(0.0, 1.0, (4, 40, 50)).astype(np.float32)
    a[2][rng.random((40, 50)) < 0.12] = np.nan
    out["scattered_one_channel"] = a
    a = rng.normal(0.0, 1.0, (4, 30, 40)).astype(np.float32)
    a[:, 7, :] = np.nan
    a[:, :, 13] = np.nan
    a[1, 20:23, 30:33] = np.nan
    out["row_col"] = a
    a = rng.normal(-12.0, 4.0, (2, 200, 160)).astype(np.float32)
    a[1] = np.nan
    discs(rng, a, 3, 4, 10, channels=[0])
    out["s1_plane"] = a
    a = rng.normal(0.0, 1.0, (4, 24, 36)).astype(np.float32)
    a[:, :, 0] = np.nan                # width-1 stripe along the left edge, every channel
    a[:, -2:, :] = np.nan              # width-2 stripe along the bottom edge
    out["tie_free"] = a
    a = np.full((4, 6, 7), np.nan, dtype=np.float32)
    a[0, 1, 2], a[2, 5, 6], a[3, 0, 0] = 1.5, -2.0, 7.25
    out["few_known"] = a
    out["nan_free"] = rng.normal(0.0, 1.0, (2, 20, 30)).astype(np.float32)
    return out


def main():
    make_golden.import_reference()
    make_golden._stub_rasterio()
    import data.PopulationDataset as PD
    fill = PD.Population_Dataset.interpolate_nan
    res = {}
    for name, a in cases().items():
        res[f"{name}/input"] = a.copy()
        res[f"{name}/output"] = np.asarray(fill(None, a.copy()), dtype=np.float32)
    np.savez_compressed(os.path.join(HERE, "g13_nan_fill.npz"), **res)


if __name__ == "__main__":
    main()
