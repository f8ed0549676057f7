#!/usr/bin/env python3
"""Generate tests/golden/g14_split.npz: the row order and the two cuts of the reference's 80 / 20 census split
(data/PopulationDataset.py:105-121) as pandas itself makes them -- ``DataFrame.sample(frac=1, random_state=1610)``, then
``[:int(n * 0.8)]`` (train) and ``[int(n * 0.8):]`` (val) -- for tables of n = 1, 2, 5, 37 and 400 rows.  It runs where pandas is
installed (the package itself never imports pandas), needs nothing of the reference and records results only:

    python tests/golden/make_golden_split.py

Per n: ``n<n>/order`` (the original row numbers in the shuffled order), ``n<n>/train`` and ``n<n>/val`` (the ``idx`` column of the two
cuts after ``reset_index``), all int64.  The ``idx`` column holds 7 * row + 3, so a test cannot confuse ids with positions."""
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 5, 37, 400)
SEED, FRAC = 1610, 0.8


def main():
    out = {}
    for n in SIZES:
        df = pd.DataFrame({"idx": 7 * np.arange(n, dtype=np.int64) + 3, "POP20": np.arange(n, dtype=np.float32) * 1.5})
        shuffled = df.sample(frac=1, random_state=SEED)
        out[f"n{n}/order"] = shuffled.index.to_numpy().astype(np.int64)
        train = df.sample(frac=1, random_state=SEED)[:int(len(df) * FRAC)].reset_index(drop=True)
        val = df.sample(frac=1, random_state=SEED)[int(len(df) * FRAC):].reset_index(drop=True)
        out[f"n{n}/train"] = train["idx"].to_numpy().astype(np.int64)
        out[f"n{n}/val"] = val["idx"].to_numpy().astype(np.int64)
    path = os.path.join(HERE, "g14_split.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} (pandas {pd.__version__}): " + ", ".join(f"n = {n}: {len(out[f'n{n}/train'])} + {len(out[f'n{n}/val'])}" for n in SIZES))


if __name__ == "__main__":
    main()
