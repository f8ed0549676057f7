"""Brute-force restatement of the NaN-fill contract (data/PopulationDataset.py:526-551 interpolate_nan, made deterministic):

  * known = not NaN (+-Inf is known);
  * no NaN: the array is returned unchanged;
  * NaNs and fewer than 4 known entries: the whole array becomes zeros;
  * otherwise every NaN at p = (c, i, j) takes A[q*], q* = the known q minimising (|p - q|^2, q_c, q_i, q_j) lexicographically --
    Euclidean distance in 3-D index space, compared exactly in integers, the value copied.

numpy only, in chunks over the missing entries.  ``tie_sets`` lists, for every missing entry, all known entries at the minimal distance
(scipy's k-d tree picks one of them in its own order)."""
from __future__ import annotations

import numpy as np


def _d2_chunks(miss, known, chunk):
    kc, ki, kj = (known[:, k].astype(np.int64) for k in range(3))
    for s in range(0, len(miss), chunk):
        m = miss[s:s + chunk].astype(np.int64)
        d2 = (m[:, 0:1] - kc) ** 2 + (m[:, 1:2] - ki) ** 2 + (m[:, 2:3] - kj) ** 2
        yield s, d2


def _chunk(n_known):
    return max(1, min(4096, (1 << 25) // max(n_known, 1)))


def nan_fill(a: np.ndarray) -> np.ndarray:
    """Filled copy of a (C, h, w) array."""
    a = np.array(a, copy=True)
    nan = np.isnan(a)
    if not nan.any():
        return a
    known = np.argwhere(~nan)                 # C order = lexicographic (c, i, j): argmin's first minimum is the tie rule
    if len(known) < 4:
        return np.zeros_like(a)
    miss = np.argwhere(nan)
    vals = a[tuple(known.T)]
    out = np.empty(len(miss), dtype=a.dtype)
    for s, d2 in _d2_chunks(miss, known, _chunk(len(known))):
        out[s:s + len(d2)] = vals[d2.argmin(1)]
    a[tuple(miss.T)] = out
    return a


def tie_sets(a: np.ndarray):
    """(missing (n, 3) indices, list of (k, 3) arrays: the known entries at minimal distance from each)."""
    nan = np.isnan(a)
    known = np.argwhere(~nan)
    miss = np.argwhere(nan)
    sets = []
    for _, d2 in _d2_chunks(miss, known, _chunk(len(known))):
        mn = d2.min(1, keepdims=True)
        for row, m in zip(d2, mn):
            sets.append(known[row == m[0]])
    return miss, sets


def nan_fill_batch(x: np.ndarray, hw=None) -> np.ndarray:
    """(B, C, H, W) with per-sample extents hw[b] = (h, w) anchored top-left: each extent filled on its own, the rest untouched."""
    x = np.array(x, copy=True)
    for b in range(x.shape[0]):
        h, w = (x.shape[2], x.shape[3]) if hw is None else (int(hw[b][0]), int(hw[b][1]))
        x[b, :, :h, :w] = nan_fill(x[b, :, :h, :w])
    return x


def nearest_value_box(a: np.ndarray, site, start=4):
    """The contract's value for ONE missing entry of a large (C, h, w) array, without a brute force over every known entry: search a
    growing box of in-plane half-width r around the site (all planes); once r exceeds the best in-plane distance found so far, no entry
    outside the box can be nearer (its in-plane offset alone is >= r + 1 > sqrt(best)), so the result is exact."""
    C, h, w = a.shape
    c0, i0, j0 = (int(v) for v in site)
    r = start
    while True:
        i_lo, i_hi, j_lo, j_hi = max(0, i0 - r), min(h, i0 + r + 1), max(0, j0 - r), min(w, j0 + r + 1)
        box = a[:, i_lo:i_hi, j_lo:j_hi]
        kn = np.argwhere(~np.isnan(box))
        covers = i_lo == 0 and j_lo == 0 and i_hi == h and j_hi == w
        if len(kn):
            q = kn + np.array([0, i_lo, j_lo])
            d2 = (q[:, 0] - c0) ** 2 + (q[:, 1] - i0) ** 2 + (q[:, 2] - j0) ** 2
            best = int(d2.min())
            if (r + 1) ** 2 > best or covers:
                k = int(d2.argmin())              # argwhere order inside the box is lexicographic too
                return a[tuple(q[k])]
        elif covers:
            return None
        r *= 2


def nan_fill_offsets(a: np.ndarray, radius=48) -> np.ndarray:
    """The same result as ``nan_fill`` for large arrays with local holes: for a fixed target, ordering the known sources by
    (|p - q|^2, q_c, q_i, q_j) is ordering the offsets q - p by (|d|^2, d_c, d_i, d_j), so the offsets of in-plane half-width <= radius
    are walked in that order and every target takes its first known source.  Offsets with |d|^2 <= radius^2 are all in the box, so a
    target resolved there is exact; the rest go through ``nearest_value_box``."""
    a = np.array(a, copy=True)
    nan = np.isnan(a)
    if not nan.any():
        return a
    if (~nan).sum() < 4:
        return np.zeros_like(a)
    C, h, w = a.shape
    r = np.arange(-radius, radius + 1)
    dc, di, dj = np.meshgrid(np.arange(-(C - 1), C), r, r, indexing="ij")
    d2 = dc ** 2 + di ** 2 + dj ** 2
    keep = d2 <= radius * radius
    off = np.stack([d2[keep], dc[keep], di[keep], dj[keep]], 1)
    off = off[np.lexsort((off[:, 3], off[:, 2], off[:, 1], off[:, 0]))]
    todo = np.argwhere(nan)
    src = a.copy()
    for _, oc, oi, oj in off:
        if not len(todo):
            break
        q = todo + np.array([oc, oi, oj])
        ok = (q[:, 0] >= 0) & (q[:, 0] < C) & (q[:, 1] >= 0) & (q[:, 1] < h) & (q[:, 2] >= 0) & (q[:, 2] < w)
        hit = np.zeros(len(todo), dtype=bool)
        qi = q[ok]
        hit[ok] = ~nan[qi[:, 0], qi[:, 1], qi[:, 2]]
        if hit.any():
            t, s = todo[hit], q[hit]
            a[t[:, 0], t[:, 1], t[:, 2]] = src[s[:, 0], s[:, 1], s[:, 2]]
            todo = todo[~hit]
    for t in todo:
        a[tuple(t)] = nearest_value_box(src, t)
    return a
