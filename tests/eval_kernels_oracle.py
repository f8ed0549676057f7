"""Float64 / int64 numpy yardsticks of the whole-raster evaluation kernels of csrc/census.hip (segment sum, dasymetric rescale, window
stitcher, its finalize, batched visit count), the derived bars they are held to, an fp32 restatement of the stitcher with switchable
planted defects, and the inputs of tests/test_gpu_eval_kernels.py -- shared with tests/test_eval_kernels_cpu.py, which checks on the
same inputs that an honest fp32 evaluation stays inside the bars and that every planted defect is rejected.  CPU only.

Coordinates as in eval.py: a window is (xl, yl, pd[M, psx, psy], sc or None[, overlap]); xl is its ROW origin, yl its COLUMN origin, psx
its row extent, psy its column extent.  Its interior (border of ``overlap`` excluded) is clipped to the raster on all four sides; the
window's own element of raster pixel (r, c) is (r - xl, c - yl).

Derived bars of the finalised maps (nothing here is measured).  u = 2^-24.  A pixel has c = sum of M over the windows that cover it,
terms v_1 .. v_c >= 0 (fp32 numbers), S = sum v, Q = sum v^2.
  mean.  Any order of c - 1 fp32 additions leaves |fl(S) - S| <= (c - 1) u sum|v| to first order; the division rounds once more:
      |mean - S / c| <= c u sum|v| / c; the bar is (c + 1) u sum|v| / c (one u of slack for the second-order terms).
  (c - 1) std^2.  fl(Q): every term passes one rounding of its square (none where the compiler fuses it) and at most c - 1 additions:
      c u Q.  m^2 c: m carries c u relative, its square 2 c u + u, the product with c one more u (none where fused): (2c + 2) u times
      S^2 / c <= Q (Cauchy-Schwarz).  The subtraction, the division by c - 1 and the root (2 u on the square) add 4 u of a value <= Q.
      First order: (3c + 6) u Q.  The bar is (3c + 10) u Q: second-order terms (c <= 12 here: below 2^-19 of the first) and the float64
      evaluation of the yardstick itself fit in the difference many times over.
  NaN.  The device takes the root of a negative difference only where the true (c - 1) var is within that bar of 0: a NaN is allowed
      only there."""
import math

import numpy as np

U = 2.0 ** -24
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def interior(xl, yl, psx, psy, ov, h, w):
    """rows [x0, x1) x columns [y0, y1) of the interior clipped to the raster; empty where psx or psy <= 2 ov or it lies outside"""
    if psx <= 2 * ov or psy <= 2 * ov:
        return 0, 0, 0, 0
    return max(xl + ov, 0), min(xl + psx - ov, h), max(yl + ov, 0), min(yl + psy - ov, w)


def _unpack(win, overlap):
    xl, yl, pd, sc = win[:4]
    return int(xl), int(yl), pd, sc, (int(win[4]) if len(win) > 4 else int(overlap))


# ---- stitcher, float64 ---------------------------------------------------------------------------------------------------------------------
def _stitch64_plane(h, w, windows, overlap, which, count):
    """sum, sum of squares, sum of |v| (float64) of plane ``which`` (2: popdense, 3: scale) and its second central moment about the mean
    over ALL c visits (a window without the plane enters as c zeros, as on the device)"""
    s, q, a = (np.zeros((h, w)) for _ in range(3))
    for win in windows:
        xl, yl, _, _, ov = _unpack(win, overlap)
        v = win[which]
        if v is None:
            continue
        v = np.asarray(v, dtype=np.float64)
        x0, x1, y0, y1 = interior(xl, yl, v.shape[1], v.shape[2], ov, h, w)
        if x1 > x0 and y1 > y0:
            t = v[:, x0 - xl:x1 - xl, y0 - yl:y1 - yl]
            s[x0:x1, y0:y1] += t.sum(0)
            q[x0:x1, y0:y1] += (t * t).sum(0)
            a[x0:x1, y0:y1] += np.abs(t).sum(0)
    mean = np.divide(s, count, out=np.zeros((h, w)), where=count > 0)
    m2, seen = np.zeros((h, w)), np.zeros((h, w), dtype=np.int64)
    for win in windows:
        xl, yl, _, _, ov = _unpack(win, overlap)
        v = win[which]
        if v is None:
            continue
        v = np.asarray(v, dtype=np.float64)
        x0, x1, y0, y1 = interior(xl, yl, v.shape[1], v.shape[2], ov, h, w)
        if x1 > x0 and y1 > y0:
            d = v[:, x0 - xl:x1 - xl, y0 - yl:y1 - yl] - mean[x0:x1, y0:y1]
            m2[x0:x1, y0:y1] += (d * d).sum(0)
            seen[x0:x1, y0:y1] += v.shape[0]
    m2 += (count - seen) * mean * mean
    return {"sum": s, "sq": q, "abs": a, "mean": mean, "m2": m2}


def stitch64(h, w, windows, overlap):
    """The stitcher in float64.  Returns {"count": int64 c, "pd": {...}, "sc": {...}} with per plane: sum, sq (sum of squares), abs (sum of
    |v|), mean (sum / c, 0 where c = 0) and m2 = (c - 1) var = sum over the c visits of (v - mean)^2, all (h, w) float64."""
    count = np.zeros((h, w), dtype=np.int64)
    for win in windows:
        xl, yl, pd, _, ov = _unpack(win, overlap)
        x0, x1, y0, y1 = interior(xl, yl, pd.shape[1], pd.shape[2], ov, h, w)
        if x1 > x0 and y1 > y0:
            count[x0:x1, y0:y1] += pd.shape[0]
    return {"count": count, "pd": _stitch64_plane(h, w, windows, overlap, 2, count),
            "sc": _stitch64_plane(h, w, windows, overlap, 3, count)}


def count64(h, w, windows, M, ps, overlap):
    """visit counts: count[r][c] += M for every (row origin, column origin) of ``windows`` whose clipped interior covers (r, c)"""
    count = np.zeros((h, w), dtype=np.int64)
    for x, y in windows:
        x0, x1, y0, y1 = interior(int(x), int(y), ps, ps, overlap, h, w)
        if x1 > x0 and y1 > y0:
            count[x0:x1, y0:y1] += M
    return count


def mean_bar(c, abs_sum):
    return (c + 1) * U * abs_sum / np.maximum(c, 1)


def var_bar(c, sq_sum):
    return (3 * c + 10) * U * sq_sum


def judge(name, mean, std, count, ref, rows=None):
    """The rules of the module docstring for one finalised plane (fp32 arrays ``mean`` / ``std``, ``ref`` = a plane of stitch64) on the
    pixels with c > 1 (of ``rows`` = (r0, r1) only, where given).  Returns (ok, report): worst ratio to each bar, NaN sites, the site of
    the first violation."""
    sel = count > 1
    if rows is not None:
        band = np.zeros_like(sel)
        band[rows[0]:rows[1]] = True
        sel &= band
    c = count[sel].astype(np.float64)
    m, s = mean[sel].astype(np.float64), std[sel].astype(np.float64)
    mb, vb = mean_bar(c, ref["abs"][sel]), var_bar(c, ref["sq"][sel])
    em = np.abs(m - ref["mean"][sel])
    nan = np.isnan(s)
    ev = np.where(nan, 0.0, np.abs((c - 1) * s * s - ref["m2"][sel]))
    bad_nan = nan & ~(ref["m2"][sel] <= vb)
    with np.errstate(divide="ignore", invalid="ignore"):
        rm = np.where(mb > 0, em / mb, np.where(em > 0, np.inf, 0.0))
        rv = np.where(vb > 0, ev / vb, np.where(ev > 0, np.inf, 0.0))
    ok = bool((rm <= 1).all() and (rv <= 1).all() and not bad_nan.any() and not np.isnan(m).any())
    rep = (f"[{name}] {int(sel.sum())} pixels: mean worst {rm.max() if rm.size else 0:.3f} of its bar, (c-1)var worst "
           f"{rv.max() if rv.size else 0:.3f} of its bar, NaN at {int(nan.sum())} (outside the cancellation zone: {int(bad_nan.sum())})")
    return ok, rep


# ---- stitcher, fp32 restatement with switchable defects -----------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _fma32(a, b, c):
    """fl32(a * b + c) through float64: the product of two fp32 numbers is exact there"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def stitch32(h, w, windows, overlap, with_scale=True, contract=False, reverse=False, defects=()):
    """csrc/census.hip's stitcher step by step in np.float32: per window the members' sum and sum of squares from 0 (members taken in
    reverse order where ``reverse``), one ``+=`` of each into the planes, count += M; then ``finalize32``.  ``contract``: the two
    contractions the compiler makes (s2 = fma(v, v, s2) and fma(-(m m), c, sq)) emulated through float64; otherwise every product is
    rounded.  ``defects``: names of planted defects (tests/test_eval_kernels_cpu.py).  Returns (planes before finalize, after finalize),
    each {"out", "out_sq", "scale", "scale_sq", "count"} (scale planes None without ``with_scale``)."""
    d = set(defects)
    P = {k: np.zeros((h, w), dtype=np.float32) for k in ("out", "out_sq", "scale", "scale_sq")}
    count = np.zeros((h, w), dtype=np.int16)
    for win in windows:
        xl, yl, pd, sc, ov = _unpack(win, overlap)
        M, psx, psy = pd.shape
        if psx <= 2 * ov or psy <= 2 * ov:
            continue
        ex, ey = (psy, psx) if "extents_swapped" in d else (psx, psy)
        x0, y0 = xl + ov, yl + ov
        if "no_top_left_clip" not in d:
            x0, y0 = max(x0, 0), max(y0, 0)
        x1, y1 = min(xl + ex - ov, h - 1 if "bottom_off_by_one" in d else h), min(yl + ey - ov, w)
        if x1 <= x0 or y1 <= y0:
            continue
        rr, cc = np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), indexing="ij")
        gr, gc = rr % h, cc % w                       # (a store before the plane lands somewhere else; here it wraps)
        members = list(range(M))[::-1] if reverse else list(range(M))
        if "member_dropped" in d:
            members = members[:-1]
        for plane, key, key2 in ((pd, "out", "out_sq"), (sc if with_scale else None, "scale", "scale_sq")):
            if plane is None:
                continue
            flat = _f32(plane).reshape(M, -1)
            at = ((rr - xl) * (psy if "extents_swapped" not in d else psx) + (cc - yl)) % flat.shape[1]
            s, s2 = np.zeros(rr.shape, np.float32), np.zeros(rr.shape, np.float32)
            for m in members:
                v = flat[m][at]
                s = s + v
                s2 = _fma32(v, v, s2) if contract else s2 + v * v
            P[key][gr, gc] += s
            P[key2][gr, gc] += s2
        count[gr, gc] += 1 if "count_plus_one" in d else M
    if not with_scale:
        P["scale"] = P["scale_sq"] = None
    before = {**{k: (None if v is None else v.copy()) for k, v in P.items()}, "count": count.copy()}
    after = dict(before)
    for key, key2 in (("out", "out_sq"), ("scale", "scale_sq")):
        if P[key] is not None:
            after[key], after[key2] = finalize32(P[key], P[key2], count, contract, d)
    return before, after


def finalize32(s, q, count, contract=False, defects=(), rows=None):
    """stitch_finalize_kernel in np.float32: where c > 1: m = s / c; std = sqrt((q - (m m) c) / (c - 1)); elsewhere untouched"""
    d = set(defects)
    s, q = s.copy(), q.copy()
    sel = count >= 1 if "c_ge_1" in d else count > 1
    if rows is not None:
        band = np.zeros_like(sel)
        band[rows[0]:rows[1]] = True
        sel &= band
    fc = count[sel].astype(np.float32)
    m = s[sel] / fc
    mm = m * m
    diff = _fma32(-mm, fc, q[sel]) if contract else q[sel] - mm * fc
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(diff / (fc if "n_for_n_minus_1" in d else fc - np.float32(1)))
    s[sel], q[sel] = m, sd
    return s, q


# ---- segment sum and rescale ---------------------------------------------------------------------------------------------------------------
def segment64(pred, boundary, num_ids, defects=()):
    """EXACT sums[id] of pred over the elements with boundary == id, id in [0, num_ids) (anything else is ignored), rounded once to
    float64, and int64 counts.  Integer-valued finite pred: an int64 sum; otherwise math.fsum per id (NaN / inf propagate)."""
    d = set(defects)
    p = np.asarray(pred, dtype=np.float64).ravel()
    b = np.asarray(boundary).astype(np.int64).ravel()
    if "tail_lost" in d:
        keep = len(p) - len(p) % 4
        p, b = p[:keep], b[:keep]
    ok = (b >= 0) & ((b <= num_ids) if "id_num_ids_counted" in d else (b < num_ids))
    p, b = p[ok], np.minimum(b[ok], num_ids - 1)
    counts = np.bincount(b, minlength=num_ids).astype(np.int64)
    if p.size == 0 or (np.isfinite(p).all() and (p == np.rint(p)).all() and np.abs(p).max() < 2.0 ** 52):
        sums = np.zeros(num_ids, dtype=np.int64)
        np.add.at(sums, b, p.astype(np.int64))
        return sums.astype(np.float64), counts
    order = np.argsort(b, kind="stable")
    p, b = p[order], b[order]
    edges = np.searchsorted(b, np.arange(num_ids + 1))
    sums = np.zeros(num_ids)
    for i in np.flatnonzero(counts):
        seg = p[edges[i]:edges[i + 1]]
        sums[i] = math.fsum(seg) if np.isfinite(seg).all() else seg.sum()
    return sums, counts


def adjust32(pred, boundary, sums64, pop, has):
    """census_adjust_kernel step by step in np.float32: s = f32(sum), q = f32(pop / s), f32(pred * q); a pixel is untouched where
    s == 0, where there is no census entry (has[id] == 0) or where its id lies outside [0, num_ids)."""
    num_ids = len(sums64)
    out = _f32(pred).copy()
    flat, b = out.reshape(-1), np.asarray(boundary).astype(np.int64).ravel()
    s = _f32(sums64)
    ok = (b >= 0) & (b < num_ids)
    idc = np.where(ok, b, 0)
    ok &= (np.asarray(has)[idc] != 0) & (s[idc] != 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = _f32(pop)[idc] / s[idc]
        flat[ok] = (flat * q)[ok]
    return out


# ---- the inputs of tests/test_gpu_eval_kernels.py ------------------------------------------------------------------------------------------
H, W, OV = 37, 45, 4
BAND = (7, 30)          # rows of the banded finalize: starts at an odd row of the odd-width raster (a 4-byte phase of the planes)

# (row origin, column origin, (psx, psy), repeats): interiors of A .. F are disjoint, so a pixel's visit count is its window's repeats
#   A sticks out at the top-left corner, B at the top, C at the left, D at the bottom-right corner, E at the bottom, F at the right
_GEOMETRY = {"A": (-8, -10, (24, 40)), "B": (-10, 22, (40, 24)), "C": (8, -14, (24, 40)), "D": (22, 31, (40, 24)), "E": (24, -2, (24, 40)),
             "F": (0, 38, (24, 40))}
_OUTSIDE = [(-30, 3, (24, 40)), (5, 60, (40, 24))]      # interiors above / right of the raster


def _ints(rng, M, shape):
    return rng.integers(0, 8, size=(M,) + shape).astype(np.float32)


def exact_windows(M, seed=0, scale="all"):
    """Integer values 0 .. 7 on the 37 x 45 raster: rectangular windows of both orientations with overlap 4, sticking out on all four
    sides and at two corners, visited 1, 2, 4 and 8 times, two windows entirely outside, one window with overlap 0 (over B and the
    uncovered strip) and one with ps <= 2 overlap.  ``scale``: "all" / "none" / "some" (every third window passes scale=None)."""
    rng = np.random.default_rng(1000 + seed + M)
    wins = []
    for name, rep in (("A", 1), ("C", 2), ("E", 4), ("B", 8), ("D", 1), ("F", 2)):
        xl, yl, shp = _GEOMETRY[name]
        wins += [(xl, yl, _ints(rng, M, shp), _ints(rng, M, shp), OV) for _ in range(rep)]
    wins += [(xl, yl, _ints(rng, M, shp), _ints(rng, M, shp), OV) for xl, yl, shp in _OUTSIDE]
    wins.append((20, 21, _ints(rng, M, (5, 7)), _ints(rng, M, (5, 7)), 0))
    wins.append((3, 3, _ints(rng, M, (8, 30)), _ints(rng, M, (8, 30)), OV))          # 8 <= 2 * 4: adds nothing
    order = rng.permutation(len(wins))
    wins = [wins[i] for i in order]
    if scale == "none":
        wins = [(a, b, pd, None, ov) for a, b, pd, sc, ov in wins]
    elif scale == "some":
        wins = [(a, b, pd, None if i % 3 == 0 else sc, ov) for i, (a, b, pd, sc, ov) in enumerate(wins)]
    return wins


MANTISSA_M = 3
_PAD = 64


def mantissa_windows(kind, seed=0):
    """M = 3 full-mantissa non-negative windows on the same geometry, visited 1, 2 and 4 times (c = 3, 6, 12).  "spread": uniform values;
    "near": every visit of a pixel is that pixel's base value times (1 + k 2^-23), k = 0 .. 3 -- the ensemble differs in the last ulps."""
    rng = np.random.default_rng(2000 + seed)
    base = {k: (0.5 + 1.5 * rng.random((H + 2 * _PAD, W + 2 * _PAD))).astype(np.float32) for k in ("pd", "sc")}

    def draw(key, xl, yl, shp):
        if kind == "spread":
            return (rng.random((MANTISSA_M,) + shp) * np.float32(3.0)).astype(np.float32)
        b = base[key][xl + _PAD:xl + _PAD + shp[0], yl + _PAD:yl + _PAD + shp[1]]
        k = rng.integers(0, 4, size=(MANTISSA_M,) + shp)
        return (b[None].astype(np.float64) * (1 + k * 2.0 ** -23)).astype(np.float32)

    wins = []
    for name, rep in (("A", 1), ("C", 2), ("E", 4), ("B", 2), ("D", 1), ("F", 4)):
        xl, yl, shp = _GEOMETRY[name]
        wins += [(xl, yl, draw("pd", xl, yl, shp), draw("sc", xl, yl, shp), OV) for _ in range(rep)]
    xl, yl, shp = _OUTSIDE[0]
    wins.append((xl, yl, draw("pd", xl, yl, shp), draw("sc", xl, yl, shp), OV))
    return [wins[i] for i in rng.permutation(len(wins))]


ACC_PS, ACC_M, ACC_IDS = 24, 2, 7


def accumulators_case(seed=0):
    """Square 24 x 24 windows (what ProductGrid / CensusTable take: one patch size per list), overlap 4, integer values, on the 37 x 45
    raster: a 3 x 4 grid of disjoint interiors that sticks out on every side, three of them revisited (visit counts 1, 2, 4 -- powers of
    two, so every division by the visit count is exact), one window outside.  Returns (windows, boundary int32 (H, W), num_ids)."""
    rng = np.random.default_rng(3000 + seed)
    origins = [(x, y) for x in (-12, 4, 20) for y in (-10, 6, 22, 38)]
    origins += [(-12, -10), (20, 38)] + [(4, 6)] * 3 + [(60, 0)]
    wins = [(x, y, _ints(rng, ACC_M, (ACC_PS, ACC_PS)), None, OV) for x, y in origins]
    wins = [wins[i] for i in rng.permutation(len(wins))]
    b = ((np.arange(H)[:, None] // 13) * 3 + np.arange(W)[None, :] // 16).astype(np.int32)      # ids 0 .. 8: 7 and 8 are out of range
    b[:2] = -1
    b[5, 5], b[6, 6] = INT_MIN, INT_MAX
    return wins, b, ACC_IDS


COUNT_PS, COUNT_OV = 6, 1
CW_CAP = 1024                                # windows per LDS batch of stitch_count_windows_kernel (csrc/census.hip)


def kernel_rows(wins, h, w, ps=COUNT_PS, ov=COUNT_OV):
    """the windows of ``wins`` that eval.count_windows hands to pc_stitch_count_windows, in order: it clips the interior at the bottom and
    right only and drops a window whose interior is empty after that (one that begins at or beyond the last row / column); a window
    wholly above or left of the raster stays in the list and matches no pixel in the kernel"""
    return [(x, y) for x, y in wins if min(x + ps - ov, h) > min(x + ov, h) and min(y + ps - ov, w) > min(y + ov, w)]


def count_case(nwin, h, w, seed=0):
    """Window origins for a visit count with patch 6, overlap 1 (interior 4 x 4) of which EXACTLY ``nwin`` reach the kernel
    (``kernel_rows``): from wholly above / left of the raster (they reach it) to partly below / right of it; a further nwin // 8 + 3
    windows that begin at or beyond the last row / column (the host drops them) are scattered through the list.  The last raster row is
    kept free of the random windows: kernel row CW_CAP - 1 (the last of the first LDS batch) alone covers pixel (h - 1, 0) and kernel row
    CW_CAP (the first of the second batch) alone covers pixel (h - 1, w - 1), where the list is that long."""
    ps, ov = COUNT_PS, COUNT_OV
    rng = np.random.default_rng(4000 + seed + 7 * nwin + w)
    hi = h - ps + ov - 1                                                 # interior rows end at x + ps - ov <= h - 1
    rows = [(int(x), int(y)) for x, y in zip(rng.integers(-7, hi + 1, nwin), rng.integers(-7, w - ov, nwin))]
    if nwin == 1:
        rows[0] = (-2, -3)
    if nwin >= CW_CAP:
        rows[CW_CAP - 1] = (h - 1 - ov, ov - ps + 1)                     # interior: row h - 1 (and below), column 0 (and left of it)
    if nwin > CW_CAP:
        rows[CW_CAP] = (h - 1 - ov, w - 1 - ov)                          # interior: row h - 1, column w - 1
    if nwin > 2 * CW_CAP:
        rows[2 * CW_CAP] = (1, 0)                                        # the one window of the third batch lies inside the raster
    wins = list(rows)
    for k in range(nwin // 8 + 3):                                       # dropped by the host: they never become kernel rows
        out = (h - ov + int(rng.integers(0, 4)), int(rng.integers(-7, w))) if k % 2 else (int(rng.integers(-7, h)), w - ov + int(rng.integers(0, 4)))
        wins.insert(int(rng.integers(0, len(wins) + 1)), out)
    assert kernel_rows(wins, h, w) == rows
    return wins


TALL = (65540, 3, [(65531, -1), (65533, 0), (65536, -2), (65538, 1), (0, 0), (3, -1), (30000, 0), (65529, -4), (-3, 0)])


def segment_case(num_ids, n, seed=0):
    """pred (n + 3 integer-valued fp32, |v| < 2^20) and ids (n + 3 int32) buffers: views [p : p + n] for p = 0 .. 3 give the alignment
    phases.  The ids -1, INT_MIN, INT_MAX and num_ids are present (and must be ignored)."""
    rng = np.random.default_rng(5000 + seed + 31 * n + num_ids)
    pred = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=n + 3).astype(np.float32)
    ids = rng.integers(0, num_ids, size=n + 3).astype(np.int64)
    special = [-1, INT_MIN, INT_MAX, num_ids]
    if n + 3 >= 64:
        at = rng.choice(n + 3, size=32, replace=False)
        ids[at] = np.tile(special, 8)
    else:
        ids[1::2] = (special * 3)[:len(ids[1::2])]
    return pred, ids.astype(np.int32)


# ---- the verdicts of tests/test_gpu_eval_kernels.py (numpy in, list of failures out: the CPU file feeds them restatements) ---------------
EXACT_C = (2, 4, 8)
PLANES = (("out", "out_sq", "pd"), ("scale", "scale_sq", "sc"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def exact_conditions(ref, M):
    """asserted on the oracle before any launch: every c of {2, 4, 8} that M divides occurs, so do c = 0 and (M = 1) c = 1, and at least
    20 % of the finalised pixels have a non-zero variance"""
    c = ref["count"]
    for k in EXACT_C:
        assert k % M or (c == k).any(), (M, k)
    assert (c == 0).any() and (M > 1 or (c == 1).any())
    fin = c > 1
    assert fin.any() and (ref["pd"]["m2"][fin] > 0).mean() >= 0.2


def exact_verdict(before, after, windows, with_scale=True, band=None):
    """before / after: {"out", "out_sq", "scale", "scale_sq", "count"} as numpy arrays (None for absent scale planes) before and after
    ``finalize`` (on rows ``band`` = (r0, r1) only, where given).  Integer inputs: the planes before finalize equal the float64 sums; after
    it, pixels with c in {2, 4, 8} equal the np.float32 evaluation bit for bit, pixels with c = 1 keep their sums, pixels with c = 0 stay
    0, rows outside the band are untouched, and any other c > 1 obeys the derived bars."""
    ref = stitch64(H, W, windows, OV)
    c = ref["count"]
    fails = []
    if not np.array_equal(before["count"].astype(np.int64), c) or not np.array_equal(after["count"].astype(np.int64), c):
        fails.append("count")
    r0, r1 = band if band is not None else (0, H)
    inband = np.zeros((H, W), dtype=bool)
    inband[r0:r1] = True
    for key, key2, name in PLANES[:2 if with_scale else 1]:
        s64, q64 = ref[name]["sum"], ref[name]["sq"]
        assert np.array_equal(s64.astype(np.float32).astype(np.float64), s64) and np.array_equal(q64.astype(np.float32).astype(np.float64), q64)
        if not np.array_equal(_bits(before[key]), _bits(s64)) or not np.array_equal(_bits(before[key2]), _bits(q64)):
            fails.append(f"{key}/{key2} before finalize")
            continue
        want_m, want_s = finalize32(s64.astype(np.float32), q64.astype(np.float32), c.astype(np.int16), rows=(r0, r1))
        pow2 = np.isin(c, EXACT_C) & inband
        for got, want, what in ((after[key], want_m, key), (after[key2], want_s, key2)):
            if not np.array_equal(_bits(got)[pow2], _bits(want)[pow2]):
                fails.append(f"{what} after finalize, c in {EXACT_C}")
            keep = (c <= 1) | ~inband
            if not np.array_equal(_bits(got)[keep], _bits(before[what])[keep]):
                fails.append(f"{what} after finalize, pixels that must keep their sums")
        ok, rep = judge(key, after[key], after[key2], np.where(np.isin(c, EXACT_C), 0, c), ref[name], rows=(r0, r1))
        if not ok:
            fails.append(rep)
    return fails


def mantissa_conditions(ref, kind):
    """asserted on the oracle before any launch.  spread: at least 90 % of the finalised pixels have (c - 1) var > 100 x its bar.  near: at
    least 1 % lie inside the cancellation zone ((c - 1) var <= the bar).  c reaches 3, 6 and 12."""
    c = ref["count"]
    assert all((c == k).any() for k in (3, 6, 12)) and (c == 0).any() and not ((c > 0) & (c < 3)).any()
    fin = c > 1
    for name in ("pd", "sc"):
        m2, bar = ref[name]["m2"][fin], var_bar(c[fin], ref[name]["sq"][fin])
        assert (ref[name]["sum"][fin] >= 0).all()
        if kind == "spread":
            assert (m2 > 100 * bar).mean() >= 0.9, (m2 > 100 * bar).mean()
        else:
            assert (m2 <= bar).mean() >= 0.01, (m2 <= bar).mean()


def mantissa_verdict(after, windows, kind):
    """the derived bars and the NaN rule on both finalised planes against stitch64; on the spread input no NaN at all.  Returns (failures,
    reports)."""
    ref = stitch64(H, W, windows, OV)
    c = ref["count"]
    fails, reports = [], []
    if not np.array_equal(after["count"].astype(np.int64), c):
        fails.append("count")
    for key, key2, name in PLANES:
        ok, rep = judge(f"{kind} {key}", after[key], after[key2], c, ref[name])
        reports.append(rep)
        if not ok:
            fails.append(rep)
        if kind == "spread" and np.isnan(after[key2]).any():
            fails.append(f"{key2}: NaN on the spread input")
        if after[key][c == 0].any() or after[key2][c == 0].any():
            fails.append(f"{key}: unvisited pixels not 0")
    return fails, reports
