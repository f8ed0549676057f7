"""Single-product known answers for the fp32 matrix kernels (CPU-only helper).

The operands of a launch are arranged so that every checked output element is exactly ONE product a * b of two full-mantissa fp32
numbers (times exact factors +-1 or 2^k).  The float64 reference of the same op is then exact, and the bar is the arithmetic's own,
element by element, relative to that element:

  pattern P ("permutation weights", data paths): one non-zero weight per output channel (forward) or per input channel (data
      gradient); launch k of a Latin-square family puts channel c on index (c * STRIDE + k) mod (9 * C) of the other two axes, so the
      9 * C launches of a family visit every (co, ci, tap) triple once;
  pattern S ("sparse gradient", weight / bias gradients and the data gradient at named pixels): one non-zero per gradient channel
      over the whole batch, the positions pairwise >= 3 apart (Chebyshev) inside an image, x and w dense.

Bars (``check``):
  "fp32mfma"  one fused multiply-add into a zero accumulator:            |got - ref| <= 2^-23 |ref|
  "split"     six exact partial products of two 3-way bf16 splits, three dropped terms (<= 3 * 2^-24 of the product), five fp32
              additions of partial sums <= (1 + 2^-7) |ab| that round or truncate by <= 2^-23 each: 13 * 2^-24 < 2^-20:
                                                                        |got - ref| <= 2^-20 |ref|
  with ``prev`` (the += forms) one more rounding of the sum:            ... + 2^-24 |prev + ref|
Where the reference is 0 the result must be +-0."""
import itertools

import torch
import torch.nn.functional as F

STRIDE = 7                     # coprime to 9 * C for every channel count used (2, 4, 8, 16, 32): channels of a launch sit on distinct indices
W_MIN = 2.0 ** -6              # weights below it are redrawn: every product keeps a full-size mantissa
BAR = {"fp32mfma": 2.0 ** -23, "split": 2.0 ** -20}
SPACING = 3


# ---- values -----------------------------------------------------------------------------------------------------------------------------

def full_mantissa(shape, gen, scale=0.2, floor=W_MIN):
    """scale * randn in fp32 with |v| >= floor (redrawn where smaller): no value whose product underflows the bar's meaning"""
    v = torch.randn(shape, generator=gen) * scale
    for _ in range(64):
        small = v.abs() < floor
        if not bool(small.any()):
            return v
        v = torch.where(small, torch.randn(shape, generator=gen) * scale, v)
    raise AssertionError("full_mantissa: could not draw values above the floor")


def bn_pow2(c):
    """BN parameters whose folded scale is exactly 2^k, k distinct per channel (gamma = 2^k, var = 1, mean = beta = 0, eps = 0.0):
    returns (gamma, beta, mean, var, eps, scale)"""
    k = torch.arange(c) - c // 2
    gamma = torch.pow(torch.tensor(2.0), k.float())
    return gamma, torch.zeros(c), torch.zeros(c), torch.ones(c), 0.0, gamma.clone()


# ---- pattern P --------------------------------------------------------------------------------------------------------------------------

def pattern_p_index(n_chan, n_other, k):
    """flat index into the (other, tap) space of size 9 * n_other for each of the n_chan channels of launch k"""
    n = 9 * n_other
    return [(c * STRIDE + k) % n for c in range(n_chan)]


def pattern_p_forward(cout, cin, k, gen):
    """weights [cout][cin][3][3] with one non-zero per OUTPUT channel, at flat (ci, tap) index (co * STRIDE + k) mod (9 cin)"""
    w = torch.zeros(cout, cin * 9)
    idx = torch.tensor(pattern_p_index(cout, cin, k))
    w[torch.arange(cout), idx] = full_mantissa((cout,), gen)
    w = w.view(cout, cin, 3, 3)
    nz = (w != 0).double()
    assert float(F.conv2d(torch.ones(1, cin, 5, 5, dtype=torch.double), nz, padding=1).max()) <= 1.0
    return w


def pattern_p_dgrad(cout, cin, k, gen):
    """weights [cout][cin][3][3] with one non-zero per INPUT channel, at flat (co, tap) index (ci * STRIDE + k) mod (9 cout)"""
    w = torch.zeros(cin, cout * 9)
    idx = torch.tensor(pattern_p_index(cin, cout, k))
    w[torch.arange(cin), idx] = full_mantissa((cin,), gen)
    w = w.view(cin, cout, 3, 3).transpose(0, 1).contiguous()
    nz = (w != 0).double()
    assert float(F.conv_transpose2d(torch.ones(1, cout, 5, 5, dtype=torch.double), nz, padding=1).max()) <= 1.0
    return w


def pattern_p_family(cout, cin, gen, kind="forward"):
    """the whole Latin-square family [K][cout][cin][3][3]; asserts that it visits every (co, ci, tap) triple exactly once"""
    n = 9 * (cin if kind == "forward" else cout)
    mk = pattern_p_forward if kind == "forward" else pattern_p_dgrad
    fam = torch.stack([mk(cout, cin, k, gen) for k in range(n)])
    assert_covers_every_triple(fam)
    return fam


def assert_covers_every_triple(fam):
    visits = (fam != 0).sum(0)
    assert bool((visits == 1).all()), "pattern P family: a (co, ci, tap) triple is visited %d..%d times" % (int(visits.min()), int(visits.max()))


def pattern_p_convt(c, k, gen, one_hot=False):
    """ConvTranspose2d(2, stride 2) weights [ci][co][2][2] with one non-zero over ci per (co, sub-pixel): ci = ((co * 4 + sub) * STRIDE
    + k) mod c; c launches visit every (ci, co, sub-pixel).  one_hot: signed +-1.0 instead of full-mantissa values."""
    w = torch.zeros(c, c * 4)
    col = torch.arange(c * 4)
    ci = (col * STRIDE + k) % c
    if one_hot:
        val = torch.where(torch.rand(c * 4, generator=gen) < 0.5, -1.0, 1.0)
    else:
        val = full_mantissa((c * 4,), gen)
    w[ci, col] = val
    return w.view(c, c, 2, 2)


# ---- pattern S --------------------------------------------------------------------------------------------------------------------------

def required_positions(H, W, row_seams=(4, 16), col_seams=(32,)):
    """(y, x) every pattern-S family must visit: the four corners, both sides of every listed tile / strip seam inside the image (seam
    s: rows / columns s - 1 | s), the last row and column (of a ragged last tile), and every crossing of those rows and columns.
    Defaults: the 3x3 kernels' 32 x 16 output tile and 4-row strips."""
    rows = {0, H - 1}
    for s in row_seams:
        if 0 < s < H:
            rows |= {s - 1, s}
    cols = {0, W - 1}
    for s in col_seams:
        if 0 < s < W:
            cols |= {s - 1, s}
    return sorted(itertools.product(sorted(rows), sorted(cols)))


def _far(p, q):
    return p[0] != q[0] or max(abs(p[1] - q[1]), abs(p[2] - q[2])) >= SPACING


def pattern_s_groups(B, H, W, n_chan, required):
    """Partition of the required (y, x) into groups of exactly n_chan positions (b, y, x), pairwise >= SPACING apart inside an image;
    groups are filled up with further positions from the interior.  Returns the list of groups."""
    groups = []
    for (y, x) in required:
        placed = False
        for grp in groups:
            if len(grp) >= n_chan:
                continue
            for b in range(B):
                if all(_far((b, y, x), q) for q in grp):
                    grp.append((b, y, x))
                    placed = True
                    break
            if placed:
                break
        if not placed:
            groups.append([(0, y, x)])
    for grp in groups:
        cand = ((b, y, x) for y in range(1, H, 2) for x in range(1, W, 2) for b in range(B))
        while len(grp) < n_chan:
            p = next(cand)          # StopIteration = the geometry is too small for n_chan spaced positions
            if all(_far(p, q) for q in grp):
                grp.append(p)
    assert_pattern_s(groups, B, H, W, n_chan, required)
    return groups


def assert_pattern_s(groups, B, H, W, n_chan, required):
    seen = set()
    for grp in groups:
        assert len(grp) == n_chan and len(set(grp)) == n_chan
        for p, q in itertools.combinations(grp, 2):
            assert _far(p, q), (p, q)
        for (b, y, x) in grp:
            assert 0 <= b < B and 0 <= y < H and 0 <= x < W
            seen.add((y, x))
    missing = [p for p in required if p not in seen]
    assert not missing, "pattern S misses required positions %s" % missing


def pattern_s_gradients(B, H, W, n_chan, groups, gen):
    """one gradient tensor [B][n_chan][H][W] per (group, rotation): channel c sits on position (c + rot) mod n_chan of the group, so
    over a group's n_chan launches every channel visits every position.  Returns (g [L][B][n_chan][H][W], placements: per launch the
    list of (c, b, y, x))."""
    gs, places = [], []
    for grp in groups:
        for rot in range(n_chan):
            g = torch.zeros(B, n_chan, H, W)
            val = full_mantissa((n_chan,), gen, scale=1.0)
            pl = []
            for c in range(n_chan):
                b, y, x = grp[(c + rot) % n_chan]
                g[b, c, y, x] = val[c]
                pl.append((c, b, y, x))
            gs.append(g)
            places.append(pl)
    g = torch.stack(gs)
    per_chan = (g != 0).flatten(3).sum(3).sum(1)                    # [L][n_chan]
    assert bool((per_chan == 1).all())
    return g, places


def visited(places):
    """{channel: set of (y, x)} over the launches of a family"""
    out = {}
    for pl in places:
        for (c, b, y, x) in pl:
            out.setdefault(c, set()).add((y, x))
    return out


def assert_every_channel_visits(places, required, n_chan):
    v = visited(places)
    for c in range(n_chan):
        missing = [p for p in required if p not in v.get(c, ())]
        assert not missing, "channel %d never sits on %s" % (c, missing)


# ---- references (torch float64 on the CPU) ----------------------------------------------------------------------------------------------

def ref_conv_fwd(x, w, scale=None, bias=None, relu=False):
    y = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=1)
    if scale is not None:
        y = y * scale.double().view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


def ref_conv_bwd(x, w, g, want_x=True):
    """(gx, dw, db) of conv3x3 pad 1 by autograd in float64"""
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = torch.zeros(w.shape[0], dtype=torch.double, requires_grad=True)
    F.conv2d(xd, wd, bd, padding=1).backward(g.double())
    return xd.grad, wd.grad, bd.grad


def ref_convt_bwd(x, w, g):
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    bd = torch.zeros(w.shape[1], dtype=torch.double, requires_grad=True)
    F.conv_transpose2d(xd, wd, bd, stride=2).backward(g.double())
    return xd.grad, wd.grad, bd.grad


def products_per_output_fwd(x, w):
    """number of non-zero products behind every output element of conv3x3 pad 1"""
    return F.conv2d((x != 0).double(), (w != 0).double(), padding=1)


def products_per_output_dgrad(g, w):
    return F.conv_transpose2d((g != 0).double(), (w != 0).double(), padding=1)


def products_per_output_wgrad(x, g):
    """number of non-zero products behind every dw element [co][ci][3][3]"""
    xn, gn = (x != 0).double(), (g != 0).double()
    wd = torch.zeros(g.shape[1], x.shape[1], 3, 3, dtype=torch.double, requires_grad=True)
    F.conv2d(xn, wd, padding=1).backward(gn)
    return wd.grad


# ---- the check --------------------------------------------------------------------------------------------------------------------------

class Result:
    """outcome of ``check``: ok, n (checked elements with a non-zero reference), beyond (of them outside the bar), share = beyond / n,
    worst (largest |got - ref| / |ref|), differing (elements that are not float32(ref64): the split form's witness), zeros_wrong
    (elements that had to be +-0 and are not), first (index of the worst offender)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return ("single-product check [%s]: %d elements, %d beyond the bar (%.2f %%), worst %.3g = 2^%.2f of the element, %d differ from "
                "float32(ref), %d non-zero where the reference is 0, worst at %s" %
                (self.form, self.n, self.beyond, 100.0 * self.share, self.worst, torch.log2(torch.tensor(max(self.worst, 1e-300))).item(),
                 self.differing, self.zeros_wrong, self.first))


def check(got, ref64, form, prev=None, where=None):
    """got: fp32 result; ref64: the exact float64 reference of the product part; prev: the previous contents of a += output (got is
    then compared with prev + ref64); where: optional bool mask of the elements that are single-product (others are ignored)."""
    assert form in BAR and ref64.dtype == torch.float64 and got.shape == ref64.shape
    got64 = got.detach().cpu().double()
    sel = torch.ones_like(ref64, dtype=torch.bool) if where is None else where
    if prev is None:
        want = ref64
        tol = BAR[form] * ref64.abs()
    else:
        want = prev.double() + ref64
        tol = BAR[form] * ref64.abs() + 2.0 ** -24 * want.abs()
    err = (got64 - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    nz = sel & (ref64 != 0)
    zero = sel & (ref64 == 0)
    if prev is None:
        zeros_wrong = int((zero & (got64 != 0)).sum())          # (NaN != 0 is True: an unwritten element counts)
    else:
        zeros_wrong = int((zero & (got64 != prev.double())).sum())
    bad = nz & (err > tol)
    n = int(nz.sum())
    # the error of the product part in units of the element: with ``prev`` the rounding of the sum (<= 2^-24 |prev + ref|) is taken off first
    perr = err if prev is None else (err - 2.0 ** -24 * want.abs()).clamp_min(0.0)
    rel = torch.where(nz, perr / ref64.abs().clamp_min(1e-300), torch.zeros_like(err))
    worst = float(rel.max()) if n else 0.0
    first = tuple(int(i) for i in torch.unravel_index(rel.argmax(), rel.shape)) if n else None
    differing = int((nz & (got64 != want.float().double())).sum())
    beyond = int(bad.sum())
    return Result(ok=(beyond == 0 and zeros_wrong == 0), form=form, n=n, beyond=beyond, share=beyond / max(n, 1), worst=worst,
                  differing=differing, zeros_wrong=zeros_wrong, first=first)


def assert_single_product(got, ref64, form, prev=None, where=None, what=""):
    r = check(got, ref64, form, prev=prev, where=where)
    print(what, r)
    assert r.ok, "%s: %r" % (what, r)
    return r


def assert_form_witness(results, what=""):
    """split-form launches with >= 1024 checked products in all: at least one element differs from float32(ref64)"""
    n = sum(r.n for r in results)
    d = sum(r.differing for r in results)
    if n >= 1024:
        assert d > 0, "%s: %d products, every one equals the rounded fp32 product: the split-form kernel did not run" % (what, n)
    return n, d


# ---- fp32 emulation of the split form (CPU tests) ---------------------------------------------------------------------------------------

def split3(x):
    """common.h: pc_split3 -- x == a0 + a1 + a2 exactly, each a bf16 number"""
    a0 = x.to(torch.bfloat16).float()
    r1 = x - a0
    a1 = r1.to(torch.bfloat16).float()
    a2 = r1 - a1
    return a0, a1, a2


SPLIT_TERMS = [(2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)]        # common.h: pc_split_product_at, (weight plane, pixel plane), smallest first


def split_product(a, b, order=None, drop=None, double=None, lose_third_of=None):
    """fp32 emulation of the six-term sum of the split form, accumulated in fp32 in ``order`` (default: the kernels' own, smallest
    first).  Planted defects: drop = a term left out, double = a term added twice, lose_third_of = "a" / "b": that operand's third piece 0."""
    A, Bp = list(split3(a)), list(split3(b))
    if lose_third_of == "a":
        A[2] = torch.zeros_like(a)
    if lose_third_of == "b":
        Bp[2] = torch.zeros_like(b)
    acc = torch.zeros_like(a)
    for t in (order or SPLIT_TERMS):
        if t == drop:
            continue
        p = A[t[0]] * Bp[t[1]]                  # exact in fp32: 8 x 8 mantissa bits
        acc = acc + p
        if t == double:
            acc = acc + p
    return acc
