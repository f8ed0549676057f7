"""tests/single_product.py checked without a GPU: the builders keep their promises (coverage, one product per output, spacing,
required positions), the two bars hold for the honest arithmetic and reject every planted arithmetic defect with a wide margin, and
planted index defects (float64 torch functions written here, never device code) are rejected under both patterns."""
import pytest
import torch
import torch.nn.functional as F

from tests import single_product as SP

N = 1_000_000


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture(scope="module")
def products():
    """10^6 products x ~ N(0, 1), w ~ 0.2 N(0, 1) (|w| >= 2^-6), and their exact float64 values"""
    g = _gen(11)
    x = torch.randn(N, generator=g)
    w = SP.full_mantissa((N,), g)
    return x, w, x.double() * w.double()


# ---- builders ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,cout", [(8, 8), (8, 16), (16, 16), (16, 8), (2, 8), (4, 8), (32, 8)])
@pytest.mark.parametrize("kind", ["forward", "dgrad"])
def test_pattern_p_covers_every_triple_once_with_one_product_per_output(cin, cout, kind):
    fam = SP.pattern_p_family(cout, cin, _gen(1), kind)          # (asserts the coverage itself)
    assert fam.shape[0] == 9 * (cin if kind == "forward" else cout)
    assert int((fam != 0).sum()) == 9 * cin * cout
    per = (fam != 0).flatten(2).sum(2) if kind == "forward" else (fam != 0).transpose(1, 2).flatten(2).sum(2)
    assert bool((per == 1).all())                                # one non-zero per output (input) channel in every launch
    assert bool((fam[fam != 0].abs() >= SP.W_MIN).all())
    x = torch.randn(1, cin if kind == "forward" else cout, 6, 7, generator=_gen(2))
    for k in (0, fam.shape[0] // 2, fam.shape[0] - 1):
        cnt = SP.products_per_output_fwd(x, fam[k]) if kind == "forward" else SP.products_per_output_dgrad(x, fam[k])
        assert float(cnt.max()) <= 1.0


@pytest.mark.parametrize("c", [8, 16])
def test_pattern_p_transposed_conv_covers_every_weight(c):
    fam = torch.stack([SP.pattern_p_convt(c, k, _gen(3)) for k in range(c)])
    assert bool(((fam != 0).sum(0) == 1).all())
    assert bool(((fam != 0).sum(1) == 1).all())                  # one input channel per (co, sub-pixel): one product per output
    hot = SP.pattern_p_convt(c, 1, _gen(4), one_hot=True)
    assert bool(((hot.abs() == 1.0) | (hot == 0)).all()) and bool(((hot != 0).sum(0) == 1).all())


# every (geometry, seams, gradient channels) tests/test_gpu_single_product.py builds pattern S for
_CONV = ((4, 16, 32), (32, 64))          # 3x3 kernels: 4-row strips, 32 x 16 output tiles
_CONVT = ((2, 8), (32,))                 # transposed conv, on the (2H, 2W) gradient
_UP = ((8, 16), (128,))                  # composed Up backward: blocks of 4 low-resolution rows, 128-column tiles
GEOMS = [(hw, *_CONV, c) for hw in [(20, 36), (36, 68), (19, 35)] for c in (8, 16)] + [((23, 35), *_CONV, 8), ((58, 69), *_CONV, 8)] + \
        [(hw, *_CONVT, c) for hw in [(18, 42), (32, 64)] for c in (8, 16)] + \
        [(hw, *_UP, 8) for hw in [(12, 16), (20, 72), (24, 136), (16, 64), (20, 136)]] + [((32, 32), (4, 16), (16,), 16)]


@pytest.mark.parametrize("hw,row_seams,col_seams,n_chan", GEOMS)
def test_pattern_s_spacing_positions_and_rotation(hw, row_seams, col_seams, n_chan):
    H, W = hw
    req = SP.required_positions(H, W, row_seams, col_seams)
    for p in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        assert p in req
    for s in row_seams:
        if s < H:
            assert any(y == s - 1 for y, _ in req) and any(y == s for y, _ in req)
    for s in col_seams:
        if s < W:
            assert any(x == s - 1 for _, x in req) and any(x == s for _, x in req)
    groups = SP.pattern_s_groups(2, H, W, n_chan, req)           # (asserts spacing and the required positions itself)
    g, places = SP.pattern_s_gradients(2, H, W, n_chan, groups, _gen(5))
    assert g.shape[0] == len(groups) * n_chan
    SP.assert_every_channel_visits(places, req, n_chan)
    # at most one product behind every data-gradient element, exactly one behind every weight-gradient element that touches the image
    w = torch.ones(n_chan, 8, 3, 3)
    x = torch.ones(2, 8, H, W)
    for l in (0, g.shape[0] - 1):
        assert float(SP.products_per_output_dgrad(g[l], w).max()) <= 1.0
        assert float(SP.products_per_output_wgrad(x, g[l]).max()) <= 1.0


def test_pow2_bn_scales_are_exact_and_distinct():
    for c in (8, 16):
        gamma, beta, mean, var, eps, scale = SP.bn_pow2(c)
        fold = gamma * (1.0 / torch.sqrt(var + eps))             # common.h: pc_bn_fold
        assert torch.equal(fold, scale) and len(set(scale.tolist())) == c
        assert bool((torch.frexp(scale)[0] == 0.5).all())        # powers of two


# ---- the bars hold for the honest arithmetic --------------------------------------------------------------------------------------------

ORDERS = [SP.SPLIT_TERMS, SP.SPLIT_TERMS[::-1], [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)], [(1, 1), (0, 0), (2, 0), (0, 1), (0, 2), (1, 0)]]


def test_the_split_bar_holds_for_the_six_term_sum_in_every_order(products):
    x, w, exact = products
    worst = 0.0
    for order in ORDERS:
        r = SP.check(SP.split_product(w, x, order), exact, "split")
        assert r.ok and r.n == N, r
        worst = max(worst, r.worst)
        # the form witness: the six-term sum is not the rounded product in a sizeable share of the elements (4.2 % in the kernels'
        # smallest-first order, more in the others): with a share p >= 1 % a launch of 1024 products shows none with (1 - p)^1024 < 4e-5
        print("differing from float32(ref):", r.differing / N)
        assert r.differing >= 0.01 * N, r
    print("six-term sum, worst |err| / |ab| over four orders: 2^%.2f" % torch.log2(torch.tensor(worst)).item())
    assert worst <= 2.0 ** -21


def test_the_fp32_bar_holds_for_the_fp32_product_with_no_differing_element(products):
    x, w, exact = products
    r = SP.check(x * w, exact, "fp32mfma")
    assert r.ok and r.differing == 0 and r.n == N, r
    acc = torch.randn(N, generator=_gen(12))
    r = SP.check(acc + (x.double() * w.double()).float(), exact, "fp32mfma", prev=acc)       # += form: one more rounding of the sum
    assert r.ok, r
    r = SP.check(acc + SP.split_product(w, x), exact, "split", prev=acc)
    assert r.ok, r


def test_zero_reference_demands_zero_and_nan_never_passes():
    ref = torch.tensor([0.0, 0.0, 1.5, 0.0], dtype=torch.double)
    assert SP.check(torch.tensor([0.0, -0.0, 1.5, 0.0]), ref, "fp32mfma").ok
    assert SP.check(torch.tensor([0.0, 1e-30, 1.5, 0.0]), ref, "fp32mfma").zeros_wrong == 1
    assert not SP.check(torch.tensor([0.0, float("nan"), 1.5, 0.0]), ref, "split").ok
    assert not SP.check(torch.tensor([0.0, 0.0, float("nan"), 0.0]), ref, "split").ok
    prev = torch.tensor([1.0, 2.0, 3.0, 4.0])
    assert SP.check(torch.tensor([1.0, 2.0, 4.5, 4.0]), ref, "split", prev=prev).ok
    assert not SP.check(torch.tensor([1.0, 2.0, 4.5, 0.0]), ref, "split", prev=prev).ok


# ---- the bars have teeth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("term", SP.SPLIT_TERMS)
@pytest.mark.parametrize("defect", ["drop", "double"])
def test_a_lost_or_doubled_partial_product_is_rejected(products, term, defect):
    x, w, exact = products
    r = SP.check(SP.split_product(w, x, **{defect: term}), exact, "split")
    print(defect, term, r)
    assert not r.ok and r.share >= 0.25, r


@pytest.mark.parametrize("operand", ["a", "b"])
def test_a_lost_third_piece_is_rejected(products, operand):
    x, w, exact = products
    r = SP.check(SP.split_product(w, x, lose_third_of=operand), exact, "split")
    print(operand, r)
    assert not r.ok and r.share >= 0.25, r


def test_a_doubled_or_halved_fp32_product_is_rejected(products):
    x, w, exact = products
    assert SP.check((x * w) * (1 + 2.0 ** -22), exact, "fp32mfma").share >= 0.25
    assert SP.check((x.bfloat16().float() * w), exact, "fp32mfma").share >= 0.25          # an operand rounded to bf16


# ---- wrong-index defects ----------------------------------------------------------------------------------------------------------------

def _conv_shift_at_last_column(x, w):
    """conv3x3 whose taps at the image's LAST column read one column to the left"""
    y = F.conv2d(x, w, padding=1)
    y_bad = F.conv2d(torch.roll(x, 1, dims=3), w, padding=1)
    y[..., -1] = y_bad[..., -1]
    return y


def _conv_column_32_from_halo(x, w):
    """conv3x3 whose source column 32 holds column 31's value (a tile that reads its first column from the neighbour's halo slot)"""
    xb = x.clone()
    xb[..., 32] = x[..., 31]
    return F.conv2d(xb, w, padding=1)


def _wgrad_of(conv, x, w, g):
    wd = w.clone().requires_grad_(True)
    conv(x, wd).backward(g)
    return wd.grad


@pytest.mark.parametrize("defect", [_conv_shift_at_last_column, _conv_column_32_from_halo])
def test_a_wrong_index_is_rejected_under_both_patterns(defect):
    B, C, H, W = 2, 8, 20, 36
    x = torch.randn(B, C, H, W, generator=_gen(21)).double()
    honest = lambda a, b: F.conv2d(a, b, padding=1)
    # pattern P, forward: some launch of the family puts a tap where the defect acts
    fam = SP.pattern_p_family(C, C, _gen(22), "forward").double()
    caught = 0
    for k in range(fam.shape[0]):
        ref = honest(x, fam[k])
        assert SP.check(ref.float(), ref, "fp32mfma").ok
        caught += not SP.check(defect(x, fam[k]).float(), ref, "fp32mfma").ok
    assert caught >= fam.shape[0] // 3, caught
    # pattern S, weight gradient: the launches that sit next to the defect's column reject it
    req = SP.required_positions(H, W)
    g, places = SP.pattern_s_gradients(B, H, W, C, SP.pattern_s_groups(B, H, W, C, req), _gen(23))
    w = SP.full_mantissa((C, C, 3, 3), _gen(24)).double()
    caught = 0
    for l in range(g.shape[0]):
        ref = _wgrad_of(honest, x, w, g[l].double())
        assert SP.check(ref.float(), ref, "fp32mfma").ok
        caught += not SP.check(_wgrad_of(defect, x, w, g[l].double()).float(), ref, "fp32mfma").ok
    assert caught >= 1, caught


def _up_bias_table(bt, w_up, H, W, missing=None):
    """the composed Up block's bias term: the transposed conv's bias bt seen through the IN-IMAGE taps of the 3x3 conv over the
    up-sampled half (w_up [co][c][3][3]); missing = (co, dy, dx): that border tap is left out of the table"""
    ones = bt.view(1, -1, 1, 1).expand(1, bt.numel(), H, W)
    y = F.conv2d(ones, w_up, padding=1)
    if missing is not None:
        co, dy, dx = missing
        one = torch.zeros_like(w_up)
        one[co, :, dy, dx] = w_up[co, :, dy, dx]
        part = F.conv2d(ones, one, padding=1)
        edge = torch.zeros(1, 1, H, W, dtype=torch.bool)
        edge[..., 0, :] = edge[..., -1, :] = edge[..., :, 0] = edge[..., :, -1] = True
        y = y - part * edge
    return y


def test_a_missing_border_tap_of_the_composed_bias_table_is_rejected():
    C, H, W = 8, 12, 16
    bt = SP.full_mantissa((C,), _gen(31), scale=1.0).double()
    caught = 0
    for k in range(9 * C):
        w = (SP.pattern_p_forward(8, C, k, _gen(32)) != 0).double()            # one tap of 1.0 per output channel
        ref = _up_bias_table(bt, w, H, W)
        assert SP.check(ref.float(), ref, "fp32mfma").ok
        co = 3
        ci, tap = divmod(SP.pattern_p_index(8, C, k)[co], 9)
        bad = _up_bias_table(bt, w, H, W, missing=(co, tap // 3, tap % 3))
        caught += not SP.check(bad.float(), ref, "fp32mfma").ok
    assert caught == 9 * C                     # every launch sees its own channel's tap missing on the border ring
