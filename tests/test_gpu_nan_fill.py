"""Device NaN fill (csrc/nan_fill.hip, ops.nan_fill_) against the brute-force oracle (tests/nanfill_oracle.py, bit-exact) and the reference's
interpolate_nan (fixture g13: exact at unique-nearest sites, in the tie set elsewhere); the orbit decision of data/nanfill.py; the raw
evaluation path and the trainer's --nan_fill."""
import os

import numpy as np
import pytest
import torch

from tests import nanfill_oracle as NO

pytestmark = pytest.mark.gpu
G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_nan_fill.npz")


def _bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def _holey(rng, shape, p=0.3, discs=0, scale=1.0):
    a = (rng.normal(size=shape) * scale).astype(np.float32)
    a[rng.random(shape) < p] = np.nan
    C, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(discs):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1, max(2, min(h, w) / 4))
        a[:, (yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = np.nan
    return a


def _fill_dev(a, hw=None):
    from popcorn_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cnt = ops.nan_fill_(x, hw)
    torch.cuda.synchronize()
    return x.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("shape,p,discs", [((1, 1, 1), 1.0, 0), ((1, 1, 1), 0.0, 0), ((4, 37, 53), 0.3, 3), ((2, 129, 257), 0.05, 6),
                                           ((4, 37, 53), 0.97, 0), ((3, 1, 300), 0.5, 0), ((4, 300, 1), 0.5, 0), ((6, 20, 30), 0.6, 2),
                                           ((8, 17, 19), 0.9, 0), ((4, 64, 1100), 0.02, 8)])
def test_op_vs_oracle_bit_exact(shape, p, discs):
    rng = np.random.default_rng(hash((shape, p)) % 2 ** 32)
    a = _holey(rng, shape, p, discs)
    got, cnt = _fill_dev(a)
    ref = NO.nan_fill(a)
    assert np.array_equal(_bits(got), _bits(ref))
    n = int(np.isnan(a).sum())
    assert cnt.tolist() == [n, a.size - n]
    again, _ = _fill_dev(a)
    assert np.array_equal(_bits(again), _bits(got))                   # deterministic


def test_op_ties_and_inf():
    """Few distinct values (ties everywhere, unique values reveal the source), +-Inf known, a fully NaN plane and row."""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 3, (4, 45, 61)).astype(np.float32)
    a[rng.random(a.shape) < 0.5] = np.nan
    a[2] = np.nan
    a[:, 17, :] = np.nan
    m = ~np.isnan(a)
    a[m] = np.arange(m.sum(), dtype=np.float32)
    a[0, 0, 5], a[1, 30, 30] = np.inf, -np.inf
    got, _ = _fill_dev(a)
    assert np.array_equal(_bits(got), _bits(NO.nan_fill(a)))
    assert np.isinf(got).sum() >= 2


def test_op_fixture_patterns_vs_oracle_and_reference():
    from tests.test_nan_fill_cpu import check_against_reference
    g = np.load(G13)
    for case in ("clouds", "scattered_one_channel", "row_col", "s1_plane", "tie_free", "few_known", "nan_free"):
        inp, ref = g[f"{case}/input"], g[f"{case}/output"]
        got, _ = _fill_dev(inp)
        assert np.array_equal(_bits(got), _bits(NO.nan_fill(inp))), case
        if case in ("tie_free", "few_known", "nan_free"):
            assert np.array_equal(_bits(got), _bits(ref)), case
        else:
            check_against_reference(inp, ref, got)


def test_batched_ragged_extents():
    """(B, C, H, W) with per-sample extents: each extent filled on its own, padding untouched and never a source -- sample 1 is built
    so that ignoring its extent would pick a padding zero (its NaNs sit on the extent's edge, the padding one column away, the nearest
    in-extent known entry farther)."""
    rng = np.random.default_rng(8)
    B, C, H, W = 3, 4, 40, 50
    x = (rng.normal(size=(B, C, H, W)) + 5).astype(np.float32)
    hw = [(40, 50), (25, 31), (13, 7)]
    for b, (h, w) in enumerate(hw):
        x[b, :, h:, :] = 0.0
        x[b, :, :h, w:] = 0.0
        x[b, :, :h, :w][rng.random((C, h, w)) < 0.25] = np.nan
    x[1, :, 5:20, 25:31] = np.nan                       # the right edge of sample 1's extent: padding at column 31
    x[2, :, 3:, 4:] = np.nan
    x[0, :, :, 45:] = np.nan                            # full extent: the tensor's own border
    x_dev = torch.from_numpy(x).cuda()
    from popcorn_amd import ops
    for hw_arg in (hw, torch.tensor(hw, dtype=torch.int32).cuda()):
        t = x_dev.clone()
        cnt = ops.nan_fill_(t, hw_arg).cpu().numpy()
        got = t.cpu().numpy()
        ref = NO.nan_fill_batch(x, hw)
        assert np.array_equal(_bits(got), _bits(ref))
        for b, (h, w) in enumerate(hw):
            n = int(np.isnan(x[b, :, :h, :w]).sum())
            assert cnt[b].tolist() == [n, C * h * w - n]
            assert not np.isnan(got[b, :, :h, :w]).any()
    # the extent matters: the padding zero at column 31 is the unique nearest entry of the targets in rows 6 - 18 of column 30
    wrong = NO.nan_fill(x[1])
    assert not np.array_equal(_bits(wrong[:, :25, :31]), _bits(got[1, :, :25, :31]))
    assert (wrong[:, 6:19, 30] == 0).all() and (got[1, :, 6:19, 30] != 0).all()


def test_op_rejects_cpu_and_bad_input():
    from popcorn_amd import ops
    from popcorn_amd._lib import PopcornHipError
    with pytest.raises(PopcornHipError):
        ops.nan_fill_(torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        ops.nan_fill_(torch.zeros(2, 4, 4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        ops.nan_fill_(torch.zeros(1, 2, 4, 4, device="cuda"), [(5, 4)])


def test_large_window_sampled_sites():
    """One 4 x 2048 x 2048 cloud window: a few thousand sampled NaN sites against the growing-box oracle (exact), every NaN filled,
    known entries unchanged."""
    from popcorn_amd.data.dataset import cloud_mask
    g = torch.Generator().manual_seed(21)
    a = (torch.randint(0, 10000, (4, 2048, 2048), generator=g).float()).numpy()
    m = cloud_mask(2048, 2048, 0.05, g).numpy()
    a[:, m] = np.nan
    a[1][np.random.default_rng(2).random((2048, 2048)) < 0.01] = np.nan
    got, cnt = _fill_dev(a)
    nan = np.isnan(a)
    assert cnt.tolist() == [int(nan.sum()), int((~nan).sum())]
    assert not np.isnan(got).any()
    assert np.array_equal(_bits(got[~nan]), _bits(a[~nan]))
    sites = np.argwhere(nan)
    pick = sites[np.random.default_rng(4).choice(len(sites), 3000, replace=False)]
    for s in pick:
        assert _bits(np.float32(NO.nearest_value_box(a, s))) == _bits(got[tuple(s)]), s


def test_decision_logic_of_fill_item():
    from popcorn_amd.data.nanfill import fill_item_
    rng = np.random.default_rng(9)
    s2 = _holey(rng, (4, 40, 50), 0.1)
    desc = rng.normal(size=(2, 40, 50)).astype(np.float32)
    asc = rng.normal(size=(2, 40, 50)).astype(np.float32)
    asc[0, 3, 4] = np.nan
    few = desc.copy()
    few[:, 0, :3] = np.nan                               # 6 / 4000 < 5 %
    many = desc.copy()
    many[:, :2, :] = np.nan                              # 200 / 4000 = 5 %: not < 5 %
    calls = []

    def load():
        calls.append(1)
        return torch.from_numpy(asc).cuda()

    def run(s1, ascfill=False, loader=load):
        t2, t1 = torch.from_numpy(s2).cuda(), torch.from_numpy(s1).cuda()
        orbit = fill_item_(t2, t1, loader, ascfill)
        return orbit, t2.cpu().numpy(), t1.cpu().numpy()

    orbit, o2, o1 = run(desc)
    assert orbit == "desc" and not calls and np.array_equal(_bits(o1), _bits(desc))
    assert np.array_equal(_bits(o2), _bits(NO.nan_fill(s2)))
    orbit, _, o1 = run(few)
    assert orbit == "desc" and not calls and np.array_equal(_bits(o1), _bits(NO.nan_fill(few)))
    orbit, _, o1 = run(many)
    assert orbit == "asc" and len(calls) == 1 and np.array_equal(_bits(o1), _bits(NO.nan_fill(asc)))
    orbit, _, o1 = run(few, ascfill=True)
    assert orbit == "asc" and len(calls) == 2 and np.array_equal(_bits(o1), _bits(NO.nan_fill(asc)))
    holey_asc = asc.copy()
    holey_asc[:, 10:14, :] = np.nan
    with pytest.raises(Exception, match="No data here!"):
        run(many, loader=lambda: torch.from_numpy(holey_asc).cuda())


def _model():
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    return POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval()


def test_evaluate_raster_raw_vs_oracle_filled_hand_loop():
    """evaluate_raster(raw=True) on a clouded raster with orbit gaps == a loop that, per window, fills with the oracle (orbit rule as the
    reference), normalises and feeds the same ensemble path -- bit for bit."""
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.dataset import SyntheticTestRaster
    from popcorn_amd.data.nanfill import asc_fill, s1_orbit
    data = SyntheticTestRaster(600, 700, n_regions=30, seed=77, device="cuda", raw=True, nan_clouds=0.04, s1_gap=0.0)
    data.s1[:, :, 100:120] = float("nan")               # 20 / 256 rows of the first window row: over 5 %, the ascending orbit
    data.s1[:, :, 500:505] = float("nan")               # 5 / 256 rows of the last one: filled
    m = _model()
    ps, ov = 256, 32
    got = E.evaluate_raster([m], data.raster, ps, ov, raw=True)
    orbits = []

    def hand(x, y, s, p):
        win = data(x, y, s, p)
        s2 = NO.nan_fill_offsets(win["S2"][0].cpu().numpy())
        s1 = win["S1"][0].cpu().numpy()
        orbit, fill = s1_orbit(int(np.isnan(s1).sum()), s1.size, False)
        if orbit == "asc":
            s1 = win["S1_asc"]()[0].cpu().numpy()
            fill = asc_fill(int(np.isnan(s1).sum()), s1.size)
        if fill:
            s1 = NO.nan_fill_offsets(s1)
        orbits.append(orbit)
        raw = torch.from_numpy(np.concatenate([s2, s1])[None]).cuda()
        return ops.select_normalize(raw, tuple(range(6)), stats.MEAN6, stats.STD6)

    ref = E.evaluate_raster([m], _Callable(hand, data.shape), ps, ov)
    assert "asc" in orbits and "desc" in orbits
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


class _Callable:
    def __init__(self, fn, shape):
        self.fn, self.shape = fn, shape

    def __call__(self, *a):
        return self.fn(*a)


def test_evaluate_raster_raw_without_nan_equals_normalised_path():
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from popcorn_amd.data.dataset import SyntheticTestRaster
    data = SyntheticTestRaster(400, 450, n_regions=20, seed=78, device="cuda", raw=True)
    m = _model()
    got = E.evaluate_raster([m], data.raster, 256, 32, raw=True)
    norm = ops.select_normalize(torch.cat([data.s2, data.s1], 1).contiguous(), tuple(range(6)), stats.MEAN6, stats.STD6)
    ref = E.evaluate_raster([m], norm, 256, 32)
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)


# ---- training ------------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, extra=""):
    from popcorn_amd.cli import Trainer, train_parser
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -lr 1e-4 --synthetic_regions 4 -wb 2 "
            f"--save_dir {tmp_path} -lt 100 -val 100 -e 1 --save-model no " + extra).split()
    return Trainer(train_parser().parse_args(argv))


def _batch(nan_clouds):
    """A B = 2 ragged batch of NaN-clouded regions, and the same batch with every item pre-filled by the oracle."""
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.dataset import SyntheticWeaksupDataset
    ds = SyntheticWeaksupDataset(4, min_hw=70, max_hw=130, seed=41, nan_clouds=nan_clouds)
    items = [ds[0], ds[1]]
    assert items[0]["S2"].shape != items[1]["S2"].shape
    filled = []
    for it in items:
        f = dict(it)
        f["S2"] = torch.from_numpy(NO.nan_fill(it["S2"].numpy()))
        f["S1"] = torch.from_numpy(NO.nan_fill(it["S1"].numpy()))
        filled.append(f)
    return Population_Dataset_collate_fn(items), Population_Dataset_collate_fn(filled)


def _to_dev(sample):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in sample.items()}


def _step(t, sample):
    from popcorn_amd.cli import seed_all
    seed_all(99)                                        # the augmentation coins / factors and the selection grid of this step
    loss = t.train_step(sample)
    torch.cuda.synchronize()
    return loss.cpu(), {n: g.detach().cpu().clone() for n, g in t.fused.grads.items()}, t.fused.flat_p.cpu().clone()


def _close(r1, r2):
    """Two steps from a restored trainer state on bit-equal inputs (checked separately, before): a step repeated from a restored state
    is not bit-reproducible (measured: losses 1.7e-4 apart on the normalize_sample path), so this is a sanity bound around that spread --
    a step on unfilled NaNs (ReLU turns them into 0) misses it by far."""
    torch.testing.assert_close(r1[0], r2[0], rtol=2e-3, atol=0)
    assert len(r1[1]) == 56 and r1[1].keys() == r2[1].keys()
    for n in r1[1]:
        torch.testing.assert_close(r1[1][n], r2[1][n], rtol=0, atol=5e-2 * max(r2[1][n].abs().max().item(), 1e-3))
    torch.testing.assert_close(r1[2], r2[2], rtol=0, atol=1e-4)


def _restorer(t):
    """Puts the trainer back to its state at this call (parameters, BN buffers, Adam moments and step counters)."""
    sd = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    opt = t.fused.optimizer_state()

    def restore():
        t.model.load_state_dict(sd)
        t.fused.sync_from_model()
        t.fused.load_optimizer_state(opt)
    return restore


def _prepared(sample, fused, nan_fill):
    """What the trainer's step consumes for ``sample`` (train_step's preparation, augmentation draws seeded)."""
    from popcorn_amd.cli import normalize_sample, prepare_sample_fused, seed_all
    from popcorn_amd.utils.transform import default_train_transform
    seed_all(99)
    if fused:
        return prepare_sample_fused(_to_dev(sample), default_train_transform(), nan_fill=nan_fill)
    return normalize_sample(sample, torch.device("cuda"), default_train_transform(), nan_fill=nan_fill)


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_nan_fill_equals_oracle_prefilled(tmp_path, fused):
    """--nan_fill on a ragged B = 2 NaN batch: what the step consumes (the fused path's raw tile as the feed stages it, or the normalised
    input of normalize_sample) is bit-equal to the same preparation of items the oracle filled; one trainer step from the same state on
    each gives the same loss, 56 gradients and parameters after Adam (to the step's own run-to-run spread)."""
    raw, pre = _batch(0.05)
    assert torch.isnan(raw["S2"]).any() and not torch.isnan(pre["S2"]).any()
    a, b = _prepared(raw, fused, True), _prepared(pre, fused, False)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    conv = _to_dev if fused else (lambda s: s)
    t = _trainer(tmp_path, "--nan_fill")
    restore = _restorer(t)
    r1 = _step(t, conv(raw))
    restore()
    r2 = _step(t, conv(pre))
    assert torch.isfinite(r1[0]).all() and torch.isfinite(r1[2]).all()
    _close(r1, r2)


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_nan_fill_on_nan_free_data_is_a_no_op(fused):
    raw, _ = _batch(0.0)
    assert not torch.isnan(raw["S2"]).any()
    a, b = _prepared(raw, fused, True), _prepared(raw, fused, False)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_region_feed_carries_data_hw():
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.dataset import SyntheticWeaksupDataset
    from popcorn_amd.data.feed import RegionFeed
    ds = SyntheticWeaksupDataset(4, min_hw=40, max_hw=90, seed=5)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=Population_Dataset_collate_fn)
    n = 0
    for k, (sample, ref) in enumerate(zip(RegionFeed(loader, "cuda"), loader)):
        assert sample["data_hw"].is_cuda and torch.equal(sample["data_hw"].cpu(), ref["data_hw"])
        assert ref["data_hw"].tolist() == [list(ds.hw[2 * k + i]) for i in range(2)]
        n += 1
    assert n == 2
