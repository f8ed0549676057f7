"""The census table (csrc/census_table.hip, eval.CensusTable, ops.census_paint, eval.census_detail_maps): every member's census-unit totals
accumulated on the device while the windows are stitched, against the float64 yardstick of tests/census_oracle.py (the reference's loop --
interior ``+=``, divide by the visit count -- followed by float64 unit sums and the mean / (n - 1) standard deviation over members).

Error bars: the module docstring of tests/census_oracle.py (derived, not measured).  Geometry: that of tests/test_gpu_product.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import census_oracle as CO
from tests.test_gpu_product import H, W, PS, OV, M3, MH, MW, MPS, MOV

pytestmark = pytest.mark.gpu
U = CO.U
INT32_MAX = 2 ** 31 - 1


# ---- census levels on the (H, W) raster -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _levels():
    """(boundaries, num_ids): a blocky map as in fixture g9 (25 units, a strip outside every unit, id 26 never occurs); "salt", a new id
    every pixel (no run, no uniform wave); ONE id over the whole raster with patches of -1, num_ids and INT32_MAX that must be ignored."""
    yy, xx = np.mgrid[0:H, 0:W]
    blocky = ((yy // 37) * 5 + xx // 41).astype(np.int32)
    blocky[60:75, :] = -1
    salt = ((yy * W + xx) % 257).astype(np.int32)
    single = np.zeros((H, W), dtype=np.int32)
    single[10:30, 20:50] = -1
    single[70:90, 100:140] = 1
    single[120:140, 5:60] = INT32_MAX
    return [blocky, salt, single], [27, 257, 1]


@functools.lru_cache(maxsize=None)
def _windows(kind, fourseasons, M=M3):
    from popcorn_amd import eval as E
    idx = E.get_patch_indices(H, W, PS, OV, fourseasons)
    g = torch.Generator().manual_seed(13)
    wins = []
    for x, y, s in idx.tolist():
        if kind == "exact":          # multiples of 16 in [0, 240]: every v / visits (visits 1 .. 16) is exact in fp32 and on the 2^-30 grid
            pd = (16 * torch.randint(0, 16, (M, PS, PS), generator=g)).float()
        else:
            pd = torch.rand(M, PS, PS, generator=g)
        wins.append((x, y, pd))
    return idx, wins


@functools.lru_cache(maxsize=None)
def _reference(kind, fourseasons, M=M3):
    b, n = _levels()
    return CO.table_reference(H, W, [(x, y, pd.numpy()) for x, y, pd in _windows(kind, fourseasons, M)[1]], OV, b, n)


def _table(boundaries, num_ids, M=M3, h=H, w=W, visits=None):
    from popcorn_amd import eval as E
    return E.CensusTable(h, w, [torch.from_numpy(b) for b in boundaries], num_ids, M, "cuda", visits=visits)


def _run(kind, fourseasons, M=M3, order=None, finalize=True):
    idx, wins = _windows(kind, fourseasons, M)
    ct = _table(*_levels(), M=M)
    ct.set_windows(idx, PS, OV)
    for i in (order if order is not None else range(len(wins))):
        x, y, pd = wins[i]
        ct.add_window(x, y, pd.cuda(), OV)
    if finalize:
        ct.finalize()
    return ct


# ---- 1. exact geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fourseasons", [False, True])
def test_exact_geometry(fourseasons):
    """No (pixel, member, level) term dropped, duplicated or added to the wrong unit: with inputs whose quotients are exact the totals of
    all three levels, accumulated at once, EQUAL the float64 oracle; so do the visit map and the mean."""
    lv, visits = _reference("exact", fourseasons)
    assert set(np.unique(visits).tolist()) == ({0, 4, 8, 16} if fourseasons else {0, 1, 2, 4})
    ct = _run("exact", fourseasons)
    assert ct.totals.shape == (M3, 27 + 257 + 1) and ct.totals.dtype == torch.float64 and ct.mean.shape == ct.std.shape == (285,)
    assert ct.mean.dtype == ct.std.dtype == torch.float32 and ct.table.dtype == torch.int64
    assert np.array_equal(ct.visits.cpu().numpy(), visits)
    for l, (totals, n_terms) in enumerate(lv):
        got, mean, std = ct.level(l)
        assert np.array_equal(got.cpu().numpy(), totals), l
        rm, rs = CO.members_mean_std(totals)
        assert np.array_equal(mean.cpu().numpy(), rm.astype(np.float32)), l
        np.testing.assert_allclose(std.cpu().numpy(), rs, rtol=2.0 ** -23, atol=0)
    assert not lv[0][0][:, 25:].any() and float(lv[2][0].min()) > 0
    assert torch.equal(ct.table, torch.round(ct.totals * CO.FIX).to(torch.int64))


def test_table_bits_equal_the_arithmetic_restated_in_numpy():
    """The int64 table itself, for random windows and visit counts 4 .. 16: every term is the fp32 quotient put on the 2^-30 grid by
    round-to-nearest-even (tests/census_oracle.fixed_point_total's arithmetic), summed exactly -- so the bits are a function of the
    inputs alone and numpy reproduces them.  Member 0 of the first window holds multiples of 2^-29: where the visit count is 4 the
    quotients are multiples of 2^-31, half of them exact ties of the grid; member 1 holds values up to 2^31 (the integer part)."""
    idx, wins = _windows("rand", True)
    g = torch.Generator().manual_seed(29)
    first = wins[0][2].clone()
    first[0] = torch.randint(0, 2 ** 20, (PS, PS), generator=g).float() * 2.0 ** -29
    first[1] = first[1] * 2.0 ** 31
    wins = [(wins[0][0], wins[0][1], first)] + list(wins[1:])
    visits = _reference("rand", True)[1]
    bs, ns = _levels()
    want = np.zeros((M3, sum(ns)), dtype=np.int64)
    ties = 0
    for x, y, pd in wins:
        x0, x1, y0, y1 = CO.interior(x, y, PS, PS, OV, H, W)
        q = pd.numpy()[:, x0 - x:x1 - x, y0 - y:y1 - y] / visits[x0:x1, y0:y1].astype(np.float32)
        assert q.dtype == np.float32
        scaled = q.astype(np.float64) * CO.FIX
        ties += int((scaled - np.floor(scaled) == 0.5).sum())
        fix = np.rint(scaled).astype(np.int64)
        off = 0
        for b, n in zip(bs, ns):
            ids = b[x0:x1, y0:y1].astype(np.int64)
            ok = (ids >= 0) & (ids < n)
            for m in range(M3):
                np.add.at(want[m], off + ids[ok], fix[m][ok])
            off += n
    assert ties > 100
    ct = _table(bs, ns)
    ct.set_windows(idx, PS, OV)
    for x, y, pd in wins:
        ct.add_window(x, y, pd.cuda(), OV)
    ct.finalize()
    assert np.array_equal(ct.table.cpu().numpy(), want)


# ---- 2. rounding ---------------------------------------------------------------------------------------------------------------------------
def _check_rounding(ct, lv):
    for l, (totals, n_terms) in enumerate(lv):
        got, mean, std = (t.cpu().numpy().astype(np.float64) for t in ct.level(l))
        bars = CO.bar(totals, n_terms)
        err = np.abs(got - totals)
        print(f"level {l} totals: worst |T - T_ref| / bar = {(err / np.maximum(bars, 1e-300)).max():.3f}")
        assert (err <= bars).all(), l
        rm, rs = CO.members_mean_std(totals)
        top = bars.max(0)                                   # the bar at the largest member (the bar grows with T)
        em = np.abs(mean - rm)
        print(f"level {l} mean: worst / bar = {(em / np.maximum(top, 1e-300)).max():.3f}")
        assert (em <= top).all(), l
        es = np.abs(std - rs)
        print(f"level {l} std: worst / bar = {(es / np.maximum(2 * top, 1e-300)).max():.3f}")
        assert (es <= 2 * top).all(), l


@pytest.mark.parametrize("fourseasons", [False, True])
def test_rounding(fourseasons):
    """Uniform random (non-negative) windows: totals within the derived bar of the float64 oracle per (member, unit), the mean within the
    bar of the largest member, the std within twice that (tests/census_oracle.py)."""
    lv, visits = _reference("rand", fourseasons)
    assert int(visits.max()) == (16 if fourseasons else 4)
    _check_rounding(_run("rand", fourseasons), lv)


# ---- 3. order --------------------------------------------------------------------------------------------------------------------------------
def test_any_window_order_and_two_runs_give_the_same_bits():
    n = len(_windows("rand", True)[1])
    a = _run("rand", True)
    b = _run("rand", True)
    assert torch.equal(a.table, b.table) and torch.equal(a.totals, b.totals) and torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std)
    rev = _run("rand", True, order=list(reversed(range(n))))
    shuf = _run("rand", True, order=torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist())
    assert torch.equal(a.table, rev.table) and torch.equal(a.table, shuf.table)
    assert bool((a.table >= 0).all()) and int(a.table.sum()) > 0


# ---- 4. the large-id path, several member passes, several column tiles ------------------------------------------------------------------
def test_large_id_level_and_more_members_than_one_pass():
    """num_ids = 70001 is more than the LDS table holds: the level adds to the global table directly.  9 members take three passes."""
    M = 9
    idx, wins = _windows("exact", False, M)
    yy, xx = np.mgrid[0:H, 0:W]
    big = (((yy // 3) * 7919 + (xx // 5) * 104729) % 70001).astype(np.int32)
    lv, visits = CO.table_reference(H, W, [(x, y, pd.numpy()) for x, y, pd in wins], OV, [big, _levels()[0][0]], [70001, 27])
    ct = _table([big, _levels()[0][0]], [70001, 27], M=M)
    ct.set_windows(idx, PS, OV)
    for x, y, pd in wins:
        ct.add_window(x, y, pd.cuda(), OV)
    ct.finalize()
    for l in (0, 1):
        assert np.array_equal(ct.level(l)[0].cpu().numpy(), lv[l][0]), l
    assert int((lv[0][1] > 0).sum()) > 1000


def test_wide_window_many_tiles_mixed_lds_and_global_levels_shared_visits():
    """ONE window of 70 x 600 (interior 62 x 592: two tile rows, three tile columns, the last one 80 columns wide -- a partial wave and two
    idle ones) whose visit map is handed in (``visits=``); levels of 4700 + 257 ids: the first fills the LDS table, the second does not
    fit beside it and adds to the global table; 5 members: a full pass and a pass of one."""
    h, w, ov, M = 70, 600, 4, 5
    g = torch.Generator().manual_seed(17)
    pd = (16 * torch.randint(0, 16, (M, h, w), generator=g)).float()
    yy, xx = np.mgrid[0:h, 0:w]
    fine = ((yy // 2) * 120 + xx // 5).astype(np.int32)               # 35 x 120 = 4200 units of 2 x 5 pixels
    salt = ((yy * w + xx) % 257).astype(np.int32)
    lv, visits = CO.table_reference(h, w, [(0, 0, pd.numpy())], ov, [fine, salt], [4700, 257])
    vis = torch.zeros(h, w, dtype=torch.int16, device="cuda")
    vis[ov:h - ov, ov:w - ov] = 1
    assert np.array_equal(vis.cpu().numpy(), visits)
    ct = _table([fine, salt], [4700, 257], M=M, h=h, w=w, visits=vis)
    ct.set_windows([(0, 0, 0)], h, ov)
    assert ct.visits is vis and int(vis.sum()) == 62 * 592
    ct.add_window(0, 0, pd.cuda(), ov)
    ct.finalize()
    for l in (0, 1):
        assert np.array_equal(ct.level(l)[0].cpu().numpy(), lv[l][0]), l
    # a window whose interior lies outside the raster adds nothing
    before = ct.table.clone()
    ct.add_window(h, 0, pd.cuda(), ov)
    ct.add_window(0, 0, pd[:, :8, :8].contiguous().cuda(), ov)
    assert torch.equal(ct.table, before)


# ---- 5. flags and arguments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), -1.0, 2.0 ** 33])
def test_a_value_the_table_cannot_take_raises(value):
    from popcorn_amd._lib import PopcornHipError
    idx, wins = _windows("exact", False)
    # member 1 of window 2, a pixel of its interior that no other window visits (so 2^33 stays 2^33) and that lies inside a unit
    x2, y2 = wins[2][0] + OV + 5, wins[2][1] + OV + 7
    assert int(_reference("exact", False)[1][x2, y2]) == 1 and _levels()[0][0][x2, y2] >= 0
    ct = _table(*_levels())
    ct.set_windows(idx, PS, OV)
    for i, (x, y, pd) in enumerate(wins):
        if i == 2:
            pd = pd.clone()
            pd[1, OV + 5, OV + 7] = value
        ct.add_window(x, y, pd.cuda(), OV)
    with pytest.raises(PopcornHipError):
        ct.finalize()
    ct.set_windows(idx, PS, OV)                    # a new accumulation clears the flag
    for x, y, pd in wins:
        ct.add_window(x, y, pd.cuda(), OV)
    ct.finalize()
    assert np.array_equal(ct.level(0)[0].cpu().numpy(), _reference("exact", False)[0][0][0])


def test_single_member_has_zero_std_and_bad_arguments_raise():
    from popcorn_amd import eval as E
    from popcorn_amd._lib import PopcornHipError
    ct = _run("rand", False, M=1)
    assert not bool(ct.std.any()) and torch.equal(ct.mean, ct.totals[0].float())
    b, n = _levels()
    tb = [torch.from_numpy(x) for x in b]
    with pytest.raises(PopcornHipError):
        E.CensusTable(H, W, tb, n, 1, "cpu")
    with pytest.raises(ValueError):
        E.CensusTable(H, W, tb, n, 0, "cuda")
    with pytest.raises(ValueError):
        E.CensusTable(H, W + 1, tb, n, 1, "cuda")
    with pytest.raises(ValueError):
        E.CensusTable(H, W, tb[:1] * 5, [3] * 5, 1, "cuda")
    with pytest.raises(PopcornHipError):
        ct.add_window(0, 0, torch.zeros(1, PS, PS), OV)
    with pytest.raises(ValueError):
        ct.add_window(0, 0, torch.zeros(2, PS, PS, device="cuda"), OV)


# ---- 6. evaluate_raster --------------------------------------------------------------------------------------------------------------------
def _model_level():
    yy, xx = np.mgrid[0:MH, 0:MW]
    b = ((yy // 40) * 6 + xx // 40).astype(np.int32)              # 5 x 6 units
    b[:, 225:] = -1
    return b, 30


def test_evaluate_raster_census_vs_the_stitched_mean_map():
    """evaluate_raster(models, raster, census=ct): the four maps are the bits of the call without it, and the member mean of the unit totals
    agrees with convert_popmap_to_census of the stitched 10 m mean map within (M + 3) * u * T + n_terms * 2^-31."""
    from popcorn_amd import eval as E
    from tests.test_gpu_product import _members, _raster
    ms, raster = _members(), _raster()
    b, n = _model_level()
    ct = _table([b], [n], M=len(ms), h=MH, w=MW)
    maps = E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV, census=ct)
    plain = E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV)
    for a, p in zip(maps, plain):
        assert torch.equal(a.nan_to_num(-1.0), p.nan_to_num(-1.0))
    idx = list(range(n))
    cp, _ = E.convert_popmap_to_census(maps[0], torch.from_numpy(b).cuda(), idx, [0.0] * n)
    n_terms = CO.unit_sums(ct.visits.cpu().numpy(), b, n)
    got = ct.level(0)[0].cpu().numpy().mean(0)
    ref = cp.cpu().numpy().astype(np.float64)
    bars = (len(ms) + 3) * U * ref + n_terms * 2.0 ** -31
    err = np.abs(got - ref)
    print(f"worst |mean_m T_m - T(mean map)| / bar = {(err / np.maximum(bars, 1e-300)).max():.3f}")
    assert float(ref.min()) > 0 and (err <= bars).all()
    pm, ps, members, gt = ct.census(0, idx, [1.0] * n)
    assert members.shape == (len(ms), n) and torch.equal(pm, ct.level(0)[1]) and float(ps.max()) > 0
    with pytest.raises(ValueError):
        E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV, census=_table([b], [n], M=3, h=MH, w=MW))


# ---- 7. the reference's own stitched maps (fixture g12) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_table_mean_vs_the_references_stitched_map_g12(name):
    """The windows of fixture g12 replayed into a CensusTable: the table mean at the census rows against float64 unit sums of the map the
    reference's own Trainer.test_target stitched (run_eval.py:71-203), within (M + 3) * u * T + n_terms * 2^-31."""
    from popcorn_amd import ops
    from popcorn_amd.data import stats
    from tests.g12_case import load_case
    c = load_case(name, lambda raw: ops.select_normalize(raw.cuda(), (0, 1, 2, 3, 4, 5), stats.MEAN6, stats.STD6))
    b = c["ref"]["boundary"].numpy()
    n = int(max(b.max(), max(c["census_idx"]))) + 1
    ct = _table([b], [n], M=c["M"], h=c["h"], w=c["w"])
    ct.set_windows(c["window_list"].tolist(), c["ips"], c["ov"])
    for x, y, pd, sc in c["windows"]:
        ct.add_window(x, y, pd, c["ov"])
    ct.finalize()
    idx = np.asarray(c["census_idx"])
    got = ct.level(0)[1].cpu().numpy().astype(np.float64)[idx]
    ref = CO.unit_sums(c["ref"]["map"].numpy(), b, n)[idx]
    n_terms = CO.unit_sums(ct.visits.cpu().numpy(), b, n)[idx]
    bars = (c["M"] + 3) * U * ref + n_terms * 2.0 ** -31
    err = np.abs(got - ref)
    print(f"case {name}: worst / bar = {(err / np.maximum(bars, 1e-300)).max():.3f}")
    assert (err <= bars).all()


# ---- 8. two ranks ----------------------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, q):
    import torch.distributed as dist
    from popcorn_amd import eval as E
    from popcorn_amd.distributed import FlatReducer
    from tests.test_gpu_product import _members, _raster
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ms = _members()
    b, n = _model_level()
    ct = _table([b], [n], M=len(ms), h=MH, w=MW)
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, reducer=FlatReducer(), rank=rank, census=ct)
    torch.cuda.synchronize()
    q.put((rank, [t.cpu().numpy() for t in (ct.table, ct.totals, ct.mean, ct.std)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_table_equals_single_process():
    """Two gloo ranks on the one GPU (the process pattern of test_two_ranks_product_equals_single_process): EVERY rank's int64 table, and
    what finalize makes of it, equals the single-process one bit for bit."""
    from popcorn_amd import eval as E
    from tests.test_gpu_dp import _free_port, _get
    from tests.test_gpu_product import _members, _raster
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ms = _members()
    b, n = _model_level()
    one = _table([b], [n], M=len(ms), h=MH, w=MW)
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, census=one)
    ref = [t.cpu() for t in (one.table, one.totals, one.mean, one.std)]
    got = dict(_get(q, procs) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(got) == [0, 1] and int(ref[0].sum()) > 0
    for r in (0, 1):
        for a, want in zip(got[r], ref):
            assert torch.equal(torch.from_numpy(a), want), r


# ---- 9. paint and the detail maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 7])
def test_paint_equals_gather(K):
    """ops.census_paint == a torch gather, for the whole raster and for a row band that starts at an odd row (W = 170: the band starts on a
    4-byte boundary only, boundary and output planes at different 16-byte phases); ids outside [0, num_ids) paint 0."""
    from popcorn_amd import ops
    b = _levels()[0][0].copy()
    b[100:110, 30:40] = 27
    b[5:9, 160:] = INT32_MAX
    bt = torch.from_numpy(b).cuda()
    g = torch.Generator().manual_seed(19)
    tables = torch.rand(K, 27, generator=g).cuda() + 1.0
    ok = (bt >= 0) & (bt < 27)
    want = torch.where(ok, tables[:, bt.clamp(0, 26).long()], torch.zeros((), device="cuda"))
    out = ops.census_paint(bt, tables)
    assert out.shape == (K, H, W) and torch.equal(out, want)
    assert int((~ok).sum()) > 0 and not bool(out[:, ~ok].any())
    for r0, r1 in ((1, 150), (3, 4), (7, 8 + K)):
        full = torch.full((K * H * W + 1,), -7.0, device="cuda")[1:].view(K, H, W)     # (planes at another 16-byte phase than the boundary's)
        ops.census_paint(bt[r0:r1], list(tables), out=[full[k][r0:r1] for k in range(K)])
        assert torch.equal(full[:, r0:r1], want[:, r0:r1])
        assert bool((full[:, :r0] == -7.0).all()) and bool((full[:, r1:] == -7.0).all())
    with pytest.raises(ValueError):
        ops.census_paint(bt, torch.rand(9, 27).cuda())


def test_detail_maps_equal_the_restated_reference():
    """eval.census_detail_maps against tests/census_oracle.detail_maps (data/PopulationDataset.py:747-804 restated), exact in fp32: the
    per-unit values are computed once and gathered.  Census rows: every blocky unit but two (pixels of units without a row stay 0), a
    row whose unit is absent from the raster (id 26), a unit with POP20 = 0."""
    from popcorn_amd import eval as E
    ct = _run("rand", False)
    b = _levels()[0][0]
    rng = np.random.default_rng(23)
    idx = [i for i in range(27) if i not in (3, 25)]
    pop = (rng.random(len(idx)) * 3000).astype(np.float32)
    pop[4] = 0.0
    _, mean, std = ct.level(0)
    got = E.census_detail_maps(mean, torch.from_numpy(b).cuda(), idx, pop, pred_std=std)
    want = CO.detail_maps(mean.cpu().numpy(), b, idx, pop, pred_std=std.cpu().numpy())
    assert set(got) == set(want) == {"densities", "totals", "densities_gt", "totals_gt", "residuals", "residuals_rel", "totals_std"}
    for k in want:
        assert got[k].shape == (H, W) and got[k].dtype == torch.float32
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert not want["totals"][b == 3].any() and not want["totals"][b == -1].any() and float(want["totals"].max()) > 0
    assert set(E.census_detail_maps(mean, torch.from_numpy(b).cuda(), idx, pop)) == set(want) - {"totals_std"}


# ---- 10. CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_run_eval_cli_census_keys(capsys, tmp_path):
    """run_eval with --census_table: the JSON line gains the metrics of the table (ensemble mean, and mean / std over members of each
    metric) and nothing else changes; the table's metrics of the ensemble mean agree with those of the stitched mean map; --census_out
    holds the table and, with --census_details, the detail maps."""
    import json
    from popcorn_amd import cli
    base = "-S2 -NIR -S1 -occmodel -senbuilds -pret --biasinit 0.9407 --raster_hw 200 232 --patchsize 96 --overlap 8 --seed 1600 --ensemble 2"
    off = cli.run_eval(base.split())
    path = tmp_path / "census.pt"
    on = cli.run_eval((base + f" --census_table --census_out {path} --census_details").split())
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(printed) == set(on)
    assert all(on[k] == off[k] for k in off if k != "seconds")
    main = [k for k in off if k.startswith("Population_MainCensus_synthetic_fine/")]
    new = set(on) - set(off)
    assert len(main) > 0 and len(new) == 3 * len(main)
    for k in main:
        t = k.replace("MainCensus", "TableCensus")
        assert {t, t + "_members_mean", t + "_members_std"} <= new
        assert abs(on[t] - off[k]) <= 1e-4 * max(1.0, abs(off[k])), (k, on[t], off[k])
        assert on[t + "_members_std"] >= 0
    saved = torch.load(path, weights_only=False)
    assert saved["totals"].shape == (2, 401) and saved["mean"].shape == saved["std"].shape == (401,) and saved["num_ids"] == [401]
    assert float(saved["std"].max()) > 0
    assert set(saved["details"]) == {"densities", "totals", "densities_gt", "totals_gt", "residuals", "residuals_rel", "totals_std"}
    assert all(v.shape == (200, 232) for v in saved["details"].values())
