"""The product grid (csrc/product.hip, eval.ProductGrid, ops.block_sum): per-member cell x cell block sums stitched across windows on the
device, against a float64 restatement of the reference's loop (interior ``+=``, divide by the visit count) followed by a float64 block sum
and the mean / (n - 1) standard deviation over members.

Rounding bars.  u = 2^-24 (fp32 unit round-off).  All terms are non-negative, so a sum in which every term passes through at most D
roundings is within D * u (relative) of the exact sum.  The kernel's order of additions per member and cell: a term is divided by its
visit count (1 rounding), added down its column inside the tile (<= cell - 1), the column sums of the cell are added left to right
(<= cell - 1), and that partial is added to the plane by this launch and by every later launch that touches the cell (<= Wn in all, Wn =
the largest number of windows whose interior meets one cell):  D = 2 * cell - 1 + Wn.  That is below the cell^2 + 8 of an arbitrary
order for every geometry used here (asserted).  The (n - 1) standard deviation is at most sqrt(2)-Lipschitz in a sup-norm perturbation of
the member totals: |std - std_ref| <= 2 * D * u * max_m T_m (the slack over sqrt(2) covers its own final rounding)."""
import functools
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


# ---- the float64 yardstick (CPU) ----------------------------------------------------------------------------------------------------------
def block_sum64(maps, cell):
    """(..., H, W) -> (..., ceil(H / cell), ceil(W / cell)) float64 sums over cells anchored at (0, 0); partial cells sum what exists."""
    h, w = maps.shape[-2:]
    hc, wc = -(-h // cell), -(-w // cell)
    p = torch.zeros(*maps.shape[:-2], hc * cell, wc * cell, dtype=torch.float64)
    p[..., :h, :w] = maps
    return p.reshape(*maps.shape[:-2], hc, cell, wc, cell).sum(dim=(-3, -1))


def members_mean_std(planes):
    """mean and (n - 1) standard deviation over dim 0 of float64 member totals (std 0 for one member)."""
    M = planes.shape[0]
    mean = planes.sum(0) / M
    std = torch.sqrt(((planes - mean) ** 2).sum(0) / (M - 1)) if M > 1 else torch.zeros_like(mean)
    return mean, std


def product_reference(h, w, wins, ps, ov, cell):
    """wins: list of (row origin, column origin, popdense (M, ps, ps)) with every window inside the raster.  Per member the full-raster map
    by the reference's loop (run_eval.py:108-154: interior ``+=``, then divide by the visit count), block-summed in float64.
    Returns (planes (M, Hc, Wc), mean, std, visits (h, w) int16)."""
    from popcorn_amd.eval import create_mask
    M = wins[0][2].shape[0]
    maps = torch.zeros(M, h, w, dtype=torch.float64)
    visits = torch.zeros(h, w, dtype=torch.int16)
    mask = create_mask(ps, ps, ov)
    for xl, yl, pd in wins:
        maps[:, xl:xl + ps, yl:yl + ps][:, mask] += pd.double()[:, mask]
        visits[xl:xl + ps, yl:yl + ps][mask] += 1
    seen = visits > 0
    maps[:, seen] /= visits[seen].double()
    planes = block_sum64(maps, cell)
    return (planes, *members_mean_std(planes), visits)


def max_windows_per_cell(h, w, idx, ps, ov, cell):
    """Wn: the largest number of windows of the list whose (clipped) interior meets one cell."""
    n = torch.zeros(-(-h // cell), -(-w // cell), dtype=torch.int64)
    for r in idx.tolist():
        x0, x1, y0, y1 = r[0] + ov, min(r[0] + ps - ov, h), r[1] + ov, min(r[1] + ps - ov, w)
        if x1 > x0 and y1 > y0:
            n[x0 // cell:(x1 - 1) // cell + 1, y0 // cell:(y1 - 1) // cell + 1] += 1
    return int(n.max())


def roundings(h, w, idx, ps, ov, cell):
    D = 2 * cell - 1 + max_windows_per_cell(h, w, idx, ps, ov, cell)
    assert D <= cell * cell + 8
    return D


# ---- stitcher level: the geometry of test_stitcher_vs_reference_loop (interior 48, regular + catch-up windows: visit counts 1, 2, 4) -----
H, W, PS, OV, M3 = 150, 170, 64, 8, 3


@functools.lru_cache(maxsize=None)
def _windows(kind, fourseasons, M=M3):
    from popcorn_amd import eval as E
    idx = E.get_patch_indices(H, W, PS, OV, fourseasons)
    g = torch.Generator().manual_seed(11)
    wins = []
    for x, y, s in idx.tolist():
        if kind == "exact":          # multiples of 4 in [0, 60]: every v / visits (visits 1, 2, 4) and every sum is exact in fp32
            pd = (4 * torch.randint(0, 16, (M, PS, PS), generator=g)).float()
        else:
            pd = torch.rand(M, PS, PS, generator=g)
        wins.append((x, y, pd))
    return idx, wins


@functools.lru_cache(maxsize=None)
def _reference(kind, fourseasons, cell, M=M3):
    return product_reference(H, W, _windows(kind, fourseasons, M)[1], PS, OV, cell)


def _run(kind, fourseasons, cell, M=M3):
    from popcorn_amd import eval as E
    idx, wins = _windows(kind, fourseasons, M)
    pg = E.ProductGrid(H, W, cell, M, "cuda")
    pg.set_windows(idx, PS, OV)
    for x, y, pd in wins:
        pg.add_window(x, y, pd.cuda(), OV)
    pg.finalize()
    return pg


@pytest.mark.parametrize("cell", [1, 7, 10, 16, 64])
def test_exact_geometry(cell):
    """No pixel dropped, duplicated or put into the wrong cell, at any cell size: with integer inputs whose quotients and sums are exact
    in fp32 the planes, the mean and the visit map EQUAL the float64 reference.  cell = 1 reproduces the 10 m mean map of the Stitcher
    wherever a pixel was visited; cell = 64 exceeds the interior of 48 (cells span several windows); 7 and 10 leave partial cells at both
    edges."""
    from popcorn_amd import eval as E
    planes, mean, std, visits = _reference("exact", False, cell)
    assert set(visits.unique().tolist()) == {0, 1, 2, 4}
    pg = _run("exact", False, cell)
    assert pg.cells.shape == (M3, *E.product_shape(H, W, cell)) and pg.mean.shape == pg.std.shape == pg.cells.shape[1:]
    assert torch.equal(pg.visits.cpu(), visits)
    assert torch.equal(pg.cells.cpu().double(), planes)
    assert torch.equal(pg.mean.cpu(), mean.float())          # sum of exact totals / M in double, rounded once
    torch.testing.assert_close(pg.std.cpu().double(), std, rtol=2.0 ** -23, atol=0)
    if cell == 1:
        st = E.Stitcher(H, W, "cuda", with_scale=False)
        for x, y, pd in _windows("exact", False)[1]:
            st.add_window(x, y, pd.cuda(), None, OV)
        out = st.finalize()[0]
        seen = st.count > 0
        assert torch.equal(st.count, M3 * pg.visits)
        assert torch.equal(pg.mean[seen], out[seen]) and not bool(pg.mean[~seen].any())


def _check_rounding(pg, ref, D):
    planes, mean, std, visits = ref
    got = pg.cells.cpu().double()
    err = (got - planes).abs() / planes.clamp_min(1e-300)
    print(f"planes: worst |T - T_ref| / T_ref = {err.max().item() / U:.2f} u (bar {D} u)")
    assert bool(((got - planes).abs() <= D * U * planes).all())
    gm = pg.mean.cpu().double()
    print(f"mean: worst {((gm - mean).abs() / mean.clamp_min(1e-300)).max().item() / U:.2f} u (bar {(D + 1)} u)")
    assert bool(((gm - mean).abs() <= (D + 1) * U * mean).all())
    tmax = planes.max(0).values
    es = (pg.std.cpu().double() - std).abs()
    print(f"std: worst |std - std_ref| / max_m T_m = {(es / tmax.clamp_min(1e-300)).max().item() / U:.2f} u (bar {2 * D} u)")
    assert bool((es <= 2 * D * U * tmax).all())


@pytest.mark.parametrize("fourseasons", [False, True])
@pytest.mark.parametrize("cell", [7, 10])
def test_rounding(cell, fourseasons):
    """Uniform random (non-negative) windows: planes and mean within D * u (D + 1 for the mean) of the float64 reference per cell, std
    within 2 * D * u * max_m T_m (module docstring; D = 2 * cell - 1 + Wn <= cell^2 + 8)."""
    idx = _windows("rand", fourseasons)[0]
    ref = _reference("rand", fourseasons, cell)
    assert int(ref[3].max()) == (16 if fourseasons else 4)
    pg = _run("rand", fourseasons, cell)
    assert torch.equal(pg.visits.cpu(), ref[3])
    _check_rounding(pg, ref, roundings(H, W, idx, PS, OV, cell))


def test_two_runs_give_the_same_bits():
    a, b = _run("rand", True, 10), _run("rand", True, 10)
    assert torch.equal(a.cells, b.cells) and torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std)


def test_single_member_has_zero_std_and_bad_arguments_raise():
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    from popcorn_amd._lib import PopcornHipError
    pg = _run("rand", False, 10, M=1)
    assert not bool(pg.std.any()) and torch.equal(pg.mean, pg.cells[0])
    with pytest.raises(ValueError):
        E.ProductGrid(H, W, 0, 1, "cuda")
    with pytest.raises(PopcornHipError):
        E.ProductGrid(H, W, 10, 1, "cpu")
    with pytest.raises(PopcornHipError):
        pg.add_window(0, 0, torch.zeros(1, PS, PS), OV)
    with pytest.raises(ValueError):
        pg.add_window(0, 0, torch.zeros(2, PS, PS, device="cuda"), OV)
    with pytest.raises(PopcornHipError):
        ops.block_sum(torch.zeros(8, 8), 2)
    with pytest.raises(ValueError):
        ops.block_sum(torch.zeros(8, 8, device="cuda"), 0)


def test_more_members_than_one_pass_holds():
    """The kernel keeps the column sums of 8 members in registers per pass: 9 members take two passes over the window."""
    planes, mean, std, visits = _reference("exact", False, 10, M=9)
    pg = _run("exact", False, 10, M=9)
    assert torch.equal(pg.cells.cpu().double(), planes) and torch.equal(pg.mean.cpu(), mean.float())


@pytest.mark.parametrize("cell", [1, 3, 10, 256, 300, 1000])
def test_block_sum_exact(cell):
    """ops.block_sum on small integers (exact sums) == the float64 block sum: 701 x 700 is no multiple of any cell, cell = 1 needs more
    tiles than the grid has workgroups (tile-stride loop), cell >= 256 is the one-cell-per-tile form whose lanes stride over the columns,
    cell = 1000 is a single partial cell."""
    from popcorn_amd import ops
    g = torch.Generator().manual_seed(12)
    m = torch.randint(0, 16, (701, 700), generator=g).float()
    assert torch.equal(ops.block_sum(m.cuda(), cell).cpu().double(), block_sum64(m.double(), cell))


# ---- model level ----------------------------------------------------------------------------------------------------------------------------
MH, MW, MPS, MOV, MCELL = 200, 232, 96, 16, 10


def _members():
    from popcorn_amd.model import POPCORN
    ms = []
    for seed in (1600, 1601):
        torch.manual_seed(seed)
        ms.append(POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda().eval())
    return ms


def _raster():
    return torch.randn(1, 6, MH, MW, generator=torch.Generator().manual_seed(5)).cuda()


def test_evaluate_raster_product_vs_single_member_maps():
    """evaluate_raster(models, raster, product=pg) of a two-member ensemble against existing functionality only: each member's own 10 m
    map (evaluate_raster([m_j], raster)), block-summed in float64 on the CPU, then mean / std over members.  A pixel of such a 10 m map
    has itself passed through V roundings (V - 1 accumulations and the division by the count, V = the largest visit count), so the bars
    are those of test_rounding with D + V.  Also: pg.mean against ops.block_sum of the ensemble's own 10 m mean map (whose pixels carry
    M + V roundings, and the block sum 2 * cell - 2 more), ops.block_sum against the float64 block sum, and the four returned maps with
    and without ``product`` are the same bits."""
    from popcorn_amd import eval as E
    from popcorn_amd import ops
    ms, raster = _members(), _raster()
    pg = E.ProductGrid(MH, MW, MCELL, len(ms), "cuda")
    maps = E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV, product=pg)
    plain = E.evaluate_raster(ms, raster, patchsize=MPS, overlap=MOV)
    for a, b in zip(maps, plain):
        assert torch.equal(a.nan_to_num(-1.0), b.nan_to_num(-1.0))
    idx = E.get_patch_indices(MH, MW, MPS, MOV, False)
    V = int(pg.visits.max())
    D = roundings(MH, MW, idx, MPS, MOV, MCELL) + V
    assert D + 2 * MCELL + len(ms) <= MCELL * MCELL + 8
    planes = torch.stack([block_sum64(E.evaluate_raster([m], raster, patchsize=MPS, overlap=MOV)[0].cpu().double(), MCELL) for m in ms])
    assert bool((planes >= 0).all()) and float(planes.max()) > 0
    _check_rounding(pg, (planes, *members_mean_std(planes), None), D)
    # the product mean IS the block sum of the 10 m mean map
    bs = ops.block_sum(maps[0], MCELL).cpu().double()
    exact = block_sum64(maps[0].cpu().double(), MCELL)
    assert bool(((bs - exact).abs() <= (2 * MCELL - 2) * U * exact).all())
    assert bool(((pg.mean.cpu().double() - bs).abs() <= (D + 2 * MCELL + len(ms)) * U * bs).all())


def _rank(rank, world, port, q):
    import torch.distributed as dist
    from popcorn_amd import eval as E
    from popcorn_amd.distributed import FlatReducer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ms = _members()
    pg = E.ProductGrid(MH, MW, MCELL, len(ms), "cuda")
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, reducer=FlatReducer(), rank=rank, product=pg)
    torch.cuda.synchronize()
    q.put((rank, [t.cpu().numpy() for t in (pg.cells, pg.mean, pg.std, pg.visits)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_product_equals_single_process():
    """Two gloo ranks on the one GPU (fresh spawned children, the process pattern of tests/test_gpu_dp.py), the default band-reduce form:
    EVERY rank's product equals the single-process one within twice the bars of test_rounding (both sides are fp32 sums of the same
    terms in different orders: each within D * u of the exact value, the all-reduce adds one rounding); the visit maps are equal."""
    from popcorn_amd import eval as E
    from tests.test_gpu_dp import _free_port, _get
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ms = _members()
    one = E.ProductGrid(MH, MW, MCELL, len(ms), "cuda")
    E.evaluate_raster(ms, _raster(), patchsize=MPS, overlap=MOV, product=one)
    D = roundings(MH, MW, E.get_patch_indices(MH, MW, MPS, MOV, False), MPS, MOV, MCELL) + 1
    ref = (one.cells.cpu().double(), one.mean.cpu().double(), one.std.cpu().double(), one.visits.cpu())
    got = dict(_get(q, procs) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert sorted(got) == [0, 1]
    for r in (0, 1):
        cells, mean, std, visits = (torch.from_numpy(a) for a in got[r])
        assert torch.equal(visits, ref[3])
        assert bool(((cells.double() - ref[0]).abs() <= 2 * D * U * ref[0]).all()), r
        assert bool(((mean.double() - ref[1]).abs() <= 2 * (D + 1) * U * ref[1]).all()), r
        assert bool(((std.double() - ref[2]).abs() <= 2 * 2 * D * U * ref[0].max(0).values).all()), r


def test_run_eval_cli_product_keys(capsys, tmp_path, monkeypatch):
    """run_eval with --product_cell: the JSON line gains the five product keys and nothing else changes; the product partitions the raster,
    so product_total is the sum of the 10 m mean map and product_adj_total the sum of the adjusted map (= the census total of the
    regions with a non-zero prediction, to the adjustment tolerance of tests/test_gpu_eval.py); --product_out holds what the line sums."""
    import json
    from popcorn_amd import cli, eval as E
    from popcorn_amd.data.dataset import SyntheticTestRaster
    seen = {}
    adjust = E.adjust_map_to_census

    def spy(pred, *a):
        seen["out"] = pred.clone()
        seen["adj"] = adjust(pred, *a)
        return seen["adj"]
    monkeypatch.setattr(E, "adjust_map_to_census", spy)
    base = "-S2 -NIR -S1 -occmodel -senbuilds -pret --biasinit 0.9407 --raster_hw 200 232 --patchsize 96 --overlap 8 --seed 1600 --ensemble 2"
    off = cli.run_eval(base.split())
    path = tmp_path / "product.pt"
    on = cli.run_eval((base + f" --product_cell {MCELL} --product_out {path}").split())
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert set(printed) == set(on)
    assert set(on) - set(off) == {"product_cell", "product_shape", "product_total", "product_std_mean", "product_adj_total"}
    assert all(on[k] == off[k] for k in off if k != "seconds")
    saved = torch.load(path, weights_only=False)
    assert on["product_cell"] == saved["cell"] == MCELL and on["product_shape"] == [20, 24] == list(saved["mean"].shape)
    assert saved["std"].shape == saved["adjusted"].shape == saved["mean"].shape and float(saved["std"].max()) > 0
    assert on["product_total"] == saved["mean"].double().sum().item() and on["product_adj_total"] == saved["adjusted"].double().sum().item()
    bar = (MCELL * MCELL + 8) * U
    total = seen["out"].double().sum().item()
    assert total > 0 and abs(on["product_total"] - total) <= bar * total
    adj_total = seen["adj"].double().sum().item()
    assert abs(on["product_adj_total"] - adj_total) <= bar * adj_total
    data = SyntheticTestRaster(200, 232, device="cuda")
    sums = E.census_sums(seen["out"].contiguous(), data.boundary, 401)[1:].cpu()
    census = data.census_pop.double()[sums != 0].sum().item()
    assert int((sums != 0).sum()) > 300 and abs(adj_total - census) <= 2e-5 * census
