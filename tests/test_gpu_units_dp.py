"""Multi-unit census supervision under data parallelism (``FusedTrainStep(device_units=True)`` with an active reducer), after the pattern
of tests/test_gpu_dp.py: two gloo ranks that share the one GPU of the test box, eagerly and with the split HIP graphs, on the two halves
of a 4-crop multi-unit batch whose ranks hold DIFFERENT numbers of pairs -- rank 0 rows [3, 1], rank 1 rows [2, 3] -- against the
single-process eager multi-unit step on the whole batch (N = 9).  The loss is the mean over the 9 pairs: each rank divides by the global
N that travelled in the stats all-reduce.  The bar on the parameters after three steps is test_gpu_dp.py's: 2e-5 of max|p|."""
import os

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_gpu_dp import _free_port, _get

pytestmark = pytest.mark.gpu

UNITS = ((12, 3, 7), (9,), (5, 8), (6, 2, 11))            # census_n = [3, 1, 2, 3]
K = 3


def _make():
    from tests import units_oracle as U
    inputs, y = U.make_case(B=4, H=32, W=32, units=UNITS, channels=6, seed=11, pad_to=K)
    return {**inputs, "y": y}


def _run(rank, world, port, use_graph, q):
    import torch.distributed as dist
    from popcorn_amd.distributed import FlatReducer
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    rccl1 = world in ("rccl1", "rccl1split")   # ONE rank on the real backend, the multi-rank code path forced (as tests/test_gpu_dp.py)
    if rccl1:
        os.environ.update(POPCORN_DIST_FORCE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                          POPCORN_DP_ONE_GRAPH="0" if world == "rccl1split" else "1")
        split = world == "rccl1split"
        world = 1
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1)
    elif world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    if world > 1 or rccl1:
        tr = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, gradient_clip=0.01, reducer=FlatReducer(), use_graph=use_graph,
                            device_units=True)
    else:           # the reference: the plain eager multi-unit step, host N
        tr = FusedTrainStep(m, lr=1e-3, weight_decay=1e-5, gradient_clip=0.01)
    full = _make()
    per = 4 // world
    rows = list(range(rank * per, (rank + 1) * per))      # contiguous halves: rank 0 rows [3, 1], rank 1 rows [2, 3]
    s = {k: (v[rows].cuda() if torch.is_tensor(v) else [v[i] for i in rows]) for k, v in full.items()}
    losses, ns = [], []
    for step in range(3):
        torch.manual_seed(100 + step)            # same selection grid on every rank
        l = tr.step(dict(s))
        losses.append(l[0].item())
        if world > 1 or rccl1:
            ns.append((int(tr.last["unit_n"].item()), float(tr.stats[2].item())))
    torch.cuda.synchronize()
    if rccl1:
        assert tr.reducer.active and dist.get_backend() == "nccl" and tr.device_unit_steps == 3
        assert ns == [(9, 9.0)] * 3, ns
        # both collectives captured inside the one replayed graph, or three graphs around two eager collectives
        assert tr.captures == 1 and len(tr._graphs[3]) == (3 if split else 1), (len(tr._graphs[3]), tr.reducer.capture_failed)
    elif world > 1:
        assert tr.reducer.active and tr.device_unit_steps == 3
        assert ns == [(sum(s["census_n"]), 9.0)] * 3, ns          # the local N, and the global one after the stats all-reduce
        if use_graph:
            assert tr.captures == 1 and len(tr._graphs[3]) == 3   # gloo: three graphs around two eager collectives
    if rank == 0:
        q.put((tr.flat_p.cpu().numpy().tolist(), losses))
    if world > 1 or rccl1:
        dist.barrier()
        dist.destroy_process_group()


def _launch(world, use_graph):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run, args=(r, world, port, use_graph, q)) for r in range(1 if isinstance(world, str) else world)]
    for p in procs:
        p.start()
    out = _get(q, procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return out


_single = []


def _reference():
    if not _single:
        _single.append(_launch(1, False))
    return _single[0]


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_ranks_with_different_n_equal_the_single_process_step(use_graph):
    p1, l1 = _reference()
    p2, l2 = _launch(2, use_graph)
    p1, p2 = torch.tensor(p1), torch.tensor(p2)
    scale = p1.abs().max().item()
    dev = (p1 - p2).abs().max().item()
    print(f"\n[multi-unit DP, use_graph={use_graph}] max |dp| = {dev:.3e} = {dev / scale:.3e} of max|p| (bar 2e-5); "
          f"rank-0 losses {l2} vs whole-batch {l1}")
    assert dev <= 2e-5 * scale, dev
    assert all(abs(a) < 1e6 for a in l2)


@pytest.mark.parametrize("mode", ["rccl1", "rccl1split"])
def test_rccl_collectives_in_the_device_n_graph_step(mode):
    """The data-parallel device-N step with its REAL backend: one rank on nccl (= RCCL), the multi-rank path forced -- the four-double
    stats all-reduce that carries N and the gradient all-reduce CAPTURED inside the one replayed graph (POPCORN_DP_ONE_GRAPH=1), or
    issued eagerly between three graphs.  With one rank the sums are identities: parameters and losses equal the plain single-process
    eager multi-unit step exactly."""
    p1, l1 = _reference()
    pr, lr = _launch(mode, True)
    assert pr == p1 and lr == l1


def _run_cli(rank, world, port, fixed_hw, save_dir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world),
                      POPCORN_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from popcorn_amd.cli import run_train
    argv = ("-S2 -NIR -S1 -occmodel -senbuilds -pret -wd 1e-5 --biasinit 0.9407 -e 1 --synthetic_regions 16 -wb 2 -lt 2 "
            f"--units_per_crop 3 --device_units --max_steps 3 --save-model no --save_dir {save_dir}").split()
    argv += ["--fixed_hw", "64", "64"] if fixed_hw else ["--synthetic_hw_range", "48", "64"]
    t = run_train(argv)
    torch.cuda.synchronize()
    ok = (t.info["iter"] == 3 and t.fused.device_unit_steps == 3 and t.fused.reducer.active and
          bool(torch.isfinite(t.fused.loss_out).all()) and bool(torch.isfinite(t.fused.flat_p).all()) and
          t.fused.captures == (1 if fixed_hw else 0))
    # every rank holds the same parameters after the same reduced gradients
    ps = [torch.zeros_like(t.fused.flat_p).cpu() for _ in range(world)]
    dist.all_gather(ps, t.fused.flat_p.cpu())
    ok = ok and all(torch.equal(ps[0], p) for p in ps[1:])
    if rank == 0:
        q.put(bool(ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("fixed_hw", [False, True])
def test_run_train_device_units_under_the_launchers_data_parallel_mode(fixed_hw, tmp_path):
    """run_train.py --units_per_crop 3 --device_units with RANK / WORLD_SIZE set as the launcher sets them (two gloo ranks on the one
    GPU): eager on variable regions, and --fixed_hw with the split graphs; three steps, finite, the ranks' parameters identical."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_run_cli, args=(r, 2, port, fixed_hw, str(tmp_path / f"r{r}"), q)) for r in range(2)]
    for p in procs:
        p.start()
    ok = _get(q, procs, timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert ok


def test_switch_off_keeps_the_refusal_under_a_reducer():
    """Without ``device_units`` an active reducer still refuses a multi-unit sample (no process group needed: the flag alone decides)."""
    from popcorn_amd.distributed import FlatReducer
    from popcorn_amd.model import POPCORN
    from popcorn_amd.train import FusedTrainStep
    torch.manual_seed(1600)
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True).cuda()
    red = FlatReducer()
    red.active = True
    tr = FusedTrainStep(m, reducer=red)
    full = _make()
    s = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in full.items()}
    with pytest.raises(NotImplementedError):
        tr.step(s)
