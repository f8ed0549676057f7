"""The two device-N kernels of csrc/units.hip, op level:

  * pc_unit_layout_dev against ``ops.unit_layout_device`` (the host-count launch) on the same counts -- entries [0, N) exact --, against
    the torch restatement of its contract (tests/units_device_oracle.py) over the WHOLE capacity, with the clamp, the zeroed workspace,
    n_dev / stats[2], and once between guard bands over poisoned memory (tests/footprint.py);
  * pc_unit_popcount_loss_dev against pc_unit_popcount_loss, bit for bit, with the tails, an Inf term, two calls on one workspace and a
    global N that is twice the local one.

Shapes: (B, K) = (1, 1) no sort round; (3, 5) ragged with junk in the padding and an id above 2^24; (2, 300) not a power of two, more
than one round of the 256 threads; (1, 1024) the cap; 1025 declined.  N = 1, 257 (crosses the one block's 256-thread stride), 1000, each
with Ncap = N + 7."""
import pytest
import torch

from tests.footprint import POISON, Footprint
from tests.units_device_oracle import I64_MAX, layout_dev_ref

pytestmark = pytest.mark.gpu

BIG = (1 << 24) + 2                      # an id above 2^24 that fp32 still holds exactly


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- pc_unit_layout_dev ----------------------------------------------------------------------------------------------------------------
def _layout_case(name):
    g = torch.Generator().manual_seed(5)
    if name == "1x1":
        cidx, cn = torch.tensor([[42]]), [1]
    elif name == "3x5_junk_padding":
        cidx = torch.tensor([[9, 3, BIG, 7, 5], [8, 8, -1, I64_MAX, 8], [12, 4, 6, 4, I64_MAX]])
        cn = [5, 1, 3]
    elif name == "2x300_ragged":
        cidx = torch.stack([1000 + torch.randperm(300, generator=g), 5000 + 3 * torch.randperm(300, generator=g)])
        cidx[1, 123:] = -1
        cn = [300, 123]
    elif name == "1x1024_cap":
        cidx, cn = (7 + 5 * torch.randperm(1024, generator=g)).reshape(1, 1024), [1024]
    else:
        raise KeyError(name)
    cidx = cidx.to(torch.int64)
    return cidx, torch.rand(cidx.shape, generator=g) * 300.0, cn


def _assert_layout(lay, ref, ws, stats):
    """every element of every output against the restatement; the workspace zero over exactly 20 Ncap bytes"""
    Ncap, N = ref["Ncap"], ref["N"]
    assert lay["Ncap"] == Ncap
    assert lay["units"].dtype == torch.int64 and torch.equal(lay["units"].cpu(), ref["units"])
    assert lay["unit_off"].dtype == torch.int32 and torch.equal(lay["unit_off"].cpu(), ref["unit_off"])
    assert torch.equal(_bits(lay["y_sorted"]), _bits(ref["y_sorted"]))
    assert lay["dest"].dtype == torch.int32 and torch.equal(lay["dest"].cpu(), ref["dest"])
    assert lay["n_dev"].dtype == torch.int32 and lay["n_dev"].tolist() == [N]
    assert float(stats[2]) == float(N)
    assert int(ws[:20 * Ncap].count_nonzero()) == 0
    assert bool((ws[20 * Ncap:] == 0xFF).all())


@pytest.mark.parametrize("name", ["1x1", "3x5_junk_padding", "2x300_ragged", "1x1024_cap"])
def test_unit_layout_dev_equals_the_host_count_launch(name):
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    cidx, y, cn = _layout_case(name)
    B, K = cidx.shape
    Ncap = B * K
    host = ops.unit_layout_device(cidx.cuda(), y.cuda(), cn)
    N = host["N"]
    need = L.lib().pc_unit_ws_bytes(Ncap)
    assert need >= 20 * Ncap and need % 16 == 0
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")          # 64 guard bytes behind the workspace
    stats = torch.tensor([11.0, 22.0, -1.0, 44.0], dtype=torch.float64, device="cuda")
    lay = ops.unit_layout_dev(cidx.cuda(), y.cuda(), torch.tensor(cn, dtype=torch.int32).cuda(), stats=stats, ws=ws)
    # entries [0, N): the host-count launch, exact
    assert torch.equal(lay["units"][:N], host["units"]) and torch.equal(lay["unit_off"], host["unit_off"])
    assert torch.equal(_bits(lay["y_sorted"][:N]), _bits(host["y_sorted"])) and torch.equal(lay["dest"][:N], host["dest"])
    # the whole capacity: the contract
    _assert_layout(lay, layout_dev_ref(cidx, y, cn), ws, stats)
    assert stats.tolist()[:2] == [11.0, 22.0] and stats.tolist()[3] == 44.0         # its neighbours in stats are not touched
    if name == "3x5_junk_padding":
        assert lay["units"][:N].tolist() == [3, 5, 7, 9, BIG, 8, 4, 6, 12]


def test_unit_layout_dev_clamps_the_device_counts():
    """The device cannot raise: 0 behaves as 1 and K + 3 as K."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    cidx, y, _ = _layout_case("3x5_junk_padding")
    out = []
    for cn in ([0, 8, 3], [1, 5, 3]):
        ws = torch.full((L.lib().pc_unit_ws_bytes(15) + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        stats = torch.zeros(4, dtype=torch.float64, device="cuda")
        lay = ops.unit_layout_dev(cidx.cuda(), y.cuda(), torch.tensor(cn, dtype=torch.int32).cuda(), stats=stats, ws=ws)
        _assert_layout(lay, layout_dev_ref(cidx, y, cn), ws, stats)
        out.append(lay)
    for k in ("units", "unit_off", "dest", "n_dev"):
        assert torch.equal(out[0][k], out[1][k])
    assert out[0]["n_dev"].tolist() == [9]


def test_unit_layout_dev_between_guard_bands_over_poisoned_memory():
    """Operands and every tensor the wrapper allocates sit between guard bands; the outputs start as 0xFF bytes.  Every element is
    written (the contract is met over the whole capacity) and nothing outside is."""
    from popcorn_amd import ops
    for name in ("3x5_junk_padding", "2x300_ragged"):
        cidx, y, cn = _layout_case(name)
        ref = layout_dev_ref(cidx, y, cn)
        with Footprint("cuda", fill=POISON) as fp:
            stats = fp.place(torch.zeros(4, dtype=torch.float64))
            lay = ops.unit_layout_dev(fp.place(cidx), fp.place(y), fp.place(torch.tensor(cn, dtype=torch.int32)), stats=stats)
            assert fp.guarded >= 10
        Ncap, N = ref["Ncap"], ref["N"]
        assert torch.equal(lay["units"].cpu(), ref["units"]) and torch.equal(lay["dest"].cpu(), ref["dest"])
        assert torch.equal(_bits(lay["y_sorted"]), _bits(ref["y_sorted"])) and torch.equal(lay["unit_off"].cpu(), ref["unit_off"])
        assert lay["n_dev"].tolist() == [N] and float(stats[2]) == float(N)
        assert int(lay["ws"][:20 * Ncap].count_nonzero()) == 0


def test_unit_layout_dev_declines_k_above_the_cap():
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    B, K = 1, L.PC_UNIT_LAYOUT_MAX_K + 1
    cidx = torch.arange(K, dtype=torch.int64, device="cuda").reshape(B, K)
    y = torch.zeros(B, K, device="cuda")
    cn = torch.full((B,), K, dtype=torch.int32, device="cuda")
    out = [torch.full((K + 8,), -7, dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.float32, torch.int32)]
    n_dev = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = L.lib().pc_unit_layout_dev(L.ptr(cidx), L.ptr(y), L.ptr(cn), B, K, *[L.ptr(t) for t in out], None, L.ptr(n_dev), None,
                                    L.stream_ptr())
    assert rc == L.PC_ENOTSUP
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in out + [n_dev])                      # nothing was launched
    with pytest.raises(L.PopcornHipError):
        ops.unit_layout_dev(cidx, y, cn)
    # argument checks return before a launch
    assert L.lib().pc_unit_layout_dev(L.ptr(cidx), L.ptr(y), None, B, 4, *[L.ptr(t) for t in out], None, L.ptr(n_dev), None,
                                      L.stream_ptr()) == L.PC_EINVAL
    with pytest.raises(ValueError):
        ops.unit_layout_dev(cidx[:, :4], y[:, :4], torch.ones(1, dtype=torch.int64, device="cuda"))


# ---- pc_unit_popcount_loss_dev ---------------------------------------------------------------------------------------------------------
LAM4, SREG, LAM_WEAK = [0.5, 1.0, 0.25, 0.125], 0.01, 100.0
# N -> (counts, K, (H, W)): B * K = N + 7
TAIL_CASES = {1: ([1], 8, (37, 53)), 257: ([132, 125], 132, (64, 64)), 1000: ([53] * 18 + [46], 53, (16, 20))}


def _tail_case(N):
    """cidx, y, counts with sum = N and B K = N + 7, a slot map in the kernels' numbering (a fifth of the pixels unowned), a density map."""
    cn, K, (H, W) = TAIL_CASES[N]
    B = len(cn)
    assert sum(cn) == N and B * K == N + 7
    g = torch.Generator().manual_seed(N * 7 + H)
    cidx = torch.full((B, K), -1, dtype=torch.int64)
    for b, c in enumerate(cn):
        cidx[b, :c] = 100 + torch.randperm(3 * K, generator=g)[:c]
    y = torch.rand(B, K, generator=g) * 300.0
    slot = torch.empty(B, H, W, dtype=torch.int32)
    off = 0
    for b, c in enumerate(cn):
        s = torch.randint(0, c, (H, W), generator=g) + off
        s[torch.rand(H, W, generator=g) < 0.2] = -1
        slot[b] = s.to(torch.int32)
        off += c
    pd = torch.rand(B, H, W, generator=g) * 10.0 ** torch.randint(-4, 2, (B, H, W), generator=g).float()
    pd[torch.rand(B, H, W, generator=g) < 0.25] = 0.0
    return cidx.cuda(), y.cuda(), cn, slot.cuda(), pd.cuda()


def _outputs():
    return torch.full((2,), -1.0, device="cuda"), torch.full((1,), -1.0, device="cuda")


def _stats(slot):
    return torch.tensor([float((slot >= 0).sum()), 1234.5, 0.0, 0.0], dtype=torch.float64, device="cuda")


def _host_tail(cidx, y, cn, slot, pd):
    """pc_unit_layout + pc_unit_popcount_loss: the host-N form."""
    from popcorn_amd import ops
    lay = ops.unit_layout_device(cidx, y, cn)
    loss, gsc = _outputs()
    g = torch.empty(lay["N"], device="cuda")
    pcs, pcc = ops.unit_popcount_loss(pd, slot, lay, _stats(slot), LAM4, SREG, LAM_WEAK, loss, g, gsc)
    return pcs, pcc, loss, g, gsc


def _dev_tail(cidx, y, cn, slot, pd, ws=None, n_global=None):
    from popcorn_amd import ops
    stats = _stats(slot)
    lay = ops.unit_layout_dev(cidx, y, torch.tensor(cn, dtype=torch.int32).cuda(), stats=stats, ws=ws)
    if n_global is not None:
        stats[2] = float(n_global)                                       # (what the stats all-reduce leaves there)
    loss, gsc = _outputs()
    g = torch.full((lay["Ncap"],), 7.0, device="cuda")
    out = (torch.full((lay["Ncap"],), 7.0, device="cuda"), torch.full((lay["Ncap"],), 7.0, device="cuda"))
    pcs, pcc = ops.unit_popcount_loss_dev(pd, slot, lay, stats, LAM4, SREG, LAM_WEAK, loss, g, gsc, out=out)
    return pcs, pcc, loss, g, gsc, lay, stats


NAMES = ("popcount sorted", "popcount caller", "loss_out", "g_popcount", "g_scale_const")


def _assert_tail(got, want, N, tag=""):
    for i, n in enumerate(NAMES):
        a, b = got[i], want[i]
        if i in (0, 1, 3):
            assert a.numel() == N + 7 and not bool(a[N:].any()), (tag, n, "tail")          # the tails are exactly 0
            a = a[:N]
        assert torch.equal(_bits(a), _bits(b)), (tag, n)


@pytest.mark.parametrize("N", list(TAIL_CASES))
def test_unit_popcount_loss_dev_is_bitwise_the_host_form(N):
    from popcorn_amd import _lib as L
    cidx, y, cn, slot, pd = _tail_case(N)
    want = _host_tail(cidx, y, cn, slot, pd)
    ws = torch.full((L.lib().pc_unit_ws_bytes(N + 7),), 0xFF, dtype=torch.uint8, device="cuda")
    got = _dev_tail(cidx, y, cn, slot, pd, ws)
    _assert_tail(got, want, N)
    assert got[5]["n_dev"].tolist() == [N] and float(got[6][2]) == float(N)
    assert bool(torch.isfinite(got[2]).all()) and float(got[0].max()) > 0
    # twice in a row on the same workspace: the layout launch re-zeroes it
    _assert_tail(_dev_tail(cidx, y, cn, slot, pd, ws), want, N, "second call")
    # an Inf term makes ITS unit NaN, bitwise as the host form does; the other units keep their bits
    tgt = int(slot[slot >= 0][0])
    pd2 = pd.clone()
    pd2.view(-1)[int((slot.view(-1) == tgt).nonzero()[0])] = float("inf")
    bad = _dev_tail(cidx, y, cn, slot, pd2, ws)
    assert bool(torch.isnan(bad[0][tgt]))
    _assert_tail(bad, _host_tail(cidx, y, cn, slot, pd2), N, "inf")
    keep = torch.arange(N + 7, device="cuda") != tgt
    assert torch.equal(_bits(bad[0][keep]), _bits(got[0][keep]))


@pytest.mark.parametrize("N", list(TAIL_CASES))
def test_unit_popcount_loss_dev_takes_the_global_n_from_stats(N):
    """stats[2] = 2 N (two ranks of N pairs each): g_popcount is ``ops.loss_fwd_bwd`` on the same popcounts with inv_B = 1 / (2 N), bit
    for bit; the popcounts themselves do not depend on it."""
    from popcorn_amd import ops
    cidx, y, cn, slot, pd = _tail_case(N)
    local = _dev_tail(cidx, y, cn, slot, pd)
    got = _dev_tail(cidx, y, cn, slot, pd, n_global=2 * N)
    lay, stats = got[5], got[6]
    assert float(stats[2]) == 2.0 * N and lay["n_dev"].tolist() == [N]
    assert torch.equal(_bits(got[0]), _bits(local[0])) and torch.equal(_bits(got[1]), _bits(local[1]))
    loss, gsc = _outputs()
    g = torch.empty(N, device="cuda")
    ops.loss_fwd_bwd(got[0][:N].contiguous(), lay["y_sorted"][:N].contiguous(), stats, LAM4, SREG, LAM_WEAK, 1.0 / (2 * N), loss, g, gsc)
    assert torch.equal(_bits(got[3][:N]), _bits(g)) and not bool(got[3][N:].any())
    assert torch.equal(_bits(got[2]), _bits(loss)) and torch.equal(_bits(got[4]), _bits(gsc))
    assert not torch.equal(_bits(got[3][:N]), _bits(local[3][:N]))                 # (and it is not the local mean's gradient)


def test_unit_popcount_loss_dev_argument_checks():
    from popcorn_amd import ops
    cidx, y, cn, slot, pd = _tail_case(1)
    stats = _stats(slot)
    lay = ops.unit_layout_dev(cidx, y, torch.tensor(cn, dtype=torch.int32).cuda(), stats=stats)
    loss, gsc = _outputs()
    with pytest.raises(ValueError):
        ops.unit_popcount_loss_dev(pd, slot, lay, stats, LAM4, SREG, LAM_WEAK, loss, torch.empty(1, device="cuda"), gsc)      # g of N, not Ncap
    with pytest.raises(ValueError):
        ops.unit_popcount_loss_dev(pd, slot, lay, stats[:2].contiguous(), LAM4, SREG, LAM_WEAK, loss, torch.empty(8, device="cuda"), gsc)
    with pytest.raises(ValueError):
        ops.unit_popcount_loss_dev(pd, slot.long(), lay, stats, LAM4, SREG, LAM_WEAK, loss, torch.empty(8, device="cuda"), gsc)
