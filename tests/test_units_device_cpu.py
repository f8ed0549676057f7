"""The device-N multi-unit step without a GPU: the switch and its defaults, the contract of the device layout (tests/units_device_oracle.py)
against ``ops.unit_layout``'s host-count result, and the packed layout of ``static_buffers(units=K)``."""
import inspect

import pytest
import torch

from tests.units_device_oracle import I64_MAX, layout_dev_ref

BIG = (1 << 24) + 2


def test_device_units_is_opt_in():
    from popcorn_amd.cli import train_parser
    from popcorn_amd.train import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["device_units"].default is False
    assert train_parser().parse_args([]).device_units is False
    a = train_parser().parse_args(["--units_per_crop", "4", "--device_units", "--fixed_hw", "100", "100"])
    assert a.device_units is True and a.units_per_crop == 4 and a.fixed_hw == [100, 100]
    # the flag alone implies nothing
    assert train_parser().parse_args(["--device_units"]).units_per_crop == 0


def test_the_c_abi_names_the_two_entries():
    import os
    import popcorn_amd
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(popcorn_amd.__file__)), "include", "popcorn_hip.h")).read()
    from popcorn_amd import _lib as L
    assert "int pc_unit_layout_dev(" in hdr and "int pc_unit_popcount_loss_dev(" in hdr
    assert L.PC_ABI_VERSION == 10                                          # additive: the version stays


RAGGED = {
    "3x5": (torch.tensor([[9, 3, BIG, 7, 5], [8, 8, -1, I64_MAX, 8], [12, 4, 6, 4, I64_MAX]]), [5, 1, 3]),
    "2x7": (torch.tensor([[70, 10, 60, 20, 50, 30, 40], [5, 9, 3, 1, -1, -1, -1]]), [7, 4]),
    "4x1": (torch.tensor([[4], [3], [2], [1]]), [1, 1, 1, 1]),
}


@pytest.mark.parametrize("name", list(RAGGED))
def test_layout_contract_against_the_host_count_layout(name, monkeypatch):
    """Entries [0, N) of the restatement are ``ops.unit_layout``'s (pure torch once the device check is out of the way); the tails and
    unit_off[B] are what the header promises."""
    from popcorn_amd import _lib as L
    from popcorn_amd import ops
    monkeypatch.setattr(L, "require_device", lambda *a: None)
    cidx, cn = RAGGED[name]
    cidx = cidx.to(torch.int64)
    B, K = cidx.shape
    y = torch.rand(B, K, generator=torch.Generator().manual_seed(3)) * 300.0
    host = ops.unit_layout(cidx, cn)
    ref = layout_dev_ref(cidx, y, cn)
    N = host["N"]
    assert ref["N"] == N == sum(cn) and ref["Ncap"] == B * K
    assert torch.equal(ref["units"][:N], host["units"])
    assert torch.equal(ref["unit_off"], host["unit_off"]) and int(ref["unit_off"][B]) == N
    assert torch.equal(ref["y_sorted"][:N], y.reshape(-1)[host["to_sorted"]])
    to_caller = torch.empty(N, dtype=torch.int64)
    to_caller[ref["dest"][:N].long()] = torch.arange(N)
    assert torch.equal(to_caller, host["to_caller"])
    assert bool((ref["units"][N:] == I64_MAX).all()) and bool((ref["y_sorted"][N:] == 0).all()) and bool((ref["dest"][N:] == -1).all())
    if name == "2x7":
        assert ref["units"][7:11].tolist() == [1, 3, 5, 9]


def test_layout_contract_clamps_counts():
    cidx = torch.tensor([[9, 3, 7], [8, 2, 5]], dtype=torch.int64)
    y = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    got = layout_dev_ref(cidx, y, [0, 6])                                  # 0 -> 1, K + 3 -> K
    want = layout_dev_ref(cidx, y, [1, 3])
    assert got["counts"] == [1, 3] and got["N"] == 4
    for k in ("units", "unit_off", "y_sorted", "dest"):
        assert torch.equal(got[k], want[k])
    assert got["units"].tolist() == [9, 2, 5, 8, I64_MAX, I64_MAX] and got["dest"].tolist() == [0, 2, 3, 1, -1, -1]
    # a VALID INT64_MAX is the row's last unit, in front of the padding: its y and its slot travel with it
    v = layout_dev_ref(torch.tensor([[5, I64_MAX, 3, -1]]), torch.tensor([[1.0, 2.0, 3.0, 4.0]]), [3])
    assert v["units"].tolist() == [3, 5, I64_MAX, I64_MAX] and v["dest"].tolist() == [2, 0, 1, -1] and v["y_sorted"].tolist() == [3.0, 1.0, 2.0, 0.0]


def test_host_validation_precedes_the_clamp():
    """The public ``census_n`` is host data and is validated there: the trainer never relies on the kernel's clamp."""
    from popcorn_amd import ops
    for bad in ([0, 2], [1, 4], [1]):
        with pytest.raises(ValueError):
            ops._unit_counts(bad, 2, 3)
    assert ops._unit_counts(None, 2, 3) == [3, 3] and ops._unit_counts(torch.tensor([1, 3]), 2, 3) == [1, 3]


@pytest.mark.parametrize("B,H,W,K", [(2, 32, 32, 3), (3, 5, 7, 4), (1, 9, 9, 1)])
def test_packed_layout_of_a_multi_unit_static_set(B, H, W, K):
    from popcorn_amd.train import FusedTrainStep as F
    lay, total = F.packed_layout(B, H, W, units=K)
    assert set(lay) == {"admin_mask", "y", "census_idx", "census_n"}
    assert lay["y"][1:] == (torch.float32, (B, K)) and lay["census_idx"][1:] == (torch.int64, (B, K)) and lay["census_n"][1:] == (torch.int32, (B,))
    # 16-byte aligned, in order, no overlap, nothing behind the last
    size = {"admin_mask": B * H * W * 4, "y": B * K * 4, "census_idx": B * K * 8, "census_n": B * 4}
    end = 0
    for name in ("admin_mask", "y", "census_idx", "census_n"):
        off = lay[name][0]
        assert off % 16 == 0 and off >= end and off - end < 16
        end = off + size[name]
    assert total == end
    # pack_small is its host-side counterpart
    g = torch.Generator().manual_seed(B + K)
    admin = torch.randint(0, 50, (B, H, W), generator=g).float()
    y = torch.rand(B, K, generator=g)
    cidx = torch.randint(0, 1000, (B, K), generator=g)
    cn = [1 + (b % K) for b in range(B)]
    buf = F.pack_small(admin, y, cidx, cn)
    assert buf.dtype == torch.uint8 and buf.numel() == total
    v = F._packed_views(buf, lay)
    assert torch.equal(v["admin_mask"], admin) and torch.equal(v["y"], y) and torch.equal(v["census_idx"], cidx)
    assert v["census_n"].tolist() == cn


def test_packed_layout_of_a_one_unit_set_is_unchanged():
    """units = 0: byte for byte what ``pack_small`` has always written (admin_mask | y [B] padded to 16 | census_idx [B])."""
    from popcorn_amd.train import FusedTrainStep as F
    B, H, W = 3, 5, 5
    lay, total = F.packed_layout(B, H, W)
    n_am, n_y = B * H * W * 4, -(-B * 4 // 16) * 16
    assert set(lay) == {"admin_mask", "y", "census_idx"}
    assert (lay["admin_mask"][0], lay["y"][0], lay["census_idx"][0], total) == (0, n_am, n_am + n_y, n_am + n_y + B * 8)
    assert lay["y"][2] == (B,) and lay["census_idx"][2] == (B,)
    with pytest.raises(ValueError):
        F.packed_layout(B, H, W, units=-1)
