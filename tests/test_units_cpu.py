"""Multi-unit census supervision, the parts that need no GPU: the C ABI additions, the one-pass restatement of tests/units_oracle.py
against the committed oracle on the replicated batch (the definition of the feature), and the multi-unit collate."""
import os
import re

import pytest
import torch

from oracle import popcorn_oracle as O
from tests import units_oracle as U

G = os.path.join(os.path.dirname(__file__), "golden")


def test_abi_additions():
    from popcorn_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "popcorn_hip.h")).read()
    for name in ("pc_unit_mask", "pc_unit_popcount", "pc_unit_ws_bytes", "pc_unit_paint"):
        assert re.search(rf"\b(int|int64_t) {name}\(", hdr), name
    lib = L.lib()
    assert all(hasattr(lib, n) for n in ("pc_unit_mask", "pc_unit_popcount", "pc_unit_ws_bytes", "pc_unit_paint"))
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10            # additive: no version bump
    assert int(re.search(r"#define PC_CENSUS_FIX_SHIFT (\d+)", hdr).group(1)) == 30 and L.PC_UNIT_QUANTUM == 2.0 ** -30
    assert lib.pc_unit_ws_bytes(1) >= 20 and lib.pc_unit_ws_bytes(300) >= 20 * 300 and lib.pc_unit_ws_bytes(300) % 16 == 0


def _state(channels):
    sd = O.load_golden_state(G)
    if channels == 6:
        return sd
    # single modality: the head's first layer sees the 8 features of the one stream (popcorn.py:68-69)
    sd = dict(sd)
    g = torch.Generator().manual_seed(5)
    sd["head.0.weight"] = sd["head.0.weight"][:, :8].clone() + 0.01 * torch.randn(64, 8, 1, 1, generator=g)
    return sd


CASES = [
    # (id, channels, occupancymodel)
    ("dual_occ", 6, True),
    ("s1_only", 2, True),
    ("dual_noocc", 6, False),
]


def _compare(sd, inputs, y, channels, occ):
    """(Nsel, popcount / loss / worst-gradient relative errors, popdensemap error) of the one-pass restatement against the committed
    oracle on the replicated batch, in the dtype of ``sd``; asserts the exact parts."""
    torch.manual_seed(11)
    l_ref, o_ref, g_ref = U.replicated_train_step_grads(sd, dict(inputs), y, occupancymodel=occ)
    torch.manual_seed(11)
    l_one, o_one, g_one = U.units_train_step_grads(sd, dict(inputs), y, occupancymodel=occ)
    if occ:
        assert o_one["scale"].numel() == o_ref["scale"].numel()                 # Nsel, exact
    rep, _, rows = U.replicate(inputs)
    torch.manual_seed(11)
    mask_ref = O.get_sparsity_mask(O.create_building_score(sd, rep["input"], channels != 4, channels != 2), rep["admin_mask"],
                                   rep["census_idx"], occ)
    assert int(mask_ref.sum()) == int(o_one["mask"].sum())
    # the union of the replicas' masks is the one-pass mask, sample by sample
    union = torch.zeros_like(o_one["mask"])
    for n, b in enumerate(rows):
        union[b] |= mask_ref[n]
    assert torch.equal(union, o_one["mask"])
    assert len(g_ref) == len(g_one) == (56 if channels == 6 else 32)
    pc_err = (o_one["popcount"] - o_ref["popcount"]).abs().max().item() / max(o_ref["popcount"].abs().max().item(), 1e-30)
    l_err = abs(l_one.item() - l_ref.item()) / max(abs(l_ref.item()), 1e-30)
    worst = max((g_one[n] - g_ref[n]).abs().max().item() / max(g_ref[n].abs().max().item(), 1e-30) for n in g_ref)
    # popdensemap: the replicas' maps have disjoint supports and add up to the one-pass map
    total = torch.zeros_like(o_one["popdensemap"])
    for n, b in enumerate(rows):
        total[b] += o_ref["popdensemap"][n]
    pd_err = (total - o_one["popdensemap"]).abs().max().item() / max(total.abs().max().item(), 1e-30)
    return int(mask_ref.sum()), pc_err, l_err, worst, pd_err


@pytest.mark.parametrize("name,channels,occ", CASES, ids=[c[0] for c in CASES])
def test_one_pass_equals_the_oracle_on_the_replicated_batch(name, channels, occ):
    """B = 2, 96 x 80, units [[3, 7, 12], [5, 9]] next to unlisted neighbours and -1 padding, log_l1_loss, scale_regularization 0.01,
    lam_weak 100, golden state g1, seed 11.  Nsel and the masks exact; popcounts, loss and every gradient within 1e-5
    (test_oracle_golden's bar).

    The bar is asserted on both sides evaluated in float64, for all three cases (measured: <= 1.5e-16 / 0 / <= 1.9e-15): there it can only be met by
    equal semantics.  In fp32 it is asserted too where the oracle's own rounding allows it -- dual_occ 7e-8 / 0 / 2.4e-6, s1_only 8e-8 / 0 / 5.8e-6 --
    and printed for dual_noocc: without the occupancy product every region pixel is selected and head.4.bias's gradient is a sum of
    7,000 terms per unit that nearly cancels; the committed oracle's own fp32 result is 7.8e-5 away from its float64 evaluation on that
    tensor (the one-pass form 8.3e-5), and the two fp32 runs differ by 7.4e-5 there (every other tensor <= 5.5e-6)."""
    sd = _state(channels)
    inputs, y = U.make_case(B=2, H=96, W=80, units=((3, 7, 12), (5, 9)), channels=channels, seed=11)
    nsel, pc_err, l_err, worst, pd_err = _compare(sd, inputs, y, channels, occ)
    print(f"{name} fp32: Nsel {nsel}, popcount {pc_err:.2e}, loss {l_err:.2e}, worst gradient {worst:.2e}, popdensemap {pd_err:.2e}")
    if name != "dual_noocc":
        assert pc_err <= 1e-5 and l_err <= 1e-5 and worst <= 1e-5 and pd_err <= 1e-5
    f64 = lambda t: t.double() if torch.is_tensor(t) and t.is_floating_point() else t  # noqa: E731
    torch.set_default_dtype(torch.float64)          # (the oracle allocates its zero maps / draw weights in the default dtype)
    try:
        nsel64, pc_err, l_err, worst, pd_err = _compare({k: f64(v) for k, v in sd.items()}, {k: f64(v) for k, v in inputs.items()},
                                                         y.double(), channels, occ)
    finally:
        torch.set_default_dtype(torch.float32)
    print(f"{name} fp64: Nsel {nsel64}, popcount {pc_err:.2e}, loss {l_err:.2e}, worst gradient {worst:.2e}, popdensemap {pd_err:.2e}")
    assert nsel64 == nsel
    assert pc_err <= 1e-5 and l_err <= 1e-5 and worst <= 1e-5 and pd_err <= 1e-5


def test_sorted_order_and_slots():
    cidx = torch.tensor([[12, 3, 7], [9, 5, -1]])
    admin = torch.tensor([[[3., 7., 12., 40.], [-1., 7., 7., 3.]], [[5., 9., 9., 41.], [5., -1., 50., 9.]]])
    slot, N = U.unit_slots(admin, cidx, [3, 2])
    assert N == 5
    assert slot.tolist() == [[[1, 2, 0, -1], [-1, 2, 2, 1]], [[4, 3, 3, -1], [4, -1, -1, 3]]]
    assert U.sorted_order(cidx, [3, 2]).tolist() == [2, 0, 1, 4, 3]
    pd = torch.arange(16, dtype=torch.float32).reshape(2, 2, 4)
    assert U.unit_sums(pd, slot, N).tolist() == [2.0, 0.0 + 7.0, 1.0 + 5.0 + 6.0, 9.0 + 10.0 + 15.0, 8.0 + 12.0]
    assert U.unit_paint(torch.tensor([1., 2., 3., 4., 5.]), slot)[1].tolist() == [[5., 4., 4., 0.], [5., 0., 0., 4.]]


def test_collate_units():
    from popcorn_amd.data.collate import Population_Dataset_collate_fn
    from popcorn_amd.data.units import PAD_ID, SyntheticMultiUnitDataset, collate_units, flat_valid
    ds = SyntheticMultiUnitDataset(6, units=4, min_hw=40, max_hw=60, seed=3, ragged=True)
    items = [ds[0], ds[1], ds[3]]                                   # 1, 4 and 3 listed units
    out = collate_units(items)
    assert out["census_n"] == [1, 4, 3] and PAD_ID == -1
    assert out["census_idx"].dtype == torch.int64 and tuple(out["census_idx"].shape) == (3, 4) and tuple(out["y"].shape) == (3, 4)
    for i, it in enumerate(items):
        c = out["census_n"][i]
        assert torch.equal(out["census_idx"][i, :c], it["census_idx"]) and bool((out["census_idx"][i, c:] == -1).all())
        assert torch.equal(out["y"][i, :c], it["y"]) and bool((out["y"][i, c:] == 0).all())
        # every listed unit lies in the crop, next to unlisted neighbours; ids are non-negative and distinct
        assert all(bool((it["admin_mask"] == float(u)).any()) for u in it["census_idx"])
        assert len(set(it["admin_mask"].unique().tolist()) - set(it["census_idx"].tolist())) >= 1
        assert len(set(it["census_idx"].tolist())) == c and int(it["census_idx"].min()) >= 0
    assert torch.equal(flat_valid(out["y"], out["census_n"]), torch.cat([it["y"] for it in items]))
    H, W = max(it["S2"].shape[1] for it in items), max(it["S2"].shape[2] for it in items)
    assert tuple(out["admin_mask"].shape) == (3, H, W) and bool((out["admin_mask"][0, items[0]["S2"].shape[1]:] == -1).all())
    # a batch of 1-unit items reduces to the plain collate's tensors
    ones = [{**it, "census_idx": it["census_idx"][:1], "y": it["y"][:1]} for it in items]
    a = collate_units(ones)
    b = Population_Dataset_collate_fn([{**it, "y": it["y"][0]} for it in ones])
    assert a["census_n"] == [1, 1, 1]
    assert torch.equal(a["census_idx"][:, 0], b["census_idx"]) and torch.equal(a["y"][:, 0], b["y"])
    for k in ("S2", "S1", "admin_mask", "season", "data_hw"):
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        collate_units([{**items[0], "y": torch.zeros(2)}])


def test_train_parser_units_flag():
    from popcorn_amd.cli import train_parser
    assert train_parser().parse_args([]).units_per_crop == 0
    assert train_parser().parse_args(["--units_per_crop", "4"]).units_per_crop == 4
