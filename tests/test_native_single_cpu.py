"""Single-modality models in the native step executor, the parts that need no GPU: which steps the trainer routes to it (``_native_ok``),
how a one-stream plan is filled (``fill_step_net``), the refusals of ``run_train.py --native_single`` and the keys of fixture g13."""
import ctypes as C
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")


# ---- routing ---------------------------------------------------------------------------------------------------------------------------
def _ok(S1, S2, single, precision="fp32", occ=True, layer=False, units=False, multi=False, given=False):
    from popcorn_amd.train import FusedTrainStep
    model = SimpleNamespace(precision=precision, S1=S1, S2=S2, occupancymodel=occ, sentinelbuildings=not given)
    me = SimpleNamespace(model=model, native_single=single, native_layer=layer, native_units=units, device_units=False)
    sample = {"census_idx": torch.zeros((2, 3) if multi else (2,), dtype=torch.int64)}
    if given:
        sample["building_counts"] = torch.zeros(2, 1, 4, 4)
    return FusedTrainStep._native_ok(me, sample)


def test_native_ok_truth_table():
    for S1, S2 in ((True, False), (False, True)):
        assert _ok(S1, S2, single=False) is False                       # opt-in
        assert _ok(S1, S2, single=True) is True
        assert _ok(S1, S2, single=True, precision="bf16") is False     # the executor is fp32
        # the other opt-ins keep their meaning for such a model
        assert _ok(S1, S2, single=True, occ=False) is False and _ok(S1, S2, single=True, occ=False, layer=True) is True
        assert _ok(S1, S2, single=True, multi=True) is False and _ok(S1, S2, single=True, multi=True, units=True) is True
        assert _ok(S1, S2, single=True, given=True) is False and _ok(S1, S2, single=True, given=True, layer=True) is True
    # a dual-stream model never asked and is not asked now
    assert _ok(True, True, single=False) is True and _ok(True, True, single=True) is True
    assert _ok(True, True, single=True, precision="bf16") is False


def test_an_engine_switch_off_its_default_keeps_the_per_launch_engine(monkeypatch):
    from popcorn_amd import engine as E
    from popcorn_amd import train as T
    assert _ok(True, False, single=True) is True
    monkeypatch.setattr(E, "COMPOSED_UP", False)
    assert _ok(True, False, single=True) is False
    monkeypatch.undo()
    monkeypatch.setattr(T, "NATIVE_STEP", False)
    assert _ok(True, False, single=True) is False


def test_the_switch_is_new_and_off_by_default():
    from popcorn_amd.cli import train_parser
    from popcorn_amd.train import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["native_single"].default is False
    assert train_parser().parse_args([]).native_single is False
    assert train_parser().parse_args(["-S1", "--native_single"]).native_single is True


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def _cpu_engine(net, streams, chmaps):
    """A UNetEngine over host tensors: the constructor's last statement refuses them, after everything the plan reads has been set."""
    from popcorn_amd import _lib as L
    from popcorn_amd import engine as E
    table = dict(net.named_parameters())
    table.update(dict(net.named_buffers()))
    eng = object.__new__(E.UNetEngine)
    with pytest.raises(L.PopcornHipError):
        E.UNetEngine.__init__(eng, table, streams, chmaps)
    return eng, table


def _zero(struct):
    return bytes(struct) == bytes(C.sizeof(struct))


@pytest.mark.parametrize("ic", [2, 4, 6])
def test_fill_step_net(ic):
    from popcorn_amd import _lib as L
    from popcorn_amd import engine as E
    from popcorn_amd import train as T
    from popcorn_amd.model import POPCORN
    torch.manual_seed(1600)
    m = POPCORN(input_channels=ic, occupancymodel=True, pretrained=True, biasinit=0.9407, sentinelbuildings=True)
    chmaps = None if ic == 6 else {"sar_stream": (0, 1, 0, 0), "optical_stream": (2, 1, 0, 3)}
    names, params = m.trainable()
    grads = {n: torch.zeros_like(p) for n, p in zip(names, params)}
    plan, keep = L.PcStepPlan(), []
    eng_u, tab_u = _cpu_engine(m.unetmodel, m._streams, chmaps)
    eng_b, tab_b = _cpu_engine(m.building_extractor, m._streams, chmaps)
    T.fill_step_net(plan.unet, eng_u, grads, "unetmodel.", keep)
    T.fill_step_net(plan.extractor, eng_b, None, None, keep)
    present = {6: (0, 1), 2: (0,), 4: (1,)}[ic]
    for net, tab, trainable in ((plan.unet, tab_u, True), (plan.extractor, tab_b, False)):
        for s, (sname, chmap6, cin, f0) in enumerate(E.STREAMS):
            st = net.s[s]
            if s not in present:
                assert _zero(st), (ic, s)                           # the absent stream: all zero, in BOTH networks
                continue
            assert (st.cin, st.feat_c0) == (cin, f0)
            want = chmap6 if ic == 6 else chmaps[sname]
            assert [st.chan[c] for c in range(4)] == list(want)
            assert st.w[0] == tab[f"{sname}.{E.CONVS['inc1'][0]}.weight"].data_ptr()
            assert st.w[9] == tab[f"{sname}.{E.CONVS['up1b'][0]}.weight"].data_ptr()
            assert st.wt[1] == tab[f"{sname}.{E.CONVTS['up1t']}.weight"].data_ptr()
            if trainable:
                assert st.dw[0] == grads[f"unetmodel.{sname}.{E.CONVS['inc1'][0]}.weight"].data_ptr()
                assert st.dbt[0] == grads[f"unetmodel.{sname}.{E.CONVTS['up2t']}.bias"].data_ptr()
            else:
                assert all(st.dw[i] in (None, 0) for i in range(10)) and all(st.dwt[i] in (None, 0) for i in range(2))
        # the building logit: fusion_out_conv, or the present stream's own out conv (8 weights, 1 bias)
        pre = {6: "fusion_out_conv", 2: "sar_out_conv", 4: "optical_out_conv"}[ic]
        assert net.fusion_w == tab[pre + ".conv.weight"].data_ptr() and net.fusion_b == tab[pre + ".conv.bias"].data_ptr()
        assert tab[pre + ".conv.weight"].numel() == (16 if ic == 6 else 8)
    # the head's first layer and its gradient are the parameter's own 64 x ic-stream tensors (the executor embeds them, not torch)
    assert tuple(m.head[0].weight.shape) == (64, 16 if ic == 6 else 8, 1, 1) and grads["head.0.weight"].shape == m.head[0].weight.shape


def test_abi_did_not_move():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10
    assert C.sizeof(L.PcStepPlan) == lib.pc_sizeof(6) == 3704 and C.sizeof(L.PcStepIo) == lib.pc_sizeof(7) == 168


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,why", [
    (["--native_single"], "exactly one of"),
    (["-S1", "-S2", "-NIR", "--native_single"], "exactly one of"),
    (["-S1", "--precision", "bf16", "--native_single"], "fp32 only"),
    (["-S2", "-NIR", "--torch_optimizer", "--native_single"], "--torch_optimizer"),
])
def test_run_train_refuses_native_single_where_it_cannot_apply(argv, why):
    from popcorn_amd.cli import check_native_single, train_parser
    with pytest.raises(SystemExit) as e:
        check_native_single(train_parser().parse_args(argv))
    assert why in str(e.value)


def test_trainer_raises_the_refusal_before_anything_else(tmp_path):
    from popcorn_amd.cli import Trainer, train_parser
    with pytest.raises(SystemExit) as e:
        Trainer(train_parser().parse_args(["--native_single", "--save_dir", str(tmp_path)]))
    assert "--native_single" in str(e.value) and not os.listdir(tmp_path)


def test_check_native_single_accepts_the_recipes():
    from popcorn_amd.cli import check_native_single, train_parser
    for argv in (["-S1", "--native_single"], ["-S2", "-NIR", "--native_single"], ["-S1", "-S2"], []):
        check_native_single(train_parser().parse_args(argv))


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
def test_g13_has_the_keys_of_g8_plus_the_dense_ones():
    g8 = np.load(os.path.join(G, "g8_single_modality.npz"))
    g13 = np.load(os.path.join(G, "g13_single_modality_shared.npz"))
    dense = {f"ic{ic}/dense_pad0/{k}" for ic in (2, 4) for k in ("popdensemap", "scale", "building_counts")}
    assert set(g13.files) == set(g8.files) | dense
    for ic in (2, 4):
        assert g13[f"ic{ic}/input"].shape == (2, ic, 36, 36) and len(g13[f"ic{ic}/grad_names"]) == 32
        assert g13[f"ic{ic}/dense_pad0/building_counts"].shape == (2, 1, 36, 36)
        # eval / train mode share the frozen extractor: one building score
        assert np.array_equal(g13[f"ic{ic}/dense_pad0/building_counts"], g13[f"ic{ic}/building_counts"])
        assert np.isfinite(g13[f"ic{ic}/loss"]) and int((g13[f"ic{ic}/popdensemap"] != 0).sum()) == 958
    assert os.path.getsize(os.path.join(G, "g13_single_modality_shared.npz")) < (1 << 20)


def test_generator_is_a_file_of_its_own_and_names_the_shared_domain():
    src = open(os.path.join(G, "make_golden_g13.py")).read()
    assert "from make_golden import" in src and "HW = (36, 36)" in src and "g13_single_modality_shared.npz" in src
    from popcorn_amd.model.popcorn import pad_geometry
    assert pad_geometry(36, 36, False) == (14, 14, 14, 14)              # = the extractor's pad: both networks on one 64 x 64 domain
    assert pad_geometry(48, 40, False) == (8, 8, 12, 12)                # g8: two domains
