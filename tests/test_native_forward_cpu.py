"""The native forward executor (pc_forward) without a GPU: the exported symbols and struct size, the ABI version, the routing predicate of
``POPCORN.forward`` as a table, and the flag of both command-line tools."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch


def test_library_exports_pc_forward_and_the_struct_size():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert hasattr(lib, "pc_forward") and hasattr(lib, "pc_sizeof_fwd_io")
    assert lib.pc_sizeof_fwd_io() == C.sizeof(L.PcFwdIo) == 120
    # the nine indices the loader has always compared stay what they were; the new struct has no index
    assert lib.pc_sizeof(8) == C.sizeof(L.PcStepUnits) and lib.pc_sizeof(7) == C.sizeof(L.PcStepIo) and lib.pc_sizeof(9) == -1


def test_abi_version_is_still_10():
    from popcorn_amd import _lib as L
    assert L.lib().pc_abi_version() == L.PC_ABI_VERSION == 10


def test_struct_field_offsets():
    from popcorn_amd import _lib as L
    f = L.PcFwdIo
    assert (f.B.offset, f.data.offset, f.craw.offset, f.admin_mask.offset, f.arena.offset, f.arena_needed.offset, f.off_popcount.offset,
            f.off_building.offset, f.launches.offset) == (0, 16, 32, 40, 56, 72, 80, 104, 112)


def _model(**kw):
    d = dict(native_forward=True, precision="fp32", S1=True, S2=True, sentinelbuildings=True, occupancymodel=True)
    d.update(kw)
    return SimpleNamespace(**d)


def _inputs(**kw):
    d = {"input": torch.zeros(2, 6, 8, 8), "admin_mask": torch.zeros(2, 8, 8), "census_idx": torch.zeros(2, dtype=torch.int64)}
    d.update(kw)
    return d


def _route(model=None, inputs=None, need_grad=False, sparse=False, padding=False, switches=True):
    from popcorn_amd import infer
    return infer.route_ok(model or _model(), inputs or _inputs(), need_grad, sparse, padding, switches_default=switches)


def test_the_route_is_taken_when_every_condition_holds():
    assert _route() is True
    assert _route(inputs={"input": torch.zeros(1, 6, 8, 8)}) is True                  # census_idx absent
    assert _route(inputs=_inputs(building_counts=torch.zeros(2, 1, 8, 8))) is True    # a layer does not exclude


EXCLUDING = {
    "flag off": dict(model=_model(native_forward=False)),
    "need_grad": dict(need_grad=True),
    "sparse": dict(sparse=True),
    "padding": dict(padding=True),
    "bf16": dict(model=_model(precision="bf16")),
    "S1 only": dict(model=_model(S2=False)),
    "S2 only": dict(model=_model(S1=False)),
    "input not fp32": dict(inputs=_inputs(input=torch.zeros(2, 6, 8, 8, dtype=torch.float64))),
    "input fp16": dict(inputs=_inputs(input=torch.zeros(2, 6, 8, 8, dtype=torch.float16))),
    "input not contiguous": dict(inputs=_inputs(input=torch.zeros(2, 6, 8, 16)[..., ::2])),
    "input not 6 channels": dict(inputs=_inputs(input=torch.zeros(2, 4, 8, 8))),
    "input not 4-D": dict(inputs=_inputs(input=torch.zeros(6, 8, 8))),
    "2-D census_idx": dict(inputs=_inputs(census_idx=torch.zeros(2, 3, dtype=torch.int64))),
    "engine switch off": dict(switches=False),
}


@pytest.mark.parametrize("name", list(EXCLUDING))
def test_each_excluding_condition_alone_declines(name):
    assert _route(**EXCLUDING[name]) is False


def test_engine_switches_are_the_training_executors_predicate(monkeypatch):
    from popcorn_amd import engine as E, infer, train as T
    assert infer.engine_switches_default() is True
    for mod, attr in ((E, "PADDED_INPUT"), (E, "COMPOSED_UP"), (E, "FUSED_LEVEL2"), (E, "FUSED_CONV_BWD"), (T, "DEFER_HEAD_REDUCE")):
        monkeypatch.setattr(mod, attr, False)
        assert infer.engine_switches_default() is False and _route(switches=None) is False, attr
        monkeypatch.setattr(mod, attr, True)
    assert _route(switches=None) is True


def test_both_command_line_tools_parse_the_flag():
    from popcorn_amd.cli import eval_parser, train_parser
    for parser in (train_parser, eval_parser):
        assert parser().parse_args([]).native_forward is False
        assert parser().parse_args(["--native_forward"]).native_forward is True
    # accepted together with what the executor declines: the run then never takes it
    assert train_parser().parse_args(["--native_forward", "--precision", "bf16"]).native_forward is True
    assert eval_parser().parse_args(["--native_forward", "-S1"]).native_forward is True


def test_model_defaults():
    from popcorn_amd.model import POPCORN
    m = POPCORN(input_channels=6, occupancymodel=True, pretrained=True, sentinelbuildings=True)
    assert m.native_forward is False and m.native_forwards == 0
