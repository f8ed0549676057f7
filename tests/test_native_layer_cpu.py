"""The native step executor on a shipped building layer, the parts that need no GPU: the two C ABI additions (pc_train_step_layer,
pc_train_step_units_layer), their argument checks -- every one of which returns before the handle is looked at -- and the opt-in flags
of the trainer and of run_train.py."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW = ("pc_train_step_layer", "pc_train_step_units_layer")


def test_new_symbols_are_declared_exported_and_bound():
    from popcorn_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "popcorn_hip.h")).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name            # bound with a signature, not called through the int default
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10               # additive: no version bump
    assert int(re.search(r"#define PC_ABI_VERSION (\d+)", hdr).group(1)) == 10


def test_step_struct_sizes_did_not_change():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert C.sizeof(L.PcStepPlan) == lib.pc_sizeof(6) and C.sizeof(L.PcStepIo) == lib.pc_sizeof(7)
    assert C.sizeof(L.PcStepUnits) == lib.pc_sizeof(8) == 48
    assert lib.pc_sizeof(9) == -1
    # the sizes of the commit before the layer entry points
    assert C.sizeof(L.PcStepIo) == 168 and C.sizeof(L.PcStepPlan) == 3704
    assert L.PcStepIo.off_building.offset == 152


def _fake(n=64):
    """A 16-byte aligned host buffer standing in for a device pointer: the checks under test return before any dereference."""
    buf = C.create_string_buffer(n + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def _io_units(p, B=2, K=3, counts=(3, 2)):
    from popcorn_amd import _lib as L
    io, u = L.PcStepIo(), L.PcStepUnits()
    io.B, io.H, io.W = B, 32, 32
    u._counts = (C.c_int32 * len(counts))(*counts)
    u.census_idx, u.y, u.census_n, u.K, u.N = p.value, p.value, u._counts, K, sum(counts)
    return io, u


def test_null_handle_or_io_is_einval():
    from popcorn_amd import _lib as L
    lib = L.lib()
    keep, p = _fake()
    handle = C.create_string_buffer(1 << 16)
    h = C.c_void_p(C.addressof(handle))
    full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    io, u = _io_units(p)
    for layer in (None, p):
        assert lib.pc_train_step_layer(None, C.byref(io), layer, full, None) == L.PC_EINVAL
        assert lib.pc_train_step_layer(h, None, layer, full, None) == L.PC_EINVAL
        assert lib.pc_train_step_units_layer(None, C.byref(io), C.byref(u), layer, full, None) == L.PC_EINVAL
        assert lib.pc_train_step_units_layer(h, None, C.byref(u), layer, full, None) == L.PC_EINVAL
        assert lib.pc_train_step_units_layer(h, C.byref(io), None, layer, full, None) == L.PC_EINVAL


def test_a_misaligned_layer_is_einval_before_the_handle_is_looked_at():
    """(the 'handle' is a zeroed host buffer, the io otherwise complete: only the layer's address decides)"""
    from popcorn_amd import _lib as L
    lib = L.lib()
    keep, p = _fake()
    handle = C.create_string_buffer(1 << 16)
    h = C.c_void_p(C.addressof(handle))
    full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    for off in (1, 2, 3, 5, 6, 7):
        bad = C.c_void_p(p.value + off)
        for phases in (full, L.PC_STEP_FWD, L.PC_STEP_BWD, L.PC_STEP_UPD):
            io, u = _io_units(p)
            io.data = io.admin_mask = io.census_idx = io.y = io.sel = p.value
            assert lib.pc_train_step_layer(h, C.byref(io), bad, phases, None) == L.PC_EINVAL, (off, phases)
            assert lib.pc_train_step_units_layer(h, C.byref(io), C.byref(u), bad, phases, None) == L.PC_EINVAL, (off, phases)
    # the units form keeps its own refusals with an aligned layer
    io, u = _io_units(p)
    io.dp = 1
    assert lib.pc_train_step_units_layer(h, C.byref(io), C.byref(u), p, full, None) == L.PC_ENOTSUP
    io, u = _io_units(p, counts=(4, 1))
    assert lib.pc_train_step_units_layer(h, C.byref(io), C.byref(u), p, full, None) == L.PC_EINVAL


def test_native_layer_is_opt_in():
    from popcorn_amd.cli import train_parser
    from popcorn_amd.train import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["native_layer"].default is False
    assert train_parser().parse_args([]).native_layer is False
    assert train_parser().parse_args(["--building_layer", "--native_layer"]).native_layer is True
    # accepted silently where it changes nothing
    assert train_parser().parse_args(["-occmodel", "-senbuilds", "--native_layer"]).native_layer is True


def test_run_train_help_lists_the_flag():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "run_train.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--native_layer" in out.stdout and "pc_train_step_layer" in out.stdout
