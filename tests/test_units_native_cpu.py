"""Multi-unit census supervision in the native step executor, the parts that need no GPU: the C ABI additions (pc_unit_layout,
pc_unit_popcount_loss, pc_train_step_units, pc_step_units), their argument checks -- every one of which returns before anything touches a
device -- and the opt-in flags of the trainer and of run_train.py."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW = ("pc_unit_layout", "pc_unit_popcount_loss", "pc_train_step_units")


def test_new_symbols_are_declared_exported_and_bound():
    from popcorn_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "popcorn_hip.h")).read()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr), name
    assert "typedef struct pc_step_units {" in hdr
    lib = L.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name            # bound with a signature, not called through the int default
    assert lib.pc_abi_version() == L.PC_ABI_VERSION == 10               # additive: no version bump
    # the caps of the header, in the binding
    assert int(re.search(r"#define PC_UNIT_LAYOUT_MAX_K (\d+)", hdr).group(1)) == L.PC_UNIT_LAYOUT_MAX_K == 1024
    assert int(re.search(r"#define PC_UNIT_LAYOUT_MAX_B (\d+)", hdr).group(1)) == L.PC_UNIT_LAYOUT_MAX_B >= 64


def test_struct_sizes_agree_with_pc_sizeof():
    from popcorn_amd import _lib as L
    lib = L.lib()
    assert C.sizeof(L.PcStepUnits) == lib.pc_sizeof(8) == 48
    # the layouts the executor already had did not change
    assert C.sizeof(L.PcStepPlan) == lib.pc_sizeof(6) and C.sizeof(L.PcStepIo) == lib.pc_sizeof(7)
    assert lib.pc_sizeof(9) == -1
    f = dict((n, getattr(L.PcStepUnits, n).offset) for n, _ in L.PcStepUnits._fields_)
    assert f == {"census_idx": 0, "y": 8, "census_n": 16, "K": 24, "N": 28, "off_slot": 32, "off_popcount": 40}


def _fake(n=64):
    """A 16-byte aligned host buffer standing in for a device pointer: the checks under test return before any dereference."""
    buf = C.create_string_buffer(n + 16)
    return buf, C.c_void_p((C.addressof(buf) + 15) & ~15)


def test_unit_layout_argument_checks():
    from popcorn_amd import _lib as L
    lib = L.lib()
    keep, p = _fake()
    n3 = (C.c_int32 * 3)(2, 1, 2)
    null = C.c_void_p(0)
    none_n = C.POINTER(C.c_int32)()
    args = lambda **kw: [kw.get("cidx", p), kw.get("y", p), kw.get("n", n3), kw.get("B", 3), kw.get("K", 2), kw.get("units", p),  # noqa: E731
                         kw.get("off", p), kw.get("ys", p), kw.get("dest", p), kw.get("ws", p), null]
    for bad in ({"cidx": null}, {"y": null}, {"n": none_n}, {"units": null}, {"off": null}, {"ys": null}, {"dest": null}, {"B": 0},
                {"K": 0}, {"K": 1}, {"n": (C.c_int32 * 3)(2, 0, 2)}, {"n": (C.c_int32 * 3)(2, 3, 2)},
                {"ws": C.c_void_p(p.value + 4)}, {"cidx": C.c_void_p(p.value + 4)}):
        assert lib.pc_unit_layout(*args(**bad)) == L.PC_EINVAL, bad
    big = (C.c_int32 * 300)(*([1] * 300))
    assert lib.pc_unit_layout(*args(K=1025)) == L.PC_ENOTSUP
    assert lib.pc_unit_layout(*args(B=L.PC_UNIT_LAYOUT_MAX_B + 1, n=big)) == L.PC_ENOTSUP


def test_unit_popcount_loss_argument_checks():
    from popcorn_amd import _lib as L
    lib = L.lib()
    keep, p = _fake()
    null = C.c_void_p(0)
    lam = (C.c_float * 4)(0, 1, 0, 0)
    names = ("popdense", "slot", "unit_off", "dest", "y_sorted", "ws", "pc_sorted", "pc_caller", "stats")
    outs = ("loss_out", "g_popcount", "g_scale_const")

    def call(**kw):
        a = [kw.get(n, p) for n in names] + [kw.get("lam", lam), 0.01, 100.0, kw.get("B", 2), kw.get("H", 8), kw.get("W", 8), kw.get("N", 3)]
        return lib.pc_unit_popcount_loss(*a, *[kw.get(n, p) for n in outs], null)
    for bad in ({"popdense": null}, {"slot": null}, {"y_sorted": null}, {"ws": null}, {"pc_sorted": null}, {"loss_out": null},
                {"g_popcount": null}, {"g_scale_const": null}, {"lam": C.POINTER(C.c_float)()}, {"dest": null}, {"B": 0}, {"H": 0}, {"W": 0},
                {"N": 0}, {"H": 1 << 14, "W": 1 << 13}, {"ws": C.c_void_p(p.value + 8)}):
        assert call(**bad) == L.PC_EINVAL, bad


def test_train_step_units_argument_checks():
    """NULL handle / io / lists and out-of-range counts: PC_EINVAL; K or B beyond the caps and data parallelism: PC_ENOTSUP -- all decided
    before the handle is looked at (the 'handle' here is a zeroed host buffer)."""
    from popcorn_amd import _lib as L
    lib = L.lib()
    keep, p = _fake()
    handle = C.create_string_buffer(1 << 16)
    h = C.c_void_p(C.addressof(handle))

    def io_units(B=2, K=3, counts=(3, 2), N=None, dp=0):
        io, u = L.PcStepIo(), L.PcStepUnits()
        io.B, io.H, io.W, io.dp = B, 32, 32, dp
        u._counts = (C.c_int32 * len(counts))(*counts)
        u.census_idx, u.y, u.census_n, u.K, u.N = p.value, p.value, u._counts, K, sum(counts) if N is None else N
        return io, u
    full = L.PC_STEP_FWD | L.PC_STEP_BWD | L.PC_STEP_UPD
    io, u = io_units()
    assert lib.pc_train_step_units(None, C.byref(io), C.byref(u), full, None) == L.PC_EINVAL
    assert lib.pc_train_step_units(h, None, C.byref(u), full, None) == L.PC_EINVAL
    assert lib.pc_train_step_units(h, C.byref(io), None, full, None) == L.PC_EINVAL
    for field in ("census_idx", "y"):
        io, u = io_units()
        setattr(u, field, None)
        assert lib.pc_train_step_units(h, C.byref(io), C.byref(u), full, None) == L.PC_EINVAL, field
    io, u = io_units()
    u.census_n = C.POINTER(C.c_int32)()
    assert lib.pc_train_step_units(h, C.byref(io), C.byref(u), full, None) == L.PC_EINVAL
    for kw in ({"K": 0}, {"counts": (3, 0)}, {"counts": (4, 1)}, {"N": 6}, {"N": 0}, {"B": 0}):
        io, u = io_units(**kw)
        assert lib.pc_train_step_units(h, C.byref(io), C.byref(u), full, None) == L.PC_EINVAL, kw
    for kw in ({"K": 1025, "counts": (1025, 1)}, {"dp": 1}, {"B": L.PC_UNIT_LAYOUT_MAX_B + 1, "counts": (1,) * (L.PC_UNIT_LAYOUT_MAX_B + 1)}):
        io, u = io_units(**kw)
        assert lib.pc_train_step_units(h, C.byref(io), C.byref(u), full, None) == L.PC_ENOTSUP, kw
    # the one-unit entry keeps its own NULL check
    assert lib.pc_train_step(None, C.byref(io), full, None) == L.PC_EINVAL


def test_native_units_is_opt_in():
    from popcorn_amd.cli import train_parser
    from popcorn_amd.train import FusedTrainStep
    assert inspect.signature(FusedTrainStep.__init__).parameters["native_units"].default is False
    assert train_parser().parse_args([]).native_units is False
    assert train_parser().parse_args(["--units_per_crop", "4", "--native_units"]).native_units is True
