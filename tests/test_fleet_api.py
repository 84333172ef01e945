"""CPU-side checks of the fleet-size boundary: the ctypes bindings of vds_set_fleet, vds_get_fleet and vds_reset_device, the header's
declarations and what it pins, the Python surface that goes with them, and that a closed handle and bad arguments are refused
without touching a GPU (tests/test_abi_symbols.py checks that header, library and bindings agree on the symbols themselves)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

NEW = ("vds_set_fleet", "vds_get_fleet", "vds_reset_device")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_three_symbols_are_declared_exported_and_bound():
    from vehicles_dispatch_simulator_amd import _lib
    for name in NEW:
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, C.c_void_p]), name
    header = open(os.path.join(ROOT, "include", "vds.h")).read()
    assert re.search(r"^int vds_set_fleet\(vds_handle \*h, const int32_t \*fleet\);", header, re.M)
    assert re.search(r"^int vds_get_fleet\(const vds_handle \*h, int32_t \*fleet\);", header, re.M)
    assert re.search(r"^int vds_reset_device\(vds_handle \*h, const void \*dev_veh_init_node\);", header, re.M)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    # a null handle is refused without touching a device
    f = np.zeros(2, dtype=np.int32)
    assert lib.vds_set_fleet(None, f.ctypes.data_as(C.c_void_p)) == -1 and lib.vds_set_fleet(None, None) == -1
    assert lib.vds_get_fleet(None, f.ctypes.data_as(C.c_void_p)) == -1
    assert lib.vds_reset_device(None, None) == -1


def test_the_header_pins_the_semantics():
    header = open(os.path.join(ROOT, "include", "vds.h")).read()
    text = " ".join(re.sub(r"\n \*", " ", header).split())          # (comment lines joined)
    for piece in (":101", ":347", ":249-258", "Simulation(VehiclesNumber = fleet[r])", "0 <= fleet[r] <= V",
                  "vds_reset_again right behind it is VDS_EINVAL", "vds_get_fleet keeps reporting the parameter",
                  "a vehicle beyond the replica's fleet", "never looked at"):
        assert piece in text, piece
    assert "cannot happen" not in header


def test_the_kernel_parameter_is_not_part_of_static():
    """One extra kernel parameter, so that the argument block of every tick kernel is what it was; one device function."""
    csrc = os.path.join(ROOT, "vehicles_dispatch_simulator_amd", "csrc")
    dev = open(os.path.join(csrc, "vds_device.h")).read()
    assert "fleet" not in dev
    launch = open(os.path.join(csrc, "vds_launch.h")).read()
    assert len(re.findall(r"int fleet_size\(", launch)) == 1
    tick = open(os.path.join(csrc, "vds_tick.hip")).read()
    rnd = open(os.path.join(csrc, "vds_random.hip")).read()
    for k in ("k_reset", "k_reset_fast", "k_reset_staged"):
        assert re.search(r"void %s\(Static S, State D, const int \*veh_node, const int \*fleet\)" % k, tick), k
        assert len(re.findall(r"void %s\(" % k, tick)) == 1, k          # no second copy of a kernel body
    assert tick.count("fleet_size(fleet, ext, S.V)") == 3
    assert rnd.count("fleet_size(fleet, r, V)") == 2
    # seg stays a function of V
    assert tick.count("const int seg = (((S.V + RESET_WAVES - 1) / RESET_WAVES) + WAVE - 1) / WAVE * WAVE;") == 2


def test_python_surface():
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv
    assert list(inspect.signature(BatchedDispatchEnv.set_fleet).parameters) == ["self", "fleet"]
    assert list(inspect.signature(BatchedDispatchEnv.reset_torch).parameters) == ["self", "nodes"]
    assert isinstance(BatchedDispatchEnv.fleet, property)


def closed_env():
    """An env object as ``close()`` leaves it (a null handle), made without a device."""
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, _lib
    e = BatchedDispatchEnv.__new__(BatchedDispatchEnv)
    e._lib = _lib.load()
    e._h = C.c_void_p()
    e.R, e.V, e.C, e.device = 2, 5, 3, 0
    return e


def test_a_closed_handle_and_bad_arguments_are_refused_without_a_gpu():
    e = closed_env()
    with pytest.raises(Exception, match="libvds error -1"):
        e.set_fleet([1, 2])
    with pytest.raises(Exception, match="libvds error -1"):
        e.set_fleet(None)
    with pytest.raises(Exception, match="libvds error -1"):
        e.fleet
    # the wrappers' own checks come first: nothing of the wrong size or type reaches the library
    for bad in ([1, 2, 3], [[1, 2]], [1.0, 2.0], np.zeros(1, np.int32), [1, 2**31]):
        with pytest.raises(Exception, match="set_fleet"):
            e.set_fleet(bad)
    for bad in (np.zeros((2, 5), np.int32), [[0] * 5] * 2, None):
        with pytest.raises(Exception, match="reset_torch"):
            e.reset_torch(bad)
    torch = pytest.importorskip("torch")
    for bad in (torch.zeros((2, 5), dtype=torch.int32), torch.zeros((2, 5), dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32)):
        with pytest.raises(Exception, match="reset_torch"):                # a CPU tensor, a wrong dtype, a wrong shape
            e.reset_torch(bad)
    e.close()


class RecordingLib:
    """Stands in for the library: every entry point returns VDS_OK and is written down with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[1:]))
            return 0
        return fn


def test_set_fleet_hands_the_library_int32_in_the_callers_order():
    e = closed_env()
    seen = []

    class Lib(RecordingLib):
        def vds_set_fleet(self, h, p):            # (the array lives only for the call: read it here)
            seen.append(None if p is None else np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(2,)).tolist())
            return 0

    e._lib = Lib()
    e.set_fleet(np.array([5, 0], dtype=np.int64))
    e.set_fleet(None)
    assert seen == [[5, 0], None]
