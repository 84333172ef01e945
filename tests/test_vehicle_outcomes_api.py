"""CPU-side checks of the per-vehicle outcome boundary: the ctypes bindings of vds_vehicle_outcomes_device,
vds_read_vehicle_outcomes and vds_run_hooked_vehicle_outcomes, the header's declarations, the Python surface that goes with them,
and that a closed handle and bad arguments are refused without touching a GPU (tests/test_abi_symbols.py checks that header,
library and bindings agree on the symbols themselves)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

NEW = ("vds_vehicle_outcomes_device", "vds_read_vehicle_outcomes", "vds_run_hooked_vehicle_outcomes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_three_symbols_are_declared_exported_and_bound():
    from vehicles_dispatch_simulator_amd import _lib
    assert _lib.SYMBOLS["vds_vehicle_outcomes_device"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)])
    assert _lib.SYMBOLS["vds_read_vehicle_outcomes"] == (C.c_int, [C.c_void_p] * 5)
    assert _lib.SYMBOLS["vds_run_hooked_vehicle_outcomes"] == (C.c_int, [C.c_void_p, C.c_int32])
    header = open(os.path.join(ROOT, "include", "vds.h")).read()
    assert re.search(r"^int vds_vehicle_outcomes_device\(vds_handle \*h, void \*\*dev_ptr\);", header, re.M)
    assert re.search(r"^int vds_read_vehicle_outcomes\(vds_handle \*h, int32_t \*order, int32_t \*wait, int32_t \*value, int32_t \*pickup\);", header, re.M)
    assert re.search(r"^int vds_run_hooked_vehicle_outcomes\(vds_handle \*h, int32_t on\);", header, re.M)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    # a null handle is refused without touching a device
    p = C.c_void_p()
    assert lib.vds_vehicle_outcomes_device(None, C.byref(p)) == -1 and not p.value
    assert lib.vds_read_vehicle_outcomes(None, None, None, None, None) == -1
    assert lib.vds_run_hooked_vehicle_outcomes(None, 1) == -1


def test_python_surface_and_defaults_keep_todays_behaviour():
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, env
    assert env.VEHICLE_OUTCOME_NAMES == ("order", "wait", "value", "pickup")
    sig = inspect.signature(BatchedDispatchEnv.run_hooked)
    assert sig.parameters["vehicle_outcomes"].default is False
    for name in ("vehicle_outcomes_device_ptr", "vehicle_outcomes_torch", "vehicle_outcomes"):
        assert list(inspect.signature(getattr(BatchedDispatchEnv, name)).parameters) == ["self"], name


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
    for call in (e.vehicle_outcomes_device_ptr, e.vehicle_outcomes, e.vehicle_outcomes_torch):
        with pytest.raises(Exception, match="libvds error -1"):
            call()
    assert e._lib.vds_run_hooked_vehicle_outcomes(e._h, 1) == -1          # the switch itself refuses the closed handle
    # the other arguments of run_hooked are checked before any entry point is called
    with pytest.raises(Exception, match=r"\[R, K, 3\]"):
        e.run_hooked(1, actions=np.zeros((3, 2), np.int32), vehicle_outcomes=True)
    e.close()          # (a second close of a null handle does nothing)


class RecordingLib:
    """Stands in for the library: every entry point returns VDS_OK and is written down with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[1:]))
            return 0
        return fn


def test_run_hooked_drives_the_switch_before_the_day_and_switches_it_off_again():
    e = closed_env()
    e._lib = RecordingLib()
    e.run_hooked(3, vehicle_outcomes=True)
    names = [n for n, _ in e._lib.calls]
    assert ("vds_run_hooked_vehicle_outcomes", (1,)) in e._lib.calls
    assert names.index("vds_run_hooked_vehicle_outcomes") < names.index("vds_run_hooked") and names[-1] == "vds_run_hooked"
    e._lib.calls.clear()
    e.run_hooked(3)                                     # a call without it: off again (the switch is sticky in the library)
    assert ("vds_run_hooked_vehicle_outcomes", (0,)) in e._lib.calls and names[-1] == "vds_run_hooked"
    for flag in (1, "yes", np.bool_(True)):
        e._lib.calls.clear()
        e.run_hooked(1, vehicle_outcomes=flag)
        assert ("vds_run_hooked_vehicle_outcomes", (1,)) in e._lib.calls, flag
