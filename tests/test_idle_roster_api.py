"""CPU-side checks of the idle-roster boundary: the ctypes bindings of vds_idle_roster_device, vds_read_idle_roster,
vds_apply_dispatch_roster_device and vds_run_hooked_roster, the header's declarations, the Python surface that goes with them, and
that a closed handle and bad arguments are refused without touching a GPU - nothing answers in the kernels' place
(tests/test_abi_symbols.py checks that header, library and bindings agree on the symbols themselves)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

NEW = ("vds_idle_roster_device", "vds_read_idle_roster", "vds_apply_dispatch_roster_device", "vds_run_hooked_roster")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_four_symbols_are_declared_exported_and_bound():
    from vehicles_dispatch_simulator_amd import _lib
    assert _lib.SYMBOLS["vds_idle_roster_device"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
    assert _lib.SYMBOLS["vds_read_idle_roster"] == (C.c_int, [C.c_void_p] * 5)
    assert _lib.SYMBOLS["vds_apply_dispatch_roster_device"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["vds_run_hooked_roster"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    header = open(os.path.join(ROOT, "include", "vds.h")).read()
    assert re.search(r"^int vds_idle_roster_device\(vds_handle \*h, void \*\*dev_planes, void \*\*dev_off\);", header, re.M)
    assert re.search(r"^int vds_read_idle_roster\(vds_handle \*h, int32_t \*veh, int32_t \*node, int32_t \*cluster, int32_t \*off\);", header, re.M)
    assert re.search(r"^int vds_apply_dispatch_roster_device\(vds_handle \*h, const void \*dev_targets\);", header, re.M)
    assert re.search(r"^int vds_run_hooked_roster\(vds_handle \*h, int32_t on, const void \*dev_targets\);", header, re.M)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    # a null handle is refused without touching a device
    p, o = C.c_void_p(), C.c_void_p()
    assert lib.vds_idle_roster_device(None, C.byref(p), C.byref(o)) == -1 and not p.value and not o.value
    assert lib.vds_read_idle_roster(None, None, None, None, None) == -1
    assert lib.vds_apply_dispatch_roster_device(None, None) == -1
    assert lib.vds_run_hooked_roster(None, 1, None) == -1


def test_the_kernel_file_is_hashed_with_the_host_sources():
    mk = open(os.path.join(ROOT, "vehicles_dispatch_simulator_amd", "csrc", "Makefile")).read()
    ksrcs = re.search(r"^KSRCS := (.*)$", mk, re.M).group(1).split()
    hsrcs = re.search(r"^HSRCS := (.*)$", mk, re.M).group(1).split()
    assert "vds_idle_roster.hip" in hsrcs and "vds_idle_roster.hip" not in ksrcs
    assert ksrcs == ["vds_tick_dense.hip", "vds_tick.hip", "vds_dfs.hip", "vds_neighbors.hip"]


def test_python_surface_and_defaults_keep_todays_behaviour():
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, env
    assert env.IDLE_ROSTER_NAMES == ("veh", "node", "cluster")
    sig = inspect.signature(BatchedDispatchEnv.run_hooked)
    assert sig.parameters["roster"].default is False and sig.parameters["roster_targets"].default is None
    for name in ("idle_roster_device_ptr", "idle_roster_torch", "idle_roster"):
        assert list(inspect.signature(getattr(BatchedDispatchEnv, name)).parameters) == ["self"], name
    assert list(inspect.signature(BatchedDispatchEnv.apply_dispatch_roster_torch).parameters) == ["self", "targets"]


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
    for call in (e.idle_roster_device_ptr, e.idle_roster, e.idle_roster_torch):
        with pytest.raises(Exception, match="libvds error -1"):
            call()
    assert e._lib.vds_run_hooked_roster(e._h, 1, None) == -1          # the switch itself refuses the closed handle
    # a tensor argument is checked before any entry point is called: nothing but a CUDA tensor of the right shape gets through
    for bad in (np.zeros((2, 5), np.int32), [[-1] * 5] * 2, None):
        with pytest.raises(Exception, match="apply_dispatch_roster_torch"):
            e.apply_dispatch_roster_torch(bad)
    with pytest.raises(Exception, match="run_hooked"):
        e.run_hooked(1, roster=True, roster_targets=np.zeros((2, 5), np.int32))
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


def test_run_hooked_touches_the_switch_only_when_asked_and_switches_it_off_again():
    e = closed_env()
    e._lib = RecordingLib()
    e.run_hooked(3)                                     # the defaults: the calls of a day before this switch existed
    names = [n for n, _ in e._lib.calls]
    assert "vds_run_hooked_roster" not in names and names[-1] == "vds_run_hooked"
    e._lib.calls.clear()
    e.run_hooked(3, roster=True)
    names = [n for n, _ in e._lib.calls]
    assert ("vds_run_hooked_roster", (1, None)) in e._lib.calls
    assert names.index("vds_run_hooked_roster") < names.index("vds_run_hooked") and names[-1] == "vds_run_hooked"
    e._lib.calls.clear()
    e.run_hooked(3)                                     # a call without it: off again (the switch is sticky in the library)
    assert ("vds_run_hooked_roster", (0, None)) in e._lib.calls
    e._lib.calls.clear()
    e.run_hooked(3)                                     # ... and then left alone
    assert "vds_run_hooked_roster" not in [n for n, _ in e._lib.calls]
