"""CPU-side checks of the per-order block's boundary: the ctypes bindings of vds_orders_device and vds_run_hooked_orders, the header's
declarations and constants, the Python surface that goes with them, and that a closed handle and bad arguments are refused without
touching a GPU (tests/test_abi_symbols.py checks that header, library and bindings agree on the symbols themselves)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

NEW = ("vds_orders_device", "vds_run_hooked_orders")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_two_symbols_are_declared_exported_and_bound():
    from vehicles_dispatch_simulator_amd import _lib
    assert _lib.SYMBOLS["vds_orders_device"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)])
    assert _lib.SYMBOLS["vds_run_hooked_orders"] == (C.c_int, [C.c_void_p, C.c_int32])
    header = open(os.path.join(ROOT, "include", "vds.h")).read()
    assert re.search(r"^int vds_orders_device\(vds_handle \*h, int32_t slot_lo, int32_t slot_hi, void \*\*dev_ptr\);", header, re.M)
    assert re.search(r"^int vds_run_hooked_orders\(vds_handle \*h, int32_t on\);", header, re.M)
    assert re.search(r"^#define VDS_ORDER_REJECTED \(-1\)", header, re.M) and re.search(r"^#define VDS_ORDER_PENDING  \(-2\)", header, re.M)
    _lib.build()
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    # a null handle is refused without touching a device
    p = C.c_void_p()
    assert lib.vds_orders_device(None, 0, 0, C.byref(p)) == -1 and not p.value
    assert lib.vds_orders_device(None, 0, 0, None) == -1
    assert lib.vds_run_hooked_orders(None, 1) == -1


def test_python_surface_and_defaults_keep_todays_behaviour():
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, env
    assert env.ORDER_REJECTED == -1 and env.ORDER_PENDING == -2
    sig = inspect.signature(BatchedDispatchEnv.run_hooked)
    assert sig.parameters["orders"].default is False
    for name in ("orders_device_ptr", "orders_torch"):
        ps = inspect.signature(getattr(BatchedDispatchEnv, name)).parameters
        assert list(ps) == ["self", "slot_lo", "slot_hi"] and ps["slot_lo"].default == 0 and ps["slot_hi"].default is None, name
    # env.orders() stays the host read it was
    assert list(inspect.signature(BatchedDispatchEnv.orders).parameters) == ["self", "r0", "nr"]


def closed_env():
    """An env object as ``close()`` leaves it (a null handle), made without a device."""
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv, _lib
    e = BatchedDispatchEnv.__new__(BatchedDispatchEnv)
    e._lib = _lib.load()
    e._h = C.c_void_p()
    e.R, e.V, e.C, e.O, e.device = 2, 5, 3, 7, 0
    return e


def test_a_closed_handle_and_bad_arguments_are_refused_without_a_gpu():
    e = closed_env()
    for call in (e.orders_device_ptr, e.orders_torch, lambda: e.orders_torch(3, 3), lambda: e.orders_device_ptr(-1), lambda: e.orders_device_ptr(4, 2)):
        with pytest.raises(Exception, match="libvds error -1"):
            call()
    assert e._lib.vds_run_hooked_orders(e._h, 1) == -1          # the switch itself refuses the closed handle
    # the other arguments of run_hooked are checked before any entry point is called
    with pytest.raises(Exception, match=r"\[R, K, 3\]"):
        e.run_hooked(1, actions=np.zeros((3, 2), np.int32), orders=True)
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


def test_run_hooked_drives_the_switch_and_the_range_arguments_reach_the_library():
    e = closed_env()
    e._lib = RecordingLib()
    e.run_hooked(3, orders=True)
    names = [n for n, _ in e._lib.calls]
    assert ("vds_run_hooked_orders", (1,)) in e._lib.calls
    assert names.index("vds_run_hooked_orders") < names.index("vds_run_hooked") and names[-1] == "vds_run_hooked"
    e._lib.calls.clear()
    e.run_hooked(3)                                     # a call without it: off again (the switch is sticky in the library)
    assert ("vds_run_hooked_orders", (0,)) in e._lib.calls
    for flag in (1, "yes", np.bool_(True)):
        e._lib.calls.clear()
        e.run_hooked(1, orders=flag)
        assert ("vds_run_hooked_orders", (1,)) in e._lib.calls, flag
    # slot_hi=None means everything: INT32_MAX
    for args, want in (((), (0, 0x7FFFFFFF)), ((5,), (5, 0x7FFFFFFF)), ((4, 4), (4, 4)), ((np.int64(2), np.int32(9)), (2, 9))):
        e._lib.calls.clear()
        e.orders_device_ptr(*args)
        (name, got), = e._lib.calls
        assert name == "vds_orders_device" and tuple(got[:2]) == want, (args, got)
