"""CPU-side checks of the per-vehicle dispatch boundary: the ctypes bindings of vds_apply_dispatch_vehicles_device and
vds_run_hooked_vehicles, the Python surface that goes with them, and - on a machine without a GPU - that nothing answers in the
kernels' place (tests/test_abi_symbols.py checks that header, library and bindings agree on the symbols themselves)."""
import ctypes as C
import inspect

import numpy as np
import pytest


def test_bindings_of_the_two_new_symbols():
    from vehicles_dispatch_simulator_amd import _lib
    assert _lib.SYMBOLS["vds_apply_dispatch_vehicles_device"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["vds_run_hooked_vehicles"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p])
    _lib.build()
    lib = _lib.load()
    for name in ("vds_apply_dispatch_vehicles_device", "vds_run_hooked_vehicles"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    # a null handle is refused without touching a device
    assert lib.vds_apply_dispatch_vehicles_device(None, None) == -1
    assert lib.vds_run_hooked_vehicles(None, 0, None) == -1


def test_python_surface_defaults_keep_todays_behaviour():
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv
    sig = inspect.signature(BatchedDispatchEnv.run_hooked)
    assert sig.parameters["vehicle_planes"].default is None and sig.parameters["vehicle_targets"].default is None
    assert list(inspect.signature(BatchedDispatchEnv.apply_dispatch_vehicles_torch).parameters) == ["self", "targets"]
    mask = BatchedDispatchEnv._vehicle_mask
    assert mask(None) == 0 and mask(0) == 0 and mask(5) == 5 and mask(np.int32(63)) == 63
    assert mask(dict(state=True, cluster=True, node=False)) == 5 and mask(("order", "state")) == 17
    assert mask(dict(state=True, node=True, cluster=True, arrive_min=True, order=True, source=True)) == 63
    for bad in (64, -1, dict(speed=True), ("state", "where")):
        with pytest.raises(Exception, match="vehicle_planes"):
            mask(bad)


def test_no_cpu_fallback_for_the_vehicle_form():
    import torch
    from vehicles_dispatch_simulator_amd import BatchedDispatchEnv
    if torch.cuda.is_available():
        return          # (a GPU is visible: tests/test_gpu_dispatch_vehicles.py runs the feature itself)
    with pytest.raises(Exception, match="no CPU fallback"):
        BatchedDispatchEnv(np.zeros((4, 4), np.int32), np.zeros(4, np.int32), np.zeros(2, np.int32), np.zeros(0, np.int32), replicas=1, vehicles=2)
