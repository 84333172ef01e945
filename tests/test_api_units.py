"""The C ABI as three lists that have to agree - the declarations of ``include/vds.h`` / ``include/vds_debug.h``, the exports of the
built ``libvds.so`` and the ctypes tables of ``_lib.py`` -, the layout of the host units in the Makefile, and what every entry point
answers to a NULL handle.  No GPU: a NULL handle is refused before any device call (on a machine without a device such a call would
make the answer VDS_EHIP, so VDS_EINVAL also says that none was made)."""
import ctypes as C
import glob
import os
import re

import pytest

from vehicles_dispatch_simulator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VDS_EINVAL = -1

DECL = re.compile(r"^(int|int32_t|const char \*|void) ?(vds_\w+)\(([^;]*?)\);", re.M | re.S)

# handle-first entry points that do not answer VDS_EINVAL to a NULL handle, by name, and why
NOT_EINVAL = {
    "vds_destroy": "destroying nothing is VDS_OK (vds.h), like free(NULL)",
    "vds_get_run_groups": "returns a group count, not a status: 1 without a handle",
    "vds_load_order_days": "dereferences the handle behind its own refusal (the parked order tables are dropped whatever the loader "
                           "answered): a NULL handle faults, before this layout and after it - left as it is here, to be fixed on its own",
}


def declared():
    """name -> (return type, parameter list) of every function the two headers declare"""
    out = {}
    for hdr in ("vds.h", "vds_debug.h"):
        for m in DECL.finditer(open(os.path.join(ROOT, "include", hdr)).read()):
            out[m.group(2)] = (m.group(1), [p.strip() for p in m.group(3).split(",")])
    return out


def null_handle_sweep(lib_path, names=None):
    """name -> status of every handle-first entry point (or of ``names``) called with a NULL handle and zeros for the rest"""
    lib = C.CDLL(lib_path)
    res = {}
    for name, (ret, params) in sorted(declared().items()):
        if names is None and (ret != "int" or "vds_handle *" not in params[0] or name in NOT_EINVAL):
            continue
        if names is not None and name not in names:
            continue
        fn = getattr(lib, name)
        fn.restype = C.c_int
        # the declared types: pointers and arrays NULL, int64_t / uint64_t and int32_t zero
        fn.argtypes = [C.c_void_p if ("*" in p or "[" in p) else C.c_int64 if "int64_t" in p else C.c_int32 for p in params]
        res[name] = fn(*([None if t is C.c_void_p else 0 for t in fn.argtypes]))
    return res


@pytest.fixture(scope="module")
def lib():
    _lib.load()                        # (torch's HIP runtime first, as everywhere: _lib.load says why)
    return C.CDLL(_lib.LIB_PATH)       # a handle of our own: the argtypes set below stay out of the package's way


def test_declared_functions_are_exported(lib):
    names = declared()
    assert len(names) > 90
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, "declared in include/ but not exported by %s: %s" % (_lib.LIB_PATH, missing)


def test_ctypes_tables_name_declared_functions():
    names = declared()
    stray = [n for n in list(_lib.SYMBOLS) + list(_lib.TEST_SYMBOLS) if n not in names]
    assert not stray, "in _lib.SYMBOLS / TEST_SYMBOLS but declared in neither header: %s" % stray


def test_makefile_lists_the_host_units():
    csrc = os.path.join(ROOT, "vehicles_dispatch_simulator_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s := (.*)$" % name, mk, re.M).group(1).split()
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "vds_api*.hip")))
    assert {"vds_api.hip", "vds_api_read.hip", "vds_api_snapshot.hip", "vds_api_debug.hip"} <= set(units)
    assert [u for u in units if u not in var("HSRCS")] == []
    assert "vds_handle.h" in var("HHDRS")
    assert var("KSRCS") == ["vds_tick_dense.hip", "vds_tick.hip", "vds_dfs.hip", "vds_neighbors.hip"]


def test_null_handle_is_einval():
    _lib.load()
    res = null_handle_sweep(_lib.LIB_PATH)
    assert len(res) >= 85, sorted(res)       # (88 handle-first status functions when the units were cut, less the three above)
    wrong = {n: rc for n, rc in res.items() if rc != VDS_EINVAL}
    assert not wrong, "a NULL handle must be refused with VDS_EINVAL: %s" % wrong
