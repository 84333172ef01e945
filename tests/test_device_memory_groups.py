"""The device-memory groups of csrc/vds_mem.h on the CPU: ``mem_check.cpp`` replays the recycling rule of the order tables, the
release of one block, clearing twice and a failing allocation over malloc / free, as a stand-alone program under the address /
undefined-behaviour sanitizer (a block that leaks, is freed twice or is used after it went back ends the program)."""
import os
import shutil
import subprocess

import pytest

from vehicles_dispatch_simulator_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="needs hipcc")
def test_mem_check_builds_and_runs_clean(tmp_path):
    prog = os.path.join(str(tmp_path), "mem_check_asan")
    out = subprocess.run(["make", "-s", "-C", _lib.CSRC, prog, "CHECKDIR=%s" % tmp_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    out = subprocess.run([prog], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"mem_check: ok" in out.stdout, out.stdout.decode()[-3000:]
