"""The hooked day's plan value of csrc/vds_hook_plan.h on the CPU: ``hook_plan_check.cpp`` compares ``HookPlan::operator==`` and
``same_shape`` with a transcription of the expressions they replaced in ``vds_run_hooked``, for every change of one and of two
fields of a call, as a stand-alone program under the address / undefined-behaviour sanitizer."""
import os
import shutil
import subprocess

import pytest

from vehicles_dispatch_simulator_amd import _lib

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="needs hipcc")
def test_hook_plan_check_builds_and_runs_clean(tmp_path):
    prog = os.path.join(str(tmp_path), "hook_plan_check_asan")
    out = subprocess.run(["make", "-s", "-C", _lib.CSRC, prog, "CHECKDIR=%s" % tmp_path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0, out.stdout.decode()[-3000:]
    out = subprocess.run([prog], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert out.returncode == 0 and b"hook_plan_check: ok" in out.stdout, out.stdout.decode()[-3000:]
