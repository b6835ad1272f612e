"""CPU: the slice stream and ring protocol of the rolling conv kernels, replayed by tools/roll_stream_model.cpp with the schedule functions the
kernels themselves call (roll_sched / roll_step / RollChunks, dffinthewild_amd/csrc/dffw_conv_roll.h).  The program is a host-only executable,
built here with AddressSanitizer and UndefinedBehaviorSanitizer; it exits non-zero at the first violated invariant."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime.h")):
            return os.path.join(d, "include")
    return None


def test_roll_stream_model(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = _rocm_include()
    assert inc, "the HIP headers (dffw_conv_roll.h includes hip_runtime.h for its host/device markers) were not found"
    exe = str(tmp_path / "roll_stream_model")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", os.path.join(ROOT, "dffinthewild_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "roll_stream_model.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "all passed" in run.stdout, run.stdout

