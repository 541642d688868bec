"""DeviceBuf (csrc/device_buf.h), the owner of every device buffer, over a malloc-backed allocator on the CPU:
tools/device_buf_host_check.cpp built as a plain host program (no sanitizer here, no GPU call) and run.  It
drives growth, failing allocations and frees, moves, swap, reset and a group regrown after a failure."""
import os
import subprocess

from conftest import ROOT
from test_kernel_resources import CSRC, HIPCC


def test_device_buf_host_check(tmp_path):
    exe = tmp_path / "device_buf_host_check"
    rocm = os.path.dirname(os.path.dirname(HIPCC))
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tools", "device_buf_host_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "DeviceBuf host checks: ok"
