"""The host layer's owners (pypevoc_amd/csrc/pvx_mem.h) on the CPU: tests/host/mem_check.cpp exercises DevMem / PinMem against a
malloc-backed fake of the HIP allocator, built with the host compiler under AddressSanitizer and UBSan.  No GPU, no GPU library."""
import os
import subprocess

from .conftest import ROOT


def test_owners_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mem_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "pypevoc_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "host", "mem_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mem_check ok" in r.stdout
