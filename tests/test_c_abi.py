"""A plain-C host of the shared library (tests/c_abi/check_abi.c): no Python, no
torch between the caller and the C ABI."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "check_abi")
    libdir = os.path.join(ROOT, "disconet_amd")
    cmd = ["gcc", "-std=c11", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "c_abi", "check_abi.c"),
           "-L", libdir, "-ldisconet_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_c_host_error_behaviour(tmp_path):
    out = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "C ABI error behaviour: ok" in out.stdout


# (hi, lo) bit patterns of sp_split.h :: split for the list check_sp_layout.cpp prints: a tie-free value, pi, a value clamped
# from below, a value whose hi is subnormal (lo rounds to -0), a value clamped from above, NaN (fminf(fmaxf()) gives -65504)
SPLIT_PAIRS = ["3c01 8002", "4248 13ee", "fbff 0000", "00a8 8000", "7bff 0000", "fbff 0000"]


def test_sp_layout_and_split_on_the_host(tmp_path):
    """The format's index maps and its split, compiled for the host: no GPU.  ROCm's clang is the host compiler
    (_Float16); the test fails where it is missing."""
    exe = str(tmp_path / "check_sp_layout")
    subprocess.check_call(["/opt/rocm/llvm/bin/clang++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "disconet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "check_sp_layout.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "SP LAYOUT CHECK PASSED" in out.stdout
    got = [ln.split(": ")[1] for ln in out.stdout.splitlines() if ln.startswith("split ")]
    assert got == SPLIT_PAIRS


@pytest.mark.gpu
def test_c_host_conv_and_voxelizer(tmp_path):
    out = subprocess.run([_build(tmp_path), "--gpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bit-exact" in out.stdout and out.stdout.strip().endswith("OK")
