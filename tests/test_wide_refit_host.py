"""The host mirror's in-place wide refit (tests/host/wide_refit_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::refitBLASesWide and refitWide are refused without wide trees and follow their preconditions and flags; on a GPU a frame
updated by refitBLASesWide + refitWide gives the wide buffers and the trace records of the same frame updated by refitBLASes + refit +
widen, byte for byte, for a deformation under which the widening provably makes the same choices (the program's header has the argument)."""
import ctypes as C
import os
import subprocess

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wide_refit_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("wide_refit_host") / "wide_refit_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_wide_refits_are_refused_without_wide_trees_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide_refit_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the wide refits stay refused" in out.stdout


@pytest.mark.gpu
def test_flags_and_a_frame_refitted_in_place_equals_the_frame_widened_again_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide_refit_host_test gpu: ok" in out.stdout
    print(out.stdout)
