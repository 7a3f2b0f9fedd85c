"""The host mirror's instanced frames (tests/host/instanced_frame_host_test.cpp, compiled here against libntrace_amd.so):
InstancedRenderer::beginFrame refuses a renderer without geometry, a TLAS that is not built and a pool with an addBLAS tree, and each
message names the remedy; on a GPU an AO frame of a 3-mesh buildBLASes pool with 5 instances equals, byte for byte, the buffers the same
calls give when made directly through the C-ABI -- rays, results, resolved results, normals, pixels -- getTotalNumRays equals
ntr_count_hits, and after refitBLASes and refit() the next frame's normals differ from the first frame's and equal the direct calls'."""
import ctypes as C
import os
import subprocess

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_frame_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_frame_host") / "instanced_frame_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_frame_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_frame_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: build refused" in out.stdout


@pytest.mark.gpu
def test_frame_equals_the_c_abi_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_frame_host_test gpu: ok" in out.stdout
    print(out.stdout)
