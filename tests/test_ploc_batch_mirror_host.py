"""The host mirror's batched BLAS build (tests/host/ploc_batch_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::buildBLASes refuses bad batches and a build without a device; on a GPU its pool equals byte for byte the pool that
addBLAS makes of one CudaPLOCBuilder tree per mesh, and a top-level tree over it traces."""
import ctypes as C
import os
import subprocess

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ploc_batch_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("ploc_batch_host") / "ploc_batch_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_build_blases_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ploc_batch_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: buildBLASes refused" in out.stdout


@pytest.mark.gpu
def test_build_blases_equals_one_builder_call_per_blas_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ploc_batch_host_test gpu: ok" in out.stdout
    print(out.stdout)
