"""The host mirror's batched BLAS refit (tests/host/refit_batch_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::refitBLASes refuses a call before buildBLASes, a selection of an addBLAS tree and a bad index; on a GPU the pool
after buildBLASes, moved vertices and refitBLASes equals byte for byte the pool of one CudaBVH::refit per BLAS, and build() and
traceBatch give the records of that pool."""
import ctypes as C
import os
import subprocess

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "refit_batch_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("refit_batch_host") / "refit_batch_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_refit_blases_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refit_batch_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: buildBLASes refused" in out.stdout


@pytest.mark.gpu
def test_refit_blases_equals_one_refit_per_blas_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refit_batch_host_test gpu: ok" in out.stdout
    print(out.stdout)
