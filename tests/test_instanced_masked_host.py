"""The host mirror's instance visibility (tests/host/instanced_masked_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::setInstanceMasks is refused before setInstances, follows the count-change rule and leaves isBuilt() alone; on a GPU
traceBatch with masks equals ntr_trace_instanced_masked byte for byte, and an InstancedRenderer AO frame whose primary mask hides an
instance shows no primary record on it while AO rays still hit it."""
import ctypes as C
import os
import subprocess

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_masked_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_masked_host") / "instanced_masked_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_instance_masks_refusals_and_bookkeeping_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_masked_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: isBuilt() stays false" in out.stdout


@pytest.mark.gpu
def test_masked_batches_equal_the_c_abi_and_a_hidden_instance_still_occludes_gpu(exe):
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_masked_host_test gpu: ok" in out.stdout
    print(out.stdout)
