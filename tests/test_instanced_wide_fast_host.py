"""The host mirror's FAST switch for the wide path (tests/host/instanced_wide_fast_host_test.cpp, compiled here against
libntrace_amd.so): CudaInstancedBVH::setTraceWideFast / getTraceWideFast and InstancedRenderer::setWideFast; the wide flags buffer goes
stale with every call that rewrites a wide box or drops the wide trees and is validated once before the next wide fast trace; on a GPU
wide traceBatch with the switch on equals wide traceBatch with it off byte for byte through a widen / refitWide / refitBLASesWide /
setWorld / clearWorld loop over seeded_scenes.world_scene, wide frames with setWideFast(true) equal the wide frames without it word for
word, and setTraceFast alone is still ignored on the wide path."""
import ctypes as C
import os
import re
import subprocess

import pytest

import ntrace_amd as nt
from test_instanced_seeded_host import _write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_wide_fast_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_wide_fast_host") / "instanced_wide_fast_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_switch_and_the_staleness_flag_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_fast_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the switch is bookkeeping only" in out.stdout


@pytest.mark.gpu
def test_wide_fast_trace_batches_and_frames_equal_the_wide_ones_gpu(exe, tmp_path):
    _write_scene(tmp_path)
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_fast_host_test gpu: ok" in out.stdout
    assert len(re.findall(r": wide fast equals wide, \d+ hits", out.stdout)) == 9 and "differs" not in out.stdout
    for how in ("with a world", "no world"):
        assert re.search(r"wide frames 64x32, 4 samples, " + how + r": wide fast equals wide; \d+ lit pixels, \d+ AO rays", out.stdout), out.stdout
