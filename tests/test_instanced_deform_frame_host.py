"""The host mirror's motion-blurred frames over deforming BLASes (tests/host/instanced_deform_frame_host_test.cpp, compiled here against
libntrace_amd.so): InstancedRenderer::setDeformGeometry refuses a short buffer, beginFrame keeps refusing the blur over deforming BLASes
without it and a scene with neither a motion key nor a deformation; on a GPU primary, AO and diffuse frames of 64 x 32 with 4 samples over
seeded_scenes.world_scene -- deforming only, then moving and deforming -- equal the same C-ABI calls byte for byte, the caller's flags and
times pointer come back, and after refitBLASes the blurred frame is the motion path's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt
import instanced_motion_cases as mc
import np_bvh_refit as rf
from test_instanced_seeded_host import _write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_deform_frame_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_deform_frame_host") / "instanced_deform_frame_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_closing_vertices_and_the_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_deform_frame_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the closing vertices are bookkeeping only" in out.stdout


@pytest.mark.gpu
def test_blurred_frames_over_deforming_blases_equal_the_c_abi_gpu(exe, tmp_path):
    sc = _write_scene(tmp_path)
    np.ascontiguousarray(mc.key1_transforms(sc["transforms"]), np.float32).tofile(str(tmp_path / "transforms1.bin"))
    pos = np.fromfile(str(tmp_path / "pos.bin"), np.float32).reshape(-1, 3)
    np.ascontiguousarray(rf.moved(pos, 0.05), np.float32).tofile(str(tmp_path / "pos1.bin"))
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_deform_frame_host_test gpu: ok" in out.stdout
    assert len(re.findall(r"deforming only, [^:]*: the blurred frame equals the C-ABI, \d+ primary hits", out.stdout)) == 4
    assert len(re.findall(r"moving and deforming, [^:]*: the blurred frame equals the C-ABI, \d+ primary hits", out.stdout)) == 3
    assert len(re.findall(r"after refitBLASes, AO: the blurred frame equals the C-ABI, \d+ primary hits", out.stdout)) == 1
