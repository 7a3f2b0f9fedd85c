"""The host mirror's motion blur over the 4-wide trees (tests/host/instanced_wide_motion_host_test.cpp, compiled here against
libntrace_amd.so): CudaInstancedBVH::setTraceWideMotion / refitMotionWide and InstancedRenderer::setWideMotion.  With the switch off every
refusal of motion with the wide, FAST and world forms is word for word what it was; on, traceBatch takes the wide motion launch after
exactly one refitMotionWide(), equals ntr_tlas_wide_motion_refit + ntr_trace_instanced_wide_motion byte for byte over
seeded_scenes.world_scene with the key 1 of instanced_motion_cases, and goes stale with every call that writes records or boxes; a blurred
AO frame on the turning cube of instanced_motion_frame_cases over the wide trees is the binary frame wherever the records agree, and no AO
ray hits the cube it starts from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt
import instanced_motion_cases as mc
from test_instanced_seeded_host import _write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_wide_motion_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_wide_motion_host") / "instanced_wide_motion_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_switch_is_opt_in_and_off_every_refusal_is_todays_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_motion_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the wide motion is bookkeeping only" in out.stdout


@pytest.mark.gpu
def test_refit_motion_wide_trace_batch_and_the_cube_frame_gpu(exe, tmp_path):
    import instanced_motion_frame_cases as fc
    sc = _write_scene(tmp_path)
    np.ascontiguousarray(mc.key1_transforms(sc["transforms"]), np.float32).tofile(str(tmp_path / "transforms1.bin"))
    d = fc.demo()
    for name, a, dt in (("cube_tri.bin", d["tri"], np.int32), ("cube_pos.bin", d["pos"], np.float32),
                        ("cube_transforms.bin", d["ms"].inst0["objectToWorld"], np.float32),
                        ("cube_transforms1.bin", d["ms"].inst1["objectToWorld"], np.float32)):
        np.ascontiguousarray(a, dt).tofile(str(tmp_path / name))
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_motion_host_test gpu: ok" in out.stdout
    assert len(re.findall(r": wide motion equals the C-ABI, \d+ hits", out.stdout)) == 8 and "differs" not in out.stdout
    got = re.search(r"AO rays that hit the cube they start from: binary (\d+), wide (\d+)", out.stdout)
    assert got and got.group(1) == "0" and got.group(2) == "0", out.stdout
