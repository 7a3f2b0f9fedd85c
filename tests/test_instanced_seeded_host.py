"""The host mirror's static world (tests/host/instanced_seeded_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::setWorld refuses a BLAS outside the pool and appends the world's instance record, clearWorld takes it away; on a GPU
traceBatch with a world equals ntr_trace_bvh + the seeded two-level trace byte for byte, and an InstancedRenderer primary and AO frame
over seeded_scenes.world_scene equal the frames with the world as an ordinary identity instance -- there the specs show that no closest
hit differs and that every any-hit ray agrees in hit or miss (test_instanced_seeded_cpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_seeded_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_seeded_host") / "instanced_seeded_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_set_world_refusals_and_the_appended_record_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_seeded_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the world is bookkeeping only" in out.stdout


def _write_scene(d):
    """seeded_scenes.world_scene as the program reads it: the meshes as ntr_ploc_build_batch takes them, the instances, the world."""
    import np_bvh_ploc as pl
    import instanced_scenes as isc
    import seeded_scenes as sds
    from test_instanced_frame_cpu import geometry

    sc = sds.world_scene()
    tri, pos, blas_tris = geometry(sc["names"])
    meshes = np.zeros(len(sc["names"]), np.dtype([("firstTri", "<i4"), ("numTris", "<i4"), ("sceneMin", "<f4", (3,)), ("sceneMax", "<f4", (3,))]))
    for k, name in enumerate(sc["names"]):
        meshes[k] = (blas_tris[k][0], blas_tris[k][1]) + tuple(np.asarray(b, np.float32) for b in pl.scene_box(isc.blas(name)[1]))
    for name, a in (("tri.bin", tri.astype(np.int32)), ("pos.bin", pos.astype(np.float32)), ("meshes.bin", meshes),
                    ("transforms.bin", sc["transforms"].astype(np.float32)), ("blas.bin", sc["blas"].astype(np.int32)),
                    ("world.bin", np.asarray([sc["world"]], np.int32))):
        np.ascontiguousarray(a).tofile(str(d / name))
    return sc


@pytest.mark.gpu
def test_trace_batch_equals_the_c_abi_and_frames_equal_the_identity_instance_gpu(exe, tmp_path):
    _write_scene(tmp_path)
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_seeded_host_test gpu: ok" in out.stdout
    assert re.search(r"primary instance ids: 0 of 2048 differ", out.stdout)
    for form in ("binary", "wide"):
        got = re.search(form + r" frames 64x32, 4 samples: world against identity instance: (\d+) of 2048 primary records differ in id or t, (\d+) in a "
                        r"real instance's words, (\d+) primary pixels, (\d+) of (\d+) AO rays in hit or miss, (\d+) AO pixels", out.stdout)
        assert got and [int(got.group(k)) for k in (1, 2, 3, 4, 6)] == [0] * 5 and int(got.group(5)) > 1000, out.stdout
