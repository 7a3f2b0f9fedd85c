"""The host mirror over ntr_bvh_motion_refit_batch (tests/host/motion_refit_batch_host_test.cpp, compiled here against
libntrace_amd.so): CudaInstancedBVH::refitBLASesMotion makes one batch call whose five pool buffers equal the loop of
ntr_bvh_motion_refit calls it replaced -- all BLASes of a five-BLAS pool, a subset in scrambled order, a second call that keeps the earlier
deforming BLASes -- and getBLASMotionRefitResult() holds the sums; one traced batch equals the records this driver's numpy rule
(tests/np_instanced_deform.py over tests/instanced_deform_cases.DeformScene) wrote for the program to compare with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt
import instanced_deform_cases as dc
import instanced_scenes as isc
import np_bvh_ploc as pl
import np_bvh_refit as rf
import np_instanced as ni

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "motion_refit_batch_host_test.cpp")
F = np.float32
NAMES = ["soup64", "soup1000", "one", "soup100", "soup64"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("motion_refit_batch_host") / "motion_refit_batch_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_what_needs_no_device_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "motion_refit_batch_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the result is bookkeeping only" in out.stdout


def _write_scene(d):
    """Five BLASes over one shared index array and three shared vertex arrays (key 0, and two second keys), ten static instances, the rays
    and their times, and the records the rule gives once BLASes 3 and 1 deform to pos1 and BLAS 4 to pos2."""
    tris, poss, meshes, t_off, v_off = [], [], [], 0, 0
    dt = np.dtype([("firstTri", "<i4"), ("numTris", "<i4"), ("sceneMin", "<f4", (3,)), ("sceneMax", "<f4", (3,))])
    for name in NAMES:
        tri, pos, _ = isc.blas(name)
        tris.append(np.asarray(tri, np.int32) + v_off)
        poss.append(np.asarray(pos, F))
        meshes.append((t_off, tri.shape[0]) + tuple(np.asarray(b, F) for b in pl.scene_box(pos)))
        t_off += tri.shape[0]
        v_off += pos.shape[0]
    key1 = [rf.moved(p, 0.05) for p in poss]
    key2 = [rf.moved(p, 0.2) for p in poss]
    which = (np.arange(10) % 5).astype(np.int32)
    tf = isc.seeded_transforms(10, 9, spread=4.0, size=0.5)
    inst = ni.instances(tf, which)
    scene = dc.DeformScene(NAMES, inst, inst, {3: (poss[3], key1[3]), 1: (poss[1], key1[1]), 4: (poss[4], key2[4])})
    rays = isc.scene_rays(primary=(48, 24), random=1024)
    n = rays.shape[0]
    times = ((np.arange(n) * 37 % 101) / 100.0).astype(F)
    rid, rt, ru, rv, rinst, cnt = scene.trace(rays, False, times=times)
    assert (rid >= 0).sum() > 50 and cnt["numDeformTriTests"] > 0
    want = np.zeros(n, nt.RESULT_DTYPE)
    want["id"], want["t"], want["padA"], want["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
    for name, a in (("tri.bin", np.concatenate(tris).astype(np.int32)), ("pos.bin", np.concatenate(poss).astype(F)),
                    ("pos1.bin", np.concatenate(key1).astype(F)), ("pos2.bin", np.concatenate(key2).astype(F)),
                    ("meshes.bin", np.array(meshes, dt)), ("transforms.bin", tf.astype(F)), ("blas.bin", which), ("rays.bin", rays),
                    ("times.bin", times), ("want_results.bin", want), ("want_ids.bin", rinst.astype(np.int32))):
        np.ascontiguousarray(a).tofile(str(d / name))
    return want, rinst.astype(np.int32)


@pytest.mark.gpu
def test_the_mirror_equals_the_loop_it_replaced_and_the_rule_gpu(exe, tmp_path):
    want, want_ids = _write_scene(tmp_path)
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    got = np.fromfile(str(tmp_path / "out_results.bin"), nt.RESULT_DTYPE) if os.path.exists(str(tmp_path / "out_results.bin")) else None
    if got is not None and got.shape == want.shape:
        print("records that differ from the rule: %d of %d" % (int((got.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1).sum()),
                                                                 want.shape[0]))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "motion_refit_batch_host_test gpu: ok" in out.stdout
    assert len(re.findall(r": the five pool buffers and the sums equal the loop's", out.stdout)) == 3 and "DIFFERS" not in out.stdout
    assert re.search(r"the traced batch equals the rule: \d+ rays, \d+ hits", out.stdout)
    assert got.tobytes() == want.tobytes() and np.fromfile(str(tmp_path / "out_ids.bin"), np.int32).tobytes() == want_ids.tobytes()
