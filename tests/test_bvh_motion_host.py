"""The host mirror's deformation motion blur (tests/host/bvh_motion_host_test.cpp, compiled here against libntrace_amd.so):
CudaBVH::refitMotion and CudaBVHTracer::setTime / setRayTimes fail by name where they must (no GPU needed); on a GPU, refitMotion over
soup1500's host SAH tree leaves the spec's buffers (tests/np_bvh_motion.py), traceBatch with setTime(0.5) and with per-ray times gives
the spec's records in all four words, a tree without motion ignores the times, and a later refit() drops the motion state."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "bvh_motion_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bvh_motion_host") / "bvh_motion_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_motion_failures_by_name_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bvh_motion_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_refit_motion_and_timed_trace_gpu(exe, tmp_path):
    import ntrace_amd as nt

    import bvh_motion_cases as mc
    import np_bvh_motion as bm
    import np_bvh_refit as rf
    import np_tracer

    tri, pos0 = mc.scene("soup1500")
    pos1 = rf.deform(pos0, 0.02)
    h = nt.sah_build(tri, pos0)
    nodes, woop, idx = h.nodes.copy(), h.woop.copy(), h.tri_index.copy()
    rays = mc.rays_of("soup1500", "tail")
    times = mc.hashed_times(rays.shape[0])
    for name, a in (("tris", tri), ("pos0", pos0), ("pos1", pos1), ("nodes", nodes), ("woop", woop), ("index", idx), ("rays", rays), ("times", times)):
        np.ascontiguousarray(a).tofile(str(tmp_path / (name + ".bin")))

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bvh_motion_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    m = bm.motion_refit(nodes, woop, idx, tri, pos0, pos1, 0.0)
    assert np.array_equal(rd("nodes0.bin", np.int32).reshape(-1, 16), m["nodes0"]) and np.array_equal(rd("nodes1.bin", np.int32).reshape(-1, 16), m["nodes1"])
    assert np.array_equal(rd("woop0.bin", np.uint8), m["woop"])
    assert np.array_equal(rd("vrows0.bin", np.uint32).reshape(-1, 4), m["vrows0"]) and np.array_equal(rd("vrows1.bin", np.uint32).reshape(-1, 4), m["vrows1"])
    half, key0 = mc.spec_trace(m, idx, rays, time=0.5), mc.spec_trace(m, idx, rays, time=0.0)
    mc.assert_records_equal_spec(rd("half.bin", nt.RESULT_DTYPE), half, "setTime(0.5)")
    mc.assert_records_equal_spec(rd("per_ray.bin", nt.RESULT_DTYPE), mc.spec_trace(m, idx, rays, times=times), "setRayTimes")
    mc.assert_records_equal_spec(rd("key0.bin", nt.RESULT_DTYPE), key0, "no time set")
    mc.assert_records_equal_spec(rd("static_after.bin", nt.RESULT_DTYPE), key0, "after refit()")
    before = rd("static_before.bin", nt.RESULT_DTYPE)
    ref = np_tracer.trace(nodes, woop, idx, rays)
    assert np.array_equal(before["id"], ref[0]) and np.array_equal(before["t"].view(np.uint32), ref[1].view(np.uint32))
    assert (rd("half.bin", np.uint32).reshape(-1, 4) != rd("key0.bin", np.uint32).reshape(-1, 4)).any()     # the time was read
