"""The host mirror's renumbering (tests/host/reorder_host_test.cpp, compiled here against libntrace_amd.so): Renderer::reorderBVH fails
for a kd-tree builder and without a scene, CudaBVH::reorder for a layout other than Compact (no GPU needed); on a GPU, for
Renderer("DeviceSAHBVH"), ("HLBVH") and ("PersistentBVH") on the Cornell box, frame -> reorderBVH -> frame gives the first frame's
primary and AO records bit for bit, and the tree's buffers after the call equal the numpy spec (tests/np_bvh_reorder.py) applied to
the buffers before it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "reorder_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reorder_host") / "reorder_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_reorder_failures_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reorder_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_renderer_reorder_frames_gpu(exe, tmp_path):
    from ntrace_amd import scenes

    import np_bvh_reorder as ro

    tri, pos, cam = scenes.cornell_box()
    w, h = 160, 120
    np.ascontiguousarray(tri, np.int32).tofile(str(tmp_path / "tri.bin"))
    np.ascontiguousarray(pos, np.float32).tofile(str(tmp_path / "pos.bin"))
    np.concatenate([np.asarray(cam["eye"], np.float32), np.asarray(scenes.nscreen_to_world(cam, w, h), np.float32).reshape(-1),
                    np.array([cam["far"], w, h], np.float32)]).tofile(str(tmp_path / "cam.bin"))
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reorder_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    for builder in ("DeviceSAHBVH", "HLBVH", "PersistentBVH"):
        spec = ro.reorder(rd(builder + "_nodes0.bin", np.uint8), rd(builder + "_woop0.bin", np.uint8), rd(builder + "_index0.bin", np.int32))
        assert rd(builder + "_nodes1.bin", np.int32).tobytes() == spec["nodes"].tobytes(), builder
        assert rd(builder + "_woop1.bin", np.uint8).tobytes() == spec["woop"].tobytes(), builder
        assert rd(builder + "_index1.bin", np.int32).tobytes() == spec["tri_index"].tobytes(), builder
