"""The host mirror's refit path (tests/host/refit_host_test.cpp, compiled here against libntrace_amd.so): Scene::setVertexPositions
gives a moved Scene's normals and box and Renderer::refit fails for a kd-tree builder (no GPU needed); on a GPU, for
Renderer("SAHBVH"), ("HLBVH") and ("PersistentBVH"), frame -> setVertexPositions -> refit -> frame gives the primary and AO records
of a second Renderer over the moved mesh whose tree was refitted through ntr_bvh_refit directly, and the refitted trees equal the
numpy spec (tests/np_bvh_refit.py) byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "refit_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("refit_host") / "refit_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_set_vertex_positions_and_refit_failures_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refit_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_renderer_refit_frames_gpu(exe, tmp_path):
    import np_bvh_refit as rf

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refit_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    tri, moved = rd("tris.bin", np.int32).reshape(-1, 3), rd("verts.bin", np.float32).reshape(-1, 3)
    for builder, eps in (("SAHBVH", 0.0), ("HLBVH", 0.001), ("PersistentBVH", 0.0)):
        nodes0, woop0, idx = rd(builder + "_nodes0.bin", np.uint8), rd(builder + "_woop0.bin", np.uint8), rd(builder + "_index.bin", np.int32)
        spec = rf.refit(nodes0, woop0, idx, tri, moved, eps)
        assert np.array_equal(rd(builder + "_nodes1.bin", np.int32).reshape(-1, 16), spec["nodes"]), builder
        assert np.array_equal(rd(builder + "_woop1.bin", np.uint8), spec["woop"]), builder
