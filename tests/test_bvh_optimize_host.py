"""The host mirror's treelet optimiser (tests/host/optimize_host_test.cpp, compiled here against libntrace_amd.so):
Renderer::optimizeBVH fails for a kd-tree builder and without a scene (no GPU needed); on a GPU, for Renderer("SAHBVH"), ("HLBVH") and ("PersistentBVH"), frame -> optimizeBVH -> frame
gives the primary and AO records of a second Renderer whose tree was optimised through ntr_bvh_optimize directly, calcSAHCost and
HLBVHBuilder::calcSAHGPU equal ntr_bvh_sah_cost, and the trees and costs equal the numpy spec (tests/np_bvh_optimize.py)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "optimize_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("optimize_host") / "optimize_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_optimize_failures_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimize_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_renderer_optimize_frames_gpu(exe, tmp_path):
    import np_bvh_optimize as op

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimize_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    for builder in ("SAHBVH", "HLBVH", "PersistentBVH"):
        nodes0, woop = rd(builder + "_nodes0.bin", np.uint8), rd(builder + "_woop.bin", np.uint8)
        spec = op.optimize(nodes0, 2)
        assert np.array_equal(rd(builder + "_nodes1.bin", np.int32).reshape(-1, 16), spec["nodes"]), builder
        sah0, sah1 = (np.float32(x) for x in open(str(tmp_path / (builder + "_sah.txt"))).read().split())
        assert sah0.tobytes() == op.sah_cost(nodes0, woop)["sahCost"].tobytes(), builder
        assert sah1.tobytes() == op.sah_cost(spec["nodes"], woop)["sahCost"].tobytes(), builder
