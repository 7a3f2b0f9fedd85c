"""The host mirror's HLBVH path (tests/host/hlbvh_host_test.cpp, compiled here against libntrace_amd.so): cache names of the LBVH and
HLBVH builders, HLBVHBuilder with hlbvh = true, and a Renderer frame on an HLBVH tree checked against the oracle."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "hlbvh_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("hlbvh_host") / "hlbvh_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_hlbvh_cache_names_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hlbvh_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_hlbvh_builder_and_renderer_gpu(exe, tmp_path):
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hlbvh_host_test gpu: ok" in out.stdout
    for kernel in ("fermi_speculative_while_while", "kepler_dynamic_fetch"):
        rd = lambda name, dt: np.fromfile(str(tmp_path / ("%s_%s.bin" % (kernel, name))), dtype=dt)  # noqa: E731
        nodes, woop, idx = rd("nodes", np.uint8), rd("woop", np.uint8), rd("index", np.int32)
        rays = rd("rays", np.float32).reshape(-1, 8)
        got = rd("results", np.int32).reshape(-1, 4)
        ref, _ = oracle.trace(nodes, woop, idx, rays)
        assert np.array_equal(got[:, 0], ref["id"]), kernel
        assert np.array_equal(got[:, 1].view(np.uint32), ref["t"].view(np.uint32)), kernel
