"""The host mirror's 4-wide tree (tests/host/wide_host_test.cpp, compiled here against libntrace_amd.so): CudaWideBVH shares its
CudaBVH's Woop and index buffers and refuses to build without a device; on a GPU its wide node buffer equals the numpy spec
(tests/np_bvh_wide.py) and its batches equal ntr_trace_wide and the spec."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wide_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("wide_host") / "wide_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_wide_bvh_sharing_and_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: build refused" in out.stdout


@pytest.mark.gpu
def test_wide_bvh_equals_spec_and_the_c_abi_gpu(exe, tmp_path):
    import torch
    from gpu_util import up

    import np_bvh_wide as wd

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wide_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    nodes, woop, index = rd("nodes.bin", np.int32).reshape(-1, 16), rd("woop.bin", np.uint8), rd("index.bin", np.int32)
    wide = rd("wide.bin", np.int32).reshape(-1, 32)
    ref = wd.widen(nodes)
    assert np.array_equal(wide, ref["nodes"])
    st = ref["stats"]
    assert "wide: %d nodes (%d %d %d), %d leaf links, height %d, stackBound %d" % (
        st["numNodes"], *st["counts"], st["numLeafLinks"], st["height"], st["stackBound"]) in out.stdout
    d_wide, d_woop, d_idx = up(wide), up(woop), up(index)
    d_nodes = up(nodes)
    flags = nt.bvh_validate(d_nodes.data_ptr(), nodes.nbytes)
    for kind, any_hit in (("closest", False), ("any", True)):
        rays = rd(kind + "_rays.bin", np.uint8).view(nt.RAY_DTYPE)
        got = rd(kind + "_results.bin", np.uint8).view(nt.RESULT_DTYPE)
        n = rays.shape[0]
        d_rays = up(rays)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
        nt.trace_wide(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_wide.data_ptr(), wide.nbytes, d_woop.data_ptr(), woop.nbytes,
                      d_idx.data_ptr(), flags)
        torch.cuda.synchronize()
        assert got.tobytes() == d_res.cpu().numpy().tobytes(), kind
        rid, rt, ru, rv = wd.trace(ref["nodes"], woop, index, rays, any_hit)
        assert np.array_equal(got["id"], rid) and np.array_equal(got["t"].view(np.uint32), rt.view(np.uint32)), kind
        assert np.array_equal(got["padA"].view(np.uint32), ru.view(np.uint32)) and np.array_equal(got["padB"].view(np.uint32), rv.view(np.uint32))
        assert (rid >= 0).any() and (rid < 0).any()
