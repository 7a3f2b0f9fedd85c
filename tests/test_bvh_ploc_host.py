"""The host mirror's PLOC path (tests/host/ploc_host_test.cpp, compiled here against libntrace_amd.so): Renderer("PLOCBVH") is a BVH
builder and a build without a device is refused with a zeroed result; on a GPU, CudaPLOCBuilder's tree equals the numpy spec at radius 8 over the scene's bounding box, its stream round-trips
byte for byte, and the Renderer's primary and AO frames equal ntr_trace_bvh on the same tree."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ploc_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("ploc_host") / "ploc_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_renderer_ploc_bvh_is_a_bvh_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ploc_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: ntr_ploc_build returned -" in out.stdout


@pytest.mark.gpu
def test_renderer_ploc_bvh_frames_gpu(exe, tmp_path):
    import torch
    from gpu_util import up

    import np_bvh_ploc as pl

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ploc_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    nodes, woop, idx = rd("nodes.bin", np.int32).reshape(-1, 16), rd("woop.bin", np.uint8), rd("index.bin", np.int32)
    # the Renderer's tree is the spec's at radius 8 over the scene's bounding box
    tri, verts = rd("tris.bin", np.int32).reshape(-1, 3), rd("verts.bin", np.float32).reshape(-1, 3)
    ref = pl.build(tri, verts, *pl.scene_box(verts), 8)
    assert np.array_equal(nodes, ref["nodes"]) and np.array_equal(idx, ref["tri_index"]) and np.array_equal(woop, ref["woop"])
    assert "%d rounds" % ref["stats"]["numRounds"] in out.stdout and "height %d" % ref["stats"]["height"] in out.stdout
    # the stream holds the three buffers as they are
    stream = rd("stream.bin", np.uint8).tobytes()
    for b in (nodes, woop, idx):
        assert b.tobytes() in stream
    d_nodes, d_woop, d_idx = up(nodes), up(woop), up(idx)
    for kind, any_hit in (("primary", False), ("ao", True)):
        rays = rd(kind + "_rays.bin", np.uint8).view(nt.RAY_DTYPE)
        got = rd(kind + "_results.bin", np.uint8).view(nt.RESULT_DTYPE)
        d_rays = up(rays)
        d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        nt.trace_bvh("fermi_speculative_while_while", rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_nodes.data_ptr(),
                     nodes.nbytes, d_woop.data_ptr(), woop.nbytes, d_idx.data_ptr())
        torch.cuda.synchronize()
        direct = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
        assert np.array_equal(got["id"], direct["id"]), kind
        if not any_hit:
            assert np.array_equal(got.view(np.uint32), direct.view(np.uint32)), kind
        assert (got["id"] >= 0).any()
