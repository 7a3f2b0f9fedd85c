"""The host mirror's kd-tree path (tests/host/kdtree_host_test.cpp, compiled here against libntrace_amd.so): KDTree / CudaKDTree and
their stream round trip, the Renderer's kd-tree switch, and Renderer frames over "SAHKDTree" checked against ntr_trace_kdtree, the
numpy restatement and an "SAHBVH" frame."""
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

import np_kdtree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "kdtree_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("kdtree_host") / "kdtree_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_kdtree_classes_and_round_trip_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kdtree_host_test cpu: ok" in out.stdout


@pytest.mark.gpu
def test_renderer_kdtree_frames_gpu(exe, tmp_path):
    import torch
    from gpu_util import up

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kdtree_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    nodes, woop, idx = rd("SAHKDTree_nodes.bin", np.int32).reshape(-1, 4), rd("SAHKDTree_woop.bin", np.uint8), rd("SAHKDTree_index.bin", np.int32)
    bbox = rd("SAHKDTree_bbox.bin", np.float32)
    rays = rd("SAHKDTree_rays.bin", np.uint8).view(nt.RAY_DTYPE)
    got = rd("SAHKDTree_results.bin", np.uint8).view(nt.RESULT_DTYPE)
    # the frame's records are ntr_trace_kdtree's on the same rays, and the restatement's
    d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
    d_nodes, d_woop, d_idx, d_rays = up(nodes), up(woop), up(idx), up(rays)
    nt.trace_kdtree(rays.shape[0], False, bbox[:3], bbox[3:], d_rays.data_ptr(), d_res.data_ptr(), d_nodes.data_ptr(), nodes.nbytes,
                    d_woop.data_ptr(), woop.nbytes, d_idx.data_ptr(), idx.nbytes)
    torch.cuda.synchronize()
    direct = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
    assert np.array_equal(got.view(np.uint32), direct.view(np.uint32))
    ref = np_kdtree.trace(nodes, woop, idx, bbox[:3], bbox[3:], rays)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the BVH frame over the same scene.  The window of the hit counts: rays whose BVH hit is a triangle the SAH builder put into a
    # zero-width cell (the reference kernel can miss those, tests/test_kdtree_gpu.py::test_agreement_with_bvh_tracer) plus 0.2 % of
    # the frame for equal-t replacements and the kernel's interval slack
    bvh = rd("SAHBVH_results.bin", np.uint8).view(nt.RESULT_DTYPE)
    assert np.array_equal(rd("SAHBVH_rays.bin", np.uint8), rays.view(np.uint8))
    num_tris = rd("tris.bin", np.int32).shape[0] // 3
    face = np.zeros(num_tris, dtype=bool)
    for lo, hi, ids in np_kdtree.leaf_cells(nodes, idx, bbox[:3], bbox[3:]):
        if ids and np.any(hi - lo == 0.0):
            face[ids] = True
    bvh_face = (bvh["id"] >= 0) & face[np.maximum(bvh["id"], 0)]
    hk, hb = int((got["id"] >= 0).sum()), int((bvh["id"] >= 0).sum())
    window = int(bvh_face.sum()) + int(0.002 * rays.shape[0])
    print("primary hits: kd-tree %d, BVH %d of %d rays (window %d)" % (hk, hb, rays.shape[0], window))
    assert abs(hk - hb) <= window
    rest = ~bvh_face
    assert ((got["id"] >= 0) == (bvh["id"] >= 0))[rest].mean() >= 0.998
    both = (got["id"] >= 0) & (bvh["id"] >= 0) & rest
    assert (np.abs(got["t"][both] - bvh["t"][both]) <= 2e-4 + 2 * float(np_kdtree.delta_of(bbox[:3], bbox[3:]))).mean() >= 0.998
