"""The host mirror's instanced scenes (tests/host/instanced_host_test.cpp, compiled here against libntrace_amd.so): CudaInstancedBVH
copies BLASes into its pool without rewriting a word, inverts with ntr_instance_invert and refuses to build without a device; on a
GPU its top-level tree and records equal the numpy spec (tests/np_instanced.py) and its batches equal ntr_trace_instanced and the spec."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_host") / "instanced_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_instanced_bvh_pool_and_refusals_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: build refused" in out.stdout


@pytest.mark.gpu
def test_instanced_bvh_equals_spec_and_the_c_abi_gpu(exe, tmp_path):
    import torch
    from gpu_util import up

    import np_instanced as ni

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_host_test gpu: ok" in out.stdout
    print(out.stdout)
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dtype=dt)  # noqa: E731
    pool = dict(nodes=rd("pool_nodes.bin", np.uint8), woop=rd("pool_woop.bin", np.uint8), tri_index=rd("pool_index.bin", np.int32),
                ranges=[tuple(int(x) for x in r) for r in rd("ranges.bin", np.int64).reshape(-1, 4)])
    inst = rd("instances.bin", nt.INSTANCE_DTYPE)
    tlas, records = rd("tlas.bin", np.int32).reshape(-1, 16), rd("records.bin", np.uint32).reshape(-1, 16)
    # worldToObject is the spec's inverse, and the tree and records are the spec's at radius 8
    assert inst.tobytes() == ni.instances(inst["objectToWorld"], inst["blas"]).tobytes()
    ref = ni.tlas_build(pool["nodes"], pool["ranges"], inst, 8)
    assert np.array_equal(tlas, ref["nodes"]) and np.array_equal(records, ref["records"])
    assert "%d rounds" % ref["stats"]["numRounds"] in out.stdout and "height %d" % ref["stats"]["height"] in out.stdout
    d_pool = up(pool["nodes"]), up(pool["woop"]), up(pool["tri_index"])
    d_tlas, d_rec = up(tlas), up(records)
    for kind, any_hit in (("closest", False), ("any", True)):
        rays = rd(kind + "_rays.bin", np.uint8).view(nt.RAY_DTYPE)
        got, ids = rd(kind + "_results.bin", np.uint8).view(nt.RESULT_DTYPE), rd(kind + "_ids.bin", np.int32)
        n = rays.shape[0]
        d_rays = up(rays)
        d_res, d_ids = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 4, dtype=torch.uint8, device="cuda:0")
        nt.trace_instanced(n, any_hit, d_rays.data_ptr(), d_res.data_ptr(), d_ids.data_ptr(), d_tlas.data_ptr(), tlas.nbytes, 0, d_rec.data_ptr(),
                           inst.shape[0], d_pool[0].data_ptr(), pool["nodes"].size, d_pool[1].data_ptr(), pool["woop"].size, d_pool[2].data_ptr())
        torch.cuda.synchronize()
        assert got.tobytes() == d_res.cpu().numpy().tobytes() and ids.tobytes() == d_ids.cpu().numpy().tobytes(), kind
        rid, rt, ru, rv, rinst = ni.trace(ref["nodes"], 0, ref["records"], pool, rays, any_hit)
        assert np.array_equal(got["id"], rid) and np.array_equal(got["t"].view(np.uint32), rt.view(np.uint32)) and np.array_equal(ids, rinst), kind
        assert np.array_equal(got["padA"].view(np.uint32), ru.view(np.uint32)) and np.array_equal(got["padB"].view(np.uint32), rv.view(np.uint32))
        assert (rid >= 0).any() and len(set(rinst[rinst >= 0])) > 3
