"""The host mirror over the batched pool widening (tests/host/pool_widen_batch_host_test.cpp, compiled here against libntrace_amd.so):
a CudaInstancedBVH over a pool of three BLASes takes ntr_pool_widen_batch in widen(); the wide pool it holds equals ntr_pool_widen's
(checked in the program) and np_instanced_wide.widen_pool's (checked here), and its wide traceBatch gives the spec's records and
instance ids, closest hit and any hit, on the buffers the program wrote."""
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pool_widen_batch_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("pool_widen_batch_host") / "pool_widen_batch_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_program_compiles_and_states_its_usage(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stdout


@pytest.mark.gpu
def test_widen_takes_the_batch_and_the_trace_gives_the_specs_records_gpu(exe, tmp_path):
    import np_instanced as ni
    import np_instanced_wide as nw

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pool_widen_batch_host_test gpu: ok" in out.stdout

    def load(name, dtype):
        return np.fromfile(str(tmp_path / name), dtype=dtype)
    ranges = [tuple(int(x) for x in r) for r in load("ranges.bin", np.int64).reshape(-1, 4)]
    assert len(ranges) == 3
    pool = dict(nodes=load("pool_nodes.bin", np.uint8), woop=load("pool_woop.bin", np.uint8), tri_index=load("pool_index.bin", np.int32), ranges=ranges)
    tlas = load("tlas_nodes.bin", np.int32).reshape(-1, 16)
    inst = load("instances.bin", ni.INSTANCE_DTYPE)
    rays = load("rays.bin", nt.RAY_DTYPE)
    wpool = nw.widen_pool(pool)
    assert load("wide_pool.bin", np.uint8).tobytes() == wpool["nodes"].tobytes()
    wt = nw.widen_tlas(tlas, 0, inst, ranges, wpool["ranges"])
    for any_hit, tag in ((False, "closest"), (True, "any")):
        rid, rt, ru, rv, rinst, _ = nw.trace(wt["nodes"], 0, wt["records"], pool, wpool, rays, any_hit)
        want = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
        want["id"], want["t"], want["padA"], want["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
        assert load("results_%s.bin" % tag, np.uint8).tobytes() == want.tobytes(), tag
        assert load("ids_%s.bin" % tag, np.int32).tobytes() == rinst.astype(np.int32).tobytes(), tag
        assert (rid >= 0).sum() > rays.shape[0] // 16
