"""The host mirror over the pool optimiser (tests/host/optimize_batch_host_test.cpp, compiled here against libntrace_amd.so): a
CudaInstancedBVH runs buildBLASes, moves its vertices, refitBLASes, refit and optimizeBLASes.  The program checks the flags (isBuilt()
kept, the wide pool dropped and restored by widen(), a world kept) and that the TLAS does not change; here the pool it wrote equals
np_optimize_batch.optimize of the pool it had, measureBLASes before and after equals np_optimize_batch.sah_costs, and its traceBatch
gives the specs' records and instance ids, closest hit and any hit, binary and -- after widen() -- wide."""
import os
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "optimize_batch_host_test.cpp")
SAH_DTYPE = np.dtype([("sahCost", "<f4"), ("numNodes", "<i4"), ("numLeaves", "<i4"), ("numTris", "<i4"), ("height", "<i4"), ("seconds", "<f4")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("optimize_batch_host") / "optimize_batch_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_program_compiles_and_states_its_usage(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "usage" in out.stdout


@pytest.mark.gpu
def test_optimize_blases_in_the_frame_loop_equals_the_specs_gpu(exe, tmp_path):
    import np_instanced as ni
    import np_instanced_wide as nw
    import np_optimize_batch as ob

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "optimize_batch_host_test gpu: ok" in out.stdout

    def load(name, dtype):
        return np.fromfile(str(tmp_path / name), dtype=dtype)
    ranges = [tuple(int(x) for x in r) for r in load("ranges.bin", np.int64).reshape(-1, 4)]
    assert len(ranges) == 3
    refitted, woop = load("pool_refitted.bin", np.uint8), load("pool_woop.bin", np.uint8)
    # optimizeBLASes(): two passes over every BLAS; then optimizeBLASes({1}, 1, 1): one more over BLAS 1
    first = ob.optimize(ranges, refitted, 2)
    second = ob.optimize([ranges[1]], first["nodes"], 1)
    assert first["rewritten"][0] > 0
    assert load("pool_optimized.bin", np.uint8).tobytes() == second["nodes"].tobytes()
    res = nt.BvhOptimizeBatchResult.from_buffer_copy(load("optimize_result.bin", np.uint8).tobytes())
    assert list(res.formed)[:2] == first["formed"] and list(res.rewritten)[:2] == first["rewritten"]
    assert (res.maxHeightBefore, res.maxHeightAfter) == (max(first["heightBefore"]), max(first["heightAfter"]))
    for name, nodes in (("sah_before.bin", refitted), ("sah_after.bin", first["nodes"])):
        got, want = load(name, SAH_DTYPE), ob.sah_costs(ranges, nodes, woop)
        for g, w in zip(got, want):
            assert g["sahCost"].tobytes() == np.float32(w["sahCost"]).tobytes(), name
            assert (g["numNodes"], g["numLeaves"], g["numTris"], g["height"]) == (w["numNodes"], w["numLeaves"], w["numTris"], w["height"]), name

    pool = dict(nodes=second["nodes"], woop=woop, tri_index=load("pool_index.bin", np.int32), ranges=ranges)
    tlas = load("tlas_nodes.bin", np.int32).reshape(-1, 16)
    records = load("records.bin", np.uint32).reshape(-1, 16)
    inst = load("instances.bin", ni.INSTANCE_DTYPE)
    rays = load("rays.bin", nt.RAY_DTYPE)
    # the TLAS the object kept is the tree a build over the optimised pool gives
    built = ni.tlas_build(pool["nodes"], ranges, inst, 8)
    assert np.array_equal(built["nodes"], tlas) and np.array_equal(built["records"], records)

    def same(tag, rid, rt, ru, rv, rinst):
        want = np.zeros(rays.shape[0], nt.RESULT_DTYPE)
        want["id"], want["t"], want["padA"], want["padB"] = rid, rt, ru.view(np.int32), rv.view(np.int32)
        assert load("results_%s.bin" % tag, np.uint8).tobytes() == want.tobytes(), tag
        assert load("ids_%s.bin" % tag, np.int32).tobytes() == rinst.astype(np.int32).tobytes(), tag
        assert (rid >= 0).sum() > rays.shape[0] // 16
    wpool = nw.widen_pool(pool)
    assert load("wide_pool.bin", np.uint8).tobytes() == wpool["nodes"].tobytes()
    wt = nw.widen_tlas(tlas, 0, inst, ranges, wpool["ranges"])
    for any_hit, tag in ((False, "closest"), (True, "any")):
        same("binary_" + tag, *ni.trace(tlas, 0, records, pool, rays, any_hit))
        same("wide_" + tag, *nw.trace(wt["nodes"], 0, wt["records"], pool, wpool, rays, any_hit)[:5])
