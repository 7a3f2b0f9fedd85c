"""The host mirror's wide path (tests/host/instanced_wide_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::widen is refused before build() and follows the invalidation rules; setTraceWide(false) gives the old bytes; on a GPU the
wide traceBatch equals ntr_trace_instanced_wide byte for byte, and an InstancedRenderer AO frame with setWide(true) reconstructs and
differs from the binary frame in no more pixels than primary records differ between the two numpy specs on the program's own scene."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_wide_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_wide_host") / "instanced_wide_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_widen_refusals_and_bookkeeping_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: widen() stays refused" in out.stdout


@pytest.mark.gpu
def test_wide_batches_equal_the_c_abi_and_a_wide_ao_frame_gpu(exe, tmp_path):
    """The share of pixels that may differ between the wide and the binary AO frame is stated from the specs: np_instanced.trace and
    np_instanced_wide.trace (over np_instanced_wide's own widening) on the buffers the program wrote -- its pool, its top-level tree,
    its records, its instances and its primary rays -- and the primary records in which the two differ."""
    import np_instanced as ni
    import np_instanced_wide as nw

    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_wide_host_test gpu: ok" in out.stdout
    print(out.stdout)
    got = re.search(r"wide against binary: (\d+) of (\d+) pixels differ, (\d+) of (\d+) primary records differ", out.stdout)
    pix_diff, n, rec_diff = int(got.group(1)), int(got.group(2)), int(got.group(3))

    def load(name, dtype):
        return np.fromfile(str(tmp_path / name), dtype=dtype)
    ranges = [tuple(int(x) for x in r) for r in load("ranges.bin", np.int64).reshape(-1, 4)]
    pool = dict(nodes=load("pool_nodes.bin", np.uint8), woop=load("pool_woop.bin", np.uint8), tri_index=load("pool_index.bin", np.int32), ranges=ranges)
    tlas = load("tlas_nodes.bin", np.int32).reshape(-1, 16)
    records = load("records.bin", np.uint32).reshape(-1, 16)
    inst = load("instances.bin", ni.INSTANCE_DTYPE)
    rays = load("rays.bin", nt.RAY_DTYPE)
    assert rays.shape[0] == n and inst.shape[0] == records.shape[0] == tlas.shape[0] + 1
    wpool = nw.widen_pool(pool)
    wt = nw.widen_tlas(tlas, 0, inst, ranges, wpool["ranges"])
    b = ni.trace(tlas, 0, records, pool, rays)
    w = nw.trace(wt["nodes"], 0, wt["records"], pool, wpool, rays)
    differ = np.zeros(n, bool)
    for k in range(5):
        differ |= np.asarray(b[k]).view(np.uint32) != np.asarray(w[k]).view(np.uint32)
    share = differ.sum() / n
    print("the two specs differ in %d of %d primary records (share %.4f); the frames differ in %d pixels" % (differ.sum(), n, share, pix_diff))
    assert (np.asarray(b[0]) >= 0).sum() > n // 8
    assert rec_diff == differ.sum()              # the device's primary records differ exactly where the specs' do
    assert pix_diff <= share * n
