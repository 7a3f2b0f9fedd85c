"""The host mirror's deforming BLASes (tests/host/instanced_deform_host_test.cpp, compiled here against libntrace_amd.so):
CudaInstancedBVH::refitBLASesMotion / clearDeform / hasDeform / getDeformRefitResult; hasDeform() drops after refitBLASes and
optimizeBLASes; the lazy refitMotion() before traceBatch; every form that is not combinable is refused by name; on a GPU the mirror's
path equals ntr_tlas_deform_refit + ntr_trace_instanced_deform byte for byte, and the records of one batch equal the numpy rule
(tests/np_instanced_deform.py) traced over the buffers the mirror made."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ntrace_amd as nt
import instanced_motion_cases as mc
import np_bvh_refit as rf
import np_instanced_deform as nd
from test_instanced_seeded_host import _write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "instanced_deform_host_test.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ntrace_amd", "csrc")])
    out = str(tmp_path_factory.mktemp("instanced_deform_host") / "instanced_deform_host_test")
    lib = os.path.join(ROOT, "ntrace_amd")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ntrace_amd", "csrc"), "-I" + os.path.join(ROOT, "ntrace_amd", "host")]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-ffp-contract=off"] + inc + [SRC, "-o", out, "-L" + lib, "-lntrace_amd",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_the_refusals_that_need_no_device_cpu(exe):
    out = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_deform_host_test cpu: ok" in out.stdout
    cnt = C.c_int(-1)
    if not (nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0):   # the no-device case ran
        assert "no device: the deformation is bookkeeping only" in out.stdout


@pytest.mark.gpu
def test_the_mirror_equals_the_c_abi_and_the_rule_gpu(exe, tmp_path):
    sc = _write_scene(tmp_path)
    np.ascontiguousarray(mc.key1_transforms(sc["transforms"]), np.float32).tofile(str(tmp_path / "transforms1.bin"))
    pos = np.fromfile(str(tmp_path / "pos.bin"), np.float32).reshape(-1, 3)
    np.ascontiguousarray(rf.moved(pos, 0.05), np.float32).tofile(str(tmp_path / "pos1.bin"))
    out = subprocess.run([exe, "gpu", str(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "instanced_deform_host_test gpu: ok" in out.stdout
    assert len(re.findall(r": deform equals the C-ABI, \d+ hits", out.stdout)) == 5 and "differs" not in out.stdout
    # the numpy rule over the buffers the mirror made, for the batch it wrote out: BLAS 1 deforms, the instances move, per-ray times
    get = lambda name, dt: np.fromfile(str(tmp_path / ("out_%s.bin" % name)), dt)   # noqa: E731
    ranges = [tuple(int(x) for x in r) for r in get("ranges", np.int64).reshape(-1, 4)]
    pool = dict(nodes=get("nodes", np.uint8), nodes1=get("nodes1", np.uint8), woop=get("woop", np.uint8), vrows0=get("vrows0", np.uint8),
                vrows1=get("vrows1", np.uint8), tri_index=get("index", np.int32), ranges=ranges)
    records = get("records", np.uint32).reshape(-1, 16)
    assert sorted(set(records[:, 15].tolist())) == [0, 1, 2, 3] or set(records[:, 15].tolist()) <= {0, 1, 2, 3}
    assert (records[:, 15] & 2 != 0).sum() == (sc["blas"] == 1).sum() > 0 and (records[:, 15] & 1).any()
    rays = get("rays", nt.RAY_DTYPE)
    want = nd.trace(get("tlas", np.uint8), 0, records, get("keys", np.uint8), pool, rays, False, times=get("times", np.float32))
    got = get("results", nt.RESULT_DTYPE)
    assert np.array_equal(got["id"], want[0]) and np.array_equal(got["t"].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got["padA"].view(np.uint32), want[2].view(np.uint32)) and np.array_equal(got["padB"].view(np.uint32), want[3].view(np.uint32))
    assert np.array_equal(get("ids", np.int32), want[4]) and want[5]["numDeformTriTests"] > 0 and want[5]["numMovingEntries"] > 0
