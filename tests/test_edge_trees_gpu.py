"""The trace kernels over trees at the ends of the range the FAST slab test admits (tests/edge_trees.py), against the oracle.

For every scene and ray set: every per-ray body, closest hit and any hit, at the full count and at a prefix that ends mid-wave, in all
four words of a record; the validated flags and flags = 0 give the same bytes; the instrumented kernel's counters equal the oracle's
(a divide one rounding short moves the counters on these rays and not the records: test_edge_trees_cpu.py); the 4-wide trace equals its
numpy spec.  ntr_bvh_validate gives each scene the flags it is built for."""
import numpy as np
import pytest
import torch

import ntrace_amd as nt

import edge_trees as et
from gpu_util import gpu_trace, up
from np_bvh_validate import expected_flags
from test_wave_setup_gpu import Placed, check

pytestmark = pytest.mark.gpu

_placed = {}


def placed(name):
    if name not in _placed:
        _placed[name] = Placed(et.scene(name))
    return _placed[name]


@pytest.mark.parametrize("name", list(et.SCENES))
def test_validate_gives_the_scene_its_flags(name):
    sc = et.scene(name)
    flags = placed(name).view.validate()
    must, must_not = et.MUST[name]
    assert flags == expected_flags(sc.nodes), "flags 0x%x" % flags
    assert flags & must == must and flags & must_not == 0, "flags 0x%x" % flags


@pytest.mark.parametrize("name,which", et.CASES)
def test_per_ray_bodies_equal_the_oracle(monkeypatch, name, which):
    sc = et.scene(name)
    rays = sc.rays(which)
    n = rays.shape[0]
    check(monkeypatch, placed(name), rays, (n, et.prefix(n)), "%s %s" % (name, which))


@pytest.mark.parametrize("name,which", et.CASES)
def test_fast_and_generic_give_the_same_bytes(name, which):
    sc = et.scene(name)
    rays = sc.rays(which)
    dbvh = placed(name)
    for kernel in ("fermi_speculative_while_while", "kepler_dynamic_fetch"):
        for any_hit in (False, True):
            ref, _ = sc.reference(which, any_hit)
            with_flags, _ = gpu_trace(kernel, dbvh, rays, any_hit)
            without, _ = gpu_trace(kernel, dbvh, rays, any_hit, flags=0)
            assert with_flags.tobytes() == without.tobytes(), "%s %s %s anyHit=%d: flags 0x%x and 0 differ" % (name, which, kernel, any_hit, dbvh.flags)
            assert np.array_equal(without["id"], ref["id"]) and np.array_equal(without["t"].view(np.uint32), ref["t"].view(np.uint32))


@pytest.mark.parametrize("name,which", et.CASES)
def test_counters_equal_the_oracle(name, which):
    sc = et.scene(name)
    rays = sc.rays(which)
    dbvh = placed(name)
    d_rays = up(rays)
    for any_hit in (False, True):
        ref, rst = sc.reference(which, any_hit)
        d_res = torch.zeros(rays.shape[0] * 16, dtype=torch.uint8, device="cuda:0")
        st = dbvh.view.trace_stats("kepler_dynamic_fetch", rays.shape[0], any_hit, d_rays.data_ptr(), d_res.data_ptr())
        assert st.as_dict() == {k: v for k, v in rst.as_dict().items() if k != "maxStackDepth"}, (name, which, any_hit)
        got = d_res.cpu().numpy().view(nt.RESULT_DTYPE)
        assert np.array_equal(got["id"], ref["id"]) and np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32))


@pytest.mark.parametrize("name,which", et.CASES)
def test_wide_trace_equals_its_spec(name, which):
    from test_bvh_wide_gpu import _Tree, _assert_trace_equals_spec
    sc = et.scene(name)
    rays = sc.rays(which)
    if ("wide", name) not in _placed:
        _placed[("wide", name)] = _Tree(sc.nodes, sc.woop, sc.tri_index)
    t = _placed[("wide", name)]
    assert t.flags == expected_flags(sc.nodes)
    rid = _assert_trace_equals_spec(t, t.wide, rays, "%s %s" % (name, which))
    assert (rid >= 0).sum() >= rays.shape[0] // 10
