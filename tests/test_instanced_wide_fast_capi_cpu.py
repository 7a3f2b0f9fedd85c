"""The entry points of the FAST wide two-level trace without a device: ntr_instanced_wide_validate, ntr_trace_instanced_wide_fast and
ntr_trace_instanced_wide_fast_stats exist; each refuses with NTR_ERR_INVALID, before any device work, what include/ntrace_amd.h says it
refuses; a refused or a zero-ray stats call leaves both stats zeroed; past the checks a call fails only for want of a device (no CPU
fallback).  Pointers are never dereferenced by a refused call."""
import ctypes as C

import pytest

import ntrace_amd as nt

FAKE = 0x10000
GOOD = dict(num_rays=64, any_hit=False, d_rays=FAKE, d_results=FAKE, d_instance_ids=FAKE, d_wide_tlas_nodes=FAKE, wide_tlas_nodes_bytes=256,
            root_link=0, d_wide_records=FAKE, num_instances=5, d_wide_pool_nodes=FAKE, wide_pool_nodes_bytes=768, d_pool_woop=FAKE,
            pool_woop_bytes=1680, d_pool_tri_index=FAKE, d_flags=FAKE)
# everything ntr_trace_instanced_wide_seeded refuses but a null seed, and the flag refusals
REFUSED = [dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_instance_ids=0), dict(num_instances=0), dict(root_link=~5),
           dict(pool_woop_bytes=8), dict(pool_woop_bytes=0xFFFFFF10), dict(d_pool_tri_index=0), dict(d_pool_woop=0),
           dict(vis=nt.InstanceVisibility(FAKE + 2, 0)), dict(vis=nt.InstanceVisibility(0, FAKE + 1)), dict(vis=nt.InstanceVisibility(FAKE, FAKE + 3, 1)),
           dict(d_seed_results=FAKE + 8), dict(d_seed_results=FAKE + 4), dict(d_seed_results=FAKE + 1),
           dict(d_wide_records=0), dict(root_link=128), dict(wide_tlas_nodes_bytes=0), dict(wide_tlas_nodes_bytes=192), dict(wide_tlas_nodes_bytes=-128),
           dict(wide_tlas_nodes_bytes=0x76543280), dict(d_wide_tlas_nodes=0), dict(d_wide_pool_nodes=0),
           dict(wide_pool_nodes_bytes=0), dict(wide_pool_nodes_bytes=704), dict(wide_pool_nodes_bytes=0xFFFFFF80),
           dict(d_flags=0), dict(d_flags=FAKE + 4), dict(d_flags=FAKE + 8), dict(d_flags=FAKE + 1)]
TRACE_ARGS = (64, 0, FAKE, None, -1, FAKE, FAKE, FAKE, 256, 0, FAKE, 5, FAKE, 768, FAKE, 1680, FAKE, None)


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols():
    L = nt.lib()
    for py, c, nargs in (("instanced_wide_validate", "ntr_instanced_wide_validate", 6),
                         ("trace_instanced_wide_fast", "ntr_trace_instanced_wide_fast", 21),
                         ("trace_instanced_wide_fast_stats", "ntr_trace_instanced_wide_fast_stats", 22)):
        assert callable(getattr(nt, py)) and py in nt.__all__
        fn = getattr(L, c)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs, c
    assert C.sizeof(nt.InstancedFastStats) == 32 and C.sizeof(nt.InstancedWideTraceStats) == 64


@pytest.mark.parametrize("stats", [False, True])
def test_the_trace_refuses_before_any_device_work(stats):
    call = nt.trace_instanced_wide_fast_stats if stats else nt.trace_instanced_wide_fast
    for base in (GOOD, dict(GOOD, d_seed_results=FAKE, seed_instance=5), dict(GOOD, vis=nt.InstanceVisibility(FAKE, FAKE, 3))):
        for change in REFUSED:
            with pytest.raises(nt.NtrError) as e:
                call(**dict(base, **change))
            assert e.value.code == -1, (change, str(e.value))
    with pytest.raises(nt.NtrError) as e:
        call(**dict(GOOD, d_flags=FAKE + 8))
    assert "flags" in str(e.value) and ("ntr_trace_instanced_wide_fast_stats" if stats else "ntr_trace_instanced_wide_fast:") in str(e.value)
    # no seed, a seed, in place, one instance without a top-level node, masks: past the checks the call fails only for want of a device
    if not _has_device():
        for kw in (GOOD, dict(GOOD, d_seed_results=FAKE, seed_instance=-2), dict(GOOD, d_seed_results=FAKE, d_results=FAKE),
                   dict(GOOD, root_link=~0, d_wide_tlas_nodes=0, wide_tlas_nodes_bytes=0), dict(GOOD, vis=nt.InstanceVisibility(FAKE, FAKE, 3))):
            with pytest.raises(nt.NtrError) as e:
                call(**kw)
            assert e.value.code in (-2, -3), str(e.value)


def test_zero_rays_null_stats_and_zeroed_stats_on_failure():
    assert nt.trace_instanced_wide_fast(**dict(GOOD, num_rays=0)) == 0.0
    assert nt.trace_instanced_wide_fast(**dict(GOOD, num_rays=0, timed=False)) is None
    st, fs = nt.trace_instanced_wide_fast_stats(**dict(GOOD, num_rays=0, d_flags=0))     # numRays == 0 returns NTR_OK whatever else is passed
    assert isinstance(st, nt.InstancedWideTraceStats) and bytes(st) == bytes(64) and bytes(fs) == bytes(32)
    L = nt.lib()
    fn = L.ntr_trace_instanced_wide_fast_stats
    st, fs = nt.InstancedWideTraceStats(), nt.InstancedFastStats()
    for a, b in ((None, None), (C.byref(st), None), (None, C.byref(fs))):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(fs), 0xFF, C.sizeof(fs))
        assert fn(*TRACE_ARGS, FAKE, a, b, None) == -1 and b"null stats" in L.ntr_last_error()
        assert (a is None or bytes(st) == bytes(64)) and (b is None or bytes(fs) == bytes(32))
    # refused for its flags, and failing for want of a device: both stats zeroed
    for flags in (None, FAKE) if not _has_device() else (None,):
        C.memset(C.byref(st), 0xFF, C.sizeof(st))
        C.memset(C.byref(fs), 0xFF, C.sizeof(fs))
        assert fn(*TRACE_ARGS, flags, C.byref(st), C.byref(fs), None) in ((-1,) if flags is None else (-2, -3))
        assert bytes(st) == bytes(64) and bytes(fs) == bytes(32)


def test_wide_validate_refuses_before_any_device_work():
    good = dict(d_wide_tlas_nodes=FAKE, wide_tlas_nodes_bytes=256, d_wide_pool_nodes=FAKE, wide_pool_nodes_bytes=768, d_flags=FAKE)
    for change in (dict(d_flags=0), dict(d_wide_pool_nodes=0), dict(wide_tlas_nodes_bytes=192), dict(wide_tlas_nodes_bytes=100),
                   dict(wide_tlas_nodes_bytes=-128), dict(wide_tlas_nodes_bytes=0x76543280), dict(wide_pool_nodes_bytes=0),
                   dict(wide_pool_nodes_bytes=704), dict(wide_pool_nodes_bytes=-128), dict(wide_pool_nodes_bytes=0xFFFFFF80), dict(d_flags=FAKE + 4),
                   dict(d_flags=FAKE + 8), dict(d_wide_tlas_nodes=FAKE + 8), dict(d_wide_pool_nodes=FAKE + 4)):
        with pytest.raises(nt.NtrError) as e:
            nt.instanced_wide_validate(**dict(good, **change))
        assert e.value.code == -1 and "ntr_instanced_wide_validate" in str(e.value), (change, str(e.value))
    if not _has_device():                                # no top level, and the largest sizes: accepted, and then there is no device
        for kw in (good, dict(good, d_wide_tlas_nodes=0, wide_tlas_nodes_bytes=0), dict(good, d_wide_tlas_nodes=0),
                   dict(good, wide_tlas_nodes_bytes=0x76543200), dict(good, wide_pool_nodes_bytes=0xFFFFFF00)):
            with pytest.raises(nt.NtrError) as e:
                nt.instanced_wide_validate(**kw)
            assert e.value.code in (-2, -3), str(e.value)
