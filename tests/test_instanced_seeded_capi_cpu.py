"""The four seeded entry points without a device: ntr_trace_instanced_seeded, ntr_trace_instanced_seeded_stats,
ntr_trace_instanced_wide_seeded and ntr_trace_instanced_wide_seeded_stats refuse, before any device work, everything their unseeded
siblings refuse plus a seed buffer that is null or not 16-byte aligned; numRays == 0 is NTR_OK; the bindings marshal every argument in
its place.  Pointers are never dereferenced by a refused call; the accepted call runs only where there is no device to run it on."""
import ctypes as C

import pytest

import ntrace_amd as nt

FAKE = 0x10000
BINARY = dict(num_rays=64, any_hit=False, d_rays=FAKE, d_seed_results=FAKE, seed_instance=5, d_results=FAKE, d_instance_ids=FAKE, d_tlas_nodes=FAKE,
              tlas_nodes_bytes=256, root_link=0, d_records=FAKE, num_instances=5, d_pool_nodes=FAKE, pool_nodes_bytes=704, d_pool_woop=FAKE,
              pool_woop_bytes=1680, d_pool_tri_index=FAKE)
WIDE = dict(num_rays=64, any_hit=False, d_rays=FAKE, d_seed_results=FAKE, seed_instance=5, d_results=FAKE, d_instance_ids=FAKE, d_wide_tlas_nodes=FAKE,
            wide_tlas_nodes_bytes=256, root_link=0, d_wide_records=FAKE, num_instances=5, d_wide_pool_nodes=FAKE, wide_pool_nodes_bytes=1408,
            d_pool_woop=FAKE, pool_woop_bytes=1680, d_pool_tri_index=FAKE)
# what the unseeded siblings refuse (test_instanced_masked_cpu.py, test_instanced_wide_cpu.py), and the two seed refusals
COMMON = [dict(num_rays=-1), dict(d_rays=0), dict(d_results=0), dict(d_instance_ids=0), dict(num_instances=0), dict(root_link=~5),
          dict(pool_woop_bytes=8), dict(pool_woop_bytes=0xFFFFFF10), dict(d_pool_tri_index=0), dict(d_pool_woop=0),
          dict(vis=nt.InstanceVisibility(FAKE + 2, 0)), dict(vis=nt.InstanceVisibility(0, FAKE + 1)), dict(vis=nt.InstanceVisibility(FAKE, FAKE + 3, 1))]
SEED = [dict(d_seed_results=0), dict(d_seed_results=FAKE + 8), dict(d_seed_results=FAKE + 4), dict(d_seed_results=FAKE + 1)]
CASES = {
    "binary": (BINARY, COMMON + SEED + [dict(d_records=0), dict(root_link=64), dict(tlas_nodes_bytes=0), dict(tlas_nodes_bytes=100), dict(d_tlas_nodes=0),
                                        dict(d_pool_nodes=0), dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700), dict(pool_nodes_bytes=0xFFFFFF40)]),
    "wide": (WIDE, COMMON + SEED + [dict(d_wide_records=0), dict(root_link=128), dict(wide_tlas_nodes_bytes=0), dict(wide_tlas_nodes_bytes=192),
                                    dict(wide_tlas_nodes_bytes=0x76543280), dict(d_wide_tlas_nodes=0), dict(d_wide_pool_nodes=0),
                                    dict(wide_pool_nodes_bytes=0), dict(wide_pool_nodes_bytes=1344), dict(wide_pool_nodes_bytes=0xFFFFFF80)]),
}
CALLS = {("binary", False): ("trace_instanced_seeded", "ntr_trace_instanced_seeded"),
         ("binary", True): ("trace_instanced_seeded_stats", "ntr_trace_instanced_seeded_stats"),
         ("wide", False): ("trace_instanced_wide_seeded", "ntr_trace_instanced_wide_seeded"),
         ("wide", True): ("trace_instanced_wide_seeded_stats", "ntr_trace_instanced_wide_seeded_stats")}


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("form", ["binary", "wide"])
def test_refusals_come_before_any_device_work(form, stats):
    call = getattr(nt, CALLS[form, stats][0])
    good, changes = CASES[form]
    for vis in (None, nt.InstanceVisibility(FAKE, FAKE, 3)):
        for change in changes:
            with pytest.raises(nt.NtrError) as e:
                call(**dict(dict(good, vis=vis), **change))
            assert e.value.code == -1, (change, str(e.value))
    with pytest.raises(nt.NtrError) as e:
        call(**dict(good, d_seed_results=FAKE + 8))
    assert "seed" in str(e.value) and CALLS[form, stats][1] in str(e.value)
    # in place is no error, and neither is any seed instance: past the checks the call fails only for want of a device
    if not _has_device():
        for kw in (good, dict(good, seed_instance=-2), dict(good, seed_instance=5), dict(good, d_results=good["d_seed_results"]),
                   dict(good, root_link=~0, **({"d_tlas_nodes": 0, "tlas_nodes_bytes": 0} if form == "binary" else
                                              {"d_wide_tlas_nodes": 0, "wide_tlas_nodes_bytes": 0})),
                   dict(good, vis=nt.InstanceVisibility(FAKE, FAKE, 3))):
            with pytest.raises(nt.NtrError) as e:
                call(**kw)
            assert e.value.code in (-2, -3), str(e.value)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("form", ["binary", "wide"])
def test_zero_rays_and_null_stats(form, stats):
    call = getattr(nt, CALLS[form, stats][0])
    good = CASES[form][0]
    # numRays == 0 returns NTR_OK whatever else is passed, as the unseeded siblings do
    zero = call(**dict(good, num_rays=0))
    assert bytes(zero) == bytes(64) if stats else zero == 0.0
    zero = call(**dict(good, num_rays=0, d_seed_results=0))
    assert bytes(zero) == bytes(64) if stats else zero == 0.0
    if not stats:
        assert call(**dict(good, num_rays=0, timed=False)) is None
        return
    L = nt.lib()
    fn = getattr(L, CALLS[form, True][1])
    args = (64, 0, FAKE, FAKE, 5, FAKE, FAKE, FAKE, 256, 0, FAKE, 5, FAKE, 704 if form == "binary" else 1408, FAKE, 1680, FAKE)
    assert fn(*args, None, None, None) == -1 and b"null stats" in L.ntr_last_error()
    st = nt.InstancedTraceStats() if form == "binary" else nt.InstancedWideTraceStats()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    assert fn(*(args[:3] + (0,) + args[4:]), None, C.byref(st), None) == -1 and bytes(st) == bytes(64)      # refused: the stats zeroed


def test_the_bindings_marshal_every_argument_in_its_place():
    """Each refusal names its argument, so a wrapper that passed two arguments in each other's place would refuse the wrong change: the
    seed pointer and the result pointer are told apart by alignment, the seed instance passes between them untouched."""
    L = nt.lib()
    for (form, stats), (py, c) in CALLS.items():
        assert callable(getattr(nt, py)) and py in nt.__all__
        fn = getattr(L, c)
        assert fn.restype is C.c_int and len(fn.argtypes) == 20 and fn.argtypes[4] is C.c_int32 and fn.argtypes[3] is C.c_void_p
        good = CASES[form][0]
        for change, word in ((dict(d_seed_results=FAKE + 8), "seed"), (dict(d_results=0), "result"), (dict(d_instance_ids=0), "instance id"),
                             (dict(root_link=~5, seed_instance=0), "rootLink"), (dict(num_instances=0, seed_instance=3), "no instances")):
            with pytest.raises(nt.NtrError) as e:
                getattr(nt, py)(**dict(good, **change))
            assert e.value.code == -1 and word in str(e.value), (py, change, str(e.value))
        # a misaligned result buffer is not the seed's business: d_results = seed + 8 passes the checks
        if not _has_device():
            with pytest.raises(nt.NtrError) as e:
                getattr(nt, py)(**dict(good, d_results=FAKE + 8))
            assert e.value.code in (-2, -3)
