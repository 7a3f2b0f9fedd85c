"""ntr_bvh_optimize_batch and ntr_bvh_sah_cost_batch without a device: the symbols are in the header, the library and the package, the
result structs have the header's sizes, every NTR_ERR_INVALID case of both calls is refused before any device work (the pointers are
fakes, which a refused call never dereferences), overlapping and repeated node ranges are refused by the optimiser and allowed by the
cost, and after the checks the calls run only where there is a device to run them on."""
import ctypes as C
import os

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, FAKE2 = 0x10000, 0x4000000
RANGES = [(0, 640, 0, 1600), (704, 64, 1600, 80)]          # a gap of one node slot between them
OPT = dict(entries=RANGES, d_pool_nodes=FAKE, pool_nodes_bytes=768, passes=2)
SAH = dict(entries=RANGES, d_pool_nodes=FAKE, pool_nodes_bytes=768, d_pool_woop=FAKE2, pool_woop_bytes=1680)
NODE_CASES = [dict(entries=[]), dict(d_pool_nodes=0), dict(d_pool_nodes=FAKE + 8), dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700),
              dict(pool_nodes_bytes=0xFFFFFF40)] + \
             [dict(entries=[r]) for r in ((32, 640, 0, 1600), (0, 96, 0, 1600), (0, 0, 0, 1600), (-64, 640, 0, 1600), (192, 640, 0, 1600),
                                          (0, 832, 0, 1600))] + \
             [dict(entries=[(0, 0x76543240, 0, 1600)], pool_nodes_bytes=0x76543240)]          # inside the pool, above Compact's node limit


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def _code(call, kw):
    kw = {k: v for k, v in kw.items() if k != "what"}
    with pytest.raises(nt.NtrError) as e:
        call(**kw)
    return e.value.code, str(e.value)


def test_symbols_in_the_header_the_library_and_the_package():
    with open(os.path.join(ROOT, "include", "ntrace_amd.h")) as f:
        header = f.read()
    L = nt.lib()
    for name in ("ntr_bvh_optimize_batch", "ntr_bvh_optimize_batch_scratch_bytes", "ntr_bvh_sah_cost_batch"):
        assert "NTR_API int %s(" % name in header
        assert hasattr(L, name)
    for name in ("bvh_optimize_batch", "bvh_optimize_batch_scratch_bytes", "bvh_sah_cost_batch", "BvhOptimizeBatchEntry",
                 "BvhOptimizeBatchResult", "BvhSahBatchResult"):
        assert name in nt.__all__ and hasattr(nt, name)
    for name in ("NtrBvhOptimizeBatchEntry", "NtrBvhOptimizeBatchResult", "NtrBvhSahBatchResult"):
        assert "} %s;" % name in header
    assert (nt.OPT_ERR_LINK, nt.OPT_ERR_ROW, nt.OPT_ERR_NO_TREE) == (1, 2, 4)
    assert "NTR_OPT_ERR_LINK = 1, NTR_OPT_ERR_ROW = 2, NTR_OPT_ERR_NO_TREE = 4" in header


def test_the_bindings_shapes():
    """The header's layouts: 32 bytes per entry; two int32, sixteen int64, six int32, a float and a pad; five int32 and a float."""
    assert C.sizeof(nt.BvhOptimizeBatchEntry) == 32
    assert C.sizeof(nt.BvhOptimizeBatchResult) == 8 + 128 + 24 + 8 == 168
    assert nt.BvhOptimizeBatchResult.formed.offset == 8 and nt.BvhOptimizeBatchResult.rewritten.offset == 72
    assert nt.BvhOptimizeBatchResult.maxHeightBefore.offset == 136 and nt.BvhOptimizeBatchResult.seconds.offset == 160
    assert C.sizeof(nt.BvhSahBatchResult) == 24 and nt.BvhSahBatchResult.seconds.offset == 20
    r = nt.BvhOptimizeBatchResult()
    r.passes = 2
    r.formed[0], r.formed[1], r.formed[2] = 5, 1 << 40, 9
    d = r.as_dict()
    assert d["formed"] == [5, 1 << 40] and d["rewritten"] == [0, 0] and "pad" not in d
    assert set(nt.BvhOptimizeBatchEntry().as_dict()) == {"numNodes", "numLeafLinks", "heightBefore", "heightAfter", "errBits"}
    assert set(nt.BvhSahBatchResult().as_dict()) == {"numEntries", "firstBadEntry", "errBits", "launches", "readBacks", "seconds"}


def test_the_scratch_query():
    L = nt.lib()
    assert L.ntr_bvh_optimize_batch_scratch_bytes(None) == -1 and b"ntr_bvh_optimize_batch_scratch_bytes" in L.ntr_last_error()
    assert nt.bvh_optimize_batch_scratch_bytes() >= 0
    if not _has_device():
        assert nt.bvh_optimize_batch_scratch_bytes() == 0


def test_every_argument_error_of_the_optimiser():
    cases = NODE_CASES + [dict(passes=0), dict(passes=9), dict(passes=-1)]
    for change in cases:
        code, msg = _code(nt.bvh_optimize_batch, dict(OPT, **change))
        assert code == -1 and "ntr_bvh_optimize_batch" in msg, (change, code, msg)


def test_every_argument_error_of_the_cost():
    rows = [dict(d_pool_woop=0), dict(d_pool_woop=FAKE2 + 4), dict(pool_woop_bytes=0), dict(pool_woop_bytes=1688),
            dict(pool_woop_bytes=0xFFFFFF10)] + \
           [dict(entries=[r]) for r in ((0, 640, 8, 1600), (0, 640, 0, 1608), (0, 640, 0, 0), (0, 640, -16, 1600), (0, 640, 96, 1600),
                                        (0, 640, 0, 1696))]
    for change in NODE_CASES + rows:
        code, msg = _code(nt.bvh_sah_cost_batch, dict(SAH, **change))
        assert code == -1 and "ntr_bvh_sah_cost_batch" in msg, (change, code, msg)
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in RANGES])
    res = nt.BvhSahBatchResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    assert L.ntr_bvh_sah_cost_batch(2, C.cast(arr, C.c_void_p), FAKE, 768, FAKE2, 1680, None, C.byref(res), None) == -1
    assert b"null entryResults" in L.ntr_last_error() and bytes(res) == bytes(C.sizeof(res))
    assert L.ntr_bvh_sah_cost_batch(2, None, FAKE, 768, FAKE2, 1680, None, None, None) == -1


def test_overlapping_and_repeated_node_ranges_are_refused_by_the_optimiser_only():
    for entries, pair in (([RANGES[0], RANGES[1], RANGES[0]], "0 and 2"), ([RANGES[1], (0, 640, 0, 1600), (576, 128, 0, 16)], "1 and 2"),
                          ([(64, 64, 0, 16), (0, 128, 0, 16)], "0 and 1")):
        code, msg = _code(nt.bvh_optimize_batch, dict(OPT, entries=entries))
        assert code == -1 and "overlap" in msg and pair in msg, (entries, msg)
    # ranges that only touch are fine: with a device the call would run, so only the refusal's absence is checked here
    if not _has_device():
        code, msg = _code(nt.bvh_optimize_batch, dict(OPT, entries=[(0, 640, 0, 16), (640, 128, 0, 16)]))
        assert code in (-2, -3), msg
        code, msg = _code(nt.bvh_sah_cost_batch, dict(SAH, entries=[RANGES[0], RANGES[0], (0, 128, 0, 160)]))
        assert code in (-2, -3), msg


def test_refused_calls_zero_their_outputs():
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in RANGES])
    res = nt.BvhOptimizeBatchResult()
    per = (nt.BvhOptimizeBatchEntry * 2)()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    C.memset(per, 0xFF, C.sizeof(per))
    assert L.ntr_bvh_optimize_batch(2, C.cast(arr, C.c_void_p), FAKE, 768, 9, C.cast(per, C.c_void_p), C.byref(res), None) == -1
    assert b"passes" in L.ntr_last_error()
    assert bytes(res) == bytes(C.sizeof(res)) and bytes(per) == bytes(C.sizeof(per))
    # numEntries has a limit, checked before any entry is read (the array here holds two)
    assert L.ntr_bvh_optimize_batch((1 << 20) + 1, C.cast(arr, C.c_void_p), FAKE, 768, 2, None, C.byref(res), None) == -1
    assert b"numEntries" in L.ntr_last_error()
    sah = (nt.BvhSahResult * 2)()
    assert L.ntr_bvh_sah_cost_batch((1 << 20) + 1, C.cast(arr, C.c_void_p), FAKE, 768, FAKE2, 1680, C.cast(sah, C.c_void_p), None, None) == -1
    assert b"numEntries" in L.ntr_last_error()
    # NULL outputs are allowed: the refusal is the same
    assert L.ntr_bvh_optimize_batch(2, C.cast(arr, C.c_void_p), FAKE, 768, 9, None, None, None) == -1


def test_after_the_checks_there_is_no_cpu_fallback():
    if _has_device():
        return                                   # the accepted calls would run on the fake pointers: test_optimize_batch_gpu.py runs them
    for call, kw in ((nt.bvh_optimize_batch, OPT), (nt.bvh_sah_cost_batch, SAH)):
        with pytest.raises(nt.NtrError) as e:
            call(**kw)
        assert e.value.code in (-2, -3), str(e.value)
        assert e.value.result is not None and e.value.entry_results is not None and len(e.value.entry_results) == 2
        assert bytes(e.value.result) == bytes(C.sizeof(e.value.result))
    assert nt.bvh_optimize_batch_scratch_bytes() == 0
