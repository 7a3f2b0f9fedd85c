"""ntr_pool_widen_batch without a device: the symbols are in the header, the library and the package; every NTR_ERR_INVALID case of
ntr_pool_widen (test_instanced_wide_cpu.py's table, with its fake pointers, which a refused call never dereferences) is refused by the
batched call too, with numBlas > 2^20 on top, and the outputs are zeroed; after the checks the call runs only where there is no
device to run it on."""
import ctypes as C
import os

import pytest

import ntrace_amd as nt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE, FAKE2 = 0x10000, 0x4000000
RANGES = [(0, 640, 0, 1600), (640, 64, 1600, 80)]
GOOD = dict(ranges=RANGES, d_pool_nodes=FAKE, pool_nodes_bytes=704, d_wide_pool_nodes=FAKE2, capacity=128 * 11)


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols_in_the_header_the_library_and_the_package():
    with open(os.path.join(ROOT, "include", "ntrace_amd.h")) as f:
        header = f.read()
    L = nt.lib()
    for name in ("ntr_pool_widen_batch", "ntr_pool_widen_batch_scratch_bytes"):
        assert "NTR_API int %s(" % name in header
        assert hasattr(L, name)
    assert callable(nt.pool_widen_batch) and callable(nt.pool_widen_batch_scratch_bytes)
    assert "pool_widen_batch" in nt.__all__ and "pool_widen_batch_scratch_bytes" in nt.__all__
    assert L.ntr_pool_widen_batch_scratch_bytes(None) == -1 and b"ntr_pool_widen_batch_scratch_bytes" in L.ntr_last_error()


def test_every_argument_error_of_the_loop_is_refused_by_the_batch():
    bad_ranges = [[(32, 640, 0, 1600)], [(0, 96, 0, 1600)], [(0, 0, 0, 1600)], [(640, 128, 0, 1600)], [(0, 640, 8, 1600)], [(0, 640, 0, 1608)],
                  [(-64, 640, 0, 1600)], [(0, 640, -16, 1600)], [(0, 640, 0xFFFFFF00, 1600)], [(0, 640, 0, 0)]]
    cases = [dict(ranges=[]), dict(d_pool_nodes=0), dict(d_wide_pool_nodes=0), dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=700),
             dict(pool_nodes_bytes=0xFFFFFF40), dict(capacity=128 * 11 - 1), dict(d_wide_pool_nodes=FAKE + 64)] + [dict(ranges=r) for r in bad_ranges]
    for change in cases:
        kw = dict(GOOD, **change)
        codes = []
        for call in (nt.pool_widen, nt.pool_widen_batch):       # the loop refuses it, and so does the batch
            with pytest.raises(nt.NtrError) as e:
                call(**kw)
            codes.append(e.value.code)
        assert codes == [-1, -1], (change, codes)
        assert "ntr_pool_widen_batch" in str(e.value)


def test_refused_calls_zero_their_outputs_and_numblas_has_a_limit():
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in RANGES])
    out = (nt.WideBlasRange * 2)()
    res = nt.BvhWideResult()

    def fill():
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        C.memset(out, 0xFF, C.sizeof(out))
    fill()
    assert L.ntr_pool_widen_batch(2, C.cast(arr, C.c_void_p), FAKE, 704, FAKE2, 128 * 11, None, C.byref(res), None) == -1
    assert bytes(res) == bytes(C.sizeof(res))
    assert L.ntr_pool_widen_batch(2, C.cast(arr, C.c_void_p), FAKE, 704, FAKE2, 128 * 11, C.cast(out, C.c_void_p), None, None) == -1
    assert L.ntr_pool_widen_batch(2, None, FAKE, 704, FAKE2, 128 * 11, C.cast(out, C.c_void_p), C.byref(res), None) == -1
    # a failure behind the first check zeroes both outputs: a capacity one byte short, an output inside the pool
    for cap, d_wide in ((128 * 11 - 1, FAKE2), (128 * 11, FAKE + 64)):
        fill()
        assert L.ntr_pool_widen_batch(2, C.cast(arr, C.c_void_p), FAKE, 704, d_wide, cap, C.cast(out, C.c_void_p), C.byref(res), None) == -1
        assert bytes(res) == bytes(C.sizeof(res)) and bytes(out) == bytes(C.sizeof(out))
    # numBlas: 2^20 ranges pass this check (and fail the next: the second range is read), 2^20 + 1 do not (and nothing is read or written
    # beyond the result: the arrays here hold two entries)
    fill()
    assert L.ntr_pool_widen_batch((1 << 20) + 1, C.cast(arr, C.c_void_p), FAKE, 704, FAKE2, 128 * 11, C.cast(out, C.c_void_p), C.byref(res), None) == -1
    assert b"exceeds 1048576" in L.ntr_last_error() and bytes(res) == bytes(C.sizeof(res))
    big = (nt.BlasRange * (1 << 20))()                           # all-zero ranges: BLAS 0 is refused, not the count
    big_out = (nt.WideBlasRange * (1 << 20))()
    assert L.ntr_pool_widen_batch(1 << 20, C.cast(big, C.c_void_p), FAKE, 704, FAKE2, 128 * 11, C.cast(big_out, C.c_void_p), C.byref(res), None) == -1
    assert b"BLAS 0" in L.ntr_last_error()
    with pytest.raises(nt.NtrError) as e:
        nt.pool_widen_batch(**dict(GOOD, ranges=[RANGES[1]] * ((1 << 20) + 1), capacity=128 * ((1 << 20) + 1)))
    assert e.value.code == -1 and "exceeds" in str(e.value)


def test_after_the_checks_there_is_no_cpu_fallback():
    if _has_device():
        return                                   # the accepted call would run on the fake pointers: test_pool_widen_batch_gpu.py runs it
    with pytest.raises(nt.NtrError) as e:
        nt.pool_widen_batch(**GOOD)
    assert e.value.code in (-2, -3), str(e.value)
    L = nt.lib()
    arr = (nt.BlasRange * 2)(*[nt.BlasRange(*r) for r in RANGES])
    out = (nt.WideBlasRange * 2)()
    res = nt.BvhWideResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    C.memset(out, 0xFF, C.sizeof(out))
    rc = L.ntr_pool_widen_batch(2, C.cast(arr, C.c_void_p), FAKE, 704, FAKE2, 128 * 11, C.cast(out, C.c_void_p), C.byref(res), None)
    assert rc in (-2, -3) and bytes(res) == bytes(C.sizeof(res)) and bytes(out) == bytes(C.sizeof(out))
    assert nt.pool_widen_batch_scratch_bytes() == 0
