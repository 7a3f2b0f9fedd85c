"""ntr_ploc_build_batch without a device: ntr_ploc_batch_capacity is host arithmetic and equals the spec (tests/np_ploc_batch.py) in extents
and ranges; every argument error that is decided before device work is reported with a message, whether or not a device is present; the
symbols are exported."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt

import np_ploc_batch as pb

UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _meshes(num_tris):
    out, first = [], 0
    for n in num_tris:
        out.append((first, n) + UNIT)
        first += n
    return out


@pytest.mark.parametrize("num_tris", [[1], [2], [1, 1], [1000, 48, 1, 2000, 3, 1, 1, 70], [1, 5, 1, 1, 2, 1], [7] * 300])
def test_capacity_equals_spec(num_tris):
    want = pb.capacity(num_tris)
    got = nt.ploc_batch_capacity(_meshes(num_tris))
    assert got[:3] == want[:3] and got[3] == want[3]
    for (no, nb, wo, wb), n in zip(got[3], num_tris):
        assert nb == 64 * max(n - 1, 1) and wb == 16 * (5 if n == 1 else 4 * n) and no % 64 == 0 and wo % 16 == 0


def test_capacity_of_the_most_meshes():
    m = pb.MAX_MESHES
    arr = (nt.PlocBatchMesh * m)()
    view = np.frombuffer(arr, np.int32).reshape(m, 8)
    view[:, 0] = np.arange(m)
    view[:, 1] = 1
    ranges = (nt.BlasRange * m)()
    a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    L = nt.lib()
    assert L.ntr_ploc_batch_capacity(m, C.cast(arr, C.c_void_p), C.cast(ranges, C.c_void_p), C.byref(a), C.byref(b), C.byref(c)) == 0
    assert (a.value, b.value, c.value) == (64 * m, 80 * m, 20 * m) == pb.capacity(np.ones(m, np.int64))[:3]
    got = np.frombuffer(ranges, np.int64).reshape(m, 4)
    k = np.arange(m, dtype=np.int64)
    assert np.array_equal(got, np.stack([64 * k, np.full(m, 64), 80 * k, np.full(m, 80)], axis=1))
    # no ranges asked for, no extents asked for
    assert L.ntr_ploc_batch_capacity(m, C.cast(arr, C.c_void_p), None, None, None, None) == 0
    assert L.ntr_ploc_batch_capacity(m + 1, C.cast(arr, C.c_void_p), None, C.byref(a), C.byref(b), C.byref(c)) == -1


def test_capacity_errors():
    for bad, code in (([], -1), (_meshes([4, 0, 4]), -1), (_meshes([4, -3]), -1), (_meshes([1 << 27, 1 << 27]), -1),
                      (_meshes([0x76543200 // 64 + 2]), -6), (_meshes([25_000_000] * 3), -6)):
        with pytest.raises(nt.NtrError) as e:
            nt.ploc_batch_capacity(bad)
        assert e.value.code == code and "ntr_ploc_batch_capacity" in str(e.value), (bad[:2], str(e.value))
    assert nt.lib().ntr_ploc_batch_capacity(1, None, None, None, None, None) == -1
    nt.ploc_batch_capacity(_meshes([0x76543200 // 64 + 1]))      # the most nodes a BLAS may have


def test_argument_errors_are_decided_before_device_work():
    """The pointers are never dereferenced: every call here is refused on the host."""
    meshes = _meshes([5, 1, 3])
    caps = pb.capacity([5, 1, 3])
    fake = 0x10000
    good = dict(meshes=meshes, num_tris_total=9, d_tri=fake, num_verts=20, d_pos=fake, d_pool_nodes=fake, nodes_cap=caps[0], d_pool_woop=fake,
                woop_cap=caps[1], d_pool_idx=fake, idx_cap=caps[2], radius=8)

    def mesh(k, **change):
        m = [list(x) for x in meshes]
        for key, v in change.items():
            m[k][dict(first=0, n=1, mn=2, mx=3)[key]] = v
        return [tuple(x) for x in m]

    cases = [(dict(d_tri=0), -1), (dict(d_pos=0), -1), (dict(d_pool_nodes=0), -1), (dict(d_pool_woop=0), -1), (dict(d_pool_idx=0), -1),
             (dict(num_tris_total=0), -1), (dict(num_verts=0), -1), (dict(meshes=[]), -1), (dict(radius=0), -1), (dict(radius=65), -1),
             (dict(radius=-1), -1), (dict(meshes=mesh(1, n=0)), -1), (dict(meshes=mesh(0, first=-1)), -1), (dict(meshes=mesh(2, first=7)), -1),
             (dict(num_tris_total=8), -1), (dict(meshes=mesh(1, mx=(1.0, np.inf, 1.0))), -1), (dict(meshes=mesh(2, mn=(0.0, 0.0, np.nan))), -1),
             (dict(meshes=mesh(0, mn=(2.0, 0.0, 0.0))), -1), (dict(nodes_cap=caps[0] - 1), -1), (dict(woop_cap=caps[1] - 1), -1),
             (dict(idx_cap=caps[2] - 1), -1), (dict(d_pool_nodes=fake + 4), -1), (dict(d_pool_woop=fake + 8), -1),
             (dict(meshes=_meshes([1 << 27, 1 << 27]), num_tris_total=1 << 28), -1),
             (dict(meshes=[(0, 25_000_000) + UNIT] * 3, num_tris_total=25_000_000, nodes_cap=1 << 40, woop_cap=1 << 40, idx_cap=1 << 40), -6),
             (dict(meshes=[(0, 0x76543200 // 64 + 2) + UNIT], num_tris_total=1 << 27, nodes_cap=1 << 40, woop_cap=1 << 40, idx_cap=1 << 40), -6)]
    for change, code in cases:
        with pytest.raises(nt.NtrError) as e:
            nt.ploc_build_batch(**dict(good, **change))
        assert e.value.code == code and "ntr_ploc_build_batch" in str(e.value), (change, str(e.value))
    # null meshes, ranges and result through the raw entry point; a failed call zeroes *result
    L = nt.lib()
    arr = (nt.PlocBatchMesh * 3)(*[nt.PlocBatchMesh(*m) for m in meshes])
    ranges = (nt.BlasRange * 3)()
    res = nt.PlocBatchResult()
    tail = (fake, caps[0], fake, caps[1], fake, caps[2])
    for marr, rng in ((None, ranges), (arr, None)):
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        assert L.ntr_ploc_build_batch(3, C.cast(marr, C.c_void_p), 9, fake, 20, fake, 8, *tail, C.cast(rng, C.c_void_p), None, C.byref(res), None) == -1
        assert bytes(res) == bytes(C.sizeof(res)) and b"ntr_ploc_build_batch" in L.ntr_last_error()
    assert L.ntr_ploc_build_batch(3, C.cast(arr, C.c_void_p), 9, fake, 20, fake, 8, *tail, C.cast(ranges, C.c_void_p), None, None, None) == -1


def test_symbols_and_the_scratch_query():
    L = nt.lib()
    for name in ("ntr_ploc_batch_capacity", "ntr_ploc_build_batch", "ntr_ploc_batch_scratch_bytes"):
        assert hasattr(L, name)
    assert L.ntr_ploc_batch_scratch_bytes(None) == -1 and b"ntr_ploc_batch_scratch_bytes" in L.ntr_last_error()
    assert C.sizeof(nt.PlocBatchMesh) == 32 and C.sizeof(nt.PlocBatchMeshResult) == 16 and C.sizeof(nt.PlocBatchResult) == 72
