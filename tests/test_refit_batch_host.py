"""ntr_bvh_refit_batch without a device: the symbols are exported; every argument error that is decided before device work is reported
with a message, whether or not a device is present (overlapping and duplicate entries and a count of 2^20 + 1 among them); and the rule
(tests/np_refit_batch.py) over a PLOC batch with unmoved vertices and epsilon 0 returns the pool unchanged."""
import ctypes as C

import numpy as np
import pytest

import ntrace_amd as nt
from ntrace_amd import scenes

import np_ploc_batch as pb
import np_refit_batch as rb

F = np.float32


def _has_device():
    cnt = C.c_int(-1)
    return nt.lib().ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0


def test_symbols_structures_and_the_scratch_query():
    L = nt.lib()
    for name in ("ntr_bvh_refit_batch", "ntr_bvh_refit_batch_scratch_bytes"):
        assert hasattr(L, name)
    assert C.sizeof(nt.RefitBatchEntry) == 48 and C.sizeof(nt.BvhRefitBatchResult) == 48
    assert L.ntr_bvh_refit_batch_scratch_bytes(None) == -1 and b"ntr_bvh_refit_batch_scratch_bytes" in L.ntr_last_error()
    if not _has_device():
        assert nt.bvh_refit_batch_scratch_bytes() == 0
    e = nt.RefitBatchEntry((64, 128, 16, 32), 3, 5, 0.5)
    assert (e.range.nodesOffset, e.range.nodesBytes, e.range.triWoopOffset, e.range.triWoopBytes) == (64, 128, 16, 32)
    assert (e.firstTri, e.numTris, e.epsilon, e.pad) == (3, 5, 0.5, 0)


def test_argument_errors_are_decided_before_device_work():
    """The pointers are never dereferenced: every call here is refused on the host, in the blocking and the asynchronous form."""
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data
    # three BLASes of 5, 1 and 3 triangles as ntr_ploc_build_batch lays them out
    _, _, _, ranges = pb.capacity([5, 1, 3])
    first = (0, 5, 6)
    entries = [(r, f, n, 0.0) for r, f, n in zip(ranges, first, (5, 1, 3))]
    nodes_bytes = ranges[-1][0] + ranges[-1][1]
    woop_bytes = ranges[-1][2] + ranges[-1][3]
    good = dict(entries=entries, d_pool_nodes=fake, pool_nodes_bytes=nodes_bytes, d_pool_woop=fake, pool_woop_bytes=woop_bytes,
                d_pool_idx=fake, num_tris_total=9, d_tri=fake, num_verts=20, d_pos=fake)

    def entry(k, rng=None, **change):
        out = [list(x) for x in entries]
        if rng is not None:
            r = list(out[k][0])
            for key, v in rng.items():
                r[dict(no=0, nb=1, wo=2, wb=3)[key]] = v
            out[k][0] = tuple(r)
        for key, v in change.items():
            out[k][dict(first=1, n=2, eps=3)[key]] = v
        return [tuple(x) for x in out]

    cases = [dict(entries=[]), dict(d_pool_nodes=0), dict(d_pool_woop=0), dict(d_pool_idx=0), dict(d_tri=0), dict(d_pos=0),
             dict(num_tris_total=0), dict(num_verts=0), dict(num_verts=-3),
             dict(pool_nodes_bytes=0), dict(pool_nodes_bytes=nodes_bytes + 8), dict(pool_nodes_bytes=0xFFFFFF00 + 64),
             dict(pool_woop_bytes=0), dict(pool_woop_bytes=woop_bytes + 4), dict(pool_woop_bytes=0xFFFFFF00 + 16),
             dict(d_pool_nodes=fake + 4), dict(d_pool_woop=fake + 8),
             # a range that is misaligned, outside the pool's extents or above the limits; triWoopBytes < 16
             dict(entries=entry(1, rng=dict(no=ranges[1][0] + 32))), dict(entries=entry(1, rng=dict(nb=96))), dict(entries=entry(0, rng=dict(nb=0))),
             dict(entries=entry(0, rng=dict(no=-64))), dict(entries=entry(2, rng=dict(nb=ranges[2][1] + 64))),
             dict(entries=entry(2, rng=dict(no=nodes_bytes))), dict(entries=entry(0, rng=dict(nb=0x76543200 + 64)), pool_nodes_bytes=0xFFFFFF00 - 192),
             dict(entries=entry(1, rng=dict(wo=ranges[1][2] + 8))), dict(entries=entry(1, rng=dict(wb=0))), dict(entries=entry(1, rng=dict(wb=8))),
             dict(entries=entry(1, rng=dict(wb=24))), dict(entries=entry(0, rng=dict(wo=-16))), dict(entries=entry(2, rng=dict(wb=ranges[2][3] + 16))),
             dict(entries=entry(2, rng=dict(wo=woop_bytes))),
             # a mesh outside [0, numTrisTotal) or with numTris < 1
             dict(entries=entry(1, n=0)), dict(entries=entry(1, n=-2)), dict(entries=entry(0, first=-1)), dict(entries=entry(2, first=7)),
             dict(num_tris_total=8), dict(entries=entry(0, first=0x7FFFFFFF, n=0x7FFFFFFF)),
             # epsilon
             dict(entries=entry(1, eps=-1e-3)), dict(entries=entry(2, eps=float("nan"))), dict(entries=entry(0, eps=float("inf"))),
             # overlapping and duplicate entries: nodes, rows, a duplicate, a range inside another
             dict(entries=entries + [entries[1]]), dict(entries=[entries[0], entries[0]]),
             dict(entries=entry(1, rng=dict(no=ranges[0][0] + 64))), dict(entries=entry(1, rng=dict(wo=ranges[2][2] + 16))),
             dict(entries=[entries[2], entries[0], (ranges[0][:2] + (woop_bytes - 16, 16), 0, 5, 0.0)], pool_woop_bytes=woop_bytes)]
    for change in cases:
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.bvh_refit_batch(**dict(good, **change), blocking=blocking)
            assert e.value.code == -1 and "ntr_bvh_refit_batch" in str(e.value), (change, str(e.value))
    for change in (dict(entries=entries + [entries[1]]), dict(entries=entry(1, rng=dict(wo=ranges[2][2] + 16)))):
        with pytest.raises(nt.NtrError) as e:
            nt.bvh_refit_batch(**dict(good, **change))
        assert "overlap" in str(e.value), str(e.value)
    assert not buf.any()

    # the raw entry point: a null entry array, 2^20 + 1 entries (the count is refused before the array is read); a failed call zeroes *result
    L = nt.lib()
    arr = (nt.RefitBatchEntry * 3)(*[nt.RefitBatchEntry(*x) for x in entries])
    res = nt.BvhRefitBatchResult()
    tail = (fake, nodes_bytes, fake, woop_bytes, fake, 9, fake, 20, fake, None)
    for count, a in ((3, None), (rb.MAX_ENTRIES + 1, arr), (0, arr), (-1, arr)):
        C.memset(C.byref(res), 0xFF, C.sizeof(res))
        assert L.ntr_bvh_refit_batch(count, C.cast(a, C.c_void_p), *tail, C.byref(res), None) == -1
        assert bytes(res) == bytes(C.sizeof(res)) and b"ntr_bvh_refit_batch" in L.ntr_last_error()
        assert L.ntr_bvh_refit_batch(count, C.cast(a, C.c_void_p), *tail, None, None) == -1

    if not _has_device():   # valid arguments and no device: no CPU fallback, after the argument checks
        for blocking in (True, False):
            with pytest.raises(nt.NtrError) as e:
                nt.bvh_refit_batch(**good, blocking=blocking)
            assert e.value.code in (-2, -3)
        assert not buf.any()


def test_the_most_entries_pass_the_checks_and_an_overlap_among_them_is_found_by_the_sort():
    """2^20 one-triangle BLASes: the checks and the overlap search take a moment, not the minutes of a quadratic scan."""
    m = rb.MAX_ENTRIES
    arr = (nt.RefitBatchEntry * m)()
    v64 = np.frombuffer(arr, np.int64).reshape(m, 6)
    k = np.arange(m, dtype=np.int64)
    v64[:, 0], v64[:, 1], v64[:, 2], v64[:, 3] = 64 * k, 64, 80 * k, 80
    v32 = np.frombuffer(arr, np.int32).reshape(m, 12)
    v32[:, 8], v32[:, 9] = k, 1
    order = np.random.default_rng(5).permutation(m)
    v64[:] = v64[order]
    dup = int(np.flatnonzero(order == 777)[0])
    other = (dup + 12345) % m
    v64[other, 0] = 64 * 777                       # two entries name the nodes of BLAS 777
    buf = np.zeros(64, np.uint8)
    fake = buf.ctypes.data
    L = nt.lib()
    rc = L.ntr_bvh_refit_batch(m, C.cast(arr, C.c_void_p), fake, 64 * m, fake, 80 * m, fake, m, fake, 3, fake, None, None, None)
    msg = L.ntr_last_error().decode()
    assert rc == -1 and "overlap" in msg and str(min(dup, other)) in msg and str(max(dup, other)) in msg, msg


def test_spec_with_unmoved_vertices_and_epsilon_0_returns_a_ploc_pool_unchanged():
    sizes = (1, 2, 3, 40, 1, 300, 1, 1200)
    tri, pos, meshes = pb.concat([scenes.random_soup(n, seed=31 + 7 * k + n, walls=False)[:2] for k, n in enumerate(sizes)])
    b = pb.build(meshes, tri, pos)
    entries = [(r, m[0], m[1], 0.0) for r, m in zip(b["ranges"], meshes)]
    out = rb.refit(entries, b["nodes"], b["woop"], b["tri_index"], tri, pos)
    assert np.array_equal(out["nodes"], b["nodes"])
    got, exp = out["woop"].view(np.uint32), b["woop"].view(np.uint32)
    assert ((got == exp) | (np.isnan(got.view(F)) & np.isnan(exp.view(F)))).all()
    assert out["stats"] == {k: sum(s[k] for s in b["stats"]) if k != "numRows" else b["woop"].size // 16
                            for k in ("numNodes", "numLeaves", "numRows")}
    for box, m in zip(out["boxes"], meshes):
        p = pos[tri[m[0]:m[0] + m[1]]].reshape(-1, 3)
        assert np.array_equal(box, np.concatenate([p.min(axis=0), p.max(axis=0)]))
    # a subset in another order touches nothing else, and moved vertices change exactly the listed ranges
    import np_bvh_refit as rf
    moved = rf.moved(pos, 0.3)
    sub = [entries[5], entries[0], entries[3]]
    part = rb.refit(sub, b["nodes"], b["woop"], b["tri_index"], tri, moved)
    mask_n, mask_w = np.zeros(b["nodes"].size, bool), np.zeros(b["woop"].size, bool)
    for (no, nb, wo, wb), _, _, _ in sub:
        mask_n[no:no + nb] = True
        mask_w[wo:wo + wb] = True
    assert np.array_equal(part["nodes"][~mask_n], b["nodes"][~mask_n]) and np.array_equal(part["woop"][~mask_w], b["woop"][~mask_w])
    assert not np.array_equal(part["nodes"][mask_n], b["nodes"][mask_n])
