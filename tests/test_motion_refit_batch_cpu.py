"""ntr_bvh_motion_refit_batch without a device: the numpy rule (tests/np_motion_refit_batch.py) against the pool-wide rule the deforming
trace's tests already use (np_instanced_deform.pool_motion_refit), subsets, per-entry epsilon, and the C-ABI surface -- every
NTR_ERR_INVALID case is refused with its message before any device work (fake, never dereferenced pointers), ntr_bvh_refit_batch's
cases first, in its order and its words (tests/golden/refit_refusals.json)."""
import copy
import ctypes as C
import json

import numpy as np
import pytest

import ntrace_amd as nt

import instanced_deform_cases as dc
import instanced_scenes as isc
import np_bvh_refit as rf
import np_motion_refit_batch as mb
import test_refit_refusals_cpu as rr

F = np.float32
FILL = 0xCD


def _shared(s):
    """A DeformScene's meshes as one shared index array and two shared vertex arrays (np_ploc_batch.concat's layout), and the entry of
    every deforming BLAS.  A static BLAS's vertices are the same under both keys; it has no entry."""
    tris, p0, p1, entries = [], [], [], []
    t_off = v_off = 0
    for b, name in enumerate(s.names):
        tri, pos, _ = isc.blas(name)
        mesh = s.meshes[b]
        tris.append(np.asarray(tri, np.int32) + v_off)
        p0.append(pos if mesh is None else mesh[1])
        p1.append(pos if mesh is None else mesh[2])
        if mesh is not None:
            entries.append((tuple(int(x) for x in s.ranges[b]), t_off, tri.shape[0], 0.0))
        t_off += tri.shape[0]
        v_off += pos.shape[0]
    return np.concatenate(tris).astype(np.int32), np.concatenate(p0).astype(F), np.concatenate(p1).astype(F), entries


def _run(pool, entries, tri, pos0, pos1):
    n, w = pool["nodes"].size, pool["woop"].size
    return mb.motion_refit(entries, pool["nodes"], np.full(n, FILL, np.uint8), pool["woop"], np.full(w, FILL, np.uint8), np.full(w, FILL, np.uint8),
                           pool["tri_index"], tri, pos0, pos1)


@pytest.mark.parametrize("which", ["three", "big"])
def test_the_rule_equals_the_pool_rule_on_the_deforming_blases(which):
    s = dc.named("three") if which == "three" else dc.big()
    tri, pos0, pos1, entries = _shared(s)
    assert len(entries) == int(s.pool["deforming"].sum()) > 0
    got = _run(isc.pool_of(s.names), entries, tri, pos0, pos1)
    for mine, theirs in (("nodes0", "nodes"), ("nodes1", "nodes1"), ("woop", "woop"), ("vrows0", "vrows0"), ("vrows1", "vrows1")):
        assert got[mine].tobytes() == s.pool[theirs].tobytes(), (which, mine)       # the listed ranges, and the fill byte elsewhere
    for k, (r, _, _, _) in enumerate(entries):
        b = s.ranges.index(r)
        m, tidx = s.blas_slices(b)
        root0 = rf.refit(m["nodes0"], m["woop"], tidx, s.meshes[b][0], s.meshes[b][1], 0.0)
        root1 = rf.refit(m["nodes0"], m["woop"], tidx, s.meshes[b][0], s.meshes[b][2], 0.0)
        lo = np.minimum(root0["scene_box"][:3], root1["scene_box"][:3])
        hi = np.maximum(root0["scene_box"][3:], root1["scene_box"][3:])
        assert np.array_equal(got["boxes"][k], np.concatenate([lo, hi]))
    assert got["stats"] == {k: sum(m["stats"][k] for m in got["per_entry"]) for k in ("numNodes", "numLeaves", "numRows")}
    assert got["stats"]["numRows"] == sum(e[0][3] // 16 for e in entries)               # PLOC trees reach every row they own


def _all_deforming():
    names = ["soup64", "one", "cornell", "soup100", "one"]
    pool = isc.pool_of(names)
    parts = [isc.blas(n)[:2] for n in names]
    tris, poss, entries, t_off, v_off = [], [], [], 0, 0
    for (tri, pos), r in zip(parts, pool["ranges"]):
        tris.append(np.asarray(tri, np.int32) + v_off)
        poss.append(np.asarray(pos, F))
        entries.append((tuple(int(x) for x in r), t_off, tri.shape[0], 0.0))
        t_off += tri.shape[0]
        v_off += pos.shape[0]
    pos0 = np.concatenate(poss).astype(F)
    return pool, np.concatenate(tris).astype(np.int32), pos0, rf.moved(pos0, 0.3), entries


def test_a_subset_in_scrambled_order_leaves_the_other_ranges_at_the_fill_byte():
    pool, tri, pos0, pos1, entries = _all_deforming()
    sel = [entries[k] for k in (3, 0, 2)]
    got, full = _run(pool, sel, tri, pos0, pos1), _run(pool, entries, tri, pos0, pos1)
    assert np.array_equal(got["boxes"], full["boxes"][[3, 0, 2]])                   # boxes in entry order
    for k, ((no, nb, wo, wb), _, _, _) in enumerate(entries):
        for name in mb.BUFFERS:
            o, b = (no, nb) if name.startswith("nodes") else (wo, wb)
            if k in (3, 0, 2):
                assert np.array_equal(got[name][o:o + b], full[name][o:o + b]), (k, name)
            elif name in ("nodes0", "woop"):
                src = pool["nodes"] if name == "nodes0" else pool["woop"]
                assert np.array_equal(got[name][o:o + b], np.ascontiguousarray(src).view(np.uint8).reshape(-1)[o:o + b]), (k, name)
            else:
                assert (got[name][o:o + b] == FILL).all(), (k, name)
    # the terminator is in the w word, and a listed BLAS's vertex rows hold no fill byte
    no, nb, wo, wb = entries[0][0]
    rows = got["vrows0"][wo:wo + wb].view(np.uint32).reshape(-1, 4)
    assert ((rows[:, 3] == 0x80000000) == (rows[:, 3] != 0)).all() and (rows[rows[:, 3] != 0][:, :3] == 0).all() and (rows[:, 3] != 0).any()


def test_per_entry_epsilon():
    pool, tri, pos0, pos1, entries = _all_deforming()
    eps = [(e[0], e[1], e[2], 0.001 if k % 2 else 0.0) for k, e in enumerate(entries)]
    got, zero = _run(pool, eps, tri, pos0, pos1), _run(pool, entries, tri, pos0, pos1)
    for k, ((no, nb, wo, wb), _, _, _) in enumerate(entries):
        for key in ("nodes0", "nodes1"):
            x, y = zero[key][no:no + nb].view(F).reshape(-1, 16), got[key][no:no + nb].view(F).reshape(-1, 16)
            if k % 2 == 0:
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
                continue
            links = zero[key][no:no + nb].view(np.int32).reshape(-1, 16)[:, 12:14]
            first = zero["woop"][wo:wo + wb].view(np.uint32).reshape(-1, 4)[:, 0]
            for c in (0, 1):
                lo, hi, m = rf.BOX_WORDS[c][rf.LO], rf.BOX_WORDS[c][rf.HI], links[:, c] < 0
                has = first[~links[m, c]] != rf.TERM                                 # a leaf without rows keeps its box
                assert np.array_equal(y[m][has][:, lo], (x[m][has][:, lo] - F(0.001)).astype(F)), (k, key)
                assert np.array_equal(y[m][has][:, hi], (x[m][has][:, hi] + F(0.001)).astype(F)), (k, key)
        for key in ("woop", "vrows0", "vrows1"):
            assert np.array_equal(got[key][wo:wo + wb], zero[key][wo:wo + wb])       # epsilon widens boxes only


# ---- the C-ABI surface without a device -----------------------------------------------------------------------------------------------
NAME = "ntr_bvh_motion_refit_batch"
A = 0x1000000               # fake buffers far enough apart that no two meet
_GOOD = dict(numEntries=2, rb_entries=rr._BATCH["rb_entries"], d_poolNodes0=1 * A, poolNodesBytes=704, d_poolNodes1=2 * A, d_poolTriWoop=3 * A,
             poolTriWoopBytes=1680, d_poolTriIndex=4 * A, d_poolVertRows0=5 * A, d_poolVertRows1=6 * A, numTrisTotal=31, d_triVtxIndex=7 * A,
             numVerts=40, d_vtxPos0=8 * A, d_vtxPos1=9 * A, d_blasBoxes=10 * A, result=None, stream=0)
_RENAMED = dict(d_poolNodes="d_poolNodes0", d_vtxPos="d_vtxPos0")


def _call(change, blocking):
    kw = copy.deepcopy(_GOOD)
    for key, v in change.items():
        m = rr.re.match(r"(\w+)\[(\d+)\]\.(\w+)$", key)
        if m:
            kw[m.group(1)][int(m.group(2))][m.group(3)] = v
        else:
            kw[_RENAMED.get(key, key)] = copy.deepcopy(v)
    res = nt.BvhRefitBatchResult()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    keep, args = [], []
    for k, v in kw.items():
        if k == "rb_entries":
            keep.append(None if v is None else rr._entries(v))
            args.append(None if v is None else C.cast(keep[-1], C.c_void_p))
        elif k == "result":
            args.append(C.byref(res) if blocking else None)
        else:
            args.append((v or None) if k.startswith("d_") or k == "stream" else v)
    L = nt.lib()
    code = getattr(L, NAME)(*args)
    return code, (L.ntr_last_error() or b"").decode() if code else "", bytes(res) == bytes(C.sizeof(res)) if blocking else None


def _refused(change, text):
    """Refused on the host in both forms with exactly `text`; the blocking form's result comes back zero."""
    for blocking in (True, False):
        code, msg, zero = _call(change, blocking)
        assert code == -1 and msg == text, (change, blocking, code, msg, text)
        assert zero is (True if blocking else None), (change, blocking)


def test_the_refit_batch_cases_are_refused_in_its_order_and_words():
    with open(rr.GOLDEN) as f:
        golden = json.load(f)["ntr_bvh_refit_batch"]
    cases = rr.cases("ntr_bvh_refit_batch")
    assert len(cases) == len(golden) > 40
    for label, change in cases:
        code, text, _ = golden[label][0]
        assert code == -1 and text.startswith("ntr_bvh_refit_batch: ")
        ch = {k: (v % A + A if k in ("d_poolNodes", "d_poolTriWoop") and v else v) for k, v in change.items()}   # misaligned, but apart
        _refused(ch, NAME + text[len("ntr_bvh_refit_batch"):])


def test_the_second_keys_buffers_are_checked_after_them():
    for arg in ("d_poolNodes1", "d_poolVertRows0", "d_poolVertRows1", "d_vtxPos1"):
        _refused({arg: 0}, "%s: null %s" % (NAME, arg))
    aligned = NAME + ": d_poolNodes0, d_poolNodes1, d_poolTriWoop, d_poolVertRows0 and d_poolVertRows1 must be 16-byte aligned"
    for arg in ("d_poolNodes1", "d_poolVertRows0", "d_poolVertRows1"):
        _refused({arg: _GOOD[arg] + 8}, aligned)
    # an earlier check wins: an entry fault before a null key-1 buffer, a null one before a misaligned one, that before an overlap
    _refused({"rb_entries[1].triWoopOffset": 1584, "d_poolNodes1": 0}, NAME + ": entries 0 and 1 overlap in the pool's rows: a BLAS is refitted "
             "once per call")
    _refused(dict(d_poolVertRows1=0, d_poolNodes1=_GOOD["d_poolNodes1"] + 8), NAME + ": null d_poolVertRows1")
    _refused(dict(d_poolVertRows0=_GOOD["d_poolVertRows0"] + 8, d_vtxPos1=_GOOD["d_vtxPos0"]), aligned)


def test_a_fresh_buffer_that_meets_another_buffer_of_the_call_is_refused_by_name():
    g = _GOOD
    meets = [(dict(d_poolNodes1=g["d_poolNodes0"]), "d_poolNodes1", "d_poolNodes0"),
             (dict(d_poolNodes1=g["d_poolNodes0"] + 704 - 64), "d_poolNodes1", "d_poolNodes0"),          # the last slot of the pool's extent
             (dict(d_poolNodes1=g["d_poolNodes0"] - 704 + 64), "d_poolNodes1", "d_poolNodes0"),
             (dict(d_poolNodes1=g["d_poolTriWoop"] + 1680 - 16), "d_poolNodes1", "d_poolTriWoop"),
             (dict(d_poolNodes1=g["d_poolTriIndex"] + 416), "d_poolNodes1", "d_poolTriIndex"),           # 420 bytes of entries
             (dict(d_poolNodes1=g["d_triVtxIndex"] + 368), "d_poolNodes1", "d_triVtxIndex"),             # 31 triangles: 372 bytes
             (dict(d_poolNodes1=g["d_vtxPos0"] + 464), "d_poolNodes1", "d_vtxPos0"),                     # 40 vertices: 480 bytes
             (dict(d_poolNodes1=g["d_blasBoxes"] + 32), "d_poolNodes1", "d_blasBoxes"),                  # two entries: 48 bytes
             (dict(d_poolVertRows0=g["d_poolTriWoop"]), "d_poolVertRows0", "d_poolTriWoop"),
             (dict(d_poolVertRows0=g["d_poolNodes0"] + 688), "d_poolVertRows0", "d_poolNodes0"),
             (dict(d_poolVertRows1=g["d_poolVertRows0"] + 1664), "d_poolVertRows0", "d_poolVertRows1"),
             (dict(d_poolVertRows1=g["d_poolNodes1"] + 16), "d_poolNodes1", "d_poolVertRows1"),
             (dict(d_vtxPos1=g["d_vtxPos0"]), "d_vtxPos1", "d_vtxPos0"),
             (dict(d_vtxPos1=g["d_vtxPos0"] + 476), "d_vtxPos1", "d_vtxPos0"),
             (dict(d_vtxPos1=g["d_poolVertRows1"] + 1676), "d_poolVertRows1", "d_vtxPos1"),
             (dict(d_vtxPos1=g["d_poolTriWoop"] - 476), "d_vtxPos1", "d_poolTriWoop")]
    for change, a, b in meets:
        _refused(change, "%s: %s overlaps %s" % (NAME, a, b))


def test_symbols_scratch_and_the_python_surface():
    L = nt.lib()
    from ntrace_amd import _capi
    names = [s[0] for s in _capi.SYMBOLS]
    for name in (NAME, NAME + "_scratch_bytes"):
        assert hasattr(L, name) and name in names
    assert callable(nt.bvh_motion_refit_batch) and callable(nt.bvh_motion_refit_batch_scratch_bytes)
    assert "bvh_motion_refit_batch" in nt.__all__ and "bvh_motion_refit_batch_scratch_bytes" in nt.__all__
    assert L.ntr_bvh_motion_refit_batch_scratch_bytes(None) == -1 and b"ntr_bvh_motion_refit_batch_scratch_bytes" in L.ntr_last_error()
    cnt = C.c_int(-1)
    if L.ntr_device_count(C.byref(cnt)) == 0 and cnt.value > 0:
        nt.lbvh_release_workspace()         # another test of this process may have made a call
    assert nt.bvh_motion_refit_batch_scratch_bytes() == 0
    # the Python wrapper raises the same refusals, and carries the zeroed result
    e = rr._entries(_GOOD["rb_entries"])
    with pytest.raises(nt.NtrError) as err:
        nt.bvh_motion_refit_batch(e, A, 704, 0, 3 * A, 1680, 4 * A, 5 * A, 6 * A, 31, 7 * A, 40, 8 * A, 9 * A)
    assert err.value.code == -1 and "null d_poolNodes1" in str(err.value) and err.value.result.numEntries == 0
