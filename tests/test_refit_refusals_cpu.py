"""What the five in-place refit entry points refuse, with which words and in which order, without a device: every call below starts from a
good call on fake, never dereferenced pointers and must return the code and the full ntr_last_error text that
tests/golden/refit_refusals.json records (written by tests/golden/make_refit_refusals.py from the library as it was before the refits'
host protocol and the two binary top-level refits' argument checks were stated once).  Single faults: one for every host
check an entry point makes, in source order, with every way a range or an entry can be bad and the batch units' overlaps.  Double faults:
two neighbouring checks fail at once, and the text says which comes first.  Every call is made in the blocking form (a result struct
filled with 0xFF, which must come back all zero) and in the asynchronous form (result = NULL)."""
import copy
import ctypes as C
import json
import os
import re

import ntrace_amd as nt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refit_refusals.json")
FAKE = 0x10000
BIG = 0xFFFFFF00            # the longest pool buffer
MAX_NODES_BYTES = 0x76543200   # the longest Compact or wide node buffer

_RANGE = ("nodesOffset", "nodesBytes", "triWoopOffset", "triWoopBytes")
_WIDE_RANGE = ("nodesOffset", "nodesBytes", "numNodes", "stackBound")
_WIDE_ENTRY = ("wideNodesOffset", "wideNodesBytes", "triWoopOffset", "triWoopBytes", "firstTri", "numTris", "epsilon")


def _ranges(v):
    return (nt.BlasRange * max(len(v), 1))(*[nt.BlasRange(*[int(r[k]) for k in _RANGE]) for r in v])


def _wide_ranges(v):
    return (nt.WideBlasRange * max(len(v), 1))(*[nt.WideBlasRange(*[int(r[k]) for k in _WIDE_RANGE]) for r in v])


def _entries(v):
    return (nt.RefitBatchEntry * max(len(v), 1))(*[nt.RefitBatchEntry([int(e[k]) for k in _RANGE], e["firstTri"], e["numTris"], e["epsilon"])
                                                    for e in v])


def _wide_entries(v):
    return (nt.WideRefitEntry * max(len(v), 1))(*[nt.WideRefitEntry(*[e[k] for k in _WIDE_ENTRY]) for e in v])


_ARRAYS = dict(blasRanges=_ranges, wideRanges=_wide_ranges, rb_entries=_entries, wr_entries=_wide_entries)

# ---- the good calls: the C arguments in their order (an array argument is a list of dicts, or None for a null pointer) ----------------
_R2 = [dict(nodesOffset=0, nodesBytes=640, triWoopOffset=0, triWoopBytes=1600), dict(nodesOffset=640, nodesBytes=64, triWoopOffset=1600, triWoopBytes=80)]
_TLAS = dict(numInstances=5, d_instances=FAKE, numBlas=2, blasRanges=_R2, d_poolNodes=FAKE, poolNodesBytes=704, d_tlasNodes=FAKE,
             tlasNodesBytes=256, rootLink=0, d_records=FAKE, recordsCapacity=320, d_sceneBox=FAKE, result=None, stream=0)
_MOTION = dict(numInstances=5, d_instances0=FAKE, d_instances1=FAKE, numBlas=2, blasRanges=_R2, d_poolNodes=FAKE, poolNodesBytes=704,
               d_tlasNodes=FAKE, tlasNodesBytes=256, rootLink=0, d_records=FAKE, recordsCapacity=320, d_motionKeys=FAKE,
               motionKeysCapacity=640, d_sceneBox=FAKE, result=None, stream=0)
_WIDE = dict(numInstances=5, d_instances=FAKE, numBlas=2, blasRanges=_R2,
             wideRanges=[dict(nodesOffset=0, nodesBytes=384, numNodes=3, stackBound=4), dict(nodesOffset=384, nodesBytes=128, numNodes=1, stackBound=1)],
             d_widePoolNodes=FAKE, widePoolNodesBytes=512, d_wideTlasNodes=FAKE, wideTlasNodesBytes=256, rootLink=0, d_wideRecords=FAKE,
             recordsCapacity=320, d_sceneBox=FAKE, result=None, stream=0)
_BATCH = dict(numEntries=2,
              rb_entries=[dict(nodesOffset=0, nodesBytes=640, triWoopOffset=0, triWoopBytes=1600, firstTri=0, numTris=30, epsilon=0.0),
                          dict(nodesOffset=640, nodesBytes=64, triWoopOffset=1600, triWoopBytes=80, firstTri=30, numTris=1, epsilon=0.5)],
              d_poolNodes=FAKE, poolNodesBytes=704, d_poolTriWoop=FAKE, poolTriWoopBytes=1680, d_poolTriIndex=FAKE, numTrisTotal=31,
              d_triVtxIndex=FAKE, numVerts=40, d_vtxPos=FAKE, d_blasBoxes=FAKE, result=None, stream=0)
_WIDE_BATCH = dict(numEntries=2,
                   wr_entries=[dict(wideNodesOffset=0, wideNodesBytes=384, triWoopOffset=0, triWoopBytes=1600, firstTri=0, numTris=30, epsilon=0.0),
                               dict(wideNodesOffset=384, wideNodesBytes=128, triWoopOffset=1600, triWoopBytes=80, firstTri=30, numTris=1, epsilon=0.5)],
                   d_widePoolNodes=FAKE, widePoolNodesBytes=512, d_poolTriWoop=FAKE, poolTriWoopBytes=1680, d_poolTriIndex=FAKE, numTrisTotal=31,
                   d_triVtxIndex=FAKE, numVerts=40, d_vtxPos=FAKE, rewriteRows=1, d_blasBoxes=FAKE, result=None, stream=0)

# ---- the checks of each entry point in source order: one fault for each (the CHAIN), and the further ways a check can fail ---------------
_R0 = "blasRanges[0]."
_BINARY_RANGE = [{_R0 + "nodesOffset": 32}, {_R0 + "nodesBytes": 768}, {_R0 + "triWoopOffset": 8}]
_BINARY_RANGE_TOO = [{_R0 + "nodesBytes": 96}, {_R0 + "nodesBytes": 0}, {_R0 + "nodesOffset": -64}, {_R0 + "nodesOffset": 128},
                     {_R0 + "nodesBytes": MAX_NODES_BYTES + 64, "poolNodesBytes": BIG}, {_R0 + "triWoopBytes": 1608},
                     {_R0 + "triWoopOffset": -16}, {_R0 + "triWoopBytes": 0}, {_R0 + "triWoopOffset": BIG}, {"blasRanges[1].nodesOffset": 704}]
_BINARY_TOO = [dict(numInstances=0), dict(numInstances=-3), dict(numInstances=MAX_NODES_BYTES // 64 + 2, tlasNodesBytes=MAX_NODES_BYTES + 64),
               dict(numBlas=0), dict(blasRanges=None), dict(d_poolNodes=0), dict(d_records=0), dict(d_tlasNodes=0),
               dict(tlasNodesBytes=320), dict(tlasNodesBytes=0), dict(rootLink=-1), dict(d_poolNodes=FAKE + 4), dict(d_tlasNodes=FAKE + 8),
               dict(d_records=FAKE + 12), dict(poolNodesBytes=0), dict(poolNodesBytes=BIG + 64),
               dict(numInstances=1, d_tlasNodes=0, tlasNodesBytes=0, rootLink=0, recordsCapacity=64),
               dict(numInstances=1, d_tlasNodes=0, tlasNodesBytes=64, rootLink=-1, recordsCapacity=64),
               dict(numInstances=1, d_tlasNodes=0, tlasNodesBytes=0, rootLink=-1, recordsCapacity=63)]
_E0, _E1, _E2 = "rb_entries[0].", "rb_entries[1].", "rb_entries[2]."
_W0, _W1, _W2 = "wr_entries[0].", "wr_entries[1].", "wr_entries[2]."
_THREE_LONG = dict(nodesOffset=0, nodesBytes=MAX_NODES_BYTES, triWoopOffset=0, triWoopBytes=64, firstTri=0, numTris=1, epsilon=0.0)
_THREE_LONG_WIDE = dict(wideNodesOffset=0, wideNodesBytes=MAX_NODES_BYTES, triWoopOffset=0, triWoopBytes=64, firstTri=0, numTris=1, epsilon=0.0)

CHECKS = {
    "ntr_tlas_refit": dict(
        result=nt.TlasRefitResult, good=_TLAS,
        chain=[dict(d_instances=0), dict(tlasNodesBytes=192), dict(rootLink=64), dict(recordsCapacity=319), dict(d_instances=FAKE + 8),
               dict(poolNodesBytes=700)] + _BINARY_RANGE,
        too=_BINARY_TOO + _BINARY_RANGE_TOO),
    "ntr_tlas_motion_refit": dict(
        result=nt.TlasMotionRefitResult, good=_MOTION,
        chain=[dict(d_instances1=0), dict(tlasNodesBytes=192), dict(rootLink=64), dict(recordsCapacity=319), dict(motionKeysCapacity=639),
               dict(d_motionKeys=FAKE + 8), dict(poolNodesBytes=700)] + _BINARY_RANGE,
        too=[dict(d_instances0=0), dict(d_motionKeys=0), dict(d_instances0=FAKE + 8), dict(d_instances1=FAKE + 4)] + _BINARY_TOO
        + _BINARY_RANGE_TOO + [dict(numInstances=1, d_tlasNodes=0, tlasNodesBytes=0, rootLink=-1, recordsCapacity=64, motionKeysCapacity=127)],
        # further pairs that straddle the motion refit's own arguments and the shared ones (the chain's neighbours hold d_instances1 == NULL
        # with a bad tlasNodesBytes, and a short motionKeysCapacity with a misaligned d_motionKeys)
        pairs=[dict(motionKeysCapacity=639, d_records=FAKE + 12),
               dict(motionKeysCapacity=639, d_instances1=FAKE + 4), dict(d_motionKeys=0, rootLink=64)]),
    "ntr_tlas_wide_refit": dict(
        result=nt.TlasRefitResult, good=_WIDE,
        chain=[dict(d_instances=0), dict(wideTlasNodesBytes=192), dict(rootLink=64), dict(recordsCapacity=319), dict(d_wideRecords=FAKE + 8),
               dict(widePoolNodesBytes=448), {_R0 + "triWoopOffset": 8}, {"wideRanges[0].nodesOffset": 64}],
        too=[dict(numInstances=0), dict(numInstances=BIG // 64 + 1), dict(numBlas=0), dict(blasRanges=None), dict(wideRanges=None),
             dict(d_widePoolNodes=0), dict(d_wideRecords=0), dict(d_wideTlasNodes=0), dict(wideTlasNodesBytes=0),
             dict(wideTlasNodesBytes=MAX_NODES_BYTES + 128), dict(rootLink=-1), dict(d_instances=FAKE + 8), dict(d_widePoolNodes=FAKE + 4),
             dict(d_wideTlasNodes=FAKE + 12), dict(widePoolNodesBytes=0), dict(widePoolNodesBytes=BIG + 128),
             {_R0 + "triWoopOffset": -16}, {_R0 + "triWoopOffset": BIG}, {"wideRanges[0].nodesOffset": -128}, {"wideRanges[0].nodesBytes": 0},
             {"wideRanges[0].nodesBytes": 192}, {"wideRanges[0].nodesBytes": MAX_NODES_BYTES + 128, "widePoolNodesBytes": BIG},
             {"wideRanges[1].nodesOffset": 512},
             dict(numInstances=1, d_wideTlasNodes=0, wideTlasNodesBytes=128, rootLink=-1, recordsCapacity=64),
             dict(numInstances=1, d_wideTlasNodes=0, wideTlasNodesBytes=0, rootLink=0, recordsCapacity=64),
             dict(numInstances=1, d_wideTlasNodes=0, wideTlasNodesBytes=0, rootLink=-1, recordsCapacity=63)]),
    "ntr_bvh_refit_batch": dict(
        result=nt.BvhRefitBatchResult, good=_BATCH,
        chain=[dict(rb_entries=None), dict(d_vtxPos=0), dict(poolNodesBytes=700), dict(poolTriWoopBytes=1688), dict(numTrisTotal=0),
               dict(numVerts=0), dict(d_poolTriWoop=FAKE + 8), {_E0 + "nodesOffset": 32}, {_E0 + "nodesBytes": 768}, {_E0 + "triWoopOffset": 8},
               {_E0 + "triWoopBytes": 3200}, {_E0 + "numTris": 0}, {_E0 + "epsilon": -1.0}, {_E1 + "nodesOffset": 576}, {_E1 + "triWoopOffset": 1584}],
        too=[dict(numEntries=0), dict(numEntries=(1 << 20) + 1), dict(d_poolNodes=0), dict(d_poolTriWoop=0), dict(d_poolTriIndex=0),
             dict(d_triVtxIndex=0), dict(poolNodesBytes=0), dict(poolTriWoopBytes=0), dict(d_poolNodes=FAKE + 4),
             {_E0 + "nodesBytes": 0}, {_E1 + "nodesOffset": 704}, {_E0 + "triWoopBytes": 0}, {_E1 + "triWoopOffset": 1616},
             {_E0 + "firstTri": -1}, {_E1 + "numTris": 2}, {_E0 + "epsilon": float("nan")}, {_E0 + "epsilon": float("inf")},
             dict(numEntries=3, rb_entries=[_THREE_LONG] * 3, poolNodesBytes=BIG)]),
    "ntr_pool_wide_refit": dict(
        result=nt.WideRefitResult, good=_WIDE_BATCH,
        chain=[dict(wr_entries=None), dict(d_vtxPos=0), dict(widePoolNodesBytes=448), dict(poolTriWoopBytes=1688), dict(numTrisTotal=0),
               dict(numVerts=0), dict(rewriteRows=2), dict(d_poolTriWoop=FAKE + 8), {_W0 + "wideNodesOffset": 64}, {_W0 + "triWoopOffset": 8},
               {_W0 + "numTris": 0}, {_W0 + "epsilon": -1.0}, {_W1 + "wideNodesOffset": 256}, {_W1 + "triWoopOffset": 1584}],
        too=[dict(numEntries=0), dict(numEntries=(1 << 20) + 1), dict(d_widePoolNodes=0), dict(d_poolTriWoop=0), dict(d_poolTriIndex=0),
             dict(d_triVtxIndex=0), dict(widePoolNodesBytes=0), dict(poolTriWoopBytes=0), dict(rewriteRows=-1), dict(d_widePoolNodes=FAKE + 4),
             {_W0 + "wideNodesOffset": -128}, {_W0 + "wideNodesBytes": 0}, {_W0 + "wideNodesBytes": 192}, {_W1 + "wideNodesOffset": 512},
             {_W0 + "wideNodesBytes": MAX_NODES_BYTES + 128, "widePoolNodesBytes": BIG}, {_W0 + "triWoopOffset": -16}, {_W0 + "triWoopBytes": 0},
             {_W0 + "triWoopBytes": 1608}, {_W0 + "triWoopBytes": 3200}, {_W0 + "firstTri": -1}, {_W1 + "numTris": 2},
             {_W0 + "epsilon": float("nan")},
             dict(numEntries=3, wr_entries=[_THREE_LONG_WIDE] * 3, widePoolNodesBytes=BIG)]),
}
# (every case is refused by a host check: a call that passed them all would hand the fake pointers to a device where there is one)


def _label(change):
    def text(v):
        if isinstance(v, list):
            return "%d x (%s)" % (len(v), " ".join("%s=%s" % (k, text(x)) for k, x in v[0].items()))
        if v is None or isinstance(v, float):
            return str(v)
        return "0x%x" % v if v > 9 else str(v)
    return " ".join("%s=%s" % (k, text(v)) for k, v in change.items())


def cases(name):
    """-> [(label, the change to the good call)]: the single faults, then the double faults."""
    c = CHECKS[name]
    doubles = [dict(a, **b) for a, b in zip(c["chain"], c["chain"][1:])] + c.get("pairs", [])
    return [(_label(ch), ch) for ch in c["chain"] + c["too"] + doubles]


def call(name, change, blocking):
    """-> [code, the ntr_last_error text, the result struct came back all zero (None in the asynchronous form)]"""
    c = CHECKS[name]
    kw = copy.deepcopy(c["good"])
    for key, v in change.items():
        m = re.match(r"(\w+)\[(\d+)\]\.(\w+)$", key)
        if m:
            kw[m.group(1)][int(m.group(2))][m.group(3)] = v
        else:
            kw[key] = copy.deepcopy(v)
    res = c["result"]()
    C.memset(C.byref(res), 0xFF, C.sizeof(res))
    keep, args = [], []
    for k, v in kw.items():
        if k in _ARRAYS:
            keep.append(None if v is None else _ARRAYS[k](v))
            args.append(None if v is None else C.cast(keep[-1], C.c_void_p))
        elif k == "result":
            args.append(C.byref(res) if blocking else None)
        else:
            args.append((v or None) if k.startswith("d_") or k == "stream" else v)
    L = nt.lib()
    code = getattr(L, name)(*args)
    return [code, (L.ntr_last_error() or b"").decode() if code else "", bytes(res) == bytes(C.sizeof(res)) if blocking else None]


def record(name):
    """Everything the golden file holds for one entry point: label -> [the blocking form's call, the asynchronous form's]."""
    return {label: [call(name, change, True), call(name, change, False)] for label, change in cases(name)}


def refused_on_the_host(value):
    return all(v[0] == -1 and v[1] for v in value) and value[0][2] is True and value[0][:2] == value[1][:2]


def test_every_refusal_and_the_order_of_the_checks_are_the_recorded_ones():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(CHECKS) == 5 and set(golden) == set(CHECKS)
    for name, c in CHECKS.items():
        got = record(name)
        assert len(got) == 2 * len(c["chain"]) - 1 + len(c["too"]) + len(c.get("pairs", [])), name   # no two cases share a label
        for label, value in got.items():
            assert label in golden[name], (name, label)
            assert value == golden[name][label], (name, label, value, golden[name][label])
            assert refused_on_the_host(value) and value[0][1].startswith(name + ": "), (name, label, value)
        assert set(golden[name]) == set(got), (name, sorted(set(golden[name]) - set(got)))


def test_the_chain_is_in_source_order():
    """Each single fault of the chain is refused with a text of its own, and a pair of neighbours with the first one's."""
    for name, c in CHECKS.items():
        texts = [call(name, ch, False)[1] for ch in c["chain"]]
        assert len(set(texts)) == len(texts), (name, texts)
        for a, b, first in zip(c["chain"], c["chain"][1:], texts):
            assert call(name, dict(a, **b), False)[1] == first, (name, a, b)
