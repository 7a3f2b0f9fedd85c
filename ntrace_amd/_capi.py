"""ctypes binding of include/ntrace_amd.h (libntrace_amd.so)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

RAY_DTYPE = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("tmin", "<f4"),
                      ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("tmax", "<f4")])
RESULT_DTYPE = np.dtype([("id", "<i4"), ("t", "<f4"), ("padA", "<i4"), ("padB", "<i4")])


class NtrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ntrace_amd error %d: %s" % (code, msg))
        self.code = code


class SchedHintState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("numBlocks", "device", "uses", "valid", "predicted")]


class KernelConfig(C.Structure):
    _fields_ = [("bvhLayout", C.c_int32), ("blockWidth", C.c_int32), ("blockHeight", C.c_int32),
                ("usePersistentThreads", C.c_int32)]


class TraceStats(C.Structure):
    _fields_ = [("numRays", C.c_int64), ("numInnerVisits", C.c_int64), ("numTriTests", C.c_int64),
                ("numLeafVisits", C.c_int64), ("numHits", C.c_int64)]

    def algorithmic_bytes(self):
        """DESIGN.md / SURVEY.md section 8(d): 32 B ray + 16 B result + 64 B per inner node visited +
        48 B per triangle tested + 16 B per leaf terminator + 4 B index remap per hit."""
        return (48 * self.numRays + 64 * self.numInnerVisits + 48 * self.numTriTests
                + 16 * self.numLeafVisits + 4 * self.numHits)

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class InstanceVisibility(C.Structure):
    """NtrInstanceVisibility: device pointers of the instance masks (num_instances uint32 words, 0: every instance 0xFFFFFFFF) and of
    the per-ray masks (num_rays words, 0: every ray has ray_mask)."""
    _fields_ = [("d_instanceMasks", C.c_void_p), ("d_rayMasks", C.c_void_p), ("rayMask", C.c_uint32), ("pad", C.c_uint32)]

    def __init__(self, d_instance_masks=0, d_ray_masks=0, ray_mask=0xFFFFFFFF):
        super().__init__(int(d_instance_masks) or None, int(d_ray_masks) or None, int(ray_mask) & 0xFFFFFFFF, 0)


class InstancedTraceStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("numRays", "numTopInnerVisits", "numInstanceEntries", "numInstancesMasked", "numInnerVisits",
                                         "numTriTests", "numLeafVisits", "numHits")]

    def algorithmic_bytes(self, instance_masks=False, ray_masks=False):
        """include/ntrace_amd.h, DESIGN.md 6q: 52 B per ray (the ray, the record, the instance id), 64 B per top-level node, instance
        record and bottom-level node fetched, 32 B per entry for the world ray reloaded on leaving, 48 B per triangle tested, 16 B per
        terminator, 4 B index remap per hit; with instance masks 4 B per entering step that asked one, with per-ray masks 4 B per ray."""
        n = (52 * self.numRays + 64 * (self.numTopInnerVisits + self.numInstanceEntries + self.numInnerVisits) + 32 * self.numInstanceEntries
             + 48 * self.numTriTests + 16 * self.numLeafVisits + 4 * self.numHits)
        if instance_masks:
            n += 4 * (self.numInstanceEntries + self.numInstancesMasked)
        if ray_masks:
            n += 4 * self.numRays
        return n

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class InstancedFastStats(C.Structure):
    """NtrInstancedFastStats (the rule is tests/np_instanced_fast.py): iterations of a wave with a live lane, those that took
    the FAST form of the step, rays that start live and nice, entering steps that leave the lane nice.  Wave w is rays [64 w, 64 w + 64)."""
    _fields_ = [(n, C.c_uint64) for n in ("waveSteps", "fastWaveSteps", "niceStarts", "niceEntries")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class LbvhResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numLevels", C.c_int32), ("pad", C.c_int32),
                ("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("seconds", C.c_float), ("mortonMs", C.c_float), ("sortMs", C.c_float), ("woopMs", C.c_float),
                ("emitMs", C.c_float), ("refitMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class HlbvhResult(C.Structure):
    _fields_ = [("lbvh", LbvhResult), ("numClusters", C.c_int32), ("topNodes", C.c_int32), ("topLevels", C.c_int32),
                ("pad", C.c_int32), ("clusterMs", C.c_float), ("topMs", C.c_float), ("bottomMs", C.c_float), ("pad2", C.c_float)]

    def as_dict(self):
        d = self.lbvh.as_dict()
        d.update({k: getattr(self, k) for k, _ in self._fields_ if k not in ("lbvh", "pad", "pad2")})
        return d


class _HostBvhInfo(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodesBytes", C.c_int64), ("triWoop", C.c_void_p),
                ("triWoopBytes", C.c_int64), ("triIndex", C.c_void_p), ("triIndexBytes", C.c_int64),
                ("layout", C.c_int32), ("numInnerNodes", C.c_int32), ("numLeafNodes", C.c_int32),
                ("maxDepth", C.c_int32), ("buildSeconds", C.c_float)]


class _HostKdtreeInfo(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodesBytes", C.c_int64), ("triWoop", C.c_void_p),
                ("triWoopBytes", C.c_int64), ("triIndex", C.c_void_p), ("triIndexBytes", C.c_int64),
                ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3), ("delta", C.c_float),
                ("numInnerNodes", C.c_int32), ("numLeafNodes", C.c_int32), ("numEmptyLeaves", C.c_int32), ("numTriRefs", C.c_int32),
                ("maxDepth", C.c_int32), ("percentDuplicates", C.c_float), ("buildSeconds", C.c_float)]


class KdtreeDeviceParams(C.Structure):
    _fields_ = [("triLimit", C.c_int32), ("triMaxLimit", C.c_int32), ("failureCount", C.c_int32), ("pad", C.c_int32),
                ("depthK1", C.c_float), ("depthK2", C.c_float), ("ci", C.c_float), ("ct", C.c_float), ("failRq", C.c_float)]


class PersistentBvhParams(C.Structure):
    _fields_ = [("triLimit", C.c_int32), ("triMaxLimit", C.c_int32), ("maxDepth", C.c_int32), ("pad", C.c_int32),
                ("ci", C.c_float), ("ct", C.c_float), ("epsilon", C.c_float), ("pad2", C.c_float)]


class PersistentBvhResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numLevels", C.c_int32), ("maxDepth", C.c_int32),
                ("medianFallbacks", C.c_int32), ("costLeaves", C.c_int32), ("depthLeaves", C.c_int32), ("pad", C.c_int32),
                ("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("seconds", C.c_float), ("prepMs", C.c_float), ("levelsMs", C.c_float), ("emitMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class SahDeviceResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numLevels", C.c_int32), ("maxDepth", C.c_int32),
                ("numDropped", C.c_int32), ("pad", C.c_int32 * 3),
                ("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("seconds", C.c_float), ("prepMs", C.c_float), ("sortMs", C.c_float), ("levelsMs", C.c_float), ("emitMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class PlocResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numRounds", C.c_int32), ("height", C.c_int32),
                ("tailClusters", C.c_int32), ("pad", C.c_int32 * 3),
                ("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("seconds", C.c_float), ("mortonMs", C.c_float), ("sortMs", C.c_float), ("roundsMs", C.c_float), ("tailMs", C.c_float),
                ("emitMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


INSTANCE_DTYPE = np.dtype([("objectToWorld", "<f4", (12,)), ("worldToObject", "<f4", (12,)), ("blas", "<i4"), ("reserved", "<i4", (3,))])


class BlasRange(C.Structure):
    _fields_ = [("nodesOffset", C.c_int64), ("nodesBytes", C.c_int64), ("triWoopOffset", C.c_int64), ("triWoopBytes", C.c_int64)]


class PlocBatchMesh(C.Structure):
    """NtrPlocBatchMesh: triangles [firstTri, +numTris) of the shared index array and the box the mesh's Morton codes are taken over."""
    _fields_ = [("firstTri", C.c_int32), ("numTris", C.c_int32), ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3)]

    def __init__(self, first_tri=0, num_tris=0, scene_min=(0, 0, 0), scene_max=(0, 0, 0)):
        super().__init__(int(first_tri), int(num_tris), (C.c_float * 3)(*[float(x) for x in scene_min]),
                         (C.c_float * 3)(*[float(x) for x in scene_max]))


class PlocBatchMeshResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numRounds", C.c_int32), ("height", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PlocBatchResult(C.Structure):
    _fields_ = [("numMeshes", C.c_int32), ("numRounds", C.c_int32), ("maxHeight", C.c_int32), ("pad", C.c_int32),
                ("numTris", C.c_int64), ("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("seconds", C.c_float), ("checkMs", C.c_float), ("sortMs", C.c_float), ("emitMs", C.c_float), ("roundsMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class RefitBatchEntry(C.Structure):
    """NtrRefitBatchEntry: one BLAS of a pool to refit -- its range, its mesh (triangles [firstTri, +numTris) of the shared index array)
    and the epsilon of its leaf boxes."""
    _fields_ = [("range", BlasRange), ("firstTri", C.c_int32), ("numTris", C.c_int32), ("epsilon", C.c_float), ("pad", C.c_int32)]

    def __init__(self, blas_range=(0, 0, 0, 0), first_tri=0, num_tris=0, epsilon=0.0):
        r = blas_range if isinstance(blas_range, BlasRange) else BlasRange(*[int(x) for x in blas_range])
        super().__init__(r, int(first_tri), int(num_tris), float(epsilon), 0)


class BvhRefitBatchResult(C.Structure):
    _fields_ = [("numEntries", C.c_int32), ("lanesPerLeaf", C.c_int32), ("numNodes", C.c_int64), ("numLeaves", C.c_int64),
                ("numRows", C.c_int64), ("firstBadEntry", C.c_int32), ("errBits", C.c_int32), ("seconds", C.c_float), ("pad", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class BlasTris(C.Structure):
    """NtrBlasTris: BLAS k of a pool is triangles [firstTri, +numTris) of the shared index array (a device array, one per BLAS)."""
    _fields_ = [("firstTri", C.c_int32), ("numTris", C.c_int32)]


BLAS_TRIS_DTYPE = np.dtype([("firstTri", "<i4"), ("numTris", "<i4")])


class InstancedGeometry(C.Structure):
    """NtrInstancedGeometry: a host struct of device pointers -- the instances, the BLASes' triangle ranges, the index array and the
    CURRENT vertex positions."""
    _fields_ = [("numInstances", C.c_int32), ("numBlas", C.c_int32), ("numTrisTotal", C.c_int32), ("numVerts", C.c_int32),
                ("d_instances", C.c_void_p), ("d_blasTris", C.c_void_p), ("d_triVtxIndex", C.c_void_p), ("d_vtxPos", C.c_void_p)]

    def __init__(self, num_instances=0, num_blas=0, num_tris_total=0, num_verts=0, d_instances=0, d_blas_tris=0, d_tri=0, d_pos=0):
        super().__init__(int(num_instances), int(num_blas), int(num_tris_total), int(num_verts), int(d_instances) or None,
                         int(d_blas_tris) or None, int(d_tri) or None, int(d_pos) or None)


class TlasResult(C.Structure):
    _fields_ = [("rootLink", C.c_int32), ("numNodes", C.c_int32), ("numRounds", C.c_int32), ("height", C.c_int32),
                ("tailClusters", C.c_int32), ("pad", C.c_int32 * 3), ("nodesBytes", C.c_int64), ("recordsBytes", C.c_int64),
                ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3), ("seconds", C.c_float), ("boxesMs", C.c_float),
                ("sortMs", C.c_float), ("clustersMs", C.c_float), ("roundsMs", C.c_float), ("tailMs", C.c_float)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.startswith("scene") else getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class TlasRefitResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("errBits", C.c_int32), ("pad", C.c_int32),
                ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3), ("seconds", C.c_float), ("pad2", C.c_float)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k.startswith("scene") else getattr(self, k)) for k, _ in self._fields_ if not k.startswith("pad")}


class TlasMotionRefitResult(C.Structure):
    """NtrTlasMotionRefitResult: ntr_tlas_refit's result and the number of instances that move between the two keys."""
    _fields_ = [("refit", TlasRefitResult), ("numMoving", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return dict(self.refit.as_dict(), numMoving=int(self.numMoving))


class InstanceMotion(C.Structure):
    """NtrInstanceMotion: the motion key buffer tlas_motion_refit wrote (128 bytes per instance) and the rays' times -- a device array
    of num_rays floats, or 0: every ray has `time`."""
    _fields_ = [("d_motionKeys", C.c_void_p), ("motionKeysBytes", C.c_int64), ("d_rayTimes", C.c_void_p), ("time", C.c_float),
                ("pad", C.c_float)]

    def __init__(self, d_motion_keys=0, motion_keys_bytes=0, d_ray_times=0, time=0.0):
        super().__init__(int(d_motion_keys) or None, int(motion_keys_bytes), int(d_ray_times) or None, float(time), 0.0)


class InstancedMotionStats(C.Structure):
    """NtrInstancedMotionStats (the rule is tests/np_instanced_motion.py): entering steps that entered a moving instance, and entering
    steps popped because the instance has no inverse at the ray's time."""
    _fields_ = [(n, C.c_int64) for n in ("numMovingEntries", "numSingular")]

    def algorithmic_bytes(self, stats, instance_masks=False, ray_masks=False, ray_times=False):
        """include/ntrace_amd.h: the masked formula of `stats` (an InstancedTraceStats), 128 B per pose, 4 B per ray with per-ray times."""
        return (stats.algorithmic_bytes(instance_masks, ray_masks) + 128 * (self.numMovingEntries + self.numSingular)
                + (4 * stats.numRays if ray_times else 0))

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class TlasDeformRefitResult(C.Structure):
    """NtrTlasDeformRefitResult: ntr_tlas_motion_refit's result and the number of instances whose BLAS deforms."""
    _fields_ = [("motion", TlasMotionRefitResult), ("numDeforming", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return dict(self.motion.as_dict(), numDeforming=int(self.numDeforming))


class InstanceDeform(C.Structure):
    """NtrInstanceDeform: the pool's key-1 buffers -- the second key's nodes (the pool's node bytes) and the two keys' vertex rows (the
    pool's row bytes each), as bvh_motion_refit wrote them at pool + offset for every deforming BLAS."""
    _fields_ = [("d_poolNodes1", C.c_void_p), ("d_poolVertRows0", C.c_void_p), ("d_poolVertRows1", C.c_void_p)]

    def __init__(self, d_pool_nodes1=0, d_pool_vert_rows0=0, d_pool_vert_rows1=0):
        super().__init__(int(d_pool_nodes1) or None, int(d_pool_vert_rows0) or None, int(d_pool_vert_rows1) or None)


class InstancedDeformGeometry(C.Structure):
    """NtrInstancedDeformGeometry: the vertices at the shutter's close (3 floats per vertex, as many as InstancedGeometry's d_pos, which
    holds the opening) and the per-BLAS deforming flags on the device, as tlas_deform_refit reads them."""
    _fields_ = [("d_vtxPos1", C.c_void_p), ("d_blasDeforming", C.c_void_p)]

    def __init__(self, d_pos1=0, d_blas_deforming=0):
        super().__init__(int(d_pos1) or None, int(d_blas_deforming) or None)


class InstancedDeformStats(C.Structure):
    """NtrInstancedDeformStats (the rule is tests/np_instanced_deform.py): entries into, inner visits in and triangle tests in instances
    of deforming BLASes; each is counted in InstancedTraceStats too."""
    _fields_ = [(n, C.c_int64) for n in ("numDeformEntries", "numDeformInnerVisits", "numDeformTriTests")]

    def algorithmic_bytes(self, stats, motion_stats, instance_masks=False, ray_masks=False, ray_times=False):
        """include/ntrace_amd.h: the motion formula, 64 B more per deforming inner visit and 48 B more per deforming triangle test."""
        return (motion_stats.algorithmic_bytes(stats, instance_masks, ray_masks, ray_times) + 64 * self.numDeformInnerVisits
                + 48 * self.numDeformTriTests)

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class InstancesUpdateResult(C.Structure):
    _fields_ = [("numInstances", C.c_int32), ("numNodes", C.c_int32), ("statusBits", C.c_uint32), ("firstBad", C.c_uint32),
                ("numBad", C.c_uint32), ("pad", C.c_uint32), ("seconds", C.c_float), ("updateMs", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class BvhWideResult(C.Structure):
    _fields_ = [("nodesBytes", C.c_int64), ("numNodes", C.c_int32), ("counts", C.c_int32 * 3), ("numLeafLinks", C.c_int32),
                ("height", C.c_int32), ("stackBound", C.c_int32), ("seconds", C.c_float)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "counts" else getattr(self, k)) for k, _ in self._fields_}


class WideBlasRange(C.Structure):
    """NtrWideBlasRange: wide BLAS k's place in the wide pool, its node count and its stackBound (pool_widen fills them)."""
    _fields_ = [("nodesOffset", C.c_int64), ("nodesBytes", C.c_int64), ("numNodes", C.c_int32), ("stackBound", C.c_int32)]


class TlasWideResult(C.Structure):
    _fields_ = [("nodesBytes", C.c_int64), ("recordsBytes", C.c_int64), ("numNodes", C.c_int32), ("counts", C.c_int32 * 3),
                ("numLeafLinks", C.c_int32), ("height", C.c_int32), ("tlasStackBound", C.c_int32), ("stackBound", C.c_int32),
                ("seconds", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "counts" else getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class WideRefitEntry(C.Structure):
    """NtrWideRefitEntry: one wide BLAS of a wide pool to refit -- its wide range (pool_widen's), its row range (the BLAS's), its mesh
    and the epsilon of its leaf boxes."""
    _fields_ = [("wideNodesOffset", C.c_int64), ("wideNodesBytes", C.c_int64), ("triWoopOffset", C.c_int64), ("triWoopBytes", C.c_int64),
                ("firstTri", C.c_int32), ("numTris", C.c_int32), ("epsilon", C.c_float), ("pad", C.c_int32)]

    def __init__(self, wide_nodes_offset=0, wide_nodes_bytes=0, tri_woop_offset=0, tri_woop_bytes=0, first_tri=0, num_tris=0, epsilon=0.0):
        super().__init__(int(wide_nodes_offset), int(wide_nodes_bytes), int(tri_woop_offset), int(tri_woop_bytes), int(first_tri),
                         int(num_tris), float(epsilon), 0)


class WideRefitResult(C.Structure):
    _fields_ = [("numEntries", C.c_int32), ("lanesPerLeaf", C.c_int32), ("numNodes", C.c_int64), ("numLeafLinks", C.c_int64),
                ("numRows", C.c_int64), ("firstBadEntry", C.c_int32), ("errBits", C.c_int32), ("seconds", C.c_float), ("pad", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class InstancedWideTraceStats(InstancedTraceStats):
    """NtrInstancedTraceStats of the wide two-level trace: numTopInnerVisits and numInnerVisits count wide nodes."""

    def algorithmic_bytes(self, instance_masks=False, ray_masks=False):
        """include/ntrace_amd.h, DESIGN.md 6r: as InstancedTraceStats.algorithmic_bytes, with 112 B (seven fetched rows) per wide node of
        either level and 64 B per instance record."""
        n = (52 * self.numRays + 112 * (self.numTopInnerVisits + self.numInnerVisits) + 64 * self.numInstanceEntries
             + 32 * self.numInstanceEntries + 48 * self.numTriTests + 16 * self.numLeafVisits + 4 * self.numHits)
        if instance_masks:
            n += 4 * (self.numInstanceEntries + self.numInstancesMasked)
        if ray_masks:
            n += 4 * self.numRays
        return n


class BvhRefitResult(C.Structure):
    _fields_ = [("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numRows", C.c_int32), ("pad", C.c_int32), ("seconds", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class BvhMotion(C.Structure):
    """NtrBvhMotion: what bvh_motion_refit wrote beside the key-0 tree (the key-1 nodes and the two keys' vertex rows) and the rays'
    times -- a device array of num_rays floats, or 0: every ray has `time`."""
    _fields_ = [("d_nodes1", C.c_void_p), ("d_vertRows0", C.c_void_p), ("d_vertRows1", C.c_void_p), ("d_rayTimes", C.c_void_p),
                ("time", C.c_float)]

    def __init__(self, d_nodes1=0, d_vert_rows0=0, d_vert_rows1=0, d_ray_times=0, time=0.0):
        super().__init__(int(d_nodes1) or None, int(d_vert_rows0) or None, int(d_vert_rows1) or None, int(d_ray_times) or None, float(time))


class BvhOptimizeResult(C.Structure):
    _fields_ = [("passes", C.c_int32), ("numNodes", C.c_int32), ("numLeafLinks", C.c_int32), ("pad", C.c_int32),
                ("formed", C.c_int32 * 8), ("rewritten", C.c_int32 * 8), ("heightBefore", C.c_int32 * 8), ("heightAfter", C.c_int32 * 8),
                ("seconds", C.c_float)]

    def as_dict(self):
        n = self.passes
        return {k: (list(getattr(self, k))[:n] if k in ("formed", "rewritten", "heightBefore", "heightAfter") else getattr(self, k))
                for k, _ in self._fields_ if k != "pad"}


class BvhReorderResult(C.Structure):
    _fields_ = [("nodesBytes", C.c_int64), ("triWoopBytes", C.c_int64), ("triIndexBytes", C.c_int64),
                ("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numRows", C.c_int32), ("numDroppedSlots", C.c_int32),
                ("seconds", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BvhSahResult(C.Structure):
    _fields_ = [("sahCost", C.c_float), ("numNodes", C.c_int32), ("numLeaves", C.c_int32), ("numTris", C.c_int32), ("height", C.c_int32),
                ("seconds", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


OPT_ERR_LINK, OPT_ERR_ROW, OPT_ERR_NO_TREE = 1, 2, 4   # NTR_OPT_ERR_*: the errBits of the two pool calls below


class BvhOptimizeBatchEntry(C.Structure):
    """NtrBvhOptimizeBatchEntry: what ntr_bvh_optimize_batch found out about one listed BLAS."""
    _fields_ = [("numNodes", C.c_int32), ("numLeafLinks", C.c_int32), ("heightBefore", C.c_int32), ("heightAfter", C.c_int32),
                ("errBits", C.c_int32), ("pad", C.c_int32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad"}


class BvhOptimizeBatchResult(C.Structure):
    _fields_ = [("numEntries", C.c_int32), ("passes", C.c_int32), ("formed", C.c_int64 * 8), ("rewritten", C.c_int64 * 8),
                ("maxHeightBefore", C.c_int32), ("maxHeightAfter", C.c_int32), ("firstBadEntry", C.c_int32), ("errBits", C.c_int32),
                ("launches", C.c_int32), ("readBacks", C.c_int32), ("seconds", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        n = self.passes
        return {k: (list(getattr(self, k))[:n] if k in ("formed", "rewritten") else getattr(self, k)) for k, _ in self._fields_ if k != "pad"}


class BvhSahBatchResult(C.Structure):
    _fields_ = [("numEntries", C.c_int32), ("firstBadEntry", C.c_int32), ("errBits", C.c_int32), ("launches", C.c_int32),
                ("readBacks", C.c_int32), ("seconds", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class _DeviceKdtreeInfo(C.Structure):
    _fields_ = [("nodes", C.c_void_p), ("nodesBytes", C.c_int64), ("triWoop", C.c_void_p),
                ("triWoopBytes", C.c_int64), ("triIndex", C.c_void_p), ("triIndexBytes", C.c_int64),
                ("sceneMin", C.c_float * 3), ("sceneMax", C.c_float * 3), ("delta", C.c_float),
                ("numInnerNodes", C.c_int32), ("numLeafNodes", C.c_int32), ("numEmptyLeaves", C.c_int32), ("numTriRefs", C.c_int32),
                ("maxDepth", C.c_int32), ("numLevels", C.c_int32), ("percentDuplicates", C.c_float), ("seconds", C.c_float),
                ("prepMs", C.c_float), ("levelsMs", C.c_float), ("emitMs", C.c_float)]


def lib_path():
    # NTR_LIB_OVERRIDE: another build of the library (scripts/ only: a patched build for an A/B run, scripts/studies/rejected_patches/)
    return os.environ.get("NTR_LIB_OVERRIDE") or os.path.join(_HERE, "libntrace_amd.so")


_lib = None
_libs = {}   # path -> loaded CDLL (use_library switches between two builds of the library inside one process: scripts/studies/lib_ab.py)

# every symbol include/ntrace_amd.h declares: (name, restype, argtypes)
_vp, _i32, _i64, _u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
SYMBOLS = [
    ("ntr_last_error", C.c_char_p, []),
    ("ntr_version", C.c_int, []),
    ("ntr_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("ntr_set_device", C.c_int, [C.c_int]),
    ("ntr_malloc", C.c_int, [C.POINTER(_vp), C.c_size_t]),
    ("ntr_free", C.c_int, [_vp]),
    ("ntr_memcpy_h2d", C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    ("ntr_memcpy_d2h", C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    ("ntr_memcpy_d2d", C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    ("ntr_memset", C.c_int, [_vp, C.c_int, C.c_size_t, _vp]),
    ("ntr_stream_synchronize", C.c_int, [_vp]),
    ("ntr_query_config", C.c_int, [C.c_char_p, C.POINTER(KernelConfig)]),
    ("ntr_trace_bvh", C.c_int, [C.c_char_p, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _u32, _vp,
                                C.POINTER(C.c_float)]),
    ("ntr_trace_bvh_hinted", C.c_int, [C.c_char_p, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _u32, _vp,
                                       C.POINTER(C.c_float), _vp]),
    ("ntr_trace_status", C.c_int, [_vp, C.POINTER(_u32)]),
    ("ntr_trace_plan", C.c_int, [C.c_char_p, _i32, _i32, C.c_uint64, _i64, C.c_uint64, _i64, _u32, _i32, _i32, _vp]),
    ("ntr_trace_plan_hint_step", C.c_int, [_i32, _i32, _i32, C.POINTER(_i32 * 3)]),
    ("ntr_trace_plan_certain", C.c_int, [_i32, C.POINTER(_i32 * 2)]),
    ("ntr_selftest_gather_rate", C.c_int, [_i64, _i32, _i32, _i32, _vp, C.POINTER(C.c_float)]),
    ("ntr_frame_shard", C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    ("ntr_frame_ao_batches", C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(_i32)]),
    ("ntr_dist_unique_id", C.c_int, [C.c_char_p]),
    ("ntr_dist_init", C.c_int, [C.c_char_p, _i32, _i32, C.POINTER(_vp)]),
    ("ntr_dist_init_all", C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_vp)]),
    ("ntr_dist_info", C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    ("ntr_dist_destroy", C.c_int, [_vp]),
    ("ntr_dist_broadcast", C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    ("ntr_dist_broadcast_bvh", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp]),
    ("ntr_dist_gather_records", C.c_int, [_vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    ("ntr_dist_gather_records_cuts", C.c_int, [_vp, _vp, C.POINTER(_i32), _vp, _i32, _vp]),
    ("ntr_dist_gather_pixels", C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp]),
    ("ntr_tunables_reload", C.c_int, []),
    ("ntr_predict_block_costs", C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp]),
    ("ntr_predict_batch_coherence", C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp]),
    ("ntr_predict_dispatch_order", C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp, _vp]),
    ("ntr_trace_graph_reserve", C.c_int, [_i32, _i32]),
    ("ntr_trace_graph_release_all", C.c_int, []),
    ("ntr_stream_release", C.c_int, [_vp]),
    ("ntr_selftest_auto_hint_table", C.c_int, [_i32, _i32, _i32, C.POINTER(_i32)]),
    ("ntr_lbvh_release_workspace", C.c_int, []),
    ("ntr_sched_hint_create", C.c_int, [C.POINTER(_vp)]),
    ("ntr_sched_hint_destroy", C.c_int, [_vp]),
    ("ntr_sched_hint_reset", C.c_int, [_vp]),
    ("ntr_sched_hint_predict", C.c_int, [_vp, _vp, _i32, _vp]),
    ("ntr_sched_hint_inspect", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("ntr_secondary_block_costs", C.c_int, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    ("ntr_bvh_leaf_depths", C.c_int, [_vp, _i64, _vp, _i64, _vp, _i32, _vp, C.POINTER(_i32), _vp]),
    ("ntr_selftest_division", C.c_int, [_vp, _i32, _vp, _i32, C.POINTER(_u32), _vp]),
    ("ntr_selftest_division_hard", C.c_int, [_i32, _i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), _vp]),
    ("ntr_selftest_ray_class", C.c_int, [_vp, _i32, _u32, C.POINTER(_u32), _vp]),
    ("ntr_selftest_onesweep", C.c_int, [_i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, C.POINTER(_i32), _i32, _vp, _vp, C.POINTER(_u32), _vp]),
    ("ntr_selftest_scan", C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("ntr_selftest_scan_block_sums", C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    ("ntr_selftest_float_order", C.c_int, [_i32, _vp, _vp, _vp, _vp]),
    ("ntr_selftest_box_words", C.c_int, [_i32, _vp, _vp, _i32, C.c_float, _vp, _vp, _vp, _vp, _vp]),
    ("ntr_trace_bvh_stats", C.c_int, [C.c_char_p, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _u32, _vp,
                                      C.POINTER(TraceStats)]),
    ("ntr_bvh_validate", C.c_int, [_vp, _i64, C.POINTER(_u32), _vp]),
    ("ntr_pixel_table", C.c_int, [_i32, _i32, _vp, _vp, _vp]),
    ("ntr_raygen_primary", C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, _i32,
                                     C.c_float, _u32, _vp]),
    ("ntr_raygen_ao", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_float, _u32, _vp]),
    ("ntr_raygen_ao_normals", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_float, _u32, _vp]),
    ("ntr_raygen_shadow", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.POINTER(C.c_float * 3), C.c_float, _u32, _vp]),
    ("ntr_count_hits", C.c_int, [_vp, _i32, C.POINTER(_i32), _vp]),
    ("ntr_lbvh_capacity", C.c_int, [_i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("ntr_lbvh_build", C.c_int, [_i32, _vp, _i32, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, C.c_float,
                                 _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(LbvhResult), _vp]),
    ("ntr_hlbvh_build", C.c_int, [_i32, _vp, _i32, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, C.c_float, _i32,
                                  _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(HlbvhResult), _vp]),
    ("ntr_reconstruct", C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("ntr_ray_morton_sort", C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_float)]),
    ("ntr_camera_decode", C.c_int, [C.c_char_p, C.POINTER(C.c_float)]),
    ("ntr_camera_reencode", C.c_int, [C.c_char_p, C.c_char_p, _i32]),
    ("ntr_camera_nscreen_to_world", C.c_int, [C.c_char_p, _i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                              C.POINTER(C.c_float)]),
    ("ntr_obj_load", C.c_int, [C.c_char_p, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    ("ntr_obj_get", C.c_int, [_vp, _vp, _vp]),
    ("ntr_obj_free", None, [_vp]),
    ("ntr_sah_build", C.c_int, [_i32, _vp, _i32, _vp, _i32, _i32, C.POINTER(_vp)]),
    ("ntr_host_bvh_info", C.c_int, [_vp, C.POINTER(_HostBvhInfo)]),
    ("ntr_host_bvh_free", None, [_vp]),
    ("ntr_host_bvh_wrap", C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(_vp)]),
    ("ntr_host_bvh_trace", C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, C.POINTER(TraceStats)]),
    ("ntr_kdtree_build", C.c_int, [_i32, _i32, _vp, _i32, _vp, _i32, C.POINTER(_vp)]),
    ("ntr_kdtree_device_params_default", C.c_int, [C.POINTER(KdtreeDeviceParams)]),
    ("ntr_kdtree_device_build", C.c_int, [_i32, _vp, _i32, _vp, C.POINTER(KdtreeDeviceParams), C.POINTER(_vp), _vp]),
    ("ntr_device_kdtree_info", C.c_int, [_vp, C.POINTER(_DeviceKdtreeInfo)]),
    ("ntr_device_kdtree_free", None, [_vp]),
    ("ntr_device_kdtree_download", C.c_int, [_vp, _vp, _vp, _vp]),
    ("ntr_kdtree_device_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_persistent_bvh_params_default", C.c_int, [C.POINTER(PersistentBvhParams)]),
    ("ntr_persistent_bvh_build", C.c_int, [_i32, _vp, _i32, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(PersistentBvhParams),
                                           _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(PersistentBvhResult), _vp]),
    ("ntr_persistent_bvh_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_sah_device_build", C.c_int, [_i32, _vp, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(SahDeviceResult), _vp]),
    ("ntr_sah_device_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_ploc_build", C.c_int, [_i32, _vp, _i32, _vp, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, _vp, _i64, _vp, _i64, _vp, _i64,
                                 C.POINTER(PlocResult), _vp]),
    ("ntr_ploc_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_instance_invert", C.c_int, [_vp, _vp]),
    ("ntr_ploc_batch_capacity", C.c_int, [_i32, _vp, _vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    ("ntr_ploc_build_batch", C.c_int, [_i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp,
                                       C.POINTER(PlocBatchResult), _vp]),
    ("ntr_ploc_batch_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_capacity", C.c_int, [_i32, C.POINTER(_i64), C.POINTER(_i64)]),
    ("ntr_tlas_build", C.c_int, [_i32, _vp, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, C.POINTER(TlasResult), _vp]),
    ("ntr_tlas_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_refit", C.c_int, [_i32, _vp, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, C.POINTER(TlasRefitResult), _vp]),
    ("ntr_tlas_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_motion_refit", C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                        C.POINTER(TlasMotionRefitResult), _vp]),
    ("ntr_tlas_motion_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_deform_refit", C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                        C.POINTER(TlasDeformRefitResult), _vp]),
    ("ntr_tlas_deform_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_trace_instanced_deform", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                             C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion), C.POINTER(InstanceDeform),
                                             C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_deform_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                   C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion), C.POINTER(InstanceDeform),
                                                   C.POINTER(InstancedTraceStats), C.POINTER(InstancedMotionStats),
                                                   C.POINTER(InstancedDeformStats), _vp]),
    ("ntr_trace_instanced_motion", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                             C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_motion_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                   C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion), C.POINTER(InstancedTraceStats),
                                                   C.POINTER(InstancedMotionStats), _vp]),
    ("ntr_instances_update", C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, C.POINTER(InstancesUpdateResult), _vp]),
    ("ntr_instances_status_read", C.c_int, [_vp, C.POINTER(_u32 * 4), _vp]),
    ("ntr_instances_update_host", C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp, C.POINTER(_u32 * 4)]),
    ("ntr_trace_instanced", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp, C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_masked", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                             C.POINTER(InstanceVisibility), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                            C.POINTER(InstanceVisibility), C.POINTER(InstancedTraceStats), _vp]),
    ("ntr_instanced_hit_attributes", C.c_int, [_i32, _vp, _vp, C.POINTER(InstancedGeometry), _vp, _vp, _vp]),
    ("ntr_instanced_hit_attributes_motion", C.c_int, [_i32, _vp, _vp, C.POINTER(InstancedGeometry), C.POINTER(InstanceMotion), _vp, _vp, _vp]),
    ("ntr_instanced_hit_attributes_deform", C.c_int, [_i32, _vp, _vp, C.POINTER(InstancedGeometry), C.POINTER(InstanceMotion),
                                                      C.POINTER(InstancedDeformGeometry), _vp, _vp, _vp]),
    ("ntr_ray_times_primary", C.c_int, [_i32, _vp, _u32, C.c_float, C.c_float, _vp, _vp]),
    ("ntr_ray_times_secondary", C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    ("ntr_bvh_widen_capacity", C.c_int, [_i64, C.POINTER(_i64)]),
    ("ntr_bvh_widen", C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(BvhWideResult), _vp]),
    ("ntr_bvh_widen_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_trace_wide", C.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _u32, _vp, C.POINTER(C.c_float)]),
    ("ntr_trace_wide_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _u32, _vp, C.POINTER(TraceStats)]),
    ("ntr_pool_widen_capacity", C.c_int, [_i32, _vp, C.POINTER(_i64)]),
    ("ntr_pool_widen", C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, C.POINTER(BvhWideResult), _vp]),
    ("ntr_pool_widen_batch", C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, C.POINTER(BvhWideResult), _vp]),
    ("ntr_pool_widen_batch_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_widen", C.c_int, [_i32, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, C.POINTER(TlasWideResult), _vp]),
    ("ntr_trace_instanced_wide", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                           C.POINTER(InstanceVisibility), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_wide_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                 C.POINTER(InstanceVisibility), C.POINTER(InstancedWideTraceStats), _vp]),
    ("ntr_trace_instanced_seeded", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                             C.POINTER(InstanceVisibility), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_seeded_stats", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                   C.POINTER(InstanceVisibility), C.POINTER(InstancedTraceStats), _vp]),
    ("ntr_trace_instanced_wide_seeded", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                  C.POINTER(InstanceVisibility), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_wide_seeded_stats", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64,
                                                        _vp, C.POINTER(InstanceVisibility), C.POINTER(InstancedWideTraceStats), _vp]),
    ("ntr_instanced_validate", C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    ("ntr_instanced_flags_read", C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), _vp]),
    ("ntr_trace_instanced_fast", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                           C.POINTER(InstanceVisibility), _vp, C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_fast_stats", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                 C.POINTER(InstanceVisibility), _vp, C.POINTER(InstancedTraceStats),
                                                 C.POINTER(InstancedFastStats), _vp]),
    ("ntr_instanced_wide_validate", C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    ("ntr_trace_instanced_wide_fast", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                C.POINTER(InstanceVisibility), _vp, C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_wide_fast_stats", C.c_int, [_i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64,
                                                      _vp, C.POINTER(InstanceVisibility), _vp, C.POINTER(InstancedWideTraceStats),
                                                      C.POINTER(InstancedFastStats), _vp]),
    ("ntr_pool_wide_refit", C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _vp, C.POINTER(WideRefitResult), _vp]),
    ("ntr_pool_wide_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_wide_refit", C.c_int, [_i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, C.POINTER(TlasRefitResult), _vp]),
    ("ntr_tlas_wide_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_tlas_wide_motion_refit", C.c_int, [_i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                             C.POINTER(TlasMotionRefitResult), _vp]),
    ("ntr_tlas_wide_motion_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_trace_instanced_wide_motion", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                  C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion), C.POINTER(C.c_float), _vp]),
    ("ntr_trace_instanced_wide_motion_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                                                        C.POINTER(InstanceVisibility), C.POINTER(InstanceMotion),
                                                        C.POINTER(InstancedTraceStats), C.POINTER(InstancedMotionStats), _vp]),
    ("ntr_bvh_refit", C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i32, _vp, C.c_float, _vp, C.POINTER(BvhRefitResult), _vp]),
    ("ntr_bvh_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_bvh_motion_refit", C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp, _i32, _vp, _vp, C.c_float, _vp,
                                       C.POINTER(BvhRefitResult), _vp]),
    ("ntr_bvh_motion_refit_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_trace_bvh_motion", C.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, C.POINTER(BvhMotion), _vp, C.POINTER(C.c_float)]),
    ("ntr_trace_bvh_motion_stats", C.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, C.POINTER(BvhMotion), _vp, C.POINTER(TraceStats)]),
    ("ntr_bvh_refit_batch", C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _vp, C.POINTER(BvhRefitBatchResult), _vp]),
    ("ntr_bvh_refit_batch_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_bvh_motion_refit_batch", C.c_int, [_i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp,
                                             C.POINTER(BvhRefitBatchResult), _vp]),
    ("ntr_bvh_motion_refit_batch_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_bvh_optimize", C.c_int, [_vp, _i64, _i32, C.POINTER(BvhOptimizeResult), _vp]),
    ("ntr_bvh_optimize_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_bvh_sah_cost", C.c_int, [_vp, _i64, _vp, _i64, C.POINTER(BvhSahResult), _vp]),
    ("ntr_bvh_optimize_batch", C.c_int, [_i32, _vp, _vp, _i64, _i32, _vp, C.POINTER(BvhOptimizeBatchResult), _vp]),
    ("ntr_bvh_optimize_batch_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_bvh_sah_cost_batch", C.c_int, [_i32, _vp, _vp, _i64, _vp, _i64, _vp, C.POINTER(BvhSahBatchResult), _vp]),
    ("ntr_bvh_reorder", C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(BvhReorderResult), _vp]),
    ("ntr_bvh_reorder_scratch_bytes", C.c_int, [C.POINTER(_i64)]),
    ("ntr_host_kdtree_info", C.c_int, [_vp, C.POINTER(_HostKdtreeInfo)]),
    ("ntr_host_kdtree_free", None, [_vp]),
    ("ntr_host_kdtree_wrap", C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(_vp)]),
    ("ntr_trace_kdtree", C.c_int, [_i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float), _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64,
                                   _vp, C.POINTER(C.c_float)]),
]


def _load(path):
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError("ntrace_amd: %s not found -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP extension is mandatory; there is no CPU fallback)" % path)
        # When torch is in the process it must load its bundled libamdhip64 first: our library
        # then binds to that same HIP runtime (two HIP runtimes in one process do not share the
        # device).  Without torch (C++ hosts) the system /opt/rocm runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _libs[path] = L
    return _libs[path]


def lib():
    """Load libntrace_amd.so; raises if it was not built (no fallback)."""
    global _lib
    if _lib is None:
        _lib = _load(lib_path())
    return _lib


def use_library(path=None):
    """Scripts only: make `path` (default: the product library, or NTR_LIB_OVERRIDE) the library every wrapper of this module calls.
    Two builds of the library can be loaded in one process (an A/B run of a patched build); each has its own tunables and workspaces."""
    global _lib
    _lib = _load(path or lib_path())
    return _lib


def _check(rc):
    if rc != 0:
        raise NtrError(rc, (lib().ntr_last_error() or b"").decode("utf-8", "replace"))


def query_config(kernel):
    cfg = KernelConfig()
    _check(lib().ntr_query_config(kernel.encode(), C.byref(cfg)))
    return cfg


class SchedHint:
    """NtrSchedHint: block-order feedback for repeated traces of one logical batch (include/ntrace_amd.h)."""

    def __init__(self):
        self._h = _vp()
        _check(lib().ntr_sched_hint_create(C.byref(self._h)))

    def reset(self):
        _check(lib().ntr_sched_hint_reset(self._h))

    def predict(self, d_block_cost, num_blocks, stream=0):
        """ntr_sched_hint_predict: dispatch the batch's next launch by these per-block cost estimates (device pointer, uint32 per block)"""
        _check(lib().ntr_sched_hint_predict(self._h, _vp(d_block_cost), int(num_blocks), _vp(stream)))

    def inspect(self, stream=0):
        """ntr_sched_hint_inspect (waits for `stream`): {numBlocks, device, uses, valid, predicted} plus, for a bound hint, "order" (its
        numBlocks block indices), "words" (the 3 batch words stored after them) and "cost" (its numBlocks cost words), as uint32 arrays"""
        st = SchedHintState()
        _check(lib().ntr_sched_hint_inspect(self._h, C.byref(st), None, None, _vp(stream)))
        out = {n: int(getattr(st, n)) for n, _ in st._fields_}
        if st.numBlocks > 0:
            order = np.zeros(st.numBlocks + 3, np.uint32)
            cost = np.zeros(st.numBlocks, np.uint32)
            _check(lib().ntr_sched_hint_inspect(self._h, C.byref(st), order.ctypes.data_as(_vp), cost.ctypes.data_as(_vp), _vp(stream)))
            out.update({n: int(getattr(st, n)) for n, _ in st._fields_})
            out["order"], out["words"], out["cost"] = order[:st.numBlocks], order[st.numBlocks:], cost
        return out

    def close(self):
        if self._h:
            lib().ntr_sched_hint_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trace_bvh(kernel, num_rays, any_hit, d_rays, d_results, d_nodes, nodes_bytes, d_woop, woop_bytes, d_tri_index,
              layout=4, bvh_flags=0, stream=0, timed=True, hint=None):
    """ntr_trace_bvh (ntr_trace_bvh_hinted with a SchedHint) on raw device pointers (ints).
    Returns GPU seconds if timed else None."""
    sec = C.c_float(0.0)
    args = (kernel.encode(), int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results), _vp(d_nodes), int(nodes_bytes),
            _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(layout), int(bvh_flags), _vp(stream),
            C.byref(sec) if timed else None)
    if hint is None:
        _check(lib().ntr_trace_bvh(*args))
    else:
        _check(lib().ntr_trace_bvh_hinted(*args, hint._h))
    return float(sec.value) if timed else None


class TracePlan(C.Structure):
    """NtrTracePlan (include/ntrace_amd.h): what ntr_trace_bvh decides before it touches the device."""
    _fields_ = [(n, C.c_int32) for n in (
        "variant", "launchVariant", "launchBlocks", "numBlocks", "orderBlocks", "chunk", "fetchThreshold", "leafSwitchBelow", "octant",
        "flatFetch", "uniformPrologue", "splitSlice", "numHeads", "shardRays", "numBlocksIncoherent", "numBlocksDivergent", "wholeWave", "prefetchAfter", "unified", "minipool", "poolKConst",
        "poolKFromDevice", "minipoolWide", "hintable", "useAutoHint", "predictable", "persistentOrder", "probeOnRefresh", "coherentRoute",
        "persistentVariant", "persistentBlocks", "persistentFetchThreshold", "perrayBlocks", "perrayFetchThreshold")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


PLAN_FLAG_STATS, PLAN_FLAG_CAPTURING, PLAN_FLAG_CALLER_HINT = 1, 2, 4


def trace_plan(kernel, num_rays, any_hit, nodes_bytes, woop_bytes, nodes_addr=1 << 32, woop_addr=None, bvh_flags=0, num_cus=256, flags=0):
    """ntr_trace_plan: the launch plan of such a batch (no device needed)."""
    if woop_addr is None:
        woop_addr = nodes_addr + nodes_bytes
    pl = TracePlan()
    _check(lib().ntr_trace_plan(kernel.encode(), int(num_rays), int(bool(any_hit)), int(nodes_addr), int(nodes_bytes), int(woop_addr),
                                int(woop_bytes), int(bvh_flags), int(num_cus), int(flags), C.byref(pl)))
    return pl


def trace_plan_hint_step(valid, predicted, uses):
    out = (_i32 * 3)()
    _check(lib().ntr_trace_plan_hint_step(int(bool(valid)), int(bool(predicted)), int(uses), C.byref(out)))
    return dict(zeroK=bool(out[0]), refresh=bool(out[1]), useOrder=bool(out[2]))


def trace_plan_certain(any_hit):
    """ntr_trace_plan_certain: what the tunables make of the prologue's certain steps for such a launch (no device needed)."""
    out = (_i32 * 2)()
    _check(lib().ntr_trace_plan_certain(int(bool(any_hit)), C.byref(out)))
    return dict(certainSteps=bool(out[0]), certainDescent=bool(out[1]))


def trace_status(stream=0):
    """ntr_trace_status: waits for `stream`, raises NtrError(NTR_ERR_OVERFLOW) if a launch since the last check
    overflowed its traversal stack; returns the status bits otherwise."""
    bits = _u32(0)
    _check(lib().ntr_trace_status(_vp(stream), C.byref(bits)))
    return int(bits.value)


def selftest_gather_rate(table_bytes, waves, lanes_per_wave=64, steps=256, stream=0):
    """ntr_selftest_gather_rate: seconds of the best of three launches of waves x lanes dependent chains of `steps` random 64-byte records."""
    sec = C.c_float(0.0)
    _check(lib().ntr_selftest_gather_rate(int(table_bytes), int(waves), int(lanes_per_wave), int(steps), _vp(stream), C.byref(sec)))
    return float(sec.value)


def frame_shard(num_primary, rank, world, align=64):
    """ntr_frame_shard: the rank-th of `world` contiguous align-aligned ranges of [0, num_primary)."""
    lo, hi = _i32(0), _i32(0)
    _check(lib().ntr_frame_shard(int(num_primary), int(rank), int(world), int(align), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def frame_ao_batches(lo, hi, samples, max_batch_rays):
    """ntr_frame_ao_batches: [(first input slot, inputs)] of the AO batches of the input range [lo, hi)."""
    n = _i32(0)
    _check(lib().ntr_frame_ao_batches(int(lo), int(hi), int(samples), int(max_batch_rays), None, None, 0, C.byref(n)))
    first, count = (_i32 * max(n.value, 1))(), (_i32 * max(n.value, 1))()
    _check(lib().ntr_frame_ao_batches(int(lo), int(hi), int(samples), int(max_batch_rays), first, count, n.value, C.byref(n)))
    return [(int(first[i]), int(count[i])) for i in range(n.value)]


class DistGroup:
    """ntr_dist_*: the native RCCL group of this process' GPU (one process per GPU).  `uid` = DistGroup.unique_id() of the root, handed to
    every rank by the caller."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().ntr_dist_unique_id(buf))
        return buf.raw

    def __init__(self, uid, rank, world, _handle=None):
        if _handle is not None:
            self._h, self.rank, self.world = _handle, int(rank), int(world)
            return
        h = _vp()
        _check(lib().ntr_dist_init(C.c_char_p(uid), int(rank), int(world), C.byref(h)))
        self._h, self.rank, self.world = h, int(rank), int(world)

    @staticmethod
    def init_all(devices):
        """ntr_dist_init_all: one group object per device of THIS process, for one host thread per GPU (thread i: ntr_set_device(devices[i]),
        then groups[i])."""
        n = len(devices)
        devs = (_i32 * n)(*[int(x) for x in devices])
        hs = (_vp * n)()
        _check(lib().ntr_dist_init_all(n, devs, hs))
        return [DistGroup(None, i, n, _handle=_vp(hs[i])) for i in range(n)]

    def broadcast(self, d_buf, nbytes, root=0, stream=0):
        _check(lib().ntr_dist_broadcast(self._h, _vp(d_buf), int(nbytes), int(root), _vp(stream)))

    def broadcast_bvh(self, d_nodes, nodes_bytes, d_woop, woop_bytes, d_tri_index, tri_index_bytes, root=0, stream=0):
        _check(lib().ntr_dist_broadcast_bvh(self._h, _vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(tri_index_bytes),
                                            int(root), _vp(stream)))

    def gather_records(self, d_own, num_primary, d_full, root=0, stream=0, align=64):
        _check(lib().ntr_dist_gather_records(self._h, _vp(d_own), int(num_primary), int(align), _vp(d_full), int(root), _vp(stream)))

    def gather_records_cuts(self, d_own, cuts, d_full, root=0, stream=0):
        """ntr_dist_gather_records_cuts: ranges cut by the host (world + 1 slot indices, the same table on every rank)."""
        if len(cuts) != self.world + 1:
            raise ValueError("gather_records_cuts: %d cut points for %d ranks" % (len(cuts), self.world))
        c = (_i32 * (self.world + 1))(*[int(x) for x in cuts])
        _check(lib().ntr_dist_gather_records_cuts(self._h, _vp(d_own), c, _vp(d_full), int(root), _vp(stream)))

    def gather_pixels(self, d_own_pixels, d_slot_to_pixel, num_primary, d_full_pixels, d_scratch, root=0, stream=0, align=64):
        _check(lib().ntr_dist_gather_pixels(self._h, _vp(d_own_pixels), _vp(d_slot_to_pixel), int(num_primary), int(align), _vp(d_full_pixels), _vp(d_scratch),
                                            int(root), _vp(stream)))

    def close(self):
        if self._h:
            lib().ntr_dist_destroy(self._h)
            self._h = None


def predict_batch_coherence(num_rays, d_rays, d_nodes, nodes_bytes, d_out, stream=0):
    """ntr_predict_batch_coherence: d_out[0] = 256-ray blocks whose sample rays start far apart, d_out[1] = the divergence score (4 per block
    of long rays that start together and point apart, 1 per block with a degenerate sample ray), d_out[2] = the batch word (bits 0-15 the
    pool K, bit 16 NTR_BATCH_DIVERGENT)."""
    _check(lib().ntr_predict_batch_coherence(int(num_rays), _vp(d_rays), _vp(d_nodes), int(nodes_bytes), _vp(d_out), _vp(stream)))


def predict_dispatch_order(num_rays, d_rays, d_nodes, nodes_bytes, d_order, d_word, stream=0):
    """ntr_predict_dispatch_order (blocking): the block order a large closest-hit launch of this batch would be given, into d_order
    ((num_rays + 255) // 256 words), and its batch word, into d_word (1 word)."""
    _check(lib().ntr_predict_dispatch_order(int(num_rays), _vp(d_rays), _vp(d_nodes), int(nodes_bytes), _vp(d_order), _vp(d_word), _vp(stream)))


def predict_block_costs(num_rays, d_rays, d_nodes, nodes_bytes, d_block_cost, stream=0):
    """ntr_predict_block_costs: predicted cost (top-of-tree boxes hit by the sample ray) of every 256-ray block, into d_block_cost."""
    _check(lib().ntr_predict_block_costs(int(num_rays), _vp(d_rays), _vp(d_nodes), int(nodes_bytes), _vp(d_block_cost), _vp(stream)))


def trace_graph_reserve(launches, num_rays):
    """ntr_trace_graph_reserve: provision scratch for `launches` captured launches of num_rays rays."""
    _check(lib().ntr_trace_graph_reserve(int(launches), int(num_rays)))


def trace_graph_release_all():
    """ntr_trace_graph_release_all: return every resource pinned by captured launches (call when their graphs are destroyed)."""
    _check(lib().ntr_trace_graph_release_all())


def stream_release(stream=0):
    """ntr_stream_release: return the scheduling state (automatic hints, prediction scratch) `stream` owns on the current device; call
    before destroying the stream."""
    _check(lib().ntr_stream_release(_vp(stream)))


def selftest_auto_hint_table(devices, keys_per_device, rounds=3):
    """ntr_selftest_auto_hint_table: per simulated device, the batches that found their automatic hint in the last round (CPU only)."""
    out = (_i32 * devices)()
    _check(lib().ntr_selftest_auto_hint_table(devices, keys_per_device, rounds, out))
    return [int(x) for x in out]


def lbvh_release_workspace():
    _check(lib().ntr_lbvh_release_workspace())


def set_tunables(**kv):
    """Sweep helper: set NTR_* environment tunables (None removes one) and make the library re-read them."""
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    _check(lib().ntr_tunables_reload())


def bvh_leaf_depths(d_nodes, nodes_bytes, d_woop, woop_bytes, d_tri_index, num_tris, d_depth_by_tri, stream=0):
    """ntr_bvh_leaf_depths: depth of every triangle's leaf into d_depth_by_tri (int32 per triangle); returns the number of levels walked"""
    m = _i32(0)
    _check(lib().ntr_bvh_leaf_depths(_vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(num_tris),
                                     _vp(d_depth_by_tri), C.byref(m), _vp(stream)))
    return int(m.value)


def secondary_block_costs(d_in_results, first, count, num_samples, d_depth_by_tri, num_tris, d_block_cost, stream=0):
    """ntr_secondary_block_costs: predicted cost of the 256-ray blocks of a secondary batch (deepest leaf among a block's input rays)"""
    _check(lib().ntr_secondary_block_costs(_vp(d_in_results), int(first), int(count), int(num_samples), _vp(d_depth_by_tri), int(num_tris),
                                           _vp(d_block_cost), _vp(stream)))


def selftest_division(d_x, nx, d_d, nd, stream=0):
    m = _u32(0)
    _check(lib().ntr_selftest_division(_vp(d_x), int(nx), _vp(d_d), int(nd), C.byref(m), _vp(stream)))
    return int(m.value)


def selftest_division_hard(x_exp, d_exp, stream=0):
    """(pairs tested, mismatches) of the FAST divide on the enumerated near-midpoint quotients (ntr_selftest_division_hard)"""
    n, m = C.c_uint64(0), C.c_uint64(0)
    _check(lib().ntr_selftest_division_hard(int(x_exp), int(d_exp), C.byref(n), C.byref(m), _vp(stream)))
    return int(n.value), int(m.value)


def selftest_ray_class(d_rays, num_rays, bvh_flags, stream=0):
    """rays on which the kernels' integer FAST-path admission test (ray_class) differs from the rule's float ranges (ntr_selftest_ray_class)"""
    m = _u32(0)
    _check(lib().ntr_selftest_ray_class(_vp(d_rays), int(num_rays), int(bvh_flags), C.byref(m), _vp(stream)))
    return int(m.value)


SCAN_U32, SCAN_I32, SCAN_U64, SCAN_U4 = 0, 1, 2, 3
_SCAN_ITEM_BYTES = {SCAN_U32: 4, SCAN_I32: 4, SCAN_U64: 8, SCAN_U4: 16}
# the (ITEMS, MODE, SKIP_TRIVIAL) instantiations of the one-sweep pass that the builders and the ray sort launch (mode 1 has no user)
ONESWEEP_COMBOS = ((8, 0, False), (16, 0, False), (24, 0, False), (32, 0, False), (8, 2, False), (8, 0, True), (8, 2, True))
ONESWEEP_MAX_PASS = 125


def selftest_onesweep(items, mode, skip_trivial, n, d_keys, stride, d_vals, passes, force_ticket, d_keys_out, d_vals_out, stream=0):
    """ntr_selftest_onesweep: n keys through the passes [(shift, pass number), ...] of one production instantiation of the one-sweep
    radix pass; the last pass's keys and values to d_keys_out / d_vals_out.  Returns the passes' error word (0: no look-back gave up)."""
    flat = (_i32 * (2 * len(passes)))(*[int(x) for p in passes for x in p])
    err = _u32(0xFFFFFFFF)
    _check(lib().ntr_selftest_onesweep(int(items), int(mode), int(bool(skip_trivial)), int(n), _vp(d_keys), int(stride), _vp(d_vals), len(passes),
                                       flat, int(bool(force_ticket)), _vp(d_keys_out), _vp(d_vals_out), C.byref(err), _vp(stream)))
    return int(err.value)


def selftest_scan(scan_type, threads, n, d_in, d_prefix, stream=0):
    """ntr_selftest_scan: the three-launch exclusive scan of n items into d_prefix; returns the total as the item's bytes"""
    total = (C.c_uint8 * 16)()
    _check(lib().ntr_selftest_scan(int(scan_type), int(threads), int(n), _vp(d_in), _vp(d_prefix), C.cast(total, _vp), _vp(stream)))
    return bytes(total)[:_SCAN_ITEM_BYTES[scan_type]]


def selftest_scan_block_sums(scan_type, threads, nb, d_in, d_out, want_total=True, stream=0):
    """ntr_selftest_scan_block_sums: scan_block_sums alone on nb sums (d_out == d_in: in place); the total's bytes, or None if not asked for"""
    total = (C.c_uint8 * 16)()
    _check(lib().ntr_selftest_scan_block_sums(int(scan_type), int(threads), int(nb), _vp(d_in), _vp(d_out),
                                              C.cast(total, _vp) if want_total else None, _vp(stream)))
    return bytes(total)[:_SCAN_ITEM_BYTES[scan_type]] if want_total else None


def selftest_float_order(n, d_words, d_single, d_pairs, stream=0):
    """ntr_selftest_float_order: the encodings of n float words to d_single [n][6], ord_min / ord_max of every ordered pair to d_pairs [n][n][2]"""
    _check(lib().ntr_selftest_float_order(int(n), _vp(d_words), _vp(d_single), _vp(d_pairs), _vp(stream)))


def selftest_box_words(m, d_boxes, d_group, groups, eps, d_lane32, d_lane64, d_groups_out, d_folds_out, stream=0):
    """ntr_selftest_box_words: m boxes merged into their groups by atomic_max_box and through wave_grouped_atomic, decoded to
    d_groups_out [2][groups][26]; the wave folds of the lane words to d_folds_out [m][6]"""
    _check(lib().ntr_selftest_box_words(int(m), _vp(d_boxes), _vp(d_group), int(groups), float(eps), _vp(d_lane32), _vp(d_lane64),
                                        _vp(d_groups_out), _vp(d_folds_out), _vp(stream)))


def trace_bvh_stats(kernel, num_rays, any_hit, d_rays, d_results, d_nodes, nodes_bytes, d_woop, woop_bytes,
                    d_tri_index, layout=4, bvh_flags=0, stream=0):
    st = TraceStats()
    _check(lib().ntr_trace_bvh_stats(kernel.encode(), int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results),
                                     _vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_tri_index),
                                     int(layout), int(bvh_flags), _vp(stream), C.byref(st)))
    return st


def bvh_validate(d_nodes, nodes_bytes, stream=0):
    flags = _u32(0)
    _check(lib().ntr_bvh_validate(_vp(d_nodes), int(nodes_bytes), C.byref(flags), _vp(stream)))
    return int(flags.value)


def pixel_table(w, h, d_index_to_pixel, d_pixel_to_index=0, stream=0):
    _check(lib().ntr_pixel_table(int(w), int(h), _vp(d_index_to_pixel), _vp(d_pixel_to_index), _vp(stream)))


def raygen_primary(d_rays, d_id_to_slot, d_slot_to_id, d_index_to_pixel, origin, nscreen_to_world, w, h, max_dist,
                   kernel_seed=0, stream=0):
    o = (C.c_float * 3)(*[float(x) for x in origin])
    m = (C.c_float * 16)(*[float(x) for x in np.asarray(nscreen_to_world, dtype=np.float32).reshape(-1)])
    _check(lib().ntr_raygen_primary(_vp(d_rays), _vp(d_id_to_slot), _vp(d_slot_to_id), _vp(d_index_to_pixel), o, m,
                                    int(w), int(h), float(max_dist), int(kernel_seed), _vp(stream)))


def raygen_ao(d_out_rays, d_out_id_to_slot, d_out_slot_to_id, d_in_rays, d_in_results, d_tri_normals, first_input_slot,
              num_input_rays, num_samples, max_dist, kernel_seed=0, stream=0):
    _check(lib().ntr_raygen_ao(_vp(d_out_rays), _vp(d_out_id_to_slot), _vp(d_out_slot_to_id), _vp(d_in_rays),
                               _vp(d_in_results), _vp(d_tri_normals), int(first_input_slot), int(num_input_rays),
                               int(num_samples), float(max_dist), int(kernel_seed), _vp(stream)))


def raygen_ao_normals(d_out_rays, d_out_id_to_slot, d_out_slot_to_id, d_in_rays, d_in_results, d_ray_normals, first_input_slot,
                      num_input_rays, num_samples, max_dist, kernel_seed=0, stream=0):
    """ntr_raygen_ao_normals: raygen_ao over per-ray normals (4 floats per input slot, as instanced_hit_attributes writes them); a
    fourth word of zero is a missed input.  Asynchronous on `stream` and capturable."""
    _check(lib().ntr_raygen_ao_normals(_vp(d_out_rays), _vp(d_out_id_to_slot), _vp(d_out_slot_to_id), _vp(d_in_rays),
                                       _vp(d_in_results), _vp(d_ray_normals), int(first_input_slot), int(num_input_rays),
                                       int(num_samples), float(max_dist), int(kernel_seed), _vp(stream)))


def raygen_shadow(d_out_rays, d_out_id_to_slot, d_out_slot_to_id, d_in_rays, d_in_results, first_input_slot, num_input_rays, num_samples,
                  light_pos, light_radius, kernel_seed=0, stream=0):
    lp = (C.c_float * 3)(*[float(x) for x in light_pos])
    _check(lib().ntr_raygen_shadow(_vp(d_out_rays), _vp(d_out_id_to_slot), _vp(d_out_slot_to_id), _vp(d_in_rays), _vp(d_in_results),
                                   int(first_input_slot), int(num_input_rays), int(num_samples), C.byref(lp), float(light_radius),
                                   int(kernel_seed), _vp(stream)))


def count_hits(d_results, num_rays, stream=0):
    cnt = _i32(0)
    _check(lib().ntr_count_hits(_vp(d_results), int(num_rays), C.byref(cnt), _vp(stream)))
    return int(cnt.value)


def reconstruct(ray_type, rays_per_primary, first_primary, num_primary, d_primary_slot_to_id, d_primary_results,
                d_batch_id_to_slot, d_batch_results, d_tri_material_color, d_tri_shaded_color, d_pixels, stream=0):
    _check(lib().ntr_reconstruct(int(ray_type), int(rays_per_primary), int(first_primary), int(num_primary),
                                 _vp(d_primary_slot_to_id), _vp(d_primary_results), _vp(d_batch_id_to_slot),
                                 _vp(d_batch_results), _vp(d_tri_material_color), _vp(d_tri_shaded_color), _vp(d_pixels),
                                 _vp(stream)))


def ray_morton_sort(num_rays, d_in_rays, d_in_slot_to_id, d_out_rays, d_out_id_to_slot, d_out_slot_to_id, stream=0):
    sec = C.c_float(0.0)
    _check(lib().ntr_ray_morton_sort(int(num_rays), _vp(d_in_rays), _vp(d_in_slot_to_id), _vp(d_out_rays),
                                     _vp(d_out_id_to_slot), _vp(d_out_slot_to_id), _vp(stream), C.byref(sec)))
    return float(sec.value)


def lbvh_capacity(num_tris):
    a, b, c = _i64(0), _i64(0), _i64(0)
    _check(lib().ntr_lbvh_capacity(int(num_tris), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def lbvh_build(num_tris, d_tri, num_verts, d_pos, scene_min, scene_max, leaf_size, epsilon, d_nodes, nodes_cap,
               d_woop, woop_cap, d_idx, idx_cap, stream=0):
    res = LbvhResult()
    mn = (C.c_float * 3)(*[float(x) for x in scene_min])
    mx = (C.c_float * 3)(*[float(x) for x in scene_max])
    _check(lib().ntr_lbvh_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos), mn, mx, int(leaf_size),
                                float(epsilon), _vp(d_nodes), int(nodes_cap), _vp(d_woop), int(woop_cap), _vp(d_idx),
                                int(idx_cap), C.byref(res), _vp(stream)))
    return res


def hlbvh_build(num_tris, d_tri, num_verts, d_pos, scene_min, scene_max, leaf_size, epsilon, hlbvh_bits, d_nodes, nodes_cap,
                d_woop, woop_cap, d_idx, idx_cap, stream=0):
    """ntr_hlbvh_build: binned SAH over Morton clusters (HLBVHBuilder::buildHLBVH) into Compact buffers of lbvh_capacity() bytes."""
    res = HlbvhResult()
    mn = (C.c_float * 3)(*[float(x) for x in scene_min])
    mx = (C.c_float * 3)(*[float(x) for x in scene_max])
    _check(lib().ntr_hlbvh_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos), mn, mx, int(leaf_size), float(epsilon),
                                 int(hlbvh_bits), _vp(d_nodes), int(nodes_cap), _vp(d_woop), int(woop_cap), _vp(d_idx), int(idx_cap),
                                 C.byref(res), _vp(stream)))
    return res


PERSISTENT_BVH_DEFAULTS = dict(triLimit=16, triMaxLimit=16, maxDepth=50, ci=1.0, ct=1.0, epsilon=float(np.finfo(np.float32).eps))


def persistent_bvh_params(**kw):
    """NtrPersistentBvhParams: config.conf's PersistentBVH block (epsilon FLT_EPSILON) with the given fields replaced."""
    p = PersistentBvhParams()
    _check(lib().ntr_persistent_bvh_params_default(C.byref(p)))
    for k, v in kw.items():
        if k not in PERSISTENT_BVH_DEFAULTS:
            raise TypeError("unknown persistent BVH parameter %r" % k)
        setattr(p, k, v)
    return p


def persistent_bvh_build(num_tris, d_tri, num_verts, d_pos, scene_min, scene_max, d_nodes, nodes_cap, d_woop, woop_cap, d_idx, idx_cap,
                         params=None, stream=0):
    """ntr_persistent_bvh_build: binned SAH on the device (the reference's PersistentBVH) into Compact buffers of lbvh_capacity() bytes.
    params: None (the defaults), a dict of NtrPersistentBvhParams fields, or a PersistentBvhParams.  Returns a PersistentBvhResult."""
    if isinstance(params, dict):
        params = persistent_bvh_params(**params)
    res = PersistentBvhResult()
    mn = (C.c_float * 3)(*[float(x) for x in scene_min])
    mx = (C.c_float * 3)(*[float(x) for x in scene_max])
    _check(lib().ntr_persistent_bvh_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos), mn, mx,
                                          C.byref(params) if params is not None else None, _vp(d_nodes), int(nodes_cap), _vp(d_woop),
                                          int(woop_cap), _vp(d_idx), int(idx_cap), C.byref(res), _vp(stream)))
    return res


def persistent_bvh_scratch_bytes():
    """ntr_persistent_bvh_scratch_bytes: bytes the device BVH builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_persistent_bvh_scratch_bytes(C.byref(v)))
    return int(v.value)


def sah_device_build(num_tris, d_tri, num_verts, d_pos, d_nodes, nodes_cap, d_woop, woop_cap, d_idx, idx_cap, min_leaf=1, max_leaf=1,
                     stream=0):
    """ntr_sah_device_build: the host SAH builder's tree (sah_build, leaf preferences min_leaf / max_leaf) built on the device by full
    sweeps over three presorted axis orders, into Compact buffers of at least lbvh_capacity() bytes.  Returns a SahDeviceResult."""
    res = SahDeviceResult()
    _check(lib().ntr_sah_device_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos), int(min_leaf), int(max_leaf), _vp(d_nodes),
                                      int(nodes_cap), _vp(d_woop), int(woop_cap), _vp(d_idx), int(idx_cap), C.byref(res), _vp(stream)))
    return res


def sah_device_scratch_bytes():
    """ntr_sah_device_scratch_bytes: bytes the device SAH builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_sah_device_scratch_bytes(C.byref(v)))
    return int(v.value)


PLOC_TAIL, PLOC_TILE = 1024, 1024   # NTR_PLOC_TAIL, NTR_PLOC_TILE (include/ntrace_amd.h)


def ploc_build(num_tris, d_tri, num_verts, d_pos, scene_min, scene_max, d_nodes, nodes_cap, d_woop, woop_cap, d_idx, idx_cap, radius=8,
               stream=0):
    """ntr_ploc_build: PLOC over the LBVH's Morton order (mutual nearest neighbours within `radius` list positions merge, round by
    round; the rule is tests/np_bvh_ploc.py) into Compact buffers of at least lbvh_capacity() bytes.  Returns a PlocResult."""
    res = PlocResult()
    mn = (C.c_float * 3)(*[float(x) for x in scene_min])
    mx = (C.c_float * 3)(*[float(x) for x in scene_max])
    _check(lib().ntr_ploc_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos), mn, mx, int(radius), _vp(d_nodes), int(nodes_cap),
                                _vp(d_woop), int(woop_cap), _vp(d_idx), int(idx_cap), C.byref(res), _vp(stream)))
    return res


def ploc_scratch_bytes():
    """ntr_ploc_scratch_bytes: bytes the PLOC builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_ploc_scratch_bytes(C.byref(v)))
    return int(v.value)


def _batch_meshes(meshes):
    """A ctypes array of PlocBatchMesh from PlocBatchMesh objects or (firstTri, numTris, sceneMin, sceneMax) tuples."""
    if isinstance(meshes, C.Array):
        return meshes
    items = [m if isinstance(m, PlocBatchMesh) else PlocBatchMesh(*m) for m in meshes]
    return (PlocBatchMesh * max(len(items), 1))(*items)


def _range_tuples(arr, n):
    return [tuple(r) for r in np.frombuffer(arr, np.int64).reshape(-1, 4)[:n].tolist()]


def ploc_batch_capacity(meshes):
    """ntr_ploc_batch_capacity (host only) -> (nodesBytes, triWoopBytes, triIndexBytes, ranges): the exact extents of the pool that
    ploc_build_batch(meshes) writes and every mesh's (nodesOffset, nodesBytes, triWoopOffset, triWoopBytes)."""
    n = len(meshes)
    arr = _batch_meshes(meshes)
    ranges = (BlasRange * max(n, 1))()
    a, b, c = _i64(0), _i64(0), _i64(0)
    _check(lib().ntr_ploc_batch_capacity(n, C.cast(arr, _vp), C.cast(ranges, _vp), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value), _range_tuples(ranges, n)


def ploc_build_batch(meshes, num_tris_total, d_tri, num_verts, d_pos, d_pool_nodes, nodes_cap, d_pool_woop, woop_cap, d_pool_idx, idx_cap,
                     radius=8, stream=0):
    """ntr_ploc_build_batch: every mesh of `meshes` (PlocBatchMesh objects or (firstTri, numTris, sceneMin, sceneMax) tuples over one shared
    index array) becomes one BLAS of the pool, all in the same launches; each BLAS is byte for byte ploc_build's tree of that mesh (the
    rule is tests/np_ploc_batch.py).  Returns (PlocBatchResult, ranges, mesh_results): ranges as tlas_build takes them, mesh_results an
    array of PlocBatchMeshResult.  An NtrError raised after the work (a tree too high) carries .ranges and .mesh_results too."""
    n = len(meshes)
    arr = _batch_meshes(meshes)
    ranges = (BlasRange * max(n, 1))()
    per_mesh = (PlocBatchMeshResult * max(n, 1))()
    res = PlocBatchResult()
    try:
        _check(lib().ntr_ploc_build_batch(n, C.cast(arr, _vp), int(num_tris_total), _vp(d_tri), int(num_verts), _vp(d_pos), int(radius),
                                          _vp(d_pool_nodes), int(nodes_cap), _vp(d_pool_woop), int(woop_cap), _vp(d_pool_idx), int(idx_cap),
                                          C.cast(ranges, _vp), C.cast(per_mesh, _vp), C.byref(res), _vp(stream)))
    except NtrError as e:
        e.ranges, e.mesh_results = _range_tuples(ranges, n), per_mesh
        raise
    return res, _range_tuples(ranges, n), per_mesh


def ploc_batch_scratch_bytes():
    """ntr_ploc_batch_scratch_bytes: bytes the batch PLOC builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_ploc_batch_scratch_bytes(C.byref(v)))
    return int(v.value)


def instance_invert(object_to_world):
    """ntr_instance_invert (host only): worldToObject, 12 float32, from a 3x4 row-major objectToWorld (the rule: tests/np_instanced.py)."""
    m = np.ascontiguousarray(np.asarray(object_to_world, np.float32).reshape(12))
    out = np.zeros(12, np.float32)
    _check(lib().ntr_instance_invert(m.ctypes.data, out.ctypes.data))
    return out


def make_instances(transforms, blas):
    """An INSTANCE_DTYPE array from objectToWorld matrices (n, 12) and BLAS indices; worldToObject by instance_invert."""
    transforms = np.asarray(transforms, np.float32).reshape(-1, 12)
    inst = np.zeros(transforms.shape[0], INSTANCE_DTYPE)
    inst["objectToWorld"] = transforms
    for i, t in enumerate(transforms):
        inst["worldToObject"][i] = instance_invert(t)
    inst["blas"] = np.asarray(blas, np.int32)
    return inst


class BlasPool:
    """Hands out aligned offsets of a pool's three buffers and remembers the ranges.  add(nodes_bytes, woop_bytes) -> (index,
    nodesOffset, triWoopOffset): a builder is handed pool + offset (triIndex + triWoopOffset / 4), or a finished tree is copied there."""

    def __init__(self):
        self.ranges = []
        self.nodes_bytes = self.woop_bytes = 0

    def add(self, nodes_bytes, woop_bytes):
        nodes_bytes = (int(nodes_bytes) + 63) // 64 * 64
        woop_bytes = (int(woop_bytes) + 15) // 16 * 16
        r = (self.nodes_bytes, nodes_bytes, self.woop_bytes, woop_bytes)
        self.ranges.append(r)
        self.nodes_bytes += nodes_bytes
        self.woop_bytes += woop_bytes
        return len(self.ranges) - 1, r[0], r[2]

    @property
    def tri_index_bytes(self):
        return self.woop_bytes // 4

    def c_ranges(self):
        return (BlasRange * len(self.ranges))(*[BlasRange(*r) for r in self.ranges])


def tlas_capacity(num_instances):
    """ntr_tlas_capacity -> (nodesBytes, recordsBytes)"""
    a, b = _i64(0), _i64(0)
    _check(lib().ntr_tlas_capacity(int(num_instances), C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def tlas_build(num_instances, d_instances, ranges, d_pool_nodes, pool_nodes_bytes, d_tlas_nodes, tlas_nodes_cap, d_records, records_cap,
               radius=8, stream=0):
    """ntr_tlas_build: the top-level tree over instances (world boxes, Morton order, ntr_ploc_build's rounds; the rule is
    tests/np_instanced.py).  ranges: a BlasPool or a list of (nodesOffset, nodesBytes, triWoopOffset, triWoopBytes).  Returns a TlasResult."""
    if isinstance(ranges, BlasPool):
        ranges = ranges.ranges
    arr = (BlasRange * max(len(ranges), 1))(*[BlasRange(*[int(x) for x in r]) for r in ranges])
    res = TlasResult()
    _check(lib().ntr_tlas_build(int(num_instances), _vp(d_instances), len(ranges), C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes),
                                int(radius), _vp(d_tlas_nodes), int(tlas_nodes_cap), _vp(d_records), int(records_cap), C.byref(res), _vp(stream)))
    return res


def tlas_scratch_bytes():
    """ntr_tlas_scratch_bytes: bytes the top-level builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_refit(num_instances, d_instances, ranges, d_pool_nodes, pool_nodes_bytes, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
               records_cap, d_scene_box=0, stream=0, blocking=True):
    """ntr_tlas_refit: keep a top-level tree's topology and rewrite its instance records and every box from the current instances and the
    pool's current node-0 boxes (an extension; the rule is tests/np_tlas_refit.py).  ranges as for tlas_build.  blocking=True returns a
    TlasRefitResult; blocking=False passes result = NULL: asynchronous on `stream` (capturable) and returns None.  An NtrError raised
    after the device work (a bad blas index, a malformed tree) carries .result, filled: errBits and the counts."""
    if isinstance(ranges, BlasPool):
        ranges = ranges.ranges
    arr = (BlasRange * max(len(ranges), 1))(*[BlasRange(*[int(x) for x in r]) for r in ranges])
    res = TlasRefitResult() if blocking else None
    try:
        _check(lib().ntr_tlas_refit(int(num_instances), _vp(d_instances), len(ranges), C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes),
                                    _vp(d_tlas_nodes), int(tlas_nodes_bytes), int(root_link), _vp(d_records), int(records_cap), _vp(d_scene_box),
                                    C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def tlas_refit_scratch_bytes():
    """ntr_tlas_refit_scratch_bytes: bytes the TLAS refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_motion_refit(num_instances, d_instances0, d_instances1, ranges, d_pool_nodes, pool_nodes_bytes, d_tlas_nodes, tlas_nodes_bytes,
                      root_link, d_records, records_cap, d_motion_keys, motion_keys_cap, d_scene_box=0, stream=0, blocking=True):
    """ntr_tlas_motion_refit: tlas_refit over two keys of the instances (shutter open, shutter close): swept leaf boxes, word 15 of a
    moving instance's record, and the motion key buffer (128 bytes per instance) that trace_instanced_motion reads; the rule is
    tests/np_instanced_motion.py.  blocking=True returns a TlasMotionRefitResult; blocking=False passes result = NULL: asynchronous on
    `stream` (capturable) and returns None.  An NtrError raised after the device work carries .result, filled."""
    if isinstance(ranges, BlasPool):
        ranges = ranges.ranges
    arr = (BlasRange * max(len(ranges), 1))(*[BlasRange(*[int(x) for x in r]) for r in ranges])
    res = TlasMotionRefitResult() if blocking else None
    try:
        _check(lib().ntr_tlas_motion_refit(int(num_instances), _vp(d_instances0), _vp(d_instances1), len(ranges), C.cast(arr, _vp),
                                           _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_tlas_nodes), int(tlas_nodes_bytes), int(root_link),
                                           _vp(d_records), int(records_cap), _vp(d_motion_keys), int(motion_keys_cap), _vp(d_scene_box),
                                           C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def tlas_motion_refit_scratch_bytes():
    """ntr_tlas_motion_refit_scratch_bytes: bytes the motion refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_motion_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_deform_refit(num_instances, d_instances0, d_instances1, ranges, d_pool_nodes, d_pool_nodes1, pool_nodes_bytes, d_blas_deforming,
                      d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, records_cap, d_motion_keys, motion_keys_cap, d_scene_box=0,
                      stream=0, blocking=True):
    """ntr_tlas_deform_refit: tlas_motion_refit over a pool in which some BLASes deform within the shutter: leaf boxes over {key 0, key 1
    of the instance} x {key 0, key 1 of the BLAS}, bit 1 of record word 15; the rule is tests/np_instanced_deform.py.  d_pool_nodes1: the
    pool's second node buffer; d_blas_deforming: one uint32 per BLAS on the device.  blocking=True returns a TlasDeformRefitResult;
    blocking=False passes result = NULL: asynchronous on `stream` (capturable) and returns None."""
    if isinstance(ranges, BlasPool):
        ranges = ranges.ranges
    arr = (BlasRange * max(len(ranges), 1))(*[BlasRange(*[int(x) for x in r]) for r in ranges])
    res = TlasDeformRefitResult() if blocking else None
    try:
        _check(lib().ntr_tlas_deform_refit(int(num_instances), _vp(d_instances0), _vp(d_instances1), len(ranges), C.cast(arr, _vp),
                                           _vp(d_pool_nodes), _vp(d_pool_nodes1), int(pool_nodes_bytes), _vp(d_blas_deforming),
                                           _vp(d_tlas_nodes), int(tlas_nodes_bytes), int(root_link), _vp(d_records), int(records_cap),
                                           _vp(d_motion_keys), int(motion_keys_cap), _vp(d_scene_box), C.byref(res) if blocking else None,
                                           _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def tlas_deform_refit_scratch_bytes():
    """ntr_tlas_deform_refit_scratch_bytes: bytes the deform refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_deform_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


INSTANCE_MAX_CHAIN = 16
INSTANCE_ERR_SINGULAR, INSTANCE_ERR_CHAIN = 1, 2


def instances_update(num_nodes, d_node_local, d_node_parent, num_instances, d_instance_node, d_blas, d_instances, d_status, stream=0,
                     blocking=True):
    """ntr_instances_update: the NtrInstance array from a hierarchy of transforms, composed and inverted on the device in one launch (an
    extension; the rule is tests/np_instance_update.py).  d_node_parent 0: every node is a root; d_instance_node 0: instance i uses node
    i.  d_status: 16 bytes, reset ahead of the kernel.  blocking=True returns an InstancesUpdateResult; blocking=False passes result =
    NULL: asynchronous on `stream` (capturable from the first call on) and returns None.  An NtrError raised after the device work (a
    bad chain, a singular transform) carries .result, filled."""
    res = InstancesUpdateResult() if blocking else None
    try:
        _check(lib().ntr_instances_update(int(num_nodes), _vp(d_node_local), _vp(d_node_parent), int(num_instances), _vp(d_instance_node),
                                          _vp(d_blas), _vp(d_instances), _vp(d_status), C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def instances_status_read(d_status, stream=0):
    """ntr_instances_status_read -> [bits, lowest bad instance (0xFFFFFFFF: none), bad instances, 0].  Blocks on `stream`."""
    st = (_u32 * 4)()
    _check(lib().ntr_instances_status_read(_vp(d_status), C.byref(st), _vp(stream)))
    return [int(x) for x in st]


def instances_update_host(node_local, node_parent, num_instances, instance_node, blas):
    """ntr_instances_update_host (no device): -> (INSTANCE_DTYPE array, status: 4 uint32).  node_parent None: every node is a root;
    instance_node None: instance i uses node i.  An NtrError for a bad instance carries .instances and .status, filled."""
    local = np.ascontiguousarray(np.asarray(node_local, np.float32).reshape(-1, 12))
    parent = None if node_parent is None else np.ascontiguousarray(node_parent, np.int32).reshape(local.shape[0])
    node = None if instance_node is None else np.ascontiguousarray(instance_node, np.int32).reshape(int(num_instances))
    blas = np.ascontiguousarray(blas, np.int32).reshape(max(int(num_instances), 0))
    out = np.zeros(max(int(num_instances), 0), INSTANCE_DTYPE)
    st = (_u32 * 4)()
    try:
        _check(lib().ntr_instances_update_host(local.shape[0], local.ctypes.data, None if parent is None else parent.ctypes.data,
                                               int(num_instances), None if node is None else node.ctypes.data, blas.ctypes.data,
                                               out.ctypes.data, C.byref(st)))
    except NtrError as e:
        e.instances, e.status = out, np.array(list(st), np.uint32)
        raise
    return out, np.array(list(st), np.uint32)


_ABSENT = object()   # an argument that an entry point does not have (None is a value: NULL)


def _trace_two_level(name, out, num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                     num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, seed=_ABSENT,
                     vis=_ABSENT, d_flags=_ABSENT, motion=_ABSENT, deform=_ABSENT):
    """The one marshalling of the ntr_trace_instanced* entry points (binary or wide buffers alike).  After the rays `seed`, a
    (d_seed_results, seed_instance) pair; after the pool `vis`, `d_flags` and `motion`; then the out-arguments and the stream.  out: True or False
    (`timed`: a float -> the seconds, or NULL -> None), or the classes of the stats -> one object of each (alone, or a tuple)."""
    outs = [C.c_float(0.0)] if isinstance(out, bool) else [cls() for cls in out]
    args = [int(num_rays), int(bool(any_hit)), _vp(d_rays)]
    if seed is not _ABSENT:
        args += [_vp(seed[0]), int(seed[1])]
    args += [_vp(d_results), _vp(d_instance_ids), _vp(d_tlas_nodes), int(tlas_nodes_bytes), int(root_link), _vp(d_records), int(num_instances),
             _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_pool_woop), int(pool_woop_bytes), _vp(d_pool_tri_index)]
    if vis is not _ABSENT:
        args.append(C.byref(vis) if vis is not None else None)
    if d_flags is not _ABSENT:
        args.append(_vp(d_flags))
    if motion is not _ABSENT:
        args.append(C.byref(motion) if motion is not None else None)
    if deform is not _ABSENT:
        args.append(C.byref(deform) if deform is not None else None)
    _check(getattr(lib(), name)(*args, *([None] if out is False else [C.byref(o) for o in outs]), _vp(stream)))
    if isinstance(out, bool):
        return float(outs[0].value) if out else None
    return outs[0] if len(outs) == 1 else tuple(outs)


def trace_instanced(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, num_instances,
                    d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream=0, timed=True):
    """ntr_trace_instanced: closest or any hit through the top-level tree and the instances' trees.  timed=True returns the GPU seconds;
    timed=False is asynchronous on `stream` (capturable) and returns None."""
    return _trace_two_level("ntr_trace_instanced", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes,
                            root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index,
                            stream)


def trace_instanced_masked(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                           num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, stream=0,
                           timed=True):
    """ntr_trace_instanced_masked: trace_instanced with instance visibility (the rule is tests/np_instanced_masked.py).  vis: an
    InstanceVisibility, or None (NULL: no masks, the unmasked kernel).  timed=True returns the GPU seconds; timed=False is asynchronous
    on `stream` (capturable; the mask arrays are read at replay time) and returns None."""
    return _trace_two_level("ntr_trace_instanced_masked", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, vis=vis)


def trace_instanced_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                          num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, stream=0):
    """ntr_trace_instanced_stats: trace_instanced_masked's records through the instrumented kernel -> InstancedTraceStats.  Blocks; not
    a timed path; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_stats", (InstancedTraceStats,), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, vis=vis)


def trace_instanced_motion(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                           num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, motion=None,
                           stream=0, timed=True):
    """ntr_trace_instanced_motion: trace_instanced_masked with time-sampled instance transforms (the rule is
    tests/np_instanced_motion.py).  motion: an InstanceMotion over what tlas_motion_refit wrote, or None (NULL: trace_instanced_masked).
    timed=False is asynchronous on `stream` (capturable; times, keys and records are read at replay time) and returns None."""
    return _trace_two_level("ntr_trace_instanced_motion", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, vis=vis, motion=motion)


def trace_instanced_motion_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                                 num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None,
                                 motion=None, stream=0):
    """ntr_trace_instanced_motion_stats: trace_instanced_motion's records through the instrumented kernel ->
    (InstancedTraceStats, InstancedMotionStats).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_motion_stats", (InstancedTraceStats, InstancedMotionStats), num_rays, any_hit, d_rays, d_results,
                            d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes,
                            d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, vis=vis, motion=motion)


def trace_instanced_deform(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                           num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, motion=None,
                           deform=None, stream=0, timed=True):
    """ntr_trace_instanced_deform: trace_instanced_motion over a pool in which some BLASes deform (the rule is
    tests/np_instanced_deform.py).  deform: an InstanceDeform over the pool's key-1 buffers, or None (NULL: trace_instanced_motion).
    timed=False is asynchronous on `stream` (capturable) and returns None."""
    return _trace_two_level("ntr_trace_instanced_deform", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, vis=vis, motion=motion, deform=deform)


def trace_instanced_deform_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                                 num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None,
                                 motion=None, deform=None, stream=0):
    """ntr_trace_instanced_deform_stats: trace_instanced_deform's records through the instrumented kernel ->
    (InstancedTraceStats, InstancedMotionStats, InstancedDeformStats).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_deform_stats", (InstancedTraceStats, InstancedMotionStats, InstancedDeformStats), num_rays,
                            any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, num_instances,
                            d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, vis=vis, motion=motion,
                            deform=deform)


def instanced_hit_attributes(num_rays, d_results, d_instance_ids, geom, d_out_results=0, d_normals=0, stream=0):
    """ntr_instanced_hit_attributes: per ray of a two-level trace, the record with the pool triangle g = firstTri + id in place of the
    BLAS's own id (d_out_results; may be d_results) and the world-space geometric normal of the hit triangle from the current vertices
    (d_normals, 4 floats per ray); the rule is tests/np_instanced_frame.py.  geom: an InstancedGeometry (None passes NULL).
    Asynchronous on `stream` and capturable."""
    _check(lib().ntr_instanced_hit_attributes(int(num_rays), _vp(d_results), _vp(d_instance_ids), C.byref(geom) if geom is not None else None,
                                              _vp(d_out_results), _vp(d_normals), _vp(stream)))


def instanced_hit_attributes_motion(num_rays, d_results, d_instance_ids, geom, motion, d_out_results=0, d_normals=0, stream=0):
    """ntr_instanced_hit_attributes_motion: instanced_hit_attributes with the normal of a moving instance's hit at the ray's time (the
    rule is tests/np_instanced_motion_frame.py).  motion: the InstanceMotion trace_instanced_motion took, or None (NULL:
    instanced_hit_attributes).  Asynchronous on `stream` and capturable."""
    _check(lib().ntr_instanced_hit_attributes_motion(int(num_rays), _vp(d_results), _vp(d_instance_ids), C.byref(geom) if geom is not None else None,
                                                     C.byref(motion) if motion is not None else None, _vp(d_out_results), _vp(d_normals),
                                                     _vp(stream)))


def instanced_hit_attributes_deform(num_rays, d_results, d_instance_ids, geom, motion, deform, d_out_results=0, d_normals=0, stream=0):
    """ntr_instanced_hit_attributes_deform: instanced_hit_attributes_motion with the triangle of a deforming BLAS's hit posed at the ray's
    time too (the rule is tests/np_instanced_deform_frame.py).  motion: the InstanceMotion trace_instanced_deform took; deform: an
    InstancedDeformGeometry, or None (NULL: instanced_hit_attributes_motion).  Asynchronous on `stream` and capturable."""
    _check(lib().ntr_instanced_hit_attributes_deform(int(num_rays), _vp(d_results), _vp(d_instance_ids), C.byref(geom) if geom is not None else None,
                                                     C.byref(motion) if motion is not None else None,
                                                     C.byref(deform) if deform is not None else None, _vp(d_out_results), _vp(d_normals),
                                                     _vp(stream)))


def ray_times_primary(num_rays, d_slot_to_id, seed, open, close, d_times, stream=0):
    """ntr_ray_times_primary: one hashed time per pixel id (d_slot_to_id, or 0: id = slot) and seed in the shutter [open, close]; the
    rule is tests/np_instanced_motion_frame.py.  Asynchronous on `stream` and capturable."""
    _check(lib().ntr_ray_times_primary(int(num_rays), _vp(d_slot_to_id), int(seed) & 0xFFFFFFFF, float(open), float(close), _vp(d_times),
                                       _vp(stream)))


def ray_times_secondary(d_in_times, first_input_slot, num_input_rays, num_samples, d_out_times, stream=0):
    """ntr_ray_times_secondary: output slot k * num_samples + j takes the time of input slot first_input_slot + k (raygen_ao_normals'
    slot rule), the word verbatim.  Asynchronous on `stream` and capturable."""
    _check(lib().ntr_ray_times_secondary(_vp(d_in_times), int(first_input_slot), int(num_input_rays), int(num_samples), _vp(d_out_times),
                                         _vp(stream)))


def bvh_widen_capacity(nodes_bytes):
    """ntr_bvh_widen_capacity -> the bytes a wide node buffer for a Compact tree of nodes_bytes needs at most (128 per binary slot)."""
    v = _i64(0)
    _check(lib().ntr_bvh_widen_capacity(int(nodes_bytes), C.byref(v)))
    return int(v.value)


def bvh_widen(d_nodes, nodes_bytes, d_wide_nodes, wide_capacity, stream=0):
    """ntr_bvh_widen: any Compact tree into 4-wide nodes, out of place (an extension; the rule is tests/np_bvh_wide.py).  Leaves, Woop
    rows and triIndex stay the binary tree's.  Returns a BvhWideResult; result.nodesBytes is what was written."""
    res = BvhWideResult()
    _check(lib().ntr_bvh_widen(_vp(d_nodes), int(nodes_bytes), _vp(d_wide_nodes), int(wide_capacity), C.byref(res), _vp(stream)))
    return res


def bvh_widen_scratch_bytes():
    """ntr_bvh_widen_scratch_bytes: bytes the widening pass's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_widen_scratch_bytes(C.byref(v)))
    return int(v.value)


def trace_wide(num_rays, any_hit, d_rays, d_results, d_wide_nodes, wide_nodes_bytes, d_woop, woop_bytes, d_tri_index, bvh_flags=0, stream=0,
               timed=True):
    """ntr_trace_wide: closest or any hit through a 4-wide tree (bvh_widen) over the binary tree's Woop rows and triIndex.  bvh_flags:
    the binary tree's validated flags, or 0 -- the records are the same.  timed=True returns the GPU seconds; timed=False is
    asynchronous on `stream` (capturable) and returns None."""
    sec = C.c_float(0.0)
    _check(lib().ntr_trace_wide(int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results), _vp(d_wide_nodes), int(wide_nodes_bytes),
                                _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(bvh_flags), _vp(stream), C.byref(sec) if timed else None))
    return float(sec.value) if timed else None


def trace_wide_stats(num_rays, any_hit, d_rays, d_results, d_wide_nodes, wide_nodes_bytes, d_woop, woop_bytes, d_tri_index, bvh_flags=0,
                     stream=0):
    """ntr_trace_wide_stats: trace_wide's records through the instrumented kernel -> TraceStats (numInnerVisits counts wide nodes)."""
    st = TraceStats()
    _check(lib().ntr_trace_wide_stats(int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results), _vp(d_wide_nodes), int(wide_nodes_bytes),
                                      _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(bvh_flags), _vp(stream), C.byref(st)))
    return st


def _blas_ranges(ranges):
    if isinstance(ranges, BlasPool):
        ranges = ranges.ranges
    return (BlasRange * max(len(ranges), 1))(*[BlasRange(*[int(x) for x in r]) for r in ranges]), len(ranges)


def _wide_ranges(wide_ranges):
    """a list of (nodesOffset, nodesBytes, numNodes, stackBound) -> the C array"""
    return (WideBlasRange * max(len(wide_ranges), 1))(*[WideBlasRange(*[int(x) for x in r]) for r in wide_ranges])


def pool_widen_capacity(ranges):
    """ntr_pool_widen_capacity -> the bytes a wide pool for these BLAS ranges needs at most (the sum of bvh_widen_capacity)."""
    arr, n = _blas_ranges(ranges)
    v = _i64(0)
    _check(lib().ntr_pool_widen_capacity(n, C.cast(arr, _vp), C.byref(v)))
    return int(v.value)


def pool_widen(ranges, d_pool_nodes, pool_nodes_bytes, d_wide_pool_nodes, capacity, stream=0):
    """ntr_pool_widen: every BLAS of a pool into 4-wide nodes, BLAS k at the sum of the exact extents before it (an extension; the rule
    is tests/np_instanced_wide.py).  ranges as for tlas_build.  -> (wide_ranges, BvhWideResult): a list of (nodesOffset, nodesBytes,
    numNodes, stackBound) per BLAS, and the pool's totals (nodesBytes is the wide pool's extent, stackBound the largest of any BLAS)."""
    arr, n = _blas_ranges(ranges)
    out = (WideBlasRange * max(n, 1))()
    res = BvhWideResult()
    _check(lib().ntr_pool_widen(n, C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_wide_pool_nodes), int(capacity),
                                C.cast(out, _vp), C.byref(res), _vp(stream)))
    return [(int(w.nodesOffset), int(w.nodesBytes), int(w.numNodes), int(w.stackBound)) for w in out[:n]], res


def pool_widen_batch(ranges, d_pool_nodes, pool_nodes_bytes, d_wide_pool_nodes, capacity, stream=0):
    """ntr_pool_widen_batch: pool_widen's arguments, bytes and return value, every BLAS in one pass -- the launches and read-backs
    follow the tallest BLAS, not the number of BLASes.  On an overflow nothing is written (stricter than pool_widen's loop)."""
    arr, n = _blas_ranges(ranges)
    out = (WideBlasRange * max(n, 1))()
    res = BvhWideResult()
    _check(lib().ntr_pool_widen_batch(n, C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_wide_pool_nodes), int(capacity),
                                      C.cast(out, _vp), C.byref(res), _vp(stream)))
    return [(int(w.nodesOffset), int(w.nodesBytes), int(w.numNodes), int(w.stackBound)) for w in out[:n]], res


def pool_widen_batch_scratch_bytes():
    """ntr_pool_widen_batch_scratch_bytes: bytes the batched pool widening's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_pool_widen_batch_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_widen(num_instances, d_instances, d_tlas_nodes, tlas_nodes_bytes, root_link, ranges, wide_ranges, d_wide_tlas_nodes, capacity,
               d_wide_records, records_cap, stream=0):
    """ntr_tlas_widen: the top-level tree into 4-wide nodes (none for one instance) and the wide instance records.  ranges as for
    tlas_build, wide_ranges as pool_widen returned them.  -> TlasWideResult; stackBound <= 104 guarantees that
    trace_instanced_wide's stack never overflows."""
    arr, n = _blas_ranges(ranges)
    warr = _wide_ranges(wide_ranges)
    res = TlasWideResult()
    _check(lib().ntr_tlas_widen(int(num_instances), _vp(d_instances), _vp(d_tlas_nodes), int(tlas_nodes_bytes), int(root_link), n,
                                C.cast(arr, _vp), C.cast(warr, _vp), _vp(d_wide_tlas_nodes), int(capacity), _vp(d_wide_records),
                                int(records_cap), C.byref(res), _vp(stream)))
    return res


def trace_instanced_wide(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                         d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                         d_pool_tri_index, vis=None, stream=0, timed=True):
    """ntr_trace_instanced_wide: trace_instanced_masked over 4-wide trees (tlas_widen, pool_widen); the rule is
    tests/np_instanced_wide.py.  vis: an InstanceVisibility or None.  timed=True returns the GPU seconds; timed=False is asynchronous on
    `stream` (capturable) and returns None."""
    return _trace_two_level("ntr_trace_instanced_wide", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes,
                            wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop,
                            pool_woop_bytes, d_pool_tri_index, stream, vis=vis)


def trace_instanced_wide_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                               d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                               d_pool_tri_index, vis=None, stream=0):
    """ntr_trace_instanced_wide_stats: trace_instanced_wide's records through the instrumented kernel -> InstancedWideTraceStats
    (numTopInnerVisits and numInnerVisits count wide nodes).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_wide_stats", (InstancedWideTraceStats,), num_rays, any_hit, d_rays, d_results, d_instance_ids,
                            d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes,
                            wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, vis=vis)


def trace_instanced_seeded(num_rays, any_hit, d_rays, d_seed_results, seed_instance, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes,
                           root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index,
                           vis=None, stream=0, timed=True):
    """ntr_trace_instanced_seeded: trace_instanced_masked started from one result record per ray (the rule is
    tests/np_instanced_seeded.py): tmax from a seed that is a hit, an any-hit ray whose seed is a hit never starts, a ray that accepts
    nothing keeps the seed's four words and, for a hit, seed_instance.  d_results may be d_seed_results.  The intended seed is trace_bvh
    of the world BLAS's range of the pool.  timed=True returns the GPU seconds; timed=False is asynchronous on `stream` (capturable) and
    returns None."""
    return _trace_two_level("ntr_trace_instanced_seeded", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis)


def trace_instanced_seeded_stats(num_rays, any_hit, d_rays, d_seed_results, seed_instance, d_results, d_instance_ids, d_tlas_nodes,
                                 tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop,
                                 pool_woop_bytes, d_pool_tri_index, vis=None, stream=0):
    """ntr_trace_instanced_seeded_stats: trace_instanced_seeded's records through the instrumented kernel -> InstancedTraceStats (the
    seed read adds 16 B per ray to algorithmic_bytes).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_seeded_stats", (InstancedTraceStats,), num_rays, any_hit, d_rays, d_results, d_instance_ids,
                            d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop,
                            pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis)


def instanced_validate(d_tlas_nodes, tlas_nodes_bytes, d_pool_nodes, pool_nodes_bytes, d_flags, stream=0):
    """ntr_instanced_validate: the withheld validate bits of the top-level tree and of the pool into d_flags[0] and d_flags[1] (four
    words, 16-byte aligned; the rule is tests/np_instanced_fast.py, validate).  Asynchronous on `stream` and capturable; to be run
    again after every call that rewrites a node box, before the next trace_instanced_fast."""
    _check(lib().ntr_instanced_validate(_vp(d_tlas_nodes), int(tlas_nodes_bytes), _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_flags),
                                        _vp(stream)))


def instanced_flags_read(d_flags, stream=0):
    """ntr_instanced_flags_read -> (granted top-level flags, granted pool flags): the complement of d_flags[0] and d_flags[1] within
    BVH_FINITE | BVH_FASTDIV | BVH_NOTINY | BVH_ORDERED.  Blocks."""
    t, q = _u32(0), _u32(0)
    _check(lib().ntr_instanced_flags_read(_vp(d_flags), C.byref(t), C.byref(q), _vp(stream)))
    return int(t.value), int(q.value)


def trace_instanced_fast(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                         num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, d_flags, vis=None,
                         d_seed_results=0, seed_instance=-1, stream=0, timed=True):
    """ntr_trace_instanced_fast: trace_instanced_masked's records -- trace_instanced_seeded's when d_seed_results is given -- with the
    FAST slab test wherever the wave's rays and d_flags (instanced_validate's words, read by the launch) allow it; the rule is
    tests/np_instanced_fast.py.  timed=True returns the GPU seconds; timed=False is asynchronous on `stream` (capturable) and returns
    None."""
    return _trace_two_level("ntr_trace_instanced_fast", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes,
                            tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                            d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis, d_flags=d_flags)


def trace_instanced_fast_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records,
                               num_instances, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, d_flags,
                               vis=None, d_seed_results=0, seed_instance=-1, stream=0):
    """ntr_trace_instanced_fast_stats: trace_instanced_fast's records through the instrumented kernels ->
    (InstancedTraceStats, InstancedFastStats).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_fast_stats", (InstancedTraceStats, InstancedFastStats), num_rays, any_hit, d_rays, d_results,
                            d_instance_ids, d_tlas_nodes, tlas_nodes_bytes, root_link, d_records, num_instances, d_pool_nodes, pool_nodes_bytes,
                            d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis, d_flags=d_flags)


def trace_instanced_wide_seeded(num_rays, any_hit, d_rays, d_seed_results, seed_instance, d_results, d_instance_ids, d_wide_tlas_nodes,
                                wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes,
                                d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, stream=0, timed=True):
    """ntr_trace_instanced_wide_seeded: trace_instanced_seeded over 4-wide trees (the rule is tests/np_instanced_seeded.py, trace_wide).
    timed=True returns the GPU seconds; timed=False is asynchronous on `stream` (capturable) and returns None."""
    return _trace_two_level("ntr_trace_instanced_wide_seeded", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes,
                            wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop,
                            pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis)


def trace_instanced_wide_seeded_stats(num_rays, any_hit, d_rays, d_seed_results, seed_instance, d_results, d_instance_ids, d_wide_tlas_nodes,
                                      wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes,
                                      wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, vis=None, stream=0):
    """ntr_trace_instanced_wide_seeded_stats: trace_instanced_wide_seeded's records through the instrumented kernel ->
    InstancedWideTraceStats.  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_wide_seeded_stats", (InstancedWideTraceStats,), num_rays, any_hit, d_rays, d_results, d_instance_ids,
                            d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes,
                            wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance),
                            vis=vis)


def instanced_wide_validate(d_wide_tlas_nodes, wide_tlas_nodes_bytes, d_wide_pool_nodes, wide_pool_nodes_bytes, d_flags, stream=0):
    """ntr_instanced_wide_validate: the withheld validate bits of the wide top-level tree and of the wide pool into d_flags[0] and
    d_flags[1] (four words, 16-byte aligned; the rule is tests/np_instanced_wide_fast.py, validate).  Asynchronous on `stream` and
    capturable; to be run again after every call that rewrites a wide box, before the next trace_instanced_wide_fast.
    instanced_flags_read reads these words too."""
    _check(lib().ntr_instanced_wide_validate(_vp(d_wide_tlas_nodes), int(wide_tlas_nodes_bytes), _vp(d_wide_pool_nodes),
                                             int(wide_pool_nodes_bytes), _vp(d_flags), _vp(stream)))


def trace_instanced_wide_fast(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                              d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                              d_pool_tri_index, d_flags, vis=None, d_seed_results=0, seed_instance=-1, stream=0, timed=True):
    """ntr_trace_instanced_wide_fast: trace_instanced_wide's records with `vis` -- trace_instanced_wide_seeded's when d_seed_results is
    given -- with the FAST slab test wherever the wave's rays and d_flags (instanced_wide_validate's words, read by the launch) allow it;
    the rule is tests/np_instanced_wide_fast.py.  timed=True returns the GPU seconds; timed=False is asynchronous on `stream`
    (capturable) and returns None."""
    return _trace_two_level("ntr_trace_instanced_wide_fast", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes,
                            wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop,
                            pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance), vis=vis, d_flags=d_flags)


def trace_instanced_wide_fast_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                                    d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                                    d_pool_tri_index, d_flags, vis=None, d_seed_results=0, seed_instance=-1, stream=0):
    """ntr_trace_instanced_wide_fast_stats: trace_instanced_wide_fast's records through the instrumented kernels ->
    (InstancedWideTraceStats, InstancedFastStats).  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_wide_fast_stats", (InstancedWideTraceStats, InstancedFastStats), num_rays, any_hit, d_rays, d_results,
                            d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes,
                            wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, seed=(d_seed_results, seed_instance),
                            vis=vis, d_flags=d_flags)


def _wide_refit_entries(entries):
    """A ctypes array of WideRefitEntry from WideRefitEntry objects or (wideNodesOffset, wideNodesBytes, triWoopOffset, triWoopBytes,
    firstTri, numTris[, epsilon]) tuples."""
    if isinstance(entries, C.Array):
        return entries
    items = [e if isinstance(e, WideRefitEntry) else WideRefitEntry(*e) for e in entries]
    return (WideRefitEntry * max(len(items), 1))(*items)


def pool_wide_refit(entries, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_idx, num_tris_total, d_tri,
                    num_verts, d_pos, rewrite_rows=True, d_blas_boxes=0, stream=0, blocking=True):
    """ntr_pool_wide_refit: refit the listed wide BLASes of a wide pool (WideRefitEntry objects or (wideNodesOffset, wideNodesBytes,
    triWoopOffset, triWoopBytes, firstTri, numTris[, epsilon]) tuples) in place to the vertex positions at d_pos, keeping their topology
    (an extension; the rule is tests/np_wide_refit.py).  rewrite_rows=True also rewrites the leaves' Woop rows, as bvh_refit_batch does;
    False only reads them (after a bvh_refit_batch over the same selection).  blocking=True returns a WideRefitResult; blocking=False
    passes result = NULL: asynchronous on `stream` (capturable) and returns None.  An NtrError for a malformed tree (NTR_ERR_LAYOUT, after
    the work) carries .result, filled: firstBadEntry, errBits and the counts."""
    n = len(entries)
    arr = _wide_refit_entries(entries)
    res = WideRefitResult() if blocking else None
    try:
        _check(lib().ntr_pool_wide_refit(n, C.cast(arr, _vp), _vp(d_wide_pool_nodes), int(wide_pool_nodes_bytes), _vp(d_pool_woop),
                                         int(pool_woop_bytes), _vp(d_pool_idx), int(num_tris_total), _vp(d_tri), int(num_verts), _vp(d_pos),
                                         int(rewrite_rows), _vp(d_blas_boxes), C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def pool_wide_refit_scratch_bytes():
    """ntr_pool_wide_refit_scratch_bytes: bytes the wide pool refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_pool_wide_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_wide_refit(num_instances, d_instances, ranges, wide_ranges, d_wide_pool_nodes, wide_pool_nodes_bytes, d_wide_tlas_nodes,
                    wide_tlas_nodes_bytes, root_link, d_wide_records, records_cap, d_scene_box=0, stream=0, blocking=True):
    """ntr_tlas_wide_refit: keep a wide top-level tree's topology and rewrite its wide records and every box from the current instances
    and the current roots of the wide pool's BLASes (an extension; the rule is tests/np_wide_refit.py).  ranges as for tlas_build,
    wide_ranges as pool_widen returned them.  blocking=True returns a TlasRefitResult; blocking=False passes result = NULL: asynchronous
    on `stream` (capturable) and returns None.  An NtrError raised after the device work (a bad blas index, a malformed tree) carries
    .result, filled: errBits and the counts."""
    arr, n = _blas_ranges(ranges)
    warr = _wide_ranges(wide_ranges)
    res = TlasRefitResult() if blocking else None
    try:
        _check(lib().ntr_tlas_wide_refit(int(num_instances), _vp(d_instances), n, C.cast(arr, _vp), C.cast(warr, _vp), _vp(d_wide_pool_nodes),
                                         int(wide_pool_nodes_bytes), _vp(d_wide_tlas_nodes), int(wide_tlas_nodes_bytes), int(root_link),
                                         _vp(d_wide_records), int(records_cap), _vp(d_scene_box), C.byref(res) if blocking else None,
                                         _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def tlas_wide_refit_scratch_bytes():
    """ntr_tlas_wide_refit_scratch_bytes: bytes the wide top-level refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_wide_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def tlas_wide_motion_refit(num_instances, d_instances0, d_instances1, ranges, wide_ranges, d_wide_pool_nodes, wide_pool_nodes_bytes,
                           d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, records_cap, d_motion_keys, motion_keys_cap,
                           d_scene_box=0, stream=0, blocking=True):
    """ntr_tlas_wide_motion_refit: tlas_wide_refit over two keys of the instances (shutter open, shutter close): swept leaf boxes from
    the wide roots, word 15 of a moving instance's wide record, and the motion key buffer (128 bytes per instance, tlas_motion_refit's
    bytes) that trace_instanced_wide_motion reads; the rule is tests/np_instanced_wide_motion.py.  blocking=True returns a
    TlasMotionRefitResult; blocking=False passes result = NULL: asynchronous on `stream` (capturable) and returns None.  An NtrError
    raised after the device work carries .result, filled."""
    arr, n = _blas_ranges(ranges)
    warr = _wide_ranges(wide_ranges)
    res = TlasMotionRefitResult() if blocking else None
    try:
        _check(lib().ntr_tlas_wide_motion_refit(int(num_instances), _vp(d_instances0), _vp(d_instances1), n, C.cast(arr, _vp),
                                                C.cast(warr, _vp), _vp(d_wide_pool_nodes), int(wide_pool_nodes_bytes),
                                                _vp(d_wide_tlas_nodes), int(wide_tlas_nodes_bytes), int(root_link), _vp(d_wide_records),
                                                int(records_cap), _vp(d_motion_keys), int(motion_keys_cap), _vp(d_scene_box),
                                                C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def tlas_wide_motion_refit_scratch_bytes():
    """ntr_tlas_wide_motion_refit_scratch_bytes: bytes the wide motion refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_tlas_wide_motion_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def trace_instanced_wide_motion(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                                d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                                d_pool_tri_index, vis=None, motion=None, stream=0, timed=True):
    """ntr_trace_instanced_wide_motion: trace_instanced_wide with time-sampled instance transforms (the rule is
    tests/np_instanced_wide_motion.py).  motion: an InstanceMotion over what tlas_wide_motion_refit wrote, or None (NULL:
    trace_instanced_wide).  timed=False is asynchronous on `stream` (capturable; times, keys and records are read at replay time) and
    returns None."""
    return _trace_two_level("ntr_trace_instanced_wide_motion", bool(timed), num_rays, any_hit, d_rays, d_results, d_instance_ids,
                            d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances, d_wide_pool_nodes,
                            wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, vis=vis, motion=motion)


def trace_instanced_wide_motion_stats(num_rays, any_hit, d_rays, d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link,
                                      d_wide_records, num_instances, d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes,
                                      d_pool_tri_index, vis=None, motion=None, stream=0):
    """ntr_trace_instanced_wide_motion_stats: trace_instanced_wide_motion's records through the instrumented kernel ->
    (InstancedWideTraceStats, InstancedMotionStats); the latter's algorithmic_bytes(stats, ...) is then the wide formula plus the poses
    and the times.  Blocks; refused on a capturing stream."""
    return _trace_two_level("ntr_trace_instanced_wide_motion_stats", (InstancedWideTraceStats, InstancedMotionStats), num_rays, any_hit, d_rays,
                            d_results, d_instance_ids, d_wide_tlas_nodes, wide_tlas_nodes_bytes, root_link, d_wide_records, num_instances,
                            d_wide_pool_nodes, wide_pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_tri_index, stream, vis=vis,
                            motion=motion)


def bvh_refit(d_nodes, nodes_bytes, d_woop, woop_bytes, d_idx, idx_bytes, num_tris, d_tri, num_verts, d_pos, epsilon=0.0, d_scene_box=0,
              stream=0, blocking=True):
    """ntr_bvh_refit: recompute a Compact tree's boxes and Woop rows in place from the vertex positions at d_pos (an extension; the
    rule is tests/np_bvh_refit.py).  blocking=True returns a BvhRefitResult (counts, GPU seconds); blocking=False passes result = NULL:
    the call is asynchronous on `stream` (capturable) and returns None."""
    res = BvhRefitResult() if blocking else None
    _check(lib().ntr_bvh_refit(_vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_idx), int(idx_bytes), int(num_tris),
                               _vp(d_tri), int(num_verts), _vp(d_pos), float(epsilon), _vp(d_scene_box),
                               C.byref(res) if blocking else None, _vp(stream)))
    return res


def bvh_refit_scratch_bytes():
    """ntr_bvh_refit_scratch_bytes: bytes the refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_motion_refit(d_nodes0, nodes_bytes, d_nodes1, d_woop, woop_bytes, d_idx, idx_bytes, d_vert_rows0, d_vert_rows1, num_tris, d_tri,
                     num_verts, d_pos0, d_pos1, epsilon=0.0, d_scene_box=0, stream=0, blocking=True):
    """ntr_bvh_motion_refit: refit a Compact tree to two vertex arrays for deformation motion blur (an extension; the rule is
    tests/np_bvh_motion.py): d_nodes0 and d_woop in place as bvh_refit(d_pos0), d_nodes1 the key-1 boxes, d_vert_rows0 / 1 (woop_bytes
    each) the triangles' vertices under either key.  blocking=True returns a BvhRefitResult; blocking=False passes result = NULL: the
    call is asynchronous on `stream` (capturable) and returns None."""
    res = BvhRefitResult() if blocking else None
    _check(lib().ntr_bvh_motion_refit(_vp(d_nodes0), int(nodes_bytes), _vp(d_nodes1), _vp(d_woop), int(woop_bytes), _vp(d_idx), int(idx_bytes),
                                      _vp(d_vert_rows0), _vp(d_vert_rows1), int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos0),
                                      _vp(d_pos1), float(epsilon), _vp(d_scene_box), C.byref(res) if blocking else None, _vp(stream)))
    return res


def bvh_motion_refit_scratch_bytes():
    """ntr_bvh_motion_refit_scratch_bytes: bytes the motion refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_motion_refit_scratch_bytes(C.byref(v)))
    return int(v.value)


def trace_bvh_motion(num_rays, any_hit, d_rays, d_results, d_nodes0, nodes_bytes, vert_rows_bytes, d_tri_index, motion, stream=0, timed=True):
    """ntr_trace_bvh_motion: closest or any hit through a tree that bvh_motion_refit prepared, every ray at its own time (the rule is
    tests/np_bvh_motion.py).  motion: a BvhMotion, or None (NULL: refused).  timed=True returns the GPU seconds; timed=False is
    asynchronous on `stream` (capturable) and returns None."""
    sec = C.c_float(0.0)
    _check(lib().ntr_trace_bvh_motion(int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results), _vp(d_nodes0), int(nodes_bytes),
                                      int(vert_rows_bytes), _vp(d_tri_index), C.byref(motion) if motion is not None else None, _vp(stream),
                                      C.byref(sec) if timed else None))
    return float(sec.value) if timed else None


def trace_bvh_motion_stats(num_rays, any_hit, d_rays, d_results, d_nodes0, nodes_bytes, vert_rows_bytes, d_tri_index, motion, stream=0):
    """ntr_trace_bvh_motion_stats: trace_bvh_motion's records through the instrumented kernel -> TraceStats.  Blocks."""
    st = TraceStats()
    _check(lib().ntr_trace_bvh_motion_stats(int(num_rays), int(bool(any_hit)), _vp(d_rays), _vp(d_results), _vp(d_nodes0), int(nodes_bytes),
                                            int(vert_rows_bytes), _vp(d_tri_index), C.byref(motion) if motion is not None else None,
                                            _vp(stream), C.byref(st)))
    return st


def _refit_entries(entries):
    """A ctypes array of RefitBatchEntry from RefitBatchEntry objects or (range, firstTri, numTris[, epsilon]) tuples."""
    if isinstance(entries, C.Array):
        return entries
    items = [e if isinstance(e, RefitBatchEntry) else RefitBatchEntry(*e) for e in entries]
    return (RefitBatchEntry * max(len(items), 1))(*items)


def bvh_refit_batch(entries, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, d_pool_idx, num_tris_total, d_tri, num_verts,
                    d_pos, d_blas_boxes=0, stream=0, blocking=True):
    """ntr_bvh_refit_batch: refit the listed BLASes of a pool (RefitBatchEntry objects or (range, firstTri, numTris[, epsilon]) tuples) to
    the vertex positions at d_pos in one pass; every BLAS comes out byte for byte as bvh_refit at pool + offset leaves it (the rule is
    tests/np_refit_batch.py).  blocking=True returns a BvhRefitBatchResult; blocking=False passes result = NULL: asynchronous on `stream`
    and returns None.  An NtrError for a malformed tree (NTR_ERR_LAYOUT, after the work) carries .result, filled: firstBadEntry, errBits
    and the counts."""
    n = len(entries)
    arr = _refit_entries(entries)
    res = BvhRefitBatchResult() if blocking else None
    try:
        _check(lib().ntr_bvh_refit_batch(n, C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_pool_woop), int(pool_woop_bytes),
                                         _vp(d_pool_idx), int(num_tris_total), _vp(d_tri), int(num_verts), _vp(d_pos), _vp(d_blas_boxes),
                                         C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def bvh_refit_batch_scratch_bytes():
    """ntr_bvh_refit_batch_scratch_bytes: bytes the batch refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_refit_batch_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_motion_refit_batch(entries, d_pool_nodes0, pool_nodes_bytes, d_pool_nodes1, d_pool_woop, pool_woop_bytes, d_pool_idx, d_pool_vert_rows0,
                           d_pool_vert_rows1, num_tris_total, d_tri, num_verts, d_pos0, d_pos1, d_blas_boxes=0, stream=0, blocking=True):
    """ntr_bvh_motion_refit_batch: refit the listed BLASes of a pool (entries as for bvh_refit_batch) to the two vertex arrays d_pos0 and
    d_pos1 in one pass; every BLAS's slices of the five pool buffers come out byte for byte as bvh_motion_refit at pool + offset leaves
    them (the rule is tests/np_motion_refit_batch.py).  blocking=True returns a BvhRefitBatchResult; blocking=False passes result = NULL:
    asynchronous on `stream` (capturable) and returns None.  An NtrError for a malformed tree (NTR_ERR_LAYOUT, after the work) carries
    .result, filled: firstBadEntry, errBits and the counts."""
    n = len(entries)
    arr = _refit_entries(entries)
    res = BvhRefitBatchResult() if blocking else None
    try:
        _check(lib().ntr_bvh_motion_refit_batch(n, C.cast(arr, _vp), _vp(d_pool_nodes0), int(pool_nodes_bytes), _vp(d_pool_nodes1),
                                                _vp(d_pool_woop), int(pool_woop_bytes), _vp(d_pool_idx), _vp(d_pool_vert_rows0),
                                                _vp(d_pool_vert_rows1), int(num_tris_total), _vp(d_tri), int(num_verts), _vp(d_pos0),
                                                _vp(d_pos1), _vp(d_blas_boxes), C.byref(res) if blocking else None, _vp(stream)))
    except NtrError as e:
        e.result = res
        raise
    return res


def bvh_motion_refit_batch_scratch_bytes():
    """ntr_bvh_motion_refit_batch_scratch_bytes: bytes the batched motion refit's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_motion_refit_batch_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_optimize(d_nodes, nodes_bytes, passes=1, stream=0):
    """ntr_bvh_optimize: restructure a Compact tree's treelets in place (an extension; the rule is tests/np_bvh_optimize.py).  Blocks;
    returns a BvhOptimizeResult (per pass: treelets formed and rewritten, height before and after; GPU seconds)."""
    res = BvhOptimizeResult()
    _check(lib().ntr_bvh_optimize(_vp(d_nodes), int(nodes_bytes), int(passes), C.byref(res), _vp(stream)))
    return res


def bvh_optimize_scratch_bytes():
    """ntr_bvh_optimize_scratch_bytes: bytes the scratch pool of bvh_optimize / bvh_sah_cost holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_optimize_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_reorder(d_nodes, nodes_bytes, d_woop, woop_bytes, d_idx, idx_bytes, d_out_nodes, out_nodes_capacity, d_out_woop, out_woop_capacity,
                d_out_idx, out_idx_capacity, stream=0, result=None):
    """ntr_bvh_reorder: copy a Compact tree into the host builder's node and row order (an extension; the rule is
    tests/np_bvh_reorder.py).  Out of place; blocks; returns a BvhReorderResult (the output's extents, counts, GPU seconds).  Pass a
    BvhReorderResult as `result` to keep the counts of a call that raises NTR_ERR_OVERFLOW or NTR_ERR_LAYOUT."""
    res = BvhReorderResult() if result is None else result
    _check(lib().ntr_bvh_reorder(_vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_idx), int(idx_bytes), _vp(d_out_nodes),
                                 int(out_nodes_capacity), _vp(d_out_woop), int(out_woop_capacity), _vp(d_out_idx), int(out_idx_capacity),
                                 C.byref(res), _vp(stream)))
    return res


def bvh_reorder_scratch_bytes():
    """ntr_bvh_reorder_scratch_bytes: bytes the reorder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_reorder_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_sah_cost(d_nodes, nodes_bytes, d_woop, woop_bytes, stream=0):
    """ntr_bvh_sah_cost: the reference's calcSAHGPU in strict binary32 (spec: tests/np_bvh_optimize.py sah_cost).  Blocks; returns a
    BvhSahResult (sahCost, reached slots, leaves, triangles, height, GPU seconds)."""
    res = BvhSahResult()
    _check(lib().ntr_bvh_sah_cost(_vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), C.byref(res), _vp(stream)))
    return res


def bvh_optimize_batch(entries, d_pool_nodes, pool_nodes_bytes, passes=2, stream=0, entry_results=True):
    """ntr_bvh_optimize_batch: bvh_optimize over the listed BLASes of a pool in one pass (an extension; the rule is
    tests/np_optimize_batch.py).  entries: (nodesOffset, nodesBytes[, triWoopOffset, triWoopBytes]) tuples or a BlasPool -- only the
    node part is read.  Blocks; returns (BvhOptimizeBatchResult, [BvhOptimizeBatchEntry] or None).  An NtrError raised after the work
    (NTR_ERR_LAYOUT) carries .result and .entry_results, filled."""
    arr, n = _blas_ranges(entries)
    res = BvhOptimizeBatchResult()
    per = (BvhOptimizeBatchEntry * max(n, 1))() if entry_results else None
    try:
        _check(lib().ntr_bvh_optimize_batch(n, C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes), int(passes),
                                            C.cast(per, _vp) if entry_results else None, C.byref(res), _vp(stream)))
    except NtrError as e:
        e.result = res
        e.entry_results = list(per[:n]) if entry_results else None
        raise
    return res, (list(per[:n]) if entry_results else None)


def bvh_optimize_batch_scratch_bytes():
    """ntr_bvh_optimize_batch_scratch_bytes: bytes the scratch pool of bvh_optimize_batch / bvh_sah_cost_batch holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_bvh_optimize_batch_scratch_bytes(C.byref(v)))
    return int(v.value)


def bvh_sah_cost_batch(entries, d_pool_nodes, pool_nodes_bytes, d_pool_woop, pool_woop_bytes, stream=0):
    """ntr_bvh_sah_cost_batch: bvh_sah_cost of the listed BLASes of a pool in two launches (spec: tests/np_optimize_batch.py sah_costs).
    Blocks; returns ([BvhSahResult], BvhSahBatchResult).  An NtrError raised after the work carries .result and .entry_results."""
    arr, n = _blas_ranges(entries)
    res = BvhSahBatchResult()
    per = (BvhSahResult * max(n, 1))()
    try:
        _check(lib().ntr_bvh_sah_cost_batch(n, C.cast(arr, _vp), _vp(d_pool_nodes), int(pool_nodes_bytes), _vp(d_pool_woop),
                                            int(pool_woop_bytes), C.cast(per, _vp), C.byref(res), _vp(stream)))
    except NtrError as e:
        e.result = res
        e.entry_results = list(per[:n])
        raise
    return list(per[:n]), res


def camera_decode(signature):
    out = (C.c_float * 16)()
    _check(lib().ntr_camera_decode(signature.encode(), out))
    v = list(out)
    return dict(position=v[0:3], forward=v[3:6], up=v[6:9], speed=v[9], fov=v[10], near=v[11], far=v[12], keep_aligned=bool(v[13]))


def camera_reencode(signature):
    buf = C.create_string_buffer(256)
    _check(lib().ntr_camera_reencode(signature.encode(), buf, 256))
    return buf.value.decode()


def camera_nscreen_to_world(signature, w, h):
    m, p, f = (C.c_float * 16)(), (C.c_float * 3)(), C.c_float(0)
    _check(lib().ntr_camera_nscreen_to_world(signature.encode(), int(w), int(h), m, p, C.byref(f)))
    return np.array(list(m), dtype=np.float32).reshape(4, 4), np.array(list(p), dtype=np.float32), float(f.value)


def obj_load(path):
    """Returns (tri[int32 n,3], pos[float32 m,3], numSubmeshes) with the reference's numbering."""
    h, nt_, nv, ns = _vp(), _i32(0), _i32(0), _i32(0)
    _check(lib().ntr_obj_load(path.encode(), C.byref(h), C.byref(nt_), C.byref(nv), C.byref(ns)))
    try:
        tri = np.zeros((nt_.value, 3), dtype=np.int32)
        pos = np.zeros((nv.value, 3), dtype=np.float32)
        _check(lib().ntr_obj_get(h, tri.ctypes.data_as(_vp), pos.ctypes.data_as(_vp)))
    finally:
        lib().ntr_obj_free(h)
    return tri, pos, int(ns.value)


class BvhView:
    """Device-side Compact BVH as raw pointers + extents (what CudaBVHTracer::traceBatch passes)."""

    def __init__(self, d_nodes, nodes_bytes, d_woop, woop_bytes, d_tri_index, flags=0, layout=4):
        self.d_nodes, self.nodes_bytes = int(d_nodes), int(nodes_bytes)
        self.d_woop, self.woop_bytes = int(d_woop), int(woop_bytes)
        self.d_tri_index, self.flags, self.layout = int(d_tri_index), int(flags), int(layout)

    def validate(self, stream=0):
        self.flags = bvh_validate(self.d_nodes, self.nodes_bytes, stream)
        return self.flags

    def trace(self, kernel, num_rays, any_hit, d_rays, d_results, stream=0, timed=True, flags=None, hint=None):
        return trace_bvh(kernel, num_rays, any_hit, d_rays, d_results, self.d_nodes, self.nodes_bytes, self.d_woop,
                         self.woop_bytes, self.d_tri_index, self.layout, self.flags if flags is None else flags,
                         stream, timed, hint)

    def trace_stats(self, kernel, num_rays, any_hit, d_rays, d_results, stream=0):
        return trace_bvh_stats(kernel, num_rays, any_hit, d_rays, d_results, self.d_nodes, self.nodes_bytes,
                               self.d_woop, self.woop_bytes, self.d_tri_index, self.layout, self.flags, stream)


class HostBvh:
    """Host Compact BVH (numpy copies of nodes / triWoop / triIndex) from ntr_sah_build."""

    def __init__(self, nodes, woop, tri_index, info=None):
        self.nodes = nodes          # uint8[nodesBytes]
        self.woop = woop            # uint8[woopBytes]
        self.tri_index = tri_index  # int32[]
        self.info = info or {}
        self.layout = 4
        self._h = None

    def host_trace(self, rays, any_hit=False, num_visibility=0, want_stats=False):
        """CudaAS::trace (the reference's host tracer, ntr_host_bvh_trace) on numpy rays; needs sah_build(keep_handle=True).
        Returns (results, visibility or None, TraceStats or None)."""
        if self._h is None:
            raise NtrError(-1, "host_trace needs sah_build(..., keep_handle=True)")
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        res = np.zeros(n, dtype=RESULT_DTYPE)
        vis = np.zeros(num_visibility, dtype=np.int32) if num_visibility else None
        st = TraceStats() if want_stats else None
        _check(lib().ntr_host_bvh_trace(self._h, n, int(bool(any_hit)), rays.ctypes.data_as(_vp), res.ctypes.data_as(_vp),
                                        vis.ctypes.data_as(_vp) if vis is not None else None, int(num_visibility),
                                        C.byref(st) if st is not None else None))
        return res, vis, st

    def close(self):
        if self._h is not None:
            lib().ntr_host_bvh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_bvh_wrap(nodes, woop, tri_index):
    """HostBvh (with a live handle, for host_trace) over copies of existing Compact buffers."""
    nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    woop = np.ascontiguousarray(woop).view(np.uint8).reshape(-1)
    tri_index = np.ascontiguousarray(tri_index, dtype=np.int32).reshape(-1)
    h = _vp()
    _check(lib().ntr_host_bvh_wrap(nodes.ctypes.data_as(_vp), nodes.nbytes, woop.ctypes.data_as(_vp), woop.nbytes,
                                   tri_index.ctypes.data_as(_vp), tri_index.nbytes, C.byref(h)))
    out = HostBvh(nodes.copy(), woop.copy(), tri_index.copy())
    out._h = h
    return out


def sah_build(tri_vtx_index, vtx_pos, min_leaf=1, max_leaf=1, keep_handle=False):
    tri = np.ascontiguousarray(tri_vtx_index, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(vtx_pos, dtype=np.float32).reshape(-1, 3)
    h = _vp()
    _check(lib().ntr_sah_build(tri.shape[0], tri.ctypes.data_as(_vp), pos.shape[0], pos.ctypes.data_as(_vp),
                               int(min_leaf), int(max_leaf), C.byref(h)))
    try:
        info = _HostBvhInfo()
        _check(lib().ntr_host_bvh_info(h, C.byref(info)))
        nodes = np.ctypeslib.as_array(C.cast(info.nodes, C.POINTER(C.c_uint8)), (info.nodesBytes,)).copy()
        woop = np.ctypeslib.as_array(C.cast(info.triWoop, C.POINTER(C.c_uint8)), (info.triWoopBytes,)).copy()
        tidx = np.ctypeslib.as_array(C.cast(info.triIndex, C.POINTER(C.c_int32)), (info.triIndexBytes // 4,)).copy()
        meta = dict(numInnerNodes=info.numInnerNodes, numLeafNodes=info.numLeafNodes, maxDepth=info.maxDepth,
                    buildSeconds=float(info.buildSeconds))
    except Exception:
        lib().ntr_host_bvh_free(h)
        raise
    out = HostBvh(nodes, woop, tidx, meta)
    if keep_handle:
        out._h = h
    else:
        lib().ntr_host_bvh_free(h)
    return out


# ---- kd-tree ------------------------------------------------------------------------------------------------------------
KDTREE_SPATIAL_MEDIAN, KDTREE_SAH = 0, 1
_KDTREE_BUILDERS = {"SpatialMedianKDTree": KDTREE_SPATIAL_MEDIAN, "SAHKDTree": KDTREE_SAH,
                    KDTREE_SPATIAL_MEDIAN: KDTREE_SPATIAL_MEDIAN, KDTREE_SAH: KDTREE_SAH}


def _f3(v):
    return (C.c_float * 3)(*[float(np.float32(x)) for x in v])


class HostKdtree:
    """Host kd-tree buffers (numpy copies of nodes / triWoop / triIndex, include/ntrace_amd.h) with the scene box, delta and
    the build's statistics (info)."""

    def __init__(self, nodes, woop, tri_index, scene_min, scene_max, delta, info=None):
        self.nodes = nodes            # int32[numInner, 4]: (left, right, floatBits(split), axis << 28)
        self.woop = woop              # uint8[triWoopBytes]
        self.tri_index = tri_index    # int32[]
        self.scene_min = scene_min    # float32[3]
        self.scene_max = scene_max
        self.delta = delta            # float32
        self.info = info or {}

    def trace(self, num_rays, any_hit, d_rays, d_results, d_nodes, d_woop, d_tri_index, stream=0, timed=True):
        """ntr_trace_kdtree over device copies of this tree's buffers."""
        return trace_kdtree(num_rays, any_hit, self.scene_min, self.scene_max, d_rays, d_results, d_nodes, self.nodes.nbytes,
                            d_woop, self.woop.nbytes, d_tri_index, self.tri_index.nbytes, stream, timed)


def _kdtree_from_handle(h):
    info = _HostKdtreeInfo()
    _check(lib().ntr_host_kdtree_info(h, C.byref(info)))
    nodes = np.ctypeslib.as_array(C.cast(info.nodes, C.POINTER(C.c_int32)), (info.nodesBytes // 4,)).copy().reshape(-1, 4)
    woop = np.ctypeslib.as_array(C.cast(info.triWoop, C.POINTER(C.c_uint8)), (info.triWoopBytes,)).copy()
    tidx = np.ctypeslib.as_array(C.cast(info.triIndex, C.POINTER(C.c_int32)), (info.triIndexBytes // 4,)).copy()
    meta = dict(numInnerNodes=info.numInnerNodes, numLeafNodes=info.numLeafNodes, numEmptyLeaves=info.numEmptyLeaves,
                numTriRefs=info.numTriRefs, maxDepth=info.maxDepth, percentDuplicates=float(info.percentDuplicates),
                buildSeconds=float(info.buildSeconds))
    return HostKdtree(nodes, woop, tidx, np.array(info.sceneMin[:], dtype=np.float32), np.array(info.sceneMax[:], dtype=np.float32),
                      np.float32(info.delta), meta)


def kdtree_build(tri_vtx_index, vtx_pos, builder="SAHKDTree", max_leaf=1):
    """ntr_kdtree_build: builder "SpatialMedianKDTree" / "SAHKDTree" (or NTR_KDTREE_* values) -> HostKdtree."""
    tri = np.ascontiguousarray(tri_vtx_index, dtype=np.int32).reshape(-1, 3)
    pos = np.ascontiguousarray(vtx_pos, dtype=np.float32).reshape(-1, 3)
    h = _vp()
    _check(lib().ntr_kdtree_build(_KDTREE_BUILDERS.get(builder, -1) if not isinstance(builder, int) else builder, tri.shape[0],
                                  tri.ctypes.data_as(_vp), pos.shape[0], pos.ctypes.data_as(_vp), int(max_leaf), C.byref(h)))
    try:
        return _kdtree_from_handle(h)
    finally:
        lib().ntr_host_kdtree_free(h)


def host_kdtree_wrap(nodes, woop, tri_index, scene_min, scene_max):
    """ntr_host_kdtree_wrap: validates buffers made elsewhere and returns them as a HostKdtree (NtrError on a bad tree)."""
    nodes = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
    woop = np.ascontiguousarray(woop).view(np.uint8).reshape(-1)
    tri_index = np.ascontiguousarray(tri_index, dtype=np.int32).reshape(-1)
    h = _vp()
    _check(lib().ntr_host_kdtree_wrap(nodes.ctypes.data_as(_vp), nodes.nbytes, woop.ctypes.data_as(_vp), woop.nbytes,
                                      tri_index.ctypes.data_as(_vp), tri_index.nbytes, _f3(scene_min), _f3(scene_max), C.byref(h)))
    try:
        return _kdtree_from_handle(h)
    finally:
        lib().ntr_host_kdtree_free(h)


def trace_kdtree(num_rays, any_hit, scene_min, scene_max, d_rays, d_results, d_nodes, nodes_bytes, d_woop, woop_bytes, d_tri_index,
                 tri_index_bytes, stream=0, timed=True):
    """ntr_trace_kdtree on raw device pointers (ints).  Returns GPU seconds if timed else None."""
    sec = C.c_float(0.0)
    _check(lib().ntr_trace_kdtree(int(num_rays), int(bool(any_hit)), _f3(scene_min), _f3(scene_max), _vp(d_rays), _vp(d_results),
                                  _vp(d_nodes), int(nodes_bytes), _vp(d_woop), int(woop_bytes), _vp(d_tri_index), int(tri_index_bytes),
                                  _vp(stream), C.byref(sec) if timed else None))
    return float(sec.value) if timed else None


# ---- on-device kd-tree build ----------------------------------------------------------------------------------------------
KDTREE_DEVICE_DEFAULTS = dict(triLimit=16, triMaxLimit=16, failureCount=0, depthK1=1.2, depthK2=2.0, ci=1.0, ct=1.0, failRq=0.9)


def kdtree_device_params(**kw):
    """NtrKdtreeDeviceParams: the config.conf defaults with the given fields replaced."""
    p = KdtreeDeviceParams()
    _check(lib().ntr_kdtree_device_params_default(C.byref(p)))
    for k, v in kw.items():
        if k not in KDTREE_DEVICE_DEFAULTS:
            raise TypeError("unknown kd-tree parameter %r" % k)
        setattr(p, k, v)
    return p


class DeviceKdtree:
    """A kd-tree built on the device (ntr_kdtree_device_build).  It owns its device buffers until close(); the info fields are
    attributes (nodes / triWoop / triIndex are device pointers, *Bytes their exact sizes)."""

    def __init__(self, handle):
        self._h = handle
        info = _DeviceKdtreeInfo()
        _check(lib().ntr_device_kdtree_info(handle, C.byref(info)))
        for name, _ in _DeviceKdtreeInfo._fields_:
            v = getattr(info, name)
            setattr(self, name, v[:] if name in ("sceneMin", "sceneMax") else v)
        self.scene_min = np.array(info.sceneMin[:], dtype=np.float32)
        self.scene_max = np.array(info.sceneMax[:], dtype=np.float32)
        self.delta = np.float32(info.delta)

    @property
    def info(self):
        return {name: getattr(self, name) for name, _ in _DeviceKdtreeInfo._fields_}

    def trace(self, num_rays, any_hit, d_rays, d_results, stream=0, timed=True):
        """ntr_trace_kdtree over this tree's buffers (the signature of HostKdtree.trace without the buffer pointers)."""
        if self._h is None:
            raise NtrError(-1, "DeviceKdtree: closed")
        return trace_kdtree(num_rays, any_hit, self.scene_min, self.scene_max, d_rays, d_results, self.nodes, self.nodesBytes,
                            self.triWoop, self.triWoopBytes, self.triIndex, self.triIndexBytes, stream, timed)

    def download(self):
        """(nodes int32[n, 4], woop uint8[], tri_index int32[]) copied to the host (ntr_device_kdtree_download)."""
        if self._h is None:
            raise NtrError(-1, "DeviceKdtree: closed")
        nodes = np.zeros(self.nodesBytes // 4, np.int32)
        woop = np.zeros(self.triWoopBytes, np.uint8)
        idx = np.zeros(self.triIndexBytes // 4, np.int32)
        _check(lib().ntr_device_kdtree_download(self._h, nodes.ctypes.data_as(_vp), woop.ctypes.data_as(_vp), idx.ctypes.data_as(_vp)))
        return nodes.reshape(-1, 4), woop, idx

    def close(self):
        if self._h is not None:
            lib().ntr_device_kdtree_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kdtree_device_scratch_bytes():
    """ntr_kdtree_device_scratch_bytes: bytes the device kd-tree builder's scratch pool holds on the current device."""
    v = _i64(0)
    _check(lib().ntr_kdtree_device_scratch_bytes(C.byref(v)))
    return int(v.value)


def kdtree_device_build(d_tri, num_tris, d_pos, num_verts, params=None, stream=0):
    """ntr_kdtree_device_build on raw device pointers (ints).  params: None (config.conf defaults), a dict of
    NtrKdtreeDeviceParams fields, or a KdtreeDeviceParams.  Returns a DeviceKdtree."""
    if isinstance(params, dict):
        params = kdtree_device_params(**params)
    h = _vp()
    _check(lib().ntr_kdtree_device_build(int(num_tris), _vp(d_tri), int(num_verts), _vp(d_pos),
                                         C.byref(params) if params is not None else None, C.byref(h), _vp(stream)))
    return DeviceKdtree(h)
