// trace_instanced_wide_body.h -- the two-level trace over 4-wide trees, its kernel stated once: trace_instanced_wide_kernels.hip (the
// three unseeded kernels) and trace_instanced_wide_seeded_kernels.hip (the seeded ones) include this text once each, and
// trace_instanced_wide_fast_kernels.hip (the FAST ones, unseeded and seeded) twice, and trace_instanced_wide_motion_kernels.hip (the two
// motion kernels) once, after trace_instanced_wide_kernels.h, with
//   NTR_TIW_TEMPLATE   the template header: <bool MASKED, bool STATS>, or <bool STATS> for the seeded kernels (MASKED is then true)
//   NTR_TIW_KERNEL     the kernel's name
//   NTR_TIW_PARAMS     its parameters: InstancedWideParams p, and for the seeded kernels InstancedWideSeed sd
//   NTR_TIW_SEEDED     1: the ray starts from a seed record (the rule is tests/np_instanced_seeded.py): tmax from a seed that is a hit,
//                      no traversal for an any-hit ray whose seed is a hit, and a lane that accepts nothing stores the seed's words
//   NTR_TIW_FAST       1: FAST slab arithmetic from device-resident flags (InstancedFast fl and level_nice of trace_instanced_nice.h;
//                      DESIGN.md 6x; the rule is tests/np_instanced_wide_fast.py): a per-lane `nice` says that the lane's current ray may
//                      take FAST on its current level, and the wave votes per iteration on the step's form.  The template header is
//                      <bool STATS>, seeded or not: the fast kernels are the masked loop
//   NTR_TIW_MOTION     1 (optional; undefined means 0): motion blur (InstancedMotion mo of trace_motion_pose.h; the rule is
//                      tests/np_instanced_wide_motion.py): the ray carries a time, and the entering step poses an instance whose record
//                      has word 15 set at that time -- trace_instanced_body.h's addition under NTR_TI_MOTION, in the same place.  The
//                      template header is <bool STATS>: the motion kernels are the masked loop
// An include and not a further template parameter for trace_instanced_body.h's reason: the unseeded kernels keep their names and stay,
// instruction for instruction, what they were (scripts/kernel_isa_diff.sh).  No include guard.
NTR_TIW_TEMPLATE
__global__ __launch_bounds__(64) void NTR_TIW_KERNEL(NTR_TIW_PARAMS)
{
#if NTR_TIW_SEEDED || NTR_TIW_FAST
    constexpr bool MASKED = true;   // the seeded kernels are the masked loop
#endif
#if NTR_TIW_MOTION
    constexpr bool MASKED = true;   // so are the motion kernels
#endif
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;
    const float4* rays4 = reinterpret_cast<const float4*>(p.rays);
    const u32x4 rTlas = rsrc_words(p.tlas, p.tlasBytes), rRec = rsrc_words(p.records, p.recordsBytes),
                rWide = rsrc_words(p.poolWide, p.poolWideBytes), rWoop = rsrc_words(p.poolWoop, p.poolWoopBytes);
    const bool anyHit = p.anyHit != 0;
    u32x4 rMasks = rTlas;
    unsigned int rayMask = 0xFFFFFFFFu;   // m_r
    bool instMasks = false;               // wave-uniform: without instance masks no entering step loads a word
    if (MASKED) {
        rMasks = rsrc_words(p.instMasks, p.instMasksBytes);
        instMasks = p.instMasks != nullptr;
        rayMask = p.rayMasks ? p.rayMasks[valid ? rayIdx : 0] : p.rayMask;
    }
    InstancedLaneStats ls = {0u, 0u, 0u, 0u, 0u, 0u};
#if NTR_TIW_MOTION
    // the ray's time, clamped so that a NaN gives 0; the key buffer's descriptor is built from kernel arguments only
    const Rsrc rKeys = make_rsrc(mo.keys, mo.keysBytes);
    float rayTime = mo.rayTimes ? mo.rayTimes[valid ? rayIdx : 0] : mo.time;
    rayTime = motion_clamp_time(rayTime);
    unsigned int movingEntries = 0u, singularSteps = 0u;   // (STATS only)
#endif

    RayRegs r;   // the current form: the world ray on the top level, the object ray inside an instance
    {
        const float4 o = rays4[(valid ? rayIdx : 0) * 2 + 0], d = rays4[(valid ? rayIdx : 0) * 2 + 1];
        r.ox = o.x; r.oy = o.y; r.oz = o.z; r.tmin = o.w;
        r.dx = d.x; r.dy = d.y; r.dz = d.z; r.tmax = d.w;
        r.rx = r.ry = r.rz = 0.0f;   // (the FAST path's reciprocals: unused)
    }
    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[0][lane];
    stack_reset(st);

    int hitAddr = -1, hitInst = -1;   // the hit's row in the pool's triWoop and its instance
    float hitU = 0.0f, hitV = 0.0f;
    int inst = -1;                    // >= 0: inside that instance
    unsigned int wideOffset = 0u, rowOffset = 0u, extent = 0u;
#if NTR_TIW_SEEDED
    // one coalesced 16-byte load beside the ray's: a seed that is a hit gives tmax.  Nothing of it is held through the loop: a lane that
    // accepts nothing reloads its record at the end, as the world ray is reloaded on leaving an instance
    const int4* seeds4 = reinterpret_cast<const int4*>(sd.seedResults);
    bool seedStops = false;
    {
        const int4 s4 = seeds4[valid ? rayIdx : 0];
        if (s4.x != -1) {
            r.tmax = __int_as_float(s4.y);
            seedStops = anyHit;   // an any-hit ray that the seed already occludes never starts
        }
    }
    // a degenerate ray (Ray::degenerate, Util.hpp:65) keeps its seed without traversal: the comparison is with the seeded tmax
    int node = (valid && !seedStops && r.tmin < r.tmax) ? p.rootLink : kSentinel;
#else
    // a degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal
    int node = (valid && r.tmin < r.tmax) ? p.rootLink : kSentinel;
#endif
#if NTR_TIW_FAST
    // the withheld bits of the two levels (ntr_instanced_wide_validate), read by the launch: a replay sees what the last validate wrote
    const unsigned int heldTlas = fl.flags[0], heldPool = fl.flags[1];
    // `nice`: of the lane's current ray on its current level; level_nice sets r.rx, r.ry, r.rz when it says yes.  The instrumented
    // variants hold it and niceStart as words pinned to vector registers (NiceWord): as lane masks in scalar pairs they are an SGPR
    // spill in the seeded one
    typedef NiceWord<STATS> NicePin;
    typename NicePin::type nice = level_nice(r, heldTlas);
    NicePin::pin(nice);
    typename NicePin::type niceStart = node != kSentinel && nice;
    NicePin::pin(niceStart);
    // (STATS only.  The wave's two counters are kept by lane 0, in vector registers, as in trace_instanced_body.h)
    const unsigned int laneZero = lane == 0 ? 1u : 0u;
    unsigned int waveSteps = 0u, fastSteps = 0u, niceEntries = 0u;
#endif

    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a, e = a, f = a, g = a;
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
#if NTR_TIW_FAST
        // the wave's vote, one ballot per iteration: FAST iff no live lane holds a ray that is not nice -- a scalar branch around the
        // two instantiations of the step
        const bool fastStep = __ballot(node != kSentinel && !nice) == 0ull;
        if (STATS) { waveSteps += laneZero; fastSteps += fastStep ? laneZero : 0u; }
#endif
        const bool top = inst < 0;
        const bool inner = (unsigned)node < (unsigned)kSentinel;
        const bool neg = node < 0;
        int ofs = kNoNode;
        if (top) {
            if (inner) ofs = node;
            else if (neg && (unsigned)~node < (unsigned)p.numInstances) ofs = ~node * kRecordBytes;
        } else if (inner) {
            // below the BLAS's extent only (node and extent are multiples of 128 in a well-formed tree: the whole node lies inside)
            const unsigned int o = wideOffset + (unsigned)node;
            if ((unsigned)node < extent && o >= wideOffset && o < (unsigned)kNoNode) ofs = (int)o;   // (a sum that wraps reads nothing)
        } else if (neg) {
            const unsigned int row = rowOffset + (unsigned)~node;
            if (row < (unsigned)(kPoolMaxBytes >> kRowShift)) ofs = (int)(row << kRowShift);
        }
        unsigned int instMask = 0xFFFFFFFFu;   // M_i of an entering lane
        {
            // the word of record ofs / 64 lies at ofs / 16; an entering lane whose index is out of range holds kNoNode, and kNoNode / 16 =
            // 0x0FFFFFF0 is at or beyond the end of any mask array (4 * numInstances <= kPoolMaxBytes / 16): it reads 0 and touches nothing
            const unsigned long long enter = __ballot(top && neg);
            fetch_two_level_wide(rTlas, rRec, rWide, rWoop, rMasks, ofs, (int)((unsigned)ofs >> 4), __ballot(top && inner), enter,
                                 __ballot(!top && inner), __ballot(!top && neg), (MASKED && instMasks) ? enter : 0ull, a, b, c, d, e, f, g,
                                 instMask);
        }
        if (node == kSentinel) {
            // done: waits for the wave
        } else if (!inner && !neg) {
            // a positive word above the sentinel: the exit marker.  Leaving: the world ray again (tmin and the shrunk tmax stay)
            if (node == kExitMarker) {
                const float4 o = rays4[rayIdx * 2 + 0], dd = rays4[rayIdx * 2 + 1];
                r.ox = o.x; r.oy = o.y; r.oz = o.z;
                r.dx = dd.x; r.dy = dd.y; r.dz = dd.z;
                inst = -1;
#if NTR_TIW_FAST
                nice = level_nice(r, heldTlas);
                NicePin::pin(nice);
#endif
            }
            node = stack_pop(st, spill);   // (any other such word is no link: it is dropped)
        } else if (inner) {
            // a wide node of either level (a lane whose fetch lay beyond an extent read zeros: four links of 0, no candidate, a pop)
            if (STATS) { if (top) ls.topInner++; else ls.inner++; }
#if NTR_TIW_FAST
            if (fastStep) wide_advance<true>(a, b, c, d, e, f, g, r, node, st, spill, p.status); else
#endif
            wide_advance<false>(a, b, c, d, e, f, g, r, node, st, spill, p.status);
        } else if (top) {
            // entering instance ~node: its record is worldToObject (a, b, c) and the wide offset, row offset and extent (d)
            const int idx = ~node;
            if ((unsigned)idx >= (unsigned)p.numInstances) {
                node = stack_pop(st, spill);
            } else if (MASKED && (instMask & rayMask) == 0u) {
                if (STATS) ls.masked++;
                node = stack_pop(st, spill);         // refused: no marker, no transform; the fetched record is dropped
            } else if (st.sp >= LDS_DEPTH + SPILL_DEPTH) {
                atomicOr(p.status, NTR_STATUS_STACK_OVERFLOW);   // no room for the marker: the instance is not entered
                node = stack_pop(st, spill);
            } else
#if NTR_TIW_MOTION
            // a record whose word 15 is set names a moving instance: worldToObject(t) replaces the record's rows a, b, c.  The wave
            // votes, so one that enters only static instances runs the masked kernel's step behind one scalar branch
            if (__ballot(__float_as_uint(d.w) != 0u) != 0ull && __float_as_uint(d.w) != 0u && !motion_pose(rKeys, idx, rayTime, a, b, c)) {
                if (STATS) singularSteps++;
                node = stack_pop(st, spill);         // no inverse at this time: no marker, no transform
            } else
#endif
            {
#if NTR_TIW_MOTION
                if (STATS) movingEntries += __float_as_uint(d.w) != 0u ? 1u : 0u;
#endif
                stack_push(st, spill, kExitMarker, p.status);
                const float ox = dot4(a, r.ox, r.oy, r.oz, 1.0f), oy = dot4(b, r.ox, r.oy, r.oz, 1.0f), oz = dot4(c, r.ox, r.oy, r.oz, 1.0f);
                const float dx = dot4(a, r.dx, r.dy, r.dz, 0.0f), dy = dot4(b, r.dx, r.dy, r.dz, 0.0f), dz = dot4(c, r.dx, r.dy, r.dz, 0.0f);
                r.ox = ox; r.oy = oy; r.oz = oz;
                r.dx = dx; r.dy = dy; r.dz = dz;
                wideOffset = __float_as_uint(d.x);
                rowOffset = __float_as_uint(d.y);
                extent = __float_as_uint(d.z);
                inst = idx;
                node = 0;
                if (STATS) ls.entries++;
#if NTR_TIW_FAST
                nice = level_nice(r, heldPool);
                NicePin::pin(nice);
                if (STATS) niceEntries += nice ? 1u : 0u;
#endif
            }
        } else {
            int row = -1;   // the BLAS's own row of a hit this step accepts
            if (STATS) {
                // leaf_step's counters: a triangle test unless the row is a terminator; a terminator read for the row itself or for the word
                // that came with a triangle -- unless an any-hit ray ended on that triangle
                const bool term = __float_as_uint(a.x) == kLeafTerm;
                if (!term) ls.tris++;
#if NTR_TIW_FAST
                if (fastStep) unified_advance<true, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status); else
#endif
                unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
                if (term || (!(anyHit && row >= 0) && __float_as_uint(d.x) == kLeafTerm)) ls.leaves++;
            } else {
#if NTR_TIW_FAST
                if (fastStep) unified_advance<true, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status); else
#endif
                unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
            }
            if (row >= 0) {
                hitAddr = (int)(rowOffset + (unsigned)row);
                hitInst = inst;
            }
        }
    }
    if (!valid) return;
#if NTR_TIW_SEEDED
    bool seedKept = false;   // the lane accepted nothing and its seed is a hit
    if (hitAddr < 0) {
        // the seed's four words verbatim, a miss's too (results may be the seed buffer: the lane reads its record before it writes it)
        const int4 s4 = seeds4[rayIdx];
        seedKept = s4.x != -1;
        reinterpret_cast<int4*>(p.results)[rayIdx] = s4;
        p.instanceIDs[rayIdx] = seedKept ? sd.seedInstance : -1;
    } else {
        store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
        p.instanceIDs[rayIdx] = hitInst;
    }
#else
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    p.instanceIDs[rayIdx] = hitInst;
#endif
    if (STATS) {   // diagnostics variant only: plain per-lane atomics
        atomicAdd(&p.stats[0], (unsigned long long)ls.topInner);
        atomicAdd(&p.stats[1], (unsigned long long)ls.entries);
        atomicAdd(&p.stats[2], (unsigned long long)ls.masked);
        atomicAdd(&p.stats[3], (unsigned long long)ls.inner);
        atomicAdd(&p.stats[4], (unsigned long long)ls.tris);
        atomicAdd(&p.stats[5], (unsigned long long)ls.leaves);
#if NTR_TIW_SEEDED
        atomicAdd(&p.stats[6], (unsigned long long)(seedKept || (hitAddr >= 0 && p.triIndex[hitAddr] != -1)));
#else
        atomicAdd(&p.stats[6], (unsigned long long)(hitAddr >= 0 && p.triIndex[hitAddr] != -1));
#endif
#if NTR_TIW_MOTION
        atomicAdd(&p.stats[12], (unsigned long long)movingEntries);
        atomicAdd(&p.stats[13], (unsigned long long)singularSteps);
#endif
#if NTR_TIW_FAST
        if (lane == 0) {   // (lane 0 of a launched wave is a ray)
            atomicAdd(&p.stats[8], (unsigned long long)waveSteps);
            atomicAdd(&p.stats[9], (unsigned long long)fastSteps);
        }
        atomicAdd(&p.stats[10], (unsigned long long)niceStart);
        atomicAdd(&p.stats[11], (unsigned long long)niceEntries);
#endif
    }
}
