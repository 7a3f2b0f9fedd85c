// trace_instanced_body.h -- the two-level trace's kernel, stated once: trace_instanced_kernels.hip (the unmasked kernel) and
// trace_instanced_masked_kernels.hip (the masked and the instrumented one) and trace_instanced_seeded_kernels.hip (the seeded masked
// and the seeded instrumented one, whose parameters add InstancedSeed sd) include this text once per variant, after
// trace_instanced_kernels.h, with
//   NTR_TI_KERNEL   the kernel's name
//   NTR_TI_PARAMS   its parameters: InstancedParams p, and for the masked variants InstancedExtras x
//   NTR_TI_MASKED   1: the entering step asks the masks (x.instMasks, x.rayMasks, x.rayMask)
//   NTR_TI_STATS    1: per-lane counters, summed into x.stats at the end
//   NTR_TI_SEEDED   1: the ray starts from a seed record (InstancedSeed sd; the rule is tests/np_instanced_seeded.py): tmax from a seed that
//                   is a hit, no traversal for an any-hit ray whose seed is a hit, and a lane that accepts nothing stores the seed's words
//   NTR_TI_FAST     1: FAST slab arithmetic from device-resident flags (InstancedFast f and level_nice of
//                   trace_instanced_nice.h; the rule is tests/np_instanced_fast.py): a per-lane `nice` says that
//                   the lane's current ray may take FAST on its current level, and the wave votes per iteration on the step's form
//   NTR_TI_MOTION   1 (optional; undefined means 0): motion blur (InstancedMotion mo; the rule is tests/np_instanced_motion.py):
//                   the ray carries a time, and the entering step poses an instance whose record has word 15 set at that time -- two
//                   keys from the motion key buffer, twelve lerps and the binary64 inverse, behind a wave-uniform branch
//   NTR_TI_DEFORM   1 (optional; undefined means 0; on top of NTR_TI_MASKED 1 and NTR_TI_MOTION 1): deforming BLASes (InstancedDeform df;
//                   DESIGN.md 6ag; the rule is tests/np_instanced_deform.py): bit 0 of record word 15 is "moving", bit 1 says that the
//                   instance's BLAS deforms.  A lane that enters remembers bit 1 until its exit marker; behind ONE wave-uniform branch on
//                   the ballot of such lanes a second fetch brings the second key's box rows, or the two keys' vertex rows, and the
//                   words are posed at the ray's time before the unchanged steps run.  A wave with no lane in a deforming BLAS runs
//                   the motion kernel's iteration after that one scalar branch
// An include and not a function template because the unmasked variant must stay the kernel it was, instruction for instruction
// (scripts/kernel_isa_diff.sh): with the loop in a __forceinline__ function that the kernels call, hipcc orders its passes differently and
// allocates other registers, and every such change would have to be measured again.  No include guard: the text is meant
// to repeat.
__global__ __launch_bounds__(64) void NTR_TI_KERNEL(NTR_TI_PARAMS)
{
    constexpr bool MASKED = NTR_TI_MASKED, STATS = NTR_TI_STATS;
#if !NTR_TI_MASKED
    const InstancedExtras x{};   // (never read: every use is under MASKED or STATS)
#endif
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;
    const float4* rays4 = reinterpret_cast<const float4*>(p.rays);
    const u32x4 rTlas = rsrc_words(p.tlas, p.tlasBytes), rRec = rsrc_words(p.records, p.recordsBytes),
                rNodes = rsrc_words(p.poolNodes, p.poolNodesBytes), rWoop = rsrc_words(p.poolWoop, p.poolWoopBytes);
    const bool anyHit = p.anyHit != 0;
    u32x4 rMasks = rTlas;
    unsigned int rayMask = 0xFFFFFFFFu;   // m_r
    bool instMasks = false;               // wave-uniform: without instance masks no entering step loads a word
    if (MASKED) {
        rMasks = rsrc_words(x.instMasks, x.instMasksBytes);
        instMasks = x.instMasks != nullptr;
        rayMask = x.rayMasks ? x.rayMasks[valid ? rayIdx : 0] : x.rayMask;
    }
    InstancedLaneStats ls = {0u, 0u, 0u, 0u, 0u, 0u};
#if NTR_TI_MOTION
    // the ray's time, clamped so that a NaN gives 0; the key buffer's descriptor is built from kernel arguments only
    const Rsrc rKeys = make_rsrc(mo.keys, mo.keysBytes);
    float rayTime = mo.rayTimes ? mo.rayTimes[valid ? rayIdx : 0] : mo.time;
    rayTime = motion_clamp_time(rayTime);
    unsigned int movingEntries = 0u, singularSteps = 0u;   // (STATS only)
#endif
#if NTR_TI_DEFORM
    // the second key's nodes and the two keys' vertex rows, with the extents of the pool's nodes and rows: range-checked descriptors
    // built from kernel arguments, so a bad link reads zeros and never faults
    const u32x4 rNodes1 = rsrc_words(df.nodes1, p.poolNodesBytes), rVerts0 = rsrc_words(df.verts0, p.poolWoopBytes),
                rVerts1 = rsrc_words(df.verts1, p.poolWoopBytes);
    const float rayTimeU = 1.0f - rayTime;
    bool deform = false;                  // inside an instance whose BLAS deforms: bit 1 of the entered record's word 15
    unsigned int deformEntries = 0u, deformInner = 0u, deformTris = 0u;   // (STATS only)
#define NTR_TI_MOVING(W) ((__float_as_uint(W) & 1u) != 0u)
#else
#define NTR_TI_MOVING(W) (__float_as_uint(W) != 0u)
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
    unsigned int nodesOffset = 0u, rowOffset = 0u;
#if NTR_TI_SEEDED
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
#if NTR_TI_FAST
    // the withheld bits of the two levels (ntr_instanced_validate), read by the launch: a replay sees what the last validate wrote
    const unsigned int heldTlas = f.flags[0], heldPool = f.flags[1];
    // `nice`: of the lane's current ray on its current level; level_nice sets r.rx, r.ry, r.rz when it says yes.  The instrumented
    // variants hold it and niceStart as words pinned to vector registers (NTR_TI_NICE_PIN): as lane masks in scalar pairs they are
    // SGPR spills in the seeded one
#if NTR_TI_STATS
    typedef unsigned int nice_t;
#define NTR_TI_NICE_PIN(V) keep(V)
#else
    typedef bool nice_t;
#define NTR_TI_NICE_PIN(V)
#endif
    nice_t nice = level_nice(r, heldTlas);
    NTR_TI_NICE_PIN(nice);
    nice_t niceStart = node != kSentinel && nice;
    NTR_TI_NICE_PIN(niceStart);
    // (STATS only.  The wave's two counters are kept by lane 0, in vector registers: as scalars they are six SGPR spills in the seeded
    // instrumented kernel)
    const unsigned int laneZero = lane == 0 ? 1u : 0u;
    unsigned int waveSteps = 0u, fastSteps = 0u, niceEntries = 0u;
#endif

    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a;
#if NTR_TI_DEFORM
    float4 e = a, f = a, g = a;           // the second key's rows of a lane in a deforming BLAS
    unsigned int nextW = 0u;              // ... and the w word of the vertex row behind its triangle
#endif
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
#if NTR_TI_FAST
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
            const unsigned int o = nodesOffset + (unsigned)node;
            if (o >= nodesOffset) ofs = (int)o;                       // (a sum that wraps reads nothing)
        } else if (neg) {
            const unsigned int row = rowOffset + (unsigned)~node;
            if (row < (unsigned)(kPoolMaxBytes >> kRowShift)) ofs = (int)(row << kRowShift);
        }
        unsigned int instMask = 0xFFFFFFFFu;   // M_i of an entering lane
        if (MASKED) {
            // the word of record ofs / 64 lies at ofs / 16; an entering lane whose index is out of range holds kNoNode, and kNoNode / 16 =
            // 0x0FFFFFF0 is at or beyond the end of any mask array (4 * numInstances <= kPoolMaxBytes / 16): it reads 0 and touches nothing
            const unsigned long long enter = __ballot(top && neg);
            fetch64_four_buffers_and_word(rTlas, rRec, rNodes, rWoop, rMasks, ofs, (int)((unsigned)ofs >> 4), __ballot(top && inner), enter,
                                          __ballot(!top && inner),
#if NTR_TI_DEFORM
                                          __ballot(!top && neg && !deform),   // (a deforming BLAS's Woop rows are key 0's: not read)
#else
                                          __ballot(!top && neg),
#endif
                                          instMasks ? enter : 0ull, a, b, c, d, instMask);
        } else {
            fetch64_four_buffers(rTlas, rRec, rNodes, rWoop, ofs, __ballot(top && inner), __ballot(top && neg), __ballot(!top && inner),
                                 __ballot(!top && neg), a, b, c, d);
        }
#if NTR_TI_DEFORM
        // the one wave-uniform branch: lanes inside a deforming BLAS (`deform` implies !top; the marker and the sentinel are neither
        // inner nor neg) fetch what the pose needs at the same offset, with one wait
        const unsigned long long deformN = __ballot(deform && inner), deformT = __ballot(deform && neg);
        const bool deformWave = (deformN | deformT) != 0ull;
        if (deformWave) fetch_deform_rows(rNodes1, rVerts0, rVerts1, ofs, deformN, deformT, a, b, c, e, f, g, nextW);
#endif
        if (node == kSentinel) {
            // done: waits for the wave
        } else if (!inner && !neg) {
            // a positive word above the sentinel: the exit marker.  Leaving: the world ray again (tmin and the shrunk tmax stay)
            if (node == kExitMarker) {
                const float4 o = rays4[rayIdx * 2 + 0], dd = rays4[rayIdx * 2 + 1];
                r.ox = o.x; r.oy = o.y; r.oz = o.z;
                r.dx = dd.x; r.dy = dd.y; r.dz = dd.z;
                inst = -1;
#if NTR_TI_DEFORM
                deform = false;
#endif
#if NTR_TI_FAST
                nice = level_nice(r, heldTlas);
                NTR_TI_NICE_PIN(nice);
#endif
            }
            node = stack_pop(st, spill);   // (any other such word is no link: it is dropped)
        } else if (top && inner) {
            if (STATS) ls.topInner++;
#if NTR_TI_FAST
            if (fastStep) inner_advance<true, 8>(a, b, c, d, r, node, st, spill, p.status); else
#endif
            inner_advance<false, 8>(a, b, c, d, r, node, st, spill, p.status);
        } else if (top) {
            // entering instance ~node: its record is worldToObject (a, b, c) and nodesOffset, row offset, nodesBytes (d)
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
#if NTR_TI_MOTION
            // a record whose word 15 is set names a moving instance: worldToObject(t) replaces the record's rows a, b, c.  The wave
            // votes, so one that enters only static instances runs the masked kernel's step behind one scalar branch
            if (__ballot(NTR_TI_MOVING(d.w)) != 0ull && NTR_TI_MOVING(d.w) && !motion_pose(rKeys, idx, rayTime, a, b, c)) {
                if (STATS) singularSteps++;
                node = stack_pop(st, spill);         // no inverse at this time: no marker, no transform
            } else
#endif
            {
#if NTR_TI_MOTION
                if (STATS) movingEntries += NTR_TI_MOVING(d.w) ? 1u : 0u;
#endif
#if NTR_TI_DEFORM
                deform = (__float_as_uint(d.w) & 2u) != 0u;
                if (STATS) deformEntries += deform ? 1u : 0u;
#endif
                stack_push(st, spill, kExitMarker, p.status);
                const float ox = dot4(a, r.ox, r.oy, r.oz, 1.0f), oy = dot4(b, r.ox, r.oy, r.oz, 1.0f), oz = dot4(c, r.ox, r.oy, r.oz, 1.0f);
                const float dx = dot4(a, r.dx, r.dy, r.dz, 0.0f), dy = dot4(b, r.dx, r.dy, r.dz, 0.0f), dz = dot4(c, r.dx, r.dy, r.dz, 0.0f);
                r.ox = ox; r.oy = oy; r.oz = oz;
                r.dx = dx; r.dy = dy; r.dz = dz;
                nodesOffset = __float_as_uint(d.x);
                rowOffset = __float_as_uint(d.y);
                inst = idx;
                node = 0;
                if (STATS) ls.entries++;
#if NTR_TI_FAST
                nice = level_nice(r, heldPool);
                NTR_TI_NICE_PIN(nice);
                if (STATS) niceEntries += nice ? 1u : 0u;
#endif
            }
        } else {
            int row = -1;   // the BLAS's own row of a hit this step accepts
#if NTR_TI_DEFORM
            // an inner lane of a deforming BLAS poses its twelve box words in place (the links are key 0's) and goes on with the others
            if (deformWave && deform && inner) {
                if (STATS) deformInner++;
                a = motion_deform_lerp4(a, e, rayTime, rayTimeU); b = motion_deform_lerp4(b, f, rayTime, rayTimeU);
                c = motion_deform_lerp4(c, g, rayTime, rayTimeU);
            }
            // a triangle lane of a deforming BLAS: the terminator is the W word of key 0's vertex row (a vertex x of -0.0f is the same
            // word as the terminator); otherwise nine posed words, their Woop rows and the unchanged triangle test
            if (deformWave && deform && neg) {
                bool leafDone = __float_as_uint(a.w) == kLeafTerm;
                if (!leafDone) {
                    if (STATS) { ls.tris++; deformTris++; }
                    float4 w0, w1, w2;
                    woop_rows_verts(motion_deform_lerp(a.x, e.x, rayTime, rayTimeU), motion_deform_lerp(a.y, e.y, rayTime, rayTimeU),
                                    motion_deform_lerp(a.z, e.z, rayTime, rayTimeU), motion_deform_lerp(b.x, f.x, rayTime, rayTimeU),
                                    motion_deform_lerp(b.y, f.y, rayTime, rayTimeU), motion_deform_lerp(b.z, f.z, rayTime, rayTimeU),
                                    motion_deform_lerp(c.x, g.x, rayTime, rayTimeU), motion_deform_lerp(c.y, g.y, rayTime, rayTimeU),
                                    motion_deform_lerp(c.z, g.z, rayTime, rayTimeU), w0, w1, w2);
                    bool terminated = false;
                    if (triangle_step(w0, w1, w2, r, hitU, hitV)) {
                        row = leaf_row(node);
                        terminated = anyHit;
                    }
                    if (terminated) node = kSentinel;
                    else if (nextW == kLeafTerm) leafDone = true;   // the terminator came with this triangle
                    else node -= kTriRows;
                }
                if (leafDone) {
                    if (STATS) ls.leaves++;
                    node = stack_pop(st, spill);
                }
            } else
#endif
            if (STATS) {
                // counted at the call site, from the row just fetched: a triangle test unless word 0 is the terminator; a terminator read for
                // the row itself or for the word that came with a triangle -- unless an any-hit ray ended on that triangle
                const bool term = __float_as_uint(a.x) == kLeafTerm;
                if (inner) ls.inner++;
                else if (!term) ls.tris++;
#if NTR_TI_FAST
                if (fastStep) unified_advance<true, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status); else
#endif
                unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
                if (!inner && (term || (!(anyHit && row >= 0) && __float_as_uint(d.x) == kLeafTerm))) ls.leaves++;
            } else {
#if NTR_TI_FAST
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
#if NTR_TI_SEEDED
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
        atomicAdd(&x.stats[0], (unsigned long long)ls.topInner);
        atomicAdd(&x.stats[1], (unsigned long long)ls.entries);
        atomicAdd(&x.stats[2], (unsigned long long)ls.masked);
        atomicAdd(&x.stats[3], (unsigned long long)ls.inner);
        atomicAdd(&x.stats[4], (unsigned long long)ls.tris);
        atomicAdd(&x.stats[5], (unsigned long long)ls.leaves);
#if NTR_TI_SEEDED
        atomicAdd(&x.stats[6], (unsigned long long)(seedKept || (hitAddr >= 0 && p.triIndex[hitAddr] != -1)));
#else
        atomicAdd(&x.stats[6], (unsigned long long)(hitAddr >= 0 && p.triIndex[hitAddr] != -1));
#endif
#if NTR_TI_MOTION
        atomicAdd(&x.stats[12], (unsigned long long)movingEntries);
        atomicAdd(&x.stats[13], (unsigned long long)singularSteps);
#endif
#if NTR_TI_DEFORM
        atomicAdd(&x.stats[14], (unsigned long long)deformEntries);
        atomicAdd(&x.stats[15], (unsigned long long)deformInner);
        atomicAdd(&x.stats[16], (unsigned long long)deformTris);
#endif
#if NTR_TI_FAST
        if (lane == 0) {   // (lane 0 of a launched wave is a ray)
            atomicAdd(&x.stats[8], (unsigned long long)waveSteps);
            atomicAdd(&x.stats[9], (unsigned long long)fastSteps);
        }
        atomicAdd(&x.stats[10], (unsigned long long)niceStart);
        atomicAdd(&x.stats[11], (unsigned long long)niceEntries);
#endif
    }
}
#if NTR_TI_FAST
#undef NTR_TI_NICE_PIN
#endif
#undef NTR_TI_MOVING
