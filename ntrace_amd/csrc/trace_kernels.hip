// trace_kernels.hip -- CDNA4 (gfx950, wave64) BVH traversal kernels.
//
// Replaces the reference's `trace_bvh` kernels (contract TRACE_FUNC_BVH,
// src/rt/kernels/CudaTracerKernels.hpp:99-112) for BVHLayout_Compact:
//   fermi_speculative_while_while.cu:54-263   -> trace_bvh_perray     (one ray per lane)
//   tesla_persistent_while_while.cu:71-316,
//   kepler_dynamic_fetch.cu:61-322            -> trace_bvh_persistent (persistent waves,
//                                                 ballot/mbcnt refill, LDS stack)
//
// This file holds the loops (traverse, traverse_unified), the three bodies that run them (perray_body, trace_bvh_persistent,
// minipool_body) and the launcher.  What a loop is made of is stated once each, in
//   trace_lane.h      a lane's ray and stack and the steps it takes; ARITHMETIC: why every step is bit-exact against the reference's CPU
//                     tracer, and the GENERIC and FAST forms of the slab test;
//   trace_fetch.h     how 64 bytes reach a lane: descriptor loads, the masked two-buffer fetch, the flat fetch and the end of a buffer;
//   trace_prologue.h  the wave-uniform prologue and its certain steps, with the proof that they decide what the slab test decides;
//   trace_split.h     the drain phase of the persistent waves: idle lanes take over parts of the wave's long rays;
//   compact_bvh.h     the node and triangle layout.
//
// DATA PATH.  The while-while loop (traverse) fetches nodes and Woop triangles with buffer
// loads through wave-uniform resource descriptors (voffset = the Compact layout's own byte
// offsets, so no 64-bit address arithmetic; out-of-range reads return 0 instead of faulting,
// which lets a leaf fetch its triangle and the following terminator word in one round trip).
// The unified-step loop (traverse_unified: every live lane advances by one node OR one
// triangle per iteration) fetches 64 bytes per lane with ONE group of global loads from the
// lane's own buffer, descriptor loads only for the lanes within 64 bytes of a buffer's end.
// The traversal stack lives in LDS ([entry][lane], conflict-free), spilling to scratch
// beyond LDS_DEPTH.  No MFMA: there is no dense contraction on this path.
//
// WHAT IS COMPUTED WHERE.  Everything that is a function of the launch's arguments alone -- the flat fetch's base and offsets, the limits of
// the end-of-buffer tests, the two descriptors, the descent limit and the combined switches -- is formed once on the host (TraceConsts,
// trace_kernels.h; trace_fill_consts, ntr_api.cpp) and copied by the per-ray bodies (unified_bufs<TRIM>, the prologue's HOSTK form); the
// persistent kernels derive their own.  Per wave: a fresh wave of perray_body votes with ballots of compares that have no other use,
// masked by its live lanes on the scalar side -- on the FAST path with ray_class (the rule's ranges as integer arithmetic, trace_lane.h), on
// the octant with three sign ballots, and on the triangle step with wave_may_quirk: a wave without tmax = +inf runs the loop instances
// whose triangle_step<QUIRK = false> writes nothing on a miss, a wave with it the general FAST (or GENERIC) loop in the reference's form.
// minipool_body takes the last vote again after every refill; its refills and the persistent kernels' ask ray_is_nice per ray.
//
// SCHEDULING (never a ray's own visiting order, hence never a hit record or a counter):
//   * a wave leaves its inner-node loop early when few lanes still hold an inner node (leafSwitchBelow);
//   * trace_bvh_perray maps workgroup i to ray block order[i] when an order is given -- predicted
//     (sched_kernels.hip, automatic for large closest-hit launches) or learned from the previous launch of
//     the batch (NtrSchedHint: per-block cost recording here, sched_order_kernel below);
//   * the closest-hit instantiation of trace_bvh_perray runs a batch as wave-private mini-pools (minipool_body: a
//     wave owns K 64-ray chunks of the dispatch order and refills its finished lanes from them) when the pool
//     depth K the device derived for the batch (coherence estimate in sched_kernels.hip) is above 1;
//   * every per-launch counter is cleared by a kernel, so an asynchronous launch can be captured in a HIP
//     graph and replayed.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trace_kernels.h"
#include "trace_lane.h"
#include "trace_fetch.h"
#include "trace_prologue.h"
#include "trace_split.h"

namespace ntr {

// While-while traversal of the lanes' current rays until every lane is done (or, in the
// persistent kernel, until too few lanes are live).  Both loops are wave-uniform (ballots); per-ray
// visiting order is exactly the CPU tracer's depth-first order, whatever the other lanes do.
// SLICED (persistent kernels): the loop also ends after `slice` rounds of it (`slice` counts down; the caller looks at the wave -- posts the
// dequeue of its next chunk -- and calls again).
template <bool FAST, bool STATS, bool DYNAMIC_FETCH, bool SLICED = false>
__device__ __forceinline__ void traverse(Rsrc nodes, Rsrc woop, RayRegs& r, int& node,
                                         LaneStack& st, int (&spill)[SPILL_DEPTH], bool anyHit,
                                         int& hitAddr, float& hitU, float& hitV, LaneStats& ls, unsigned int* status,
                                         bool poolEmpty, int fetchThreshold, int leafSwitchBelow, int* slice = nullptr)
{
    unsigned long long live = __ballot(node != kSentinel);
    while (live != 0ull) {
        if (SLICED && --*slice < 0) break;
        for (;;) {
            const bool inner = (unsigned)node < (unsigned)kSentinel;
            const unsigned long long innerMask = __ballot(inner);
            if (innerMask == 0ull) break;
            // Phase switch policy (affects scheduling only, never a ray's own visiting order): when few
            // lanes still hold an inner node while others already wait at a leaf, serve the leaves first
            // instead of letting a handful of stragglers stall the wave.
            if (__popcll(innerMask) < leafSwitchBelow && __ballot(node < 0) != 0ull) break;
            inner_step<FAST>(nodes, inner, r, node, st, spill, status);
            if (STATS && inner) ls.inner++;
        }
        if (node < 0) {
            if (leaf_step<STATS>(woop, r, node, anyHit, hitAddr, hitU, hitV, ls)) node = kSentinel;
            else node = stack_pop(st, spill);
        }
        live = __ballot(node != kSentinel);
        // dynamic fetch (kepler_dynamic_fetch.cu:310): too few live lanes while rays remain
        // in the pool -> leave the loop so that the idle lanes are refilled.
        if (DYNAMIC_FETCH && !poolEmpty && __popcll(live) < fetchThreshold) break;
    }
}

// Unified-step traversal (the dynamic-fetch kernel's loop).  The while-while loop above lets a wave alternate between an
// inner-node phase and a leaf phase, and a leaf of k triangles costs k dependent round trips during which the lanes that hold
// inner nodes idle: on divergent batches (diffuse / incoherent rays in LBVH trees with 6-triangle leaves) only 9-20 % of the
// lane slots of a wave iteration do work (profiles/r03_divergence_*).  Here EVERY live lane advances by one step per iteration,
// whatever it holds: an inner node (64 B from `nodes`) or the next triangle of its leaf (48 B + the following word from
// `woop`: also 64 contiguous bytes).  Both fetches are issued before the wave waits, so an iteration is ONE memory round trip.
// A lane's own visiting order -- and with it every hit record -- is exactly that of traverse(): only the interleaving of the
// lanes changes.  `node` < 0 doubles as the triangle cursor: the lane's next triangle is at float4 index ~node (a leaf
// reference IS the index of its first triangle; advancing one triangle subtracts 3).
// SLICED (persistent kernels): the loop also ends after `slice` iterations (`slice` counts down: the caller posts the dequeue of the wave's
// next chunk, or -- drain phase -- looks at the wave's lanes again: split_settle / split_donate, trace_split.h).
// TRIM (the per-ray bodies): the loop's upkeep in its cheaper forms -- the fetch's end-of-buffer test (unified_fetch<.., TRIM>), the fetched
// rows kept as the tuples the loads wrote (keep_row) and the straight-line pop (stack_pop_flat).  Same steps, same stack content.  The
// persistent kernels keep the earlier forms: they have no scalar register to give (EXPERIMENTS.md).
// QUIRK = false (the per-ray bodies, a wave without tmax = +inf): triangle_step's form in which a miss writes nothing (trace_lane.h).
template <bool FAST, bool FLAT, int OCT = 8, bool PROLOGUE = false, bool SLICED = false, bool TRIM = false, bool QUIRK = true>
__device__ __forceinline__ void traverse_unified(const UnifiedBufs& ub, RayRegs& r, int& node, LaneStack& st,
                                                 int (&spill)[SPILL_DEPTH], bool anyHit, int& hitAddr, float& hitU, float& hitV,
                                                 unsigned int* status, bool poolEmpty, int fetchThreshold, int* slice = nullptr)
{
    if (PROLOGUE && ub.uniformPrologue) uniform_prologue<FAST, OCT, true, TRIM>(ub, r, node, st, spill, status);   // (PROLOGUE: the per-ray kernels)
    for (;;) {
        const unsigned long long live = __ballot(node != kSentinel);
        if (live == 0ull) break;
        // dynamic fetch (kepler_dynamic_fetch.cu:310): too few live lanes while rays remain in the pool -> refill
        if (!poolEmpty && __popcll(live) < fetchThreshold) break;
        if (SLICED && --*slice < 0) break;
        float4 a, b, c, d;
        unified_fetch<FLAT, TRIM>(ub, node, live, a, b, c, d);
        if (FLAT && TRIM) { keep_row(a); keep_row(b); keep_row(c); keep_row(d); }
        else if (FLAT) { keep(a); keep(b); keep(c); keep(d); }
        unified_advance<FAST, OCT, LDS_DEPTH, TRIM, QUIRK>(a, b, c, d, r, node, st, spill, anyHit, hitAddr, hitU, hitV, status);
    }
}
// A lane of a ray pool (the persistent kernels' refill, minipool_body) starts ray rayIdx at the root.  Returns whether the ray qualifies for the FAST path.
// (the rule in its float form: ray_class, the fresh waves' form, costs the persistent kernels two or three VGPRs and the mini kernel its 60th)
__device__ __forceinline__ bool start_ray(const TraceParams& p, int rayIdx, RayRegs& r, int& node, LaneStack& st,
                                          int& hitAddr, float& hitU, float& hitV)
{
    load_ray(p.rays, rayIdx, r);
    hitAddr = -1;
    hitU = hitV = 0.0f;
    stack_reset(st);
    // tmin < tmax is necessary for any accept (t>tmin && t<tmax):
    // degenerate rays (Util.hpp:65) are misses without traversal.
    node = (r.tmin < r.tmax) ? 0 : kSentinel;
    return ray_is_nice(r, p.bvhFlags);
}

// a whole-wave refill's walk down the top of the tree through the scalar cache while the wave's rays agree (uniform_prologue)
__device__ __forceinline__ void fresh_prologue(bool fastWave, const UnifiedBufs& ub, const RayRegs& r, int& node, LaneStack& st,
                                               int (&spill)[SPILL_DEPTH], unsigned int* status)
{
    if (fastWave) uniform_prologue<true, 8>(ub, r, node, st, spill, status);
    else uniform_prologue<false, 8>(ub, r, node, st, spill, status);
}

// ---------------------------------------------------------------------------------
// Variant 1: one ray per lane ("fermi_speculative_while_while" slot).
// ---------------------------------------------------------------------------------
// UNIFIED: the unified-step loop (traverse_unified) -- every per-ray launch but the stats one, which counts the while-while loop's steps.
// MINI: the launch may run as the wave-private mini-pool instead (minipool_body below), decided on the device per batch.
template <bool FLATF>
__device__ __forceinline__ void minipool_body(const TraceParams& p, unsigned int K, lds_int* stackBase);

#define NTR_PERRAY_BOUNDS(W) __launch_bounds__((W) * 64, NTR_TRACE_MIN_WAVES_PER_SIMD)
template <int WAVES, bool STATS, bool UNIFIED = false, bool FLATF = true, bool MINI = false>
__device__ __forceinline__ void perray_body(const TraceParams& p)
{
    __shared__ int s_stack[WAVES][LDS_DEPTH][64];  // [wave][entry][lane]
    if constexpr (MINI) {
        static_assert(WAVES == 1 && UNIFIED && !STATS, "the mini-pool shares the one-wave unified-step launch");
        unsigned int K = (unsigned int)p.poolKConst;
        if (p.poolK) {               // wave-uniform (scalar load)
            const unsigned int word = *p.poolK;
            if (p.routeSkip == NTR_ROUTE_SKIP_INCOHERENT && NTR_BATCH_WORD_INCOHERENT(word)) return;   // the persistent body behind this launch traces the batch
            K = NTR_BATCH_WORD_K(word);
        }
        bool pooled = K >= 2u && K <= (unsigned int)NTR_MINIPOOL_MAX_K;
        if (pooled) {
            minipool_body<FLATF>(p, K, (lds_int*)&s_stack[0][0][threadIdx.x]);
            return;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // A "block" is 256 consecutive rays (the unit of the dispatch order and of the cost feedback) whatever the workgroup size: a
    // workgroup of WAVES waves traces one of its 4 / WAVES parts.
    constexpr int PARTS = 4 / WAVES;
    const unsigned int g = blockIdx.x / PARTS, part = blockIdx.x % PARTS;
    const unsigned int block = p.order ? p.order[g] : g;
    const int rayIdx = block * 256 + part * (WAVES * 64) + threadIdx.x;
    const bool valid = rayIdx < p.numRays;
    const Rsrc nodes = make_rsrc(p.nodes, p.nodesBytes), woop = make_rsrc(p.woop, p.woopBytes);
    // The launch's scalars and the lane's stack stand in front of the ray's loads.  (Measured, not reasoned: with the loads issued first and
    // the scalars behind them, as the loads' latency suggests, the AO launches are 0.5 % slower, and with the scalars formed where the loops
    // are entered the frame gains nothing from the trims below: EXPERIMENTS.md, wave set-up.)
    UnifiedBufs ub;
    if (UNIFIED) ub = unified_bufs<true>(p);

    unsigned long long tl0 = 0;
    if (p.cost) tl0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz; scheduling feedback

    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[wave][0][lane];
    stack_reset(st);
    RayRegs r;
    load_ray(p.rays, valid ? rayIdx : 0, r);

    int hitAddr = -1;
    float hitU = 0.0f, hitV = 0.0f;
    // No triangle can be accepted unless tmin < tmax (t>tmin && t<tmax), so a
    // degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal.
    const bool live = valid && r.tmin < r.tmax;
    int node = live ? 0 : kSentinel;
    LaneStats ls = {0u, 0u, 0u};
    // the wave's live lanes, once: the votes below are ballots of compares that have no other use, masked on the scalar side (of a predicate
    // that also steers lanes hipcc makes a 0 / 1 VGPR and a second compare), so a dead lane -- a degenerate ray, an index past numRays -- has no say
    const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(live);

    // the launch's switches as the host combined them (TraceConsts)
    const bool fastAllowed = (p.k.switches & NTR_K_FAST) != 0u, octantAllowed = (p.k.switches & NTR_K_OCTANT) != 0u;
    const unsigned int zeroWord = (p.k.switches & NTR_K_ZERO_ORIGIN) ? kPosZero : (kPosZero | 1u);
    const bool fastWave = fastAllowed && (liveMask & __builtin_amdgcn_ballot_w64(ray_class(r, zeroWord) > kNiceMax)) == 0ull;
    // direction signs shared by every live ray of the wave (a primary wave is an 8 x 8 pixel tile): the octant's own slab test
    // (a wave that holds tmax = +inf keeps the general FAST loop, whose triangle step records the reference's missed test: triangle_step)
    int oct = wave_may_quirk(r) ? 9 : 8;   // 9: the general FAST loop with the reference's triangle step, no octant vote
    // Three sign ballots of compares that have no other use, masked by the live lanes on the scalar side; nothing of it runs unless the wave is
    // FAST and the launch allows the vote.
    if (UNIFIED && fastWave && __builtin_expect(oct == 8, 1) && octantAllowed) {
        const unsigned long long sx = liveMask & __builtin_amdgcn_ballot_w64(r.dx < 0.0f), sy = liveMask & __builtin_amdgcn_ballot_w64(r.dy < 0.0f),
                                 sz = liveMask & __builtin_amdgcn_ballot_w64(r.dz < 0.0f);
        if ((sx == 0ull || sx == liveMask) && (sy == 0ull || sy == liveMask) && (sz == 0ull || sz == liveMask))
            oct = (sx ? 1 : 0) | (sy ? 2 : 0) | (sz ? 4 : 0);
    }
    if (UNIFIED) {
#define NTR_UNIFIED_OCT(O) traverse_unified<true, FLATF, O, true, false, true, false>(ub, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, p.status, true, 0)
        if (oct < 8) {
            switch (oct) {
                case 0: NTR_UNIFIED_OCT(0); break;
                case 1: NTR_UNIFIED_OCT(1); break;
                case 2: NTR_UNIFIED_OCT(2); break;
                case 3: NTR_UNIFIED_OCT(3); break;
                case 4: NTR_UNIFIED_OCT(4); break;
                case 5: NTR_UNIFIED_OCT(5); break;
                case 6: NTR_UNIFIED_OCT(6); break;
                default: NTR_UNIFIED_OCT(7); break;
            }
        }
#undef NTR_UNIFIED_OCT
        else if (__builtin_expect(fastWave && oct == 8, 1)) traverse_unified<true, FLATF, 8, true, false, true, false>(ub, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, p.status, true, 0);
        else if (fastWave) traverse_unified<true, FLATF, 8, true, false, true>(ub, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, p.status, true, 0);
        else traverse_unified<false, FLATF, 8, true, false, true>(ub, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, p.status, true, 0);
    } else if (fastWave) traverse<true, STATS, false>(nodes, woop, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, ls, p.status, true, 0, p.leafSwitchBelow);
    else traverse<false, STATS, false>(nodes, woop, r, node, st, spill, p.anyHit != 0, hitAddr, hitU, hitV, ls, p.status, true, 0, p.leafSwitchBelow);

    if (p.cost && lane == 0)  // scheduling feedback: a block's cost is the lifetime of its longest wave
        atomicMax(&p.cost[block], (unsigned int)(__builtin_amdgcn_s_memrealtime() - tl0));
    if (!valid) return;
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    if (STATS) {  // diagnostics variant only: plain per-lane atomics
        atomicAdd(&p.stats[0], (unsigned long long)ls.inner);
        atomicAdd(&p.stats[1], (unsigned long long)ls.tris);
        atomicAdd(&p.stats[2], (unsigned long long)ls.leaves);
        atomicAdd(&p.stats[3], (unsigned long long)(hitAddr >= 0));
    }
}

template <int WAVES, bool STATS, bool UNIFIED = false, bool FLATF = true>
__global__ NTR_PERRAY_BOUNDS(WAVES) void trace_bvh_perray(TraceParams p)
{
    perray_body<WAVES, STATS, UNIFIED, FLATF, false>(p);
}
// The one-wave unified-step launch that may run as mini-pools (K decided on the device).
#define NTR_MINI_BOUNDS __launch_bounds__(64)
__global__ NTR_MINI_BOUNDS void trace_bvh_perray_mini(TraceParams p)
{
    perray_body<1, false, true, true, true>(p);
}
// ... with the two-descriptor fetch, for a BVH whose node and triangle buffers do not lie inside one 4 GiB window (the flat fetch's
// condition): such a batch keeps its ray pools -- without them an incoherent batch is 60 % slower (hairball box rays 3.6 -> 5.8 ms)
__global__ NTR_MINI_BOUNDS void trace_bvh_perray_mini_desc(TraceParams p)
{
    perray_body<1, false, true, false, true>(p);
}

// ---------------------------------------------------------------------------------
// Variant 2: persistent waves.  Each wave owns a chunk [next,end) of the ray index
// space; empty lanes are refilled from the chunk by ballot + mbcnt prefix
// (kepler_dynamic_fetch.cu:97-111 on wave64: 64-bit ballot, v_mbcnt_lo/hi).
// Pool: the index space is cut into numHeads contiguous ranges, one head (counter) each.  A returning atomic on ONE
// address is served at about 88 per us (MI355X_MICROARCH price list, "dequeue"); with 6 144 waves asking at once --
// at launch, and again whenever equally long rays (AO) end together -- eight heads made a dequeue wait 8-12 us
// (profiles/r02b_persistent_vs_perray_timelines.jsonl: 32 % of a wave's life on AO; r02k: 13 % with 64-256 heads, AO batch
// 208 -> 134 us; 512 heads and more lose again to end-of-pool probing).  So: (1) a wave's FIRST chunk is
// assigned statically, no atomic; (2) 128 heads, a block works on head blockIdx % numHeads (blocks are dealt round-robin
// to the XCDs, so head h stays on XCD h % 8 and an XCD's heads cover one contiguous screen region); (3) a wave whose
// head ran dry reads all heads with one 64-lane load and moves to the next one that still has rays, instead of
// paying an atomic round trip per dry head.
// ---------------------------------------------------------------------------------
// UNIFIED: the unified-step loop (traverse_unified) instead of the while-while loop -- what kepler_dynamic_fetch launches.
// Round 6: what a persistent wave does between two chunks used to be 40 % of its life on coherent batches (an AO batch of the headline
// frame: 7 us per refill -- the returning atomic on the pool head, then the ray load, one dependent round trip after the other -- of
// a 20 us chunk; profiles/r05_persist_ao_timeline.jsonl), and a refilled wave ran the general loop where a fresh wave of the per-ray
// kernel runs the octant-specialised one behind the uniform prologue.  Now:
//   * WHOLE-WAVE refills are fresh waves: a wave that was empty and took its rays from one chunk walks the top of the tree through the
//     scalar cache exactly like a wave of the per-ray kernel (uniform_prologue; the octant-specialised slab test is left to the
//     per-ray kernel: eight more loop bodies cost these kernels 6-7 VGPRs, i.e. a wave per SIMD, for +3 %);
//   * the NEXT chunk is dequeued while the current one is traced: `prefetchAfter` iterations into a chunk lane 0 posts the atomic for the
//     wave's next chunk, and the value is there when the wave comes back (not at the start of the chunk: that would commit every wave
//     to two chunks at launch -- 16 384 chunks of an AO batch over 8 192 waves -- and give up the dynamic balancing a pool is for);
//   * kepler_dynamic_fetch refills single lanes (ballot / mbcnt, fetchThreshold) only on batches the device's coherence estimate (poolK)
//     found incoherent -- dynamic fetch pays exactly where the rays of one chunk differ in length, and costs ~10 % where they do not
//     (refilled lanes de-cohere a wave's node fetches) -- and refills whole waves otherwise.  (A per-wave switch decided by how busy a
//     chunk kept its lanes was built first: changing the policy inside the wave's main loop costs 13 VGPRs, i.e. a wave per SIMD.)
// None of this touches a ray's own visiting order: records cannot change.
template <int WAVES, bool UNIFIED = false, bool FLATF = true>
__global__ __launch_bounds__(WAVES * 64, NTR_TRACE_PERSISTENT_MIN_WAVES_PER_SIMD) void trace_bvh_persistent(TraceParams p)
{
    __shared__ int s_stack[WAVES][LDS_DEPTH][64];  // [wave][entry][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Rsrc nodes = make_rsrc(p.nodes, p.nodesBytes), woop = make_rsrc(p.woop, p.woopBytes);
    const bool anyHit = p.anyHit != 0;
    const bool bvhFast = (p.bvhFlags & NTR_BVH_FASTDIV) != 0;
    // How many rays should be in flight?  Beyond the L2 the chip serves ~56 G requests/s from ~64 k requests in flight on; more in flight
    // only adds queueing delay, which every ray -- the batch's longest included -- pays per step (EXPERIMENTS.md, gather roof).  A batch the
    // device found incoherent (pool word > 1: scattered origins, every step a cache miss) is therefore traced by HALF the grid:
    // courtyard-10M box rays 5.12 -> 4.60 ms, hairball 4.16 -> 3.43 ms; coherent batches keep the full grid (atrium primary 0.57 against
    // 0.67 ms with half).  Workgroups beyond the effective grid leave at once; everything below counts with the effective grid.
    int numBlocksEff = p.numBlocks;   // wave-uniform
    const unsigned int batchWord = p.poolK ? *p.poolK : 1u;
    const bool incoherentBatch = NTR_BATCH_WORD_INCOHERENT(batchWord);   // scattered origins, or long rays that point apart: single-lane refills
    if (p.routeSkip == NTR_ROUTE_SKIP_COHERENT && !incoherentBatch) return;   // the per-ray body beside this launch traces the batch
    // (round 6: a diffuse batch -- rays that start together and wander apart -- gains from fewer rays in flight too: one hairball batch 2.03 ms with
    // eight workgroups per CU, 1.57 with four, 1.63-1.74 with three; scattered origins -- box rays -- are best with three: 2.86 against 3.4 ms with four)
    const int gridIncoherent = NTR_BATCH_WORD_K(batchWord) > 1u ? p.numBlocksIncoherent : p.numBlocksDivergent;
    if (incoherentBatch && gridIncoherent > 0 && gridIncoherent < numBlocksEff) numBlocksEff = gridIncoherent;
    if ((int)blockIdx.x >= numBlocksEff) return;

    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[wave][0][lane];
    stack_reset(st);

    RayRegs r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int node = kSentinel, rayIdx = -1, hitAddr = -1;
    float hitU = 0.0f, hitV = 0.0f;
    bool nice = true;                 // this lane's current ray qualifies for the FAST path
    int chunkNext = 0, chunkEnd = 0;  // wave-uniform
    bool poolEmpty = false;           // wave-uniform
    const int numHeads = p.numHeads;
    int shard = (int)(blockIdx.x % (unsigned)numHeads);  // wave-uniform
    bool firstChunk = true;
    // Pool positions: head h owns positions [h * shardRays, (h + 1) * shardRays).  Buffer order (p.order == null): the k-th chunk of head h
    // is chunk k * numHeads + h of the batch -- the heads interleave, so every head holds an even sample of the batch and all of them
    // run dry together.  (Until round 6 a head owned a CONTIGUOUS range of the batch, "so that an XCD's L2 sees one screen region": the
    // heads of cheap screen regions then ran dry early, their waves all moved to the same next head -- a returning atomic on one address
    // is served at ~88 per us -- and a coherent launch spent most of its time in that queue whatever its occupancy: AO batches 145 us
    // with 6, 7 or 8 workgroups per CU alike, against 52 us for the per-ray kernel, whose workgroups interleave over the XCDs the same
    // way.)  Predicted-cost order (p.order: the 256-ray blocks heaviest class first, sched_kernels.hip): the positions of head h are the
    // blocks order[h], order[h + numHeads], order[h + 2 numHeads], ... -- every head hands its blocks out from heavy to light, so the
    // long-lived rays of the batch start first instead of forming the tail of the launch.  Either way the pool spans numHeads * shardRays
    // positions and a position may lie beyond the batch: it is skipped.
    const unsigned int* const order = p.order;
    const int poolEnd = numHeads * p.shardRays;
    auto range_beg = [&](int h) { return h * p.shardRays; };
    int chunkDelta = 0;               // wave-uniform: ray index - pool position inside the current chunk (a chunk never spans two 256-ray blocks)
    // the chunk at position `base` of head h: where its rays are in the batch.  One scalar load per chunk in the ordered pool (until round 6
    // every lane looked its block up in order[] itself: a dependent vector load on the refill's critical path)
    auto chunk_delta = [&](int base, int h) {
        const int off = base - h * p.shardRays;
        if (!order) return ((off / p.chunk) * numHeads + h) * p.chunk - base;
        const int q = (off >> 8) * numHeads + h;                  // the block's place in the predicted / learned order
        if (q >= p.orderBlocks) return 0x3FFFFFFF - base;          // beyond the batch: every position of the chunk maps past numRays
        return (int)order[q] * 256 + (off & 255) - base;
    };
    // chunks of head h handed out statically: one per wave of every block with blockIdx % numHeads == h
    auto static_rays = [&](int h) { return ((numBlocksEff - h + numHeads - 1) / numHeads) * WAVES * p.chunk; };
    LaneStats ls = {0u, 0u, 0u};
    // drain phase (unified-step loop): once the pool is dry, idle lanes take over parts of the wave's rays (trace_split.h)
    SplitState split;
    split_reset(split);
    bool splitOn = false;             // wave-uniform
    const int splitSlice = UNIFIED ? p.splitSlice : 0;

    // refill policy (wave-uniform): whole-wave (a wave takes rays only when it holds none) or dynamic fetch (fewer than fetchThreshold
    // lanes live -> the idle lanes take rays; kepler_dynamic_fetch.cu:310)
    const bool dynamicFetch = p.fetchThreshold > 0 && (!UNIFIED || p.wholeWave == 0 || incoherentBatch);
    // dequeue-ahead: the atomic of the wave's next chunk, posted `prefetchAfter` iterations into the current one
    int prefetched = 0;               // lane 0: what the atomic returned
    bool havePrefetch = false;        // wave-uniform
    int prefetchHead = 0;             // wave-uniform: the head it was posted on
    int prefetchIn = -1;              // wave-uniform: iterations until the prefetch is posted (< 0: none pending)
    // scheduling feedback (a hint's refresh launch, whole-wave mode): a 256-ray block's cost is the life of the longest chunk taken from it
    int costBlock = -1;               // wave-uniform: the block of the chunk in flight (-1: none / not recorded)
    unsigned long long costT0 = 0;

    // The wave's next chunk: its statically assigned first one, the one it dequeued ahead, or an atomic on its head -- and when that head
    // is dry, on the next head that still has rays.  Sets chunkNext / chunkEnd / chunkHead / chunkDelta; false = the pool is dry.
    // The ray index space is dealt to numHeads pool heads (a single head saturates near 88 dequeues/us, MI355X_MICROARCH price list "dequeue").
    auto grab = [&]() -> bool {
        bool got = false;
        auto take = [&](int base, int h) {
            const int rangeBeg = range_beg(h);
            const int rangeEnd = min(rangeBeg + p.shardRays, poolEnd);
            if (base >= rangeEnd) return false;
            chunkNext = base;
            chunkEnd = min(base + p.chunk, rangeEnd);
            chunkDelta = chunk_delta(base, h);
            return true;
        };
        if (firstChunk) {  // static: the (blockIdx / numHeads * WAVES + wave)-th chunk of the block's head
            firstChunk = false;
            got = take(range_beg(shard) + ((int)(blockIdx.x / (unsigned)numHeads) * WAVES + __builtin_amdgcn_readfirstlane(wave)) * p.chunk, shard);
        } else if (havePrefetch) {   // the dequeue posted while the previous chunk was traced
            havePrefetch = false;    // (a head that ran dry meanwhile: the search below starts on it and moves on)
            got = take(__builtin_amdgcn_readfirstlane(prefetched) + static_rays(prefetchHead) + range_beg(prefetchHead), prefetchHead);
        }
        while (!got) {
            int base = 0;
            if (lane == 0) base = atomicAdd(p.counter + shard * 16, p.chunk);
            if (take(__builtin_amdgcn_readfirstlane(base) + static_rays(shard) + range_beg(shard), shard)) { got = true; break; }
            // dry: lane l looks at head (shard + 1 + l) % numHeads; counters only grow, so a head seen dry stays dry
            unsigned long long live = 0ull;
            int ofs = 1;
            for (; ofs < numHeads && live == 0ull; ofs += 64) {
                bool has = false;
                if (ofs + lane < numHeads) {
                    const int h = (shard + ofs + lane) % numHeads;
                    const int hb = range_beg(h);
                    const int he = min(hb + p.shardRays, poolEnd);
                    const int taken = __hip_atomic_load(p.counter + h * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    has = hb + static_rays(h) + taken < he;
                }
                live = __ballot(has);
            }
            if (live == 0ull) break;
            shard = (shard + ofs - 64 + (int)__builtin_ctzll(live)) % numHeads;
        }
        if (got) prefetchIn = p.prefetchAfter;   // (negative: no dequeue-ahead)
        return got;
    };
    // scheduling feedback: the 256-ray block of the chunk just grabbed
    auto cost_open = [&]() {
        costBlock = (chunkEnd - p.chunk + chunkDelta) >> 8;
        if ((unsigned)costBlock >= (unsigned)((p.numRays + 255) >> 8)) costBlock = -1;
        costT0 = __builtin_amdgcn_s_memrealtime();
    };

    // Invariant at the top of the loop: a lane either holds a live ray
    // (rayIdx >= 0, node != sentinel) or is empty (rayIdx < 0, node == sentinel).
    for (;;) {
        // ---- refill empty lanes from the wave's chunk ----------------------------
        unsigned long long empty = __ballot(rayIdx < 0);
        const bool wholeWave = empty == ~0ull;
        const bool refill = !poolEmpty && (wholeWave || (dynamicFetch && 64 - __popcll(empty) < p.fetchThreshold));
        while (refill && empty != 0ull && !poolEmpty) {
            if (chunkNext >= chunkEnd && !grab()) { poolEmpty = true; break; }
            const int prefix = lane_rank(empty);
            const int avail = chunkEnd - chunkNext;
            const int pos = chunkNext + prefix + chunkDelta;   // pool position -> ray index (beyond the batch: skipped)
            if (rayIdx < 0 && prefix < avail && pos < p.numRays) {
                rayIdx = pos;
                nice = start_ray(p, rayIdx, r, node, st, hitAddr, hitU, hitV);
            }
            chunkNext += min(__popcll(empty), avail);
            empty = __ballot(rayIdx < 0);
            if (wholeWave && !dynamicFetch) break;   // whole-wave mode takes rays ONCE per refill (a short last chunk stays short)
        }
        const bool fresh = refill && wholeWave;   // every ray the wave holds starts at the root now
        if (p.cost && refill && wholeWave && !dynamicFetch && !poolEmpty) cost_open();

        // ---- drain phase: lanes without a ray take over stack entries of the wave's live rays (unified-step loop) ------------------
        if (UNIFIED && poolEmpty && splitSlice > 0) {
            if (!splitOn) { splitOn = true; split_reset(split); }
            split_donate(split, r, node, st, rayIdx, hitAddr, hitU, hitV, nice);
        }
        const bool fastWave = bvhFast && __ballot(node != kSentinel && !nice) == 0ull;
        // dequeue-ahead: the traversal comes back after `prefetchIn` iterations, the atomic is posted, the traversal goes on
        int slice = 0x7FFFFFFF;
        if (splitOn) slice = splitSlice;   // drain phase with splitting: the lanes are looked at again every `slice` steps
        else if (prefetchIn >= 0 && !poolEmpty) slice = prefetchIn;
        const int fetchBelow = dynamicFetch ? p.fetchThreshold : 0;
        if (UNIFIED) {
            const UnifiedBufs ub = unified_bufs(p);
            if (fresh && p.uniformPrologue) fresh_prologue(fastWave, ub, r, node, st, spill, p.status);
            if (fastWave) traverse_unified<true, FLATF, 8, false, true>(ub, r, node, st, spill, anyHit, hitAddr, hitU, hitV, p.status, poolEmpty, fetchBelow, &slice);
            else traverse_unified<false, FLATF, 8, false, true>(ub, r, node, st, spill, anyHit, hitAddr, hitU, hitV, p.status, poolEmpty, fetchBelow, &slice);
            if (splitOn) split_settle(split, r, node, st, hitAddr, hitU, hitV, anyHit);
        } else {
            if (fresh && p.uniformPrologue) fresh_prologue(fastWave, unified_bufs(p), r, node, st, spill, p.status);
            if (fastWave) traverse<true, false, true, true>(nodes, woop, r, node, st, spill, anyHit, hitAddr, hitU, hitV, ls, p.status, poolEmpty, fetchBelow, p.leafSwitchBelow, &slice);
            else traverse<false, false, true, true>(nodes, woop, r, node, st, spill, anyHit, hitAddr, hitU, hitV, ls, p.status, poolEmpty, fetchBelow, p.leafSwitchBelow, &slice);
        }
        // ---- dequeue-ahead: post the atomic of the wave's next chunk now (its latency hides behind the rest of this chunk) -------------
        if (!splitOn && prefetchIn >= 0 && !poolEmpty) {
            prefetchIn = -1;
            if (!havePrefetch && __ballot(node != kSentinel) != 0ull) {   // (a wave that is done already dequeues in the refill above)
                if (lane == 0) prefetched = atomicAdd(p.counter + shard * 16, p.chunk);
                havePrefetch = true;
                prefetchHead = shard;
            }
        }

        // ---- retire finished rays (an owner whose helpers are still out waits for their reports) ------
        if (rayIdx >= 0 && node == kSentinel && (!splitOn || split.base == 0)) {
            store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
            rayIdx = -1;
        }
        if (costBlock >= 0 && __ballot(rayIdx >= 0) == 0ull) {   // the chunk is done
            if (lane == 0) atomicMax(&p.cost[costBlock], (unsigned int)(__builtin_amdgcn_s_memrealtime() - costT0));
            costBlock = -1;
        }
        if (poolEmpty && __ballot(rayIdx >= 0) == 0ull) break;
    }
}

// ---------------------------------------------------------------------------------
// Variant 3: per-ray kernel with a wave-private mini-pool (round 3).  A hardware-scheduled 64-thread workgroup owns K x 64 consecutive
// rays instead of 64: its lanes start on the first 64, and a lane that finishes takes the wave's next unstarted ray (ballot + mbcnt
// prefix over the wave's OWN range: no atomic, no shared head).  On divergent batches the per-ray kernel's waves live as long as their
// longest ray while most lanes idle (lane utilisation 0.22-0.48 on the LBVH scenes, scripts/studies/divergence_study.py); list scheduling K x 64
// rays on 64 lanes lifts that to 0.33-0.63 (K = 2) / 0.49-0.77 (K = 4) by the per-ray step counts, at the price of a longer critical
// path per wave -- which is why the pool stays small and private: the global pool of the persistent kernels keeps every lane busy
// until it runs dry, and then 6 144 waves each hold a few long rays (a tail of 60-70 % of their launch, profiles/r03_divergence_timelines.jsonl).
// Unified-step loop, flat fetch; 256-ray blocks keep their role as the unit of the dispatch order and of the cost feedback.
// ---------------------------------------------------------------------------------
template <bool FLATF>
__device__ __forceinline__ void minipool_body(const TraceParams& p, unsigned int K, lds_int* stackBase)
{
    // The launch has one wave per 64-ray chunk (the per-ray kernel's grid); K consecutive chunks of the dispatch order form a pool, and one
    // workgroup of every K owns it, the others exit at once.  WHICH one must not follow a regular pattern: workgroups are dealt round-robin
    // to XCDs, shader engines and CUs, and "every 4th workgroup" put all live waves on a quarter of the chip (measured 2.7x slower, with the
    // XCD bits excluded just the same).  So the live member of a group is picked by a golden-ratio hash of the group's position.
    const int lane = threadIdx.x;
    const unsigned int numChunks = gridDim.x;                                    // 4 per 256-ray block of the order, the last block's empty ones included
    const unsigned int q = blockIdx.x / K;                                       // wave-uniform (one software division per wave)
    const unsigned int members = min(K, numChunks - q * K);                      // (the last group may be short)
    if (blockIdx.x - q * K != ((((q * 0x9E3779B1u) >> 16) * members) >> 16)) return;
    unsigned int chunk = q * K;
    const unsigned int chunkEnd = min(chunk + K, numChunks);
    if (chunk >= chunkEnd) return;
    // chunk c of the order = quarter (c & 3) of block order[c >> 2]
    unsigned int block = p.order ? p.order[chunk >> 2] : (chunk >> 2);
    int poolNext = (int)(block * 256u + (chunk & 3u) * 64u);                     // wave-uniform: the unstarted rays of the current chunk
    int poolEnd = min(poolNext + 64, p.numRays);
    const bool anyHit = p.anyHit != 0;
    const bool bvhFast = (p.bvhFlags & NTR_BVH_FASTDIV) != 0;
    const UnifiedBufs ub = unified_bufs<true>(p);

    unsigned long long tl0 = 0;
    if (p.cost) tl0 = __builtin_amdgcn_s_memrealtime();

    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = stackBase;
    stack_reset(st);
    RayRegs r = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int node = kSentinel, rayIdx = -1, hitAddr = -1;
    float hitU = 0.0f, hitV = 0.0f;
    bool nice = true;

    for (;;) {
        // ---- start the wave's next rays on its empty lanes (from the current chunk; what it cannot fill is filled next time round) --
        while (poolNext >= poolEnd && chunk + 1u < chunkEnd) {
            chunk++;
            block = p.order ? p.order[chunk >> 2] : (chunk >> 2);
            poolNext = (int)(block * 256u + (chunk & 3u) * 64u);
            poolEnd = min(poolNext + 64, p.numRays);
        }
        const unsigned long long empty = __ballot(rayIdx < 0);
        if (empty != 0ull && poolNext < poolEnd) {
            const int prefix = lane_rank(empty);
            const int avail = poolEnd - poolNext;
            if (rayIdx < 0 && prefix < avail) {
                rayIdx = poolNext + prefix;
                nice = start_ray(p, rayIdx, r, node, st, hitAddr, hitU, hitV);
            }
            poolNext += min(__popcll(empty), avail);
        }
        const bool poolEmpty = poolNext >= poolEnd && chunk + 1u >= chunkEnd;
        // ---- unified-step traversal until every lane is done, or (rays left in the pool) until enough lanes are free to be worth a refill --
        const bool fastWave = bvhFast && __ballot(node != kSentinel && !nice) == 0ull;
        if (fastWave && !wave_may_quirk(r)) traverse_unified<true, FLATF, 8, false, false, true, false>(ub, r, node, st, spill, anyHit, hitAddr, hitU, hitV, p.status, poolEmpty, p.fetchThreshold);
        else if (fastWave) traverse_unified<true, FLATF, 8, false, false, true>(ub, r, node, st, spill, anyHit, hitAddr, hitU, hitV, p.status, poolEmpty, p.fetchThreshold);
        else traverse_unified<false, FLATF, 8, false, false, true>(ub, r, node, st, spill, anyHit, hitAddr, hitU, hitV, p.status, poolEmpty, p.fetchThreshold);
        // ---- retire finished rays -------------------------------------------------------------------------------------------------
        if (rayIdx >= 0 && node == kSentinel) {
            store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
            rayIdx = -1;
        }
        if (poolEmpty && __ballot(rayIdx >= 0) == 0ull) break;
    }
    if (p.cost && lane == 0) {  // scheduling feedback: a block's cost is the lifetime of the longest wave that traced a part of it
        const unsigned int life = (unsigned int)(__builtin_amdgcn_s_memrealtime() - tl0);
        for (unsigned int c = q * K; c < chunkEnd; c += 4u - (c & 3u)) atomicMax(&p.cost[p.order ? p.order[c >> 2] : (c >> 2)], life);
    }
}

}  // namespace ntr

// ---- host-side launchers (called from ntr_api.cpp) -----------------------------------
extern "C" hipError_t ntr_launch_trace(int variant, const ntr::TraceParams* p, int numBlocks, hipStream_t stream)
{
    constexpr int WAVES = NTR_TRACE_WAVES_PER_BLOCK;
    switch (variant) {
    case NTR_VARIANT_PERRAY_UNIFIED_W1:   // flatFetch 0: the two-group descriptor fetch (A/B; extents below 64 bytes)
        if (p->flatFetch) hipLaunchKernelGGL((ntr::trace_bvh_perray<1, false, true, true>), dim3(numBlocks), dim3(64), 0, stream, *p);
        else hipLaunchKernelGGL((ntr::trace_bvh_perray<1, false, true, false>), dim3(numBlocks), dim3(64), 0, stream, *p);
        break;
    case NTR_VARIANT_PERRAY_UNIFIED_MINI:   // numBlocks counts waves of 64 rays
        if (p->flatFetch) hipLaunchKernelGGL(ntr::trace_bvh_perray_mini, dim3(numBlocks), dim3(64), 0, stream, *p);
        else hipLaunchKernelGGL(ntr::trace_bvh_perray_mini_desc, dim3(numBlocks), dim3(64), 0, stream, *p);
        break;
    case NTR_VARIANT_PERRAY_STATS:
        hipLaunchKernelGGL((ntr::trace_bvh_perray<WAVES, true>), dim3(numBlocks), dim3(WAVES * 64), 0, stream, *p);
        break;
    case NTR_VARIANT_PERSISTENT_UNIFIED:
        if (p->flatFetch) hipLaunchKernelGGL((ntr::trace_bvh_persistent<WAVES, true, true>), dim3(numBlocks), dim3(WAVES * 64), 0, stream, *p);
        else hipLaunchKernelGGL((ntr::trace_bvh_persistent<WAVES, true, false>), dim3(numBlocks), dim3(WAVES * 64), 0, stream, *p);
        break;
    case NTR_VARIANT_PERSISTENT:
        hipLaunchKernelGGL((ntr::trace_bvh_persistent<WAVES, false>), dim3(numBlocks), dim3(WAVES * 64), 0, stream, *p);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
