// ntr_api.cpp -- C-ABI of libntrace_amd.so (declared in include/ntrace_amd.h).
//
// Thin layer: argument checks mirroring the reference's host-side checks, HIP
// event timing mirroring CudaKernel::launchTimed (src/framework/gpu/CudaKernel.cpp:188-221),
// and kernel launches.  There is deliberately no CPU path here: with no HIP device
// every compute entry point fails (NTR_ERR_NO_DEVICE / NTR_ERR_HIP).

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "ntrace_amd.h"
#include "ntr_internal.h"
#include "compact_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
#include "trace_kernels.h"
#include "trace_plan.h"

namespace {

thread_local char g_err[512] = "";

}  // namespace

namespace ntr {

int set_error(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    int code = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver)
                   ? NTR_ERR_NO_DEVICE : NTR_ERR_HIP;
    return set_error(code, "%s: %s", what, hipGetErrorString(e));
}

bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); return false; }
    return st != hipStreamCaptureStatusNone;
}

struct KernelInfo {
    const char* name;
    int variant;
    NtrKernelConfig cfg;
};

// Reference kernel selectors (file names under src/rt/kernels/) -> CDNA4 variants.
// All CDNA4 variants consume BVHLayout_Compact (the reference fork asserts Compact
// for every BVH it builds, src/rt/cuda/CudaBVH.cpp:65-82).
static const KernelInfo kKernels[] = {
    {"fermi_speculative_while_while", NTR_VARIANT_PERRAY,
     {NTR_BVHLayout_Compact, 64, 1, 0}},   // the per-ray kernel is launched in 64-thread workgroups (one wave)
    {"tesla_persistent_while_while", NTR_VARIANT_PERSISTENT,
     {NTR_BVHLayout_Compact, 64, NTR_TRACE_WAVES_PER_BLOCK, 1}},
    {"tesla_persistent_speculative_while_while", NTR_VARIANT_PERSISTENT,
     {NTR_BVHLayout_Compact, 64, NTR_TRACE_WAVES_PER_BLOCK, 1}},
    {"kepler_dynamic_fetch", NTR_VARIANT_PERSISTENT,
     {NTR_BVHLayout_Compact, 64, NTR_TRACE_WAVES_PER_BLOCK, 1}},
};

static const KernelInfo* find_kernel(const char* name)
{
    if (!name) return nullptr;
    for (const KernelInfo& k : kKernels)
        if (strcmp(k.name, name) == 0) return &k;
    return nullptr;
}

// The batch as the launch plan sees it (trace_plan.h): for a launch (trace_impl) and for the CPU tier's query (ntr_trace_plan) alike.
static TraceBatchDesc describe_batch(const KernelInfo* k, int32_t numRays, int32_t anyHit, uint64_t nodesAddr, int64_t nodesBytes,
                                     uint64_t woopAddr, int64_t triWoopBytes, uint32_t bvhFlags, bool wantStats, bool capturing,
                                     bool callerHint, int numCUs)
{
    TraceBatchDesc bd;
    bd.variant = k->variant; bd.dynamicFetch = strcmp(k->name, "kepler_dynamic_fetch") == 0;
    bd.numRays = numRays; bd.anyHit = anyHit != 0; bd.bvhFlags = bvhFlags;
    bd.nodesBytes = nodesBytes; bd.triWoopBytes = triWoopBytes;
    bd.nodesAddr = nodesAddr; bd.woopAddr = woopAddr;
    bd.wantStats = wantStats; bd.capturing = capturing; bd.callerHint = callerHint;
    bd.numCUs = numCUs;
    return bd;
}

// What trace_impl's bind step hands its launch step: the parameters of the two sides and the scheduling work around them.
struct TraceLaunch {
    TraceParams p{};                  // the per-ray side (p holds the batch when the bind step starts)
    TraceParams pp{};                 // the persistent side
    bool persistentSide = false, perraySide = false;
    NtrSchedHint* hint = nullptr;     // the caller's hint or the library's own (auto_hint_get)
    bool refresh = false;             // the launch records per-block costs; the next order is derived right after it
    bool probeCoherence = false;      // the hint's coherence words are estimated again before the launch
    TopTable* predTable = nullptr;
    PredictScratch* predScratch = nullptr;   // non-null: the dispatch order is predicted before the launch
};

// The launch constants of the per-ray bodies (TraceParams::k): everything a wave would derive from the launch's arguments alone.
static void trace_fill_consts(TraceParams& p)
{
    TraceConsts& k = p.k;
    const unsigned long long an = (unsigned long long)p.nodes, aw = (unsigned long long)p.woop, lo = an < aw ? an : aw;
    k.base = (const char*)lo;
    k.dN = (uint32_t)(an - lo); k.dW = (uint32_t)(aw - lo);
    k.limNode = p.nodesBytes - (uint32_t)kNodeBytes;
    k.limTri = leaf_link((int)((p.woopBytes - (uint32_t)kNodeBytes) >> kRowShift));
    k.oddBase = k.limNode + 1u; k.oddSpan = (uint32_t)k.limTri - k.oddBase;
    // descriptor words: base, base_hi (stride 0), extent in bytes, flags (what make_rsrc builds)
    k.rNodes[0] = (uint32_t)an; k.rNodes[1] = (uint32_t)(an >> 32) & 0xFFFFu; k.rNodes[2] = p.nodesBytes; k.rNodes[3] = 0x00020000u;
    k.rWoop[0] = (uint32_t)aw; k.rWoop[1] = (uint32_t)(aw >> 32) & 0xFFFFu; k.rWoop[2] = p.woopBytes; k.rWoop[3] = 0x00020000u;
    k.descentLim = !p.certainDescent ? 0u : k.limNode < (uint32_t)kSentinel ? k.limNode : (uint32_t)kSentinel - 1u;
    const bool ordered = (p.bvhFlags & NTR_BVH_ORDERED) != 0;
    k.switches = ((p.bvhFlags & NTR_BVH_FASTDIV) ? NTR_K_FAST : 0u) | ((p.bvhFlags & NTR_BVH_NOTINY) ? NTR_K_ZERO_ORIGIN : 0u) |
                 ((p.octant && ordered) ? NTR_K_OCTANT : 0u) | ((p.certainSteps && ordered) ? NTR_K_CERTAIN : 0u) |
                 ((p.uniformPrologue && (an & (unsigned long long)(kNodeBytes - 1)) == 0ull) ? NTR_K_PROLOGUE : 0u);
}

// Binds the run-time state the plan asks for -- hint, prediction scratch, pool counters -- and derives both sides' parameters from L->p.
static int bind_trace(DeviceState* ds, const Tunables& tun, const TracePlan& pl, bool capturing, int64_t nodesBytes, hipStream_t s,
                      NtrSchedHint* hint, TraceLaunch* L)
{
    TraceParams& p = L->p;
    const int variant = pl.variant, orderBlocks = pl.orderBlocks;
    int rc = NTR_OK;
    // no hint from the caller: the library's own, keyed by (stream, batch, BVH)
    if (pl.useAutoHint) {
        rc = auto_hint_get(ds, p.rays, p.nodes, p.numRays, p.anyHit, s, orderBlocks, &hint);
        if (rc != NTR_OK) return rc;
    }
    L->hint = hint;
    // Scheduling hint: the per-ray kernel dispatches blocks in the hint's order, the persistent kernels hand their pool out in it; on
    // refresh launches per-block costs are recorded, from which the next order is derived right after the launch.
    if (hint && pl.hintable) {
        if (hint->numBlocks != orderBlocks || hint->device != ds->device) {
            rc = sched_hint_bind(hint, orderBlocks, ds->device, s);   // (automatic hints arrive bound: auto_hint_get)
            if (rc != NTR_OK) return rc;
        }
        const HintStep hs = plan_hint_step(tun, hint->valid, hint->predicted, hint->uses);
        if (hs.zeroK) {
            const hipError_t zk = ntr_launch_zero_words(hint->order + orderBlocks, 3, s);
            if (zk != hipSuccess) return hip_fail(zk, "zero_words launch");
        }
        L->refresh = hs.refresh;
        hint->predicted = false;
        hint->uses++;
        if (hs.useOrder) p.order = hint->order;
        if (L->refresh) {
            const hipError_t ze = ntr_launch_zero_words(hint->cost, orderBlocks, s);
            if (ze != hipSuccess) return hip_fail(ze, "zero_words launch");
            p.cost = hint->cost;
        }
    }

    // Dispatch-order prediction (plan_trace: which launches qualify).  A launch whose hint holds no measured order yet -- the first one
    // of a batch -- is predicted like an unhinted one, and the prediction is flattened straight into the hint's order (its batch word goes
    // there too): when the launch records no cost -- the persistent body in dynamic-fetch mode -- the hint keeps the predicted order
    // instead of one derived from nothing.
    if (pl.predictable && !(hint && hint->valid) && !p.order) {
        rc = top_table_get(ds, p.nodes, nodesBytes, s, false, &L->predTable);
        if (rc != NTR_OK) return rc;
        rc = predict_scratch_get(ds, s, orderBlocks, &L->predScratch);
        if (rc != NTR_OK) return rc;
        if (L->predScratch) p.order = (hint && pl.hintable) ? hint->order : L->predScratch->order;
        else L->predTable = nullptr;   // (a captured launch that found no spare scratch: buffer order)
    }

    // A hinted batch is predicted once (its hint then holds a measured order); its coherence words -- the batch word: mini-pool K, routing --
    // are estimated again on the hint's refresh launches by a probe of their own (three small launches, on the refresh launches only -- trace_plan.h plan_hint_step): rays drift.
    L->probeCoherence = !L->predScratch && hint && L->refresh && pl.probeOnRefresh;
    if (L->probeCoherence) {
        rc = top_table_get(ds, p.nodes, nodesBytes, s, false, &L->predTable);
        if (rc != NTR_OK) return rc;
    }
    // The batch word (sched_kernels.hip pool_k): the prediction of this launch writes it, or the batch's hint kept it from its first,
    // predicted launch (zero -- "coherent", K = 1 -- when there never was one).  It sets the mini-pool depth of the per-ray launch, the grid
    // and refill policy of a persistent launch, and -- routed launches -- which of the two bodies works.
    const unsigned int* word = nullptr;
    if (L->predScratch) word = L->predScratch->classCount + NTR_SCHED_PRED_CLASSES + 2;
    else if (hint && pl.hintable && hint->numBlocks == orderBlocks && hint->order) word = hint->order + orderBlocks + 2;
    const bool routed = pl.coherentRoute == 1 && word != nullptr;
    L->persistentSide = variant == NTR_VARIANT_PERSISTENT || routed;
    L->perraySide = variant != NTR_VARIANT_PERSISTENT || routed;
    if ((pl.minipool && pl.poolKFromDevice) || L->persistentSide) p.poolK = word;

    TraceParams& pp = L->pp = p;
    if (L->persistentSide) {
        rc = counter_set_take(ds, capturing, &pp.counter);
        if (rc != NTR_OK) return rc;
        pp.numBlocks = pl.persistentBlocks; pp.numBlocksIncoherent = pl.numBlocksIncoherent; pp.numBlocksDivergent = pl.numBlocksDivergent;
        pp.fetchThreshold = pl.persistentFetchThreshold;
        pp.shardRays = pl.shardRays;
        if (pp.order) {   // every head walks its share of the order: ranges of whole 256-ray blocks
            pp.orderBlocks = orderBlocks;
            pp.shardRays = ((orderBlocks + pp.numHeads - 1) / pp.numHeads) * 256;
        }
        pp.routeSkip = routed ? NTR_ROUTE_SKIP_COHERENT : 0;
    }
    if (routed) {
        p.routeSkip = NTR_ROUTE_SKIP_INCOHERENT;
        if (variant == NTR_VARIANT_PERSISTENT) { p.fetchThreshold = pl.perrayFetchThreshold; p.poolKConst = 1; }
    }
    trace_fill_consts(p);
    trace_fill_consts(pp);
    return NTR_OK;
}

// The kernels of a bound launch, the prediction or probe inside the timed bracket, then the refresh of the hint's order.
static int launch_trace(DeviceState* ds, const Tunables& tun, const TracePlan& pl, const TraceLaunch& L, hipStream_t s, float* seconds,
                        NtrTraceStats* stats)
{
    const TraceParams& p = L.p;
    NtrSchedHint* hint = L.hint;
    const int orderBlocks = pl.orderBlocks;
    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));  // launchTimed syncs first (CudaKernel.cpp:193)
        NTR_HIP(ev.record(0));
    }
    if (L.predScratch) {  // inside the timed bracket: the prediction is part of what the launch costs
        const hipError_t pe = ntr_launch_predict(p.rays, p.numRays, orderBlocks, L.predTable->table, L.predTable->count, L.predScratch->classCount,
                                                 L.predScratch->classList, (hint && pl.hintable) ? hint->order : L.predScratch->order,
                                                 (hint && pl.hintable) ? hint->order + orderBlocks + 2 : nullptr, pl.minipoolWide, s);
        if (pe != hipSuccess) return hip_fail(pe, "predict launch");
    } else if (L.probeCoherence) {   // (also inside the bracket)
        const hipError_t ce = ntr_launch_coherence(p.rays, p.numRays, orderBlocks, L.predTable->table, L.predTable->count, hint->order + orderBlocks,
                                                  pl.minipoolWide, s);
        if (ce != hipSuccess) return hip_fail(ce, "coherence launch");
    }
    hipError_t le = hipSuccess;
    if (L.persistentSide) {
        // the pool heads are cleared by a kernel: memset nodes do not survive HIP graph replays (see sched_kernels.hip)
        le = ntr_launch_zero_words(L.pp.counter, kPoolHeadsMax * 16, s);
        if (le != hipSuccess) return hip_fail(le, "zero_words launch");
        le = ntr_launch_trace(pl.persistentVariant, &L.pp, pl.persistentBlocks, s);
        if (le != hipSuccess) return hip_fail(le, "trace_bvh launch");
    }
    if (L.perraySide) {
        le = pl.variant == NTR_VARIANT_PERSISTENT ? ntr_launch_trace(NTR_VARIANT_PERRAY_UNIFIED_MINI, &p, pl.perrayBlocks, s)
                                                  : ntr_launch_trace(pl.launchVariant, &p, pl.launchBlocks, s);
        if (le != hipSuccess) return hip_fail(le, "trace_bvh launch");
    }
    if (seconds) NTR_HIP(ev.record(1));
    if (L.refresh) {
        le = ntr_launch_sched_order(hint->cost, orderBlocks, tun.schedClasses, hint->order, 1, s);
        if (le != hipSuccess) return hip_fail(le, "sched_order launch");
        hint->valid = true;
    }
    if (seconds) {
        float ms = 0.0f;
        NTR_HIP(ev.elapsed(0, 1, &ms));
        *seconds = ms * 1e-3f;
        unsigned int st = 0;
        const int rc = status_fetch(ds, s, &st);
        if (rc != NTR_OK) return rc;
        if (st & NTR_STATUS_STACK_OVERFLOW) return set_error(NTR_ERR_OVERFLOW, "trace_bvh: traversal stack overflow");
    }
    if (stats) {
        unsigned long long h[4];
        NTR_HIP(hipMemcpyAsync(h, ds->stats, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        stats->numRays = p.numRays;
        stats->numInnerVisits = (int64_t)h[0]; stats->numTriTests = (int64_t)h[1]; stats->numLeafVisits = (int64_t)h[2]; stats->numHits = (int64_t)h[3];
    }
    return NTR_OK;
}

// validate -> describe -> bind -> launch
static int32_t certain_steps_of(const Tunables& tun, bool anyHit) { return (tun.certainSteps >= 2 || (tun.certainSteps == 1 && anyHit)) ? 1 : 0; }

static int trace_impl(const char* kernelName, int32_t numRays, int32_t anyHit, const NtrRay* d_rays,
                      NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes, const void* d_triWoop,
                      int64_t triWoopBytes, const int32_t* d_triIndex, int32_t layout, uint32_t bvhFlags,
                      void* stream, float* seconds, NtrTraceStats* stats, NtrSchedHint* hint = nullptr)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    const KernelInfo* k = find_kernel(kernelName);
    if (!k) return set_error(NTR_ERR_UNKNOWN_KERNEL, "unknown kernel '%s'", kernelName ? kernelName : "(null)");
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "ntr_trace_bvh: numRays < 0");
    if (numRays == 0) return NTR_OK;  // CudaBVHTracer.cpp:92-94
    if (!d_nodes || !d_triWoop || !d_triIndex)
        return set_error(NTR_ERR_INVALID, "CudaBVHTracer: No BVH!");  // :97-98
    if (layout != k->cfg.bvhLayout)
        return set_error(NTR_ERR_LAYOUT, "CudaBVHTracer: Incorrect BVH layout!");  // :99-100
    if (!d_rays || !d_results) return set_error(NTR_ERR_INVALID, "ntr_trace_bvh: null ray/result buffer");
    // The sizes play the role of the reference's texref extents (setTexRef(..., size),
    // CudaBVHTracer.cpp:142-150); buffer descriptors address at most 4 GiB.
    int rc = check_nodes_bytes("ntr_trace_bvh", "node buffer size", nodesBytes);
    if (rc != NTR_OK) return rc;
    if (triWoopBytes < 16 || (triWoopBytes % 16) != 0 || triWoopBytes > 0xFFFFFFFFll)
        return set_error(NTR_ERR_INVALID, "ntr_trace_bvh: triWoop buffer size must be a multiple of 16 in [16, 4 GiB)");

    DeviceState* ds = nullptr;
    rc = current_device_state_ready(&ds);
    if (rc != NTR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;

    // the plan: a pure function of the tunables and the batch (trace_plan.h; ntr_trace_plan exposes it to the CPU test tier)
    const Tunables tun = tunables();
    const TraceBatchDesc bd = describe_batch(k, numRays, anyHit, (uint64_t)d_nodes, nodesBytes, (uint64_t)d_triWoop, triWoopBytes, bvhFlags,
                                             stats != nullptr, stream_is_capturing(s), hint != nullptr, ds->numCUs);
    const TracePlan pl = plan_trace(tun, bd);

    TraceLaunch L;
    TraceParams& p = L.p;   // the batch, the device's words and the plan's constants; the bind step sets counter, order, cost, pool word,
                            // shards and route skip (zero until then)
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results; p.bvhFlags = bvhFlags;
    p.nodes = d_nodes; p.woop = d_triWoop; p.triIndex = d_triIndex; p.nodesBytes = (uint32_t)nodesBytes; p.woopBytes = (uint32_t)triWoopBytes;
    p.status = ds->status; p.stats = ds->stats;
    p.numHeads = pl.numHeads; p.chunk = pl.chunk; p.fetchThreshold = pl.fetchThreshold; p.wholeWave = pl.wholeWave; p.prefetchAfter = pl.prefetchAfter;
    p.flatFetch = pl.flatFetch; p.uniformPrologue = pl.uniformPrologue; p.splitSlice = pl.splitSlice; p.leafSwitchBelow = pl.leafSwitchBelow;
    p.octant = pl.octant; p.poolKConst = pl.poolKConst;
    // (not part of the plan: it changes no launch shape)  1: any-hit launches -- short occlusion rays, where four prologue steps in five are
    // certain; the closest-hit launch of a camera batch finds one step in eight certain and lost 1 % to asking (EXPERIMENTS.md); 2: every launch
    p.certainSteps = certain_steps_of(tun, anyHit != 0);
    p.certainDescent = tun.certainDescent != 0 ? 1 : 0;
    if (stats) NTR_HIP(hipMemsetAsync(ds->stats, 0, 4 * sizeof(unsigned long long), s));

    rc = bind_trace(ds, tun, pl, bd.capturing, nodesBytes, s, hint, &L);
    if (rc != NTR_OK) return rc;
    return launch_trace(ds, tun, pl, L, s, seconds, stats);
}

}  // namespace ntr

// Tunables.  Environment overrides exist for benchmarking sweeps; they are read ONCE, when the library is first
// used (and again on ntr_tunables_reload(), which the sweep scripts call after changing a variable), never per
// launch.  No pointer is ever taken from the environment.
static int env_int(const char* name, int def)
{
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : def;
}

namespace ntr {
static Tunables g_tun;
static bool g_tunLoaded = false;
static std::mutex g_tunMu;

static void tunables_load_locked()
{
    Tunables t;
    t.chunk = env_int("NTR_TRACE_CHUNK", 64);
    t.fetchThreshold = env_int("NTR_TRACE_FETCH_THRESHOLD", -1);  // -1: 24 for kepler_dynamic_fetch, 0 otherwise
    t.leafSwitchBelow = env_int("NTR_TRACE_LEAF_SWITCH", -1);     // -1: 32 for closest-hit, 24 for any-hit launches (bench-protocol sweep, scripts/jobs/gpu_job_r02ls.sh)
    t.blocksPerCU = env_int("NTR_TRACE_BLOCKS_PER_CU", 7);          // persistent kernels: 7 x 4 waves per CU -- what 69 VGPRs let be resident (a workgroup that is not resident at launch holds its statically assigned first chunks back until another one leaves)
    t.blocksPerCUIncoherent = env_int("NTR_TRACE_BLOCKS_PER_CU_INCOHERENT", 3);   // persistent kernels, batches the device finds incoherent (scattered origins): fewer rays in flight = less queueing per step (scripts/studies/inflight_sweep.py)
    t.blocksPerCUDivergent = env_int("NTR_TRACE_BLOCKS_PER_CU_DIVERGENT", 4);     // ... batches whose rays start together and wander apart (a diffuse batch)
    t.octant = env_int("NTR_TRACE_OCTANT", 1);
    t.flatFetch = env_int("NTR_TRACE_FLAT_FETCH", 1);             // unified-step loop: one group of global loads per iteration (0 = two masked groups of range-checked buffer loads)
    t.uniformPrologue = env_int("NTR_TRACE_UNIFORM_PROLOGUE", 1);  // per-ray kernels: scalar node fetches while the lanes of a fresh wave all hold the same inner node
    t.certainSteps = env_int("NTR_TRACE_CERTAIN_STEPS", 1);   // per-ray kernels, in the uniform prologue: steps that comparisons settle for every live lane skip the exact slab test (1 = any-hit launches, 2 = every launch, 0 = off)
    t.certainDescent = env_int("NTR_TRACE_CERTAIN_DESCENT", 1);   // ... and the node stays in a scalar register from one certain step to the next while every live lane takes the same inner child (0 = every step writes the child to the lanes and the loop top reads it back)
    t.splitSlice = env_int("NTR_TRACE_SPLIT_SLICE", 8);   // persistent kernels, unified-step loop: once the pool is dry, lanes without a ray take over stack entries of the wave's live rays; looked at every N steps (0 = off)
    t.wholeWave = env_int("NTR_TRACE_WHOLE_WAVE", 1);      // kepler_dynamic_fetch: waves start in whole-wave mode and switch to single-lane refills per wave (0 = dynamic fetch from the start, as until round 5)
    t.prefetchAfter = env_int("NTR_TRACE_PREFETCH_AFTER", 8);   // persistent kernels: iterations into a chunk after which a wave posts the dequeue of its next one (-1 = never)
    t.minipool = env_int("NTR_TRACE_MINIPOOL", -1);              // closest-hit per-ray launches: rays owned by a wave / 64.  -1: decided per batch on the device (1, or minipoolWide when the prediction finds the batch incoherent); 0: the plain per-ray kernel; 1 ... 16: forced
    t.minipoolWide = env_int("NTR_TRACE_MINIPOOL_WIDE", -1);     // K of an incoherent batch: 2 / 4, or -1 = by tree size (4 from 32 MB of nodes up)
    t.minipoolThreshold = env_int("NTR_TRACE_MINIPOOL_THRESHOLD", 48);   // refill a wave's finished lanes when fewer than this many are live
    t.unified = env_int("NTR_TRACE_UNIFIED", 1);                  // kepler_dynamic_fetch: unified-step loop (0 = while-while loop + dynamic fetch)
    t.poolHeads = env_int("NTR_TRACE_POOL_HEADS", 128);           // persistent kernels: 8..1024, a multiple of 8 (sweep: scripts/studies/persist_diag.py)
    t.autoHint = env_int("NTR_TRACE_AUTO_HINT", 1);               // dispatch order learned from the previous launch of the same batch (stream, rays, count, BVH)
    t.autoHintMinRays = env_int("NTR_TRACE_AUTO_HINT_MIN_RAYS", 1 << 17);
    t.route = env_int("NTR_TRACE_ROUTE", 1);   // batches are traced by the body that is fast on them, whatever the kernel name (trace_plan.h ROUTING); 0 = the named body always
    t.persistentHints = env_int("NTR_TRACE_PERSISTENT_HINTS", 1);   // the persistent kernels honour scheduling hints too (pool handed out in the hint's order, chunk lives recorded as block costs)
    t.predict = env_int("NTR_TRACE_PREDICT", 1);
    t.predictPersistent = env_int("NTR_TRACE_PREDICT_PERSISTENT", 1);   // persistent kernels: pool in predicted-cost order (closest-hit launches of >= predictMinRays)
    t.predictDepth = env_int("NTR_TRACE_PREDICT_DEPTH", 9);
    t.predictMinRays = env_int("NTR_TRACE_PREDICT_MIN_RAYS", 1 << 20);
    t.predictMinNodes = env_int("NTR_TRACE_PREDICT_MIN_NODES", 4096);
    t.schedRefreshEvery = env_int("NTR_SCHED_REFRESH_EVERY", 16);
    t.schedClasses = env_int("NTR_SCHED_CLASSES", 32);
    t.lbvhSplit = env_int("NTR_LBVH_SPLIT", 3072);
    t.lbvhAggLds = env_int("NTR_LBVH_AGG_LDS", 1);     // bottom-up emit: meetings inside a tile through LDS
    t.lbvhSortItems = env_int("NTR_LBVH_SORT_ITEMS", 0);   // keys per thread of a one-sweep tile (8 / 16 / 24 / 32; 0 = by size)
    t.lbvhAggStaged = env_int("NTR_LBVH_AGG_STAGED", -1);  // bottom-up emit in two launches: -1 = from 2^20 triangles, 0 / 1 = never / always
    if (t.chunk < 1) t.chunk = 1;
    // a refill threshold above the wave size asks a FULL wave for a refill: the loops leave their traversal for it before any lane has
    // stepped and, with no lane free to take a ray, come straight back -- for ever (trace_kernels.hip: traverse / traverse_unified,
    // `popcount(live) < fetchThreshold` while the pool holds rays).  64 already means "refill as soon as one lane is free".
    if (t.fetchThreshold > 64) t.fetchThreshold = 64;
    if (t.minipoolThreshold > 64) t.minipoolThreshold = 64;
    if (t.blocksPerCU < 1) t.blocksPerCU = 1;   // (a persistent grid of no workgroups is no launch)
    g_tun = t;
    g_tunLoaded = true;
}

Tunables tunables()
{
    std::lock_guard<std::mutex> lk(g_tunMu);
    if (!g_tunLoaded) tunables_load_locked();
    return g_tun;
}
}  // namespace ntr

extern "C" int ntr_tunables_reload(void)
{
    std::lock_guard<std::mutex> lk(ntr::g_tunMu);
    ntr::tunables_load_locked();
    return NTR_OK;
}


using namespace ntr;

extern "C" {

const char* ntr_last_error(void) { return g_err; }
int ntr_version(void) { return 100; }

int ntr_device_count(int* count)
{
    if (!count) return set_error(NTR_ERR_INVALID, "ntr_device_count: null argument");
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; return hip_fail(e, "hipGetDeviceCount"); }
    return NTR_OK;
}

int ntr_set_device(int device) { NTR_HIP(hipSetDevice(device)); return NTR_OK; }

int ntr_malloc(void** d_ptr, size_t bytes)
{
    if (!d_ptr) return set_error(NTR_ERR_INVALID, "ntr_malloc: null argument");
    *d_ptr = nullptr;
    if (bytes == 0) return NTR_OK;
    NTR_HIP(hipMalloc(d_ptr, bytes));
    return NTR_OK;
}

int ntr_free(void* d_ptr)
{
    if (d_ptr) NTR_HIP(hipFree(d_ptr));
    return NTR_OK;
}

int ntr_memcpy_h2d(void* d, const void* h, size_t n, void* stream)
{
    if (n == 0) return NTR_OK;
    NTR_HIP(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, (hipStream_t)stream));
    NTR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return NTR_OK;
}

int ntr_memcpy_d2h(void* h, const void* d, size_t n, void* stream)
{
    if (n == 0) return NTR_OK;
    NTR_HIP(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, (hipStream_t)stream));
    NTR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return NTR_OK;
}

int ntr_memcpy_d2d(void* dst, const void* src, size_t n, void* stream)
{
    if (n == 0) return NTR_OK;
    NTR_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return NTR_OK;
}

int ntr_memset(void* d, int value, size_t n, void* stream)
{
    if (n == 0) return NTR_OK;
    NTR_HIP(hipMemsetAsync(d, value, n, (hipStream_t)stream));
    return NTR_OK;
}

int ntr_stream_synchronize(void* stream)
{
    NTR_HIP(hipStreamSynchronize((hipStream_t)stream));
    return NTR_OK;
}

int ntr_query_config(const char* kernelName, NtrKernelConfig* config)
{
    if (!config) return set_error(NTR_ERR_INVALID, "ntr_query_config: null config");
    const KernelInfo* k = find_kernel(kernelName);
    if (!k) {
        // CudaBVHTracer::setKernel leaves bvhLayout = BVHLayout_Max when queryConfig
        // does not run (CudaBVHTracer.cpp:66-71).
        config->bvhLayout = NTR_BVHLayout_Max;
        config->blockWidth = config->blockHeight = config->usePersistentThreads = 0;
        return set_error(NTR_ERR_UNKNOWN_KERNEL, "unknown kernel '%s'", kernelName ? kernelName : "(null)");
    }
    *config = k->cfg;
    return NTR_OK;
}

int ntr_trace_bvh(const char* kernelName, int32_t numRays, int32_t anyHit, const NtrRay* d_rays,
                  NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes, const void* d_triWoop,
                  int64_t triWoopBytes, const int32_t* d_triIndex, int32_t layout, uint32_t bvhFlags, void* stream,
                  float* seconds)
{
    return trace_impl(kernelName, numRays, anyHit, d_rays, d_results, d_nodes, nodesBytes, d_triWoop, triWoopBytes,
                      d_triIndex, layout, bvhFlags, stream, seconds, nullptr);
}

int ntr_trace_bvh_hinted(const char* kernelName, int32_t numRays, int32_t anyHit, const NtrRay* d_rays,
                         NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes, const void* d_triWoop,
                         int64_t triWoopBytes, const int32_t* d_triIndex, int32_t layout, uint32_t bvhFlags, void* stream,
                         float* seconds, NtrSchedHint* hint)
{
    return trace_impl(kernelName, numRays, anyHit, d_rays, d_results, d_nodes, nodesBytes, d_triWoop, triWoopBytes,
                      d_triIndex, layout, bvhFlags, stream, seconds, nullptr, hint);
}

int ntr_trace_plan(const char* kernelName, int32_t numRays, int32_t anyHit, uint64_t nodesAddr, int64_t nodesBytes, uint64_t triWoopAddr,
                   int64_t triWoopBytes, uint32_t bvhFlags, int32_t numCUs, int32_t flags, NtrTracePlan* plan)
{
    if (!plan) return set_error(NTR_ERR_INVALID, "ntr_trace_plan: null plan");
    memset(plan, 0, sizeof(*plan));
    const KernelInfo* k = find_kernel(kernelName);
    if (!k) return set_error(NTR_ERR_UNKNOWN_KERNEL, "unknown kernel '%s'", kernelName ? kernelName : "(null)");
    if (numRays < 0 || numCUs < 1 || nodesBytes < 0 || triWoopBytes < 0) return set_error(NTR_ERR_INVALID, "ntr_trace_plan: bad argument");
    const TraceBatchDesc bd = describe_batch(k, numRays, anyHit, nodesAddr, nodesBytes, triWoopAddr, triWoopBytes, bvhFlags,
                                             (flags & NTR_PLAN_FLAG_STATS) != 0, (flags & NTR_PLAN_FLAG_CAPTURING) != 0,
                                             (flags & NTR_PLAN_FLAG_CALLER_HINT) != 0, numCUs);
    *plan = plan_trace(tunables(), bd);
    return NTR_OK;
}

int ntr_trace_plan_certain(int32_t anyHit, int32_t out[2])
{
    if (!out) return set_error(NTR_ERR_INVALID, "ntr_trace_plan_certain: null argument");
    const Tunables tun = tunables();
    out[0] = certain_steps_of(tun, anyHit != 0); out[1] = tun.certainDescent != 0 ? 1 : 0;
    return NTR_OK;
}

int ntr_trace_plan_hint_step(int32_t valid, int32_t predicted, int32_t uses, int32_t out[3])
{
    if (!out || uses < 0) return set_error(NTR_ERR_INVALID, "ntr_trace_plan_hint_step: bad argument");
    const HintStep h = plan_hint_step(tunables(), valid != 0, predicted != 0, uses);
    out[0] = h.zeroK; out[1] = h.refresh; out[2] = h.useOrder;
    return NTR_OK;
}

int ntr_trace_status(void* stream, uint32_t* statusBits)
{
    if (statusBits) *statusBits = 0;
    unsigned int st = 0;
    DeviceState* ds = nullptr;
    int rc = current_device_state_ready(&ds);
    if (rc == NTR_OK) rc = status_fetch(ds, (hipStream_t)stream, &st);
    if (rc != NTR_OK) return rc;
    if (statusBits) *statusBits = st;
    if (st & NTR_STATUS_STACK_OVERFLOW)
        return set_error(NTR_ERR_OVERFLOW, "trace_bvh: traversal stack overflow in a launch since the last status check");
    return NTR_OK;
}

// The current device's top-of-tree table for the node buffer of a prediction query (`fn` names the query in messages).
static int query_table(const char* fn, const void* d_nodes, int64_t nodesBytes, hipStream_t s, DeviceState** ds, TopTable** t)
{
    int rc = check_nodes_bytes(fn, "node buffer size", nodesBytes);
    if (rc == NTR_OK) rc = current_device_state(ds, "hipGetDevice(&dev)");
    if (rc == NTR_OK) rc = top_table_get(*ds, d_nodes, nodesBytes, s, false, t);
    return rc;
}

int ntr_predict_block_costs(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes, uint32_t* d_blockCost, void* stream)
{
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "ntr_predict_block_costs: numRays < 0");
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_nodes || !d_blockCost) return set_error(NTR_ERR_INVALID, "ntr_predict_block_costs: null argument");
    DeviceState* ds = nullptr;
    TopTable* t = nullptr;
    const int rc = query_table("ntr_predict_block_costs", d_nodes, nodesBytes, (hipStream_t)stream, &ds, &t);
    if (rc != NTR_OK) return rc;
    const hipError_t e = ntr_launch_predict_costs(d_rays, numRays, (numRays + 255) / 256, t->table, t->count, d_blockCost, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "predict_costs launch");
    return NTR_OK;
}

int ntr_predict_batch_coherence(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes, uint32_t* d_out, void* stream)
{
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "ntr_predict_batch_coherence: numRays < 0");
    if (!d_out) return set_error(NTR_ERR_INVALID, "ntr_predict_batch_coherence: null argument");
    if (numRays > 0 && (!d_rays || !d_nodes)) return set_error(NTR_ERR_INVALID, "ntr_predict_batch_coherence: null argument");
    if (numRays == 0) {   // nothing to look at: {0, 0, K = 1} without touching the node buffer
        const unsigned int none[3] = {0u, 0u, 1u};
        NTR_HIP(hipMemcpyAsync(d_out, none, sizeof(none), hipMemcpyHostToDevice, (hipStream_t)stream));
        NTR_HIP(hipStreamSynchronize((hipStream_t)stream));
        return NTR_OK;
    }
    DeviceState* ds = nullptr;
    TopTable* t = nullptr;
    const int rc = query_table("ntr_predict_batch_coherence", d_nodes, nodesBytes, (hipStream_t)stream, &ds, &t);
    if (rc != NTR_OK) return rc;
    const hipError_t e = ntr_launch_coherence(d_rays, numRays, (numRays + 255) / 256, t->table, t->count, d_out, minipool_wide(tunables(), nodesBytes, numRays),
                                              (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "coherence launch");
    return NTR_OK;
}

int ntr_predict_dispatch_order(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes, uint32_t* d_order, uint32_t* d_word,
                               void* stream)
{
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "ntr_predict_dispatch_order: numRays < 0");
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_nodes || !d_order || !d_word) return set_error(NTR_ERR_INVALID, "ntr_predict_dispatch_order: null argument");
    hipStream_t s = (hipStream_t)stream;
    DeviceState* ds = nullptr;
    TopTable* t = nullptr;
    int rc = query_table("ntr_predict_dispatch_order", d_nodes, nodesBytes, s, &ds, &t);
    if (rc != NTR_OK) return rc;
    // the device's scratch for this query (never a launch's): held until the launches that use it have run
    std::lock_guard<std::mutex> lk(ds->queryMu);
    const int numBlocks = (numRays + 255) / 256;
    PredictScratch* p = &ds->query;
    if (p->capBlocks < numBlocks && p->classList) NTR_HIP(hipStreamSynchronize(s));
    rc = scratch_alloc(p, numBlocks);
    if (rc != NTR_OK) return rc;
    const hipError_t e = ntr_launch_predict(d_rays, numRays, numBlocks, t->table, t->count, p->classCount, p->classList, d_order, d_word,
                                            minipool_wide(tunables(), nodesBytes, numRays), s);
    if (e != hipSuccess) return hip_fail(e, "predict launch");
    NTR_HIP(hipStreamSynchronize(s));
    return NTR_OK;
}

int ntr_secondary_block_costs(const NtrRayResult* d_inResults, int32_t first, int32_t count, int32_t numSamples, const int32_t* d_depthByTri,
                              int32_t numTris, uint32_t* d_blockCost, void* stream)
{
    if (first < 0 || count < 0 || numSamples < 1 || numTris < 0 || (count > 0 && (!d_inResults || !d_depthByTri || !d_blockCost)))
        return set_error(NTR_ERR_INVALID, "ntr_secondary_block_costs: bad argument");
    if (count == 0) return NTR_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = ((int64_t)count * numSamples + 255) / 256;
    if (blocks > 0x7FFFFFFF) return set_error(NTR_ERR_INVALID, "ntr_secondary_block_costs: batch too large");
    hipError_t e = ntr_launch_zero_words(d_blockCost, (int)blocks, s);
    if (e == hipSuccess) e = ntr_launch_secondary_block_costs(d_inResults, first, count, numSamples, d_depthByTri, numTris, d_blockCost, s);
    if (e != hipSuccess) return hip_fail(e, "secondary_block_costs launch");
    return NTR_OK;
}

int ntr_bvh_leaf_depths(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                        int32_t numTris, int32_t* d_depthByTri, int32_t* maxDepth, void* stream)
{
    if (maxDepth) *maxDepth = 0;
    if (!d_nodes || nodesBytes < 64 || (nodesBytes % 64) != 0 || nodesBytes > kMaxNodesBytes || !d_triWoop || triWoopBytes < 16 || !d_triIndex ||
        numTris < 1 || !d_depthByTri)
        return set_error(NTR_ERR_INVALID, "ntr_bvh_leaf_depths: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const unsigned int capacity = (unsigned int)(nodesBytes / 64);
    // two frontier queues + their counters (counter k of level L at counts[L & 1]; cleared before it is filled)
    unsigned int* d_q = nullptr;
    NTR_HIP(hipMalloc((void**)&d_q, (2 * (size_t)capacity + 2) * sizeof(unsigned int)));
    unsigned int* q[2] = {d_q, d_q + capacity};
    unsigned int* cnt = d_q + 2 * (size_t)capacity;
    hipError_t e = hipMemsetAsync(d_depthByTri, 0, (size_t)numTris * sizeof(int32_t), s);
    const unsigned int init[3] = {0u, 1u, 0u};   // q[0][0] = root offset 0; counts = {1, 0}
    if (e == hipSuccess) e = hipMemcpyAsync(q[0], &init[0], sizeof(unsigned int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, &init[1], 2 * sizeof(unsigned int), hipMemcpyHostToDevice, s);
    int depth = 0;
    unsigned long long bound = 1;   // the frontier of level L holds at most min(2^L, capacity) nodes
    unsigned int frontier = 1;
    while (e == hipSuccess && frontier > 0 && depth < 4096) {
        const int in = depth & 1, out = in ^ 1;
        e = ntr_launch_zero_words(cnt + out, 1, s);
        const unsigned int threads = (unsigned int)(bound < capacity ? bound : capacity);
        if (e == hipSuccess)
            e = ntr_launch_leaf_depth_level(d_nodes, (unsigned int)nodesBytes, d_triWoop, (unsigned int)(triWoopBytes / 16), d_triIndex, numTris, q[in], cnt + in,
                                            q[out], cnt + out, capacity, threads, depth, d_depthByTri, s);
        depth++;
        bound = bound < capacity ? bound * 2 : bound;
        if ((depth & 3) == 0 && e == hipSuccess) {   // every fourth level: has the frontier run empty?
            e = hipMemcpyAsync(&frontier, cnt + (depth & 1), sizeof(frontier), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (frontier > capacity) frontier = capacity;
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_q);
    if (e != hipSuccess) return hip_fail(e, "ntr_bvh_leaf_depths");
    if (depth >= 4096) return set_error(NTR_ERR_INVALID, "ntr_bvh_leaf_depths: the tree is deeper than 4096 levels (a cycle in the child references?)");
    if (maxDepth) *maxDepth = depth;
    return NTR_OK;
}

int ntr_trace_bvh_stats(const char* kernelName, int32_t numRays, int32_t anyHit, const NtrRay* d_rays,
                        NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes, const void* d_triWoop,
                        int64_t triWoopBytes, const int32_t* d_triIndex, int32_t layout, uint32_t bvhFlags,
                        void* stream, NtrTraceStats* stats)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_bvh_stats: null stats");
    return trace_impl(kernelName, numRays, anyHit, d_rays, d_results, d_nodes, nodesBytes, d_triWoop, triWoopBytes,
                      d_triIndex, layout, bvhFlags, stream, nullptr, stats);
}

int ntr_selftest_division(const float* d_x, int32_t nx, const float* d_d, int32_t nd, uint32_t* mismatches, void* stream)
{
    if (!mismatches || !d_x || !d_d || nx <= 0 || nd <= 0) return set_error(NTR_ERR_INVALID, "ntr_selftest_division: bad argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned int* d_m = nullptr;
    NTR_HIP(hipMalloc((void**)&d_m, sizeof(unsigned int)));
    NTR_HIP(hipMemsetAsync(d_m, 0, sizeof(unsigned int), s));
    hipError_t le = ntr_launch_selftest_division(d_x, d_d, nx, nd, d_m, s);
    if (le != hipSuccess) return hip_fail(le, "selftest launch");
    unsigned int m = 0;
    NTR_HIP(hipMemcpyAsync(&m, d_m, sizeof(m), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    NTR_HIP(hipFree(d_m));
    *mismatches = m;
    return NTR_OK;
}

int ntr_selftest_ray_class(const NtrRay* d_rays, int32_t numRays, uint32_t bvhFlags, uint32_t* mismatches, void* stream)
{
    if (!mismatches || !d_rays || numRays <= 0) return set_error(NTR_ERR_INVALID, "ntr_selftest_ray_class: bad argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned int* d_m = nullptr;
    NTR_HIP(hipMalloc((void**)&d_m, sizeof(unsigned int)));
    hipError_t e = hipMemsetAsync(d_m, 0, sizeof(unsigned int), s);
    if (e == hipSuccess) e = ntr_launch_selftest_ray_class(d_rays, numRays, bvhFlags, d_m, s);
    unsigned int m = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&m, d_m, sizeof(m), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_m);
    if (e != hipSuccess) return hip_fail(e, "ntr_selftest_ray_class");
    *mismatches = m;
    return NTR_OK;
}

int ntr_selftest_division_hard(int32_t xExp, int32_t dExp, uint64_t* pairs, uint64_t* mismatches, void* stream)
{
    // FASTDIV range of the operands the kernel forms (x = X 2^(xExp .. xExp + 3 - 23), d = D 2^(dExp .. dExp + 3 - 23), X, D in [2^23, 2^24))
    if (!pairs || !mismatches || xExp < -84 || xExp > 51 || dExp < -40 || dExp > 16)
        return set_error(NTR_ERR_INVALID, "ntr_selftest_division_hard: bad argument (x exponents in [-84, 51], d exponents in [-40, 16])");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d_c = nullptr;
    NTR_HIP(hipMalloc((void**)&d_c, 2 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_c, 0, 2 * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = ntr_launch_selftest_division_hard(xExp, dExp, d_c, s);
    unsigned long long h[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_c, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_c);
    if (e != hipSuccess) return hip_fail(e, "ntr_selftest_division_hard");
    *pairs = h[0];
    *mismatches = h[1];
    return NTR_OK;
}

// ---- self tests of the shared device toolkit (selftest_prims_kernels.hip): the argument checks ----
int ntr_selftest_onesweep(int32_t items, int32_t mode, int32_t skipTrivial, int32_t n, const uint32_t* d_keys, int32_t stride, const int32_t* d_vals,
                          int32_t numPasses, const int32_t* passes, int32_t forceTicket, uint32_t* d_keysOut, int32_t* d_valsOut, uint32_t* errWord,
                          void* stream)
{
    if (!selftest_onesweep_offered(items, mode, skipTrivial))
        return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: no user launches onesweep_pass_kernel<%d, %d, %d>", items, mode, skipTrivial);
    if (n < 1 || n >= (1 << 28)) return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: n must be in [1, 2^28)");
    if (!d_keys || !d_keysOut || !d_valsOut || !errWord || !passes || (mode == 2 && !d_vals))
        return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: null argument");
    if (mode == 0 ? stride != 1 : (stride != 1 && stride != 6)) return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: stride must be 1 (mode 2: 1 or 6)");
    if (numPasses < 1 || numPasses > kSelftestMaxPasses) return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: 1 to %d passes", kSelftestMaxPasses);
    for (int p = 0; p < numPasses; p++) {
        if (passes[2 * p] < 0 || passes[2 * p] > 24) return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: shift %d outside [0, 24]", passes[2 * p]);
        if (passes[2 * p + 1] < 0 || passes[2 * p + 1] > kSelftestMaxPassNumber)
            return set_error(NTR_ERR_INVALID, "ntr_selftest_onesweep: pass number %d outside [0, %d]", passes[2 * p + 1], kSelftestMaxPassNumber);
    }
    *errWord = 0;
    return selftest_onesweep_run(items, mode, skipTrivial, n, d_keys, stride, d_vals, numPasses, passes, forceTicket, d_keysOut, d_valsOut, errWord,
                                 (hipStream_t)stream);
}

int ntr_selftest_scan(int32_t type, int32_t threads, int32_t n, const void* d_in, void* d_prefix, void* total, void* stream)
{
    if (type < NTR_SCAN_U32 || type > NTR_SCAN_U4 || (threads != 256 && threads != 1024) || n < 1 || n >= (1 << 28) || !d_in || !d_prefix || !total)
        return set_error(NTR_ERR_INVALID, "ntr_selftest_scan: bad argument");
    return selftest_scan_run(type, threads, n, d_in, d_prefix, total, (hipStream_t)stream);
}

int ntr_selftest_scan_block_sums(int32_t type, int32_t threads, int32_t nb, const void* d_in, void* d_out, void* total, void* stream)
{
    if (type < NTR_SCAN_U32 || type > NTR_SCAN_U4 || (threads != 256 && threads != 1024) || nb < 0 || nb >= (1 << 28) || (nb > 0 && (!d_in || !d_out)))
        return set_error(NTR_ERR_INVALID, "ntr_selftest_scan_block_sums: bad argument");
    return selftest_block_sums_run(type, threads, nb, d_in, d_out, total, (hipStream_t)stream);
}

int ntr_selftest_float_order(int32_t n, const uint32_t* d_words, uint32_t* d_single, uint32_t* d_pairs, void* stream)
{
    if (n < 1 || n > 2048 || !d_words || !d_single || !d_pairs) return set_error(NTR_ERR_INVALID, "ntr_selftest_float_order: bad argument (1 to 2048 words)");
    return selftest_float_order_run(n, d_words, d_single, d_pairs, (hipStream_t)stream);
}

int ntr_selftest_box_words(int32_t m, const float* d_boxes, const int32_t* d_group, int32_t groups, float eps, const uint32_t* d_lane32,
                           const uint64_t* d_lane64, uint32_t* d_groupsOut, uint32_t* d_foldsOut, void* stream)
{
    if (m < 64 || (m & 63) || m > (1 << 24) || groups < 1 || groups > (1 << 20) || !d_boxes || !d_group || !d_lane32 || !d_lane64 || !d_groupsOut || !d_foldsOut)
        return set_error(NTR_ERR_INVALID, "ntr_selftest_box_words: bad argument (whole waves: m a multiple of 64)");
    return selftest_box_words_run(m, d_boxes, d_group, groups, eps, d_lane32, d_lane64, d_groupsOut, d_foldsOut, (hipStream_t)stream);
}

}  // extern "C"
