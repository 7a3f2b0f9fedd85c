/*
 * ntrace_amd.h -- C-ABI of the MI355X-native NTrace tracer backend (libntrace_amd.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point cites the reference interface it replaces (paths relative to
 * the NTrace checkout).  The reference-side binding is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns NTR_OK (0) or a negative NtrStatus; the message of
 *     the last failure on the calling thread is ntr_last_error().  The C++ host
 *     mirror (ntrace_amd/host) maps non-zero to FW::fail(), as the reference's
 *     CudaModule::checkError does (src/framework/gpu/CudaModule.cpp).
 *   - "d_" pointers are device (HIP) pointers owned by the caller (Buffer in the
 *     reference, src/framework/gpu/Buffer.hpp:107-113); the library never frees
 *     or retains them past the call (or past stream completion for async calls).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - calls are thread-compatible: one caller per device at a time.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry
 *     point fails with NTR_ERR_NO_DEVICE.
 */
#ifndef NTRACE_AMD_H
#define NTRACE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTR_API __attribute__((visibility("default")))

typedef enum NtrStatus {
    NTR_OK = 0,
    NTR_ERR_INVALID = -1,     /* bad argument                                  */
    NTR_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at init   */
    NTR_ERR_HIP = -3,         /* a HIP call failed (message has the HIP error) */
    NTR_ERR_LAYOUT = -4,      /* "CudaBVHTracer: Incorrect BVH layout!"        */
    NTR_ERR_UNKNOWN_KERNEL = -5,
    NTR_ERR_OVERFLOW = -6,    /* traversal stack / workspace overflow          */
    NTR_ERR_NOMEM = -7
} NtrStatus;

/* src/rt/kernels/CudaTracerKernels.hpp:52-63 */
typedef enum NtrBVHLayout {
    NTR_BVHLayout_AOS_AOS = 0,
    NTR_BVHLayout_AOS_SOA,
    NTR_BVHLayout_SOA_AOS,
    NTR_BVHLayout_SOA_SOA,
    NTR_BVHLayout_Compact,
    NTR_BVHLayout_Compact2,
    NTR_BVHLayout_CPU,
    NTR_BVHLayout_Max
} NtrBVHLayout;

/* src/rt/kernels/CudaTracerKernels.hpp:69-75 (KernelConfig) */
typedef struct NtrKernelConfig {
    int32_t bvhLayout;
    int32_t blockWidth;            /* wave64: 64                           */
    int32_t blockHeight;           /* waves per workgroup                  */
    int32_t usePersistentThreads;
} NtrKernelConfig;

/* src/rt/Util.hpp:62-71 */
typedef struct NtrRay {
    float ox, oy, oz, tmin;
    float dx, dy, dz, tmax;
} NtrRay;

/* src/rt/Util.hpp:77-87.  The tracer writes id and t; padA/padB receive the
 * barycentrics (u,v) bit patterns on a hit like STORE_RESULT
 * (CudaTracerKernels.hpp:222) and are 0 on a miss.  Parity is on (id,t). */
typedef struct NtrRayResult {
    int32_t id;
    float   t;
    int32_t padA;
    int32_t padB;
} NtrRayResult;

/* ---- library / device ------------------------------------------------------ */

NTR_API const char* ntr_last_error(void);
NTR_API int         ntr_version(void);

/* Thin device-memory plumbing for the C++ Buffer mirror
 * (src/framework/gpu/Buffer.cpp:238- cuMemAlloc/cuMemcpy* call sites). */
NTR_API int ntr_device_count(int* count);
NTR_API int ntr_set_device(int device);
NTR_API int ntr_malloc(void** d_ptr, size_t bytes);
NTR_API int ntr_free(void* d_ptr);
NTR_API int ntr_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
NTR_API int ntr_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
NTR_API int ntr_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
NTR_API int ntr_memset(void* d_dst, int value, size_t bytes, void* stream);
NTR_API int ntr_stream_synchronize(void* stream);

/* ---- tracer ---------------------------------------------------------------- */

/* Replaces the per-kernel-file `queryConfig` launch + g_config read-back
 * (src/rt/cuda/CudaBVHTracer.cpp:52-84).  `kernelName` keeps the reference's
 * file-name selectors: "fermi_speculative_while_while",
 * "tesla_persistent_while_while", "tesla_persistent_speculative_while_while",
 * "kepler_dynamic_fetch" (all mapped to precompiled CDNA4 variants).
 *
 * The answer describes the NAMED body (per-ray kernel: 64-thread workgroups, not persistent; tesla_* / kepler_*: persistent waves in
 * 256-thread workgroups) and every name consumes BVHLayout_Compact.  A name selects semantics, and the semantics of all names are
 * identical here (same hit records, bit for bit); which body actually traces a batch follows the batch (csrc/trace_plan.h ROUTING):
 * any-hit launches run the per-ray body under every name, closest-hit launches of >= 2^20 rays are launched as both bodies and the
 * device's batch word (ntr_predict_batch_coherence) decides which one works -- the per-ray body on coherent batches, the persistent
 * dynamic-fetch body on incoherent ones --, smaller launches run the named body.  NTR_TRACE_ROUTE=0 (environment, read once) forces
 * the named body always; ntr_trace_plan() reports the decision for a given batch. */
NTR_API int ntr_query_config(const char* kernelName, NtrKernelConfig* config);

/* Replaces the `trace_bvh` launch of CudaBVHTracer::traceBatch
 * (src/rt/cuda/CudaBVHTracer.cpp:88-168; signature TRACE_FUNC_BVH,
 * src/rt/kernels/CudaTracerKernels.hpp:99-112; nodesB-D / trisB-C exist only for
 * the SOA layouts and are dropped).
 *
 *   numRays == 0          -> NTR_OK, *seconds = 0 (CudaBVHTracer.cpp:92-94)
 *   layout != the kernel's desired layout -> NTR_ERR_LAYOUT (:99-100)
 *   seconds != NULL       -> launch is bracketed by HIP events on `stream`, the
 *                            call blocks and returns the kernel's GPU time in
 *                            seconds (CudaKernel::launchTimed, CudaKernel.cpp:188-221)
 *   seconds == NULL       -> asynchronous launch on `stream`.
 *
 * nodesBytes / triWoopBytes are the buffer extents the reference binds as texture sizes
 * (setTexRef(..., size), CudaBVHTracer.cpp:142-150); here they bound the kernels' buffer
 * descriptors: triWoopBytes < 4 GiB; nodesBytes <= 0x76543200, because Compact child pointers are signed
 * 32-bit byte offsets and 0x76543210 is the traversal sentinel (EntrypointSentinel, CudaTracerKernels.hpp:38).
 *
 * Results follow the reference CPU tracer bit for bit in (id, t): miss =
 * (-1, ray.tmax) (CudaBVH.cpp:273-274).  `bvhFlags`: 0, or hints from
 * ntr_bvh_validate() (hints only select between two exact code paths).
 *
 * Closest-hit launches of the per-ray kernel with at least 2^20 rays dispatch their 256-ray blocks in
 * predicted-cost order (two small launches in front of the trace kernel, inside the timed bracket; the
 * order never changes a result; NTR_TRACE_PREDICT=0 disables it).  Launches of
 * "kepler_dynamic_fetch" end with ray splitting: once the ray pool is dry, lanes without a ray traverse
 * stack entries of the wave's live rays, and a helper's result counts only where it provably is the
 * result the ray alone would have computed (csrc/trace_split.h; NTR_TRACE_SPLIT_SLICE=0 disables it) --
 * records are the reference CPU tracer's either way.  An asynchronous call can be captured
 * into a HIP graph and replayed once a first call on that stream has allocated its scratch buffers. */
NTR_API int ntr_trace_bvh(const char* kernelName, int32_t numRays, int32_t anyHit,
                          const NtrRay* d_rays, NtrRayResult* d_results,
                          const void* d_nodes, int64_t nodesBytes,
                          const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                          int32_t layout, uint32_t bvhFlags, void* stream, float* seconds);

/* Device status of the launches made since the last check, for callers of the ASYNCHRONOUS form
 * (seconds == NULL), which cannot report it themselves.  The reference's launches are synchronous and its
 * kernels silently assume a 64-entry stack (STACK_SIZE, CudaTracerKernels.hpp:37); here a ray whose
 * traversal stack would exceed 104 entries (LDS + scratch, more than the CPU tracer's 100, CudaBVH.cpp:701)
 * sets a sticky bit in a per-device status word instead of corrupting memory -- its hit record is then not
 * to be trusted.  ntr_trace_status waits for `stream`, returns the word in *statusBits (may be NULL), clears
 * it, and returns NTR_ERR_OVERFLOW if the overflow bit was set (bit 0), NTR_OK otherwise.  Timed calls
 * (seconds != NULL) perform the same check themselves.  The word is shared by all streams of the device. */
NTR_API int ntr_trace_status(void* stream, uint32_t* statusBits);

/* Measurement aid (bench.py extras.gather_roof; no counterpart in the reference): every one of `waves` x `lanesPerWave` lanes walks
 * a dependent chain of `steps` random 64-byte records of a `tableBytes` table (four 16-byte loads per record, the next index a hash of
 * the bytes just loaded) -- the memory side of a divergent traversal without its arithmetic.  *seconds = best of three launches;
 * waves x lanesPerWave x steps / seconds is the record rate.  On a table larger than the Infinity Cache with a full grid this is the
 * practical roof of an HBM-resident BVH's fetches (56 G records/s = 3.6 TB/s on MI355X, whatever the record size: DESIGN.md 4.1). */
NTR_API int ntr_selftest_gather_rate(int64_t tableBytes, int32_t waves, int32_t lanesPerWave, int32_t steps, void* stream, float* seconds);

/* HIP graphs.  An asynchronous ntr_trace_bvh (seconds == NULL) may be captured into a HIP graph.  Nothing can be allocated
 * during a capture, and the scratch of a captured launch must outlive the graph, so the library hands such a launch scratch
 * of its OWN from per-device stores that are filled outside captures and never recycled while pinned:
 *   - pool counters of the persistent kernels: 192 captured launches per device;
 *   - dispatch-order prediction scratch (closest-hit per-ray launches of >= 2^20 rays): private to each captured launch
 *     (a replay on any stream never shares it with a live launch); every live launch of a size keeps 4 spares of that size
 *     ready, ntr_trace_graph_reserve(launches, numRays) provisions more (48 entries per device in all);
 *   - the top-of-tree table of a BVH (16 BVHs per device): trace the BVH once, or call ntr_bvh_validate, before capturing.
 * The predicted order is an optimisation: a captured launch that finds no spare scratch is captured in buffer order
 * (no error).
 * When one of the other stores is exhausted the capture-time call fails with NTR_ERR_NOMEM / NTR_ERR_INVALID and says so.  A host that
 * re-captures graphs (e.g. every frame) calls ntr_trace_graph_release_all() once the graphs holding earlier captures are
 * destroyed: it waits for the device and returns every pinned resource of the current device to its store. */
NTR_API int ntr_trace_graph_reserve(int32_t launches, int32_t numRays);
NTR_API int ntr_trace_graph_release_all(void);

/* Scheduling state is kept PER DEVICE (one mutex, 96 automatic hints, 48 prediction scratches, 16 top-of-tree tables each), so the
 * host threads of a thread-per-GPU driver (ntr_dist_init_all) neither share entries nor contend for one lock.  Within a device an
 * entry belongs to the stream that created it and is recycled only by that stream (the launch path never synchronises or records an
 * event).  ntr_stream_release(stream): call before destroying a stream -- waits for it and returns the automatic hints and the
 * prediction scratch it owns on the current device.  Without it the entries of dead streams stay allocated for the life of the
 * process; a device whose 96 hint entries all belong to dead streams gives later streams buffer / predicted order only (about
 * 9 % on re-traced batches), never an error. */
NTR_API int ntr_stream_release(void* stream);

/* CPU-side self test of the automatic-hint table (no device needed): `devices` simulated devices each trace `keysPerDevice` distinct
 * batches on a stream of their own, `rounds` times; hintedLastRound[d] = batches of device d that found their hint entry in the
 * last round (keysPerDevice for every device while keysPerDevice <= 96: no device is starved by the others). */
NTR_API int ntr_selftest_auto_hint_table(int32_t devices, int32_t keysPerDevice, int32_t rounds, int32_t* hintedLastRound);

/* The PLAN of a trace launch (diagnostic; no device needed): everything ntr_trace_bvh decides from the tunables, the kernel name and the
 * batch's sizes and flags alone -- which kernel variant, how many workgroups, which loop, pool geometry, and which scheduling aids
 * (automatic hint, dispatch-order prediction, pool depth decided on the device) the launch will ask for.  ntr_trace_bvh computes exactly
 * this (csrc/trace_plan.h) before it touches the device; what depends on run-time state (which hint entry, which prediction scratch)
 * is not part of it.  No counterpart in the reference (CudaBVHTracer::traceBatch sizes its grid inline, CudaBVHTracer.cpp:152-160). */
typedef struct NtrTracePlan {
    int32_t variant;            /* NTR_VARIANT_* after the stats override (csrc/trace_kernels.h) */
    int32_t launchVariant;      /* the kernel that is launched */
    int32_t launchBlocks;       /* its workgroups */
    int32_t numBlocks;          /* per-ray kernels: 256-ray blocks (unit of dispatch order and cost feedback); persistent: the grid */
    int32_t orderBlocks;        /* 256-ray blocks of the batch */
    int32_t chunk, fetchThreshold, leafSwitchBelow, octant, flatFetch, uniformPrologue, splitSlice;
    int32_t numHeads, shardRays, numBlocksIncoherent;   /* persistent kernels: pool heads, rays per head, grid of an incoherent batch */
    int32_t numBlocksDivergent; /* ... of a batch whose rays start together and wander apart (NTR_BATCH_DIVERGENT only) */
    int32_t wholeWave;          /* persistent, dynamic fetch: waves start in whole-wave mode and switch per wave (csrc/trace_kernels.hip) */
    int32_t prefetchAfter;      /* persistent: iterations into a chunk after which a wave posts the dequeue of its next one (< 0: never) */
    int32_t unified;            /* persistent: unified-step loop (kepler_dynamic_fetch) */
    int32_t minipool;           /* closest-hit per-ray launch that may run as wave-private ray pools */
    int32_t poolKConst;         /* pool depth when it is not decided on the device */
    int32_t poolKFromDevice;    /* it is: the prediction of this launch, or the batch's hint, holds K */
    int32_t minipoolWide;       /* K of a batch the device finds incoherent */
    int32_t hintable;           /* the variant honours a scheduling hint */
    int32_t useAutoHint;        /* the batch is looked up in the library's own hint table */
    int32_t predictable;        /* dispatch-order prediction applies when no measured order is at hand */
    int32_t persistentOrder;    /* ... for a persistent launch: the pool is handed out in predicted order */
    int32_t probeOnRefresh;     /* a hinted batch's pool depth is estimated again on the hint's refresh launches */
    int32_t coherentRoute;      /* routing by coherence (ntr_query_config): 0 = the named body; 1 = BOTH bodies are launched and the device's
                                 * batch word decides which one works (closest-hit launches large enough for the estimate); 2 = the per-ray
                                 * body under a persistent name (any-hit launches) */
    int32_t persistentVariant, persistentBlocks, persistentFetchThreshold;   /* the persistent side of a launch (named, or routed) */
    int32_t perrayBlocks, perrayFetchThreshold;                              /* the per-ray side of a routed launch */
} NtrTracePlan;
#define NTR_PLAN_FLAG_STATS 1        /* ntr_trace_bvh_stats */
#define NTR_PLAN_FLAG_CAPTURING 2    /* the stream is being captured into a HIP graph */
#define NTR_PLAN_FLAG_CALLER_HINT 4  /* the caller passes an NtrSchedHint */
NTR_API int ntr_trace_plan(const char* kernelName, int32_t numRays, int32_t anyHit, uint64_t nodesAddr, int64_t nodesBytes,
                           uint64_t triWoopAddr, int64_t triWoopBytes, uint32_t bvhFlags, int32_t numCUs, int32_t flags,
                           NtrTracePlan* plan);
/* One launch in the life of a scheduling hint: out[0] = the hint's pool-depth words are cleared, out[1] = the launch records per-block
 * costs (refresh), out[2] = the launch is dispatched in the hint's order. */
NTR_API int ntr_trace_plan_hint_step(int32_t valid, int32_t predicted, int32_t uses, int32_t out[3]);
/* The two per-launch switches of the per-ray kernels' prologue that change no launch shape and so are not part of NtrTracePlan:
 * out[0] = a closest-hit (anyHit = 0) or any-hit launch takes certain steps (NTR_TRACE_CERTAIN_STEPS), out[1] = ... and keeps the node in a
 * scalar register through a run of them (NTR_TRACE_CERTAIN_DESCENT). */
NTR_API int ntr_trace_plan_certain(int32_t anyHit, int32_t out[2]);

/* Re-reads the NTR_* environment tunables.  They are read once, at first use; sweep scripts
 * that change a variable inside one process call this afterwards.  Not needed by applications. */
NTR_API int ntr_tunables_reload(void);

/* Scheduling hint (no counterpart in the reference; its kernels take rays in buffer order).
 *
 * The per-ray kernel's launch time is set by where the long-lived waves start: blocks of 256 rays
 * that traverse deep geometry live several times longer than the average block, and when they start
 * late they are the tail of the launch.  A hint object remembers, per block, how long its slowest
 * wave lived in the previous trace of the SAME logical batch (the benchmark protocol traces every
 * batch 1 + warmup + measure times, App.cpp:955-958; an interactive renderer traces nearly the same
 * rays frame after frame) and makes the next launch start the heaviest cost classes first.  Only the
 * ORDER in which blocks are dispatched changes: every ray is traced exactly as without a hint and
 * the hit records are identical.  A hint made for other rays is harmless (any order is valid); it
 * adapts after a launch or two.  The caller owns the hint and passes one per logical batch; it is
 * bound to the first (numRays) it is used with and re-initialises itself when that changes.
 * The persistent kernels honour a hint too (round 6): their pool is handed out in the hint's order and whole-wave chunks record
 * their lives as block costs.  ONE STREAM AT A TIME: a hint's arrays are read by the launches it was passed to and rewritten when it is
 * rebound (another ray count) or refreshed; use a hint on one stream only, or synchronise that stream before passing the hint to a
 * launch on another (the launch path itself never synchronises or records events: ADVICE r05). */
typedef struct NtrSchedHint NtrSchedHint;
NTR_API int ntr_sched_hint_create(NtrSchedHint** out);
NTR_API int ntr_sched_hint_destroy(NtrSchedHint* hint);
/* Forget what was measured (e.g. after a camera cut). */
NTR_API int ntr_sched_hint_reset(NtrSchedHint* hint);
/* ntr_trace_bvh with a scheduling hint (hint == NULL: identical to ntr_trace_bvh). */
NTR_API int ntr_trace_bvh_hinted(const char* kernelName, int32_t numRays, int32_t anyHit,
                                 const NtrRay* d_rays, NtrRayResult* d_results,
                                 const void* d_nodes, int64_t nodesBytes,
                                 const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                                 int32_t layout, uint32_t bvhFlags, void* stream, float* seconds,
                                 NtrSchedHint* hint);

/* A hint can also start from a PREDICTION instead of a measurement: ntr_sched_hint_predict binds the hint to a batch of numBlocks 256-ray
 * blocks and orders them by the caller's per-block cost estimates (any monotone score; heaviest class first).  The next launch with the
 * hint uses that order, measures, and refines it as usual.  For secondary batches the estimate comes from the tree itself:
 *   ntr_bvh_leaf_depths        once per BVH: d_depthByTri[t] = depth of the leaf that holds triangle t (number of inner nodes from the
 *                              root down; triangles in no leaf: 0).  One small launch per tree level; blocking.  *levels = levels walked.
 *   ntr_secondary_block_costs  per batch, beside ray generation: d_blockCost[b] = the deepest leaf among the input rays (primary hits
 *                              d_inResults[first .. first + count)) whose numSamples output rays fall into block b; misses count 0.
 *                              d_blockCost holds (count * numSamples + 255) / 256 words; the call clears them first.
 * Short secondary rays mostly pay for descending to where they start: on the bench frame's AO batches this order recovers what the
 * order learned from a previous launch gives (-9 % launch time), without a previous launch (EXPERIMENTS.md).  No counterpart in the
 * reference, which generates secondary rays (RayGen::ao, src/rt/ray/RayGen.cpp) and traces them in buffer order. */
NTR_API int ntr_sched_hint_predict(NtrSchedHint* hint, const uint32_t* d_blockCost, int32_t numBlocks, void* stream);
NTR_API int ntr_bvh_leaf_depths(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes,
                                const int32_t* d_triIndex, int32_t numTris, int32_t* d_depthByTri, int32_t* levels, void* stream);
NTR_API int ntr_secondary_block_costs(const NtrRayResult* d_inResults, int32_t first, int32_t count, int32_t numSamples,
                                      const int32_t* d_depthByTri, int32_t numTris, uint32_t* d_blockCost, void* stream);

/* Cost estimate of every 256-ray block of a batch, without tracing it: d_blockCost[b] = number of boxes of the BVH's top-of-tree
 * table (the child boxes of the nodes of depth <= 9) that the block's sample ray (its 100th) intersects -- the predictor behind
 * the dispatch order of large closest-hit launches (Spearman 0.86-0.89 against the true block cost on primary batches).  No
 * counterpart in the reference; a multi-GPU host uses it to cut a frame into ranges of equal predicted cost instead of equal
 * ray count (ntrace_amd/dist.py FramePlan).  d_blockCost: (numRays + 255) / 256 words.  Asynchronous on `stream`. */
NTR_API int ntr_predict_block_costs(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes,
                                    uint32_t* d_blockCost, void* stream);

/* Coherence estimate of a batch, without tracing it, from two sample rays (the 100th and the 227th) of every 256-ray block:
 * d_out[0] = blocks whose samples start further apart than 1/8 of the scene's extent, d_out[1] = the divergence score: 4 for every block
 * whose samples start together but point more than 60 degrees apart AND reach further than 1/8 of the scene's extent (bounce rays of a
 * diffuse batch; the short rays of an AO batch do not count) + 1 for every block whose sample ray is degenerate (a missed pixel's
 * secondary ray: no say), d_out[2] = the batch word large closest-hit launches derive on the device: bits 0-15 the pool K
 * of the per-ray kernel (1 = one ray per lane; K > 1 = a wave owns K x 64 rays and refills its finished lanes from them: chosen when
 * origins are scattered in at least half of the blocks -- 4 on trees of 32 MB of nodes and more for batches of 1.5 M rays and more,
 * else 2), bit 16 (NTR_BATCH_DIVERGENT) set when 4 x d_out[0] + d_out[1] reaches the number of blocks (a quarter of the blocks with live
 * rays are incoherent one way or the other).  K > 1 or bit 16 =
 * "incoherent": such a batch is traced by the persistent dynamic-fetch body under every kernel name, a coherent one by the per-ray
 * body (ntr_query_config).  The launch itself does not call this -- its dispatch-order prediction computes the same words -- it is the query
 * for tests and for hosts that plan batches.  No counterpart in the reference.  d_out: 3 words.  Asynchronous on `stream`. */
NTR_API int ntr_predict_batch_coherence(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes,
                                        uint32_t* d_out, void* stream);

/* The dispatch order a large closest-hit launch of this batch would be given, without tracing it: the same two launches as the launch
 * path (class of every 256-ray block = min(boxes hit / 2, 63), class lists concatenated heaviest class first; inside one class the blocks
 * of one group of 64 stay in buffer order) on the BVH's cached top-of-tree table, with the launch's wide pool K.  d_order receives
 * (numRays + 255) / 256 block indices, d_word the batch word (ntr_predict_batch_coherence d_out[2]).  The class counters live in scratch
 * of this call's own (never a launch's) and are zero again when it returns.  numRays == 0: nothing to do.  Blocking (waits for
 * `stream`).  A diagnostic: no trace launch calls it or is changed by it. */
NTR_API int ntr_predict_dispatch_order(int32_t numRays, const NtrRay* d_rays, const void* d_nodes, int64_t nodesBytes,
                                       uint32_t* d_order, uint32_t* d_word, void* stream);

/* What a scheduling hint holds, read back for tests and diagnostics: waits for `stream`, then fills *state and, when the pointers are
 * non-null, copies the hint's numBlocks order words followed by its 3 batch words (h_order: numBlocks + 3 words; the last one is the
 * batch word, ntr_predict_batch_coherence d_out[2]) and its numBlocks cost words (the costs the last refresh launch recorded, or the
 * caller's prediction).  An unbound hint (numBlocks == 0) has no arrays: only *state is filled, and asking for them is an error.
 * Changes nothing in the hint. */
typedef struct {
    int32_t numBlocks;   /* 0 = unbound */
    int32_t device;
    int32_t uses;        /* launches since the hint was (re)bound or predicted */
    int32_t valid;       /* the next launch is dispatched in the hint's order */
    int32_t predicted;   /* the order comes from ntr_sched_hint_predict and no launch has run it yet */
} NtrSchedHintState;
NTR_API int ntr_sched_hint_inspect(const NtrSchedHint* hint, NtrSchedHintState* state, uint32_t* h_order, uint32_t* h_cost, void* stream);

/* Traversal counters: the reference's RayStats (src/rt/bvh/BVH.hpp:44-60), filled by its
 * CPU tracer at src/rt/cuda/CudaBVH.cpp:746-757 and 1107-1111.  numInnerVisits =
 * numNodeTests / 2.  These define the algorithmic bytes of a batch:
 *   48*numRays + 64*numInnerVisits + 48*numTriTests + 16*numLeafVisits + 4*numHits. */
typedef struct NtrTraceStats {
    int64_t numRays;
    int64_t numInnerVisits;
    int64_t numTriTests;
    int64_t numLeafVisits;   /* leaf terminators read */
    int64_t numHits;
} NtrTraceStats;

/* ntr_trace_bvh through an instrumented kernel: same results, plus the counters.
 * Blocking; not a timed path. */
NTR_API int ntr_trace_bvh_stats(const char* kernelName, int32_t numRays, int32_t anyHit,
                                const NtrRay* d_rays, NtrRayResult* d_results,
                                const void* d_nodes, int64_t nodesBytes,
                                const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                                int32_t layout, uint32_t bvhFlags, void* stream, NtrTraceStats* stats);

/* One pass over a Compact node buffer computing hint flags for ntr_trace_bvh:
 *   NTR_BVH_FINITE   every box coordinate is finite and |x| < 2^100.
 *   NTR_BVH_FASTDIV  every box coordinate has |x| < 2^55: together with a per-ray check this
 *                    is the range in which the kernels' refactored divide is the hardware
 *                    divide (see csrc/trace_lane.h).
 *   NTR_BVH_NOTINY   every box coordinate is 0 or |x| >= 2^-93 (lets rays with an exactly-zero
 *                    origin component use the same path).  A NaN is neither: it withholds this flag as it does the other three box flags.
 *   NTR_BVH_ORDERED  every child box has lo <= hi on each axis: for a wave whose rays share the signs of their direction
 *                    components the kernels then know which of a slab's two quotients is the smaller one without comparing.
 *   NTR_BVH_WIDE_LEAVES  leaves hold two or more triangles on average (the device LBVH with leafSize 8; a host SAH tree built with
 *                    leaf preferences (1,1) has one): the per-ray kernel then advances every lane by one node OR one triangle
 *                    per iteration instead of alternating between a node phase and a leaf phase (trace_kernels.hip). */
#define NTR_BVH_FINITE 1u
#define NTR_BVH_FASTDIV 2u
#define NTR_BVH_NOTINY 4u
#define NTR_BVH_ORDERED 8u
#define NTR_BVH_WIDE_LEAVES 16u
/* bit 16 of the batch word (ntr_predict_batch_coherence d_out[2]): long rays that start together and point apart in a quarter of the blocks */
#define NTR_BATCH_DIVERGENT 0x10000u
NTR_API int ntr_bvh_validate(const void* d_nodes, int64_t nodesBytes, uint32_t* flags, void* stream);

/* Device self test: counts quotients x[i]/d[j] for which the FAST divide differs from the
 * hardware `/` (must be 0 inside the FASTDIV range).  Diagnostic, blocking. */
NTR_API int ntr_selftest_division(const float* d_x, int32_t nx, const float* d_d, int32_t nd,
                                  uint32_t* mismatches, void* stream);
/* The same on the quotients that are hardest to round: for every significand D in [2^23, 2^24) the significands X whose quotient X / D
 * lies within 8 / (2^24 D) of a midpoint of two neighbouring floats (enumerated on the device, both quotient binades; what
 * scripts/studies/div_one_correction_check.py checks in exact integer arithmetic), as x = X 2^(xExp + i - 23), d = +-D 2^(dExp + j - 23),
 * i, j = 0..3.  pairs = quotients tested, mismatches = FAST differs from `/` (must be 0).  Diagnostic, blocking. */
NTR_API int ntr_selftest_division_hard(int32_t xExp, int32_t dExp, uint64_t* pairs, uint64_t* mismatches, void* stream);
/* Device self test of the FAST path's admission test: counts the rays of d_rays on which the integer form the trace kernels run (ray_class,
 * trace_lane.h) and the rule's float ranges (directions 2^-40 <= |d| <= 2^20, origins 2^-36 <= |o| < 2^55, a zero origin component only
 * with NTR_BVH_NOTINY in bvhFlags) disagree (must be 0 for every bit pattern).  Diagnostic, blocking. */
NTR_API int ntr_selftest_ray_class(const NtrRay* d_rays, int32_t numRays, uint32_t bvhFlags, uint32_t* mismatches, void* stream);

/* ---- device self tests of the shared device toolkit (radix_sort.h, device_prims.h) on inputs of the caller's choice: the production
 * templates run as they stand and their results come back word for word (tests/test_device_prims_gpu.py compares them with the numpy
 * references of tests/np_device_prims.py).  Diagnostic, blocking. ---- */

/* Sorts n key words with ONE instantiation onesweep_pass_kernel<items, mode, skipTrivial> of those the builders and the ray sort launch:
 * mode 0 with items 8, 16, 24 or 32 (skipTrivial 0) or items 8 (skipTrivial 1); mode 2 with items 8 (skipTrivial 0 or 1).  Mode 1 has no
 * user and is not offered.
 *   mode 0: d_keys[i] is the key of element i (stride must be 1), d_vals[i] its value; d_vals == NULL: the value of element i is i.
 *   mode 2: the key word of element i is d_keys[d_vals[i] * stride], stride 1 or 6, every value in [0, n); the first pass fetches the word
 *           and the others run in mode 0 on the dense (word, value) pairs, as the users chain them.
 * passes (host): numPasses (1 .. 16) pairs (shift, pass number), shift in [0, 24], pass number in [0, 125] (the tile state's status
 * bits hold no more).  The digit histograms of all passes are taken on the device, the tile state is cleared once, the passes ping-pong
 * between two buffers of the library; the inputs are not written.  d_keysOut / d_valsOut (n words each) receive the last pass's keys and
 * values, *errWord the passes' error word (0, or 2 after a look-back that gave up waiting).  forceTicket != 0 hands every pass the
 * ticket counter whatever the grid size; otherwise the pass decides as it does for its users. */
NTR_API int ntr_selftest_onesweep(int32_t items, int32_t mode, int32_t skipTrivial, int32_t n, const uint32_t* d_keys, int32_t stride,
                                  const int32_t* d_vals, int32_t numPasses, const int32_t* passes, int32_t forceTicket,
                                  uint32_t* d_keysOut, int32_t* d_valsOut, uint32_t* errWord, void* stream);
/* The three-launch exclusive scan of n items of `type` (scan_local_store in workgroups of `threads` = 256 or 1024, scan_block_sums, the
 * add): d_prefix[i] = in[0] + .. + in[i - 1], *total (host, one item) the sum of all.  NTR_SCAN_U4: four 32-bit counters per item. */
#define NTR_SCAN_U32 0
#define NTR_SCAN_I32 1
#define NTR_SCAN_U64 2
#define NTR_SCAN_U4 3
NTR_API int ntr_selftest_scan(int32_t type, int32_t threads, int32_t n, const void* d_in, void* d_prefix, void* total, void* stream);
/* scan_block_sums alone, one workgroup of `threads`, on nb >= 0 sums: d_out[i] = d_in[0] + .. + d_in[i - 1] (d_out == d_in: in place),
 * the grand total to *total (host, one item) unless it is NULL. */
NTR_API int ntr_selftest_scan_block_sums(int32_t type, int32_t threads, int32_t nb, const void* d_in, void* d_out, void* total, void* stream);
/* The order-preserving float encoding on n (1 .. 2048) float words: d_single[i][6] = ord_enc, ord_dec(ord_enc), ord_enc_int,
 * ord_dec_int(ord_enc_int), ord_to_int(ord_enc), ord_from_int(ord_to_int(ord_enc)) of word i; d_pairs[i * n + j][2] = ord_min, ord_max of
 * (word i, word j) as float words, for every ordered pair. */
NTR_API int ntr_selftest_float_order(int32_t n, const uint32_t* d_words, uint32_t* d_single, uint32_t* d_pairs, void* stream);
/* Lane i of m (a multiple of 64: whole waves) merges box i (d_boxes[i][6]: min x y z, max x y z) into group d_group[i] (in [0, groups), or
 * -1: none), once with atomic_max_box per lane and once word by word through wave_grouped_atomic.  d_groupsOut[path][group][26], path 0 the
 * plain merge, 1 the grouped one: the six words, the group's member count, its corners by words_box without grow, with grow by eps, with
 * count 0, and words_area.  d_foldsOut[i][6]: wave_min_u32, wave_max_u32, wave_sum_u32, wave_or_u32 of d_lane32 over lane i's wave and
 * wave_min_u64 of d_lane64 (low, high word), as lane i received them. */
NTR_API int ntr_selftest_box_words(int32_t m, const float* d_boxes, const int32_t* d_group, int32_t groups, float eps,
                                   const uint32_t* d_lane32, const uint64_t* d_lane64, uint32_t* d_groupsOut, uint32_t* d_foldsOut,
                                   void* stream);

/* ---- ray production (callers of the hot path) -------- */

/* PixelTable::recalculate (src/rt/ray/PixelTable.cpp:57-143): 8x8 pixel blocks in Morton
 * order then edge stripes.  Either output may be NULL. */
NTR_API int ntr_pixel_table(int32_t w, int32_t h, int32_t* d_indexToPixel, int32_t* d_pixelToIndex, void* stream);

/* rayGenPrimaryKernel (src/rt/ray/RayGenKernels.cu:77-125; RayGenPrimaryInput,
 * RayGenKernels.hpp:37-49).  nscreenToWorld is row-major 4x4.  kernelSeed is the value the
 * reference kernel receives: 0, or Random(seed).getU32() (RayGen.cpp:66). */
NTR_API int ntr_raygen_primary(NtrRay* d_rays, int32_t* d_idToSlot, int32_t* d_slotToID,
                               const int32_t* d_indexToPixel, const float origin[3],
                               const float nscreenToWorld[16], int32_t w, int32_t h, float maxDist,
                               uint32_t kernelSeed, void* stream);

/* rayGenAOKernel (src/rt/ray/RayGenKernels.cu:129-236; RayGenAOInput, RayGenKernels.hpp:53-66):
 * numSamples cosine-hemisphere rays per input ray [firstInputSlot, +numInputRays); rays of
 * missed inputs are degenerate (tmax = -1).  d_triNormals: 3 floats per scene triangle. */
NTR_API int ntr_raygen_ao(NtrRay* d_outRays, int32_t* d_outIDToSlot, int32_t* d_outSlotToID,
                          const NtrRay* d_inRays, const NtrRayResult* d_inResults,
                          const float* d_triNormals, int32_t firstInputSlot, int32_t numInputRays,
                          int32_t numSamples, float maxDist, uint32_t kernelSeed, void* stream);

/* ntr_raygen_ao over per-ray normals: the AO / diffuse generator of a batch whose hits have no table of triangle normals to index,
 * the two-level hits of an instanced scene (ntr_instanced_hit_attributes below writes d_rayNormals).  EXTENSION without a reference
 * counterpart; it is ntr_raygen_ao in every respect -- the same kernel body (csrc/raygen_kernels.hip), the same seeds, slots and
 * outputs -- except where the normal comes from: input slot s uses d_rayNormals[4s .. 4s+2].  An input with id == -1 OR a normal whose
 * fourth word is zero (+0 or -0: no normal could be formed) is a missed input: normal (1, 0, 0), degenerate rays with tmax = -1.  With
 * d_rayNormals[4s..] = (d_triNormals[3 id_s ..], 1) the output equals ntr_raygen_ao's bit for bit.  With maxDist = the camera's far
 * plane and closest hit this is the diffuse batch, as for ntr_raygen_ao.  Asynchronous on `stream` and capturable.
 * NTR_ERR_INVALID: a negative count or slot, a null buffer (when there is a ray to make), d_rayNormals not 16-byte aligned. */
NTR_API int ntr_raygen_ao_normals(NtrRay* d_outRays, int32_t* d_outIDToSlot, int32_t* d_outSlotToID, const NtrRay* d_inRays,
                                  const NtrRayResult* d_inResults, const float* d_rayNormals /* 4 floats per input slot */,
                                  int32_t firstInputSlot, int32_t numInputRays, int32_t numSamples, float maxDist,
                                  uint32_t kernelSeed, void* stream);

/* The times of a motion-blurred frame's rays (csrc/ray_times_kernels.hip): what ntr_trace_instanced_motion and
 * ntr_instanced_hit_attributes_motion take as NtrInstanceMotion::d_rayTimes.  EXTENSION without a reference counterpart: the rule is the
 * numpy spec tests/np_instanced_motion_frame.py, which the device equals bit for bit.  Both calls are asynchronous on `stream` and
 * capturable; they allocate nothing and read nothing back.
 * ntr_ray_times_primary: one hashed time per PIXEL in the shutter [open, close].  Integer arithmetic mod 2^32, binary32, no contraction:
 *   id = d_slotToID ? d_slotToID[s] : s;  x = (uint32)id + (seed + 1) * 0x9E3779B9;
 *   x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16;
 *   u = (float)(x >> 8) * 2^-24 (exact, in [0, 1 - 2^-24]);  span = close - open;  t = open + u * span (the product rounded, then the
 *   sum);  d_times[s] = t < close ? t : close.  With open = 0, close = 1 the time is u bit for bit.
 *   The time depends on the pixel id, not on the slot: ntr_ray_morton_sort and the pixel table may reorder the rays without changing a
 *   pixel's time; another seed per accumulated frame gives another sample.
 * ntr_ray_times_secondary: d_outTimes[k * numSamples + j] = d_inTimes[firstInputSlot + k] for k < numInputRays, j < numSamples, the
 *   word verbatim (a NaN included) -- ntr_raygen_ao_normals' slot rule, so a secondary ray sees its instance where its primary ray saw
 *   it.  Nothing outside that window is written.
 * NTR_ERR_INVALID (before any device work): a negative count or slot, numSamples < 1, numInputRays * numSamples >= 2^31, open or close
 * not finite or not 0 <= open <= close <= 1; then, when there is a time to write, a null buffer or a times pointer that is not 4-byte
 * aligned.  Zero rays return NTR_OK.  Without a device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP. */
NTR_API int ntr_ray_times_primary(int32_t numRays, const int32_t* d_slotToID /* NULL: id = slot */, uint32_t seed, float open, float close,
                                  float* d_times, void* stream);
NTR_API int ntr_ray_times_secondary(const float* d_inTimes, int32_t firstInputSlot, int32_t numInputRays, int32_t numSamples,
                                    float* d_outTimes, void* stream);

/* rayGenShadowKernel (src/rt/ray/RayGenKernels.cu:240-301; RayGen::shadow, RayGen.cpp:114-150): numSamples rays per input ray
 * [firstInputSlot, +numInputRays) from its hit point (backed off 1e-2 along the ray) towards quasi-random points of the cube of
 * half-edge lightRadius around lightPos; tmax = the distance to that point, rays of missed inputs are degenerate (tmax = -1).
 * kernelSeed as for ntr_raygen_ao (Random(seed).getU32(), RayGen.cpp:139).  The output batch is an any-hit batch. */
NTR_API int ntr_raygen_shadow(NtrRay* d_outRays, int32_t* d_outIDToSlot, int32_t* d_outSlotToID, const NtrRay* d_inRays,
                              const NtrRayResult* d_inResults, int32_t firstInputSlot, int32_t numInputRays, int32_t numSamples,
                              const float lightPos[3], float lightRadius, uint32_t kernelSeed, void* stream);

/* countHitsKernel (src/rt/cuda/RendererKernels.cu:174-226; Renderer::getTotalNumRays,
 * Renderer.cpp:676-709): number of results with id >= 0 (RendererKernels.cu:193).  Blocking. */
NTR_API int ntr_count_hits(const NtrRayResult* d_results, int32_t numRays, int32_t* count, void* stream);

/* ---- on-device LBVH build ------------------------------------------------------------------ */

/* Result of ntr_lbvh_build: exact buffer sizes (the reference resizes its buffers to these,
 * HLBVHBuilder.cpp:382-386) and per-phase GPU times (HLBVHBuilder::getGPUTime, :571-573). */
typedef struct NtrLbvhResult {
    int32_t numNodes, numLeaves, numLevels, pad;
    /* extents of what was written.  nodesBytes >= 64 * numNodes and triWoopBytes >= 16 * (3 * numTris + numLeaves): equality except
     * where the depth rule (level bit 0, emitTreeKernel.cu:289-292) made a leaf of more than leafSize equal Morton codes -- the node
     * indices and terminator slots set aside inside such a leaf stay unused and are zero-filled. */
    int64_t nodesBytes, triWoopBytes, triIndexBytes;
    float   seconds;                                   /* whole build, GPU time          */
    /* phase times.  Default (bottom-up) path: Morton codes + digit histograms; the four sort passes; woopMs ~ 0; emitMs =
     * leaf marks + their prefix counts; refitMs = bottom-up emit writing nodes, boxes, Woop rows (agglomerate kernels + equal-key runs).
     * Legacy paths: per-triangle box terms (per-level path: Woop rows) in woopMs; emitMs = top pass (per-level: all levels);
     * refitMs = subtree emit + refit + top refit + Woop placement (per-level: refit). */
    float   mortonMs, sortMs, woopMs, emitMs, refitMs;
} NtrLbvhResult;

/* Worst-case output sizes for numTris triangles (what HLBVHBuilder allocates before the build,
 * HLBVHBuilder.cpp:532-538, 772-784). */
NTR_API int ntr_lbvh_capacity(int32_t numTris, int64_t* nodesBytes, int64_t* triWoopBytes, int64_t* triIndexBytes);

/* HLBVHBuilder::buildLBVH (src/rt/bvh/HLBVH/HLBVHBuilder.cpp:451-593; the path taken for
 * !hlbvh || hlbvhBits == 10, :44-47): Morton codes -> stable radix sort -> Woop rows -> level-by-level
 * emit -> bottom-up refit, all on the device, into caller-owned BVHLayout_Compact buffers of at least
 * ntr_lbvh_capacity() bytes.  d_triVtxIndex: 3 ints per triangle, d_vtxPos: 3 floats per vertex
 * (Scene::getTriVtxIndexBuffer / getVtxPosBuffer), sceneMin/Max = Scene::getBBox.  Renderer passes
 * leafSize 8, epsilon 0.001 (Renderer.cpp:203-207).  Blocking: the call reads counts back and
 * synchronises the stream, so a stream that is being captured is refused with NTR_ERR_INVALID before
 * anything is allocated or launched (the capture stays valid and the outputs untouched). */
NTR_API int ntr_lbvh_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                           const float sceneMin[3], const float sceneMax[3], int32_t leafSize, float epsilon,
                           void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                           int32_t* d_triIndex, int64_t triIndexCapacity, NtrLbvhResult* result, void* stream);

/* Result of ntr_hlbvh_build: the LBVH's counts, exact extents and times (lbvh.sortMs = Morton codes + sort, lbvh.emitMs = bottom-level
 * emit, lbvh.refitMs = refit, lbvh.numLevels = creation batches refit), plus the cluster count, the number of top-level (SAH) inner
 * nodes and levels, and the phase times of the clusters, the top level and the bottom level (emit + refit).  For hlbvhBits == 10 or
 * numTris <= leafSize (the LBVH's tree) numClusters, topNodes and topLevels are 0 and lbvh is ntr_lbvh_build's result. */
typedef struct NtrHlbvhResult {
    NtrLbvhResult lbvh;
    int32_t numClusters, topNodes, topLevels, pad;
    float   clusterMs, topMs, bottomMs, pad2;
} NtrHlbvhResult;

/* HLBVHBuilder::buildHLBVH (src/rt/bvh/HLBVH/HLBVHBuilder.cpp:595-750; the path taken for hlbvh && hlbvhBits != 10, :44-47):
 * the triangles are grouped into Morton clusters (equal code >> 3 * hlbvhBits, radixSort.cu:48-115), a binned-SAH tree of 8 bins per
 * axis is built over the clusters (buildTopLevel :156-317, fillBins / findSplit / distribute, emitTreeKernel.cu:713-1027) and an LBVH
 * inside each cluster (buildBottomLevel :319-406, starting level 3 * hlbvhBits - 1).  The ntr_lbvh_build arguments plus hlbvhBits in
 * 0..10 (anything else is NTR_ERR_INVALID; 10 is ntr_lbvh_build).  Same Compact conventions, capacities (ntr_lbvh_capacity) and
 * stream rules as ntr_lbvh_build; Renderer's HLBVH setup is hlbvhBits 4, leafSize 8, epsilon 0.001 (Renderer.cpp:201-209).  The
 * tree equals the restatement tests/np_hlbvh.py in canonical form; its header lists the canonical choices where the reference is
 * nondeterministic or broken.  Blocking (one read-back after the clusters, one per eight top levels, one at the end); as
 * ntr_lbvh_build, a capturing stream is refused with NTR_ERR_INVALID before any allocation or launch.  On the cluster path
 * (hlbvhBits < 10 and numTris > leafSize) no byte of the output buffers past the reported extents is written. */
NTR_API int ntr_hlbvh_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                            const float sceneMin[3], const float sceneMax[3], int32_t leafSize, float epsilon, int32_t hlbvhBits,
                            void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                            int32_t* d_triIndex, int64_t triIndexCapacity, NtrHlbvhResult* result, void* stream);

/* The builder keeps one grow-only scratch workspace per device between builds (a rebuild per frame must not pay allocations):
 * about 175 B per triangle on the default path (1.75 GB after a 10 M-triangle build).  A host that builds once and then only
 * traces returns it with this call (it waits for the device first); the next build allocates again.  ntr_ray_morton_sort keeps its
 * temporaries the same way (about 40 B per ray of the largest batch sorted so far), and ntr_hlbvh_build its own scratch (about 60 B per
 * triangle plus about 500 B per Morton cluster); this call returns them too. */
NTR_API int ntr_lbvh_release_workspace(void);

/* On-device binned SAH BVH build: the reference's persistent BVH builder as configured (Renderer.cpp:262-267 "PersistentBVH";
 * CudaPersistentBVHBuilder.cpp, persistent_bvh.cu with CudaTracerDefines.h SPLIT_TYPE 5, PLANE_COUNT 32, BINNING_TYPE 2, AABB_TYPE 3,
 * SAH_TERMINATION, COMPUTE_MEDIAN_BOUNDS; config.conf block PersistentBVH), rebuilt breadth first, one level per round, without its
 * persistent task pool or device heap (csrc/bvh_build_kernels.hip; the spec is tests/np_bvh_binned.py).  The tree feeds ntr_trace_bvh
 * unchanged.
 *   candidates  32 planes per task, 11 / 11 / 10 on x / y / z, pos = lo + (hi - lo) * ((1 + k) / 12.f), two roundings, over the task's
 *               box as written into its parent node (the root's: sceneMin / sceneMax) (findPlaneAABB, rt_common.cu:1007-1030)
 *   sides       the centroid c = fl(fl(mn + mx) * 0.5f) of the triangle's box; fl(pos - c) < 1e-8f is side -1, which goes to child 0
 *               (getPlaneCentroidPosition, rt_common.cu:449-468): child 0 holds the centroids at or above the plane
 *   cost        s = area(boxL) * nL + area(boxR) * nR over the sides' union boxes; an empty side's box is (FLT_MAX, -FLT_MAX), so its
 *               cost is NaN.  CANONICAL: the lowest finite s wins (+0 == -0), then the lowest plane; NaN and infinite s never win
 *   median      no winning plane -> child 0 gets the first n / 2 references of the task, child 1 the rest (persistent_bvh.cu:1815-1822)
 *   boxes       a child's box is fl(min - epsilon) / fl(max + epsilon) of its triangles' union (min / max with -0 < +0), on the SAH
 *               and the median path alike (persistent_bvh.cu:1855-1863, 4259-4261)
 *   termination (persistent_bvh.cu:245-271) nL + nR <= triMaxLimit and ci * n < ct + ci * (areaL / area * nL + areaR / area * nR)
 *               makes the task a leaf; otherwise a child with <= triLimit references or below a parent of depth > maxDepth - 2 is a
 *               leaf, root depth 0
 *   order       inner nodes in level order (root 0, child 0 before child 1); leaf Woop blocks and triIndex entries in the same order,
 *               ascending triangle ids (the partition is stable): 3 rows per triangle (woop_rows.h), then a terminator row of
 *               0x80000000; the triIndex entry of a triangle's first row is its id, the others are 0.  Compact nodes as ntr_lbvh_build
 *               writes them: an inner child is 64 * index, a leaf child ~row, word 14 the split axis (0 for a median split), word 15 0.
 * DEVIATION: the root is never a leaf (a Compact root is an inner node).  A root that termination ends (numTris <= triLimit, or the
 *   SAH test) is split by its plane, else the median, into two leaves; one triangle gives an empty child 0 (box (FLT_MAX, -FLT_MAX),
 *   a terminator row only) and the triangle in child 1, as the LBVH's one-triangle tree.
 * Output: caller-owned BVHLayout_Compact buffers of at least ntr_lbvh_capacity() bytes, which bound the tree: a BVH without duplicate
 *   references has at most max(N - 1, 1) inner nodes and 3N + leaves <= 4N + 1 Woop rows.  The result's *Bytes are the exact extents.
 * Params: triLimit, triMaxLimit, maxDepth, ci, ct, epsilon; params == NULL is config.conf's block with epsilon = FLT_EPSILON
 *   (Renderer.cpp:264).  childLimit, popCount and granularity configure SPLIT_TYPE 6 and the task pool and have no counterpart here.
 * NTR_ERR_INVALID: numTris < 1 or >= 2^28, numVerts < 1, a null pointer, triLimit < 1, triMaxLimit < 0, maxDepth outside 1..100 (the
 *   reference CPU tracer's stack of 100 entries, CudaBVH.cpp:701; the kernels hold 16 + 88), a non-finite ci / ct / epsilon, a
 *   negative epsilon, a scene box with a non-finite coordinate or min > max on an axis (the planes must not decrease along an axis),
 *   output buffers smaller than ntr_lbvh_capacity(), or (found on the device) a vertex index outside [0, numVerts).
 *   NTR_ERR_OVERFLOW: the tree would have more than 0x76543200 / 64 = 31 019 208 inner nodes, which Compact's signed 32-bit child byte
 *   offsets below the sentinel 0x76543210 cannot address (as ntr_lbvh_build; possible only beyond 31 M triangles with small leaves).
 *   No node at or beyond that bound is written.  NTR_ERR_NOMEM: device memory (for numTris < 2^28 every index of the kernels fits
 *   int32, so no level exceeds their indexing).  NTR_ERR_LAYOUT: an internal consistency check failed (not expected; reported instead
 *   of writing out of bounds).
 * The call blocks (one 32 B read-back per level).  The scratch is a per-device grow-only pool that ntr_lbvh_release_workspace returns:
 *   one build per device at a time. */
typedef struct NtrPersistentBvhParams {
    int32_t triLimit, triMaxLimit, maxDepth, pad;
    float   ci, ct, epsilon, pad2;
} NtrPersistentBvhParams;
typedef struct NtrPersistentBvhResult {
    int32_t numNodes, numLeaves, numLevels, maxDepth;   /* inner nodes, leaves (the empty one included), rounds, inner nodes on the
                                                           longest root-to-leaf path */
    int32_t medianFallbacks, costLeaves, depthLeaves, pad;   /* tasks split at the median; tasks the SAH test ended; children with
                                                                more than triLimit references made leaves by the depth cap */
    int64_t nodesBytes, triWoopBytes, triIndexBytes;   /* exact extents of what was written */
    float   seconds;                   /* host wall clock of the whole call */
    float   prepMs, levelsMs, emitMs;  /* GPU event times: per-triangle terms, the level loop, the leaves' Woop rows */
} NtrPersistentBvhResult;
NTR_API int ntr_persistent_bvh_params_default(NtrPersistentBvhParams* params);
NTR_API int ntr_persistent_bvh_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                                     const float sceneMin[3], const float sceneMax[3], const NtrPersistentBvhParams* params,
                                     void* d_nodes, int64_t nodesCapacity, void* d_triWoop, int64_t triWoopCapacity,
                                     int32_t* d_triIndex, int64_t triIndexCapacity, NtrPersistentBvhResult* result, void* stream);
/* Bytes the builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_persistent_bvh_scratch_bytes(int64_t* bytes);

/* On-device full-sweep SAH BVH build: the tree of ntr_sah_build -- the host builder host/bvh/SAHBVHBuilder.cpp, i.e. the reference's
 * SAHBVHBuilder (src/rt/bvh/SAHBVHBuilder.cpp:51-254) with Platform("GPU") (Renderer.cpp:88-89: node cost 1, triangle cost 1, batch
 * sizes 1) and leaf preferences (minLeafSize, maxLeafSize) -- node for node and triangle for triangle, built one level per round
 * from three axis orders sorted once (csrc/sah_build_kernels.hip; the spec is tests/np_sah_sweep.py).  The tree feeds ntr_trace_bvh,
 * ntr_bvh_refit and ntr_bvh_optimize unchanged.
 *   triangles   box = min / max of the vertices (-0 < +0); key on axis d = fl(min[d] + max[d]); a triangle whose box has a negative
 *               extent or at most one non-zero extent (size.min() < 0 || size.sum() == size.max(), :141-151) is dropped and reaches no
 *               leaf; the root's box covers every triangle, the dropped ones too (:70-84)
 *   order       ascending key (-0 == +0), ties by ascending triangle id (:106-115); every node owns the same range of all three orders
 *   sweep       node of m references, area A (AABB::area, 0 for an invalid box): for each axis and i = 1 .. m-1
 *               sah = fl(fl(A * 2 + fl(areaL(i) * fl(i))) + fl(areaR(i) * fl(m - i))), balance = fl(fl(i)^2 + fl(m - i)^2); the winner is
 *               the lexicographic minimum of (sah, balance, axis, i) under float < / == starting from (FLT_MAX, FLT_MAX) (:221-232): a
 *               NaN or infinite sah never wins.  Without a winner (m < 2, overflowing areas) ALL references go to child 1 and none to
 *               child 0, as the host's default split has it; that chain ends at depth 64
 *   leaves      level != 0 && m <= minLeafSize, or level >= 64, before the search; level != 0 && min(leafSAH, sah) == leafSAH &&
 *               m <= maxLeafSize after it (:155-156, :163-165), leafSAH = fl(A * fl(m)).  The root is never a leaf.  A leaf lists its
 *               triangles back to front of the order its range was last arranged by: axis 2 after a search, else the parent's split
 *               axis (:193-203)
 *   children    the first numLeft of the winning axis' order are child 0; boxes are the exact unions without epsilon, an empty child's
 *               (FLT_MAX, -FLT_MAX); word 14 is SplitInfo::getBitCode() (the axis; 0 without a winner), word 15 is 0
 *   order       CANONICAL (the host's createCompact numbers by an explicit stack instead; compare the trees by walking them): inner
 *               nodes in level order (root 0, child 0 before child 1); leaf Woop blocks and triIndex entries in the same order: 3 rows
 *               per triangle (woop_rows.h, as the other device builders), then a terminator row of 0x80000000; the triIndex entry of a
 *               triangle's first row is its id, the others are 0
 * The sign of a zero box coordinate is the one freedom against the host tree (FW::min / max keep the first operand's zero); no area,
 * cost or decision depends on it.  NaN coordinates are out of contract.
 * Output: caller-owned BVHLayout_Compact buffers of at least ntr_lbvh_capacity() bytes.  They hold every tree whose splits all have a
 *   winner (at most max(N - 1, 1) inner nodes, 3N + leaves <= 4N + 1 rows); a chain of splits without a winner adds one inner node and
 *   one empty leaf per level, and a tree that outgrows the buffers passed is NTR_ERR_OVERFLOW (pass larger ones).  The result's *Bytes
 *   are the exact extents.
 * NTR_ERR_INVALID (before any device work): numTris < 1 or >= 2^28, numVerts < 1, a null pointer, minLeafSize < 1, maxLeafSize <
 *   minLeafSize, output buffers smaller than ntr_lbvh_capacity(); (found on the device) a vertex index outside [0, numVerts).
 *   NTR_ERR_OVERFLOW: more than 0x76543200 / 64 inner nodes (Compact's 32-bit child offsets), or a tree beyond the buffers passed; no
 *   node or row beyond either bound is written.  NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a device: there is no CPU fallback.
 *   NTR_ERR_NOMEM: device memory.  NTR_ERR_LAYOUT: an internal consistency check failed (not expected).  A failed call zeroes *result.
 * The call blocks (one 32 B read-back per level).  The scratch (about 310 B per triangle) is a per-device grow-only pool that
 *   ntr_lbvh_release_workspace returns: one build per device at a time. */
typedef struct NtrSahDeviceResult {
    int32_t numNodes, numLeaves, numLevels, maxDepth;   /* inner nodes, leaves (empty ones included), rounds, inner nodes on the
                                                           longest root-to-leaf path */
    int32_t numDropped, pad[3];            /* triangles the drop test removed */
    int64_t nodesBytes, triWoopBytes, triIndexBytes;   /* exact extents of what was written */
    float   seconds;                       /* host wall clock of the whole call */
    float   prepMs, sortMs, levelsMs, emitMs;          /* GPU event times: boxes and live list, the three sorts, the level loop, the
                                                           leaves' Woop rows */
} NtrSahDeviceResult;
NTR_API int ntr_sah_device_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                                 int32_t minLeafSize, int32_t maxLeafSize, void* d_nodes, int64_t nodesCapacity, void* d_triWoop,
                                 int64_t triWoopCapacity, int32_t* d_triIndex, int64_t triIndexCapacity, NtrSahDeviceResult* result,
                                 void* stream);
/* Bytes the builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_sah_device_scratch_bytes(int64_t* bytes);

/* On-device PLOC build (parallel locally-ordered clustering, Meister and Bittner 2018): a bottom-up tree over the LBVH's Morton order
 * (csrc/bvh_ploc_kernels.hip).  On the CPU the rule's tree at radius 8 has SAH cost 73.1 on the 262 k atrium, where the LBVH has 99.3,
 * HLBVH (bits 4) 72.4 and the host SAH tree 66.4; what the build costs on the device is in DESIGN.md 6j.  EXTENSION without a reference counterpart:
 * the rule is the numpy spec tests/np_bvh_ploc.py, which the build equals byte for byte.  The tree feeds ntr_trace_bvh,
 * ntr_bvh_validate, ntr_bvh_refit, ntr_bvh_optimize, ntr_bvh_sah_cost and ntr_bvh_reorder unchanged.
 *   order       ntr_lbvh_build's Morton codes over sceneMin / sceneMax and its stable sort (ties by triangle id); no triangle is dropped
 *   leaves      one triangle per leaf in sorted order: leaf p owns rows 4p .. 4p + 3 (three Woop rows, woop_rows.h, and a terminator
 *               row of 0x80000000), link ~(4p); the triIndex entry of the first row is the triangle id, the others 0; box = min / max
 *               of the vertices (-0 < +0), no epsilon
 *   clusters    (box, link, height); the list starts as the leaves, height 0.  A round, while the list has n > 1 clusters:
 *   distance    d(i, j) = fl(fl(fl(dx * dy) + fl(dy * dz)) + fl(dz * dx)) of the union box (min / max with -0 < +0), dx = fl(hi.x - lo.x)
 *               ..., no contraction; a NaN counts as +inf
 *   neighbour   nn[i] = the j != i with |i - j| <= radius inside the list of least key (d, k, b), k = |i - j|, b = (min(i, j) / k) & 1;
 *               d compared as floats (+0 == -0).  The key is symmetric and no two candidates of one cluster share (k, b), so the pair
 *               of least key is mutual: every round merges at least one pair
 *   merge       i and j = nn[i] merge iff nn[j] == i.  Of a round's m pairs the one whose lower index has rank r (ascending, from 0)
 *               gets node slot (n - 1 - m) + r: the last round writes slot 0, the root; N - 1 slots in all.  Child 0 is the lower-index
 *               cluster, child 1 the upper, boxes and links as they stand; word 14 and word 15 are 0
 *   compaction  the merged cluster takes the lower index's place (box the union, link 64 * slot, height 1 + max); the upper index
 *               disappears; everything else keeps its relative order
 *   N == 1      one node: child 0 an empty leaf (box (FLT_MAX, -FLT_MAX), row 0 a terminator), child 1 the triangle (rows 1..3, a
 *               terminator at row 4), as ntr_persistent_bvh_build's one-triangle tree
 * Once the list has at most NTR_PLOC_TAIL clusters one workgroup runs the remaining rounds out of LDS in one launch; before that a
 * round is four launches over tiles of NTR_PLOC_TILE clusters.  Neither constant changes a byte of the result.
 * Output: caller-owned BVHLayout_Compact buffers of at least ntr_lbvh_capacity() bytes: max(N - 1, 1) nodes, 4N rows (5 for N == 1).
 *   The result's *Bytes are the exact extents.
 * NTR_ERR_INVALID (before any device work): numTris < 1 or >= 2^28, numVerts < 1, a null pointer, radius outside 1..64, a scene box
 *   with a non-finite coordinate or min > max on an axis, output buffers smaller than ntr_lbvh_capacity(); (found on the device, before
 *   anything is written) a vertex index outside [0, numVerts).  NTR_ERR_OVERFLOW: a tree of height above 100 (inner nodes on the
 *   longest path; the reference CPU tracer's stack, ntr_persistent_bvh_build's bound): the buffers are then not to be traced; or more
 *   than 0x76543200 / 64 inner nodes.  NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a device: there is no CPU fallback.  NTR_ERR_NOMEM:
 *   device memory.  NTR_ERR_LAYOUT: an internal consistency check failed (not expected).  A failed call zeroes *result.
 * The call blocks (one 32 B read-back per four rounds before the tail).  The scratch (about 100 B per triangle) is a per-device
 *   grow-only pool that ntr_lbvh_release_workspace returns: one build per device at a time. */
#define NTR_PLOC_TAIL 1024   /* list length at or below which the single-workgroup tail takes over */
#define NTR_PLOC_TILE 1024   /* clusters per workgroup of the rounds before the tail */
typedef struct NtrPlocResult {
    int32_t numNodes, numLeaves, numRounds, height;   /* inner nodes, leaves (N == 1: the empty one included), rounds (tail rounds
                                                         included), inner nodes on the longest root-to-leaf path */
    int32_t tailClusters, pad[3];          /* list length when the tail launch took over, 0 if none (N == 1) */
    int64_t nodesBytes, triWoopBytes, triIndexBytes;   /* exact extents of what was written */
    float   seconds;                       /* host wall clock of the whole call */
    float   mortonMs, sortMs, roundsMs, tailMs, emitMs;   /* GPU event times: the vertex index check and its read-back (the Morton
                                                             codes come with the sort's launches, as in ntr_hlbvh_build); codes and
                                                             sort; the rounds before the tail; the tail; leaf clusters and Woop rows */
} NtrPlocResult;
NTR_API int ntr_ploc_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                           const float sceneMin[3], const float sceneMax[3], int32_t radius, void* d_nodes, int64_t nodesCapacity,
                           void* d_triWoop, int64_t triWoopCapacity, int32_t* d_triIndex, int64_t triIndexCapacity, NtrPlocResult* result,
                           void* stream);
/* Bytes the builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_ploc_scratch_bytes(int64_t* bytes);

/* Instanced scenes: a top-level tree (TLAS) over instances of bottom-level trees (BLAS), built on the device, and a two-level trace
 * (csrc/tlas_build_kernels.hip, csrc/trace_instanced_kernels.hip, csrc/instanced_bvh.h).  EXTENSION without a reference counterpart:
 * the rule is the numpy spec tests/np_instanced.py, which ntr_instance_invert, ntr_tlas_build and ntr_trace_instanced equal bit for bit.
 *   pool        three device buffers: nodes, triWoop, triIndex.  BLAS k occupies [nodesOffset, +nodesBytes) of the pool's nodes (multiples
 *               of 64, nodesBytes >= 64) and [triWoopOffset, +triWoopBytes) of its triWoop (multiples of 16); its triIndex entries
 *               start at entry triWoopOffset / 16.  A BLAS is byte for byte what any builder of this library wrote when it was handed
 *               pool + offset (or what was copied there): links stay relative to its own start, its root is its node 0.  A BLAS keeps
 *               Compact's limits (nodesBytes <= 0x76543200); each pool buffer is at most 0xFFFFFF00 bytes.
 *   instance    objectToWorld and worldToObject, 3x4 row-major, and the index of its BLAS.  ntr_instance_invert makes the second from
 *               the first in binary64 (cofactors over the determinant, translation -(inv * t), each result rounded once).
 *   world box   the union of the two child boxes of the BLAS's node 0, its eight corners through objectToWorld, min / max (-0 < +0);
 *               no padding: a hit within rounding of an instance's box surface can be culled, as in every two-level tracer
 *   top level   the LBVH's Morton code of the world box over the union of all world boxes, a stable sort, then ntr_ploc_build's rounds
 *               over (world box, link ~i, height 0), i the instance's index in the caller's array; N - 1 nodes, rootLink 0.
 *               N == 1: no node, rootLink ~0
 *   record i    64 bytes: words 0..11 worldToObject, 12 nodesOffset, 13 triWoopOffset / 16, 14 nodesBytes, 15 zero
 *   trace       closest or any hit through both levels with one stack (16 + 88 entries) and one shrinking tmax; the ray is transformed
 *               by worldToObject on entering an instance (origin with w = 1, direction with w = 0, not normalised: t means the same on
 *               both levels).  GENERIC arithmetic only.  Every fetch is range checked: whatever a link or an offset holds, nothing
 *               outside the buffers is read.  d_instanceIDs[r] receives the instance of ray r's hit, -1 for a miss.
 * ntr_tlas_build: NTR_ERR_INVALID for numInstances < 1, a radius outside 1..64, null buffers, capacities below ntr_tlas_capacity, a
 *   BLAS range that is misaligned, outside the pool or above the limits; (found on the device) a blas index outside [0, numBlas).
 *   NTR_ERR_OVERFLOW: a top-level tree higher than 100.  NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a device.  A failed call zeroes
 *   *result.  The call blocks; its scratch is a per-device pool that ntr_lbvh_release_workspace returns.
 * ntr_trace_instanced: seconds == NULL is asynchronous on `stream` and capturable, like ntr_trace_bvh; a traversal stack overflow
 *   sets the status word that ntr_trace_status reads. */
typedef struct NtrBlasRange { int64_t nodesOffset, nodesBytes, triWoopOffset, triWoopBytes; } NtrBlasRange;   /* host array */
typedef struct NtrInstance {                                                                                  /* device array, 112 B */
    float   objectToWorld[12];
    float   worldToObject[12];
    int32_t blas;
    int32_t reserved[3];
} NtrInstance;
typedef struct NtrTlasResult {
    int32_t rootLink, numNodes, numRounds, height;   /* 0 (N >= 2) or ~0 (N == 1); N - 1; rounds, tail rounds included; inner nodes on the longest path */
    int32_t tailClusters, pad[3];                    /* list length when the tail launch took over, 0 if none (N == 1) */
    int64_t nodesBytes, recordsBytes;                /* exact extents of what was written */
    float   sceneMin[3], sceneMax[3];                /* the union of the instances' world boxes */
    float   seconds;                                 /* host wall clock of the whole call */
    float   boxesMs, sortMs, clustersMs, roundsMs, tailMs;   /* GPU event times: world boxes, records and the index check's read-back;
                                                                codes and sort; the cluster list; the rounds before the tail; the tail */
} NtrTlasResult;
/* host only, no device: worldToObject from objectToWorld.  NTR_ERR_INVALID: null, or a zero or non-finite determinant. */
NTR_API int ntr_instance_invert(const float objectToWorld[12], float worldToObject[12]);
/* max(N - 1, 1) * 64 and N * 64 bytes */
NTR_API int ntr_tlas_capacity(int32_t numInstances, int64_t* nodesBytes, int64_t* recordsBytes);
NTR_API int ntr_tlas_build(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                           const void* d_poolNodes, int64_t poolNodesBytes, int32_t radius, void* d_tlasNodes, int64_t tlasNodesCapacity,
                           void* d_records, int64_t recordsCapacity, NtrTlasResult* result, void* stream);
/* Bytes the builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_scratch_bytes(int64_t* bytes);
NTR_API int ntr_trace_instanced(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, float* seconds /* NULL: asynchronous */,
                                void* stream);

/* Instance visibility and counters of the two-level trace (csrc/trace_instanced_kernels.hip).  EXTENSION; the rule is the
 * numpy spec tests/np_instanced_masked.py: ntr_trace_instanced's rule with one change to the step "top level, link ~i".
 *   masks       ray r carries m_r = d_rayMasks[r] when per-ray masks are given, else rayMask; instance i carries M_i =
 *               d_instanceMasks[i] when instance masks are given, else 0xFFFFFFFF.  All 32 bits are mask bits.
 *   entering    if (M_i & m_r) != 0 the ray enters instance i exactly as in ntr_trace_instanced.  Otherwise the step is a pop: no exit
 *               marker is pushed, the ray is not transformed, tmax, the hit and the instance id are untouched.  A ray with m_r == 0
 *               still walks the top level and ends as a miss.  A link ~i with i >= numInstances is popped and its mask is never read.
 *   tree        visibility is not geometry: NtrInstance, the 64-byte record, ntr_tlas_build and ntr_tlas_refit know nothing of the
 *               masks, which live in an array of their own; a build or a refit neither needs nor erases them.
 *   counters    summed over the rays of a launch, a step being one iteration of a ray in the spec's loop; one ray is traced by one lane
 *               with no sharing, so they are deterministic and equal the spec's exactly.  An entering step whose index is outside
 *               [0, numInstances) or that finds no room for the marker counts as neither an entry nor a masked step.
 *   bytes       the algorithmic bytes of a launch are
 *                 52 numRays + 64 (numTopInnerVisits + numInstanceEntries + numInnerVisits) + 32 numInstanceEntries + 48 numTriTests
 *                 + 16 numLeafVisits + 4 numHits
 *               (the ray, the record and the instance id; the 64-byte fetches; the world ray reloaded on leaving; triangles;
 *               terminators; the index remap), plus 4 (numInstanceEntries + numInstancesMasked) when instance masks are given and
 *               4 numRays when per-ray masks are given.
 * ntr_trace_instanced_masked: seconds == NULL is asynchronous on `stream` and capturable, like ntr_trace_instanced; the call allocates
 *   nothing and reads nothing back.  With vis == NULL -- or a vis that can refuse nothing: no arrays and rayMask 0xFFFFFFFF -- it launches
 *   the very kernel ntr_trace_instanced launches.  The mask arrays are read by the launch: a captured launch reads their contents at
 *   replay time, and rewriting them between replays is the intended way to change visibility.  Every mask read is range checked.
 * ntr_trace_instanced_stats: the same records through an instrumented variant of the kernel, plus the counters.  It blocks, is refused
 *   with NTR_ERR_INVALID on a capturing stream and is not a timed path.
 * Errors: NTR_ERR_INVALID before any device work for everything ntr_trace_instanced refuses, a mask pointer that is not 4-byte aligned
 *   and a null stats; numRays == 0 returns NTR_OK with the stats zeroed; without a device, after these checks, NTR_ERR_NO_DEVICE /
 *   NTR_ERR_HIP. */
typedef struct NtrInstanceVisibility {      /* host struct of device pointers */
    const uint32_t* d_instanceMasks;        /* numInstances words, or NULL: every instance 0xFFFFFFFF */
    const uint32_t* d_rayMasks;             /* numRays words, or NULL: every ray has rayMask */
    uint32_t rayMask, pad;
} NtrInstanceVisibility;
typedef struct NtrInstancedTraceStats {
    int64_t numRays;              /* rays of the launch */
    int64_t numTopInnerVisits;    /* inner steps on the top level */
    int64_t numInstanceEntries;   /* entering steps that entered */
    int64_t numInstancesMasked;   /* entering steps the masks refused */
    int64_t numInnerVisits;       /* inner steps inside instances */
    int64_t numTriTests;          /* rows tested that are not a terminator */
    int64_t numLeafVisits;        /* terminator rows read */
    int64_t numHits;              /* rays whose record has id != -1 */
} NtrInstancedTraceStats;
NTR_API int ntr_trace_instanced_masked(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                       const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                       int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                       int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                       const NtrInstanceVisibility* vis /* NULL: no masks */, float* seconds /* NULL: asynchronous */,
                                       void* stream);
NTR_API int ntr_trace_instanced_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                      const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                      int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                      int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                      const NtrInstanceVisibility* vis /* may be NULL */, NtrInstancedTraceStats* stats, void* stream);

/* Refit of a top-level tree: the TLAS keeps its topology and gets its instance records and every box again, from the current
 * instances and the pool's current node-0 boxes, in two launches (csrc/tlas_refit_kernels.hip).  It is the update path
 * of a frame whose instances moved rigidly or whose BLASes were refitted (ntr_bvh_refit_batch); ntr_tlas_build, a blocking chain of
 * some dozens of launches, restores the tree's quality every so many frames.  EXTENSION without a reference counterpart: the rule is
 * the numpy spec tests/np_tlas_refit.py, which the device equals byte for byte.
 *   input       the node buffer, rootLink and record buffer ntr_tlas_build filled for the same number of instances (or any buffers
 *               of that layout); d_instances as for ntr_tlas_build (here 16-byte aligned), with new transforms and, where an instance
 *               switched its BLAS (a level of detail), a new blas index
 *   record i    ntr_tlas_build's record of the current instance i
 *   boxes       the box of a child ~i is instance i's world box as ntr_tlas_build forms it; the box of an inner child is the union of
 *               the two boxes in that child's node (-0 < +0).  PLOC forms a cluster's box by the same union, so the refit of a fresh
 *               build with unchanged instances changes no byte
 *   untouched   words 12..15 of every node, every node slot no link reaches, everything beyond the extents
 *   d_sceneBox  optional, 6 floats, min.xyz max.xyz: the union of node 0's two boxes (N == 1: instance 0's box)
 *   counts      numNodes: 1 + the links that name a slot; numLeaves: the leaf links (N == 1: 0 and 1, the root link)
 * With result == NULL the call is asynchronous on `stream` and capturable: two launches (one for N == 1), no read-back, no memset; the
 * first launch clears the arrival counters.  With result != NULL it blocks and reads the counts, the error bits, the scene box and the
 * GPU time back.  A bad part is never followed, and nothing outside the buffers is read or written whatever a link, an index or a
 * record holds: an instance whose blas index lies outside [0, numBlas) keeps its record and its leaf box, a link > 0 that names no slot
 * and a leaf link ~i with i >= numInstances are skipped; the boxes of the ancestors of such a place stay as they were (a box is
 * rewritten exactly where everything below it is well formed), and everything else is refitted completely.  The blocking form then
 * returns NTR_ERR_INVALID (bit 1, ntr_tlas_build's "blas index" message) or NTR_ERR_LAYOUT (bits 2, 4) with *result filled, sceneMin /
 * sceneMax zero where the root was not refitted; the asynchronous form skips such a part silently.  Slots that only a bad link named
 * are out of the rule: they may be refitted among themselves.
 * The scratch -- 8 B per node slot (parent word, arrival counter), 16 B per BLAS (the range table), 16 KB of counters -- is a per-device
 * grow-only pool of its own that ntr_lbvh_release_workspace returns.  The range table is uploaded only when it differs from the one
 * the previous call on this device uploaded (that call then waits for its upload; a frame loop over one pool pays it once).  A captured
 * call uploads nothing and allocates nothing: it is accepted only when the last uncaptured call on this device had the same ranges and
 * instance count and the pool has not been released since, else NTR_ERR_INVALID says so.  While such a graph lives, make no call with
 * other ranges and do not release the workspace.  One call per device at a time.
 * NTR_ERR_INVALID (before any device work; *result zeroed): a null pointer (d_sceneBox and result may be null, d_tlasNodes only when
 * numInstances == 1), numInstances < 1 or numInstances - 1 above Compact's node limit, numBlas < 1, tlasNodesBytes other than
 * 64 * (numInstances - 1), rootLink other than 0 (N >= 2) or ~0 (N == 1), recordsCapacity < 64 * numInstances, buffers not 16-byte
 * aligned, a pool size or BLAS range that ntr_tlas_build refuses, a captured call with a result.  Without a device, after these
 * checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrTlasRefitResult {
    int32_t numNodes, numLeaves;        /* reached node slots; leaf links of reached slots (== numInstances for a tree ntr_tlas_build made) */
    int32_t errBits, pad;               /* 0, or: 1 an instance's blas index outside [0, numBlas); 2 a link > 0 that names no slot;
                                           4 a leaf link ~i with i >= numInstances */
    float   sceneMin[3], sceneMax[3];
    float   seconds, pad2;              /* GPU time */
} NtrTlasRefitResult;
NTR_API int ntr_tlas_refit(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                           const void* d_poolNodes, int64_t poolNodesBytes, void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                           void* d_records, int64_t recordsCapacity, float* d_sceneBox /* may be NULL: 6 floats */,
                           NtrTlasRefitResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the TLAS refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_refit_scratch_bytes(int64_t* bytes);

/* Instance update: the NtrInstance array from a hierarchy of transforms, composed and inverted on the device in one launch
 * (csrc/instances_update_kernels.hip), and its restatement on the host (csrc/instances_update_host.cpp).  It is the
 * device form of what a caller otherwise does on the host -- N calls of ntr_instance_invert and an upload of 112 B x N -- and the step
 * that makes the instanced frame loop (ntr_bvh_refit_batch -> instances -> ntr_tlas_refit -> trace) capturable as a whole; flattening
 * a hierarchy is also how "instances of instances" reach the two-level trace.  EXTENSION without a reference counterpart: the rule is
 * the numpy spec tests/np_instance_update.py, which both forms equal byte for byte.
 *   nodes       numNodes transforms: nodeLocal, 3x4 row-major binary32 (12 floats each), and nodeParent, -1 for a root (NULL: every
 *               node is a root).  The order of the nodes is free: a parent may come after its child.
 *   instances   instanceNode[i] names instance i's node (NULL: instance i uses node i, which needs numNodes >= numInstances);
 *               blas[i] is copied through, reserved is zero
 *   chain       from the instance's node up to a root: at most NTR_INSTANCE_MAX_CHAIN transforms
 *   fold        from the root down, in binary64 without contraction: acc = local[root]; acc = acc o local[k] for every node below,
 *               W[r][c] = (P[r][0] L[0][c] + P[r][1] L[1][c]) + P[r][2] L[2][c] and
 *               W[r][3] = ((P[r][0] L[0][3] + P[r][1] L[1][3]) + P[r][2] L[2][3]) + P[r][3]; objectToWorld is acc rounded to binary32
 *               once; worldToObject is ntr_instance_invert(objectToWorld) bit for bit.  One node per instance and no parents gives
 *               exactly the array a loop over ntr_instance_invert makes.
 *   errors      per instance.  NTR_INSTANCE_ERR_CHAIN: a node index outside [0, numNodes), a parent outside [-1, numNodes) or a
 *               chain of more than 16 transforms (a cycle); both matrices of the instance are twelve +0.
 *               NTR_INSTANCE_ERR_SINGULAR: a zero or non-finite determinant; objectToWorld as rounded, worldToObject twelve +0.
 *   status      four words: the OR of the bits; the lowest bad instance index, 0xFFFFFFFF if none; the number of bad instances; zero
 * ntr_instances_update: one thread per instance, which walks its own chain; a shared ancestor is recomputed by every instance below
 *   it, so there is one launch, no scratch and one association order.  d_status (16 bytes, 16-byte aligned) is reset on `stream` ahead
 *   of the kernel.  With result == NULL the call is asynchronous on `stream` and capturable from the first call on: it allocates nothing
 *   and keeps nothing on the host.  With result != NULL it blocks, reads the status back and returns NTR_ERR_INVALID naming the first
 *   bad instance when a bit is set, *result filled all the same.  A bad index is never followed: nothing outside the arrays is read.
 *   d_nodeLocal and d_instances must be 16-byte aligned.  An array that is written to the NtrInstance array of a scene must not be
 *   traced through a bad instance: read the status first (ntr_instances_status_read blocks on `stream`).
 * ntr_instances_update_host: the same rule over host arrays, no device; NTR_ERR_INVALID naming the first bad instance when
 *   status[0] != 0, out and status filled all the same.
 * NTR_ERR_INVALID before anything is touched: a null required pointer, numInstances < 1, numNodes < 1, instanceNode == NULL with
 *   numNodes < numInstances, misaligned device buffers, a captured call with a result.  Without a device, after these checks, the
 *   device calls return NTR_ERR_NO_DEVICE / NTR_ERR_HIP. */
#define NTR_INSTANCE_MAX_CHAIN 16
#define NTR_INSTANCE_ERR_SINGULAR 1u
#define NTR_INSTANCE_ERR_CHAIN 2u
typedef struct NtrInstancesUpdateResult {
    int32_t  numInstances, numNodes;
    uint32_t statusBits, firstBad, numBad, pad;   /* the status words 0..2 */
    float    seconds, updateMs;                   /* host wall clock of the call; GPU event time of the reset and the kernel */
} NtrInstancesUpdateResult;
NTR_API int ntr_instances_update(int32_t numNodes, const float* d_nodeLocal, const int32_t* d_nodeParent /* may be NULL */,
                                 int32_t numInstances, const int32_t* d_instanceNode /* may be NULL */, const int32_t* d_blas,
                                 NtrInstance* d_instances, uint32_t* d_status /* 16 bytes */,
                                 NtrInstancesUpdateResult* result /* NULL: asynchronous */, void* stream);
NTR_API int ntr_instances_status_read(const uint32_t* d_status, uint32_t status[4], void* stream);
NTR_API int ntr_instances_update_host(int32_t numNodes, const float* nodeLocal, const int32_t* nodeParent /* may be NULL */,
                                      int32_t numInstances, const int32_t* instanceNode /* may be NULL */, const int32_t* blas,
                                      NtrInstance* out, uint32_t status[4]);

/* Motion blur in instanced scenes: a time-sampled two-level trace (csrc/tlas_motion_refit_kernels.hip,
 * csrc/trace_instanced_motion_kernels.hip).  Every other piece of the instanced path poses the scene at one instant; here
 * each ray carries a time, and a moving instance is posed at that time when the ray enters it.  EXTENSION without a reference
 * counterpart: the rule is the numpy spec tests/np_instanced_motion.py, which the refit equals byte for byte and the trace bit for bit
 * in all four result words, the instance id and every counter.
 *   keys        two NtrInstance arrays of numInstances entries: key 0 is the shutter's opening, key 1 its close (two
 *               ntr_instances_update calls give exactly these).  The blas index and worldToObject are taken from key 0; of key 1 only
 *               objectToWorld is read.  Instance i is MOVING iff any of the twelve objectToWorld words differs bitwise between the keys.
 *   time        ray r has t_r = d_rayTimes[r], or the launch's scalar `time`; clamped by t > 0 ? (t < 1 ? t : 1) : 0, so a NaN gives 0
 *   pose        for a moving instance, with u = 1.0f - t, each component of M(t) is a where t == 0 or a and b are the same word, b
 *               where t == 1, otherwise u * a + t * b in binary32 with both products rounded before the sum.  M(0) and M(1) are the
 *               keys bit for bit, and a component that does not move never changes.  worldToObject(t) is ntr_instance_invert's
 *               function of M(t): binary64, each of the 12 results rounded once
 *   boxes       the leaf box of a moving instance is the union, in the integer order, of its world box (ntr_tlas_refit's) under key 0
 *               and under key 1: every corner moves on a straight line between its two end positions, up to rounding, so the union
 *               bounds the sweep; no padding.  A static instance's box and the climb are ntr_tlas_refit's
 *   records     record i is ntr_tlas_refit's record of key-0 instance i, except that word 15 is 1 for a moving instance, 0 otherwise.
 *               No kernel but the motion trace reads word 15.  A later plain ntr_tlas_refit (or ntr_tlas_build) writes word 15 = 0 and
 *               thereby FREEZES the scene at key 0, boxes included
 *   motion keys beside the records, 128 bytes per instance: words 0..11 objectToWorld of key 0, words 16..27 objectToWorld of key 1,
 *               every other word zero; written for every instance, static ones and ones with a bad blas index too
 *   entering    the trace is ntr_trace_instanced_masked's with one change to the step "top level, link ~i"; the checks run in this
 *               order: index in range; masks; room for the marker; then, if word 15 of the fetched record is non-zero, the two keys
 *               are read from the motion key buffer at 128 * i (range checked: beyond min(motionKeysBytes, 0xFFFFFF00) a read returns
 *               zeros), M(t_r) is formed and inverted -- a zero or non-finite determinant makes the step a pop: no marker, no
 *               transform, nothing else touched, counted as numSingular and as neither an entry nor a masked step; then the marker is
 *               pushed and the ray transformed by worldToObject(t_r).  A static instance's step is the masked kernel's, from the
 *               record alone
 *   bytes       the masked formula plus 128 (numMovingEntries + numSingular), plus 4 numRays when per-ray times are given
 * ntr_tlas_motion_refit: ntr_tlas_refit over d_instances0 with the three changes above (swept leaf boxes, word 15, the motion key
 *   buffer), and ntr_tlas_refit's contract in every respect not named here: result == NULL is asynchronous on `stream` and capturable
 *   (two launches, one for N == 1, no read-back, no memset), the tolerant walk and its error bits, the cached range table and its
 *   rule for captured calls, one call per device at a time.  Its scratch is a per-device grow-only pool of its own
 *   (ntr_tlas_motion_refit_scratch_bytes) that ntr_lbvh_release_workspace returns.  It also requires d_instances1 non-null and 16-byte
 *   aligned, d_motionKeys non-null and 16-byte aligned, motionKeysCapacity >= 128 * numInstances.  numMoving counts the moving
 *   instances among all numInstances.  The topology is whatever ntr_tlas_build made at key 0.
 * ntr_trace_instanced_motion: ntr_trace_instanced_masked's arguments plus `motion`.  With motion == NULL the call IS
 *   ntr_trace_instanced_masked -- the same launch, and its refusals name that function.  seconds == NULL is asynchronous on `stream` and
 *   capturable; the times, the keys and the records are read by the launch, so a replay sees what is there at replay time.
 * ntr_trace_instanced_motion_stats: the same records through the instrumented kernel, plus ntr_trace_instanced_stats's counters and the
 *   two of NtrInstancedMotionStats.  It blocks and is refused on a capturing stream.  With motion == NULL it is
 *   ntr_trace_instanced_stats and the motion counters are zero.
 * Errors: NTR_ERR_INVALID before any device work for everything ntr_trace_instanced_masked refuses, in its words and order, then: a
 *   d_rayTimes that is not 4-byte aligned, a d_motionKeys that is null or not 16-byte aligned, motionKeysBytes < 128 * numInstances;
 *   a null stats or motionStats.  numRays == 0 returns NTR_OK with the stats zeroed; without a device, after these checks,
 *   NTR_ERR_NO_DEVICE / NTR_ERR_HIP.
 * Not combinable with the seeded / world form or FAST (over the 4-wide trees: ntr_tlas_wide_motion_refit and
 * ntr_trace_instanced_wide_motion, below); ntr_instanced_hit_attributes gives the normal at key 0,
 * ntr_instanced_hit_attributes_motion (below) the normal at the ray's time. */
typedef struct NtrTlasMotionRefitResult {
    NtrTlasRefitResult refit;           /* as ntr_tlas_refit reports it */
    int32_t numMoving, pad;             /* instances whose objectToWorld differs between the keys */
} NtrTlasMotionRefitResult;
typedef struct NtrInstanceMotion {      /* host struct of device pointers */
    const void*  d_motionKeys;          /* what ntr_tlas_motion_refit wrote: 128 bytes per instance, 16-byte aligned */
    int64_t      motionKeysBytes;       /* at least 128 * numInstances */
    const float* d_rayTimes;            /* numRays floats, or NULL: every ray has `time` */
    float        time, pad;
} NtrInstanceMotion;
typedef struct NtrInstancedMotionStats {
    int64_t numMovingEntries;           /* entering steps that entered a moving instance (counted in numInstanceEntries too) */
    int64_t numSingular;                /* entering steps popped because M(t) has no inverse */
} NtrInstancedMotionStats;
NTR_API int ntr_tlas_motion_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1, int32_t numBlas,
                                  const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes, void* d_tlasNodes,
                                  int64_t tlasNodesBytes, int32_t rootLink, void* d_records, int64_t recordsCapacity, void* d_motionKeys,
                                  int64_t motionKeysCapacity, float* d_sceneBox /* may be NULL: 6 floats */,
                                  NtrTlasMotionRefitResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the motion refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_motion_refit_scratch_bytes(int64_t* bytes);
NTR_API int ntr_trace_instanced_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                       const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                       int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                       int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                       const NtrInstanceVisibility* vis /* NULL: no masks */,
                                       const NtrInstanceMotion* motion /* NULL: ntr_trace_instanced_masked */,
                                       float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                             int32_t* d_instanceIDs, const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                                             const void* d_records, int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes,
                                             const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                             const NtrInstanceVisibility* vis /* may be NULL */,
                                             const NtrInstanceMotion* motion /* may be NULL */, NtrInstancedTraceStats* stats,
                                             NtrInstancedMotionStats* motionStats, void* stream);

/* Deforming BLASes in the motion-blurred two-level trace (csrc/tlas_deform_refit_kernels.hip, csrc/trace_instanced_deform_kernels.hip,
 * DESIGN.md 6ag): instances that move AND meshes that deform within the shutter, in one instanced scene.  It joins the two halves above
 * and below: ntr_tlas_motion_refit / ntr_trace_instanced_motion (rigid motion, every BLAS frozen at key 0) and ntr_bvh_motion_refit /
 * ntr_trace_bvh_motion (deformation over one tree).  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_deform.py, which the refit equals byte for byte and the trace bit for bit in all four result words, the instance
 * id and every counter.
 *   pool, key 1  beside d_poolNodes, d_poolTriWoop and d_poolTriIndex the pool has d_poolNodes1 (poolNodesBytes) and d_poolVertRows0,
 *                d_poolVertRows1 (poolTriWoopBytes each).  For a deforming BLAS the four slices at its NtrBlasRange hold what
 *                ntr_bvh_motion_refit wrote when it was handed pool + offset.  For a BLAS that is not deforming nothing of the three
 *                buffers is ever read; the caller need not initialise those bytes
 *   deforming    d_blasDeforming: numBlas words ON THE DEVICE, non-zero: that BLAS deforms.  The refit's kernels read it, so a replay
 *                of a captured refit sees the current flags
 *   leaf box     instance i has BLAS b.  K = {key 0's objectToWorld, key 1's} if the instance is moving, else {key 0's}; J =
 *                {d_poolNodes, d_poolNodes1} if b deforms, else {d_poolNodes}.  The box is the union, in the integer order, of the
 *                instance's world box (ntr_tlas_refit's) over ALL pairs of K x J: up to four boxes.  A posed point is M(t) c(t) with
 *                both factors linear in t -- a quadratic Bezier curve that lies in the hull of the four products, not of its two ends.
 *                No padding
 *   word 15      bit 0: moving, as ntr_tlas_motion_refit writes it; bit 1: the instance's BLAS deforms.  Records with bit 1 set are
 *                meant for ntr_trace_instanced_deform ONLY: ntr_trace_instanced_motion takes any non-zero word 15 for "moving".  A later
 *                ntr_tlas_refit or ntr_tlas_motion_refit rewrites word 15 without bit 1
 *   trace        ntr_trace_instanced_motion's, with two changed bottom-level steps for a lane inside an instance whose record has bit 1
 *                (remembered from the entering step to the exit marker; bit 0 alone decides the instance's pose): the inner step poses
 *                the twelve box words from d_poolNodes and d_poolNodes1 at nodesOffset + node (links from d_poolNodes) and the triangle
 *                step is ntr_trace_bvh_motion's at the pool's row offset -- a terminator iff the W word of d_poolVertRows0's row is
 *                0x80000000, otherwise nine posed vertex words, their Woop rows and the unchanged test.  The pose is
 *                ntr_trace_bvh_motion's (no "same word" shortcut).  In every other instance each step is ntr_trace_instanced_motion's
 *   bytes        the motion formula plus 64 per deforming inner visit and 48 per deforming triangle test
 * ntr_tlas_deform_refit: ntr_tlas_motion_refit plus d_poolNodes1 and d_blasDeforming, and its contract in every respect not named here
 *   (result == NULL is asynchronous and capturable: launches only, no memset or copy node; the tolerant walk; the cached range table;
 *   a scratch pool of its own, ntr_tlas_deform_refit_scratch_bytes).  With no flag set every byte it writes is ntr_tlas_motion_refit's.
 *   It also requires d_poolNodes1 non-null and 16-byte aligned and d_blasDeforming non-null and 4-byte aligned.
 * ntr_trace_instanced_deform / _deform_stats: ntr_trace_instanced_motion's arguments plus `deform`.  With deform == NULL the call IS
 *   ntr_trace_instanced_motion (_motion_stats, and the three deform counters are zero).  NTR_ERR_INVALID before any device work for
 *   everything ntr_trace_instanced_motion refuses, in its words and order, then: a null motion with a non-null deform; a null
 *   d_poolNodes1, d_poolVertRows0 or d_poolVertRows1; one of them not 16-byte aligned; one of them overlapping another buffer of the
 *   call; a null stats, motionStats or deformStats.  The _stats form blocks and is refused on a capturing stream.
 * Not combinable with the 4-wide trees, FAST, or the seeded / world form; the normal of a deforming BLAS's hit at the ray's time is
 * ntr_instanced_hit_attributes_deform's (below); two keys only. */
typedef struct NtrTlasDeformRefitResult {
    NtrTlasMotionRefitResult motion;    /* as ntr_tlas_motion_refit reports it */
    int32_t numDeforming, pad;          /* instances whose BLAS deforms */
} NtrTlasDeformRefitResult;
typedef struct NtrInstanceDeform {      /* host struct of device pointers; the extents are the call's poolNodesBytes and poolTriWoopBytes */
    const void *d_poolNodes1, *d_poolVertRows0, *d_poolVertRows1;
} NtrInstanceDeform;
typedef struct NtrInstancedDeformStats {
    int64_t numDeformEntries;           /* entering steps that entered an instance of a deforming BLAS (in numInstanceEntries too) */
    int64_t numDeformInnerVisits;       /* inner steps inside such instances (in numInnerVisits too) */
    int64_t numDeformTriTests;          /* triangle tests inside such instances (in numTriTests too) */
} NtrInstancedDeformStats;
NTR_API int ntr_tlas_deform_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1, int32_t numBlas,
                                  const NtrBlasRange* blasRanges, const void* d_poolNodes, const void* d_poolNodes1, int64_t poolNodesBytes,
                                  const uint32_t* d_blasDeforming, void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                                  void* d_records, int64_t recordsCapacity, void* d_motionKeys, int64_t motionKeysCapacity,
                                  float* d_sceneBox /* may be NULL: 6 floats */, NtrTlasDeformRefitResult* result /* NULL: asynchronous */,
                                  void* stream);
/* Bytes the deform refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_deform_refit_scratch_bytes(int64_t* bytes);
NTR_API int ntr_trace_instanced_deform(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                       const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                       int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                       int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                       const NtrInstanceVisibility* vis /* NULL: no masks */, const NtrInstanceMotion* motion,
                                       const NtrInstanceDeform* deform /* NULL: ntr_trace_instanced_motion */,
                                       float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_deform_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                             int32_t* d_instanceIDs, const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                                             const void* d_records, int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes,
                                             const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                             const NtrInstanceVisibility* vis /* may be NULL */, const NtrInstanceMotion* motion,
                                             const NtrInstanceDeform* deform /* may be NULL */, NtrInstancedTraceStats* stats,
                                             NtrInstancedMotionStats* motionStats, NtrInstancedDeformStats* deformStats, void* stream);

/* Many PLOC builds in one pass: every mesh of a batch becomes one BLAS of a pool, all of them in the same launches
 * (csrc/bvh_ploc_batch_kernels.hip; it stands here, not beside ntr_ploc_build, because it fills NtrBlasRange).  ntr_ploc_build is a
 * chain of some hundred launches and a read-back per four rounds whatever the mesh's size; a scene of a thousand small meshes pays that
 * chain a thousand times, the batch once.  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_ploc_batch.py -- np_bvh_ploc.build per mesh, np_instanced.make_pool over the results -- which the build equals byte for byte.
 *   layout      mesh k of n_k triangles occupies nodes [nodesOffset_k, +64 * max(n_k - 1, 1)) and rows [triWoopOffset_k, +16 * rows_k),
 *               rows_k = 4 n_k (5 for n_k == 1), packed in mesh order without gaps: the offsets are the running sums; its triIndex
 *               entries start at entry triWoopOffset_k / 16
 *   bytes       those ranges hold what ntr_ploc_build writes when given d_triVtxIndex + 3 * firstTri, numTris, the same vertices, the
 *               mesh's box, radius and the pool pointers plus the offsets: links relative to the BLAS's own start, leaf rows to its own
 *               row base, triangle ids to its own firstTri; the one-triangle tree included.  meshResults[k] are that build's counts,
 *               ranges[k] feeds ntr_tlas_build unchanged
 *   meshes      may name overlapping or identical triangle ranges (two BLASes of one mesh) and need not cover the array
 * NTR_ERR_INVALID (before any device work): a null pointer (meshResults may be NULL), numMeshes outside 1..2^20, a mesh with numTris < 1
 *   or a range outside [0, numTrisTotal), 2^28 triangles or more in all, radius outside 1..64, a box with a non-finite coordinate or
 *   min > max on an axis, capacities below ntr_ploc_batch_capacity, pool nodes or triWoop not 16-byte aligned, a capturing stream (the call
 *   blocks: one 32 B read-back per four rounds); (found on the device, before anything is written to the pool) a vertex index outside
 *   [0, numVerts) in any mesh.  NTR_ERR_OVERFLOW (before any device work): a pool extent above 0xFFFFFF00 or a mesh of more than
 *   0x76543200 / 64 nodes; (after the work) a mesh whose tree is higher than 100 -- the message names the first such mesh; ranges,
 *   meshResults and the pool's bytes are the rule's all the same, as with ntr_ploc_build.  NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a
 *   device: there is no CPU fallback.  NTR_ERR_LAYOUT: an internal consistency check failed (not expected).  A failed call zeroes *result.
 * The scratch (about 105 B per triangle and 76 B per mesh) is a per-device grow-only pool of its own that ntr_lbvh_release_workspace
 *   returns: one build per device at a time. */
typedef struct NtrPlocBatchMesh {      /* host array, one per mesh */
    int32_t firstTri, numTris;         /* triangles [firstTri, +numTris) of the shared d_triVtxIndex */
    float   sceneMin[3], sceneMax[3];  /* the box this mesh's Morton codes are taken over, as ntr_ploc_build's */
} NtrPlocBatchMesh;
typedef struct NtrPlocBatchMeshResult { int32_t numNodes, numLeaves, numRounds, height; } NtrPlocBatchMeshResult;  /* host array */
typedef struct NtrPlocBatchResult {
    int32_t numMeshes, numRounds, maxHeight, pad;       /* rounds launched = max over meshes; greatest height */
    int64_t numTris, nodesBytes, triWoopBytes, triIndexBytes;   /* exact extents of the pool written */
    float   seconds;                                    /* host wall clock */
    float   checkMs, sortMs, emitMs, roundsMs;          /* GPU event times: codes, index check and its read-back; the sort; leaf clusters
                                                           and Woop rows; the rounds */
} NtrPlocBatchResult;
/* host only, no device: the exact pool extents and, when ranges != NULL, the NtrBlasRange of every mesh */
NTR_API int ntr_ploc_batch_capacity(int32_t numMeshes, const NtrPlocBatchMesh* meshes, NtrBlasRange* ranges,
                                    int64_t* nodesBytes, int64_t* triWoopBytes, int64_t* triIndexBytes);
NTR_API int ntr_ploc_build_batch(int32_t numMeshes, const NtrPlocBatchMesh* meshes, int32_t numTrisTotal, const int32_t* d_triVtxIndex,
                                 int32_t numVerts, const float* d_vtxPos, int32_t radius,
                                 void* d_poolNodes, int64_t nodesCapacity, void* d_poolTriWoop, int64_t triWoopCapacity,
                                 int32_t* d_poolTriIndex, int64_t triIndexCapacity,
                                 NtrBlasRange* ranges /* numMeshes, out */, NtrPlocBatchMeshResult* meshResults /* may be NULL */,
                                 NtrPlocBatchResult* result, void* stream);
/* Bytes the batch builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_ploc_batch_scratch_bytes(int64_t* bytes);

/* Many refits in one pass: the listed BLASes of a pool are refitted to moved vertices in the same two launches
 * (csrc/bvh_refit_batch_kernels.hip).  The pool is built once (ntr_ploc_build_batch, addBLAS); rigid motion is the TLAS
 * rebuild or refit; a mesh that DEFORMS keeps its triangles and moves its vertices, and this call is its update path: refit, then
 * ntr_tlas_refit (or ntr_tlas_build) from the new node-0 boxes.  ntr_bvh_refit (below) at pool + offset gives the same bytes, two launches per BLAS.  EXTENSION without a
 * reference counterpart: the rule is the numpy spec tests/np_refit_batch.py -- np_bvh_refit.refit over every entry's slices of the pool.
 *   entry       the BLAS's range as ntr_ploc_build_batch / addBLAS report it; its mesh, triangles [firstTri, +numTris) of the shared
 *               d_triVtxIndex (the BLAS's triIndex entries are relative to firstTri); its epsilon, the leaf-box rule of ntr_bvh_refit
 *               (0 for PLOC and host SAH trees, 0.001 for the LBVH's)
 *   bytes       every entry's ranges hold what ntr_bvh_refit writes when called on pool + offset with d_triVtxIndex + 3 * firstTri,
 *               numTris and the entry's epsilon.  Every other byte of the pool is untouched, those inside a listed range that
 *               ntr_bvh_refit leaves alone included (links, terminators, triIndex, unreached slots)
 *   entries     any subset of the pool's BLASes in any order; two entries may name the same or overlapping triangles; two entries whose
 *               node ranges or row ranges overlap are refused (two threads would refit one tree)
 *   d_poolTriIndex  one entry per pool row (poolTriWoopBytes / 4 bytes), as the pool's builders leave it
 *   d_blasBoxes optional, 6 floats per entry in entry order, min.xyz max.xyz: the union of the two boxes of the BLAS's node 0
 *   lanesPerLeaf  1, 4 or 8, chosen once per call from the selection's mean leaf size by ntr_bvh_refit's thresholds: speed only
 * With result == NULL the call is asynchronous on `stream`: two launches, no read-back, no memset.  With result != NULL it blocks and
 * reads the counts and the GPU time back.  A malformed tree is never followed (the errors are ntr_bvh_refit's): the blocking form
 * returns NTR_ERR_LAYOUT, fills *result all the same, and names the lowest bad entry in firstBadEntry and the message; every other
 * entry has been refitted completely, since entries share no node.  With result == NULL such a part is skipped silently.
 * The device's entry table (32 B per entry and a running sum) and the topology arrays (8 B per listed node slot, 16 KB of counters)
 * live in a per-device grow-only pool of its own that ntr_lbvh_release_workspace returns.  The table is uploaded only when it differs
 * from the one the previous call on this device uploaded (that call then waits for its upload; a frame loop over one selection pays
 * it once).  A captured call uploads nothing and allocates nothing: it is accepted only when the last uncaptured call on this device
 * had the same entries and the pool has not been released since, else NTR_ERR_INVALID says so.  While such a graph
 * lives, make no call with other entries and do not release the workspace: the graph's launches read the table and the arrays in
 * place.  One call per device at a time.
 * NTR_ERR_INVALID (before any device work): a null pointer (d_blasBoxes and result may be null), numEntries outside 1..2^20, pool
 * sizes that are not multiples of 64 / 16 within 0xFFFFFF00, pool pointers not 16-byte aligned, a range that is misaligned, outside
 * the pool's extents or above the limits of ntr_tlas_build, triWoopBytes < 16, a mesh outside [0, numTrisTotal) or with numTris < 1,
 * a negative or non-finite epsilon, overlapping or duplicate entries, numVerts < 1.  Without a device, after these checks:
 * NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback).  Every failure but NTR_ERR_LAYOUT zeroes *result. */
typedef struct NtrRefitBatchEntry {      /* host array, one per BLAS to refit: 48 bytes */
    NtrBlasRange range;
    int32_t firstTri, numTris;
    float   epsilon;
    int32_t pad;
} NtrRefitBatchEntry;
typedef struct NtrBvhRefitBatchResult {
    int32_t numEntries, lanesPerLeaf;    /* lanesPerLeaf says which kernel ran */
    int64_t numNodes, numLeaves, numRows;/* sums over the entries of what ntr_bvh_refit counts */
    int32_t firstBadEntry, errBits;      /* -1 / 0, or the lowest entry whose tree is malformed and the OR of ntr_bvh_refit's error bits */
    float   seconds, pad;                /* GPU time */
} NtrBvhRefitBatchResult;
NTR_API int ntr_bvh_refit_batch(int32_t numEntries, const NtrRefitBatchEntry* entries,
                                void* d_poolNodes, int64_t poolNodesBytes, void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                const int32_t* d_poolTriIndex, int32_t numTrisTotal, const int32_t* d_triVtxIndex,
                                int32_t numVerts, const float* d_vtxPos, float* d_blasBoxes /* may be NULL: 6 floats per entry */,
                                NtrBvhRefitBatchResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the batch refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_refit_batch_scratch_bytes(int64_t* bytes);

/* Many two-key refits in one pass: the update path of a pool whose BLASes deform inside the shutter (ntr_trace_instanced_deform above),
 * the listed BLASes in the same three launches and a fourth for the boxes (csrc/bvh_motion_refit_batch_kernels.hip).
 * ntr_bvh_motion_refit (below) at pool + offset gives the same bytes, three launches per BLAS.  EXTENSION without a reference
 * counterpart: the rule is the numpy spec tests/np_motion_refit_batch.py -- np_bvh_motion.motion_refit over every entry's slices.
 *   pool        the five buffers ntr_trace_instanced_deform reads: d_poolNodes0 and d_poolNodes1 (poolNodesBytes each), d_poolTriWoop,
 *               d_poolVertRows0 and d_poolVertRows1 (poolTriWoopBytes each), and d_poolTriIndex, which is never written
 *   bytes       every entry's slices of the five buffers hold what ntr_bvh_motion_refit writes when handed pool + offset,
 *               d_triVtxIndex + 3 * firstTri, numTris and the entry's epsilon: nodes0 and the Woop rows refitted to d_vtxPos0 in place,
 *               nodes1 a copy of nodes0 refitted to d_vtxPos1, the vertex rows zero but for the leaves' vertices under either key and
 *               the terminator (0, 0, 0, 0x80000000) in the w word; a leaf whose walk met an error keeps zero rows.  Every byte outside
 *               the listed ranges is untouched: the three key-1 buffers need no initialisation by the caller
 *   d_blasBoxes optional, 6 floats per entry in entry order, min.xyz max.xyz: the union, in the total order, of the two keys' node-0
 *               boxes -- ntr_bvh_motion_refit's d_sceneBox for that BLAS
 *   counts      the sums of what ntr_bvh_motion_refit reports per entry (both keys walk the same leaves: counted once)
 * Entries, lanesPerLeaf, the two forms (result == NULL is asynchronous and capturable: launches only, no memset or copy node, no
 * read-back; result != NULL blocks, times and reports), the malformed tree (never followed; NTR_ERR_LAYOUT with *result filled and the
 * lowest bad entry named, every other entry refitted completely; skipped silently by the asynchronous form), the held entry table and
 * the rule for a captured call are ntr_bvh_refit_batch's in every respect.  The table (32 B per entry and two running sums, over node
 * slots and over rows), the topology arrays (12 B per listed node slot), 48 B of boxes per entry and 16 KB of counters live in a
 * per-device grow-only pool of its own (ntr_bvh_motion_refit_batch_scratch_bytes) that ntr_lbvh_release_workspace returns.
 * NTR_ERR_INVALID (before any device work): ntr_bvh_refit_batch's cases in its order, then a null d_poolNodes1, d_poolVertRows0,
 * d_poolVertRows1 or d_vtxPos1; one of d_poolNodes0, d_poolNodes1, d_poolTriWoop, d_poolVertRows0, d_poolVertRows1 not 16-byte aligned;
 * one of d_poolNodes1, d_poolVertRows0, d_poolVertRows1, d_vtxPos1 overlapping another buffer of the call (the pools' whole extents). */
NTR_API int ntr_bvh_motion_refit_batch(int32_t numEntries, const NtrRefitBatchEntry* entries,
                                       void* d_poolNodes0, int64_t poolNodesBytes, void* d_poolNodes1,
                                       void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                       void* d_poolVertRows0, void* d_poolVertRows1,
                                       int32_t numTrisTotal, const int32_t* d_triVtxIndex, int32_t numVerts,
                                       const float* d_vtxPos0, const float* d_vtxPos1,
                                       float* d_blasBoxes /* may be NULL: 6 floats per entry */,
                                       NtrBvhRefitBatchResult* result /* NULL: asynchronous, capturable */, void* stream);
/* Bytes the batched motion refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_motion_refit_batch_scratch_bytes(int64_t* bytes);

/* Instanced frames: what a two-level hit needs before anything indexes by triangle, in one launch with a thread per ray
 * (csrc/instanced_attr_kernels.hip).  ntr_trace_instanced leaves (id, t, u, v) and an instance id per ray; that id is the
 * BLAS's own triangle id, relative to its mesh's firstTri.  This call turns it into the pool triangle g -- so that ntr_reconstruct,
 * ntr_count_hits and ntr_secondary_block_costs work unchanged over d_outResults, with tables per pool triangle -- and forms the hit
 * triangle's world-space geometric normal from the CURRENT vertices, which ntr_raygen_ao_normals (above) takes: primary -> two-level
 * trace -> attributes -> AO or diffuse rays -> two-level trace -> ntr_reconstruct, all on one stream or in one graph, after
 * ntr_bvh_refit_batch and ntr_tlas_refit when the frame moved.  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_frame.py, which the device equals in every word.  Binary32 throughout, every operation rounded once.
 *   resolved    ray r is resolved iff id = d_results[r].id != -1, i = d_instanceIDs[r] in [0, numInstances), b = d_instances[i].blas in
 *               [0, numBlas), id in [0, d_blasTris[b].numTris), g = d_blasTris[b].firstTri + id in [0, numTrisTotal), and the three
 *               vertex indices of triangle g in [0, numVerts).  No read happens before its index is checked: whatever the records,
 *               the instances, the table and the index array hold, nothing outside the buffers is read
 *   d_outResults[r]  d_results[r] with id replaced by g when resolved and by -1 otherwise; t and the two pad words verbatim
 *   normal      e1 = v[b] - v[a], e2 = v[c] - v[a]; n_o = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z, e1.x e2.y - e1.y e2.x)
 *               (Scene.cpp:112's cross product); with W the instance's worldToObject, n_w.k = (W[0][k] n_o.x + W[1][k] n_o.y) +
 *               W[2][k] n_o.z -- the transpose of W's linear part, so the inverse transpose of objectToWorld;
 *               l2 = (n_w.x n_w.x + n_w.y n_w.y) + n_w.z n_w.z.  A resolved ray whose l2 is finite and > 0 gets inv = 1.0f / sqrtf(l2)
 *               and d_normals[4r ..] = (n_w.x inv, n_w.y inv, n_w.z inv, 1.0f); every other ray gets (0, 0, 0, 0)
 *   orientation the normal follows the OBJECT's winding: under a mirroring instance (negative determinant) it is the world triangle's
 *               geometric normal negated.  The AO generator turns the normal against the ray anyway
 *   colours     the caller's per-triangle tables are per POOL triangle and in object space: two instances of one BLAS share a
 *               triangle's colours, however they are turned (colour tables lit per instance are out of scope)
 *   d_blasTris  BLAS k is triangles [firstTri, +numTris) of d_triVtxIndex, the meshes ntr_ploc_build_batch was given; numTris 0 (a
 *               tree whose mesh is not known) resolves none of its hits
 * One 16-byte store per output per ray; d_outResults may equal d_results (in place); either output may be NULL, not both.  The call is
 * asynchronous on `stream` and capturable; it allocates nothing and reads nothing back.  numRays == 0 returns NTR_OK.
 * NTR_ERR_INVALID (before any device work): numRays < 0, a null geom or a null pointer inside it, a count < 1, null d_results or
 * d_instanceIDs, both outputs null, d_results, d_outResults, d_normals or d_instances not 16-byte aligned (d_blasTris: 8).  Without a
 * device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrBlasTris { int32_t firstTri, numTris; } NtrBlasTris;        /* device array, one per BLAS */
typedef struct NtrInstancedGeometry {                                         /* host struct of device pointers */
    int32_t numInstances, numBlas, numTrisTotal, numVerts;
    const NtrInstance* d_instances;    /* as ntr_tlas_build / ntr_tlas_refit take them */
    const NtrBlasTris* d_blasTris;     /* BLAS k is triangles [firstTri, +numTris) of d_triVtxIndex (ntr_ploc_build_batch's meshes) */
    const int32_t*     d_triVtxIndex;  /* 3 per triangle: the arrays ntr_ploc_build_batch / ntr_bvh_refit_batch were given */
    const float*       d_vtxPos;       /* 3 per vertex, the CURRENT positions */
} NtrInstancedGeometry;
NTR_API int ntr_instanced_hit_attributes(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs,
                                         const NtrInstancedGeometry* geom,
                                         NtrRayResult* d_outResults /* may be NULL; may equal d_results */,
                                         float* d_normals /* may be NULL; 4 floats per ray */, void* stream);

/* ntr_instanced_hit_attributes with the normal at the RAY'S time (csrc/instanced_motion_attr_kernels.hip): the attributes
 * of the hits ntr_trace_instanced_motion wrote.  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_motion_frame.py (hit_attributes_motion), which the device equals in every word.  `motion` is what the trace took:
 * the key buffer ntr_tlas_motion_refit wrote, d_rayTimes or the scalar `time`.  The call is ntr_instanced_hit_attributes in every
 * respect -- the resolution rule, the id rewrite, the cross product, the transpose, the normalisation, the (0, 0, 0, 0) cases, the
 * in-place and one-NULL-output forms, the range checks before every read -- except where W comes from for a resolved ray r of
 * instance i:
 *   time        t_r = d_rayTimes[r] or `time`, clamped by t > 0 ? (t < 1 ? t : 1) : 0
 *   moving      instance i is moving iff words 0..11 and 16..27 of its 128-byte key entry differ bitwise (this call has no records)
 *   static      W = geom->d_instances[i].worldToObject, as ntr_instanced_hit_attributes
 *   moving      W = ntr_instance_invert's function (binary64) of M(t_r), the trace's lerp of the two keys: the matrix the trace
 *               transformed that ray with.  No inverse: the id is still resolved, the normal is (0, 0, 0, 0)
 *   unchanged   the blas index comes from geom->d_instances (key 0); d_vtxPos is the current mesh (BLASes deforming within the shutter:
 *               ntr_instanced_hit_attributes_deform, below)
 * With motion == NULL the call IS ntr_instanced_hit_attributes, and its refusals name that function.
 * NTR_ERR_INVALID (before any device work): everything ntr_instanced_hit_attributes refuses, in its words and order, then: a d_rayTimes
 * that is not 4-byte aligned, a d_motionKeys that is null or not 16-byte aligned, motionKeysBytes < 128 * geom->numInstances.
 * numRays == 0 returns NTR_OK.  Without a device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP. */
NTR_API int ntr_instanced_hit_attributes_motion(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs,
                                                const NtrInstancedGeometry* geom,
                                                const NtrInstanceMotion* motion /* NULL: ntr_instanced_hit_attributes */,
                                                NtrRayResult* d_outResults /* may be NULL; may equal d_results */,
                                                float* d_normals /* may be NULL; 4 floats per ray */, void* stream);

/* ntr_instanced_hit_attributes_motion with the TRIANGLE at the ray's time too (csrc/instanced_deform_attr_kernels.hip):
 * the attributes of the hits ntr_trace_instanced_deform wrote.  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_deform_frame.py (hit_attributes_deform), which the device equals in every word.  `motion` is what the trace took;
 * `deform` names the second vertex key and the per-BLAS flags ntr_tlas_deform_refit read.  The call is
 * ntr_instanced_hit_attributes_motion in every respect -- the resolution rule, the id rewrite, the moving test, W at the ray's time,
 * the transpose, the normalisation, the (0, 0, 0, 0) cases, the in-place and one-NULL-output forms, the range checks before every read
 * -- except where the three vertices come from for a resolved ray r of instance i with b = geom->d_instances[i].blas:
 *   time        t_r = d_rayTimes[r] or `time`, clamped by t > 0 ? (t < 1 ? t : 1) : 0: the time the trace posed that ray's triangle with
 *   static      d_blasDeforming[b] == 0: the vertices are geom->d_vtxPos's; nothing of d_vtxPos1 is read
 *   deforming   d_blasDeforming[b] != 0: each of the nine words is ntr_trace_bvh_motion's pose of the two keys' words -- a at t_r == 0,
 *               b at t_r == 1, (1 - t_r) * a + t_r * b with both products rounded in between (no "same word" shortcut).  The vertex
 *               rows ntr_bvh_motion_refit writes are the vertices' words verbatim, so this is, bit for bit, the triangle the ray was
 *               tested against
 *   unchanged   the cross product, in its rounding order, over the posed words; a posed triangle whose cross product has length 0 or
 *               a non-finite length resolves the id and gives (0, 0, 0, 0)
 * geom->d_vtxPos is the shutter's opening and d_vtxPos1 its close: the two arrays ntr_bvh_motion_refit(_batch) was given, numVerts
 * vertices each.  The flags are read on the device, so a replay of a captured call sees the current ones.
 * With deform == NULL the call IS ntr_instanced_hit_attributes_motion, and its refusals name that function.
 * NTR_ERR_INVALID (before any device work): everything ntr_instanced_hit_attributes_motion refuses, in its words and order, then: a null
 * motion with a non-null deform (ntr_trace_instanced_deform's rule), a null d_vtxPos1 or d_blasDeforming, either of them not 4-byte
 * aligned.  numRays == 0 returns NTR_OK.  Without a device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP. */
typedef struct NtrInstancedDeformGeometry {   /* host struct of device pointers */
    const float*    d_vtxPos1;        /* 3 per vertex, geom->numVerts of them: the shutter's close; geom->d_vtxPos is its opening */
    const uint32_t* d_blasDeforming;  /* geom->numBlas words on the device, as ntr_tlas_deform_refit reads them */
} NtrInstancedDeformGeometry;
NTR_API int ntr_instanced_hit_attributes_deform(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs,
                                                const NtrInstancedGeometry* geom, const NtrInstanceMotion* motion,
                                                const NtrInstancedDeformGeometry* deform /* NULL: ntr_instanced_hit_attributes_motion */,
                                                NtrRayResult* d_outResults /* may be NULL; may equal d_results */,
                                                float* d_normals /* may be NULL; 4 floats per ray */, void* stream);

/* 4-wide BVH: an out-of-place pass that turns any BVHLayout_Compact tree into 4-wide nodes, and the trace that walks them
 * (csrc/bvh_widen_kernels.hip, csrc/trace_wide_kernels.hip, csrc/wide_bvh.h).  EXTENSION without a reference counterpart: the rule is the
 * numpy spec tests/np_bvh_wide.py, which ntr_bvh_widen equals byte for byte and ntr_trace_wide in all four result words.  Leaves, Woop rows
 * and triIndex are the binary tree's, unchanged: only a new node buffer is written, and the binary tree stays usable.
 *   wide node   32 words, 128 bytes: words 0..11 the boxes of children 0 and 1 in Compact's box words, 12..15 the links of children 0..3,
 *               16..27 the boxes of children 2 and 3 (16 + Compact's word for child k - 2), 28 the child count (2..4), 29..31 zero.
 *               A link < 0 is a leaf (~link its first Woop row, verbatim from the binary tree), > 0 is 128 * index of a wide node, 0 an
 *               empty slot; slot k >= count holds link 0 and a copy of slot 0's box, so every box word is a box word of the binary tree
 *               and ntr_bvh_validate's flags for the binary tree hold for the wide one.  The buffer is a multiple of 128 bytes in
 *               [128, 0x76543200] (the stack sentinel stays 0x76543210)
 *   widening    a kept binary slot becomes a wide node (slot 0 is kept): its two children, of which the inner one of largest area
 *               (fl(fl(fl(dx*dy) + fl(dy*dz)) + fl(dz*dx)); a NaN loses, ties to the lowest position) is replaced in place by its own two
 *               children until there are four entries or no inner one; the inner entries left are kept slots.  The wide index of a kept
 *               slot is its rank among the kept slots in ascending slot index: the root is 0 and the binary tree's node order is inherited
 *   trace       per wide node all four slab tests as the binary tracer computes one; a child is a candidate iff its link is non-zero and
 *               mn <= mx && mx >= tmin && mn <= tmax; candidates are visited in ascending mn, ties by ascending slot, the others pushed
 *               farthest first; triangles, any hit, degenerate rays and the miss record as ntr_trace_bvh.  The stack is ntr_trace_bvh's
 *               (16 + 88 entries): result->stackBound <= 104 guarantees that it never overflows
 * KNOWN LIMIT: the records may differ from ntr_trace_bvh's on the same tree -- a rounded box test is not conservative, so a triangle
 *   within rounding of a box surface can be reached through one tree and culled in the other, and the visiting order decides among hits
 *   of equal t.  The spec is the definition, not the binary tracer.
 * ntr_bvh_widen: NTR_ERR_INVALID, before any device work, for a null pointer, nodesBytes not a multiple of 64 in [64, 0x76543200], a
 *   capacity below ntr_bvh_widen_capacity, an output range that overlaps the input, or a capturing stream (the call blocks: it reads a
 *   level's extent back once per four levels).  NTR_ERR_OVERFLOW: more than 0x76543200 / 128 wide nodes, nothing written.  NTR_ERR_LAYOUT,
 *   after the work: a link > 0 that names no slot was written as an empty slot; the tree is complete otherwise and *result describes it.
 *   Every other failure zeroes *result.  A slot named by several links is kept once, and the pass ends on any input.  Nothing beyond
 *   result->nodesBytes is written.  NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a device: there is no CPU fallback.  The scratch is a
 *   per-device grow-only pool that ntr_lbvh_release_workspace returns.  A wide tree is refitted in place by a one-entry
 *   ntr_pool_wide_refit (below); it is not optimized: optimize the binary tree, then widen again.
 * ntr_trace_wide: bvhFlags are the binary tree's (ntr_bvh_validate) or 0; the records are identical under any flags.  numRays == 0 ->
 *   NTR_OK, 0 seconds.  seconds == NULL is asynchronous on `stream` and capturable, a stack overflow sets the status word that
 *   ntr_trace_status reads; seconds != NULL is timed and blocking, NTR_ERR_OVERFLOW if a ray's stack overflowed.
 * ntr_trace_wide_stats: the same records through an instrumented kernel, plus the counters (numInnerVisits counts wide nodes).  Blocking. */
typedef struct NtrBvhWideResult {
    int64_t nodesBytes;                    /* the exact extent written: 128 * numNodes */
    int32_t numNodes, counts[3];           /* wide nodes; those with 2, 3 and 4 children */
    int32_t numLeafLinks, height;          /* leaf links written; wide nodes on the longest root-to-leaf path */
    int32_t stackBound;                    /* the maximum over root-to-leaf paths of the sum of (count - 1): the most entries a traversal holds */
    float   seconds;                       /* GPU time */
} NtrBvhWideResult;
/* 128 * (nodesBytes / 64): a bound, not the extent */
NTR_API int ntr_bvh_widen_capacity(int64_t nodesBytes, int64_t* wideNodesBytes);
NTR_API int ntr_bvh_widen(const void* d_nodes, int64_t nodesBytes, void* d_wideNodes, int64_t wideCapacity, NtrBvhWideResult* result,
                          void* stream);
/* Bytes the pass's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_widen_scratch_bytes(int64_t* bytes);
NTR_API int ntr_trace_wide(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_wideNodes,
                           int64_t wideNodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex, uint32_t bvhFlags,
                           void* stream, float* seconds /* NULL: asynchronous */);
NTR_API int ntr_trace_wide_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_wideNodes,
                                 int64_t wideNodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                                 uint32_t bvhFlags, void* stream, NtrTraceStats* stats);

/* Two-level trace over 4-wide trees: the pool and the top-level tree of an instanced scene widened, and the trace that walks them
 * (csrc/instanced_widen_kernels.hip, csrc/trace_instanced_wide_kernels.hip, csrc/instanced_wide_bvh.h).  EXTENSION without a
 * reference counterpart: the rule is the numpy spec tests/np_instanced_wide.py, which ntr_pool_widen and ntr_tlas_widen equal byte for
 * byte and ntr_trace_instanced_wide in all four result words, the instance id and every counter.  The binary pool, top-level tree and
 * records are only read and stay usable; the pool's triWoop and triIndex serve both paths.
 *   wide pool   one more node buffer: wide BLAS k is byte for byte what ntr_bvh_widen writes for binary BLAS k when handed
 *               pool + nodesOffset_k, placed at the sum of the exact wide extents of the BLASes before it (multiples of 128, no gaps);
 *               links stay relative to the BLAS's own start.  At most 0xFFFFFF00 bytes
 *   wide TLAS   ntr_bvh_widen applied to the top-level node buffer; leaf links ~i pass through verbatim.  N == 1: no node, rootLink ~0
 *   record i    64 bytes: words 0..11 worldToObject, 12 the wide BLAS's offset in the wide pool, 13 triWoopOffset / 16, 14 the wide
 *               BLAS's extent, 15 zero.  An instance whose blas index lies outside [0, numBlas) gets offset and extent 0: a wide node
 *               inside an instance is fetched only below the extent, so nothing of such an instance is ever read
 *   trace       ntr_trace_instanced_masked's rule with both inner steps replaced by ntr_trace_wide's wide-node step (four slab tests; a
 *               candidate iff its link is non-zero and mn <= mx && mx >= tmin && mn <= tmax; ascending (mn, slot), the others pushed
 *               farthest first).  Entering, masks, the exit marker, triangles, any hit, the miss record, degenerate rays and the 16 + 88
 *               stack are unchanged.  GENERIC arithmetic only; every fetch is range checked
 *   bytes       52 numRays + 112 (numTopInnerVisits + numInnerVisits) + 64 numInstanceEntries + 32 numInstanceEntries + 48 numTriTests
 *               + 16 numLeafVisits + 4 numHits, plus the two mask terms of ntr_trace_instanced_stats (112: a wide node's seven fetched rows)
 * KNOWN LIMIT, ntr_trace_wide's: the records may differ from the binary two-level trace's on the same scene.  The spec is the definition.
 * ntr_pool_widen_capacity: host only; the sum of ntr_bvh_widen_capacity over the ranges (a bound, not the extent).
 * ntr_pool_widen: a loop of ntr_bvh_widen, one BLAS after the other (the loop pays the pass's launches and read-backs per BLAS;
 *   ntr_pool_widen_batch, below, is the batched pass and writes the same bytes).  It blocks and is refused on a capturing stream.
 *   wideRanges[k] receives BLAS k's offset, extent, node
 *   count and stackBound; *result the total extent (nodesBytes), the sums of numNodes, counts and numLeafLinks, the largest height and
 *   stackBound of any BLAS, and the summed GPU time.  NTR_ERR_INVALID before any device work for numBlas < 1, null pointers, a pool size
 *   or BLAS range that ntr_tlas_build refuses, a capacity below ntr_pool_widen_capacity, an output that overlaps the pool.
 *   NTR_ERR_OVERFLOW: the wide pool would exceed 0xFFFFFF00 bytes.  NTR_ERR_LAYOUT, after the work, as ntr_bvh_widen reports it.
 * ntr_tlas_widen: widens the top-level tree (skipped when rootLink < 0, the one-instance tree) and writes the wide records from
 *   d_instances in one element-wise launch.  result->stackBound = the wide TLAS's bound + 1 (the exit marker) + the largest
 *   wideRanges[k].stackBound: <= 104 guarantees that the trace's stack never overflows.  It blocks and is refused on a capturing
 *   stream.  After ntr_tlas_refit or ntr_bvh_refit_batch the caller widens again, or refits the wide trees in place
 *   (ntr_pool_wide_refit, ntr_tlas_wide_refit, below), which keeps their topology and can be captured.
 *   NTR_ERR_INVALID before any device work for numInstances < 1, null or misaligned (16 B) buffers, a rootLink that is neither 0 nor an
 *   instance's link, a top-level buffer that ntr_bvh_widen refuses, capacities below ntr_bvh_widen_capacity / 64 * numInstances, a
 *   triWoopOffset that is no multiple of 16 inside the pool limit, a wide range that is not multiples of 128 inside the pool limit.
 * ntr_trace_instanced_wide: ntr_trace_instanced_masked's arguments with the wide top-level tree, wide records and wide pool nodes in
 *   place of the binary ones.  vis may be NULL; vis == NULL or a vis that can refuse nothing launches the unmasked kernel.
 *   seconds == NULL is asynchronous on `stream` and capturable; the call allocates nothing and reads nothing back.  A wide buffer that
 *   is not a multiple of 128 is refused with NTR_ERR_INVALID, like everything ntr_trace_instanced_masked refuses.
 * ntr_trace_instanced_wide_stats: the same records through an instrumented variant, plus the counters (numTopInnerVisits and
 *   numInnerVisits count wide nodes).  It blocks and is refused on a capturing stream.
 * Without a device, after the argument checks, NTR_ERR_NO_DEVICE / NTR_ERR_HIP.  The calls hold no scratch pool of their own: the BLAS
 *   table lives in ntr_bvh_widen's pool, which ntr_lbvh_release_workspace returns. */
typedef struct NtrWideBlasRange {        /* host array */
    int64_t nodesOffset, nodesBytes;     /* wide BLAS k's place in the wide pool: multiples of 128 */
    int32_t numNodes, stackBound;        /* NtrBvhWideResult's of that BLAS */
} NtrWideBlasRange;
typedef struct NtrTlasWideResult {
    int64_t nodesBytes, recordsBytes;      /* exact extents written: 128 * numNodes (0 for one instance), 64 * numInstances */
    int32_t numNodes, counts[3];           /* wide top-level nodes; those with 2, 3 and 4 children */
    int32_t numLeafLinks, height;          /* instance links written; wide nodes on the longest path of the top level */
    int32_t tlasStackBound, stackBound;    /* the top level's own bound; that + 1 + the largest BLAS bound: the most entries a trace holds */
    float   seconds;                       /* GPU time: the widening pass and the record launch */
    int32_t pad;
} NtrTlasWideResult;
NTR_API int ntr_pool_widen_capacity(int32_t numBlas, const NtrBlasRange* blasRanges, int64_t* widePoolNodesBytes);
NTR_API int ntr_pool_widen(int32_t numBlas, const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes,
                           void* d_widePoolNodes, int64_t capacity, NtrWideBlasRange* wideRanges /* numBlas, host out */,
                           NtrBvhWideResult* result, void* stream);
/* ntr_pool_widen_batch: ntr_pool_widen's arguments and outputs, every BLAS in one pass (csrc/pool_widen_batch_kernels.hip):
 *   the marking runs level by level over all BLASes at once, so the launches and read-backs number what one ntr_bvh_widen of the
 *   tallest BLAS takes plus a fixed few, whatever numBlas is.  The bytes written, wideRanges and *result (but for seconds, the GPU
 *   time of the whole pass) equal ntr_pool_widen's, that is tests/np_instanced_wide.py::widen_pool: wide BLAS k is what ntr_bvh_widen
 *   writes for pool + nodesOffset_k, at the sum of the exact extents of BLASes 0..k-1 in k order.  blasRanges may come in any order,
 *   alias or overlap each other and leave gaps: each is a tree of its own, and a link is judged against its own BLAS's slot count only.
 *   NTR_ERR_INVALID before any device work for everything ntr_pool_widen refuses, in its order (a capturing stream included: the call
 *   blocks), and for numBlas > 2^20 (wideRanges is then left untouched; every other failure zeroes it, and every failure but
 *   NTR_ERR_LAYOUT zeroes *result).  After the checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP without a device.  NTR_ERR_OVERFLOW: the wide
 *   pool would exceed 0xFFFFFF00 bytes, a wide BLAS would exceed 0x76543200 / 128 nodes, or the ranges list more than 0xFFFFFF00 / 64
 *   slots in all (possible only where they alias).  STRICTER than the loop: the node counts are known before anything is emitted, so
 *   here NOTHING is written, where ntr_pool_widen has written the BLASes before the one that overflows.  NTR_ERR_LAYOUT, after the
 *   work: some link > 0 names no slot of its own BLAS and was written as an empty slot; every wide BLAS is complete, *result and
 *   wideRanges are filled, and the message names the lowest such BLAS and the number of such links.  Nothing beyond result->nodesBytes
 *   is written.  The scratch is a per-device grow-only pool of its own that ntr_lbvh_release_workspace returns; ntr_bvh_widen's pool
 *   is not touched. */
NTR_API int ntr_pool_widen_batch(int32_t numBlas, const NtrBlasRange* blasRanges, const void* d_poolNodes, int64_t poolNodesBytes,
                                 void* d_widePoolNodes, int64_t capacity, NtrWideBlasRange* wideRanges /* numBlas, host out */,
                                 NtrBvhWideResult* result, void* stream);
/* Bytes ntr_pool_widen_batch's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_pool_widen_batch_scratch_bytes(int64_t* bytes);
NTR_API int ntr_tlas_widen(int32_t numInstances, const NtrInstance* d_instances, const void* d_tlasNodes, int64_t tlasNodesBytes,
                           int32_t rootLink, int32_t numBlas, const NtrBlasRange* blasRanges, const NtrWideBlasRange* wideRanges,
                           void* d_wideTlasNodes, int64_t capacity, void* d_wideRecords, int64_t recordsCapacity, NtrTlasWideResult* result,
                           void* stream);
NTR_API int ntr_trace_instanced_wide(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                     const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink, const void* d_wideRecords,
                                     int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes, const void* d_poolTriWoop,
                                     int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                     const NtrInstanceVisibility* vis /* NULL: no masks */, float* seconds /* NULL: asynchronous */,
                                     void* stream);
NTR_API int ntr_trace_instanced_wide_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                           int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                           const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                           int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                           const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis /* may be NULL */,
                                           NtrInstancedTraceStats* stats, void* stream);

/* A static world beside the instances: the seeded two-level trace (csrc/trace_instanced_seeded_kernels.hip,
 * csrc/trace_instanced_wide_seeded_kernels.hip).  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_seeded.py, which the device equals in all four result words, the instance id and every counter.
 * Intended use: a large static world is ONE BLAS of the pool, in its own space, and no instance.  Per batch, on one stream or in one
 * graph: ntr_trace_bvh on that BLAS's range of the pool (nodes at d_poolNodes + nodesOffset, rows at d_poolTriWoop + triWoopOffset,
 * indices at d_poolTriIndex + triWoopOffset / 16 -- a BLAS of a pool is byte for byte a Compact tree there) writes one record per ray;
 * the seeded call then traces the moving instances starting from those records.  The world pays the single-level kernel's price, and
 * the two-level kernel sees rays that are already as short as the world makes them.
 *   seed        d_seedResults[r] is ray r's record so far, four words (id, t, w2, w3).  s_hit = (id != -1).
 *   start       tmax0 = seed.t if s_hit, else the ray's tmax; the hit record starts as the seed's four words; the instance id starts
 *               as seedInstance if s_hit, else -1.  !(tmin < tmax0): no traversal (the degenerate rule, applied to tmax0).  anyHit
 *               and s_hit: no traversal.
 *   traversal   ntr_trace_instanced_masked's (ntr_trace_instanced_wide's), unchanged, from that state: masks, exit marker, the stack
 *               of 104, counters.  An accepted hit overwrites all four words and the instance id, as in the unseeded trace.
 *   no hit      a ray whose traversal accepts nothing ends with the seed's four words verbatim -- w2 and w3 are not interpreted, and
 *               a seed that is a miss keeps its own t, not the ray's -- and with seedInstance (s_hit) or -1.
 *   seed.t      taken as it is: a NaN, an infinity or a negative t makes the ray degenerate or not by the comparison above and nothing
 *               else.  Whatever the seed holds, nothing outside the buffers is read.
 *   seedInstance  any int32, stored verbatim.  With the world's NtrInstance appended behind the N instances (identity both ways, blas
 *               = the world's), seedInstance = N lets ntr_instanced_hit_attributes resolve world hits with numInstances = N + 1.
 *   counters    ntr_trace_instanced_stats's; numHits counts the final records with id != -1.  Algorithmic bytes: the unseeded formula
 *               + 16 numRays (the seed read).
 * d_results may equal d_seedResults: each lane reads its own record before it writes it.  seconds == NULL is asynchronous on `stream`
 * and capturable; the call allocates nothing and reads nothing back.  The seeded kernels are the masked loop whatever vis holds.  The
 * _stats forms block and are refused on a capturing stream.  Errors: NTR_ERR_INVALID before any device work for everything the
 * unseeded sibling refuses, a null d_seedResults and a d_seedResults that is not 16-byte aligned; numRays == 0 returns NTR_OK.
 * Without a device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
NTR_API int ntr_trace_instanced_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                       int32_t seedInstance, NtrRayResult* d_results /* may equal d_seedResults */, int32_t* d_instanceIDs,
                                       const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                       int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                       int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                       const NtrInstanceVisibility* vis /* NULL: no masks */, float* seconds /* NULL: asynchronous */,
                                       void* stream);
NTR_API int ntr_trace_instanced_seeded_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                             int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                             int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                             const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                             int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                             const NtrInstanceVisibility* vis /* may be NULL */, NtrInstancedTraceStats* stats, void* stream);
NTR_API int ntr_trace_instanced_wide_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                            int32_t seedInstance, NtrRayResult* d_results /* may equal d_seedResults */,
                                            int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                            const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                            int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                            const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis /* NULL: no masks */,
                                            float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_wide_seeded_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                  int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                                  const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                                  const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                                  int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                                  const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis /* may be NULL */,
                                                  NtrInstancedTraceStats* stats, void* stream);

/* FAST slab arithmetic in the two-level trace, from device-resident flags (csrc/instanced_validate_kernels.hip,
 * csrc/trace_instanced_fast_kernels.hip).  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_fast.py.  The records, the instance ids, the status word and the eight counters are ntr_trace_instanced_masked's
 * (or, with a seed, ntr_trace_instanced_seeded's) in every word, for closest hit and any hit, whatever the flags say: in its range the
 * FAST quotient is the IEEE divide bit for bit (ntr_selftest_division), so the flags and the vote only select between two exact forms
 * of the inner-node step.  An opt-in entry point; nothing else launches these kernels.
 * ntr_instanced_validate: a one-wave launch that clears the four words and one grid-stride launch over both node buffers (two kernels:
 *   a memset node does not replay reliably in a captured graph); asynchronous on `stream`, capturable, allocates nothing and reads
 *   nothing back.
 *   layout      d_flags[0], d_flags[1]: the WITHHELD bits of the top-level tree and of the pool, bit values NTR_BVH_FINITE / FASTDIV /
 *               NOTINY / ORDERED; d_flags[2], d_flags[3]: zero.  Withheld and not granted, so that an OR from any wave is the whole
 *               protocol.  The trace reads FASTDIV and NOTINY; FINITE and ORDERED are recorded for the caller.
 *   rule        ntr_bvh_validate's, word for word, for those four flags: the twelve box floats of every 64-byte node are tested, the
 *               child words are not.  No NTR_BVH_WIDE_LEAVES, no refresh of a top-of-tree table.
 *   extent      EVERY node slot in [0, bytes) of both buffers: the slack and the gaps of a pool count, whatever they hold.  That is
 *               conservative: it can only withhold.  tlasNodesBytes == 0 (one instance: rootLink ~0), or d_tlasNodes == NULL, withholds
 *               nothing for the top level.
 *   consequence the tree of a one-triangle BLAS has an empty sibling box (lo = FLT_MAX, hi = -FLT_MAX): a pool that holds one has
 *               FINITE, FASTDIV and ORDERED withheld for the whole pool, and FAST then runs on the top level only.  Per-BLAS flags are
 *               out of scope.
 *   when        after every call that rewrites a node box of either buffer, and before the next fast trace (on one stream, or in one
 *               graph, in that order): ntr_ploc_build_batch and every other build into the pool, ntr_bvh_refit / ntr_bvh_refit_batch,
 *               ntr_bvh_optimize / ntr_bvh_optimize_batch and ntr_bvh_reorder on the pool; ntr_tlas_build and ntr_tlas_refit on the top
 *               level; any copy into the buffers.  Flags that grant what the buffers do not hold -- stale flags, or another pool's --
 *               are a caller error: the records are then undefined (nothing outside the buffers is read all the same).  Flags that
 *               wrongly WITHHOLD only cost speed.
 *   errors      NTR_ERR_INVALID before any device work: a null d_flags or d_poolNodes; sizes that are not multiples of 64,
 *               tlasNodesBytes above the Compact limit or poolNodesBytes outside the pool limits; d_flags, d_tlasNodes or d_poolNodes not
 *               16-byte aligned.  Nothing else is refused: a capturing stream is accepted.
 * ntr_instanced_flags_read: the GRANTED sets, the complement within the four bits; blocking (it synchronises `stream`), refused on a
 *   capturing stream.
 * ntr_trace_instanced_fast: ntr_trace_instanced_seeded's argument list with d_flags before `seconds`; vis may be NULL, and d_seedResults
 *   may be NULL, which means unseeded (seedInstance is then ignored, and the rule is ntr_trace_instanced_masked's).  The loop is the
 *   masked (seeded) one with one addition, a per-lane state `nice`: the lane's CURRENT ray may take FAST on its CURRENT level.
 *   start       nice = !(d_flags[0] & FASTDIV) && the world ray is in the FAST ranges (directions 2^-40 <= |d| <= 2^20, origin
 *               components 2^-36 <= |o| < 2^55, a zero origin component only when d_flags[0] does not withhold NOTINY)
 *   entering    after the transform: the same test of the object ray against d_flags[1]
 *   leaving     the world ray's value again
 *   vote        one ballot per iteration of a wave: the iteration runs the FAST form of the inner-node step iff no live lane has
 *               nice == false, else the GENERIC form; the choice is wave-uniform
 *   flag words  read once per wave by the launch: a captured launch reads them at replay time, after a captured validate
 * ntr_trace_instanced_fast_stats: the same records through the instrumented kernels, plus ntr_trace_instanced_stats's counters and
 *   NtrInstancedFastStats (wave w is rays [64 w, 64 w + 64); all exact and equal to the spec's).  Blocks; refused on a capturing stream.
 * Errors: NTR_ERR_INVALID before any device work for everything ntr_trace_instanced_seeded refuses (but a null d_seedResults), a null
 *   d_flags and a d_flags that is not 16-byte aligned, null stats; numRays == 0 returns NTR_OK with the stats zeroed.  Without a device,
 *   after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrInstancedFastStats {
    uint64_t waveSteps;       /* iterations of a wave with at least one live lane, summed over the waves */
    uint64_t fastWaveSteps;   /* those that took the FAST form */
    uint64_t niceStarts;      /* rays that start live and nice */
    uint64_t niceEntries;     /* entering steps that entered and leave the lane nice */
} NtrInstancedFastStats;
NTR_API int ntr_instanced_validate(const void* d_tlasNodes, int64_t tlasNodesBytes, const void* d_poolNodes, int64_t poolNodesBytes,
                                   uint32_t* d_flags /* 4 words, 16-byte aligned */, void* stream);
NTR_API int ntr_instanced_flags_read(const uint32_t* d_flags, uint32_t* tlasFlags, uint32_t* poolFlags, void* stream);
NTR_API int ntr_trace_instanced_fast(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults /* NULL: unseeded */,
                                     int32_t seedInstance, NtrRayResult* d_results /* may equal d_seedResults */, int32_t* d_instanceIDs,
                                     const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                     int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                     int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                     const NtrInstanceVisibility* vis /* NULL: no masks */, const uint32_t* d_flags,
                                     float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_fast_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                           int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                           int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                           const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                           int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                           const NtrInstanceVisibility* vis /* may be NULL */, const uint32_t* d_flags,
                                           NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats, void* stream);

/* FAST slab arithmetic in the two-level trace over 4-wide trees (csrc/instanced_validate_kernels.hip,
 * csrc/trace_instanced_wide_fast_kernels.hip).  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_wide_fast.py.  The block above, point for point, over the wide buffers: the records, the instance ids, the status
 * word and the seven counters are ntr_trace_instanced_wide's with `vis` (or, with a seed, ntr_trace_instanced_wide_seeded's) in every
 * word, for closest hit and any hit, whatever the flags say.  Opt-in entry points; nothing else launches these kernels, and the wide
 * kernels above stay what they were.
 * ntr_instanced_wide_validate: ntr_instanced_validate over the wide top-level tree and the wide pool -- the same two launches,
 *   asynchronous on `stream`, capturable, allocating nothing and reading nothing back.  A pass of its own because the binary buffers'
 *   flags do not carry over: ntr_pool_wide_refit(rewriteRows = 1) + ntr_tlas_wide_refit update the wide trees without any binary refit,
 *   after which the binary boxes, and whatever ntr_instanced_validate said of them, are stale.
 *   layout      the same four words with the same meaning, WITHHELD bits: d_flags[0] the wide top level, d_flags[1] the wide pool,
 *               d_flags[2] and d_flags[3] zero.  ntr_instanced_flags_read serves both layouts.
 *   rule        ntr_bvh_validate's for FINITE, FASTDIV, NOTINY and ORDERED over EVERY 128-byte slot in [0, bytes) of both buffers: words
 *               0..11 and 16..27 are twelve (lo, hi) pairs (rows 0, 1, 2, 4, 5, 6); words 12..15 (links) and 28..31 (count) are never
 *               looked at.  Padding slots (k >= count: a copy of slot 0's box), empty slots below count, nodes that no link reaches and
 *               slack behind the last BLAS count: all of this can only withhold.  wideTlasNodesBytes == 0, or d_wideTlasNodes == NULL
 *               (one instance), withholds nothing for the top level.
 *   when        after every call that rewrites a box of either wide buffer and before the next wide fast trace (on one stream, or in
 *               one graph, in that order): ntr_pool_widen / ntr_pool_widen_batch, ntr_tlas_widen, ntr_pool_wide_refit,
 *               ntr_tlas_wide_refit, any copy into the buffers.  Flags that grant what the buffers do not hold are a caller error with
 *               undefined records (nothing outside the buffers is read all the same); flags that wrongly WITHHOLD only cost speed.
 *   errors      NTR_ERR_INVALID before any device work: a null d_flags or d_widePoolNodes; sizes that are not multiples of 128,
 *               wideTlasNodesBytes neither 0 nor within the wide limit, widePoolNodesBytes outside the wide pool limits; d_flags,
 *               d_wideTlasNodes or d_widePoolNodes not 16-byte aligned.  A capturing stream is accepted.
 * ntr_trace_instanced_wide_fast: ntr_trace_instanced_wide_seeded's argument list with d_flags before `seconds`; vis may be NULL, and
 *   d_seedResults may be NULL, which means unseeded (seedInstance is then ignored).  The loop is the masked (seeded) wide one with the
 *   per-lane `nice` of ntr_trace_instanced_fast: at the start from the world ray against d_flags[0], on entering an instance, after the
 *   transform, from the object ray against d_flags[1], at the exit marker from the reloaded world ray against d_flags[0]; one ballot per
 *   iteration, FAST iff no live lane has nice == false, and the wave then takes the FAST form of the wide-node step and of the triangle
 *   step; the two flag words are read once per wave by the launch.  No prologue, no octant vote, no use of ORDERED.
 * ntr_trace_instanced_wide_fast_stats: the same records through the instrumented kernels, plus ntr_trace_instanced_wide_stats's
 *   counters and NtrInstancedFastStats with 6w's definitions; a step is one iteration of the device's wide loop (a triangle step also
 *   takes the terminator behind its triangle).  Blocks; refused on a capturing stream.
 * Errors: NTR_ERR_INVALID before any device work for everything ntr_trace_instanced_wide_seeded refuses (but a null d_seedResults), a
 *   null d_flags and a d_flags that is not 16-byte aligned, null stats; numRays == 0 returns NTR_OK with the stats zeroed.  Without a
 *   device, after these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
NTR_API int ntr_instanced_wide_validate(const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, const void* d_widePoolNodes,
                                        int64_t widePoolNodesBytes, uint32_t* d_flags /* 4 words, 16-byte aligned */, void* stream);
NTR_API int ntr_trace_instanced_wide_fast(int32_t numRays, int32_t anyHit, const NtrRay* d_rays,
                                          const NtrRayResult* d_seedResults /* NULL: unseeded */, int32_t seedInstance,
                                          NtrRayResult* d_results /* may equal d_seedResults */, int32_t* d_instanceIDs,
                                          const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink, const void* d_wideRecords,
                                          int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                                          const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                          const NtrInstanceVisibility* vis /* NULL: no masks */, const uint32_t* d_flags,
                                          float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_wide_fast_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                                const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                                const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                                int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                                const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis /* may be NULL */,
                                                const uint32_t* d_flags, NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats,
                                                void* stream);

/* In-place refit of 4-wide trees: the update path of an animated instanced frame for the wide two-level trace
 * (csrc/wide_refit_batch_kernels.hip, csrc/tlas_wide_refit_kernels.hip, csrc/wide_climb.h).  ntr_pool_widen and
 * ntr_tlas_widen block, read back and may change a wide tree's topology from frame to frame; these two calls keep the wide topology
 * and rewrite every box in place, asynchronously and capturably, the pool's BLASes in one pass.  EXTENSION without a reference
 * counterpart: the rule is the numpy spec tests/np_wide_refit.py, which the device equals byte for byte.
 *   leaf box     slot k < count with link < 0: ntr_bvh_refit's leaf rule over the leaf's triangles and the entry's epsilon; a leaf
 *                without rows keeps its box
 *   inner box    slot k < count with link > 0: the union, in the integer order, of slots 0..count-1 of the wide node it names
 *   empty slot   link 0 below count: keeps its box and takes part in its node's union
 *   padding      slot k >= count: a copy of slot 0's new box (ntr_bvh_widen's invariant)
 *   not written  words 12..15 and 28..31 of every wide node, wide nodes no link reaches, terminators, triIndex; the Woop rows unless
 *                rewriteRows
 *   equal to     the boxes of the refitted binary tree at the slots' sources: after ntr_bvh_refit_batch (or with rewriteRows = 1) the
 *                wide tree is what ntr_bvh_widen's expansion of the OLD binary boxes selects from the NEW binary boxes.  A fresh
 *                widening of the refitted binary tree may choose another topology (areas changed): both are valid wide trees
 * ntr_pool_wide_refit: an entry is a wide BLAS's range (NtrWideBlasRange's offset and extent), the BLAS's row range (NtrBlasRange's),
 *   its mesh and its epsilon, as NtrRefitBatchEntry's.  rewriteRows = 1 also rewrites the Woop rows of every leaf, bit for bit as
 *   ntr_bvh_refit_batch does: the all-wide path of a caller that traces wide only (no binary refit; ntr_tlas_wide_refit then takes the
 *   boxes from the wide roots).  rewriteRows = 0 only reads the rows: for a caller that has just run ntr_bvh_refit_batch over the same
 *   selection.  d_blasBoxes: optional, 6 floats per entry in entry order, min.xyz max.xyz, the union of the root's slots -- equal to
 *   ntr_bvh_refit_batch's.  lanesPerLeaf is chosen by ntr_bvh_refit's thresholds from numTris / max(rows - 3 numTris, 1) summed over
 *   the entries (a leaf is a terminator row): speed only.  A single-level wide tree (ntr_bvh_widen) is refitted as a one-entry pool.
 * ntr_tlas_wide_refit: writes wide record i from the current d_instances[i] as ntr_tlas_widen does, forms the box of a leaf ~i from
 *   the union of the root slots of instance i's wide BLAS (the pool's node 0 is not read) through objectToWorld as ntr_tlas_refit
 *   does, and climbs.  N == 1: no node, rootLink ~0, wideTlasNodesBytes 0; record 0 and the scene box.
 * Both follow ntr_bvh_refit_batch and ntr_tlas_refit point for point: result == NULL is asynchronous on `stream` (two launches, no
 * read-back, no memset, capturable); result != NULL blocks, reads counts, error bits and GPU time back and is refused on a capturing
 * stream.  A malformed part is never followed and nothing outside the buffers is read or written, whatever the wide buffers hold: the
 * blocking form returns NTR_ERR_LAYOUT after the work with *result filled (error bits as ntr_bvh_refit's / ntr_tlas_refit's; bit 1 of
 * the pool and bit 2 of the top level also cover a link that is no multiple of 128 or lies outside the tree, a node named by two links
 * and a count word outside 2..4; NTR_ERR_INVALID for a blas index out of range, as ntr_tlas_refit), every other entry has been
 * refitted completely; the asynchronous form skips such a part silently.  The scratch (8 B per listed wide node, the entry or range
 * table, 16 KB of counters) is a per-device grow-only pool of each call's own that ntr_lbvh_release_workspace returns.  Tables are
 * uploaded only when they differ from the last uncaptured call's; a captured call is accepted only when the last uncaptured call had
 * the same table (and the same instance count and extent) and the pool has not been released since, else NTR_ERR_INVALID says so.  One
 * call per device at a time.
 * NTR_ERR_INVALID (before any device work): null pointers (d_blasBoxes, d_sceneBox, result may be null; d_wideTlasNodes for N == 1),
 * numEntries outside 1..2^20, sizes that are not multiples of 128 / 16 / 64 within the pool limits, pointers not 16-byte aligned, a
 * range that is misaligned or outside the extents, entries whose wide ranges or row ranges overlap, a mesh outside [0, numTrisTotal), a
 * negative or non-finite epsilon, a rewriteRows other than 0 or 1, a rootLink that is neither 0 nor ~0 as N requires,
 * wideTlasNodesBytes that is no multiple of 128 (0 only for N == 1), recordsCapacity < 64 * numInstances.  Without a device, after
 * these checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrWideRefitEntry {            /* host array, one per wide BLAS to refit: 48 bytes */
    int64_t wideNodesOffset, wideNodesBytes;  /* NtrWideBlasRange's of that BLAS */
    int64_t triWoopOffset, triWoopBytes;      /* NtrBlasRange's of that BLAS */
    int32_t firstTri, numTris;
    float   epsilon;
    int32_t pad;
} NtrWideRefitEntry;
typedef struct NtrWideRefitResult {
    int32_t numEntries, lanesPerLeaf;         /* lanesPerLeaf says which kernel ran */
    int64_t numNodes, numLeafLinks, numRows;  /* sums over the entries: wide nodes, negative links, rows (terminators included) */
    int32_t firstBadEntry, errBits;           /* -1 / 0, or the lowest entry whose tree is malformed and the OR of the error bits */
    float   seconds, pad;                     /* GPU time */
} NtrWideRefitResult;
NTR_API int ntr_pool_wide_refit(int32_t numEntries, const NtrWideRefitEntry* entries, void* d_widePoolNodes, int64_t widePoolNodesBytes,
                                void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, int32_t numTrisTotal,
                                const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos, int32_t rewriteRows,
                                float* d_blasBoxes /* may be NULL */, NtrWideRefitResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the wide pool refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_pool_wide_refit_scratch_bytes(int64_t* bytes);
NTR_API int ntr_tlas_wide_refit(int32_t numInstances, const NtrInstance* d_instances, int32_t numBlas, const NtrBlasRange* blasRanges,
                                const NtrWideBlasRange* wideRanges, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                                void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink, void* d_wideRecords,
                                int64_t recordsCapacity, float* d_sceneBox /* may be NULL */,
                                NtrTlasRefitResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the wide top-level refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_wide_refit_scratch_bytes(int64_t* bytes);

/* Motion blur over the 4-wide trees: the swept wide refit and the timed wide trace (csrc/tlas_wide_motion_refit_kernels.hip,
 * csrc/trace_instanced_wide_motion_kernels.hip).  EXTENSION without a reference counterpart: the rule is the numpy spec
 * tests/np_instanced_wide_motion.py, which the refit equals byte for byte and the trace bit for bit in all four result words, the
 * instance id and every counter.  Keys, time, pose, the moving flag, the 128-byte motion key entry, the entering step's order of checks
 * and singular poses are ntr_tlas_motion_refit's and ntr_trace_instanced_motion's (above); the wide loop is ntr_trace_instanced_wide's;
 * the wide leaf box is ntr_tlas_wide_refit's.
 * ntr_tlas_wide_motion_refit: ntr_tlas_wide_refit over two instance arrays, d_instances0 the shutter's opening and d_instances1 its
 *   close, with the three changes ntr_tlas_motion_refit makes to ntr_tlas_refit:
 *   records     wide record i is ntr_tlas_widen's record of key-0 instance i; word 15 is 1 where the twelve objectToWorld words differ
 *               bitwise between the keys, else 0.  No kernel but the wide motion trace reads word 15.  A later plain
 *               ntr_tlas_wide_refit or ntr_tlas_widen writes word 15 = 0 and thereby FREEZES the scene at key 0, boxes included
 *   motion keys entry i is written for every instance, byte for byte what ntr_tlas_motion_refit writes for the same two arrays: the
 *               all-wide update path needs no binary motion refit, and one key buffer serves both trees
 *   boxes       the box of a leaf ~i is the union, in the integer order, of instance i's world box under key 0 and under key 1, both
 *               from the union of the root slots of i's wide BLAS (the pool's node 0 is not read); a static instance's box is
 *               ntr_tlas_wide_refit's.  The climb is ntr_tlas_wide_refit's
 *   N == 1: no node, rootLink ~0, wideTlasNodesBytes 0; one small launch writes record 0, key entry 0 and the scene box.
 *   The contract is ntr_tlas_wide_refit's in every respect not named here: result == NULL is asynchronous on `stream` and capturable
 *   (two launches, no read-back, no memset); the blocking form is refused on a capturing stream; a bad part is never followed and the
 *   error bits are unchanged; the held range table and its rule for captured calls; a per-device grow-only scratch pool of its own
 *   (ntr_tlas_wide_motion_refit_scratch_bytes) that ntr_lbvh_release_workspace returns; one call per device at a time.  It also
 *   requires d_instances1 non-null and 16-byte aligned, d_motionKeys non-null and 16-byte aligned, and motionKeysCapacity >=
 *   128 * numInstances, refused where ntr_tlas_motion_refit refuses them in the order of the checks.  numMoving counts the moving
 *   instances among all numInstances.
 * ntr_trace_instanced_wide_motion: ntr_trace_instanced_wide's arguments plus `motion`.  With motion == NULL the call IS
 *   ntr_trace_instanced_wide -- the same launch, and its refusals name that function.  Otherwise the masked wide loop with
 *   ntr_trace_instanced_motion's entering step: index in range; masks; room for the marker; then, if word 15 of the fetched wide record
 *   is non-zero, the two keys are read from the motion key buffer at 128 * i (range checked: beyond min(motionKeysBytes, 0xFFFFFF00) a
 *   read returns zeros, and a zero matrix is singular), M(t_r) is formed and inverted -- no inverse makes the step a pop, counted as
 *   numSingular only -- then the marker is pushed and the ray transformed by worldToObject(t_r).  seconds == NULL is asynchronous on
 *   `stream` and capturable; times, keys and records are read by the launch, so a replay sees what is there at replay time.
 * ntr_trace_instanced_wide_motion_stats: the same records through the instrumented kernel, plus ntr_trace_instanced_wide_stats's
 *   counters and the two of NtrInstancedMotionStats.  It blocks and is refused on a capturing stream.  With motion == NULL it is
 *   ntr_trace_instanced_wide_stats and the motion counters are zero.
 * Algorithmic bytes: ntr_trace_instanced_wide's formula plus 128 (numMovingEntries + numSingular), plus 4 numRays with per-ray times.
 * Errors: NTR_ERR_INVALID before any device work for everything ntr_trace_instanced_wide refuses, in its words and order, then the
 *   three motion refusals of ntr_trace_instanced_motion in its words; a null stats or motionStats.  numRays == 0 returns NTR_OK with
 *   the stats zeroed; without a device, after these checks, NTR_ERR_NO_DEVICE / NTR_ERR_HIP.
 * ntr_instanced_hit_attributes_motion takes no records and works behind a wide motion trace unchanged.
 * Out of scope: the seeded / world form, FAST, more than two keys, BLASes that deform within the shutter, a TLAS build over swept
 * boxes (the topology is whatever ntr_tlas_build and ntr_tlas_widen made at key 0). */
NTR_API int ntr_tlas_wide_motion_refit(int32_t numInstances, const NtrInstance* d_instances0, const NtrInstance* d_instances1,
                                       int32_t numBlas, const NtrBlasRange* blasRanges, const NtrWideBlasRange* wideRanges,
                                       const void* d_widePoolNodes, int64_t widePoolNodesBytes, void* d_wideTlasNodes,
                                       int64_t wideTlasNodesBytes, int32_t rootLink, void* d_wideRecords, int64_t recordsCapacity,
                                       void* d_motionKeys, int64_t motionKeysCapacity, float* d_sceneBox /* may be NULL: 6 floats */,
                                       NtrTlasMotionRefitResult* result /* NULL: asynchronous */, void* stream);
/* Bytes the wide motion refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_tlas_wide_motion_refit_scratch_bytes(int64_t* bytes);
NTR_API int ntr_trace_instanced_wide_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                            int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes,
                                            int32_t rootLink, const void* d_wideRecords, int32_t numInstances,
                                            const void* d_widePoolNodes, int64_t widePoolNodesBytes, const void* d_poolTriWoop,
                                            int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                            const NtrInstanceVisibility* vis /* NULL: no masks */,
                                            const NtrInstanceMotion* motion /* NULL: ntr_trace_instanced_wide */,
                                            float* seconds /* NULL: asynchronous */, void* stream);
NTR_API int ntr_trace_instanced_wide_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                                  int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes,
                                                  int32_t rootLink, const void* d_wideRecords, int32_t numInstances,
                                                  const void* d_widePoolNodes, int64_t widePoolNodesBytes, const void* d_poolTriWoop,
                                                  int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                                  const NtrInstanceVisibility* vis /* may be NULL */,
                                                  const NtrInstanceMotion* motion /* may be NULL */, NtrInstancedTraceStats* stats,
                                                  NtrInstancedMotionStats* motionStats, void* stream);

/* On-device refit: keep a BVHLayout_Compact tree's topology and recompute its boxes and Woop rows from moved vertex positions
 * (csrc/bvh_refit_kernels.hip).  EXTENSION without a reference counterpart (the reference's scenes are static): the rule is pinned by
 * the numpy spec tests/np_bvh_refit.py, not by reference lines.  It works on any Compact tree whatever built it -- ntr_sah_build
 * (uploaded), ntr_lbvh_build, ntr_hlbvh_build, ntr_persistent_bvh_build, a bvhcache file -- as long as the mesh keeps its triangles
 * (d_triVtxIndex, numTris) and only d_vtxPos changes.
 *   written      in place: the 12 box floats of every node a link reaches, and the three Woop rows of every triangle of every leaf
 *   not written  child words, the split word and the fourth word of a node's link float4, leaf terminators, d_triIndex, the rows
 *                behind a leaf's terminator, and node slots no link reaches (zero-filled slots inside the extent, NtrLbvhResult)
 *   Woop rows    of the row group r, r+1, r+2 of a leaf: woop_rows.h of triangle d_triIndex[r] over the new positions -- the device
 *                builders' function, so the rows equal a fresh device build's bit for bit (a host SAH tree's rows, made by the
 *                host's woopify, may change in their last bits even for unmoved vertices)
 *   leaf box     per axis the minimum and maximum over the three vertices of every triangle of the leaf, then fl(lo - epsilon),
 *                fl(hi + epsilon) (the LBVH's rule; epsilon 0 is the exact union, which a host SAH tree stores).  A leaf without
 *                rows (the one-triangle tree's empty child 0) keeps its box words
 *   inner box    the union of the two boxes stored in that child's node; epsilon is applied at the leaves only (a "PersistentBVH"
 *                tree, which grows every level by its epsilon, comes out valid and slightly tighter, not identical)
 *   min / max    in the total order -0 < +0, so no result depends on the order of the operands or of the threads: the output is
 *                deterministic.  NaN coordinates are out of contract (result unspecified; nothing outside the buffers is touched)
 *   d_sceneBox   optional, 6 floats min.xyz max.xyz: the union of the root's two boxes
 * Two launches on `stream` that re-initialise their own state, no host read-back: with result == NULL the call is asynchronous and
 * can be captured into a HIP graph like ntr_trace_bvh.  With result != NULL it blocks, reads back what the passes counted and the
 * GPU time, and reports a malformed tree (a link or row outside the extents, a triangle or vertex index out of range:
 * NTR_ERR_LAYOUT; such a part is never followed, and with result == NULL it is skipped silently).  The topology arrays (8 B per node
 * slot, and 16 KB of counters) live in a per-device grow-only pool that ntr_lbvh_release_workspace returns.  The pool regrows only
 * after the device has drained, so a call that must grow it cannot be captured: a captured call needs one earlier uncaptured call on
 * a tree at least as large (inside a capture a too-small pool is NTR_ERR_INVALID, never an allocation), and the pool must not be
 * regrown or released while such a graph lives.  One refit per device at a time.
 * Afterwards the caller re-runs ntr_bvh_validate: the FASTDIV / NOTINY / ORDERED / FINITE flags and the top-of-tree table depend on the
 * boxes.  Scheduling hints (NtrSchedHint) learned on the old boxes stay legal, because they only ever order blocks.
 * NTR_ERR_INVALID (before any device work): a null pointer (d_sceneBox and result may be null), nodesBytes not a multiple of 64 in
 * [64, 0x76543200], triWoopBytes not a positive multiple of 16, triIndexBytes * 4 < triWoopBytes, numTris < 1, numVerts < 1, epsilon
 * negative or not finite.  Without a device: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrBvhRefitResult {
    int32_t numNodes, numLeaves, numRows, pad;   /* what the passes counted: 1 + inner links, leaf links, rows of the leaves with
                                                    their terminators (read back only when result != NULL) */
    float   seconds;                             /* GPU time of the call when result != NULL, else untouched */
} NtrBvhRefitResult;
NTR_API int ntr_bvh_refit(void* d_nodes, int64_t nodesBytes, void* d_triWoop, int64_t triWoopBytes,
                          const int32_t* d_triIndex, int64_t triIndexBytes,
                          int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                          float epsilon, float* d_sceneBox /* may be NULL */,
                          NtrBvhRefitResult* result /* NULL: asynchronous, capturable */, void* stream);
/* Bytes the refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_refit_scratch_bytes(int64_t* bytes);

/* Deformation motion blur over one BVHLayout_Compact tree: a refit to TWO vertex arrays (csrc/bvh_motion_refit_kernels.hip) and a trace
 * that poses boxes and triangles at each ray's time (csrc/trace_motion_kernels.hip).  EXTENSION without a reference counterpart: the rule
 * is the numpy spec tests/np_bvh_motion.py, whose docstring is the normative text; ntr_bvh_motion_refit equals its motion_refit byte for
 * byte and ntr_trace_bvh_motion its trace in all four result words and every counter.  One mesh topology (d_triVtxIndex, numTris), two
 * position arrays: d_vtxPos0 is the shutter's opening, d_vtxPos1 its close.  Any Compact tree, whatever built it; single level only
 * (not inside ntr_trace_instanced_*), binary trees only, two keys only, no FAST flags.
 * ntr_bvh_motion_refit
 *   d_nodes0, d_triWoop  in place, exactly what ntr_bvh_refit(d_vtxPos0) writes and leaves alone: afterwards ntr_trace_bvh over them is the
 *                        scene at the shutter's opening
 *   d_nodes1             nodesBytes, written: first a copy of d_nodes0 as it was handed in (the caller need not initialise it), then the
 *                        boxes ntr_bvh_refit(d_vtxPos1) writes -- so links, split words and slots no link reaches are d_nodes0's
 *   d_vertRows0/1        triWoopBytes each, written: zero-filled, then for every row group r, r+1, r+2 of a reached leaf the rows
 *                        (x, y, z, 0) of vertices 0, 1, 2 of triangle d_triIndex[r] under that key, and at a reached leaf's terminator row
 *                        (0, 0, 0, 0x80000000).  The terminator lives in W: a vertex x of -0.0f is the terminator's word
 *   d_sceneBox           optional, 6 floats min.xyz max.xyz: the union of the two keys' scene boxes
 *   result               ntr_bvh_refit's counts (the same for both keys) and the GPU time of the whole call
 * The protocol is ntr_bvh_refit's in every respect: launches only on `stream`, which re-initialise their own state (no memset or copy
 * node); result == NULL is asynchronous and capturable after one uncaptured call on a tree at least as large; result != NULL blocks and
 * reports a malformed tree as NTR_ERR_LAYOUT (never followed; skipped silently when result == NULL); a per-device grow-only pool (12 B
 * per node slot and 16 KB of counters) that ntr_lbvh_release_workspace returns and that must not regrow or be released while a graph
 * lives.  One refit per device at a time.
 * NTR_ERR_INVALID (before any device work): ntr_bvh_refit's cases; a null d_nodes1, d_vertRows0, d_vertRows1 or d_vtxPos1; node, Woop or
 * vertex-row buffers not 16-byte aligned; any of those four buffers overlapping another buffer of the call.
 * ntr_trace_bvh_motion / _stats
 *   time         ray r has time d_rayTimes[r] when d_rayTimes is given, else `time`; clamped by t > 0 ? (t < 1 ? t : 1) : 0 (NaN -> 0).
 *                The times are read by the kernel -- at replay when the call was captured; `time` is then the value at capture
 *   pose         per word a at t == 0, b at t == 1, else fl(fl((1 - t) a) + fl(t b)).  NOT ntr_trace_instanced_motion's lerp: no "same
 *                word" shortcut, so that the posed box contains the posed triangle exactly, with no padding (a vertex that does not move
 *                may wobble by an ulp inside the shutter; its Woop rows are recomputed from the posed vertices anyway)
 *   inner node   the twelve box words posed from d_nodes0 and d_nodes1, links from d_nodes0, then ntr_trace_bvh's exact slab test and order
 *   triangle     a row group is a terminator iff the W word of d_vertRows0's row is 0x80000000; otherwise the nine vertex words are
 *                posed, woop_rows.h gives the Woop rows and ntr_trace_bvh's triangle test runs on them
 *   consequences at time 0 / 1 the records are ntr_trace_bvh's over the tree refitted to d_vtxPos0 / d_vtxPos1, word for word; at a scalar
 *                time t they are ntr_trace_bvh's over the posed static tree
 *   counters     NtrTraceStats as ntr_trace_bvh_stats fills it; algorithmic bytes are 128 per inner visit, 96 per triangle test, 16 per
 *                terminator, 48 per ray and 4 more per ray with d_rayTimes
 * seconds == NULL: asynchronous on `stream` and capturable; a traversal stack overflow (16 LDS + 88 scratch entries) is the sticky bit
 * of ntr_trace_status.  seconds != NULL: drains the stream, times the launch and reports an overflow as NTR_ERR_OVERFLOW.  The _stats form
 * runs the instrumented kernel, blocks and is refused on a capturing stream.
 * NTR_ERR_INVALID (before any device work): numRays < 0; a null ray, result or tree buffer or a null motion; nodesBytes not a multiple
 * of 64 in [64, 0x76543200]; vertRowsBytes not a multiple of 16 in [16, 0xFFFFFF00]; d_rayTimes not 4-byte aligned.  numRays == 0 ->
 * NTR_OK, 0 seconds.  Without a device: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
NTR_API int ntr_bvh_motion_refit(void* d_nodes0, int64_t nodesBytes, void* d_nodes1, void* d_triWoop, int64_t triWoopBytes,
                                 const int32_t* d_triIndex, int64_t triIndexBytes,
                                 void* d_vertRows0, void* d_vertRows1 /* triWoopBytes each */,
                                 int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos0,
                                 const float* d_vtxPos1, float epsilon, float* d_sceneBox /* may be NULL */,
                                 NtrBvhRefitResult* result /* NULL: asynchronous, capturable */, void* stream);
/* Bytes the motion refit's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_motion_refit_scratch_bytes(int64_t* bytes);
typedef struct NtrBvhMotion {
    const void *d_nodes1, *d_vertRows0, *d_vertRows1;   /* ntr_bvh_motion_refit's */
    const float* d_rayTimes;                             /* may be NULL: every ray has `time` */
    float time;
} NtrBvhMotion;
NTR_API int ntr_trace_bvh_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                 const void* d_nodes0, int64_t nodesBytes, int64_t vertRowsBytes, const int32_t* d_triIndex,
                                 const NtrBvhMotion* motion, void* stream, float* seconds /* NULL: asynchronous, capturable */);
NTR_API int ntr_trace_bvh_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                       const void* d_nodes0, int64_t nodesBytes, int64_t vertRowsBytes, const int32_t* d_triIndex,
                                       const NtrBvhMotion* motion, void* stream, NtrTraceStats* stats);   /* blocking, instrumented kernel */

/* On-device treelet restructuring: raise the quality of a BVHLayout_Compact tree in place, whatever built or refitted it
 * (csrc/bvh_optimize_kernels.hip).  EXTENSION without a reference counterpart: the rule is pinned by the numpy spec
 * tests/np_bvh_optimize.py (its docstring is the normative text), not by reference lines.  The algorithm is the treelet part of Karras
 * and Aila, "Fast parallel construction of high-quality bounding volume hierarchies" (HPG 2013) with treelets of 7 entries.
 * Only the node buffer is read and written: leaves stay as they are (d_triWoop and d_triIndex are not even passed), leaf links move
 * between parents, so ntr_trace_bvh and ntr_bvh_refit work on the result unchanged.
 *   per pass     every reached slot with at least 7 leaf links below it roots a treelet, in ascending height (slots of one height have
 *                disjoint subtrees: one launch per height).  The treelet grows from the root's two children by expanding, six times
 *                in all, the inner entry of the largest area; a dynamic programme over the 127 subsets of the 7 entries finds the
 *                binary topology with the smallest sum of inner-node areas (binary32, no contraction, ties to the lowest mask)
 *   written      a treelet is rewritten only if that sum is STRICTLY smaller than its existing topology's; then its root and its five
 *                other internal slots (handed out in ascending index in preorder) get the new boxes (unions in the total order
 *                -0 < +0) and links, and split word 0 (no kernel reads the split word).  The output is deterministic
 *   not written  the fourth word of a link float4, every treelet that does not improve, slots no link reaches, the root's parent
 * passes in 1..8; the gain per pass falls quickly.  Restructuring can deepen a tree: the tracer's stack limit (104
 * entries) and its sticky overflow word (ntr_trace_status) are unchanged, and result->heightAfter lets a caller check.
 * The call BLOCKS: per pass the host reads the height histogram back to size its launches, so it cannot be captured into a HIP graph
 * (NTR_ERR_INVALID on a capturing stream).  result may be NULL.  Scratch (48 B per node slot; 56 B for ntr_bvh_sah_cost, which shares the pool) comes from a per-device grow-only
 * pool that ntr_lbvh_release_workspace returns.  One optimise or refit per device at a time.
 * Afterwards the caller re-runs ntr_bvh_validate (flags and the top-of-tree table depend on the boxes) and recomputes
 * ntr_bvh_leaf_depths (they are topology); scheduling hints (NtrSchedHint) stay legal, because they only ever order blocks.
 * A child link outside the node extent, or a child word 0 below the root, is never followed: it counts as a leaf link that cannot be
 * expanded, and the former makes the call return NTR_ERR_LAYOUT after the work, as ntr_bvh_refit's blocking form does.  Boxes with
 * NaN are out of contract: the result is then unspecified but still a tree over the same leaf links, and nothing outside the buffer
 * is touched.
 * NTR_ERR_INVALID (before any device work): null d_nodes, nodesBytes not a multiple of 64 in [64, 0x76543200], passes outside 1..8.
 * Without a device: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrBvhOptimizeResult {
    int32_t passes, numNodes, numLeafLinks, pad;   /* passes run; reached slots and the leaf links below them */
    int32_t formed[8], rewritten[8];               /* per pass: treelets formed, and those of them rewritten */
    int32_t heightBefore[8], heightAfter[8];       /* per pass: inner nodes on the longest root-to-leaf path */
    float   seconds;                               /* GPU time of the call */
} NtrBvhOptimizeResult;
NTR_API int ntr_bvh_optimize(void* d_nodes, int64_t nodesBytes, int32_t passes, NtrBvhOptimizeResult* result /* may be NULL */,
                             void* stream);
/* Bytes the scratch pool of ntr_bvh_optimize / ntr_bvh_sah_cost holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_optimize_scratch_bytes(int64_t* bytes);

/* HLBVHBuilder::calcSAHGPU (src/rt/bvh/HLBVH/HLBVHBuilder.cpp:752-770; kernel calcSAH / calcSAHNode / calcLeafs,
 * emitTreeKernel.cu:1351-1400): the SAH cost of a Compact tree, sahCost = calcSAHNode(0).  The reference runs the recursion in one
 * thread and compiles it -use_fast_math, so it defines no bits; here every node is computed in strict binary32 in source order
 * (fminf / fmaxf: the other operand for a NaN, else the total order -0 < +0; areas 2*((dx*dy + dy*dz) + dz*dx); the node's value
 * fl(fl(1 + fl(fl(pl/pa) * l)) + fl(fl(pr/pa) * r)) with the correctly rounded divide; a leaf child's value is its triangle count up
 * to the terminator) by a parallel bottom-up pass in which the second arrival at a node computes it, so the result does not depend on
 * timing.  Zero areas give infinities and NaNs as IEEE does; they are returned as they come.  The numpy spec is
 * tests/np_bvh_optimize.py sah_cost().  Blocking, not capturable.  A child link outside the extent or a leaf without a terminator
 * inside d_triWoop counts as 0 and makes the call return NTR_ERR_LAYOUT; a child word 0 counts as 0.
 * NTR_ERR_INVALID (before any device work): a null pointer, nodesBytes not a multiple of 64 in [64, 0x76543200], triWoopBytes not a
 * positive multiple of 16.  Without a device: NTR_ERR_NO_DEVICE / NTR_ERR_HIP. */
typedef struct NtrBvhSahResult {
    float   sahCost;
    int32_t numNodes, numLeaves, numTris, height;   /* reached slots, their negative child words, the leaves' triangles, inner nodes
                                                       on the longest root-to-leaf path */
    float   seconds;                                /* GPU time of the call */
} NtrBvhSahResult;
NTR_API int ntr_bvh_sah_cost(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes,
                             NtrBvhSahResult* result, void* stream);

/* ntr_bvh_optimize_batch: ntr_bvh_optimize over many BLASes of a pool in one pass (csrc/bvh_optimize_batch_kernels.hip).
 * EXTENSION without a reference counterpart; the rule is tests/np_optimize_batch.py::optimize, that is np_bvh_optimize.optimize over
 * every entry's node slice.  After the call every listed BLAS's node range holds what ntr_bvh_optimize(pool + nodesOffset, nodesBytes,
 * passes) writes, and every other byte of the pool is untouched.  Only nodesOffset and nodesBytes of an entry are read: leaves, Woop rows
 * and triIndex stay as they are, so no row pointer is passed.  The entries are any subset of the pool's BLASes in any order, with gaps.
 *   what stays valid  slot 0 of a BLAS is only ever re-split: the union of its two child boxes (min / max, exact) keeps its bits, so a
 *                top-level tree over the pool, its records and ntr_tlas_refit's result stay valid.  A wide pool made from the BLASes
 *                does not: re-widen it (ntr_pool_widen_batch)
 *   host cost    every kernel covers all entries (a joint slot space: the running sum of the entries' slot counts), and a height of
 *                treelets is one launch for all entries, so launches <= passes * (5 + H) + 2, H the greatest height of any entry in
 *                any pass.  One read-back per pass (the tallest height and the histogram's first 1024 words; one more only for a tree
 *                taller than that), one after the final measuring round, one more for entryResults != NULL.  result->launches and
 *                result->readBacks report what was issued
 *   results      entryResults[k] (may be NULL): reached slots and leaf links, the height before the first and after the last pass,
 *                errBits.  *result (may be NULL): formed / rewritten per pass summed over the entries, the tallest heights,
 *                firstBadEntry (-1: none; the lowest index) and the OR of the entries' errBits, seconds (GPU time of the call)
 * The call BLOCKS and is refused on a capturing stream.  Scratch: 40 B per listed slot (56 B for ntr_bvh_sah_cost_batch, which shares
 * the pool), 88 B per entry and two tables of as many words as the largest entry has slots, in a per-device grow-only pool of its own
 * that ntr_lbvh_release_workspace returns.
 * NTR_ERR_INVALID before any device work: null entries or d_poolNodes; numEntries outside 1..2^20; passes outside 1..8; poolNodesBytes
 * not a multiple of 64 in [64, 0xFFFFFF00]; d_poolNodes not 16-byte aligned; an entry's node range misaligned, empty, outside the pool or
 * above 0x76543200 bytes; two entries whose node ranges overlap or repeat (a BLAS is restructured once per call); a capturing stream.
 * Without a device, after those checks: NTR_ERR_NO_DEVICE / NTR_ERR_HIP.
 * NTR_ERR_LAYOUT, after the work, with *result and entryResults filled and every other entry optimised completely:
 *   NTR_OPT_ERR_LINK     a child link outside its BLAS's extent: never followed, it counts as a leaf link (ntr_bvh_optimize's rule);
 *                        a link is always judged against its own BLAS's slot count, so one that would land in a neighbour names nobody
 *   NTR_OPT_ERR_NO_TREE  the links form no tree under the entry's slot 0 -- the bottom-up pass never completes slot 0, or slot 0 has no
 *                        child at all, as a zero-filled slot has: the entry is left entirely unchanged in every pass (ntr_bvh_optimize
 *                        leaves a zero-filled slot 0 unchanged too, without an error) */
enum { NTR_OPT_ERR_LINK = 1, NTR_OPT_ERR_ROW = 2, NTR_OPT_ERR_NO_TREE = 4 };
typedef struct NtrBvhOptimizeBatchEntry {          /* host array, one per listed BLAS: 32 bytes */
    int32_t numNodes, numLeafLinks;                /* reached slots and the leaf links below them (0, 0 without a tree) */
    int32_t heightBefore, heightAfter;             /* before the first pass, after the last */
    int32_t errBits, pad[3];
} NtrBvhOptimizeBatchEntry;
typedef struct NtrBvhOptimizeBatchResult {
    int32_t numEntries, passes;
    int64_t formed[8], rewritten[8];               /* per pass, summed over the entries */
    int32_t maxHeightBefore, maxHeightAfter;       /* the tallest entry before the first pass and after the last */
    int32_t firstBadEntry, errBits;
    int32_t launches, readBacks;                   /* kernel launches and blocking device-to-host copies issued */
    float   seconds;
    int32_t pad;
} NtrBvhOptimizeBatchResult;
NTR_API int ntr_bvh_optimize_batch(int32_t numEntries, const NtrBlasRange* entries, void* d_poolNodes, int64_t poolNodesBytes,
                                   int32_t passes, NtrBvhOptimizeBatchEntry* entryResults /* numEntries, may be NULL */,
                                   NtrBvhOptimizeBatchResult* result /* may be NULL */, void* stream);
/* Bytes the scratch pool of ntr_bvh_optimize_batch / ntr_bvh_sah_cost_batch holds on the current device (0 after
 * ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_optimize_batch_scratch_bytes(int64_t* bytes);

/* ntr_bvh_sah_cost_batch: ntr_bvh_sah_cost of many BLASes of a pool in two launches and one read-back (same unit; the rule is
 * tests/np_optimize_batch.py::sah_costs).  entryResults[k] equals what ntr_bvh_sah_cost returns at pool + offsets in sahCost (bit for
 * bit), numNodes, numLeaves, numTris and height; its seconds is 0, the call's GPU time is result->seconds.  A leaf counts its rows to
 * the terminator inside its own BLAS's row range only.  The call only reads the pool, so entries may repeat or overlap.  Blocking, not
 * capturable.  A malformed entry counts 0 where it cannot follow (NTR_OPT_ERR_LINK, NTR_OPT_ERR_ROW) or, without a tree under its slot 0,
 * is reported as zeros (NTR_OPT_ERR_NO_TREE); the call then returns NTR_ERR_LAYOUT with firstBadEntry, and every result is filled.
 * NTR_ERR_INVALID before any device work: ntr_bvh_optimize_batch's cases for the nodes (but for the overlap rule), the same for the
 * rows (poolTriWoopBytes a multiple of 16 in [16, 0xFFFFFF00], a 16-byte aligned pointer, every row range a positive multiple of 16
 * inside it), null entryResults.  NTR_ERR_OVERFLOW: the entries list more than 0xFFFFFF00 / 64 slots in all (only where they repeat). */
typedef struct NtrBvhSahBatchResult {
    int32_t numEntries, firstBadEntry, errBits;
    int32_t launches, readBacks;
    float   seconds;
} NtrBvhSahBatchResult;
NTR_API int ntr_bvh_sah_cost_batch(int32_t numEntries, const NtrBlasRange* entries, const void* d_poolNodes, int64_t poolNodesBytes,
                                   const void* d_poolTriWoop, int64_t poolTriWoopBytes, NtrBvhSahResult* entryResults /* numEntries */,
                                   NtrBvhSahBatchResult* result /* may be NULL */, void* stream);

/* On-device renumbering: copy a BVHLayout_Compact tree, whatever built, refitted or restructured it, into the node and row order of
 * the host builder (CudaBVH::createCompact, CudaBVH.cpp:594-652): a stack holding slot 0; pop a slot and, for child 0 then child 1, an
 * inner child takes the next node slot and is pushed, a leaf child takes the next rows.  So siblings share a 128-byte line, a node's
 * direct leaves precede everything below it, and a subtree is contiguous (child 1's before child 0's).
 * (csrc/bvh_reorder_kernels.hip).  EXTENSION without a reference counterpart as a pass of its own: the rule is pinned by the numpy
 * spec tests/np_bvh_reorder.py (its docstring is the normative text).  Out of place and deterministic; the input tree is only read.
 *   written      d_outNodes[0, 64 * numNodes): node v at its new slot, words 0-11, 14 and 15 unchanged, words 12 and 13 the new links
 *                (64 * new slot, ~new row, or 0); d_outTriWoop[0, 16 * numRows) and d_outTriIndex[0, 4 * numRows): for every leaf
 *                link its own copy, bit for bit, of the leaf's rows (row ~link + 3j up to the first whose x word is 0x80000000, that
 *                terminator included; only a triangle's first row is tested) and of the triIndex words beside them.  A leaf two
 *                links name is copied twice
 *   not written  everything beyond those extents; node slots no link reaches and rows no reached leaf link names are dropped
 *   errors       a child link > 0 that names no slot of the buffer is copied unchanged, and a leaf without a terminator inside
 *                d_triWoop is emitted as a lone terminator row (so the output stays traceable); either makes the call return
 *                NTR_ERR_LAYOUT after the work.  Links that form no tree under slot 0 (a cycle, a slot named twice): NTR_ERR_LAYOUT,
 *                nothing written.  NTR_ERR_OVERFLOW, nothing written: the tree has more nodes or rows (the counts saturate) than the
 *                output capacities, 31 019 208 nodes or 2^31 - 1 rows hold; result then still carries the counts and extents.
 *                Capacities equal to the input extents always suffice for a tree whose leaf links name distinct leaves
 * The call BLOCKS and makes one read-back (the totals and the error word) between the placement and the copies, so it cannot be
 * captured into a HIP graph (NTR_ERR_INVALID on a capturing stream).  It ends on any input: every loop is bounded and no workgroup
 * waits for another.  Scratch (52 B per node slot and 16 KB of counters) comes from a per-device grow-only pool that
 * ntr_lbvh_release_workspace returns.  One reorder, optimise or refit per device at a time.
 * Afterwards ntr_bvh_validate flags, ntr_bvh_sah_cost and ntr_bvh_leaf_depths of the output equal the input's (the tree is the same);
 * the top-of-tree table is the output buffer's own, so the caller validates the new buffer before a flagged trace.
 * NTR_ERR_INVALID (before any device work): a null pointer (result included), nodesBytes not a multiple of 64 in [64, 0x76543200],
 * triWoopBytes not a positive multiple of 16, triIndexBytes * 4 < triWoopBytes, an output capacity <= 0, an output range that
 * overlaps an input range or another output range.  Without a device: NTR_ERR_NO_DEVICE / NTR_ERR_HIP (no CPU fallback). */
typedef struct NtrBvhReorderResult {
    int64_t nodesBytes, triWoopBytes, triIndexBytes;   /* extents of the output tree */
    int32_t numNodes, numLeaves, numRows, numDroppedSlots;   /* reached slots, their leaf links, the rows written, slots of the
                                                                 input no link reaches */
    float   seconds;                                   /* GPU time of the call */
} NtrBvhReorderResult;
NTR_API int ntr_bvh_reorder(const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes,
                            const int32_t* d_triIndex, int64_t triIndexBytes,
                            void* d_outNodes, int64_t outNodesCapacity, void* d_outTriWoop, int64_t outTriWoopCapacity,
                            int32_t* d_outTriIndex, int64_t outTriIndexCapacity,
                            NtrBvhReorderResult* result, void* stream);
/* Bytes the reorder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int ntr_bvh_reorder_scratch_bytes(int64_t* bytes);

/* reconstructKernel (src/rt/cuda/RendererKernels.cu:59-172; ReconstructInput, RendererKernels.hpp:46-70;
 * Renderer::updateResult, Renderer.cpp:583-659): hit records of one batch -> ABGR8 pixels.
 * rayType 0 = primary, 1 = AO, 2 = diffuse (textured / path-traced / VPL shading: out of scope). */
NTR_API int ntr_reconstruct(int32_t rayType, int32_t numRaysPerPrimary, int32_t firstPrimary, int32_t numPrimary,
                            const int32_t* d_primarySlotToID, const NtrRayResult* d_primaryResults,
                            const int32_t* d_batchIDToSlot, const NtrRayResult* d_batchResults,
                            const uint32_t* d_triMaterialColor, const uint32_t* d_triShadedColor,
                            uint32_t* d_pixels, void* stream);

/* RayBuffer::mortonSort (src/rt/ray/RayBuffer.cpp:103-165; kernels RayBufferKernels.cu:70-197): reorder a
 * batch by the 192-bit origin/direction Morton key.  The reference sorts the keys on the CPU; here the
 * whole pipeline runs on the device.  Ties keep their original slot order.  Out-of-place. Blocking. */
NTR_API int ntr_ray_morton_sort(int32_t numRays, const NtrRay* d_inRays, const int32_t* d_inSlotToID,
                                NtrRay* d_outRays, int32_t* d_outIDToSlot, int32_t* d_outSlotToID,
                                void* stream, float* seconds);

/* ---- multi-GPU (new design: the reference is single-device, its launches synchronous on one
 * context, src/framework/gpu/CudaKernel.cpp:188-221) ----------------------------------------------------------------
 * One process per GPU, or one host thread per GPU in one process.  Rays shard by screen tile: the primary-ray index
 * space [0, W*H) -- already 8 x 8 pixel blocks in Morton order (PixelTable, src/rt/ray/PixelTable.cpp:77-122) -- is
 * cut into `world` contiguous ranges of whole 64-ray blocks; a rank's AO / diffuse rays derive from its own primary
 * hits, so no ray ever crosses a rank boundary.  The BVH is built once and replicated by broadcast; the ONLY
 * collective of a frame is the final gather of hit records (16 B per primary ray) or of the RGBA8 framebuffer (4 B per
 * pixel: 8.3 MB at 1080p) to the root, over RCCL (grouped point-to-point sends over xGMI).  RCCL is bound at run time
 * (dlopen), only by the ntr_dist_* calls.  The group calls are collective: every rank makes the same call. */
typedef struct NtrDist NtrDist;
#define NTR_DIST_ID_BYTES 128
/* The rank-th of `world` contiguous, align-ray-aligned ranges of [0, numPrimary) (the first ranges one block longer
 * when the blocks do not divide), and the AO batches of a range as RayGen::batching cuts them (src/rt/ray/RayGen.cpp:
 * 582-602; at most maxBatchRays output rays each): first[b], count[b] are input slots.  No device, no RCCL. */
NTR_API int ntr_frame_shard(int32_t numPrimary, int32_t rank, int32_t world, int32_t align, int32_t* lo, int32_t* hi);
NTR_API int ntr_frame_ao_batches(int32_t lo, int32_t hi, int32_t samples, int32_t maxBatchRays, int32_t* first, int32_t* count,
                                 int32_t capacity, int32_t* numBatches);
/* Group set-up.  Processes: the root calls ntr_dist_unique_id and hands the 128 bytes to every rank by any means (file,
 * socket, MPI, environment); every rank then calls ntr_dist_init on ITS device (ntr_set_device first).  Threads of one
 * process: ntr_dist_init_all creates one group object per device (devices == NULL: 0 .. numDevices - 1); thread i uses
 * out[i] after ntr_set_device(devices[i]). */
NTR_API int ntr_dist_unique_id(char id[NTR_DIST_ID_BYTES]);
NTR_API int ntr_dist_init(const char id[NTR_DIST_ID_BYTES], int32_t rank, int32_t world, NtrDist** out);
NTR_API int ntr_dist_init_all(int32_t numDevices, const int32_t* devices, NtrDist** out /* numDevices entries */);
NTR_API int ntr_dist_info(const NtrDist* dist, int32_t* rank, int32_t* world);
NTR_API int ntr_dist_destroy(NtrDist* dist);
/* BVH replication: `bytes` of device memory from `root` to every rank (asynchronous on `stream`); _bvh does the three
 * BVHLayout_Compact buffers (every rank passes buffers of the root's sizes). */
NTR_API int ntr_dist_broadcast(NtrDist* dist, void* d_buf, int64_t bytes, int32_t root, void* stream);
NTR_API int ntr_dist_broadcast_bvh(NtrDist* dist, void* d_nodes, int64_t nodesBytes, void* d_triWoop, int64_t triWoopBytes,
                                   int32_t* d_triIndex, int64_t triIndexBytes, int32_t root, void* stream);
/* The frame's one collective.  _records: rank r's hit records of its range (hi_r - lo_r records, d_ownRecords) land at
 * d_fullRecords + lo_r on the root (numPrimary records; ignored elsewhere).  _pixels: rank r's pixels -- the tiles of
 * its range inside its own W*H framebuffer d_ownPixels, as ntr_reconstruct wrote them -- land in the root's framebuffer
 * d_fullPixels; d_slotToPixel is the PixelTable's index-to-pixel map (ntr_pixel_table), d_scratch numPrimary words on
 * every rank.  Asynchronous on `stream`.  As with any collective, every rank of the group makes the matching call: a rank that
 * returns an argument error has posted nothing and its peers wait for it (argument errors must be uniform across ranks; the ranges
 * are, by construction).  _records_cuts: the same gather for ranges the host cut itself (cuts[0] = 0 <= cuts[1] <= ... <=
 * cuts[world] = numPrimary, the same table on every rank: ranges of equal predicted cost instead of equal ray counts).
 * bench.py --gpus N gathers through these calls (torch.distributed only carries the 128-byte id and the barriers);
 * tests/test_dist_native_gpu.py runs them over two devices from two host threads wherever the box has two GPUs (on one-GPU boxes:
 * world size 1, and the N-rank flow at N = 2-3 with host-staged collectives, bench.py --dist-backend gloo --one-device). */
NTR_API int ntr_dist_gather_records(NtrDist* dist, const NtrRayResult* d_ownRecords, int32_t numPrimary, int32_t align,
                                    NtrRayResult* d_fullRecords, int32_t root, void* stream);
NTR_API int ntr_dist_gather_records_cuts(NtrDist* dist, const NtrRayResult* d_ownRecords, const int32_t* cuts /* world + 1 */,
                                         NtrRayResult* d_fullRecords, int32_t root, void* stream);
NTR_API int ntr_dist_gather_pixels(NtrDist* dist, const uint32_t* d_ownPixels, const int32_t* d_slotToPixel, int32_t numPrimary,
                                   int32_t align, uint32_t* d_fullPixels, uint32_t* d_scratch, int32_t root, void* stream);

/* ---- host-side BVH production (no device work) ---------------------------- */

/* Host SAH build + Compact flatten: `BVH bvh(scene, platform, params);
 * CudaBVH(bvh, BVHLayout_Compact)` of Renderer::getCudaBVH
 * (src/rt/cuda/Renderer.cpp:282-285; SAHBVHBuilder.cpp:51-254; CudaBVH.cpp:579-687)
 * with Platform("GPU") and setLeafPreferences(minLeaf,maxLeaf) (Renderer.cpp:88-89
 * uses 1,1).  Returns an opaque handle holding host copies of the three buffers. */
typedef struct NtrHostBvh NtrHostBvh;
typedef struct NtrHostBvhInfo {
    const void*    nodes;     int64_t nodesBytes;
    const void*    triWoop;   int64_t triWoopBytes;
    const int32_t* triIndex;  int64_t triIndexBytes;
    int32_t layout;
    int32_t numInnerNodes, numLeafNodes, maxDepth;
    float   buildSeconds;
} NtrHostBvhInfo;
NTR_API int  ntr_sah_build(int32_t numTris, const int32_t* triVtxIndex /* 3 per tri */,
                           int32_t numVerts, const float* vtxPos /* 3 per vertex */,
                           int32_t minLeafSize, int32_t maxLeafSize, NtrHostBvh** out);
NTR_API int  ntr_host_bvh_info(const NtrHostBvh* bvh, NtrHostBvhInfo* info);
NTR_API void ntr_host_bvh_free(NtrHostBvh* bvh);

/* A host BVH object over copies of existing BVHLayout_Compact buffers (e.g. the three buffers of a bvhcache file,
 * CudaBVH::CudaBVH(InputStream&), src/rt/cuda/CudaBVH.cpp:105-116, or a device-built LBVH downloaded to the host). */
NTR_API int ntr_host_bvh_wrap(const void* nodes, int64_t nodesBytes, const void* triWoop, int64_t triWoopBytes,
                              const int32_t* triIndex, int64_t triIndexBytes, NtrHostBvh** out);

/* CudaAS::trace(RayBuffer&, Buffer& visibility) -- the reference's HOST tracer (src/rt/cuda/CudaAS.hpp:62,
 * CudaBVH::trace, src/rt/cuda/CudaBVH.cpp:213-302; used by its CPURenderer and by BASELINE configuration 1): rays
 * and results are HOST arrays, visibility (may be NULL / 0) receives 1 at the id of every triangle hit, stats (may
 * be NULL) the reference's RayStats counters (numLeafVisits / numHits stay 0: the reference does not count them).
 * Single-threaded, like the reference.  This is an API of its own for host-side callers, NOT a fallback of
 * ntr_trace_bvh, which never runs on the CPU and fails without a HIP device. */
NTR_API int ntr_host_bvh_trace(const NtrHostBvh* bvh, int32_t numRays, int32_t anyHit, const NtrRay* rays,
                               NtrRayResult* results, int32_t* visibility, int32_t numVisibility, NtrTraceStats* stats);

/* ---- kd-tree (Renderer.dataStructure KDTree: Renderer.cpp:75-76, 309-382, 415-416) ---------------------- */

/* Host kd-tree build + flatten: `KDTree kdtree(scene, platform, params); CudaKDTree(kdtree)` of Renderer::getCudaKDTree
 * (Renderer.cpp:309-382; KDTree.cpp:36-63; CudaKDTree.cpp:18-183), no device work.  builder: NTR_KDTREE_SPATIAL_MEDIAN
 * (NaiveKDTreeBuilder: axis level % 3, split at the cell's middle, leaves at <= maxLeafSize references or depth 18) or
 * NTR_KDTREE_SAH (FastKDTreeBuilder: event sweep with clipping of straddling triangles, Platform("GPU") costs, depth
 * <= (int)(1.2 log2 N + 2)); maxLeafSize applies to the spatial median only (the Renderer passes 1, Renderer.cpp:88-89).
 * Both builders are single-threaded and deterministic.  numTris == 0 -> NTR_ERR_INVALID.
 *
 * Buffers (ntrace_amd/host/CudaKDTree.hpp):
 *   nodes    16 B per inner node (left, right, floatBits(split), axis << 28), numbered by createNodeTriIdx's explicit stack;
 *            a child is a node index (>= 0), ~offset of a non-empty leaf's list in triIndex, or 0x80000000 (empty leaf)
 *   triIndex each non-empty leaf's triangle ids, then 0x80000000
 *   triWoop  3 x float4 per scene triangle, by triangle id, padded to 4096 B (the rows of ntr_sah_build's tree)
 *   sceneMin / sceneMax  the box of every triangle some leaf references; delta = length(sceneMax + sceneMin) * 1e-6
 * DEVIATION: when the root is a leaf (one triangle, or no SAH split at the root) -- where the reference's kernel reads a
 * child of the root -- the tree is one inner node on axis 0 at sceneMax.x with the leaf as child 0 and an empty leaf as
 * child 1. */
#define NTR_KDTREE_SPATIAL_MEDIAN 0
#define NTR_KDTREE_SAH 1
typedef struct NtrHostKdtree NtrHostKdtree;
typedef struct NtrHostKdtreeInfo {
    const void*    nodes;     int64_t nodesBytes;
    const void*    triWoop;   int64_t triWoopBytes;
    const int32_t* triIndex;  int64_t triIndexBytes;
    float   sceneMin[3], sceneMax[3];
    float   delta;
    int32_t numInnerNodes, numLeafNodes, numEmptyLeaves, numTriRefs;
    int32_t maxDepth;          /* inner nodes on the longest root-to-leaf path: the kernel's stack never holds more entries */
    float   percentDuplicates; /* duplicated references / triangles * 100 (KDTree.cpp:68) */
    float   buildSeconds;
} NtrHostKdtreeInfo;
NTR_API int  ntr_kdtree_build(int32_t builder, int32_t numTris, const int32_t* triVtxIndex /* 3 per tri */,
                              int32_t numVerts, const float* vtxPos /* 3 per vertex */, int32_t maxLeafSize, NtrHostKdtree** out);
NTR_API int  ntr_host_kdtree_info(const NtrHostKdtree* kdtree, NtrHostKdtreeInfo* info);
NTR_API void ntr_host_kdtree_free(NtrHostKdtree* kdtree);

/* A host kd-tree over copies of buffers made elsewhere (e.g. CudaKDTree(InputStream&), CudaKDTree.cpp:35-40).  The tree is
 * walked from node 0 first: every child index in range, every axis 0..2, every leaf list inside triIndex and terminated by
 * 0x80000000 with its ids inside triWoop, no node reached twice (no cycles, no shared subtrees), and a depth (inner nodes on a
 * root-to-leaf path) of at most 64, the kernel's stack.  Otherwise NTR_ERR_INVALID (sizes, nulls) or NTR_ERR_LAYOUT. */
NTR_API int  ntr_host_kdtree_wrap(const void* nodes, int64_t nodesBytes, const void* triWoop, int64_t triWoopBytes,
                                  const int32_t* triIndex, int64_t triIndexBytes, const float sceneMin[3], const float sceneMax[3],
                                  NtrHostKdtree** out);

/* Replaces the `trace_kdtree` launch of CudaKDTreeTracer::traceBatch (CudaKDTreeTracer.cpp:70-128; kernel
 * fermi_kdtree_while_while_leafRef.cu with SHORTSTACK 0, restated in csrc/kdtree_kernels.hip).  delta is computed here as
 * the reference does: length(sceneMax + sceneMin) * 1e-6f in binary32.
 *   numRays == 0 -> NTR_OK, *seconds = 0;  a null buffer -> NTR_ERR_INVALID;  seconds != NULL -> timed and blocking (the
 *   kernel's GPU time), NTR_ERR_OVERFLOW if a ray's stack overflowed, NTR_ERR_LAYOUT if a ray met an index outside its
 *   buffer;  seconds == NULL -> asynchronous, the status bits go to the per-device word of ntr_trace_status (bit 0 overflow,
 *   bit 1 index out of range).
 * Records: hit = (triId, t, bits(u), bits(v)); miss = (-1, ray.tmax, 0, 0) -- DEVIATION: the reference stores its working
 * tmax on a miss, a value nothing reads.  anyHit is ignored, as by the reference's kernel. */
NTR_API int ntr_trace_kdtree(int32_t numRays, int32_t anyHit, const float sceneMin[3], const float sceneMax[3],
                             const NtrRay* d_rays, NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes,
                             const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex, int64_t triIndexBytes,
                             void* stream, float* seconds);

/* On-device kd-tree build: the reference's persistent kd-tree builder as configured (Renderer.cpp:348-353 "PersistentKDTree";
 * CudaPersistentKDTreeBuilder.cpp, persistent_kdtree.cu with CudaTracerDefines.h SPLIT_TYPE 5, PLANE_COUNT 32, TRIANGLE_CLIPPING 0,
 * BINNING_TYPE 2; config.conf block PersistentKDTree), rebuilt breadth first, one level per round, without its persistent task pool
 * or device heap (csrc/kdtree_build_kernels.hip; the spec is tests/np_kdtree_binned.py).  The tree feeds ntr_trace_kdtree unchanged.
 *   candidates  32 planes per task, 11 / 11 / 10 on x / y / z, pos = lo + (hi - lo) * ((1 + k) / 12.f), two roundings
 *               (findPlaneAABB, rt_common.cu:1007-1030)
 *   sides       no clipping: a triangle is left iff fl(pos - min) > -1e-8f and right iff fl(pos - max) < 1e-8f over its extent on
 *               the axis -- exactly getPlanePosition (rt_common.cu:331-400) over its three vertices, as rounded subtraction is monotone
 *   cost        s = areaL * nL + areaR * nR (areaAABBX/Y/Z, rt_common.cu:850-905); CANONICAL: the lowest finite s wins (+0 == -0),
 *               then the lowest plane (lower axis, then lower position); NaN and infinite s never win; no finite s -> the task is a leaf
 *   termination (persistent_kdtree.cu:454-510) ratio = (ct + ci * s / areaParent) / (ci * n); ratio > failRq increments the task's
 *               failure counter (children inherit it) and a counter above failureCount makes the task a leaf; a NaN ratio (a cell of
 *               zero area) does not; a child with <= triLimit references or below a parent of depth > maxDepth - 2 is a leaf, with
 *               maxDepth = int(depthK1 * log2f(numTris) + depthK2) (CudaPersistentKDTreeBuilder.cpp:451), root depth 0.
 *               triMaxLimit is only read by the reference's object-SAH path (not compiled with SPLIT_TYPE 5): accepted, unused.
 *   cells       the root cell is the box of the triangles' vertices (min / max with -0 < +0); children cut it at the plane
 *   order       inner nodes in level order (root 0, child 0 before child 1); leaf lists in the same order, ascending triangle ids
 *               (the partition is stable), each followed by 0x80000000; empty leaves are the child 0x80000000.  The buffers are those
 *               of NtrHostKdtreeInfo: Woop rows of woop_rows.h (the device builders' rows) by triangle id, padded to 4096 B.
 * DEVIATION: a root with <= triLimit triangles, or one the failure test or the no-finite-cost rule ends, is the root-leaf tree of
 *   ntr_kdtree_build (one inner node on axis 0 at sceneMax.x over the leaf and an empty leaf).
 * DEVIATION: the reference's builder overwrites failureCount with int(failK1 * maxDepth + failK2) (CudaPersistentKDTreeBuilder.cpp:452);
 *   here it is the parameter as given (config.conf: 0).
 * NTR_ERR_INVALID: numTris < 1 or > 2^28, numVerts < 1, a null pointer, triLimit < 1, triMaxLimit < 0, failureCount < 0, a
 *   non-finite depthK1 / depthK2 / ci / ct / failRq, a maxDepth above 64 (the trace kernel's stack), or (found on the device) a
 *   vertex index outside [0, numVerts).  NTR_ERR_NOMEM: device memory, or a level whose references, leaf entries or nodes would not
 *   fit the kernels' int32 indexing.  NTR_ERR_LAYOUT: an internal consistency check of the partition failed (a reference's rank
 *   outside its child's range; not expected, reported instead of writing out of bounds).
 * The call blocks (one 32 B read-back per level).  The scratch is a per-device grow-only pool returned by ntr_lbvh_release_workspace:
 * one build per device at a time.  The tree's buffers belong to its handle, so trees coexist until ntr_device_kdtree_free.
 * params == NULL: the config.conf defaults (ntr_kdtree_device_params_default). */
typedef struct NtrKdtreeDeviceParams {
    int32_t triLimit, triMaxLimit, failureCount, pad;
    float   depthK1, depthK2, ci, ct, failRq;
} NtrKdtreeDeviceParams;
typedef struct NtrDeviceKdtree NtrDeviceKdtree;
typedef struct NtrDeviceKdtreeInfo {   /* device pointers (owned by the tree) and exact byte sizes, as NtrHostKdtreeInfo */
    const void*    nodes;     int64_t nodesBytes;
    const void*    triWoop;   int64_t triWoopBytes;
    const int32_t* triIndex;  int64_t triIndexBytes;
    float   sceneMin[3], sceneMax[3], delta;
    int32_t numInnerNodes, numLeafNodes, numEmptyLeaves, numTriRefs;
    int32_t maxDepth;          /* inner nodes on the longest root-to-leaf path */
    int32_t numLevels;         /* rounds of the level loop */
    float   percentDuplicates; /* (numTriRefs - numTris) / numTris * 100 */
    float   seconds;           /* host wall clock of the whole call */
    float   prepMs, levelsMs, emitMs;   /* GPU event times: per-triangle data, the level loop, the final copies */
} NtrDeviceKdtreeInfo;
NTR_API int  ntr_kdtree_device_params_default(NtrKdtreeDeviceParams* params);
NTR_API int  ntr_kdtree_device_build(int32_t numTris, const int32_t* d_triVtxIndex, int32_t numVerts, const float* d_vtxPos,
                                     const NtrKdtreeDeviceParams* params, NtrDeviceKdtree** out, void* stream);
NTR_API int  ntr_device_kdtree_info(const NtrDeviceKdtree* tree, NtrDeviceKdtreeInfo* info);
NTR_API void ntr_device_kdtree_free(NtrDeviceKdtree* tree);
/* Blocking copies of the three buffers (nodesBytes / triWoopBytes / triIndexBytes of the info) to host memory; a null destination
 * is skipped. */
/* Bytes the builder's per-device scratch pool holds on the current device (0 after ntr_lbvh_release_workspace). */
NTR_API int  ntr_kdtree_device_scratch_bytes(int64_t* bytes);
NTR_API int  ntr_device_kdtree_download(const NtrDeviceKdtree* tree, void* nodes, void* triWoop, int32_t* triIndex);

/* ---- scene ingest (host only) ----------------------------------------------- */

/* CameraControls::decodeSignature / encodeSignature (src/framework/3d/CameraControls.cpp:342-399, 471-545):
 * out = position[3], forward[3], up[3], speed, fov, near, far, keepAligned. */
NTR_API int ntr_camera_decode(const char* signature, float out[16]);
NTR_API int ntr_camera_reencode(const char* signature, char* out, int32_t outSize);
/* invert(fitToView(-1, 2) * perspective * worldToCamera) of Renderer::beginFrame (Renderer.cpp:473-477),
 * row-major, ready for ntr_raygen_primary. */
NTR_API int ntr_camera_nscreen_to_world(const char* signature, int32_t viewW, int32_t viewH, float matrix[16],
                                        float position[3], float* cameraFar);

/* Wavefront OBJ import with the reference's vertex / triangle numbering
 * (src/framework/io/MeshWavefrontIO.cpp:412-485, src/rt/Scene.cpp:101-136). */
typedef struct NtrObjMesh NtrObjMesh;
NTR_API int  ntr_obj_load(const char* path, NtrObjMesh** out, int32_t* numTris, int32_t* numVerts, int32_t* numSubmeshes);
NTR_API int  ntr_obj_get(const NtrObjMesh* mesh, int32_t* triVtxIndex /* 3/tri */, float* vtxPos /* 3/vertex */);
NTR_API void ntr_obj_free(NtrObjMesh* mesh);

#ifdef __cplusplus
}
#endif
#endif
