// sched_state.h -- what the trace launch path keeps per device (DeviceState): pool counters, the sticky status word, and the scheduling
// tables -- top-of-tree tables, prediction scratch, automatic hints.  Defined in sched_state.cpp; ntr_api.cpp's trace_impl resolves the
// current device's state once per launch and passes it down.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "ntr_internal.h"

// Scheduling hint (include/ntrace_amd.h): per-block cost of the previous launch -> block order of the next.
struct NtrSchedHint {
    unsigned int* order = nullptr;  // device, numBlocks entries
    unsigned int* cost = nullptr;   // device, numBlocks entries
    int numBlocks = 0;              // 0 = unbound
    int capBlocks = 0;              // blocks the arrays have room for (caller-owned hints grow, never shrink: a frame's short last batch
                                    // must not cost a hipFree -- a device-wide synchronisation -- and two hipMallocs every frame)
    int device = -1;
    int uses = 0;                   // launches since the hint was (re)bound
    bool valid = false;             // order[] holds a permutation
    bool predicted = false;         // order[] comes from ntr_sched_hint_predict and has not been used yet
};

namespace ntr {

// ---- dispatch-order prediction (sched_kernels.hip) ---------------------------------------------------
// Top-of-tree box tables, one per node buffer seen (keyed by pointer and size; rebuilt by
// ntr_bvh_validate, which hosts call after every (re)build).  A stale table only costs scheduling quality.
struct TopTable {
    const void* nodes = nullptr;
    int64_t bytes = 0;
    void* table = nullptr;           // 2 float4 per box
    unsigned int* count = nullptr;   // boxes in the table
    unsigned long long lastUse = 0;
    bool pinned = false;             // referenced by a captured HIP graph: never evicted
};
constexpr int kTopTables = 16;

// Class counters / lists / block order of one prediction.  A live (not captured) launch uses the entry owned by its stream
// (launches on one stream are ordered; two streams must not share an entry).  A launch that is being captured into a HIP graph
// gets an entry of its OWN, taken from spares that live launches provision (nothing may be allocated during a capture): a graph
// replayed on whatever stream then never shares order[] with a live launch or with another captured launch.  Pinned entries are
// returned to the spares by ntr_trace_graph_release_all().
struct PredictScratch {
    enum State { FREE = 0, LIVE, SPARE, PINNED };
    State state = FREE;
    void* stream = nullptr;              // LIVE: the owning stream (the null stream is a stream like any other)
    unsigned int* classCount = nullptr;  // NTR_SCHED_PRED_WORDS words: class counters + incoherent-block counter (zero whenever no prediction is
                                         // in flight) + the mini-pool K of the last prediction
    unsigned int* classList = nullptr;
    unsigned int* order = nullptr;
    int capBlocks = 0;
    unsigned long long lastUse = 0;
};
constexpr int kScratch = 48;

// Automatic scheduling feedback.  The launch time of the per-ray kernel is set by where its long-lived blocks start;
// what a launch MEASURED about its blocks is the best order for the next launch of the same batch.  The reference's benchmark traces
// every batch 1 + warm-up + measure times (App.cpp:955-958), a renderer with a parked or slowly moving camera regenerates nearly the
// same rays into the same buffers frame after frame -- so the library keeps, per (stream, ray buffer, ray count, ray kind, BVH), the
// scheduling hint a caller could have kept by hand (NtrSchedHint) and uses it without being asked.  Only the dispatch ORDER changes;
// a stale entry (new rays at the old address) is merely a worse order and adapts within a launch or two.  Entries are per stream
// (launches on one stream are ordered, so order[] is never rewritten under a launch that reads it); captured launches do not use them.
struct AutoHint {
    const void* rays = nullptr;
    const void* nodes = nullptr;
    void* stream = nullptr;
    int numRays = 0, anyHit = 0;
    bool used = false;
    int sightings = 0;              // launches of this key: storage is allocated at the second one (a batch seen once pays nothing)
    unsigned long long lastUse = 0;
    NtrSchedHint hint;              // (its arrays come from the stream-ordered allocator: hipMallocAsync / hipFreeAsync on `stream`)
};
constexpr int kAutoHints = 96;

constexpr int kNumCounters = 64;      // ring of counter sets (kPoolHeadsMax heads x 64 B each)
constexpr int kPinnedCounters = 192;  // counter sets handed to launches captured into HIP graphs: never reused

// Everything the trace launch path keeps for ONE device: created on first use without a HIP call, never destroyed (its entries hold
// device memory of a live context).  Per device, because process-global tables behind one lock served a thread-per-GPU driver
// (ntr_dist_init_all) badly: 8 devices x 17 batches are 136 automatic-hint keys for 96 entries, and every launch of
// every device took the same lock.  Only creating a device's state takes a process-wide lock.
struct DeviceState {
    int device = -1;
    std::mutex mu;                       // the counter ring, the pinned counters and the three tables
    std::atomic<bool> ready{false};      // the device memory below exists (current_device_state_ready)
    int numCUs = 0;
    int32_t* counters = nullptr;         // (kNumCounters + kPinnedCounters) sets of pool heads, 64 B apart
    unsigned int* status = nullptr;      // sticky status word; [8] receives its fetch-and-clear
    unsigned long long* stats = nullptr; // 4 counters of the stats variant
    int next = 0;
    int nextPinned = 0;
    unsigned long long clock = 0;        // LRU stamps
    TopTable top[kTopTables];
    PredictScratch scratch[kScratch];
    AutoHint autoHints[kAutoHints];
    std::mutex queryMu;                  // ntr_predict_dispatch_order's own scratch (never a launch's): held until its launches have run
    PredictScratch query;
    std::mutex statusMu;                 // the result word status[8] is shared by the status fetches of the device
};

// The current device's state (created on first use, without a HIP call).  `what` names hipGetDevice in the message of a failure: each
// entry point keeps the text it always had.
int current_device_state(DeviceState** out, const char* what = "hipGetDevice");
// ... and its device memory, allocated on first use: all of it, or nothing (a failed attempt frees what it took).
int current_device_state_ready(DeviceState** out);
// Fetches and clears the sticky status word in ONE device-side step (waits for `s`; *bits receives the word).
int status_fetch(DeviceState* ds, hipStream_t s, unsigned int* bits);

// The device's table for this node buffer (built on first sight, or when `rebuild`).
int top_table_get(DeviceState* ds, const void* d_nodes, int64_t nodesBytes, hipStream_t s, bool rebuild, TopTable** out);
// Grows a prediction scratch to numBlocks (class counters zeroed when first allocated).
int scratch_alloc(PredictScratch* p, int numBlocks);
// The launch's prediction scratch: its stream's entry, or a spare of its own when `s` is being captured (null: none to spare).
int predict_scratch_get(DeviceState* ds, hipStream_t s, int numBlocks, PredictScratch** out);
// The automatic hint of this batch, bound to numBlocks, or null (first sighting, or no entry to be had).
int auto_hint_get(DeviceState* ds, const void* d_rays, const void* d_nodes, int numRays, int anyHit, hipStream_t s, int numBlocks, NtrSchedHint** out);
// Binds a caller-owned hint to a batch of numBlocks blocks on `dev` (its arrays only grow).
int sched_hint_bind(NtrSchedHint* h, int numBlocks, int dev, hipStream_t s);
// A pool-head counter set for a persistent launch: from the ring, or pinned for the graph's lifetime when the launch is captured.
int counter_set_take(DeviceState* ds, bool capturing, int32_t** out);

}  // namespace ntr
