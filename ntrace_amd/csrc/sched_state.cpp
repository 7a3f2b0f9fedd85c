// sched_state.cpp -- the per-device state of the trace launch path (sched_state.h) and the scheduling tables it holds: their lookup
// and recycling rules, hint binding, and the C-ABI entry points that walk the tables (graph reserve / release, stream release, the
// hint objects, the CPU-tier self test of the automatic-hint table).

#include <new>

#include "sched_state.h"
#include "trace_kernels.h"
#include "trace_plan.h"

namespace ntr {

static constexpr size_t kTopTableBytes = (((size_t)2 << NTR_TOP_DEPTH_MAX) + 16) * 32;  // + padding read by predict_kernel's batches
static constexpr int kScratchSpares = 4;   // spares a live launch keeps ready (per device, sized for the largest launch seen) for captured launches
static constexpr int kScratchLive = 16;    // streams with an entry of their own before the least recently used one is recycled

static std::atomic<DeviceState*> g_state[kMaxDevices];
static std::mutex g_stateMu;   // creation only

int current_device_state(DeviceState** out, const char* what)
{
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, what);
    if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
    // the launch path only reads the pointer (acquire): the host threads of a thread-per-GPU driver share no lock here; the process-wide
    // mutex is taken once per device, to create its state
    DeviceState* ds = g_state[dev].load(std::memory_order_acquire);
    if (!ds) {
        std::lock_guard<std::mutex> lk(g_stateMu);
        ds = g_state[dev].load(std::memory_order_relaxed);
        if (!ds) {
            ds = new (std::nothrow) DeviceState();
            if (!ds) return set_error(NTR_ERR_NOMEM, "out of host memory (scheduling state of device %d)", dev);
            ds->device = dev;
            g_state[dev].store(ds, std::memory_order_release);
        }
    }
    *out = ds;
    return NTR_OK;
}

static int alloc_device_memory(DeviceState& s)
{
    const int dev = s.device;
    hipDeviceProp_t prop;
    NTR_HIP(hipGetDeviceProperties(&prop, dev));
    s.numCUs = prop.multiProcessorCount;
    // Counters sit 64 B apart so concurrent launches never share a line.
    NTR_HIP(hipMalloc((void**)&s.counters, (kNumCounters + kPinnedCounters) * kPoolHeadsMax * 64));
    NTR_HIP(hipMalloc((void**)&s.status, 64));
    NTR_HIP(hipMalloc((void**)&s.stats, 256));
    NTR_HIP(hipMemset(s.status, 0, 64));
    return NTR_OK;
}

int current_device_state_ready(DeviceState** out)
{
    int rc = current_device_state(out);
    if (rc != NTR_OK || (*out)->ready.load(std::memory_order_acquire)) return rc;
    DeviceState& s = **out;
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.ready.load(std::memory_order_relaxed)) return NTR_OK;
    rc = alloc_device_memory(s);
    if (rc != NTR_OK) {   // nothing kept: the next call starts over
        if (s.counters) (void)hipFree(s.counters);
        if (s.status) (void)hipFree(s.status);
        if (s.stats) (void)hipFree(s.stats);
        s.counters = nullptr; s.status = nullptr; s.stats = nullptr;
        return rc;
    }
    s.ready.store(true, std::memory_order_release);
    return NTR_OK;
}

int status_fetch(DeviceState* ds, hipStream_t s, unsigned int* bits)
{
    *bits = 0;
    unsigned int st = 0;
    // fetched and cleared in ONE device-side step: a bit set by a launch on another stream is either in this answer or in the next
    std::lock_guard<std::mutex> lk(ds->statusMu);
    const hipError_t xe = ntr_launch_status_exchange(ds->status, ds->status + 8, s);
    if (xe != hipSuccess) return hip_fail(xe, "status_exchange launch");
    NTR_HIP(hipMemcpyAsync(&st, ds->status + 8, sizeof(st), hipMemcpyDeviceToHost, s));
    NTR_HIP(hipStreamSynchronize(s));
    *bits = st;
    return NTR_OK;
}

int counter_set_take(DeviceState* ds, bool capturing, int32_t** out)
{
    // a launch that is being captured into a HIP graph keeps its pool heads for the graph's lifetime
    std::lock_guard<std::mutex> lk(ds->mu);
    if (capturing) {
        if (ds->nextPinned >= kPinnedCounters)
            return set_error(NTR_ERR_NOMEM, "ntr_trace_bvh: more than %d persistent launches captured into HIP graphs", kPinnedCounters);
        *out = ds->counters + kPoolHeadsMax * 16 * (kNumCounters + ds->nextPinned++);
    } else {
        *out = ds->counters + kPoolHeadsMax * 16 * ds->next;
        ds->next = (ds->next + 1) % kNumCounters;
    }
    return NTR_OK;
}

int top_table_get(DeviceState* ds, const void* d_nodes, int64_t nodesBytes, hipStream_t s, bool rebuild, TopTable** out)
{
    std::lock_guard<std::mutex> lk(ds->mu);
    const bool capturing = stream_is_capturing(s);
    TopTable* t = nullptr;
    TopTable* lru = nullptr;
    for (auto& e : ds->top) {
        if (e.nodes == d_nodes && e.bytes == nodesBytes) { t = &e; break; }
        if (!e.pinned && (!lru || e.lastUse < lru->lastUse)) lru = &e;
    }
    bool build = rebuild;
    if (!t) {
        if (!lru) return set_error(NTR_ERR_NOMEM, "ntr_trace_bvh: every top-of-tree table is held by a captured HIP graph");
        if (capturing) return set_error(NTR_ERR_INVALID, "ntr_trace_bvh: first launch on a BVH cannot be captured (trace it once, or call ntr_bvh_validate, before capturing)");
        t = lru;
        if (!t->table) {
            NTR_HIP(hipMalloc(&t->table, kTopTableBytes));
            NTR_HIP(hipMalloc((void**)&t->count, sizeof(unsigned int)));
        }
        t->nodes = d_nodes; t->bytes = nodesBytes;
        build = true;
    }
    t->lastUse = ++ds->clock;
    if (capturing) t->pinned = true;
    if (build) {
        const hipError_t e = ntr_launch_top_table(d_nodes, (unsigned int)nodesBytes, tunables().predictDepth, t->table, t->count, s);
        if (e != hipSuccess) return hip_fail(e, "top_table launch");
    }
    *out = t;
    return NTR_OK;
}

int scratch_alloc(PredictScratch* p, int numBlocks)
{
    if (!p->classCount) {
        NTR_HIP(hipMalloc((void**)&p->classCount, NTR_SCHED_PRED_WORDS * sizeof(unsigned int)));
        NTR_HIP(hipMemset(p->classCount, 0, NTR_SCHED_PRED_WORDS * sizeof(unsigned int)));
    }
    if (p->capBlocks < numBlocks) {
        if (p->classList) { (void)hipFree(p->classList); (void)hipFree(p->order); p->classList = p->order = nullptr; p->capBlocks = 0; }
        NTR_HIP(hipMalloc((void**)&p->classList, (size_t)NTR_SCHED_PRED_CLASSES * numBlocks * sizeof(unsigned int)));
        NTR_HIP(hipMalloc((void**)&p->order, (size_t)numBlocks * sizeof(unsigned int)));
        p->capBlocks = numBlocks;
    }
    return NTR_OK;
}

static void scratch_free(PredictScratch* p)
{
    if (p->classCount) (void)hipFree(p->classCount);
    if (p->classList) (void)hipFree(p->classList);
    if (p->order) (void)hipFree(p->order);
    *p = PredictScratch();
}

// spares of at least numBlocks (the state's mutex held)
static int scratch_count_spares(DeviceState* ds, int numBlocks)
{
    int n = 0;
    for (auto& e : ds->scratch)
        if (e.state == PredictScratch::SPARE && e.capBlocks >= numBlocks) n++;
    return n;
}

// makes sure `want` spares of at least numBlocks exist (the state's mutex held, not capturing): smaller spares are regrown
// first (nothing references a spare), then free slots are taken; running out of slots is not an error here
static int scratch_provision_spares(DeviceState* ds, int numBlocks, int want)
{
    int have = scratch_count_spares(ds, numBlocks);
    for (auto& e : ds->scratch) {
        if (have >= want) break;
        if (e.state == PredictScratch::SPARE && e.capBlocks < numBlocks) {
            const int rc = scratch_alloc(&e, numBlocks);
            if (rc != NTR_OK) return rc;
            have++;
        }
    }
    for (auto& e : ds->scratch) {
        if (have >= want) break;
        if (e.state != PredictScratch::FREE) continue;
        const int rc = scratch_alloc(&e, numBlocks);
        if (rc != NTR_OK) return rc;
        e.state = PredictScratch::SPARE;
        have++;
    }
    return NTR_OK;
}

int predict_scratch_get(DeviceState* ds, hipStream_t s, int numBlocks, PredictScratch** out)
{
    std::lock_guard<std::mutex> lk(ds->mu);
    const bool capturing = stream_is_capturing(s);
    if (capturing) {   // a private entry from the spares: the smallest that fits
        PredictScratch* best = nullptr;
        for (auto& e : ds->scratch)
            if (e.state == PredictScratch::SPARE && e.capBlocks >= numBlocks && (!best || e.capBlocks < best->capBlocks)) best = &e;
        // no spare of this size: the launch is captured without a predicted order (an optimisation, not a contract);
        // ntr_trace_graph_reserve provisions spares for graphs that want it
        if (!best) { *out = nullptr; return NTR_OK; }
        best->state = PredictScratch::PINNED;
        best->lastUse = ++ds->clock;
        *out = best;
        return NTR_OK;
    }
    PredictScratch* p = nullptr;
    PredictScratch* lru = nullptr;
    PredictScratch* empty = nullptr;
    int live = 0;
    for (auto& e : ds->scratch) {
        if (e.state == PredictScratch::LIVE) {
            live++;
            if (e.stream == (void*)s) { p = &e; break; }
            if (!lru || e.lastUse < lru->lastUse) lru = &e;
        } else if (e.state == PredictScratch::FREE && !empty) {
            empty = &e;
        }
    }
    if (!p) {
        p = (empty && live < kScratchLive) ? empty : (lru ? lru : empty);
        if (!p) return set_error(NTR_ERR_NOMEM, "ntr_trace_bvh: every prediction scratch is held by a captured HIP graph (ntr_trace_graph_release_all)");
        if (p->state == PredictScratch::LIVE) {
            NTR_HIP(hipDeviceSynchronize());  // the evicted stream's launches may still read it
            scratch_free(p);
        }
    } else if (p->capBlocks < numBlocks && p->classList) {
        NTR_HIP(hipStreamSynchronize(s));
    }
    int rc = scratch_alloc(p, numBlocks);
    if (rc != NTR_OK) return rc;
    p->state = PredictScratch::LIVE;
    p->stream = (void*)s;
    p->lastUse = ++ds->clock;
    rc = scratch_provision_spares(ds, numBlocks, kScratchSpares);
    if (rc != NTR_OK) return rc;
    *out = p;
    return NTR_OK;
}

static void sched_hint_release(NtrSchedHint* h)
{
    if (h->order) (void)hipFree(h->order);
    if (h->cost) (void)hipFree(h->cost);
    h->order = h->cost = nullptr;
    h->numBlocks = 0; h->capBlocks = 0; h->uses = 0; h->valid = false; h->predicted = false;
}

// Binds a caller-owned hint to a batch of numBlocks blocks on `dev`: the arrays are reallocated only to grow (or on another device); a
// hint bound to a different block count starts over, its order the identity (in the order of `s`): a refresh launch that records no
// cost leaves the order as it is (sched_order_kernel), so it must be a permutation of the blocks from the start.
int sched_hint_bind(NtrSchedHint* h, int numBlocks, int dev, hipStream_t s)
{
    if (h->device != dev || h->capBlocks < numBlocks || !h->order) {
        sched_hint_release(h);
        // order[numBlocks .. numBlocks + 2]: the batch's coherence words, the last one its mini-pool K (0 = not estimated yet, read as 1):
        // written by the dispatch-order prediction of the batch's first launch, or by the coherence probe of its refresh launches
        NTR_HIP(hipMalloc((void**)&h->order, ((size_t)numBlocks + 3) * sizeof(unsigned int)));
        NTR_HIP(hipMalloc((void**)&h->cost, (size_t)numBlocks * sizeof(unsigned int)));
        h->capBlocks = numBlocks;
        h->device = dev;
    }
    if (h->numBlocks != numBlocks) {
        h->numBlocks = numBlocks;
        h->uses = 0; h->valid = false; h->predicted = false;
        const hipError_t e = ntr_launch_identity_order(h->order, numBlocks, s);
        if (e != hipSuccess) return hip_fail(e, "identity_order launch");
    }
    return NTR_OK;
}

// returns an automatic hint's arrays in stream order: behind every launch of `s` that reads them (no synchronisation, no event)
static void auto_hint_release_async(NtrSchedHint* h, hipStream_t s)
{
    if (h->order) (void)hipFreeAsync(h->order, s);
    if (h->cost) (void)hipFreeAsync(h->cost, s);
    h->order = h->cost = nullptr;
    h->numBlocks = 0; h->uses = 0; h->valid = false; h->predicted = false;
}

// The hint of this batch, or null: the first launch of a key only registers it (no allocation, no hint); from the second on the key owns a
// hint.  Nothing here synchronises, records an event or frees under a launch in flight: an entry is recycled only if it holds no storage
// or belongs to THIS stream (its arrays are then freed in stream order, behind the launches that read them), and if no entry can be had
// the launch simply goes without (buffer / predicted order).
// The table logic alone (no HIP call: ntr_selftest_auto_hint_table drives it on the CPU tier).  Returns the entry of the key on a repeated
// sighting; on a first sighting registers the key and returns null, *evicted then being an entry whose arrays the caller must return in
// the order of `stream` (or null).  *noEntry: the table had no entry this launch may take.
static AutoHint* auto_hint_lookup(DeviceState* ds, const void* d_rays, const void* d_nodes, int numRays, int anyHit, void* stream,
                                  NtrSchedHint** evicted, bool* noEntry)
{
    *evicted = nullptr;
    *noEntry = false;
    AutoHint* hit = nullptr;
    AutoHint* freeE = nullptr;
    for (auto& e : ds->autoHints) {
        if (e.used && e.rays == d_rays && e.nodes == d_nodes && e.numRays == numRays && e.anyHit == anyHit && e.stream == stream) { hit = &e; break; }
        if (!e.used && !freeE) freeE = &e;
    }
    if (hit) {
        hit->lastUse = ++ds->clock;
        hit->sightings++;
        return hit;
    }
    AutoHint* v = freeE;
    if (!v) {   // least recently used among the entries this launch may recycle: those without storage, and this stream's own
        for (auto& e : ds->autoHints) {
            if (e.hint.order && e.stream != stream) continue;
            if (!v || e.lastUse < v->lastUse) v = &e;
        }
        if (!v) { *noEntry = true; return nullptr; }
        if (v->hint.order) *evicted = &v->hint;
    }
    v->rays = d_rays; v->nodes = d_nodes; v->numRays = numRays; v->anyHit = anyHit; v->stream = stream;
    v->used = true;
    v->sightings = 1;
    v->lastUse = ++ds->clock;
    v->hint.uses = 0; v->hint.valid = false;
    return nullptr;   // first sighting: registered, not hinted
}

int auto_hint_get(DeviceState* ds, const void* d_rays, const void* d_nodes, int numRays, int anyHit, hipStream_t s, int numBlocks,
                  NtrSchedHint** out)
{
    *out = nullptr;
    const int dev = ds->device;
    std::lock_guard<std::mutex> lk(ds->mu);
    NtrSchedHint* evicted = nullptr;
    bool noEntry = false;
    AutoHint* hit = auto_hint_lookup(ds, d_rays, d_nodes, numRays, anyHit, (void*)s, &evicted, &noEntry);
    if (evicted) auto_hint_release_async(evicted, s);
    if (!hit) return NTR_OK;
    NtrSchedHint* h = &hit->hint;
    if (h->numBlocks != numBlocks || h->device != dev) {   // second sighting: the storage
        if (h->order) auto_hint_release_async(h, s);
        unsigned int* order = nullptr;
        unsigned int* cost = nullptr;
        // (failing here -- another thread capturing in global mode, memory -- only means: no hint for this launch)
        if (hipMallocAsync((void**)&order, ((size_t)numBlocks + 3) * sizeof(unsigned int), s) != hipSuccess) { (void)hipGetLastError(); return NTR_OK; }
        if (hipMallocAsync((void**)&cost, (size_t)numBlocks * sizeof(unsigned int), s) != hipSuccess) { (void)hipGetLastError(); (void)hipFreeAsync(order, s); return NTR_OK; }
        h->order = order; h->cost = cost;
        h->numBlocks = numBlocks;
        h->device = dev;
        h->uses = 0; h->valid = false;
        if (ntr_launch_identity_order(order, numBlocks, s) != hipSuccess) {   // (see sched_hint_bind)
            (void)hipGetLastError();
            auto_hint_release_async(h, s);
            return NTR_OK;
        }
    }
    *out = h;
    return NTR_OK;
}

}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_top_table_refresh(const void* d_nodes, int64_t nodesBytes, void* stream)
{
    DeviceState* ds = nullptr;
    const int rc = current_device_state(&ds, "hipGetDevice(&dev)");
    if (rc != NTR_OK) return rc;
    TopTable* t = nullptr;
    return top_table_get(ds, d_nodes, nodesBytes, (hipStream_t)stream, true, &t);
}

int ntr_trace_graph_reserve(int32_t launches, int32_t numRays)
{
    if (launches < 0 || numRays < 0) return set_error(NTR_ERR_INVALID, "ntr_trace_graph_reserve: negative argument");
    DeviceState* ds = nullptr;
    int rc = current_device_state_ready(&ds);
    if (rc != NTR_OK) return rc;
    const int numBlocks = (numRays + 255) / 256;
    std::lock_guard<std::mutex> lk(ds->mu);
    if (numBlocks > 0 && launches > 0) {
        rc = scratch_provision_spares(ds, numBlocks, launches);
        if (rc != NTR_OK) return rc;
        if (scratch_count_spares(ds, numBlocks) < launches)
            return set_error(NTR_ERR_NOMEM, "ntr_trace_graph_reserve: at most %d prediction scratches exist (ntr_trace_graph_release_all returns the pinned ones)", kScratch);
    }
    return NTR_OK;
}

int ntr_trace_graph_release_all(void)
{
    DeviceState* ds = nullptr;
    const int rc = current_device_state(&ds, "hipGetDevice(&dev)");
    if (rc != NTR_OK) return rc;
    NTR_HIP(hipDeviceSynchronize());   // replays in flight still read the scratch
    std::lock_guard<std::mutex> lk(ds->mu);
    for (auto& e : ds->scratch)
        if (e.state == PredictScratch::PINNED) e.state = PredictScratch::SPARE;   // back to the spares
    for (auto& t : ds->top) t.pinned = false;
    ds->nextPinned = 0;
    return NTR_OK;
}

int ntr_stream_release(void* stream)
{
    // The library keeps per-stream scheduling state on the current device -- automatic hints (their arrays come from the stream-ordered
    // allocator) and the stream's prediction scratch -- and recycles an entry only for the stream that owns it (nothing on the launch path
    // synchronises).  A host that destroys a stream returns that state here first; otherwise entries of dead streams stay allocated for
    // the life of the process, and a table full of them (96 hints per device) leaves later streams without the learned dispatch order.
    DeviceState* ds = nullptr;
    const int rc = current_device_state(&ds, "hipGetDevice(&dev)");
    if (rc != NTR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "ntr_stream_release: the stream is being captured");
    NTR_HIP(hipStreamSynchronize(s));   // launches in flight still read the arrays
    std::lock_guard<std::mutex> lk(ds->mu);
    for (auto& e : ds->autoHints)
        if (e.used && e.stream == stream) {
            if (e.hint.order) auto_hint_release_async(&e.hint, s);
            e = AutoHint();
        }
    for (auto& e : ds->scratch)
        if (e.state == PredictScratch::LIVE && e.stream == stream) scratch_free(&e);
    return NTR_OK;
}

int ntr_selftest_auto_hint_table(int32_t devices, int32_t keysPerDevice, int32_t rounds, int32_t* hintedLastRound)
{
    // CPU-side check of the automatic-hint table logic (no device needed): `devices` fake devices, each tracing `keysPerDevice` distinct
    // batches on one stream of its own, `rounds` times over; hintedLastRound[d] = batches of device d that found their entry in the last
    // round.  With per-device tables every device is served alike (keysPerDevice each while keysPerDevice <= 96).
    if (devices < 1 || devices > kMaxDevices || keysPerDevice < 1 || rounds < 1 || !hintedLastRound)
        return set_error(NTR_ERR_INVALID, "ntr_selftest_auto_hint_table: bad argument");
    for (int d = 0; d < devices; d++) hintedLastRound[d] = 0;
    DeviceState* fake = new (std::nothrow) DeviceState[devices];   // (never touches g_state: the live tables stay as they are)
    if (!fake) return set_error(NTR_ERR_NOMEM, "ntr_selftest_auto_hint_table: out of host memory");
    for (int r = 0; r < rounds; r++)
        for (int k = 0; k < keysPerDevice; k++)        // batch by batch across the devices, as eight host threads would interleave
            for (int d = 0; d < devices; d++) {
                NtrSchedHint* evicted = nullptr;
                bool noEntry = false;
                std::lock_guard<std::mutex> lk(fake[d].mu);
                AutoHint* hit = auto_hint_lookup(&fake[d], (const void*)(uintptr_t)(0x1000 + 64 * k), (const void*)(uintptr_t)0x10, 1 << 20, k & 1,
                                                 (void*)(uintptr_t)(d + 1), &evicted, &noEntry);
                if (hit) hit->hint.order = (unsigned int*)(uintptr_t)1;   // stands for "storage allocated" (a later eviction must not take it from another stream)
                if (hit && r == rounds - 1) hintedLastRound[d]++;
            }
    delete[] fake;
    return NTR_OK;
}

int ntr_sched_hint_create(NtrSchedHint** out)
{
    if (!out) return set_error(NTR_ERR_INVALID, "ntr_sched_hint_create: null out");
    *out = new (std::nothrow) NtrSchedHint();
    return *out ? NTR_OK : set_error(NTR_ERR_NOMEM, "ntr_sched_hint_create: out of memory");
}

int ntr_sched_hint_destroy(NtrSchedHint* hint)
{
    if (!hint) return NTR_OK;
    sched_hint_release(hint);
    delete hint;
    return NTR_OK;
}

int ntr_sched_hint_reset(NtrSchedHint* hint)
{
    if (!hint) return set_error(NTR_ERR_INVALID, "ntr_sched_hint_reset: null hint");
    hint->uses = 0;
    hint->valid = false;
    hint->predicted = false;
    return NTR_OK;
}

int ntr_sched_hint_inspect(const NtrSchedHint* hint, NtrSchedHintState* state, uint32_t* h_order, uint32_t* h_cost, void* stream)
{
    if (!hint || !state) return set_error(NTR_ERR_INVALID, "ntr_sched_hint_inspect: null argument");
    if (hint->numBlocks == 0 && (h_order || h_cost)) return set_error(NTR_ERR_INVALID, "ntr_sched_hint_inspect: the hint is not bound (it has no arrays)");
    hipStream_t s = (hipStream_t)stream;
    if (hint->numBlocks > 0) {
        NTR_HIP(hipStreamSynchronize(s));
        if (h_order) NTR_HIP(hipMemcpyAsync(h_order, hint->order, ((size_t)hint->numBlocks + 3) * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        if (h_cost) NTR_HIP(hipMemcpyAsync(h_cost, hint->cost, (size_t)hint->numBlocks * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        if (h_order || h_cost) NTR_HIP(hipStreamSynchronize(s));
    }
    state->numBlocks = hint->numBlocks;
    state->device = hint->device;
    state->uses = hint->uses;
    state->valid = hint->valid ? 1 : 0;
    state->predicted = hint->predicted ? 1 : 0;
    return NTR_OK;
}

int ntr_sched_hint_predict(NtrSchedHint* hint, const uint32_t* d_blockCost, int32_t numBlocks, void* stream)
{
    if (!hint || !d_blockCost || numBlocks < 1) return set_error(NTR_ERR_INVALID, "ntr_sched_hint_predict: bad argument");
    hipStream_t s = (hipStream_t)stream;
    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    if (hint->numBlocks != numBlocks || hint->device != dev) {   // (the binding ntr_trace_bvh_hinted would make on first use)
        const int rc = sched_hint_bind(hint, numBlocks, dev, s);
        if (rc != NTR_OK) return rc;
    }
    NTR_HIP(hipMemcpyAsync(hint->cost, d_blockCost, (size_t)numBlocks * sizeof(unsigned int), hipMemcpyDeviceToDevice, s));
    hipError_t le = ntr_launch_sched_order(hint->cost, numBlocks, tunables().schedClasses, hint->order, 0, s);
    if (le == hipSuccess) le = ntr_launch_zero_words(hint->order + numBlocks, 3, s);   // the batch's coherence words / pool K: not estimated yet
    if (le != hipSuccess) return hip_fail(le, "sched_order launch");
    hint->uses = 0;      // the next launch starts the hint's life: it runs this order; the launches after it measure and refine
    hint->valid = true;
    hint->predicted = true;
    return NTR_OK;
}

}  // extern "C"
