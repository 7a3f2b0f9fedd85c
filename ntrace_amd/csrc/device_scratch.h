// device_scratch.h -- the host toolkit of the device builders and the timed entry points:
//   DeviceScratchPool  a grow-only scratch allocation per device, kept between calls (the builders' workspaces, the ray sort's
//                      temporaries): a rebuild or a sort per frame must not pay hipMalloc / hipFree pairs, each of which synchronises
//                      the device.  Every pool registers itself; ntr_lbvh_release_workspace returns them all (release_all).
//   ScratchCarver      256-byte aligned slices of one scratch block
//   StreamEvents<N>    N events recorded on one stream, destroyed on every return path
//   device_malloc      hipMalloc with out-of-memory reported as NTR_ERR_NOMEM
// One caller per device at a time, as everywhere in the C-ABI; host threads driving different devices never touch each other's memory.
// A pool is only regrown after the device has drained, so work still in flight on another stream keeps its memory.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "ntr_internal.h"

namespace ntr {

// hipMalloc of `bytes` (at least one, so that success always means a pointer); out of memory is NTR_ERR_NOMEM, any other failure
// NTR_ERR_HIP.  `what` names the allocation in the error message.
inline int device_malloc(void** p, size_t bytes, const char* what)
{
    const hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
        (void)hipGetLastError();
        return set_error(NTR_ERR_NOMEM, "%s: out of device memory (%zu B)", what, bytes);
    }
    if (e != hipSuccess) return hip_fail(e, what);
    return NTR_OK;
}

struct ScratchCarver {   // off: the bytes taken so far, the block size to reserve
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
};

// Marks on a stream read back after ONE synchronisation, so a timed build has no host round trips inside it.  The timed launches check
// every event call (create, record, elapsed); the builders' phase marks are best effort (mark, ms): a failed event call reads as 0 ms
// and does not fail the build.
template <int N>
class StreamEvents {
public:
    explicit StreamEvents(hipStream_t s) : s_(s) {}
    StreamEvents(const StreamEvents&) = delete;
    StreamEvents& operator=(const StreamEvents&) = delete;
    ~StreamEvents() { for (hipEvent_t e : ev_) if (e) (void)hipEventDestroy(e); }
    hipError_t create()
    {
        for (hipEvent_t& e : ev_) {
            const hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    hipError_t record(int i) { return hipEventRecord(ev_[i], s_); }
    hipError_t elapsed(int a, int b, float* ms)   // waits for mark b
    {
        *ms = 0.0f;
        const hipError_t e = hipEventSynchronize(ev_[b]);
        return e != hipSuccess ? e : hipEventElapsedTime(ms, ev_[a], ev_[b]);
    }
    void mark(int i) { (void)record(i); }
    float ms(int a, int b)   // marks a and b have completed
    {
        float v = 0.0f;
        return hipEventElapsedTime(&v, ev_[a], ev_[b]) == hipSuccess ? v : 0.0f;
    }

private:
    hipEvent_t ev_[N] = {};
    hipStream_t s_;
};

// A pool lives as long as the program (a namespace-scope object); it registers itself on construction.
class DeviceScratchPool {
public:
    DeviceScratchPool()
    {
        std::lock_guard<std::mutex> lk(registry_mu());
        registry().push_back(this);
    }
    ~DeviceScratchPool()
    {
        std::lock_guard<std::mutex> lk(registry_mu());
        auto& r = registry();
        r.erase(std::remove(r.begin(), r.end(), this), r.end());
    }
    DeviceScratchPool(const DeviceScratchPool&) = delete;
    DeviceScratchPool& operator=(const DeviceScratchPool&) = delete;

    // Every pool's allocation on the current device; every pool is tried, the first error is returned.
    static int release_all()
    {
        std::lock_guard<std::mutex> lk(registry_mu());
        int rc = NTR_OK;
        for (DeviceScratchPool* p : registry()) {
            const int r = p->release();
            if (rc == NTR_OK) rc = r;
        }
        return rc;
    }

    int reserve(size_t bytes, void** out)
    {
        int dev = 0;
        NTR_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
        std::lock_guard<std::mutex> lk(mu_);
        Slot& w = slots_[dev];
        if (w.p && w.bytes < bytes) {
            NTR_HIP(hipDeviceSynchronize());
            NTR_HIP(hipFree(w.p));
            w.p = nullptr; w.bytes = 0;
        }
        if (!w.p) {
            NTR_HIP(hipMalloc(&w.p, bytes));
            w.bytes = bytes;
        }
        *out = w.p;
        return NTR_OK;
    }
    // For a caller that lays several arrays out in the pool and changes that layout mid-use.  relayout == false: as reserve, but a
    // pool that has to grow keeps its old block until move(oldBlock, newBlock) has carried the caller's live data over.  relayout ==
    // true: always a fresh block of max(bytes, current size) and a move, since the live data sit at the old layout's offsets.  move
    // returns an NTR_ status and must leave the old block idle (it synchronises the stream it copied on); only that caller's stream
    // uses the pool, so the device as a whole is not drained.  Out of memory is NTR_ERR_NOMEM; on any failure the new block is freed
    // and the pool keeps the old one.
    template <class Move>
    int regrow(size_t bytes, void** out, Move&& move, bool relayout = false)
    {
        int dev = 0;
        NTR_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
        std::lock_guard<std::mutex> lk(mu_);
        Slot& w = slots_[dev];
        if (w.p && w.bytes >= bytes && !relayout) {
            *out = w.p;
            return NTR_OK;
        }
        if (w.p && w.bytes > bytes) bytes = w.bytes;
        void* np = nullptr;
        {
            const int rc = device_malloc(&np, bytes, "scratch");
            if (rc != NTR_OK) return rc;
        }
        if (w.p) {
            const int rc = move(w.p, np);
            if (rc != NTR_OK) {
                (void)hipFree(np);
                return rc;
            }
            const hipError_t fe = hipFree(w.p);
            if (fe != hipSuccess) {
                (void)hipFree(np);
                w.p = nullptr; w.bytes = 0;
                return hip_fail(fe, "hipFree (scratch)");
            }
        }
        w.p = np;
        w.bytes = bytes;
        *out = np;
        return NTR_OK;
    }
    size_t held()   // bytes held for the current device (0 if none)
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
        std::lock_guard<std::mutex> lk(mu_);
        return slots_[dev].p ? slots_[dev].bytes : 0;
    }
    int release()   // the current device's allocation (waits for the device first)
    {
        int dev = 0;
        NTR_HIP(hipGetDevice(&dev));
        if (dev < 0 || dev >= kMaxDevices) return set_error(NTR_ERR_INVALID, "device index %d out of range", dev);
        std::lock_guard<std::mutex> lk(mu_);
        Slot& w = slots_[dev];
        if (w.p) {
            NTR_HIP(hipDeviceSynchronize());
            NTR_HIP(hipFree(w.p));
            w.p = nullptr; w.bytes = 0;
        }
        return NTR_OK;
    }

private:
    static std::vector<DeviceScratchPool*>& registry() { static std::vector<DeviceScratchPool*> r; return r; }
    static std::mutex& registry_mu() { static std::mutex m; return m; }
    struct Slot { void* p = nullptr; size_t bytes = 0; };
    Slot slots_[kMaxDevices];
    std::mutex mu_;
};

}  // namespace ntr
