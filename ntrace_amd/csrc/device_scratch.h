// device_scratch.h -- a grow-only scratch allocation per device, kept between calls (the LBVH builder's workspace, the ray sort's
// temporaries): a rebuild or a sort per frame must not pay hipMalloc / hipFree pairs, each of which synchronises the device.
// One caller per device at a time, as everywhere in the C-ABI; host threads driving different devices never touch each other's memory.
// A pool is only regrown after the device has drained, so work still in flight on another stream keeps its memory.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "ntr_internal.h"

namespace ntr {

class DeviceScratchPool {
public:
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
        const hipError_t e = hipMalloc(&np, bytes);
        if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {
            (void)hipGetLastError();
            return set_error(NTR_ERR_NOMEM, "scratch of %zu B: out of device memory", bytes);
        }
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (scratch)");
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
    static constexpr int kMaxDevices = 64;
    struct Slot { void* p = nullptr; size_t bytes = 0; };
    Slot slots_[kMaxDevices];
    std::mutex mu_;
};

}  // namespace ntr
