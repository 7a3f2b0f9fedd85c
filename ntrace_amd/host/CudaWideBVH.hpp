// CudaWideBVH.hpp -- a 4-wide tree over a CudaBVH: the node buffer ntr_bvh_widen writes (include/ntrace_amd.h, csrc/wide_bvh.h,
// DESIGN.md 6l; the rule is tests/np_bvh_wide.py) and the trace ntr_trace_wide.  An extension without a reference class.
//   CudaWideBVH(bvh)  no device work; owns the wide node buffer, shares the CudaBVH's Woop and index buffers (the CudaBVH must
//                     outlive this object and keep its buffers)
//   build             widens the Compact tree on the device; refuses (FW::fail) without a device: there is no CPU fallback
//   traceBatch        closest hit or any hit as the RayBuffer asks, with the binary tree's validated flags
// This class does not refit or optimize its wide tree: refit or optimize the CudaBVH, then build() again (at the C ABI a one-entry
// ntr_pool_wide_refit refits a single-level wide tree in place).
#pragma once
#include "CudaBVH.hpp"
#include "RayBuffer.hpp"

namespace FW {

class CudaWideBVH {
public:
    explicit CudaWideBVH(CudaBVH& bvh);
    ~CudaWideBVH(void) {}

    void build(void);                                                            // again after the CudaBVH was refitted or optimized
    bool isBuilt(void) const { return m_result.nodesBytes != 0; }
    F32  traceBatch(RayBuffer& rays);                                            // GPU seconds

    CudaBVH& getBVH(void) { return m_bvh; }
    Buffer&  getWideNodeBuffer(void) { return m_wideNodes; }
    Buffer&  getTriWoopBuffer(void) { return m_bvh.getTriWoopBuffer(); }         // the CudaBVH's own
    Buffer&  getTriIndexBuffer(void) { return m_bvh.getTriIndexBuffer(); }
    const NtrBvhWideResult& getWidenResult(void) const { return m_result; }

private:
    CudaWideBVH(const CudaWideBVH&);
    CudaWideBVH& operator=(const CudaWideBVH&);

    CudaBVH&         m_bvh;
    Buffer           m_wideNodes;
    NtrBvhWideResult m_result;
};

}  // namespace FW
