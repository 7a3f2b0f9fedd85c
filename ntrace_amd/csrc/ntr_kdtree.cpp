// ntr_kdtree.cpp -- C-ABI of the kd-tree path (declared in include/ntrace_amd.h): host build (KDTree + CudaKDTree of the host
// mirror), wrapping of buffers made elsewhere, and the trace_kdtree launch of CudaKDTreeTracer::traceBatch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "CudaKDTree.hpp"
#include "device_scratch.h"
#include "kdtree_kernels.h"
#include "ntr_internal.h"
#include "sched_state.h"
#include "trace_kernels.h"

using namespace FW;

struct NtrHostKdtree {
    Scene*        scene;
    CudaKDTree*   ckd;
    KDTree::Stats stats;
};

namespace {

// The walk of ntr_host_kdtree_wrap: every entry reachable from node 0 checked, counted into `st`.
int validate_kdtree(const int32_t* nodes, int64_t numNodes, const int32_t* triIndex, int64_t numIndex, int64_t numWoopTris,
                    KDTree::Stats& st)
{
    st.clear();
    std::vector<uint8_t> seen((size_t)numNodes, 0);
    struct Item { int64_t node; int depth; };
    std::vector<Item> stack(1, Item{0, 1});
    seen[0] = 1;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const int32_t* n = nodes + it.node * 4;
        if (((uint32_t)n[3] >> 28) > 2u)
            return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: node %lld has axis %u", (long long)it.node, (uint32_t)n[3] >> 28);
        if (it.depth > NTR_KDTREE_STACK_DEPTH)
            return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: depth above %d (the trace kernel's stack)", NTR_KDTREE_STACK_DEPTH);
        st.numInnerNodes++;
        if (it.depth > st.maxDepth) st.maxDepth = it.depth;
        for (int c = 0; c < 2; c++) {
            const int32_t ch = n[c];
            if (ch >= 0) {
                if (ch >= numNodes)
                    return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: child %d of node %lld out of range", (int)ch, (long long)it.node);
                if (seen[(size_t)ch])
                    return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: node %d is reached twice (cycle or shared subtree)", (int)ch);
                seen[(size_t)ch] = 1;
                stack.push_back(Item{ch, it.depth + 1});
                continue;
            }
            st.numLeafNodes++;
            if (ch == NTR_KDTREE_EMPTYLEAF) { st.numEmptyLeaves++; continue; }
            if (((uint32_t)ch & 0xF0000000u) == 0x80000000u)   // the kernel reads any such child as an empty leaf
                return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: leaf child 0x%08x of node %lld", (uint32_t)ch, (long long)it.node);
            int64_t k = (int64_t)~ch;
            for (;; k++) {
                if (k >= numIndex)
                    return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: leaf list at %d has no terminator", (int)~ch);
                if (triIndex[k] == NTR_KDTREE_EMPTYLEAF) break;
                if (triIndex[k] < 0 || triIndex[k] >= numWoopTris)
                    return ntr::set_error(NTR_ERR_LAYOUT, "ntr_host_kdtree_wrap: triangle id %d at %lld out of range", (int)triIndex[k], (long long)k);
                st.numTris++;
            }
            if (k == (int64_t)~ch) st.numEmptyLeaves++;
        }
    }
    return NTR_OK;
}

template <class F>
int guarded(const char* fn, F&& f)
{
    try {
        return f();
    } catch (const FatalError& e) {
        return ntr::set_error(NTR_ERR_INVALID, "%s", e.message.c_str());
    } catch (const std::bad_alloc&) {
        return ntr::set_error(NTR_ERR_NOMEM, "%s: out of host memory", fn);
    } catch (const std::exception& e) {   // nothing may escape the extern "C" boundary
        return ntr::set_error(NTR_ERR_INVALID, "%s: %s", fn, e.what());
    } catch (...) {
        return ntr::set_error(NTR_ERR_INVALID, "%s: unknown exception", fn);
    }
}

}  // namespace

extern "C" {

int ntr_kdtree_build(int32_t builder, int32_t numTris, const int32_t* triVtxIndex, int32_t numVerts, const float* vtxPos,
                     int32_t maxLeafSize, NtrHostKdtree** out)
{
    if (!out) return ntr::set_error(NTR_ERR_INVALID, "ntr_kdtree_build: null out");
    *out = nullptr;
    if (builder != NTR_KDTREE_SPATIAL_MEDIAN && builder != NTR_KDTREE_SAH)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_kdtree_build: unknown builder %d", (int)builder);
    if (numTris <= 0 || numVerts < 0 || !triVtxIndex || (numVerts && !vtxPos))
        return ntr::set_error(NTR_ERR_INVALID, "ntr_kdtree_build: bad geometry arguments (a kd-tree needs at least one triangle)");
    if (builder == NTR_KDTREE_SPATIAL_MEDIAN && maxLeafSize < 1)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_kdtree_build: maxLeafSize < 1");
    for (int64_t i = 0; i < (int64_t)numTris * 3; i++)
        if (triVtxIndex[i] < 0 || triVtxIndex[i] >= numVerts)
            return ntr::set_error(NTR_ERR_INVALID, "ntr_kdtree_build: vertex index out of range at triangle %lld", (long long)(i / 3));
    return guarded(__func__, [&]() {
        NtrHostKdtree* h = new NtrHostKdtree();
        h->scene = new Scene(numTris, (const Vec3i*)triVtxIndex, numVerts, (const Vec3f*)vtxPos);
        h->ckd = nullptr;
        Platform platform("GPU");  // Renderer.cpp:88-89
        platform.setLeafPreferences(1, builder == NTR_KDTREE_SPATIAL_MEDIAN ? maxLeafSize : 1);
        KDTree::BuildParams params;
        params.stats = &h->stats;
        params.builder = builder == NTR_KDTREE_SAH ? "SAHKDTree" : "SpatialMedianKDTree";
        try {
            KDTree kdtree(h->scene, platform, params);
            h->ckd = new CudaKDTree(kdtree);
            if (kdtree.getRoot()->isLeaf()) {   // the emitted tree: one inner node over the leaf and an empty leaf (CudaKDTree.hpp)
                h->stats.numInnerNodes = 1;
                h->stats.numLeafNodes = 2;
                h->stats.numChildNodes = 2;
                h->stats.numEmptyLeaves += 1;
                h->stats.maxDepth = 1;
            }
        } catch (...) {
            delete h->ckd;
            delete h->scene;
            delete h;
            throw;
        }
        *out = h;
        return (int)NTR_OK;
    });
}

int ntr_host_kdtree_info(const NtrHostKdtree* kd, NtrHostKdtreeInfo* info)
{
    if (!kd || !info) return ntr::set_error(NTR_ERR_INVALID, "ntr_host_kdtree_info: null argument");
    memset(info, 0, sizeof(*info));
    CudaKDTree* c = kd->ckd;
    info->nodes = c->getNodeBuffer().getPtr();
    info->nodesBytes = c->getNodeBuffer().getSize();
    info->triWoop = c->getTriWoopBuffer().getPtr();
    info->triWoopBytes = c->getTriWoopBuffer().getSize();
    info->triIndex = (const int32_t*)c->getTriIndexBuffer().getPtr();
    info->triIndexBytes = c->getTriIndexBuffer().getSize();
    for (int k = 0; k < 3; k++) {
        info->sceneMin[k] = c->getBBox().min()[k];
        info->sceneMax[k] = c->getBBox().max()[k];
    }
    info->delta = c->getDelta();
    info->numInnerNodes = kd->stats.numInnerNodes;
    info->numLeafNodes = kd->stats.numLeafNodes;
    info->numEmptyLeaves = kd->stats.numEmptyLeaves;
    info->numTriRefs = kd->stats.numTris;
    info->maxDepth = kd->stats.maxDepth;
    info->percentDuplicates = kd->stats.percentDuplicates;
    info->buildSeconds = kd->stats.buildTime;
    return NTR_OK;
}

void ntr_host_kdtree_free(NtrHostKdtree* kd)
{
    if (!kd) return;
    delete kd->ckd;
    delete kd->scene;
    delete kd;
}

int ntr_host_kdtree_wrap(const void* nodes, int64_t nodesBytes, const void* triWoop, int64_t triWoopBytes, const int32_t* triIndex,
                         int64_t triIndexBytes, const float sceneMin[3], const float sceneMax[3], NtrHostKdtree** out)
{
    if (!out) return ntr::set_error(NTR_ERR_INVALID, "ntr_host_kdtree_wrap: null out");
    *out = nullptr;
    if (!nodes || !triWoop || !triIndex || !sceneMin || !sceneMax)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_host_kdtree_wrap: null argument");
    if (nodesBytes < 16 || (nodesBytes % 16) != 0 || nodesBytes / 16 > 0x7FFFFFFFll || triWoopBytes < 48 || (triWoopBytes % 16) != 0 ||
        triWoopBytes / 48 > 0xFFFFFFFFll || triIndexBytes < 4 || (triIndexBytes % 4) != 0 || triIndexBytes / 4 > 0xFFFFFFFFll)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_host_kdtree_wrap: bad buffer sizes");
    return guarded(__func__, [&]() {
        KDTree::Stats st;
        const int rc = validate_kdtree((const int32_t*)nodes, nodesBytes / 16, triIndex, triIndexBytes / 4, triWoopBytes / 48, st);
        if (rc != NTR_OK) return rc;
        NtrHostKdtree* h = new NtrHostKdtree();
        h->scene = nullptr;
        h->stats = st;
        h->ckd = new CudaKDTree();
        h->ckd->getNodeBuffer().set(nodes, nodesBytes);
        h->ckd->getTriWoopBuffer().set(triWoop, triWoopBytes);
        h->ckd->getTriIndexBuffer().set(triIndex, triIndexBytes);
        h->ckd->setBBox(AABB(Vec3f(sceneMin[0], sceneMin[1], sceneMin[2]), Vec3f(sceneMax[0], sceneMax[1], sceneMax[2])));
        *out = h;
        return (int)NTR_OK;
    });
}

int ntr_trace_kdtree(int32_t numRays, int32_t anyHit, const float sceneMin[3], const float sceneMax[3], const NtrRay* d_rays,
                     NtrRayResult* d_results, const void* d_nodes, int64_t nodesBytes, const void* d_triWoop, int64_t triWoopBytes,
                     const int32_t* d_triIndex, int64_t triIndexBytes, void* stream, float* seconds)
{
    (void)anyHit;  // the reference's kernel ignores it (fermi_kdtree_while_while_leafRef.cu)
    if (seconds) *seconds = 0.0f;
    if (numRays < 0) return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: numRays < 0");
    if (numRays == 0) return NTR_OK;  // CudaKDTreeTracer.cpp:73-75
    if (!d_nodes || !d_triWoop || !d_triIndex) return ntr::set_error(NTR_ERR_INVALID, "CudaKDTreeTracer: No kd-tree!");
    if (!sceneMin || !sceneMax) return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: null scene box");
    if (!d_rays || !d_results) return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: null ray/result buffer");
    if (nodesBytes < 16 || (nodesBytes % 16) != 0 || nodesBytes / 16 > 0x7FFFFFFFll)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: node buffer size must be a positive multiple of 16 below 32 GiB");
    if (triWoopBytes < 48 || (triWoopBytes % 16) != 0 || triWoopBytes / 48 > 0xFFFFFFFFll)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: triWoop buffer size must be a multiple of 16, at least 48");
    if (triIndexBytes < 4 || (triIndexBytes % 4) != 0 || triIndexBytes / 4 > 0xFFFFFFFFll)
        return ntr::set_error(NTR_ERR_INVALID, "ntr_trace_kdtree: triIndex buffer size must be a positive multiple of 4");

    ntr::KdTraceParams p;
    p.numRays = numRays;
    p.rays = d_rays;
    p.results = d_results;
    p.nodes = (const int4*)d_nodes;
    p.numNodes = (uint32_t)(nodesBytes / 16);
    p.woop = (const float4*)d_triWoop;
    p.numWoopTris = (uint32_t)(triWoopBytes / 48);
    p.triIndex = d_triIndex;
    p.numTriIndex = (uint32_t)(triIndexBytes / 4);
    for (int k = 0; k < 3; k++) { p.bmin[k] = sceneMin[k]; p.bmax[k] = sceneMax[k]; }
    // CudaKDTreeTracer.cpp:97: (bbox.max + bbox.min).length() * 0.000001f
    const float sx = sceneMax[0] + sceneMin[0], sy = sceneMax[1] + sceneMin[1], sz = sceneMax[2] + sceneMin[2];
    p.delta = ::sqrtf(sx * sx + sy * sy + sz * sz) * 0.000001f;
    ntr::DeviceState* ds = nullptr;   // the sticky status word ntr_trace_status reads
    int rc = ntr::current_device_state_ready(&ds);
    if (rc != NTR_OK) return rc;
    p.status = ds->status;

    hipStream_t s = (hipStream_t)stream;
    ntr::StreamEvents<2> ev(s);
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(ev.record(0));
    }
    const hipError_t le = ntr_launch_trace_kdtree(&p, s);
    if (le != hipSuccess) return ntr::hip_fail(le, "trace_kdtree launch");
    if (seconds) {
        float ms = 0.0f;
        NTR_HIP(ev.record(1));
        NTR_HIP(ev.elapsed(0, 1, &ms));
        *seconds = ms * 1e-3f;
        unsigned int st = 0;
        rc = ntr::status_fetch(ds, s, &st);
        if (rc != NTR_OK) return rc;
        if (st & NTR_STATUS_STACK_OVERFLOW) return ntr::set_error(NTR_ERR_OVERFLOW, "trace_kdtree: traversal stack overflow");
        if (st & NTR_STATUS_KDTREE_RANGE) return ntr::set_error(NTR_ERR_LAYOUT, "trace_kdtree: an index outside its buffer");
    }
    return NTR_OK;
}

}  // extern "C"
