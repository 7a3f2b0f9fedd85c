// trace_fetch.h -- how 64 bytes reach a lane of the BVH traversal kernels (trace_kernels.hip): buffer loads through wave-uniform resource
// descriptors, the masked two-buffer fetch, and the unified-step loop's one fetch per lane and iteration (flat or through descriptors).
// A node is 64 bytes and so is a Woop triangle with the word that follows it (compact_bvh.h): one fetch serves either.
// The fetch's wave-uniform operands (UnifiedBufs) are derived from the launch's arguments: by the host, once, for the per-ray bodies
// (TraceConsts; unified_bufs<TRIM = true> copies), per wave in the persistent kernels (unified_bufs<false>, the same arithmetic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "trace_kernels.h"
#include "compact_bvh.h"

namespace ntr {

typedef __amdgpu_buffer_rsrc_t Rsrc;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned int kFetchBytes = kNodeBytes;   // what a unified step fetches: a node, or a triangle and the row after it (kTriBytes + kRowBytes)

__device__ __forceinline__ Rsrc make_rsrc(const void* p, unsigned int bytes)
{
    // built from kernel arguments only -> provably wave-uniform (no waterfall loops)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 as_f4(u32x4 v) { return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)); }
__device__ __forceinline__ u32x4 as_u4(const float4& f) { return u32x4{__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w)}; }
__device__ __forceinline__ float4 ld4(Rsrc r, int byteOfs) { return as_f4(__builtin_amdgcn_raw_buffer_load_b128(r, byteOfs, 0, 0)); }
__device__ __forceinline__ unsigned int ld1(Rsrc r, int byteOfs)
{
    return __builtin_amdgcn_raw_buffer_load_b32(r, byteOfs, 0, 0);
}

// Buffer resource descriptor as four scalar words (what make_rsrc builds): base, base_hi (stride 0), extent in bytes, flags.
__device__ __forceinline__ u32x4 rsrc_words(const void* p, unsigned int bytes)
{
    const unsigned long long a = (unsigned long long)p;
    u32x4 w;
    w.x = __builtin_amdgcn_readfirstlane((unsigned int)a);
    w.y = __builtin_amdgcn_readfirstlane((unsigned int)(a >> 32) & 0xFFFFu);
    w.z = __builtin_amdgcn_readfirstlane(bytes);
    w.w = 0x00020000u;
    return w;
}

// Lanes of maskA fetch 64 B at byte offset `ofs` of buffer A, lanes of maskB at `ofs` of buffer B (range-checked: beyond the extent
// a load returns 0 and touches no memory); the other lanes fetch nothing.  Two statements of one text: the operands a..d are write-only
// in the first and read-write in the second.
#define NTR_FETCH64_TWO_BUFFERS_TEXT                                        \
    "s_mov_b64 %[sav], exec\n\t"                                            \
    "s_and_b64 exec, %[sav], %[ma]\n\t"                                     \
    "buffer_load_dwordx4 %[a], %[ofs], %[ra], 0 offen\n\t"                  \
    "buffer_load_dwordx4 %[b], %[ofs], %[ra], 0 offen offset:16\n\t"        \
    "buffer_load_dwordx4 %[c], %[ofs], %[ra], 0 offen offset:32\n\t"        \
    "buffer_load_dwordx4 %[d], %[ofs], %[ra], 0 offen offset:48\n\t"        \
    "s_and_b64 exec, %[sav], %[mb]\n\t"                                     \
    "buffer_load_dwordx4 %[a], %[ofs], %[rb], 0 offen\n\t"                  \
    "buffer_load_dwordx4 %[b], %[ofs], %[rb], 0 offen offset:16\n\t"        \
    "buffer_load_dwordx4 %[c], %[ofs], %[rb], 0 offen offset:32\n\t"        \
    "buffer_load_dwordx4 %[d], %[ofs], %[rb], 0 offen offset:48\n\t"        \
    "s_mov_b64 exec, %[sav]\n\t"                                            \
    "s_waitcnt vmcnt(0)"
#define NTR_FETCH64_TWO_BUFFERS_INPUTS [ofs] "v"(ofs), [ra] "s"(rsrcA), [rb] "s"(rsrcB), [ma] "s"(maskA), [mb] "s"(maskB)

// ... the lanes outside both masks are left with undefined a..d
__device__ __forceinline__ void fetch64_two_buffers(u32x4 rsrcA, u32x4 rsrcB, int ofs, unsigned long long maskA,
                                                    unsigned long long maskB, float4& a, float4& b, float4& c, float4& d)
{
    u32x4 va, vb, vc, vd;
    unsigned long long sav;
    asm volatile(NTR_FETCH64_TWO_BUFFERS_TEXT
                 : [a] "=&v"(va), [b] "=&v"(vb), [c] "=&v"(vc), [d] "=&v"(vd), [sav] "=&s"(sav)
                 : NTR_FETCH64_TWO_BUFFERS_INPUTS
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd);
}

// The same loads INTO registers that already hold other lanes' data (read-write operands: lanes outside both masks keep theirs).
__device__ __forceinline__ void fetch64_two_buffers_into(u32x4 rsrcA, u32x4 rsrcB, int ofs, unsigned long long maskA,
                                                         unsigned long long maskB, float4& a, float4& b, float4& c, float4& d)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d);
    unsigned long long sav;
    asm volatile(NTR_FETCH64_TWO_BUFFERS_TEXT
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [sav] "=&s"(sav)
                 : NTR_FETCH64_TWO_BUFFERS_INPUTS
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd);
}
#undef NTR_FETCH64_TWO_BUFFERS_TEXT
#undef NTR_FETCH64_TWO_BUFFERS_INPUTS

// The two buffers of a unified fetch, as plain pointers + extents (FLAT = true: one set of four global loads for all live lanes) and as
// descriptor words (the range-checked two-buffer form: lanes whose 64 bytes would cross the end of their buffer, FLAT = false).
struct UnifiedBufs {
    const char* nodes; const char* woop;
    unsigned int nodesBytes, woopBytes;
    u32x4 rNodes, rWoop;
    bool uniformPrologue;   // per-ray kernels: scalar fetches while the wave's lanes all hold the same inner node (TraceParams::uniformPrologue)
    bool certainSteps;      // ... and their steps decided by comparisons where the slab test's outcome is certain (TraceParams::certainSteps; boxes lo <= hi)
    bool certainDescent;    // ... and the node kept a scalar from one such step to the next while every live lane takes the same child (TraceParams::certainDescent)
    // FLAT fetch: both buffers lie inside one 4 GiB window (the host checks it before it selects the flat fetch), so a lane's 64 bytes
    // are base + a 32-bit offset -- the global load takes the scalar base and the lane's offset as they are, where two unrelated 64-bit
    // pointers cost every iteration a per-lane 64-bit select and add (round 5)
    const char* base;       // the lower of the two buffers
    unsigned int dN, dW;    // nodes - base, woop - base
    unsigned int limNode;   // largest inner-node offset whose 64 bytes lie inside the node buffer (below the sentinel: `node <= limNode` implies inner)
    int limTri;             // smallest (most negative) triangle cursor ~index whose 64 bytes lie inside triWoop
    unsigned int oddBase, oddSpan;   // limNode < (unsigned)node < (unsigned)limTri, as node - oddBase < oddSpan: neither of the two (the sentinel included)
    unsigned int descentLim;         // TRIM bodies: TraceConsts::descentLim (the persistent kernels' prologue forms its own)
};
template <bool TRIM = false>   // TRIM: the bodies whose fetch asks for its end-of-buffer lanes with one range test (unified_fetch<.., TRIM>)
__device__ __forceinline__ UnifiedBufs unified_bufs(const TraceParams& p)
{
    UnifiedBufs u;
    u.nodes = (const char*)p.nodes; u.woop = (const char*)p.woop;
    u.nodesBytes = p.nodesBytes; u.woopBytes = p.woopBytes;
    if (TRIM) {   // the per-ray bodies: the host's values (TraceParams::k), copied
        const TraceConsts& k = p.k;
        u.rNodes = u32x4{k.rNodes[0], k.rNodes[1], k.rNodes[2], k.rNodes[3]}; u.rWoop = u32x4{k.rWoop[0], k.rWoop[1], k.rWoop[2], k.rWoop[3]};
        u.uniformPrologue = (k.switches & NTR_K_PROLOGUE) != 0u;
        u.certainSteps = (k.switches & NTR_K_CERTAIN) != 0u;
        u.certainDescent = k.descentLim != 0u;
        u.base = k.base; u.dN = k.dN; u.dW = k.dW; u.limNode = k.limNode; u.limTri = k.limTri;
        u.oddBase = k.oddBase; u.oddSpan = k.oddSpan; u.descentLim = k.descentLim;
        return u;
    }
    u.rNodes = rsrc_words(p.nodes, p.nodesBytes); u.rWoop = rsrc_words(p.woop, p.woopBytes);
    u.uniformPrologue = p.uniformPrologue != 0;
    u.certainSteps = p.certainSteps != 0 && (p.bvhFlags & NTR_BVH_ORDERED) != 0;
    u.certainDescent = p.certainDescent != 0;
    const unsigned long long an = (unsigned long long)p.nodes, aw = (unsigned long long)p.woop;
    const unsigned long long lo = an < aw ? an : aw;
    u.base = (const char*)lo;
    u.dN = (unsigned int)(an - lo); u.dW = (unsigned int)(aw - lo);
    u.limNode = p.nodesBytes - kFetchBytes;
    u.limTri = leaf_link((int)((p.woopBytes - kFetchBytes) >> kRowShift));
    u.oddBase = u.limNode + 1u; u.oddSpan = (unsigned)u.limTri - u.oddBase;
    if (TRIM) asm volatile("" : "+s"(u.oddBase), "+s"(u.oddSpan));   // (two numbers of their own: seen through, the range test is folded back into flatOk's compares and their 0 / 1 VGPR)
    return u;
}

// FLAT: the texture-address unit charges a wave-level load instruction about 16 cycles whatever its exec mask, so the two masked
// groups of fetch64_two_buffers cost 128 TA cycles per iteration and made the unified loop TA-bound (0.6-0.87 busy, profiles/r03v_*).
// With FLAT every live lane forms the 64-bit address of its own 64 bytes and ONE group of four global loads serves nodes and triangles
// alike (64 TA cycles).  Global loads are not range-checked: a lane whose 64 bytes would end beyond its buffer (an empty leaf's
// terminator in the last 48 bytes of triWoop; a malformed child offset) takes the descriptor path instead, which reads zeros there.
// One unified step, in two halves (the two-rays-per-lane experiment of round 5 stepped two rays per iteration with them: 24 % slower --
// 85 VGPRs, five waves per SIMD; scripts/studies/rejected_patches/two_rays_per_lane.patch, EXPERIMENTS.md).
// unified_fetch: one 64-byte fetch per lane from its own buffer -- the node of a lane at an inner node, the triangle (48 B + the following
// word) of a lane at a leaf.  Issues the loads and, apart from the rare end-of-buffer lanes, does not wait for them.
// `live`: the wave's lanes that hold a node or a triangle cursor (node != kSentinel), as the loop's own ballot has them.
// TRIM (the per-ray bodies): the end-of-buffer test as one unsigned compare per kind and one range test for "neither", the masks formed
// as SGPR pairs.  The persistent kernels keep the earlier form: the two scalars more cost them scalar spills.
template <bool FLAT, bool TRIM = false>
__device__ __forceinline__ void unified_fetch(const UnifiedBufs& ub, int node, unsigned long long live, float4& a, float4& b, float4& c, float4& d)
{
    const bool inner = (unsigned)node < (unsigned)kSentinel;
    const bool atTri = node < 0;
    // (Written as `inner ? ld4(nodes, ..) : ld4(woop, ..)` hipcc selects the descriptor per lane and wraps every load in a waterfall loop.)
    if (FLAT) {
        asm volatile("" : "=v"(a.x), "=v"(a.y), "=v"(a.z), "=v"(a.w), "=v"(b.x), "=v"(b.y), "=v"(b.z), "=v"(b.w));   // defined, whatever the lane
        asm volatile("" : "=v"(c.x), "=v"(c.y), "=v"(c.z), "=v"(c.w), "=v"(d.x), "=v"(d.y), "=v"(d.z), "=v"(d.w));
        // one unsigned compare per kind (extents are >= 64 here, so limTri < 0: as unsigned numbers the cursors from limTri up are the
        // negative ones >= limTri, and limNode lies below the sentinel)
        const bool okNode = (unsigned)node <= ub.limNode, okTri = TRIM ? (unsigned)node >= (unsigned)ub.limTri : atTri && node >= ub.limTri;
        const bool flatOk = okNode || okTri;
        const unsigned int cofs = okNode ? ub.dN + (unsigned)node : ub.dW + ((unsigned)leaf_row(node) << kRowShift);   // from the scalar base: a 32-bit offset
        if (flatOk) {   // (global address space spelled out: the base comes out of integer arithmetic, and a generic pointer would be a flat_load)
            typedef const __attribute__((address_space(1))) u32x4* global_u4_ptr;
            const global_u4_ptr q = (global_u4_ptr)((const __attribute__((address_space(1))) char*)ub.base + cofs);
            const u32x4 qa = q[0], qb = q[1], qc = q[2], qd = q[3];
            a = as_f4(qa); b = as_f4(qb); c = as_f4(qc); d = as_f4(qd);
        }
        if (TRIM) {
            // masks stay masks: the ballot of a compare that has no other use is the compare's own SGPR pair (of a predicate that also steers
            // lanes, like flatOk, hipcc makes a 0 / 1 VGPR and compares that) -- so "neither" is asked once more, as one range test
            const unsigned long long odd = live & __builtin_amdgcn_ballot_w64((unsigned)node - ub.oddBase < ub.oddSpan);
            if (__builtin_expect(odd != 0ull, 0))   // rare: range-checked descriptor loads, into the same registers, for the lanes at the very end of a buffer
                fetch64_two_buffers_into(ub.rNodes, ub.rWoop, inner ? node : leaf_row(node) * kRowBytes, odd & __builtin_amdgcn_ballot_w64(inner),
                                         odd & __builtin_amdgcn_ballot_w64(atTri), a, b, c, d);
        } else {
            const unsigned long long odd = __ballot((inner || atTri) && !flatOk);
            if (odd != 0ull)   // rare: range-checked descriptor loads, into the same registers, for the lanes at the very end of a buffer
                fetch64_two_buffers_into(ub.rNodes, ub.rWoop, inner ? node : leaf_row(node) * kRowBytes, __ballot(inner && !flatOk), __ballot(atTri && !flatOk), a, b, c, d);
        }
    } else {
        const int ofs = inner ? node : leaf_row(node) * kRowBytes;   // four loads under the inner lanes' mask and four under the triangle lanes' mask into the SAME registers, one wait
        fetch64_two_buffers(ub.rNodes, ub.rWoop, ofs, __ballot(inner), __ballot(atTri), a, b, c, d);
    }
}

}  // namespace ntr
