// trace_wide_lane.h -- one lane's step on a 4-wide node (wide_bvh.h), stated once for the two kernels that walk such nodes:
// trace_wide_kernels.hip (ntr_trace_wide) and trace_instanced_wide_kernels.hip (ntr_trace_instanced_wide).  The rule is the numpy spec
// tests/np_bvh_wide.py.  Shared by both: order2 and wide_advance (the step), and NTR_WIDE_ROWS4 / NTR_WIDE_ROWS3, the loads of a node's or
// a triangle's rows, from which each unit's fetch is built -- fetch_wide_or_triangle here, for ntr_trace_wide's two descriptors, and
// fetch_two_level_wide in trace_instanced_wide_kernels.hip, for the two-level trace's five.  The helpers stay in an anonymous namespace,
// as they were in trace_wide_kernels.hip: that unit's kernels are the kernels they were, instruction for instruction
// (scripts/kernel_isa_diff.sh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wide_bvh.h"
#include "trace_lane.h"

// The loads of one exec-masked group of a wide fetch, through descriptor operand R at byte offset %[ofs]: rows 0..3 into %[a]..%[d] (a
// wide node's first four rows, a triangle and the word behind it, an instance record), rows 4..6 into %[e]..%[g] (a wide node's others)
#define NTR_WIDE_ROWS4(R)                                                   \
    "buffer_load_dwordx4 %[a], %[ofs], %[" R "], 0 offen\n\t"               \
    "buffer_load_dwordx4 %[b], %[ofs], %[" R "], 0 offen offset:16\n\t"     \
    "buffer_load_dwordx4 %[c], %[ofs], %[" R "], 0 offen offset:32\n\t"     \
    "buffer_load_dwordx4 %[d], %[ofs], %[" R "], 0 offen offset:48\n\t"
#define NTR_WIDE_ROWS3(R)                                                   \
    "buffer_load_dwordx4 %[e], %[ofs], %[" R "], 0 offen offset:64\n\t"     \
    "buffer_load_dwordx4 %[f], %[ofs], %[" R "], 0 offen offset:80\n\t"     \
    "buffer_load_dwordx4 %[g], %[ofs], %[" R "], 0 offen offset:96\n\t"

namespace ntr {
namespace {

// Lanes of maskN fetch rows 0..6 of the wide node at byte offset `ofs` into a..g, lanes of maskT the 64 bytes at `ofs` of the Woop rows
// into a..d (range-checked: beyond the extent a load returns 0 and touches no memory); the other lanes keep what the registers held.
__device__ __forceinline__ void fetch_wide_or_triangle(u32x4 rWide, u32x4 rWoop, int ofs, unsigned long long maskN, unsigned long long maskT,
                                                       float4& a, float4& b, float4& c, float4& d, float4& e, float4& f, float4& g)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d), ve = as_u4(e), vf = as_u4(f), vg = as_u4(g);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 "s_and_b64 exec, %[sav], %[mn]\n\t"
                 "s_cbranch_execz .Lwd_fetch_n%=\n\t"
                 NTR_WIDE_ROWS4("rn") NTR_WIDE_ROWS3("rn")
                 ".Lwd_fetch_n%=:\n\t"
                 "s_and_b64 exec, %[sav], %[mt]\n\t"
                 "s_cbranch_execz .Lwd_fetch_t%=\n\t"
                 NTR_WIDE_ROWS4("rt")
                 ".Lwd_fetch_t%=:\n\t"
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [e] "+v"(ve), [f] "+v"(vf), [g] "+v"(vg), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [rn] "s"(rWide), [rt] "s"(rWoop), [mn] "s"(maskN), [mt] "s"(maskT)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd); e = as_f4(ve); f = as_f4(vf); g = as_f4(vg);
}

// compare-exchange on (mn, k, link): afterwards the pair is in ascending (mn, k).  No mn is a NaN here, and k differs, so the order is total.
__device__ __forceinline__ void order2(float& mA, int& kA, int& lA, float& mB, int& kB, int& lB)
{
    const bool swp = mA > mB || (mA == mB && kA > kB);
    const float m = swp ? mB : mA; mB = swp ? mA : mB; mA = m;
    const int k = swp ? kB : kA; kB = swp ? kA : kB; kA = k;
    const int l = swp ? lB : lA; lB = swp ? lA : lB; lA = l;
}

// One wide node of the spec: the four boxes, the candidates in ascending (mn, k), the nearest first and the others pushed farthest first
template <bool FAST>
__device__ __forceinline__ void wide_advance(const float4& a, const float4& b, const float4& c, const float4& d, const float4& e, const float4& f,
                                             const float4& g, const RayRegs& r, int& node, LaneStack& st, int (&spill)[SPILL_DEPTH],
                                             unsigned int* status)
{
    float mn[4], mx[4];
    ray_box2<FAST, 8>(r, a, b, c, mn[0], mx[0], mn[1], mx[1]);
    ray_box2<FAST, 8>(r, e, f, g, mn[2], mx[2], mn[3], mx[3]);
    int link[4] = {__float_as_int(d.x), __float_as_int(d.y), __float_as_int(d.z), __float_as_int(d.w)};
    int k[4];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool cand = link[i] != 0 && (mn[i] <= mx[i]) && (mx[i] >= r.tmin) && (mn[i] <= r.tmax);
        n += cand ? 1 : 0;
        // a slot that is no candidate sorts behind every candidate: +inf, and a k above the candidates' (a candidate's mn may be +inf too)
        mn[i] = cand ? mn[i] : __builtin_inff();
        k[i] = cand ? i : i + 4;
    }
    order2(mn[0], k[0], link[0], mn[1], k[1], link[1]);
    order2(mn[2], k[2], link[2], mn[3], k[3], link[3]);
    order2(mn[0], k[0], link[0], mn[2], k[2], link[2]);
    order2(mn[1], k[1], link[1], mn[3], k[3], link[3]);
    order2(mn[1], k[1], link[1], mn[2], k[2], link[2]);
    if (n > 3) stack_push(st, spill, link[3], status);
    if (n > 2) stack_push(st, spill, link[2], status);
    if (n > 1) stack_push(st, spill, link[1], status);
    node = n > 0 ? link[0] : stack_pop(st, spill);
}

}  // namespace
}  // namespace ntr
