// trace_prologue.h -- the wave-uniform prologue of the BVH traversal kernels (trace_kernels.hip): the top of the tree through the scalar
// cache while every live lane of a wave holds the same inner node, and the certain steps that skip the exact slab test there.
// Its preconditions (the node buffer's 64-byte alignment, certainSteps with NTR_BVH_ORDERED) and the descent limit reach the per-ray bodies
// combined by the host (HOSTK: TraceConsts::switches, descentLim); the persistent kernels' fresh waves check and form them here.
#pragma once
#include "trace_lane.h"

namespace ntr {

// Wave-uniform prologue (round 5).  The rays of a fresh wave all start at the root, and the rays of one wave -- an 8 x 8 pixel tile, or
// the AO samples of eight neighbouring pixels -- take the same way down the top of the tree: while every live lane holds the SAME inner
// node, that node is fetched ONCE through the scalar cache (s_load, no texture-path cycles: the per-lane fetch costs the TA 64 cycles per
// wave and iteration whatever the lanes hold) and the planes are scalar operands of the same arithmetic.  The loop ends for good at the
// first iteration in which the lanes disagree, or hold a leaf: the test (one v_readlane, one compare) is paid only while it succeeds --
// run on EVERY iteration it cost more than the fetches it saved (round 2), and looking again every 2 / 4 / 8 / 16 iterations of the
// general loop loses 1-4 % (profiles/r05_uniform_recheck_knob.txt): once apart, the lanes of a wave rarely all meet again.  Measured
// and left out as well: the same for a triangle every lane stands at (no gain, and 2.5 % lost to the larger loop:
// profiles/r05_uniform_prologue_levels_knob.txt), and the prologue after a persistent wave's refill (nothing).  Per-ray arithmetic, visiting order and
// stack are untouched: hit records cannot change.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) f32x4* const_f32x4_ptr;   // constant address space: a wave-uniform load becomes s_load

// CERTAIN (per-ray kernels, TraceParams::certainSteps): certain steps.  A short ray near the top of the tree -- an AO ray of length 5 in a
// 3 600-unit hall, 1e-4 off the surface it starts from -- has its origin inside one child box while the sibling is out of its reach, and
// plain comparisons of the planes against per-ray constants decide that exactly as the twelve quotients of the slab test would.
// Per ray and axis k, once per wave: the segment [segLo[k], segHi[k]] that contains the ray's extent on that axis.  The origin side is
// o[k] itself; the far side is o[k] +- reach[k] rounded outward (certain_reach, certain_end).  Per step and child c:
//   inside_c: lo_c[k] <= o[k] <= hi_c[k] on the three axes;    out_c: lo_c[k] > segHi[k] or hi_c[k] < segLo[k] on some axis.
// A lane is certain when (inside_0 && out_1) || (inside_1 && out_0); when EVERY live lane is, each takes the child it is inside, nothing
// is pushed and no quotient is formed.  Otherwise the step is inner_advance as before.
// Why the outcome is the slab test's own (FAST ranges above: no NaN, no zero divisor, every x = plane - o and every quotient is 0 or a
// normal number; tmin == 0; boxes lo <= hi; u = 2^-24; the quotient of the FAST path is the correctly rounded one, trace_arith.h):
//  (a) RN(a - b) has the sign of a - b and RN(x / d) the sign of x / d (0 only for x == 0).  So for inside_c the near quotient of every axis
//      is <= 0 and the far one >= 0, whichever way d points: mn <= 0 <= mx, mx >= 0 = tmin, mn <= 0 < tmax (a live ray has tmin < tmax; no
//      leaf is visited in the prologue, so tmax is still the ray's own).  All three accept tests hold: the child is accepted.
//  (b) Behind the origin.  d > 0: segLo = o, and hi_c < o makes the far quotient RN(RN(hi_c - o) / d) < 0.  d < 0: segHi = o, and lo_c > o
//      makes the far quotient RN(RN(lo_c - o) / d) < 0.  Either way mx < 0 = tmin: rejected.  No margin is needed.
//  (c) Beyond the reach.  d > 0: lo_c > segHi >= o + reach (real numbers, certain_end) gives x = lo_c - o > reach >= tmax |d| (1 + 13 u)
//      (certain_reach).  RN(x) >= x (1 - u), and the exact quotient of that by d is >= tmax (1 + 13 u)(1 - u) > tmax (1 + 2 u), which is at
//      least the float after tmax, so by monotone rounding the near quotient is > tmax.  d < 0: the same with hi_c < segLo <= o - reach and
//      the near plane hi_c.  So mn > tmax: rejected.
//  (d) inside_c and out_c exclude each other (segLo <= o <= segHi), so a certain lane accepts exactly one child: no ordering decision, no push.
// The test costs 12 to 24 VALU against the 88 of the exact step; a wave whose lanes are uncertain twice in a row stops asking.
// Carried descent (TraceParams::certainDescent).  A certain step in which every live lane is inside the SAME child c gives every live lane
// the node c, pushes nothing and leaves tmax alone; the loop top would then read c back out of the first live lane and find the lanes
// agreed.  So while c is an inner node whose record lies inside the buffer (the loop top's own test) the wave keeps it in a scalar register
// and loads the next record at once: about 30 instructions a step where writing c to the lanes and proving them uniform again issues
// about 75.  The lanes are written once, when the run ends: the lanes part (certain, both children taken), some lane is uncertain (the
// exact step runs on the record already loaded, counted as uncertain as before), or the child is a leaf.  There node, stack and tmax of
// every lane are what the per-step path has at the same step, and lanes at kSentinel are never written.  The predicate is certain_masks'
// either way, so (a)-(d) are the whole argument.
static constexpr int kCertainGiveUpAfter = 2;   // consecutive uncertain steps after which a wave runs the exact prologue only

// reach >= tmax |d| (1 + 13 u): p = RN(tmax |d|) >= tmax |d| (1 - u) while p is normal, and RN(p (1 + 2^-20)) >= p (1 + 16 u)(1 - u).  A product
// too small for that argument (or not a number) makes the far side unbounded: such a ray is never certain there.  tmax = inf likewise.
__device__ __forceinline__ float certain_reach(float tmax, float d)
{
    const float p = tmax * fabsf(d);
    return (p >= 0x1p-100f) ? p * 0x1.00001p0f : __builtin_inff();
}
// The far end o + reach (SIGN = +1) or o - reach (SIGN = -1), rounded outward: s = RN(o +- reach) is off by at most half an ulp of s -- a
// large loss relative to reach when |o| >> reach -- and |s| 2^-22 is two to four ulp of s (|s| < 2^-100 happens only when o and reach
// cancel, and then the sum is exact), so the result lies on the far side of the real o +- reach, and of o.  (Comparing a PLANE against s
// would already be safe -- a float above RN(y) is above y, rounding being monotone; the step outward is margin, one fma per axis and wave.)
template <int SIGN>
__device__ __forceinline__ float certain_end(float o, float reach)
{
    const float s = SIGN > 0 ? o + reach : o - reach;
    return __builtin_fmaf(fabsf(s), SIGN > 0 ? 0x1p-22f : -0x1p-22f, s);
}

// The comparisons of a certain step as lane masks, for the lanes of `live`: in0 = origin inside the closed box of child 0; in1 = the other lanes
// whose origin is inside child 1; reach = lanes of in0 / in1 whose sibling box is NOT out of reach (lo <= segHi and hi >= segLo on every axis).
// The wave is certain when in0 | in1 == live and reach == 0.  (A lane inside both boxes counts for in0 and then shows in `reach`: its sibling
// holds the origin.)  Each conjunction of six comparisons is a chain of v_cmpx, which narrows EXEC as it goes: twelve to twenty-four VALU
// instructions and no mask arithmetic -- written as `a <= x && x <= b && ...` the compiler forms every comparison into an SGPR pair and
// folds them with one scalar instruction each, about 50 SALU a step that wait for the VALU one by one (measured: VALU -12 %, SALU +19 %, no
// time gained).  Planes are scalar operands (the node came through the scalar cache).
// Returns the wave's next node where it is a scalar: the child word c0 (c1) when the wave is certain AND every live lane is inside child 0
// (child 1) -- in0 (in1) == live, reach == 0 -- and kSentinel otherwise.  The common case, every live lane inside child 0, is tested first and
// costs the twelve v_cmpx and eight scalar instructions; the masks are the same whichever path formed them.
__device__ __forceinline__ int certain_masks(f32x4 A, f32x4 B, f32x4 C, int c0, int c1, const RayRegs& r, float loX, float hiX, float loY, float hiY,
                                             float loZ, float hiZ, unsigned long long live, unsigned long long& in0, unsigned long long& in1,
                                             unsigned long long& reach)
{
    unsigned long long sav;
    int next;
    asm volatile(
        "s_mov_b64 %[sav], exec\n\t"
        "s_mov_b32 %[next], %[none]\n\t"
        "s_and_b64 exec, %[sav], %[live]\n\t"
        "v_cmpx_le_f32 vcc, %[ax], %[ox]\n\t"      // inside child 0: lo <= o && hi >= o per axis
        "v_cmpx_ge_f32 vcc, %[ay], %[ox]\n\t"
        "v_cmpx_le_f32 vcc, %[az], %[oy]\n\t"
        "v_cmpx_ge_f32 vcc, %[aw], %[oy]\n\t"
        "v_cmpx_le_f32 vcc, %[cx], %[oz]\n\t"
        "v_cmpx_ge_f32 vcc, %[cy], %[oz]\n\t"
        "s_mov_b64 %[in0], exec\n\t"
        "s_cmp_eq_u64 %[in0], %[live]\n\t"
        "s_cbranch_scc0 .Lcs_g%=\n\t"
        "s_mov_b64 %[in1], 0\n\t"                   // every live lane is inside child 0: child 1 within reach of any?
        "v_cmpx_le_f32 vcc, %[bx], %[hx]\n\t"
        "v_cmpx_ge_f32 vcc, %[by], %[lx]\n\t"
        "v_cmpx_le_f32 vcc, %[bz], %[hy]\n\t"
        "v_cmpx_ge_f32 vcc, %[bw], %[ly]\n\t"
        "v_cmpx_le_f32 vcc, %[cz], %[hz]\n\t"
        "v_cmpx_ge_f32 vcc, %[cw], %[lz]\n\t"
        "s_mov_b64 %[reach], exec\n\t"
        "s_cbranch_execnz .Lcs_e%=\n\t"
        "s_mov_b32 %[next], %[c0]\n\t"
        "s_branch .Lcs_e%=\n"
        ".Lcs_g%=:\n\t"
        "s_and_b64 exec, %[sav], %[live]\n\t"
        "s_andn2_b64 exec, exec, %[in0]\n\t"      // the other live lanes: inside child 1?
        "s_cbranch_execz .Lcs_a%=\n\t"
        "v_cmpx_le_f32 vcc, %[bx], %[ox]\n\t"
        "v_cmpx_ge_f32 vcc, %[by], %[ox]\n\t"
        "v_cmpx_le_f32 vcc, %[bz], %[oy]\n\t"
        "v_cmpx_ge_f32 vcc, %[bw], %[oy]\n\t"
        "v_cmpx_le_f32 vcc, %[cz], %[oz]\n\t"
        "v_cmpx_ge_f32 vcc, %[cw], %[oz]\n\t"
        "s_cbranch_execz .Lcs_a%=\n\t"
        "s_mov_b64 %[in1], exec\n\t"
        "v_cmpx_le_f32 vcc, %[ax], %[hx]\n\t"      // ... and child 0 within their reach?  lo <= segHi && hi >= segLo per axis
        "v_cmpx_ge_f32 vcc, %[ay], %[lx]\n\t"
        "v_cmpx_le_f32 vcc, %[az], %[hy]\n\t"
        "v_cmpx_ge_f32 vcc, %[aw], %[ly]\n\t"
        "v_cmpx_le_f32 vcc, %[cx], %[hz]\n\t"
        "v_cmpx_ge_f32 vcc, %[cy], %[lz]\n\t"
        "s_mov_b64 %[reach], exec\n\t"
        "s_branch .Lcs_b%=\n"
        ".Lcs_a%=:\n\t"
        "s_mov_b64 %[in1], 0\n\t"
        "s_mov_b64 %[reach], 0\n"
        ".Lcs_b%=:\n\t"
        "s_mov_b64 exec, %[in0]\n\t"
        "s_cbranch_execz .Lcs_c%=\n\t"
        "v_cmpx_le_f32 vcc, %[bx], %[hx]\n\t"      // the lanes inside child 0: child 1 within their reach?
        "v_cmpx_ge_f32 vcc, %[by], %[lx]\n\t"
        "v_cmpx_le_f32 vcc, %[bz], %[hy]\n\t"
        "v_cmpx_ge_f32 vcc, %[bw], %[ly]\n\t"
        "v_cmpx_le_f32 vcc, %[cz], %[hz]\n\t"
        "v_cmpx_ge_f32 vcc, %[cw], %[lz]\n\t"
        "s_or_b64 %[reach], %[reach], exec\n"
        ".Lcs_c%=:\n\t"
        "s_cmp_eq_u64 %[in1], %[live]\n\t"          // every live lane inside child 1 and child 0 out of everyone's reach?
        "s_cbranch_scc0 .Lcs_e%=\n\t"
        "s_cmp_eq_u64 %[reach], 0\n\t"
        "s_cselect_b32 %[next], %[c1], %[next]\n"
        ".Lcs_e%=:\n\t"
        "s_mov_b64 exec, %[sav]"
        : [sav] "=&s"(sav), [in0] "=&s"(in0), [in1] "=&s"(in1), [reach] "=&s"(reach), [next] "=&s"(next)
        : [live] "s"(live), [ax] "s"(A.x), [ay] "s"(A.y), [az] "s"(A.z), [aw] "s"(A.w), [bx] "s"(B.x), [by] "s"(B.y), [bz] "s"(B.z), [bw] "s"(B.w),
          [cx] "s"(C.x), [cy] "s"(C.y), [cz] "s"(C.z), [cw] "s"(C.w), [c0] "s"(c0), [c1] "s"(c1), [none] "i"(kSentinel), [ox] "v"(r.ox), [oy] "v"(r.oy),
          [oz] "v"(r.oz), [lx] "v"(loX), [hx] "v"(hiX), [ly] "v"(loY), [hy] "v"(hiY), [lz] "v"(loZ), [hz] "v"(hiZ)
        : "vcc", "scc");
    return next;
}
// node = c0 in the lanes of m0, c1 in the lanes of m1 (disjoint); the other lanes keep theirs
__device__ __forceinline__ void take_children(int& node, int c0, int c1, unsigned long long m0, unsigned long long m1)
{
    unsigned long long sav;
    asm volatile(
        "s_mov_b64 %[sav], exec\n\t"
        "s_mov_b64 exec, %[m1]\n\t"
        "v_mov_b32 %[node], %[c1]\n\t"
        "s_mov_b64 exec, %[m0]\n\t"
        "v_mov_b32 %[node], %[c0]\n\t"
        "s_mov_b64 exec, %[sav]"
        : [sav] "=&s"(sav), [node] "+v"(node)
        : [m0] "s"(m0), [m1] "s"(m1), [c0] "s"(c0), [c1] "s"(c1));
}

// HOSTK (the per-ray bodies): the preconditions come checked and the descent limit formed by the host (TraceConsts).
template <bool FAST, int OCT, bool CERTAIN = false, bool HOSTK = false>
__device__ __forceinline__ void uniform_prologue(const UnifiedBufs& ub, const RayRegs& r, int& node, LaneStack& st, int (&spill)[SPILL_DEPTH],
                                                 unsigned int* status)
{
    if (!HOSTK && (reinterpret_cast<unsigned long long>(ub.nodes) & (unsigned long long)(kNodeBytes - 1)) != 0ull) return;   // (s_load_dwordx16 wants the record 64-byte aligned; HOSTK: part of ub.uniformPrologue)
    // certain steps: wave-uniform preconditions, checked once (FAST is the caller's fastWave)
    bool tryCertain = false;
    int uncertain = 0;
    float loX = 0.0f, hiX = 0.0f, loY = 0.0f, hiY = 0.0f, loZ = 0.0f, hiZ = 0.0f;   // segLo / segHi
    if (CERTAIN && FAST) {
        tryCertain = ub.certainSteps && __ballot(node != kSentinel && r.tmin != 0.0f) == 0ull;
        if (tryCertain) {
            const float fx = certain_reach(r.tmax, r.dx), fy = certain_reach(r.tmax, r.dy), fz = certain_reach(r.tmax, r.dz);
            loX = r.dx < 0.0f ? certain_end<-1>(r.ox, fx) : r.ox; hiX = r.dx < 0.0f ? r.ox : certain_end<1>(r.ox, fx);
            loY = r.dy < 0.0f ? certain_end<-1>(r.oy, fy) : r.oy; hiY = r.dy < 0.0f ? r.oy : certain_end<1>(r.oy, fy);
            loZ = r.dz < 0.0f ? certain_end<-1>(r.oz, fz) : r.oz; hiZ = r.dz < 0.0f ? r.oz : certain_end<1>(r.oz, fz);
        }
    }
    // carried certain descent: a child word c is the wave's next scalar node when 1 <= c <= descentLim -- an inner node whose 64 bytes lie
    // inside the buffer (the test of the loop top below; 0, the root, is no child of a well-formed tree and goes through the lanes); 0 = off
    unsigned int descentLim = HOSTK ? ub.descentLim : !ub.certainDescent ? 0u : ub.nodesBytes - (unsigned)kNodeBytes < (unsigned)kSentinel ? ub.nodesBytes - (unsigned)kNodeBytes : (unsigned)kSentinel - 1u;
    if (!HOSTK) asm volatile("" : "+s"(descentLim));   // (one number to compare with: left to see through it, the compiler tests the switch again on every step)
    for (;;) {
        const bool live = node != kSentinel;
        const unsigned long long liveMask = __ballot(live);
        if (liveMask == 0ull) return;
        const int unode = __builtin_amdgcn_readlane(node, (int)__builtin_ctzll(liveMask));   // the first live lane's node: a scalar
        if (__ballot(live && node != unode) != 0ull) return;                                  // the lanes disagree: the general loop from here on
        if ((unsigned)unode >= (unsigned)kSentinel || (unsigned)unode > (HOSTK ? ub.limNode : ub.nodesBytes - (unsigned)kNodeBytes)) return;   // a leaf (or a malformed offset): likewise
        unsigned int snode = (unsigned)unode;   // the wave's node while it is a scalar (carried certain descent)
        f32x4 A, B, C, D;
        if (CERTAIN && FAST && tryCertain) {
            unsigned long long in0, in1, reach;
            for (;;) {
                const const_f32x4_ptr q = (const_f32x4_ptr)(ub.nodes + snode);
                A = q[0]; B = q[1]; C = q[2]; D = q[3];
                const int next = certain_masks(A, B, C, __float_as_int(D.x), __float_as_int(D.y), r, loX, hiX, loY, hiY, loZ, hiZ, liveMask, in0, in1, reach);
                if ((unsigned)next - 1u >= descentLim) break;   // not certain, the lanes part, or the child is a leaf (beyond the extent): the lanes take over
                snode = (unsigned)next;                   // certain, every live lane to the same inner child: nothing to write, the next record
            }
            if (snode != (unsigned)unode) {               // carried steps were certain steps: the lanes arrive where they would have stepped to
                if (live) node = (int)snode;
                uncertain = 0;
            }
            if ((in0 | in1) == liveMask && reach == 0ull) {
                take_children(node, __float_as_int(D.x), __float_as_int(D.y), in0, in1);
                uncertain = 0;
                continue;
            }
            if (++uncertain >= kCertainGiveUpAfter) tryCertain = false;
        } else {
            const const_f32x4_ptr q = (const_f32x4_ptr)(ub.nodes + snode);
            A = q[0]; B = q[1]; C = q[2]; D = q[3];
        }
        if (live)
            inner_advance<FAST, OCT>(make_float4(A.x, A.y, A.z, A.w), make_float4(B.x, B.y, B.z, B.w), make_float4(C.x, C.y, C.z, C.w),
                                     make_float4(D.x, D.y, D.z, D.w), r, node, st, spill, status);
    }
}

}  // namespace ntr
