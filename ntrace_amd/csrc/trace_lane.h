// trace_lane.h -- one lane of the BVH traversal kernels (trace_kernels.hip): its ray, its stack, and the steps the ray takes -- one inner
// node, one leaf, or (unified-step loop) whichever of the two the lane's 64 bytes hold.  Each step is stated once.
//
// ARITHMETIC.  The hit records must be bit-exact against the reference's *CPU*
// tracer (CudaBVH::trace<BVHLayout_Compact>, src/rt/cuda/CudaBVH.cpp:698-784), so
// every decision reproduces its binary32 expressions, not the CUDA kernels':
//   slabs      (lo - o) / d, true IEEE division      (src/rt/Util.cpp:39-40)
//   min / max  selects (a<b)?a:b, folded x,y,z       (Defs.hpp:212-213, Math.hpp:146-147)
//   accept     tmin<=tmax && tmax>=ray.tmin && tmin<=ray.tmax   (CudaBVH.cpp:742-743)
//   order      near child = smaller tmin, ties -> child 0         (CudaBVH.cpp:761)
//   Woop       unfused left-to-right dots incl. the leading 0 and the w term
//              (Util.cpp:106-121, Math.hpp:185), 1.f/x then multiply
// Compiled with -ffp-contract=off and without fast-math.
//
// Two code paths compute the slab test, both exact:
//   GENERIC  `/` (hipcc's correctly rounded f32 divide: v_div_scale / v_rcp / fma chain /
//            v_div_fmas / v_div_fixup) and select-form min/max.  Valid for every input
//            (zero direction components, NaN, infinities, denormals).
//   FAST     for waves whose rays are all "nice" (see ray_is_nice) over a BVH flagged
//            NTR_BVH_FASTDIV: in that range nothing over- or underflows and v_div_scale never
//            rescales, so a quotient is  r = RN(1/d)  (the IEEE divide, once per ray and axis) and,
//            per quotient,  q0 = x*r;  e = fma(-d,q0,x);  q = fma(e,r,q0)  -- three operations.
//            With the CORRECTLY ROUNDED reciprocal one residual correction gives RN(x/d), the
//            GENERIC path's bits (exact_rcp, trace_arith.h: why, and how every quotient that could differ
//            was checked).  Rounds 1-3 used the hardware divide's own chain instead -- v_rcp
//            refined once, which is not always RN(1/d), and therefore TWO corrections: five
//            operations per quotient, sixty of the ~100 vector instructions of an inner-node step.
//            No NaN/inf can arise in the range either, so v_min3/v_max3 equal the select-form
//            folds up to the sign of zero, which no later comparison can observe.
//   ntr_selftest_division() / ntr_selftest_division_hard() check FAST == GENERIC bit for bit on the device.
// Who may take FAST is stated twice: ray_is_nice, the rule in float compares (the pools' refills, the wide and instanced traces), and
// ray_class, the same ranges as integer arithmetic on the words with one compare at the end (a fresh wave's vote in perray_body);
// ntr_selftest_ray_class holds the second against the first.  triangle_step<QUIRK> likewise has the reference's form and, for waves in
// which no lane holds tmax = +inf (wave_may_quirk), the form in which a miss writes nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

#include "trace_kernels.h"
#include "trace_arith.h"
#include "trace_fetch.h"

namespace ntr {

static constexpr int LDS_DEPTH = 16;
static constexpr int SPILL_DEPTH = 88;        // 16 + 88 >= the reference CPU stack of 100 (CudaBVH.cpp:701)

__device__ __forceinline__ float sel_min(float a, float b) { return (a < b) ? a : b; }
__device__ __forceinline__ float sel_max(float a, float b) { return (a > b) ? a : b; }

struct RayRegs {
    float ox, oy, oz, tmin;
    float dx, dy, dz, tmax;  // tmax shrinks to the closest accepted t (CudaBVH.cpp:1215)
    float rx, ry, rz;        // FAST path: correctly rounded reciprocals of dx,dy,dz
};

// ---- FAST-path preconditions ---------------------------------------------------------
// FAST-path ranges.  Directions: 2^-40 <= |d| <= 2^20.  Box coordinates: |c| < 2^55 (BVH flag
// NTR_BVH_FASTDIV).  Ray origin components: 2^-36 <= |o| < 2^55 -- then x = c - o is 0 or
// |x| >= 2^-84 for ANY such c (a c much smaller than o leaves x = -o; otherwise both operands
// are >= 2^-61 and a non-zero difference is at least one ulp of that).  An origin component
// that is exactly 0 makes x = c, which is only safe when the BVH has no tiny coordinates
// (flag NTR_BVH_NOTINY: c == 0 or |c| >= 2^-93).  In these ranges |x| < 2^56,
// exponent(x) - exponent(d) < 96, |x| >= 2^-103 and |x/d| >= 2^-113: none of v_div_scale's
// rescaling cases, and every residual of the fma chain is exactly representable.
__device__ __forceinline__ bool nice_dir(float v) { const float a = fabsf(v); return a >= 0x1p-40f && a <= 0x1p20f; }
__device__ __forceinline__ bool nice_pos(float v, bool zeroOk)
{
    const float a = fabsf(v);
    return (a >= 0x1p-36f && a < 0x1p55f) || (zeroOk && v == 0.0f);
}
// THE RULE, as the ranges above state it: what the pools' refills ask per ray (start_ray), and what the device self test
// ntr_selftest_ray_class holds ray_class against.
__device__ __forceinline__ bool ray_is_nice(const RayRegs& r, uint32_t bvhFlags)
{
    const bool zeroOk = (bvhFlags & NTR_BVH_NOTINY) != 0;
    return nice_dir(r.dx) && nice_dir(r.dy) && nice_dir(r.dz) && nice_pos(r.ox, zeroOk) && nice_pos(r.oy, zeroOk) &&
           nice_pos(r.oz, zeroOk);
}
// What a fresh wave of the per-ray kernels votes with (perray_body): the rule as integer arithmetic on the six words, straight-line, one number per ray.  As floats the twelve range
// compares fold through five exec-mask levels, ~62 instructions of every wave's set-up; here it is 17 VALU and the wave's vote is ONE
// compare whose only use is the ballot (EXPERIMENTS.md).
// Non-negative floats order like their bit patterns, so with s = word << 1 (the sign shifted out; s is even) a magnitude range [lo, hi] is
// s - 2 lo <= 2 (hi - lo) in unsigned arithmetic: below the range the difference wraps to at least 2^32 - 2 lo, which is above every
// bound used here; infinities and NaN (s >= 0xFF000000) land above the bounds as well, denormals and zeros (s < 2^24) below the range.
//   direction  2^-40 <= |d| <= 2^20:  wd = s - 0x57000000 <= 0x3C000000    (both ends included)
//   position   2^-36 <= |o| <  2^55:  wp = s - 0x5B000000 <= 0x5AFFFFFE    (2^55 itself, wp = 0x5B000000, excluded: wp is even)
//   +0 / -0 position (s = 0, wp = kPosZero) passes under NTR_BVH_NOTINY only: wp == zeroWord ? 0 : wp, where zeroWord is kPosZero with the
//   flag and the odd kPosZero | 1, which no wp equals, without it.
// The class is the largest of the three wp and of the largest wd moved up by kDirPad = 0x5AFFFFFE - 0x3C000000 with a SATURATING add (a
// wrapped wd stays large): nice <=> class <= kNiceMax, for every bit pattern of every component.
static constexpr unsigned int kDirLo2 = 0x57000000u, kDirSpan2 = 0x3C000000u, kPosLo2 = 0x5B000000u, kNiceMax = 0x5AFFFFFEu;
static constexpr unsigned int kDirPad = kNiceMax - kDirSpan2, kPosZero = 0u - kPosLo2;
__device__ __forceinline__ unsigned int nice_zero_word(uint32_t bvhFlags) { return (bvhFlags & NTR_BVH_NOTINY) ? kPosZero : (kPosZero | 1u); }
__device__ __forceinline__ unsigned int ray_class(const RayRegs& r, unsigned int zeroWord)
{
    const unsigned int dx = (__float_as_uint(r.dx) << 1) - kDirLo2, dy = (__float_as_uint(r.dy) << 1) - kDirLo2, dz = (__float_as_uint(r.dz) << 1) - kDirLo2;
    unsigned int px = (__float_as_uint(r.ox) << 1) - kPosLo2, py = (__float_as_uint(r.oy) << 1) - kPosLo2, pz = (__float_as_uint(r.oz) << 1) - kPosLo2;
    px = px == zeroWord ? 0u : px; py = py == zeroWord ? 0u : py; pz = pz == zeroWord ? 0u : pz;
    const unsigned int d = max(max(dx, dy), dz), p = max(max(px, py), pz);
    return max(p, __builtin_elementwise_add_sat(d, kDirPad));
}
// Intersect::RayBox for BOTH children of a node (Util.cpp:34-46).  The FAST form evaluates
// the twelve quotients stage by stage (all q0, then all e1, ...) so that consecutive
// instructions are independent: a lone wave cannot issue a VALU op that depends on the
// previous one back to back.
// OCT < 8 (FAST only): every live ray of the wave has direction signs OCT (bit 0: dx < 0, bit 1: dy < 0, bit 2: dz < 0) and every box
// has lo <= hi (NTR_BVH_ORDERED).  Rounding is monotone, so (lo - o) / d <= (hi - o) / d for d > 0 and >= for d < 0: the smaller
// quotient of a slab is known without comparing -- the same value min / max would pick, six instructions per child less.
template <bool FAST, int OCT = 8>
__device__ __forceinline__ void ray_box2(const RayRegs& r, const float4& n0, const float4& n1, const float4& nz,
                                         float& mn0, float& mx0, float& mn1, float& mx1)
{
    if (FAST) {
        // x[k] = plane - origin ; axis of slot k: x x y y z z (child 0), x x y y z z (child 1)
        float x[12] = {n0.x - r.ox, n0.y - r.ox, n0.z - r.oy, n0.w - r.oy, nz.x - r.oz, nz.y - r.oz,
                       n1.x - r.ox, n1.y - r.ox, n1.z - r.oy, n1.w - r.oy, nz.z - r.oz, nz.w - r.oz};
        const float d[3] = {r.dx, r.dy, r.dz};
        const float rc[3] = {r.rx, r.ry, r.rz};
        float q[12], e[12];
#pragma unroll
        for (int k = 0; k < 12; k++) q[k] = x[k] * rc[(k % 6) >> 1];
#pragma unroll
        for (int k = 0; k < 12; k++) e[k] = __builtin_fmaf(-d[(k % 6) >> 1], q[k], x[k]);
#pragma unroll
        for (int k = 0; k < 12; k++) q[k] = __builtin_fmaf(e[k], rc[(k % 6) >> 1], q[k]);
        if (OCT < 8) {
            constexpr int sx = OCT & 1, sy = (OCT >> 1) & 1, sz = (OCT >> 2) & 1;   // 1: the hi plane is the near one
            mn0 = fmaxf(fmaxf(q[0 + sx], q[2 + sy]), q[4 + sz]);
            mx0 = fminf(fminf(q[1 - sx], q[3 - sy]), q[5 - sz]);
            mn1 = fmaxf(fmaxf(q[6 + sx], q[8 + sy]), q[10 + sz]);
            mx1 = fminf(fminf(q[7 - sx], q[9 - sy]), q[11 - sz]);
        } else {
            mn0 = fmaxf(fmaxf(fminf(q[0], q[1]), fminf(q[2], q[3])), fminf(q[4], q[5]));
            mx0 = fminf(fminf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3])), fmaxf(q[4], q[5]));
            mn1 = fmaxf(fmaxf(fminf(q[6], q[7]), fminf(q[8], q[9])), fminf(q[10], q[11]));
            mx1 = fminf(fminf(fmaxf(q[6], q[7]), fmaxf(q[8], q[9])), fmaxf(q[10], q[11]));
        }
    } else {
        float t0x = (n0.x - r.ox) / r.dx, t1x = (n0.y - r.ox) / r.dx;
        float t0y = (n0.z - r.oy) / r.dy, t1y = (n0.w - r.oy) / r.dy;
        float t0z = (nz.x - r.oz) / r.dz, t1z = (nz.y - r.oz) / r.dz;
        mn0 = sel_max(sel_max(sel_min(t0x, t1x), sel_min(t0y, t1y)), sel_min(t0z, t1z));
        mx0 = sel_min(sel_min(sel_max(t0x, t1x), sel_max(t0y, t1y)), sel_max(t0z, t1z));
        t0x = (n1.x - r.ox) / r.dx; t1x = (n1.y - r.ox) / r.dx;
        t0y = (n1.z - r.oy) / r.dy; t1y = (n1.w - r.oy) / r.dy;
        t0z = (nz.z - r.oz) / r.dz; t1z = (nz.w - r.oz) / r.dz;
        mn1 = sel_max(sel_max(sel_min(t0x, t1x), sel_min(t0y, t1y)), sel_min(t0z, t1z));
        mx1 = sel_min(sel_min(sel_max(t0x, t1x), sel_max(t0y, t1y)), sel_max(t0z, t1z));
    }
}

// dot(Vec4f a, Vec4f(b,bw)) as Math.hpp:185: r = 0; r += a[i]*b[i].
__device__ __forceinline__ float dot4(float4 a, float bx, float by, float bz, float bw)
{
    float r = 0.0f;
    r += a.x * bx;
    r += a.y * by;
    r += a.z * bz;
    r += a.w * bw;
    return r;
}

// Per-lane traversal stack: entries [0, LDS_DEPTH) in LDS laid out [entry][lane] (bank =
// lane % 32 whatever the per-lane depth -> conflict-free), deeper entries in a scratch array
// that only the (rare) overflow branches touch.  `sp` and the LDS base stay in registers.
typedef __attribute__((address_space(3))) int lds_int;

struct LaneStack {
    lds_int* lds;  // &s_stack[wave][0][lane]
    int sp;        // entries held in memory (LDS, then scratch)
    int tos;       // top of the stack, kept in a register: a pop hands out the next node without
                   // waiting for LDS; the entry below it is fetched off the critical path
};

__device__ __forceinline__ void stack_reset(LaneStack& st) { st.sp = 0; st.tos = kSentinel; }

template <int LD = LDS_DEPTH>   // LD: the entries this stack has in LDS
__device__ __forceinline__ void stack_push(LaneStack& st, int (&spill)[SPILL_DEPTH], int v, unsigned int* status)
{
    if (__builtin_expect(st.sp < LD, 1)) st.lds[st.sp * 64] = st.tos;
    else if (st.sp < LD + SPILL_DEPTH) spill[st.sp - LD] = st.tos;
    else { atomicOr(status, NTR_STATUS_STACK_OVERFLOW); return; }
    st.sp++;
    st.tos = v;
}
template <int LD = LDS_DEPTH>
__device__ __forceinline__ int stack_pop(LaneStack& st, int (&spill)[SPILL_DEPTH])
{
    const int r = st.tos;
    if (st.sp > 0) {
        st.sp--;
        st.tos = __builtin_expect(st.sp < LD, 1) ? st.lds[st.sp * 64] : spill[st.sp - LD];
    } else {
        st.tos = kSentinel;
    }
    return r;
}

// The per-ray bodies' pop (unified_advance<.., TRIM = true>): ONE LDS read in straight-line code, of the entry clamped into the LDS part,
// and the scratch entry fetched over it in the rare lanes that are deep -- an exec-mask level and half a dozen scalar instructions per
// site less than stack_pop's nested LDS / scratch select, in every step, whether or not a lane pops (EXPERIMENTS.md).  An empty stack needs no third source for `tos`: sp == 0 implies tos == kSentinel
// (stack_reset sets it, a push at sp == 0 stores it into entry 0, and the pop that returns to sp == 0 reads it back; the drain phase of
// the persistent kernels, which plants sentinels inside a stack, does not use this form), so the pop of the sentinel leaves `tos` as it is.
template <int LD = LDS_DEPTH>
__device__ __forceinline__ int stack_pop_flat(LaneStack& st, int (&spill)[SPILL_DEPTH])
{
    const int r = st.tos;
    if (st.sp > 0) {
        st.sp--;
        int v = st.lds[min(st.sp, LD - 1) * 64];
        if (__builtin_expect(st.sp >= LD, 0)) v = spill[st.sp - LD];
        st.tos = v;
    }
    return r;
}

// Keeps a loaded value live at this point so that hipcc cannot sink its load into a later
// conditional block (which would turn one memory round trip per node into two).
__device__ __forceinline__ void keep(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }
__device__ __forceinline__ void keep(unsigned int& v) { asm volatile("" : "+v"(v)); }
// ... the four words of a row as the register tuple the load wrote (kept word by word, hipcc renames five of the sixteen fetched registers
// with v_mov after the wait)
__device__ __forceinline__ void keep_row(float4& v) { u32x4 t = as_u4(v); asm volatile("" : "+v"(t)); v = as_f4(t); }

// rank of this lane among the lanes of m: the set bits of m below it (wave64 prefix popcount)
__device__ __forceinline__ int lane_rank(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

struct LaneStats {
    unsigned int inner, tris, leaves;
};

static constexpr int kNoNode = (int)0xFFFFFF00u;  // buffer offset beyond any extent (< 4 GiB)

__device__ __forceinline__ void load_ray(const NtrRay* __restrict__ rays, int rayIdx, RayRegs& r)
{
    const float4 o = reinterpret_cast<const float4*>(rays)[rayIdx * 2 + 0];
    const float4 d = reinterpret_cast<const float4*>(rays)[rayIdx * 2 + 1];
    r.ox = o.x; r.oy = o.y; r.oz = o.z; r.tmin = o.w;
    r.dx = d.x; r.dy = d.y; r.dz = d.z; r.tmax = d.w;
    r.rx = exact_rcp(d.x); r.ry = exact_rcp(d.y); r.rz = exact_rcp(d.z);
}

__device__ __forceinline__ void store_result(NtrRayResult* __restrict__ results, const int* __restrict__ triIndex,
                                             int rayIdx, int hitAddr, float t, float u, float v)
{
    int4 out;
    out.x = (hitAddr < 0) ? -1 : triIndex[hitAddr];
    out.y = __float_as_int(t);
    out.z = (hitAddr < 0) ? 0 : __float_as_int(u);
    out.w = (hitAddr < 0) ? 0 : __float_as_int(v);
    reinterpret_cast<int4*>(results)[rayIdx] = out;
}

// one inner node of trace<BVHLayout_Compact> (CudaBVH.cpp:721-775): both child boxes, nearer child first (ties -> child 0), the other pushed
template <bool FAST, int OCT, int LD = LDS_DEPTH, bool TRIM = false>
__device__ __forceinline__ void inner_advance(const float4& a, const float4& b, const float4& c, const float4& d, const RayRegs& r, int& node,
                                              LaneStack& st, int (&spill)[SPILL_DEPTH], unsigned int* status)
{
    float mn0, mx0, mn1, mx1;
    ray_box2<FAST, OCT>(r, a, b, c, mn0, mx0, mn1, mx1);
    const bool i0 = (mn0 <= mx0) && (mx0 >= r.tmin) && (mn0 <= r.tmax);
    const bool i1 = (mn1 <= mx1) && (mx1 >= r.tmin) && (mn1 <= r.tmax);
    const int c0 = __float_as_int(d.x), c1 = __float_as_int(d.y);
    const bool swp = i1 && (!i0 || mn0 > mn1);  // visit c1 first (ties -> c0, CudaBVH.cpp:761)
    const int nearC = swp ? c1 : c0, farC = swp ? c0 : c1;
    if (i0 && i1) stack_push<LD>(st, spill, farC, status);
    node = (i0 || i1) ? nearC : TRIM ? stack_pop_flat<LD>(st, spill) : stack_pop<LD>(st, spill);
}

// One inner-node step of trace<BVHLayout_Compact> (CudaBVH.cpp:721-775).  Executed by the whole
// wave; only lanes whose current node is an inner node (`inner`) update their state.
template <bool FAST>
__device__ __forceinline__ void inner_step(Rsrc nodes, bool inner, const RayRegs& r,
                                           int& node, LaneStack& st, int (&spill)[SPILL_DEPTH], unsigned int* status)
{
    // every lane fetches its own node (4 x 16 B; the quad-cooperative LDS-DMA fetch of rounds 1-2 was 1.2-3.7x slower in this loop:
    // scripts/studies/rejected_patches/coop_fetch.patch)
    const int ofs = inner ? node : kNoNode;
    const float4 n0 = ld4(nodes, ofs), n1 = ld4(nodes, ofs + kRowBytes), nz = ld4(nodes, ofs + 2 * kRowBytes);
    float4 nc = ld4(nodes, ofs + 3 * kRowBytes);   // (an 8-byte load of the two child words alone: 0.9 % slower, profiles/r03_ab_child_load_b64.jsonl)
    keep(nc);
    if (inner) inner_advance<FAST, 8>(n0, n1, nz, nc, r, node, st, spill, status);
}

// One triangle of a leaf: Intersect::RayTriangleWoop (Util.cpp:99-127) on its rows z, u4, v4 and updateHit (CudaBVH.cpp:1183-1225).
// Returns true when the hit is accepted: r.tmax, hitU and hitV are then its, and the caller records the triangle's row.
// The reference returns (t, u, v) for an accepted test and (FW_F32_MAX, 0, 0) for a missed one, and updateHit re-tests the returned t against
// (tmin, tmax) (CudaBVH.cpp:1200).  What that comes to, for every input:
//   accepted test: the returned t already passed t > tmin && t < tmax, so the re-test holds and the record is (t, u, v);
//   missed test:   the re-test is FLT_MAX > tmin && FLT_MAX < tmax.  FLT_MAX is the largest finite float, so the second half holds for
//                  tmax = +inf alone (a NaN on either side fails its compare): the missed test is then RECORDED at t = FLT_MAX, u = v = 0
//                  (the reference's quirk); for every other tmax nothing is recorded and ray and hit stay as they are.
// QUIRK = true states that as the reference does -- the miss values materialised, merged at the three exits and re-tested -- and is right for
// every ray.  QUIRK = false (the per-ray bodies, for a wave in which NO lane holds tmax = +inf: wave_may_quirk below) is the same function on
// those rays with the second case gone: a miss writes nothing, the accepted test writes its three values where it is accepted.  tmax only
// shrinks during a traversal (an accepted t is < tmax), so a wave that starts without +inf stays without.
template <bool QUIRK = true>
__device__ __forceinline__ bool triangle_step(const float4& z, const float4& u4, const float4& v4, RayRegs& r, float& hitU, float& hitV)
{
    const float Oz = z.w - r.ox * z.x - r.oy * z.y - r.oz * z.z;
    const float ooDz = 1.0f / dot4(z, r.dx, r.dy, r.dz, 0.0f);
    const float t = Oz * ooDz;
    if (!QUIRK) {
        bool hit = false;
        if (t > r.tmin && t < r.tmax) {
            const float u = dot4(u4, r.ox, r.oy, r.oz, 1.0f) + t * dot4(u4, r.dx, r.dy, r.dz, 0.0f);
            if (u >= 0.0f) {
                const float v = dot4(v4, r.ox, r.oy, r.oz, 1.0f) + t * dot4(v4, r.dx, r.dy, r.dz, 0.0f);
                if (v >= 0.0f && (u + v) <= 1.0f) { r.tmax = t; hitU = u; hitV = v; hit = true; }
            }
        }
        return hit;
    }
    float tt = FLT_MAX, uu = 0.0f, vv = 0.0f;  // miss -> bary[2] = FW_F32_MAX
    if (t > r.tmin && t < r.tmax) {
        const float u = dot4(u4, r.ox, r.oy, r.oz, 1.0f) + t * dot4(u4, r.dx, r.dy, r.dz, 0.0f);
        if (u >= 0.0f) {
            const float v = dot4(v4, r.ox, r.oy, r.oz, 1.0f) + t * dot4(v4, r.dx, r.dy, r.dz, 0.0f);
            if (v >= 0.0f && (u + v) <= 1.0f) { tt = t; uu = u; vv = v; }
        }
    }
    // updateHit re-tests the returned t, so with tmax = +inf a *missed* test
    // is recorded at t = FLT_MAX exactly like the reference (CudaBVH.cpp:1200).
    const bool hit = tt > r.tmin && tt < r.tmax;
    if (hit) { r.tmax = tt; hitU = uu; hitV = vv; }
    return hit;
}
// Whether some lane of the wave holds tmax = +inf (the one value at which a missed test is recorded): such a wave runs the QUIRK = true loop.
// Every lane votes, whatever it holds -- a finished or unused lane can only make the answer the careful one.
__device__ __forceinline__ bool wave_may_quirk(const RayRegs& r) { return __builtin_amdgcn_ballot_w64(!(r.tmax <= FLT_MAX)) != 0ull; }

// intersectTriangles<BVHLayout_Compact> + updateHit (CudaBVH.cpp:1084-1126, 1183-1225).
// Returns true when an any-hit ray terminates.
template <bool STATS>
__device__ __forceinline__ bool leaf_step(Rsrc woop, RayRegs& r, int leaf, bool anyHit, int& hitAddr,
                                          float& hitU, float& hitV, LaneStats& ls)
{
    for (int ofs = leaf_row(leaf) * kRowBytes;; ofs += kTriBytes) {
        const float4 z = ld4(woop, ofs);
        float4 u4 = ld4(woop, ofs + kRowBytes);      // past a terminator these may run off the
        float4 v4 = ld4(woop, ofs + 2 * kRowBytes);  // buffer: range-checked loads return 0
        unsigned int nextWord = ld1(woop, ofs + kTriBytes);
        keep(u4); keep(v4); keep(nextWord);           // one round trip per triangle, not four
        if (__float_as_uint(z.x) == kLeafTerm) {  // terminator (CudaBVH.cpp:1091)
            if (STATS) ls.leaves++;
            break;
        }
        if (STATS) ls.tris++;  // numTriangleTests (CudaBVH.cpp:1107-1111)

        const int row = ofs >> kRowShift;   // (formed ahead of the test: inside the branch hipcc gives the persistent while-while kernel 65 VGPRs for 62, a wave per SIMD)
        if (triangle_step(z, u4, v4, r, hitU, hitV)) {
            hitAddr = row;
            if (anyHit) return true;
        }
        if (nextWord == kLeafTerm) {  // the terminator was fetched with this triangle
            if (STATS) ls.leaves++;
            break;
        }
    }
    return false;
}

// unified_advance: the lane's ray takes the step its 64 bytes allow -- one inner node (trace<BVHLayout_Compact>, CudaBVH.cpp:721-775) or one
// triangle (intersectTriangles + updateHit, CudaBVH.cpp:1084-1126, 1183-1225).  TRIM: the per-ray bodies' pop (stack_pop_flat).  QUIRK: triangle_step's.
template <bool FAST, int OCT, int LD = LDS_DEPTH, bool TRIM = false, bool QUIRK = true>
__device__ __forceinline__ void unified_advance(const float4& a, const float4& b, const float4& c, const float4& d, RayRegs& r, int& node,
                                                LaneStack& st, int (&spill)[SPILL_DEPTH], bool anyHit, int& hitAddr, float& hitU, float& hitV,
                                                unsigned int* status)
{
    const bool inner = (unsigned)node < (unsigned)kSentinel;
    const bool atTri = node < 0;
    if (inner) {
        inner_advance<FAST, OCT, LD, TRIM>(a, b, c, d, r, node, st, spill, status);
    } else if (atTri) {
        bool leafDone = __float_as_uint(a.x) == kLeafTerm;   // terminator: an empty leaf
        if (!leafDone) {
            bool terminated = false;
            if (triangle_step<QUIRK>(a, b, c, r, hitU, hitV)) {
                hitAddr = leaf_row(node);
                terminated = anyHit;
            }
            if (terminated) node = kSentinel;
            else if (__float_as_uint(d.x) == kLeafTerm) leafDone = true;   // the terminator came with this triangle
            else node -= kTriRows;
        }
        if (leafDone) node = TRIM ? stack_pop_flat<LD>(st, spill) : stack_pop<LD>(st, spill);
    }
}

}  // namespace ntr
