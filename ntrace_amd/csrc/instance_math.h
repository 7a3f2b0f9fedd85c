// instance_math.h -- the binary64 arithmetic of instance transforms, stated once for the host (ntr_instance_invert,
// ntr_instances_update_host) and the device (instances_update_kernels.hip): np_instanced.invert and np_instance_update.compose.
// Every product is rounded before the sum or difference that uses it: the library is compiled without contraction, and so must be
// whatever else includes this file.  Plain C++, no device runtime: a host-only translation unit may include it.
#pragma once

#if defined(__HIPCC__)
#define NTR_INSTANCE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NTR_INSTANCE_HD inline
#endif

namespace ntr {

// np_instanced.invert: worldToObject from objectToWorld, each of the 12 results rounded once.  false (and nothing written) for a zero or
// non-finite determinant.
NTR_INSTANCE_HD bool instance_invert(const float* f, float* worldToObject)
{
    const double m00 = f[0], m01 = f[1], m02 = f[2], t0 = f[3], m10 = f[4], m11 = f[5], m12 = f[6], t1 = f[7], m20 = f[8], m21 = f[9],
                 m22 = f[10], t2 = f[11];
    const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
    const double det = (m00 * c00 + m01 * c01) + m02 * c02;
    if (!(det - det == 0.0) || det == 0.0) return false;   // (det - det is NaN for an infinity and for a NaN)
    const double inv[3][3] = {{c00 / det, (m02 * m21 - m01 * m22) / det, (m01 * m12 - m02 * m11) / det},
                              {c01 / det, (m00 * m22 - m02 * m20) / det, (m02 * m10 - m00 * m12) / det},
                              {c02 / det, (m01 * m20 - m00 * m21) / det, (m00 * m11 - m01 * m10) / det}};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) worldToObject[4 * r + c] = (float)inv[r][c];
        worldToObject[4 * r + 3] = (float)-((inv[r][0] * t0 + inv[r][1] * t1) + inv[r][2] * t2);
    }
    return true;
}

// np_instance_update.compose: acc = acc * l as 3x4 affine maps (l applied first), l a binary32 matrix widened exactly
NTR_INSTANCE_HD void instance_compose(double* acc, const float* l)
{
    double w[12];
    for (int r = 0; r < 3; r++) {
        const double p0 = acc[4 * r], p1 = acc[4 * r + 1], p2 = acc[4 * r + 2], p3 = acc[4 * r + 3];
        for (int c = 0; c < 3; c++) w[4 * r + c] = (p0 * (double)l[c] + p1 * (double)l[4 + c]) + p2 * (double)l[8 + c];
        w[4 * r + 3] = ((p0 * (double)l[3] + p1 * (double)l[7]) + p2 * (double)l[11]) + p3;
    }
    for (int k = 0; k < 12; k++) acc[k] = w[k];
}

// the message of both forms of the update when a status bit is set: function, first bad instance, count, bits
constexpr const char* kInstanceBadFormat =
    "%s: instance %u is the first of %u bad instances (status bits 0x%x: 1 a zero or non-finite determinant, 2 a node or parent index "
    "outside the nodes or a chain of more than 16 transforms); a bad instance's worldToObject is zero, every other instance was written";

}  // namespace ntr
