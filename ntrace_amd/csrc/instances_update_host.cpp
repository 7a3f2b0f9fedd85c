// instances_update_host.cpp -- ntr_instances_update_host: the instance update's rule (tests/np_instance_update.py) over host arrays.
// Plain C++ with no device call: what csrc/instances_update_kernels.hip computes, restated for callers without a device and as the
// thing the kernel is compared with.  The arithmetic is instance_math.h's, which ntr_instance_invert and the kernel use as well; it
// needs a build without contraction, which the library's flags give.
#include <stdint.h>
#include <string.h>

#include "ntrace_amd.h"
#include "instance_math.h"

namespace ntr {
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));   // ntr_internal.h, without its device headers
}

using namespace ntr;

extern "C" int ntr_instances_update_host(int32_t numNodes, const float* nodeLocal, const int32_t* nodeParent, int32_t numInstances,
                                         const int32_t* instanceNode, const int32_t* blas, NtrInstance* out, uint32_t status[4])
{
    const char* fn = "ntr_instances_update_host";
    if (!nodeLocal || !blas || !out || !status) return set_error(NTR_ERR_INVALID, "%s: null argument", fn);
    if (numInstances < 1 || numNodes < 1) return set_error(NTR_ERR_INVALID, "%s: numInstances < 1 or numNodes < 1", fn);
    if (!instanceNode && numNodes < numInstances)
        return set_error(NTR_ERR_INVALID, "%s: without instanceNode instance i uses node i: numNodes %d < numInstances %d", fn, (int)numNodes,
                         (int)numInstances);
    uint32_t bits = 0u, first = 0xFFFFFFFFu, count = 0u;
    for (int32_t i = 0; i < numInstances; i++) {
        NtrInstance& o = out[i];
        memset(&o, 0, sizeof(o));
        o.blas = blas[i];
        // upward: path[0] the instance's own node ... path[len - 1] the root
        int32_t path[NTR_INSTANCE_MAX_CHAIN];
        int len = 0;
        int32_t k = instanceNode ? instanceNode[i] : i;
        uint32_t bad = (k < 0 || k >= numNodes) ? NTR_INSTANCE_ERR_CHAIN : 0u;
        while (!bad) {
            path[len++] = k;
            const int32_t p = nodeParent ? nodeParent[k] : -1;
            if (p == -1) break;
            if (p < 0 || p >= numNodes || len == NTR_INSTANCE_MAX_CHAIN) bad = NTR_INSTANCE_ERR_CHAIN;
            k = p;
        }
        if (!bad) {
            double acc[12];
            for (int j = len - 1; j >= 0; j--) {
                const float* l = nodeLocal + 12 * (size_t)path[j];
                if (j == len - 1)
                    for (int c = 0; c < 12; c++) acc[c] = (double)l[c];
                else
                    instance_compose(acc, l);
            }
            for (int c = 0; c < 12; c++) o.objectToWorld[c] = (float)acc[c];
            if (!instance_invert(o.objectToWorld, o.worldToObject)) bad = NTR_INSTANCE_ERR_SINGULAR;   // (worldToObject stays twelve +0)
        }
        if (bad) {
            bits |= bad;
            if (first == 0xFFFFFFFFu) first = (uint32_t)i;
            count++;
        }
    }
    status[0] = bits;
    status[1] = first;
    status[2] = count;
    status[3] = 0u;
    if (bits) return set_error(NTR_ERR_INVALID, kInstanceBadFormat, fn, first, count, bits);
    return NTR_OK;
}
