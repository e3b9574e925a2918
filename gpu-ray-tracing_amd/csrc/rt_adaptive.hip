// rt_adaptive.hip — the kernel of rt_adaptive_error (include/rt_adaptive.h has the normative
// definition; DESIGN.md §4.10 the measurements).  A translation unit of its own, like
// rt_variance.hip: the render's kernels are not recompiled with it.
//
// Every float operation below is the one the header names, in its order: the build has
// -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical to the
// NumPy restatement in tests/test_adaptive.py.
#include <hip/hip_runtime.h>

#include "rt_adaptive_kernels.h"

namespace rtk {

// One lane per pixel: the count's word of the accumulator texel, one 16-byte load of the
// moments and one 4-byte store; consecutive lanes consecutive pixels.  A lane past the image
// does nothing.
__global__ __launch_bounds__(256) void rt_adaptive_error_kernel(const AdaptiveErrorParams p) {
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)p.width * p.height) return;
    const float n = p.image[at].w;
    const float4 m = p.moments[at];
    float d = m.y - m.x * m.x;
    d = d > 0.0f ? d : 0.0f;
    const float nn = n > 1.0f ? n : 1.0f;
    p.error[at] = m.w >= p.min_history ? d / nn : __builtin_inff();
}

hipError_t launch_adaptive_error(const AdaptiveErrorParams& p, hipStream_t stream) {
    const size_t px = (size_t)p.width * p.height;
    hipLaunchKernelGGL(rt_adaptive_error_kernel, dim3((uint32_t)((px + 255u) / 256u)), dim3(256),
                       0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
