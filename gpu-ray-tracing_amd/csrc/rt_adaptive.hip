// rt_adaptive.hip — the kernel of rt_adaptive_error (include/rt_adaptive.h has the normative
// definition; DESIGN.md §4.10 the measurements).  A translation unit of its own, like
// rt_variance.hip: the render's kernels are not recompiled with it.  (rt_update_adaptive's and
// rt_converge_frames' kernels trace rays: they are in rt_sampler.hip, over the tracer's device
// library.)
//
// Every float operation below is the one the header names, in its order (rt_pixel_rules.h): the
// build has -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical
// to the NumPy restatement in tests/test_adaptive.py.
#include <hip/hip_runtime.h>

#include "rt_adaptive_kernels.h"
#include "rt_pixel_rules.h"

namespace rtk {

// One lane per pixel: the count's word of the accumulator texel, one 16-byte load of the
// moments and one 4-byte store; consecutive lanes consecutive pixels.  A lane past the image
// does nothing.
__global__ __launch_bounds__(256) void rt_adaptive_error_kernel(const AdaptiveErrorParams p) {
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)p.width * p.height) return;
    const float n = p.image[at].w;
    const float4 m = p.moments[at];
    p.error[at] = gated_variance(m.x, m.y, m.w, n, p.min_history, __builtin_inff());
}

hipError_t launch_adaptive_error(const AdaptiveErrorParams& p, hipStream_t stream) {
    const size_t px = (size_t)p.width * p.height;
    hipLaunchKernelGGL(rt_adaptive_error_kernel, dim3((uint32_t)((px + 255u) / 256u)), dim3(256),
                       0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
