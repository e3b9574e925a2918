// rt_adaptive_kernels.h — launch interface of rt_adaptive_error's kernel (rt_adaptive.hip) for
// rt_post.cpp.  Internal; the public boundary is include/rt_adaptive.h.  (The sampler's kernels
// trace rays and live in rt_sampler.hip, over rt_trace_device.h: rt_kernels.h, launch_adaptive.)
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rtk {

struct AdaptiveErrorParams {
    const float4* image;    // the accumulator: .w is the sample count
    const float4* moments;  // (m1, m2, 0, k)
    float* error;           // width * height floats
    uint32_t width, height;
    float min_history;      // (float)min_history
};

hipError_t launch_adaptive_error(const AdaptiveErrorParams& p, hipStream_t stream);

}  // namespace rtk
