// rt_variance_kernels.h — launch interface of the moments and variance-guided filter kernels
// (rt_variance.hip) for rt_post.cpp.  Internal; the public boundary is include/rt_variance.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "rt_atrous_route.h"

namespace rtk {

struct MomentsParams {
    const float4* in;      // the update's input image
    const float4* out;     // the update's output image
    float4* moments;       // (m1, m2, 0, k), rewritten in place
    uint32_t width, height;
};

hipError_t launch_moments_update(const MomentsParams& p, hipStream_t stream);

struct VarianceParams {
    const float4* in;       // this iteration's input image
    float4* out;
    const float* vin;       // this iteration's input variance (unused when moments is set)
    float* vout;
    const float4* moments;  // iteration 0: v0 is computed from it and in[.].a; null afterwards
    const float4* hit;      // guide planes of rt_trace_aov
    const float4* normal;
    const uint32_t* id;     // null: no id test
    uint32_t width, height;
    uint32_t shift;         // log2 of the tap spacing
    uint32_t npow;          // the normal weight is squared this many times
    float il, ip;           // 1 / sigma_l^2, 1 / sigma_p^2
    float min_history;      // (float)min_history
    float fallback;         // fallback_variance
};

hipError_t launch_variance_filter(const VarianceParams& p, AtrousRoute route, hipStream_t stream);

}  // namespace rtk
