// rt_denoise_kernels.h — launch interface of the denoiser's kernels (rt_denoise.hip) for
// rt_post.cpp.  Internal; the public boundary is include/rt_denoise.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "rt_atrous_route.h"

namespace rtk {

struct DenoiseParams {
    const float4* in;      // this iteration's input image
    float4* out;
    const float4* hit;     // guide planes of rt_trace_aov
    const float4* normal;
    const uint32_t* id;    // null: no id test
    uint32_t width, height;
    uint32_t shift;        // log2 of the tap spacing
    uint32_t npow;         // the normal weight is squared this many times
    float ic, ip;          // this iteration's 1 / sigma_c^2 (clamped to FLT_MAX), 1 / sigma_p^2
};

hipError_t launch_denoise(const DenoiseParams& p, AtrousRoute route, hipStream_t stream);

}  // namespace rtk
