// rt_reproject_kernels.h — launch interface of the reprojection kernel (rt_reproject.hip) for
// rt_post.cpp.  Internal; the public boundary is include/rt_reproject.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rtk {

// A workgroup covers kReprojectTileW x kReprojectTileH pixels: 2 x 2 waves of 16 x 4 each.
constexpr uint32_t kReprojectTileW = 32, kReprojectTileH = 8;

// Everything goes by value in the kernarg (128 bytes).
struct ReprojectParams {
    const float4* prev;        // the previous view's accumulator
    float4* dst;
    const uint32_t* prev_id;   // previous view: planes of rt_trace_aov
    const float4* prev_hit;
    const uint32_t* id;        // current view
    const float4* hit;
    const float4* normal;
    const float4* material;    // null: no material test (lambertian_only 0)
    uint32_t width, height;
    float r0[3], r1[3], r2[3]; // rt_reproject_basis' rows
    float o[3];                // the previous camera's centre
    float tol2;                // position_tolerance2
    float max_history;         // exact: max_history <= 2^24
};

hipError_t launch_reproject(const ReprojectParams& p, hipStream_t stream);

}  // namespace rtk
