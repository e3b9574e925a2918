// rt_resize_kernels.h — launch interface of the resize-carry kernel (rt_resize.hip) for
// rt_resize.cpp.  Internal; the public boundary is include/rt_resize.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rtk {

// rt_reproject_kernel's mapping: a workgroup covers kResizeTileW x kResizeTileH pixels of the
// current image, 2 x 2 waves of 16 x 4 each.
constexpr uint32_t kResizeTileW = 32, kResizeTileH = 8;

// Everything goes by value in the kernarg (208 bytes).
struct ResizeParams {
    const float4* prev;        // the previous view's accumulator, prev_width x prev_height
    float4* dst;               // width x height
    const float4* prev2;       // the second pair: both null or both set
    float4* dst2;
    const uint32_t* prev_id;   // previous view: planes of rt_trace_aov
    const float4* prev_hit;
    const uint32_t* id;        // current view
    const float4* hit;
    const float4* normal;
    const float4* material;    // null: no material test (lambertian_only 0)
    uint32_t width, height;
    uint32_t prev_width, prev_height;
    float r0[3], r1[3], r2[3]; // rt_reproject_basis' rows
    float o[3];                // the previous camera's centre
    float tol2;                // position_tolerance2
    float max_history;         // exact: max_history <= 2^24
    uint32_t sky, fill;        // 0 / 1 each
    float center[3], vul[3], pdu[3], pdv[3];   // the current camera's ray grid (sky || fill)
};

hipError_t launch_resize_carry(const ResizeParams& p, hipStream_t stream);

}  // namespace rtk
