// rt_edit_kernels.h — launch interface of the scene-edit carry kernel (rt_edit.hip) for
// rt_scene_edit.cpp.  Internal; the public boundary is include/rt_scene_edit.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rtk {

// rt_reproject_kernel's mapping: a workgroup covers kEditTileW x kEditTileH pixels, 2 x 2 waves
// of 16 x 4 each.
constexpr uint32_t kEditTileW = 32, kEditTileH = 8;

// Everything goes by value in the kernarg (144 bytes, and the plan's pointer beside it).
struct EditParams {
    const float4* prev;        // the previous frame's accumulator
    float4* dst;
    const uint32_t* prev_id;   // previous scene and view: planes of rt_trace_aov
    const float4* prev_hit;
    const uint32_t* id;        // current scene and view
    const float4* hit;
    const float4* normal;
    const float4* material;    // null: no material test (lambertian_only 0)
    uint32_t width, height;
    float r0[3], r1[3], r2[3]; // rt_reproject_basis' rows
    float o[3];                // the previous camera's centre
    float tol2;                // position_tolerance2
    float max_history;         // exact: max_history <= 2^24
    float edit_history;        // exact likewise
    uint32_t n_records;        // plan: 2 float4 per record, then 2 float4 per ball
    uint32_t n_balls;          // <= RT_EDIT_MAX_BALLS
    uint32_t _pad;
};

// `plan` is the device copy of rt_edit_plan's table (null only with no records and no balls).
hipError_t launch_edit_carry(const EditParams& p, const float4* plan, hipStream_t stream);

}  // namespace rtk
