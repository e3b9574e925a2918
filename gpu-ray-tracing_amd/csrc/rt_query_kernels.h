// rt_query_kernels.h — launch interface between rt_query.cpp and rt_query.hip (include/rt_query.h:
// rt_cast_rays, rt_cast_ray).  Internal; rt_kernels.h stays as it is.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace rtk {

constexpr uint32_t kQueryWaves = 4;          // waves (64 rays each) per workgroup

// The context's XZ sphere grid as the scans take it (rt_trace_device.h GridP, field for field;
// nx == 0: no grid).
struct QueryGrid {
    const uint2* cells;
    const float4* geom;
    const uint32_t* items;
    const uint32_t* big;
    uint32_t nx, nz, nbig;
    float x0, z0, s, inv_s, ylo, yhi, cx, cy, cz, reach, m, e;
    uint32_t roots_fast;     // the scene's |C| + |R| stay within 2^40 (TraceParams::roots_fast)
};

struct QueryParams {
    // rays: count records of 32 bytes, (o, tmax) then (d, reserved); null: the one ray `one`
    // (rt_cast_ray: count 1, its record to element 0 of each plane)
    const float4* rays;
    uint64_t count;
    uint32_t* id;            // the planes of rt_query_planes; null = not wanted
    float4* hit;
    float4* normal;
    float4* material;
    uint32_t* occluded;      // non-null: RT_QUERY_OCCLUSION (the four above are null)
    uint32_t* routes;        // route_counts, or null
    const float4* geom;      // the context's scan records and sphere records (TraceParams)
    const float4* sph;
    uint32_t spheres;
    uint32_t culled;         // 1: grid / cone / exhaustive per wave (RT_SCAN_CULLED), 0: exhaustive
    QueryGrid grid;
    float4 one[2];
};

// ceil(count / 64) waves, kQueryWaves per workgroup (a lone wave is a one-wave workgroup)
hipError_t launch_query(const QueryParams& p, hipStream_t stream);

}  // namespace rtk
