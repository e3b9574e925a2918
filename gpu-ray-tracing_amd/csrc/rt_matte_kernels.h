// rt_matte_kernels.h — launch interface between rt_matte.cpp and rt_matte.hip (include/rt_matte.h).
// Internal; not part of the public boundary.  A header of its own, so that rt_kernels.h and the
// units that include it do not change with it.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace rtk {

constexpr uint32_t kMatteSlots = 4;              // RT_MATTE_SLOTS
constexpr uint32_t kMatteMaxFrames = 64;         // frames per launch: their seeds fit the kernarg
constexpr uint32_t kMatteListCap = 64;           // RT_MATTE_LIST_CAPACITY
// How a launch finds first hits: each tile's own index list with the per-frame culled scan as the
// fallback, that scan everywhere, or the reference's linear walk (RT_SCAN_EXHAUSTIVE).
constexpr uint32_t kMatteRouteList = 0, kMatteRouteScan = 1, kMatteRouteExhaustive = 2;

struct MatteParams {
    uint4* ids;            // the local planes (compact stripes), row pitch = width
    uint4* counts;
    uint2* tally;
    const float4* geom;    // the context's scan records (TraceParams::geom)
    uint32_t* info;        // rt_matte_info's four words, or null: this launch is not counted
    uint32_t width, height, count;
    uint32_t band_first, band_step;   // the planes' stripe map (local band j = global band first + j * step)
    uint32_t frames;       // 1..kMatteMaxFrames
    uint32_t reset_first;  // camera_has_moved > 0.5 applies to frame 0 only
    uint32_t route;
    float center[3], vul[3], pdu[3], pdv[3], ddu[3], ddv[3];
    float defocus_angle;
    uint32_t seed_b[kMatteMaxFrames];
};
// one wave per 8x8 tile of local bands [0, bands): four tiles of a band per workgroup
hipError_t launch_matte(const MatteParams& p, uint32_t bands, hipStream_t stream);

struct MatteResolveParams {
    const uint4* ids;
    const uint4* counts;
    const uint2* tally;
    const uint32_t* mask;  // bit i of the mask: id i is selected, for i < mask_bits
    uint32_t mask_bits;
    uint32_t background;   // 1: RT_AOV_MISS is selected
    uint64_t pixels;
    float* alpha;          // null = not wanted (not both)
    uint32_t* dominant;
};
hipError_t launch_matte_resolve(const MatteResolveParams& p, hipStream_t stream);

}  // namespace rtk
