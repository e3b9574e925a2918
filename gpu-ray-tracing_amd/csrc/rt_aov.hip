// rt_aov.hip — the first-hit G-buffer kernel of rt_trace_aov and rt_pick (include/rt_aov.h has
// the normative definition).  A translation unit of its own over the tracer's device library
// (rt_trace_device.h), built with the render kernels' flags: the render kernels' compile unit
// (rt_kernels.hip) does not change with it.
#include "rt_trace_device.h"

namespace rtk {

// ---- First-hit G-buffer (rt_aov.h) ---------------------------------------------------
//
// One wave per 8x8 tile, lanes row-major inside the tile and the packed stripe map of
// rt_trace_kernel (tile_coord).  Each lane traces the ray through its pixel's centre from
// camera.center — get_ray (wgsl:305-325) with both offsets 0 and no lens — with the exact
// scans of the progressive render, and writes the winner's hit record (wgsl:205-218) out
// instead of shading it.  Culling is the per-wave cone over the uploaded records
// (scan_culled with bounce = false: scenes under kCullMinSpheres and degenerate or non-finite
// waves walk the whole list); the per-tile candidate lists carry no sphere index and belong to
// the render's camera, so they are not read.  Lanes outside the image are not live for the
// cone's reductions and store nothing.  The normal is the plain IEEE (p - C) / R: three
// divisions per pixel beside a scan, and valid for every radius.
__global__ __launch_bounds__(256) void rt_aov_kernel(const AovParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tx = p.tx0 + blockIdx.x * (blockDim.x >> 6) + wave;
    if (tx >= tiles_x) return;                                    // whole wave exits
    const TileCoord tc = tile_coord(p.width, p.height, p.bands & 0xFFFFu,
                                    (p.bands >> 16) & 0x7FFFu, tx, blockIdx.y, lane);
    const bool live = tc.valid;
    const v3 o = mk(p.center[0], p.center[1], p.center[2]);
    const float sx = (float)tc.x + 0.5f, sy = (float)tc.y + 0.5f;
    const v3 pc = fmas(sy, mk(p.pdv[0], p.pdv[1], p.pdv[2]),
                       fmas(sx, mk(p.pdu[0], p.pdu[1], p.pdu[2]),
                            mk(p.vul[0], p.vul[1], p.vul[2])));
    const v3 d = sub(pc, o);
    Hit h;
    if (p.culled) {
        const GridP none = {};                                    // (bounce rays only)
        h = scan_culled<false>(none, p.geom, p.count, o, d, live, false);
    } else {
        h = scan_exhaustive<RT_SCAN_CHUNK>(p.geom, p.count, o, d);
    }
    const bool hit = live && h.idx >= 0;
    float4 pr = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mat = pr;
    if (hit) {
        pr = p.sph[2 * h.idx];                                    // position, radius
        mat = p.sph[2 * h.idx + 1];                               // material color
    }
    const v3 hp = fmas(h.t, d, o);                                // wgsl:205
    const v3 outward = divs(sub(hp, mk(pr.x, pr.y, pr.z)), pr.w); // wgsl:206
    const bool front = dot(d, outward) < 0.0f;                    // wgsl:159-160
    const v3 n = sel3(front, outward, neg(outward));
    // which planes are wanted is wave-uniform: a plane not wanted costs no store
    const bool store = p.pick ? lane + 1u == p.pick : live;
    const size_t at = p.pick ? 0 : tc.idx;
    if (!store) return;
    if (p.id) p.id[at] = hit ? (uint32_t)h.idx : 0xFFFFFFFFu;
    if (p.hit)
        p.hit[at] = hit ? make_float4(hp.x, hp.y, hp.z, h.t)
                        : make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
    if (p.normal)
        p.normal[at] = hit ? make_float4(n.x, n.y, n.z, front ? 1.0f : 0.0f)
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.material) p.material[at] = mat;
}

hipError_t launch_aov(const AovParams& p, uint32_t tiles_x, uint32_t bands, hipStream_t stream) {
    if (tiles_x == 0 || bands == 0) return hipSuccess;
    // four tiles of a band per workgroup, as rt_trace_kernel; a lone tile (rt_pick) is one wave
    const uint32_t waves = tiles_x == 1u ? 1u : 4u;
    hipLaunchKernelGGL(rt_aov_kernel, dim3((tiles_x + waves - 1u) / waves, bands),
                       dim3(64u * waves), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
