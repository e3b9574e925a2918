// rt_query.hip — the ray-query kernel of rt_cast_rays and rt_cast_ray (include/rt_query.h has
// the normative definition).  A translation unit of its own over the tracer's device library
// (rt_trace_device.h: its scans take the ray's bound as their seed and, for occlusion, leave at
// the first acceptance), built with the render kernels' flags.
#include "rt_trace_device.h"

#include "rt_query_kernels.h"

namespace rtk {

__device__ __forceinline__ GridP query_grid_params(const QueryParams& p) {
    GridP g;
    g.roots_fast = p.grid.roots_fast;
    g.cells = p.grid.cells;
    g.geom = p.grid.geom;
    g.items = p.grid.items;
    g.big = p.grid.big;
    g.sgeom = p.geom;
    g.nx = p.grid.nx;
    g.nz = p.grid.nz;
    g.nbig = p.grid.nbig;
    g.x0 = p.grid.x0;
    g.z0 = p.grid.z0;
    g.s = p.grid.s;
    g.inv_s = p.grid.inv_s;
    g.ylo = p.grid.ylo;
    g.yhi = p.grid.yhi;
    g.cx = p.grid.cx;
    g.cy = p.grid.cy;
    g.cz = p.grid.cz;
    g.reach = p.grid.reach;
    g.m = p.grid.m;
    g.e = p.grid.e;
    return g;
}

// One lane per ray, 64 consecutive rays per wave.  A lane past `count` is not live: it traces a
// copy of the last ray (so that it adds no ray of its own to the wave's cone or walk), stays out
// of the ballots and stores nothing.  The wave's route is the library's bounce-ray rule
// (scan_culled with bounce = true): the grid where grid_usable allows it, else the cone where
// wave_cone finds one, else the exhaustive walk — each from the ray's bound T (t_seed).
// kOcc: RT_QUERY_OCCLUSION (one word per ray, the scans leave at the first acceptance).
template <bool kOcc>
__global__ __launch_bounds__(256) void rt_query_kernel(const QueryParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t first = ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave) * 64u;
    if (first >= p.count) return;                                 // whole wave exits
    const uint64_t at = first + lane;
    const bool live = at < p.count;
    float4 r0, r1;
    if (p.rays) {
        const uint64_t src = live ? at : p.count - 1u;
        r0 = p.rays[2u * src];                                    // o, tmax
        r1 = p.rays[2u * src + 1u];                               // d, reserved
    } else {
        r0 = p.one[0];
        r1 = p.one[1];
    }
    const v3 o = mk(r0.x, r0.y, r0.z), d = mk(r1.x, r1.y, r1.z);
    const float T = r0.w < 0x1.05ed2ep+118f ? r0.w : 0x1.05ed2ep+118f;   // NaN, inf -> 3.4e35
    Hit h;
    uint32_t route = kRouteExhaustive;
    if (p.culled)
        h = scan_culled<false, kOcc>(query_grid_params(p), p.geom, p.spheres, o, d, live, true, T,
                                     &route);
    else
        h = scan_exhaustive<RT_SCAN_CHUNK, false, true, kOcc>(p.geom, p.spheres, o, d, T, live);
    if (p.routes && lane == 0u) atomicAdd(&p.routes[route], 1u);
    const bool hit = live && h.idx >= 0;
    if (kOcc) {
        if (live) p.occluded[at] = hit ? 1u : 0u;
        return;
    }
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
    if (!live) return;
    if (p.id) p.id[at] = hit ? (uint32_t)h.idx : 0xFFFFFFFFu;
    if (p.hit)
        p.hit[at] = hit ? make_float4(hp.x, hp.y, hp.z, h.t)
                        : make_float4(0.0f, 0.0f, 0.0f, __builtin_inff());
    if (p.normal)
        p.normal[at] = hit ? make_float4(n.x, n.y, n.z, front ? 1.0f : 0.0f)
                           : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.material) p.material[at] = mat;
}

hipError_t launch_query(const QueryParams& p, hipStream_t stream) {
    if (p.count == 0) return hipSuccess;
    const uint64_t waves = (p.count + 63u) / 64u;
    const uint32_t per = waves == 1u ? 1u : kQueryWaves;
    const dim3 grid((uint32_t)((waves + per - 1u) / per)), block(64u * per);
    if (p.occluded)
        hipLaunchKernelGGL(rt_query_kernel<true>, grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL(rt_query_kernel<false>, grid, block, 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
