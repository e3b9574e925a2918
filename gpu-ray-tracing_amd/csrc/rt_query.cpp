// rt_query.cpp — C-ABI entry points of include/rt_query.h: the argument checks and the launch of
// the ray-query kernel (rt_query.hip).  Of the context they use the device, the scan mode, the
// uploaded sphere records with the grid built from them (rti::upload_spheres: the upload every
// trace call does) and rt_pick's record slots; candidate lists, orders, sample-count records,
// launch info and timing events are not touched.
#include <hip/hip_runtime_api.h>

#include <cstring>

#include "rt_internal.h"
#include "rt_query.h"
#include "rt_query_kernels.h"

namespace {

using rti::DeviceGuard;
using rti::fail;
using rti::hip_fail;

static_assert(sizeof(rt_ray) == 32 && sizeof(rt_query_planes) == 40,
              "rt_query.h's structs are two float4 and five pointers");
static_assert(sizeof(rt_ray) == sizeof(rtk::QueryParams::one), "the kernel's inline ray is rt_ray");

constexpr uint64_t kMaxRays = (1ull << 32) - 64u;   // one grid row of four-wave workgroups

// The scene half of a launch's parameters: the records, the scan mode and the context's grid
// (build_grid, at every upload: a context that has never rendered has it too).
void fill_scene(const rt_ctx* ctx, uint32_t count, rtk::QueryParams& p) {
    p.geom = ctx->d_geom;
    p.sph = ctx->d_sph;
    p.spheres = count;
    p.culled = ctx->scan_mode == RT_SCAN_CULLED ? 1u : 0u;
    const rt_ctx::Grid& g = ctx->grid;
    if (!p.culled || !g.nx || !ctx->d_grid) return;
    const unsigned char* base = static_cast<const unsigned char*>(ctx->d_grid);
    const size_t cells = (size_t)g.nx * g.nz;
    const size_t geom_off = (cells * 8 + 15) & ~(size_t)15;     // as build_grid
    rtk::QueryGrid& q = p.grid;
    q.cells = reinterpret_cast<const uint2*>(base);
    q.geom = reinterpret_cast<const float4*>(base + geom_off);
    q.items = reinterpret_cast<const uint32_t*>(base + geom_off + g.items * 16ull);
    q.big = q.items + g.items;
    q.nx = g.nx;
    q.nz = g.nz;
    q.nbig = g.nbig;
    q.x0 = g.x0;
    q.z0 = g.z0;
    q.s = g.s;
    q.inv_s = g.inv_s;
    q.ylo = g.ylo;
    q.yhi = g.yhi;
    q.cx = g.cx;
    q.cy = g.cy;
    q.cz = g.cz;
    q.reach = g.reach;
    q.m = g.m;
    q.e = g.e;
    q.roots_fast = ctx->scene_bound <= 0x1p40 ? 1u : 0u;
}

}  // namespace

extern "C" {

rt_status rt_cast_rays(rt_ctx* ctx, const rt_ray* rays, uint64_t count, uint32_t mode,
                       const rt_query_planes* planes, const rt_sphere* spheres,
                       uint32_t sphere_count, uint32_t* route_counts, void* stream_v) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!rays && count > 0u) return fail(RT_ERR_INVALID_ARGUMENT, "rays is NULL with count > 0");
    if (!planes) return fail(RT_ERR_INVALID_ARGUMENT, "planes is NULL");
    if (mode > RT_QUERY_OCCLUSION) return fail(RT_ERR_INVALID_ARGUMENT, "mode above 1");
    const bool record = planes->sphere_id || planes->hit || planes->normal || planes->material;
    if (mode == RT_QUERY_OCCLUSION ? (record || !planes->occluded) : (!record || planes->occluded))
        return fail(RT_ERR_INVALID_ARGUMENT,
                    mode == RT_QUERY_OCCLUSION
                        ? "an occlusion query takes the occluded plane and no other"
                        : "a closest-hit query takes a record plane and not the occluded plane");
    if (!spheres && sphere_count > 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "spheres is NULL with sphere_count > 0");
    if (count > kMaxRays) return fail(RT_ERR_INVALID_SIZE, "count above 2^32 - 64");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (rt_status s = rti::upload_spheres(ctx, spheres, sphere_count, stream)) return s;
    if (count == 0u) return RT_OK;
    rtk::QueryParams p;
    std::memset(&p, 0, sizeof(p));
    p.rays = reinterpret_cast<const float4*>(rays);
    p.count = count;
    p.id = planes->sphere_id;
    p.hit = reinterpret_cast<float4*>(planes->hit);
    p.normal = reinterpret_cast<float4*>(planes->normal);
    p.material = reinterpret_cast<float4*>(planes->material);
    p.occluded = planes->occluded;
    p.routes = route_counts;
    fill_scene(ctx, sphere_count, p);
    hipError_t e = rtk::launch_query(p, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_query_kernel launch");
    return RT_OK;
}

rt_status rt_cast_ray(rt_ctx* ctx, const rt_ray* ray, const rt_sphere* spheres,
                      uint32_t sphere_count, void* stream_v, rt_pick_result* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!ray || !out) return fail(RT_ERR_INVALID_ARGUMENT, "ray or out is NULL");
    if (!spheres && sphere_count > 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "spheres is NULL with sphere_count > 0");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    // rt_pick's record on the device serves: the ray itself travels in the kernel arguments
    if (!ctx->d_pick) {
        hipError_t e = hipMalloc(&ctx->d_pick, 4 * sizeof(float4));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(pick record)");
    }
    if (rt_status s = rti::upload_spheres(ctx, spheres, sphere_count, stream)) return s;
    rtk::QueryParams p;
    std::memset(&p, 0, sizeof(p));
    p.count = 1u;
    p.id = reinterpret_cast<uint32_t*>(ctx->d_pick);
    p.hit = ctx->d_pick + 1;
    p.normal = ctx->d_pick + 2;
    p.material = ctx->d_pick + 3;
    std::memcpy(p.one, ray, sizeof(*ray));
    fill_scene(ctx, sphere_count, p);
    hipError_t e = rtk::launch_query(p, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_query_kernel launch");
    float rec[16];
    e = hipMemcpyAsync(rec, ctx->d_pick, sizeof(rec), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "rt_cast_ray read-back");
    std::memcpy(&out->sphere_id, &rec[0], sizeof(uint32_t));
    out->t = rec[7];
    for (int i = 0; i < 3; ++i) {
        out->p[i] = rec[4 + i];
        out->normal[i] = rec[8 + i];
    }
    out->front_face = rec[11] != 0.0f ? 1u : 0u;
    for (int i = 0; i < 4; ++i) out->color[i] = rec[12 + i];
    return RT_OK;
}

}  // extern "C"
