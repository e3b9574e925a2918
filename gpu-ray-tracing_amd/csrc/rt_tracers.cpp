// rt_tracers.cpp — C-ABI entry points of the trace launches beside the render, each over
// prepare() or the scene upload alone: the first-hit G-buffer and pick (include/rt_aov.h,
// rt_aov.hip), the adaptive sampler and its fused rounds (rt_adaptive.h's rt_update_adaptive,
// rt_converge.h; rt_sampler.hip).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>

#include "rt_adaptive.h"
#include "rt_aov.h"
#include "rt_converge.h"
#include "rt_internal.h"
#include "rt_kernels.h"

namespace {

using namespace rti;

// Shared body of rt_trace_aov / rt_trace_aov_bands / rt_pick (rt_aov.h): argument checks and
// scene upload as prepare(), then one rt_aov_kernel launch over the band set — or, for a pick
// (pick_lane != 0), over the one tile (tx0, bs.first).  Of the context's state it touches the
// sphere records alone: no candidate lists, orders, counts, launch info or timing events.
rt_status trace_aov(rt_ctx* ctx, const rt_aov_planes* planes, uint32_t w, uint32_t h,
                    const rt_band_set& bs, const rt_scene_camera* cam, const rt_sphere* spheres,
                    uint32_t count, hipStream_t stream, uint32_t tx0, uint32_t pick_lane) {
    if (!planes || !cam) return fail(RT_ERR_INVALID_ARGUMENT, "NULL planes or camera");
    if (!planes->sphere_id && !planes->hit && !planes->normal && !planes->material)
        return fail(RT_ERR_INVALID_ARGUMENT, "no plane requested");
    if (rt_status s = check_image(w, h)) return s;
    if (rt_status s = check_band_set(h, bs)) return s;
    if (rt_status s = upload_spheres(ctx, spheres, count, stream)) return s;
    if (bs.count == 0) return RT_OK;
    rtk::AovParams p;
    std::memset(&p, 0, sizeof(p));
    p.id = planes->sphere_id;
    p.hit = reinterpret_cast<float4*>(planes->hit);
    p.normal = reinterpret_cast<float4*>(planes->normal);
    p.material = reinterpret_cast<float4*>(planes->material);
    p.geom = ctx->d_geom;
    p.sph = ctx->d_sph;
    p.width = w;
    p.height = h;
    p.count = count;
    p.bands = rtk::pack_bands(bs.first, bs.step, false);
    p.tx0 = tx0;
    p.culled = ctx->scan_mode == RT_SCAN_CULLED ? 1u : 0u;
    p.pick = pick_lane;
    fill_camera_grid(p, *cam);
    const uint32_t tiles_x = pick_lane ? 1u : (w + 7u) >> 3;
    hipError_t e = rtk::launch_aov(p, tiles_x, bs.count, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_aov_kernel launch");
    return RT_OK;
}

// The instance of rt_adaptive_kernel / rt_converge_kernel for a prepared launch: the context's
// as trace_kernel_for chooses it, with ray_color's culled scans in place of the bounce instance
// at max_depth >= 2.  The culled scans read the records from L2: no LDS copy.
int adaptive_kernel_for(const rt_ctx* ctx, rtk::TraceParams& p) {
    p.lds_records = 0u;
    const int auto_kernel = trace_kernel_for(ctx, p);
    return auto_kernel == rtk::kTraceBounce ? rtk::kTraceCulled : auto_kernel;
}

// Shared body of rt_update_adaptive / rt_update_adaptive_bands (rt_adaptive.h): the argument
// checks, then prepare() as every trace launch (scene upload, hash tables, candidate lists) and
// one rt_adaptive_kernel launch over the band set.  The instance follows the context as
// trace_kernel_for does, with ray_color's culled scans in place of the bounce instance at
// max_depth >= 2.  No hint, no tile order, no cost recording, no launch info.
rt_status update_adaptive(rt_ctx* ctx, const float* in, float* out, const float* error,
                          uint64_t* tile_mask, uint32_t w, uint32_t h, const rt_band_set& bs,
                          const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                          const rt_adaptive_params* params, void* stream_v) {
    if (!in || !out || !error || !cam || !params)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL in_rgba, out_rgba, error, camera or params");
    if (out == in || static_cast<const void*>(out) == error ||
        static_cast<const void*>(out) == tile_mask)
        return fail(RT_ERR_INVALID_ARGUMENT, "out_rgba is in_rgba, error or tile_mask");
    if (rt_status s = check_adaptive_params(*params)) return s;
    if (rt_status s = check_image(w, h)) return s;
    if (rt_status s = check_band_set(h, bs)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    const float seed = cam->random_seed;
    rtk::TraceParams p;
    if (rt_status s = prepare(ctx, in, out, w, h, bs, cam, spheres, count, &seed, stream, p))
        return s;
    if (bs.count == 0) return RT_OK;
    p.in = reinterpret_cast<const float4*>(in);
    p.out = reinterpret_cast<float4*>(out);
    p.frames = 1u;
    p.reset_first = cam->camera_has_moved > 0.5f ? 1u : 0u;
    fill_seeds(p.seed_b, &seed, 1u);
    const int kernel = adaptive_kernel_for(ctx, p);
    rtk::AdaptiveParams a;
    a.error = error;
    a.tile_mask = tile_mask;
    a.min_samples = params->min_samples;
    a.abs_tolerance2 = params->abs_tolerance2;
    a.rel_tolerance2 = params->rel_tolerance2;
    forget_count(ctx, out);          // the counts now differ per pixel
    hipError_t e = rtk::launch_adaptive(p, a, kernel, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_adaptive_kernel launch");
    return RT_OK;
}

// Shared body of rt_converge_frames / rt_converge_frames_bands (rt_converge.h): the argument
// checks, prepare() as update_adaptive, then one rt_converge_kernel launch per
// RT_CONVERGE_MAX_FRAMES_PER_LAUNCH frames, in order on the caller's stream, with the seeds
// converted as rt_update_frames converts them.  The same instance choice, and like
// update_adaptive no hint, no tile order, no cost recording, no launch info.
static_assert(rtk::kConvergeMaxFrames == RT_CONVERGE_MAX_FRAMES_PER_LAUNCH,
              "the kernel's frames per launch are the header's");
rt_status converge_frames(rt_ctx* ctx, float* image, float* moments, float* error,
                          uint64_t* tile_mask, uint32_t* tile_samples, uint32_t w, uint32_t h,
                          const rt_band_set& bs, const rt_scene_camera* cam,
                          const rt_sphere* spheres, uint32_t count, uint32_t frames,
                          const float* seeds, const rt_adaptive_params* params,
                          uint32_t min_history, void* stream_v) {
    if (!image || !moments || !cam || !params || !seeds)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "NULL image, moments, camera, params or random_seeds");
    const void* const bufs[5] = {image, moments, error, tile_mask, tile_samples};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (bufs[i] && bufs[i] == bufs[j])
                return fail(RT_ERR_INVALID_ARGUMENT,
                            "two of image, moments, error, tile_mask and tile_samples are equal");
    if (frames == 0u || frames > 65536u)
        return fail(RT_ERR_INVALID_ARGUMENT, "frames outside 1..65536");
    if (min_history == 0u || min_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "min_history outside 1..16777216");
    if (rt_status s = check_adaptive_params(*params)) return s;
    if (rt_status s = check_image(w, h)) return s;
    if (rt_status s = check_band_set(h, bs)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rtk::TraceParams p;
    if (rt_status s = prepare(ctx, image, image, w, h, bs, cam, spheres, count, seeds, stream, p))
        return s;
    if (bs.count == 0) return RT_OK;
    p.in = reinterpret_cast<const float4*>(image);
    p.out = reinterpret_cast<float4*>(image);
    const int kernel = adaptive_kernel_for(ctx, p);
    rtk::ConvergeParams a;
    a.moments = reinterpret_cast<float4*>(moments);
    a.error = error;
    a.tile_mask = tile_mask;
    a.tile_samples = tile_samples;
    a.min_samples = params->min_samples;
    a.abs_tolerance2 = params->abs_tolerance2;
    a.rel_tolerance2 = params->rel_tolerance2;
    a.min_history = (float)min_history;
    forget_count(ctx, image);        // the counts now differ per pixel
    for (uint32_t f0 = 0; f0 < frames; f0 += rtk::kConvergeMaxFrames) {
        const uint32_t nf = std::min(frames - f0, rtk::kConvergeMaxFrames);
        p.frames = nf;
        p.reset_first = (f0 == 0u && cam->camera_has_moved > 0.5f) ? 1u : 0u;
        fill_seeds(p.seed_b, seeds + f0, nf);
        a.first = f0 == 0u ? 1u : 0u;
        hipError_t e = rtk::launch_converge(p, a, kernel, stream);
        if (e != hipSuccess) return hip_fail(e, "rt_converge_kernel launch");
    }
    return RT_OK;
}

}  // namespace

extern "C" {

rt_status rt_trace_aov_bands(rt_ctx* ctx, const rt_aov_planes* planes, uint32_t w, uint32_t h,
                             const rt_band_set* bands, const rt_scene_camera* cam,
                             const rt_sphere* spheres, uint32_t count, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    return trace_aov(ctx, planes, w, h, *bands, cam, spheres, count,
                     static_cast<hipStream_t>(stream), 0u, 0u);
}

rt_status rt_trace_aov(rt_ctx* ctx, const rt_aov_planes* planes, uint32_t w, uint32_t h,
                       const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                       void* stream) {
    const rt_band_set all = stripe_set(h, 0, 1);
    return rt_trace_aov_bands(ctx, planes, w, h, &all, cam, spheres, count, stream);
}

rt_status rt_pick(rt_ctx* ctx, uint32_t w, uint32_t h, uint32_t x, uint32_t y,
                  const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                  void* stream_v, rt_pick_result* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    if (rt_status s = check_image(w, h)) return s;
    if (x >= w || y >= h) return fail(RT_ERR_INVALID_ARGUMENT, "pixel outside the image");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (!ctx->d_pick) {
        hipError_t e = hipMalloc(&ctx->d_pick, 4 * sizeof(float4));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(pick record)");
    }
    // the one wave of the pixel's tile; its record lands in element 0 of each "plane"
    rt_aov_planes planes;
    planes.sphere_id = reinterpret_cast<uint32_t*>(ctx->d_pick);
    planes.hit = reinterpret_cast<float*>(ctx->d_pick + 1);
    planes.normal = reinterpret_cast<float*>(ctx->d_pick + 2);
    planes.material = reinterpret_cast<float*>(ctx->d_pick + 3);
    const rt_band_set band = {y / RT_STRIPE_ROWS, 1u, 1u};
    const uint32_t lane = (y % RT_STRIPE_ROWS) * 8u + (x & 7u);
    if (rt_status s = trace_aov(ctx, &planes, w, h, band, cam, spheres, count, stream, x >> 3,
                                lane + 1u))
        return s;
    float rec[16];
    hipError_t e = hipMemcpyAsync(rec, ctx->d_pick, sizeof(rec), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "rt_pick read-back");
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

void rt_adaptive_params_default(rt_adaptive_params* p) {
    if (!p) return;
    p->min_samples = 16u;
    p->abs_tolerance2 = 1e-5f;
    p->rel_tolerance2 = 2.5e-4f;
}

rt_status rt_update_adaptive_bands(rt_ctx* ctx, const float* in, float* out, const float* error,
                                   uint64_t* tile_mask, uint32_t w, uint32_t h,
                                   const rt_band_set* bands, const rt_scene_camera* cam,
                                   const rt_sphere* spheres, uint32_t count,
                                   const rt_adaptive_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    return update_adaptive(ctx, in, out, error, tile_mask, w, h, *bands, cam, spheres, count,
                           params, stream);
}

rt_status rt_update_adaptive(rt_ctx* ctx, const float* in, float* out, const float* error,
                             uint64_t* tile_mask, uint32_t w, uint32_t h,
                             const rt_scene_camera* cam, const rt_sphere* spheres,
                             uint32_t count, const rt_adaptive_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    const rt_band_set all = stripe_set(h, 0, 1);    // (h is checked below, before the set is)
    return update_adaptive(ctx, in, out, error, tile_mask, w, h, all, cam, spheres, count, params,
                           stream);
}

rt_status rt_converge_frames_bands(rt_ctx* ctx, float* image, float* moments, float* error,
                                   uint64_t* tile_mask, uint32_t* tile_samples, uint32_t w,
                                   uint32_t h, const rt_band_set* bands,
                                   const rt_scene_camera* cam, const rt_sphere* spheres,
                                   uint32_t count, uint32_t frames, const float* seeds,
                                   const rt_adaptive_params* params, uint32_t min_history,
                                   void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    return converge_frames(ctx, image, moments, error, tile_mask, tile_samples, w, h, *bands, cam,
                           spheres, count, frames, seeds, params, min_history, stream);
}

rt_status rt_converge_frames(rt_ctx* ctx, float* image, float* moments, float* error,
                             uint64_t* tile_mask, uint32_t* tile_samples, uint32_t w, uint32_t h,
                             const rt_scene_camera* cam, const rt_sphere* spheres,
                             uint32_t count, uint32_t frames, const float* seeds,
                             const rt_adaptive_params* params, uint32_t min_history,
                             void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    const rt_band_set all = stripe_set(h, 0, 1);    // (h is checked below, before the set is)
    return converge_frames(ctx, image, moments, error, tile_mask, tile_samples, w, h, all, cam,
                           spheres, count, frames, seeds, params, min_history, stream);
}

}  // extern "C"
