// rt_post.cpp — C-ABI entry points of the post-processing stages (include/rt_denoise.h,
// rt_reproject.h, rt_variance.h, rt_adaptive.h's rt_adaptive_error, rt_progress.h): argument
// checks and kernel launches.  Of the context they use the device; rt_reproject also drops dst's
// sample-count record, and rt_progress_stats uses the context's report blocks.
// (rt_update_adaptive and rt_converge_frames are trace launches and live in rt_tracers.cpp;
// rt_progress_run calls rt_converge_frames through its public symbol.)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "rt_adaptive.h"
#include "rt_adaptive_kernels.h"
#include "rt_converge.h"
#include "rt_denoise.h"
#include "rt_denoise_kernels.h"
#include "rt_internal.h"
#include "rt_progress.h"
#include "rt_progress_kernels.h"
#include "rt_reproject.h"
#include "rt_reproject_kernels.h"
#include "rt_variance.h"
#include "rt_variance_kernels.h"

namespace {

using rti::check_image;
using rti::DeviceGuard;
using rti::fail;
using rti::hip_fail;
using rti::nonneg_finite;

// RT_DENOISE_ROUTE=direct (environment, diagnostic) takes the direct route at every step.
bool direct_forced() {
    const char* env = std::getenv("RT_DENOISE_ROUTE");
    return env && !std::strcmp(env, "direct");
}

// Iteration i of an a-trous filter: steps up to 16 stage their texels in LDS, larger steps load
// every tap from global memory.
rtk::AtrousRoute route_for(uint32_t i, bool direct) {
    return !direct && (1u << i) <= rtk::kAtrousRowsMaxStep ? rtk::kAtrousRows : rtk::kAtrousDirect;
}

// The last of n iterations writes the final buffers, so iteration i writes them when the number
// of iterations after it is even and the scratch buffers when it is odd.
bool writes_final(uint32_t n, uint32_t i) { return (n - 1u - i) % 2u == 0u; }

// The report's layout is the kernels' record.
static_assert(sizeof(rt_progress_report) == sizeof(rtk::ProgressRecord) &&
                  offsetof(rt_progress_report, samples) ==
                      offsetof(rtk::ProgressRecord, count) + rtk::kProgSamples * 8 &&
                  offsetof(rt_progress_report, active_tiles) ==
                      offsetof(rtk::ProgressRecord, count) + rtk::kProgActiveTiles * 8 &&
                  offsetof(rt_progress_report, min_count) ==
                      offsetof(rtk::ProgressRecord, min_count) &&
                  offsetof(rt_progress_report, max_error) ==
                      offsetof(rtk::ProgressRecord, max_error),
              "rt_progress_report and rtk::ProgressRecord differ");

// The argument checks rt_progress_stats and rt_progress_run share.
rt_status check_progress(const float* image, const float* moments, const float* error,
                         const uint64_t* tile_active, uint32_t w, uint32_t h,
                         const rt_adaptive_params* params, uint32_t min_history,
                         const rt_progress_report* out) {
    if (!image || !params || !out)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL image, params or out_report");
    if ((moments != nullptr) == (error != nullptr))
        return fail(RT_ERR_INVALID_ARGUMENT, "exactly one of moments and error is given");
    const void* const mask = tile_active;
    if (mask && (mask == image || mask == moments || mask == error))
        return fail(RT_ERR_INVALID_ARGUMENT, "tile_active is image, moments or error");
    if (rt_status s = rti::check_adaptive_params(*params)) return s;
    if (moments && (min_history < 1u || min_history > (1u << 24)))
        return fail(RT_ERR_INVALID_ARGUMENT, "min_history outside 1..16777216");
    return check_image(w, h);
}

// The context's blocks of rt_progress_stats, allocated on first use (the device must be
// current): rtk::kProgressBlockBytes on the device, the report in pinned host memory.
rt_status progress_blocks(rt_ctx* ctx) {
    if (!ctx->d_progress) {
        hipError_t e = hipMalloc(&ctx->d_progress, rtk::kProgressBlockBytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(progress block)");
    }
    if (!ctx->h_progress) {
        hipError_t e = hipHostMalloc(&ctx->h_progress, sizeof(rt_progress_report),
                                     hipHostMallocDefault);
        if (e != hipSuccess) return hip_fail(e, "hipHostMalloc(progress report)");
    }
    return RT_OK;
}

// Shared body of rt_progress_stats / rt_progress_stats_bands after the checks: the two launches
// (rt_progress.hip), the report's copy to the context's pinned block and the wait for it.
rt_status progress_stats(rt_ctx* ctx, const float* image, const float* moments,
                         const float* error, uint64_t* tile_active, uint32_t w, uint32_t h,
                         const rt_band_set& bs, uint32_t spp, const rt_adaptive_params& params,
                         uint32_t min_history, void* stream_v, rt_progress_report* out) {
    if (bs.count == 0u) {                                 // no pixels: nothing to launch
        std::memset(out, 0, sizeof(*out));
        out->min_count = 0xFFFFFFFFu;
        out->max_error = -HUGE_VALF;
        return RT_OK;
    }
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    if (rt_status s = progress_blocks(ctx)) return s;
    void *const dev = ctx->d_progress, *const host = ctx->h_progress;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rtk::ProgressParams p;
    std::memset(&p, 0, sizeof(p));
    p.image = reinterpret_cast<const float4*>(image);
    p.moments = reinterpret_cast<const float4*>(moments);
    p.error = error;
    p.tile_active = tile_active;
    p.block = static_cast<rtk::ProgressRecord*>(dev);
    p.width = w;
    p.height = h;
    p.band_first = bs.first;
    p.band_step = bs.step;
    p.local_bands = bs.count;
    p.spp = spp;
    p.min_samples = params.min_samples;
    p.abs_tolerance2 = params.abs_tolerance2;
    p.rel_tolerance2 = params.rel_tolerance2;
    p.min_history = (float)min_history;
    hipError_t e = rtk::launch_progress(p, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_progress_kernel launch");
    e = hipMemcpyAsync(host, dev, sizeof(rt_progress_report), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "rt_progress_stats read-back");
    std::memcpy(out, host, sizeof(*out));
    return RT_OK;
}

}  // namespace

extern "C" {

void rt_denoise_params_default(rt_denoise_params* p) {
    if (!p) return;
    p->iterations = 5u;
    p->normal_power_log2 = 5u;
    p->inv_sigma_color2 = 1.0f;
    p->inv_sigma_position2 = 4.0f;
}

// One launch per iteration (rt_denoise.hip); src is read by iteration 0 alone.
rt_status rt_denoise(rt_ctx* ctx, const float* src, float* dst, float* scratch, uint32_t w,
                     uint32_t h, const float* hit, const float* normal, const uint32_t* sphere_id,
                     const rt_denoise_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!src || !dst || !hit || !normal || !params)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL src, dst, hit, normal or params");
    if (dst == src) return fail(RT_ERR_INVALID_ARGUMENT, "dst is src");
    const uint32_t n = params->iterations;
    if (n < 1u || n > RT_DENOISE_MAX_ITERATIONS)
        return fail(RT_ERR_INVALID_ARGUMENT, "iterations outside 1..RT_DENOISE_MAX_ITERATIONS");
    if (params->normal_power_log2 > 10u)
        return fail(RT_ERR_INVALID_ARGUMENT, "normal_power_log2 above 10");
    const float ic0 = params->inv_sigma_color2, ip = params->inv_sigma_position2;
    if (!nonneg_finite(ic0) || !nonneg_finite(ip))
        return fail(RT_ERR_INVALID_ARGUMENT, "a sigma term is negative, NaN or infinite");
    if (n >= 2u && (!scratch || scratch == src || scratch == dst))
        return fail(RT_ERR_INVALID_ARGUMENT, "iterations >= 2 need a scratch image of their own");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    const bool direct = direct_forced();
    rtk::DenoiseParams p;
    std::memset(&p, 0, sizeof(p));
    p.hit = reinterpret_cast<const float4*>(hit);
    p.normal = reinterpret_cast<const float4*>(normal);
    p.id = sphere_id;
    p.width = w;
    p.height = h;
    p.npow = params->normal_power_log2;
    p.ip = ip;
    p.in = reinterpret_cast<const float4*>(src);
    float ic = ic0;                                       // ic0 * 4^i: exact, or +inf
    for (uint32_t i = 0; i < n; ++i) {
        p.out = reinterpret_cast<float4*>(writes_final(n, i) ? dst : scratch);
        p.shift = i;
        p.ic = std::min(ic, FLT_MAX);
        hipError_t e =
            rtk::launch_denoise(p, route_for(i, direct), static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return hip_fail(e, "rt_denoise_kernel launch");
        p.in = p.out;
        ic = ic * 4.0f;
    }
    return RT_OK;
}

void rt_reproject_params_default(rt_reproject_params* p) {
    if (!p) return;
    p->max_history = 64u;
    p->lambertian_only = 1u;
    p->position_tolerance2 = 1e-5f;
    p->_reserved = 0u;
}

// The rows of the inverse of [du' dv' e'] in double, each operation as rt_reproject.h states it
// (this file is built with -ffp-contract=off).
rt_status rt_reproject_basis(const rt_scene_camera* cam, float out[9]) {
    if (!cam || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL prev_camera or out");
    double o[3], du[3], dv[3], e[3];
    for (int k = 0; k < 3; ++k) {
        o[k] = (double)cam->center[k];
        du[k] = (double)cam->pixel_delta_u[k];
        dv[k] = (double)cam->pixel_delta_v[k];
        e[k] = (double)cam->viewport_upper_left[k] - o[k];
    }
    auto cross = [](const double* a, const double* b, double* r) {
        r[0] = a[1] * b[2] - a[2] * b[1];
        r[1] = a[2] * b[0] - a[0] * b[2];
        r[2] = a[0] * b[1] - a[1] * b[0];
    };
    double c[3][3];
    cross(dv, e, c[0]);
    cross(e, du, c[1]);
    cross(du, dv, c[2]);
    const double det = (du[0] * c[0][0] + du[1] * c[0][1]) + du[2] * c[0][2];
    if (det == 0.0 || !std::isfinite(det))
        return fail(RT_ERR_INVALID_ARGUMENT, "degenerate prev_camera: [du dv e] is singular");
    float rows[9];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            rows[3 * i + k] = (float)(c[i][k] / det);
            if (!std::isfinite(rows[3 * i + k]))
                return fail(RT_ERR_INVALID_ARGUMENT,
                            "degenerate prev_camera: the basis is not finite");
        }
    std::memcpy(out, rows, sizeof(rows));
    return RT_OK;
}

// One launch (rt_reproject.hip).  dst's uniform-count record is dropped: dst holds per-pixel
// counts afterwards.
rt_status rt_reproject(rt_ctx* ctx, const float* prev, float* dst, uint32_t w, uint32_t h,
                       const rt_scene_camera* prev_camera, const rt_reproject_planes* planes,
                       const rt_reproject_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!prev || !dst || !prev_camera || !planes || !params)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "NULL prev_rgba, dst_rgba, prev_camera, planes or params");
    if (dst == prev) return fail(RT_ERR_INVALID_ARGUMENT, "dst_rgba is prev_rgba");
    if (params->max_history < 1u || params->max_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "max_history outside 1..16777216");
    if (params->lambertian_only > 1u)
        return fail(RT_ERR_INVALID_ARGUMENT, "lambertian_only is neither 0 nor 1");
    if (params->_reserved != 0u) return fail(RT_ERR_INVALID_ARGUMENT, "_reserved is not 0");
    const float tol2 = params->position_tolerance2;
    if (!nonneg_finite(tol2))
        return fail(RT_ERR_INVALID_ARGUMENT, "position_tolerance2 is negative, NaN or infinite");
    if (!planes->prev_sphere_id || !planes->prev_hit || !planes->sphere_id || !planes->hit ||
        !planes->normal || (params->lambertian_only && !planes->material))
        return fail(RT_ERR_INVALID_ARGUMENT, "a required plane is NULL");
    if (rt_status s = check_image(w, h)) return s;
    rtk::ReprojectParams p;
    std::memset(&p, 0, sizeof(p));
    float rows[9];
    if (rt_status s = rt_reproject_basis(prev_camera, rows)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    p.prev = reinterpret_cast<const float4*>(prev);
    p.dst = reinterpret_cast<float4*>(dst);
    p.prev_id = planes->prev_sphere_id;
    p.prev_hit = reinterpret_cast<const float4*>(planes->prev_hit);
    p.id = planes->sphere_id;
    p.hit = reinterpret_cast<const float4*>(planes->hit);
    p.normal = reinterpret_cast<const float4*>(planes->normal);
    p.material = params->lambertian_only
                     ? reinterpret_cast<const float4*>(planes->material) : nullptr;
    p.width = w;
    p.height = h;
    for (int k = 0; k < 3; ++k) {
        p.r0[k] = rows[k];
        p.r1[k] = rows[3 + k];
        p.r2[k] = rows[6 + k];
        p.o[k] = prev_camera->center[k];
    }
    p.tol2 = tol2;
    p.max_history = (float)params->max_history;
    rti::forget_count(ctx, dst);
    hipError_t e = rtk::launch_reproject(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_reproject_kernel launch");
    return RT_OK;
}

void rt_variance_filter_params_default(rt_variance_filter_params* p) {
    if (!p) return;
    p->iterations = 5u;
    p->normal_power_log2 = 5u;
    p->inv_sigma_luminance2 = 1.0f;
    p->inv_sigma_position2 = 4.0f;
    p->min_history = 4u;
    p->fallback_variance = 1.0f;
}

// One launch (rt_variance.hip).
rt_status rt_moments_update(rt_ctx* ctx, const float* in, const float* out, float* moments,
                            uint32_t w, uint32_t h, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!in || !out || !moments)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL in_rgba, out_rgba or moments");
    if (in == out || moments == in || moments == out)
        return fail(RT_ERR_INVALID_ARGUMENT, "two of in_rgba, out_rgba and moments are equal");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    rtk::MomentsParams p;
    p.in = reinterpret_cast<const float4*>(in);
    p.out = reinterpret_cast<const float4*>(out);
    p.moments = reinterpret_cast<float4*>(moments);
    p.width = w;
    p.height = h;
    hipError_t e = rtk::launch_moments_update(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_moments_update_kernel launch");
    return RT_OK;
}

// One launch per iteration (rt_variance.hip), rt_denoise's scheme with the variance plane beside
// the image; src and moments are read by iteration 0 alone, which computes v0 as it loads.
rt_status rt_variance_filter(rt_ctx* ctx, const float* src, float* dst, float* scratch,
                             const float* moments, float* variance, float* variance_scratch,
                             uint32_t w, uint32_t h, const float* hit, const float* normal,
                             const uint32_t* sphere_id, const rt_variance_filter_params* params,
                             void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!src || !dst || !moments || !variance || !hit || !normal || !params)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "NULL src, dst, moments, variance, hit, normal or params");
    if (dst == src || dst == moments)
        return fail(RT_ERR_INVALID_ARGUMENT, "dst is src or moments");
    if (variance == src || variance == dst || variance == moments)
        return fail(RT_ERR_INVALID_ARGUMENT, "variance is src, dst or moments");
    const uint32_t n = params->iterations;
    if (n < 1u || n > RT_VARIANCE_MAX_ITERATIONS)
        return fail(RT_ERR_INVALID_ARGUMENT, "iterations outside 1..RT_VARIANCE_MAX_ITERATIONS");
    if (params->normal_power_log2 > 10u)
        return fail(RT_ERR_INVALID_ARGUMENT, "normal_power_log2 above 10");
    if (params->min_history < 1u || params->min_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "min_history outside 1..16777216");
    const float il = params->inv_sigma_luminance2, ip = params->inv_sigma_position2;
    const float fb = params->fallback_variance;
    if (!nonneg_finite(il) || !nonneg_finite(ip) || !nonneg_finite(fb))
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "a sigma term or fallback_variance is negative, NaN or infinite");
    if (n >= 2u) {
        if (!scratch || scratch == src || scratch == dst || scratch == moments ||
            scratch == variance)
            return fail(RT_ERR_INVALID_ARGUMENT,
                        "iterations >= 2 need a scratch image of their own");
        if (!variance_scratch || variance_scratch == src || variance_scratch == dst ||
            variance_scratch == scratch || variance_scratch == moments ||
            variance_scratch == variance)
            return fail(RT_ERR_INVALID_ARGUMENT,
                        "iterations >= 2 need a variance_scratch plane of their own");
    }
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    const bool direct = direct_forced();
    rtk::VarianceParams p;
    std::memset(&p, 0, sizeof(p));
    p.hit = reinterpret_cast<const float4*>(hit);
    p.normal = reinterpret_cast<const float4*>(normal);
    p.id = sphere_id;
    p.width = w;
    p.height = h;
    p.npow = params->normal_power_log2;
    p.il = il;
    p.ip = ip;
    p.min_history = (float)params->min_history;
    p.fallback = fb;
    p.in = reinterpret_cast<const float4*>(src);
    p.moments = reinterpret_cast<const float4*>(moments);
    for (uint32_t i = 0; i < n; ++i) {
        const bool last = writes_final(n, i);
        p.out = reinterpret_cast<float4*>(last ? dst : scratch);
        p.vout = last ? variance : variance_scratch;
        p.shift = i;
        hipError_t e = rtk::launch_variance_filter(p, route_for(i, direct),
                                                   static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return hip_fail(e, "rt_variance_filter_kernel launch");
        p.in = p.out;
        p.vin = p.vout;
        p.moments = nullptr;
    }
    return RT_OK;
}

// One launch (rt_adaptive.hip).
rt_status rt_adaptive_error(rt_ctx* ctx, const float* image, const float* moments, float* error,
                            uint32_t w, uint32_t h, uint32_t min_history, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!image || !moments || !error)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL image, moments or error");
    if (error == image || error == moments)
        return fail(RT_ERR_INVALID_ARGUMENT, "error is image or moments");
    if (min_history < 1u || min_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "min_history outside 1..16777216");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    rtk::AdaptiveErrorParams p;
    p.image = reinterpret_cast<const float4*>(image);
    p.moments = reinterpret_cast<const float4*>(moments);
    p.error = error;
    p.width = w;
    p.height = h;
    p.min_history = (float)min_history;
    hipError_t e = rtk::launch_adaptive_error(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_adaptive_error_kernel launch");
    return RT_OK;
}

rt_status rt_progress_stats_bands(rt_ctx* ctx, const float* image, const float* moments,
                                  const float* error, uint64_t* tile_active, uint32_t w,
                                  uint32_t h, const rt_band_set* bands, uint32_t spp,
                                  const rt_adaptive_params* params, uint32_t min_history,
                                  void* stream, rt_progress_report* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    if (rt_status s = check_progress(image, moments, error, tile_active, w, h, params,
                                     min_history, out))
        return s;
    if (rt_status s = rti::check_band_set(h, *bands)) return s;
    return progress_stats(ctx, image, moments, error, tile_active, w, h, *bands, spp, *params,
                          min_history, stream, out);
}

rt_status rt_progress_stats(rt_ctx* ctx, const float* image, const float* moments,
                            const float* error, uint64_t* tile_active, uint32_t w, uint32_t h,
                            uint32_t spp, const rt_adaptive_params* params, uint32_t min_history,
                            void* stream, rt_progress_report* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (rt_status s = check_progress(image, moments, error, tile_active, w, h, params,
                                     min_history, out))
        return s;
    return progress_stats(ctx, image, moments, error, tile_active, w, h,
                          rti::stripe_set(h, 0, 1), spp, *params, min_history, stream, out);
}

// rt_progress.h's loop: reports through progress_stats, frames through rt_converge_frames.
rt_status rt_progress_run(rt_ctx* ctx, float* image, float* moments, uint64_t* tile_active,
                          uint32_t w, uint32_t h, const rt_scene_camera* cam,
                          const rt_sphere* spheres, uint32_t count, const float* seeds,
                          const rt_adaptive_params* params, uint32_t min_history,
                          const rt_progress_goal* goal, void* stream, uint32_t* frames_run,
                          rt_progress_report* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!moments || !cam || !seeds || !goal || !frames_run)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "NULL moments, camera, random_seeds, goal or frames_run");
    if (image == moments) return fail(RT_ERR_INVALID_ARGUMENT, "image is moments");
    if (goal->max_frames < 1u || goal->max_frames > 65536u || goal->check_every < 1u ||
        goal->check_every > 65536u)
        return fail(RT_ERR_INVALID_ARGUMENT, "max_frames or check_every outside 1..65536");
    if (rt_status s = check_progress(image, moments, nullptr, tile_active, w, h, params,
                                     min_history, out))
        return s;
    const rt_band_set all = rti::stripe_set(h, 0, 1);
    const uint32_t spp = rti::host_f2u(cam->samples_per_pixel);
    rt_progress_report report;
    auto stats = [&]() {
        return progress_stats(ctx, image, moments, nullptr, tile_active, w, h, all, spp, *params,
                              min_history, stream, &report);
    };
    uint32_t done = 0;
    const bool moved = cam->camera_has_moved > 0.5f;
    bool more = true;
    if (!moved) {
        if (rt_status s = stats()) return s;
        more = report.active > goal->max_active;
    }
    rt_scene_camera still = *cam;
    still.camera_has_moved = 0.0f;
    while (more) {
        const uint32_t f = std::min(goal->check_every, goal->max_frames - done);
        if (rt_status s = rt_converge_frames(ctx, image, moments, nullptr, nullptr, nullptr, w, h,
                                             done == 0u ? cam : &still, spheres, count, f,
                                             seeds + done, params, min_history, stream))
            return s;
        done += f;
        if (rt_status s = stats()) return s;
        more = report.active > goal->max_active && done < goal->max_frames;
    }
    *frames_run = done;
    *out = report;
    return RT_OK;
}

}  // extern "C"
