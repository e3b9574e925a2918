// rt_resize.cpp — C-ABI entry points of include/rt_resize.h: the argument checks and launch of
// the resize-carry kernel (rt_resize.hip).  Of the context rt_resize_carry uses the device and
// drops the destinations' sample-count records, as rt_reproject does.
#include <hip/hip_runtime_api.h>

#include <cstring>

#include "rt_internal.h"
#include "rt_resize.h"
#include "rt_resize_kernels.h"

namespace {

using rti::check_image;
using rti::DeviceGuard;
using rti::fail;
using rti::hip_fail;
using rti::nonneg_finite;

static_assert(sizeof(rt_resize_params) == 32 && sizeof(rt_resize_images) == 32,
              "rt_resize.h's structs are 32 bytes each");

}  // namespace

extern "C" {

void rt_resize_params_default(rt_resize_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_history = 64u;
    p->lambertian_only = 1u;
    p->position_tolerance2 = 1e-5f;
    p->sky = 0u;
    p->fill = RT_RESIZE_FILL_NONE;
}

// One launch (rt_resize.hip).  The checks are rt_reproject's, over both sizes, and then the
// header's own; the destinations' uniform-count records are dropped: they hold per-pixel counts
// afterwards.
rt_status rt_resize_carry(rt_ctx* ctx, const rt_resize_images* images, uint32_t pw, uint32_t ph,
                          uint32_t w, uint32_t h, const rt_scene_camera* prev_camera,
                          const rt_scene_camera* camera, const rt_reproject_planes* planes,
                          const rt_resize_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!images || !prev_camera || !planes || !params)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL images, prev_camera, planes or params");
    const float* prev = images->prev_rgba;
    float* dst = images->dst_rgba;
    const float* prev2 = images->prev_second;
    float* dst2 = images->dst_second;
    if (!prev || !dst) return fail(RT_ERR_INVALID_ARGUMENT, "NULL prev_rgba or dst_rgba");
    if ((prev2 == nullptr) != (dst2 == nullptr))
        return fail(RT_ERR_INVALID_ARGUMENT, "exactly one of prev_second and dst_second is NULL");
    if (dst == prev || (dst2 && (dst2 == prev || dst2 == prev2 || dst == prev2)))
        return fail(RT_ERR_INVALID_ARGUMENT, "a destination is a previous image");
    if (dst2 && dst2 == dst) return fail(RT_ERR_INVALID_ARGUMENT, "dst_second is dst_rgba");
    if (params->max_history < 1u || params->max_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "max_history outside 1..16777216");
    if (params->lambertian_only > 1u)
        return fail(RT_ERR_INVALID_ARGUMENT, "lambertian_only is neither 0 nor 1");
    if (params->sky > 1u) return fail(RT_ERR_INVALID_ARGUMENT, "sky is neither 0 nor 1");
    if (params->fill > RT_RESIZE_FILL_NEAREST)
        return fail(RT_ERR_INVALID_ARGUMENT, "fill is not an RT_RESIZE_FILL_* value");
    if (params->_reserved[0] != 0u || params->_reserved[1] != 0u || params->_reserved[2] != 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "a reserved word is not 0");
    const float tol2 = params->position_tolerance2;
    if (!nonneg_finite(tol2))
        return fail(RT_ERR_INVALID_ARGUMENT, "position_tolerance2 is negative, NaN or infinite");
    if (!planes->prev_sphere_id || !planes->prev_hit || !planes->sphere_id || !planes->hit ||
        !planes->normal || (params->lambertian_only && !planes->material))
        return fail(RT_ERR_INVALID_ARGUMENT, "a required plane is NULL");
    const bool reads_camera = params->sky != 0u || params->fill != RT_RESIZE_FILL_NONE;
    if (reads_camera && !camera)
        return fail(RT_ERR_INVALID_ARGUMENT, "camera is NULL with sky or fill");
    if (rt_status s = check_image(pw, ph)) return s;
    if (rt_status s = check_image(w, h)) return s;
    float rows[9];
    if (rt_status s = rt_reproject_basis(prev_camera, rows)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    rtk::ResizeParams p;
    std::memset(&p, 0, sizeof(p));
    p.prev = reinterpret_cast<const float4*>(prev);
    p.dst = reinterpret_cast<float4*>(dst);
    p.prev2 = reinterpret_cast<const float4*>(prev2);
    p.dst2 = reinterpret_cast<float4*>(dst2);
    p.prev_id = planes->prev_sphere_id;
    p.prev_hit = reinterpret_cast<const float4*>(planes->prev_hit);
    p.id = planes->sphere_id;
    p.hit = reinterpret_cast<const float4*>(planes->hit);
    p.normal = reinterpret_cast<const float4*>(planes->normal);
    p.material = params->lambertian_only
                     ? reinterpret_cast<const float4*>(planes->material) : nullptr;
    p.width = w;
    p.height = h;
    p.prev_width = pw;
    p.prev_height = ph;
    for (int k = 0; k < 3; ++k) {
        p.r0[k] = rows[k];
        p.r1[k] = rows[3 + k];
        p.r2[k] = rows[6 + k];
        p.o[k] = prev_camera->center[k];
    }
    p.tol2 = tol2;
    p.max_history = (float)params->max_history;
    p.sky = params->sky;
    p.fill = params->fill;
    if (reads_camera) rti::fill_camera_grid(p, *camera);
    rti::forget_count(ctx, dst);
    if (dst2) rti::forget_count(ctx, dst2);
    hipError_t e = rtk::launch_resize_carry(p, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_resize_carry_kernel launch");
    return RT_OK;
}

}  // extern "C"
