// rt_scene_edit.cpp — C-ABI entry points of include/rt_scene_edit.h: the host-only plan and the
// argument checks and launch of the carry kernel (rt_edit.hip).  Of the context rt_edit_carry
// uses the device and drops dst's sample-count record, as rt_reproject does.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "rt_edit_kernels.h"
#include "rt_internal.h"
#include "rt_scene_edit.h"

namespace {

using rti::check_image;
using rti::DeviceGuard;
using rti::fail;
using rti::hip_fail;
using rti::nonneg_finite;

static_assert(sizeof(rt_edit_record) == 32 && sizeof(rt_edit_ball) == 32 &&
                  sizeof(rt_edit_params) == 32 && sizeof(rt_edit_info) == 32,
              "rt_scene_edit.h's structs are 32 bytes each");

// What both entry points refuse of an rt_edit_params beyond rt_reproject's own checks.
rt_status check_edit_params(const rt_edit_params& p) {
    if (p.edit_history > p.carry.max_history)
        return fail(RT_ERR_INVALID_ARGUMENT, "edit_history above carry.max_history");
    if (p._reserved[0] != 0u || p._reserved[1] != 0u || p.carry._reserved != 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "a reserved word is not 0");
    return RT_OK;
}

bool same_words(const float* a, const float* b, int n) {
    return std::memcmp(a, b, sizeof(float) * (size_t)n) == 0;
}

rt_edit_ball ball_of(const rt_sphere& s, float influence, uint32_t owner) {
    rt_edit_ball b;
    std::memset(&b, 0, sizeof(b));
    std::memcpy(b.center, s.position, sizeof(b.center));
    const float t = influence * std::fabs(s.radius);
    b.radius2 = t * t;
    b.owner = owner;
    return b;
}

}  // namespace

extern "C" {

void rt_edit_params_default(rt_edit_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    rt_reproject_params_default(&p->carry);
    p->edit_history = 4u;
    p->influence = 3.0f;
}

size_t rt_edit_plan_bytes(uint32_t n_cur) {
    return sizeof(rt_edit_record) * ((size_t)n_cur + RT_EDIT_MAX_BALLS);
}

// Each operation as rt_scene_edit.h states it (this file is built with -ffp-contract=off).
rt_status rt_edit_plan(const rt_sphere* prev_spheres, uint32_t n_prev, const rt_sphere* spheres,
                       uint32_t n_cur, const uint32_t* prev_index, const rt_edit_params* params,
                       void* table, size_t table_bytes, rt_edit_info* info) {
    if (!params || !table || !info)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL params, table or info");
    if ((!spheres && n_cur > 0u) || (!prev_spheres && n_prev > 0u))
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL spheres or prev_spheres");
    if (n_prev > RT_EDIT_MAX_SPHERES || n_cur > RT_EDIT_MAX_SPHERES)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_prev or n_cur above RT_EDIT_MAX_SPHERES");
    if (table_bytes < rt_edit_plan_bytes(n_cur))
        return fail(RT_ERR_INVALID_ARGUMENT, "table_bytes below rt_edit_plan_bytes(n_cur)");
    if (!prev_index && n_prev != n_cur)
        return fail(RT_ERR_INVALID_ARGUMENT, "prev_index is NULL and n_prev != n_cur");
    const float influence = params->influence;
    if (!nonneg_finite(influence))
        return fail(RT_ERR_INVALID_ARGUMENT, "influence is negative, NaN or infinite");
    if (rt_status s = check_edit_params(*params)) return s;
    std::vector<unsigned char> named(n_prev, 0);
    for (uint32_t i = 0; i < n_cur; ++i) {
        const uint32_t j = prev_index ? prev_index[i] : i;
        if (j == RT_EDIT_NONE) continue;
        if (j >= n_prev) return fail(RT_ERR_INVALID_ARGUMENT, "a prev_index entry is >= n_prev");
        if (named[j]) return fail(RT_ERR_INVALID_ARGUMENT, "a previous index is named twice");
        named[j] = 1;
    }

    std::vector<rt_edit_record> recs(n_cur);
    std::vector<rt_edit_ball> balls;
    rt_edit_info out;
    std::memset(&out, 0, sizeof(out));
    out.n_records = n_cur;
    size_t n_balls = 0;                                   // counted past the limit too
    auto add = [&](const rt_sphere& s, uint32_t owner) {
        if (++n_balls <= RT_EDIT_MAX_BALLS) balls.push_back(ball_of(s, influence, owner));
    };
    for (uint32_t i = 0; i < n_cur; ++i) {
        const rt_sphere& s = spheres[i];
        const uint32_t j = prev_index ? prev_index[i] : i;
        rt_edit_record& r = recs[i];
        std::memcpy(r.center, s.position, sizeof(r.center));
        std::memcpy(r.prev_center, s.position, sizeof(r.prev_center));
        r.scale = 1.0f;
        r.link = RT_EDIT_NONE;
        bool geometry = false;                            // there is a j and the geometry differs
        if (j != RT_EDIT_NONE) {
            const rt_sphere& o = prev_spheres[j];
            std::memcpy(r.prev_center, o.position, sizeof(r.prev_center));
            r.scale = o.radius / s.radius;
            geometry = !(same_words(o.position, s.position, 3) && same_words(&o.radius, &s.radius, 1));
            if (same_words(o.color, s.color, 4)) {
                if (!geometry)
                    r.link = j;
                else if (std::isfinite(o.radius) && std::isfinite(s.radius) && o.radius != 0.0f &&
                         s.radius != 0.0f && std::isfinite(r.scale) && r.scale > 0.0f)
                    r.link = j | RT_EDIT_MOVED;
            }
        }
        if (r.link == j && j != RT_EDIT_NONE) continue;   // unchanged
        ++out.n_changed;
        add(s, i);
        if (geometry) add(prev_spheres[j], i);
    }
    for (uint32_t j = 0; j < n_prev; ++j)
        if (!named[j]) {
            ++out.n_deleted;
            add(prev_spheres[j], RT_EDIT_NONE);
        }
    if (n_balls > RT_EDIT_MAX_BALLS) {
        out.full_restart = 1u;
        balls.clear();
        for (rt_edit_record& r : recs) r.link = RT_EDIT_NONE;
    }
    for (const rt_edit_record& r : recs) {
        if (r.link == RT_EDIT_NONE) ++out.n_restart;
        else if (r.link & RT_EDIT_MOVED) ++out.n_moved;
    }
    out.n_balls = (uint32_t)balls.size();

    unsigned char* t = static_cast<unsigned char*>(table);
    std::memset(t, 0, rt_edit_plan_bytes(n_cur));
    if (n_cur) std::memcpy(t, recs.data(), sizeof(rt_edit_record) * n_cur);
    if (!balls.empty())
        std::memcpy(t + sizeof(rt_edit_record) * n_cur, balls.data(),
                    sizeof(rt_edit_ball) * balls.size());
    *info = out;
    return RT_OK;
}

// One launch (rt_edit.hip).  The checks are rt_reproject's and then the plan's; dst's
// uniform-count record is dropped: dst holds per-pixel counts afterwards.
rt_status rt_edit_carry(rt_ctx* ctx, const float* prev, float* dst, uint32_t w, uint32_t h,
                        const rt_scene_camera* prev_camera, const rt_reproject_planes* planes,
                        const void* plan_dev, uint32_t n_records, uint32_t n_balls,
                        const rt_edit_params* params, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!prev || !dst || !prev_camera || !planes || !params)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "NULL prev_rgba, dst_rgba, prev_camera, planes or params");
    if (dst == prev) return fail(RT_ERR_INVALID_ARGUMENT, "dst_rgba is prev_rgba");
    const rt_reproject_params& carry = params->carry;
    if (carry.max_history < 1u || carry.max_history > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "max_history outside 1..16777216");
    if (carry.lambertian_only > 1u)
        return fail(RT_ERR_INVALID_ARGUMENT, "lambertian_only is neither 0 nor 1");
    const float tol2 = carry.position_tolerance2;
    if (!nonneg_finite(tol2))
        return fail(RT_ERR_INVALID_ARGUMENT, "position_tolerance2 is negative, NaN or infinite");
    if (rt_status s = check_edit_params(*params)) return s;
    if (!planes->prev_sphere_id || !planes->prev_hit || !planes->sphere_id || !planes->hit ||
        !planes->normal || (carry.lambertian_only && !planes->material))
        return fail(RT_ERR_INVALID_ARGUMENT, "a required plane is NULL");
    if (n_balls > RT_EDIT_MAX_BALLS)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_balls above RT_EDIT_MAX_BALLS");
    if (n_records > RT_EDIT_MAX_SPHERES)
        return fail(RT_ERR_INVALID_ARGUMENT, "n_records above RT_EDIT_MAX_SPHERES");
    if (!plan_dev && n_records + n_balls != 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "plan_dev is NULL with records or balls");
    if (rt_status s = check_image(w, h)) return s;
    float rows[9];
    if (rt_status s = rt_reproject_basis(prev_camera, rows)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    rtk::EditParams p;
    std::memset(&p, 0, sizeof(p));
    p.prev = reinterpret_cast<const float4*>(prev);
    p.dst = reinterpret_cast<float4*>(dst);
    p.prev_id = planes->prev_sphere_id;
    p.prev_hit = reinterpret_cast<const float4*>(planes->prev_hit);
    p.id = planes->sphere_id;
    p.hit = reinterpret_cast<const float4*>(planes->hit);
    p.normal = reinterpret_cast<const float4*>(planes->normal);
    p.material = carry.lambertian_only
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
    p.max_history = (float)carry.max_history;
    p.edit_history = (float)params->edit_history;
    p.n_records = n_records;
    p.n_balls = n_balls;
    rti::forget_count(ctx, dst);
    hipError_t e = rtk::launch_edit_carry(p, static_cast<const float4*>(plan_dev),
                                          static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_edit_carry_kernel launch");
    return RT_OK;
}

}  // extern "C"
