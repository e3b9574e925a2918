/*
 * rt_reproject.h — carries the accumulator of a previous view into the current one, guided by
 * the first-hit G-buffers of rt_aov.h for both views (librt_hip.so), an addition to the boundary
 * of rt_abi.h (ABI 7): three entry points and two structs.  Plain C types only.
 */
#ifndef RT_REPROJECT_H
#define RT_REPROJECT_H

#include "rt_abi.h"
#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Both views have the same width and height and the same scene: the sphere records are unchanged
 * between them (a sphere that moved keeps its id and would carry history it should not here:
 * rt_scene_edit.h carries the accumulator across an edited scene).  The current camera is not an
 * argument: the current view's hit points are already in world space.
 *
 * All device arithmetic is f32: every *, + and - is its own IEEE operation (no contraction, no
 * fma), / is correctly rounded, subnormals are kept.  Every output bit equals a CPU restatement
 * of this text (tests/test_reproject.py).
 *
 * Basis (host, double).  From prev_camera take as doubles o' = center, ul' =
 * viewport_upper_left, du' = pixel_delta_u, dv' = pixel_delta_v.  With
 *   e'         = ul' - o'
 *   cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *   dot(a,b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   c0 = cross(dv', e'),  c1 = cross(e', du'),  c2 = cross(du', dv'),  det = dot(du', c0)
 * the rows of the inverse of [du' dv' e'] are out[3*i + k] = (float)(c_i[k] / det): a world
 * point o' + a du' + b dv' + c e' has (a, b, c) = (r0 . q, r1 . q, r2 . q), q its offset from
 * o', and lies on the previous view's ray through sample position (a / c, b / c), where pixel
 * (x, y)'s centre is (x + 0.5, y + 0.5).  det zero or not finite, or any out not finite, is
 * RT_ERR_INVALID_ARGUMENT.  Call the rows r0, r1, r2.
 *
 * Per pixel P = (x, y).  Let id = sphere_id[P], p = hit[P].xyz, nP = normal[P].xyz.  The result
 * is "no history", dst[P] = (0, 0, 0, 0), when any of these holds, tested in this order:
 *   1. id == RT_AOV_MISS
 *   2. lambertian_only and !(material[P].w < -1)
 *   3. !(c > 0), with q = p - o' per component (o' as f32),
 *      a = (r0.x*q.x + r0.y*q.y) + r0.z*q.z, and likewise b with r1 and c with r2
 *   4. not (px >= -1 && px < (float)width && py >= -1 && py < (float)height), where
 *      px = a / c - 0.5f and py = b / c - 0.5f (written so that NaN fails)
 *   5. no tap is kept (below).
 *
 * Taps.  fx = floorf(px), fy = floorf(py), tx = px - fx, ty = py - fy, x0 = (int)fx,
 * y0 = (int)fy, r2q = (q.x*q.x + q.y*q.y) + q.z*q.z, lim = position_tolerance2 * r2q.  The taps
 * are Q = (x0 + i, y0 + j), j = 0, 1 outer and i = 0, 1 inner, with the bilinear weight
 * bw = (j ? ty : 1 - ty) * (i ? tx : 1 - tx).  A tap is skipped when
 *   - it is off the image;
 *   - prev_sphere_id[Q] != id;
 *   - !(dl * dl <= lim), where e = p - prev_hit[Q].xyz and
 *     dl = (nP.x*e.x + nP.y*e.y) + nP.z*e.z: the distance of the previous hit point from P's
 *     tangent plane, relative to the distance to the previous eye;
 *   - !(prev_rgba[Q].a > 0);
 *   - !(bw > 0).
 * Kept taps accumulate in tap order: sw += bw, sum.c += bw * prev_rgba[Q].c for c in rgb,
 * n = min(n, prev_rgba[Q].a) starting from +inf.  Then dst[P].rgb = sum.rgb / sw and
 * dst[P].a = min(n, (float)max_history).  A non-finite colour in a kept tap propagates into
 * dst[P]; a NaN in p or nP fails the tests it enters.
 */
typedef struct rt_reproject_params {
    uint32_t max_history;          /* 1 .. 16777216: cap on the carried sample count          */
    uint32_t lambertian_only;      /* 0 / 1: pixels whose material is not Lambertian restart  */
    float    position_tolerance2;  /* >= 0, finite: see the plane-distance test               */
    uint32_t _reserved;            /* must be 0                                               */
} rt_reproject_params;             /* 16 bytes */
/* max_history 64, lambertian_only 1, position_tolerance2 1e-5f; NULL is a no-op */
RT_API void rt_reproject_params_default(rt_reproject_params* p);

/* Host only, no device: the rows of the inverse of [du' dv' e'] (above), 9 floats.
 * RT_ERR_INVALID_ARGUMENT: prev_camera or out NULL, or a degenerate camera. */
RT_API rt_status rt_reproject_basis(const rt_scene_camera* prev_camera, float out[9]);

typedef struct rt_reproject_planes {   /* device pointers, planes of rt_trace_aov */
    const uint32_t* prev_sphere_id;    /* previous view, required */
    const float*    prev_hit;          /* previous view, required */
    const uint32_t* sphere_id;         /* current view, required  */
    const float*    hit;               /* current view, required  */
    const float*    normal;            /* current view, required  */
    const float*    material;          /* current view; required iff lambertian_only */
} rt_reproject_planes;

/* Writes every pixel of the width x height RGBA32F device image `dst_rgba` from the previous
 * view's accumulator `prev_rgba` (alpha = sample count), one kernel launch on `stream`; nothing
 * else is written.  `prev_camera` is a host pointer.  The result's alpha differs from pixel to
 * pixel (0 = restart); rt_update / rt_update_frames take it with camera_has_moved = 0, and
 * rt_denoise takes it as it is.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: prev_rgba, dst_rgba,
 * prev_camera, planes, params or a required plane NULL (material counts as required only with
 * lambertian_only); dst_rgba == prev_rgba; max_history outside 1..2^24; lambertian_only > 1;
 * _reserved != 0; position_tolerance2 negative, NaN or infinite; a degenerate prev_camera
 * (basis).  RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused call launches
 * nothing.
 *
 * Like the calls of rt_aov.h it touches no candidate lists, tile orders, launch info or timing
 * events.  One exception: the context forgets the uniform sample count it may know for
 * dst_rgba, which no longer holds one count (the trace kernels verify that hint per pixel
 * anyway; this only saves a wasted hinted first frame). */
RT_API rt_status rt_reproject(rt_ctx* ctx, const float* prev_rgba, float* dst_rgba,
                              uint32_t width, uint32_t height,
                              const rt_scene_camera* prev_camera,
                              const rt_reproject_planes* planes,
                              const rt_reproject_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_REPROJECT_H */
