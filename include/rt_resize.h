/*
 * rt_resize.h — carries the accumulator of a previous view into a current view of another image
 * size (librt_hip.so): rt_reproject with a previous size of its own, misses optionally carried by
 * direction, holes optionally filled from the nearest previous texel, and optionally a second
 * image pair in the same launch.  An addition to the boundary of rt_abi.h (ABI 7): two entry
 * points and two structs.  Plain C types only.
 */
#ifndef RT_RESIZE_H
#define RT_RESIZE_H

#include "rt_abi.h"
#include "rt_aov.h"
#include "rt_reproject.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The previous view is prev_width x prev_height, the current one width x height; the scene is
 * the same in both (rt_reproject.h).  The planes are rt_reproject_planes: the prev_* planes are
 * prev_width x prev_height, the others width x height.
 *
 * All device arithmetic is f32: every *, + and - is its own IEEE operation (no contraction), the
 * only fused operations are the two fmaf named below, / is correctly rounded, subnormals are
 * kept.  Every output bit equals a CPU restatement of this text (tests/test_resize.py).
 *
 * Symbols.  o', r0, r1, r2 are prev_camera's centre (as f32) and rt_reproject_basis(prev_camera),
 * as in rt_reproject.  pw, ph are prev_width, prev_height.
 *
 * Per pixel P = (x, y) of the current image.  Let id = sphere_id[P] and
 * surface = (id != RT_AOV_MISS).
 *   1. eligible = surface ? (!lambertian_only || material[P].w < -1) : (sky != 0).
 *   2. If !eligible and fill == RT_RESIZE_FILL_NONE: dst[P] = (0, 0, 0, 0), and nothing more is
 *      read.
 *   3. The offset q.  For a surface q = hit[P].xyz - o' per component.  For a miss q = pc - o per
 *      component, where o = camera.center and
 *        pc.k = fmaf(y + 0.5f, pixel_delta_v.k, fmaf(x + 0.5f, pixel_delta_u.k,
 *                                                    viewport_upper_left.k))
 *      of `camera`: the centre ray of rt_aov.h.  A direction is a point at infinity, so its
 *      projection into the previous view is exact whatever the two centres are.
 *   4. a = (r0.x*q.x + r0.y*q.y) + r0.z*q.z, likewise b with r1 and c with r2;
 *      px = a / c - 0.5f, py = b / c - 0.5f;
 *      projected = c > 0 && px >= -1 && px < (float)pw && py >= -1 && py < (float)ph
 *      (written so that NaN fails).
 *   5. If eligible && projected: the four taps of rt_reproject.h, with pw, ph for the bounds and
 *      pw for the pitch: the same tap order, weights bw and skip rules, except that for a miss a
 *      tap is skipped when prev_sphere_id[Q] != RT_AOV_MISS instead of by the id and plane tests
 *      (normal[P] and lim are not read; off the image, !(prev[Q].a > 0) and !(bw > 0) skip as
 *      ever).  Kept taps give rgb = sum / sw and a = min(n, (float)max_history), exactly as in
 *      rt_reproject.
 *   6. Otherwise, and also when no tap is kept, the pixel is a hole.  With
 *      fill == RT_RESIZE_FILL_NEAREST and projected:
 *        X = min(max((int)floorf(px + 0.5f), 0), pw - 1), Y likewise from py and ph,
 *        dst[P] = (prev[Y][X].rgb, 0):
 *      the colour is shown, and with alpha 0 the next rt_update treats the pixel as a restart.
 *      In every other case dst[P] = (0, 0, 0, 0).
 *   7. The second pair, when given, is carried by the same text with prev_second / dst_second in
 *      place of the first pair: its own alpha > 0 test, its own n and its own sw.  The result is
 *      bit for bit what a second call with that pair alone leaves; the geometry and the guide
 *      loads are shared, which is why the pair is in the call.
 *
 * Guarantee.  With prev_width == width, prev_height == height, sky == 0,
 * fill == RT_RESIZE_FILL_NONE and no second pair, every output bit equals rt_reproject's for any
 * input, non-finite input included.
 */
#define RT_RESIZE_FILL_NONE    0u
#define RT_RESIZE_FILL_NEAREST 1u
typedef struct rt_resize_params {
    uint32_t max_history;          /* 1 .. 2^24, as rt_reproject                         */
    uint32_t lambertian_only;      /* 0 / 1, as rt_reproject                             */
    float    position_tolerance2;  /* >= 0, finite, as rt_reproject                      */
    uint32_t sky;                  /* 0 / 1: carry misses by direction                   */
    uint32_t fill;                 /* RT_RESIZE_FILL_*                                   */
    uint32_t _reserved[3];         /* must be 0                                          */
} rt_resize_params;                /* 32 bytes */
/* 64, 1, 1e-5f, 0, RT_RESIZE_FILL_NONE; NULL is a no-op */
RT_API void rt_resize_params_default(rt_resize_params* p);

typedef struct rt_resize_images {  /* device pointers, RGBA32F, alpha = sample count     */
    const float* prev_rgba;        /* prev_width x prev_height, required                 */
    float*       dst_rgba;         /* width x height, required                           */
    const float* prev_second;      /* optional second pair (a moments image, say):       */
    float*       dst_second;       /* both NULL or both non-NULL                         */
} rt_resize_images;                /* 32 bytes */

/* Writes every pixel of dst_rgba (and of dst_second, when given), one kernel launch on `stream`;
 * nothing else is written.  No destination may overlap a previous image, a plane or the other
 * destination in any byte: the images differ in size, and the call refuses only equal pointers;
 * what an overlap leaves is undefined.  `images`, `prev_camera`, `camera`, `planes` and `params` are host
 * pointers; `camera`, the current view's, is read only if sky || fill.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: images, prev_camera, planes or
 * params NULL; prev_rgba or dst_rgba NULL; exactly one of prev_second / dst_second NULL; any dst
 * equal to any prev, or dst_second == dst_rgba; a required plane NULL (material counts as
 * required only with lambertian_only); max_history outside 1..2^24; lambertian_only > 1;
 * sky > 1; fill > 1; a reserved word non-zero; position_tolerance2 negative, NaN or infinite;
 * a degenerate prev_camera (rt_reproject_basis); camera NULL while sky || fill.
 * RT_ERR_INVALID_SIZE: prev_width, prev_height, width or height outside 1..65536.  A refused
 * call launches nothing.
 *
 * The context forgets the uniform sample count it may know for dst_rgba and dst_second, and
 * touches no other render state: candidate lists, tile orders, launch info and timing events
 * stay as they were. */
RT_API rt_status rt_resize_carry(rt_ctx* ctx, const rt_resize_images* images,
                                 uint32_t prev_width, uint32_t prev_height,
                                 uint32_t width, uint32_t height,
                                 const rt_scene_camera* prev_camera,
                                 const rt_scene_camera* camera,   /* read only if sky || fill */
                                 const rt_reproject_planes* planes,
                                 const rt_resize_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_RESIZE_H */
