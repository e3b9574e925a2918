/*
 * rt_aov.h — first-hit G-buffer and picking (librt_hip.so), an addition to the boundary of
 * rt_abi.h (ABI 7): three entry points and two structs.  Plain C types only.
 */
#ifndef RT_AOV_H
#define RT_AOV_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is under each pixel, without noise: the first hit of the ray through the pixel's
 * centre.  For global pixel (x, y):
 *   o  = camera.center (always a pinhole: defocus_angle is not read, nor are random_seed,
 *        samples_per_pixel, max_depth and camera_has_moved),
 *   pc = fma(y + 0.5, pixel_delta_v, fma(x + 0.5, pixel_delta_u, viewport_upper_left)),
 *   d  = pc - o (not normalised),
 * traced by sphere_list_hit (wgsl:164-221): index order, tmin = 0.001, tmax = 3.4e35, a later
 * sphere wins only if strictly nearer; p = fma(t, d, o), outward = (p - C) / R, front =
 * dot(d, outward) < 0, n = front ? outward : -outward.  Every float is bit-identical to the
 * CPU oracle's sphere_hit, in both scan modes (rt_set_scan_mode).
 *
 * Planes: tightly packed, row-major device buffers, any non-empty subset (NULL = not wanted).
 *   sphere_id  u32 per pixel   index of the winning sphere        miss: RT_AOV_MISS
 *   hit        4 x f32         p.x, p.y, p.z, t                   miss: 0, 0, 0, +inf
 *   normal     4 x f32         n.x, n.y, n.z, front ? 1 : 0       miss: 0, 0, 0, 0
 *   material   4 x f32         the sphere's color[4] verbatim     miss: 0, 0, 0, 0
 */
#define RT_AOV_MISS 0xFFFFFFFFu
typedef struct rt_aov_planes {      /* device pointers; NULL = not wanted; not all NULL */
    uint32_t* sphere_id;
    float*    hit;
    float*    normal;
    float*    material;
} rt_aov_planes;

/* The planes of a width x height image.  Arguments and status codes as rt_update: camera and
 * spheres are host pointers, the spheres are uploaded only when their bytes change, and
 * sphere_count == 0 is valid (every pixel is a miss).  The call shares the context's sphere
 * records with the progressive render and nothing else: it neither reads nor rebuilds the
 * candidate lists, tile costs and orders, and leaves rt_last_launch_info, the launch-timing
 * events and the images' known sample counts as they were. */
RT_API rt_status rt_trace_aov(rt_ctx* ctx, const rt_aov_planes* planes, uint32_t width,
                              uint32_t height, const rt_scene_camera* camera,
                              const rt_sphere* spheres, uint32_t sphere_count, void* stream);
/* The same over a band set: the planes are compact local buffers of width x (bands->count *
 * RT_STRIPE_ROWS) rows, pixel coordinates stay global (as rt_update_frames_bands).  Rows past
 * the image's last row are not written.  A set with count == 0 launches nothing. */
RT_API rt_status rt_trace_aov_bands(rt_ctx* ctx, const rt_aov_planes* planes, uint32_t width,
                                    uint32_t height, const rt_band_set* bands,
                                    const rt_scene_camera* camera, const rt_sphere* spheres,
                                    uint32_t sphere_count, void* stream);

/* One pixel's record; a miss has sphere_id == RT_AOV_MISS, t = +inf and zeros elsewhere. */
typedef struct rt_pick_result {
    uint32_t sphere_id;
    float    t;
    float    p[3];
    float    normal[3];
    uint32_t front_face;
    float    color[4];
} rt_pick_result;
/* What is under pixel (x, y): the texel rt_trace_aov writes there, from a launch of the one
 * wave that owns the pixel's 8 x 8 tile.  x >= width or y >= height is
 * RT_ERR_INVALID_ARGUMENT.  Synchronous on `stream` (returns after the record is on the
 * host). */
RT_API rt_status rt_pick(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                         const rt_scene_camera* camera, const rt_sphere* spheres,
                         uint32_t sphere_count, void* stream, rt_pick_result* out);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_AOV_H */
