/*
 * rt_adaptive.h — variance-driven adaptive sampling (librt_hip.so), an addition to the boundary
 * of rt_abi.h (ABI 7): four entry points and one struct.  Plain C types only.  rt_update gives
 * every pixel below the camera's samples_per_pixel one more sample; rt_update_adaptive gives one
 * only to the pixels whose estimated error is still above a tolerance and passes the others
 * through.  The error estimate is rt_variance.h's variance of the mean (rt_adaptive_error), or
 * any other plane of the caller's.
 *
 * Every exported symbol of this header contains "adaptive", and none contains "variance",
 * "moments", "denoise" or "reproject": those sets are exactly their own headers'.
 */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All of the text below is in f32: every *, + and - is its own IEEE operation (no
 * contraction), / is correctly rounded, subnormals are kept.  Every output bit equals a CPU
 * restatement of this text (tests/test_adaptive.py).
 *   L(c)   = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z      (rt_variance.h's)
 *   u32(a) = the conversion rt_update applies to the accumulator's alpha (truncate, saturate,
 *            NaN and negatives -> 0)
 */
typedef struct rt_adaptive_params {
    uint32_t min_samples;      /* 0..16777216: a pixel with fewer samples is always sampled */
    float    abs_tolerance2;   /* >= 0, finite: the tolerated variance of the mean's luminance */
    float    rel_tolerance2;   /* >= 0, finite: the same relative to L(mean)^2 */
} rt_adaptive_params;
/* 16, 1e-5f, 2.5e-4f */
RT_API void rt_adaptive_params_default(rt_adaptive_params* p);

/* ---- rt_adaptive_error ------------------------------------------------------------------------
 * Writes the error plane the sampler reads: rt_variance.h's initial variance with +inf where the
 * moments are too young.  `error` is width * height floats.  Per pixel X, with n = image[X].a
 * and (m1, m2, _, k) = moments[X]:
 *   d  = m2 - m1 * m1,  d = d when d > 0, else 0 (NaN -> 0)
 *   nn = n when n > 1, else 1 (NaN -> 1)
 *   error[X] = d / nn when k >= (float)min_history, else +inf (NaN k: +inf)
 * One kernel launch on `stream`, one lane per pixel; `image` and `moments` are only read.  A
 * caller may pass any other plane to the sampler instead: rt_variance_filter's `variance` output
 * is a spatially smoothed one.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: image, moments or error NULL;
 * error equal to image or moments; min_history outside 1..16777216.  RT_ERR_INVALID_SIZE: width
 * or height outside 1..65536.  A refused call launches nothing.  It touches no render state. */
RT_API rt_status rt_adaptive_error(rt_ctx* ctx, const float* image, const float* moments,
                                   float* error, uint32_t width, uint32_t height,
                                   uint32_t min_history, void* stream);

/* ---- rt_update_adaptive -----------------------------------------------------------------------
 * One update of the width x height RGBA32F device image `in_rgba` into `out_rgba` in which only
 * some pixels take a sample.  Per pixel X, with I = in[X], n = u32(I.a) and
 * spp = u32(camera->samples_per_pixel):
 *   - camera->camera_has_moved > 0.5:  what rt_update does on a reset: the count is 0, and
 *     sampled = 0 < spp.  `error` is not consulted.
 *   - otherwise:
 *       Lm        = L(I.rgb)
 *       thr       = abs_tolerance2 + rel_tolerance2 * (Lm * Lm)
 *       converged = n >= min_samples && error[X] <= thr     (a NaN on either side: not converged)
 *       sampled   = n < spp && !converged
 * When sampled, out[X] is the texel rt_update writes for these arguments, bit for bit.  When not
 * sampled, out[X] is the texel rt_update writes when the camera's samples_per_pixel is 0: for an
 * integral count that is I itself (after a reset: zeros).
 *
 * `tile_mask` is optional (NULL: not wanted): one uint64_t per 8 x 8 tile,
 * ceil(width / 8) * ceil(height / 8) words, tile rows first.  Bit (y & 7) * 8 + (x & 7) of the
 * word of tile (x / 8, y / 8) is set when pixel (x, y) was sampled; bits of lanes off the image
 * are 0; every word is written.
 *
 * One kernel launch on `stream`, one wave per tile.  A tile without a sampled pixel copies its
 * texels and reads nothing of the scene.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: in_rgba, out_rgba, error, camera
 * or params NULL; out_rgba equal to in_rgba, error or tile_mask; min_samples above 16777216; a
 * tolerance negative, NaN or infinite.  RT_ERR_INVALID_SIZE: width or height outside 1..65536.
 * A refused call launches nothing.
 *
 * Like rt_update it uploads the spheres when their bytes change, and it may build the per-tile
 * candidate lists.  It forgets any uniform sample count the context recorded for `out_rgba` (the
 * counts now differ per pixel).  rt_last_launch_info, the timing events, the tile costs and
 * orders and the known count of `in_rgba` stay as they were. */
RT_API rt_status rt_update_adaptive(rt_ctx* ctx, const float* in_rgba, float* out_rgba,
                                    const float* error, uint64_t* tile_mask, uint32_t width,
                                    uint32_t height, const rt_scene_camera* camera,
                                    const rt_sphere* spheres, uint32_t sphere_count,
                                    const rt_adaptive_params* params, void* stream);

/* The same over a band set, as rt_update_frames_bands and rt_trace_aov_bands: `in_rgba`,
 * `out_rgba`, `error` and `tile_mask` are compact local buffers of bands->count * 8 rows
 * (tile_mask: ceil(width / 8) * bands->count words), local band j being global band
 * bands->first + j * bands->step; pixel coordinates stay global.  count == 0 launches nothing.
 * Also RT_ERR_INVALID_ARGUMENT: bands NULL or not a band set of the image. */
RT_API rt_status rt_update_adaptive_bands(rt_ctx* ctx, const float* in_rgba, float* out_rgba,
                                          const float* error, uint64_t* tile_mask,
                                          uint32_t width, uint32_t height,
                                          const rt_band_set* bands,
                                          const rt_scene_camera* camera,
                                          const rt_sphere* spheres, uint32_t sphere_count,
                                          const rt_adaptive_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_ADAPTIVE_H */
