/*
 * rt_converge.h — the adaptive round as one multi-frame launch (librt_hip.so), an addition to the
 * boundary of rt_abi.h (ABI 7): two entry points.  Plain C types only.  One adaptive sample per
 * pixel is three calls (rt_adaptive_error, rt_update_adaptive, rt_moments_update) and three
 * trips through memory; rt_converge_frames runs `frames` such rounds with each tile's
 * accumulator and moments kept in registers, and a tile that has settled stops early.
 *
 * Every exported symbol of this header contains "converge", and none contains "adaptive",
 * "variance", "moments", "denoise" or "reproject": those sets are exactly their own headers'.
 */
#ifndef RT_CONVERGE_H
#define RT_CONVERGE_H

#include "rt_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames of one kernel launch; a call with more runs consecutive launches. */
#define RT_CONVERGE_MAX_FRAMES_PER_LAUNCH 64u

/* ---- rt_converge_frames -----------------------------------------------------------------------
 * All of the text below is in f32: every *, + and - is its own IEEE operation (no contraction),
 * / is correctly rounded, subnormals are kept.  Every output bit equals the chain of CPU
 * restatements of the three headers' texts (tests/test_converge.py).
 *
 * `image` (the width x height RGBA32F accumulator) and `moments` (rt_variance.h's image of the
 * same size) are read and rewritten in place.  After the call they hold, bit for bit, what this
 * loop leaves:
 *
 *   for f in 0 .. frames - 1:
 *       cam_f   = *camera with random_seed = random_seeds[f] and
 *                 camera_has_moved = (f == 0 ? camera->camera_has_moved : 0)
 *       err     = rt_adaptive_error(image, moments, min_history)       (rt_adaptive.h's text)
 *       new     = rt_update_adaptive(image, err, cam_f, params)        (rt_adaptive.h's text)
 *       moments = rt_moments_update(image, new, moments)               (rt_variance.h's rules 1-4)
 *       image   = new
 *
 * A pixel's texels depend on its own texels only, so the order of pixels does not matter.  Note
 * that rt_adaptive_error reads the count as the float it is (7.5 stays 7.5) while
 * rt_update_adaptive converts it with u32(), and that a frame without a sample can still change a
 * pixel: a count of 7.5 passes through as 7, which rt_moments_update's rule 4 answers by zeroing
 * the moments, so the error is +inf and the pixel is sampled in the next frame.
 *
 * The optional outputs (NULL: not wanted):
 *   error         width * height floats: rt_adaptive_error of the final image and moments.
 *   tile_mask     one uint64_t per 8 x 8 tile in rt_update_adaptive's layout: the lanes sampled in
 *                 the last frame (frame frames - 1).  Bits of lanes off the image are 0; every
 *                 word is written.
 *   tile_samples  one uint32_t per tile, the tile mask's order: the samples the tile's pixels took
 *                 over the whole call (the sum over the frames of the sampled lanes).  Every word
 *                 is written.
 *
 * frames is 1..65536.  Up to RT_CONVERGE_MAX_FRAMES_PER_LAUNCH frames are one kernel launch on
 * `stream`, one wave per tile; more run as consecutive launches (tile_samples accumulates across
 * them).  Within a launch a tile leaves the frame loop after a frame that is not a reset, sampled
 * none of its pixels and left all of their texels bit-identical: every later frame would do the
 * same.  A tile without a sampled pixel reads nothing of the scene, and a tile no frame changed
 * stores no texel.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: image, moments, camera, params or
 * random_seeds NULL; any two of image, moments, error, tile_mask and tile_samples equal; frames 0
 * or above 65536; min_history outside 1..16777216; min_samples above 16777216; a tolerance
 * negative, NaN or infinite.  RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused
 * call launches nothing.
 *
 * Like rt_update_adaptive it uploads the spheres when their bytes change, and it may build the
 * per-tile candidate lists.  It forgets any uniform sample count the context recorded for `image`.
 * rt_last_launch_info, the timing events, the tile costs and orders stay as they were. */
RT_API rt_status rt_converge_frames(rt_ctx* ctx, float* image, float* moments, float* error,
                                    uint64_t* tile_mask, uint32_t* tile_samples, uint32_t width,
                                    uint32_t height, const rt_scene_camera* camera,
                                    const rt_sphere* spheres, uint32_t sphere_count,
                                    uint32_t frames, const float* random_seeds,
                                    const rt_adaptive_params* params, uint32_t min_history,
                                    void* stream);

/* The same over a band set, as rt_update_adaptive_bands: `image`, `moments`, `error`, `tile_mask`
 * and `tile_samples` are compact local buffers of bands->count * 8 rows (the tile planes:
 * ceil(width / 8) * bands->count words), local band j being global band
 * bands->first + j * bands->step; pixel coordinates stay global.  count == 0 launches nothing.
 * Also RT_ERR_INVALID_ARGUMENT: bands NULL or not a band set of the image. */
RT_API rt_status rt_converge_frames_bands(rt_ctx* ctx, float* image, float* moments, float* error,
                                          uint64_t* tile_mask, uint32_t* tile_samples,
                                          uint32_t width, uint32_t height,
                                          const rt_band_set* bands,
                                          const rt_scene_camera* camera,
                                          const rt_sphere* spheres, uint32_t sphere_count,
                                          uint32_t frames, const float* random_seeds,
                                          const rt_adaptive_params* params, uint32_t min_history,
                                          void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_CONVERGE_H */
