/*
 * rt_matte.h — sample-coverage ID mattes (librt_hip.so), an addition to the boundary of
 * rt_abi.h (ABI 7): four entry points and two structs.  Plain C types only.
 */
#ifndef RT_MATTE_H
#define RT_MATTE_H

#include "rt_abi.h"
#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which spheres the samples of a pixel saw, and how often: the per-object coverage matte that
 * goes beside the beauty image.  rt_trace_aov names the one sphere under the pixel's centre, seen
 * through a pinhole; the render jitters every sample over the pixel and starts it on the lens
 * disk (get_ray, wgsl:305-331).  rt_matte_frames traces exactly those camera rays — the ray of
 * sample n of pixel (x, y) is a pure function of (x, y, n, random_seed) and its first hit is an
 * integer — and counts the first hits per pixel in RT_MATTE_SLOTS slots.
 *
 * State: three tightly packed, row-major device planes.
 *   ids     4 x u32 per pixel   the id of each slot
 *   counts  4 x u32 per pixel   the samples that slot has seen; 0 = the slot is empty, and its id
 *                               is written as 0 and means nothing
 *   tally   2 x u32 per pixel   .x = samples taken, .y = samples whose id found no slot (overflow)
 * The background (a ray that hits nothing) is the id RT_AOV_MISS and takes a slot like any sphere.
 */
#define RT_MATTE_SLOTS 4
typedef struct rt_matte_planes {    /* device pointers, none NULL */
    uint32_t* ids;
    uint32_t* counts;
    uint32_t* tally;
} rt_matte_planes;

/* `frames` (1..RT_MATTE_MAX_FRAMES) frames over the planes of a width x height image, in place.
 * For frame f and global pixel (x, y), with B = u32(random_seeds[f] * 2^32) converted as rt_update
 * converts camera.random_seed:
 *   - if f == 0 and camera.camera_has_moved > 0.5 the pixel's ten words are first treated as zero;
 *     their previous contents are not read for the decision (wgsl:345-350);
 *   - n = tally.x;
 *   - the ray is get_ray(location, 1 + n + B) of wgsl:305-331 with u32 wrap-around: the ray
 *     rt_update traces for a pixel whose count is n, jitter and lens included (defocus_angle <= 0
 *     means no lens);
 *   - v = the index sphere_list_hit returns (wgsl:164-180: index order, tmin 0.001, tmax 3.4e35, a
 *     later sphere only if strictly nearer; NaN rays behave as sphere_hit makes them behave), or
 *     RT_AOV_MISS for a ray that hits nothing;
 *   - for j ascending: the first slot with count > 0 and id == v gets count + 1; otherwise the
 *     lowest empty slot becomes (v, 1); otherwise tally.y += 1;
 *   - tally.x += 1.
 * There is no sorting and no eviction: the result depends on the sample order, which is the frame
 * order.  Every word is bit-identical to the CPU restatement in tests/test_matte.py, in both scan
 * modes (rt_set_scan_mode).  max_depth, samples_per_pixel and camera.random_seed are not read
 * (the array replaces the seed).
 *
 * Consequences:
 *   - a call of a + b frames equals a call of a frames followed by a call of b frames with
 *     camera_has_moved 0;
 *   - called with the same seeds and frame counts as rt_update_frames from the same reset (and
 *     fewer samples than samples_per_pixel), tally.x equals the accumulator's alpha and the rays
 *     are the render's camera rays.
 *
 * Arguments and status codes as rt_trace_aov: camera and spheres are host pointers, the spheres
 * are uploaded only when their bytes change, sphere_count == 0 is valid (every sample is
 * background).  The call shares the context's sphere records with the progressive render and
 * nothing else: it neither reads nor rebuilds the candidate lists, tile costs and orders, and
 * leaves rt_last_launch_info, the launch-timing events and the images' known sample counts as
 * they were.  NULL planes, random_seeds or any of the three planes, frames out of range, or a
 * zero width / height give RT_ERR_INVALID_ARGUMENT, and nothing is launched.
 *
 * Out of scope: a foreground-only ("transparent background") beauty image, which needs the colour
 * split by first hit; slot eviction or ranking on the device; feeding coverage into the filters
 * (rt_denoise, rt_variance_filter). */
#define RT_MATTE_MAX_FRAMES 65536u
RT_API rt_status rt_matte_frames(rt_ctx* ctx, const rt_matte_planes* planes, uint32_t width,
                                 uint32_t height, const rt_scene_camera* camera,
                                 const rt_sphere* spheres, uint32_t sphere_count,
                                 const float* random_seeds, uint32_t frames, void* stream);
/* The same over a band set: the planes are compact local buffers of width x (bands->count *
 * RT_STRIPE_ROWS) rows, pixel coordinates stay global (as rt_trace_aov_bands).  Rows past the
 * image's last row are neither read nor written.  A set with count == 0 launches nothing. */
RT_API rt_status rt_matte_frames_bands(rt_ctx* ctx, const rt_matte_planes* planes, uint32_t width,
                                       uint32_t height, const rt_band_set* bands,
                                       const rt_scene_camera* camera, const rt_sphere* spheres,
                                       uint32_t sphere_count, const float* random_seeds,
                                       uint32_t frames, void* stream);

/* The planes resolved for a selection of ids, over pixel_count pixels (a whole image or a band
 * buffer).  selected_ids is a host array of selected_count entries (0 is valid: nothing is
 * selected), each below 2^20 or equal to RT_AOV_MISS (the background); anything else is
 * RT_ERR_INVALID_ARGUMENT.  Outputs, each optional but not both NULL:
 *   alpha     f32 per pixel: f32(s) / f32(tally.x), one IEEE division of the two u32 -> f32
 *             conversions, s the sum of the counts of the non-empty slots whose id is selected; 0
 *             for a pixel with tally.x == 0.  Overflow samples count for nothing: alpha is a
 *             lower bound there, and tally.y says by how much.
 *   dominant  u32 per pixel: the id of the non-empty slot with the largest count, ties to the
 *             lowest slot; RT_AOV_MISS for a pixel with no samples. */
RT_API rt_status rt_matte_resolve(rt_ctx* ctx, const rt_matte_planes* planes,
                                  uint64_t pixel_count, const uint32_t* selected_ids,
                                  uint32_t selected_count, float* alpha, uint32_t* dominant,
                                  void* stream);

/* How the last rt_matte_frames / rt_matte_frames_bands call of the context found its first hits
 * (a diagnostic, as rt_candidate_stats; waits for that call).  Each 8 x 8 tile either walked its
 * own list of the spheres its camera rays can reach, built once per launch, or fell back to the
 * per-frame scan over every sphere (its list overflowed RT_MATTE_LIST_CAPACITY, its cone was
 * degenerate or non-finite, the scene has fewer than 32 spheres, the scan mode is
 * RT_SCAN_EXHAUSTIVE, or RT_MATTE_ROUTE=scan is set in the environment). */
#define RT_MATTE_LIST_CAPACITY 64
typedef struct rt_matte_info {
    uint32_t list_tiles;       /* tiles that walked a list */
    uint32_t fallback_tiles;   /* tiles that fell back */
    uint32_t longest_list;     /* entries of the longest list walked */
    uint32_t overflow_tiles;   /* of the tiles that fell back, those whose list overflowed */
} rt_matte_info;
RT_API rt_status rt_matte_last_info(rt_ctx* ctx, rt_matte_info* out);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_MATTE_H */
