/*
 * rt_progress.h — convergence reports and render-to-tolerance (librt_hip.so), an addition to the
 * boundary of rt_abi.h (ABI 7): three entry points and two structs.  Plain C types only.
 * rt_update_adaptive and rt_converge_frames decide per pixel whether it still takes samples;
 * rt_progress_stats classifies every pixel by that same decision and returns the tallies to the
 * host, and rt_progress_run uses them to run rt_converge_frames up to a goal.
 *
 * Every exported symbol of this header contains "progress", and none contains "converge",
 * "adaptive", "variance", "moments", "denoise" or "reproject": those sets are exactly their own
 * headers'.
 */
#ifndef RT_PROGRESS_H
#define RT_PROGRESS_H

#include "rt_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the classification -----------------------------------------------------------------------
 * All of the text below is in f32 as rt_adaptive.h states it (every *, + and - its own IEEE
 * operation, / correctly rounded, subnormals kept), with rt_adaptive.h's L(c) and u32(a).  Per
 * pixel X of the image, with I = image[X]:
 *   n   = u32(I.a)
 *   spp = the call's argument; a caller passes u32(camera->samples_per_pixel)
 *   err = with `moments`: rt_adaptive_error's text for I, moments[X] and min_history (the count
 *         enters it as the float it is: 7.5 stays 7.5);
 *         with `error`:   error[X], any plane rt_update_adaptive accepts
 *   Lm, thr, converged = rt_update_adaptive's text for a camera that has not moved:
 *         Lm = L(I.rgb), thr = abs_tolerance2 + rel_tolerance2 * (Lm * Lm),
 *         converged = n >= min_samples && err <= thr        (a NaN on either side: not converged)
 * The classes, first match; they partition the pixels of the image:
 *   capped     !(n < spp)
 *   converged  n >= min_samples && err <= thr
 *   active     every other pixel: exactly the pixels rt_update_adaptive samples for these
 *              arguments and a camera that has not moved (and rt_converge_frames in a frame that
 *              is not a reset)
 * and of the active pixels
 *   below_min   n < min_samples
 *   no_history  not below_min, and err is +inf
 *
 * Every field of the report is a count, a sum of integers or a maximum, so the report does not
 * depend on the order in which pixels are visited: two calls on the same inputs return the same
 * bytes, on any stream, and the reports of band sets that partition an image combine into the
 * whole image's (counts and `samples` add, min_count, max_count and max_error combine). */
typedef struct rt_progress_report {
    uint64_t pixels;         /* pixels classified: the image's, or the band set's rows on it */
    uint64_t active;
    uint64_t converged;
    uint64_t capped;         /* pixels == active + converged + capped */
    uint64_t below_min;      /* of active */
    uint64_t no_history;     /* of active */
    uint64_t nonfinite;      /* pixels whose r, g or b is NaN or infinite */
    uint64_t samples;        /* the sum of n (one saturated count is 2^32 - 1) */
    uint64_t active_tiles;   /* 8 x 8 tiles with at least one active pixel */
    uint32_t min_count;      /* of n; 0xFFFFFFFF when pixels is 0 */
    uint32_t max_count;      /* of n; 0 when pixels is 0 */
    float    max_error;      /* the largest err with err < +inf (a NaN is not); compared as floats
                                with +0 above -0; -inf when there is no such pixel */
    uint32_t _reserved[3];   /* 0 */
} rt_progress_report;
#ifdef __cplusplus
static_assert(sizeof(rt_progress_report) == 96, "rt_progress_report is 96 bytes");
#else
_Static_assert(sizeof(rt_progress_report) == 96, "rt_progress_report is 96 bytes");
#endif

/* ---- rt_progress_stats ------------------------------------------------------------------------
 * Classifies the width x height RGBA32F device image `image` and writes the report to the host
 * memory at `out_report`.  Exactly one of `moments` (rt_variance.h's image of the same size) and
 * `error` (width * height floats) is non-NULL; min_history is read with `moments` only.
 *
 * `tile_active` is optional (NULL: not wanted): one uint64_t per 8 x 8 tile in
 * rt_update_adaptive's tile_mask layout, ceil(width / 8) * ceil(height / 8) words, tile rows
 * first.  Bit (y & 7) * 8 + (x & 7) of the word of tile (x / 8, y / 8) is set when pixel (x, y)
 * is active; bits of lanes off the image are 0; every word is written.
 *
 * The call is synchronous, as rt_pick is: two kernel launches on `stream` (one wave per tile at
 * a time over a bounded grid, each workgroup leaving one partial record; then one workgroup that
 * folds the records), one asynchronous copy of the report from a block the context owns on the
 * device to a pinned block it owns on the host, and one synchronisation of `stream`.  The inputs
 * are only read.  Calls on one context must not overlap.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: image, params or out_report NULL;
 * both or neither of moments and error; tile_active equal to image, moments or error;
 * min_samples above 16777216; a tolerance negative, NaN or infinite; with moments, min_history
 * outside 1..16777216.  RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused call
 * launches nothing and leaves *out_report as it was.  It touches no render state. */
RT_API rt_status rt_progress_stats(rt_ctx* ctx, const float* image, const float* moments,
                                   const float* error, uint64_t* tile_active, uint32_t width,
                                   uint32_t height, uint32_t spp,
                                   const rt_adaptive_params* params, uint32_t min_history,
                                   void* stream, rt_progress_report* out_report);

/* The same over a band set, as rt_update_adaptive_bands: `image`, `moments`, `error` and
 * `tile_active` are compact local buffers of bands->count * 8 rows (tile_active:
 * ceil(width / 8) * bands->count words), local band j being global band
 * bands->first + j * bands->step.  Only rows that lie on the image are counted: the rows of a
 * last, ragged band below the image are not pixels, and their bits are 0.  count == 0 launches
 * nothing and returns the report of no pixels.  Also RT_ERR_INVALID_ARGUMENT: bands NULL or not
 * a band set of the image. */
RT_API rt_status rt_progress_stats_bands(rt_ctx* ctx, const float* image, const float* moments,
                                         const float* error, uint64_t* tile_active,
                                         uint32_t width, uint32_t height,
                                         const rt_band_set* bands, uint32_t spp,
                                         const rt_adaptive_params* params, uint32_t min_history,
                                         void* stream, rt_progress_report* out_report);

/* ---- rt_progress_run --------------------------------------------------------------------------
 * Runs rt_converge_frames until at most max_active pixels are active, or max_frames frames have
 * run, looking every check_every frames. */
typedef struct rt_progress_goal {
    uint64_t max_active;     /* stop once report.active <= max_active */
    uint32_t max_frames;     /* 1..65536: the frames run at most */
    uint32_t check_every;    /* 1..65536: frames per rt_converge_frames call, between two reports */
} rt_progress_goal;
#ifdef __cplusplus
static_assert(sizeof(rt_progress_goal) == 16, "rt_progress_goal is 16 bytes");
#else
_Static_assert(sizeof(rt_progress_goal) == 16, "rt_progress_goal is 16 bytes");
#endif

/* Whole images only.  `random_seeds` holds goal->max_frames floats.  The call is this loop, with
 * stats = rt_progress_stats(image, moments, error NULL, spp = u32(camera->samples_per_pixel),
 * params, min_history), and nothing else writes `image` or `moments`:
 *
 *   done = 0
 *   if !(camera->camera_has_moved > 0.5):
 *       report = stats()
 *       if report.active <= max_active: return (0, report)
 *   loop:
 *       f = min(check_every, max_frames - done)
 *       rt_converge_frames(image, moments, NULL, NULL, NULL, frames = f, random_seeds + done,
 *                          camera_has_moved as given only when done == 0, else 0)
 *       done += f
 *       report = stats()
 *       if report.active <= max_active or done == max_frames: break
 *   return (done, report)
 *
 * *frames_run receives `done` and *out_report the last report; `tile_active` (optional, as
 * above) belongs to the last report.  A camera that has moved gets no first report: its frame 0
 * is a reset, which the classification does not describe.  `image` and `moments` are, bit for
 * bit, what one rt_converge_frames call of `done` frames leaves (that call's text makes a split
 * call equal an unsplit one); with done == 0 they are untouched.
 *
 * A loop over several ranks is the caller's: per rank rt_converge_frames_bands and
 * rt_progress_stats_bands, then the sum of `active` across the ranks, which the decision to stop
 * needs.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: image, moments, camera,
 * random_seeds, params, goal, frames_run or out_report NULL; image equal to moments; tile_active
 * equal to image or moments; max_frames or check_every outside 1..65536; min_history outside
 * 1..16777216; min_samples above 16777216; a tolerance negative, NaN or infinite.
 * RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused call launches nothing and
 * leaves *frames_run and *out_report as they were.  An error rt_converge_frames itself reports
 * (the spheres, the device) is returned as it is, with both left as they were.  The render state
 * it touches is rt_converge_frames'. */
RT_API rt_status rt_progress_run(rt_ctx* ctx, float* image, float* moments,
                                 uint64_t* tile_active, uint32_t width, uint32_t height,
                                 const rt_scene_camera* camera, const rt_sphere* spheres,
                                 uint32_t sphere_count, const float* random_seeds,
                                 const rt_adaptive_params* params, uint32_t min_history,
                                 const rt_progress_goal* goal, void* stream,
                                 uint32_t* frames_run, rt_progress_report* out_report);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_PROGRESS_H */
