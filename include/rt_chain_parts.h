/*
 * rt_chain_parts.h — chain parts of rt_update_frames (librt_hip.so), an addition to the
 * boundary of rt_abi.h (ABI 7): two entry points and one struct.  Plain C types only.
 */
#ifndef RT_CHAIN_PARTS_H
#define RT_CHAIN_PARTS_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Chain parts: an rt_update_frames call that needs two or more fused launches (frames above
 * the frames-per-launch cap), every one a frame-group launch (rt_set_frame_pairs not OFF, the
 * camera-ray-only case, the images' sample count known to the context), as two chains of
 * launches over disjoint halves of the image.  Between two launches of one chain the first
 * must drain: its last round of workgroups leaves SIMDs short of waves.  The call's scheduling
 * units (tiles, or tile pairs), in the order the launches would use anyway (cost order, else
 * raster), are dealt alternately to two parts; part 0 runs its launches on the caller's stream
 * and part 1 on a context-owned stream, forked from and joined back into the caller's stream
 * by events inside the call, exactly as the one-frame parts of rt_set_update_queues.  A part's
 * pixels are read and written by that part alone for the whole call, and the parts' launch
 * boundaries are staggered (rt_chain_schedule) so that one part drains while the other is in
 * mid-launch.  0 = automatic (two parts for launches of 4 000 tiles or more: a whole
 * 1920x1080 image down to its 8-rank share, each measured faster; one chain below), 1 = one
 * chain, 2 = two parts wherever the conditions hold; above RT_MAX_CHAIN_PARTS is an error.
 * The context's first call of a share that may split creates part 1's stream and events.
 * A call that fits one launch is one launch in every mode, and while rt_set_launch_timing is
 * enabled every call is one chain (its kernel time is defined per sequential launch).
 * rt_launch_info.chain_parts reports what the last call ran; `queues` keeps its meaning.
 * Pixel results are identical. */
#define RT_MAX_CHAIN_PARTS 2u
RT_API rt_status rt_set_chain_parts(rt_ctx* ctx, uint32_t parts);
/* The launches of such a call (host only, no context): launch i runs frames [first, first +
 * frames) of the call for part `part`, in issue order.  Every part covers every frame once, in
 * order; no launch is above `cap` frames or (in a two-part schedule) below two; no boundary
 * of one part is a boundary of the other except frame 0 and the end.  frames <= cap, or
 * cap < 4: the single chain (part 0 only, launches of cap frames).  variant 0 = the library's
 * choice (4), 1 = each part ends with a short launch (cap / 4 and cap / 8 frames), 2 = plain
 * stagger (part 1's first launch is cap / 2, every other launch cap, the remainders last),
 * 3 = as 2 with a short last launch for part 1, 4 = as 2 with part 1's first launch 3 cap / 4.
 * *out_count receives the launches; RT_ERR_INVALID_SIZE when they exceed max_out. */
typedef struct rt_chain_launch {
    uint32_t part, first, frames;
} rt_chain_launch;
RT_API rt_status rt_chain_schedule(uint32_t frames, uint32_t cap, int variant,
                                   rt_chain_launch* out, uint32_t max_out, uint32_t* out_count);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_CHAIN_PARTS_H */
