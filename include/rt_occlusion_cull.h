/*
 * rt_occlusion_cull.h — occlusion culling of the camera rays' per-tile candidate lists
 * (librt_hip.so), an addition to the boundary of rt_abi.h (ABI 7): two entry points.  Plain C
 * types only.
 */
#ifndef RT_OCCLUSION_CULL_H
#define RT_OCCLUSION_CULL_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-tile candidate lists (RT_SCAN_CULLED; rt_candidate_stats) hold every sphere a camera
 * ray of the tile can touch.  With occlusion culling on (the default) the list build also
 * drops every entry that another entry of the same list hides from every camera ray of the
 * tile, for every jitter, lens sample and frame of the camera: the occluder is hit by every
 * ray of the tile from outside, its near root is accepted, and the dropped sphere's roots
 * are larger by more than the f32 error of both.  The dropped sphere can then never be the
 * first hit, so pixel results are identical; only the lists get shorter.  The rule needs the
 * bounded camera and scene domain of the camera-ray-only kernels and switches itself off
 * outside it.  on: 0 or 1.  The setting is part of the lists' key: the next trace call
 * rebuilds them.  RT_SCAN_EXHAUSTIVE is not affected. */
RT_API rt_status rt_set_occlusion_cull(rt_ctx* ctx, int on);
/* Of the lists built last: out[0] = entries occlusion removed, out[1] = tiles that lost at
 * least one entry.  rt_candidate_stats counts what remains. */
RT_API rt_status rt_occlusion_cull_stats(rt_ctx* ctx, uint64_t out[2]);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_OCCLUSION_CULL_H */
