/*
 * rt_certain_tiles.h — certain tiles of the camera rays' per-tile candidate lists
 * (librt_hip.so), an addition to the boundary of rt_abi.h (ABI 7): two entry points.  Plain C
 * types only.
 */
#ifndef RT_CERTAIN_TILES_H
#define RT_CERTAIN_TILES_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where occlusion culling runs (rt_occlusion_cull.h: the setting on, the bounded camera and
 * scene domain), the list build also marks a tile certain when its culled list is one sphere
 * of positive finite radius that every camera ray of the tile certainly hits, for every
 * jitter, lens sample and frame of the camera: from outside, on its front face, with a
 * discriminant that is certainly positive in f32 and a near root that certainly exceeds
 * 0.001.  The frame loops over tile pairs (RT_KERNEL_LIST_PAIR2, RT_KERNEL_LIST_QUAD2) trace a
 * pair of two certain tiles with a straight-line sample that skips the hit test, the root
 * selection, the face test and the material tests, all of them decided at list build: pixel
 * results are identical.  on: 0 or 1, default 1.  The setting is part of the lists' key: the
 * next trace call rebuilds them.  No tile is certain with occlusion culling off, outside its
 * domain, or in RT_SCAN_EXHAUSTIVE. */
RT_API rt_status rt_set_certain_tiles(rt_ctx* ctx, int on);
/* out[0] = certain tiles of the lists built last; out[1] = pairs of two certain tiles among
 * the units of the last tile-pair launch (the pairs that take the straight-line sample; 0 when
 * the lists were rebuilt since, or no such launch has run).  Both 0 in RT_SCAN_EXHAUSTIVE. */
RT_API rt_status rt_certain_tiles_stats(rt_ctx* ctx, uint64_t out[2]);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_CERTAIN_TILES_H */
