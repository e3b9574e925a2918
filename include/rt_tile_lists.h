/*
 * rt_tile_lists.h — the camera rays' per-tile candidate lists as the list build left them, and
 * the choice of the ray bundle they are built against (librt_hip.so), an addition to the
 * boundary of rt_abi.h (ABI 7): two entry points.  Plain C types only.
 */
#ifndef RT_TILE_LISTS_H
#define RT_TILE_LISTS_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_TILE_LIST_MAX 19u            /* entries a tile's list can hold */
#define RT_TILE_LIST_NONE 0xFFFFFFFFu   /* count of a tile without a list (scanned in full) */
#define RT_TILE_CERTAIN 1u              /* flags bit 0 (rt_certain_tiles.h); bits 1-2: the class */

/* One 8 x 8 tile's list.  Tiles are in the order the kernels index them: local band by local
 * band of the band set the lists were built for, (width + 7) / 8 tiles per band. */
typedef struct rt_tile_list {
    uint32_t count;     /* entries kept, or RT_TILE_LIST_NONE */
    uint32_t removed;   /* entries occlusion culling dropped (rt_occlusion_cull.h) */
    uint32_t flags;     /* the tile's flag word */
    uint32_t reserved;  /* 0 */
    /* the scan record (centre x, y, z, radius squared) of entry j < count, in sphere index
     * order; zero beyond the count */
    float records[RT_TILE_LIST_MAX][4];
} rt_tile_list;

/* Copies the lists built last to the host (it waits for the device): *tiles = their number;
 * out, when not NULL, receives min(*tiles, capacity) of them.  0 tiles before the first trace
 * call of a context and in RT_SCAN_EXHAUSTIVE.  Read-only: nothing on the device changes. */
RT_API rt_status rt_tile_lists(rt_ctx* ctx, rt_tile_list* out, uint64_t capacity,
                               uint64_t* tiles);

/* The bundle of camera rays a tile's list is built against.  1 (default): the two-slope beam
 * between the lens disk and the tile's footprint on the focus plane, the lens disk's radius the
 * largest singular value of (defocus_disk_u, defocus_disk_v).  0: the single cone about the
 * footprint with the lens radius sqrt(|u|^2 + |v|^2), as before the beam: longer lists, fewer
 * certain tiles, identical pixels.  on: 0 or 1.  The setting is part of the lists' key: the
 * next trace call rebuilds them. */
RT_API rt_status rt_set_tight_bundle(rt_ctx* ctx, int on);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_TILE_LISTS_H */
