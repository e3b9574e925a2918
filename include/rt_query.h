/*
 * rt_query.h — ray queries against the uploaded scene (librt_hip.so): closest hit and
 * occlusion for rays the caller chooses, an addition to the boundary of rt_abi.h (ABI 7): two
 * entry points and two structs.  Plain C types only.  It is the general form of rt_aov.h's
 * rt_pick: the same scans and the same record, for any ray instead of a camera's.
 */
#ifndef RT_QUERY_H
#define RT_QUERY_H

#include "rt_abi.h"
#include "rt_aov.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One ray: 32 bytes, read by the device as two 16-byte loads. */
typedef struct rt_ray {
    float    o[3];       /* origin */
    float    tmax;       /* upper bound of t (below) */
    float    d[3];       /* direction, not normalised */
    uint32_t _reserved;  /* ignored */
} rt_ray;

/* Results, one element per ray, tightly packed device buffers; NULL = not wanted.
 *   sphere_id  u32       index of the winning sphere           miss: RT_AOV_MISS
 *   hit        4 x f32   p.x, p.y, p.z, t                      miss: 0, 0, 0, +inf
 *   normal     4 x f32   n.x, n.y, n.z, front ? 1 : 0          miss: 0, 0, 0, 0
 *   material   4 x f32   the sphere's color[4] verbatim        miss: 0, 0, 0, 0
 *   occluded   u32       1 / 0; RT_QUERY_OCCLUSION only
 * The first four hold exactly the values of rt_aov.h's planes. */
typedef struct rt_query_planes {
    uint32_t* sphere_id;
    float*    hit;
    float*    normal;
    float*    material;
    uint32_t* occluded;
} rt_query_planes;

#define RT_QUERY_CLOSEST   0u
#define RT_QUERY_OCCLUSION 1u

/* RT_QUERY_CLOSEST.  For ray r let T = r.tmax < 3.4e35f ? r.tmax : 3.4e35f: NaN, +inf and
 * anything larger give the shader's own 3.4e35 (wgsl:266); a T <= 0.001 can accept nothing.
 * The result is sphere_list_hit (wgsl:164-221) over the uploaded spheres in index order with
 * tmin = 0.001 and the running tmax started at T: a root at or beyond T is rejected (wgsl:196's
 * "tmax <= root"), and a later sphere wins only if strictly nearer.  p = fma(t, d, o), outward =
 * (p - C) / R (IEEE division), front = dot(d, outward) < 0, n = front ? outward : -outward.
 * Every float equals what the CPU oracle's sphere_hit leaves when chained that way, NaN for
 * NaN, in both scan modes (rt_set_scan_mode) — rays with d = 0 and with non-finite o, d or
 * roots included: such rays take the scan that accepts them as the shader does.  tmin is not a
 * parameter: it is part of the proven root selections.
 *
 * The bound and the fast roots.  The culled scans test spheres in another order than the
 * shader's, and some waves find their roots with exact fast cores instead of the IEEE sqrt and
 * divisions.  Both are proven for any incoming bound, not only for the sentinel: a root is the
 * IEEE root bit for bit whenever it exceeds 0.001, and is at or below 0.001 with either
 * arithmetic otherwise, so its comparison with the running tmax — which T only seeds, exactly
 * as an earlier, nearer hit would have — is the shader's.  In the any-order scans a root equal
 * to T is refused because no sphere has been accepted yet (the tie goes to the lower index, and
 * "none" is lower than every index).  rt_selftest_roots replays the selections with incoming
 * bounds between, below and on the roots.
 *
 * RT_QUERY_OCCLUSION.  occluded[r] = 1 exactly when RT_QUERY_CLOSEST reports a hit for r.  A
 * sphere that passes its own test against T is accepted by whichever walk meets it first, so the
 * answer does not depend on the scan order and the scan stops at the first acceptance.  In this
 * mode the four record planes must be NULL and `occluded` non-NULL; in RT_QUERY_CLOSEST
 * `occluded` must be NULL and at least one other plane non-NULL.
 *
 * rays and the planes are device pointers; spheres is a host pointer, uploaded only when the
 * bytes change (as rt_trace_aov).  sphere_count == 0 is valid (every ray misses); count == 0
 * launches nothing.  One lane per ray, 64 consecutive rays per wave; each wave takes, by the
 * library's bounce-ray rule, the XZ sphere grid, else its rays' cone, else the exhaustive walk
 * (RT_SCAN_EXHAUSTIVE: always the walk).  route_counts (device, 3 words, may be NULL; the
 * caller zeroes it) receives one atomic add per wave that scans: [0] grid, [1] cone, [2]
 * exhaustive; their sum is ceil(count / 64).  It is a diagnostic, no part of the result.
 *
 * Like the rt_aov.h calls, the call shares the context's sphere records and grid with the
 * render and nothing else: candidate lists, tile costs and orders, rt_last_launch_info, the
 * launch-timing events and the images' known sample counts stay as they were.
 *
 * A refused call launches nothing.  RT_ERR_INVALID_CONTEXT: ctx is NULL.
 * RT_ERR_INVALID_ARGUMENT: rays NULL with count > 0, planes NULL, mode above 1, a plane set
 * that does not fit the mode, spheres NULL with sphere_count > 0.  RT_ERR_INVALID_SIZE: count
 * above 2^32 - 64 (one grid row of four-wave workgroups). */
RT_API rt_status rt_cast_rays(rt_ctx* ctx, const rt_ray* rays, uint64_t count, uint32_t mode,
                              const rt_query_planes* planes, const rt_sphere* spheres,
                              uint32_t sphere_count, uint32_t* route_counts, void* stream);

/* One ray from the host (RT_QUERY_CLOSEST): the record rt_cast_rays writes for it, from a
 * launch of one wave with one live lane; a miss as rt_pick's.  ray or out NULL is
 * RT_ERR_INVALID_ARGUMENT.  Synchronous on `stream` (returns after the record is on the
 * host). */
RT_API rt_status rt_cast_ray(rt_ctx* ctx, const rt_ray* ray, const rt_sphere* spheres,
                             uint32_t sphere_count, void* stream, rt_pick_result* out);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_QUERY_H */
