/*
 * rt_scene_edit.h — carries the accumulator across an edit of the scene: spheres moved, resized,
 * recoloured, deleted or inserted between the previous frame and the current one, the camera
 * moved or not (librt_hip.so), an addition to the boundary of rt_abi.h (ABI 7): four entry
 * points and four structs.  It reuses rt_reproject.h's planes, parameters and basis.  Plain C
 * types only.
 *
 * rt_edit_plan (host, no device) compares the two sphere arrays and writes a table: one record
 * per current sphere, saying which previous sphere's history it may take and how its surface
 * points map back, then the balls around everything that changed, inside which lighting may
 * have changed and history is held to a short count.  The caller copies the table to the device;
 * rt_edit_carry is rt_reproject with that table.
 */
#ifndef RT_SCENE_EDIT_H
#define RT_SCENE_EDIT_H

#include <stddef.h>

#include "rt_abi.h"
#include "rt_reproject.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_EDIT_NONE      0xFFFFFFFFu  /* no previous sphere / no owner / restart          */
#define RT_EDIT_MOVED     0x80000000u  /* bit 31 of a link: the geometry differs           */
#define RT_EDIT_MAX_BALLS 32u
#define RT_EDIT_MAX_SPHERES (1u << 20) /* largest n_prev and n_cur rt_edit_plan takes      */

typedef struct rt_edit_record {
    float    prev_center[3];  /* the previous sphere's position (the current one's without one) */
    float    scale;           /* previous radius / current radius (1 without a previous sphere) */
    float    center[3];       /* the current sphere's position                                  */
    uint32_t link;            /* RT_EDIT_NONE, or the previous index, | RT_EDIT_MOVED           */
} rt_edit_record;             /* 32 bytes */

typedef struct rt_edit_ball {
    float    center[3];
    float    radius2;         /* squared radius of the ball                                     */
    uint32_t owner;           /* the current sphere whose own pixels it spares, or RT_EDIT_NONE */
    uint32_t _pad[3];         /* 0                                                              */
} rt_edit_ball;               /* 32 bytes */

typedef struct rt_edit_params {
    rt_reproject_params carry;   /* rt_reproject's parameters, with their meaning there         */
    uint32_t edit_history;       /* 0 .. carry.max_history: cap on the count inside a ball      */
    float    influence;          /* >= 0, finite: a ball's radius in radii of its sphere        */
    uint32_t _reserved[2];       /* must be 0                                                   */
} rt_edit_params;                /* 32 bytes */
/* carry = rt_reproject_params_default's, edit_history 4, influence 3.0f; NULL is a no-op.  The
 * two numbers come from a CPU prototype (a radius-1 sphere of the 40-sphere
 * scene moved by half a radius, 16 frames of history, against 512 samples of the edited scene),
 * not from a sweep. */
RT_API void rt_edit_params_default(rt_edit_params* p);

typedef struct rt_edit_info {
    uint32_t n_records;     /* = n_cur                                                          */
    uint32_t n_balls;       /* 0 .. RT_EDIT_MAX_BALLS                                           */
    uint32_t n_changed;     /* current spheres that are not unchanged (below)                   */
    uint32_t n_moved;       /* records whose link has RT_EDIT_MOVED                             */
    uint32_t n_restart;     /* records whose link is RT_EDIT_NONE                               */
    uint32_t n_deleted;     /* previous spheres that no current sphere names                    */
    uint32_t full_restart;  /* 1: more than RT_EDIT_MAX_BALLS balls were needed                 */
    uint32_t _reserved;     /* 0                                                                */
} rt_edit_info;             /* 32 bytes */

/* The table's capacity in bytes for n_cur current spheres: 32 * (n_cur + RT_EDIT_MAX_BALLS). */
RT_API size_t rt_edit_plan_bytes(uint32_t n_cur);

/* Host only, pure, no device.  prev_spheres[n_prev] is the scene of the previous frame,
 * spheres[n_cur] the current one.  prev_index[i] is the index current sphere i had in the
 * previous scene, or RT_EDIT_NONE for a new sphere; NULL stands for the identity and requires
 * n_prev == n_cur.  `table` receives n_cur records followed by info->n_balls balls; the rest of
 * its rt_edit_plan_bytes(n_cur) bytes are set to 0.
 *
 * All arithmetic is f32.  For current sphere i, S = spheres[i], j = prev_index[i] and, when
 * j != RT_EDIT_NONE, S' = prev_spheres[j]:
 *   same geometry: the three position words and the radius word of S and S' are bit-equal
 *                  (so -0 and +0 differ, and a NaN equals itself);
 *   same material: the four colour words are bit-equal;
 *   unchanged:     both.
 * The record is center = S.position and, with a j, prev_center = S'.position and
 * scale = S'.radius / S.radius (IEEE f32 division, whatever it gives); without one,
 * prev_center = S.position and scale = 1.  Its link is
 *   j                    when unchanged;
 *   j | RT_EDIT_MOVED    when the material is the same, the geometry differs, both radii are
 *                        finite and nonzero and scale is finite and > 0 (equal signs);
 *   RT_EDIT_NONE         otherwise: the material differs, there is no j, or a radius is unfit.
 *
 * Balls, in this order.  (1) For i ascending, every current sphere that is not unchanged: the
 * new ball (S.position, radius2 = t * t with t = influence * fabsf(S.radius), owner i) and then,
 * if it has a j and the geometry differs, the old ball (S'.position, t = influence *
 * fabsf(S'.radius), owner i).  (2) For j ascending, every previous sphere no prev_index entry
 * names (a deleted sphere): its old ball, owner RT_EDIT_NONE.
 *
 * More than RT_EDIT_MAX_BALLS balls: full_restart = 1, every link is RT_EDIT_NONE
 * (n_restart = n_cur, n_moved = 0) and there are no balls; rt_edit_carry then writes zeros
 * everywhere by its ordinary rules.  n_changed and n_deleted are counted either way.
 *
 * RT_ERR_INVALID_ARGUMENT: params, table or info NULL; spheres NULL with n_cur > 0 or
 * prev_spheres NULL with n_prev > 0; table_bytes < rt_edit_plan_bytes(n_cur); prev_index NULL
 * with n_prev != n_cur; an entry >= n_prev that is not RT_EDIT_NONE; a previous index named
 * twice; influence negative, NaN or infinite; edit_history > carry.max_history; a reserved word
 * (params->_reserved, params->carry._reserved) nonzero; n_prev or n_cur above
 * RT_EDIT_MAX_SPHERES.  n_cur = 0 and n_prev = 0 are valid.  A refused call writes nothing. */
RT_API rt_status rt_edit_plan(const rt_sphere* prev_spheres, uint32_t n_prev,
                              const rt_sphere* spheres, uint32_t n_cur,
                              const uint32_t* prev_index, const rt_edit_params* params,
                              void* table, size_t table_bytes, rt_edit_info* info);

/* rt_reproject (rt_reproject.h) with a plan: writes every pixel of the width x height RGBA32F
 * device image `dst_rgba` from the previous frame's accumulator `prev_rgba`, one kernel launch
 * on `stream`; nothing else is written.  The previous planes are rt_trace_aov's for the previous
 * scene and the previous camera, the current planes its planes for the current scene and the
 * current camera, which may differ too.  `plan_dev` is the device copy of rt_edit_plan's table:
 * n_records records, then n_balls balls.  The basis, o', r0, r1, r2, and the arithmetic are
 * rt_reproject.h's: f32, every *, + and - its own IEEE operation (no contraction, no fma), /
 * correctly rounded, subnormals kept.  Every output bit equals a CPU restatement of this text
 * (tests/test_scene_edit.py).
 *
 * Per pixel P = (x, y).  Let id = sphere_id[P], p = hit[P].xyz, nP = normal[P].xyz,
 * max_history, lambertian_only and position_tolerance2 those of params->carry.  The result is
 * "no history", dst[P] = (0, 0, 0, 0), when any of these holds, tested in this order:
 *   1.  id == RT_AOV_MISS
 *   1b. id >= n_records (a stale id plane; the record is not read), or, with
 *       rec = records[id], rec.link == RT_EDIT_NONE
 *   2.  lambertian_only and !(material[P].w < -1)
 *   2b. near and edit_history == 0, where near is true when some ball B = balls[k],
 *       k < n_balls, has B.owner != id and
 *       ((p.x - B.center.x)^2 + (p.y - B.center.y)^2) + (p.z - B.center.z)^2 < B.radius2
 *       (each difference squared by one multiplication, summed in the order written; a NaN
 *       fails the comparison)
 *   3.  !(c > 0), with q = p' - o' per component (o' as f32),
 *       a = (r0.x*q.x + r0.y*q.y) + r0.z*q.z, and likewise b with r1 and c with r2
 *   4.  not (px >= -1 && px < (float)width && py >= -1 && py < (float)height), where
 *       px = a / c - 0.5f and py = b / c - 0.5f (written so that NaN fails)
 *   5.  no tap is kept (below).
 *
 * The point in the previous scene, p'.  If rec.link has RT_EDIT_MOVED,
 *   p'.c = rec.prev_center.c + (p.c - rec.center.c) * rec.scale   for c in x, y, z
 * (a subtraction, a multiplication, an addition); otherwise p' = p bit for bit, so a plan of
 * unchanged spheres and no balls gives rt_reproject's output exactly.  nP is used as it is: a
 * translated and positively scaled sphere keeps its normals.
 *
 * Taps.  fx = floorf(px), fy = floorf(py), tx = px - fx, ty = py - fy, x0 = (int)fx,
 * y0 = (int)fy, r2q = (q.x*q.x + q.y*q.y) + q.z*q.z, lim = position_tolerance2 * r2q.  The taps
 * are Q = (x0 + i, y0 + j), j = 0, 1 outer and i = 0, 1 inner, with the bilinear weight
 * bw = (j ? ty : 1 - ty) * (i ? tx : 1 - tx).  A tap is skipped when
 *   - it is off the image;
 *   - prev_sphere_id[Q] != (rec.link & 0x7FFFFFFF);
 *   - !(dl * dl <= lim), where e = p' - prev_hit[Q].xyz and
 *     dl = (nP.x*e.x + nP.y*e.y) + nP.z*e.z;
 *   - !(prev_rgba[Q].a > 0);
 *   - !(bw > 0).
 * Kept taps accumulate in tap order: sw += bw, sum.c += bw * prev_rgba[Q].c for c in rgb,
 * n = min(n, prev_rgba[Q].a) starting from +inf.  Then dst[P].rgb = sum.rgb / sw and
 * dst[P].a = min(n, near ? (float)edit_history : (float)max_history).  A non-finite colour in a
 * kept tap propagates into dst[P]; a NaN in p or nP fails the tests it enters.
 *
 * A ball does not apply to its owner's own pixels: a sphere that only moved takes its own
 * surface's history at the full count, while what lies around its old and new places, where its
 * shadow and its reflections changed, is held to edit_history samples and converges to the new
 * lighting quickly.  A moments image (rt_variance.h) is carried by a second call, as with
 * rt_reproject.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: params NULL or anything
 * rt_reproject refuses of the other arguments and of params->carry; plan_dev NULL unless
 * n_records + n_balls == 0; n_balls > RT_EDIT_MAX_BALLS; n_records > RT_EDIT_MAX_SPHERES;
 * edit_history > carry.max_history; params->_reserved nonzero.  (influence is rt_edit_plan's
 * and is not looked at.)  RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused
 * call launches nothing.
 *
 * Like rt_reproject it takes whole images only, touches no candidate lists, tile orders, launch
 * info or timing events and no scene state of the context, and makes the context forget the
 * uniform sample count it may know for dst_rgba. */
RT_API rt_status rt_edit_carry(rt_ctx* ctx, const float* prev_rgba, float* dst_rgba,
                               uint32_t width, uint32_t height,
                               const rt_scene_camera* prev_camera,
                               const rt_reproject_planes* planes, const void* plan_dev,
                               uint32_t n_records, uint32_t n_balls,
                               const rt_edit_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_SCENE_EDIT_H */
