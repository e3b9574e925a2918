// rt_occlusion.h — occlusion culling of a tile's candidate list at list build
// (rt_kernels.hip rt_candidates_kernel).  Device code, included by the
// render kernels' unit only and used by the list build alone: the per-frame kernels read
// shorter lists and are not otherwise touched.
//
// beam_misses() asks whether a camera ray of the tile could touch a sphere; it never asks
// whether the sphere could be the first hit.  An entry O of a tile's list is dropped when
// another entry S of the same list provably wins against it in every lane and frame:
//   (a) every ray of the tile's bundle hits S with a discriminant that is certainly positive
//       in f32, from outside S, heading towards it, and S's near root certainly exceeds
//       0.001, so every lane accepts S's near root unless tmax is already below it;
//   (b) the computed root of O (either root) certainly exceeds S's computed near root in
//       every lane.
// Then O is never the winner of sphere_list_hit, whatever the two indices: before S, S
// replaces it (root_S < root_O = tmax); after S, O fails `tmax <= root` (tmax <= root_S).
// The separation is strict, so the first-index tie rule never decides between them.
//
// The bundle of a tile (footprint_beam, rt_trace_device.h): every ray's line lies in the union
// of the balls of radius rho(t) about the axis point at t from the apex (the footprint centre on
// the focus plane; rho: the two-slope beam, or with rt_set_tight_bundle off the single cone),
// every direction lies within theta of the axis (sin theta = the beam's far slope), and every
// origin lies within rl of the camera centre (bundle_lens: the lens radius of lens_radius(),
// widened as footprint_beam widens its own).  For a sphere (C, R), a ray with origin o and unit
// direction u: s = |C - o|, dl = the distance of C from the ray's line.  A ray that heads
// towards C from outside hits at distance near(s, dl) = sqrt(s^2 - dl^2) - sqrt(R^2 - dl^2),
// increasing in s and in dl (R < s), and evaluated as (s - R)(s + R) / (sqrt(s^2 - dl^2)
// + sqrt(R^2 - dl^2)) without cancellation (the ground: s - R = 2 of 1000).  Over the bundle
// s lies in [D - rl, D + rl] (D = |C - centre|).  dl lies in [p cos - rho(t), p + rho(t)]
// (t, p: C along and across the axis from the apex): the lower end is beam_misses' bound; the
// upper end holds because the line's point with the axis parameter of t lies within rho(t) of
// the axis point at t, which lies p from C, and dl is at most the distance to any point of the
// line.  So near() at the lower corner bounds O's near hit from below and near() at the upper
// corner bounds S's from above (never above the tangent length).  `ahead`: with tc, pc the
// centre along and across the axis from the camera centre, (C - o).u >= tc cos - pc sin - rl
// for every direction within theta of the axis and every origin within rl of the centre.
//
// f32 error of the computed root, as a distance (root |d|; both roots of a lane share d and
// the computed a, so comparing distances compares roots): the discriminant's error is
// E' = eps |d|^2 (16 s^2 + 6 R^2), so sqrt(D)/|d| errs by at most E'/q where
// the true q = sqrt(R^2 - dl^2) is known to be at least q, and by at most sqrt(E') anywhere;
// h, the subtraction, a and the division add less than 9 eps (s + R).  occ_bounds() takes
// E = 2e-6 (s^2 + R^2) >= 2 E' and 1e-6 (s + R) > 16 eps (s + R).
//
// Certain tiles (certainly_front below).  A tile whose culled list is one entry S
// with (a), of positive finite radius, needs no hit test in the frame loop: every lane's walk
// ends with index 0 and S's near root.  The frame loop's straight-line sample also skips the
// face test (wgsl:210-216), so the list build proves its outcome too: the computed
// dot(d, outward) is negative in every lane.  With u = d / |d| the true value is -|d| q / R,
// q = sqrt(R^2 - dl^2) the half chord, at least q_lo = sqrt(R^2 - dl_hi^2) (q_lo^2 > E by
// `inside`).  The computed value, scaled by R / |d|, differs from -q by at most
//   D   the computed root's error as a distance, along u itself: at most `err` above;
//   2^-24 (l1(C) + 3 (R + D))   the fma of hp = o + root d, a single rounding per component of a
//       value within R + D of C (the camera and the centre may lie far from the origin: this
//       term scales with the coordinates, not with s);
//   2^-24 sqrt(3) (R + D)   the subtraction rel = hp - C;
//   2^-24 2 R   the division by R (correctly rounded by either form, normal_div or IEEE);
//   2^-24 4 R   the dot product's three roundings, each of a partial sum of at most |d| 1.01;
// together less than err + 1e-6 (l1(C) + R).  certainly_front() asks for twice that under
// 0.9 q_lo (q2's own f32 error is at most 2 eps R^2 < 0.06 E, and the hardware square root's
// an ulp).  Nothing here can underflow: |d|^2 >= 2^-11 (camera_rays_bounded) and q / R >
// sqrt(2e-6), so the sum's leading term is far above the normal range's floor.
#pragma once

#include "rt_trace_device.h"

namespace rtk {

__device__ __forceinline__ v3 cross3(v3 a, v3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float l1(v3 v) { return fabsf(v.x) + fabsf(v.y) + fabsf(v.z); }

// What the occlusion rule needs beyond the tile's Beam: the camera centre and the radius of
// the lens disk about it, widened exactly as footprint_beam widens its own.
struct Lens {
    v3 ctr;
    float rl;
};
__device__ __forceinline__ Lens bundle_lens(const TraceParams& p, const Beam& k, bool parent) {
    Lens b;
    b.ctr = mk(p.center[0], p.center[1], p.center[2]);
    const float rl = lens_radius(p, parent);
    b.rl = rl * 1.001f + 1e-5f * (l1(k.apex) + l1(b.ctr));
    return b;
}

// One entry's bounds over the tile's bundle, as distances along the rays:
//   lo  <= the computed near root of any ray that the entry could win with (-inf: unknown)
//   hi  >= the computed near root of every ray, valid when `covers`
//   covers: (a) above holds for this entry
//   q2, err: R^2 - dl_hi^2 and the root's error bound, for certainly_front (valid when `covers`)
struct OccBounds {
    float lo, hi;
    bool covers;
    float q2, err;
};
__device__ __forceinline__ OccBounds occ_bounds(const Beam& k, const Lens& b, float4 g) {
    OccBounds r;
    r.lo = -__builtin_inff();
    r.hi = __builtin_inff();
    r.covers = false;
    r.q2 = r.err = 0.0f;
    const v3 C = mk(g.x, g.y, g.z);
    const float R2 = g.w, R = __builtin_amdgcn_sqrtf(g.w);        // |radius|
    // the ray lines, from the apex (the cross product: no cancellation in p)
    const v3 v = sub(C, k.apex);
    const float t = dot(v, k.axis), at = fabsf(t), p = len3(cross3(v, k.axis));
    const float spread = beam_spread(k, t);   // rho(t) - r_o, the beam at the centre's position
    const float sl = 1e-5f * (at + p + k.r_o) + 1e-6f * (l1(C) + l1(k.apex));
    const float dl_hi = p + spread + k.r_o + sl;
    const float dl_lo = fmaf(p, k.cos_t, -spread) - k.r_o - sl;
    // the origins, from the camera centre
    const v3 w = sub(C, b.ctr);
    const float D = len3(w), tc = dot(w, k.axis), pc = len3(cross3(w, k.axis));
    const float sd = 1e-5f * D + 1e-6f * (l1(C) + l1(b.ctr));
    const float s_hi = D + b.rl + sd, s_lo = D - b.rl - sd;
    // every ray heads towards C (oc.u > 0) from outside the sphere
    const bool ahead = tc * k.cos_t - pc * k.sin_t - b.rl - sd > 0.0f && s_lo > R * 1.0001f;
    if (!ahead || !__builtin_isfinite(s_hi + dl_hi + R)) return r;
    const float E = 2e-6f * fmaf(s_hi, s_hi, R2);
    const float q2 = R2 - dl_hi * dl_hi;      // <= R^2 - dl^2 of every ray
    const bool inside = q2 > E;               // the discriminant is certainly positive
    const float err = 1e-6f * (s_hi + R) +
                      (inside ? E * __builtin_amdgcn_rsqf(q2) * 1.0001f
                              : __builtin_amdgcn_sqrtf(E) * 1.0001f);
    {   // near(s_lo, dl_lo), the denominator rounded up
        const float dl = fminf(fmaxf(dl_lo, 0.0f), R);
        const float num = (s_lo - R) * (s_lo + R);
        const float den = __builtin_amdgcn_sqrtf(fmaf(-dl, dl, s_lo * s_lo) * 1.000001f +
                                                 1e-6f * s_lo * s_lo) +
                          __builtin_amdgcn_sqrtf(fmaxf(fmaf(-dl, dl, R2), 0.0f) + 1e-6f * R2);
        r.lo = num / den * 0.9999f - err;
    }
    if (inside) {   // near(s_hi, dl_hi), the denominator rounded down
        const float num = (s_hi - R) * (s_hi + R);
        const float den =
            __builtin_amdgcn_sqrtf(fmaxf(fmaf(-dl_hi, dl_hi, s_hi * s_hi) - 1e-6f * s_hi * s_hi,
                                         0.0f)) +
            __builtin_amdgcn_sqrtf(fmaxf(q2 - 1e-6f * R2, 0.0f));
        const float tangent = __builtin_amdgcn_sqrtf(num);
        r.hi = fminf(num / den, tangent) * 1.0001f + err;
        // the near root (distance / |d|, |d| <= d_max) certainly exceeds 0.001
        r.covers = s_lo - R - err > 1.1e-3f * k.d_max && __builtin_isfinite(r.hi);
        r.q2 = q2;
        r.err = err;
    }
    return r;
}

// The computed dot(d, outward) of an entry with `covers` is negative in every lane (the
// header's argument).  g: the entry's scan record, b: its bounds.
__device__ __forceinline__ bool certainly_front(const OccBounds& b, float4 g) {
    const float R = __builtin_amdgcn_sqrtf(g.w);
    return b.covers && 0.9f * __builtin_amdgcn_sqrtf(b.q2) >
                           2.0f * (b.err + 1e-6f * (l1(mk(g.x, g.y, g.z)) + R));
}

// The material class of a tile's flag word (rt_kernels.h), as ray_color tests albedo.w
// (wgsl:272-280; a NaN is a dielectric there)
__device__ __forceinline__ uint32_t material_class(float w) {
    return w < -1.0f ? kClassLambertian : w <= 1.0f ? kClassMetal : kClassDielectric;
}

}  // namespace rtk
