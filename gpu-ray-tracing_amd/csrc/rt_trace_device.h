// rt_trace_device.h — the tracer's device library: the sphere scans, cone and grid culling,
// the camera, ray_color, sample and trace_pixel, with the constants they need.
//
// Shared by the units whose kernels trace rays or replay the tracer's arithmetic:
// rt_kernels.hip (the render kernels), rt_aov.hip (the G-buffer), rt_sampler.hip (the adaptive
// sampler and its fused rounds), rt_selftest.hip (the fast-math self-tests), rt_matte.hip and
// rt_query.hip (the ray queries: the scans' t_seed / kOcc / route parameters are theirs).  Everything
// here is __forceinline__ device code, a template or a constant, so a unit pays only for what
// its kernels call; static LDS (the bounce kernels' s_bounce) is not here, where it would be
// charged to every kernel of every unit.
//
// Diagnostic hooks: BCOUNT is called from this code, WAVE_TRACE, SST_V and SST_S from the
// render kernels.  A unit that wants them live (rt_kernels.hip in an RT_WAVE_TRACE /
// RT_BOUNCE_COUNTS / RT_SSTAMPS build) defines them before including this header; here they
// default to no-ops, so the other units compile in such a build and its counters see the
// render unit's kernels only.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_kernels.h"

#include <cstddef>
#include <cstring>

// The device code is written for gfx950 only (see rt_kernels.hip: the sc1 hand-offs).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "rt_trace_device.h targets gfx950 only"
#endif

#ifndef WAVE_TRACE
#define WAVE_TRACE(e) ((void)0)
#endif
#ifndef BCOUNT
#define BCOUNT(k) ((void)0)
#endif
#ifndef SST_V
#define SST_V(k, dep) ((void)0)
#endif
#ifndef SST_S
#define SST_S(k, dep) ((void)0)
#endif

namespace rtk {

using namespace rtd;

// Wave ballot of a per-lane condition.  HIP's __ballot(int) takes the predicate as an int,
// and the bool -> int -> bool round trip costs a v_cndmask + v_cmp per ballot on gfx950;
// the builtin takes the condition's lane mask as it is.
__device__ __forceinline__ unsigned long long rt_ballot(bool x) {
    return __builtin_amdgcn_ballot_w64(x);
}
// The one-frame kernel's (and normalize_w's) wave-uniform decisions come from lane masks
// (mask_*) instead of ballots: lane masks straight from one compare (llvm.amdgcn.icmp /
// fcmp: the v_cmp's SGPR result), combined with & and | as 64-bit scalars.  A ballot of a
// boolean that crosses blocks or combines earlier booleans compiles to a v_cndmask 0/1 +
// v_cmp_ne round trip (two 4-cycle VALU operations) at every use; these do not (round 3:
// K3 19.5-19.8 -> 18.9-19.1 µs, K2 13.6-13.8 -> 13.4 µs per update,
// profiles/r03/r03t_ab_single_masks_all.log).
__device__ __forceinline__ uint64_t mask_ult(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_uicmp(a, b, 36);          // ICMP_ULT
}
__device__ __forceinline__ uint64_t mask_uge(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_uicmp(a, b, 35);          // ICMP_UGE
}
__device__ __forceinline__ uint64_t mask_ne(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_uicmp(a, b, 33);          // ICMP_NE
}
__device__ __forceinline__ uint64_t mask_sge(int a, int b) {
    return __builtin_amdgcn_sicmp(a, b, 39);          // ICMP_SGE
}
__device__ __forceinline__ uint64_t mask_sgt(int a, int b) {
    return __builtin_amdgcn_sicmp(a, b, 38);          // ICMP_SGT
}
__device__ __forceinline__ uint64_t mask_not_lt(float a, float b) {
    return __builtin_amdgcn_fcmpf(a, b, 11);          // FCMP_UGE: !(a < b)
}

// Constant address space (read-only for the whole launch; eligible for scalar loads).
// (The host pass of hipcc also parses device code; there the qualifier is dropped.)
#if defined(__HIP_DEVICE_COMPILE__)
#define kconst __attribute__((address_space(4)))
#else
#define kconst
#endif

// min(|x|, |y|, |z|) (v_min3_f32 with abs modifiers; NaN channels ignored, as IEEE minNum)
__device__ __forceinline__ float min_abs3(v3 v) {
    return fminf(fminf(fabsf(v.x), fabsf(v.y)), fabsf(v.z));
}

struct Hit {
    int idx;     // winning sphere, -1 = miss
    float t;     // its root
};

// sphere_list_hit (wgsl:164-180) + sphere_hit (wgsl:182-201) without the hit record:
// only the closest root and its index are tracked; the record (p, normal, face,
// material) is rebuilt once for the winner, bit-identical to the WGSL's last assignment.
//
// The scan walks the list in chunks of 4 spheres.  The 16-byte scan records of the next
// chunk are fetched with scalar loads while the current chunk is computed (the index is
// wave-uniform, so the records live in SGPRs and feed the VALU directly).  Per sphere the
// common (miss) path is 12 VALU ops for the discriminant; the chunk's four "!(D < 0)"
// tests collapse into one integer max + compare on the float bit patterns (exact: D is
// never -0, see below), so the root-finding path is entered once per chunk at most.

// Discriminant of wgsl:183-187 for one sphere record g = (center, r*r).
__device__ __forceinline__ float discriminant(const float4 g, v3 o, v3 d, float a, float& h) {
    const float ocx = g.x - o.x;                                        // wgsl:183
    const float ocy = g.y - o.y;
    const float ocz = g.z - o.z;
    h = fmaf(ocz, d.z, fmaf(ocy, d.y, ocx * d.x));                      // wgsl:185
    const float c = fmaf(ocz, ocz, fmaf(ocy, ocy, ocx * ocx)) - g.w;    // wgsl:186
    return fmaf(h, h, -(a * c));                                        // wgsl:187
}

// Root selection of wgsl:189-201 for sphere i, given its discriminant.  (Callers only
// pass indices < count.)  The IEEE sqrt and divisions are kept as the compiler emits them:
// exact unscaled fast paths with per-lane domain checks measured slower here (the checks
// and their branches cost more SALU/VALU issue than the shorter sequences save).
__device__ __forceinline__ void consider(float disc, float h, float a, uint32_t i, float& tmax,
                                         int& idx) {
    if (!(disc < 0.0f)) {                                               // wgsl:189
        const float q = sqrtf(disc);
        float root = (h - q) / a;
        if (root <= 0x1.0624dep-10f || tmax <= root) {                  // wgsl:196
            root = (h + q) / a;
            if (root <= 0x1.0624dep-10f || tmax <= root) return;        // wgsl:198
        }
        tmax = root;
        idx = (int)i;
    }
}

// consider() for camera rays whose domain the host has proven (camera_rays_bounded in
// rt_abi.cpp): a = |d|^2 in [2^-11, 2^20] and |h|, sqrt(D) <= 2^53 for every sphere.  Then
// sqrt_core(D + 2^-126) and div_core (ya = the shared reciprocal of a) give the IEEE bits
// wherever the bits matter: for D >= 2^-96 adding 2^-126 (< half an ulp of D) changes
// nothing; for D in [0, 2^-96) both sqrt(D) and sqrt_core(D + 2^-126) are below 2^-47, so
// h -+ q rounds to h when |h| >= 2^-22, and below that both roots are under 0.001 (rejected)
// with either q; |h -+ q| < 2^-100 gives a root under 2^-89 (rejected) with either quotient;
// every other quotient is inside div_core's exact domain.  A first root above 0.001 and at
// or beyond tmax also rejects the second: h + q >= h - q and a > 0 make that root larger
// still.  The device self-test replays both functions on random grazing and ordinary
// cases (rt_selftest_fastmath, out[4]).
__device__ __forceinline__ void consider_fast(float disc, float h, float a, float ya,
                                              uint32_t i, float& tmax, int& idx) {
    if (!(disc < 0.0f)) {                                               // wgsl:189
        const float q = sqrt_core(disc + 0x1p-126f);
        float root = div_core(h - q, a, ya);
        if (root <= 0x1.0624dep-10f) {                                  // wgsl:196
            root = div_core(h + q, a, ya);
            if (root <= 0x1.0624dep-10f || tmax <= root) return;        // wgsl:198
        } else if (tmax <= root) {
            return;
        }
        tmax = root;
        idx = (int)i;
    }
}

// "!(D < 0)" for any of K discriminants, on the bit patterns: a float is < 0 exactly
// when its int32 view is <= 0xFF800000 (-inf) and it is not -0.  D = fma(h, h, -(a*c))
// with h*h >= +0 and a >= +0 cannot round to -0, so the test is one max-tree and one
// compare per chunk (max_bits below).

// Exhaustive scan: the reference's linear walk over every sphere (wgsl:169-177).

// max over the int32 views of K discriminants
template <int K>
__device__ __forceinline__ int max_bits(const float (&dd)[K]) {
    int m = __float_as_int(dd[0]);
#pragma unroll
    for (int k = 1; k < K; ++k) m = max(m, __float_as_int(dd[k]));
    return m;
}

// Chunk sizes: a full-list walk is 4 spheres per s_load_dwordx16 (267 us at K3 against
// 330 us one sphere at a time).  The list-only kernel (max_depth <= 1) walks the short
// per-tile candidate lists (2.7 spheres on average at K3) 2 at a time, testing fewer
// padding records (-2 % at K3; mixing both sizes in one kernel measured slower).
#ifndef RT_SCAN_CHUNK
#define RT_SCAN_CHUNK 4
#endif
#ifndef RT_LIST_CHUNK
#define RT_LIST_CHUNK 2
#endif
// the bounce instance's camera rays over their tile's list (K5: 2.1 entries per tile)
#ifndef RT_BOUNCE_LIST_CHUNK
#define RT_BOUNCE_LIST_CHUNK 2
#endif
template <int kScan>
constexpr int scan_chunk() { return is_list_kernel(kScan) ? RT_LIST_CHUNK : RT_SCAN_CHUNK; }
// Per-frame stores of fused launches (TraceParams::store_each) in rt_trace_kernel exist in
// the camera-ray-only instances alone (the culled instance would spill registers for them
// and runs one frame per launch); the bounce instance (rt_bounce_kernel) has its own
// two-last-frames stores and fuses frames too (rt_abi.cpp frames_per_launch_for).
template <int kScan>
constexpr bool kStoreEach = is_list_kernel(kScan);
// Exact fast division / sqrt cores (rt_device.h) in the camera-ray-only instances, which
// rt_abi.cpp selects only for cameras and scenes inside the proven domain
// (camera_rays_bounded): bit 1 the roots of the scan, 2 the normal, 4 the sky, 8 the
// metal / dielectric normalisations (the last three behind a wave-wide check of their
// operands), 16 the defocus disk's reciprocal table (disk_unit).  K3 per frame (fused): 21.7 us without, 20.9 / 20.1 / 20.1 us with bits
// 1 / 1-2 / 1-4; the accumulator's three divisions by f32(n + 1) the same way (checked
// numerators in [2^-88, 2^88)) measured +0.75 us and are left to the compiler.
// The accumulator's division by f32(n + 1) (wgsl:356) where every pixel of the wave holds
// the hinted count n (the one-frame kernel, the frame groups of trace_pair): a Markstein
// division by k = f32(n + 1) with y = RN32(1 / k) from the host (acc_rn: a multiply and two
// fmas per channel; round 5, against round 2's RN32(num * RN64(1 / k)), acc_f64: two
// conversions and an f64 multiply per channel, each a 4-cycle VALU form).  Exactness: for
// an integer k < 2^22 (kAccRnMax below), div_rn (rt_device.h) returns the IEEE quotient
// whenever num and the quotient are normal; numerators in (0, 2^-102) could give subnormal quotients and take the
// IEEE division (acc_ok: one unsigned compare per channel on the bit patterns; zero passes).
// Zero, inf and NaN numerators need no exclusion in this use: num = col - c with the sample
// colour col finite (|col| <= 1: a product of albedos in [0, 1] and the sky's [0.5, 1]) or
// NaN (a degenerate refraction); -0 / k comes out +0, but num = -0 needs c = +0 and c + (+-0)
// is +0 either way; num = +-inf needs c = -+inf, and c + num / k and c + div_rn(...) are NaN
// both (inf - inf); NaN propagates through both.  rt_selftest_fastmath replays it on random
// accumulators and colours.
constexpr uint32_t kBits2m102 = 0x0C800000u;   // 2^-102
// The Markstein step by k = f32(n + 1) is the IEEE quotient for integer k < 2^22 even where
// q = RN(num y) is 1.5 ulp off (Markstein's hypothesis needs one): num - mid k is a nonzero
// multiple of ulp(num / k) / 2 for every rounding midpoint mid, so |num / k - mid| >=
// ulp / (2 k) > 2^-23 ulp, more than the corrected quotient's error |q - num / k| |k y - 1|
// <= 1.5 ulp 2^-24 (round-5 ADVICE).  Counts of 2^22 or more take the IEEE division.
constexpr uint32_t kAccRnMax = 1u << 22;
// |x| >= 2^-102 or x == +-0 (NaN, inf pass) as one unsigned compare per channel on
// 2 (abs_bits(x) - 1) mod 2^32 = (bits << 1) - 2: the sign shifted out, one v_lshl_add per
// channel instead of an and and an add (x = +-0 wraps to 0xFFFFFFFE, above the bound, as
// abs_bits(x) - 1 wraps to 0xFFFFFFFF; otherwise the doubling is exact, abs_bits < 2^31)
constexpr uint32_t kAccOkDbl = 2u * (kBits2m102 - 1u);
__device__ __forceinline__ uint32_t dbl_m2(float x) { return (__float_as_uint(x) << 1) - 2u; }
// (acc_ok(num) == acc_min_bits(num) >= kAccOkDbl)
__device__ __forceinline__ uint32_t acc_min_bits(v3 num) {
    return min(min(dbl_m2(num.x), dbl_m2(num.y)), dbl_m2(num.z));
}
__device__ __forceinline__ bool acc_ok(v3 num) { return acc_min_bits(num) >= kAccOkDbl; }
// c + num / k with y = RN32(1 / k)
__device__ __forceinline__ v3 acc_rn(v3 c, v3 num, float k, float y) {
    return mk(c.x + div_rn(num.x, k, y), c.y + div_rn(num.y, k, y), c.z + div_rn(num.z, k, y));
}
template <int kScan>
constexpr bool fast_core(int bit) { return is_list_kernel(kScan); }
// The defocus disk's normalisation in the camera-ray-only trace instances (disk_unit)
constexpr int kTraceDisk = 3;

// Scan records are read through the constant address space: they do not change during a
// launch, and only then may the compiler use scalar loads (s_load_dwordx8/16 into SGPRs)
// in kernels that store images inside the frame loop.  (The single-frame list instance
// keeps vector loads: its SGPRs are short, scalar records measured +0.6 us per update.)
template <bool kScalar>
__device__ __forceinline__ float4 load_rec(const float4* __restrict__ geom, uint32_t i) {
    if (kScalar) return ((const kconst float4*)geom)[i];
    return geom[i];
}

// A tile's candidate count through the constant address space: a scalar load (the lists do
// not change during a launch), not a vector load + readfirstlane.
__device__ __forceinline__ uint32_t load_cnt(const float4* cand, uint32_t tile) {
    return ((const kconst uint32_t*)cand)[(size_t)tile * (4u * kCandStride)];
}

// kFast: camera rays in the host-proven domain (consider_fast).  kScalar: read the records
// through the constant address space (below).
// The ray queries' two additions (rt_query.hip), compiled out of every other caller by their
// defaults, here and in scan_grid_t / scan_grid / scan_culled below:
//   t_seed  the running tmax starts at the ray's own bound instead of 3.4e35.  Every root
//           selection takes the running tmax as it finds it — an earlier, nearer hit leaves the
//           same kind of value there — so their proofs carry over; with idx = -1 beside it,
//           consider_any's "root < tmax || si < idx" refuses a root equal to the seed as
//           consider's "tmax <= root" does.
//   kOcc    occlusion queries: any acceptance answers the query (a sphere that passes its own
//           test against the seed is accepted by whichever walk meets it first), so a wave
//           leaves the scan as soon as no live lane is still without one — in the wave-uniform
//           walks one ballot per chunk that reached a root test (exhaustive) or per 64 records
//           (cone), in the per-lane grid walk the lane's own exit.  live: the lanes whose
//           answer is wanted.
constexpr float kTmaxShader = 0x1.05ed2ep+118f;   // 3.4e35 (wgsl:266)
template <int K, bool kFast = false, bool kScalar = true, bool kOcc = false>
__device__ __forceinline__ Hit scan_exhaustive(const float4* __restrict__ geom, uint32_t count,
                                               v3 o, v3 d, float t_seed = kTmaxShader,
                                               bool live = true) {
    float tmax = t_seed;                       // 3.4e35 (wgsl:266) unless a query seeds it
    int idx = -1;
    if (count == 0) return Hit{idx, tmax};
    const float a = dot(d, d);                 // wgsl:184 (ray-invariant)
    const float ya = kFast ? rcp_refined(a) : 0.0f;
    // The record list is zero-padded to whole chunks plus one chunk more (rt_abi.cpp), so
    // every chunk (and the one-ahead prefetch) is a full scalar load; padding records are
    // never accepted (consider() is only called for indices < count).
    float4 cur[K];
#pragma unroll
    for (int k = 0; k < K; ++k) cur[k] = load_rec<kScalar>(geom, k);
    for (uint32_t i = 0; i < count; i += K) {
        float4 nxt[K];
#pragma unroll
        for (int k = 0; k < K; ++k) nxt[k] = load_rec<kScalar>(geom, i + K + k);
        float hh[K], dd[K];
#pragma unroll
        for (int k = 0; k < K; ++k) dd[k] = discriminant(cur[k], o, d, a, hh[k]);
        if (__builtin_expect(max_bits<K>(dd) > (int)0xFF800000, 0)) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (i + k < count) {
                    if (kFast)
                        consider_fast(dd[k], hh[k], a, ya, i + k, tmax, idx);
                    else
                        consider(dd[k], hh[k], a, i + k, tmax, idx);
                }
            if (kOcc && rt_ballot(live && idx < 0) == 0ull) break;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) cur[k] = nxt[k];
    }
    return Hit{idx, tmax};
}

// ---- Exact wave-level culling --------------------------------------------------------
//
// The 64 rays of a wave (one 8x8 tile, plus lens offsets) are nearly coherent.  Bound all
// of the wave's live rays by one double cone: apex = centroid of the origins, every
// origin within r_O of it, every unit direction within angle theta of the axis A (either
// sign).  For sphere (C, R) with v = C - apex, t = v.A, p = |v - tA|, every ray line is at
// distance >= p cos(theta) - |t| sin(theta) - r_O from C.  In exact arithmetic
// D = |d|^2 (R^2 - dist^2), and the f32 evaluation of wgsl:183-187 errs by less than
// ~32 eps |d|^2 (|oc|^2 + R^2) (eps = 2^-24), so the computed D is certainly negative when
// dist > R + m with m = 2.5e-3 (|oc| + |R|) >= 2.5x sqrt(16 eps)|oc| + sqrt(6 eps)|R|, and
// |oc| <= |t| + p + r_O + d_max (DESIGN.md §5 has the derivation).
// Such a sphere can never be the hit of any lane and is skipped; every other sphere goes
// through the exact per-lane test in list order, so the closest-hit result (including
// the first-index-wins tie rule) is bit-identical to the exhaustive scan.  One sphere
// per lane is tested against the cone (64 spheres per VALU instruction); survivors are
// picked from the ballot mask in increasing index order.  Bounce rays walk the sphere grid
// instead when the scene has one (scan_grid below); non-finite or degenerate rays, wide
// cones (theta >~ 60 deg) and short lists use the exhaustive scan.
constexpr uint32_t kCullMinSpheres = 32;

// Wave-wide reductions on the VALU: row_ror DPP inside each 16-lane row, then the four
// row results are read into SGPRs (v_readlane) and combined, so every lane receives the
// same (uniform) value.  Rounding order does not matter here: the cone only needs to be
// conservative, and the margins of cone_misses() dwarf these errors.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
constexpr int kRowRor8 = 0x128, kRowRor4 = 0x124, kRowRor2 = 0x122, kRowRor1 = 0x121;
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp<kRowRor8>(v);
    v += dpp<kRowRor4>(v);
    v += dpp<kRowRor2>(v);
    v += dpp<kRowRor1>(v);
    return (lane_f(v, 0) + lane_f(v, 16)) + (lane_f(v, 32) + lane_f(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp<kRowRor8>(v));
    v = fmaxf(v, dpp<kRowRor4>(v));
    v = fmaxf(v, dpp<kRowRor2>(v));
    v = fmaxf(v, dpp<kRowRor1>(v));
    return fmaxf(fmaxf(lane_f(v, 0), lane_f(v, 16)), fmaxf(lane_f(v, 32), lane_f(v, 48)));
}
__device__ __forceinline__ bool finite3(v3 v) {
    return __builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z);
}

struct Cone {
    v3 apex, axis;
    float cos_t, sin_t, r_o, d_max;
};

// Builds the cone of the live lanes' rays; false when culling cannot be used.  Must be
// called with the whole wave active (it reduces across lanes).  The apex is the centroid
// of the points q = o + d: for camera rays these are the sample points on the focus
// plane, where the beam of a tile is narrowest; r_o bounds |q - apex| and d_max bounds
// |d| (so |o - apex| <= r_o + d_max for the rounding margin).
__device__ __forceinline__ bool wave_cone(v3 o, v3 d, bool live, Cone& k) {
    const float dd = dot(d, d);
    const v3 q = add(o, d);
    const bool bad = live && !(finite3(o) && finite3(q) && dd > 0.0f && __builtin_isfinite(dd));
    const unsigned long long lm = rt_ballot(live);
    if (lm == 0ull || rt_ballot(bad)) return false;
    // Axis and apex come from the first live lane (v_readlane: no cross-lane reduction);
    // the half-angle, the apex radius and max |d| are then exact max-reductions.
    const int L = (int)__builtin_ctzll(lm);
    const float inv = rsqrtf(dd);
    const v3 u = mk(d.x * inv, d.y * inv, d.z * inv);
    k.axis = mk(lane_f(u.x, L), lane_f(u.y, L), lane_f(u.z, L));
    k.apex = mk(lane_f(q.x, L), lane_f(q.y, L), lane_f(q.z, L));
    const v3 du = sub(u, k.axis), dq = sub(q, k.apex);
    const float s = wave_max(live ? __builtin_amdgcn_sqrtf(dot(du, du)) : 0.0f);  // chord
    const float r = wave_max(live ? __builtin_amdgcn_sqrtf(dot(dq, dq)) : 0.0f);
    const float dm = wave_max(live ? __builtin_amdgcn_sqrtf(dd) : 0.0f);
    const float su = s * 1.001f + 1e-6f;
    if (!(su < 1.0f)) return false;                                  // theta >~ 60 degrees
    k.cos_t = 1.0f - 0.5f * su * su;
    k.sin_t = su * __builtin_amdgcn_sqrtf(1.0f - 0.25f * su * su) * 1.001f;
    k.r_o = r * 1.001f + 1e-6f * (fabsf(k.apex.x) + fabsf(k.apex.y) + fabsf(k.apex.z));
    k.d_max = dm * 1.001f;
    return true;
}

// True when sphere record g = (center, r*r) provably misses every ray of the cone.
// lhs bounds the distance of every ray line from C from below (less 1e-5 of the magnitudes
// for its own f32 evaluation); the computed discriminant is certainly negative when
// dist^2 > R^2 + E, E = eps (16 |oc|^2 + 6 R^2), and m^2 >= 6.25e-6 (|oc|^2 +
// R^2) >= E, so the test is dist > sqrt(R^2 + m^2) — round 4 used R + m, which is larger by
// up to m, about a fifth of a small sphere's radius at the K3 camera's distances (K3's
// candidate lists 2.68 -> 2.22 entries per tile, profiles/r05/r05t/).
__device__ __forceinline__ bool cone_misses(const Cone& k, float4 g) {
    const v3 v = mk(g.x - k.apex.x, g.y - k.apex.y, g.z - k.apex.z);
    const float t = dot(v, k.axis);
    const float p = __builtin_amdgcn_sqrtf(fmaxf(fmaf(-t, t, dot(v, v)), 0.0f));
    const float at = fabsf(t), R = __builtin_amdgcn_sqrtf(g.w) * 1.0001f;
    const float mag = at + p + k.r_o;
    const float lhs = fmaf(p, k.cos_t, -at * k.sin_t) - k.r_o - 1e-5f * mag;
    const float m = 2.5e-3f * (mag + k.d_max + R);
    return lhs > R && lhs * lhs > fmaf(R, R, m * m) * 1.0001f;   // NaN anywhere -> keep
}

// Scan records staged in LDS by the workgroup (culled scan, lists up to kLdsMaxRecords).
extern __shared__ float4 lds_recs[];

// kLds: read the cull records from the workgroup's LDS copy (else from the global array);
// both hold count records zero-padded to a multiple of 64.
// ---- Exact grid walk for incoherent bounce rays ---------------------------------------
//
// The closest hit of the linear scan (consider() in index order: a later sphere wins only
// if strictly nearer) is the minimum over spheres of c_i = root1 if root1 > 0.001, else
// root2 if root2 > 0.001, with ties going to the lower index: a sphere whose first root is
// valid but not below the running tmax has a second root at least as large (h + q >= h - q,
// a > 0), and a tie keeps the earlier index.  So the spheres may be tested in any order with
// consider_any's rule.  A sphere can be accepted only at a root t > 0 whose point lies
// within sqrt(R^2 + m^2) of its centre (m the f32 margin of the discriminant, as in the cone
// test), so the grid walk visits every cell the ray passes through for t >= 0 inside the
// gridded spheres' slab, and each sphere is registered in every cell within
// sqrt(R^2 + grid_m^2) + grid_e of its centre (rt_abi.cpp): no sphere that could be accepted
// is skipped.
// (items: the grid's item index array — the sphere index items[i] is loaded only for a root
// that is accepted or ties; null: i is the sphere index)
__device__ __forceinline__ void consider_any(float disc, float h, float a, uint32_t i,
                                             float& tmax, int& idx,
                                             const uint32_t* items = nullptr) {
    if (!(disc < 0.0f)) {                                               // wgsl:189
        const float q = sqrtf(disc);
        float root = (h - q) / a;
        if (root <= 0x1.0624dep-10f) {                                  // wgsl:196
            root = (h + q) / a;
            if (root <= 0x1.0624dep-10f) return;                        // wgsl:198
        }
        if (root <= tmax) {
            const int si = (int)(items ? items[i] : i);
            if (root < tmax || si < idx) {
                tmax = root;
                idx = si;
            }
        }
    }
}
// consider_any with consider_fast's arithmetic (sqrt_core of D + 2^-126, div_core with the
// shared reciprocal ya of a): the IEEE roots wherever they decide anything, on consider_fast's
// domain (a in [2^-11, 2^20], |h| and sqrt(D) <= 2^53), which roots_fast_wave checks per wave.
__device__ __forceinline__ void consider_any_fast(float disc, float h, float a, float ya,
                                                  uint32_t i, float& tmax, int& idx,
                                                  const uint32_t* items = nullptr) {
    if (!(disc < 0.0f)) {                                               // wgsl:189
        const float q = sqrt_core(disc + 0x1p-126f);
        float root = div_core(h - q, a, ya);
        if (root <= 0x1.0624dep-10f) {                                  // wgsl:196
            root = div_core(h + q, a, ya);
            if (root <= 0x1.0624dep-10f) return;                        // wgsl:198
        }
        if (root <= tmax) {
            const int si = (int)(items ? items[i] : i);
            if (root < tmax || si < idx) {
                tmax = root;
                idx = si;
            }
        }
    }
}
// Whether every live ray of the wave is in consider_fast's domain against every sphere of a
// scene with |C| + |R| <= 2^40 (scene_ok: TraceParams::roots_fast): a = |d|^2 in
// [2^-11, 2^20] and |o|'s components below 2^39.  Then |oc| <= |C| + |o| < 2^41,
// |h| <= |d| |oc| < 2^51 and, with c = |oc|^2 - R^2 >= -R^2, sqrt(D) <= sqrt(h^2 + a R^2)
// < 2^52.  NaN or infinite a / o fail the test.  (Bounce rays and the bounce instance's camera
// rays: the camera-ray-only instances have the host's camera_rays_bounded instead.)
__device__ __forceinline__ bool roots_fast_wave(uint32_t scene_ok, v3 o, float a, bool live) {
    const uint32_t om = max(max(abs_bits(o.x), abs_bits(o.y)), abs_bits(o.z));
    const bool ok = __float_as_uint(a) - 0x3A000000u <= 0x49800000u - 0x3A000000u &&  // a
                    om < 0x53000000u;                                               // 2^39
    return scene_ok != 0u && rt_ballot(live && !ok) == 0ull;
}
// The grid's launch parameters (TraceParams grid_*), as one value: built from the kernel
// argument, or (rt_bounce_kernel) re-read from the kernarg segment at every use so that they
// do not stay live in SGPRs across the frame loop.
struct GridP {
    const uint2* cells;
    const float4* geom;
    const uint32_t* items;
    const uint32_t* big;
    const float4* sgeom;     // TraceParams::geom (the big spheres' records)
    uint32_t nx, nz, nbig;
    float x0, z0, s, inv_s, ylo, yhi, cx, cy, cz, reach, m, e;
    uint32_t roots_fast;     // TraceParams::roots_fast
};
template <typename P>
__device__ __forceinline__ GridP grid_params(const P& p) {
    GridP g;
    g.roots_fast = p.roots_fast;
    g.cells = p.grid_cells;
    g.geom = p.grid_geom;
    g.items = p.grid_items;
    g.big = p.grid_big;
    g.sgeom = p.geom;
    g.nx = p.grid_nx;
    g.nz = p.grid_nz;
    g.nbig = p.grid_nbig;
    g.x0 = p.grid_x0;
    g.z0 = p.grid_z0;
    g.s = p.grid_s;
    g.inv_s = p.grid_inv_s;
    g.ylo = p.grid_ylo;
    g.yhi = p.grid_yhi;
    g.cx = p.grid_cx;
    g.cy = p.grid_cy;
    g.cz = p.grid_cz;
    g.reach = p.grid_reach;
    g.m = p.grid_m;
    g.e = p.grid_e;
    return g;
}
// kFast: the roots by consider_any_fast (the wave passed roots_fast_wave; same bits).
// The walk's own t values (slab and box entry / exit, cell-boundary crossings and their
// steps) are products with refined reciprocals of d's components (rcp_refined: one Newton
// step from v_rcp_f32) rather than IEEE quotients: they only steer the traversal, whose cells
// are padded by e (build_grid).  Each such product is within 1 ulp (<= 2 eps, eps = 2^-24) of
// its exact value instead of half an ulp, so a crossing after k steps is off by at most
// (4 + 6k) eps x the coordinate magnitudes (the start and the k additions of the step,
// each step's own error included), inside e's (k + 16) x 8 eps.  A zero component keeps its
// branch; a subnormal one gives an infinite or huge reciprocal, i.e. an axis the ray does not
// cross (it moves less than 2^-60 along it inside the box), or a NaN t that fminf / fmaxf /
// the compares skip the same way.
// walk: this lane walks the grid (false: a far ray that misses every small sphere, which only
// tests the big list; grid_usable).
template <bool kFast, bool kOcc = false>
__device__ __forceinline__ Hit scan_grid_t(const GridP& p, v3 o, v3 d, bool live, bool walk,
                                           float t_seed = kTmaxShader) {
    const float a = dot(d, d);
    const float ya = kFast ? rcp_refined(a) : 0.0f;
    float tmax = t_seed;                       // 3.4e35 (wgsl:266) unless a query seeds it
    int idx = -1;
    auto test = [&](float disc, float h, uint32_t i, const uint32_t* items) {
        if (kFast)
            consider_any_fast(disc, h, a, ya, i, tmax, idx, items);
        else
            consider_any(disc, h, a, i, tmax, idx, items);
    };
    // spheres outside the grid (the ground, large ones): every live lane tests them
    for (uint32_t b = 0; b < p.nbig; ++b) {
        const uint32_t i = p.big[b];
        const float4 g = p.sgeom[i];
        float h;
        const float disc = discriminant(g, o, d, a, h);
        if (live) test(disc, h, i, nullptr);
    }
    BCOUNT(26);
    if (!live || !walk || (kOcc && idx >= 0)) return Hit{idx, tmax};
    BCOUNT(kFast ? 0 : 14);
    // t range of the ray inside the slab and the grid box (t >= 0)
    const float rx = rcp_refined(d.x), ry = rcp_refined(d.y), rz = rcp_refined(d.z);
    float t0 = 0.0f, t1 = 0x1.05ed2ep+118f;
    auto clip = [&](float oc, float dc, float rc, float lo, float hi) {
        if (dc != 0.0f) {
            const float ta = (lo - oc) * rc, tb = (hi - oc) * rc;
            t0 = fmaxf(t0, fminf(ta, tb));
            t1 = fminf(t1, fmaxf(ta, tb));
        } else if (oc < lo || oc > hi) {
            t1 = -1.0f;
        }
    };
    const float xhi = p.x0 + p.s * (float)p.nx;
    const float zhi = p.z0 + p.s * (float)p.nz;
    clip(o.y, d.y, ry, p.ylo, p.yhi);
    clip(o.x, d.x, rx, p.x0, xhi);
    clip(o.z, d.z, rz, p.z0, zhi);
    if (!(t0 <= t1)) return Hit{idx, tmax};
    // 2-D DDA over the cells from P(t0) to P(t1)
    const int nx = (int)p.nx, nz = (int)p.nz;
    int ix = (int)floorf((fmaf(t0, d.x, o.x) - p.x0) * p.inv_s);
    int iz = (int)floorf((fmaf(t0, d.z, o.z) - p.z0) * p.inv_s);
    ix = min(max(ix, 0), nx - 1);
    iz = min(max(iz, 0), nz - 1);
    const int sx = d.x > 0.0f ? 1 : -1, sz = d.z > 0.0f ? 1 : -1;
    const float inf = 0x1.05ed2ep+118f;
    float tx = d.x != 0.0f ? (p.x0 + p.s * (float)(ix + (sx > 0)) - o.x) * rx : inf;
    float tz = d.z != 0.0f ? (p.z0 + p.s * (float)(iz + (sz > 0)) - o.z) * rz : inf;
    const float dtx = d.x != 0.0f ? p.s * fabsf(rx) : inf;
    const float dtz = d.z != 0.0f ? p.s * fabsf(rz) : inf;
    const float slack = 2.0f * p.e * rsqrtf(a) * 1.01f;
    for (int step = 0; step < nx + nz + 2; ++step) {
        BCOUNT(2);
        const uint2 range = p.cells[iz * nx + ix];
        for (uint32_t k = range.x; k < range.y; ++k) {
            BCOUNT(4);
            float h;
            const float disc = discriminant(p.geom[k], o, d, a, h);
            test(disc, h, k, p.items);
        }
        if (kOcc && idx >= 0) break;
        // A cell entered beyond t1, or beyond the closest hit so far, holds no better hit;
        // slack: the walk's position error (grid_e, as t) and 1e-4 of t.
        const float tn = fminf(tx, tz);
        if (tn > fminf(t1, tmax) * 1.0001f + slack) break;
        if (tx < tz) {
            ix += sx;
            tx += dtx;
            if (ix < 0 || ix >= nx) break;
        } else {
            iz += sz;
            tz += dtz;
            if (iz < 0 || iz >= nz) break;
        }
    }
    return Hit{idx, tmax};
}
template <bool kOcc = false>
__device__ __forceinline__ Hit scan_grid(const GridP& p, v3 o, v3 d, bool live, bool walk,
                                         float t_seed = kTmaxShader) {
    if (roots_fast_wave(p.roots_fast, o, dot(d, d), live))
        return scan_grid_t<true, kOcc>(p, o, d, live, walk, t_seed);
    return scan_grid_t<false, kOcc>(p, o, d, live, walk, t_seed);
}

// The wave may walk the grid: every live ray finite and within reach of the grid margin.
// A ray farther out (walk false) may still share the wave's walk when it certainly misses
// every small sphere: it tests the big list only.  The small spheres lie in the ball B(c,
// reach); sphere i's discriminant is certainly negative where the line passes farther than
// sqrt(R_i^2 + m_i^2) from C_i, m_i = 2.5e-3 (|o - C_i| + R_i) <= m_far = 2.5e-3 (|o - c| +
// reach) (the cone test's margin), so a line at least reach + m_far from c misses them all
// (|C_i - c| + R_i <= reach), and so does a ray whose origin lies past the whole ball (c's
// projection t < -(reach + m_far): both roots of every small sphere negative).  Evaluated with
// a 1.01 / 1.001 widening and 1e-5 |o - c| for the f32 rounding of t and of |o - c|^2 - t^2.
// (K5: 0.038 of every wave-frame fell back to the 500-sphere exhaustive scan for the
// far ground's bounce rays, profiles/r06/r06v/.)
__device__ __forceinline__ bool grid_usable(const GridP& p, v3 o, v3 d, bool live, bool& walk) {
    if (p.nx == 0u) return false;
    const v3 oc = mk(o.x - p.cx, o.y - p.cy, o.z - p.cz);
    const float vv = dot(oc, oc);
    const float dist = __builtin_amdgcn_sqrtf(vv);
    const float dd = dot(d, d);
    const bool fin = finite3(o) && finite3(d) && dd >= 0x1p-20f && dd <= 0x1p20f;
    walk = 2.5e-3f * 1.01f * (dist + p.reach) <= p.m;
    bool far_miss = false;
    if (fin && !walk) {
        const float t = -dot(oc, d) * __builtin_amdgcn_rsqf(dd);   // c along the unit ray
        const float thr = (p.reach + 2.5e-3f * 1.01f * (dist + p.reach)) * 1.001f + 1e-5f * dist;
        far_miss = fmaf(-t, t, vv) > fmaf(1e-5f, vv, thr * thr * 1.0001f) || t < -thr;
    }
    return rt_ballot(live && !(fin && (walk || far_miss))) == 0ull;
}

// route (the ray queries' counters; null: not wanted): receives the scan the wave took.
constexpr uint32_t kRouteGrid = 0, kRouteCone = 1, kRouteExhaustive = 2;
template <bool kLds, bool kOcc = false>
__device__ __forceinline__ Hit scan_culled(const GridP& gp, const float4* __restrict__ geom,
                                           uint32_t count, v3 o, v3 d, bool live, bool bounce,
                                           float t_seed = kTmaxShader, uint32_t* route = nullptr) {
    const float4* recs = kLds ? lds_recs : geom;
    // Bounce rays walk the grid whenever the wave may (measured faster than the cone
    // culling even for coherent specular waves); camera rays of tiles without a candidate
    // list keep the cone, whose rays share a narrow beam.
    bool walk;
    if (bounce && count >= kCullMinSpheres && grid_usable(gp, o, d, live, walk)) {
        if (route) *route = kRouteGrid;
        return scan_grid<kOcc>(gp, o, d, live, walk, t_seed);
    }
    (void)bounce;
    (void)gp;
    Cone k;
    if (count < kCullMinSpheres || !wave_cone(o, d, live, k)) {
        BCOUNT(bounce ? 18 : 20);
        if (route) *route = kRouteExhaustive;
        return scan_exhaustive<RT_SCAN_CHUNK, false, true, kOcc>(geom, count, o, d, t_seed, live);
    }
    BCOUNT(bounce ? 22 : 24);
    if (route) *route = kRouteCone;
    const uint32_t lane = threadIdx.x & 63u;
    const float a = dot(d, d);
    float tmax = t_seed;
    int idx = -1;
    for (uint32_t base = 0; base < count; base += 64u) {
        const float4 g = recs[base + lane];
        const bool keep = (base + lane < count) && !cone_misses(k, g);
        unsigned long long mask = rt_ballot(keep);
        while (mask) {                                    // survivors, in index order
            const int j = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const float4 gs = recs[base + (uint32_t)j];   // broadcast read
            float h;
            const float disc = discriminant(gs, o, d, a, h);
            consider(disc, h, a, base + (uint32_t)j, tmax, idx);
        }
        if (kOcc && rt_ballot(live && idx < 0) == 0ull) break;
    }
    return Hit{idx, tmax};
}

// ---- Per-tile candidate lists for camera rays -----------------------------------------
//
// Every camera ray of a tile passes through the tile's footprint on the focus plane
// (pc = vul + pdu*sx + pdv*sy with sx in [x0, x0+8], sy in [y0, y0+8] for any jitter, since
// rounding is monotonic): q with |q - Pc| <= r_q, Pc the footprint's centre, and starts on the
// lens disk: o = center + ux ddu + uy ddv with |o - center| <= r_l, whatever the frame seed.
//
// The lens radius.  |ux ddu + uy ddv| <= sigma |(ux, uy)|, sigma the largest singular value of
// the 3 x 2 matrix [ddu ddv]: the square root of the largest eigenvalue of its Gram matrix
// [[a c] [c b]] (a = |ddu|^2, b = |ddv|^2, c = ddu.ddv), (a + b) / 2 + sqrt(((a - b) / 2)^2 +
// c^2).  For orthogonal vectors of one length that is the length itself, where sqrt(a + b),
// the bound used before, is sqrt(2) of it.  disk_unit's computed (ux, uy) has a length within
// a few ulp of 1 and the f32 evaluation of the eigenvalue errs by a few ulp of a + b <= twice
// the eigenvalue: lens_radius() returns 1.0001 sigma, and the callers widen it further.
//
// The beam.  The ray's line is x(l) = (1 - l) o + l q over all real l, and the point of the
// axis line with the same parameter is a(l) = (1 - l) center + l Pc, so
//     |x(l) - a(l)| <= |1 - l| r_l + |l| r_q  =: rho.
// Nothing else is used: neither that the lens and the focus plane are parallel nor that ddu
// and ddv lie in a plane across the axis.  With L = |Pc - center| and t = (l - 1) L, the
// position of a(l) along the axis from Pc (positive beyond the focus plane), rho is the
// largest of three straight lines in t:
//     far    r_q + t (r_l + r_q) / L      (|1 - l| = l - 1, |l| = l:  beyond the focus plane)
//     near   r_q - t (r_l - r_q) / L      (1 - l, l:   between the lens and the focus plane)
//     back  -r_q - t (r_l + r_q) / L      (1 - l, -l:  behind the lens)
// (the fourth combination is the negative of `near` and never the largest of a set whose
// maximum is >= 0).  So every ray lies in the union over t of the balls of radius rho(t) about
// the axis point at t.  For a sphere centre C at t along and p across the axis, a line
// c + s t' of that set with |s| <= sin(theta) and any axis position t' = t - u:
//     sqrt(p^2 + u^2) - (c + s t') >= p cos + |u| sin - c - s t + s u >= p cos - (c + s t),
// by Cauchy-Schwarz and |s u| <= |u| sin.  Hence every ray line stays at least
//     p cos(theta) - rho(t)
// from C, theta the angle of the steepest line: sin(theta) = (r_l + r_q) / L.  The single
// cone used before (kept as `parent`, and the one rt_matte.hip restates) is the far line's
// slope on both sides of Pc with L - r_l - r_q for L; between the lens and the focus plane
// the beam in truth narrows or widens by (r_l - r_q) / L only, and there the largest spheres
// on screen lie.  The same sin(theta) bounds the angle between any ray's direction q - o and
// the axis (|q - o - (Pc - center)| <= r_l + r_q against |Pc - center| = L).
//
// f32: r_q and r_l are widened by 0.1 % and by 1e-5 of the coordinates' magnitudes (the
// evaluation of pc and of o = pc - d + d), the slopes by 1 % upwards — the near slope, when
// negative, towards zero — and cos(theta) by 0.1 % downwards; the beam is built only where
// L > 4 (r_q + r_l) and everything is finite, else the tile gets no list.
//
// Spheres that beam_misses() rejects can never be hit by a camera ray of the tile; the others
// are listed (records + indices, in index order) once per camera/scene by
// rt_candidates_kernel, and each frame's camera rays test only that list.
__device__ __forceinline__ float len3(v3 v) { return __builtin_amdgcn_sqrtf(dot(v, v)); }

// The radius of the lens disk about the camera centre (0 without a lens), not yet widened for
// the f32 evaluation of the origins.  parent: the bound used before the beam.
__device__ __forceinline__ float lens_radius(const TraceParams& p, bool parent) {
    if (!(p.defocus_angle > 0.0f)) return 0.0f;
    const v3 du = mk(p.ddu[0], p.ddu[1], p.ddu[2]), dv = mk(p.ddv[0], p.ddv[1], p.ddv[2]);
    const float a = dot(du, du), b = dot(dv, dv), c = dot(du, dv);
    if (parent) return __builtin_amdgcn_sqrtf(a + b);
    const float h = 0.5f * (a + b), g = 0.5f * (a - b);
    return __builtin_amdgcn_sqrtf(h + __builtin_amdgcn_sqrtf(fmaf(g, g, c * c))) * 1.0001f;
}

// The bundle of a tile's camera rays, for the list build: rho(t) = r_o + the largest of
// sin_t t, -sin_n t and -sin_t t - 2 r_o (far, near, back above).
struct Beam {
    v3 apex, axis;          // Pc and the unit vector from the camera centre to it
    float cos_t, sin_t;     // the far slope, also the directions' half-angle
    float sin_n;            // the near slope: growth towards the lens (negative: a narrowing)
    float r_o, d_max;       // r_q; a bound on |d| of every ray
};

// The beam of the camera rays through the focus-plane rectangle of pixel columns [x0, x1)
// and rows [y0, y1) (one tile: 8 x 8).  parent: the single cone (sin_n = sin_t, the slope
// taken against L - r_l - r_q, the lens radius sqrt(|ddu|^2 + |ddv|^2)), whose tests
// evaluate to the bits they had.
__device__ __forceinline__ bool footprint_beam(const TraceParams& p, float x0, float x1,
                                               float y0, float y1, bool parent, Beam& k) {
    const v3 vul = mk(p.vul[0], p.vul[1], p.vul[2]), pdu = mk(p.pdu[0], p.pdu[1], p.pdu[2]),
             pdv = mk(p.pdv[0], p.pdv[1], p.pdv[2]);
    const v3 ctr = mk(p.center[0], p.center[1], p.center[2]);
    const v3 pc = fmas(0.5f * (y0 + y1), pdv, fmas(0.5f * (x0 + x1), pdu, vul));
    float rq = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const v3 q = fmas(c & 2 ? y1 : y0, pdv, fmas(c & 1 ? x1 : x0, pdu, vul));
        rq = fmaxf(rq, len3(sub(q, pc)));
    }
    float rl = lens_radius(p, parent);
    const float mag = fabsf(pc.x) + fabsf(pc.y) + fabsf(pc.z) + fabsf(ctr.x) + fabsf(ctr.y) +
                      fabsf(ctr.z);
    rq = rq * 1.001f + 1e-5f * mag;                 // f32 evaluation of pc and o = pc - d + d
    rl = rl * 1.001f + 1e-5f * mag;
    const v3 w = sub(pc, ctr);
    const float L = len3(w), delta = rq + rl;
    if (!(L > 4.0f * delta) || !__builtin_isfinite(L + mag)) return false;
    k.axis = mk(w.x / L, w.y / L, w.z / L);
    k.apex = pc;
    if (parent) {
        k.sin_t = delta / (L - delta) * 1.01f;
        k.sin_n = k.sin_t;
    } else {
        k.sin_t = delta / L * 1.01f;
        const float sn = (rl - rq) / L;
        k.sin_n = sn * (sn > 0.0f ? 1.01f : 0.99f);
    }
    k.cos_t = __builtin_amdgcn_sqrtf(1.0f - k.sin_t * k.sin_t) * 0.999f;
    k.r_o = rq;
    k.d_max = (L + delta) * 1.001f;
    return true;
}

// rho(t) - r_o: how far the beam has spread at t along the axis from the apex.  (A NaN or
// infinite t leaves a NaN or +inf here, whatever the slopes' signs: the tests then keep.)
__device__ __forceinline__ float beam_spread(const Beam& k, float t) {
    return fmaxf(fmaxf(k.sin_t * t, -k.sin_n * t), fmaf(-k.sin_t, t, -2.0f * k.r_o));
}

// cone_misses() for the list build: true when sphere record g = (center, r*r) provably misses
// every ray of the beam.  lhs is p cos - rho(t) above, less 1e-5 of the magnitudes for its own
// f32 evaluation; R, m and the comparison are cone_misses' (|oc| <= |t| + p + r_o + d_max holds
// for the beam as for the cone: C to the apex, the apex to q, q to o).
__device__ __forceinline__ bool beam_misses(const Beam& k, float4 g) {
    const v3 v = mk(g.x - k.apex.x, g.y - k.apex.y, g.z - k.apex.z);
    const float t = dot(v, k.axis);
    const float p = __builtin_amdgcn_sqrtf(fmaxf(fmaf(-t, t, dot(v, v)), 0.0f));
    const float at = fabsf(t), R = __builtin_amdgcn_sqrtf(g.w) * 1.0001f;
    const float mag = at + p + k.r_o;
    const float lhs = fmaf(p, k.cos_t, -beam_spread(k, t)) - k.r_o - 1e-5f * mag;
    const float m = 2.5e-3f * (mag + k.d_max + R);
    return lhs > R && lhs * lhs > fmaf(R, R, m * m) * 1.0001f;   // NaN anywhere -> keep
}

struct Cam {
    v3 center, vul, pdu, pdv, ddu, ddv;
    float defocus_angle;
    float k1s = -0x1.9943f2p-13f, k1c = 0x1.99eb9cp-16f;   // sincos_k's leading coefficients
};
template <typename P>
__device__ __forceinline__ Cam cam_params(const P& p) {
    Cam cam;
    cam.center = mk(p.center[0], p.center[1], p.center[2]);
    cam.vul = mk(p.vul[0], p.vul[1], p.vul[2]);
    cam.pdu = mk(p.pdu[0], p.pdu[1], p.pdu[2]);
    cam.pdv = mk(p.pdv[0], p.pdv[1], p.pdv[2]);
    cam.ddu = mk(p.ddu[0], p.ddu[1], p.ddu[2]);
    cam.ddv = mk(p.ddv[0], p.ddv[1], p.ddv[2]);
    cam.defocus_angle = p.defocus_angle;
    return cam;
}

// The defocus disk's normalize((cos, sin)) (wgsl:327-331).  Over all 2^32 values of
// hash(seed + 1), len2 = sa^2 + ca^2 takes only the eight f32 values of
// [1 - 6*2^-24, 1 + 2^-23], |sa| >= 2^-30 or sa == +0 and |ca| >= 2^-27 (checked
// exhaustively by rt_selftest_fastmath), so sqrtf(len2) = 1 - m 2^-24 with
// m = (0x3F800001 - bits(len2)) >> 1 in {3, 3, 2, 2, 1, 1, 0, 0}.
// kTable: 0 = sqrt_core / div_core (exact on this domain);
// 3 = all-f32: len = sqrtf(len2) = 1 - m 2^-24 (bits 0x3F800000 - m) and y = RN32(1 / len)
// = 1 + ((m + 1) >> 1) 2^-23 (m = 1: 1 + 2^-24 + 2^-48 rounds up; m = 3: 1 + 1.5 ulp + 9
// 2^-48 rounds to 2 ulp) from the bits of len2, then one Markstein step — q0 = RN(a y), the
// exact residual r = fma(-len, q0, a), q = RN(q0 + r y) — the correctly rounded a / len
// for a correctly rounded y (checked against the IEEE division for all 2^32 seeds by
// rt_selftest_fastmath).  Six f32 operations and four integer ones.  (Rounds 2-4 also had
// an f64 table of RN64(1 / len), per workgroup in LDS or in closed form: the all-f32 form
// replaced it in the one-frame kernel in round 3 and in the frame groups in round 5 — no
// table, no barrier at wave start; an 8-rank K3 chain share 2.69 -> 2.65 us per step,
// profiles/r05/r05h/.)
template <int kTable>
__device__ __forceinline__ void disk_unit(float sa, float ca, float& ux, float& uy) {
    const float len2 = fmaf(sa, sa, ca * ca);
    if (kTable == 3) {
        const uint32_t m = (0x3F800001u - __float_as_uint(len2)) >> 1;
        const float len = __uint_as_float(0x3F800000u - m);
        const float y = __uint_as_float(0x3F800000u + ((m + 1u) >> 1));
        const float qx = ca * y, qy = sa * y;
        ux = fmaf(fmaf(-len, qx, ca), y, qx);
        uy = fmaf(fmaf(-len, qy, sa), y, qy);
    } else {
        const float len = sqrt_core(len2);
        const float y = rcp_refined(len);
        ux = div_core(ca, len, y);
        uy = div_core(sa, len, y);
    }
}

// The lens sample's sincos runs without a NaN guard on its quadrant (the angle is finite):
// K3 14.26 against 14.42 µs per update over three interleaved rounds
// (profiles/r04/r04q_ab_front_fin.txt).
// get_ray (wgsl:305-325) with the pixel-invariant hash(hash(x*73) ^ hash(y*51)) part
// precomputed per pixel: seed = hash(hxy ^ su), su = sample_index*25 + B (wave-uniform
// when every pixel of the wave holds the same sample count).
template <int kTable>
__device__ __forceinline__ void get_ray(const Cam& cam, uint32_t x, uint32_t y, uint32_t hxy,
                                        uint32_t su, v3& o, v3& d,
                                        const v3* c0v = nullptr) {
    const uint32_t seed = hash(hxy ^ su);
    // rf(v) = f32(hash(v)) * 2^-32 is exact (a power-of-two scale of a value >= 1 or 0), so
    // the next rounding is the only one: rf - 0.5 is one fma, 2pi * rf one multiply by
    // 2pi * 2^-32 — the same bits as the two-step forms.
    const float offx = fmaf((float)hash(seed), 0x1p-32f, -0.5f);         // sample_square
    const float offy = fmaf((float)hash(seed * seed), 0x1p-32f, -0.5f);  // wgsl:299-303
    const float sx = ((float)x + 0.5f) + offx;
    const float sy = ((float)y + 0.5f) + offy;
    const v3 pc = fmas(sy, cam.pdv, fmas(sx, cam.pdu, cam.vul));
    // the lens centre in VGPRs (c0v, the copies the lens-less path needs anyway), so that
    // fma(u, ddu, centre) has one scalar operand (gfx950 VALU: one SGPR per instruction)
    // instead of a second copy per component; a caller tracing several pixels per lane
    // passes one copy for all of them
    v3 c0 = c0v ? *c0v : cam.center;
    if (!c0v) asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z));
    if (cam.defocus_angle > 0.0f) {                     // defocus_disk_sample wgsl:327-331
        const float ang = (float)hash(seed + 1u) * 0x1.921fb4p-30f;  // 2*3.1415926 * rf
        float sa, ca, ux, uy;
        // (ang = f32(hash) * 2pi 2^-32: always finite, so no NaN guard)
        sincos_k(ang, sa, ca, cam.k1s, cam.k1c, true);
        disk_unit<kTable>(sa, ca, ux, uy);
        o = fmas(uy, cam.ddv, fmas(ux, cam.ddu, c0));
    } else {
        // (made here: as a plain copy the compiler hoists it ahead of the branch, three
        // v_mov per pixel on every lens frame)
        o = c0;
        asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z));
    }
    d = sub(pc, o);
}

// A zero vector materialised where this is called: the frame loops' colour of a frame that
// traces nothing.  As a plain constant the compiler hoists its six v_mov ahead of the branch,
// onto every traced frame (12 per tile-pair frame in rt_tpair_kernel<2>).
__device__ __forceinline__ v3 zero_v3_here() {
    float x, y, z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(x));
    asm volatile("v_mov_b32 %0, 0" : "=v"(y));
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return mk(x, y, z);
}

// component-wise select of two v3 (a select of whole v3 values can leave them in
// scratch memory)
__device__ __forceinline__ v3 sel3(bool c, v3 a, v3 b) {
    return mk(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z);
}

// The reciprocal of |v| in the sky's normalize(d).y and in normalize_w comes from the square
// root's own rsq (sqrt_core_rcp) instead of a second transcendental (v_rcp).  Adopted in
// round 4 with the one-frame kernel's select skipping, the AND sign test and one record per
// tile and step (K3 14.95 -> 14.68 µs per update over three interleaved rounds;
// profiles/r04/r04k_ab_single_variants.txt).
// normalize(v) = v / sqrt(v.v) (WGSL normalize).  kFast: when every active lane's |v|^2 is
// in [2^-20, 2^40] (NaN, 0 and inf are not) and its components are >= 2^-100 in
// magnitude, sqrt_core and div_core with the shared reciprocal of |v| in [2^-10, 2^20]
// (components <= |v|: inside div_core's exact domain); otherwise the IEEE operations.
template <bool kFast>
__device__ __forceinline__ v3 normalize_w(v3 v) {
    if (kFast) {
        const float dd = dot(v, v);
        const uint32_t span = __float_as_uint(dd) - kBits2m20;
        // (a component below 2^-100: min_abs3 and an ordered compare, as in shade_hit)
        if ((mask_uge(span, kBits2p40 - kBits2m20) |
             __builtin_amdgcn_fcmpf(min_abs3(v), 0x1p-100f, 4)) == 0ull) {
            float y;
            const float len = sqrt_core_rcp(dd, y);
            return mk(div_core(v.x, len, y), div_core(v.y, len, y), div_core(v.z, len, y));
        }
    }
    return normalize(v);
}

// ray_color (wgsl:261-297), executed by the whole wave: `live` marks the lanes whose path
// is still being traced; the bounce loop runs while any lane is live, and a lane's
// values are only updated while it is live, so each lane computes exactly its own
// per-pixel result.
// uni (wave-uniform): every live lane of the wave holds the hinted sample count of frame
// f, so the scatter step's random numbers (pixel-independent, see TraceParams::hint_n)
// come from the host-computed hint_rs table instead of three hashes, a sqrt and a sincos
// per lane.
// The hit normal's (p - C) / R (wgsl:209) on div_core's domain (the callers check it),
// y = rcp_refined(R).  rn (wave-uniform, TraceParams::normal_rn): one Markstein step per
// component from y is the IEEE quotient for every numerator of the domain (the numerators
// >= 2^-100, R in [2^-20, 2^20] and |p - C| <= 2^43 keep the quotients normal) — checked
// exhaustively for every distinct radius of the scene on the device at upload
// (rt_rcp_check_kernel); otherwise div_core's two.
__device__ __forceinline__ v3 normal_div(v3 rel, float r, float y, bool rn) {
    if (rn) return mk(div_rn(rel.x, r, y), div_rn(rel.y, r, y), div_rn(rel.z, r, y));
    return mk(div_core(rel.x, r, y), div_core(rel.y, r, y), div_core(rel.z, r, y));
}

// One 16-B buffer load at a byte offset (raw buffer, no format conversion)
__device__ __forceinline__ float4 buf_f4(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                       __uint_as_float(v.w));
}

template <int kScan>
__device__ __forceinline__ v3 ray_color(const TraceParams& p, uint32_t tile, uint32_t ncand,
                                        uint32_t depth, v3 o, v3 d, uint32_t seed, bool live,
                                        bool uni, uint32_t f) {
    v3 cf = mk(1.0f, 1.0f, 1.0f);
    bool black = false;
    for (uint32_t i = 0; i < depth; ++i) {
        if (rt_ballot(live) == 0ull) break;
        // Camera rays of a tile with a candidate list (ncand != kCandNone) test only the
        // listed spheres: their records are in index order and padded like the full list,
        // so the same chunk loop applies; hit.idx then indexes the tile's copy of the
        // sphere records.
        const bool listed = kScan != kTraceExhaustive && i == 0 && ncand != kCandNone;
        const float4* blk = p.cand + (size_t)tile * kCandStride;
        // (one inlined walk for both pointers: two copies measured slower)
        const Hit hit =
            (kScan != kTraceCulled || listed)
                ? scan_exhaustive<scan_chunk<kScan>(), fast_core<kScan>(1), kScan != kTraceList>(
                      listed ? blk + kCandRecOff : p.geom, listed ? ncand : p.count, o, d)
            : p.lds_records ? scan_culled<true>(grid_params(p), p.geom, p.count, o, d, live, i > 0)
                            : scan_culled<false>(grid_params(p), p.geom, p.count, o, d, live, i > 0);
        const float4* hs = listed ? blk + kCandSphOff : p.sph;
        if (!live) continue;
        if (hit.idx < 0) {                                        // wgsl:288-290
            live = false;
            continue;
        }
        // Hit record of the winner (wgsl:205-218).  The two record loads are per-lane and
        // depend on the scan; the scatter's random numbers do not depend on the material
        // (lambertian and metal draw random_unit_vector(sb), dielectric draws rf(sb), its
        // first component), so they are computed while the loads are in flight.
        // (buffer loads here, as in single_sample, measured 1.5 % slower in the 8-rank share
        // kernel: profiles/r06/r06ax/)
        const float4 pr = hs[2 * hit.idx];          // position, radius
        const float4 mat = hs[2 * hit.idx + 1];     // material color
        float r_sb;
        v3 ruv;
        if (uni) {
            const float4 h = p.hint_rs[f * depth + i];
            r_sb = h.x;
            ruv = mk(h.y, h.z, h.w);
        } else {
            const uint32_t sb = hash(seed + i * 1000u);           // wgsl:268
            r_sb = rf(sb);
            ruv = random_unit_vector(r_sb, sb);
        }
        const v3 hp = fmas(hit.t, d, o);
        const v3 C = mk(pr.x, pr.y, pr.z);
        // wgsl:209: (p - C) / R.  Fast core: |R| in [2^-20, 2^20] (host-proven) and every
        // hit lane's three numerators >= 2^-100 in magnitude (they are <= 2^43: the hit
        // lies on a sphere of the bounded scene).
        const v3 rel = sub(hp, C);
        v3 outward;
        if (fast_core<kScan>(2) &&
            rt_ballot(min_abs3(rel) < 0x1p-100f) == 0ull) {    // (see shade_hit)
            const float y = rcp_refined(pr.w);
            outward = normal_div(rel, pr.w, y, p.normal_rn != 0u);
        } else {
            outward = divs(rel, pr.w);
        }
        const bool front = dot(d, outward) < 0.0f;
        const v3 n = sel3(front, outward, neg(outward));
        v3 att = mk(1.0f, 1.0f, 1.0f), nd = d;   // (defined on every path: kept in registers)
        if (mat.w < -1.0f) {                                      // lambertian wgsl:84-93
            const v3 dir = add(n, ruv);
            nd = sel3(dot(dir, dir) < 0x1.0c6f7ap-20f, n, dir);
            att = mk(mat.x, mat.y, mat.z);
        } else if (mat.w <= 1.0f) {                               // metal wgsl:95-100
            constexpr bool kF = fast_core<kScan>(8);
            const v3 refl = fmas(mat.w, ruv, normalize_w<kF>(reflect(d, n)));
            if (!(dot(refl, n) > 0.0f)) {                         // wgsl:277-279
                black = true;
                live = false;
                continue;
            }
            nd = normalize_w<kF>(refl);
            att = mk(mat.x, mat.y, mat.z);
        } else {                                                  // dielectric wgsl:102-135
            att = mk(1.0f, 1.0f, 1.0f);
            const float ratio = front ? 1.0f / mat.x : mat.x;
            constexpr bool kF = fast_core<kScan>(8);
            const v3 u = normalize_w<kF>(d);
            const float cos_t = fminf(dot(neg(u), n), 1.0f);
            const float sin_t = sqrtf(fmaf(-cos_t, cos_t, 1.0f));
            const bool cannot = ratio * sin_t > 1.0f;
            const bool refl = cannot || reflectance(cos_t, ratio) > r_sb;
            nd = normalize_w<kF>(sel3(refl, reflect(u, n), refract(u, n, ratio)));
        }
        cf = mul(cf, att);                                        // wgsl:285-286
        o = hp;
        d = nd;
    }
    if (black) return mk(0.0f, 0.0f, 0.0f);
    // Sky (wgsl:293-296): only normalize(d).y is used.  Fast core when every lane's |d|^2
    // is in [2^-20, 2^40] (NaN and 0 are not): sqrt_core is exact there, and so is
    // div_core(d.y, |d|) for |d.y| >= 2^-100; below that |uy| < 2^-80 and uy + 1 == 1
    // with either quotient.
    const float dd = dot(d, d);
    float uy;
    if (fast_core<kScan>(4) &&
        rt_ballot(__float_as_uint(dd) - kBits2m20 >= kBits2p40 - kBits2m20) == 0ull) {
        // (|d| and its reciprocal from one rsq, as the one-frame kernel's sky: no v_rcp)
        float y;
        const float len = sqrt_core_rcp(dd, y);
        uy = div_core(d.y, len, y);
    } else {
        uy = d.y / sqrtf(dd);
    }
    const float a = 0.5f * (uy + 1.0f);
    const float om = 1.0f - a;
    return mul(cf, mk(fmaf(a, 0.5f, om), fmaf(a, 0x1.666666p-1f, om), fmaf(a, 1.0f, om)));
}

// One wave = one 8x8 tile of the (local) image; lanes are row-major inside the tile.
// Control flow is wave-uniform down to the shading (the culled scan reduces across
// lanes); per-lane conditions of the reference (n < spp, the image bounds) become the
// `live` flag instead of branches.
// a colour's three channels as one vector store (LDS slots of the frame groups)
typedef float f3v __attribute__((ext_vector_type(3)));
struct TileCoord {
    uint32_t x, y;
    size_t idx;
    bool valid;
};

// Launch grid: blockIdx.y = local stripe band, blockIdx.x * 4 + wave = tile column.
__device__ __forceinline__ TileCoord tile_coord(uint32_t width, uint32_t height,
                                                uint32_t band_first, uint32_t band_step,
                                                uint32_t tx, uint32_t lband, uint32_t lane) {
    TileCoord t;
    t.x = tx * 8u + (lane & 7u);
    const uint32_t gband = band_first + lband * band_step;
    t.y = gband * RT_STRIPE_ROWS + (lane >> 3);
    const uint32_t ly = lband * RT_STRIPE_ROWS + (lane >> 3);
    t.valid = (t.x < width) && (t.y < height);
    t.idx = (size_t)ly * width + t.x;
    return t;
}
__device__ __forceinline__ TileCoord tile_coord(const TraceParams& p, uint32_t tx,
                                                uint32_t lband, uint32_t lane) {
    return tile_coord(p.width, p.height, p.band_first, p.band_step, tx, lband, lane);
}

// One sample of one frame for the pixels with `live` set, traced with sample count n
// (wgsl:352-358 without the accumulation).
template <int kScan>
__device__ __forceinline__ v3 sample(const TraceParams& p, const Cam& cam, uint32_t tile,
                                     uint32_t ncand, const TileCoord& tc, uint32_t hxy,
                                     uint32_t n, uint32_t B, uint32_t f, bool live, bool uni) {
    const uint32_t depth = p.depth;
    const uint32_t seed = 1u + n + B;                             // wgsl:353
    v3 o, d;
    get_ray<fast_core<kScan>(16) ? kTraceDisk : 0>(cam, tc.x, tc.y, hxy, seed * 25u + B, o,
                                                  d);                          // wgsl:311
    const v3 col = ray_color<kScan>(p, tile, ncand, depth, o, d, seed + 1u, live, uni, f);
    return col;
}

// acc: the pixel's loaded accumulator (unused when frame 0 resets it).  Without a hint the
// count is taken from acc before the first sample; with a hint the first frame is traced
// with the hinted count while the load is in flight and verified afterwards.
// kHint = false ignores the hint (counts from acc, full per-pixel random numbers): the
// frame-group instance's fallback, kept small so that the instance stays within 64 VGPRs.
template <int kScan, bool kHint = true>
__device__ __forceinline__ float4 trace_pixel(const TraceParams& p, const Cam& cam,
                                              uint32_t tile, uint32_t ncand,
                                              const TileCoord& tc, uint32_t hxy, float4 acc) {
    const uint32_t spp = p.spp;                                   // wgsl:343
    v3 c = mk(0.0f, 0.0f, 0.0f);
    uint32_t n = 0u;
    bool known = p.reset_first != 0u;                             // wgsl:345-350
    if (!known && (!kHint || p.hint_frames == 0u)) {
        c = mk(acc.x, acc.y, acc.z);                              // wgsl:339-341
        n = f2u(acc.w);
        known = true;
    }
    for (uint32_t f = 0; f < p.frames; ++f) {
        const uint32_t B = p.seed_b[f];                           // wgsl:311,353
        if (f == 0 && p.reset_first) {                            // wgsl:345-350
            c = mk(0.0f, 0.0f, 0.0f);
            n = 0u;
        }
        const bool hinted = kHint && f < p.hint_frames;
        uint32_t ng = known ? n : p.hint_n[0];   // count to trace with (unknown: f == 0)
        bool pending = tc.valid;
        for (;;) {
            const bool live = pending && ng < spp;                // wgsl:352
            v3 col = mk(0.0f, 0.0f, 0.0f);
            if (rt_ballot(live) != 0ull) {
                const bool uni = hinted && rt_ballot(live && ng != p.hint_n[f]) == 0ull;
                col = sample<kScan>(p, cam, tile, ncand, tc, hxy, ng, B, f, live, uni);
            }
            bool wrong = false;
            if (!known) {                                         // verify the hint
                c = mk(acc.x, acc.y, acc.z);
                n = f2u(acc.w);
                known = true;
                wrong = pending && n != ng;
            }
            if (pending && !wrong && n < spp) {
                const float k = (float)(n + 1u);                  // wgsl:356
                c = mk(c.x + (col.x - c.x) / k, c.y + (col.y - c.y) / k,
                       c.z + (col.z - c.z) / k);
                n += 1u;
            }
            if (rt_ballot(wrong) == 0ull) break;
            pending = wrong;                                      // retrace these pixels
            ng = n;
        }
        // Chained updates: frame f's image (wgsl:362-363) lands in the other ping-pong
        // buffer; the next frame would read it back (u32(f32(n)), wgsl:341) — here the
        // registers already hold it.  Only the last two frames' images survive the launch
        // (each buffer keeps the last frame written to it, and nothing reads a tile's
        // pixels during the launch but its own wave), so only they are stored — or every
        // frame's (store_each 2, rt_set_frame_images EVERY).
        if (kStoreEach<kScan> && p.store_each && (p.store_each == 2u || f + 2u >= p.frames) &&
            tc.valid)
            ((f & 1u) ? p.out2 : p.out)[tc.idx] = make_float4(c.x, c.y, c.z, (float)n);
        n = f2u((float)n);
    }
    return make_float4(c.x, c.y, c.z, (float)n);                  // wgsl:362
}
// Minimum waves per SIMD the compiler plans registers for.  7 rather than 8: at 8 it caps
// SGPRs near 80 and spills ~25 of them into VGPR lanes (v_writelane / v_readlane in the
// frame loop); at 7 the instances use 94 SGPRs and, at <= 64 VGPRs, still run 8 waves per
// SIMD (the frame-group instance needs 66 VGPRs: 7 waves).  K3: 29.0 vs 30.3 us per
// single-frame update, 18.2 vs 18.4 us per fused frame.
#ifndef RT_TRACE_MIN_WAVES
#define RT_TRACE_MIN_WAVES 7
#endif

// 256-thread workgroups: 4 waves = 4 tiles along a stripe band; grid (columns/4, bands).
inline dim3 tile_grid(const TraceParams& p, uint32_t waves = 4) {
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    return dim3((tiles_x + waves - 1u) / waves, p.local_bands);
}
}  // namespace rtk
