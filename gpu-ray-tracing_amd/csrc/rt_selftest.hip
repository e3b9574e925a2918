// rt_selftest.hip — the device checks of the exact fast paths: rt_selftest_fastmath
// (rt_selftest_kernel), rt_selftest_roots (include/rt_selftest_roots.h) and the scene upload's
// rt_rcp_check_kernel.  They replay rt_device.h's cores and the root selections of the tracer's
// device library (rt_trace_device.h) against the IEEE operations.  A translation unit of its
// own, built with the render kernels' flags: the render kernels' compile unit (rt_kernels.hip)
// does not change with it.
//
// rt_rcp_check_kernel is here although its caller is the scene upload (rt_abi.cpp, which sets
// TraceParams::normal_rn from it) and not a self-test entry point: it is the same kind of
// kernel — an exhaustive comparison of div_rn with the IEEE division, untimed — and the
// self-test's div_rn cases lean on it for the radii they leave out.
#include "rt_trace_device.h"

namespace rtk {

// ---- Self-test of the exact fast paths (rt_selftest_fastmath) ------------------------
// cnt[0]: defocus normalisation, all 2^32 values of hash(seed + 1): both disk_unit forms vs
//         sqrtf and the IEEE divisions (also the eight-value range of len2 disk_unit<3> needs).
// cnt[1]: div_core_signed vs a / b on random a, b over div_core's domain (rt_device.h:
//         |b| in [2^-20, 2^33), |a| in [2^-100, 2^91), exponent gap in [-120, 88]; a also
//         +-0, b also the accumulator's n + 1 up to 2^32) and over [2^-40, 2^40]^2;
//         div_rn (y = RN32(1 / b)) vs a / b beyond integer denominators (|b| in
//         [2^-20, 2^20], |a| in [2^-100, 2^43], where |b y - 1| <= 2^-25; half of them with
//         both significands near 2); and acc_rn vs c + num / k for numerators acc_ok accepts
//         (finite f32 bits or NaN, many near the subnormal range) and k in [1, 2^22).
// cnt[2]: sqrt_core vs sqrtf on every finite x >= 2^-96 (exhaustive).
// cnt[3]: consider_fast vs consider and consider_any_fast vs consider_any (root selection:
//         tmax and index) on the first n_rand cases of make_root_case below, over the domain
//         the guards admit (roots_fast_wave and TraceParams::roots_fast: |d|^2 in
//         [2^-11, 2^20], every origin component below 2^39, |C| + |R| <= 2^40); the cases in
//         which either pair differs.  rt_selftest_roots counts the same cases per family and
//         stratum, with what was drawn and what was really compared.
// cnt[4]: cases run.
RT_HD uint32_t mix32(uint64_t i, uint32_t salt) {
    return hash((uint32_t)i ^ hash((uint32_t)(i >> 32) + salt));
}
// sign from r's top bit, mantissa from r, exponent e (unbiased; -127: a subnormal)
RT_HD float with_exp(uint32_t r, int e) {
    const uint32_t u = (r & 0x807FFFFFu) | ((uint32_t)(127 + e) << 23);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
RT_HD float unit_rand(uint32_t r) {   // [-1, 1)
    return (float)(int32_t)r * 0x1p-31f;
}
__device__ __forceinline__ bool same_bits(float x, float y) {   // NaN == NaN
    return __float_as_uint(x) == __float_as_uint(y) || (x != x && y != y);
}
// One generated ray and sphere.  Case i belongs to stratum i & 3: bit 0 = "far" (|O| or |C|
// in [2^38, 2^40]), bit 1 = "edge" (a = |d|^2 within one binade of an end of [2^-11, 2^20]).
// The magnitudes are chosen so that nearly every case lands in the guards' domain and in
// its stratum by construction; `ok` is the check of both on the values as generated, and
// only such cases are compared.  (Host and device: plain f32 / f64 arithmetic.)
struct RootCase {
    v3 o, d, C;
    float R, t0;       // t0: the ray parameter of the point the centre was placed beside
    uint32_t bits;     // random bits for the incoming (tmax, idx) and the item table
    bool ok;
};
RT_HD RootCase make_root_case(uint64_t i) {
    const bool far = (i & 1u) != 0u, edge = (i & 2u) != 0u;
    const uint32_t r0 = mix32(i, 11u), r1 = mix32(i, 12u), r2 = mix32(i, 13u),
                   r3 = mix32(i, 14u), r4 = mix32(i, 15u), r5 = mix32(i, 16u),
                   r6 = mix32(i, 17u), r7 = mix32(i, 18u), r8 = mix32(i, 19u),
                   r9 = mix32(i, 20u);
    // one in sixteen edge cases: a exactly 2^-11 or 2^20 (axis-aligned components)
    const bool exact = edge && (r0 & 0xFu) == 0u;
    // far cases, where the large magnitudes sit: 0 = O far with C near it, 1 = C far from a
    // near O, 2 = O far looking back at a C near the coordinate origin, 3 = O far on one
    // side and C far on the other (the largest |C - O|, |h| and sqrt(D))
    const uint32_t mode = ((r0 >> 4) & 3u) & (exact ? 1u : 3u);
    const bool high = ((r0 >> 6) & 1u) != 0u;
    const float ta = with_exp(r1 & 0x7FFFFFu,
                              edge ? (high ? 19 : -11) : -11 + (int)((r0 >> 7) % 31u));
    // the origin: every component below 2^37 (2^36 beside a far one); far: one in [2^38, 2^39)
    const bool o_far = far && mode != 1u;
    const float os = with_exp(0u, -10 + (int)((r0 >> 12) % (far ? 47u : 48u)));
    v3 o = mk(unit_rand(r2) * os, unit_rand(r3) * os, unit_rand(r4) * os);
    if (o_far) {
        const float big = with_exp(r2, 38);
        const uint32_t ax = r5 % 3u;
        o = mk(ax == 0u ? big : o.x, ax == 1u ? big : o.y, ax == 2u ? big : o.z);
    }
    // the direction: anywhere; in modes 2 and 3 within 2^-3 or less of the way back
    v3 u = mk(unit_rand(r5), unit_rand(r6), unit_rand(r7));
    const float ol = sqrtf(dot(o, o));
    if (o_far && mode >= 2u) {
        const float w = with_exp(0u, -3 - (int)(r8 % 18u));
        u = mk(fmaf(w, u.x, -o.x / ol), fmaf(w, u.y, -o.y / ol), fmaf(w, u.z, -o.z / ol));
    }
    float us = sqrtf(ta / dot(u, u));
    if (exact) {
        const float s0 = (r5 >> 31) ? -1.0f : 1.0f, s1 = (r6 >> 31) ? -1.0f : 1.0f;
        const float t1 = high ? 0.0f : s1;     // 2^20 = (2^10)^2; 2^-11 = 2 (2^-6)^2
        const uint32_t ax = r7 % 3u;
        u = ax == 0u ? mk(s0, t1, 0.0f) : ax == 1u ? mk(0.0f, s0, t1) : mk(t1, 0.0f, s0);
        us = high ? 0x1p10f : 0x1p-6f;
    }
    const v3 d = mk(u.x * us, u.y * us, u.z * us);
    const float a = dot(d, d);
    // the radius: half in [2^-20, 2^21), a quarter below (subnormals included), a quarter
    // above (to 2^36: with the placements below the sphere stays inside 2^40)
    const uint32_t rc = (r0 >> 20) & 3u;
    const int er = rc < 2u ? -20 + (int)(r9 % 41u)
                           : rc == 2u ? -127 + (int)(r9 % 107u) : 21 + (int)(r9 % 15u);
    float R = with_exp(r3 & 0x7FFFFFu, er);
    // the point of the ray the centre is placed beside, |t0 d| away from the origin
    float reach = with_exp(r4 & 0x7FFFFFu, -12 + (int)((r0 >> 26) % (far ? 48u : 50u)));
    if (far && mode == 1u) reach = with_exp(r4 & 0x7FFFFFu, 38);
    if (o_far && mode == 2u) reach = ol + unit_rand(r4) * with_exp(0u, 36);
    if (o_far && mode == 3u) reach = ol + with_exp(r4 & 0x7FFFFFu, 38);
    // (one in eight behind the origin, where that keeps the placement)
    const bool behind = ((r8 >> 18) & 7u) == 0u && !(o_far && mode >= 2u);
    const float t0 = behind ? -reach / sqrtf(a) : reach / sqrtf(a);
    const v3 P = mk(fmaf(t0, d.x, o.x), fmaf(t0, d.y, o.y), fmaf(t0, d.z, o.z));
    // sideways from it: by R (1 + 2^-j) to either side of grazing, anywhere inside the sphere,
    // or (a quarter of the large radii) anywhere, with the radius that brings |C| + R to
    // 2^40 (1 - 2^-j): the scene bound's end, evaluated in double as rt_abi.cpp does
    v3 side = mk(unit_rand(r4 ^ r2), unit_rand(r5 ^ r3), unit_rand(r6 ^ r4));
    const float sd = dot(side, d) / a;
    side = sub(side, mk(sd * d.x, sd * d.y, sd * d.z));           // ~perpendicular to d
    const float sl = sqrtf(dot(side, side));
    const bool graze = ((r8 >> 21) & 1u) != 0u;
    const bool brim = !graze && rc == 3u && ((r8 >> 22) & 1u) != 0u;
    const float jitter = 1.0f + unit_rand(r5) * with_exp(0u, -(int)(r1 % 31u));
    const float k = (brim ? unit_rand(r7) * with_exp(0u, (int)((r8 >> 23) % 36u))
                          : graze ? R * jitter : R * fabsf(unit_rand(r7))) / sl;
    const v3 C = mk(fmaf(k, side.x, P.x), fmaf(k, side.y, P.y), fmaf(k, side.z, P.z));
    const double cl = sqrt((double)C.x * C.x + (double)C.y * C.y + (double)C.z * C.z);
    if (brim) {
        const double want = 0x1p40 * (1.0 - (double)with_exp(0u, -1 - (int)((r8 >> 8) % 40u))) - cl;
        if (want > 0.0 && (double)(float)want <= want) R = (float)want;   // (else as drawn)
    }
    const double om = fmax(fmax(fabs((double)o.x), fabs((double)o.y)), fabs((double)o.z));
    const double far_of = fmax(sqrt((double)o.x * o.x + (double)o.y * o.y + (double)o.z * o.z), cl);
    RootCase c;
    c.o = o;
    c.d = d;
    c.C = C;
    c.R = R;
    c.t0 = t0;
    c.bits = mix32(i, 21u);
    c.ok = a >= 0x1p-11f && a <= 0x1p20f && om < 0x1p39 && R >= 0.0f && cl + (double)R <= 0x1p40 &&
           sl > 0.0f && (!far || (far_of >= 0x1p38 && far_of <= 0x1p40)) &&
           (!edge || a <= 0x1p-10f || a >= 0x1p19f);
    return c;
}
// The grid's item array in miniature (consider_any's `items`: slot -> sphere index)
__device__ const uint32_t kRootItems[8] = {5u, 2u, 9u, 0u, 7u, 3u, 11u, 1u};
struct RootResult {
    bool ok, rooted, bad_fast, bad_any;
};
// Case i through both root selections and their IEEE originals.  The incoming tmax: the
// scan's sentinel, |t0| (between the sphere's two roots), |t0| / 2 (below them), or a tie —
// the root the IEEE selection accepts from the sentinel, itself or one of its two neighbours
// (itself: consider's "tmax <= root" rejects and consider_any's "si < idx" decides, so a fast
// root one ulp off flips the answer).  consider_any's incoming idx is the sphere's own
// index + 1 or - 1, its index read from the item table or the slot itself.
__device__ __forceinline__ RootResult root_case(uint64_t i) {
    const RootCase c = make_root_case(i);
    RootResult res = {c.ok, false, false, false};
    if (!c.ok) return res;
    const float a = dot(c.d, c.d);
    const float ya = rcp_refined(a);
    float h;
    const float disc = discriminant(make_float4(c.C.x, c.C.y, c.C.z, c.R * c.R), c.o, c.d, a, h);
    res.rooted = !(disc < 0.0f);
    float tr = 0x1.05ed2ep+118f;
    int ir = -1;
    consider(disc, h, a, 3u, tr, ir);
    const uint32_t tk = c.bits & 3u;
    float t_in = tk == 0u ? 0x1.05ed2ep+118f : tk == 1u ? fabsf(c.t0) : fabsf(c.t0) * 0.5f;
    if (tk == 3u) {
        const uint32_t nb = (c.bits >> 2) & 3u;       // 0, 1: the root; 2: above; 3: below
        t_in = ir < 0 ? fabsf(c.t0)
                      : __uint_as_float(__float_as_uint(tr) + (nb == 2u ? 1u : nb == 3u ? ~0u : 0u));
    }
    {
        float t1 = t_in, t2 = t_in;
        int i1 = 7, i2 = 7;
        consider(disc, h, a, 3u, t1, i1);
        consider_fast(disc, h, a, ya, 3u, t2, i2);
        res.bad_fast = !(same_bits(t1, t2) && i1 == i2);
    }
    {
        const uint32_t* items = (c.bits & 0x10u) ? kRootItems : nullptr;
        const uint32_t slot = (c.bits >> 5) & 7u;
        const int si = (int)(items ? kRootItems[slot] : slot);
        const int i_in = (c.bits & 0x100u) ? si + 1 : si - 1;
        float t1 = t_in, t2 = t_in;
        int i1 = i_in, i2 = i_in;
        consider_any(disc, h, a, slot, t1, i1, items);
        consider_any_fast(disc, h, a, ya, slot, t2, i2, items);
        res.bad_any = !(same_bits(t1, t2) && i1 == i2);
    }
    return res;
}
// rt_selftest_roots: cnt[(family * kRootStrata + stratum) * 4 + {mismatches, drawn, compared,
// rooted}].  The grid's stride is a multiple of four, so a thread's cases share a stratum.
__global__ __launch_bounds__(256) void rt_selftest_roots_kernel(unsigned long long* cnt,
                                                                uint64_t n_rand) {
    unsigned long long drawn = 0, compared = 0, rooted = 0, bad_fast = 0, bad_any = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = first; i < n_rand; i += stride) {
        const RootResult r = root_case(i);
        ++drawn;
        compared += r.ok;
        rooted += r.rooted;
        bad_fast += r.bad_fast;
        bad_any += r.bad_any;
    }
    const uint32_t stratum = (uint32_t)first & (kRootStrata - 1u);
    for (uint32_t f = 0; f < kRootFamilies; ++f) {
        unsigned long long* c = cnt + (f * kRootStrata + stratum) * 4u;
        atomicAdd(&c[0], f == 0u ? bad_fast : bad_any);
        atomicAdd(&c[1], drawn);
        atomicAdd(&c[2], compared);
        atomicAdd(&c[3], rooted);
    }
}
__global__ __launch_bounds__(256) void rt_selftest_kernel(unsigned long long* cnt, uint64_t n_rand) {
    unsigned long long bad0 = 0, bad1 = 0, bad2 = 0, bad3 = 0, runs = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32);
         i += stride) {
        const float ang = 0x1.921fb4p+2f * rf((uint32_t)i);
        float sa, ca;
        sincos_c(ang, sa, ca);
        const float len_ref = sqrtf(fmaf(sa, sa, ca * ca));
        const float ux_ref = ca / len_ref, uy_ref = sa / len_ref;
        float ux, uy, fx, fy;
        disk_unit<0>(sa, ca, ux, uy);
        disk_unit<3>(sa, ca, fx, fy);
        bad0 += (__float_as_uint(fx) != __float_as_uint(ux_ref)) ||
                (__float_as_uint(fy) != __float_as_uint(uy_ref)) ||
                (__float_as_uint(ux) != __float_as_uint(ux_ref)) ||
                (__float_as_uint(uy) != __float_as_uint(uy_ref));
        const float x = __uint_as_float((uint32_t)i);
        if ((uint32_t)i >= 0x0F800000u && (uint32_t)i < 0x7F800000u)   // [2^-96, +inf)
            bad2 += __float_as_uint(sqrt_core(x)) != __float_as_uint(sqrtf(x));
        ++runs;
    }
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_rand; i += stride) {
        const uint32_t r0 = mix32(i, 1u), r1 = mix32(i, 2u), r2 = mix32(i, 3u);
        float a, b;
        if (r2 & 0x40000000u) {                       // the general domain
            const int eb = -20 + (int)(r2 % 53u);
            int ea = -100 + (int)((r2 >> 8) % 191u);
            ea = max(eb - 120, min(eb + 88, ea));
            a = with_exp(r0, ea);
            b = with_exp(r1, eb);
        } else {                                      // [2^-40, 2^40]^2
            a = with_exp(r0, -40 + (int)(r2 % 80u));
            b = with_exp(r1, -40 + (int)((r2 >> 8) % 80u));
        }
        if ((r2 & 0x70000u) == 0) a = (r0 & 1u) ? -0.0f : 0.0f;
        if ((r2 & 0x380000u) == 0)                    // n + 1 counts, n < 2^32 - 1
            b = (float)((r2 & 0x400000u) ? 1u + (r1 & 0xFFFFFFu) : max(r1, 1u));
        bad1 += !same_bits(div_core_signed(a, b, rcp_refined(b)), a / b);
        {   // root selection: both families on case i (compared only inside the domain)
            const RootResult rr = root_case(i);
            bad3 += rr.bad_fast || rr.bad_any;
        }
        {   // the sky's d.y / |d| with |d| and its reciprocal from one rsq (sqrt_core_rcp):
            // |d|^2 in [2^-20, 2^40], |d.y| <= |d| (and >= 2^-100 or zero)
            const float dd = with_exp(r1 & 0x7FFFFFu, -20 + (int)(r2 % 60u));
            float y;
            const float len = sqrt_core_rcp(dd, y);
            const float dy = (r0 & 0x1000u) ? 0.0f : unit_rand(r0) * len;
            if (dd <= 0x1p40f && (dy == 0.0f || fabsf(dy) >= 0x1p-100f))
                bad1 += !same_bits(div_core(dy, len, y), dy / sqrtf(dd));
        }
        {   // div_rn with real denominators where Markstein's hypothesis holds: y = RN32(1 / b)
            // and |b y - 1| <= 2^-25, so q = RN(a y) is within an ulp of a / b; every other
            // case the kernels' callers rule out (the radii are checked exhaustively at
            // upload, rt_rcp_check_kernel; the accumulator's k is an integer < 2^22).  Half
            // the cases in the corner where |b y - 1| approaches 2^-24: divisor significands
            // in [1.99, 2), numerator significands within 2^-11 of 2.
            const bool corner = (r2 >> 20) & 1u;
            const uint32_t mb = corner ? 0x7EB852u + r1 % (0x800000u - 0x7EB852u) : r1;
            const uint32_t ma = corner ? 0x7FFFFFu - (r0 % 4096u) : (r0 ^ r2);
            const float rb = with_exp((r1 & 0x80000000u) | (mb & 0x7FFFFFu), -20 + (int)(r2 % 41u));
            const float ra = with_exp((r0 & 0x80000000u) | (ma & 0x7FFFFFu),
                                      -100 + (int)((r2 >> 8) % 144u));
            const float yb = 1.0f / rb;
            if (fabsf(fmaf(rb, yb, -1.0f)) <= 0x1p-25f)
                bad1 += !same_bits(div_rn(ra, rb, yb), ra / rb);
        }
        // the accumulator's Markstein division: any finite f32 numerator or NaN (r0's bits:
        // zeros and subnormals included; the kernels' num = col - c is never +-inf against a
        // finite c, see acc_ok), k = f32(n + 1) for n + 1 in [1, 2^22) (kAccRnMax)
        const uint32_t kk = (r2 & 0x800000u) ? 1u + (r1 % (kAccRnMax - 1u))
                                             : 1u + (r1 % 4096u);   // small counts too
        const v3 num = mk(__uint_as_float(r0), __uint_as_float(r0 ^ r1),
                          __uint_as_float(r2 & 0x83FFFFFFu));       // (many tiny ones)
        if (acc_ok(num) && !isinf(num.x) && !isinf(num.y) && !isinf(num.z)) {
            const float kf = (float)kk;
            const v3 c0 = mk(0.0f, 0.0f, 0.0f);
            const v3 q = acc_rn(c0, num, kf, 1.0f / kf);
            bad1 += !same_bits(q.x, 0.0f + num.x / kf) || !same_bits(q.y, 0.0f + num.y / kf) ||
                    !same_bits(q.z, 0.0f + num.z / kf);
        }
        ++runs;
    }
    atomicAdd(&cnt[0], bad0);
    atomicAdd(&cnt[1], bad1);
    atomicAdd(&cnt[2], bad2);
    atomicAdd(&cnt[3], bad3);
    atomicAdd(&cnt[4], runs);
}

// TraceParams::normal_rn: is one Markstein step from y = rcp_refined(R) the IEEE quotient
// a / R for every numerator the kernels divide, for every distinct radius R of the scene?
// Markstein's theorem needs y within half an ulp of 1 / R AND q = RN(a y) within one ulp of
// a / R; a correctly rounded y alone gives |R y - 1| <= 2^-24, and with a divisor's and a
// quotient's significands both near 2 q can then be 1.5 ulp off (round-5 ADVICE).  So the
// check is exhaustive instead of sufficient: for each radius every numerator significand
// (2^23 of them) in two binades, [1, 2) and [2^-100, 2^-99) (the kernels' smallest
// numerators), against the IEEE division.  A step and its operands scale exactly by powers of
// two while q, the residual and the result stay normal (numerators in [2^-100, 2^43], R in
// [2^-20, 2^20]: the callers' domain), so these two binades cover every numerator; the sign
// is symmetric.  One thread per (radius, significand, binade), a vector atomic OR on a miss.
constexpr uint32_t kRcpCheckPerRadius = 2u << 23;
__global__ __launch_bounds__(256) void rt_rcp_check_kernel(const float* radii, uint32_t n,
                                                           uint32_t* bad) {
    const uint64_t total = (uint64_t)n * kRcpCheckPerRadius;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t miss = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const float r = radii[i / kRcpCheckPerRadius];
        const uint32_t j = (uint32_t)(i % kRcpCheckPerRadius);
        // significand j & 0x7FFFFF; binade 2^0 or 2^-100
        const float a = __uint_as_float(((j >> 23) ? 0x0D800000u : 0x3F800000u) | (j & 0x7FFFFFu));
        const float y = rcp_refined(r);
        miss |= __float_as_uint(div_rn(a, r, y)) != __float_as_uint(a / r);
    }
    if (miss) atomicOr(bad, 1u);
}
hipError_t launch_rcp_check(const float* radii, uint32_t n, uint32_t* bad, hipStream_t stream) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(rt_rcp_check_kernel, dim3(2048), dim3(256), 0, stream, radii, n, bad);
    return hipGetLastError();
}

hipError_t launch_selftest(unsigned long long* cnt, uint64_t n_rand, hipStream_t stream) {
    hipLaunchKernelGGL(rt_selftest_kernel, dim3(8192), dim3(256), 0, stream, cnt, n_rand);
    return hipGetLastError();
}
hipError_t launch_selftest_roots(unsigned long long* cnt, uint64_t n_rand, hipStream_t stream) {
    // (256 x 2048 threads: a multiple of kRootStrata, see the kernel)
    hipLaunchKernelGGL(rt_selftest_roots_kernel, dim3(2048), dim3(256), 0, stream, cnt, n_rand);
    return hipGetLastError();
}

}  // namespace rtk
