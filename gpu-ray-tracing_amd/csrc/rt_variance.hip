// rt_variance.hip — the kernels of rt_moments_update and rt_variance_filter
// (include/rt_variance.h has the normative definition; DESIGN.md §4.9 the measurements).  A
// translation unit of its own: the render's kernels (rt_kernels.hip), the denoiser's
// (rt_denoise.hip) and the reprojection's (rt_reproject.hip) are not recompiled with it.
//
// Every float operation below is the one the header names, in its order (the rules shared with
// the sampler: rt_pixel_rules.h): the build has -ffp-contract=off, IEEE division and
// subnormals on, so the output is bit-identical to the NumPy restatements in
// tests/test_variance.py.
#include "rt_atrous.h"
#include "rt_pixel_rules.h"
#include "rt_variance_kernels.h"

namespace rtk {

// One lane per pixel, 16-byte loads and one 16-byte store; consecutive lanes consecutive
// pixels.  A lane past the image does nothing; a pixel under rule 3 stores nothing.
__global__ __launch_bounds__(256) void rt_moments_update_kernel(const MomentsParams p) {
    const size_t at = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= (size_t)p.width * p.height) return;
    const float4 O = p.out[at];
    float sx, sy, sz, k0, m1 = 0.0f, m2 = 0.0f;
    if (O.w == 1.0f) {                                                // rule 1
        sx = O.x;
        sy = O.y;
        sz = O.z;
        k0 = 0.0f;
    } else {
        const float4 I = p.in[at];
        if (O.w == I.w + 1.0f) {                                      // rule 2
            const float4 M = p.moments[at];
            // (recover_sample, written out: see rt_pixel_rules.h)
            sx = I.x + O.w * (O.x - I.x);
            sy = I.y + O.w * (O.y - I.y);
            sz = I.z + O.w * (O.z - I.z);
            k0 = M.w;
            if (!(k0 == 0.0f)) {
                m1 = M.x;
                m2 = M.y;
            }
        } else {
            if (!(O.w == I.w))                                        // rule 4 (rule 3: M stays)
                p.moments[at] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            return;
        }
    }
    p.moments[at] = moments_push(m1, m2, k0, luminance(sx, sy, sz));
}

hipError_t launch_moments_update(const MomentsParams& p, hipStream_t stream) {
    const size_t px = (size_t)p.width * p.height;
    hipLaunchKernelGGL(rt_moments_update_kernel, dim3((uint32_t)((px + 255u) / 256u)), dim3(256),
                       0, stream, p);
    return hipGetLastError();
}

template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_kernel(const VarianceParams p);
template <int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_direct_kernel(const VarianceParams p);

namespace {

// The variance-guided filter as rt_atrous.h's policy: the denoiser's three planes and the
// float plane of the variance, a 3 x 3 local variance at the iteration's spacing first (its
// taps are among the staged texels, which is why that mean runs at that spacing), the
// luminance weight, and the variance as a second output.
struct VarianceFilter {
    using Params = VarianceParams;
    static constexpr bool kPrefilter = true;

    // What a tap needs of a pixel: three 16-byte records and the variance, the LDS image's
    // layout.
    struct Texel {
        float4 a;   // c.r, c.g, c.b, the bits of sphere_id (0 without an id plane)
        float4 b;   // hit: p.x, p.y, p.z, t
        float4 n;   // n.x, n.y, n.z, c.a (the normal plane's face flag is not used)
        float v;    // this iteration's input variance
    };

    // What a tap of the 3 x 3 local variance needs of a pixel.
    struct Local {
        float t, idbits, v;
    };

    template <uint32_t N>
    struct Lds {
        float4 a[N], b[N], n[N];
        float v[N];
        __device__ __forceinline__ void put(uint32_t e, const Texel& t) {
            a[e] = t.a;
            b[e] = t.b;
            n[e] = t.n;
            v[e] = t.v;
        }
        __device__ __forceinline__ Texel get(int e) const { return {a[e], b[e], n[e], v[e]}; }
        __device__ __forceinline__ Local local(int e) const { return {b[e].w, a[e].w, v[e]}; }
    };

    // v[idx] of this iteration: the header's v0 in iteration 0 (n: the image's count there)
    static __device__ __forceinline__ float load_variance(const Params& p, size_t idx, float n) {
        if (!p.moments) return p.vin[idx];
        const float4 m = p.moments[idx];
        return gated_variance(m.x, m.y, m.w, n, p.min_history, p.fallback);
    }

    static __device__ __forceinline__ Texel load(const Params& p, size_t idx) {
        const float4 c = p.in[idx];
        const float4 nn = p.normal[idx];
        const uint32_t id = p.id ? p.id[idx] : 0u;
        return {make_float4(c.x, c.y, c.z, __uint_as_float(id)), p.hit[idx],
                make_float4(nn.x, nn.y, nn.z, c.w), load_variance(p, idx, c.w)};
    }

    static __device__ __forceinline__ Local load_local(const Params& p, size_t idx) {
        const uint32_t id = p.id ? p.id[idx] : 0u;
        const float n = p.moments ? p.in[idx].w : 0.0f;
        return {p.hit[idx].w, __uint_as_float(id), load_variance(p, idx, n)};
    }

    static __device__ __forceinline__ Texel zero() {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return {z, z, z, 0.0f};
    }

    template <int NP>
    struct Pixel {
        const Params& p;
        const Texel P;
        const bool missP;
        float sg = 0.0f, sgv = 0.0f;
        float lP = 0.0f, ve = 0.0f;   // L(c[P]); the local variance + 1e-8f
        float sw = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f, sv = 0.0f;

        __device__ __forceinline__ Pixel(const Params& p, const Texel& P)
            : p(p), P(P), missP(atrous::is_miss(P.b.w)) {}

        __device__ __forceinline__ void local(const Local& Q, bool inside, float k) {
            if (inside && atrous::is_miss(Q.t) == missP &&
                __float_as_uint(Q.idbits) == __float_as_uint(P.a.w)) {
                sg = sg + k;
                sgv = sgv + k * Q.v;
            }
        }

        __device__ __forceinline__ void local_done() {
            ve = sgv / sg + 1e-8f;
            lP = luminance(P.a.x, P.a.y, P.a.z);
        }

        __device__ __forceinline__ void tap(const Texel& Q, bool inside, float k) {
            const bool same = atrous::is_miss(Q.b.w) == missP &&
                              __float_as_uint(Q.a.w) == __float_as_uint(P.a.w);
            const float dl = lP - luminance(Q.a.x, Q.a.y, Q.a.z);
            const float px = P.b.x - Q.b.x, py = P.b.y - Q.b.y, pz = P.b.z - Q.b.z;
            const float dp = missP ? 0.0f : (px * px + py * py) + pz * pz;
            const float dn = (P.n.x * Q.n.x + P.n.y * Q.n.y) + P.n.z * Q.n.z;
            float wn = atrous::normal_weight<NP>(dn, p.npow);
            if (missP) wn = 1.0f;
            const float w =
                (((k * wn) * Q.n.w) * ve) / ((1.0f + dp * p.ip) * (ve + (dl * dl) * p.il));
            if (inside && same && w > 0.0f) {
                sw = sw + w;
                r = r + w * Q.a.x;
                g = g + w * Q.a.y;
                b = b + w * Q.a.z;
                sv = sv + (w * w) * Q.v;
            }
        }

        __device__ __forceinline__ void resolve(size_t at) const {
            const bool ok = sw > 0.0f;
            p.out[at] = make_float4(ok ? r / sw : P.a.x, ok ? g / sw : P.a.y,
                                    ok ? b / sw : P.a.z, P.n.w);
            const float sw2 = sw * sw;                    // 0 for a sum of weights near 1e-30
            p.vout[at] = sw2 > 0.0f ? sv / sw2 : P.v;
        }
    };

    template <uint32_t S, int NP>
    static constexpr auto rows = &rt_variance_filter_kernel<S, NP>;
    template <int NP>
    static constexpr auto direct = &rt_variance_filter_direct_kernel<NP>;
};

}  // namespace

template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_kernel(const VarianceParams p) {
    atrous::rows<VarianceFilter, S, NP>(p);
}

template <int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_direct_kernel(const VarianceParams p) {
    atrous::direct<VarianceFilter, NP>(p);
}

hipError_t launch_variance_filter(const VarianceParams& p, AtrousRoute route, hipStream_t stream) {
    return atrous::launch<VarianceFilter>(p, route, stream);
}

}  // namespace rtk
