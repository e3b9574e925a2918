// rt_denoise.hip — the edge-avoiding a-trous denoiser's kernels (include/rt_denoise.h has the
// normative definition; DESIGN.md §4.7 the measurements).  A translation unit of its own: the
// render's kernels (rt_kernels.hip) are not recompiled with it.
//
// One launch per iteration; the routes' geometry and tap walks are rt_atrous.h's, the filter
// below is its policy.  Every float operation is the one the header names, in its order: the
// build has -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical
// to the NumPy restatement in tests/test_denoise.py.
#include "rt_atrous.h"
#include "rt_denoise_kernels.h"

namespace rtk {

template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_denoise_kernel(const DenoiseParams p);
template <int NP>
__global__ __launch_bounds__(256) void rt_denoise_direct_kernel(const DenoiseParams p);

namespace {

struct DenoiseFilter {
    using Params = DenoiseParams;
    static constexpr bool kPrefilter = false;

    // What a tap needs of a pixel, as three 16-byte records: the LDS image's layout.
    struct Texel {
        float4 a;   // c.r, c.g, c.b, the bits of sphere_id (0 without an id plane)
        float4 b;   // hit: p.x, p.y, p.z, t
        float4 n;   // n.x, n.y, n.z, c.a (the normal plane's face flag is not used)
    };

    template <uint32_t N>
    struct Lds {
        float4 a[N], b[N], n[N];
        __device__ __forceinline__ void put(uint32_t e, const Texel& t) {
            a[e] = t.a;
            b[e] = t.b;
            n[e] = t.n;
        }
        __device__ __forceinline__ Texel get(int e) const { return {a[e], b[e], n[e]}; }
    };

    static __device__ __forceinline__ Texel load(const Params& p, size_t idx) {
        const float4 c = p.in[idx];
        const float4 nn = p.normal[idx];
        const uint32_t id = p.id ? p.id[idx] : 0u;
        return {make_float4(c.x, c.y, c.z, __uint_as_float(id)), p.hit[idx],
                make_float4(nn.x, nn.y, nn.z, c.w)};
    }

    static __device__ __forceinline__ Texel zero() {
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return {z, z, z};
    }

    template <int NP>
    struct Pixel {
        const Params& p;
        const Texel P;
        const bool missP;
        float sw = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f;

        __device__ __forceinline__ Pixel(const Params& p, const Texel& P)
            : p(p), P(P), missP(atrous::is_miss(P.b.w)) {}

        __device__ __forceinline__ void tap(const Texel& Q, bool inside, float k) {
            const bool same = atrous::is_miss(Q.b.w) == missP &&
                              __float_as_uint(Q.a.w) == __float_as_uint(P.a.w);
            const float ex = P.a.x - Q.a.x, ey = P.a.y - Q.a.y, ez = P.a.z - Q.a.z;
            const float dc = (ex * ex + ey * ey) + ez * ez;
            const float px = P.b.x - Q.b.x, py = P.b.y - Q.b.y, pz = P.b.z - Q.b.z;
            const float dp = missP ? 0.0f : (px * px + py * py) + pz * pz;
            const float dn = (P.n.x * Q.n.x + P.n.y * Q.n.y) + P.n.z * Q.n.z;
            float wn = atrous::normal_weight<NP>(dn, p.npow);
            if (missP) wn = 1.0f;
            const float w = (k * wn) / ((1.0f + dp * p.ip) * (1.0f + dc * p.ic));
            if (inside && same && w > 0.0f) {
                sw = sw + w;
                r = r + w * Q.a.x;
                g = g + w * Q.a.y;
                b = b + w * Q.a.z;
            }
        }

        __device__ __forceinline__ void resolve(size_t at) const {
            const bool ok = sw > 0.0f;
            p.out[at] = make_float4(ok ? r / sw : P.a.x, ok ? g / sw : P.a.y,
                                    ok ? b / sw : P.a.z, P.n.w);
        }
    };

    template <uint32_t S, int NP>
    static constexpr auto rows = &rt_denoise_kernel<S, NP>;
    template <int NP>
    static constexpr auto direct = &rt_denoise_direct_kernel<NP>;
};

}  // namespace

template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_denoise_kernel(const DenoiseParams p) {
    atrous::rows<DenoiseFilter, S, NP>(p);
}

template <int NP>
__global__ __launch_bounds__(256) void rt_denoise_direct_kernel(const DenoiseParams p) {
    atrous::direct<DenoiseFilter, NP>(p);
}

hipError_t launch_denoise(const DenoiseParams& p, AtrousRoute route, hipStream_t stream) {
    return atrous::launch<DenoiseFilter>(p, route, stream);
}

}  // namespace rtk
