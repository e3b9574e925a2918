// rt_variance.hip — the kernels of rt_moments_update and rt_variance_filter
// (include/rt_variance.h has the normative definition; DESIGN.md §4.9 the measurements).  A
// translation unit of its own: the render's kernels (rt_kernels.hip), the denoiser's
// (rt_denoise.hip) and the reprojection's (rt_reproject.hip) are not recompiled with it.
//
// Every float operation below is the one the header names, in its order: the build has
// -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical to the
// NumPy restatements in tests/test_variance.py.
#include <hip/hip_runtime.h>

#include "rt_variance_kernels.h"

namespace rtk {

namespace {

__device__ __forceinline__ float luminance(float x, float y, float z) {
    return (0.2126f * x + 0.7152f * y) + 0.0722f * z;
}

}  // namespace

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
    const float L = luminance(sx, sy, sz);
    const float kk = k0 + 1.0f;
    p.moments[at] = make_float4(m1 + (L - m1) / kk, m2 + (L * L - m2) / kk, 0.0f, kk);
}

hipError_t launch_moments_update(const MomentsParams& p, hipStream_t stream) {
    const size_t px = (size_t)p.width * p.height;
    hipLaunchKernelGGL(rt_moments_update_kernel, dim3((uint32_t)((px + 255u) / 256u)), dim3(256),
                       0, stream, p);
    return hipGetLastError();
}

namespace {

// What a tap needs of a pixel: three 16-byte records and the variance, the LDS image's layout.
struct Texel {
    float4 a;   // c.r, c.g, c.b, the bits of sphere_id (0 without an id plane)
    float4 b;   // hit: p.x, p.y, p.z, t
    float4 n;   // n.x, n.y, n.z, c.a (the normal plane's face flag is not used)
    float v;    // this iteration's input variance
};

struct Acc {
    float sw, r, g, b, sv;
};

__device__ __forceinline__ bool is_miss(float t) {
    return !(t < __builtin_inff());
}

// v[idx] of this iteration: the header's v0 in iteration 0 (n: the image's count there)
__device__ __forceinline__ float load_variance(const VarianceParams& p, size_t idx, float n) {
    if (!p.moments) return p.vin[idx];
    const float4 m = p.moments[idx];
    float d = m.y - m.x * m.x;
    d = d > 0.0f ? d : 0.0f;
    const float nn = n > 1.0f ? n : 1.0f;
    return m.w >= p.min_history ? d / nn : p.fallback;
}

__device__ __forceinline__ Texel load_texel(const VarianceParams& p, size_t idx) {
    const float4 c = p.in[idx];
    const float4 nn = p.normal[idx];
    const uint32_t id = p.id ? p.id[idx] : 0u;
    Texel t;
    t.a = make_float4(c.x, c.y, c.z, __uint_as_float(id));
    t.b = p.hit[idx];
    t.n = make_float4(nn.x, nn.y, nn.z, c.w);
    t.v = load_variance(p, idx, c.w);
    return t;
}

// One tap of the 3 x 3 local variance: t, idbits and v are Q's, `inside`: Q is on the image.
__device__ __forceinline__ void local_tap(const Texel& P, bool missP, float t, float idbits,
                                          float v, bool inside, float g, float& sg,
                                          float& sgv) {
    if (inside && is_miss(t) == missP && __float_as_uint(idbits) == __float_as_uint(P.a.w)) {
        sg = sg + g;
        sgv = sgv + g * v;
    }
}

// One tap Q of pixel P with kernel weight k; `inside`: Q is on the image (Q's records are any
// readable texel's otherwise).  NP: normal_power_log2 at compile time, or -1 for the
// parameter's (a wave-uniform loop).  lP: L(c[P]); ve: the local variance + 1e-8f.
template <int NP>
__device__ __forceinline__ void tap(const VarianceParams& p, const Texel& P, bool missP,
                                    float lP, float ve, const Texel& Q, bool inside, float k,
                                    Acc& acc) {
    const bool same = is_miss(Q.b.w) == missP &&
                      __float_as_uint(Q.a.w) == __float_as_uint(P.a.w);
    const float dl = lP - luminance(Q.a.x, Q.a.y, Q.a.z);
    const float px = P.b.x - Q.b.x, py = P.b.y - Q.b.y, pz = P.b.z - Q.b.z;
    const float dp = missP ? 0.0f : (px * px + py * py) + pz * pz;
    const float dn = (P.n.x * Q.n.x + P.n.y * Q.n.y) + P.n.z * Q.n.z;
    float wn = dn > 0.0f ? dn : 0.0f;                     // max(dn, 0), NaN -> 0
    if (NP >= 0) {
#pragma unroll
        for (int r = 0; r < NP; ++r) wn = wn * wn;
    } else {
        for (uint32_t r = 0; r < p.npow; ++r) wn = wn * wn;
    }
    if (missP) wn = 1.0f;
    const float w = (((k * wn) * Q.n.w) * ve) / ((1.0f + dp * p.ip) * (ve + (dl * dl) * p.il));
    if (inside && same && w > 0.0f) {
        acc.sw = acc.sw + w;
        acc.r = acc.r + w * Q.a.x;
        acc.g = acc.g + w * Q.a.y;
        acc.b = acc.b + w * Q.a.z;
        acc.sv = acc.sv + (w * w) * Q.v;
    }
}

__device__ __forceinline__ void resolve(const VarianceParams& p, size_t at, const Texel& P,
                                        const Acc& acc) {
    const bool ok = acc.sw > 0.0f;
    p.out[at] = make_float4(ok ? acc.r / acc.sw : P.a.x, ok ? acc.g / acc.sw : P.a.y,
                            ok ? acc.b / acc.sw : P.a.z, P.n.w);
    const float sw2 = acc.sw * acc.sw;                    // 0 for a sum of weights near 1e-30
    p.vout[at] = sw2 > 0.0f ? acc.sv / sw2 : P.v;
}

// h (x) h, h = (1/16, 1/4, 3/8, 1/4, 1/16), and h3 (x) h3, h3 = (1/4, 1/2, 1/4): every
// product is exact
__device__ __forceinline__ constexpr float tap_h(int d) {
    return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f;
}
__device__ __forceinline__ constexpr float tap_h3(int d) {
    return d == 0 ? 0.5f : 0.25f;
}

}  // namespace

// The LDS route ("rows"), for a step S up to 16: rt_denoise_kernel's design (rt_denoise.hip,
// DESIGN.md §4.7) with one more staged plane.  A workgroup of 256 threads filters 64 x 4
// pixels: 64 consecutive pixels x0 + i of the four rows y0 + S * j, rows of one residue class
// y mod S.  It first stages the RX x 8 texels (x0 - 2 S + u, y0 + S * (v - 2)), RX = 64 + 4 S,
// as three float4 planes and the float plane of the variance: 52 * 8 * RX = 26 624 + 1 664 S
// bytes (28 288 for S = 1, 53 248 for S = 16).  Tap (dx, dy) of a pixel is then (S dx, dy)
// texels away in LDS, the 3 x 3 local variance's taps among them, which is why that mean runs
// at the iteration's spacing.  Block b of the grid's y axis is class b mod S, tile b / S.
// Texels off the image are zeros and never count (`inside`).
template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_kernel(const VarianceParams p) {
    constexpr uint32_t RX = 64u + 4u * S, RY = 8u;
    static_assert((S & (S - 1u)) == 0u && 52u * RX * RY <= 65536u,
                  "a power of two whose region fits a workgroup's LDS");
    __shared__ float4 sa[RX * RY];
    __shared__ float4 sb[RX * RY];
    __shared__ float4 sn[RX * RY];
    __shared__ float sv[RX * RY];
    const int W = (int)p.width, H = (int)p.height;
    constexpr int s = (int)S;
    const int x0 = (int)(64u * blockIdx.x);
    const int y0 = (int)(blockIdx.y & (S - 1u)) + s * (int)(4u * (blockIdx.y >> p.shift));
    if (y0 >= H) return;                                  // the whole workgroup: a short class
    for (uint32_t e = threadIdx.x; e < RX * RY; e += 256u) {
        const uint32_t v = e / RX, u = e - v * RX;
        const int X = x0 + (int)u - 2 * s;
        const int Y = y0 + s * ((int)v - 2);
        Texel t;
        t.a = t.b = t.n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        t.v = 0.0f;
        if (X >= 0 && X < W && Y >= 0 && Y < H) t = load_texel(p, (size_t)Y * p.width + (size_t)X);
        sa[e] = t.a;
        sb[e] = t.b;
        sn[e] = t.n;
        sv[e] = t.v;
    }
    __syncthreads();
    const uint32_t i = threadIdx.x & 63u, j = threadIdx.x >> 6;
    const int x = x0 + (int)i, y = y0 + s * (int)j;
    if (x >= W || y >= H) return;
    const int ctr = (int)((j + 2u) * RX + i + 2u * S);
    Texel P;
    P.a = sa[ctr];
    P.b = sb[ctr];
    P.n = sn[ctr];
    P.v = sv[ctr];
    const bool missP = is_miss(P.b.w);
    float sg = 0.0f, sgv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy * s;
        const bool row = qy >= 0 && qy < H;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx * s;
            const int q = ctr + dy * (int)RX + dx * s;
            local_tap(P, missP, sb[q].w, sa[q].w, sv[q], row && qx >= 0 && qx < W,
                      tap_h3(dy) * tap_h3(dx), sg, sgv);
        }
    }
    const float ve = sgv / sg + 1e-8f;
    const float lP = luminance(P.a.x, P.a.y, P.a.z);
    Acc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        const bool row = qy >= 0 && qy < H;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const int q = ctr + dy * (int)RX + dx * s;    // always inside the region
            Texel Q;
            Q.a = sa[q];
            Q.b = sb[q];
            Q.n = sn[q];
            Q.v = sv[q];
            tap<NP>(p, P, missP, lP, ve, Q, row && qx >= 0 && qx < W, tap_h(dy) * tap_h(dx),
                    acc);
        }
    }
    resolve(p, (size_t)y * p.width + (size_t)x, P, acc);
}

// The direct route: no LDS, every tap loads its texel from global memory.  A wave is 64
// consecutive pixels of a row, a workgroup four such rows.  A tap off the image reads the
// pixel's own texel instead and does not count.
template <int NP>
__global__ __launch_bounds__(256) void rt_variance_filter_direct_kernel(const VarianceParams p) {
    const int W = (int)p.width, H = (int)p.height;
    const int s = 1 << p.shift;
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= W || y >= H) return;
    const size_t at = (size_t)y * p.width + (size_t)x;
    const Texel P = load_texel(p, at);
    const bool missP = is_miss(P.b.w);
    float sg = 0.0f, sgv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;                  // wave-uniform: a wave is one row
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx * s;
            const bool inside = qx >= 0 && qx < W;
            const size_t q = inside ? (size_t)qy * p.width + (size_t)qx : at;
            const uint32_t id = p.id ? p.id[q] : 0u;
            const float n = p.moments ? p.in[q].w : 0.0f;
            local_tap(P, missP, p.hit[q].w, __uint_as_float(id), load_variance(p, q, n), inside,
                      tap_h3(dy) * tap_h3(dx), sg, sgv);
        }
    }
    const float ve = sgv / sg + 1e-8f;
    const float lP = luminance(P.a.x, P.a.y, P.a.z);
    Acc acc = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;                  // wave-uniform: a wave is one row
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const bool inside = qx >= 0 && qx < W;
            const Texel Q = load_texel(p, inside ? (size_t)qy * p.width + (size_t)qx : at);
            tap<NP>(p, P, missP, lP, ve, Q, inside, tap_h(dy) * tap_h(dx), acc);
        }
    }
    resolve(p, at, P, acc);
}

namespace {

template <uint32_t S>
void launch_rows(const VarianceParams& p, hipStream_t stream) {
    // per class of rows y mod S: ceil(ceil(height / S) / 4) tiles (classes past the image exit)
    const dim3 grid((p.width + 63u) / 64u, S * (((p.height + S - 1u) / S + 3u) / 4u));
    // the default power as straight-line code, any other as a loop
    if (p.npow == 5u)
        hipLaunchKernelGGL((rt_variance_filter_kernel<S, 5>), grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL((rt_variance_filter_kernel<S, -1>), grid, dim3(256), 0, stream, p);
}

}  // namespace

hipError_t launch_variance_filter(const VarianceParams& p, VarianceRoute route,
                                  hipStream_t stream) {
    if (route == kVarianceRows) {
        switch (p.shift) {
            case 0: launch_rows<1>(p, stream); break;
            case 1: launch_rows<2>(p, stream); break;
            case 2: launch_rows<4>(p, stream); break;
            case 3: launch_rows<8>(p, stream); break;
            case 4: launch_rows<16>(p, stream); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        const dim3 grid((p.width + 63u) / 64u, (p.height + 3u) / 4u);
        if (p.npow == 5u)
            hipLaunchKernelGGL(rt_variance_filter_direct_kernel<5>, grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL(rt_variance_filter_direct_kernel<-1>, grid, dim3(256), 0, stream,
                               p);
    }
    return hipGetLastError();
}

}  // namespace rtk
