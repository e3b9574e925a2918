// rt_denoise.hip — the edge-avoiding a-trous denoiser's kernels (include/rt_denoise.h has the
// normative definition; DESIGN.md §4.7 the measurements).  A translation unit of its own: the
// render's kernels (rt_kernels.hip) are not recompiled with it.
//
// One launch per iteration.  Every float operation below is the one the header names, in its
// order: the build has -ffp-contract=off, IEEE division and subnormals on, so the output is
// bit-identical to the NumPy restatement in tests/test_denoise.py.
#include <hip/hip_runtime.h>

#include "rt_denoise_kernels.h"

namespace rtk {

namespace {

// What a tap needs of a pixel, as three 16-byte records: the LDS image's layout.
struct Texel {
    float4 a;   // c.r, c.g, c.b, the bits of sphere_id (0 without an id plane)
    float4 b;   // hit: p.x, p.y, p.z, t
    float4 n;   // n.x, n.y, n.z, c.a (the normal plane's face flag is not used)
};

struct Acc {
    float sw, r, g, b;
};

__device__ __forceinline__ bool is_miss(const float4& hit) {
    return !(hit.w < __builtin_inff());
}

__device__ __forceinline__ Texel load_texel(const DenoiseParams& p, size_t idx) {
    const float4 c = p.in[idx];
    const float4 nn = p.normal[idx];
    const uint32_t id = p.id ? p.id[idx] : 0u;
    Texel t;
    t.a = make_float4(c.x, c.y, c.z, __uint_as_float(id));
    t.b = p.hit[idx];
    t.n = make_float4(nn.x, nn.y, nn.z, c.w);
    return t;
}

// One tap Q of pixel P with kernel weight k; `inside`: Q is on the image (Q's records are
// any readable texel's otherwise).  NP: normal_power_log2 at compile time, or -1 for the
// parameter's (a wave-uniform loop).
template <int NP>
__device__ __forceinline__ void tap(const DenoiseParams& p, const Texel& P, bool missP,
                                    const Texel& Q, bool inside, float k, Acc& acc) {
    const bool same = is_miss(Q.b) == missP &&
                      __float_as_uint(Q.a.w) == __float_as_uint(P.a.w);
    const float ex = P.a.x - Q.a.x, ey = P.a.y - Q.a.y, ez = P.a.z - Q.a.z;
    const float dc = (ex * ex + ey * ey) + ez * ez;
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
    const float w = (k * wn) / ((1.0f + dp * p.ip) * (1.0f + dc * p.ic));
    if (inside && same && w > 0.0f) {
        acc.sw = acc.sw + w;
        acc.r = acc.r + w * Q.a.x;
        acc.g = acc.g + w * Q.a.y;
        acc.b = acc.b + w * Q.a.z;
    }
}

__device__ __forceinline__ float4 resolve(const Texel& P, const Acc& acc) {
    const bool ok = acc.sw > 0.0f;
    return make_float4(ok ? acc.r / acc.sw : P.a.x, ok ? acc.g / acc.sw : P.a.y,
                       ok ? acc.b / acc.sw : P.a.z, P.n.w);
}

// h (x) h, h = (1/16, 1/4, 3/8, 1/4, 1/16): every product is exact
__device__ __forceinline__ constexpr float tap_h(int d) {
    return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f;
}

}  // namespace

// The LDS route ("rows"), for a step S up to 16.  A workgroup of 256 threads filters 64 x 4
// pixels: 64 consecutive pixels x0 + i of the four rows y0 + S * j, rows of one residue class
// y mod S, for which the filter's vertical taps are the neighbouring rows of the class.  It
// first stages the RX x 8 texels (x0 - 2 S + u, y0 + S * (v - 2)), RX = 64 + 4 S — a halo of 2 S
// pixels along x, of 2 class rows along y — as three float4 planes: 48 * 8 * RX = 24 576 +
// 1 536 S bytes (26 112 for S = 1, 49 152 for S = 16).  Tap (dx, dy) of a pixel is then
// (S dx, dy) texels away in LDS.  Block b of the grid's y axis is class b mod S, tile b / S, so
// blocks whose rows are neighbours on the image are neighbours in launch order.  Staging loads
// go row by row of the region, 16 bytes per lane, consecutive lanes consecutive texels; a wave
// filters one row piece, so its ds_read_b128 cover 1 KiB of contiguous LDS (no bank conflicts)
// and its store one contiguous KiB.  Texels off the image are zeros and never count (tap's
// `inside`).
template <uint32_t S, int NP>
__global__ __launch_bounds__(256) void rt_denoise_kernel(const DenoiseParams p) {
    constexpr uint32_t RX = 64u + 4u * S, RY = 8u;
    static_assert((S & (S - 1u)) == 0u && 48u * RX * RY <= 65536u,
                  "a power of two whose region fits a workgroup's LDS");
    __shared__ float4 sa[RX * RY];
    __shared__ float4 sb[RX * RY];
    __shared__ float4 sn[RX * RY];
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
        if (X >= 0 && X < W && Y >= 0 && Y < H) t = load_texel(p, (size_t)Y * p.width + (size_t)X);
        sa[e] = t.a;
        sb[e] = t.b;
        sn[e] = t.n;
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
    const bool missP = is_miss(P.b);
    Acc acc = {0.0f, 0.0f, 0.0f, 0.0f};
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
            tap<NP>(p, P, missP, Q, row && qx >= 0 && qx < W, tap_h(dy) * tap_h(dx), acc);
        }
    }
    p.out[(size_t)y * p.width + (size_t)x] = resolve(P, acc);
}

// The direct route: no LDS, every tap loads its texel from global memory (L2 and the Infinity
// Cache hold the planes).  A wave is 64 consecutive pixels of a row, so each of a tap's loads
// is one contiguous kilobyte; a workgroup is four such rows.  A tap off the image reads the
// pixel's own texel instead and does not count.
template <int NP>
__global__ __launch_bounds__(256) void rt_denoise_direct_kernel(const DenoiseParams p) {
    const int W = (int)p.width, H = (int)p.height;
    const int s = 1 << p.shift;
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= W || y >= H) return;
    const size_t at = (size_t)y * p.width + (size_t)x;
    const Texel P = load_texel(p, at);
    const bool missP = is_miss(P.b);
    Acc acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;                  // wave-uniform: a wave is one row
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const bool inside = qx >= 0 && qx < W;
            const Texel Q = load_texel(p, inside ? (size_t)qy * p.width + (size_t)qx : at);
            tap<NP>(p, P, missP, Q, inside, tap_h(dy) * tap_h(dx), acc);
        }
    }
    p.out[at] = resolve(P, acc);
}

namespace {

template <uint32_t S>
void launch_rows(const DenoiseParams& p, hipStream_t stream) {
    // per class of rows y mod S: ceil(ceil(height / S) / 4) tiles (classes past the image exit)
    const dim3 grid((p.width + 63u) / 64u, S * (((p.height + S - 1u) / S + 3u) / 4u));
    // the default power as straight-line code, any other as a loop
    if (p.npow == 5u)
        hipLaunchKernelGGL((rt_denoise_kernel<S, 5>), grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL((rt_denoise_kernel<S, -1>), grid, dim3(256), 0, stream, p);
}

}  // namespace

hipError_t launch_denoise(const DenoiseParams& p, DenoiseRoute route, hipStream_t stream) {
    if (route == kDenoiseRows) {
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
            hipLaunchKernelGGL(rt_denoise_direct_kernel<5>, grid, dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL(rt_denoise_direct_kernel<-1>, grid, dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace rtk
