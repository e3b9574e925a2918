// rt_atrous.h — the device skeleton the edge-avoiding a-trous filters share (rt_denoise.hip,
// rt_variance.hip): the two routes' geometry and tap walks and their launcher,
// written once.  Internal, for those two translation units only.
//
// A filter is a policy struct F:
//   Params             the kernel's argument: width, height, shift (log2 of the tap spacing),
//                      npow, and what load and Pixel read
//   Texel              what a tap needs of a pixel
//   Lds<N>             N texels as LDS plane arrays, with put(e, t) and get(e)
//   load(p, idx), zero()   a texel from global memory; the texel of a pixel off the image
//   kPrefilter         whether a 3 x 3 walk at the iteration's spacing precedes the 5 x 5 one;
//                      if so Lds<N>::local(e) and load_local(p, idx) read what that walk needs
//   Pixel<NP>(p, P)    the filter of pixel P: tap(Q, inside, k) per 5 x 5 tap, dy outer, dx
//                      inner (`inside`: Q is on the image; Q is any readable texel otherwise),
//                      then resolve(at), which stores; with kPrefilter local(q, inside, k) per
//                      3 x 3 tap and local_done() before the first tap.  NP: normal_power_log2
//                      at compile time, or -1 for the parameter's
//   rows<S, NP>, direct<NP>   the __global__ wrappers of rows<F, S, NP> and direct<F, NP>
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "rt_atrous_route.h"

namespace rtk {
namespace atrous {

__device__ __forceinline__ bool is_miss(float t) {
    return !(t < __builtin_inff());
}

// h (x) h, h = (1/16, 1/4, 3/8, 1/4, 1/16), and h3 (x) h3, h3 = (1/4, 1/2, 1/4): every
// product is exact
__device__ __forceinline__ constexpr float tap_h(int d) {
    return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f;
}
__device__ __forceinline__ constexpr float tap_h3(int d) {
    return d == 0 ? 0.5f : 0.25f;
}

// max(dn, 0) squared NP times in line, or npow times for NP = -1 (a wave-uniform loop)
template <int NP>
__device__ __forceinline__ float normal_weight(float dn, uint32_t npow) {
    float wn = dn > 0.0f ? dn : 0.0f;                     // max(dn, 0), NaN -> 0
    if (NP >= 0) {
#pragma unroll
        for (int r = 0; r < NP; ++r) wn = wn * wn;
    } else {
        for (uint32_t r = 0; r < npow; ++r) wn = wn * wn;
    }
    return wn;
}

// The LDS route ("rows"), for a step S up to 16.  A workgroup of 256 threads filters 64 x 4
// pixels: 64 consecutive pixels x0 + i of the four rows y0 + S * j, rows of one residue class
// y mod S, for which the filter's vertical taps are the neighbouring rows of the class.  It
// first stages the RX x 8 texels (x0 - 2 S + u, y0 + S * (v - 2)), RX = 64 + 4 S — a halo of 2 S
// pixels along x, of 2 class rows along y — as F's planes: sizeof(Lds<8 RX>) = (512 + 32 S)
// times the planes' bytes per texel (48 and 52: 26 112 and 28 288 bytes for S = 1, 49 152 and
// 53 248 for S = 16).  Tap (dx, dy) of a pixel is then (S dx, dy) texels away in LDS, the
// prefilter's taps among them.  Block b of the grid's y axis is class b mod S, tile b / S, so
// blocks whose rows are neighbours on the image are neighbours in launch order.  Staging loads
// go row by row of the region, 16 bytes per lane, consecutive lanes consecutive texels; a wave
// filters one row piece, so its ds_read_b128 cover 1 KiB of contiguous LDS (no bank conflicts)
// and its store one contiguous KiB.  Texels off the image are zeros and never count (`inside`).
template <class F, uint32_t S, int NP>
__device__ __forceinline__ void rows(const typename F::Params& p) {
    constexpr uint32_t RX = 64u + 4u * S, RY = 8u;
    using Lds = typename F::template Lds<RX * RY>;
    static_assert((S & (S - 1u)) == 0u && sizeof(Lds) <= 65536u,
                  "a power of two whose region fits a workgroup's LDS");
    __shared__ Lds lds;
    const int W = (int)p.width, H = (int)p.height;
    constexpr int s = (int)S;
    const int x0 = (int)(64u * blockIdx.x);
    const int y0 = (int)(blockIdx.y & (S - 1u)) + s * (int)(4u * (blockIdx.y >> p.shift));
    if (y0 >= H) return;                                  // the whole workgroup: a short class
    for (uint32_t e = threadIdx.x; e < RX * RY; e += 256u) {
        const uint32_t v = e / RX, u = e - v * RX;
        const int X = x0 + (int)u - 2 * s;
        const int Y = y0 + s * ((int)v - 2);
        typename F::Texel t = F::zero();
        if (X >= 0 && X < W && Y >= 0 && Y < H) t = F::load(p, (size_t)Y * p.width + (size_t)X);
        lds.put(e, t);
    }
    __syncthreads();
    const uint32_t i = threadIdx.x & 63u, j = threadIdx.x >> 6;
    const int x = x0 + (int)i, y = y0 + s * (int)j;
    if (x >= W || y >= H) return;
    const int ctr = (int)((j + 2u) * RX + i + 2u * S);
    typename F::template Pixel<NP> px(p, lds.get(ctr));
    if constexpr (F::kPrefilter) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy * s;
            const bool row = qy >= 0 && qy < H;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx * s;
                px.local(lds.local(ctr + dy * (int)RX + dx * s), row && qx >= 0 && qx < W,
                         tap_h3(dy) * tap_h3(dx));
            }
        }
        px.local_done();
    }
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        const bool row = qy >= 0 && qy < H;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const int q = ctr + dy * (int)RX + dx * s;    // always inside the region
            px.tap(lds.get(q), row && qx >= 0 && qx < W, tap_h(dy) * tap_h(dx));
        }
    }
    px.resolve((size_t)y * p.width + (size_t)x);
}

// The direct route: no LDS, every tap loads its texel from global memory (L2 and the Infinity
// Cache hold the planes).  A wave is 64 consecutive pixels of a row, so each of a tap's loads
// is one contiguous kilobyte; a workgroup is four such rows.  A tap off the image reads the
// pixel's own texel instead and does not count.
template <class F, int NP>
__device__ __forceinline__ void direct(const typename F::Params& p) {
    const int W = (int)p.width, H = (int)p.height;
    const int s = 1 << p.shift;
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u));
    const int y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= W || y >= H) return;
    const size_t at = (size_t)y * p.width + (size_t)x;
    typename F::template Pixel<NP> px(p, F::load(p, at));
    if constexpr (F::kPrefilter) {
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy * s;
            if (qy < 0 || qy >= H) continue;              // wave-uniform: a wave is one row
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx * s;
                const bool inside = qx >= 0 && qx < W;
                px.local(F::load_local(p, inside ? (size_t)qy * p.width + (size_t)qx : at),
                         inside, tap_h3(dy) * tap_h3(dx));
            }
        }
        px.local_done();
    }
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
        if (qy < 0 || qy >= H) continue;                  // wave-uniform: a wave is one row
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            const bool inside = qx >= 0 && qx < W;
            px.tap(F::load(p, inside ? (size_t)qy * p.width + (size_t)qx : at), inside,
                   tap_h(dy) * tap_h(dx));
        }
    }
    px.resolve(at);
}

// One iteration of filter F on `route`; the default power as straight-line code, any other as
// a loop.
template <class F>
hipError_t launch(const typename F::Params& p, AtrousRoute route, hipStream_t stream) {
    const uint32_t cols = (p.width + 63u) / 64u;
    const bool np5 = p.npow == 5u;
    const auto rows_step = [&](auto step) {
        constexpr uint32_t S = decltype(step)::value;
        // per class of rows y mod S: ceil(ceil(height / S) / 4) tiles (classes past the image exit)
        const dim3 grid(cols, S * (((p.height + S - 1u) / S + 3u) / 4u));
        hipLaunchKernelGGL((np5 ? F::template rows<S, 5> : F::template rows<S, -1>), grid,
                           dim3(256), 0, stream, p);
    };
    if (route == kAtrousRows) {
        switch (p.shift) {
            case 0: rows_step(std::integral_constant<uint32_t, 1>{}); break;
            case 1: rows_step(std::integral_constant<uint32_t, 2>{}); break;
            case 2: rows_step(std::integral_constant<uint32_t, 4>{}); break;
            case 3: rows_step(std::integral_constant<uint32_t, 8>{}); break;
            case 4: rows_step(std::integral_constant<uint32_t, 16>{}); break;
            default: return hipErrorInvalidValue;
        }
    } else {
        const dim3 grid(cols, (p.height + 3u) / 4u);
        hipLaunchKernelGGL((np5 ? F::template direct<5> : F::template direct<-1>), grid,
                           dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace atrous
}  // namespace rtk
