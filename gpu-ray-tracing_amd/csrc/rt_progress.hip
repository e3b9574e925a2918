// rt_progress.hip — the kernels of rt_progress_stats (include/rt_progress.h has the normative
// definition; DESIGN.md §4.12 the measurements).  A translation unit of its own, like
// rt_adaptive.hip: no other kernel is recompiled with it, and it traces no ray.
//
// The classification is the sampler's, through the functions the sampler's kernels call
// (rt_pixel_rules.h: gated_variance, adaptive_decide): a pixel is active here exactly when
// rt_adaptive_kernel or rt_converge_kernel would sample it.  Everything the report holds is a
// count, a sum of integers or a maximum, so no order of waves, workgroups or lanes shows in it.
//
// Two launches, no waiting inside either: rt_progress_kernel leaves one plain record per
// workgroup, rt_progress_fold_kernel (one workgroup) folds them into the report.  No atomics.
#include <hip/hip_runtime.h>

#include "rt_pixel_rules.h"
#include "rt_progress_kernels.h"

namespace rtk {

namespace {

constexpr uint32_t kWaves = 4;                   // waves of a classifying workgroup

// A float's bits as an unsigned key of the same order (-inf lowest, -0 below +0, +inf highest
// of the numbers), and back.
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_bits(uint32_t k) {
    return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k;
}
constexpr uint32_t kKeyNone = 0x007FFFFFu;       // order_key(-inf): no pixel with err < +inf

__device__ __forceinline__ bool nonfinite(float f) {
    return (__float_as_uint(f) & 0x7F800000u) == 0x7F800000u;
}

// Reductions over the 64 lanes of a wave (every lane gets the result).
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v = min(v, (uint32_t)__shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor(v, m, 64));
    return v;
}

// a <- a combined with b.
__device__ __forceinline__ void combine(ProgressRecord& a, const ProgressRecord& b) {
    for (int i = 0; i < kProgCounts; ++i) a.count[i] += b.count[i];
    a.min_count = min(a.min_count, b.min_count);
    a.max_count = max(a.max_count, b.max_count);
    a.max_error = max(a.max_error, b.max_error);
}

__device__ __forceinline__ void clear(ProgressRecord& r) {
    for (int i = 0; i < kProgCounts; ++i) r.count[i] = 0;
    r.min_count = 0xFFFFFFFFu;
    r.max_count = 0u;
    r.max_error = kKeyNone;
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0u;
}

}  // namespace

// One wave owns one 8 x 8 tile at a time: lane l is pixel (8 tx + (l & 7), 8 band + (l >> 3)) of
// tile column tx and global band `band`, which is the bit (y & 7) * 8 + (x & 7) = l of the
// tile's word (rt_progress.h).  The tiles of the band set are numbered local band rows first;
// wave g of G takes tiles g, g + G, ...
//
// A tile's texels are loaded one trip ahead, without a branch: a lane off the image loads the
// nearest texel of its tile that is on it (the same cache lines, no byte more) and `valid`
// keeps it out of every tally, and the trip past the wave's last tile loads that tile again.
// With the loads in straight-line code the classification of one tile waits for its own texels
// only, while the next tile's are in flight.  The class ballots are scalar values, their
// pop-counts scalar adds; the count's sum, minimum and maximum and the error's key stay per lane
// across the trips and meet across the lanes once, after the loop.
// kMoments: err from the moments (rt_adaptive_error's text), else the error plane's value.
struct ProgressTexels {
    float4 c;       // the accumulator's texel
    float4 m;       // the moments' texel, or the error value in .x
    bool valid;     // the lane's pixel is on the image
};

template <bool kMoments>
__device__ __forceinline__ ProgressTexels progress_fetch(const ProgressParams& p, uint32_t t,
                                                         uint32_t tiles_x, uint32_t lane) {
    const uint32_t row = t / tiles_x, tx = t - row * tiles_x;
    const uint32_t ly = lane >> 3;
    const uint32_t x = tx * 8u + (lane & 7u);
    const uint32_t y0 = (p.band_first + row * p.band_step) * 8u;          // global, < height
    // the texel loaded: (x, ly) itself, or the tile's nearest one on the image
    const uint32_t xc = min(x, p.width - 1u), lyc = min(ly, p.height - 1u - y0);
    const size_t at = (size_t)(row * 8u + lyc) * p.width + xc;           // local
    ProgressTexels f;
    f.valid = x < p.width && y0 + ly < p.height;
    f.c = p.image[at];
    if (kMoments) f.m = p.moments[at];
    else f.m = make_float4(p.error[at], 0.0f, 0.0f, 0.0f);
    return f;
}

// The per-wave tallies: `count` are wave-uniform (scalar registers), the rest per lane.
struct ProgressTally {
    uint64_t count[kProgCounts];
    uint64_t sum;
    uint32_t lo, hi, key;
};

template <bool kMoments>
__device__ __forceinline__ void progress_classify(const ProgressParams& p,
                                                  const ProgressTexels& f, uint32_t t,
                                                  uint32_t lane, ProgressTally& a) {
    const float inf = __builtin_inff();
    const float4 c = f.c;
    const bool valid = f.valid;
    const float err =
        kMoments ? gated_variance(f.m.x, f.m.y, f.m.w, c.w, p.min_history, inf) : f.m.x;
    const uint32_t n = rtd::f2u(c.w);
    const bool active = valid && adaptive_decide(c.x, c.y, c.z, n, err, p.spp, p);
    const bool capped = valid && !(n < p.spp);
    const bool below = active && n < p.min_samples;
    const uint64_t b_active = __ballot(active);
    a.count[kProgPixels] += (uint32_t)__popcll(__ballot(valid));
    a.count[kProgActive] += (uint32_t)__popcll(b_active);
    a.count[kProgConverged] += (uint32_t)__popcll(__ballot(valid && !capped && !active));
    a.count[kProgCapped] += (uint32_t)__popcll(__ballot(capped));
    a.count[kProgBelowMin] += (uint32_t)__popcll(__ballot(below));
    a.count[kProgNoHistory] += (uint32_t)__popcll(__ballot(active && !below && err == inf));
    a.count[kProgNonfinite] += (uint32_t)__popcll(
        __ballot(valid && (nonfinite(c.x) || nonfinite(c.y) || nonfinite(c.z))));
    a.count[kProgActiveTiles] += b_active != 0ull ? 1u : 0u;
    a.sum += valid ? n : 0u;
    a.lo = min(a.lo, valid ? n : 0xFFFFFFFFu);
    a.hi = max(a.hi, valid ? n : 0u);
    a.key = max(a.key, valid && err < inf ? order_key(err) : kKeyNone);
    if (p.tile_active && lane == 0u) p.tile_active[t] = b_active;
}

template <bool kMoments>
__global__ __launch_bounds__(kWaves * 64) void rt_progress_kernel(const ProgressParams p) {
    __shared__ ProgressRecord part[kWaves];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tiles = tiles_x * p.local_bands;
    const uint32_t stride = gridDim.x * kWaves;

    ProgressTally a = {};
    a.lo = 0xFFFFFFFFu;
    a.key = kKeyNone;
    uint32_t t = blockIdx.x * kWaves + wave;
    if (t < tiles) {
        // two tiles' texels in turn: f0 is classified while f1 loads, and the other way round
        ProgressTexels f0 = progress_fetch<kMoments>(p, t, tiles_x, lane), f1;
        for (;;) {
            f1 = progress_fetch<kMoments>(p, min(t + stride, tiles - 1u), tiles_x, lane);
            progress_classify<kMoments>(p, f0, t, lane, a);
            t += stride;
            if (t >= tiles) break;
            f0 = progress_fetch<kMoments>(p, min(t + stride, tiles - 1u), tiles_x, lane);
            progress_classify<kMoments>(p, f1, t, lane, a);
            t += stride;
            if (t >= tiles) break;
        }
    }
    a.count[kProgSamples] = wave_sum(a.sum);
    a.lo = wave_min(a.lo);
    a.hi = wave_max(a.hi);
    a.key = wave_max(a.key);
    if (lane == 0u) {
        ProgressRecord& r = part[wave];
        for (int i = 0; i < kProgCounts; ++i) r.count[i] = a.count[i];
        r.min_count = a.lo;
        r.max_count = a.hi;
        r.max_error = a.key;
        r.reserved[0] = r.reserved[1] = r.reserved[2] = 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        ProgressRecord r = part[0];
        for (uint32_t k = 1; k < kWaves; ++k) combine(r, part[k]);
        p.block[1u + blockIdx.x] = r;
    }
}

// One workgroup: thread i folds records i, i + 256, ..., the lanes of each wave meet, the waves
// meet through LDS, and thread 0 stores the report with the error's key decoded.  (Loading a
// thread's records in straight-line code instead of this loop changes nothing measurable: the
// launch takes what the smallest launches take here)
__global__ __launch_bounds__(kWaves * 64) void rt_progress_fold_kernel(ProgressRecord* block,
                                                                       uint32_t groups) {
    __shared__ ProgressRecord part[kWaves];
    ProgressRecord r;
    clear(r);
    for (uint32_t g = threadIdx.x; g < groups; g += kWaves * 64u) combine(r, block[1u + g]);
    for (int i = 0; i < kProgCounts; ++i) r.count[i] = wave_sum(r.count[i]);
    r.min_count = wave_min(r.min_count);
    r.max_count = wave_max(r.max_count);
    r.max_error = wave_max(r.max_error);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t k = 1; k < kWaves; ++k) combine(r, part[k]);
        r.max_error = key_bits(r.max_error);
        block[0] = r;
    }
}

hipError_t launch_progress(const ProgressParams& p, hipStream_t stream) {
    const uint32_t tiles = ((p.width + 7u) >> 3) * p.local_bands;
    const uint32_t groups = (tiles + kWaves - 1u) / kWaves;
    const uint32_t grid = groups < kProgressMaxGroups ? groups : kProgressMaxGroups;
    if (p.moments)
        hipLaunchKernelGGL(rt_progress_kernel<true>, dim3(grid), dim3(kWaves * 64u), 0, stream, p);
    else
        hipLaunchKernelGGL(rt_progress_kernel<false>, dim3(grid), dim3(kWaves * 64u), 0, stream,
                           p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rt_progress_fold_kernel, dim3(1), dim3(kWaves * 64u), 0, stream, p.block,
                       grid);
    return hipGetLastError();
}

}  // namespace rtk
