// rt_sampler.hip — the adaptive sampler's kernels: rt_update_adaptive (include/rt_adaptive.h)
// and its fused multi-frame rounds, rt_converge_frames (include/rt_converge.h).  Both trace
// with sample<kScan> and ray_color of the tracer's device library (rt_trace_device.h) as they
// are, and state the per-pixel rules through rt_pixel_rules.h.  A translation unit of its own,
// built with the render kernels' flags (kernel-argument preload included): the render kernels'
// compile unit (rt_kernels.hip) does not change with it.  rt_adaptive_error's kernel is in
// rt_adaptive.hip, which is built without the preload.
#include "rt_pixel_rules.h"
#include "rt_trace_device.h"

namespace rtk {

// ---- Adaptive sampling (rt_adaptive.h) -----------------------------------------------
//
// One `update` in which only the pixels whose error estimate is still above the tolerance
// take a sample.  One wave per 8x8 tile on rt_trace_kernel's stripe map (tile_coord), four
// tiles of a band per workgroup.  The wave loads its accumulator texels and error values,
// decides per lane (rt_adaptive.h: the reset, min_samples, the tolerance, the spp cap), forms
// the tile's mask with one ballot and lane 0 stores the word.  A wave whose ballot is empty
// writes its texels back as they pass through and ends: it reads no candidate list, hash table
// or sphere record.  Any other wave traces one sample with the mask as the per-lane `live` flag
// — trace_pixel's mechanism for n < spp — through sample<kScan> and ray_color as they are,
// without a sample-count hint (uni = false: the counts differ per pixel), and accumulates with
// the reference's IEEE division (wgsl:356), so a sampled texel has rt_update's bits.
// kScan: kTraceExhaustive, kTraceList (depth <= 1, camera in the proven domain: the fast
// cores) or kTraceCulled (candidate lists for camera rays, cone / grid culling for bounce rays
// in ray_color; no LDS copy of the records: TraceParams::lds_records is 0 here).
template <int kScan>
__global__ __launch_bounds__(256, RT_TRACE_MIN_WAVES) void rt_adaptive_kernel(
    const TraceParams p, const AdaptiveParams a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tx = blockIdx.x * 4u + wave;
    if (tx >= tiles_x) return;                                    // whole wave exits
    const uint32_t lband = blockIdx.y;
    const TileCoord tc = tile_coord(p, tx, lband, lane);
    const uint32_t tile = lband * tiles_x + tx;
    // (a lane off the image reads texel 0 of the local buffers and stores nothing)
    const size_t at = tc.valid ? tc.idx : 0;
    const float4 I = p.in[at];
    const float err = a.error[at];
    const uint32_t spp = p.spp;                                   // wgsl:343
    v3 c = mk(0.0f, 0.0f, 0.0f);
    uint32_t n = 0u;
    bool sampled = 0u < spp;                                      // a reset: wgsl:345-350
    if (!p.reset_first) {
        c = mk(I.x, I.y, I.z);                                    // wgsl:339-341
        n = f2u(I.w);
        sampled = adaptive_decide(I.x, I.y, I.z, n, err, spp, a);
    }
    sampled = sampled && tc.valid;
    const uint64_t m = rt_ballot(sampled);
    if (a.tile_mask && lane == 0u) a.tile_mask[tile] = m;
    if (m != 0ull) {
        const uint32_t ncand =
            (kScan != kTraceExhaustive && p.cand) ? load_cnt(p.cand, tile) : kCandNone;
        const uint32_t hxy =
            p.hx[min(tc.x, p.width - 1u)] ^ p.hy[min(tc.y, p.height - 1u)];
        const Cam cam = cam_params(p);
        const v3 col = sample<kScan>(p, cam, tile, ncand, tc, hxy, n, p.seed_b[0], 0u, sampled,
                                     false);
        if (sampled) {
            c = accumulate(c, col, n);                            // wgsl:356
            n += 1u;
        }
    }
    // wgsl:362-363; a texel that passes through is what spp = 0 would write: u32(alpha) again
    if (tc.valid) p.out[tc.idx] = make_float4(c.x, c.y, c.z, (float)n);
}

hipError_t launch_adaptive(const TraceParams& p, const AdaptiveParams& a, int kernel,
                           hipStream_t stream) {
    const dim3 grid = tile_grid(p);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    if (kernel == kTraceList)
        hipLaunchKernelGGL(rt_adaptive_kernel<kTraceList>, grid, dim3(256), 0, stream, p, a);
    else if (kernel == kTraceCulled)
        hipLaunchKernelGGL(rt_adaptive_kernel<kTraceCulled>, grid, dim3(256), 0, stream, p, a);
    else if (kernel == kTraceExhaustive)
        hipLaunchKernelGGL(rt_adaptive_kernel<kTraceExhaustive>, grid, dim3(256), 0, stream, p,
                           a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- Fused adaptive rounds (rt_converge.h) ---------------------------------------------
//
// p.frames rounds of rt_adaptive_error, rt_update_adaptive and rt_moments_update over one tile
// in one launch, beside rt_adaptive_kernel for that kernel's reason (sample<kScan> and
// ray_color as they are) and on its grid: one wave per 8x8 tile, four tiles of a band per
// workgroup.  The wave loads its accumulator and moments texels once, keeps both in registers
// over the frames and stores them once, in place (p.out; nothing reads a tile's texels during
// the launch but its own wave).  Each frame, in f32 and in the headers' order of operations:
// the error from the moments and the count (rt_adaptive.h), the decision and its ballot, one
// sample with the ballot's lanes live when it is not empty (seed_b[f]; no hint), the IEEE
// division of wgsl:356, and rt_variance.h's four rules on the texel before and after the frame.
// Control flow is wave-uniform (ballots); the per-lane rules are selects.
//
// Early exit: a frame that is not a reset, in which no lane was sampled and
// which left every on-image lane's accumulator and moments texels bit-identical to what it
// read, is a fixed point: every later frame reads the same state, decides the same (only the
// seed differs, and no idle lane reads it) and writes the same.  The wave leaves the loop
// there.  "No lane sampled" alone would not do: a count of 7.5 passes through as 7, rule 4 then
// zeroes the moments, the error becomes +inf and the pixel is sampled in the next frame.
// A wave none of whose frames changed a bit stores no texel.
// The culled instance holds eight more live registers than rt_adaptive_kernel's across ray_color's
// culled scans: planned for RT_TRACE_MIN_WAVES it spills to scratch (44 bytes per lane), so it is
// planned for 6 waves per SIMD (74 VGPRs, no scratch); the other two fit as they are.
template <int kScan>
constexpr int converge_min_waves() {
    return kScan == kTraceCulled ? 6 : RT_TRACE_MIN_WAVES;
}
template <int kScan>
__global__ __launch_bounds__(256, converge_min_waves<kScan>()) void rt_converge_kernel(
    const TraceParams p, const ConvergeParams a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tx = blockIdx.x * 4u + wave;
    if (tx >= tiles_x) return;                                    // whole wave exits
    const uint32_t lband = blockIdx.y;
    const TileCoord tc = tile_coord(p, tx, lband, lane);
    const uint32_t tile = lband * tiles_x + tx;
    // (a lane off the image holds zeros, is never sampled and stores nothing)
    float4 I = make_float4(0.0f, 0.0f, 0.0f, 0.0f), M = I;
    if (tc.valid) {
        I = p.out[tc.idx];
        M = a.moments[tc.idx];
    }
    const uint32_t spp = p.spp;                                   // wgsl:343
    uint32_t ncand = kCandNone, hxy = 0u;
    bool scene_read = false;                // the tile's list and seed hashes: on first use
    bool dirty = false;                     // some frame changed a bit of the tile
    uint64_t m = 0ull;
    uint32_t taken = 0u;
    for (uint32_t f = 0; f < p.frames; ++f) {
        const bool reset = f == 0u && p.reset_first != 0u;
        // rt_adaptive_error
        const float err = gated_variance(M.x, M.y, M.w, I.w, a.min_history, __builtin_inff());
        // rt_update_adaptive
        v3 c = mk(0.0f, 0.0f, 0.0f);
        uint32_t n = 0u;
        bool sampled = 0u < spp;                                  // a reset: wgsl:345-350
        if (!reset) {
            c = mk(I.x, I.y, I.z);                                // wgsl:339-341
            n = f2u(I.w);
            sampled = adaptive_decide(I.x, I.y, I.z, n, err, spp, a);
        }
        sampled = sampled && tc.valid;
        m = rt_ballot(sampled);
        if (m != 0ull) {
            if (!scene_read) {
                ncand = (kScan != kTraceExhaustive && p.cand) ? load_cnt(p.cand, tile)
                                                              : kCandNone;
                hxy = p.hx[min(tc.x, p.width - 1u)] ^ p.hy[min(tc.y, p.height - 1u)];
                scene_read = true;
            }
            const Cam cam = cam_params(p);
            const v3 col = sample<kScan>(p, cam, tile, ncand, tc, hxy, n, p.seed_b[f], f, sampled,
                                         false);
            if (sampled) {
                c = accumulate(c, col, n);                        // wgsl:356
                n += 1u;
            }
            taken += (uint32_t)__popcll(m);
        }
        const float4 O = make_float4(c.x, c.y, c.z, (float)n);    // wgsl:362-363
        // rt_moments_update on (I, O): rules 1 and 2 share the running means' step, rule 3 keeps
        // M and rule 4 zeroes it
        const bool r1 = O.w == 1.0f;
        const bool r2 = !r1 && O.w == I.w + 1.0f;
        float4 N = M;
        if (!(r1 || r2) && !(O.w == I.w)) N = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (rt_ballot(r1 || r2) != 0ull) {
            const float sx = r1 ? O.x : recover_sample(I.x, O.x, O.w);
            const float sy = r1 ? O.y : recover_sample(I.y, O.y, O.w);
            const float sz = r1 ? O.z : recover_sample(I.z, O.z, O.w);
            const float k0 = r1 ? 0.0f : M.w;
            const bool fresh = k0 == 0.0f;
            const float m1 = fresh ? 0.0f : M.x, m2 = fresh ? 0.0f : M.y;
            const float4 S = moments_push(m1, m2, k0, luminance(sx, sy, sz));
            if (r1 || r2) N = S;
        }
        const bool changed =
            tc.valid &&
            (((__float_as_uint(O.x) ^ __float_as_uint(I.x)) |
              (__float_as_uint(O.y) ^ __float_as_uint(I.y)) |
              (__float_as_uint(O.z) ^ __float_as_uint(I.z)) |
              (__float_as_uint(O.w) ^ __float_as_uint(I.w)) |
              (__float_as_uint(N.x) ^ __float_as_uint(M.x)) |
              (__float_as_uint(N.y) ^ __float_as_uint(M.y)) |
              (__float_as_uint(N.z) ^ __float_as_uint(M.z)) |
              (__float_as_uint(N.w) ^ __float_as_uint(M.w))) != 0u);
        const bool any_changed = rt_ballot(changed) != 0ull;
        I = O;
        M = N;
        dirty = dirty || any_changed;
        if (!any_changed && m == 0ull && !reset) break;           // a fixed point: see above
    }
    // (after an early exit m is 0: the frames left out sample nothing)
    if (lane == 0u) {
        if (a.tile_mask) a.tile_mask[tile] = m;
        if (a.tile_samples) {
            if (a.first)
                a.tile_samples[tile] = taken;
            else if (taken != 0u)
                a.tile_samples[tile] += taken;
        }
    }
    // a later launch of the call that changes nothing finds the plane its predecessor wrote
    if (!tc.valid || !(dirty || a.first)) return;
    if (dirty) {
        p.out[tc.idx] = I;
        a.moments[tc.idx] = M;
    }
    if (a.error)
        a.error[tc.idx] = gated_variance(M.x, M.y, M.w, I.w, a.min_history, __builtin_inff());
}

hipError_t launch_converge(const TraceParams& p, const ConvergeParams& a, int kernel,
                           hipStream_t stream) {
    const dim3 grid = tile_grid(p);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    if (kernel == kTraceList)
        hipLaunchKernelGGL(rt_converge_kernel<kTraceList>, grid, dim3(256), 0, stream, p, a);
    else if (kernel == kTraceCulled)
        hipLaunchKernelGGL(rt_converge_kernel<kTraceCulled>, grid, dim3(256), 0, stream, p, a);
    else if (kernel == kTraceExhaustive)
        hipLaunchKernelGGL(rt_converge_kernel<kTraceExhaustive>, grid, dim3(256), 0, stream, p,
                           a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace rtk
