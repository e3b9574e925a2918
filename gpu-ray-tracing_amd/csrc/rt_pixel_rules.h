// rt_pixel_rules.h — the per-pixel rules of the sampling features, each stated once.
//
// include/rt_variance.h, include/rt_adaptive.h and include/rt_converge.h are normative about
// the order of the float operations; the builds have -ffp-contract=off, IEEE division and
// subnormals on, so a kernel that applies a rule through the function below has the bits of the
// NumPy restatements in tests/.  Used by rt_adaptive.hip (the error), rt_variance.hip (the
// moments and the filter's input variance) and rt_sampler.hip (the sampler and its fused
// rounds, which apply all of them).
//
// These share expressions only: which texels a kernel loads, what it stores and how it
// branches stays with the kernel.  The functions take and return scalars (or v3) rather than
// texels and parameter blocks by value: with those the compiler's code for the callers is
// instruction for instruction what it was with the expressions written out
// (tools/kernel_isa_diff.py, profiles/tu_split/isa_diff.txt), which a float4 copied into a
// helper did not give.  Three things stay at the call sites for that reason:
//   - rule 2's sample in rt_moments_update_kernel (rt_variance.hip) is written out there:
//     through recover_sample the compiler turns the kernel's `k0 == 0` branch after it into
//     selects (two more VGPRs).  rt_converge_kernel, whose rules are selects already, calls it;
//   - the start of a frame in rt_adaptive_kernel and rt_converge_kernel (the reset of
//     wgsl:345-350, the texel's colour and u32 count of wgsl:339-341, the `valid` lane flag):
//     adaptive_decide is the decision proper, for a texel that is not reset;
//   - the variance of the mean has no function of its own beside gated_variance: the history
//     gate sits between the clamps and the division, as in the kernels before.
#pragma once

#include <hip/hip_runtime.h>

#include "rt_device.h"

namespace rtk {

// Rec. 709 luminance, left to right (rt_variance.h: L(c)).
__device__ __forceinline__ float luminance(float x, float y, float z) {
    return (0.2126f * x + 0.7152f * y) + 0.0722f * z;
}

// Variance of the mean from the moments (m1, m2, 0, k) and the accumulator's count n
// (rt_adaptive.h, rt_variance.h v0): max(m2 - m1^2, 0) / max(n, 1) with a history of at least
// min_history samples, `otherwise` without one (+inf for the error of rt_adaptive_error, the
// caller's fallback for the filter's input variance).
__device__ __forceinline__ float gated_variance(float m1, float m2, float k, float n,
                                                float min_history, float otherwise) {
    float d = m2 - m1 * m1;
    d = d > 0.0f ? d : 0.0f;
    const float nn = n > 1.0f ? n : 1.0f;
    return k >= min_history ? d / nn : otherwise;
}

// rt_update_adaptive's decision for a texel that is not reset: colour (x, y, z), count n,
// error estimate err.  Does the pixel take a sample?  a: AdaptiveParams or ConvergeParams
// (min_samples and the squared tolerances; read here, where the kernels read them).
template <typename A>
__device__ __forceinline__ bool adaptive_decide(float x, float y, float z, uint32_t n, float err,
                                                uint32_t spp, const A& a) {
    const float lm = luminance(x, y, z);
    const float thr = a.abs_tolerance2 + a.rel_tolerance2 * (lm * lm);
    const bool converged = n >= a.min_samples && err <= thr;      // (a NaN: not converged)
    return n < spp && !converged;
}

// The running mean after sample col, the (n + 1)-th: the reference's IEEE division (wgsl:356).
__device__ __forceinline__ rtd::v3 accumulate(rtd::v3 c, rtd::v3 col, uint32_t n) {
    const float k = (float)(n + 1u);                              // wgsl:356
    return rtd::mk(c.x + (col.x - c.x) / k, c.y + (col.y - c.y) / k, c.z + (col.z - c.z) / k);
}

// rt_variance.h rule 2, per channel: the sample that took the texel's channel from i to o when
// the count became w, i + w (o - i).
__device__ __forceinline__ float recover_sample(float i, float o, float w) {
    return i + w * (o - i);
}

// rt_variance.h rules 1 and 2: the moments (m1, m2) of k0 samples after one more of luminance L.
__device__ __forceinline__ float4 moments_push(float m1, float m2, float k0, float L) {
    const float kk = k0 + 1.0f;
    return make_float4(m1 + (L - m1) / kk, m2 + (L * L - m2) / kk, 0.0f, kk);
}

}  // namespace rtk
