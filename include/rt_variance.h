/*
 * rt_variance.h — per-pixel luminance moments and the variance-guided a-trous filter
 * (librt_hip.so), an addition to the boundary of rt_abi.h (ABI 7): three entry points and one
 * struct.  Plain C types only.  Together with rt_reproject.h and rt_aov.h they make an
 * SVGF-style filter: a moments image has the accumulator's layout, and rt_reproject carries it
 * across a camera move as it stands.
 *
 * The filter's entry points are named rt_variance_filter*, not after rt_denoise: the library's
 * symbols that contain "denoise" are exactly those of rt_denoise.h.
 */
#ifndef RT_VARIANCE_H
#define RT_VARIANCE_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* All of the text below is in f32: every *, + and - is its own IEEE operation (no
 * contraction), / is correctly rounded, subnormals are kept.  Every output bit equals a CPU
 * restatement of this text (tests/test_variance.py).
 *   L(c) = (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z
 *
 * ---- rt_moments_update ------------------------------------------------------------------------
 * `in_rgba` and `out_rgba` are the input and the output of one update (rt_update, or the two
 * images an rt_update_frames call leaves behind); `moments` is a device RGBA32F image
 * (m1, m2, 0, k) of the same size, read and rewritten in place: m1 and m2 are the running means
 * of the luminance and of its square over the samples recovered so far, k their number.  k is a
 * count of its own: after a fused call of `frames` frames the accumulator's count has advanced
 * by `frames` and k, on the next rt_moments_update of two consecutive images, by one.
 *
 * Per pixel, I = in, O = out, M = moments, the first rule that matches:
 *   1. O.a == 1 (a first sample, or a reset):  s = O.rgb, k0 = 0; I and M are not used.
 *   2. O.a == I.a + 1:  s.c = I.c + O.a * (O.c - I.c) per channel, k0 = M.a.
 *   3. O.a == I.a (no sample was taken: the cap on samples per pixel):  M stays, bit for bit.
 *   4. anything else (NaN counts among them) is no consecutive pair:  M = (0, 0, 0, 0).
 * After rules 1 and 2, with (m1, m2) = (M.x, M.y), or (0, 0) when k0 == 0:
 *   kk = k0 + 1
 *   M  = (m1 + (L(s) - m1) / kk,  m2 + (L(s) * L(s) - m2) / kk,  0,  kk)
 *
 * ---- rt_variance_filter -----------------------------------------------------------------------
 * rt_denoise.h's filter with a luminance term scaled by each pixel's own variance in place of
 * the colour term, taps weighted by their sample counts, and the variance filtered along.
 * Iteration i = 0 .. iterations - 1 filters with tap spacing s = 1 << i; its inputs are the
 * image c (`src` for i = 0, the previous iteration's output after that) and the plane v (v0 for
 * i = 0, the previous iteration's variance output after that).  With
 *   miss(X) = !(hit[X].w < +inf)
 *   same(Q) = Q is on the image, miss(P) == miss(Q), and id[P] == id[Q] when sphere_id is given
 *   il = inv_sigma_luminance2,  ip = inv_sigma_position2
 *
 * Initial variance, per pixel X with n = src[X].a, (m1, m2, _, k) = moments[X]:
 *   d     = m2 - m1 * m1,  d = d when d > 0, else 0 (NaN -> 0)
 *   nn    = n when n > 1, else 1 (NaN -> 1)
 *   v0[X] = d / nn when k >= (float)min_history, else fallback_variance (a restarted pixel's
 *           few samples say nothing about its variance; NaN k: the fallback).
 *
 * Local variance of pixel P = (x, y): over Q = (x + dx * s, y + dy * s), dy = -1 .. 1 outer and
 * dx = -1 .. 1 inner, g = h3[dy + 1] * h3[dx + 1], h3 = (1/4, 1/2, 1/4), the taps with same(Q)
 * (the centre always is one) accumulate in this order: sg += g, sgv += g * v[Q].  Then
 *   vt = sgv / sg,  ve = vt + 1e-8f
 *
 * The 25 taps Q = (x + dx * s, y + dy * s), dy = -2 .. 2 outer and dx = -2 .. 2 inner, with
 * k = h[dy + 2] * h[dx + 2], h = (1/16, 1/4, 3/8, 1/4, 1/16):  a tap is skipped when !same(Q)
 * and when its weight w fails w > 0 (zero, NaN).  The weight:
 *   dl = L(c[P]) - L(c[Q])
 *   dp, dn, wn as in rt_denoise.h (dp = 0 and wn = 1 when miss(P))
 *   w  = (((k * wn) * c[Q].a) * ve) / ((1 + dp * ip) * (ve + (dl * dl) * il))
 * c[Q].a is the tap's sample count: a 17-sample neighbour counts for more than a 1-sample one,
 * and a 0-sample pixel (rt_reproject hands those over) counts for nothing and is filled by its
 * neighbours.  Kept taps accumulate in tap order:
 *   sw += w,  sum.c += w * c[Q].c for c in rgb,  sv += (w * w) * v[Q]
 * Then
 *   out.rgb  = sum.rgb / sw per channel when sw > 0, else c[P].rgb bit for bit
 *   out.a    = c[P].a
 *   v_out[P] = sv / (sw * sw) when sw * sw > 0, else v[P] bit for bit (a 0-sample pixel whose
 *              only neighbours of its surface have weights near 1e-30 keeps its variance: their
 *              squares underflow, and 0 / 0 would make a NaN that later iterations spread).
 * A variance that is not finite (it takes moments that are not) makes the weights of the pixels
 * whose 3 x 3 holds it NaN: they pass through, colour and variance.
 * There is no 4^i growth of a sigma: the variance shrinks as the iterations proceed.
 */
#define RT_VARIANCE_MAX_ITERATIONS 8u
typedef struct rt_variance_filter_params {
    uint32_t iterations;          /* 1..8; iteration i filters with tap spacing 1 << i          */
    uint32_t normal_power_log2;   /* 0..10; the normal weight is squared this many times        */
    float    inv_sigma_luminance2;/* >= 0, finite: 1 / sigma_l^2, in units of the variance      */
    float    inv_sigma_position2; /* >= 0, finite: 1 / sigma_p^2                                */
    uint32_t min_history;         /* 1..16777216: moments with fewer samples use the fallback   */
    float    fallback_variance;   /* >= 0, finite: v0 of such a pixel                           */
} rt_variance_filter_params;
/* iterations 5, normal_power_log2 5, inv_sigma_luminance2 1.0f, inv_sigma_position2 4.0f,
 * min_history 4, fallback_variance 1.0f */
RT_API void rt_variance_filter_params_default(rt_variance_filter_params* p);

/* One kernel launch on `stream`, one lane per pixel.  `in_rgba` and `out_rgba` are only read.
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: in_rgba, out_rgba or moments
 * NULL; any two of the three equal.  RT_ERR_INVALID_SIZE: width or height outside 1..65536.
 * A refused call launches nothing.
 *
 * Like the calls of rt_aov.h it touches no render state: candidate lists, tile orders, the
 * images' known sample counts, rt_last_launch_info and the timing events stay as they were. */
RT_API rt_status rt_moments_update(rt_ctx* ctx, const float* in_rgba, const float* out_rgba,
                                   float* moments, uint32_t width, uint32_t height,
                                   void* stream);

/* Filters the width x height RGBA32F device image `src` into `dst`, one kernel launch per
 * iteration on `stream` (v0 is computed by iteration 0 as it reads `moments`).  `src`,
 * `moments` and the guide planes (as in rt_denoise) are only read; `sphere_id` is optional.
 * `dst` receives the last iteration's image and `variance`, width * height floats and
 * required, the variance of its luminance, whatever the parity of `iterations`; `scratch`, an
 * image, and `variance_scratch`, width * height floats, hold the iterations in between and are
 * needed only when iterations >= 2 (NULL otherwise is fine).
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: src, dst, moments, variance,
 * hit, normal or params NULL; dst equal to src or moments; variance equal to src, dst or
 * moments; with iterations >= 2, scratch NULL or equal to src, dst, moments or variance, or
 * variance_scratch NULL or equal to src, dst, scratch, moments or variance; iterations,
 * normal_power_log2 or min_history out of range; a sigma term or fallback_variance negative,
 * NaN or infinite.  RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused call
 * launches nothing.
 *
 * It touches no render state, in the words above. */
RT_API rt_status rt_variance_filter(rt_ctx* ctx, const float* src, float* dst, float* scratch,
                                    const float* moments, float* variance,
                                    float* variance_scratch, uint32_t width, uint32_t height,
                                    const float* hit, const float* normal,
                                    const uint32_t* sphere_id,
                                    const rt_variance_filter_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_VARIANCE_H */
