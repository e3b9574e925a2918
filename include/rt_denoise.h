/*
 * rt_denoise.h — edge-avoiding a-trous denoiser guided by the first-hit G-buffer of rt_aov.h
 * (librt_hip.so), an addition to the boundary of rt_abi.h (ABI 7): two entry points and one
 * struct.  Plain C types only.
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The filter, all in f32: every * and + is its own IEEE operation (no contraction), / is
 * correctly rounded, subnormals are kept.  Every output bit equals a CPU restatement of this
 * text (tests/test_denoise.py).
 *
 * Iteration i = 0 .. iterations - 1 filters with tap spacing s = 1 << i; its input c is `src`
 * for i = 0 and the previous iteration's output after that.
 *   ic_i = min(inv_sigma_color2 * 4^i, FLT_MAX)   (the product is exact or +inf)
 *   ip   = inv_sigma_position2
 * For pixel P = (x, y) the taps are Q = (x + dx * s, y + dy * s), dy = -2 .. 2 outer and
 * dx = -2 .. 2 inner.  A tap off the image is skipped (not clamped).  With
 *   k       = h[dy + 2] * h[dx + 2],  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *   miss(X) = !(hit[X].w < +inf)
 * a tap is also skipped when miss(P) != miss(Q), when sphere_id is given and id[P] != id[Q],
 * and when its weight w fails w > 0 (zero, NaN: non-finite pixels, overflowed distances,
 * opposed normals).  The weight:
 *   e  = c[P].rgb - c[Q].rgb,   dc = (e.x * e.x + e.y * e.y) + e.z * e.z
 *   dp = the same expression on hit[.].xyz, 0 when miss(P)
 *   dn = (nP.x * nQ.x + nP.y * nQ.y) + nP.z * nQ.z
 *   wn = max(dn, 0) with NaN -> 0, then wn = wn * wn normal_power_log2 times; 1 when miss(P)
 *   w  = (k * wn) / ((1 + dp * ip) * (1 + dc * ic_i))
 * Kept taps accumulate in tap order: sw += w, sum.c += w * c[Q].c for c in rgb.  Then
 *   out.rgb = sum.rgb / sw per channel when sw > 0, else c[P].rgb bit for bit (a NaN or Inf
 *             pixel passes through and reaches no neighbour)
 *   out.a   = c[P].a (the sample count).
 */
#define RT_DENOISE_MAX_ITERATIONS 8u
typedef struct rt_denoise_params {
    uint32_t iterations;         /* 1..8; iteration i filters with tap spacing 1 << i           */
    uint32_t normal_power_log2;  /* 0..10; the normal weight is squared this many times         */
    float    inv_sigma_color2;   /* >= 0, finite: 1 / sigma_c^2 of iteration 0                  */
    float    inv_sigma_position2;/* >= 0, finite: 1 / sigma_p^2                                 */
} rt_denoise_params;
/* iterations 5, normal_power_log2 5, inv_sigma_color2 1.0f, inv_sigma_position2 4.0f */
RT_API void rt_denoise_params_default(rt_denoise_params* p);

/* Filters the width x height RGBA32F device image `src` (the accumulator's layout) into `dst`,
 * one kernel launch per iteration on `stream`.  `hit` and `normal` are the planes rt_trace_aov
 * writes for the same image and are required; `sphere_id` is optional (NULL: no id test).
 * `src` and the guide planes are only read.  `dst` receives the last iteration whatever the
 * parity of `iterations`; `scratch`, a third image of the same size, holds the iterations in
 * between and is needed only when iterations >= 2 (NULL otherwise is fine).
 *
 * RT_ERR_INVALID_CONTEXT: ctx NULL.  RT_ERR_INVALID_ARGUMENT: src, dst, hit, normal or params
 * NULL; dst == src; with iterations >= 2, scratch NULL or equal to src or dst; iterations or
 * normal_power_log2 out of range; a sigma term negative, NaN or infinite.
 * RT_ERR_INVALID_SIZE: width or height outside 1..65536.  A refused call launches nothing.
 *
 * Like the calls of rt_aov.h it touches no render state: candidate lists, tile orders, the
 * images' known sample counts, rt_last_launch_info and the timing events stay as they were. */
RT_API rt_status rt_denoise(rt_ctx* ctx, const float* src, float* dst, float* scratch,
                            uint32_t width, uint32_t height,
                            const float* hit, const float* normal, const uint32_t* sphere_id,
                            const rt_denoise_params* params, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_DENOISE_H */
