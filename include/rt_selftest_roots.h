/*
 * rt_selftest_roots.h — device self-test of the exact root selection (librt_hip.so), an
 * addition to the boundary of rt_abi.h (ABI 7): one entry point and one struct.  Plain C
 * types only.
 */
#ifndef RT_SELFTEST_ROOTS_H
#define RT_SELFTEST_ROOTS_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two fast root selections against the IEEE ones they replace, on n_random generated
 * rays and spheres (case i of the generator, i < n_random; the same cases rt_selftest_fastmath
 * counts in out[3]): family 0 = the list scan's consider_fast against consider, family 1 = the
 * bounce kernel's and the grid walk's consider_any_fast against consider_any (with and
 * without an item table, with incoming (tmax, index) pairs that tie the sphere's root).
 *
 * A case is compared when it lies in the domain the guards admit — every origin component
 * below 2^39, |C| + |R| <= 2^40 (evaluated in double, as the scene bound is), a = |d|^2 in
 * [2^-11, 2^20] — and in its stratum; radii cover the whole f32 range, half the spheres
 * graze the ray, and the incoming tmax is the scan's sentinel, a value between the two roots,
 * one below them, or the IEEE root itself (and its two neighbours).  Case i belongs to
 * stratum i mod 4:
 *   0  anywhere in the domain (magnitudes up to 2^38);
 *   1  |O| or |C| in [2^38, 2^40];
 *   2  a within one binade of an end of its range, [2^-11, 2^-10] or [2^19, 2^20] (one in
 *      sixteen exactly 2^-11 or 2^20);
 *   3  both.
 * out[family * RT_ROOTS_STRATA + stratum]: the cases drawn, those compared, those of them
 * whose discriminant was not negative (the square root and the divisions ran), and those
 * where the fast selection's (tmax, index) differed from the IEEE one's in any bit. */
#define RT_ROOTS_FAMILIES 2u
#define RT_ROOTS_STRATA 4u
typedef struct rt_roots_tally {
    uint64_t mismatches, drawn, compared, rooted;
} rt_roots_tally;
RT_API rt_status rt_selftest_roots(rt_ctx* ctx, uint64_t n_random,
                                   rt_roots_tally out[RT_ROOTS_FAMILIES * RT_ROOTS_STRATA]);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_SELFTEST_ROOTS_H */
