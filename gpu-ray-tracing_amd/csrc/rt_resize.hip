// rt_resize.hip — the resize-carry kernel (include/rt_resize.h has the normative definition;
// DESIGN.md §4.16 the rationale and measurements).  A translation unit of its own: neither the
// render's kernels (rt_kernels.hip) nor rt_reproject.hip are recompiled with it.
//
// Every float operation below is the one the header names, in its order: the build has
// -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical to the
// NumPy restatement in tests/test_resize.py, and at equal sizes with sky and fill off to
// rt_reproject_kernel's.
#include <hip/hip_runtime.h>

#include "rt_resize_kernels.h"

namespace rtk {

namespace {

constexpr uint32_t kMiss = 0xFFFFFFFFu;        // RT_AOV_MISS

__device__ __forceinline__ float dot3(const float* r, float x, float y, float z) {
    return (r[0] * x + r[1] * y) + r[2] * z;
}

// Rules 5 and 6 of the header for one image pair: the kept taps' mean and capped count, or the
// nearest texel `near` of the four (alpha 0) for a hole under fill, or zeros.
__device__ __forceinline__ float4 carry(const float4 (&pc)[4], const bool (&ok)[4],
                                        const float (&bw)[4], int near, bool fill,
                                        float max_history) {
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    float n = __builtin_inff();
    bool kept = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!ok[t] || !(pc[t].w > 0.0f) || !(bw[t] > 0.0f)) continue;
        sw = sw + bw[t];
        sr = sr + bw[t] * pc[t].x;
        sg = sg + bw[t] * pc[t].y;
        sb = sb + bw[t] * pc[t].z;
        n = pc[t].w < n ? pc[t].w : n;
        kept = true;
    }
    if (kept) return make_float4(sr / sw, sg / sw, sb / sw, n < max_history ? n : max_history);
    if (!fill) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // (selects, not an indexed array: no scratch)
    const float4 lo = (near & 1) ? pc[1] : pc[0], hi = (near & 1) ? pc[3] : pc[2];
    const float4 c = (near & 2) ? hi : lo;
    return make_float4(c.x, c.y, c.z, 0.0f);
}

}  // namespace

// rt_reproject_kernel's shape: one lane per pixel of the current image, no LDS, a wave 16 x 4
// pixels and a workgroup 2 x 2 waves.  A lane that fails rule 2 or 4 of the header loads nothing
// more and stores zeros; a lane past the image does nothing.  Every index into a current plane
// is inside width x height and every index into a previous plane inside prev_width x
// prev_height: the taps' coordinates are clamped to the previous image, so a tap off it reads
// the nearest texel on it and is dropped by ok[t], and the texel rule 6 names is always one of
// the four clamped taps (floorf(px + 0.5f) is x0 or x0 + 1), so the fill needs no load of its
// own.  Second: the second image pair is carried too (four more loads, one more store).
template <bool Second>
__global__ __launch_bounds__(256) void rt_resize_carry_kernel(const ResizeParams p) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * kResizeTileW + (wave & 1u) * 16u + (lane & 15u);
    const uint32_t y = blockIdx.y * kResizeTileH + (wave >> 1) * 4u + (lane >> 4);
    if (x >= p.width || y >= p.height) return;
    const int PW = (int)p.prev_width, PH = (int)p.prev_height;
    const size_t at = (size_t)y * p.width + (size_t)x;
    const bool fill = p.fill != 0u;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f), out2 = out;
    const uint32_t id = p.id[at];
    const bool surface = id != kMiss;
    bool eligible = p.sky != 0u;                                      // rule 1
    if (surface) eligible = p.material ? p.material[at].w < -1.0f : true;
    if (eligible || fill) {                                           // rule 2
        float4 hp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float qx, qy, qz;                                             // rule 3
        if (surface) {
            hp = p.hit[at];
            qx = hp.x - p.o[0], qy = hp.y - p.o[1], qz = hp.z - p.o[2];
        } else {
            const float sx = (float)x + 0.5f, sy = (float)y + 0.5f;
            qx = fmaf(sy, p.pdv[0], fmaf(sx, p.pdu[0], p.vul[0])) - p.center[0];
            qy = fmaf(sy, p.pdv[1], fmaf(sx, p.pdu[1], p.vul[1])) - p.center[1];
            qz = fmaf(sy, p.pdv[2], fmaf(sx, p.pdu[2], p.vul[2])) - p.center[2];
        }
        const float a = dot3(p.r0, qx, qy, qz);
        const float b = dot3(p.r1, qx, qy, qz);
        const float c = dot3(p.r2, qx, qy, qz);
        if (c > 0.0f) {                                               // rule 4
            const float px = a / c - 0.5f, py = b / c - 0.5f;
            if (px >= -1.0f && px < (float)PW && py >= -1.0f && py < (float)PH) {
                const float fx = floorf(px), fy = floorf(py);
                const float tx = px - fx, ty = py - fy;
                const int x0 = (int)fx, y0 = (int)fy;                 // -1 .. PW - 1, -1 .. PH - 1
                // the tap nearest (px, py): 0 or 1 past (x0, y0) each way
                const int near = ((int)floorf(px + 0.5f) - x0) | (((int)floorf(py + 0.5f) - y0) << 1);
                // The taps' loads are independent of one another and go out together, as in
                // rt_reproject_kernel.  Tap t is (i, j) = (t & 1, t >> 1).
                size_t q[4];
                bool ok[4];
                float bw[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int X = x0 + (t & 1), Y = y0 + (t >> 1);
                    bw[t] = ((t >> 1) ? ty : 1.0f - ty) * ((t & 1) ? tx : 1.0f - tx);
                    ok[t] = eligible && X >= 0 && X < PW && Y >= 0 && Y < PH;
                    const int Xc = X < 0 ? 0 : (X < PW ? X : PW - 1);
                    const int Yc = Y < 0 ? 0 : (Y < PH ? Y : PH - 1);
                    q[t] = (size_t)Yc * p.prev_width + (size_t)Xc;
                }
                float4 pc[4], pc2[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    pc[t] = p.prev[q[t]];
                    if (Second) pc2[t] = p.prev2[q[t]];
                }
                if (eligible) {
                    uint32_t pid[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) pid[t] = p.prev_id[q[t]];
                    if (surface) {
                        float4 ph[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) ph[t] = p.prev_hit[q[t]];
                        const float4 nP = p.normal[at];
                        const float r2q = (qx * qx + qy * qy) + qz * qz;
                        const float lim = p.tol2 * r2q;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const float ex = hp.x - ph[t].x, ey = hp.y - ph[t].y,
                                        ez = hp.z - ph[t].z;
                            const float dl = (nP.x * ex + nP.y * ey) + nP.z * ez;
                            ok[t] = ok[t] && pid[t] == id && dl * dl <= lim;
                        }
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) ok[t] = ok[t] && pid[t] == kMiss;
                    }
                }
                out = carry(pc, ok, bw, near, fill, p.max_history);   // rules 5, 6
                if (Second) out2 = carry(pc2, ok, bw, near, fill, p.max_history);   // rule 7
            }
        }
    }
    p.dst[at] = out;
    if (Second) p.dst2[at] = out2;
}

hipError_t launch_resize_carry(const ResizeParams& p, hipStream_t stream) {
    const dim3 grid((p.width + kResizeTileW - 1u) / kResizeTileW,
                    (p.height + kResizeTileH - 1u) / kResizeTileH);
    if (p.prev2)
        hipLaunchKernelGGL(rt_resize_carry_kernel<true>, grid, dim3(256), 0, stream, p);
    else
        hipLaunchKernelGGL(rt_resize_carry_kernel<false>, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
