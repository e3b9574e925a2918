// rt_reproject.hip — the reprojection kernel (include/rt_reproject.h has the normative
// definition; DESIGN.md §4.8 the rationale and measurements).  A translation unit of its own:
// the render's kernels (rt_kernels.hip) are not recompiled with it.
//
// Every float operation below is the one the header names, in its order: the build has
// -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical to the
// NumPy restatement in tests/test_reproject.py.
#include <hip/hip_runtime.h>

#include "rt_reproject_kernels.h"

namespace rtk {

namespace {

constexpr uint32_t kMiss = 0xFFFFFFFFu;        // RT_AOV_MISS

__device__ __forceinline__ float dot3(const float* r, float x, float y, float z) {
    return (r[0] * x + r[1] * y) + r[2] * z;
}

}  // namespace

// One lane per pixel, no LDS.  A wave is 16 x 4 pixels and a workgroup 2 x 2 waves, so under a
// rotation or a zoom a wave's four taps stay within a few rows of the previous planes: rows of
// 16 lanes load 256 contiguous bytes of a float4 plane.  A lane that fails rules 1-4 of the
// header loads nothing more and stores zeros; a lane past the image does nothing.  Every index
// below is inside width x height.
__global__ __launch_bounds__(256) void rt_reproject_kernel(const ReprojectParams p) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * kReprojectTileW + (wave & 1u) * 16u + (lane & 15u);
    const uint32_t y = blockIdx.y * kReprojectTileH + (wave >> 1) * 4u + (lane >> 4);
    if (x >= p.width || y >= p.height) return;
    const int W = (int)p.width, H = (int)p.height;
    const size_t at = (size_t)y * p.width + (size_t)x;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t id = p.id[at];
    bool go = id != kMiss;                                            // rule 1
    if (go && p.material) go = p.material[at].w < -1.0f;              // rule 2
    if (go) {
        const float4 hp = p.hit[at];
        const float qx = hp.x - p.o[0], qy = hp.y - p.o[1], qz = hp.z - p.o[2];
        const float a = dot3(p.r0, qx, qy, qz);
        const float b = dot3(p.r1, qx, qy, qz);
        const float c = dot3(p.r2, qx, qy, qz);
        if (c > 0.0f) {                                               // rule 3
            const float px = a / c - 0.5f, py = b / c - 0.5f;
            if (px >= -1.0f && px < (float)W && py >= -1.0f && py < (float)H) {   // rule 4
                const float4 nP = p.normal[at];
                const float fx = floorf(px), fy = floorf(py);
                const float tx = px - fx, ty = py - fy;
                const int x0 = (int)fx, y0 = (int)fy;                 // -1 .. W - 1, -1 .. H - 1
                const float r2q = (qx * qx + qy * qy) + qz * qz;
                const float lim = p.tol2 * r2q;
                // The four taps' twelve loads are independent of one another and go out
                // together, one round trip instead of a dependent chain per tap: a tap off the
                // image reads the lane's own texel of the previous planes (a valid index) and
                // is dropped by ok[t].  Tap t is (i, j) = (t & 1, t >> 1).
                size_t q[4];
                bool ok[4];
                float bw[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int X = x0 + (t & 1), Y = y0 + (t >> 1);
                    bw[t] = ((t >> 1) ? ty : 1.0f - ty) * ((t & 1) ? tx : 1.0f - tx);
                    ok[t] = X >= 0 && X < W && Y >= 0 && Y < H;
                    q[t] = ok[t] ? (size_t)Y * p.width + (size_t)X : at;
                }
                uint32_t pid[4];
                float4 ph[4], pc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    pid[t] = p.prev_id[q[t]];
                    ph[t] = p.prev_hit[q[t]];
                    pc[t] = p.prev[q[t]];
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float ex = hp.x - ph[t].x, ey = hp.y - ph[t].y, ez = hp.z - ph[t].z;
                    const float dl = (nP.x * ex + nP.y * ey) + nP.z * ez;
                    ok[t] = ok[t] && pid[t] == id && dl * dl <= lim;
                }
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
                if (kept)                                             // rule 5
                    out = make_float4(sr / sw, sg / sw, sb / sw,
                                      n < p.max_history ? n : p.max_history);
            }
        }
    }
    p.dst[at] = out;
}

hipError_t launch_reproject(const ReprojectParams& p, hipStream_t stream) {
    const dim3 grid((p.width + kReprojectTileW - 1u) / kReprojectTileW,
                    (p.height + kReprojectTileH - 1u) / kReprojectTileH);
    hipLaunchKernelGGL(rt_reproject_kernel, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
