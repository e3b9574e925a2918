// rt_edit.hip — the scene-edit carry kernel (include/rt_scene_edit.h has the normative
// definition; DESIGN.md §4.13 the rationale and measurements).  A translation unit of its own:
// neither the render's kernels (rt_kernels.hip) nor rt_reproject.hip are recompiled with it.
// The tap walk restates rt_reproject_kernel's instead of sharing it through a header, so that
// kernel's compile unit and instruction stream stay what they were.
//
// Every float operation below is the one the header names, in its order: the build has
// -ffp-contract=off, IEEE division and subnormals on, so the output is bit-identical to the
// NumPy restatement in tests/test_scene_edit.py.
#include <hip/hip_runtime.h>

#include "rt_edit_kernels.h"

namespace rtk {

namespace {

constexpr uint32_t kMiss = 0xFFFFFFFFu;        // RT_AOV_MISS
constexpr uint32_t kNone = 0xFFFFFFFFu;        // RT_EDIT_NONE
constexpr uint32_t kMoved = 0x80000000u;       // RT_EDIT_MOVED

__device__ __forceinline__ float dot3(const float* r, float x, float y, float z) {
    return (r[0] * x + r[1] * y) + r[2] * z;
}

}  // namespace

// rt_reproject_kernel's mapping and load discipline: one lane per pixel, no LDS, a wave 16 x 4
// pixels and a workgroup 2 x 2 waves.  A lane that an early rule stops loads nothing more and
// stores zeros; a lane past the image does nothing.  Every image index below is inside
// width x height, and the record is read only for id < n_records.
//
// The plan holds two float4 per entry.  A lane gathers its sphere's record (32 bytes) by id; its
// material texel is independent of it and goes out with it.  The balls are read at a
// wave-uniform index from a table nothing in the kernel writes before the final store, so they
// arrive through the scalar cache, one 32-byte scalar load per ball and wave, and the test
// against them is VALU work alone.
__global__ __launch_bounds__(256) void rt_edit_carry_kernel(const EditParams p,
                                                            const float4* __restrict__ plan) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * kEditTileW + (wave & 1u) * 16u + (lane & 15u);
    const uint32_t y = blockIdx.y * kEditTileH + (wave >> 1) * 4u + (lane >> 4);
    if (x >= p.width || y >= p.height) return;
    const int W = (int)p.width, H = (int)p.height;
    const size_t at = (size_t)y * p.width + (size_t)x;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const uint32_t id = p.id[at];
    if (id != kMiss && id < p.n_records) {                            // rule 1, rule 1b's guard
        const float4 ra = plan[2u * (size_t)id];                      // prev_center, scale
        const float4 rb = plan[2u * (size_t)id + 1u];                 // center, link
        const uint32_t link = __float_as_uint(rb.w);
        bool go = link != kNone;                                      // rule 1b
        if (p.material) go = p.material[at].w < -1.0f && go;          // rule 2
        if (go) {
            const float4 hp = p.hit[at];
            bool near = false;
            const float4* balls = plan + 2u * (size_t)p.n_records;
            // (no short circuit: the trip count stays uniform and four balls' loads go out
            // together)
#pragma unroll 4
            for (uint32_t k = 0; k < p.n_balls; ++k) {
                const float4 ba = balls[2u * (size_t)k];              // center, radius2
                const uint32_t owner = __float_as_uint(balls[2u * (size_t)k + 1u].x);
                const float dx = hp.x - ba.x, dy = hp.y - ba.y, dz = hp.z - ba.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                near |= (owner != id) & (d2 < ba.w);
            }
            const float cap = near ? p.edit_history : p.max_history;
            if (cap > 0.0f) {                                         // rule 2b (max_history >= 1)
                float sx = hp.x, sy = hp.y, sz = hp.z;                // p'
                if (link & kMoved) {
                    sx = ra.x + (hp.x - rb.x) * ra.w;
                    sy = ra.y + (hp.y - rb.y) * ra.w;
                    sz = ra.z + (hp.z - rb.z) * ra.w;
                }
                const uint32_t from = link & ~kMoved;
                const float qx = sx - p.o[0], qy = sy - p.o[1], qz = sz - p.o[2];
                const float a = dot3(p.r0, qx, qy, qz);
                const float b = dot3(p.r1, qx, qy, qz);
                const float c = dot3(p.r2, qx, qy, qz);
                if (c > 0.0f) {                                       // rule 3
                    const float px = a / c - 0.5f, py = b / c - 0.5f;
                    if (px >= -1.0f && px < (float)W && py >= -1.0f && py < (float)H) {  // rule 4
                        const float4 nP = p.normal[at];
                        const float fx = floorf(px), fy = floorf(py);
                        const float tx = px - fx, ty = py - fy;
                        const int x0 = (int)fx, y0 = (int)fy;         // -1 .. W - 1, -1 .. H - 1
                        const float r2q = (qx * qx + qy * qy) + qz * qz;
                        const float lim = p.tol2 * r2q;
                        // The four taps' twelve loads go out together; a tap off the image reads
                        // the lane's own texel of the previous planes (a valid index) and is
                        // dropped by ok[t].  Tap t is (i, j) = (t & 1, t >> 1).
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
                            const float ex = sx - ph[t].x, ey = sy - ph[t].y, ez = sz - ph[t].z;
                            const float dl = (nP.x * ex + nP.y * ey) + nP.z * ez;
                            ok[t] = ok[t] && pid[t] == from && dl * dl <= lim;
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
                        if (kept)                                     // rule 5
                            out = make_float4(sr / sw, sg / sw, sb / sw, n < cap ? n : cap);
                    }
                }
            }
        }
    }
    p.dst[at] = out;
}

hipError_t launch_edit_carry(const EditParams& p, const float4* plan, hipStream_t stream) {
    const dim3 grid((p.width + kEditTileW - 1u) / kEditTileW,
                    (p.height + kEditTileH - 1u) / kEditTileH);
    hipLaunchKernelGGL(rt_edit_carry_kernel, grid, dim3(256), 0, stream, p, plan);
    return hipGetLastError();
}

}  // namespace rtk
