// rt_scene.cpp — the context's scene: the sphere upload (only when the bytes change) with the
// radius check and the bounce grid, and the scene and camera bounds of the fast cores' domain.
//   prepare_sphere_buffer (lib.rs:177-207) -> upload_spheres
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_kernels.h"

namespace rti {
namespace {

constexpr uint32_t kMaxSpheres = 1u << 20;
constexpr uint32_t kScanPad = 68;  // >= chunk round-up + one chunk + a 64-lane block

double norm3(const float* v) {
    return std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
}
double norm3d(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// Uniform XZ grid of the small spheres (rt_trace_device.h scan_grid), built on every scene
// upload of at least kGridMinSpheres spheres whose |C| + |R| stay within 2^40 (so no f32
// intermediate of the root test overflows for the rays that may use the grid).  Small:
// |R| <= 4x the median radius; the others (the ground, the few large spheres) go to the
// big list that every ray tests.  Cells are about one small sphere's worth of the centres'
// bounding area, at most kGridMaxDim per axis.  A ray may walk the grid when
// 2.5e-3 (|o - c| + reach) <= m (c, reach: centre and radius of the small spheres' extent),
// which bounds the f32 discriminant margin of every small sphere by m; each sphere is then
// registered in every cell within sqrt(R^2 + m^2) + e of its centre, e bounding the f32 error of
// the walk's cell positions: (steps + 16) x 8 eps x the largest coordinate magnitude it
// handles, plus 1e-3 of a cell.  Rays further out, with |d|^2 outside [2^-20, 2^20] or
// non-finite, keep the exhaustive scan.
constexpr uint32_t kGridMinSpheres = 64;
// small spheres' centres per cell (round 5, with the sqrt(R^2 + m^2) registration: 1.0 —
// K5 436 against 445 us per fused frame at 2.0, profiles/r05/r05ab/, r05ac/)
#ifndef RT_GRID_PER_CELL
#define RT_GRID_PER_CELL 1.0
#endif
// (A/B) round 4's registration pad, R + m
#ifndef RT_GRID_PAD_ROUND4
#define RT_GRID_PAD_ROUND4 0
#endif
// (K5 per 64-spp step with far rays sharing the walk, tools/k5_ab.py, profiles/r06/r06x/,
// r06y/: 2 / 2.5 / 3 / 3.5 / 4 reaches 18.75 / 17.82 / 17.83-17.90 / 17.97 / 18.14 ms — a wider
// reach pads every registration, a narrower one leaves more far lanes that fail the miss test)
#ifndef RT_GRID_REACHES
#define RT_GRID_REACHES 3.0
#endif
#ifndef RT_GRID_E_STEPS
#define RT_GRID_E_STEPS 1
#endif
#ifndef RT_GRID_DISK
#define RT_GRID_DISK 1
#endif
constexpr uint32_t kGridMaxDim = 256;

rt_status build_grid(rt_ctx* ctx, const rt_sphere* sp, uint32_t count, hipStream_t stream) {
    ctx->grid.nx = 0;
    if (count < kGridMinSpheres || !(ctx->scene_bound <= 0x1p40)) return RT_OK;
    std::vector<double> radii(count);
    for (uint32_t i = 0; i < count; ++i) radii[i] = std::fabs((double)sp[i].radius);
    std::vector<double> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + count / 2, sorted.end());
    const double r_small = 4.0 * sorted[count / 2];
    std::vector<uint32_t> small, big;
    for (uint32_t i = 0; i < count; ++i) (radii[i] <= r_small ? small : big).push_back(i);
    if (small.size() < kGridMinSpheres / 2) return RT_OK;
    // extent of the small spheres: centre c (mid-point of the bounding box) and reach
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double rmax = 0.0;
    for (uint32_t i : small) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], (double)sp[i].position[k]);
            hi[k] = std::max(hi[k], (double)sp[i].position[k]);
        }
        rmax = std::max(rmax, radii[i]);
    }
    double c[3], g_r = 0.0;
    for (int k = 0; k < 3; ++k) c[k] = (double)(float)(0.5 * (lo[k] + hi[k]));
    for (uint32_t i : small) {
        double v[3];
        for (int k = 0; k < 3; ++k) v[k] = (double)sp[i].position[k] - c[k];
        g_r = std::max(g_r, norm3d(v));
    }
    const double reach = (g_r + rmax) * 1.001;
    // rays up to RT_GRID_REACHES - 1 reaches from the centre may use the grid
    const double m = 2.5e-3 * RT_GRID_REACHES * reach * 1.001 + 1e-30;
    const double area = std::max(hi[0] - lo[0], 1e-30) * std::max(hi[2] - lo[2], 1e-30);
    double s = std::sqrt(area * RT_GRID_PER_CELL / (double)small.size());
    s = std::max({s, (hi[0] - lo[0]) / (kGridMaxDim - 8), (hi[2] - lo[2]) / (kGridMaxDim - 8),
                  2.0 * rmax / 8.0, 1e-6});
    const double L = norm3d(c) + m / 2.5e-3 + 2.0 * reach + 4.0 * s;
    // e for walks of up to 2 kGridMaxDim steps; re-derived below from the grid's own step
    // bound nx + nz + 2 (RT_GRID_E_STEPS)
    double e = (2.0 * kGridMaxDim + 16.0) * 8.0 * 0x1p-24 * L + 1e-3 * s;
    // A ray that may use the grid accepts sphere (C, R) only at a point within
    // sqrt(R^2 + m^2) of C, plus the root's own rounding (< 1e-5 L): the computed
    // discriminant is negative beyond (the bound E <= m^2 of the culled scan).
    // Round 4 padded by R + m, up to m more (2.40 -> 1.98 registrations per small sphere of
    // the K5 scene).
    auto reg_w = [&](double r) {
        const double rr = r * 1.0001;
#if RT_GRID_PAD_ROUND4
        return rr + m + e;
#else
        return std::sqrt(rr * rr + m * m) + e + 1e-5 * L;
#endif
    };
    double x0, x1, z0, z1, ylo, yhi;
    uint32_t nx = 0, nz = 0;
    s = (double)(float)s;
    auto box = [&]() {
        x0 = INFINITY, x1 = -INFINITY, z0 = INFINITY, z1 = -INFINITY;
        ylo = INFINITY, yhi = -INFINITY;
        for (uint32_t i : small) {
            const double w = reg_w(radii[i]);
            x0 = std::min(x0, sp[i].position[0] - w);
            x1 = std::max(x1, sp[i].position[0] + w);
            z0 = std::min(z0, sp[i].position[2] - w);
            z1 = std::max(z1, sp[i].position[2] + w);
            ylo = std::min(ylo, sp[i].position[1] - w);
            yhi = std::max(yhi, sp[i].position[1] + w);
        }
        x0 = (double)(float)x0 - e;
        z0 = (double)(float)z0 - e;
        const double fx = std::ceil((x1 + e - x0) / s), fz = std::ceil((z1 + e - z0) / s);
        nx = fx >= 1.0 && fx <= kGridMaxDim ? (uint32_t)fx : 0u;
        nz = fz >= 1.0 && fz <= kGridMaxDim ? (uint32_t)fz : 0u;
    };
    box();
    if (nx < 1 || nz < 1) return RT_OK;
#if RT_GRID_E_STEPS
    // A walk takes at most nx + nz + 2 steps of this grid; e for that many is smaller, and
    // the box it gives lies inside this one (nx, nz do not grow), so it still bounds the
    // walks of the final grid (K5: 0.019 -> 0.003, 12 % fewer registrations).
    e = ((double)nx + (double)nz + 2.0 + 16.0) * 8.0 * 0x1p-24 * L + 1e-3 * s;
    box();
    if (nx < 1 || nz < 1) return RT_OK;
#endif
    // CSR: count, prefix, fill (small spheres in index order within every cell)
    const uint32_t cells = nx * nz;
    std::vector<uint32_t> start(cells + 1, 0u);
    auto span = [&](uint32_t i, uint32_t& ax, uint32_t& bx, uint32_t& az, uint32_t& bz) {
        const double w = reg_w(radii[i]);
        auto cell = [&](double v, double o, uint32_t n) {
            const double f = std::floor((v - o) / s);
            return (uint32_t)std::min(std::max(f, 0.0), (double)(n - 1));
        };
        ax = cell(sp[i].position[0] - w, x0, nx);
        bx = cell(sp[i].position[0] + w, x0, nx);
        az = cell(sp[i].position[2] - w, z0, nz);
        bz = cell(sp[i].position[2] + w, z0, nz);
    };
    // Of the square of cells, only those that meet the disk of radius w around the centre
    // (in XZ) can hold a point where the sphere is accepted, so only they list it (a walk
    // that passes such a point passes through the cell that contains it).  Widened by 1e-6
    // of a cell for the float rounding of the cell origin the kernel uses (RT_GRID_DISK).
    auto touches = [&](uint32_t i, uint32_t x, uint32_t z) {
#if RT_GRID_DISK
        const double w = reg_w(radii[i]) + 1e-6 * s;
        const double cx = sp[i].position[0], cz = sp[i].position[2];
        const double lx = x0 + s * x, hx = lx + s, lz = z0 + s * z, hz = lz + s;
        const double dx = std::max({lx - cx, cx - hx, 0.0});
        const double dz = std::max({lz - cz, cz - hz, 0.0});
        return dx * dx + dz * dz <= w * w;
#else
        (void)i, (void)x, (void)z;
        return true;
#endif
    };
    for (uint32_t i : small) {
        uint32_t ax, bx, az, bz;
        span(i, ax, bx, az, bz);
        for (uint32_t z = az; z <= bz; ++z)
            for (uint32_t x = ax; x <= bx; ++x)
                if (touches(i, x, z)) start[z * nx + x + 1]++;
    }
    for (uint32_t k = 0; k < cells; ++k) start[k + 1] += start[k];
    const uint32_t items = start[cells];
    // one buffer: cells x uint2, items x float4, items x u32, big x u32
    const size_t geom_off = ((size_t)cells * 8 + 15) & ~(size_t)15;   // float4-aligned
    const size_t idx_off = geom_off + (size_t)items * 16;
    const size_t big_off = idx_off + (size_t)items * 4;
    std::vector<unsigned char> buf(big_off + big.size() * 4 + 16);
    uint2* rng = reinterpret_cast<uint2*>(buf.data());
    float4* gg = reinterpret_cast<float4*>(buf.data() + geom_off);
    uint32_t* gi = reinterpret_cast<uint32_t*>(buf.data() + idx_off);
    for (uint32_t k = 0; k < cells; ++k) rng[k] = make_uint2(start[k], start[k + 1]);
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (uint32_t i : small) {
        uint32_t ax, bx, az, bz;
        span(i, ax, bx, az, bz);
        const float4 rec = make_float4(sp[i].position[0], sp[i].position[1], sp[i].position[2],
                                       sp[i].radius * sp[i].radius);   // as upload_spheres
        for (uint32_t z = az; z <= bz; ++z)
            for (uint32_t x = ax; x <= bx; ++x) {
                if (!touches(i, x, z)) continue;
                const uint32_t k = fill[z * nx + x]++;
                gg[k] = rec;
                gi[k] = i;
            }
    }
    std::memcpy(buf.data() + big_off, big.data(), big.size() * 4);
    // The previous grid may still be read by queued launches: order on the stream.
    hipError_t err = hipStreamSynchronize(stream);
    if (err != hipSuccess) return hip_fail(err, "hipStreamSynchronize");
    (void)hipFree(ctx->d_grid);
    ctx->d_grid = nullptr;
    err = hipMalloc(&ctx->d_grid, buf.size());
    if (err != hipSuccess) return hip_fail(err, "hipMalloc(sphere grid)");
    err = hipMemcpyAsync(ctx->d_grid, buf.data(), buf.size(), hipMemcpyHostToDevice, stream);
    if (err == hipSuccess) err = hipStreamSynchronize(stream);
    if (err != hipSuccess) return hip_fail(err, "hipMemcpyAsync(sphere grid)");
    rt_ctx::Grid& g = ctx->grid;
    g.nx = nx;
    g.nz = nz;
    g.nbig = (uint32_t)big.size();
    g.items = items;
    g.x0 = (float)x0;
    g.z0 = (float)z0;
    g.s = (float)s;
    g.inv_s = (float)(1.0 / s);
    g.ylo = (float)(ylo - e);
    g.yhi = (float)(yhi + e);
    g.cx = (float)c[0];
    g.cy = (float)c[1];
    g.cz = (float)c[2];
    g.reach = (float)reach;
    g.m = (float)m;
    g.e = (float)e;
    return RT_OK;
}

}  // namespace

// Whether every camera ray of p's camera, image and stripes, against the context's scene,
// stays inside the domain where the camera-ray-only instances use the exact fast division
// and sqrt cores (rt_trace_device.h consider_fast / fast_core): a = |d|^2 in [2^-11, 2^20],
// |O| + max(|C| + |R|) <= 2^40 (so |h|, sqrt(D) <= 2^53 and the hit-point numerators of
// the normal <= 2^43), and every |R| in [2^-20, 2^20].  d = pc - O (get_ray,
// wgsl:305-325) with pc = vul + sx pdu + sy pdv, sx in [0, W + 8], sy in [0, H + 8] (lanes
// past a ragged edge included), and O = center, or center + (cos, sin) (ddu, ddv) with a
// unit (cos, sin) when defocus_angle > 0.  |d| is bounded above by the sum of the parts and
// below by the distance along the normal of the pixel-delta plane, each widened by
// 1e-5 x the magnitudes entering the f32 evaluation (its rounding is < 1e-6 of them).
// Cameras or scenes outside the domain (degenerate, huge, non-finite, zero radii) run the
// IEEE operations in the culled instance instead.  Evaluated in double; NaN fails.
bool camera_rays_bounded(const rt_ctx* ctx, const rtk::TraceParams& p) {
    if (!ctx->radii_ok) return false;
    const bool defocus = p.defocus_angle > 0.0f;
    const double W = (double)p.width + 8.0, H = (double)p.height + 8.0;
    double e[3], nrm[3];
    for (int i = 0; i < 3; ++i) e[i] = (double)p.vul[i] - p.center[i];
    nrm[0] = (double)p.pdu[1] * p.pdv[2] - (double)p.pdu[2] * p.pdv[1];
    nrm[1] = (double)p.pdu[2] * p.pdv[0] - (double)p.pdu[0] * p.pdv[2];
    nrm[2] = (double)p.pdu[0] * p.pdv[1] - (double)p.pdu[1] * p.pdv[0];
    const double nn = std::sqrt(nrm[0] * nrm[0] + nrm[1] * nrm[1] + nrm[2] * nrm[2]);
    if (!(nn > 0.0) || !std::isfinite(nn)) return false;
    auto along = [&](const double* v) {
        return std::fabs(v[0] * nrm[0] + v[1] * nrm[1] + v[2] * nrm[2]) / nn;
    };
    double du[3], dv[3];
    for (int i = 0; i < 3; ++i) {
        du[i] = defocus ? p.ddu[i] : 0.0;
        dv[i] = defocus ? p.ddv[i] : 0.0;
    }
    const double lens = std::sqrt(du[0] * du[0] + du[1] * du[1] + du[2] * du[2]) +
                        std::sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    const double span = W * norm3(p.pdu) + H * norm3(p.pdv);
    const double mag = norm3(p.vul) + norm3(p.center) + span + lens;
    const double dmax = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + span + lens +
                        1e-5 * mag;
    const double dmin = along(e) - along(du) - along(dv) - 1e-5 * mag;
    if (!(dmin > 0.0 && dmin * dmin >= 0x1p-11 && dmax * dmax <= 0x1p20)) return false;
    const double origin = norm3(p.center) + lens * (1.0 + 1e-5);
    return origin + ctx->scene_bound <= 0x1p40;
}

rt_status upload_spheres(rt_ctx* ctx, const rt_sphere* spheres, uint32_t count,
                         hipStream_t stream) {
    if (count > kMaxSpheres) return fail(RT_ERR_INVALID_SIZE, "sphere_count too large");
    if (count > 0 && spheres == nullptr)
        return fail(RT_ERR_INVALID_ARGUMENT, "spheres is NULL with sphere_count > 0");
    if (ctx->valid && count == ctx->count &&
        (count == 0 || std::memcmp(ctx->cached.data(), spheres, count * sizeof(rt_sphere)) == 0))
        return RT_OK;  // unchanged since the last upload
    // From here the device copy no longer matches `cached`: a failure below leaves the
    // context invalid (the next call uploads again) and retires every scene-derived cache
    // (candidate lists, tile costs) by bumping the generation.
    ctx->valid = false;
    ctx->normal_rn = false;
    ctx->scene_gen++;
    if (count > ctx->capacity || ctx->d_geom == nullptr) {
        uint32_t cap = ctx->capacity ? ctx->capacity : 64u;
        while (cap < count) cap *= 2u;
        float4 *g = nullptr, *s = nullptr;
        // kScanPad zero records after the list: the scan prefetches one chunk ahead.
        const size_t geom_bytes = ((size_t)cap + kScanPad) * sizeof(float4);
        hipError_t e = hipMalloc(&g, geom_bytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(sphere geometry)");
        e = hipMemsetAsync(g, 0, geom_bytes, stream);
        if (e != hipSuccess) {
            (void)hipFree(g);
            return hip_fail(e, "hipMemsetAsync(sphere geometry)");
        }
        e = hipMalloc(&s, (size_t)cap * 2 * sizeof(float4));
        if (e != hipSuccess) {
            (void)hipFree(g);
            return hip_fail(e, "hipMalloc(sphere records)");
        }
        // The previous buffers may still be read by queued launches on `stream`.
        if (ctx->d_geom || ctx->d_sph) {
            e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
            (void)hipFree(ctx->d_geom);
            (void)hipFree(ctx->d_sph);
        }
        ctx->d_geom = g;
        ctx->d_sph = s;
        ctx->capacity = cap;
    }
    if (count > 0) {
        // Scan record: center + radius^2.  r*r is one IEEE f32 multiply, bit-identical to
        // the shader's `sphere.radius * sphere.radius` (wgsl:186).
        std::vector<float4> geom(count);
        for (uint32_t i = 0; i < count; ++i) {
            const rt_sphere& s = spheres[i];
            geom[i] = make_float4(s.position[0], s.position[1], s.position[2],
                                  s.radius * s.radius);
        }
        // Queued launches may still read the old scene: order the copies on the stream,
        // and wait for them so the host staging vectors can be released.
        hipError_t e = hipMemcpyAsync(ctx->d_geom, geom.data(), geom.size() * sizeof(float4),
                                      hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(sphere geometry)");
        // the sphere records as the reference uploads them (bytemuck, lib.rs:186)
        e = hipMemcpyAsync(ctx->d_sph, spheres, count * sizeof(rt_sphere),
                           hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(sphere records)");
        // the hit normal's one-step division by each distinct radius, checked on the device
        // against the IEEE division for every numerator significand (2^24 divisions per
        // radius); scenes with more than kRcpRadii distinct radii keep the two-step form.
        // (RT_NORMAL_RN=0 in the environment turns the Markstein normal off: a test switch)
        constexpr size_t kRcpRadii = 16;
        std::vector<float> radii(count);
        for (uint32_t i = 0; i < count; ++i) radii[i] = spheres[i].radius;
        std::sort(radii.begin(), radii.end(), [](float a, float b) {
            uint32_t x, y;
            std::memcpy(&x, &a, 4);
            std::memcpy(&y, &b, 4);
            return x < y;
        });
        radii.erase(std::unique(radii.begin(), radii.end(), [](float a, float b) {
                        return std::memcmp(&a, &b, 4) == 0;
                    }), radii.end());
        uint32_t bad = 1u;
        if (radii.size() <= kRcpRadii) {
            if (!ctx->d_flag) {
                e = hipMalloc(&ctx->d_flag, sizeof(uint32_t) * (1 + kRcpRadii));
                if (e != hipSuccess) return hip_fail(e, "hipMalloc(check flag)");
            }
            float* d_radii = reinterpret_cast<float*>(ctx->d_flag + 1);
            e = hipMemsetAsync(ctx->d_flag, 0, sizeof(uint32_t), stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(d_radii, radii.data(), radii.size() * sizeof(float),
                                   hipMemcpyHostToDevice, stream);
            if (e == hipSuccess)
                e = rtk::launch_rcp_check(d_radii, (uint32_t)radii.size(), ctx->d_flag, stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(&bad, ctx->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   stream);
            if (e != hipSuccess) return hip_fail(e, "radius reciprocal check");
        }
        e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        const char* env = std::getenv("RT_NORMAL_RN");
        ctx->normal_rn = bad == 0u && !(env && env[0] == '0');
    }
    double bound = 0.0;
    bool radii_ok = true;
    for (uint32_t i = 0; i < count; ++i) {
        const double r = std::fabs((double)spheres[i].radius);
        const double b = norm3(spheres[i].position) + r;
        bound = std::isfinite(b) ? std::max(bound, b) : INFINITY;
        radii_ok = radii_ok && r >= 0x1p-20 && r <= 0x1p20;
    }
    ctx->scene_bound = bound;
    ctx->radii_ok = radii_ok;
    if (rt_status s = build_grid(ctx, spheres, count, stream)) return s;
    ctx->cached.assign(spheres, spheres + count);
    ctx->count = count;
    ctx->valid = true;
    return RT_OK;
}

}  // namespace rti
