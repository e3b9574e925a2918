// rt_matte.hip — the sample-coverage ID matte kernels of rt_matte_frames and rt_matte_resolve
// (include/rt_matte.h has the normative definition; DESIGN.md §4.14 the rationale and
// measurements).  A translation unit of its own over the tracer's device library
// (rt_trace_device.h), built with the render kernels' flags: the render kernels' compile unit
// (rt_kernels.hip) does not change with it.
#include "rt_trace_device.h"

#include "rt_matte_kernels.h"

namespace rtk {

namespace {

constexpr uint32_t kMiss = 0xFFFFFFFFu;          // RT_AOV_MISS

// The single cone of footprint_beam (rt_trace_device.h, its `parent` form) for a parameter block
// other than TraceParams: the cone of every camera ray through the focus-plane rectangle of pixel
// columns [x0, x1) and rows [y0, y1), whatever the jitter, the lens point and the frame seed.  The
// construction and its margins are that form's, restated here so that the shared header stays as
// it is.
template <typename P>
__device__ __forceinline__ bool footprint_cone_of(const P& p, float x0, float x1, float y0,
                                                  float y1, Cone& k) {
    const v3 vul = mk(p.vul[0], p.vul[1], p.vul[2]), pdu = mk(p.pdu[0], p.pdu[1], p.pdu[2]),
             pdv = mk(p.pdv[0], p.pdv[1], p.pdv[2]);
    const v3 ctr = mk(p.center[0], p.center[1], p.center[2]);
    const v3 pc = fmas(0.5f * (y0 + y1), pdv, fmas(0.5f * (x0 + x1), pdu, vul));
    float rq = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const v3 q = fmas(c & 2 ? y1 : y0, pdv, fmas(c & 1 ? x1 : x0, pdu, vul));
        rq = fmaxf(rq, len3(sub(q, pc)));
    }
    float rl = 0.0f;
    if (p.defocus_angle > 0.0f) {
        const v3 du = mk(p.ddu[0], p.ddu[1], p.ddu[2]), dv = mk(p.ddv[0], p.ddv[1], p.ddv[2]);
        rl = __builtin_amdgcn_sqrtf(dot(du, du) + dot(dv, dv));
    }
    const float mag = fabsf(pc.x) + fabsf(pc.y) + fabsf(pc.z) + fabsf(ctr.x) + fabsf(ctr.y) +
                      fabsf(ctr.z);
    rq = rq * 1.001f + 1e-5f * mag;                 // f32 evaluation of pc and o = pc - d + d
    rl = rl * 1.001f + 1e-5f * mag;
    const v3 w = sub(pc, ctr);
    const float L = len3(w), delta = rq + rl;
    // (rq and rl enter the test through delta: a NaN or infinite camera value fails it)
    if (!(L > 4.0f * delta) || !__builtin_isfinite(L + mag + delta)) return false;
    k.axis = mk(w.x / L, w.y / L, w.z / L);
    k.apex = pc;
    k.sin_t = delta / (L - delta) * 1.01f;
    k.cos_t = __builtin_amdgcn_sqrtf(1.0f - k.sin_t * k.sin_t) * 0.999f;
    k.r_o = rq;
    k.d_max = (L + delta) * 1.001f;
    return true;
}

// lanes below this one in a ballot mask
__device__ __forceinline__ uint32_t prefix_of(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

}  // namespace

// ---- rt_matte_frames ------------------------------------------------------------------------
//
// One wave per 8x8 tile on tile_coord's map, four tiles of a band per workgroup, up to
// kMatteMaxFrames frames per launch with their seeds in the kernarg.  A lane loads its pixel's ten
// words once, keeps them in registers over the frames and stores them once; a lane off the image
// or the band is not live: it loads and stores nothing and takes no part in the cones' reductions.
//
// First hits.  The per-tile candidate blocks of the render carry no sphere index and belong to the
// render's camera, so they are not read.  Instead the wave builds its own index list once per
// launch: the tile's all-frames cone (footprint_cone_of: valid for every jitter, lens point and
// seed), every record tested against it with cone_misses, 64 records per step, and the survivors'
// indices compacted in index order into the wave's row of s_list (a ballot gives the mask, mbcnt
// the prefix).  A sphere the cone rejects has a negative discriminant for every camera ray of the
// tile (cone_misses' margins), so consider() would not look at it; each frame walks the list with
// the exhaustive scan's own discriminant and consider, in index order, and gets the exhaustive
// scan's winner, ties included.  The index is wave-uniform, so each record arrives through the
// scalar path, the next one fetched while the current one is tested.
//
// Capacity: 64 entries per wave, 1 KiB of LDS per workgroup — one compaction step can add up to 64
// entries and the render's own lists (19 entries at most, 2.2 on average on the bench scene) show
// that a tile's cone rarely reaches more.  A tile whose list overflows, whose cone is degenerate or
// non-finite, or whose scene is below kCullMinSpheres falls back, for the whole launch, to the
// per-frame scan_culled (which itself walks the whole list where it must); route kMatteRouteScan
// sends every tile there and kMatteRouteExhaustive to the reference's linear walk.  Control flow
// is wave-uniform down to consider()'s own lane mask.
__global__ __launch_bounds__(256) void rt_matte_kernel(const MatteParams p) {
    __shared__ uint32_t s_list[4][kMatteListCap];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tx = blockIdx.x * 4u + wave;
    if (tx >= tiles_x) return;                                    // whole wave exits
    const TileCoord tc = tile_coord(p.width, p.height, p.band_first, p.band_step, tx, blockIdx.y,
                                    lane);
    const bool live = tc.valid;
    uint4 id = make_uint4(0u, 0u, 0u, 0u), cnt = id;
    uint2 tal = make_uint2(0u, 0u);
    if (live && !p.reset_first) {                                 // wgsl:345-350: not read
        id = p.ids[tc.idx];
        cnt = p.counts[tc.idx];
        tal = p.tally[tc.idx];
    }
    const uint32_t hxy = hash(tc.x * 73u) ^ hash(tc.y * 51u);      // wgsl:309-310
    const Cam cam = cam_params(p);
    const float4* __restrict__ geom = p.geom;
    const uint32_t count = p.count;

    // the wave's list
    uint32_t* const lst = s_list[wave];
    uint32_t n_list = 0u;
    bool listed = false, overflow = false;
    if (p.route == kMatteRouteList && count >= kCullMinSpheres) {
        const float gy = (float)((p.band_first + blockIdx.y * p.band_step) * RT_STRIPE_ROWS);
        const float gx = (float)(tx * 8u);
        Cone k;
        listed = footprint_cone_of(p, gx, gx + 8.0f, gy, gy + 8.0f, k);
        for (uint32_t base = 0; listed && base < count; base += 64u) {
            const uint32_t i = base + lane;
            const float4 g = geom[i < count ? i : 0u];
            const bool keep = i < count && !cone_misses(k, g);
            const unsigned long long mask = rt_ballot(keep);
            const uint32_t c = (uint32_t)__popcll(mask);
            if (n_list + c > kMatteListCap) {                     // (uniform)
                overflow = true;
                listed = false;
                break;
            }
            if (keep) lst[n_list + prefix_of(mask)] = i;
            n_list += c;
        }
        // (the row is this wave's alone: its LDS operations complete in order, no barrier)
        __builtin_amdgcn_wave_barrier();
    }
    // entry j of the finished list in lane j: the frames read it with v_readlane at the uniform j,
    // not through LDS again
    const uint32_t mine = lst[lane];
    if (p.info && lane == 0u) {
        atomicAdd(p.info + (listed ? 0 : 1), 1u);
        if (listed) atomicMax(p.info + 2, n_list);
        if (overflow) atomicAdd(p.info + 3, 1u);
    }

    for (uint32_t f = 0; f < p.frames; ++f) {
        const uint32_t B = p.seed_b[f];
        const uint32_t seed = 1u + tal.x + B;                     // wgsl:353
        v3 o, d;
        get_ray<0>(cam, tc.x, tc.y, hxy, seed * 25u + B, o, d);    // wgsl:311
        Hit h;
        if (listed) {
            const float a = dot(d, d);                            // wgsl:184
            h.t = 0x1.05ed2ep+118f;                               // 3.4e35 (wgsl:266)
            h.idx = -1;
            if (n_list != 0u) {
                uint32_t i = __builtin_amdgcn_readlane(mine, 0);
                float4 g = load_rec<true>(geom, i);
                for (uint32_t j = 0; j < n_list; ++j) {
                    const uint32_t in =
                        __builtin_amdgcn_readlane(mine, (int)min(j + 1u, n_list - 1u));
                    const float4 gn = load_rec<true>(geom, in);
                    float hh;
                    const float disc = discriminant(g, o, d, a, hh);
                    consider(disc, hh, a, i, h.t, h.idx);
                    i = in;
                    g = gn;
                }
            }
        } else if (p.route == kMatteRouteExhaustive) {
            h = scan_exhaustive<RT_SCAN_CHUNK>(geom, count, o, d);
        } else {
            const GridP none = {};                                // (bounce rays only)
            h = scan_culled<false>(none, geom, count, o, d, live, false);
        }
        const uint32_t v = h.idx >= 0 ? (uint32_t)h.idx : kMiss;
        // the slot rule: the first slot that holds v, else the lowest empty slot, else overflow
        const bool m0 = cnt.x != 0u && id.x == v;
        const bool m1 = !m0 && cnt.y != 0u && id.y == v;
        const bool m2 = !(m0 || m1) && cnt.z != 0u && id.z == v;
        const bool m3 = !(m0 || m1 || m2) && cnt.w != 0u && id.w == v;
        const bool found = m0 || m1 || m2 || m3;
        const bool e0 = !found && cnt.x == 0u;
        const bool e1 = !found && !e0 && cnt.y == 0u;
        const bool e2 = !found && !(e0 || e1) && cnt.z == 0u;
        const bool e3 = !found && !(e0 || e1 || e2) && cnt.w == 0u;
        id.x = e0 ? v : id.x;
        id.y = e1 ? v : id.y;
        id.z = e2 ? v : id.z;
        id.w = e3 ? v : id.w;
        cnt.x += (m0 || e0) ? 1u : 0u;
        cnt.y += (m1 || e1) ? 1u : 0u;
        cnt.z += (m2 || e2) ? 1u : 0u;
        cnt.w += (m3 || e3) ? 1u : 0u;
        tal.y += (found || e0 || e1 || e2 || e3) ? 0u : 1u;
        tal.x += 1u;
    }
    if (!live) return;
    // an empty slot's id is written as 0
    id.x = cnt.x ? id.x : 0u;
    id.y = cnt.y ? id.y : 0u;
    id.z = cnt.z ? id.z : 0u;
    id.w = cnt.w ? id.w : 0u;
    p.ids[tc.idx] = id;
    p.counts[tc.idx] = cnt;
    p.tally[tc.idx] = tal;
}

hipError_t launch_matte(const MatteParams& p, uint32_t bands, hipStream_t stream) {
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    if (tiles_x == 0 || bands == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_matte_kernel, dim3((tiles_x + 3u) / 4u, bands), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// ---- rt_matte_resolve -----------------------------------------------------------------------
//
// One lane per pixel: 40 bytes read, 4 or 8 written.  The selection is a bit mask over the ids
// below mask_bits and a flag for the background.
__global__ __launch_bounds__(256) void rt_matte_resolve_kernel(const MatteResolveParams p) {
    const uint64_t at = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (at >= p.pixels) return;
    const uint4 id = p.ids[at], cnt = p.counts[at];
    const uint32_t taken = p.tally[at].x;
    const uint32_t ids[4] = {id.x, id.y, id.z, id.w}, cs[4] = {cnt.x, cnt.y, cnt.z, cnt.w};
    uint32_t s = 0u, best = 0u, dom = kMiss;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = ids[j], c = cs[j];
        bool sel = false;
        if (c != 0u) {
            if (v == kMiss)
                sel = p.background != 0u;
            else if (v < p.mask_bits)
                sel = (p.mask[v >> 5] >> (v & 31u)) & 1u;
        }
        s += sel ? c : 0u;
        if (c > best) {                                           // ties: the lowest slot
            best = c;
            dom = v;
        }
    }
    if (p.alpha) p.alpha[at] = taken ? (float)s / (float)taken : 0.0f;
    if (p.dominant) p.dominant[at] = taken ? dom : kMiss;
}

hipError_t launch_matte_resolve(const MatteResolveParams& p, hipStream_t stream) {
    if (p.pixels == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_matte_resolve_kernel, dim3((uint32_t)((p.pixels + 255u) / 256u)),
                       dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace rtk
