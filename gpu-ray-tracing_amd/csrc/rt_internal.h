// rt_internal.h — what the C-ABI translation units of librt_hip.so share: the context
// (rt_context.h), the error and argument helpers, and what each unit exports to the others.
//   rt_abi.cpp      errors, argument checks, create / destroy, setters, diagnostics, bands, present
//   rt_scene.cpp    scene upload, bounce grid, the fast cores' domain
//   rt_plan.cpp     kernel choice, candidate lists, orders, count records and hints, prepare
//   rt_frames.cpp   rt_update_frames and the render calls: fork / join, AQL glue, chain schedule
//   rt_tracers.cpp  the trace launches beside the render: G-buffer, pick, adaptive, converge
//   rt_post.cpp, rt_scene_edit.cpp, rt_matte.cpp, rt_query.cpp, rt_comm.cpp, rt_chain.cpp
// Internal; not part of the public boundary.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "rt_context.h"

struct rt_adaptive_params;  // include/rt_adaptive.h
namespace rtk {
struct TraceParams;         // rt_kernels.h
}

namespace rti {

// ---- rt_abi.cpp ----
// Records `msg` as this thread's rt_last_error() text and returns `s`.
rt_status fail(rt_status s, const std::string& msg);
rt_status hip_fail(hipError_t e, const char* what);
// RT_ERR_INVALID_SIZE unless 1 <= w, h <= 65536.
rt_status check_image(uint32_t w, uint32_t h);
// Whether a parameter is neither negative, NaN nor infinite.
inline bool nonneg_finite(float x) { return x >= 0.0f && x <= FLT_MAX; }
// WGSL u32(f32) on the host (truncate, saturate, NaN -> 0), as rtd::f2u.
inline uint32_t host_f2u(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}
// The seed words of a launch's n frames (wgsl:311: u32(random_seed * 2^32)).
inline void fill_seeds(uint32_t* seed_b, const float* seeds, uint32_t n) {
    for (uint32_t f = 0; f < n; ++f) seed_b[f] = host_f2u(seeds[f] * 4294967296.0f);
}
// The camera's ray grid, and its lens, in a kernel parameter block (TraceParams, AovParams,
// MatteParams).
template <class P>
void fill_camera_grid(P& p, const rt_scene_camera& c) {
    for (int i = 0; i < 3; ++i) {
        p.center[i] = c.center[i];
        p.vul[i] = c.viewport_upper_left[i];
        p.pdu[i] = c.pixel_delta_u[i];
        p.pdv[i] = c.pixel_delta_v[i];
    }
}
template <class P>
void fill_camera_lens(P& p, const rt_scene_camera& c) {
    for (int i = 0; i < 3; ++i) {
        p.ddu[i] = c.defocus_disk_u[i];
        p.ddv[i] = c.defocus_disk_v[i];
    }
    p.defocus_angle = c.defocus_angle;
}
// The 8x8 tiles of a launch over b bands of a w-texel-wide image.
inline uint64_t launch_tiles(uint32_t w, uint32_t b) { return (uint64_t)((w + 7u) >> 3) * b; }
// The round-robin stripes of rank / nranks as a band set (band b -> rank b mod nranks).
rt_band_set stripe_set(uint32_t h, uint32_t rank, uint32_t nranks);
// A band set the kernels can run: inside the image, step >= 1, and (for two or more bands)
// first and step within the packed stripe map's 16 / 15 bits (rtk::pack_bands).
rt_status check_band_set(uint32_t h, const rt_band_set& bs);
// What rt_update_adaptive, rt_converge_frames and rt_progress_stats refuse of an
// rt_adaptive_params.
rt_status check_adaptive_params(const rt_adaptive_params& params);
// Whether nranks band sets cover every band of a height-row image exactly once, each within
// rows_per_rank rows (rt_deinterleave_bands' precondition).
bool band_sets_cover(uint32_t height, uint32_t nranks, const rt_band_set* sets,
                     uint32_t rows_per_rank);

// ---- rt_scene.cpp ----
bool camera_rays_bounded(const rt_ctx* ctx, const rtk::TraceParams& p);
// The scene upload every trace call does (only when the bytes change; the device must be
// current): afterwards ctx->d_geom holds the scan records (cx, cy, cz, r*r), zero-padded as the
// scans expect, and ctx->d_sph the sphere records.  Nothing outside the scene fields changes.
rt_status upload_spheres(rt_ctx* ctx, const rt_sphere* spheres, uint32_t count,
                         hipStream_t stream);

// ---- rt_plan.cpp ----
int trace_kernel_for(const rt_ctx* ctx, const rtk::TraceParams& p);
int single_or(const rt_ctx* ctx, const rtk::TraceParams& p, int kernel);
uint32_t frames_per_launch_for(const rt_ctx* ctx, const rtk::TraceParams& p);
int frame_group_kernel(const rt_ctx* ctx, const rtk::TraceParams& p);
// The scheduling units of a frame-group kernel's launch: tiles per unit, units per band row, units.
struct UnitGrid {
    uint32_t group, units_x;
    uint64_t units;
};
UnitGrid frame_group_units(int kernel, uint32_t w, uint32_t bands);
uint32_t update_parts(const rt_ctx* ctx, const rtk::TraceParams& p, int kernel);
uint32_t update_parts_aql(const rt_ctx* ctx, const rtk::TraceParams& p);
void free_candidates(rt_ctx* ctx);
rt_status ensure_order_buffers(rt_ctx* ctx, uint64_t tiles, hipStream_t stream);
rt_status plan_tile_order(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream);
rt_status plan_wg_order(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream);
rt_status plan_hint_rs(rt_ctx* ctx, rtk::TraceParams& p, int kernel);
rt_status plan_split(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream);
void finish_tile_order(rt_ctx* ctx, const rtk::TraceParams& p);
bool lookup_count(const rt_ctx* ctx, const void* image, const rtk::TraceParams& p, uint32_t& n);
void record_count(rt_ctx* ctx, const void* image, const rtk::TraceParams& p, uint32_t n);
// Drops what the context knows about `image`'s sample counts (the source of the kernels' count
// hint): for a call that leaves per-pixel counts in it.
void forget_count(rt_ctx* ctx, const void* image);
uint32_t next_count(uint32_t n, uint32_t spp);
uint32_t fill_hint(rtk::TraceParams& p, uint32_t n_in);
void plan_hint(rt_ctx* ctx, rtk::TraceParams& p, const void* in, const void* out);
void fill_camera(rtk::TraceParams& p, const rt_scene_camera& c);
rt_status prepare(rt_ctx* ctx, const void* in, const void* out, uint32_t w, uint32_t h,
                  const rt_band_set& bs, const rt_scene_camera* cam, const rt_sphere* spheres,
                  uint32_t count, const float* seeds, hipStream_t stream, rtk::TraceParams& p);

// ---- rt_frames.cpp ----
rt_status chain_report(rt_ctx* ctx);

// Switches to a device for the duration of a call.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

}  // namespace rti

// One-frame updates as AQL packets on context-owned HSA queues (rt_chain.cpp).  A segment
// is begin, up to kMaxSegmentPackets frame packets (one per frame and part, part k on queue
// k), end; it is ordered after the work issued on `stream` before begin, and `stream`'s
// later work after it.  chain_create never fails softly: chain_ok tells whether the
// machine offers what the chain needs (why: the reason if not), a hard error is returned.
// Every wait is bounded: a segment whose go wait gives up drops its frames (the chain
// kernels check the abort word before storing), a queue error or a segment that does not
// complete within the bound marks the chain failed (chain_failed), and the context then
// runs HIP launches.
namespace rtc {
struct Chain;
constexpr uint32_t kMaxSegmentPackets = 1024;
Chain* chain_create(int device, rt_status* status);
// RT_ERR_HIP (and the resources left in place) if a segment did not complete in time
rt_status chain_destroy(Chain* c);
bool chain_ok(const Chain* c, const char** why);
// whether a go wait gave up or a queue reported an error (no synchronisation)
bool chain_failed(Chain* c);
// the queues of `parts` parts exist (created now if not); false if one cannot be created
bool chain_queues(Chain* c, uint32_t parts);
rt_status chain_begin(Chain* c, hipStream_t stream, uint32_t parts);
rt_status chain_frame(Chain* c, const rtk::TraceParams& p, int kernel, uint32_t part);
rt_status chain_end(Chain* c, hipStream_t stream);
// drops an open segment (nothing of it has been submitted yet)
void chain_abort(Chain* c);
// 1 if a go wait gave up (its segment's frames were dropped), else 0; waits (bounded) for
// every segment in flight
rt_status chain_errors(Chain* c, uint32_t* out);
uint64_t chain_packets(const Chain* c);
}  // namespace rtc
