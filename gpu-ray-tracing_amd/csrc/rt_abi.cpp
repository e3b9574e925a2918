// rt_abi.cpp — the core of the C ABI of librt_hip.so (declared in include/rt_abi.h): the
// last-error text and the argument checks every unit uses, rt_create / rt_destroy, the setters
// and getters, the diagnostics, the band partition and the de-interleave, the self-tests and
// present.  The scene, the launch planning, the render calls and the other trace launches are
// units of their own (rt_scene.cpp, rt_plan.cpp, rt_frames.cpp, rt_tracers.cpp; rt_internal.h).
//
// Replaces the render-world half of the reference's plugin (src/lib.rs):
//   ComputeShaderPipeline::from_world (240-324)  -> rt_create (code objects are linked in)
//   ComputeShaderNode::run (379-421)             -> rt_init_image (rt_update: rt_frames.cpp)
// Errors are status codes instead of panics/unwraps (lib.rs:216-217, 356-358, 399-411).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt_adaptive.h"
#include "rt_chain_parts.h"
#include "rt_internal.h"
#include "rt_kernels.h"
#include "rt_certain_tiles.h"
#include "rt_occlusion_cull.h"
#include "rt_selftest_roots.h"
#include "rt_tile_lists.h"

namespace {
thread_local std::string g_last_error = "";
}  // namespace

namespace rti {

rt_status fail(rt_status s, const std::string& msg) {
    g_last_error = msg;
    return s;
}

rt_status hip_fail(hipError_t e, const char* what) {
    return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

constexpr uint32_t kMaxDim = 1u << 16;         // 65536 x 65536 texels

rt_status check_image(uint32_t w, uint32_t h) {
    if (w == 0 || h == 0 || w > kMaxDim || h > kMaxDim)
        return fail(RT_ERR_INVALID_SIZE, "image size out of range (1..65536 per side)");
    return RT_OK;
}

// The round-robin stripes of rank / nranks as a band set (band b -> rank b mod nranks).
rt_band_set stripe_set(uint32_t h, uint32_t rank, uint32_t nranks) {
    const uint32_t bands = (h + RT_STRIPE_ROWS - 1) / RT_STRIPE_ROWS;
    return {rank, nranks, bands > rank ? (bands - rank + nranks - 1) / nranks : 0u};
}

// A band set the kernels can run: inside the image, step >= 1, and (for two or more bands)
// first and step within the packed stripe map's 16 / 15 bits (rtk::pack_bands).
rt_status check_band_set(uint32_t h, const rt_band_set& bs) {
    const uint32_t bands = (h + RT_STRIPE_ROWS - 1) / RT_STRIPE_ROWS;
    if (bs.step == 0) return fail(RT_ERR_INVALID_ARGUMENT, "band set step is 0");
    if (bs.count == 0) return RT_OK;
    if (bs.first >= bands || (uint64_t)bs.first + (uint64_t)(bs.count - 1u) * bs.step >= bands)
        return fail(RT_ERR_INVALID_ARGUMENT, "band set reaches past the image");
    if (bs.first > 0xFFFFu || (bs.count >= 2u && bs.step >= 0x7FFFu))
        return fail(RT_ERR_INVALID_ARGUMENT, "band set first / step out of range");
    return RT_OK;
}

// What rt_update_adaptive, rt_converge_frames and rt_progress_stats refuse of an
// rt_adaptive_params.
rt_status check_adaptive_params(const rt_adaptive_params& params) {
    if (params.min_samples > (1u << 24))
        return fail(RT_ERR_INVALID_ARGUMENT, "min_samples above 16777216");
    if (!nonneg_finite(params.abs_tolerance2) || !nonneg_finite(params.rel_tolerance2))
        return fail(RT_ERR_INVALID_ARGUMENT, "a tolerance is negative, NaN or infinite");
    return RT_OK;
}

}  // namespace rti

namespace {

using namespace rti;

// gathered row of every output band: band_src[b] = the row (in rows_per_rank-row rank
// buffers back to back) where band b's first row lies; false if the sets do not cover every
// band exactly once or a set exceeds rows_per_rank
bool band_sources(uint32_t h, uint32_t nranks, const rt_band_set* sets, uint32_t rows_per_rank,
                  std::vector<uint32_t>& out) {
    const uint32_t bands = (h + RT_STRIPE_ROWS - 1) / RT_STRIPE_ROWS;
    out.assign(bands, ~0u);
    uint64_t seen = 0;
    for (uint32_t r = 0; r < nranks; ++r) {
        const rt_band_set& bs = sets[r];
        if (check_band_set(h, bs) != RT_OK) return false;
        if ((uint64_t)bs.count * RT_STRIPE_ROWS > rows_per_rank) return false;
        for (uint32_t j = 0; j < bs.count; ++j) {
            const uint32_t b = bs.first + j * bs.step;
            if (out[b] != ~0u) return false;          // two owners
            out[b] = (uint32_t)((uint64_t)r * rows_per_rank + (uint64_t)j * RT_STRIPE_ROWS);
            ++seen;
        }
    }
    return seen == bands;
}

}  // namespace

namespace rti {
bool band_sets_cover(uint32_t h, uint32_t nranks, const rt_band_set* sets,
                     uint32_t rows_per_rank) {
    std::vector<uint32_t> src;
    return band_sources(h, nranks, sets, rows_per_rank, src);
}
}  // namespace rti

extern "C" {

uint32_t rt_abi_version(void) { return RT_ABI_VERSION; }

const char* rt_last_error(void) { return g_last_error.c_str(); }

const char* rt_kernel_name(int which) {
    static const char* const names[] = {"rt_trace_kernel<0>",      "rt_trace_kernel<1>",
                                        "rt_trace_kernel<2>",      "rt_trace_kernel<3>",
                                        "rt_trace_kernel<4>",      "rt_bounce_kernel<0>",
                                        "rt_bounce_kernel<1>",     "rt_bounce_kernel<2>",
                                        rtk::single_kernel_name(0),
                                        rtk::single_kernel_name(1),
                                        "rt_bounce_kernel<3>",     "rt_tpair_kernel<2>",
                                        "rt_tpair_kernel<4>"};
    if (which >= 0 && which < (int)(sizeof(names) / sizeof(names[0]))) return names[which];
    return rtk::trace_kernel_name();
}

rt_status rt_last_launch_info(const rt_ctx* ctx, rt_launch_info* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = ctx->last;
    return RT_OK;
}

rt_status rt_candidate_stats(rt_ctx* ctx, uint64_t out[5]) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    for (int i = 0; i < 5; ++i) out[i] = 0;
    out[4] = rtk::kCandMax;
    if (!ctx->cand || ctx->cand_live == 0) return RT_OK;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    // the count is the first word of each tile's kCandStride-float4 block
    std::vector<uint32_t> cnt(ctx->cand_live);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy2D(cnt.data(), sizeof(uint32_t), ctx->cand, rtk::kCandStride * sizeof(float4),
                        sizeof(uint32_t), cnt.size(), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy2D(candidate counts)");
    out[0] = cnt.size();
    for (uint32_t c : cnt) {
        if (c == rtk::kCandNone) {
            out[1]++;
        } else {
            out[2] += c;
            out[3] = std::max<uint64_t>(out[3], c);
        }
    }
    return RT_OK;
}

rt_status rt_set_occlusion_cull(rt_ctx* ctx, int on) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (on != 0 && on != 1) return fail(RT_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    ctx->occlusion_cull = on != 0;   // (part of the lists' key: the next trace call rebuilds them)
    return RT_OK;
}

rt_status rt_occlusion_cull_stats(rt_ctx* ctx, uint64_t out[2]) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    out[0] = out[1] = 0;
    if (!ctx->cand || ctx->cand_live == 0) return RT_OK;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    // (count, removed) are the first two words of each tile's kCandStride-float4 block
    std::vector<uint32_t> head(2 * ctx->cand_live);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy2D(head.data(), 2 * sizeof(uint32_t), ctx->cand,
                        rtk::kCandStride * sizeof(float4), 2 * sizeof(uint32_t), ctx->cand_live,
                        hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy2D(candidate counts)");
    for (uint64_t t = 0; t < ctx->cand_live; ++t) {
        if (head[2 * t] == rtk::kCandNone) continue;
        out[0] += head[2 * t + 1];
        out[1] += head[2 * t + 1] ? 1u : 0u;
    }
    return RT_OK;
}

rt_status rt_set_certain_tiles(rt_ctx* ctx, int on) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (on != 0 && on != 1) return fail(RT_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    ctx->certain_tiles = on != 0;    // (part of the lists' key: the next trace call rebuilds them)
    return RT_OK;
}

rt_status rt_certain_tiles_stats(rt_ctx* ctx, uint64_t out[2]) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    out[0] = out[1] = 0;
    // (RT_SCAN_EXHAUSTIVE reads no lists: whatever an earlier build left is not in use)
    if (!ctx->cand || ctx->cand_live == 0 || ctx->scan_mode != RT_SCAN_CULLED) return RT_OK;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    // the flag word is the third word of each tile's kCandStride-float4 block
    std::vector<uint32_t> flags(ctx->cand_live);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy2D(flags.data(), sizeof(uint32_t),
                        reinterpret_cast<const uint32_t*>(ctx->cand) + 2,
                        rtk::kCandStride * sizeof(float4), sizeof(uint32_t), ctx->cand_live,
                        hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy2D(tile flags)");
    for (uint32_t f : flags) out[0] += f & rtk::kTileCertain;
    // the pairs of the last tile-pair launch, if it read these lists: tiles 2u and 2u + 1 of a
    // band, both inside the image
    const uint64_t tx = ctx->pair_tiles_x;
    if (ctx->pair_gen == ctx->cand_gen && tx * ctx->pair_bands == ctx->cand_live)
        for (uint64_t b = 0; b < ctx->pair_bands; ++b)
            for (uint64_t x = 0; x + 1 < tx; x += 2)
                out[1] += flags[b * tx + x] & flags[b * tx + x + 1] & rtk::kTileCertain;
    return RT_OK;
}

rt_status rt_set_tight_bundle(rt_ctx* ctx, int on) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (on != 0 && on != 1) return fail(RT_ERR_INVALID_ARGUMENT, "on must be 0 or 1");
    ctx->tight_bundle = on != 0;     // (part of the lists' key: the next trace call rebuilds them)
    return RT_OK;
}

// an rt_tile_list is the head of a tile's candidate block: the count word's float4, then the
// scan records
static_assert(RT_TILE_LIST_MAX == rtk::kCandMax && rtk::kCandRecOff == 1u &&
                  sizeof(rt_tile_list) == (1u + rtk::kCandMax) * sizeof(float4) &&
                  RT_TILE_LIST_NONE == rtk::kCandNone && RT_TILE_CERTAIN == rtk::kTileCertain,
              "rt_tile_list mirrors the candidate block");

rt_status rt_tile_lists(rt_ctx* ctx, rt_tile_list* out, uint64_t capacity, uint64_t* tiles) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!tiles) return fail(RT_ERR_INVALID_ARGUMENT, "tiles is NULL");
    *tiles = 0;
    // (RT_SCAN_EXHAUSTIVE reads no lists: whatever an earlier build left is not in use)
    if (!ctx->cand || ctx->cand_live == 0 || ctx->scan_mode != RT_SCAN_CULLED) return RT_OK;
    *tiles = ctx->cand_live;
    const uint64_t n = std::min<uint64_t>(ctx->cand_live, capacity);
    if (!out || n == 0) return RT_OK;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy2D(out, sizeof(rt_tile_list), ctx->cand, rtk::kCandStride * sizeof(float4),
                        sizeof(rt_tile_list), n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy2D(tile lists)");
    for (uint64_t t = 0; t < n; ++t) {
        rt_tile_list& l = out[t];
        l.reserved = 0;
        const uint32_t kept = l.count == RT_TILE_LIST_NONE ? 0u : std::min(l.count, RT_TILE_LIST_MAX);
        if (kept < RT_TILE_LIST_MAX)
            std::memset(l.records[kept], 0, (RT_TILE_LIST_MAX - kept) * sizeof(l.records[0]));
    }
    return RT_OK;
}

rt_status rt_create(int device, rt_ctx** out_ctx) {
    if (!out_ctx) return fail(RT_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (device < 0 || device >= n) return fail(RT_ERR_INVALID_DEVICE, "no such HIP device");
    rt_ctx* ctx = new (std::nothrow) rt_ctx();
    if (!ctx) return fail(RT_ERR_NO_MEMORY, "out of host memory");
    ctx->device = device;
    *out_ctx = ctx;
    return RT_OK;
}

rt_status rt_destroy(rt_ctx* ctx) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    rt_status st = RT_OK;
    {
        DeviceGuard guard(ctx->device);
        if (ctx->d_geom || ctx->d_sph || ctx->cand) (void)hipDeviceSynchronize();
        (void)hipFree(ctx->d_geom);
        (void)hipFree(ctx->d_sph);
        (void)hipFree(ctx->d_flag);
        (void)hipFree(ctx->d_hint_rs);
        (void)hipFree(ctx->d_band_src);
        for (hipEvent_t ev : ctx->time_ev)
            if (ev) (void)hipEventDestroy(ev);
        (void)hipFree(ctx->d_srgb);
        (void)hipFree(ctx->d_hx);
        (void)hipFree(ctx->tile_cost);
        (void)hipFree(ctx->tile_order);
        (void)hipFree(ctx->d_grid);
        (void)hipFree(ctx->wg_buf);
        (void)hipFree(ctx->split_col);
        (void)hipFree(ctx->split_cnt);
        (void)hipFree(ctx->unit_order);
        (void)hipFree(ctx->d_pick);
        (void)hipFree(ctx->d_progress);
        (void)hipFree(ctx->d_matte);
        if (ctx->h_progress) (void)hipHostFree(ctx->h_progress);
        free_candidates(ctx);
        for (uint32_t k = 0; k + 1 < RT_MAX_UPDATE_QUEUES; ++k) {
            if (ctx->aux[k]) (void)hipStreamDestroy(ctx->aux[k]);
            if (ctx->join_ev[k]) (void)hipEventDestroy(ctx->join_ev[k]);
        }
        if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
        st = chain_report(ctx);
        // (a segment still outstanding after the bound leaves the chain's resources in place)
        if (rt_status d = rtc::chain_destroy(ctx->chain)) st = d;
    }
    delete ctx;
    return st;
}

rt_status rt_set_scan_mode(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_SCAN_EXHAUSTIVE && mode != RT_SCAN_CULLED)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown scan mode");
    ctx->scan_mode = mode;
    return RT_OK;
}

rt_status rt_set_frames_per_launch(rt_ctx* ctx, uint32_t frames_per_launch) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    ctx->frames_per_launch = frames_per_launch;
    return RT_OK;
}

rt_status rt_set_frame_pairs(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_FRAME_PAIRS_AUTO && mode != RT_FRAME_PAIRS_OFF && mode != RT_FRAME_PAIRS_ON &&
        mode != RT_FRAME_PAIRS_QUAD && mode != RT_FRAME_PAIRS_ON2 && mode != RT_FRAME_PAIRS_QUAD2)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown frame-pair mode");
    ctx->frame_pairs = mode;
    return RT_OK;
}

rt_status rt_set_path_compaction(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_PATHS_AUTO && mode != RT_PATHS_PER_WAVE && mode != RT_PATHS_COMPACT &&
        mode != RT_PATHS_PAIR && mode != RT_PATHS_SPLIT)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown path-compaction mode");
    ctx->path_compaction = mode;
    return RT_OK;
}

rt_status rt_set_single_kernel(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_SINGLE_AUTO && mode != RT_SINGLE_OFF && mode != RT_SINGLE_PAIR &&
        mode != RT_SINGLE_ONE)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown single-kernel mode");
    ctx->single_kernel = mode;
    return RT_OK;
}

rt_status rt_set_update_queues(rt_ctx* ctx, uint32_t queues) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (queues > RT_MAX_UPDATE_QUEUES)
        return fail(RT_ERR_INVALID_ARGUMENT, "queues above RT_MAX_UPDATE_QUEUES");
    ctx->update_queues = queues;
    return RT_OK;
}

rt_status rt_set_update_submit(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_SUBMIT_AUTO && mode != RT_SUBMIT_HIP && mode != RT_SUBMIT_AQL)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown submit mode");
    ctx->update_submit = mode;
    return RT_OK;
}

rt_status rt_update_submit_status(rt_ctx* ctx, int* aql_available, uint32_t* go_give_ups,
                                  uint64_t* packets) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    if (!ctx->chain_tried) {
        // (sets the chain up without any HSA queue: queues are created by the first segment)
        ctx->chain_tried = true;
        rt_status st = RT_OK;
        ctx->chain = rtc::chain_create(ctx->device, &st);
        if (st != RT_OK) return st;
    }
    uint32_t gave_up = 0;
    if (ctx->chain && !rtc::chain_failed(ctx->chain))
        if (rt_status s = rtc::chain_errors(ctx->chain, &gave_up)) return s;
    if (rt_status s = chain_report(ctx)) return s;
    const char* why = "";
    const bool ok = rtc::chain_ok(ctx->chain, &why);
    if (aql_available) *aql_available = ok ? 1 : 0;
    if (packets) *packets = rtc::chain_packets(ctx->chain);
    if (go_give_ups) *go_give_ups = (ctx->chain && rtc::chain_failed(ctx->chain)) ? 1u : gave_up;
    if (!ok) fail(RT_OK, std::string("AQL submission unavailable: ") + why);
    return RT_OK;
}

rt_status rt_set_frame_images(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_FRAME_IMAGES_LAST_TWO && mode != RT_FRAME_IMAGES_EVERY)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown frame-images mode");
    ctx->frame_images = mode;
    return RT_OK;
}

rt_status rt_set_tile_order(rt_ctx* ctx, int mode) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (mode != RT_TILE_ORDER_AUTO && mode != RT_TILE_ORDER_OFF)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown tile-order mode");
    ctx->tile_order_mode = mode;
    return RT_OK;
}

rt_status rt_get_frames_per_launch(const rt_ctx* ctx, const rt_scene_camera* cam,
                                   uint32_t* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!cam || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL camera or out");
    rtk::TraceParams p;
    std::memset(&p, 0, sizeof(p));
    fill_camera(p, *cam);
    *out = frames_per_launch_for(ctx, p);
    return RT_OK;
}

rt_status rt_set_spheres(rt_ctx* ctx, const rt_sphere* spheres, uint32_t count, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    return upload_spheres(ctx, spheres, count, static_cast<hipStream_t>(stream));
}

rt_status rt_init_image(rt_ctx* ctx, float* out, uint32_t w, uint32_t h, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out_rgba is NULL");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipError_t e = rtk::launch_init(reinterpret_cast<float4*>(out), (uint64_t)w * h,
                                    static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "rt_init_kernel launch");
    // every pixel now holds count 0 (for a whole-image update of this size)
    rtk::TraceParams p;
    std::memset(&p, 0, sizeof(p));
    p.width = w;
    p.height = h;
    p.band_step = 1;
    record_count(ctx, out, p, 0u);
    return RT_OK;
}

rt_status rt_band_costs(rt_ctx* ctx, uint32_t w, uint32_t h, const rt_band_set* bands,
                        double* out_cost) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands || !out_cost) return fail(RT_ERR_INVALID_ARGUMENT, "NULL bands or out_cost");
    const uint32_t group = ctx->cost_key[5];
    const uint32_t want[5] = {w, h, bands->first, bands->step, bands->count};
    // (and for the lists the context holds now: another camera geometry, scene or share
    // since then starts a new generation, whose costs are not measured yet)
    if (!ctx->cost_key_ok || !ctx->tile_cost || !std::equal(want, want + 5, ctx->cost_key) ||
        ctx->cost_gen != ctx->cand_gen)
        return fail(RT_ERR_INVALID_ARGUMENT, "no tile costs recorded for this share");
    const uint32_t tiles_x = (((w + 7u) >> 3) + group - 1u) / group;
    const uint64_t units = (uint64_t)tiles_x * bands->count;
    std::vector<uint32_t> c(units);
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    if (units) {
        hipError_t e = hipMemcpy(c.data(), ctx->tile_cost, units * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(tile costs)");
    }
    for (uint32_t j = 0; j < bands->count; ++j) {
        double sum = 0.0;
        for (uint32_t x = 0; x < tiles_x; ++x) sum += c[(uint64_t)j * tiles_x + x];
        out_cost[j] = sum;
    }
    return RT_OK;
}

rt_status rt_set_chain_parts(rt_ctx* ctx, uint32_t parts) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (parts > RT_MAX_CHAIN_PARTS)
        return fail(RT_ERR_INVALID_ARGUMENT, "parts above RT_MAX_CHAIN_PARTS");
    ctx->chain_parts = parts;
    return RT_OK;
}

rt_status rt_partition_bands(const double* cost, uint32_t nbands, uint32_t nranks,
                             rt_band_set* out) {
    if (!cost || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL band_cost or out");
    if (nranks == 0) return fail(RT_ERR_INVALID_ARGUMENT, "nranks is 0");
    if (nbands > 65536u) return fail(RT_ERR_INVALID_SIZE, "more than 65536 bands");
    for (uint32_t b = 0; b < nbands; ++b)
        if (!(cost[b] >= 0.0) || !std::isfinite(cost[b]))
            return fail(RT_ERR_INVALID_ARGUMENT, "band costs must be finite and >= 0");
    // The smallest largest-range cost B* over all cuts into at most nranks contiguous ranges
    // (a range's cost: the difference of prefix sums), by bisection over B with the greedy
    // test "ranges as long as they fit under B" (O(bands) per step, memory O(bands)).  The
    // test is monotone in B and changes only at range costs, so once lo < hi are adjacent
    // doubles with hi feasible and lo not, B* = hi exactly.  The cut under hi then takes
    // ranges as long as fit but always leaves one band for each rank still to come, so it
    // uses min(nranks, nbands) ranges: once that bound binds, every later range is one band,
    // which fits (B* >= every band's cost).
    std::vector<double> pre(nbands + 1, 0.0);
    for (uint32_t b = 0; b < nbands; ++b) pre[b + 1] = pre[b] + cost[b];
    auto cuts = [&](double B, std::vector<uint32_t>* starts) -> uint64_t {
        uint64_t n = 0;
        for (uint32_t i = 0; i < nbands;) {
            uint32_t j = i + 1;                      // a range holds at least one band
            if (pre[j] - pre[i] > B) return UINT64_MAX;
            // (the final cut: leave a band for each of the ranks after this one)
            const uint64_t left = starts && nranks > n + 1 ? nranks - n - 1 : 0;
            const uint32_t jmax = left >= nbands ? i + 1
                                                 : std::max<uint32_t>(i + 1, nbands - (uint32_t)left);
            while (j < jmax && pre[j + 1] - pre[i] <= B) ++j;
            if (starts) starts->push_back(i);
            ++n;
            i = j;
        }
        return n;
    };
    double lo = 0.0, hi = pre[nbands];
    for (uint32_t b = 0; b < nbands; ++b) lo = std::max(lo, cost[b]);
    if (cuts(lo, nullptr) <= nranks) {
        hi = lo;
    } else {
        for (int it = 0; it < 2200; ++it) {              // (2^-1074 steps cover any range)
            const double mid = lo + (hi - lo) / 2.0;
            if (!(mid > lo && mid < hi)) break;
            if (cuts(mid, nullptr) <= nranks) hi = mid; else lo = mid;
        }
    }
    std::vector<uint32_t> starts;
    cuts(hi, &starts);
    starts.push_back(nbands);
    for (uint32_t r = 0; r < nranks; ++r) {
        if (r + 1 < starts.size())
            out[r] = {starts[r], 1u, starts[r + 1] - starts[r]};
        else
            out[r] = {0u, 1u, 0u};   // no band left (more ranks than ranges)
    }
    return RT_OK;
}

rt_status rt_deinterleave_bands(rt_ctx* ctx, const float* gathered, float* out, uint32_t w,
                                uint32_t h, uint32_t nranks, const rt_band_set* sets,
                                uint32_t rows_per_rank, void* stream_v) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!gathered || !out || !sets) return fail(RT_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (gathered == out) return fail(RT_ERR_INVALID_ARGUMENT, "gathered and out alias");
    if (nranks == 0) return fail(RT_ERR_INVALID_ARGUMENT, "nranks is 0");
    if (rt_status s = check_image(w, h)) return s;
    std::vector<uint32_t> src;
    if (!band_sources(h, nranks, sets, rows_per_rank, src))
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "band sets must cover every band once, each within rows_per_rank rows");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (src != ctx->band_src) {
        // (the previous table may still be read by a queued de-interleave)
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        if (src.size() > ctx->band_src.size() || !ctx->d_band_src) {
            (void)hipFree(ctx->d_band_src);
            ctx->d_band_src = nullptr;
            ctx->band_src.clear();
            e = hipMalloc(&ctx->d_band_src, src.size() * sizeof(uint32_t));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(band table)");
        }
        e = hipMemcpy(ctx->d_band_src, src.data(), src.size() * sizeof(uint32_t),
                      hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy(band table)");
        ctx->band_src = src;
    }
    hipError_t e = rtk::launch_deinterleave_bands(
        reinterpret_cast<const float4*>(gathered), reinterpret_cast<float4*>(out), w, h,
        ctx->d_band_src, stream);
    return e == hipSuccess ? RT_OK : hip_fail(e, "rt_deinterleave_bands_kernel launch");
}

uint32_t rt_stripe_local_rows(uint32_t height, uint32_t rank, uint32_t nranks) {
    if (nranks == 0 || rank >= nranks) return 0;
    const uint32_t bands = (height + RT_STRIPE_ROWS - 1) / RT_STRIPE_ROWS;
    const uint32_t local = bands > rank ? (bands - rank + nranks - 1) / nranks : 0;
    return local * RT_STRIPE_ROWS;
}


rt_status rt_deinterleave_stripes(rt_ctx* ctx, const float* gathered, float* out, uint32_t w,
                                  uint32_t h, uint32_t nranks, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!gathered || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (gathered == out) return fail(RT_ERR_INVALID_ARGUMENT, "gathered and out alias");
    if (nranks == 0) return fail(RT_ERR_INVALID_ARGUMENT, "nranks is 0");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipError_t e = rtk::launch_deinterleave(
        reinterpret_cast<const float4*>(gathered), reinterpret_cast<float4*>(out), w, h,
        nranks, rt_stripe_local_rows(h, 0, nranks), static_cast<hipStream_t>(stream));
    return e == hipSuccess ? RT_OK : hip_fail(e, "rt_deinterleave_kernel launch");
}

rt_status rt_selftest_fastmath(rt_ctx* ctx, uint64_t n_random, uint64_t out[5]) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    unsigned long long* d = nullptr;
    hipError_t e = hipMalloc(&d, 5 * sizeof(unsigned long long));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(selftest)");
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    e = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtk::launch_selftest(d, n_random, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "rt_selftest_kernel");
    for (int i = 0; i < 5; ++i) out[i] = h[i];
    return RT_OK;
}

rt_status rt_selftest_roots(rt_ctx* ctx, uint64_t n_random,
                            rt_roots_tally out[RT_ROOTS_FAMILIES * RT_ROOTS_STRATA]) {
    static_assert(RT_ROOTS_FAMILIES == rtk::kRootFamilies && RT_ROOTS_STRATA == rtk::kRootStrata,
                  "rt_selftest_roots.h and rt_kernels.h disagree");
    constexpr size_t kN = RT_ROOTS_FAMILIES * RT_ROOTS_STRATA * 4u;
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    unsigned long long* d = nullptr;
    hipError_t e = hipMalloc(&d, kN * sizeof(unsigned long long));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(selftest roots)");
    unsigned long long h[kN] = {};
    e = hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtk::launch_selftest_roots(d, n_random, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "rt_selftest_roots_kernel");
    for (size_t i = 0; i < kN / 4u; ++i) {
        out[i].mismatches = h[4 * i];
        out[i].drawn = h[4 * i + 1];
        out[i].compared = h[4 * i + 2];
        out[i].rooted = h[4 * i + 3];
    }
    return RT_OK;
}

void rt_srgb_thresholds(float out[256]) {
    out[0] = 0.0f;
    for (int j = 1; j < 256; ++j) {
        const double v = (j - 0.5) / 255.0;  // encoded boundary between j-1 and j
        const double lin = v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4);
        float f = (float)lin;
        if ((double)f < lin) f = std::nextafter(f, 2.0f);
        out[j] = f;
    }
}

rt_status rt_present_rgba8(rt_ctx* ctx, const float* in, uint8_t* out, uint32_t w, uint32_t h,
                           int encoding, void* stream_v) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!in || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL image");
    if (encoding != RT_ENCODE_LINEAR && encoding != RT_ENCODE_SRGB)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown encoding");
    if (rt_status s = check_image(w, h)) return s;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (encoding == RT_ENCODE_SRGB && !ctx->d_srgb) {
        float t[256];
        rt_srgb_thresholds(t);
        float* d = nullptr;
        hipError_t e = hipMalloc(&d, sizeof(t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(sRGB table)");
        e = hipMemcpy(d, t, sizeof(t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return hip_fail(e, "hipMemcpy(sRGB table)");
        }
        ctx->d_srgb = d;
    }
    hipError_t e = rtk::launch_present(reinterpret_cast<const float4*>(in),
                                       reinterpret_cast<uchar4*>(out), (uint64_t)w * h,
                                       encoding == RT_ENCODE_SRGB ? ctx->d_srgb : nullptr,
                                       stream);
    return e == hipSuccess ? RT_OK : hip_fail(e, "rt_present_kernel launch");
}

}  // extern "C"
