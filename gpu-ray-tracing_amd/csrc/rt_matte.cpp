// rt_matte.cpp — C-ABI entry points of include/rt_matte.h: the argument checks and launches of the
// coverage matte kernels (rt_matte.hip).  Of the context they use the device, the scan mode, the
// uploaded sphere records (rti::upload_spheres: the upload every trace call does) and the matte's
// own blocks (matte_blocks); candidate lists, orders, sample-count records, launch info and timing
// events are not touched.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_matte.h"
#include "rt_matte_kernels.h"

namespace {

using rti::check_band_set;
using rti::check_image;
using rti::DeviceGuard;
using rti::fail;
using rti::hip_fail;

static_assert(RT_MATTE_SLOTS == rtk::kMatteSlots, "the kernel's slots are the header's");
static_assert(RT_MATTE_LIST_CAPACITY == rtk::kMatteListCap, "the kernel's list is the header's");
static_assert(sizeof(rt_matte_planes) == 24 && sizeof(rt_matte_info) == 16,
              "rt_matte.h's structs are three pointers and four words");

constexpr uint32_t kMaxSelectable = 1u << 20;     // ids below this, or RT_AOV_MISS

// RT_MATTE_ROUTE=scan (environment, diagnostic) sends every tile to the per-frame scan.
bool scan_forced() {
    const char* env = std::getenv("RT_MATTE_ROUTE");
    return env && !std::strcmp(env, "scan");
}

// The context's blocks of rt_matte.h, allocated on first use (the device must be current): the
// last call's rt_matte_info on the device (d_matte, kInfoWords words), behind it rt_matte_resolve's
// selection mask (mask_words words); matte_mask is the host copy of the words the mask holds.
constexpr size_t kInfoWords = 16;               // rt_matte_info, padded to 64 bytes
rt_status matte_blocks(rt_ctx* ctx, size_t mask_words) {
    if (ctx->d_matte && ctx->matte_mask_words >= mask_words) return RT_OK;
    uint32_t* d = nullptr;
    hipError_t e = hipMalloc(&d, (kInfoWords + mask_words) * sizeof(uint32_t));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(matte blocks)");
    e = hipMemset(d, 0, (kInfoWords + mask_words) * sizeof(uint32_t));
    if (e == hipSuccess && ctx->d_matte) {
        // queued launches may still read the old block
        e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e = hipMemcpy(d, ctx->d_matte, kInfoWords * sizeof(uint32_t),
                          hipMemcpyDeviceToDevice);
    }
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "matte blocks setup");
    }
    (void)hipFree(ctx->d_matte);
    ctx->d_matte = d;
    ctx->matte_mask_words = mask_words;
    ctx->matte_mask.clear();                    // the new mask holds zeros
    return RT_OK;
}

// Shared body of rt_matte_frames / rt_matte_frames_bands: the checks, the scene upload, then one
// launch per kMatteMaxFrames frames on the caller's stream, each continuing in place.
rt_status matte_frames(rt_ctx* ctx, const rt_matte_planes* planes, uint32_t w, uint32_t h,
                       const rt_band_set& bs, const rt_scene_camera* cam, const rt_sphere* spheres,
                       uint32_t count, const float* seeds, uint32_t frames, hipStream_t stream) {
    if (!planes || !cam || !seeds)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL planes, camera or random_seeds");
    if (!planes->ids || !planes->counts || !planes->tally)
        return fail(RT_ERR_INVALID_ARGUMENT, "a matte plane is NULL");
    if (frames < 1u || frames > RT_MATTE_MAX_FRAMES)
        return fail(RT_ERR_INVALID_ARGUMENT, "frames outside 1..65536");
    if (w == 0u || h == 0u) return fail(RT_ERR_INVALID_ARGUMENT, "width or height is 0");
    if (rt_status s = check_image(w, h)) return s;
    if (rt_status s = check_band_set(h, bs)) return s;
    if (rt_status s = rti::upload_spheres(ctx, spheres, count, stream)) return s;
    if (rt_status s = matte_blocks(ctx, 64)) return s;
    // the call's counters start at zero, in stream order with the launches that add to them
    hipError_t e = hipMemsetAsync(ctx->d_matte, 0, sizeof(rt_matte_info), stream);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(matte info)");
    if (bs.count == 0) return RT_OK;

    rtk::MatteParams p;
    std::memset(&p, 0, sizeof(p));
    p.ids = reinterpret_cast<uint4*>(planes->ids);
    p.counts = reinterpret_cast<uint4*>(planes->counts);
    p.tally = reinterpret_cast<uint2*>(planes->tally);
    p.geom = ctx->d_geom;
    p.width = w;
    p.height = h;
    p.count = count;
    p.band_first = bs.first;
    p.band_step = bs.step;
    p.route = ctx->scan_mode == RT_SCAN_EXHAUSTIVE ? rtk::kMatteRouteExhaustive
              : scan_forced()                      ? rtk::kMatteRouteScan
                                                   : rtk::kMatteRouteList;
    rti::fill_camera_grid(p, *cam);
    rti::fill_camera_lens(p, *cam);
    for (uint32_t done = 0; done < frames; done += rtk::kMatteMaxFrames) {
        p.frames = std::min(frames - done, rtk::kMatteMaxFrames);
        p.reset_first = done == 0u && cam->camera_has_moved > 0.5f ? 1u : 0u;
        p.info = done == 0u ? ctx->d_matte : nullptr;  // every launch builds the same lists
        rti::fill_seeds(p.seed_b, seeds + done, p.frames);
        e = rtk::launch_matte(p, bs.count, stream);
        if (e != hipSuccess) return hip_fail(e, "rt_matte_kernel launch");
    }
    return RT_OK;
}

}  // namespace

extern "C" {

rt_status rt_matte_frames_bands(rt_ctx* ctx, const rt_matte_planes* planes, uint32_t w, uint32_t h,
                                const rt_band_set* bands, const rt_scene_camera* cam,
                                const rt_sphere* spheres, uint32_t count, const float* seeds,
                                uint32_t frames, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    return matte_frames(ctx, planes, w, h, *bands, cam, spheres, count, seeds, frames,
                        static_cast<hipStream_t>(stream));
}

rt_status rt_matte_frames(rt_ctx* ctx, const rt_matte_planes* planes, uint32_t w, uint32_t h,
                          const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                          const float* seeds, uint32_t frames, void* stream) {
    const rt_band_set all = rti::stripe_set(h, 0, 1);
    return rt_matte_frames_bands(ctx, planes, w, h, &all, cam, spheres, count, seeds, frames,
                                 stream);
}

rt_status rt_matte_resolve(rt_ctx* ctx, const rt_matte_planes* planes, uint64_t pixels,
                           const uint32_t* selected, uint32_t n_selected, float* alpha,
                           uint32_t* dominant, void* stream_v) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!planes || !planes->ids || !planes->counts || !planes->tally)
        return fail(RT_ERR_INVALID_ARGUMENT, "NULL planes or a matte plane is NULL");
    if (!alpha && !dominant) return fail(RT_ERR_INVALID_ARGUMENT, "alpha and dominant are NULL");
    if (!selected && n_selected > 0u)
        return fail(RT_ERR_INVALID_ARGUMENT, "selected_ids is NULL with selected_count > 0");
    if (pixels == 0u || pixels > (1ull << 32))
        return fail(RT_ERR_INVALID_ARGUMENT, "pixel_count outside 1..2^32");
    // the selection as a bit mask over the ids up to the largest one, and the background flag
    uint32_t background = 0u, top = 0u;
    for (uint32_t k = 0; k < n_selected; ++k) {
        if (selected[k] == RT_AOV_MISS)
            background = 1u;
        else if (selected[k] >= kMaxSelectable)
            return fail(RT_ERR_INVALID_ARGUMENT,
                        "a selected id is neither below 2^20 nor RT_AOV_MISS");
        else
            top = std::max(top, selected[k] + 1u);
    }
    std::vector<uint32_t> words((top + 31u) / 32u, 0u);
    for (uint32_t k = 0; k < n_selected; ++k)
        if (selected[k] != RT_AOV_MISS) words[selected[k] >> 5] |= 1u << (selected[k] & 31u);
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    size_t cap = 64;
    while (cap < words.size()) cap *= 2;
    if (rt_status s = matte_blocks(ctx, cap)) return s;
    uint32_t* const mask = ctx->d_matte + kInfoWords;
    // The mask is uploaded only when its words change, in stream order behind the launches that
    // read the old one, and waited for so that the staging vector can be replaced next time.
    if (words.size() > ctx->matte_mask.size() ||
        !std::equal(words.begin(), words.end(), ctx->matte_mask.begin())) {
        ctx->matte_mask.clear();
        hipError_t e = hipMemcpyAsync(mask, words.data(), words.size() * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(matte selection mask)");
        ctx->matte_mask = words;
    }
    rtk::MatteResolveParams p;
    std::memset(&p, 0, sizeof(p));
    p.ids = reinterpret_cast<const uint4*>(planes->ids);
    p.counts = reinterpret_cast<const uint4*>(planes->counts);
    p.tally = reinterpret_cast<const uint2*>(planes->tally);
    p.mask = mask;
    p.mask_bits = (uint32_t)words.size() * 32u;
    p.background = background;
    p.pixels = pixels;
    p.alpha = alpha;
    p.dominant = dominant;
    hipError_t e = rtk::launch_matte_resolve(p, stream);
    if (e != hipSuccess) return hip_fail(e, "rt_matte_resolve_kernel launch");
    return RT_OK;
}

rt_status rt_matte_last_info(rt_ctx* ctx, rt_matte_info* out) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "out is NULL");
    std::memset(out, 0, sizeof(*out));
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    if (rt_status s = matte_blocks(ctx, 64)) return s;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, ctx->d_matte, sizeof(*out), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(matte info)");
    return RT_OK;
}

}  // extern "C"
