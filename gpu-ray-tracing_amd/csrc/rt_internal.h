// rt_internal.h — helpers shared by the C-ABI translation units of librt_hip.so
// (rt_abi.cpp, rt_post.cpp, rt_scene_edit.cpp, rt_matte.cpp, rt_comm.cpp, rt_chain.cpp).  Internal; not part of the public
// boundary.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <string>
#include <vector>

#include "rt_abi.h"

struct rt_adaptive_params;  // include/rt_adaptive.h

namespace rti {

// Records `msg` as this thread's rt_last_error() text and returns `s`.
rt_status fail(rt_status s, const std::string& msg);
rt_status hip_fail(hipError_t e, const char* what);
// RT_ERR_INVALID_SIZE unless 1 <= w, h <= 65536.
rt_status check_image(uint32_t w, uint32_t h);
// Whether a parameter is neither negative, NaN nor infinite.
inline bool nonneg_finite(float x) { return x >= 0.0f && x <= FLT_MAX; }
// The HIP device of a context (rt_create's argument).
int ctx_device(const rt_ctx* ctx);
// Drops what the context knows about `image`'s sample counts (the source of the kernels' count
// hint): for a call that leaves per-pixel counts in it.
void forget_count(rt_ctx* ctx, const void* image);
// WGSL u32(f32) on the host (truncate, saturate, NaN -> 0), as rtd::f2u.
inline uint32_t host_f2u(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)f;
}
// The round-robin stripes of rank / nranks as a band set (band b -> rank b mod nranks).
rt_band_set stripe_set(uint32_t h, uint32_t rank, uint32_t nranks);
// A band set the kernels can run: inside the image, step >= 1, and (for two or more bands)
// first and step within the packed stripe map's 16 / 15 bits (rtk::pack_bands).
rt_status check_band_set(uint32_t h, const rt_band_set& bs);
// What rt_update_adaptive, rt_converge_frames and rt_progress_stats refuse of an
// rt_adaptive_params.
rt_status check_adaptive_params(const rt_adaptive_params& params);
// The context's blocks of rt_progress_stats, allocated on first use (the device must be
// current): dev_bytes on the device, host_bytes of pinned host memory.
rt_status progress_blocks(rt_ctx* ctx, size_t dev_bytes, size_t host_bytes, void** dev,
                          void** host);
// The context's scene for an entry point outside rt_abi.cpp: uploads the spheres as every trace
// call does (only when their bytes change; the device must be current) and returns the scan
// records (cx, cy, cz, r*r), zero-padded as the scans expect.  Nothing else of the context changes.
rt_status scene_records(rt_ctx* ctx, const rt_sphere* spheres, uint32_t count, hipStream_t stream,
                        const float4** geom);
// rt_set_scan_mode's value.
int ctx_scan_mode(const rt_ctx* ctx);
// The context's blocks of rt_matte.h, allocated on first use (the device must be current): the
// last call's rt_matte_info on the device, rt_matte_resolve's selection mask (mask_words words)
// and the host copy of the words the device mask holds.
struct MatteBlocks {
    uint32_t* info;
    uint32_t* mask;
    std::vector<uint32_t>* mask_host;
};
rt_status matte_blocks(rt_ctx* ctx, size_t mask_words, MatteBlocks* out);
// Whether nranks band sets cover every band of a height-row image exactly once, each within
// rows_per_rank rows (rt_deinterleave_bands' precondition).
bool band_sets_cover(uint32_t height, uint32_t nranks, const rt_band_set* sets,
                     uint32_t rows_per_rank);

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

namespace rtk {
struct TraceParams;
}

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
