// rt_context.h — struct rt_ctx, the context every C-ABI unit of librt_hip.so works on (included
// through rt_internal.h).  Plain data: each field belongs to the unit its comment names.
#pragma once

#include <hip/hip_runtime_api.h>

#include <vector>

#include "rt_abi.h"

namespace rtc {
struct Chain;
}

struct rt_ctx {
    int device = 0;                  // the HIP device (rt_create's argument)
    int scan_mode = RT_SCAN_CULLED;  // rt_set_scan_mode's value
    float4* d_geom = nullptr;  // count x (cx, cy, cz, r*r)
    float4* d_sph = nullptr;   // count x 2 float4 (the 32-B GpuSphere records)
    uint32_t capacity = 0;
    uint32_t count = 0;
    bool valid = false;
    std::vector<rt_sphere> cached;  // bytes currently on the device
    uint64_t scene_gen = 0;         // bumped on every sphere upload
    // max over spheres of |C| + |R| (inf if any value is not finite) and whether every
    // |R| lies in [2^-20, 2^20]: the scene half of camera_rays_bounded
    double scene_bound = 0.0;
    bool radii_ok = true;
    // one Markstein step from rcp_refined(R) is the IEEE division by every distinct radius
    // (rt_rcp_check_kernel, exhaustive over the numerators; TraceParams::normal_rn)
    bool normal_rn = false;
    uint32_t* d_flag = nullptr;     // the check's result word, then up to kRcpRadii radii
    float4* d_hint_rs = nullptr;    // TraceParams::hint_rs_dev (plan_hint_rs)
    // XZ grid of the small spheres for bounce rays (build_grid; TraceParams
    // grid_*): device arrays and the parameters copied into every launch.
    void* d_grid = nullptr;  // cell ranges (uint2), item records (float4), item indices, big list
    struct Grid {
        uint32_t nx = 0, nz = 0, nbig = 0, items = 0;
        float x0, z0, s, inv_s, ylo, yhi, cx, cy, cz, reach, m, e;
    } grid;
    // Per-tile candidate lists of camera rays (culled scan), valid for cand_key.
    float4* cand = nullptr;   // [tile][rtk::kCandStride] candidate blocks
    // workgroup order of one-frame launches (rtk::launch_wg_order), for candidate generation
    // band_gen; built when a generation is used a second time (a camera that moves every
    // frame never pays for it)
    uint32_t* wg_buf = nullptr;      // cost + order words
    uint64_t wg_cap = 0;
    uint32_t wg_pix = 0;
    uint32_t wg_parts = 0;           // sub-lists the order was dealt into
    uint64_t wg_builds = 0;          // order launches so far (a new order needs a new fork)
    uint64_t band_gen = ~0ull, band_seen_gen = ~0ull;
    uint64_t cand_tiles = 0;        // allocated tiles
    uint64_t cand_live = 0;         // tiles of the current lists
    std::vector<unsigned char> cand_key;
    uint64_t cand_gen = 0;          // bumped whenever the lists are rebuilt
    // rt_set_occlusion_cull: the list build also drops the entries another entry hides from
    // every camera ray of the tile (part of cand_key, with the proofs it needs)
    bool occlusion_cull = true;
    // rt_set_certain_tiles: where the occlusion rule runs, the list build also flags the
    // certain tiles for the pair frame loops (part of cand_key)
    bool certain_tiles = true;
    // rt_set_tight_bundle: the lists are built against the two-slope beam of a tile's camera
    // rays, else against the single cone (part of cand_key)
    bool tight_bundle = true;
    // the last tile-pair launch, for rt_certain_tiles_stats: the lists' generation it read,
    // its tiles per row and its local bands (pair_gen ~0: none yet)
    uint64_t pair_gen = ~0ull;
    uint32_t pair_tiles_x = 0, pair_bands = 0;
    // Cost-ordered tiles (TraceParams::tile_order): per-tile durations recorded by the
    // first camera-ray-only launch of a list generation, and the order derived from them.
    uint32_t* tile_cost = nullptr;
    // order_tiles entries, then the same order dealt into the two chain parts' sub-lists
    // (rt_set_chain_parts), then the raster order dealt the same way (chain_raster_key)
    uint32_t* tile_order = nullptr;
    uint64_t order_tiles = 0;       // allocated tiles
    uint64_t chain_raster_key[2] = {0, 0};   // units, units per band row of the raster table
    uint64_t cost_gen = ~0ull;      // cand_gen tile_cost was measured for
    uint32_t cost_frames = 0;       // frames of the launch that measured it
    uint64_t order_gen = ~0ull;     // cand_gen tile_order was derived for
    uint32_t order_frames = 0;      // frames of the measurement it came from
    uint32_t cost_group = 1;        // tiles per tile_cost/tile_order unit (bounce workgroups, pairs)
    // the share the last cost-recording launch ran (rt_band_costs): width, height, band
    // first, step, count, unit group; valid when cost_key_ok
    uint32_t cost_key[6] = {};
    bool cost_key_ok = false;
    // rt_deinterleave_bands' per-band source table on the device, and its host copy
    uint32_t* d_band_src = nullptr;
    std::vector<uint32_t> band_src;
    int tile_order_mode = RT_TILE_ORDER_AUTO;
    float* d_srgb = nullptr;  // rt_srgb_thresholds table on the device (256 floats)
    // hash(x*73) for x < hx_len (= rtk::hy_offset(width)), then hash(y*51) for y < hy_len
    // (wgsl:309-310), one buffer
    uint32_t* d_hx = nullptr;
    uint32_t hx_len = 0, hy_len = 0;
    // Sample counts of images this context wrote, when every pixel holds the same count:
    // the source of TraceParams::hint_n (a hint only: the kernel verifies it per pixel).
    struct CountRecord {
        const void* image;
        uint32_t w, h, first, step, bands, n;   // the image's size and band set, its count
    };
    std::vector<CountRecord> counts;
    uint32_t frames_per_launch = 0;  // rt_update_frames fusion cap (0 = automatic)
    rt_launch_info last = {0, 0, 0, -1, 0, 0, 0, 1};  // the last call's launches (rt_last_launch_info)
    int path_compaction = RT_PATHS_AUTO;
    int frame_pairs = RT_FRAME_PAIRS_AUTO;
    int single_kernel = RT_SINGLE_AUTO;
    // Concurrent parts of one-frame updates (rt_set_update_queues): part 0 on the caller's
    // stream, part k on aux[k - 1], forked and joined through events.
    uint32_t update_queues = 0;      // 0 = automatic
    // Two staggered parts of a call's fused frame-group launches (rt_set_chain_parts): part 0
    // on the caller's stream, part 1 on aux[0]
    uint32_t chain_parts = 0;        // 0 = automatic
    hipStream_t aux[RT_MAX_UPDATE_QUEUES - 1] = {};
    hipEvent_t fork_ev = nullptr;
    hipEvent_t join_ev[RT_MAX_UPDATE_QUEUES - 1] = {};
    // One-frame updates as AQL packets on the context's own HSA queues (rt_chain.cpp,
    // rt_set_update_submit), created on first use.
    int update_submit = RT_SUBMIT_AUTO;
    rtc::Chain* chain = nullptr;
    bool chain_tried = false;
    bool chain_reported = false;     // a chain failure has been returned to the caller once
    // Images of fused multi-frame launches (rt_set_frame_images): the last two frames' only,
    // or every frame's (TraceParams::store_each 1 / 2)
    int frame_images = RT_FRAME_IMAGES_LAST_TWO;
    // split bounce launches (TraceParams::split_col / split_cnt, plan_split)
    float4* split_col = nullptr;
    uint32_t* split_cnt = nullptr;
    uint64_t split_col_bytes = 0, split_cnt_tiles = 0;
    // their unit order (launch_unit_order) and its count, rebuilt when unit_key changes
    uint32_t* unit_order = nullptr;     // unit_cap entries, then the count
    uint64_t unit_cap = 0;
    uint64_t unit_key[5] = {~0ull, 0, 0, 0, 0};
    int cus = 0;                        // compute units of `device` (0: not queried yet)
    // rt_set_launch_timing: events the fused launches of each call carry, and how many
    // launches the last call timed
    hipEvent_t time_ev[2] = {};
    bool timing = false;
    uint32_t timed_launches = 0;
    // rt_pick's record on the device: four 16-B slots (id, hit, normal, material)
    float4* d_pick = nullptr;
    // rt_progress_stats' blocks (rt_post.cpp progress_blocks): the report and the workgroups'
    // records on the device, the report's pinned landing place on the host
    void* d_progress = nullptr;
    void* h_progress = nullptr;
    // rt_matte.h's blocks (rt_matte.cpp matte_blocks): the last call's info words, then the
    // selection mask of rt_matte_resolve; the words the device mask holds
    uint32_t* d_matte = nullptr;
    size_t matte_mask_words = 0;
    std::vector<uint32_t> matte_mask;
};
