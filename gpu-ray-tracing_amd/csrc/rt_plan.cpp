// rt_plan.cpp — what a trace launch needs decided before it goes out: the kernel instance and
// its parts, the candidate lists, the tile, workgroup and unit orders, the split plan, the sample
// count records with the hint tables, and prepare(), the common setup of every trace launch.
//   prepare_camera_bind_group (lib.rs:151-175) -> camera passed by value as kernarg (fill_camera)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"
#include "rt_internal.h"
#include "rt_kernels.h"

namespace rti {

// Kernel instance for a launch (rtk::kTrace*): without bounce rays (max_depth <= 1) the
// culled mode needs only the candidate lists; the camera-ray-only instance also requires
// camera_rays_bounded (its fast cores).  Bounce rays (max_depth >= 2) run the bounce
// instance, whose path schedule (per wave by default, compacted or frame pairs) is
// rt_set_path_compaction's.
int trace_kernel_for(const rt_ctx* ctx, const rtk::TraceParams& p) {
    if (ctx->scan_mode == RT_SCAN_EXHAUSTIVE) return rtk::kTraceExhaustive;
#ifndef RT_FORCE_CULLED_KERNEL
    if (p.depth <= 1u && camera_rays_bounded(ctx, p)) return rtk::kTraceList;
#endif
#ifndef RT_NO_BOUNCE_KERNEL
    // bounce rays: the bounce instance (path schedule: TraceParams::compact)
    if (p.depth >= 2u) return rtk::kTraceBounce;
#endif
    return rtk::kTraceCulled;
}

// One-frame launches of the camera-ray-only instance run rt_single_kernel (rt_kernels.hip)
// unless rt_set_single_kernel(OFF).
int single_or(const rt_ctx* ctx, const rtk::TraceParams& p, int kernel) {
    if (kernel != rtk::kTraceList || p.frames != 1u || !p.cand ||
        ctx->single_kernel == RT_SINGLE_OFF)
        return kernel;
    if (ctx->single_kernel == RT_SINGLE_PAIR) return rtk::kTraceSingle;
    if (ctx->single_kernel == RT_SINGLE_ONE) return rtk::kTraceSingleOne;
    const uint64_t tiles = launch_tiles(p.width, p.local_bands);
    return tiles <= rtk::kSingleOneMaxTiles ? rtk::kTraceSingleOne : rtk::kTraceSingle;
}

// Frames per rt_update_frames launch (see rt_update_frames): the camera-ray-only and the
// bounce instances fuse frames (both keep the accumulator in registers and store the last
// two frames' images); the others run one frame per launch.
uint32_t frames_per_launch_for(const rt_ctx* ctx, const rtk::TraceParams& p) {
    const int k = trace_kernel_for(ctx, p);
    const bool fusable = k == rtk::kTraceList || k == rtk::kTraceBounce;
    if (!fusable) return 1u;
    if (ctx->frames_per_launch)
        return std::min<uint32_t>(ctx->frames_per_launch, rtk::kMaxFramesPerLaunch);
    return rtk::kHintFrames;
}

// The frame-group instance of a launch whose every frame is hinted (rt_set_frame_pairs, not
// OFF).  AUTO: four waves per tile when the share is small (a few tiles per SIMD), four per
// pair of tiles up to twice that, two per pair above (rt_kernels.h kQuadMaxTiles /
// kQuad2MaxTiles; DESIGN.md §5 "Frame groups over tile pairs").
int frame_group_kernel(const rt_ctx* ctx, const rtk::TraceParams& p) {
    const int mode = ctx->frame_pairs;
    const uint64_t tiles = launch_tiles(p.width, p.local_bands);
    const bool automode = mode == RT_FRAME_PAIRS_AUTO;
    // (the tile-pair instances read the candidate blocks: lists required)
    const bool tpair = p.cand && (mode == RT_FRAME_PAIRS_ON2 || mode == RT_FRAME_PAIRS_QUAD2 ||
                                  (automode && tiles > rtk::kQuadMaxTiles));
    const bool quad = mode == RT_FRAME_PAIRS_QUAD || mode == RT_FRAME_PAIRS_QUAD2 ||
                      (automode && (tiles <= rtk::kQuadMaxTiles ||
                                    (tpair && tiles <= rtk::kQuad2MaxTiles)));
    return quad ? (tpair ? rtk::kTraceListQuad2 : rtk::kTraceListQuad)
                : (tpair ? rtk::kTraceListPair2 : rtk::kTraceListPair);
}

UnitGrid frame_group_units(int kernel, uint32_t w, uint32_t bands) {
    const uint32_t group =
        kernel == rtk::kTraceListQuad2 || kernel == rtk::kTraceListPair2 ? 2u : 1u;
    const uint32_t units_x = (((w + 7u) >> 3) + group - 1u) / group;
    return {group, units_x, (uint64_t)units_x * bands};
}

void free_candidates(rt_ctx* ctx) {
    (void)hipFree(ctx->cand);
    ctx->cand = nullptr;
    ctx->cand_tiles = 0;
    ctx->cand_live = 0;
    ctx->cand_key.clear();
}

// Makes the per-tile candidate lists current for p's camera geometry, image, stripes and
// scene; rebuilds them (one small kernel) only when one of those changed.  The per-frame
// fields (random_seed, camera_has_moved, samples_per_pixel, max_depth) are not part of
// the key: the lists hold for every frame of a camera.
static rt_status ensure_candidates(rt_ctx* ctx, rtk::TraceParams& p, hipStream_t stream) {
    struct Key {
        float center[3], vul[3], pdu[3], pdv[3], ddu[3], ddv[3], defocus;
        uint32_t w, h, first, step, bands, occlusion, certain, tight;
        uint64_t scene;
    } key;
    std::memset(&key, 0, sizeof(key));
    std::memcpy(key.center, p.center, sizeof(key.center));
    std::memcpy(key.vul, p.vul, sizeof(key.vul));
    std::memcpy(key.pdu, p.pdu, sizeof(key.pdu));
    std::memcpy(key.pdv, p.pdv, sizeof(key.pdv));
    std::memcpy(key.ddu, p.ddu, sizeof(key.ddu));
    std::memcpy(key.ddv, p.ddv, sizeof(key.ddv));
    key.defocus = p.defocus_angle;
    key.w = p.width;
    key.h = p.height;
    key.first = p.band_first;
    key.step = p.band_step;
    key.bands = p.local_bands;
    key.scene = ctx->scene_gen;
    // The occlusion rule bounds the f32 roots, so it runs only inside the domain the fast
    // cores are proven for (no overflow or underflow in the root test's intermediates).
    const bool occlusion = ctx->occlusion_cull && ctx->scene_bound <= 0x1p40 &&
                           camera_rays_bounded(ctx, p);
    key.occlusion = occlusion ? 1u : 0u;
    // (certain tiles are a by-product of the occlusion rule's bounds: flagged only where it runs)
    const bool certain = occlusion && ctx->certain_tiles;
    key.certain = certain ? 1u : 0u;
    key.tight = ctx->tight_bundle ? 1u : 0u;
    const unsigned char* kb = reinterpret_cast<const unsigned char*>(&key);
    const uint64_t tiles = launch_tiles(p.width, p.local_bands);
    p.cand_k = rtk::kCandMax;
    if (ctx->cand_key.size() != sizeof(key) ||
        std::memcmp(ctx->cand_key.data(), kb, sizeof(key)) != 0) {
        if (tiles > ctx->cand_tiles) {
            if (ctx->cand_tiles) {
                hipError_t e = hipStreamSynchronize(stream);  // old lists may be in use
                if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
            }
            free_candidates(ctx);
            hipError_t e = hipMalloc(&ctx->cand, tiles * rtk::kCandStride * sizeof(float4));
            if (e != hipSuccess) {
                free_candidates(ctx);
                return hip_fail(e, "hipMalloc(candidate lists)");
            }
            ctx->cand_tiles = tiles;
        }
        hipError_t e = rtk::launch_candidates(p, ctx->cand, occlusion, certain,
                                              ctx->tight_bundle, stream);
        if (e != hipSuccess) return hip_fail(e, "rt_candidates_kernel launch");
        ctx->cand_key.assign(kb, kb + sizeof(key));
        ctx->cand_gen++;
        ctx->cand_live = tiles;
    }
    p.cand = ctx->cand;
    return RT_OK;
}

// Cost-ordered tiles for the camera-ray-only instances: a fused launch of a candidate-list
// generation (same camera geometry, image, stripes and scene) records each tile's
// duration; the next launch of the generation first sorts the tiles by it
// (rtk::launch_tile_order, on the stream) and then starts the costliest tiles first so
// that the cheap ones fill the tail.  The sort runs only when a generation is reused, so a
// camera that moves every call never pays for it.  Only the workgroup -> tile assignment
// changes, never a pixel's result.
rt_status ensure_order_buffers(rt_ctx* ctx, uint64_t tiles, hipStream_t stream) {
    if (tiles <= ctx->order_tiles) return RT_OK;
    if (ctx->order_tiles) {
        hipError_t e = hipStreamSynchronize(stream);   // old order may be in use
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    }
    (void)hipFree(ctx->tile_cost);
    (void)hipFree(ctx->tile_order);
    ctx->tile_cost = ctx->tile_order = nullptr;
    ctx->order_tiles = 0;
    ctx->cost_gen = ctx->order_gen = ~0ull;
    ctx->chain_raster_key[0] = 0;
    hipError_t e = hipMalloc(&ctx->tile_cost, tiles * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&ctx->tile_order, 3 * tiles * sizeof(uint32_t));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(tile order)");
    ctx->order_tiles = tiles;
    return RT_OK;
}

rt_status plan_tile_order(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream) {
    p.tile_order = nullptr;
    p.tile_cost = nullptr;
    // (single-frame launches keep raster order: their accumulator traffic is a large part
    // of the frame, and scattered tiles cost more in HBM than the tail they save)
    const bool bounce = kernel == rtk::kTraceBounce;
    if (!(rtk::trace_ordered(kernel) || bounce) || ctx->tile_order_mode == RT_TILE_ORDER_OFF ||
        p.cand_k == 0 || p.frames < 2)
        return RT_OK;
    // scheduling units: 8x8 tiles, the compacting bounce instance's workgroups of
    // kBounceWaves tiles or rt_tpair_kernel's tile pairs (costs measured in another unit are
    // discarded)
    const uint32_t group = (bounce && p.compact == 1u)         ? rtk::kBounceWaves
                           : (kernel == rtk::kTraceListQuad2 ||
                              kernel == rtk::kTraceListPair2) ? 2u
                                                            : 1u;
    if (ctx->cost_group != group) {
        ctx->cost_gen = ctx->order_gen = ~0ull;
        ctx->cost_group = group;
    }
    const uint64_t gen = ctx->cand_gen;
    const uint32_t tiles_x0 = (p.width + 7u) >> 3;
    const uint32_t tiles_x = (tiles_x0 + group - 1u) / group;
    const uint64_t tiles = (uint64_t)tiles_x * p.local_bands;
    if (rt_status s = ensure_order_buffers(ctx, tiles, stream)) return s;
    // the order from the newest measurement of this generation
    if (ctx->cost_gen == gen && (ctx->order_gen != gen || ctx->order_frames < ctx->cost_frames)) {
        hipError_t e = rtk::launch_tile_order(ctx->tile_cost, ctx->tile_order,
                                              (uint32_t)tiles, tiles_x, stream, 1u,
                                              ctx->tile_order + ctx->order_tiles, 2u);
        if (e != hipSuccess) return hip_fail(e, "rt_tile_order_kernel launch");
        ctx->order_gen = gen;
        ctx->order_frames = ctx->cost_frames;
    }
    const bool have = ctx->order_gen == gen;
    if (have) p.tile_order = ctx->tile_order;
    // A launch of a few frames measures mostly start-up and placement noise: launches keep
    // re-measuring (in the current order) until one of kOrderFrames frames or more has.
    constexpr uint32_t kOrderFrames = 16;
    if (have && ctx->order_frames >= std::min(kOrderFrames, p.frames)) return RT_OK;
    p.tile_cost = ctx->tile_cost;
    return RT_OK;
}

// Dispatch order of one-frame launches (rt_single_kernel): the workgroups of the current
// candidate generation by decreasing candidate-list load, costliest first (scheduling only;
// rtk::launch_wg_order).  Built on the second launch of a generation (a camera that moves
// every frame never pays for it); rt_set_tile_order(OFF) keeps raster order.
rt_status plan_wg_order(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream) {
    const uint32_t parts = p.parts > 1u ? p.parts : 1u;
    p.wg_order = nullptr;
    if ((kernel != rtk::kTraceSingle && kernel != rtk::kTraceSingleOne) || p.cand_k == 0 ||
        p.local_bands < 2 || ctx->tile_order_mode == RT_TILE_ORDER_OFF)
        return RT_OK;
    const uint64_t gen = ctx->cand_gen;
    if (ctx->band_gen != gen) {
        if (ctx->band_seen_gen != gen) {        // first launch of this generation
            ctx->band_seen_gen = gen;
            return RT_OK;
        }
        ctx->band_gen = gen;
        ctx->wg_pix = 0;
        ctx->wg_parts = 0;
    }
    const uint32_t pix = kernel == rtk::kTraceSingle ? rtk::single_pix() : 1u;
    const uint32_t per = rtk::single_wg_tiles(pix);
    const uint64_t units = (uint64_t)((((p.width + 7u) >> 3) + per - 1u) / per) * p.local_bands;
    if (units > ctx->wg_cap) {
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        (void)hipFree(ctx->wg_buf);
        ctx->wg_buf = nullptr;
        ctx->wg_cap = 0;
        e = hipMalloc(&ctx->wg_buf, (2 * units + 1) * sizeof(uint32_t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(workgroup order)");
        ctx->wg_cap = units;
        ctx->wg_pix = 0;
    }
    if (ctx->wg_pix != pix || ctx->wg_parts != parts) {
        hipError_t e = rtk::launch_wg_order(p.cand, (p.width + 7u) >> 3, p.local_bands, pix,
                                            ctx->wg_buf, ctx->wg_buf + units, stream, parts);
        if (e != hipSuccess) return hip_fail(e, "workgroup order launch");
        ctx->wg_pix = pix;
        ctx->wg_parts = parts;
        ctx->wg_builds++;
    }
    p.wg_order = ctx->wg_buf + units;
    return RT_OK;
}

// Split bounce launches (rt_kernels.hip kBounceSplit; RT_PATHS_SPLIT, or AUTO for small
// launches): each tile's frames in S chunks traced by separate waves.  A share of a few
// waves per SIMD in per-wave mode ends with SIMDs idle behind its costliest tiles' 64-frame
// chains (an 8-rank K5 share's longest waves last 0.91-1.0 of the launch, 4.75
// waves resident per SIMD on average); S times as many, S times shorter waves keep them
// busy to the end.  S = 4 up to kSplit4MaxTiles tiles per launch, 2 up to kSplit2MaxTiles,
// else 1 (per wave; RT_PATHS_SPLIT forces at least 2); never more chunks than frames.
// RT_BOUNCE_SPLIT (environment, diagnostic) overrides S.  With a measured tile order only the
// costliest tiles split (the unit order below).  Measured (tools/k5_ab.py, 64-frame K5
// launches, the modes interleaved launch by launch): every tile split, first build
// (profiles/r04/k5_ab_r04e.jsonl): 8-rank share per wave 4 635 µs, S = 2 4 422, S = 4 4 821,
// S = 8 4 970; 4-rank per wave 8 010, S = 2 8 388 — the chunks' hand-off traffic, merges and
// extra wave starts cost more than the shorter tail saves.  The unit order
// (profiles/r04/r04l_k5_unit_order.jsonl, 7 launches each): 8-rank share per wave 4 593, every
// tile in 2 chunks 4 447, the unit order with S = 4 and alpha 0.25 4 253 (0.879 of the 1-GPU
// per-wave rate); 4-rank per wave 7 896 against 8 008, whole image 29 911 against 30 185 — so
// AUTO splits (S = 4, unit order) shares of at most 20 000 tiles and runs larger ones per wave.
// Against S = 8 and other alphas (profiles/r04/r04e2_k5_chunks_alpha.jsonl, 8-rank share):
// AUTO 4 248, S = 8 alpha 0.25 / 0.5 4 318 / 4 391, S = 4 alpha 0.125 / 0.5 4 686 / 4 264.
#ifndef RT_SPLIT4_MAX_TILES
#define RT_SPLIT4_MAX_TILES 20000
#endif
#ifndef RT_SPLIT2_MAX_TILES
#define RT_SPLIT2_MAX_TILES 20000
#endif
constexpr uint64_t kSplit4MaxTiles = RT_SPLIT4_MAX_TILES, kSplit2MaxTiles = RT_SPLIT2_MAX_TILES;
// Only the costliest tiles split: the first ceil(tiles * kSplitFrac) slots of the cost order
// (a launch without an order: its first slots in raster order).  RT_SPLIT_FRAC (environment,
// diagnostic) overrides the fraction.
#ifndef RT_SPLIT_FRAC
#define RT_SPLIT_FRAC 1.0
#endif
// alpha: a tile splits when its recorded cost exceeds alpha times the launch's ideal span
// (the sum of all costs over the device's resident waves); 0.25 measured best with S = 4
#ifndef RT_SPLIT_ALPHA
#define RT_SPLIT_ALPHA 0.25
#endif
// The bounce instance's table of scatter random numbers (TraceParams::hint_rs_dev) for the
// hinted frames of a launch: the context's buffer, filled on the stream by launch_bounce.
rt_status plan_hint_rs(rt_ctx* ctx, rtk::TraceParams& p, int kernel) {
    p.hint_rs_dev = nullptr;
    p.hint_rs_dev_frames = 0;
    if (kernel != rtk::kTraceBounce || p.hint_acc_frames == 0 || p.depth == 0 ||
        p.depth > rtk::kHintRsDepth)
        return RT_OK;
    if (!ctx->d_hint_rs) {
        const hipError_t e = hipMalloc(&ctx->d_hint_rs, sizeof(float4) * rtk::kHintFrames *
                                                            rtk::kHintRsDepth);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(hint table)");
    }
    p.hint_rs_dev = ctx->d_hint_rs;
    p.hint_rs_dev_frames = p.hint_acc_frames;
    return RT_OK;
}

rt_status plan_split(rt_ctx* ctx, rtk::TraceParams& p, int kernel, hipStream_t stream) {
    p.split = 1;
    p.split_tiles = 0;
    p.unit_order = nullptr;
    p.unit_count = nullptr;
    p.split_col = nullptr;
    p.split_cnt = nullptr;
    const int mode = ctx->path_compaction;
    if (kernel != rtk::kTraceBounce || (mode != RT_PATHS_AUTO && mode != RT_PATHS_SPLIT))
        return RT_OK;
    const uint64_t tiles = launch_tiles(p.width, p.local_bands);
    uint32_t S = tiles <= kSplit4MaxTiles ? 4u : tiles <= kSplit2MaxTiles ? 2u : 1u;
    if (mode == RT_PATHS_SPLIT) S = std::max(S, 2u);
    if (const char* e = std::getenv("RT_BOUNCE_SPLIT")) S = (uint32_t)std::max(1L, std::atol(e));
    S = std::min(std::min(S, p.frames), 8u);   // a unit-order entry holds chunks 0-7
    // a power of two: rt_unit_order_kernel moves a split tile's cost bucket by 4·log2 S
    // places (cost / S), and launches of 3, 5, 6 or 7 frames would otherwise give S = 3..7
    while (S & (S - 1u)) S &= S - 1u;
    // AUTO splits only with a measured order (the unit order below): a launch without one runs
    // per wave, so the costs it records are whole tiles', not a chunk's scaled by S
    if (mode == RT_PATHS_AUTO && !p.tile_order && !std::getenv("RT_SPLIT_FRAC")) S = 1u;
    if (S <= 1u || tiles == 0) {
        p.compact = 0u;
        return RT_OK;
    }
    const uint64_t bytes = tiles * p.frames * 1024ull;
    if (bytes > ctx->split_col_bytes || tiles > ctx->split_cnt_tiles) {
        hipError_t e = hipStreamSynchronize(stream);    // the old buffers may be in use
        if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
        if (bytes > ctx->split_col_bytes) {
            (void)hipFree(ctx->split_col);
            ctx->split_col = nullptr;
            ctx->split_col_bytes = 0;
            e = hipMalloc(&ctx->split_col, bytes);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(split colours)");
            ctx->split_col_bytes = bytes;
        }
        if (tiles > ctx->split_cnt_tiles) {
            (void)hipFree(ctx->split_cnt);
            ctx->split_cnt = nullptr;
            ctx->split_cnt_tiles = 0;
            e = hipMalloc(&ctx->split_cnt, tiles * sizeof(uint32_t));
            // (zero once: every launch leaves the arrival counters at zero)
            if (e == hipSuccess) e = hipMemsetAsync(ctx->split_cnt, 0, tiles * sizeof(uint32_t), stream);
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(split counters)");
            ctx->split_cnt_tiles = tiles;
        }
    }
    // With a measured tile order: the unit order (longest-processing-time-first over the
    // units; tiles above alpha times the launch's ideal span split).  RT_SPLIT_FRAC (the
    // first fraction of the tile order splits, no unit order) and RT_SPLIT_ALPHA: diagnostic.
    const char* frac_env = std::getenv("RT_SPLIT_FRAC");
    if (p.tile_order && !frac_env && p.local_bands < 4096u && ((p.width + 7u) >> 3) < 65536u) {
        double alpha = RT_SPLIT_ALPHA;
        if (const char* e = std::getenv("RT_SPLIT_ALPHA")) alpha = std::atof(e);
        const uint64_t cap = tiles * S;
        if (cap + 1 > ctx->unit_cap) {
            hipError_t e = hipStreamSynchronize(stream);   // the old order may be in use
            if (e == hipSuccess) {
                (void)hipFree(ctx->unit_order);
                ctx->unit_order = nullptr;
                ctx->unit_cap = 0;
                e = hipMalloc(&ctx->unit_order, (cap + 1) * sizeof(uint32_t));
            }
            if (e != hipSuccess) return hip_fail(e, "hipMalloc(unit order)");
            ctx->unit_cap = cap + 1;
            ctx->unit_key[0] = ~0ull;
        }
        // (resident waves of the launch: every SIMD of the context's device at 8 waves)
        if (ctx->cus == 0) {
            int n = 0;
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) !=
                    hipSuccess || n <= 0)
                n = 256;
            ctx->cus = n;
        }
        const int cus = ctx->cus;
        const float k_thr = (float)(alpha / (cus * 4.0 * 8.0));
        uint32_t kbits;
        std::memcpy(&kbits, &k_thr, 4);
        const uint64_t key[5] = {ctx->order_gen, ctx->order_frames, tiles, S, kbits};
        if (!std::equal(key, key + 5, ctx->unit_key)) {
            hipError_t e = rtk::launch_unit_order(ctx->tile_cost, ctx->unit_order,
                                                  ctx->unit_order + cap, (uint32_t)tiles,
                                                  (p.width + 7u) >> 3, S, k_thr, stream);
            if (e != hipSuccess) return hip_fail(e, "rt_unit_order_kernel launch");
            std::copy(key, key + 5, ctx->unit_key);
        }
        p.compact = 3u;
        p.split = S;
        p.split_tiles = 0;
        p.split_col = ctx->split_col;
        p.split_cnt = ctx->split_cnt;
        p.unit_order = ctx->unit_order;
        p.unit_count = ctx->unit_order + cap;
        return RT_OK;
    }
    double frac = RT_SPLIT_FRAC;
    if (frac_env) frac = std::atof(frac_env);
    const uint64_t st = std::min<uint64_t>(tiles, (uint64_t)std::ceil(tiles * std::max(0.0, frac)));
    if (st == 0) {
        p.compact = 0u;
        return RT_OK;
    }
    p.compact = 3u;
    p.split = S;
    p.split_tiles = (uint32_t)st;
    p.split_col = ctx->split_col;
    p.split_cnt = ctx->split_cnt;
    return RT_OK;
}

// After a launch that recorded tile costs.
void finish_tile_order(rt_ctx* ctx, const rtk::TraceParams& p) {
    if (!p.tile_cost) return;
    ctx->cost_gen = ctx->cand_gen;
    ctx->cost_frames = p.frames;
    const uint32_t key[6] = {p.width, p.height, p.band_first, p.band_step, p.local_bands,
                             ctx->cost_group};
    std::copy(key, key + 6, ctx->cost_key);
    ctx->cost_key_ok = true;
}

// Per-column / per-row halves of the pixel-invariant seed hash (wgsl:309-310), built on
// the host once per image size: one buffer, hash(x*73) for x < rtk::hy_offset(w), then
// hash(y*51) for y < h (the trace kernel derives the row table from the column table's
// pointer and the width: one preloaded pointer for both).
static rt_status ensure_hash_tables(rt_ctx* ctx, uint32_t w, uint32_t h,
                                    hipStream_t stream) {
    const uint32_t xpad = rtk::hy_offset(w);
    if (ctx->d_hx && ctx->hx_len == xpad && ctx->hy_len >= h) return RT_OK;
    const uint32_t ylen = std::max(h, ctx->hx_len == xpad ? ctx->hy_len : 0u);
    std::vector<uint32_t> v((size_t)xpad + ylen);
    for (uint32_t i = 0; i < xpad; ++i) v[i] = rtd::hash(i * 73u);
    for (uint32_t i = 0; i < ylen; ++i) v[xpad + i] = rtd::hash(i * 51u);
    uint32_t* d = nullptr;
    hipError_t e = hipMalloc(&d, v.size() * sizeof(uint32_t));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(hash table)");
    e = hipMemcpyAsync(d, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // also retires old readers
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemcpyAsync(hash table)");
    }
    (void)hipFree(ctx->d_hx);
    ctx->d_hx = d;
    ctx->hx_len = xpad;
    ctx->hy_len = ylen;
    return RT_OK;
}

// ---- sample-count hints (TraceParams::hint_n) ------------------------------------------
bool lookup_count(const rt_ctx* ctx, const void* image, const rtk::TraceParams& p,
                  uint32_t& n) {
    for (const rt_ctx::CountRecord& r : ctx->counts)
        if (r.image == image && r.w == p.width && r.h == p.height && r.first == p.band_first &&
            r.step == p.band_step && r.bands == p.local_bands) {
            n = r.n;
            return true;
        }
    return false;
}

void record_count(rt_ctx* ctx, const void* image, const rtk::TraceParams& p, uint32_t n) {
    forget_count(ctx, image);
    if (ctx->counts.size() >= 16) ctx->counts.erase(ctx->counts.begin());
    ctx->counts.push_back({image, p.width, p.height, p.band_first, p.band_step, p.local_bands, n});
}

void forget_count(rt_ctx* ctx, const void* image) {
    for (size_t i = 0; i < ctx->counts.size(); ++i)
        if (ctx->counts[i].image == image) {
            ctx->counts.erase(ctx->counts.begin() + (long)i);
            return;
        }
}

// The count a pixel holds after frame f of the kernel's loop, given the count before it
// (wgsl:352-362, including the f32 round trip of the stored count).
uint32_t next_count(uint32_t n, uint32_t spp) {
    return host_f2u((float)(n < spp ? n + 1u : n));
}

// Fills p.hint_* for a launch whose input pixels all hold count n_in (frame 0 of a reset
// launch: 0) and returns the count every pixel holds after the launch.
uint32_t fill_hint(rtk::TraceParams& p, uint32_t n_in) {
    const uint32_t spp = p.spp, depth = p.depth;
    const uint32_t af = std::min<uint32_t>(p.frames, rtk::kHintFrames);
    uint32_t hf = af;
    if (depth > 0) hf = std::min<uint32_t>(hf, rtk::kHintEntries / depth);
    p.hint_frames = hf;
    p.hint_acc_frames = af;
    uint32_t n = n_in;
    for (uint32_t f = 0; f < p.frames; ++f) {
        if (f < af) {
            p.hint_n[f] = n;
            // RN32(1 / f32(n + 1)) (exact integer for n + 1 <= 2^24, where the kernels use it)
            p.hint_rcp[f] = 1.0f / (float)(n + 1u);
            p.hint_cnt[f] = (float)(n < spp ? n + 1u : n);
        }
        if (f < hf) {
            const uint32_t B = p.seed_b[f];
            for (uint32_t i = 0; i < depth; ++i) {
                // wgsl:268 with seed + 1 = n + B + 2 (wgsl:353, 358)
                const uint32_t sb = rtd::hash(n + B + 2u + i * 1000u);
                const float r_sb = rtd::rf(sb);
                const rtd::v3 u = rtd::random_unit_vector(r_sb, sb);
                p.hint_rs[f * depth + i] = make_float4(r_sb, u.x, u.y, u.z);
            }
        }
        n = next_count(n, spp);
    }
    return n;
}

// Sets the hint of one launch from what the context knows about `in` and records the
// count of `out` afterwards (or forgets it when unknown).
void plan_hint(rt_ctx* ctx, rtk::TraceParams& p, const void* in, const void* out) {
    uint32_t n_in = 0;
    const bool known = p.reset_first || lookup_count(ctx, in, p, n_in);
    if (!known) {
        p.hint_frames = 0;
        p.hint_acc_frames = 0;
        forget_count(ctx, out);
        return;
    }
    record_count(ctx, out, p, fill_hint(p, p.reset_first ? 0u : n_in));
}

void fill_camera(rtk::TraceParams& p, const rt_scene_camera& c) {
    fill_camera_grid(p, c);
    fill_camera_lens(p, c);
    p.depth = host_f2u(c.max_depth);
    p.spp = host_f2u(c.samples_per_pixel);
}

// Common setup of every trace launch: argument checks, scene upload, kernel parameters
// (camera, stripe map, scan-mode data such as the candidate lists).
rt_status prepare(rt_ctx* ctx, const void* in, const void* out, uint32_t w, uint32_t h,
                  const rt_band_set& bs, const rt_scene_camera* cam,
                  const rt_sphere* spheres, uint32_t count, const float* seeds,
                  hipStream_t stream, rtk::TraceParams& p) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!in || !out || !cam) return fail(RT_ERR_INVALID_ARGUMENT, "NULL image or camera");
    if (rt_status s = check_image(w, h)) return s;
    if (rt_status s = check_band_set(h, bs)) return s;
    if (!seeds) return fail(RT_ERR_INVALID_ARGUMENT, "random_seeds is NULL");
    if (rt_status s = upload_spheres(ctx, spheres, count, stream)) return s;

    std::memset(&p, 0, sizeof(p));
    p.geom = ctx->d_geom;
    p.sph = ctx->d_sph;
    p.width = w;
    p.height = h;
    p.count = count;
    p.normal_rn = ctx->normal_rn ? 1u : 0u;
    p.roots_fast = ctx->scene_bound <= 0x1p40 ? 1u : 0u;
    p.band_first = bs.first;
    p.band_step = bs.step;
    p.local_bands = bs.count;
    fill_camera(p, *cam);
    // bounce instance mode (rt_kernels.hip rt_bounce_kernel: 0 per wave, 1 compact, 2 pairs)
    p.compact = ctx->path_compaction == RT_PATHS_COMPACT ? 1u
                : ctx->path_compaction == RT_PATHS_PAIR  ? 2u
                                                         : 0u;
    if (rt_status s = ensure_hash_tables(ctx, w, h, stream)) return s;
    p.hx = ctx->d_hx;
    p.hy = ctx->d_hx + rtk::hy_offset(w);
    if (ctx->scan_mode == RT_SCAN_CULLED) {
        // Camera rays use the per-tile candidate lists; the LDS copy of the records only
        // serves the per-wave cone culling of bounce rays, so it is skipped at depth <= 1
        // (tiles without a list then read the records from L2).
        const uint32_t padded = (count + 63u) & ~63u;   // <= count + 63 < count + kScanPad
        const bool bounces = cam->max_depth >= 2.0f;
        // (the per-wave bounce instance runs one-wave workgroups: no LDS copy, which each
        // of them would stage)
        p.lds_records = (bounces && padded <= rtk::kLdsMaxRecords &&
                         ctx->path_compaction == RT_PATHS_COMPACT)
                            ? padded
                            : 0u;
        if (rt_status s = ensure_candidates(ctx, p, stream)) return s;
        if (bounces && ctx->grid.nx) {
            const rt_ctx::Grid& g = ctx->grid;
            const unsigned char* base = static_cast<const unsigned char*>(ctx->d_grid);
            const size_t cells = (size_t)g.nx * g.nz;
            p.grid_cells = reinterpret_cast<const uint2*>(base);
            const size_t geom_off = (cells * 8 + 15) & ~(size_t)15;     // as build_grid
            p.grid_geom = reinterpret_cast<const float4*>(base + geom_off);
            p.grid_items = reinterpret_cast<const uint32_t*>(base + geom_off + g.items * 16ull);
            p.grid_big = p.grid_items + g.items;
            p.grid_nx = g.nx;
            p.grid_nz = g.nz;
            p.grid_nbig = g.nbig;
            p.grid_x0 = g.x0;
            p.grid_z0 = g.z0;
            p.grid_s = g.s;
            p.grid_inv_s = g.inv_s;
            p.grid_ylo = g.ylo;
            p.grid_yhi = g.yhi;
            p.grid_cx = g.cx;
            p.grid_cy = g.cy;
            p.grid_cz = g.cz;
            p.grid_reach = g.reach;
            p.grid_m = g.m;
            p.grid_e = g.e;
        }
    }
    return RT_OK;
}

// Concurrent parts of a one-frame update (rt_set_update_queues).  AUTO by the launch's
// tiles (profiles/r03/r03e_ab_queues.log, r03/r03e_rank_sim_k3_q*.jsonl; µs per K3 update at 1 / 2
// / 3 / 4 parts: whole image 22.7 / 19.6 / 19.6 / 19.0, K2 15.9 / 13.6 / 13.5 / 13.5; a
// 2-rank share 12.5 / 11.4 / 11.5; 4-rank 7.8 / 7.5 / 9.7; 8-rank 5.9 / 7.9 / 10.9): each
// part costs the host one more launch (2.7-4.4 µs each on the boxes measured,
// profiles/r03/r03g_launch_rate.jsonl, r03/r03h_launch_rate.jsonl), which small shares cannot hide,
// and a slow host turns 4 parts into a host-bound chain (the driver's 20-step command:
// 72-77 G rays/s at 4 parts, 87-90 at 2, 81-85 at 1, profiles/r03/r03h_bench_driver_q*.json).
constexpr uint64_t kQueues4MinTiles = ~0ull, kQueues2MinTiles = 12000;
uint32_t update_parts(const rt_ctx* ctx, const rtk::TraceParams& p, int kernel) {
    if ((kernel != rtk::kTraceSingle && kernel != rtk::kTraceSingleOne) || p.frames != 1u)
        return 1u;
    uint32_t q = ctx->update_queues;
    if (q == 0) {
        const uint64_t tiles = launch_tiles(p.width, p.local_bands);
        q = tiles >= kQueues4MinTiles ? 4u : tiles >= kQueues2MinTiles ? 2u : 1u;
    }
    return std::max(1u, std::min(q, p.local_bands));
}

// Parts of a one-frame update submitted as AQL packets: a packet costs the host ≈0.25 µs
// (profiles/r03/r03r_aql_probe.txt), so the host never bounds the parts; but four HSA queues
// beside HIP's own measured 38.7 µs per K3 update against 20.4 with two
// (profiles/r03/r03s_ab_aql_nckarg.log): AUTO takes 2 from 2 000 tiles, else 1
// (rt_set_update_queues overrides).
constexpr uint64_t kAqlQueues4MinTiles = ~0ull, kAqlQueues2MinTiles = 2000;
uint32_t update_parts_aql(const rt_ctx* ctx, const rtk::TraceParams& p) {
    uint32_t q = ctx->update_queues;
    if (q == 0) {
        const uint64_t tiles = launch_tiles(p.width, p.local_bands);
        q = tiles >= kAqlQueues4MinTiles ? 4u : tiles >= kAqlQueues2MinTiles ? 2u : 1u;
    }
    return std::max(1u, std::min(q, p.local_bands));
}

}  // namespace rti
