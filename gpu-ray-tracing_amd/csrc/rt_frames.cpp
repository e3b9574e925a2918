// rt_frames.cpp — C-ABI entry points of the render calls (rt_update, rt_render,
// rt_render_stripes, rt_update_frames) and what carries their launches: the context's aux
// streams with their fork and join, the glue around the AQL chain (rt_chain.cpp), the chain
// parts' schedule, and update_frames, the host function the benchmark times.
//   ComputeShaderNode::run (lib.rs:379-421) -> rt_update launches
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt_chain_parts.h"
#include "rt_internal.h"
#include "rt_kernels.h"
#ifdef RT_CALL_STAMPS
// (diagnostic builds: host time stamps of rt_update_frames' phases, one stderr line per call)
#include <chrono>
static thread_local unsigned long long g_call_stamp[8];
static void call_stamp(int i) {
    g_call_stamp[i] = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now().time_since_epoch())
                          .count();
}
#define CALL_STAMP(i) call_stamp(i)
#else
#define CALL_STAMP(i) ((void)0)
#endif

// A chain failure (a go wait that gave up, so a segment's frames were dropped; a queue
// error; a segment that did not complete in time) is returned once, by the context's next
// call (rt_update_frames, rt_destroy, rt_update_submit_status); the context runs HIP launches
// from then on.  No synchronisation: the flags live in host memory.
rt_status rti::chain_report(rt_ctx* ctx) {
    if (!ctx->chain || ctx->chain_reported || !rtc::chain_failed(ctx->chain)) return RT_OK;
    ctx->chain_reported = true;
    const char* why = "";
    (void)rtc::chain_ok(ctx->chain, &why);
    return fail(RT_ERR_HIP, std::string("AQL submission failed earlier (") + why +
                                "); the context runs HIP launches from now on");
}

namespace {

using namespace rti;

// The context's extra streams and fork/join events (created on first use, on ctx->device).
rt_status ensure_aux_streams(rt_ctx* ctx, uint32_t n) {
    if (!ctx->fork_ev) {
        hipError_t e = hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags");
    }
    for (uint32_t k = 0; k < n; ++k) {
        if (!ctx->aux[k]) {
            hipError_t e = hipStreamCreateWithFlags(&ctx->aux[k], hipStreamNonBlocking);
            if (e != hipSuccess) return hip_fail(e, "hipStreamCreateWithFlags");
        }
        if (!ctx->join_ev[k]) {
            hipError_t e = hipEventCreateWithFlags(&ctx->join_ev[k], hipEventDisableTiming);
            if (e != hipSuccess) return hip_fail(e, "hipEventCreateWithFlags");
        }
    }
    return RT_OK;
}

// The fork: the aux streams wait for an event recorded on `stream` — unless `stream` has
// nothing left to run (a new call on an idle stream: then everything it was given is complete
// and the aux streams, joined into it at the end of the previous call, are idle too), which
// spares the host the event record and the waits (two HIP calls; the GPU time measured the same
// either way, profiles/r05/r05b_region_k3.jsonl).  *wait_fork: whether the event was recorded.
rt_status fork_if_busy(rt_ctx* ctx, hipStream_t stream, bool* wait_fork) {
    *wait_fork = false;
    if (hipStreamQuery(stream) == hipSuccess) return RT_OK;
    hipError_t e = hipEventRecord(ctx->fork_ev, stream);
    if (e != hipSuccess) return hip_fail(e, "fork (hipEventRecord)");
    *wait_fork = true;
    return RT_OK;
}

// `stream` waits for everything issued on aux[0..n) so far
rt_status join_aux(rt_ctx* ctx, uint32_t n, hipStream_t stream) {
    hipError_t e = hipSuccess;
    for (uint32_t k = 0; e == hipSuccess && k < n; ++k) {
        e = hipEventRecord(ctx->join_ev[k], ctx->aux[k]);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, ctx->join_ev[k], 0);
    }
    return e == hipSuccess ? RT_OK : hip_fail(e, "join (hipEventRecord / hipStreamWaitEvent)");
}

void note_launch(rt_ctx* ctx, const rtk::TraceParams& p, int kernel, uint32_t frames,
                 uint32_t parts = 1u, bool aql = false) {
    ctx->last.launches += parts;
    ctx->last.queues = parts;
    ctx->last.submit = aql ? RT_SUBMIT_AQL : RT_SUBMIT_HIP;
    ctx->last.frames += frames;
    ctx->last.max_frames_per_launch = std::max(ctx->last.max_frames_per_launch, frames);
    ctx->last.normal_rn = p.normal_rn;
    ctx->last.kernel = kernel != rtk::kTraceBounce ? kernel
                       : p.compact == 3u             ? RT_KERNEL_BOUNCE_SPLIT
                                                     : RT_KERNEL_BOUNCE + (int)p.compact;
    if (kernel == rtk::kTraceListPair2 || kernel == rtk::kTraceListQuad2) {
        // (rt_certain_tiles_stats: which lists the last tile-pair launch paired, and how)
        ctx->pair_gen = ctx->cand_gen;
        ctx->pair_tiles_x = (p.width + 7u) >> 3;
        ctx->pair_bands = p.local_bands;
    }
}

// The context's AQL chain if one-frame updates go through it (rt_set_update_submit AQL, or
// AUTO inside [kAqlAutoMinTiles, kAqlAutoMaxTiles) tiles — an empty range since round 4:
// AQL submission is opt-in): created on first use; AQL fails the call with the reason when
// the machine does not offer it, AUTO falls back to HIP launches, and after a chain failure
// every mode runs HIP launches.  Round 3 measured AQL faster only on mid-sized rank shares
// of per-dispatch updates (a 4-rank K3 share 6.76 against 7.54-7.68 µs per update,
// profiles/r03/r03zd_rank_sim_*.jsonl; whole images and 2-rank shares alike either way, 8-rank
// shares slower); rank shares now run fused frame chains in one launch instead
// (rt_set_frame_images), and no multi-GPU record of AQL submission exists.
#ifndef RT_AQL_AUTO_MIN_TILES
#define RT_AQL_AUTO_MIN_TILES 0
#endif
#ifndef RT_AQL_AUTO_MAX_TILES
#define RT_AQL_AUTO_MAX_TILES 0
#endif
constexpr uint64_t kAqlAutoMinTiles = RT_AQL_AUTO_MIN_TILES,
                   kAqlAutoMaxTiles = RT_AQL_AUTO_MAX_TILES;
rt_status usable_chain(rt_ctx* ctx, const rtk::TraceParams& p, rtc::Chain** out) {
    *out = nullptr;
    if (ctx->update_submit == RT_SUBMIT_HIP || ctx->chain_reported) return RT_OK;
    if (ctx->update_submit == RT_SUBMIT_AUTO) {
        const uint64_t tiles = launch_tiles(p.width, p.local_bands);
        if (tiles < kAqlAutoMinTiles || tiles >= kAqlAutoMaxTiles) return RT_OK;
    }
    const bool aql = ctx->update_submit == RT_SUBMIT_AQL;
    if (!ctx->chain_tried) {
        ctx->chain_tried = true;
        rt_status st = RT_OK;
        ctx->chain = rtc::chain_create(ctx->device, &st);
        // (AUTO: a chain that could not be set up leaves the call on HIP launches)
        if (st != RT_OK && aql) return st;
    }
    const char* why = "";
    // AUTO also needs the queues of its parts up front: no failure once frames are packed
    if (rtc::chain_ok(ctx->chain, &why) && (aql || rtc::chain_queues(ctx->chain, 2u))) {
        *out = ctx->chain;
        return RT_OK;
    }
    if (aql) return fail(RT_ERR_HIP, std::string("AQL submission unavailable: ") + why);
    return RT_OK;
}

// Whether plan_wg_order would issue work on the stream or reallocate for this launch (an
// open AQL segment still reads the current order: it is closed first).
bool wg_order_pending(const rt_ctx* ctx, const rtk::TraceParams& p, int kernel) {
    const uint32_t parts = p.parts > 1u ? p.parts : 1u;
    if ((kernel != rtk::kTraceSingle && kernel != rtk::kTraceSingleOne) || p.cand_k == 0 ||
        p.local_bands < 2 || ctx->tile_order_mode == RT_TILE_ORDER_OFF)
        return false;
    const uint64_t gen = ctx->cand_gen;
    if (ctx->band_gen != gen) return ctx->band_seen_gen == gen;   // builds on this launch
    const uint32_t pix = kernel == rtk::kTraceSingle ? rtk::single_pix() : 1u;
    const uint32_t per = rtk::single_wg_tiles(pix);
    const uint64_t units = (uint64_t)((((p.width + 7u) >> 3) + per - 1u) / per) * p.local_bands;
    return units > ctx->wg_cap || ctx->wg_pix != pix || ctx->wg_parts != parts;
}

// Shared body of rt_update / rt_render / rt_render_stripes: `frames` accumulated in
// launches of up to kMaxFramesPerLaunch frames each.
rt_status trace(rt_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                uint32_t rank, uint32_t nranks, const rt_scene_camera* cam,
                const rt_sphere* spheres, uint32_t count, uint32_t frames,
                const float* seeds, void* stream_v) {
    if (frames == 0) return ctx ? RT_OK : fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    if (nranks == 0 || rank >= nranks) return fail(RT_ERR_INVALID_ARGUMENT, "bad rank/nranks");
    rtk::TraceParams p;
    if (rt_status s = prepare(ctx, in, out, w, h, stripe_set(h, rank, nranks), cam, spheres,
                              count, seeds, stream, p))
        return s;
    const float4* src = reinterpret_cast<const float4*>(in);
    float4* dst = reinterpret_cast<float4*>(out);
    ctx->last = {0, 0, 0, -1, 0, 0, 0, 1};
    for (uint32_t f0 = 0; f0 < frames; f0 += rtk::kMaxFramesPerLaunch) {
        const uint32_t nf = std::min<uint32_t>(frames - f0, rtk::kMaxFramesPerLaunch);
        p.in = src;
        p.out = dst;
        p.frames = nf;
        p.reset_first = (f0 == 0 && cam->camera_has_moved > 0.5f) ? 1u : 0u;
        fill_seeds(p.seed_b, seeds + f0, nf);
        plan_hint(ctx, p, src, dst);
        const int kernel = single_or(ctx, p, trace_kernel_for(ctx, p));
        if (rt_status s = plan_tile_order(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_wg_order(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_split(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_hint_rs(ctx, p, kernel)) return s;
        hipError_t e = rtk::launch_trace(p, kernel, stream);
        if (e != hipSuccess) return hip_fail(e, "rt_trace_kernel launch");
        finish_tile_order(ctx, p);
        note_launch(ctx, p, kernel, nf);
        src = dst;  // later launches continue the accumulation in place
    }
    return RT_OK;
}

// ---- chain parts (rt_set_chain_parts) ------------------------------------------------------
// A call of several fused frame-group launches waits, between two launches, for the first to
// drain: its last round of workgroups leaves SIMDs below their resident waves or idle.  The
// frames of a chain depend on each other per pixel only, so the call's scheduling units are
// dealt into two parts, each a chain of launches on its own stream, and the parts' launch
// boundaries are staggered: one part drains while the other is in mid-launch.
//
// The schedule, a pure function of (frames, cap): part 0 cuts at multiples of cap, part 1 at
// its first launch (cap / 2, or 3 cap / 4) + multiples of cap.  Variant kScheduleShortTails ends each part with a short launch
// (cap / 4 and cap / 8 frames: the one drain nothing overlaps is that of the call's last
// launches), variant kSchedulePlain does not.  No launch is above cap or, above a one-launch
// call, below two frames (a one-frame launch is not a frame-group launch); no cut of one part
// is a cut of the other.  frames <= cap, or cap < 4 (no stagger of two frames or more fits):
// the unsplit chain, part 0 only.  Launches in issue order (by first frame, part 0 first).
constexpr int kScheduleShortTails = 1, kSchedulePlain = 2;
// further candidates: part 1 alone ends with a short launch (just under cap / 8, so that its
// cut misses part 0's last); part 1's first launch is 3 cap / 4
constexpr int kScheduleShortTail1 = 3, kScheduleLateStagger = 4, kScheduleVariants = 4;
// Measured (plain bench.py, K3, 200 frames at cap 64, µs per frame, seven interleaved runs
// each, profiles/chain_parts/ab_k3_200_schedules.jsonl): one chain 11.87 (11.85-11.92); short
// tails 64/64/56/16 + 32/64/64/32/8 11.81 (11.71-11.95); plain 64/64/64/8 + 32/64/64/40 11.70
// (11.62-11.75); part 1's short tail 64/64/64/8 + 32/64/64/34/6 11.69 (11.63-11.88); late
// stagger 64/64/64/8 + 48/64/64/24 11.65 (11.62-11.70).  The kernel trace shows why the
// tails do not pay: part 0, issued first, runs ahead (its launches get the larger share of
// the machine), so part 1's last launch runs alone whatever its length, and every extra
// launch costs its workgroups' start.  The late stagger leaves part 1 the shortest last launch
// without an extra one.
constexpr int kScheduleDefault = kScheduleLateStagger;

void unsplit_schedule(uint32_t frames, uint32_t cap, std::vector<rt_chain_launch>& out) {
    out.clear();
    for (uint32_t f = 0; f < frames; f += cap) out.push_back({0u, f, std::min(cap, frames - f)});
}

// one part's launch lengths: `first`, then cap each, then (tail > 0) a last launch of `tail`
bool part_lengths(uint32_t frames, uint32_t cap, uint32_t first, uint32_t tail,
                  std::vector<uint32_t>& len) {
    len.clear();
    if (tail >= frames || first == 0) return false;
    uint32_t body = frames - tail;
    for (uint32_t n = std::min(first, body); body; n = std::min(cap, body)) {
        len.push_back(n);
        body -= n;
    }
    if (tail) len.push_back(tail);
    // a one-frame last launch takes a frame from its predecessor; a one-frame launch before
    // the tail joins the tail
    const size_t k = len.size();
    if (tail && k >= 2 && len[k - 2] == 1u) {
        len[k - 1] += 1u;
        len.erase(len.begin() + (long)(k - 2));
    } else if (k >= 2 && len[k - 1] == 1u) {
        len[k - 2] -= 1u;
        len[k - 1] = 2u;
    }
    for (uint32_t n : len)
        if (n < 2u || n > cap) return false;
    return true;
}

bool staggered_schedule(uint32_t frames, uint32_t cap, int variant,
                        std::vector<rt_chain_launch>& out) {
    // per variant: part 1's first launch, and the parts' last (0: the remainder)
    uint32_t first1 = cap / 2u, tail0 = 0u, tail1 = 0u;
    if (variant == kScheduleShortTails) {
        tail0 = std::max(2u, cap / 4u);
        tail1 = std::max(2u, cap / 8u);
    } else if (variant == kScheduleShortTail1) {
        tail1 = cap >= 32u ? cap / 8u - 2u : 2u;
    } else if (variant == kScheduleLateStagger) {
        first1 = cap - cap / 4u;
    }
    std::vector<uint32_t> len[2];
    if (!part_lengths(frames, cap, cap, tail0, len[0]) ||
        !part_lengths(frames, cap, first1, tail1, len[1]))
        return false;
    if (len[0].size() < 2 || len[1].size() < 2) return false;
    // cuts of part 0 and part 1, merged in issue order; a shared cut rejects the schedule
    out.clear();
    size_t i[2] = {0, 0};
    uint32_t at[2] = {0, 0};
    while (i[0] < len[0].size() || i[1] < len[1].size()) {
        const int k = i[1] >= len[1].size() || (i[0] < len[0].size() && at[0] <= at[1]) ? 0 : 1;
        if (at[0] == at[1] && at[0] != 0u) return false;
        out.push_back({(uint32_t)k, at[k], len[k][i[k]]});
        at[k] += len[k][i[k]++];
    }
    return at[0] == frames && at[1] == frames;
}

void chain_schedule(uint32_t frames, uint32_t cap, int variant, std::vector<rt_chain_launch>& out) {
    cap = std::max(cap, 1u);
    if (variant == 0) variant = kScheduleDefault;
    if (frames > cap && cap >= 4u) {
        if (staggered_schedule(frames, cap, variant, out)) return;
        if (variant != kSchedulePlain && staggered_schedule(frames, cap, kSchedulePlain, out))
            return;
    }
    unsplit_schedule(frames, cap, out);
}

// AUTO's chain parts by tiles per launch.  Measured per size class (K3, 200-frame chain calls
// that write every frame's image, rank 0's share at 1 / 2 / 4 / 8 ranks, µs per frame, one
// chain against two parts, medians of three interleaved processes of five calls each,
// profiles/chain_parts/rank_sim_cp*.jsonl): 32 400 tiles 11.89-11.97 against 11.58-11.65,
// 16 320 tiles 6.24-6.33 against 6.09-6.14, 8 160 tiles 3.36-3.40 against 3.22-3.29, 4 080
// tiles 2.09-2.12 against 1.99-2.04 — two parts in every class measured; smaller launches are
// not measured and stay one chain.
constexpr uint64_t kChainPartsMinTiles = 4000;

// What the call has in flight beside the caller's stream, closed on every exit path (an
// error return included): an AQL segment still being packed is dropped (nothing of it has
// been submitted), and the context's aux streams are joined back into `stream`, so the
// caller's later work stays ordered after everything the call issued.
struct InFlight {
    rt_ctx* ctx;
    hipStream_t stream;
    rtc::Chain* chain = nullptr;
    bool seg_open = false;      // an AQL segment of this call is open
    uint32_t aux_live = 0;      // aux streams with work of this call not yet joined
    ~InFlight() {
        if (seg_open) rtc::chain_abort(chain);
        for (uint32_t k = 0; k < aux_live; ++k)   // (errors here: the call already failed)
            if (hipEventRecord(ctx->join_ev[k], ctx->aux[k]) == hipSuccess)
                (void)hipStreamWaitEvent(stream, ctx->join_ev[k], 0);
    }
};

// launch timing (rt_set_launch_timing): armed for this call's fused launches, disarmed on
// every exit path
struct Timing {
    rt_ctx* ctx;
    explicit Timing(rt_ctx* c) : ctx(c) {
        if (ctx->timing) rtk::arm_launch_events(ctx->time_ev[0], ctx->time_ev[1]);
    }
    ~Timing() {
        if (ctx->timing) ctx->timed_launches = rtk::disarm_launch_events();
    }
};

// One rt_update_frames call as its steps see it, beside the prepared launch parameters.
struct FrameCall {
    rt_ctx* ctx;
    hipStream_t stream;
    float4* img[2];          // frame f of the call writes img[(1 + f) % 2]
    const float* seeds;
    uint32_t frames, per;    // the call's frames; frames per launch (frames_per_launch_for)
    bool moved;              // camera_has_moved: frame 0 starts the accumulation again
};

// The first call of the context whose share is of the chain-parts class — usually a short one,
// long before a call that splits — sets up what part 1 needs: the stream, the events, and the
// raster unit table, which part 1's stream builds here (forked from and joined into `stream`).
// The stream's hardware queue exists from this launch on; created by the first split
// call instead, it cost that call several milliseconds.
rt_status chain_parts_setup(const FrameCall& c, const rtk::TraceParams& p, InFlight& fl) {
    rt_ctx* const ctx = c.ctx;
    const UnitGrid u = frame_group_units(frame_group_kernel(ctx, p), p.width, p.local_bands);
    if (rt_status s = ensure_aux_streams(ctx, 1u)) return s;
    if (rt_status s = ensure_order_buffers(ctx, u.units, c.stream)) return s;
    hipError_t e = hipEventRecord(ctx->fork_ev, c.stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->aux[0], ctx->fork_ev, 0);
    if (e != hipSuccess) return hip_fail(e, "fork (chain part set-up)");
    fl.aux_live = 1u;
    e = rtk::launch_raster_order(ctx->tile_order + 2 * ctx->order_tiles, (uint32_t)u.units,
                                 u.units_x, 2u, ctx->aux[0]);
    if (e != hipSuccess) return hip_fail(e, "rt_raster_order_kernel launch");
    ctx->chain_raster_key[0] = u.units;
    ctx->chain_raster_key[1] = u.units_x;
    fl.aux_live = 0;
    return join_aux(ctx, 1u, c.stream);
}

// The staggered schedule of a call that splits, empty if (frames, cap) has none: one chain.
std::vector<rt_chain_launch> split_schedule(uint32_t frames, uint32_t cap) {
    std::vector<rt_chain_launch> sched;
    int variant = 0;   // RT_CHAIN_SCHEDULE (environment, diagnostic): a schedule variant
    if (const char* e = std::getenv("RT_CHAIN_SCHEDULE")) variant = std::atoi(e);
    chain_schedule(frames, cap, variant, sched);
    if (std::none_of(sched.begin(), sched.end(),
                     [](const rt_chain_launch& l) { return l.part != 0u; }))
        sched.clear();
    return sched;
}

// The whole call as two staggered chains (`sched`, from split_schedule): part 0 on the caller's
// stream, part 1 on aux[0], joined at the end.  n_in0: the count every pixel of img[0] holds.
rt_status update_chain_parts(const FrameCall& c, rtk::TraceParams& p, InFlight& fl,
                             const std::vector<rt_chain_launch>& sched, uint32_t n_in0,
                             int* out_newest) {
    rt_ctx* const ctx = c.ctx;
    hipStream_t const stream = c.stream;
    const uint32_t frames = c.frames, per = c.per;
    const int kernel = frame_group_kernel(ctx, p);
    const UnitGrid u = frame_group_units(kernel, p.width, p.local_bands);
    // The unit order is frozen for the call: the cost order when this generation has one
    // (its dealt copy; the sort, if due, runs on `stream` here, before the fork), else the
    // raster order dealt the same way.  Costs are recorded by the first launch of cap
    // frames of each part (the same frames for every unit), when both parts have one.
    p.frames = per;
    p.store_each = ctx->frame_images == RT_FRAME_IMAGES_EVERY ? 2u : 1u;
    if (rt_status s = plan_tile_order(ctx, p, kernel, stream)) return s;
    if (rt_status s = ensure_order_buffers(ctx, u.units, stream)) return s;
    const uint32_t* table = ctx->tile_order + ctx->order_tiles;
    if (!p.tile_order) {
        table = ctx->tile_order + 2 * ctx->order_tiles;
        if (ctx->chain_raster_key[0] != u.units || ctx->chain_raster_key[1] != u.units_x) {
            hipError_t e = rtk::launch_raster_order(ctx->tile_order + 2 * ctx->order_tiles,
                                                    (uint32_t)u.units, u.units_x, 2u, stream);
            if (e != hipSuccess) return hip_fail(e, "rt_raster_order_kernel launch");
            ctx->chain_raster_key[0] = u.units;
            ctx->chain_raster_key[1] = u.units_x;
        }
    }
    uint32_t* const cost = p.tile_cost;
    size_t rec[2] = {sched.size(), sched.size()};
    for (size_t i = sched.size(); i-- > 0;)
        if (sched[i].frames == per) rec[sched[i].part] = i;
    const bool record = cost && rec[0] < sched.size() && rec[1] < sched.size();
    // the count every pixel holds before frame f of the call
    std::vector<uint32_t> n_at(frames + 1u);
    n_at[0] = c.moved ? 0u : n_in0;
    for (uint32_t f = 0; f < frames; ++f) n_at[f + 1u] = next_count(n_at[f], p.spp);
    if (rt_status s = ensure_aux_streams(ctx, 1u)) return s;
    // the fork, as the one-frame parts': no event when `stream` has nothing left to run
    bool wait_fork = false;
    if (rt_status s = fork_if_busy(ctx, stream, &wait_fork)) return s;
    p.parts = 2u;
    for (size_t i = 0; i < sched.size(); ++i) {
        const rt_chain_launch& L = sched[i];
        // frame f of the call writes img[(1 + f) % 2], whichever launch carries it
        p.part = L.part;
        p.in = c.img[L.first & 1u];
        p.out = c.img[1u - (L.first & 1u)];
        p.out2 = c.img[L.first & 1u];
        p.frames = L.frames;
        p.reset_first = (L.first == 0u && c.moved) ? 1u : 0u;
        fill_seeds(p.seed_b, c.seeds + L.first, L.frames);
        (void)fill_hint(p, n_at[L.first]);
        if (p.hint_frames != L.frames)
            return fail(RT_ERR_INVALID_ARGUMENT, "chain part launch is not fully hinted");
        p.tile_order = table;
        p.tile_cost = record && rec[L.part] == i ? cost : nullptr;
        if (rt_status s = plan_split(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_hint_rs(ctx, p, kernel)) return s;
        if (L.part == 1u && wait_fork) {
            hipError_t e = hipStreamWaitEvent(ctx->aux[0], ctx->fork_ev, 0);
            if (e != hipSuccess) return hip_fail(e, "fork (hipStreamWaitEvent)");
            wait_fork = false;
        }
        hipError_t e = rtk::launch_trace(p, kernel, L.part ? ctx->aux[0] : stream);
        if (e != hipSuccess) return hip_fail(e, "frame-group launch (chain part)");
        if (L.part) fl.aux_live = 1u;
        note_launch(ctx, p, kernel, L.frames);
        if (L.part) ctx->last.frames -= L.frames;   // (the call's frames, counted once)
    }
    ctx->last.chain_parts = 2u;
    if (record) {
        p.frames = per;
        p.tile_cost = cost;
        finish_tile_order(ctx, p);
    }
    fl.aux_live = 0;
    if (rt_status s = join_aux(ctx, 1u, stream)) return s;
    const int newest = (int)(frames & 1u);
    record_count(ctx, c.img[newest], p, n_at[frames]);
    record_count(ctx, c.img[1 - newest], p, n_at[frames - 1u]);
    if (out_newest) *out_newest = newest;
    return RT_OK;
}

// The call as one chain: a launch per `per` frames, each submitted in one of three forms — an
// AQL segment's packets, forked parts on the aux streams, or a single launch on `stream` —
// with everything in flight ended on the caller's stream afterwards.
rt_status update_launches(const FrameCall& c, rtk::TraceParams& p, InFlight& fl,
                          int* out_newest) {
    rt_ctx* const ctx = c.ctx;
    hipStream_t const stream = c.stream;
    rtc::Chain* const chain = fl.chain;
    int cur = 0;
    bool forked = false;        // aux streams ordered after the last work on `stream`
    uint32_t seg_parts = 0, seg_packets = 0;
    for (uint32_t f0 = 0; f0 < c.frames; f0 += c.per) {
        const uint32_t nf = std::min<uint32_t>(c.per, c.frames - f0);
        p.in = c.img[cur];
        p.out = c.img[1 - cur];
        p.out2 = c.img[cur];
        // (nf == 1: the plain single-frame store; else the ping-pong images of the last two
        // frames, or of every frame: rt_set_frame_images)
        p.store_each = nf == 1u ? 0u : ctx->frame_images == RT_FRAME_IMAGES_EVERY ? 2u : 1u;
        p.frames = nf;
        p.reset_first = (f0 == 0 && c.moved) ? 1u : 0u;
        fill_seeds(p.seed_b, c.seeds + f0, nf);
        // the counts both buffers hold afterwards (hint bookkeeping, see plan_hint)
        uint32_t n_in = 0;
        const bool known = p.reset_first || lookup_count(ctx, p.in, p, n_in);
        uint32_t n_prev = 0, n_last = 0;
        if (known) {
            n_last = fill_hint(p, p.reset_first ? 0u : n_in);
            // the frame before the last: what the other buffer holds when nf >= 2
            n_prev = p.reset_first ? 0u : n_in;
            for (uint32_t f = 0; f + 1u < nf; ++f) n_prev = next_count(n_prev, p.spp);
        } else {
            p.hint_frames = 0;
            p.hint_acc_frames = 0;
        }
        // Frame groups (several waves per tile, alternate frames) whenever every frame of
        // the launch is hinted: faster at every rank count measured.
        int kernel = trace_kernel_for(ctx, p);
        const bool pairable = kernel == rtk::kTraceList && p.store_each && known &&
                              p.hint_frames == nf;
        if (pairable && ctx->frame_pairs != RT_FRAME_PAIRS_OFF) kernel = frame_group_kernel(ctx, p);
        kernel = single_or(ctx, p, kernel);
        const bool aql = chain && nf == 1u &&
                         (kernel == rtk::kTraceSingle || kernel == rtk::kTraceSingleOne);
        const uint32_t parts = aql ? update_parts_aql(ctx, p) : update_parts(ctx, p, kernel);
        p.parts = parts;
        p.part = 0;
        // A new workgroup order (built on the stream by plan_wg_order) changes which pixels
        // each part owns, and rewrites the order buffer the parts may still be reading: the
        // parts in flight are joined into `stream` first and forked again after it.
        const bool new_order = wg_order_pending(ctx, p, kernel);
        if (fl.seg_open && (!aql || parts != seg_parts || new_order ||
                            seg_packets + parts > rtc::kMaxSegmentPackets)) {
            fl.seg_open = false;
            if (rt_status s = rtc::chain_end(chain, stream)) return s;
        }
        if ((parts == 1u || aql || new_order) && fl.aux_live) {  // wait for the parts
            if (rt_status s = join_aux(ctx, fl.aux_live, stream)) return s;
            fl.aux_live = 0;
            forked = false;
        }
        CALL_STAMP(3);
        if (rt_status s = plan_tile_order(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_wg_order(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_split(ctx, p, kernel, stream)) return s;
        if (rt_status s = plan_hint_rs(ctx, p, kernel)) return s;
        CALL_STAMP(4);
        if (aql) {
            // frame f of part k is a packet on the chain's queue k, after part k's frame f - 1
            if (!fl.seg_open) {
                if (rt_status s = rtc::chain_begin(chain, stream, parts)) return s;
                fl.seg_open = true;
                seg_parts = parts;
                seg_packets = 0;
            }
            for (uint32_t k = 0; k < parts; ++k) {
                p.part = k;
                if (rt_status s = rtc::chain_frame(chain, p, kernel, k)) return s;
            }
            seg_packets += parts;
        } else if (parts > 1u) {
            // every part's next frame reads only the pixels its own previous frame wrote;
            // what `stream` prepared (lists, order, the input image) is forked to the others
            // (fork_if_busy).  Part 0 goes out before the waits.
            if (rt_status s = ensure_aux_streams(ctx, parts - 1u)) return s;
            bool wait_fork = false;
            if (!forked) {
                if (rt_status s = fork_if_busy(ctx, stream, &wait_fork)) return s;
                forked = true;
            }
            for (uint32_t k = 0; k < parts; ++k) {
                p.part = k;
                if (k == 1u && wait_fork)
                    for (uint32_t j = 0; j + 1u < parts; ++j) {
                        hipError_t e = hipStreamWaitEvent(ctx->aux[j], ctx->fork_ev, 0);
                        if (e != hipSuccess) return hip_fail(e, "fork (hipStreamWaitEvent)");
                    }
                hipError_t e = rtk::launch_trace(p, kernel, k ? ctx->aux[k - 1] : stream);
                if (e != hipSuccess) return hip_fail(e, "rt_single_kernel launch");
                if (k) fl.aux_live = std::max(fl.aux_live, k);
            }
        } else {
            hipError_t e = rtk::launch_trace(p, kernel, stream);
            if (e != hipSuccess) return hip_fail(e, "rt_trace_kernel launch");
        }
        CALL_STAMP(5);
        finish_tile_order(ctx, p);
        note_launch(ctx, p, kernel, nf, parts, aql);
        // frame f of the launch wrote img[(cur + 1 + f) % 2]
        const int newest = (nf & 1u) ? 1 - cur : cur;
        if (known) {
            record_count(ctx, c.img[newest], p, n_last);
            if (nf >= 2) record_count(ctx, c.img[1 - newest], p, n_prev);
        } else {
            forget_count(ctx, c.img[newest]);
            if (nf >= 2) forget_count(ctx, c.img[1 - newest]);
        }
        cur = newest;
    }
    if (fl.seg_open) {   // the call's work ends on the caller's stream
        fl.seg_open = false;
        if (rt_status s = rtc::chain_end(chain, stream)) return s;
    }
    if (fl.aux_live) {
        const uint32_t n = fl.aux_live;
        fl.aux_live = 0;
        if (rt_status s = join_aux(ctx, n, stream)) return s;
    }
    if (out_newest) *out_newest = cur;
    return RT_OK;
}

rt_status update_frames(rt_ctx* ctx, float* image_a, float* image_b, uint32_t w, uint32_t h,
                        const rt_band_set& bands, const rt_scene_camera* cam,
                        const rt_sphere* spheres, uint32_t count, uint32_t frames,
                        const float* seeds, void* stream_v, int* out_newest) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (image_a == image_b) return fail(RT_ERR_INVALID_ARGUMENT, "image_a and image_b alias");
    DeviceGuard guard(ctx->device);
    CALL_STAMP(1);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    // an earlier call's AQL segment that failed is reported here, once
    if (rt_status s = chain_report(ctx)) return s;
    hipStream_t stream = static_cast<hipStream_t>(stream_v);
    rtk::TraceParams p;
    if (rt_status s = prepare(ctx, image_a, image_b, w, h, bands, cam, spheres, count, seeds,
                              stream, p))
        return s;
    CALL_STAMP(2);
    // Frames per launch (frames_per_launch_for).  Fusing removes the per-launch fill, tail
    // and kernel boundary (≈ 6 µs of a 30-µs K3 frame): the camera-ray-only instances
    // (max_depth <= 1) and the bounce instance (max_depth >= 2) run up to kHintFrames
    // frames per launch, the hint's reach; rt_set_frames_per_launch caps both (1 = one
    // dispatch per frame, the reference's structure).  The exhaustive and general culled
    // instances run one frame per launch.
    const uint32_t per = frames_per_launch_for(ctx, p);
    const FrameCall c{ctx, stream,
                      {reinterpret_cast<float4*>(image_a), reinterpret_cast<float4*>(image_b)},
                      seeds, frames, per, cam->camera_has_moved > 0.5f};
    ctx->last = {0, 0, 0, -1, 0, 0, 0, 1};
    InFlight fl{ctx, stream};
    // One-frame launches of the one-frame instances go out as AQL packets when the call has
    // two or more of them (rt_set_update_submit; a single update gains nothing from it).
    if (per == 1u && frames >= 2u)
        if (rt_status s = usable_chain(ctx, p, &fl.chain)) return s;
    Timing timing_scope{ctx};
    // Chain parts (rt_set_chain_parts): a call of two or more fused launches, every one a
    // frame-group launch, as two staggered chains over disjoint halves of the scheduling units
    // (chain_schedule).  With launch timing armed the call stays one chain: its kernel time is
    // defined per sequential launch.
    // the share is of a class whose longer calls split (whatever this call's frames)
    const bool chain_class =
        ctx->chain_parts != 1u && per >= 4u && per <= rtk::kHintFrames &&
        ctx->frame_pairs != RT_FRAME_PAIRS_OFF && trace_kernel_for(ctx, p) == rtk::kTraceList &&
        (ctx->chain_parts == 2u || launch_tiles(w, p.local_bands) >= kChainPartsMinTiles);
    if (chain_class && !ctx->aux[0])
        if (rt_status s = chain_parts_setup(c, p, fl)) return s;
    std::vector<rt_chain_launch> sched;
    uint32_t n_in0 = 0;
    if (chain_class && frames > per && !ctx->timing &&
        (c.moved || lookup_count(ctx, c.img[0], p, n_in0)))
        sched = split_schedule(frames, per);
    if (!sched.empty()) return update_chain_parts(c, p, fl, sched, n_in0, out_newest);
    if (rt_status s = update_launches(c, p, fl, out_newest)) return s;
    CALL_STAMP(6);
#ifdef RT_CALL_STAMPS
    std::fprintf(stderr, "RT_CALL_STAMPS %u %llu %llu %llu %llu %llu %llu\n", frames,
                 g_call_stamp[1] - g_call_stamp[0], g_call_stamp[2] - g_call_stamp[0],
                 g_call_stamp[3] - g_call_stamp[0], g_call_stamp[4] - g_call_stamp[0],
                 g_call_stamp[5] - g_call_stamp[0], g_call_stamp[6] - g_call_stamp[0]);
#endif
    return RT_OK;
}

}  // namespace

extern "C" {

rt_status rt_update(rt_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                    const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                    void* stream) {
    if (in != nullptr && in == out)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_update: in and out must not alias");
    if (!cam) return fail(RT_ERR_INVALID_ARGUMENT, "camera is NULL");
    const float seed = cam->random_seed;
    return trace(ctx, in, out, w, h, 0, 1, cam, spheres, count, 1, &seed, stream);
}

rt_status rt_render(rt_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                    const rt_scene_camera* cam, const rt_sphere* spheres, uint32_t count,
                    uint32_t frames, const float* seeds, void* stream) {
    return trace(ctx, in, out, w, h, 0, 1, cam, spheres, count, frames, seeds, stream);
}

rt_status rt_render_stripes(rt_ctx* ctx, const float* in, float* out, uint32_t w, uint32_t h,
                            uint32_t rank, uint32_t nranks, const rt_scene_camera* cam,
                            const rt_sphere* spheres, uint32_t count, uint32_t frames,
                            const float* seeds, void* stream) {
    return trace(ctx, in, out, w, h, rank, nranks, cam, spheres, count, frames, seeds, stream);
}

rt_status rt_update_frames(rt_ctx* ctx, float* image_a, float* image_b, uint32_t w, uint32_t h,
                           uint32_t rank, uint32_t nranks, const rt_scene_camera* cam,
                           const rt_sphere* spheres, uint32_t count, uint32_t frames,
                           const float* seeds, void* stream_v, int* out_newest) {
    CALL_STAMP(0);
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (nranks == 0 || rank >= nranks) return fail(RT_ERR_INVALID_ARGUMENT, "bad rank/nranks");
    return update_frames(ctx, image_a, image_b, w, h, stripe_set(h, rank, nranks), cam, spheres,
                         count, frames, seeds, stream_v, out_newest);
}

rt_status rt_update_frames_bands(rt_ctx* ctx, float* image_a, float* image_b, uint32_t w,
                                 uint32_t h, const rt_band_set* bands,
                                 const rt_scene_camera* cam, const rt_sphere* spheres,
                                 uint32_t count, uint32_t frames, const float* seeds,
                                 void* stream_v, int* out_newest) {
    CALL_STAMP(0);
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!bands) return fail(RT_ERR_INVALID_ARGUMENT, "bands is NULL");
    return update_frames(ctx, image_a, image_b, w, h, *bands, cam, spheres, count, frames,
                         seeds, stream_v, out_newest);
}

rt_status rt_set_launch_timing(rt_ctx* ctx, int enable) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    if (enable && !ctx->time_ev[0]) {
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipEventCreate(&ctx->time_ev[i]);
            if (e != hipSuccess) return hip_fail(e, "hipEventCreate(launch timing)");
        }
    }
    ctx->timing = enable != 0;
    ctx->timed_launches = 0;
    return RT_OK;
}

rt_status rt_last_call_kernel_time(rt_ctx* ctx, float* out_ms, uint32_t* out_launches) {
    if (!ctx) return fail(RT_ERR_INVALID_CONTEXT, "ctx is NULL");
    if (!out_ms) return fail(RT_ERR_INVALID_ARGUMENT, "out_ms is NULL");
    if (!ctx->timing || ctx->timed_launches == 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "the last call carried no timed launch");
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return fail(RT_ERR_INVALID_DEVICE, "hipSetDevice failed");
    hipError_t e = hipEventSynchronize(ctx->time_ev[1]);
    if (e == hipSuccess) e = hipEventElapsedTime(out_ms, ctx->time_ev[0], ctx->time_ev[1]);
    if (e != hipSuccess) return hip_fail(e, "hipEventElapsedTime(launch timing)");
    if (out_launches) *out_launches = ctx->timed_launches;
    return RT_OK;
}

rt_status rt_chain_schedule(uint32_t frames, uint32_t cap, int variant, rt_chain_launch* out,
                            uint32_t max_out, uint32_t* out_count) {
    if (!out_count) return fail(RT_ERR_INVALID_ARGUMENT, "out_count is NULL");
    if (frames == 0 || cap == 0) return fail(RT_ERR_INVALID_ARGUMENT, "frames or cap is 0");
    if (variant < 0 || variant > kScheduleVariants)
        return fail(RT_ERR_INVALID_ARGUMENT, "unknown schedule variant");
    std::vector<rt_chain_launch> sched;
    chain_schedule(frames, cap, variant, sched);
    *out_count = (uint32_t)sched.size();
    if (sched.size() > max_out || (!out && !sched.empty()))
        return fail(RT_ERR_INVALID_SIZE, "the schedule has more launches than `out` holds");
    std::copy(sched.begin(), sched.end(), out);
    return RT_OK;
}

}  // extern "C"
