// rt_kernels.hip — gfx950 kernels for the per-pixel ray tracer.
//
// Replaces the reference's WGSL compute kernels (assets/compute_shader.wgsl):
//   rt_trace_kernel   == `update` (wgsl:333-364), optionally fused over several frames
//   rt_init_kernel    == `init`   (wgsl:65-70)
//   rt_deinterleave   root-side scatter of gathered stripe tiles (multi-GPU)
//
// Mapping onto CDNA4: one wave64 = one 8x8 pixel tile (the reference's 8x8 workgroup,
// wgsl:333), four waves per 256-thread workgroup.  The sphere scan (wgsl:164-221) walks
// a wave-uniform index, so the 16-byte scan records are fetched with scalar loads into
// SGPRs and consumed directly as VALU operands — no VGPRs and no LDS traffic per test.
// The 32-byte material record is fetched only for the winning hit.  Each lane keeps its
// pixel's accumulator in registers across fused frames and writes it back with one
// coalesced 16-byte store (one HBM read + one write per pixel per launch).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_kernels.h"

#include <cstddef>
#include <cstring>

// The device code is written for gfx950 only.  Two of its hand-offs between workgroups (the
// split bounce schedule's chunk colours, the AQL chain's frames) rely on that target's cache
// policy bits — the buffer intrinsics' aux = 16 is sc1: write-through stores and L1-bypassing
// loads — and on the drained-`sc1` forms MI355X_MICROARCH.md measures for it (inter-workgroup
// visibility, "Valid forms") in place of agent-scope release / acquire fences.  Another
// target would need those re-checked (or the fences), so it does not compile.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "rt_kernels.hip targets gfx950 only (cache-policy bits of the sc1 hand-offs)"
#endif

namespace rtk {

using namespace rtd;

// ---- diagnostic wave trace (RT_WAVE_TRACE=1 builds only; never in the product) -------
// Per wave of the camera-ray-only and bounce instances: start and end s_memrealtime, HW_ID, XCC_ID,
// indexed by workgroup * 4 + wave (tools/wave_trace.py reads them via rt_diag_wave_trace).
#ifndef RT_WAVE_TRACE
#define RT_WAVE_TRACE 0
#endif
#if RT_WAVE_TRACE
constexpr uint32_t kTraceWaves = 1u << 18;
__device__ unsigned long long g_wave_t[kTraceWaves][2];
__device__ unsigned g_wave_id[kTraceWaves][2];
__device__ __forceinline__ void wave_trace(int end) {
    const uint32_t gw = (blockIdx.y * gridDim.x + blockIdx.x) * 4u + (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0 && gw < kTraceWaves) {
        g_wave_t[gw][end] = __builtin_amdgcn_s_memrealtime();   // 100 MHz, chip-wide
        if (end) {
            g_wave_id[gw][0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID
            g_wave_id[gw][1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID
        }
    }
}
#define WAVE_TRACE(e) wave_trace(e)
#endif

// ---- diagnostic bounce counters (RT_BOUNCE_COUNTS=1 builds only; never in the product) ---
// BCOUNT(k): the wave's first active lane adds 1 to g_bcount[k] and the active lanes' count
// to g_bcount[k + 1] — wave-level trips and lane-level work of a code region
// (tools/bounce_counts.py reads them via rt_diag_bounce_counts).
#ifndef RT_BOUNCE_COUNTS
#define RT_BOUNCE_COUNTS 0
#endif
#if RT_BOUNCE_COUNTS
__device__ unsigned long long g_bcount[32];
__device__ __forceinline__ void bcount(int k) {
    const uint64_t ex = __builtin_amdgcn_read_exec();
    if ((threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(ex)) {
        atomicAdd(&g_bcount[k], 1ull);
        atomicAdd(&g_bcount[k + 1], (unsigned long long)__builtin_popcountll(ex));
    }
}
#define BCOUNT(k) bcount(k)
#endif

// ---- diagnostic phase stamps of the one-frame kernel (RT_SSTAMPS=1 builds only) ------
// Per wave of rt_single_kernel: s_memtime when each phase's result is available (the asm
// consumes the value, so the stamp waits for it): 0 entry, 1 workgroup order resolved,
// 2 seed tables + candidate counts arrived, 3 camera rays built, 4 list walk done, 5 hit
// shading + sky done, 6 accumulator consumed, 7 stores issued; 8 / 9 s_memrealtime at entry
// / end (100 MHz), 10 HW_ID, 11 XCC_ID.  tools/stamps_single.py reads them
// (rt_diag_single_stamps).
#ifndef RT_SSTAMPS
#define RT_SSTAMPS 0
#endif
#if RT_SSTAMPS
constexpr uint32_t kSStampWaves = 1u << 17;
__device__ unsigned long long g_sst[kSStampWaves][12];
__device__ __forceinline__ uint32_t sst_wave() {
    return (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
}
__device__ __forceinline__ void sst_put(int k, unsigned long long t) {
    const uint32_t gw = sst_wave();
    if ((threadIdx.x & 63u) == 0u && gw < kSStampWaves) g_sst[gw][k] = t;
}
#define SST_V(k, dep)                                        \
    do {                                                     \
        asm volatile("" ::"v"(dep));                         \
        sst_put((k), __builtin_amdgcn_s_memtime());          \
    } while (0)
#define SST_S(k, dep)                                        \
    do {                                                     \
        asm volatile("" ::"s"(dep));                         \
        sst_put((k), __builtin_amdgcn_s_memtime());          \
    } while (0)
#elif defined(RT_MARKS)
// (asm-inspection builds: a comment in the code at each phase boundary, after its value)
#define SST_V(k, dep) asm volatile(";MARK " #k ::"v"(dep))
#define SST_S(k, dep) asm volatile(";MARK " #k ::"s"(dep))
#endif

}  // namespace rtk

// The tracer's device library (scans, culling, camera, ray_color, sample, trace_pixel), shared
// with rt_aov.hip, rt_sampler.hip and rt_selftest.hip.  Included after the diagnostic macros
// above: the header defines the ones left undefined as no-ops.
#include "rt_trace_device.h"
// the list build's occlusion rule (rt_candidates_kernel)
#include "rt_occlusion.h"

namespace rtk {

// Frame groups (kTraceListPair, rt_update_frames with every pixel at the hinted count):
// kFrameGroup waves own the same tile; wave w traces frames f + w of each group of
// kFrameGroup frames (the samples are independent — the count each one uses is the hinted
// n + f, verified up front), waves 1.. hand their colours to wave 0 through LDS, and wave 0
// accumulates the group's frames in order and stores the surviving images (wgsl:352-363)
// — bit-identical to one wave doing every frame.  More waves, each with a shorter
// sequential chain.
// Called only when every valid pixel's loaded count is the hinted one (rt_trace_kernel).
// Waves per tile: 2 (kTraceListPair) or 4 (kTraceListQuad).  K3 per frame, whole image on
// one GPU: 16.8 / 18.8 us; 8-rank share: 3.13 / 2.95 us (`profiles/r01_rank_sim_groups_k3.txt`).
// Round 5: one more wave per tile that only accumulates and stores, so that every group's
// samplers all trace, measured slower at every size (8-rank share 2.91 against 2.54 us per
// step, whole image 17.2 against 14.6; profiles/r05/r05j/); so did tracing each frame with
// the one-frame kernel's sample (single_sample<1>, records from LDS or by scalar loads:
// profiles/r05/r05h/, r05m/).
template <int kScan>
constexpr uint32_t frame_group() {
    return kScan == kTraceListQuad ? 4u : 2u;
}
// LDS of a frame group: two slots of the producer waves' colours (double-buffered groups)
template <int kScan>
constexpr size_t group_lds_bytes() {
    return (size_t)2u * (frame_group<kScan>() - 1u) * 64u * 16u;
}
template <int kScan>
__device__ __forceinline__ void trace_pair(const TraceParams& p, const Cam& cam, uint32_t tile,
                                           uint32_t ncand, const TileCoord& tc, uint32_t hxy,
                                           float4 acc, uint32_t w) {
    const uint32_t spp = p.spp;                                   // wgsl:343
    v3 c = mk(0.0f, 0.0f, 0.0f);
    if (!p.reset_first) c = mk(acc.x, acc.y, acc.z);              // wgsl:339-341
    // From here every valid pixel holds hint_n[f] before frame f (the host's count
    // bookkeeping, rt_abi.cpp fill_hint): the count arithmetic of wgsl:341-362 is scalar.
    const uint32_t lane = threadIdx.x & 63u;
    constexpr uint32_t kFrameGroup = frame_group<kScan>();
    for (uint32_t f = 0; f < p.frames; f += kFrameGroup) {
        const uint32_t fw = f + w;
        const uint32_t ng = fw < p.frames ? p.hint_n[fw] : spp;  // count before frame fw
        v3 col;
        if (ng < spp && rt_ballot(tc.valid) != 0ull) {             // wgsl:352
            col = sample<kScan>(p, cam, tile, ncand, tc, hxy, ng, p.seed_b[fw], fw, tc.valid,
                                fw < p.hint_frames);
        } else {
            col = zero_v3_here();
        }
        // two LDS slots alternating by group: wave 0 reads group g's slot before it reaches
        // the barrier of group g + 1, so one barrier per group suffices
        float4* slot = lds_recs + ((f / kFrameGroup) & 1u) * (kFrameGroup - 1u) * 64u;
        if (w != 0u)
            *reinterpret_cast<f3v*>(&slot[(w - 1u) * 64u + lane]) = f3v{col.x, col.y, col.z};
        __syncthreads();
        if (w == 0u) {
            const uint64_t valid_m = rt_ballot(tc.valid);
#pragma unroll
            for (uint32_t j = 0; j < kFrameGroup; ++j) {
                const uint32_t fj = f + j;
                if (fj >= p.frames) break;
                if (j != 0) {
                    const float4 cj = slot[(j - 1u) * 64u + lane];
                    col = mk(cj.x, cj.y, cj.z);
                }
                const uint32_t nb = p.hint_n[fj];                 // count before frame fj
                // f32(nb + 1) (the divisor k, wgsl:356) or f32(nb): the host's table
                const float cnt = p.hint_cnt[fj];
                if (nb < spp) {                                   // wgsl:352-358
                    const v3 num = sub(col, c);
                    // num / f32(nb + 1) (wgsl:356) as a Markstein division (acc_rn); both
                    // conditions scalar (see rt_tpair_kernel)
                    const bool rn = (nb < kAccRnMax) &
                                    ((mask_ult(acc_min_bits(num), kAccOkDbl) & valid_m) == 0ull);
                    if (rn) {
                        c = acc_rn(c, num, cnt, p.hint_rcp[fj]);
                    } else {
                        const float k = cnt;                      // wgsl:356
                        c = mk(c.x + num.x / k, c.y + num.y / k, c.z + num.z / k);
                    }
                }
                // wgsl:362-363: the images that survive (or every frame's, store_each 2)
                if ((p.store_each == 2u || fj + 2u >= p.frames) && tc.valid)
                    ((fj & 1u) ? p.out2 : p.out)[tc.idx] = make_float4(c.x, c.y, c.z, cnt);
            }
        }
    }
}

// One workgroup = 4 waves = 4 consecutive tiles.  (A persistent grid that walks tiles
// with the next tile's accumulator prefetched — into VGPRs, or into LDS with
// global_load_lds — measured 15-50 % slower: the loop pushes the kernel past 64 VGPRs /
// into scratch, and the hardware dispatcher already overlaps the waves' HBM phases.)
// (RT_TRACE_MIN_WAVES, the waves per SIMD these instances are planned for: rt_trace_device.h.)
// Kernel-argument prefetch (single-frame list instance, one tile per wave): the launch
// parameters a wave reads are spread over ~12 cache lines of the 2.6-KB kernarg segment and
// the compiler loads each just before its use — a chain of dependent scalar-cache misses at
// every wave start.  One scalar load per line, all in flight together and awaited once,
// brings them into the scalar cache first (K3 single-frame 30.56 -> 30.28 us, K2 23.72 ->
// 23.40, profiles/r02_ab_single_frame.log).  Adding the first lines of the tile's candidate
// and sphere records to it measured +1.0 us (the wave then waits for two HBM misses before
// its first instruction of ray setup).
// Leading scalar arguments of rt_trace_kernel (before the TraceParams block): what a wave
// needs before its first ray — the tile's candidate count, the seed-hash tables, the
// accumulator and the tile geometry.  Built with -mllvm -amdgpu-kernarg-preload-count=9
// (Makefile), the command processor places these 9 dwords in SGPRs at wave launch, so the
// count, hash and accumulator loads issue at once, together with the kernel-argument
// prefetch, instead of after a kernarg round trip (K3 single-frame 30.7 -> 29.6 us, K2 23.7
// -> 22.9, profiles/r02_ab_single_frame.log).  TraceParams (alignment 16) starts at byte 48.
constexpr uint32_t kParamsOff = 48;
__device__ __forceinline__ void karg_prefetch() {
    const char kconst* kp =
        (const char kconst*)__builtin_amdgcn_kernarg_segment_ptr() + kParamsOff;
    uint32_t d0, d1, d2, d3, d4, d5, d6, d7, d8, d9, d10;
    asm volatile(
        "s_load_dword %0, %11, 0x0\n\t"
        "s_load_dword %1, %11, 0x40\n\t"
        "s_load_dword %2, %11, 0x80\n\t"
        "s_load_dword %3, %11, 0xc0\n\t"
        "s_load_dword %4, %11, 0x100\n\t"
        "s_load_dword %5, %11, 0x140\n\t"
        "s_load_dword %6, %11, 0x180\n\t"
        "s_load_dword %7, %11, %12\n\t"
        "s_load_dword %8, %11, %13\n\t"
        "s_load_dword %9, %11, %14\n\t"
        "s_load_dword %10, %11, %15\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4), "=&s"(d5), "=&s"(d6),
          "=&s"(d7), "=&s"(d8), "=&s"(d9), "=&s"(d10)
        : "s"(kp), "i"(offsetof(TraceParams, hint_n)), "i"(offsetof(TraceParams, hint_rcp)),
          "i"(offsetof(TraceParams, hint_rs)), "i"(offsetof(TraceParams, seed_b))
        : "memory");
    (void)d0; (void)d1; (void)d2; (void)d3; (void)d4; (void)d5;
    (void)d6; (void)d7; (void)d8; (void)d9; (void)d10;
}

// Waves (tiles) per workgroup: the culled instance shares the LDS copy of the records among
// 4 waves; a frame-group instance is one tile's group; the others RT_WG_WAVES (rt_kernels.h).
template <int kScan>
constexpr uint32_t wg_waves() {
    return kScan == kTraceCulled ? 4u : is_group_kernel(kScan) ? frame_group<kScan>() : RT_WG_WAVES;
}


// Cost-ordered tiles (TraceParams::tile_order / tile_cost) in the camera-ray-only
// instances, whose workgroups are one tile each.

template <int kScan>
constexpr bool kOrdered = trace_ordered(kScan);
// (the start time is parked in tile_cost itself: no register stays live for it)
template <int kScan>
__device__ __forceinline__ void cost_start(const TraceParams& p, uint32_t tile, uint32_t wave,
                                           uint32_t lane) {
    if (kOrdered<kScan> && p.tile_cost && wave == 0u && lane == 0u)
        p.tile_cost[tile] = (uint32_t)__builtin_amdgcn_s_memtime();
}
template <int kScan>
__device__ __forceinline__ void record_cost(const TraceParams& p, uint32_t tile, uint32_t wave,
                                            uint32_t lane) {
    if (kOrdered<kScan> && p.tile_cost && wave == 0u && lane == 0u)
        p.tile_cost[tile] = (uint32_t)__builtin_amdgcn_s_memtime() - p.tile_cost[tile];
}

template <int kScan>
__global__ __launch_bounds__(64 * wg_waves<kScan>(), RT_TRACE_MIN_WAVES) void rt_trace_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const TraceParams p) {
    WAVE_TRACE(0);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tiles_x = (a_width + 7u) >> 3;
    // The wave index is uniform, but the compiler's divergence analysis does not know it;
    // readfirstlane makes the tile (and the candidate-list pointers and counts derived from
    // it) scalar, so list records are read with s_load into SGPRs.
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // (frame groups: all waves of the workgroup own the same tile)
    uint32_t tx = is_group_kernel(kScan) ? blockIdx.x : blockIdx.x * wg_waves<kScan>() + wave;
    uint32_t lband = blockIdx.y;
    const uint32_t band_first = a_bands & 0xFFFFu, band_step = (a_bands >> 16) & 0x7FFFu;
    if (kOrdered<kScan> && (a_bands >> 31)) {         // costliest tiles first (tile_order)
        const uint32_t slot = blockIdx.y * gridDim.x + blockIdx.x;
        // (readfirstlane: the loaded value is uniform, but only the scalar form keeps the
        // list pointer and records in SGPRs — s_load chunks instead of vector loads)
        const uint32_t t = __builtin_amdgcn_readfirstlane(p.tile_order[slot]);
        tx = t & 0xFFFFu;
        lband = t >> 16;
    }
    const bool wave_in = tx < tiles_x;
    const TileCoord tc = tile_coord(a_width, a_height, band_first, band_step, tx, lband, lane);
    const uint32_t tile = lband * tiles_x + tx;
    // the tile's candidate count (kCandNone: no list), the accumulator (wgsl:339; a frame-0
    // reset discards it: no load) and hash(x*73) ^ hash(y*51) (wgsl:309-310) from the
    // per-column / per-row tables: issued from the preloaded arguments, before the
    // kernel-argument prefetch below is awaited
    const uint32_t ncand = (kScan != kTraceExhaustive && a_cand && wave_in)
                               ? load_cnt(a_cand, tile)
                               : kCandNone;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // (loaded even when frame 0 resets the pixel or the wave has no tile, so that the load
    // waits for no kernarg read and no branch; the value is discarded then)
    acc = a_in[tc.valid ? tc.idx : 0];
    const uint32_t hxy =
        a_hx[min(tc.x, a_width - 1u)] ^ a_hx[hy_offset(a_width) + min(tc.y, a_height - 1u)];
    if (kScan == kTraceList) karg_prefetch();
    // Culled scan: the workgroup stages the scan records (count padded to 64) in LDS once;
    // the per-block cone test then reads them at LDS latency instead of L2 latency.
    if (kScan == kTraceCulled && p.lds_records) {
        for (uint32_t j = threadIdx.x; j < p.lds_records; j += 512u) {
            const float4 g0 = p.geom[j];
            const float4 g1 = p.geom[j + 256u < p.lds_records ? j + 256u : j];
            lds_recs[j] = g0;
            if (j + 256u < p.lds_records) lds_recs[j + 256u] = g1;
        }
        __syncthreads();
    }
    if (!wave_in) return;                                         // whole wave exits
    cost_start<kScan>(p, tile, wave, lane);

    Cam cam;
    cam.center = mk(p.center[0], p.center[1], p.center[2]);
    cam.vul = mk(p.vul[0], p.vul[1], p.vul[2]);
    cam.pdu = mk(p.pdu[0], p.pdu[1], p.pdu[2]);
    cam.pdv = mk(p.pdv[0], p.pdv[1], p.pdv[2]);
    cam.ddu = mk(p.ddu[0], p.ddu[1], p.ddu[2]);
    cam.ddv = mk(p.ddv[0], p.ddv[1], p.ddv[2]);
    cam.defocus_angle = p.defocus_angle;

    if (is_group_kernel(kScan)) {
        // every frame's image is stored inside; on a count mismatch (every wave sees the
        // same pixels, hence takes the same decision) wave 0 runs the single-wave loop and
        // the others have nothing to do
        if (p.reset_first || rt_ballot(tc.valid && f2u(acc.w) != p.hint_n[0]) == 0ull) {
            trace_pair<kScan>(p, cam, tile, ncand, tc, hxy, acc, wave);
            record_cost<kScan>(p, tile, wave, lane);
            WAVE_TRACE(1);
            return;
        }
        if (wave != 0u) return;
    }
    const float4 res = trace_pixel<kScan, !is_group_kernel(kScan)>(p, cam, tile, ncand, tc,
                                                                   hxy, acc);
    if (tc.valid && !(kStoreEach<kScan> && p.store_each))        // wgsl:363
        p.out[tc.idx] = res;
    record_cost<kScan>(p, tile, wave, lane);
    WAVE_TRACE(1);
}

// ---- Single-frame update (kTraceSingle): one `update` dispatch, camera rays only --------
//
// The reference's step (lib.rs:408-417: one `update` per frame, wgsl:333-364) at
// max_depth <= 1 for cameras in the proven domain (the kTraceList conditions) and one frame
// per launch.  rt_trace_kernel<kTraceList> pays its general machinery (frame loop, retrace
// loop, per-frame kernarg reads spread over a 2.6-KB parameter block) for the one frame;
// this kernel does the one frame only, with its parameters in one compact block, and gives
// each lane kSinglePix pixels — the same column of kSinglePix horizontally adjacent 8x8
// tiles — so that a wave's fixed costs (launch, parameter and list loads, the disk table)
// are shared and its independent pixel chains interleave (more instructions in flight per
// wave while the list and accumulator loads are outstanding).  The per-pixel arithmetic is
// ray_color's (wgsl:261-297) for depth <= 1, operation for operation: the image bits are
// those of rt_trace_kernel (every parity test runs both, rt_set_single_kernel).
struct SingleParams {
    float4* out;
    const float4* geom;    // full scan records (tiles without a candidate list)
    const float4* sph;     // full sphere records
    uint32_t count, depth, spp;
    uint32_t hinted;       // hint_n / hint_rcp / hint_rs of frame 0 are valid
    uint32_t n_hint;       // every pixel's count before the frame (0 on reset)
    uint32_t seed_b;       // B = u32(random_seed * 2^32) (wgsl:311, 353)
    uint32_t hy_off;       // hash(y * 51) table offset in the hx buffer
    float rcp_hint;        // RN32(1 / f32(n_hint + 1)) (acc_rn)
    uint32_t normal_rn;    // TraceParams::normal_rn
    uint32_t reserved[4];  // (the fields after keep round 4's offsets)
    // local bands of a launch in raster order (no a_order): lband = first + blockIdx.y *
    // step, first | step << 16 — one of the update's concurrent parts (launch_single)
    uint32_t lbands;
    float4 rs;             // (rf(sb), random_unit_vector(sb)) of frame 0, bounce 0
    float center[3], vul[3], pdu[3], pdv[3], ddu[3], ddv[3];
    float defocus_angle;
    // the launch's workgroups per row (rt_chain_kernel reads it here instead of the hidden
    // kernel arguments: its packets are written by rt_chain.cpp)
    uint32_t grid_x;
    // rt_chain_kernel only: non-zero once a segment's go wait gave up — the frame's image
    // stores are dropped (rt_chain.cpp; rt_single_kernel ignores it)
    const uint32_t* abort;
};
static_assert(offsetof(SingleParams, lbands) == 76,
              "SingleParams keeps round 4's offsets after rcp_hint");

// Tiles per wave of the two instances: kTraceSingle (whole-image launches) and
// kTraceSingleOne (small per-rank shares, where more, shorter waves fill the chip).
#ifndef RT_SINGLE_PIX
#define RT_SINGLE_PIX 2
#endif
constexpr uint32_t kSinglePix = RT_SINGLE_PIX;
static_assert(kSinglePix >= 1 && kSinglePix <= 4, "1 to 4 tiles per wave");
// Waves per SIMD the one-frame kernel's register plan targets.  The compiler fills the
// SGPR budget the bound allows: at 5 it reached 98 SGPRs (6 resident waves per SIMD on
// gfx950: MI355X_MICROARCH.md, Residency), at 7 it stays at <= 96 (7 waves) without spills.
#ifndef RT_SINGLE_MIN_WAVES
#define RT_SINGLE_MIN_WAVES 7
#endif
// (Knock-out builds of the one-frame kernel — no accumulator load, sphere scan, random
// camera ray, hit shading or image store, for cost attribution — are an experiment-only
// patch: tools/patches/single_knockouts.patch, DESIGN_HISTORY.md §5.)
// waves per workgroup of the one-frame kernel: 2 since round 4 (profiles/r04/r04a2_single_shape.txt,
// r04b2_driver_wg2.txt: 0.2 us per update faster than 4 at K3, same bits)
#ifndef RT_SINGLE_WG
#define RT_SINGLE_WG 2
#endif
constexpr uint32_t kSingleWg = RT_SINGLE_WG;
// The one-frame kernel walks both tiles' candidate lists in one loop, one record of each per
// step (round 4: fewer padding records tested when the two lists differ in length).
// The tiles' 1-KB candidate blocks are loaded whole at wave start (one 16-B load per lane,
// beside the seed and accumulator loads) and kept in LDS: the scan records and the hit
// records are then LDS reads instead of dependent L2/HBM round trips.  It shortens a
// wave's memory chain (8-rank K3 share, one tile per wave: 7.10 -> 6.64 us per update) but
// costs a whole launch more than it saves (K3 24.9 -> 25.8 us, K2 18.3 -> 19.9;
// profiles/r02_ab_single_lds_k*.log): 1 = the one-tile instance only, 2 = both, 0 = none.
#ifndef RT_SINGLE_LDS
#define RT_SINGLE_LDS 1
#endif
// The defocus disk's reciprocal in the one-frame kernel is all-f32 (disk_unit<3>: the length
// and its reciprocal from the bits of len2, one Markstein step; no f64, no LDS table, no
// barrier).  The workgroup's LDS table made every wave wait for wave 0's kernarg read at
// wave start (K3 23.30 -> 22.46 µs per update without it, profiles/r03/r03a_ab_single.log); the
// all-f32 form with the lane masks: profiles/r03/r03t_ab_single_masks_all.log.
constexpr int kSingleDisk = 3;
// hash(x*73) ^ hash(y*51) (wgsl:309-310) of the one-frame kernel: from the per-column /
// per-row tables (two dependent loads behind the order entry) or computed in the wave —
// one hash per lane (lanes [0, 8*kPix) the wave's columns, the next 8 its rows), handed to
// the pixels with ds_bpermute — so the camera rays need no memory at all.  Bit k set =
// computed in the kPix = k + 1 instance.  Default: the one-tile instance (rank shares)
// computes them — 4-rank shares 0.1-0.3 µs faster per update, 8-rank unchanged
// (profiles/r03/r03zn_single_hash1.txt); the two-tile instance (whole images) reads the tables
// (computing them there cost 0.9 µs at K3, profiles/r03/r03e_ab_single_switches.log).
#ifndef RT_SINGLE_HASH
#define RT_SINGLE_HASH 1
#endif

// The one-frame kernel's per-lane selects after the hit shading (hit / miss, the degenerate
// scatter direction, metal absorption) run only in waves whose lanes differ: a wave-uniform
// branch on a lane mask skips them otherwise (round 4, with sqrt_core_rcp above).  The
// sky's |d|^2 (wgsl:294's normalize) is taken from where the direction was made — the
// camera ray's a = d.d (wgsl:184, computed for the scan), the Lambertian scatter's
// |n + ruv|^2 (computed for its degenerate-direction test, wgsl:89), or the normalised metal
// / dielectric direction's own dot — instead of one more dot product per pixel (the same
// operations on the same operands: the same bits; K3 15.93 against 16.37 µs per update in
// the driver's command, profiles/r04/r04p_ab_skydd.txt).

// Shading of a camera ray's hit at depth 1 (ray_color's loop body at i = 0, wgsl:266-286):
// sets the scattered direction and attenuation, or black (metal absorbed).  r_sb / ruv are
// the scatter's random numbers.  Lanes with !hit compute garbage that the caller drops.
__device__ __forceinline__ void shade_hit(float4 pr, float4 mat, float t, v3 o, v3 d,
                                          float r_sb, v3 ruv, bool hit, uint64_t hm,
                                          bool normal_rn, v3& nd, v3& att, bool& black,
                                          bool& took_other, float& ndd) {
    const v3 hp = fmas(t, d, o);
    const v3 rel = sub(hp, mk(pr.x, pr.y, pr.z));
    v3 outward;                                                   // wgsl:209
    // (some |rel| below 2^-100 as one v_min3_f32 on |.| and one ordered compare: the same
    // lanes as the minimum of the abs bit patterns — a NaN channel is never the small one
    // either way, and rel, an arithmetic result, is never a signalling NaN)
    if ((__builtin_amdgcn_fcmpf(min_abs3(rel), 0x1p-100f, 4) & hm) == 0ull) {   // (FCMP_OLT)
        const float y = rcp_refined(pr.w);
        outward = normal_div(rel, pr.w, y, normal_rn);
    } else {
        outward = divs(rel, pr.w);
    }
    const float dno = dot(d, outward);
    const bool front = dno < 0.0f;
    const v3 n = front ? outward : neg(outward);
    // lambertian (wgsl:84-93), computed for every lane; the other materials below
    v3 dir = add(n, ruv);
    const float ddir = dot(dir, dir);
    ndd = ddir;                     // |nd|^2 for the sky (sky_w's dd)
    if ((__builtin_amdgcn_fcmpf(ddir, 0x1.0c6f7ap-20f, 4) & hm) != 0ull) {   // (FCMP_OLT)
        // (the degenerate scatter direction, wgsl:89-91: per-lane selects only in a wave
        // that has one)
        asm volatile("");
        if (ddir < 0x1.0c6f7ap-20f) {
            dir = n;
            ndd = dot(n, n);
        }
    }
    nd = dir;
    att = mk(mat.x, mat.y, mat.z);
    black = false;
    took_other = false;
    const bool other = hit && !(mat.w < -1.0f);
    if ((mask_not_lt(mat.w, -1.0f) & hm) != 0ull)
        took_other = true;
    if ((mask_not_lt(mat.w, -1.0f) & hm) != 0ull && other) {
        if (mat.w <= 1.0f) {                                      // metal wgsl:95-100
            const v3 refl = fmas(mat.w, ruv, normalize_w<true>(reflect(d, n)));
            black = !(dot(refl, n) > 0.0f);                       // wgsl:277-279
            nd = normalize_w<true>(refl);
            ndd = dot(nd, nd);
        } else {                                                  // dielectric wgsl:102-135
            att = mk(1.0f, 1.0f, 1.0f);
            const float ratio = front ? 1.0f / mat.x : mat.x;
            const v3 u = normalize_w<true>(d);
            const float cos_t = fminf(dot(neg(u), n), 1.0f);
            const float sin_t = sqrtf(fmaf(-cos_t, cos_t, 1.0f));
            const bool cannot = ratio * sin_t > 1.0f;
            const bool refl = cannot || reflectance(cos_t, ratio) > r_sb;
            nd = normalize_w<true>(refl ? reflect(u, n) : refract(u, n, ratio));
            ndd = dot(nd, nd);
        }
    }
}

// normalize(d).y of the sky (wgsl:293-296) and its colour times cf
__device__ __forceinline__ v3 sky_w(v3 cf, v3 d, float dd) {
    float uy;
    if (rt_ballot(__float_as_uint(dd) - kBits2m20 >= kBits2p40 - kBits2m20) == 0ull) {
        float y;
        const float len = sqrt_core_rcp(dd, y);
        uy = div_core(d.y, len, y);
    } else {
        uy = d.y / sqrtf(dd);
    }
    const float a = 0.5f * (uy + 1.0f);
    const float om = 1.0f - a;
    return mul(cf, mk(fmaf(a, 0.5f, om), fmaf(a, 0x1.666666p-1f, om), fmaf(a, 1.0f, om)));
}
__device__ __forceinline__ v3 sky_w(v3 cf, v3 d) { return sky_w(cf, d, dot(d, d)); }

// One sample of kSinglePix pixels per lane (get_ray + ray_color at depth <= 1).  seed[s] =
// 1 + n + B (wgsl:353) of pixel s; kUniRs: every live pixel holds the hinted count, and the
// scatter's random numbers come from p.rs.  Tiles: blk[s] = the tile's candidate block,
// ncand[s] its count (kCandNone: the full list; 0 for a tile past the image edge).
template <uint32_t S>
constexpr bool kSingleLds = RT_SINGLE_LDS == 2 || (RT_SINGLE_LDS == 1 && S == 1);
// single_sample's parameters for one frame of a frame group (rt_tpair_kernel)
struct FrameView {
    const float4* geom;
    const float4* sph;
    uint32_t count, depth, seed_b, normal_rn;
    float4 rs;
};
// A wave-uniform flag word where single_sample tests it.  In a frame loop the word is a loop
// invariant and so is its test: the compiler hoists the comparison and keeps the i1 as a
// 64-bit lane mask across the loop (in rt_tpair_kernel spilled to VGPR lanes: two v_readlane
// a frame per flag, and for normal_rn a v_cndmask + v_cmp_ne to turn the mask back into a
// branch condition).  Made opaque here, the word is tested where it is used, by s_cmp.  The
// one-frame kernels have no loop to hoist out of: their flags stay as they are.
// (kInFrameLoop: single_sample instantiated for a frame loop, i.e. with a FrameView)
template <typename P>
constexpr bool kInFrameLoop = false;
template <>
constexpr bool kInFrameLoop<FrameView> = true;
template <typename P>
__device__ __forceinline__ uint32_t flag_here(const P&, uint32_t x) {
    if (kInFrameLoop<P>) asm volatile("" : "+s"(x));
    return x;
}
// The list walk's start values (no hit: tmax 3.4e35, index -1) materialised where the walk
// starts.  As plain constants in a frame loop they are hoisted into four VGPRs that stay
// live across the loop, and the two tiles' values are copied from them as register pairs
// (two v_mov_b32 and two v_mov_b64 a frame).
__device__ __forceinline__ float walk_tmax_here() {
    float t;
    asm volatile("v_mov_b32 %0, 0x7a82f697" : "=v"(t));          // 0x1.05ed2ep+118f
    return t;
}
__device__ __forceinline__ int walk_idx_here() {
    int i;
    asm volatile("v_mov_b32 %0, -1" : "=v"(i));
    return i;
}
template <uint32_t S, bool kUniRs, typename P>
__device__ __forceinline__ void single_sample(const P& p, const Cam& cam,
                                              const TileCoord (&tc)[S],
                                              const uint32_t (&hxy)[S],
                                              const uint32_t (&seed)[S],
                                              const float4* const (&blk)[S],
                                              const uint32_t (&ncand)[S],
                                              const bool (&live)[S],
                                              const uint64_t (&live_m)[S],
                                              const float4 (&bv)[S], float4* lblk,
                                              v3 (&col)[S]) {
    constexpr int K = 1;    // records per tile and step of the joint list walk
    v3 o[S], d[S];
    // one VGPR copy of the lens centre for the S pixels (get_ray's c0v)
    v3 c0 = cam.center;
    if (S > 1) asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z));
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {                            // wgsl:311, 305-325
        get_ray<kSingleDisk>(cam, tc[s].x, tc[s].y, hxy[s], seed[s] * 25u + p.seed_b, o[s],
                             d[s], S > 1 ? &c0 : nullptr);
    }
    // (the frame loop keeps the shared copy live to here: where it died in the last pixel's
    // lens FMAs they were written over it, and three v_mov then carried the origin to where
    // the pinhole branch leaves it)
    if (S > 1 && kInFrameLoop<P>) asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z));
    SST_V(3, d[S - 1].x);
    const uint32_t lane = threadIdx.x & 63u;
    if (kSingleLds<S>) {
        // (this wave's own LDS slots: written and read by this wave only, in order)
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) lblk[s * kCandStride + lane] = bv[s];
    }
    v3 cf[S], dsky[S];
    float ddsky[S];                   // |dsky|^2 (sky_w's dd)
    bool black[S], any_other[S];      // (any_other: wave-uniform, a metal / dielectric hit)
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {
        cf[s] = mk(1.0f, 1.0f, 1.0f);
        dsky[s] = d[s];
        ddsky[s] = dot(d[s], d[s]);   // (wgsl:184's a as well)
        black[s] = false;
        any_other[s] = false;
    }
    if (flag_here(p, p.depth) != 0u) {                            // wgsl:264
        // sphere_list_hit over each tile's list, the tiles' chunks interleaved
        float tmax[S], a[S];
        int idx[S];
        bool joint = true;
        uint32_t m = 0;
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            tmax[s] = 0x1.05ed2ep+118f;                           // 3.4e35 (wgsl:266)
            idx[s] = -1;
            a[s] = ddsky[s];
            joint = joint && ncand[s] != kCandNone;
            m = max(m, ncand[s]);
        }
        if (joint) {
            if (kInFrameLoop<P>) {
#pragma unroll
                for (uint32_t s = 0; s < S; ++s) {
                    tmax[s] = walk_tmax_here();
                    idx[s] = walk_idx_here();
                }
            }
            // (walking the common length jointly and the longer list's rest alone measured
            // neutral: profiles/r06/r06av/)
            for (uint32_t i = 0; i < m; i += K) {
                float hh[S][K], dd[S][K];
                // "some discriminant of the step is not negative" as the sign of the AND of
                // their bit patterns (one 2-cycle v_and per record): exact on the camera-ray
                // domain the host proves for these instances — every discriminant is finite
                // (consider_fast) and never -0 (max_bits), so its sign bit is set exactly when
                // it is < 0
                uint32_t an = 0xFFFFFFFFu;
#pragma unroll
                for (uint32_t s = 0; s < S; ++s)
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float4 g =
                            kSingleLds<S> ? lblk[s * kCandStride + kCandRecOff + i + k]
                                          : load_rec<true>(blk[s] + kCandRecOff, i + k);
                        dd[s][k] = discriminant(g, o[s], d[s], a[s], hh[s][k]);
                        an &= __float_as_uint(dd[s][k]);
                    }
                if (__builtin_expect((int)an >= 0, 0)) {
#pragma unroll
                    for (uint32_t s = 0; s < S; ++s)
#pragma unroll
                        for (int k = 0; k < K; ++k)
                            if (i + k < ncand[s])
                                // (1 / a only where some discriminant is not negative:
                                // waves without candidates, the sky's, skip the v_rcp)
                                consider_fast(dd[s][k], hh[s][k], a[s], rcp_refined(a[s]), i + k, tmax[s],
                                              idx[s]);
                }
            }
        } else {
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) {
                const bool listed = ncand[s] != kCandNone;
                const Hit h = scan_exhaustive<K, true, true>(
                    listed ? blk[s] + kCandRecOff : p.geom, listed ? ncand[s] : p.count, o[s],
                    d[s]);
                idx[s] = h.idx;
                tmax[s] = h.t;
            }
        }
        SST_V(4, tmax[S - 1]);
        // hit records and the scatter (wgsl:205-218, 268-286)
        bool hit[S];
        bool any = false;
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            hit[s] = live[s] && idx[s] >= 0;
            any = any || hit[s];
        }
        uint64_t hm[S], any_m = 0;
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            // idx >= 0; in the frame loop written as the compiler writes the boolean's compare
            // above (idx > -1): the lane mask and hit[s] then come from one v_cmp instead of
            // one each (the one-frame kernels' code stays as it was measured)
            hm[s] = (kInFrameLoop<P> ? mask_sgt(idx[s], -1) : mask_sge(idx[s], 0)) & live_m[s];
            any_m |= hm[s];
        }
        if (any_m != 0ull) {
            float4 pr[S], mat[S];
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) {
                const uint32_t j = hit[s] ? (uint32_t)idx[s] : 0u;
                if (kSingleLds<S> && ncand[s] != kCandNone) {
                    pr[s] = lblk[s * kCandStride + kCandSphOff + 2u * j];
                    mat[s] = lblk[s * kCandStride + kCandSphOff + 2u * j + 1u];
                } else {
                    // the wave-uniform record array as a buffer, the lane's 32-bit byte offset
                    // (j < 2^20 spheres, rt_abi.cpp kMaxSpheres): no 64-bit address arithmetic
                    // per lane
                    const float4* hs = ncand[s] != kCandNone ? blk[s] + kCandSphOff : p.sph;
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                        (void*)hs, 0, (int)0x7FFFFFFF, 0x00020000);
                    pr[s] = buf_f4(rs, j * 32u);
                    mat[s] = buf_f4(rs, j * 32u + 16u);
                }
            }
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) {
                float r_sb;
                v3 ruv;
                if (kUniRs) {
                    r_sb = p.rs.x;
                    ruv = mk(p.rs.y, p.rs.z, p.rs.w);
                } else {
                    const uint32_t sb = hash(seed[s] + 1u);       // wgsl:268, 355 (i = 0)
                    r_sb = rf(sb);
                    ruv = random_unit_vector(r_sb, sb);
                }
                v3 nd, att;
                bool blk_s, other_s;
                float ndd;
                shade_hit(pr[s], mat[s], tmax[s], o[s], d[s], r_sb, ruv, hit[s], hm[s],
                          flag_here(p, p.normal_rn) != 0u, nd, att, blk_s, other_s, ndd);
                any_other[s] = other_s;
                if (hm[s] == live_m[s]) {
                    // every live lane hit (a tile inside a sphere's image): no selects
                    asm volatile("");
                    cf[s] = att;
                    dsky[s] = nd;
                    ddsky[s] = ndd;
                    black[s] = blk_s;
                } else if (hit[s]) {                              // wgsl:285-286
                    cf[s] = att;
                    dsky[s] = nd;
                    ddsky[s] = ndd;
                    black[s] = blk_s;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {
        const v3 c = sky_w(cf[s], dsky[s], ddsky[s]);             // wgsl:293-296
        // (black: only metal hits absorb, so only a wave that shaded one selects)
        if (!any_other[s]) {
            asm volatile("");
            col[s] = c;
        } else {
            col[s] = black[s] ? mk(0.0f, 0.0f, 0.0f) : c;         // wgsl:277-279
        }
    }
    SST_V(5, col[S - 1].x);
}

// A tile's flag word (kTileCertain and the class, rt_kernels.h) through the constant address
// space, as load_cnt reads the count beside it.
__device__ __forceinline__ uint32_t load_flags(const float4* cand, uint32_t tile) {
    return ((const kconst uint32_t*)cand)[(size_t)tile * (4u * kCandStride) + 2u];
}

// single_sample<2, true> of a frame loop for a pair of certain tiles (rt_occlusion.h): each
// tile's list is one sphere that every lane certainly hits from outside, on its front face,
// with its near root accepted — proven once per camera at list build.  What single_sample
// decides per lane and frame is therefore known: the walk ends with index 0 and the near
// root (consider_fast's first quotient, neither test taken), every live lane hits, the normal
// is the outward one, and the material is the tile's class cls[s], a scalar.  Straight-line:
// the scan record and the sphere record by scalar loads, no walk, no hit mask, no face test,
// and the class's scatter alone under a scalar branch.  On every live lane it runs the
// operations of single_sample and shade_hit on the same operands in the same order: the same
// bits (lanes outside the image compute values nobody reads, there as here).
template <typename P>
__device__ __forceinline__ void certain_sample(const P& p, const Cam& cam,
                                               const TileCoord (&tc)[2],
                                               const uint32_t (&hxy)[2],
                                               const uint32_t (&seed)[2],
                                               const float4* const (&blk)[2],
                                               const uint32_t (&cls)[2], const bool (&live)[2],
                                               const uint64_t (&live_m)[2], v3 (&col)[2]) {
    constexpr uint32_t S = 2;
    v3 o[S], d[S];
    v3 c0 = cam.center;                                           // (as single_sample)
    asm volatile("" : "+v"(c0.x), "+v"(c0.y), "+v"(c0.z));
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)                              // wgsl:311, 305-325
        get_ray<kSingleDisk>(cam, tc[s].x, tc[s].y, hxy[s], seed[s] * 25u + p.seed_b, o[s],
                             d[s], &c0);
    asm volatile("" ::"v"(c0.x), "v"(c0.y), "v"(c0.z));
    if (flag_here(p, p.depth) == 0u) {                            // wgsl:264: the sky alone
#pragma unroll
        for (uint32_t s = 0; s < S; ++s)
            col[s] = sky_w(mk(1.0f, 1.0f, 1.0f), d[s], dot(d[s], d[s]));
        return;
    }
    const float r_sb = p.rs.x;
    const v3 ruv = mk(p.rs.y, p.rs.z, p.rs.w);
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {
        const float a = dot(d[s], d[s]);                          // wgsl:184
        const float4 g = load_rec<true>(blk[s] + kCandRecOff, 0);
        const float4 pr = load_rec<true>(blk[s] + kCandSphOff, 0);
        const float4 mat = load_rec<true>(blk[s] + kCandSphOff, 1);
        float h;
        const float disc = discriminant(g, o[s], d[s], a, h);
        const float q = sqrt_core(disc + 0x1p-126f);              // consider_fast, accepted
        const float t = div_core(h - q, a, rcp_refined(a));
        const v3 hp = fmas(t, d[s], o[s]);                        // shade_hit, front face
        const v3 rel = sub(hp, mk(pr.x, pr.y, pr.z));
        v3 n;                                                     // wgsl:209
        if ((__builtin_amdgcn_fcmpf(min_abs3(rel), 0x1p-100f, 4) & live_m[s]) == 0ull) {
            const float y = rcp_refined(pr.w);
            n = normal_div(rel, pr.w, y, flag_here(p, p.normal_rn) != 0u);
        } else {
            n = divs(rel, pr.w);
        }
        const v3 att = mk(mat.x, mat.y, mat.z);
        if (cls[s] == kClassLambertian) {                         // wgsl:84-93
            v3 dir = add(n, ruv);
            float ndd = dot(dir, dir);
            if ((__builtin_amdgcn_fcmpf(ndd, 0x1.0c6f7ap-20f, 4) & live_m[s]) != 0ull) {
                asm volatile("");
                if (ndd < 0x1.0c6f7ap-20f) {                      // wgsl:89-91
                    dir = n;
                    ndd = dot(n, n);
                }
            }
            col[s] = sky_w(att, dir, ndd);
        } else {
            // (under the live lanes, as shade_hit's per-lane branch runs them: the wave-wide
            // operand checks of normalize_w see the same lanes)
            v3 nd = d[s], cf = att;
            float ndd = a;
            bool black = false;
            if (live[s]) {
                if (cls[s] == kClassMetal) {                      // wgsl:95-100
                    const v3 refl = fmas(mat.w, ruv, normalize_w<true>(reflect(d[s], n)));
                    black = !(dot(refl, n) > 0.0f);               // wgsl:277-279
                    nd = normalize_w<true>(refl);
                    ndd = dot(nd, nd);
                } else {                                          // wgsl:102-135, front face
                    cf = mk(1.0f, 1.0f, 1.0f);
                    const float ratio = 1.0f / mat.x;
                    const v3 u = normalize_w<true>(d[s]);
                    const float cos_t = fminf(dot(neg(u), n), 1.0f);
                    const float sin_t = sqrtf(fmaf(-cos_t, cos_t, 1.0f));
                    const bool cannot = ratio * sin_t > 1.0f;
                    const bool refl = cannot || reflectance(cos_t, ratio) > r_sb;
                    nd = normalize_w<true>(refl ? reflect(u, n) : refract(u, n, ratio));
                    ndd = dot(nd, nd);
                }
            }
            const v3 c = sky_w(cf, nd, ndd);
            col[s] = black ? mk(0.0f, 0.0f, 0.0f) : c;            // wgsl:277-279
        }
    }
}

// kReset: the frame resets the accumulator (camera_has_moved > 0.5, wgsl:345-350) — a
// separate kernel (rt_single_reset_kernel), so that the steady-state kernel carries no
// per-pixel selects between the loaded and the zero accumulator, and the reset kernel no
// accumulator load at all.
template <int kPix, bool kReset, bool kChain>
__device__ __forceinline__ void single_body(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const uint32_t* __restrict__ a_order, const SingleParams& p) {
    static_assert(kPix >= 1 && kPix <= 4, "1 to 4 tiles per wave");
    constexpr uint32_t S = kPix;
    WAVE_TRACE(0);
#if RT_SSTAMPS
    sst_put(8, __builtin_amdgcn_s_memrealtime());
    sst_put(0, __builtin_amdgcn_s_memtime());
#endif
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (a_width + 7u) >> 3;
    // frame chains: a segment whose go wait gave up drops its image stores (the frames must
    // not run before the caller's stream reached them; rt_chain_go_kernel)
    // (a system-scope load: no cache between it and the go kernel's store; waited for only
    // at the stores)
    const uint32_t aborted =
        kChain ? __builtin_amdgcn_readfirstlane(
                     __hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))
               : 0u;
    // workgroups by decreasing candidate-list load (wg_order, launch_wg_order): the
    // costliest are dispatched first and the cheap ones fill the tail
    uint32_t gx = blockIdx.x, lband = (p.lbands & 0xFFFFu) + blockIdx.y * (p.lbands >> 16);
    if (a_order) {   // (a leading, preloadable argument: one scalar load to the entry)
        const uint32_t pos = blockIdx.y * (kChain ? p.grid_x : gridDim.x) + blockIdx.x;
        const uint32_t e = __builtin_amdgcn_readfirstlane(a_order[pos]);
        gx = e & 0xFFFFu;
        lband = e >> 16;
    }
    SST_S(1, lband);
    const uint32_t tx0 = (gx * kSingleWg + wave) * S;
    const uint32_t band_first = a_bands & 0xFFFFu, band_step = (a_bands >> 16) & 0x7FFFu;
    TileCoord tc[S];
    uint32_t ncand[S], hxy[S];
    const float4* blk[S];
    float4 acc[S], bv[S];
    __shared__ float4 s_blk[kSingleWg * kPix * kCandStride];
    float4* lblk = s_blk + wave * S * kCandStride;
    constexpr bool kHash = (RT_SINGLE_HASH >> (kPix - 1)) & 1;
    uint32_t hy = 0u, hv = 0u;
    if (kHash) {
        // (all 64 lanes active here: ds_bpermute reads every lane)
        const uint32_t row = (band_first + lband * band_step) * RT_STRIPE_ROWS + lane - 8u * S;
        const bool col = lane < 8u * S;                           // (selects, no branch)
        hv = hash((col ? tx0 * 8u + lane : row) * (col ? 73u : 51u));    // wgsl:309-310
        hy = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((8u * S + (lane >> 3)) * 4u), (int)hv);
    } else {
        hy = a_hx[p.hy_off + min(band_first * RT_STRIPE_ROWS +
                                     lband * band_step * RT_STRIPE_ROWS + (lane >> 3),
                                 a_height - 1u)];
    }
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t tx = tx0 + s;
        const bool in = tx < tiles_x;
        const uint32_t tile = lband * tiles_x + (in ? tx : tx0);
        tc[s] = tile_coord(a_width, a_height, band_first, band_step, tx, lband, lane);
        blk[s] = a_cand + (size_t)tile * kCandStride;
        ncand[s] = in ? load_cnt(a_cand, tile) : 0u;
        const uint32_t hx =
            kHash ? (uint32_t)__builtin_amdgcn_ds_bpermute((int)((8u * s + (lane & 7u)) * 4u),
                                                           (int)hv)
                  : a_hx[min(tc[s].x, a_width - 1u)];
        hxy[s] = hx ^ hy;                                         // wgsl:309-310
    }
    uint64_t valid_m[S];        // (tc[s].valid as a lane mask)
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)
        valid_m[s] = mask_ult(tc[s].x, a_width) & mask_ult(tc[s].y, a_height);
    // (issued after the seed-table loads: vmcnt waits in issue order, and the camera rays
    // need the seeds long before the scan and the accumulation need these)
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)
        bv[s] = (kSingleLds<S> && tx0 + s < tiles_x) ? blk[s][lane]
                                                      : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // Frame chains (rt_chain.cpp): consecutive frames of a part are AQL packets with no
    // cache acquire between them, so the accumulator the previous frame stored (write-
    // through, sc1) is read with sc1 loads: this CU's L1 may hold lines of an older frame.
    if (kChain && !kReset) {
        const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
            (void*)a_in, 0, (int)0x7FFFFFFF, 0x00020000);
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                rin, (int)((tc[s].valid ? tc[s].idx : 0) * 16u), 0, 16);   // sc1, wgsl:339
            acc[s] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y),
                                 __uint_as_float(v.z), __uint_as_float(v.w));
        }
    } else {
#pragma unroll
        for (uint32_t s = 0; s < S; ++s)
            acc[s] = kReset ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)   // (discarded: no load)
                            : a_in[tc[s].valid ? tc[s].idx : 0];            // wgsl:339
    }
    if (tx0 >= tiles_x) return;
    SST_V(2, hxy[S - 1]);
    SST_S(2, ncand[S - 1]);

    Cam cam;
    cam.center = mk(p.center[0], p.center[1], p.center[2]);
    cam.vul = mk(p.vul[0], p.vul[1], p.vul[2]);
    cam.pdu = mk(p.pdu[0], p.pdu[1], p.pdu[2]);
    cam.pdv = mk(p.pdv[0], p.pdv[1], p.pdv[2]);
    cam.ddu = mk(p.ddu[0], p.ddu[1], p.ddu[2]);
    cam.ddv = mk(p.ddv[0], p.ddv[1], p.ddv[2]);
    cam.defocus_angle = p.defocus_angle;
    const uint32_t spp = p.spp;                                   // wgsl:343

    v3 c[S];
    uint32_t n[S];
    bool pending[S];
    bool any_pending = true;
    uint64_t pend_m = 0;        // (the lanes with pending pixels)
    if (p.hinted) {
        // Every pixel is expected to hold n_hint (the host's count bookkeeping): trace with
        // it while the accumulator loads are in flight, then verify.
        const uint32_t ng = p.n_hint;
        v3 col[S];
        if (ng < spp) {                                           // wgsl:352
            uint32_t seed[S];
            bool live[S];
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) {
                seed[s] = 1u + ng + p.seed_b;                     // wgsl:353
                live[s] = tc[s].valid;
            }
            single_sample<S, true>(p, cam, tc, hxy, seed, blk, ncand, live, valid_m, bv, lblk,
                                   col);
        }
        any_pending = false;
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            c[s] = kReset ? mk(0.0f, 0.0f, 0.0f) : mk(acc[s].x, acc[s].y, acc[s].z);
            n[s] = kReset ? 0u : f2u(acc[s].w);                   // wgsl:339-350
            pending[s] = tc[s].valid && n[s] != ng;               // a foreign count
            if (!kReset) pend_m |= mask_ne(n[s], ng) & valid_m[s];
            any_pending = any_pending || pending[s];
            if (ng < spp) {                                       // wgsl:352-357
                const v3 num = sub(col[s], c[s]);
                if (ng < kAccRnMax &&
                    (mask_ult(acc_min_bits(num), kAccOkDbl) & valid_m[s]) == 0ull) {
                    c[s] = acc_rn(c[s], num, (float)(ng + 1u), p.rcp_hint);
                } else {
                    const float k = (float)(ng + 1u);             // wgsl:356
                    c[s] = mk(c[s].x + num.x / k, c[s].y + num.y / k, c[s].z + num.z / k);
                }
                n[s] = ng + 1u;
            }
        }
    } else {
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            pending[s] = tc[s].valid;
            pend_m |= valid_m[s];
        }
    }
    const bool wave_pending = pend_m != 0ull;
    if (wave_pending) {
        // pixels whose count is not the hinted one (or no hint): traced with their own
        // count and per-pixel random numbers
        uint32_t seed[S];
        bool live[S];
        v3 col[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) {
            if (pending[s]) {
                c[s] = kReset ? mk(0.0f, 0.0f, 0.0f) : mk(acc[s].x, acc[s].y, acc[s].z);
                n[s] = kReset ? 0u : f2u(acc[s].w);
            }
            live[s] = pending[s] && n[s] < spp;                   // wgsl:352
            seed[s] = 1u + n[s] + p.seed_b;                       // wgsl:353
        }
        uint64_t live_m[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) live_m[s] = rt_ballot(live[s]);
        single_sample<S, false>(p, cam, tc, hxy, seed, blk, ncand, live, live_m, bv, lblk, col);
#pragma unroll
        for (uint32_t s = 0; s < S; ++s)
            if (live[s]) {                                        // wgsl:356-357
                const float k = (float)(n[s] + 1u);
                c[s] = mk(c[s].x + (col[s].x - c[s].x) / k, c[s].y + (col[s].y - c[s].y) / k,
                          c[s].z + (col[s].z - c[s].z) / k);
                n[s] += 1u;
            }
    }
    SST_V(6, c[S - 1].x);
    // write-through (sc1) stores: the lines leave the XCD's L2 as they are written, so the
    // launch ends with no dirty image lines to write back at the kernel boundary
    float4* band = p.out + (size_t)lband * RT_STRIPE_ROWS * a_width;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        band, 0, (int)(RT_STRIPE_ROWS * 16u * a_width), 0x00020000);
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)
    {                                                             // wgsl:362-363
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = {__float_as_uint(c[s].x), __float_as_uint(c[s].y),
                             __float_as_uint(c[s].z), __float_as_uint((float)n[s])};
            // no branch: a pixel past the image edge stores to an offset past the band's
            // buffer record, which the buffer unit drops
            const uint32_t off = ((lane >> 3) * a_width + tc[s].x) * 16u;
            const bool drop = !tc[s].valid || (kChain && aborted != 0u);
            __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (int)(drop ? 0x7FFFFFF0u : off), 0,
                                                   16);
        }
#if RT_SSTAMPS
    sst_put(7, __builtin_amdgcn_s_memtime());
    sst_put(9, __builtin_amdgcn_s_memrealtime());
    sst_put(10, __builtin_amdgcn_s_getreg((31 << 11) | 4));    // HW_ID
    sst_put(11, __builtin_amdgcn_s_getreg((31 << 11) | 20));   // XCC_ID
#endif
    WAVE_TRACE(1);
}

template <int kPix>
__global__ __launch_bounds__(64 * kSingleWg, RT_SINGLE_MIN_WAVES) void rt_single_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const uint32_t* __restrict__ a_order, const SingleParams p) {
    single_body<kPix, false, false>(a_cand, a_hx, a_in, a_width, a_height, a_bands, a_order, p);
}
template <int kPix>
__global__ __launch_bounds__(64 * kSingleWg, RT_SINGLE_MIN_WAVES) void rt_single_reset_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const uint32_t* __restrict__ a_order, const SingleParams p) {
    single_body<kPix, true, false>(a_cand, a_hx, a_in, a_width, a_height, a_bands, a_order, p);
}
// The same kernels for frame chains (rt_chain.cpp: one AQL packet per frame and part on
// context-owned HSA queues; accumulator loads sc1, see single_body).
template <int kPix>
__global__ __launch_bounds__(64 * kSingleWg, RT_SINGLE_MIN_WAVES) void rt_chain_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const uint32_t* __restrict__ a_order, const SingleParams p) {
    single_body<kPix, false, true>(a_cand, a_hx, a_in, a_width, a_height, a_bands, a_order, p);
}
template <int kPix>
__global__ __launch_bounds__(64 * kSingleWg, RT_SINGLE_MIN_WAVES) void rt_chain_reset_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const uint32_t* __restrict__ a_order, const SingleParams p) {
    single_body<kPix, true, true>(a_cand, a_hx, a_in, a_width, a_height, a_bands, a_order, p);
}
// A chain's first packet: wait until the caller's stream has reached the chain (its
// hipStreamWriteValue32 of `want` into *go, signal memory).  Bounded by `ticks` of
// s_memrealtime (100 MHz; rt_chain.cpp, default 10 s): a wait that gives up sets *abort
// (device memory: every later chain frame drops its image stores, so no frame runs before
// the caller's stream has reached it) and *gave_up (coherent host memory: the host fails the
// chain on its next call, rt_abi.cpp, and runs HIP launches from then on).  Vector stores.
__global__ __launch_bounds__(64) void rt_chain_go_kernel(const uint32_t* go, uint32_t want,
                                                         uint32_t* abort, uint32_t* gave_up,
                                                         uint64_t ticks) {
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    while (true) {
        const uint32_t v = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
        if ((int32_t)(v - want) >= 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > ticks) {
            if (threadIdx.x == 0u) {
                __hip_atomic_store(abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(gave_up, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            break;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}
// A chain's last packet (barrier bit: after every frame): the caller's stream, waiting in
// hipStreamWaitValue32 for `value`, continues.  A release store at system scope: the frames'
// stores are written back before the stream (or a copy engine, or RCCL over xGMI) reads on.
__global__ __launch_bounds__(64) void rt_chain_done_kernel(uint32_t* done, uint32_t value) {
    if (threadIdx.x == 0u)
        __hip_atomic_store(done, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- Frame groups over tile pairs (kTraceListPair2, kTraceListQuad2) -----------------
//
// The frame-group schedule of trace_pair (kFrameGroup waves, wave w traces frames f + w of
// each group, wave 0 accumulates through LDS) with the one-frame kernel's sample: each
// workgroup owns two horizontally adjacent tiles and each lane one pixel of each, the two
// tiles' candidate lists walked jointly (single_sample<2>) — two independent pixel chains per
// lane instead of one, and half the waves for the same work.  Called for launches whose
// every frame is hinted (rt_abi.cpp: the frame-group conditions); a workgroup whose loaded
// counts differ from the hint traces each tile with the general per-tile loop (waves 0 and
// 1).  Scheduling units (tile order, costs): tile pairs.  G: frames per group (2 or 4).
// Waves per SIMD the register plan targets: 7 (71 VGPRs, no scratch) — at 8 the compiler
// fits 64 VGPRs with 40 B of scratch per lane and 69 SGPR spills, and a whole-image 64-frame
// pair launch takes 14.94 against 14.27 us per frame (profiles/r05/r05af/ab_k3_fused.log).
#ifndef RT_TPAIR_MIN_WAVES
#define RT_TPAIR_MIN_WAVES 7
#endif
// (G an int: rocprofv3 lists the instances as rt_tpair_kernel<2> / <4>, rt_kernel_name's names)
template <int G>
__global__ __launch_bounds__(64 * G, RT_TPAIR_MIN_WAVES) void rt_tpair_kernel(
    const float4* __restrict__ a_cand, const uint32_t* __restrict__ a_hx,
    const float4* __restrict__ a_in, uint32_t a_width, uint32_t a_height, uint32_t a_bands,
    const TraceParams p) {
    WAVE_TRACE(0);
    constexpr uint32_t S = 2, Gu = (uint32_t)G;
    static_assert(!kSingleLds<S>, "the pair sample reads its records from the candidate blocks");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t tiles_x = (a_width + 7u) >> 3;
    const uint32_t units_x = (tiles_x + S - 1u) / S;
    uint32_t ux = blockIdx.x, lband = blockIdx.y;
    const uint32_t band_first = a_bands & 0xFFFFu, band_step = (a_bands >> 16) & 0x7FFFu;
    if (a_bands >> 31) {                                 // costliest units first (tile_order)
        const uint32_t t =
            __builtin_amdgcn_readfirstlane(p.tile_order[blockIdx.y * gridDim.x + blockIdx.x]);
        ux = t & 0xFFFFu;
        lband = t >> 16;
    }
    const uint32_t unit = lband * units_x + ux;
    const uint32_t tx0 = ux * S;
    TileCoord tc[S];
    uint32_t ncand[S], hxy[S], tile[S], tflags[S];
    const float4* blk[S];
    float4 acc[S];
    uint64_t valid_m[S];
#pragma unroll
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t tx = tx0 + s;
        const bool in = tx < tiles_x;
        tile[s] = lband * tiles_x + (in ? tx : tx0);
        tc[s] = tile_coord(a_width, a_height, band_first, band_step, tx, lband, lane);
        blk[s] = a_cand + (size_t)tile[s] * kCandStride;
        ncand[s] = in ? load_cnt(a_cand, tile[s]) : 0u;
        tflags[s] = in ? load_flags(a_cand, tile[s]) : 0u;
        acc[s] = a_in[tc[s].valid ? tc[s].idx : 0];               // wgsl:339
        hxy[s] = a_hx[min(tc[s].x, a_width - 1u)] ^                // wgsl:309-310
                 a_hx[hy_offset(a_width) + min(tc[s].y, a_height - 1u)];
        valid_m[s] = mask_ult(tc[s].x, a_width) & mask_ult(tc[s].y, a_height);
    }
    if (p.tile_cost && w == 0u && lane == 0u)
        p.tile_cost[unit] = (uint32_t)__builtin_amdgcn_s_memtime();
    const Cam cam = cam_params(p);
    const uint32_t n0 = p.hint_n[0];
    if (!p.reset_first &&
        rt_ballot((tc[0].valid && f2u(acc[0].w) != n0) || (tc[1].valid && f2u(acc[1].w) != n0)) !=
            0ull) {
        // a foreign count: wave s traces tile s frame after frame (stores every image itself)
        if (w < S && tx0 + w < tiles_x) {
            const float4 res = trace_pixel<kTraceListQuad, false>(
                p, cam, w ? tile[1] : tile[0], w ? ncand[1] : ncand[0], w ? tc[1] : tc[0],
                w ? hxy[1] : hxy[0], w ? acc[1] : acc[0]);
            const TileCoord& t = w ? tc[1] : tc[0];
            if (t.valid && !p.store_each) p.out[t.idx] = res;     // wgsl:363
        }
    } else {
        const uint32_t spp = p.spp;                               // wgsl:343
        // the tiles' accumulators stay in LDS between groups (no registers live across the
        // samples; the foreign-count fallback above sets the register peak)
        __shared__ float4 s_cols[2u * Gu * S * 64u];
        __shared__ float4 s_acc[S * 64u];
        if (w == 0u)
#pragma unroll
            for (uint32_t s = 0; s < S; ++s)
                s_acc[s * 64u + lane] = p.reset_first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f)
                                                      : acc[s];
        const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // both counts as signed bytes (a count is at most kCandMax, kCandNone is -1) and, from
        // bit 16, tile[1] - tile[0]: 1, or 0 where the partner tile is outside the image
        static_assert(kCandMax < 0x80u && kCandNone == 0xFFFFFFFFu, "a count fits a signed byte");
        // and, from bits 24 and 27, the tiles' flag words (certain, class: three bits each)
        const uint32_t unit_state =
            (ncand[0] & 0xFFu) | (ncand[1] & 0xFFu) << 8 | (tile[1] - tile[0]) << 16 |
            (tflags[0] & 7u) << 24 | (tflags[1] & 7u) << 27;
        constexpr uint32_t kPairCertain = kTileCertain << 24 | kTileCertain << 27;
        for (uint32_t f = 0; f < p.frames; f += Gu) {
            const uint32_t fw = f + w;
            // (single_sample writes every lane's colour; zeros only where nothing is traced)
            v3 col[S];
            const uint32_t ng = fw < p.frames ? p.hint_n[fw] : spp;  // count before frame fw
            if (ng >= spp) {
#pragma unroll
                for (uint32_t s = 0; s < S; ++s) col[s] = zero_v3_here();
            } else {                                              // wgsl:352
                {
                    FrameView v;
                    v.geom = p.geom;
                    v.sph = p.sph;
                    v.count = p.count;
                    v.depth = p.depth;
                    v.seed_b = p.seed_b[fw];
                    // (depth and normal_rn as words: single_sample tests them where it uses
                    // them, flag_here)
                    v.normal_rn = p.normal_rn;
                    v.rs = p.hint_rs[fw * p.depth];
                    uint32_t seed[S];
                    bool live[S];
                    const float4 bv[S] = {zero4, zero4};
#pragma unroll
                    for (uint32_t s = 0; s < S; ++s) {
                        seed[s] = 1u + ng + v.seed_b;             // wgsl:353
                        live[s] = tc[s].valid;
                    }
                    // the tiles' list pointers re-derived from the tile indices every frame
                    // (SALU) instead of staying live across the loop: 45 -> 28 SGPRs spilled
                    // to VGPR lanes, 30 -> 14 v_readlane in the loop; K3 13.60 -> 13.37 us per
                    // frame (tools/chain_ab.py, profiles/r06/r06ae/); re-reading the unit and
                    // the counts through the scalar cache every frame instead: 14.17 (r06af/).
                    // What stays live across the loop is two words, tile[0] and unit_state
                    // (both counts as signed bytes and the partner bit): tile[1], the
                    // pointers and the counts are SALU per frame (s_bfe_i32 sign-extends
                    // the kCandNone byte back to kCandNone); 6 -> 2 v_readlane a frame, 23
                    // SGPRs spilled (profiles/chain_trim/)
                    const float4* blkf[S];
                    uint32_t ncf[S];
                    uint32_t t0 = tile[0], st = unit_state;
                    asm volatile("" : "+s"(t0), "+s"(st));
#pragma unroll
                    for (uint32_t s = 0; s < S; ++s) {
                        const uint32_t t = t0 + (s ? (st >> 16) & 1u : 0u);
                        blkf[s] = a_cand + (size_t)t * kCandStride;
                        ncf[s] = (uint32_t)((int32_t)(st << (24u - 8u * s)) >> 24);
                    }
                    if ((st & kPairCertain) == kPairCertain) {
                        // both tiles certain: the straight-line sample (certain_sample)
                        const uint32_t cls[S] = {(st >> 25) & 3u, (st >> 28) & 3u};
                        certain_sample(v, cam, tc, hxy, seed, blkf, cls, live, valid_m, col);
                    } else {
                        single_sample<S, true>(v, cam, tc, hxy, seed, blkf, ncf, live, valid_m,
                                               bv, nullptr, col);
                    }
                }
            }
            // two LDS slots alternating by group (one barrier per group, as trace_pair): wave w
            // leaves its colour of tile t (frame f + w) in slot [w][t] unless it accumulates
            // that tile itself; wave t (< S) accumulates tile t's G frames in frame order —
            // the tiles' accumulation on two waves instead of all of it on wave 0.  The colours
            // as 12-B records (ds_write_b96: no register quad to fill with a zero).
            float4* slot = s_cols + ((f / Gu) & 1u) * Gu * S * 64u;
#pragma unroll
            for (uint32_t t = 0; t < S; ++t)
                if (w != t)
                    *reinterpret_cast<f3v*>(&slot[(w * S + t) * 64u + lane]) =
                        f3v{col[t].x, col[t].y, col[t].z};
            __syncthreads();
#pragma unroll
            for (uint32_t t = 0; t < S; ++t) {
                if (w != t) continue;                             // (wave-uniform)
#pragma unroll
                for (uint32_t j = 0; j < Gu; ++j) {
                    const uint32_t fj = f + j;
                    if (fj >= p.frames) break;
                    const uint32_t nb = p.hint_n[fj];             // count before frame fj
                    const bool acc_frame = nb < spp;              // wgsl:352-358
                    // f32(nb + 1) (the divisor k, wgsl:356) or f32(nb): the host's table
                    const float cnt = p.hint_cnt[fj];
                    float4* out = (fj & 1u) ? p.out2 : p.out;
                    const bool store = p.store_each == 2u || fj + 2u >= p.frames;
                    const float4 ca = s_acc[t * 64u + lane];
                    v3 cs = mk(ca.x, ca.y, ca.z);
                    v3 cj = col[t];
                    if (j != t) {
                        const float4 c4 = slot[(j * S + t) * 64u + lane];
                        cj = mk(c4.x, c4.y, c4.z);
                    }
                    if (acc_frame) {
                        const v3 num = sub(cj, cs);
                        // num / f32(nb + 1) (wgsl:356) as a Markstein division (acc_rn)
                        // (both conditions scalar, combined without a branch: a short-
                        // circuit && here kept nb's test in a VGPR)
                        const bool rn = (nb < kAccRnMax) &
                                        ((mask_ult(acc_min_bits(num), kAccOkDbl) &
                                          valid_m[t]) == 0ull);
                        if (rn) {
                            cs = acc_rn(cs, num, cnt, p.hint_rcp[fj]);
                        } else {
                            const float k = cnt;                     // wgsl:356
                            cs = mk(cs.x + num.x / k, cs.y + num.y / k, cs.z + num.z / k);
                        }
                    }
                    // (the alpha rides in the LDS copy: one register quad serves the LDS
                    // write and the image store)
                    const float4 v = make_float4(cs.x, cs.y, cs.z, cnt);
                    s_acc[t * 64u + lane] = v;
                    // wgsl:362-363: the images that survive (or every frame's)
                    if (store && tc[t].valid) out[tc[t].idx] = v;
                }
            }
        }
    }
    if (p.tile_cost && w == 0u && lane == 0u)
        p.tile_cost[unit] = (uint32_t)__builtin_amdgcn_s_memtime() - p.tile_cost[unit];
    WAVE_TRACE(1);
}

// ---- Bounce paths with workgroup-wide compaction (kTraceBounce) -----------------------
//
// rt_update_frames with bounce rays (max_depth >= 2), several frames per launch.  One
// workgroup = kBounceWaves waves = kBounceWaves consecutive 8x8 tiles of a stripe band; each
// lane owns one pixel and keeps its accumulator in registers across the launch's frames.
// Per frame the camera rays of a wave are its own tile's (candidate list or cone scan, as
// in the culled instance).  After every bounce the paths still alive in the workgroup are
// compacted: a ballot per wave, the popcounts combined through LDS into wave offsets, and
// mbcnt gives each live lane its slot; the path state (origin, direction, throughput, seed,
// owner) goes to LDS slot `prefix`, and the next bounce is traced by the first
// ceil(live / 64) waves only — the others wait at the barrier, their SIMD time free for
// other workgroups.  A path that ends (sky, absorbed, depth exhausted) writes its colour to
// its owner's LDS result slot; the owner accumulates it after the frame (wgsl:352-363).
// Every path runs exactly the reference's per-pixel arithmetic (ray_color, wgsl:261-297):
// only which lane executes it changes.  kBounceWaves = 4: a bounce's live paths of four
// tiles fill one wave where they filled four (K5: path lengths fall off geometrically, the
// longest of 64 lanes sets a wave's bounce count without compaction).
constexpr uint32_t kBounceLanes = 64 * kBounceWaves;
struct BounceLds {
    float4 po[kBounceLanes];   // origin, seed + 1 (bits) of the path in slot k
    float4 pd[kBounceLanes];   // direction, owner lane (bits)
    float4 pc[kBounceLanes];   // throughput
    float4 res[kBounceLanes];  // colour of the path owned by lane k
    uint32_t cnt[kBounceWaves];
};
__shared__ BounceLds s_bounce;


// One bounce of a path after its hit (wgsl:205-218 record, wgsl:268-286 scatter): the new
// direction and attenuation, or false when the metal scatter absorbs it.
struct Scatter {
    v3 hp, nd, att;
    bool ok;   // false: the metal scatter absorbed the path
};
// The divisions and square roots run on the exact fast cores where a wave-wide check of
// their operands allows (the camera-ray instances' checks, same bits): the normal's
// (p - C) / R by normal_div when every hit lane has |R| in [2^-20, 2^20] and its three
// numerators in [2^-100, 2^60] (div_core's domain; normal_rn: the scene's radii passed the
// one-step check), the metal / dielectric normalisations by normalize_w<true>.  (The
// dielectric's 1 / ir, reflectance division and square roots on the cores too measured
// neutral, K5 21.53 against 21.56 ms, and stay IEEE: profiles/r06/r06p/.)
__device__ __forceinline__ Scatter scatter_path(float4 pr, float4 mat, float t, v3 o, v3 d,
                                                float r_sb, v3 ruv, bool normal_rn) {
    // (results returned by value: out-parameters through references stayed in scratch)
    const v3 hp = fmas(t, d, o);
    v3 nd, att;
    const v3 rel = sub(hp, mk(pr.x, pr.y, pr.z));
    const uint32_t rel_lo = min(min(abs_bits(rel.x), abs_bits(rel.y)), abs_bits(rel.z));
    const uint32_t rel_hi = max(max(abs_bits(rel.x), abs_bits(rel.y)), abs_bits(rel.z));
    const bool nfast = rel_lo >= kBits2m100 && rel_hi <= 0x5D800000u &&            // 2^60
                       abs_bits(pr.w) - kBits2m20 <= 0x49800000u - kBits2m20;      // 2^20
    v3 outward;                                                                    // wgsl:209
    if (rt_ballot(!nfast) == 0ull)
        outward = normal_div(rel, pr.w, rcp_refined(pr.w), normal_rn);
    else
        outward = divs(rel, pr.w);
    const bool front = dot(d, outward) < 0.0f;
    // (component selects: a select of whole v3 values made the compiler keep them in
    // scratch memory)
    const v3 n = sel3(front, outward, neg(outward));
    if (mat.w < -1.0f) {                                      // lambertian wgsl:84-93
        const v3 dir = add(n, ruv);
        nd = sel3(dot(dir, dir) < 0x1.0c6f7ap-20f, n, dir);
        att = mk(mat.x, mat.y, mat.z);
    } else if (mat.w <= 1.0f) {                               // metal wgsl:95-100
        const v3 refl = fmas(mat.w, ruv, normalize_w<true>(reflect(d, n)));
        if (!(dot(refl, n) > 0.0f)) return Scatter{hp, d, d, false};   // wgsl:277-279
        nd = normalize_w<true>(refl);
        att = mk(mat.x, mat.y, mat.z);
    } else {                                                  // dielectric wgsl:102-135
        att = mk(1.0f, 1.0f, 1.0f);
        const float ratio = front ? 1.0f / mat.x : mat.x;
        const v3 u = normalize_w<true>(d);
        const float cos_t = fminf(dot(neg(u), n), 1.0f);
        const float sin_t = sqrtf(fmaf(-cos_t, cos_t, 1.0f));
        const bool cannot = ratio * sin_t > 1.0f;
        const bool refl = cannot || reflectance(cos_t, ratio) > r_sb;
        nd = normalize_w<true>(sel3(refl, reflect(u, n), refract(u, n, ratio)));
    }
    return Scatter{hp, nd, att, true};
}

// Sky colour of the final direction times the throughput (wgsl:293-296).
__device__ __forceinline__ v3 sky(v3 cf, v3 d) {
    const float uy = d.y / sqrtf(dot(d, d));
    const float a = 0.5f * (uy + 1.0f);
    const float om = 1.0f - a;
    return mul(cf, mk(fmaf(a, 0.5f, om), fmaf(a, 0x1.666666p-1f, om), fmaf(a, 1.0f, om)));
}

// Workgroup-wide prefix of `live` over the kBounceWaves waves: returns this lane's slot
// (valid when live) and the total.  Two barriers (counts written, counts read).
__device__ __forceinline__ uint32_t compact_slot(bool live, uint32_t wave, uint32_t& total) {
    const unsigned long long m = rt_ballot(live);
    if ((threadIdx.x & 63u) == 0u) s_bounce.cnt[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBounceWaves; ++w) {
        const uint32_t c = s_bounce.cnt[w];
        before += w < wave ? c : 0u;
        sum += c;
    }
    total = sum;
    return before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Register plan of the bounce instance.  The camera (per frame) and the grid parameters (per bounce scan) are re-read from the kernarg segment through a pointer
// the compiler cannot see through (scalar-cache hits), instead of staying live in SGPRs for
// the whole launch; with it a 7-wave plan fits 94 SGPRs (106 and 6 waves before).  K5 per
// 64-spp step (profiles/r03/r03f_ab_k5.log, two rounds): 31.3 ms as before, 29.7 reloading at 6
// waves, 28.8 reloading at 7 (the default), 30.2 at 8 (78 SGPRs, 53 spilled to VGPR lanes),
// 30.5 at 7 without reloading (81 spilled).
#ifndef RT_BOUNCE_MIN_WAVES
#define RT_BOUNCE_MIN_WAVES 7
#endif
// RT_BOUNCE_PRIO: the first RT_BOUNCE_PRIO workgroups of the cost order run at raised wave
// priority (s_setprio), 0 = off.  K5 per-rank prediction (profiles/r03/r03m_rank_sim_k5_*: two
// rounds of five 64-frame launches each, the same frames for every build): 8-rank share
// 74.7 µs per spp off, 72.6 with 512 (efficiency 0.745 -> 0.769), 73.5 with 2048; the
// whole image unchanged (445 µs per spp).
#ifndef RT_BOUNCE_PRIO
#define RT_BOUNCE_PRIO 512
#endif
__device__ __forceinline__ const kconst TraceParams* karg_bounce_params() {
    // rt_bounce_kernel's only argument: the TraceParams block at kernarg offset 0
    const kconst TraceParams* q =
        (const kconst TraceParams*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return q;
}
// Modes: kBounceWave — one-wave workgroups (one tile each: the finest unit for the
// cost-ordered schedule) whose paths stay in their lanes, colours in registers, no
// barriers; kBounceCompact — four-wave workgroups exchanging paths through LDS (above);
// kBouncePair — two waves per tile on alternate frames, wave 1 handing its colours to wave
// 0 through LDS, which accumulates both in order (the frame groups of the camera-ray
// instance, trace_pair): half as long a chain per wave, for small per-rank shares;
// kBounceSplit — one-wave workgroups, each tile's frames split into p.split consecutive
// chunks traced by separate waves (units (tile, chunk), the costliest tiles' chunks first):
// a chunk stores its frames' colours write-through, the wave whose arrival is the tile's
// last accumulates all of them in frame order (wgsl:352-363) and stores the images.  Small
// rank shares (a few waves per SIMD in per-wave mode) then run S times as many, S times
// shorter waves, so the launch no longer ends with SIMDs idle behind the costliest tiles'
// 64-frame chains.
constexpr int kBounceWave = 0, kBounceCompact = 1, kBouncePair = 2, kBounceSplit = 3;
template <int kMode>
constexpr uint32_t bounce_waves() {
    return kMode == kBounceCompact ? kBounceWaves : kMode == kBouncePair ? 2u : 1u;
}
__shared__ float4 s_pair_col[64];   // kBouncePair: wave 1's colours of the current pair
template <int kMode>
__global__ __launch_bounds__(64 * bounce_waves<kMode>(), RT_BOUNCE_MIN_WAVES) void
rt_bounce_kernel(const TraceParams p) {
    WAVE_TRACE(0);
    constexpr bool kCompact = kMode == kBounceCompact, kPair = kMode == kBouncePair;
    constexpr bool kSplit = kMode == kBounceSplit;
    constexpr uint32_t kW = bounce_waves<kMode>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = kW == 1u ? 0u : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t me = threadIdx.x;                    // lane in the workgroup
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    uint32_t gx = blockIdx.x, lband = blockIdx.y;       // group of kW tiles
    // kSplit: workgroup u = unit; the first p.split_tiles slots of the order (the costliest
    // tiles) run as p.split chunks each (slot u / S, chunk u % S), every later slot as one
    // unit (S = 1: the per-wave schedule); a one-dimensional grid of tiles + split_tiles *
    // (S - 1) units
    const uint32_t unit = blockIdx.y * gridDim.x + blockIdx.x;
    uint32_t S = 1u, chunk = 0u, slot = unit;
    bool ordered_units = false;
    if (kSplit && p.unit_order) {
        // the measured unit order (launch_unit_order): the costliest tiles split, every unit
        // placed by its own cost; the grid's units past the count exit at once
        if (unit >= __builtin_amdgcn_readfirstlane(*p.unit_count)) return;
        const uint32_t e = __builtin_amdgcn_readfirstlane(p.unit_order[unit]);
        gx = e & 0xFFFFu;
        lband = (e >> 16) & 0xFFFu;
        chunk = (e >> 28) & 7u;
        S = (e >> 31) ? p.split : 1u;
        ordered_units = true;
    } else if (kSplit) {
        const uint32_t su = p.split_tiles * p.split;
        if (unit < su) {
            S = p.split;
            slot = unit / S;
            chunk = unit % S;
        } else {
            slot = unit - su + p.split_tiles;
        }
        gx = slot % tiles_x;
        lband = slot / tiles_x;
    }
    const bool sp = kSplit && S > 1u;                   // (wave-uniform)
    if (p.tile_order && !ordered_units) {               // costliest groups first
        const uint32_t pos = slot;
        const uint32_t t = __builtin_amdgcn_readfirstlane(p.tile_order[pos]);
        gx = t & 0xFFFFu;
        lband = t >> 16;
#if RT_BOUNCE_PRIO
        // the costliest tiles' waves carry the launch's critical path (a small rank
        // share's launch lasts as long as its heaviest tile's frames): they win the
        // SIMD's instruction arbitration over the cheap waves that fill around them
        if (pos < RT_BOUNCE_PRIO) __builtin_amdgcn_s_setprio(2);
#endif
    }
    const uint32_t tx = kPair ? gx : gx * kW + wave;   // (pairs: both waves, one tile)
    const bool wave_in = tx < tiles_x;
    const TileCoord tc = tile_coord(p, wave_in ? tx : 0u, lband, lane);
    const bool valid = wave_in && tc.valid;
    if (p.lds_records) {                                // records for the cone culling
        for (uint32_t j = threadIdx.x; j < p.lds_records; j += 64u * kW) lds_recs[j] = p.geom[j];
    }
    constexpr uint32_t kTiles = kPair ? 1u : kW;        // tiles per workgroup
    const uint32_t group = lband * ((tiles_x + kTiles - 1u) / kTiles) + gx;
    if (p.tile_cost && threadIdx.x == 0u && chunk == 0u)
        p.tile_cost[group] = (uint32_t)__builtin_amdgcn_s_memtime();
    if (p.lds_records || kW > 1u) __syncthreads();
    const uint32_t tile = lband * tiles_x + (wave_in ? tx : 0u);
    const uint32_t ncand = (p.cand_k && wave_in) ? load_cnt(p.cand, tile) : kCandNone;
    const float4* blk = p.cand + (size_t)tile * kCandStride;
    const uint32_t hxy = p.hx[min(tc.x, p.width - 1u)] ^ p.hy[min(tc.y, p.height - 1u)];
    const uint32_t spp = p.spp, depth = p.depth;        // wgsl:343, 264
    // the pixel's accumulator (wgsl:339-341; a frame-0 reset discards it)
    v3 c = mk(0.0f, 0.0f, 0.0f);
    uint32_t n = 0u;
    if (!p.reset_first && valid) {
        const float4 acc = p.in[tc.idx];
        c = mk(acc.x, acc.y, acc.z);
        n = f2u(acc.w);
    }
    constexpr uint32_t kStep = kPair ? 2u : 1u;               // frames per iteration
    // kSplit: this chunk's frames [f_lo, f_hi), and the pixel's count before f_lo (the
    // count arithmetic of wgsl:345-362 over the frames before it, f32 round trip included)
    uint32_t f_lo = 0u, f_hi = p.frames;
    // kSplit: chunk 0 accumulates its frames in registers when none of them stores an image
    // (an image store of an early frame may go to the input buffer, p.out2, which the later
    // chunks read at their start); otherwise it stores colours like the others
    const uint32_t cs = sp ? (p.frames + S - 1u) / S : p.frames;
    const bool c0_regs = sp && cs < p.frames && p.store_each != 2u &&
                         !(p.store_each && p.frames - 2u < cs);
    if (sp) {
        f_lo = min(chunk * cs, p.frames);
        f_hi = min(f_lo + cs, p.frames);
        for (uint32_t f = 0; f < f_lo; ++f) {
            if (f == 0u && p.reset_first) n = 0u;
            n = f2u((float)(n < spp ? n + 1u : n));
        }
    }
    // (kSplit: this tile's colour rows, one 1-KB row per frame)
    const __amdgpu_buffer_rsrc_t col_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        p.split_col + ((size_t)lband * tiles_x + (wave_in ? tx : 0u)) * p.frames * 64u, 0,
        (int)(p.frames * 1024u), 0x00020000);
    for (uint32_t f0 = f_lo; f0 < f_hi; f0 += kStep) {
        if (f0 == 0 && p.reset_first) {                           // wgsl:345-350
            c = mk(0.0f, 0.0f, 0.0f);
            n = 0u;
        }
        // this wave's frame and the pixel's count before it (pairs: wave 1 takes the next
        // frame, whose count follows from wgsl:352-362 with the f32 round trip)
        const uint32_t f = f0 + (kPair ? wave : 0u);
        const uint32_t n_next = f2u((float)(n < spp ? n + 1u : n));
        const uint32_t nf = (kPair && wave == 1u) ? n_next : n;
        const bool frame_in = f < p.frames;
        const uint32_t B = p.seed_b[frame_in ? f : f0];           // wgsl:311, 353
        const bool sampling = valid && frame_in && nf < spp;      // wgsl:352
        const uint32_t seed = 1u + nf + B;                        // wgsl:353
        // every sampling pixel of the wave at the hinted count of frame f: the scatter's
        // random numbers (pixel-independent given the count) come from hint_rs_dev
        // (compaction moves paths between waves: it keeps computing them)
        const bool uni_rs = !kCompact && f < p.hint_rs_dev_frames &&
                            rt_ballot(sampling && nf != p.hint_n[f]) == 0ull;
        BCOUNT(uni_rs ? 12 : 16);
        v3 res = mk(0.0f, 0.0f, 0.0f);                            // this pixel's colour
        if (kCompact) s_bounce.res[me] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        // bounce 0: this wave's own camera rays (wgsl:305-325), its tile's scan
        v3 o, d, cf = mk(1.0f, 1.0f, 1.0f);
        const Cam cam = cam_params(*karg_bounce_params());
        get_ray<kSingleDisk>(cam, tc.x, tc.y, hxy, seed * 25u + B, o, d);
        uint32_t pseed = seed + 1u;                               // ray_color's seed
        bool live = sampling;
        uint32_t owner = me;
        if (depth == 0u && live) {                                // no bounce: the sky
            res = sky(cf, d);
            if (kCompact) s_bounce.res[me] = make_float4(res.x, res.y, res.z, 0.0f);
        }
        for (uint32_t i = 0; i < depth; ++i) {
            // this wave's paths of bounce i (slot = lane for i == 0)
            Hit hit{-1, 0.0f};
            const float4* hs = p.sph;
            if (rt_ballot(live) != 0ull) {
                const bool listed = i == 0u && ncand != kCandNone;
                BCOUNT(i == 0u ? 6 : 8);
                const GridP gp = grid_params(*karg_bounce_params());
                if (listed) {
                    // the tile's camera rays: consider_fast's roots where the wave is in
                    // their domain (roots_fast_wave), the IEEE ones otherwise
                    if (roots_fast_wave(p.roots_fast, o, dot(d, d), live))
                        hit = scan_exhaustive<RT_BOUNCE_LIST_CHUNK, true, true>(blk + kCandRecOff,
                                                                         ncand, o, d);
                    else
                        hit = scan_exhaustive<RT_BOUNCE_LIST_CHUNK, false, true>(blk + kCandRecOff,
                                                                          ncand, o, d);
                } else {
                    hit = p.lds_records
                              ? scan_culled<true>(gp, p.geom, p.count, o, d, live, i > 0)
                              : scan_culled<false>(gp, p.geom, p.count, o, d, live, i > 0);
                }
                if (listed) hs = blk + kCandSphOff;
            }
            bool done = false, keep = false;
            v3 col = mk(0.0f, 0.0f, 0.0f);
            if (live) {
                if (hit.idx < 0) {                                // wgsl:288-290: sky
                    done = true;
                    col = sky_w(cf, d);
                } else {
                    const float4 pr = hs[2 * hit.idx], mat = hs[2 * hit.idx + 1];
                    // the scatter's random numbers (wgsl:268, 234-243): from the device
                    // table when every path of the wave is at the hinted count
                    float r_sb;
                    v3 ruv;
                    if (uni_rs) {
                        const float4 hr =
                            ((const kconst float4*)p.hint_rs_dev)[f * depth + i];
                        r_sb = hr.x;
                        ruv = mk(hr.y, hr.z, hr.w);
                    } else {
                        const uint32_t sb = hash(pseed + i * 1000u);
                        r_sb = rf(sb);
                        ruv = random_unit_vector(r_sb, sb);
                    }
                    BCOUNT(10);
                    const Scatter sc = scatter_path(pr, mat, hit.t, o, d, r_sb, ruv,
                                                    p.normal_rn != 0u);
                    const v3 hp = sc.hp, nd = sc.nd, att = sc.att;
                    if (!sc.ok) {
                        done = true;                              // absorbed: black
                    } else {
                        cf = mul(cf, att);                        // wgsl:285-286
                        o = hp;
                        d = nd;
                        if (i + 1u == depth) {                    // depth exhausted: sky
                            done = true;
                            col = sky_w(cf, d);
                        } else {
                            keep = true;
                        }
                    }
                }
                if (done) {
                    if (kCompact)
                        s_bounce.res[owner] = make_float4(col.x, col.y, col.z, 0.0f);
                    else
                        res = col;
                }
            }
            if (!kCompact) {                                      // paths stay in their lane
                live = keep;
                if (rt_ballot(keep) == 0ull) break;
                continue;
            }
            // compact the surviving paths into the first slots (uniform trip count)
            uint32_t total;
            const uint32_t slot = compact_slot(keep, wave, total);
            if (keep) {
                s_bounce.po[slot] = make_float4(o.x, o.y, o.z, __uint_as_float(pseed));
                s_bounce.pd[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(owner));
                s_bounce.pc[slot] = make_float4(cf.x, cf.y, cf.z, 0.0f);
            }
            __syncthreads();
            if (total == 0u) break;                               // workgroup-uniform
            live = me < total;
            if (live) {
                const float4 a = s_bounce.po[me], b = s_bounce.pd[me], e = s_bounce.pc[me];
                o = mk(a.x, a.y, a.z);
                pseed = __float_as_uint(a.w);
                d = mk(b.x, b.y, b.z);
                owner = __float_as_uint(b.w);
                cf = mk(e.x, e.y, e.z);
            }
            __syncthreads();                                      // slots read
        }
        if (kCompact) {
            __syncthreads();                                      // results written
            const float4 r = s_bounce.res[me];
            res = mk(r.x, r.y, r.z);
        }
        if (kPair) {                                              // wave 1's colour to wave 0
            if (wave == 1u) s_pair_col[lane] = make_float4(res.x, res.y, res.z, 0.0f);
            __syncthreads();
        }
        if (sp && (chunk != 0u || !c0_regs)) {
            // the frame's colour, write-through (sc1): the tile's last arriver reads it
            // (chunk 0 accumulates its frames in registers, as the per-wave mode does)
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 v = {__float_as_uint(res.x), __float_as_uint(res.y),
                             __float_as_uint(res.z), 0u};
            __builtin_amdgcn_raw_buffer_store_b128(v, col_rsrc, (int)((f0 * 64u + lane) * 16u),
                                                   0, 16);
            n = f2u((float)(n < spp ? n + 1u : n));
            continue;
        }
        // accumulate this iteration's frames in order (pairs: wave 0 does both; wave 1 only
        // follows the count)
        for (uint32_t j = 0; j < kStep; ++j) {
            const uint32_t fj = f0 + j;
            if (fj >= p.frames) break;
            if (!kPair || wave == 0u) {
                v3 col = res;
                if (kPair && j == 1u) {
                    const float4 r = s_pair_col[lane];
                    col = mk(r.x, r.y, r.z);
                }
                // wgsl:352, 356-357; num / f32(n + 1) as the Markstein step from the host's
                // RN32(1 / f32(n + 1)) (acc_rn) when every accumulating pixel of the wave holds
                // the hinted count (a reset launch's pixels all do), else the IEEE division
                const bool acc = valid && n < spp;
                const v3 num = sub(col, c);
                if (fj < p.hint_acc_frames && p.hint_n[fj] < kAccRnMax &&
                    rt_ballot(acc && (n != p.hint_n[fj] || !acc_ok(num))) == 0ull) {
                    if (acc) c = acc_rn(c, num, (float)(n + 1u), p.hint_rcp[fj]);
                } else if (acc) {
                    const float k = (float)(n + 1u);
                    c = mk(c.x + num.x / k, c.y + num.y / k, c.z + num.z / k);
                }
                // the images of the launch's last two frames survive (wgsl:362-363): frame
                // fj's image belongs to out for even fj, out2 (the input buffer) for odd fj
                // (store_each; 2: every frame's image is stored); otherwise only the last
                // frame's, to out
                if (valid && (fj + 1u == p.frames ||
                              (p.store_each && (p.store_each == 2u || fj + 2u == p.frames)))) {
                    float4* dst = (p.store_each && (fj & 1u)) ? p.out2 : p.out;
                    dst[tc.idx] = make_float4(c.x, c.y, c.z, (float)(n < spp ? n + 1u : n));
                }
            }
            n = f2u((float)(n < spp ? n + 1u : n));
        }
        if (kCompact || kPair) __syncthreads();                   // LDS reused next frame
    }
    if (sp) {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        // chunk 0 leaves its accumulator after its frames (colour and count: the state every
        // later frame starts from) in row 0, which holds no colour of its own
        if (chunk == 0u && c0_regs) {
            const u32x4 v = {__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), n};
            __builtin_amdgcn_raw_buffer_store_b128(v, col_rsrc, (int)(lane * 16u), 0, 16);
        }
        // arrival: every colour of this chunk has left the CU (sc1 stores, drained), then one
        // agent-scope add; the tile's last arriver (told by the add's value) reads the other
        // chunks' colours with sc1 loads (MI355X_MICROARCH.md, inter-workgroup visibility,
        // first row of the hand-off table) and accumulates their frames in order after chunk
        // 0's state
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t* cnt = p.split_cnt + (size_t)lband * tiles_x + (wave_in ? tx : 0u);
        uint32_t old = 0u;
        if (lane == 0u) old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
        old = __builtin_amdgcn_readlane(old, 0);
        if (old + 1u == S) {
            if (lane == 0u)    // (the next launch starts after this one ends)
                __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!c0_regs) {      // every frame's colour is in the buffer
                c = mk(0.0f, 0.0f, 0.0f);
                n = 0u;
                if (!p.reset_first && valid) {
                    const float4 acc = p.in[tc.idx];
                    c = mk(acc.x, acc.y, acc.z);
                    n = f2u(acc.w);
                }
            } else if (chunk != 0u) {   // (chunk 0 arriving last holds its state in registers)
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(col_rsrc, (int)(lane * 16u),
                                                                      0, 16);
                c = mk(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z));
                n = v.w;
            }
            // the colours of the frames after chunk 0's state in batches of kMergeBatch
            // frames, all of a batch's loads in flight before its accumulation (one dependent
            // load per frame made the merge as long as 64 load latencies)
            constexpr uint32_t kMergeBatch = 8;
            for (uint32_t f0 = c0_regs ? cs : 0u; f0 < p.frames; f0 += kMergeBatch) {
                u32x4 v[kMergeBatch];
#pragma unroll
                for (uint32_t j = 0; j < kMergeBatch; ++j)   // (rows past the last frame:
                    v[j] = __builtin_amdgcn_raw_buffer_load_b128(   // dropped by the buffer)
                        col_rsrc, (int)(((f0 + j) * 64u + lane) * 16u), 0, 16);
#pragma unroll
                for (uint32_t j = 0; j < kMergeBatch; ++j) {
                    const uint32_t fj = f0 + j;
                    if (fj >= p.frames) break;
                    if (fj == 0u && p.reset_first) {              // wgsl:345-350
                        c = mk(0.0f, 0.0f, 0.0f);
                        n = 0u;
                    }
                    const v3 col = mk(__uint_as_float(v[j].x), __uint_as_float(v[j].y),
                                      __uint_as_float(v[j].z));
                    if (valid && n < spp) {                       // wgsl:352, 356-357
                        const float k = (float)(n + 1u);
                        c = mk(c.x + (col.x - c.x) / k, c.y + (col.y - c.y) / k,
                               c.z + (col.z - c.z) / k);
                    }
                    // wgsl:362-363, the same images as the per-wave mode
                    if (valid && (fj + 1u == p.frames ||
                                  (p.store_each && (p.store_each == 2u || fj + 2u == p.frames)))) {
                        float4* dst = (p.store_each && (fj & 1u)) ? p.out2 : p.out;
                        dst[tc.idx] = make_float4(c.x, c.y, c.z, (float)(n < spp ? n + 1u : n));
                    }
                    n = f2u((float)(n < spp ? n + 1u : n));
                }
            }
        }
    }
    // (a split tile's cost: its chunk 0's duration times S, the chunks carrying equal frames,
    // so that the next launch's order ranks it with the unsplit tiles)
    if (p.tile_cost && threadIdx.x == 0u && chunk == 0u)
        p.tile_cost[group] =
            ((uint32_t)__builtin_amdgcn_s_memtime() - p.tile_cost[group]) * S;
    WAVE_TRACE(1);
}

// launch_tile_order: one 1024-thread workgroup; bucket = quantised log2 of the cost (four
// buckets per octave).  Each wave counts its tiles into its own LDS histogram (atomics only
// contend inside a wave), one block-wide scan over the [bucket][wave] counts turns them
// into offsets, costliest bucket first, and each tile is placed at its wave's next slot of
// its bucket (order inside a bucket is arbitrary: tiles are independent).
// parts > 1: the sorted list is dealt round-robin into `parts` contiguous sub-lists (entry
// pos to part pos % parts), one per concurrent part of a one-frame update (launch_single):
// every part gets the same mix of costly and cheap workgroups, costliest first.
// dealt (non-null): a second copy of the list dealt into dealt_parts sub-lists (the chain
// parts of rt_update_frames, which run beside launches that use the undealt list).
__device__ __forceinline__ uint32_t part_pos(uint32_t pos, uint32_t n, uint32_t parts) {
    if (parts <= 1u) return pos;
    const uint32_t k = pos % parts, j = pos / parts;
    return k * (n / parts) + min(k, n % parts) + j;
}
__global__ __launch_bounds__(1024) void rt_tile_order_kernel(const uint32_t* __restrict__ cost,
                                                             uint32_t* __restrict__ order,
                                                             uint32_t tiles, uint32_t tiles_x,
                                                             uint32_t parts,
                                                             uint32_t* __restrict__ dealt,
                                                             uint32_t dealt_parts) {
    constexpr uint32_t kBuckets = 128, kWaves = 16, kSlots = kBuckets * kWaves;
    __shared__ uint32_t hist[kSlots];          // [bucket][wave]
    __shared__ uint32_t scan[1024];
    auto bucket = [](uint32_t c) -> uint32_t {
        if (c == 0u) return kBuckets - 1u;
        const uint32_t lz = (uint32_t)__builtin_clz(c);
        const uint32_t e = 31u - lz;
        const uint32_t m = e >= 2u ? (c >> (e - 2u)) & 3u : (c << (2u - e)) & 3u;
        return kBuckets - 1u - (e * 4u + m);          // descending cost
    };
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    hist[2 * tid] = 0u;
    hist[2 * tid + 1] = 0u;
    __syncthreads();
    // (loads in batches of 8 per thread: one memory latency per batch, not per tile)
    constexpr uint32_t kBatch = 8;
    for (uint32_t t0 = tid; t0 < tiles; t0 += 1024u * kBatch) {
        uint32_t c[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t t = t0 + k * 1024u;
            c[k] = t < tiles ? cost[t] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k)
            if (t0 + k * 1024u < tiles) atomicAdd(&hist[bucket(c[k]) * kWaves + wave], 1u);
    }
    __syncthreads();
    // exclusive scan of the 2048 counts: pairs per thread, Hillis-Steele over the threads
    const uint32_t a0 = hist[2 * tid], a1 = hist[2 * tid + 1];
    uint32_t v = a0 + a1;
    scan[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t add = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        v += add;
        scan[tid] = v;
        __syncthreads();
    }
    const uint32_t before = v - a0 - a1;               // exclusive prefix of the pair
    hist[2 * tid] = before;
    hist[2 * tid + 1] = before + a0;
    __syncthreads();
    for (uint32_t t0 = tid; t0 < tiles; t0 += 1024u * kBatch) {
        uint32_t c[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t t = t0 + k * 1024u;
            c[k] = t < tiles ? cost[t] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            const uint32_t t = t0 + k * 1024u;
            if (t < tiles) {
                const uint32_t pos = atomicAdd(&hist[bucket(c[k]) * kWaves + wave], 1u);
                const uint32_t e = ((t / tiles_x) << 16) | (t % tiles_x);
                order[part_pos(pos, tiles, parts)] = e;
                if (dealt) dealt[part_pos(pos, tiles, dealt_parts)] = e;
            }
        }
    }
}

hipError_t launch_tile_order(const uint32_t* tile_cost, uint32_t* tile_order, uint32_t tiles,
                             uint32_t tiles_x, hipStream_t stream, uint32_t parts,
                             uint32_t* dealt, uint32_t dealt_parts) {
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_tile_order_kernel, dim3(1), dim3(1024), 0, stream, tile_cost,
                       tile_order, tiles, tiles_x, parts, dealt, dealt_parts);
    return hipGetLastError();
}

// The units of a launch in raster order, dealt round-robin into `parts` sub-lists (the chain
// parts of a generation whose costs are not measured yet).
__global__ __launch_bounds__(256) void rt_raster_order_kernel(uint32_t* __restrict__ order,
                                                              uint32_t units, uint32_t units_x,
                                                              uint32_t parts) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < units) order[part_pos(t, units, parts)] = ((t / units_x) << 16) | (t % units_x);
}
hipError_t launch_raster_order(uint32_t* order, uint32_t units, uint32_t units_x, uint32_t parts,
                               hipStream_t stream) {
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_raster_order_kernel, dim3((units + 255u) / 256u), dim3(256), 0, stream,
                       order, units, units_x, parts);
    return hipGetLastError();
}

// launch_unit_order: the split bounce schedule's units by their own recorded cost (one
// 1024-thread workgroup, the buckets of rt_tile_order_kernel).  A tile whose cost exceeds
// thr = k_thr * (sum of all costs) — k_thr = alpha / (resident waves of the launch), i.e. alpha
// times the launch's ideal span — becomes S chunk units of cost / S (its bucket moves 4 * log2 S
// places: four per octave), every other tile one unit; the units are then placed costliest
// first, a split tile's chunks side by side, so the tail after the last dispatch is bounded by
// the costliest unit rather than by the costliest tile (longest-processing-time-first on the
// units).  *count = the number of units.
__global__ __launch_bounds__(1024) void rt_unit_order_kernel(const uint32_t* __restrict__ cost,
                                                             uint32_t* __restrict__ order,
                                                             uint32_t* __restrict__ count,
                                                             uint32_t tiles, uint32_t tiles_x,
                                                             uint32_t S, float k_thr) {
    constexpr uint32_t kBuckets = 128, kWaves = 16;
    __shared__ uint32_t hist[kBuckets * kWaves];       // [bucket][wave]
    __shared__ uint32_t scan[1024];
    __shared__ unsigned long long total;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const uint32_t shift = 4u * (31u - (uint32_t)__builtin_clz(S));   // 4 * log2 S (S = 2^k)
    auto bucket = [](uint32_t c) -> uint32_t {
        if (c == 0u) return kBuckets - 1u;
        const uint32_t lz = (uint32_t)__builtin_clz(c);
        const uint32_t e = 31u - lz;
        const uint32_t m = e >= 2u ? (c >> (e - 2u)) & 3u : (c << (2u - e)) & 3u;
        return kBuckets - 1u - (e * 4u + m);          // descending cost
    };
    hist[2 * tid] = 0u;
    hist[2 * tid + 1] = 0u;
    if (tid == 0u) total = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (uint32_t t = tid; t < tiles; t += 1024u) mine += cost[t];
    atomicAdd(&total, mine);
    __syncthreads();
    const double thr_d = (double)total * (double)k_thr;
    const uint32_t thr = thr_d >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)thr_d;
    auto unit_bucket = [&](uint32_t c, bool& split) -> uint32_t {
        split = S > 1u && c > thr;
        const uint32_t b = bucket(c);
        return split ? min(b + shift, kBuckets - 1u) : b;
    };
    for (uint32_t t = tid; t < tiles; t += 1024u) {
        bool split;
        const uint32_t b = unit_bucket(cost[t], split);
        atomicAdd(&hist[b * kWaves + wave], split ? S : 1u);
    }
    __syncthreads();
    const uint32_t a0 = hist[2 * tid], a1 = hist[2 * tid + 1];
    uint32_t v = a0 + a1;
    scan[tid] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t add = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        v += add;
        scan[tid] = v;
        __syncthreads();
    }
    const uint32_t before = v - a0 - a1;
    hist[2 * tid] = before;
    hist[2 * tid + 1] = before + a0;
    if (tid == 1023u) *count = v;                      // (the inclusive total)
    __syncthreads();
    for (uint32_t t = tid; t < tiles; t += 1024u) {
        bool split;
        const uint32_t b = unit_bucket(cost[t], split);
        const uint32_t n = split ? S : 1u;
        const uint32_t pos = atomicAdd(&hist[b * kWaves + wave], n);
        const uint32_t e = (split ? 0x80000000u : 0u) | ((t / tiles_x) << 16) | (t % tiles_x);
        for (uint32_t k = 0; k < n; ++k) order[pos + k] = e | (k << 28);
    }
}

hipError_t launch_unit_order(const uint32_t* tile_cost, uint32_t* unit_order,
                             uint32_t* unit_count, uint32_t tiles, uint32_t tiles_x,
                             uint32_t split, float k_thr, hipStream_t stream) {
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_unit_order_kernel, dim3(1), dim3(1024), 0, stream, tile_cost,
                       unit_order, unit_count, tiles, tiles_x, split, k_thr);
    return hipGetLastError();
}

// Per-workgroup candidate-list load of one-frame launches (wg_order's sort key): the sum of
// its `per` tiles' loads (4 + count for a tile with a list, 64 for a tile without one).
__global__ __launch_bounds__(256) void rt_wg_cost_kernel(const float4* __restrict__ cand,
                                                         uint32_t tiles_x, uint32_t cols,
                                                         uint32_t per, uint32_t units,
                                                         uint32_t* __restrict__ cost) {
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u >= units) return;
    const uint32_t b = u / cols, g = u % cols;
    uint32_t sum = 1u;                                  // (cost 0 sorts last)
    for (uint32_t k = 0; k < per; ++k) {
        const uint32_t tx = g * per + k;
        if (tx >= tiles_x) break;
        const uint32_t c = load_cnt(cand, b * tiles_x + tx);
        sum += c == kCandNone ? 64u : (c ? 4u + c : 0u);
    }
    cost[u] = sum;
}

// List the spheres the camera rays of each tile can hit (see footprint_beam).
// One wave per block of 8 x 8 tiles (8 columns of tiles x 8 local bands), one lane per
// tile.  The wave first tests the spheres, 64 at a time, against the cone of the whole
// block's footprint and stages the survivors (scan + sphere records, index order) in LDS,
// kCandStage spheres per pass with all their loads in flight together; then every lane
// tests the staged spheres against its own
// tile's cone, one sphere per step (an LDS broadcast), appending hits to its tile's list.
// A sphere the block cone rejects provably misses every camera ray of the block (the same
// exact margins as the tile test), so the lists hold every sphere a camera ray of the tile
// can hit, in index order, and the scans over them return the full scan's bits.  (A block
// whose cone is degenerate stages every sphere.)  Per tile the cone setup is done once per
// lane and a sphere costs one cone test, instead of 64 lanes repeating the setup and
// testing all spheres per tile.
// occl (rt_set_occlusion_cull, and the host's camera_rays_bounded and scene bound hold): each
// lane then drops from its finished list the entries that another entry of the list hides
// from every camera ray of the tile (rt_occlusion.h: the entry with the smallest upper bound
// on its near root among those every ray certainly hits hides every entry whose lower bound
// exceeds it), closes the gaps in place (index order kept, each entry's sphere record beside
// its scan record as before) and leaves the number dropped in the count word's .y (u32 bits;
// rt_occlusion_cull_stats).  A tile without a list, or whose cone is degenerate, is left alone.
// occl bit 1 (rt_set_certain_tiles, with bit 0 only): a tile whose list is then one entry that
// every ray certainly hits on its front face is flagged certain, with the entry's material
// class, in the count word's .z (rt_occlusion.h certainly_front; rt_certain_tiles_stats).
// occl bit 2 (rt_set_tight_bundle off): the block's and the tiles' bundles are the single cone
// with the wider lens radius instead of the two-slope beam (footprint_beam's `parent`).
#ifndef RT_CAND_BX
#define RT_CAND_BX 8
#endif
#ifndef RT_CAND_BY
#define RT_CAND_BY 8
#endif
constexpr uint32_t kCandBX = RT_CAND_BX;   // block width in tiles
constexpr uint32_t kCandBY = RT_CAND_BY;   // block height in local bands (kCandBX * kCandBY <= 64)
static_assert(kCandBX * kCandBY <= 64, "one lane per tile");
constexpr uint32_t kCandGroup = 8;                 // blocks of 64 spheres per pass
constexpr uint32_t kCandStage = 64 * kCandGroup;   // spheres per pass
__global__ __launch_bounds__(64) void rt_candidates_kernel(const TraceParams p,
                                                           float4* __restrict__ cand,
                                                           const uint32_t occl) {
    __shared__ float4 s_rec[kCandStage];
    __shared__ float4 s_sph[2 * kCandStage];
    __shared__ uint32_t s_idx[kCandStage];
    // the occlusion pass's copy of each lane's list and of its entries' lower bounds (a lane
    // reads its own slots only)
    __shared__ float4 s_own[kCandMax][64];
    __shared__ float s_lo[kCandMax][64];
    const float4* __restrict__ geom = p.geom;
    const float4* __restrict__ gsph = p.sph;
    const uint32_t count = p.count;
    const uint32_t lane = threadIdx.x;
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t tx0 = blockIdx.x * kCandBX, lb0 = blockIdx.y * kCandBY;
    const uint32_t tx1 = min(tx0 + kCandBX, tiles_x);
    const uint32_t lb1 = min(lb0 + kCandBY, p.local_bands);
    const auto row0 = [&](uint32_t lb) {
        return (float)((p.band_first + lb * p.band_step) * RT_STRIPE_ROWS);
    };
    const bool parent = (occl & 4u) != 0u;
    Beam kb;
    const bool in_blk = footprint_beam(p, (float)(tx0 * 8u), (float)(tx1 * 8u), row0(lb0),
                                    row0(lb1 - 1u) + 8.0f, parent, kb);
    // this lane's tile and its cone
    const uint32_t tx = tx0 + lane % kCandBX, lb = lb0 + lane / kCandBX;
    const bool mine = tx < tx1 && lb < lb1;
    Beam k;
    const bool ok = mine && footprint_beam(p, (float)(tx * 8u), (float)(tx * 8u + 8u), row0(lb),
                                           row0(lb) + 8.0f, parent, k);
    const uint32_t tile = lb * tiles_x + tx;
    const uint32_t K = min(p.cand_k, kCandMax);
    float4* const own = cand + (size_t)tile * kCandStride;
    float4* const rec = own + kCandRecOff;
    float4* const sph = own + kCandSphOff;
    uint32_t n = 0;
    for (uint32_t gbase = 0; gbase < count; gbase += kCandStage) {   // (uniform)
        // the group's scan records, all loads in flight together
        float4 gv[kCandGroup];
#pragma unroll
        for (uint32_t b = 0; b < kCandGroup; ++b) {
            const uint32_t i = gbase + b * 64u + lane;
            gv[b] = geom[i < count ? i : 0u];
        }
        uint32_t m = 0;
#pragma unroll
        for (uint32_t b = 0; b < kCandGroup; ++b) {             // block-cone survivors
            const uint32_t i = gbase + b * 64u + lane;
            const bool keep = i < count && (!in_blk || !beam_misses(kb, gv[b]));
            const unsigned long long mask = rt_ballot(keep);
            if (keep) {
                const uint32_t pos = m + __builtin_amdgcn_mbcnt_hi(
                    (uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                s_rec[pos] = gv[b];
                s_idx[pos] = i;
            }
            m += (uint32_t)__builtin_popcountll(mask);
        }
        __syncthreads();
        for (uint32_t j = lane; j < m; j += 64u) {              // their sphere records
            const uint32_t i = s_idx[j];
            s_sph[2u * j] = gsph[2u * i];
            s_sph[2u * j + 1u] = gsph[2u * i + 1u];
        }
        __syncthreads();
        for (uint32_t j = 0; j < m; ++j) {                      // this lane's tile test
            const float4 gj = s_rec[j];
            if (ok && !beam_misses(k, gj)) {
                if (n < K) {
                    rec[n] = gj;
                    s_own[n][lane] = gj;
                    sph[2u * n] = s_sph[2u * j];
                    sph[2u * n + 1u] = s_sph[2u * j + 1u];
                }
                ++n;
            }
        }
        __syncthreads();                                        // (the next group restages)
    }
    if (!mine) return;
    uint32_t removed = 0;
    // certain tiles: whether the one entry left certainly shows every ray its front face — the
    // occluder's, from the bounds the cull computes anyway
    bool front_one = false;
    if ((occl & 1u) && ok && n <= K && n >= 2u) {
        const Lens lens = bundle_lens(p, k, parent);
        // the occluder: the smallest upper bound among the entries every ray certainly hits
        float t_occ = __builtin_inff();
        uint32_t j_occ = kCandNone;
        for (uint32_t j = 0; j < n; ++j) {
            const float4 gj = s_own[j][lane];
            const OccBounds b = occ_bounds(k, lens, gj);
            s_lo[j][lane] = b.lo;
            if (b.covers && b.hi < t_occ) {
                t_occ = b.hi;
                j_occ = j;
                front_one = certainly_front(b, gj);
            }
        }
        if (j_occ != kCandNone) {
            uint32_t m = 0;
            for (uint32_t j = 0; j < n; ++j) {
                if (j != j_occ && s_lo[j][lane] > t_occ) continue;   // hidden
                if (m != j) {
                    rec[m] = s_own[j][lane];
                    sph[2u * m] = sph[2u * j];
                    sph[2u * m + 1u] = sph[2u * j + 1u];
                }
                ++m;
            }
            removed = n - m;
            n = m;   // (the occluder is never dropped: a list of one is the occluder)
        }
    } else if ((occl & 3u) == 3u && ok && n == 1u && n <= K) {
        // a list of one from the start: nothing to cull, its bounds for the flag alone
        const float4 g = s_own[0][lane];
        front_one = certainly_front(occ_bounds(k, bundle_lens(p, k, parent), g), g);
    }
    // a certain tile (rt_occlusion.h): one entry left, every ray certainly hits it from
    // outside on its front face with the near root accepted; a negative radius flips the
    // normal (wgsl:209 divides by it), so such a tile stays general
    uint32_t flags = 0;
    if ((occl & 2u) && ok && n <= K && n == 1u && front_one) {
        const float radius = sph[0].w, matw = sph[1].w;
        if (radius > 0.0f && __builtin_isfinite(radius))
            flags = kTileCertain | material_class(matw) << 1;
    }
    const uint32_t c = ok && n <= K ? n : kCandNone;
    // zero the chunk padding after the last record
    if (c != kCandNone)
        for (uint32_t q = n; q < ((n + 3u) & ~3u); ++q)
            rec[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    own[0] = make_float4(__uint_as_float(c), __uint_as_float(removed), __uint_as_float(flags),
                         0.0f);
}

__global__ __launch_bounds__(256) void rt_init_kernel(float4* __restrict__ out, uint64_t n) {
    const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = z;
}

// gathered = nranks x max_local_rows x width texels; band b of the full image is local
// band b / nranks of rank b % nranks.
__global__ __launch_bounds__(256) void rt_deinterleave_kernel(const float4* __restrict__ g,
                                                              float4* __restrict__ out,
                                                              uint32_t width, uint32_t height,
                                                              uint32_t nranks,
                                                              uint32_t max_local_rows) {
    const uint64_t total = (uint64_t)width * height;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(i / width);
        const uint32_t x = (uint32_t)(i - (uint64_t)y * width);
        const uint32_t band = y / RT_STRIPE_ROWS;
        const uint32_t rank = band % nranks;
        const uint32_t lrow = (band / nranks) * RT_STRIPE_ROWS + (y % RT_STRIPE_ROWS);
        out[i] = g[((uint64_t)rank * max_local_rows + lrow) * width + x];
    }
}

// Band-set partitions (rt_deinterleave_bands): band_src[b] = the gathered row holding band
// b's first row (rank * rows_per_rank + local band * 8), built and checked on the host.
__global__ __launch_bounds__(256) void rt_deinterleave_bands_kernel(
    const float4* __restrict__ g, float4* __restrict__ out, uint32_t width, uint32_t height,
    const uint32_t* __restrict__ band_src) {
    const uint64_t texels = (uint64_t)width * height;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < texels;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t y = (uint32_t)(i / width), x = (uint32_t)(i % width);
        const uint32_t row = band_src[y / RT_STRIPE_ROWS] + y % RT_STRIPE_ROWS;
        out[i] = g[(uint64_t)row * width + x];
    }
}

// rt_present_rgba8: one texel per lane per step, 16 B in / 4 B out.  The sRGB boundary
// table (1 KB) is staged in LDS; each channel is a branch-free 8-step binary search.
template <bool kSrgb>
__global__ __launch_bounds__(256) void rt_present_kernel(const float4* __restrict__ in,
                                                         uchar4* __restrict__ out,
                                                         uint64_t texels,
                                                         const float* __restrict__ srgb_t) {
    __shared__ float T[256];
    if (kSrgb) {
        T[threadIdx.x] = srgb_t[threadIdx.x];
        __syncthreads();
    }
    auto enc = [&](float c) -> uint32_t {
        if (kSrgb) {
            uint32_t k = 0;
#pragma unroll
            for (uint32_t s = 128; s >= 1; s >>= 1)
                k += (c >= T[k + s]) ? s : 0u;   // NaN compares false -> 0
            return k;
        }
        const float v = fminf(fmaxf(c, 0.0f), 1.0f);  // fmaxf(NaN, 0) = 0
        return (uint32_t)(v * 255.0f + 0.5f);
    };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < texels;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const float4 v = in[i];
        out[i] = make_uchar4((uint8_t)enc(v.x), (uint8_t)enc(v.y), (uint8_t)enc(v.z), 255);
    }
}

// Launches through hipModuleLaunchKernel with the arguments packed in the kernel's layout and
// a function handle cached per device and kernel (the launch_single path below): no
// per-launch symbol lookup or per-argument marshalling of the 2.6-KB TraceParams block.
// Slots: 0-4 rt_trace_kernel<k>, 5-8 rt_bounce_kernel<m>, 9-10 rt_tpair_kernel<4 / 2>.
constexpr int kLaunchSlots = 12;
// Launch timing (rt_set_launch_timing): while armed, launch_packed goes through
// hipExtModuleLaunchKernel with the armed events — the start event on the first launch
// after arming, the stop event on every launch — so the dispatch packets themselves carry
// the timestamps (no marker packets on the stream, which cost an idle GPU's short region
// ≈ 2.5 µs).  Per host thread, like the calls that arm it.
static thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
static thread_local uint32_t g_ev_launches = 0;
void arm_launch_events(hipEvent_t start, hipEvent_t stop) {
    g_ev_start = start;
    g_ev_stop = stop;
    g_ev_launches = 0;
}
uint32_t disarm_launch_events() {
    g_ev_start = g_ev_stop = nullptr;
    return g_ev_launches;
}
static hipError_t launch_packed(int slot, const void* sym, dim3 grid, dim3 block, size_t lds,
                                hipStream_t stream, void* args, size_t bytes) {
    constexpr int kMaxDevices = 64;
    static hipFunction_t fn[kMaxDevices][kLaunchSlots] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices || slot < 0 || slot >= kLaunchSlots)
        return hipErrorInvalidValue;
    if (!fn[dev][slot]) {
        e = hipGetFuncBySymbol(&fn[dev][slot], sym);
        if (e != hipSuccess) {
            fn[dev][slot] = nullptr;
            return e;
        }
    }
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes,
                     HIP_LAUNCH_PARAM_END};
    if (g_ev_stop) {
        // (global work sizes in work-items)
        e = hipExtModuleLaunchKernel(fn[dev][slot], grid.x * block.x, grid.y * block.y,
                                     grid.z * block.z, block.x, block.y, block.z, lds, stream,
                                     nullptr, extra, g_ev_start, g_ev_stop, 0);
        if (e == hipSuccess) {
            g_ev_start = nullptr;
            ++g_ev_launches;
        }
        return e;
    }
    return hipModuleLaunchKernel(fn[dev][slot], grid.x, grid.y, grid.z, block.x, block.y,
                                 block.z, (unsigned)lds, stream, nullptr, extra);
}

// rt_trace_kernel's explicit arguments in its layout (the preloaded leading dwords, then
// TraceParams at kParamsOff)
struct TraceArgs {
    const float4* cand;
    const uint32_t* hx;
    const float4* in;
    uint32_t width, height, bands;
    TraceParams p;
};
static_assert(offsetof(TraceArgs, p) == kParamsOff, "rt_trace_kernel's argument layout");

// Chain parts (TraceParams::parts > 1 on a fused launch, rt_set_chain_parts): the launch runs
// sub-list `part` of a unit order dealt into `parts` sub-lists (launch_tile_order's dealt copy
// or launch_raster_order) as a one-row grid — workgroup i takes entry i of the sub-list, the
// kernels' ordered path with the order pointer moved to the sub-list's first entry.  Only the
// instances that read an order (`ordered`), and only with one; false otherwise.
static bool chain_part_grid(const TraceParams& p, bool ordered, dim3& grid, uint32_t& first) {
    first = 0;
    if (p.parts <= 1u) return true;
    if (!ordered || !p.tile_order || p.part >= p.parts) return false;
    uint32_t len = 0;
    part_range(grid.x * grid.y, p.parts, p.part, first, len);
    grid = dim3(len, 1);
    return true;
}

template <int kScan>
static hipError_t launch_trace_as(const TraceParams& p, size_t lds, hipStream_t stream) {
    constexpr uint32_t w = wg_waves<kScan>();
    dim3 grid = tile_grid(p, is_group_kernel(kScan) ? 1u : w);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    uint32_t first = 0;
    if (!chain_part_grid(p, kOrdered<kScan> && is_group_kernel(kScan), grid, first))
        return hipErrorInvalidValue;
    if (grid.x == 0) return hipSuccess;
    TraceArgs args;
    std::memset(&args, 0, offsetof(TraceArgs, p));
    args.cand = p.cand;
    args.hx = p.hx;
    args.in = p.in;
    args.width = p.width;
    args.height = p.height;
    args.bands = pack_bands(p.band_first, p.band_step, p.tile_order != nullptr);
    args.p = p;
    if (args.p.tile_order) args.p.tile_order += first;
    return launch_packed(kScan, reinterpret_cast<const void*>(&rt_trace_kernel<kScan>), grid,
                         dim3(64 * w), lds, stream, &args, sizeof(args));
}

// rt_tpair_kernel<G>: one workgroup of G waves per pair of tiles along a stripe band, grid
// (tile pairs, bands) — or the tile order's units in that shape.
template <int G>
static hipError_t launch_tpair(const TraceParams& p, hipStream_t stream) {
    dim3 grid((((p.width + 7u) >> 3) + 1u) >> 1, p.local_bands);
    if (grid.x == 0 || grid.y == 0 || !p.cand) return grid.x && grid.y ? hipErrorInvalidValue
                                                                      : hipSuccess;
    uint32_t first = 0;
    if (!chain_part_grid(p, true, grid, first)) return hipErrorInvalidValue;
    if (grid.x == 0) return hipSuccess;
    TraceArgs args;
    std::memset(&args, 0, offsetof(TraceArgs, p));
    args.cand = p.cand;
    args.hx = p.hx;
    args.in = p.in;
    args.width = p.width;
    args.height = p.height;
    args.bands = pack_bands(p.band_first, p.band_step, p.tile_order != nullptr);
    args.p = p;
    if (args.p.tile_order) args.p.tile_order += first;
    return launch_packed(G == 4 ? 9 : 10, reinterpret_cast<const void*>(&rt_tpair_kernel<G>),
                         grid, dim3(64 * G), 0, stream, &args, sizeof(args));
}

// TraceParams::hint_rs_dev: row f * depth + i = (rf(sb), random_unit_vector(sb)) with
// sb = hash(hint_n[f] + seed_b[f] + 2 + 1000 i) (wgsl:268, 353) — the values a pixel at the
// hinted count computes itself, by the same device functions.
__global__ __launch_bounds__(256) void rt_hint_rs_kernel(const TraceParams p) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= p.hint_rs_dev_frames * p.depth) return;
    const uint32_t f = t / p.depth, i = t % p.depth;
    const uint32_t sb = hash(p.hint_n[f] + p.seed_b[f] + 2u + i * 1000u);
    const float r_sb = rf(sb);
    const v3 u = random_unit_vector(r_sb, sb);
    p.hint_rs_dev[t] = make_float4(r_sb, u.x, u.y, u.z);
}

// Workgroups of kBounceWaves tiles along a stripe band: grid (column groups, bands).
static hipError_t launch_bounce(const TraceParams& p, hipStream_t stream) {
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    if (p.hint_rs_dev && p.hint_rs_dev_frames) {
        if (p.hint_rs_dev_frames > kHintFrames || p.depth > kHintRsDepth)
            return hipErrorInvalidValue;
        const uint32_t n = p.hint_rs_dev_frames * p.depth;
        rt_hint_rs_kernel<<<dim3((n + 255u) / 256u), dim3(256), 0, stream>>>(p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t w = p.compact == 1u ? kBounceWaves : 1u;   // tiles per workgroup
    dim3 grid((tiles_x + w - 1u) / w, p.local_bands);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    const size_t lds = (size_t)p.lds_records * sizeof(float4);
    TraceParams args = p;
    const void* sym = reinterpret_cast<const void*>(&rt_bounce_kernel<kBounceWave>);
    uint32_t threads = 64;
    if (p.compact == 3u) {                                    // (tile, chunk) units
        grid = dim3(p.unit_order ? tiles_x * p.local_bands * p.split
                                 : tiles_x * p.local_bands + p.split_tiles * (p.split - 1u), 1);
        sym = reinterpret_cast<const void*>(&rt_bounce_kernel<kBounceSplit>);
    } else if (p.compact == 1u) {
        sym = reinterpret_cast<const void*>(&rt_bounce_kernel<kBounceCompact>);
        threads = 64 * kBounceWaves;
    } else if (p.compact == 2u) {
        sym = reinterpret_cast<const void*>(&rt_bounce_kernel<kBouncePair>);
        threads = 128;
    }
    return launch_packed(5 + (int)p.compact, sym, grid, dim3(threads), lds, stream, &args,
                         sizeof(args));
}

// The explicit arguments of rt_single_kernel / rt_chain_kernel, in the kernels' layout.
struct SingleArgs {
    const float4* cand;
    const uint32_t* hx;
    const float4* in;
    uint32_t width, height, bands;
    const uint32_t* order;
    SingleParams q;
};
static_assert(offsetof(SingleArgs, q) == 48, "rt_single_kernel's argument layout");

// One part of a one-frame launch (kSingleWg waves of kPix tiles each per workgroup along a
// stripe band): its arguments and grid; false when the part has no workgroup.
template <int kPix>
static bool single_args(const TraceParams& p, SingleArgs& args, dim3& grid) {
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const uint32_t per = kSingleWg * kPix;
    const uint32_t cols = (tiles_x + per - 1u) / per;
    const uint32_t parts = p.parts > 1u ? p.parts : 1u, part = parts > 1u ? p.part : 0u;
    // this part's workgroups: its sub-list of the order, or every parts-th local band
    grid = dim3(cols, p.local_bands);
    const uint32_t* order = p.wg_order;
    uint32_t lbands = 1u << 16;
    if (parts > 1u) {
        if (order) {
            uint32_t first = 0, len = 0;
            part_range(cols * p.local_bands, parts, part, first, len);
            grid = dim3(len, 1);
            order += first;
        } else {
            grid.y = p.local_bands > part ? (p.local_bands - part + parts - 1u) / parts : 0u;
            lbands = part | (parts << 16);
        }
    }
    if (grid.x == 0 || grid.y == 0) return false;
    SingleParams& q = args.q;
    std::memset(&args, 0, sizeof(args));
    args.cand = p.cand;
    args.hx = p.hx;
    args.in = p.in;
    args.width = p.width;
    args.height = p.height;
    args.bands = pack_bands(p.band_first, p.band_step, false);
    args.order = order;
    q.lbands = lbands;
    q.out = p.out;
    q.geom = p.geom;
    q.sph = p.sph;
    q.count = p.count;
    q.depth = p.depth;
    q.spp = p.spp;
    q.hinted = p.hint_frames != 0u;
    q.n_hint = p.hint_n[0];
    q.seed_b = p.seed_b[0];
    q.hy_off = (uint32_t)(p.hy - p.hx);
    q.rcp_hint = p.hint_rcp[0];
    q.normal_rn = p.normal_rn;
    q.rs = p.hint_rs[0];
    for (int i = 0; i < 3; ++i) {
        q.center[i] = p.center[i];
        q.vul[i] = p.vul[i];
        q.pdu[i] = p.pdu[i];
        q.pdv[i] = p.pdv[i];
        q.ddu[i] = p.ddu[i];
        q.ddv[i] = p.ddv[i];
    }
    q.defocus_angle = p.defocus_angle;
    q.grid_x = grid.x;
    return true;
}

template <int kPix>
static hipError_t launch_single(const TraceParams& p, hipStream_t stream) {
    SingleArgs args;
    dim3 grid;
    if (!single_args<kPix>(p, args, grid)) return hipSuccess;
    // hipModuleLaunchKernel with the arguments packed in the kernel's layout and a cached
    // function handle: no per-launch symbol lookup or per-argument marshalling (320-byte
    // arguments: 4.2-4.4 against 5.0-6.0 µs of host time per launch through the
    // hipLaunchKernelGGL path, profiles/r03/r03j_launch_rate.jsonl) — the host's issue rate
    // bounds small rank shares and the concurrent parts
    size_t bytes = sizeof(args);
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes,
                     HIP_LAUNCH_PARAM_END};
    // (function handles are per device: the caller's DeviceGuard has made it current)
    constexpr int kMaxDevices = 64;
    static hipFunction_t fn[kMaxDevices][2] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    const int r = p.reset_first ? 1 : 0;
    if (!fn[dev][r]) {
        e = hipGetFuncBySymbol(&fn[dev][r],
                               r ? reinterpret_cast<const void*>(&rt_single_reset_kernel<kPix>)
                                 : reinterpret_cast<const void*>(&rt_single_kernel<kPix>));
        if (e != hipSuccess) {
            fn[dev][r] = nullptr;
            return e;
        }
    }
    return hipModuleLaunchKernel(fn[dev][r], grid.x, grid.y, 1, 64 * kSingleWg, 1, 1, 0, stream,
                                 nullptr, extra);
}

// ---- Frame chains (rt_chain.cpp) ----------------------------------------------------------
// The code object's chain kernels: [pix == 1 ? 0 : 1][reset], the go and the done kernel.
// hipGetFuncBySymbol makes HIP load the code object on the current device, so that the
// HSA loader lists their symbols (rt_chain.cpp looks them up by these mangled-name parts).
hipError_t chain_load_kernels() {
    const void* k[] = {reinterpret_cast<const void*>(&rt_chain_kernel<1>),
                       reinterpret_cast<const void*>(&rt_chain_reset_kernel<1>),
                       reinterpret_cast<const void*>(&rt_chain_kernel<(int)kSinglePix>),
                       reinterpret_cast<const void*>(&rt_chain_reset_kernel<(int)kSinglePix>),
                       reinterpret_cast<const void*>(&rt_chain_go_kernel),
                       reinterpret_cast<const void*>(&rt_chain_done_kernel)};
    for (const void* f : k) {
        hipFunction_t h = nullptr;
        hipError_t e = hipGetFuncBySymbol(&h, f);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
const char* chain_kernel_symbol(int which) {
    // (Itanium mangling of rtk::rt_chain_kernel<N> etc.: "ILi<N>E" is the template argument)
    static const char* const pix1[2] = {"15rt_chain_kernelILi1EE", "21rt_chain_reset_kernelILi1EE"};
    static const char* const pix2[2] = {"15rt_chain_kernelILi2EE", "21rt_chain_reset_kernelILi2EE"};
    static const char* const pix3[2] = {"15rt_chain_kernelILi3EE", "21rt_chain_reset_kernelILi3EE"};
    static const char* const pix4[2] = {"15rt_chain_kernelILi4EE", "21rt_chain_reset_kernelILi4EE"};
    const char* const* big = kSinglePix == 2 ? pix2 : kSinglePix == 3 ? pix3 : kSinglePix == 4 ? pix4 : pix1;
    switch (which) {
        case kChainPix1: return pix1[0];
        case kChainPix1Reset: return pix1[1];
        case kChainPix: return big[0];
        case kChainPixReset: return big[1];
        case kChainGo: return "18rt_chain_go_kernel";
        default: return "20rt_chain_done_kernel";
    }
}
// The kernel arguments of one part of a one-frame launch of `kernel` (kTraceSingle /
// kTraceSingleOne) for an AQL packet: the explicit arguments, then the hidden ones of code
// object v5 at the next 8-byte boundary (block counts, group sizes, grid dimensions; the
// chain kernels read none of them — the workgroups per row come in SingleParams::grid_x).
// Returns the bytes written (0: the part has no workgroup), the grid in workgroups and the
// chain kernel (kChain*).
uint32_t chain_args(const TraceParams& p, int kernel, const uint32_t* abort, unsigned char* out,
                    uint32_t cap, uint32_t grid[2], uint32_t* group_threads, int* which) {
    SingleArgs args;
    dim3 g;
    const bool one = kernel == kTraceSingleOne;
    const bool any = one ? single_args<1>(p, args, g) : single_args<(int)kSinglePix>(p, args, g);
    if (!any) return 0;
    args.q.abort = abort;
    const uint32_t hb = (uint32_t)((sizeof(args) + 7u) & ~(size_t)7u);
    const uint32_t total = hb + kHiddenArgsBytes;
    if (total > cap) return 0;
    std::memset(out, 0, total);
    std::memcpy(out, &args, sizeof(args));
    const uint32_t bc[3] = {g.x, g.y, 1u};
    const uint16_t gs[3] = {(uint16_t)(64u * kSingleWg), 1u, 1u};
    const uint16_t dims = 2;
    std::memcpy(out + hb, bc, sizeof(bc));                 // hidden_block_count_x/y/z
    std::memcpy(out + hb + 12, gs, sizeof(gs));            // hidden_group_size_x/y/z
    std::memcpy(out + hb + 64, &dims, sizeof(dims));       // hidden_grid_dims
    grid[0] = g.x;
    grid[1] = g.y;
    *group_threads = 64u * kSingleWg;
    *which = (one ? kChainPix1 : kChainPix) + (p.reset_first ? 1 : 0);
    return total;
}

hipError_t launch_trace(const TraceParams& p, int kernel, hipStream_t stream) {
    if (kernel == kTraceSingle) return launch_single<(int)kSinglePix>(p, stream);
    if (kernel == kTraceSingleOne) return launch_single<1>(p, stream);
    if (kernel == kTraceCulled)
        return launch_trace_as<kTraceCulled>(p, (size_t)p.lds_records * sizeof(float4), stream);
    if (kernel == kTraceList) return launch_trace_as<kTraceList>(p, 0, stream);
    if (kernel == kTraceListPair)
        return launch_trace_as<kTraceListPair>(p, group_lds_bytes<kTraceListPair>(), stream);
    if (kernel == kTraceBounce) return launch_bounce(p, stream);
    if (kernel == kTraceListQuad)
        return launch_trace_as<kTraceListQuad>(p, group_lds_bytes<kTraceListQuad>(), stream);
    if (kernel == kTraceListQuad2) return launch_tpair<4>(p, stream);
    if (kernel == kTraceListPair2) return launch_tpair<2>(p, stream);
    return launch_trace_as<kTraceExhaustive>(p, 0, stream);
}

hipError_t launch_candidates(const TraceParams& p, float4* cand, bool occlusion, bool certain,
                             bool tight, hipStream_t stream) {
    const uint32_t tiles_x = (p.width + 7u) >> 3;
    const dim3 grid((tiles_x + kCandBX - 1u) / kCandBX,
                    (p.local_bands + kCandBY - 1u) / kCandBY);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_candidates_kernel, grid, dim3(64), 0, stream, p, cand,
                       (occlusion ? (certain ? 3u : 1u) : 0u) | (tight ? 0u : 4u));
    return hipGetLastError();
}

uint32_t single_wg_tiles(uint32_t pix) { return kSingleWg * pix; }
uint32_t single_pix() { return kSinglePix; }

hipError_t launch_wg_order(const float4* cand, uint32_t tiles_x, uint32_t bands, uint32_t pix,
                           uint32_t* wg_cost, uint32_t* wg_order, hipStream_t stream,
                           uint32_t parts) {
    const uint32_t per = kSingleWg * pix;
    const uint32_t cols = (tiles_x + per - 1u) / per;
    const uint32_t units = cols * bands;
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_wg_cost_kernel, dim3((units + 255u) / 256u), dim3(256), 0, stream, cand,
                       tiles_x, cols, per, units, wg_cost);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_tile_order(wg_cost, wg_order, units, cols, stream, parts);
}

hipError_t launch_init(float4* out, uint64_t texels, hipStream_t stream) {
    if (texels == 0) return hipSuccess;
    uint64_t blocks = (texels + 255u) / 256u;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(rt_init_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, out,
                       texels);
    return hipGetLastError();
}

hipError_t launch_deinterleave(const float4* gathered, float4* out, uint32_t width,
                               uint32_t height, uint32_t nranks, uint32_t max_local_rows,
                               hipStream_t stream) {
    const uint64_t texels = (uint64_t)width * height;
    if (texels == 0) return hipSuccess;
    uint64_t blocks = (texels + 255u) / 256u;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(rt_deinterleave_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream,
                       gathered, out, width, height, nranks, max_local_rows);
    return hipGetLastError();
}

hipError_t launch_deinterleave_bands(const float4* gathered, float4* out, uint32_t width,
                                     uint32_t height, const uint32_t* band_src,
                                     hipStream_t stream) {
    const uint64_t texels = (uint64_t)width * height;
    if (texels == 0) return hipSuccess;
    uint64_t blocks = (texels + 255u) / 256u;
    if (blocks > 8192u) blocks = 8192u;
    hipLaunchKernelGGL(rt_deinterleave_bands_kernel, dim3((uint32_t)blocks), dim3(256), 0,
                       stream, gathered, out, width, height, band_src);
    return hipGetLastError();
}

hipError_t launch_present(const float4* in, uchar4* out, uint64_t texels,
                          const float* srgb_t, hipStream_t stream) {
    if (texels == 0) return hipSuccess;
    uint64_t blocks = (texels + 255u) / 256u;
    if (blocks > 16384u) blocks = 16384u;
    if (srgb_t)
        hipLaunchKernelGGL(rt_present_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0,
                           stream, in, out, texels, srgb_t);
    else
        hipLaunchKernelGGL(rt_present_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0,
                           stream, in, out, texels, srgb_t);
    return hipGetLastError();
}

const char* trace_kernel_name() { return "rt_trace_kernel"; }
const char* single_kernel_name(uint32_t pix) {
    static const char* const names[] = {"rt_single_kernel<1>", "rt_single_kernel<2>",
                                        "rt_single_kernel<3>", "rt_single_kernel<4>"};
    return names[(pix ? pix : kSinglePix) - 1];
}

}  // namespace rtk


#if RT_SSTAMPS
// Diagnostic builds: copies the one-frame kernel's per-wave stamps (12 words each, see
// RT_SSTAMPS) of the first n waves of the last launch to out[12 n] and clears them.
extern "C" __attribute__((visibility("default"))) int rt_diag_single_stamps(
    unsigned long long* out, unsigned n) {
    if (n > rtk::kSStampWaves) n = rtk::kSStampWaves;
    static unsigned long long t[rtk::kSStampWaves][12];
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(t, HIP_SYMBOL(rtk::g_sst), sizeof(t)) != hipSuccess) return 1;
    std::memcpy(out, t, (size_t)n * 12 * sizeof(unsigned long long));
    std::memset(t, 0, sizeof(t));
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_sst), t, sizeof(t)) != hipSuccess) return 1;
    return 0;
}
#endif

#if RT_BOUNCE_COUNTS
// Diagnostic builds: copies the bounce counters (n <= 32) to out and clears them.
extern "C" __attribute__((visibility("default"))) int rt_diag_bounce_counts(unsigned long long* out,
                                                                            unsigned n) {
    if (n > 32) n = 32;
    static unsigned long long c[32];
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(c, HIP_SYMBOL(rtk::g_bcount), sizeof(c)) != hipSuccess) return 1;
    for (unsigned i = 0; i < n; ++i) out[i] = c[i];
    static const unsigned long long zero[32] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_bcount), zero, sizeof(zero)) == hipSuccess ? 0 : 1;
}
#endif
#if RT_WAVE_TRACE
// Diagnostic builds: copies (start, end, hw_id, xcc_id) of the first n waves of the last
// traced launch to out[4 n] and clears them.
extern "C" __attribute__((visibility("default"))) int rt_diag_wave_trace(unsigned long long* out,
                                                                         unsigned n) {
    if (n > rtk::kTraceWaves) n = rtk::kTraceWaves;
    static unsigned long long t[rtk::kTraceWaves][2];
    static unsigned id[rtk::kTraceWaves][2];
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(t, HIP_SYMBOL(rtk::g_wave_t), sizeof(t)) != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(id, HIP_SYMBOL(rtk::g_wave_id), sizeof(id)) != hipSuccess) return 1;
    for (unsigned i = 0; i < n; ++i) {
        out[4 * i] = t[i][0];
        out[4 * i + 1] = t[i][1];
        out[4 * i + 2] = id[i][0];
        out[4 * i + 3] = id[i][1];
    }
    std::memset(t, 0, sizeof(t));
    if (hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_wave_t), t, sizeof(t)) != hipSuccess) return 1;
    return 0;
}
#endif
