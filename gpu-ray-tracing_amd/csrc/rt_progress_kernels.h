// rt_progress_kernels.h — launch interface of rt_progress_stats' kernels (rt_progress.hip) for
// rt_post.cpp.  Internal; the public boundary is include/rt_progress.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rtk {

// One partial of the report, and the report itself: rt_progress_report's layout (rt_post.cpp
// asserts it) with the maximum error as its order-preserving key until the fold decodes it.
enum { kProgPixels, kProgActive, kProgConverged, kProgCapped, kProgBelowMin, kProgNoHistory,
       kProgNonfinite, kProgSamples, kProgActiveTiles, kProgCounts };
struct ProgressRecord {
    uint64_t count[kProgCounts];
    uint32_t min_count, max_count;
    uint32_t max_error;             // the key in a partial, the float's bits in the report
    uint32_t reserved[3];
};

// Workgroups of the classifying launch at most: four per compute unit of a 256-CU device, so
// the records the fold reads are bounded by the machine and not by the image.
constexpr uint32_t kProgressMaxGroups = 1024;
// The context's device block: the report, then one record per workgroup.
constexpr size_t kProgressBlockBytes = (kProgressMaxGroups + 1u) * sizeof(ProgressRecord);

struct ProgressParams {
    const float4* image;      // the accumulator (local rows of the band set)
    const float4* moments;    // (m1, m2, 0, k), or NULL: `error` is read
    const float* error;
    uint64_t* tile_active;    // optional
    ProgressRecord* block;    // kProgressBlockBytes
    uint32_t width, height;
    uint32_t band_first, band_step, local_bands;
    uint32_t spp;
    uint32_t min_samples;
    float abs_tolerance2, rel_tolerance2;
    float min_history;        // (float)min_history
};

// The classifying launch and the fold, in order on `stream`; block[0] is the report afterwards.
hipError_t launch_progress(const ProgressParams& p, hipStream_t stream);

}  // namespace rtk
