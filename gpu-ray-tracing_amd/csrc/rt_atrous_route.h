// rt_atrous_route.h — how one iteration of an a-trous filter reaches its taps: what the launch
// interfaces (rt_denoise_kernels.h, rt_variance_kernels.h), their caller (rt_post.cpp) and the
// device skeleton (rt_atrous.h) share.  Internal.
#pragma once

#include <cstdint>

namespace rtk {

enum AtrousRoute : uint32_t {
    kAtrousRows = 0,    // LDS: 64 x 4 pixels of one (y mod step) class of rows with a halo of
                        // 2 * step along x (step <= kAtrousRowsMaxStep)
    kAtrousDirect = 1,  // no LDS: every tap is a global load, one wave per 64-pixel row piece
};

// kAtrousRows with a step above this is hipErrorInvalidValue.
constexpr uint32_t kAtrousRowsMaxStep = 16;

}  // namespace rtk
