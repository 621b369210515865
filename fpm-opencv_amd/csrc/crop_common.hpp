// crop_common.hpp -- what more than one objCrop kernel family (crop256m.hip,
// crop600.hip, crop360.hip) uses on the device.
#pragma once
#include <hip/hip_runtime.h>

namespace fpm {

typedef float f32x4_nt __attribute__((ext_vector_type(4)));

namespace {

// live-band test: a <= i <= b
__device__ __forceinline__ bool in_band(int i, int a, int b) { return (unsigned)(i - a) <= (unsigned)(b - a); }

}  // namespace

}  // namespace fpm
