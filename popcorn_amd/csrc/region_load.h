// region_load.h -- how the kernels over resident rasters (region.hip, region_batch.hip) read them: crop origins are arbitrary, so a group of
// four pixels of a raster row is one 16-byte access at 4-byte alignment (8 bytes at 2-byte alignment for uint16 digital numbers).  fp32
// payloads pass through registers untouched (a NaN keeps its payload); uint16 converts exactly.
#pragma once
#include "common.h"

typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));                 // 16-byte access at 4-byte alignment
typedef unsigned short u16x4u __attribute__((ext_vector_type(4), aligned(2)));      // 8-byte access at 2-byte alignment

__device__ __forceinline__ float rg_val(const float* p) { return *p; }
__device__ __forceinline__ float rg_val(const uint16_t* p) { return (float)*p; }
__device__ __forceinline__ f32x4 rg_ld4(const float* p) { return *reinterpret_cast<const f32x4u*>(p); }
__device__ __forceinline__ f32x4 rg_ld4(const uint16_t* p) {
    const u16x4u q = *reinterpret_cast<const u16x4u*>(p);
    return f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]};
}
