// region_args.h -- what every entry point over the resident rasters (region.hip, region_batch.hip, region_repair.hip, region_crop.hip)
// checks and computes, once: the sources and the band selection as they travel in the kernel arguments, the validity of a crop, the
// orbit mask of a launch, the building layer of the `_layer` forms (both pointers or neither, aligned for fp32), and the device prologue
// that turns (sources, crop) into the crop's origin, extent and season planes.
// Every failure is PC_EINVAL and nothing is enqueued before the checks are through.
#pragma once
#include "common.h"

struct RegionSources {
    const void* s2; const float* s1; const float* s1_asc; const int32_t* boundary;
    int C2, C1, h, w;
    int band2[4], band1[2];                                     // source band of output channel c
};

// The sources of an entry point: non-NULL (boundary: only where the entry point reads one), aligned for their element type, non-empty,
// h * w < 2^31, every selected band inside its source.
static inline int rg_sources(RegionSources& r, const void* s2, int s2_u16, const float* s1, const float* s1_asc, const int32_t* boundary,
                             bool need_boundary, int S, int C2, int C1, int h, int w, const int32_t* band_sel) {
    if (!s2 || !s1 || !band_sel || (need_boundary && !boundary)) return PC_EINVAL;
    if (S < 1 || C2 < 1 || C1 < 1 || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s1_asc) | reinterpret_cast<uintptr_t>(boundary)) & 3) return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(s2) & (s2_u16 ? 1 : 3)) return PC_EINVAL;
    for (int c = 0; c < 6; ++c)
        if (band_sel[c] < 0 || band_sel[c] >= (c < 4 ? C2 : C1)) return PC_EINVAL;
    r.s2 = s2; r.s1 = s1; r.s1_asc = s1_asc; r.boundary = boundary; r.C2 = C2; r.C1 = C1; r.h = h; r.w = w;
    for (int c = 0; c < 4; ++c) r.band2[c] = band_sel[c];
    for (int c = 0; c < 2; ++c) r.band1[c] = band_sel[4 + c];
    return 0;
}

// The building layer of an entry point that takes one (the `_layer` forms): a resident fp32 (h, w) raster without a season axis and the
// output it is copied to.  Both or neither, and both aligned for fp32.  `given` tells the caller which launch to make.
static inline int rg_layer(const float* layer, const float* layer_out, bool& given) {
    given = layer != nullptr;
    if ((layer != nullptr) != (layer_out != nullptr)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(layer) | reinterpret_cast<uintptr_t>(layer_out)) & 3) return PC_EINVAL;
    return 0;
}

// crop c = {x0, x1, y0, y1, season}: non-empty, inside the h x w raster, inside the Hm x Wm tile, of an existing season
static inline bool rg_crop_ok(const int32_t* c, int h, int w, int S, int Hm, int Wm) {
    if (c[0] < 0 || c[1] <= c[0] || c[1] > h || c[2] < 0 || c[3] <= c[2] || c[3] > w) return false;
    return c[1] - c[0] <= Hm && c[3] - c[2] <= Wm && c[4] >= 0 && c[4] < S;
}

// The orbit mask of a launch of Bc crops: bit b = crop b reads its S1 from s1_asc.  orbit NULL: every crop from s1.  A byte above 1 and
// an ascending crop without the ascending raster are refused.
static inline int rg_orbit_mask(uint32_t (&mask)[PC_REGION_GATHER_MAX_B / 32], const uint8_t* orbit, int Bc, const float* s1_asc) {
    for (int k = 0; k < PC_REGION_GATHER_MAX_B / 32; ++k) mask[k] = 0;
    if (!orbit) return 0;
    for (int b = 0; b < Bc; ++b) {
        if (orbit[b] > 1 || (orbit[b] && !s1_asc)) return PC_EINVAL;
        if (orbit[b]) mask[b >> 5] |= 1u << (b & 31);
    }
    return 0;
}

// The crop prologue of a kernel whose blockIdx.y is the crop: origin and extent (1 <= hb <= Hm, 1 <= wb <= Wm: host), the S2 planes of
// the crop's season and its S1 planes, from the source the orbit bit names.
struct RegionCrop { int x0, y0, hb, wb; };
template <typename T2>
__device__ __forceinline__ RegionCrop rg_crop(const RegionSources& r, const uint32_t* orbit, const int32_t (*crops)[5], int b, const T2*& s2,
                                              const float*& s1) {
    const int32_t* c = crops[b];
    const int64_t plane = (int64_t)r.h * r.w;
    s2 = reinterpret_cast<const T2*>(r.s2) + (int64_t)c[4] * r.C2 * plane;
    s1 = (((orbit[b >> 5] >> (b & 31)) & 1u) ? r.s1_asc : r.s1) + (int64_t)c[4] * r.C1 * plane;
    return RegionCrop{c[0], c[2], c[1] - c[0], c[3] - c[2]};
}
