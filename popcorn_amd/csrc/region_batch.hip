// region_batch.hip -- the batch a fused training step takes, assembled from the resident rasters in ONE launch.
//
// pc_region_gather (region.hip) writes S2, S1 and admin_mask at the batch maximum, pc_augment_raw (train_ops.hip) reads all three again and
// writes the raw [S2 | S1] tile and a second admin_mask, and the feed indexes y / census_idx with several torch ops.  pc_region_batch is the
// composite, by definition and bit for bit:
//
//   raw, admin_out  ==  pc_augment_raw( pc_region_gather(crops; Hm, Wm), coins )
//
// Output pixel (i, j) of crop b is pixel (y, x) of the gathered tile T (Hm x Wm), where (y, x) undoes the rotation and then the flips exactly
// as augment_raw_kernel does; T[y][x] is raster pixel (x0 + y, y0 + x) when y < hb and x < wb and the padding 0 / 0 / -1 otherwise, so the
// padding lands wherever the composite puts it.  The S2 value transform (aug_value.h, shared with pc_augment_raw) is applied to padding as
// well, as the composite applies it.  Every address is formed from a row and a column clamped to the crop; every output element is written.
//
//   even rot   a thread owns four consecutive pixels of an output row through all seven planes: four consecutive pixels of a raster row,
//              ascending or (horizontal mirror) descending -- one 16-byte load at the source's natural alignment (8 bytes for uint16), one
//              aligned 16-byte store, when Wm % 4 == 0 and the outputs are 16-byte aligned; a group that straddles the crop's edge goes
//              element by element, and so does everything else (V = 1)
//   odd rot    32 x 32 output tiles through a [7][32][33] LDS image, as augment_raw_transposed_kernel: reads run along raster rows, writes
//              along output rows, both coalesced
//
// Label assembly rides in the same launch: the first workgroup of crop b copies row items[b] of the device plan tables (plan_cidx int64,
// plan_y fp32, (n, Kp), uploaded once) into census_idx_out / y_out (B, K).  Crops, items, coins and the band selection travel by value in
// the kernel arguments (the idiom of RegionGatherArgs): no device descriptor, no copy, no synchronisation.  The host wrapper validates
// everything before anything is enqueued.
// pc_region_batch_orbit is the same code with the S1 source chosen per crop (s1_asc and a 128-bit mask per launch in the kernel arguments);
// pc_region_batch is its call without either.  The map between output and tile positions is region_index.h's, which the patch launch of
// region_repair.hip uses in the other direction.
// pc_region_batch_layer is the same code again with a building layer (region.hip: pc_region_gather_layer): building_counts (B, 1, Ho, Wo)
// follows the admin mask's map, its padding is 0.0 and it gets no value transform -- by definition and bit for bit the layer of
// pc_augment_raw_layer( pc_region_gather_layer(...) ).  pc_region_batch_orbit is its call without a layer.  The layer is the template
// parameter BL of the one kernel body (why a template parameter and not a pointer test: region.hip's header): the odd-rot LDS image is
// [8][32][33] with a layer and [7][32][33] without.
#include "common.h"
#include "aug_value.h"
#include "region_args.h"
#include "region_index.h"
#include "region_load.h"

namespace {

constexpr int RB_THREADS = 256;
constexpr int RB_MAX_BLOCKS = 2048;      // workgroups of a launch

struct RegionBatchArgs {
    RegionSources src;
    uint32_t orbit[PC_REGION_GATHER_MAX_B / 32];                // bit b: crop b reads its S1 from s1_asc (16 bytes; zero: every crop from s1)
    float* raw; float* adm;                                     // already offset to the launch's first crop
    const float* bld; float* obld;                              // the building layer (h, w) and its output, offset likewise (BL)
    int Hm, Wm, Ho, Wo;                                         // the gathered tile and the output: (Ho, Wo) = (Wm, Hm) for odd rot
    int vflip, hflip, rot;
    int bright, gam;
    float beta, gamma;
    const int64_t* plan_cidx; const float* plan_y;              // (n, Kp); plan_cidx == nullptr: no label assembly
    int64_t* cidx_out; float* y_out;                            // (B, K), already offset to the launch's first crop
    int Kp, K;
    int32_t crop[PC_REGION_GATHER_MAX_B][5];                    // {x0, x1, y0, y1, season}, validated by the host
    int32_t item[PC_REGION_GATHER_MAX_B];                       // plan row of crop b, validated by the host: 3,072 bytes with the crops
};

__device__ __forceinline__ f32x4 rb_rev(f32x4 v) { return f32x4{v[3], v[2], v[1], v[0]}; }

// out[b][k] = plan[item[b]][k], by the first workgroup of crop b
__device__ __forceinline__ void rb_labels(const RegionBatchArgs& a, int b, int t) {
    if (blockIdx.x != 0 || !a.plan_cidx) return;
    const int64_t src = (int64_t)a.item[b] * a.Kp, dst = (int64_t)b * a.K;
    for (int k = t; k < a.K; k += RB_THREADS) {
        a.cidx_out[dst + k] = a.plan_cidx[src + k];
        a.y_out[dst + k] = a.plan_y[src + k];
    }
}

// even rot: the output row i is tile row i or Hm - 1 - i, its columns run along the tile row, ascending or descending.
// V = 4: Wm % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V, bool BL>
__global__ __launch_bounds__(RB_THREADS) void region_batch_kernel(const RegionBatchArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    rb_labels(a, b, t);
    const RegionSources& r = a.src;
    const T2* s2; const float* s1;
    const RegionCrop cr = rg_crop(r, a.orbit, a.crop, b, s2, s1);
    const int x0 = cr.x0, y0 = cr.y0, hb = cr.hb, wb = cr.wb;
    const int64_t plane = (int64_t)r.h * r.w, oplane = (int64_t)a.Hm * a.Wm;
    float* raw = a.raw + (int64_t)b * 6 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
    const float* bld = a.bld;
    float* obld = BL ? a.obld + (int64_t)b * oplane : nullptr;
    // out = rot90^k(hflip(vflip(T))), k in {0, 2}: a half turn mirrors both axes, a flip mirrors one
    const bool yrev = pc_region_yrev(a.vflip, a.rot), xrev = pc_region_xrev(a.hflip, a.rot);
    const bool value = a.bright || a.gam;
    const float pad2 = pc_aug_s2_value(0.f, a.bright, a.beta, a.gam, a.gamma);     // what the composite makes of the S2 padding
    const int wg = a.Wm / V, groups = a.Hm * wg;                   // (Hm * Wm < 2^31: host)
    for (int g = blockIdx.x * RB_THREADS + t; g < groups; g += gridDim.x * RB_THREADS) {
        const int i = g / wg, j = (g - i * wg) * V;
        const int y = yrev ? a.Hm - 1 - i : i;                     // tile row
        const int xl = xrev ? a.Wm - V - j : j;                    // lowest tile column of the group (>= 0: Wm % V == 0)
        const int64_t o = (int64_t)i * a.Wm + j;
        const int64_t src = (int64_t)(x0 + min(y, hb - 1)) * r.w + y0;      // the crop's row (a padding row: its last row, not used)
        if constexpr (V == 4) {
            if (y < hb && xl + 4 <= wb) {
                // four pixels inside the crop
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    f32x4 v = rg_ld4(s2 + r.band2[c] * plane + src + xl);
                    if (xrev) v = rb_rev(v);
                    if (value) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = pc_aug_s2_value(v[e], a.bright, a.beta, a.gam, a.gamma);
                    }
                    pc_st4(raw + c * oplane + o, v);
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    f32x4 v = rg_ld4(s1 + r.band1[c] * plane + src + xl);
                    if (xrev) v = rb_rev(v);
                    pc_st4(raw + (4 + c) * oplane + o, v);
                }
                const i32x4u id = *reinterpret_cast<const i32x4u*>(r.boundary + src + xl);
                f32x4 m = f32x4{(float)id[0], (float)id[1], (float)id[2], (float)id[3]};
                if (xrev) m = rb_rev(m);
                pc_st4(adm + o, m);
                if constexpr (BL) {
                    f32x4 v = rg_ld4(bld + src + xl);
                    if (xrev) v = rb_rev(v);
                    pc_st4(obld + o, v);
                }
                continue;
            }
            if (y >= hb || xl >= wb) {
                // four pixels of padding
#pragma unroll
                for (int c = 0; c < 4; ++c) pc_st4(raw + c * oplane + o, f32x4{pad2, pad2, pad2, pad2});
#pragma unroll
                for (int c = 0; c < 2; ++c) pc_st4(raw + (4 + c) * oplane + o, f32x4{0.f, 0.f, 0.f, 0.f});
                pc_st4(adm + o, f32x4{-1.f, -1.f, -1.f, -1.f});
                if constexpr (BL) pc_st4(obld + o, f32x4{0.f, 0.f, 0.f, 0.f});
                continue;
            }
        }
        // element by element: the group that straddles the crop's right edge, and the whole V = 1 form
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int x = xrev ? xl + V - 1 - e : xl + e;          // tile column of output column j + e
            const bool in = y < hb && x < wb;
            const int64_t s = src + min(x, wb - 1);                // inside the crop whatever `in` says
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float v = rg_val(s2 + r.band2[c] * plane + s);
                raw[c * oplane + o + e] = in ? pc_aug_s2_value(v, a.bright, a.beta, a.gam, a.gamma) : pad2;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float v = s1[r.band1[c] * plane + s];
                raw[(4 + c) * oplane + o + e] = in ? v : 0.f;
            }
            adm[o + e] = in ? (float)r.boundary[s] : -1.f;
            if constexpr (BL) {
                const float v = bld[s];
                obld[o + e] = in ? v : 0.f;
            }
        }
    }
}

// odd rot: a 32 x 32 tile of the output is a 32 x 32 tile of the gathered tile read ACROSS its rows -- staged through LDS so that both the
// reads (along raster rows) and the writes (along output rows) are coalesced
template <typename T2, bool BL>
__global__ __launch_bounds__(RB_THREADS) void region_batch_transposed_kernel(const RegionBatchArgs a) {
    __shared__ float tile[BL ? 8 : 7][32][33];
    const int t = threadIdx.x, b = blockIdx.y;
    rb_labels(a, b, t);
    const RegionSources& r = a.src;
    const T2* s2; const float* s1;
    const RegionCrop cr = rg_crop(r, a.orbit, a.crop, b, s2, s1);
    const int x0 = cr.x0, y0 = cr.y0, hb = cr.hb, wb = cr.wb;
    const int64_t plane = (int64_t)r.h * r.w, oplane = (int64_t)a.Ho * a.Wo;
    float* raw = a.raw + (int64_t)b * 6 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
    const float* bld = a.bld;
    float* obld = BL ? a.obld + (int64_t)b * oplane : nullptr;
    const float pad2 = pc_aug_s2_value(0.f, a.bright, a.beta, a.gam, a.gamma);
    const int tiles_j = (a.Wo + 31) / 32, tiles = ((a.Ho + 31) / 32) * tiles_j;
    const int tx = t & 31, ty0 = t >> 5;                           // 32 x 8 threads, four rows each
    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {       // (the same trip count for every thread of the workgroup)
        const int i0 = (tl / tiles_j) * 32, j0 = (tl % tiles_j) * 32;
        // tile coordinates of output (i, j): rot 1: (y, x) = (j, Wm - 1 - i); rot 3: (Hm - 1 - j, i); then the flips.  Along a tile ROW x
        // follows i: the tile is read with tx -> i (x direction), ty -> j (y direction)
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int dj = ty0 + 8 * q, di = tx;
            const int i = i0 + di, j = j0 + dj;
            if (i < a.Ho && j < a.Wo) {
                int y, x;
                pc_region_out_to_tile(i, j, a.Hm, a.Wm, a.vflip, a.hflip, a.rot, y, x);
                const bool in = y < hb && x < wb;
                const int64_t s = (int64_t)(x0 + min(y, hb - 1)) * r.w + y0 + min(x, wb - 1);      // inside the crop whatever `in` says
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float v = rg_val(s2 + r.band2[c] * plane + s);
                    tile[c][dj][di] = in ? pc_aug_s2_value(v, a.bright, a.beta, a.gam, a.gamma) : pad2;
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float v = s1[r.band1[c] * plane + s];
                    tile[4 + c][dj][di] = in ? v : 0.f;
                }
                tile[6][dj][di] = in ? (float)r.boundary[s] : -1.f;
                if constexpr (BL) {
                    const float v = bld[s];
                    tile[7][dj][di] = in ? v : 0.f;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int di = ty0 + 8 * q, dj = tx;                   // output row i0 + di, column j0 + dj: tx along the output row
            const int i = i0 + di, j = j0 + dj;
            if (i < a.Ho && j < a.Wo) {
                const int64_t o = (int64_t)i * a.Wo + j;
#pragma unroll
                for (int c = 0; c < 6; ++c) raw[c * oplane + o] = tile[c][dj][di];
                adm[o] = tile[6][dj][di];
                if constexpr (BL) obld[o] = tile[7][dj][di];
            }
        }
    }
}

template <typename T2>
inline void rb_launch(const RegionBatchArgs& a, int Bc, bool vec, hipStream_t st) {
    const int cap = RB_MAX_BLOCKS / Bc > 1 ? RB_MAX_BLOCKS / Bc : 1;
    if (a.rot & 1) {
        int gx = ((a.Ho + 31) / 32) * ((a.Wo + 31) / 32);          // (< 2^31 / 1024 + Ho + Wo)
        if (gx > cap) gx = cap;
        if (a.bld) hipLaunchKernelGGL((region_batch_transposed_kernel<T2, true>), dim3(gx, Bc), dim3(RB_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_batch_transposed_kernel<T2, false>), dim3(gx, Bc), dim3(RB_THREADS), 0, st, a);
        return;
    }
    const int64_t groups = (int64_t)a.Hm * (vec ? a.Wm / 4 : a.Wm);
    int64_t gx = (groups + RB_THREADS - 1) / RB_THREADS;
    if (gx > cap) gx = cap;
    const dim3 grid((int)gx, Bc);
    if (a.bld) {
        if (vec) hipLaunchKernelGGL((region_batch_kernel<T2, 4, true>), grid, dim3(RB_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_batch_kernel<T2, 1, true>), grid, dim3(RB_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((region_batch_kernel<T2, 4, false>), grid, dim3(RB_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_batch_kernel<T2, 1, false>), grid, dim3(RB_THREADS), 0, st, a);
    }
}

}  // namespace

extern "C" int pc_region_batch_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit,
                                     const int32_t* boundary, const float* layer, int S, int C2, int C1, int h, int w,
                                     const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, int vflip, int hflip, int rot,
                                     int bright, float beta, int gam, float gamma, float* raw, float* admin_out, float* layer_out, int Ho,
                                     int Wo, const pc_region_labels* labels, void* stream) {
    RegionBatchArgs a{};
    bool bl;
    if (rg_layer(layer, layer_out, bl)) return PC_EINVAL;
    if (rg_sources(a.src, s2, s2_u16, s1, s1_asc, boundary, true, S, C2, C1, h, w, band_sel)) return PC_EINVAL;
    if (!crops || !raw || !admin_out || B < 1 || Hm < 1 || Wm < 1 || rot < 0 || rot > 3) return PC_EINVAL;
    if (Ho != ((rot & 1) ? Wm : Hm) || Wo != ((rot & 1) ? Hm : Wm)) return PC_EINVAL;
    if ((int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(admin_out)) & 3) return PC_EINVAL;
    // every crop valid and every orbit byte good: nothing is enqueued otherwise
    for (int b = 0; b < B; ++b)
        if (!rg_crop_ok(crops + 5 * (int64_t)b, h, w, S, Hm, Wm)) return PC_EINVAL;
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B)
        if (rg_orbit_mask(a.orbit, orbit ? orbit + b0 : nullptr, B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B, s1_asc))
            return PC_EINVAL;
    if (labels) {
        if (!labels->plan_cidx || !labels->plan_y || !labels->items || !labels->census_idx_out || !labels->y_out) return PC_EINVAL;
        if (labels->n < 1 || labels->Kp < 1 || labels->K < 1 || labels->K > labels->Kp) return PC_EINVAL;
        if ((reinterpret_cast<uintptr_t>(labels->plan_cidx) | reinterpret_cast<uintptr_t>(labels->census_idx_out)) & 7) return PC_EINVAL;
        if ((reinterpret_cast<uintptr_t>(labels->plan_y) | reinterpret_cast<uintptr_t>(labels->y_out)) & 3) return PC_EINVAL;
        for (int b = 0; b < B; ++b)
            if (labels->items[b] < 0 || labels->items[b] >= labels->n) return PC_EINVAL;
    }
    const bool vec = (Wm & 3) == 0 && ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(admin_out) |
                                        reinterpret_cast<uintptr_t>(layer_out)) & 15) == 0;
    const int64_t oplane = (int64_t)Hm * Wm;
    a.bld = layer;
    a.Hm = Hm; a.Wm = Wm; a.Ho = Ho; a.Wo = Wo;
    a.vflip = vflip != 0; a.hflip = hflip != 0; a.rot = rot; a.bright = bright != 0; a.gam = gam != 0; a.beta = beta; a.gamma = gamma;
    if (labels) { a.plan_cidx = labels->plan_cidx; a.plan_y = labels->plan_y; a.Kp = labels->Kp; a.K = labels->K; }
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B) {
        const int Bc = B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B;
        a.raw = raw + (int64_t)b0 * 6 * oplane; a.adm = admin_out + (int64_t)b0 * oplane;
        a.obld = bl ? layer_out + (int64_t)b0 * oplane : nullptr;
        for (int b = 0; b < Bc; ++b)
            for (int k = 0; k < 5; ++k) a.crop[b][k] = crops[5 * (int64_t)(b0 + b) + k];
        rg_orbit_mask(a.orbit, orbit ? orbit + b0 : nullptr, Bc, s1_asc);
        if (labels) {
            a.cidx_out = labels->census_idx_out + (int64_t)b0 * labels->K; a.y_out = labels->y_out + (int64_t)b0 * labels->K;
            for (int b = 0; b < Bc; ++b) a.item[b] = labels->items[b0 + b];
        }
        if (s2_u16) rb_launch<uint16_t>(a, Bc, vec, (hipStream_t)stream);
        else rb_launch<float>(a, Bc, vec, (hipStream_t)stream);
        PC_CHECK_LAUNCH();
    }
    return 0;
}

// the call of the same code without a layer
extern "C" int pc_region_batch_orbit(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit,
                                     const int32_t* boundary, int S, int C2, int C1, int h, int w, const int32_t* band_sel,
                                     const int32_t* crops, int B, int Hm, int Wm, int vflip, int hflip, int rot, int bright, float beta,
                                     int gam, float gamma, float* raw, float* admin_out, int Ho, int Wo, const pc_region_labels* labels,
                                     void* stream) {
    return pc_region_batch_layer(s2, s2_u16, s1, s1_asc, orbit, boundary, nullptr, S, C2, C1, h, w, band_sel, crops, B, Hm, Wm, vflip, hflip,
                                 rot, bright, beta, gam, gamma, raw, admin_out, nullptr, Ho, Wo, labels, stream);
}

// the mask-zero call of the same code
extern "C" int pc_region_batch(const void* s2, int s2_u16, const float* s1, const int32_t* boundary, int S, int C2, int C1, int h, int w,
                               const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, int vflip, int hflip, int rot,
                               int bright, float beta, int gam, float gamma, float* raw, float* admin_out, int Ho, int Wo,
                               const pc_region_labels* labels, void* stream) {
    return pc_region_batch_orbit(s2, s2_u16, s1, nullptr, nullptr, boundary, S, C2, C1, h, w, band_sel, crops, B, Hm, Wm, vflip, hflip, rot,
                                 bright, beta, gam, gamma, raw, admin_out, Ho, Wo, labels, stream);
}
