// region_atlas.hip -- several resident regions behind one handle: a batch whose crops come from different regions is still ONE launch.
//
// The reference trains on several countries at once: one Population_Dataset per entry of -tregtrain, concatenated and shuffled with
// weak_batch_size = 2 (run_train.py:423-431), so the two crops of a step usually come from different rasters.  pc_region_gather_layer
// (region.hip) and pc_region_batch_layer (region_batch.hip) take ONE set of raster pointers per launch.  An ATLAS is R resident regions,
// 1 <= R <= PC_ATLAS_MAX_REGIONS, each with its own extent, season count, band counts and band selection:
//
//   pc_atlas_create   validates R descriptors (pc_atlas_region: what rg_sources / rg_layer validate per region; a building layer on all
//                     regions or on none), keeps a host copy and uploads a device copy ONCE -- the only copy and the only synchronisation
//   pc_atlas_gather   crop b is crop crops[b] of region region_of[b].  By definition, bit for bit (fp32 compared as integers, NaN payloads
//                     kept): row b == row 0 of pc_region_gather_layer on region region_of[b] alone with crop b, orbit b and tile (Hm, Wm)
//   pc_atlas_batch    == pc_augment_raw_layer( pc_atlas_gather(...), coins ), plus the label rows of pc_region_batch (items index ONE
//                     concatenated plan table)
//
// With R = 1 both equal the single-region entry points on every output.  The kernels are the bodies of region.hip / region_batch.hip --
// the template idiom <T2, V, BL>, the even-rot vector form and the odd-rot 32 x 32 LDS tiles, the same padding 0 / 0 / -1 / 0.0, the same
// vector-path rule -- with one difference: blockIdx.y is the crop, so its region is wave-uniform, and a workgroup reads its region's
// descriptor from the device table ONCE before its loops, folds season and band into eight plane pointers, and pins them (common.h: pc_pin;
// DESIGN 2 records what hipcc does with arguments that are re-read inside strip loops).  region_of (128 bytes) travels by value next to the
// crops; eight descriptors of 88 bytes would not fit the 4 KB of kernel arguments next to them, hence the device table.
// Every address is formed from a row and a column clamped to the crop inside its OWN region's plane; the host validates every crop against
// its own region's (h, w, S) before anything is enqueued.  The single-region entry points and their kernels are untouched.
#include <new>
#include "common.h"
#include "aug_value.h"
#include "region_args.h"
#include "region_index.h"
#include "region_load.h"

namespace {

constexpr int AT_THREADS = 256;
constexpr int AT_MAX_BLOCKS = 2048;      // workgroups of a launch

struct AtlasHandle {
    int R, s2_u16;
    bool layer;
    pc_atlas_region host[PC_ATLAS_MAX_REGIONS];
    pc_atlas_region* dev;
};

// what both launches carry: the device table, the region and crop of every batch row, the orbit mask
struct AtlasCrops {
    const pc_atlas_region* table;                               // DEVICE [R], uploaded at creation
    uint32_t orbit[PC_REGION_GATHER_MAX_B / 32];                // bit b: crop b reads its S1 from its region's s1_asc
    int32_t crop[PC_REGION_GATHER_MAX_B][5];                    // {x0, x1, y0, y1, season}, validated by the host in its own region
    uint8_t region_of[PC_REGION_GATHER_MAX_B];                  // validated by the host: < R
};

struct AtlasGatherArgs {
    AtlasCrops c;
    float* o2; float* o1; float* adm; int32_t* data_hw;         // already offset to the launch's first crop
    float* obld;                                                // the building layer's output, offset likewise (BL)
    int Hm, Wm;
};

struct AtlasBatchArgs {
    AtlasCrops c;
    float* raw; float* adm;                                     // already offset to the launch's first crop
    float* obld;
    int Hm, Wm, Ho, Wo;                                         // the gathered tile and the output: (Ho, Wo) = (Wm, Hm) for odd rot
    int vflip, hflip, rot;
    int bright, gam;
    float beta, gamma;
    const int64_t* plan_cidx; const float* plan_y;              // (n, Kp); plan_cidx == nullptr: no label assembly
    int64_t* cidx_out; float* y_out;                            // (B, K), already offset to the launch's first crop
    int Kp, K;
    int32_t item[PC_REGION_GATHER_MAX_B];                       // row of the concatenated plan table, validated by the host
};
static_assert(sizeof(AtlasGatherArgs) <= 4096 && sizeof(AtlasBatchArgs) <= 4096, "kernel arguments are limited to 4 KB");

// The crop prologue: the descriptor of the crop's region, read once per workgroup (b = blockIdx.y is uniform) and reduced to what the loops
// use -- the four S2 planes and two S1 planes of the crop's season and bands, the boundary and layer planes, the row stride, the crop's
// origin and extent (1 <= hb <= Hm, 1 <= wb <= Wm: host) -- pinned, so that no loop iteration goes back to the table.
template <typename T2>
struct AtlasCrop {
    const T2* s2[4]; const float* s1[2]; const int32_t* bnd; const float* bld;
    int w, x0, y0, hb, wb;
};
template <typename T2, bool BL>
__device__ __forceinline__ AtlasCrop<T2> at_crop(const AtlasCrops& a, int b) {
    // (through the constant address space: the table is written once, at creation, and a uniform address there is a scalar load)
    typedef __attribute__((address_space(4))) const pc_atlas_region* at_const_ptr;
    const at_const_ptr d = (at_const_ptr) reinterpret_cast<uint64_t>(a.table + a.region_of[b]);
    const int32_t* c = a.crop[b];
    const int64_t plane = (int64_t)d->h * d->w;
    const T2* s2 = reinterpret_cast<const T2*>(d->s2) + (int64_t)c[4] * d->C2 * plane;
    const float* s1 = (((a.orbit[b >> 5] >> (b & 31)) & 1u) ? d->s1_asc : d->s1) + (int64_t)c[4] * d->C1 * plane;
    AtlasCrop<T2> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.s2[k] = pc_pin_ptr(s2 + d->band_sel[k] * plane);
#pragma unroll
    for (int k = 0; k < 2; ++k) r.s1[k] = pc_pin_ptr(s1 + d->band_sel[4 + k] * plane);
    r.bnd = pc_pin_ptr(d->boundary);
    r.bld = BL ? pc_pin_ptr(d->layer) : nullptr;
    r.w = d->w; r.x0 = c[0]; r.y0 = c[2]; r.hb = c[1] - c[0]; r.wb = c[3] - c[2];
    pc_pin(r.w); pc_pin(r.x0); pc_pin(r.y0); pc_pin(r.hb); pc_pin(r.wb);
    return r;
}

// ---- the gather (region.hip: region_gather_kernel) ---------------------------------------------------------------------------------------
// V = 4: Wm % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V, bool BL>
__global__ __launch_bounds__(AT_THREADS) void atlas_gather_kernel(const AtlasGatherArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    const AtlasCrop<T2> r = at_crop<T2, BL>(a.c, b);
    const int x0 = r.x0, y0 = r.y0, hb = r.hb, wb = r.wb;
    if (blockIdx.x == 0 && t == 0) { a.data_hw[2 * b] = hb; a.data_hw[2 * b + 1] = wb; }
    const int64_t oplane = (int64_t)a.Hm * a.Wm;
    float* o2 = a.o2 + (int64_t)b * 4 * oplane;
    float* o1 = a.o1 + (int64_t)b * 2 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
    float* obld = BL ? a.obld + (int64_t)b * oplane : nullptr;
    const int wg = a.Wm / V, groups = a.Hm * wg;                   // (Hm * Wm < 2^31: host)
    for (int g = blockIdx.x * AT_THREADS + t; g < groups; g += gridDim.x * AT_THREADS) {
        const int y = g / wg, x = (g - y * wg) * V;
        const int64_t o = (int64_t)y * a.Wm + x;
        const int64_t src = (int64_t)(x0 + min(y, hb - 1)) * r.w + y0;      // the crop's row (a padding row: its last row, not read)
        if constexpr (V == 4) {
            if (y < hb && x + 4 <= wb) {
                // four pixels inside the crop
#pragma unroll
                for (int c = 0; c < 4; ++c) pc_st4(o2 + c * oplane + o, rg_ld4(r.s2[c] + src + x));
#pragma unroll
                for (int c = 0; c < 2; ++c) pc_st4(o1 + c * oplane + o, rg_ld4(r.s1[c] + src + x));
                const i32x4u id = *reinterpret_cast<const i32x4u*>(r.bnd + src + x);
                pc_st4(adm + o, f32x4{(float)id[0], (float)id[1], (float)id[2], (float)id[3]});
                if constexpr (BL) pc_st4(obld + o, rg_ld4(r.bld + src + x));
                continue;
            }
            if (y >= hb || x >= wb) {
                // four pixels of padding
                const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 4; ++c) pc_st4(o2 + c * oplane + o, zero);
#pragma unroll
                for (int c = 0; c < 2; ++c) pc_st4(o1 + c * oplane + o, zero);
                pc_st4(adm + o, f32x4{-1.f, -1.f, -1.f, -1.f});
                if constexpr (BL) pc_st4(obld + o, zero);
                continue;
            }
        }
        // element by element: the group that straddles the crop's right edge, and the whole V = 1 form
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const bool in = y < hb && x + e < wb;
            const int64_t s = src + min(x + e, wb - 1);            // inside the crop whatever `in` says
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float v = rg_val(r.s2[c] + s);
                o2[c * oplane + o + e] = in ? v : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float v = r.s1[c][s];
                o1[c * oplane + o + e] = in ? v : 0.f;
            }
            adm[o + e] = in ? (float)r.bnd[s] : -1.f;
            if constexpr (BL) {
                const float v = r.bld[s];
                obld[o + e] = in ? v : 0.f;
            }
        }
    }
}

template <typename T2>
inline void ag_launch(const AtlasGatherArgs& a, int Bc, bool vec, bool bl, hipStream_t st) {
    const int64_t groups = (int64_t)a.Hm * (vec ? a.Wm / 4 : a.Wm);
    int64_t gx = (groups + AT_THREADS - 1) / AT_THREADS;
    const int cap = AT_MAX_BLOCKS / Bc > 1 ? AT_MAX_BLOCKS / Bc : 1;
    if (gx > cap) gx = cap;
    const dim3 grid((int)gx, Bc);
    if (bl) {
        if (vec) hipLaunchKernelGGL((atlas_gather_kernel<T2, 4, true>), grid, dim3(AT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((atlas_gather_kernel<T2, 1, true>), grid, dim3(AT_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((atlas_gather_kernel<T2, 4, false>), grid, dim3(AT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((atlas_gather_kernel<T2, 1, false>), grid, dim3(AT_THREADS), 0, st, a);
    }
}

// ---- the one-launch assembly (region_batch.hip) ------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 ab_rev(f32x4 v) { return f32x4{v[3], v[2], v[1], v[0]}; }

// out[b][k] = plan[item[b]][k], by the first workgroup of crop b
__device__ __forceinline__ void ab_labels(const AtlasBatchArgs& a, int b, int t) {
    if (blockIdx.x != 0 || !a.plan_cidx) return;
    const int64_t src = (int64_t)a.item[b] * a.Kp, dst = (int64_t)b * a.K;
    for (int k = t; k < a.K; k += AT_THREADS) {
        a.cidx_out[dst + k] = a.plan_cidx[src + k];
        a.y_out[dst + k] = a.plan_y[src + k];
    }
}

// even rot: the output row i is tile row i or Hm - 1 - i, its columns run along the tile row, ascending or descending.
// V = 4: Wm % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V, bool BL>
__global__ __launch_bounds__(AT_THREADS) void atlas_batch_kernel(const AtlasBatchArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    const AtlasCrop<T2> r = at_crop<T2, BL>(a.c, b);               // (before the first store: the descriptor reads stay scalar loads)
    ab_labels(a, b, t);
    const int x0 = r.x0, y0 = r.y0, hb = r.hb, wb = r.wb;
    const int64_t oplane = (int64_t)a.Hm * a.Wm;
    float* raw = a.raw + (int64_t)b * 6 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
    float* obld = BL ? a.obld + (int64_t)b * oplane : nullptr;
    // out = rot90^k(hflip(vflip(T))), k in {0, 2}: a half turn mirrors both axes, a flip mirrors one
    const bool yrev = pc_region_yrev(a.vflip, a.rot), xrev = pc_region_xrev(a.hflip, a.rot);
    const bool value = a.bright || a.gam;
    const float pad2 = pc_aug_s2_value(0.f, a.bright, a.beta, a.gam, a.gamma);     // what the composite makes of the S2 padding
    const int wg = a.Wm / V, groups = a.Hm * wg;                   // (Hm * Wm < 2^31: host)
    for (int g = blockIdx.x * AT_THREADS + t; g < groups; g += gridDim.x * AT_THREADS) {
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
                    f32x4 v = rg_ld4(r.s2[c] + src + xl);
                    if (xrev) v = ab_rev(v);
                    if (value) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = pc_aug_s2_value(v[e], a.bright, a.beta, a.gam, a.gamma);
                    }
                    pc_st4(raw + c * oplane + o, v);
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    f32x4 v = rg_ld4(r.s1[c] + src + xl);
                    if (xrev) v = ab_rev(v);
                    pc_st4(raw + (4 + c) * oplane + o, v);
                }
                const i32x4u id = *reinterpret_cast<const i32x4u*>(r.bnd + src + xl);
                f32x4 m = f32x4{(float)id[0], (float)id[1], (float)id[2], (float)id[3]};
                if (xrev) m = ab_rev(m);
                pc_st4(adm + o, m);
                if constexpr (BL) {
                    f32x4 v = rg_ld4(r.bld + src + xl);
                    if (xrev) v = ab_rev(v);
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
                const float v = rg_val(r.s2[c] + s);
                raw[c * oplane + o + e] = in ? pc_aug_s2_value(v, a.bright, a.beta, a.gam, a.gamma) : pad2;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float v = r.s1[c][s];
                raw[(4 + c) * oplane + o + e] = in ? v : 0.f;
            }
            adm[o + e] = in ? (float)r.bnd[s] : -1.f;
            if constexpr (BL) {
                const float v = r.bld[s];
                obld[o + e] = in ? v : 0.f;
            }
        }
    }
}

// odd rot: a 32 x 32 tile of the output is a 32 x 32 tile of the gathered tile read ACROSS its rows -- staged through LDS so that both the
// reads (along raster rows) and the writes (along output rows) are coalesced
template <typename T2, bool BL>
__global__ __launch_bounds__(AT_THREADS) void atlas_batch_transposed_kernel(const AtlasBatchArgs a) {
    __shared__ float tile[BL ? 8 : 7][32][33];
    const int t = threadIdx.x, b = blockIdx.y;
    const AtlasCrop<T2> r = at_crop<T2, BL>(a.c, b);               // (before the first store: the descriptor reads stay scalar loads)
    ab_labels(a, b, t);
    const int x0 = r.x0, y0 = r.y0, hb = r.hb, wb = r.wb;
    const int64_t oplane = (int64_t)a.Ho * a.Wo;
    float* raw = a.raw + (int64_t)b * 6 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
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
                    const float v = rg_val(r.s2[c] + s);
                    tile[c][dj][di] = in ? pc_aug_s2_value(v, a.bright, a.beta, a.gam, a.gamma) : pad2;
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float v = r.s1[c][s];
                    tile[4 + c][dj][di] = in ? v : 0.f;
                }
                tile[6][dj][di] = in ? (float)r.bnd[s] : -1.f;
                if constexpr (BL) {
                    const float v = r.bld[s];
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
inline void ab_launch(const AtlasBatchArgs& a, int Bc, bool vec, bool bl, hipStream_t st) {
    const int cap = AT_MAX_BLOCKS / Bc > 1 ? AT_MAX_BLOCKS / Bc : 1;
    if (a.rot & 1) {
        int gx = ((a.Ho + 31) / 32) * ((a.Wo + 31) / 32);          // (< 2^31 / 1024 + Ho + Wo)
        if (gx > cap) gx = cap;
        if (bl) hipLaunchKernelGGL((atlas_batch_transposed_kernel<T2, true>), dim3(gx, Bc), dim3(AT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((atlas_batch_transposed_kernel<T2, false>), dim3(gx, Bc), dim3(AT_THREADS), 0, st, a);
        return;
    }
    const int64_t groups = (int64_t)a.Hm * (vec ? a.Wm / 4 : a.Wm);
    int64_t gx = (groups + AT_THREADS - 1) / AT_THREADS;
    if (gx > cap) gx = cap;
    const dim3 grid((int)gx, Bc);
    if (bl) {
        if (vec) hipLaunchKernelGGL((atlas_batch_kernel<T2, 4, true>), grid, dim3(AT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((atlas_batch_kernel<T2, 1, true>), grid, dim3(AT_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((atlas_batch_kernel<T2, 4, false>), grid, dim3(AT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((atlas_batch_kernel<T2, 1, false>), grid, dim3(AT_THREADS), 0, st, a);
    }
}

// ---- host checks both entry points share ---------------------------------------------------------------------------------------------
// Every crop in its own region, every orbit byte good, layer_out exactly when the atlas has a layer: nothing is enqueued otherwise.
inline int at_check(const AtlasHandle* H, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int B, int Hm, int Wm,
                    const float* layer_out) {
    if (!H || !region_of || !crops || B < 1 || Hm < 1 || Wm < 1) return PC_EINVAL;
    if ((int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PC_EINVAL;
    if (H->layer != (layer_out != nullptr) || (reinterpret_cast<uintptr_t>(layer_out) & 3)) return PC_EINVAL;
    for (int b = 0; b < B; ++b) {
        if (region_of[b] >= H->R) return PC_EINVAL;
        const pc_atlas_region& d = H->host[region_of[b]];
        if (!rg_crop_ok(crops + 5 * (int64_t)b, d.h, d.w, d.S, Hm, Wm)) return PC_EINVAL;
        if (orbit && (orbit[b] > 1 || (orbit[b] && !d.s1_asc))) return PC_EINVAL;
    }
    return 0;
}

// the crops, regions and orbit mask of the launch that starts at crop b0
inline void at_fill(AtlasCrops& c, const AtlasHandle* H, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int b0, int Bc) {
    c.table = H->dev;
    for (int k = 0; k < PC_REGION_GATHER_MAX_B / 32; ++k) c.orbit[k] = 0;
    for (int b = 0; b < Bc; ++b) {
        for (int k = 0; k < 5; ++k) c.crop[b][k] = crops[5 * (int64_t)(b0 + b) + k];
        c.region_of[b] = region_of[b0 + b];
        if (orbit && orbit[b0 + b]) c.orbit[b >> 5] |= 1u << (b & 31);
    }
}

}  // namespace

extern "C" int pc_sizeof_atlas_region(void) { return (int)sizeof(pc_atlas_region); }

extern "C" int pc_atlas_create(const pc_atlas_region* regions, int R, int s2_u16, void** handle) {
    if (!regions || !handle || R < 1 || R > PC_ATLAS_MAX_REGIONS) return PC_EINVAL;
    for (int k = 0; k < R; ++k) {
        const pc_atlas_region& d = regions[k];
        RegionSources tmp;
        if (rg_sources(tmp, d.s2, s2_u16, d.s1, d.s1_asc, d.boundary, true, d.S, d.C2, d.C1, d.h, d.w, d.band_sel)) return PC_EINVAL;
        if (reinterpret_cast<uintptr_t>(d.layer) & 3) return PC_EINVAL;
        if ((d.layer != nullptr) != (regions[0].layer != nullptr)) return PC_EINVAL;      // a layer on all regions or on none
    }
    AtlasHandle* H = new (std::nothrow) AtlasHandle();
    if (!H) return PC_ENOMEM;
    H->R = R; H->s2_u16 = s2_u16 != 0; H->layer = regions[0].layer != nullptr;
    for (int k = 0; k < R; ++k) { H->host[k] = regions[k]; H->host[k]._pad = 0; }
    if (hipMalloc(reinterpret_cast<void**>(&H->dev), sizeof(pc_atlas_region) * R) != hipSuccess) {
        (void)hipGetLastError();
        delete H;
        return PC_ENOMEM;
    }
    // the only copy and the only synchronisation of an atlas
    const hipError_t e = hipMemcpy(H->dev, H->host, sizeof(pc_atlas_region) * R, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(H->dev);
        delete H;
        return (int)e;
    }
    *handle = H;
    return 0;
}

extern "C" void pc_atlas_destroy(void* handle) {
    AtlasHandle* H = static_cast<AtlasHandle*>(handle);
    if (!H) return;
    (void)hipFree(H->dev);
    delete H;
}

extern "C" int pc_atlas_gather(void* handle, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int B, int Hm, int Wm,
                               float* s2_out, float* s1_out, float* admin_out, float* layer_out, int32_t* data_hw, void* stream) {
    const AtlasHandle* H = static_cast<const AtlasHandle*>(handle);
    if (!s2_out || !s1_out || !admin_out || !data_hw) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(s2_out) | reinterpret_cast<uintptr_t>(s1_out) | reinterpret_cast<uintptr_t>(admin_out) |
         reinterpret_cast<uintptr_t>(data_hw)) & 3)
        return PC_EINVAL;
    if (at_check(H, region_of, crops, orbit, B, Hm, Wm, layer_out)) return PC_EINVAL;
    const bool vec = (Wm & 3) == 0 && ((reinterpret_cast<uintptr_t>(s2_out) | reinterpret_cast<uintptr_t>(s1_out) |
                                        reinterpret_cast<uintptr_t>(admin_out) | reinterpret_cast<uintptr_t>(layer_out)) & 15) == 0;
    const int64_t oplane = (int64_t)Hm * Wm;
    AtlasGatherArgs a{};
    a.Hm = Hm; a.Wm = Wm;
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B) {
        const int Bc = B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B;
        a.o2 = s2_out + (int64_t)b0 * 4 * oplane; a.o1 = s1_out + (int64_t)b0 * 2 * oplane; a.adm = admin_out + (int64_t)b0 * oplane;
        a.data_hw = data_hw + 2 * (int64_t)b0;
        a.obld = H->layer ? layer_out + (int64_t)b0 * oplane : nullptr;
        at_fill(a.c, H, region_of, crops, orbit, b0, Bc);
        if (H->s2_u16) ag_launch<uint16_t>(a, Bc, vec, H->layer, (hipStream_t)stream);
        else ag_launch<float>(a, Bc, vec, H->layer, (hipStream_t)stream);
        PC_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int pc_atlas_batch(void* handle, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int B, int Hm, int Wm,
                              int vflip, int hflip, int rot, int bright, float beta, int gam, float gamma, float* raw, float* admin_out,
                              float* layer_out, int Ho, int Wo, const pc_region_labels* labels, void* stream) {
    const AtlasHandle* H = static_cast<const AtlasHandle*>(handle);
    if (!raw || !admin_out || rot < 0 || rot > 3) return PC_EINVAL;
    if (Ho != ((rot & 1) ? Wm : Hm) || Wo != ((rot & 1) ? Hm : Wm)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(admin_out)) & 3) return PC_EINVAL;
    if (at_check(H, region_of, crops, orbit, B, Hm, Wm, layer_out)) return PC_EINVAL;
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
    AtlasBatchArgs a{};
    a.Hm = Hm; a.Wm = Wm; a.Ho = Ho; a.Wo = Wo;
    a.vflip = vflip != 0; a.hflip = hflip != 0; a.rot = rot; a.bright = bright != 0; a.gam = gam != 0; a.beta = beta; a.gamma = gamma;
    if (labels) { a.plan_cidx = labels->plan_cidx; a.plan_y = labels->plan_y; a.Kp = labels->Kp; a.K = labels->K; }
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B) {
        const int Bc = B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B;
        a.raw = raw + (int64_t)b0 * 6 * oplane; a.adm = admin_out + (int64_t)b0 * oplane;
        a.obld = H->layer ? layer_out + (int64_t)b0 * oplane : nullptr;
        at_fill(a.c, H, region_of, crops, orbit, b0, Bc);
        if (labels) {
            a.cidx_out = labels->census_idx_out + (int64_t)b0 * labels->K; a.y_out = labels->y_out + (int64_t)b0 * labels->K;
            for (int b = 0; b < Bc; ++b) a.item[b] = labels->items[b0 + b];
        }
        if (H->s2_u16) ab_launch<uint16_t>(a, Bc, vec, H->layer, (hipStream_t)stream);
        else ab_launch<float>(a, Bc, vec, H->layer, (hipStream_t)stream);
        PC_CHECK_LAUNCH();
    }
    return 0;
}
