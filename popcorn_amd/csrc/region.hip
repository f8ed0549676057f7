// region.hip -- region-resident training data: the census bookkeeping of a boundary raster and the crops of a batch, on the device.
//
// The reference trains from a region: Population_Dataset(mode="weaksup") cuts the bounding box of one census unit, grown by 32 px, out of
// the country's rasters per item (data/PopulationDataset.py:403-458, :624-649) and its collate pads the items of a batch to the largest
// (:885-958); the bounding boxes and pixel counts come from one Python pass PER UNIT over the boundary raster at preprocessing time
// (utils/02_preprocess_rwa_shapefile.py:142-161).  Here the rasters stay in HBM and both are single passes:
//
//   pc_region_units   table[id] = {xmin, xmax, ymin, ymax, count} of every unit id in [0, num_ids) from ONE pass over the boundary raster, in
//                     the reference's convention: x indexes ROWS, y indexes COLUMNS, the maxima are exclusive, a unit without pixels gets
//                     five zeros.  Ids outside [0, num_ids) contribute nothing and are counted in *stray
//   pc_region_gather  the batch of B crops {x0, x1, y0, y1, season}: 4 selected S2 bands (fp32 or uint16 source), 2 selected S1 bands and the
//                     boundary window as (float)id, written at the batch maximum (Hm, Wm) with the collate's padding 0 / 0 / -1 at the
//                     bottom and right, plus each crop's extent -- ONE launch, every element of every output written
//
// The table.  Integer min / max / add are associative and commutative, so the table holds the same bits for any launch geometry and arrival
// order although atomics are used.  Three stages keep them on chip: a lane owns V adjacent columns of a tile of RU_ROWS rows and carries the
// running {id, rows, columns, count} of the run it is in (units are runs down a column and along a row), handing it on when the id changes;
// hand-ons go to bins in LDS.  A bin is claimed for an id by ONE compare-and-swap on slot id % RU_BINS (no probing, no retry): the ids a
// workgroup meets get bins as far as they fit, an id whose slot another id holds adds to the global table directly.  When the workgroup is
// done it issues one global atomicMin / atomicMax / atomicAdd per (unit, workgroup) it holds a bin for.  An init launch (identities of min /
// max) and a finish launch (exclusive maxima, empty units -> zeros) surround the pass.
// No loop's trip count depends on another lane's, wave's or workgroup's progress; every bound is a function of the launch geometry.
//
// The gather.  A thread moves V = 4 consecutive pixels of one output row through all 7 planes: destination rows are 16-byte aligned when
// Wm % 4 == 0 (aligned vector stores); crop origins are arbitrary, so source rows are not (16-byte loads at 4-byte alignment, 8-byte loads at
// 2-byte alignment for uint16).  A group that straddles the crop's edge and everything else (Wm % 4 != 0, unaligned outputs) goes element by
// element.  fp32 payloads pass through registers untouched: a NaN keeps its payload.  The crop list travels in the kernel arguments (up to
// PC_REGION_GATHER_MAX_B crops per launch; longer batches are split): no host-to-device copy, no synchronisation.  The host wrapper
// validates every crop before anything is enqueued; the kernel never forms an address outside the sources.
// pc_region_gather_orbit is the same kernel with the S1 source chosen per crop: a second raster (the ascending orbit) and a 128-bit mask per
// launch in the kernel arguments; pc_region_gather is its call without either (region_repair.hip plans the mask once per region).
// pc_region_gather_layer is the same kernel again with a building layer: a resident fp32 (h, w) raster without a season axis, copied as an
// eighth plane building_counts (B, 1, Hm, Wm) under the admin mask's map, padded with the collate's 0.0 and otherwise bit for bit (no value
// transform, no repair: a NaN keeps its payload).  pc_region_gather_orbit is its call without a layer.  The layer is a TEMPLATE PARAMETER
// (BL) of the one kernel body, not a pointer test, here and in region_batch.hip / train_ops.hip: the transposed forms of those files size
// their static LDS image by it (8 planes against 7), so the instantiation without a layer is the code it was, and one rule serves all
// three files.
#include "common.h"
#include "region_args.h"
#include "region_load.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RU_ROWS = 32;              // rows of a tile
constexpr int RU_R = 8;                  // rows per group of loads in flight
constexpr int RU_BINS = 1024;            // LDS bins of a workgroup (6 x 4 KB); a power of two
constexpr int RU_MAX_BLOCKS = 1024;      // workgroups of the pass: four per CU
constexpr int RG_MAX_BLOCKS = 2048;      // workgroups of a gather launch
constexpr int RU_NONE = 0x7fffffff;      // identity of min
static_assert((RU_BINS & (RU_BINS - 1)) == 0, "the slot of an id is id & (RU_BINS - 1)");
static_assert(RU_ROWS % RU_R == 0, "a tile is whole groups of rows");

typedef unsigned long long rg_u64;

// ---- the unit table --------------------------------------------------------------------------------------------------------------------
struct RegionUnitsArgs {
    const int32_t* boundary; int h, w, num_ids;
    int ntx, ntiles;                // tiles per tile row; tiles in all
    int32_t* table;                 // [num_ids][5] = {row min, row max, column min, column max, count}, inclusive maxima until the finish
    rg_u64* stray;
};

__global__ __launch_bounds__(256) void region_units_init_kernel(int32_t* table, int num_ids, rg_u64* stray) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < num_ids; i += gridDim.x * 256) {
        int32_t* row = table + 5 * (int64_t)i;
        row[0] = RU_NONE; row[1] = -1; row[2] = RU_NONE; row[3] = -1; row[4] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *stray = 0;
}

// V = 4: w % 4 == 0 and a 16-byte aligned raster, one 16-byte load per lane and row; V = 1: any raster, one column per lane
template <int V>
__global__ __launch_bounds__(RG_THREADS) void region_units_kernel(const RegionUnitsArgs a) {
    __shared__ int owner[RU_BINS];
    __shared__ int bin[5][RU_BINS];
    __shared__ unsigned stray_sh[RG_THREADS / 64];
    const int t = threadIdx.x;
    for (int i = t; i < RU_BINS; i += RG_THREADS) {
        owner[i] = -1;
        bin[0][i] = RU_NONE; bin[1][i] = -1; bin[2][i] = RU_NONE; bin[3][i] = -1; bin[4][i] = 0;
    }
    __syncthreads();
    // the run this lane is in
    int cur = -1, rmin = 0, rmax = 0, cmin = 0, cmax = 0, cnt = 0;
    unsigned stray = 0;                                            // (a lane sees fewer than 2^31 pixels: h * w < 2^31)
    auto hand_on = [&]() {
        if (cur < 0) return;
        const int s = cur & (RU_BINS - 1);
        const int prev = atomicCAS(&owner[s], -1, cur);            // one attempt: the slot is ours, already ours, or somebody else's
        if (prev == -1 || prev == cur) {
            atomicMin(&bin[0][s], rmin); atomicMax(&bin[1][s], rmax);
            atomicMin(&bin[2][s], cmin); atomicMax(&bin[3][s], cmax);
            atomicAdd(&bin[4][s], cnt);
        } else {
            int32_t* row = a.table + 5 * (int64_t)cur;
            atomicMin(row + 0, rmin); atomicMax(row + 1, rmax);
            atomicMin(row + 2, cmin); atomicMax(row + 3, cmax);
            atomicAdd(row + 4, cnt);
        }
    };
    auto pixel = [&](int id, int y, int x) {
        if ((unsigned)id >= (unsigned)a.num_ids) { ++stray; id = -1; }
        if (id != cur) {
            hand_on();
            cur = id; rmin = rmax = y; cmin = cmax = x; cnt = 1;
        } else if (id >= 0) {
            rmin = min(rmin, y); rmax = max(rmax, y); cmin = min(cmin, x); cmax = max(cmax, x); ++cnt;
        }
    };
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
        const int ya = ty * RU_ROWS, yb = min(ya + RU_ROWS, a.h);
        const int x0 = tx * (RG_THREADS * V) + V * t;
        if (x0 >= a.w) continue;                                   // a lane without a column (no barrier inside this loop)
        const int32_t* col = a.boundary + x0;
        for (int y = ya; y < yb; y += RU_R) {
            // RU_R rows in flight (a row past the tile is loaded from the tile's last row and not used)
            int ids[RU_R][V];
#pragma unroll
            for (int r = 0; r < RU_R; ++r) {
                const int32_t* p = col + (int64_t)min(y + r, yb - 1) * a.w;
                if constexpr (V == 4) {
                    const int4 q = *reinterpret_cast<const int4*>(p);
                    ids[r][0] = q.x; ids[r][1] = q.y; ids[r][2] = q.z; ids[r][3] = q.w;
                } else ids[r][0] = *p;
            }
#pragma unroll
            for (int r = 0; r < RU_R; ++r) {
                if (y + r >= yb) break;
#pragma unroll
                for (int e = 0; e < V; ++e) pixel(ids[r][e], y + r, x0 + e);
            }
        }
    }
    hand_on();
    for (int off = 32; off > 0; off >>= 1) stray += __shfl_down(stray, off);
    if ((t & 63) == 0) stray_sh[t >> 6] = stray;
    __syncthreads();
    // one global min / max / add per unit this workgroup holds a bin for
    for (int s = t; s < RU_BINS; s += RG_THREADS) {
        const int id = owner[s];
        if (id >= 0) {
            int32_t* row = a.table + 5 * (int64_t)id;
            atomicMin(row + 0, bin[0][s]); atomicMax(row + 1, bin[1][s]);
            atomicMin(row + 2, bin[2][s]); atomicMax(row + 3, bin[3][s]);
            atomicAdd(row + 4, bin[4][s]);
        }
    }
    if (t == 0) {
        rg_u64 n = 0;
#pragma unroll
        for (int wv = 0; wv < RG_THREADS / 64; ++wv) n += stray_sh[wv];
        if (n) atomicAdd(a.stray, n);
    }
}

// exclusive maxima; a unit without pixels gets five zeros (02_preprocess_rwa_shapefile.py:150-157)
__global__ __launch_bounds__(256) void region_units_finish_kernel(int32_t* table, int num_ids) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < num_ids; i += gridDim.x * 256) {
        int32_t* row = table + 5 * (int64_t)i;
        if (row[4] == 0) { row[0] = 0; row[1] = 0; row[2] = 0; row[3] = 0; }
        else { row[1] += 1; row[3] += 1; }
    }
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------------
struct RegionGatherArgs {
    RegionSources src;
    uint32_t orbit[PC_REGION_GATHER_MAX_B / 32];                // bit b: crop b reads its S1 from s1_asc (16 bytes; zero: every crop from s1)
    float* o2; float* o1; float* adm; int32_t* data_hw;          // already offset to the launch's first crop
    const float* bld; float* obld;                               // the building layer (h, w) and its output, offset likewise (BL)
    int Hm, Wm;
    int32_t crop[PC_REGION_GATHER_MAX_B][5];                     // {x0, x1, y0, y1, season}, validated by the host: 2,560 bytes of arguments
};

// V = 4: Wm % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V, bool BL>
__global__ __launch_bounds__(RG_THREADS) void region_gather_kernel(const RegionGatherArgs a) {
    const int t = threadIdx.x, b = blockIdx.y;
    const RegionSources& r = a.src;
    const T2* s2; const float* s1;
    const RegionCrop cr = rg_crop(r, a.orbit, a.crop, b, s2, s1);
    const int x0 = cr.x0, y0 = cr.y0, hb = cr.hb, wb = cr.wb;
    if (blockIdx.x == 0 && t == 0) { a.data_hw[2 * b] = hb; a.data_hw[2 * b + 1] = wb; }
    const int64_t plane = (int64_t)r.h * r.w, oplane = (int64_t)a.Hm * a.Wm;
    float* o2 = a.o2 + (int64_t)b * 4 * oplane;
    float* o1 = a.o1 + (int64_t)b * 2 * oplane;
    float* adm = a.adm + (int64_t)b * oplane;
    const float* bld = a.bld;
    float* obld = BL ? a.obld + (int64_t)b * oplane : nullptr;
    const int wg = a.Wm / V, groups = a.Hm * wg;                   // (Hm * Wm < 2^31: host)
    for (int g = blockIdx.x * RG_THREADS + t; g < groups; g += gridDim.x * RG_THREADS) {
        const int y = g / wg, x = (g - y * wg) * V;
        const int64_t o = (int64_t)y * a.Wm + x;
        const int64_t src = (int64_t)(x0 + min(y, hb - 1)) * r.w + y0;      // the crop's row (a padding row: its last row, not read)
        if constexpr (V == 4) {
            if (y < hb && x + 4 <= wb) {
                // four pixels inside the crop
#pragma unroll
                for (int c = 0; c < 4; ++c) pc_st4(o2 + c * oplane + o, rg_ld4(s2 + r.band2[c] * plane + src + x));
#pragma unroll
                for (int c = 0; c < 2; ++c) pc_st4(o1 + c * oplane + o, rg_ld4(s1 + r.band1[c] * plane + src + x));
                const i32x4u id = *reinterpret_cast<const i32x4u*>(r.boundary + src + x);
                pc_st4(adm + o, f32x4{(float)id[0], (float)id[1], (float)id[2], (float)id[3]});
                if constexpr (BL) pc_st4(obld + o, rg_ld4(bld + src + x));
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
                const float v = rg_val(s2 + r.band2[c] * plane + s);
                o2[c * oplane + o + e] = in ? v : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float v = s1[r.band1[c] * plane + s];
                o1[c * oplane + o + e] = in ? v : 0.f;
            }
            adm[o + e] = in ? (float)r.boundary[s] : -1.f;
            if constexpr (BL) {
                const float v = bld[s];
                obld[o + e] = in ? v : 0.f;
            }
        }
    }
}

template <typename T2>
inline void rg_launch(const RegionGatherArgs& a, int Bc, bool vec, hipStream_t st) {
    const int64_t groups = (int64_t)a.Hm * (vec ? a.Wm / 4 : a.Wm);
    int64_t gx = (groups + RG_THREADS - 1) / RG_THREADS;
    const int cap = RG_MAX_BLOCKS / Bc > 1 ? RG_MAX_BLOCKS / Bc : 1;
    if (gx > cap) gx = cap;
    const dim3 grid((int)gx, Bc);
    if (a.bld) {
        if (vec) hipLaunchKernelGGL((region_gather_kernel<T2, 4, true>), grid, dim3(RG_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_gather_kernel<T2, 1, true>), grid, dim3(RG_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((region_gather_kernel<T2, 4, false>), grid, dim3(RG_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_gather_kernel<T2, 1, false>), grid, dim3(RG_THREADS), 0, st, a);
    }
}

}  // namespace

extern "C" int pc_region_units(const int32_t* boundary, int h, int w, int num_ids, int32_t* table, int64_t* stray, int max_blocks,
                               void* stream) {
    if (!boundary || !table || !stray || h < 1 || w < 1 || num_ids < 1) return PC_EINVAL;
    if ((int64_t)h * w >= ((int64_t)1 << 31) || (int64_t)num_ids * 5 >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(boundary) | reinterpret_cast<uintptr_t>(table)) & 3 || (reinterpret_cast<uintptr_t>(stray) & 7)) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int gi = (num_ids + 255) / 256 < 256 ? (num_ids + 255) / 256 : 256;
    hipLaunchKernelGGL(region_units_init_kernel, dim3(gi), dim3(256), 0, st, table, num_ids, reinterpret_cast<rg_u64*>(stray));
    PC_CHECK_LAUNCH();
    const bool vec = (w & 3) == 0 && (reinterpret_cast<uintptr_t>(boundary) & 15) == 0;
    RegionUnitsArgs a{};
    a.boundary = boundary; a.h = h; a.w = w; a.num_ids = num_ids; a.table = table; a.stray = reinterpret_cast<rg_u64*>(stray);
    const int tw = RG_THREADS * (vec ? 4 : 1);
    a.ntx = (w + tw - 1) / tw;
    const int64_t ntiles = (int64_t)a.ntx * ((h + RU_ROWS - 1) / RU_ROWS);       // (< 2^31 / 8192 + h + w)
    a.ntiles = (int)ntiles;
    int grid = max_blocks > 0 ? max_blocks : RU_MAX_BLOCKS;                       // max_blocks: a smaller launch, for tests of the geometry
    if (grid > RU_MAX_BLOCKS) grid = RU_MAX_BLOCKS;
    if (grid > a.ntiles) grid = a.ntiles;
    if (vec) hipLaunchKernelGGL(region_units_kernel<4>, dim3(grid), dim3(RG_THREADS), 0, st, a);
    else hipLaunchKernelGGL(region_units_kernel<1>, dim3(grid), dim3(RG_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(region_units_finish_kernel, dim3(gi), dim3(256), 0, st, table, num_ids);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_region_gather_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit,
                                      const int32_t* boundary, const float* layer, int S, int C2, int C1, int h, int w,
                                      const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, float* s2_out, float* s1_out,
                                      float* admin_out, float* layer_out, int32_t* data_hw, void* stream) {
    RegionGatherArgs a{};
    bool bl;
    if (rg_layer(layer, layer_out, bl)) return PC_EINVAL;
    if (rg_sources(a.src, s2, s2_u16, s1, s1_asc, boundary, true, S, C2, C1, h, w, band_sel)) return PC_EINVAL;
    if (!crops || !s2_out || !s1_out || !admin_out || !data_hw || B < 1 || Hm < 1 || Wm < 1) return PC_EINVAL;
    if ((int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(s2_out) | reinterpret_cast<uintptr_t>(s1_out) | reinterpret_cast<uintptr_t>(admin_out) |
         reinterpret_cast<uintptr_t>(data_hw)) & 3)
        return PC_EINVAL;
    // every crop valid and every orbit byte good: nothing is enqueued otherwise
    for (int b = 0; b < B; ++b)
        if (!rg_crop_ok(crops + 5 * (int64_t)b, h, w, S, Hm, Wm)) return PC_EINVAL;
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B)
        if (rg_orbit_mask(a.orbit, orbit ? orbit + b0 : nullptr, B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B, s1_asc))
            return PC_EINVAL;
    const bool vec = (Wm & 3) == 0 && ((reinterpret_cast<uintptr_t>(s2_out) | reinterpret_cast<uintptr_t>(s1_out) |
                                        reinterpret_cast<uintptr_t>(admin_out) | reinterpret_cast<uintptr_t>(layer_out)) & 15) == 0;
    const int64_t oplane = (int64_t)Hm * Wm;
    a.Hm = Hm; a.Wm = Wm; a.bld = layer;
    for (int b0 = 0; b0 < B; b0 += PC_REGION_GATHER_MAX_B) {
        const int Bc = B - b0 < PC_REGION_GATHER_MAX_B ? B - b0 : PC_REGION_GATHER_MAX_B;
        a.o2 = s2_out + (int64_t)b0 * 4 * oplane; a.o1 = s1_out + (int64_t)b0 * 2 * oplane; a.adm = admin_out + (int64_t)b0 * oplane;
        a.data_hw = data_hw + 2 * (int64_t)b0;
        a.obld = bl ? layer_out + (int64_t)b0 * oplane : nullptr;
        for (int b = 0; b < Bc; ++b)
            for (int k = 0; k < 5; ++k) a.crop[b][k] = crops[5 * (int64_t)(b0 + b) + k];
        rg_orbit_mask(a.orbit, orbit ? orbit + b0 : nullptr, Bc, s1_asc);
        if (s2_u16) rg_launch<uint16_t>(a, Bc, vec, (hipStream_t)stream);
        else rg_launch<float>(a, Bc, vec, (hipStream_t)stream);
        PC_CHECK_LAUNCH();
    }
    return 0;
}

// the call of the same code without a layer
extern "C" int pc_region_gather_orbit(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit,
                                      const int32_t* boundary, int S, int C2, int C1, int h, int w, const int32_t* band_sel,
                                      const int32_t* crops, int B, int Hm, int Wm, float* s2_out, float* s1_out, float* admin_out,
                                      int32_t* data_hw, void* stream) {
    return pc_region_gather_layer(s2, s2_u16, s1, s1_asc, orbit, boundary, nullptr, S, C2, C1, h, w, band_sel, crops, B, Hm, Wm, s2_out,
                                  s1_out, admin_out, nullptr, data_hw, stream);
}

// the mask-zero call of the same code
extern "C" int pc_region_gather(const void* s2, int s2_u16, const float* s1, const int32_t* boundary, int S, int C2, int C1, int h, int w,
                                const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, float* s2_out, float* s1_out,
                                float* admin_out, int32_t* data_hw, void* stream) {
    return pc_region_gather_orbit(s2, s2_u16, s1, nullptr, nullptr, boundary, S, C2, C1, h, w, band_sel, crops, B, Hm, Wm, s2_out, s1_out,
                                  admin_out, data_hw, stream);
}
