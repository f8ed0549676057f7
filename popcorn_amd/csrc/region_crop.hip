// region_crop.hip -- the normalised, patched crop: the model input of ONE rectangular crop of the resident rasters, repaired from a planned
// patch table and normalised in ONE launch, with or without the crop's admin mask.  Two entry points are two calls of it:
//
//   pc_region_item     resident validation (data/region.py: ResidentItems): out (6, hc, wc) and admin_out (hc, wc) = (float)boundary of the
//                      crop {x0, x1, y0, y1, season}; no cap on a side (a long thin census unit gives a wide crop)
//   pc_region_window   resident evaluation (data/region.py: ResidentWindows): out (6, ps, ps) of the sliding window (x, y, season) -- a
//                      square item without an admin plane whose ranges start on row boundaries
//
//   out[c] = (v - mean[c]) / std[c], channels [S2 R G B NIR | S1 VV VH], v = the patch value where the slice [start, start + count) of the
//   table (region_repair.hip's) holds an entry for the site, the raster's value otherwise
//
// The reference pays a gather or a clone, a NaN fill pair, a host synchronisation for the 5 % orbit rule, a concatenation and a
// normalisation pass per item and per window, every time (cli.py: normalize_sample(..., nan_fill=True); eval.py: raw_window_input).  The
// repaired values depend only on (crop, season, orbit), so orbit and repaired sites are planned once and a crop then costs this launch.
//
// The partition.  A workgroup owns the CONTIGUOUS RANGE [o0, o0 + n), o0 = blockIdx.x * range, n = min(range, hc * wc - o0), of one
// plane's hc * wc index space = [c * hc * wc + o0, ... + n) of the table's index space.  A range need not begin or end on a row boundary:
// every group of V elements finds its row by one division by wc / V.  blockIdx.y = 0 .. 5 are the channels; 6, in a launch that has it,
// is the admin plane (no table, no LDS, no barrier).  `range` is a kernel argument: an item passes PC_REGION_ITEM_TILE = 4,096; a window
// passes R * ps, R = pc_region_window_rows(ps) whole rows (at most 16 rows and at most 4,096 elements; one row of up to
// PC_REGION_WINDOW_MAX_PS = 8,192 elements at the widest), so its ranges are blocks of R rows.  LDS is dynamic: 16 bytes for the range's
// two ends, then the tile of `range` floats on a 16-byte boundary (16 KB; 32 KB for a single row above 4,096).
//
// Store-once.  The patch value replaces the raw value BEFORE the normalisation and every output element is stored to global memory
// exactly once, by the thread that owns it: no ordering between the stores of different waves is relied upon.  The first two lanes of
// wave 0 find the range's two ends in the ascending slice by binary search (64-bit keys) and hand them to the workgroup through LDS.  A
// workgroup whose range holds no entry -- every workgroup of a crop without NaN -- normalises and stores straight from registers.
// Otherwise it stages its range of RAW values in LDS, lays the entries over it after a barrier (an entry's place is checked against the
// range whatever the table holds), and after a second barrier every thread normalises and stores the groups it staged.
//
// Loads are region_load.h's (crop origins are arbitrary: 16-byte access at 4-byte alignment, 8-byte for uint16, which converts exactly);
// a thread moves V = 4 consecutive pixels of a row, or V = 1 when wc % 4 != 0 or an output is not 16-byte aligned.  With wc % 4 == 0 a
// range starts at a multiple of 4 (range % 4 == 0), so a group of 4 never leaves its row.  The division is the fp32 division of
// pc_select_normalize (train_ops.hip), the same expression on the same operands.
// No loop's trip count depends on another lane's, wave's or workgroup's progress; both barriers sit in code the whole workgroup takes.
//
// pc_region_window_layer / pc_region_item_layer: the same launch with a building layer, a resident fp32 (h, w) raster without a season
// axis, copied over the crop to layer_out (hc, wc) bit for bit (no normalisation, no table: a NaN keeps its payload).  It is one more
// blockIdx.y plane after the channels and the admin plane, a plain copy like the admin plane.  Here the layer is a POINTER TEST, not a
// template parameter: a launch without one simply has no such plane in its grid, so the code every other workgroup runs is what it was.
// pc_region_window / pc_region_item are the calls without a layer.
#include "common.h"
#include "region_args.h"
#include "region_load.h"

namespace {

constexpr int RC_THREADS = 256;
constexpr int RC_HEAD = 16;                // bytes of LDS in front of the tile: the range's two ends, the tile stays 16-byte aligned
constexpr int RW_MAX_ROWS = 16;            // rows of a window's range, at most
constexpr int RW_TILE = 4096;              // elements of a window's range of more than one row, at most (16 KB)
static_assert(PC_REGION_ITEM_TILE % 4 == 0, "a range starts at a multiple of the vector width");
static_assert(PC_REGION_WINDOW_MAX_PS * 4 <= 32 * 1024, "one row of the widest window is a tile of at most 32 KB");
static_assert(6 * (int64_t)PC_REGION_WINDOW_MAX_PS * PC_REGION_WINDOW_MAX_PS < ((int64_t)1 << 31), "idx is int32 in the window's own space");

struct RegionCropArgs {
    const void* src[6];                     // channel c's source plane at the crop's origin (c < 4: S2 in its own type, else fp32 S1)
    const int32_t* boundary;                // the boundary raster at the crop's origin (a launch with the admin plane)
    int w, plane, range;                    // source row stride; hc * wc; elements of a workgroup's range
    pc_fastdiv div;                         // groups per row: wc / V
    float mean[6], stdv[6];
    const int32_t* idx; const float* val;   // the crop's slice of the patch table (already offset by start)
    int count;
    float* out; float* admin;
    const float* layer; float* layer_out;   // the building layer at the crop's origin and its output (a launch with the layer plane)
};

__device__ __forceinline__ float rc_norm(float v, float mean, float stdv) { return (v - mean) / stdv; }

// the first entry of the ascending slice idx[0, n) that is >= key
__device__ __forceinline__ int rc_lower_bound(const int32_t* idx, int n, int64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// range [o0, o0 + n) of channel c's plane; o0 and n are multiples of V
template <typename T, int V>
__device__ __forceinline__ void rc_channel(const RegionCropArgs& a, int c, int o0, int n, int* ends, float* tile) {
    const int t = threadIdx.x;
    const T* src = pc_pin_ptr(reinterpret_cast<const T*>(a.src[c]));
    int w = a.w;
    pc_fastdiv div = a.div;
    float mean = a.mean[c], stdv = a.stdv[c];
    pc_pin(w); pc_pin(div); pc_pin(mean); pc_pin(stdv);
    const int first = c * a.plane + o0;                                 // (< 6 * hc * wc < 2^31: host)
    const int groups = n / V, g0 = o0 / V;
    float* out = pc_pin_ptr(a.out + first);
    int e0 = 0, e1 = 0;
    if (a.count > 0) {                                                   // (a kernel argument: uniform)
        if (t < 2) ends[t] = rc_lower_bound(a.idx, a.count, (int64_t)first + (int64_t)t * n);
        __syncthreads();
        e0 = __builtin_amdgcn_readfirstlane(ends[0]); e1 = __builtin_amdgcn_readfirstlane(ends[1]);      // (one value per workgroup)
    }
    if (e0 >= e1) {
        // no entry in this workgroup's range: registers -> global
        for (int g = t; g < groups; g += RC_THREADS) {
            const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
            const T* p = src + (int64_t)r * w + j;
            if constexpr (V == 4) {
                const f32x4 v = rg_ld4(p);
                pc_st4(out + g * 4, f32x4{rc_norm(v[0], mean, stdv), rc_norm(v[1], mean, stdv), rc_norm(v[2], mean, stdv),
                                          rc_norm(v[3], mean, stdv)});
            } else {
                out[g] = rc_norm(rg_val(p), mean, stdv);
            }
        }
        return;
    }
    // raw values -> LDS
    for (int g = t; g < groups; g += RC_THREADS) {
        const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
        const T* p = src + (int64_t)r * w + j;
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(tile + g * 4) = rg_ld4(p);
        else tile[g] = rg_val(p);
    }
    __syncthreads();
    // the entries of the range over it: raw, un-normalised repaired values
    for (int e = e0 + t; e < e1; e += RC_THREADS) {
        const int64_t p = (int64_t)a.idx[e] - first;
        if (p >= 0 && p < n) tile[p] = a.val[e];                         // inside the range whatever the table holds
    }
    __syncthreads();
    for (int g = t; g < groups; g += RC_THREADS) {
        const int o = g * V;
        if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + o);
            pc_st4(out + o, f32x4{rc_norm(v[0], mean, stdv), rc_norm(v[1], mean, stdv), rc_norm(v[2], mean, stdv), rc_norm(v[3], mean, stdv)});
        } else {
            out[o] = rc_norm(tile[o], mean, stdv);
        }
    }
}

// the admin plane: (float)boundary over the same range
template <int V>
__device__ __forceinline__ void rc_admin(const RegionCropArgs& a, int o0, int n) {
    const int t = threadIdx.x;
    const int32_t* src = pc_pin_ptr(a.boundary);
    int w = a.w;
    pc_fastdiv div = a.div;
    pc_pin(w); pc_pin(div);
    const int groups = n / V, g0 = o0 / V;
    float* out = pc_pin_ptr(a.admin + o0);
    for (int g = t; g < groups; g += RC_THREADS) {
        const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
        const int32_t* p = src + (int64_t)r * w + j;
        if constexpr (V == 4) {
            const i32x4u q = *reinterpret_cast<const i32x4u*>(p);
            pc_st4(out + g * 4, f32x4{(float)q[0], (float)q[1], (float)q[2], (float)q[3]});
        } else {
            out[g] = (float)*p;
        }
    }
}

// the layer plane: the building layer over the same range, bit for bit
template <int V>
__device__ __forceinline__ void rc_layer(const RegionCropArgs& a, int o0, int n) {
    const int t = threadIdx.x;
    const float* src = pc_pin_ptr(a.layer);
    int w = a.w;
    pc_fastdiv div = a.div;
    pc_pin(w); pc_pin(div);
    const int groups = n / V, g0 = o0 / V;
    float* out = pc_pin_ptr(a.layer_out + o0);
    for (int g = t; g < groups; g += RC_THREADS) {
        const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
        const float* p = src + (int64_t)r * w + j;
        if constexpr (V == 4) pc_st4(out + g * 4, rg_ld4(p));
        else out[g] = *p;
    }
}

// V = 4: wc % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V>
__global__ __launch_bounds__(RC_THREADS) void region_crop_kernel(const RegionCropArgs a) {
    // all LDS in the dynamic region, the tile at a multiple of 16 bytes: a static variable in front of it would shift its base off the
    // alignment of the 16-byte LDS accesses
    extern __shared__ __attribute__((aligned(16))) unsigned char rc_lds[];      // [RC_HEAD bytes: the range's two ends][range floats: the tile]
    int* ends = reinterpret_cast<int*>(rc_lds);
    float* tile = reinterpret_cast<float*>(rc_lds + RC_HEAD);
    const int c = blockIdx.y;
    const int o0 = blockIdx.x * a.range;                                 // (o0 < plane: the grid)
    const int n = min(a.range, a.plane - o0);
    // blockIdx.y: the whole workgroup takes one branch
    if (c >= 6) {
        // the planes after the channels: the admin plane where the launch has one, then the layer plane (kernel arguments: uniform)
        if (c == 6 && a.admin) rc_admin<V>(a, o0, n);
        else rc_layer<V>(a, o0, n);
    } else if constexpr (sizeof(T2) == 4) {
        rc_channel<float, V>(a, c, o0, n, ends, tile);
    } else {
        if (c < 4) rc_channel<T2, V>(a, c, o0, n, ends, tile);
        else rc_channel<float, V>(a, c, o0, n, ends, tile);
    }
}

// What both entry points share, for the crop of hc x wc at (x0, y0) of `season` that the caller found inside the raster with
// 6 * hc * wc < 2^31: the remaining checks, the six channel pointers, the fastdiv, the vector / scalar choice and the type dispatch.
// boundary / admin_out NULL: a launch without the admin plane.  layer / layer_out NULL: a launch without the layer plane.
int rc_launch(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary, const float* layer,
              int S, int C2, int C1, int h, int w, const int32_t* band_sel, int x0, int y0, int hc, int wc, int season, int range, const float* mean6,
              const float* std6, const int32_t* idx, const float* val, int64_t cap, int64_t start, int64_t count, float* out,
              float* admin_out, float* layer_out, void* stream) {
    RegionSources r{};
    bool bl;
    if (rg_layer(layer, layer_out, bl)) return PC_EINVAL;
    if (rg_sources(r, s2, s2_u16, s1, s1_asc, boundary, admin_out != nullptr, S, C2, C1, h, w, band_sel)) return PC_EINVAL;
    if (!mean6 || !std6 || !out || season < 0 || season >= S) return PC_EINVAL;
    if (orbit < 0 || orbit > 1 || (orbit == 1 && !s1_asc)) return PC_EINVAL;
    const int64_t plane = (int64_t)hc * wc;
    if (count < 0 || start < 0 || cap < 0 || count > 6 * plane) return PC_EINVAL;
    if (count > 0 && (!idx || !val || start > cap || count > cap - start)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(admin_out) | reinterpret_cast<uintptr_t>(idx) |
         reinterpret_cast<uintptr_t>(val)) & 3)
        return PC_EINVAL;
    const bool vec = (wc & 3) == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(admin_out) |
                                        reinterpret_cast<uintptr_t>(layer_out)) & 15) == 0;
    const int64_t rplane = (int64_t)h * w, origin = (int64_t)x0 * w + y0;
    RegionCropArgs a{};
    for (int c = 0; c < 4; ++c) {
        const int64_t at = ((int64_t)season * C2 + r.band2[c]) * rplane + origin;
        a.src[c] = s2_u16 ? (const void*)(reinterpret_cast<const uint16_t*>(s2) + at) : (const void*)(reinterpret_cast<const float*>(s2) + at);
    }
    for (int c = 0; c < 2; ++c) a.src[4 + c] = (orbit ? s1_asc : s1) + ((int64_t)season * C1 + r.band1[c]) * rplane + origin;
    a.boundary = admin_out ? boundary + origin : nullptr;
    a.w = w; a.plane = (int)plane; a.range = range;
    a.div = pc_make_fastdiv((uint32_t)(vec ? wc / 4 : wc));
    for (int c = 0; c < 6; ++c) { a.mean[c] = mean6[c]; a.stdv[c] = std6[c]; }
    a.idx = count > 0 ? idx + start : nullptr; a.val = count > 0 ? val + start : nullptr; a.count = (int)count;
    a.out = out; a.admin = admin_out;
    a.layer = bl ? layer + origin : nullptr; a.layer_out = layer_out;
    const dim3 grid((unsigned)((plane + range - 1) / range), 6 + (admin_out ? 1 : 0) + (bl ? 1 : 0));
    const size_t lds = RC_HEAD + (size_t)range * sizeof(float);          // the tile: <= 32 KB
    hipStream_t st = (hipStream_t)stream;
    if (s2_u16) {
        if (vec) hipLaunchKernelGGL((region_crop_kernel<uint16_t, 4>), grid, dim3(RC_THREADS), lds, st, a);
        else hipLaunchKernelGGL((region_crop_kernel<uint16_t, 1>), grid, dim3(RC_THREADS), lds, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((region_crop_kernel<float, 4>), grid, dim3(RC_THREADS), lds, st, a);
        else hipLaunchKernelGGL((region_crop_kernel<float, 1>), grid, dim3(RC_THREADS), lds, st, a);
    }
    PC_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int pc_region_window_rows(int ps) {
    if (ps < 1 || ps > PC_REGION_WINDOW_MAX_PS) return 0;
    int R = RW_TILE / ps;
    if (R > RW_MAX_ROWS) R = RW_MAX_ROWS;
    if (R > ps) R = ps;
    return R < 1 ? 1 : R;
}

extern "C" int pc_region_window_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const float* layer, int S,
                                      int C2, int C1, int h, int w, const int32_t* band_sel, int x, int y, int season, int ps,
                                      const float* mean6, const float* std6, const int32_t* idx, const float* val, int64_t cap,
                                      int64_t start, int64_t count, float* out, float* layer_out, void* stream) {
    if (ps < 1 || ps > PC_REGION_WINDOW_MAX_PS) return PC_EINVAL;
    if (x < 0 || y < 0 || ps > h || ps > w || x > h - ps || y > w - ps) return PC_EINVAL;         // the window stays inside the raster
    return rc_launch(s2, s2_u16, s1, s1_asc, orbit, nullptr, layer, S, C2, C1, h, w, band_sel, x, y, ps, ps, season,
                     pc_region_window_rows(ps) * ps, mean6, std6, idx, val, cap, start, count, out, nullptr, layer_out, stream);
}

// the call of the same code without a layer
extern "C" int pc_region_window(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, int S, int C2, int C1, int h,
                                int w, const int32_t* band_sel, int x, int y, int season, int ps, const float* mean6, const float* std6,
                                const int32_t* idx, const float* val, int64_t cap, int64_t start, int64_t count, float* out,
                                void* stream) {
    return pc_region_window_layer(s2, s2_u16, s1, s1_asc, orbit, nullptr, S, C2, C1, h, w, band_sel, x, y, season, ps, mean6, std6, idx, val,
                                  cap, start, count, out, nullptr, stream);
}

extern "C" int pc_region_item_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary,
                                    const float* layer, int S, int C2, int C1, int h, int w, const int32_t* band_sel, int x0, int x1, int y0,
                                    int y1, int season, const float* mean6, const float* std6, const int32_t* idx, const float* val,
                                    int64_t cap, int64_t start, int64_t count, float* out, float* admin_out, float* layer_out,
                                    void* stream) {
    if (!boundary || !admin_out) return PC_EINVAL;
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > h || y1 > w) return PC_EINVAL;          // non-empty, inside the raster
    if (6 * (int64_t)(x1 - x0) * (y1 - y0) >= ((int64_t)1 << 31)) return PC_EINVAL;             // idx is int32 in the item's own space
    return rc_launch(s2, s2_u16, s1, s1_asc, orbit, boundary, layer, S, C2, C1, h, w, band_sel, x0, y0, x1 - x0, y1 - y0, season,
                     PC_REGION_ITEM_TILE, mean6, std6, idx, val, cap, start, count, out, admin_out, layer_out, stream);
}

// the call of the same code without a layer
extern "C" int pc_region_item(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary, int S,
                              int C2, int C1, int h, int w, const int32_t* band_sel, int x0, int x1, int y0, int y1, int season,
                              const float* mean6, const float* std6, const int32_t* idx, const float* val, int64_t cap, int64_t start,
                              int64_t count, float* out, float* admin_out, void* stream) {
    return pc_region_item_layer(s2, s2_u16, s1, s1_asc, orbit, boundary, nullptr, S, C2, C1, h, w, band_sel, x0, x1, y0, y1, season, mean6,
                                std6, idx, val, cap, start, count, out, admin_out, nullptr, stream);
}
