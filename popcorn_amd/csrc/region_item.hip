// region_item.hip -- resident validation: the normalised model input and the admin mask of ONE rectangular crop of the resident rasters,
// repaired from a planned patch table and normalised in ONE launch.
//
// Validating a raw region item by item (cli.py: normalize_sample(..., nan_fill=True) behind a gather) costs a gather, a NaN fill pair,
// a host synchronisation for the 5 % orbit rule, a concatenation and a normalisation pass -- per item, at every validation.  An item's
// orbit and repaired sites depend only on (item, season), so they are planned once (data/region.py: ResidentItems; the table is
// region_repair.hip's) and an item then costs this launch:
//
//   pc_region_item   out (6, hc, wc) = (v - mean[c]) / std[c], channels [S2 R G B NIR | S1 VV VH], v = the patch value where the slice
//                    [start, start + count) of the table holds an entry for the site, the raster's value otherwise;
//                    admin_out (hc, wc) = (float)boundary over the crop
//
// region_window.hip is the model; the extent is rectangular and there is no cap on a side (a long thin census unit gives a wide crop), so
// the work is cut differently.  A workgroup owns a CONTIGUOUS RANGE of PC_REGION_ITEM_TILE = 4,096 elements of one plane's hc * wc index
// space -- range k of channel c is [c * hc * wc + k * TILE, ... + min(TILE, hc * wc - k * TILE)) of the table's index space -- which need
// not begin or end on a row boundary: every element finds its row by one division by wc.  blockIdx.y = 0 .. 5 are the channels, 6 is the
// admin plane (no table, no LDS, no barrier).
//
// Store-once.  The patch value replaces the raw value BEFORE the normalisation and every output element is stored to global memory
// exactly once, by the thread that owns it.  The first two lanes of wave 0 find the range's two ends in the ascending slice by binary
// search and hand them to the workgroup through LDS.  A workgroup whose range holds no entry normalises and stores straight from
// registers.  Otherwise it stages its range of RAW values in LDS (16 KB), lays the entries over it after a barrier (an entry's place is
// checked against the range whatever the table holds), and after a second barrier every thread normalises and stores the groups it
// staged.
//
// Loads are region_load.h's (crop origins are arbitrary); a thread moves V = 4 consecutive pixels of a row, or V = 1 when wc % 4 != 0 or
// an output is not 16-byte aligned.  With wc % 4 == 0 a range starts at a multiple of 4, so a group of 4 never leaves its row.  The
// division is the fp32 division of pc_select_normalize (train_ops.hip), the same expression on the same operands.
// No loop's trip count depends on another lane's, wave's or workgroup's progress; both barriers sit in code the whole workgroup takes.
#include "common.h"
#include "region_load.h"

namespace {

constexpr int RI_THREADS = 256;
constexpr int RI_TILE = PC_REGION_ITEM_TILE;    // elements of a workgroup's range (16 KB of LDS)
constexpr int RI_HEAD = 4;                      // floats of LDS in front of the tile: the range's two ends, the tile stays 16-byte aligned
static_assert(RI_TILE % 4 == 0, "a range starts at a multiple of the vector width");

struct RegionItemArgs {
    const void* src[6];                     // channel c's source plane at the crop's origin (c < 4: S2 in its own type, else fp32 S1)
    const int32_t* boundary;                // the boundary raster at the crop's origin
    int w, wc, plane;                       // source row stride; crop width; hc * wc
    pc_fastdiv div;                         // groups per row: wc / V
    float mean[6], stdv[6];
    const int32_t* idx; const float* val;   // the item's slice of the patch table (already offset by start)
    int count;
    float* out; float* admin;
};

__device__ __forceinline__ float ri_norm(float v, float mean, float stdv) { return (v - mean) / stdv; }

// the first entry of the ascending slice idx[0, n) that is >= key
__device__ __forceinline__ int ri_lower_bound(const int32_t* idx, int n, int64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// range [o0, o0 + n) of channel c's plane; o0 and n are multiples of V
template <typename T, int V>
__device__ __forceinline__ void ri_channel(const RegionItemArgs& a, int c, int o0, int n, float* lds) {
    const int t = threadIdx.x;
    const T* src = pc_pin_ptr(reinterpret_cast<const T*>(a.src[c]));
    int w = a.w;
    pc_fastdiv div = a.div;
    float mean = a.mean[c], stdv = a.stdv[c];
    pc_pin(w); pc_pin(div); pc_pin(mean); pc_pin(stdv);
    const int first = c * a.plane + o0;                                 // (< 6 * hc * wc < 2^31: host)
    const int groups = n / V, g0 = o0 / V;
    float* out = pc_pin_ptr(a.out + first);
    int* ends = reinterpret_cast<int*>(lds);
    float* tile = lds + RI_HEAD;
    int e0 = 0, e1 = 0;
    if (a.count > 0) {                                                   // (a kernel argument: uniform)
        if (t < 2) ends[t] = ri_lower_bound(a.idx, a.count, (int64_t)first + (int64_t)t * n);
        __syncthreads();
        e0 = __builtin_amdgcn_readfirstlane(ends[0]); e1 = __builtin_amdgcn_readfirstlane(ends[1]);      // (one value per workgroup)
    }
    if (e0 >= e1) {
        // no entry in this workgroup's range: registers -> global
        for (int g = t; g < groups; g += RI_THREADS) {
            const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
            const T* p = src + (int64_t)r * w + j;
            if constexpr (V == 4) {
                const f32x4 v = rg_ld4(p);
                pc_st4(out + g * 4, f32x4{ri_norm(v[0], mean, stdv), ri_norm(v[1], mean, stdv), ri_norm(v[2], mean, stdv),
                                          ri_norm(v[3], mean, stdv)});
            } else {
                out[g] = ri_norm(rg_val(p), mean, stdv);
            }
        }
        return;
    }
    // raw values -> LDS
    for (int g = t; g < groups; g += RI_THREADS) {
        const int r = (int)pc_div((uint32_t)(g0 + g), div), j = (g0 + g - r * (int)div.d) * V;
        const T* p = src + (int64_t)r * w + j;
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(tile + g * 4) = rg_ld4(p);
        else tile[g] = rg_val(p);
    }
    __syncthreads();
    // the entries of the range over it: raw, un-normalised repaired values
    for (int e = e0 + t; e < e1; e += RI_THREADS) {
        const int64_t p = (int64_t)a.idx[e] - first;
        if (p >= 0 && p < n) tile[p] = a.val[e];                         // inside the range whatever the table holds
    }
    __syncthreads();
    for (int g = t; g < groups; g += RI_THREADS) {
        const int o = g * V;
        if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + o);
            pc_st4(out + o, f32x4{ri_norm(v[0], mean, stdv), ri_norm(v[1], mean, stdv), ri_norm(v[2], mean, stdv), ri_norm(v[3], mean, stdv)});
        } else {
            out[o] = ri_norm(tile[o], mean, stdv);
        }
    }
}

// the admin plane: (float)boundary over the same range
template <int V>
__device__ __forceinline__ void ri_admin(const RegionItemArgs& a, int o0, int n) {
    const int t = threadIdx.x;
    const int32_t* src = pc_pin_ptr(a.boundary);
    int w = a.w;
    pc_fastdiv div = a.div;
    pc_pin(w); pc_pin(div);
    const int groups = n / V, g0 = o0 / V;
    float* out = pc_pin_ptr(a.admin + o0);
    for (int g = t; g < groups; g += RI_THREADS) {
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

// V = 4: wc % 4 == 0 and 16-byte aligned outputs; V = 1: anything
template <typename T2, int V>
__global__ __launch_bounds__(RI_THREADS) void region_item_kernel(const RegionItemArgs a) {
    __shared__ __attribute__((aligned(16))) float ri_lds[RI_HEAD + RI_TILE];      // [the range's two ends | the tile]
    const int c = blockIdx.y;
    const int o0 = blockIdx.x * RI_TILE;                                 // (o0 < plane: the grid)
    const int n = min(RI_TILE, a.plane - o0);
    // blockIdx.y: the whole workgroup takes one branch
    if (c == 6) {
        ri_admin<V>(a, o0, n);
    } else if constexpr (sizeof(T2) == 4) {
        ri_channel<float, V>(a, c, o0, n, ri_lds);
    } else {
        if (c < 4) ri_channel<T2, V>(a, c, o0, n, ri_lds);
        else ri_channel<float, V>(a, c, o0, n, ri_lds);
    }
}

}  // namespace

extern "C" int pc_region_item(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary, int S,
                              int C2, int C1, int h, int w, const int32_t* band_sel, int x0, int x1, int y0, int y1, int season,
                              const float* mean6, const float* std6, const int32_t* idx, const float* val, int64_t cap, int64_t start,
                              int64_t count, float* out, float* admin_out, void* stream) {
    if (!s2 || !s1 || !boundary || !band_sel || !mean6 || !std6 || !out || !admin_out) return PC_EINVAL;
    if (S < 1 || C2 < 1 || C1 < 1 || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return PC_EINVAL;
    if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > h || y1 > w) return PC_EINVAL;          // non-empty, inside the raster
    const int hc = x1 - x0, wc = y1 - y0;
    const int64_t plane = (int64_t)hc * wc;
    if (6 * plane >= ((int64_t)1 << 31)) return PC_EINVAL;               // idx is int32 in the item's own space
    if (season < 0 || season >= S) return PC_EINVAL;
    if (orbit < 0 || orbit > 1 || (orbit == 1 && !s1_asc)) return PC_EINVAL;
    for (int c = 0; c < 6; ++c)
        if (band_sel[c] < 0 || band_sel[c] >= (c < 4 ? C2 : C1)) return PC_EINVAL;
    if (count < 0 || start < 0 || cap < 0 || count > 6 * plane) return PC_EINVAL;
    if (count > 0 && (!idx || !val || start > cap || count > cap - start)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s1_asc) | reinterpret_cast<uintptr_t>(boundary) |
         reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(admin_out) | reinterpret_cast<uintptr_t>(idx) |
         reinterpret_cast<uintptr_t>(val)) & 3)
        return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(s2) & (s2_u16 ? 1 : 3)) return PC_EINVAL;
    const bool vec = (wc & 3) == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(admin_out)) & 15) == 0;
    const int64_t rplane = (int64_t)h * w, origin = (int64_t)x0 * w + y0;
    const float* s1_src = orbit ? s1_asc : s1;
    RegionItemArgs a{};
    for (int c = 0; c < 4; ++c) {
        const int64_t at = ((int64_t)season * C2 + band_sel[c]) * rplane + origin;
        a.src[c] = s2_u16 ? (const void*)(reinterpret_cast<const uint16_t*>(s2) + at) : (const void*)(reinterpret_cast<const float*>(s2) + at);
    }
    for (int c = 4; c < 6; ++c) a.src[c] = s1_src + ((int64_t)season * C1 + band_sel[c]) * rplane + origin;
    a.boundary = boundary + origin;
    a.w = w; a.wc = wc; a.plane = (int)plane;
    a.div = pc_make_fastdiv((uint32_t)(vec ? wc / 4 : wc));
    for (int c = 0; c < 6; ++c) { a.mean[c] = mean6[c]; a.stdv[c] = std6[c]; }
    a.idx = count > 0 ? idx + start : nullptr; a.val = count > 0 ? val + start : nullptr; a.count = (int)count;
    a.out = out; a.admin = admin_out;
    const dim3 grid((unsigned)((plane + RI_TILE - 1) / RI_TILE), 7);
    hipStream_t st = (hipStream_t)stream;
    if (s2_u16) {
        if (vec) hipLaunchKernelGGL((region_item_kernel<uint16_t, 4>), grid, dim3(RI_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_item_kernel<uint16_t, 1>), grid, dim3(RI_THREADS), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((region_item_kernel<float, 4>), grid, dim3(RI_THREADS), 0, st, a);
        else hipLaunchKernelGGL((region_item_kernel<float, 1>), grid, dim3(RI_THREADS), 0, st, a);
    }
    PC_CHECK_LAUNCH();
    return 0;
}
