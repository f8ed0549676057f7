// region_window.hip -- resident evaluation: the normalised model input of ONE sliding window, cut out of the resident rasters, repaired from
// a planned patch table and normalised in ONE launch.
//
// The evaluation of a raw raster (eval.py: raw_window_input) clones a window's bands, concatenates them, runs the nearest-value fill on
// S2 and S1, synchronises for the 5 % orbit rule and normalises in a further pass -- per window, every time.  A window's repaired values
// depend only on (window, season, orbit) and the window list is fixed by (h, w, patchsize, overlap), so the orbit and the repaired sites
// are planned once (data/region.py: ResidentWindows; the table is region_repair.hip's) and a window then costs this launch:
//
//   pc_region_window   out (6, ps, ps) = (v - mean[c]) / std[c], channels [S2 R G B NIR | S1 VV VH], v = the patch value where the slice
//                      [start, start + count) of the table holds an entry for the site, the raster's value otherwise
//
// Store-once.  The patch value replaces the raw value BEFORE the normalisation and every output element is stored to global memory
// exactly once, by the thread that owns it: no ordering between the stores of different waves is relied upon.  A workgroup owns (channel c,
// a block of R rows) = the contiguous range [(c * ps + r0) * ps, (c * ps + r0 + rows) * ps) of the table's index space.  The first two
// lanes of wave 0 find the range's two ends in the ascending slice by binary search and hand them to the workgroup through LDS.  A
// workgroup whose range holds no entry -- every workgroup of a window without NaN -- normalises and stores straight from registers.
// Otherwise it stages its R x ps tile of RAW values in LDS, lays the entries over it after a barrier (an entry's place is checked against
// the tile whatever the table holds), and after a second barrier every thread normalises and stores the groups it staged.
// R = pc_region_window_rows(ps): at most 16 rows and at most 4,096 elements (16 KB of LDS; one row of up to PC_REGION_WINDOW_MAX_PS = 8,192
// elements = 32 KB at the widest).
//
// Loads are region_load.h's (window origins are arbitrary: 16-byte access at 4-byte alignment, 8-byte for uint16, which converts
// exactly); a thread moves V = 4 consecutive pixels of a row, or V = 1 when ps % 4 != 0 or the output is not 16-byte aligned.  The
// division is the fp32 division of pc_select_normalize (train_ops.hip), the same expression on the same operands.
// No loop's trip count depends on another lane's, wave's or workgroup's progress; both barriers sit in code the whole workgroup takes.
#include "common.h"
#include "region_load.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr int RW_MAX_ROWS = 16;            // rows of a workgroup's tile, at most
constexpr int RW_TILE = 4096;              // elements of a tile of more than one row, at most (16 KB)
constexpr int RW_HEAD = 16;                // bytes of LDS in front of the tile
static_assert(PC_REGION_WINDOW_MAX_PS * 4 <= 32 * 1024, "one row of the widest window is a tile of at most 32 KB");
static_assert(6 * (int64_t)PC_REGION_WINDOW_MAX_PS * PC_REGION_WINDOW_MAX_PS < ((int64_t)1 << 31), "idx is int32 in the window's own space");

struct RegionWindowArgs {
    const void* src[6];                     // channel c's source plane at the window's origin (c < 4: S2 in its own type, else fp32 S1)
    int w, ps, R;                           // source row stride; window side; rows per workgroup
    pc_fastdiv div;                         // groups per row: ps / V
    float mean[6], stdv[6];
    const int32_t* idx; const float* val;   // the window's slice of the patch table (already offset by start)
    int count;
    float* out;
};

__device__ __forceinline__ float rw_norm(float v, float mean, float stdv) { return (v - mean) / stdv; }

// the first entry of the ascending slice idx[0, n) that is >= key
__device__ __forceinline__ int rw_lower_bound(const int32_t* idx, int n, int key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <typename T, int V>
__device__ __forceinline__ void rw_channel(const RegionWindowArgs& a, int c, int r0, int rows, float* tile, int* ends) {
    const int t = threadIdx.x;
    const T* src = pc_pin_ptr(reinterpret_cast<const T*>(a.src[c]));
    int w = a.w, ps = a.ps;
    pc_fastdiv div = a.div;
    float mean = a.mean[c], stdv = a.stdv[c];
    pc_pin(w); pc_pin(ps); pc_pin(div); pc_pin(mean); pc_pin(stdv);
    const int first = (c * ps + r0) * ps;                               // (< 6 * ps * ps < 2^31: host)
    const int n = rows * ps, groups = n / V;                            // (n <= 8192)
    float* out = pc_pin_ptr(a.out + first);
    int e0 = 0, e1 = 0;
    if (a.count > 0) {                                                   // (a kernel argument: uniform)
        if (t < 2) ends[t] = rw_lower_bound(a.idx, a.count, first + t * n);
        __syncthreads();
        e0 = __builtin_amdgcn_readfirstlane(ends[0]); e1 = __builtin_amdgcn_readfirstlane(ends[1]);      // (one value per workgroup)
    }
    if (e0 >= e1) {
        // no entry in this workgroup's range: registers -> global
        for (int g = t; g < groups; g += RW_THREADS) {
            const int r = (int)pc_div((uint32_t)g, div), j = (g - r * (int)div.d) * V;
            const T* p = src + (int64_t)(r0 + r) * w + j;
            if constexpr (V == 4) {
                const f32x4 v = rg_ld4(p);
                pc_st4(out + r * ps + j, f32x4{rw_norm(v[0], mean, stdv), rw_norm(v[1], mean, stdv), rw_norm(v[2], mean, stdv),
                                               rw_norm(v[3], mean, stdv)});
            } else {
                out[r * ps + j] = rw_norm(rg_val(p), mean, stdv);
            }
        }
        return;
    }
    // raw values -> LDS
    for (int g = t; g < groups; g += RW_THREADS) {
        const int r = (int)pc_div((uint32_t)g, div), j = (g - r * (int)div.d) * V;
        const T* p = src + (int64_t)(r0 + r) * w + j;
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(tile + r * ps + j) = rg_ld4(p);      // (ps % 4 == 0: 16-byte aligned in LDS)
        else tile[r * ps + j] = rg_val(p);
    }
    __syncthreads();
    // the entries of the range over it: raw, un-normalised repaired values
    for (int e = e0 + t; e < e1; e += RW_THREADS) {
        const int p = a.idx[e] - first;
        if (p >= 0 && p < n) tile[p] = a.val[e];                         // inside the tile whatever the table holds
    }
    __syncthreads();
    for (int g = t; g < groups; g += RW_THREADS) {
        const int o = g * V;                                             // (= r * ps + j: the tile is the output range itself)
        if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(tile + o);
            pc_st4(out + o, f32x4{rw_norm(v[0], mean, stdv), rw_norm(v[1], mean, stdv), rw_norm(v[2], mean, stdv), rw_norm(v[3], mean, stdv)});
        } else {
            out[o] = rw_norm(tile[o], mean, stdv);
        }
    }
}

// V = 4: ps % 4 == 0 and a 16-byte aligned output; V = 1: anything
template <typename T2, int V>
__global__ __launch_bounds__(RW_THREADS) void region_window_kernel(const RegionWindowArgs a) {
    // all LDS in the dynamic region, the tile at a multiple of 16 bytes: a static variable in front of it would shift its base off the
    // alignment of the 16-byte LDS accesses
    extern __shared__ __attribute__((aligned(16))) unsigned char rw_lds[];      // [RW_HEAD bytes: the range's two ends][R * ps floats: the tile]
    int* ends = reinterpret_cast<int*>(rw_lds);
    float* rw_tile = reinterpret_cast<float*>(rw_lds + RW_HEAD);
    const int c = blockIdx.y, r0 = blockIdx.x * a.R;                     // (r0 < ps: the grid)
    const int rows = min(a.R, a.ps - r0);
    if constexpr (sizeof(T2) == 4) {
        rw_channel<float, V>(a, c, r0, rows, rw_tile, ends);
    } else {
        if (c < 4) rw_channel<T2, V>(a, c, r0, rows, rw_tile, ends);     // (blockIdx.y: the whole workgroup takes one branch)
        else rw_channel<float, V>(a, c, r0, rows, rw_tile, ends);
    }
}

}  // namespace

extern "C" int pc_region_window_rows(int ps) {
    if (ps < 1 || ps > PC_REGION_WINDOW_MAX_PS) return 0;
    int R = RW_TILE / ps;
    if (R > RW_MAX_ROWS) R = RW_MAX_ROWS;
    if (R > ps) R = ps;
    return R < 1 ? 1 : R;
}

extern "C" int pc_region_window(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, int S, int C2, int C1, int h,
                                int w, const int32_t* band_sel, int x, int y, int season, int ps, const float* mean6, const float* std6,
                                const int32_t* idx, const float* val, int64_t cap, int64_t start, int64_t count, float* out,
                                void* stream) {
    if (!s2 || !s1 || !band_sel || !mean6 || !std6 || !out) return PC_EINVAL;
    if (S < 1 || C2 < 1 || C1 < 1 || h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31)) return PC_EINVAL;
    if (ps < 1 || ps > PC_REGION_WINDOW_MAX_PS) return PC_EINVAL;
    if (x < 0 || y < 0 || ps > h || ps > w || x > h - ps || y > w - ps) return PC_EINVAL;         // the window stays inside the raster
    if (season < 0 || season >= S) return PC_EINVAL;
    if (orbit < 0 || orbit > 1 || (orbit == 1 && !s1_asc)) return PC_EINVAL;
    for (int c = 0; c < 6; ++c)
        if (band_sel[c] < 0 || band_sel[c] >= (c < 4 ? C2 : C1)) return PC_EINVAL;
    if (count < 0 || start < 0 || cap < 0 || count > 6 * (int64_t)ps * ps) return PC_EINVAL;
    if (count > 0 && (!idx || !val || start + count > cap)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s1_asc) | reinterpret_cast<uintptr_t>(out) |
         reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(val)) & 3)
        return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(s2) & (s2_u16 ? 1 : 3)) return PC_EINVAL;
    const bool vec = (ps & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int64_t plane = (int64_t)h * w, origin = (int64_t)x * w + y;
    const float* s1_src = orbit ? s1_asc : s1;
    RegionWindowArgs a{};
    for (int c = 0; c < 4; ++c) {
        const int64_t at = ((int64_t)season * C2 + band_sel[c]) * plane + origin;
        a.src[c] = s2_u16 ? (const void*)(reinterpret_cast<const uint16_t*>(s2) + at) : (const void*)(reinterpret_cast<const float*>(s2) + at);
    }
    for (int c = 4; c < 6; ++c) a.src[c] = s1_src + ((int64_t)season * C1 + band_sel[c]) * plane + origin;
    a.w = w; a.ps = ps; a.R = pc_region_window_rows(ps);
    a.div = pc_make_fastdiv((uint32_t)(vec ? ps / 4 : ps));
    for (int c = 0; c < 6; ++c) { a.mean[c] = mean6[c]; a.stdv[c] = std6[c]; }
    a.idx = count > 0 ? idx + start : nullptr; a.val = count > 0 ? val + start : nullptr; a.count = (int)count;
    a.out = out;
    const dim3 grid((ps + a.R - 1) / a.R, 6);
    const size_t lds = RW_HEAD + (size_t)a.R * ps * sizeof(float);       // the tile: <= 32 KB
    hipStream_t st = (hipStream_t)stream;
    if (s2_u16) {
        if (vec) hipLaunchKernelGGL((region_window_kernel<uint16_t, 4>), grid, dim3(RW_THREADS), lds, st, a);
        else hipLaunchKernelGGL((region_window_kernel<uint16_t, 1>), grid, dim3(RW_THREADS), lds, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((region_window_kernel<float, 4>), grid, dim3(RW_THREADS), lds, st, a);
        else hipLaunchKernelGGL((region_window_kernel<float, 1>), grid, dim3(RW_THREADS), lds, st, a);
    }
    PC_CHECK_LAUNCH();
    return 0;
}
