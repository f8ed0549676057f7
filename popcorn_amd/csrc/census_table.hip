// census_table.hip -- the per-member census table: every member's census-unit totals, accumulated while the windows are stitched, and the
// per-unit detail maps painted from such tables.
//
//   pc_census_accumulate  one window: table[m][off[l] + boundary_l[y][x]] += fix(popdense[m][y][x] / visits[y][x]) over the window interior,
//                         for every member m and every census level l <= PC_CENSUS_MAX_LEVELS in ONE pass over the pixels
//   pc_census_finalize    totals (double), mean and (n - 1) standard deviation over the members of every unit, two passes in double
//   pc_census_paint       out_k[i] = tables_k[boundary[i]] for K <= PC_CENSUS_MAX_PLANES tables, the boundary plane read once
//
// The ensemble spread of a unit total is the spread over members of each member's own total (the argument of product.hip's header): one
// row of the table per member, each completed across windows with every pixel weighted by 1 / its visit count.
//
// Arithmetic.  fix(q) = llrint((double)q * 2^PC_CENSUS_FIX_SHIFT): the fp32 quotient of block_sum_kernel<true, .> put on a 2^-30 grid, summed
// as 64-bit integers.  Integer addition is associative, so the table holds the same bits for any window order, grid size, tile shape and
// rank sharding, although atomics are used (product.hip's "no floating-point atomics" rule, met with integer atomics: census units have
// no geometry that could hand a unit to one lane).  Range: a term must lie in [0, 2^32) and a unit total below 2^33 ~ 8.6e9 per member
// (2^63 / 2^30).  A term that is NaN, +-Inf, negative or >= 2^32 adds nothing and sets bit 0 of *flags: nothing wraps silently.
//
// Structure of the accumulate (4 M + 2 + 4 L bytes read per pixel and member pass, coalesced rows, one column per lane as in
// block_sum_kernel; measured times and counters: DESIGN.md section 13).  A workgroup owns compact tiles of CT_ROWS rows x 256 columns of the interior, so it touches few units.  Sums stay
// on chip in three stages:
//   1. registers: a lane walks its column top to bottom and keeps ONE running sum per member plus, per level, its value where the current
//      unit began (units are runs along a column); it hands the difference on when the id changes and at the end of the tile;
//   2. wave: when the lanes that hand on agree on the id (readfirstlane, then ballot) their sums are reduced across the wave and one lane
//      adds; otherwise every lane adds its own;
//   3. LDS: while the ids of a level fit, the adds of stage 2 go to a table in LDS indexed by id (64-bit LDS integer atomics), CT_MB members
//      per pass, and the workgroup issues ONE global 64-bit atomic add per (member, id) it touched when it is done.  Levels with more ids
//      than the LDS table holds send the adds of stage 2 to the global table directly.
// No loop's trip count depends on another lane's, wave's or workgroup's progress: no hash probing, no compare-and-swap retry, no spin wait,
// no ticket; every loop bound is a function of the launch geometry.
#include "common.h"

namespace {

constexpr int CT_MB = 4;                 // members per pass: their running sums are held in registers, their LDS rows side by side
constexpr int CT_R = 8;                  // rows per group of loads in flight
constexpr int CT_ROWS = 32;              // rows of a tile
constexpr int CT_LDS_IDS = 4864;         // ids (of all levels together) the LDS table holds: CT_MB * 4864 * 8 B = 152 KB of the 160 KB
constexpr int CT_MAX_GRID = 2048;
constexpr int CT_WAVE_MIN = 8;           // lanes that must agree before the wave reduction (6 exchanges) replaces their own adds
constexpr double CT_FIX = (double)(1ull << PC_CENSUS_FIX_SHIFT);
static_assert(PC_CENSUS_FIX_SHIFT == 30, "ct_fix scales the fraction by 2^30");

typedef unsigned long long ct_u64;

struct CensusArgs {
    const float* src;               // pixel (m, y, x) of the raster at src[m * mstride + (y - oy) * rstride + (x - ox)]
    int64_t mstride; int rstride, oy, ox;
    const int16_t* visits;          // [H][W]
    int W;
    int y0, y1, x0, x1;             // the interior (raster coordinates, clipped to the raster, not empty)
    int ntx, ntiles;                // tiles per tile row; tiles in all
    int M, L;
    const int32_t* boundary[PC_CENSUS_MAX_LEVELS];
    int num_ids[PC_CENSUS_MAX_LEVELS], off[PC_CENSUS_MAX_LEVELS];
    int lds_off[PC_CENSUS_MAX_LEVELS];      // first slot of the level in an LDS row, -1: the level adds to the global table directly
    int lds_ids;                    // slots of an LDS row
    ct_u64* table; int64_t T;       // table[m * T + off[l] + id], two's complement
    int32_t* flags;
};

__device__ __forceinline__ long long ct_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// fix(q) for q in [0, 2^32): llrint((double)q * 2^30) without double arithmetic.  trunc(q) and q - trunc(q) are exact in fp32, so is the
// scaling of the fraction by 2^30; trunc(q) * 2^30 is an even integer, hence rounding the fraction's part to nearest-even rounds the sum
// to nearest-even.
__device__ __forceinline__ long long ct_fix(float q) {
    const float hi = truncf(q);
    const float lo = rintf((q - hi) * 1073741824.f);
    return (long long)(((ct_u64)(unsigned)hi << PC_CENSUS_FIX_SHIFT) + (ct_u64)(unsigned)lo);
}

// Stage 2 for one level: the lanes with `go` hand the sums run[0 .. mc) - start[0 .. mc) of unit `id` (in range) on.  Called by every lane
// of the wave in uniform control flow.
__device__ __forceinline__ void ct_hand_on(const CensusArgs& a, ct_u64* tab, int l, int m0, int mc, bool go, int id,
                                           const long long (&run)[CT_MB], const long long (&start)[CT_MB]) {
    const unsigned long long want = __ballot(go);
    if (!want) return;
    const int lead = __ffsll((long long)want) - 1;                // the first lane that hands on (wave-uniform: `want` is a ballot)
    const int first = __builtin_amdgcn_readlane(id, lead);        // its id: readfirstlane over the lanes with `go`
    const bool uniform = __ballot(go && id == first) == want && __popcll(want) >= CT_WAVE_MIN;
    const int lo = a.lds_off[l];
    const bool leader = (int)(threadIdx.x & 63) == lead;
#pragma unroll
    for (int k = 0; k < CT_MB; ++k)
        if (k < mc) {
            long long v = go ? run[k] - start[k] : 0;
            bool add = go;
            if (uniform) { v = ct_wave_sum(v); add = leader; }
            if (add && v != 0) {
                if (lo >= 0) atomicAdd(&tab[k * a.lds_ids + lo + id], (ct_u64)v);
                else atomicAdd(&a.table[(m0 + k) * a.T + a.off[l] + id], (ct_u64)v);
            }
        }
}

// the loads of CT_R rows of one column: visit counts, ids of every level, values of the pass's members (a row past the tile is loaded
// from the tile's last row and not used)
struct CtRows {
    short v[CT_R];
    float p[CT_MB][CT_R];
    int ids[PC_CENSUS_MAX_LEVELS][CT_R];
};

__device__ __forceinline__ void ct_load(const CensusArgs& a, CtRows& g, const float* col, int x, int y, int yb, int mc) {
    int64_t row[CT_R], brow[CT_R];
#pragma unroll
    for (int r = 0; r < CT_R; ++r) {
        const int yr = min(y + r, yb - 1);
        row[r] = (int64_t)(yr - a.oy) * a.rstride;
        brow[r] = (int64_t)yr * a.W + x;
        g.v[r] = a.visits[brow[r]];
    }
#pragma unroll
    for (int l = 0; l < PC_CENSUS_MAX_LEVELS; ++l)
        if (l < a.L) {
#pragma unroll
            for (int r = 0; r < CT_R; ++r) g.ids[l][r] = a.boundary[l][brow[r]];
        }
#pragma unroll
    for (int k = 0; k < CT_MB; ++k)
        if (k < mc) {
#pragma unroll
            for (int r = 0; r < CT_R; ++r) g.p[k][r] = col[k * a.mstride + row[r]];
        }
}

__global__ __launch_bounds__(256) void census_accumulate_kernel(const CensusArgs a) {
    extern __shared__ __attribute__((aligned(16))) ct_u64 ct_tab[];          // [mc][lds_ids]
    const int t = threadIdx.x;
    bool bad = false;
    for (int m0 = 0; m0 < a.M; m0 += CT_MB) {
        const int mc = min(CT_MB, a.M - m0);
        for (int i = t; i < mc * a.lds_ids; i += 256) ct_tab[i] = 0;
        __syncthreads();
        for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
            const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
            const int ya = a.y0 + ty * CT_ROWS, yb = min(ya + CT_ROWS, a.y1);
            const int xa = a.x0 + tx * 256, xb = min(xa + 256, a.x1);
            if (xa + (t & ~63) >= xb) continue;                       // a wave without a column (wave-uniform)
            const bool active = xa + t < xb;
            const int x = active ? xa + t : xb - 1;                   // an idle lane loads the tile's last column and adds nothing
            const float* col = a.src + m0 * a.mstride + (x - a.ox);
            // stage 1: run[k] = the sum of member k's terms down the column so far; start[l][k] = its value where the current unit of
            // level l began (cur[l], -1: none) -- one addition per term whatever the number of levels
            long long run[CT_MB], start[PC_CENSUS_MAX_LEVELS][CT_MB];
            int cur[PC_CENSUS_MAX_LEVELS];
#pragma unroll
            for (int k = 0; k < CT_MB; ++k) run[k] = 0;
#pragma unroll
            for (int l = 0; l < PC_CENSUS_MAX_LEVELS; ++l) {
                cur[l] = -1;
#pragma unroll
                for (int k = 0; k < CT_MB; ++k) start[l][k] = 0;
            }
            // CT_R rows at a time, the loads of the next group in flight while this one is summed
            CtRows g;
            ct_load(a, g, col, x, ya, yb, mc);
            for (int y = ya; y < yb; y += CT_R) {
                CtRows nx;
                const bool more = y + CT_R < yb;
                if (more) ct_load(a, nx, col, x, y + CT_R, yb, mc);
#pragma unroll
                for (int r = 0; r < CT_R; ++r) {
                    if (y + r >= yb) break;
                    long long term[CT_MB];
                    bool ok = true;
#pragma unroll
                    for (int k = 0; k < CT_MB; ++k) {
                        term[k] = 0;
                        if (k < mc) {
                            const float q = g.p[k][r] / (float)g.v[r];
                            const bool in = q >= 0.f && q < 4294967296.f;            // false for NaN
                            ok = ok && in;
                            if (in) term[k] = ct_fix(q);
                        }
                    }
                    bool any = false;
#pragma unroll
                    for (int l = 0; l < PC_CENSUS_MAX_LEVELS; ++l)
                        if (l < a.L) {
                            const int id = g.ids[l][r];
                            const int nid = active && (unsigned)id < (unsigned)a.num_ids[l] ? id : -1;
                            any = any || nid >= 0;
                            ct_hand_on(a, ct_tab, l, m0, mc, nid != cur[l] && cur[l] >= 0, cur[l], run, start[l]);
                            if (nid != cur[l]) {
                                cur[l] = nid;
#pragma unroll
                                for (int k = 0; k < CT_MB; ++k) start[l][k] = run[k];
                            }
                        }
#pragma unroll
                    for (int k = 0; k < CT_MB; ++k) run[k] += term[k];
                    bad = bad || (any && !ok);
                }
                if (more) g = nx;
            }
#pragma unroll
            for (int l = 0; l < PC_CENSUS_MAX_LEVELS; ++l)
                if (l < a.L) ct_hand_on(a, ct_tab, l, m0, mc, cur[l] >= 0, cur[l], run, start[l]);
        }
        __syncthreads();
        // one global add per (member, id) this workgroup touched
        for (int i = t; i < mc * a.lds_ids; i += 256) {
            const ct_u64 s = ct_tab[i];
            if (s) {
                const int k = i / a.lds_ids, j = i - k * a.lds_ids;
                int c = -1;
#pragma unroll
                for (int l = 0; l < PC_CENSUS_MAX_LEVELS; ++l)
                    if (l < a.L && a.lds_off[l] >= 0 && j >= a.lds_off[l] && j < a.lds_off[l] + a.num_ids[l]) c = a.off[l] + j - a.lds_off[l];
                if (c >= 0) atomicAdd(&a.table[(m0 + k) * a.T + c], s);
            }
        }
        __syncthreads();
    }
    if (bad) atomicOr(a.flags, 1);
}

// totals = table * 2^-30 (exact: |table| < 2^63 has at most 63 significant bits, the conversion rounds once); mean / std as
// product_finalize_kernel: two passes over the M totals of a unit in double
__global__ __launch_bounds__(256) void census_finalize_kernel(const long long* __restrict__ table, int M, int64_t n, double* __restrict__ totals,
                                                              float* __restrict__ mean, float* __restrict__ stdv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) {
            const double tm = (double)table[m * n + i] * (1.0 / CT_FIX);
            totals[m * n + i] = tm;
            s += tm;
        }
        const double mu = s / (double)M;
        double ss = 0.0;
        for (int m = 0; m < M; ++m) {
            const double d = (double)table[m * n + i] * (1.0 / CT_FIX) - mu;
            ss += d * d;
        }
        mean[i] = (float)mu;
        stdv[i] = M > 1 ? (float)sqrt(ss / (double)(M - 1)) : 0.f;
    }
}

// ---- paint: K planes from one pass over the boundary plane -----------------------------------------------------------------------------
struct PaintArgs {
    const int32_t* boundary; int64_t n;
    int K, num_ids;
    const float* tables[PC_CENSUS_MAX_PLANES];
    float* out[PC_CENSUS_MAX_PLANES];
    int64_t head; int vec;          // elements before the first 16-byte boundary of `boundary`; planes whose 16-byte phase agrees with it
};

__device__ __forceinline__ float ct_pick(const float* tab, int id, int num_ids) { return (unsigned)id < (unsigned)num_ids ? tab[id] : 0.f; }

// any 4-byte aligned band (a rank's row band starts at r0 * w): a scalar head up to boundary's first 16-byte boundary, 16-byte loads from
// there and 16-byte stores to every plane that is aligned at the same element (bit k of vec), scalar stores to the others, scalar tail
__global__ __launch_bounds__(256) void census_paint_kernel(const PaintArgs a) {
    const int32_t* bv = a.boundary + a.head;
    const int64_t n4 = (a.n - a.head) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int4 b = *reinterpret_cast<const int4*>(bv + 4 * i);
#pragma unroll
        for (int k = 0; k < PC_CENSUS_MAX_PLANES; ++k)
            if (k < a.K) {
                const float* tab = a.tables[k];
                const f32x4 o = f32x4{ct_pick(tab, b.x, a.num_ids), ct_pick(tab, b.y, a.num_ids), ct_pick(tab, b.z, a.num_ids),
                                      ct_pick(tab, b.w, a.num_ids)};
                float* dst = a.out[k] + a.head + 4 * i;
                if ((a.vec >> k) & 1) pc_st4(dst, o);
                else { dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2]; dst[3] = o[3]; }
            }
    }
    if (blockIdx.x == 0) {
        for (int64_t j = threadIdx.x; j < a.head + (a.n - a.head - 4 * n4); j += 256) {
            const int64_t i = j < a.head ? j : a.head + 4 * n4 + (j - a.head);
            const int id = a.boundary[i];
#pragma unroll
            for (int k = 0; k < PC_CENSUS_MAX_PLANES; ++k)
                if (k < a.K) a.out[k][i] = ct_pick(a.tables[k], id, a.num_ids);
        }
    }
}

}  // namespace

extern "C" int pc_census_accumulate(const float* popdense, int M, int ps_y, int ps_x, int overlap, int yl, int xl, const int16_t* visits,
                                    int H, int W, int L, const int32_t* const* boundaries, const int32_t* num_ids, const int32_t* off,
                                    int64_t* table, int64_t T, int32_t* flags, void* stream) {
    if (!popdense || !visits || !boundaries || !num_ids || !off || !table || !flags) return PC_EINVAL;
    if (M < 1 || H < 1 || W < 1 || overlap < 0 || L < 1 || L > PC_CENSUS_MAX_LEVELS || T < 1) return PC_EINVAL;
    CensusArgs a{};
    int used = 0;
    for (int l = 0; l < L; ++l) {
        if (!boundaries[l] || num_ids[l] < 1 || off[l] < 0 || (int64_t)off[l] + num_ids[l] > T) return PC_EINVAL;
        a.boundary[l] = boundaries[l]; a.num_ids[l] = num_ids[l]; a.off[l] = off[l];
        // the LDS table takes the levels in order while they fit; the others add to the global table
        if (used + num_ids[l] <= CT_LDS_IDS) { a.lds_off[l] = used; used += num_ids[l]; }
        else a.lds_off[l] = -1;
    }
    if (ps_y <= 2 * overlap || ps_x <= 2 * overlap) return 0;
    a.y0 = yl + overlap > 0 ? yl + overlap : 0;
    a.x0 = xl + overlap > 0 ? xl + overlap : 0;
    a.y1 = yl + ps_y - overlap < H ? yl + ps_y - overlap : H;
    a.x1 = xl + ps_x - overlap < W ? xl + ps_x - overlap : W;
    if (a.y1 <= a.y0 || a.x1 <= a.x0) return 0;              // the interior lies outside the raster
    a.src = popdense; a.mstride = (int64_t)ps_y * ps_x; a.rstride = ps_x; a.oy = yl; a.ox = xl;
    a.visits = visits; a.W = W; a.M = M; a.L = L;
    a.lds_ids = used;
    a.table = reinterpret_cast<ct_u64*>(table); a.T = T; a.flags = flags;
    a.ntx = (a.x1 - a.x0 + 255) / 256;
    a.ntiles = a.ntx * ((a.y1 - a.y0 + CT_ROWS - 1) / CT_ROWS);       // (< 2^31: at most 2^23 x 2^26 / 2^13 tiles of a 2^31-pixel side)
    const size_t lds = (size_t)(M < CT_MB ? M : CT_MB) * used * sizeof(ct_u64);
    static pc_launch_setup setup;
    const hipError_t e = setup(reinterpret_cast<const void*>(&census_accumulate_kernel), (size_t)CT_MB * CT_LDS_IDS * sizeof(ct_u64), PC_SETUP_LDS,
                               __PRETTY_FUNCTION__);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(census_accumulate_kernel, dim3(a.ntiles < CT_MAX_GRID ? a.ntiles : CT_MAX_GRID), dim3(256), lds, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_census_finalize(const int64_t* table, int M, int64_t T, double* totals, float* mean, float* stdv, void* stream) {
    if (!table || !totals || !mean || !stdv || M < 1 || T < 0) return PC_EINVAL;
    if (T == 0) return 0;
    const int64_t g = (T + 255) / 256;
    hipLaunchKernelGGL(census_finalize_kernel, dim3((int)(g < CT_MAX_GRID ? g : CT_MAX_GRID)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(table), M, T, totals, mean, stdv);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_census_paint(const int32_t* boundary, int64_t n, int num_ids, int K, const float* const* tables, float* const* out,
                               void* stream) {
    if (!boundary || !tables || !out || n < 0 || num_ids < 1 || K < 1 || K > PC_CENSUS_MAX_PLANES) return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(boundary) & 3) return PC_EINVAL;
    if (n == 0) return 0;
    PaintArgs a{};
    a.boundary = boundary; a.n = n; a.K = K; a.num_ids = num_ids;
    a.head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(boundary) & 15)) & 15) >> 2);
    if (a.head > n) a.head = n;
    for (int k = 0; k < K; ++k) {
        if (!tables[k] || !out[k] || (reinterpret_cast<uintptr_t>(out[k]) & 3)) return PC_EINVAL;
        a.tables[k] = tables[k]; a.out[k] = out[k];
        if ((reinterpret_cast<uintptr_t>(out[k] + a.head) & 15) == 0) a.vec |= 1 << k;
    }
    int64_t g = (n / 4 + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(census_paint_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}
