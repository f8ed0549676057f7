// product.hip -- the product grid: k x k block sums of the 10 m maps (the reference's README: "for the final product and evaluation, we
// recommend aggregating the raw output to a 1ha (100x100m) grid"), per ensemble member and stitched across windows on the device.
//
//   pc_product_accumulate  one window: cells[m][y / cell][x / cell] += popdense[m][y][x] / visits[y][x] over the window interior
//   pc_product_finalize    mean and (n - 1) standard deviation over the members of every cell, two passes in double
//   pc_block_sum           the plain k x k sum pooling of one (H, W) map (same geometry, same summation order)
//
// A hectare cell is never aligned with a window interior (overlap 128 = 12 cells + 8 px), and the ensemble spread of a cell is the spread
// of the members' cell TOTALS, which is no function of the 10 m std map: each member's total has to be completed across windows (every
// pixel weighted by 1 / its visit count) before anything is squared.  Hence one plane per member.
//
// No floating-point atomics: a launch hands every coarse cell to exactly one lane, which adds to it with a plain read-modify-write;
// launches of one stream serialise.  The summation order is a function of the geometry alone, so two runs give the same bits.
// HBM-bound streaming kernels: 4 M + 2 bytes read per pixel, coalesced rows, nothing written but the small planes.
#include "common.h"

namespace {

constexpr int PG_MB = 8;          // members per pass: their column sums are held in registers
constexpr int PG_R = 8;           // rows per group of loads in flight
constexpr int PG_MAX_GRID = 2048;

struct BlockSumArgs {
    const float* src;               // pixel (m, y, x) of the raster at src[m * mstride + (y - oy) * rstride + (x - ox)]
    int64_t mstride; int rstride, oy, ox;
    const int16_t* visits;          // [H][W] (VISITS only)
    int W;
    int y0, y1, x0, x1;             // the region to sum (raster coordinates, clipped to the raster, not empty)
    int cell, cpw;                  // cpw = cells per tile along x: a tile is one row of cpw whole cells, clipped to the region
    int cx0, ntx, ntiles;           // first cell column of the region; tiles per cell row; tiles in all
    int cy0;
    float* cells; int64_t pstride; int Wc;     // cells[m * pstride + cy * Wc + cx]
    int M;
};

// Tile = cell row cy x cell columns [cxa, cxb) (cxb - cxa <= cpw), clipped to the region: at most `cell` rows.  cell <= 256: the tile is at
// most 256 columns wide, lane t owns column xa + t; cell > 256: cpw = 1 and lane t owns columns xa + t, xa + t + 256, ... of the one cell.
// Order of the additions into a cell, per member: each lane top to bottom over its column(s), then the lanes of the cell left to right,
// then the plane.  A term therefore passes through at most 1 (division) + (cell - 1) + (cell - 1) + 1 roundings per launch for
// cell <= 256, plus one for every later launch that adds to the same cell.
template <bool VISITS, bool ACCUM>
__global__ __launch_bounds__(256) void block_sum_kernel(const BlockSumArgs a) {
    __shared__ float part[PG_MB][256];
    const int t = threadIdx.x;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
        const int cy = a.cy0 + ty, cxa = a.cx0 + tx * a.cpw;
        const int ya = max(cy * a.cell, a.y0), yb = (int)min((int64_t)(cy + 1) * a.cell, (int64_t)a.y1);
        const int xa = max(cxa * a.cell, a.x0), xb = (int)min((int64_t)(cxa + a.cpw) * a.cell, (int64_t)a.x1);
        const int ncell = (xb - 1) / a.cell - cxa + 1;
        for (int m0 = 0; m0 < a.M; m0 += PG_MB) {
            const int mc = min(PG_MB, a.M - m0);
            float acc[PG_MB];
#pragma unroll
            for (int k = 0; k < PG_MB; ++k) acc[k] = 0.f;
            for (int x = xa + t; x < xb; x += 256) {
                const float* col = a.src + m0 * a.mstride + (x - a.ox);
                // PG_R rows at a time: every load of the group is issued before the first addition waits for one (a row past the tile is
                // loaded from the tile's last row and enters the sum as + 0)
                for (int y = ya; y < yb; y += PG_R) {
                    float v[PG_R], p[PG_MB][PG_R];
                    int64_t row[PG_R];
#pragma unroll
                    for (int r = 0; r < PG_R; ++r) {
                        const int yr = min(y + r, yb - 1);
                        row[r] = (int64_t)(yr - a.oy) * a.rstride;
                        v[r] = VISITS ? (float)a.visits[(int64_t)yr * a.W + x] : 1.f;
                    }
#pragma unroll
                    for (int k = 0; k < PG_MB; ++k)
                        if (k < mc) {
#pragma unroll
                            for (int r = 0; r < PG_R; ++r) p[k][r] = col[k * a.mstride + row[r]];
                        }
#pragma unroll
                    for (int k = 0; k < PG_MB; ++k)
                        if (k < mc) {
#pragma unroll
                            for (int r = 0; r < PG_R; ++r) acc[k] += y + r < yb ? (VISITS ? p[k][r] / v[r] : p[k][r]) : 0.f;
                        }
                }
            }
#pragma unroll
            for (int k = 0; k < PG_MB; ++k) part[k][t] = acc[k];
            __syncthreads();
            // one lane per (member, cell): its column sums in a fixed order, then the one read-modify-write of the cell in this launch
            for (int u = t; u < mc * ncell; u += 256) {
                const int k = u / ncell, j = u - k * ncell;
                const int la = max((cxa + j) * a.cell, xa) - xa;
                const int lb = min((int)min((int64_t)(cxa + j + 1) * a.cell, (int64_t)xb) - xa, 256);
                float s = part[k][la];
                for (int l = la + 1; l < lb; ++l) s += part[k][l];
                float* o = a.cells + (m0 + k) * a.pstride + (int64_t)cy * a.Wc + (cxa + j);
                *o = ACCUM ? *o + s : s;
            }
            __syncthreads();
        }
    }
}

// mean = sum_m T_m / M;  std = sqrt(sum_m (T_m - mean)^2 / (M - 1)): two passes over the M totals of a cell in double (the sum-of-squares
// form of stitch_finalize_kernel cancels: a cell total is ~100 x a pixel value, its spread over members a small fraction of it)
__global__ __launch_bounds__(256) void product_finalize_kernel(const float* __restrict__ cells, int M, int64_t n, float* __restrict__ mean,
                                                               float* __restrict__ stdv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += (double)cells[m * n + i];
        const double mu = s / (double)M;
        double ss = 0.0;
        for (int m = 0; m < M; ++m) {
            const double d = (double)cells[m * n + i] - mu;
            ss += d * d;
        }
        mean[i] = (float)mu;
        stdv[i] = M > 1 ? (float)sqrt(ss / (double)(M - 1)) : 0.f;
    }
}

// tiles of the region [y0, y1) x [x0, x1) (not empty) on the cell grid; false when they do not fit the 32-bit tile index
bool block_sum_tiles(BlockSumArgs& a) {
    a.cpw = a.cell >= 256 ? 1 : 256 / a.cell;
    a.cy0 = a.y0 / a.cell;
    a.cx0 = a.x0 / a.cell;
    const int ncy = (a.y1 - 1) / a.cell - a.cy0 + 1, ncx = (a.x1 - 1) / a.cell - a.cx0 + 1;
    a.ntx = (ncx + a.cpw - 1) / a.cpw;
    const int64_t ntiles = (int64_t)a.ntx * ncy;
    if (ntiles > INT32_MAX) return false;
    a.ntiles = (int)ntiles;
    return true;
}

}  // namespace

extern "C" int pc_product_accumulate(const float* popdense, int M, int ps_y, int ps_x, int overlap, int yl, int xl,
                                     const int16_t* visits, int H, int W, int cell, float* cells, void* stream) {
    if (!popdense || !visits || !cells || M < 1 || H < 1 || W < 1 || cell < 1 || overlap < 0) return PC_EINVAL;
    if (ps_y <= 2 * overlap || ps_x <= 2 * overlap) return 0;
    BlockSumArgs a{};
    a.y0 = yl + overlap > 0 ? yl + overlap : 0;
    a.x0 = xl + overlap > 0 ? xl + overlap : 0;
    a.y1 = yl + ps_y - overlap < H ? yl + ps_y - overlap : H;
    a.x1 = xl + ps_x - overlap < W ? xl + ps_x - overlap : W;
    if (a.y1 <= a.y0 || a.x1 <= a.x0) return 0;              // the interior lies outside the raster
    a.src = popdense; a.mstride = (int64_t)ps_y * ps_x; a.rstride = ps_x; a.oy = yl; a.ox = xl;
    a.visits = visits; a.W = W; a.cell = cell; a.M = M;
    a.Wc = (W + cell - 1) / cell;
    a.cells = cells; a.pstride = (int64_t)((H + cell - 1) / cell) * a.Wc;
    if (!block_sum_tiles(a)) return PC_EINVAL;
    hipLaunchKernelGGL((block_sum_kernel<true, true>), dim3(a.ntiles < PG_MAX_GRID ? a.ntiles : PG_MAX_GRID), dim3(256), 0,
                       (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_product_finalize(const float* cells, int M, int64_t n, float* mean, float* stdv, void* stream) {
    if (!cells || !mean || !stdv || M < 1 || n < 0) return PC_EINVAL;
    if (n == 0) return 0;
    const int64_t g = (n + 255) / 256;
    hipLaunchKernelGGL(product_finalize_kernel, dim3((int)(g < PG_MAX_GRID ? g : PG_MAX_GRID)), dim3(256), 0, (hipStream_t)stream, cells, M,
                       n, mean, stdv);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_block_sum(const float* map, int H, int W, int cell, float* out, void* stream) {
    if (!map || !out || H < 1 || W < 1 || cell < 1) return PC_EINVAL;
    BlockSumArgs a{};
    a.y1 = H; a.x1 = W;
    a.src = map; a.rstride = W; a.W = W; a.cell = cell; a.M = 1;
    a.Wc = (W + cell - 1) / cell;
    a.cells = out;
    if (!block_sum_tiles(a)) return PC_EINVAL;
    hipLaunchKernelGGL((block_sum_kernel<false, false>), dim3(a.ntiles < PG_MAX_GRID ? a.ntiles : PG_MAX_GRID), dim3(256), 0,
                       (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}
