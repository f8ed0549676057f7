// Nearest-value NaN fill of Sentinel-1 / -2 inputs (data/PopulationDataset.py:526-551 interpolate_nan: scipy griddata "nearest" over the
// np.where indices of the whole (C, h, w) array).  Exact separable Euclidean feature transform in 3-D index space (c, i, j):
//
//   (a) count   per (sample, plane): NaN / known entries inside the sample's extent -> counts[b] = {nan, known}, plane_nan[b][c].
//               Every later launch reads them and returns at once for a sample without NaN (a NaN-free window costs one read).
//   (b) rows    per (sample, plane, row): nearest known column of every pixel (left prefix-max / right suffix-min block scans),
//               ties to the left column.  col[i][j] = that column, or -1 for a row without a known entry.
//   (c) columns one thread per column (neighbouring lanes read neighbouring columns): lower envelope of
//               f_i'(i) = (i - i')^2 + (j - col[i'][j])^2 over the rows i' that hold a known entry (Felzenszwalb / Meijster) with
//               exact integer breakpoints, ties to the smaller row; at each NaN site col[i][j] is overwritten with the winner
//               {row i', offset j - j'} (29 bits), or -1 when the plane holds no known entry.
//   (d) combine per NaN target (c, i, j): the plane c' minimising D2(c', i, j) + (c - c')^2, ties to the smaller c' (the 3-D minimum
//               is the minimum over planes of that plane's 2-D minimum), and a copy of the winning value (bit-exact).
//   (e) a sample with NaNs and fewer than 4 known entries is zeroed over its whole extent (PopulationDataset.py:541-543).
//
// Together: every NaN takes A[q*] with q* = argmin over known q of (|p - q|^2, q_c, q_i, q_j) in lexicographic order.
// Entries outside a sample's extent (hw[b], anchored top-left like the collate's padding) are neither sources nor targets.
#include <climits>
#include "common.h"

namespace {

constexpr int NF_THREADS = 256;
constexpr int NF_TILE = 4 * NF_THREADS;         // row pass: four consecutive columns per thread
constexpr int NF_COUNT_ROWS = 8;                // count pass: rows per workgroup
constexpr int NF_OFF = 16383;                   // bias of the column offset in the packed winner (|j - j'| <= 16383)

struct nf_ws {
    int32_t* plane_nan;   // [B * C]
    int32_t* col;         // [B * C][H][W]
    int2* stack;          // [B * C][H][W]: per column, envelope entries {row | start << 16, column of the row's nearest known}
};

__host__ __device__ inline int64_t nf_align(int64_t n) { return (n + 255) & ~int64_t(255); }

__device__ __forceinline__ void nf_extent(const int32_t* hw, int b, int H, int W, int& h, int& w) {
    h = H;
    w = W;
    if (hw) {
        h = min(max(hw[2 * b], 0), H);
        w = min(max(hw[2 * b + 1], 0), W);
    }
}

// fill mode of a sample: 0 = nothing to do (no NaN), 1 = fill, 2 = zero the extent (NaNs and fewer than 4 known entries)
__device__ __forceinline__ int nf_mode(const unsigned long long* counts, int b) {
    const unsigned long long nan = counts[2 * b], known = counts[2 * b + 1];
    if (nan == 0) return 0;
    return known < 4 ? 2 : 1;
}

__device__ __forceinline__ bool nf_isnan(float v) { return __builtin_isnan(v); }

// ---- (a) counts -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_THREADS) nan_count_kernel(const float* __restrict__ x, const int32_t* __restrict__ hw,
                                                               unsigned long long* __restrict__ counts, int32_t* __restrict__ plane_nan,
                                                               int C, int H, int W, int vec4) {
    __shared__ int red[NF_THREADS / 64];
    const int pl = blockIdx.y, b = pl / C;
    int h, w;
    nf_extent(hw, b, H, W, h, w);
    const int i0 = blockIdx.x * NF_COUNT_ROWS;
    const int i1 = min(i0 + NF_COUNT_ROWS, h);
    if (i0 >= i1 || w <= 0) return;                     // workgroup-uniform
    int n = 0;
    for (int i = i0; i < i1; ++i) {
        const float* row = x + ((int64_t)pl * H + i) * W;
        int j = threadIdx.x * 4;
        if (vec4) {
            const int w4 = w & ~3;
            for (; j < w4; j += 4 * NF_THREADS) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + j);
                n += nf_isnan(v[0]) + nf_isnan(v[1]) + nf_isnan(v[2]) + nf_isnan(v[3]);
            }
            for (j = w4 + threadIdx.x; j < w; j += NF_THREADS) n += nf_isnan(row[j]);
        } else {
            for (j = threadIdx.x; j < w; j += NF_THREADS) n += nf_isnan(row[j]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int k = 0; k < NF_THREADS / 64; ++k) tot += red[k];
        const unsigned long long all = (unsigned long long)(i1 - i0) * (unsigned long long)w;
        if (tot) {
            atomicAdd(plane_nan + pl, tot);
            atomicAdd(counts + 2 * b, (unsigned long long)tot);
        }
        atomicAdd(counts + 2 * b + 1, all - (unsigned long long)tot);
    }
}

// ---- block scans over one value per thread (256 threads = 4 waves) -------------------------------------------------------------------
// exclusive prefix maximum (identity -1) and the block's total
__device__ __forceinline__ int nf_scan_max(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc = max(inc, t);
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    int pre = -1;
    total = -1;
    for (int k = 0; k < NF_THREADS / 64; ++k) {
        if (k < wid) pre = max(pre, lds[k]);
        total = max(total, lds[k]);
    }
    int ex = __shfl_up(inc, 1);
    if (lane == 0) ex = -1;
    __syncthreads();                                    // lds is reused by the next call
    return max(ex, pre);
}

// exclusive suffix minimum (identity INT_MAX) and the block's total
__device__ __forceinline__ int nf_scan_min_rev(int v, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(inc, off);
        if (lane + off < 64) inc = min(inc, t);
    }
    if (lane == 0) lds[wid] = inc;
    __syncthreads();
    int post = INT_MAX;
    total = INT_MAX;
    for (int k = 0; k < NF_THREADS / 64; ++k) {
        if (k > wid) post = min(post, lds[k]);
        total = min(total, lds[k]);
    }
    int ex = __shfl_down(inc, 1);
    if (lane == 63) ex = INT_MAX;
    __syncthreads();
    return min(ex, post);
}

// ---- (b) nearest known column within each row ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NF_THREADS) nan_fill_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ hw,
                                                                   const unsigned long long* __restrict__ counts,
                                                                   const int32_t* __restrict__ plane_nan, int32_t* __restrict__ col,
                                                                   int C, int H, int W) {
    __shared__ int lds[NF_THREADS / 64];
    const int pl = blockIdx.y, b = pl / C, i = blockIdx.x;
    int h, w;
    nf_extent(hw, b, H, W, h, w);
    if (i >= h || w <= 0 || nf_mode(counts, b) != 1 || plane_nan[pl] == 0) return;     // workgroup-uniform
    const float* row = x + ((int64_t)pl * H + i) * W;
    int32_t* crow = col + ((int64_t)pl * H + i) * W;
    const int jt = 4 * threadIdx.x;
    // forward: nearest known column at or left of j (running maximum of the known columns), stored in crow
    int carry = -1;
    for (int t0 = 0; t0 < w; t0 += NF_TILE) {
        int run[4];
        int m = -1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = t0 + jt + e;
            if (j < w && !nf_isnan(row[j])) m = j;
            run[e] = m;
        }
        int total;
        const int pre = max(nf_scan_max(m, lds, total), carry);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = t0 + jt + e;
            if (j < w) crow[j] = max(pre, run[e]);
        }
        carry = max(carry, total);
    }
    // backward: nearest known column at or right of j (running minimum), then the nearer of the two, ties to the left.
    // Known columns are the ones whose left neighbour is themselves: the data is not read again.
    int rcarry = INT_MAX;
    for (int t0 = ((w - 1) / NF_TILE) * NF_TILE; t0 >= 0; t0 -= NF_TILE) {
        int left[4], run[4];
        int m = INT_MAX;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            const int j = t0 + jt + e;
            left[e] = j < w ? crow[j] : -1;
            if (j < w && left[e] == j) m = j;
            run[e] = m;
        }
        int total;
        const int post = min(nf_scan_min_rev(m, lds, total), rcarry);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = t0 + jt + e;
            if (j >= w) continue;
            const int l = left[e], r = min(post, run[e]);
            int best;
            if (l < 0) best = r == INT_MAX ? -1 : r;
            else if (r == INT_MAX) best = l;
            else best = (j - l) <= (r - j) ? l : r;
            crow[j] = best;
        }
        rcarry = min(rcarry, total);
    }
}

// ---- (c) lower envelope along each column ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int nf_floordiv(int num, int den) {        // den > 0
    return num >= 0 ? num / den : -((-num + den - 1) / den);
}

__global__ void __launch_bounds__(NF_THREADS) nan_fill_cols_kernel(const int32_t* __restrict__ hw,
                                                                   const unsigned long long* __restrict__ counts,
                                                                   const int32_t* __restrict__ plane_nan, int32_t* __restrict__ col,
                                                                   int2* __restrict__ stack, int C, int H, int W) {
    const int pl = blockIdx.y, b = pl / C;
    const int j = blockIdx.x * NF_THREADS + threadIdx.x;
    int h, w;
    nf_extent(hw, b, H, W, h, w);
    if (nf_mode(counts, b) != 1 || plane_nan[pl] == 0 || j >= w) return;
    int32_t* cp = col + (int64_t)pl * H * W + j;
    int2* sp = stack + (int64_t)pl * H * W + j;
    // envelope: entry k = {row v_k | start_k << 16, column c_k}; row v_k is the nearest for rows [start_k, start_{k+1})
    int top = -1, tv = 0, ts = 0, tc = 0;         // top entry, kept in registers
    for (int q = 0; q < h; ++q) {
        const int cq = cp[(int64_t)q * W];
        if (cq < 0) continue;                         // a row without a known entry drops out
        const int gq = (j - cq) * (j - cq);
        int st = 0;
        while (top >= 0) {
            // q is strictly nearer than v for rows i > ((q^2 + gq) - (v^2 + gv)) / (2 (q - v)): its region starts at floor(.) + 1
            const int gv = (j - tc) * (j - tc);
            st = nf_floordiv((q * q + gq) - (tv * tv + gv), 2 * (q - tv)) + 1;
            if (st > ts) break;
            if (--top >= 0) {                         // v is never the nearest: pop it
                const int2 e = sp[(int64_t)top * W];
                tv = e.x & 0xffff;
                ts = e.x >> 16;
                tc = e.y;
            }
        }
        if (top < 0) {
            top = 0;
            tv = q; ts = 0; tc = cq;
            sp[0] = make_int2(tv, tc);
        } else if (st < h) {
            ++top;
            tv = q; ts = st; tc = cq;
            sp[(int64_t)top * W] = make_int2(tv | (ts << 16), tc);
        }
    }
    // walk the rows: the winner of each NaN site replaces its entry in col (known sites hold col == j)
    if (top < 0) {
        for (int i = 0; i < h; ++i)
            if (cp[(int64_t)i * W] != j) cp[(int64_t)i * W] = -1;
        return;
    }
    const int last = top;
    int k = 0;
    int2 cur = sp[0];
    int2 nxt = last > 0 ? sp[W] : make_int2(0, 0);
    for (int i = 0; i < h; ++i) {
        while (k < last && (nxt.x >> 16) <= i) {
            ++k;
            cur = nxt;
            if (k < last) nxt = sp[(int64_t)(k + 1) * W];
        }
        int32_t* ci = cp + (int64_t)i * W;
        if (*ci != j) *ci = (cur.x & 0xffff) | ((j - cur.y + NF_OFF) << 14);
    }
}

// ---- (d) + (e) combine over planes / zero fill ---------------------------------------------------------------------------------------
template <int CMAX>
__global__ void __launch_bounds__(NF_THREADS) nan_fill_combine_kernel(float* __restrict__ x, const int32_t* __restrict__ hw,
                                                                      const unsigned long long* __restrict__ counts,
                                                                      const int32_t* __restrict__ col, int C, int H, int W) {
    const int b = blockIdx.y;
    int h, w;
    nf_extent(hw, b, H, W, h, w);
    const int mode = nf_mode(counts, b);
    if (mode == 0 || h <= 0 || w <= 0) return;
    const int64_t plane = (int64_t)H * W;
    float* xb = x + (int64_t)b * C * plane;
    const int32_t* cb = col + (int64_t)b * C * plane;
    const int64_t n = (int64_t)h * w;
    for (int64_t p = (int64_t)blockIdx.x * NF_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * NF_THREADS) {
        const int i = (int)(p / w), j = (int)(p - (int64_t)i * w);
        const int64_t o = (int64_t)i * W + j;
        if (mode == 2) {
            for (int c = 0; c < C; ++c) xb[c * plane + o] = 0.f;
            continue;
        }
        float v[CMAX];
        bool any = false;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            v[c] = c < C ? xb[c * plane + o] : 0.f;
            any |= c < C && nf_isnan(v[c]);
        }
        if (!any) continue;
        // per plane: squared in-plane distance of its nearest known entry and that entry's value (-1: none)
        int d2[CMAX];
        float src[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            d2[c] = -1;
            src[c] = 0.f;
            if (c >= C) continue;
            if (!nf_isnan(v[c])) {
                d2[c] = 0;
                src[c] = v[c];
            } else {
                const int e = cb[c * plane + o];
                if (e >= 0) {
                    const int vi = e & 0x3fff, dj = (e >> 14) - NF_OFF;
                    d2[c] = (i - vi) * (i - vi) + dj * dj;
                    src[c] = xb[c * plane + (int64_t)vi * W + (j - dj)];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c >= C || !nf_isnan(v[c])) continue;
            int best = INT_MAX;
            float val = 0.f;
#pragma unroll
            for (int c2 = 0; c2 < CMAX; ++c2) {
                if (c2 >= C || d2[c2] < 0) continue;
                const int d = d2[c2] + (c - c2) * (c - c2);
                if (d < best) {                       // ascending c2, strict: ties to the smaller plane
                    best = d;
                    val = src[c2];
                }
            }
            xb[c * plane + o] = val;                  // fill mode: >= 4 known entries, so some plane has one
        }
    }
}

nf_ws nf_carve(void* ws, int B, int C, int H, int W) {
    char* p = static_cast<char*>(ws);
    const int64_t n = (int64_t)B * C * H * W;
    nf_ws r;
    r.plane_nan = reinterpret_cast<int32_t*>(p);
    p += nf_align((int64_t)B * C * 4);
    r.col = reinterpret_cast<int32_t*>(p);
    p += nf_align(n * 4);
    r.stack = reinterpret_cast<int2*>(p);
    return r;
}

}  // namespace

extern "C" int64_t pc_nan_fill_ws_bytes(int B, int C, int H, int W) {
    if (B < 0 || C < 0 || H < 0 || W < 0) return 0;
    const int64_t n = (int64_t)B * C * H * W;
    return nf_align((int64_t)B * C * 4) + nf_align(n * 4) + nf_align(n * 8);
}

extern "C" int pc_nan_fill(float* x, const int32_t* hw, int64_t* counts, void* ws, int B, int C, int H, int W, int flags,
                           void* stream) {
    if (!x || !counts || !ws || B < 1 || C < 1 || C > PC_NAN_FILL_MAX_C || H < 1 || W < 1 || H > PC_NAN_FILL_MAX_HW ||
        W > PC_NAN_FILL_MAX_HW || B * C > 65535 || (flags & ~PC_NAN_FILL_COUNT_ONLY))
        return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const nf_ws s = nf_carve(ws, B, C, H, W);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * B, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(s.plane_nan, 0, sizeof(int32_t) * B * C, st);
    if (e != hipSuccess) return (int)e;
    const int vec4 = (W % 4 == 0) && ((reinterpret_cast<uintptr_t>(x) & 15) == 0);
    hipLaunchKernelGGL(nan_count_kernel, dim3((H + NF_COUNT_ROWS - 1) / NF_COUNT_ROWS, B * C), dim3(NF_THREADS), 0, st, x, hw, cnt,
                       s.plane_nan, C, H, W, vec4);
    PC_CHECK_LAUNCH();
    if (flags & PC_NAN_FILL_COUNT_ONLY) return 0;
    hipLaunchKernelGGL(nan_fill_rows_kernel, dim3(H, B * C), dim3(NF_THREADS), 0, st, x, hw, cnt, s.plane_nan, s.col, C, H, W);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(nan_fill_cols_kernel, dim3((W + NF_THREADS - 1) / NF_THREADS, B * C), dim3(NF_THREADS), 0, st, hw, cnt,
                       s.plane_nan, s.col, s.stack, C, H, W);
    PC_CHECK_LAUNCH();
    const int64_t px = (int64_t)H * W;
    const int64_t g = (px + NF_THREADS - 1) / NF_THREADS;
    const int gx = (int)(g < 2048 ? g : 2048);
    if (C <= 2)
        hipLaunchKernelGGL(nan_fill_combine_kernel<2>, dim3(gx, B), dim3(NF_THREADS), 0, st, x, hw, cnt, s.col, C, H, W);
    else if (C <= 4)
        hipLaunchKernelGGL(nan_fill_combine_kernel<4>, dim3(gx, B), dim3(NF_THREADS), 0, st, x, hw, cnt, s.col, C, H, W);
    else
        hipLaunchKernelGGL(nan_fill_combine_kernel<8>, dim3(gx, B), dim3(NF_THREADS), 0, st, x, hw, cnt, s.col, C, H, W);
    PC_CHECK_LAUNCH();
    return 0;
}
