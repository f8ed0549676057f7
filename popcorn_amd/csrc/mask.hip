// mask.hip -- the per-pixel kernels between the U-Net and the occupancy head: building score, sparsity mask, masked compaction.
//
// Replaces (reference model/popcorn.py):
//   :155,271-276    revert_padding (crop)                                          -> crop offsets in the loader
//   :301,317-320    fusion_out_conv + sigmoid + crop (building score)
//   :361-377        get_sparsity_mask (:374-375 the empty-selection fallback)
//   :336-359        get_sparsity_mask(sparse_unet=True)
//   :173            boolean-index gather and its autograd (ordered compaction / scatter)
//
// Also the zero fills that the train step runs as kernels (pc_zero_fill; see zero_fill_kernel for why not memset nodes).
#include "common.h"

namespace {

// ---- fusion_out_conv (1x1, 16->1) + sigmoid + crop ------------------------------------------------------------
__global__ __launch_bounds__(256) void outconv_sigmoid_crop_kernel(pc_src feat, const float* w, const float* bias,
                                                                   pc_dst out, int B, int H, int W, int py, int px, int bf) {
    const int64_t n = (int64_t)B * H * W;
    float wv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {      // C = 16 (fusion_out_conv) or 8 (sar/optical_out_conv); bf16 mode: operand rounding
        const float t = c < feat.C ? w[c] : 0.f;
        wv[c] = bf ? pc_bf16r(t) : t;
    }
    const float bv = bias[0];
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / (unsigned)W;
        const int x = (int)(i - row * (unsigned)W), y = (int)(row % (unsigned)H), b = (int)(row / (unsigned)H);
        const int64_t fo = b * feat.bstride + (int64_t)(py + y) * feat.rstride + (int64_t)(px + x) * pc_xs(feat);
        float s = bv;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < feat.C) s = fmaf(pc_src_at(feat, fo + c * feat.cstride), wv[c], s);
        out.ptr[b * out.bstride + (int64_t)y * out.rstride + x] = 1.f / (1.f + expf(-s));
    }
}

// ---- sparsity mask ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sparsity_mask_kernel(const float* building, const float* admin, const int64_t* census,
                                                            const uint8_t* rowsel, const uint8_t* colsel, int occ,
                                                            uint8_t* mask, int32_t* counts, int B, int H, int W) {
    const int64_t n = (int64_t)B * H * W;
    int nsel = 0, nreg = 0;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / (unsigned)W;
        const int x = (int)(i - row * (unsigned)W), y = (int)(row % (unsigned)H), b = (int)(row / (unsigned)H);
        const bool region = admin[i] == (float)census[b];
        // popcorn.py:365-372: ((building>0)*region | grid) & region  [occupancymodel]   /   region | grid) & region
        const bool base = occ ? (building[i] > 0.f) : true;
        const bool m = region && (base || (rowsel[y] && colsel[x]));
        mask[i] = m ? 1 : 0;
        nsel += m;
        nreg += region;
    }
    // integer counts: order-independent, atomics are exact.  One atomic pair per BLOCK (a per-wave atomic on two words
    // serialised 16 k atomics: 188 us for a 640 k-pixel batch, profiles/r1_v0).
    __shared__ int red[2][4];
    for (int off = 32; off > 0; off >>= 1) { nsel += __shfl_down(nsel, off); nreg += __shfl_down(nreg, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = nsel; red[1][threadIdx.x >> 6] = nreg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = red[0][0] + red[0][1] + red[0][2] + red[0][3], b2 = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (a) atomicAdd(&counts[0], a);
        if (b2) atomicAdd(&counts[1], b2);
    }
}

// popcorn.py:374-375: an empty selection falls back to the region mask
__global__ __launch_bounds__(256) void sparsity_mask_fallback_kernel(const float* admin, const int64_t* census, uint8_t* mask,
                                                                     int32_t* counts, int B, int H, int W) {
    if (counts[0] != 0) return;
    const int64_t n = (int64_t)B * H * W;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
        const int b = (int)(i / (unsigned)(W * H));
        mask[i] = admin[i] == (float)census[b] ? 1 : 0;
    }
}

__global__ void sparsity_mask_fix_count_kernel(int32_t* counts) {
    if (counts[0] == 0) counts[0] = counts[1];
}

// ---- building score + sparsity mask in ONE launch -----------------------------------------------------------------
// outconv_sigmoid_crop_kernel + sparsity_mask_kernel + the empty-selection fallback + the count fix-up (a memset and four
// dependent launches, ~38 us between the U-Net forward and the head) as one kernel: every block accumulates {nsel, nregion}
// into a scratch pair and takes a ticket; the block that draws the last ticket publishes the counts, applies the
// fallback of popcorn.py:374-375 if the whole batch selected nothing (rare; done by that one block).  The accumulators live
// in a library-owned scratch that a one-wave kernel zeroes in front of every launch.
// Zero fills inside the train step are kernels, not hipMemsetAsync: memset nodes captured into the step's HIP graph were
// not reliably re-executed / ordered on replay once the node sequence of the graph changed (a 16- or 32-byte one never
// replayed; with it gone the 67 MB one of the head backward went wrong too: garbage gradients from the second replay on,
// eager launches always correct).
__global__ __launch_bounds__(256) void zero_fill_kernel(float* p, int64_t n4, int64_t rem) {
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) reinterpret_cast<f32x4*>(p)[i] = z;
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < rem) p[4 * n4 + threadIdx.x] = 0.f;
}

__global__ void zero_words_kernel(uint32_t* p, int n) {
    if ((int)threadIdx.x < n) p[threadIdx.x] = 0u;
}

struct ScoreMaskArgs {
    pc_src feat; const float* w; const float* bias; pc_dst out;      // 1x1 conv + sigmoid + crop (as outconv_sigmoid_crop)
    const float* admin; const int64_t* census; const uint8_t* rowsel; const uint8_t* colsel;
    int occ; uint8_t* mask; int32_t* counts; unsigned* scratch;      // scratch: one packed 64-bit accumulator {nsel, nregion, ticket} (see the kernel), zero between launches
    int B, H, W, py, px;
    int bf;
};

constexpr int SM_THREADS = 1024;       // 16 waves per block, at most one block per CU: B = 64 tiles (160 k four-pixel items) in ONE round of loads
__global__ __launch_bounds__(SM_THREADS) void score_mask_kernel(const ScoreMaskArgs a) {
    const int64_t n = (int64_t)a.B * a.H * a.W;
    float wv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const float t = c < a.feat.C ? a.w[c] : 0.f;
        wv[c] = a.bf ? pc_bf16r(t) : t;
    }
    const float bv = a.bias[0];
    int nsel = 0, nreg = 0;
    const bool vec4 = a.feat.dtype == PC_F32 && pc_planar(a.feat) &&      // (a bf16 feature map -- the non-dot fallback of bf16 mode -- takes the scalar loop)
                      (a.W & 3) == 0 && (a.out.rstride & 3) == 0 && (a.out.bstride & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(a.out.ptr) | reinterpret_cast<uintptr_t>(a.admin) |
                        reinterpret_cast<uintptr_t>(a.mask)) & 15) == 0;
    if (vec4) {
        // four consecutive pixels of a row per thread: 16-byte accesses (the feature read is 4-byte aligned only: the crop
        // offset px is arbitrary), a quarter of the dependent iterations of the scalar loop
        const unsigned n4 = (unsigned)(n >> 2), w4 = (unsigned)a.W >> 2;
        for (unsigned i4 = blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += gridDim.x * blockDim.x) {
            const unsigned row = i4 / w4;
            const int x = (int)(i4 - row * w4) * 4, y = (int)(row % (unsigned)a.H), b = (int)(row / (unsigned)a.H);
            const float* fp = a.feat.ptr + b * a.feat.bstride + (int64_t)(a.py + y) * a.feat.rstride + a.px + x;
            f32x4 s = f32x4{bv, bv, bv, bv};
#pragma unroll
            for (int c = 0; c < 16; ++c)
                if (c < a.feat.C) {
                    const f32x4u f = *reinterpret_cast<const f32x4u*>(fp + c * a.feat.cstride);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] = fmaf(f[e], wv[c], s[e]);
                }
            const f32x4 adm = *reinterpret_cast<const f32x4*>(a.admin + 4 * (int64_t)i4);
            const float cid = (float)a.census[b];
            const bool rs = a.rowsel[y] != 0;
            f32x4 bld;
            unsigned mbits = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bld[e] = 1.f / (1.f + expf(-s[e]));
                const bool region = adm[e] == cid;
                const bool base = a.occ ? (bld[e] > 0.f) : true;
                const bool m = region && (base || (rs && a.colsel[x + e]));
                mbits |= (m ? 1u : 0u) << (8 * e);
                nsel += m;
                nreg += region;
            }
            *reinterpret_cast<f32x4*>(a.out.ptr + b * a.out.bstride + (int64_t)y * a.out.rstride + x) = bld;
            *reinterpret_cast<unsigned*>(a.mask + 4 * (int64_t)i4) = mbits;
        }
    } else
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
        const unsigned row = i / (unsigned)a.W;
        const int x = (int)(i - row * (unsigned)a.W), y = (int)(row % (unsigned)a.H), b = (int)(row / (unsigned)a.H);
        const int64_t fo = b * a.feat.bstride + (int64_t)(a.py + y) * a.feat.rstride + (int64_t)(a.px + x) * pc_xs(a.feat);
        float s = bv;
#pragma unroll
        for (int c = 0; c < 16; ++c)
            if (c < a.feat.C) s = fmaf(pc_src_at(a.feat, fo + c * a.feat.cstride), wv[c], s);
        const float building = 1.f / (1.f + expf(-s));
        a.out.ptr[b * a.out.bstride + (int64_t)y * a.out.rstride + x] = building;
        const bool region = a.admin[i] == (float)a.census[b];
        const bool base = a.occ ? (building > 0.f) : true;
        const bool m = region && (base || (a.rowsel[y] && a.colsel[x]));
        a.mask[i] = m ? 1 : 0;
        nsel += m;
        nreg += region;
    }
    __shared__ int red[2][SM_THREADS / 64];
    __shared__ unsigned last;
    for (int off = 32; off > 0; off >>= 1) { nsel += __shfl_down(nsel, off); nreg += __shfl_down(nreg, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = nsel; red[1][threadIdx.x >> 6] = nreg; }
    __syncthreads();
    __shared__ unsigned long long tot_sh;
    if (threadIdx.x == 0) {
        int s0 = 0, s1 = 0;
#pragma unroll
        for (int w = 0; w < SM_THREADS / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
        // integer counts: order-independent, exact.  ONE 64-bit atomic per block carries {nsel : 27 | nregion : 27 | ticket : 10}
        // (device-scope atomics on one address retire at ~13 ns each, and every dependent one is a round trip to the memory side:
        // counts, ticket and the last block's read of the totals were three of them); the block that draws the last ticket has the
        // totals in the returned value
        __threadfence();
        const unsigned long long add = (unsigned long long)(unsigned)s0 | ((unsigned long long)(unsigned)s1 << 27) | (1ull << 54);
        const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long*>(a.scratch), add);
        last = (unsigned)(old >> 54) == gridDim.x - 1 ? 1u : 0u;
        tot_sh = old + add;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    const unsigned tot_sel = (unsigned)(tot_sh & ((1ull << 27) - 1)), tot_reg = (unsigned)((tot_sh >> 27) & ((1ull << 27) - 1));
    if (tot_sel == 0) {
        // an empty selection falls back to the region mask (popcorn.py:374-375)
        for (unsigned i = threadIdx.x; i < (unsigned)n; i += blockDim.x) {
            const int b = (int)(i / (unsigned)(a.W * a.H));
            a.mask[i] = a.admin[i] == (float)a.census[b] ? 1 : 0;
        }
    }
    if (threadIdx.x == 0) {
        a.counts[0] = (int32_t)(tot_sel ? tot_sel : tot_reg);
        a.counts[1] = (int32_t)tot_reg;
        // this block is the last one alive: leave the accumulator and the ticket at zero for the next call (which is ordered
        // behind this kernel on the stream), instead of a zeroing launch in front of every call
        a.scratch[0] = 0u; a.scratch[1] = 0u;
        __threadfence();
    }
}

// ---- ordered compaction: out[rank(i)] = src[i] for mask[i] != 0 (row-major order) --------------------------------
constexpr int CBLK = 1024;   // elements per block

__global__ __launch_bounds__(256) void compact_count_kernel(const uint8_t* mask, int32_t* block_counts, int64_t n) {
    __shared__ int red[4];
    const int64_t base = (int64_t)blockIdx.x * CBLK;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        c += (i < n && mask[i]) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// single block exclusive scan of block_counts (nblocks <= a few thousand)
__global__ __launch_bounds__(1024) void compact_scan_kernel(int32_t* block_counts, int nblocks, int32_t* n_out) {
    __shared__ int sh[1024];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = i < nblocks ? block_counts[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int t = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblocks) block_counts[i] = carry + sh[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = carry;
}

__global__ __launch_bounds__(256) void compact_write_kernel(const float* src, const uint8_t* mask, const int32_t* block_off,
                                                            float* out, int64_t n) {
    __shared__ int wave_tot[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * CBLK;
    // element order inside a block: k-major (k*256 + tid) keeps the global order row-major
    bool m[4];
    unsigned long long bal[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        m[k] = i < n && mask[i];
        bal[k] = __ballot(m[k]);
        if (lane == 0) wave_tot[k][wave] = __popcll(bal[k]);
    }
    __syncthreads();
    int off = block_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int pre = 0;
        for (int w = 0; w < wave; ++w) pre += wave_tot[k][w];
        if (m[k]) {
            const int rank = __popcll(bal[k] & ((1ull << lane) - 1ull));
            out[off + pre + rank] = src[base + k * 256 + threadIdx.x];
        }
        off += wave_tot[k][0] + wave_tot[k][1] + wave_tot[k][2] + wave_tot[k][3];
    }
}

// inverse of compact_write_kernel: out[i] = mask[i] ? src[rank(i)] : 0  (autograd of the boolean-index gather, popcorn.py:173)
__global__ __launch_bounds__(256) void scatter_masked_kernel(const float* src, const uint8_t* mask, const int32_t* block_off,
                                                             float* out, int64_t n) {
    __shared__ int wave_tot[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * CBLK;
    bool m[4];
    unsigned long long bal[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        m[k] = i < n && mask[i];
        bal[k] = __ballot(m[k]);
        if (lane == 0) wave_tot[k][wave] = __popcll(bal[k]);
    }
    __syncthreads();
    int off = block_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int pre = 0;
        for (int w = 0; w < wave; ++w) pre += wave_tot[k][w];
        const int64_t i = base + k * 256 + threadIdx.x;
        if (i < n) out[i] = m[k] ? src[off + pre + __popcll(bal[k] & ((1ull << lane) - 1ull))] : 0.f;
        off += wave_tot[k][0] + wave_tot[k][1] + wave_tot[k][2] + wave_tot[k][3];
    }
}

// get_sparsity_mask(sparse_unet=True), popcorn.py:336-359: one workgroup per sample.
//   bmask = building > thresh;  mask = (bmask | grid) & region;  ratio = #(region & ~bmask) / (#(grid & region & ~bmask) + 1e-5)
__global__ __launch_bounds__(256) void sparsity_mask_unet_kernel(const float* building, const float* admin, const int64_t* census,
                                                                 const uint8_t* rowsel, const uint8_t* colsel, float thresh,
                                                                 uint8_t* mask, float* ratio, int H, int W) {
    __shared__ int red[2][256];
    const int b = blockIdx.x;
    const float cid = (float)census[b];
    const int64_t base = (int64_t)b * H * W;
    int n_empty = 0, n_sub = 0;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        const bool region = admin[base + i] == cid;
        const bool bm = building[base + i] > thresh;
        const bool grid = rowsel[y] && colsel[x];
        mask[base + i] = (uint8_t)((bm || grid) && region);
        n_empty += (region && !bm) ? 1 : 0;
        n_sub += (grid && region && !bm) ? 1 : 0;
    }
    red[0][threadIdx.x] = n_empty;
    red[1][threadIdx.x] = n_sub;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { red[0][threadIdx.x] += red[0][threadIdx.x + off]; red[1][threadIdx.x] += red[1][threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) ratio[b] = (float)red[0][0] / ((float)red[1][0] + 1e-5f);
}

}  // namespace

// zero fill by a kernel (not a memset node: see zero_fill_kernel); p 16-byte aligned
extern "C" int pc_zero_fill(float* p, int64_t n, void* stream) {
    if (!p || n < 0 || (reinterpret_cast<uintptr_t>(p) & 15)) return PC_EINVAL;
    if (n == 0) return 0;
    const int64_t n4 = n / 4, rem = n - 4 * n4;
    int grid = (int)((n4 + 255) / 256);
    grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);
    hipLaunchKernelGGL(zero_fill_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, n4, rem);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_sparsity_mask_unet(const float* building, const float* admin_mask, const int64_t* census_idx,
                                     const uint8_t* rowsel, const uint8_t* colsel, float threshold, uint8_t* mask, float* ratio,
                                     int B, int H, int W, void* stream) {
    if (!building || !admin_mask || !census_idx || !rowsel || !colsel || !mask || !ratio || B < 1) return PC_EINVAL;
    hipLaunchKernelGGL(sparsity_mask_unet_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, building, admin_mask, census_idx,
                       rowsel, colsel, threshold, mask, ratio, H, W);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_scatter_masked(const float* src, const uint8_t* mask, float* out, void* ws, int64_t n, void* stream) {
    if (!src || !mask || !out || !ws) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nblocks = (int)((n + CBLK - 1) / CBLK);
    if (nblocks == 0) return 0;
    int32_t* bc = reinterpret_cast<int32_t*>(ws);
    hipLaunchKernelGGL(compact_count_kernel, dim3(nblocks), dim3(256), 0, st, mask, bc, n);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, st, bc, nblocks, bc + nblocks);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(scatter_masked_kernel, dim3(nblocks), dim3(256), 0, st, src, mask, bc, out, n);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_outconv_sigmoid_crop(const pc_src* feat, const float* w, const float* bias, const pc_dst* out,
                                       int B, int H, int W, int py, int px, void* stream) {
    if (!feat || !w || !bias || !out || feat->C < 1 || feat->C > 16) return PC_EINVAL;
    const int64_t n = (int64_t)B * H * W;
    int grid = (int)((n + 255) / 256);
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(outconv_sigmoid_crop_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *feat, w, bias, *out,
                       B, H, W, py, px, (int)(g_pc_precision == PC_PREC_BF16));
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_building_score_mask(const pc_src* feat, const float* w, const float* bias, const pc_dst* building_out,
                                      const float* admin_mask, const int64_t* census_idx, const uint8_t* rowsel,
                                      const uint8_t* colsel, int occupancymodel, uint8_t* mask, int32_t* counts,
                                      int B, int H, int W, int py, int px, void* stream) {
    if (!feat || !w || !bias || !building_out || !admin_mask || !census_idx || !rowsel || !colsel || !mask || !counts ||
        feat->C < 1 || feat->C > 16)
        return PC_EINVAL;
    if ((int64_t)B * H * W >= ((int64_t)1 << 27)) return PC_EINVAL;      // the packed 64-bit accumulator holds two 27-bit counts
    static unsigned* scratch = nullptr;     // one 64-bit word {nsel : 27 | nregion : 27 | ticket : 10}: device-scope atomics only; zero
                                            // between calls (the kernel's last block resets it), zeroed once here
    if (!scratch) {
        hipError_t e = hipMalloc(&scratch, 4 * sizeof(unsigned));
        if (e != hipSuccess) return (int)e;
        e = hipMemset(scratch, 0, 4 * sizeof(unsigned));
        if (e != hipSuccess) return (int)e;
        e = hipDeviceSynchronize();            // the first kernel may run on a non-blocking stream
        if (e != hipSuccess) return (int)e;
    }
    ScoreMaskArgs a{};
    a.feat = *feat; a.w = w; a.bias = bias; a.out = *building_out; a.admin = admin_mask; a.census = census_idx;
    a.rowsel = rowsel; a.colsel = colsel; a.occ = occupancymodel; a.mask = mask; a.counts = counts; a.scratch = scratch;
    a.B = B; a.H = H; a.W = W; a.py = py; a.px = px; a.bf = g_pc_precision == PC_PREC_BF16;
    const int64_t n = (int64_t)B * H * W;
    int grid = (int)((n + SM_THREADS - 1) / SM_THREADS);
    if (grid > 256) grid = 256;            // one block per CU: the per-block atomics are the serial part
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(score_mask_kernel, dim3(grid), dim3(SM_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_sparsity_mask(const float* building, const float* admin_mask, const int64_t* census_idx,
                                const uint8_t* rowsel, const uint8_t* colsel, int occupancymodel,
                                uint8_t* mask, int32_t* counts, int B, int H, int W, void* stream) {
    if (!building || !admin_mask || !census_idx || !rowsel || !colsel || !mask || !counts) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<uint32_t*>(counts), 2);
    PC_CHECK_LAUNCH();
    const int64_t n = (int64_t)B * H * W;
    int grid = (int)((n + 255) / 256);
    if (grid > 512) grid = 512;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(sparsity_mask_kernel, dim3(grid), dim3(256), 0, st, building, admin_mask, census_idx, rowsel, colsel,
                       occupancymodel, mask, counts, B, H, W);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(sparsity_mask_fallback_kernel, dim3(grid), dim3(256), 0, st, admin_mask, census_idx, mask, counts, B, H, W);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(sparsity_mask_fix_count_kernel, dim3(1), dim3(1), 0, st, counts);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t pc_compact_ws_bytes(int64_t n) { return ((n + CBLK - 1) / CBLK + 1) * (int64_t)sizeof(int32_t); }

extern "C" int pc_compact_masked(const float* src, const uint8_t* mask, float* out, int32_t* n_out, void* ws, int64_t n,
                                 void* stream) {
    if (!src || !mask || !out || !n_out || !ws) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nblocks = (int)((n + CBLK - 1) / CBLK);
    int32_t* bc = reinterpret_cast<int32_t*>(ws);
    if (nblocks == 0) {           // (a kernel, not a memset node: see zero_fill_kernel)
        hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<uint32_t*>(n_out), 1);
        PC_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(compact_count_kernel, dim3(nblocks), dim3(256), 0, st, mask, bc, n);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, st, bc, nblocks, n_out);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_write_kernel, dim3(nblocks), dim3(256), 0, st, src, mask, bc, out, n);
    PC_CHECK_LAUNCH();
    return 0;
}
