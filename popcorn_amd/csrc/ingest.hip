// ingest.hip -- input ingest: band selection, normalisation and reflect padding of the Sentinel-1 / -2 tiles in one pass.
//
// Replaces (reference):
//   model/popcorn.py:231-258    add_padding (F.pad, mode="reflect")
//   utils/utils.py:105-127      apply_normalize, with the band selection in front of it
#include "common.h"

namespace {

// F.pad(x, (left, right, top, bottom), mode="reflect") for NCHW planes (add_padding, popcorn.py:231-258)
__global__ __launch_bounds__(256) void reflect_pad_kernel(const float* in, float* out, int64_t planes, int H, int W, int Hp, int Wp,
                                                          int top, int left) {
    const int64_t n = planes * Hp * Wp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int x = (int)(i % Wp), y = (int)((i / Wp) % Hp);
        const int64_t pl = i / ((int64_t)Wp * Hp);
        out[i] = in[(pl * H + pc_reflect(y - top, H)) * W + pc_reflect(x - left, W)];
    }
}

// the same with a channel gather: out[b][j] = pad(in[b][sel[j]]); one thread = 4 consecutive x of one output row
// NORM: also (x - mean[j]) / std[j] per output plane -- band selection + apply_normalize (utils/utils.py:105-127) + add_padding in
// ONE pass over the raw tile (pc_select_normalize_pad); the division is the one pc_select_normalize performs (same bits)
struct PadSel { int sel[8]; float mean[8]; float stdv[8]; };
template <bool NORM>
__global__ __launch_bounds__(256) void reflect_pad_select_kernel(const float* in, float* out, PadSel ps, int Cin, int nsel, int H, int W,
                                                                 int Hp, int Wp, int top, int left, int nrows, int wq, int rows_per_block) {
    // a block = rows_per_block output rows x wq 4-pixel pieces (wq * rows_per_block <= 256)
    const int tr = threadIdx.x / wq, piece = threadIdx.x - tr * wq;
    const int row = blockIdx.x * rows_per_block + tr;
    if (tr >= rows_per_block || row >= nrows) return;
    const int pl = row / Hp, y = row - pl * Hp;             // pl = b * nsel + j
    const int b = pl / nsel, j = pl - b * nsel;
    const float* src = in + ((int64_t)(b * Cin + ps.sel[j]) * H + pc_reflect(y - top, H)) * W;
    float* dst = out + (int64_t)row * Wp + 4 * piece;
    const int x0 = 4 * piece, xs = x0 - left;
    f32x4 v;
    if (xs >= 0 && xs + 3 < W) {
        if (((xs | W) & 1) == 0) {
            // even pad and even width (14 / 100 for the training tiles): the piece is 8-byte aligned -- two 8-byte loads (the
            // 4-byte-aligned vector type below is split into four dword loads by the compiler)
            const f32x2 t0 = *reinterpret_cast<const f32x2*>(src + xs), t1 = *reinterpret_cast<const f32x2*>(src + xs + 2);
            v = f32x4{t0[0], t0[1], t1[0], t1[1]};
        } else {
            const f32x4u t = *reinterpret_cast<const f32x4u*>(src + xs);   // interior: one (unaligned) 16-byte load
            v = f32x4{t[0], t[1], t[2], t[3]};
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x0 + e < Wp ? src[pc_reflect(xs + e, W)] : 0.f;
    }
    if (NORM) {
        const float mu = ps.mean[j], sd = ps.stdv[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] - mu) / sd;
    }
    if ((Wp & 3) == 0) {
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x0 + e < Wp) dst[e] = v[e];
    }
}

// PC_PREC_BF16 ingest (pc_ingest_cl8): one thread = one pixel of the padded domain = ONE aligned 16-byte channels-last slot:
// band select + normalise + reflect padding + stream order + round to bf16; channel slots >= nsel are zero
template <bool NORM>
__global__ __launch_bounds__(256) void ingest_cl8_kernel(const float* __restrict__ in, uint4* __restrict__ out, PadSel ps, int Cin, int nsel,
                                                         int H, int W, int Hp, int Wp, int top, int left, int npix) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int x = i % Wp, r = i / Wp;
    const int y = r % Hp, b = r / Hp;
    const int64_t o = (int64_t)pc_reflect(y - top, H) * W + pc_reflect(x - left, W);
    const int64_t plane = (int64_t)H * W;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = 0.f;
        if (j < nsel) {
            t = in[((int64_t)b * Cin + ps.sel[j]) * plane + o];
            if (NORM) t = (t - ps.mean[j]) / ps.stdv[j];
        }
        v[j] = t;
    }
    out[i] = make_uint4(pc_pack_bf16(v[0], v[1]), pc_pack_bf16(v[2], v[3]), pc_pack_bf16(v[4], v[5]), pc_pack_bf16(v[6], v[7]));
}

// the same ingest from the two tensors a loader ships (pc_ingest_split): S2 reflectances as UINT16 digital numbers (planar, C2 bands) and
// S1 backscatter as fp32 (planar, C1 bands); channel index sel[j] < C2 -> s2, else s1[sel[j] - C2].  One thread = one pixel of the padded
// domain, all nsel channels: the planar fp32 form writes nsel coalesced words, the channels-last bf16 form one 16-byte slot.
template <bool CL8>
__global__ __launch_bounds__(256) void ingest_split_kernel(const uint16_t* __restrict__ s2, const float* __restrict__ s1, void* __restrict__ out, PadSel ps,
                                                           int C2, int C1, int nsel, int H, int W, int Hp, int Wp, int top, int left, int npix) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int x = i % Wp, r = i / Wp;
    const int y = r % Hp, b = r / Hp;
    const int64_t o = (int64_t)pc_reflect(y - top, H) * W + pc_reflect(x - left, W);
    const int64_t plane = (int64_t)H * W;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = 0.f;
        if (j < nsel) {
            const int c = ps.sel[j];
            t = c < C2 ? (float)s2[((int64_t)b * C2 + c) * plane + o] : s1[((int64_t)b * C1 + (c - C2)) * plane + o];
            t = (t - ps.mean[j]) / ps.stdv[j];
        }
        v[j] = t;
    }
    if (CL8) {
        reinterpret_cast<uint4*>(out)[i] = make_uint4(pc_pack_bf16(v[0], v[1]), pc_pack_bf16(v[2], v[3]), pc_pack_bf16(v[4], v[5]), pc_pack_bf16(v[6], v[7]));
    } else {
        float* op = reinterpret_cast<float*>(out) + (int64_t)b * nsel * Hp * Wp + (int64_t)y * Wp + x;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < nsel) op[(int64_t)j * Hp * Wp] = v[j];
    }
}


// pc_ingest_pad_strided: the three ingests above for rows of ANY width and an output whose rows are `rs` >= Wp floats apart (the native
// step executor's arena pads rows to 16 bytes): one thread = one 16-byte piece of an output row.  KIND 0: planar fp32 source (model input or
// raw tile), 2: uint16 S2 + fp32 S1 (channel index sel < C2 -> s2).  Same arithmetic as the kernels above ((x - mean) / std), so the same bits.
template <int KIND, bool NORM>
__global__ __launch_bounds__(256) void ingest_pad_strided_kernel(const void* __restrict__ data, const void* __restrict__ data2, float* __restrict__ out, PadSel ps,
                                                                 int Cin, int C2, int nsel, int H, int W, int Hp, int Wp, int rs, int top, int left,
                                                                 int64_t npieces, int wq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npieces) return;
    const int64_t row = i / wq;
    const int piece = (int)(i - row * wq);
    const int pl = (int)(row / Hp), y = (int)(row - (int64_t)pl * Hp);
    const int b = pl / nsel, j = pl - b * nsel;
    const int ys = pc_reflect(y - top, H);
    const int x0 = 4 * piece, xs = x0 - left;
    const int c = ps.sel[j];
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (KIND == 2 && c < C2) {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(data) + ((int64_t)(b * C2 + c) * H + ys) * W;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (x0 + e < Wp) v[e] = (float)src[pc_reflect(xs + e, W)];
    } else {
        const float* src = KIND == 2 ? reinterpret_cast<const float*>(data2) + ((int64_t)(b * (Cin - C2) + (c - C2)) * H + ys) * W
                                     : reinterpret_cast<const float*>(data) + ((int64_t)(b * Cin + c) * H + ys) * W;
        if (xs >= 0 && xs + 3 < W) {
            const f32x4u t = *reinterpret_cast<const f32x4u*>(src + xs);
            v = f32x4{t[0], t[1], t[2], t[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e < Wp) v[e] = src[pc_reflect(xs + e, W)];
        }
    }
    if (NORM) {
        const float mu = ps.mean[j], sd = ps.stdv[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = x0 + e < Wp ? (v[e] - mu) / sd : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + ((int64_t)pl * Hp + y) * rs + x0) = v;      // (rs % 4 == 0: the pad columns of the row get zeros)
}

}  // namespace

static int launch_pad_select(const float* in, float* out, int B, int Cin, int nsel, const int* sel, const float* mean, const float* stdv,
                             int H, int W, int top, int bottom, int left, int right, void* stream) {
    if (!in || !out || !sel || B < 1 || nsel < 1 || nsel > 8 || top >= H || bottom >= H || left >= W || right >= W || top < 0 ||
        bottom < 0 || left < 0 || right < 0)
        return PC_EINVAL;
    PadSel ps{};
    for (int j = 0; j < nsel; ++j) {
        if (sel[j] < 0 || sel[j] >= Cin) return PC_EINVAL;
        ps.sel[j] = sel[j];
        ps.mean[j] = mean ? mean[j] : 0.f;
        ps.stdv[j] = stdv ? stdv[j] : 1.f;
    }
    const int Hp = H + top + bottom, Wp = W + left + right;
    const int64_t nrows = (int64_t)B * nsel * Hp;
    const int wq = (Wp + 3) >> 2;
    if (wq > 256 || nrows > 0x7fffffff) return PC_EINVAL;          // rows of up to 1024 pixels (the training tiles; windows are not padded)
    const int rpb = 256 / wq;
    const dim3 grid((unsigned)((nrows + rpb - 1) / rpb));
    if (mean)
        hipLaunchKernelGGL(reflect_pad_select_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, out, ps, Cin, nsel, H, W, Hp, Wp,
                           top, left, (int)nrows, wq, rpb);
    else
        hipLaunchKernelGGL(reflect_pad_select_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, out, ps, Cin, nsel, H, W, Hp, Wp,
                           top, left, (int)nrows, wq, rpb);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_reflect_pad_select(const float* in, float* out, int B, int Cin, int nsel, const int* sel, int H, int W, int top,
                                     int bottom, int left, int right, void* stream) {
    return launch_pad_select(in, out, B, Cin, nsel, sel, nullptr, nullptr, H, W, top, bottom, left, right, stream);
}

extern "C" int pc_select_normalize_pad(const float* raw, float* out, int B, int Craw, int nsel, const int* band, const float* mean,
                                       const float* stdv, int H, int W, int top, int bottom, int left, int right, void* stream) {
    if (!mean || !stdv) return PC_EINVAL;
    return launch_pad_select(raw, out, B, Craw, nsel, band, mean, stdv, H, W, top, bottom, left, right, stream);
}

extern "C" int pc_ingest_cl8(const float* raw, void* out, int B, int Craw, int nsel, const int* band, const float* mean, const float* stdv,
                             int H, int W, int top, int bottom, int left, int right, void* stream) {
    if (!raw || !out || !band || B < 1 || nsel < 1 || nsel > 8 || top >= H || bottom >= H || left >= W || right >= W || top < 0 ||
        bottom < 0 || left < 0 || right < 0 || (mean == nullptr) != (stdv == nullptr) || (reinterpret_cast<uintptr_t>(out) & 15))
        return PC_EINVAL;
    PadSel ps{};
    for (int j = 0; j < nsel; ++j) {
        if (band[j] < 0 || band[j] >= Craw) return PC_EINVAL;
        ps.sel[j] = band[j];
        ps.mean[j] = mean ? mean[j] : 0.f;
        ps.stdv[j] = stdv ? stdv[j] : 1.f;
    }
    const int Hp = H + top + bottom, Wp = W + left + right;
    const int64_t npix = (int64_t)B * Hp * Wp;
    if (npix > 0x7fffffff) return PC_EINVAL;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (mean)
        hipLaunchKernelGGL(ingest_cl8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, raw, reinterpret_cast<uint4*>(out), ps, Craw, nsel,
                           H, W, Hp, Wp, top, left, (int)npix);
    else
        hipLaunchKernelGGL(ingest_cl8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, raw, reinterpret_cast<uint4*>(out), ps, Craw, nsel,
                           H, W, Hp, Wp, top, left, (int)npix);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_ingest_split(const uint16_t* s2, int C2, const float* s1, int C1, void* out, int cl8, int B, int nsel, const int* band,
                               const float* mean, const float* stdv, int H, int W, int top, int bottom, int left, int right, void* stream) {
    if (!s2 || !s1 || !out || !band || !mean || !stdv || B < 1 || C2 < 1 || C1 < 1 || nsel < 1 || nsel > 8 || top >= H || bottom >= H ||
        left >= W || right >= W || top < 0 || bottom < 0 || left < 0 || right < 0 || (reinterpret_cast<uintptr_t>(out) & 15))
        return PC_EINVAL;
    PadSel ps{};
    for (int j = 0; j < nsel; ++j) {
        if (band[j] < 0 || band[j] >= C2 + C1) return PC_EINVAL;
        ps.sel[j] = band[j];
        ps.mean[j] = mean[j];
        ps.stdv[j] = stdv[j];
    }
    const int Hp = H + top + bottom, Wp = W + left + right;
    const int64_t npix = (int64_t)B * Hp * Wp;
    if (npix > 0x7fffffff) return PC_EINVAL;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (cl8)
        hipLaunchKernelGGL(ingest_split_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, s2, s1, out, ps, C2, C1, nsel, H, W, Hp, Wp, top,
                           left, (int)npix);
    else
        hipLaunchKernelGGL(ingest_split_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, s2, s1, out, ps, C2, C1, nsel, H, W, Hp, Wp, top,
                           left, (int)npix);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_ingest_pad_strided(int kind, const void* data, const void* data2, int Cin, float* out, int out_rstride, int B, int nsel,
                                     const int* sel, const float* mean, const float* stdv, int H, int W, int top, int bottom, int left, int right,
                                     void* stream) {
    if (!data || !out || !sel || B < 1 || nsel < 1 || nsel > 8 || top >= H || bottom >= H || left >= W || right >= W || top < 0 || bottom < 0 ||
        left < 0 || right < 0 || (mean == nullptr) != (stdv == nullptr) || (kind == PC_DATA_SPLIT && (!data2 || !mean)) ||
        (kind != PC_DATA_INPUT && kind != PC_DATA_RAW && kind != PC_DATA_SPLIT))
        return PC_EINVAL;
    const int Hp = H + top + bottom, Wp = W + left + right;
    if (out_rstride < Wp || (out_rstride & 3) || (reinterpret_cast<uintptr_t>(out) & 15)) return PC_EINVAL;
    const int C2 = kind == PC_DATA_SPLIT ? 4 : 0;
    const int Ctot = kind == PC_DATA_SPLIT ? 6 : Cin;
    PadSel ps{};
    for (int j = 0; j < nsel; ++j) {
        if (sel[j] < 0 || sel[j] >= Ctot) return PC_EINVAL;
        ps.sel[j] = sel[j];
        ps.mean[j] = mean ? mean[j] : 0.f;
        ps.stdv[j] = stdv ? stdv[j] : 1.f;
    }
    const int wq = (Wp + 3) >> 2;
    const int64_t npieces = (int64_t)B * nsel * Hp * wq;
    const int64_t nblk = (npieces + 255) / 256;
    if (nblk > 0x7fffffff) return PC_EINVAL;
    const dim3 grid((unsigned)nblk);
    hipStream_t st = (hipStream_t)stream;
    if (kind == PC_DATA_SPLIT)
        hipLaunchKernelGGL((ingest_pad_strided_kernel<2, true>), grid, dim3(256), 0, st, data, data2, out, ps, 6, C2, nsel, H, W, Hp, Wp, out_rstride, top,
                           left, npieces, wq);
    else if (mean)
        hipLaunchKernelGGL((ingest_pad_strided_kernel<0, true>), grid, dim3(256), 0, st, data, data2, out, ps, Cin, 0, nsel, H, W, Hp, Wp, out_rstride, top,
                           left, npieces, wq);
    else
        hipLaunchKernelGGL((ingest_pad_strided_kernel<0, false>), grid, dim3(256), 0, st, data, data2, out, ps, Cin, 0, nsel, H, W, Hp, Wp, out_rstride, top,
                           left, npieces, wq);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_reflect_pad(const float* in, float* out, int64_t planes, int H, int W, int top, int bottom, int left, int right,
                              void* stream) {
    if (!in || !out || top >= H || bottom >= H || left >= W || right >= W || top < 0 || bottom < 0 || left < 0 || right < 0) return PC_EINVAL;
    const int Hp = H + top + bottom, Wp = W + left + right;
    int64_t g = (planes * Hp * Wp + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(reflect_pad_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, in, out, planes, H, W, Hp, Wp, top, left);
    PC_CHECK_LAUNCH();
    return 0;
}
