// input_grad.hip -- gradient w.r.t. the model input: the data gradient of each stream's first convolution (networks.py:130-133: 2 SAR / 4
// optical input channels -> 8) followed by the adjoint of what that convolution's loader fuses, the reflect padding and the channel
// gather (PC_SRC_REFLECT + chmap; popcorn.py:231-258,130-134).  One launch for all active streams:
//
//   dXp_s[b,c,p,q]          = sum_{o<8} sum_{ky,kx<3} w_s[o,c,ky,kx] * G_s[b,o,p-ky+1,q-kx+1]          (G_s = 0 outside Hp x Wp)
//   dX[b,chmap_s[c],h,w]    = sum_{p: r_H(p)=h} sum_{q: r_W(q)=w} dXp_s[b,c,p,q]
//   r_H(p) = |p-pt| if |p-pt| < H else 2(H-1) - (p-pt)                                                 (likewise r_W with pl, W)
//
// Gather formulation: a workgroup owns a tile of IG_TH x IG_TW OUTPUT pixels of one (image, stream).  An output row h has at most three
// preimages in the padded domain -- h + pt always, pt - h for 1 <= h <= pt (top mirror), pt + 2(H-1) - h for 1 <= H-1-h <= pb (bottom
// mirror) -- and so has a column: at most 3 x 3 preimage tiles, each a contiguous (for a mirror: reversed) range of the padded domain.  The
// workgroup walks them in a fixed order and skips the empty ones with a workgroup-uniform branch.  For each it stages the G tile plus a
// one-pixel halo (8 channels) in LDS IN OUTPUT ORDER (LDS row r holds the padded row of output row h0 + r - 1, extended linearly past the
// range the preimage is valid on), so that the conv taps of an output pixel are its 3 x 3 LDS neighbourhood whatever the direction; a
// mirror only reverses the tap index, which is a template argument.  Each lane owns 4 consecutive rows of one column: the 6 x 3 window
// of a G channel is read once for the four pixels.  The weights sit in LDS too (rounded there in bf16 mode) and are read as broadcasts.
//
// No atomics; every dX element is accumulated in registers in the order (row preimage, column preimage, o, tap) and stored once, so equal
// inputs give equal bits.  G leaves HBM once plus the halo (18 x 66 / 16 x 64 = 1.16); 288 (144) FMA per padded pixel is VALU work far below
// the vector peak -- no MFMA.  PC_PREC_BF16: G is a channels-last bf16 tensor read as one 16-byte slot per pixel and lane; each weight is
// rounded to bf16 where it is used; accumulation and result are fp32 (oracle/popcorn_oracle.py: _qw on the weight, _rb on G, _rf on the input).
#include "common.h"

namespace {

constexpr int IG_TW = 64;                 // tile columns = lanes of a wave
constexpr int IG_TH = 16;                 // tile rows: 4 waves x 4 rows per lane
constexpr int IG_LH = IG_TH + 2;
constexpr int IG_LW = IG_TW + 2;

struct IgProblem {
    const void* g;                        // element (b = 0, o = 0, p = 0, q = 0)
    int64_t bstride, cstride;             // elements
    int rstride, xstride;                 // xstride: 1 (planar fp32) or the channel count of the channels-last bf16 tensor
    const float* w;                       // [8][cin][3][3]
    int cin;
    int chmap[4];
};

struct IgArgs {
    IgProblem p[2];
    float* dx;                            // (B, Cx, H, W) contiguous
    int Cx, H, W, Hp, Wp;
    int pt, pb, pl, pr;
    int tiles_x;
};

// output coordinate u -> padded coordinate a + s * u of preimage kind k (0 direct, 1 top / left mirror, 2 bottom / right mirror), and
// the range [lo, hi] of u the preimage exists on
__device__ __forceinline__ void ig_preimage(int k, int n, int pad0, int pad1, int& a, int& s, int& lo, int& hi) {
    if (k == 0) { a = pad0; s = 1; lo = 0; hi = n - 1; }
    else if (k == 1) { a = pad0; s = -1; lo = 1; hi = pad0; }
    else { a = pad0 + 2 * (n - 1); s = -1; lo = n - 1 - pad1; hi = n - 2; }
}

// the taps of one preimage tile for the lane's four pixels: part[k][c] = sum_o sum_taps w[o][c][ky][kx] * lds[o][i0 + k + a][j + b] with
// ky = FY ? a : 2 - a, kx = FX ? b : 2 - b (FY / FX: the preimage is a mirror along that axis)
template <int CIN, bool FY, bool FX>
__device__ __forceinline__ void ig_taps(const float (*lds)[IG_LH][IG_LW], const float* wl, int i0, int j, float (&part)[4][CIN]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < CIN; ++c) part[k][c] = 0.f;
#pragma unroll 1
    for (int o = 0; o < 8; ++o) {
        float wr[CIN * 9];                        // one address for all lanes: broadcast reads, four weights each
#pragma unroll
        for (int i = 0; i < CIN * 9; ++i) wr[i] = wl[o * CIN * 9 + i];
        float g[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[r][b] = lds[o][i0 + r][j + b];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
#pragma unroll
                    for (int c = 0; c < CIN; ++c) part[k][c] = fmaf(wr[(c * 3 + (FY ? a : 2 - a)) * 3 + (FX ? b : 2 - b)], g[k + a][b], part[k][c]);
    }
}

template <int CIN, bool BF>
__device__ __forceinline__ void ig_tile(const IgArgs& a, const IgProblem& P, float (*lds)[IG_LH][IG_LW], float* wl, int b, int h0, int w0) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i0 = 4 * wv;                          // the lane's local rows i0 .. i0 + 3, local column `lane`
    const int h1 = min(h0 + IG_TH, a.H) - 1, w1 = min(w0 + IG_TW, a.W) - 1;
    // global (not generic) pointers: flat loads would count on the LDS counter as well
    const float* wp = pc_pin_ptr(P.w);
    const float* g32 = pc_pin_ptr(static_cast<const float*>(P.g));
    const pc_bf16_t* g16 = pc_pin_ptr(static_cast<const pc_bf16_t*>(P.g));
    float* dx = pc_pin_ptr(a.dx);
    // the weights [8][CIN][3][3] into LDS, rounded in bf16 mode (the first barrier pair below orders them before their readers)
    for (int i = threadIdx.x; i < 72 * CIN; i += 256) wl[i] = BF ? pc_bf16r(wp[i]) : wp[i];
    float acc[4][CIN];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[k][c] = 0.f;

    for (int ky = 0; ky < 3; ++ky) {
        int ay, sy, ylo, yhi;
        ig_preimage(ky, a.H, a.pt, a.pb, ay, sy, ylo, yhi);
        ylo = max(ylo, h0);
        yhi = min(yhi, h1);
        if (ylo > yhi) continue;                    // workgroup-uniform
        for (int kx = 0; kx < 3; ++kx) {
            int ax, sx, xlo, xhi;
            ig_preimage(kx, a.W, a.pl, a.pr, ax, sx, xlo, xhi);
            xlo = max(xlo, w0);
            xhi = min(xhi, w1);
            if (xlo > xhi) continue;                // workgroup-uniform
            const int ia = ylo - h0, ib = yhi - h0, ja = xlo - w0, jb = xhi - w0;      // local ranges the preimage exists on
            __syncthreads();                        // the previous preimage's readers are done
            // stage LDS rows ia .. ib + 2, columns ja .. jb + 2: LDS (r, cc) = padded (ay + sy (h0 + r - 1), ax + sx (w0 + cc - 1))
            for (int r = ia + wv; r <= ib + 2; r += 4) {
                const int p = ay + sy * (h0 + r - 1);
                const bool rok = (unsigned)p < (unsigned)a.Hp;
                for (int cc = ja + lane; cc <= jb + 2; cc += 64) {
                    const int q = ax + sx * (w0 + cc - 1);
                    const bool ok = rok && (unsigned)q < (unsigned)a.Wp;
                    if (BF) {
                        u32x4 v = u32x4{0u, 0u, 0u, 0u};
                        if (ok)
                            v = *reinterpret_cast<const u32x4*>(g16 + b * P.bstride + (int64_t)p * P.rstride +
                                                                (int64_t)q * P.xstride);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            lds[2 * e][r][cc] = __uint_as_float(v[e] << 16);
                            lds[2 * e + 1][r][cc] = __uint_as_float(v[e] & 0xffff0000u);
                        }
                    } else {
                        const float* gp = g32 + b * P.bstride + (int64_t)p * P.rstride + q;
                        float v[8];
#pragma unroll
                        for (int o = 0; o < 8; ++o) v[o] = ok ? gp[o * P.cstride] : 0.f;
#pragma unroll
                        for (int o = 0; o < 8; ++o) lds[o][r][cc] = v[o];
                    }
                }
            }
            __syncthreads();
            if (i0 > ib || i0 + 3 < ia) continue;   // wave-uniform: none of this wave's rows has the preimage
            float part[4][CIN];
            if (sy > 0) {
                if (sx > 0) ig_taps<CIN, false, false>(lds, wl, i0, lane, part);
                else ig_taps<CIN, false, true>(lds, wl, i0, lane, part);
            } else {
                if (sx > 0) ig_taps<CIN, true, false>(lds, wl, i0, lane, part);
                else ig_taps<CIN, true, true>(lds, wl, i0, lane, part);
            }
            const bool xok = lane >= ja && lane <= jb;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = xok && i0 + k >= ia && i0 + k <= ib;
#pragma unroll
                for (int c = 0; c < CIN; ++c) acc[k][c] += ok ? part[k][c] : 0.f;
            }
        }
    }
    const int w = w0 + lane;
    if (w >= a.W) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int h = h0 + i0 + k;
        if (h >= a.H) continue;
#pragma unroll
        for (int c = 0; c < CIN; ++c) dx[(((int64_t)b * a.Cx + P.chmap[c]) * a.H + h) * a.W + w] = acc[k][c];
    }
}

template <bool BF>
__global__ void __launch_bounds__(256) input_grad_kernel(const IgArgs a) {
    __shared__ float lds[8][IG_LH][IG_LW];
    __shared__ __attribute__((aligned(16))) float wl[8 * 4 * 9];
    const IgProblem& P = a.p[blockIdx.z];
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    if (P.cin == 2) ig_tile<2, BF>(a, P, lds, wl, blockIdx.y, ty * IG_TH, tx * IG_TW);
    else ig_tile<4, BF>(a, P, lds, wl, blockIdx.y, ty * IG_TH, tx * IG_TW);
}

}  // namespace

extern "C" int pc_input_grad(int n, const pc_input_grad_desc* d, float* dx, int B, int Cx, int H, int W, int pad_top, int pad_bottom,
                             int pad_left, int pad_right, void* stream) {
    if (!d || !dx || n < 1 || n > 2 || B < 1 || B > 65535 || H < 1 || W < 1 || (Cx != 2 && Cx != 4 && Cx != 6)) return PC_EINVAL;
    // torch's reflect rule: every pad smaller than the extent it mirrors
    if (pad_top < 0 || pad_bottom < 0 || pad_left < 0 || pad_right < 0 || pad_top > H - 1 || pad_bottom > H - 1 || pad_left > W - 1 ||
        pad_right > W - 1)
        return PC_EINVAL;
    const bool bf = g_pc_precision == PC_PREC_BF16;
    IgArgs a{};
    a.dx = dx; a.Cx = Cx; a.H = H; a.W = W;
    a.Hp = H + pad_top + pad_bottom; a.Wp = W + pad_left + pad_right;
    a.pt = pad_top; a.pb = pad_bottom; a.pl = pad_left; a.pr = pad_right;
    int covered[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) {
        const pc_src* g = d[i].g;
        if (!g || !g->ptr || !d[i].w || (d[i].cin != 2 && d[i].cin != 4)) return PC_EINVAL;
        if (g->C != 8 || g->mode != PC_SRC_DIRECT || g->oy != 0 || g->ox != 0 || g->H != a.Hp || g->W != a.Wp) return PC_EINVAL;
        if (bf ? !pc_cl_ok(*g) : (g->dtype != PC_F32 || !pc_planar(*g))) return PC_EINVAL;
        IgProblem& P = a.p[i];
        P.g = g->ptr; P.bstride = g->bstride; P.cstride = g->cstride; P.rstride = g->rstride; P.xstride = pc_xs(*g);
        P.w = d[i].w; P.cin = d[i].cin;
        for (int c = 0; c < d[i].cin; ++c) {
            const int ch = d[i].chmap[c];
            if (ch < 0 || ch >= Cx || covered[ch]++) return PC_EINVAL;       // outside dX, or a channel written twice
            P.chmap[c] = ch;
        }
    }
    for (int ch = 0; ch < Cx; ++ch)
        if (!covered[ch]) return PC_EINVAL;                                  // a channel of dX nobody writes
    a.tiles_x = (W + IG_TW - 1) / IG_TW;
    const int64_t tiles = (int64_t)a.tiles_x * ((H + IG_TH - 1) / IG_TH);
    if (tiles > INT32_MAX) return PC_EINVAL;
    const dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)n);
    if (bf) hipLaunchKernelGGL(input_grad_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(input_grad_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}
