// conv3x3_up.h -- the first conv of an Up block taken straight from the low-resolution map: compose_up_kernel and the pc_conv3x3_up_*
// entry points; included at the end of conv3x3.hip (file scope: it uses the launchers and ConvArgs defined there).
//
// Up block without the up-sampled map:  conv3x3(cat[skip, ConvTranspose2d(z)]) = conv3x3(skip; W[:, :Cs]) + a parity-dependent
// 2 x 2-neighbourhood map of z + the transposed conv's bias through the taps (networks.py:302-318).
// compose_up_kernel builds, once per call (the weights change every step):
//   wz[stage][lane = 16 lk + li][4 m + 2 tj + j], K-slot q = 4 m + lk = (channel ci = q / 3, low-res row offset index v = q % 3):
//       sum over c' and the taps (dy, dx) that land on (v, sub-row a) / (column offset tj + j - 1, sub-column b) for output parity
//       (pY = li >> 3, pX = j) of  W[co = li & 7][Cs + c'][dy][dx] * Wt[8 stage + ci][c'][a][b]
//   tb[co] = {R0, R2, C0, C2, T00, T02, T20, T22, S} with T[co][dy][dx] = sum_c' W[co][Cs + c'][dy][dx] * bt[c']
namespace {
constexpr int COMPOSE_MAX = 2 * PC_MAX_GROUP;      // both Up levels of a forward pass in one launch
struct ComposeArgs {
    const float* w[COMPOSE_MAX]; const float* wt[COMPOSE_MAX]; const float* bt[COMPOSE_MAX]; float* ws[COMPOSE_MAX];
    int Cs[COMPOSE_MAX], C[COMPOSE_MAX];
};
__device__ __forceinline__ void up_rowmap(int p, int d, int& v, int& a) {      // parity p, tap d -> low-res offset index v (0..2), sub-pixel a
    const int t = p + d - 1;
    const int i = t < 0 ? -1 : (t >> 1);
    v = i + 1;
    a = t - 2 * i;
}
__global__ __launch_bounds__(256) void compose_up_kernel(const ComposeArgs a) {
    // the two small weight tensors go to LDS first (coalesced), the 64-term sums then read LDS (the direct form spent 18 us
    // of dependent L2 round trips per call)
    __shared__ float sW[8 * 16 * 9], sT[16 * 16 * 4], sB[16];
    const float* W = a.w[blockIdx.y];
    const float* Wt = a.wt[blockIdx.y];
    const float* bt = a.bt[blockIdx.y];
    float* ws = a.ws[blockIdx.y];
    const int C = a.C[blockIdx.y], Cs = a.Cs[blockIdx.y], Ct = Cs + C;
    for (int e = threadIdx.x; e < 8 * C * 9; e += 256) {
        const int co = e / (C * 9), r = e - co * C * 9;
        sW[e] = W[(co * Ct + Cs) * 9 + r];                      // [co][c'][tap] of the up half
    }
    for (int e = threadIdx.x; e < C * C * 4; e += 256) sT[e] = Wt[e];
    if (threadIdx.x < C) sB[threadIdx.x] = bt ? bt[threadIdx.x] : 0.f;
    __syncthreads();
    const int nwz = (C / 8) * 1536;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < nwz + 72 + 2048; e += gridDim.x * 256) {
        if (e >= nwz + 72) {
            // operand image of the BACKWARD data gradient (up_bwd.hip): wd[(4 (4 co + r) + c) * 16 + ci] = Kd[co][ci][r][c], the weight
            // of output pixel (2i - 1 + r, 2j - 1 + c) in dL/dz[ci][i][j]: window row r -> (pY, v) = (1,2), (0,1), (1,1), (0,0)
            const int k = e - nwz - 72, ci = k & 15, c = (k >> 4) & 3, r = (k >> 6) & 3, co = k >> 8;
            float acc = 0.f;
            if (ci < C) {
                const int pY = (r & 1) ^ 1, v = r == 0 ? 2 : (r == 3 ? 0 : 1);
                const int pX = (c & 1) ^ 1, c3 = c == 0 ? 2 : (c == 3 ? 0 : 1);
                for (int dy = 0; dy < 3; ++dy) {
                    int vv, sa;
                    up_rowmap(pY, dy, vv, sa);
                    if (vv != v) continue;
                    for (int dx = 0; dx < 3; ++dx) {
                        int cc, sb;
                        up_rowmap(pX, dx, cc, sb);
                        if (cc != c3) continue;
                        for (int cp = 0; cp < C; ++cp) acc += sW[(co * C + cp) * 9 + dy * 3 + dx] * sT[((ci * C + cp) * 2 + sa) * 2 + sb];
                    }
                }
            }
            ws[e] = acc;
        } else if (e < nwz) {
            const int stage = e / 1536, r = e - stage * 1536, lane = r / 24, qq = r - lane * 24;
            const int lk = lane >> 4, li = lane & 15, pY = li >> 3, co = li & 7;
            const int m = qq >> 2, tj = (qq >> 1) & 1, j = qq & 1;
            const int qs = 4 * m + lk, ci = stage * 8 + qs / 3, vrow = qs % 3;
            float acc = 0.f;
            for (int dy = 0; dy < 3; ++dy) {
                int v, sa;
                up_rowmap(pY, dy, v, sa);
                if (v != vrow) continue;
                for (int dx = 0; dx < 3; ++dx) {
                    int c3, sb;
                    up_rowmap(j, dx, c3, sb);
                    if (c3 != tj + j) continue;
                    for (int c = 0; c < C; ++c) acc += sW[(co * C + c) * 9 + dy * 3 + dx] * sT[((ci * C + c) * 2 + sa) * 2 + sb];
                }
            }
            ws[e] = acc;
        } else {
            const int k = e - nwz, co = k / 9, which = k - 9 * co;
            float T[3][3];
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) {
                    float t = 0.f;
                    for (int c = 0; c < C; ++c) t += sW[(co * C + c) * 9 + dy * 3 + dx] * sB[c];
                    T[dy][dx] = t;
                }
            float v;
            switch (which) {
                case 0: v = T[0][0] + T[0][1] + T[0][2]; break;
                case 1: v = T[2][0] + T[2][1] + T[2][2]; break;
                case 2: v = T[0][0] + T[1][0] + T[2][0]; break;
                case 3: v = T[0][2] + T[1][2] + T[2][2]; break;
                case 4: v = T[0][0]; break;
                case 5: v = T[0][2]; break;
                case 6: v = T[2][0]; break;
                case 7: v = T[2][2]; break;
                default: v = T[0][0] + T[0][1] + T[0][2] + T[1][0] + T[1][1] + T[1][2] + T[2][0] + T[2][1] + T[2][2]; break;
            }
            ws[nwz + k] = v;
        }
    }
}
}  // namespace

extern "C" int64_t pc_conv3x3_up_ws_bytes(int C) { return (int64_t)((C / 8) * 1536 + 72 + 2048) * sizeof(float); }

extern "C" int pc_conv3x3_up_fwd_ok(const pc_src* skip, const pc_src* z, const pc_dst* out, int H, int W, int Cs, int C) {
    if (g_pc_precision != PC_PREC_FP32 || !skip || !z || !out) return 0;
    // (any even width with 16-byte aligned rows: the low-resolution piece is masked per column, the border bias per pixel, the ragged
    // last strip of a row is stored by the per-element epilogue)
    if (!((Cs == 8 && C == 8) || (Cs == 16 && C == 16)) || (H & 3) || (W & 1)) return 0;
    if (skip->C != Cs || z->C != C || z->H * 2 != H || z->W * 2 != W || z->mode != PC_SRC_DIRECT || z->oy || z->ox) return 0;
    if (z->dtype != PC_F32 || !pc_planar(*z) || skip->dtype != PC_F32 || !pc_planar(*skip) || out->dtype != PC_F32 || !pc_planar(*out)) return 0;
    if (conv_src_mode(*skip, H, W) != 1) return 0;
    return (out->rstride % 4 == 0) && (out->cstride % 4 == 0) && (out->bstride % 4 == 0) && ((reinterpret_cast<uintptr_t>(out->ptr) & 15) == 0);
}

// composed operand images of up to 2 * PC_MAX_GROUP Up-block convolutions (any mix of (Cs, C) = (8, 8) / (16, 16)) in ONE launch:
// d[i].ws <- compose(d[i].w, d[i].wt, d[i].bt); a following pc_conv3x3_up_fwd_group(..., relu | PC_UP_PRECOMPOSED, ...) skips its own
extern "C" int pc_conv3x3_up_compose_group(int n, const pc_conv_up_fwd_desc* d, const int* Cs, const int* C, void* stream) {
    if (n < 1 || n > COMPOSE_MAX || !d || !Cs || !C) return PC_EINVAL;
    ComposeArgs ca{};
    int cmax = 0;
    for (int i = 0; i < n; ++i) {
        if (!d[i].w || !d[i].wt || !d[i].ws || !((Cs[i] == 8 && C[i] == 8) || (Cs[i] == 16 && C[i] == 16))) return PC_EINVAL;
        ca.w[i] = d[i].w; ca.wt[i] = d[i].wt; ca.bt[i] = d[i].bt; ca.ws[i] = (float*)d[i].ws;
        ca.Cs[i] = Cs[i]; ca.C[i] = C[i];
        if (C[i] > cmax) cmax = C[i];
    }
    hipLaunchKernelGGL(compose_up_kernel, dim3(((cmax / 8) * 1536 + 72 + 2048 + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, ca);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_conv3x3_up_fwd_group(int n, const pc_conv_up_fwd_desc* d, int relu, int B, int H, int W, int Cs, int C, void* stream) {
    if (n < 1 || n > MAXG || !d) return PC_EINVAL;
    const bool precomposed = (relu & PC_UP_PRECOMPOSED) != 0;
    relu &= 1;
    ConvArgs p{};
    ComposeArgs ca{};
    for (int i = 0; i < n; ++i) {
        if (!d[i].skip || !d[i].z || !d[i].w || !d[i].wt || !d[i].bn || !d[i].out || !d[i].ws ||
            !pc_conv3x3_up_fwd_ok(d[i].skip, d[i].z, d[i].out, H, W, Cs, C))
            return PC_EINVAL;
        ConvProb& q = p.pr[i];
        q.a = *d[i].skip;
        q.w = d[i].w;
        q.bn = *d[i].bn;
        q.out = *d[i].out;
        q.z = d[i].z->ptr; q.z_bs = d[i].z->bstride; q.z_cs = d[i].z->cstride; q.z_rs = d[i].z->rstride;
        q.wz = (const float*)d[i].ws;
        q.tb = (const float*)d[i].ws + (C / 8) * 1536;
        q.fast_a = 1;
        ca.w[i] = d[i].w; ca.wt[i] = d[i].wt; ca.bt[i] = d[i].bt; ca.ws[i] = (float*)d[i].ws;
        ca.Cs[i] = Cs; ca.C[i] = C;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!precomposed) {
        hipLaunchKernelGGL(compose_up_kernel, dim3(((C / 8) * 1536 + 72 + 2048 + 255) / 256, n), dim3(256), 0, st, ca);
        PC_CHECK_LAUNCH();
    }
    p.w_co_stride = (Cs + C) * 9;
    p.w_ci_stride = 9;
    p.relu = relu;
    p.B = B; p.H = H; p.W = W;
    p.vec_ok = 1;
    if (!conv_fill_geometry(p)) return 0;
    if (Cs == 8) {
        if (fwd_s3_ok<8, 8>(p, n, 8)) return launch_fwd_s3<8, 8, EPI_NONE, 8>(p, n, st);
        return launch_conv_po<8, 8, MODE_FWD, LD_DIRECT, EPI_NONE, 8>(p, n, st);
    }
    if (fwd_s3_ok<16, 8>(p, n, 16)) return launch_fwd_s3<16, 8, EPI_NONE, 16>(p, n, st);
    return launch_conv_po<16, 8, MODE_FWD, LD_DIRECT, EPI_NONE, 16>(p, n, st);
}
