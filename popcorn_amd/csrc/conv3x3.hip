// conv3x3.hip -- 3x3 / pad-1 convolution on fp32 MFMA (v_mfma_f32_16x16x4_f32) for gfx950.
//
// Replaces nn.Conv2d(3, padding=1) + BatchNorm2d(eval) + ReLU (reference model/DDA_model/utils/networks.py:259-266)
// and, with transposed weight indexing, its autograd data-gradient.
//
// GEMM mapping ("vertical pair" im2col): one MFMA produces a 16(x) x 2(rows) patch for 8 output channels:
//     M (16)  = 16 consecutive output x
//     N (16)  = (s, co):  s in {0,1} = which of the two output rows, co = 8 output channels
//     K (4)   = v: the 4 input rows (y0-1 .. y0+2) that the two output rows touch
//     one MFMA per (input channel ci, horizontal tap dx);  B[v][(s,co)] = w[co][ci][v-s][dx] (0 when v-s not in 0..2)
// so 9 useful taps ride on 12 K-slots: 75 % MFMA efficiency at Cout = 8 (a plain im2col with N = Cout = 8 wastes half
// of every MFMA).  The 16-output layers use the plain im2col instead (N16 below: N = 16 channels, K = 4 consecutive
// (ci, dy, dx) of a chunk's 72): every issued K-slot is a tap.
//
// Data movement: a workgroup (4 waves) owns a 32 x 16 output tile; the (CHUNK x 18 x 40) input halo tile is staged
// in LDS with row stride 48 (= 16 mod 32 banks), which makes the A-operand read -- lane (i = x, k = row) ->
// lds[ci][2*rp + k][x + dx] -- bank-conflict free.  Weights live in registers as ready-made B fragments for the
// whole kernel; workgroups are persistent over tiles (XCD-aware tile order).
//
// The tile loop is a software pipeline: every 16-lane group owns one (channel, row-range) of the halo tile and moves
// its rows as aligned 16-byte segments; the loads of tile t+1 are issued into registers before the MFMA phase of tile
// t and written to LDS after it, so HBM latency hides under MFMA inside one workgroup.  The first version spent ~1200
// mostly scalar/branch instructions per tile per wave on loader index arithmetic and was instruction-issue bound at
// 4x the MFMA time (profiles/r1_v0, tools/ablate_conv.py); the hot path below is ~10 VALU per 16-byte segment.
//
// Up to PC_MAX_GROUP independent problems of identical geometry (e.g. the SAR and optical streams, or the frozen
// building extractor next to the trainable U-Net) share one launch: blockIdx.y selects the problem.
//
// ONE translation unit (one code object, one set of per-file compiler flags) in five pieces:
//   conv3x3_args.h    ConvProb / ConvArgs, the strip geometry, the MODE_* / LD_* / EPI_* constants
//   conv3x3.hip       conv3x3_mfma_kernel (planar fp32 on the fp32 matrix pipe), the dispatch, the C entry points of the forward and the
//                     data gradient
//   conv3x3_fwd_s3.h  conv3x3_fwd_s3_kernel: the planar fp32 forward on the bf16 matrix pipe (split operands)
//   conv3x3_cl.h      conv3x3_cl_kernel: channels-last bf16, its launchers and descriptor validation
//   conv3x3_up.h      compose_up_kernel and the pc_conv3x3_up_* entry points (the first conv of an Up block without the up-sampled map)
//
// Which form is what:
//   kernel                   PC_PREC_FP32                                                        PC_PREC_BF16
//   conv3x3_fwd_s3_kernel    product: every aligned 8- / 16-channel forward layer, composed Up   --
//   conv3x3_mfma_kernel      product: first layers (2 / 4 inputs), 32 -> 8, unaligned or pooled   --
//                            launches, every data gradient outside the fused backward;
//                            test fixture behind pc_set_conv_split(0): every layer (A/B, the
//                            strict fp32-product tests)
//   conv3x3_cl_kernel        --                                                                  product: every conv forward and data gradient
//   compose_up_kernel        product (once per step)                                             --
// Ablation build (-DPOPCORN_CONV_ABLATE, tools/build_variant.sh): the phase switches of pc_debug_conv and the timeline stamps of
// pc_debug_conv_ts; a product build compiles them out (forced grid sizes are host code and work everywhere).
// Instantiated: forward (Cin, Cout) = (2,8) (4,8) (8,8) (16,8) (32,8) (8,16) (16,16) with every loader and epilogue a launch can select;
// data gradient (Cg, Cn) in {8, 16}^2 with the DIRECT (fp32 also: GENERIC) loader, plain or with the max-pool scatter.
#include "common.h"
#include <type_traits>
#include "tile_loader.h"

static int g_conv_dbg = 0, g_conv_max_grid = 0;
static long long* g_conv_ts = nullptr;     // debug: per-workgroup (start, end, hw id) timestamps (tools/conv_timeline.py)
extern "C" void pc_debug_conv(int dbg, int max_grid) { g_conv_dbg = dbg; g_conv_max_grid = max_grid; }
extern "C" void pc_debug_conv_ts(void* buf) { g_conv_ts = (long long*)buf; }

namespace {

#include "conv3x3_args.h"

// Wave-private strips.  Each wave owns a 32 x 4 output strip (4 MFMA units), stages its own (CHUNK x 6 x 40) halo
// strip in a private LDS region and runs its own software pipeline -- there is NO workgroup barrier in the loop: DS
// operations of one wave execute in order, so "ds_write strip t+1" behind "ds_read strip t" needs no synchronisation.
// Waves therefore drift apart and the hardware interleaves one wave's MFMA phase with the others' loads, LDS writes
// and epilogue stores.  (The workgroup-tile version kept all waves of a CU in lock-step through its two barriers per
// tile: MFMA pipe 42 % busy with waves parked in issue stalls, total time == sum of the phases; tools/ablate_conv.py.)
// The price is a 6/4 instead of 18/16 row halo, served by L2.
template <int CIN, int COUT, int MODE, int LD, int EPI, int ZC = 0>
__global__ __launch_bounds__(256) void conv3x3_mfma_kernel(const ConvArgs p) {
    constexpr int CHUNK = CIN < 8 ? CIN : 8;       // 8 channels per LDS stage: 36 KB per workgroup, 4 workgroups per CU
    constexpr int NCHUNK = CIN / CHUNK;
    // ZC > 0: ZC more input "channels" that exist only at HALF the resolution -- the map z that ConvTranspose2d(ZC, ZC, 2, 2) would
    // have up-sampled into the second half of torch.cat([skip, up]) (networks.py:302-318).  conv3x3(convT(z)) is a linear map
    // with a 2 x 2 low-resolution neighbourhood per output-pixel parity (pY, pX); its weights are composed once per step
    // (compose_up_kernel) and every 8 low-resolution channels are one more stage of the strip: a 4-row x 18-column piece of z
    // in the wave's LDS region (a quarter of a regular chunk's bytes) and 64 MFMAs instead of 96 -- K = the 3 low-res rows a row
    // pair touches, one MFMA per (channel, column tap tj, x parity j); the up-sampled map is neither written nor read.
    constexpr int NZ = ZC / 8;                          // composed stages per strip
    constexpr int NST = NCHUNK + NZ;                    // stages per strip
    constexpr int NB = COUT / 8;
    constexpr bool STAGED = LD != LD_GENERIC;
    constexpr int NIT = CHUNK;                           // one 16-byte segment per channel per lane
    constexpr int W_RL = CIN * 3 + 4;                    // weight image: floats per (dy, co) row (== 4 mod 8: spreads banks)
    constexpr int W_DYS = COUT * W_RL + 16;              // ... and per dy plane
    // 16 output channels: plain im2col, N = 16 channels, M = 16 x of ONE row, K = 4 consecutive (ci, dy, dx) of a chunk's 72 --
    // every issued MFMA slot is a tap (the row-pair mapping of the 8-channel blocks spends 12 K-slots on 9 taps)
    constexpr bool N16 = COUT == 16 && CHUNK == 8;
    constexpr int W16_S = CIN * 9 + 1;                   // N16 weight image [co][ci * 9 + tap], odd row stride: 16 channels on 16 banks
    // P2 ("paired pixels", the strips of a launch with a composed stage): M index i of an MFMA is pixel x = 2 i + j of the
    // 32-px strip row (j = 0, 1: two MFMAs), so that ONE aligned ds_read_b64 feeds two pixels = operands of several (j, dx)
    // MFMAs: 3 LDS reads per 6 MFMAs instead of 6 (tools/mfma_peak.hip: the fp32 matrix pipe sustains 153 TFLOP/s from
    // registers but 97-107 with one ds_read_b32 per MFMA -- the conv kernels' MFMA phase was LDS-operand-issue bound, not power
    // bound).  The strip image becomes [row][channel][40] with a row-plane stride == 32 (mod 64) dwords: the two rows a 32-lane
    // half of a b64 read touches fall on complementary bank halves.
    constexpr bool P2 = ZC > 0 && !N16 && CHUNK == 8;
    static_assert(ZC == 0 || (P2 && MODE == MODE_FWD && LD == LD_DIRECT && EPI == EPI_NONE && COUT == 8), "composed up-sampling stage");
    constexpr int ZROW = 48, ZCH = 4 * ZROW + 16;       // low-res piece: [8 ch][4 rows][48] floats; ZROW == ZCH - 2 ZROW == 16 (mod 32)
    constexpr int WZ_L = 28;                            // composed weight image: [stage][lane][24 (+4 pad)] floats
    constexpr int LCH = P2 ? 40 : CSW;                   // floats between channels of the strip image
    constexpr int LROW = P2 ? 8 * 40 + 32 : RS;          // floats between rows
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const ConvProb& q = p.pr[blockIdx.y];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;      // A: (i, k);  B: (k, n = li);  D: (n = li, rows 4*lk + r)
    const int s_row = li >> 3, col = li & 7;
    // ablation switches and timeline stamps (pc_debug_conv, pc_debug_conv_ts) exist in -DPOPCORN_CONV_ABLATE builds only
    // (tools/build_variant.sh): as run-time flags they made issue() / commit() conditional (conv3x3_fwd_s3.h: what that costs)
#ifdef POPCORN_CONV_ABLATE
    int dbg = p.dbg;
    pc_pin(dbg);
    if (dbg & 8) return;
    if (p.ts && tid == 0) {
        long long* t = p.ts + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
        t[0] = wall_clock64();
        t[2] = __builtin_amdgcn_s_getreg((31 << 11) | 4) | ((long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
    }
#else
    int dbg = 0;
    if constexpr (conv_mfma_keeps_switch_tests(CIN, COUT, MODE, LD, EPI, ZC)) pc_pin(dbg);
#endif

    constexpr int WAVE_F = P2 ? SROWS * LROW : CHUNK * CSW;   // floats of one wave's LDS region
    float* const wl = lds + wave * WAVE_F;               // this wave's LDS region

    // ---- staged loader: lane = (row r of the 6-row strip, 16-byte segment seg of the 40-float row)
    const int l_r = lane / 10, l_seg = lane - l_r * 10;
    const bool l_act = lane < 60;
    const int CA = q.a.C;
    using act_t = float;
    const act_t* const a_ptr = reinterpret_cast<const act_t*>(q.a.ptr);
    const act_t* const b_ptr = reinterpret_cast<const act_t*>(q.b.ptr);
    const int64_t a_cstr = q.a.cstride, b_cstr = q.b.cstride;
    const int64_t my_bs = q.a.bstride;
    const int my_rs = q.a.rstride;                       // launch_conv guarantees identical layouts for both sources
    // Loads are issued UNCONDITIONALLY (out-of-image segments read a clamped, always-valid address) and the validity
    // mask is applied when the registers are written to LDS: a predicated load is if-converted into load + select,
    // i.e. an s_waitcnt right behind the load and no overlap with the MFMA phase.
    f32x4 R[NIT];
    int rvalid = 0;                                       // how many of the segment's 4 pixels are inside the image (0 .. 4)
    // the sources' extents, pinned in scalar registers: read from the descriptor inside issue() they were three DEPENDENT scalar-memory
    // round trips (s_load + s_waitcnt lgkmcnt(0), which also drains the LDS queue) in front of every strip's prefetch (round 6)
    int aW = q.a.W, aH = q.a.H, bW = q.b.W, bH = q.b.H, pW = p.W, pH = p.H;
    pc_pin(aW); pc_pin(aH); pc_pin(bW); pc_pin(bH); pc_pin(pW); pc_pin(pH);
    auto issue = [&](int ch, int b, int y0, int x0) {
        const int xg = x0 - 4 + 4 * l_seg, y = y0 - 1 + l_r;
        // DIRECT: a source placed at (0, 0) may be SMALLER than the conv domain -- the up-sampled half of an Up block's concatenated input
        // when the skip map has an odd extent (zero F.pad on the bottom / right, networks.py:309-312): rows / columns beyond the extent of
        // the chunk's own source are zeros.  (A chunk never straddles the two sources: the first one has 8 or 16 channels.)
        const int sW = LD == LD_DIRECT ? (ch * CHUNK < CA ? aW : bW) : pW;
        const int sH = LD == LD_DIRECT ? (ch * CHUNK < CA ? aH : bH) : pH;
        const bool ok = l_act && xg >= 0 && xg < sW && (unsigned)y < (unsigned)sH;
        // a row whose width is not a multiple of 4 ends inside a segment: the tail of that segment is read (the row stride is a
        // multiple of 4, so the 16 bytes exist) and masked per pixel when it is written to LDS
        rvalid = ok ? (sW - xg < 4 ? sW - xg : 4) : 0;
        if (LD == LD_REFLECT) {
            // first layer: reflect padding + channel gather; handles its own bounds (segments may straddle x = 0 / W)
            rvalid = l_act ? 4 : 0;
#pragma unroll
            for (int it = 0; it < NIT; ++it)
                R[it] = l_act ? pc_fetch_reflect_seg(q.a, b, ch * CHUNK + it, y, xg, p.H, p.W) : f32x4{0.f, 0.f, 0.f, 0.f};
            // (bf16 mode: the model input is the one operand no producer has rounded -- the pack in commit() rounds it)
        } else if (LD == LD_DIRECT) {
            const int64_t off = ok ? b * my_bs + (int64_t)y * my_rs + xg : 0;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int cg = ch * CHUNK + it;
                const act_t* cp = cg < CA ? a_ptr + cg * a_cstr : b_ptr + (cg - CA) * b_cstr;
                R[it] = pc_ld4(cp + off);
            }
        } else if (LD == LD_POOL) {
            const int64_t off = ok ? b * my_bs + (int64_t)(2 * y) * my_rs + 2 * xg : 0;
            const int rs1 = ok ? my_rs : 0;
            // the second 16-byte piece of the window: beyond the source row when fewer than 3 output pixels of this segment exist
            // (ragged width) -- it is then masked anyway and reads the first piece's address instead
            const int o4 = rvalid > 2 ? 4 : 0;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const act_t* s0 = a_ptr + (ch * CHUNK + it) * a_cstr + off;
                const f32x4 a0 = pc_ld4(s0), a1 = pc_ld4(s0 + o4);
                const f32x4 b0 = pc_ld4(s0 + rs1), b1 = pc_ld4(s0 + rs1 + o4);
                f32x4 v;
                v[0] = fmaxf(fmaxf(a0[0], a0[1]), fmaxf(b0[0], b0[1]));
                v[1] = fmaxf(fmaxf(a0[2], a0[3]), fmaxf(b0[2], b0[3]));
                v[2] = fmaxf(fmaxf(a1[0], a1[1]), fmaxf(b1[0], b1[1]));
                v[3] = fmaxf(fmaxf(a1[2], a1[3]), fmaxf(b1[2], b1[3]));
                R[it] = v;
            }
        }
    };
    auto commit = [&]() {
        if (l_act) {
            float* d = wl + l_r * LROW + 4 * l_seg;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = e < rvalid ? R[it][e] : 0.f;
                *reinterpret_cast<f32x4*>(d + it * LCH) = v;
            }
        }
    };
    auto load_generic = [&](int ch, int b, int y0, int x0) {
        for (int idx = lane; idx < CHUNK * SROWS * 34; idx += 64) {
            const int c = idx % 34, r = (idx / 34) % SROWS, ci = idx / (34 * SROWS);
            const int cg = ch * CHUNK + ci;
            const float v = cg < CA ? pc_fetch(q.a, b, cg, y0 - 1 + r, x0 - 1 + c, p.H, p.W)
                                    : pc_fetch(q.b, b, cg - CA, y0 - 1 + r, x0 - 1 + c, p.H, p.W);
            wl[ci * LCH + r * LROW + (COL0 - 1) + c] = v;
        }
    };

    // ---- composed stage: 8 low-res channels x 4 rows (y0/2 - 1 ..) x 18 columns (x0/2 - 1 ..) = 576 floats: lane = (channel, row,
    // half of the 18 columns), 9 consecutive floats each -- one address per lane, immediate offsets (a generic element index per
    // load cost 50 registers of hoisted address arithmetic)
    float Rz[ZC > 0 ? 9 : 1];
    bool pend_z = false;                                 // the prefetch in flight is a low-res piece (wave-uniform)
    const int z_ch = lane >> 3, z_row = (lane >> 1) & 3, z_half = lane & 1;
    auto issue_z = [&](int zc, int b, int y0, int x0) {
        if constexpr (ZC > 0) {
            const int Hh = p.H >> 1, Wh = p.W >> 1;
            int I = (y0 >> 1) - 1 + z_row;
            I = I < 0 ? 0 : (I >= Hh ? Hh - 1 : I);                            // clamped: masked when it is written to LDS
            const int c0 = (x0 >> 1) - 1 + 9 * z_half;                          // first of the lane's 9 columns (>= -1)
            const float* rowp = q.z + b * q.z_bs + (int64_t)(zc * 8 + z_ch) * q.z_cs + (int64_t)I * q.z_rs;
            if (c0 + 7 < Wh) {                                                  // columns 1..7 inside the row: immediate offsets
                Rz[0] = rowp[c0 < 0 ? 0 : c0];
#pragma unroll
                for (int k = 1; k < 8; ++k) Rz[k] = rowp[c0 + k];
                Rz[8] = rowp[c0 + 8 < Wh ? c0 + 8 : Wh - 1];                    // (the halo column of the image's last tile)
            } else {
                // the piece ends beyond the row (a map narrower than 18 columns, the ragged last tile): clamped like the rows, masked
                // when it is written to LDS -- unclamped these loads ran into the next row and, in the last row of the last channel
                // of the last image, up to 16 floats past the end of z
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const int c = c0 + k;
                    Rz[k] = rowp[c < 0 ? 0 : (c < Wh ? c : Wh - 1)];
                }
            }
        }
    };
    auto commit_z = [&](int y0, int x0) {        // the coordinates of the strip whose piece is pending
        if constexpr (ZC > 0) {
            const int Hh = p.H >> 1, Wh = p.W >> 1;
            const bool rok = (unsigned)((y0 >> 1) - 1 + z_row) < (unsigned)Hh;
            const int c0 = (x0 >> 1) - 1 + 9 * z_half;
            float* d = wl + z_ch * ZCH + z_row * ZROW + 9 * z_half;
#pragma unroll
            for (int k = 0; k < 9; ++k) d[k] = rok && (unsigned)(c0 + k) < (unsigned)Wh ? Rz[k] : 0.f;
        }
    };

    // strips: tile-major so that the 4 waves of a workgroup take the 4 strips of one 32 x 16 tile (shared halo rows
    // hit in L1/L2); workgroups walk the tiles in the XCD-aware order.
    int gdim = (int)gridDim.x;                           // (pinned: read from the dispatch packet inside the loop it was one more scalar round trip per strip)
    pc_pin(gdim);
    const int my_tiles = p.ntiles > (int)blockIdx.x ? (p.ntiles - 1 - (int)blockIdx.x) / gdim + 1 : 0;
    const int nstages = my_tiles * NST;
    auto strip_coords = [&](int stage, int& b, int& y0, int& x0) {
        pc_strip_coords<TW, TH>(blockIdx.x + (stage / NST) * gdim, &p.ntiles, &p.tiles_x, &p.tiles_y, &p.div_tpi, &p.div_tx, wave, b, y0, x0);
    };

    // The loads of the first strip are in flight while the weights are staged.
    int b = 0, y0 = 0, x0 = 0;
    if (nstages > 0) {
        strip_coords(0, b, y0, x0);
        if (STAGED && !(dbg & 1)) issue(0, b, y0, x0);
    }

    // ---- B fragments: bw[ci][dx][nb] = w[co = nb*8+col][ch*CHUNK + ci][dy = lk - s_row][dx]  (0 when dy is not a tap)
    // The (strided, possibly transposed) weight tensor is copied ONCE per workgroup into an LDS image behind the wave
    // regions, laid out [dy 0..3][co][ci*3+dx] with an all-zero dy = 3 plane for the lanes whose (row, output row) pair
    // is not a tap; a lane's fragments for one 8-channel chunk are then 24 consecutive floats = 6 ds_read_b128.  Only
    // the current chunk's fragments live in registers (24 per 8 output channels whatever CIN is): holding all of them
    // cost 96 registers at CIN = 32 and left 16->8 / 32->8 / 16->16 with two or ONE wave per SIMD.
    // Prologue latency: the weight elements and the raw BN parameters are loaded into registers FIRST (one memory round
    // trip, in flight together with the first strip), the LDS image is zeroed meanwhile, and only then are they consumed
    // -- the prologue used to be three dependent round trips (zero fill + barrier, weights, BN), ~4.6 us of every launch.
    float* const w2 = lds + 4 * WAVE_F;
    float* const wzimg = w2 + (N16 ? 16 * W16_S : 4 * W_DYS);          // ZC > 0: composed weights [stage][lane][WZ_L]
    float wzreg[ZC > 0 ? NZ * 6 : 1];
    if constexpr (ZC > 0) {
#pragma unroll
        for (int k = 0; k < NZ * 6; ++k) wzreg[k] = q.wz[tid + 256 * k];          // NZ * 1536 floats, coalesced
    }
    constexpr int NWR = (COUT * CIN * 9 + 255) / 256;
    float wreg[NWR];
#pragma unroll
    for (int k = 0; k < NWR; ++k) {
        const int e = tid + k * 256;
        const int ec = e < COUT * CIN * 9 ? e : 0;
        const int tap = ec % 9, ci = (ec / 9) % CIN, co = ec / (9 * CIN);
        wreg[k] = q.w[co * p.w_co_stride + ci * p.w_ci_stride + (p.w_flip ? 8 - tap : tap)];
    }
    const bool has_bn = MODE == MODE_FWD || q.act != nullptr;
    float bn_raw[NB][5];            // {conv bias, gamma, var, mean, beta} of channel nb*8 + col
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = N16 ? li : nb * 8 + col;          // N16: one channel per lane (slot nb = 0 is the one that is used)
        bn_raw[nb][0] = has_bn && q.bn.conv_bias ? q.bn.conv_bias[c] : 0.f;
        bn_raw[nb][1] = has_bn && q.bn.gamma ? q.bn.gamma[c] : 1.f;
        bn_raw[nb][2] = has_bn && q.bn.gamma ? q.bn.var[c] : 1.f;
        bn_raw[nb][3] = has_bn && q.bn.gamma ? q.bn.mean[c] : 0.f;
        bn_raw[nb][4] = has_bn && q.bn.gamma ? q.bn.beta[c] : 0.f;
    }
    {
        // only the dy = 3 plane has to be zero (the pad floats of the other planes are never read): disjoint from the weight
        // writes below, so one barrier covers both
        if constexpr (!N16)
            for (int e = tid; e < W_DYS; e += 256) w2[3 * W_DYS + e] = 0.f;
        if constexpr (ZC > 0) {
#pragma unroll
            for (int k = 0; k < NZ * 6; ++k) {
                const int e = tid + 256 * k, zc = e / 1536, r = e - zc * 1536;    // global order [stage][lane][24]
                wzimg[zc * 64 * WZ_L + (r / 24) * WZ_L + (r % 24)] = wzreg[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NWR; ++k) {
            const int e = tid + k * 256;
            if (e < COUT * CIN * 9) {
                const int tap = e % 9, ci = (e / 9) % CIN, co = e / (9 * CIN);
                if constexpr (N16) w2[co * W16_S + ci * 9 + tap] = wreg[k];
                else w2[(tap / 3) * W_DYS + co * W_RL + ci * 3 + (tap % 3)] = wreg[k];
            }
        }
        __syncthreads();
    }
    const float* const wlane = w2 + (((unsigned)(lk - s_row) <= 2u) ? lk - s_row : 3) * W_DYS + col * W_RL;
    float bw[CHUNK][3][NB];
    // N16: B fragment of step m = weight (co = li, K-slot 4 * m + lk of the chunk); A = pixel (row + dy, x + dx) of channel ci
    const float* const wlane16 = w2 + li * W16_S + lk;
    int aoff16[18];
#pragma unroll
    for (int m = 0; m < 18; ++m) {
        const int kk = 4 * m + lk, ci = kk / 9, t = kk - 9 * ci, dy = t / 3;
        aoff16[m] = ci * CSW + dy * RS + (t - 3 * dy);
    }
    auto load_bw = [&](int ch) {
        if constexpr (N16) {
#pragma unroll
            for (int m = 0; m < 18; ++m) bw[m / 6][(m % 6) / 2][m % 2] = wlane16[ch * 72 + 4 * m];
        } else if constexpr (CHUNK == 8) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(wlane + nb * 8 * W_RL + ch * 24 + 4 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) bw[(4 * j + e) / 3][(4 * j + e) % 3][nb] = t[e];
                }
        } else {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int k = 0; k < CHUNK * 3; ++k) bw[k / 3][k % 3][nb] = wlane[nb * 8 * W_RL + k];
        }
    };
    // ---- per-lane epilogue constants for co = nb*8 + col
    float e_scale[NB], e_shift[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        // folded BN (pc_bn_fold): scale = gamma / sqrt(var + eps); shift = (bias - mean) * scale + beta
        if (has_bn && q.bn.gamma) {
            e_scale[nb] = bn_raw[nb][1] * (1.0f / sqrtf(bn_raw[nb][2] + q.bn.eps));
            e_shift[nb] = (bn_raw[nb][0] - bn_raw[nb][3]) * e_scale[nb] + bn_raw[nb][4];
        } else {
            e_scale[nb] = 1.f;
            e_shift[nb] = has_bn ? bn_raw[nb][0] : 0.f;
        }
    }
    // Consume the BN constants HERE.  They come from global loads issued before the strip loop and are first used in
    // the epilogue inside it; hipcc's waitcnt pass then keeps them "pending" at the loop header on every iteration and,
    // unable to count how many prefetch loads were issued since, emits `s_waitcnt vmcnt(0)` in front of the epilogue --
    // draining the just-issued prefetch loads of the next strip on EVERY strip (load, store and MFMA phases add up
    // instead of overlapping: tools/ablate_conv.py).  An empty asm use forces the one wait to happen before the loop.
    // ZC > 0: the transposed conv's bias reaches the output through every tap whose up-sampled pixel lies inside the image: the full
    // sum S joins the shift, the border rows / columns / corners subtract their missing taps (tb[co] = {R0, R2, C0, C2, T00, T02,
    // T20, T22, S}: sums over the taps of row dy = 0 / 2, column dx = 0 / 2, the four corner taps, all nine)
    float zb[ZC > 0 ? 8 : 1];
    if constexpr (ZC > 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) zb[k] = q.tb[col * 9 + k];
        e_shift[0] += q.tb[col * 9 + 8] * e_scale[0];
#pragma unroll
        for (int k = 0; k < 8; ++k) asm volatile("" : : "v"(zb[k]));
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) asm volatile("" : : "v"(e_scale[nb]), "v"(e_shift[nb]));
    const act_t* const act = reinterpret_cast<const act_t*>(q.act);
    act_t* const outp = reinterpret_cast<act_t*>(q.out.ptr);
    const int64_t o_bs = q.out.bstride, o_cs = q.out.cstride, a_bs = q.act_bstride, a_cs = q.act_cstride;
    const int o_rs = q.out.rstride, a_rs = q.act_rstride;

    // deferred epilogue: the results of strip t are stored while strip t+1 is in its MFMA phase
    f32x4 pacc[4][NB];
    int eb = 0, ey0 = 0, ex0 = 0;
    bool have_prev = false;
    // x offset (inside the 32-px strip row) of the four consecutive pixels a lane holds for unit u
    auto xu = [&](int u) { return P2 ? 8 * lk + 4 * (u & 1) : (u & 1) * 16 + 4 * lk; };
    auto epilogue = [&]() {
        // lane holds (co = nb*8+col, y = ey0 + 2*(u>>1) + s_row, x = ex0 + xu(u) + r), r = 0..3
        if (ey0 >= p.H) return;
        constexpr bool POOLB = MODE == MODE_DGRAD && EPI == EPI_POOLBWD;   // p.pool, as a compile-time property
        if constexpr (N16) {
            // lane holds (co = li, y = ey0 + r, x = ex0 + h*16 + 4*lk + e) in pacc[r][h][e]
            const float sc = e_scale[0], sh = e_shift[0];
            const bool vec = p.vec_ok && (ey0 + 4 <= p.H) && (ex0 + TW <= p.W);
            if (POOLB) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int y = ey0 + r, x = ex0 + h * 16 + 4 * lk;
                        if (y >= p.H || x >= p.W) continue;
                        const f32x4 v = pacc[r][h];
                        const act_t* a0 = act + eb * a_bs + li * a_cs + (int64_t)(2 * y) * a_rs + 2 * x;
                        act_t* o0 = outp + eb * o_bs + li * o_cs + (int64_t)(2 * y) * o_rs + 2 * x;
                        if (vec) {
                            f32x4 A[2][2], O[2][2];
#pragma unroll
                            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                                for (int hh = 0; hh < 2; ++hh) {
                                    A[rr][hh] = pc_ld4(a0 + rr * a_rs + 4 * hh);
                                    O[rr][hh] = pc_ld4(o0 + rr * o_rs + 4 * hh);
                                }
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int hh = e >> 1, c = (e & 1) * 2;
                                const float w00 = A[0][hh][c], w01 = A[0][hh][c + 1], w10 = A[1][hh][c], w11 = A[1][hh][c + 1];
                                int am = 0;
                                float m = w00;
                                if (w01 > m) { m = w01; am = 1; }
                                if (w10 > m) { m = w10; am = 2; }
                                if (w11 > m) { m = w11; am = 3; }
                                const float g = m > 0.f ? v[e] * sc : 0.f;
                                O[0][hh][c] += am == 0 ? g : 0.f;
                                O[0][hh][c + 1] += am == 1 ? g : 0.f;
                                O[1][hh][c] += am == 2 ? g : 0.f;
                                O[1][hh][c + 1] += am == 3 ? g : 0.f;
                            }
#pragma unroll
                            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                                for (int hh = 0; hh < 2; ++hh) pc_st4(o0 + rr * o_rs + 4 * hh, O[rr][hh]);
                        } else {
                            const act_t* a1 = a0 + a_rs;
                            act_t* o1 = o0 + o_rs;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if (x + e >= p.W) continue;
                                const float w00 = pc_ld1(a0 + 2 * e), w01 = pc_ld1(a0 + 2 * e + 1), w10 = pc_ld1(a1 + 2 * e), w11 = pc_ld1(a1 + 2 * e + 1);
                                int am = 0;
                                float m = w00;
                                if (w01 > m) { m = w01; am = 1; }
                                if (w10 > m) { m = w10; am = 2; }
                                if (w11 > m) { m = w11; am = 3; }
                                const float g = m > 0.f ? v[e] * sc : 0.f;
                                pc_st1(o0 + 2 * e, pc_ld1(o0 + 2 * e) + (am == 0 ? g : 0.f));
                                pc_st1(o0 + 2 * e + 1, pc_ld1(o0 + 2 * e + 1) + (am == 1 ? g : 0.f));
                                pc_st1(o1 + 2 * e, pc_ld1(o1 + 2 * e) + (am == 2 ? g : 0.f));
                                pc_st1(o1 + 2 * e + 1, pc_ld1(o1 + 2 * e + 1) + (am == 3 ? g : 0.f));
                            }
                        }
                    }
                return;
            }
#pragma unroll
            for (int rp = 0; rp < 2; ++rp)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4 vv[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const int r = 2 * rp + s, y = ey0 + r, x = ex0 + h * 16 + 4 * lk;
                        f32x4 v = pacc[r][h];
                        vv[s] = v;
                        if (y >= p.H || x >= p.W) continue;
                        act_t* op = outp + eb * o_bs + li * o_cs + (int64_t)y * o_rs + x;
                        const act_t* ap = act ? act + eb * a_bs + li * a_cs + (int64_t)y * a_rs + x : nullptr;
                        if (vec) {
                            if (MODE == MODE_FWD) {
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const float o = v[e] * sc + sh;
                                    v[e] = p.relu ? fmaxf(o, 0.f) : o;
                                }
                            } else {
                                if (ap) {
                                    const f32x4 a4 = pc_ld4(ap);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] = a4[e] > 0.f ? v[e] * sc : 0.f;
                                }
                                if (p.accumulate) {
                                    const f32x4 o4 = pc_ld4(op);
#pragma unroll
                                    for (int e = 0; e < 4; ++e) v[e] += o4[e];
                                }
                            }
                            pc_st4(op, v);
                            vv[s] = v;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                if (x + e >= p.W) continue;
                                float o = v[e];
                                if (MODE == MODE_FWD) {
                                    o = o * sc + sh;
                                    o = p.relu ? fmaxf(o, 0.f) : o;
                                } else {
                                    if (ap) o = pc_ld1(ap + e) > 0.f ? o * sc : 0.f;
                                    if (p.accumulate) o += pc_ld1(op + e);
                                }
                                pc_st1(op + e, o);
                            }
                        }
                    }
                    if (EPI == EPI_POOL && MODE == MODE_FWD && q.pool_out.ptr && vec) {
                        // MaxPool2d(2): both rows of the pair and both x of a pair are in the lane
                        act_t* pp = reinterpret_cast<act_t*>(q.pool_out.ptr) + eb * q.pool_out.bstride + li * q.pool_out.cstride +
                                    (int64_t)((ey0 >> 1) + rp) * q.pool_out.rstride + (ex0 >> 1) + h * 8 + 2 * lk;
                        pc_st2(pp, fmaxf(fmaxf(vv[0][0], vv[0][1]), fmaxf(vv[1][0], vv[1][1])),
                               fmaxf(fmaxf(vv[0][2], vv[0][3]), fmaxf(vv[1][2], vv[1][3])));
                    }
                }
            return;
        }
        if (POOLB && p.vec_ok && (ey0 + 4 <= p.H) && (ex0 + TW <= p.W)) {
            // MaxPool2d(2) backward on an interior strip of aligned tensors: the lane's four pooled pixels cover 8 x 2
            // full-resolution pixels = two 16-byte pieces per row of `act` and of the accumulated output (the scalar path
            // below issues 12 four-byte accesses per pooled pixel; these two launches were 127 us of the step)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int y = ey0 + 2 * (u >> 1) + s_row, x = ex0 + xu(u);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int co = nb * 8 + col;
                    const f32x4 v = pacc[u][nb];
                    const act_t* a0 = act + eb * a_bs + co * a_cs + (int64_t)(2 * y) * a_rs + 2 * x;
                    act_t* o0 = outp + eb * o_bs + co * o_cs + (int64_t)(2 * y) * o_rs + 2 * x;
                    f32x4 A[2][2], O[2][2];
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            A[rr][h] = pc_ld4(a0 + rr * a_rs + 4 * h);
                            O[rr][h] = pc_ld4(o0 + rr * o_rs + 4 * h);
                        }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int h = r >> 1, e = (r & 1) * 2;
                        const float w00 = A[0][h][e], w01 = A[0][h][e + 1], w10 = A[1][h][e], w11 = A[1][h][e + 1];
                        int am = 0;
                        float m = w00;
                        if (w01 > m) { m = w01; am = 1; }
                        if (w10 > m) { m = w10; am = 2; }
                        if (w11 > m) { m = w11; am = 3; }
                        const float g = m > 0.f ? v[r] * e_scale[nb] : 0.f;
                        O[0][h][e] += am == 0 ? g : 0.f;
                        O[0][h][e + 1] += am == 1 ? g : 0.f;
                        O[1][h][e] += am == 2 ? g : 0.f;
                        O[1][h][e + 1] += am == 3 ? g : 0.f;
                    }
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int h = 0; h < 2; ++h) pc_st4(o0 + rr * o_rs + 4 * h, O[rr][h]);
                }
            }
            return;
        }
        const bool full = !POOLB && p.vec_ok && (ey0 + 4 <= p.H) && (ex0 + TW <= p.W);
        if (full) {
            // interior strip, aligned tensors: no bounds checks, 16-byte accesses only
            act_t* ob = outp + eb * o_bs + col * o_cs + (int64_t)(ey0 + s_row) * o_rs + ex0;
            const act_t* ab = act ? act + eb * a_bs + col * a_cs + (int64_t)(ey0 + s_row) * a_rs + ex0 : nullptr;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    f32x4 v = pacc[u][nb];
                    act_t* op = ob + nb * 8 * o_cs + (int64_t)((u >> 1) * 2) * o_rs + xu(u);
                    if (MODE == MODE_FWD) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float o = v[r] * e_scale[nb] + e_shift[nb];
                            v[r] = p.relu ? fmaxf(o, 0.f) : o;
                        }
                    } else {
                        if (ab) {
                            const f32x4 a4 = pc_ld4(ab + nb * 8 * a_cs + (int64_t)((u >> 1) * 2) * a_rs + xu(u));
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] = a4[r] > 0.f ? v[r] * e_scale[nb] : 0.f;
                        }
                        if (p.accumulate) {
                            const f32x4 o4 = pc_ld4(op);
#pragma unroll
                            for (int r = 0; r < 4; ++r) v[r] += o4[r];
                        }
                    }
                    if (EPI == EPI_DOT && MODE == MODE_FWD && q.dot_w) {
                        // sum over the 8 channels = the 8 lanes `col` of a 16-lane group half; lane col == 0 stores
                        const float wl = q.dot_w[nb * 8 + col];
                        f32x4 t;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            t[r] = pc_sum8(__fmul_rn(v[r], wl));      // (rounded product: as `v * wl + dpp(..)` the first step contracts into an fma)
                        }
                        if (col == 0)
                            *reinterpret_cast<f32x4*>(q.dot_out.ptr + eb * q.dot_out.bstride +
                                                      (int64_t)(ey0 + s_row + (u >> 1) * 2) * q.dot_out.rstride + ex0 + xu(u)) = t;
                        continue;
                    }
                    pc_st4(op, v);
                    if (EPI == EPI_POOL && MODE == MODE_FWD && q.pool_out.ptr) {
                        // MaxPool2d(2): the x pairs are in the lane, the row pair (s_row 0 / 1) sits 8 lanes apart
                        float m0 = fmaxf(v[0], v[1]), m1 = fmaxf(v[2], v[3]);
                        m0 = fmaxf(m0, pc_lane_xor8(m0));
                        m1 = fmaxf(m1, pc_lane_xor8(m1));
                        if (s_row == 0) {
                            act_t* pp = reinterpret_cast<act_t*>(q.pool_out.ptr) + eb * q.pool_out.bstride + (nb * 8 + col) * q.pool_out.cstride +
                                        (int64_t)((ey0 >> 1) + (u >> 1)) * q.pool_out.rstride + (ex0 >> 1) + (xu(u) >> 1);
                            pc_st2(pp, m0, m1);
                        }
                    }
                }
            return;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int y = ey0 + 2 * (u >> 1) + s_row;
            const int x = ex0 + xu(u);
            if (y >= p.H || x >= p.W) continue;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int co = nb * 8 + col;
                const f32x4 v = pacc[u][nb];
                if (MODE == MODE_FWD) {
                    if (EPI == EPI_DOT && q.dot_w) {
                        // partial strip (ragged width / height): the 1x1 partial logit per element; the 8 lanes `col` of a group hold
                        // the same pixels, so they are active together and the cross-lane sum is complete
                        const float wl = q.dot_w[co];
                        float* dp = q.dot_out.ptr + eb * q.dot_out.bstride + (int64_t)y * q.dot_out.rstride + x;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float o = v[r] * e_scale[nb] + e_shift[nb];
                            float t = __fmul_rn(p.relu ? fmaxf(o, 0.f) : o, wl);
                            t = pc_sum8(t);
                            if (col == 0 && x + r < p.W) dp[r] = t;
                        }
                        continue;
                    }
                    act_t* op = outp + eb * o_bs + co * o_cs + (int64_t)y * o_rs + x;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float o = v[r] * e_scale[nb] + e_shift[nb];
                        if (x + r < p.W) pc_st1(op + r, p.relu ? fmaxf(o, 0.f) : o);
                    }
                } else if (!POOLB) {
                    act_t* op = outp + eb * o_bs + co * o_cs + (int64_t)y * o_rs + x;
                    const act_t* ap = act ? act + eb * a_bs + co * a_cs + (int64_t)y * a_rs + x : nullptr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (x + r < p.W) {
                            float o = v[r];
                            if (ap) o = pc_ld1(ap + r) > 0.f ? o * e_scale[nb] : 0.f;
                            if (p.accumulate) o += pc_ld1(op + r);
                            pc_st1(op + r, o);
                        }
                    }
                } else {
                    // MaxPool2d(2) backward: (y,x) is a pooled coordinate; route to the first arg-max of the window.
                    const act_t* a0 = act + eb * a_bs + co * a_cs + (int64_t)(2 * y) * a_rs;
                    const act_t* a1 = a0 + a_rs;
                    act_t* o0 = outp + eb * o_bs + co * o_cs + (int64_t)(2 * y) * o_rs;
                    act_t* o1 = o0 + o_rs;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int xx = x + r;
                        if (xx < p.W) {
                            const float w00 = pc_ld1(a0 + 2 * xx), w01 = pc_ld1(a0 + 2 * xx + 1), w10 = pc_ld1(a1 + 2 * xx), w11 = pc_ld1(a1 + 2 * xx + 1);
                            int am = 0;
                            float m = w00;
                            if (w01 > m) { m = w01; am = 1; }
                            if (w10 > m) { m = w10; am = 2; }
                            if (w11 > m) { m = w11; am = 3; }
                            const float g = m > 0.f ? v[r] * e_scale[nb] : 0.f;
                            pc_st1(o0 + 2 * xx, pc_ld1(o0 + 2 * xx) + (am == 0 ? g : 0.f));
                            pc_st1(o0 + 2 * xx + 1, pc_ld1(o0 + 2 * xx + 1) + (am == 1 ? g : 0.f));
                            pc_st1(o1 + 2 * xx, pc_ld1(o1 + 2 * xx) + (am == 2 ? g : 0.f));
                            pc_st1(o1 + 2 * xx + 1, pc_ld1(o1 + 2 * xx + 1) + (am == 3 ? g : 0.f));
                        }
                    }
                }
            }
        }
    };

    f32x4 acc[4][NB];
    for (int stage = 0; stage < nstages; ++stage) {
        const int ch = stage % NST;
        if (!(dbg & 1)) {
            if (ZC > 0 && pend_z) commit_z(y0, x0);
            else if (STAGED) commit();
            else load_generic(ch, b, y0, x0);
        }
        int nb_ = b, ny0 = y0, nx0 = x0;
        if (stage + 1 < nstages) {
            const int nch = (stage + 1) % NST;
            if (nch == 0) strip_coords(stage + 1, nb_, ny0, nx0);
            if (STAGED && !(dbg & 1)) {
                if (ZC > 0 && nch >= NCHUNK) { issue_z(nch - NCHUNK, nb_, ny0, nx0); pend_z = true; }
                else { issue(nch, nb_, ny0, nx0); pend_z = false; }
            }
        }
        if (have_prev) {
            if (!(dbg & 4)) epilogue();
            have_prev = false;
        }
        if (ch == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[u][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (ZC > 0 && ch >= NCHUNK) {
            if constexpr (ZC > 0) {
                if (!(dbg & 2)) {
                    // composed stage: B[k = low-res row lk][n = (s, co)] of (channel ci, column tap tj, x parity j) = register 4 ci + 2 tj + j
                    // K-slot q = 4 m + lk (m = 0..5) = (channel q / 3, low-res row q % 3 of the pair's three): 24 (channel, row) slots in
                    // 6 MFMAs per (column tap tj, x parity j, row pair) = 48 per stage (one K-slot per row with a 4th unused slot took 64);
                    // the two slots a 32-lane half reads together are 16 banks apart
                    const float* wzl = wzimg + (ch - NCHUNK) * 64 * WZ_L + lane * WZ_L;
                    const float* zl = wl + li;                              // A: column li + tj + j of (channel, row) slot lk of step m
#pragma unroll
                    for (int m = 0; m < 6; ++m) {
                        const int qs = 4 * m + lk, zci = qs / 3, zv_ = qs - 3 * zci;
                        const f32x4 bz = *reinterpret_cast<const f32x4*>(wzl + 4 * m);        // [2 tj + j] of this step
                        float zv[2][3];
#pragma unroll
                        for (int rp = 0; rp < 2; ++rp)
#pragma unroll
                            for (int c3 = 0; c3 < 3; ++c3) zv[rp][c3] = zl[zci * ZCH + (rp + zv_) * ZROW + c3];
#pragma unroll
                        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int rp = 0; rp < 2; ++rp)
                                    acc[rp * 2 + j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(zv[rp][tj + j], bz[2 * tj + j], acc[rp * 2 + j][0], 0, 0, 0);
                    }
                }
            }
        } else if (!(dbg & 2)) {
            load_bw(ch);                    // re-read every stage, also when CIN == CHUNK: not live across the epilogue
            const float* lrow = wl + lk * RS + (COL0 - 1) + li;
            if constexpr (P2) {
                // lane (li, lk): input row 2 rp + lk, columns 2 + 2 li .. 7 + 2 li (three aligned b64) = pixels x0 - 2 + 2 li ..;
                // operand of (j, dx) = pixel x0 - 1 + 2 li + j + dx = element 1 + j + dx of the six
                const float* l2 = wl + lk * LROW + 2 + 2 * li;
#pragma unroll
                for (int ci = 0; ci < CHUNK; ++ci) {
#pragma unroll
                    for (int rp = 0; rp < 2; ++rp) {
                        const float* src = l2 + ci * LCH + rp * 2 * LROW;
                        const float2 q0 = *reinterpret_cast<const float2*>(src), q1 = *reinterpret_cast<const float2*>(src + 2),
                                     q2 = *reinterpret_cast<const float2*>(src + 4);
                        const float sv[4] = {q0.y, q1.x, q1.y, q2.x};
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
#pragma unroll
                                for (int nb = 0; nb < NB; ++nb)
                                    acc[rp * 2 + j][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[j + dx], bw[ci][dx][nb], acc[rp * 2 + j][nb], 0, 0, 0);
                    }
                }
            } else if constexpr (N16) {
                // acc[r][h]: output row y0 + r, x half h, channel li
                const float* l16 = wl + (COL0 - 1) + li;
#pragma unroll
                for (int m = 0; m < 18; ++m) {
                    float av[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) av[u] = l16[aoff16[m] + (u >> 1) * RS + (u & 1) * 16];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        acc[u >> 1][u & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bw[m / 6][(m % 6) / 2][m % 2], acc[u >> 1][u & 1], 0, 0, 0);
                }
            } else
#pragma unroll
            for (int ci = 0; ci < CHUNK; ++ci) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    float av[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) av[u] = lrow[ci * CSW + (u >> 1) * 2 * RS + (u & 1) * 16 + dx];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[u][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bw[ci][dx][nb], acc[u][nb], 0, 0, 0);
                }
            }
        }
        if (ch == NST - 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if constexpr (P2) {
                        // acc[rp*2 + j][nb][r] = pixel 2 (4 lk + r) + j  ->  pacc[rp*2 + h][nb][e] = pixel 8 lk + 4 h + e
                        const int rp = u >> 1, h = u & 1;
                        const f32x4 a0 = acc[rp * 2][nb], a1 = acc[rp * 2 + 1][nb];
                        pacc[u][nb] = f32x4{a0[2 * h], a1[2 * h], a0[2 * h + 1], a1[2 * h + 1]};
                        if constexpr (ZC > 0) {
                            // border pixels: the taps whose up-sampled pixel falls outside the image carry no bias
                            const int Y = y0 + 2 * rp + s_row, X0 = x0 + 8 * lk + 4 * h;
                            const bool top = Y == 0, bot = Y == p.H - 1;
                            const float rowt = top ? zb[0] : (bot ? zb[1] : 0.f);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const bool lft = X0 + e == 0, rgt = X0 + e == p.W - 1;
                                float c = rowt + (lft ? zb[2] : (rgt ? zb[3] : 0.f));
                                c -= top ? (lft ? zb[4] : (rgt ? zb[5] : 0.f)) : (bot ? (lft ? zb[6] : (rgt ? zb[7] : 0.f)) : 0.f);
                                pacc[u][nb][e] -= c;
                            }
                        }
                    } else {
                        pacc[u][nb] = acc[u][nb];
                    }
                }
            eb = b; ey0 = y0; ex0 = x0;
            have_prev = true;
        }
        b = nb_; y0 = ny0; x0 = nx0;
    }
    if (have_prev && !(dbg & 4)) epilogue();
#ifdef POPCORN_CONV_ABLATE
    if (p.ts && tid == 0) p.ts[8 * (blockIdx.y * gridDim.x + blockIdx.x) + 1] = wall_clock64();
#endif
}

// Persistent workgroups, all resident at once (one wave of a 256-thread workgroup per SIMD; the register count decides how many
// workgroups a CU holds), split over the grouped problems -- or the grid pc_debug_conv forces
int conv_grid(const ConvArgs& p, int resident, int nprob) {
    return pc_balanced_grid(p.ntiles, g_conv_max_grid > 0 ? g_conv_max_grid : resident / nprob);
}

// The epilogue instantiation of a forward launch, from what its problems ask for: EPI_POOL (layers with >= 8 inputs in front of a Down
// block: inc.conv.3, down1 conv.3), EPI_DOT (8 -> 8: up1.conv.3, the layer in front of the 1x1 out-conv), EPI_UPT (8 -> 8, channels-last
// bf16: all problems of the launch or none), else EPI_NONE; -1 = an invalid mix
template <int CIN, int COUT>
int conv_fwd_epi(const ConvArgs& p, int nprob) {
    int npo = 0, ndot = 0, nupt = 0;
    for (int i = 0; i < nprob; ++i) {
        npo += p.pr[i].pool_out.ptr != nullptr;
        ndot += p.pr[i].dot_w != nullptr;
        nupt += p.pr[i].upt_w != nullptr;
    }
    if (CIN >= 8 && npo) return EPI_POOL;
    if (CIN == 8 && COUT == 8 && ndot) return EPI_DOT;
    if (CIN == 8 && COUT == 8 && nupt) return nupt == nprob ? EPI_UPT : -1;
    return EPI_NONE;
}

// tile geometry of a launch and the hooks of pc_debug_conv*; false = an empty domain, nothing to launch
bool conv_fill_geometry(ConvArgs& p) {
    p.tiles_x = (p.W + TW - 1) / TW;
    p.tiles_y = (p.H + TH - 1) / TH;
    p.ntiles = p.B * p.tiles_x * p.tiles_y;
    if (p.ntiles <= 0) return false;
    p.div_tx = pc_make_fastdiv(p.tiles_x);
    p.div_tpi = pc_make_fastdiv(p.tiles_x * p.tiles_y);
    p.dbg = g_conv_dbg;
    p.ts = g_conv_ts;
    return true;
}

template <int CIN, int COUT, int MODE, int LD, int EPI, int ZC = 0>
int launch_conv_po(ConvArgs& p, int nprob, hipStream_t stream) {
    constexpr int CHUNK = CIN < 8 ? CIN : 8;       // 8 channels per LDS stage: 36 KB per workgroup, 4 workgroups per CU
    constexpr bool N16 = COUT == 16 && CHUNK == 8;
    constexpr bool P2 = ZC > 0 && !N16 && CHUNK == 8;
    const size_t lds = ((size_t)4 * (P2 ? SROWS * (8 * 40 + 32) : CHUNK * CSW) + (N16 ? 16 * (CIN * 9 + 1) : 4 * (COUT * (CIN * 3 + 4) + 16)) +
                        (ZC / 8) * 64 * 28) * sizeof(float);   // wave strips + weight image (+ composed weight image)
    static pc_launch_setup setup;
    const hipError_t e = setup(reinterpret_cast<const void*>(&conv3x3_mfma_kernel<CIN, COUT, MODE, LD, EPI, ZC>), lds,
                               PC_SETUP_LDS | PC_SETUP_PROBE, __PRETTY_FUNCTION__);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((conv3x3_mfma_kernel<CIN, COUT, MODE, LD, EPI, ZC>), dim3(conv_grid(p, setup.resident, nprob), nprob), dim3(256), lds,
                       stream, p);
    PC_CHECK_LAUNCH();
    return 0;
}

#include "conv3x3_fwd_s3.h"
#include "conv3x3_cl.h"

template <int CIN, int COUT, int MODE, int LD>
int launch_conv_ld(ConvArgs& p, int nprob, hipStream_t stream) {
    if constexpr (MODE == MODE_DGRAD) {
        // the pool-backward epilogues live in their own instantiation: in the plain one they cost a wave per SIMD
        return p.pool ? launch_conv_po<CIN, COUT, MODE, LD, EPI_POOLBWD>(p, nprob, stream) : launch_conv_po<CIN, COUT, MODE, LD, EPI_NONE>(p, nprob, stream);
    } else {
        const int epi = conv_fwd_epi<CIN, COUT>(p, nprob);
        if constexpr (LD == LD_DIRECT && (CIN == 8 || CIN == 16) && (COUT == 8 || COUT == 16)) {
            // split-operand form (conv3x3_fwd_s3.h): every 8- / 16-channel layer whose tensors are aligned
            if (fwd_s3_ok<CIN, COUT>(p, nprob, 0)) {
                if constexpr (CIN == 8 && COUT == 8) {
                    if (epi == EPI_DOT) return launch_fwd_s3<CIN, COUT, EPI_DOT, 0>(p, nprob, stream);
                }
                if (epi == EPI_POOL) return launch_fwd_s3<CIN, COUT, EPI_POOL, 0>(p, nprob, stream);
                if (epi == EPI_NONE) return launch_fwd_s3<CIN, COUT, EPI_NONE, 0>(p, nprob, stream);
            }
        }
        if constexpr (CIN >= 8) {
            if (epi == EPI_POOL) return launch_conv_po<CIN, COUT, MODE, LD, EPI_POOL>(p, nprob, stream);
        }
        if constexpr (CIN == 8 && COUT == 8) {
            if (epi == EPI_DOT) return launch_conv_po<CIN, COUT, MODE, LD, EPI_DOT>(p, nprob, stream);
        }
        if (epi != EPI_NONE) return PC_EINVAL;              // (EPI_UPT: channels-last bf16 only)
        return launch_conv_po<CIN, COUT, MODE, LD, EPI_NONE>(p, nprob, stream);
    }
}

// staged-loader classification of a planar fp32 source (1 = aligned DIRECT, 2 = aligned POOL2, 0 = generic)
int conv_src_mode(const pc_src& s, int H, int W) {
    if (s.C == 0) return 0;
    const bool al = ((reinterpret_cast<uintptr_t>(s.ptr) & 15) == 0) && (s.rstride % 4 == 0) && (s.cstride % 4 == 0) && (s.bstride % 4 == 0);
    if (!al) return 0;
    // (W % 4 != 0 is fine: the row stride is a multiple of 4, so every 16-byte segment that starts inside a row exists in
    // memory; the loader masks its tail per pixel.  POOL2 reads source columns 2 xg .. 2 xg + 7 of which only those below 2 W are
    // used: with 1 or 2 valid pixels in the last segment (W % 4 = 1, 2) the second 16-byte piece is not read at all, with 3
    // (W % 4 = 3) it ends at column 2 W + 1: the source row must then have at least 2 W + 2 floats.)
    // (a DIRECT source at the origin that ends before the conv domain does is zero beyond its extent: the loader masks per source)
    if (s.mode == PC_SRC_DIRECT && s.oy == 0 && s.ox == 0 && s.H <= H && s.W <= W && s.H >= 1 && s.W >= 1) return 1;
    if (s.mode == PC_SRC_POOL2 && s.W == 2 * W && s.H >= 2 * H && ((W % 4) != 3 || s.rstride >= 2 * W + 2)) return 2;
    return 0;
}

bool same_layout(const pc_src& a, const pc_src& b) { return b.C == 0 || (a.bstride == b.bstride && a.rstride == b.rstride); }

template <int CIN, int COUT, int MODE>
int launch_conv(ConvArgs& p, int nprob, hipStream_t stream) {
    constexpr int CHUNK = CIN < 8 ? CIN : 8;       // 8 channels per LDS stage: 36 KB per workgroup, 4 workgroups per CU
    if (!conv_fill_geometry(p)) return 0;
    if (g_pc_precision == PC_PREC_BF16) return launch_conv_bf16<CIN, COUT, MODE>(p, nprob, stream);
    // loader choice: all problems of the group must qualify for a staged loader
    bool direct = true, pool = CHUNK >= 8, reflect = true;      // DIRECT also for the 2 / 4-channel first layers (pre-padded input)
    bool vec = true;      // (any width: the vector epilogues only take strips that lie completely inside the image; a ragged last strip
                          // of a row takes the per-element path)
    // fp32 mode: planar fp32 tensors everywhere
    const uintptr_t amask = 15;                        // a 4-pixel vector access: 16 bytes
    for (int i = 0; i < nprob; ++i) {
        ConvProb& q = p.pr[i];
        if (q.a.dtype != PC_F32 || !pc_planar(q.a) || (q.b.C && (q.b.dtype != PC_F32 || !pc_planar(q.b)))) return PC_EINVAL;
        if ((q.out.ptr != reinterpret_cast<float*>(q.dot_out.ptr) && (q.out.dtype != PC_F32 || !pc_planar(q.out))) ||
            (q.pool_out.ptr && (q.pool_out.dtype != PC_F32 || !pc_planar(q.pool_out))) ||
            (q.dot_out.ptr && (q.dot_out.dtype != PC_F32 || !pc_planar(q.dot_out))) || (q.act && (q.act_dtype != PC_F32 || q.act_xstride > 1)))
            return PC_EINVAL;
        q.fast_a = conv_src_mode(q.a, p.H, p.W);
        q.fast_b = conv_src_mode(q.b, p.H, p.W);
        const bool lay = same_layout(q.a, q.b);
        direct = direct && q.fast_a == 1 && (q.b.C == 0 || q.fast_b == 1) && lay && (CIN <= 16 || q.a.C == 16);
        pool = pool && q.fast_a == 2 && q.b.C == 0;
        vec = vec && (q.out.rstride % 4 == 0) && (q.out.cstride % 4 == 0) && (q.out.bstride % 4 == 0) &&
              ((reinterpret_cast<uintptr_t>(q.out.ptr) & amask) == 0);
        if (q.act) vec = vec && (q.act_rstride % 4 == 0) && (q.act_cstride % 4 == 0) && (q.act_bstride % 4 == 0) &&
                         ((reinterpret_cast<uintptr_t>(q.act) & amask) == 0);
        reflect = reflect && q.a.mode == PC_SRC_REFLECT && q.b.C == 0;
    }
    p.vec_ok = vec ? 1 : 0;
    if (direct) return launch_conv_ld<CIN, COUT, MODE, LD_DIRECT>(p, nprob, stream);
    // (the gradient of a data-gradient launch is a plain DIRECT source, fill_dgrad: aligned or generic)
    if constexpr (MODE == MODE_FWD && CHUNK >= 8 && CIN <= 16) {
        if (pool) return launch_conv_ld<CIN, COUT, MODE, LD_POOL>(p, nprob, stream);
    }
    if constexpr (MODE == MODE_FWD && CIN <= 4) {
        if (reflect) return launch_conv_ld<CIN, COUT, MODE, LD_REFLECT>(p, nprob, stream);
    }
    return launch_conv_ld<CIN, COUT, MODE, LD_GENERIC>(p, nprob, stream);
}

// the (Cin, Cout) a caller can reach.  Forward: every layer shape of the network.  Data gradient: (Cin, Cout) = (Cg, Cn), Cg = the output
// width of a conv layer (8 or 16) -- a 2-, 4- or 32-channel gradient does not exist
template <int MODE>
int dispatch_conv(ConvArgs& p, int nprob, int Cin, int Cout, hipStream_t stream) {
#define PC_CASE(ci, co) \
    if (Cin == ci && Cout == co) return launch_conv<ci, co, MODE>(p, nprob, stream);
    if constexpr (MODE == MODE_FWD) {
        PC_CASE(2, 8) PC_CASE(4, 8) PC_CASE(32, 8)
    }
    PC_CASE(8, 8) PC_CASE(16, 8) PC_CASE(8, 16) PC_CASE(16, 16)
#undef PC_CASE
    return PC_EINVAL;
}

int fill_fwd(ConvProb& q, const pc_src* a, const pc_src* b, const float* w, const pc_bn* bn, const pc_dst* out, int Cin) {
    if (!a || !w || !bn) return PC_EINVAL;
    q.a = *a;
    if (b) q.b = *b;
    if (q.a.C + q.b.C != Cin) return PC_EINVAL;
    q.w = w;
    q.bn = *bn;
    if (out) q.out = *out;
    return 0;
}

int fill_dgrad(ConvProb& q, const pc_src* g, const float* w, int c0, const pc_src* act, const pc_bn* act_bn, int pool,
               const pc_dst* out, int Cg) {
    if (!g || !w || !out || g->C != Cg || g->mode != PC_SRC_DIRECT) return PC_EINVAL;
    if (pool && !act) return PC_EINVAL;
    q.a = *g;
    // forward weight w[cg][Cin_total][3][3]; as a conv over g producing input channel (c0 + co):
    //   weight(out = co, in = cg, tap) = w[cg][c0 + co][8 - tap]
    q.w = w + (int64_t)c0 * 9;
    if (act) {
        if (!act_bn) return PC_EINVAL;
        q.bn = *act_bn;
        q.act = act->ptr;
        q.act_bstride = act->bstride;
        q.act_cstride = act->cstride;
        q.act_rstride = act->rstride;
        q.act_dtype = act->dtype;
        q.act_xstride = act->xstride;
    }
    q.out = *out;
    return 0;
}

// the pooled second output needs every strip on the vector epilogue: full 32 x 4 strips, 16-byte aligned output
bool pool_out_geometry_ok(const pc_dst& out, int H, int W) {
    if (out.dtype == PC_BF16) return W % 32 == 0 && H % 4 == 0 && pc_cl_ok(out);      // channels-last bf16 (bf16 mode)
    return W % 32 == 0 && H % 4 == 0 && pc_planar(out) && out.rstride % 4 == 0 && out.cstride % 4 == 0 && out.bstride % 4 == 0 &&
           (reinterpret_cast<uintptr_t>(out.ptr) & 15) == 0;
}

}  // namespace

extern "C" int pc_conv3x3_pool_out_ok(const pc_dst* out, int H, int W) { return out && pool_out_geometry_ok(*out, H, W) ? 1 : 0; }

extern "C" int pc_conv3x3_bn_relu_fwd(const pc_src* a, const pc_src* b, const float* w, const pc_bn* bn, int relu,
                                      const pc_dst* out, int B, int H, int W, int Cin, int Cout, void* stream) {
    pc_conv_fwd_desc d{};
    d.a = a; d.b = b; d.w = w; d.bn = bn; d.out = out;
    return pc_conv3x3_bn_relu_fwd_group(1, &d, relu, B, H, W, Cin, Cout, stream);
}

extern "C" int pc_conv3x3_bn_relu_fwd_group(int n, const pc_conv_fwd_desc* d, int relu, int B, int H, int W, int Cin, int Cout,
                                            void* stream) {
    if (n < 1 || n > MAXG || !d) return PC_EINVAL;
    ConvArgs p{};
    for (int i = 0; i < n; ++i) {
        const int rc = fill_fwd(p.pr[i], d[i].a, d[i].b, d[i].w, d[i].bn, d[i].out, Cin);
        if (rc) return rc;
        if (d[i].upt_w) {
            // the transposed conv of the Up block that follows, in this launch's epilogue (channels-last bf16, 8 -> 8 layers)
            if (g_pc_precision != PC_PREC_BF16 || Cin != 8 || Cout != 8 || !relu || d[i].b || d[i].pool_out || d[i].dot_w || !d[i].upt_out ||
                !d[i].upt_out->ptr || !pc_cl_ok(*d[i].upt_out) || d[i].upt_out->xstride < 8 || d[i].a->mode != PC_SRC_DIRECT)
                return PC_EINVAL;
            p.pr[i].upt_w = d[i].upt_w;
            p.pr[i].upt_b = d[i].upt_b;
            p.pr[i].upt_out = *d[i].upt_out;
        }
        if (d[i].w_cin) {
            if (g_pc_precision != PC_PREC_BF16 || Cin != 8 || d[i].b || d[i].w_ci0 < 0 || d[i].w_cin < 1 || d[i].w_ci0 + d[i].w_cin > 8 ||
                d[i].a->mode != PC_SRC_DIRECT)
                return PC_EINVAL;
            p.pr[i].w_ci0 = d[i].w_ci0;
            p.pr[i].w_cin = d[i].w_cin;
        }
        if (d[i].dot_w) {
            // the partial 1x1 sum replaces the feature map.  bf16 mode: all strips must take the vector epilogue; fp32: any geometry
            // (partial strips take the per-element form), planar fp32 output
            const bool dot_geom = d[i].dot_out && (g_pc_precision == PC_PREC_BF16 ? pool_out_geometry_ok(*d[i].dot_out, H, W)
                                                                                  : (d[i].dot_out->dtype == PC_F32 && pc_planar(*d[i].dot_out)));
            if (!d[i].dot_out || !d[i].dot_out->ptr || Cin != 8 || Cout != 8 || !relu || d[i].pool_out || !dot_geom)
                return PC_EINVAL;
            p.pr[i].dot_w = d[i].dot_w;
            p.pr[i].dot_out = *d[i].dot_out;
            if (!d[i].out) p.pr[i].out = *d[i].dot_out;     // keeps the alignment checks of the launcher meaningful
        } else if (!d[i].out) {
            return PC_EINVAL;
        }
        if (d[i].pool_out) {
            const pc_dst& po = *d[i].pool_out;
            const bool po_ok = po.dtype == PC_BF16 ? pc_cl_ok(po)
                                                   : (po.rstride % 2 == 0 && po.cstride % 2 == 0 && po.bstride % 2 == 0 &&
                                                      (reinterpret_cast<uintptr_t>(po.ptr) & 7) == 0 && pc_planar(po));
            if (Cin < 8 || !pool_out_geometry_ok(*d[i].out, H, W) || !po.ptr || !po_ok) return PC_EINVAL;
            p.pr[i].pool_out = po;
        }
    }
    p.w_co_stride = Cin * 9;
    p.w_ci_stride = 9;
    p.relu = relu;
    p.B = B; p.H = H; p.W = W;
    return dispatch_conv<MODE_FWD>(p, n, Cin, Cout, (hipStream_t)stream);
}

extern "C" int pc_conv3x3_dgrad(const pc_src* g, const float* w, int Cin_total, int c0, int Cn,
                                const pc_src* act, const pc_bn* act_bn, int pool, int accumulate,
                                const pc_dst* out, int B, int H, int W, int Cg, void* stream) {
    const pc_conv_dgrad_desc d{g, w, act, act_bn, out};
    return pc_conv3x3_dgrad_group(1, &d, Cin_total, c0, Cn, pool, accumulate, B, H, W, Cg, stream);
}

extern "C" int pc_conv3x3_dgrad_group(int n, const pc_conv_dgrad_desc* d, int Cin_total, int c0, int Cn, int pool,
                                      int accumulate, int B, int H, int W, int Cg, void* stream) {
    if (n < 1 || n > MAXG || !d) return PC_EINVAL;
    ConvArgs p{};
    for (int i = 0; i < n; ++i) {
        const int rc = fill_dgrad(p.pr[i], d[i].g, d[i].w, c0, d[i].act, d[i].act_bn, pool, d[i].out, Cg);
        if (rc) return rc;         // (act is a per-problem property: the masked skip block and the plain up block of a concat layer mix)
    }
    p.w_co_stride = 9;
    p.w_ci_stride = Cin_total * 9;
    p.w_flip = 1;
    p.pool = pool;
    p.accumulate = accumulate;
    p.B = B; p.H = H; p.W = W;
    return dispatch_conv<MODE_DGRAD>(p, n, Cg, Cn, (hipStream_t)stream);
}

#include "conv3x3_up.h"
