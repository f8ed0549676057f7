// conv3x3_args.h -- launch arguments and strip geometry shared by the conv kernels of conv3x3.hip (the planar fp32 kernel there,
// conv3x3_fwd_s3.h, conv3x3_cl.h, conv3x3_up.h); included by conv3x3.hip inside its anonymous namespace.

constexpr int TW = 32, TH = 16;          // output tile
constexpr int RS = 48;                   // LDS row stride  (== 16 mod 32)
constexpr int COL0 = 4;                  // LDS column of tile x0 (left halo at COL0-1): keeps float4 stores aligned
constexpr int MAXG = PC_MAX_GROUP;       // problems per launch

enum { MODE_FWD = 0, MODE_DGRAD = 1 };
enum { LD_GENERIC = 0, LD_DIRECT = 1, LD_POOL = 2, LD_REFLECT = 3 };

struct ConvProb {
    pc_src a, b;          // input sources (channels a.C then b.C)
    const float* w;       // weights
    pc_bn bn;             // FWD: this layer's BN; DGRAD: BN of the layer that produced `act`
    const float* act;     // DGRAD: post-ReLU activations of the producer (NULL = plain)
    int64_t act_bstride, act_cstride;
    int act_rstride;
    int act_dtype;
    int act_xstride;
    int fast_a, fast_b;   // pc_src_fast_mode of the two sources (generic loader)
    pc_dst out;
    pc_dst pool_out;      // FWD: 2x2-max-pooled copy of the output (ptr NULL = not wanted)
    const float* dot_w;   // FWD (EPI_DOT): weights of a following 1x1 conv over this layer's 8 channels ...
    pc_dst dot_out;       // ... whose partial sum replaces the output (ptr NULL = ordinary output)
    // FWD with ZC > 0 (pc_conv3x3_up_fwd_group): the up-sampled half of an Up block's concatenated input, never materialised --
    // z is the LOW-resolution map (ZC channels, H/2 x W/2) the transposed conv would have up-sampled; wz / tb come from
    // compose_up_kernel (composed 2x2-neighbourhood weights per output parity; bias-through-the-taps table)
    const float* z; int64_t z_bs, z_cs; int z_rs;
    const float* wz; const float* tb;
    // channels-last bf16, CIN == 8: w is [COUT][w_cin][3][3] over input channels [w_ci0, w_ci0 + w_cin) (w_cin == 0: full weight)
    int w_ci0, w_cin;
    // EPI_UPT: the ConvTranspose2d(8, 8, 2, stride 2) that consumes this layer's output (Up.up, networks.py:302-306), applied in the
    // epilogue: upt_out = (B, 8, 2H, 2W) channels-last bf16
    const float* upt_w; const float* upt_b;
    pc_dst upt_out;
};

struct ConvArgs {
    ConvProb pr[MAXG];
    int w_co_stride;      // element stride between output channels in w
    int w_ci_stride;      // element stride between input channels in w
    int w_flip;           // 1: tap index 8 - t (dgrad)
    int relu;             // FWD
    int pool;             // DGRAD: max-pool backward scatter into a 2x resolution output
    int accumulate;       // DGRAD: out += instead of out =
    int vec_ok;           // outputs (and act) are 16-byte aligned with W % 4 == 0: vector epilogue allowed
    int B, H, W;
    int tiles_x, tiles_y, ntiles;
    pc_fastdiv div_tx, div_tpi;   // by tiles_x, by tiles per image
    int dbg;              // ablation switches (pc_debug_conv): read by -DPOPCORN_CONV_ABLATE builds only
    long long* ts;        // debug timeline buffer (8 slots per workgroup) or NULL: read by -DPOPCORN_CONV_ABLATE builds only
};

constexpr int SROWS = 6;                 // input rows of a 4-row strip (wave-private strips: see conv3x3_mfma_kernel)
constexpr int CSW = SROWS * RS;          // channel stride inside a wave's LDS region

// EPI: extra work of the forward vector epilogue, as separate instantiations so that the other shapes keep their register
// count.  EPI_POOL: also write the 2x2-max-pooled output (ConvProb::pool_out).  EPI_DOT: problems with ConvProb::dot_w
// write the 1x1-conv partial sum over their 8 channels instead of the feature map (ConvProb::dot_out).
// EPI_UPT (channels-last bf16, 8 -> 8 forward): also the ConvTranspose2d that follows.  EPI_POOLBWD: DGRAD with the MaxPool2d(2) backward scatter.
enum { EPI_NONE = 0, EPI_POOL = 1, EPI_DOT = 2, EPI_POOLBWD = 3, EPI_UPT = 4 };

// The ablation switches of the two strip kernels (pc_debug_conv) are compiled out of product builds.  These instantiations keep the
// (never taken) branches on an opaque zero instead: with the tests folded away hipcc allocates them enough more registers to lose a
// resident wave per SIMD (head.hip keeps HeadBwdArgs::zero_in_kernel for the same reason)
constexpr bool conv_mfma_keeps_switch_tests(int cin, int cout, int mode, int ld, int epi, int zc) {
    return mode == MODE_FWD && cout == 8 && zc == 0 &&
           ((cin == 4 && epi == EPI_NONE && (ld == LD_DIRECT || ld == LD_REFLECT)) || (cin == 8 && ld == LD_DIRECT && (epi == EPI_NONE || epi == EPI_POOL)));
}
constexpr bool conv_cl_keeps_switch_tests(int cin, int cout, int ld, int epi) {
    return cout == 8 && epi == EPI_NONE && ((cin == 2 && ld == LD_REFLECT) || (cin == 8 && ld == LD_DIRECT));
}
