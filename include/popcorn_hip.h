/*
 * popcorn_hip.h -- C ABI of libpopcorn_hip.so: the MI355X (gfx950) kernels behind POPCORN's dense
 * per-pixel CNN path.
 *
 * The reference (prs-eth/Popcorn) has no FFI: its boundary is the Python nn.Module API
 * (model/get_model.py:19-61, model/popcorn.py:20-22,100-101) and all arithmetic is stock PyTorch ops.
 * This header is the FFI a maintainer would bind *inside* that nn.Module: every
 * entry point below cites the reference op it replaces.  Conventions:
 *   - plain C, device pointers + sizes only, no torch types;
 *   - every function enqueues on the hipStream_t passed as `void* stream` (0 = the null stream),
 *     never synchronises, and returns 0 or a hipError_t / negative PC_E* code -- with ONE exception: pc_train_step, the eager
 *     whole-step executor, measures on its FIRST call per caller stream which of its side streams runs beside that stream (one host
 *     synchronisation, ~3 ms, cached per stream) and forks / joins through events of its own; it cannot be called while `stream` is
 *     being captured (PC_ENOTSUP) -- captured steps are built from the per-launch entry points; pc_forward, the whole-forward
 *     executor on the same handle type, shares the side stream and the rule;
 *   - tensors are NCHW, described by pc_src / pc_dst (strides in ELEMENTS; element type = `dtype`: fp32, or bf16 for the
 *     activation / activation-gradient tensors of PC_PREC_BF16); parameters, weight gradients and scalars are always fp32;
 *   - pointers are borrowed for the duration of the enqueued work only.
 */
#ifndef POPCORN_HIP_H
#define POPCORN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_ABI_VERSION 10

/* error codes (negative; positive values are hipError_t) */
#define PC_EINVAL (-1)     /* bad argument / unsupported channel combination */
#define PC_ENOGPU (-2)     /* no HIP device */
#define PC_ENOMEM (-3)     /* pc_train_step: the arena is too small (pc_step_io.arena_needed says how much it takes) */
#define PC_ENOTSUP (-4)    /* pc_train_step: a variant the native executor does not cover (the caller keeps the per-launch path) */

/* ---- tensor descriptors ------------------------------------------------------------------------- */

/* how a conv loader maps conv-domain coordinates onto a source tensor */
enum pc_src_mode {
    PC_SRC_DIRECT  = 0,  /* src(y-oy, x-ox); zero outside the source extent (Up's zero F.pad,
                            model/DDA_model/utils/networks.py:309-312) */
    PC_SRC_POOL2   = 1,  /* max over the 2x2 window of a source at twice the resolution: nn.MaxPool2d(2) fused into
                            the consumer (networks.py:289) */
    PC_SRC_REFLECT = 2   /* reflect padding (oy rows on top, ox cols on the left) + channel gather through `chmap`:
                            add_padding + channel reorder fused into the first conv (model/popcorn.py:231-258,130-134) */
};

enum pc_dtype { PC_F32 = 0, PC_BF16 = 1 };

typedef struct pc_src {
    const float* ptr;    /* element (b=0, c=0, y=0, x=0); points at 2-byte elements when dtype == PC_BF16 */
    int32_t C;           /* channels taken from this source (0 = unused) */
    int32_t H, W;        /* spatial extent of the source tensor */
    int64_t bstride;     /* elements between consecutive batch items */
    int64_t cstride;     /* elements between consecutive channels */
    int32_t rstride;     /* elements between consecutive rows */
    int32_t mode;        /* enum pc_src_mode */
    int32_t oy, ox;      /* DIRECT: placement of the source origin in the conv domain; REFLECT: top/left pad */
    int32_t chmap[4];    /* REFLECT only: conv channel c reads source channel chmap[c] */
    int32_t dtype;       /* enum pc_dtype */
    int32_t xstride;     /* elements between x-neighbours: 0 or 1 = planar rows (NCHW); a channels-last tensor
                            (bf16 mode, see below) has cstride = 1 and xstride = its channel count */
} pc_src;

typedef struct pc_dst {
    float* ptr;          /* 2-byte elements when dtype == PC_BF16 */
    int64_t bstride, cstride;
    int32_t rstride;
    int32_t dtype;       /* enum pc_dtype */
    int32_t xstride;     /* as pc_src.xstride */
    int32_t _pad;
} pc_dst;

/* folded BatchNorm2d(eval) + conv bias of one layer: y = relu(conv * scale + shift) with
   scale = gamma / sqrt(var + eps), shift = (bias - mean) * scale + beta   (networks.py:259-266) */
typedef struct pc_bn {
    const float* conv_bias;   /* [C] (may be NULL = 0) */
    const float* gamma;       /* [C] (NULL = no BN: scale 1, shift = conv_bias) */
    const float* beta;
    const float* mean;
    const float* var;
    float eps;
    int32_t _pad;
} pc_bn;

/* ---- library ------------------------------------------------------------------------------------- */
int pc_abi_version(void);
/* number of HIP devices visible (0 on a CPU-only host; never initialises a context) */
int pc_device_count(void);
const char* pc_error_string(int code);
/* sizeof of the ABI structs as compiled: 0 = pc_src, 1 = pc_dst, 2 = pc_bn, 3 = pc_conv_fwd_desc, 4 = pc_adam_groups,
   5 = pc_level2_fwd_desc, 6 = pc_step_plan, 7 = pc_step_io, 8 = pc_step_units (lets a binding verify its struct layout) */
int pc_sizeof(int which);

/* ---- arithmetic mode -----------------------------------------------------------------------------------
 * PC_PREC_FP32 (default): fp32 operands on the fp32 MFMA (v_mfma_f32_16x16x4_f32), the reference's arithmetic.
 * PC_PREC_BF16: bf16 mixed precision (BASELINE config 4; the reference has no such mode -- its only hook is the unused
 *   `half` flag of to_cuda_inplace, utils/utils.py:22-27).  Rounding points, restated by oracle/popcorn_oracle.py (bf16_mode):
 *     - every operand of a matrix product (conv / transposed conv / 1x1 head layer: activations, gradients, weights) is a
 *       bf16 value (round-to-nearest-even); products accumulate in fp32;
 *     - every activation / activation-gradient tensor a kernel writes (conv + BN + ReLU outputs, pooled copies, transposed-
 *       conv outputs, the feature map, all data gradients) is rounded to bf16 by the producing epilogue, after the fp32
 *       bias / BN / ReLU-mask / accumulate arithmetic; the head's hidden layers are rounded after their ReLU;
 *     - everything else stays fp32: BN folding, partial logits and the building score, masks, occupancy product, census
 *       sums, loss, all WEIGHT gradients, the gradient all-reduce, clip, Adam and the master weights.
 *   Activation / activation-gradient tensors (everything a conv, transposed-conv or head kernel hands to another kernel:
 *   pc_src / pc_dst operands) are CHANNELS-LAST bf16 tensors in this mode: dtype = PC_BF16, cstride = 1, xstride = number
 *   of channels of the tensor (8 or 16; a slice of 8 channels of a 16-channel tensor is fine), ptr / rstride / bstride
 *   multiples of 8 elements -- one aligned 16-byte slot per pixel and 8-channel group (torch.channels_last of a bf16 tensor).
 *   The model input (PC_SRC_REFLECT sources), the partial logits / building score, masks, popdensemap, scale map, all
 *   parameters and all weight gradients stay planar fp32.  In PC_PREC_FP32 every tensor is planar fp32 (xstride 0 / 1).
 *   A call whose descriptors do not match the mode returns PC_EINVAL.  The mode is read when a call is enqueued.
 * Process-global; returns the previous mode (pc_set_precision) / the current one. */
enum pc_precision { PC_PREC_FP32 = 0, PC_PREC_BF16 = 1 };
int pc_set_precision(int mode);
int pc_get_precision(void);

/* fp32 mode only: how the sparse head (popcorn.py:80-85,161-190; pc_head_fwd / pc_head_bwd) multiplies.
 *   1 (default; POPCORN_HEAD_SPLIT=0 in the environment starts with 0): every fp32 operand is split EXACTLY into three bf16 numbers
 *     (8 + 8 + 8 mantissa bits) and a product is the fp32-accumulated sum of six bf16 x bf16 partial products on
 *     v_mfma_f32_16x16x32_bf16 / 16x16x16_bf16 -- the three dropped ones are below 2^-23 of the product, i.e. the per-product error is
 *     of the size of one fp32 rounding; results pass every fp32 parity test of the repository unchanged;
 *   0: v_mfma_f32_16x16x4_f32 (one fma chain per accumulator: the summation structure closest to the reference's fp32 GEMMs; the
 *     strict flat-bar parity tests and A/B runs use it).
 * Process-global, read when a call is enqueued (a forward call packs the weight images of BOTH head kernels: switch between steps, not
 * between a forward and its backward).  Returns the previous / the current setting. */
int pc_set_head_split(int on);
int pc_get_head_split(void);

/* fp32 mode only (round 6, ABI 9): how the 3x3 convolution kernels that have a split-operand form multiply: the fused data + weight
 * gradient pc_conv3x3_bwd_group (networks.py:259-266 backward) and the forward convs pc_conv3x3_bn_relu_fwd[_group] /
 * pc_conv3x3_up_fwd_group on aligned planar tensors with 8 or 16 channels (csrc/conv3x3_fwd_s3.h; results differ from the
 * v_mfma_f32_16x16x4_f32 form by rounding only, both are measured against float64 in tests/test_gpu_conv_fwd_split.py).  Same arithmetic
 * as pc_set_head_split:
 *   1 (default; POPCORN_CONV_SPLIT=0 in the environment starts with 0): operands are split exactly into three bf16 numbers when a strip is
 *     staged into LDS (once per strip, not per use), products are six bf16 x bf16 partial products accumulated in fp32 on
 *     v_mfma_f32_16x16x32_bf16; also opens the forms that exist only this way (16 gradient channels, the Down blocks' pool_act);
 *   0: v_mfma_f32_16x16x4_f32 kernels only (8 -> 8 channels; the strict flat-bar tests and A/B runs).
 * Process-global, read when a call is enqueued.  Returns the previous / the current setting. */
int pc_set_conv_split(int on);
int pc_get_conv_split(void);
/* does pc_conv3x3_bwd_group take these fp32 tensors (planar, aligned; Cg = 8 or 16 gradient channels, 8 x channels)?  1 / 0 */
int pc_conv3x3_bwd_ok(const pc_src* g, const pc_src* x, const pc_dst* out, const pc_src* pool_act, int B, int H, int W);
/* ... and with pc_conv_bwd_desc::pool_grad (the pool-add form)? */
int pc_conv3x3_bwd_pool_add_ok(const pc_src* g, const pc_src* x, const pc_dst* out, const pc_src* pool_grad, int B, int H, int W);

/* ---- conv3x3 (+BN +ReLU) forward: nn.Conv2d(3,pad 1) -> BatchNorm2d(eval) -> ReLU, networks.py:259-266.
 * Input channels = a.C + b.C (torch.cat([skip, up]) fused, networks.py:318); conv domain H x W, batch B.
 * w: [Cout][Cin][3][3].  Supported (Cin,Cout): (2,8) (4,8) (8,8) (16,8) (32,8) (8,16) (16,16). */
int pc_conv3x3_bn_relu_fwd(const pc_src* a, const pc_src* b, const float* w, const pc_bn* bn, int relu,
                           const pc_dst* out, int B, int H, int W, int Cin, int Cout, void* stream);

/* Grouped form: up to PC_MAX_GROUP independent problems of identical geometry (B,H,W,Cin,Cout, loader modes) in ONE
 * launch -- e.g. the SAR and optical streams of a layer, or the frozen building extractor next to the trainable U-Net
 * (the four share every layer shape).  Cuts launch count and fills the chip on the 32x32 layers. */
#define PC_MAX_GROUP 4
typedef struct pc_conv_fwd_desc {
    const pc_src* a; const pc_src* b; const float* w; const pc_bn* bn; const pc_dst* out;
    /* optional second output: MaxPool2d(2) of `out` (B x Cout x H/2 x W/2), written by the same epilogue, so that the
     * `Down` block that follows (networks.py:284-295) reads a quarter of the bytes instead of pooling the full-resolution
     * map on the fly.  Only when pc_conv3x3_pool_out_ok(out, H, W) (W % 32 == 0, H % 4 == 0, 16-byte aligned `out`);
     * otherwise the call returns PC_EINVAL. */
    const pc_dst* pool_out;
    /* optional, Cout == 8 only: instead of `out` (may then be NULL) write the single-channel map
     * dot_out[b][0][y][x] = sum_co dot_w[co] * relu(bn(conv))[co] -- the contribution of this layer's 8 feature channels to a
     * following 1x1 convolution (the frozen building extractor's fusion_out_conv, popcorn.py:301: its feature map has no
     * other consumer, so it is never written).  PC_PREC_FP32: any geometry, planar fp32 dot_out; PC_PREC_BF16: the geometry
     * condition of pool_out. */
    const float* dot_w; const pc_dst* dot_out;
    /* optional (PC_PREC_BF16, Cin == 8, no second source): w is [Cout][w_cin][3][3] and applies to input channels
     * [w_ci0, w_ci0 + w_cin) of `a`; the other channels of the 8-channel slot get zero weights.  w_cin == 0: the ordinary full
     * weight.  Lets the first convolutions of both streams (2 SAR / 4 optical channels, networks.py:130-133) read ONE shared
     * 8-channel channels-last input (pc_ingest_cl8) with the standard 8 -> 8 kernel, all (network, stream) pairs in one launch. */
    int32_t w_ci0, w_cin;
    /* optional (PC_PREC_BF16, 8 -> 8 layers, ReLU, no second source / pooled / dot output): the ConvTranspose2d(8, 8, 2, stride 2) of the
     * Up block that consumes this layer's output (networks.py:302-306: weight upt_w [8][8][2][2], bias upt_b) runs in this launch's
     * epilogue and writes upt_out (B x 8 x 2H x 2W, channels-last bf16): the rounded output of a lane IS the matrix operand of the
     * transposed conv, so the separate launch and its read of `out` disappear (`out` is still written for the backward pass).  All
     * problems of a launch or none. */
    const float* upt_w; const float* upt_b; const pc_dst* upt_out;
} pc_conv_fwd_desc;
int pc_conv3x3_pool_out_ok(const pc_dst* out, int H, int W);
int pc_conv3x3_bn_relu_fwd_group(int n, const pc_conv_fwd_desc* d, int relu, int B, int H, int W, int Cin, int Cout,
                                 void* stream);

/* ---- the first conv of an Up block WITHOUT the up-sampled map (PC_PREC_FP32): for an exactly 2x geometry,
 *     conv3x3(torch.cat([skip, ConvTranspose2d(C, C, 2, 2)(z)]))        (networks.py:302-318)
 * is computed from `skip` (Cs channels, H x W) and the LOW-resolution map z (C channels, H/2 x W/2) directly: conv3x3 o convT is a
 * linear map with a 2 x 2 low-resolution neighbourhood per output-pixel parity, whose weights (and the transposed conv's bias seen
 * through the taps that stay inside the image) are composed from w [8][Cs + C][3][3], wt [C][C][2][2], bt [C] into `ws`
 * (pc_conv3x3_up_ws_bytes(C) bytes) by a small first launch.  The up-sampled tensor is neither written nor read, and its half of
 * the convolution costs 2/3 of the MFMAs on a quarter of the input bytes.  (Cs, C) = (8, 8) or (16, 16), Cout = 8, H % 4 == 0,
 * W even, planar fp32 with 16-byte aligned rows (pc_conv3x3_up_fwd_ok); otherwise PC_EINVAL and the callers run
 * pc_convt2x2_fwd_group + pc_conv3x3_bn_relu_fwd_group.  (The backward below exists for W = 64 and 128.) */
typedef struct pc_conv_up_fwd_desc {
    const pc_src* skip; const pc_src* z; const float* w; const float* wt; const float* bt; const pc_bn* bn; const pc_dst* out; void* ws;
} pc_conv_up_fwd_desc;
int64_t pc_conv3x3_up_ws_bytes(int C);
int pc_conv3x3_up_fwd_ok(const pc_src* skip, const pc_src* z, const pc_dst* out, int H, int W, int Cs, int C);
int pc_conv3x3_up_fwd_group(int n, const pc_conv_up_fwd_desc* d, int relu, int B, int H, int W, int Cs, int C, void* stream);
/* The composition alone, for up to 2 * PC_MAX_GROUP convolutions of any mix of the two (Cs, C) shapes in ONE launch (only w, wt, bt, ws of
 * the descriptors are read); pc_conv3x3_up_fwd_group called with relu | PC_UP_PRECOMPOSED then takes ws as it is. */
#define PC_UP_PRECOMPOSED 2
int pc_conv3x3_up_compose_group(int n, const pc_conv_up_fwd_desc* d, const int* Cs, const int* C, void* stream);
/* Backward of that up-sampled half, again without the up-sampled tensor: from g = dL/d(conv output) (8 channels, H x W, already times
 * relu' * bn scale of the conv's layer) and z, ONE pass over g produces
 *   gz (optional) = relu'(z) * z_bn scale * dL/dz                    (what pc_convt2x2_bwd_group wrote for the transposed conv's input)
 *   dw[:, Cs:Cs + C] (=|+=), dwt, dbt                                 (gradients of w's up-sampled half, wt and bt; chain rule through the
 *                                                                     composed weights, incl. the bias seen through the in-image taps)
 * fwd_ws = the workspace the forward call filled (composed operand images), ws = pc_conv3x3_up_bwd_ws_bytes(B, H, C) bytes of scratch.
 * Three launches (the pass, the reduction over its workgroups, the chain rule).  Replaces the up-sampled column block's share of
 * pc_conv3x3_bwd_group / pc_conv3x3_dgrad_group + pc_conv3x3_wgrad_partial_group, pc_convt2x2_bwd_group and pc_convt2x2_fwd_group.
 * The skip half of w and the bias gradient of the conv still come from the skip column block's launch. */
typedef struct pc_conv_up_bwd_desc {
    const pc_src* g; const pc_src* z; const pc_bn* z_bn; const pc_dst* gz;
    const float* w; const float* wt; const float* bt; const void* fwd_ws; void* ws;
    float* dw; float* dwt; float* dbt;
} pc_conv_up_bwd_desc;
int64_t pc_conv3x3_up_bwd_ws_bytes(int B, int H, int C);
int pc_conv3x3_up_bwd_ok(const pc_src* g, const pc_src* z, const pc_dst* gz, int H, int W, int Cs, int C);
int pc_conv3x3_up_bwd_group(int n, const pc_conv_up_bwd_desc* d, int accumulate, int B, int H, int W, int Cs, int C, void* stream);
/* The same in pieces, for callers that batch the reduction with their other weight-gradient reductions: the pass alone (partials
 * [*nwg_out][*part_out] floats at d[i].ws), then pc_wgrad_reduce_batch with a kind-2 entry {partial = ws, dw = ws + nwg * part,
 * Cin = part} per problem, then the chain rule. */
int pc_conv3x3_up_bwd_partial_group(int n, const pc_conv_up_bwd_desc* d, int B, int H, int W, int Cs, int C, int* nwg_out,
                                    int* part_out, void* stream);
int pc_conv3x3_up_chain_group(int n, const pc_conv_up_bwd_desc* d, int accumulate, int nwg, int Cs, int C, void* stream);
/* the chain rules of an (8, 8) level and a (16, 16) level in one launch */
int pc_conv3x3_up_chain_both(int n8, const pc_conv_up_bwd_desc* d8, int nwg8, int n16, const pc_conv_up_bwd_desc* d16, int nwg16,
                             int accumulate, void* stream);

/* ---- conv3x3 data gradient (autograd of the op above w.r.t. its input).
 * g: gradient w.r.t. the conv output (already multiplied by relu-mask * bn-scale), Cg = forward Cout channels.
 * Produces the gradient for forward input channels [c0, c0+Cn) of a forward weight w: [Cg][Cin_total][3][3].
 * Epilogue (what the consumer of that gradient needs):
 *   act == NULL                : out (=|+=) dgrad
 *   act != NULL, pool == 0     : out (=|+=) dgrad * (act > 0) * act_bn.scale      (ReLU + frozen-BN backward of the
 *                                producing layer, whose post-ReLU output is `act`)
 *   act != NULL, pool == 1     : MaxPool2d(2) backward fused: dgrad lives at the pooled resolution; it is routed to the
 *                                first arg-max of each 2x2 window of `act` (full resolution), times (act>0)*scale, and
 *                                ACCUMULATED into out (full resolution).
 * Supported (Cg, Cn): {8, 16} x {8, 16} -- g is the output gradient of a conv layer.  g must be a PC_SRC_DIRECT source (a pooled or
 * reflect-padded gradient does not exist).  Anything else returns PC_EINVAL before a launch.
 */
int pc_conv3x3_dgrad(const pc_src* g, const float* w, int Cin_total, int c0, int Cn,
                     const pc_src* act, const pc_bn* act_bn, int pool, int accumulate,
                     const pc_dst* out, int B, int H, int W, int Cg, void* stream);

typedef struct pc_conv_dgrad_desc {
    const pc_src* g; const float* w; const pc_src* act; const pc_bn* act_bn; const pc_dst* out;
} pc_conv_dgrad_desc;
int pc_conv3x3_dgrad_group(int n, const pc_conv_dgrad_desc* d, int Cin_total, int c0, int Cn, int pool,
                           int accumulate, int B, int H, int W, int Cg, void* stream);
/* ---- backward of one conv3x3 layer in ONE launch (PC_PREC_BF16 only): data gradient AND weight / bias gradient
 * partials from one pass over the layer's output gradient g and input x (both channels-last bf16, 8 or 16 channels).
 *   out (=|+=) relu'(x) * bn_scale(x_bn) * conv^T(g, w[:, c0:c0+XC])     (x_bn NULL: no ReLU / BN factor)
 *   ws <- per-workgroup partials of dW[:, c0:c0+XC] and db, to be finished by pc_wgrad_reduce_batch (Cin = XC, Cout = GC,
 *         dw = &dW[0][c0][0][0], dw_co_stride = Cin_total * 9; *nwg_out partials per problem)
 * (GC, XC) = channels of g and x: (8,8), (8,16), (16,16); with pool_act (16,8), (16,16).  x may be one column block of a
 * concatenated input: x->oy / ox = its placement in the conv domain (zero outside).  Replaces a pc_conv3x3_dgrad +
 * pc_conv3x3_wgrad_partial pair (5 tensor reads + 1 write) by 2 reads + 1 write. */
typedef struct pc_conv_bwd_desc {
    const pc_src* g; const pc_src* x; const float* w; const pc_bn* x_bn; const pc_dst* out; void* ws;
    /* optional (Down blocks): x is the 2x2-max-pooled copy of this full-resolution activation; the data gradient is then
     * scattered (+=) to the first arg-max of every window of `out` (twice the resolution), times relu'(pool_act) * bn_scale(x_bn) */
    const pc_src* pool_act;
    /* added to the call's c0 for THIS problem: the column blocks of a concat layer (same g, different x) can share one launch */
    int32_t c0_add; int32_t _pad;
    /* optional (fp32, 8 gradient channels, x_bn set, no pool_act, no accumulate; W % 32 == 0, H % 4 == 0): x ALSO went through a
     * MaxPool2d(2), and this is the raw data gradient of its pooled copy (planar fp32, 8 channels, H/2 x W/2, rows on 8-byte
     * boundaries).  The epilogue adds its scatter -- first arg-max of every 2x2 window of x, times relu'(x) * bn_scale(x_bn) -- and
     * writes out once: bit for bit what this launch without the operand, followed by a pool_act launch into the same out, leaves */
    const pc_src* pool_grad;
} pc_conv_bwd_desc;
int pc_conv3x3_bwd_group(int n, const pc_conv_bwd_desc* d, int Cin_total, int c0, int accumulate, int B, int H, int W,
                         int* nwg_out, void* stream);
/* ablation switches of the split-operand fused backward kernel (tools/time_conv_bwd.py --ablate; 0 = normal operation): 1 no split / LDS
 * writes, 2 no data-gradient matrix phase, 4 no weight-gradient matrix phase, 8 no prefetch loads, 16 no epilogue.  Honoured by builds with
 * -DPOPCORN_CONV_ABLATE only (tools/build_variant.sh): as run-time flags they cost the shipped kernel its wait placement */
void pc_debug_conv_bwd(int dbg);
/* ablation switches of the forward / data-gradient conv kernels (0, 0 = normal operation).  dbg (tools/ablate_conv.py: 1 no loader, 2 no
 * matrix phase, 4 no epilogue, 8 empty kernel; the split-form forward kernel, tools/time_conv_fwd.py --ablate: 1 no loads / LDS writes,
 * 2 no matrix phase, 4 no epilogue, 32 no split + LDS writes, 64 no loads) is honoured by builds with -DPOPCORN_CONV_ABLATE only
 * (tools/build_variant.sh): as run-time flags the switches cost the shipped kernels their wait placement.
 * max_grid > 0 forces the persistent grid of these launches (host code: every build). */
void pc_debug_conv(int dbg, int max_grid);
/* debug: buffer of 8 x int64 per workgroup receiving wall-clock stamps of conv3x3_mfma_kernel's start and end (NULL = off;
 * tools/conv_timeline.py).  Honoured by builds with -DPOPCORN_CONV_ABLATE only. */
void pc_debug_conv_ts(void* buf);

/* ---- conv3x3 weight/bias gradient.  x = forward input (a,b sources as in fwd), g as in dgrad.
 * Two stages: one partial (dW[co][ci][3][3] + db[co] of the workgroup's tiles) per workgroup into ws, a workspace of
 * pc_conv3x3_wgrad_ws_bytes() per problem; *nwg_out = number of partials.  pc_wgrad_reduce_batch then finishes the partials
 * of many layers in ONE launch: dw [Cout][Cin][3][3], db [Cout]; (=|+=). */
int64_t pc_conv3x3_wgrad_ws_bytes(int Cin, int Cout);
/* one problem, with the grid of a lone problem (more workgroups than a group gives each of its problems) */
int pc_conv3x3_wgrad_partial(const pc_src* a, const pc_src* b, const pc_src* g, void* ws, int B, int H, int W,
                             int Cin, int Cout, int* nwg_out, void* stream);
/* grouped first stage (e.g. the SAR and optical streams of a layer): one launch, each problem with its own ws slice;
 * *nwg_out = partials per problem (identical for all) */
typedef struct pc_conv_wgrad_desc { const pc_src* a; const pc_src* b; const pc_src* g; void* ws; } pc_conv_wgrad_desc;
int pc_conv3x3_wgrad_partial_group(int n, const pc_conv_wgrad_desc* d, int B, int H, int W, int Cin, int Cout,
                                   int* nwg_out, void* stream);
/* transposed conv (dw [Cin][Cout][2][2], db [Cout]): n <= PC_MAX_GROUP problems of identical geometry (the two streams of an Up block) in one launch; every
 * problem gets *nwg_out partials in its own ws */
typedef struct pc_convt_wgrad_desc { const pc_src* x; const pc_src* g; void* ws; } pc_convt_wgrad_desc;
int pc_convt2x2_wgrad_partial_group(int n, const pc_convt_wgrad_desc* d, int B, int H, int W, int C, int* nwg_out,
                                    void* stream);
/* Whole backward of a transposed conv in ONE launch: the weight / bias gradient partials of pc_convt2x2_wgrad_partial_group AND the
 * data gradient of pc_convt2x2_dgrad_group (out = relu'(x) * bn_scale(x_bn) * W^T g; x_bn NULL: no factor) -- both read the 2x
 * resolution gradient g, which passes through the kernel once.  fp32: aligned tensors with W % 16 == 0 only (PC_EINVAL otherwise:
 * the callers keep the two launches); PC_PREC_BF16: any geometry. */
typedef struct pc_convt_bwd_desc {
    const pc_src* x; const pc_src* g; const float* w; const pc_bn* x_bn; const pc_dst* out; void* ws;
} pc_convt_bwd_desc;
int pc_convt2x2_bwd_group(int n, const pc_convt_bwd_desc* d, int B, int H, int W, int C, int* nwg_out, void* stream);

/* ---- the whole 32 x 32 level of a U-Net stream in ONE launch (PC_PREC_FP32): Down.mpconv[1] = DoubleConv(16, 16)
 * (networks.py:253-271,284-295) on an already pooled 16-channel 32 x 32 map, followed by Up.up = ConvTranspose2d(16, 16, 2, 2)
 * (networks.py:302,306):   c1 = relu(bn1(conv3x3(x, w1)));  c2 = relu(bn2(conv3x3(c1, w2)));  u2 = convT(c2, wt) + bt.
 * One workgroup per (tile, problem) keeps x, c1 and c2 in LDS (a whole map is 64 KB: no halo exists at whole-tile residency);
 * only u2 (B x 16 x 64 x 64) and, when c1 / c2 are given (networks whose backward pass needs them), those two maps go to HBM.
 * Replaces two pc_conv3x3_bn_relu_fwd_group launches and one pc_convt2x2_fwd_group launch.  Geometry: x 16 channels, 32 x 32,
 * planar fp32, 16-byte aligned rows (pc_level2_fwd_ok); anything else returns PC_EINVAL and the callers keep the three launches.
 * PC_PREC_BF16 (level2_cl.hip): the same call on channels-last bf16 tensors (x, c1, c2: 16-channel pixels; u2 B x 16 x 64 x 64) --
 * the whole tile as the LDS strip image of the channels-last conv kernel, bit-identical to the three launches it replaces. */
typedef struct pc_level2_fwd_desc {
    const pc_src* x; const float* w1; const pc_bn* bn1; const float* w2; const pc_bn* bn2; const float* wt; const float* bt;
    const pc_dst* c1; const pc_dst* c2;   /* optional (NULL: not written) */
    const pc_dst* u2;                     /* optional when c2 is given: NULL skips the transposed conv (a consumer that takes c2
                                             through pc_conv3x3_up_fwd_group needs no up-sampled map) */
} pc_level2_fwd_desc;
int pc_level2_fwd_ok(const pc_src* x, const pc_dst* u2);
int pc_level2_fwd_group(int n, const pc_level2_fwd_desc* d, int B, void* stream);
/* Backward of the two convolutions of that level in ONE launch (both arithmetic modes: level2.hip; channels-last bf16 tensors
 * in PC_PREC_BF16: level2_cl.hip, one partial per tile, *nwg_out = B, replacing two pc_conv3x3_bwd_group launches), given g2 = dL/d(conv2 output) (already times
 * relu'(c2) * bn2 scale: pc_convt2x2_bwd_group writes it): weight / bias gradient partials of both layers (ws2: dW2, db2 from
 * g2 x c1; ws1: dW1, db1 from g1 x x; fp32: 2 partials per tile in the layout pc_wgrad_reduce_batch finishes as kind 0, Cin = Cout = 16:
 * *nwg_out = 2 B, each ws pc_level2_bwd_ws_bytes(B) bytes), the data gradient g1 = relu'(c1) * bn1 scale * conv^T(g2, w2) kept in
 * LDS, and the MaxPool2d(2) backward of conv^T(g1, w1) accumulated into `out` (B x 16 x 64 x 64: the first arg-max of every 2 x 2
 * window of `act`, times relu'(act) * act_bn scale).  Replaces two pc_conv3x3_wgrad_partial_group and two
 * pc_conv3x3_dgrad_group launches; same geometry rule as the forward (pc_level2_bwd_ok). */
typedef struct pc_level2_bwd_desc {
    const pc_src* g2; const pc_src* c1; const pc_src* x; const float* w1; const float* w2; const pc_bn* bn1;
    const pc_src* act; const pc_bn* act_bn; const pc_dst* out; void* ws1; void* ws2;
    /* optional (fp32): B x 16 x 32 x 32, planar, 16-byte rows.  conv^T(g1, w1) is written there raw, at the pooled resolution, INSTEAD
     * of the scatter: `act` is not read and `out` not touched (both still describe valid tensors).  The launch that writes `out`
     * adds the scatter (pc_conv_bwd_desc::pool_grad) */
    const pc_dst* pool_grad_out;
} pc_level2_bwd_desc;
int64_t pc_level2_bwd_ws_bytes(int B);
int pc_level2_bwd_ok(const pc_src* g2, const pc_src* c1, const pc_src* x, const pc_src* act, const pc_dst* out);
int pc_level2_bwd_group(int n, const pc_level2_bwd_desc* d, int B, int* nwg_out, void* stream);
/* debug: 16 x int64 buffer receiving wall-clock (100 MHz) phase stamps of workgroup (0, 0) of pc_level2_bwd_group (NULL = off) */
void pc_debug_level2_ts(void* buf);
/* test hook: the cross-lane helpers the kernels use instead of __shfl_xor (= ds_bpermute_b32), applied to one 64-lane wave of floats.
 * out[384]: [0,64) sum over the 8 lanes sharing lane >> 3 in the association order of the xor-1, -2, -4 butterfly; [64,128) max(x, x of
 * lane ^ 8); [128,192) x + x of lane ^ 16; [192,256) x + x of lane ^ 32; [256,320) x of lane ^ 1; [320,384) x of lane ^ 2 */
int pc_debug_lane_ops(const float* in, float* out, void* stream);
typedef struct pc_wgrad_reduce_desc {
    const float* partial;   /* ws of the deferred call */
    float* dw; float* db;   /* outputs ([Cout][Cin][3][3] / [Cin][Cout][2][2]; db may be NULL) */
    int32_t nwg, Cin, Cout; /* convT: Cin = Cout = C */
    int32_t kind;           /* 0: conv3x3, 1: convT 2x2, 2: raw sum of Cin floats per partial into dw (pc_conv3x3_up_bwd_partial_group),
                               3: the sparse head's partials (pc_head_bwd with PC_HEAD_BWD_DEFER_REDUCE; partial / nwg from
                               pc_head_bwd_partials): dw = HOST array of the head's 8 gradient tensors (device pointers in the order of
                               pc_head_bwd's dhw, NULL = skip), db / Cin / Cout unused; at most one such entry per call */
    int32_t accumulate;
    int32_t dw_co_stride;   /* conv3x3: elements between output channels of dw (0 = Cin * 9); > Cin * 9 when the entry is one
                               8-channel column block of a wider weight gradient (dw then points at its first column) */
    int32_t src_cin, src_ci0; /* conv3x3: the partials were computed over src_cin input channels (0 = Cin) of which this entry
                               writes the Cin channels starting at src_ci0 into dw -- the weight gradient of a first layer whose
                               input is a channel window of the shared 8-channel input (pc_conv_fwd_desc.w_ci0 / w_cin) */
} pc_wgrad_reduce_desc;
int pc_wgrad_reduce_batch(int n, const pc_wgrad_reduce_desc* d, void* stream);

/* ---- ConvTranspose2d(C, C, 2, stride 2), networks.py:302,306.  w: [Cin][Cout][2][2].  x: B x C x H x W -> out B x C x 2H x 2W */
int pc_convt2x2_fwd(const pc_src* x, const float* w, const float* bias, const pc_dst* out, int B, int H, int W, int C,
                    void* stream);
/* data gradient, fused with the ReLU+BN backward of the layer that produced x (act = x's post-ReLU values) */
int pc_convt2x2_dgrad(const pc_src* g, const float* w, const pc_src* act, const pc_bn* act_bn,
                      const pc_dst* out, int B, int H, int W, int C, void* stream);
/* grouped forms (problems of identical geometry in one launch, blockIdx.y = problem) */
typedef struct pc_convt_fwd_desc { const pc_src* x; const float* w; const float* bias; const pc_dst* out; } pc_convt_fwd_desc;
typedef struct pc_convt_dgrad_desc {
    const pc_src* g; const float* w; const pc_src* act; const pc_bn* act_bn; const pc_dst* out;
} pc_convt_dgrad_desc;
int pc_convt2x2_fwd_group(int n, const pc_convt_fwd_desc* d, int B, int H, int W, int C, void* stream);
int pc_convt2x2_dgrad_group(int n, const pc_convt_dgrad_desc* d, int B, int H, int W, int C, void* stream);
int64_t pc_convt2x2_wgrad_ws_bytes(int C);

/* ---- fusion_out_conv (1x1, 16->1) + sigmoid + crop: create_building_score's tail, popcorn.py:301,317-320;
 * networks.py:232,323-330.  feat: B x C x Hp x Wp with C = 16 (fusion_out_conv) or 8 (sar_out_conv / optical_out_conv of the
 * single-modality variants, networks.py:217-228), out: B x 1 x H x W taken at offset (py,px). */
int pc_outconv_sigmoid_crop(const pc_src* feat, const float* w, const float* bias, const pc_dst* out,
                            int B, int H, int W, int py, int px, void* stream);

/* ---- sparsity mask, popcorn.py:361-377 (non-sparse_unet branch).
 * mask[b,y,x] = region & ((building>0) | (rowsel[y] & colsel[x])), region = (admin_mask == census_idx[b]);
 * rowsel/colsel: uint8 [H]/[W] (the sorted multinomial draws, made on the host CPU generator like the reference).
 * If the whole batch selects nothing the mask falls back to the region (popcorn.py:374-375).
 * counts: int32[2] device scratch {nsel, nregion}. */
int pc_sparsity_mask(const float* building, const float* admin_mask, const int64_t* census_idx,
                     const uint8_t* rowsel, const uint8_t* colsel, int occupancymodel,
                     uint8_t* mask, int32_t* counts, int B, int H, int W, void* stream);

/* The sparse_unet branch of get_sparsity_mask (popcorn.py:336-359; no caller in the reference uses it):
 * mask = ((building > threshold) | (rowsel[y] & colsel[x])) & region, and per sample the undersampling ratio
 * ratio[b] = #(region & building <= threshold) / (#(grid & region & building <= threshold) + 1e-5).  threshold = 0.001 and a
 * 250 x 250 grid in the reference. */
int pc_sparsity_mask_unet(const float* building, const float* admin_mask, const int64_t* census_idx,
                          const uint8_t* rowsel, const uint8_t* colsel, float threshold, uint8_t* mask, float* ratio,
                          int B, int H, int W, void* stream);

/* pc_outconv_sigmoid_crop + pc_sparsity_mask in ONE launch (the building score feeds the mask directly; the empty-selection
 * fallback and the count fix-up are done by the last block to finish).  Same arguments and results as the two calls.
 * Must not run concurrently with itself on two streams of one process (library-owned accumulator + ticket). */
int pc_building_score_mask(const pc_src* feat, const float* w, const float* bias, const pc_dst* building_out,
                           const float* admin_mask, const int64_t* census_idx, const uint8_t* rowsel,
                           const uint8_t* colsel, int occupancymodel, uint8_t* mask, int32_t* counts,
                           int B, int H, int W, int py, int px, void* stream);

/* ---- the sparse head, popcorn.py:80-85,161-190,195-228:
 * per selected pixel 16 -> 64 -> 64 -> 64 -> (channel 0 of 2) 1x1-conv MLP with ReLUs, scale = relu(out),
 * popdensemap = scale * building, popcount[b] = sum over region pixels.  mask == NULL: dense head.
 * admin_mask == NULL: popcount = plain sum (popcorn.py:189-190).
 * feat: B x 16 x Hp x Wp read at crop offset (py,px) (revert_padding fused, popcorn.py:155).
 * hw: the 8 head tensors {w0,b0,w2,b2,w4,b4,w6,b6}.  ws: pc_head_ws_bytes().
 * stats (optional, device double[2]) receives {Nsel, sum(scale)}: Nsel = nsel_counts[0] (the int32 count written by
 * pc_sparsity_mask) or B*H*W for the dense head -- the inputs of the scale regulariser (utils/losses.py:74). */
int64_t pc_head_ws_bytes(int B, int H, int W);
int pc_head_fwd(const pc_src* feat, int py, int px, const float* const* hw, const uint8_t* mask,
                const float* building, const float* admin_mask, const int64_t* census_idx,
                float* scale_map, float* popdensemap, float* popcount, double* stats,
                const int32_t* nsel_counts, void* ws, int B, int H, int W, int flags, void* stream);
/* flags of pc_head_fwd / pc_head_bwd.  Both kernels read the head's weights from an LDS image that a small launch assembles in `ws`
 * per call.  A training step runs pc_head_fwd and pc_head_bwd on the SAME weights and workspace: PC_HEAD_FWD_PACK_BOTH makes the
 * forward call's pack launch write the backward's image as well, PC_HEAD_BWD_PACKED tells the backward call that it is there (the
 * caller guarantees: same hw contents, same ws, same B / H / W, same arithmetic mode in between) -- one launch less per step. */
#define PC_HEAD_FWD_PACK_BOTH 1
#define PC_HEAD_BWD_PACKED 1
/* PC_HEAD_FWD_DEFER_REDUCE: pc_head_fwd leaves popcount / stats unreduced (its last, single-block launch is skipped);
 * pc_head_popcount_loss(ws, ...) -- same ws, B, H, W -- then finishes popcount[B] and stats[2] AND computes the loss forward + backward
 * of pc_loss_fwd_bwd in one single-block launch (a single-process training step: one launch less; a data-parallel step all-reduces
 * the stats between the two and keeps the separate calls). */
#define PC_HEAD_FWD_DEFER_REDUCE 2
/* PC_HEAD_BWD_DEFER_REDUCE: pc_head_bwd leaves its per-workgroup weight-gradient partials in ws unreduced (its last launch is
 * skipped; g_feat is complete); the caller finishes them with an entry of kind 3 in the pc_wgrad_reduce_batch call of the same
 * backward pass -- partial / nwg from pc_head_bwd_partials(ws, B, H, W) (same ws, B, H, W, same arithmetic mode) -- one launch less. */
#define PC_HEAD_BWD_DEFER_REDUCE 2
int pc_head_bwd_partials(void* ws, int B, int H, int W, const float** partial, int* nwg);
int pc_head_popcount_loss(void* ws, int B, int H, int W, const int32_t* nsel_counts, const float* y, const float* lam4,
                          float scale_regularization, float lam_weak, float inv_B, float* popcount, double* stats,
                          float* loss_out, float* g_popcount, float* g_scale_const, void* stream);

/* backward of pc_head_fwd (the forward chain is recomputed in registers).  Upstream gradients, all optional (NULL):
 *   g_popcount[B]; g_popdense[B][H][W]; g_scale_map[B][H][W] (gradient w.r.t. scale = relu(out), e.g. the scattered
 *   gradient of the compacted scale vector); g_scale_const: DEVICE scalar added on every selected pixel (the
 *   scale-regularisation term scale_regularization * lam / Nsel, utils/losses.py:74-76).
 * Produces the 8 head gradients dhw[i] (=|+=; entries may be NULL; head.6 row/bias 1 get exact zeros, as autograd
 * gives for the unused second output channel) and the gradient w.r.t. the padded 16-channel feature map g_feat
 * (contiguous B x 16 x Hp x Wp; zero outside the crop and on unselected pixels).  If feat_bn_sar/feat_bn_opt are given
 * (BN of the layers that produced feature channels 0-7 / 8-15, networks.py:263-266) g_feat is additionally multiplied by
 * (feat > 0) * bn_scale, i.e. it is the gradient w.r.t. those layers' conv outputs. */
int pc_head_bwd(const pc_src* feat, int py, int px, const float* const* hw, const uint8_t* mask,
                const float* building, const float* admin_mask, const int64_t* census_idx,
                const float* g_popcount, const float* g_popdense, const float* g_scale_map,
                const float* g_scale_const, float* const* dhw, int accumulate,
                const pc_dst* g_feat, const pc_bn* feat_bn_sar, const pc_bn* feat_bn_opt,
                int Hp, int Wp, void* ws, int B, int H, int W, int flags, void* stream);
/* debug (tests/tie_adjudication.py, tests/test_gpu_convt_head.py): the ReLU decisions pc_head_bwd actually takes.  The kernel keeps
 * the head's hidden activations in registers; while a device buffer is registered here (NULL = off), pc_head_bwd in fp32 mode launches
 * an instantiation of its producer / consumer kernel -- in the multiplication form in force, pc_set_head_split -- that ALSO writes one
 * record per SELECTED pixel of the B x H x W crop (mask == NULL: every pixel), record b * H * W + y * W + x, whatever the upstream
 * gradients are; the records of unselected pixels are left untouched.  Everything else the call computes is unchanged bit for bit
 * (the call drains its stream once before the launch; one exporting call at a time).  A record is PC_HEAD_DEC_BYTES = 4 little-endian 64-bit words, word k (0 - 3):
 *   bit 16 l + 4 m + r  (l = 0, 1, 2; m, r = 0 - 3): the pre-activation of unit 16 m + 4 k + r of hidden layer l (head.0 / .2 / .4)
 *                        is > 0, i.e. the unit passes gradient;
 *   bit 48              : the output decision out[:, 0] > 0 of the final relu (the same in all four words);
 *   bit 63              : set in every word the kernel wrote; all other bits are 0.
 * pc_head_bwd returns PC_EINVAL, launching nothing, when a buffer is registered and it is smaller than B * H * W records or not 8-byte
 * aligned, or the call would run a kernel without the export (bf16 mode). */
#define PC_HEAD_DEC_BYTES 32
void pc_debug_head_decisions(void* buf, int64_t bytes);

/* ---- compaction of scale[mask] in row-major (b,y,x) order (the boolean-index gather of popcorn.py:173).
 * out must hold B*H*W floats; *n_out (device int32) receives Nsel. */
int pc_compact_masked(const float* src, const uint8_t* mask, float* out, int32_t* n_out, void* ws, int64_t n,
                      void* stream);
int64_t pc_compact_ws_bytes(int64_t n);
/* The inverse (autograd of that gather): out[i] = mask[i] ? src[rank of i among the selected] : 0, i < n.  src holds at least
 * Nsel floats; ws as for pc_compact_masked. */
int pc_scatter_masked(const float* src, const uint8_t* mask, float* out, void* ws, int64_t n, void* stream);

/* F.pad(x, (left, right, top, bottom), mode="reflect") on `planes` contiguous H x W planes -> (H+top+bottom) x (W+left+right):
 * add_padding as a standalone op (popcorn.py:231-258).  The model path never calls it (the padding is fused into the first
 * convolution's loader); it backs the POPCORN.add_padding API method. */
int pc_reflect_pad(const float* in, float* out, int64_t planes, int H, int W, int top, int bottom, int left, int right,
                   void* stream);
/* The same with the channel gather of popcorn.py:130-134 (S1 / S2 band selection and order): out[b][j] = pad(in[b][sel[j]]) for
 * in (B, Cin, H, W) -> out (B, nsel, Hp, Wp), nsel <= 8, sel = HOST array.  The fp32 path materialises the padded input once per
 * forward pass with it: the first convolutions of all (network, stream) pairs and their weight gradients then take the aligned
 * DIRECT loader instead of running the reflect loader once per consumer. */
int pc_reflect_pad_select(const float* in, float* out, int B, int Cin, int nsel, const int* sel, int H, int W, int top, int bottom,
                          int left, int right, void* stream);
/* The ingest of a raw tile in ONE pass: band selection (data/PopulationDataset.py:566-568) + apply_normalize (utils/utils.py:105-127)
 * + the reflect padding / channel order above:  out[b][j] = pad((raw[b][band[j]] - mean[j]) / std[j]),  raw (B, Craw, H, W),
 * band / mean / std = HOST arrays of nsel <= 8 entries.  Replaces pc_select_normalize followed by pc_reflect_pad_select. */
int pc_select_normalize_pad(const float* raw, float* out, int B, int Craw, int nsel, const int* band, const float* mean,
                            const float* stdv, int H, int W, int top, int bottom, int left, int right, void* stream);
/* The same ingest for PC_PREC_BF16: out is ONE channels-last bf16 tensor (B, 8, Hp, Wp) -- an aligned 16-byte slot per pixel
 * holding the nsel <= 8 selected, normalised (mean / stdv may be NULL: input already normalised), reflect-padded channels rounded
 * to bf16, the remaining channels zero.  Both streams' first convolutions (pc_conv_fwd_desc.w_ci0 / w_cin) and their weight
 * gradients (pc_wgrad_reduce_desc.src_cin / src_ci0) read this one tensor through the standard 8-channel kernels instead of
 * running a planar-fp32 reflect loader per consumer. */
int pc_ingest_cl8(const float* raw, void* out, int B, int Craw, int nsel, const int* band, const float* mean, const float* stdv,
                  int H, int W, int top, int bottom, int left, int right, void* stream);
/* Either ingest from the TWO tensors a loader ships per sample (data/PopulationDataset.py:566-600: the Sentinel-2 GeoTIFF bands and the
 * Sentinel-1 bands, separately): s2 (B, C2, H, W) UINT16 digital numbers (reflectance x 10,000: 0 .. ~10,000 -- the file's own type, two
 * thirds of the host-to-device bytes of an fp32 tile) and s1 (B, C1, H, W) fp32 backscatter.  band[j] indexes the concatenation
 * [s2 | s1]; the uint16 -> fp32 conversion is exact, so the result equals the fp32-fed ingest bit for bit.  cl8 = 0: planar fp32
 * out (B, nsel, Hp, Wp) as pc_select_normalize_pad writes it; cl8 = 1: the channels-last bf16 slot tensor of pc_ingest_cl8. */
int pc_ingest_split(const uint16_t* s2, int C2, const float* s1, int C1, void* out, int cl8, int B, int nsel, const int* band,
                    const float* mean, const float* stdv, int H, int W, int top, int bottom, int left, int right, void* stream);

/* ---- training-step scalars ------------------------------------------------------------------------- */

/* Population loss + scale regulariser and their gradients, utils/losses.py:49-76 + autograd.
 * lam4 = weights of {l1_loss, log_l1_loss, mse_loss, log_mse_loss} (host array of 4); the batch mean is taken with
 * inv_B = 1 / (world_size * B) so that the SUM of all ranks' gradients equals the single-process gradient.
 * stats: device double[2] {Nsel, sum(scale)} from pc_head_fwd (all-reduced across ranks in data-parallel runs).
 * loss_out[2] = {loss, regulariser};  g_popcount[B] = d(lam_weak*loss)/d popcount;  *g_scale_const = lam_weak *
 * scale_regularization / Nsel (the constant gradient of the regulariser on every selected pixel). */
int pc_loss_fwd_bwd(const float* popcount, const float* y, const double* stats, const float* lam4,
                    float scale_regularization, float lam_weak, float inv_B, int B,
                    float* loss_out, float* g_popcount, float* g_scale_const, void* stream);

/* Parameter groups of the flat buffer for the Adam step.  The reference gives the encoder (limit1) or the whole U-Net
 * (limit2) no gradient on large samples (run_train.py:191-198; networks.py:124-132), and torch.optim.Adam skips a
 * parameter whose .grad is None entirely: no weight decay, no moment update, no per-parameter step increment.  The flat
 * buffer is cut into nseg consecutive segments [seg_end[i-1], seg_end[i]) (seg_end[nseg-1] == n), each belonging to one
 * of PC_ADAM_GROUPS groups; groups whose bit is clear in active_mask are left untouched (p, m, v and the group's step
 * counter), and step_dev is then int32[PC_ADAM_GROUPS] -- one counter per group, torch's per-parameter `step`. */
#define PC_ADAM_MAX_SEG 8
#define PC_ADAM_GROUPS 4
typedef struct pc_adam_groups {
    int32_t nseg;
    int32_t seg_end[PC_ADAM_MAX_SEG];
    int32_t seg_group[PC_ADAM_MAX_SEG];
    int32_t active_mask;
} pc_adam_groups;

/* clip_grad_norm_(max_norm) + torch.optim.Adam step over flat buffers (run_train.py:82-90,233-238) in ONE launch: every
 * workgroup computes the total L2 norm of g itself (clip_grad_norm_'s total_norm, deterministic; written to norm_out_dev if
 * non-NULL), then clips and updates; max_norm <= 0: no clipping.  Weight decay (L2, added to the gradient) applies to elements
 * [0, n_decay) only.  hyper_dev: device float[1] {lr}; step_dev: device int32 step counter(s), incremented by the call
 * (groups == NULL: one counter, everything updated).  g must be 16-byte aligned.  Must not run concurrently with itself on
 * two streams of one process (a device-side ticket decides which workgroup advances the step counter). */
int pc_adam_clip_step_fused(float* p, const float* g, float* m, float* v, int n, int n_decay, const float* hyper_dev,
                            float weight_decay, float beta1, float beta2, float eps, float max_norm,
                            float* norm_out_dev, int32_t* step_dev, const pc_adam_groups* groups, void* stream);

/* Band selection + per-band (x - mean) / std: data/PopulationDataset.py:566-568 + utils/utils.py:105-127.
 * raw: B x Craw x H x W; out: B x 6 x H x W; band6/mean6/std6: host arrays of 6. */
int pc_select_normalize(const float* raw, int Craw, const int* band6, const float* mean6, const float* std6,
                        float* out, int B, int H, int W, void* stream);

/* The trainer's augmentations applied in ONE pass while the raw 6-channel tile is assembled (run_train.py:386-402, utils/transform.py:
 * RandomBrightness / RandomGamma on the 4 Sentinel-2 bands, then vertical flip, horizontal flip and a rotation by rot quarter turns
 * counter-clockwise, jointly on input and admin_mask; one coin per batch, drawn by the caller with the reference's generators):
 *   raw[b] = rot90^rot(hflip(vflip(cat[aug(s2[b]), s1[b]]))),   admin_out[b] = the same geometric map of admin[b]
 * s2 (B, 4, H, W) digital numbers, s1 (B, 2, H, W), admin (B, H, W), all fp32; raw (B, 6, Ho, Wo), admin_out (B, Ho, Wo) with
 * (Ho, Wo) = (W, H) for odd rot.  bright / gam: apply x -> clamp(x / 1e4 * beta, 0, 1) * 1e4, then x -> clamp((max(x, 0) / 1e4)^gamma, 0, 1) * 1e4.
 * Replaces apply_transformations_and_normalize's augmentation half (utils/utils.py:130-214); the normalisation is the step's ingest. */
int pc_augment_raw(const float* s2, const float* s1, const float* admin, float* raw, float* admin_out, int B, int H, int W,
                   int vflip, int hflip, int rot, int bright, float beta, int gam, float gamma, void* stream);

/* ---- native executor of ONE training step: the body of the reference's inner loop (run_train.py:186-238) as one call -----------
 *   forward(train, padding=False, sparse=True) (popcorn.py:100-193) -> get_loss (utils/losses.py:49-76) -> x lam_weak -> backward
 *   -> clip_grad_norm_ -> Adam step -> zero_grad
 * for ANY batch geometry (B, H, W) and truncation regime (encoder_no_grad / unet_no_grad: run_train.py:191-198): the reference
 * trains on weak_batch_size = 2 census regions of varying size (arguments/train.py:16,34-36), which cannot replay a captured HIP
 * graph -- and launching the step's ~45 kernels one ctypes call at a time costs more host time than a small region's kernels take
 * (tools/host_time_eager.py).  pc_train_step computes the geometry of both networks (the trainable U-Net on the add_padding domain,
 * popcorn.py:231-258; the frozen building extractor on its own 14-pixel reflect-padded domain, popcorn.py:279-322), carves every
 * activation / gradient / workspace out of ONE caller-provided arena (bump allocation, rows padded to 16 bytes so that every conv
 * launch takes the aligned staged loaders whatever the region's width), fills the descriptors and issues all launches from C++.
 * The plan (parameter pointers, BN descriptors, optimiser constants) is built once per trainer (pc_step_create); a step passes only
 * its batch.  PC_PREC_FP32, dual-stream (S1 + S2) and one-stream models, with or without the occupancy product (plan.occupancymodel = 0:
 * the mask is the region only and the head multiplies by a plane of ones the step fills in the arena, popcorn.py:179-181), whose building
 * score comes from the frozen extractor or from the layer the batch ships (pc_train_step_layer, below); bf16 returns PC_ENOTSUP and the
 * caller keeps the per-launch path (same kernels, launched through the entry points above).
 * A ONE-STREAM PLAN (the reference's -S1 alone / -S2 -NIR alone models, popcorn.py:48-54,135-145,302-314) is the same pc_step_plan with
 *   - the table of the absent stream (pc_step_stream: s[0] sar, s[1] optical -- a stream keeps its slot) ALL ZERO in both unet and extractor;
 *   - fusion_w / fusion_b of each net pointing at the present stream's own out conv (sar_out_conv / optical_out_conv, networks.py:217-228:
 *     8 weights, 1 bias): the building score is sigmoid(out conv over the stream's 8 feature channels) on both domains;
 *   - head_w[0] / head_dw[0] pointing at the 64 x 8 first head layer and its gradient inside flat_g (the other seven as ever);
 *   - feat_c0 of the present stream 0 or 8, the same in both nets.
 * pc_train_step, pc_train_step_layer, pc_train_step_units and pc_train_step_units_layer take it and compute the bits of the per-launch
 * step.  The feature map stays 16 channels: inside the call the absent stream's 8 are zero-filled, w0 is embedded at feat_c0 of a zeroed
 * 64 x 16 image in the arena in front of the head forward, and the live half of the head's 64 x 16 first-layer gradient image is copied
 * into head_dw[0] behind the reduction that finishes it, in front of the gradient norm.  Data: PC_DATA_INPUT is (B, cin, H, W) -- the
 * stream's own channels, picked by chan[] --, or (B, io->craw, H, W) when io->craw > 0 (a wider tile of which chan[] picks);
 * PC_DATA_RAW / PC_DATA_SPLIT as for two streams.  Side stream, phases (io->dp), arena_needed, the output offsets and launches behave as
 * for a dual-stream plan.  Refused before anything is enqueued: a stream present in one net and absent in the other, or in neither
 * (present: cin >= 1 and w[0] != NULL), a chan[] beyond the PC_DATA_INPUT tensor: PC_EINVAL.  pc_forward keeps refusing a one-stream
 * plan (PC_ENOTSUP).
 * Small regions fork the frozen extractor's chain and the weight-gradient launches onto an internal side stream; WHICH stream is
 * measured at the first call on a caller's stream (HIP multiplexes streams onto a few hardware queues, and a side stream on the
 * caller's queue serialises with it): that first call launches a few microsecond-long probe kernels and synchronises once, so
 * pc_train_step is an EAGER entry point -- not to be called on a stream that is being captured into a graph.
 * Conv layer order of the arrays below: inc.conv.0, inc.conv.3, down1.conv.0, down1.conv.3, down2.conv.0, down2.conv.3,
 * up2.conv.0, up2.conv.3, up1.conv.0, up1.conv.3 (networks.py:121-151,253-320); transposed convs: up2.up, up1.up. */
#define PC_STEP_CONVS 10
typedef struct pc_step_stream {
    const float* w[PC_STEP_CONVS];      /* conv weights [Cout][Cin][3][3] */
    pc_bn bn[PC_STEP_CONVS];            /* conv bias + BatchNorm2d(eval) of the layer */
    const float* wt[2]; const float* bt[2];      /* ConvTranspose2d weights [C][C][2][2] and biases */
    float* dw[PC_STEP_CONVS]; float* db[PC_STEP_CONVS]; float* dwt[2]; float* dbt[2];   /* gradient targets (trainable network only) */
    int32_t chan[4];                    /* model-input channel of conv channel c ([R,G,B,NIR,VV,VH]: SAR 4,5; optical 2,1,0,3) */
    int32_t cin, feat_c0;               /* 2 / 4 input channels; first channel of this stream in the 16-channel feature map */
} pc_step_stream;
typedef struct pc_step_net { pc_step_stream s[2]; const float* fusion_w; const float* fusion_b; } pc_step_net;   /* one-stream plan: the stream's out conv */
typedef struct pc_step_plan {
    pc_step_net unet, extractor;        /* model.unetmodel (trainable), model.building_extractor (frozen) */
    const float* head_w[8]; float* head_dw[8];     /* {w0,b0,w2,b2,w4,b4,w6,b6} and their gradients (w0: 64 x 16; one-stream plan: 64 x 8) */
    float* flat_p; float* flat_g; float* adam_m; float* adam_v;     /* flat parameter / gradient / moment buffers (n floats) */
    int32_t n, n_decay, n_head, occupancymodel;
    const float* hyper_dev; int32_t* step_dev; float* norm_dev; double* stats_dev; float* loss_dev; float* g_scale_const_dev;
    pc_adam_groups groups;              /* segments of the flat buffer; active_mask is set per step from the regime */
    float weight_decay, beta1, beta2, eps, max_norm, scale_regularization, lam_weak;
    float lam4[4];
    int32_t extractor_pad;              /* 14 (popcorn.py:46) */
    int32_t band[8]; float mean[8]; float stdv[8];      /* raw-tile ingest: model channel c = (raw band band[c] - mean[c]) / stdv[c] */
} pc_step_plan;
enum pc_step_data { PC_DATA_INPUT = 0,   /* data = normalised model input (B, 6, H, W) fp32 */
                    PC_DATA_RAW = 1,     /* data = raw tile (B, craw, H, W) fp32 (data/PopulationDataset.py:566-568 + utils/utils.py:105-127 fused) */
                    PC_DATA_SPLIT = 2 }; /* data = uint16 S2 digital numbers (B, 4, H, W), data2 = fp32 S1 (B, 2, H, W) */
#define PC_STEP_SEL_MAX 16384
#define PC_STEP_FWD 1      /* ingest .. head forward (+ popcount / stats unless the loss launch finishes them) */
#define PC_STEP_BWD 2      /* loss, head backward, U-Net backward into flat_g */
#define PC_STEP_UPD 4      /* clip + Adam */
typedef struct pc_step_io {
    int32_t B, H, W, data_kind;
    const void* data; const void* data2; int32_t craw, dp;          /* dp != 0: data parallel -- the caller all-reduces stats_dev between the
                                                                       FWD and BWD phases and flat_g between BWD and UPD */
    const float* admin_mask; const int64_t* census_idx; const float* y;
    const uint8_t* sel;          /* DEVICE: H row flags then W column flags (the two multinomial draws of get_sparsity_mask, popcorn.py:366-369) */
    int32_t encoder_no_grad, unet_no_grad; float inv_B; int32_t _pad;
    const uint8_t* sel_host;     /* or HOST: the same H + W flags in host memory (sel is then ignored): they travel bit-packed in the kernel
                                    arguments of a one-block launch -- no H2D copy command (and none of its dispatch latency) per step;
                                    H + W <= PC_STEP_SEL_MAX */
    void* arena; int64_t arena_bytes;       /* device scratch, 256-byte aligned; contents are undefined between steps */
    /* results */
    int64_t arena_needed;                   /* bytes this geometry takes (always set; PC_ENOMEM when arena_bytes is smaller) */
    int64_t off_popcount, off_popdense, off_scale, off_mask, off_building;   /* byte offsets of the step's outputs inside the arena:
                                               popcount f32[B], popdensemap f32[B][H][W], scale map f32[B][H][W], mask u8[B][H][W],
                                               building score f32[B][1][H][W] -- valid until the next call.  With a given layer
                                               (pc_train_step_layer) no plane is allocated and off_building = -1: the caller's tensor is
                                               the output */
    int32_t launches, _pad2;                /* kernels enqueued by the call */
} pc_step_io;
void* pc_step_create(const pc_step_plan* plan);
void pc_step_destroy(void* handle);
int pc_train_step(void* handle, pc_step_io* io, int phases, void* stream);
/* pc_train_step on a building layer the batch ships (a dataset's building counts; popcorn.py:113-114 with sentinelbuildings = False):
 * layer = the batch's building_counts, fp32 (B, 1, H, W), dense, on the device, 4-byte aligned (else PC_EINVAL); read, never written,
 * its payloads used bit for bit (NaN included).  The frozen extractor does not run at all -- no ingest of its domain, no forward, no
 * side-stream fork, on the shared 128 x 128 domain either: pc_sparsity_mask on the layer, the trainable U-Net alone, and the head
 * forward / backward multiply by the layer.  No building plane is allocated (io->off_building = -1, io->arena_needed shrinks).
 * layer == NULL is pc_train_step: the same bits, arena and launches.  Phases (io->dp): the pointer passed with PC_STEP_FWD is the one
 * PC_STEP_BWD reads, so the layer must stay unchanged until BWD has been enqueued; a BWD or UPD call passes the same pointer or NULL
 * (anything else: PC_EINVAL).  Refusals as pc_train_step, all before anything is enqueued.  No gradient with respect to the layer. */
int pc_train_step_layer(void* handle, pc_step_io* io, const float* layer, int phases, void* stream);
/* debug: host nanoseconds the LAST pc_train_step call spent in its sizing pass (out[0]) and in its launching pass (out[1])
 * (tools/host_time_eager.py); pc_forward records its two passes there as well */
void pc_debug_step_host_ns(double* out);

/* ---- native executor of ONE forward pass: inference and validation in one call -----------------------------------------------------
 *   model(sample, padding=False) in eval mode under no_grad with the dense head (popcorn.py:100-193):
 *   ingest -> building score from the frozen extractor on its 14-pixel reflect domain (on the shared domain, e.g. 100 x 100 tiles, the
 *   score and the features come from the grouped launches of both networks) -> the trainable U-Net on the add_padding(force=False)
 *   domain with nothing saved -> pc_head_fwd with mask = NULL: scale map, popdensemap, popcount.
 * The launches are those of pc_train_step's forward under unet_no_grad without everything a step adds: no selection flags, no sparsity
 * mask, no counts, no loss, no statistics (pc_head_fwd's stats = NULL).  popcount[b] sums the pixels with admin_mask == census_idx[b],
 * or every pixel when both are NULL (popcorn.py:189-190); one without the other is PC_EINVAL.  A model without the occupancy product
 * (plan.occupancymodel = 0) multiplies by a plane of ones the call fills in the arena, as the step does.  The building score is an
 * output (off_building).  layer != NULL replaces the extractor exactly as in pc_train_step_layer: fp32 (B, 1, H, W), dense, 4-byte
 * aligned (else PC_EINVAL), only read, its payloads used bit for bit; no plane is allocated and off_building = -1.
 * handle: from pc_step_create.  A plan whose gradient, optimiser, loss and statistics pointers (dw / db / dwt / dbt, head_dw, flat_p,
 * flat_g, adam_m, adam_v, hyper_dev, step_dev, norm_dev, stats_dev, loss_dev, g_scale_const_dev) are NULL is a valid INFERENCE plan:
 * pc_forward reads none of them.  A plan with ANY of flat_p, flat_g, adam_m, adam_v, loss_dev, stats_dev NULL is not a training plan:
 * pc_train_step* on such a handle returns PC_EINVAL before anything is enqueued (the others are not examined).  pc_forward works
 * on a copy of the handle's state: the context a training step keeps between its phases is not touched, so a FWD / BWD pair of a
 * data-parallel step survives a pc_forward call in between (on a handle of its own or on the same one, given an arena of its own).
 * An EAGER entry point like pc_train_step: small regions fork the extractor's chain onto the handle's side stream (measured per
 * caller's stream), so a capturing stream gets PC_ENOTSUP.  The arena is sized by a dry pass (arena_needed is always set; the
 * extractor's activations are released before the U-Net's are carved where the chain is not forked); outputs are valid until the next
 * call on that arena.  Refusals, all before anything is enqueued: bf16 mode, a one-stream (single-modality) plan -- which the training
 * entries take, this one does not --, B * H * W >= 2^31: PC_ENOTSUP;
 * the reflect rule of pc_train_step (a pad of either domain >= the side), NULL data, PC_DATA_SPLIT without data2, one of admin_mask /
 * census_idx alone, a misaligned layer: PC_EINVAL; an arena that is too small (or not 256-byte aligned): PC_ENOMEM. */
typedef struct pc_fwd_io {
    int32_t B, H, W, data_kind;                 /* enum pc_step_data */
    const void* data; const void* data2; int32_t craw, flags;      /* flags: 0, or PC_FWD_DENSE_ROW_RULE */
    const float* admin_mask; const int64_t* census_idx;   /* both NULL: popcount = plain sum (popcorn.py:189-190); both or neither */
    void* arena; int64_t arena_bytes;           /* as pc_step_io */
    /* results */
    int64_t arena_needed;
    int64_t off_popcount, off_popdense, off_scale, off_building;   /* off_building = -1 with a layer */
    int32_t launches, _pad2;
} pc_fwd_io;
/* PC_FWD_DENSE_ROW_RULE: the arena pads every row to 16 bytes, so the composed form of an Up block (pc_conv3x3_up_fwd_ok) is open at
 * every even width; a caller whose own tensors have dense rows composes only where the width is a multiple of 4 as well.  The two forms
 * round differently (the composed weights are products), so a binding that must return the bits of such a caller -- the per-launch
 * engine outside padded_rows() -- sets this flag and the decision is taken on dense rows; the arena's layout stays what it is.  It
 * matters on the extractor's (H + 28) x (W + 28) domain only: the U-Net's sides are multiples of 32. */
#define PC_FWD_DENSE_ROW_RULE 1
int pc_forward(void* handle, pc_fwd_io* io, const float* layer, void* stream);
/* sizeof(pc_fwd_io) as compiled (pc_sizeof's nine indices stay as they are) */
int pc_sizeof_fwd_io(void);

/* pc_reflect_pad_select / pc_select_normalize_pad / pc_ingest_split (planar form) for rows of any width and an output whose rows are
 * out_rstride >= Wp floats apart (planes of Hp * out_rstride): kind as enum pc_step_data; mean == NULL: no normalisation. */
int pc_ingest_pad_strided(int kind, const void* data, const void* data2, int Cin, float* out, int out_rstride, int B, int nsel,
                          const int* sel, const float* mean, const float* stdv, int H, int W, int top, int bottom, int left, int right,
                          void* stream);
/* p[0 .. n) = 0 by a kernel (zero fills inside a captured step must not be memset nodes: DESIGN.md); p 16-byte aligned */
int pc_zero_fill(float* p, int64_t n, void* stream);

/* ---- census aggregation + sliding-window stitching ----------------------- */

/* Region totals: sums[id] = sum of pred over pixels with boundary == id, id in [0, num_ids) (other ids, e.g. the -1
 * fill, are ignored); counts[id] (optional) = pixel count.  One pass instead of the per-census-row bbox-crop loop of
 * convert_popmap_to_census (data/PopulationDataset.py:705-712).  fp64 accumulation; pred/boundary: any 4-byte aligned
 * address (a row band of a larger map): scalar head up to the first 16-byte boundary, 16-byte reads from there. */
int pc_census_sum(const float* pred, const int32_t* boundary, int64_t n, int num_ids, double* sums, int32_t* counts,
                  void* stream);
/* Dasymetric adjustment, adjust_map_to_census (PopulationDataset.py:823-852): pred[i] *= pop[id] / float(sums[id]) for
 * regions with a census entry (has_entry[id] != 0, NULL = all) and a non-zero total. */
int pc_census_adjust(float* pred, const int32_t* boundary, int64_t n, int num_ids, const double* sums, const float* pop,
                     const uint8_t* has_entry, void* stream);
/* One sliding window of an M-member ensemble into the (H,W) device accumulators (run_eval.py:108-135): interior pixels
 * only (border of `overlap` excluded, PopulationDataset.py:656-672), window origin (yl,xl) = img_coords.
 * popdense/scale: [M][ps_y][ps_x] (scale may be NULL).  The interior is clipped to [0, H) x [0, W) on all four sides, so (yl, xl) may
 * be negative or lie beyond the raster; a window with ps <= 2 * overlap, or whose interior lies outside, adds nothing.  overlap < 0:
 * PC_EINVAL. */
int pc_stitch_accumulate(const float* popdense, const float* scale, int M, int ps_y, int ps_x, int overlap, int yl, int xl,
                         float* out_sum, float* out_sq, float* scale_sum, float* scale_sq, int16_t* count, int H, int W,
                         void* stream);
/* The visit counts of nwin windows that OTHER ranks computed (sharded sliding-window inference: every rank needs the complete count map,
 * run_eval.py:140-154), in one pass: count[r][c] += M for every window whose interior rows [x0, x1) x columns [y0, y1) cover (r, c).
 * win: DEVICE array of nwin x {x0, x1, y0, y1}; the kernel compares every (r, c) of the raster with them, so bounds below 0 or beyond the
 * raster clip themselves and no store leaves the map; overlapping interiors (the catch-up windows at the bottom /
 * right edge) add up.  No scratch plane, no atomics on the map. */
int pc_stitch_count_windows(const int32_t* win, int nwin, int M, int16_t* count, int H, int W, void* stream);
/* run_eval.py:140-154: where count > 1: sum -> mean, sq -> unbiased std; pixels visited once keep their raw values. */
int pc_stitch_finalize(float* out_sum, float* out_sq, float* scale_sum, float* scale_sq, const int16_t* count, int64_t n,
                       void* stream);

/* ---- product grid: cell x cell block sums of the 10 m maps (cell = 10: the hectare grid the reference's README recommends) ----
 * Cell grid anchored at raster pixel (0, 0): Hc = ceil(H / cell), Wc = ceil(W / cell); partial cells at the bottom / right edge sum what
 * exists.  cell >= 1, any value (no power of two needed, may exceed a window interior).  No floating-point atomics anywhere: within a
 * launch every coarse cell is written by exactly one lane in a fixed order, so equal inputs give equal bits.
 *
 * One sliding window of an M-member ensemble into the per-member planes cells[M][Hc][Wc]: for every member m and every interior pixel p
 * of the window inside the raster (interior and origin (yl, xl) as for pc_stitch_accumulate)
 *     cells[m][p.y / cell][p.x / cell] += popdense[m][p] / float(visits[p]).
 * visits: [H][W] visit count of ONE member over the WHOLE window list (seasons included), complete before the first window is added
 * (pc_stitch_count_windows with M = 1); it is not 0 anywhere inside an interior. */
int pc_product_accumulate(const float* popdense, int M, int ps_y, int ps_x, int overlap, int yl, int xl, const int16_t* visits, int H,
                          int W, int cell, float* cells, void* stream);
/* Over the M member totals T_m of each of the n cells of cells[M][n]: mean[i] = sum_m T_m / M, stdv[i] = sqrt(sum_m (T_m - mean)^2 /
 * (M - 1)), two passes in double (0 for M == 1). */
int pc_product_finalize(const float* cells, int M, int64_t n, float* mean, float* stdv, void* stream);
/* out[Hc][Wc] = the cell x cell sum pooling of map[H][W] (every cell of out is written). */
int pc_block_sum(const float* map, int H, int W, int cell, float* out, void* stream);

/* ---- census table: every member's census-unit totals, accumulated while the windows are stitched (csrc/census_table.hip) ----
 * The ensemble spread of a unit total is the spread over members of each member's own total, completed across windows with every pixel
 * weighted by 1 / its visit count: table[M][T] int64, T = sum of num_ids[l] over the L <= PC_CENSUS_MAX_LEVELS census levels, level l in
 * columns [off[l], off[l] + num_ids[l]).  Sums are 64-bit fixed point on a 2^-PC_CENSUS_FIX_SHIFT grid: integer addition is associative,
 * so equal inputs give equal bits for any window order, grid size and rank sharding (ranks add their tables with an exact int64 sum).
 * Range: every term in [0, 2^32), a unit total below 2^33 ~ 8.6e9 per member.
 *
 * One sliding window of an M-member ensemble (geometry as for pc_product_accumulate; an empty interior returns 0 without a launch):
 * for every interior pixel p inside the raster, member m and level l with id = boundaries[l][p] in [0, num_ids[l]) (other ids ignored)
 *     table[m][off[l] + id] += llrint((double)(popdense[m][p] / float(visits[p])) * 2^30)        (the quotient: one fp32 division).
 * A term that is NaN, +-Inf, negative or >= 2^32 adds nothing and sets bit 0 of the device word *flags (never a silent wrap).
 * boundaries / num_ids / off: HOST arrays of L entries; boundaries[l]: device int32 [H][W].  table and *flags are zeroed by the caller
 * before the first window. */
#define PC_CENSUS_MAX_LEVELS 4
#define PC_CENSUS_FIX_SHIFT 30
#define PC_CENSUS_MAX_PLANES 8
int pc_census_accumulate(const float* popdense, int M, int ps_y, int ps_x, int overlap, int yl, int xl, const int16_t* visits, int H,
                         int W, int L, const int32_t* const* boundaries, const int32_t* num_ids, const int32_t* off, int64_t* table,
                         int64_t T, int32_t* flags, void* stream);
/* totals[m][j] = (double)table[m][j] * 2^-30 (float64 [M][T]); mean[j] / stdv[j] (float32 [T]) over the members as pc_product_finalize:
 * two passes in double, the n - 1 form, 0 for M == 1. */
int pc_census_finalize(const int64_t* table, int M, int64_t T, double* totals, float* mean, float* stdv, void* stream);
/* K <= PC_CENSUS_MAX_PLANES per-unit tables painted onto the raster in one pass over the boundary plane:
 * out[k][i] = tables[k][boundary[i]] for boundary[i] in [0, num_ids), 0 elsewhere, i in [0, n).  tables / out: HOST arrays of K device
 * pointers (tables[k]: float32 [num_ids]).  boundary / out[k]: any 4-byte aligned address (a row band of a larger map): scalar head,
 * 16-byte loads and stores where aligned, scalar tail. */
int pc_census_paint(const int32_t* boundary, int64_t n, int num_ids, int K, const float* const* tables, float* const* out, void* stream);

/* ---- dasymetric adjustment across census levels on the census table, per member (csrc/census_adjust.hip) ----
 * adjust_map_to_census (data/PopulationDataset.py:823-852) scales every pixel of a unit c of level a by one factor POP[c] / P[c], so the
 * adjusted total of a unit f of another level l follows from the joint sums over (f, c) pairs; the pairs are one more id raster, filled
 * by pc_census_accumulate as one more level (num_ids = NP), and ride in the table's exact int64 all-reduce.
 *
 * Pair plan of two id rasters of n pixels (any 4-byte aligned address).  A pixel belongs to f = b_l[p] when 0 <= f < num_l and to
 * c = b_a[p] when 0 <= c < num_a; anything else is "no unit".  Two calls:
 *   pair_plane == NULL   partners[num_l][PC_CENSUS_PAIR_SLOTS] (16-byte aligned): the distinct c that share a pixel with f, ascending,
 *                        padded with -1; count[num_l]; flags[2] = {bit 0: a unit has more than PC_CENSUS_PAIR_SLOTS partners (its first
 *                        four are kept), the smallest such unit (INT32_MAX: none)}; scratch: int32 [num_l].
 *   pair_plane != NULL   pair_plane[p] = base[f] + k where partners[f][k] == c, -1 where f or c is no unit (or c is a fifth partner);
 *                        base[num_l + 1]: the exclusive prefix sum of count (the caller's); count / flags / scratch may be NULL.
 * The outputs are a function of the two rasters alone (integer minima; equal bits for every run). */
#define PC_CENSUS_PAIR_SLOTS 4
int pc_census_pair_plan(const int32_t* b_l, const int32_t* b_a, int64_t n, int num_l, int num_a, int32_t* partners, int32_t* count,
                        int32_t* flags, int32_t* scratch, const int32_t* base, int32_t* pair_plane, void* stream);
/* Adjusted totals of level l (columns [off_l, off_l + num_l) of table[M][T]) after the adjustment to level a (columns [off_a, off_a +
 * num_a)), with the pair columns [off_p, off_p + num_p), base[num_l + 1] and pair_c[num_p] (the c of every pair) of the plan, pop[num_a]
 * (float32, widened) and has[num_a] (uint8: the unit has a census row).  Per member m (every operation in double, rounded on its own):
 *     P[m][c]      = table[m][off_a + c]
 *     factor[m][c] = (double)pop[c] / ((double)P[m][c] * 2^-30)  when has[c] and P[m][c] > 0, else 1.0
 *     rem[m][f]    = table[m][off_l + f] - sum_k pair_k,  pair_k = table[m][off_p + base[f] + k]           (exact integer difference)
 *     adj[m][f]    = 2^-30 * ((double)rem + sum_k (double)pair_k * factor[m][c_k]),  k ascending
 * adj[M][f]: the adjustment of the ensemble-mean map -- the same formulas on the exact integer sums over members of P, pair and rem, with
 * factor[c] = ((double)pop[c] * M) / ((double)sum_m P * 2^-30), the result divided by M (the sums over members must stay below 2^63).
 * adj: float64 [M + 1][num_l]; mean / stdv: float32 [num_l] over rows 0 .. M - 1 as pc_census_finalize.
 * base == NULL: level a judged on itself (off_l == off_a, num_l == num_a): adj[m][c] = pop[c] where c is scaled, P[m][c] * 2^-30 where not. */
int pc_census_adjust_finalize(const int64_t* table, int M, int64_t T, int64_t off_l, int64_t off_a, int64_t off_p, int num_l, int num_a,
                              int64_t num_p, const int32_t* base, const int32_t* pair_c, const float* pop, const uint8_t* has,
                              double* adj, float* mean, float* stdv, void* stream);

/* ---- NaN fill of Sentinel inputs (data/PopulationDataset.py:526-551 interpolate_nan, scipy griddata "nearest") ----
 * x: contiguous fp32 (B, C, H, W), filled in place.  Per sample b, over its extent rows [0, h_b) x columns [0, w_b) (hw: DEVICE int32
 * [B][2] = {h_b, w_b}, NULL = the whole H x W; anchored top-left like the collate's zero padding; entries outside the extent are neither
 * read as sources nor written):
 *   - no NaN: untouched;
 *   - NaNs and fewer than 4 known (non-NaN; +-Inf is known) entries: the whole extent is zeroed;
 *   - otherwise every NaN at p = (c, i, j) takes the value of the known q minimising (|p - q|^2, q_c, q_i, q_j) lexicographically:
 *     Euclidean distance in 3-D index space, compared exactly in integers; the value is copied bit for bit.
 * counts: DEVICE int64 [B][2] receives {NaN entries, known entries} of each sample's extent (the 5 % orbit rule of
 * PopulationDataset.py:426,486 needs no second pass).  flags: PC_NAN_FILL_COUNT_ONLY = count, do not fill.
 * C <= PC_NAN_FILL_MAX_C, H, W <= PC_NAN_FILL_MAX_HW, B * C <= 65535.  ws: pc_nan_fill_ws_bytes(B, C, H, W) bytes of scratch.
 * Every launch after the count reads the counts and returns at once for a sample without NaN. */
#define PC_NAN_FILL_MAX_C 8
#define PC_NAN_FILL_MAX_HW 16384
#define PC_NAN_FILL_COUNT_ONLY 1
int64_t pc_nan_fill_ws_bytes(int B, int C, int H, int W);
int pc_nan_fill(float* x, const int32_t* hw, int64_t* counts, void* ws, int B, int C, int H, int W, int flags, void* stream);

/* ---- gradient w.r.t. the model input (autograd of the first convolution of each stream through add_padding and the channel reorder,
 * popcorn.py:109-156,231-258; networks.py:130-133) ----
 * For each of the n = 1 or 2 active streams s, from G_s = dL/d(first conv output) (already times relu' * bn scale of that layer):
 *   dXp_s[b,c,p,q]       = sum_{o<8} sum_{ky,kx<3} w_s[o,c,ky,kx] * G_s[b,o,p-ky+1,q-kx+1]        (G_s = 0 outside Hp x Wp)
 *   dX[b,chmap_s[c],h,w] = sum_{p: r_H(p)=h} sum_{q: r_W(q)=w} dXp_s[b,c,p,q]
 *   r_H(p) = |p-pt| if |p-pt| < H else 2(H-1) - (p-pt)                                              (likewise r_W with pl, W)
 * i.e. the data gradient of the conv folded back through the reflect padding (Hp = H + pt + pb, Wp = W + pl + pr; every pad <= extent - 1,
 * torch's reflect rule) and scattered through the channel gather -- the adjoint of the PC_SRC_REFLECT loader.  ONE launch, a gather: no
 * atomics, a fixed summation order (equal inputs give equal bits), every element of dX written exactly once with `=`.
 *   g    : PC_SRC_DIRECT source of 8 channels and extent Hp x Wp at (0, 0).  PC_PREC_FP32: planar fp32, any row / channel / batch strides;
 *          PC_PREC_BF16: channels-last bf16 (one 16-byte slot per pixel).
 *   w    : the layer's fp32 weight [8][cin][3][3], cin = 2 or 4.  PC_PREC_BF16: each weight is rounded to bf16 where it is used; the sums
 *          are fp32 and the result is not rounded.
 *   dx   : contiguous fp32 (B, Cx, H, W), Cx = 2, 4 or 6; the chmaps of the n streams must cover its channels exactly once.
 * Anything else returns PC_EINVAL before a launch. */
typedef struct pc_input_grad_desc {
    const pc_src* g; const float* w;
    int32_t cin;          /* 2 or 4 */
    int32_t chmap[4];     /* conv input channel c is channel chmap[c] of dx (c < cin) */
    int32_t _pad;
} pc_input_grad_desc;
int pc_input_grad(int n, const pc_input_grad_desc* d, float* dx, int B, int Cx, int H, int W, int pad_top, int pad_bottom, int pad_left,
                  int pad_right, void* stream);

/* ---- multi-unit census supervision: all listed census units of a crop in one step (csrc/units.hip) ----
 * The reference supervises one census unit per sample (popcorn.py:184-190,361-377).  A multi-unit batch lists K_b >= 1 units per sample and
 * is defined as the reference's result on the replicated batch (input[b], admin_mask[b], unit, y) of N = sum K_b samples with the same two
 * multinomial draws.  The lists arrive flattened: units = DEVICE int64 [N], non-negative, distinct and ASCENDING within each sample;
 * unit_off = DEVICE int32 [B + 1], sample b owns units[unit_off[b] .. unit_off[b + 1]), unit_off[0] = 0, unit_off[B] = N.  No compile-time
 * cap on K_b.  Ids compare as the one-unit kernels do, admin_mask == (float)id: ids above 2^24 that round to one float are one unit.
 *
 * pc_unit_mask, ONE launch (last-block ticket as pc_building_score_mask; must not run concurrently with itself on two streams of one
 * device).  building (B, 1, H, W), admin_mask (B, H, W) float ids, rowsel / colsel as for pc_sparsity_mask:
 *   slot[b,y,x]  int32: the flat index n in [0, N) of the listed unit of sample b that owns the pixel, else -1 (unlisted neighbours, the
 *                collate's -1 padding, the rotation's -1 fill, NaN)
 *   mask[b,y,x]  uint8 = slot >= 0 && (base || (rowsel[y] && colsel[x])), base = occupancymodel ? building > 0 : true  (popcorn.py:365-372
 *                with the union of the listed units as the region)
 *   counts       int32[2] = {nsel, nregion}; if the whole batch selects nothing, mask := slot >= 0 and nsel := nregion (popcorn.py:374-375)
 *   unit_pixels  optional (NULL) int32 [N]: pixels of each unit in the crop (exact integer atomics; one more tiny launch zeroes it)
 * B * H * W < 2^31.  16-byte accesses of four pixels per thread when W % 4 == 0 and the maps are 16-byte aligned, a scalar path otherwise. */
int pc_unit_mask(const float* building, const float* admin_mask, const int64_t* units, const int32_t* unit_off, const uint8_t* rowsel,
                 const uint8_t* colsel, int occupancymodel, int32_t* slot, uint8_t* mask, int32_t* counts, int32_t* unit_pixels,
                 int B, int H, int W, int N, void* stream);
/* popcount[n] = sum of popdense (B, H, W) over slot == n, n in [0, N): the N region sums of popcorn.py:186-188.  Bit-reproducible: each
 * term q is split exactly into trunc(q) and its fraction, the integer parts and the fractions rounded to a 2^-PC_CENSUS_FIX_SHIFT grid are
 * summed as two 64-bit integers per unit (associative: equal bits for any batch position of the sample, launch geometry and arrival
 * order), and popcount = float(double(int) + double(frac) * 2^-30).  Grid quantum q = 2^-30 per term: |popcount - exact sum| <=
 * 2^-24 |sum| + n_px(unit) * 2^-31 (+ 2^-53 relative from the double sum).  Range: |term| < 2^32, H * W < 2^27 -- the integers cannot
 * wrap; a term that is NaN, +-Inf or out of range makes its unit's popcount NaN, the other units are unaffected.  Pixels with slot outside
 * [0, N) add nothing.  unit_off (optional, as above): lets a workgroup keep bins in LDS in front of the global atomics where the
 * sample's K_b fits.  ws: pc_unit_ws_bytes(N) bytes, 16-byte aligned (zeroed by the call's first launch). */
int64_t pc_unit_ws_bytes(int64_t N);
int pc_unit_popcount(const float* popdense, const int32_t* slot, const int32_t* unit_off, float* popcount, void* ws, int B, int H, int W,
                     int N, void* stream);
/* The autograd of pc_unit_popcount: g_popdense[i] = slot[i] in [0, N) ? g_popcount[slot[i]] : 0 for i < n = B * H * W; every element is
 * written (no zero fill needed).  16-byte loads and stores when both maps are 16-byte aligned. */
int pc_unit_paint(const float* g_popcount, const int32_t* slot, float* g_popdense, int64_t n, int N, void* stream);

/* The flattened lists above from the caller's padded batch, ONE launch with one workgroup per sample row (what ops.unit_layout does with
 * a sort, a masked fill, three gathers, a scatter and a host-to-device copy).  census_idx (B, K) int64 and y (B, K) fp32 on the DEVICE;
 * census_n = HOST int32 [B], the valid count of each row, 1 <= census_n[b] <= K: the counts travel in the kernel arguments (no
 * host-to-device copy command).  Slots at or past census_n[b] are ignored whatever they hold.  Each row is sorted in LDS (a bitonic network
 * over (id, slot) pairs padded to a power of two; every trip count is fixed by K).  Writes, with N = sum census_n:
 *   units     int64 [N]      ascending per row             unit_off  int32 [B + 1]
 *   y_sorted  fp32 [N]       y in the sorted order         dest      int32 [N]: the flat (b, k) position, in the caller's order over the
 *                                                                     valid slots, of sorted slot n (popcount_caller[dest[n]] = popcount[n])
 *   ws        the first 20 * N bytes of the pc_unit_ws_bytes(N) workspace of the population sum := 0 (16-byte aligned; NULL: skipped), so
 *             that pc_unit_popcount_loss needs no zeroing launch
 * Duplicate ids inside the valid range break the contract of the lists; the call still terminates and stays in bounds.
 * Caps: K <= PC_UNIT_LAYOUT_MAX_K (the LDS id list of pc_unit_mask) and B <= PC_UNIT_LAYOUT_MAX_B (16-bit counts in the kernel-argument
 * block); beyond either the call returns PC_ENOTSUP before a launch and the caller keeps its own plumbing. */
#define PC_UNIT_LAYOUT_MAX_K 1024
#define PC_UNIT_LAYOUT_MAX_B 256
int pc_unit_layout(const int64_t* census_idx, const float* y, const int32_t* census_n, int B, int K, int64_t* units, int32_t* unit_off,
                   float* y_sorted, int32_t* dest, void* ws, void* stream);
/* pc_unit_popcount + pc_loss_fwd_bwd over the N (b, k) pairs (B := N, inv_B := 1 / N) in TWO launches instead of four: the accumulate
 * launch of pc_unit_popcount on a workspace that pc_unit_layout zeroed, then one block that finishes popcount_sorted[n] (the arithmetic of
 * pc_unit_popcount), writes the same value to popcount_caller[dest[n]] (optional, NULL) and runs the loss block on (popcount_sorted,
 * y_sorted).  Bit-identical to the two separate calls on the same inputs: same device functions, same order.  g_popcount [N] is in the
 * sorted order (what pc_unit_paint takes).  stats, lam4, loss_out, g_scale_const as for pc_loss_fwd_bwd. */
int pc_unit_popcount_loss(const float* popdense, const int32_t* slot, const int32_t* unit_off, const int32_t* dest, const float* y_sorted,
                          void* ws, float* popcount_sorted, float* popcount_caller, const double* stats, const float* lam4,
                          float scale_regularization, float lam_weak, int B, int H, int W, int N, float* loss_out, float* g_popcount,
                          float* g_scale_const, void* stream);

/* The device-N forms of the two entries above, for a step that is replayed from a captured graph or runs data parallel: nothing in a launch
 * depends on the counts.  Every buffer has the capacity Ncap = B * K and every launch runs at it.
 *
 * pc_unit_layout_dev: pc_unit_layout with census_n_dev = DEVICE int32 [B] (a loader rewrites it between replays).  The device cannot raise:
 * a count outside [1, K] is CLAMPED into [1, K] (a caller that wants an error validates on the host).  Same LDS sort and total order (a
 * valid INT64_MAX sorts in front of the padding); row b's offset is the sum of the clamped counts in front of it.  With N = the sum of the
 * clamped counts, every element of every output is written on every call:
 *   units [Ncap], y_sorted [Ncap], dest [Ncap]: entries [0, N) as pc_unit_layout; units[N..) = INT64_MAX, y_sorted[N..) = 0, dest[N..) = -1
 *   unit_off [B + 1], unit_off[B] = N
 *   ws        20 * Ncap bytes := 0: the sums' workspace LAID OUT BY Ncap (pc_unit_ws_bytes(Ncap); 16-byte aligned; NULL: skipped)
 *   n_dev     int32 [1] = N        stats (optional, NULL): stats[2] = (double)N, the local N next to {Nsel, sum scale} in stats[0..1]
 * Caps as pc_unit_layout (PC_ENOTSUP beyond them).  One workgroup per row; every trip count is fixed by (B, K). */
int pc_unit_layout_dev(const int64_t* census_idx, const float* y, const int32_t* census_n_dev, int B, int K, int64_t* units,
                       int32_t* unit_off, float* y_sorted, int32_t* dest, void* ws, int32_t* n_dev, double* stats, void* stream);
/* pc_unit_popcount_loss on a pc_unit_layout_dev result: the accumulate launch with the workspace laid out by Ncap, then ONE block that reads
 * N_local = n_dev[0] and N_global = stats[2] (the local N, or its sum after the caller's all-reduce of stats: an exact integer in a double),
 * forms inv_N = (float)(1.0 / N_global) in double arithmetic -- pc_unit_popcount_loss's host expression: with stats[2] = N_local the results
 * equal that entry's bit for bit --, finishes popcount_sorted[0..N_local), scatters it to popcount_caller[dest] (optional, NULL) and runs
 * the loss block over the N_local pairs with inv_N.  popcount_sorted, popcount_caller and g_popcount have Ncap elements; their tails
 * [N_local, Ncap) := 0, so pc_unit_paint runs with N := Ncap.  loss_out[0] is this rank's part of the global mean plus the regulariser. */
int pc_unit_popcount_loss_dev(const float* popdense, const int32_t* slot, const int32_t* unit_off, const int32_t* dest,
                              const float* y_sorted, void* ws, const int32_t* n_dev, float* popcount_sorted, float* popcount_caller,
                              const double* stats, const float* lam4, float scale_regularization, float lam_weak, int B, int H, int W,
                              int Ncap, float* loss_out, float* g_popcount, float* g_scale_const, void* stream);

/* ---- the native step executor for a multi-unit batch (csrc/step.hip) ----
 * pc_train_step for a batch whose samples list K units each: io as for pc_train_step, except that io->census_idx, io->y and
 * io->off_popcount are unused; the unit lists travel here.  Stage order: pc_unit_layout (on the stream whose chain ends in the mask) ->
 * ingest and networks as pc_train_step -> pc_outconv_sigmoid_crop -> pc_unit_mask -> pc_head_fwd on the union mask without a region ->
 * pc_unit_popcount_loss -> pc_unit_paint -> pc_head_bwd with g_popdense -> U-Net backward and update as pc_train_step.  popdensemap is
 * written at EVERY pixel by the head (0 * building where the mask does not select), which is what the unit sums rely on.  The unit sums,
 * the loss and popcount belong to the PC_STEP_BWD phase.  PC_ENOTSUP (nothing enqueued; the caller keeps the per-launch path): K or B
 * beyond pc_unit_layout's caps, io->dp != 0 (N differs per rank: the global mean needs a collective), a stream under capture, and what
 * pc_train_step declines. */
typedef struct pc_step_units {
    const int64_t* census_idx; const float* y;      /* DEVICE (B, K) */
    const int32_t* census_n;                        /* HOST [B]: valid units per row, 1 <= census_n[b] <= K */
    int32_t K, N;                                   /* N = sum census_n */
    /* results: byte offsets inside the arena, valid until the next call */
    int64_t off_slot;                               /* slot i32 [B][H][W] (pc_unit_mask) */
    int64_t off_popcount;                           /* popcount f32 [N] in the caller's (b, k) order */
} pc_step_units;
int pc_train_step_units(void* handle, pc_step_io* io, pc_step_units* u, int phases, void* stream);
/* ... on a given building layer (as pc_train_step_layer): pc_unit_layout -> pc_unit_mask on the layer -> the trainable U-Net alone ->
 * the multi-unit tail.  layer == NULL is pc_train_step_units. */
int pc_train_step_units_layer(void* handle, pc_step_io* io, pc_step_units* u, const float* layer, int phases, void* stream);

/* ---- region-resident training data (csrc/region.hip) ----
 * The reference's weaksup items are crops of a country's rasters around one census unit (data/PopulationDataset.py:403-458,624-649) and its
 * preprocessing makes the units' bounding boxes and pixel counts with one pass per unit (utils/02_preprocess_rwa_shapefile.py:142-161).
 *
 * pc_region_units: boundary = DEVICE int32 (h, w), h * w < 2^31.  table = DEVICE int32 [num_ids][5] = {xmin, xmax, ymin, ymax, count} in the
 * reference's convention -- x indexes rows, y indexes columns, xmax / ymax exclusive, five zeros for a unit without pixels.  Ids outside
 * [0, num_ids), negative ones included, contribute nothing; *stray (DEVICE int64) receives their pixel count.  Every element of table and
 * *stray is written.  ONE pass over the raster between an init and a finish launch over the table; integer min / max / add only, so the
 * table holds the same bits for any launch geometry.  16-byte loads when w % 4 == 0 and the raster is 16-byte aligned, scalar loads
 * otherwise.  max_blocks <= 0: the library's launch geometry; > 0: at most that many workgroups (tests of the geometry). */
int pc_region_units(const int32_t* boundary, int h, int w, int num_ids, int32_t* table, int64_t* stray, int max_blocks, void* stream);
/* pc_region_gather: the batch of B crops of the resident rasters, as the reference's collate would assemble it (PopulationDataset.py:885-958).
 *   s2        DEVICE (S, C2, h, w), fp32 or (s2_u16 != 0) uint16 digital numbers        s1  DEVICE fp32 (S, C1, h, w)
 *   boundary  DEVICE int32 (h, w)
 *   band_sel  HOST int32 [6]: the source band (0-based) of S2 output channels 0 .. 3 and of S1 output channels 0 .. 1
 *   crops     HOST int32 [B][5] = {x0, x1, y0, y1, season}: rows [x0, x1), columns [y0, y1) of season `season`
 *   s2_out (B, 4, Hm, Wm), s1_out (B, 2, Hm, Wm), admin_out (B, Hm, Wm) = (float)id: DEVICE fp32; data_hw DEVICE int32 (B, 2) = {x1 - x0, y1 - y0}
 * Every element of every output is written; outside a crop's extent (bottom, right) the padding is 0 / 0 / -1.  fp32 sources are copied
 * bit for bit (a NaN keeps its payload); uint16 converts exactly.  A crop that is empty, leaves the raster, exceeds (Hm, Wm) or names a season
 * >= S, a band outside its source, h * w or Hm * Wm >= 2^31: PC_EINVAL before anything is enqueued.  The crops travel in the kernel
 * arguments (no copy, no synchronisation): one launch per PC_REGION_GATHER_MAX_B crops.  16-byte stores when Wm % 4 == 0 and the outputs are
 * 16-byte aligned (loads at the sources' natural 4- / 2-byte alignment: crop origins are arbitrary), element by element otherwise. */
#define PC_REGION_GATHER_MAX_B 128
int pc_region_gather(const void* s2, int s2_u16, const float* s1, const int32_t* boundary, int S, int C2, int C1, int h, int w,
                     const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, float* s2_out, float* s1_out, float* admin_out,
                     int32_t* data_hw, void* stream);
/* pc_region_batch (csrc/region_batch.hip): the batch a fused step takes, assembled from the resident rasters in ONE launch per
 * PC_REGION_GATHER_MAX_B crops.  By definition, bit for bit (fp32 compared as integers, NaN payloads included):
 *   raw, admin_out  ==  pc_augment_raw( pc_region_gather(crops; Hm, Wm), vflip, hflip, rot, bright, beta, gam, gamma )
 * Sources, band_sel and crops as pc_region_gather takes them; (Hm, Wm) is the gathered tile and may exceed the batch maximum.  raw DEVICE
 * fp32 (B, 6, Ho, Wo), admin_out DEVICE fp32 (B, Ho, Wo) with (Ho, Wo) = (Hm, Wm) for even rot and (Wm, Hm) for odd rot.  The padding is
 * 0 / 0 / -1 in the gathered tile's coordinates (bottom, right) and sits wherever the flips and the rotation put it; the S2 value transform is
 * applied to it as pc_augment_raw applies it.  Every element of both outputs is written; every address is formed from a row and a column
 * clamped to the crop.  Even rot: a thread moves four consecutive pixels of an output row (aligned 16-byte stores when Wm % 4 == 0 and the
 * outputs are 16-byte aligned, loads at the sources' natural alignment, element by element across the crop's edge and otherwise); odd rot:
 * 32 x 32 tiles through LDS.  Crops, coins, band selection and items travel in the kernel arguments: no copy, no synchronisation.
 * labels (NULL: none) assembles the step's labels in the same launch:
 *   census_idx_out[b][k] = plan_cidx[items[b]][k],  y_out[b][k] = plan_y[items[b]][k]      for k < K,  1 <= K <= Kp
 * PC_EINVAL before anything is enqueued: everything pc_region_gather refuses, rot outside 0 .. 3, (Ho, Wo) other than stated above, an item
 * outside [0, n), K outside [1, Kp]. */
typedef struct pc_region_labels {
    const int64_t* plan_cidx;                       /* DEVICE int64 (n, Kp), uploaded once */
    const float* plan_y;                            /* DEVICE fp32 (n, Kp) */
    const int32_t* items;                           /* HOST [B]: the plan row of crop b */
    int64_t* census_idx_out;                        /* DEVICE int64 (B, K) */
    float* y_out;                                   /* DEVICE fp32 (B, K) */
    int32_t n, Kp, K, _pad;
} pc_region_labels;
int pc_region_batch(const void* s2, int s2_u16, const float* s1, const int32_t* boundary, int S, int C2, int C1, int h, int w,
                    const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, int vflip, int hflip, int rot, int bright, float beta,
                    int gam, float gamma, float* raw, float* admin_out, int Ho, int Wo, const pc_region_labels* labels, void* stream);

/* ---- NaN repair of a resident plan, planned once (csrc/region_repair.hip; data/PopulationDataset.py:419-441) ----
 * pc_region_gather_orbit / pc_region_batch_orbit: pc_region_gather / pc_region_batch with the S1 source chosen per crop.  s1_asc DEVICE fp32
 * (S, C1, h, w) or NULL; orbit HOST uint8 [B] or NULL (= all zero): crop b reads its two S1 bands from s1_asc where orbit[b] == 1 and from s1
 * where it is 0.  The choice travels as a 128-bit mask per launch in the kernel arguments.  pc_region_gather and pc_region_batch ARE the calls
 * with s1_asc = orbit = NULL.  PC_EINVAL before anything is enqueued: everything the plain entry points refuse, orbit[b] > 1, orbit[b] == 1
 * without s1_asc. */
int pc_region_gather_orbit(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit, const int32_t* boundary,
                           int S, int C2, int C1, int h, int w, const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm,
                           float* s2_out, float* s1_out, float* admin_out, int32_t* data_hw, void* stream);
int pc_region_batch_orbit(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit, const int32_t* boundary,
                          int S, int C2, int C1, int h, int w, const int32_t* band_sel, const int32_t* crops, int B, int Hm, int Wm, int vflip,
                          int hflip, int rot, int bright, float beta, int gam, float gamma, float* raw, float* admin_out, int Ho, int Wo,
                          const pc_region_labels* labels, void* stream);
/* pc_region_nan_census: counts[k] = {NaN entries of S2 over its four selected bands (a band listed twice counts twice; 0 for uint16 S2), of
 * s1 over its two selected bands, of s1_asc likewise (0 when s1_asc is NULL)} of box k.  boxes DEVICE int32 [n][5] = {x0, x1, y0, y1, season},
 * uploaded once by the caller (n runs to thousands: it does not travel in the kernel arguments); rows_max = the largest x1 - x0 of the list
 * (1 .. h; it sizes the launch: rows of a box beyond it are not counted).  counts DEVICE int64 [n][3], every element written (an init launch,
 * then one 64-bit atomic add of three lanes per workgroup).  The kernel clamps every box to the rasters and every season to [0, S): the list
 * is the caller's to validate, a bad one never makes an address outside the sources.  Integer adds only: the same bits for any launch
 * geometry; max_blocks as pc_region_units takes it.  Sources and band_sel as pc_region_gather; w < 2^29.  PC_EINVAL before anything is
 * enqueued for whatever pc_region_gather refuses of them. */
int pc_region_nan_census(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int S, int C2, int C1, int h, int w,
                         const int32_t* band_sel, const int32_t* boxes, int n, int rows_max, int64_t* counts, int max_blocks, void* stream);
/* The patch table of a gathered batch and its filled copy (pc_nan_fill): the entries whose 32-bit pattern differs, inside each item's extent
 * data_hw[b] = {h_b, w_b} (DEVICE int32, what pc_region_gather wrote), as idx = (c * h_b + i) * w_b + j in the item's own (6, h_b, w_b) space
 * (c = 0 .. 3: S2, 4 .. 5: S1; 6 * Hm * Wm < 2^31) and val = the filled tile's bits.  g2 / f2 DEVICE fp32 (B, 4, Hm, Wm), g1 / f1 (B, 2, Hm, Wm).
 *   pc_region_patch_count   counts[b][k] (DEVICE int32 [B][nchunk]) = differing entries of chunk k (PC_REGION_PATCH_CHUNK entries of the index
 *                           space) of item b; nchunk = ceil(6 * Hm * Wm / PC_REGION_PATCH_CHUNK); every element written
 *   pc_region_patch_write   chunk_off[b][k] (DEVICE int64: the exclusive prefix of the counts, taken by the caller, + the item's base in the
 *                           table): the entries of chunk k go to idx / val [chunk_off[b][k] ...) in ascending order of idx, so the entries of an
 *                           item ascend.  Nothing is written at or beyond cap (the table's length).
 * Deterministic: an entry's place is a function of the data alone (wave ballots, no atomics). */
#define PC_REGION_PATCH_CHUNK 4096
int pc_region_patch_count(const float* g2, const float* f2, const float* g1, const float* f1, const int32_t* data_hw, int B, int Hm, int Wm,
                          int32_t* counts, int nchunk, void* stream);
int pc_region_patch_write(const float* g2, const float* f2, const float* g1, const float* f1, const int32_t* data_hw, int B, int Hm, int Wm,
                          const int64_t* chunk_off, int nchunk, int32_t* idx, float* val, int64_t cap, void* stream);
/* pc_region_patch_apply: lays the patches of B batch items over an assembled batch.  idx / val DEVICE tables of cap entries; per item b, HOST:
 * off[b] (int64) and count[b] (int32) = its range in the table, item_hw[b] = {h_b, w_b}.  Entry (c, i, j, val) is stored at the image of tile
 * position (i, j) under vflip, then hflip, then rot quarter turns of the (Hm, Wm) tile -- (Ho, Wo) as pc_region_batch --, as
 * pc_aug_s2_value(val, bright, beta, gam, gamma) for c < 4 and as val for c >= 4:
 *   s2 + b * s2_stride + c * Ho * Wo + i' * Wo + j'        s1 + b * s1_stride + (c - 4) * Ho * Wo + i' * Wo + j'        (strides in elements)
 * which serves raw (B, 6, Ho, Wo) (s1 = raw + 4 * Ho * Wo, both strides 6 * Ho * Wo) and separate S2 / S1 tensors alike.  By definition, bit
 * for bit:  patch_apply(pc_region_batch_orbit(crops, orbit, coins)) == pc_augment_raw(pc_nan_fill(pc_region_gather_orbit(crops, orbit)), coins).
 * Plain 4-byte stores on `stream`, no synchronisation; a launch takes up to PC_REGION_GATHER_MAX_B items (their ranges travel in the kernel
 * arguments), none is made for items without entries.  PC_EINVAL before anything is enqueued: a range outside [0, cap], an item with entries
 * whose extent is empty or exceeds (Hm, Wm), (Ho, Wo) other than stated, rot outside 0 .. 3, a stride smaller than the planes it spans. */
int pc_region_patch_apply(const int32_t* idx, const float* val, int64_t cap, const int64_t* off, const int32_t* count, const int32_t* item_hw,
                          int B, float* s2, int64_t s2_stride, float* s1, int64_t s1_stride, int Hm, int Wm, int Ho, int Wo, int vflip,
                          int hflip, int rot, int bright, float beta, int gam, float gamma, void* stream);
/* pc_region_window (csrc/region_crop.hip; the kernel of pc_region_item below: a window is a square item without the admin plane whose
 * workgroup ranges are blocks of whole rows): the normalised model input of ONE evaluation window of the resident rasters in ONE launch.
 * out DEVICE fp32 (6, ps, ps), channels [S2 R G B NIR | S1 VV VH]:  out[c][i][j] = (v - mean6[c]) / std6[c]  (the fp32 division of
 * pc_select_normalize), v = the value of the patch table where its slice [start, start + count) holds an entry for the site, otherwise the
 * raster's value at (season, band_sel[c], x + i, y + j); orbit 1 reads the two S1 channels from s1_asc.  Sources and band_sel as
 * pc_region_gather.  idx / val DEVICE tables of cap entries as pc_region_patch_write makes them: the slice ascends, idx = (c * ps + i) * ps + j
 * in the window's own (6, ps, ps) space, val = the raw, un-normalised repaired value; both may be NULL with count = 0.  By definition, on
 * every non-NaN element and with NaN at the same sites:
 *   pc_region_window(window, orbit; no table) == pc_select_normalize(cat(S2, S1 of pc_region_gather_orbit(window, orbit)), 0 .. 5, mean6, std6)
 * Every element of out is stored exactly once, the patch value before the normalisation; nothing outside out is written.  16-byte accesses
 * when ps % 4 == 0 and out is 16-byte aligned, element by element otherwise.  A workgroup owns pc_region_window_rows(ps) rows of one
 * channel (0 for a ps the launch refuses).  PC_EINVAL before anything is enqueued: a NULL pointer, ps < 1 or > PC_REGION_WINDOW_MAX_PS, a
 * window that leaves the raster, a season outside [0, S), a band outside its source, an orbit outside {0, 1} or 1 without s1_asc, count > 0
 * without tables, a slice outside [0, cap] or longer than 6 * ps * ps. */
#define PC_REGION_WINDOW_MAX_PS 8192
int pc_region_window_rows(int ps);
int pc_region_window(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, int S, int C2, int C1, int h, int w,
                     const int32_t* band_sel, int x, int y, int season, int ps, const float* mean6, const float* std6, const int32_t* idx,
                     const float* val, int64_t cap, int64_t start, int64_t count, float* out, void* stream);
/* pc_region_item (csrc/region_crop.hip): the normalised model input AND the admin mask of ONE rectangular crop {x0, x1, y0, y1, season} of
 * the resident rasters (rows [x0, x1), columns [y0, y1); hc = x1 - x0, wc = y1 - y0) in ONE launch -- a validation item.
 * out DEVICE fp32 (6, hc, wc), channels [S2 R G B NIR | S1 VV VH]:  out[c][i][j] = (v - mean6[c]) / std6[c]  (the fp32 division of
 * pc_select_normalize), v = the value of the patch table where its slice [start, start + count) holds an entry for the site, otherwise the
 * raster's value at (season, band_sel[c], x0 + i, y0 + j); orbit 1 reads the two S1 channels from s1_asc; uint16 S2 converts exactly.
 * admin_out DEVICE fp32 (hc, wc) = (float)boundary[x0 + i][y0 + j].  Sources and band_sel as pc_region_gather.  idx / val DEVICE tables of
 * cap entries as pc_region_patch_write makes them: the slice ascends, idx = (c * hc + i) * wc + j in the item's own (6, hc, wc) space, val =
 * the raw, un-normalised repaired value; both may be NULL with count = 0.  By definition, bit for bit on every non-NaN element and with NaN
 * at the same sites:
 *   out       == pc_select_normalize(cat(S2, S1 of patch_apply(pc_region_gather_orbit({crop}, orbit))), 0 .. 5, mean6, std6)
 *   admin_out == admin_mask of that gather (B = 1: no padding)
 * Every element of both outputs is stored exactly once, the patch value before the normalisation; nothing outside them is written.  There
 * is no cap on a side: a workgroup owns a contiguous range of PC_REGION_ITEM_TILE elements of one plane's hc * wc index space, which need
 * not end on a row boundary (an entry's place is checked against that range whatever the table holds).  16-byte accesses when wc % 4 == 0
 * and both outputs are 16-byte aligned, element by element otherwise.  PC_EINVAL before anything is enqueued: a NULL pointer, an empty crop
 * or one that leaves the raster, 6 * hc * wc >= 2^31, a season outside [0, S), a band outside its source, an orbit outside {0, 1} or 1
 * without s1_asc, count > 0 without tables, a slice outside [0, cap] or longer than 6 * hc * wc, misaligned pointers. */
#define PC_REGION_ITEM_TILE 4096
int pc_region_item(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary, int S, int C2, int C1,
                   int h, int w, const int32_t* band_sel, int x0, int x1, int y0, int y1, int season, const float* mean6, const float* std6,
                   const int32_t* idx, const float* val, int64_t cap, int64_t start, int64_t count, float* out, float* admin_out,
                   void* stream);

/* ---- the building layer a dataset ships (data/PopulationDataset.py:606-612; popcorn.py:112-114) ----
 * A building layer is an fp32 raster without a season axis: resident (h, w) for the region entry points, (B, 1, H, W) in a batch.  It
 * follows the admin mask's geometry (crop, flips, quarter turns; utils/utils.py:182-209), its padding is the collate's 0.0
 * (PopulationDataset.py:909-956), and it gets no value transform, no normalisation and no repair: payloads arrive bit for bit, NaN included.
 * Each `_layer` entry point below IS the code of the entry point it is named after, which is its call with layer = layer_out = NULL:
 *   pc_augment_raw_layer     layer (B, 1, H, W) -> layer_out (B, 1, Ho, Wo), the map of admin_out
 *   pc_region_gather_layer   layer DEVICE (h, w) -> layer_out (B, 1, Hm, Wm), 0.0 outside the crop (pc_region_gather_orbit's other arguments)
 *   pc_region_batch_layer    layer DEVICE (h, w) -> layer_out (B, 1, Ho, Wo) == the layer of
 *                            pc_augment_raw_layer( pc_region_gather_layer(...) ), bit for bit (pc_region_batch_orbit's other arguments)
 *   pc_region_window_layer   layer DEVICE (h, w) -> layer_out (ps, ps), the raster's slice: one more blockIdx.y plane of the same launch
 *   pc_region_item_layer     layer DEVICE (h, w) -> layer_out (hc, wc), likewise
 * PC_EINVAL before anything is enqueued, besides what the plain entry point refuses: layer without layer_out, layer_out without layer,
 * either misaligned for fp32.  The 16-byte forms are taken only when layer_out is 16-byte aligned as well. */
int pc_augment_raw_layer(const float* s2, const float* s1, const float* admin, const float* layer, float* raw, float* admin_out,
                         float* layer_out, int B, int H, int W, int vflip, int hflip, int rot, int bright, float beta, int gam, float gamma,
                         void* stream);
int pc_region_gather_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit, const int32_t* boundary,
                           const float* layer, int S, int C2, int C1, int h, int w, const int32_t* band_sel, const int32_t* crops, int B,
                           int Hm, int Wm, float* s2_out, float* s1_out, float* admin_out, float* layer_out, int32_t* data_hw, void* stream);
int pc_region_batch_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, const uint8_t* orbit, const int32_t* boundary,
                          const float* layer, int S, int C2, int C1, int h, int w, const int32_t* band_sel, const int32_t* crops, int B,
                          int Hm, int Wm, int vflip, int hflip, int rot, int bright, float beta, int gam, float gamma, float* raw,
                          float* admin_out, float* layer_out, int Ho, int Wo, const pc_region_labels* labels, void* stream);
int pc_region_window_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const float* layer, int S, int C2,
                           int C1, int h, int w, const int32_t* band_sel, int x, int y, int season, int ps, const float* mean6,
                           const float* std6, const int32_t* idx, const float* val, int64_t cap, int64_t start, int64_t count, float* out,
                           float* layer_out, void* stream);
int pc_region_item_layer(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int orbit, const int32_t* boundary,
                         const float* layer, int S, int C2, int C1, int h, int w, const int32_t* band_sel, int x0, int x1, int y0, int y1,
                         int season, const float* mean6, const float* std6, const int32_t* idx, const float* val, int64_t cap, int64_t start,
                         int64_t count, float* out, float* admin_out, float* layer_out, void* stream);

/* ---- the resident atlas: several resident regions, one launch per batch (csrc/region_atlas.hip; run_train.py:423-431) ----
 * An atlas is R resident regions, 1 <= R <= PC_ATLAS_MAX_REGIONS, each with its own rasters, extent, season count, band counts and band
 * selection; a batch whose crops come from different regions is still one launch per PC_REGION_GATHER_MAX_B crops.
 * pc_atlas_create: regions HOST [R]; s2_u16 is one flag for the whole atlas (mixed S2 types are not part of it).  Per region everything
 * pc_region_gather_layer validates of its sources (s1_asc and layer may be NULL); a layer on all regions or on none.  The handle keeps a
 * host copy of the descriptors and uploads a device copy once, on the current device: the only copy and the only synchronisation.
 * pc_atlas_gather: crop b = crops[b] = {x0, x1, y0, y1, season} of region region_of[b] (HOST uint8 [B]); orbit HOST uint8 [B] or NULL.
 * Outputs, padding (0 / 0 / -1 / 0.0) and the rule of the 16-byte forms are pc_region_gather_layer's.  By definition, bit for bit (fp32
 * compared as integers, NaN payloads kept):
 *   row b of pc_atlas_gather == row 0 of pc_region_gather_layer on region region_of[b] alone with crop b, orbit[b] and the tile (Hm, Wm)
 * pc_atlas_batch: the one-launch assembly of pc_region_batch_layer with a region per crop:
 *   raw, admin_out, layer_out == pc_augment_raw_layer( pc_atlas_gather(...; Hm, Wm), coins )
 * plus the label rows as pc_region_batch writes them; labels->items index ONE plan table, the regions' tables concatenated.
 * With R = 1 both equal the single-region entry points on every output.
 * PC_EINVAL before anything is enqueued: everything the single-region entry points refuse; region_of[b] >= R; a crop or season that is
 * invalid in its OWN region's (h, w, S), even if another region of the atlas would hold it; orbit[b] == 1 for a region without s1_asc;
 * layer_out when the atlas has no layer, and no layer_out when it has one. */
#define PC_ATLAS_MAX_REGIONS 16
typedef struct pc_atlas_region {
    const void* s2;                                 /* DEVICE (S, C2, h, w) fp32 or uint16 */
    const float* s1;                                /* DEVICE fp32 (S, C1, h, w) */
    const float* s1_asc;                            /* DEVICE fp32 (S, C1, h, w) or NULL */
    const int32_t* boundary;                        /* DEVICE int32 (h, w) */
    const float* layer;                             /* DEVICE fp32 (h, w) or NULL: on all regions of an atlas or on none */
    int32_t S, C2, C1, h, w;
    int32_t band_sel[6];
    int32_t _pad;
} pc_atlas_region;
int pc_sizeof_atlas_region(void);
int pc_atlas_create(const pc_atlas_region* regions, int R, int s2_u16, void** handle);
void pc_atlas_destroy(void* handle);
int pc_atlas_gather(void* handle, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int B, int Hm, int Wm,
                    float* s2_out, float* s1_out, float* admin_out, float* layer_out, int32_t* data_hw, void* stream);
int pc_atlas_batch(void* handle, const uint8_t* region_of, const int32_t* crops, const uint8_t* orbit, int B, int Hm, int Wm, int vflip,
                   int hflip, int rot, int bright, float beta, int gam, float gamma, float* raw, float* admin_out, float* layer_out, int Ho,
                   int Wo, const pc_region_labels* labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POPCORN_HIP_H */
