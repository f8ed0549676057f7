// step.hip -- native executor of one training step (pc_train_step): the body of the reference's inner loop
// (run_train.py:186-238: forward(train, padding=False, sparse=True) -> get_loss -> x lam_weak -> backward -> clip -> Adam) issued from
// C++ for ANY batch geometry and truncation regime.  Host code only: it computes geometry, carves tensors out of the caller's arena,
// fills the descriptors of the entry points of this library (popcorn_hip.h) and calls them.  The Python engine (popcorn_amd/engine.py)
// issues the same launches one ctypes call at a time; at the reference's real training geometry (weak_batch_size = 2 census regions of
// varying size) those ~45 calls cost more host time than a small region's kernels take.
//
// Layout rules of the arena (what makes every launch take its fast path whatever the region's width):
//   * planar fp32 activations (B, C, H, W) with rows padded to a multiple of 4 floats: every row starts on a 16-byte boundary, so the
//     conv kernels keep the aligned staged loaders and vector epilogues on the building extractor's (H + 28) x (W + 28) domain too
//     (the pad columns are never read as data);
//   * the up-sampled map of an Up block is allocated with the extent and strides of the skip tensor it is concatenated with (the
//     transposed conv fills the top-left 2h x 2w of it): the two-source conv then sees two sources of identical layout;
//   * a pooled source is handed over cropped to even extents (MaxPool2d(2) floors).
//
// A multi-unit batch (pc_train_step_units, Step::un / Step::U: K census units per crop, units.hip) takes the same path with another
// tail around the head: unit lists -> score -> unit mask -> head without a region -> unit sums + loss -> paint -> head backward on
// g_popdense; everything between ingest and the U-Net update is shared, and a one-unit call (un == nullptr) issues what it always did.
//
// A one-stream plan (popcorn_hip.h: an S1-only / S2-only model; Step::ns / ps / cs) takes the same path over the present streams: every
// per-stream loop and grouped launch runs over Step::ns of them, the feature map keeps its 16 channels with the absent stream's 8 zeroed
// (zero_chans_kernel), the building score is the stream's own out conv over its 8 channels, and the head's 64 x 8 first layer travels
// through 64 x 16 images in the arena (head_w0_embed_kernel, head_dw0_extract_kernel).  A dual-stream plan issues what it always did.
//
// The backward pass (struct Backward) is the network in reverse, one function per U-Net block, to be read next to engine.py: _Backward.
// It has the COMPOSED form of the two Up blocks only: the trainable U-Net works on the add_padding domain, whose sides are multiples of
// 32 (pad_geometry), so both levels have exact 2x geometry, widths that are multiples of 16 and 16-byte rows -- everything the composed
// forward and backward ask for.  forward_nets refuses (PC_ENOTSUP, in the sizing pass) a network that saves activations otherwise.
// One launch leaves its block: inc2's output a2 feeds both up1a (skip) and, through the max-pool, d1a, so its gradient has two sources.
// With the encoder trained, up(UP1) holds its skip launch back (pool_add_plan); down(DOWN1) runs d1a as a plain launch into a gradient at
// the pooled resolution and issues the skip launch after it, with that gradient as pool_grad: the scatter is added in the epilogue and
// a2's gradient is written once, not written and then read, added to and written again.  Under encoder_no_grad the order is the old one.
// Level 2 likewise: up(UP2) holds its skip-halves launch back (pool_add_plan2), level2() runs the whole-level kernel with pool_grad_out
// and issues the halves after it, each with its 8-channel slice of that gradient.
#include "common.h"
#include <chrono>

#include <string.h>
#include <new>

namespace {

enum { L_INC1 = 0, L_INC2, L_D1A, L_D1B, L_D2A, L_D2B, L_UP2A, L_UP2B, L_UP1A, L_UP1B };
enum { T_UP2 = 0, T_UP1 = 1 };
constexpr int MAXK = PC_MAX_GROUP;        // (network, stream) pairs of one grouped launch
constexpr long long PC_STEP_SIDE_PX_DEFAULT = 1ll << 40;      // pixels (B * Hp * Wp) up to which the extractor's chain runs on the side stream

// ---- tensors ------------------------------------------------------------------------------------------------------------------------
struct Ten {                               // planar fp32 view (B, C, H, W)
    float* p = nullptr;
    int B = 0, C = 0, H = 0, W = 0;
    int64_t sb = 0, sc = 0;
    int sr = 0;
    bool ok() const { return p != nullptr; }
};

inline pc_src S(const Ten& t, int mode = PC_SRC_DIRECT, int oy = 0, int ox = 0) {
    pc_src s{};
    s.ptr = t.p; s.C = t.C; s.H = t.H; s.W = t.W; s.bstride = t.sb; s.cstride = t.sc; s.rstride = t.sr;
    s.mode = mode; s.oy = oy; s.ox = ox; s.chmap[0] = 0; s.chmap[1] = 1; s.chmap[2] = 2; s.chmap[3] = 3;
    s.dtype = PC_F32; s.xstride = 1;
    return s;
}
inline pc_dst D(const Ten& t) {
    pc_dst d{};
    d.ptr = t.p; d.bstride = t.sb; d.cstride = t.sc; d.rstride = t.sr; d.dtype = PC_F32; d.xstride = 1;
    return d;
}
inline Ten chans(const Ten& t, int c0, int n) {      // t[:, c0:c0 + n]
    Ten v = t;
    v.p = t.p + (int64_t)c0 * t.sc;
    v.C = n;
    return v;
}
inline Ten crop(const Ten& t, int H, int W) {        // t[:, :, :H, :W]
    Ten v = t;
    v.H = H; v.W = W;
    return v;
}

struct Arena {
    char* base = nullptr;
    int64_t cap = 0, off = 0, peak = 0;
    bool dry = true;
    void* raw(int64_t bytes) {
        off = (off + 255) & ~(int64_t)255;
        char* p = base + off;
        off += bytes;
        if (off > peak) peak = off;
        return p;
    }
    Ten act(int B, int C, int H, int W, bool dense = false) {
        Ten t;
        t.B = B; t.C = C; t.H = H; t.W = W;
        t.sr = dense ? W : (W + 3) & ~3;
        t.sc = (int64_t)H * t.sr;
        t.sb = (int64_t)C * t.sc;
        t.p = reinterpret_cast<float*>(raw((int64_t)B * t.sb * (int64_t)sizeof(float)));
        return t;
    }
};

// ---- the executor -------------------------------------------------------------------------------------------------------------------
struct Saved {                 // activations of one (network, stream) pair that the backward pass reads
    Ten a1, a2, b1, b2, c1, c2, e1, e2, f1, pa2, pb2;
    void* ws_up1 = nullptr;    // composed operand images of the two Up blocks (never null: forward_nets)
    void* ws_up2 = nullptr;
};

struct Step {
    pc_step_plan plan;
    pc_bn bn_nobias[2][PC_STEP_CONVS];          // trainable network: ReLU / BN factor of a layer's output (no conv bias)
    pc_bn bn_half[2][2];                        // d1b's factor for the two 8-channel halves of its output (pointers into the same BN tensors)
    pc_bn bn_half_d1a[2][2];                    // ... and d1a's (the fused backward of d1b runs per 8-channel half of its input)
    float* ones2 = nullptr;                     // device {1, 1}: weights of the partial-logit sum
    // the streams that are present (popcorn_hip.h: a one-stream plan has the table of the absent stream all zero in both networks).
    // Everything per stream below -- cs, bn_nobias, bn_half, bn_half_d1a, sv -- is indexed by the position in ps, not by the stream
    int ns = 2;
    int ps[2] = {0, 1};
    pc_step_stream cs[2];                       // the trainable network's tables of the present streams
    pc_bn feat_bn[2];                           // ReLU / BN factor of the two halves of the feature map (absent stream: plain, its half is zero)
    // one-stream plan: the 64 x 16 images of the head's first layer in the arena (head_w[0] / head_dw[0] of the plan are 64 x 8)
    float* w0_img = nullptr;
    float* dw0_img = nullptr;
    const float* hw[8];                         // the head's tensors and gradient targets as its kernels get them (set by forward())
    float* hdw[8];
    // small regions: the frozen extractor's forward chain runs on a side stream next to the trainable U-Net's (two chains of ~13 small,
    // latency-bound launches each; at B = 64 tiles -- a full chip per launch -- every multi-stream attempt lost)
    hipStream_t side = nullptr;
    hipStream_t side_for = nullptr;             // the caller's stream the side stream was measured against (pick_side_stream)
    bool side_picked = false;
    struct SideFor { hipStream_t caller; hipStream_t side; } side_cache[4] = {};     // measured pairs (caller's stream -> its side stream)
    int n_side_cache = 0;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_dep[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int ev_next = 0;
    int64_t side_px = 0;                        // use the side stream when B * Hp * Wp <= side_px
    int64_t side_bwd_px = 0;                    // backward: the weight-gradient-only launches on the side stream up to this many pixels
    // context of the step between its phases
    bool have_fwd = false;
    int B = 0, H = 0, W = 0, pt = 0, pl = 0, Hp = 0, Wp = 0;
    Ten feats, building, Xp_u;
    const float* layer = nullptr;               // the batch's building layer of this call (pc_train_step_layer; null: the extractor's score)
    const float* fwd_layer = nullptr;           // ... of the forward pass in the arena
    const float* bld = nullptr;                 // the plane the head multiplies by: the score, the layer, or ones (no occupancy product)
    uint8_t* mask = nullptr;
    const uint8_t* sel = nullptr;               // device selection flags of this step (io.sel, or unpacked from io.sel_host)
    int32_t* counts = nullptr;
    float* popcount = nullptr;
    float* popdense = nullptr;
    float* scale_map = nullptr;
    float* g_pc = nullptr;
    void* head_ws = nullptr;
    Saved sv[2];
    bool unet_ng = false, enc_ng = false, deferred_popcount = false;
    // multi-unit batch (pc_train_step_units; null: one unit per sample): the lists of the call, and what forward() carved for them
    pc_step_units* un = nullptr;
    bool fwd_units = false;                     // the forward pass in the arena was a multi-unit one
    struct Units {
        int64_t* units = nullptr; int32_t* unit_off = nullptr; float* y_sorted = nullptr; int32_t* dest = nullptr;
        void* ws = nullptr; int32_t* slot = nullptr; float* pc_sorted = nullptr; float* pc_caller = nullptr; float* g_pc = nullptr;
        int N = 0;
    } U;
    int64_t fwd_end = 0;                        // arena offset behind the forward pass's tensors
    // per call
    Arena ar;
    hipStream_t st = nullptr;
    int launches = 0;
    int err = 0;
    bool infer = false;                         // pc_forward: the dense no-grad forward -- no mask, no selection, no loss context
    bool dense_rule = false;                    // pc_forward(PC_FWD_DENSE_ROW_RULE): compose the Up blocks only where dense rows would be aligned

    bool go() const { return !ar.dry && err == 0; }
    bool one() const { return ns == 1; }
    void rc(int code) {
        if (code != 0 && err == 0) err = code;
        ++launches;
    }
};

// a stream's table is either filled or all zero (popcorn_hip.h: one-stream plan)
inline bool stream_present(const pc_step_stream& t) { return t.cin >= 1 && t.w[0] != nullptr; }

// the streams of a training plan: the same ones in both networks, at least one; a one-stream plan needs its feature half named (0 / 8)
// and room for its channels in the 4-entry chan[]
inline int plan_streams_ok(const pc_step_plan& P) {
    int n = 0;
    for (int s = 0; s < 2; ++s) {
        const bool u = stream_present(P.unet.s[s]), e = stream_present(P.extractor.s[s]);
        if (u != e) return PC_EINVAL;
        if (!u) continue;
        ++n;
        if (P.unet.s[s].cin > 4 || P.unet.s[s].cin != P.extractor.s[s].cin) return PC_EINVAL;
    }
    if (n == 0) return PC_EINVAL;
    if (n == 1)
        for (int s = 0; s < 2; ++s) {
            if (!stream_present(P.unet.s[s])) continue;
            const int f0 = P.unet.s[s].feat_c0;
            if ((f0 != 0 && f0 != 8) || P.extractor.s[s].feat_c0 != f0) return PC_EINVAL;
        }
    return 0;
}

inline void pad_geometry(int H, int W, int& pt, int& pb, int& pl, int& pr) {          // add_padding(force=False), popcorn.py:231-258
    pt = pb = pl = pr = 0;
    if (H % 32 != 0) { pt = (64 - H % 64) / 2; pb = (64 - H % 64) - pt; }
    if (W % 32 != 0) { pl = (64 - W % 64) / 2; pr = (64 - W % 64) - pl; }
}

// the per-step selection flags from HOST memory: bit-packed into the kernel arguments of a one-block launch that writes them as bytes
struct SelBits { uint32_t w[PC_STEP_SEL_MAX / 32]; };
__global__ __launch_bounds__(256) void sel_unpack_kernel(const SelBits b, uint8_t* out, int n) {
    for (int i = threadIdx.x; i < n; i += 256) out[i] = (b.w[i >> 5] >> (i & 31)) & 1u;
}

// the plane of ones the head multiplies by in a model without the occupancy product (train.py: torch.ones_like(building))
__global__ __launch_bounds__(256) void ones_fill_kernel(float* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 1.f;
}

// ---- one-stream plan (S1-only / S2-only model): the head kernels keep their 16-channel form, the absent stream's half is zero ----------
// the dead 8 channels of the dense (B, 16, Hp, Wp) feature map (the arena's contents are undefined)
__global__ __launch_bounds__(256) void zero_chans_kernel(float* p, int64_t bstride, int64_t per_b, int B) {
    const int64_t n = per_b * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per_b;
        p[b * bstride + (i - b * per_b)] = 0.f;
    }
}

// the head's first layer w0 (64 x 8) at columns [c0, c0 + 8) of a zeroed 64 x 16 image (model.head_tensors of the per-launch step)
__global__ __launch_bounds__(256) void head_w0_embed_kernel(const float* __restrict__ w0, float* __restrict__ img, int c0) {
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
        const int r = i >> 4, c = (i & 15) - c0;
        img[i] = (c >= 0 && c < 8) ? w0[r * 8 + c] : 0.f;
    }
}

// ... and back: the live half of the first layer's 64 x 16 gradient image -> the parameter's gradient (model.head_grad_targets: fix)
__global__ __launch_bounds__(256) void head_dw0_extract_kernel(const float* __restrict__ img, float* __restrict__ dw0, int c0) {
    for (int i = threadIdx.x; i < 64 * 8; i += 256) dw0[i] = img[(i >> 3) * 16 + c0 + (i & 7)];
}

struct Net {                   // one DualStreamUNet taking part in a forward pass
    const pc_step_net* n;
    bool save;                 // keep the activations for the backward pass
    bool logit_only;           // write the two partial fusion_out_conv logits instead of the feature map
};

struct Key { int e, s, c; };          // network, stream, position of the stream among the present ones

// Forward of `nE` networks on the same padded input Xp (B, the present streams' channels in stream order, Hp, Wp), one grouped launch per layer for all
// (network, stream) pairs -- engine.py: forward_multi.  feats[e]: (B, 16, Hp, Wp) or, for logit_only networks, (B, 2, Hp, Wp).
void forward_nets(Step& X, const Net* nets, int nE, const Ten& Xp, int Hp, int Wp, Ten* feats, Saved (*saved)[2]) {
    const int B = Xp.B;
    const int H1 = Hp / 2, W1 = Wp / 2, H2 = H1 / 2, W2 = W1 / 2;
    Arena& A = X.ar;
    Key keys[MAXK];
    int K = 0;
    for (int e = 0; e < nE; ++e)
        for (int c = 0; c < X.ns; ++c) keys[K++] = Key{e, X.ps[c], c};
    auto lay = [&](const Key& k) -> const pc_step_stream& { return nets[k.e].n->s[k.s]; };
    bool any_save = false;
    for (int e = 0; e < nE; ++e) any_save = any_save || nets[e].save;

    Ten a1[MAXK], a2[MAXK], pa2[MAXK], b1[MAXK], b2[MAXK], pb2[MAXK], c1[MAXK], c2[MAXK], u2[MAXK], e1[MAXK], e2[MAXK], u1[MAXK], f1[MAXK];
    void* ws1[MAXK] = {nullptr, nullptr, nullptr, nullptr};
    void* ws2[MAXK] = {nullptr, nullptr, nullptr, nullptr};

    // generic grouped conv launch over all keys
    auto conv = [&](int L, const Ten* in, const Ten* in_b, Ten* out, int Cout, int H, int W, int mode, Ten* pooled) {
        pc_src sa[MAXK], sb[MAXK];
        pc_dst dout[MAXK], dpool[MAXK];
        pc_conv_fwd_desc d[MAXK];
        bool pool_ok = pooled != nullptr;
        for (int i = 0; i < K; ++i) {
            out[i] = A.act(B, Cout, H, W);
            dout[i] = D(out[i]);
            if (pooled && !pc_conv3x3_pool_out_ok(&dout[i], H, W)) pool_ok = false;
        }
        int Cin = 0;
        for (int i = 0; i < K; ++i) {
            memset(&d[i], 0, sizeof(d[i]));
            Ten src = in[i];
            if (mode == PC_SRC_POOL2) src = crop(src, 2 * H, 2 * W);
            sa[i] = S(src, mode);
            d[i].a = &sa[i];
            Cin = src.C;
            if (in_b) {
                sb[i] = S(in_b[i]);
                d[i].b = &sb[i];
                Cin += in_b[i].C;
            }
            d[i].w = lay(keys[i]).w[L];
            d[i].bn = &lay(keys[i]).bn[L];
            d[i].out = &dout[i];
            if (pool_ok) {
                pooled[i] = A.act(B, Cout, H / 2, W / 2);
                dpool[i] = D(pooled[i]);
                d[i].pool_out = &dpool[i];
            }
        }
        if (pooled && !pool_ok)
            for (int i = 0; i < K; ++i) pooled[i] = Ten{};
        if (X.go()) X.rc(pc_conv3x3_bn_relu_fwd_group(K, d, 1, B, H, W, Cin, Cout, X.st));
    };

    // first layer: Cin differs per stream -> one launch per stream over the networks (aligned DIRECT loader on the padded input)
    {
        int c0 = 0;
        for (int c = 0; c < X.ns; ++c) {
            const int s = X.ps[c];
            const int cin = nets[0].n->s[s].cin;
            pc_src sa[MAXK];
            pc_dst dout[MAXK];
            pc_conv_fwd_desc d[MAXK];
            const Ten xin = chans(Xp, c0, cin);
            int n = 0;
            for (int i = 0; i < K; ++i) {
                if (keys[i].s != s) continue;
                a1[i] = A.act(B, 8, Hp, Wp);
                sa[n] = S(xin);
                dout[n] = D(a1[i]);
                memset(&d[n], 0, sizeof(d[n]));
                d[n].a = &sa[n]; d[n].w = lay(keys[i]).w[L_INC1]; d[n].bn = &lay(keys[i]).bn[L_INC1]; d[n].out = &dout[n];
                ++n;
            }
            if (X.go()) X.rc(pc_conv3x3_bn_relu_fwd_group(n, d, 1, B, Hp, Wp, cin, 8, X.st));
            c0 += cin;
        }
    }
    conv(L_INC2, a1, nullptr, a2, 8, Hp, Wp, PC_SRC_DIRECT, pa2);
    if (pa2[0].ok()) conv(L_D1A, pa2, nullptr, b1, 16, H1, W1, PC_SRC_DIRECT, nullptr);
    else conv(L_D1A, a2, nullptr, b1, 16, H1, W1, PC_SRC_POOL2, nullptr);
    conv(L_D1B, b1, nullptr, b2, 16, H1, W1, PC_SRC_DIRECT, pb2);

    // composed Up blocks (conv3x3 o convT from the low-resolution map, no up-sampled tensor): exact 2x geometry; with a backward pass
    // only where pc_conv3x3_up_bwd_ok takes the level
    auto fake = [&](int C, int h, int w) {          // a tensor of the arena's layout at an aligned address (for the *_ok predicates)
        Ten t;
        t.p = reinterpret_cast<float*>(A.base); t.B = B; t.C = C; t.H = h; t.W = w;
        // (dense_rule: the question is asked of dense rows, as the per-launch engine asks it of its tensors outside padded_rows() --
        // composed and plain Up blocks round differently, so the executor must take the form that engine takes)
        t.sr = X.dense_rule ? w : (w + 3) & ~3; t.sc = (int64_t)h * t.sr; t.sb = C * t.sc;
        return t;
    };
    auto can_compose = [&](int h, int w, int hz, int wz, int Cz) {
        if (h != 2 * hz || w != 2 * wz || (h & 3)) return false;
        const Ten sk = fake(Cz, h, w), z = fake(Cz, hz, wz), g = fake(8, h, w);
        const pc_src ss = S(sk), sz = S(z), sg = S(g);
        const pc_dst dz = D(z), dg = D(g);
        if (!pc_conv3x3_up_fwd_ok(&ss, &sz, &dg, h, w, Cz, Cz)) return false;
        return !any_save || pc_conv3x3_up_bwd_ok(&sg, &sz, &dz, h, w, Cz, Cz) != 0;
    };
    const bool compose2 = can_compose(H1, W1, H2, W2, 16);
    const bool compose1 = can_compose(Hp, Wp, H1, W1, 8);
    // backward() has the composed form only.  Cannot fail today: a saving network runs on the add_padding domain (sides % 32 == 0, fp32).
    if (any_save && !(compose1 && compose2)) return X.rc(PC_ENOTSUP);
    if (compose1 || compose2) {
        // the composed operand images of the levels in use, all (network, stream) pairs: one launch (they depend on the weights only)
        pc_conv_up_fwd_desc d[2 * MAXK];
        int cs[2 * MAXK], cz[2 * MAXK];
        int n = 0;
        if (compose2)
            for (int i = 0; i < K; ++i) {
                ws2[i] = A.raw(pc_conv3x3_up_ws_bytes(16));
                memset(&d[n], 0, sizeof(d[n]));
                d[n].w = lay(keys[i]).w[L_UP2A]; d[n].wt = lay(keys[i]).wt[T_UP2]; d[n].bt = lay(keys[i]).bt[T_UP2]; d[n].ws = ws2[i];
                cs[n] = 16; cz[n] = 16; ++n;
            }
        if (compose1)
            for (int i = 0; i < K; ++i) {
                ws1[i] = A.raw(pc_conv3x3_up_ws_bytes(8));
                memset(&d[n], 0, sizeof(d[n]));
                d[n].w = lay(keys[i]).w[L_UP1A]; d[n].wt = lay(keys[i]).wt[T_UP1]; d[n].bt = lay(keys[i]).bt[T_UP1]; d[n].ws = ws1[i];
                cs[n] = 8; cz[n] = 8; ++n;
            }
        if (X.go()) X.rc(pc_conv3x3_up_compose_group(n, d, cs, cz, X.st));
    }

    // the 32 x 32 level in one launch (down2's DoubleConv + up2's transposed conv with the maps in LDS)
    // (a saved pooled map has W1 % 32 == 0 and H1 % 4 == 0, so this is H1 = W1 = 64 exactly: a geometry every composed predicate takes,
    // extractor included -- the launch writes c2 for the composed conv and never the up-sampled map)
    bool level2 = false;
    if (compose2 && pb2[0].ok() && H2 == 32 && W2 == 32) {
        pc_src sx[MAXK];
        pc_dst d1[MAXK], d2[MAXK];
        pc_level2_fwd_desc d[MAXK];
        level2 = true;
        const int64_t mark = A.off;
        for (int i = 0; i < K; ++i) {
            c1[i] = nets[keys[i].e].save ? A.act(B, 16, 32, 32) : Ten{};
            c2[i] = A.act(B, 16, 32, 32);
            sx[i] = S(pb2[i]);
            memset(&d[i], 0, sizeof(d[i]));
            d[i].x = &sx[i];
            d[i].w1 = lay(keys[i]).w[L_D2A]; d[i].bn1 = &lay(keys[i]).bn[L_D2A];
            d[i].w2 = lay(keys[i]).w[L_D2B]; d[i].bn2 = &lay(keys[i]).bn[L_D2B];
            d[i].wt = lay(keys[i]).wt[T_UP2]; d[i].bt = lay(keys[i]).bt[T_UP2];
            if (c1[i].ok()) { d1[i] = D(c1[i]); d[i].c1 = &d1[i]; }
            d2[i] = D(c2[i]); d[i].c2 = &d2[i];
            if (!pc_level2_fwd_ok(&sx[i], nullptr)) level2 = false;
        }
        if (level2) {
            if (X.go()) X.rc(pc_level2_fwd_group(K, d, B, X.st));
        } else {
            A.off = mark;
            for (int i = 0; i < K; ++i) c1[i] = c2[i] = Ten{};
        }
    }
    if (!level2) {
        if (pb2[0].ok()) conv(L_D2A, pb2, nullptr, c1, 16, H2, W2, PC_SRC_DIRECT, nullptr);
        else conv(L_D2A, b2, nullptr, c1, 16, H2, W2, PC_SRC_POOL2, nullptr);
        conv(L_D2B, c1, nullptr, c2, 16, H2, W2, PC_SRC_DIRECT, nullptr);
    }

    auto convt = [&](int T, const Ten* in, Ten* out, int C, int h, int w, int Hs, int Ws) {
        // ConvTranspose2d(C, C, 2, 2): (h, w) -> (2h, 2w), written into the top-left corner of a tensor with the extent and strides of
        // the skip map (Hs, Ws) it is concatenated with; rows / columns beyond 2h / 2w are the zero padding of Up (networks.py:309-312)
        pc_src sx[MAXK];
        pc_dst dout[MAXK];
        pc_convt_fwd_desc d[MAXK];
        for (int i = 0; i < K; ++i) {
            const Ten full = A.act(B, C, Hs, Ws);
            out[i] = crop(full, 2 * h, 2 * w);
            sx[i] = S(in[i]);
            dout[i] = D(out[i]);
            d[i] = pc_convt_fwd_desc{&sx[i], lay(keys[i]).wt[T], lay(keys[i]).bt[T], &dout[i]};
        }
        if (X.go()) X.rc(pc_convt2x2_fwd_group(K, d, B, h, w, C, X.st));
    };
    auto up_conv = [&](int L, int T, const Ten* skip, const Ten* z, Ten* out, void** ws, int h, int w) {
        pc_src ss[MAXK], sz[MAXK];
        pc_dst dout[MAXK];
        pc_conv_up_fwd_desc d[MAXK];
        for (int i = 0; i < K; ++i) {
            out[i] = A.act(B, 8, h, w);
            ss[i] = S(skip[i]); sz[i] = S(z[i]); dout[i] = D(out[i]);
            d[i] = pc_conv_up_fwd_desc{&ss[i], &sz[i], lay(keys[i]).w[L], lay(keys[i]).wt[T], lay(keys[i]).bt[T], &lay(keys[i]).bn[L], &dout[i], ws[i]};
        }
        if (X.go()) X.rc(pc_conv3x3_up_fwd_group(K, d, 1 | PC_UP_PRECOMPOSED, B, h, w, skip[0].C, z[0].C, X.st));
    };

    if (compose2) {
        up_conv(L_UP2A, T_UP2, b2, c2, e1, ws2, H1, W1);
    } else {
        convt(T_UP2, c2, u2, 16, H2, W2, H1, W1);
        conv(L_UP2A, b2, u2, e1, 8, H1, W1, PC_SRC_DIRECT, nullptr);
    }
    conv(L_UP2B, e1, nullptr, e2, 8, H1, W1, PC_SRC_DIRECT, nullptr);
    if (compose1) {
        up_conv(L_UP1A, T_UP1, a2, e2, f1, ws1, Hp, Wp);
    } else {
        convt(T_UP1, e2, u1, 8, H1, W1, Hp, Wp);
        conv(L_UP1A, a2, u1, f1, 8, Hp, Wp, PC_SRC_DIRECT, nullptr);
    }
    // last layer: the two streams write their halves of the feature map, or (logit_only) their partial fusion_out_conv logit
    {
        for (int e = 0; e < nE; ++e) feats[e] = nets[e].logit_only ? A.act(B, 2, Hp, Wp) : A.act(B, 16, Hp, Wp, /*dense=*/true);
        pc_src sa[MAXK];
        pc_dst dout[MAXK];
        pc_conv_fwd_desc d[MAXK];
        for (int i = 0; i < K; ++i) {
            const Net& nt = nets[keys[i].e];
            const int f0 = lay(keys[i]).feat_c0;
            sa[i] = S(f1[i]);
            memset(&d[i], 0, sizeof(d[i]));
            d[i].a = &sa[i]; d[i].w = lay(keys[i]).w[L_UP1B]; d[i].bn = &lay(keys[i]).bn[L_UP1B];
            if (nt.logit_only) {
                dout[i] = D(chans(feats[keys[i].e], f0 / 8, 1));
                d[i].dot_w = nt.n->fusion_w + f0;
                d[i].dot_out = &dout[i];
            } else {
                dout[i] = D(chans(feats[keys[i].e], f0, 8));
                d[i].out = &dout[i];
            }
        }
        if (X.go()) X.rc(pc_conv3x3_bn_relu_fwd_group(K, d, 1, B, Hp, Wp, 8, 8, X.st));
        // one stream: the head reads all 16 channels of the trainable network's map -- the absent stream's 8 are zero (engine.py:
        // forward_multi allocates that map zeroed).  The extractor's map is read through its live half only (forward: score_mask)
        for (int e = 0; e < nE && X.one(); ++e) {
            if (nets[e].n != &X.plan.unet) continue;
            const Ten dead = chans(feats[e], 8 - nets[e].n->s[X.ps[0]].feat_c0, 8);
            if (X.go()) {
                const int64_t per_b = 8 * dead.sc, blocks = (per_b * B + 255) / 256;
                hipLaunchKernelGGL(zero_chans_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, X.st, dead.p, dead.sb, per_b, B);
                X.rc((int)hipGetLastError());
            }
        }
    }
    for (int i = 0; i < K; ++i) {
        if (!saved || !nets[keys[i].e].save) continue;
        Saved& sv = saved[keys[i].e][keys[i].c];
        sv.a1 = a1[i]; sv.a2 = a2[i]; sv.b1 = b1[i]; sv.b2 = b2[i]; sv.c1 = c1[i]; sv.c2 = c2[i]; sv.e1 = e1[i];
        sv.e2 = e2[i]; sv.f1 = f1[i]; sv.pa2 = pa2[i]; sv.pb2 = pb2[i]; sv.ws_up1 = ws1[i]; sv.ws_up2 = ws2[i];
    }
}

// channels of a PC_DATA_INPUT tensor: 6, or for a one-stream plan the stream's own (2 / 4: the model's input_channels) unless io.craw
// names another count (a 6-channel tile fed to a one-stream model: the stream's chan[] picks from it, as the per-launch step does)
inline int input_channels(const Step& X, const pc_step_io& io) {
    if (!X.one()) return 6;
    return io.craw > 0 ? io.craw : X.cs[0].cin;
}

// the padded, normalised, stream-ordered input of a domain: (B, 6 -- one stream: 2 / 4 --, H + top + bottom, W + left + right), rows padded to 16 bytes
Ten ingest(Step& X, const pc_step_io& io, int top, int bottom, int left, int right) {
    const pc_step_plan& P = X.plan;
    const Ten out = X.ar.act(io.B, P.unet.s[0].cin + P.unet.s[1].cin, io.H + top + bottom, io.W + left + right);
    int sel[8];
    float mean[8], stdv[8];
    int n = 0;
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < P.unet.s[s].cin; ++c) {
            const int ch = P.unet.s[s].chan[c];                    // model channel ([R,G,B,NIR,VV,VH])
            sel[n] = io.data_kind == PC_DATA_RAW ? P.band[ch] : ch;
            mean[n] = P.mean[ch]; stdv[n] = P.stdv[ch];
            ++n;
        }
    const bool norm = io.data_kind != PC_DATA_INPUT;
    const int Cin = io.data_kind == PC_DATA_RAW ? io.craw : (io.data_kind == PC_DATA_SPLIT ? 4 : input_channels(X, io));
    if (X.go())
        X.rc(pc_ingest_pad_strided(io.data_kind, io.data, io.data2, Cin, out.p, out.sr, io.B, n, sel, norm ? mean : nullptr, norm ? stdv : nullptr,
                                   io.H, io.W, top, bottom, left, right, X.st));
    return out;
}

// One forward pass in the arena.  X.infer (pc_forward): model(sample, padding=False) in eval mode under no_grad with the dense head --
// the same ingest, networks and head launches without the sparsity mask, its counts and selection flags, the loss's popcount gradient
// and the statistics; nothing is saved (io.unet_no_grad is set by the caller) and nothing of it outlives the call.
void forward(Step& X, pc_step_io& io) {
    const pc_step_plan& P = X.plan;
    Arena& A = X.ar;
    const int B = io.B, H = io.H, W = io.W;
    int pt, pb, pl, pr;
    pad_geometry(H, W, pt, pb, pl, pr);
    const int Hp = H + pt + pb, Wp = W + pl + pr;
    const int p = P.extractor_pad;
    X.B = B; X.H = H; X.W = W; X.pt = pt; X.pl = pl; X.Hp = Hp; X.Wp = Wp;
    X.unet_ng = io.unet_no_grad != 0;
    X.enc_ng = io.encoder_no_grad != 0 || X.unet_ng;
    // outputs first (fixed offsets whatever follows)
    X.popcount = reinterpret_cast<float*>(A.raw((int64_t)B * 4));
    io.off_popcount = reinterpret_cast<char*>(X.popcount) - A.base;
    X.popdense = reinterpret_cast<float*>(A.raw((int64_t)B * H * W * 4));
    io.off_popdense = reinterpret_cast<char*>(X.popdense) - A.base;
    X.scale_map = reinterpret_cast<float*>(A.raw((int64_t)B * H * W * 4));
    io.off_scale = reinterpret_cast<char*>(X.scale_map) - A.base;
    const bool infer = X.infer, one = X.one();
    X.mask = infer ? nullptr : reinterpret_cast<uint8_t*>(A.raw((int64_t)B * H * W));
    io.off_mask = infer ? -1 : reinterpret_cast<char*>(X.mask) - A.base;
    const bool given = X.layer != nullptr;
    X.fwd_layer = X.layer;
    if (given) {
        // the caller's tensor IS the output: no plane, no offset
        X.building = Ten{};
        io.off_building = -1;
    } else {
        X.building = A.act(B, 1, H, W, /*dense=*/true);
        io.off_building = reinterpret_cast<char*>(X.building.p) - A.base;
    }
    X.counts = infer ? nullptr : reinterpret_cast<int32_t*>(A.raw(16));
    X.sel = io.sel;
    uint8_t* sel_dev = io.sel_host && !infer ? reinterpret_cast<uint8_t*>(A.raw(H + W)) : nullptr;
    auto unpack_sel = [&]() {          // (on the stream whose chain ends in the mask kernel)
        if (!sel_dev) return;
        X.sel = sel_dev;
        if (!X.go()) return;
        SelBits bits;
        memset(&bits, 0, sizeof(bits));
        for (int i = 0; i < H + W; ++i)
            if (io.sel_host[i]) bits.w[i >> 5] |= 1u << (i & 31);
        hipLaunchKernelGGL(sel_unpack_kernel, dim3(1), dim3(256), 0, X.st, bits, sel_dev, H + W);
        X.rc((int)hipGetLastError());
    };
    X.g_pc = infer ? nullptr : reinterpret_cast<float*>(A.raw((int64_t)B * 4));
    X.head_ws = A.raw(pc_head_ws_bytes(B, H, W));
    for (int t = 0; t < 8; ++t) { X.hw[t] = P.head_w[t]; X.hdw[t] = P.head_dw[t]; }
    if (one) {
        // the head kernels take a 64 x 16 first layer: the parameter embedded in a zeroed image, and an image for its gradient
        X.w0_img = reinterpret_cast<float*>(A.raw(64 * 16 * 4));
        X.dw0_img = reinterpret_cast<float*>(A.raw(64 * 16 * 4));
        X.hw[0] = X.w0_img;
        X.hdw[0] = X.dw0_img;
    }
    X.fwd_units = X.un != nullptr;
    if (X.un) {
        // multi-unit batch: the flattened lists, the slot map and the N popcounts (sorted order for the loss, caller's order as the result)
        Step::Units& U = X.U;
        const int64_t N = U.N = X.un->N;
        U.pc_caller = reinterpret_cast<float*>(A.raw(N * 4));
        X.un->off_popcount = reinterpret_cast<char*>(U.pc_caller) - A.base;
        U.slot = reinterpret_cast<int32_t*>(A.raw((int64_t)B * H * W * 4));
        X.un->off_slot = reinterpret_cast<char*>(U.slot) - A.base;
        U.units = reinterpret_cast<int64_t*>(A.raw(N * 8));
        U.unit_off = reinterpret_cast<int32_t*>(A.raw((int64_t)(B + 1) * 4));
        U.y_sorted = reinterpret_cast<float*>(A.raw(N * 4));
        U.dest = reinterpret_cast<int32_t*>(A.raw(N * 4));
        U.ws = A.raw(pc_unit_ws_bytes(N));
        U.pc_sorted = reinterpret_cast<float*>(A.raw(N * 4));
        U.g_pc = reinterpret_cast<float*>(A.raw(N * 4));
    }
    // the lists (and the zeroed workspace of the unit sums) are made once per step, in front of the chain that ends in the mask
    auto unit_layout = [&]() {
        if (!X.un || !X.go()) return;
        X.rc(pc_unit_layout(X.un->census_idx, X.un->y, X.un->census_n, B, X.un->K, X.U.units, X.U.unit_off, X.U.y_sorted, X.U.dest, X.U.ws,
                            X.st));
    };

    const bool same_domain = pt == p && pb == p && pl == p && pr == p;     // e.g. 100 x 100 tiles: both networks on the 128 x 128 domain
    Ten feats[2];
    Saved (*sv)[2] = nullptr;
    Saved svbuf[2][2];
    const float* am = io.admin_mask;
    // building score + mask + census counts from the extractor's partial logits, which start (oy, ox) inside its domain
    // (one stream -- engine.py: _logit_operands: the extractor's 16-channel map read through its live half with the stream's own out conv,
    // which is what the plan's fusion_w / fusion_b point at; no partial-logit epilogue there, as dot_ok has it)
    auto score_mask = [&](const Ten& logits, int oy, int ox) {
        const pc_src fs = one ? S(chans(logits, P.extractor.s[X.ps[0]].feat_c0, 8)) : S(logits);
        const float* lw = one ? P.extractor.fusion_w : X.ones2;
        const pc_dst db = D(X.building);
        if (infer) {
            // the score alone (engine.py: building_score / score_from_features): the dense head has no mask
            if (X.go()) X.rc(pc_outconv_sigmoid_crop(&fs, lw, P.extractor.fusion_b, &db, B, H, W, oy, ox, X.st));
            return;
        }
        if (X.un) {
            // multi-unit: the score as a map, then the unit lookup + union mask (train.py: score_from_features + ops.unit_mask)
            if (X.go()) X.rc(pc_outconv_sigmoid_crop(&fs, lw, P.extractor.fusion_b, &db, B, H, W, oy, ox, X.st));
            if (X.go())
                X.rc(pc_unit_mask(X.building.p, am, X.U.units, X.U.unit_off, X.sel, X.sel + H, P.occupancymodel, X.U.slot, X.mask, X.counts,
                                  nullptr, B, H, W, X.U.N, X.st));
            return;
        }
        if (X.go())
            X.rc(pc_building_score_mask(&fs, lw, P.extractor.fusion_b, &db, am, io.census_idx, X.sel, X.sel + H, P.occupancymodel, X.mask,
                                        X.counts, B, H, W, oy, ox, X.st));
    };
    if (given) {
        // a shipped building layer (train.py: _forward, `given`): no extractor on either domain -- the mask on the layer, then the
        // trainable U-Net alone (forward_multi([eng_u]))
        unpack_sel();
        unit_layout();
        if (infer) {
            // (the layer is only read: by the head)
        } else if (X.un) {
            if (X.go())
                X.rc(pc_unit_mask(X.layer, am, X.U.units, X.U.unit_off, X.sel, X.sel + H, P.occupancymodel, X.U.slot, X.mask, X.counts,
                                  nullptr, B, H, W, X.U.N, X.st));
        } else if (X.go()) {
            X.rc(pc_sparsity_mask(X.layer, am, io.census_idx, X.sel, X.sel + H, P.occupancymodel, X.mask, X.counts, B, H, W, X.st));
        }
        const Ten Xp = ingest(X, io, pt, pb, pl, pr);
        X.Xp_u = Xp;
        const Net nu[1] = {Net{&P.unet, !X.unet_ng, false}};
        sv = svbuf;
        forward_nets(X, nu, 1, Xp, Hp, Wp, feats, sv);
        X.feats = feats[0];
        X.sv[0] = svbuf[0][0]; X.sv[1] = svbuf[0][1];
    } else if (same_domain) {
        unpack_sel();
        unit_layout();
        const Ten Xp = ingest(X, io, pt, pb, pl, pr);
        X.Xp_u = Xp;
        const Net nets[2] = {Net{&P.extractor, false, !one}, Net{&P.unet, !X.unet_ng, false}};
        sv = svbuf;
        forward_nets(X, nets, 2, Xp, Hp, Wp, feats, sv);
        X.feats = feats[1];
        X.sv[0] = svbuf[1][0]; X.sv[1] = svbuf[1][1];
        score_mask(feats[0], pt, pl);
    } else {
        // the frozen extractor on its own 14-pixel reflect-padded domain (popcorn.py:279-322)
        const bool two = X.side != nullptr && (int64_t)B * Hp * Wp <= X.side_px;
        hipStream_t main_st = X.st;
        const int64_t mark = A.off;
        if (two && X.go()) {
            // fork: the side chain starts behind everything already enqueued on the caller's stream (the batch's copies, the previous step)
            X.rc((int)hipEventRecord(X.ev_fork, main_st));
            X.rc((int)hipStreamWaitEvent(X.side, X.ev_fork, 0));
        }
        if (two) X.st = X.side;
        {
            unpack_sel();
            unit_layout();
            const Ten Xb = ingest(X, io, p, p, p, p);
            const Net nb[1] = {Net{&P.extractor, false, !one}};
            forward_nets(X, nb, 1, Xb, H + 2 * p, W + 2 * p, feats, nullptr);
            score_mask(feats[0], p, p);
        }
        if (two) {
            if (X.go()) X.rc((int)hipEventRecord(X.ev_join, X.side));
            X.st = main_st;
        } else {
            A.off = mark;      // its activations are released (stream order: everything that follows is enqueued behind the extractor's launches)
        }
        const Ten Xp = ingest(X, io, pt, pb, pl, pr);
        X.Xp_u = Xp;
        const Net nu[1] = {Net{&P.unet, !X.unet_ng, false}};
        sv = svbuf;
        forward_nets(X, nu, 1, Xp, Hp, Wp, feats, sv);
        X.feats = feats[0];
        X.sv[0] = svbuf[0][0]; X.sv[1] = svbuf[0][1];
        if (two && X.go()) X.rc((int)hipStreamWaitEvent(main_st, X.ev_join, 0));      // join: the head needs the building score and the mask
    }
    // sparse head + occupancy product + census sums (popcorn.py:161-190,195-228)
    X.bld = given ? X.layer : X.building.p;
    if (!P.occupancymodel) {
        // popcorn.py:179-181: popdensemap = relu(out), no building product -- the head multiplies by a plane of ones
        // (train.py: _forward, torch.ones_like(building)); the score / the layer stays the step's building output
        const int64_t n = (int64_t)B * H * W;
        float* ones = reinterpret_cast<float*>(A.raw(n * 4));
        X.bld = ones;
        if (X.go()) {
            const int64_t blocks = (n + 255) / 256;
            hipLaunchKernelGGL(ones_fill_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, X.st, ones, n);
            X.rc((int)hipGetLastError());
        }
    }
    if (one && X.go()) {
        hipLaunchKernelGGL(head_w0_embed_kernel, dim3(1), dim3(256), 0, X.st, P.head_w[0], X.w0_img, X.cs[0].feat_c0);
        X.rc((int)hipGetLastError());
    }
    const float* bld = X.bld;
    const pc_src sf = S(X.feats);
    if (infer) {
        // dense head (mask == NULL), popcount over the region or the plain sum (admin_mask == NULL), no statistics
        if (X.go())
            X.rc(pc_head_fwd(&sf, pt, pl, X.hw, nullptr, bld, am, io.census_idx, X.scale_map, X.popdense, X.popcount, nullptr, nullptr,
                             X.head_ws, B, H, W, 0, X.st));
        X.launches += 2;           // (X.rc counted one; flags = 0 is three launches: head_pack_kernel + the head kernel + head_popcount_reduce_kernel)
        return;
    }
    if (X.un) {
        // the union mask, no region: popdensemap is written at every pixel (0 * building outside the mask -- what the unit sums of
        // backward() rely on), {Nsel, sum scale} finished by the call, popcount[B] = the plain sums (unused)
        X.deferred_popcount = false;
        if (X.go())
            X.rc(pc_head_fwd(&sf, pt, pl, X.hw, X.mask, bld, nullptr, nullptr, X.scale_map, X.popdense, X.popcount, P.stats_dev, X.counts,
                             X.head_ws, B, H, W, PC_HEAD_FWD_PACK_BOTH, X.st));
        X.launches += 2;           // (pack + kernel + reduction)
        X.fwd_end = A.off;
        X.have_fwd = true;
        return;
    }
    X.deferred_popcount = io.dp == 0;
    if (X.go())
        X.rc(pc_head_fwd(&sf, pt, pl, X.hw, X.mask, bld, am, io.census_idx, X.scale_map, X.popdense, X.popcount, P.stats_dev, X.counts,
                         X.head_ws, B, H, W, PC_HEAD_FWD_PACK_BOTH | (X.deferred_popcount ? PC_HEAD_FWD_DEFER_REDUCE : 0), X.st));
    X.launches += 1;           // (pack + kernel)
    X.fwd_end = A.off;
    X.have_fwd = true;
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
struct Reduce {                // the batched second stage of all weight gradients of a backward pass (ops.py: WgradBatch)
    pc_wgrad_reduce_desc e[40];
    int n = 0;
    float* head_ptrs[8];
    // composed Up blocks: chain-rule launches behind the reduction
    pc_conv_up_bwd_desc ch8[2], ch16[2];
    pc_src ch_g[2][2], ch_z[2][2];
    pc_dst ch_gz[2][2];
    int n8 = 0, n16 = 0, nwg8 = 0, nwg16 = 0;

    // one entry (popcorn_hip.h: pc_wgrad_reduce_desc).  kind 0: a conv's partials -> dw (rows co_stride apart, 0 = dense) and db;
    // 2: a composed level's -> their total of Cin floats at dw; 3: the head's -> its 8 tensors (dw: the table of their pointers)
    void add(const void* partial, float* dw, float* db, int nwg, int Cin, int Cout, int kind, int co_stride = 0) {
        pc_wgrad_reduce_desc& d = e[n++];
        memset(&d, 0, sizeof(d));
        d.partial = reinterpret_cast<const float*>(partial);
        d.dw = dw; d.db = db; d.nwg = nwg; d.Cin = Cin; d.Cout = Cout; d.kind = kind; d.accumulate = 0; d.dw_co_stride = co_stride;
    }
};

struct T2 {                    // one tensor per stream
    Ten t[2];
    Ten& operator[](int s) { return t[s]; }
    const Ten& operator[](int s) const { return t[s]; }
};

// The blocks of the network as the backward pass walks them (engine.py: _Up / _Down): layer indices and saved activations.
// Up: first conv (over cat[skip | up-sampled z]) and transposed conv; c = channels of the skip tensor = of z
struct UpLv { int conv, convt; Ten Saved::*skip; int skip_act; Ten Saved::*z; int z_act; void* Saved::*ws; int c; };
constexpr UpLv UP1 = {L_UP1A, T_UP1, &Saved::a2, L_INC2, &Saved::e2, L_UP2B, &Saved::ws_up1, 8};
constexpr UpLv UP2 = {L_UP2A, T_UP2, &Saved::b2, L_D1B, &Saved::c2, L_D2B, &Saved::ws_up2, 16};
// Down: the DoubleConv behind a MaxPool2d(2); cin = channels of the pooled map (`pooled`: its saved copy, `full`: what it was pooled from)
struct DownLv { int conv1, conv2; Ten Saved::*mid; Ten Saved::*pooled; Ten Saved::*full; int full_act, cin; };
constexpr DownLv DOWN1 = {L_D1A, L_D1B, &Saved::b1, &Saved::pa2, &Saved::a2, L_INC2, 8};
constexpr DownLv DOWN2 = {L_D2A, L_D2B, &Saved::c1, &Saved::pb2, &Saved::b2, L_D1B, 16};

// One backward pass of the trainable U-Net: its context, the launch helpers (bwd8 ... up_bwd: one grouped entry point each, both streams)
// and one function per block of the network (conv8, up, level2, down, first_layer), each of which decides its launch form where it
// stands -- engine.py: _Backward issues the same launches in the same order.
struct Backward {
    Step& X;
    const pc_step_stream* ST;
    const Saved* sv;
    const int B;
    const int NS;               // present streams: every per-stream loop and grouped launch below runs over them
    const bool enc_ng;
    Reduce R;
    // The weight-gradient-only launches (16-channel encoder layers, first layers) run on the side stream next to the data-gradient chain:
    // they only feed the batched reduction at the end.
    const hipStream_t main_st;
    const bool two;
    bool side_used = false;
    bool deferred = false;      // up(UP1)'s skip launch waits for down(DOWN1) (pool_add_plan)
    T2 deferred_g;              // ... its gradient operand
    bool deferred2 = false;     // up(UP2)'s skip-halves launch waits for level2() (pool_add_plan2)
    T2 deferred_g2;
    const int64_t slot_bytes = pc_conv3x3_wgrad_ws_bytes(32, 8);      // partials of one weight-gradient problem

    explicit Backward(Step& x)
        : X(x), ST(x.cs), sv(x.sv), B(x.B), NS(x.ns), enc_ng(x.enc_ng), main_st(x.st),
          two(x.side != nullptr && (int64_t)x.B * x.Hp * x.Wp <= x.side_bwd_px) {}

    void* slot(int64_t bytes = 0) { return X.ar.raw(bytes > slot_bytes ? bytes : slot_bytes); }
    T2 fresh(int C, int h, int w) {
        T2 t;
        for (int s = 0; s < NS; ++s) t[s] = X.ar.act(B, C, h, w);
        return t;
    }
    T2 saved(Ten Saved::*m) const { return T2{{sv[0].*m, sv[1].*m}}; }
    // side_on(): everything enqueued on the caller's stream so far (the producers of the launch's operands) is ordered in front of the
    // side stream's next launch
    void side_on() {
        if (!two) return;
        if (X.go()) {
            hipEvent_t ev = X.ev_dep[X.ev_next];
            X.ev_next = (X.ev_next + 1) & 7;
            X.rc((int)hipEventRecord(ev, main_st));
            X.rc((int)hipStreamWaitEvent(X.side, ev, 0));
        }
        X.st = X.side;
        side_used = true;
    }
    void side_off() { X.st = main_st; }

    // ---- launch helpers
    // data + weight gradient of an 8 -> 8 layer (or of an 8-channel column block of a wider one) in ONE launch, both streams
    // (x_bn nullptr: the raw data gradient; pool_grad: the pool-add form -- out also receives the max-pool scatter of that gradient)
    struct Blk {
        const Ten* g; const Ten* x; const pc_bn* x_bn; Ten* out; int L; int s; int c0_add; bool with_db; const Ten* pool_act = nullptr;
        const Ten* pool_grad = nullptr;
    };
    void bwd8(const Blk* blk, int n, int cin_total, int h, int w) {
        pc_src sg[MAXK], sx[MAXK], spa[MAXK], spg[MAXK];
        pc_dst dout[MAXK];
        pc_conv_bwd_desc d[MAXK];
        void* ws[MAXK];
        for (int i = 0; i < n; ++i) {
            sg[i] = S(*blk[i].g); sx[i] = S(*blk[i].x); dout[i] = D(*blk[i].out);
            ws[i] = slot();
            memset(&d[i], 0, sizeof(d[i]));
            d[i].g = &sg[i]; d[i].x = &sx[i]; d[i].w = ST[blk[i].s].w[blk[i].L]; d[i].x_bn = blk[i].x_bn; d[i].out = &dout[i]; d[i].ws = ws[i];
            d[i].c0_add = blk[i].c0_add;
            if (blk[i].pool_act) { spa[i] = S(*blk[i].pool_act); d[i].pool_act = &spa[i]; }     // Down block: scatter (+=) into the full-resolution gradient
            if (blk[i].pool_grad) { spg[i] = S(*blk[i].pool_grad); d[i].pool_grad = &spg[i]; }
        }
        int nwg = 0;
        if (X.go()) X.rc(pc_conv3x3_bwd_group(n, d, cin_total, 0, blk[0].pool_act ? 1 : 0, B, h, w, &nwg, X.st));
        for (int i = 0; i < n; ++i)
            R.add(ws[i], ST[blk[i].s].dw[blk[i].L] + blk[i].c0_add * 9, blk[i].with_db ? ST[blk[i].s].db[blk[i].L] : nullptr, nwg, 8, blk[i].g->C, 0,
                  cin_total * 9);
    }
    // a layer with a 16-channel input as ONE launch of bwd8: the two 8-channel halves of x (masked by half_bn[s][i]) are two problems per
    // stream over the same gradient, each writing its half of the data gradient and its column block of the weight gradient
    // (pool_grad: the pool-add form, each half with its 8-channel slice of the pooled gradient)
    void bwd_halves(int L, const T2& g, const T2& x, const pc_bn (*half_bn)[2], T2& out, int cin_total, int h, int w, const T2* pool_grad = nullptr) {
        Blk b[4];
        Ten xh[2][2], oh[2][2], ph[2][2];
        for (int s = 0; s < NS; ++s)
            for (int i = 0; i < 2; ++i) {
                xh[s][i] = chans(x[s], 8 * i, 8);
                oh[s][i] = chans(out[s], 8 * i, 8);
                b[2 * s + i] = Blk{&g[s], &xh[s][i], &half_bn[s][i], &oh[s][i], L, s, 8 * i, i == 0};
                if (pool_grad) {
                    ph[s][i] = chans((*pool_grad)[s], 8 * i, 8);
                    b[2 * s + i].pool_grad = &ph[s][i];
                }
            }
        bwd8(b, 2 * NS, cin_total, h, w);
    }
    // does the fused launch take this (gradient, input block, output, pooled-from) combination?  (split-operand form, aligned fp32 tensors)
    bool bwd_ok(const Ten& g, const Ten& x, const Ten& out, const Ten* pool_act, int h, int w) const {
        const pc_src sg = S(g), sx = S(x);
        const pc_dst dout = D(out);
        pc_src spa;
        if (pool_act) spa = S(*pool_act);
        return pc_conv3x3_bwd_ok(&sg, &sx, &dout, pool_act ? &spa : nullptr, B, h, w) != 0;
    }
    // Level 1, encoder trained (engine.py: _Backward.pool_add_plan, the same predicates): may the Up block's skip launch wait for the Down
    // block that pooled the same map and add that block's max-pool scatter in its own epilogue?  Asked of tensors laid out as the pass
    // will allocate them (the arena gives every tensor the same alignment); nothing stays allocated.
    bool pool_add_plan(const T2& g, const T2& skip, const T2& g_skip, int h, int w) {
        if (enc_ng) return false;
        const int64_t mark = X.ar.off;
        const T2 g_out = fresh(16, h / 2, w / 2), g_mid = fresh(16, h / 2, w / 2), g_pooled = fresh(DOWN1.cin, h / 2, w / 2);
        const T2 mid = saved(DOWN1.mid), pooled = saved(DOWN1.pooled), full = saved(DOWN1.full);
        bool ok = true;
        for (int s = 0; s < NS && ok; ++s) {
            const pc_src sg = S(g[s]), sx = S(skip[s]), spg = S(g_pooled[s]);
            const pc_dst dout = D(g_skip[s]);
            ok = pooled[s].ok() && bwd_ok(g_mid[s], pooled[s], g_skip[s], &full[s], h / 2, w / 2) &&
                 bwd_ok(g_out[s], chans(mid[s], 8, 8), chans(g_mid[s], 8, 8), nullptr, h / 2, w / 2) &&
                 bwd_ok(g_mid[s], pooled[s], g_pooled[s], nullptr, h / 2, w / 2) &&
                 pc_conv3x3_bwd_pool_add_ok(&sg, &sx, &dout, &spg, B, h, w) != 0;
        }
        X.ar.off = mark;
        return ok;
    }
    // ... and one level down (engine.py: _Backward.pool_add_plan2): where the whole-level kernel will take the 32 x 32 level and the launcher
    // takes both skip halves with their slices of the pooled gradient
    bool pool_add_plan2(const T2& g, const T2& skip, const T2& g_skip, int h, int w) {
        if (enc_ng || !sv[0].pb2.ok() || h != 64 || w != 64) return false;
        const int64_t mark = X.ar.off;
        const T2 gz = fresh(16, 32, 32), g_pooled = fresh(16, 32, 32);
        bool ok = true;
        for (int s = 0; s < NS && ok; ++s) {
            const pc_src sg2 = S(gz[s]), sc = S(sv[s].c1), sx = S(sv[s].pb2), sa = S(sv[s].b2);
            const pc_dst dz = D(g_skip[s]);
            ok = pc_level2_bwd_ok(&sg2, &sc, &sx, &sa, &dz) != 0;
            for (int i = 0; i < 2 && ok; ++i) {
                const pc_src sg = S(g[s]), sxh = S(chans(skip[s], 8 * i, 8)), spg = S(chans(g_pooled[s], 8 * i, 8));
                const pc_dst dout = D(chans(g_skip[s], 8 * i, 8));
                ok = pc_conv3x3_bwd_ok(&sg, &sxh, &dout, nullptr, B, h, w) != 0 && pc_conv3x3_bwd_pool_add_ok(&sg, &sxh, &dout, &spg, B, h, w) != 0;
            }
        }
        X.ar.off = mark;
        return ok;
    }
    // grouped weight gradient of layer L over both streams (side stream); cin_total: the layer's input channels where a is a column block
    void wgrad(int L, const T2& a, int mode, const T2& g, int h, int w, int cin_total = 0) {
        side_on();
        pc_src sa[2], sg[2];
        pc_conv_wgrad_desc d[2];
        void* ws[2];
        int Cin = 0;
        for (int s = 0; s < NS; ++s) {
            Ten src = a[s];
            if (mode == PC_SRC_POOL2) src = crop(src, 2 * h, 2 * w);
            sa[s] = S(src, mode); sg[s] = S(g[s]);
            ws[s] = slot();
            d[s] = pc_conv_wgrad_desc{&sa[s], nullptr, &sg[s], ws[s]};
            Cin = src.C;
        }
        int nwg = 0;
        if (X.go()) X.rc(pc_conv3x3_wgrad_partial_group(NS, d, B, h, w, Cin, g[0].C, &nwg, X.st));
        for (int s = 0; s < NS; ++s) R.add(ws[s], ST[s].dw[L], ST[s].db[L], nwg, Cin, g[0].C, 0, cin_total * 9);
        side_off();
    }
    // data gradient of layer L w.r.t. all its cin input channels, masked by the producer actL of act; pool: scattered (+=) through the
    // MaxPool2d(2) that act went into
    void dgrad(int L, const T2& g, T2& out, int cin, const T2& act, int actL, bool pool, int h, int w) {
        pc_src sg[2], sa[2];
        pc_dst dout[2];
        pc_conv_dgrad_desc d[2];
        for (int s = 0; s < NS; ++s) {
            sg[s] = S(g[s]); sa[s] = S(act[s]); dout[s] = D(out[s]);
            d[s] = pc_conv_dgrad_desc{&sg[s], ST[s].w[L], &sa[s], &X.bn_nobias[s][actL], &dout[s]};
        }
        if (X.go()) X.rc(pc_conv3x3_dgrad_group(NS, d, cin, 0, cin, pool ? 1 : 0, pool ? 1 : 0, B, h, w, g[0].C, X.st));
    }
    // composed Up block: dz, the composed weight gradient and the border sums from one pass over g (up_bwd.hip)
    void up_bwd(const UpLv& lv, const T2& g, const T2* gz, int h, int w) {
        pc_conv_up_bwd_desc* d = lv.c == 8 ? R.ch8 : R.ch16;
        const int k = lv.c == 8 ? 0 : 1;
        void* ws[2];
        for (int s = 0; s < NS; ++s) {
            R.ch_g[k][s] = S(g[s]); R.ch_z[k][s] = S(sv[s].*lv.z);
            if (gz) R.ch_gz[k][s] = D((*gz)[s]);
            ws[s] = slot(pc_conv3x3_up_bwd_ws_bytes(B, h, lv.c));
            memset(&d[s], 0, sizeof(d[s]));
            d[s].g = &R.ch_g[k][s]; d[s].z = &R.ch_z[k][s]; d[s].z_bn = &X.bn_nobias[s][lv.z_act]; d[s].gz = gz ? &R.ch_gz[k][s] : nullptr;
            d[s].w = ST[s].w[lv.conv]; d[s].wt = ST[s].wt[lv.convt]; d[s].bt = ST[s].bt[lv.convt]; d[s].fwd_ws = sv[s].*lv.ws; d[s].ws = ws[s];
            d[s].dw = ST[s].dw[lv.conv]; d[s].dwt = ST[s].dwt[lv.convt]; d[s].dbt = ST[s].dbt[lv.convt];
        }
        int nwg = 0, part = 0;
        if (X.go()) X.rc(pc_conv3x3_up_bwd_partial_group(NS, d, B, h, w, lv.c, lv.c, &nwg, &part, X.st));
        else { nwg = 1; part = 1; }
        for (int s = 0; s < NS; ++s) R.add(ws[s], reinterpret_cast<float*>(ws[s]) + (int64_t)nwg * part, nullptr, nwg, part, 0, 2);
        if (lv.c == 8) { R.n8 = NS; R.nwg8 = nwg; } else { R.n16 = NS; R.nwg16 = nwg; }
    }

    // ---- the blocks
    // an 8 -> 8 layer L (second conv of a DoubleConv at full or half resolution) over the saved x, made by layer actL: returns the
    // gradient of its input
    T2 conv8(int L, const T2& g, Ten Saved::*x, int actL, int h, int w) {
        T2 out = fresh(8, h, w);
        Blk b[2];
        for (int s = 0; s < NS; ++s) b[s] = Blk{&g[s], &(sv[s].*x), &X.bn_nobias[s][actL], &out[s], L, s, 0, true};
        bwd8(b, NS, 8, h, w);
        return out;
    }
    // An Up block from the gradient g of its first conv's output at (h, w): the skip column block of that conv (weight gradient into the
    // first c input columns, data gradient masked by the skip tensor's producer), then the composed pass for the up-sampled half and the
    // transposed conv.  g_skip: gradient of the skip tensor (level 2 under encoder_no_grad: none, nobody reads it); gz: gradient of z
    // (nullptr: not wanted)
    void up(const UpLv& lv, const T2& g, int h, int w, T2& g_skip, T2* gz) {
        const T2 skip = saved(lv.skip);
        if (lv.c == 8) {            // one problem per stream, whatever the regime
            g_skip = fresh(8, h, w);
            deferred = pool_add_plan(g, skip, g_skip, h, w);
            if (deferred) {         // down(DOWN1) issues the launch, behind its own first layer
                deferred_g = g;
            } else {
                Blk b[2];
                for (int s = 0; s < NS; ++s) b[s] = Blk{&g[s], &skip[s], &X.bn_nobias[s][lv.skip_act], &g_skip[s], lv.conv, s, 0, true};
                bwd8(b, NS, 16, h, w);
            }
        } else if (!enc_ng) {       // the two 8-channel halves of the 16-channel skip tensor
            g_skip = fresh(16, h, w);
            deferred2 = pool_add_plan2(g, skip, g_skip, h, w);
            if (deferred2) deferred_g2 = g;             // level2() issues the launch, behind its own
            else bwd_halves(lv.conv, g, skip, X.bn_half, g_skip, 32, h, w);
        } else {
            wgrad(lv.conv, skip, PC_SRC_DIRECT, g, h, w, 32);
        }
        if (gz) *gz = fresh(lv.c, h / 2, w / 2);
        up_bwd(lv, g, gz, h, w);
    }
    // the 32 x 32 level: both weight gradients, the data gradient chain d2b -> d2a and the pooling scatter in one launch.  false: the
    // geometry does not qualify, nothing was enqueued
    bool level2(const T2& g_out, T2& g_in, int h, int w) {
        if (!sv[0].pb2.ok() || h != 32 || w != 32) return false;
        pc_src sg[2], sc[2], sx[2], sa[2];
        pc_dst dout[2], dpg[2];
        T2 g_pooled;
        if (deferred2) g_pooled = fresh(16, h, w);
        pc_level2_bwd_desc d[2];
        void* w1[2];
        void* w2[2];
        const int64_t mark = X.ar.off;
        for (int s = 0; s < NS; ++s) {
            sg[s] = S(g_out[s]); sc[s] = S(sv[s].c1); sx[s] = S(sv[s].pb2); sa[s] = S(sv[s].b2); dout[s] = D(g_in[s]);
            w1[s] = slot(pc_level2_bwd_ws_bytes(B)); w2[s] = slot(pc_level2_bwd_ws_bytes(B));
            d[s] = pc_level2_bwd_desc{&sg[s], &sc[s], &sx[s], ST[s].w[L_D2A], ST[s].w[L_D2B], &X.bn_nobias[s][L_D2A], &sa[s],
                                      &X.bn_nobias[s][L_D1B], &dout[s], w1[s], w2[s]};
            if (!pc_level2_bwd_ok(&sg[s], &sc[s], &sx[s], &sa[s], &dout[s])) {
                if (deferred2) X.rc(PC_EINVAL);         // (pool_add_plan2 asked the same predicate of the same layout)
                X.ar.off = mark;
                return false;
            }
            if (deferred2) { dpg[s] = D(g_pooled[s]); d[s].pool_grad_out = &dpg[s]; }
        }
        int nwg = 0;
        if (X.go()) X.rc(pc_level2_bwd_group(NS, d, B, &nwg, X.st));
        for (int s = 0; s < NS; ++s) {
            R.add(w1[s], ST[s].dw[L_D2A], ST[s].db[L_D2A], nwg, 16, 16, 0);
            R.add(w2[s], ST[s].dw[L_D2B], ST[s].db[L_D2B], nwg, 16, 16, 0);
        }
        if (deferred2) {
            // pool-add order (pool_add_plan2): the Up block's skip-halves launch scatters the level's raw data gradient while it writes g_in
            deferred2 = false;
            bwd_halves(UP2.conv, deferred_g2, saved(UP2.skip), X.bn_half, g_in, 32, 2 * h, 2 * w, &g_pooled);
        }
        return true;
    }
    // A Down block's DoubleConv at (h, w), 16 channels: the second conv, then the first conv with the max-pool scatter (+=) into g_in, the
    // gradient of the full-resolution map.
    void down(const DownLv& lv, const T2& g_out, T2& g_in, int h, int w) {
        const T2 mid = saved(lv.mid), pooled = saved(lv.pooled), full = saved(lv.full);
        T2 g_mid = fresh(16, h, w);
        if (deferred && lv.cin == 8) {
            // pool-add order (pool_add_plan): the first layer's raw data gradient stays at the pooled resolution; the Up block's deferred skip
            // launch scatters it into g_in while it writes that map -- once
            deferred = false;
            T2 g_pooled = fresh(lv.cin, h, w);
            bwd_halves(lv.conv2, g_out, mid, X.bn_half_d1a, g_mid, 16, h, w);
            Blk a[2], b[2];
            for (int s = 0; s < NS; ++s) a[s] = Blk{&g_mid[s], &pooled[s], nullptr, &g_pooled[s], lv.conv1, s, 0, true};
            bwd8(a, NS, lv.cin, h, w);
            for (int s = 0; s < NS; ++s)
                b[s] = Blk{&deferred_g[s], &full[s], &X.bn_nobias[s][lv.full_act], &g_in[s], UP1.conv, s, 0, true, nullptr, &g_pooled[s]};
            bwd8(b, NS, 16, 2 * h, 2 * w);
            return;
        }
        // down1, round 6: data + weight gradient of each layer in ONE launch of the split-operand kernel -- the second conv as the two
        // 8-channel halves of its input over the same 16-channel gradient (two problems per stream), the first with the max-pool scatter
        // into inc2's gradient -- instead of four launches (weight gradient 16 -> 16, data gradient 16 -> 16, weight gradient 8 -> 16,
        // pooled data gradient 16 -> 8).  Both layers take it, or neither; the launcher declines a 16-channel pooled map (down2).
        bool fused = lv.cin == 8;
        for (int s = 0; s < NS && fused; ++s)
            fused = bwd_ok(g_out[s], chans(mid[s], 8, 8), chans(g_mid[s], 8, 8), nullptr, h, w) && bwd_ok(g_mid[s], pooled[s], g_in[s], &full[s], h, w);
        if (fused) {
            bwd_halves(lv.conv2, g_out, mid, X.bn_half_d1a, g_mid, 16, h, w);
            Blk a[2];
            for (int s = 0; s < NS; ++s) a[s] = Blk{&g_mid[s], &pooled[s], &X.bn_nobias[s][lv.full_act], &g_in[s], lv.conv1, s, 0, true, &full[s]};
            bwd8(a, NS, lv.cin, h, w);
            return;
        }
        wgrad(lv.conv2, mid, PC_SRC_DIRECT, g_out, h, w);
        dgrad(lv.conv2, g_out, g_mid, 16, mid, lv.conv1, false, h, w);
        // (the forward saves the pooled map where the full one's width is a multiple of 32: always at level 1, at level 2 when W1 % 32 == 0)
        if (pooled[0].ok()) wgrad(lv.conv1, pooled, PC_SRC_DIRECT, g_mid, h, w);
        else wgrad(lv.conv1, full, PC_SRC_POOL2, g_mid, h, w);
        dgrad(lv.conv1, g_mid, g_in, lv.cin, full, lv.full_act, true, h, w);
    }
    // first layers: weight gradients only, one launch per stream (2 / 4 input channels) over the padded input
    void first_layer(const T2& G_a1) {
        int c0 = 0;
        side_on();
        for (int s = 0; s < NS; ++s) {
            const Ten xin = chans(X.Xp_u, c0, ST[s].cin);
            const pc_src sa = S(xin), sg = S(G_a1[s]);
            void* ws = slot();
            int nwg = 0;
            if (X.go()) X.rc(pc_conv3x3_wgrad_partial(&sa, nullptr, &sg, ws, B, X.Hp, X.Wp, ST[s].cin, 8, &nwg, X.st));
            R.add(ws, ST[s].dw[L_INC1], ST[s].db[L_INC1], nwg, ST[s].cin, 8, 0);
            c0 += ST[s].cin;
        }
        side_off();
    }
    // ONE batched fixed-order reduction for all layers (+ the head), then the chain rule of the composed levels
    void finish() {
        if (side_used && X.go()) {         // join: the reduction reads the side stream's partials
            X.rc((int)hipEventRecord(X.ev_join, X.side));
            X.rc((int)hipStreamWaitEvent(main_st, X.ev_join, 0));
        }
        if (X.go()) X.rc(pc_wgrad_reduce_batch(R.n, R.e, X.st));
        if (R.n8 && R.n16) {
            if (X.go()) X.rc(pc_conv3x3_up_chain_both(R.n8, R.ch8, R.nwg8, R.n16, R.ch16, R.nwg16, 0, X.st));
        } else {
            if (R.n8 && X.go()) X.rc(pc_conv3x3_up_chain_group(R.n8, R.ch8, 0, R.nwg8, 8, 8, X.st));
            if (R.n16 && X.go()) X.rc(pc_conv3x3_up_chain_group(R.n16, R.ch16, 0, R.nwg16, 16, 16, X.st));
        }
    }
};

void backward(Step& X, pc_step_io& io) {
    const pc_step_plan& P = X.plan;
    Arena& A = X.ar;
    const int B = X.B, H = X.H, W = X.W, Hp = X.Hp, Wp = X.Wp;
    const int H1 = Hp / 2, W1 = Wp / 2, H2 = H1 / 2, W2 = W1 / 2;
    A.off = X.fwd_end;
    // loss forward + backward (utils/losses.py:49-76); single process: also finishes popcount / stats of the head forward
    float* g_pd = nullptr;
    if (X.fwd_units) {
        // multi-unit: the N unit sums and the loss over the N (b, k) pairs, then its gradient painted onto the units' pixels
        const Step::Units& U = X.U;
        g_pd = reinterpret_cast<float*>(A.raw((int64_t)B * H * W * 4));
        if (X.go())
            X.rc(pc_unit_popcount_loss(X.popdense, U.slot, U.unit_off, U.dest, U.y_sorted, U.ws, U.pc_sorted, U.pc_caller, P.stats_dev, P.lam4,
                                       P.scale_regularization, P.lam_weak, B, H, W, U.N, P.loss_dev, U.g_pc, P.g_scale_const_dev, X.st));
        X.launches += 1;           // (accumulate + finish / loss)
        if (X.go()) X.rc(pc_unit_paint(U.g_pc, U.slot, g_pd, (int64_t)B * H * W, U.N, X.st));
    } else if (X.deferred_popcount) {
        if (X.go())
            X.rc(pc_head_popcount_loss(X.head_ws, B, H, W, X.counts, io.y, P.lam4, P.scale_regularization, P.lam_weak, io.inv_B, X.popcount,
                                       P.stats_dev, P.loss_dev, X.g_pc, P.g_scale_const_dev, X.st));
    } else if (X.go()) {
        X.rc(pc_loss_fwd_bwd(X.popcount, io.y, P.stats_dev, P.lam4, P.scale_regularization, P.lam_weak, io.inv_B, B, P.loss_dev, X.g_pc,
                             P.g_scale_const_dev, X.st));
    }
    // head backward: the 8 head gradients (partials, finished by the batched reduction below) + dL/d(conv outputs of the up1b layers)
    const Ten G = A.act(B, 16, Hp, Wp, /*dense=*/true);
    {
        const pc_src sf = S(X.feats);
        const pc_dst dg = D(G);
        const bool defer = !X.unet_ng;
        if (X.go())
            X.rc(pc_head_bwd(&sf, X.pt, X.pl, X.hw, X.mask, X.bld, g_pd ? nullptr : io.admin_mask, g_pd ? nullptr : io.census_idx,
                             g_pd ? nullptr : X.g_pc, g_pd, nullptr,
                             P.g_scale_const_dev, X.hdw, 0, &dg, X.unet_ng ? nullptr : &X.feat_bn[0],
                             X.unet_ng ? nullptr : &X.feat_bn[1], Hp, Wp, X.head_ws, B, H, W,
                             PC_HEAD_BWD_PACKED | (defer ? PC_HEAD_BWD_DEFER_REDUCE : 0), X.st));
        if (!defer) X.launches += 1;
    }
    if (X.unet_ng || X.enc_ng) {
        // parameters without a gradient in this regime keep exact zeros in the flat buffer (the clip norm runs over all of it)
        if (X.go()) X.rc(pc_zero_fill(P.flat_g, P.n - P.n_head, X.st));
    }
    // one stream: the live half of the first layer's 64 x 16 gradient image -> the parameter's gradient, behind the reduction that
    // finishes the image (the head's own here, the batched one of finish() below) and in front of the gradient norm of update()
    auto extract_dw0 = [&]() {
        if (!X.one() || !X.go()) return;
        hipLaunchKernelGGL(head_dw0_extract_kernel, dim3(1), dim3(256), 0, X.st, X.dw0_img, P.head_dw[0], X.cs[0].feat_c0);
        X.rc((int)hipGetLastError());
    };
    if (X.unet_ng) return extract_dw0();

    Backward p(X);
    {
        // the head's partials
        const float* pp = nullptr;
        int nwg = 0;
        pc_head_bwd_partials(X.head_ws, B, H, W, &pp, &nwg);
        for (int t = 0; t < 8; ++t) p.R.head_ptrs[t] = X.hdw[t];
        p.R.add(pp, reinterpret_cast<float*>(p.R.head_ptrs), nullptr, nwg, 0, 0, 3);
    }
    // the network in reverse, one call per block (engine.py: UNetEngine.backward)
    T2 G_f2, G_a2, G_e2, G_b2, G_c2;
    for (int s = 0; s < X.ns; ++s) G_f2[s] = chans(G, p.ST[s].feat_c0, 8);
    const T2 G_f1 = p.conv8(L_UP1B, G_f2, &Saved::f1, L_UP1A, Hp, Wp);
    p.up(UP1, G_f1, Hp, Wp, G_a2, &G_e2);
    const T2 G_e1 = p.conv8(L_UP2B, G_e2, &Saved::e1, L_UP2A, H1, W1);
    p.up(UP2, G_e1, H1, W1, G_b2, X.enc_ng ? nullptr : &G_c2);
    if (!X.enc_ng) {
        if (!p.level2(G_c2, G_b2, H2, W2)) p.down(DOWN2, G_c2, G_b2, H2, W2);
        p.down(DOWN1, G_b2, G_a2, H1, W1);
        const T2 G_a1 = p.conv8(L_INC2, G_a2, &Saved::a1, L_INC1, Hp, Wp);
        p.first_layer(G_a1);
    }
    p.finish();
    extract_dw0();
}

void update(Step& X) {
    const pc_step_plan& P = X.plan;
    pc_adam_groups g = P.groups;
    g.active_mask = X.unet_ng ? 4 : (X.enc_ng ? 6 : 7);          // groups: 0 = encoder, 1 = decoder, 2 = head
    if (X.go())
        X.rc(pc_adam_clip_step_fused(P.flat_p, P.flat_g, P.adam_m, P.adam_v, P.n, P.n_decay, P.hyper_dev, P.weight_decay, P.beta1, P.beta2,
                                     P.eps, P.max_norm, P.norm_dev, P.step_dev, &g, X.st));
}

int run(Step& X, pc_step_io& io, int phases, bool dry) {
    X.ar.dry = dry;
    X.ar.base = dry ? reinterpret_cast<char*>((uintptr_t)1 << 40) : reinterpret_cast<char*>(io.arena);
    X.ar.cap = io.arena_bytes;
    X.ar.peak = 0;
    X.err = 0;
    X.launches = 0;
    if (phases & PC_STEP_FWD) {
        X.ar.off = 0;
        forward(X, io);
    }
    if ((phases & PC_STEP_BWD) && X.err == 0) {
        if (!X.have_fwd) return PC_EINVAL;
        backward(X, io);
    }
    if ((phases & PC_STEP_UPD) && X.err == 0) update(X);
    return X.err;
}

}  // namespace

namespace {
// ---- the side stream must not share a hardware queue with the caller's stream -----------------------------------------------------
// HIP multiplexes its streams onto a handful of hardware queues (4 by default) in creation order: a side stream that lands on the
// caller's queue runs its kernels IN ORDER with the caller's, and the fork buys nothing (the same effect serialised the copy stream of
// bench.py's host-feed legs in round 4: popcorn_amd/data/feed.py).  Which stream aliases depends on what the process created before, so
// the choice is MEASURED at the first step on a caller's stream, with the launch pattern of a small-region step: a fork, twelve 10 us
// spin kernels on either stream with a cross-stream dependency every fourth one (the backward's side_on), a join.  (Two long kernels
// alone overlap even on a shared queue; what serialises a shared queue are the barrier packets of the event waits: 1.47 instead of
// 0.57 ms per 2 x 230 x 220 step, tools/step_side_alias_probe.py.)  About 130 us when the two chains run side by side, 250+ when they
// do not; up to six fresh streams are tried, the first that overlaps is kept.
__global__ void step_spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

void pick_side_stream(Step& X, hipStream_t main_st) {
    X.side_picked = true;
    X.side_for = main_st;
    if (!X.side) return;
    // a caller's stream that was measured before keeps its side stream (a trainer stepped alternately from two streams used to pay the
    // probe -- a host synchronisation + ~3 ms of spin kernels -- at every step: ADVICE round 5)
    for (int i = 0; i < X.n_side_cache; ++i)
        if (X.side_cache[i].caller == main_st) { X.side = X.side_cache[i].side; return; }
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) {
        (void)hipGetLastError();
        if (t0) (void)hipEventDestroy(t0);
        return;
    }
    const long long ticks = 10 * 100;                       // 10 us of the 100 MHz wall clock
    // the pattern on the caller's stream ALONE: the yardstick of this GPU / clock (two chains side by side take about as long, two
    // chains through one hardware queue about twice as long) -- no absolute threshold
    float base_ms = 1e9f;
    for (int rep = 0; rep < 2; ++rep) {
        bool ok = hipEventRecord(t0, main_st) == hipSuccess;
        for (int i = 0; i < 12; ++i) hipLaunchKernelGGL(step_spin_kernel, dim3(1), dim3(64), 0, main_st, ticks);
        ok = ok && hipEventRecord(t1, main_st) == hipSuccess && hipEventSynchronize(t1) == hipSuccess;
        float e = 1e9f;
        if (!ok || hipEventElapsedTime(&e, t0, t1) != hipSuccess) { (void)hipGetLastError(); e = 1e9f; }
        if (rep == 1) base_ms = e;
    }
    hipStream_t best = X.side;
    float best_ms = 1e9f;
    hipStream_t cand = X.side;
    hipStream_t tried[6];
    int ntried = 0;
    for (int k = 0; k < 6 && cand; ++k) {
        tried[ntried++] = cand;
        float ms = 1e9f;
        for (int rep = 0; rep < 2; ++rep) {                 // (the first round also absorbs the kernel's first-launch cost)
            bool ok = hipEventRecord(t0, main_st) == hipSuccess && hipEventRecord(X.ev_fork, main_st) == hipSuccess &&
                      hipStreamWaitEvent(cand, X.ev_fork, 0) == hipSuccess;
            for (int i = 0; i < 12; ++i) {
                hipLaunchKernelGGL(step_spin_kernel, dim3(1), dim3(64), 0, main_st, ticks);
                hipLaunchKernelGGL(step_spin_kernel, dim3(1), dim3(64), 0, cand, ticks);
                if ((i & 3) == 3 && i < 11)
                    ok = ok && hipEventRecord(X.ev_dep[i >> 2], main_st) == hipSuccess && hipStreamWaitEvent(cand, X.ev_dep[i >> 2], 0) == hipSuccess;
            }
            ok = ok && hipEventRecord(X.ev_join, cand) == hipSuccess && hipStreamWaitEvent(main_st, X.ev_join, 0) == hipSuccess &&
                 hipEventRecord(t1, main_st) == hipSuccess && hipEventSynchronize(t1) == hipSuccess;
            float e = 1e9f;
            if (!ok || hipEventElapsedTime(&e, t0, t1) != hipSuccess) { (void)hipGetLastError(); e = 1e9f; }
            if (rep == 1) ms = e;
        }
        if (ms < best_ms) { best_ms = ms; best = cand; }
        if (ms < 1.45f * base_ms) break;                    // side by side
        cand = nullptr;
        if (k + 1 < 6 && hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); cand = nullptr; }
    }
    // streams that lost are destroyed unless an earlier caller's entry of the cache uses them
    for (int i = 0; i < ntried; ++i) {
        bool cached = false;
        for (int c = 0; c < X.n_side_cache; ++c) cached = cached || X.side_cache[c].side == tried[i];
        if (tried[i] != best && !cached) (void)hipStreamDestroy(tried[i]);
    }
    X.side = best;
    if (X.n_side_cache < 4) { X.side_cache[X.n_side_cache].caller = main_st; X.side_cache[X.n_side_cache].side = best; ++X.n_side_cache; }
    if (getenv("POPCORN_CONV_DBG"))
        fprintf(stderr, "pc_train_step: side stream %p, probe pattern took %.3f ms against %.3f ms on the caller's stream alone (%d tried)\n",
                (void*)best, best_ms, base_ms, ntried);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
}

}  // namespace

// debug (tools/host_time_eager.py): host nanoseconds of the last call's sizing pass and of its launching pass
static double g_step_host_ns[2] = {0, 0};
extern "C" void pc_debug_step_host_ns(double* out) { out[0] = g_step_host_ns[0]; out[1] = g_step_host_ns[1]; }

extern "C" void* pc_step_create(const pc_step_plan* plan) {
    if (!plan) return nullptr;
    Step* X = new (std::nothrow) Step();
    if (!X) return nullptr;
    X->plan = *plan;
    // the present streams.  A plan whose two networks disagree, or without a stream, still makes a handle: every entry point refuses it
    // (plan_streams_ok) before anything is enqueued
    X->ns = 0;
    for (int s = 0; s < 2; ++s)
        if (stream_present(plan->unet.s[s])) X->ps[X->ns++] = s;
    memset(X->cs, 0, sizeof(X->cs));
    memset(X->feat_bn, 0, sizeof(X->feat_bn));
    X->feat_bn[0].eps = X->feat_bn[1].eps = 1e-5f;          // (plain: engine.py: feat_bn of a missing stream)
    for (int s = 0; s < 2; ++s) {
        if (s >= X->ns) {
            memset(X->bn_nobias[s], 0, sizeof(X->bn_nobias[s]));
            memset(X->bn_half[s], 0, sizeof(X->bn_half[s]));
            memset(X->bn_half_d1a[s], 0, sizeof(X->bn_half_d1a[s]));
            continue;
        }
        const pc_step_stream& T = plan->unet.s[X->ps[s]];
        X->cs[s] = T;
        for (int L = 0; L < PC_STEP_CONVS; ++L) {
            X->bn_nobias[s][L] = T.bn[L];
            X->bn_nobias[s][L].conv_bias = nullptr;
        }
        X->feat_bn[T.feat_c0 == 8 ? 1 : 0] = X->bn_nobias[s][L_UP1B];
        for (int i = 0; i < 2; ++i) {         // d1b's ReLU / BN factor for channels [8 i, 8 i + 8)
            pc_bn b = X->bn_nobias[s][L_D1B];
            if (b.gamma) { b.gamma += 8 * i; b.beta += 8 * i; b.mean += 8 * i; b.var += 8 * i; }
            X->bn_half[s][i] = b;
            pc_bn a = X->bn_nobias[s][L_D1A];
            if (a.gamma) { a.gamma += 8 * i; a.beta += 8 * i; a.mean += 8 * i; a.var += 8 * i; }
            X->bn_half_d1a[s][i] = a;
        }
    }
    float one[2] = {1.f, 1.f};
    if (hipMalloc(reinterpret_cast<void**>(&X->ones2), sizeof(one)) != hipSuccess ||
        hipMemcpy(X->ones2, one, sizeof(one), hipMemcpyHostToDevice) != hipSuccess) {
        delete X;
        return nullptr;
    }
    {
        const char* ev = getenv("POPCORN_STEP_SIDE_PX");          // A/B switch: 0 = never fork
        X->side_px = ev ? atoll(ev) : PC_STEP_SIDE_PX_DEFAULT;
        if (X->side_px > 0 && (hipStreamCreateWithFlags(&X->side, hipStreamNonBlocking) != hipSuccess ||
                               hipEventCreateWithFlags(&X->ev_fork, hipEventDisableTiming) != hipSuccess ||
                               hipEventCreateWithFlags(&X->ev_join, hipEventDisableTiming) != hipSuccess)) {
            (void)hipGetLastError();
            X->side = nullptr;                                    // no side stream: the sequential form
        }
        for (int i = 0; i < 8 && X->side; ++i)
            if (hipEventCreateWithFlags(&X->ev_dep[i], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); X->side = nullptr; }
        // backward: measured on 2 x H x W regions (tools/ab_regions.sh): -2 % .. -1 % up to 4.3 Mpx, +1.5 % from 7 Mpx on
        const char* eb = getenv("POPCORN_STEP_SIDE_BWD_PX");      // A/B switch: 0 = weight-gradient launches stay on the caller's stream
        X->side_bwd_px = eb ? atoll(eb) : 5000000ll;
    }
    return X;
}

extern "C" void pc_step_destroy(void* handle) {
    Step* X = reinterpret_cast<Step*>(handle);
    if (!X) return;
    if (X->ones2) (void)hipFree(X->ones2);
    if (X->ev_fork) (void)hipEventDestroy(X->ev_fork);
    if (X->ev_join) (void)hipEventDestroy(X->ev_join);
    for (int i = 0; i < 8; ++i)
        if (X->ev_dep[i]) (void)hipEventDestroy(X->ev_dep[i]);
    for (int i = 0; i < X->n_side_cache; ++i) {                 // side streams kept for other callers' streams
        bool dup = X->side_cache[i].side == X->side;
        for (int k = 0; k < i; ++k) dup = dup || X->side_cache[k].side == X->side_cache[i].side;
        if (!dup && X->side_cache[i].side) (void)hipStreamDestroy(X->side_cache[i].side);
    }
    if (X->side) (void)hipStreamDestroy(X->side);
    delete X;
}

// any of these NULL: not a training plan (popcorn_hip.h).  pc_forward reads none of the gradient / optimiser / loss / statistics pointers
static bool inference_plan(const pc_step_plan& P) {
    return !P.flat_p || !P.flat_g || !P.adam_m || !P.adam_v || !P.loss_dev || !P.stats_dev;
}

// un: the unit lists of pc_train_step_units (checked by it), or null: one unit per sample, io->census_idx / io->y
// layer: the batch's building layer (pc_train_step_layer), or null: the frozen extractor's score
static int train_step(void* handle, pc_step_io* io, pc_step_units* un, const float* layer, int phases, void* stream) {
    Step* X = reinterpret_cast<Step*>(handle);
    if (!X || !io || io->B < 1 || io->H < 1 || io->W < 1 || !(phases & 7)) return PC_EINVAL;
    if (inference_plan(X->plan)) return PC_EINVAL;          // (a plan without gradient / optimiser / loss targets serves pc_forward only)
    if (int bad = plan_streams_ok(X->plan)) return bad;     // (a stream in one network only, or none)
    // a backward / update phase continues the forward pass in the arena: its layer, named again or left out
    if (!(phases & PC_STEP_FWD) && layer && layer != X->fwd_layer) return PC_EINVAL;
    if (g_pc_precision != PC_PREC_FP32) return PC_ENOTSUP;
    if ((phases & PC_STEP_FWD) && (!io->data || !io->admin_mask || (!un && !io->census_idx) || (!io->sel && !io->sel_host) ||
                                   (io->sel_host && io->H + io->W > PC_STEP_SEL_MAX) || (io->data_kind == PC_DATA_SPLIT && !io->data2)))
        return PC_EINVAL;
    if ((phases & PC_STEP_BWD) && !un && !io->y) return PC_EINVAL;
    // a backward phase continues the forward pass that is in the arena: of the same kind
    if ((phases & PC_STEP_BWD) && !(phases & PC_STEP_FWD) && X->have_fwd && X->fwd_units != (un != nullptr)) return PC_EINVAL;
    X->un = un;
    X->layer = layer;
    if (phases & PC_STEP_FWD) {
        int pt, pb, pl, pr;
        pad_geometry(io->H, io->W, pt, pb, pl, pr);
        const int p = X->plan.extractor_pad;
        // reflect padding must be smaller than the input (F.pad's rule); two 2 x 2 poolings need a 4 x 4 domain
        if (pt >= io->H || pb >= io->H || pl >= io->W || pr >= io->W || p >= io->H || p >= io->W) return PC_EINVAL;
        // one-stream plan, PC_DATA_INPUT: the stream's channels must lie inside the tensor (the ingest would refuse after the first launches)
        if (X->one() && io->data_kind == PC_DATA_INPUT)
            for (int c = 0; c < X->cs[0].cin; ++c)
                if (X->cs[0].chan[c] < 0 || X->cs[0].chan[c] >= input_channels(*X, *io)) return PC_EINVAL;
    }
    X->st = reinterpret_cast<hipStream_t>(stream);
    // An EAGER entry point: it forks onto a side stream through events of its own, and the first call on a caller's stream measures
    // which side stream runs beside it (a host synchronisation).  Under stream capture neither is legal: say so instead of failing
    // inside the probe with an opaque HIP error (captured steps go through the per-launch entry points, train.py: _capture).
    {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(X->st, &cs) != hipSuccess) { (void)hipGetLastError(); return PC_EINVAL; }
        if (cs != hipStreamCaptureStatusNone) return PC_ENOTSUP;
    }
    // dry pass: the same code path with launches off -- sizes the arena (bump allocation is deterministic)
    // (a FWD-only call of a data-parallel step is sized for its BWD / UPD calls too: they continue in the same arena)
    const auto t_a = std::chrono::steady_clock::now();
    Step probe = *X;
    int rc = run(probe, *io, (phases & PC_STEP_FWD) ? (PC_STEP_FWD | PC_STEP_BWD | PC_STEP_UPD) : phases, true);
    if (rc) return rc;
    io->arena_needed = probe.ar.peak + 256;
    if (!io->arena || io->arena_bytes < io->arena_needed || (reinterpret_cast<uintptr_t>(io->arena) & 255)) return PC_ENOMEM;
    // (the side-stream probe only once the call is going to launch: a call that returns PC_ENOMEM has not paid for it)
    if (X->side && (!X->side_picked || X->side_for != X->st)) pick_side_stream(*X, X->st);
    const auto t_b = std::chrono::steady_clock::now();
    rc = run(*X, *io, phases, false);
    io->launches = X->launches;
    g_step_host_ns[0] = std::chrono::duration<double, std::nano>(t_b - t_a).count();
    g_step_host_ns[1] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t_b).count();
    return rc;
}

extern "C" int pc_train_step_layer(void* handle, pc_step_io* io, const float* layer, int phases, void* stream) {
    if (!handle || !io || (reinterpret_cast<uintptr_t>(layer) & 3)) return PC_EINVAL;      // (before the handle is looked at)
    const int rc = train_step(handle, io, nullptr, layer, phases, stream);
    reinterpret_cast<Step*>(handle)->layer = nullptr;       // (the layer is the caller's: only fwd_layer, compared and never read, outlives the call)
    return rc;
}

extern "C" int pc_train_step(void* handle, pc_step_io* io, int phases, void* stream) { return pc_train_step_layer(handle, io, nullptr, phases, stream); }

extern "C" int pc_train_step_units_layer(void* handle, pc_step_io* io, pc_step_units* u, const float* layer, int phases, void* stream) {
    // every check of the lists comes before the handle is looked at: nothing here touches a device
    if (reinterpret_cast<uintptr_t>(layer) & 3) return PC_EINVAL;
    if (!handle || !io || !u || !u->census_idx || !u->y || !u->census_n || u->K < 1 || u->N < 1 || io->B < 1) return PC_EINVAL;
    if (u->K > PC_UNIT_LAYOUT_MAX_K || io->B > PC_UNIT_LAYOUT_MAX_B || io->dp != 0) return PC_ENOTSUP;
    int64_t n = 0;
    for (int b = 0; b < io->B; ++b) {
        if (u->census_n[b] < 1 || u->census_n[b] > u->K) return PC_EINVAL;
        n += u->census_n[b];
    }
    if (n != u->N) return PC_EINVAL;
    // (the unit sums' range, pc_unit_popcount: a unit's integer sums cannot wrap below 2^27 pixels per sample)
    if ((int64_t)io->H * io->W >= ((int64_t)1 << 27) || (int64_t)io->B * io->H * io->W >= ((int64_t)1 << 31)) return PC_ENOTSUP;
    const int rc = train_step(handle, io, u, layer, phases, stream);
    reinterpret_cast<Step*>(handle)->un = nullptr;          // (the lists are the caller's: no pointer to them outlives the call)
    reinterpret_cast<Step*>(handle)->layer = nullptr;
    return rc;
}

extern "C" int pc_train_step_units(void* handle, pc_step_io* io, pc_step_units* u, int phases, void* stream) {
    return pc_train_step_units_layer(handle, io, u, nullptr, phases, stream);
}

// ---- pc_forward: inference and validation in one call (popcorn_hip.h) ------------------------------------------------------------------
extern "C" int pc_sizeof_fwd_io(void) { return (int)sizeof(pc_fwd_io); }

extern "C" int pc_forward(void* handle, pc_fwd_io* fio, const float* layer, void* stream) {
    Step* X = reinterpret_cast<Step*>(handle);
    if (!X || !fio || (reinterpret_cast<uintptr_t>(layer) & 3)) return PC_EINVAL;
    if (fio->B < 1 || fio->H < 1 || fio->W < 1) return PC_EINVAL;
    if (g_pc_precision != PC_PREC_FP32) return PC_ENOTSUP;
    const pc_step_plan& P = X->plan;
    for (int s = 0; s < 2; ++s)               // single-modality plan: one stream's table is empty
        if (P.unet.s[s].cin < 1 || !P.unet.s[s].w[0] || !P.extractor.s[s].w[0]) return PC_ENOTSUP;
    if ((int64_t)fio->B * fio->H * fio->W >= ((int64_t)1 << 31)) return PC_ENOTSUP;
    if (!fio->data || (fio->data_kind == PC_DATA_SPLIT && !fio->data2) || (fio->admin_mask == nullptr) != (fio->census_idx == nullptr))
        return PC_EINVAL;
    if (fio->data_kind != PC_DATA_INPUT && fio->data_kind != PC_DATA_RAW && fio->data_kind != PC_DATA_SPLIT) return PC_EINVAL;
    {
        int pt, pb, pl, pr;
        pad_geometry(fio->H, fio->W, pt, pb, pl, pr);
        const int p = P.extractor_pad;
        // the reflect rule of train_step (the extractor's pad is checked with a layer too: one rule per geometry)
        if (pt >= fio->H || pb >= fio->H || pl >= fio->W || pr >= fio->W || p >= fio->H || p >= fio->W) return PC_EINVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    {
        // an eager entry point, as pc_train_step: the fork's events and the side-stream probe are illegal under capture
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return PC_EINVAL; }
        if (cs != hipStreamCaptureStatusNone) return PC_ENOTSUP;
    }
    pc_step_io io;
    memset(&io, 0, sizeof(io));
    io.B = fio->B; io.H = fio->H; io.W = fio->W; io.data_kind = fio->data_kind;
    io.data = fio->data; io.data2 = fio->data2; io.craw = fio->craw;
    io.admin_mask = fio->admin_mask; io.census_idx = fio->census_idx;
    io.encoder_no_grad = 1; io.unet_no_grad = 1;
    io.arena = fio->arena; io.arena_bytes = fio->arena_bytes;
    // the pass runs on a copy of the handle: the context a training step keeps between its phases stays as it is
    const auto t_a = std::chrono::steady_clock::now();
    Step work = *X;
    work.infer = true;
    work.dense_rule = (fio->flags & PC_FWD_DENSE_ROW_RULE) != 0;
    work.un = nullptr;
    work.layer = layer;
    work.st = st;
    int rc = run(work, io, PC_STEP_FWD, true);
    if (rc) return rc;
    fio->arena_needed = work.ar.peak + 256;
    if (!fio->arena || fio->arena_bytes < fio->arena_needed || (reinterpret_cast<uintptr_t>(fio->arena) & 255)) return PC_ENOMEM;
    if (X->side && (!X->side_picked || X->side_for != st)) {
        pick_side_stream(*X, st);          // (which stream runs beside the caller's: the handle's, not a step's context)
        work.side = X->side;
    }
    const auto t_b = std::chrono::steady_clock::now();
    rc = run(work, io, PC_STEP_FWD, false);
    fio->off_popcount = io.off_popcount; fio->off_popdense = io.off_popdense; fio->off_scale = io.off_scale;
    fio->off_building = io.off_building;
    fio->launches = work.launches;
    g_step_host_ns[0] = std::chrono::duration<double, std::nano>(t_b - t_a).count();
    g_step_host_ns[1] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t_b).count();
    return rc;
}
