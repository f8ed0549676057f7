// region_repair.hip -- NaN repair of a resident plan, planned ONCE: the counts that choose an item's S1 orbit, the sparse table of repaired
// sites, and the launch that lays a batch's patches over it.
//
// The reference repairs every weaksup item it loads (data/PopulationDataset.py:419-441): S2 is filled where it holds NaN, the descending S1
// below 5 % NaN, otherwise the ascending orbit under the same rule.  An item's repaired values depend only on (crop, season, orbit), and a
// resident plan fixes all three before the first step, so the answer is computed when the plan is made (data/region.py: plan_repair):
//
//   pc_region_nan_census   counts[k] = {NaN entries of S2 over its four selected bands, of the descending S1 over its two, of the ascending
//                          S1 likewise} of box k = {x0, x1, y0, y1, season}: ONE pass over a DEVICE list of boxes.  One workgroup per (box,
//                          block of CN_ROWS rows), the loads of region_load.h (four pixels per access at the source's natural alignment,
//                          element by element across the box's edge), a wave64 reduction, one 64-bit vector atomic add (three lanes: the
//                          three counts) per workgroup, after an init launch that writes every element.  Integer adds only: the same bits
//                          for any launch geometry.  The kernel clamps every box to the rasters, whatever the device list holds
//   pc_region_patch_count  per (item, chunk of PC_REGION_PATCH_CHUNK entries of the item's own (6, h_b, w_b) index space): the entries
//                          whose 32-bit pattern differs between the gathered and the filled tile; every count is written by its owner
//   pc_region_patch_write  the same scan again; an entry's place is its chunk's offset (an exclusive prefix the host takes between the
//                          two) + the differing entries before it in the chunk: __ballot / __popcll of the lanes below (a 64-bit mask),
//                          the waves before it through LDS, the rounds before it in a register -- ascending and deterministic
//   pc_region_patch_apply  threads run flat over the entries of up to PC_REGION_GATHER_MAX_B items, each finds its item by a search in the
//                          prefix counts (kernel arguments) and stores its value at the image of its tile position under the batch's flips
//                          and quarter turns (region_index.h, shared with region_batch.hip), S2 entries through pc_aug_s2_value
//                          (aug_value.h): plain 4-byte stores, each bounded by the entry's own item
//
// No loop's trip count depends on another lane's, wave's or workgroup's progress.
#include "common.h"
#include "aug_value.h"
#include "region_args.h"
#include "region_index.h"
#include "region_load.h"

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_WAVES = RR_THREADS / 64;
constexpr int CN_ROWS = 16;                // rows of a census work item
constexpr int CN_MAX_BLOCKS = 4096;        // workgroups of the census pass
constexpr int PA_MAX_BLOCKS = 4096;        // workgroups of a patch-apply launch
static_assert(PC_REGION_PATCH_CHUNK % RR_THREADS == 0, "a chunk is whole rounds of the workgroup");

typedef unsigned long long rr_u64;

// ---- the census ------------------------------------------------------------------------------------------------------------------------
struct RegionCensusArgs {
    RegionSources src;                      // (no boundary: the census reads none)
    const int32_t* boxes;
    int S, n;
    int nrb;                                // row blocks per box: ceil(rows_max / CN_ROWS)
    int64_t items;                          // n * nrb
    rr_u64* counts;                         // [n][3]
};

__global__ __launch_bounds__(256) void region_census_init_kernel(rr_u64* counts, int64_t n3) {
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n3; i += (int64_t)gridDim.x * 256) counts[i] = 0;
}

__device__ __forceinline__ int rr_nan4(f32x4 v) { return (v[0] != v[0]) + (v[1] != v[1]) + (v[2] != v[2]) + (v[3] != v[3]); }

// T2 = float: S2 can hold NaN; T2 = uint16_t: it cannot, and is not read
template <typename T2>
__global__ __launch_bounds__(RR_THREADS) void region_census_kernel(const RegionCensusArgs a) {
    __shared__ int part[RR_WAVES][3];
    const int t = threadIdx.x;
    const RegionSources& rs = a.src;
    const int64_t plane = (int64_t)rs.h * rs.w;
    for (int64_t it = blockIdx.x; it < a.items; it += gridDim.x) {      // (the same trip count for every thread of the workgroup)
        const int k = (int)(it / a.nrb), rb = (int)(it - (int64_t)k * a.nrb);
        const int32_t* box = a.boxes + 5 * (int64_t)k;
        // the box, clamped to the raster whatever the list holds: no address outside the sources is ever formed
        const int x0 = min(max(box[0], 0), rs.h), x1 = min(max(box[1], x0), rs.h);
        const int y0 = min(max(box[2], 0), rs.w), y1 = min(max(box[3], y0), rs.w);
        const int season = min(max(box[4], 0), a.S - 1);
        const int hb = x1 - x0, wb = y1 - y0;
        const int r0 = rb * CN_ROWS;
        if (r0 >= hb || wb == 0) continue;                               // (uniform over the workgroup: no barrier is skipped by a part of it)
        const int rows = min(CN_ROWS, hb - r0);
        const T2* s2 = reinterpret_cast<const T2*>(rs.s2) + (int64_t)season * rs.C2 * plane;
        const float* s1 = rs.s1 + (int64_t)season * rs.C1 * plane;
        const float* sa = rs.s1_asc ? rs.s1_asc + (int64_t)season * rs.C1 * plane : nullptr;
        const int wg = (wb + 3) >> 2, groups = rows * wg;                // (rows * wg <= 16 * 2^29)
        int n2 = 0, n1 = 0, na = 0;
        for (int g = t; g < groups; g += RR_THREADS) {
            const int r = g / wg, x = (g - r * wg) << 2;
            const int64_t src = (int64_t)(x0 + r0 + r) * rs.w + y0 + x;
            if (x + 4 <= wb) {
                if constexpr (sizeof(T2) == 4) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) n2 += rr_nan4(rg_ld4(s2 + rs.band2[c] * plane + src));
                }
#pragma unroll
                for (int c = 0; c < 2; ++c) n1 += rr_nan4(rg_ld4(s1 + rs.band1[c] * plane + src));
                if (sa) {
#pragma unroll
                    for (int c = 0; c < 2; ++c) na += rr_nan4(rg_ld4(sa + rs.band1[c] * plane + src));
                }
            } else {
                for (int e = 0; x + e < wb; ++e) {                       // the group across the box's right edge: element by element
                    if constexpr (sizeof(T2) == 4) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) { const float v = rg_val(s2 + rs.band2[c] * plane + src + e); n2 += v != v; }
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c) { const float v = s1[rs.band1[c] * plane + src + e]; n1 += v != v; }
                    if (sa) {
#pragma unroll
                        for (int c = 0; c < 2; ++c) { const float v = sa[rs.band1[c] * plane + src + e]; na += v != v; }
                    }
                }
            }
        }
        // wave64 reduction, then the four waves through LDS
        for (int off = 32; off > 0; off >>= 1) {
            n2 += __shfl_down(n2, off); n1 += __shfl_down(n1, off); na += __shfl_down(na, off);
        }
        __syncthreads();                                                 // the previous item's readers are done with `part`
        if ((t & 63) == 0) { part[t >> 6][0] = n2; part[t >> 6][1] = n1; part[t >> 6][2] = na; }
        __syncthreads();
        if (t < 3) {
            rr_u64 s = 0;
#pragma unroll
            for (int wv = 0; wv < RR_WAVES; ++wv) s += (rr_u64)part[wv][t];
            if (s) atomicAdd(a.counts + 3 * (int64_t)k + t, s);           // one vector atomic of three lanes per workgroup
        }
    }
}

// ---- the patch table -------------------------------------------------------------------------------------------------------------------
struct RegionPatchArgs {
    const int32_t* g2; const int32_t* f2;   // gathered / filled S2 (B, 4, Hm, Wm) as bits
    const int32_t* g1; const int32_t* f1;   // gathered / filled S1 (B, 2, Hm, Wm)
    const int32_t* data_hw;                 // (B, 2)
    int B, Hm, Wm, nchunk;
    int32_t* counts;                        // [B][nchunk]                       (count pass)
    const int64_t* chunk_off;               // [B][nchunk] places in the table    (write pass)
    int32_t* idx; int32_t* val; int64_t cap;
};

// entry e of item b's (6, hb, wb) space: do the two tiles differ there?  `bits` receives the filled tile's pattern
__device__ __forceinline__ bool rr_differs(const RegionPatchArgs& a, int b, int hb, int wb, int64_t e, int64_t n, int32_t& bits) {
    if (e >= n) return false;
    const int64_t hw = (int64_t)hb * wb;
    const int c = (int)(e / hw);
    const int rem = (int)(e - c * hw), i = rem / wb, j = rem - i * wb;
    const int64_t oplane = (int64_t)a.Hm * a.Wm, o = (int64_t)i * a.Wm + j;
    int32_t g;
    if (c < 4) { const int64_t p = ((int64_t)b * 4 + c) * oplane + o; g = a.g2[p]; bits = a.f2[p]; }
    else { const int64_t p = ((int64_t)b * 2 + (c - 4)) * oplane + o; g = a.g1[p]; bits = a.f1[p]; }
    return g != bits;
}

template <bool WRITE>
__global__ __launch_bounds__(RR_THREADS) void region_patch_kernel(const RegionPatchArgs a) {
    __shared__ int wave_n[RR_WAVES];
    const int t = threadIdx.x, b = blockIdx.y, lane = t & 63, wv = t >> 6;
    const int hb = min(max(a.data_hw[2 * b], 0), a.Hm), wb = min(max(a.data_hw[2 * b + 1], 0), a.Wm);
    const int64_t n = 6 * (int64_t)hb * wb;                              // (< 2^31: host)
    for (int ch = blockIdx.x; ch < a.nchunk; ch += gridDim.x) {          // (the same trip count for every thread of the workgroup)
        const int64_t e0 = (int64_t)ch * PC_REGION_PATCH_CHUNK;
        int64_t base = WRITE ? a.chunk_off[(int64_t)b * a.nchunk + ch] : 0;
        int total = 0;
        for (int r = 0; r < PC_REGION_PATCH_CHUNK / RR_THREADS; ++r) {
            const int64_t e = e0 + r * RR_THREADS + t;
            int32_t bits = 0;
            const bool d = rr_differs(a, b, hb, wb, e, n, bits);
            const rr_u64 m = __ballot(d);                                // 64-bit on this hardware
            __syncthreads();                                             // the previous round's readers are done with `wave_n`
            if (lane == 0) wave_n[wv] = __popcll(m);
            __syncthreads();
            int before = 0, round = 0;
#pragma unroll
            for (int k = 0; k < RR_WAVES; ++k) { const int c = wave_n[k]; round += c; if (k < wv) before += c; }
            if constexpr (WRITE) {
                if (d) {
                    const int64_t at = base + total + before + __popcll(m & (((rr_u64)1 << lane) - 1));
                    if (at >= 0 && at < a.cap) { a.idx[at] = (int32_t)e; a.val[at] = bits; }
                }
            }
            total += round;
        }
        if constexpr (!WRITE) {
            if (t == 0) a.counts[(int64_t)b * a.nchunk + ch] = total;    // the owner of this element: every count is written
        }
    }
}

// ---- the application -------------------------------------------------------------------------------------------------------------------
struct RegionPatchItem { int64_t off; int32_t start, hb, wb, _pad; };      // start: entries of the launch before this item
struct RegionPatchApplyArgs {
    const int32_t* idx; const float* val;
    float* s2; float* s1; int64_t stride2, stride1;                       // item strides in elements; already offset to the launch's first item
    int Hm, Wm, Ho, Wo, vflip, hflip, rot, bright, gam;
    float beta, gamma;
    int nb, total;                                                         // items and entries of the launch
    RegionPatchItem item[PC_REGION_GATHER_MAX_B];                          // 3,072 bytes of arguments
};

__global__ __launch_bounds__(RR_THREADS) void region_patch_apply_kernel(const RegionPatchApplyArgs a) {
    const int64_t oplane = (int64_t)a.Ho * a.Wo;
    for (int e = blockIdx.x * RR_THREADS + threadIdx.x; e < a.total; e += gridDim.x * RR_THREADS) {
        // the last item whose start is <= e (items without entries share a start with their successor and are passed over)
        int lo = 0, hi = a.nb - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.item[mid].start <= e) lo = mid; else hi = mid - 1;
        }
        const RegionPatchItem it = a.item[lo];
        const int64_t at = it.off + (e - it.start);
        const int32_t p = a.idx[at];
        const int64_t hw = (int64_t)it.hb * it.wb;
        if (p < 0 || (int64_t)p >= 6 * hw) continue;                       // bounded by the entry's own item
        const int c = (int)(p / hw);
        const int rem = (int)(p - c * hw), y = rem / it.wb, x = rem - y * it.wb;      // y < hb <= Hm, x < wb <= Wm (host)
        int i, j;
        pc_region_tile_to_out(y, x, a.Hm, a.Wm, a.vflip, a.hflip, a.rot, i, j);
        const float v = a.val[at];
        const int64_t o = (int64_t)i * a.Wo + j;
        if (c < 4) a.s2[lo * a.stride2 + c * oplane + o] = pc_aug_s2_value(v, a.bright, a.beta, a.gam, a.gamma);
        else a.s1[lo * a.stride1 + (c - 4) * oplane + o] = v;
    }
}

}  // namespace

extern "C" int pc_region_nan_census(const void* s2, int s2_u16, const float* s1, const float* s1_asc, int S, int C2, int C1, int h, int w,
                                    const int32_t* band_sel, const int32_t* boxes, int n, int rows_max, int64_t* counts, int max_blocks,
                                    void* stream) {
    RegionCensusArgs a{};
    if (rg_sources(a.src, s2, s2_u16, s1, s1_asc, nullptr, false, S, C2, C1, h, w, band_sel)) return PC_EINVAL;
    if (!boxes || !counts || n < 1 || rows_max < 1 || rows_max > h) return PC_EINVAL;
    if ((int64_t)n * 5 >= ((int64_t)1 << 31) || w >= (1 << 29)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(boxes) & 3) || (reinterpret_cast<uintptr_t>(counts) & 7)) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n3 = 3 * (int64_t)n;
    const int gi = (int)((n3 + 255) / 256 < 256 ? (n3 + 255) / 256 : 256);
    hipLaunchKernelGGL(region_census_init_kernel, dim3(gi), dim3(256), 0, st, reinterpret_cast<rr_u64*>(counts), n3);
    PC_CHECK_LAUNCH();
    a.boxes = boxes; a.S = S; a.n = n;
    a.nrb = (rows_max + CN_ROWS - 1) / CN_ROWS;
    a.items = (int64_t)n * a.nrb;
    a.counts = reinterpret_cast<rr_u64*>(counts);
    int64_t grid = max_blocks > 0 ? max_blocks : CN_MAX_BLOCKS;          // max_blocks: a smaller launch, for tests of the geometry
    if (grid > CN_MAX_BLOCKS) grid = CN_MAX_BLOCKS;
    if (grid > a.items) grid = a.items;
    if (s2_u16) hipLaunchKernelGGL(region_census_kernel<uint16_t>, dim3((int)grid), dim3(RR_THREADS), 0, st, a);
    else hipLaunchKernelGGL(region_census_kernel<float>, dim3((int)grid), dim3(RR_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    return 0;
}

namespace {
int rr_patch_args(RegionPatchArgs& a, const float* g2, const float* f2, const float* g1, const float* f1, const int32_t* data_hw, int B,
                  int Hm, int Wm, int nchunk) {
    if (!g2 || !f2 || !g1 || !f1 || !data_hw || B < 1 || B > 65535 || Hm < 1 || Wm < 1 || nchunk < 1) return PC_EINVAL;
    if (6 * (int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PC_EINVAL;       // idx is int32 in the item's own space
    if (nchunk != (int)((6 * (int64_t)Hm * Wm + PC_REGION_PATCH_CHUNK - 1) / PC_REGION_PATCH_CHUNK)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(g2) | reinterpret_cast<uintptr_t>(f2) | reinterpret_cast<uintptr_t>(g1) | reinterpret_cast<uintptr_t>(f1) |
         reinterpret_cast<uintptr_t>(data_hw)) & 3)
        return PC_EINVAL;
    a.g2 = reinterpret_cast<const int32_t*>(g2); a.f2 = reinterpret_cast<const int32_t*>(f2);
    a.g1 = reinterpret_cast<const int32_t*>(g1); a.f1 = reinterpret_cast<const int32_t*>(f1);
    a.data_hw = data_hw; a.B = B; a.Hm = Hm; a.Wm = Wm; a.nchunk = nchunk;
    return 0;
}
inline int rr_patch_grid(int nchunk, int B) {
    const int cap = 65535 / B > 1 ? 65535 / B : 1;                           // chunks beyond the cap are walked by the workgroups' own loop
    return nchunk < cap ? nchunk : cap;
}
}  // namespace

extern "C" int pc_region_patch_count(const float* g2, const float* f2, const float* g1, const float* f1, const int32_t* data_hw, int B, int Hm,
                                     int Wm, int32_t* counts, int nchunk, void* stream) {
    RegionPatchArgs a{};
    if (!counts || (reinterpret_cast<uintptr_t>(counts) & 3)) return PC_EINVAL;
    if (int rc = rr_patch_args(a, g2, f2, g1, f1, data_hw, B, Hm, Wm, nchunk)) return rc;
    a.counts = counts;
    hipLaunchKernelGGL(region_patch_kernel<false>, dim3(rr_patch_grid(nchunk, B), B), dim3(RR_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_region_patch_write(const float* g2, const float* f2, const float* g1, const float* f1, const int32_t* data_hw, int B, int Hm,
                                     int Wm, const int64_t* chunk_off, int nchunk, int32_t* idx, float* val, int64_t cap, void* stream) {
    RegionPatchArgs a{};
    if (!chunk_off || !idx || !val || cap < 1) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(chunk_off) & 7) || ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(val)) & 3)) return PC_EINVAL;
    if (int rc = rr_patch_args(a, g2, f2, g1, f1, data_hw, B, Hm, Wm, nchunk)) return rc;
    a.chunk_off = chunk_off; a.idx = idx; a.val = reinterpret_cast<int32_t*>(val); a.cap = cap;
    hipLaunchKernelGGL(region_patch_kernel<true>, dim3(rr_patch_grid(nchunk, B), B), dim3(RR_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_region_patch_apply(const int32_t* idx, const float* val, int64_t cap, const int64_t* off, const int32_t* count,
                                     const int32_t* item_hw, int B, float* s2, int64_t s2_stride, float* s1, int64_t s1_stride, int Hm, int Wm,
                                     int Ho, int Wo, int vflip, int hflip, int rot, int bright, float beta, int gam, float gamma,
                                     void* stream) {
    if (!idx || !val || !off || !count || !item_hw || !s2 || !s1 || B < 1 || Hm < 1 || Wm < 1 || rot < 0 || rot > 3 || cap < 0) return PC_EINVAL;
    if (Ho != ((rot & 1) ? Wm : Hm) || Wo != ((rot & 1) ? Hm : Wm)) return PC_EINVAL;
    if ((int64_t)Hm * Wm >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(val) | reinterpret_cast<uintptr_t>(s2) | reinterpret_cast<uintptr_t>(s1)) & 3)
        return PC_EINVAL;
    const int64_t oplane = (int64_t)Hm * Wm;
    if (s2_stride < 4 * oplane || s1_stride < 2 * oplane) return PC_EINVAL;
    // every item's range inside the table, its extent inside the tile and its index space inside int32: nothing is enqueued otherwise
    for (int b = 0; b < B; ++b) {
        const int hb = item_hw[2 * b], wb = item_hw[2 * b + 1];
        if (count[b] < 0 || off[b] < 0 || off[b] + count[b] > cap) return PC_EINVAL;
        if (count[b] > 0 && (hb < 1 || wb < 1 || hb > Hm || wb > Wm || 6 * (int64_t)hb * wb >= ((int64_t)1 << 31))) return PC_EINVAL;
    }
    RegionPatchApplyArgs a{};
    a.idx = idx; a.val = val; a.stride2 = s2_stride; a.stride1 = s1_stride; a.Hm = Hm; a.Wm = Wm; a.Ho = Ho; a.Wo = Wo;
    a.vflip = vflip != 0; a.hflip = hflip != 0; a.rot = rot; a.bright = bright != 0; a.gam = gam != 0; a.beta = beta; a.gamma = gamma;
    int b0 = 0;
    while (b0 < B) {
        // one launch: up to PC_REGION_GATHER_MAX_B items and fewer than 2^31 entries
        int nb = 0;
        int64_t total = 0;
        while (b0 + nb < B && nb < PC_REGION_GATHER_MAX_B && (nb == 0 || total + count[b0 + nb] < ((int64_t)1 << 31) - 1)) {
            RegionPatchItem& it = a.item[nb];
            it.off = off[b0 + nb]; it.start = (int32_t)total; it.hb = item_hw[2 * (b0 + nb)]; it.wb = item_hw[2 * (b0 + nb) + 1]; it._pad = 0;
            total += count[b0 + nb];
            ++nb;
        }
        if (total > 0) {
            a.s2 = s2 + (int64_t)b0 * s2_stride; a.s1 = s1 + (int64_t)b0 * s1_stride;
            a.nb = nb; a.total = (int)total;
            int64_t gx = (total + RR_THREADS - 1) / RR_THREADS;
            if (gx > PA_MAX_BLOCKS) gx = PA_MAX_BLOCKS;
            hipLaunchKernelGGL(region_patch_apply_kernel, dim3((int)gx), dim3(RR_THREADS), 0, (hipStream_t)stream, a);
            PC_CHECK_LAUNCH();
        }
        b0 += nb;
    }
    return 0;
}
