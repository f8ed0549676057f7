// units.hip -- multi-unit census supervision: every listed census unit of a crop in one training step.
//
// The reference supervises ONE census unit per sample (model/popcorn.py:184-190 the region sum, :361-377 the sparsity mask;
// data/PopulationDataset.py weaksup items): the U-Net runs over the unit's bounding box and only the unit's own pixels reach the head and
// the loss.  A multi-unit sample lists K units of the same crop; it is DEFINED as what the reference computes on the replicated batch
// (input[b], admin_mask[b], census_idx[b, k], y[b, k]) with the same two multinomial draws.  The per-pixel machinery of that, here:
//
//   pc_unit_mask      slot[b,y,x] = flat index of the listed unit that owns the pixel (binary search of the sample's sorted list), the
//                     union sparsity mask (popcorn.py:365-372 with region := "owned by a listed unit"), {Nsel, Nregion} with the batch-wide
//                     empty-selection fallback of :374-375, optionally the pixels per unit -- ONE launch (last-block ticket as
//                     mask.hip: score_mask_kernel)
//   pc_unit_popcount  popcount[n] = sum of popdense over slot == n: the N region sums of :186-188, bit-reproducible
//   pc_unit_paint     g_popdense[b,y,x] = g_popcount[slot] (0 for slot < 0): the autograd of those sums
// and, for the native step executor (step.hip: pc_train_step_units), what surrounds them without torch launches:
//   pc_unit_layout         the sorted, flattened unit lists from the caller's padded (B, K) batch -- rows sorted in LDS, the host's valid
//                          counts in the kernel arguments -- and the zeroed workspace of the sums: ONE launch
//   pc_unit_popcount_loss  the accumulate launch of pc_unit_popcount, then one block: finish, scatter to the caller's order, loss
// and, for steps that are replayed from a captured graph or run data parallel, the same two with N out of the host's hands:
//   pc_unit_layout_dev         pc_unit_layout with the counts in device memory; outputs of capacity B K, every element written
//   pc_unit_popcount_loss_dev  pc_unit_popcount_loss at that capacity; N and the (global) 1 / N read on the device
//
// Arithmetic of the sums.  A term q is split exactly into trunc(q) and its fraction; the integer parts and the fractions on a
// 2^-PC_CENSUS_FIX_SHIFT grid (census_table.hip's grid) are summed as two 64-bit integers per unit.  Integer addition is associative, so
// the sums hold the same bits for any batch position, grid size and arrival order although atomics are used (no floating-point atomics).
// With |q| < 2^32 and fewer than 2^27 pixels neither integer can wrap; a term that is NaN, +-Inf or >= 2^32 in magnitude makes ITS unit's
// popcount NaN (the trainer's loss guard then sees it), never a wrapped number.  Sums stay on chip in two stages: a lane carries the running
// sums of the unit it is in (units are runs along a row and recur a few rows down) and hands them on when the unit changes; while the
// sample's K fits, the hand-ons go to bins in LDS and the workgroup issues one global 64-bit add per unit and accumulator it touched.
// No loop's trip count depends on another lane's, wave's or workgroup's progress: no retry, no spin wait.
#include "common.h"

namespace {

constexpr int UN_THREADS = 256;
constexpr int UN_LDS_IDS = 1024;         // unit ids of a sample held in LDS for the search (4 KB); longer lists are searched in global memory
constexpr int UN_LDS_BINS = 256;         // units of a sample with bins in LDS (popcount: 5 KB, pixel counts: 1 KB); more add to global memory directly
constexpr int UN_MAX_BLOCKS = 512;       // workgroups of a launch: two per CU
constexpr int UN_PX_PER_BLOCK = 4096;    // popcount: pixels a workgroup walks before it hands its bins on

typedef unsigned long long un_u64;

// index in [0, n) of the entry equal to v in the ascending list id_at(0 .. n), or -1.  The compare is the existing kernels'
// admin == (float)id; a NaN v compares false everywhere and finds nothing.
template <typename IdAt>
__device__ __forceinline__ int un_find(float v, int n, IdAt id_at) {
    int l = 0, h = n;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (id_at(m) < v) l = m + 1; else h = m;
    }
    return (l < n && id_at(l) == v) ? l : -1;
}

struct UnitMaskArgs {
    const float* building; const float* admin; const int64_t* units; const int32_t* unit_off;
    const uint8_t* rowsel; const uint8_t* colsel;
    int occ;
    int32_t* slot; uint8_t* mask; int32_t* counts; int32_t* unit_pixels;
    unsigned* scratch;              // {nsel | nregion << 32} as one 64-bit word, then the ticket: zero between launches
    int B, H, W;
};

__global__ __launch_bounds__(UN_THREADS) void unit_mask_kernel(const UnitMaskArgs a) {
    __shared__ float ids[UN_LDS_IDS];
    __shared__ int pix[UN_LDS_BINS];
    __shared__ int red[2][UN_THREADS / 64];
    __shared__ unsigned last;
    __shared__ un_u64 tot_sh;
    const int t = threadIdx.x, b = blockIdx.y;
    const int HW = a.H * a.W;
    const int u0 = a.unit_off[b], K = a.unit_off[b + 1] - u0;
    const bool ids_lds = K <= UN_LDS_IDS, pix_lds = a.unit_pixels != nullptr && K <= UN_LDS_BINS;
    if (ids_lds)
        for (int i = t; i < K; i += UN_THREADS) ids[i] = (float)a.units[u0 + i];
    if (pix_lds)
        for (int i = t; i < K; i += UN_THREADS) pix[i] = 0;
    __syncthreads();
    // neighbouring pixels mostly belong to one unit: the last (id, slot) pair answers without a search
    float seen = __builtin_nanf("");
    int seen_slot = -1;
    auto lookup = [&](float v) -> int {
        if (v == seen) return seen_slot;
        const int r = ids_lds ? un_find(v, K, [&](int j) { return ids[j]; })
                              : un_find(v, K, [&](int j) { return (float)a.units[u0 + j]; });
        seen = v;
        seen_slot = r < 0 ? -1 : u0 + r;
        return seen_slot;
    };
    // pixels per unit: exact integer atomics, one per run of a unit along this lane's pixels
    int run_slot = -1, run_n = 0;
    auto count = [&](int s) {
        if (s == run_slot) { ++run_n; return; }
        if (run_slot >= 0) {
            if (pix_lds) atomicAdd(&pix[run_slot - u0], run_n);
            else atomicAdd(&a.unit_pixels[run_slot], run_n);
        }
        run_slot = s; run_n = 1;
    };
    const float* adm_b = a.admin + (int64_t)b * HW;
    const float* bld_b = a.building + (int64_t)b * HW;
    int32_t* slot_b = a.slot + (int64_t)b * HW;
    uint8_t* mask_b = a.mask + (int64_t)b * HW;
    int nsel = 0, nreg = 0;
    const bool vec4 = (a.W & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.admin) | reinterpret_cast<uintptr_t>(a.building) |
                                          reinterpret_cast<uintptr_t>(a.slot)) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.mask) & 3) == 0;
    if (vec4) {
        // four consecutive pixels of a row per thread: 16-byte accesses
        const int n4 = HW >> 2, w4 = a.W >> 2;
        for (int i4 = blockIdx.x * UN_THREADS + t; i4 < n4; i4 += gridDim.x * UN_THREADS) {
            const int y = i4 / w4, x = (i4 - y * w4) * 4;
            const f32x4 adm = pc_ld4(adm_b + 4 * (int64_t)i4);
            const f32x4 bld = pc_ld4(bld_b + 4 * (int64_t)i4);
            const bool rs = a.rowsel[y] != 0;
            int4 sv;
            int* sp = reinterpret_cast<int*>(&sv);
            unsigned mbits = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int s = lookup(adm[e]);
                const bool region = s >= 0;
                const bool base = a.occ ? (bld[e] > 0.f) : true;
                const bool m = region && (base || (rs && a.colsel[x + e]));
                sp[e] = s;
                mbits |= (m ? 1u : 0u) << (8 * e);
                nsel += m;
                nreg += region;
                if (a.unit_pixels) count(s);
            }
            *reinterpret_cast<int4*>(slot_b + 4 * (int64_t)i4) = sv;
            *reinterpret_cast<unsigned*>(mask_b + 4 * (int64_t)i4) = mbits;
        }
    } else {
        for (int i = blockIdx.x * UN_THREADS + t; i < HW; i += gridDim.x * UN_THREADS) {
            const int y = i / a.W, x = i - y * a.W;
            const int s = lookup(adm_b[i]);
            const bool region = s >= 0;
            const bool base = a.occ ? (bld_b[i] > 0.f) : true;
            const bool m = region && (base || (a.rowsel[y] && a.colsel[x]));
            slot_b[i] = s;
            mask_b[i] = m ? 1 : 0;
            nsel += m;
            nreg += region;
            if (a.unit_pixels) count(s);
        }
    }
    if (a.unit_pixels) {
        count(-1);                 // hands the last run on
        if (pix_lds) {
            __syncthreads();
            for (int i = t; i < K; i += UN_THREADS)
                if (pix[i]) atomicAdd(&a.unit_pixels[u0 + i], pix[i]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) { nsel += __shfl_down(nsel, off); nreg += __shfl_down(nreg, off); }
    if ((t & 63) == 0) { red[0][t >> 6] = nsel; red[1][t >> 6] = nreg; }
    __syncthreads();
    if (t == 0) {
        int s0 = 0, s1 = 0;
#pragma unroll
        for (int w = 0; w < UN_THREADS / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
        // integer counts: order-independent, exact.  One 64-bit atomic per block carries both; the ticket follows it behind a fence, so the
        // block that draws the last ticket reads complete totals (with an atomic: the word lives on the memory side)
        un_u64* acc = reinterpret_cast<un_u64*>(a.scratch);
        atomicAdd(acc, (un_u64)(unsigned)s0 | ((un_u64)(unsigned)s1 << 32));
        __threadfence();
        const unsigned ticket = atomicAdd(a.scratch + 2, 1u);
        last = ticket == gridDim.x * gridDim.y - 1 ? 1u : 0u;
        if (last) {
            __threadfence();
            tot_sh = atomicAdd(acc, 0ull);
        }
    }
    __syncthreads();
    if (!last) return;
    const unsigned tot_sel = (unsigned)(tot_sh & 0xffffffffull), tot_reg = (unsigned)(tot_sh >> 32);
    if (tot_sel == 0) {
        // an empty selection falls back to the region mask (popcorn.py:374-375), batch-wide.  Rare; this one block redoes the search from
        // the inputs (it reads nothing another block wrote)
        const int n = a.B * HW;
        for (int i = t; i < n; i += UN_THREADS) {
            const int bb = i / HW;
            const int v0 = a.unit_off[bb], kk = a.unit_off[bb + 1] - v0;
            a.mask[i] = un_find(a.admin[i], kk, [&](int j) { return (float)a.units[v0 + j]; }) >= 0 ? 1 : 0;
        }
    }
    if (t == 0) {
        a.counts[0] = (int32_t)(tot_sel ? tot_sel : tot_reg);
        a.counts[1] = (int32_t)tot_reg;
        // this block is the last one alive: leave the accumulator and the ticket at zero for the next call (ordered behind this kernel
        // on the stream), instead of a zeroing launch in front of every call
        a.scratch[0] = 0u; a.scratch[1] = 0u; a.scratch[2] = 0u;
        __threadfence();
    }
}

__global__ __launch_bounds__(256) void unit_zero_words_kernel(uint32_t* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}

// ---- segmented population sum -------------------------------------------------------------------------------------------------------
struct UnitSumArgs {
    const float* popdense; const int32_t* slot; const int32_t* unit_off;
    un_u64* acc_int; un_u64* acc_frac; int32_t* bad;          // [N] each, zero before the launch (two's complement sums)
    int HW, N, chunks;
};

__global__ __launch_bounds__(UN_THREADS) void unit_popcount_kernel(const UnitSumArgs a) {
    __shared__ un_u64 bin_int[UN_LDS_BINS], bin_frac[UN_LDS_BINS];
    __shared__ int bin_bad[UN_LDS_BINS];
    const int t = threadIdx.x, b = blockIdx.y;
    const int u0 = a.unit_off ? a.unit_off[b] : 0, K = a.unit_off ? a.unit_off[b + 1] - u0 : 0;
    const bool lds = a.unit_off != nullptr && K >= 1 && K <= UN_LDS_BINS;
    if (lds)
        for (int i = t; i < K; i += UN_THREADS) { bin_int[i] = 0; bin_frac[i] = 0; bin_bad[i] = 0; }
    __syncthreads();
    const float* pd_b = a.popdense + (int64_t)b * a.HW;
    const int32_t* slot_b = a.slot + (int64_t)b * a.HW;
    // the running sums of the unit this lane is in
    int cur = -1;
    long long run_int = 0, run_frac = 0;
    bool run_bad = false;
    auto hand_on = [&]() {
        if ((unsigned)cur < (unsigned)a.N) {
            if (lds && cur >= u0 && cur < u0 + K) {
                if (run_int) atomicAdd(&bin_int[cur - u0], (un_u64)run_int);
                if (run_frac) atomicAdd(&bin_frac[cur - u0], (un_u64)run_frac);
                if (run_bad) bin_bad[cur - u0] = 1;
            } else {
                if (run_int) atomicAdd(&a.acc_int[cur], (un_u64)run_int);
                if (run_frac) atomicAdd(&a.acc_frac[cur], (un_u64)run_frac);
                if (run_bad) atomicOr(&a.bad[cur], 1);
            }
        }
        run_int = 0; run_frac = 0; run_bad = false;
    };
    auto term = [&](int s, float q) {
        if (s != cur) { hand_on(); cur = s; }
        if (s < 0) return;
        // trunc(q) and q - trunc(q) are exact in fp32, so is the scaling of the fraction by 2^30: the only rounding is rintf's, to the grid
        const bool in = fabsf(q) < 4294967296.f;          // false for NaN and +-Inf
        if (in) {
            const float hi = truncf(q);
            run_int += (long long)hi;
            run_frac += (long long)rintf((q - hi) * 1073741824.f);
        } else run_bad = true;
    };
    const bool vec4 = (a.HW & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.popdense) | reinterpret_cast<uintptr_t>(a.slot)) & 15) == 0;
    for (int c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        const int p0 = c * UN_PX_PER_BLOCK, p1 = min(p0 + UN_PX_PER_BLOCK, a.HW);
        if (vec4) {
            for (int i = p0 + 4 * t; i < p1; i += 4 * UN_THREADS) {
                const f32x4 q = pc_ld4(pd_b + i);
                const int4 s = *reinterpret_cast<const int4*>(slot_b + i);
                term(s.x, q[0]); term(s.y, q[1]); term(s.z, q[2]); term(s.w, q[3]);
            }
        } else {
            for (int i = p0 + t; i < p1; i += UN_THREADS) term(slot_b[i], pd_b[i]);
        }
    }
    hand_on();
    if (!lds) return;
    __syncthreads();
    // one global add per unit and accumulator this workgroup touched
    for (int i = t; i < K; i += UN_THREADS) {
        if (bin_int[i]) atomicAdd(&a.acc_int[u0 + i], bin_int[i]);
        if (bin_frac[i]) atomicAdd(&a.acc_frac[u0 + i], bin_frac[i]);
        if (bin_bad[i]) atomicOr(&a.bad[u0 + i], 1);
    }
}
static_assert(PC_CENSUS_FIX_SHIFT == 30, "unit_popcount_kernel scales the fraction by 2^30");
static_assert(UN_PX_PER_BLOCK % (4 * UN_THREADS) == 0, "a chunk is whole rounds of four pixels per lane");

// popcount = int + frac * 2^-30: both conversions are exact below 2^53 and the sum rounds once; then once more to fp32
__device__ __forceinline__ float un_finish(long long acc_int, long long acc_frac, int32_t bad) {
    const double s = (double)acc_int + (double)acc_frac * (1.0 / 1073741824.0);
    return bad ? __builtin_nanf("") : (float)s;
}

__global__ __launch_bounds__(256) void unit_popcount_finish_kernel(const long long* __restrict__ acc_int, const long long* __restrict__ acc_frac,
                                                                   const int32_t* __restrict__ bad, float* __restrict__ popcount, int N) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) popcount[i] = un_finish(acc_int[i], acc_frac[i], bad[i]);
}

// pc_unit_popcount_loss's second launch, ONE block (the pattern of head.hip: head_popcount_loss_kernel): the finish above for all N units,
// the same value scattered to the caller's (b, k) order, then the loss block over the N pairs.  Thread t finishes and reads back the units
// t, t + 256, ...: pc_loss_block walks them with the same stride.
__global__ __launch_bounds__(256) void unit_finish_loss_kernel(const long long* __restrict__ acc_int, const long long* __restrict__ acc_frac,
                                                               const int32_t* __restrict__ bad, const int32_t* __restrict__ dest,
                                                               float* popcount, float* __restrict__ popcount_caller, const double* stats,
                                                               const pc_loss_args a) {
    __shared__ double red[256];
    const int N = a.B;
    for (int i = threadIdx.x; i < N; i += 256) {
        const float v = un_finish(acc_int[i], acc_frac[i], bad[i]);
        popcount[i] = v;
        if (popcount_caller) {
            const int d = dest[i];
            if ((unsigned)d < (unsigned)N) popcount_caller[d] = v;
        }
    }
    __syncthreads();
    pc_loss_block(a, popcount, stats, red);
}

// ---- the flattened lists from the padded batch ------------------------------------------------------------------------------------------
constexpr int UL_MAX_K = PC_UNIT_LAYOUT_MAX_K;
constexpr int UL_MAX_B = PC_UNIT_LAYOUT_MAX_B;
static_assert(UL_MAX_K <= UN_LDS_IDS, "a row that pc_unit_layout sorts fits the LDS id list of unit_mask_kernel");
static_assert(UL_MAX_K < 65536, "a count fits 16 bits");

struct UnitLayoutArgs {
    const int64_t* census_idx; const float* y;
    int64_t* units; int32_t* unit_off; float* y_sorted; int32_t* dest;
    un_u64* acc_int; un_u64* acc_frac; int32_t* bad;          // the population sum's workspace (NULL: not zeroed)
    int B, K, P, N;                                              // P: K rounded up to a power of two
    uint16_t n[UL_MAX_B];                                        // the host's valid counts: 512 bytes of kernel arguments
};

// (key, tag) pairs in ascending order; tag = the slot k of a valid entry, 65536 + k of a padding entry, so that the order is total and a
// valid INT64_MAX still sorts in front of the padding
__device__ __forceinline__ bool ul_less(long long ka, int ta, long long kb, int tb) { return ka != kb ? ka < kb : ta < tb; }

__global__ __launch_bounds__(UN_THREADS) void unit_layout_kernel(const UnitLayoutArgs a) {
    __shared__ long long key[UL_MAX_K];
    __shared__ int tag[UL_MAX_K];
    const int t = threadIdx.x, b = blockIdx.x;
    const int nb = a.n[b];
    int off = 0;
    for (int i = 0; i < b; ++i) off += a.n[i];
    const int64_t* row = a.census_idx + (int64_t)b * a.K;
    for (int i = t; i < a.P; i += UN_THREADS) {
        const bool valid = i < nb;                                // nb <= K (checked by the host)
        key[i] = valid ? (long long)row[i] : 0x7fffffffffffffffll;
        tag[i] = valid ? i : 65536 + i;
    }
    __syncthreads();
    // bitonic network: log2(P) (log2(P) + 1) / 2 rounds of P / 2 disjoint compare-exchanges, a barrier between rounds
    for (int k = 2; k <= a.P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < a.P; i += UN_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const long long ki = key[i], kp = key[p];
                    const int ti = tag[i], tp = tag[p];
                    const bool up = (i & k) == 0;
                    if (up ? ul_less(kp, tp, ki, ti) : ul_less(ki, ti, kp, tp)) { key[i] = kp; key[p] = ki; tag[i] = tp; tag[p] = ti; }
                }
            }
            __syncthreads();
        }
    if (t == 0) {
        a.unit_off[b] = off;
        if (b == a.B - 1) a.unit_off[a.B] = off + nb;
    }
    // the nb valid entries sort in front of the padding: sorted slot j < nb holds the caller's slot tag[j] < nb.  off + nb <= N (host)
    for (int j = t; j < nb; j += UN_THREADS) {
        const int n = off + j;
        int src = tag[j] & 65535;
        if (src >= nb) src = j;                                   // (cannot happen; keeps every index in the row whatever the sort did)
        a.units[n] = key[j];
        a.y_sorted[n] = a.y[(int64_t)b * a.K + src];
        a.dest[n] = off + src;
        if (a.acc_int) { a.acc_int[n] = 0; a.acc_frac[n] = 0; a.bad[n] = 0; }
    }
}

// ---- the device-N forms: the valid counts, N and 1 / N come from device memory, every launch runs at the capacity Ncap = B * K ---------------
// A captured step replays its kernel arguments, and a data-parallel rank knows only its own N: neither can carry N in a launch.  Here the
// launches are shaped by (B, K) alone; what depends on the counts is read from memory that the loader (census_n) or the stats all-reduce
// (the global N in stats[2]) rewrites between replays.
struct UnitLayoutDevArgs {
    const int64_t* census_idx; const float* y; const int32_t* census_n;      // census_n: DEVICE int32 [B]
    int64_t* units; int32_t* unit_off; float* y_sorted; int32_t* dest;      // capacity Ncap each (unit_off: B + 1)
    un_u64* acc_int; un_u64* acc_frac; int32_t* bad;                         // the population sum's workspace laid out by Ncap (NULL: not zeroed)
    int32_t* n_dev; double* stats;                                           // N as int32; N as a double in stats[2] (NULL: not written)
    int B, K, P;                                                             // P: K rounded up to a power of two
};

// unit_layout_kernel with the counts read from memory.  Workgroup b writes exactly K elements of every capacity-sized output: its nb valid
// entries at [off, off + nb) and K - nb tail entries at N + (b K - off) + ..., the paddings of the rows in front of it -- together the B
// workgroups cover [0, Ncap) once, whatever the counts are.  Every trip count is fixed by (B, K).
__global__ __launch_bounds__(UN_THREADS) void unit_layout_dev_kernel(const UnitLayoutDevArgs a) {
    __shared__ long long key[UL_MAX_K];
    __shared__ int tag[UL_MAX_K];
    __shared__ int cnt[UL_MAX_B];
    const int t = threadIdx.x, b = blockIdx.x;
    // the device cannot raise: a count outside [1, K] is clamped into it
    for (int i = t; i < a.B; i += UN_THREADS) cnt[i] = min(max(a.census_n[i], 1), a.K);
    __syncthreads();
    int off = 0, N = 0;
    for (int i = 0; i < a.B; ++i) {
        const int c = cnt[i];                                     // (an LDS broadcast)
        if (i < b) off += c;
        N += c;
    }
    const int nb = cnt[b];
    const int64_t* row = a.census_idx + (int64_t)b * a.K;
    for (int i = t; i < a.P; i += UN_THREADS) {
        const bool valid = i < nb;
        key[i] = valid ? (long long)row[i] : 0x7fffffffffffffffll;
        tag[i] = valid ? i : 65536 + i;
    }
    __syncthreads();
    for (int k = 2; k <= a.P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < a.P; i += UN_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const long long ki = key[i], kp = key[p];
                    const int ti = tag[i], tp = tag[p];
                    const bool up = (i & k) == 0;
                    if (up ? ul_less(kp, tp, ki, ti) : ul_less(ki, ti, kp, tp)) { key[i] = kp; key[p] = ki; tag[i] = tp; tag[p] = ti; }
                }
            }
            __syncthreads();
        }
    if (t == 0) {
        a.unit_off[b] = off;
        if (b == a.B - 1) a.unit_off[a.B] = N;
        if (b == 0) {
            *a.n_dev = N;
            if (a.stats) a.stats[2] = (double)N;
        }
    }
    const int tail0 = N + b * a.K - off;                          // N + the paddings of rows 0 .. b - 1; tail0 + (K - nb) <= B K
    for (int j = t; j < a.K; j += UN_THREADS) {
        int n;
        if (j < nb) {
            n = off + j;
            int src = tag[j] & 65535;
            if (src >= nb) src = j;                               // (cannot happen; keeps every index in the row whatever the sort did)
            a.units[n] = key[j];
            a.y_sorted[n] = a.y[(int64_t)b * a.K + src];
            a.dest[n] = off + src;
        } else {
            n = tail0 + (j - nb);
            a.units[n] = 0x7fffffffffffffffll;
            a.y_sorted[n] = 0.f;
            a.dest[n] = -1;
        }
        if (a.acc_int) { a.acc_int[n] = 0; a.acc_frac[n] = 0; a.bad[n] = 0; }
    }
}

// unit_finish_loss_kernel at capacity: N_local from n_dev, N_global from stats[2] (the local N, or its sum over the ranks after the stats
// all-reduce: an exact integer in a double), inv_N = (float)(1.0 / N_global) -- the host's expression in pc_unit_popcount_loss, so one
// process gets that entry's bits.  Tails [N_local, Ncap) of both popcount orders and of g_popcount := 0.
__global__ __launch_bounds__(256) void unit_finish_loss_dev_kernel(const long long* __restrict__ acc_int, const long long* __restrict__ acc_frac,
                                                                   const int32_t* __restrict__ bad, const int32_t* __restrict__ dest,
                                                                   const int32_t* __restrict__ n_dev, float* popcount,
                                                                   float* __restrict__ popcount_caller, const double* stats,
                                                                   const pc_loss_args a) {
    __shared__ double red[256];
    const int Ncap = a.B;
    const int N = min(max(*n_dev, 1), Ncap);
    double Ng = stats[2];
    if (!(Ng >= 1.0)) Ng = (double)N;                             // (never written / NaN: the local count; the device cannot raise)
    for (int i = threadIdx.x; i < Ncap; i += 256) {
        if (i < N) {
            const float v = un_finish(acc_int[i], acc_frac[i], bad[i]);
            popcount[i] = v;
            if (popcount_caller) {
                const int d = dest[i];
                if ((unsigned)d < (unsigned)N) popcount_caller[d] = v;
            }
        } else {
            popcount[i] = 0.f;
            if (popcount_caller) popcount_caller[i] = 0.f;
            a.g_popcount[i] = 0.f;
        }
    }
    __syncthreads();
    pc_loss_args l = a;
    l.B = N;
    l.inv_B = (float)(1.0 / Ng);
    pc_loss_block(l, popcount, stats, red);
}

// ---- gradient paint ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float un_pick(const float* g, int s, int N) { return (unsigned)s < (unsigned)N ? g[s] : 0.f; }

__global__ __launch_bounds__(256) void unit_paint_kernel(const float* __restrict__ g_popcount, const int32_t* __restrict__ slot,
                                                         float* __restrict__ out, int64_t n, int N, int vec) {
    const int64_t n4 = vec ? (n >> 2) : 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int4 s = *reinterpret_cast<const int4*>(slot + 4 * i);
        pc_st4(out + 4 * i, f32x4{un_pick(g_popcount, s.x, N), un_pick(g_popcount, s.y, N), un_pick(g_popcount, s.z, N),
                                  un_pick(g_popcount, s.w, N)});
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = un_pick(g_popcount, slot[i], N);
}

inline int64_t un_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int64_t pc_unit_ws_bytes(int64_t N) { return N < 1 ? 16 : un_align16(20 * N); }

extern "C" int pc_unit_mask(const float* building, const float* admin_mask, const int64_t* units, const int32_t* unit_off,
                            const uint8_t* rowsel, const uint8_t* colsel, int occupancymodel, int32_t* slot, uint8_t* mask,
                            int32_t* counts, int32_t* unit_pixels, int B, int H, int W, int N, void* stream) {
    if (!building || !admin_mask || !units || !unit_off || !rowsel || !colsel || !slot || !mask || !counts) return PC_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || N < 1 || (int64_t)B * H * W >= ((int64_t)1 << 31)) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(admin_mask) | reinterpret_cast<uintptr_t>(building)) & 3) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    // {counts, ticket} of the launch in flight: library-owned, per device, zero between calls (the kernel's last block resets it)
    static unsigned* scratch[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    dev &= 63;
    if (!scratch[dev]) {
        unsigned* p = nullptr;
        hipError_t e = hipMalloc(&p, 4 * sizeof(unsigned));
        if (e != hipSuccess) return (int)e;
        e = hipMemset(p, 0, 4 * sizeof(unsigned));
        if (e != hipSuccess) return (int)e;
        e = hipDeviceSynchronize();            // the first kernel may run on a non-blocking stream
        if (e != hipSuccess) return (int)e;
        scratch[dev] = p;
    }
    if (unit_pixels) {
        hipLaunchKernelGGL(unit_zero_words_kernel, dim3((N + 255) / 256 < 64 ? (N + 255) / 256 : 64), dim3(256), 0, st,
                           reinterpret_cast<uint32_t*>(unit_pixels), (int64_t)N);
        PC_CHECK_LAUNCH();
    }
    UnitMaskArgs a{};
    a.building = building; a.admin = admin_mask; a.units = units; a.unit_off = unit_off; a.rowsel = rowsel; a.colsel = colsel;
    a.occ = occupancymodel; a.slot = slot; a.mask = mask; a.counts = counts; a.unit_pixels = unit_pixels; a.scratch = scratch[dev];
    a.B = B; a.H = H; a.W = W;
    const int items = (W & 3) == 0 ? H * W / 4 : H * W;
    int gx = (items + UN_THREADS - 1) / UN_THREADS;
    const int cap = UN_MAX_BLOCKS / B > 1 ? UN_MAX_BLOCKS / B : 1;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL(unit_mask_kernel, dim3(gx, B), dim3(UN_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_popcount(const float* popdense, const int32_t* slot, const int32_t* unit_off, float* popcount, void* ws,
                                int B, int H, int W, int N, void* stream) {
    if (!popdense || !slot || !popcount || !ws) return PC_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || N < 1 || (int64_t)H * W >= ((int64_t)1 << 27)) return PC_EINVAL;      // a unit's integer sums cannot wrap
    if ((reinterpret_cast<uintptr_t>(ws) & 15) || ((reinterpret_cast<uintptr_t>(popdense) | reinterpret_cast<uintptr_t>(slot)) & 3)) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    UnitSumArgs a{};
    a.popdense = popdense; a.slot = slot; a.unit_off = unit_off;
    a.acc_int = reinterpret_cast<un_u64*>(ws);
    a.acc_frac = a.acc_int + N;
    a.bad = reinterpret_cast<int32_t*>(a.acc_frac + N);
    a.HW = H * W; a.N = N;
    a.chunks = (a.HW + UN_PX_PER_BLOCK - 1) / UN_PX_PER_BLOCK;
    const int64_t words = 5 * (int64_t)N;
    hipLaunchKernelGGL(unit_zero_words_kernel, dim3((int)((words + 255) / 256 < 64 ? (words + 255) / 256 : 64)), dim3(256), 0, st,
                       reinterpret_cast<uint32_t*>(ws), words);
    PC_CHECK_LAUNCH();
    const int cap = 4 * UN_MAX_BLOCKS / B > 1 ? 4 * UN_MAX_BLOCKS / B : 1;
    hipLaunchKernelGGL(unit_popcount_kernel, dim3(a.chunks < cap ? a.chunks : cap, B), dim3(UN_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    hipLaunchKernelGGL(unit_popcount_finish_kernel, dim3((N + 255) / 256 < 64 ? (N + 255) / 256 : 64), dim3(256), 0, st,
                       reinterpret_cast<const long long*>(a.acc_int), reinterpret_cast<const long long*>(a.acc_frac), a.bad, popcount, N);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_paint(const float* g_popcount, const int32_t* slot, float* g_popdense, int64_t n, int N, void* stream) {
    if (!g_popcount || !slot || !g_popdense || n < 0 || N < 1) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(g_popdense)) & 3) return PC_EINVAL;
    if (n == 0) return 0;
    const int vec = ((reinterpret_cast<uintptr_t>(slot) | reinterpret_cast<uintptr_t>(g_popdense)) & 15) == 0;
    int64_t g = ((vec ? n / 4 : n) + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    hipLaunchKernelGGL(unit_paint_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, g_popcount, slot, g_popdense, n, N, vec);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_layout(const int64_t* census_idx, const float* y, const int32_t* census_n, int B, int K, int64_t* units,
                              int32_t* unit_off, float* y_sorted, int32_t* dest, void* ws, void* stream) {
    if (!census_idx || !y || !census_n || !units || !unit_off || !y_sorted || !dest || B < 1 || K < 1) return PC_EINVAL;
    if (K > UL_MAX_K || B > UL_MAX_B) return PC_ENOTSUP;
    if ((reinterpret_cast<uintptr_t>(census_idx) | reinterpret_cast<uintptr_t>(units)) & 7) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y_sorted) | reinterpret_cast<uintptr_t>(unit_off) |
         reinterpret_cast<uintptr_t>(dest)) & 3)
        return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return PC_EINVAL;
    UnitLayoutArgs a{};
    int N = 0;
    for (int b = 0; b < B; ++b) {
        if (census_n[b] < 1 || census_n[b] > K) return PC_EINVAL;
        a.n[b] = (uint16_t)census_n[b];
        N += census_n[b];
    }
    a.census_idx = census_idx; a.y = y; a.units = units; a.unit_off = unit_off; a.y_sorted = y_sorted; a.dest = dest;
    if (ws) {
        a.acc_int = reinterpret_cast<un_u64*>(ws);
        a.acc_frac = a.acc_int + N;
        a.bad = reinterpret_cast<int32_t*>(a.acc_frac + N);
    }
    a.B = B; a.K = K; a.N = N;
    a.P = 1;
    while (a.P < K) a.P <<= 1;
    hipLaunchKernelGGL(unit_layout_kernel, dim3(B), dim3(UN_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_layout_dev(const int64_t* census_idx, const float* y, const int32_t* census_n_dev, int B, int K, int64_t* units,
                                  int32_t* unit_off, float* y_sorted, int32_t* dest, void* ws, int32_t* n_dev, double* stats, void* stream) {
    if (!census_idx || !y || !census_n_dev || !units || !unit_off || !y_sorted || !dest || !n_dev || B < 1 || K < 1) return PC_EINVAL;
    if (K > UL_MAX_K || B > UL_MAX_B) return PC_ENOTSUP;
    if ((reinterpret_cast<uintptr_t>(census_idx) | reinterpret_cast<uintptr_t>(units) | reinterpret_cast<uintptr_t>(stats)) & 7) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y_sorted) | reinterpret_cast<uintptr_t>(unit_off) |
         reinterpret_cast<uintptr_t>(dest) | reinterpret_cast<uintptr_t>(census_n_dev) | reinterpret_cast<uintptr_t>(n_dev)) & 3)
        return PC_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return PC_EINVAL;
    UnitLayoutDevArgs a{};
    const int64_t Ncap = (int64_t)B * K;
    a.census_idx = census_idx; a.y = y; a.census_n = census_n_dev;
    a.units = units; a.unit_off = unit_off; a.y_sorted = y_sorted; a.dest = dest; a.n_dev = n_dev; a.stats = stats;
    if (ws) {
        a.acc_int = reinterpret_cast<un_u64*>(ws);
        a.acc_frac = a.acc_int + Ncap;
        a.bad = reinterpret_cast<int32_t*>(a.acc_frac + Ncap);
    }
    a.B = B; a.K = K;
    a.P = 1;
    while (a.P < K) a.P <<= 1;
    hipLaunchKernelGGL(unit_layout_dev_kernel, dim3(B), dim3(UN_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_popcount_loss_dev(const float* popdense, const int32_t* slot, const int32_t* unit_off, const int32_t* dest,
                                         const float* y_sorted, void* ws, const int32_t* n_dev, float* popcount_sorted,
                                         float* popcount_caller, const double* stats, const float* lam4, float scale_regularization,
                                         float lam_weak, int B, int H, int W, int Ncap, float* loss_out, float* g_popcount,
                                         float* g_scale_const, void* stream) {
    if (!popdense || !slot || !y_sorted || !ws || !n_dev || !popcount_sorted || !stats || !lam4 || !loss_out || !g_popcount || !g_scale_const)
        return PC_EINVAL;
    if (popcount_caller && !dest) return PC_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || Ncap < 1 || (int64_t)H * W >= ((int64_t)1 << 27)) return PC_EINVAL;   // as pc_unit_popcount
    if ((reinterpret_cast<uintptr_t>(ws) & 15) || ((reinterpret_cast<uintptr_t>(popdense) | reinterpret_cast<uintptr_t>(slot) |
                                                    reinterpret_cast<uintptr_t>(n_dev)) & 3) || (reinterpret_cast<uintptr_t>(stats) & 7))
        return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    UnitSumArgs a{};
    a.popdense = popdense; a.slot = slot; a.unit_off = unit_off;
    a.acc_int = reinterpret_cast<un_u64*>(ws);
    a.acc_frac = a.acc_int + Ncap;
    a.bad = reinterpret_cast<int32_t*>(a.acc_frac + Ncap);
    a.HW = H * W; a.N = Ncap;
    a.chunks = (a.HW + UN_PX_PER_BLOCK - 1) / UN_PX_PER_BLOCK;
    const int cap = 4 * UN_MAX_BLOCKS / B > 1 ? 4 * UN_MAX_BLOCKS / B : 1;
    hipLaunchKernelGGL(unit_popcount_kernel, dim3(a.chunks < cap ? a.chunks : cap, B), dim3(UN_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    pc_loss_args l{};
    l.y = y_sorted;
    for (int i = 0; i < 4; ++i) l.lam[i] = lam4[i];
    l.sreg = scale_regularization; l.lam_weak = lam_weak; l.B = Ncap;     // (the capacity; N and inv_B are read on the device)
    l.loss_out = loss_out; l.g_popcount = g_popcount; l.g_scale_const = g_scale_const;
    hipLaunchKernelGGL(unit_finish_loss_dev_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const long long*>(a.acc_int),
                       reinterpret_cast<const long long*>(a.acc_frac), a.bad, dest, n_dev, popcount_sorted, popcount_caller, stats, l);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_unit_popcount_loss(const float* popdense, const int32_t* slot, const int32_t* unit_off, const int32_t* dest,
                                     const float* y_sorted, void* ws, float* popcount_sorted, float* popcount_caller, const double* stats,
                                     const float* lam4, float scale_regularization, float lam_weak, int B, int H, int W, int N,
                                     float* loss_out, float* g_popcount, float* g_scale_const, void* stream) {
    if (!popdense || !slot || !y_sorted || !ws || !popcount_sorted || !lam4 || !loss_out || !g_popcount || !g_scale_const) return PC_EINVAL;
    if (popcount_caller && !dest) return PC_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || N < 1 || (int64_t)H * W >= ((int64_t)1 << 27)) return PC_EINVAL;      // as pc_unit_popcount
    if ((reinterpret_cast<uintptr_t>(ws) & 15) || ((reinterpret_cast<uintptr_t>(popdense) | reinterpret_cast<uintptr_t>(slot)) & 3)) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    UnitSumArgs a{};
    a.popdense = popdense; a.slot = slot; a.unit_off = unit_off;
    a.acc_int = reinterpret_cast<un_u64*>(ws);
    a.acc_frac = a.acc_int + N;
    a.bad = reinterpret_cast<int32_t*>(a.acc_frac + N);
    a.HW = H * W; a.N = N;
    a.chunks = (a.HW + UN_PX_PER_BLOCK - 1) / UN_PX_PER_BLOCK;
    const int cap = 4 * UN_MAX_BLOCKS / B > 1 ? 4 * UN_MAX_BLOCKS / B : 1;
    hipLaunchKernelGGL(unit_popcount_kernel, dim3(a.chunks < cap ? a.chunks : cap, B), dim3(UN_THREADS), 0, st, a);
    PC_CHECK_LAUNCH();
    pc_loss_args l{};
    l.y = y_sorted;
    for (int i = 0; i < 4; ++i) l.lam[i] = lam4[i];
    l.sreg = scale_regularization; l.lam_weak = lam_weak; l.B = N;
    l.inv_B = (float)(1.0 / (double)N);           // (the double quotient rounded once more: what a caller of pc_loss_fwd_bwd passes)
    l.loss_out = loss_out; l.g_popcount = g_popcount; l.g_scale_const = g_scale_const;
    hipLaunchKernelGGL(unit_finish_loss_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const long long*>(a.acc_int),
                       reinterpret_cast<const long long*>(a.acc_frac), a.bad, dest, popcount_sorted, popcount_caller, stats, l);
    PC_CHECK_LAUNCH();
    return 0;
}
