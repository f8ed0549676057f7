// census_adjust.hip -- dasymetric adjustment across census levels on the census table (census_table.hip), per member: the totals of
// the units of a level l after the map has been rescaled so that every unit of a level a sums to its census count, without the map.
//
//   pc_census_pair_plan       the (unit of l, unit of a) pairs that share a pixel, as one more id raster (planned once per region); the
//                             existing pc_census_accumulate fills its columns as one more level
//   pc_census_adjust_finalize adjusted totals of every member and of the ensemble-mean map, mean and (n - 1) standard deviation
//
// The adjustment (adjust_map_to_census, data/PopulationDataset.py:823-852) multiplies every pixel of a unit c of level a by ONE factor
// POP[c] / P[c], so the adjusted total of a unit f of level l follows from the joint sums S[f, c] over the pixels that lie in f and c:
//     A[f] = sum_c S[f, c] * POP[c] / P[c]  +  (what f holds outside every unit of a, unscaled).
// Rasters of nested polygons give almost every f one partner c and a border f two or three: a unit has at most PC_CENSUS_PAIR_SLOTS
// partners, a unit with more is reported (flag word) and the plan refused.
//
// Pair plan.  Pixel p belongs to f = b_l[p] when 0 <= f < num_l and to c = b_a[p] when 0 <= c < num_a; anything else is "no unit".
//   partners[f][k]  the distinct c that share a pixel with f, ASCENDING, padded with -1          (a function of the two rasters alone)
//   count[f]        how many
//   pair_plane[p]   base[f] + k with partners[f][k] == c, -1 where f or c is no unit; base = exclusive prefix sum of count (the caller's),
//                   so the ids are compact, NP = base[num_l] pairs ordered by (f, c)
// PC_CENSUS_PAIR_SLOTS + 1 rounds over the rasters: round k takes, per f, the integer minimum of the c above round k - 1's result
// (atomicMin: order-free, so the result has the same bits whatever the schedule); the last round only detects a fifth partner.  While
// num_l fits, a workgroup takes its minima in an LDS table first and issues one global atomicMin per unit it met.  census_table.hip's
// rule holds: no hash probing, no compare-and-swap retry, no spin wait, no ticket; every loop bound is a function of the launch geometry.
// Both planes are read with 16-byte loads from any 4-byte aligned address (a row band of a larger raster): a scalar head up to b_l's first
// 16-byte boundary, vector loads from there (b_a and the pair plane at whatever phase they have), scalar tail; 64-bit pixel indices.
//
// Adjusted finalize, one lane per unit f of level l, no atomics.  table: the int64 census table (2^-30 fixed point), member m in row m.
//   P[m][c]      = table[m][off_a + c]: the sum over ALL pixels of c whatever their unit of l (the reference's pred_census_count)
//   factor[m][c] = (double)pop[c] / ((double)P[m][c] * 2^-30)  when has[c] and P[m][c] > 0, else 1.0   (:847-848 skips a zero total; a unit
//                  without a census row is never scaled)
//   pair_k       = table[m][off_p + base[f] + k], c_k = pair_c[base[f] + k], k < base[f + 1] - base[f] <= PC_CENSUS_PAIR_SLOTS
//   rem[m][f]    = table[m][off_l + f] - sum_k pair_k                     (exact integer difference: the pixels of f in no unit of a)
//   adj[m][f]    = 2^-30 * ((double)rem + sum_k (double)pair_k * factor[m][c_k]),  k ascending, every operation rounded on its own (no fma)
//   adj[M][f]    the adjustment of the ENSEMBLE-MEAN map (what the reference adjusts): the same formulas on the exact integer sums over
//                the members of P, pair and rem, with factor[c] = ((double)pop[c] * (double)M) / ((double)sum_m P * 2^-30) when has[c] and
//                sum_m P > 0, and the result divided by (double)M
//   mean / std   over rows 0 .. M - 1, two passes in double as census_finalize_kernel (std 0 for M == 1)
// Level a judged on itself needs no pair plane (base == NULL): adj[m][c] = (double)pop[c] where c is scaled, P[m][c] * 2^-30 otherwise;
// row M likewise with sum_m P (divided by M where unscaled).
#include "common.h"

namespace {

constexpr int CA_THREADS = 256;
constexpr int CA_MAX_GRID = 2048;
constexpr int CA_LDS_IDS = 8192;                 // units of level l whose minima a workgroup keeps in LDS (32 KB)
constexpr int CA_NONE = 0x7fffffff;              // "no partner yet": the identity of the integer minimum
constexpr double CA_FIX = (double)(1ull << PC_CENSUS_FIX_SHIFT);
static_assert(PC_CENSUS_PAIR_SLOTS == 4, "a unit's partners are one 16-byte row");

typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));      // 16-byte access at 4-byte alignment (global memory only)

struct PairArgs {
    const int32_t* bl; const int32_t* ba; int64_t n;
    int num_l, num_a;
    int64_t head;                       // elements before b_l's first 16-byte boundary
    const int32_t* prev; int prev_stride;    // round k - 1's result per unit (NULL: round 0, every c qualifies)
    int32_t* cur; int cur_stride;            // this round's minimum per unit, CA_NONE before the launch
    int lds;                                 // 1: num_l <= CA_LDS_IDS, minima go through the LDS table
};

// one pixel of a round: the minimum over the c above prev[f]; (lf, lc) is the lane's last pair handed on (runs along a row repeat it)
__device__ __forceinline__ void ca_round_pixel(const PairArgs& a, int* tab, int f, int c, int& lf, int& lc) {
    if ((unsigned)f >= (unsigned)a.num_l || (unsigned)c >= (unsigned)a.num_a) return;
    if (f == lf && c == lc) return;
    lf = f; lc = c;
    if (a.prev) {
        const int p = a.prev[(int64_t)f * a.prev_stride];
        if (p == CA_NONE || c <= p) return;                 // (p == CA_NONE: the unit had no further partner one round ago)
    }
    if (a.lds) atomicMin(&tab[f], c);
    else atomicMin(&a.cur[(int64_t)f * a.cur_stride], c);
}

__global__ __launch_bounds__(CA_THREADS) void census_pair_round_kernel(const PairArgs a) {
    __shared__ int tab[CA_LDS_IDS];
    const int t = threadIdx.x;
    if (a.lds) {
        for (int i = t; i < a.num_l; i += CA_THREADS) tab[i] = CA_NONE;
        __syncthreads();
    }
    int lf = -1, lc = -1;
    const int32_t* lv = a.bl + a.head;
    const int32_t* av = a.ba + a.head;
    const int64_t n4 = (a.n - a.head) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * CA_THREADS + t; i < n4; i += (int64_t)gridDim.x * CA_THREADS) {
        const int4 f = *reinterpret_cast<const int4*>(lv + 4 * i);
        const i32x4u c = *reinterpret_cast<const i32x4u*>(av + 4 * i);
        ca_round_pixel(a, tab, f.x, c[0], lf, lc);
        ca_round_pixel(a, tab, f.y, c[1], lf, lc);
        ca_round_pixel(a, tab, f.z, c[2], lf, lc);
        ca_round_pixel(a, tab, f.w, c[3], lf, lc);
    }
    if (blockIdx.x == 0) {
        for (int64_t j = t; j < a.head + (a.n - a.head - 4 * n4); j += CA_THREADS) {
            const int64_t i = j < a.head ? j : a.head + 4 * n4 + (j - a.head);
            ca_round_pixel(a, tab, a.bl[i], a.ba[i], lf, lc);
        }
    }
    if (a.lds) {
        __syncthreads();
        for (int i = t; i < a.num_l; i += CA_THREADS) {
            const int v = tab[i];
            if (v != CA_NONE) atomicMin(&a.cur[(int64_t)i * a.cur_stride], v);
        }
    }
}

// partners[num_l][SLOTS] and over[num_l] = CA_NONE; flags = {0, CA_NONE}
__global__ __launch_bounds__(CA_THREADS) void census_pair_init_kernel(int32_t* partners, int32_t* over, int num_l, int32_t* flags) {
    const int64_t n = (int64_t)num_l * (PC_CENSUS_PAIR_SLOTS + 1);
    for (int64_t i = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CA_THREADS) {
        if (i < (int64_t)num_l * PC_CENSUS_PAIR_SLOTS) partners[i] = CA_NONE;
        else over[i - (int64_t)num_l * PC_CENSUS_PAIR_SLOTS] = CA_NONE;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { flags[0] = 0; flags[1] = CA_NONE; }
}

// count[f], the -1 padding, and the flag word: bit 0 of flags[0] and flags[1] = the smallest unit with a fifth partner
__global__ __launch_bounds__(CA_THREADS) void census_pair_count_kernel(int32_t* partners, const int32_t* __restrict__ over, int num_l,
                                                                      int32_t* __restrict__ count, int32_t* flags) {
    for (int f = blockIdx.x * CA_THREADS + threadIdx.x; f < num_l; f += gridDim.x * CA_THREADS) {
        int4 p = *reinterpret_cast<const int4*>(partners + (int64_t)f * PC_CENSUS_PAIR_SLOTS);
        const int n = (p.x != CA_NONE) + (p.y != CA_NONE) + (p.z != CA_NONE) + (p.w != CA_NONE);
        if (p.x == CA_NONE) p.x = -1;
        if (p.y == CA_NONE) p.y = -1;
        if (p.z == CA_NONE) p.z = -1;
        if (p.w == CA_NONE) p.w = -1;
        *reinterpret_cast<int4*>(partners + (int64_t)f * PC_CENSUS_PAIR_SLOTS) = p;
        count[f] = n;
        if (over[f] != CA_NONE) { atomicOr(&flags[0], 1); atomicMin(&flags[1], f); }
    }
}

struct WriteArgs {
    const int32_t* bl; const int32_t* ba; int64_t n;
    int num_l, num_a;
    int64_t head;
    const int32_t* partners; const int32_t* base;
    int32_t* plane;
};

__device__ __forceinline__ int ca_pair_id(const WriteArgs& a, int f, int c) {
    if ((unsigned)f >= (unsigned)a.num_l || (unsigned)c >= (unsigned)a.num_a) return -1;
    const int4 p = *reinterpret_cast<const int4*>(a.partners + (int64_t)f * PC_CENSUS_PAIR_SLOTS);
    const int k = p.x == c ? 0 : p.y == c ? 1 : p.z == c ? 2 : p.w == c ? 3 : -1;          // (c >= 0: the -1 padding never matches)
    return k < 0 ? -1 : a.base[f] + k;
}

__global__ __launch_bounds__(CA_THREADS) void census_pair_write_kernel(const WriteArgs a) {
    const int32_t* lv = a.bl + a.head;
    const int32_t* av = a.ba + a.head;
    int32_t* ov = a.plane + a.head;
    const int64_t n4 = (a.n - a.head) >> 2;
    for (int64_t i = (int64_t)blockIdx.x * CA_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * CA_THREADS) {
        const int4 f = *reinterpret_cast<const int4*>(lv + 4 * i);
        const i32x4u c = *reinterpret_cast<const i32x4u*>(av + 4 * i);
        i32x4u o;
        o[0] = ca_pair_id(a, f.x, c[0]); o[1] = ca_pair_id(a, f.y, c[1]); o[2] = ca_pair_id(a, f.z, c[2]); o[3] = ca_pair_id(a, f.w, c[3]);
        *reinterpret_cast<i32x4u*>(ov + 4 * i) = o;
    }
    if (blockIdx.x == 0) {
        for (int64_t j = threadIdx.x; j < a.head + (a.n - a.head - 4 * n4); j += CA_THREADS) {
            const int64_t i = j < a.head ? j : a.head + 4 * n4 + (j - a.head);
            a.plane[i] = ca_pair_id(a, a.bl[i], a.ba[i]);
        }
    }
}

// ---- adjusted finalize -------------------------------------------------------------------------------------------------------------
struct AdjustArgs {
    const long long* table; int M; int64_t T;
    int64_t off_l, off_a, off_p;
    int num_l, num_a; int64_t num_p;
    const int32_t* base; const int32_t* pair_c;         // base == NULL: level a judged on itself
    const float* pop; const uint8_t* has;
    double* adj; float* mean; float* stdv;
};

// factor of a unit of level a with the integer total P (of one member: scale 1; of the sum over members: scale M)
__device__ __forceinline__ double ca_factor(const AdjustArgs& a, int c, long long P, double scale) {
    if (!a.has[c] || P <= 0) return 1.0;
    return __ddiv_rn(__dmul_rn((double)a.pop[c], scale), __dmul_rn((double)P, 1.0 / CA_FIX));
}

__global__ __launch_bounds__(CA_THREADS) void census_adjust_finalize_kernel(const AdjustArgs a) {
    for (int f = blockIdx.x * CA_THREADS + threadIdx.x; f < a.num_l; f += gridDim.x * CA_THREADS) {
        const double dM = (double)a.M;
        if (!a.base) {
            long long sP = 0;
            const bool row = a.has[f] != 0;
            for (int m = 0; m < a.M; ++m) {
                const long long P = a.table[m * a.T + a.off_a + f];
                sP += P;
                a.adj[(int64_t)m * a.num_l + f] = row && P > 0 ? (double)a.pop[f] : (double)P * (1.0 / CA_FIX);
            }
            a.adj[(int64_t)a.M * a.num_l + f] = row && sP > 0 ? (double)a.pop[f] : __ddiv_rn((double)sP * (1.0 / CA_FIX), dM);
        } else {
            // (a plan of pc_census_pair_plan meets these bounds; one that does not must not send a load out of the tables)
            const int b0 = a.base[f];
            const int nk = b0 < 0 || a.base[f + 1] > a.num_p ? 0 : min(max(a.base[f + 1] - b0, 0), PC_CENSUS_PAIR_SLOTS);
            int ck[PC_CENSUS_PAIR_SLOTS];
            long long sPair[PC_CENSUS_PAIR_SLOTS], sPc[PC_CENSUS_PAIR_SLOTS], sRem = 0;
#pragma unroll
            for (int k = 0; k < PC_CENSUS_PAIR_SLOTS; ++k) {
                ck[k] = k < nk ? min(max(a.pair_c[b0 + k], 0), a.num_a - 1) : 0;
                sPair[k] = 0; sPc[k] = 0;
            }
            for (int m = 0; m < a.M; ++m) {
                const long long* row = a.table + m * a.T;
                long long rem = row[a.off_l + f];
                long long pair[PC_CENSUS_PAIR_SLOTS];
                double fac[PC_CENSUS_PAIR_SLOTS];
#pragma unroll
                for (int k = 0; k < PC_CENSUS_PAIR_SLOTS; ++k) {
                    pair[k] = 0; fac[k] = 1.0;
                    if (k < nk) {
                        pair[k] = row[a.off_p + b0 + k];
                        const long long P = row[a.off_a + ck[k]];
                        fac[k] = ca_factor(a, ck[k], P, 1.0);
                        rem -= pair[k];
                        sPair[k] += pair[k]; sPc[k] += P;
                    }
                }
                sRem += rem;
                double s = (double)rem;
#pragma unroll
                for (int k = 0; k < PC_CENSUS_PAIR_SLOTS; ++k)
                    if (k < nk) s = __dadd_rn(s, __dmul_rn((double)pair[k], fac[k]));
                a.adj[(int64_t)m * a.num_l + f] = s * (1.0 / CA_FIX);
            }
            double s = (double)sRem;
#pragma unroll
            for (int k = 0; k < PC_CENSUS_PAIR_SLOTS; ++k)
                if (k < nk) s = __dadd_rn(s, __dmul_rn((double)sPair[k], ca_factor(a, ck[k], sPc[k], dM)));
            a.adj[(int64_t)a.M * a.num_l + f] = __ddiv_rn(s * (1.0 / CA_FIX), dM);
        }
        // mean / std over the members' rows (this lane wrote them)
        double sum = 0.0;
        for (int m = 0; m < a.M; ++m) sum += a.adj[(int64_t)m * a.num_l + f];
        const double mu = sum / dM;
        double ss = 0.0;
        for (int m = 0; m < a.M; ++m) {
            const double d = a.adj[(int64_t)m * a.num_l + f] - mu;
            ss += d * d;
        }
        a.mean[f] = (float)mu;
        a.stdv[f] = a.M > 1 ? (float)sqrt(ss / (double)(a.M - 1)) : 0.f;
    }
}

int ca_grid(int64_t items) {
    const int64_t g = (items + CA_THREADS - 1) / CA_THREADS;
    return (int)(g < 1 ? 1 : g < CA_MAX_GRID ? g : CA_MAX_GRID);
}

int64_t ca_head(const void* p, int64_t n) {
    const int64_t h = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
    return h < n ? h : n;
}

}  // namespace

// pair_plane == NULL: the rounds -- partners[num_l][PC_CENSUS_PAIR_SLOTS], count[num_l], flags[2] = {bit 0: a unit has more partners than
// slots, the smallest such unit}; scratch: int32 [num_l].  pair_plane != NULL: the write pass from partners and base[num_l] (exclusive
// prefix sum of count); count, flags and scratch are not touched (may be NULL).
extern "C" int pc_census_pair_plan(const int32_t* b_l, const int32_t* b_a, int64_t n, int num_l, int num_a, int32_t* partners,
                                   int32_t* count, int32_t* flags, int32_t* scratch, const int32_t* base, int32_t* pair_plane,
                                   void* stream) {
    if (!b_l || !b_a || !partners || n < 0 || num_l < 1 || num_a < 1) return PC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(b_l) & 3) || (reinterpret_cast<uintptr_t>(b_a) & 3) || (reinterpret_cast<uintptr_t>(partners) & 15))
        return PC_EINVAL;
    if (pair_plane ? (!base || (reinterpret_cast<uintptr_t>(pair_plane) & 3)) : (!count || !flags || !scratch)) return PC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t head = ca_head(b_l, n);
    if (pair_plane) {
        if (n == 0) return 0;
        WriteArgs w{};
        w.bl = b_l; w.ba = b_a; w.n = n; w.num_l = num_l; w.num_a = num_a; w.head = head;
        w.partners = partners; w.base = base; w.plane = pair_plane;
        hipLaunchKernelGGL(census_pair_write_kernel, dim3(ca_grid(n / 4)), dim3(CA_THREADS), 0, s, w);
        PC_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(census_pair_init_kernel, dim3(ca_grid((int64_t)num_l * (PC_CENSUS_PAIR_SLOTS + 1))), dim3(CA_THREADS), 0, s, partners,
                       scratch, num_l, flags);
    PC_CHECK_LAUNCH();
    for (int k = 0; k <= PC_CENSUS_PAIR_SLOTS && n > 0; ++k) {
        PairArgs a{};
        a.bl = b_l; a.ba = b_a; a.n = n; a.num_l = num_l; a.num_a = num_a; a.head = head;
        a.prev = k ? partners + (k - 1) : nullptr; a.prev_stride = PC_CENSUS_PAIR_SLOTS;
        if (k < PC_CENSUS_PAIR_SLOTS) { a.cur = partners + k; a.cur_stride = PC_CENSUS_PAIR_SLOTS; }
        else { a.cur = scratch; a.cur_stride = 1; }
        a.lds = num_l <= CA_LDS_IDS;
        hipLaunchKernelGGL(census_pair_round_kernel, dim3(ca_grid(n / 4)), dim3(CA_THREADS), 0, s, a);
        PC_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(census_pair_count_kernel, dim3(ca_grid(num_l)), dim3(CA_THREADS), 0, s, partners, scratch, num_l, count, flags);
    PC_CHECK_LAUNCH();
    return 0;
}

extern "C" int pc_census_adjust_finalize(const int64_t* table, int M, int64_t T, int64_t off_l, int64_t off_a, int64_t off_p, int num_l,
                                         int num_a, int64_t num_p, const int32_t* base, const int32_t* pair_c, const float* pop,
                                         const uint8_t* has, double* adj, float* mean, float* stdv, void* stream) {
    if (!table || !pop || !has || !adj || !mean || !stdv) return PC_EINVAL;
    if (M < 1 || T < 1 || num_l < 1 || num_a < 1 || off_l < 0 || off_a < 0 || off_l + num_l > T || off_a + num_a > T) return PC_EINVAL;
    if (base) {
        if ((!pair_c && num_p > 0) || num_p < 0 || off_p < 0 || off_p + num_p > T) return PC_EINVAL;        // (no pair at all: num_p == 0)
    } else if (off_l != off_a || num_l != num_a) return PC_EINVAL;
    AdjustArgs a{};
    a.table = reinterpret_cast<const long long*>(table); a.M = M; a.T = T;
    a.off_l = off_l; a.off_a = off_a; a.off_p = off_p; a.num_l = num_l; a.num_a = num_a; a.num_p = num_p;
    a.base = base; a.pair_c = pair_c; a.pop = pop; a.has = has; a.adj = adj; a.mean = mean; a.stdv = stdv;
    hipLaunchKernelGGL(census_adjust_finalize_kernel, dim3(ca_grid(num_l)), dim3(CA_THREADS), 0, (hipStream_t)stream, a);
    PC_CHECK_LAUNCH();
    return 0;
}
