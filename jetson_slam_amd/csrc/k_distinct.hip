// k_distinct.hip - MapPoint::ComputeDistinctiveDescriptors (MapPoint.cpp:273-338) for many map points in one call, on the device: per point the
//   descriptor of its observations with the least median Hamming distance to the others (the contract: include/jsorb.h,
//   jsorb_distinctive_descriptors_async).  Integer work throughout: pairwise popcounts, one rank per row, one first minimum.
// k_distinct_plan   one thread per point: the CSR checks (obs_start inside [0, n_obs] and not descending, the output row inside [0, n_out_rows)),
//                   -1 / -1 / unchanged for the empty and the invalid points, and the others binned by N into three lists with one ballot and one
//                   atomic per wave and list (the order within a list is free: points are independent).  The lists' counters ARE the first three
//                   statistics words.
// k_distinct_lanes<W>  W lanes per point, 256 / W points per workgroup, for N <= W: lane j holds D[j] in two uint4; row i's eight dwords come by
//                   __shfl(.., i, W); the row's rank-(N-1)/2 value is the smallest v with popcount(ballot(d <= v)) >= (N-1)/2 + 1 over the point's
//                   lanes below N - nine halving steps over [0, 256], the self-distance 0 one value among the others (:323-325 sort the whole row).
//                   Instantiated at DD_GROUP_LANES (the window kernels' SL_LANES: 4 points per wave) and at DD_WAVE_LANES (one wave per point).
// k_distinct_block  one workgroup per point for N > DD_WAVE_LANES: the descriptors staged in LDS by 16-byte loads (two planes of uint4: consecutive
//                   lanes read consecutive 16-byte slots) up to DD_LDS_DESC of them, read from global memory through obs_row beyond; rows dealt
//                   to the workgroup's DD_BLOCK_WAVES waves, columns to the lanes; the rank from a 257-bin count per row and a wave scan over the bins.
// The winner is the minimum of the key (median, i) - median << 16 | i in the lanes kernels, median << 32 | i in the block kernel, where i has no
// bound - which IS "the first i with the smallest median" (:319-332, strict < from INT_MAX with i ascending).
// A point whose obs_row holds an entry outside [0, n_rows) is found by the kernel that loads its rows, before any descriptor is read: -1 / -1, row
// untouched, one more in the invalid count.  No kernel reads or writes outside the arrays whatever the device inputs hold.
// The launch shapes depend on host sizes only: a list of points with N > c holds at most n_obs / (c + 1) of them when the points' ranges do not
// overlap, and each kernel strides over its list for the CSR where they do.
#include "jsorb_launch.h"
#include "k_search_common.h"

#ifndef DD_GROUP_LANES
#define DD_GROUP_LANES 16                        // = SL_LANES: lanes per point of the group tier
#endif
#ifndef DD_WAVE_LANES
#define DD_WAVE_LANES 64                         // lanes per point of the wave tier
#endif
#ifndef DD_LDS_DESC
#define DD_LDS_DESC 1024                         // descriptors k_distinct_block stages in LDS (32 KiB)
#endif
#ifndef DD_BLOCK_WAVES
#define DD_BLOCK_WAVES 16                        // waves of k_distinct_block's workgroup: rows in flight per point (measured against 4: DESIGN.md section 22)
#endif

namespace jsorb {

static_assert(DD_GROUP_LANES >= 1 && DD_GROUP_LANES <= DD_WAVE_LANES && DD_WAVE_LANES <= 64, "tiers ascend, a point's lanes fit a wave");
static_assert((DD_GROUP_LANES & (DD_GROUP_LANES - 1)) == 0 && (DD_WAVE_LANES & (DD_WAVE_LANES - 1)) == 0, "__shfl widths are powers of two");
static_assert(DD_BLOCK_WAVES >= 1 && DD_BLOCK_WAVES <= 16 && DD_LDS_DESC >= 1 && DD_LDS_DESC * 32 <= 32 * 1024, "the staged descriptors fit LDS next to the bins");

// the output row of point p, or -1: nothing is written for it (no desc_out, or a row outside the array - the plan kernel has made such a point invalid)
__device__ __forceinline__ int dd_out_row(const DistinctArgs &a, int p)
{
    if (!a.desc_out) return -1;
    const int r = a.out_row ? a.out_row[p] : p;
    return (unsigned)r < (unsigned)a.n_out_rows ? r : -1;
}

// :336 by one lane: the winner's bytes into the point's row, `changed` from a compare with what the row held
__device__ __forceinline__ void dd_store(const DistinctArgs &a, int p, const uint4 &lo, const uint4 &hi)
{
    const int r = dd_out_row(a, p);
    int diff = 0;
    if (r >= 0) {
        uint4 *q = reinterpret_cast<uint4 *>(a.desc_out + 32 * (size_t)r);
        const uint4 olo = q[0], ohi = q[1];
        diff = SL_HAMMING(lo, hi, olo, ohi) != 0;
        if (diff) { q[0] = lo; q[1] = hi; }          // equal bytes need no store: the row holds them
    }
    if (a.changed) a.changed[p] = (uint8_t)diff;
    if (diff) atomicAdd(&a.stats[6], 1);
}

__device__ __forceinline__ void dd_invalid(const DistinctArgs &a, int p)
{
    a.best_obs[p] = -1;
    a.best_median[p] = -1;
    if (a.changed) a.changed[p] = 0;
    atomicAdd(&a.stats[5], 1);
}

__global__ __launch_bounds__(256) void k_distinct_plan(DistinctArgs a)
{
    const int p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64;
    int tier = -1, n = 0;                        // 0 group, 1 wave, 2 block, 3 empty, 4 invalid; -1 no point
    if (p < a.n_points) {
        const int s = a.obs_start[p], e = a.obs_start[p + 1];
        n = e - s;
        if (s < 0 || s > a.n_obs || e < 0 || e > a.n_obs || e < s || (a.desc_out && dd_out_row(a, p) < 0)) tier = 4;
        else if (n == 0) tier = 3;                                                       // :287, :300: mDescriptor stays
        else tier = n <= DD_GROUP_LANES ? 0 : n <= DD_WAVE_LANES ? 1 : 2;
        if (tier >= 3) {
            a.best_obs[p] = -1;
            a.best_median[p] = -1;
            if (a.changed) a.changed[p] = 0;
            n = 0;
        }
    }
    const unsigned long long below = (1ull << lane) - 1;
    for (int t = 0; t < 3; t++) {
        const unsigned long long m = __ballot(tier == t);
        if (!m) continue;
        int base = 0;
        if (lane == __ffsll((long long)m) - 1) base = atomicAdd(&a.stats[t], __popcll(m));
        base = __shfl(base, __ffsll((long long)m) - 1);
        if (tier == t) a.list[(size_t)t * a.n_points + base + __popcll(m & below)] = p;
    }
    const int n_lds_over = __popcll(__ballot(tier == 2 && n > DD_LDS_DESC)), n_empty = __popcll(__ballot(tier == 3)), n_bad = __popcll(__ballot(tier == 4));
    for (int s = 32; s > 0; s >>= 1) n = max(n, __shfl_xor(n, s));
    if (lane == 0) {
        if (n_lds_over) atomicAdd(&a.stats[3], n_lds_over);
        if (n_empty) atomicAdd(&a.stats[4], n_empty);
        if (n_bad) atomicAdd(&a.stats[5], n_bad);
        if (n) atomicMax(&a.stats[7], n);
    }
}

// one point of a lanes tier by its W lanes; every lane of the point makes the same decisions, so the shuffles and ballots stay among them
template <int W> __device__ __forceinline__ void dd_lanes_point(const DistinctArgs &a, int p)
{
    const int j = threadIdx.x % W, shift = threadIdx.x % 64 / W * W;
    const int s = a.obs_start[p], N = a.obs_start[p + 1] - s;                // 1 <= N <= W: the plan's bin
    const unsigned long long mine = (W == 64 ? ~0ull : (1ull << W) - 1) << shift;
    const int row = j < N ? a.obs_row[s + j] : 0;
    if (__ballot(j < N && (unsigned)row >= (unsigned)a.n_rows) & mine) {
        if (j == 0) dd_invalid(a, p);
        return;
    }
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (j < N) sl_load_desc(a.kf_desc + 32 * (size_t)row, lo, hi);
    const int need = (N - 1) / 2 + 1;            // :325: vDists[0.5*(N-1)] of the sorted row is the smallest v with `need` values <= v
    unsigned best = ~0u;
    for (int i = 0; i < N; i++) {
        uint4 rlo, rhi;
        rlo.x = __shfl(lo.x, i, W); rlo.y = __shfl(lo.y, i, W); rlo.z = __shfl(lo.z, i, W); rlo.w = __shfl(lo.w, i, W);
        rhi.x = __shfl(hi.x, i, W); rhi.y = __shfl(hi.y, i, W); rhi.z = __shfl(hi.z, i, W); rhi.w = __shfl(hi.w, i, W);
        const int d = j < N ? SL_HAMMING(lo, hi, rlo, rhi) : 1 << 20;        // :310-315 (lane i: 0, the self-distance of :309)
        int v0 = 0, v1 = 256;
        for (int step = 0; step < 9; step++) {
            const int mid = (v0 + v1) >> 1;
            if (__popcll(__ballot(d <= mid) & mine) >= need) v1 = mid; else v0 = mid + 1;
        }
        best = min(best, (unsigned)v0 << 16 | (unsigned)i);                   // :327-331
    }
    const int bi = (int)(best & 0xffff);
    uint4 wlo, whi;
    wlo.x = __shfl(lo.x, bi, W); wlo.y = __shfl(lo.y, bi, W); wlo.z = __shfl(lo.z, bi, W); wlo.w = __shfl(lo.w, bi, W);
    whi.x = __shfl(hi.x, bi, W); whi.y = __shfl(hi.y, bi, W); whi.z = __shfl(hi.z, bi, W); whi.w = __shfl(hi.w, bi, W);
    if (j == 0) {
        a.best_obs[p] = bi;
        a.best_median[p] = (int)(best >> 16);
        dd_store(a, p, wlo, whi);
    }
}

// The tiers' launches are sized for observation ranges that do not overlap (launch_distinct); every kernel strides over its list, so a CSR whose
// valid points share observations - more points in a list than the host sizes promise - is served all the same.
template <int W> __global__ __launch_bounds__(256) void k_distinct_lanes(DistinctArgs a, int tier)
{
    const int count = a.stats[tier];
    for (int q = blockIdx.x * (256 / W) + threadIdx.x / W; q < count; q += gridDim.x * (256 / W)) dd_lanes_point<W>(a, a.list[(size_t)tier * a.n_points + q]);
}

__global__ __launch_bounds__(64 * DD_BLOCK_WAVES) void k_distinct_block(DistinctArgs a)
{
    __shared__ uint4 s_lo[DD_LDS_DESC], s_hi[DD_LDS_DESC];
    __shared__ int s_bins[DD_BLOCK_WAVES][260];  // 257 bins per wave, a multiple of 4 words apart
    __shared__ unsigned long long s_best[DD_BLOCK_WAVES];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, count = a.stats[2];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {        // (uniform over the workgroup: every barrier below is met by everyone)
        const int p = a.list[(size_t)2 * a.n_points + q], s = a.obs_start[p], N = a.obs_start[p + 1] - s;
        const bool staged = N <= DD_LDS_DESC;
        int bad = 0;
        for (int j = threadIdx.x; j < N; j += 64 * DD_BLOCK_WAVES) {
            const int row = a.obs_row[s + j];
            if ((unsigned)row >= (unsigned)a.n_rows) bad = 1;
            else if (staged) sl_load_desc(a.kf_desc + 32 * (size_t)row, s_lo[j], s_hi[j]);
        }
        for (int b = threadIdx.x; b < DD_BLOCK_WAVES * 260; b += 64 * DD_BLOCK_WAVES) (&s_bins[0][0])[b] = 0;
        if (__syncthreads_or(bad)) {                 // also the barrier behind the staging and the cleared bins
            if (threadIdx.x == 0) dd_invalid(a, p);
            continue;
        }
        const int need = (N - 1) / 2 + 1;
        int *bins = s_bins[wave];
        unsigned long long best = ~0ull;
        for (int i0 = 0; i0 < N; i0 += DD_BLOCK_WAVES) {      // the same trip count for every wave: both barriers are met by everyone
            const int i = i0 + wave;
            if (i < N) {
                uint4 rlo, rhi;
                if (staged) { rlo = s_lo[i]; rhi = s_hi[i]; } else sl_load_desc(a.kf_desc + 32 * (size_t)a.obs_row[s + i], rlo, rhi);
                for (int j = lane; j < N; j += 64) {
                    uint4 lo, hi;
                    if (staged) { lo = s_lo[j]; hi = s_hi[j]; } else sl_load_desc(a.kf_desc + 32 * (size_t)a.obs_row[s + j], lo, hi);
                    atomicAdd(&bins[SL_HAMMING(lo, hi, rlo, rhi)], 1);
                }
            }
            __syncthreads();
            if (i < N) {
                // the smallest v whose bins 0 .. v hold `need` values: lane l sums the bins 4 l .. 4 l + 3, a wave scan, then the lane that crosses
                int c[4], sum = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) { c[k] = bins[4 * lane + k]; bins[4 * lane + k] = 0; sum += c[k]; }
                if (lane == 0) bins[256] = 0;        // (a row that does not cross below 256 has its median there)
                int incl = sum;
                for (int d = 1; d < 64; d <<= 1) {
                    const int t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                const unsigned long long cross = __ballot(incl >= need);
                int v = 256;
                if (cross) {
                    const int l = __ffsll((long long)cross) - 1;
                    int run = incl, bin = 4 * lane + 3;                          // (meaningful in lane l: its four bins cross)
#pragma unroll
                    for (int k = 3; k > 0; k--) { run -= c[k]; if (run >= need) bin = 4 * lane + k - 1; }
                    v = __shfl(bin, l);
                }
                best = min(best, (unsigned long long)v << 32 | (unsigned)i);
            }
            __syncthreads();
        }
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < DD_BLOCK_WAVES; w++) best = min(best, s_best[w]);
            const int bi = (int)(best & 0xffffffffu);
            a.best_obs[p] = bi;
            a.best_median[p] = (int)(best >> 32);
            uint4 lo, hi;
            sl_load_desc(a.kf_desc + 32 * (size_t)a.obs_row[s + bi], lo, hi);
            dd_store(a, p, lo, hi);
        }
    }   // the next point: thread 0 has read s_best before it meets the others at that point's first barrier
}

int distinct_group_lanes() { return DD_GROUP_LANES; }
int distinct_wave_lanes() { return DD_WAVE_LANES; }
int distinct_lds_desc() { return DD_LDS_DESC; }

void launch_distinct(const DistinctArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    hipLaunchKernelGGL(k_distinct_plan, dim3((a.n_points + 255) / 256), dim3(256), 0, s, a);
    // a list of points with more than c observations each holds at most n_obs / (c + 1) points (ranges that overlap: the kernels stride)
    const int n_group = a.n_points, n_wave = std::min(a.n_points, a.n_obs / (DD_GROUP_LANES + 1)), n_block = std::min(a.n_points, a.n_obs / (DD_WAVE_LANES + 1));
    const int per_group = 256 / DD_GROUP_LANES, per_wave = 256 / DD_WAVE_LANES;
    hipLaunchKernelGGL(k_distinct_lanes<DD_GROUP_LANES>, dim3((n_group + per_group - 1) / per_group), dim3(256), 0, s, a, 0);
    if (n_wave > 0) hipLaunchKernelGGL(k_distinct_lanes<DD_WAVE_LANES>, dim3((n_wave + per_wave - 1) / per_wave), dim3(256), 0, s, a, 1);
    if (n_block > 0) hipLaunchKernelGGL(k_distinct_block, dim3(n_block), dim3(64 * DD_BLOCK_WAVES), 0, s, a);
}

} // namespace jsorb
