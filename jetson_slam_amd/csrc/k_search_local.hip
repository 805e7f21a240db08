// k_search_local.hip - the matching loop of Tracking::SearchLocalPoints (Tracking.cpp:1346-1805) on the device:
//   ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)  ORBmatcher.cpp:32-116, with Frame::GetFeaturesInArea  Frame.cpp:641-694
// The reference walks the local map points in order on the host; a point claims its best keypoint (F.mvpMapPoints[bestIdx] = pMP), which hides
// that keypoint from every LATER point.  Here:
//   k_local_candidates  SL_LANES lanes per map point: the window's grid cells in the reference's order (ix outer, iy inner, items of a cell
//                       ascending; the cells of one ix form one contiguous range of the CSR), level / window / blocked_in / uRight filters,
//                       Hamming distance; the first SL_CAP survivors are written packed (keypoint, octave, distance) in that order, and the
//                       count of all of them.  A point with more than SL_CAP candidates is flagged by its count and rescanned by the resolver.
//   k_local_resolve     one workgroup: the claim rule as a fixed point.  Every round each point takes its best / second best over the candidates
//                       no point j < i has claimed in the previous round; then claim[k] = min i whose choice is k.  Point i depends only on the
//                       choices of j < i, so after round r the points < r are final: at most n + 1 rounds, and the fixed point is the
//                       sequential result.
// The contract (include/jsorb.h, jsorb_search_local_points_async) is restated in numpy in tests/test_search_local_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef SL_CAP
#define SL_CAP 128                               // candidates kept per map point (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define SL_LDS_CLAIMS 16384                      // k_local_resolve keeps claim[] in LDS up to this many keypoints (64 KiB)
#define SL_LANES 16                              // lanes per map point in k_local_candidates (4 points per wave)
#define SL_PACK(k, oct, d) ((k) << 13 | (oct) << 9 | (d))      // keypoint < 2^18, octave < 16, distance <= 256

int search_local_cap() { return SL_CAP; }

// the window of point i: GetFeaturesInArea(u, v, R, L-1, L)'s cell range with its early returns (sl_cells); false: no candidate at all
struct SlPoint {
    float x, y, R, xr;
    int L, x0, x1, y0, y1;
};
__device__ __forceinline__ bool sl_point(const SearchLocalArgs &a, int i, SlPoint &p)
{
    if (!a.in_frustum[i]) return false;              // !pMP->mbTrackInView
    p.L = a.level[i];
    if (p.L < 0 || p.L >= a.n_levels) return false;  // outside the contract: matches nothing
    // RadiusByViewingCos (ORBmatcher.cpp:118-124) compares the float with the DOUBLE 0.998: (double)c > 0.998 <=> c >= 0.998f
    float r = a.view_cos[i] >= 0.998f ? 2.5f : 4.0f;
    if (a.th != 1.0f) r *= a.th;
    p.R = r * a.scale[p.L];
    p.x = a.u[i];
    p.y = a.v[i];
    const float m = a.mbf * a.invz[i];                // mTrackProjXR = u - mbf*invz (Tracking.cpp:1617), two roundings
    p.xr = p.x - m;
    return sl_cells(a, p.x, p.y, p.R, p.x0, p.x1, p.y0, p.y1);
}

// keypoint k as a candidate of the point: -1 if a filter drops it, else its packed entry
__device__ __forceinline__ int sl_candidate(const SearchLocalArgs &a, const SlPoint &p, uint4 mlo, uint4 mhi, int k)
{
    const int n = a.n_kp;
    const int oct = a.soa[4 * (size_t)n + k];
    if (oct < p.L - 1 || oct > p.L) return -1;
    const float kx = a.xy_un ? a.xy_un[k] : (float)a.soa[k];
    const float ky = a.xy_un ? a.xy_un[n + k] : (float)a.soa[n + k];
    if (!(fabsf(kx - p.x) < p.R && fabsf(ky - p.y) < p.R)) return -1;
    if (a.blocked && a.blocked[k]) return -1;          // F.mvpMapPoints[idx] && Observations() > 0
    if (a.u_right) {
        const float ur = a.u_right[k];
        if (ur > 0 && fabsf(p.xr - ur) > p.R) return -1;
    }
    uint4 lo, hi;
    sl_load_desc(a.desc + 32 * (size_t)k, lo, hi);
    const int d = SL_HAMMING(lo, hi, mlo, mhi);
    return SL_PACK(k, oct, d);
}

__global__ __launch_bounds__(256) void k_local_candidates(SearchLocalArgs a)
{
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    if (i >= a.n_points) return;                     // (whole groups of SL_LANES lanes leave together)
    SlPoint p;
    if (!sl_point(a, i, p)) {
        if (lane == 0) a.cand_n[i] = 0;
        return;
    }
    uint4 mlo, mhi;
    sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
    const int shift = threadIdx.x % 64 / SL_LANES * SL_LANES;
    int *out = a.cand + (size_t)i * SL_CAP;
    int count = 0;
    for (int ix = p.x0; ix <= p.x1; ix++) {
        const int b = a.cell_start[ix * a.rows + p.y0], e = a.cell_start[ix * a.rows + p.y1 + 1];
        for (int base = b; base < e; base += SL_LANES) {
            const int j = base + lane;
            const int c = j < e ? sl_candidate(a, p, mlo, mhi, a.cell_items[j]) : -1;
            const unsigned m = (unsigned)(__ballot(c >= 0) >> shift) & ((1u << SL_LANES) - 1);
            const int pos = count + __popc(m & ((1u << lane) - 1));
            if (c >= 0 && pos < SL_CAP) out[pos] = c;
            count += __popc(m);
        }
    }
    if (lane == 0) a.cand_n[i] = count;
}

// the top two of point i over the candidates no point j < i claims: ORBmatcher.cpp:66-105 (strict < updates, ratio test only on equal levels)
__device__ void sl_best(const SearchLocalArgs &a, const int *claim, int i, int &match, int &match_dist)
{
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    auto take = [&](int c) {
        const int k = c >> 13, oct = (c >> 9) & 15, d = c & 511;
        if (claim[k] < i) return;                    // F.mvpMapPoints[k] = an earlier point of this call
        if (d < bestDist) {
            bestDist2 = bestDist; bestDist = d;
            bestLevel2 = bestLevel; bestLevel = oct;
            bestIdx = k;
        } else if (d < bestDist2) {
            bestLevel2 = oct; bestDist2 = d;
        }
    };
    const int cnt = a.cand_n[i];
    if (cnt <= SL_CAP) {
        const int *l = a.cand + (size_t)i * SL_CAP;
        for (int t = 0; t < cnt; t++) take(l[t]);
    } else {                                         // overflow: walk the window again, serially, in the same order
        SlPoint p;
        sl_point(a, i, p);
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        for (int ix = p.x0; ix <= p.x1; ix++) {
            const int b = a.cell_start[ix * a.rows + p.y0], e = a.cell_start[ix * a.rows + p.y1 + 1];
            for (int j = b; j < e; j++) {
                const int c = sl_candidate(a, p, mlo, mhi, a.cell_items[j]);
                if (c >= 0) take(c);
            }
        }
    }
    match = -1;
    match_dist = -1;
    if (bestIdx >= 0 && bestDist <= a.th_high && !(bestLevel == bestLevel2 && (float)bestDist > a.nn_ratio * (float)bestDist2)) {
        match = bestIdx;
        match_dist = bestDist;
    }
}

// One workgroup.  claim: LDS when the frame's keypoints fit (dynamic LDS of n_kp ints), else kp_match itself in global memory.
__global__ __launch_bounds__(1024) void k_local_resolve(SearchLocalArgs a, int claim_in_lds)
{
    extern __shared__ int s_claim[];
    __shared__ int s_count, s_cand, s_over;
    const int tid = threadIdx.x, n = a.n_points, N = a.n_kp;
    int *claim = claim_in_lds ? s_claim : a.kp_match;
    if (tid == 0) { s_count = 0; s_cand = 0; s_over = 0; }
    for (int k = tid; k < N; k += 1024) claim[k] = INT_MAX;
    int cand = 0, over = 0;
    for (int i = tid; i < n; i += 1024) {
        a.match_kp[i] = -2;                          // no choice yet: the first round changes every point
        const int c = a.cand_n[i];
        cand += c;
        over += c > SL_CAP;
    }
    __syncthreads();
    atomicAdd(&s_cand, cand);
    atomicAdd(&s_over, over);
    int rounds = 0;
    while (true) {
        rounds++;
        int changed = 0;
        for (int i = tid; i < n; i += 1024) {
            int m, d;
            sl_best(a, claim, i, m, d);
            if (m != a.match_kp[i]) { changed = 1; a.match_kp[i] = m; }
            a.match_dist[i] = d;
        }
        if (!__syncthreads_or(changed) || rounds > n) break;      // (the bound is never reached: n + 1 rounds suffice)
        for (int k = tid; k < N; k += 1024) claim[k] = INT_MAX;
        __syncthreads();
        for (int i = tid; i < n; i += 1024) {
            const int m = a.match_kp[i];
            if (m >= 0) atomicMin(&claim[m], i);
        }
        __syncthreads();
    }
    int matched = 0;
    for (int i = tid; i < n; i += 1024) matched += a.match_kp[i] >= 0;
    for (int k = tid; k < N; k += 1024) {
        const int c = claim[k];
        a.kp_match[k] = c == INT_MAX ? -1 : c;
    }
    atomicAdd(&s_count, matched);
    __syncthreads();
    if (tid == 0) {
        *a.n_matches = s_count;
        a.stats[0] = rounds;
        a.stats[1] = s_cand;
        a.stats[2] = s_over;
    }
}

void launch_local_candidates(const SearchLocalArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_local_candidates, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_local_resolve(const SearchLocalArgs &a, hipStream_t s)
{
    const int lds = a.n_kp <= SL_LDS_CLAIMS;
    hipLaunchKernelGGL(k_local_resolve, dim3(1), dim3(1024), lds ? (size_t)a.n_kp * sizeof(int) : 0, s, a, lds);
}

} // namespace jsorb
