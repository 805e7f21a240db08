// k_search_local.hip - the matching loop of Tracking::SearchLocalPoints (Tracking.cpp:1346-1805) on the device:
//   ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)  ORBmatcher.cpp:32-116, with Frame::GetFeaturesInArea  Frame.cpp:641-694
// The reference walks the local map points in order on the host; a point claims its best keypoint (F.mvpMapPoints[bestIdx] = pMP), which hides
// that keypoint from every LATER point.  Here:
//   k_local_candidates  SL_LANES lanes per map point: the window's grid cells in the reference's order (ix outer, iy inner, items of a cell
//                       ascending; the cells of one ix form one contiguous range of the CSR), level / window / blocked_in / uRight filters,
//                       Hamming distance; the first SL_CAP survivors are written packed (keypoint, octave, distance) in that order, and the
//                       count of all of them.  A point with more than SL_CAP candidates is flagged by its count and rescanned by the resolver.
//   k_local_resolve     one workgroup: the claim rule as a fixed point (claim_resolve, k_search_common.h).  Every round each point takes its
//                       best / second best over the candidates no point j < i has claimed in the previous round.
// The window walk, its compaction and the fixed point are k_search_common.h's (walk_window, compact_window, claim_resolve).
// The contract (include/jsorb.h, jsorb_search_local_points_async) is restated in numpy in tests/test_search_local_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef SL_CAP
#define SL_CAP 128                               // candidates kept per map point (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define SL_LDS_CLAIMS 16384                      // k_local_resolve keeps claim[] in LDS up to this many keypoints (64 KiB)
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
    if (p.L < 0 || p.L >= a.f.n_levels) return false;  // outside the contract: matches nothing
    // RadiusByViewingCos (ORBmatcher.cpp:118-124) compares the float with the DOUBLE 0.998: (double)c > 0.998 <=> c >= 0.998f
    float r = a.view_cos[i] >= 0.998f ? 2.5f : 4.0f;
    if (a.th != 1.0f) r *= a.th;
    p.R = r * a.f.scale[p.L];
    p.x = a.u[i];
    p.y = a.v[i];
    const float m = a.mbf * a.invz[i];                // mTrackProjXR = u - mbf*invz (Tracking.cpp:1617), two roundings
    p.xr = p.x - m;
    return sl_cells(a, p.x, p.y, p.R, p.x0, p.x1, p.y0, p.y1);
}

// keypoint k as a candidate of the point: -1 if a filter drops it, else its packed entry
__device__ __forceinline__ int sl_candidate(const SearchLocalArgs &a, const SlPoint &p, uint4 mlo, uint4 mhi, int k)
{
    const FrameView &f = a.f;
    const int oct = f.octave(k);
    if (oct < p.L - 1 || oct > p.L) return -1;
    if (!(fabsf(f.x(k) - p.x) < p.R && fabsf(f.y(k) - p.y) < p.R)) return -1;
    if (f.blocked && f.blocked[k]) return -1;          // F.mvpMapPoints[idx] && Observations() > 0
    if (f.u_right) {
        const float ur = f.u_right[k];
        if (ur > 0 && fabsf(p.xr - ur) > p.R) return -1;
    }
    uint4 lo, hi;
    sl_load_desc(f.desc + 32 * (size_t)k, lo, hi);
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
    const int count = compact_window<SL_CAP>(a.f.cell_start, a.rows, p.x0, p.x1, p.y0, p.y1, a.cand + (size_t)i * SL_CAP,
                                             [&](int j) { return sl_candidate(a, p, mlo, mhi, a.f.cell_items[j]); });
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
        walk_window<false>(a.f.cell_start, a.rows, p.x0, p.x1, p.y0, p.y1, 0, 1, [&](int j, bool) {
            const int c = sl_candidate(a, p, mlo, mhi, a.f.cell_items[j]);
            if (c >= 0) take(c);
        });
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
    __shared__ int s_count;
    const int tid = threadIdx.x, n = a.n_points;
    if (tid == 0) s_count = 0;
    claim_resolve<SL_CAP>(claim_in_lds ? s_claim : a.kp_match, n, a.f.n_kp, a.cand_n, a.match_kp, a.match_dist, a.kp_match, a.stats,
                          [&](const int *claim, int i, int &m, int &d) { sl_best(a, claim, i, m, d); });
    int matched = 0;
    for (int i = tid; i < n; i += 1024) matched += a.match_kp[i] >= 0;
    atomicAdd(&s_count, matched);
    __syncthreads();
    if (tid == 0) *a.n_matches = s_count;
}

void launch_local_candidates(const SearchLocalArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_local_candidates, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_local_resolve(const SearchLocalArgs &a, hipStream_t s)
{
    const int lds = a.f.n_kp <= SL_LDS_CLAIMS;
    hipLaunchKernelGGL(k_local_resolve, dim3(1), dim3(1024), lds ? (size_t)a.f.n_kp * sizeof(int) : 0, s, a, lds);
}

} // namespace jsorb
