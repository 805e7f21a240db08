// k_search_kf.hip - the matcher Tracking::Relocalization runs twice per pose hypothesis (Tracking.cpp:2062-2092) on the device:
//   ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist)  ORBmatcher.cpp:1968-2095, with
//   Frame::GetFeaturesInArea (Frame.cpp:641-694) and ComputeThreeMaxima (ORBmatcher.cpp:2097-2138).
// It projects by pose and checks rotations like the motion-model matcher (k_search_last.hip), and like the local-map matcher (k_search_local.hip) a
// point's keypoint is hidden from every LATER point (CurrentFrame.mvpMapPoints[bestIdx2] = pMP, tested at :2037).  The distance gate and the predicted
// level come per point, with K16's arithmetic (k16_gate / k16_level, shared with k_is_in_frustum).  Here:
//   k_kf_candidates  SL_LANES lanes per point: K14's projection, K16's gate and level, the window's cells in the reference's order (ix outer, iy inner,
//                    a cell's items ascending: the CSR position grows with the walk), the level / window / blocked_in filters and the Hamming
//                    distance; the first SK_CAP survivors are written as distance << 18 | CSR position in that order, and the count of all of them.
//                    The reference's strict-< best over any subset of the survivors is the minimum key of the subset.
//   k_kf_resolve     one workgroup: the claim rule as the fixed point k_local_resolve runs (claim_resolve, k_search_common.h).  Every round each
//                    point takes its minimum key over the candidates no point j < i claimed in the previous round (a match iff its distance <=
//                    orb_dist).  A point with more than SK_CAP survivors walks its window again, serially, in the same order.  Then the rotation histogram (one
//                    entry per matched point: a keypoint is matched at most once), ComputeThreeMaxima, and the cull - after every claim, as the
//                    reference culls after its loop: a culled keypoint stayed hidden from the later points.
// The contract (include/jsorb.h, jsorb_search_by_projection_kf_async) is restated in numpy in tests/test_search_kf_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef SK_CAP
#define SK_CAP 128                               // keys kept per point (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#ifndef SK_LDS_CLAIMS
#define SK_LDS_CLAIMS 16384                      // k_kf_resolve keeps claim[] in LDS up to this many keypoints (64 KiB; a test build lowers it)
#endif
#define SK_POS ((1 << 18) - 1)
#define SK_KEY(d, j) ((d) << 18 | (j))           // distance <= 256, CSR position < 2^18

int search_kf_cap() { return SK_CAP; }
int search_kf_lds_claims() { return SK_LDS_CLAIMS; }

// the window of point i: projection, gate, level, radius and GetFeaturesInArea(u, v, R, L-1, L+1)'s cell range; false: no candidate at all
struct KfPoint {
    float u, v, R;
    int L, x0, x1, y0, y1;
};
__device__ __forceinline__ bool kf_point(const SearchKfArgs &a, int i, KfPoint &w)
{
    const jsorb_kf_projection_params &p = a.p;
    const float x = a.Px[i], y = a.Py[i], z = a.Pz[i];
    float invz;
    if (!k14_project(p.Rcw, p.tcw, x, y, z, p.fx, p.fy, p.cx, p.cy, p.min_x, p.max_x, p.min_y, p.max_y, w.u, w.v, invz)) return false;
    float ox, oy, oz, dist;
    if (!k16_gate(p.Ow, x, y, z, a.min_dist_inv + i, a.max_dist_inv + i, ox, oy, oz, dist)) return false;
    w.L = k16_level(a.max_distance[i], dist, p.log_scale_factor, a.f.n_levels);
    w.R = p.th * a.f.scale[w.L];                       // radius = th * mvScaleFactors[nPredictedLevel], one float product
    return sl_cells(p, w.u, w.v, w.R, w.x0, w.x1, w.y0, w.y1);
}

// the item at CSR position j as a candidate of the point: -1 if a filter drops it, else its key
__device__ __forceinline__ int kf_candidate(const SearchKfArgs &a, const KfPoint &w, uint4 mlo, uint4 mhi, int j)
{
    const FrameView &f = a.f;
    const int k = f.cell_items[j];
    const int oct = f.octave(k);
    if (oct < w.L - 1 || oct > w.L + 1) return -1;
    if (!(fabsf(f.x(k) - w.u) < w.R && fabsf(f.y(k) - w.v) < w.R)) return -1;
    if (f.blocked && f.blocked[k]) return -1;          // CurrentFrame.mvpMapPoints[k] before the call
    uint4 lo, hi;
    sl_load_desc(f.desc + 32 * (size_t)k, lo, hi);
    const int d = SL_HAMMING(lo, hi, mlo, mhi);
    return SK_KEY(d, j);
}

__global__ __launch_bounds__(256) void k_kf_candidates(SearchKfArgs a)
{
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    if (i >= a.n_points) return;                     // (whole groups of SL_LANES lanes leave together)
    KfPoint w;
    if (!kf_point(a, i, w)) {                        // uniform across the lanes of a point
        if (lane == 0) a.cand_n[i] = 0;
        return;
    }
    uint4 mlo, mhi;
    sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
    const int count = compact_window<SK_CAP>(a.f.cell_start, a.p.rows, w.x0, w.x1, w.y0, w.y1, a.cand + (size_t)i * SK_CAP,
                                             [&](int j) { return kf_candidate(a, w, mlo, mhi, j); });
    if (lane == 0) a.cand_n[i] = count;
}

// the best of point i over the candidates no point j < i claims: ORBmatcher.cpp:2031-2051 (strict < updates from 256, a match iff bestDist <= ORBdist)
__device__ void kf_best(const SearchKfArgs &a, const int *claim, int i, int &match, int &match_dist)
{
    int best = INT_MAX;
    const int cnt = a.cand_n[i];
    if (cnt <= SK_CAP) {
        const int *l = a.cand + (size_t)i * SK_CAP;
        for (int t = 0; t < cnt; t++) {
            const int c = l[t];
            if (claim[a.f.cell_items[c & SK_POS]] >= i) best = min(best, c);      // (< i: CurrentFrame.mvpMapPoints[k] = an earlier point of this call)
        }
    } else {                                         // overflow: walk the window again, serially, in the same order
        KfPoint w;
        kf_point(a, i, w);
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        walk_window<false>(a.f.cell_start, a.p.rows, w.x0, w.x1, w.y0, w.y1, 0, 1, [&](int j, bool) {
            const int c = kf_candidate(a, w, mlo, mhi, j);
            if (c >= 0 && claim[a.f.cell_items[j]] >= i) best = min(best, c);
        });
    }
    match = -1;
    match_dist = -1;
    const int d = best >> 18;
    if (d < 256 && d <= a.p.orb_dist) {
        match = a.f.cell_items[best & SK_POS];
        match_dist = d;
    }
}

// One workgroup.  claim: LDS when the frame's keypoints fit (dynamic LDS of n_kp ints), else kp_match itself in global memory.
__global__ __launch_bounds__(1024) void k_kf_resolve(SearchKfArgs a, int claim_in_lds)
{
    extern __shared__ int s_claim[];
    __shared__ int s_hist[HISTO_LENGTH + 1], s_keep[HISTO_LENGTH + 1], s_count, s_culled;
    const int tid = threadIdx.x, n = a.n_points;
    const bool rot = a.p.check_orientation != 0;
    if (tid <= HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) { s_count = 0; s_culled = 0; }
    claim_resolve<SK_CAP>(claim_in_lds ? s_claim : a.kp_match, n, a.f.n_kp, a.cand_n, a.match_kp, a.match_dist, a.kp_match, a.stats,
                          [&](const int *claim, int i, int &m, int &d) { kf_best(a, claim, i, m, d); });
    // the fixed point: claim[match_kp[i]] == i for every matched point.  kp_match before the cull, the histogram over the matched points
    int matched = 0;
    for (int i = tid; i < n; i += 1024) {
        const int m = a.match_kp[i];
        if (m < 0) continue;
        matched++;
        if (rot) atomicAdd(&s_hist[rot_bin(a.angle[i], a.f.angle(m))], 1);      // rotHist[bin].push_back(bestIdx2)
    }
    atomicAdd(&s_count, matched);
    __syncthreads();
    if (tid == 0) {
        const ThreeMaxima t = rot_keep(s_hist, s_keep, rot);
        a.stats[3] = t.ind1; a.stats[4] = t.ind2; a.stats[5] = t.ind3;
    }
    __syncthreads();
    int culled = 0;
    if (rot)
        for (int i = tid; i < n; i += 1024) {
            const int m = a.match_kp[i];
            if (m >= 0 && !s_keep[rot_bin(a.angle[i], a.f.angle(m))]) {      // CurrentFrame.mvpMapPoints[rotHist[i][j]] = NULL; nmatches--
                a.kp_match[m] = -1;
                culled++;
            }
        }
    atomicAdd(&s_culled, culled);
    __syncthreads();
    if (tid == 0) *a.n_matches = s_count - s_culled;
}

void launch_kf_candidates(const SearchKfArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_kf_candidates, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_kf_resolve(const SearchKfArgs &a, hipStream_t s)
{
    const int lds = a.f.n_kp <= SK_LDS_CLAIMS;
    hipLaunchKernelGGL(k_kf_resolve, dim3(1), dim3(1024), lds ? (size_t)a.f.n_kp * sizeof(int) : 0, s, a, lds);
}

} // namespace jsorb
