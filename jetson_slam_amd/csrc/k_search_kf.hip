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
//   k_kf_resolve     one workgroup: the claim rule as the fixed point k_local_resolve runs.  Every round each point takes its minimum key over the
//                    candidates no point j < i claimed in the previous round (a match iff its distance <= orb_dist), then claim[k] = min i whose
//                    choice is k.  Point i depends only on the choices of j < i, so after round r the points < r are final: at most n + 1 rounds.  A
//                    point with more than SK_CAP survivors walks its window again, serially, in the same order.  Then the rotation histogram (one
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
#define SL_LANES 16                              // lanes per point (4 points per wave), as k_local_candidates
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
    w.L = k16_level(a.max_distance[i], dist, p.log_scale_factor, a.n_levels);
    w.R = p.th * a.scale[w.L];                       // radius = th * mvScaleFactors[nPredictedLevel], one float product
    return sl_cells(p, w.u, w.v, w.R, w.x0, w.x1, w.y0, w.y1);
}

// the item at CSR position j as a candidate of the point: -1 if a filter drops it, else its key
__device__ __forceinline__ int kf_candidate(const SearchKfArgs &a, const KfPoint &w, uint4 mlo, uint4 mhi, int j)
{
    const int n = a.n_kp, k = a.cell_items[j];
    const int oct = a.soa[4 * (size_t)n + k];
    if (oct < w.L - 1 || oct > w.L + 1) return -1;
    const float kx = a.xy_un ? a.xy_un[k] : (float)a.soa[k];
    const float ky = a.xy_un ? a.xy_un[n + k] : (float)a.soa[n + k];
    if (!(fabsf(kx - w.u) < w.R && fabsf(ky - w.v) < w.R)) return -1;
    if (a.blocked && a.blocked[k]) return -1;          // CurrentFrame.mvpMapPoints[k] before the call
    uint4 lo, hi;
    sl_load_desc(a.desc + 32 * (size_t)k, lo, hi);
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
    const int shift = threadIdx.x % 64 / SL_LANES * SL_LANES;
    int *out = a.cand + (size_t)i * SK_CAP;
    int count = 0;
    for (int ix = w.x0; ix <= w.x1; ix++) {
        const int b = a.cell_start[ix * a.p.rows + w.y0], e = a.cell_start[ix * a.p.rows + w.y1 + 1];
        for (int base = b; base < e; base += SL_LANES) {
            const int j = base + lane;
            const int c = j < e ? kf_candidate(a, w, mlo, mhi, j) : -1;
            const unsigned m = (unsigned)(__ballot(c >= 0) >> shift) & ((1u << SL_LANES) - 1);
            const int pos = count + __popc(m & ((1u << lane) - 1));
            if (c >= 0 && pos < SK_CAP) out[pos] = c;
            count += __popc(m);
        }
    }
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
            if (claim[a.cell_items[c & SK_POS]] >= i) best = min(best, c);      // (< i: CurrentFrame.mvpMapPoints[k] = an earlier point of this call)
        }
    } else {                                         // overflow: walk the window again, serially, in the same order
        KfPoint w;
        kf_point(a, i, w);
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        for (int ix = w.x0; ix <= w.x1; ix++) {
            const int b = a.cell_start[ix * a.p.rows + w.y0], e = a.cell_start[ix * a.p.rows + w.y1 + 1];
            for (int j = b; j < e; j++) {
                const int c = kf_candidate(a, w, mlo, mhi, j);
                if (c >= 0 && claim[a.cell_items[j]] >= i) best = min(best, c);
            }
        }
    }
    match = -1;
    match_dist = -1;
    const int d = best >> 18;
    if (d < 256 && d <= a.p.orb_dist) {
        match = a.cell_items[best & SK_POS];
        match_dist = d;
    }
}

// One workgroup.  claim: LDS when the frame's keypoints fit (dynamic LDS of n_kp ints), else kp_match itself in global memory.
__global__ __launch_bounds__(1024) void k_kf_resolve(SearchKfArgs a, int claim_in_lds)
{
    extern __shared__ int s_claim[];
    __shared__ int s_hist[LF_BINS + 1], s_keep[LF_BINS + 1], s_count, s_cand, s_over, s_culled;
    const int tid = threadIdx.x, n = a.n_points, N = a.n_kp;
    const bool rot = a.p.check_orientation != 0;
    int *claim = claim_in_lds ? s_claim : a.kp_match;
    if (tid <= LF_BINS) s_hist[tid] = 0;
    if (tid == 0) { s_count = 0; s_cand = 0; s_over = 0; s_culled = 0; }
    for (int k = tid; k < N; k += 1024) claim[k] = INT_MAX;
    int cand = 0, over = 0;
    for (int i = tid; i < n; i += 1024) {
        a.match_kp[i] = -2;                          // no choice yet: the first round changes every point
        const int c = a.cand_n[i];
        cand += c;
        over += c > SK_CAP;
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
            kf_best(a, claim, i, m, d);
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
    // the fixed point: claim[match_kp[i]] == i for every matched point.  kp_match before the cull, the histogram over the matched points
    int matched = 0;
    for (int i = tid; i < n; i += 1024) {
        const int m = a.match_kp[i];
        if (m < 0) continue;
        matched++;
        if (rot) atomicAdd(&s_hist[lf_bin(a.angle[i], __int_as_float(a.soa[3 * (size_t)N + m]))], 1);      // rotHist[bin].push_back(bestIdx2)
    }
    for (int k = tid; k < N; k += 1024) {
        const int c = claim[k];
        a.kp_match[k] = c == INT_MAX ? -1 : c;
    }
    atomicAdd(&s_count, matched);
    __syncthreads();
    if (tid == 0) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        if (rot) three_maxima(s_hist, ind1, ind2, ind3);
        for (int b = 0; b <= LF_BINS; b++) s_keep[b] = !rot || b == ind1 || b == ind2 || b == ind3;
        a.stats[3] = ind1; a.stats[4] = ind2; a.stats[5] = ind3;
    }
    __syncthreads();
    int culled = 0;
    if (rot)
        for (int i = tid; i < n; i += 1024) {
            const int m = a.match_kp[i];
            if (m >= 0 && !s_keep[lf_bin(a.angle[i], __int_as_float(a.soa[3 * (size_t)N + m]))]) {      // CurrentFrame.mvpMapPoints[rotHist[i][j]] = NULL; nmatches--
                a.kp_match[m] = -1;
                culled++;
            }
        }
    atomicAdd(&s_culled, culled);
    __syncthreads();
    if (tid == 0) {
        *a.n_matches = s_count - s_culled;
        a.stats[0] = rounds;
        a.stats[1] = s_cand;
        a.stats[2] = s_over;
    }
}

void launch_kf_candidates(const SearchKfArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_kf_candidates, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_kf_resolve(const SearchKfArgs &a, hipStream_t s)
{
    const int lds = a.n_kp <= SK_LDS_CLAIMS;
    hipLaunchKernelGGL(k_kf_resolve, dim3(1), dim3(1024), lds ? (size_t)a.n_kp * sizeof(int) : 0, s, a, lds);
}

} // namespace jsorb
