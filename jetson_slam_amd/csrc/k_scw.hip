// k_scw.hip - the matcher that decides whether LoopClosing::ComputeSim3 accepts a loop (LoopClosing.cpp:380) on the device:
//   ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
//   (ORBmatcher.cpp:277-390) with KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage (KeyFrame.cpp:573-617).
// The search of one point is Fuse(pKF, Scw, ...)'s (k_fuse_match with check_reprojection = 0: the same gates, the predicted level, the level window
// [L-1, L]).  What is new is state: a keypoint with vpMatched[idx] != NULL is hidden (:362), and a point that matches sets vpMatched[bestIdx] and so
// hides that keypoint from every LATER point (:383) - the claim rule k_kf_resolve and k_local_resolve solve as a fixed point, here without a
// rotation check.  The grid is k_fuse_grids' (k_fuse.hip) over the one keyframe.  Here:
//   k_scw_candidates  SL_LANES lanes per point: proj_pixel, the K16 gate with Ow and the normal test as k_fuse_match places them, proj_cells, then
//                     compact_window<SC_CAP> over the window in the ONE walk order; the filters drop the keypoints outside the window, the `blocked`
//                     ones and those outside [L-1, L].  A KEY IS KEPT ONLY WHEN ITS DISTANCE IS <= th_low.  That is exact: a point's result is the
//                     minimum key over its non-hidden candidates if that key's distance is <= th_low, and no match otherwise (:374, :381); a key above
//                     th_low can never be that minimum-with-a-match, and hiding keypoints only raises the minimum - if the minimum over the kept,
//                     non-hidden keys exists it is the minimum over all non-hidden candidates (every dropped key is larger), and if none exists
//                     every non-hidden candidate lies above th_low.  A point above th_low claims nothing (:381), so the dropped keys carry no
//                     state either.  It keeps the lists short (SC_CAP = 32) and makes overflow rare.  The count is that of all kept keys.
//   k_scw_resolve     one workgroup: claim_resolve<SC_CAP> unchanged.  Every round each point takes its minimum key over the kept keys whose
//                     keypoint no point j < i claimed in the previous round; a point with more than SC_CAP kept keys walks its window again,
//                     serially, in the same order and with the same filters.  claim[] in LDS up to SC_LDS_CLAIMS keypoints, in kp_match above that.
//                     Then the match count.  No histogram, no cull.
// The contract (include/jsorb.h, jsorb_search_by_projection_sim3_async) is restated in numpy in tests/test_search_scw_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef SC_CAP
#define SC_CAP 32                                // keys kept per point (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#ifndef SC_LDS_CLAIMS
#define SC_LDS_CLAIMS 16384                      // k_scw_resolve keeps claim[] in LDS up to this many keypoints (64 KiB; a test build lowers it)
#endif
#define SC_KEY(d, j) ((d) << 18 | (j))           // distance <= 255, CSR position < 2^18
static_assert(sizeof(ScwArgs) <= 4096, "the kernels' arguments must fit a launch");

int scw_cap() { return SC_CAP; }
int scw_lds_claims() { return SC_LDS_CLAIMS; }

// the window of point i: :311-349 with the contract's arithmetic (jsorb_fuse_async items 1, 2, 4-7); false: no candidate at all
__device__ __forceinline__ bool scw_point(const ScwArgs &a, int i, ProjWindow &w)
{
    const jsorb_scw_params &p = a.p;
    const float x = a.Px[i], y = a.Py[i], z = a.Pz[i];
    float invz;
    if (!proj_pixel(p, p.tcw[0] + rot_row(p.Rcw, x, y, z), p.tcw[1] + rot_row(p.Rcw + 3, x, y, z), p.tcw[2] + rot_row(p.Rcw + 6, x, y, z), w, invz)) return false;
    float ox, oy, oz, dist;
    if (!k16_gate(p.Ow, x, y, z, a.min_dist_inv + i, a.max_dist_inv + i, ox, oy, oz, dist)) return false;      // :335
    const float dot = __builtin_fmaf(oz, a.Nz[i], __builtin_fmaf(ox, a.Nx[i], oy * a.Ny[i]));
    if (dot < 0.5f * dist) return false;                                                          // :341, a NaN passes
    return proj_cells(p, a.max_distance[i], dist, w);                                             // :344-349
}

// the item at CSR position j as a candidate of the point: -1 if a filter drops it or its distance is above th_low, else its key
__device__ __forceinline__ int scw_candidate(const ScwArgs &a, const ProjWindow &w, uint4 mlo, uint4 mhi, int j, int &n_dist)
{
    const int k = a.cell_items[j];
    if (!(fabsf(a.x[k] - w.u) < w.R && fabsf(a.y[k] - w.v) < w.R)) return -1;      // KeyFrame.cpp:602-606
    if (a.blocked && a.blocked[k]) return -1;          // vpMatched[k] before the call (:362)
    const int oct = a.octave[k];
    if (oct < w.L - 1 || oct > w.L) return -1;         // :367
    uint4 lo, hi;
    sl_load_desc(a.kf_desc + 32 * (size_t)k, lo, hi);
    const int d = SL_HAMMING(lo, hi, mlo, mhi);
    n_dist++;
    return d <= a.p.th_low ? SC_KEY(d, j) : -1;
}

__global__ __launch_bounds__(256) void k_scw_candidates(ScwArgs a)
{
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    const bool in_range = i < a.n_points;
    // every lane stays to the end (the workgroup meets at block_totals' barrier)
    ProjWindow w;
    const bool win = in_range && scw_point(a, i, w);      // uniform across the lanes of a point
    int sum[2] = {win && lane == 0 ? 1 : 0, 0}, window = 0, count = 0;      // points with a window, distances
    if (win) {
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        count = compact_window<SC_CAP>(a.cell_start, a.p.rows, w.x0, w.x1, w.y0, w.y1, a.cand + (size_t)i * SC_CAP, [&](int j) {
            window++;
            return scw_candidate(a, w, mlo, mhi, j, sum[1]);
        });
    }
    for (int s = SL_LANES / 2; s > 0; s >>= 1) window += __shfl_xor(window, s, SL_LANES);      // the point's walked keypoints
    if (lane == 0 && in_range) a.cand_n[i] = count;
    block_totals(sum, window);
    if (threadIdx.x == 0) {
        if (sum[0]) atomicAdd(&a.stats[3], sum[0]);
        if (sum[1]) atomicAdd(&a.stats[4], sum[1]);
        if (window) atomicMax(&a.stats[5], window);
    }
}

// the best of point i over the kept keys no point j < i claims: :357-385 (strict < from 256 in walk order is the minimum key; every kept key matches)
__device__ void scw_best(const ScwArgs &a, const int *claim, int i, int &match, int &match_dist)
{
    int best = INT_MAX;
    const int cnt = a.cand_n[i];
    if (cnt <= SC_CAP) {
        const int *l = a.cand + (size_t)i * SC_CAP;
        for (int t = 0; t < cnt; t++) {
            const int c = l[t];
            if (claim[a.cell_items[c & PW_POS]] >= i) best = min(best, c);      // (< i: vpMatched[k] = an earlier point of this call)
        }
    } else {                                         // overflow: walk the window again, serially, in the same order
        ProjWindow w;
        scw_point(a, i, w);
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        int n_dist = 0;
        walk_window<false>(a.cell_start, a.p.rows, w.x0, w.x1, w.y0, w.y1, 0, 1, [&](int j, bool) {
            const int c = scw_candidate(a, w, mlo, mhi, j, n_dist);
            if (c >= 0 && claim[a.cell_items[j]] >= i) best = min(best, c);
        });
    }
    match = -1;
    match_dist = -1;
    if (best != INT_MAX) {                           // bestDist <= TH_LOW (:381): only such keys are kept
        match = a.cell_items[best & PW_POS];
        match_dist = best >> 18;
    }
}

// One workgroup.  claim: LDS when the keyframe's keypoints fit (dynamic LDS of n_kp ints), else kp_match itself in global memory.
__global__ __launch_bounds__(1024) void k_scw_resolve(ScwArgs a, int claim_in_lds)
{
    extern __shared__ int s_claim[];
    __shared__ int s_count;
    const int tid = threadIdx.x, n = a.n_points;
    if (tid == 0) s_count = 0;
    claim_resolve<SC_CAP>(claim_in_lds ? s_claim : a.kp_match, n, a.n_kp, a.cand_n, a.match_kp, a.match_dist, a.kp_match, a.stats,
                          [&](const int *claim, int i, int &m, int &d) { scw_best(a, claim, i, m, d); });
    // the fixed point: claim[match_kp[i]] == i for every matched point
    int matched = 0;
    for (int i = tid; i < n; i += 1024) matched += a.match_kp[i] >= 0;
    if (matched) atomicAdd(&s_count, matched);
    __syncthreads();
    if (tid == 0) *a.n_matches = s_count;            // nmatches (:384)
}

void launch_scw_candidates(const ScwArgs &a, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_scw_candidates, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_scw_resolve(const ScwArgs &a, hipStream_t s)
{
    const int lds = a.n_kp <= SC_LDS_CLAIMS;
    hipLaunchKernelGGL(k_scw_resolve, dim3(1), dim3(1024), lds ? (size_t)a.n_kp * sizeof(int) : 0, s, a, lds);
}

} // namespace jsorb
