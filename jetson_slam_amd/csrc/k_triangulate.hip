// k_triangulate.hip - the matcher of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:216-274) on the device:
//   ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cpp:644-810) with CheckDistEpipolarLine (:127-144)
//   and ComputeThreeMaxima (:2097-2138), one keyframe KF1 against several neighbours KF2 in one call.
// In this reference vbMatched2 (:664) is read (:712) and never set: the result of a KF1 keypoint depends on no other KF1 keypoint, two of them may
// take the same KF2 keypoint and there is no sequential claim rule.  The kernels reproduce exactly that; an "exclusive" mode is out of scope.
// Grouping     k_bow_group (k_bow.hip, as it is; its key layout and bisection are k_search_common.h's BW_IDX / bw_lower_bound): KF1 is the frame side of a BowMatchArgs, the KF2s are its keyframe sides - the keys
//              node << 18 | index sorted ascending, a node's keypoints one run in ascending index.
// k_tri_match  grid (positions of KF1's sorted keys, keyframe of the launch's chunk); TR_LANES lanes take one sorted KF1 position: its descriptor,
//              point and flags once, the KF2 run of its node by bisection, the epipolar line a, b, c once.  The lanes take the run's entries
//              lane, lane + TR_LANES, ...: flags before the descriptor, the distance before the geometry.  Every lane keeps the minimum of
//              d << 18 | (BW_IDX_MASK - t) over the entries that pass the geometry (a lane meets its entries in ascending t, so a later equal d
//              is the smaller key and replaces the earlier one: the last position in walk order wins a tie, as `dist > bestDist` at :725 lets it);
//              the minimum over the lanes is the reference's winner.  An entry whose distance lies above the lane's best so far cannot win and
//              skips the line test, as :725 does in walk order.  No LDS, no barrier; the per-keyframe geometry (F12, epipole) comes in the launch
//              arguments, TR_KF_CHUNK keyframes per launch.
// k_tri_resolve one workgroup per keyframe: the rotation histogram over idx1, ComputeThreeMaxima, the culling and the count (:778-797):
//              k_search_common.h's row_resolve, shared with k_bow_resolve, with KF1's angle first.  It also resolves k_loop_bow_match's rows.
// The contract (include/jsorb.h, jsorb_search_for_triangulation_async) is restated in numpy in tests/test_triangulation_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#define TR_LANES 16                              // lanes per KF1 keypoint in k_tri_match (provisional: DESIGN.md section 16)
__global__ __launch_bounds__(256) void k_tri_match(TriArgs a, TriGeom g)
{
    const int lane = threadIdx.x % TR_LANES, kf = g.kf0 + blockIdx.y;
    const int p = blockIdx.x * (256 / TR_LANES) + threadIdx.x / TR_LANES;
    const int off = a.kf_start[kf], len = a.kf_start[kf + 1] - off;
    const float *G = g.f[blockIdx.y];                // F12 row-major, ex, ey
    // every lane stays to the end (the reductions below take whole waves); a group's trip count is uniform
    const unsigned long long k1 = p < a.n1 && len > 0 ? a.sorted1[p] : BW_NOKEY;
    const bool in_node = k1 != BW_NOKEY;
    const unsigned long long v = k1 >> BW_IDX;       // the node
    const int idx1 = (int)(k1 & BW_IDX_MASK);
    const bool head = in_node && (p == 0 || a.sorted1[p - 1] >> BW_IDX != v);      // the first KF1 keypoint of the node: it counts the pair
    bool stereo1 = false, take = false;
    if (in_node) {
        stereo1 = a.stereo1[idx1] != 0;
        take = a.free1[idx1] != 0 && (!a.only_stereo || stereo1);                  // :686-696
    }
    const unsigned long long *ks = a.sorted2 + off;
    int fb = 0, m = 0;
    if (head || take) {
        fb = bw_lower_bound(ks, len, v << BW_IDX);
        m = bw_lower_bound(ks, len, (v + 1) << BW_IDX) - fb;
    }
    unsigned key = ~0u;
    int n_dist = 0, n_line = 0;
    if (take && m > 0) {
        uint4 lo, hi;
        sl_load_desc(a.desc1 + 32 * (size_t)idx1, lo, hi);
        const float x1 = a.x1[idx1], y1 = a.y1[idx1];
        // :130-136, left to right, separate multiplies and adds
        const float la = x1 * G[0] + y1 * G[3] + G[6];
        const float lb = x1 * G[1] + y1 * G[4] + G[7];
        const float lc = x1 * G[2] + y1 * G[5] + G[8];
        const float den = la * la + lb * lb;
        const float ex = G[9], ey = G[10];
        for (int t = lane; t < m; t += TR_LANES) {
            const int j = off + (int)(ks[fb + t] & BW_IDX_MASK);
            if (!a.free2[j]) continue;                                             // :712
            const bool stereo2 = a.stereo2[j] != 0;
            if (a.only_stereo && !stereo2) continue;                               // :717-719
            uint4 mlo, mhi;
            sl_load_desc(a.desc2 + 32 * (size_t)j, mlo, mhi);
            const int d = SL_HAMMING(lo, hi, mlo, mhi);
            n_dist++;
            if (d > a.th_low) continue;                                            // :725 (bestDist starts at TH_LOW and only falls)
            const int oct = a.octave2[j];
            if ((unsigned)oct >= (unsigned)a.n_levels) continue;                   // defined here: the entry never passes
            const float x2 = a.x2[j], y2 = a.y2[j];
            if (!stereo1 && !stereo2) {                                            // :730-736
                const float distex = ex - x2, distey = ey - y2;
                if (distex * distex + distey * distey < a.gate[oct]) continue;
            }
            n_line++;
            if ((unsigned)d > key >> BW_IDX) continue;                             // above the lane's best: it cannot win
            const float num = la * x2 + lb * y2 + lc;
            if (den == 0) continue;                                                // :138
            const float dsqr = num * num / den;
            if (!((double)dsqr < a.line[oct])) continue;                           // :143, a double comparison; a NaN rejects
            key = min(key, (unsigned)d << BW_IDX | (BW_IDX_MASK - (unsigned)t));
        }
    }
    for (int s = TR_LANES / 2; s > 0; s >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, s, TR_LANES));
    if (lane == 0 && key != ~0u)                                                   // :745-748
        a.match12[(size_t)kf * a.n1 + idx1] = (int)(ks[fb + (int)(BW_IDX_MASK - (key & BW_IDX_MASK))] & BW_IDX_MASK);
    int pairs = head && m > 0 && lane == 0 ? 1 : 0, largest = head ? m : 0;
    for (int s = 32; s > 0; s >>= 1) {
        pairs += __shfl_xor(pairs, s);
        n_dist += __shfl_xor(n_dist, s);
        n_line += __shfl_xor(n_line, s);
        largest = max(largest, __shfl_xor(largest, s));
    }
    if (threadIdx.x % 64 == 0) {
        if (pairs) atomicAdd(&a.stats[0], pairs);
        if (n_dist) atomicAdd(&a.stats[1], n_dist);
        if (n_line) atomicAdd(&a.stats[2], n_line);
        if (largest) atomicMax(&a.stats[3], largest);
    }
}

__global__ __launch_bounds__(256) void k_tri_resolve(RowResolveArgs a)
{
    // :753-760 and :778-797; KF1's angle comes first (rot = angle1[idx1] - angle2[idx2])
    row_resolve(a, [&](int k, int j) { return rot_bin(a.row_angle[k], a.kf_angle[j]); }, a.kept, a.n);
}

void launch_tri_match(const TriArgs &a, const TriGeom &g, hipStream_t s)
{
    if (a.n1 <= 0 || g.n <= 0) return;
    const int per_block = 256 / TR_LANES;
    hipLaunchKernelGGL(k_tri_match, dim3((a.n1 + per_block - 1) / per_block, g.n), dim3(256), 0, s, a, g);
}

void launch_tri_resolve(const RowResolveArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_tri_resolve, dim3(a.n_kf), dim3(256), 0, s, a); }

} // namespace jsorb
