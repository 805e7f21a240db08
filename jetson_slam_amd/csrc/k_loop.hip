// k_loop.hip - the matchers of LoopClosing::ComputeSim3 (LoopClosing.cpp:238-410) on the device:
//   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cpp:509-642) with ComputeThreeMaxima (:2097-2138), the current keyframe against
//     several loop candidates in one call: k_bow_group (k_bow.hip), k_loop_bow_match, k_tri_resolve (k_triangulate.hip: the same indexing)
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1089-1313) with KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage
//     (KeyFrame.cpp:573-617): k_fuse_grids (k_fuse.hip) per keyframe, k_sim3_match, k_sim3_agree
// k_loop_bow_match  one wave per (candidate, node present on both sides): the wave at the first position of a candidate's run finds KF1's run of the
//                   same node by bisection.  The search is k_search_common.h's node_walk with the roles of k_bow_match turned round: the single
//                   side (KF1) is the ordered outer walk (:541), the candidate's run the claimed side - the first LB_NODE_REGS entries of a lane
//                   in registers (!valid2 hides an entry at load), the rest read again for every KF1 keypoint with their vbMatched2, a byte per
//                   candidate keypoint in the matcher's scratch, written and read by the owning lane only; accepted at bestDist1 < th_low, strict.
//                   Every keypoint is in at most one node, so no two waves touch the same entry and no order of nodes can change a result.
// k_sim3_match      grid (blocks of 16 slots, direction); SL_LANES lanes take one (direction, slot): the two transformations here, then
//                   k_search_common.h's projected-window search, shared with k_fuse_match - proj_pixel and proj_cells around the K16 gate,
//                   window_best with the level as the only per-keypoint filter, block_totals for the statistics.  No claim rule.
// k_sim3_agree      one thread per i1 (:1294-1310), a block reduction for the count.  A launch of its own: it needs both directions complete.
// The contracts (include/jsorb.h, jsorb_search_by_bow_kf_async / jsorb_search_by_sim3_async) are restated in numpy in tests/test_loop_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef LB_NODE_REGS
#define LB_NODE_REGS 2                           // candidate entries of a node a lane of k_loop_bow_match keeps in registers (a test build lowers it: build.py VARIANTS)
#endif
static_assert(sizeof(Sim3Args) <= 4096 && sizeof(LoopBowArgs) <= 4096, "the kernels' arguments must fit a launch");

int loop_node_regs() { return LB_NODE_REGS; }

__global__ __launch_bounds__(256) void k_loop_bow_match(LoopBowArgs a)
{
    const int lane = threadIdx.x % 64, kf = blockIdx.y;
    const int p = blockIdx.x * 4 + threadIdx.x / 64;
    const int off = a.kf_start[kf], len = a.kf_start[kf + 1] - off;
    if (p >= len) return;                            // (wave-uniform, like every return below)
    const unsigned long long *ks = a.sorted2 + off;
    const unsigned long long head = ks[p];
    if (head == BW_NOKEY) return;
    const unsigned long long v = head >> BW_IDX;     // the node
    if (p > 0 && ks[p - 1] >> BW_IDX == v) return;   // not the first keypoint of the node: the wave at the first one takes them all
    const int fb = bw_lower_bound(a.sorted1, a.n1, v << BW_IDX), m1 = bw_lower_bound(a.sorted1, a.n1, (v + 1) << BW_IDX) - fb;
    if (m1 == 0) return;                             // the node is not in KF1's FeatureVector (:611-618)
    const int m = bw_lower_bound(ks, len, (v + 1) << BW_IDX) - p;
    const unsigned long long *cs = ks + p;           // the candidate's entries of the node, ascending index
    const unsigned long long *fs = a.sorted1 + fb;
    int32_t *row = a.match12 + (size_t)kf * a.n1;
    uint8_t *matched2 = a.matched2 + off;
    // the candidate's run is the claimed side (vbMatched2[idx2] || !valid2[idx2], :563-567; !valid2 hides a register entry at load), KF1's
    // keypoints of the node the outer walk (f1it->second in ascending index, :541)
    struct {
        const LoopBowArgs &a;
        const unsigned long long *cs, *fs;
        int32_t *row;
        uint8_t *matched2;
        int off;
        __device__ int index(int t) const { return (int)(cs[t] & BW_IDX_MASK); }
        __device__ const uint8_t *desc(int j) const { return a.desc2 + 32 * (size_t)(off + j); }
        __device__ bool hidden_at_load(int j) const { return !a.valid2[off + j]; }
        __device__ bool hidden_late(int j) const { return matched2[j] || !a.valid2[off + j]; }
        __device__ bool outer(int q, int &idx1, uint4 &lo, uint4 &hi) const
        {
            idx1 = (int)(fs[q] & BW_IDX_MASK);
            if (!a.valid1[idx1]) return false;       // !pMP1 || pMP1->isBad() (:545-549)
            sl_load_desc(a.desc1 + 32 * (size_t)idx1, lo, hi);
            return true;
        }
        __device__ bool accept(int d1) const { return d1 < a.p.th_low; }       // :585, strict
        __device__ void claim(int j, int idx1, bool late) const                // vpMatches12[idx1] = vpMapPoints2[bestIdx2], vbMatched2[bestIdx2] = true
        {
            if (late) matched2[j] = 1;
            row[idx1] = j;
        }
    } w{a, cs, fs, row, matched2, off};
    int n_dist = node_walk<LB_NODE_REGS>(w, lane, m, 0, m1, a.p.nn_ratio);
    for (int s = 32; s > 0; s >>= 1) n_dist += __shfl_xor(n_dist, s);
    if (lane == 0) {
        atomicAdd(&a.stats[0], 1);
        atomicAdd(&a.stats[1], n_dist);
        atomicMax(&a.stats[3], m);
    }
}

// the window of slot i of side S in the other keyframe: items 1-9 of the contract up to the cells; false: no candidate at all
__device__ __forceinline__ bool sim3_point(const jsorb_sim3_params &p, const Sim3Side &S, int i, ProjWindow &w)
{
    const float *T = S.T;
    const float x = S.Px[i], y = S.Py[i], z = S.Pz[i];
    // the keyframe's own camera, then the similarity into the other one: K14's rows
    const float ox = T[9] + rot_row(T, x, y, z);
    const float oy = T[10] + rot_row(T + 3, x, y, z);
    const float oz = T[11] + rot_row(T + 6, x, y, z);
    const float Pcx = T[21] + rot_row(T + 12, ox, oy, oz);
    const float Pcy = T[22] + rot_row(T + 15, ox, oy, oz);
    const float Pcz = T[23] + rot_row(T + 18, ox, oy, oz);
    float invz;
    if (!proj_pixel(p, Pcx, Pcy, Pcz, w, invz)) return false;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float dx, dy, dz, dist;
    if (!k16_gate(zero, Pcx, Pcy, Pcz, S.min_dist_inv + i, S.max_dist_inv + i, dx, dy, dz, dist)) return false;      // :1169, a NaN passes
    return proj_cells(p, S.max_distance[i], dist, w);                                             // :1176
}

__global__ __launch_bounds__(256) void k_sim3_match(Sim3Args a)
{
    const int lane = threadIdx.x % SL_LANES, dir = blockIdx.y;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    const Sim3Side &S = a.s[dir], &O = a.s[1 - dir];      // the searched side and the keyframe it is projected into
    const bool in_range = i < S.n;
    // every lane stays to the end (the reductions below take whole waves and the workgroup meets at a barrier)
    const bool live = in_range && S.search[i] != 0;
    ProjWindow w;
    const bool win = live && sim3_point(a.p, S, i, w);   // uniform across the lanes of a slot
    int sum[3] = {win && lane == 0 ? 1 : 0, 0, 0}, window;                               // slots with a window, keypoints walked, distances
    const unsigned key = window_best(win, w, O.cell_start, a.p.rows, O.cell_items, O.x, O.y, O.octave, O.kp_desc, S.mp_desc + 32 * (size_t)i,
                                     [](int, float, float, int) { return true; }, sum[1], sum[2], window);      // :1194-1201: the level alone
    if (lane == 0 && in_range) {
        const bool m = key != ~0u && (int)(key >> 18) <= a.p.th_high;                    // :1208
        S.match[i] = m ? O.cell_items[(int)(key & PW_POS)] : -1;
    }
    block_totals(sum, window);
    if (threadIdx.x == 0) {
        if (sum[0]) atomicAdd(&a.stats[0], sum[0]);
        if (sum[1]) atomicAdd(&a.stats[1], sum[1]);
        if (sum[2]) atomicAdd(&a.stats[2], sum[2]);
        if (window) atomicMax(&a.stats[3], window);
    }
}

__global__ __launch_bounds__(256) void k_sim3_agree(Sim3Args a)
{
    __shared__ int s_found;
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    int found = 0;
    if (i1 < a.s[0].n) {
        const int idx2 = a.s[0].match[i1];           // an index of keyframe 2's CSR items: in [0, n2), or -1
        const bool m = idx2 >= 0 && a.s[1].match[idx2] == i1;
        a.match12[i1] = m ? idx2 : -1;
        found = m;
    }
    for (int s = 32; s > 0; s >>= 1) found += __shfl_xor(found, s);
    if (threadIdx.x % 64 == 0 && found) atomicAdd(&s_found, found);
    __syncthreads();
    if (threadIdx.x == 0 && s_found) {
        atomicAdd(a.n_found, s_found);
        atomicAdd(&a.stats[4], s_found);
    }
}

void launch_loop_bow_match(const LoopBowArgs &a, hipStream_t s)
{
    int longest = 0;
    for (int i = 0; i < a.n_kf; i++) longest = max(longest, a.kf_start[i + 1] - a.kf_start[i]);
    if (longest <= 0 || a.n1 <= 0) return;
    hipLaunchKernelGGL(k_loop_bow_match, dim3((longest + 3) / 4, a.n_kf), dim3(256), 0, s, a);
}

void launch_sim3_match(const Sim3Args &a, hipStream_t s)
{
    const int n = max(a.s[0].n, a.s[1].n), per_block = 256 / SL_LANES;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sim3_match, dim3((n + per_block - 1) / per_block, 2), dim3(256), 0, s, a);
}

void launch_sim3_agree(const Sim3Args &a, hipStream_t s)
{
    if (a.s[0].n <= 0) return;
    hipLaunchKernelGGL(k_sim3_agree, dim3((a.s[0].n + 255) / 256), dim3(256), 0, s, a);
}

} // namespace jsorb
