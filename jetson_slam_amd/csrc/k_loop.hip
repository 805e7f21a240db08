// k_loop.hip - the matchers of LoopClosing::ComputeSim3 (LoopClosing.cpp:238-410) on the device:
//   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cpp:509-642) with ComputeThreeMaxima (:2097-2138), the current keyframe against
//     several loop candidates in one call: k_bow_group (k_bow.hip), k_loop_bow_match, k_tri_resolve (k_triangulate.hip: the same indexing)
//   ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1089-1313) with KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage
//     (KeyFrame.cpp:573-617): k_fuse_grids (k_fuse.hip) per keyframe, k_sim3_match, k_sim3_agree
// k_loop_bow_match  one wave per (candidate, node present on both sides): the wave at the first position of a candidate's run finds KF1's run of the
//                   same node by bisection.  The roles are the reverse of k_bow_match: the single side (KF1) is the ordered outer walk (:541), the
//                   candidate is the claimed side.  Lane l owns the candidate entries l, l + 64, ...: the first LB_NODE_REGS of them with their
//                   descriptor and a claimed bit in registers (!valid2 is folded into the bit at load), the rest read again for every KF1 keypoint -
//                   their vbMatched2 is a byte per candidate keypoint in the matcher's scratch, written and read by the owning lane only.  The wave
//                   reduces to (bestDist1, first position with it, bestDist2) and the owner of the winning entry claims it and writes match12.
//                   Every keypoint is in at most one node, so no two waves touch the same entry and no order of nodes can change a result.
// k_sim3_match      grid (blocks of 16 slots, direction); SL_LANES lanes take one (direction, slot): the two transformations, the gates, the level
//                   and the window's cells once (uniform over the lanes), then the window's CSR positions lane, lane + SL_LANES, ... in the ONE walk
//                   order (walk_window).  Every lane keeps the minimum of distance << 18 | CSR position; the minimum over the lanes (shuffles) is
//                   the reference's strict-< best.  No claim rule, no LDS on that path.
// k_sim3_agree      one thread per i1 (:1294-1310), a block reduction for the count.  A launch of its own: it needs both directions complete.
// The contracts (include/jsorb.h, jsorb_search_by_bow_kf_async / jsorb_search_by_sim3_async) are restated in numpy in tests/test_loop_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef LB_NODE_REGS
#define LB_NODE_REGS 2                           // candidate entries of a node a lane of k_loop_bow_match keeps in registers (a test build lowers it: build.py VARIANTS)
#endif
#define S3_POS ((1u << 18) - 1)
static_assert(LB_NODE_REGS >= 1 && LB_NODE_REGS <= 8, "the claimed bits of a lane's register entries");
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
    // the lane's first entries: index, descriptor; claimed = vbMatched2[idx2] || !valid2[idx2], or no entry at all
    int kreg[LB_NODE_REGS];
    uint4 rlo[LB_NODE_REGS], rhi[LB_NODE_REGS];
    unsigned claimed = 0;
#pragma unroll
    for (int r = 0; r < LB_NODE_REGS; r++) {
        const int t = lane + 64 * r;
        kreg[r] = t < m ? (int)(cs[t] & BW_IDX_MASK) : -1;
        if (t < m) {
            sl_load_desc(a.desc2 + 32 * (size_t)(off + kreg[r]), rlo[r], rhi[r]);
            if (!a.valid2[off + kreg[r]]) claimed |= 1u << r;
        } else {
            rlo[r] = make_uint4(0, 0, 0, 0); rhi[r] = rlo[r];
            claimed |= 1u << r;
        }
    }
    const float ratio = a.p.nn_ratio;
    int n_dist = 0;
    for (int q = 0; q < m1; q++) {                   // f1it->second in ascending index (:541)
        const int idx1 = (int)(fs[q] & BW_IDX_MASK);
        if (!a.valid1[idx1]) continue;               // !pMP1 || pMP1->isBad() (:545-549)
        uint4 klo, khi;
        sl_load_desc(a.desc1 + 32 * (size_t)idx1, klo, khi);
        // bestDist1 / bestDist2 from 256 over the entries not yet matched (:553-583): the two smallest of the multiset, the first position with the smallest
        int d1 = 256, d2 = 256;
        unsigned best = ~0u;
        auto take = [&](int d, int t) {
            n_dist++;
            if (d < d1) {                            // a lane meets its entries in ascending position: a tie never replaces
                d2 = d1; d1 = d;
                best = (unsigned)d << BW_IDX | (unsigned)t;
            } else if (d < d2) {
                d2 = d;
            }
        };
#pragma unroll
        for (int r = 0; r < LB_NODE_REGS; r++)
            if (!(claimed >> r & 1)) take(SL_HAMMING(rlo[r], rhi[r], klo, khi), lane + 64 * r);
        for (int t = lane + 64 * LB_NODE_REGS; t < m; t += 64) {
            const int j = (int)(cs[t] & BW_IDX_MASK);
            if (matched2[j] || !a.valid2[off + j]) continue;      // :563-567; the byte is written by this lane, if at all
            uint4 lo, hi;
            sl_load_desc(a.desc2 + 32 * (size_t)(off + j), lo, hi);
            take(SL_HAMMING(lo, hi, klo, khi), t);
        }
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned ob = (unsigned)__shfl_xor((int)best, s);
            const int o1 = __shfl_xor(d1, s), o2 = __shfl_xor(d2, s);
            d2 = min(max(d1, o1), min(d2, o2));
            d1 = min(d1, o1);
            best = min(best, ob);
        }
        if (best == ~0u || !(d1 < a.p.th_low) || !((float)d1 < ratio * (float)d2)) continue;      // :585-587, the first one strict
        const int t = (int)(best & BW_IDX_MASK);
        if (t % 64 == lane) {                        // the owner of the entry: vpMatches12[idx1] = vpMapPoints2[bestIdx2], vbMatched2[bestIdx2] = true
            int j = -1;
#pragma unroll
            for (int r = 0; r < LB_NODE_REGS; r++)
                if (t == lane + 64 * r) { j = kreg[r]; claimed |= 1u << r; }
            if (j < 0) {
                j = (int)(cs[t] & BW_IDX_MASK);
                matched2[j] = 1;
            }
            row[idx1] = j;
        }
    }
    for (int s = 32; s > 0; s >>= 1) n_dist += __shfl_xor(n_dist, s);
    if (lane == 0) {
        atomicAdd(&a.stats[0], 1);
        atomicAdd(&a.stats[1], n_dist);
        atomicMax(&a.stats[3], m);
    }
}

// the window of slot i of side S in the other keyframe: items 1-9 of the contract up to the cells; false: no candidate at all
struct Sim3Window {
    float u, v, R;
    int L, x0, x1, y0, y1;
};
__device__ __forceinline__ bool sim3_point(const jsorb_sim3_params &p, const Sim3Side &S, int i, Sim3Window &w)
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
    if (!(Pcz > 0.0f)) return false;
    const float invz = 1.0f / Pcz;
    w.u = __builtin_fmaf(Pcx * p.fx, invz, p.cx);
    w.v = __builtin_fmaf(Pcy * p.fy, invz, p.cy);
    if (!(w.u >= p.min_x && w.u < p.max_x && w.v >= p.min_y && w.v < p.max_y)) return false;      // KeyFrame::IsInImage, half open; a NaN fails
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    float dx, dy, dz, dist;
    if (!k16_gate(zero, Pcx, Pcy, Pcz, S.min_dist_inv + i, S.max_dist_inv + i, dx, dy, dz, dist)) return false;      // :1169, a NaN passes
    w.L = k16_level(S.max_distance[i], dist, p.log_scale_factor, p.n_levels);
    w.R = p.th * p.scale_factor[w.L];                                                             // :1176, one float product
    return sl_cells(p, w.u, w.v, w.R, w.x0, w.x1, w.y0, w.y1);
}

__global__ __launch_bounds__(256) void k_sim3_match(Sim3Args a)
{
    __shared__ int s_part[4][4];
    const int lane = threadIdx.x % SL_LANES, dir = blockIdx.y;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    const Sim3Side &S = a.s[dir], &O = a.s[1 - dir];      // the searched side and the keyframe it is projected into
    const bool in_range = i < S.n;
    // every lane stays to the end (the reductions below take whole waves and the workgroup meets at a barrier)
    const bool live = in_range && S.search[i] != 0;
    Sim3Window w;
    const bool win = live && sim3_point(a.p, S, i, w);   // uniform across the lanes of a slot
    unsigned key = ~0u;
    int walked = 0, n_dist = 0;
    if (win) {
        uint4 mlo, mhi;
        sl_load_desc(S.mp_desc + 32 * (size_t)i, mlo, mhi);
        walk_window<true>(O.cell_start, a.p.rows, w.x0, w.x1, w.y0, w.y1, lane, SL_LANES, [&](int j, bool in) {
            if (!in) return;
            walked++;
            const int k = O.cell_items[j];
            if (!(fabsf(O.x[k] - w.u) < w.R && fabsf(O.y[k] - w.v) < w.R)) return;      // KeyFrame.cpp:602-606
            const int oct = O.octave[k];
            if (oct < w.L - 1 || oct > w.L) return;                                      // :1194
            uint4 lo, hi;
            sl_load_desc(O.kp_desc + 32 * (size_t)k, lo, hi);
            const int d = SL_HAMMING(lo, hi, mlo, mhi);
            n_dist++;
            key = min(key, (unsigned)d << 18 | (unsigned)j);                             // :1201, strict <: the first in walk order wins a tie
        });
    }
    int window = walked;
    for (int s = SL_LANES / 2; s > 0; s >>= 1) {
        key = min(key, (unsigned)__shfl_xor((int)key, s, SL_LANES));
        window += __shfl_xor(window, s, SL_LANES);
    }
    if (lane == 0 && in_range) {
        const bool m = key != ~0u && (int)(key >> 18) <= a.p.th_high;                    // :1208
        S.match[i] = m ? O.cell_items[(int)(key & S3_POS)] : -1;
    }
    int pairs = win && lane == 0 ? 1 : 0;
    for (int s = 32; s > 0; s >>= 1) {
        pairs += __shfl_xor(pairs, s);
        walked += __shfl_xor(walked, s);
        n_dist += __shfl_xor(n_dist, s);
        window = max(window, __shfl_xor(window, s));
    }
    if (threadIdx.x % 64 == 0) {
        int *q = s_part[threadIdx.x / 64];
        q[0] = pairs; q[1] = walked; q[2] = n_dist; q[3] = window;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; v++) {
            pairs += s_part[v][0]; walked += s_part[v][1]; n_dist += s_part[v][2];
            window = max(window, s_part[v][3]);
        }
        if (pairs) atomicAdd(&a.stats[0], pairs);
        if (walked) atomicAdd(&a.stats[1], walked);
        if (n_dist) atomicAdd(&a.stats[2], n_dist);
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
