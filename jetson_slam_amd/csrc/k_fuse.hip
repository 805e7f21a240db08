// k_fuse.hip - the matcher of LocalMapping::SearchInNeighbors (LocalMapping.cpp:460-540) and of loop closing on the device:
//   ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:812-962) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:964-1087), the search part
//   (:829-936) with KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage (KeyFrame.cpp:573-617), map points against several keyframes in one call.
// :839-936 are a pure function of (keyframe, point): no claim rule, no rotation check.  The head test (:833-837) and the tail (:938-958: Replace,
// AddObservation, AddMapPoint) touch the map and stay with the caller, who replays them over best_idx in the reference's order (include/jsorb.h).
// k_fuse_grids  one workgroup per keyframe: AssignFeaturesToGrid's CSR over the keyframe's mvKeysUn (assign_grid_csr, the rule of k_assign_grid),
//               cols * rows + 1 starts per keyframe and the items at the keyframe's offset, both relative to the keyframe.
// k_fuse_match  grid (blocks of 16 points, keyframe of the launch's chunk); SL_LANES lanes take one (keyframe, point): projection, gates, level and
//               the window's cells once (uniform over the lanes), then the window's CSR positions lane, lane + SL_LANES, ... in the ONE walk order
//               (walk_window).  Every lane keeps the minimum of distance << 18 | CSR position over the keypoints that pass the window, level and
//               chi-square tests; the minimum over the lanes (shuffles) is the reference's strict-< best, because the position grows with the
//               walk.  No candidate list, no cap, no LDS on that path; the per-keyframe pose comes in the launch arguments, FUSE_KF_CHUNK keyframes
//               per launch.  Counts and statistics: a reduction in the wave, the four waves' sums through LDS, one atomic per workgroup and word.
// Items 3 and 8 of the contract (ur and the chi-square sums) are written with __fmul_rn / __fadd_rn / __fsub_rn: every product and sum rounded on
// its own, whatever the contraction setting of the build.
// The contract (include/jsorb.h, jsorb_fuse_async) is restated in numpy in tests/test_fuse_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#define FU_POS ((1u << 18) - 1)
static_assert(sizeof(FuseArgs) + sizeof(FusePose) <= 4096, "k_fuse_match's arguments must fit a launch");

__global__ __launch_bounds__(1024) void k_fuse_grids(FuseGridArgs g)
{
    extern __shared__ int s_grid[];          // [n_cells] counts -> starts, [n_cells] cursors, [1024] scan scratch
    const int kf = blockIdx.x, off = g.kf_start[kf], n = g.kf_start[kf + 1] - off, n_cells = g.cols * g.rows;
    const float *x = g.x + off, *y = g.y + off;
    assign_grid_csr(n, n_cells, s_grid, g.cell_start + (size_t)kf * (n_cells + 1), g.cell_items + off,
                    [&](int i) -> int { return pos_in_grid(x[i], y[i], g.min_x, g.min_y, g.inv_w, g.inv_h, g.cols, g.rows); });
}

// the window of point i in a keyframe of pose T (Rcw, tcw, Ow): :839-879 with the contract's arithmetic; false: no candidate at all
struct FuseWindow {
    float u, v, ur, R;
    int L, x0, x1, y0, y1;
};
__device__ __forceinline__ bool fuse_point(const FuseArgs &a, const float *T, int i, FuseWindow &w)
{
    const jsorb_fuse_params &p = a.p;
    const float x = a.Px[i], y = a.Py[i], z = a.Pz[i];
    // K14's projection without its gate
    const float Pcx = T[9] + rot_row(T, x, y, z);
    const float Pcy = T[10] + rot_row(T + 3, x, y, z);
    const float Pcz = T[11] + rot_row(T + 6, x, y, z);
    if (!(Pcz > 0.0f)) return false;
    const float invz = 1.0f / Pcz;
    w.u = __builtin_fmaf(Pcx * p.fx, invz, p.cx);
    w.v = __builtin_fmaf(Pcy * p.fy, invz, p.cy);
    if (!(w.u >= p.min_x && w.u < p.max_x && w.v >= p.min_y && w.v < p.max_y)) return false;      // KeyFrame::IsInImage, half open; a NaN fails
    w.ur = __fsub_rn(w.u, __fmul_rn(p.bf, invz));                                                 // :857
    float ox, oy, oz, dist;
    if (!k16_gate(T + 12, x, y, z, a.min_dist_inv + i, a.max_dist_inv + i, ox, oy, oz, dist)) return false;      // :865
    const float dot = __builtin_fmaf(oz, a.Nz[i], __builtin_fmaf(ox, a.Nx[i], oy * a.Ny[i]));
    if (dot < 0.5f * dist) return false;                                                          // :871, a NaN passes
    w.L = k16_level(a.max_distance[i], dist, p.log_scale_factor, p.n_levels);
    w.R = p.th * p.scale_factor[w.L];                                                             // :877, one float product
    return sl_cells(p, w.u, w.v, w.R, w.x0, w.x1, w.y0, w.y1);
}

__global__ __launch_bounds__(256) void k_fuse_match(FuseArgs a, FusePose g)
{
    __shared__ int s_part[4][5];
    const int lane = threadIdx.x % SL_LANES, slot = blockIdx.y, kf = g.kf0 + slot;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    const int off = g.start[slot], len = g.start[slot + 1] - off;
    const bool in_range = i < a.n_points;
    const size_t o = (size_t)kf * a.n_points + (in_range ? i : 0);
    // every lane stays to the end (the reductions below take whole waves and the workgroup meets at a barrier)
    const bool live = in_range && len > 0 && !(a.skip && a.skip[o]);
    FuseWindow w;
    const bool win = live && fuse_point(a, g.pose[slot], i, w);      // uniform across the lanes of a point
    unsigned key = ~0u;
    int walked = 0, n_dist = 0;
    if (win) {
        const jsorb_fuse_params &p = a.p;
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        const int32_t *items = a.cell_items + off;
        walk_window<true>(a.cell_start + (size_t)kf * (p.cols * p.rows + 1), p.rows, w.x0, w.x1, w.y0, w.y1, lane, SL_LANES, [&](int j, bool in) {
            if (!in) return;
            walked++;
            const int k = off + items[j];
            const float kx = a.x[k], ky = a.y[k];
            if (!(fabsf(kx - w.u) < w.R && fabsf(ky - w.v) < w.R)) return;              // KeyFrame.cpp:602-606
            const int oct = a.octave[k];
            if (oct < w.L - 1 || oct > w.L) return;                                      // :898
            if ((unsigned)oct >= (unsigned)p.n_levels) return;                           // defined here: never a candidate
            if (p.check_reprojection) {                                                  // :901-925
                const float ex = __fsub_rn(w.u, kx), ey = __fsub_rn(w.v, ky);
                float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                const float kr = a.uright ? a.uright[k] : -1.0f;
                double chi = 5.99;
                if (kr >= 0.0f) {
                    const float er = __fsub_rn(w.ur, kr);
                    e2 = __fadd_rn(e2, __fmul_rn(er, er));
                    chi = 7.8;
                }
                if ((double)__fmul_rn(e2, p.inv_level_sigma2[oct]) > chi) return;        // a double comparison, as the C++ promotes it
            }
            uint4 lo, hi;
            sl_load_desc(a.kf_desc + 32 * (size_t)k, lo, hi);
            const int d = SL_HAMMING(lo, hi, mlo, mhi);
            n_dist++;
            key = min(key, (unsigned)d << 18 | (unsigned)j);                             // :931, strict <: the first in walk order wins a tie
        });
    }
    int window = walked;
    for (int s = SL_LANES / 2; s > 0; s >>= 1) {
        key = min(key, (unsigned)__shfl_xor((int)key, s, SL_LANES));
        window += __shfl_xor(window, s, SL_LANES);
    }
    int matched = 0;
    if (lane == 0 && in_range) {
        const int d = (int)(key >> 18);
        const bool m = key != ~0u && d <= a.p.th_low;                                    // :939
        a.best_idx[o] = m ? a.cell_items[off + (int)(key & FU_POS)] : -1;
        a.best_dist[o] = m ? d : -1;
        matched = m;
    }
    int pairs = win && lane == 0 ? 1 : 0;
    for (int s = 32; s > 0; s >>= 1) {
        matched += __shfl_xor(matched, s);
        pairs += __shfl_xor(pairs, s);
        walked += __shfl_xor(walked, s);
        n_dist += __shfl_xor(n_dist, s);
        window = max(window, __shfl_xor(window, s));
    }
    if (threadIdx.x % 64 == 0) {
        int *q = s_part[threadIdx.x / 64];
        q[0] = matched; q[1] = pairs; q[2] = walked; q[3] = n_dist; q[4] = window;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; v++) {
            matched += s_part[v][0]; pairs += s_part[v][1]; walked += s_part[v][2]; n_dist += s_part[v][3];
            window = max(window, s_part[v][4]);
        }
        if (matched) atomicAdd(&a.n_matched[kf], matched);
        if (pairs) atomicAdd(&a.stats[0], pairs);
        if (walked) atomicAdd(&a.stats[1], walked);
        if (n_dist) atomicAdd(&a.stats[2], n_dist);
        if (window) atomicMax(&a.stats[3], window);
    }
}

void launch_fuse_grids(const FuseGridArgs &g, int n_kf, hipStream_t s)
{
    if (n_kf <= 0) return;
    const size_t lds = (size_t)(2 * g.cols * g.rows + 1024) * sizeof(int);
    hipLaunchKernelGGL(k_fuse_grids, dim3(n_kf), dim3(1024), lds, s, g);
}

void launch_fuse_match(const FuseArgs &a, const FusePose &g, hipStream_t s)
{
    if (a.n_points <= 0 || g.n <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_fuse_match, dim3((a.n_points + per_block - 1) / per_block, g.n), dim3(256), 0, s, a, g);
}

} // namespace jsorb
