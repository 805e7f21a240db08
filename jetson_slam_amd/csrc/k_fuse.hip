// k_fuse.hip - the matcher of LocalMapping::SearchInNeighbors (LocalMapping.cpp:460-540) and of loop closing on the device:
//   ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cpp:812-962) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:964-1087), the search part
//   (:829-936) with KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage (KeyFrame.cpp:573-617), map points against several keyframes in one call.
// :839-936 are a pure function of (keyframe, point): no claim rule, no rotation check.  The head test (:833-837) and the tail (:938-958: Replace,
// AddObservation, AddMapPoint) touch the map and stay with the caller, who replays them over best_idx in the reference's order (include/jsorb.h).
// k_fuse_grids  one workgroup per keyframe: AssignFeaturesToGrid's CSR over the keyframe's mvKeysUn (assign_grid_csr, the rule of k_assign_grid),
//               cols * rows + 1 starts per keyframe and the items at the keyframe's offset, both relative to the keyframe.
// k_fuse_match  grid (blocks of 16 points, keyframe of the launch's chunk); SL_LANES lanes take one (keyframe, point): projection, gates, level and
//               the window's cells once (uniform over the lanes), then the window's best keypoint.  The projected-window search is
//               k_search_common.h's, shared with k_sim3_match: proj_pixel and proj_cells around the K16 gate (ur and the normal test stay here),
//               window_best - walk_window<true> dealt over the lanes, the minimum of distance << 18 | CSR position - with the chi-square test
//               as the per-keypoint filter, block_totals for the counts and statistics (one atomic per workgroup and word).  No candidate list, no cap; the
//               per-keyframe pose comes in the launch arguments, FUSE_KF_CHUNK keyframes per launch.
// k_fuse_match_run  the same body over one keyframe whose run is read from the graph on the device (jsorb_fuse_map_async, k_fuse_apply.hip).
// Items 3 and 8 of the contract (ur and the chi-square sums) are written with __fmul_rn / __fadd_rn / __fsub_rn: every product and sum rounded on
// its own, whatever the contraction setting of the build.
// The contract (include/jsorb.h, jsorb_fuse_async) is restated in numpy in tests/test_fuse_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

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
__device__ __forceinline__ bool fuse_point(const FuseArgs &a, const float *T, int i, ProjWindow &w, float &ur)
{
    const jsorb_fuse_params &p = a.p;
    const float x = a.Px[i], y = a.Py[i], z = a.Pz[i];
    // K14's projection without its gate
    float invz;
    if (!proj_pixel(p, T[9] + rot_row(T, x, y, z), T[10] + rot_row(T + 3, x, y, z), T[11] + rot_row(T + 6, x, y, z), w, invz)) return false;
    ur = __fsub_rn(w.u, __fmul_rn(p.bf, invz));                                                   // :857
    float ox, oy, oz, dist;
    if (!k16_gate(T + 12, x, y, z, a.min_dist_inv + i, a.max_dist_inv + i, ox, oy, oz, dist)) return false;      // :865
    const float dot = __builtin_fmaf(oz, a.Nz[i], __builtin_fmaf(ox, a.Nx[i], oy * a.Ny[i]));
    if (dot < 0.5f * dist) return false;                                                          // :871, a NaN passes
    return proj_cells(p, a.max_distance[i], dist, w);                                             // :877
}

// one (keyframe, point) per SL_LANES lanes.  kf: the keyframe's row of the outputs, of `skip` and of n_matched; grid: its CSR among cell_start's;
// off, len: its run of the concatenated keyframe arrays; T: its pose
__device__ __forceinline__ void fuse_match_body(const FuseArgs &a, const float *T, int kf, int grid, int off, int len)
{
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    const bool in_range = i < a.n_points;
    const size_t o = (size_t)kf * a.n_points + (in_range ? i : 0);
    // every lane stays to the end (the reductions below take whole waves and the workgroup meets at a barrier)
    const bool live = in_range && len > 0 && !(a.skip && a.skip[o]);
    ProjWindow w;
    float ur;
    const bool win = live && fuse_point(a, T, i, w, ur);                 // uniform across the lanes of a point
    const jsorb_fuse_params &p = a.p;
    const float *uright = a.uright ? a.uright + off : nullptr;
    int sum[4] = {0, win && lane == 0 ? 1 : 0, 0, 0}, window;             // matched, pairs with a window, keypoints walked, distances
    const unsigned key = window_best(
        win, w, a.cell_start + (size_t)grid * (p.cols * p.rows + 1), p.rows, a.cell_items + off, a.x + off, a.y + off, a.octave + off,
        a.kf_desc + 32 * (size_t)off, a.mp_desc + 32 * (size_t)i,
        [&](int k, float kx, float ky, int oct) {                                        // :898 left the level; the chi-square test
            if ((unsigned)oct >= (unsigned)p.n_levels) return false;                     // defined here: never a candidate
            if (p.check_reprojection) {                                                  // :901-925
                const float ex = __fsub_rn(w.u, kx), ey = __fsub_rn(w.v, ky);
                float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                const float kr = uright ? uright[k] : -1.0f;
                double chi = 5.99;
                if (kr >= 0.0f) {
                    const float er = __fsub_rn(ur, kr);
                    e2 = __fadd_rn(e2, __fmul_rn(er, er));
                    chi = 7.8;
                }
                if ((double)__fmul_rn(e2, p.inv_level_sigma2[oct]) > chi) return false;  // a double comparison, as the C++ promotes it
            }
            return true;
        },
        sum[2], sum[3], window);
    if (lane == 0 && in_range) {
        const int d = (int)(key >> 18);
        const bool m = key != ~0u && d <= a.p.th_low;                                    // :939
        a.best_idx[o] = m ? a.cell_items[off + (int)(key & PW_POS)] : -1;
        a.best_dist[o] = m ? d : -1;
        sum[0] = m;
    }
    block_totals(sum, window);
    if (threadIdx.x == 0) {
        if (sum[0]) atomicAdd(&a.n_matched[kf], sum[0]);
        if (sum[1]) atomicAdd(&a.stats[0], sum[1]);
        if (sum[2]) atomicAdd(&a.stats[1], sum[2]);
        if (sum[3]) atomicAdd(&a.stats[2], sum[3]);
        if (window) atomicMax(&a.stats[3], window);
    }
}

__global__ __launch_bounds__(256) void k_fuse_match(FuseArgs a, FusePose g)
{
    const int slot = blockIdx.y, kf = g.kf0 + slot;
    fuse_match_body(a, g.pose[slot], kf, kf, g.start[slot], g.start[slot + 1] - g.start[slot]);
}

// the same over ONE keyframe whose run is read on the device (jsorb_fuse_map_async): the keyframe arrays are the whole pool, the run that of slot
// r.slot where the slot is a live target (fuse_target_run), the output row r.row of best_idx / best_dist, `skip` and the grid the target's own
__global__ __launch_bounds__(256) void k_fuse_match_run(FuseArgs a, FuseRun r)
{
    int off, len;
    fuse_target_run(r.state, r.point_off, r.point_len, r.n_slots, r.pool_entries, r.slot, off, len);
    a.best_idx += (size_t)r.row * a.n_points;
    a.best_dist += (size_t)r.row * a.n_points;
    a.n_matched += r.row;
    fuse_match_body(a, r.pose, 0, 0, off, len);
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

void launch_fuse_match_run(const FuseArgs &a, const FuseRun &r, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_fuse_match_run, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a, r);
}

} // namespace jsorb
