// k_search_last.hip - the matcher of Tracking::TrackWithMotionModel (Tracking.cpp:1030-1066) on the device:
//   ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono), the GPU branch that runs (ORBmatcher.cpp:1647-1963), with
//   the invz variant of Frame::GetFeaturesInArea (Frame.cpp:569-639) and ComputeThreeMaxima (ORBmatcher.cpp:2097-2138).
// The reference gathers every point's candidates before it assigns any, and TrackWithMotionModel clears mvpMapPoints before each pass: no point
// hides a keypoint from another, so every point's best is independent of the others.  Here:
//   k_last_match    SL_LANES lanes per point: K14's projection (k14_project, shared with k_project_points), the window's cells in the reference's
//                   order (ix outer, iy inner, a cell's items ascending: the CSR position grows with the walk), the level / window / uRight filters and
//                   the minimum of (distance, CSR position) over the lanes, which is the reference's strict-< best.  Writes the point's match, its
//                   rotation bin and candidate count, and atomicMax(owner[k], i): of the points that choose k the last one stays.
//   k_last_resolve  one workgroup: the rotation histogram, ComputeThreeMaxima, kp_match = owner with the keypoints of culled entries nulled, the count.
// The window walk and the rotation check are k_search_common.h's (walk_window; rot_bin, rot_keep).
// A second pass with 2 th replaces the first when it found fewer than retry_below matches: its two kernels are enqueued behind the first pass's
// and return at once when the first pass's count (ctl[0], written by its k_last_resolve) says no.
// The contract (include/jsorb.h, jsorb_search_last_frame_async) is restated in numpy in tests/test_search_last_frame_host.py.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#define LF_KEY(d, j) ((d) << 18 | (j))           // distance <= 256, CSR position < 2^18

// the second pass, when the first found enough matches (or retry is off): nothing to do
__device__ __forceinline__ bool lf_skip(const LastFrameArgs &a, int pass) { return pass && !a.ctl[0]; }

__global__ __launch_bounds__(256) void k_last_match(LastFrameArgs a, int pass)
{
    if (lf_skip(a, pass)) return;
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    if (i >= a.n_points) return;                     // (whole groups of SL_LANES lanes leave together)
    const jsorb_last_frame_params &p = a.p;
    const FrameView &f = a.f;
    float u, v, invz;
    const bool valid = k14_project(p.Rcw, p.tcw, a.Px[i], a.Py[i], a.Pz[i], p.fx, p.fy, p.cx, p.cy, p.min_x, p.max_x, p.min_y, p.max_y, u, v, invz);
    const int L = a.octave[i];
    int best = INT_MAX, count = 0;
    int x0, x1, y0, y1;
    float R = 0.0f;
    if (valid && L >= 0 && L < f.n_levels) R = (pass ? 2.0f * p.th : p.th) * f.scale[L];     // radius = th * mvScaleFactors[last_octave]
    // everything up to here is uniform across the lanes of a point
    if (valid && L >= 0 && L < f.n_levels && sl_cells(p, u, v, R, x0, x1, y0, y1)) {
        // GetFeaturesInArea's level window: (L, -1) forward, (0, L) backward, (L-1, L+1) otherwise; levels only checked when minLevel > 0 || maxLevel >= 0
        const int lo = p.direction > 0 ? L : p.direction < 0 ? 0 : L - 1;
        const int hi = p.direction > 0 ? -1 : p.direction < 0 ? L : L + 1;
        const bool levels = lo > 0 || hi >= 0;
        const float m = p.mbf * invz;                // ur = x - mbf*invzc (Frame.cpp:628), two roundings
        const float xr = u - m;
        uint4 mlo, mhi;
        sl_load_desc(a.mp_desc + 32 * (size_t)i, mlo, mhi);
        walk_window<false>(f.cell_start, p.rows, x0, x1, y0, y1, lane, SL_LANES, [&](int j, bool) {
            const int k = f.cell_items[j];
            const int oct = f.octave(k);
            if (levels && (oct < lo || (hi >= 0 && oct > hi))) return;
            if (!(fabsf(f.x(k) - u) < R && fabsf(f.y(k) - v) < R)) return;
            if (f.u_right) {
                const float ur = f.u_right[k];
                if (ur > 0 && fabsf(xr - ur) > R) return;
            }
            count++;
            uint4 lo4, hi4;
            sl_load_desc(f.desc + 32 * (size_t)k, lo4, hi4);
            best = min(best, LF_KEY(SL_HAMMING(lo4, hi4, mlo, mhi), j));
        });
    }
    for (int s = SL_LANES / 2; s > 0; s >>= 1) {      // the point's lanes are all here: reduce over them
        best = min(best, __shfl_xor(best, s, SL_LANES));
        count += __shfl_xor(count, s, SL_LANES);
    }
    if (lane) return;
    // bestDist starts at 256 with strict < updates (ORBmatcher.cpp:1898-1913): a distance of 256 is never taken; match iff bestDist <= TH_HIGH
    const int d = best >> 18;
    int match = -1, dist = -1, bin = -1;
    if (d < 256 && d <= p.th_high) {
        match = f.cell_items[best & ((1 << 18) - 1)];
        dist = d;
        atomicMax(&a.owner[match], i);               // CurrentFrame.mvpMapPoints[bestIdx2] = point i, in point order: the largest i stays
        if (p.check_orientation) bin = rot_bin(a.angle[i], f.angle(match));
    }
    a.match_kp[i] = match;
    a.match_dist[i] = dist;
    a.bin[i] = bin;
    a.cand[i] = count;
}

// One workgroup: the histogram over the matched points, ComputeThreeMaxima, kp_match and the count; owner is reset to -1 for the next call.
__global__ __launch_bounds__(1024) void k_last_resolve(LastFrameArgs a, int pass)
{
    __shared__ int s_hist[HISTO_LENGTH + 1], s_keep[HISTO_LENGTH + 1], s_matched, s_culled, s_cand;
    if (lf_skip(a, pass)) return;
    const int tid = threadIdx.x, n = a.n_points, N = a.f.n_kp;
    const bool rot = a.p.check_orientation != 0;
    if (tid <= HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) { s_matched = 0; s_culled = 0; s_cand = 0; }
    __syncthreads();
    int matched = 0, cand = 0;
    for (int i = tid; i < n; i += 1024) {
        cand += a.cand[i];
        if (a.match_kp[i] >= 0) {
            matched++;
            if (rot) atomicAdd(&s_hist[a.bin[i]], 1);      // rotHist[bin].push_back(bestIdx2): one entry per matched point
        }
    }
    atomicAdd(&s_matched, matched);
    atomicAdd(&s_cand, cand);
    for (int k = tid; k < N; k += 1024) {
        a.kp_match[k] = a.owner[k];
        a.owner[k] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        const ThreeMaxima m = rot_keep(s_hist, s_keep, rot);
        a.ctl[3] = m.ind1; a.ctl[4] = m.ind2; a.ctl[5] = m.ind3;
    }
    __syncthreads();
    int culled = 0;
    if (rot)
        for (int i = tid; i < n; i += 1024) {
            const int m = a.match_kp[i];
            if (m >= 0 && !s_keep[a.bin[i]]) {       // CurrentFrame.mvpMapPoints[rotHist[i][j]] = NULL; nmatches--
                a.kp_match[m] = -1;
                culled++;
            }
        }
    atomicAdd(&s_culled, culled);
    __syncthreads();
    if (tid == 0) {
        const int count = s_matched - s_culled;
        *a.n_matches = count;
        a.ctl[1] = pass + 1;
        a.ctl[2] = s_cand;
        if (!pass) a.ctl[0] = a.p.retry_below > 0 && count < a.p.retry_below;
    }
}

void launch_last_match(const LastFrameArgs &a, int pass, hipStream_t s)
{
    if (a.n_points <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_last_match, dim3((a.n_points + per_block - 1) / per_block), dim3(256), 0, s, a, pass);
}

void launch_last_resolve(const LastFrameArgs &a, int pass, hipStream_t s) { hipLaunchKernelGGL(k_last_resolve, dim3(1), dim3(1024), 0, s, a, pass); }

} // namespace jsorb
