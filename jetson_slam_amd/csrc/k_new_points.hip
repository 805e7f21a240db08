// k_new_points.hip - the loop of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-457) over the device state, all neighbours of a call
// (include/jsorb.h, jsorb_create_new_map_points_async; restated in numpy in tests/new_points_cases.py).
// k_np_gather   a lane per gathered entry: the current run's n1 keypoints and every neighbour's, `cap` apart, copied out of the pool as the sides
//               k_bow_group / k_tri_match take (node, free, stereo, x, y, octave, descriptor); a skipped neighbour and the padding behind a run are
//               keypoints in no node.  The first 1 + n_nb lanes also write each run's offset (-1: skipped) and the neighbours' slots.
// k_np_verdict  a lane per (neighbour, idx1), coalesced over idx1; NP_KF_CHUNK neighbours' poses per launch in the arguments.  The pair's verdict
//               (:297-437) with the 4x4 double Jacobi in registers: A and V are 32 doubles, every index a constant after unrolling.
// k_np_own      a lane per idx1 walks its column of verdicts: the first accepted neighbour keeps it, later matches are `taken`.
// k_np_count / k_np_scan / k_np_write   the order-preserving compaction of the owning pairs in k_local_map.hip's form (chunk sums, one
//               workgroup's exclusive prefix, ballot ranks): pair k takes new_row[k] and writes the row, its KF1 entry and its log record, and
//               claims its KF2 entry by atomicMax of its position.
// k_np_link     a lane per pair: the claim's winner writes the KF2 entry.  k_np_finish: the counts.
// Every float and double operation is written as the contract orders it; the build passes -ffp-contract=off.
#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef NP_CHUNK
#define NP_CHUNK 1024                            // pairs per chunk of the compaction (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define NP_SCAN_THREADS 1024
#define NP_SWEEPS 8
static_assert(NP_CHUNK >= 64 && NP_CHUNK % 64 == 0 && NP_CHUNK <= 4096, "a chunk is whole waves");
static_assert(sizeof(NewPointsArgs) + sizeof(NewPointsPoses) <= 4096 && sizeof(NewPointsArgs) + sizeof(NewPointsSlots) <= 4096, "kernel arguments");

typedef unsigned long long u64;
enum { NP_NO_MATCH = 0, NP_CREATED, NP_TAKEN, NP_LOW_PARALLAX, NP_W_ZERO, NP_Z1, NP_Z2, NP_REPROJ1, NP_REPROJ2, NP_ZERO_DIST, NP_SCALE, NP_NO_ROW, NP_EMPTY,
       NP_SKIPPED };
enum { NP_C_MATCHES = 0, NP_C_ACCEPTED, NP_C_OWNING, NP_C_CREATED, NP_C_SHARED, NP_C_NO_ROW, NP_C_TAKEN, NP_C_SKIPPED, NP_C_LOG_OVERFLOW, NP_C_SVD,
       NP_C_UNPROJECT, NP_C_NO_CURRENT };

__device__ __forceinline__ bool np_run_ok(int off, int len, int entries) { return off >= 0 && len >= 0 && (long long)off + len <= entries; }
__device__ __forceinline__ bool np_good(const NewPointsArgs &a, int s) { return s >= 0 && s < a.g.max_keyframes && a.g.state[s] == 1; }
// the current keyframe's run offset, or -1
__device__ __forceinline__ int np_current(const NewPointsArgs &a)
{
    if (!np_good(a, a.current_slot)) return -1;
    const int off = a.g.point_off[a.current_slot], len = a.g.point_len[a.current_slot];
    return np_run_ok(off, len, a.g.pool_entries) && len == a.n1 ? off : -1;
}
// neighbour t of the list: its run's offset and length, or -1 (a slot an earlier position of the list holds is skipped: the reference's list
// holds a keyframe once)
__device__ __forceinline__ int np_neighbour(const NewPointsArgs &a, const NewPointsSlots &sl, int t, int &len)
{
    const int s = sl.slot[t];
    len = 0;
    if (!np_good(a, s) || s == a.current_slot || np_current(a) < 0) return -1;
    for (int u = 0; u < t; u++)
        if (sl.slot[u] == s) return -1;
    const int off = a.g.point_off[s], n = a.g.point_len[s];
    if (!np_run_ok(off, n, a.g.pool_entries) || n > a.cap) return -1;
    len = n;
    return off;
}
// the sum over a wave of a lane's 0 / 1 into one statistics word
__device__ __forceinline__ void np_tally(int *word, bool one)
{
    const u64 m = __ballot(one);
    if (m && (threadIdx.x % 64) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(word, (int)__popcll(m));
}

__global__ __launch_bounds__(256) void k_np_gather(NewPointsArgs a, NewPointsSlots s)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x, total = (long long)a.n1 + (long long)a.n_nb * a.cap;
    if (i < 1 + a.n_nb) {
        if (i == 0) {
            const int off = np_current(a);
            a.info[0] = off;
            if (off < 0) a.stats[NP_C_NO_CURRENT] = 1;
        } else {
            int len;
            const int off = np_neighbour(a, s, (int)i - 1, len);
            a.info[i] = off;
            a.nb_slot[i - 1] = s.slot[i - 1];
            if (off < 0) atomicAdd(&a.stats[NP_C_SKIPPED], 1);
        }
    }
    if (i >= total) return;
    const bool side1 = i < a.n1;
    const int t = side1 ? 0 : (int)((i - a.n1) / a.cap), j = side1 ? (int)i : (int)((i - a.n1) % a.cap);
    int len = a.n1;
    const int off = side1 ? np_current(a) : np_neighbour(a, s, t, len);
    const bool real = off >= 0 && j < len;
    const size_t e = real ? (size_t)off + j : 0, d = side1 ? (size_t)j : (size_t)t * a.cap + j;
    int32_t *node = side1 ? a.node1 : a.node2;
    uint8_t *fr = side1 ? a.free1 : a.free2, *ste = side1 ? a.stereo1 : a.stereo2, *desc = side1 ? a.desc1 : a.desc2;
    float *x = side1 ? a.x1 : a.x2, *y = side1 ? a.y1 : a.y2;
    int oct = real ? a.kp.octave[e] : 0;
    // a KF1 keypoint whose octave is out of range is in no node: the pair counts as no match
    node[d] = real && (!side1 || (unsigned)oct < (unsigned)a.n_levels) ? a.ex.node[e] : -1;
    fr[d] = real && a.g.point_pool[e] == -1;
    ste[d] = real && a.kp.uright && a.kp.uright[e] >= 0.0f;
    x[d] = real ? a.kp.x[e] : 0.0f;
    y[d] = real ? a.kp.y[e] : 0.0f;
    if (!side1) a.octave2[d] = oct;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (real) sl_load_desc(a.kp.desc + 32 * e, lo, hi);
    uint4 *q = reinterpret_cast<uint4 *>(desc) + 2 * d;
    q[0] = lo; q[1] = hi;
}

// Mat::dot of a row of three with x: double products summed left to right
__device__ __forceinline__ double np_dot3(const float *r, const float *x)
{
    double s = (double)r[0] * (double)x[0];
    s = s + (double)r[1] * (double)x[1];
    s = s + (double)r[2] * (double)x[2];
    return s;
}
// cv::norm of three floats
__device__ __forceinline__ float np_norm3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }
// Rwc v (+ nothing): Rwc = Rcw^T, each row summed left to right
__device__ __forceinline__ void np_rwc(const float *R, const float *v, float *o)
{
    for (int i = 0; i < 3; i++) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2];
}

// the contract's cv::SVD::compute of the float 4x4 A: the null vector (vt.row(3)) rounded to float
__device__ __forceinline__ void np_null_vector(const float Af[4][4], float out[4])
{
    double A[4][4], V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) { A[i][j] = (double)Af[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sweep = 0; sweep < NP_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = A[0][p] * A[0][p], beta = A[0][q] * A[0][q], gamma = A[0][p] * A[0][q];
#pragma unroll
                for (int k = 1; k < 4; k++) {
                    alpha = alpha + A[k][p] * A[k][p];
                    beta = beta + A[k][q] * A[k][q];
                    gamma = gamma + A[k][p] * A[k][q];
                }
                if (gamma == 0.0) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = c * ap - s * aq;
                    A[k][q] = s * ap + c * aq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
    }
    int best = 0;
    double least = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double n = A[0][j] * A[0][j];
#pragma unroll
        for (int k = 1; k < 4; k++) n = n + A[k][j] * A[k][j];
        if (j == 0 || n <= least) { least = n; best = j; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = (float)(best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3]);
}

// the reprojection gate of one keyframe (:368-419): true = rejected.  mbf is the CURRENT keyframe's for both (:412)
__device__ __forceinline__ bool np_reproject(const jsorb_keyframe_pose &P, const float *X, float z, float kx, float ky, float ur, bool stereo, float mbf,
                                             double chi2_mono, double chi2_stereo)
{
    const float xc = (float)(np_dot3(P.Rcw, X) + (double)P.tcw[0]);
    const float yc = (float)(np_dot3(P.Rcw + 3, X) + (double)P.tcw[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = P.fx * xc * invz + P.cx, v = P.fy * yc * invz + P.cy;
    const float ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > chi2_mono;
    const float u_r = u - mbf * invz;
    const float er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > chi2_stereo;
}

__global__ __launch_bounds__(256) void k_np_verdict(NewPointsArgs a, NewPointsPoses g)
{
    const int t = g.kf0 + blockIdx.y, idx1 = blockIdx.x * 256 + threadIdx.x;
    const bool in = idx1 < a.n1;
    const int off1 = a.info[0], off2 = a.info[1 + t];
    const jsorb_keyframe_pose &P1 = g.cur, &P2 = g.nb[blockIdx.y];
    if (idx1 < 3) {                                  // the camera centres k_np_write reads: the neighbours', then the current keyframe's
        a.ow[3 * t + idx1] = P2.Ow[idx1];
        if (blockIdx.y == 0) a.ow[3 * a.n_nb + idx1] = P1.Ow[idx1];
    }
    const size_t p = (size_t)t * a.n1 + (in ? idx1 : 0);
    const int idx2 = in && off2 >= 0 ? a.match12[p] : -1;
    int verdict = off2 < 0 ? NP_SKIPPED : NP_NO_MATCH, path = 0;
    float X[3] = {0.0f, 0.0f, 0.0f};
    if (idx2 >= 0) {
        const size_t e1 = (size_t)off1 + idx1, e2 = (size_t)off2 + idx2;
        const float k1x = a.kp.x[e1], k1y = a.kp.y[e1], k2x = a.kp.x[e2], k2y = a.kp.y[e2];
        const float ur1 = a.kp.uright ? a.kp.uright[e1] : -1.0f, ur2 = a.kp.uright ? a.kp.uright[e2] : -1.0f;
        const bool st1 = ur1 >= 0.0f, st2 = ur2 >= 0.0f;
        const int oct1 = a.kp.octave[e1], oct2 = a.kp.octave[e2];      // both in [0, n_levels): k_np_gather and k_tri_match checked them
        // :306-311
        const float xn1[3] = {(k1x - P1.cx) * P1.invfx, (k1y - P1.cy) * P1.invfy, 1.0f};
        const float xn2[3] = {(k2x - P2.cx) * P2.invfx, (k2y - P2.cy) * P2.invfy, 1.0f};
        float ray1[3], ray2[3];
        np_rwc(P1.Rcw, xn1, ray1);
        np_rwc(P2.Rcw, xn2, ray2);
        const float cos_rays = (float)(np_dot3(ray1, ray2) / ((double)np_norm3(ray1[0], ray1[1], ray1[2]) * (double)np_norm3(ray2[0], ray2[1], ray2[2])));
        // :313-322
        float cos1 = cos_rays + 1.0f, cos2 = cos1;
        if (st1) cos1 = a.ex.cos_stereo[e1];
        else if (st2) cos2 = a.ex.cos_stereo[e2];
        const float cos_stereo = cos2 < cos1 ? cos2 : cos1;
        verdict = NP_CREATED;
        if (cos_rays < cos_stereo && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {      // :325
            path = 1;
            float A[4][4], h[4];
            for (int j = 0; j < 4; j++) {
                const float t1r0 = j < 3 ? P1.Rcw[j] : P1.tcw[0], t1r1 = j < 3 ? P1.Rcw[3 + j] : P1.tcw[1], t1r2 = j < 3 ? P1.Rcw[6 + j] : P1.tcw[2];
                const float t2r0 = j < 3 ? P2.Rcw[j] : P2.tcw[0], t2r1 = j < 3 ? P2.Rcw[3 + j] : P2.tcw[1], t2r2 = j < 3 ? P2.Rcw[6 + j] : P2.tcw[2];
                A[0][j] = xn1[0] * t1r2 - t1r0;
                A[1][j] = xn1[1] * t1r2 - t1r1;
                A[2][j] = xn2[0] * t2r2 - t2r0;
                A[3][j] = xn2[1] * t2r2 - t2r1;
            }
            np_null_vector(A, h);
            if (h[3] == 0.0f) verdict = NP_W_ZERO;                                                        // :339
            else { X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3]; }                          // :343
        } else if ((st1 && cos1 < cos2) || (st2 && cos2 < cos1)) {                                        // :346-353, KeyFrame.cpp:619-635
            const bool first = st1 && cos1 < cos2;
            path = first ? 2 : 3;
            const jsorb_keyframe_pose &P = first ? P1 : P2;
            const size_t e = first ? e1 : e2;
            const float z = a.ex.depth[e];
            if (z > 0.0f) {
                const float u = a.ex.raw_x ? a.ex.raw_x[e] : a.kp.x[e], v = a.ex.raw_y ? a.ex.raw_y[e] : a.kp.y[e];
                const float xc[3] = {(u - P.cx) * z * P.invfx, (v - P.cy) * z * P.invfy, z};
                float r[3];
                np_rwc(P.Rcw, xc, r);
                X[0] = r[0] + P.Ow[0]; X[1] = r[1] + P.Ow[1]; X[2] = r[2] + P.Ow[2];
            } else {
                verdict = NP_EMPTY;
            }
        } else {
            verdict = NP_LOW_PARALLAX;                                                                    // :355
        }
        if (verdict == NP_CREATED) {
            const float z1 = (float)(np_dot3(P1.Rcw + 6, X) + (double)P1.tcw[2]);                          // :360-366
            const float z2 = (float)(np_dot3(P2.Rcw + 6, X) + (double)P2.tcw[2]);
            if (z1 <= 0.0f) verdict = NP_Z1;
            else if (z2 <= 0.0f) verdict = NP_Z2;
            else if (np_reproject(P1, X, z1, k1x, k1y, ur1, st1, P1.mbf, a.chi2_mono[oct1], a.chi2_stereo[oct1])) verdict = NP_REPROJ1;
            else if (np_reproject(P2, X, z2, k2x, k2y, ur2, st2, P1.mbf, a.chi2_mono[oct2], a.chi2_stereo[oct2])) verdict = NP_REPROJ2;
            else {
                const float dist1 = np_norm3(X[0] - P1.Ow[0], X[1] - P1.Ow[1], X[2] - P1.Ow[2]);          // :422-437
                const float dist2 = np_norm3(X[0] - P2.Ow[0], X[1] - P2.Ow[1], X[2] - P2.Ow[2]);
                if (dist1 == 0.0f || dist2 == 0.0f) verdict = NP_ZERO_DIST;
                else {
                    const float ratio_dist = dist2 / dist1, ratio_octave = a.scale_factor[oct1] / a.scale_factor[oct2];
                    if (ratio_dist * a.ratio_factor < ratio_octave || ratio_dist > ratio_octave * a.ratio_factor) verdict = NP_SCALE;
                }
            }
        }
    }
    if (in) {
        a.verdict[p] = verdict;
        a.path[p] = (uint8_t)path;
        a.x3D[3 * p] = X[0]; a.x3D[3 * p + 1] = X[1]; a.x3D[3 * p + 2] = X[2];
    }
    np_tally(&a.stats[NP_C_MATCHES], idx2 >= 0);
    np_tally(&a.stats[NP_C_ACCEPTED], idx2 >= 0 && verdict == NP_CREATED);
    np_tally(&a.stats[NP_C_SVD], path == 1);
    np_tally(&a.stats[NP_C_UNPROJECT], path >= 2);
}

__global__ __launch_bounds__(256) void k_np_own(NewPointsArgs a)
{
    const int idx1 = blockIdx.x * 256 + threadIdx.x;
    int taken = 0;
    if (idx1 < a.n1) {
        bool owned = false;
        for (int t = 0; t < a.n_nb; t++) {
            const size_t p = (size_t)t * a.n1 + idx1;
            const int v = a.verdict[p];
            if (owned && v != NP_NO_MATCH && v != NP_SKIPPED) {
                a.verdict[p] = NP_TAKEN; a.path[p] = 0;
                a.x3D[3 * p] = 0.0f; a.x3D[3 * p + 1] = 0.0f; a.x3D[3 * p + 2] = 0.0f;
                taken++;
            } else if (v == NP_CREATED) {
                owned = true;
            }
        }
    }
    for (int s = 32; s > 0; s >>= 1) taken += __shfl_xor(taken, s);
    if (threadIdx.x % 64 == 0 && taken) atomicAdd(&a.stats[NP_C_TAKEN], taken);
}

__global__ __launch_bounds__(256) void k_np_count(NewPointsArgs a, long long n_pairs)
{
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * NP_CHUNK;
    unsigned mine = 0;
    for (int idx = threadIdx.x; idx < NP_CHUNK; idx += 256) {
        const long long p = base + idx;
        if (p < n_pairs && a.verdict[p] == NP_CREATED) mine++;
    }
    for (int s = 32; s > 0; s >>= 1) mine += (unsigned)__shfl_xor((int)mine, s);
    if (threadIdx.x % 64 == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) a.chunk_sum[blockIdx.x] = s_cnt;
}

// pre[i] = the sum of sum[i'] over i' < i, for i = 0 .. n (k_lm_scan's form)
__global__ __launch_bounds__(NP_SCAN_THREADS) void k_np_scan(NewPointsArgs a, int n)
{
    __shared__ unsigned wsum[NP_SCAN_THREADS / 64];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    unsigned carry = 0;
    for (int base = 0; base < n; base += NP_SCAN_THREADS) {
        const int i = base + (int)threadIdx.x;
        const unsigned x = i < n ? a.chunk_sum[i] : 0u;
        unsigned inc = x;
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)inc, s);
            if (lane >= s) inc += y;
        }
        __syncthreads();
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int w = 0; w < NP_SCAN_THREADS / 64; w++) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (i < n) a.chunk_pre[i] = carry + before + inc - x;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.chunk_pre[n] = carry;
        a.stats[NP_C_OWNING] = (int)carry;
        a.stats[NP_C_LOG_OVERFLOW] = carry > (unsigned)a.log_cap;
    }
}

__global__ __launch_bounds__(256) void k_np_write(NewPointsArgs a, long long n_pairs)
{
    __shared__ unsigned wcnt[4];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const long long base = (long long)blockIdx.x * NP_CHUNK;
    const int off1 = a.info[0];
    unsigned running = a.chunk_pre[blockIdx.x];
    int created = 0, dropped = 0;
    for (int r0 = 0; r0 < NP_CHUNK && base + r0 < n_pairs; r0 += 256) {      // (uniform over the workgroup)
        const int idx = r0 + (int)threadIdx.x;
        const long long p = base + idx;
        const bool own = idx < NP_CHUNK && p < n_pairs && a.verdict[p] == NP_CREATED;
        const u64 m = __ballot(own);
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned k = running + (unsigned)__popcll(m & ((1ull << lane) - 1));
        for (int w = 0; w < wave; w++) k += wcnt[w];
        if (own) {
            const int t = (int)(p / a.n1), idx1 = (int)(p % a.n1), idx2 = a.match12[p];
            const int r = k < (unsigned)a.row_capacity ? a.new_row[k] : -1;
            const bool ok = r >= 0 && r < a.n_rows;
            if (k < (unsigned)a.log_cap) {
                int32_t *rec = a.log_out + 4 * (size_t)k;
                rec[0] = ok ? r : -1; rec[1] = idx1; rec[2] = t; rec[3] = idx2;
            }
            if (!ok) {
                a.verdict[p] = NP_NO_ROW;
                dropped++;
            } else {
                const int slot2 = a.nb_slot[t];
                const size_t e1 = (size_t)off1 + idx1, e2 = (size_t)a.info[1 + t] + idx2;
                const float X[3] = {a.x3D[3 * p], a.x3D[3 * p + 1], a.x3D[3 * p + 2]};
                const float *Ow2 = a.ow + 3 * t;
                // the two observations in (order_key, slot) order
                const long long key1 = a.g.order_key[a.current_slot], key2 = a.g.order_key[slot2];
                const bool cur_first = key1 < key2 || (key1 == key2 && a.current_slot < slot2);
                const float n1v[3] = {X[0] - a.ow[3 * a.n_nb], X[1] - a.ow[3 * a.n_nb + 1], X[2] - a.ow[3 * a.n_nb + 2]};
                const float n2v[3] = {X[0] - Ow2[0], X[1] - Ow2[1], X[2] - Ow2[2]};
                const float d1 = np_norm3(n1v[0], n1v[1], n1v[2]), d2 = np_norm3(n2v[0], n2v[1], n2v[2]);
                const float *na = cur_first ? n1v : n2v, *nb = cur_first ? n2v : n1v;
                const float da = cur_first ? d1 : d2, db = cur_first ? d2 : d1;
                float Pn[3];
                for (int c = 0; c < 3; c++) Pn[c] = ((0.0f + na[c] / da) + nb[c] / db) / 2.0f;            // MapPoint.cpp:385-394, :406
                const float max_d = d1 * a.scale_factor[a.kp.octave[e1]];                                 // :396-404
                const float min_d = max_d / a.scale_factor[a.n_levels - 1];
                a.st.Px[r] = X[0]; a.st.Py[r] = X[1]; a.st.Pz[r] = X[2];
                a.st.Pnx[r] = Pn[0]; a.st.Pny[r] = Pn[1]; a.st.Pnz[r] = Pn[2];
                a.st.MaxDistance[r] = max_d;
                a.st.invariance_maxDistance[r] = 1.2f * max_d;
                a.st.invariance_minDistance[r] = 0.8f * min_d;
                a.st.bad[r] = 0;
                if (a.st.ref_slot) a.st.ref_slot[r] = a.current_slot;
                if (a.st.replaced) a.st.replaced[r] = -1;
                if (a.st.visible) { a.st.visible[r] = 1; a.st.found[r] = 1; }
                if (a.st.first_kf_id) a.st.first_kf_id[r] = a.current_kf_id;
                uint4 lo, hi;
                sl_load_desc(a.kp.desc + 32 * (cur_first ? e1 : e2), lo, hi);
                uint4 *q = reinterpret_cast<uint4 *>(a.st.desc) + 2 * (size_t)r;
                q[0] = lo; q[1] = hi;
                a.st.point_pool[e1] = r; a.st.registered[e1] = 1;
                a.pair_row[p] = r;
                atomicMax(&a.claim[(size_t)t * a.cap + idx2], (int)p);
                created++;
            }
        }
        running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    for (int s = 32; s > 0; s >>= 1) {
        created += __shfl_xor(created, s);
        dropped += __shfl_xor(dropped, s);
    }
    if (lane == 0) {
        if (created) atomicAdd(&a.stats[NP_C_CREATED], created);
        if (dropped) atomicAdd(&a.stats[NP_C_NO_ROW], dropped);
    }
}

__global__ __launch_bounds__(256) void k_np_link(NewPointsArgs a, long long n_pairs)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    bool lost = false;
    if (p < n_pairs && a.verdict[p] == NP_CREATED) {
        const int t = (int)(p / a.n1), idx2 = a.match12[p];
        if (a.claim[(size_t)t * a.cap + idx2] == (int)p) {
            const size_t e2 = (size_t)a.info[1 + t] + idx2;
            a.st.point_pool[e2] = a.pair_row[p]; a.st.registered[e2] = 1;
        } else {
            lost = true;
        }
    }
    np_tally(&a.stats[NP_C_SHARED], lost);
}

__global__ void k_np_finish(NewPointsArgs a)
{
    if (threadIdx.x < NP_COUNTS) a.counts_dev[threadIdx.x] = a.stats[threadIdx.x];
}

int new_points_chunk() { return NP_CHUNK; }

void launch_new_points_gather(const NewPointsArgs &a, const NewPointsSlots &s, hipStream_t st)
{
    const long long items = std::max<long long>((long long)a.n1 + (long long)a.n_nb * a.cap, 1 + a.n_nb);
    hipLaunchKernelGGL(k_np_gather, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a, s);
}

void launch_new_points_verdict(const NewPointsArgs &a, const NewPointsPoses &p, hipStream_t st)
{
    if (a.n1 <= 0 || p.n <= 0) return;
    hipLaunchKernelGGL(k_np_verdict, dim3((a.n1 + 255) / 256, p.n), dim3(256), 0, st, a, p);
}

// Launch shapes from n1 and n_nb alone.  k_np_scan and k_np_finish always run: they write the zero counts of an empty call.
void launch_new_points_apply(const NewPointsArgs &a, hipStream_t st)
{
    const long long n_pairs = (long long)a.n1 * a.n_nb;
    const int chunks = (int)((n_pairs + NP_CHUNK - 1) / NP_CHUNK);
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_np_own, dim3((a.n1 + 255) / 256), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_np_count, dim3(chunks), dim3(256), 0, st, a, n_pairs);
    }
    hipLaunchKernelGGL(k_np_scan, dim3(1), dim3(NP_SCAN_THREADS), 0, st, a, chunks);
    if (n_pairs > 0) {
        hipLaunchKernelGGL(k_np_write, dim3(chunks), dim3(256), 0, st, a, n_pairs);
        hipLaunchKernelGGL(k_np_link, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, a, n_pairs);
    }
    hipLaunchKernelGGL(k_np_finish, dim3(1), dim3(64), 0, st, a);
}

} // namespace jsorb
