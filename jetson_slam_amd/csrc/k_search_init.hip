// k_search_init.hip - the matcher of Tracking::MonocularInitialization (Tracking.cpp:724-794) on the device:
//   ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)  ORBmatcher.cpp:392-507, with Frame::GetFeaturesInArea
//   (Frame.cpp:641-694) and ComputeThreeMaxima (ORBmatcher.cpp:2097-2138).
// The reference walks F1's keypoints in order on the host.  A point that claims keypoint k records its distance in vMatchedDistance[k], which
// hides k from every LATER point whose distance to k is not smaller - and a later point with a smaller distance takes k away.  Point i therefore
// depends on the claims of the points j < i only, through md_i[k] = min over the j < i that claimed k of their distance (the claims on one
// keypoint have strictly decreasing distances, so the minimum is the last one).  Here:
//   k_init_candidates  SL_LANES lanes per F1 point: the window's grid cells in the reference's order (ix outer, iy inner, a cell's items ascending),
//                      the octave and window filters, the Hamming distance; the first SI_CAP survivors packed (keypoint, distance) in walk order
//                      and the count of all of them.  A point over SI_CAP is rescanned from the grid by the resolver.
//   k_init_resolve     one workgroup.  The points that have candidates, in ascending order, in chunks of SI_CHUNK (one wave's worth of points,
//                      SL_LANES lanes each).  state[k] = md of all FINISHED chunks << 8 | mark.  Inside a chunk the rule is iterated to its fixed
//                      point: every round each point chooses over md = min(finished md, distances of the LOWER points of the chunk that chose k
//                      in the previous round).  The first point of a chunk depends on finished chunks only, so it is final after round 1; point
//                      p of the chunk sees final lower points from round p + 1 on, so it is final after round p + 1: all SI_CHUNK points
//                      after SI_CHUNK rounds, and one more round sees no change: at most SI_CHUNK + 1 rounds per chunk (a chain of displacements
//                      through every point of a chunk needs them all), at least 2.  The mark is the lowest point of the chunk that chose k in
//                      the previous round (SI_FREE: none): a point scans the lower points' choices only for candidates so marked.
//                      Then the claims' last owners (vnMatches21), the rotation histogram over ALL claims, ComputeThreeMaxima, the culling, the
//                      count and vbPrevMatched.
// The window walk, its compaction and the rotation check are k_search_common.h's (walk_window, compact_window; rot_bin, rot_keep).  The chunked
// claim rule is this matcher's own: a later point takes a keypoint away, so it is not claim_resolve's fixed point.
// The contract (include/jsorb.h, jsorb_search_for_initialization_async) is restated in numpy in tests/test_search_init_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef SI_CAP
#define SI_CAP 192                               // candidates kept per F1 point (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define SI_LDS_STATE 12288                       // k_init_resolve keeps state[] in LDS up to this many keypoints (48 KiB)
#define SI_CHUNK 64                              // points per chunk of k_init_resolve (1024 threads / SL_LANES)
#define SI_NONE 511                              // vMatchedDistance = INT_MAX: above every distance (<= 256)
#define SI_FREE 0xff                             // mark: no point of the running chunk chose the keypoint in the previous round
#define SI_PACK(k, d) ((k) << 9 | (d))           // keypoint < 2^18, distance <= 256

int search_init_cap() { return SI_CAP; }

// the window of F1 point i: GetFeaturesInArea(x, y, windowSize, level1, level1)'s cell range with its early returns; false: no candidate at all
struct SiPoint {
    float x, y;
    int x0, x1, y0, y1;
    bool levels;
};
__device__ __forceinline__ bool si_point(const SearchInitArgs &a, int i, SiPoint &p)
{
    const int oct = a.octave[i];
    if (oct > 0) return false;                       // level1 > 0: continue
    p.levels = oct >= 0;                             // bCheckLevels = (minLevel > 0) || (maxLevel >= 0) with minLevel = maxLevel = level1
    p.x = a.prev[i];
    p.y = a.prev[a.n1 + i];
    return sl_cells(a.p, p.x, p.y, a.p.window, p.x0, p.x1, p.y0, p.y1);
}

// keypoint k as a candidate of the point: -1 if a filter drops it, else its Hamming distance
__device__ __forceinline__ int si_candidate(const SearchInitArgs &a, const SiPoint &p, uint4 mlo, uint4 mhi, int k)
{
    const FrameView &f = a.f;
    if (p.levels && f.octave(k) != 0) return -1;      // octave < 0 or > 0 against (minLevel, maxLevel) = (0, 0)
    const float R = a.p.window;
    if (!(fabsf(f.x(k) - p.x) < R && fabsf(f.y(k) - p.y) < R)) return -1;
    uint4 lo, hi;
    sl_load_desc(f.desc + 32 * (size_t)k, lo, hi);
    return SL_HAMMING(lo, hi, mlo, mhi);
}

__global__ __launch_bounds__(256) void k_init_candidates(SearchInitArgs a)
{
    const int lane = threadIdx.x % SL_LANES;
    const int i = blockIdx.x * (256 / SL_LANES) + threadIdx.x / SL_LANES;
    if (i >= a.n1) return;                           // (whole groups of SL_LANES lanes leave together)
    if (lane == 0) a.matches12[i] = -1;
    SiPoint p;
    if (!si_point(a, i, p)) {
        if (lane == 0) a.cand_n[i] = 0;
        return;
    }
    uint4 mlo, mhi;
    sl_load_desc(a.f1_desc + 32 * (size_t)i, mlo, mhi);
    const int count = compact_window<SI_CAP>(a.f.cell_start, a.p.rows, p.x0, p.x1, p.y0, p.y1, a.cand + (size_t)i * SI_CAP, [&](int j) {
        const int k = a.f.cell_items[j], d = si_candidate(a, p, mlo, mhi, k);
        return d >= 0 ? SI_PACK(k, d) : -1;
    });
    if (lane == 0) a.cand_n[i] = count;
}

// a word that other waves of the workgroup update with atomics (state in global memory, owner): read past the vector cache, where a line fetched
// before the atomic could still sit
__device__ __forceinline__ int si_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One workgroup of SI_CHUNK x SL_LANES threads.  state: LDS when the frame's keypoints fit (dynamic LDS of n_kp ints), else global memory.
__global__ __launch_bounds__(1024) void k_init_resolve(SearchInitArgs a, int state_in_lds)
{
    extern __shared__ int s_state[];
    __shared__ int s_k[SI_CHUNK], s_d[SI_CHUNK], s_wave[1024 / 64], s_hist[HISTO_LENGTH + 1], s_keep[HISTO_LENGTH + 1], s_claims, s_owned, s_culled, s_cand, s_over;
    const int tid = threadIdx.x, n1 = a.n1, N = a.f.n_kp;
    int *state = state_in_lds ? s_state : a.state;
    for (int k = tid; k < N; k += 1024) {
        state[k] = SI_NONE << 8 | SI_FREE;
        a.owner[k] = -1;
    }
    if (tid <= HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) { s_claims = 0; s_owned = 0; s_culled = 0; s_cand = 0; s_over = 0; }
    // order[]: the points that have candidates, ascending (the others claim nothing and hide nothing)
    int total = 0, cand = 0, over = 0;
    for (int base = 0; base < n1; base += 1024) {
        const int i = base + tid;
        const int c = i < n1 ? a.cand_n[i] : 0;
        cand += c;
        over += c > SI_CAP;
        const unsigned long long m = __ballot(c > 0);
        if (tid % 64 == 0) s_wave[tid / 64] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < 1024 / 64; w++) {
            if (w < tid / 64) off += s_wave[w];
            total += s_wave[w];
        }
        if (c > 0) a.order[off + __popcll(m & ((1ull << (tid % 64)) - 1))] = i;
        __syncthreads();
    }
    atomicAdd(&s_cand, cand);
    atomicAdd(&s_over, over);
    __syncthreads();

    const int p = tid / SL_LANES, lane = tid % SL_LANES;
    const float ratio = a.p.nn_ratio;
    int rounds = 0;
    for (int base = 0; base < total; base += SI_CHUNK) {
        const int i = base + p < total ? a.order[base + p] : -1;
        const int cnt = i >= 0 ? a.cand_n[i] : 0;
        SiPoint pt;
        uint4 mlo = {0, 0, 0, 0}, mhi = {0, 0, 0, 0};
        if (cnt > SI_CAP) {                          // overflow: the point's lanes walk its window again every round, in the same order
            si_point(a, i, pt);
            sl_load_desc(a.f1_desc + 32 * (size_t)i, mlo, mhi);
        }
        const int *list = a.cand + (size_t)max(i, 0) * SI_CAP;
        if (lane == 0) s_k[p] = -1;
        int prev = -2, prev_d = 0;                   // no choice yet: the first round changes every point
        __syncthreads();
        for (int r = 0; r <= SI_CHUNK; r++) {        // (the bound is never cut short: SI_CHUNK + 1 rounds suffice)
            rounds++;
            // best / second best over the candidates that vMatchedDistance does not hide: the two smallest distances of the multiset, the
            // first in walk order (pos) with the smallest
            unsigned long long best = ~0ull;
            int d1 = INT_MAX, d2 = INT_MAX;
            auto take = [&](int k, int d, int pos) {
                const int w = si_ld(&state[k]);
                int md = w >> 8;
                for (int l = w & SI_FREE; l < p; l++)      // lower points of this chunk chose k in the previous round (rare)
                    if (s_k[l] == k) md = min(md, s_d[l]);
                if (md <= d) return;                 // vMatchedDistance[i2] <= dist
                if (d < d1) {                        // a lane meets its candidates in walk order: a tie never replaces
                    d2 = d1; d1 = d;
                    best = (unsigned long long)d << 36 | (unsigned long long)pos << 18 | (unsigned)k;
                } else if (d < d2) {
                    d2 = d;
                }
            };
            if (cnt <= SI_CAP) {
                for (int t = lane; t < cnt; t += SL_LANES) {
                    const int c = list[t];
                    take(c >> 9, c & 511, t);
                }
            } else {
                walk_window<false>(a.f.cell_start, a.p.rows, pt.x0, pt.x1, pt.y0, pt.y1, lane, SL_LANES, [&](int j, bool) {
                    const int k = a.f.cell_items[j];
                    const int d = si_candidate(a, pt, mlo, mhi, k);
                    if (d >= 0) take(k, d, j);       // the CSR position grows with the walk
                });
            }
            for (int s = SL_LANES / 2; s > 0; s >>= 1) {      // the point's lanes are all here: the two smallest over them
                const unsigned long long ob = __shfl_xor(best, s, SL_LANES);
                const int o1 = __shfl_xor(d1, s, SL_LANES), o2 = __shfl_xor(d2, s, SL_LANES);
                d2 = min(max(d1, o1), min(d2, o2));
                d1 = min(d1, o1);
                best = min(best, ob);
            }
            int k = -1, d = 0;
            if (best != ~0ull && d1 <= a.p.th_low && (float)d1 < (float)d2 * ratio) {      // bestDist <= TH_LOW && bestDist < (float)bestDist2 * mfNNratio
                k = (int)(best & ((1u << 18) - 1));
                d = d1;
            }
            if (!__syncthreads_or(k != prev)) break; // (every thread has read state and s_k by now)
            if (lane == 0 && prev >= 0) atomicOr(&state[prev], SI_FREE);
            __syncthreads();
            if (lane == 0) {
                s_k[p] = k;
                s_d[p] = d;
                if (k >= 0) atomicMin(&state[k], (si_ld(&state[k]) & ~SI_FREE) | p);      // the finished md stays, the lowest p wins the mark
            }
            prev = k;
            prev_d = d;
            __syncthreads();
        }
        // the chunk is final: its claims join the finished state
        if (lane == 0 && prev >= 0) atomicOr(&state[prev], SI_FREE);
        __syncthreads();
        if (lane == 0 && prev >= 0) {
            atomicMin(&state[prev], prev_d << 8 | SI_FREE);      // claims on one keypoint have decreasing distances: the last is the smallest
            atomicMax(&a.owner[prev], i);                         // vnMatches21: the last claimant
            a.matches12[i] = prev;                                // (before displacement and culling: settled below)
        }
        __syncthreads();
    }

    // every claim sits in its rotation bin, displaced or not; a claim stands while its point still owns the keypoint
    const bool rot = a.p.check_orientation != 0;
    int claims = 0, owned = 0;
    for (int i = tid; i < n1; i += 1024) {
        const int k = a.matches12[i];
        if (k < 0) continue;
        claims++;
        owned += si_ld(&a.owner[k]) == i;
        if (rot) atomicAdd(&s_hist[rot_bin(a.angle[i], a.f.angle(k))], 1);
    }
    atomicAdd(&s_claims, claims);
    atomicAdd(&s_owned, owned);
    __syncthreads();
    if (tid == 0) {
        const ThreeMaxima t = rot_keep(s_hist, s_keep, rot);
        a.stats[4] = t.ind1; a.stats[5] = t.ind2; a.stats[6] = t.ind3;
    }
    __syncthreads();
    int culled = 0;
    for (int i = tid; i < n1; i += 1024) {
        const int k = a.matches12[i];
        if (k < 0) continue;
        int m = si_ld(&a.owner[k]) == i ? k : -1;            // vnMatches12[vnMatches21[bestIdx2]] = -1
        if (m >= 0 && rot && !s_keep[rot_bin(a.angle[i], a.f.angle(k))]) {
            m = -1;                                  // a culled bin: vnMatches12[idx1] = -1, nmatches--
            culled++;
        }
        a.matches12[i] = m;
        if (m >= 0) {                                // vbPrevMatched[i1] = F2.mvKeysUn[vnMatches12[i1]].pt
            a.prev[i] = a.f.x(m);
            a.prev[n1 + i] = a.f.y(m);
        }
    }
    atomicAdd(&s_culled, culled);
    if (a.matches21)
        for (int k = tid; k < N; k += 1024) a.matches21[k] = si_ld(&a.owner[k]);
    __syncthreads();
    if (tid == 0) {
        *a.n_matches = s_owned - s_culled;
        a.stats[0] = rounds;
        a.stats[1] = s_cand;
        a.stats[2] = s_over;
        a.stats[3] = s_claims - s_owned;             // every claim on a keypoint but its first took it from an earlier point
    }
}

// mvKeysUn's points of one image as x[n] y[n]: the undistorted coordinates, or the keypoints as floats
__global__ __launch_bounds__(256) void k_init_keys_un(const int32_t *soa, const float *xy_un, int n, float *dst)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n) return;
    dst[t] = xy_un ? xy_un[t] : (float)soa[t];
}

void launch_init_candidates(const SearchInitArgs &a, hipStream_t s)
{
    if (a.n1 <= 0) return;
    const int per_block = 256 / SL_LANES;
    hipLaunchKernelGGL(k_init_candidates, dim3((a.n1 + per_block - 1) / per_block), dim3(256), 0, s, a);
}

void launch_init_resolve(const SearchInitArgs &a, hipStream_t s)
{
    const int lds = a.f.n_kp <= SI_LDS_STATE;
    hipLaunchKernelGGL(k_init_resolve, dim3(1), dim3(1024), lds ? (size_t)a.f.n_kp * sizeof(int) : 0, s, a, lds);
}

void launch_init_keys_un(const int32_t *soa, const float *xy_un, int n, float *dst, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_init_keys_un, dim3((2 * n + 255) / 256), dim3(256), 0, s, soa, xy_un, n, dst);
}

} // namespace jsorb
