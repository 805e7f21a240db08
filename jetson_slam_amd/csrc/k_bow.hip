// k_bow.hip - the bag-of-words side of Tracking::TrackReferenceKeyFrame (Tracking.cpp:919-932) and Tracking::Relocalization (:1954-2004) on the
// device:
//   Frame::ComputeBoW (Frame.cpp:709-716) -> TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
//     (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1217-1259), per descriptor: k_bow_transform
//   ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (ORBmatcher.cpp:146-275) with ComputeThreeMaxima (:2097-2138), for several
//     keyframes against one frame: k_bow_group, k_bow_match, k_bow_resolve
// k_bow_transform  BW_LANES lanes per descriptor.  The descent of :1229-1258: at every level each lane takes the children c, c + BW_LANES, ... of the
//                  node (their descriptors lie in child order, 32 bytes apart: two 16-byte loads per child), the key distance << 22 | child position
//                  is reduced with a minimum over the lanes - the lowest position wins a tie, as the strict < of :1244 lets the first child win -
//                  and all lanes go on from the winner.  No LDS, no barrier.
// k_bow_group      one workgroup per side (workgroup 0: the frame, workgroup 1 + i: keyframe i): the keys node << 18 | index of the keypoints that
//                  are in a node, sorted ascending (a bitonic network whose exchanges all put the minimum at the lower index, so that the padding
//                  above n never moves and is never stored): a node's keypoints are one run of the array, in ascending index.  In LDS up to
//                  BW_SORT_LDS keys, in place in global memory above.
// k_bow_match      one wave per (keyframe, node present on both sides): the wave at the first position of a keyframe's run finds the frame's run of
//                  the same node by bisection.  Lane l owns the frame entries l, l + 64, ...: the first BW_NODE_REGS of them with their descriptor
//                  and claimed flag in registers, the rest read again for every keyframe keypoint (their claimed flag is match_kf itself, written
//                  by the owning lane).  The keyframe's keypoints of the node are taken in turn (:174-238); the wave reduces to (bestDist1, first
//                  position with it, bestDist2) and the owner of the winning entry claims it.  Every keypoint is in at most one node, so no two
//                  waves touch the same entry of match_kf and no order of nodes can change a result.
// k_bow_resolve    one workgroup per keyframe: the rotation histogram of the claims, ComputeThreeMaxima, the culling and the count (:254-272).
// The rotation check, the key layout and the bisection are k_search_common.h's (rot_bin, rot_keep; BW_IDX, bw_lower_bound).
// The contract (include/jsorb.h, jsorb_bow_transform_async / jsorb_search_by_bow_async) is restated in numpy in tests/test_bow_host.py.
#include <climits>

#include "jsorb_launch.h"
#include "k_search_common.h"

namespace jsorb {

#ifndef BW_NODE_REGS
#define BW_NODE_REGS 2                           // frame entries of a node a lane of k_bow_match keeps in registers (a test build lowers it: build.py VARIANTS)
#endif
#define BW_LANES 16                              // lanes per descriptor in k_bow_transform
#ifndef BW_SORT_LDS
#define BW_SORT_LDS 4096                         // k_bow_group sorts up to this many keys in LDS (32 KiB; a test build lowers it: build.py VARIANTS)
#endif
#define BW_POS 22                                // bits of a child position in k_bow_transform's key (max_children < 2^22)

int bow_node_regs() { return BW_NODE_REGS; }
int bow_sort_lds() { return BW_SORT_LDS; }

__global__ __launch_bounds__(256) void k_bow_transform(BowVocab v, const uint8_t *desc, size_t desc_stride, const int *counts, int counts_stride,
                                                       int n_fixed, int32_t *word, int32_t *node, size_t out_stride, int *n_shallow)
{
    const int img = blockIdx.y, lane = threadIdx.x % BW_LANES;
    const int i = blockIdx.x * (256 / BW_LANES) + threadIdx.x / BW_LANES;
    const int n = counts ? counts[(size_t)img * counts_stride] : n_fixed;
    const bool on = i < n;                           // (whole groups of BW_LANES lanes; the loop below has a wave-uniform trip count)
    uint4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
    if (on) sl_load_desc(desc + (size_t)img * desc_stride + 32 * (size_t)i, lo, hi);
    int cur = 0, nid = 0, level = 0;                 // final_id = 0 (root), current_level = 0
    bool leaf = !on;
    for (int l = 0; l < v.depth_L; l++) {            // the tree is no deeper than depth_L (jsorb_vocabulary_create checked it)
        if (!__any(!leaf)) break;
        unsigned key = ~0u;
        int b = 0;
        if (!leaf) {
            b = v.child_start[cur];
            const int e = v.child_start[cur + 1];
            leaf = b == e;                           // isLeaf(): no children
            for (int c = b + lane; c < e; c += BW_LANES) {
                uint4 clo, chi;
                sl_load_desc(v.child_desc + 32 * (size_t)c, clo, chi);
                const unsigned d = SL_HAMMING(clo, chi, lo, hi);
                key = min(key, d << BW_POS | (unsigned)(c - b));      // a lane meets its children in ascending position
            }
        }
        for (int s = BW_LANES / 2; s > 0; s >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, s, BW_LANES));
        if (!leaf) {
            cur = v.children[b + (int)(key & ((1u << BW_POS) - 1))];
            level++;
            if (level == v.nid_level) nid = cur;     // :1251-1252
        }
    }
    if (!on || lane != 0) return;
    const bool shallow = v.nid_level > 0 && level < v.nid_level;     // the leaf lies above the node level: the reference leaves nid unset
    if (v.nid_level <= 0) nid = 0;                   // :1227
    else if (shallow) nid = cur;
    if (shallow && n_shallow) atomicAdd(n_shallow, 1);
    if (!v.live[cur]) nid = -1;                      // weight not > 0: a stopped word is in no FeatureVector entry (:1157)
    if (word) word[(size_t)img * out_stride + i] = v.word[cur];
    if (node) node[(size_t)img * out_stride + i] = nid;
}

// 8-byte accesses to keys that other waves of the workgroup exchange in global memory: past the vector cache on both sides
template <bool G> __device__ __forceinline__ unsigned long long bw_ld(const unsigned long long *p)
{
    if (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool G> __device__ __forceinline__ void bw_st(unsigned long long *p, unsigned long long x)
{
    if (G) __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = x;
}

// keys[0 .. n) ascending.  Merges of size 2, 4, ...: the first step of a merge pairs i with its mirror image in the block, the following ones
// with i ^ stride; every exchange leaves the minimum at the lower index, so keys at or above n (all larger than any key) stay where they are.
template <bool G> __device__ void bw_sort(unsigned long long *keys, int n)
{
    for (int size = 2; size / 2 < n; size <<= 1) {
        for (int stride = size / 2; stride > 0; stride >>= 1) {
            const bool first = stride == size / 2;
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int l = first ? i ^ (size - 1) : i ^ stride;
                if (l > i && l < n) {
                    const unsigned long long a = bw_ld<G>(keys + i), b = bw_ld<G>(keys + l);
                    if (b < a) { bw_st<G>(keys + i, b); bw_st<G>(keys + l, a); }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(1024) void k_bow_group(BowMatchArgs a)
{
    __shared__ unsigned long long s_keys[BW_SORT_LDS];
    const int side = blockIdx.x;                     // 0: the frame, 1 + i: keyframe i
    const int off = side ? a.kf_start[side - 1] : 0;
    const int n = side ? a.kf_start[side] - off : a.N;
    const int32_t *src = side ? a.kf_node + off : a.f_node;
    unsigned long long *dst = side ? a.kf_sorted + off : a.f_sorted;
    if (n <= 0) return;
    const bool lds = n <= BW_SORT_LDS;
    unsigned long long *keys = lds ? s_keys : dst;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int v = src[i];
        const unsigned long long k = v >= 0 ? (unsigned long long)v << BW_IDX | (unsigned)i : BW_NOKEY;
        if (lds) keys[i] = k; else bw_st<true>(keys + i, k);
    }
    __syncthreads();
    if (lds) {
        bw_sort<false>(keys, n);
        for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = keys[i];
    } else {
        bw_sort<true>(keys, n);
    }
}

__global__ __launch_bounds__(256) void k_bow_match(BowMatchArgs a)
{
    const int lane = threadIdx.x % 64, kf = blockIdx.y;
    const int p = blockIdx.x * 4 + threadIdx.x / 64;
    const int off = a.kf_start[kf], len = a.kf_start[kf + 1] - off;
    if (p >= len) return;
    const unsigned long long *ks = a.kf_sorted + off;
    const unsigned long long head = ks[p];
    if (head == BW_NOKEY) return;
    const unsigned long long v = head >> BW_IDX;     // the node
    if (p > 0 && ks[p - 1] >> BW_IDX == v) return;   // not the first keypoint of the node: the wave at the first one takes them all
    const int fb = bw_lower_bound(a.f_sorted, a.N, v << BW_IDX), m = bw_lower_bound(a.f_sorted, a.N, (v + 1) << BW_IDX) - fb;
    if (m == 0) return;                              // the node is not in the frame's FeatureVector (:243-250)
    const int pe = bw_lower_bound(ks, len, (v + 1) << BW_IDX);
    const unsigned long long *fs = a.f_sorted + fb;
    int32_t *row = a.match_kf + (size_t)kf * a.N;
    // the lane's first entries: index, descriptor, claimed flag
    int kreg[BW_NODE_REGS];
    uint4 rlo[BW_NODE_REGS], rhi[BW_NODE_REGS];
    unsigned claimed = 0;
#pragma unroll
    for (int r = 0; r < BW_NODE_REGS; r++) {
        const int t = lane + 64 * r;
        kreg[r] = t < m ? (int)(fs[t] & BW_IDX_MASK) : -1;
        if (t < m) sl_load_desc(a.desc + 32 * (size_t)kreg[r], rlo[r], rhi[r]);
        else { rlo[r] = make_uint4(0, 0, 0, 0); rhi[r] = rlo[r]; }
    }
    const float ratio = a.p.nn_ratio;
    int n_dist = 0;
    for (int q = p; q < pe; q++) {                   // vIndicesKF in ascending index (:174)
        const int j = (int)(ks[q] & BW_IDX_MASK);
        if (!a.kf_valid[off + j]) continue;          // !pMP || pMP->isBad() (:178-184)
        uint4 klo, khi;
        sl_load_desc(a.kf_desc + 32 * (size_t)(off + j), klo, khi);
        // bestDist1 / bestDist2 from 256 over the entries not yet matched (:188-213): the two smallest of the multiset, the first position with the smallest
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
        for (int r = 0; r < BW_NODE_REGS; r++)
            if (kreg[r] >= 0 && !(claimed >> r & 1)) take(SL_HAMMING(rlo[r], rhi[r], klo, khi), lane + 64 * r);
        for (int t = lane + 64 * BW_NODE_REGS; t < m; t += 64) {
            const int k = (int)(fs[t] & BW_IDX_MASK);
            if (row[k] >= 0) continue;               // vpMapPointMatches[realIdxF] (:196): written by this lane, if at all
            uint4 lo, hi;
            sl_load_desc(a.desc + 32 * (size_t)k, lo, hi);
            take(SL_HAMMING(lo, hi, klo, khi), t);
        }
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned ob = (unsigned)__shfl_xor((int)best, s);
            const int o1 = __shfl_xor(d1, s), o2 = __shfl_xor(d2, s);
            d2 = min(max(d1, o1), min(d2, o2));
            d1 = min(d1, o1);
            best = min(best, ob);
        }
        if (best == ~0u || d1 > a.p.th_low || !((float)d1 < ratio * (float)d2)) continue;      // :215-217 (no entry below 256: bestIdxF = -1)
        const int t = (int)(best & BW_IDX_MASK);
        if (t % 64 == lane) {                        // the owner of the entry: vpMapPointMatches[bestIdxF] = pMP
            int k = -1;
#pragma unroll
            for (int r = 0; r < BW_NODE_REGS; r++)
                if (t == lane + 64 * r) { k = kreg[r]; claimed |= 1u << r; }
            if (k < 0) k = (int)(fs[t] & BW_IDX_MASK);
            row[k] = j;
        }
    }
    for (int s = 32; s > 0; s >>= 1) n_dist += __shfl_xor(n_dist, s);
    if (lane == 0) {
        atomicAdd(&a.stats[0], 1);
        atomicAdd(&a.stats[1], n_dist);
        atomicMax(&a.stats[2], m);
    }
}

__global__ __launch_bounds__(256) void k_bow_resolve(BowMatchArgs a)
{
    __shared__ int s_hist[HISTO_LENGTH + 1], s_keep[HISTO_LENGTH + 1], s_claims, s_culled;
    const int kf = blockIdx.x, tid = threadIdx.x, N = a.N;
    const int off = a.kf_start[kf];
    if (a.kf_start[kf + 1] - off <= 0) return;       // an empty keyframe: its row and count were cleared with the others
    int32_t *row = a.match_kf + (size_t)kf * N;
    const bool rot = a.p.check_orientation != 0;
    if (tid <= HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) { s_claims = 0; s_culled = 0; }
    __syncthreads();
    int claims = 0;
    for (int k = tid; k < N; k += 256) {
        const int j = row[k];
        if (j < 0) continue;
        claims++;
        if (rot) atomicAdd(&s_hist[rot_bin(a.kf_angle[off + j], __int_as_float(a.soa[3 * (size_t)N + k]))], 1);
    }
    atomicAdd(&s_claims, claims);
    __syncthreads();
    if (tid == 0) {
        const ThreeMaxima t = rot_keep(s_hist, s_keep, rot);
        if (kf == 0) { a.stats[3] = t.ind1 + 1; a.stats[4] = t.ind2 + 1; a.stats[5] = t.ind3 + 1; }      // (0: none - the cleared state)
    }
    __syncthreads();
    if (rot) {
        int culled = 0;
        for (int k = tid; k < N; k += 256) {
            const int j = row[k];
            if (j < 0) continue;
            if (!s_keep[rot_bin(a.kf_angle[off + j], __int_as_float(a.soa[3 * (size_t)N + k]))]) {
                row[k] = -1;                         // :268-269
                culled++;
            }
        }
        atomicAdd(&s_culled, culled);
        __syncthreads();
    }
    if (tid == 0) a.n_matches[kf] = s_claims - s_culled;
}

void launch_bow_transform(const BowVocab &v, const uint8_t *desc, size_t desc_stride, const int *counts, int counts_stride, int n, int32_t *word,
                          int32_t *node, size_t out_stride, int *n_shallow, int n_images, hipStream_t s)
{
    if (n <= 0 || n_images <= 0) return;
    const int per_block = 256 / BW_LANES;
    hipLaunchKernelGGL(k_bow_transform, dim3((n + per_block - 1) / per_block, n_images), dim3(256), 0, s, v, desc, desc_stride, counts, counts_stride, n,
                       word, node, out_stride, n_shallow);
}

void launch_bow_group(const BowMatchArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_bow_group, dim3(1 + a.n_kf), dim3(1024), 0, s, a); }

void launch_bow_match(const BowMatchArgs &a, hipStream_t s)
{
    int longest = 0;
    for (int i = 0; i < a.n_kf; i++) longest = max(longest, a.kf_start[i + 1] - a.kf_start[i]);
    if (longest <= 0) return;
    hipLaunchKernelGGL(k_bow_match, dim3((longest + 3) / 4, a.n_kf), dim3(256), 0, s, a);
}

void launch_bow_resolve(const BowMatchArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_bow_resolve, dim3(a.n_kf), dim3(256), 0, s, a); }

} // namespace jsorb
