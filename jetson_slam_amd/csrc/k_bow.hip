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
//                  the same node by bisection.  The search itself is k_search_common.h's node_walk, shared with k_loop_bow_match: the frame's run
//                  is the claimed side (the first BW_NODE_REGS entries of a lane in registers; past them the claimed flag is match_kf itself,
//                  written by the owning lane), the keyframe's keypoints of the node are the outer walk (:174-238), accepted at bestDist1 <=
//                  th_low.  Every keypoint is in at most one node, so no two waves touch the same entry of match_kf and no order of nodes can
//                  change a result.
// k_bow_resolve    one workgroup per keyframe: the rotation histogram of the claims, ComputeThreeMaxima, the culling and the count (:254-272):
//                  k_search_common.h's row_resolve, shared with k_tri_resolve, with the keyframe's angle first.
// The key layout and the bisection are k_search_common.h's too (BW_IDX, bw_lower_bound).
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
    // the frame's run is the claimed side (vpMapPointMatches[realIdxF], :196 - match_kf itself past the register cap), the keyframe's keypoints of
    // the node the outer walk (vIndicesKF in ascending index, :174)
    struct {
        const BowMatchArgs &a;
        const unsigned long long *fs, *ks;
        int32_t *row;
        int off;
        __device__ int index(int t) const { return (int)(fs[t] & BW_IDX_MASK); }
        __device__ const uint8_t *desc(int k) const { return a.desc + 32 * (size_t)k; }
        __device__ bool hidden_at_load(int) const { return false; }
        __device__ bool hidden_late(int k) const { return row[k] >= 0; }
        __device__ bool outer(int q, int &j, uint4 &lo, uint4 &hi) const
        {
            j = (int)(ks[q] & BW_IDX_MASK);
            if (!a.kf_valid[off + j]) return false;  // !pMP || pMP->isBad() (:178-184)
            sl_load_desc(a.kf_desc + 32 * (size_t)(off + j), lo, hi);
            return true;
        }
        __device__ bool accept(int d1) const { return d1 <= a.p.th_low; }      // :215
        __device__ void claim(int k, int j, bool) const { row[k] = j; }        // vpMapPointMatches[bestIdxF] = pMP
    } w{a, fs, ks, row, off};
    int n_dist = node_walk<BW_NODE_REGS>(w, lane, m, p, pe, a.p.nn_ratio);
    for (int s = 32; s > 0; s >>= 1) n_dist += __shfl_xor(n_dist, s);
    if (lane == 0) {
        atomicAdd(&a.stats[0], 1);
        atomicAdd(&a.stats[1], n_dist);
        atomicMax(&a.stats[2], m);
    }
}

__global__ __launch_bounds__(256) void k_bow_resolve(RowResolveArgs a)
{
    // :254-272; the keyframe's angle comes first (rot = kf angle - frame angle)
    row_resolve(a, [&](int k, int j) { return rot_bin(a.kf_angle[j], a.row_angle[k]); }, a.kept, a.n);
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

void launch_bow_resolve(const RowResolveArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_bow_resolve, dim3(a.n_kf), dim3(256), 0, s, a); }

} // namespace jsorb
