// k_kfdb.hip - the keyframe database's BoW queries on the device (the contract: include/jsorb.h, jsorb_keyframe_database_*): DBoW2's BowVector fold
//   (BowVector.cpp:34-84 behind TemplatedVocabulary.h:1148-1193), L1Scoring::score (ScoringObject.cpp:23-68) and KeyFrameDatabase's
//   DetectLoopCandidates / DetectRelocalizationCandidates (KeyFrameDatabase.cpp:80-313).  All `double` sums run in the reference's order.
// k_kfdb_bow_vector  one workgroup: the word ids as 32-bit keys (a stopped or out-of-range id: the key above all others), sorted in LDS up to
//                    KD_SORT_LDS of them and in global scratch beyond; the run heads are the vector's entries (ordered compaction by ballot);
//                    a head's value is w added to itself run - 1 times; the norm is summed by wave 0, 64 values a step in registers, added in
//                    lane order; every value is divided by it.
// k_kfdb_add         copies a device BowVector into the pool and gives the slot the KeyFrame constructor's query state.
// kd_common          one wave per keyframe: lanes take 64 consecutive entries a step and binary-search the query (staged in LDS up to
//                    KD_QUERY_LDS entries, in global memory beyond); the ballot's popcount is the count of common words, its first lane the lowest
//                    common word, and the score's terms are added over the hit lanes in ascending order - which is the merge walk's order.
// k_kfdb_score       the minScore loop (LoopClosing.cpp:129-143): one workgroup, a wave per listed slot, the minimum with `<` from 1.0f.
// k_kfdb_common      per present slot: the common words, the persistent state's update (:90-108 / :211-226), the list key and the score.
// k_kfdb_rank        a listed slot's place in lKFsSharingWords = the number of smaller keys (keys are distinct: the sequence number); the slots
//                    above minCommonWords get their score (:137-139 / :253-254), those the query keeps (:140) are flagged.
// k_kfdb_accumulate  per kept entry the covisibility walk (:152-177 / :266-291) in row order; bestAccScore as the maximum of (value, earliest).
// k_kfdb_emit        one workgroup: retain (:180), the first list position per best slot (:191), the ordered compaction (:193).
// Kernels hand data to each other only across launches.  Inside a workgroup, data other waves wrote to global memory is read and written by
// agent-scope relaxed atomics (k_bow.hip's bw_ld / bw_st), behind a barrier.
#include "jsorb_launch.h"

#include <limits.h>

#ifndef KD_QUERY_LDS
#define KD_QUERY_LDS 4096                        // query entries staged in LDS (48 KiB; a test build lowers it: build.py VARIANTS)
#endif
#ifndef KD_SORT_LDS
#define KD_SORT_LDS 8192                         // word ids k_kfdb_bow_vector sorts in LDS (32 KiB)
#endif

namespace jsorb {

static_assert(KD_QUERY_LDS >= 1 && KD_QUERY_LDS * 12 <= 48 * 1024 && KD_SORT_LDS >= 1 && KD_SORT_LDS * 4 <= 32 * 1024, "the staged arrays fit LDS");

#define KD_NOKEY 0xffffffffu

template <bool G, class T> __device__ __forceinline__ T kd_ld(const T *p)
{
    if (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool G, class T> __device__ __forceinline__ void kd_st(T *p, T x)
{
    if (G) __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = x;
}
__device__ __forceinline__ double kd_ld_f64(const double *p)
{
    return __longlong_as_double(__hip_atomic_load(reinterpret_cast<const long long *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void kd_st_f64(double *p, double x)
{
    __hip_atomic_store(reinterpret_cast<long long *>(p), __double_as_longlong(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lane l's value for every lane, l wave-uniform: two v_readlane_b32 (a __shfl goes through LDS, ~4x the latency in a chain of dependent adds)
__device__ __forceinline__ double kd_lane(double v, int l)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

// k_bow.hip's bw_sort on 32-bit keys: keys[0 .. n) ascending, keys at or above n untouched
template <bool G> __device__ void kd_sort(uint32_t *keys, int n)
{
    for (int size = 2; size / 2 < n; size <<= 1) {
        for (int stride = size / 2; stride > 0; stride >>= 1) {
            const bool first = stride == size / 2;
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                const int l = first ? i ^ (size - 1) : i ^ stride;
                if (l > i && l < n) {
                    const uint32_t a = kd_ld<G>(keys + i), b = kd_ld<G>(keys + l);
                    if (b < a) { kd_st<G>(keys + i, b); kd_st<G>(keys + l, a); }
                }
            }
            __syncthreads();
        }
    }
}

// The ordered compaction's step for up to 1024 threads: the number of set flags below this thread in the workgroup plus *s_base, which then
// advances by the workgroup's total.  s_wsum: 16 words.
__device__ __forceinline__ int kd_block_offset(bool flag, int *s_wsum, int *s_base)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) s_wsum[wave] = __popcll(m);
    __syncthreads();
    int o = *s_base;
    for (int w = 0; w < wave; w++) o += s_wsum[w];
    o += __popcll(m & ((1ull << lane) - 1));
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < waves; w++) t += s_wsum[w];
        *s_base += t;
    }
    __syncthreads();
    return o;
}

template <bool G> __device__ void kd_bow_vector(const uint32_t *keys, int n, const double *weight, int32_t *bow_word, double *bow_value, int32_t *bow_n,
                                                int *s_wsum, int *s_base, double *s_norm)
{
    if (threadIdx.x == 0) *s_base = 0;
    __syncthreads();
    for (int b = 0; b < n; b += blockDim.x) {
        const int i = b + threadIdx.x;
        const uint32_t k = i < n ? kd_ld<G>(keys + i) : KD_NOKEY;
        const bool head = k != KD_NOKEY && (i == 0 || kd_ld<G>(keys + i - 1) != k);
        const int o = kd_block_offset(head, s_wsum, s_base);
        if (head) {
            int lo = i + 1, hi = n;                              // the run's end: the first key above k
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (kd_ld<G>(keys + mid) <= k) lo = mid + 1; else hi = mid;
            }
            const double w = weight[k];
            double v = w;
            for (int r = lo - i; r > 1; r--) v += w;             // BowVector::addWeight, once per further occurrence
            bow_word[o] = (int32_t)k;
            kd_st_f64(bow_value + o, v);
        }
    }
    __syncthreads();                                            // the heads' values are stored: wave 0 reads them all
    const int m = *s_base;
    if (threadIdx.x < 64) {                                    // BowVector::normalize(L1): norm += fabs(value) in ascending word order
        double norm = 0.0;
        double next = (int)threadIdx.x < m ? fabs(kd_ld_f64(bow_value + threadIdx.x)) : 0.0;
        for (int b = 0; b < m; b += 64) {
            const double v = next;                              // the following 64 values are on their way while these are added
            next = b + 64 + (int)threadIdx.x < m ? fabs(kd_ld_f64(bow_value + b + 64 + threadIdx.x)) : 0.0;
            const int cnt = min(64, m - b);
            for (int l = 0; l < cnt; l++) norm += kd_lane(v, l);
        }
        if (threadIdx.x == 0) *s_norm = norm;
    }
    __syncthreads();
    const double norm = *s_norm;
    if (norm > 0.0)
        for (int j = threadIdx.x; j < m; j += blockDim.x) bow_value[j] = kd_ld_f64(bow_value + j) / norm;
    if (threadIdx.x == 0) *bow_n = m;
}

__global__ __launch_bounds__(1024) void k_kfdb_bow_vector(const int32_t *word_id, int n, const double *weight, int n_words, uint32_t *scratch,
                                                          int32_t *bow_word, double *bow_value, int32_t *bow_n)
{
    __shared__ uint32_t s_keys[KD_SORT_LDS];
    __shared__ int s_wsum[16], s_base;
    __shared__ double s_norm;
    const bool lds = n <= KD_SORT_LDS;
    uint32_t *keys = lds ? s_keys : scratch;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int id = word_id[i];
        const uint32_t k = (unsigned)id < (unsigned)n_words && weight[id] > 0 ? (uint32_t)id : KD_NOKEY;      // TemplatedVocabulary.h:1157
        if (lds) keys[i] = k; else kd_st<true>(keys + i, k);
    }
    __syncthreads();
    if (lds) {
        kd_sort<false>(keys, n);
        kd_bow_vector<false>(keys, n, weight, bow_word, bow_value, bow_n, s_wsum, &s_base, &s_norm);
    } else {
        kd_sort<true>(keys, n);
        kd_bow_vector<true>(keys, n, weight, bow_word, bow_value, bow_n, s_wsum, &s_base, &s_norm);
    }
}

__device__ __forceinline__ int kd_count(const KfdbVector &v)
{
    return min(max(*v.n, 0), v.cap);
}

__global__ __launch_bounds__(256) void k_kfdb_add(KfdbState st, int slot, uint32_t seq, int off, KfdbVector v)
{
    const int n = kd_count(v);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        st.pool_word[off + i] = v.word[i];
        st.pool_value[off + i] = v.value[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st.present[slot] = 1; st.off[slot] = off; st.len[slot] = n; st.seq[slot] = seq;
        st.loop_query[slot] = 0; st.reloc_query[slot] = 0;      // KeyFrame.cpp:39
        st.loop_words[slot] = 0; st.reloc_words[slot] = 0;
        st.loop_score[slot] = 0.0f; st.reloc_score[slot] = 0.0f;
    }
}

// the query in LDS when it fits `lds_entries` (values first: 8-byte aligned), else where it is
struct KdQuery {
    const int32_t *w;
    const double *v;
    int n;
};
__device__ __forceinline__ KdQuery kd_stage(const KfdbVector &q, int lds_entries, char *smem)
{
    KdQuery r{q.word, q.value, kd_count(q)};
    if (r.n <= lds_entries) {
        double *s_v = reinterpret_cast<double *>(smem);
        int32_t *s_w = reinterpret_cast<int32_t *>(smem + 8 * (size_t)lds_entries);
        for (int i = threadIdx.x; i < r.n; i += blockDim.x) { s_v[i] = q.value[i]; s_w[i] = q.word[i]; }
        r.w = s_w; r.v = s_v;
    }
    __syncthreads();
    return r;
}

struct KdHit {
    int c, first;                                // words in common, the lowest of them
    double sum;                                  // ScoringObject.cpp:41 over them, ascending
};
// by a whole wave; every lane returns the same
__device__ __forceinline__ KdHit kd_common(const KfdbState &st, int slot, const KdQuery &q)
{
    const int lane = threadIdx.x & 63;
    KdHit h{0, -1, 0.0};
    const int off = st.off[slot], n = st.len[slot];
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        bool hit = false;
        double t = 0.0;
        int w = 0;
        if (i < n) {
            w = st.pool_word[off + i];
            int lo = 0, hi = q.n;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (q.w[mid] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < q.n && q.w[lo] == w) {
                hit = true;
                const double vi = q.v[lo], wi = st.pool_value[off + i];
                t = fabs(vi - wi) - fabs(vi) - fabs(wi);
            }
        }
        unsigned long long m = __ballot(hit);
        if (m) {
            if (h.c == 0) h.first = __shfl(w, __ffsll((long long)m) - 1);
            h.c += __popcll(m);
            while (m) {
                const int l = __ffsll((long long)m) - 1;
                m &= m - 1;
                h.sum += kd_lane(t, l);
            }
        }
    }
    return h;
}

__global__ __launch_bounds__(1024) void k_kfdb_score(KfdbScoreArgs a, int lds_entries)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float s_min[16];
    __shared__ int s_idx[16];
    const KdQuery q = kd_stage(a.q, lds_entries, smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float best = 1.0f;
    int best_j = INT_MAX;
    for (int j = wave; j < a.n_slots; j += 16) {
        const int s = a.slot_list[j];
        double d = -1.0;
        const bool present = (unsigned)s < (unsigned)a.st.slots && a.st.present[s];
        if (present) d = -kd_common(a.st, s, q).sum / 2.0;
        const float f = (float)d;
        if (lane == 0) {
            a.score[j] = f;
            if (a.score_f64) a.score_f64[j] = d;
        }
        if (present && f < best) { best = f; best_j = j; }
    }
    if (lane == 0) { s_min[wave] = best; s_idx[wave] = best_j; }
    __syncthreads();
    if (threadIdx.x == 0) {                                     // the first of the values that compare equal to the least: what `<` in list order keeps
        float m = 1.0f;
        int mj = -1;
        for (int w = 0; w < 16; w++)
            if (s_min[w] < m || (s_min[w] == m && s_idx[w] < mj)) { m = s_min[w]; mj = s_idx[w]; }
        *a.min_score = m;
    }
}

// control words of a query
enum { KC_LISTED = 0, KC_MAXW, KC_SCORED, KC_KEPT, KC_BESTKEY /* 2 words */, KC_CAND = 6, KC_MINW, KC_BESTACC };

__device__ __forceinline__ int kd_min_words(int maxw) { return (int)((float)maxw * 0.8f); }          // :124 / :239, one float product
__device__ __forceinline__ float kd_start(const KfdbQueryArgs &a) { return a.reloc ? 0.0f : a.min_score_dev ? *a.min_score_dev : a.min_score; }
// (value, position) so that the largest key is the largest value, and among values that compare equal the earliest position (-1: the start)
__device__ __forceinline__ unsigned long long kd_acc_key(float v, int pos)
{
    if (v == 0.0f) v = 0.0f;
    const unsigned b = __float_as_uint(v);
    return (unsigned long long)(b & 0x80000000u ? ~b : b | 0x80000000u) << 32 | (0xffffffffu - (unsigned)(pos + 1));
}

__global__ __launch_bounds__(256) void k_kfdb_common(KfdbQueryArgs a, int lds_entries)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KdQuery q = kd_stage(a.q, lds_entries, smem);
    const int lane = threadIdx.x & 63;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < a.st.slots; s += gridDim.x * 4) {
        unsigned long long key = ~0ull;
        if (a.st.present[s]) {
            const KdHit h = kd_common(a.st, s, q);
            if (h.c > 0 && lane == 0) {
                bool listed = false;
                if (a.reloc) {
                    if (a.st.reloc_query[s] != a.id) { a.st.reloc_query[s] = a.id; a.st.reloc_words[s] = h.c; listed = true; }
                    else a.st.reloc_words[s] += h.c;
                } else if (a.st.loop_query[s] != a.id) {
                    if (a.connected && a.connected[s]) a.st.loop_words[s] = 1;         // reset at every encounter, then incremented
                    else { a.st.loop_query[s] = a.id; a.st.loop_words[s] = h.c; listed = true; }
                } else a.st.loop_words[s] += h.c;
                if (listed) {
                    key = (unsigned long long)(unsigned)h.first << 32 | a.st.seq[s];
                    a.tscore[s] = (float)(-h.sum / 2.0);
                    atomicAdd(&a.ctrl[KC_LISTED], 1);
                    atomicMax(&a.ctrl[KC_MAXW], h.c);
                }
            }
        }
        if (lane == 0) { a.key[s] = key; a.first_pos[s] = INT_MAX; }
    }
}

__global__ __launch_bounds__(256) void k_kfdb_rank(KfdbQueryArgs a)
{
    __shared__ unsigned long long s_k[256];
    const int M = a.st.slots, s = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = s < M ? a.key[s] : ~0ull;
    int rank = 0;
    for (int t0 = 0; t0 < M; t0 += 256) {
        __syncthreads();
        s_k[threadIdx.x] = t0 + (int)threadIdx.x < M ? a.key[t0 + threadIdx.x] : ~0ull;
        __syncthreads();
        if (mine != ~0ull)
            for (int j = 0; j < 256; j++) rank += s_k[j] < mine;
    }
    if (mine == ~0ull) return;
    a.list[rank] = s;
    const int minw = kd_min_words(a.ctrl[KC_MAXW]);
    int flag = 0;
    if ((a.reloc ? a.st.reloc_words[s] : a.st.loop_words[s]) > minw) {
        const float si = a.tscore[s];
        (a.reloc ? a.st.reloc_score : a.st.loop_score)[s] = si;
        atomicAdd(&a.ctrl[KC_SCORED], 1);
        if (a.reloc || si >= kd_start(a)) { flag = 1; atomicAdd(&a.ctrl[KC_KEPT], 1); }
    }
    a.ent_flag[rank] = flag;
}

__global__ __launch_bounds__(256) void k_kfdb_accumulate(KfdbQueryArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.ctrl[KC_LISTED] || !a.ent_flag[i]) return;
    const int s = a.list[i], minw = kd_min_words(a.ctrl[KC_MAXW]);
    const float *score = a.reloc ? a.st.reloc_score : a.st.loop_score;
    float acc = score[s], best = acc;
    int bs = s;
    for (int k = 0; k < KFDB_NEIGHBOURS; k++) {
        const int n = a.neighbours[(size_t)s * KFDB_NEIGHBOURS + k];
        if ((unsigned)n >= (unsigned)a.st.slots || !a.st.present[n]) continue;
        if (a.reloc ? a.st.reloc_query[n] != a.id : !(a.st.loop_query[n] == a.id && a.st.loop_words[n] > minw)) continue;
        const float sn = score[n];
        acc += sn;
        if (sn > best) { best = sn; bs = n; }
    }
    a.ent_acc[i] = acc;
    a.ent_best[i] = bs;
    atomicMax(reinterpret_cast<unsigned long long *>(a.ctrl + KC_BESTKEY), kd_acc_key(acc, i));
}

__global__ __launch_bounds__(1024) void k_kfdb_emit(KfdbQueryArgs a)
{
    __shared__ int s_wsum[16], s_base;
    const int L = a.ctrl[KC_LISTED];
    const float start = kd_start(a);
    const unsigned long long k0 = kd_acc_key(start, -1), k1 = *reinterpret_cast<const unsigned long long *>(a.ctrl + KC_BESTKEY);
    const int pos = (int)(0xffffffffu - (unsigned)(max(k0, k1) & 0xffffffffu)) - 1;
    const float best_acc = pos < 0 ? start : a.ent_acc[pos];
    const float retain = 0.75f * best_acc;
    if (threadIdx.x == 0) s_base = 0;
    for (int i = threadIdx.x; i < L; i += blockDim.x)
        if (a.ent_flag[i] && a.ent_acc[i] > retain) atomicMin(&a.first_pos[a.ent_best[i]], i);
    __syncthreads();
    for (int b = 0; b < L; b += blockDim.x) {
        const int i = b + threadIdx.x;
        int bs = -1;
        if (i < L && a.ent_flag[i] && a.ent_acc[i] > retain) {
            bs = a.ent_best[i];
            if (kd_ld<true>(a.first_pos + bs) != i) bs = -1;
        }
        const int o = kd_block_offset(bs >= 0, s_wsum, &s_base);
        if (bs >= 0) a.candidates[o] = bs;
    }
    if (threadIdx.x == 0) {
        *a.n_candidates = s_base;
        a.ctrl[KC_CAND] = s_base;
        a.ctrl[KC_MINW] = kd_min_words(a.ctrl[KC_MAXW]);
        a.ctrl[KC_BESTACC] = (int)__float_as_uint(best_acc);
    }
}

int kfdb_query_lds() { return KD_QUERY_LDS; }
int kfdb_sort_lds() { return KD_SORT_LDS; }

static int kd_lds_entries(int cap) { return cap < KD_QUERY_LDS ? (cap > 0 ? cap : 1) : KD_QUERY_LDS; }

void launch_kfdb_bow_vector(const int32_t *word_id, int n, const double *weight, int n_words, uint32_t *sort_scratch, int32_t *bow_word, double *bow_value,
                            int32_t *bow_n, hipStream_t s)
{
    hipLaunchKernelGGL(k_kfdb_bow_vector, dim3(1), dim3(1024), 0, s, word_id, n, weight, n_words, sort_scratch, bow_word, bow_value, bow_n);
}

void launch_kfdb_add(const KfdbState &st, int slot, uint32_t seq, int off, const KfdbVector &v, hipStream_t s)
{
    const int blocks = v.cap > 256 ? (v.cap + 255) / 256 : 1;
    hipLaunchKernelGGL(k_kfdb_add, dim3(blocks < 64 ? blocks : 64), dim3(256), 0, s, st, slot, seq, off, v);
}

void launch_kfdb_score(const KfdbScoreArgs &a, hipStream_t s)
{
    const int e = kd_lds_entries(a.q.cap);
    hipLaunchKernelGGL(k_kfdb_score, dim3(1), dim3(1024), (size_t)12 * e, s, a, e);
}

void launch_kfdb_query(const KfdbQueryArgs &a, hipStream_t s)
{
    const int M = a.st.slots;
    if (M <= 0) return;
    const int e = kd_lds_entries(a.q.cap), per = (M + 3) / 4, blocks = (M + 255) / 256;
    hipLaunchKernelGGL(k_kfdb_common, dim3(per < 512 ? per : 512), dim3(256), (size_t)12 * e, s, a, e);
    hipLaunchKernelGGL(k_kfdb_rank, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kfdb_accumulate, dim3(blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_kfdb_emit, dim3(1), dim3(1024), 0, s, a);
}

} // namespace jsorb
