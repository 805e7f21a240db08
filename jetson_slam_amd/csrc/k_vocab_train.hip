// k_vocab_train.hip - TemplatedVocabulary::create (TemplatedVocabulary.h:557-996) on the device, one level of the tree at a time (the contract:
//   include/jsorb.h, jsorb_vocabulary_train).  All runs of a level are in flight together: a run is a segment of the m positions, in ascending
//   input order.  Integer work throughout: popcounts, counts, sums; the one floating-point decision is the draw of cut_d, by one lane per run.
// There are no tiers by segment size.  Every "sum over a segment" and "first index of a segment whose running sum reaches a value" is taken from ONE
//   prefix over all positions, segments ignored: P(x) = the sum over the positions below x.  A segment's sum is P(end) - P(start), its running sum
//   at i is P(i + 1) - P(start), and P is kept as the sums of chunks of VT_CHUNK positions, scanned, plus a walk inside one chunk.  A segment of
//   ten million positions and a hundred thousand segments of a hundred take the same kernels; the launch shapes depend on m and S only.
// k_vt_seg_of       a position's segment, by bisection of seg_start
// k_vt_seed_first   one thread per segment: the trivial run's clusters, or the first centre (RandomInt)
// k_vt_seed_dist    step t of kmeans++: min_dists lowered by centre t - 1 (0 for the positions of runs that are trivial or have stopped), chunk sums
// k_vt_scan         one workgroup: the exclusive prefix of `cols` interleaved columns of chunk values, VT_SCAN_THREADS at a time with a carry
// k_vt_seed_pick    one wave per segment: dist_sum, the draws, the chunk by bisection, the position by a wave scan; centre t copied
// k_vt_assign       one pass of the association: the key distance << 5 | cluster, its minimum is the first of the nearest.  The 256 bit counts per
//                   (run, cluster): in LDS when the workgroup's chunk lies in one run, then one global atomic per non-zero counter; global
//                   atomics per bit where runs share a chunk (small runs: little contention)
// k_vt_means        a thread per (run, cluster, dword): the counts against N / 2 + N % 2, and the counters zeroed for the next pass
// k_vt_hist / k_vt_seg_rank / k_vt_scatter   the stable partition by cluster: the rank of a position among its run's positions with the same
//                   cluster is R(pos) - R(start), R the prefix count of that cluster index over ALL positions (chunk counts, scanned, plus ballots)
// k_vt_doc_words    Ni: a bit per (document, word) of a batch of documents, atomicOr; the first to set it counts
// Every index read from device memory is used only after a range check: nothing is read or written outside the arrays whatever they hold.
#include "jsorb_launch.h"
#include "k_search_common.h"

#ifndef VT_CHUNK
#define VT_CHUNK 1024                            // positions per chunk (whole waves)
#endif
#ifndef VT_SCAN_THREADS
#define VT_SCAN_THREADS 1024                     // chunk values k_vt_scan takes per tile
#endif
#define VT_KMAX 32

namespace jsorb {

static_assert(VT_CHUNK >= 64 && VT_CHUNK % 64 == 0 && VT_CHUNK <= 4096, "a chunk is whole waves; its sum of distances fits 32 bits");
static_assert(VT_SCAN_THREADS >= 64 && VT_SCAN_THREADS <= 1024 && VT_SCAN_THREADS % 64 == 0, "the scan's workgroup is whole waves");

typedef unsigned long long u64;

__device__ __forceinline__ u64 vt_mix(u64 x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// the j-th 31-bit value of the run (seed, first, size)
__device__ __forceinline__ unsigned vt_draw(u64 seed, int first, int size, int j)
{
    return (unsigned)(vt_mix(vt_mix(seed ^ ((u64)(unsigned)first << 32 | (u64)(unsigned)size)) + (u64)j) >> 33);
}

__device__ __forceinline__ void vt_row(const VocabTrainArgs &a, int pos, uint4 &lo, uint4 &hi)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(a.rows) + 2 * (size_t)(unsigned)a.perm[pos];      // the rows stay where the caller has them
    lo = q[0]; hi = q[1];
}
__device__ __forceinline__ void vt_centre(const VocabTrainArgs &a, int seg, int c, uint4 &lo, uint4 &hi)
{
    const uint4 *q = reinterpret_cast<const uint4 *>(a.centres) + 2 * ((size_t)seg * a.k + c);
    lo = q[0]; hi = q[1];
}

__global__ __launch_bounds__(256) void k_vt_iota(int32_t *perm, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = i;
}

__global__ __launch_bounds__(256) void k_vt_seg_of(VocabTrainArgs a)
{
    const int pos = blockIdx.x * 256 + threadIdx.x;
    if (pos >= a.m) return;
    int lo = 0, hi = a.S - 1;                    // the last segment with seg_start <= pos
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg_start[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    a.seg_of[pos] = lo;
}

__global__ __launch_bounds__(256) void k_vt_seed_first(VocabTrainArgs a)
{
    const int seg = blockIdx.x * 256 + threadIdx.x;
    if (seg >= a.S) return;
    const int start = a.seg_start[seg], size = a.seg_start[seg + 1] - start;
    uint4 *cen = reinterpret_cast<uint4 *>(a.centres) + 2 * (size_t)seg * a.k;
    a.seg_changed[seg] = 0;
    if (a.cslot[seg] < 0) {                      // :660-670
        const int nc = min(size, a.k);
        for (int c = 0; c < nc; c++) {
            uint4 lo, hi;
            vt_row(a, start + c, lo, hi);
            cen[2 * c] = lo; cen[2 * c + 1] = hi;
            a.cnt[(size_t)seg * a.k + c] = 1;
        }
        a.seg_nc[seg] = nc; a.seg_j[seg] = 0;
        return;
    }
    const unsigned r = vt_draw(a.seed, a.perm[start], size, 0);
    int idx = (int)(((double)r / 2147483648.0) * (double)size);      // Random.cpp:47-50
    idx = min(max(idx, 0), size - 1);
    uint4 lo, hi;
    vt_row(a, start + idx, lo, hi);
    cen[0] = lo; cen[1] = hi;
    a.seg_nc[seg] = 1; a.seg_j[seg] = 1;
}

// the sum of v over the workgroup's THREADS threads, to every thread (red: THREADS / 64 words of LDS)
template <int THREADS> __device__ __forceinline__ unsigned vt_block_sum(unsigned v, unsigned *red)
{
    for (int s = 32; s > 0; s >>= 1) v += (unsigned)__shfl_xor((int)v, s);
    __syncthreads();
    if (threadIdx.x % 64 == 0) red[threadIdx.x / 64] = v;
    __syncthreads();
    unsigned t = 0;
    for (int w = 0; w < THREADS / 64; w++) t += red[w];
    return t;
}

__global__ __launch_bounds__(256) void k_vt_seed_dist(VocabTrainArgs a, int t)
{
    __shared__ unsigned red[4];
    const int base = blockIdx.x * VT_CHUNK;
    unsigned sum = 0;
    for (int i = threadIdx.x; i < VT_CHUNK; i += 256) {
        const int pos = base + i;
        if (pos >= a.m) break;
        const int seg = a.seg_of[pos];
        unsigned v = 0;
        if (a.cslot[seg] >= 0 && a.seg_nc[seg] == t) {               // the run has its t centres: :872-880 with the last of them
            uint4 lo, hi, clo, chi;
            vt_row(a, pos, lo, hi);
            vt_centre(a, seg, t - 1, clo, chi);
            v = (unsigned)SL_HAMMING(lo, hi, clo, chi);
            if (t > 1) v = min(v, a.mind[pos]);
        }
        a.mind[pos] = v;
        sum += v;
    }
    sum = vt_block_sum<256>(sum, red);
    if (threadIdx.x == 0) a.chunk_sum[blockIdx.x] = sum;
}

// out[i * cols + c] = the sum of in[i' * cols + c] over i' < i, for i = 0 .. n (n + 1 rows of out)
template <class T> __global__ __launch_bounds__(VT_SCAN_THREADS) void k_vt_scan(const unsigned *in, T *out, int n, int cols)
{
    __shared__ T wsum[VT_SCAN_THREADS / 64];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int c = 0; c < cols; c++) {
        T carry = 0;
        for (int base = 0; base < n; base += VT_SCAN_THREADS) {
            const int i = base + threadIdx.x;
            const T x = i < n ? (T)in[(size_t)i * cols + c] : (T)0;
            T inc = x;
            for (int s = 1; s < 64; s <<= 1) {
                const T y = __shfl_up(inc, s);
                if (lane >= s) inc += y;
            }
            __syncthreads();
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            T before = 0, total = 0;
            for (int w = 0; w < VT_SCAN_THREADS / 64; w++) {
                if (w < wave) before += wsum[w];
                total += wsum[w];
            }
            if (i < n) out[(size_t)i * cols + c] = carry + before + inc - x;
            carry += total;
        }
        if (threadIdx.x == 0) out[(size_t)n * cols + c] = carry;
    }
}

// P(x) by one wave: the chunks below x from chunk_pre, the positions of x's chunk below x from mind
__device__ __forceinline__ u64 vt_prefix(const VocabTrainArgs &a, int x, int lane)
{
    const int c = x / VT_CHUNK;
    unsigned s = 0;
    for (int i = c * VT_CHUNK + lane; i < x; i += 64) s += a.mind[i];
    for (int d = 32; d > 0; d >>= 1) s += (unsigned)__shfl_xor((int)s, d);
    return a.chunk_pre[c] + s;
}

__global__ __launch_bounds__(256) void k_vt_seed_pick(VocabTrainArgs a, int t)
{
    const int seg = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (seg >= a.S || a.cslot[seg] < 0 || a.seg_nc[seg] != t) return;          // (uniform over the wave)
    const int start = a.seg_start[seg], end = a.seg_start[seg + 1];
    const u64 p0 = vt_prefix(a, start, lane), dist_sum = vt_prefix(a, end, lane) - p0;
    if (dist_sum == 0) return;                   // :908 - the run keeps its t centres
    int j = a.seg_j[seg];
    const int first = a.perm[start];
    double cut;
    do {                                         // :888-891
        const unsigned r = vt_draw(a.seed, first, end - start, j++);
        cut = ((double)r / 2147483647.0) * (double)dist_sum;         // Random.h:55-69
    } while (cut == 0.0);
    const u64 goal = p0 + (u64)ceil(cut);        // the first i with P(i + 1) >= goal; goal > p0, goal <= P(end)
    int lo = start / VT_CHUNK, hi = (end - 1) / VT_CHUNK;            // the last chunk whose positions all lie behind a prefix < goal
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk_pre[mid] < goal) lo = mid; else hi = mid - 1;
    }
    const int x0 = max(lo * VT_CHUNK, start), x1 = min((lo + 1) * VT_CHUNK, end);
    u64 run = lo * VT_CHUNK >= start ? a.chunk_pre[lo] : p0;
    int pick = end - 1;                          // :900-901
    for (int b = x0; b < x1; b += 64) {
        const int i = b + lane;
        const unsigned v = i < x1 ? a.mind[i] : 0u;
        unsigned inc = v;
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)inc, s);
            if (lane >= s) inc += y;
        }
        const u64 hit = __ballot(i < x1 && run + inc >= goal);
        if (hit) { pick = b + (int)__builtin_ctzll(hit); break; }
        run += (unsigned)__shfl((int)inc, 63);
    }
    if (lane < 2) {                              // the row's two halves by two lanes
        const size_t row = (unsigned)a.perm[pick];
        reinterpret_cast<uint4 *>(a.centres)[2 * ((size_t)seg * a.k + t) + lane] = reinterpret_cast<const uint4 *>(a.rows)[2 * row + lane];
    }
    if (lane == 0) { a.seg_nc[seg] = t + 1; a.seg_j[seg] = j; }
}

__global__ __launch_bounds__(256) void k_vt_assign(VocabTrainArgs a, int pass)
{
    extern __shared__ unsigned lds[];            // k x 256 bit counts, k member counts: used when the chunk lies in one run
    const int base = blockIdx.x * VT_CHUNK, last = min(base + VT_CHUNK, a.m) - 1, k = a.k;
    const int seg0 = a.seg_of[base];
    const bool one = seg0 == a.seg_of[last];
    const int slot0 = a.cslot[seg0];
    if (one && slot0 < 0) {                      // a chunk inside a trivial run (k >= VT_CHUNK only): the positions are their own clusters
        for (int i = threadIdx.x; base + i <= last; i += 256) a.assoc[base + i] = (uint8_t)min(base + i - a.seg_start[seg0], k - 1);
        return;
    }
    if (one) {
        for (int i = threadIdx.x; i < k * 257; i += 256) lds[i] = 0;
        __syncthreads();
    }
    bool moved = false;
    for (int i = threadIdx.x; base + i <= last; i += 256) {
        const int pos = base + i, seg = one ? seg0 : a.seg_of[pos];
        const int slot = one ? slot0 : a.cslot[seg];
        if (slot < 0) {
            a.assoc[pos] = (uint8_t)min(pos - a.seg_start[seg], k - 1);
            continue;
        }
        uint4 lo, hi;
        vt_row(a, pos, lo, hi);
        const int nc = min(a.seg_nc[seg], k);
        if (nc < 1) continue;                    // (k_vt_seed_first leaves every run a centre)
        unsigned best = 0xffffffffu;
        for (int c = 0; c < nc; c++) {           // :734-745
            uint4 clo, chi;
            vt_centre(a, seg, c, clo, chi);
            best = min(best, (unsigned)SL_HAMMING(lo, hi, clo, chi) << 5 | (unsigned)c);
        }
        const int cl = (int)(best & 31u);
        if (a.assoc[pos] != cl) {
            a.assoc[pos] = (uint8_t)cl;
            a.seg_changed[seg] = pass;
            moved = true;
        }
        const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        if (one) {
            atomicAdd(&lds[k * 256 + cl], 1u);
            unsigned *q = lds + cl * 256;
#pragma unroll
            for (int d = 0; d < 8; d++)
                for (unsigned x = w[d]; x; x &= x - 1) atomicAdd(&q[d * 32 + __builtin_ctz(x)], 1u);
        } else {
            atomicAdd(&a.cnt[(size_t)seg * k + cl], 1u);
            unsigned *q = a.counters + ((size_t)slot * k + cl) * 256;
#pragma unroll
            for (int d = 0; d < 8; d++)
                for (unsigned x = w[d]; x; x &= x - 1) atomicAdd(&q[d * 32 + __builtin_ctz(x)], 1u);
        }
    }
    if (moved) *a.level_word = pass;
    if (one) {
        __syncthreads();
        unsigned *q = a.counters + (size_t)slot0 * k * 256;
        for (int i = threadIdx.x; i < k * 256; i += 256)
            if (lds[i]) atomicAdd(&q[i], lds[i]);
        if ((int)threadIdx.x < k && lds[k * 256 + threadIdx.x]) atomicAdd(&a.cnt[(size_t)seg0 * k + threadIdx.x], lds[k * 256 + threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void k_vt_means(VocabTrainArgs a)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t sc = id / 8;                    // (segment, cluster): its eight threads are neighbours in one wave
    const int d = (int)(id % 8);
    if (sc >= (size_t)a.S * a.k) return;
    const int seg = (int)(sc / a.k), c = (int)(sc % a.k), slot = a.cslot[seg];
    if (slot < 0) return;
    const unsigned N = a.cnt[sc];
    if (N == 0) return;                          // no member (or no such centre): the centre stays, the counters are zero
    const unsigned n2 = N / 2 + N % 2;           // FORB.cpp:65
    unsigned *q = a.counters + ((size_t)slot * a.k + c) * 256 + d * 32;
    unsigned word = 0;
    for (int b = 0; b < 32; b++) {
        if (q[b] >= n2) word |= 1u << b;
        q[b] = 0;
    }
    a.centres[sc * 8 + d] = word;
    __builtin_amdgcn_wave_barrier();             // the eight threads have read N
    if (d == 0) a.cnt[sc] = 0;
}

__global__ __launch_bounds__(256) void k_vt_hist(VocabTrainArgs a)
{
    __shared__ unsigned h[VT_KMAX];
    if (threadIdx.x < VT_KMAX) h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * VT_CHUNK;
    for (int i = threadIdx.x; i < VT_CHUNK && base + i < a.m; i += 256) atomicAdd(&h[a.assoc[base + i] & (VT_KMAX - 1)], 1u);
    __syncthreads();
    if ((int)threadIdx.x < a.k) a.hist[(size_t)blockIdx.x * a.k + threadIdx.x] = h[threadIdx.x];
}

// R(start) per segment and cluster index: lane c of the segment's wave counts the positions of start's chunk below start with index c
__global__ __launch_bounds__(256) void k_vt_seg_rank(VocabTrainArgs a)
{
    const int seg = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (seg >= a.S) return;
    const int start = a.seg_start[seg], chunk = start / VT_CHUNK;
    unsigned count = 0;
    for (int b = chunk * VT_CHUNK; b < start; b += 64) {
        const int i = b + lane;
        const int v = i < start ? (int)a.assoc[i] : -1;
        for (int c = 0; c < a.k; c++) {
            const u64 mk = __ballot(v == c);
            if (lane == c) count += (unsigned)__popcll(mk);
        }
    }
    if (lane < a.k) a.seg_rank[(size_t)seg * a.k + lane] = a.hist_pre[(size_t)chunk * a.k + lane] + count;
}

__global__ __launch_bounds__(256) void k_vt_scatter(VocabTrainArgs a)
{
    __shared__ unsigned running[VT_KMAX], wcnt[4][VT_KMAX];
    const int base = blockIdx.x * VT_CHUNK, lane = threadIdx.x % 64, wave = threadIdx.x / 64, k = a.k;
    if ((int)threadIdx.x < k) running[threadIdx.x] = a.hist_pre[(size_t)blockIdx.x * k + threadIdx.x];
    for (int r0 = 0; r0 < VT_CHUNK && base + r0 < a.m; r0 += 256) {          // (uniform over the workgroup)
        const int pos = base + r0 + threadIdx.x;
        const bool in = pos < a.m && r0 + (int)threadIdx.x < VT_CHUNK;
        const int cl = in ? (int)a.assoc[pos] & (VT_KMAX - 1) : -1;
        unsigned below = 0;
        for (int c = 0; c < k; c++) {
            const u64 mk = __ballot(cl == c);
            if (cl == c) below = (unsigned)__popcll(mk & ((1ull << lane) - 1));
            if (lane == c) wcnt[wave][c] = (unsigned)__popcll(mk);
        }
        __syncthreads();
        if (in && cl < k) {
            unsigned R = running[cl] + below;
            for (int w = 0; w < wave; w++) R += wcnt[w][cl];
            const int seg = a.seg_of[pos], src = a.perm[pos];
            const size_t sc = (size_t)seg * k + cl;
            const int d0 = a.dest_base[sc];
            if (d0 < 0) {
                a.leaf[src] = a.node_base[seg] + cl;
            } else {
                const long long dst = (long long)d0 + (long long)(R - a.seg_rank[sc]);
                if (dst >= 0 && dst < a.m_next) a.perm_out[dst] = src;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < k) running[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_vt_doc_words(const int32_t *word_id, int i0, int i1, const int32_t *doc_start, int d0, int d1, int n_words,
                                                      uint32_t *bitmap, int32_t *ni)
{
    const int i = i0 + blockIdx.x * 256 + threadIdx.x;
    if (i >= i1) return;
    int lo = d0, hi = d1 - 1;                    // the last document of the batch that starts at or before i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (doc_start[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int w = word_id[i];
    if (w < 0 || w >= n_words) return;
    const size_t words32 = ((size_t)n_words + 31) / 32;
    const unsigned bit = 1u << (w & 31);
    if (!(atomicOr(&bitmap[(size_t)(lo - d0) * words32 + (w >> 5)], bit) & bit)) atomicAdd(&ni[w], 1);
}

int vocab_train_chunk() { return VT_CHUNK; }
int vocab_train_scan_threads() { return VT_SCAN_THREADS; }

void launch_vocab_train_iota(int32_t *perm, int n, hipStream_t s)
{
    hipLaunchKernelGGL(k_vt_iota, dim3((n + 255) / 256), dim3(256), 0, s, perm, n);
}

void launch_vocab_train_seed(const VocabTrainArgs &a, hipStream_t s)
{
    const int chunks = vocab_train_chunks(a.m);
    hipLaunchKernelGGL(k_vt_seg_of, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vt_seed_first, dim3((a.S + 255) / 256), dim3(256), 0, s, a);
    for (int t = 1; t < a.k; t++) {
        hipLaunchKernelGGL(k_vt_seed_dist, dim3(chunks), dim3(256), 0, s, a, t);
        hipLaunchKernelGGL(k_vt_scan<u64>, dim3(1), dim3(VT_SCAN_THREADS), 0, s, a.chunk_sum, a.chunk_pre, chunks, 1);
        hipLaunchKernelGGL(k_vt_seed_pick, dim3((a.S + 3) / 4), dim3(256), 0, s, a, t);
    }
}

void launch_vocab_train_assign(const VocabTrainArgs &a, int pass, hipStream_t s)
{
    hipLaunchKernelGGL(k_vt_assign, dim3(vocab_train_chunks(a.m)), dim3(256), (size_t)a.k * 257 * sizeof(unsigned), s, a, pass);
}

void launch_vocab_train_means(const VocabTrainArgs &a, hipStream_t s)
{
    const size_t threads = (size_t)a.S * a.k * 8;
    hipLaunchKernelGGL(k_vt_means, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
}

void launch_vocab_train_regroup(const VocabTrainArgs &a, hipStream_t s)
{
    const int chunks = vocab_train_chunks(a.m);
    hipLaunchKernelGGL(k_vt_hist, dim3(chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vt_scan<unsigned>, dim3(1), dim3(VT_SCAN_THREADS), 0, s, a.hist, a.hist_pre, chunks, a.k);
    hipLaunchKernelGGL(k_vt_seg_rank, dim3((a.S + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vt_scatter, dim3(chunks), dim3(256), 0, s, a);
}

void launch_vocab_train_doc_words(const int32_t *word_id, int i0, int i1, const int32_t *doc_start, int d0, int d1, int n_words, uint32_t *bitmap,
                                  int32_t *ni, hipStream_t s)
{
    if (i1 <= i0) return;
    hipLaunchKernelGGL(k_vt_doc_words, dim3((i1 - i0 + 255) / 256), dim3(256), 0, s, word_id, i0, i1, doc_start, d0, d1, n_words, bitmap, ni);
}

} // namespace jsorb
