// k_local_map.hip - the local map of Tracking::TrackLocalMap on the device (the contract: include/jsorb.h, jsorb_local_map_points_async):
//   Tracking::UpdateLocalPoints (Tracking.cpp:1818-1841), the frame marks and the map_points list of SearchLocalPoints (:1352-1367, :1410-1420) and
//   K16 (k16_frustum, k_search_common.h: the function k_is_in_frustum runs) over that list, compacted in order into the arrays k_local_candidates reads.
// The reference dedupes through a field of the map point (mnTrackReferenceForFrame) and skips the frame's own points through another
// (mnLastFrameSeen).  Here both live in ONE word per table row, all ones between calls: bit 31 = the frame has NOT seen the row, the low 31 bits =
// the smallest entry position with the row.  The first entry with a row is the one whose position the word holds.
// k_lm_marks   a thread per keypoint and per entry, one launch: a keypoint clears bit 31 of its row (atomicAnd) and writes blocked_in; an entry
//              lowers its row's position (a compare-and-swap loop that keeps bit 31, so the two commute); the counters are zeroed
// k_lm_list    a workgroup per chunk of LM_CHUNK entries: the drop rules in the reference's order, K16 for what is left, one byte per entry
//              (inside the frustum or not), the chunk's number of those, the counts and statistics by one atomic per workgroup and counter
// k_lm_scan    one workgroup: the exclusive prefix of the chunk numbers, with a carry from tile to tile; counts[2..4]
// k_lm_write   a workgroup per chunk: an entry's slot = the chunk's prefix + the waves before it (LDS) + the lanes before it (ballot, popcount);
//              K16 again for the slots below the capacity (the same function on the same inputs), the descriptor by two 16-byte loads and
//              stores; every word an entry or a keypoint touched is set back to all ones; further workgroups write the padding
// The order-preserving compaction is the scheme of k_vocab_train.hip (chunk sums, a scan, a walk inside the chunk).
// Every row read from device memory is used only after a range check: nothing is read or written outside the arrays whatever they hold.
#include <algorithm>

#include "jsorb_launch.h"
#include "k_search_common.h"

#ifndef LM_CHUNK
#define LM_CHUNK 1024                            // entries per chunk (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define LM_SCAN_THREADS 1024
#define LM_CLEAN 0xFFFFFFFFu
#define LM_UNSEEN 0x80000000u
#define LM_POS 0x7FFFFFFFu

namespace jsorb {

static_assert(LM_CHUNK >= 64 && LM_CHUNK % 64 == 0 && LM_CHUNK <= 4096, "a chunk is whole waves");

typedef unsigned long long u64;

// the entry's fate, in the order the rules fire; LM_NONE: no entry at this position
enum { LM_NULL, LM_INVALID, LM_BAD, LM_DUPLICATE, LM_SEEN, LM_OUTSIDE, LM_INSIDE, LM_KINDS, LM_NONE = LM_KINDS };

__device__ __forceinline__ bool lm_row_ok(const LocalMapArgs &a, int r) { return r >= 0 && r < a.t.n_rows; }

__device__ __forceinline__ bool lm_k16(const LocalMapArgs &a, int r, K16Out &o)
{
    const jsorb_map_point_table &t = a.t;
    const jsorb_frustum_params &p = a.p;
    return k16_frustum(p.Rcw, p.tcw, p.Ow, p.fx, p.fy, p.cx, p.cy, p.minX, p.maxX, p.minY, p.maxY, p.nScaleLevels, p.logScaleFactor, p.viewCosAngle,
                       t.Px[r], t.Py[r], t.Pz[r], t.Pnx + r, t.Pny + r, t.Pnz + r, t.MaxDistance + r, t.invariance_maxDistance + r,
                       t.invariance_minDistance + r, o);
}

__global__ __launch_bounds__(256) void k_lm_marks(LocalMapArgs a)
{
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g == 0) {
        a.stats[0] = a.E;
        for (int i = 1; i < 6; i++) a.stats[i] = 0;      // null, invalid rows, duplicates, bad, seen
        a.counts[0] = 0; a.counts[1] = 0;
    }
    if (g < a.N) {                               // :1352-1367
        const int r = a.frame_row ? a.frame_row[g] : -1;
        const bool seen = lm_row_ok(a, r) && !a.t.bad[r];
        if (seen) atomicAnd(&a.word[r], LM_POS);
        if (a.blocked_in) a.blocked_in[g] = seen ? 1 : 0;
        return;
    }
    const long long e = g - a.N;
    if (e >= a.E) return;
    const int r = a.entry_row[e];
    if (!lm_row_ok(a, r) || a.t.bad[r]) return;
    uint32_t old = a.word[r];
    while ((old & LM_POS) > (uint32_t)e) {       // (the position of the first entry with the row; bit 31 is the marks')
        const uint32_t seen = atomicCAS(&a.word[r], old, (old & LM_UNSEEN) | (uint32_t)e);
        if (seen == old) break;
        old = seen;
    }
}

__global__ __launch_bounds__(256) void k_lm_list(LocalMapArgs a)
{
    __shared__ unsigned s_cnt[LM_KINDS];
    const int base = blockIdx.x * LM_CHUNK, lane = threadIdx.x % 64;
    if (threadIdx.x < LM_KINDS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    unsigned mine = 0;                           // lane k of a wave: its entries of kind k
    for (int r0 = 0; r0 < LM_CHUNK; r0 += 256) {                         // (uniform over the workgroup)
        const int idx = r0 + (int)threadIdx.x, pos = base + idx;
        int kind = LM_NONE;
        if (idx < LM_CHUNK && pos < a.E) {
            const int r = a.entry_row[pos];
            if (r < 0) kind = LM_NULL;                                   // :1830 !pMP
            else if (r >= a.t.n_rows) kind = LM_INVALID;
            else if (a.t.bad[r]) kind = LM_BAD;                          // :1834
            else {
                const uint32_t w = a.word[r];
                K16Out o;
                if ((w & LM_POS) != (uint32_t)pos) kind = LM_DUPLICATE;  // :1832 mnTrackReferenceForFrame
                else if (!(w & LM_UNSEEN)) kind = LM_SEEN;               // :1414 mnLastFrameSeen
                else kind = lm_k16(a, r, o) ? LM_INSIDE : LM_OUTSIDE;
            }
            a.keep[pos] = kind == LM_INSIDE;
        }
        for (int k = 0; k < LM_KINDS; k++) {
            const u64 m = __ballot(kind == k);
            if (lane == k) mine += (unsigned)__popcll(m);
        }
    }
    if (lane < LM_KINDS && mine) atomicAdd(&s_cnt[lane], mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned inside = s_cnt[LM_INSIDE], listed = inside + s_cnt[LM_OUTSIDE], local = listed + s_cnt[LM_SEEN];
        a.chunk_sum[blockIdx.x] = inside;
        if (s_cnt[LM_NULL]) atomicAdd(&a.stats[1], (int)s_cnt[LM_NULL]);
        if (s_cnt[LM_INVALID]) atomicAdd(&a.stats[2], (int)s_cnt[LM_INVALID]);
        if (s_cnt[LM_DUPLICATE]) atomicAdd(&a.stats[3], (int)s_cnt[LM_DUPLICATE]);
        if (s_cnt[LM_BAD]) atomicAdd(&a.stats[4], (int)s_cnt[LM_BAD]);
        if (s_cnt[LM_SEEN]) atomicAdd(&a.stats[5], (int)s_cnt[LM_SEEN]);
        if (local) atomicAdd(&a.counts[0], (int)local);
        if (listed) atomicAdd(&a.counts[1], (int)listed);
    }
}

// pre[i] = the sum of sum[i'] over i' < i, for i = 0 .. n; counts[2] = pre[n] = nToMatch, counts[3] = the slots written, counts[4] = overflow
__global__ __launch_bounds__(LM_SCAN_THREADS) void k_lm_scan(LocalMapArgs a, int n)
{
    __shared__ unsigned wsum[LM_SCAN_THREADS / 64];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    unsigned carry = 0;
    for (int base = 0; base < n; base += LM_SCAN_THREADS) {
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
        for (int w = 0; w < LM_SCAN_THREADS / 64; w++) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (i < n) a.chunk_pre[i] = carry + before + inc - x;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.chunk_pre[n] = carry;
        a.counts[2] = (int)carry;
        a.counts[3] = (int)min(carry, (unsigned)a.capacity);
        a.counts[4] = carry > (unsigned)a.capacity;
    }
}

__global__ __launch_bounds__(256) void k_lm_write(LocalMapArgs a, int chunks, int pad_blocks)
{
    __shared__ unsigned wcnt[4];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    if ((int)blockIdx.x >= chunks + pad_blocks) {                        // the frame's marks back to all ones
        const long long k = (long long)(blockIdx.x - chunks - pad_blocks) * 256 + threadIdx.x;
        if (k < a.N && a.frame_row) {
            const int r = a.frame_row[k];
            if (lm_row_ok(a, r)) a.word[r] = LM_CLEAN;
        }
        return;
    }
    if ((int)blockIdx.x >= chunks) {                                     // the padding behind the points written
        const long long i = (long long)(blockIdx.x - chunks) * 256 + threadIdx.x;
        if (i < a.capacity && i >= (long long)a.chunk_pre[chunks]) {
            a.point_row[i] = -1; a.in_frustum[i] = 0;
            a.u[i] = 0.0f; a.v[i] = 0.0f; a.invz[i] = 0.0f; a.view_cos[i] = 0.0f; a.level[i] = 0;
            uint4 *d = reinterpret_cast<uint4 *>(a.mp_desc) + 2 * i;
            d[0] = make_uint4(0, 0, 0, 0); d[1] = make_uint4(0, 0, 0, 0);
        }
        return;
    }
    const int base = blockIdx.x * LM_CHUNK;
    unsigned running = a.chunk_pre[blockIdx.x];
    for (int r0 = 0; r0 < LM_CHUNK && base + r0 < a.E; r0 += 256) {      // (uniform over the workgroup)
        const int idx = r0 + (int)threadIdx.x, pos = base + idx;
        const bool in = idx < LM_CHUNK && pos < a.E;
        const int r = in ? a.entry_row[pos] : -1;
        const bool keep = in && a.keep[pos];
        const u64 m = __ballot(keep);
        if (lane == 0) wcnt[wave] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned slot = running + (unsigned)__popcll(m & ((1ull << lane) - 1));
        for (int w = 0; w < wave; w++) slot += wcnt[w];
        if (keep && slot < (unsigned)a.capacity && lm_row_ok(a, r)) {    // (a kept entry's row is in the table: k_lm_list checked it)
            K16Out o = {0.0f, 0.0f, 0.0f, 0.0f, 0};
            lm_k16(a, r, o);
            a.point_row[slot] = r; a.in_frustum[slot] = 1;
            a.u[slot] = o.u; a.v[slot] = o.v; a.invz[slot] = o.invz; a.view_cos[slot] = o.view_cos; a.level[slot] = o.level;
            const uint4 *q = reinterpret_cast<const uint4 *>(a.t.desc) + 2 * (size_t)r;
            uint4 *d = reinterpret_cast<uint4 *>(a.mp_desc) + 2 * (size_t)slot;
            const uint4 lo = q[0], hi = q[1];
            d[0] = lo; d[1] = hi;
        }
        if (lm_row_ok(a, r)) a.word[r] = LM_CLEAN;                       // the word this entry may have lowered
        running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_map_points_scatter(int n_rows, float *d0, float *d1, float *d2, float *d3, float *d4, float *d5, float *d6, float *d7,
                                                            float *d8, uint8_t *bad, int n, const int32_t *rows, const jsorb_map_point_record *records)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i];
    if (r < 0 || r >= n_rows) return;
    const jsorb_map_point_record q = records[i];
    d0[r] = q.P[0]; d1[r] = q.P[1]; d2[r] = q.P[2];
    d3[r] = q.Pn[0]; d4[r] = q.Pn[1]; d5[r] = q.Pn[2];
    d6[r] = q.MaxDistance; d7[r] = q.invariance_maxDistance; d8[r] = q.invariance_minDistance;
    bad[r] = q.bad;
}

int local_map_chunk() { return LM_CHUNK; }

// Launch shapes from E, N and capacity alone.  k_lm_marks and k_lm_scan always run: they write the zero counts of an empty call.
void launch_local_map(const LocalMapArgs &a, hipStream_t s)
{
    const int chunks = local_map_chunks(a.E), pad_blocks = (a.capacity + 255) / 256, kp_blocks = (a.N + 255) / 256;
    const long long items = (long long)a.N + a.E;
    hipLaunchKernelGGL(k_lm_marks, dim3((unsigned)std::max<long long>((items + 255) / 256, 1)), dim3(256), 0, s, a);
    if (chunks > 0) hipLaunchKernelGGL(k_lm_list, dim3(chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LM_SCAN_THREADS), 0, s, a, chunks);
    if (chunks + pad_blocks + kp_blocks > 0) hipLaunchKernelGGL(k_lm_write, dim3(chunks + pad_blocks + kp_blocks), dim3(256), 0, s, a, chunks, pad_blocks);
}

void launch_map_points_scatter(int n_rows, float *const dst[9], uint8_t *bad, int n, const int32_t *rows, const jsorb_map_point_record *records, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_map_points_scatter, dim3((n + 255) / 256), dim3(256), 0, s, n_rows, dst[0], dst[1], dst[2], dst[3], dst[4], dst[5], dst[6], dst[7],
                       dst[8], bad, n, rows, records);
}

} // namespace jsorb
