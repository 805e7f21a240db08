// k_local_keyframes.hip - Tracking::UpdateLocalKeyFrames (Tracking.cpp:1844-1952) on the device (the contract: include/jsorb.h,
// jsorb_local_keyframes_async), and the local keyframes' GetMapPointMatches() concatenated as jsorb_local_map_points_async reads them.
// Integer work only.  The reference counts votes in a std::map<KeyFrame*, int> filled from the points' observations; here a keyframe's vote is the
// sum over its own run of rows of the row's multiplicity in the frame, which is the same number.  The multiplicity lives in the local map's
// scratch word of the row (jsorb_handle.h, struct lm), all ones between calls: a keypoint SUBTRACTS one, so mult = ~word.
// k_lk_marks   a thread per keypoint: word[row] -= 1 for a row in the table that is not bad (:1850-1858); the counters are zeroed
// k_lk_votes   a wave per slot: the run by coalesced loads, the words gathered, the sum by shuffles; vote[s], first[s] = state == 1 && vote > 0,
//              n_counter (state != 0 && vote > 0), the invalid runs
// k_lk_rank    a wave per slot of the first list: its rank by (order_key, slot) among the list, counted; order[rank] = slot; the reference
//              keyframe (:1883-1887: the first strict maximum in order = the largest vote, the lowest rank among equals) by one 64-bit atomicMax
// k_lk_expand  one workgroup: the first list into local_kf_slot, or the kept list when the counter is empty (:1866); the candidates of up to 80
//              elements filtered in parallel into LDS (neighbour row, child run, parent: range and state tests), then ONE wave walks the elements
//              in order against the membership set (an LDS bitmap for slots below LK_MEMBER_LDS, first[] beyond), picking "first eligible" by
//              ballot (:1895-1945); local_kf_start by a scan of the run lengths; state_io, counts, stats
// k_lk_gather  a thread per output entry: its keyframe by binary search in local_kf_start, the run's entry copied, -1 behind E_total; further
//              workgroups set the words of the frame's rows back to all ones
// Every slot, row and run read from device memory is used only after a range check: nothing is read or written outside the arrays whatever they
// hold.
#include <algorithm>

#include "jsorb_launch.h"

#ifndef LK_MEMBER_LDS
#define LK_MEMBER_LDS 32768                      // slots whose membership bit lives in LDS (a test build lowers both: jetson_slam_amd/build.py VARIANTS)
#endif
#ifndef LK_CHILD_LDS
#define LK_CHILD_LDS 4096                        // filtered child candidates of all elements kept in LDS; a run that does not fit is read from global memory
#endif
#define LK_LIMIT 80                              // :1898 mvpLocalKeyFrames.size() > 80
#define LK_NEIGH 10                              // GetBestCovisibilityKeyFrames(10)
#define LK_CLEAN 0xFFFFFFFFu

namespace jsorb {

static_assert(LK_MEMBER_LDS >= 64 && LK_MEMBER_LDS % 64 == 0 && LK_MEMBER_LDS <= 262144, "the bitmap is whole ballots and fits LDS");
static_assert(LK_CHILD_LDS >= 1 && LK_CHILD_LDS <= 8192, "the child candidates fit LDS");

typedef unsigned long long u64;

__device__ __forceinline__ bool lk_row_ok(const LocalKfArgs &a, int r) { return r >= 0 && r < a.n_rows; }
__device__ __forceinline__ bool lk_usable(const LocalKfArgs &a, int s) { return s >= 0 && s < a.g.max_keyframes && a.g.state[s] != 0; }
__device__ __forceinline__ bool lk_run_ok(int off, int len, int entries) { return off >= 0 && len >= 0 && (long long)off + len <= entries; }

__device__ __forceinline__ int lk_wave_sum(int x)
{
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s);
    return x;
}

__global__ __launch_bounds__(256) void k_lk_marks(LocalKfArgs a)
{
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) {
        for (int i = 0; i < LK_STATS; i++) a.stats[i] = 0;
        *a.best = 0;
    }
    if (k < a.n_frame && a.frame_row) {          // :1848-1858
        const int r = a.frame_row[k];
        if (lk_row_ok(a, r) && !a.bad[r]) atomicSub(&a.word[r], 1u);
    }
}

__global__ __launch_bounds__(256) void k_lk_votes(LocalKfArgs a)
{
    __shared__ int s_cnt[2];                     // voters, invalid runs
    const int lane = threadIdx.x % 64, s = blockIdx.x * 4 + threadIdx.x / 64;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (s < a.g.max_keyframes) {                 // (uniform over the wave)
        const int state = a.g.state[s];
        int vote = 0, invalid = 0;
        if (state != 0) {
            const int off = a.g.point_off[s], len = a.g.point_len[s];
            if (lk_run_ok(off, len, a.g.pool_entries)) {
                for (int j = lane; j < len; j += 64) {                   // :1855-1857, from the keyframe's side
                    const int r = a.g.point_pool[off + j];
                    const bool reg = a.g.registered ? a.g.registered[off + j] != 0 : true;
                    if (reg && lk_row_ok(a, r)) vote += (int)~a.word[r];
                }
                vote = lk_wave_sum(vote);
            } else
                invalid = 1;
            if (!lk_run_ok(a.g.child_off[s], a.g.child_len[s], a.g.child_entries)) invalid++;
        }
        if (lane == 0) {
            a.vote[s] = vote;
            a.first[s] = state == 1 && vote > 0;
            if (vote > 0) atomicAdd(&s_cnt[0], 1);
            if (invalid) atomicAdd(&s_cnt[1], invalid);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(&a.stats[0], s_cnt[0]);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(&a.stats[6], s_cnt[1]);
}

__global__ __launch_bounds__(256) void k_lk_rank(LocalKfArgs a)
{
    const int lane = threadIdx.x % 64, s = blockIdx.x * 4 + threadIdx.x / 64, S = a.g.max_keyframes;
    if (s >= S || !a.first[s]) return;           // (uniform over the wave)
    const long long key = a.g.order_key[s];
    int before = 0;
    for (int t = lane; t < S; t += 64)           // std::map<KeyFrame*, int>'s order, equal keys by slot
        if (a.first[t]) {
            const long long kt = a.g.order_key[t];
            before += kt < key || (kt == key && t < s);
        }
    before = lk_wave_sum(before);
    if (lane == 0) {
        a.order[before] = s;                     // (ranks are distinct and below the list's length <= S)
        atomicAdd(&a.stats[1], 1);
        atomicMax(a.best, (u64)(unsigned)a.vote[s] << 32 | (u64)(0xFFFFFFFFu - (unsigned)before));
    }
}

// membership of slot c in the list: the first list and everything appended so far.  Only wave 0 calls these; in lk_add every lane writes the
// same value to the same place, so a lane reads back what it wrote itself.
__device__ __forceinline__ bool lk_member(const LocalKfArgs &a, const unsigned *bits, int c)
{
    return c < LK_MEMBER_LDS ? (bits[c >> 5] >> (c & 31)) & 1u : a.first[c] != 0;
}

__device__ __forceinline__ void lk_add(const LocalKfArgs &a, unsigned *bits, int lane, int c, int &size)
{
    if (c < LK_MEMBER_LDS)
        bits[c >> 5] |= 1u << (c & 31);
    else
        a.first[c] = 1;
    if (lane == 0) a.local_kf_slot[size] = c;
    size++;
}

__global__ __launch_bounds__(256) void k_lk_expand(LocalKfArgs a)
{
    __shared__ unsigned s_bits[LK_MEMBER_LDS / 32];
    __shared__ int s_nb[LK_LIMIT * LK_NEIGH], s_par[LK_LIMIT], s_coff[LK_LIMIT + 1], s_clen[LK_LIMIT], s_cglob[LK_LIMIT], s_child[LK_CHILD_LDS];
    __shared__ int s_n[2];                       // the list's length, the reason the expansion ended
    __shared__ long long s_wsum[4];
    const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, S = a.g.max_keyframes;
    const int n_counter = a.stats[0], n_first = a.stats[1];
    const bool kept = n_counter == 0;            // :1866
    const int n0 = kept ? std::min(std::max(a.state_io[0], 0), a.kf_capacity) : std::min(n_first, a.kf_capacity);
    const int n_el = !kept && n_first <= LK_LIMIT ? n_first : 0;         // the elements the loop of :1895 can reach: none once size > 80
    int ref = a.state_io[1];
    if (!kept) {
        const u64 best = *a.best;
        if (best) ref = a.order[0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu)];
        for (int i = tid; i < n0; i += 256) a.local_kf_slot[i] = a.order[i];         // :1876-1891
    }
    if (n_el > 0) {
        // the membership bits of the first list
        for (int base = wave * 64; base < LK_MEMBER_LDS && base < S; base += 256) {
            const u64 m = __ballot(base + lane < S && a.first[base + lane]);
            if (lane == 0) { s_bits[base >> 5] = (unsigned)m; s_bits[(base >> 5) + 1] = (unsigned)(m >> 32); }
        }
        // the candidates: a neighbour or a child must be usable and good, a parent usable (:1908, :1923, :1935)
        for (int i = tid; i < n_el * LK_NEIGH; i += 256) {
            const int c = a.g.neighbours[(size_t)a.order[i / LK_NEIGH] * LK_NEIGH + i % LK_NEIGH];
            s_nb[i] = lk_usable(a, c) && a.g.state[c] == 1 ? c : -1;
        }
        for (int i = tid; i < n_el; i += 256) {
            const int s = a.order[i], p = a.g.parent[s], off = a.g.child_off[s], len = a.g.child_len[s];
            s_par[i] = lk_usable(a, p) ? p : -1;
            const bool ok = lk_run_ok(off, len, a.g.child_entries);
            s_clen[i] = ok ? len : 0;
            s_cglob[i] = ok ? off : 0;
        }
        __syncthreads();
        if (tid == 0) {                          // where each child run lies in s_child; a run that does not fit whole stays in global memory
            long long at = 0;
            for (int i = 0; i < n_el; i++) {
                s_coff[i] = at + s_clen[i] <= LK_CHILD_LDS ? (int)at : -1;
                at = std::min<long long>(at + s_clen[i], LK_CHILD_LDS + 1);
            }
            s_coff[n_el] = (int)std::min<long long>(at, LK_CHILD_LDS);
        }
        __syncthreads();
        for (int pos = tid; pos < s_coff[n_el]; pos += 256) {
            int lo = 0, hi = n_el - 1;           // the last element whose run starts at or before pos: the runs that fit are a prefix, back to back
            while (lo < hi) {
                const int mid = (lo + hi + 1) / 2;
                if (s_coff[mid] >= 0 && s_coff[mid] <= pos) lo = mid; else hi = mid - 1;
            }
            int c = -1;
            if (s_coff[lo] >= 0 && pos - s_coff[lo] < s_clen[lo]) {
                c = a.g.child_pool[s_cglob[lo] + (pos - s_coff[lo])];
                if (!(lk_usable(a, c) && a.g.state[c] == 1)) c = -1;
            }
            s_child[pos] = c;
        }
    }
    __syncthreads();
    if (wave == 0) {
        int size = n0, reason = 0, added_nb = 0, added_child = 0, added_par = 0;
        for (int i = 0; i < n_el; i++) {         // :1895-1945 (itEndKF is taken once: the first list only)
            if (size > LK_LIMIT) { reason = 1; break; }
            {
                const int c = lane < LK_NEIGH ? s_nb[i * LK_NEIGH + lane] : -1;
                const u64 m = __ballot(c >= 0 && !lk_member(a, s_bits, c));
                if (m) { lk_add(a, s_bits, lane, __shfl(c, __ffsll((long long)m) - 1), size); added_nb++; }
            }
            for (int base = 0; base < s_clen[i]; base += 64) {
                int c = -1;
                if (base + lane < s_clen[i]) {
                    if (s_coff[i] >= 0) c = s_child[s_coff[i] + base + lane];
                    else {
                        c = a.g.child_pool[s_cglob[i] + base + lane];
                        if (!(lk_usable(a, c) && a.g.state[c] == 1)) c = -1;
                    }
                }
                const u64 m = __ballot(c >= 0 && !lk_member(a, s_bits, c));
                if (m) { lk_add(a, s_bits, lane, __shfl(c, __ffsll((long long)m) - 1), size); added_child++; break; }
            }
            const int p = s_par[i];
            if (p >= 0 && !lk_member(a, s_bits, p)) {                    // whatever its state; the break leaves the outer loop (:1941)
                lk_add(a, s_bits, lane, p, size);
                added_par++; reason = 2;
                break;
            }
        }
        if (!kept && n_first > LK_LIMIT) reason = 1;
        if (lane == 0) {
            s_n[0] = size; s_n[1] = reason;
            a.stats[2] = size; a.stats[3] = added_nb; a.stats[4] = added_child; a.stats[5] = added_par; a.stats[7] = reason;
        }
    }
    __syncthreads();                             // (the slots wave 0 appended are visible to the workgroup behind it)
    const int n_local = s_n[0];
    // local_kf_start: the running sum of the run lengths, an absent slot or an invalid run counting 0
    long long carry = 0;
    for (int base = 0; base < a.kf_capacity; base += 256) {
        const int i = base + tid;
        long long x = 0;
        if (i < n_local) {
            const int s = a.local_kf_slot[i];
            if (lk_usable(a, s) && lk_run_ok(a.g.point_off[s], a.g.point_len[s], a.g.pool_entries)) x = a.g.point_len[s];
        }
        long long inc = x;
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = __shfl_up(inc, d);
            if (lane >= d) inc += y;
        }
        __syncthreads();
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        long long before = 0, total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) before += s_wsum[w];
            total += s_wsum[w];
        }
        if (i < a.kf_capacity) a.local_kf_start[i] = (int)std::min<long long>(carry + before + inc - x, 0x7FFFFFFF);
        carry += total;
    }
    if (tid == 0) {
        const int E = (int)std::min<long long>(carry, 0x7FFFFFFF);
        a.local_kf_start[a.kf_capacity] = E;
        a.state_io[0] = n_local; a.state_io[1] = ref;
        a.counts[0] = n_counter; a.counts[1] = kept ? 0 : n_first; a.counts[2] = n_local; a.counts[3] = ref; a.counts[4] = E;
        a.counts[5] = !kept && n_first > a.kf_capacity; a.counts[6] = E > a.entry_capacity; a.counts[7] = kept;
    }
}

__global__ __launch_bounds__(256) void k_lk_gather(LocalKfArgs a, int copy_blocks)
{
    if ((int)blockIdx.x >= copy_blocks) {        // the frame's words back to all ones
        const long long k = (long long)(blockIdx.x - copy_blocks) * 256 + threadIdx.x;
        if (k < a.n_frame && a.frame_row) {
            const int r = a.frame_row[k];
            if (lk_row_ok(a, r)) a.word[r] = LK_CLEAN;
        }
        return;
    }
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= a.entry_capacity) return;
    int v = -1;
    if (p < a.local_kf_start[a.kf_capacity]) {
        int lo = 0, hi = a.kf_capacity - 1;      // the last keyframe whose run starts at or before p: the one that holds it (empty runs lie before it)
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (a.local_kf_start[mid] <= p) lo = mid; else hi = mid - 1;
        }
        const int s = a.local_kf_slot[lo], j = p - a.local_kf_start[lo];
        if (lk_usable(a, s)) {
            const int off = a.g.point_off[s], len = a.g.point_len[s];
            if (lk_run_ok(off, len, a.g.pool_entries) && j < len) v = a.g.point_pool[off + j];
        }
    }
    a.local_point_row[p] = v;
}

int local_kf_member_lds() { return LK_MEMBER_LDS; }
int local_kf_child_lds() { return LK_CHILD_LDS; }

// Launch shapes from S, n_frame and the capacities alone.
void launch_local_keyframes(const LocalKfArgs &a, hipStream_t s)
{
    const int slot_blocks = (a.g.max_keyframes + 3) / 4, kp_blocks = (a.n_frame + 255) / 256, copy_blocks = (a.entry_capacity + 255) / 256;
    hipLaunchKernelGGL(k_lk_marks, dim3(std::max(kp_blocks, 1)), dim3(256), 0, s, a);
    if (slot_blocks > 0) {
        hipLaunchKernelGGL(k_lk_votes, dim3(slot_blocks), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_lk_rank, dim3(slot_blocks), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_lk_expand, dim3(1), dim3(256), 0, s, a);
    if (copy_blocks + kp_blocks > 0) hipLaunchKernelGGL(k_lk_gather, dim3(copy_blocks + kp_blocks), dim3(256), 0, s, a, copy_blocks);
}

} // namespace jsorb
