// k_kf_culling.hip - redundant keyframes culled on the device: LocalMapping::KeyFrameCulling (LocalMapping.cpp:638-702) with KeyFrame::SetBadFlag
// (KeyFrame.cpp:457-549) and MapPoint::EraseObservation / SetBadFlag (MapPoint.cpp:142-168, :182-199).  The contract: include/jsorb.h,
// jsorb_cull_keyframes_async.  Integer work except the depth gate (float) and the 0.9 comparison (double).
// The reference reads a point's observations through the point; here the observations are grouped by row once per call (a CSR over the table's
// rows: count, scan, scatter), and every later step reads a row's list and checks each entry against the CURRENT state[], registered[],
// point_pool[] and bad[] - the call only ever clears observations, so the lists stay a superset of what is live.  The candidates are then decided
// in rounds, one culled keyframe per round: everything in front of the first cull is final, because nothing earlier changes the state.
// k_kc_init          the outputs' padding, the counts, the scratch's counters
// k_kc_count         a wave per slot: its run by coalesced loads, one atomic per observation into cnt[row]
// k_kc_scan_blocks   a workgroup per 256 rows: the exclusive scan of cnt inside the block, the block's sum
// k_kc_scan_top      one workgroup: the exclusive scan of the blocks' sums
// k_kc_scatter       a wave per slot: (slot, entry) of every observation into its row's list (order inside a list is free: nothing depends on it)
// k_kc_eval          a workgroup per candidate at or behind the cursor: skipped / n_mps / n_redundant / the verdict on the current state
// k_kc_pick          one workgroup: the first candidate that is culled and may be erased; the decisions up to it, to_be_erased, the cursor
// k_cv_erase_dev     (k_covisibility.hip) EraseConnection on every key of the culled slot's map
// k_kc_apply         one workgroup: the slot's own map emptied, its observations erased, rows turned bad, ref_slot, state, the spanning tree
// k_kc_finish        the counts copied for jsorb_cull_keyframes_stats
// No kernel waits for another workgroup: order comes from the launches.  Every loop is bounded by a host-given size, and every slot, row and run
// read from device memory is used only after a range check.  LDS: k_kc_eval 16 bytes, k_kc_pick 20, k_kc_apply 3 088, k_kc_scan_* 1 028 - none
// limits the occupancy (k_cv_erase_dev's 41 600 bytes of sort buffers do: three workgroups per CU, as in jsorb_erase_connections_async).
#include <algorithm>

#include "jsorb_launch.h"

namespace jsorb {

namespace {

enum { CTL_CURSOR = 0, CTL_DONE = 1, CTL_SLOT = 2, CTL_CULLED = 3 };
enum { KC_NEIGH = 10 };

__device__ __forceinline__ bool kc_row_ok(const CullArgs &a, int r) { return r >= 0 && r < a.n_rows; }
__device__ __forceinline__ bool kc_slot_ok(int s, int S) { return s >= 0 && s < S; }
__device__ __forceinline__ bool kc_run_ok(int off, int len, int entries) { return off >= 0 && len >= 0 && (long long)off + len <= entries; }
__device__ __forceinline__ bool kc_key_less(long long ka, int sa, long long kb, int sb) { return ka < kb || (ka == kb && sa < sb); }
__device__ __forceinline__ int kc_row_start(const CullArgs &a, int r) { return a.off[r] + a.bsum[r / KC_SCAN]; }
// entry e of slot B's run (B in range, its run valid: the lists hold nothing else) is an observation of the good row r now
__device__ __forceinline__ bool kc_live(const CullArgs &a, int B, int e, int r) { return a.st.state[B] == 1 && a.st.registered[e] != 0 && a.st.point_pool[e] == r; }

__global__ __launch_bounds__(256) void k_kc_init(CullArgs a, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i < a.n_rows) { a.cnt[i] = 0; a.fill[i] = 0; }
    if (i < a.g.max_keyframes) a.pmark[i] = 0;
    if (i < a.n_cand) { a.decision[i] = -1; a.n_mps[i] = 0; a.n_redundant[i] = 0; }
    if (i < a.max_cull) a.culled_slot[i] = -1;
    for (int j = i; j < 2 * a.reparent_cap; j += n) a.reparent_out[j] = -1;       // (strided: the grid does not follow reparent_cap)
    if (i < KC_COUNTS) a.counts[i] = 0;
    if (i < 8) a.ctl[i] = i == CTL_SLOT ? -1 : 0;
    if (i < 2) a.erase_counts[i] = 0;
}

// count: cnt[row]++, scatter: the entry into the row's list
template <bool SCATTER> __device__ __forceinline__ void kc_walk_slot(const CullArgs &a)
{
    const int lane = threadIdx.x % 64, s = blockIdx.x * 4 + threadIdx.x / 64, S = a.g.max_keyframes;
    if (s >= S || a.st.state[s] != 1) return;
    const int off = a.g.point_off[s], len = a.g.point_len[s];
    if (!kc_run_ok(off, len, a.g.pool_entries)) return;
    for (int j = lane; j < len; j += 64) {
        const int e = off + j, r = a.st.point_pool[e];
        if (!kc_row_ok(a, r) || a.st.bad[r] || !a.st.registered[e]) continue;
        if (!SCATTER) atomicAdd(&a.cnt[r], 1);
        else {
            const int p = kc_row_start(a, r) + atomicAdd(&a.fill[r], 1);
            if (p >= 0 && p < a.g.pool_entries) { a.csr_slot[p] = s; a.csr_ent[p] = e; }       // (the lists' total is at most pool_entries)
        }
    }
}
__global__ __launch_bounds__(256) void k_kc_count(CullArgs a) { kc_walk_slot<false>(a); }
__global__ __launch_bounds__(256) void k_kc_scatter(CullArgs a) { kc_walk_slot<true>(a); }

// exclusive scan of v over the workgroup's 256 threads; *total = the sum
__device__ __forceinline__ int kc_scan256(int v, int *s_buf, int *total)
{
    const int tid = threadIdx.x;
    s_buf[tid] = v;
    __syncthreads();
    for (int d = 1; d < KC_SCAN; d <<= 1) {
        const int t = tid >= d ? s_buf[tid - d] : 0;
        __syncthreads();
        s_buf[tid] += t;
        __syncthreads();
    }
    const int incl = s_buf[tid];
    *total = s_buf[KC_SCAN - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(KC_SCAN) void k_kc_scan_blocks(CullArgs a)
{
    __shared__ int s_buf[KC_SCAN];
    const int r = blockIdx.x * KC_SCAN + threadIdx.x;
    int total;
    const int ex = kc_scan256(r < a.n_rows ? a.cnt[r] : 0, s_buf, &total);
    if (r < a.n_rows) a.off[r] = ex;
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(KC_SCAN) void k_kc_scan_top(CullArgs a, int n_blocks)
{
    __shared__ int s_buf[KC_SCAN];
    int carry = 0;
    for (int base = 0; base < n_blocks; base += KC_SCAN) {
        const int b = base + threadIdx.x;
        int total;
        const int ex = kc_scan256(b < n_blocks ? a.bsum[b] : 0, s_buf, &total);
        if (b < n_blocks) a.bsum[b] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(256) void k_kc_eval(CullArgs a)
{
    __shared__ int s_acc[2];
    const int i = blockIdx.x, tid = threadIdx.x, S = a.g.max_keyframes;
    if (a.ctl[CTL_DONE] || i < a.ctl[CTL_CURSOR]) return;
    const int A = a.cand_slot[i];
    int off = 0, len = 0;
    bool ok = kc_slot_ok(A, S) && a.st.state[A] == 1 && A != a.first_slot;
    if (ok) {
        off = a.g.point_off[A]; len = a.g.point_len[A];
        ok = kc_run_ok(off, len, a.g.pool_entries);
    }
    int dup = 0;
    for (int f = tid; f < i; f += 256) dup |= a.cand_slot[f] == A;
    if (tid < 2) s_acc[tid] = 0;
    dup = __syncthreads_or(dup);
    int32_t *ev = a.ev + (size_t)i * 3;
    if (!ok || dup) {
        if (tid == 0) { ev[0] = 3; ev[1] = 0; ev[2] = 0; }
        return;
    }
    int mps = 0, red = 0;
    for (int j = tid; j < len; j += 256) {       // :657-697
        const int e = off + j, r = a.st.point_pool[e];
        if (!kc_row_ok(a, r) || a.st.bad[r]) continue;
        if (!a.monocular) {
            const float d = a.v.depth[e];
            if (d > a.v.th_depth[A] || d < 0) continue;                  // :666, literally: a NaN passes
        }
        mps++;
        const int oct = a.v.octave[e], p0 = kc_row_start(a, r), n = a.cnt[r];
        int n_obs = 0, q = 0;
        for (int p = p0; p < p0 + n; p++) {
            if (p < 0 || p >= a.g.pool_entries) break;
            const int B = a.csr_slot[p], e2 = a.csr_ent[p];
            if (!kc_live(a, B, e2, r)) continue;
            n_obs += 1 + (a.v.stereo[e2] != 0);
            q += B != A && (int)a.v.octave[e2] <= oct + 1;               // :679-688 (the break at 3 only stops early)
        }
        red += n_obs > 3 && q >= 3;              // :671, :690
    }
    if (mps) atomicAdd(&s_acc[0], mps);
    if (red) atomicAdd(&s_acc[1], red);
    __syncthreads();
    if (tid == 0) {
        // :699, int against double as written.  It equals 10 * n_redundant > 9 * n_mps for every n_mps < 2^31: the product's relative error is
        // below a quarter ulp, so where 0.9 * n_mps is an integer (the multiples of 10) it rounds to that integer, and elsewhere it stays on its
        // side of the integers next to it.
        const bool cull = (double)s_acc[1] > 0.9 * (double)s_acc[0];
        ev[0] = cull ? 1 : 0; ev[1] = s_acc[0]; ev[2] = s_acc[1];
    }
}

__global__ __launch_bounds__(256) void k_kc_pick(CullArgs a)
{
    __shared__ int s_first, s_n[4];
    const int tid = threadIdx.x, S = a.g.max_keyframes;
    if (a.ctl[CTL_DONE]) return;                 // (ctl[CTL_SLOT] is -1 already)
    const int cursor = a.ctl[CTL_CURSOR];
    if (tid == 0) s_first = a.n_cand;
    if (tid < 4) s_n[tid] = 0;
    __syncthreads();
    for (int i = cursor + tid; i < a.n_cand; i += 256) {
        if (a.ev[(size_t)i * 3] != 1) continue;
        const int A = a.cand_slot[i];            // (in range: the verdict says so)
        if (a.st.not_erase && a.st.not_erase[A]) continue;
        atomicMin(&s_first, i);
        break;
    }
    __syncthreads();
    const int first = s_first, end = std::min(first, a.n_cand - 1);
    for (int i = cursor + tid; i <= end; i += 256) {
        const int32_t *ev = a.ev + (size_t)i * 3;
        int d = ev[0];
        if (d == 1 && i != first) {              // :463-467
            d = 2;
            const int A = a.cand_slot[i];
            if (kc_slot_ok(A, S)) a.st.to_be_erased[A] = 1;
        }
        a.decision[i] = d; a.n_mps[i] = ev[1]; a.n_redundant[i] = ev[2];
        atomicAdd(&s_n[d], 1);
    }
    __syncthreads();
    if (tid == 0) {
        a.counts[1] += s_n[0]; a.counts[2] += s_n[1]; a.counts[3] += s_n[2]; a.counts[4] += s_n[3];
        if (first < a.n_cand) {
            const int k = a.ctl[CTL_CULLED];
            if (k < a.max_cull) a.culled_slot[k] = a.cand_slot[first];
            a.ctl[CTL_SLOT] = a.cand_slot[first]; a.ctl[CTL_CURSOR] = first + 1; a.ctl[CTL_CULLED] = k + 1;
        } else {
            a.ctl[CTL_SLOT] = -1; a.ctl[CTL_CURSOR] = a.n_cand; a.ctl[CTL_DONE] = 1;
        }
    }
}

__device__ void kc_log_reparent(const CullArgs &a, int child, int parent)
{
    const int n = a.counts[8]++;
    if (n < a.reparent_cap) { a.reparent_out[(size_t)n * 2] = child; a.reparent_out[(size_t)n * 2 + 1] = parent; }
    else a.counts[9] = 1;
}

__global__ __launch_bounds__(256) void k_kc_apply(CullArgs a)
{
    __shared__ int s_n[4];                       // observations erased, rows turned bad, ref_slot entries moved, the children
    __shared__ int s_bw[256], s_bi[256], s_bp[256];
    const int tid = threadIdx.x, S = a.g.max_keyframes, C = a.cv.conn_capacity;
    const int A = a.ctl[CTL_SLOT];
    if (!kc_slot_ok(A, S)) return;               // (k_kc_pick writes the word in every round it runs, -1 with the done flag: nothing here resets it)
    if (tid < 4) s_n[tid] = 0;
    if (tid == 0) { a.cv.conn_len[A] = 0; a.cv.ord_len[A] = 0; }                 // :480-481
    if (a.neighbours && tid < KC_NEIGH) a.neighbours[(size_t)A * KC_NEIGH + tid] = -1;
    const int off = a.g.point_off[A], len = a.g.point_len[A];                    // (valid: k_kc_eval checked it)
    __syncthreads();
    // :473-475, EraseObservation on every entry that is an observation; the entries first, then each row once
    int n_er = 0;
    for (int j = tid; j < len; j += 256) {
        const int e = off + j, r = a.st.point_pool[e];
        const int obs = kc_row_ok(a, r) && !a.st.bad[r] && a.st.registered[e] != 0;
        a.was_obs[e] = obs;
        if (obs) { a.st.registered[e] = 0; n_er++; }
    }
    if (n_er) atomicAdd(&s_n[0], n_er);
    __threadfence_block();
    __syncthreads();
    for (int j = tid; j < len; j += 256) {
        const int e = off + j;
        if (!a.was_obs[e]) continue;
        const int r = a.st.point_pool[e], p0 = kc_row_start(a, r), n = a.cnt[r];
        bool owner = true;                       // a row the run lists twice is handled by its first erased entry
        int n_obs = 0, best = -1;
        long long best_key = 0;
        for (int p = p0; p < p0 + n; p++) {
            if (p < 0 || p >= a.g.pool_entries) break;
            const int B = a.csr_slot[p], e2 = a.csr_ent[p];
            if (B == A) { owner = owner && !(e2 < e && a.was_obs[e2]); continue; }
            if (!kc_live(a, B, e2, r)) continue;
            n_obs += 1 + (a.v.stereo[e2] != 0);
            const long long k = a.g.order_key[B];
            if (best < 0 || kc_key_less(k, B, best_key, best)) { best = B; best_key = k; }
        }
        if (!owner) continue;
        if (a.st.ref_slot && a.st.ref_slot[r] == A) { a.st.ref_slot[r] = best; atomicAdd(&s_n[2], 1); }       // MapPoint.cpp:157-158
        if (n_obs > 2) continue;
        a.st.bad[r] = 1;                         // MapPoint.cpp:160-167, :182-199
        atomicAdd(&s_n[1], 1);
        for (int p = p0; p < p0 + n; p++) {
            if (p < 0 || p >= a.g.pool_entries) break;
            const int B = a.csr_slot[p], e2 = a.csr_ent[p];
            if (B == A || !kc_live(a, B, e2, r)) continue;
            a.st.point_pool[e2] = -1; a.st.registered[e2] = 0;
        }
    }
    __syncthreads();
    // the spanning tree, :483-541
    const int stamp = a.ctl[CTL_CULLED];         // (at least 1, and another one for every cull of the call)
    const int par = a.st.parent[A];
    if (tid == 0) {
        a.st.state[A] = 2;
        if (kc_slot_ok(par, S) && a.st.state[par] != 0 && par != A) a.pmark[par] = stamp;
    }
    for (int s = tid; s < S; s += 256)
        if (s != A && a.st.parent[s] == A && a.st.state[s] != 0) a.ch_raw[atomicAdd(&s_n[3], 1)] = s;
    __threadfence_block();
    __syncthreads();
    const int n_ch = s_n[3];
    for (int e = tid; e < n_ch; e += 256) {      // std::set<KeyFrame*>'s order by counting rank
        const int c = a.ch_raw[e];
        const long long k = a.g.order_key[c];
        int rank = 0;
        for (int f = 0; f < n_ch; f++) rank += kc_key_less(a.g.order_key[a.ch_raw[f]], a.ch_raw[f], k, c);
        a.ch[rank] = c; a.ch_done[e] = 0;
    }
    __threadfence_block();
    __syncthreads();
    for (int pass = 0; pass < n_ch; pass++) {
        int bw = -1, bi = -1, bp = -1;           // int max = -1 (:493); a thread meets its pairs in (child, list position) order
        for (int idx = tid; idx < n_ch; idx += 256) {
            const int c = a.ch[idx];
            if (a.ch_done[idx] || a.st.state[c] != 1) continue;                  // :500
            const int n_ord = std::min(std::max(a.cv.ord_len[c], 0), C), n_conn = std::min(std::max(a.cv.conn_len[c], 0), C);
            for (int j = 0; j < n_ord; j++) {
                const int p = a.cv.ord_slot[(size_t)c * C + j];
                if (!kc_slot_ok(p, S) || a.pmark[p] != stamp) continue;
                int w = 0;                       // GetWeight: 0 when the map lacks it
                for (int f = 0; f < n_conn; f++)
                    if (a.cv.conn_slot[(size_t)c * C + f] == p) { w = a.cv.conn_weight[(size_t)c * C + f]; break; }
                if (w > bw) { bw = w; bi = idx; bp = p; }
            }
        }
        s_bw[tid] = bw; s_bi[tid] = bi; s_bp[tid] = bp;
        __syncthreads();
        if (tid == 0) {
            for (int t = 1; t < 256; t++)
                if (s_bi[t] >= 0 && (s_bw[t] > bw || (s_bw[t] == bw && s_bi[t] < bi))) { bw = s_bw[t]; bi = s_bi[t]; bp = s_bp[t]; }
            s_bi[0] = bi;
            if (bi >= 0) {
                const int c = a.ch[bi];
                a.st.parent[c] = bp; a.pmark[c] = stamp; a.ch_done[bi] = 1;     // :526-528
                kc_log_reparent(a, c, bp);
            }
        }
        __threadfence_block();
        __syncthreads();
        const int found = s_bi[0];
        __syncthreads();
        if (found < 0) break;                    // :530-531
    }
    if (tid == 0) {
        for (int idx = 0; idx < n_ch; idx++)     // :535-539, in the set's order
            if (!a.ch_done[idx]) { a.st.parent[a.ch[idx]] = par; kc_log_reparent(a, a.ch[idx], par); }
        a.counts[5] += s_n[1]; a.counts[6] += s_n[0]; a.counts[7] += s_n[2];
    }
}

__global__ void k_kc_finish(CullArgs a)
{
    const int tid = threadIdx.x;
    if (tid == 0) a.counts[0] = a.ctl[CTL_CURSOR];
    __syncthreads();
    if (tid < KC_COUNTS) a.stats[tid] = a.counts[tid];
}

} // namespace

// Launch shapes from S, n_rows, n_cand, max_cull and C alone.
void launch_cull_keyframes(const CullArgs &a, hipStream_t s)
{
    const int S = a.g.max_keyframes, n_blocks = (a.n_rows + KC_SCAN - 1) / KC_SCAN;
    const int n_init = std::max({a.n_rows, S, a.n_cand, (int)KC_MAX_CULL});
    hipLaunchKernelGGL(k_kc_init, dim3((n_init + 255) / 256), dim3(256), 0, s, a, n_init);
    if (S > 0 && a.n_rows > 0) {
        hipLaunchKernelGGL(k_kc_count, dim3((S + 3) / 4), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_kc_scan_blocks, dim3(n_blocks), dim3(KC_SCAN), 0, s, a);
        hipLaunchKernelGGL(k_kc_scan_top, dim3(1), dim3(KC_SCAN), 0, s, a, n_blocks);
        hipLaunchKernelGGL(k_kc_scatter, dim3((S + 3) / 4), dim3(256), 0, s, a);
    }
    if (a.n_cand > 0)
        for (int round = 0; round < a.max_cull; round++) {
            hipLaunchKernelGGL(k_kc_eval, dim3(a.n_cand), dim3(256), 0, s, a);
            hipLaunchKernelGGL(k_kc_pick, dim3(1), dim3(256), 0, s, a);
            launch_erase_connections_dev(a.cv, a.neighbours, a.g.order_key, a.ctl + CTL_SLOT, a.erase_counts, s);
            hipLaunchKernelGGL(k_kc_apply, dim3(1), dim3(256), 0, s, a);
        }
    hipLaunchKernelGGL(k_kc_finish, dim3(1), dim3(64), 0, s, a);
}

} // namespace jsorb
