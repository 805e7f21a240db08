// k_covisibility.hip - the covisibility graph kept on the device: KeyFrame::UpdateConnections (KeyFrame.cpp:293-383) with AddConnection /
// UpdateBestCovisibles (:127-161) for up to 32 keyframes one after the other in one call, SetBadFlag's EraseConnection walk (:470-471, :480-481,
// :557-571), GetConnectedKeyFrames (:163-170) and GetBestCovisibilityKeyFrames (:178-186).  The contract: include/jsorb.h,
// jsorb_update_connections_async.  Integer work only.
// The reference counts, for every point of the keyframe, the keyframes in the point's observations; here member i sets bit i in the scratch word
// of each of its rows and every slot counts, per bit, the registered entries of its own run whose word has the bit - the same number, and the
// counts depend only on runs that no member changes.  The sequence of updates then has a closed form per slot (tests/covis_cases.py proves it
// against a literal transcription): a slot that is member q ends with K of its own update plus the AddConnections of the members behind q, any
// other slot with its old map plus all members' AddConnections, and its ordered list is the full re-sort exactly when one of those changed its map.
// k_cv_marks    a workgroup per member: validity (usable, valid run, not listed before), bit i of word[row] by atomicOr over rows(A) (:306-314)
// k_cv_counts   a wave per slot: the run by coalesced loads, the words gathered, skipped when the ballot of non-zero words is empty, a popcount
//               per member bit into count[32][S] (:316-323)
// k_cv_select   a workgroup per member: K compacted and put in (order_key, slot) order by counting rank, the first strict maximum (:338-344),
//               T sorted descending by counting rank (:358-365), parent_out and first_connection (:375-380), the snapshot
// k_cv_apply    a workgroup per slot that leaves at once when it is no member and no member targets it: base and incoming connections merged in
//               LDS, the map in key order and the list re-sorted by counting rank, the slot's neighbours row
// k_cv_reset    a workgroup per member: its rows' words back to zero; the counts copied for jsorb_update_connections_stats
// k_cv_erase    a workgroup per key of the erased slot's map (EraseConnection), k_cv_erase_clear empties the slot itself; k_cv_erase_dev is the
//               same walk for a slot read from device memory (the keyframe culling's rounds, k_kf_culling.hip)
// k_cv_mask, k_cv_best   the two getters
// Every slot, row and run read from device memory is used only after a range check: nothing is read or written outside the arrays whatever they
// hold.
#include <algorithm>

#include "jsorb_launch.h"

#ifndef CV_CAP_MAX
#define CV_CAP_MAX 2048                          // the largest conn_capacity: a map of that many entries and 32 incoming ones are sorted in one workgroup's LDS (a test build lowers it: jetson_slam_amd/build.py VARIANTS)
#endif
#define CV_CAP_MIN 16
#define CV_TH 15                                 // :334
#define CV_NEIGH 10                              // the rows of jsorb_keyframe_graph.neighbours
#define CV_LDS (CV_CAP_MAX + CV_MAX_UPDATE)

namespace jsorb {

static_assert(CV_CAP_MAX >= CV_CAP_MIN && CV_CAP_MAX <= 2048, "slot, weight, key and rank of CV_CAP_MAX + 32 entries fit 64 KiB of LDS");

typedef unsigned long long u64;

__device__ __forceinline__ bool cv_row_ok(const CovisArgs &a, int r) { return r >= 0 && r < a.n_rows; }
__device__ __forceinline__ bool cv_slot_ok(int s, int S) { return s >= 0 && s < S; }
__device__ __forceinline__ bool cv_run_ok(int off, int len, int entries) { return off >= 0 && len >= 0 && (long long)off + len <= entries; }
__device__ __forceinline__ int cv_clamp_len(int len, int C) { return std::min(std::max(len, 0), C); }
// std::map<KeyFrame*, int>'s order, equal keys by slot
__device__ __forceinline__ bool cv_key_less(long long ka, int sa, long long kb, int sb) { return ka < kb || (ka == kb && sa < sb); }
// the order of the ordered lists: sort() of pair<int, KeyFrame*> and push_front, i.e. (weight, key, slot) descending; true when a comes first
__device__ __forceinline__ bool cv_ord_before(int wa, long long ka, int sa, int wb, long long kb, int sb)
{
    return wa > wb || (wa == wb && cv_key_less(kb, sb, ka, sa));
}

__global__ __launch_bounds__(256) void k_cv_marks(CovisArgs a)
{
    const int i = blockIdx.x, tid = threadIdx.x, S = a.g.max_keyframes;
    if (i == 0 && tid < 8) a.counts[tid] = 0;
    if (i >= a.n_update) return;
    const int A = a.update_slot[i];
    int off = 0, len = 0;
    bool ok = cv_slot_ok(A, S) && a.g.state[A] != 0;
    if (ok) {
        off = a.g.point_off[A]; len = a.g.point_len[A];
        ok = cv_run_ok(off, len, a.g.pool_entries);
    }
    const int dup = __syncthreads_or(tid < i && a.update_slot[tid] == A);        // (n_update <= 32 < 256)
    ok = ok && !dup;
    if (tid == 0) {
        a.minfo[i * 4 + 0] = ok ? A : -1;
        a.minfo[i * 4 + 1] = 0; a.minfo[i * 4 + 2] = 0; a.minfo[i * 4 + 3] = -1;
    }
    if (!ok) return;
    for (int j = tid; j < len; j += 256) {       // :306-314
        const int r = a.g.point_pool[off + j];
        if (cv_row_ok(a, r) && !a.bad[r]) atomicOr(&a.word[r], 1u << i);
    }
}

__global__ __launch_bounds__(256) void k_cv_counts(CovisArgs a)
{
    const int lane = threadIdx.x % 64, s = blockIdx.x * 4 + threadIdx.x / 64, S = a.g.max_keyframes;
    if (s >= S) return;                          // (uniform over the wave)
    int acc = 0;                                 // lane i: the count of member i
    if (a.g.state[s] != 0) {
        const int off = a.g.point_off[s], len = a.g.point_len[s];
        if (cv_run_ok(off, len, a.g.pool_entries))
            for (int base = 0; base < len; base += 64) {
                unsigned w = 0;
                if (base + lane < len) {
                    const int r = a.g.point_pool[off + base + lane];
                    const bool reg = a.g.registered ? a.g.registered[off + base + lane] != 0 : true;
                    if (reg && cv_row_ok(a, r)) w = a.word[r];
                }
                if (__ballot(w != 0) == 0) continue;
                for (int i = 0; i < a.n_update; i++) {
                    const u64 m = __ballot((w >> i) & 1u);
                    if (lane == i) acc += __popcll(m);
                }
            }
    }
    if (lane < a.n_update) a.count[(size_t)lane * S + s] = a.minfo[lane * 4] == s ? 0 : acc;       // :320
}

__global__ __launch_bounds__(256) void k_cv_select(CovisArgs a)
{
    __shared__ int s_n[2];                       // |K|, the entries at or above the threshold
    __shared__ int s_bc[256], s_bs[256];         // per thread: the best count and its slot, lowest key among equals (:338-344)
    __shared__ int s_tc[256], s_ts[256];         // per thread: the front of the ordered list, largest key among equals
    const int i = blockIdx.x, tid = threadIdx.x, S = a.g.max_keyframes, C = a.cv.conn_capacity;
    const int A = a.minfo[i * 4];
    if (A < 0) {
        if (tid == 0) {
            if (a.parent_out) a.parent_out[i] = -1;
            if (a.snap_len) a.snap_len[i] = -1;
            atomicAdd(&a.counts[1], 1);
        }
        return;
    }
    if (tid < 2) s_n[tid] = 0;
    __syncthreads();
    const int32_t *cnt = a.count + (size_t)i * S;
    int32_t *raw = a.kraw + (size_t)i * S, *kl = a.klist + (size_t)i * S, *tl = a.tlist + (size_t)i * S;
    int bc = 0, bs = -1, tc = 0, ts = -1;
    long long bk = 0, tk = 0;
    for (int B = tid; B < S; B += 256) {
        const int c = cnt[B];
        if (c <= 0) continue;
        raw[atomicAdd(&s_n[0], 1)] = B;          // (at most S entries)
        if (c >= CV_TH) atomicAdd(&s_n[1], 1);
        const long long k = a.g.order_key[B];
        if (c > bc || (c == bc && cv_key_less(k, B, bk, bs))) { bc = c; bs = B; bk = k; }
        if (ts < 0 || cv_ord_before(c, k, B, tc, tk, ts)) { tc = c; ts = B; tk = k; }
    }
    s_bc[tid] = bc; s_bs[tid] = bs; s_tc[tid] = tc; s_ts[tid] = ts;
    __syncthreads();
    const int nK = s_n[0], nT = s_n[1];
    if (nK == 0) {                               // :327
        if (tid == 0) {
            if (a.parent_out) a.parent_out[i] = -1;
            if (a.snap_len) a.snap_len[i] = -1;
            atomicAdd(&a.counts[2], 1);
        }
        return;
    }
    if (tid == 0) {
        for (int t = 1; t < 256; t++) {
            if (s_bs[t] >= 0 && (s_bc[t] > bc || (s_bc[t] == bc && cv_key_less(a.g.order_key[s_bs[t]], s_bs[t], bk, bs)))) {
                bc = s_bc[t]; bs = s_bs[t]; bk = a.g.order_key[bs];
            }
            if (s_ts[t] >= 0 && cv_ord_before(s_tc[t], a.g.order_key[s_ts[t]], s_ts[t], tc, tk, ts)) { tc = s_tc[t]; ts = s_ts[t]; tk = a.g.order_key[ts]; }
        }
        s_bs[0] = bs; s_ts[0] = ts;
    }
    __syncthreads();
    const int fallback = nT == 0 ? s_bs[0] : -1; // :352-356
    const int front = nT == 0 ? s_bs[0] : s_ts[0];
    for (int e = tid; e < nK; e += 256) {
        const int B = raw[e], c = cnt[B];
        const long long k = a.g.order_key[B];
        const bool inT = c >= CV_TH || B == fallback;
        int kr = 0, tr = 0;
        for (int f = 0; f < nK; f++) {
            const int Bf = raw[f], cf = cnt[Bf];
            const long long kf = a.g.order_key[Bf];
            kr += cv_key_less(kf, Bf, k, B);
            tr += (cf >= CV_TH || Bf == fallback) && cv_ord_before(cf, kf, Bf, c, k, B);
        }
        kl[kr] = B;                              // (ranks are distinct and below nK <= S)
        if (inT) tl[tr] = B;
        if (a.snap_len && kr < C) { a.snap_slot[(size_t)i * C + kr] = B; a.snap_weight[(size_t)i * C + kr] = c; }
    }
    if (tid == 0) {
        a.minfo[i * 4 + 1] = nK; a.minfo[i * 4 + 2] = nT == 0 ? 1 : nT; a.minfo[i * 4 + 3] = fallback;
        if (a.snap_len) a.snap_len[i] = std::min(nK, C);
        const bool first = a.cv.first_connection[A] != 0;                // :375-380
        if (a.parent_out) a.parent_out[i] = first ? front : -1;
        a.cv.first_connection[A] = 0;
        atomicAdd(&a.counts[0], 1);
        atomicAdd(&a.counts[3], nT == 0 ? 1 : nT);
        if (nT == 0) atomicAdd(&a.counts[5], 1);
    }
}

// The n entries in LDS (slot < 0: dropped) become slot B's map: the C lowest in (order_key, slot) order.  resort: its ordered list becomes that
// map by (weight, key, slot) descending (UpdateBestCovisibles, :142-161), and its neighbours row the first 10 of it.  Returns the entries before the cut at C.
// s_kr is scratch of n words.  The whole workgroup calls it.
__device__ int cv_store(const jsorb_covisibility &cv, int32_t *neighbours, int B, int n, const int *s_slot, const int *s_w, const long long *s_key, int *s_kr,
                        bool resort)
{
    const int tid = threadIdx.x, C = cv.conn_capacity;
    for (int e = tid; e < n; e += 256) {
        int kr = -1;
        if (s_slot[e] >= 0) {
            kr = 0;
            for (int f = 0; f < n; f++) kr += s_slot[f] >= 0 && cv_key_less(s_key[f], s_slot[f], s_key[e], s_slot[e]);
        }
        s_kr[e] = kr;
    }
    int n_valid = 0;
    __syncthreads();
    for (int e = 0; e < n; e++) n_valid += s_kr[e] >= 0;                 // (every thread counts the same; n <= CV_LDS)
    const int kept = std::min(n_valid, C);
    for (int e = tid; e < n; e += 256) {
        const int kr = s_kr[e];
        if (kr < 0 || kr >= C) continue;
        cv.conn_slot[(size_t)B * C + kr] = s_slot[e]; cv.conn_weight[(size_t)B * C + kr] = s_w[e];
        if (resort) {
            int r = 0;
            for (int f = 0; f < n; f++) r += s_kr[f] >= 0 && s_kr[f] < C && cv_ord_before(s_w[f], s_key[f], s_slot[f], s_w[e], s_key[e], s_slot[e]);
            cv.ord_slot[(size_t)B * C + r] = s_slot[e]; cv.ord_weight[(size_t)B * C + r] = s_w[e];
            if (neighbours && r < CV_NEIGH) neighbours[(size_t)B * CV_NEIGH + r] = s_slot[e];
        }
    }
    if (tid == 0) {
        cv.conn_len[B] = kept;
        if (resort) cv.ord_len[B] = kept;
    }
    if (resort && neighbours && tid >= kept && tid < CV_NEIGH) neighbours[(size_t)B * CV_NEIGH + tid] = -1;
    return n_valid;
}

__global__ __launch_bounds__(256) void k_cv_apply(CovisArgs a)
{
    __shared__ int s_slot[CV_LDS], s_w[CV_LDS], s_kr[CV_LDS];
    __shared__ long long s_key[CV_LDS];
    __shared__ int s_in_slot[CV_MAX_UPDATE], s_in_w[CV_MAX_UPDATE], s_in_new[CV_MAX_UPDATE], s_in_chg[CV_MAX_UPDATE];
    __shared__ int s_res[3];                     // entries after the merge, whether a connection changed the map, the connections that are new
    const int B = blockIdx.x, tid = threadIdx.x, lane = tid % 64, S = a.g.max_keyframes, C = a.cv.conn_capacity;
    // which member this slot is, and which members behind it target it: every wave works it out for itself (uniform over the workgroup)
    int Aj = -1, nKj = 0, cj = 0;
    if (lane < a.n_update) {
        Aj = a.minfo[lane * 4]; nKj = a.minfo[lane * 4 + 1];
        if (Aj >= 0 && nKj > 0 && Aj != B) cj = a.count[(size_t)lane * S + B];
    }
    const u64 qm = __ballot(Aj == B && nKj > 0);
    const int q = qm ? __ffsll((long long)qm) - 1 : -1;
    const u64 in = __ballot(lane > q && cj > 0 && (cj >= CV_TH || a.minfo[lane * 4 + 3] == B));
    if (q < 0 && in == 0) return;
    const int n_in = __popcll(in);
    if (tid < 64 && ((in >> lane) & 1)) {
        const int t = __popcll(in & ((1ull << lane) - 1));
        s_in_slot[t] = Aj; s_in_w[t] = cj;
    }
    // the base: K of the slot's own update (its C lowest keys; the rest cannot be among the C lowest of the merge), or its stored map
    const int32_t *cq = q >= 0 ? a.count + (size_t)q * S : nullptr;
    const int nK = q >= 0 ? a.minfo[q * 4 + 1] : 0;
    const int nb = q >= 0 ? std::min(nK, C) : cv_clamp_len(a.cv.conn_len[B], C);
    for (int e = tid; e < nb; e += 256) {
        int s, w;
        if (q >= 0) { s = a.klist[(size_t)q * S + e]; w = cv_slot_ok(s, S) ? cq[s] : 0; }
        else { s = a.cv.conn_slot[(size_t)B * C + e]; w = a.cv.conn_weight[(size_t)B * C + e]; }
        if (!cv_slot_ok(s, S)) s = -1;
        s_slot[e] = s; s_w[e] = w; s_key[e] = s >= 0 ? a.g.order_key[s] : 0;
    }
    __syncthreads();
    if (tid < n_in) {                            // AddConnection (:127-140): absent, another weight, or the early return
        const int s = s_in_slot[tid], w = s_in_w[tid];
        int found = 0, chg = 0;
        for (int e = 0; e < nb; e++)
            if (s_slot[e] == s) {                // (incoming slots are distinct: each writes its own entry)
                found = 1;
                if (s_w[e] != w) { s_w[e] = w; chg = 1; }
                break;
            }
        if (!found && q >= 0 && cq[s] > 0) { found = 1; chg = cq[s] != w; }      // in K beyond the C lowest keys
        s_in_new[tid] = !found; s_in_chg[tid] = chg || !found;
    }
    __syncthreads();
    if (tid == 0) {
        int n = nb, chg = 0, n_new = 0;
        for (int t = 0; t < n_in; t++) {
            chg |= s_in_chg[t];
            if (s_in_new[t]) {
                s_slot[n] = s_in_slot[t]; s_w[n] = s_in_w[t]; s_key[n] = a.g.order_key[s_in_slot[t]];
                n++; n_new++;
            }
        }
        s_res[0] = n; s_res[1] = chg; s_res[2] = n_new;
    }
    __syncthreads();
    const int n = s_res[0], chg = s_res[1];
    if (q < 0 && !chg) return;                   // every AddConnection returned early: the map and the list keep their form
    const int n_valid = cv_store(a.cv, a.neighbours, B, n, s_slot, s_w, s_key, s_kr, chg != 0);
    if (!chg) {                                  // the slot's own update alone: the list is T sorted (:358-373)
        const int nt = std::min(a.minfo[q * 4 + 2], C);
        for (int e = tid; e < nt; e += 256) {
            const int s = a.tlist[(size_t)q * S + e];
            a.cv.ord_slot[(size_t)B * C + e] = s; a.cv.ord_weight[(size_t)B * C + e] = cv_slot_ok(s, S) ? cq[s] : 0;
        }
        if (a.neighbours && tid < CV_NEIGH) a.neighbours[(size_t)B * CV_NEIGH + tid] = tid < nt ? a.tlist[(size_t)q * S + tid] : -1;
        if (tid == 0) a.cv.ord_len[B] = nt;
    }
    if (tid == 0) {
        if (chg) atomicAdd(&a.counts[4], 1);
        if ((q >= 0 ? nK + s_res[2] : n_valid) > C) atomicAdd(&a.counts[6], 1);       // the whole merge, K beyond the C lowest keys included
    }
}

__global__ __launch_bounds__(256) void k_cv_reset(CovisArgs a)
{
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i == 0 && tid < 8) a.stats[tid] = a.counts[tid];
    if (i >= a.n_update) return;
    const int A = a.minfo[i * 4];
    if (A < 0) return;
    const int off = a.g.point_off[A], len = a.g.point_len[A];
    if (!cv_run_ok(off, len, a.g.pool_entries)) return;
    for (int j = tid; j < len; j += 256) {
        const int r = a.g.point_pool[off + j];
        if (cv_row_ok(a, r)) a.word[r] = 0;
    }
}

// counts[2]: the keys walked, the maps that held the slot
__device__ __forceinline__ void cv_erase_body(const jsorb_covisibility &cv, int32_t *neighbours, const int64_t *order_key, int slot, int32_t *counts)
{
    __shared__ int s_slot[CV_LDS], s_w[CV_LDS], s_kr[CV_LDS];
    __shared__ long long s_key[CV_LDS];
    const int k = blockIdx.x, tid = threadIdx.x, S = cv.max_keyframes, C = cv.conn_capacity;
    const int len = cv_clamp_len(cv.conn_len[slot], C);
    if (k >= len) return;
    const int B = cv.conn_slot[(size_t)slot * C + k];
    if (!cv_slot_ok(B, S) || B == slot) return;
    int dup = 0;
    for (int f = tid; f < k; f += 256) dup |= cv.conn_slot[(size_t)slot * C + f] == B;
    if (__syncthreads_or(dup)) return;           // a key listed twice is walked once
    const int nb = cv_clamp_len(cv.conn_len[B], C);
    int held = 0;
    for (int e = tid; e < nb; e += 256) {
        int s = cv.conn_slot[(size_t)B * C + e];
        if (s == slot) { held = 1; s = -1; }     // :562-566
        if (!cv_slot_ok(s, S)) s = -1;
        s_slot[e] = s; s_w[e] = cv.conn_weight[(size_t)B * C + e]; s_key[e] = s >= 0 ? order_key[s] : 0;
    }
    held = __syncthreads_or(held);
    if (tid == 0) { atomicAdd(&counts[0], 1); if (held) atomicAdd(&counts[1], 1); }
    if (!held) return;                           // its map did not hold the slot: left alone, lists included
    cv_store(cv, neighbours, B, nb, s_slot, s_w, s_key, s_kr, true);
}

__global__ __launch_bounds__(256) void k_cv_erase(jsorb_covisibility cv, int32_t *neighbours, const int64_t *order_key, int slot, int32_t *counts)
{
    cv_erase_body(cv, neighbours, order_key, slot, counts);
}

// the same walk for a slot the device chose (jsorb_cull_keyframes_async, k_kf_culling.hip): *slot_dev < 0 = nothing to erase in this round
__global__ __launch_bounds__(256) void k_cv_erase_dev(jsorb_covisibility cv, int32_t *neighbours, const int64_t *order_key, const int32_t *slot_dev, int32_t *counts)
{
    const int slot = *slot_dev;
    if (!cv_slot_ok(slot, cv.max_keyframes)) return;                     // (uniform over the launch)
    cv_erase_body(cv, neighbours, order_key, slot, counts);
}

__global__ void k_cv_erase_clear(jsorb_covisibility cv, int32_t *neighbours, int slot)
{
    const int tid = threadIdx.x;
    if (tid == 0) { cv.conn_len[slot] = 0; cv.ord_len[slot] = 0; }       // :480-481
    if (neighbours && tid < CV_NEIGH) neighbours[(size_t)slot * CV_NEIGH + tid] = -1;
}

__global__ __launch_bounds__(256) void k_cv_mask(jsorb_covisibility cv, int slot, uint8_t *mask)
{
    const int k = blockIdx.x * 256 + threadIdx.x, C = cv.conn_capacity;
    if (k >= cv_clamp_len(cv.conn_len[slot], C)) return;
    const int s = cv.conn_slot[(size_t)slot * C + k];
    if (cv_slot_ok(s, cv.max_keyframes)) mask[s] = 1;
}

__global__ __launch_bounds__(256) void k_cv_best(jsorb_covisibility cv, int n, const int32_t *slots, int N, int32_t *out, int32_t *out_len)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long long)n * N) return;
    const int i = (int)(p / N), j = (int)(p % N), C = cv.conn_capacity;
    const int s = slots[i];
    const int len = cv_slot_ok(s, cv.max_keyframes) ? std::min(cv_clamp_len(cv.ord_len[s], C), N) : 0;
    int v = -1;
    if (j < len) {
        v = cv.ord_slot[(size_t)s * C + j];
        if (!cv_slot_ok(v, cv.max_keyframes)) v = -1;
    }
    out[p] = v;
    if (j == 0 && out_len) out_len[i] = len;
}

int covis_cap_min() { return CV_CAP_MIN; }
int covis_cap_max() { return CV_CAP_MAX; }

// Launch shapes from S, n_update and the capacities alone.
void launch_update_connections(const CovisArgs &a, hipStream_t s)
{
    const int S = a.g.max_keyframes, members = std::max(a.n_update, 1);
    hipLaunchKernelGGL(k_cv_marks, dim3(members), dim3(256), 0, s, a);
    if (a.n_update > 0) {                        // (no slots at all: every member is skipped, and k_cv_select still says so)
        if (S > 0) hipLaunchKernelGGL(k_cv_counts, dim3((S + 3) / 4), dim3(256), 0, s, a);
        hipLaunchKernelGGL(k_cv_select, dim3(a.n_update), dim3(256), 0, s, a);
        if (S > 0) hipLaunchKernelGGL(k_cv_apply, dim3(S), dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(k_cv_reset, dim3(members), dim3(256), 0, s, a);
}

void launch_erase_connections(const jsorb_covisibility &cv, int32_t *neighbours, const int64_t *order_key, int slot, int32_t *counts, hipStream_t s)
{
    hipLaunchKernelGGL(k_cv_erase, dim3(cv.conn_capacity), dim3(256), 0, s, cv, neighbours, order_key, slot, counts);
    hipLaunchKernelGGL(k_cv_erase_clear, dim3(1), dim3(64), 0, s, cv, neighbours, slot);
}

void launch_erase_connections_dev(const jsorb_covisibility &cv, int32_t *neighbours, const int64_t *order_key, const int32_t *slot_dev, int32_t *counts,
                                  hipStream_t s)
{
    hipLaunchKernelGGL(k_cv_erase_dev, dim3(cv.conn_capacity), dim3(256), 0, s, cv, neighbours, order_key, slot_dev, counts);
}

void launch_connected_mask(const jsorb_covisibility &cv, int slot, uint8_t *mask, hipStream_t s)
{
    hipLaunchKernelGGL(k_cv_mask, dim3((cv.conn_capacity + 255) / 256), dim3(256), 0, s, cv, slot, mask);
}

void launch_best_covisibles(const jsorb_covisibility &cv, int n, const int32_t *slots, int N, int32_t *out, int32_t *out_len, hipStream_t s)
{
    const long long total = (long long)n * N;
    if (total > 0) hipLaunchKernelGGL(k_cv_best, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cv, n, slots, N, out, out_len);
}

} // namespace jsorb
