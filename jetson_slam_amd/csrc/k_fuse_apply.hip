// k_fuse_apply.hip - ORBmatcher::Fuse WITH its map mutations over the device state (include/jsorb.h, jsorb_fuse_map_async): the head test
//   (ORBmatcher.cpp:833-837, :980-992), the tail (:939-958, :1071-1081), MapPoint::Replace / AddObservation (MapPoint.cpp:129-140, :208-246) and the
//   Replace loop of LoopClosing::SearchAndFuse (LoopClosing.cpp:609-616) on the graph's point_pool / registered and the table's bad / desc.  The
//   search itself is k_fuse_match_run (k_fuse.hip), the descriptors of the surviving points k_distinct.hip's kernels over the CSR built here.
// The observation index is threaded through the pool: head[row] is the first entry of the row's list, next[entry] the following one, ent_slot[entry]
// the slot whose run holds the entry.  AddObservation is a push; Replace walks the dying point's list and pushes what the survivor keeps onto the
// survivor's.  Nothing can overflow and nothing after the build costs n_rows.  A reader checks every entry against the current point_pool,
// registered and state, and every walk is bounded by pool_entries hops.
// k_fa_index     per call: blocks stride over the slots with state != 0 and a valid run, threads over the run; an entry with registered != 0 and a
//                row inside the table is claimed for the slot (one compare-and-swap: an entry that two overlapping runs hold belongs to one of
//                them) and pushed with one atomic exchange.  The order inside a list is free: nothing below depends on it.
// k_fa_snapshot  overload 2, per target: the rows in the target's run that are in range and not bad get the target's stamp (:980)
// k_fa_grid      per target, ONE workgroup: AssignFeaturesToGrid's CSR over the target's run (assign_grid_csr, as k_fuse_grids)
// k_fa_head      per target, a thread per list point: the head test at this moment -> the skip byte; the point's nine floats and its descriptor
//                (two 16-byte loads and stores) from the table row, in the layout k_fuse_match_run reads
// k_fa_apply     per target, ONE workgroup: steps 3 and 4.  The list is taken 256 entries at a time, the entries with best_idx >= 0 compacted in
//                order by ballots (a wave passes a run of 64 others in one step), and each of those is handled by the whole workgroup: thread 0
//                follows a list's links FA_CHUNK entries at a time into LDS, the threads check and count or rewrite the staged entries.
//                Whatever decides a branch (bad, the slot's point) is read by thread 0 alone, which is also the writer, and handed on through LDS
//                between two barriers (fa_decide): no wave sees the map before and another after a write.
//                Observations() is such a reduction.  In Replace(p -> q) the survivor's observers are stamped into slot_mark[] with the Replace's
//                own number, then p's entries are resolved against the stamps in parallel - each touches another keyframe.  The log slot comes from
//                one counter; "marked for this target" is a stamp, so nothing is cleared between targets.
// k_fa_csr       per target, ONE workgroup: the marked rows that are still good, each with its observations in slots of state 1 ranked by
//                (order_key, slot), as the CSR k_distinct_plan takes (out_row = the rows).  Marked rows own disjoint entries: pool_entries bounds it.
// k_fa_finish    per call: the counts.
// Order comes from the launches alone; no kernel waits for another workgroup; the launch shapes depend on S, n_rows, pool_entries, n_list and
// n_targets only.  Every slot, row, run, entry and keypoint index read from device memory is range-checked before it is used.
#include "jsorb_launch.h"
#include "k_search_common.h"

#ifndef FA_CHUNK
#define FA_CHUNK 256                             // entries of a list thread 0 stages in LDS at a time
#endif

namespace jsorb {

static_assert(FA_CHUNK >= 1 && FA_CHUNK <= 4096, "the staged chunk fits LDS");
static_assert(sizeof(FuseMapArgs) + 2 * sizeof(int) <= 4096, "the arguments must fit a launch");

#define FA_THREADS 256

__device__ __forceinline__ bool fa_row_ok(const FuseMapArgs &a, int r) { return r >= 0 && r < a.n_rows; }
__device__ __forceinline__ bool fa_target(const FuseMapArgs &a, int slot, int &off, int &len)
{
    return fuse_target_run(a.g.state, a.g.point_off, a.g.point_len, a.g.max_keyframes, a.g.pool_entries, slot, off, len);
}
// entry e is in the index as an entry of row r: it holds r, is registered and was claimed for a slot.  *slot: that slot
__device__ __forceinline__ bool fa_holds(const FuseMapArgs &a, int e, int r, int &slot)
{
    slot = a.ent_slot[e];
    return a.st.point_pool[e] == r && a.st.registered[e] != 0 && slot >= 0 && slot < a.g.max_keyframes;
}
__device__ __forceinline__ bool fa_key_less(long long ka, int sa, long long kb, int sb) { return ka < kb || (ka == kb && sa < sb); }

__global__ __launch_bounds__(256) void k_fa_index(FuseMapArgs a)
{
    const int S = a.g.max_keyframes, pool = a.g.pool_entries;
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        if (a.g.state[s] == 0) continue;
        const int off = a.g.point_off[s], len = a.g.point_len[s];
        if (off < 0 || len < 0 || (long long)off + len > pool) continue;
        for (int e = off + threadIdx.x; e < off + len; e += 256) {
            const int r = a.st.point_pool[e];
            if (a.st.registered[e] == 0 || !fa_row_ok(a, r)) continue;
            if (atomicCAS(&a.ent_slot[e], -1, s) != -1) continue;
            a.next[e] = atomicExch(&a.head[r], e);
        }
    }
}

__global__ __launch_bounds__(256) void k_fa_snapshot(FuseMapArgs a, int t, int slot)
{
    int off, len;
    if (!fa_target(a, slot, off, len)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    const int r = a.st.point_pool[off + i];
    if (fa_row_ok(a, r) && a.st.bad[r] == 0) a.snap[r] = t + 1;
}

__global__ __launch_bounds__(1024) void k_fa_grid(FuseMapArgs a, int slot)
{
    extern __shared__ int s_grid[];          // [n_cells] counts -> starts, [n_cells] cursors, [1024] scan scratch
    int off, len;
    fa_target(a, slot, off, len);            // (a skipped target: an empty grid)
    const float *x = a.kp.x + off, *y = a.kp.y + off;
    const jsorb_fuse_params &p = a.p;
    assign_grid_csr(len, p.cols * p.rows, s_grid, a.grid_start, a.grid_items + off,             // (the items at the run's offset, as k_fuse_grids has them)
                    [&](int i) -> int { return pos_in_grid(x[i], y[i], p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows); });
}

__global__ __launch_bounds__(256) void k_fa_head(FuseMapArgs a, int t, int slot)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_list) return;
    int off, len;
    const bool target = fa_target(a, slot, off, len);
    const int r = a.list_row[i];
    bool pass = target && fa_row_ok(a, r) && a.st.bad[r] == 0;
    if (pass && a.sim3) pass = a.snap[r] != t + 1;                       // :992
    if (pass && !a.sim3) {                                               // IsInKeyFrame, :835
        int e = a.head[r];
        for (int hops = a.g.pool_entries; hops > 0 && (unsigned)e < (unsigned)a.g.pool_entries; hops--) {
            int s;
            if (fa_holds(a, e, r, s) && s == slot) { pass = false; break; }
            e = a.next[e];
        }
    }
    a.skip[i] = pass ? 0 : 1;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (pass) sl_load_desc(a.st.desc + 32 * (size_t)r, lo, hi);
    uint4 *d = reinterpret_cast<uint4 *>(a.gdesc + 32 * (size_t)i);
    d[0] = lo;
    d[1] = hi;
#pragma unroll
    for (int k = 0; k < 9; k++) a.gf[(size_t)k * a.n_list + i] = pass ? a.tab[k][r] : 0.0f;
}

// ---- k_fa_apply: one workgroup; every function below is called by all its threads with the same arguments ----
struct FaShared {
    int ent[FA_CHUNK];
    int n, cur, hops;                            // the walk: entries staged, where it continues, hops left
    int acc[2];
    int verdict[2];                              // thread 0's reading of the map for the point at hand (fa_decide)
    int cand[FA_THREADS], wave_n[FA_THREADS / 64];
};

// What steers the workgroup is read from the map by thread 0 ALONE and handed on through LDS between two barriers: thread 0 is also the one that
// writes point_pool, registered and bad, so no wave can see an entry before and another after such a write and take another branch.
template <class F> __device__ __forceinline__ void fa_decide(FaShared &sh, int &v0, int &v1, F read)
{
    if (threadIdx.x == 0) {
        int x = 0, y = 0;
        read(x, y);
        sh.verdict[0] = x; sh.verdict[1] = y;
    }
    __syncthreads();
    v0 = sh.verdict[0];
    v1 = sh.verdict[1];
    __syncthreads();                             // (read by everyone before thread 0 decides again or writes the map)
}

// f(e) for every entry of row's list, FA_CHUNK at a time: thread 0 follows the links (it has read an entry's link before f may rewrite it)
template <class F> __device__ __forceinline__ void fa_walk(const FuseMapArgs &a, FaShared &sh, int row, F f)
{
    const int pool = a.g.pool_entries;
    if (threadIdx.x == 0) { sh.cur = a.head[row]; sh.hops = pool; }
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) {
            int e = sh.cur, n = 0, hops = sh.hops;
            while (n < FA_CHUNK && hops > 0 && (unsigned)e < (unsigned)pool) { sh.ent[n++] = e; e = a.next[e]; hops--; }
            sh.n = n; sh.cur = e; sh.hops = hops;
        }
        __syncthreads();
        const int n = sh.n;
        for (int k = threadIdx.x; k < n; k += FA_THREADS) f(sh.ent[k]);
        if (n < FA_CHUNK) break;
    }
    __syncthreads();
}

// Observations(row) over the observations in slots with state 1, and whether one of them lies in `slot`
__device__ __forceinline__ int fa_observations(const FuseMapArgs &a, FaShared &sh, int row, int slot, bool &in_slot)
{
    if (threadIdx.x == 0) sh.acc[0] = sh.acc[1] = 0;
    fa_walk(a, sh, row, [&](int e) {
        int s;
        if (!fa_holds(a, e, row, s) || a.g.state[s] != 1) return;
        atomicAdd(&sh.acc[0], 1 + (a.kp.uright && a.kp.uright[e] >= 0.0f ? 1 : 0));
        if (s == slot) atomicOr(&sh.acc[1], 1);
    });
    const int n = sh.acc[0];
    in_slot = sh.acc[1] != 0;
    __syncthreads();
    return n;
}

struct FaTally { int fused, replaces, adds, bad_slot, turned, dropped, n_marked, stamp; };      // thread 0's

__device__ __forceinline__ void fa_log(const FuseMapArgs &a, int code, int x, int y, int z)       // thread 0
{
    const int at = a.stats[8]++;
    if (at < a.log_cap) {
        int32_t *o = a.log_out + 4 * (size_t)at;
        o[0] = code; o[1] = x; o[2] = y; o[3] = z;
    }
}

// MapPoint::Replace, p->Replace(q) (:208-246); p and q inside the table
__device__ __forceinline__ void fa_replace(const FuseMapArgs &a, FaShared &sh, FaTally &c, int t, int p, int q)
{
    if (p == q) return;
    if (threadIdx.x == 0) {
        sh.acc[0] = ++c.stamp;
        fa_log(a, 2, p, q, -1);
        c.replaces++;
    }
    __syncthreads();
    const int stamp = sh.acc[0];
    fa_walk(a, sh, q, [&](int e) {
        int s;
        if (fa_holds(a, e, q, s)) a.slot_mark[s] = stamp;
    });
    fa_walk(a, sh, p, [&](int e) {
        int s;
        if (!fa_holds(a, e, p, s)) return;
        if (a.slot_mark[s] == stamp) {           // q is in that keyframe: EraseMapPointMatch
            a.st.point_pool[e] = -1;
            a.st.registered[e] = 0;
        } else {                                 // ReplaceMapPointMatch, AddObservation
            a.st.point_pool[e] = q;
            a.next[e] = atomicExch(&a.head[q], e);
        }
    });
    if (threadIdx.x == 0) {
        a.head[p] = -1;
        if (a.st.bad[p] == 0) c.turned++;
        a.st.bad[p] = 1;
        if (a.st.replaced) a.st.replaced[p] = q;
        if (a.st.found) { a.st.found[q] += a.st.found[p]; a.st.visible[q] += a.st.visible[p]; }
        if (a.mark[q] != t + 1) {
            a.mark[q] = t + 1;
            if (c.n_marked < a.n_list) a.marked[c.n_marked++] = q;
        }
    }
    __syncthreads();
}

// the entries i of [base, base + 256) with v[i] >= 0, in order, into sh.cand; returns how many
__device__ __forceinline__ int fa_compact(const FuseMapArgs &a, FaShared &sh, const int32_t *v, int base)
{
    const int i = base + threadIdx.x, wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const bool c = i < a.n_list && v[i] >= 0;
    const unsigned long long m = __ballot(c);
    __syncthreads();                             // (the last round's candidates have been read)
    if (lane == 0) sh.wave_n[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < FA_THREADS / 64; w++) { if (w < wave) before += sh.wave_n[w]; total += sh.wave_n[w]; }
    if (c) sh.cand[before + __popcll(m & ((1ull << lane) - 1))] = i;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(FA_THREADS) void k_fa_apply(FuseMapArgs a, int t, int slot)
{
    __shared__ FaShared sh;
    int off, len;
    const bool target = fa_target(a, slot, off, len);
    const int32_t *bi = a.best_idx + (size_t)t * a.n_list;
    int32_t *rp = a.replace_point ? a.replace_point + (size_t)t * a.n_list : nullptr;
    if (rp) for (int i = threadIdx.x; i < a.n_list; i += FA_THREADS) rp[i] = -1;
    if (!target) {                               // step 0
        if (threadIdx.x == 0) { a.n_fused[t] = 0; a.stats[6]++; a.ctl[1] = 0; }
        return;
    }
    FaTally c{};
    c.stamp = a.ctl[0];
    for (int base = 0; base < a.n_list; base += FA_THREADS) {          // step 3
        const int nc = fa_compact(a, sh, bi, base);
        for (int k = 0; k < nc; k++) {
            const int i = sh.cand[k], r = a.list_row[i], b = bi[i];  // (list_row and best_idx are written by nobody here)
            int head, unused_v;
            fa_decide(sh, head, unused_v, [&](int &x, int &) {       // the head test, live: :833-834, :992
                x = fa_row_ok(a, r) && a.st.bad[r] == 0 && !(a.sim3 && a.snap[r] == t + 1);
            });
            if (!head) continue;
            int obs_r = 0;
            if (!a.sim3) {                       // IsInKeyFrame, :835; Observations() for the tail
                bool in_kf;
                obs_r = fa_observations(a, sh, r, slot, in_kf);
                if (in_kf) continue;
            }
            c.fused++;
            const int e = off + b;
            enum { DROP, ADD, BAD_SLOT, HAND_BACK, COMPARE };
            int what, q;
            fa_decide(sh, what, q, [&](int &x, int &y) {
                y = b < len ? a.st.point_pool[e] : -2;
                x = y < -1 || y >= a.n_rows ? DROP : y == -1 ? ADD : a.st.bad[y] != 0 ? BAD_SLOT : a.sim3 ? HAND_BACK : COMPARE;
            });
            if (what == DROP) {
                c.dropped++;
            } else if (what == ADD) {            // AddObservation, AddMapPoint
                if (threadIdx.x == 0) {
                    a.st.point_pool[e] = r;
                    a.st.registered[e] = 1;
                    a.ent_slot[e] = slot;
                    a.next[e] = a.head[r];
                    a.head[r] = e;
                    fa_log(a, 3, r, slot, b);
                    c.adds++;
                }
                __syncthreads();
            } else if (what == BAD_SLOT) {
                c.bad_slot++;
            } else if (what == HAND_BACK) {
                if (threadIdx.x == 0) rp[i] = q;
            } else {
                bool unused;
                const int obs_q = fa_observations(a, sh, q, slot, unused);
                if (obs_q > obs_r) fa_replace(a, sh, c, t, r, q); else fa_replace(a, sh, c, t, q, r);
            }
        }
    }
    if (a.sim3 && a.replace_loop && rp) {        // step 4
        __syncthreads();
        for (int base = 0; base < a.n_list; base += FA_THREADS) {
            const int nc = fa_compact(a, sh, rp, base);
            for (int k = 0; k < nc; k++) {
                const int i = sh.cand[k], p = rp[i], q = a.list_row[i];      // (replace_point is complete behind the barrier above and not written again)
                if (fa_row_ok(a, p) && fa_row_ok(a, q)) fa_replace(a, sh, c, t, p, q);
            }
        }
    }
    if (threadIdx.x == 0) {
        a.n_fused[t] = c.fused;
        a.stats[0] += c.fused; a.stats[1] += c.replaces; a.stats[2] += c.adds; a.stats[3] += c.bad_slot; a.stats[4] += c.turned;
        a.stats[7] += c.dropped;
        a.ctl[0] = c.stamp;
        a.ctl[1] = c.n_marked;
    }
}

// f(e, slot) for the observations of `row` in slots with state 1, by one thread
template <class F> __device__ __forceinline__ void fa_each_observation(const FuseMapArgs &a, int row, F f)
{
    int e = a.head[row];
    for (int hops = a.g.pool_entries; hops > 0 && (unsigned)e < (unsigned)a.g.pool_entries; hops--) {
        int s;
        if (fa_holds(a, e, row, s) && a.g.state[s] == 1) f(e, s);
        e = a.next[e];
    }
}

__global__ __launch_bounds__(256) void k_fa_csr(FuseMapArgs a)
{
    __shared__ int s_scan[256];
    if (threadIdx.x == 0) a.stats[5] += a.ds[6];                      // the last target's descriptors written with other bytes
    __syncthreads();
    if (threadIdx.x < 8) a.ds[threadIdx.x] = 0;
    const int n_marked = min(max(a.ctl[1], 0), a.n_list), pool = a.g.pool_entries;
    int carry = 0;
    for (int base = 0; base < a.n_list; base += 256) {
        const int j = base + threadIdx.x;
        int n = 0, row = 0;
        if (j < n_marked) {
            row = a.marked[j];
            if (fa_row_ok(a, row) && a.st.bad[row] == 0) fa_each_observation(a, row, [&](int, int) { n++; });
            else row = fa_row_ok(a, row) ? row : 0;
        }
        if (j < a.n_list) a.out_row[j] = row;
        s_scan[threadIdx.x] = n;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0;
            __syncthreads();
            s_scan[threadIdx.x] += v;
            __syncthreads();
        }
        const int start = carry + s_scan[threadIdx.x] - n;
        carry += s_scan[255];
        if (j < a.n_list) a.obs_start[j] = min(start, pool);
        if (n > 0 && (long long)start + n <= pool) {
            int k = 0;
            fa_each_observation(a, row, [&](int e, int s) {          // placed in (order_key, slot) order: the lists are short
                if (k >= n) return;
                const long long key = a.g.order_key[s];
                int at = start + k;
                while (at > start) {
                    const int o = a.csr_ent[at - 1], os = a.ent_slot[o];
                    if (!fa_key_less(key, s, a.g.order_key[os], os)) break;
                    a.csr_ent[at] = o;
                    at--;
                }
                a.csr_ent[at] = e;
                k++;
            });
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.obs_start[a.n_list] = min(carry, pool);
}

__global__ void k_fa_finish(FuseMapArgs a)
{
    if (threadIdx.x != 0) return;
    a.stats[5] += a.ds[6];
    a.ds[6] = 0;
    a.stats[9] = a.stats[8] > a.log_cap ? 1 : 0;
    for (int i = 0; i < FM_COUNTS; i++) a.counts_dev[i] = a.stats[i];
}

int fuse_map_list_chunk() { return FA_CHUNK; }

void launch_fuse_map_index(const FuseMapArgs &a, hipStream_t s)
{
    if (a.g.max_keyframes <= 0 || a.g.pool_entries <= 0) return;
    hipLaunchKernelGGL(k_fa_index, dim3(std::min(a.g.max_keyframes, 1024)), dim3(256), 0, s, a);
}

void launch_fuse_map_head(const FuseMapArgs &a, int t, int slot, hipStream_t s)
{
    if (a.n_list <= 0) return;
    const int pool = a.g.pool_entries;
    if (a.sim3 && pool > 0) hipLaunchKernelGGL(k_fa_snapshot, dim3((std::min(pool, 1 << 18) + 255) / 256), dim3(256), 0, s, a, t, slot);
    const size_t lds = (size_t)(2 * a.p.cols * a.p.rows + 1024) * sizeof(int);
    hipLaunchKernelGGL(k_fa_grid, dim3(1), dim3(1024), lds, s, a, slot);
    hipLaunchKernelGGL(k_fa_head, dim3((a.n_list + 255) / 256), dim3(256), 0, s, a, t, slot);
}

void launch_fuse_map_apply(const FuseMapArgs &a, int t, int slot, hipStream_t s)
{
    hipLaunchKernelGGL(k_fa_apply, dim3(1), dim3(FA_THREADS), 0, s, a, t, slot);
    if (a.n_list > 0) hipLaunchKernelGGL(k_fa_csr, dim3(1), dim3(256), 0, s, a);
}

void launch_fuse_map_finish(const FuseMapArgs &a, hipStream_t s) { hipLaunchKernelGGL(k_fa_finish, dim3(1), dim3(64), 0, s, a); }

} // namespace jsorb
