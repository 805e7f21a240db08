// jsorb_fuse_apply.hip - host side of Fuse applied to the map on the device: jsorb_fuse_map* (ORBmatcher::Fuse with MapPoint::Replace /
// AddObservation and the Replace loop of LoopClosing::SearchAndFuse, all target keyframes of a call in the reference's order).  It runs on a keyframe
// matcher (its stream; scratch of its own in struct fmap, jsorb_handle.h).  The kernels are in k_fuse_apply.hip, k_fuse.hip (k_fuse_match_run) and
// k_distinct.hip.  The state (the graph, the table, the keypoints) is the caller's.
#include "jsorb_handle.h"

namespace {

const char *const FM = "fuse_map";

// the pieces of the scratch that are not k_fuse_apply's own: the spans the call clears and what k_fuse_match_run and k_distinct write
struct FuseMapScratch {
    int32_t *minus, *zero, *rest;                // [minus, zero) is cleared to -1, [zero, rest) to 0
    int32_t *search_stats, *n_matched;           // k_fuse_match_run's counts per target: cleared with the rest, read by nobody (n_fused is the call's count)
    int32_t *best_obs, *best_median, *dlist;
};

// The scratch of one call in 32-bit words, placed into a and s: the list points' descriptors first (16-byte aligned), the words cleared to -1,
// those cleared to 0, the rest.  Returns the words it takes (base NULL: only that).
long long fuse_map_layout(FuseMapArgs &a, FuseMapScratch &s, int32_t *base, long long rows, long long slots, long long ents, long long nl, long long cells)
{
    Carve c(base);
    a.gdesc = (uint8_t *)c.take(8 * nl);
    s.minus = a.head = c.take(rows); a.ent_slot = c.take(ents);
    s.zero = a.mark = c.take(rows); a.snap = c.take(rows); a.slot_mark = c.take(slots); a.ctl = c.take(8); a.ds = c.take(8);
    s.search_stats = c.take(16); s.n_matched = c.take(JSORB_BOW_MAX_KEYFRAMES);
    s.rest = a.next = c.take(ents); a.csr_ent = c.take(ents); a.grid_items = c.take(ents); a.grid_start = c.take(cells);
    a.gf = (float *)c.take(9 * nl); a.skip = (uint8_t *)c.take((nl + 3) / 4);
    a.marked = c.take(nl); a.obs_start = c.take(nl + 1); a.out_row = c.take(nl);
    s.best_obs = c.take(nl); s.best_median = c.take(nl); s.dlist = c.take(3 * nl);
    return c.at;
}

} // namespace

extern "C" {

int jsorb_fuse_map_async(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int replace_loop, const jsorb_keyframe_graph *graph,
                         const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_fuse_state *state, int n_list,
                         const int32_t *list_row, int n_targets, const int32_t *target_slot, const float *Rcw, const float *tcw, const float *Ow,
                         int32_t *best_idx, int32_t *best_dist, int32_t *replace_point, int32_t *n_fused, int log_cap, int32_t *log_out,
                         int32_t *counts_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!params || !graph || !table || !kp || !state || !counts_dev) return kf_fail(m, FM, "NULL params, graph, table, kp, state or counts_dev");
    if (params->n_levels < 1 || params->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, FM, "n_levels out of range");
    if (params->th_low < 0 || params->th_low > 255) return kf_fail(m, FM, "th_low must be in [0, 255]");
    if (params->cols < 1 || params->rows < 1 || (long long)params->cols * params->rows > FUSE_MAX_CELLS) return kf_fail(m, FM, "grid size out of range (cols*rows <= 4096)");
    const jsorb_keyframe_graph &g = *graph;
    const int S = g.max_keyframes, pool = g.pool_entries, n_rows = table->n_rows, sim3 = params->check_reprojection ? 0 : 1;
    if (S < 0 || pool < 0 || n_rows < 0 || n_list < 0 || log_cap < 0) return kf_fail(m, FM, "max_keyframes, pool_entries, n_rows, n_list and log_cap must not be negative");
    if (n_targets < 0 || n_targets > JSORB_BOW_MAX_KEYFRAMES) return kf_fail(m, FM, "n_targets must be in [0, 256]");
    if (log_cap >= (1 << 27)) return kf_fail(m, FM, "log_cap too large");
    if (kp->pool_entries != pool) return kf_fail(m, FM, "the keypoints and the graph differ in pool_entries");
    if ((long long)n_targets * n_list > (long long)INT_MAX - JSORB_BOW_MAX_KEYFRAMES) return kf_fail(m, FM, "n_targets x n_list too large", JSORB_ERR_UNSUPPORTED);
    if (S > 0 && (!g.state || !g.order_key || !g.point_off || !g.point_len || (pool > 0 && !g.point_pool))) return kf_fail(m, FM, "NULL graph array");
    if (pool > 0 && !g.registered) return kf_fail(m, FM, "graph->registered is NULL: the call writes those bytes");
    if (pool > 0 && (!kp->x || !kp->y || !kp->octave || !kp->desc)) return kf_fail(m, FM, "NULL keypoint array");
    if (n_rows > 0 && (!table->Px || !table->Py || !table->Pz || !table->Pnx || !table->Pny || !table->Pnz || !table->MaxDistance ||
                       !table->invariance_maxDistance || !table->invariance_minDistance || !table->desc || !table->bad))
        return kf_fail(m, FM, "NULL table array");
    if ((uintptr_t)kp->desc % 16 || (uintptr_t)table->desc % 16) return kf_fail(m, FM, "descriptors must be 16-byte aligned");
    if (state->point_pool != g.point_pool || state->registered != g.registered || state->bad != table->bad || state->desc != table->desc)
        return kf_fail(m, FM, "a fuse_state array is not the graph's or the table's");
    if (!state->visible != !state->found) return kf_fail(m, FM, "visible and found: both NULL or both given");
    if (n_list > 0 && !list_row) return kf_fail(m, FM, "NULL list_row");
    if (n_targets > 0 && (!target_slot || !Rcw || !tcw || !Ow || !n_fused)) return kf_fail(m, FM, "NULL target_slot, Rcw, tcw, Ow or n_fused");
    if (n_targets > 0 && n_list > 0 && (!best_idx || !best_dist)) return kf_fail(m, FM, "NULL best_idx or best_dist");
    if (n_targets > 0 && n_list > 0 && sim3 && !replace_point) return kf_fail(m, FM, "the overload with Scw needs replace_point");
    if (log_cap > 0 && !log_out) return kf_fail(m, FM, "NULL log_out");
    HIPCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    KfCall &c = m->call[jsorb_keyframe_matcher::FUSE_MAP];
    RCCHK(reserve_device(m, c.stats, 16 * sizeof(int)));
    const long long rows = std::max(n_rows, 1), slots = std::max(S, 1), ents = std::max(pool, 1), nl = std::max(n_list, 1), cells = (long long)params->cols * params->rows + 1;
    FuseMapArgs a{};
    FuseMapScratch s{};
    RCCHK(reserve_words(m, m->fmap, fuse_map_layout(a, s, nullptr, rows, slots, ents, nl, cells)));
    fuse_map_layout(a, s, m->fmap.p, rows, slots, ents, nl, cells);
    a.g = g; a.kp = *kp; a.st = *state; a.p = *params; a.n_rows = n_rows;
    const float *const tab[9] = {table->Px, table->Py, table->Pz, table->Pnx, table->Pny, table->Pnz, table->MaxDistance, table->invariance_minDistance,
                                 table->invariance_maxDistance};
    memcpy(a.tab, tab, sizeof(tab));
    a.n_list = n_list; a.n_targets = n_targets; a.sim3 = sim3; a.replace_loop = replace_loop != 0; a.log_cap = log_cap; a.list_row = list_row;
    a.best_idx = best_idx; a.replace_point = replace_point; a.n_fused = n_fused; a.log_out = log_out; a.counts_dev = counts_dev; a.stats = c.stats;
    HIPCHK(m, hipMemsetAsync(c.stats, 0, 16 * sizeof(int), st));
    c.done = true;
    HIPCHK(m, hipMemsetAsync(s.minus, 0xFF, (size_t)(s.zero - s.minus) * sizeof(int32_t), st));
    HIPCHK(m, hipMemsetAsync(s.zero, 0, (size_t)(s.rest - s.zero) * sizeof(int32_t), st));
    if (log_cap > 0) HIPCHK(m, hipMemsetAsync(log_out, 0xFF, (size_t)log_cap * 4 * sizeof(int32_t), st));
    if (n_targets > 0) {
        launch_fuse_map_index(a, st);
        HIPCHK(m, hipGetLastError());
    }
    FuseArgs f{};
    f.p = *params; f.n_points = n_list;
    float *const plane[9] = {a.gf, a.gf + (size_t)n_list, a.gf + 2 * (size_t)n_list, a.gf + 3 * (size_t)n_list, a.gf + 4 * (size_t)n_list, a.gf + 5 * (size_t)n_list,
                             a.gf + 6 * (size_t)n_list, a.gf + 7 * (size_t)n_list, a.gf + 8 * (size_t)n_list};
    f.Px = plane[0]; f.Py = plane[1]; f.Pz = plane[2]; f.Nx = plane[3]; f.Ny = plane[4]; f.Nz = plane[5];
    f.max_distance = plane[6]; f.min_dist_inv = plane[7]; f.max_dist_inv = plane[8];
    f.mp_desc = a.gdesc;
    f.x = kp->x; f.y = kp->y; f.uright = kp->uright; f.octave = kp->octave; f.kf_desc = kp->desc;
    f.skip = a.skip; f.cell_start = a.grid_start; f.cell_items = a.grid_items;
    f.best_idx = best_idx; f.best_dist = best_dist; f.n_matched = s.n_matched; f.stats = s.search_stats;
    DistinctArgs d{};
    d.n_points = n_list; d.n_obs = pool; d.n_rows = pool; d.n_out_rows = n_rows;
    d.obs_start = a.obs_start; d.obs_row = a.csr_ent; d.kf_desc = kp->desc; d.out_row = a.out_row;
    d.list = s.dlist; d.best_obs = s.best_obs; d.best_median = s.best_median; d.desc_out = state->desc; d.changed = nullptr; d.stats = a.ds;
    for (int t = 0; t < n_targets; t++) {
        const int slot = target_slot[t];
        launch_fuse_map_head(a, t, slot, st);
        HIPCHK(m, hipGetLastError());
        FuseRun r{};
        r.row = t; r.slot = slot; r.n_slots = S; r.pool_entries = pool; r.state = g.state; r.point_off = g.point_off; r.point_len = g.point_len;
        memcpy(r.pose, Rcw + 9 * (size_t)t, 9 * sizeof(float));
        memcpy(r.pose + 9, tcw + 3 * (size_t)t, 3 * sizeof(float));
        memcpy(r.pose + 12, Ow + 3 * (size_t)t, 3 * sizeof(float));
        launch_fuse_match_run(f, r, st);
        HIPCHK(m, hipGetLastError());
        launch_fuse_map_apply(a, t, slot, st);
        HIPCHK(m, hipGetLastError());
        if (n_list > 0 && pool > 0 && n_rows > 0) {
            launch_distinct(d, st);
            HIPCHK(m, hipGetLastError());
        }
    }
    launch_fuse_map_finish(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_fuse_map(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int replace_loop, const jsorb_keyframe_graph *graph,
                   const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_fuse_state *state, int n_list,
                   const int32_t *list_row, int n_targets, const int32_t *target_slot, const float *Rcw, const float *tcw, const float *Ow,
                   int32_t *best_idx, int32_t *best_dist, int32_t *replace_point, int32_t *n_fused, int log_cap, int32_t *log_out, int32_t *counts_dev,
                   int32_t *best_idx_host, int32_t *best_dist_host, int32_t *replace_point_host, int32_t *n_fused_host, int32_t *log_host,
                   int32_t counts_host[10])
{
    if (!m) return JSORB_ERR_INVALID;
    if (n_targets < 0 || n_list < 0 || log_cap < 0) return kf_fail(m, FM, "n_targets, n_list and log_cap must not be negative");
    const size_t pairs = (size_t)n_targets * n_list, nt = (size_t)n_targets, nlog = (size_t)log_cap * 4;
    if (!counts_host || (nt && !n_fused_host) || (pairs && (!best_idx_host || !best_dist_host || (replace_point && !replace_point_host))) || (nlog && !log_host))
        return kf_fail(m, FM, "NULL host output");
    RCCHK(jsorb_fuse_map_async(m, params, replace_loop, graph, table, kp, state, n_list, list_row, n_targets, target_slot, Rcw, tcw, Ow, best_idx, best_dist,
                               replace_point, n_fused, log_cap, log_out, counts_dev));
    const int32_t *const src[6] = {counts_dev, n_fused, best_idx, best_dist, replace_point, log_out};
    int32_t *const dst[6] = {counts_host, n_fused_host, best_idx_host, best_dist_host, replace_point_host, log_host};
    const size_t n[6] = {FM_COUNTS, nt, pairs, pairs, replace_point ? pairs : 0, nlog};
    return read_back(m, m->stream, m->staging, 6, src, dst, n);
}

int jsorb_fuse_map_stats(jsorb_keyframe_matcher *m, int32_t counts[10])
{
    if (!m) return JSORB_ERR_INVALID;
    if (!counts) return kf_fail(m, FM, "NULL counts");
    return read_stats(m, m->call[jsorb_keyframe_matcher::FUSE_MAP].done, "fuse_map_stats before jsorb_fuse_map", m->call[jsorb_keyframe_matcher::FUSE_MAP].stats,
                      counts, FM_COUNTS);
}

int jsorb_fuse_map_build_caps(int *list_chunk)
{
    if (list_chunk) *list_chunk = fuse_map_list_chunk();
    return JSORB_OK;
}

} // extern "C"
