// jsorb_culling.hip - host side of the keyframe culling kept on the device: jsorb_cull_keyframes* (LocalMapping::KeyFrameCulling with
// KeyFrame::SetBadFlag and MapPoint::EraseObservation / SetBadFlag for up to 16 culled keyframes in a row).  It runs on a keyframe matcher (its
// stream; scratch of its own in struct cull, jsorb_handle.h).  The kernels are in k_kf_culling.hip and k_covisibility.hip (k_cv_erase_dev).  The
// state (the graph, the table, the covisibility arrays, the views) is the caller's.
#include "jsorb_handle.h"

namespace {

const char *const CK = "cull_keyframes";

// The scratch of one call in 32-bit words, placed into a: the order and the sizes of the pieces.  Returns the words it takes (base NULL: only that).
long long cull_layout(CullArgs &a, int32_t *base, long long rows, long long pool, long long slots, long long cands)
{
    Carve c(base);
    a.cnt = c.take(rows); a.fill = c.take(rows); a.off = c.take(rows); a.bsum = c.take((rows + KC_SCAN - 1) / KC_SCAN);
    a.csr_slot = c.take(pool); a.csr_ent = c.take(pool); a.was_obs = c.take(pool);
    a.pmark = c.take(slots); a.ch_raw = c.take(slots); a.ch = c.take(slots); a.ch_done = c.take(slots);
    a.ev = c.take(3 * cands); a.ctl = c.take(8); a.erase_counts = c.take(2);
    return c.at;
}

} // namespace

extern "C" {

int jsorb_cull_keyframes_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                               const jsorb_covisibility *cov, const jsorb_keyframe_views *views, const jsorb_culling_state *state, int monocular,
                               int first_slot, int n_cand, const int32_t *cand_slot, int max_cull, int32_t *neighbours, int reparent_cap,
                               int32_t *decision, int32_t *n_mps, int32_t *n_redundant, int32_t *culled_slot, int32_t *reparent_out,
                               int32_t *counts_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!graph || !table || !cov || !views || !state || !counts_dev) return kf_fail(m, CK, "NULL graph, table, cov, views, state or counts_dev");
    const jsorb_keyframe_graph &g = *graph;
    const int S = g.max_keyframes;
    if (S < 0 || g.pool_entries < 0 || table->n_rows < 0) return kf_fail(m, CK, "max_keyframes, pool_entries and n_rows must not be negative");
    if (S >= (1 << 24)) return kf_fail(m, CK, "more than 16777215 keyframe slots");
    if (S != cov->max_keyframes) return kf_fail(m, CK, "the graph and the covisibility state differ in max_keyframes");
    RCCHK(check_conn_capacity(m, CK, cov->conn_capacity));
    if (S > 0 && (!cov->conn_len || !cov->conn_slot || !cov->conn_weight || !cov->ord_len || !cov->ord_slot || !cov->ord_weight))
        return kf_fail(m, CK, "NULL covisibility array");
    if (max_cull < 1 || max_cull > KC_MAX_CULL) return kf_fail(m, CK, "max_cull must be in [1, 16]");
    if (n_cand < 0 || n_cand > KC_MAX_CAND) return kf_fail(m, CK, "n_cand must be in [0, " + std::to_string((int)KC_MAX_CAND) + "]");
    if (n_cand > 0 && (!cand_slot || !decision || !n_mps || !n_redundant)) return kf_fail(m, CK, "NULL cand_slot, decision, n_mps or n_redundant");
    if (!culled_slot) return kf_fail(m, CK, "NULL culled_slot");
    if (reparent_cap < 0 || reparent_cap >= (1 << 24) || (reparent_cap > 0 && !reparent_out)) return kf_fail(m, CK, "reparent_cap negative or too large, or NULL reparent_out");
    if (first_slot < -1 || first_slot >= S) return kf_fail(m, CK, "first_slot outside [-1, max_keyframes)");
    if (S > 0 && (!g.state || !g.order_key || !g.point_off || !g.point_len || !g.parent || (g.pool_entries > 0 && !g.point_pool))) return kf_fail(m, CK, "NULL graph array");
    if (g.pool_entries > 0 && !g.registered) return kf_fail(m, CK, "graph->registered is NULL: the call writes those bytes");
    if (table->n_rows > 0 && !table->bad) return kf_fail(m, CK, "NULL table array");
    if (views->pool_entries != g.pool_entries) return kf_fail(m, CK, "the views and the graph differ in pool_entries");
    if (g.pool_entries > 0 && (!views->octave || !views->stereo)) return kf_fail(m, CK, "NULL views array");
    if (!monocular && ((g.pool_entries > 0 && !views->depth) || (S > 0 && !views->th_depth))) return kf_fail(m, CK, "monocular is 0 and depth or th_depth is NULL");
    if (state->state != g.state || state->registered != g.registered || state->point_pool != g.point_pool || state->parent != g.parent ||
        state->bad != table->bad)
        return kf_fail(m, CK, "a culling_state array is not the graph's or the table's");
    if (state->not_erase && !state->to_be_erased) return kf_fail(m, CK, "not_erase without to_be_erased");
    HIPCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    KfCall &c = m->call[jsorb_keyframe_matcher::CULL];
    RCCHK(reserve_device(m, c.stats, 16 * sizeof(int)));
    const long long rows = std::max(table->n_rows, 1), slots = std::max(S, 1), pool = std::max(g.pool_entries, 1), cands = std::max(n_cand, 1);
    CullArgs a{};
    RCCHK(reserve_words(m, m->cull, cull_layout(a, nullptr, rows, pool, slots, cands)));
    cull_layout(a, m->cull.p, rows, pool, slots, cands);
    a.g = g; a.cv = *cov; a.v = *views; a.st = *state;
    a.n_rows = table->n_rows; a.monocular = monocular != 0; a.first_slot = first_slot; a.n_cand = n_cand; a.max_cull = max_cull; a.reparent_cap = reparent_cap;
    a.cand_slot = cand_slot; a.neighbours = neighbours;
    a.decision = decision; a.n_mps = n_mps; a.n_redundant = n_redundant; a.culled_slot = culled_slot; a.reparent_out = reparent_out; a.counts = counts_dev;
    a.stats = c.stats;
    launch_cull_keyframes(a, st);
    HIPCHK(m, hipGetLastError());
    c.done = true;
    return JSORB_OK;
}

int jsorb_cull_keyframes(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                         const jsorb_covisibility *cov, const jsorb_keyframe_views *views, const jsorb_culling_state *state, int monocular,
                         int first_slot, int n_cand, const int32_t *cand_slot, int max_cull, int32_t *neighbours, int reparent_cap, int32_t *decision,
                         int32_t *n_mps, int32_t *n_redundant, int32_t *culled_slot, int32_t *reparent_out, int32_t *counts_dev,
                         int32_t *decision_host, int32_t *n_mps_host, int32_t *n_redundant_host, int32_t *culled_slot_host, int32_t *reparent_host,
                         int32_t counts_host[10])
{
    if (!m) return JSORB_ERR_INVALID;
    if (!counts_host || !culled_slot_host || (n_cand > 0 && (!decision_host || !n_mps_host || !n_redundant_host)) || (reparent_cap > 0 && !reparent_host))
        return kf_fail(m, CK, "NULL host output");
    RCCHK(jsorb_cull_keyframes_async(m, graph, table, cov, views, state, monocular, first_slot, n_cand, cand_slot, max_cull, neighbours, reparent_cap,
                                     decision, n_mps, n_redundant, culled_slot, reparent_out, counts_dev));
    const size_t nc = (size_t)n_cand, nr = (size_t)reparent_cap * 2;
    const int32_t *const src[6] = {counts_dev, culled_slot, decision, n_mps, n_redundant, reparent_out};
    int32_t *const dst[6] = {counts_host, culled_slot_host, decision_host, n_mps_host, n_redundant_host, reparent_host};
    const size_t n[6] = {KC_COUNTS, (size_t)max_cull, nc, nc, nc, nr};
    return read_back(m, m->stream, m->staging, 6, src, dst, n);
}

int jsorb_cull_keyframes_stats(jsorb_keyframe_matcher *m, int32_t counts[10])
{
    if (!m) return JSORB_ERR_INVALID;
    if (!counts) return kf_fail(m, CK, "NULL counts");
    return read_stats(m, m->call[jsorb_keyframe_matcher::CULL].done, "cull_keyframes_stats before jsorb_cull_keyframes", m->call[jsorb_keyframe_matcher::CULL].stats,
                      counts, KC_COUNTS);
}

int jsorb_cull_keyframes_build_caps(int *max_candidates, int *max_cull)
{
    if (max_candidates) *max_candidates = KC_MAX_CAND;
    if (max_cull) *max_cull = KC_MAX_CULL;
    return JSORB_OK;
}

} // extern "C"
