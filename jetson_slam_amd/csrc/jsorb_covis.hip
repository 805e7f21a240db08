// jsorb_covis.hip - host side of the covisibility graph kept on the device: jsorb_update_connections* (KeyFrame::UpdateConnections for up to 32
// keyframes in a row), jsorb_erase_connections_async (SetBadFlag's EraseConnection walk), jsorb_connected_mask_async, jsorb_best_covisibles_async,
// jsorb_covisibility_copy.  They run on a keyframe matcher (its stream; scratch of its own in struct covis, jsorb_handle.h).  The kernels are in
// k_covisibility.hip.  The state (jsorb_covisibility) is the caller's, like the keyframe graph.
#include "jsorb_handle.h"

namespace {

const char *const UC = "update_connections", *const EC = "erase_connections", *const CM = "connected_mask", *const BC = "best_covisibles";

int covis_check(jsorb_keyframe_matcher *m, const char *name, const jsorb_covisibility *cov)
{
    if (!cov) return kf_fail(m, name, "NULL cov");
    if (cov->max_keyframes < 0) return kf_fail(m, name, "max_keyframes must not be negative");
    if (cov->max_keyframes >= (1 << 24)) return kf_fail(m, name, "more than 16777215 keyframe slots");
    RCCHK(check_conn_capacity(m, name, cov->conn_capacity));
    if (cov->max_keyframes > 0 && (!cov->conn_len || !cov->conn_slot || !cov->conn_weight || !cov->ord_len || !cov->ord_slot || !cov->ord_weight ||
                                   !cov->first_connection))
        return kf_fail(m, name, "NULL covisibility array");
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_update_connections_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                                   const jsorb_covisibility *cov, int n_update, const int32_t *update_slot, int32_t *neighbours, int32_t *parent_out,
                                   const jsorb_conn_snapshot *conn_snapshot, int32_t *counts_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!graph || !table || !counts_dev) return kf_fail(m, UC, "NULL graph, table or counts_dev");
    RCCHK(covis_check(m, UC, cov));
    const jsorb_keyframe_graph &g = *graph;
    const int S = g.max_keyframes;
    if (S != cov->max_keyframes) return kf_fail(m, UC, "the graph and the covisibility state differ in max_keyframes");
    if (g.pool_entries < 0 || table->n_rows < 0) return kf_fail(m, UC, "pool_entries and n_rows must not be negative");
    if (n_update < 0 || n_update > CV_MAX_UPDATE) return kf_fail(m, UC, "n_update must be in [0, 32]");
    if (n_update > 0 && !update_slot) return kf_fail(m, UC, "NULL update_slot");
    if (S > 0 && (!g.state || !g.order_key || !g.point_off || !g.point_len || (g.pool_entries > 0 && !g.point_pool))) return kf_fail(m, UC, "NULL graph array");
    if (table->n_rows > 0 && !table->bad) return kf_fail(m, UC, "NULL table array");
    if (conn_snapshot && (!conn_snapshot->slot || !conn_snapshot->weight || !conn_snapshot->len)) return kf_fail(m, UC, "NULL snapshot array");
    HIPCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    KfCall &c = m->call[jsorb_keyframe_matcher::COVIS];
    RCCHK(reserve_device(m, c.stats, KF_STATS * sizeof(int)));
    const int slots = std::max(S, 1);
    RCCHK(reserve_row_words(m, m->covis.row, table->n_rows, 0, st));      // the scratch: grown only; a word is zero between calls
    RCCHK(reserve_device(m, m->covis.slot, ((size_t)4 * CV_MAX_UPDATE * slots + 4 * CV_MAX_UPDATE) * sizeof(int32_t), &m->covis.slots, slots));
    CovisArgs a{};
    a.g = g; a.cv = *cov;
    a.n_rows = table->n_rows; a.bad = table->bad;
    a.n_update = n_update; a.update_slot = update_slot;
    a.neighbours = neighbours; a.parent_out = parent_out;
    if (conn_snapshot) { a.snap_slot = conn_snapshot->slot; a.snap_weight = conn_snapshot->weight; a.snap_len = conn_snapshot->len; }
    a.counts = counts_dev;
    const size_t plane = (size_t)CV_MAX_UPDATE * m->covis.slots;
    a.word = m->covis.row.word;
    a.count = m->covis.slot; a.kraw = a.count + plane; a.klist = a.kraw + plane; a.tlist = a.klist + plane; a.minfo = a.tlist + plane;
    // the planes are laid out for the slots reserved, and indexed by S <= that
    a.stats = c.stats;
    m->covis.row.dirty = true;         // until all five kernels are enqueued: k_cv_reset is the one that sets the words back
    launch_update_connections(a, st);
    HIPCHK(m, hipGetLastError());
    m->covis.row.dirty = false;
    c.done = true;
    return JSORB_OK;
}

int jsorb_update_connections(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                             const jsorb_covisibility *cov, int n_update, const int32_t *update_slot, int32_t *neighbours, int32_t *parent_out,
                             const jsorb_conn_snapshot *conn_snapshot, int32_t *counts_dev, int32_t *parent_host, int32_t counts_host[8])
{
    if (!m) return JSORB_ERR_INVALID;
    if (!counts_host || (parent_out && n_update > 0 && !parent_host)) return kf_fail(m, UC, "NULL host output");
    RCCHK(jsorb_update_connections_async(m, graph, table, cov, n_update, update_slot, neighbours, parent_out, conn_snapshot, counts_dev));
    const int32_t *const src[2] = {counts_dev, parent_out};
    int32_t *const dst[2] = {counts_host, parent_host};
    const size_t n[2] = {8, parent_out ? (size_t)n_update : 0};
    return read_back(m, m->stream, m->staging, 2, src, dst, n);
}

int jsorb_update_connections_stats(jsorb_keyframe_matcher *m, int *n_processed, int *n_skipped, int *n_empty, int *n_add_connection, int *n_resorted,
                                   int *n_fallback, int *n_overflow)
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::COVIS], "update_connections_stats before jsorb_update_connections", s));
    int *const out[7] = {n_processed, n_skipped, n_empty, n_add_connection, n_resorted, n_fallback, n_overflow};
    for (int i = 0; i < 7; i++)
        if (out[i]) *out[i] = s[i];
    return JSORB_OK;
}

int jsorb_update_connections_scratch(jsorb_keyframe_matcher *m, int *n_words, int *n_nonzero)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!m->call[jsorb_keyframe_matcher::COVIS].done) return kf_fail(m, UC, "update_connections_scratch before jsorb_update_connections", JSORB_ERR_STATE);
    HIPCHK(m, hipSetDevice(m->device));
    std::vector<uint32_t> h((size_t)m->covis.row.rows);
    HIPCHK(m, hipMemcpyAsync(h.data(), m->covis.row.word, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (n_words) *n_words = m->covis.row.rows;
    if (n_nonzero) *n_nonzero = (int)std::count_if(h.begin(), h.end(), [](uint32_t w) { return w != 0; });
    return JSORB_OK;
}

int jsorb_erase_connections_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_covisibility *cov, int slot,
                                  int32_t *neighbours, int32_t *counts_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!graph || !counts_dev) return kf_fail(m, EC, "NULL graph or counts_dev");
    RCCHK(covis_check(m, EC, cov));
    if (graph->max_keyframes != cov->max_keyframes) return kf_fail(m, EC, "the graph and the covisibility state differ in max_keyframes");
    if (slot < 0 || slot >= cov->max_keyframes) return kf_fail(m, EC, "slot outside [0, max_keyframes)");
    if (!graph->order_key) return kf_fail(m, EC, "NULL graph array");
    HIPCHK(m, hipSetDevice(m->device));
    HIPCHK(m, hipMemsetAsync(counts_dev, 0, 2 * sizeof(int32_t), m->stream));
    launch_erase_connections(*cov, neighbours, graph->order_key, slot, counts_dev, m->stream);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_connected_mask_async(jsorb_keyframe_matcher *m, const jsorb_covisibility *cov, int slot, uint8_t *mask)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(covis_check(m, CM, cov));
    if (slot < 0 || slot >= cov->max_keyframes) return kf_fail(m, CM, "slot outside [0, max_keyframes)");
    if (!mask) return kf_fail(m, CM, "NULL mask");
    HIPCHK(m, hipSetDevice(m->device));
    HIPCHK(m, hipMemsetAsync(mask, 0, (size_t)cov->max_keyframes, m->stream));
    launch_connected_mask(*cov, slot, mask, m->stream);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_best_covisibles_async(jsorb_keyframe_matcher *m, const jsorb_covisibility *cov, int n, const int32_t *slots, int N, int32_t *out,
                                int32_t *out_len)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(covis_check(m, BC, cov));
    if (n < 0 || N < 1 || (long long)n * N >= (1ll << 31)) return kf_fail(m, BC, "n must not be negative, N at least 1, n x N below 2^31");
    if (n > 0 && (!slots || !out)) return kf_fail(m, BC, "NULL slots or out");
    HIPCHK(m, hipSetDevice(m->device));
    launch_best_covisibles(*cov, n, slots, N, out, out_len, m->stream);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_covisibility_copy(const jsorb_covisibility *cov, int slot, int32_t lens[2], int32_t *conn_slot, int32_t *conn_weight, int32_t *ord_slot,
                            int32_t *ord_weight)
{
    if (!cov || !lens || slot < 0 || slot >= cov->max_keyframes || cov->conn_capacity < 1 || !cov->conn_len || !cov->conn_slot || !cov->conn_weight ||
        !cov->ord_len || !cov->ord_slot || !cov->ord_weight)
        return JSORB_ERR_INVALID;
    const size_t C = (size_t)cov->conn_capacity, row = C * sizeof(int32_t);
    if (hipDeviceSynchronize() != hipSuccess) return JSORB_ERR_HIP;
    const int32_t *const src[4] = {cov->conn_slot, cov->conn_weight, cov->ord_slot, cov->ord_weight};
    int32_t *const dst[4] = {conn_slot, conn_weight, ord_slot, ord_weight};
    if (hipMemcpy(&lens[0], cov->conn_len + slot, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&lens[1], cov->ord_len + slot, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return JSORB_ERR_HIP;
    for (int i = 0; i < 4; i++)
        if (dst[i] && hipMemcpy(dst[i], src[i] + (size_t)slot * C, row, hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
    return JSORB_OK;
}

int jsorb_covisibility_build_caps(int *min_capacity, int *max_capacity)
{
    if (min_capacity) *min_capacity = covis_cap_min();
    if (max_capacity) *max_capacity = covis_cap_max();
    return JSORB_OK;
}

} // extern "C"
