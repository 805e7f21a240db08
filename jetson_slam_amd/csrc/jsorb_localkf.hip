// jsorb_localkf.hip - host side of the local keyframes of Tracking::TrackLocalMap: jsorb_local_keyframes* (UpdateLocalKeyFrames and the
// concatenation of the keyframes' rows in one call on the handle's stream, k_local_keyframes.hip).  The row words are the local map's (struct lm,
// jsorb_handle.h): all ones between calls, set back by every call; the rest of the scratch is struct lk.
#include "jsorb_handle.h"

namespace jsorb_host __attribute__((visibility("hidden"))) {

void local_kf_release(jsorb_extractor *e) { free_device(e->lk.slot, e->lk.stats, e->lk.out.p); }

} // namespace jsorb_host

namespace {

const char *const LK = "local_keyframes";

} // namespace

extern "C" {

int jsorb_local_keyframes_async(jsorb_extractor *e, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                                const int32_t *frame_point_row, int n_frame, int kf_capacity, int entry_capacity, int32_t *local_kf_slot,
                                int32_t *state_io, int32_t *local_kf_start, int32_t *local_point_row, int32_t *counts_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!graph || !table || !local_kf_slot || !state_io || !local_kf_start || !counts_dev)
        return kf_fail(e, LK, "NULL graph, table, local_kf_slot, state_io, local_kf_start or counts_dev");
    const jsorb_keyframe_graph &g = *graph;
    const int S = g.max_keyframes;
    if (S < 0 || g.pool_entries < 0 || g.child_entries < 0 || table->n_rows < 0 || n_frame < 0 || entry_capacity < 0)
        return kf_fail(e, LK, "max_keyframes, pool_entries, child_entries, n_rows, n_frame and entry_capacity must not be negative");
    if (S >= (1 << 24)) return kf_fail(e, LK, "more than 16777215 keyframe slots");
    if (kf_capacity < 84) return kf_fail(e, LK, "kf_capacity must be at least 84");
    if (entry_capacity >= (1 << 24)) return kf_fail(e, LK, "more than 16777215 entries");
    if (S > 0 && (!g.state || !g.order_key || !g.point_off || !g.point_len || !g.neighbours || !g.child_off || !g.child_len || !g.parent ||
                  (g.pool_entries > 0 && !g.point_pool) || (g.child_entries > 0 && !g.child_pool)))
        return kf_fail(e, LK, "NULL graph array");
    if (table->n_rows > 0 && !table->bad) return kf_fail(e, LK, "NULL table array");
    if (entry_capacity > 0 && !local_point_row) return kf_fail(e, LK, "NULL local_point_row");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    RCCHK(reserve_row_words(e, e->lm.row, table->n_rows, 0xff, st));
    const int slots = std::max(S, 1);
    RCCHK(reserve_device(e, e->lk.slot, (size_t)slots * (2 * sizeof(int32_t) + 1), &e->lk.slots, slots));
    RCCHK(reserve_device(e, e->lk.stats, (LK_STATS + 2) * sizeof(int32_t)));
    RCCHK(wait_lanes(e, st, e));       // frame_point_row may come from work on the lanes of a batch
    mark_main_stream(e);
    LocalKfArgs a{};
    a.g = g;
    a.n_rows = table->n_rows; a.bad = table->bad;
    a.frame_row = frame_point_row; a.n_frame = frame_point_row ? n_frame : 0;
    a.kf_capacity = kf_capacity; a.entry_capacity = entry_capacity;
    a.word = e->lm.row.word;
    a.vote = e->lk.slot; a.order = e->lk.slot + e->lk.slots; a.first = reinterpret_cast<uint8_t *>(e->lk.slot + 2 * (size_t)e->lk.slots);
    a.stats = e->lk.stats; a.best = reinterpret_cast<unsigned long long *>(e->lk.stats + LK_STATS);
    a.local_kf_slot = local_kf_slot; a.state_io = state_io;
    a.local_kf_start = local_kf_start; a.local_point_row = local_point_row; a.counts = counts_dev;
    e->lm.row.dirty = true;            // until all five kernels are enqueued: k_lk_gather is the one that sets the words back
    launch_local_keyframes(a, st);
    HIPCHK(e, hipGetLastError());
    e->lm.row.dirty = false;
    e->lk.done = true;
    return JSORB_OK;
}

int jsorb_local_keyframes(jsorb_extractor *e, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table, const int32_t *frame_point_row,
                          int n_frame, int kf_capacity, int entry_capacity, int32_t *local_kf_slot, int32_t *state_io, int32_t *local_kf_start,
                          int32_t *local_point_row, int32_t *counts_dev, int32_t *local_kf_slot_host, int32_t state_host[2], int32_t counts_host[8])
{
    if (!e) return JSORB_ERR_INVALID;
    if (!local_kf_slot_host || !state_host || !counts_host) return kf_fail(e, LK, "NULL host output");
    RCCHK(jsorb_local_keyframes_async(e, graph, table, frame_point_row, n_frame, kf_capacity, entry_capacity, local_kf_slot, state_io, local_kf_start,
                                      local_point_row, counts_dev));
    const int32_t *const src[3] = {counts_dev, state_io, local_kf_slot};
    int32_t *const dst[3] = {counts_host, state_host, local_kf_slot_host};
    const size_t n[3] = {8, 2, (size_t)kf_capacity};
    return read_back(e, e->stream, e->lk.out, 3, src, dst, n);
}

int jsorb_local_keyframes_stats(jsorb_extractor *e, int *n_counter, int *n_first, int *n_local, int *n_neighbours, int *n_children, int *n_parents,
                                int *n_invalid_runs, int *end_reason)
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[LK_STATS] = {0};
    RCCHK(read_stats(e, e->lk.done, "local_keyframes_stats before jsorb_local_keyframes", e->lk.stats, s, LK_STATS));
    int *const out[LK_STATS] = {n_counter, n_first, n_local, n_neighbours, n_children, n_parents, n_invalid_runs, end_reason};
    for (int i = 0; i < LK_STATS; i++)
        if (out[i]) *out[i] = s[i];
    return JSORB_OK;
}

int jsorb_local_keyframes_build_caps(int *member_lds_slots, int *child_lds_entries)
{
    if (member_lds_slots) *member_lds_slots = local_kf_member_lds();
    if (child_lds_entries) *child_lds_entries = local_kf_child_lds();
    return JSORB_OK;
}

} // extern "C"
