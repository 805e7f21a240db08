// jsorb_new_points.hip - host side of LocalMapping::CreateNewMapPoints on the device: jsorb_create_new_map_points* (LocalMapping.cpp:243-457, all
// neighbours of a call).  It runs on a keyframe matcher (its stream; scratch of its own in npts, jsorb_handle.h).  The kernels are in
// k_new_points.hip, k_bow.hip (k_bow_group) and k_triangulate.hip (k_tri_match), the last two as jsorb_search_for_triangulation_async launches
// them, over the sides k_np_gather copies out of the pool runs.  The state (the graph, the table, the keypoints) is the caller's.
#include "jsorb_handle.h"

namespace {

const char *const NP = "create_new_map_points";

// The scratch of one call in 32-bit words, placed into a: the gathered descriptors first (16-byte aligned), then the words cleared to -1 (match12,
// claim), the rest.  Returns the words it takes (base NULL: only that).
long long new_points_layout(NewPointsArgs &a, int32_t *&minus, int32_t *&rest, int32_t *&tri_stats, int32_t *base, long long n1, long long total, long long pairs,
                            long long n_nb, long long chunks)
{
    Carve c(base);
    a.desc1 = (uint8_t *)c.take(8 * n1); a.desc2 = (uint8_t *)c.take(8 * total);
    minus = a.match12 = c.take(pairs); a.claim = c.take(total);
    rest = a.pair_row = c.take(pairs);
    a.node1 = c.take(n1); a.node2 = c.take(total); a.octave2 = c.take(total);
    a.x1 = (float *)c.take(n1); a.y1 = (float *)c.take(n1); a.x2 = (float *)c.take(total); a.y2 = (float *)c.take(total);
    a.free1 = (uint8_t *)c.take((n1 + 3) / 4); a.stereo1 = (uint8_t *)c.take((n1 + 3) / 4);
    a.free2 = (uint8_t *)c.take((total + 3) / 4); a.stereo2 = (uint8_t *)c.take((total + 3) / 4);
    a.info = c.take(1 + n_nb); a.nb_slot = c.take(n_nb); a.ow = (float *)c.take(3 * (n_nb + 1));
    a.chunk_sum = (unsigned *)c.take(chunks); a.chunk_pre = (unsigned *)c.take(chunks + 1);
    tri_stats = c.take(KF_STATS);
    return c.at;
}

} // namespace

extern "C" {

int jsorb_create_new_map_points_async(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, const jsorb_keyframe_graph *graph,
                                      const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_new_point_keypoints *extra,
                                      const jsorb_new_point_state *state, int current_slot, int n1, int run_capacity, int n_neighbours,
                                      const int32_t *neighbour_slot, const jsorb_keyframe_pose *pose, const float *F12, const float *epipole,
                                      float ratio_factor, int current_kf_id, int row_capacity, const int32_t *new_row, int log_cap, int32_t *verdict,
                                      uint8_t *path, float *x3D, int32_t *log_out, int32_t *counts_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!params || !graph || !table || !kp || !extra || !state || !pose || !counts_dev) return kf_fail(m, NP, "NULL params, graph, table, kp, extra, state, pose or counts_dev");
    if (params->n_levels < 1 || params->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, NP, "n_levels out of range");
    if (params->th_low < 0 || params->th_low > 255) return kf_fail(m, NP, "th_low must be in [0, 255]");
    if (params->check_orientation) return kf_fail(m, NP, "check_orientation must be 0 (LocalMapping.cpp:221)", JSORB_ERR_UNSUPPORTED);
    const jsorb_keyframe_graph &g = *graph;
    const int S = g.max_keyframes, pool = g.pool_entries, n_rows = table->n_rows;
    if (S < 0 || pool < 0 || n_rows < 0 || n1 < 0 || run_capacity < 0 || row_capacity < 0 || log_cap < 0)
        return kf_fail(m, NP, "max_keyframes, pool_entries, n_rows, n1, run_capacity, row_capacity and log_cap must not be negative");
    if (n_neighbours < 0 || n_neighbours > JSORB_BOW_MAX_KEYFRAMES) return kf_fail(m, NP, "n_neighbours must be in [0, 256]");
    if (n1 >= (1 << 18) || run_capacity >= (1 << 18)) return kf_fail(m, NP, "n1 and run_capacity must be below 262144");
    if (log_cap >= (1 << 27)) return kf_fail(m, NP, "log_cap too large");
    if (kp->pool_entries != pool) return kf_fail(m, NP, "the keypoints and the graph differ in pool_entries");
    if ((long long)n_neighbours * std::max(n1, run_capacity) >= (1 << 24)) return kf_fail(m, NP, "n_neighbours x max(n1, run_capacity) too large", JSORB_ERR_UNSUPPORTED);
    if (S > 0 && (!g.state || !g.order_key || !g.point_off || !g.point_len || (pool > 0 && !g.point_pool))) return kf_fail(m, NP, "NULL graph array");
    if (pool > 0 && !g.registered) return kf_fail(m, NP, "graph->registered is NULL: the call writes those bytes");
    if (pool > 0 && (!kp->x || !kp->y || !kp->octave || !kp->desc || !extra->node)) return kf_fail(m, NP, "NULL keypoint array");
    if (pool > 0 && kp->uright && (!extra->depth || !extra->cos_stereo)) return kf_fail(m, NP, "depth and cos_stereo are needed with uright");
    if (!extra->raw_x != !extra->raw_y) return kf_fail(m, NP, "raw_x and raw_y: both NULL or both given");
    if (n_rows > 0 && (!table->Px || !table->Py || !table->Pz || !table->Pnx || !table->Pny || !table->Pnz || !table->MaxDistance ||
                       !table->invariance_maxDistance || !table->invariance_minDistance || !table->desc || !table->bad))
        return kf_fail(m, NP, "NULL table array");
    if ((uintptr_t)kp->desc % 16 || (uintptr_t)table->desc % 16) return kf_fail(m, NP, "descriptors must be 16-byte aligned");
    if (state->point_pool != g.point_pool || state->registered != g.registered || state->bad != table->bad || state->desc != table->desc ||
        state->Px != table->Px || state->Py != table->Py || state->Pz != table->Pz || state->Pnx != table->Pnx || state->Pny != table->Pny ||
        state->Pnz != table->Pnz || state->MaxDistance != table->MaxDistance || state->invariance_maxDistance != table->invariance_maxDistance ||
        state->invariance_minDistance != table->invariance_minDistance)
        return kf_fail(m, NP, "a new_point_state array is not the graph's or the table's");
    if (!state->visible != !state->found) return kf_fail(m, NP, "visible and found: both NULL or both given");
    if (n_neighbours > 0 && (!neighbour_slot || !F12 || !epipole)) return kf_fail(m, NP, "NULL neighbour_slot, F12 or epipole");
    if (row_capacity > 0 && !new_row) return kf_fail(m, NP, "NULL new_row");
    if (log_cap > 0 && !log_out) return kf_fail(m, NP, "NULL log_out");
    if (n_neighbours > 0 && n1 > 0 && (!verdict || !path || !x3D)) return kf_fail(m, NP, "NULL verdict, path or x3D");
    HIPCHK(m, hipSetDevice(m->device));
    hipStream_t st = m->stream;
    KfCall &c = m->call[jsorb_keyframe_matcher::NEW_POINTS];
    RCCHK(reserve_device(m, c.stats, 16 * sizeof(int)));
    const long long pairs = (long long)n_neighbours * n1, total = (long long)n_neighbours * run_capacity, chunks = (pairs + new_points_chunk() - 1) / new_points_chunk();
    RCCHK(reserve_sort_keys(m, n1, (int)total));
    NewPointsArgs a{};
    int32_t *minus = nullptr, *rest = nullptr, *tri_stats = nullptr;
    RCCHK(reserve_words(m, m->npts, new_points_layout(a, minus, rest, tri_stats, nullptr, n1, total, pairs, n_neighbours, chunks)));
    new_points_layout(a, minus, rest, tri_stats, m->npts.p, n1, total, pairs, n_neighbours, chunks);
    a.g = g; a.kp = *kp; a.ex = *extra; a.st = *state;
    a.n_rows = n_rows; a.current_slot = current_slot; a.n1 = n1; a.cap = run_capacity; a.n_nb = n_neighbours;
    a.row_capacity = row_capacity; a.log_cap = log_cap; a.current_kf_id = current_kf_id; a.n_levels = params->n_levels; a.ratio_factor = ratio_factor;
    for (int l = 0; l < params->n_levels; l++) {
        a.scale_factor[l] = params->scale_factor[l];
        a.chi2_mono[l] = 5.991 * (double)params->level_sigma2[l];        // :380, the double product of the promoted comparison
        a.chi2_stereo[l] = 7.8 * (double)params->level_sigma2[l];        // :391
    }
    a.new_row = new_row; a.verdict = verdict; a.path = path; a.x3D = x3D; a.log_out = log_out; a.counts_dev = counts_dev; a.stats = c.stats;
    HIPCHK(m, hipMemsetAsync(c.stats, 0, 16 * sizeof(int), st));
    c.done = true;
    if (rest > minus) HIPCHK(m, hipMemsetAsync(minus, 0xFF, (size_t)(rest - minus) * sizeof(int32_t), st));
    HIPCHK(m, hipMemsetAsync(tri_stats, 0, KF_STATS * sizeof(int32_t), st));
    if (log_cap > 0) HIPCHK(m, hipMemsetAsync(log_out, 0xFF, (size_t)log_cap * 4 * sizeof(int32_t), st));
    NewPointsSlots slots{};
    for (int t = 0; t < n_neighbours; t++) slots.slot[t] = neighbour_slot[t];
    launch_new_points_gather(a, slots, st);
    HIPCHK(m, hipGetLastError());
    if (pairs > 0 && total > 0) {
        // the matcher's two stages as jsorb_search_for_triangulation_async launches them: neighbour t is entries t * run_capacity ..
        TriArgs tr{};
        for (int t = 0; t <= n_neighbours; t++) tr.kf_start[t] = t * run_capacity;
        tr.n1 = n1; tr.free1 = a.free1; tr.stereo1 = a.stereo1; tr.x1 = a.x1; tr.y1 = a.y1; tr.desc1 = a.desc1;
        tr.n_kf = n_neighbours; tr.free2 = a.free2; tr.stereo2 = a.stereo2; tr.x2 = a.x2; tr.y2 = a.y2; tr.octave2 = a.octave2; tr.desc2 = a.desc2;
        tr.th_low = params->th_low; tr.only_stereo = params->only_stereo; tr.n_levels = params->n_levels;
        for (int l = 0; l < params->n_levels; l++) {
            tr.gate[l] = 100.0f * params->scale_factor[l];
            tr.line[l] = 3.84 * (double)params->level_sigma2[l];
        }
        tr.sorted1 = m->sort1; tr.sorted2 = m->sort2; tr.match12 = a.match12; tr.stats = tri_stats;
        launch_bow_group(bow_group_args(tr.kf_start, a.node1, n1, n_neighbours, a.node2, m->sort1, m->sort2), st);
        HIPCHK(m, hipGetLastError());
        for (int k0 = 0; k0 < n_neighbours; k0 += TR_KF_CHUNK) {
            TriGeom tg{};
            tg.kf0 = k0; tg.n = std::min(TR_KF_CHUNK, n_neighbours - k0);
            for (int i = 0; i < tg.n; i++) {
                memcpy(tg.f[i], F12 + 9 * (size_t)(k0 + i), 9 * sizeof(float));
                tg.f[i][9] = epipole[2 * (size_t)(k0 + i)];
                tg.f[i][10] = epipole[2 * (size_t)(k0 + i) + 1];
            }
            launch_tri_match(tr, tg, st);
            HIPCHK(m, hipGetLastError());
        }
    }
    for (int k0 = 0; k0 < n_neighbours; k0 += NP_KF_CHUNK) {
        NewPointsPoses q{};
        q.kf0 = k0; q.n = std::min(NP_KF_CHUNK, n_neighbours - k0);
        q.cur = pose[0];
        for (int i = 0; i < q.n; i++) q.nb[i] = pose[1 + k0 + i];
        launch_new_points_verdict(a, q, st);
        HIPCHK(m, hipGetLastError());
    }
    launch_new_points_apply(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_create_new_map_points(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, const jsorb_keyframe_graph *graph,
                                const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_new_point_keypoints *extra,
                                const jsorb_new_point_state *state, int current_slot, int n1, int run_capacity, int n_neighbours,
                                const int32_t *neighbour_slot, const jsorb_keyframe_pose *pose, const float *F12, const float *epipole,
                                float ratio_factor, int current_kf_id, int row_capacity, const int32_t *new_row, int log_cap, int32_t *verdict,
                                uint8_t *path, float *x3D, int32_t *log_out, int32_t *counts_dev, int32_t *verdict_host, uint8_t *path_host,
                                float *x3D_host, int32_t *log_host, int32_t counts_host[12])
{
    if (!m) return JSORB_ERR_INVALID;
    if (n_neighbours < 0 || n1 < 0 || log_cap < 0) return kf_fail(m, NP, "n_neighbours, n1 and log_cap must not be negative");
    const size_t pairs = (size_t)n_neighbours * n1, nlog = (size_t)log_cap * 4;
    if (!counts_host || (pairs && (!verdict_host || !path_host || !x3D_host)) || (nlog && !log_host)) return kf_fail(m, NP, "NULL host output");
    RCCHK(jsorb_create_new_map_points_async(m, params, graph, table, kp, extra, state, current_slot, n1, run_capacity, n_neighbours, neighbour_slot, pose,
                                            F12, epipole, ratio_factor, current_kf_id, row_capacity, new_row, log_cap, verdict, path, x3D, log_out,
                                            counts_dev));
    // the byte array on its own, the words gathered for one copy back
    if (pairs) HIPCHK(m, hipMemcpyAsync(path_host, path, pairs, hipMemcpyDeviceToHost, m->stream));
    const int32_t *const src[4] = {counts_dev, verdict, (const int32_t *)x3D, log_out};
    int32_t *const dst[4] = {counts_host, verdict_host, (int32_t *)x3D_host, log_host};
    const size_t n[4] = {NP_COUNTS, pairs, 3 * pairs, nlog};
    return read_back(m, m->stream, m->staging, 4, src, dst, n);
}

int jsorb_create_new_map_points_stats(jsorb_keyframe_matcher *m, int32_t counts[12])
{
    if (!m) return JSORB_ERR_INVALID;
    if (!counts) return kf_fail(m, NP, "NULL counts");
    return read_stats(m, m->call[jsorb_keyframe_matcher::NEW_POINTS].done, "create_new_map_points_stats before jsorb_create_new_map_points",
                      m->call[jsorb_keyframe_matcher::NEW_POINTS].stats, counts, NP_COUNTS);
}

int jsorb_create_new_map_points_build_caps(int *scan_chunk)
{
    if (scan_chunk) *scan_chunk = new_points_chunk();
    return JSORB_OK;
}

} // extern "C"
