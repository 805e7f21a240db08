// jsorb_loop.hip - host side of the keyframe matcher's loop-closing calls (jsorb_search_by_bow_kf*, jsorb_search_by_sim3*): the matchers of
// LoopClosing::ComputeSim3.  They run on the jsorb_keyframe_matcher of jsorb_keyframes.hip (LoopClosing is a thread of its own and creates its own),
// with statistics and "done" marks of their own.  The kernels are in k_loop.hip; the grouping is k_bow.hip's k_bow_group with KF1 as the frame side,
// the rotation check k_triangulate.hip's k_tri_resolve, the grids k_fuse.hip's k_fuse_grids.
#include "jsorb_handle.h"

namespace {

#define LOOP_STATS 8                            // k_tri_resolve's layout: node pairs, distances, ., largest node, ind1 + 1, ind2 + 1, ind3 + 1
#define SIM3_STATS 8                            // windows, walked, distances, largest window, agreements

int loop_fail(jsorb_keyframe_matcher *m, const std::string &msg, int rc = JSORB_ERR_INVALID)
{
    m->err = msg;
    return rc;
}

int sim3_check(jsorb_keyframe_matcher *m, const jsorb_sim3_params *p, const jsorb_sim3_side *s1, const jsorb_sim3_side *s2)
{
    if (!p || !s1 || !s2) return loop_fail(m, "search_by_sim3: NULL params or side");
    if (p->n_levels < 1 || p->n_levels > JSORB_MAX_LEVELS) return loop_fail(m, "search_by_sim3: n_levels out of range");
    if (p->th_high < 0 || p->th_high > 255) return loop_fail(m, "search_by_sim3: th_high must be in [0, 255]");
    if (p->cols < 1 || p->rows < 1 || (long long)p->cols * p->rows > FUSE_MAX_CELLS) return loop_fail(m, "search_by_sim3: grid size out of range (cols*rows <= 4096)");
    if (s1->n < 0 || s2->n < 0 || (long long)s1->n + s2->n >= (1 << 18)) return loop_fail(m, "search_by_sim3: n1 + n2 must be in [0, 262143]");
    for (const jsorb_sim3_side *s : {s1, s2}) {
        if (s->n > 0 && (!s->x || !s->y || !s->octave || !s->kp_desc || !s->Px || !s->Py || !s->Pz || !s->max_distance || !s->min_dist_inv || !s->max_dist_inv ||
                         !s->mp_desc || !s->search))
            return loop_fail(m, "search_by_sim3: NULL side array");
        if (s->n > 0 && ((uintptr_t)s->kp_desc % 16 || (uintptr_t)s->mp_desc % 16)) return loop_fail(m, "search_by_sim3: descriptors must be 16-byte aligned");
    }
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_loop_build_caps(int *node_regs)
{
    if (node_regs) *node_regs = loop_node_regs();
    return JSORB_OK;
}

int jsorb_search_by_bow_kf_async(jsorb_keyframe_matcher *m, const jsorb_bow_params *params, int n1, const int32_t *node1, const uint8_t *valid1,
                                 const float *angle1, const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2,
                                 const uint8_t *valid2, const float *angle2, const uint8_t *desc2, int32_t *match12, int32_t *n_matches_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!params) return loop_fail(m, "search_by_bow_kf: NULL params");
    if (n_keyframes < 0 || n_keyframes > JSORB_BOW_MAX_KEYFRAMES) return loop_fail(m, "search_by_bow_kf: n_keyframes must be in [0, 256]");
    if (n1 < 0 || n1 >= (1 << 18)) return loop_fail(m, "search_by_bow_kf: n1 must be in [0, 262143]");
    if (n_keyframes > 0 && (!kf_start || !n_matches_dev)) return loop_fail(m, "search_by_bow_kf: NULL kf_start or n_matches");
    LoopBowArgs a{};
    int base = 0, total = 0, rc = 0;
    if (const char *bad = rebase_kf_start(kf_start, n_keyframes, a.kf_start, &base, &total, &rc)) return loop_fail(m, std::string("search_by_bow_kf: ") + bad);
    if (n1 > 0 && (!node1 || !valid1 || !angle1 || !desc1)) return loop_fail(m, "search_by_bow_kf: NULL KF1 array");
    if (total > 0 && (!node2 || !valid2 || !angle2 || !desc2)) return loop_fail(m, "search_by_bow_kf: NULL candidate array");
    if ((uintptr_t)desc1 % 16 || (uintptr_t)desc2 % 16) return loop_fail(m, "search_by_bow_kf: descriptors must be 16-byte aligned");
    if (n_keyframes > 0 && n1 > 0 && !match12) return loop_fail(m, "search_by_bow_kf: NULL match12");
    HIPCHK(m, hipSetDevice(m->device));
    RCCHK(reserve_device(m, m->loop_stats, LOOP_STATS * sizeof(int)));
    RCCHK(reserve_device(m, m->sort1, (size_t)std::max(n1, 1) * sizeof(unsigned long long), &m->cap1, std::max(n1, 1)));
    RCCHK(reserve_device(m, m->sort2, (size_t)std::max(total, 1) * sizeof(unsigned long long), &m->cap2, std::max(total, 1)));
    RCCHK(reserve_device(m, m->matched2, (size_t)std::max(total, 1), &m->matched2_cap, std::max(total, 1)));
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(clear_kf_outputs(m, st, m->loop_stats, LOOP_STATS, n_keyframes, n1, total, n_matches_dev, match12, &run));
    m->loop_done = true;
    if (!run) return JSORB_OK;
    HIPCHK(m, hipMemsetAsync(m->matched2, 0, (size_t)total, st));
    // the grouping: KF1 as the frame side of k_bow_group, the candidates as its keyframes
    BowMatchArgs b{};
    memcpy(b.kf_start, a.kf_start, sizeof(b.kf_start));
    b.f_node = node1; b.N = n1; b.n_kf = n_keyframes; b.kf_node = node2 + base;
    b.f_sorted = m->sort1; b.kf_sorted = m->sort2;
    a.n1 = n1; a.valid1 = valid1; a.desc1 = desc1;
    a.n_kf = n_keyframes; a.valid2 = valid2 + base; a.desc2 = desc2 + (size_t)32 * base;
    a.p = *params;
    a.sorted1 = m->sort1; a.sorted2 = m->sort2; a.matched2 = m->matched2;
    a.match12 = match12; a.stats = m->loop_stats;
    // the rotation check: k_tri_resolve over the same rows (angle1[idx1] - angle2[match12[idx1]]), its kept bins in the same statistics words
    TriArgs r{};
    memcpy(r.kf_start, a.kf_start, sizeof(r.kf_start));
    r.n1 = n1; r.angle1 = angle1; r.n_kf = n_keyframes; r.angle2 = angle2 + base; r.check_orientation = params->check_orientation;
    r.match12 = match12; r.n_matches = n_matches_dev; r.stats = m->loop_stats;
    launch_bow_group(b, st);
    HIPCHK(m, hipGetLastError());
    launch_loop_bow_match(a, st);
    HIPCHK(m, hipGetLastError());
    launch_tri_resolve(r, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_search_by_bow_kf(jsorb_keyframe_matcher *m, const jsorb_bow_params *params, int n1, const int32_t *node1, const uint8_t *valid1,
                           const float *angle1, const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2,
                           const uint8_t *valid2, const float *angle2, const uint8_t *desc2, int32_t *match12_host, int *n_matches_host)
{
    if (!m) return JSORB_ERR_INVALID;
    if (n_keyframes < 0 || n_keyframes > JSORB_BOW_MAX_KEYFRAMES) return loop_fail(m, "search_by_bow_kf: n_keyframes must be in [0, 256]");
    if (n1 < 0 || n1 >= (1 << 18)) return loop_fail(m, "search_by_bow_kf: n1 must be in [0, 262143]");
    if (n_keyframes > 0 && (!n_matches_host || (n1 > 0 && !match12_host))) return loop_fail(m, "search_by_bow_kf: NULL host output");
    HIPCHK(m, hipSetDevice(m->device));
    const size_t rows = (size_t)n_keyframes * n1;
    if (rows > (size_t)INT_MAX - JSORB_BOW_MAX_KEYFRAMES) return loop_fail(m, "search_by_bow_kf: n_keyframes x n1 too large", JSORB_ERR_UNSUPPORTED);
    const int want = (int)std::max(rows, (size_t)1);
    RCCHK(reserve_device(m, m->loop_out, ((size_t)JSORB_BOW_MAX_KEYFRAMES + want) * sizeof(int32_t), &m->loop_out_cap, want));
    int32_t *cnt = m->loop_out, *mk = cnt + JSORB_BOW_MAX_KEYFRAMES;
    RCCHK(jsorb_search_by_bow_kf_async(m, params, n1, node1, valid1, angle1, desc1, n_keyframes, kf_start, node2, valid2, angle2, desc2, mk, cnt));
    return copy_kf_results(m, n_keyframes, rows, cnt, mk, match12_host, n_matches_host);
}

int jsorb_search_by_bow_kf_stats(jsorb_keyframe_matcher *m, int *n_node_pairs, int *n_distances, int *largest_node, int kept_bins[3])
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[LOOP_STATS] = {0};
    RCCHK(read_stats(m, m->loop_done, "search_by_bow_kf_stats before jsorb_search_by_bow_kf", m->loop_stats, s, LOOP_STATS));
    if (n_node_pairs) *n_node_pairs = s[0];
    if (n_distances) *n_distances = s[1];
    if (largest_node) *largest_node = s[3];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[4 + b] - 1;
    return JSORB_OK;
}

int jsorb_search_by_sim3_async(jsorb_keyframe_matcher *m, const jsorb_sim3_params *params, const jsorb_sim3_side *side1, const jsorb_sim3_side *side2,
                               int32_t *match1, int32_t *match2, int32_t *match12, int32_t *n_found_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(sim3_check(m, params, side1, side2));
    const int n1 = side1->n, n2 = side2->n;
    if (!n_found_dev || (n1 > 0 && (!match1 || !match12)) || (n2 > 0 && !match2)) return loop_fail(m, "search_by_sim3: NULL output");
    HIPCHK(m, hipSetDevice(m->device));
    const int n_cells = params->cols * params->rows, want_grid = 2 * (n_cells + 1), total = std::max(n1 + n2, 1);
    RCCHK(reserve_device(m, m->sim3_stats, SIM3_STATS * sizeof(int)));
    RCCHK(reserve_device(m, m->grid_start, (size_t)want_grid * sizeof(int32_t), &m->grid_cap, want_grid));
    RCCHK(reserve_device(m, m->grid_items, (size_t)total * sizeof(int32_t), &m->items_cap, total));
    hipStream_t st = m->stream;
    HIPCHK(m, hipMemsetAsync(m->sim3_stats, 0, SIM3_STATS * sizeof(int), st));
    HIPCHK(m, hipMemsetAsync(n_found_dev, 0, sizeof(int32_t), st));
    m->sim3_done = true;
    if (n1 == 0 || n2 == 0) {                       // nothing to search in, or nothing to search: everything is -1 / 0
        if (n1 > 0) {
            HIPCHK(m, hipMemsetAsync(match1, 0xff, (size_t)n1 * sizeof(int32_t), st));
            HIPCHK(m, hipMemsetAsync(match12, 0xff, (size_t)n1 * sizeof(int32_t), st));
        }
        if (n2 > 0) HIPCHK(m, hipMemsetAsync(match2, 0xff, (size_t)n2 * sizeof(int32_t), st));
        return JSORB_OK;
    }
    Sim3Args a{};
    a.p = *params;
    const jsorb_sim3_side *in[2] = {side1, side2};
    int32_t *out[2] = {match1, match2};
    for (int d = 0; d < 2; d++) {
        const jsorb_sim3_side &s = *in[d];
        Sim3Side &k = a.s[d];
        k.n = s.n; k.x = s.x; k.y = s.y; k.octave = s.octave; k.kp_desc = s.kp_desc;
        k.Px = s.Px; k.Py = s.Py; k.Pz = s.Pz; k.max_distance = s.max_distance; k.min_dist_inv = s.min_dist_inv; k.max_dist_inv = s.max_dist_inv;
        k.mp_desc = s.mp_desc; k.search = s.search;
        memcpy(k.T, s.Rw, 9 * sizeof(float)); memcpy(k.T + 9, s.tw, 3 * sizeof(float));
        memcpy(k.T + 12, s.sR, 9 * sizeof(float)); memcpy(k.T + 21, s.t, 3 * sizeof(float));
        k.cell_start = m->grid_start + (size_t)d * (n_cells + 1);
        k.cell_items = m->grid_items + (d ? n1 : 0);
        k.match = out[d];
        // the keyframe's grid: k_fuse_grids over one keyframe, its CSR behind the other one's in the matcher's grid scratch
        FuseGridArgs g{};
        g.kf_start[0] = 0; g.kf_start[1] = s.n;
        g.x = s.x; g.y = s.y;
        g.min_x = params->min_x; g.min_y = params->min_y; g.inv_w = params->inv_w; g.inv_h = params->inv_h; g.cols = params->cols; g.rows = params->rows;
        g.cell_start = m->grid_start + (size_t)d * (n_cells + 1); g.cell_items = m->grid_items + (d ? n1 : 0);
        launch_fuse_grids(g, 1, st);
        HIPCHK(m, hipGetLastError());
    }
    a.match12 = match12; a.n_found = n_found_dev; a.stats = m->sim3_stats;
    launch_sim3_match(a, st);
    HIPCHK(m, hipGetLastError());
    launch_sim3_agree(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_search_by_sim3(jsorb_keyframe_matcher *m, const jsorb_sim3_params *params, const jsorb_sim3_side *side1, const jsorb_sim3_side *side2,
                         int32_t *match1_host, int32_t *match2_host, int32_t *match12_host, int *n_found)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(sim3_check(m, params, side1, side2));
    const int n1 = side1->n, n2 = side2->n;
    if (!n_found || (n1 > 0 && !match12_host)) return loop_fail(m, "search_by_sim3: NULL host output");
    HIPCHK(m, hipSetDevice(m->device));
    const int want = 2 * n1 + n2 + 1;
    RCCHK(reserve_device(m, m->sim3_out, (size_t)want * sizeof(int32_t), &m->sim3_out_cap, want));
    int32_t *cnt = m->sim3_out, *m1 = cnt + 1, *m2 = m1 + n1, *m12 = m2 + n2;
    RCCHK(jsorb_search_by_sim3_async(m, params, side1, side2, m1, m2, m12, cnt));
    std::vector<int32_t> h((size_t)want);            // the count and the three arrays lie next to each other: one copy
    HIPCHK(m, hipMemcpyAsync(h.data(), cnt, (size_t)want * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    *n_found = h[0];
    if (n1 > 0 && match1_host) memcpy(match1_host, h.data() + 1, (size_t)n1 * sizeof(int32_t));
    if (n2 > 0 && match2_host) memcpy(match2_host, h.data() + 1 + n1, (size_t)n2 * sizeof(int32_t));
    if (n1 > 0) memcpy(match12_host, h.data() + 1 + n1 + n2, (size_t)n1 * sizeof(int32_t));
    return JSORB_OK;
}

int jsorb_search_by_sim3_stats(jsorb_keyframe_matcher *m, int *n_windows, int *n_walked, int *n_distances, int *largest_window, int *n_agree)
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[SIM3_STATS] = {0};
    RCCHK(read_stats(m, m->sim3_done, "search_by_sim3_stats before jsorb_search_by_sim3", m->sim3_stats, s, SIM3_STATS));
    if (n_windows) *n_windows = s[0];
    if (n_walked) *n_walked = s[1];
    if (n_distances) *n_distances = s[2];
    if (largest_window) *largest_window = s[3];
    if (n_agree) *n_agree = s[4];
    return JSORB_OK;
}

} // extern "C"
