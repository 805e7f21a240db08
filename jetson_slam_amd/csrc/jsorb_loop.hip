// jsorb_loop.hip - host side of the keyframe matcher's loop-closing calls (jsorb_search_by_bow_kf*, jsorb_search_by_sim3*,
// jsorb_search_by_projection_sim3*): the matchers of LoopClosing::ComputeSim3.  They run on the jsorb_keyframe_matcher of jsorb_keyframes.hip (LoopClosing is a thread of its own and creates its own),
// each with a call state of its own (KfCall).  The kernels are in k_loop.hip; the grouping is k_bow.hip's k_bow_group with KF1 as the frame side,
// the rotation check k_triangulate.hip's k_tri_resolve, the grids k_fuse.hip's k_fuse_grids; SearchByProjection(pKF, Scw, ...)'s are in k_scw.hip.
#include "jsorb_handle.h"

namespace {

// The calls' statistics words (KF_STATS each).  search_by_bow_kf: node pairs, distances, ., largest node, ind1 + 1, ind2 + 1, ind3 + 1 (the triangulation
// matcher's layout, k_tri_resolve's kept bins).  search_by_sim3: windows, walked, distances, largest window, agreements.
// search_by_projection_sim3: rounds, keys kept, points over the cap (claim_resolve's three), windows, distances, largest window.
// The feature names and texts the shared frames (jsorb_handle.h: kf_*) put into the refusals:
const char *const BOW_KF = "search_by_bow_kf", *const BOW_KF_N1 = "n1 must be in [0, 262143]", *const SIM3 = "search_by_sim3";
const char *const SCW = "search_by_projection_sim3";

int sim3_check(jsorb_keyframe_matcher *m, const jsorb_sim3_params *p, const jsorb_sim3_side *s1, const jsorb_sim3_side *s2)
{
    if (!p || !s1 || !s2) return kf_fail(m, SIM3, "NULL params or side");
    if (p->n_levels < 1 || p->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, SIM3, "n_levels out of range");
    if (p->th_high < 0 || p->th_high > 255) return kf_fail(m, SIM3, "th_high must be in [0, 255]");
    if (p->cols < 1 || p->rows < 1 || (long long)p->cols * p->rows > FUSE_MAX_CELLS) return kf_fail(m, SIM3, "grid size out of range (cols*rows <= 4096)");
    if (s1->n < 0 || s2->n < 0 || (long long)s1->n + s2->n >= (1 << 18)) return kf_fail(m, SIM3, "n1 + n2 must be in [0, 262143]");
    for (const jsorb_sim3_side *s : {s1, s2}) {
        if (s->n > 0 && (!s->x || !s->y || !s->octave || !s->kp_desc || !s->Px || !s->Py || !s->Pz || !s->max_distance || !s->min_dist_inv || !s->max_dist_inv ||
                         !s->mp_desc || !s->search))
            return kf_fail(m, SIM3, "NULL side array");
        if (s->n > 0 && ((uintptr_t)s->kp_desc % 16 || (uintptr_t)s->mp_desc % 16)) return kf_fail(m, SIM3, "descriptors must be 16-byte aligned");
    }
    return JSORB_OK;
}

// the argument checks both forms of jsorb_search_by_projection_sim3 share (the outputs are each form's own)
int scw_check(jsorb_keyframe_matcher *m, const jsorb_scw_params *p, int n_points, const float *Px, const float *Py, const float *Pz, const float *Nx,
              const float *Ny, const float *Nz, const float *max_distance, const float *min_dist_inv, const float *max_dist_inv, const uint8_t *desc,
              int n_keypoints, const float *x, const float *y, const int32_t *octave, const uint8_t *kf_desc)
{
    if (!p) return kf_fail(m, SCW, "NULL params");
    if (p->n_levels < 1 || p->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, SCW, "n_levels out of range");
    if (p->th_low < 0 || p->th_low > 255) return kf_fail(m, SCW, "th_low must be in [0, 255]");
    if (p->cols < 1 || p->rows < 1 || (long long)p->cols * p->rows > FUSE_MAX_CELLS) return kf_fail(m, SCW, "grid size out of range (cols*rows <= 4096)");
    if (n_points < 0) return kf_fail(m, SCW, "n_points must not be negative");
    if (n_keypoints < 0 || n_keypoints >= (1 << 18)) return kf_fail(m, SCW, "n_keypoints must be in [0, 262143]");
    if (n_points > 0 && (!Px || !Py || !Pz || !Nx || !Ny || !Nz || !max_distance || !min_dist_inv || !max_dist_inv || !desc))
        return kf_fail(m, SCW, "NULL point array");
    if (n_keypoints > 0 && (!x || !y || !octave || !kf_desc)) return kf_fail(m, SCW, "NULL keyframe array");
    if ((n_points > 0 && (uintptr_t)desc % 16) || (n_keypoints > 0 && (uintptr_t)kf_desc % 16)) return kf_fail(m, SCW, "descriptors must be 16-byte aligned");
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
    if (!params) return kf_fail(m, BOW_KF, "NULL params");
    RCCHK(kf_check_sizes(m, BOW_KF, n_keyframes, n1, 1 << 18, BOW_KF_N1));
    if (n_keyframes > 0 && (!kf_start || !n_matches_dev)) return kf_fail(m, BOW_KF, "NULL kf_start or n_matches");
    LoopBowArgs a{};
    int base = 0, total = 0;
    RCCHK(kf_rebase(m, BOW_KF, kf_start, n_keyframes, a.kf_start, &base, &total));
    if (n1 > 0 && (!node1 || !valid1 || !angle1 || !desc1)) return kf_fail(m, BOW_KF, "NULL KF1 array");
    if (total > 0 && (!node2 || !valid2 || !angle2 || !desc2)) return kf_fail(m, BOW_KF, "NULL candidate array");
    if ((uintptr_t)desc1 % 16 || (uintptr_t)desc2 % 16) return kf_fail(m, BOW_KF, "descriptors must be 16-byte aligned");
    if (n_keyframes > 0 && n1 > 0 && !match12) return kf_fail(m, BOW_KF, "NULL match12");
    HIPCHK(m, hipSetDevice(m->device));
    RCCHK(reserve_sort_keys(m, n1, total));
    RCCHK(reserve_device(m, m->matched2, (size_t)std::max(total, 1), &m->matched2_cap, std::max(total, 1)));
    KfCall &c = m->call[jsorb_keyframe_matcher::BOW_KF];
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(kf_clear(m, c, st, n_keyframes, n1, total, n_matches_dev, match12, &run));
    if (!run) return JSORB_OK;
    HIPCHK(m, hipMemsetAsync(m->matched2, 0, (size_t)total, st));
    a.n1 = n1; a.valid1 = valid1; a.desc1 = desc1;
    a.n_kf = n_keyframes; a.valid2 = valid2 + base; a.desc2 = desc2 + (size_t)32 * base;
    a.p = *params;
    a.sorted1 = m->sort1; a.sorted2 = m->sort2; a.matched2 = m->matched2;
    a.match12 = match12; a.stats = c.stats;
    // the grouping: KF1 as the frame side of k_bow_group, the candidates as its keyframes
    launch_bow_group(bow_group_args(a.kf_start, node1, n1, n_keyframes, node2 + base, m->sort1, m->sort2), st);
    HIPCHK(m, hipGetLastError());
    launch_loop_bow_match(a, st);
    HIPCHK(m, hipGetLastError());
    // the rotation check: k_tri_resolve over the same rows (angle1[idx1] - angle2[match12[idx1]]), its kept bins in the same statistics words
    launch_tri_resolve(row_resolve_args(a.kf_start, n_keyframes, n1, angle1, angle2 + base, params->check_orientation, match12, n_matches_dev, c.stats + 4), st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_search_by_bow_kf(jsorb_keyframe_matcher *m, const jsorb_bow_params *params, int n1, const int32_t *node1, const uint8_t *valid1,
                           const float *angle1, const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2,
                           const uint8_t *valid2, const float *angle2, const uint8_t *desc2, int32_t *match12_host, int *n_matches_host)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(kf_check_sizes(m, BOW_KF, n_keyframes, n1, 1 << 18, BOW_KF_N1));
    return kf_sync(m, BOW_KF, m->call[jsorb_keyframe_matcher::BOW_KF], n_keyframes, n1, "n1", !n_matches_host || (n1 > 0 && !match12_host), 1, match12_host, nullptr,
                   n_matches_host, [&](int32_t *cnt, int32_t *mk, int32_t *) {
                       return jsorb_search_by_bow_kf_async(m, params, n1, node1, valid1, angle1, desc1, n_keyframes, kf_start, node2, valid2, angle2, desc2, mk, cnt);
                   });
}

int jsorb_search_by_bow_kf_stats(jsorb_keyframe_matcher *m, int *n_node_pairs, int *n_distances, int *largest_node, int kept_bins[3])
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::BOW_KF], "search_by_bow_kf_stats before jsorb_search_by_bow_kf", s));
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
    if (!n_found_dev || (n1 > 0 && (!match1 || !match12)) || (n2 > 0 && !match2)) return kf_fail(m, SIM3, "NULL output");
    HIPCHK(m, hipSetDevice(m->device));
    const int n_cells = params->cols * params->rows;
    RCCHK(reserve_grids(m, 2, n_cells, n1 + n2));
    KfCall &c = m->call[jsorb_keyframe_matcher::SIM3];
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(kf_clear(m, c, st, 1, 0, 0, n_found_dev, nullptr, &run));      // the statistics and the one count; the three arrays are written below
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
        FuseGridArgs g = fuse_grid_args(*params, s.x, s.y, m->grid_start + (size_t)d * (n_cells + 1), m->grid_items + (d ? n1 : 0));      // (the two addresses again: k's fields are pointers to const, the grid kernel writes)
        g.kf_start[1] = s.n;
        launch_fuse_grids(g, 1, st);
        HIPCHK(m, hipGetLastError());
    }
    a.match12 = match12; a.n_found = n_found_dev; a.stats = c.stats;
    launch_sim3_match(a, st);
    HIPCHK(m, hipGetLastError());
    launch_sim3_agree(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

// The synchronous form is its own, not kf_sync's: a different layout (one count, three arrays of two lengths) that comes back in one copy
int jsorb_search_by_sim3(jsorb_keyframe_matcher *m, const jsorb_sim3_params *params, const jsorb_sim3_side *side1, const jsorb_sim3_side *side2,
                         int32_t *match1_host, int32_t *match2_host, int32_t *match12_host, int *n_found)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(sim3_check(m, params, side1, side2));
    const int n1 = side1->n, n2 = side2->n;
    if (!n_found || (n1 > 0 && !match12_host)) return kf_fail(m, SIM3, "NULL host output");
    HIPCHK(m, hipSetDevice(m->device));
    const int want = 2 * n1 + n2 + 1;
    KfCall &c = m->call[jsorb_keyframe_matcher::SIM3];
    RCCHK(reserve_device(m, c.out, (size_t)want * sizeof(int32_t), &c.out_cap, want));
    int32_t *cnt = c.out, *m1 = cnt + 1, *m2 = m1 + n1, *m12 = m2 + n2;
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
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::SIM3], "search_by_sim3_stats before jsorb_search_by_sim3", s));
    if (n_windows) *n_windows = s[0];
    if (n_walked) *n_walked = s[1];
    if (n_distances) *n_distances = s[2];
    if (largest_window) *largest_window = s[3];
    if (n_agree) *n_agree = s[4];
    return JSORB_OK;
}

int jsorb_scw_build_caps(int *cap, int *lds_claims)
{
    if (cap) *cap = scw_cap();
    if (lds_claims) *lds_claims = scw_lds_claims();
    return JSORB_OK;
}

int jsorb_search_by_projection_sim3_async(jsorb_keyframe_matcher *m, const jsorb_scw_params *params, int n_points, const float *Px, const float *Py,
                                          const float *Pz, const float *Nx, const float *Ny, const float *Nz, const float *max_distance,
                                          const float *min_dist_inv, const float *max_dist_inv, const uint8_t *desc, int n_keypoints, const float *x,
                                          const float *y, const int32_t *octave, const uint8_t *kf_desc, const uint8_t *blocked, int32_t *match_kp,
                                          int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(scw_check(m, params, n_points, Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv, desc, n_keypoints, x, y, octave, kf_desc));
    if (!n_matches_dev || (n_points > 0 && (!match_kp || !match_dist)) || (n_keypoints > 0 && !kp_match)) return kf_fail(m, SCW, "NULL output");
    HIPCHK(m, hipSetDevice(m->device));
    const int n_cells = params->cols * params->rows;
    RCCHK(reserve_grids(m, 1, n_cells, n_keypoints));
    const int want = std::max(n_points, 1);
    RCCHK(reserve_device(m, m->scw.cand, (size_t)want * scw_cap() * sizeof(int), &m->scw.cand_cap, want));
    RCCHK(reserve_device(m, m->scw.cand_n, (size_t)want * sizeof(int), &m->scw.cand_n_cap, want));
    KfCall &c = m->call[jsorb_keyframe_matcher::SCW];
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(kf_clear(m, c, st, 1, 0, 0, n_matches_dev, nullptr, &run));      // the statistics and the one count; the three arrays are written below
    if (n_points == 0 || n_keypoints == 0) {        // nothing to search, or nothing to search in: everything is -1 / 0
        if (n_points > 0) {
            HIPCHK(m, hipMemsetAsync(match_kp, 0xff, (size_t)n_points * sizeof(int32_t), st));
            HIPCHK(m, hipMemsetAsync(match_dist, 0xff, (size_t)n_points * sizeof(int32_t), st));
        }
        if (n_keypoints > 0) HIPCHK(m, hipMemsetAsync(kp_match, 0xff, (size_t)n_keypoints * sizeof(int32_t), st));
        return JSORB_OK;
    }
    // the keyframe's grid: k_fuse_grids over one keyframe
    FuseGridArgs g = fuse_grid_args(*params, x, y, m->grid_start, m->grid_items);
    g.kf_start[1] = n_keypoints;
    launch_fuse_grids(g, 1, st);
    HIPCHK(m, hipGetLastError());
    ScwArgs a{};
    a.p = *params;
    a.n_points = n_points; a.Px = Px; a.Py = Py; a.Pz = Pz; a.Nx = Nx; a.Ny = Ny; a.Nz = Nz;
    a.max_distance = max_distance; a.min_dist_inv = min_dist_inv; a.max_dist_inv = max_dist_inv; a.mp_desc = desc;
    a.n_kp = n_keypoints; a.x = x; a.y = y; a.octave = octave; a.kf_desc = kf_desc; a.blocked = blocked;
    a.cell_start = m->grid_start; a.cell_items = m->grid_items;
    a.cand = m->scw.cand; a.cand_n = m->scw.cand_n;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev; a.stats = c.stats;
    launch_scw_candidates(a, st);
    HIPCHK(m, hipGetLastError());
    launch_scw_resolve(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

// The synchronous form, in the manner of jsorb_search_by_sim3: one count and three arrays of two lengths that come back in one copy
int jsorb_search_by_projection_sim3(jsorb_keyframe_matcher *m, const jsorb_scw_params *params, int n_points, const float *Px, const float *Py,
                                    const float *Pz, const float *Nx, const float *Ny, const float *Nz, const float *max_distance,
                                    const float *min_dist_inv, const float *max_dist_inv, const uint8_t *desc, int n_keypoints, const float *x,
                                    const float *y, const int32_t *octave, const uint8_t *kf_desc, const uint8_t *blocked, int32_t *match_kp_host,
                                    int32_t *match_dist_host, int32_t *kp_match_host, int *n_matches)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(scw_check(m, params, n_points, Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv, desc, n_keypoints, x, y, octave, kf_desc));
    if (!n_matches || (n_points > 0 && !match_kp_host)) return kf_fail(m, SCW, "NULL host output");
    HIPCHK(m, hipSetDevice(m->device));
    const int want = 2 * n_points + n_keypoints + 1;
    KfCall &c = m->call[jsorb_keyframe_matcher::SCW];
    RCCHK(reserve_device(m, c.out, (size_t)want * sizeof(int32_t), &c.out_cap, want));
    int32_t *cnt = c.out, *mk = cnt + 1, *md = mk + n_points, *km = md + n_points;
    RCCHK(jsorb_search_by_projection_sim3_async(m, params, n_points, Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv, desc, n_keypoints, x,
                                                y, octave, kf_desc, blocked, mk, md, km, cnt));
    std::vector<int32_t> h((size_t)want);            // the count and the three arrays lie next to each other: one copy
    HIPCHK(m, hipMemcpyAsync(h.data(), cnt, (size_t)want * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    *n_matches = h[0];
    if (n_points > 0) memcpy(match_kp_host, h.data() + 1, (size_t)n_points * sizeof(int32_t));
    if (n_points > 0 && match_dist_host) memcpy(match_dist_host, h.data() + 1 + n_points, (size_t)n_points * sizeof(int32_t));
    if (n_keypoints > 0 && kp_match_host) memcpy(kp_match_host, h.data() + 1 + 2 * n_points, (size_t)n_keypoints * sizeof(int32_t));
    return JSORB_OK;
}

int jsorb_search_by_projection_sim3_stats(jsorb_keyframe_matcher *m, int *rounds, int *n_kept, int *n_overflow, int *n_windows, int *n_distances,
                                          int *largest_window)
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::SCW], "search_by_projection_sim3_stats before jsorb_search_by_projection_sim3", s));
    int *out[6] = {rounds, n_kept, n_overflow, n_windows, n_distances, largest_window};
    for (int i = 0; i < 6; i++)
        if (out[i]) *out[i] = s[i];
    return JSORB_OK;
}

} // extern "C"
