// jsorb_keyframes.hip - host side of the keyframe matcher of LocalMapping (jsorb_keyframe_matcher_*, jsorb_search_for_triangulation*, jsorb_fuse*);
// LoopClosing's calls on the same kind of matcher are in jsorb_loop.hip, the map points' distinctive descriptors in jsorb_mappoints.hip.
// The matcher belongs to no extractor handle: it owns its stream and scratch, so LocalMapping's thread never enqueues on Tracking's handles.  The
// kernels are in k_triangulate.hip (the grouping is k_bow.hip's k_bow_group with KF1 as the frame side) and k_fuse.hip.  The checks on sizes and
// kf_start, the start of the device work and the synchronous forms are jsorb_handle.h's frames (kf_check_sizes, kf_rebase, kf_clear, kf_sync).
#include "jsorb_handle.h"      // struct jsorb_keyframe_matcher: shared with jsorb_loop.hip

namespace {

const char *const TRI = "search_for_triangulation", *const TRI_N1 = "n1 must be in [0, 262143]";
const char *const FUSE = "fuse", *const FUSE_N = "n_points must not be negative";

} // namespace

extern "C" {

int jsorb_keyframe_matcher_create(int device_id, jsorb_keyframe_matcher **out)
{
    if (!out) return JSORB_ERR_INVALID;
    *out = nullptr;
    if (device_id < 0) return JSORB_ERR_INVALID;
    jsorb_keyframe_matcher *m = new (std::nothrow) jsorb_keyframe_matcher;
    if (!m) return JSORB_ERR_HIP;
    m->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&m->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev_switch, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (m->ev_switch) (void)hipEventDestroy(m->ev_switch);
        if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
        delete m;
        return JSORB_ERR_HIP;
    }
    m->stream = m->own_stream;
    *out = m;
    return JSORB_OK;
}

void jsorb_keyframe_matcher_destroy(jsorb_keyframe_matcher *m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipStreamSynchronize(m->stream);
    free_device(m->sort1, m->sort2, m->grid_start, m->grid_items, m->matched2, m->scw.cand, m->scw.cand_n, m->distinct.list, m->covis.row.word, m->covis.slot, m->cull.p, m->fmap.p, m->npts.p, m->staging.p);
    for (KfCall &c : m->call) free_device(c.stats, c.out);
    destroy_event(m->ev_switch);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    delete m;
}

int jsorb_keyframe_matcher_set_stream(jsorb_keyframe_matcher *m, void *hip_stream)
{
    if (!m) return JSORB_ERR_INVALID;
    hipStream_t ns = hip_stream ? (hipStream_t)hip_stream : m->own_stream;
    if (ns != m->stream && std::any_of(std::begin(m->call), std::end(m->call), [](const KfCall &c) { return c.done; })) {               // the new stream continues after what the old one still carries (it reads the same scratch)
        HIPCHK(m, hipSetDevice(m->device));
        HIPCHK(m, hipEventRecord(m->ev_switch, m->stream));
        HIPCHK(m, hipStreamWaitEvent(ns, m->ev_switch, 0));
    }
    m->stream = ns;
    return JSORB_OK;
}
void *jsorb_keyframe_matcher_get_stream(const jsorb_keyframe_matcher *m) { return m ? (void *)m->stream : nullptr; }
const char *jsorb_keyframe_matcher_last_error(const jsorb_keyframe_matcher *m) { return m ? m->err.c_str() : "NULL matcher"; }

int jsorb_search_for_triangulation_async(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, int n1, const int32_t *node1,
                                         const uint8_t *free1, const uint8_t *stereo1, const float *x1, const float *y1, const float *angle1,
                                         const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2, const uint8_t *free2,
                                         const uint8_t *stereo2, const float *x2, const float *y2, const int32_t *octave2, const float *angle2,
                                         const uint8_t *desc2, const float *F12, const float *epipole, int32_t *match12, int32_t *n_matches_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!params) return kf_fail(m, TRI, "NULL params");
    if (params->n_levels < 1 || params->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, TRI, "n_levels out of range");
    RCCHK(kf_check_sizes(m, TRI, n_keyframes, n1, 1 << 18, TRI_N1));
    if (n_keyframes > 0 && (!kf_start || !n_matches_dev || !F12 || !epipole)) return kf_fail(m, TRI, "NULL kf_start, F12, epipole or n_matches");
    TriArgs a{};
    int base = 0, total = 0;
    RCCHK(kf_rebase(m, TRI, kf_start, n_keyframes, a.kf_start, &base, &total));
    if (n1 > 0 && (!node1 || !free1 || !stereo1 || !x1 || !y1 || !angle1 || !desc1)) return kf_fail(m, TRI, "NULL KF1 array");
    if (total > 0 && (!node2 || !free2 || !stereo2 || !x2 || !y2 || !octave2 || !angle2 || !desc2)) return kf_fail(m, TRI, "NULL KF2 array");
    if ((uintptr_t)desc1 % 16 || (uintptr_t)desc2 % 16) return kf_fail(m, TRI, "descriptors must be 16-byte aligned");
    if (n_keyframes > 0 && n1 > 0 && !match12) return kf_fail(m, TRI, "NULL match12");
    HIPCHK(m, hipSetDevice(m->device));
    RCCHK(reserve_sort_keys(m, n1, total));
    KfCall &c = m->call[jsorb_keyframe_matcher::TRIANGULATION];
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(kf_clear(m, c, st, n_keyframes, n1, total, n_matches_dev, match12, &run));
    if (!run) return JSORB_OK;
    // the grouping: KF1 as the frame side of k_bow_group, the KF2s as its keyframes
    const BowMatchArgs b = bow_group_args(a.kf_start, node1, n1, n_keyframes, node2 + base, m->sort1, m->sort2);
    a.n1 = n1; a.free1 = free1; a.stereo1 = stereo1; a.x1 = x1; a.y1 = y1; a.desc1 = desc1;
    a.n_kf = n_keyframes;
    a.free2 = free2 + base; a.stereo2 = stereo2 + base; a.x2 = x2 + base; a.y2 = y2 + base; a.octave2 = octave2 + base;
    a.desc2 = desc2 + (size_t)32 * base;
    a.th_low = params->th_low; a.only_stereo = params->only_stereo; a.n_levels = params->n_levels;
    for (int l = 0; l < params->n_levels; l++) {
        a.gate[l] = 100.0f * params->scale_factor[l];            // :734, one float product
        a.line[l] = 3.84 * (double)params->level_sigma2[l];      // :143, the double product of the promoted comparison
    }
    a.sorted1 = m->sort1; a.sorted2 = m->sort2;
    a.match12 = match12; a.stats = c.stats;
    launch_bow_group(b, st);
    HIPCHK(m, hipGetLastError());
    for (int k0 = 0; k0 < n_keyframes; k0 += TR_KF_CHUNK) {
        TriGeom g{};
        g.kf0 = k0; g.n = std::min(TR_KF_CHUNK, n_keyframes - k0);
        for (int i = 0; i < g.n; i++) {
            memcpy(g.f[i], F12 + 9 * (size_t)(k0 + i), 9 * sizeof(float));
            g.f[i][9] = epipole[2 * (size_t)(k0 + i)];
            g.f[i][10] = epipole[2 * (size_t)(k0 + i) + 1];
        }
        launch_tri_match(a, g, st);
        HIPCHK(m, hipGetLastError());
    }
    launch_tri_resolve(row_resolve_args(a.kf_start, n_keyframes, n1, angle1, angle2 + base, params->check_orientation, match12, n_matches_dev, c.stats + 4), st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_search_for_triangulation(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, int n1, const int32_t *node1,
                                   const uint8_t *free1, const uint8_t *stereo1, const float *x1, const float *y1, const float *angle1,
                                   const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2, const uint8_t *free2,
                                   const uint8_t *stereo2, const float *x2, const float *y2, const int32_t *octave2, const float *angle2,
                                   const uint8_t *desc2, const float *F12, const float *epipole, int32_t *match12_host, int *n_matches_host)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(kf_check_sizes(m, TRI, n_keyframes, n1, 1 << 18, TRI_N1));
    return kf_sync(m, TRI, m->call[jsorb_keyframe_matcher::TRIANGULATION], n_keyframes, n1, "n1", !n_matches_host || (n1 > 0 && !match12_host), 1, match12_host,
                   nullptr, n_matches_host, [&](int32_t *cnt, int32_t *mk, int32_t *) {
                       return jsorb_search_for_triangulation_async(m, params, n1, node1, free1, stereo1, x1, y1, angle1, desc1, n_keyframes, kf_start, node2, free2,
                                                                   stereo2, x2, y2, octave2, angle2, desc2, F12, epipole, mk, cnt);
                   });
}

int jsorb_search_for_triangulation_stats(jsorb_keyframe_matcher *m, int *n_node_pairs, int *n_distances, int *n_line_tests, int *largest_node,
                                         int kept_bins[3])
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::TRIANGULATION], "search_for_triangulation_stats before jsorb_search_for_triangulation", s));
    if (n_node_pairs) *n_node_pairs = s[0];
    if (n_distances) *n_distances = s[1];
    if (n_line_tests) *n_line_tests = s[2];
    if (largest_node) *largest_node = s[3];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[4 + b] - 1;
    return JSORB_OK;
}

int jsorb_fuse_async(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int n_points, const float *Px, const float *Py, const float *Pz,
                     const float *Nx, const float *Ny, const float *Nz, const float *max_distance, const float *min_dist_inv,
                     const float *max_dist_inv, const uint8_t *desc, int n_keyframes, const int32_t *kf_start, const float *x, const float *y,
                     const int32_t *octave, const float *uright, const uint8_t *kf_desc, const float *Rcw, const float *tcw, const float *Ow,
                     const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, int32_t *n_matched_dev)
{
    if (!m) return JSORB_ERR_INVALID;
    if (!params) return kf_fail(m, FUSE, "NULL params");
    if (params->n_levels < 1 || params->n_levels > JSORB_MAX_LEVELS) return kf_fail(m, FUSE, "n_levels out of range");
    if (params->th_low < 0 || params->th_low > 255) return kf_fail(m, FUSE, "th_low must be in [0, 255]");
    if (params->cols < 1 || params->rows < 1 || (long long)params->cols * params->rows > FUSE_MAX_CELLS) return kf_fail(m, FUSE, "grid size out of range (cols*rows <= 4096)");
    RCCHK(kf_check_sizes(m, FUSE, n_keyframes, n_points, 0, FUSE_N));
    if (n_keyframes > 0 && (!kf_start || !n_matched_dev || !Rcw || !tcw || !Ow)) return kf_fail(m, FUSE, "NULL kf_start, Rcw, tcw, Ow or n_matched");
    int rel[JSORB_BOW_MAX_KEYFRAMES + 1] = {0}, base = 0, total = 0;
    RCCHK(kf_rebase(m, FUSE, kf_start, n_keyframes, rel, &base, &total));
    if (total >= (1 << 18)) return kf_fail(m, FUSE, "the keyframes of a call must hold fewer than 262144 keypoints");
    if ((long long)n_keyframes * n_points > (long long)INT_MAX - JSORB_BOW_MAX_KEYFRAMES) return kf_fail(m, FUSE, "n_keyframes x n_points too large", JSORB_ERR_UNSUPPORTED);
    if (n_points > 0 && (!Px || !Py || !Pz || !Nx || !Ny || !Nz || !max_distance || !min_dist_inv || !max_dist_inv || !desc)) return kf_fail(m, FUSE, "NULL point array");
    if (total > 0 && (!x || !y || !octave || !kf_desc)) return kf_fail(m, FUSE, "NULL keyframe array");
    if ((uintptr_t)desc % 16 || (uintptr_t)kf_desc % 16) return kf_fail(m, FUSE, "descriptors must be 16-byte aligned");
    if (n_keyframes > 0 && n_points > 0 && (!best_idx || !best_dist)) return kf_fail(m, FUSE, "NULL best_idx or best_dist");
    HIPCHK(m, hipSetDevice(m->device));
    RCCHK(reserve_grids(m, std::max(n_keyframes, 1), params->cols * params->rows, total));
    KfCall &c = m->call[jsorb_keyframe_matcher::FUSE];
    hipStream_t st = m->stream;
    bool run = false;
    RCCHK(kf_clear(m, c, st, n_keyframes, 0, 0, n_matched_dev, nullptr, &run));      // (every best_idx / best_dist entry is written: no rows to clear)
    if (n_keyframes == 0 || n_points == 0) return JSORB_OK;
    FuseGridArgs g = fuse_grid_args(*params, x + base, y + base, m->grid_start, m->grid_items);
    memcpy(g.kf_start, rel, sizeof(g.kf_start));
    launch_fuse_grids(g, n_keyframes, st);
    HIPCHK(m, hipGetLastError());
    FuseArgs a{};
    a.p = *params;
    a.n_points = n_points;
    a.Px = Px; a.Py = Py; a.Pz = Pz; a.Nx = Nx; a.Ny = Ny; a.Nz = Nz;
    a.max_distance = max_distance; a.min_dist_inv = min_dist_inv; a.max_dist_inv = max_dist_inv; a.mp_desc = desc;
    a.x = g.x; a.y = g.y; a.uright = uright ? uright + base : nullptr; a.octave = octave + base; a.kf_desc = kf_desc + (size_t)32 * base;
    a.skip = skip;
    a.cell_start = m->grid_start; a.cell_items = m->grid_items;
    a.best_idx = best_idx; a.best_dist = best_dist; a.n_matched = n_matched_dev; a.stats = c.stats;
    for (int k0 = 0; k0 < n_keyframes; k0 += FUSE_KF_CHUNK) {
        FusePose q{};
        q.kf0 = k0; q.n = std::min(FUSE_KF_CHUNK, n_keyframes - k0);
        for (int i = 0; i <= q.n; i++) q.start[i] = g.kf_start[k0 + i];
        for (int i = 0; i < q.n; i++) {
            memcpy(q.pose[i], Rcw + 9 * (size_t)(k0 + i), 9 * sizeof(float));
            memcpy(q.pose[i] + 9, tcw + 3 * (size_t)(k0 + i), 3 * sizeof(float));
            memcpy(q.pose[i] + 12, Ow + 3 * (size_t)(k0 + i), 3 * sizeof(float));
        }
        launch_fuse_match(a, q, st);
        HIPCHK(m, hipGetLastError());
    }
    return JSORB_OK;
}

int jsorb_fuse(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int n_points, const float *Px, const float *Py, const float *Pz,
               const float *Nx, const float *Ny, const float *Nz, const float *max_distance, const float *min_dist_inv, const float *max_dist_inv,
               const uint8_t *desc, int n_keyframes, const int32_t *kf_start, const float *x, const float *y, const int32_t *octave,
               const float *uright, const uint8_t *kf_desc, const float *Rcw, const float *tcw, const float *Ow, const uint8_t *skip,
               int32_t *best_idx_host, int32_t *best_dist_host, int *n_matched_host)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(kf_check_sizes(m, FUSE, n_keyframes, n_points, 0, FUSE_N));
    return kf_sync(m, FUSE, m->call[jsorb_keyframe_matcher::FUSE], n_keyframes, n_points, "n_points",
                   !n_matched_host || (n_points > 0 && (!best_idx_host || !best_dist_host)), 2, best_idx_host, best_dist_host, n_matched_host,
                   [&](int32_t *cnt, int32_t *bi, int32_t *bd) {
                       return jsorb_fuse_async(m, params, n_points, Px, Py, Pz, Nx, Ny, Nz, max_distance, min_dist_inv, max_dist_inv, desc, n_keyframes, kf_start,
                                               x, y, octave, uright, kf_desc, Rcw, tcw, Ow, skip, bi, bd, cnt);
                   });
}

int jsorb_fuse_stats(jsorb_keyframe_matcher *m, int *n_windows, int *n_walked, int *n_distances, int *largest_window)
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::FUSE], "fuse_stats before jsorb_fuse", s));
    if (n_windows) *n_windows = s[0];
    if (n_walked) *n_walked = s[1];
    if (n_distances) *n_distances = s[2];
    if (largest_window) *largest_window = s[3];
    return JSORB_OK;
}

} // extern "C"
