// jsorb_search.hip - host side of the four grid matchers of Tracking: local-map search (k_search_local.hip), motion-model search
// (k_search_last.hip), keyframe-projection search (k_search_kf.hip) and monocular-initialisation search (k_search_init.hip).  Every call bins the
// image's keypoints into the caller's grid (k_assign_grid) and matches over it on the handle's main stream.  What the four share is here once:
// the checks of an entry point (search_check, search_begin), the frame view and the grid launch (search_begin), the synchronous forms' end
// (search_sync) and the statistics reader (read_stats, jsorb_handle.h).  Each entry point keeps its own checks and its own argument block.
#include "jsorb_handle.h"

namespace jsorb_host __attribute__((visibility("hidden"))) {

void search_local_release(jsorb_extractor *e) { free_device(e->sl.cand, e->sl.stats, e->sl.out); }
void search_last_release(jsorb_extractor *e) { free_device(e->lf.ws, e->lf.pts, e->lf.out); }
void search_init_release(jsorb_extractor *e) { free_device(e->si.cand, e->si.ws, e->si.out, e->si.ref); }
void search_kf_release(jsorb_extractor *e) { free_device(e->kf.cand, e->kf.stats, e->kf.out); }

} // namespace jsorb_host

namespace {

int fail(jsorb_extractor *e, const char *name, const char *what, int rc = JSORB_ERR_INVALID)
{
    e->err = std::string(name) + ": " + what;
    return rc;
}

// The first checks of an asynchronous entry point, in the order they fire: the handle, the image, the parameters and the grid size.  P is the
// matcher's parameter struct (cols, rows).
template <class P> int search_check(jsorb_extractor *e, const char *name, int image, const P *params, const void *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return fail(e, name, "no extract result for this image", JSORB_ERR_STATE);
    if (!params || !n_matches_dev) return fail(e, name, "NULL params or n_matches");
    if (params->cols < 1 || params->rows < 1 || (long long)params->cols * params->rows > 16384) return fail(e, name, "grid size out of range (cols*rows <= 16384)");
    return JSORB_OK;
}

// the points of a call as the shared checks see them
struct SearchPoints {
    int n;
    const char *n_name;                // "n_points" / "n1" in the error text
    bool null_arrays;                  // n > 0 and one of the point arrays or per-point outputs is NULL
    const char *null_text;
    bool has_kp_match;                 // (a matcher without a kp_match output: true)
    const void *descs;                 // the points' descriptors and their name in the alignment error
    const char *descs_name;
};

// The rest of the prologue, behind an entry point's own parameter checks: the checks on the points, then the device, the grid CSR, the order
// behind the lanes of a batch, k_assign_grid over the caller's grid (P: min_x, min_y, inv_w, inv_h, cols, rows) and the frame view.
template <class P>
int search_begin(jsorb_extractor *e, const char *name, int image, const P &p, const SearchPoints &q, const float *u_right, const uint8_t *blocked, FrameView &f)
{
    if (q.n < 0) return fail(e, name, (std::string(q.n_name) + " < 0").c_str());
    const int n = jsorb_n_keypoints(e, image);
    if (n >= (1 << 18)) return fail(e, name, "more than 262143 keypoints", JSORB_ERR_UNSUPPORTED);
    if (q.null_arrays) return fail(e, name, q.null_text);
    if (n > 0 && !q.has_kp_match) return fail(e, name, "NULL kp_match");
    if ((uintptr_t)q.descs % 16) return fail(e, name, (std::string(q.descs_name) + " must be 16-byte aligned").c_str());
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(grid_reserve(e, p.cols * p.rows));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the frame (and its uRight) may come from the lanes of a batch
    mark_main_stream(e);               // ... and the next batch's lanes must not rewrite it before these kernels have read it
    f = FrameView{};
    f.soa = jsorb_keypoints_device(e, image);
    f.xy_un = jsorb_keypoints_un_device(e, image);
    f.desc = jsorb_descriptors_device(e, image);
    f.u_right = u_right;
    f.blocked = blocked;
    f.n_kp = n;
    f.cell_start = e->grid.start;
    f.cell_items = e->grid.items;
    f.n_levels = e->g.L;
    for (int l = 0; l < e->g.L; l++) f.scale[l] = e->g.lv[l].scale;
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(f.soa, f.xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows, e->grid.start, e->grid.items, st));
    HIPCHK(e, hipGetLastError());
    return JSORB_OK;
}

// The synchronous form of a matcher whose result is kp_match: the handle's buffer `out` (grown with the points) as count, kp_match (T),
// match_kp, match_dist (out_points each); run(match_kp, match_dist, kp_match, count) is the asynchronous form; count and kp_match come back in
// one copy.
template <class Run>
int search_sync(jsorb_extractor *e, const char *name, int image, int n_points, int32_t *&out, int &out_points, int32_t *kp_match_host, int *n_matches, Run run)
{
    if (!n_matches) return fail(e, name, "NULL n_matches");
    if (n_points < 0) return fail(e, name, "n_points < 0");
    if (!check_image(e, image)) return fail(e, name, "no extract result for this image", JSORB_ERR_STATE);
    const int N = jsorb_n_keypoints(e, image);
    if (N > 0 && !kp_match_host) return fail(e, name, "NULL host output");
    HIPCHK(e, hipSetDevice(e->device));
    const int pts = std::max(n_points, 1);
    RCCHK(reserve_device(e, out, ((size_t)2 * pts + e->g.T + 1) * sizeof(int32_t), &out_points, pts));
    int32_t *cnt = out, *km = cnt + 1, *mk = km + e->g.T, *md = mk + out_points;
    RCCHK(run(mk, md, km, cnt));
    std::vector<int32_t> h((size_t)N + 1);
    HIPCHK(e, hipMemcpyAsync(h.data(), cnt, ((size_t)N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *n_matches = h[0];
    if (N > 0) memcpy(kp_match_host, h.data() + 1, (size_t)N * sizeof(int32_t));
    return JSORB_OK;
}

#define SEARCH_STATS 8             // control / statistics words of a matcher (k_last_resolve's ctl, the stats of the others)

} // namespace

extern "C" {

// ---- local map matching: ORBmatcher::SearchByProjection(Frame&, map points, th) (ORBmatcher.cpp:32-116), k_search_local.hip ----
int jsorb_search_local_points_async(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                                    const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                                    const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp,
                                    int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    const char *name = "search_local_points";
    RCCHK(search_check(e, name, image, params, n_matches_dev));
    const jsorb_search_params &p = *params;
    const bool nulls = n_points > 0 && (!u || !v || !invz || !predicted_level || !view_cos || !in_frustum || !mp_descriptors || !match_kp || !match_dist);
    SearchLocalArgs a{};
    RCCHK(search_begin(e, name, image, p, SearchPoints{n_points, "n_points", nulls, "NULL point array or output", kp_match != nullptr, mp_descriptors, "mp_descriptors"},
                       u_right, blocked_in, a.f));
    const int cap = search_local_cap();
    RCCHK(reserve_device(e, e->sl.cand, (size_t)n_points * (cap + 1) * sizeof(int), &e->sl.points, n_points));
    RCCHK(reserve_device(e, e->sl.stats, 4 * sizeof(int)));
    a.min_x = p.min_x; a.min_y = p.min_y; a.inv_w = p.inv_w; a.inv_h = p.inv_h;
    a.cols = p.cols; a.rows = p.rows;
    a.n_points = n_points;
    a.u = u; a.v = v; a.invz = invz; a.view_cos = view_cos; a.level = predicted_level; a.in_frustum = in_frustum; a.mp_desc = mp_descriptors;
    a.th = p.th; a.nn_ratio = p.nn_ratio; a.mbf = p.mbf; a.th_high = p.th_high;
    a.cand = e->sl.cand;
    a.cand_n = e->sl.cand + (size_t)e->sl.points * cap;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    a.stats = e->sl.stats;
    TIMED(e, JSORB_K_LOCAL_CANDIDATES, launch_local_candidates(a, e->stream));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_LOCAL_RESOLVE, launch_local_resolve(a, e->stream));
    HIPCHK(e, hipGetLastError());
    e->sl.done = true;
    return JSORB_OK;
}

// (match_kp and the count from the layout match_kp, match_dist, kp_match, count: not search_sync's, whose result is kp_match)
int jsorb_search_local_points(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                              const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                              const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp_host, int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!n_matches || (n_points > 0 && !match_kp_host)) { e->err = "search_local_points: NULL host output"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_local_points: n_points < 0"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int pts = std::max(n_points, 1);
    RCCHK(reserve_device(e, e->sl.out, ((size_t)2 * pts + e->g.T + 1) * sizeof(int32_t), &e->sl.out_points, pts));
    int32_t *mk = e->sl.out, *md = mk + e->sl.out_points, *km = md + e->sl.out_points, *cnt = km + e->g.T;
    RCCHK(jsorb_search_local_points_async(e, image, params, n_points, u, v, invz, predicted_level, view_cos, in_frustum, mp_descriptors, u_right,
                                blocked_in, mk, md, km, cnt));
    int32_t count = 0;
    HIPCHK(e, hipMemcpyAsync(&count, cnt, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (n_points > 0) HIPCHK(e, hipMemcpyAsync(match_kp_host, mk, (size_t)n_points * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *n_matches = count;
    return JSORB_OK;
}

int jsorb_search_local_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow)
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[3] = {0, 0, 0};
    RCCHK(read_stats(e, e->sl.done, "search_local_stats before jsorb_search_local_points", e->sl.stats, s, 3));
    if (rounds) *rounds = s[0];
    if (n_candidates) *n_candidates = s[1];
    if (n_overflow) *n_overflow = s[2];
    return JSORB_OK;
}

// ---- motion-model matching: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cpp:1647-1963), k_search_last.hip ----
// (SEARCH_STATS control and statistics words behind the owner array: run the second pass, passes, candidates, ind1..3)
int jsorb_search_last_frame_async(jsorb_extractor *e, int image, const jsorb_last_frame_params *params, int n_points, const float *Px, const float *Py,
                                  const float *Pz, const int32_t *last_octave, const float *last_angle, const uint8_t *mp_descriptors,
                                  const float *u_right, int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    const char *name = "search_last_frame";
    RCCHK(search_check(e, name, image, params, n_matches_dev));
    const jsorb_last_frame_params &p = *params;
    if (p.direction < -1 || p.direction > 1) return fail(e, name, "direction must be -1, 0 or 1");
    const bool nulls = n_points > 0 && (!Px || !Py || !Pz || !last_octave || !last_angle || !mp_descriptors || !match_kp || !match_dist);
    LastFrameArgs a{};
    RCCHK(search_begin(e, name, image, p, SearchPoints{n_points, "n_points", nulls, "NULL point array or output", kp_match != nullptr, mp_descriptors, "mp_descriptors"},
                       u_right, nullptr, a.f));
    hipStream_t st = e->stream;
    if (!e->lf.ws) {                   // owner starts at -1; afterwards every k_last_resolve leaves it so
        RCCHK(reserve_device(e, e->lf.ws, ((size_t)e->g.T + SEARCH_STATS) * sizeof(int)));
        HIPCHK(e, hipMemsetAsync(e->lf.ws, 0xff, ((size_t)e->g.T + SEARCH_STATS) * sizeof(int), st));
    }
    RCCHK(reserve_device(e, e->lf.pts, (size_t)2 * std::max(n_points, 1) * sizeof(int), &e->lf.points, std::max(n_points, 1)));
    a.n_points = n_points;
    a.Px = Px; a.Py = Py; a.Pz = Pz; a.angle = last_angle; a.octave = last_octave; a.mp_desc = mp_descriptors;
    a.p = p;
    a.owner = e->lf.ws;
    a.ctl = e->lf.ws + e->g.T;
    a.bin = e->lf.pts;
    a.cand = e->lf.pts + e->lf.points;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    // the second pass is enqueued whenever it may be needed; its kernels return at once when the first pass's count says so
    for (int pass = 0; pass < (p.retry_below > 0 ? 2 : 1); pass++) {
        TIMED(e, JSORB_K_LAST_MATCH, launch_last_match(a, pass, st));
        HIPCHK(e, hipGetLastError());
        TIMED(e, JSORB_K_LAST_RESOLVE, launch_last_resolve(a, pass, st));
        HIPCHK(e, hipGetLastError());
    }
    e->lf.done = true;
    return JSORB_OK;
}

int jsorb_search_last_frame(jsorb_extractor *e, int image, const jsorb_last_frame_params *params, int n_points, const float *Px, const float *Py,
                            const float *Pz, const int32_t *last_octave, const float *last_angle, const uint8_t *mp_descriptors, const float *u_right,
                            int32_t *kp_match_host, int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    return search_sync(e, "search_last_frame", image, n_points, e->lf.out, e->lf.out_points, kp_match_host, n_matches,
                       [&](int32_t *mk, int32_t *md, int32_t *km, int32_t *cnt) {
                           return jsorb_search_last_frame_async(e, image, params, n_points, Px, Py, Pz, last_octave, last_angle, mp_descriptors, u_right, mk, md, km, cnt);
                       });
}

int jsorb_search_last_frame_stats(jsorb_extractor *e, int *passes, int *n_candidates, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[SEARCH_STATS] = {0};
    RCCHK(read_stats(e, e->lf.done, "search_last_frame_stats before jsorb_search_last_frame", e->lf.ws + e->g.T, s, SEARCH_STATS));
    if (passes) *passes = s[1];
    if (n_candidates) *n_candidates = s[2];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[3 + b];
    return JSORB_OK;
}

// ---- relocalisation matching: ORBmatcher::SearchByProjection(CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1968-2095), k_search_kf.hip ----
// (statistics words: rounds, candidates, overflowed points, ind1..3)
int jsorb_search_by_projection_kf_async(jsorb_extractor *e, int image, const jsorb_kf_projection_params *params, int n_points, const float *Px,
                                        const float *Py, const float *Pz, const float *max_distance, const float *max_dist_inv,
                                        const float *min_dist_inv, const float *kf_angle, const uint8_t *mp_descriptors, const uint8_t *blocked_in,
                                        int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    const char *name = "search_by_projection_kf";
    RCCHK(search_check(e, name, image, params, n_matches_dev));
    const bool nulls = n_points > 0 && (!Px || !Py || !Pz || !max_distance || !max_dist_inv || !min_dist_inv || !kf_angle || !mp_descriptors || !match_kp || !match_dist);
    SearchKfArgs a{};
    RCCHK(search_begin(e, name, image, *params, SearchPoints{n_points, "n_points", nulls, "NULL point array or output", kp_match != nullptr, mp_descriptors, "mp_descriptors"},
                       nullptr, blocked_in, a.f));
    const int cap = search_kf_cap(), pts = std::max(n_points, 1);
    RCCHK(reserve_device(e, e->kf.cand, (size_t)pts * (cap + 1) * sizeof(int), &e->kf.points, pts));
    RCCHK(reserve_device(e, e->kf.stats, SEARCH_STATS * sizeof(int)));
    a.n_points = n_points;
    a.Px = Px; a.Py = Py; a.Pz = Pz; a.max_distance = max_distance; a.max_dist_inv = max_dist_inv; a.min_dist_inv = min_dist_inv;
    a.angle = kf_angle; a.mp_desc = mp_descriptors;
    a.p = *params;
    a.cand = e->kf.cand;
    a.cand_n = e->kf.cand + (size_t)e->kf.points * cap;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    a.stats = e->kf.stats;
    TIMED(e, JSORB_K_KF_CANDIDATES, launch_kf_candidates(a, e->stream));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_KF_RESOLVE, launch_kf_resolve(a, e->stream));
    HIPCHK(e, hipGetLastError());
    e->kf.done = true;
    return JSORB_OK;
}

int jsorb_search_by_projection_kf(jsorb_extractor *e, int image, const jsorb_kf_projection_params *params, int n_points, const float *Px,
                                  const float *Py, const float *Pz, const float *max_distance, const float *max_dist_inv, const float *min_dist_inv,
                                  const float *kf_angle, const uint8_t *mp_descriptors, const uint8_t *blocked_in, int32_t *kp_match_host,
                                  int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    return search_sync(e, "search_by_projection_kf", image, n_points, e->kf.out, e->kf.out_points, kp_match_host, n_matches,
                       [&](int32_t *mk, int32_t *md, int32_t *km, int32_t *cnt) {
                           return jsorb_search_by_projection_kf_async(e, image, params, n_points, Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle,
                                                                      mp_descriptors, blocked_in, mk, md, km, cnt);
                       });
}

int jsorb_search_by_projection_kf_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[SEARCH_STATS] = {0};
    RCCHK(read_stats(e, e->kf.done, "search_by_projection_kf_stats before jsorb_search_by_projection_kf", e->kf.stats, s, SEARCH_STATS));
    if (rounds) *rounds = s[0];
    if (n_candidates) *n_candidates = s[1];
    if (n_overflow) *n_overflow = s[2];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[3 + b];
    return JSORB_OK;
}

int jsorb_search_kf_build_caps(int *list_cap, int *lds_claims)
{
    if (list_cap) *list_cap = search_kf_cap();
    if (lds_claims) *lds_claims = search_kf_lds_claims();
    return JSORB_OK;
}

// ---- monocular initialisation matching: ORBmatcher::SearchForInitialization (ORBmatcher.cpp:392-507), k_search_init.hip ----
// (statistics words behind state and owner: rounds, candidates, overflowed points, displaced claims, ind1..3)
int jsorb_search_for_initialization_async(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave,
                                          const float *f1_angle, const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12,
                                          int32_t *matches21, int32_t *n_matches_dev)
{
    const char *name = "search_for_initialization";
    RCCHK(search_check(e, name, image, params, n_matches_dev));
    const bool nulls = n1 > 0 && (!f1_octave || !f1_angle || !f1_descriptors || !prev_matched || !matches12);
    SearchInitArgs a{};
    RCCHK(search_begin(e, name, image, *params, SearchPoints{n1, "n1", nulls, "NULL F1 array or output", true, f1_descriptors, "f1_descriptors"}, nullptr, nullptr, a.f));
    const int cap = search_init_cap(), pts = std::max(n1, 1);
    const size_t T = (size_t)e->g.T;
    RCCHK(reserve_device(e, e->si.cand, (size_t)pts * (cap + 2) * sizeof(int), &e->si.points, pts));
    RCCHK(reserve_device(e, e->si.ws, (2 * T + SEARCH_STATS) * sizeof(int)));
    a.p = *params;
    a.n1 = n1;
    a.octave = f1_octave; a.angle = f1_angle; a.f1_desc = f1_descriptors; a.prev = prev_matched;
    a.cand = e->si.cand;
    a.cand_n = e->si.cand + (size_t)e->si.points * cap;
    a.order = a.cand_n + e->si.points;
    a.state = e->si.ws;
    a.owner = e->si.ws + T;
    a.stats = e->si.ws + 2 * T;
    a.matches12 = matches12; a.matches21 = matches21; a.n_matches = n_matches_dev;
    launch_init_candidates(a, e->stream);
    HIPCHK(e, hipGetLastError());
    launch_init_resolve(a, e->stream);
    HIPCHK(e, hipGetLastError());
    e->si.done = true;
    return JSORB_OK;
}

// the synchronous forms' common end: matches12 in the handle's buffer, the count in front of it
static int search_init_sync(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave, const float *f1_angle,
                            const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12_host, float *prev_matched_host, int *n_matches)
{
    HIPCHK(e, hipSetDevice(e->device));
    const int pts = std::max(n1, 1);
    RCCHK(reserve_device(e, e->si.out, ((size_t)pts + 1) * sizeof(int32_t), &e->si.out_points, pts));
    int32_t *cnt = e->si.out, *m12 = cnt + 1;
    RCCHK(jsorb_search_for_initialization_async(e, image, params, n1, f1_octave, f1_angle, f1_descriptors, prev_matched, m12, nullptr, cnt));
    int32_t count = 0;
    HIPCHK(e, hipMemcpyAsync(&count, cnt, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (n1 > 0 && matches12_host) HIPCHK(e, hipMemcpyAsync(matches12_host, m12, (size_t)n1 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (n1 > 0 && prev_matched_host) HIPCHK(e, hipMemcpyAsync(prev_matched_host, prev_matched, (size_t)2 * n1 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *n_matches = count;
    return JSORB_OK;
}

int jsorb_search_for_initialization(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave,
                                    const float *f1_angle, const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12_host,
                                    float *prev_matched_host, int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!n_matches) { e->err = "search_for_initialization: NULL n_matches"; return JSORB_ERR_INVALID; }
    if (n1 < 0) { e->err = "search_for_initialization: n1 < 0"; return JSORB_ERR_INVALID; }
    return search_init_sync(e, image, params, n1, f1_octave, f1_angle, f1_descriptors, prev_matched, matches12_host, prev_matched_host, n_matches);
}

int jsorb_search_for_initialization_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow, int *n_displaced, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[SEARCH_STATS] = {0};
    RCCHK(read_stats(e, e->si.done, "search_for_initialization_stats before jsorb_search_for_initialization", e->si.ws + 2 * (size_t)e->g.T, s, SEARCH_STATS));
    if (rounds) *rounds = s[0];
    if (n_candidates) *n_candidates = s[1];
    if (n_overflow) *n_overflow = s[2];
    if (n_displaced) *n_displaced = s[3];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[4 + b];
    return JSORB_OK;
}

// the kept initial frame: ref_cap entries each of descriptors, octave, angle and prev_matched x, y in one allocation
static uint8_t *ref_desc(const jsorb_extractor *e) { return e->si.ref; }
static int32_t *ref_octave(const jsorb_extractor *e) { return reinterpret_cast<int32_t *>(e->si.ref + (size_t)32 * e->si.ref_cap); }
static float *ref_angle(const jsorb_extractor *e) { return reinterpret_cast<float *>(e->si.ref + (size_t)36 * e->si.ref_cap); }
static float *ref_prev(const jsorb_extractor *e) { return reinterpret_cast<float *>(e->si.ref + (size_t)40 * e->si.ref_cap); }

int jsorb_init_reference_set(jsorb_extractor *e, int image)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) { e->err = "init_reference_set: no extract result for this image"; return JSORB_ERR_STATE; }
    const int n = jsorb_n_keypoints(e, image), cap = round_up(std::max(n, 1), 64);
    HIPCHK(e, hipSetDevice(e->device));
    e->si.ref_n = -1;
    RCCHK(reserve_device(e, e->si.ref, (size_t)48 * cap, &e->si.ref_cap, cap));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));
    mark_main_stream(e);
    if (n > 0) {
        const int32_t *soa = jsorb_keypoints_device(e, image);
        HIPCHK(e, hipMemcpyAsync(ref_desc(e), jsorb_descriptors_device(e, image), (size_t)32 * n, hipMemcpyDeviceToDevice, st));
        HIPCHK(e, hipMemcpyAsync(ref_octave(e), soa + 4 * (size_t)n, (size_t)4 * n, hipMemcpyDeviceToDevice, st));
        HIPCHK(e, hipMemcpyAsync(ref_angle(e), soa + 3 * (size_t)n, (size_t)4 * n, hipMemcpyDeviceToDevice, st));
        launch_init_keys_un(soa, jsorb_keypoints_un_device(e, image), n, ref_prev(e), st);      // vbPrevMatched[i] = mvKeysUn[i].pt
        HIPCHK(e, hipGetLastError());
    }
    e->si.ref_n = n;
    return JSORB_OK;
}

int jsorb_init_reference_clear(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    e->si.ref_n = -1;
    return JSORB_OK;
}

int jsorb_init_reference_n(const jsorb_extractor *e) { return e ? e->si.ref_n : JSORB_ERR_INVALID; }

int jsorb_search_initial_frame(jsorb_extractor *e, int image, const jsorb_init_params *params, int32_t *matches12_host, float *prev_matched_host,
                               int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!n_matches) { e->err = "search_initial_frame: NULL n_matches"; return JSORB_ERR_INVALID; }
    if (e->si.ref_n < 0) { e->err = "search_initial_frame: no initial frame kept (jsorb_init_reference_set)"; return JSORB_ERR_STATE; }
    const int n1 = e->si.ref_n;
    // prev_matched is x[n1] y[n1] at pitch n1 for the kernels: the stored one is kept at that pitch (jsorb_init_reference_set wrote 2 n1 floats)
    return search_init_sync(e, image, params, n1, ref_octave(e), ref_angle(e), ref_desc(e), ref_prev(e), matches12_host, prev_matched_host, n_matches);
}

} // extern "C"
