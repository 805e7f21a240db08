// jsorb_handle.h - internal, host only: the extractor handle and the host helpers shared by the translation units of the C ABI
// (jsorb_api.hip: handles, streams, timing, memory calls; jsorb_extract.hip: the extract pipeline and its results; jsorb_stereo.hip:
// stereo match and speculation; jsorb_frame.hip: rectification, camera, RGB-D, grid; jsorb_search.hip: the four grid matchers; jsorb_localmap.hip: the local map; jsorb_bow.hip:
// vocabulary, BoW transform and BoW matching; jsorb_keyframes.hip, jsorb_loop.hip and jsorb_mappoints.hip: the keyframe matcher, which shares the helpers that take any owner).
// include/jsorb.h only forward-declares the handle, so its layout is free to change.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/jsorb.h"
#include "jsorb_launch.h"

#define JSORB_MAX_LANES 8

using namespace jsorb;

// Stereo match enqueued AHEAD of the call that asks for it (the synchronous single-frame call shape, Frame.cpp:107-125: extract L and R
// from two threads, join, ComputeStereoMatches).  Between the end of the two extracts on the GPU and the start of the match there is
// a host round trip (wake-up of two waits, thread joins, the next call's launch) during which the GPU idles: 53 of the 182 us GPU
// span of a frame.  Once a (left, right) pair has been matched through jsorb_stereo_match, the library repeats that match with the
// same parameters right behind the NEXT pair of single-image extracts, on the GPU, without a host round trip: whichever of the two
// extract calls enqueues last also enqueues k_stereo + k_median behind both (into twin output buffers).  The next jsorb_stereo_match
// on the same pair with the same parameters and no extract in between finds the result finished (or nearly) and adopts it by
// swapping the twin buffers in; anything else (other parameters, another partner, an extract in between, batches) runs the normal
// path and the speculative result is dropped.  The outputs are the outputs of the same kernels on the same inputs either way.
// Shared by the two handles; every field is guarded by `mu` (the two extract calls come from two host threads).
struct jsorb_spec_state {
    std::mutex mu;
    jsorb_extractor *l = nullptr, *r = nullptr;
    bool armed = false;
    float mb = 0.f, mbf = 0.f;
    int th_high = 0, th_low = 0;
    unsigned long long l_base = 0, r_base = 0;   // extract sequence numbers of the two handles when the pair was armed (same frame)
    bool inflight = false;                       // a speculative match is enqueued and not yet adopted or invalidated
    unsigned long long l_seq = 0, r_seq = 0;     // the extracts it matched
    bool wait_l = false, wait_r = false;         // the handle's next extract has to be ordered after the speculative kernels (they read its buffers)
    hipEvent_t ev_done = nullptr;
    long n_adopted = 0, n_dropped = 0;
};

// The handle: the core (geometry, buffers of the extract pipeline, main stream) directly, then one plain struct per feature.  Each feature's
// fields are allocated, reset after an extract and released in the translation unit that holds its entry points.
// The state of one kind of matcher call over keyframe sets, on an extractor (jsorb_search_by_bow*) or a keyframe matcher: allocated on first use
struct KfCall {
    int *stats = nullptr;                  // KF_STATS statistics words of the last call (device)
    int32_t *out = nullptr;                // the synchronous form's outputs (device), grown with the rows
    int out_cap = 0;
    bool done = false;                     // a call has run: the statistics can be read
};
#define KF_STATS 8

// What the map-maintenance calls share (the routines are further down).  A device buffer of 32-bit words that only grows:
// scratch or the staging buffer of a synchronous form.  reserve_words(owner, buf, need) frees and allocates when `need` exceeds it (hipFree waits
// for the device: the last call may still read it), the contents are not kept; free_device(p) releases it.
struct WordBuf {
    int32_t *p = nullptr;
    long long words = 0;
};
// One word per table row with the value every call leaves behind (`fill` bytes): set after growth, and again after a call whose launches were
// cut short (dirty).  reserve_row_words below.
struct RowWords {
    uint32_t *word = nullptr;
    int rows = 0;
    bool dirty = false;
};
// A call's scratch layout, written once as a sequence of take(n): run without a base it only adds up the words the layout needs, run with the
// base it places the pieces, so the two cannot disagree.
struct Carve {
    int32_t *base;
    long long at = 0;
    explicit Carve(int32_t *b) : base(b) {}
    int32_t *take(long long n) { int32_t *p = base ? base + at : nullptr; at += n; return p; }
};

struct jsorb_extractor {
    // ---- core buffers and geometry (jsorb_api.hip: jsorb_create_masked / jsorb_destroy) ----
    jsorb_params p{};
    Geometry g{};
    int B = 1;                 // max_batch
    int n_images = 0;          // images of the last extract
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    int spin_wait = 1;                 // poll instead of block when waiting for a single frame (JSORB_SPIN_WAIT=0 disables)
    // level 0 has to be copied into the pitched slab first (strided host input, device input with unaligned rows): done per lane, on
    // the lane's stream, right before its kernels
    const uint8_t *copy_src = nullptr;
    size_t copy_stride = 0;
    int copy_step = 0, copy_kind = 0;      // 0 none, 1 host (hipMemcpy2DAsync per image), 2 device (one copy kernel per lane)
    bool counts_synced = false;        // h_counts / h_stats reflect the last enqueued batch (set by jsorb_sync)
    size_t detect_lds = 0, pyr_lds = 0;
    unsigned *det_spill = nullptr, *det_spill_flags = nullptr;      // compact k_detect: arena of spill chunks (positives beyond a workgroup's LDS pool) and one busy flag per chunk
    // device buffers
    uint8_t *slab = nullptr, *blur = nullptr, *mask = nullptr;
    uint32_t *lut_bits = nullptr;
    unsigned long long *tile_out = nullptr, *kp = nullptr;
    int *counts = nullptr, *row_tab = nullptr;
    float *angles = nullptr;
    uint8_t *desc = nullptr;
    int32_t *out_kp = nullptr;
    bool nms_ms = false;
    int *ms_grid = nullptr, *ms_scratch = nullptr;   // NMS-MS: level-0 accumulator plane (GPU mode) / mutable scores (CPU mode)
    int *h_counts = nullptr;           // pinned host mirror
    ImageSrc src{};            // where level 0 of the last extract lives
    bool extracted = false;
    std::string err;

    // ---- lanes and streams (jsorb_api.hip) ----
    // Lanes: a batch of many images is split into up to JSORB_MAX_LANES contiguous sub-batches, each enqueued on its own HIP stream
    // (lane 0 = `stream`, the handle's main / caller-provided stream).  The sparse, latency-bound stages of one lane (FAST ring
    // test / NMS, descriptor gathers, the single-workgroup compaction and median kernels) then overlap the streaming stages of
    // another one.  A single frame (the reference's call shape) uses lane 0 only.
    struct {
        hipStream_t used[JSORB_MAX_LANES] = {};   // the stream lane j of the LAST batch ran on (main stream for a one-lane batch, the device's lane pool otherwise)
        hipStream_t readers_stream[JSORB_MAX_LANES] = {};
        hipEvent_t done[JSORB_MAX_LANES] = {};          // after the last work enqueued on lane j
        hipEvent_t readers_done[JSORB_MAX_LANES] = {};  // recorded on ANOTHER handle's lanes after they read this handle's buffers
        hipEvent_t ev_fork = nullptr;
        int max = 4;
        double min_px = 7.0e6;
        int K = 1;                 // lanes used by the last batch
        int first[JSORB_MAX_LANES + 1] = {};
        bool has_readers = false;
        int readers_K = 0, readers_n = 0;
        int cap = JSORB_MAX_LANES;         // transient: cap for the batch being enqueued
        bool main_stream_dirty = false;    // the main stream carries work the lanes' `done` events do not cover (mark_main_stream): the next batch's lanes fork after it
        int order = -1;                    // schedule of the last batch (jsorb_handle_forms): lane order, lanes that ran k_blur_compact / k_blur before k_detect
        unsigned fuse_bc_mask = 0, blur_first_mask = 0;
    } lanes;

    // ---- landing buffers (jsorb_extract.hip) ----
    // host uploads: two dense B x H0 x W0 landing buffers filled by ONE hipMemcpyAsync per batch on a dedicated copy stream, then read
    // in place as level 0.  Double buffering lets the upload of batch k+1 overlap the kernels of batch k.
    struct {
        uint8_t *stage[2] = {nullptr, nullptr};
        int host_lanes = 1;                     // cap on the lanes of a host-uploaded batch (JSORB_HOST_LANES): PCIe-bound, see extract_batch_host_enqueue
        hipEvent_t ev_copied[2][JSORB_MAX_LANES] = {};   // per landing buffer and lane: the lane's images have arrived
        int consumed_n[2] = {0, 0};        // images of the batch that last used the buffer (with consumed_K: its lane partition)
        hipEvent_t ev_consumed[2][JSORB_MAX_LANES] = {};   // per landing buffer and lane
        int consumed_K[2] = {0, 0};        // lanes whose ev_consumed must be waited for before the buffer is refilled (0: never used)
        int cur = 0, last = -1;
    } land;

    // ---- single-frame upload (jsorb_extract.hip) ----
    // single frame from pageable host memory: the calling thread copies the image into this pinned buffer and the first kernel of the
    // frame pulls it over PCIe (JSORB_KERNEL_UPLOAD=0: hipMemcpyAsync instead).  hipMemcpyAsync from pageable memory goes through a
    // staging buffer of the runtime that the two extractor threads of a stereo frame take turns on: the right image started ~20 us late.
    struct {
        uint8_t *h_upload = nullptr;
        hipEvent_t ev_read = nullptr;   // recorded right behind k_upload_level0: the pinned buffer may be rewritten once it has fired
        bool inflight = false;
        bool sync_single = false;       // inside jsorb_extract / jsorb_extract_into: the call itself waits for the frame, nobody needs ev_read (one barrier packet less in front of the match)
        int kernel = 1;
        bool pending = false;           // transient: run_pipeline starts the single-image chain with the upload kernel
    } up;

    // ---- frame graph (jsorb_extract.hip) ----
    // the 5-kernel chain of a single image as a HIP graph (captured on first use, replayed while the arguments stay the same): one
    // hipGraphLaunch instead of five kernel launches on the host's critical path (JSORB_FRAME_GRAPH=0 disables)
    struct {
        hipGraphExec_t exec = nullptr;
        hipGraph_t tmpl = nullptr;                   // the captured graph the executable one was instantiated from (owns the node handles)
        hipGraphNode_t describe_node = nullptr;      // its k_describe node: carries the caller-owned destinations of jsorb_extract_into
        int32_t *dst_kp = nullptr;                   // ... as currently set in the executable graph
        uint8_t *dst_desc = nullptr;
        const void *key[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // l0 source, its pitch, main stream, rectification map, camera, upload node
        int recaptures = 0;             // consecutive frames whose arguments differed from the captured ones
        int on = 1;
    } fg;

    // ---- result mirrors (jsorb_extract.hip) ----
    // single-image calls (the reference's call shape): the kernels write their results into these pinned mirrors themselves (struct
    // Deliver), so that SyncedMem::to_cpu() costs a memcpy instead of a blocking D2H
    struct {
        int32_t *h_kp = nullptr;
        uint8_t *h_desc = nullptr;
        bool mirror_valid = false;
        bool mirror_pending = false;    // a single-image call is in flight whose kernels write the pinned mirrors themselves (struct Deliver)
        int32_t *deliver_kp = nullptr;  // jsorb_extract_into: caller-owned device destinations of the next single-image pipeline
        uint8_t *deliver_desc = nullptr;
        jsorb_keypoint *frame_aos = nullptr;    // Frame-side unpacking (allocated on first use, then kept): AoS keypoints of one image
    } res;

    // ---- stereo outputs and speculation (jsorb_stereo.hip) ----
    struct {
        float *u = nullptr, *d = nullptr;
        int *l1 = nullptr, *stats = nullptr;
        unsigned *aux = nullptr;
        int *h_stats = nullptr;            // pinned mirrors: statistics of every pair; uRight and depth of a single pair (struct DeliverStereo)
        float *h_u = nullptr, *h_d = nullptr;
        bool mirror_valid = false, mirror_pending = false;
        bool done = false;
        int pairs = 0;
        int *diag = nullptr;               // jsorb_set_stereo_diagnostics: 13 int per left keypoint and image (B x T x 13), written by k_stereo when allocated
        const int *l1_view = nullptr;      // L1 distances of the last match: l1, or sp_l1 after an adopted speculative match (jsorb_copy_stereo_l1)
        // speculative stereo match of the synchronous single-frame call shape (struct jsorb_spec_state)
        jsorb_spec_state *spec = nullptr;
        unsigned long long spec_seq = 0;   // extract calls of this handle (written under spec->mu once paired)
        bool spec_single = false;          // the last extract was a single image on an untimed handle
        int speculate = 0;                 // opt-in: jsorb_set_speculative_stereo(l, 1) (the C++ shim does it when it sees Frame's call shape) or JSORB_SPECULATE=1
        int speculate_env = -1;            // JSORB_SPECULATE, when set, wins over the call (0: never, 1: always)
        float *sp_u = nullptr, *sp_d = nullptr, *h_sp_u = nullptr, *h_sp_d = nullptr;   // twin output buffers (left handle), swapped in on adoption
        int *sp_stats = nullptr, *h_sp_stats = nullptr, *sp_l1 = nullptr;   // sp_l1 / sp_aux: scratch of the speculative match (one pair)
        unsigned *sp_aux = nullptr;
    } st;

    // ---- rectification map (jsorb_frame.hip, jsorb_set_rectify_maps) ----
    // the entry points point `src` at the RAW input, run_pipeline remaps it into level 0 of the slab (k_rectify, first kernel of each lane)
    // and points `src` there
    struct {
        bool on = false;
        RectMap map{};
        void *buf = nullptr;               // the map's xy, a and tile table in one device allocation (kept until destroy)
        uint8_t *raw = nullptr;            // strided host input with maps: the raw images land here, dense (B x H x W), allocated on first use
    } rect;

    // ---- camera / undistortion (jsorb_frame.hip, jsorb_set_camera) ----
    // with k1 != 0 run_pipeline appends k_undistort to every lane; buffers allocated on the first set, then kept
    struct {
        bool on = false;
        UndistortCam c{};
        float *un = nullptr;               // B x 2T floats: x_un[N] y_un[N] per image
        float *h_un = nullptr;             // pinned mirror of image 0, written by k_undistort on the single-frame path
        bool un_valid = false;             // `un` holds the last batch undistorted with the current camera
        bool un_mirror = false;            // h_un was written by the last (single-image) pipeline: valid together with res.mirror_valid
    } cam;

    // ---- RGB-D (jsorb_frame.hip, jsorb_rgbd_depth*): allocated on the first call, then kept ----
    struct {
        float *out = nullptr;              // B x T uRight, then B x T depth
        float *h_out = nullptr;            // pinned: T uRight, T depth of image 0 (synchronous call)
        uint8_t *h_depth = nullptr;        // pinned staging of one host depth image (dense rows), read in place by k_rgbd
        bool mirror = false;
        int images = 0;                    // images of the last batch the last RGB-D call covered (0: none; the synchronous call covers image 0 only)
    } rgbd;

    // ---- grid CSR (jsorb_frame.hip): allocated on first use, grown with the number of cells ----
    struct {
        int32_t *start = nullptr, *items = nullptr;
        int cells = 0;
    } grid;

    // ---- local-map search (jsorb_search.hip, jsorb_search_local_points*): allocated on the first call, grown with the number of map points ----
    struct {
        int *cand = nullptr;               // points x search_local_cap() packed candidates, then points counts
        int points = 0;
        int *stats = nullptr;              // rounds, candidates, points over the capacity of the last call (device)
        int32_t *out = nullptr;            // synchronous call: match_kp, match_dist (out_points each), kp_match (T), count
        int out_points = 0;
        bool done = false;
    } sl;

    // ---- motion-model matching (jsorb_search.hip, jsorb_search_last_frame*): allocated on the first call, the per-point part grown with the points ----
    struct {
        int *ws = nullptr;                 // owner (T entries, -1 between calls: k_last_resolve resets what k_last_match set), then 8 control / statistics words
        int *pts = nullptr;                // points x 2: rotation bin, then candidates
        int points = 0;
        int32_t *out = nullptr;            // synchronous call: count, kp_match (T), match_kp, match_dist (out_points each)
        int out_points = 0;
        bool done = false;
    } lf;

    // ---- monocular initialisation matching (jsorb_search.hip, jsorb_search_for_initialization*, jsorb_init_reference_*): allocated on first use, grown only ----
    struct {
        int *cand = nullptr;               // points x search_init_cap() packed candidates, then points counts, then points ordered indices
        int points = 0;
        int *ws = nullptr;                 // state (T entries, when it does not fit k_init_resolve's LDS), owner (T), then 8 statistics words
        int32_t *out = nullptr;            // synchronous calls: count, matches12 (out_points)
        int out_points = 0;
        bool done = false;
        uint8_t *ref = nullptr;            // the kept initial frame, ref_cap entries each: descriptors (32 B), octave, angle, prev_matched x, y
        int ref_cap = 0, ref_n = -1;       // ref_n: its keypoints (-1: none kept)
    } si;

    // ---- keyframe projection matching (jsorb_search.hip, jsorb_search_by_projection_kf*): allocated on the first call, grown with the number of points ----
    struct {
        int *cand = nullptr;               // points x search_kf_cap() keys, then points counts
        int points = 0;
        int *stats = nullptr;              // rounds, candidates, points over the capacity, ind1..3 of the last call (device)
        int32_t *out = nullptr;            // synchronous call: count, kp_match (T), match_kp, match_dist (out_points each)
        int out_points = 0;
        bool done = false;
    } kf;

    // ---- the local map (jsorb_localmap.hip, jsorb_local_map_points*): allocated on the first call, grown only ----
    struct {
        RowWords row;                      // all ones between calls: bit 31 = not seen by the frame, below it the first entry with the row
        uint8_t *keep = nullptr;           // one byte per entry: inside the frustum
        int entries = 0;
        uint32_t *chunk = nullptr;         // chunks sums, then chunks + 1 prefixes
        int chunks = 0;
        int32_t *stats = nullptr;          // E, null, invalid rows, duplicates, bad, seen of the last call (device)
        int32_t *out = nullptr;            // synchronous call: counts (8 words, 5 used), then point_row (out_cap)
        int out_cap = 0;
        bool done = false;
    } lm;

    // ---- the local keyframes (jsorb_localkf.hip, jsorb_local_keyframes*): allocated on the first call, grown only; the row words are lm.row ----
    struct {
        int32_t *slot = nullptr;           // per graph slot: vote, then the first list in order (2 x slots words), then slots bytes `first`
        int slots = 0;
        int32_t *stats = nullptr;          // LK_STATS words of the last call, then the 64-bit `best` (device)
        WordBuf out;                       // synchronous call: counts (8), state_io (2), then local_kf_slot, gathered for one copy back
        bool done = false;
    } lk;

    // ---- the pose optimisation (jsorb_pose.hip, jsorb_pose_optimization*): allocated on the first call, grown only ----
    struct {
        WordBuf edges;                     // n_problems x N: a problem's edges as keypoints in ascending order (PoseArgs::edge_kp)
        int *stats = nullptr;              // PO_STATS words of the last call (device)
        WordBuf io;                        // synchronous call: Tcw_in, Tcw_out (16 floats a problem each), pose (12 doubles), counts (4), outlier (N bytes)
        bool done = false;
    } po;

    // ---- bag of words (jsorb_bow.hip, jsorb_bow_transform_async / jsorb_search_by_bow*): allocated on first use, the keyframe parts grown only ----
    struct {
        int32_t *ids = nullptr;            // B x T word ids, then B x T node ids, then 2 statistics words (descriptors with a shallow leaf)
        std::vector<char> have;            // per image: transformed since the last extract
        unsigned long long *fsort = nullptr, *ksort = nullptr;      // sorted keys of the frame (T) and of the keyframes (kf_cap)
        int kf_cap = 0;
        KfCall search;                     // jsorb_search_by_bow*: 8 statistics words; synchronous call: counts (256), then match_kf (out_cap)
        bool transformed = false;
    } bow;

    // ---- per-kernel timing (jsorb_api.hip) ----
    struct TimedLaunch { int id; hipEvent_t a, b; };
    struct {
        bool on = false;
        std::vector<TimedLaunch> timed;
        double k_ms[JSORB_K_ID_LAST] = {0};
        long k_n[JSORB_K_ID_LAST] = {0};
    } tm;

    // ---- JSORB_TRACE_HOST=1: host-side time of the single-frame calls (H2D enqueue, kernel enqueue, wait), printed at destroy ----
    struct {
        bool on = false;
        double h2d = 0, enq = 0, wait = 0, st_enq = 0, st_wait = 0;
        long n = 0, st_n = 0;
    } trace;
};

// The keyframe matcher of LocalMapping and LoopClosing (jsorb_keyframes.hip: create, destroy, streams, triangulation, fuse; jsorb_loop.hip: the
// loop-closing matchers, SearchByProjection(pKF, Scw, ...) among them; jsorb_mappoints.hip: the map points' distinctive descriptors).  It belongs to
// no extractor handle.
struct jsorb_keyframe_matcher {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev_switch = nullptr;                             // orders a new stream behind the old one (jsorb_keyframe_matcher_set_stream)
    unsigned long long *sort1 = nullptr, *sort2 = nullptr;      // sorted keys of KF1 (cap1) and of the KF2s (cap2): grown only
    int cap1 = 0, cap2 = 0;
    // one state per kind of call, each with statistics and a "done" mark of its own.  The synchronous forms' buffers: counts (256), then match12
    // (triangulation, BoW) or best_idx and best_dist (fuse), out_cap entries each; sim3: the count, then match1, match2 and match12, out_cap in all;
    // scw: the count, then match_kp, match_dist and kp_match, out_cap in all
    // distinct: best_obs, then best_median, out_cap entries each
    enum { TRIANGULATION, FUSE, BOW_KF, SIM3, SCW, DISTINCT, COVIS, CULL, FUSE_MAP, NEW_POINTS, N_CALLS };
    KfCall call[N_CALLS];
    int32_t *grid_start = nullptr, *grid_items = nullptr;       // fuse, sim3: n_keyframes x (cells + 1) starts (grid_cap), the keypoints' items (items_cap)
    int grid_cap = 0, items_cap = 0;
    uint8_t *matched2 = nullptr;                                // BoW: vbMatched2, one byte per candidate keypoint (matched2_cap)
    int matched2_cap = 0;
    struct {                                                    // jsorb_search_by_projection_sim3* (jsorb_loop.hip): k_scw_candidates' lists, grown only
        int *cand = nullptr, *cand_n = nullptr;                 // cand_cap x scw_cap() kept keys, cand_n_cap counts
        int cand_cap = 0, cand_n_cap = 0;
    } scw;
    struct {                                                    // jsorb_distinctive_descriptors* (jsorb_mappoints.hip): k_distinct_plan's tier lists, grown only
        int *list = nullptr;                                    // 3 x list_cap points
        int list_cap = 0;
    } distinct;
    struct {                                                    // jsorb_update_connections* (jsorb_covis.hip), grown only
        RowWords row;                                           // the members' bits, all zero between calls
        int32_t *slot = nullptr;                                // 4 x 32 x slots words: count, kraw, klist, tlist; then 32 x 4 words minfo
        int slots = 0;
    } covis;
    WordBuf cull;                                               // jsorb_cull_keyframes* (jsorb_culling.hip): the observations grouped by row, the rounds' verdicts, the tree repair's lists (CullArgs)
    WordBuf fmap;                                               // jsorb_fuse_map* (jsorb_fuse_apply.hip): the observation index, the stamps, the target's grid, list points and CSR (FuseMapArgs)
    WordBuf npts;                                               // jsorb_create_new_map_points* (jsorb_new_points.hip): the gathered sides, the matches, the compaction (NewPointsArgs)
    WordBuf staging;                                            // the synchronous forms of the three: their outputs gathered for one copy back (read_back; the call waits for it)
    std::string err;
};

#define HIPCHK(e, call)                                                                                   \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess) {                                                                           \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_s);                                 \
            return JSORB_ERR_HIP;                                                                         \
        }                                                                                                 \
    } while (0)
// a call that returns JSORB_OK or an error code (which it has reported itself): the error is passed on
#define RCCHK(call) do { int _rc = (call); if (_rc) return _rc; } while (0)

// Everything below is internal to libjsorb.so (hidden: the exported symbols are the C ABI of include/jsorb.h).
namespace jsorb_host __attribute__((visibility("hidden"))) {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline hipStream_t lane_stream(const jsorb_extractor *e, int j) { return e->lanes.used[j]; }      // of the LAST batch
inline bool check_image(const jsorb_extractor *e, int image) { return e && e->extracted && image >= 0 && image < e->n_images; }

// ---- per-kernel timing: TIMED(e, id, launch) brackets one launch with two events (drained by drain_timed) ----
inline int enqueue_timed(jsorb_extractor *e, int id)
{
    if (!e->tm.on) return JSORB_OK;
    jsorb_extractor::TimedLaunch t{id, nullptr, nullptr};
    HIPCHK(e, hipEventCreate(&t.a));
    HIPCHK(e, hipEventCreate(&t.b));
    HIPCHK(e, hipEventRecord(t.a, e->stream));          // timing forces one lane: everything runs on the main stream
    e->tm.timed.push_back(t);
    return JSORB_OK;
}
inline int finish_timed(jsorb_extractor *e)
{
    if (e->tm.on) HIPCHK(e, hipEventRecord(e->tm.timed.back().b, e->stream));
    return JSORB_OK;
}
int drain_timed(jsorb_extractor *e);

#define TIMED(e, id, stmt) do { RCCHK(enqueue_timed((e), (id))); stmt; RCCHK(finish_timed((e))); } while (0)

// Polls `query` (hipStreamQuery / hipEventQuery on what is waited for) a bounded number of times before the caller blocks: a single frame is
// ~100 us of GPU time, and a blocking wait adds tens of microseconds of wake-up latency.  *done: the query reported completion.
template <class Query> int spin_poll(jsorb_extractor *e, Query query, const char *what, bool *done)
{
    *done = false;
    for (int it = 0; it < 400000; it++) {
        const hipError_t q = query();
        if (q == hipSuccess) { *done = true; return JSORB_OK; }
        if (q != hipErrorNotReady) { e->err = std::string(what) + ": " + hipGetErrorString(q); return JSORB_ERR_HIP; }
        __builtin_ia32_pause();
    }
    return JSORB_OK;
}

// Stream `s` waits for the events ev[0..K-1] of K lanes that ran on the streams on[0..K-1] (errors are reported on `e`).  A lane that ran on `s`
// itself is ordered already.  wait_lanes: the last work of every lane of handle `h`.
inline int wait_events(jsorb_extractor *e, hipStream_t s, const hipStream_t *on, const hipEvent_t *ev, int K)
{
    for (int j = 0; j < K; j++)
        if (on[j] != s) HIPCHK(e, hipStreamWaitEvent(s, ev[j], 0));
    return JSORB_OK;
}
inline int wait_lanes(jsorb_extractor *e, hipStream_t s, const jsorb_extractor *h) { return wait_events(e, s, h->lanes.used, h->lanes.done, h->lanes.K); }
// The other way round: every lane of the handles `hs` that is not `s` continues after what is enqueued on `s` so far (e->lanes.ev_fork,
// recorded on `s` once, and only if some lane needs it).
inline int fork_lanes(jsorb_extractor *e, hipStream_t s, std::initializer_list<const jsorb_extractor *> hs)
{
    bool forked = false;
    for (const jsorb_extractor *h : hs)
        for (int j = 0; j < h->lanes.K; j++)
            if (lane_stream(h, j) != s) {
                if (!forked) { HIPCHK(e, hipEventRecord(e->lanes.ev_fork, s)); forked = true; }
                HIPCHK(e, hipStreamWaitEvent(lane_stream(h, j), e->lanes.ev_fork, 0));
            }
    return JSORB_OK;
}

// Work that reads the last extract's results was enqueued on the main stream outside run_pipeline (a matcher, a transform, a copy into kept
// buffers): the lanes' `done` events were recorded before it, so the pool lanes of the next multi-lane batch - which rewrites those results -
// must fork behind it (order_lanes_for_new_batch), and a new main stream must continue after it (jsorb_set_stream).  A flag, not a fork on
// every batch: a batch that follows only batches and stereo matches (which run on the lanes) enqueues no event for it.  jsorb_sync, which
// waits for the main stream, clears it.
inline void mark_main_stream(jsorb_extractor *e) { e->lanes.main_stream_dirty = true; }

// n x elem bytes of one image's result into dst (nothing when dst is NULL or n <= 0): from its pinned mirror when that holds the image
// (`mirror`, else NULL), otherwise from `dev`, the image's device slice.  Does not touch e->err (the const getters).
inline int copy_result(void *dst, const void *mirror, const void *dev, int n, size_t elem)
{
    if (!dst || n <= 0) return JSORB_OK;
    if (mirror) { memcpy(dst, mirror, (size_t)n * elem); return JSORB_OK; }
    return hipMemcpy(dst, dev, (size_t)n * elem, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

// A device buffer allocated on first use and then kept.  With `have` (units allocated so far, 0: none) it grows on demand instead: when `want`
// units exceed *have the old buffer is freed (hipFree waits for the device: the last call may still read it) and `bytes` are allocated for
// `want` units; the contents are not kept.  The owner is a handle or a keyframe matcher: whatever has `err`.
template <class H, class T> int reserve_device(H *e, T *&p, size_t bytes, int *have = nullptr, int want = 0)
{
    if (have ? *have >= want : p != nullptr) return JSORB_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    if (have) *have = 0;
    HIPCHK(e, hipMalloc(&p, bytes));
    if (have) *have = want;
    return JSORB_OK;
}

// The `_stats` calls' common part: n statistics words of the owner's last search from the device, behind what its stream carries (owner: a handle
// or a keyframe matcher - `device`, `stream`, `err`).  `before`: the error when no search has run.
template <class H> int read_stats(H *h, bool done, const char *before, const int *dev, int32_t *s, int n)
{
    if (!done) { h->err = before; return JSORB_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(s, dev, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return JSORB_OK;
}

// ---- keyframes given as concatenated arrays (jsorb_search_by_bow*, jsorb_search_for_triangulation*) ----
// kf_start of n_keyframes keyframes (keyframe i is kf_start[i] .. kf_start[i + 1]): ascending offsets, every keyframe below 2^18 keypoints.
// rel[] = the offsets relative to *base = kf_start[0], *total = the keypoints of all of them.  NULL, or the error's text behind the feature's
// name with its code in *rc.
inline const char *rebase_kf_start(const int32_t *kf_start, int n_keyframes, int *rel, int *base, int *total, int *rc)
{
    for (int i = 0; i < n_keyframes; i++) {
        const long long len = (long long)kf_start[i + 1] - kf_start[i];
        if (kf_start[i] < 0 || len < 0) { *rc = JSORB_ERR_INVALID; return "kf_start must be ascending offsets"; }
        if (len >= (1 << 18)) { *rc = JSORB_ERR_UNSUPPORTED; return "a keyframe with more than 262143 keypoints"; }
    }
    *base = n_keyframes > 0 ? kf_start[0] : 0;
    *total = n_keyframes > 0 ? kf_start[n_keyframes] - *base : 0;
    for (int i = 0; i <= n_keyframes && n_keyframes > 0; i++) rel[i] = kf_start[i] - *base;
    return nullptr;
}

// The outputs of a search over n_kf keyframes x n keypoints in their "nothing matched" state, on st: the statistics words, the counts (0) and the
// match rows (-1).  *run: the kernels have something to do (a keyframe, a keypoint on this side and one on the other).
template <class H> int clear_kf_outputs(H *h, hipStream_t st, int *stats, int n_stats, int n_kf, int n, int total, int32_t *n_matches, int32_t *match, bool *run)
{
    *run = false;
    HIPCHK(h, hipMemsetAsync(stats, 0, (size_t)n_stats * sizeof(int), st));
    if (n_kf == 0) return JSORB_OK;
    HIPCHK(h, hipMemsetAsync(n_matches, 0, (size_t)n_kf * sizeof(int32_t), st));
    if (n == 0) return JSORB_OK;
    HIPCHK(h, hipMemsetAsync(match, 0xff, (size_t)n_kf * n * sizeof(int32_t), st));
    *run = total > 0;
    return JSORB_OK;
}

// The synchronous forms' end: the n_kf counts and the `rows` match entries behind what the owner's stream carries
template <class H> int copy_kf_results(H *h, int n_kf, size_t rows, const int32_t *cnt, const int32_t *match, int32_t *match_host, int *n_matches_host)
{
    if (n_kf == 0) return JSORB_OK;
    std::vector<int32_t> c((size_t)n_kf);
    HIPCHK(h, hipMemcpyAsync(c.data(), cnt, (size_t)n_kf * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (rows > 0) HIPCHK(h, hipMemcpyAsync(match_host, match, rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n_kf; i++) n_matches_host[i] = c[i];
    return JSORB_OK;
}
// ---- the frames of the keyframe-set entry points, in the manner of jsorb_search.hip's search_check / search_begin /
// search_sync.  The owner H is a handle or a keyframe matcher; `name` is the feature's name in front of every error text.  An entry point's own
// checks (parameters, NULL arrays, alignment) stay written out between these, where they fire. ----
template <class H> int kf_fail(H *h, const char *name, const std::string &what, int rc = JSORB_ERR_INVALID)
{
    h->err = std::string(name) + ": " + what;
    return rc;
}

// The sizes, the first shared check of both forms: n_keyframes, then the single side's n against [0, n_limit) (n_limit 0: no upper bound) with
// the entry point's text for it (NULL: it has no such check - the frame of jsorb_search_by_bow).
template <class H> int kf_check_sizes(H *h, const char *name, int n_keyframes, int n, int n_limit, const char *n_text)
{
    if (n_keyframes < 0 || n_keyframes > JSORB_BOW_MAX_KEYFRAMES) return kf_fail(h, name, "n_keyframes must be in [0, 256]");
    if (n_text && (n < 0 || (n_limit && n >= n_limit))) return kf_fail(h, name, n_text);
    return JSORB_OK;
}

// rebase_kf_start as a check.  keep_rc: the error's own code (a keyframe of more than 262143 keypoints is JSORB_ERR_UNSUPPORTED for
// jsorb_search_by_bow_async); the keyframe matcher's entry points answer JSORB_ERR_INVALID for both - kept as it is.
template <class H> int kf_rebase(H *h, const char *name, const int32_t *kf_start, int n_keyframes, int *rel, int *base, int *total, bool keep_rc = false)
{
    int rc = 0;
    if (const char *bad = rebase_kf_start(kf_start, n_keyframes, rel, base, total, &rc)) return kf_fail(h, name, bad, keep_rc ? rc : JSORB_ERR_INVALID);
    return JSORB_OK;
}

// The start of a call's device work: its statistics words on first use, then clear_kf_outputs and the "done" mark
template <class H> int kf_clear(H *h, KfCall &c, hipStream_t st, int n_kf, int n, int total, int32_t *n_matches, int32_t *match, bool *run)
{
    RCCHK(reserve_device(h, c.stats, KF_STATS * sizeof(int)));
    RCCHK(clear_kf_outputs(h, st, c.stats, KF_STATS, n_kf, n, total, n_matches, match, run));
    c.done = true;
    return JSORB_OK;
}

// The synchronous form behind kf_check_sizes: the call's buffer as counts (256), then `arrays` (1 or 2) arrays of n_keyframes x n entries;
// run(cnt, a0, a1) is the asynchronous form.  The counts and a0 come back through copy_kf_results, a1 (when there is one) into host1.
template <class H, class Run>
int kf_sync(H *h, const char *name, KfCall &c, int n_keyframes, int n, const char *n_name, bool null_host, int arrays, int32_t *host0, int32_t *host1,
            int *n_matches_host, Run run)
{
    if (n_keyframes > 0 && null_host) return kf_fail(h, name, "NULL host output");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t rows = (size_t)n_keyframes * std::max(n, 0);
    if (rows > (size_t)INT_MAX - JSORB_BOW_MAX_KEYFRAMES) return kf_fail(h, name, std::string("n_keyframes x ") + n_name + " too large", JSORB_ERR_UNSUPPORTED);
    const int want = (int)std::max(rows, (size_t)1);
    RCCHK(reserve_device(h, c.out, ((size_t)JSORB_BOW_MAX_KEYFRAMES + arrays * (size_t)want) * sizeof(int32_t), &c.out_cap, want));
    int32_t *cnt = c.out, *a0 = cnt + JSORB_BOW_MAX_KEYFRAMES, *a1 = a0 + want;
    RCCHK(run(cnt, a0, a1));
    if (arrays > 1 && rows > 0) HIPCHK(h, hipMemcpyAsync(host1, a1, rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return copy_kf_results(h, n_keyframes, rows, cnt, a0, host0, n_matches_host);
}

// The statistics words of a call's last run into s[KF_STATS] (read_stats; `before`: the error when none has run)
template <class H> int kf_stats(H *h, const KfCall &c, const char *before, int32_t *s) { return read_stats(h, c.done, before, c.stats, s, KF_STATS); }

template <class T> int reserve_pinned(jsorb_extractor *e, T *&p, size_t bytes) { if (!p) HIPCHK(e, hipHostMalloc(&p, bytes)); return JSORB_OK; }
// release functions: free (and forget) what a feature allocated
template <class... T> void free_device(T *&...p) { ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...); }
template <class... T> void free_pinned(T *&...p) { ((p ? (void)hipHostFree(p) : (void)0, p = nullptr), ...); }
template <class... T> void destroy_event(T &...ev) { ((ev ? (void)hipEventDestroy(ev) : (void)0, ev = nullptr), ...); }

// ---- what the map-maintenance calls share: jsorb_localmap.hip, jsorb_localkf.hip, jsorb_covis.hip, jsorb_culling.hip,
// jsorb_fuse_apply.hip.  Each entry point's own NULL / range / alignment checks stay written out where they fire. ----
template <class H> int reserve_words(H *h, WordBuf &b, long long need)
{
    if (b.words >= need) return JSORB_OK;
    free_device(b.p);
    b.words = 0;
    HIPCHK(h, hipMalloc(&b.p, (size_t)need * sizeof(int32_t)));
    b.words = need;
    return JSORB_OK;
}

// r for a table of n_rows rows: grown on demand; every byte set to `fill` on st after growth or a call that was cut short
template <class H> int reserve_row_words(H *h, RowWords &r, int n_rows, int fill, hipStream_t st)
{
    const int rows_before = r.rows, want = std::max(n_rows, 1);
    RCCHK(reserve_device(h, r.word, (size_t)want * sizeof(uint32_t), &r.rows, want));
    if (r.rows != rows_before || r.dirty) {
        HIPCHK(h, hipMemsetAsync(r.word, fill, (size_t)r.rows * sizeof(uint32_t), st));
        r.dirty = false;
    }
    return JSORB_OK;
}

// The synchronous forms' end: the device arrays src[i] of n[i] words each are gathered into `staging` behind what st carries, come back in one
// copy, and are handed out to dst[i] once the stream has been waited for.  An empty segment is skipped: its src and dst may be NULL.
template <class H> int read_back(H *h, hipStream_t st, WordBuf &staging, int n_segments, const int32_t *const src[], int32_t *const dst[], const size_t n[])
{
    size_t total = 0, at = 0;
    for (int i = 0; i < n_segments; i++) total += n[i];
    RCCHK(reserve_words(h, staging, (long long)total));
    for (int i = 0; i < n_segments; at += n[i++])
        if (n[i]) HIPCHK(h, hipMemcpyAsync(staging.p + at, src[i], n[i] * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    std::vector<int32_t> host(total);
    HIPCHK(h, hipMemcpyAsync(host.data(), staging.p, total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    at = 0;
    for (int i = 0; i < n_segments; at += n[i++])
        if (n[i]) memcpy(dst[i], host.data() + at, n[i] * sizeof(int32_t));
    return JSORB_OK;
}

// conn_capacity of a jsorb_covisibility against what the build's kernels take
inline int check_conn_capacity(jsorb_keyframe_matcher *m, const char *name, int conn_capacity)
{
    if (conn_capacity < covis_cap_min() || conn_capacity > covis_cap_max())
        return kf_fail(m, name, "conn_capacity outside [" + std::to_string(covis_cap_min()) + ", " + std::to_string(covis_cap_max()) + "]");
    return JSORB_OK;
}

// k_bow_group's launch arguments: the single side (f_node, N) and the concatenated keyframes (kf_node at the rebased offsets `rel`)
inline BowMatchArgs bow_group_args(const int *rel, const int32_t *f_node, int N, int n_kf, const int32_t *kf_node, unsigned long long *f_sorted,
                                   unsigned long long *kf_sorted)
{
    BowMatchArgs b{};
    memcpy(b.kf_start, rel, sizeof(b.kf_start));
    b.f_node = f_node; b.N = N; b.n_kf = n_kf; b.kf_node = kf_node;
    b.f_sorted = f_sorted; b.kf_sorted = kf_sorted;
    return b;
}

// k_bow_resolve's / k_tri_resolve's launch arguments: the rows `match` (n_kf x n) over the rebased offsets `rel`, the three kept-bin words
inline RowResolveArgs row_resolve_args(const int *rel, int n_kf, int n, const float *row_angle, const float *kf_angle, int check_orientation, int32_t *match,
                                       int32_t *n_matches, int *kept)
{
    RowResolveArgs r{};
    memcpy(r.kf_start, rel, sizeof(r.kf_start));
    r.n_kf = n_kf; r.n = n; r.row_angle = row_angle; r.kf_angle = kf_angle; r.check_orientation = check_orientation;
    r.match = match; r.n_matches = n_matches; r.kept = kept;
    return r;
}

// the keyframe matcher's grown-only scratch: k_bow_group's keys of both sides; the grid CSRs of n_grids keyframes with `total` keypoints in all
inline int reserve_sort_keys(jsorb_keyframe_matcher *m, int n1, int total)
{
    RCCHK(reserve_device(m, m->sort1, (size_t)std::max(n1, 1) * sizeof(unsigned long long), &m->cap1, std::max(n1, 1)));
    return reserve_device(m, m->sort2, (size_t)std::max(total, 1) * sizeof(unsigned long long), &m->cap2, std::max(total, 1));
}
inline int reserve_grids(jsorb_keyframe_matcher *m, int n_grids, int n_cells, int total)
{
    const int want = n_grids * (n_cells + 1);
    RCCHK(reserve_device(m, m->grid_start, (size_t)want * sizeof(int32_t), &m->grid_cap, want));
    return reserve_device(m, m->grid_items, (size_t)std::max(total, 1) * sizeof(int32_t), &m->items_cap, std::max(total, 1));
}

// k_fuse_grids' launch arguments from any parameter struct with min_x ... rows; the caller fills kf_start
template <class P> FuseGridArgs fuse_grid_args(const P &p, const float *x, const float *y, int32_t *cell_start, int32_t *cell_items)
{
    FuseGridArgs g{};
    g.x = x; g.y = y;
    g.min_x = p.min_x; g.min_y = p.min_y; g.inv_w = p.inv_w; g.inv_h = p.inv_h; g.cols = p.cols; g.rows = p.rows;
    g.cell_start = cell_start; g.cell_items = cell_items;
    return g;
}

// ---- jsorb_api.hip ----
int pool_stream(jsorb_extractor *e, int j, hipStream_t *out);      // lane stream j of the device's pool
int pool_copy_stream(jsorb_extractor *e, hipStream_t *out);         // the device's upload stream

// ---- jsorb_extract.hip ----
int landing_create(jsorb_extractor *e);
int results_create(jsorb_extractor *e);
void frame_graph_drop(jsorb_extractor *e);
int wait_event(jsorb_extractor *e, hipEvent_t ev, bool spin);
void mirrors_landed(jsorb_extractor *e);
void extract_release(jsorb_extractor *e);         // frame graph, single-frame upload, landing buffers, result mirrors
bool frame_fuses_detect_blur(const jsorb_extractor *e);      // a single frame of this handle runs k_detect and k_blur as one launch (timing off)

// ---- jsorb_stereo.hip ----
int stereo_create(jsorb_extractor *e);
int spec_guard(jsorb_extractor *e, int n);
void spec_after_extract(jsorb_extractor *e, int n);
void spec_detach(jsorb_spec_state *S);
void stereo_after_extract(jsorb_extractor *e);
void stereo_release(jsorb_extractor *e);

// ---- jsorb_frame.hip ----
int rectify_reserve_raw(jsorb_extractor *e, size_t image_bytes);
void rectify_release(jsorb_extractor *e);
void camera_after_extract(jsorb_extractor *e, bool direct);
void camera_release(jsorb_extractor *e);
void rgbd_invalidate(jsorb_extractor *e);
void rgbd_release(jsorb_extractor *e);
void grid_release(jsorb_extractor *e);
int grid_reserve(jsorb_extractor *e, int n_cells);      // the grid CSR for n_cells cells (grown on demand)

// ---- jsorb_search.hip ----
void search_local_release(jsorb_extractor *e);
void search_last_release(jsorb_extractor *e);
void search_init_release(jsorb_extractor *e);
void search_kf_release(jsorb_extractor *e);

// ---- jsorb_localmap.hip ----
void local_map_release(jsorb_extractor *e);

// ---- jsorb_localkf.hip ----
void local_kf_release(jsorb_extractor *e);

// ---- jsorb_pose.hip ----
void pose_release(jsorb_extractor *e);

// ---- jsorb_bow.hip ----
void bow_after_extract(jsorb_extractor *e);
void bow_release(jsorb_extractor *e);

} // namespace jsorb_host

using namespace jsorb_host;
