// jsorb_api.hip - host side of libjsorb: the C ABI declared in include/jsorb.h.
//
// Mirrors ORB_GPU's host orchestration (src/cuda/orb_gpu.cpp) with an MI355X-first structure:
//   reference: ~7L+1 launches on L streams + 3 blocking copies + 2 full stream-sync rounds per image,
//              per-frame cudaMalloc/cudaFree + cublasCreate/Destroy in the stereo matcher
//   here:      5 launches per BATCH of images (pyramid, detect, compact, blur, describe) + 2 per batch of pairs
//              (stereo, median) on one stream, no host round trip in the middle, one small D2H of counts at the end,
//              nothing allocated after jsorb_create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/jsorb.h"
#include "jsorb_launch.h"

// pyramid megapixels per lane and launch below which every lane of a batch runs the fused k_blur_compact launch (run_pipeline)
#ifndef JSORB_FUSE_ALL_BELOW_MPX
#define JSORB_FUSE_ALL_BELOW_MPX 24.0
#endif

#define JSORB_MAX_LANES 8

using namespace jsorb;

namespace {

const char *k_names[JSORB_K_COUNT_ALL] = {"k_pyramid", "k_detect", "k_compact", "k_blur", "k_describe", "k_stereo", "k_median", "k_nms_ms", "k_rectify",
                                          "k_undistort", "k_rgbd"};
// kernels of jsorb_search_local_points*: ids JSORB_K_ASSIGN_GRID .. JSORB_K_ID_END - 1 (JSORB_K_COUNT_ALL itself names no kernel)
const char *k_names_local[JSORB_K_ID_END - JSORB_K_ASSIGN_GRID] = {"k_assign_grid", "k_local_candidates", "k_local_resolve"};

struct TimedLaunch { int id; hipEvent_t a, b; };

// HIP multiplexes every stream of a process over GPU_MAX_HW_QUEUES hardware queues (default 4), and a stream that waits for an event
// holds up every other stream that shares its queue.  This library runs 4 lane streams + 1 upload stream + one main stream per handle;
// on 4 queues which of them share is decided by creation order (measured with otherwise identical code, only the number of idle streams
// created earlier differing: 85.7 k against 91.4 k pairs/s device-resident, 47 k against 71 k host-streamed).  Sixteen queues give every
// stream of a few handle pairs its own (8 were not enough for bench.py, which keeps two sets of handles alive).  The variable is read when the HIP runtime initialises (its first API call), so this
// constructor - run when the library is loaded - is early enough for a process that links the library or imports the Python binding
// before it touches the GPU; an explicit setting by the user wins.  ("Runtime environment")
// JSORB_NO_ENV=1 forbids it: an integrator who does not want a library to touch the process environment sets the variable itself (or not).
__attribute__((constructor)) void jsorb_runtime_defaults()
{
    const char *no = product_env("JSORB_NO_ENV");
    if (!(no && atoi(no) != 0)) setenv("GPU_MAX_HW_QUEUES", "16", 0);
}

} // namespace

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

struct jsorb_extractor {
    jsorb_params p{};
    Geometry g{};
    int B = 1;                 // max_batch
    int n_images = 0;          // images of the last extract
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // Lanes: a batch of many images is split into up to JSORB_MAX_LANES contiguous sub-batches, each enqueued on its own HIP stream
    // (lane 0 = `stream`, the handle's main / caller-provided stream).  The sparse, latency-bound stages of one lane (FAST ring
    // test / NMS, descriptor gathers, the single-workgroup compaction and median kernels) then overlap the streaming stages of
    // another one.  A single frame (the reference's call shape) uses lane 0 only.
    hipStream_t lane_used[JSORB_MAX_LANES] = {};   // the stream lane j of the LAST batch ran on (main stream for a one-lane batch, the device's lane pool otherwise)
    hipStream_t readers_stream[JSORB_MAX_LANES] = {};
    hipEvent_t lane_done[JSORB_MAX_LANES] = {};          // after the last work enqueued on lane j
    hipEvent_t lane_readers_done[JSORB_MAX_LANES] = {};  // recorded on ANOTHER handle's lanes after they read this handle's buffers
    hipEvent_t ev_fork = nullptr;
    int max_lanes = 4;
    int spin_wait = 1;                 // poll instead of block when waiting for a single frame (JSORB_SPIN_WAIT=0 disables)
    double lane_min_px = 7.0e6;
    int K = 1;                 // lanes used by the last batch
    int lane_first[JSORB_MAX_LANES + 1] = {};
    bool has_readers = false;
    int readers_K = 0, readers_n = 0;
    // level 0 has to be copied into the pitched slab first (strided host input, device input with unaligned rows): done per lane, on
    // the lane's stream, right before its kernels
    const uint8_t *copy_src = nullptr;
    size_t copy_stride = 0;
    int copy_step = 0, copy_kind = 0;      // 0 none, 1 host (hipMemcpy2DAsync per image), 2 device (one copy kernel per lane)
    bool main_stream_dirty = false;    // this call enqueued input copies on the main stream: the lanes must fork after them
    bool counts_synced = false;        // h_counts / h_stats reflect the last enqueued batch (set by jsorb_sync)
    size_t detect_lds = 0, pyr_lds = 0;
    unsigned *det_spill = nullptr, *det_spill_flags = nullptr;      // compact k_detect: arena of spill chunks (positives beyond a workgroup's LDS pool) and one busy flag per chunk
    // device buffers
    uint8_t *slab = nullptr, *blur = nullptr, *mask = nullptr;
    // host uploads: two dense B x H0 x W0 landing buffers filled by ONE hipMemcpyAsync per batch on a dedicated copy stream, then read
    // in place as level 0.  Double buffering lets the upload of batch k+1 overlap the kernels of batch k.
    uint8_t *stage[2] = {nullptr, nullptr};
    int host_lanes = 1;                     // cap on the lanes of a host-uploaded batch (JSORB_HOST_LANES): PCIe-bound, see extract_batch_host_enqueue
    int lane_cap = JSORB_MAX_LANES;         // transient: cap for the batch being enqueued
    hipEvent_t ev_copied[2][JSORB_MAX_LANES] = {};   // per landing buffer and lane: the lane's images have arrived
    int consumed_n[2] = {0, 0};        // images of the batch that last used the buffer (with consumed_K: its lane partition)
    hipEvent_t ev_consumed[2][JSORB_MAX_LANES] = {};   // per landing buffer and lane
    int consumed_K[2] = {0, 0};        // lanes whose ev_consumed must be waited for before the buffer is refilled (0: never used)
    int stage_cur = 0, last_stage = -1;
    uint32_t *lut_bits = nullptr;
    unsigned long long *tile_out = nullptr, *kp = nullptr;
    int *counts = nullptr, *row_tab = nullptr;
    float *angles = nullptr;
    uint8_t *desc = nullptr;
    int32_t *out_kp = nullptr;
    float *st_u = nullptr, *st_d = nullptr;
    int *st_l1 = nullptr, *st_stats = nullptr;
    unsigned *st_aux = nullptr;
    // Frame-side unpacking (allocated on first use, then kept): AoS keypoints of one image, grid CSR
    jsorb_keypoint *frame_aos = nullptr;
    int32_t *grid_start = nullptr, *grid_items = nullptr;
    int grid_cells = 0;
    bool nms_ms = false;
    int *ms_grid = nullptr, *ms_scratch = nullptr;   // NMS-MS: level-0 accumulator plane (GPU mode) / mutable scores (CPU mode)
    // pinned host mirrors
    int *h_counts = nullptr, *h_stats = nullptr;
    // single-image calls (the reference's call shape): the kernels write their results into these pinned mirrors themselves (struct
    // Deliver), so that SyncedMem::to_cpu() / the stereo outputs cost a memcpy instead of a blocking D2H
    int32_t *h_kp = nullptr;
    uint8_t *h_desc = nullptr;
    float *h_u = nullptr, *h_d = nullptr;
    bool mirror_valid = false, st_mirror_valid = false;
    bool mirror_pending = false, st_mirror_pending = false;   // a single-image call is in flight whose kernels write the pinned mirrors themselves (struct Deliver)
    // the 5-kernel chain of a single image as a HIP graph (captured on first use, replayed while the arguments stay the same): one
    // hipGraphLaunch instead of five kernel launches on the host's critical path (JSORB_FRAME_GRAPH=0 disables)
    hipGraphExec_t frame_graph = nullptr;
    hipGraph_t frame_graph_tmpl = nullptr;          // the captured graph the executable one was instantiated from (owns the node handles)
    hipGraphNode_t fg_describe_node = nullptr;      // its k_describe node: carries the caller-owned destinations of jsorb_extract_into
    int32_t *fg_dst_kp = nullptr;                   // ... as currently set in the executable graph
    uint8_t *fg_dst_desc = nullptr;
    const void *fg_key[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // l0 source, its pitch, main stream, rectification map, camera, upload node
    // single frame from pageable host memory: the calling thread copies the image into this pinned buffer and the first kernel of the
    // frame pulls it over PCIe (JSORB_KERNEL_UPLOAD=0: hipMemcpyAsync instead).  hipMemcpyAsync from pageable memory goes through a
    // staging buffer of the runtime that the two extractor threads of a stereo frame take turns on: the right image started ~20 us late.
    uint8_t *h_upload = nullptr;
    hipEvent_t ev_upload_read = nullptr;   // recorded right behind k_upload_level0: the pinned buffer may be rewritten once it has fired
    bool upload_inflight = false;
    bool sync_single = false;              // inside jsorb_extract / jsorb_extract_into: the call itself waits for the frame, nobody needs ev_upload_read (one barrier packet less in front of the match)
    int kernel_upload = 1;
    bool upload_pending = false;       // transient: run_pipeline starts the single-image chain with the upload kernel
    int fg_recaptures = 0;             // consecutive frames whose arguments differed from the captured ones
    int use_frame_graph = 1;
    int32_t *deliver_kp_dev = nullptr;      // jsorb_extract_into: caller-owned device destinations of the next single-image pipeline
    uint8_t *deliver_desc_dev = nullptr;
    // speculative stereo match of the synchronous single-frame call shape (struct jsorb_spec_state)
    jsorb_spec_state *spec = nullptr;
    unsigned long long spec_seq = 0;   // extract calls of this handle (written under spec->mu once paired)
    bool spec_single = false;          // the last extract was a single image on an untimed handle
    int speculate = 0;                 // opt-in: jsorb_set_speculative_stereo(l, 1) (the C++ shim does it when it sees Frame's call shape) or JSORB_SPECULATE=1
    int speculate_env = -1;            // JSORB_SPECULATE, when set, wins over the call (0: never, 1: always)
    float *sp_u = nullptr, *sp_d = nullptr, *h_sp_u = nullptr, *h_sp_d = nullptr;   // twin output buffers (left handle), swapped in on adoption
    int *st_diag = nullptr;            // jsorb_set_stereo_diagnostics: 13 int per left keypoint and image (B x T x 13), written by k_stereo when allocated
    const int *l1_view = nullptr;      // L1 distances of the last match: st_l1, or sp_l1 after an adopted speculative match (jsorb_copy_stereo_l1)
    int *sp_stats = nullptr, *h_sp_stats = nullptr, *sp_l1 = nullptr;   // sp_l1 / sp_aux: scratch of the speculative match (one pair)
    unsigned *sp_aux = nullptr;
    ImageSrc src{};            // where level 0 of the last extract lives
    // rectification map (jsorb_set_rectify_maps): the entry points point `src` at the RAW input, run_pipeline remaps it into level 0 of the slab
    // (k_rectify, first kernel of each lane) and points `src` there
    bool rect_on = false;
    RectMap rmap{};
    void *rect_buf = nullptr;          // the map's xy, a and tile table in one device allocation (kept until destroy)
    uint8_t *rect_raw = nullptr;       // strided host input with maps: the raw images land here, dense (B x H x W), allocated on first use
    // camera (jsorb_set_camera): with k1 != 0 run_pipeline appends k_undistort to every lane; buffers allocated on the first set, then kept
    bool cam_on = false;
    UndistortCam cam{};
    float *un = nullptr;               // B x 2T floats: x_un[N] y_un[N] per image
    float *h_un = nullptr;             // pinned mirror of image 0, written by k_undistort on the single-frame path
    bool un_valid = false;             // `un` holds the last batch undistorted with the current camera
    bool un_mirror = false;            // h_un was written by the last (single-image) pipeline: valid together with mirror_valid
    // RGB-D (jsorb_rgbd_depth*): allocated on the first call, then kept
    float *rg = nullptr;               // B x T uRight, then B x T depth
    float *h_rg = nullptr;             // pinned: T uRight, T depth of image 0 (synchronous call)
    uint8_t *h_depth = nullptr;        // pinned staging of one host depth image (dense rows), read in place by k_rgbd
    bool rgbd_mirror = false;
    int rgbd_images = 0;               // images of the last batch the last RGB-D call covered (0: none; the synchronous call covers image 0 only)
    // jsorb_search_local_points*: allocated on the first call, grown with the number of map points
    int *sl_cand = nullptr;            // sl_points x search_local_cap() packed candidates, then sl_points counts
    int sl_points = 0;
    int *sl_stats = nullptr;           // rounds, candidates, points over the capacity of the last call (device)
    int32_t *sl_out = nullptr;         // synchronous call: match_kp, match_dist (sl_out_points each), kp_match (T), count
    int sl_out_points = 0;
    bool sl_done = false;
    bool extracted = false, stereo_done = false;
    int stereo_pairs = 0;
    bool timing = false;
    std::vector<TimedLaunch> timed;
    double k_ms[JSORB_K_ID_END] = {0};
    long k_n[JSORB_K_ID_END] = {0};
    std::string err;
    // JSORB_TRACE_HOST=1: host-side time of the single-frame calls (H2D enqueue, kernel enqueue, wait), printed at destroy
    bool trace_host = false;
    double th_h2d = 0, th_enq = 0, th_wait = 0, th_st_enq = 0, th_st_wait = 0;
    long th_n = 0, th_st_n = 0;
};

namespace {

#define HIPCHK(e, call)                                                                                   \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess) {                                                                           \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_s);                                 \
            return JSORB_ERR_HIP;                                                                         \
        }                                                                                                 \
    } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Geometry exactly as ORB_GPU::ORB_GPU computes it (orb_gpu.cpp:49-62, 224-258, 305-327) plus this build's launch tables.
int build_geometry(const jsorb_params &p, Geometry &g, std::string &err)
{
    if (p.n_levels < 1 || p.n_levels > JSORB_MAX_LEVELS) { err = "n_levels out of range"; return JSORB_ERR_INVALID; }
    if (p.height < 1 || p.width < 1 || p.height > 32767 || p.width > 32767) { err = "image size out of range"; return JSORB_ERR_INVALID; }
    if (p.tile_h < 1 || p.tile_w < 1 || p.tile_w > 128 || p.tile_h > 128) {
        // the reference launches 128/tile_w tiles per block (orb_FAST_apply_NMS_G.cu:1434): tile_w > 128 divides by zero there
        err = "tile size must be in [1,128]";
        return JSORB_ERR_INVALID;
    }
    if (!(p.scale_factor > 1.0f) && p.n_levels > 1) { err = "scale_factor must be > 1"; return JSORB_ERR_INVALID; }
    memset(&g, 0, sizeof(g));
    g.L = p.n_levels;
    g.latency = p.max_batch <= 1 && !(product_env("JSORB_THROUGHPUT_LAYOUT") && atoi(product_env("JSORB_THROUGHPUT_LAYOUT")) != 0);
    g.threshold = p.th_fast_max;   // th_FAST_MIN is overwritten in the reference (orb_gpu.cpp:42-47)
    float scale[JSORB_MAX_LEVELS], inv[JSORB_MAX_LEVELS];
    scale[0] = 1.0f; inv[0] = 1.0f;
    g.lv[0].H = p.height; g.lv[0].W = p.width;
    for (int i = 1; i < g.L; i++) {
        scale[i] = p.scale_factor * scale[i - 1];
        inv[i] = 1.0f / scale[i];
        g.lv[i].H = (int)((float)p.height * inv[i]);
        g.lv[i].W = (int)((float)p.width * inv[i]);
        if (g.lv[i].H < 1 || g.lv[i].W < 1) { err = "pyramid level collapses to zero size"; return JSORB_ERR_INVALID; }
    }
    int tiles = 0, dblk = 0, bblk = 0, pblk = 0, rtab = 0;
    unsigned long long off = 0;
    for (int i = 0; i < g.L; i++) {
        LevelDesc &lv = g.lv[i];
        lv.scale = scale[i]; lv.inv_scale = inv[i];
        lv.pyr_s = 1.0f / inv[i];
        lv.pitch = round_up(lv.W, 64);
        lv.img_off = off;
        off += (unsigned long long)lv.pitch * lv.H;
        off = (off + 255) & ~255ull;
        if (p.fixed_multi_scale_tile_size || i == 0) { lv.th = p.tile_h; lv.tw = p.tile_w; }
        else { lv.th = (int)((float)p.tile_h * inv[i]); lv.tw = (int)((float)p.tile_w * inv[i]); }
        if (lv.th < 1 || lv.tw < 1) { err = "tile size collapses to zero at a pyramid level"; return JSORB_ERR_INVALID; }
        lv.nth = (lv.H - 1) / lv.th + 1;
        lv.ntw = (lv.W - 1) / lv.tw + 1;
        lv.tile_off = tiles;
        tiles += lv.nth * lv.ntw;
        // K3 launch constants that define the tie-break order (orb_FAST_apply_NMS_G.cu:1405-1434)
        int n_loc = std::max(1, std::min(10, lv.tw / 3));
        if (n_loc > lv.th) n_loc = lv.th;
        int n_ty = (lv.th - 1) / n_loc + 1;
        if (n_ty * 128 > 1024) n_ty = 1024 / 128;
        lv.n_ty = n_ty;
        lv.mini_tile = (lv.th - 1) / n_ty + 1;
        lv.recip_nty = (65536 + n_ty - 1) / n_ty;
        lv.recip_tw = (65536 + lv.tw - 1) / lv.tw;
        lv.recip_th = (65536 + lv.th - 1) / lv.th;
        lv.log2_tw = 0;
        while ((1 << lv.log2_tw) < lv.tw) lv.log2_tw++;
        // this build's workgroup tables
        lv.k_tiles = std::max(1, 122 / lv.tw);   // k*tw + 2 <= 124: a score-region row fits 32 aligned LDS dwords (k_detect phase 1)
        lv.groups_per_row = (lv.ntw - 1) / lv.k_tiles + 1;
        lv.det_R = 1;
        lv.detect_blk0 = dblk;           // provisional: fill_detect_layout() may put several tile rows into one workgroup
        dblk += lv.nth * lv.groups_per_row;
        lv.row_tab_off = rtab;
        rtab += lv.nth + 1;
    }
    fill_blur_layout(g);                 // k_blur: strips of 8 columns x bands of rows, 256 items per workgroup
    bblk = g.blur_blocks;
    (void)pblk;
    g.T = tiles;
    if (tiles >= (1 << 20)) { err = "too many tiles"; return JSORB_ERR_INVALID; }
    g.detect_blocks = dblk; g.blur_blocks = bblk; g.row_tab_len = rtab;
    g.row_tab_stride = rtab + tiles + 1;
    // Column pruning in the stereo matcher (k_stereo): measured k_stereo time per step 0.191 -> 0.175 ms at the EuRoC shape (26 tiles per row,
    // the disparity window reaches 15), 0.160 -> 0.145 ms KITTI-shaped, 0.65 -> 0.52 ms KAIST-shaped (64 tiles per row, 23 in the window).
    // JSORB_STEREO_COLPRUNE=0 restores the whole-row scan.
    g.stereo_colprune = 1;
    if (const char *cp = experiment_env("JSORB_STEREO_COLPRUNE")) g.stereo_colprune = atoi(cp) != 0;
    // Scan-line buckets (k_compact sorts the keypoints by level and level-0 row, k_stereo scans the few buckets around the left keypoint's
    // row instead of whole tile rows): 370 -> 35 right keypoints looked at per left keypoint at the EuRoC shape.  Needs the flat k_compact
    // (T <= 65536), L * H0 counters in its LDS, and level-0 coordinates that fit 16 bits.  JSORB_STEREO_EPI=0 keeps the tile-based scan.
    g.epi_rows = 0; g.epi_off = 0;
    {
        const bool want = !env_is(experiment_env("JSORB_STEREO_EPI"), 0);
        if (want && tiles <= 65536 && g.L * g.lv[0].H <= 12288 && g.lv[0].W < 32768 && g.lv[0].H < 32768) {
            g.epi_rows = g.lv[0].H;
            g.epi_off = (g.row_tab_stride + 1) & ~1;
            g.row_tab_stride = g.epi_off + ((g.L * g.epi_rows + 2) & ~1) + 2 * tiles;
        }
    }
    g.slab_bytes = off;
    fill_pyramid_layout(g);              // k_pyramid: PYR_TW x pyr_th output tile per (single-wave) workgroup
    return JSORB_OK;
}

// FAST bounded-arc LUT (orb_gpu.cpp:367-436) for all 65536 indices, packed 1 bit per entry.
// K3's horizontal reduction (orb_FAST_apply_NMS_G.cu:1318-1352) on one tile row of tw column winners: ceil-halving rounds,
// slot j takes slot j+gs only if strictly greater, stale slots included.  Returns the winning column.
static int tree_winner(const int *score, int tw, int log2_tw)
{
    int sc[128], col[128];
    for (int j = 0; j < tw; j++) { sc[j] = score[j]; col[j] = j; }
    int gs = (tw - 1) / 2 + 1;
    for (int it = 0; it < log2_tw; it++) {
        for (int j = 0; j < gs; j++)                       // reads of a round see the previous round's slots (j+gs >= gs is not written)
            if (j + gs < tw && sc[j] < sc[j + gs]) { sc[j] = sc[j + gs]; col[j] = col[j + gs]; }
        gs = (gs - 1) / 2 + 1;
    }
    return col[0];
}

// The tree above is a tournament in which the left slot wins ties, so among equal scores the winner is fixed by a priority order
// of the columns.  The order is derived here from all pairwise duels and then CHECKED against the literal tree on random tie
// sets; k_detect uses the arg-max form only if the check passes (otherwise it replays the tree literally).
static bool build_tree_rank(int tw, int log2_tw, uint8_t *rank, uint8_t *inv)
{
    int sc[128];
    std::vector<int> beaten(tw, 0);
    for (int a = 0; a < tw; a++)
        for (int b = a + 1; b < tw; b++) {
            for (int j = 0; j < tw; j++) sc[j] = (j == a || j == b) ? 1 : 0;
            const int w = tree_winner(sc, tw, log2_tw);
            if (w != a && w != b) return false;
            beaten[w == a ? b : a]++;
        }
    std::vector<int> seen(tw, 0);
    for (int c = 0; c < tw; c++) {
        if (beaten[c] < 0 || beaten[c] >= tw || seen[beaten[c]]) return false;      // not a total order
        seen[beaten[c]] = 1;
        rank[c] = (uint8_t)beaten[c];
        inv[beaten[c]] = (uint8_t)c;
    }
    uint64_t rs = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; };
    for (int trial = 0; trial < 3000; trial++) {
        // random scores with few distinct values (many ties), random active width like a tile at the right image border
        const int levels = 1 + (int)(rnd() % 3), wa = trial % 5 == 0 ? 1 + (int)(rnd() % tw) : tw;
        int best = -1, best_c = 0;
        for (int j = 0; j < tw; j++) {
            sc[j] = j < wa ? (int)(rnd() % (levels + 1)) : 0;
            if (sc[j] > best || (sc[j] == best && rank[j] < rank[best_c])) { best = sc[j]; best_c = j; }
        }
        if (best == 0) best_c = 0;                          // nothing positive: slot 0 is never replaced
        if (tree_winner(sc, tw, log2_tw) != best_c) return false;
    }
    return true;
}

void build_lut_bits(int nmin, int nmax, std::vector<uint32_t> &bits)
{
    bits.assign(2048, 0u);
    for (int j = 0; j < 65536; j++) {
        int run = 0, probe = 0x8000;
        bool undecided = true;
        for (int k = 0; k < 16; k++, probe >>= 1) {
            if (j & probe) { run++; continue; }
            if (run >= nmin && run <= nmax) { undecided = false; break; }
            run = 0;
        }
        if (undecided) {   // wrap-around: the leading run is appended to the trailing one
            probe = 0x8000;
            for (int k = 0; k < 16 && (j & probe); k++, probe >>= 1) run++;
        }
        if (run >= nmin && run <= nmax) bits[j >> 5] |= 1u << (j & 31);
    }
}

// The device copy of the LUT is stored at the index k_detect forms: ring pixel k (bit k of the reference's mask) sits at bit
// detect_ring_bit_of_pixel(k) of the index.
void permute_lut_bits(const std::vector<uint32_t> &ref, uint32_t *out)
{
    int perm[16];
    for (int k = 0; k < 16; k++) perm[k] = detect_ring_bit_of_pixel(k);
    for (int w = 0; w < 2048; w++) out[w] = 0u;
    for (int j = 0; j < 65536; j++)
        if ((ref[j >> 5] >> (j & 31)) & 1u) {
            unsigned ix = 0;
            for (int k = 0; k < 16; k++)
                if (j & (1 << k)) ix |= 1u << perm[k];
            out[ix >> 5] |= 1u << (ix & 31);
        }
}

int enqueue_timed(jsorb_extractor *e, int id)
{
    if (!e->timing) return JSORB_OK;
    TimedLaunch t{id, nullptr, nullptr};
    HIPCHK(e, hipEventCreate(&t.a));
    HIPCHK(e, hipEventCreate(&t.b));
    HIPCHK(e, hipEventRecord(t.a, e->stream));          // timing forces one lane: everything runs on the main stream
    e->timed.push_back(t);
    return JSORB_OK;
}
int finish_timed(jsorb_extractor *e)
{
    if (!e->timing) return JSORB_OK;
    HIPCHK(e, hipEventRecord(e->timed.back().b, e->stream));
    return JSORB_OK;
}
int drain_timed(jsorb_extractor *e)
{
    for (auto &t : e->timed) {
        float ms = 0.f;
        HIPCHK(e, hipEventSynchronize(t.b));
        HIPCHK(e, hipEventElapsedTime(&ms, t.a, t.b));
        e->k_ms[t.id] += ms;
        e->k_n[t.id] += 1;
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    e->timed.clear();
    return JSORB_OK;
}

#define TIMED(e, id, stmt)                                   \
    do {                                                     \
        int _rc = enqueue_timed((e), (id));                  \
        if (_rc) return _rc;                                 \
        stmt;                                                \
        _rc = finish_timed((e));                             \
        if (_rc) return _rc;                                 \
    } while (0)

// Lane streams are a per-device POOL shared by every handle of the process: lane j of the left extractor, lane j of the right
// extractor and lane j of their stereo match land on the SAME stream, in call order - a chain of 12 kernels per lane with no
// cross-stream dependency inside it, and the chains of different lanes drift out of phase so that different stages overlap on the
// GPU.  (Private lane streams per handle put all lanes in lock-step on the same stage and tie left and right together with
// events: measured 80 k pairs/s against 85 k for the pooled form at C2.)
struct LanePool {
    std::mutex m;
    hipStream_t s[JSORB_MAX_LANES] = {};
    hipStream_t copy = nullptr;     // uploads of host batches, all handles: see pool_copy_stream
    std::vector<hipStream_t> idle_main;   // main streams of destroyed handles, handed to the next jsorb_create (see pool_main_stream)
};
LanePool g_pool[16];

// k_detect's spill arena (compact form) is shared by every handle of a device whose spill chunks have the same size - a left / right pair, the
// handles of a bench or test process: the busy flags make it safe under concurrent kernels of any number of handles (a chunk is claimed with a
// compare-and-swap and returned by the workgroup that took it), and its size depends on how many workgroups the DEVICE can hold, not on how many
// handles exist.  Reference counted; the last handle frees it.  (Round-5 review: ~80 MB per handle before.)
struct SpillArena { int device; int chunk_entries; unsigned *data; unsigned *flags; int refs; };
std::mutex g_arena_mu;
std::vector<SpillArena> g_arenas;

int arena_acquire(jsorb_extractor *e, int chunk_entries, size_t bytes, size_t flag_words, unsigned **data, unsigned **flags)
{
    std::lock_guard<std::mutex> lk(g_arena_mu);
    for (auto &a : g_arenas)
        if (a.device == e->device && a.chunk_entries == chunk_entries) { a.refs++; *data = a.data; *flags = a.flags; return JSORB_OK; }
    SpillArena a{e->device, chunk_entries, nullptr, nullptr, 1};
    if (hipMalloc(&a.data, bytes) != hipSuccess) { (void)hipGetLastError(); return JSORB_ERR_HIP; }
    if (hipMalloc(&a.flags, flag_words * sizeof(unsigned)) != hipSuccess || hipMemset(a.flags, 0, flag_words * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(a.data);
        if (a.flags) (void)hipFree(a.flags);
        return JSORB_ERR_HIP;
    }
    g_arenas.push_back(a);
    *data = a.data; *flags = a.flags;
    return JSORB_OK;
}
void arena_release(unsigned *data)
{
    if (!data) return;
    std::lock_guard<std::mutex> lk(g_arena_mu);
    for (size_t i = 0; i < g_arenas.size(); i++)
        if (g_arenas[i].data == data) {
            if (--g_arenas[i].refs == 0) { (void)hipFree(g_arenas[i].data); (void)hipFree(g_arenas[i].flags); g_arenas.erase(g_arenas.begin() + i); }
            return;
        }
}

int pool_stream(jsorb_extractor *e, int j, hipStream_t *out)
{
    LanePool &p = g_pool[e->device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    if (!p.s[j]) HIPCHK(e, hipStreamCreateWithFlags(&p.s[j], hipStreamNonBlocking));
    *out = p.s[j];
    return JSORB_OK;
}

// ONE upload stream per device for the host batches of every handle.  The regime is PCIe-bound, so the ORDER of the uploads is what
// matters: left chunks then right chunks, each at full bandwidth, in the order the lanes consume them.  With a copy stream per handle
// the left and right uploads ran concurrently on two SDMA engines at half speed each and every lane got its images later.
int pool_copy_stream(jsorb_extractor *e, hipStream_t *out)
{
    LanePool &p = g_pool[e->device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    if (!p.copy) {
        int least = 0, greatest = 0;
        HIPCHK(e, hipDeviceGetStreamPriorityRange(&least, &greatest));
        const int prio = experiment_env("JSORB_COPY_PRIORITY") ? std::max(greatest, std::min(least, atoi(experiment_env("JSORB_COPY_PRIORITY")))) : greatest;
        HIPCHK(e, hipStreamCreateWithPriority(&p.copy, hipStreamNonBlocking, prio));
    }
    *out = p.copy;
    return JSORB_OK;
}

// Main streams are recycled, never destroyed: which hardware queue HIP gives a new stream depends on every stream created and destroyed
// before it, and a process that had closed one handle pair and opened another (same code, same sizes) measured 57 k instead of 68 k
// pairs/s in the host-streamed regime.  With recycled streams the stream -> queue assignment of the process settles once.
int pool_main_stream(jsorb_extractor *e, hipStream_t *out)
{
    LanePool &p = g_pool[e->device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    if (!p.idle_main.empty()) { *out = p.idle_main.back(); p.idle_main.pop_back(); return JSORB_OK; }
    HIPCHK(e, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return JSORB_OK;
}
void pool_return_main_stream(int device, hipStream_t s)
{
    LanePool &p = g_pool[device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    p.idle_main.push_back(s);
}

inline hipStream_t lane_stream(const jsorb_extractor *e, int j) { return e->lane_used[j]; }      // of the LAST batch

// Split n images into contiguous lanes.  A lane keeps at least ~7 Mpx of level-0 pixels (about 20 images of 752x480) so that each
// launch still fills the 256 CUs; per-kernel timing (which serialises launches anyway) and small batches use one lane.
int plan_lanes(const jsorb_extractor *e, int n, int *first)
{
    const double px = (double)e->g.lv[0].H * e->g.lv[0].W;
    const int min_per_lane = std::max(1, (int)std::ceil(e->lane_min_px / px));
    int K = std::min(std::min(e->max_lanes, e->lane_cap), n / min_per_lane);
    if (K < 1 || e->timing) K = 1;
    // lane sizes in units of 8 images where possible: the XCD-aware workgroup mapping (xcd_map) pads a launch to a multiple of 8 images,
    // and 43 + 43 + 42 images cost 10 % more workgroup slots than 48 + 40 + 40 (measured: 3 uneven lanes 77.8 k, 4 even lanes 84.8 k pairs/s)
    const int unit = n >= 8 * K ? 8 : 1;
    const int units = n / unit, base = units / K, rem = units % K;
    first[0] = 0;
    for (int j = 0; j < K; j++) first[j + 1] = first[j] + unit * (base + (j < rem ? 1 : 0));
    first[K] = n;                                   // the last lane takes the remainder (< 8 images)
    return K;
}

// Orders the lanes of a NEW batch (K lanes over n images) after everything that touched the handle's buffers before:
//  * work the caller (or this handle) enqueued on the main stream: lanes >= 1 wait for a fork event recorded on lane 0
//  * the previous batch of this handle, when its lane partition differs (same partition: same-stream order is enough)
//  * a stereo match enqueued on ANOTHER handle's lanes that may still read this handle's previous results
//  * `input_ready` (optional, one event per lane): e.g. the upload of the lane's images on the copy stream
int order_lanes_for_new_batch(jsorb_extractor *e, int K, int n, const hipStream_t *ls, const hipEvent_t *input_ready)
{
    if ((K > 1 || ls[0] != e->stream) && (e->stream != e->own_stream || e->main_stream_dirty)) {
        // a caller-provided main stream (or copies this call put on the main stream) may carry work the images depend on.  The
        // handle's OWN stream only ever carries this handle's work, which the lanes order themselves against below.
        HIPCHK(e, hipEventRecord(e->ev_fork, e->stream));
        for (int j = 0; j < K; j++)
            if (ls[j] != e->stream) HIPCHK(e, hipStreamWaitEvent(ls[j], e->ev_fork, 0));
    }
    e->main_stream_dirty = false;
    if (e->extracted) {         // the previous batch of this handle: wherever a lane now runs on another stream than the lane that last touched its images
        const bool same_split = K == e->K && n == e->n_images;
        for (int j = 0; j < K; j++)
            for (int i = 0; i < e->K; i++)
                if ((same_split ? i == j : true) && e->lane_used[i] != ls[j]) HIPCHK(e, hipStreamWaitEvent(ls[j], e->lane_done[i], 0));
    }
    if (e->has_readers) {       // a stereo match enqueued through ANOTHER handle may still read this handle's previous results
        const bool aligned = e->readers_K == K && e->readers_n == n;
        for (int j = 0; j < K; j++)
            for (int i = 0; i < e->readers_K; i++)
                if ((aligned ? i == j : true) && e->readers_stream[i] != ls[j]) HIPCHK(e, hipStreamWaitEvent(ls[j], e->lane_readers_done[i], 0));
        e->has_readers = false;
    }
    if (input_ready)            // per lane: e.g. the upload of this lane's images on the copy stream
        for (int j = 0; j < K; j++) HIPCHK(e, hipStreamWaitEvent(ls[j], input_ready[j], 0));
    return JSORB_OK;
}

// ---- the single-frame graph (struct jsorb_extractor: frame_graph*) ----
void frame_graph_drop(jsorb_extractor *e)
{
    if (e->frame_graph) { (void)hipGraphExecDestroy(e->frame_graph); e->frame_graph = nullptr; }
    if (e->frame_graph_tmpl) { (void)hipGraphDestroy(e->frame_graph_tmpl); e->frame_graph_tmpl = nullptr; }
    e->fg_describe_node = nullptr;
    memset(e->fg_key, 0, sizeof e->fg_key);
}

hipGraphNode_t frame_graph_find_describe(hipGraph_t graph)
{
    size_t n = 0;
    if (hipGraphGetNodes(graph, nullptr, &n) != hipSuccess || n == 0 || n > 64) return nullptr;
    hipGraphNode_t nodes[64];
    if (hipGraphGetNodes(graph, nodes, &n) != hipSuccess) return nullptr;
    for (size_t i = 0; i < n; i++) {
        hipGraphNodeType t;
        if (hipGraphNodeGetType(nodes[i], &t) != hipSuccess || t != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams p{};
        if (hipGraphKernelNodeGetParams(nodes[i], &p) == hipSuccess && p.func == describe_kernel_address()) return nodes[i];
    }
    return nullptr;
}

// The captured k_describe node writes the frame's keypoints / descriptors also into caller-owned device buffers (struct Deliver).  When
// the caller's buffers differ from the ones in the executable graph - every frame with the reference's Frame, whose SyncedMem members
// are per-Frame objects - the node's parameters are updated in place (a few microseconds on the host) instead of re-capturing the graph
// (which the first version did, giving up on graphs after 8 frames).  false: not possible, capture again.
bool frame_graph_set_destinations(jsorb_extractor *e)
{
    if (e->deliver_kp_dev == e->fg_dst_kp && e->deliver_desc_dev == e->fg_dst_desc) return true;
    if (!e->fg_describe_node || !e->frame_graph) return false;
    hipKernelNodeParams p{};
    if (hipGraphKernelNodeGetParams(e->fg_describe_node, &p) != hipSuccess || !p.kernelParams) { (void)hipGetLastError(); return false; }
    Deliver *dl = static_cast<Deliver *>(p.kernelParams[describe_kernel_deliver_arg()]);
    if (!dl) return false;
    dl->kp_dev = e->deliver_kp_dev;
    dl->desc_dev = e->deliver_desc_dev;
    if (hipGraphExecKernelNodeSetParams(e->frame_graph, e->fg_describe_node, &p) != hipSuccess) { (void)hipGetLastError(); return false; }
    e->fg_dst_kp = e->deliver_kp_dev; e->fg_dst_desc = e->deliver_desc_dev;
    return true;
}

int run_pipeline(jsorb_extractor *e, int n, const hipEvent_t *input_ready = nullptr)
{
    const Geometry &g = e->g;
    int first[JSORB_MAX_LANES + 1];
    const int K = plan_lanes(e, n, first);
    hipStream_t ls[JSORB_MAX_LANES];
    int rc;
    if (K == 1) ls[0] = e->stream;                  // one lane (single frame, small batch, per-kernel timing): the handle's main stream
    else
        for (int j = 0; j < K; j++)
            if ((rc = pool_stream(e, j, &ls[j]))) return rc;
    if ((rc = order_lanes_for_new_batch(e, K, n, ls, input_ready))) return rc;
    const size_t T = (size_t)g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    // k_compact writes the counts of every image straight into the pinned host mirror (no copy behind the kernels, for batches as
    // well); for a single image k_describe also delivers keypoints and descriptors there and into the caller's device buffers
    // (jsorb_extract_into)
    const bool direct = n == 1;
    for (int j = 0; j < K; j++) {
        const int f = first[j], m = first[j + 1] - f;
        hipStream_t st = ls[j];
        ImageSrc src = e->src;
        src.l0 += (size_t)f * src.l0_stride;
        uint8_t *slab = e->slab + (size_t)f * g.slab_bytes, *blur = e->blur + (size_t)f * g.slab_bytes;
        unsigned long long *tile_out = e->tile_out + f * T, *kp = e->kp + f * T;
        int *counts = e->counts + f * CW;
        const ImageSrc raw = src;                   // with maps: the raw input k_rectify reads; level 0 is then its output in the slab
        if (e->rect_on) { src.l0 = slab; src.l0_stride = g.slab_bytes; src.l0_pitch = g.lv[0].pitch; }
        if (e->copy_kind == 1 && e->rect_on) {
            for (int i = f; i < f + m; i++)
                HIPCHK(e, hipMemcpy2DAsync(e->rect_raw + (size_t)i * raw.l0_stride, raw.l0_pitch, e->copy_src + (size_t)i * e->copy_stride, e->copy_step,
                                           g.lv[0].W, g.lv[0].H, hipMemcpyHostToDevice, st));
        } else if (e->copy_kind == 1) {
            for (int i = f; i < f + m; i++)
                HIPCHK(e, hipMemcpy2DAsync(e->slab + (size_t)i * g.slab_bytes, g.lv[0].pitch, e->copy_src + (size_t)i * e->copy_stride, e->copy_step,
                                           g.lv[0].W, g.lv[0].H, hipMemcpyHostToDevice, st));
        } else if (e->copy_kind == 2) {
            launch_copy_level0(e->copy_src + (size_t)f * e->copy_stride, e->copy_stride, e->copy_step, e->slab + (size_t)f * g.slab_bytes, g.slab_bytes,
                               g.lv[0].pitch, g.lv[0].W, g.lv[0].H, m, st);
        }
        // single image on an untimed handle: replay the captured graph of the five launches when nothing they depend on has changed
        bool capturing = false;
        // (only on the handle's own stream: a caller-provided stream may be the legacy / null stream, which cannot be captured, and a capture
        // that fails half way would leave the CALLER's stream in capture mode)
        if (direct && e->use_frame_graph && !e->timing && !e->nms_ms && st == e->own_stream) {
            // The caller-owned destinations (jsorb_extract_into) are NOT part of the key: the reference's Frame builds fresh SyncedMem members
            // every frame, so they change from frame to frame - the k_describe node of the instantiated graph gets them patched in
            // (frame_graph_set_destinations) instead of the graph being captured again.
            const void *key[6] = {e->src.l0, (const void *)(uintptr_t)e->src.l0_pitch, st, e->rect_on ? e->rect_buf : nullptr, e->cam_on ? e->un : nullptr,
                                  e->upload_pending ? e->h_upload : nullptr};      // (jsorb_set_camera drops the graph: the camera is a kernel argument)
            if (e->frame_graph && memcmp(key, e->fg_key, sizeof key) == 0) {
                e->fg_recaptures = 0;
                if (!frame_graph_set_destinations(e)) { /* fall through to a fresh capture */ }
                else {
                    HIPCHK(e, hipGraphLaunch(e->frame_graph, st));
                    HIPCHK(e, hipEventRecord(e->lane_done[j], st));
                    if (e->upload_pending && !e->sync_single) { HIPCHK(e, hipEventRecord(e->ev_upload_read, st)); e->upload_inflight = true; }
                    continue;
                }
            }
            frame_graph_drop(e);
            if (++e->fg_recaptures > 8) e->use_frame_graph = 0;      // a caller that rotates its INPUT buffers: plain launches are cheaper than re-capturing
            if (e->use_frame_graph) {
                memcpy(e->fg_key, key, sizeof key);
                e->fg_dst_kp = e->deliver_kp_dev; e->fg_dst_desc = e->deliver_desc_dev;
                HIPCHK(e, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
                capturing = true;
            }
        }
        // (a software pipeline across the lanes - stage s of lane j behind stage s of lane j-1 - was measured slower than free-running lanes: 77.8 k
        // against 80 k pairs/s in round 2; removed in round 6)
        // (experiments build only: JSORB_SKIP_KERNELS = bit mask of kernel ids whose launches are left out - WRONG results, what is measured is a kernel's
        // marginal cost inside the overlapped pipeline; tools/micro/r6_exp3.sh)
        const int skip_mask = experiment_env("JSORB_SKIP_KERNELS") ? atoi(experiment_env("JSORB_SKIP_KERNELS")) : 0;      // (read per call: the driver warms up with every kernel, then sets it)
#define JSORB_STAGE(id, launch_stmt) do { if (!((skip_mask >> (id)) & 1)) TIMED(e, id, launch_stmt); } while (0)
        if (e->upload_pending) launch_upload_level0(e->h_upload, e->stage[0], (size_t)g.lv[0].H * g.lv[0].W, st);
        if (e->rect_on)
            JSORB_STAGE(JSORB_K_RECTIFY, launch_rectify(e->rmap, raw.l0, raw.l0_stride, raw.l0_pitch, slab, g.slab_bytes, g.lv[0].pitch, g.lv[0].W, g.lv[0].H, m, st));
        JSORB_STAGE(JSORB_K_PYRAMID, launch_pyramid(g, src, slab, e->lut_bits, m, e->pyr_lds, st));
        // single image: k_detect and k_blur (independent of each other) as ONE launch - a frame is a chain of small launches whose latencies add up
        static const bool fuse_env = !env_is(experiment_env("JSORB_FUSED_DETECT_BLUR"), 0);
        const bool fused = direct && fuse_env && !e->timing && g.blur_blocks > 0 && !g.det_compact && e->detect_lds + 12 * 1024 <= 64 * 1024;      // (k_blur's 10 KB of static LDS come on top of k_detect's request)
        // Lane order of a batch (round 6; every arm measured A/B on one box, profiles/r06_experiments.txt).  The lanes of a batch start together and run
        // the same stages at the same time; on handles with many keypoints per image (the yaml tiles: tile height <= 40) the ODD lanes therefore run
        // k_blur BEFORE k_detect (the two are independent: both read the pyramid), and the even lanes' k_compact rides inside their k_blur launch
        // (k_blur_compact, k_blur.hip; k_compact as a launch of its own is a bubble in its lane): C2 +1.3 %, C5 +1.7 %, C3 +-0 against one order for all
        // lanes.  With large tiles (few keypoints, k_detect most of the step) the same order costs 1-2.5 %: those handles keep the plain order.
        // Not while per-kernel timing is on (stages are timed one by one then).
        // SMALL launches and ODD lane counts (end of round 6): what the alternating order gains grows with the size of a lane's launches, what the fused
        // launch saves - one launch and its dependency gap per extract - does not, and with three lanes the alternation is lopsided.  Below 24 megapixels of
        // pyramid per lane and launch (16 KITTI-shaped images: a 64-pair step), or with an odd number of lanes (64 EuRoC-shaped images: 24 + 24 + 16), every
        // lane runs the plain order with the fused launch: +3 % in both cases; +-0.6 % between 24 and 36 MPx, -1 ... -4.5 % above (twelve geometry / batch
        // combinations, tools/micro/r6_lane_order.sh, log sections 33-35).
        // A batch too small to be split (one lane) takes the fused launch as well when its compaction workgroup is short (<= CMP_MID_T tiles: +8 ... 10 % at 8 / 16
        // EuRoC-shaped and 12 KITTI-shaped pairs; the 21 053 tiles of the KAIST shape outlast so small a k_blur launch: -13 %, those keep k_compact's own launch).
        // JSORB_LANE_ORDER (experiments build): 0 - every lane plain order with the fused launch, 1 - alternating, 2 - plain order, nothing fused.
        double lane_mpx = 0;
        for (int l = 0; l < g.L; l++) lane_mpx += (double)g.lv[l].W * g.lv[l].H;
        lane_mpx *= (double)n / K * 1e-6;
        const int lane_order = experiment_env("JSORB_LANE_ORDER") ? atoi(experiment_env("JSORB_LANE_ORDER"))
                                                                  : ((K & 1) || lane_mpx < JSORB_FUSE_ALL_BELOW_MPX ? 0 : (g.lv[0].th <= 40 ? 1 : 2));      // (tall tiles as well: C3 / tile 46 +1.1 %, C2 / tile 58 with 64 pairs +1.7 %)
        const bool blur_first = !fused && K > 1 && (j & 1) && lane_order == 1;
        const bool fuse_bc = !fused && !direct && (K > 1 || g.T <= CMP_MID_T) && !blur_first && !e->timing && lane_order != 2 && blur_compact_fusable(g);
        if (blur_first) JSORB_STAGE(JSORB_K_BLUR, launch_blur(g, src, slab, blur, e->lut_bits, m, st));
        if (fused) JSORB_STAGE(JSORB_K_DETECT, launch_detect_blur(g, src, slab, e->mask, e->lut_bits, tile_out, blur, e->detect_lds, st));
        else JSORB_STAGE(JSORB_K_DETECT, launch_detect(g, src, slab, e->mask, e->lut_bits, tile_out, m, e->detect_lds, st, e->det_spill, e->det_spill_flags));
        if (e->nms_ms)
            JSORB_STAGE(JSORB_K_NMS_MS, launch_nms_ms(g, tile_out, e->ms_grid ? e->ms_grid + (size_t)f * g.lv[0].H * g.lv[0].W : nullptr,
                                                      e->ms_scratch ? e->ms_scratch + f * T : nullptr, e->p.nms_ms_mode_gpu, m, st));
        if (fuse_bc) JSORB_STAGE(JSORB_K_BLUR, launch_blur_compact(g, src, slab, blur, e->lut_bits, m, st, tile_out, kp, counts, e->row_tab + (size_t)f * g.row_tab_stride, e->h_counts + f * CW));
        else {
            JSORB_STAGE(JSORB_K_COMPACT, launch_compact(g, tile_out, kp, counts, e->row_tab + (size_t)f * g.row_tab_stride, m, st, e->h_counts + f * CW));
            if (!fused && !blur_first) JSORB_STAGE(JSORB_K_BLUR, launch_blur(g, src, slab, blur, e->lut_bits, m, st));
        }
        JSORB_STAGE(JSORB_K_DESCRIBE, launch_describe(g, src, slab, blur, kp, counts, e->angles + f * T, e->desc + f * T * 32, e->out_kp + f * T * 6, m, st,
                                                      direct ? Deliver{e->deliver_kp_dev, e->deliver_desc_dev, e->h_kp, e->h_desc, nullptr}
                                                             : Deliver{nullptr, nullptr, nullptr, nullptr, nullptr}));
        if (e->cam_on)      // Frame::UndistortKeyPoints (Frame.cpp:718-748) behind the extraction, on the device counts
            JSORB_STAGE(JSORB_K_UNDISTORT, launch_undistort(e->cam, e->out_kp + f * T * 6, counts, (int)T, e->un + f * T * 2, direct ? e->h_un : nullptr, m, st));
#undef JSORB_STAGE
        if (capturing) {
            // Whatever happened between Begin and End (a launch error included), the stream must leave capture mode; on any failure the
            // partial graph is dropped, the key forgotten, graphs switched off for this handle and the frame re-issued as plain launches.
            hipGraph_t graph = nullptr;
            const hipError_t launch_err = hipGetLastError();
            const hipError_t ec = hipStreamEndCapture(st, &graph);
            hipError_t gi = ec != hipSuccess ? ec : launch_err;
            if (gi == hipSuccess) gi = hipGraphInstantiate(&e->frame_graph, graph, nullptr, nullptr, 0);
            if (gi == hipSuccess) {
                e->frame_graph_tmpl = graph;                 // kept: its k_describe node is the handle for later parameter updates
                e->fg_describe_node = frame_graph_find_describe(graph);
                gi = hipGraphLaunch(e->frame_graph, st);
            } else if (graph) (void)hipGraphDestroy(graph);
            if (gi != hipSuccess) {
                (void)hipGetLastError();
                frame_graph_drop(e);
                e->use_frame_graph = 0;
                j--;                                         // redo this lane without a graph
                continue;
            }
        }
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->lane_done[j], st));
        if (e->upload_pending && !e->sync_single) { HIPCHK(e, hipEventRecord(e->ev_upload_read, st)); e->upload_inflight = true; }      // (recorded behind the frame: an event record inside the captured graph is not an option on this runtime)
    }
    e->copy_kind = 0;
    e->un_valid = e->cam_on;
    e->un_mirror = direct && e->cam_on;
    e->rgbd_images = 0;
    e->rgbd_mirror = false;
    if (e->rect_on) { e->src.l0 = e->slab; e->src.l0_stride = g.slab_bytes; e->src.l0_pitch = g.lv[0].pitch; }
    e->upload_pending = false;
    e->mirror_pending = direct;
    e->deliver_kp_dev = nullptr;
    e->deliver_desc_dev = nullptr;
    e->K = K;
    for (int j = 0; j <= K; j++) e->lane_first[j] = first[j];
    for (int j = 0; j < K; j++) e->lane_used[j] = ls[j];
    if (K > 1 && e->stream != e->own_stream)        // a caller-provided main stream observes the batch: whatever the caller enqueues on it next runs after the lanes
        for (int j = 0; j < K; j++) HIPCHK(e, hipStreamWaitEvent(e->stream, e->lane_done[j], 0));
    e->n_images = n;
    e->extracted = true;
    e->stereo_done = false;
    e->counts_synced = false;
    return JSORB_OK;
}

StereoArgs make_stereo_args(float mb, float mbf, int th_high, int th_low)
{
    StereoArgs sa;
    sa.maxD = mbf / mb;                  // const float maxD = mbf/minZ  (orb_stereo_match.cu:144-146)
    sa.mbf = mbf;
    sa.th_high = th_high;
    sa.th_orb = (th_high + th_low) / 2;
    return sa;
}

// ---- speculative stereo (struct jsorb_spec_state) ----
// Before a handle's buffers are rewritten: the speculative kernels of the previous frame read them (both handles' keypoints,
// descriptors, row tables and level images, the landing buffers included).  A single image is ordered on the GPU (its copy and
// kernels go to e->stream); a batch, whose copies and lanes use other streams, waits on the host (rare: a pair that alternates
// between the two call shapes).  Any new extract also invalidates a result nobody has asked for.
int spec_guard(jsorb_extractor *e, int n)
{
    jsorb_spec_state *S = e->spec;
    if (!S) return JSORB_OK;
    std::lock_guard<std::mutex> lk(S->mu);
    bool &need = e == S->l ? S->wait_l : S->wait_r;
    if (need) {
        if (n == 1) HIPCHK(e, hipStreamWaitEvent(e->stream, S->ev_done, 0));
        else HIPCHK(e, hipEventSynchronize(S->ev_done));
        need = false;
    }
    if (S->inflight) { S->inflight = false; S->n_dropped++; }
    return JSORB_OK;
}

// After a handle has enqueued an extract.  The second of the two handles to get here for the same new frame enqueues the match.
// Failures only disarm the pair (the caller's jsorb_stereo_match then runs the normal path and reports its own errors).
void spec_after_extract(jsorb_extractor *e, int n)
{
    jsorb_spec_state *S = e->spec;
    if (!S) { e->spec_seq++; return; }
    std::lock_guard<std::mutex> lk(S->mu);
    e->spec_seq++;
    e->spec_single = n == 1 && !e->timing;
    jsorb_extractor *l = S->l, *r = S->r;
    if (!S->armed || !l->spec_single || !r->spec_single) return;
    if (l->spec_seq - S->l_base != r->spec_seq - S->r_base || l->spec_seq == S->l_base) return;     // not the same new frame on both sides (yet)
    // on the stream of the extract that was enqueued LAST (this one): it is the one that finishes last, so the match follows it in stream
    // order and the event of the other extract has usually fired by then (a cross-stream wait that is still pending when the GPU
    // reaches it costs ~20 us of idle time on this path).  Own scratch: a normal match on l's stream may follow while this one runs.
    jsorb_extractor *other = e == l ? r : l;
    hipStream_t st = e->lane_used[0];
    bool ok = true;
    if (other->lane_used[0] != st) ok = hipStreamWaitEvent(st, other->lane_done[0], 0) == hipSuccess;
    if (ok) {
        const StereoArgs sa = make_stereo_args(S->mb, S->mbf, S->th_high, S->th_low);
        launch_stereo(l->g, l->src, l->slab, r->src, r->slab, l->out_kp, l->counts, l->desc, r->out_kp, r->counts, r->desc, r->row_tab,
                      l->sp_u, l->sp_d, l->sp_l1, l->sp_aux, sa, 1, st, nullptr);
        launch_median(l->g, l->counts, l->sp_u, l->sp_d, l->sp_l1, l->sp_aux, l->sp_stats, 1, st, DeliverStereo{l->h_sp_u, l->h_sp_d, l->h_sp_stats});
        ok = hipGetLastError() == hipSuccess && hipEventRecord(S->ev_done, st) == hipSuccess;
        // whatever went out on the stream reads both handles' buffers: their next extracts are ordered after it in any case
        S->wait_l = S->wait_r = true;
    }
    if (!ok) { S->armed = false; return; }
    S->inflight = true;
    S->l_seq = l->spec_seq;
    S->r_seq = r->spec_seq;
}

void spec_detach(jsorb_spec_state *S)
{
    if (!S) return;
    {
        std::lock_guard<std::mutex> lk(S->mu);
        S->armed = false;
        if (S->wait_l || S->wait_r || S->inflight) (void)hipEventSynchronize(S->ev_done);
    }
    if (S->l) S->l->spec = nullptr;
    if (S->r) S->r->spec = nullptr;
    if (S->ev_done) (void)hipEventDestroy(S->ev_done);
    delete S;
}

// Called by a synchronous single-pair jsorb_stereo_match that ran the normal path: from now on the pair is matched speculatively.
int spec_arm(jsorb_extractor *l, jsorb_extractor *r, float mb, float mbf, int th_high, int th_low)
{
    if (l->spec && (l->spec->l != l || l->spec->r != r)) spec_detach(l->spec);
    if (r->spec && (r->spec->l != l || r->spec->r != r)) spec_detach(r->spec);
    if (!l->spec) {
        const size_t B = (size_t)l->B, T = (size_t)l->g.T;
        if (!l->sp_u) {
            HIPCHK(l, hipMalloc(&l->sp_u, B * T * 4));
            HIPCHK(l, hipMalloc(&l->sp_d, B * T * 4));
            HIPCHK(l, hipMalloc(&l->sp_stats, B * 8 * sizeof(int)));
            HIPCHK(l, hipMalloc(&l->sp_l1, T * 4));
            HIPCHK(l, hipMalloc(&l->sp_aux, T * 4));
            HIPCHK(l, hipHostMalloc(&l->h_sp_u, T * sizeof(float)));
            HIPCHK(l, hipHostMalloc(&l->h_sp_d, T * sizeof(float)));
            HIPCHK(l, hipHostMalloc(&l->h_sp_stats, B * 8 * sizeof(int)));
        }
        jsorb_spec_state *S = new (std::nothrow) jsorb_spec_state;
        if (!S) { l->err = "out of memory (speculative stereo)"; return JSORB_ERR_HIP; }
        if (hipEventCreateWithFlags(&S->ev_done, hipEventDisableTiming) != hipSuccess) { delete S; l->err = "hipEventCreate (speculative stereo)"; return JSORB_ERR_HIP; }
        S->l = l; S->r = r;
        l->spec = r->spec = S;
    }
    jsorb_spec_state *S = l->spec;
    std::lock_guard<std::mutex> lk(S->mu);
    S->armed = true;
    S->mb = mb; S->mbf = mbf; S->th_high = th_high; S->th_low = th_low;
    S->l_base = l->spec_seq;
    S->r_base = r->spec_seq;
    if (S->inflight) { S->inflight = false; S->n_dropped++; }
    return JSORB_OK;
}

bool check_image(const jsorb_extractor *e, int image) { return e && e->extracted && image >= 0 && image < e->n_images; }

} // namespace

extern "C" {

const char *jsorb_version(void) { return "jsorb 0.1 (gfx950)"; }

const char *jsorb_kernel_name(int id)
{
    if (id >= 0 && id < JSORB_K_COUNT_ALL) return k_names[id];
    if (id >= JSORB_K_ASSIGN_GRID && id < JSORB_K_ID_END) return k_names_local[id - JSORB_K_ASSIGN_GRID];
    return "";
}

const char *jsorb_last_error(const jsorb_extractor *e) { return e ? e->err.c_str() : "null handle"; }

int jsorb_create(const jsorb_params *params, const uint8_t *mask, jsorb_extractor **out)
{
    return jsorb_create_masked(params, mask, params ? params->width : 0, params ? params->height : 0, out);
}

// host-only part of a handle's launch plan for k_detect (also behind jsorb_plan_launch)
static void plan_detect(Geometry &g, bool compact_possible = true)
{
    for (int i = 0; i < g.L; i++) {                        // needed by the LDS layout: the arg-max form needs 256 B where the literal tree needs 1 KB
        uint8_t tr[256];
        g.lv[i].tree_rank_ok = (build_tree_rank(g.lv[i].tw, g.lv[i].log2_tw, tr, tr + 128) && !experiment_env("JSORB_FORCE_TREE_REPLAY")) ? 1 : 0;
    }
    // Batch handles run k_detect's compact form (score plane built late, on top of the dead image tile; positives in an LDS pool that spills into a
    // borrowed chunk of global memory: 7 workgroups per CU instead of 4).  Round 5 kept the full-plane form for tiles above 40 rows (the "1000 / 2000 /
    // 3000 features" tiles 58 / 46 / 52), where the compact kernel was 20-30 % faster alone and the 4-lane pipeline no faster.  Round 6 found what ate
    // the difference - k_compact's 1024-thread workgroups starving behind the fuller CUs (k_compact.hip) - and with 256-thread compaction the compact
    // form wins at every tile size (A/B on one box, pairs/s full-plane -> compact: tile 58 148.4 k -> 150.1 k, C3 tile 46 111.7 k -> 114.7 k, C5 tile 52
    // 53.1 k -> 55.6 k; profiles/r06_experiments.txt).  Single-image handles keep the full-plane form (one image does not fill the chip).
    // JSORB_DETECT_FULLPLANE=1 / 0 forces the full-plane / the compact form on a batch handle (A/B measurements, tests).
    const char *force = product_env("JSORB_DETECT_FULLPLANE");
    const bool want_compact = force ? atoi(force) == 0 : true;
    g.det_compact = (!g.latency && want_compact && compact_possible) ? 1 : 0;
    fill_detect_layout(g);
}

/* Host-only (no device is touched): the launch plan a handle with these parameters gets - what tests/test_round5_host_logic.py checks the LDS
 * layouts against.  out[0..7] = levels, compact form (0 / 1), k_detect LDS bytes (before jsorb_create's per-CU partition adjustment of the full-plane
 * form), spill chunks in the handle's arena, k_pyramid LDS bytes, k_detect workgroups per image, entries of a spill chunk, 0; then 8 ints
 * per level: det_R, k_tiles, pool entries, score-plane stride, survivor-list capacity, pyr_ns16, the NS k_pyramid instantiates for it, tile rows. */
int jsorb_plan_launch(const jsorb_params *params, int32_t *out, int capacity)
{
    if (!params || !out) return JSORB_ERR_INVALID;
    Geometry g;
    std::string err;
    const int rc = build_geometry(*params, g, err);
    if (rc) return rc;
    plan_detect(g);
    if (capacity < 8 + 8 * g.L) return JSORB_ERR_INVALID;
    out[0] = g.L; out[1] = g.det_compact; out[2] = (int32_t)detect_lds_bytes(g); out[3] = g.det_compact ? (int32_t)detect_arena_flag_words() : 0;
    out[4] = (int32_t)pyramid_lds_bytes(g); out[5] = g.detect_blocks; out[6] = g.det_compact ? detect_spill_chunk_entries(g) : 0; out[7] = 0;
    for (int i = 0; i < g.L; i++) {
        int32_t *o = out + 8 + 8 * i;
        o[0] = g.lv[i].det_R; o[1] = g.lv[i].k_tiles; o[2] = g.det_compact ? g.lv[i].det_pos_cap : 0; o[3] = g.lv[i].det_score_stride;
        o[4] = g.lv[i].det_list_cap; o[5] = g.lv[i].pyr_ns16; o[6] = pyramid_ns_dispatched(g.lv[i].pyr_ns16); o[7] = g.lv[i].nth;
    }
    return JSORB_OK;
}

int jsorb_create_masked(const jsorb_params *params, const uint8_t *mask, int mask_width, int mask_height, jsorb_extractor **out)
{
    if (!params || !out) return JSORB_ERR_INVALID;
    if (mask && (mask_width < 1 || mask_height < 1)) return JSORB_ERR_INVALID;
    *out = nullptr;
    jsorb_extractor *e = new (std::nothrow) jsorb_extractor();
    if (!e) return JSORB_ERR_INVALID;
    // on any failure the handle is still returned so that jsorb_last_error can be read; the caller destroys it
    *out = e;
    e->p = *params;
    e->B = params->max_batch < 1 ? 1 : params->max_batch;
    e->device = params->device_id;
    e->nms_ms = params->apply_nms_ms && params->n_levels > 1;      // auto-disabled for one level (orb_gpu.cpp:37)
    int rc = build_geometry(*params, e->g, e->err);
    if (rc) return rc;
    Geometry &g = e->g;
    g.has_mask = mask ? 1 : 0;
    HIPCHK(e, hipSetDevice(e->device));
    { int rc = pool_main_stream(e, &e->own_stream); if (rc) return rc; }
    e->stream = e->own_stream;
    HIPCHK(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    for (int j = 0; j < JSORB_MAX_LANES; j++) {      // the extra lane STREAMS are created on first use (run_pipeline): a single-frame handle never needs them
        HIPCHK(e, hipEventCreateWithFlags(&e->lane_done[j], hipEventDisableTiming));
        HIPCHK(e, hipEventCreateWithFlags(&e->lane_readers_done[j], hipEventDisableTiming));
    }
    if (const char *ml = product_env("JSORB_MAX_LANES")) e->max_lanes = std::max(1, std::min(JSORB_MAX_LANES, atoi(ml)));
    if (const char *sw = experiment_env("JSORB_SPIN_WAIT")) e->spin_wait = atoi(sw);
    if (const char *sp = product_env("JSORB_SPECULATE")) { e->speculate_env = atoi(sp) != 0; e->speculate = e->speculate_env; }
    if (const char *ku = experiment_env("JSORB_KERNEL_UPLOAD")) e->kernel_upload = atoi(ku);
    if (const char *hl = experiment_env("JSORB_HOST_LANES")) e->host_lanes = std::max(1, std::min(JSORB_MAX_LANES, atoi(hl)));
    if (const char *tr = experiment_env("JSORB_TRACE_HOST")) e->trace_host = atoi(tr) != 0;
    if (const char *fg = product_env("JSORB_FRAME_GRAPH")) e->use_frame_graph = atoi(fg);
    if (const char *mp = product_env("JSORB_LANE_MIN_MPX")) e->lane_min_px = std::max(0.01, atof(mp)) * 1e6;
    plan_detect(g);
    if (g.det_compact) {
        // The compact form borrows spill chunks from a per-device arena laid out for 8 XCDs of at most 40 CUs.  Where that does not hold, or the arena
        // cannot be allocated, the handle runs the full-plane form (which needs no global resource) - unless the compact form was asked for by name.
        int cus = 0;
        HIPCHK(e, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
        const bool forced = env_is(product_env("JSORB_DETECT_FULLPLANE"), 0);
        int arc = detect_arena_covers(cus) ? arena_acquire(e, detect_spill_chunk_entries(g), detect_arena_bytes(g), detect_arena_flag_words(), &e->det_spill, &e->det_spill_flags)
                                           : JSORB_ERR_UNSUPPORTED;
        if (arc != JSORB_OK) {
            if (forced) {
                e->err = arc == JSORB_ERR_UNSUPPORTED ? "JSORB_DETECT_FULLPLANE=0: k_detect's spill arena is laid out for 8 XCDs of at most 40 CUs, not for this device"
                                                      : "JSORB_DETECT_FULLPLANE=0: k_detect's spill arena could not be allocated";
                return arc;
            }
            plan_detect(g, false);
        }
    }
    e->detect_lds = detect_lds_bytes(g);
    if (e->detect_lds > 160 * 1024) { e->err = "tile too large for LDS"; return JSORB_ERR_INVALID; }
    // LDS partition of a CU in the batch pipeline (profiles/r04_lds_counters.txt, "LDS request sweep"): the lanes overlap k_detect of one image
    // group with k_describe of another, and what decides whether a k_describe workgroup can start on a CU that k_detect fills is LDS, which
    // is handed out in 1280-byte granules.  The request is therefore raised to the largest one that still lets four k_detect workgroups AND
    // one k_describe workgroup share the 160 KB: (163840 - 30720) / 4 = 33280 B.  One granule more loses k_describe's slot (C2: 119.6 k ->
    // 116.7 k pairs/s), one less admits a fifth k_detect workgroup that takes it (118.2 k; tile 58: 138.7 k against 146.0 k).
    {
        hipFuncAttributes fa{};
        const size_t cu_lds = 160 * 1024, gran = 1280;
        if (!g.det_compact && hipFuncGetAttributes(&fa, describe_kernel_address()) == hipSuccess) {
            const size_t desc = (fa.sharedSizeBytes + gran - 1) / gran * gran;
            const size_t want = desc < cu_lds ? (cu_lds - desc) / 4 / gran * gran : 0;
            if (e->detect_lds <= want) e->detect_lds = want;
        }
        // (experiments build: an explicit request, never below what the layout needs, never above what one workgroup may have - what else fits on a CU next
        // to k_detect is decided by this number)
        if (const char *rq = experiment_env("JSORB_DETECT_LDS_REQUEST")) {
            e->detect_lds = std::max(detect_lds_bytes(g), (size_t)std::max(0, atoi(rq)));
            if (e->detect_lds > 64 * 1024) { e->err = "JSORB_DETECT_LDS_REQUEST: a workgroup may request at most 64 KB of dynamic LDS"; return JSORB_ERR_INVALID; }
        }
    }
    e->pyr_lds = pyramid_lds_bytes(g);
    for (int i = 1; i < g.L; i++)
        if (g.lv[i].pyr_ns16 > 4) { e->err = "pyramid scale too large for the resampler (level scale must stay below 19)"; return JSORB_ERR_INVALID; }
    const size_t B = (size_t)e->B, T = (size_t)g.T;
    const size_t slab_total = B * g.slab_bytes + 4096;
    HIPCHK(e, hipMalloc(&e->slab, slab_total));
    HIPCHK(e, hipMalloc(&e->blur, slab_total));
    HIPCHK(e, hipMemset(e->slab, 0, slab_total));
    HIPCHK(e, hipMemset(e->blur, 0, slab_total));   // blurred image is 0 outside the ROI (Appendix C-2)
    if (g.lv[0].W % 16 == 0) {
        for (int k = 0; k < 2; k++) {
            HIPCHK(e, hipMalloc(&e->stage[k], B * (size_t)g.lv[0].H * g.lv[0].W + 256));
            for (int j = 0; j < JSORB_MAX_LANES; j++) {
                HIPCHK(e, hipEventCreateWithFlags(&e->ev_copied[k][j], hipEventDisableTiming));
                HIPCHK(e, hipEventCreateWithFlags(&e->ev_consumed[k][j], hipEventDisableTiming));
            }
        }
    }
    HIPCHK(e, hipMalloc(&e->lut_bits, (2048 + (size_t)g.detect_blocks + g.blur_blocks + g.pyr_blocks + 64 * JSORB_MAX_LEVELS) * sizeof(uint32_t)));      // arc LUT + workgroup tables + tree priorities
    HIPCHK(e, hipMalloc(&e->tile_out, B * T * 8));
    HIPCHK(e, hipMalloc(&e->kp, B * T * 8));
    HIPCHK(e, hipMalloc(&e->counts, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    HIPCHK(e, hipMalloc(&e->row_tab, B * (size_t)g.row_tab_stride * sizeof(int)));
    HIPCHK(e, hipMalloc(&e->angles, B * T * 4));
    HIPCHK(e, hipMalloc(&e->desc, B * T * 32));
    HIPCHK(e, hipMalloc(&e->out_kp, B * T * 6 * 4));
    HIPCHK(e, hipMalloc(&e->st_u, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st_d, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st_l1, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st_aux, B * T * 4));
    if (e->nms_ms) {
        if (params->nms_ms_mode_gpu) {
            const size_t n = B * (size_t)g.lv[0].H * g.lv[0].W * sizeof(int);
            HIPCHK(e, hipMalloc(&e->ms_grid, n));
            HIPCHK(e, hipMemset(e->ms_grid, 0, n));
        } else {
            if (g.T > 32768 || g.lv[0].nth * g.lv[0].ntw > 65535) { e->err = "NMS-MS CPU mode supports at most 32768 tiles"; return JSORB_ERR_UNSUPPORTED; }
            HIPCHK(e, hipMalloc(&e->ms_scratch, B * T * sizeof(int)));
        }
    }
    HIPCHK(e, hipMalloc(&e->st_stats, B * 8 * sizeof(int)));
    HIPCHK(e, hipMemset(e->counts, 0, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    HIPCHK(e, hipHostMalloc(&e->h_counts, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    HIPCHK(e, hipHostMalloc(&e->h_stats, B * 8 * sizeof(int)));
    memset(e->h_counts, 0, B * (JSORB_MAX_LEVELS + 1) * sizeof(int));
    HIPCHK(e, hipHostMalloc(&e->h_kp, T * 6 * sizeof(int32_t)));
    HIPCHK(e, hipHostMalloc(&e->h_desc, T * 32));
    HIPCHK(e, hipHostMalloc(&e->h_u, T * sizeof(float)));
    HIPCHK(e, hipHostMalloc(&e->h_d, T * sizeof(float)));
    {
        std::vector<uint32_t> bits;
        build_lut_bits(params->fast_n_min, params->fast_n_max, bits);
        g.lut_min_pop = 17;
        g.lut_compass = 1;
        for (int j = 0; j < 65536; j++)
            if ((bits[j >> 5] >> (j & 31)) & 1u) {
                g.lut_min_pop = std::min(g.lut_min_pop, __builtin_popcount(j));
                const int m0 = j & 1, m4 = (j >> 4) & 1, m8 = (j >> 8) & 1, m12 = (j >> 12) & 1;
                if (!((m0 | m8) & (m4 | m12))) g.lut_compass = 0;
            }
        // The 6-bit early rejects accept a superset of the exact ones; that is only allowed where the early rejects are no part of the result, i.e.
        // where the arc LUT alone decides (lut_compass: every accepted mask passes the compass test, so the exact ring test of phase 2 is the whole
        // semantics).  With an arc LUT that accepts masks the reference's early rejects throw away (N_MIN < 9) the exact form stays.
        g.det_swar_t4 = g.lut_compass ? detect_swar6_threshold(g.threshold) : 0;
        {   // reference bit order -> the order k_detect indexes the table with
            std::vector<uint32_t> ref(bits.begin(), bits.begin() + 2048);
            permute_lut_bits(ref, bits.data());
        }
        // workgroup tables (jsorb_device.h, CTAB_*): level | tile row << 4 | tile column << 18
        bits.resize(2048 + (size_t)g.detect_blocks + g.blur_blocks + g.pyr_blocks + 64 * JSORB_MAX_LEVELS, 0u);
        for (int i = 0; i < g.L; i++) {                    // column priorities of K3's horizontal tree (k_detect phase 3/4)
            uint8_t *tr = reinterpret_cast<uint8_t *>(&bits[ctab_tree(g) + 64 * i]);
            (void)build_tree_rank(g.lv[i].tw, g.lv[i].log2_tw, tr, tr + 128);      // tree_rank_ok was decided before the LDS layout (JSORB_FORCE_TREE_REPLAY: test hook)
        }
        for (int i = 0; i < g.L; i++) {
            const LevelDesc &lv = g.lv[i];
            for (int r = 0; r < (lv.nth + lv.det_R - 1) / lv.det_R; r++)          // r: group of det_R tile rows
                for (int gr = 0; gr < lv.groups_per_row; gr++)
                    bits[CTAB_DETECT + lv.detect_blk0 + r * lv.groups_per_row + gr] = (uint32_t)i | ((uint32_t)r << 4) | ((uint32_t)gr << 18);
            for (int wbk = 0; wbk < blur_level_blocks(lv); wbk++)
                bits[ctab_blur(g) + lv.blur_blk0 + wbk] = (uint32_t)i | ((uint32_t)wbk << 4);      // level | workgroup of the level << 4
            if (i >= 1)
                for (int by = 0; by < (lv.H + lv.pyr_th - 1) / lv.pyr_th; by++)
                    for (int bx = 0; bx < lv.pyr_bx; bx++)
                        bits[ctab_pyramid(g) + lv.pyr_blk0 + by * lv.pyr_bx + bx] = (uint32_t)i | ((uint32_t)by << 4) | ((uint32_t)bx << 18);
        }
        HIPCHK(e, hipMemcpy(e->lut_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (mask) {
        // orb_gpu.cpp:77-81: cv::resize(..., CV_INTER_NN) per level, then threshold (>10 -> 255).  The source index is OpenCV's
        // resizeNN one: ifx = 1./(dst/(double)src), sx = min(cvFloor(x*ifx), src-1) - NOT floor(x*src/dst), which differs on
        // exact-integer quotients (752->626 column 313, 480->231 rows 77 and 154, ...).  The source is the mask AT ITS OWN SIZE, every level
        // (level 0 included) resized from it directly as the reference does - resizing to level-0 size first and from there to the levels
        // composes two floor() maps and can pick other source pixels.
        std::vector<uint8_t> m(g.slab_bytes, 0);
        for (int i = 0; i < g.L; i++) {
            const LevelDesc &lv = g.lv[i];
            const double ifx = 1.0 / ((double)lv.W / (double)mask_width), ify = 1.0 / ((double)lv.H / (double)mask_height);
            for (int y = 0; y < lv.H; y++) {
                const int sy = std::min((int)std::floor((double)y * ify), mask_height - 1);
                for (int x = 0; x < lv.W; x++) {
                    const int sx = std::min((int)std::floor((double)x * ifx), mask_width - 1);
                    m[lv.img_off + (size_t)y * lv.pitch + x] = mask[(size_t)sy * mask_width + sx] > 10 ? 255 : 0;
                }
            }
        }
        HIPCHK(e, hipMalloc(&e->mask, g.slab_bytes));
        HIPCHK(e, hipMemcpy(e->mask, m.data(), g.slab_bytes, hipMemcpyHostToDevice));
    }
    HIPCHK(e, hipDeviceSynchronize());
    return JSORB_OK;
}

static inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void jsorb_destroy(jsorb_extractor *e)
{
    if (!e) return;
    if (e->trace_host && e->th_n)
        fprintf(stderr, "[jsorb host trace] extract x%ld: h2d enqueue %.1f us, kernel enqueue %.1f us, wait %.1f us ; stereo x%ld: enqueue %.1f us, wait %.1f us\n",
                e->th_n, e->th_h2d / e->th_n, e->th_enq / e->th_n, e->th_wait / e->th_n, e->th_st_n, e->th_st_n ? e->th_st_enq / e->th_st_n : 0.0,
                e->th_st_n ? e->th_st_wait / e->th_st_n : 0.0);
    (void)hipSetDevice(e->device);
    spec_detach(e->spec);        // waits for a speculative match that still reads this handle's buffers; the partner continues unpaired
    if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    if (e->has_readers)       // a stereo match enqueued through another handle may still be reading this handle's buffers
        for (int j = 0; j < e->readers_K; j++) (void)hipEventSynchronize(e->lane_readers_done[j]);
    frame_graph_drop(e);
    if (e->ev_upload_read) (void)hipEventDestroy(e->ev_upload_read);
    for (int j = 0; j < e->K; j++)
        if (e->lane_used[j]) (void)hipStreamSynchronize(e->lane_used[j]);
    for (auto &t : e->timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    void *bufs[] = {e->stage[0], e->stage[1], e->slab, e->blur, e->mask, e->lut_bits, e->tile_out, e->kp, e->counts, e->row_tab, e->angles, e->desc,
                    e->out_kp, e->st_u, e->st_d, e->st_l1, e->st_stats, e->st_aux, e->st_diag, e->sp_u, e->sp_d, e->sp_stats, e->sp_l1, e->sp_aux, e->ms_grid, e->ms_scratch, e->frame_aos, e->grid_start, e->grid_items, e->rect_buf, e->rect_raw, e->un, e->rg, e->sl_cand, e->sl_stats, e->sl_out};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    arena_release(e->det_spill);      // (every kernel of this handle has finished: the lanes were synchronised above)
    if (e->h_counts) (void)hipHostFree(e->h_counts);
    for (void *hp : {(void *)e->h_kp, (void *)e->h_desc, (void *)e->h_u, (void *)e->h_d, (void *)e->h_sp_u, (void *)e->h_sp_d, (void *)e->h_sp_stats, (void *)e->h_upload, (void *)e->h_un, (void *)e->h_rg, (void *)e->h_depth})
        if (hp) (void)hipHostFree(hp);
    if (e->h_stats) (void)hipHostFree(e->h_stats);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    for (int j = 0; j < JSORB_MAX_LANES; j++) {
        if (e->lane_done[j]) (void)hipEventDestroy(e->lane_done[j]);
        if (e->lane_readers_done[j]) (void)hipEventDestroy(e->lane_readers_done[j]);
    }
    for (int k = 0; k < 2; k++) {
        for (int j = 0; j < JSORB_MAX_LANES; j++) {
            if (e->ev_copied[k][j]) (void)hipEventDestroy(e->ev_copied[k][j]);
            if (e->ev_consumed[k][j]) (void)hipEventDestroy(e->ev_consumed[k][j]);
        }
    }
    {   // uploads of this handle still in flight on the device's copy stream read caller memory and write the landing buffers
        LanePool &lp = g_pool[e->device & 15];
        hipStream_t cs;
        { std::lock_guard<std::mutex> lk(lp.m); cs = lp.copy; }
        if (cs) (void)hipStreamSynchronize(cs);
    }
    if (e->own_stream) { (void)hipStreamSynchronize(e->own_stream); pool_return_main_stream(e->device, e->own_stream); }
    delete e;
}

int jsorb_set_stream(jsorb_extractor *e, void *hip_stream)
{
    if (!e) return JSORB_ERR_INVALID;
    hipStream_t ns = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    if (ns != e->stream && e->extracted) {      // the new main stream continues after whatever the old one (and the lanes) were doing
        HIPCHK(e, hipSetDevice(e->device));
        for (int j = 0; j < e->K; j++) HIPCHK(e, hipStreamWaitEvent(ns, e->lane_done[j], 0));
    }
    e->stream = ns;
    return JSORB_OK;
}
void *jsorb_get_stream(const jsorb_extractor *e) { return e ? (void *)e->stream : nullptr; }

int jsorb_stream_wait_done(jsorb_extractor *e, void *other)
{
    if (!e) return JSORB_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->device));
    for (int j = 0; j < e->K; j++)
        if ((hipStream_t)other != lane_stream(e, j)) HIPCHK(e, hipStreamWaitEvent((hipStream_t)other, e->lane_done[j], 0));
    return JSORB_OK;
}

int jsorb_sync(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->device));
    if (e->extracted && e->K == 1 && e->n_images == 1 && e->spin_wait) {
        // single frame: the whole frame is ~100 us of GPU time, and a blocking hipStreamSynchronize adds tens of microseconds of wake-up
        // latency per call (three calls per stereo frame).  Poll the stream instead (bounded), then fall through to the blocking call.
        for (int it = 0; it < 400000; it++) {
            const hipError_t q = hipStreamQuery(e->stream);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) { e->err = std::string("hipStreamQuery: ") + hipGetErrorString(q); return JSORB_ERR_HIP; }
            __builtin_ia32_pause();
        }
    }
    if (e->extracted)
        for (int j = 0; j < e->K; j++) HIPCHK(e, hipStreamSynchronize(lane_stream(e, j)));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->counts_synced = true;
    if (e->mirror_pending) { e->mirror_valid = true; e->mirror_pending = false; }
    if (e->st_mirror_pending) { e->st_mirror_valid = true; e->st_mirror_pending = false; }
    return drain_timed(e);
}

// Copies into the level-0 plane of the internal slab are enqueued on the main stream BEFORE the lanes of the new batch are ordered:
// the main stream first has to wait for whoever may still read the slab (other lanes of the previous batch, a stereo match).
static int join_previous_on_main(jsorb_extractor *e)
{
    if (e->extracted)
        for (int i = 0; i < e->K; i++)
            if (e->lane_used[i] != e->stream) HIPCHK(e, hipStreamWaitEvent(e->stream, e->lane_done[i], 0));
    if (e->has_readers)
        for (int i = 0; i < e->readers_K; i++)
            if (e->readers_stream[i] != e->stream) HIPCHK(e, hipStreamWaitEvent(e->stream, e->lane_readers_done[i], 0));
    return JSORB_OK;
}

// A landing buffer may be refilled only after every lane that read it in place (extract kernels and, if any, the stereo match)
static int wait_buffer_consumed(jsorb_extractor *e, int k, hipStream_t s)
{
    for (int j = 0; j < e->consumed_K[k]; j++) HIPCHK(e, hipStreamWaitEvent(s, e->ev_consumed[k][j], 0));
    return JSORB_OK;
}
static int mark_buffer_consumed(jsorb_extractor *e, int k)
{
    for (int j = 0; j < e->K; j++) HIPCHK(e, hipEventRecord(e->ev_consumed[k][j], lane_stream(e, j)));
    e->consumed_K[k] = e->K;
    e->consumed_n[k] = e->n_images;
    e->last_stage = k;
    return JSORB_OK;
}

static int wait_event(jsorb_extractor *e, hipEvent_t ev, bool spin);

// *mark: the landing buffer whose "consumed" events the caller records after everything else it enqueues for this call (-1: none)
static int extract_batch_host_enqueue(jsorb_extractor *e, const uint8_t *host_images, size_t image_stride, int step, int n_images, int *mark)
{
    *mark = -1;
    const LevelDesc &l0 = e->g.lv[0];
    const size_t img_bytes = (size_t)l0.H * l0.W;
    int rc;
    if (e->stage[0] && step == l0.W && n_images == 1) {
        // single frame (the reference-shaped call): lowest latency - upload on the compute stream itself, no cross-stream hops.
        // The buffer may still be read by an earlier batch on other lanes / by a stereo match on the other handle's stream.
        if ((rc = wait_buffer_consumed(e, 0, e->stream))) return rc;
        if ((rc = join_previous_on_main(e))) return rc;
        const double t0 = e->trace_host ? now_us() : 0.0;
        if (e->kernel_upload) {
            if (!e->h_upload) {
                HIPCHK(e, hipHostMalloc(&e->h_upload, img_bytes));
                HIPCHK(e, hipEventCreateWithFlags(&e->ev_upload_read, hipEventDisableTiming));
            }
            // the previous frame's upload kernel must have read the pinned buffer before it is rewritten: its own event (asynchronous
            // callers that have not waited for that frame yet wait here; a batch enqueued in between does not change what has to be waited for)
            if (e->upload_inflight && (rc = wait_event(e, e->ev_upload_read, e->spin_wait != 0))) return rc;
            e->upload_inflight = false;
            memcpy(e->h_upload, host_images, img_bytes);
            e->upload_pending = true;
        } else {
            HIPCHK(e, hipMemcpyAsync(e->stage[0], host_images, img_bytes, hipMemcpyHostToDevice, e->stream));
        }
        const double t1 = e->trace_host ? now_us() : 0.0;
        e->src.l0 = e->stage[0]; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
        if ((rc = run_pipeline(e, n_images))) return rc;
        if (e->trace_host) { e->th_h2d += t1 - t0; e->th_enq += now_us() - t1; e->th_n++; }
        e->stage_cur = 1;       // a following batch call starts on the other buffer
        *mark = 0;
        return JSORB_OK;
    }
    if (e->stage[0] && step == l0.W && image_stride == img_bytes) {
        // dense batch: pinned hipMemcpyAsync on the device's upload stream into a landing buffer, then level 0 is read in place from
        // there.  The buffer being refilled was last read two batches ago (its extract kernels and, if any, the stereo match), so the
        // upload of batch k+1 runs under the kernels of batch k.  With more than one lane (JSORB_HOST_LANES) the upload is cut at the
        // lane boundaries: lane j starts as soon as ITS images have landed and its part of the buffer is refilled as soon as lane j of
        // the batch that used it has finished.
        // One lane: the regime is PCIe-bound (a pair is 722 kB; 57 GB/s = 79 k pairs/s against 85 k for the kernels on one lane), so the
        // kernels do not need the overlap of several lanes, and one upload per handle and batch runs at the full rate of the link where
        // lane-sized chunks reach 49-51 GB/s with 18-24 us between them (measured at 64 / 128 / 256 pairs per batch on 16 hardware
        // queues: 1 lane 60.6 / 70.2 / 73.1 k, 2 lanes 55.5 / 62.4 / 69.9 k, 4 lanes 48 / 58 k pairs/s).  JSORB_HOST_LANES raises the cap.
        const int k = e->stage_cur;
        int first[JSORB_MAX_LANES + 1];
        e->lane_cap = e->host_lanes;
        const int K = plan_lanes(e, n_images, first);
        hipStream_t cs = nullptr;
        if ((rc = pool_copy_stream(e, &cs))) { e->lane_cap = JSORB_MAX_LANES; return rc; }
        const bool same_split = e->consumed_K[k] == K && e->consumed_n[k] == n_images;
        if (!same_split && (rc = wait_buffer_consumed(e, k, cs))) { e->lane_cap = JSORB_MAX_LANES; return rc; }
        for (int j = 0; j < K; j++) {
            if (same_split) HIPCHK(e, hipStreamWaitEvent(cs, e->ev_consumed[k][j], 0));
            HIPCHK(e, hipMemcpyAsync(e->stage[k] + (size_t)first[j] * img_bytes, host_images + (size_t)first[j] * img_bytes,
                                     img_bytes * (size_t)(first[j + 1] - first[j]), hipMemcpyHostToDevice, cs));
            HIPCHK(e, hipEventRecord(e->ev_copied[k][j], cs));
        }
        e->src.l0 = e->stage[k]; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
        rc = run_pipeline(e, n_images, e->ev_copied[k]);
        e->lane_cap = JSORB_MAX_LANES;
        if (rc) return rc;
        e->stage_cur = k ^ 1;
        *mark = k;
        return JSORB_OK;
    }
    // strided input: one 2-D copy per image into the pitched slab, enqueued by run_pipeline on the stream of the lane that owns the image
    // (with maps: into the dense raw buffer that k_rectify reads)
    e->copy_src = host_images; e->copy_stride = image_stride; e->copy_step = step; e->copy_kind = 1;
    e->src.l0 = e->slab; e->src.l0_stride = e->g.slab_bytes; e->src.l0_pitch = l0.pitch;
    if (e->rect_on) {
        if (!e->rect_raw) HIPCHK(e, hipMalloc(&e->rect_raw, (size_t)e->B * img_bytes + 256));
        e->src.l0 = e->rect_raw; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
    }
    e->last_stage = -1;
    return run_pipeline(e, n_images);
}

int jsorb_extract_batch_host_async(jsorb_extractor *e, const uint8_t *host_images, size_t image_stride, int step, int n_images)
{
    if (!e || !host_images || n_images < 1 || n_images > e->B || step < e->g.lv[0].W) return JSORB_ERR_INVALID;
    e->mirror_valid = e->st_mirror_valid = false;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = spec_guard(e, n_images);
    if (rc) return rc;
    e->lane_cap = JSORB_MAX_LANES;
    int mark;
    if ((rc = extract_batch_host_enqueue(e, host_images, image_stride, step, n_images, &mark))) return rc;
    // the speculative match goes out first: every packet between the extract kernels and k_stereo (an event record is a barrier
    // packet, ~5 us on the GPU's command processor) delays the match
    spec_after_extract(e, n_images);
    return mark >= 0 ? mark_buffer_consumed(e, mark) : JSORB_OK;
}

static int extract_batch_device_enqueue(jsorb_extractor *e, const uint8_t *dev_images, size_t image_stride, int step, int n_images)
{
    const LevelDesc &l0 = e->g.lv[0];
    // Level 0 is read where it lies, whatever its alignment (round 3): the kernels' 16-byte staging loads of a plane whose rows are not
    // 16-byte aligned (a dense 1241-pixel-wide KITTI plane) are unaligned vector-memory accesses - about twice the cost per cache line
    // for those loads, in kernels that are instruction-issue bound - instead of a copy kernel over the whole plane first (7 % of the
    // KITTI-shaped configuration's kernel time).  Every 16-byte chunk a kernel samples lies inside its row; chunks that cross the end of a
    // row are zero-filled (k_detect, k_blur: never sampled), bounds-checked (k_pyramid) or continue into the next row of the same image
    // (k_describe, k_stereo: rows at least 5 above the last).  JSORB_COPY_UNALIGNED=1 restores the copy.
    static const bool copy_unaligned = experiment_env("JSORB_COPY_UNALIGNED") && atoi(experiment_env("JSORB_COPY_UNALIGNED")) != 0;
    const bool aligned16 = (step % 16 == 0) && (((uintptr_t)dev_images) % 16 == 0) && (image_stride % 16 == 0);
    const bool in_place = aligned16 || !copy_unaligned || e->rect_on;      // (k_rectify reads any alignment)
    if (in_place) {   // no copy of the grayscale plane
        e->src.l0 = dev_images; e->src.l0_stride = image_stride; e->src.l0_pitch = step;
    } else {
        // rows that are not 16-byte aligned: one copy kernel per lane brings level 0 into the pitched slab (run_pipeline, lane stream)
        e->copy_src = dev_images; e->copy_stride = image_stride; e->copy_step = step; e->copy_kind = 2;
        e->src.l0 = e->slab; e->src.l0_stride = e->g.slab_bytes; e->src.l0_pitch = l0.pitch;
    }
    e->last_stage = -1;
    return run_pipeline(e, n_images);
}

int jsorb_extract_batch_device_async(jsorb_extractor *e, const uint8_t *dev_images, size_t image_stride, int step, int n_images)
{
    if (!e || !dev_images || n_images < 1 || n_images > e->B || step < e->g.lv[0].W) return JSORB_ERR_INVALID;
    e->mirror_valid = e->st_mirror_valid = false;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = spec_guard(e, n_images);
    if (rc) return rc;
    e->lane_cap = JSORB_MAX_LANES;
    if ((rc = extract_batch_device_enqueue(e, dev_images, image_stride, step, n_images))) return rc;
    spec_after_extract(e, n_images);
    return JSORB_OK;
}

// Waits for an event by polling first (a frame is ~100 us of GPU time; a blocking wait adds tens of microseconds of wake-up latency)
static int wait_event(jsorb_extractor *e, hipEvent_t ev, bool spin)
{
    if (spin)
        for (int it = 0; it < 400000; it++) {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) return JSORB_OK;
            if (q != hipErrorNotReady) { e->err = std::string("hipEventQuery: ") + hipGetErrorString(q); return JSORB_ERR_HIP; }
            __builtin_ia32_pause();
        }
    HIPCHK(e, hipEventSynchronize(ev));
    return JSORB_OK;
}

// Tail of the synchronous single-frame calls: ONE wait - counts, keypoints and descriptors were written into the pinned mirrors (and
// the caller's device buffers) by the kernels themselves.  The wait is for the event behind the extract kernels, not for the stream:
// the other extractor's thread may already have put this frame's speculative stereo match on it (struct jsorb_spec_state).
static int finish_single_frame(jsorb_extractor *e, int *n_keypoints)
{
    const double t0 = e->trace_host ? now_us() : 0.0;
    int rc;
    if (e->timing || e->K != 1) rc = jsorb_sync(e);
    else if (!(rc = wait_event(e, e->lane_done[0], e->spin_wait != 0))) {
        e->counts_synced = true;
        if (e->mirror_pending) { e->mirror_valid = true; e->mirror_pending = false; }
    }
    if (e->trace_host) e->th_wait += now_us() - t0;
    if (rc) return rc;
    if (n_keypoints) *n_keypoints = e->h_counts[JSORB_MAX_LEVELS];
    return JSORB_OK;
}

// The synchronous single-image calls wait for the frame themselves, so nobody needs ev_upload_read (one barrier packet less in front of the
// match) - `sync_single` tells run_pipeline so.  The flag is reset on every way out (scope guard), and a call that fails AFTER the frame was
// enqueued (mark_buffer_consumed / finish_single_frame) waits for the stream before it returns: the next call memcpys into the pinned upload
// buffer without an event to wait for, and k_upload_level0 of the failed frame may still be reading it (round-4 review).
static int extract_single_sync(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints)
{
    struct Reset { jsorb_extractor *e; ~Reset() { e->sync_single = false; } } reset{e};
    e->sync_single = true;
    int rc = jsorb_extract_batch_host_async(e, host_image, 0, step, 1);
    if (!rc) rc = finish_single_frame(e, n_keypoints);
    if (rc && e->stream) (void)hipStreamSynchronize(e->stream);
    return rc;
}

int jsorb_extract(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints)
{
    if (!e) return JSORB_ERR_INVALID;
    return extract_single_sync(e, host_image, step, n_keypoints);
}

int jsorb_extract_into(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints, int32_t *dev_keypoints_dst, uint8_t *dev_descriptors_dst)
{
    if (!e) return JSORB_ERR_INVALID;
    e->deliver_kp_dev = dev_keypoints_dst;
    e->deliver_desc_dev = dev_descriptors_dst;
    const int rc = extract_single_sync(e, host_image, step, n_keypoints);
    e->deliver_kp_dev = nullptr;
    e->deliver_desc_dev = nullptr;
    return rc;
}

int jsorb_extract_device(jsorb_extractor *e, const uint8_t *dev_image, int step, int *n_keypoints)
{
    int rc = jsorb_extract_batch_device_async(e, dev_image, 0, step, 1);
    if (rc) return rc;
    return finish_single_frame(e, n_keypoints);
}

// ---- rectification maps (Examples/Stereo/stereo_euroc.cpp:106-107, 145-146) ----
int jsorb_rectify_convert_maps(const float *mapx, const float *mapy, int n, int16_t *xy, uint16_t *a)
{
    if (!mapx || !mapy || !xy || !a || n < 0) return JSORB_ERR_INVALID;
    rectify_convert_maps(mapx, mapy, (size_t)n, xy, a);
    return JSORB_OK;
}

// The map's entries at pitch round_up(W, 4) (one 16-byte + one 8-byte load per lane of k_rectify), entries beyond W point outside the source, then
// the per-tile source boxes.  The handle's work in flight is waited for first: its k_rectify launches read the buffer that is overwritten.
static int rectify_upload(jsorb_extractor *e, const int16_t *xy, const uint16_t *a, int xy_step, int a_step)
{
    const int W = e->g.lv[0].W, H = e->g.lv[0].H, MP = round_up(W, 4);
    const int ntx = (W + RECT_TW - 1) / RECT_TW, nty = (H + RECT_TH - 1) / RECT_TH;
    std::vector<int16_t> hxy((size_t)2 * MP * H, (int16_t)-32768);
    std::vector<uint16_t> ha((size_t)MP * H, 0);
    for (int y = 0; y < H; y++) {
        memcpy(&hxy[(size_t)2 * MP * y], xy + (size_t)2 * xy_step * y, (size_t)4 * W);
        for (int x = 0; x < W; x++) ha[(size_t)MP * y + x] = a[(size_t)a_step * y + x] & 1023;
    }
    std::vector<int32_t> tiles((size_t)4 * ntx * nty);
    rectify_tile_table(hxy.data(), ha.data(), W, H, MP, ntx, nty, tiles.data());
    const size_t xy_bytes = (size_t)4 * MP * H, a_bytes = ((size_t)2 * MP * H + 255) & ~(size_t)255, t_bytes = tiles.size() * 4;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = jsorb_sync(e);
    if (rc) return rc;
    if (!e->rect_buf) HIPCHK(e, hipMalloc(&e->rect_buf, xy_bytes + a_bytes + t_bytes));
    uint8_t *base = static_cast<uint8_t *>(e->rect_buf);
    HIPCHK(e, hipMemcpy(base, hxy.data(), xy_bytes, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(base + xy_bytes, ha.data(), (size_t)2 * MP * H, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(base + xy_bytes + a_bytes, tiles.data(), t_bytes, hipMemcpyHostToDevice));
    e->rmap = RectMap{reinterpret_cast<const int *>(base), reinterpret_cast<const uint16_t *>(base + xy_bytes), reinterpret_cast<const int4 *>(base + xy_bytes + a_bytes),
                      MP, ntx, nty};
    e->rect_on = true;
    frame_graph_drop(e);        // the single-frame graph starts with k_rectify now: captured again on the next frame
    return JSORB_OK;
}

int jsorb_set_rectify_maps_fixed(jsorb_extractor *e, const int16_t *xy, const uint16_t *a, int width, int height, int xy_step, int a_step)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!xy || !a || width != e->g.lv[0].W || height != e->g.lv[0].H || xy_step < width || a_step < width) {
        e->err = "rectification maps must have the handle's image size (and steps >= width)";
        return JSORB_ERR_INVALID;
    }
    return rectify_upload(e, xy, a, xy_step, a_step);
}

int jsorb_set_rectify_maps(jsorb_extractor *e, const float *mapx, const float *mapy, int width, int height, int map_step_floats)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!mapx || !mapy || width != e->g.lv[0].W || height != e->g.lv[0].H || map_step_floats < width) {
        e->err = "rectification maps must have the handle's image size (and a step >= width)";
        return JSORB_ERR_INVALID;
    }
    std::vector<int16_t> xy((size_t)2 * width * height);
    std::vector<uint16_t> a((size_t)width * height);
    for (int y = 0; y < height; y++)
        rectify_convert_maps(mapx + (size_t)map_step_floats * y, mapy + (size_t)map_step_floats * y, (size_t)width, &xy[(size_t)2 * width * y], &a[(size_t)width * y]);
    return rectify_upload(e, xy.data(), a.data(), width, width);
}

int jsorb_clear_rectify_maps(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!e->rect_on) return JSORB_OK;
    HIPCHK(e, hipSetDevice(e->device));
    int rc = jsorb_sync(e);
    if (rc) return rc;
    e->rect_on = false;
    frame_graph_drop(e);
    return JSORB_OK;
}

int jsorb_rectify_enabled(const jsorb_extractor *e) { return e ? (e->rect_on ? 1 : 0) : JSORB_ERR_INVALID; }

// ---- camera: Frame::UndistortKeyPoints / ComputeImageBounds (Frame.cpp:718-778) ----
static UndistortCam to_cam(const jsorb_camera &c) { return UndistortCam{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3}; }

int jsorb_image_bounds(const jsorb_camera *camera, int width, int height, float out[4])
{
    if (!camera || !out || width < 1 || height < 1) return JSORB_ERR_INVALID;
    const UndistortCam c = to_cam(*camera);
    if (!camera_active(c)) {
        out[0] = 0.0f; out[1] = (float)width; out[2] = 0.0f; out[3] = (float)height;
        return JSORB_OK;
    }
    const float W = (float)width, H = (float)height;
    const float cx[4] = {0.0f, W, 0.0f, W}, cy[4] = {0.0f, 0.0f, H, H};
    float ux[4], uy[4];
    for (int i = 0; i < 4; i++) undistort_point(c, cx[i], cy[i], &ux[i], &uy[i]);
    out[0] = std::min(ux[0], ux[2]);
    out[1] = std::max(ux[1], ux[3]);
    out[2] = std::min(uy[0], uy[1]);
    out[3] = std::max(uy[2], uy[3]);
    return JSORB_OK;
}

int jsorb_set_camera(jsorb_extractor *e, const jsorb_camera *camera)
{
    if (!e) return JSORB_ERR_INVALID;
    const bool on = camera && camera->k1 != 0.0f;
    if (!on && !e->cam_on) return JSORB_OK;          // nothing to undo, nothing to allocate
    HIPCHK(e, hipSetDevice(e->device));
    int rc = jsorb_sync(e);
    if (rc) return rc;
    frame_graph_drop(e);          // the single-frame graph carries the camera as a kernel argument (or lacks k_undistort): captured again
    e->un_valid = false;
    e->un_mirror = false;
    e->rgbd_images = 0;           // its uRight used the old mvKeysUn
    e->rgbd_mirror = false;
    e->cam_on = on;
    if (!on) return JSORB_OK;
    e->cam = to_cam(*camera);
    const size_t T = (size_t)e->g.T;
    if (!e->un) HIPCHK(e, hipMalloc(&e->un, (size_t)e->B * 2 * T * sizeof(float)));
    if (!e->h_un) HIPCHK(e, hipHostMalloc(&e->h_un, 2 * T * sizeof(float)));
    if (e->extracted && e->n_images > 0) {      // the results already there are undistorted with the new camera (device copy only)
        launch_undistort(e->cam, e->out_kp, e->counts, (int)T, e->un, nullptr, e->n_images, e->stream);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->stream));
        e->un_valid = true;
    }
    return JSORB_OK;
}

int jsorb_camera_enabled(const jsorb_extractor *e) { return e ? (e->cam_on ? 1 : 0) : JSORB_ERR_INVALID; }

const float *jsorb_keypoints_un_device(const jsorb_extractor *e, int image)
{
    return (check_image(e, image) && e->un_valid) ? e->un + (size_t)image * 2 * e->g.T : nullptr;
}

int jsorb_copy_keypoints_un(const jsorb_extractor *e, int image, float *xy)
{
    if (!check_image(e, image) || !xy) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (!e->un_valid) {           // mvKeysUn = mvKeys: the keypoint coordinates as floats
        std::vector<int32_t> kp((size_t)6 * n);
        int rc = jsorb_copy_keypoints(e, image, kp.data());
        if (rc) return rc;
        for (size_t i = 0; i < (size_t)2 * n; i++) xy[i] = (float)kp[i];
        return JSORB_OK;
    }
    if (e->mirror_valid && e->un_mirror && image == 0) { memcpy(xy, e->h_un, (size_t)n * 2 * sizeof(float)); return JSORB_OK; }
    return hipMemcpy(xy, jsorb_keypoints_un_device(e, image), (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

int jsorb_unpack_frame_un(jsorb_extractor *e, int image, jsorb_keypoint *keys, jsorb_keypoint *keys_un, uint8_t *descriptors)
{
    if (!check_image(e, image)) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (!keys_un) return jsorb_unpack_frame(e, image, keys, descriptors);
    if (e->mirror_valid && image == 0 && (!e->un_valid || e->un_mirror)) {
        // synchronous single frame: keypoints, descriptors and x_un / y_un are in pinned host memory already - interleave here (Frame.cpp:139-147, 741-747)
        int rc = jsorb_unpack_frame(e, 0, keys_un, descriptors);
        if (rc) return rc;
        if (keys) memcpy(keys, keys_un, (size_t)n * sizeof(jsorb_keypoint));
        if (e->un_valid)
            for (int i = 0; i < n; i++) { keys_un[i].x = e->h_un[i]; keys_un[i].y = e->h_un[n + i]; }
        return JSORB_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->frame_aos) HIPCHK(e, hipMalloc(&e->frame_aos, (size_t)e->g.T * sizeof(jsorb_keypoint)));
    std::vector<float> xy(e->un_valid ? (size_t)2 * n : 0);
    launch_unpack_keypoints(jsorb_keypoints_device(e, image), n, e->frame_aos, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(keys_un, e->frame_aos, (size_t)n * sizeof(jsorb_keypoint), hipMemcpyDeviceToHost, e->stream));
    if (keys) HIPCHK(e, hipMemcpyAsync(keys, e->frame_aos, (size_t)n * sizeof(jsorb_keypoint), hipMemcpyDeviceToHost, e->stream));
    if (e->un_valid) HIPCHK(e, hipMemcpyAsync(xy.data(), jsorb_keypoints_un_device(e, image), (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (descriptors) HIPCHK(e, hipMemcpyAsync(descriptors, jsorb_descriptors_device(e, image), (size_t)n * 32, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->un_valid)
        for (int i = 0; i < n; i++) { keys_un[i].x = xy[i]; keys_un[i].y = xy[n + i]; }
    return JSORB_OK;
}

// ---- RGB-D: Frame::ComputeStereoFromRGBD (Frame.cpp:996-1017) + Tracking.cpp:333-334 ----
static int rgbd_check(jsorb_extractor *e, const void *depth, int format, size_t step_bytes, size_t image_stride, int n_images)
{
    if (!e->extracted) { e->err = "RGB-D depth before extract"; return JSORB_ERR_STATE; }
    const size_t bpp = format == JSORB_DEPTH_U16 ? 2 : format == JSORB_DEPTH_F32 ? 4 : 0;
    if (!depth || !bpp || step_bytes < (size_t)e->g.lv[0].W * bpp || step_bytes % bpp || image_stride % bpp || (uintptr_t)depth % bpp) {
        e->err = "RGB-D depth: bad format, step or alignment (rows of W elements, element-aligned)";
        return JSORB_ERR_INVALID;
    }
    if (n_images > 1 && image_stride < (size_t)e->g.lv[0].H * step_bytes) {      // depth images must not overlap
        e->err = "RGB-D depth batch: image_stride must be at least height * step_bytes";
        return JSORB_ERR_INVALID;
    }
    const size_t T = (size_t)e->g.T;
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->rg) HIPCHK(e, hipMalloc(&e->rg, (size_t)e->B * 2 * T * sizeof(float)));
    if (!e->h_rg) HIPCHK(e, hipHostMalloc(&e->h_rg, 2 * T * sizeof(float)));
    return JSORB_OK;
}

static RgbdArgs rgbd_args(int format, float factor, float mbf)
{
    // Tracking.cpp:333: if ((fabs(mDepthMapFactor - 1.0f) > 1e-5) || imDepth.type() != CV_32F) imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)
    const bool scale = format == JSORB_DEPTH_U16 || std::fabs(factor - 1.0f) > 1e-5;
    return RgbdArgs{format, scale ? 1 : 0, factor, mbf};
}

int jsorb_rgbd_depth_batch_device_async(jsorb_extractor *e, const void *dev_depths, size_t image_stride, size_t step_bytes, int format, float factor,
                                        float mbf, int n_images)
{
    if (!e) return JSORB_ERR_INVALID;
    if (n_images != e->n_images) { e->err = "RGB-D batch: n_images must be the last batch's"; return JSORB_ERR_INVALID; }
    int rc = rgbd_check(e, dev_depths, format, step_bytes, image_stride, n_images);
    if (rc) return rc;
    const size_t T = (size_t)e->g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    const RgbdArgs a = rgbd_args(format, factor, mbf);
    // the depth images may come from work the caller enqueued on the main stream after the extract call (e.g. torch's current stream through
    // jsorb_set_stream): every lane that is not the main stream starts after a fork event recorded there
    bool forked = false;
    for (int j = 0; j < e->K; j++)
        if (lane_stream(e, j) != e->stream) {
            if (!forked) { HIPCHK(e, hipEventRecord(e->ev_fork, e->stream)); forked = true; }
            HIPCHK(e, hipStreamWaitEvent(lane_stream(e, j), e->ev_fork, 0));
        }
    for (int j = 0; j < e->K; j++) {        // lane j samples its own images, behind its extraction (and k_undistort) on its stream
        hipStream_t st = lane_stream(e, j);
        const int f = e->lane_first[j], m = e->lane_first[j + 1] - f;
        TIMED(e, JSORB_K_RGBD, launch_rgbd(e->out_kp + f * T * 6, e->counts + f * CW, (int)T, e->un_valid ? e->un + f * T * 2 : nullptr,
                                           static_cast<const uint8_t *>(dev_depths) + (size_t)f * image_stride, image_stride, step_bytes, e->g.lv[0].W,
                                           e->g.lv[0].H, a, e->rg + f * T, e->rg + (size_t)e->B * T + f * T, nullptr, nullptr, m, st));
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->lane_done[j], st));
    }
    // ... and whatever the caller enqueues on its main stream next (reading jsorb_rgbd_uright_device, say) runs after every lane, as behind an extract
    if (e->stream != e->own_stream)
        for (int j = 0; j < e->K; j++)
            if (lane_stream(e, j) != e->stream) HIPCHK(e, hipStreamWaitEvent(e->stream, e->lane_done[j], 0));
    e->rgbd_images = n_images;
    e->rgbd_mirror = false;
    e->counts_synced = false;
    return JSORB_OK;
}

int jsorb_rgbd_depth(jsorb_extractor *e, const void *host_depth, int format, size_t step_bytes, float factor, float mbf, float *u_right, float *depth)
{
    if (!e) return JSORB_ERR_INVALID;
    int rc = rgbd_check(e, host_depth, format, step_bytes, 0, 1);
    if (rc) return rc;
    if (e->n_images < 1) return JSORB_ERR_STATE;
    const int W = e->g.lv[0].W, H = e->g.lv[0].H;
    const size_t bpp = format == JSORB_DEPTH_U16 ? 2 : 4, row = (size_t)W * bpp, T = (size_t)e->g.T;
    if (!e->h_depth) HIPCHK(e, hipHostMalloc(&e->h_depth, (size_t)H * W * 4));
    // the host image reaches the device the way a single host image does: copied into a pinned buffer of the handle by the calling thread,
    // then read in place over PCIe by the kernel - which reads only the N sampled pixels
    const uint8_t *src = static_cast<const uint8_t *>(host_depth);
    if (step_bytes == row) memcpy(e->h_depth, src, row * H);
    else
        for (int y = 0; y < H; y++) memcpy(e->h_depth + row * y, src + step_bytes * y, row);
    hipStream_t st = lane_stream(e, 0);
    if (e->K != 1 || !st) st = e->stream;
    for (int j = 0; j < e->K; j++)
        if (lane_stream(e, j) != st) HIPCHK(e, hipStreamWaitEvent(st, e->lane_done[j], 0));
    TIMED(e, JSORB_K_RGBD, launch_rgbd(e->out_kp, e->counts, (int)T, e->un_valid ? e->un : nullptr, e->h_depth, 0, row, W, H, rgbd_args(format, factor, mbf),
                                       e->rg, e->rg + (size_t)e->B * T, e->h_rg, e->h_rg + T, 1, st));
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->lane_done[0], st));
    if (st != lane_stream(e, 0)) for (int j = 1; j < e->K; j++) HIPCHK(e, hipEventRecord(e->lane_done[j], st));
    if (e->timing || e->K != 1) rc = jsorb_sync(e);
    else rc = wait_event(e, e->lane_done[0], e->spin_wait != 0);
    if (rc) return rc;
    e->rgbd_images = 1;           // image 0 only
    e->rgbd_mirror = true;
    const int n = e->h_counts[JSORB_MAX_LEVELS];
    if (u_right && n > 0) memcpy(u_right, e->h_rg, (size_t)n * sizeof(float));
    if (depth && n > 0) memcpy(depth, e->h_rg + T, (size_t)n * sizeof(float));
    return JSORB_OK;
}

const float *jsorb_rgbd_uright_device(const jsorb_extractor *e, int image)
{
    return (check_image(e, image) && image < e->rgbd_images) ? e->rg + (size_t)image * e->g.T : nullptr;
}
const float *jsorb_rgbd_depth_device(const jsorb_extractor *e, int image)
{
    return (check_image(e, image) && image < e->rgbd_images) ? e->rg + (size_t)e->B * e->g.T + (size_t)image * e->g.T : nullptr;
}
int jsorb_copy_rgbd(const jsorb_extractor *e, int image, float *u_right, float *depth)
{
    if (!check_image(e, image) || image >= e->rgbd_images) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (e->rgbd_mirror && image == 0) {
        if (u_right) memcpy(u_right, e->h_rg, (size_t)n * sizeof(float));
        if (depth) memcpy(depth, e->h_rg + e->g.T, (size_t)n * sizeof(float));
        return JSORB_OK;
    }
    if (u_right && hipMemcpy(u_right, jsorb_rgbd_uright_device(e, image), (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
    if (depth && hipMemcpy(depth, jsorb_rgbd_depth_device(e, image), (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
    return JSORB_OK;
}

int jsorb_n_images(const jsorb_extractor *e) { return e ? e->n_images : 0; }
int jsorb_n_keypoints(const jsorb_extractor *e, int image)
{
    return check_image(e, image) ? e->h_counts[image * (JSORB_MAX_LEVELS + 1) + JSORB_MAX_LEVELS] : JSORB_ERR_STATE;
}
int jsorb_level_n_keypoints(const jsorb_extractor *e, int image, int level)
{
    if (!check_image(e, image) || level < 0 || level >= e->g.L) return JSORB_ERR_STATE;
    return e->h_counts[image * (JSORB_MAX_LEVELS + 1) + level];
}
const int32_t *jsorb_keypoints_device(const jsorb_extractor *e, int image)
{
    return check_image(e, image) ? e->out_kp + (size_t)image * 6 * e->g.T : nullptr;
}
const uint8_t *jsorb_descriptors_device(const jsorb_extractor *e, int image)
{
    return check_image(e, image) ? e->desc + (size_t)image * 32 * e->g.T : nullptr;
}
int jsorb_copy_keypoints(const jsorb_extractor *e, int image, int32_t *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (e->mirror_valid && image == 0) { memcpy(dst, e->h_kp, (size_t)n * 6 * 4); return JSORB_OK; }
    return hipMemcpy(dst, jsorb_keypoints_device(e, image), (size_t)n * 6 * 4, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}
int jsorb_copy_descriptors(const jsorb_extractor *e, int image, uint8_t *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (e->mirror_valid && image == 0) { memcpy(dst, e->h_desc, (size_t)n * 32); return JSORB_OK; }
    return hipMemcpy(dst, jsorb_descriptors_device(e, image), (size_t)n * 32, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

// ---- Frame-side unpacking ----
int jsorb_unpack_frame(jsorb_extractor *e, int image, jsorb_keypoint *keypoints, uint8_t *descriptors)
{
    if (!check_image(e, image)) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (e->mirror_valid && image == 0) {
        // after a synchronous single-frame extract the SoA already sits in pinned host memory: interleave it here (the
        // reference's own host loop, Frame.cpp:139-147) instead of a kernel + two copies + a synchronisation
        if (keypoints) {
            const int32_t *s = e->h_kp;
            for (int i = 0; i < n; i++) {
                jsorb_keypoint &k = keypoints[i];
                k.x = (float)s[i]; k.y = (float)s[n + i]; k.response = (float)s[2 * (size_t)n + i];
                memcpy(&k.angle, &s[3 * (size_t)n + i], 4);
                k.octave = s[4 * (size_t)n + i]; k.size = (float)s[5 * (size_t)n + i]; k.class_id = -1;
            }
        }
        if (descriptors) memcpy(descriptors, e->h_desc, (size_t)n * 32);
        return JSORB_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (keypoints) {
        if (!e->frame_aos) HIPCHK(e, hipMalloc(&e->frame_aos, (size_t)e->g.T * sizeof(jsorb_keypoint)));
        launch_unpack_keypoints(jsorb_keypoints_device(e, image), n, e->frame_aos, e->stream);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemcpyAsync(keypoints, e->frame_aos, (size_t)n * sizeof(jsorb_keypoint), hipMemcpyDeviceToHost, e->stream));
    }
    if (descriptors) HIPCHK(e, hipMemcpyAsync(descriptors, jsorb_descriptors_device(e, image), (size_t)n * 32, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return JSORB_OK;
}

int jsorb_assign_features_to_grid(jsorb_extractor *e, int image, float min_x, float min_y, float grid_element_width_inv,
                                  float grid_element_height_inv, int cols, int rows, int32_t *cell_start, int32_t *cell_items)
{
    if (!check_image(e, image) || !cell_start || !cell_items) return JSORB_ERR_STATE;
    if (cols < 1 || rows < 1 || (long long)cols * rows > 16384) { e->err = "grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image), n_cells = cols * rows;
    HIPCHK(e, hipSetDevice(e->device));
    if (e->grid_cells < n_cells) {
        if (e->grid_start) (void)hipFree(e->grid_start);
        e->grid_start = nullptr;
        HIPCHK(e, hipMalloc(&e->grid_start, (size_t)(n_cells + 1) * sizeof(int32_t)));
        e->grid_cells = n_cells;
    }
    if (!e->grid_items) HIPCHK(e, hipMalloc(&e->grid_items, (size_t)e->g.T * sizeof(int32_t)));
    launch_assign_grid(jsorb_keypoints_device(e, image), jsorb_keypoints_un_device(e, image), n, min_x, min_y, grid_element_width_inv, grid_element_height_inv, cols, rows,
                       e->grid_start, e->grid_items, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(cell_start, e->grid_start, (size_t)(n_cells + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const int in_grid = cell_start[n_cells];
    if (in_grid > 0) HIPCHK(e, hipMemcpy(cell_items, e->grid_items, (size_t)in_grid * sizeof(int32_t), hipMemcpyDeviceToHost));
    return JSORB_OK;
}

// ---- local map matching: ORBmatcher::SearchByProjection(Frame&, map points, th) (ORBmatcher.cpp:32-116), k_search_local.hip ----
int jsorb_search_local_points_async(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                                    const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                                    const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp,
                                    int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) { e->err = "search_local_points: no extract result for this image"; return JSORB_ERR_STATE; }
    if (!params || !n_matches_dev) { e->err = "search_local_points: NULL params or n_matches"; return JSORB_ERR_INVALID; }
    const jsorb_search_params &p = *params;
    if (p.cols < 1 || p.rows < 1 || (long long)p.cols * p.rows > 16384) { e->err = "search_local_points: grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_local_points: n_points < 0"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image);
    if (n >= (1 << 18)) { e->err = "search_local_points: more than 262143 keypoints"; return JSORB_ERR_UNSUPPORTED; }
    if (n_points > 0 && (!u || !v || !invz || !predicted_level || !view_cos || !in_frustum || !mp_descriptors || !match_kp || !match_dist)) {
        e->err = "search_local_points: NULL point array or output";
        return JSORB_ERR_INVALID;
    }
    if (n > 0 && !kp_match) { e->err = "search_local_points: NULL kp_match"; return JSORB_ERR_INVALID; }
    if ((uintptr_t)mp_descriptors % 16) { e->err = "search_local_points: mp_descriptors must be 16-byte aligned"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int n_cells = p.cols * p.rows, cap = search_local_cap();
    if (e->grid_cells < n_cells) {
        if (e->grid_start) (void)hipFree(e->grid_start);
        e->grid_start = nullptr;
        HIPCHK(e, hipMalloc(&e->grid_start, (size_t)(n_cells + 1) * sizeof(int32_t)));
        e->grid_cells = n_cells;
    }
    if (!e->grid_items) HIPCHK(e, hipMalloc(&e->grid_items, (size_t)e->g.T * sizeof(int32_t)));
    if (e->sl_points < n_points) {
        if (e->sl_cand) (void)hipFree(e->sl_cand);        // (waits for the device: the last call may still read it)
        e->sl_cand = nullptr;
        HIPCHK(e, hipMalloc(&e->sl_cand, (size_t)n_points * (cap + 1) * sizeof(int)));
        e->sl_points = n_points;
    }
    if (!e->sl_stats) HIPCHK(e, hipMalloc(&e->sl_stats, 4 * sizeof(int)));
    hipStream_t st = e->stream;
    for (int j = 0; j < e->K; j++)       // the frame (and its uRight) may come from the lanes of a batch
        if (lane_stream(e, j) && lane_stream(e, j) != st) HIPCHK(e, hipStreamWaitEvent(st, e->lane_done[j], 0));
    const float *xy_un = jsorb_keypoints_un_device(e, image);
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(jsorb_keypoints_device(e, image), xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows,
                                                     e->grid_start, e->grid_items, st));
    HIPCHK(e, hipGetLastError());
    SearchLocalArgs a{};
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = xy_un;
    a.desc = jsorb_descriptors_device(e, image);
    a.u_right = u_right;
    a.blocked = blocked_in;
    a.n_kp = n;
    a.cell_start = e->grid_start;
    a.cell_items = e->grid_items;
    a.min_x = p.min_x; a.min_y = p.min_y; a.inv_w = p.inv_w; a.inv_h = p.inv_h;
    a.cols = p.cols; a.rows = p.rows;
    a.n_points = n_points;
    a.u = u; a.v = v; a.invz = invz; a.view_cos = view_cos; a.level = predicted_level; a.in_frustum = in_frustum; a.mp_desc = mp_descriptors;
    a.th = p.th; a.nn_ratio = p.nn_ratio; a.mbf = p.mbf; a.th_high = p.th_high;
    a.n_levels = e->g.L;
    for (int l = 0; l < e->g.L; l++) a.scale[l] = e->g.lv[l].scale;
    a.cand = e->sl_cand;
    a.cand_n = e->sl_cand + (size_t)e->sl_points * cap;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    a.stats = e->sl_stats;
    TIMED(e, JSORB_K_LOCAL_CANDIDATES, launch_local_candidates(a, st));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_LOCAL_RESOLVE, launch_local_resolve(a, st));
    HIPCHK(e, hipGetLastError());
    e->sl_done = true;
    return JSORB_OK;
}

int jsorb_search_local_points(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                              const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                              const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp_host, int *n_matches)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!n_matches || (n_points > 0 && !match_kp_host)) { e->err = "search_local_points: NULL host output"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_local_points: n_points < 0"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    if (e->sl_out_points < n_points || !e->sl_out) {
        if (e->sl_out) (void)hipFree(e->sl_out);
        e->sl_out = nullptr;
        e->sl_out_points = std::max(n_points, 1);
        HIPCHK(e, hipMalloc(&e->sl_out, ((size_t)2 * e->sl_out_points + e->g.T + 1) * sizeof(int32_t)));
    }
    int32_t *mk = e->sl_out, *md = mk + e->sl_out_points, *km = md + e->sl_out_points, *cnt = km + e->g.T;
    int rc = jsorb_search_local_points_async(e, image, params, n_points, u, v, invz, predicted_level, view_cos, in_frustum, mp_descriptors, u_right,
                                             blocked_in, mk, md, km, cnt);
    if (rc) return rc;
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
    if (!e->sl_done) { e->err = "search_local_stats before jsorb_search_local_points"; return JSORB_ERR_STATE; }
    int32_t s[4] = {0, 0, 0, 0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(s, e->sl_stats, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (rounds) *rounds = s[0];
    if (n_candidates) *n_candidates = s[1];
    if (n_overflow) *n_overflow = s[2];
    return JSORB_OK;
}

int jsorb_n_levels(const jsorb_extractor *e) { return e ? e->g.L : 0; }
int jsorb_total_tiles(const jsorb_extractor *e) { return e ? e->g.T : 0; }
int jsorb_level_dims(const jsorb_extractor *e, int level, int *h, int *w, int *pitch)
{
    if (!e || level < 0 || level >= e->g.L) return JSORB_ERR_INVALID;
    if (h) *h = e->g.lv[level].H;
    if (w) *w = e->g.lv[level].W;
    if (pitch) *pitch = (level == 0 && e->extracted) ? e->src.l0_pitch : e->g.lv[level].pitch;
    return JSORB_OK;
}
int jsorb_level_tiles(const jsorb_extractor *e, int level, int *th, int *tw, int *nth, int *ntw, int *off)
{
    if (!e || level < 0 || level >= e->g.L) return JSORB_ERR_INVALID;
    const LevelDesc &lv = e->g.lv[level];
    if (th) *th = lv.th;
    if (tw) *tw = lv.tw;
    if (nth) *nth = lv.nth;
    if (ntw) *ntw = lv.ntw;
    if (off) *off = lv.tile_off;
    return JSORB_OK;
}
float jsorb_scale(const jsorb_extractor *e, int level) { return (e && level >= 0 && level < e->g.L) ? e->g.lv[level].scale : 0.f; }
float jsorb_inv_scale(const jsorb_extractor *e, int level) { return (e && level >= 0 && level < e->g.L) ? e->g.lv[level].inv_scale : 0.f; }

const uint8_t *jsorb_level_image_device(const jsorb_extractor *e, int image, int level, int blurred)
{
    if (!check_image(e, image) || level < 0 || level >= e->g.L) return nullptr;
    if (blurred) return e->blur + (size_t)image * e->g.slab_bytes + e->g.lv[level].img_off;
    if (level == 0) return e->src.l0 + (size_t)image * e->src.l0_stride;
    return e->slab + (size_t)image * e->g.slab_bytes + e->g.lv[level].img_off;
}
int jsorb_copy_level_image(const jsorb_extractor *e, int image, int level, int blurred, uint8_t *dst)
{
    const uint8_t *p = jsorb_level_image_device(e, image, level, blurred);
    if (!p || !dst) return JSORB_ERR_STATE;
    const LevelDesc &lv = e->g.lv[level];
    const int pitch = (!blurred && level == 0) ? e->src.l0_pitch : lv.pitch;
    return hipMemcpy2D(dst, lv.W, p, pitch, lv.W, lv.H, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}
int jsorb_copy_level_mask(const jsorb_extractor *e, int level, uint8_t *dst)
{
    if (!e || !dst || level < 0 || level >= e->g.L) return JSORB_ERR_INVALID;
    const LevelDesc &lv = e->g.lv[level];
    if (!e->mask) { memset(dst, 255, (size_t)lv.H * lv.W); return JSORB_OK; }
    if (hipSetDevice(e->device) != hipSuccess) return JSORB_ERR_HIP;
    return hipMemcpy2D(dst, lv.W, e->mask + lv.img_off, lv.pitch, lv.W, lv.H, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}
int jsorb_copy_tile_candidates(const jsorb_extractor *e, int image, int32_t *x, int32_t *y, int32_t *score)
{
    if (!check_image(e, image)) return JSORB_ERR_STATE;
    std::vector<unsigned long long> t(e->g.T);
    if (hipMemcpy(t.data(), e->tile_out + (size_t)image * e->g.T, (size_t)e->g.T * 8, hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
    for (int i = 0; i < e->g.T; i++) {
        if (x) x[i] = (int32_t)(t[i] & 0xFFFF);
        if (y) y[i] = (int32_t)((t[i] >> 16) & 0xFFFF);
        if (score) score[i] = (int32_t)((t[i] >> 32) & 0xFFF);
    }
    return JSORB_OK;
}
int jsorb_copy_angles(const jsorb_extractor *e, int image, float *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    return hipMemcpy(dst, e->angles + (size_t)image * e->g.T, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

int jsorb_stereo_match_batch_async(jsorb_extractor *l, jsorb_extractor *r, float mb, float mbf, int th_high, int th_low)
{
    if (!l || !r) return JSORB_ERR_INVALID;
    if (!l->extracted || !r->extracted || l->n_images != r->n_images) { l->err = "stereo_match needs one extract on each handle with equal image counts"; return JSORB_ERR_STATE; }
    if (l->g.T != r->g.T || l->g.L != r->g.L || l->g.lv[0].H != r->g.lv[0].H || l->g.lv[0].W != r->g.lv[0].W || l->device != r->device) {
        l->err = "left/right extractors differ in geometry";
        return JSORB_ERR_INVALID;
    }
    HIPCHK(l, hipSetDevice(l->device));
    const int n = l->n_images;
    const StereoArgs sa = make_stereo_args(mb, mbf, th_high, th_low);
    // Lane j of the left handle matches its own pairs as soon as lane j of the right handle has finished them (both handles split
    // the same n into the same lanes); with different partitions every left lane waits for all right lanes.
    const bool aligned = l->K == r->K;
    const bool direct = n == 1;          // one pair: k_median writes uRight, depth and the statistics straight into the pinned host mirrors
    const size_t T = (size_t)l->g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    for (int j = 0; j < l->K; j++) {
        hipStream_t st = lane_stream(l, j);
        if (r != l) {
            if (aligned) { if (lane_stream(r, j) != st) HIPCHK(l, hipStreamWaitEvent(st, r->lane_done[j], 0)); }
            else
                for (int i = 0; i < r->K; i++)
                    if (lane_stream(r, i) != st) HIPCHK(l, hipStreamWaitEvent(st, r->lane_done[i], 0));
        }
        const int f = l->lane_first[j], m = l->lane_first[j + 1] - f;
        ImageSrc srcL = l->src, srcR = r->src;
        srcL.l0 += (size_t)f * srcL.l0_stride;
        srcR.l0 += (size_t)f * srcR.l0_stride;
        const int skip_mask_st = experiment_env("JSORB_SKIP_KERNELS") ? atoi(experiment_env("JSORB_SKIP_KERNELS")) : 0;
        if (!((skip_mask_st >> JSORB_K_STEREO) & 1))
        TIMED(l, JSORB_K_STEREO, launch_stereo(l->g, srcL, l->slab + (size_t)f * l->g.slab_bytes, srcR, r->slab + (size_t)f * r->g.slab_bytes,
                                              l->out_kp + f * T * 6, l->counts + f * CW, l->desc + f * T * 32,
                                              r->out_kp + f * T * 6, r->counts + f * CW, r->desc + f * T * 32, r->row_tab + (size_t)f * r->g.row_tab_stride,
                                              l->st_u + f * T, l->st_d + f * T, l->st_l1 + f * T, l->st_aux + f * T, sa, m, st,
                                              l->st_diag ? l->st_diag + f * T * JSORB_STEREO_DIAG_INTS : nullptr));
        TIMED(l, JSORB_K_MEDIAN, launch_median(l->g, l->counts + f * CW, l->st_u + f * T, l->st_d + f * T, l->st_l1 + f * T, l->st_aux + f * T,
                                              l->st_stats + f * 8, m, st, direct ? DeliverStereo{l->h_u, l->h_d, l->h_stats} : DeliverStereo{nullptr, nullptr, l->h_stats + f * 8}));
        HIPCHK(l, hipGetLastError());
        HIPCHK(l, hipEventRecord(l->lane_done[j], st));
        if (r != l) { HIPCHK(l, hipEventRecord(r->lane_readers_done[j], st)); r->readers_stream[j] = st; }
        // the L1 refinement reads both level-0 planes in place: a landing buffer is free for the next upload only after this point
        if (l->last_stage >= 0) HIPCHK(l, hipEventRecord(l->ev_consumed[l->last_stage][j], st));
        if (r != l && r->last_stage >= 0) HIPCHK(l, hipEventRecord(r->ev_consumed[r->last_stage][j], st));
    }
    if (r != l) {
        r->has_readers = true;
        r->readers_K = l->K;
        r->readers_n = n;
        // the right handle's extract kernels finished before the left lanes started matching (waits above), so the left lanes'
        // events are the ones a refill of the right landing buffer has to wait for
        if (r->last_stage >= 0) r->consumed_K[r->last_stage] = l->K;
    }
    l->stereo_done = true;
    l->l1_view = l->st_l1;
    l->st_mirror_valid = false;
    l->st_mirror_pending = direct;
    l->stereo_pairs = n;
    l->counts_synced = false;
    return JSORB_OK;
}

const float *jsorb_stereo_uright_device(const jsorb_extractor *l, int image)
{
    return (check_image(l, image) && l->stereo_done) ? l->st_u + (size_t)image * l->g.T : nullptr;
}
const float *jsorb_stereo_depth_device(const jsorb_extractor *l, int image)
{
    return (check_image(l, image) && l->stereo_done) ? l->st_d + (size_t)image * l->g.T : nullptr;
}

int jsorb_copy_stereo(const jsorb_extractor *l, int image, float *u_right, float *depth, jsorb_stereo_stats *stats)
{
    if (!check_image(l, image) || !l->stereo_done) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(l, image);
    if (l->st_mirror_valid && image == 0) {
        if (n > 0 && u_right) memcpy(u_right, l->h_u, (size_t)n * 4);
        if (n > 0 && depth) memcpy(depth, l->h_d, (size_t)n * 4);
    } else {
        if (n > 0 && u_right && hipMemcpy(u_right, l->st_u + (size_t)image * l->g.T, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
        if (n > 0 && depth && hipMemcpy(depth, l->st_d + (size_t)image * l->g.T, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return JSORB_ERR_HIP;
    }
    if (stats) {
        const int *s = l->h_stats + image * 8;
        stats->n_left = n;
        stats->n_right = -1;
        stats->n_candidate_pairs = s[0];
        stats->n_corr_match = s[1];
        stats->n_depth = s[2];
        stats->n_final = s[3];
    }
    return JSORB_OK;
}

int jsorb_copy_stereo_l1(const jsorb_extractor *l, int image, int32_t *dst)
{
    if (!check_image(l, image) || !l->stereo_done || !dst || !l->l1_view) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(l, image);
    if (n <= 0) return JSORB_OK;
    return hipMemcpy(dst, l->l1_view + (size_t)image * l->g.T, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

int jsorb_set_stereo_diagnostics(jsorb_extractor *l, int on)
{
    if (!l) return JSORB_ERR_INVALID;
    HIPCHK(l, hipSetDevice(l->device));
    if (on && !l->st_diag) {
        const size_t n = (size_t)l->B * l->g.T * JSORB_STEREO_DIAG_INTS * sizeof(int);
        HIPCHK(l, hipMalloc(&l->st_diag, n));
        HIPCHK(l, hipMemset(l->st_diag, 0xFF, n));
        // hipMemset on device memory returns before the fill has run, and the fill is ordered with the NULL stream only - the handles' streams are non-blocking.
        // Without this wait the fill could land on top of what the next k_stereo had already written: the arg-min / window-list diagnostics of a few hundred
        // keypoints read back as -1 while every product output was right (caught by tools/micro/chain_stress.py in round 5: 1 iteration in ~6 000; in all
        // likelihood also the "unexplained failure of the full GPU suite" of round 4, the round that introduced this hook and the test that reads it)
        HIPCHK(l, hipDeviceSynchronize());
    } else if (!on && l->st_diag) {
        HIPCHK(l, hipDeviceSynchronize());
        HIPCHK(l, hipFree(l->st_diag));
        l->st_diag = nullptr;
    }
    return JSORB_OK;
}
int jsorb_copy_stereo_diagnostics(const jsorb_extractor *l, int image, int32_t *dst)
{
    if (!check_image(l, image) || !l->stereo_done || !dst || !l->st_diag) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(l, image);
    if (n <= 0) return JSORB_OK;
    return hipMemcpy(dst, l->st_diag + (size_t)image * l->g.T * JSORB_STEREO_DIAG_INTS, (size_t)n * JSORB_STEREO_DIAG_INTS * 4, hipMemcpyDeviceToHost) == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

int jsorb_gather_counts_async(jsorb_extractor *l, jsorb_extractor *r, int32_t *dev_dst)
{
    if (!l || !r || !dev_dst) return JSORB_ERR_INVALID;
    if (!l->stereo_done || l->n_images != r->n_images) { l->err = "gather_counts needs a finished stereo batch"; return JSORB_ERR_STATE; }
    HIPCHK(l, hipSetDevice(l->device));
    for (int j = 0; j < l->K; j++)                                                                         // all lanes' statistics
        if (lane_stream(l, j) != l->stream) HIPCHK(l, hipStreamWaitEvent(l->stream, l->lane_done[j], 0));
    for (int j = 0; j < r->K; j++)
        if (lane_stream(r, j) != l->stream) HIPCHK(l, hipStreamWaitEvent(l->stream, r->lane_done[j], 0));
    launch_gather_counts(l->counts, r->counts, l->st_stats, dev_dst, l->n_images, l->stream);
    HIPCHK(l, hipGetLastError());
    HIPCHK(l, hipEventRecord(l->lane_done[0], l->stream));      // "everything of this handle so far" now includes the gather (it waited for every lane)
    // the next batch of either handle rewrites the count tables the gather kernel reads: their lanes continue after it
    HIPCHK(l, hipEventRecord(l->ev_fork, l->stream));
    for (jsorb_extractor *h : {l, r})
        for (int j = 0; j < h->K; j++)
            if (lane_stream(h, j) != l->stream) HIPCHK(l, hipStreamWaitEvent(lane_stream(h, j), l->ev_fork, 0));
    return JSORB_OK;
}

int jsorb_stereo_match(jsorb_extractor *l, jsorb_extractor *r, float mb, float mbf, int th_high, int th_low, float *u_right,
                       float *depth, jsorb_stereo_stats *stats)
{
    if (!l || !r) return JSORB_ERR_INVALID;
    const double t0 = l->trace_host ? now_us() : 0.0;
    int rc;
    bool adopt = false;
    if (jsorb_spec_state *S = l->spec) {
        // this very match may already be on the GPU, enqueued behind the two extracts (struct jsorb_spec_state)
        std::lock_guard<std::mutex> lk(S->mu);
        adopt = !l->st_diag && S->l == l && S->r == r && S->inflight && S->l_seq == l->spec_seq && S->r_seq == r->spec_seq && S->mb == mb && S->mbf == mbf &&
                S->th_high == th_high && S->th_low == th_low && l->extracted && r->extracted && l->n_images == 1 && r->n_images == 1 && !l->stereo_done;
        if (adopt) { S->inflight = false; S->n_adopted++; }
    }
    if (adopt) {
        HIPCHK(l, hipSetDevice(l->device));
        const double t1 = l->trace_host ? now_us() : 0.0;
        if ((rc = wait_event(l, l->spec->ev_done, l->spin_wait != 0))) return rc;
        if (!l->counts_synced && (rc = jsorb_sync(l))) return rc;          // extracts enqueued through the asynchronous calls
        std::swap(l->st_u, l->sp_u); std::swap(l->st_d, l->sp_d); std::swap(l->st_stats, l->sp_stats);
        std::swap(l->h_u, l->h_sp_u); std::swap(l->h_d, l->h_sp_d); std::swap(l->h_stats, l->h_sp_stats);
        l->stereo_done = true;
        l->l1_view = l->sp_l1;
        l->stereo_pairs = 1;
        l->st_mirror_valid = true;
        l->st_mirror_pending = false;
        if (l->trace_host) { l->th_st_enq += t1 - t0; l->th_st_wait += now_us() - t1; l->th_st_n++; }
    } else {
        rc = jsorb_stereo_match_batch_async(l, r, mb, mbf, th_high, th_low);
        if (rc) return rc;
        const double t1 = l->trace_host ? now_us() : 0.0;
        rc = jsorb_sync(l);
        if (rc) return rc;
        if (l->trace_host) { l->th_st_enq += t1 - t0; l->th_st_wait += now_us() - t1; l->th_st_n++; }
        if (l != r && l->speculate && l->n_images == 1 && !l->timing && !r->timing && (rc = spec_arm(l, r, mb, mbf, th_high, th_low))) return rc;
    }
    rc = jsorb_copy_stereo(l, 0, u_right, depth, stats);
    if (rc) return rc;
    if (stats) stats->n_right = jsorb_n_keypoints(r, 0);
    return JSORB_OK;
}

int jsorb_set_speculative_stereo(jsorb_extractor *l, int on)
{
    if (!l) return JSORB_ERR_INVALID;
    l->speculate = l->speculate_env >= 0 ? l->speculate_env : (on ? 1 : 0);
    if (!l->speculate && l->spec) { (void)hipSetDevice(l->device); spec_detach(l->spec); }
    return JSORB_OK;
}

int jsorb_speculative_stereo_stats(const jsorb_extractor *l, long *n_adopted, long *n_dropped)
{
    if (!l) return JSORB_ERR_INVALID;
    long a = 0, d = 0;
    if (jsorb_spec_state *S = l->spec) { std::lock_guard<std::mutex> lk(S->mu); a = S->n_adopted; d = S->n_dropped; }
    if (n_adopted) *n_adopted = a;
    if (n_dropped) *n_dropped = d;
    return JSORB_OK;
}

// ---- memory calls behind orb_cuda::SyncedMem<T> (include/jsorb_compat.hpp) ----
static thread_local std::string g_mem_err;
#define MEMCHK(call)                                                              \
    do {                                                                          \
        hipError_t _s = (call);                                                   \
        if (_s != hipSuccess) {                                                   \
            g_mem_err = std::string(#call) + ": " + hipGetErrorString(_s);        \
            return JSORB_ERR_HIP;                                                 \
        }                                                                         \
    } while (0)

const char *jsorb_mem_last_error(void) { return g_mem_err.c_str(); }
int jsorb_mem_set_device(int device_id) { MEMCHK(hipSetDevice(device_id)); return JSORB_OK; }
int jsorb_mem_alloc_host(size_t bytes, void **host_pinned)
{
    if (!host_pinned) return JSORB_ERR_INVALID;
    *host_pinned = nullptr;
    if (bytes == 0) return JSORB_OK;
    MEMCHK(hipHostMalloc(host_pinned, bytes));
    return JSORB_OK;
}
int jsorb_mem_alloc_device(size_t bytes, void **device)
{
    if (!device) return JSORB_ERR_INVALID;
    *device = nullptr;
    if (bytes == 0) return JSORB_OK;
    MEMCHK(hipMalloc(device, bytes));
    return JSORB_OK;
}
int jsorb_mem_alloc_device_pitched(size_t width_bytes, size_t height, void **device, size_t *pitch)
{
    if (!device || !pitch) return JSORB_ERR_INVALID;
    *device = nullptr; *pitch = 0;
    if (width_bytes == 0 || height == 0) return JSORB_OK;
    MEMCHK(hipMallocPitch(device, pitch, width_bytes, height));
    return JSORB_OK;
}
int jsorb_mem_free_host(void *p) { if (p) MEMCHK(hipHostFree(p)); return JSORB_OK; }
int jsorb_mem_free_device(void *p) { if (p) MEMCHK(hipFree(p)); return JSORB_OK; }
int jsorb_mem_stream_create(void **stream)
{
    if (!stream) return JSORB_ERR_INVALID;
    hipStream_t s = nullptr;
    MEMCHK(hipStreamCreate(&s));         // blocking flag like cudaStreamCreate: ordered against the null stream
    *stream = (void *)s;
    return JSORB_OK;
}
int jsorb_mem_stream_destroy(void *stream) { if (stream) MEMCHK(hipStreamDestroy((hipStream_t)stream)); return JSORB_OK; }
int jsorb_mem_stream_sync(void *stream) { MEMCHK(hipStreamSynchronize((hipStream_t)stream)); return JSORB_OK; }
int jsorb_mem_device_sync(void) { MEMCHK(hipDeviceSynchronize()); return JSORB_OK; }
// the same wait for the device that OWNS a buffer, whatever the calling thread's current device is (a SyncedMem may be released by a thread that
// has selected another GPU); the current device is restored
int jsorb_mem_buffer_sync(const void *device_ptr)
{
    int cur = -1, dev = -1;
    MEMCHK(hipGetDevice(&cur));
    hipPointerAttribute_t at{};
    if (device_ptr && hipPointerGetAttributes(&at, device_ptr) == hipSuccess) dev = at.device;
    else (void)hipGetLastError();
    if (dev >= 0 && dev != cur) MEMCHK(hipSetDevice(dev));
    const hipError_t rc = hipDeviceSynchronize();
    if (dev >= 0 && dev != cur) (void)hipSetDevice(cur);
    MEMCHK(rc);
    return JSORB_OK;
}
int jsorb_mem_h2d(void *d, const void *h, size_t n) { if (n) MEMCHK(hipMemcpy(d, h, n, hipMemcpyHostToDevice)); return JSORB_OK; }
int jsorb_mem_d2h(void *h, const void *d, size_t n) { if (n) MEMCHK(hipMemcpy(h, d, n, hipMemcpyDeviceToHost)); return JSORB_OK; }
int jsorb_mem_d2d(void *d, const void *s, size_t n) { if (n) MEMCHK(hipMemcpy(d, s, n, hipMemcpyDeviceToDevice)); return JSORB_OK; }
int jsorb_mem_h2d_async(void *d, const void *h, size_t n, void *st) { if (n) MEMCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, (hipStream_t)st)); return JSORB_OK; }
int jsorb_mem_d2h_async(void *h, const void *d, size_t n, void *st) { if (n) MEMCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, (hipStream_t)st)); return JSORB_OK; }
int jsorb_mem_d2d_async(void *d, const void *s, size_t n, void *st) { if (n) MEMCHK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st)); return JSORB_OK; }
int jsorb_mem_set_zero(void *d, size_t n) { if (n) MEMCHK(hipMemset(d, 0, n)); return JSORB_OK; }
int jsorb_mem_set_zero_async(void *d, size_t n, void *st) { if (n) MEMCHK(hipMemsetAsync(d, 0, n, (hipStream_t)st)); return JSORB_OK; }

int jsorb_enable_kernel_timing(jsorb_extractor *e, int on)
{
    if (!e) return JSORB_ERR_INVALID;
    e->timing = on != 0;
    return JSORB_OK;
}
int jsorb_kernel_time(jsorb_extractor *e, int id, double *total_ms, long *launches)
{
    if (!e || id < 0 || id >= JSORB_K_ID_END || (id >= JSORB_K_COUNT_ALL && id < JSORB_K_ASSIGN_GRID)) return JSORB_ERR_INVALID;
    int rc = drain_timed(e);
    if (rc) return rc;
    if (total_ms) *total_ms = e->k_ms[id];
    if (launches) *launches = e->k_n[id];
    return JSORB_OK;
}
int jsorb_reset_kernel_timing(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    int rc = drain_timed(e);
    for (int i = 0; i < JSORB_K_ID_END; i++) { e->k_ms[i] = 0; e->k_n[i] = 0; }
    return rc;
}

} // extern "C"
