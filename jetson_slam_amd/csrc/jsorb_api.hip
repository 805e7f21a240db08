// jsorb_api.hip - host side of libjsorb, the C ABI declared in include/jsorb.h: handle creation and destruction, geometry and launch plan,
// the lane / copy / main stream pools and the spill arena, streams and synchronisation, level getters, the memory calls and kernel timing.
// The extract pipeline is in jsorb_extract.hip, the stereo match in jsorb_stereo.hip, the Frame-side features in jsorb_frame.hip, the grid
// matchers in jsorb_search.hip; the handle and the host helpers they share in jsorb_handle.h.
//
// Mirrors ORB_GPU's host orchestration (src/cuda/orb_gpu.cpp) with an MI355X-first structure:
//   reference: ~7L+1 launches on L streams + 3 blocking copies + 2 full stream-sync rounds per image,
//              per-frame cudaMalloc/cudaFree + cublasCreate/Destroy in the stereo matcher
//   here:      5 launches per BATCH of images (pyramid, detect, compact, blur, describe) + 2 per batch of pairs
//              (stereo, median) on one stream, no host round trip in the middle, one small D2H of counts at the end,
//              nothing allocated after jsorb_create.
#include "jsorb_handle.h"

namespace {

const char *k_names[JSORB_K_COUNT_ALL] = {"k_pyramid", "k_detect", "k_compact", "k_blur", "k_describe", "k_stereo", "k_median", "k_nms_ms", "k_rectify",
                                          "k_undistort", "k_rgbd"};
// kernels of jsorb_search_local_points*: ids JSORB_K_ASSIGN_GRID .. JSORB_K_ID_END - 1 (JSORB_K_COUNT_ALL itself names no kernel)
const char *k_names_local[JSORB_K_ID_END - JSORB_K_ASSIGN_GRID] = {"k_assign_grid", "k_local_candidates", "k_local_resolve"};
// kernels of jsorb_search_last_frame*: ids JSORB_K_ID_END .. JSORB_K_ID_COUNT - 1
const char *k_names_last[JSORB_K_ID_COUNT - JSORB_K_ID_END] = {"k_last_match", "k_last_resolve"};
// kernels of jsorb_bow_transform* / jsorb_search_by_bow*: ids JSORB_K_BOW_TRANSFORM .. JSORB_K_ID_ALL - 1 (JSORB_K_ID_COUNT itself names no kernel)
const char *k_names_bow[JSORB_K_ID_ALL - JSORB_K_BOW_TRANSFORM] = {"k_bow_transform", "k_bow_group", "k_bow_match", "k_bow_resolve"};
// kernels of jsorb_search_by_projection_kf*: ids JSORB_K_KF_CANDIDATES .. JSORB_K_ID_LAST - 1 (JSORB_K_ID_ALL itself names no kernel)
const char *k_names_kf[JSORB_K_ID_LAST - JSORB_K_KF_CANDIDATES] = {"k_kf_candidates", "k_kf_resolve"};

// HIP multiplexes every stream of a process over GPU_MAX_HW_QUEUES hardware queues (default 4), and a stream that waits for an event
// holds up every other stream that shares its queue.  This library runs 4 lane streams + 1 upload stream + one main stream per handle;
// on 4 queues which of them share is decided by creation order (measured with otherwise identical code, only the number of idle streams
// created earlier differing: 85.7 k against 91.4 k pairs/s device-resident, 47 k against 71 k host-streamed).  Sixteen queues give every
// stream of a few handle pairs its own (8 were not enough for bench.py, which keeps two sets of handles alive).  Where the user has set fewer, the
// lane pool is created in the order that still gives the four lanes of the device-resident batch path a queue each (pool_create below).
// The variable is read when the HIP runtime initialises (its first API call), so this
// constructor - run when the library is loaded - is early enough for a process that links the library or imports the Python binding
// before it touches the GPU; an explicit setting by the user wins.  ("Runtime environment")
// JSORB_NO_ENV=1 forbids it: an integrator who does not want a library to touch the process environment sets the variable itself (or not).
__attribute__((constructor)) void jsorb_runtime_defaults()
{
    const char *no = product_env("JSORB_NO_ENV");
    if (!(no && atoi(no) != 0)) setenv("GPU_MAX_HW_QUEUES", "16", 0);
}

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
    int n_main = 0;                 // main streams created on this device so far (pool_create)
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


// Main streams are recycled, never destroyed: which hardware queue HIP gives a new stream depends on every stream created and destroyed
// before it, and a process that had closed one handle pair and opened another (same code, same sizes) measured 57 k instead of 68 k
// pairs/s in the host-streamed regime.  With recycled streams the stream -> queue assignment of the process settles once.
//
// Which hardware queue a stream gets is decided when it is CREATED, so the device's first four lane streams are created here, with the device's first
// handle that can run a multi-lane batch (max_batch > 1), in an order that leaves each of them a queue of its own even with four queues.  The runtime
// gives a new stream a new queue until GPU_MAX_HW_QUEUES exist and from then on the queue with the fewest streams - among equals the one created LAST
// (rocprofv3 queue ids, profiles/r09_overlap.txt).  The legacy stream holds the first queue (torch, hipMemset: touched below so that it does in every
// process).  With four queues the next three streams therefore take the three new queues, and from the fourth stream on any FOUR CONSECUTIVE streams
// land on four different queues (q4, q3, q2, q1, q4, ...).  So: three main streams first (those the device's handles have created already count; the
// rest are kept for the next handles), then lanes 0-3 in a row.  Every lane then shares its queue with a main stream or with the legacy stream, which are
// idle while a multi-lane batch runs; single frames and one-lane batches, which do run on a main stream, use no lane.  (Lanes created lazily in
// run_pipeline, behind the legacy stream and TWO main streams: lanes 0 and 1 on ONE queue, never four kernels in flight, 118 k against 130 k pairs/s at
// C2.)  With eight or more queues every stream of a handle pair has its own in any order.
// A handle that takes single images only (max_batch = 1: the C++ shim's) never uses a lane and does not bring the pool up: in a process of such
// handles the streams are what they were - with the pool's seven streams ahead of them the frame took 175 us instead of 133 (the shim's own streams
// then share queues with the main streams).
#ifndef JSORB_POOL_MAINS_AHEAD
#define JSORB_POOL_MAINS_AHEAD 3
#endif
int pool_create(jsorb_extractor *e, LanePool &p)      // p.m is held
{
    if (p.s[0]) return JSORB_OK;
    HIPCHK(e, hipStreamSynchronize(nullptr));      // (jsorb_create waits for the whole device at its end anyway)
    for (; p.n_main < JSORB_POOL_MAINS_AHEAD; p.n_main++) {
        hipStream_t s = nullptr;
        HIPCHK(e, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        p.idle_main.insert(p.idle_main.begin(), s);      // handed out in creation order
    }
    for (int j = 0; j < std::min(4, JSORB_MAX_LANES); j++) HIPCHK(e, hipStreamCreateWithFlags(&p.s[j], hipStreamNonBlocking));
    return JSORB_OK;
}

int pool_main_stream(jsorb_extractor *e, hipStream_t *out)
{
    LanePool &p = g_pool[e->device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    if (e->B > 1) RCCHK(pool_create(e, p));
    if (!p.idle_main.empty()) { *out = p.idle_main.back(); p.idle_main.pop_back(); return JSORB_OK; }
    HIPCHK(e, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    p.n_main++;
    return JSORB_OK;
}
void pool_return_main_stream(int device, hipStream_t s)
{
    LanePool &p = g_pool[device & 15];
    std::lock_guard<std::mutex> lk(p.m);
    p.idle_main.push_back(s);
}

// Uploads of a destroyed handle still in flight on the device's copy stream read caller memory and write the handle's landing buffers.
void sync_copy_stream(int device)
{
    LanePool &lp = g_pool[device & 15];
    hipStream_t cs;
    { std::lock_guard<std::mutex> lk(lp.m); cs = lp.copy; }
    if (cs) (void)hipStreamSynchronize(cs);
}

// The core buffers of jsorb_create_masked (the features release their own: jsorb_destroy)
void core_release(jsorb_extractor *e)
{
    free_device(e->slab, e->blur, e->mask, e->lut_bits, e->tile_out, e->kp, e->counts, e->row_tab, e->angles, e->desc, e->out_kp, e->ms_grid, e->ms_scratch);
    free_pinned(e->h_counts);
    destroy_event(e->lanes.ev_fork);
    for (int j = 0; j < JSORB_MAX_LANES; j++) destroy_event(e->lanes.done[j], e->lanes.readers_done[j]);
}

} // namespace

namespace jsorb_host __attribute__((visibility("hidden"))) {

int drain_timed(jsorb_extractor *e)
{
    for (auto &t : e->tm.timed) {
        float ms = 0.f;
        HIPCHK(e, hipEventSynchronize(t.b));
        HIPCHK(e, hipEventElapsedTime(&ms, t.a, t.b));
        e->tm.k_ms[t.id] += ms;
        e->tm.k_n[t.id] += 1;
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    e->tm.timed.clear();
    return JSORB_OK;
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

} // namespace jsorb_host

extern "C" {

const char *jsorb_version(void) { return "jsorb 0.1 (gfx950)"; }

const char *jsorb_kernel_name(int id)
{
    if (id >= 0 && id < JSORB_K_COUNT_ALL) return k_names[id];
    if (id >= JSORB_K_ASSIGN_GRID && id < JSORB_K_ID_END) return k_names_local[id - JSORB_K_ASSIGN_GRID];
    if (id >= JSORB_K_ID_END && id < JSORB_K_ID_COUNT) return k_names_last[id - JSORB_K_ID_END];
    if (id >= JSORB_K_BOW_TRANSFORM && id < JSORB_K_ID_ALL) return k_names_bow[id - JSORB_K_BOW_TRANSFORM];
    if (id >= JSORB_K_KF_CANDIDATES && id < JSORB_K_ID_LAST) return k_names_kf[id - JSORB_K_KF_CANDIDATES];
    return "";
}

const char *jsorb_last_error(const jsorb_extractor *e) { return e ? e->err.c_str() : "null handle"; }

int jsorb_create(const jsorb_params *params, const uint8_t *mask, jsorb_extractor **out) { return jsorb_create_masked(params, mask, params ? params->width : 0, params ? params->height : 0, out); }

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
    RCCHK(build_geometry(*params, g, err));
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

// NMS-MS in the reference's CPU mode: k_nms_ms's tables of that mode hold at most 32768 tiles
static bool nms_ms_cpu_supported(const Geometry &g) { return g.T <= 32768 && g.lv[0].nth * g.lv[0].ntw <= 65535; }

// out[0..7] of jsorb_plan_forms / jsorb_handle_forms: the kernel forms the geometry selects, from the same rules the launch code applies
static void geometry_forms(const Geometry &g, bool frame_fuse, int32_t *out)
{
    int replay = 0;
    for (int i = 0; i < g.L; i++) replay += g.lv[i].tree_rank_ok ? 0 : 1;
    out[0] = g.det_compact; out[1] = compact_form(g); out[2] = g.epi_rows != 0; out[3] = blur_compact_fusable(g) ? 1 : 0;
    out[4] = frame_fuse ? 1 : 0; out[5] = replay; out[6] = nms_ms_cpu_supported(g) ? 1 : 0; out[7] = 0;
}

int jsorb_plan_forms(const jsorb_params *params, int32_t *out, int capacity)
{
    if (!params || !out || capacity < 8) return JSORB_ERR_INVALID;
    Geometry g;
    std::string err;
    RCCHK(build_geometry(*params, g, err));
    plan_detect(g);
    // (jsorb_create may raise the full-plane k_detect's LDS request, to at most 40 KB: that never crosses the bound of the fused launch)
    geometry_forms(g, detect_blur_fusable(g, detect_lds_bytes(g)), out);
    return JSORB_OK;
}

int jsorb_handle_forms(const jsorb_extractor *e, int32_t *out, int capacity)
{
    if (!e || !out || capacity < 12) return JSORB_ERR_INVALID;
    geometry_forms(e->g, frame_fuses_detect_blur(e), out);
    out[8] = e->extracted ? e->lanes.K : 0;
    out[9] = e->extracted ? e->lanes.order : -1;
    out[10] = e->extracted ? (int32_t)e->lanes.fuse_bc_mask : 0;
    out[11] = e->extracted ? (int32_t)e->lanes.blur_first_mask : 0;
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
    RCCHK(build_geometry(*params, e->g, e->err));
    Geometry &g = e->g;
    g.has_mask = mask ? 1 : 0;
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(pool_main_stream(e, &e->own_stream));
    e->stream = e->own_stream;
    HIPCHK(e, hipEventCreateWithFlags(&e->lanes.ev_fork, hipEventDisableTiming));
    for (int j = 0; j < JSORB_MAX_LANES; j++) {      // (the lane STREAMS belong to the device's pool: pool_create made the first four for a handle that takes batches, lanes 4-7 are created on first use)
        HIPCHK(e, hipEventCreateWithFlags(&e->lanes.done[j], hipEventDisableTiming));
        HIPCHK(e, hipEventCreateWithFlags(&e->lanes.readers_done[j], hipEventDisableTiming));
    }
    if (const char *ml = product_env("JSORB_MAX_LANES")) e->lanes.max = std::max(1, std::min(JSORB_MAX_LANES, atoi(ml)));
    if (const char *sw = experiment_env("JSORB_SPIN_WAIT")) e->spin_wait = atoi(sw);
    if (const char *sp = product_env("JSORB_SPECULATE")) { e->st.speculate_env = atoi(sp) != 0; e->st.speculate = e->st.speculate_env; }
    if (const char *ku = experiment_env("JSORB_KERNEL_UPLOAD")) e->up.kernel = atoi(ku);
    if (const char *hl = experiment_env("JSORB_HOST_LANES")) e->land.host_lanes = std::max(1, std::min(JSORB_MAX_LANES, atoi(hl)));
    if (const char *tr = experiment_env("JSORB_TRACE_HOST")) e->trace.on = atoi(tr) != 0;
    if (const char *fg = product_env("JSORB_FRAME_GRAPH")) e->fg.on = atoi(fg);
    if (const char *mp = product_env("JSORB_LANE_MIN_MPX")) e->lanes.min_px = std::max(0.01, atof(mp)) * 1e6;
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
    RCCHK(landing_create(e));
    HIPCHK(e, hipMalloc(&e->lut_bits, (2048 + (size_t)g.detect_blocks + g.blur_blocks + g.pyr_blocks + 64 * JSORB_MAX_LEVELS) * sizeof(uint32_t)));      // arc LUT + workgroup tables + tree priorities
    HIPCHK(e, hipMalloc(&e->tile_out, B * T * 8));
    HIPCHK(e, hipMalloc(&e->kp, B * T * 8));
    HIPCHK(e, hipMalloc(&e->counts, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    HIPCHK(e, hipMalloc(&e->row_tab, B * (size_t)g.row_tab_stride * sizeof(int)));
    HIPCHK(e, hipMalloc(&e->angles, B * T * 4));
    HIPCHK(e, hipMalloc(&e->desc, B * T * 32));
    HIPCHK(e, hipMalloc(&e->out_kp, B * T * 6 * 4));
    RCCHK(stereo_create(e));
    if (e->nms_ms) {
        if (params->nms_ms_mode_gpu) {
            const size_t n = B * (size_t)g.lv[0].H * g.lv[0].W * sizeof(int);
            HIPCHK(e, hipMalloc(&e->ms_grid, n));
            HIPCHK(e, hipMemset(e->ms_grid, 0, n));
        } else {
            if (!nms_ms_cpu_supported(g)) { e->err = "NMS-MS CPU mode supports at most 32768 tiles"; return JSORB_ERR_UNSUPPORTED; }
            HIPCHK(e, hipMalloc(&e->ms_scratch, B * T * sizeof(int)));
        }
    }
    HIPCHK(e, hipMemset(e->counts, 0, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    HIPCHK(e, hipHostMalloc(&e->h_counts, B * (JSORB_MAX_LEVELS + 1) * sizeof(int)));
    memset(e->h_counts, 0, B * (JSORB_MAX_LEVELS + 1) * sizeof(int));
    RCCHK(results_create(e));
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

void jsorb_destroy(jsorb_extractor *e)
{
    if (!e) return;
    if (e->trace.on && e->trace.n)
        fprintf(stderr, "[jsorb host trace] extract x%ld: h2d enqueue %.1f us, kernel enqueue %.1f us, wait %.1f us ; stereo x%ld: enqueue %.1f us, wait %.1f us\n",
                e->trace.n, e->trace.h2d / e->trace.n, e->trace.enq / e->trace.n, e->trace.wait / e->trace.n, e->trace.st_n, e->trace.st_n ? e->trace.st_enq / e->trace.st_n : 0.0,
                e->trace.st_n ? e->trace.st_wait / e->trace.st_n : 0.0);
    (void)hipSetDevice(e->device);
    spec_detach(e->st.spec);        // waits for a speculative match that still reads this handle's buffers; the partner continues unpaired
    if (e->own_stream) (void)hipStreamSynchronize(e->own_stream);
    if (e->lanes.has_readers)       // a stereo match enqueued through another handle may still be reading this handle's buffers
        for (int j = 0; j < e->lanes.readers_K; j++) (void)hipEventSynchronize(e->lanes.readers_done[j]);
    for (int j = 0; j < e->lanes.K; j++)
        if (e->lanes.used[j]) (void)hipStreamSynchronize(e->lanes.used[j]);
    sync_copy_stream(e->device);
    // every kernel and copy of this handle has finished: each feature frees what it allocated
    for (auto &t : e->tm.timed) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
    extract_release(e);
    stereo_release(e);
    rectify_release(e);
    camera_release(e);
    rgbd_release(e);
    grid_release(e);
    search_local_release(e);
    local_map_release(e);
    local_kf_release(e);
    pose_release(e);
    search_last_release(e);
    search_kf_release(e);
    search_init_release(e);
    bow_release(e);
    core_release(e);
    arena_release(e->det_spill);
    if (e->own_stream) { (void)hipStreamSynchronize(e->own_stream); pool_return_main_stream(e->device, e->own_stream); }
    delete e;
}

int jsorb_set_stream(jsorb_extractor *e, void *hip_stream)
{
    if (!e) return JSORB_ERR_INVALID;
    hipStream_t ns = hip_stream ? (hipStream_t)hip_stream : e->own_stream;
    if (ns != e->stream && e->extracted) {      // the new main stream continues after whatever the old one (and the lanes) were doing
        HIPCHK(e, hipSetDevice(e->device));
        RCCHK(wait_lanes(e, ns, e));
        if (e->lanes.main_stream_dirty) {       // ... and after the readers of the last results the old one still carries (the mark stays: the lanes have not seen them)
            HIPCHK(e, hipEventRecord(e->lanes.ev_fork, e->stream));
            HIPCHK(e, hipStreamWaitEvent(ns, e->lanes.ev_fork, 0));
        }
    }
    e->stream = ns;
    return JSORB_OK;
}
void *jsorb_get_stream(const jsorb_extractor *e) { return e ? (void *)e->stream : nullptr; }

int jsorb_stream_wait_done(jsorb_extractor *e, void *other)
{
    if (!e) return JSORB_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->device));
    return wait_lanes(e, (hipStream_t)other, e);
}

int jsorb_sync(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->device));
    // single frame: a blocking hipStreamSynchronize adds tens of microseconds of wake-up latency per call (three calls per stereo frame).
    // Poll the stream instead (bounded), then fall through to the blocking calls.
    bool done;
    if (e->extracted && e->lanes.K == 1 && e->n_images == 1 && e->spin_wait) RCCHK(spin_poll(e, [e] { return hipStreamQuery(e->stream); }, "hipStreamQuery", &done));
    if (e->extracted)
        for (int j = 0; j < e->lanes.K; j++) HIPCHK(e, hipStreamSynchronize(lane_stream(e, j)));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->lanes.main_stream_dirty = false;       // nothing is left on the main stream for the next batch's lanes to wait for
    e->counts_synced = true;
    mirrors_landed(e);
    return drain_timed(e);
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
    e->tm.on = on != 0;
    return JSORB_OK;
}
int jsorb_kernel_time(jsorb_extractor *e, int id, double *total_ms, long *launches)
{
    if (!e || id < 0 || id >= JSORB_K_ID_LAST || id == JSORB_K_ID_ALL || id == JSORB_K_ID_COUNT || (id >= JSORB_K_COUNT_ALL && id < JSORB_K_ASSIGN_GRID)) return JSORB_ERR_INVALID;
    RCCHK(drain_timed(e));
    if (total_ms) *total_ms = e->tm.k_ms[id];
    if (launches) *launches = e->tm.k_n[id];
    return JSORB_OK;
}
int jsorb_reset_kernel_timing(jsorb_extractor *e)
{
    if (!e) return JSORB_ERR_INVALID;
    int rc = drain_timed(e);
    for (int i = 0; i < JSORB_K_ID_LAST; i++) { e->tm.k_ms[i] = 0; e->tm.k_n[i] = 0; }
    return rc;
}

} // extern "C"

