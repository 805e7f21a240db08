// jsorb_extract.hip - host side of the extract pipeline (ORB_GPU::extract, orb_gpu.cpp:489-841): lanes and their ordering, the single-frame
// graph, run_pipeline, landing buffers and uploads, the extract entry points, the synchronous single-frame path (kept in this one translation
// unit: it is host-bound) and the results of an extract (counts, copies, Frame-side unpacking).
#include "jsorb_handle.h"

// pyramid megapixels per lane and launch below which every lane of a batch runs the fused k_blur_compact launch (run_pipeline)
#ifndef JSORB_FUSE_ALL_BELOW_MPX
#define JSORB_FUSE_ALL_BELOW_MPX 24.0
#endif

namespace jsorb_host __attribute__((visibility("hidden"))) {

// Landing buffers of host batches (images of a width that is a multiple of 16 only: they are read in place as level 0) and their events.
int landing_create(jsorb_extractor *e)
{
    if (e->g.lv[0].W % 16 != 0) return JSORB_OK;
    for (int k = 0; k < 2; k++) {
        HIPCHK(e, hipMalloc(&e->land.stage[k], (size_t)e->B * e->g.lv[0].H * e->g.lv[0].W + 256));
        for (int j = 0; j < JSORB_MAX_LANES; j++) {
            HIPCHK(e, hipEventCreateWithFlags(&e->land.ev_copied[k][j], hipEventDisableTiming));
            HIPCHK(e, hipEventCreateWithFlags(&e->land.ev_consumed[k][j], hipEventDisableTiming));
        }
    }
    return JSORB_OK;
}

// Pinned mirrors of a single image's keypoints and descriptors (written by k_describe itself, struct Deliver).
int results_create(jsorb_extractor *e)
{
    HIPCHK(e, hipHostMalloc(&e->res.h_kp, (size_t)e->g.T * 6 * sizeof(int32_t)));
    HIPCHK(e, hipHostMalloc(&e->res.h_desc, (size_t)e->g.T * 32));
    return JSORB_OK;
}

// ---- the single-frame graph (struct jsorb_extractor: fg) ----
void frame_graph_drop(jsorb_extractor *e)
{
    if (e->fg.exec) { (void)hipGraphExecDestroy(e->fg.exec); e->fg.exec = nullptr; }
    if (e->fg.tmpl) { (void)hipGraphDestroy(e->fg.tmpl); e->fg.tmpl = nullptr; }
    e->fg.describe_node = nullptr;
    memset(e->fg.key, 0, sizeof e->fg.key);
}

// Waits for an event, polling first when `spin` (spin_poll)
int wait_event(jsorb_extractor *e, hipEvent_t ev, bool spin)
{
    bool done = false;
    if (spin) RCCHK(spin_poll(e, [ev] { return hipEventQuery(ev); }, "hipEventQuery", &done));
    if (!done) HIPCHK(e, hipEventSynchronize(ev));
    return JSORB_OK;
}

// The single-image call in flight has finished: the kernels' writes into the pinned mirrors (struct Deliver, DeliverStereo) have landed.
void mirrors_landed(jsorb_extractor *e)
{
    if (e->res.mirror_pending) { e->res.mirror_valid = true; e->res.mirror_pending = false; }
    if (e->st.mirror_pending) { e->st.mirror_valid = true; e->st.mirror_pending = false; }
}

// (the lanes, the device's copy stream and the handle's main stream have been synchronised)
void extract_release(jsorb_extractor *e)
{
    frame_graph_drop(e);
    destroy_event(e->up.ev_read);
    free_pinned(e->up.h_upload);
    free_device(e->land.stage[0], e->land.stage[1]);
    for (int k = 0; k < 2; k++)
        for (int j = 0; j < JSORB_MAX_LANES; j++) destroy_event(e->land.ev_copied[k][j], e->land.ev_consumed[k][j]);
    free_pinned(e->res.h_kp, e->res.h_desc);
    free_device(e->res.frame_aos);
}

bool frame_fuses_detect_blur(const jsorb_extractor *e)
{
    static const bool fuse_env = !env_is(experiment_env("JSORB_FUSED_DETECT_BLUR"), 0);
    return fuse_env && detect_blur_fusable(e->g, e->detect_lds);
}

} // namespace jsorb_host

namespace {

// Split n images into contiguous lanes.  A lane keeps at least ~7 Mpx of level-0 pixels (about 20 images of 752x480) so that each
// launch still fills the 256 CUs; per-kernel timing (which serialises launches anyway) and small batches use one lane.
int plan_lanes(const jsorb_extractor *e, int n, int *first)
{
    const double px = (double)e->g.lv[0].H * e->g.lv[0].W;
    const int min_per_lane = std::max(1, (int)std::ceil(e->lanes.min_px / px));
    int K = std::min(std::min(e->lanes.max, e->lanes.cap), n / min_per_lane);
    if (K < 1 || e->tm.on) K = 1;
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
//  * work the caller enqueued on a main stream of its own, or readers of the last results this handle enqueued on its main stream
//    (mark_main_stream): every lane that is not the main stream waits for a fork event recorded there
//  * the previous batch of this handle, when its lane partition differs (same partition: same-stream order is enough)
//  * a stereo match enqueued on ANOTHER handle's lanes that may still read this handle's previous results
//  * `input_ready` (optional, one event per lane): e.g. the upload of the lane's images on the copy stream
int order_lanes_for_new_batch(jsorb_extractor *e, int K, int n, const hipStream_t *ls, const hipEvent_t *input_ready)
{
    if ((K > 1 || ls[0] != e->stream) && (e->stream != e->own_stream || e->lanes.main_stream_dirty)) {
        // a caller-provided main stream may carry work the images depend on.  The handle's OWN stream carries this handle's work only: single frames
        // and one-lane batches, which the lanes order themselves against below through their `done` events - and whatever the library enqueued there
        // behind the last extract to read its results (matchers, BoW transform, the kept initial frame: mark_main_stream), which no `done` event covers
        // and which must have read out_kp / desc / counts / cam.un before this batch rewrites them.
        HIPCHK(e, hipEventRecord(e->lanes.ev_fork, e->stream));
        for (int j = 0; j < K; j++)
            if (ls[j] != e->stream) HIPCHK(e, hipStreamWaitEvent(ls[j], e->lanes.ev_fork, 0));
    }
    e->lanes.main_stream_dirty = false;
    // the previous batch of this handle: wherever a lane now runs on another stream than the lane that last touched its images (same partition:
    // lane j waits for lane j only)
    const bool same_split = K == e->lanes.K && n == e->n_images, aligned = e->lanes.readers_K == K && e->lanes.readers_n == n;
    for (int j = 0; j < K && e->extracted; j++)
        RCCHK(same_split ? wait_events(e, ls[j], e->lanes.used + j, e->lanes.done + j, 1) : wait_lanes(e, ls[j], e));
    // a stereo match enqueued through ANOTHER handle may still read this handle's previous results
    for (int j = 0; j < K && e->lanes.has_readers; j++)
        RCCHK(aligned ? wait_events(e, ls[j], e->lanes.readers_stream + j, e->lanes.readers_done + j, 1)
                      : wait_events(e, ls[j], e->lanes.readers_stream, e->lanes.readers_done, e->lanes.readers_K));
    e->lanes.has_readers = false;
    if (input_ready)            // per lane: e.g. the upload of this lane's images on the copy stream
        for (int j = 0; j < K; j++) HIPCHK(e, hipStreamWaitEvent(ls[j], input_ready[j], 0));
    return JSORB_OK;
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
    if (e->res.deliver_kp == e->fg.dst_kp && e->res.deliver_desc == e->fg.dst_desc) return true;
    if (!e->fg.describe_node || !e->fg.exec) return false;
    hipKernelNodeParams p{};
    if (hipGraphKernelNodeGetParams(e->fg.describe_node, &p) != hipSuccess || !p.kernelParams) { (void)hipGetLastError(); return false; }
    Deliver *dl = static_cast<Deliver *>(p.kernelParams[describe_kernel_deliver_arg()]);
    if (!dl) return false;
    dl->kp_dev = e->res.deliver_kp;
    dl->desc_dev = e->res.deliver_desc;
    if (hipGraphExecKernelNodeSetParams(e->fg.exec, e->fg.describe_node, &p) != hipSuccess) { (void)hipGetLastError(); return false; }
    e->fg.dst_kp = e->res.deliver_kp; e->fg.dst_desc = e->res.deliver_desc;
    return true;
}

// Lane order of a batch of n images on K lanes (round 6; every arm measured A/B on one box, profiles/r06_experiments.txt).  The lanes of a batch start together and run
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
int lane_order(const Geometry &g, int n, int K)
{
    double lane_mpx = 0;
    for (int l = 0; l < g.L; l++) lane_mpx += (double)g.lv[l].W * g.lv[l].H;
    lane_mpx *= (double)n / K * 1e-6;
    return experiment_env("JSORB_LANE_ORDER") ? atoi(experiment_env("JSORB_LANE_ORDER"))
                                              : ((K & 1) || lane_mpx < JSORB_FUSE_ALL_BELOW_MPX ? 0 : (g.lv[0].th <= 40 ? 1 : 2));      // (tall tiles as well: C3 / tile 46 +1.1 %, C2 / tile 58 with 64 pairs +1.7 %)
}

int run_pipeline(jsorb_extractor *e, int n, const hipEvent_t *input_ready = nullptr)
{
    const Geometry &g = e->g;
    int first[JSORB_MAX_LANES + 1];
    const int K = plan_lanes(e, n, first);
    hipStream_t ls[JSORB_MAX_LANES];
    if (K == 1) ls[0] = e->stream;                  // one lane (single frame, small batch, per-kernel timing): the handle's main stream
    else
        for (int j = 0; j < K; j++)
            RCCHK(pool_stream(e, j, &ls[j]));
    RCCHK(order_lanes_for_new_batch(e, K, n, ls, input_ready));
    const size_t T = (size_t)g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    // k_compact writes the counts of every image straight into the pinned host mirror (no copy behind the kernels, for batches as
    // well); for a single image k_describe also delivers keypoints and descriptors there and into the caller's device buffers
    // (jsorb_extract_into)
    const bool direct = n == 1;
    // single image: k_detect and k_blur (independent of each other) as ONE launch - a frame is a chain of small launches whose latencies add up
    const bool fused = direct && !e->tm.on && frame_fuses_detect_blur(e);
    const int order = lane_order(g, n, K);
    unsigned fuse_bc_mask = 0, blur_first_mask = 0;
    for (int j = 0; j < K; j++) {
        const int f = first[j], m = first[j + 1] - f;
        hipStream_t st = ls[j];
        ImageSrc src = e->src;
        src.l0 += (size_t)f * src.l0_stride;
        uint8_t *slab = e->slab + (size_t)f * g.slab_bytes, *blur = e->blur + (size_t)f * g.slab_bytes;
        unsigned long long *tile_out = e->tile_out + f * T, *kp = e->kp + f * T;
        int *counts = e->counts + f * CW;
        const ImageSrc raw = src;                   // with maps: the raw input k_rectify reads; level 0 is then its output in the slab
        if (e->rect.on) { src.l0 = slab; src.l0_stride = g.slab_bytes; src.l0_pitch = g.lv[0].pitch; }
        if (e->copy_kind == 1) {      // into what the lane reads as its input: the slab's level 0, or with maps the dense raw buffer (extract_batch_host_enqueue)
            for (int i = 0; i < m; i++)
                HIPCHK(e, hipMemcpy2DAsync(const_cast<uint8_t *>(raw.l0) + (size_t)i * raw.l0_stride, raw.l0_pitch, e->copy_src + (size_t)(f + i) * e->copy_stride,
                                           e->copy_step, g.lv[0].W, g.lv[0].H, hipMemcpyHostToDevice, st));
        } else if (e->copy_kind == 2) {
            launch_copy_level0(e->copy_src + (size_t)f * e->copy_stride, e->copy_stride, e->copy_step, e->slab + (size_t)f * g.slab_bytes, g.slab_bytes,
                               g.lv[0].pitch, g.lv[0].W, g.lv[0].H, m, st);
        }
        // single image on an untimed handle: replay the captured graph of the five launches when nothing they depend on has changed
        bool capturing = false;
        // (only on the handle's own stream: a caller-provided stream may be the legacy / null stream, which cannot be captured, and a capture
        // that fails half way would leave the CALLER's stream in capture mode)
        if (direct && e->fg.on && !e->tm.on && !e->nms_ms && st == e->own_stream) {
            // The caller-owned destinations (jsorb_extract_into) are NOT part of the key: the reference's Frame builds fresh SyncedMem members
            // every frame, so they change from frame to frame - the k_describe node of the instantiated graph gets them patched in
            // (frame_graph_set_destinations) instead of the graph being captured again.
            const void *key[6] = {e->src.l0, (const void *)(uintptr_t)e->src.l0_pitch, st, e->rect.on ? e->rect.buf : nullptr, e->cam.on ? e->cam.un : nullptr,
                                  e->up.pending ? e->up.h_upload : nullptr};      // (jsorb_set_camera drops the graph: the camera is a kernel argument)
            if (e->fg.exec && memcmp(key, e->fg.key, sizeof key) == 0) {
                e->fg.recaptures = 0;
                if (!frame_graph_set_destinations(e)) { /* fall through to a fresh capture */ }
                else {
                    HIPCHK(e, hipGraphLaunch(e->fg.exec, st));
                    HIPCHK(e, hipEventRecord(e->lanes.done[j], st));
                    if (e->up.pending && !e->up.sync_single) { HIPCHK(e, hipEventRecord(e->up.ev_read, st)); e->up.inflight = true; }
                    continue;
                }
            }
            frame_graph_drop(e);
            if (++e->fg.recaptures > 8) e->fg.on = 0;      // a caller that rotates its INPUT buffers: plain launches are cheaper than re-capturing
            if (e->fg.on) {
                memcpy(e->fg.key, key, sizeof key);
                e->fg.dst_kp = e->res.deliver_kp; e->fg.dst_desc = e->res.deliver_desc;
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
        if (e->up.pending) launch_upload_level0(e->up.h_upload, e->land.stage[0], (size_t)g.lv[0].H * g.lv[0].W, st);
        if (e->rect.on)
            JSORB_STAGE(JSORB_K_RECTIFY, launch_rectify(e->rect.map, raw.l0, raw.l0_stride, raw.l0_pitch, slab, g.slab_bytes, g.lv[0].pitch, g.lv[0].W, g.lv[0].H, m, st));
        JSORB_STAGE(JSORB_K_PYRAMID, launch_pyramid(g, src, slab, e->lut_bits, m, e->pyr_lds, st));
        const bool blur_first = !fused && K > 1 && (j & 1) && order == 1;
        const bool fuse_bc = !fused && !direct && (K > 1 || g.T <= CMP_MID_T) && !blur_first && !e->tm.on && order != 2 && blur_compact_fusable(g);
        if (blur_first) blur_first_mask |= 1u << j;
        if (fuse_bc) fuse_bc_mask |= 1u << j;
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
                                                      direct ? Deliver{e->res.deliver_kp, e->res.deliver_desc, e->res.h_kp, e->res.h_desc, nullptr}
                                                             : Deliver{nullptr, nullptr, nullptr, nullptr, nullptr}));
        if (e->cam.on)      // Frame::UndistortKeyPoints (Frame.cpp:718-748) behind the extraction, on the device counts
            JSORB_STAGE(JSORB_K_UNDISTORT, launch_undistort(e->cam.c, e->out_kp + f * T * 6, counts, (int)T, e->cam.un + f * T * 2, direct ? e->cam.h_un : nullptr, m, st));
#undef JSORB_STAGE
        if (capturing) {
            // Whatever happened between Begin and End (a launch error included), the stream must leave capture mode; on any failure the
            // partial graph is dropped, the key forgotten, graphs switched off for this handle and the frame re-issued as plain launches.
            hipGraph_t graph = nullptr;
            const hipError_t launch_err = hipGetLastError();
            const hipError_t ec = hipStreamEndCapture(st, &graph);
            hipError_t gi = ec != hipSuccess ? ec : launch_err;
            if (gi == hipSuccess) gi = hipGraphInstantiate(&e->fg.exec, graph, nullptr, nullptr, 0);
            if (gi == hipSuccess) {
                e->fg.tmpl = graph;                 // kept: its k_describe node is the handle for later parameter updates
                e->fg.describe_node = frame_graph_find_describe(graph);
                gi = hipGraphLaunch(e->fg.exec, st);
            } else if (graph) (void)hipGraphDestroy(graph);
            if (gi != hipSuccess) {
                (void)hipGetLastError();
                frame_graph_drop(e);
                e->fg.on = 0;
                j--;                                         // redo this lane without a graph
                continue;
            }
        }
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->lanes.done[j], st));
        if (e->up.pending && !e->up.sync_single) { HIPCHK(e, hipEventRecord(e->up.ev_read, st)); e->up.inflight = true; }      // (recorded behind the frame: an event record inside the captured graph is not an option on this runtime)
    }
    e->copy_kind = 0;
    camera_after_extract(e, direct);
    rgbd_invalidate(e);
    if (e->rect.on) { e->src.l0 = e->slab; e->src.l0_stride = g.slab_bytes; e->src.l0_pitch = g.lv[0].pitch; }
    e->up.pending = false;
    e->res.mirror_pending = direct;
    e->res.deliver_kp = nullptr;
    e->res.deliver_desc = nullptr;
    e->lanes.K = K;
    e->lanes.order = order; e->lanes.fuse_bc_mask = fuse_bc_mask; e->lanes.blur_first_mask = blur_first_mask;
    for (int j = 0; j <= K; j++) e->lanes.first[j] = first[j];
    for (int j = 0; j < K; j++) e->lanes.used[j] = ls[j];
    // a caller-provided main stream observes the batch: whatever the caller enqueues on it next runs after the lanes
    if (K > 1 && e->stream != e->own_stream) RCCHK(wait_lanes(e, e->stream, e));
    e->n_images = n;
    e->extracted = true;
    stereo_after_extract(e);
    bow_after_extract(e);
    e->counts_synced = false;
    return JSORB_OK;
}

// Copies into the level-0 plane of the internal slab are enqueued on the main stream BEFORE the lanes of the new batch are ordered:
// the main stream first has to wait for whoever may still read the slab (other lanes of the previous batch, a stereo match).
int join_previous_on_main(jsorb_extractor *e)
{
    if (e->extracted) RCCHK(wait_lanes(e, e->stream, e));
    if (e->lanes.has_readers) RCCHK(wait_events(e, e->stream, e->lanes.readers_stream, e->lanes.readers_done, e->lanes.readers_K));
    return JSORB_OK;
}

// A landing buffer may be refilled only after every lane that read it in place (extract kernels and, if any, the stereo match)
int wait_buffer_consumed(jsorb_extractor *e, int k, hipStream_t s)
{
    for (int j = 0; j < e->land.consumed_K[k]; j++) HIPCHK(e, hipStreamWaitEvent(s, e->land.ev_consumed[k][j], 0));
    return JSORB_OK;
}
int mark_buffer_consumed(jsorb_extractor *e, int k)
{
    for (int j = 0; j < e->lanes.K; j++) HIPCHK(e, hipEventRecord(e->land.ev_consumed[k][j], lane_stream(e, j)));
    e->land.consumed_K[k] = e->lanes.K;
    e->land.consumed_n[k] = e->n_images;
    e->land.last = k;
    return JSORB_OK;
}

// *mark: the landing buffer whose "consumed" events the caller records after everything else it enqueues for this call (-1: none)
int extract_batch_host_enqueue(jsorb_extractor *e, const uint8_t *host_images, size_t image_stride, int step, int n_images, int *mark)
{
    *mark = -1;
    const LevelDesc &l0 = e->g.lv[0];
    const size_t img_bytes = (size_t)l0.H * l0.W;
    int rc;
    if (e->land.stage[0] && step == l0.W && n_images == 1) {
        // single frame (the reference-shaped call): lowest latency - upload on the compute stream itself, no cross-stream hops.
        // The buffer may still be read by an earlier batch on other lanes / by a stereo match on the other handle's stream.
        RCCHK(wait_buffer_consumed(e, 0, e->stream));
        RCCHK(join_previous_on_main(e));
        const double t0 = e->trace.on ? now_us() : 0.0;
        if (e->up.kernel) {
            RCCHK(reserve_pinned(e, e->up.h_upload, img_bytes));
            if (!e->up.ev_read) HIPCHK(e, hipEventCreateWithFlags(&e->up.ev_read, hipEventDisableTiming));
            // the previous frame's upload kernel must have read the pinned buffer before it is rewritten: its own event (asynchronous
            // callers that have not waited for that frame yet wait here; a batch enqueued in between does not change what has to be waited for)
            if (e->up.inflight) RCCHK(wait_event(e, e->up.ev_read, e->spin_wait != 0));
            e->up.inflight = false;
            memcpy(e->up.h_upload, host_images, img_bytes);
            e->up.pending = true;
        } else {
            HIPCHK(e, hipMemcpyAsync(e->land.stage[0], host_images, img_bytes, hipMemcpyHostToDevice, e->stream));
        }
        const double t1 = e->trace.on ? now_us() : 0.0;
        e->src.l0 = e->land.stage[0]; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
        RCCHK(run_pipeline(e, n_images));
        if (e->trace.on) { e->trace.h2d += t1 - t0; e->trace.enq += now_us() - t1; e->trace.n++; }
        e->land.cur = 1;       // a following batch call starts on the other buffer
        *mark = 0;
        return JSORB_OK;
    }
    if (e->land.stage[0] && step == l0.W && image_stride == img_bytes) {
        // dense batch: pinned hipMemcpyAsync on the device's upload stream into a landing buffer, then level 0 is read in place from
        // there.  The buffer being refilled was last read two batches ago (its extract kernels and, if any, the stereo match), so the
        // upload of batch k+1 runs under the kernels of batch k.  With more than one lane (JSORB_HOST_LANES) the upload is cut at the
        // lane boundaries: lane j starts as soon as ITS images have landed and its part of the buffer is refilled as soon as lane j of
        // the batch that used it has finished.
        // One lane: the regime is PCIe-bound (a pair is 722 kB; 57 GB/s = 79 k pairs/s against 85 k for the kernels on one lane), so the
        // kernels do not need the overlap of several lanes, and one upload per handle and batch runs at the full rate of the link where
        // lane-sized chunks reach 49-51 GB/s with 18-24 us between them (measured at 64 / 128 / 256 pairs per batch on 16 hardware
        // queues: 1 lane 60.6 / 70.2 / 73.1 k, 2 lanes 55.5 / 62.4 / 69.9 k, 4 lanes 48 / 58 k pairs/s).  JSORB_HOST_LANES raises the cap.
        const int k = e->land.cur;
        int first[JSORB_MAX_LANES + 1];
        e->lanes.cap = e->land.host_lanes;
        const int K = plan_lanes(e, n_images, first);
        hipStream_t cs = nullptr;
        if ((rc = pool_copy_stream(e, &cs))) { e->lanes.cap = JSORB_MAX_LANES; return rc; }
        const bool same_split = e->land.consumed_K[k] == K && e->land.consumed_n[k] == n_images;
        if (!same_split && (rc = wait_buffer_consumed(e, k, cs))) { e->lanes.cap = JSORB_MAX_LANES; return rc; }
        for (int j = 0; j < K; j++) {
            if (same_split) HIPCHK(e, hipStreamWaitEvent(cs, e->land.ev_consumed[k][j], 0));
            HIPCHK(e, hipMemcpyAsync(e->land.stage[k] + (size_t)first[j] * img_bytes, host_images + (size_t)first[j] * img_bytes,
                                     img_bytes * (size_t)(first[j + 1] - first[j]), hipMemcpyHostToDevice, cs));
            HIPCHK(e, hipEventRecord(e->land.ev_copied[k][j], cs));
        }
        e->src.l0 = e->land.stage[k]; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
        rc = run_pipeline(e, n_images, e->land.ev_copied[k]);
        e->lanes.cap = JSORB_MAX_LANES;
        if (rc) return rc;
        e->land.cur = k ^ 1;
        *mark = k;
        return JSORB_OK;
    }
    // strided input: one 2-D copy per image into the pitched slab, enqueued by run_pipeline on the stream of the lane that owns the image
    // (with maps: into the dense raw buffer that k_rectify reads)
    e->copy_src = host_images; e->copy_stride = image_stride; e->copy_step = step; e->copy_kind = 1;
    e->src.l0 = e->slab; e->src.l0_stride = e->g.slab_bytes; e->src.l0_pitch = l0.pitch;
    if (e->rect.on) {
        RCCHK(rectify_reserve_raw(e, img_bytes));
        e->src.l0 = e->rect.raw; e->src.l0_stride = img_bytes; e->src.l0_pitch = l0.W;
    }
    e->land.last = -1;
    return run_pipeline(e, n_images);
}

int extract_batch_device_enqueue(jsorb_extractor *e, const uint8_t *dev_images, size_t image_stride, int step, int n_images)
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
    const bool in_place = aligned16 || !copy_unaligned || e->rect.on;      // (k_rectify reads any alignment)
    if (in_place) {   // no copy of the grayscale plane
        e->src.l0 = dev_images; e->src.l0_stride = image_stride; e->src.l0_pitch = step;
    } else {
        // rows that are not 16-byte aligned: one copy kernel per lane brings level 0 into the pitched slab (run_pipeline, lane stream)
        e->copy_src = dev_images; e->copy_stride = image_stride; e->copy_step = step; e->copy_kind = 2;
        e->src.l0 = e->slab; e->src.l0_stride = e->g.slab_bytes; e->src.l0_pitch = l0.pitch;
    }
    e->land.last = -1;
    return run_pipeline(e, n_images);
}

// What both batch entry points do first: check the arguments, drop the mirrors of the previous call, select the device, order the new extract
// after a speculative match that still reads the handle's buffers, reset the lane cap.
int extract_begin(jsorb_extractor *e, const uint8_t *images, int step, int n_images)
{
    if (!e || !images || n_images < 1 || n_images > e->B || step < e->g.lv[0].W) return JSORB_ERR_INVALID;
    e->res.mirror_valid = e->st.mirror_valid = false;
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(spec_guard(e, n_images));
    e->lanes.cap = JSORB_MAX_LANES;
    return JSORB_OK;
}

// Tail of the synchronous single-frame calls: ONE wait - counts, keypoints and descriptors were written into the pinned mirrors (and
// the caller's device buffers) by the kernels themselves.  The wait is for the event behind the extract kernels, not for the stream:
// the other extractor's thread may already have put this frame's speculative stereo match on it (struct jsorb_spec_state).
int finish_single_frame(jsorb_extractor *e, int *n_keypoints)
{
    const double t0 = e->trace.on ? now_us() : 0.0;
    int rc;
    if (e->tm.on || e->lanes.K != 1) rc = jsorb_sync(e);
    else if (!(rc = wait_event(e, e->lanes.done[0], e->spin_wait != 0))) {
        e->counts_synced = true;
        mirrors_landed(e);
    }
    if (e->trace.on) e->trace.wait += now_us() - t0;
    if (rc) return rc;
    if (n_keypoints) *n_keypoints = e->h_counts[JSORB_MAX_LEVELS];
    return JSORB_OK;
}

// ---- Frame-side unpacking: keypoints as AoS (keys), optionally with mvKeysUn (keys_un: the same keypoints at x_un / y_un), descriptors ----
int unpack_frame(jsorb_extractor *e, int image, jsorb_keypoint *keys, jsorb_keypoint *keys_un, uint8_t *descriptors)
{
    if (!check_image(e, image)) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    const bool un = keys_un && e->cam.un_valid;          // keys_un differs from keys only with a camera
    jsorb_keypoint *out = keys_un ? keys_un : keys;      // the keypoints are unpacked once, into keys_un when it is asked for
    if (e->res.mirror_valid && image == 0 && (!un || e->cam.un_mirror)) {
        // after a synchronous single-frame extract the SoA (and x_un / y_un) already sits in pinned host memory: interleave it here (the
        // reference's own host loop, Frame.cpp:139-147, 741-747) instead of a kernel + copies + a synchronisation
        if (out) {
            const int32_t *s = e->res.h_kp;
            for (int i = 0; i < n; i++) {
                jsorb_keypoint &k = out[i];
                k.x = (float)s[i]; k.y = (float)s[n + i]; k.response = (float)s[2 * (size_t)n + i];
                memcpy(&k.angle, &s[3 * (size_t)n + i], 4);
                k.octave = s[4 * (size_t)n + i]; k.size = (float)s[5 * (size_t)n + i]; k.class_id = -1;
            }
        }
        if (descriptors) memcpy(descriptors, e->res.h_desc, (size_t)n * 32);
        if (keys_un && keys) memcpy(keys, keys_un, (size_t)n * sizeof(jsorb_keypoint));
        if (un)
            for (int i = 0; i < n; i++) { keys_un[i].x = e->cam.h_un[i]; keys_un[i].y = e->cam.h_un[n + i]; }
        return JSORB_OK;
    }
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<float> xy(un ? (size_t)2 * n : 0);
    mark_main_stream(e);
    if (out) {
        RCCHK(reserve_device(e, e->res.frame_aos, (size_t)e->g.T * sizeof(jsorb_keypoint)));
        launch_unpack_keypoints(jsorb_keypoints_device(e, image), n, e->res.frame_aos, e->stream);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipMemcpyAsync(out, e->res.frame_aos, (size_t)n * sizeof(jsorb_keypoint), hipMemcpyDeviceToHost, e->stream));
        if (keys_un && keys) HIPCHK(e, hipMemcpyAsync(keys, e->res.frame_aos, (size_t)n * sizeof(jsorb_keypoint), hipMemcpyDeviceToHost, e->stream));
    }
    if (un) HIPCHK(e, hipMemcpyAsync(xy.data(), jsorb_keypoints_un_device(e, image), (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (descriptors) HIPCHK(e, hipMemcpyAsync(descriptors, jsorb_descriptors_device(e, image), (size_t)n * 32, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (un)
        for (int i = 0; i < n; i++) { keys_un[i].x = xy[i]; keys_un[i].y = xy[n + i]; }
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_extract_batch_host_async(jsorb_extractor *e, const uint8_t *host_images, size_t image_stride, int step, int n_images)
{
    RCCHK(extract_begin(e, host_images, step, n_images));
    int mark;
    RCCHK(extract_batch_host_enqueue(e, host_images, image_stride, step, n_images, &mark));
    // the speculative match goes out first: every packet between the extract kernels and k_stereo (an event record is a barrier
    // packet, ~5 us on the GPU's command processor) delays the match
    spec_after_extract(e, n_images);
    return mark >= 0 ? mark_buffer_consumed(e, mark) : JSORB_OK;
}

int jsorb_extract_batch_device_async(jsorb_extractor *e, const uint8_t *dev_images, size_t image_stride, int step, int n_images)
{
    RCCHK(extract_begin(e, dev_images, step, n_images));
    RCCHK(extract_batch_device_enqueue(e, dev_images, image_stride, step, n_images));
    spec_after_extract(e, n_images);
    return JSORB_OK;
}

int jsorb_extract(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints) { return jsorb_extract_into(e, host_image, step, n_keypoints, nullptr, nullptr); }

// The synchronous single-image calls wait for the frame themselves, so nobody needs up.ev_read (one barrier packet less in front of the
// match) - `up.sync_single` tells run_pipeline so.  The flag and the caller's destinations are reset on every way out (scope guard), and a call
// that fails AFTER the frame was enqueued (mark_buffer_consumed / finish_single_frame) waits for the stream before it returns: the next call
// memcpys into the pinned upload buffer without an event to wait for, and k_upload_level0 of the failed frame may still be reading it (round-4 review).
int jsorb_extract_into(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints, int32_t *dev_keypoints_dst, uint8_t *dev_descriptors_dst)
{
    if (!e) return JSORB_ERR_INVALID;
    struct Reset { jsorb_extractor *e; ~Reset() { e->up.sync_single = false; e->res.deliver_kp = nullptr; e->res.deliver_desc = nullptr; } } reset{e};
    e->res.deliver_kp = dev_keypoints_dst;
    e->res.deliver_desc = dev_descriptors_dst;
    e->up.sync_single = true;
    int rc = jsorb_extract_batch_host_async(e, host_image, 0, step, 1);
    if (!rc) rc = finish_single_frame(e, n_keypoints);
    if (rc && e->stream) (void)hipStreamSynchronize(e->stream);
    return rc;
}

int jsorb_extract_device(jsorb_extractor *e, const uint8_t *dev_image, int step, int *n_keypoints)
{
    RCCHK(jsorb_extract_batch_device_async(e, dev_image, 0, step, 1));
    return finish_single_frame(e, n_keypoints);
}

int jsorb_n_images(const jsorb_extractor *e) { return e ? e->n_images : 0; }
int jsorb_n_keypoints(const jsorb_extractor *e, int image) { return check_image(e, image) ? e->h_counts[image * (JSORB_MAX_LEVELS + 1) + JSORB_MAX_LEVELS] : JSORB_ERR_STATE; }
int jsorb_level_n_keypoints(const jsorb_extractor *e, int image, int level)
{
    if (!check_image(e, image) || level < 0 || level >= e->g.L) return JSORB_ERR_STATE;
    return e->h_counts[image * (JSORB_MAX_LEVELS + 1) + level];
}
const int32_t *jsorb_keypoints_device(const jsorb_extractor *e, int image) { return check_image(e, image) ? e->out_kp + (size_t)image * 6 * e->g.T : nullptr; }
const uint8_t *jsorb_descriptors_device(const jsorb_extractor *e, int image) { return check_image(e, image) ? e->desc + (size_t)image * 32 * e->g.T : nullptr; }
int jsorb_copy_keypoints(const jsorb_extractor *e, int image, int32_t *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    return copy_result(dst, e->res.mirror_valid && image == 0 ? e->res.h_kp : nullptr, jsorb_keypoints_device(e, image), jsorb_n_keypoints(e, image), 6 * 4);
}
int jsorb_copy_descriptors(const jsorb_extractor *e, int image, uint8_t *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    return copy_result(dst, e->res.mirror_valid && image == 0 ? e->res.h_desc : nullptr, jsorb_descriptors_device(e, image), jsorb_n_keypoints(e, image), 32);
}
int jsorb_copy_angles(const jsorb_extractor *e, int image, float *dst)
{
    if (!check_image(e, image) || !dst) return JSORB_ERR_STATE;
    return copy_result(dst, nullptr, e->angles + (size_t)image * e->g.T, jsorb_n_keypoints(e, image), 4);
}

int jsorb_unpack_frame(jsorb_extractor *e, int image, jsorb_keypoint *keypoints, uint8_t *descriptors) { return unpack_frame(e, image, keypoints, nullptr, descriptors); }
int jsorb_unpack_frame_un(jsorb_extractor *e, int image, jsorb_keypoint *keys, jsorb_keypoint *keys_un, uint8_t *descriptors) { return unpack_frame(e, image, keys, keys_un, descriptors); }

} // extern "C"
