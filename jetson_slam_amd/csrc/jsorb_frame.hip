// jsorb_frame.hip - host side of the Frame- and Tracking-side features around an extract: rectification maps, the camera (undistorted
// keypoints, image bounds), RGB-D depth, the feature grid, local-map search, motion-model search, monocular-initialisation search and keyframe-projection search.  Each feature keeps its state in its own part of the handle
// (jsorb_handle.h); run_pipeline and jsorb_destroy reach it through the *_after_extract / *_release functions here.
#include "jsorb_handle.h"

namespace jsorb_host __attribute__((visibility("hidden"))) {

// ---- rectification maps (Examples/Stereo/stereo_euroc.cpp:106-107, 145-146) ----
// strided host input with maps: the raw images land in a dense B x H x W buffer that k_rectify reads (run_pipeline copies them there)
int rectify_reserve_raw(jsorb_extractor *e, size_t image_bytes) { return reserve_device(e, e->rect.raw, (size_t)e->B * image_bytes + 256); }
void rectify_release(jsorb_extractor *e) { free_device(e->rect.buf, e->rect.raw); }

// ---- camera ----
// an extract leaves `un` undistorted with the current camera (k_undistort ran behind every lane); a single image also wrote h_un
void camera_after_extract(jsorb_extractor *e, bool direct) { e->cam.un_valid = e->cam.on; e->cam.un_mirror = direct && e->cam.on; }
void camera_release(jsorb_extractor *e) { free_device(e->cam.un); free_pinned(e->cam.h_un); }

// ---- RGB-D: results exist only for the images the last call computed, with the keypoints (and mvKeysUn) it read ----
void rgbd_invalidate(jsorb_extractor *e) { e->rgbd.images = 0; e->rgbd.mirror = false; }
void rgbd_release(jsorb_extractor *e) { free_device(e->rgbd.out); free_pinned(e->rgbd.h_out, e->rgbd.h_depth); }

void grid_release(jsorb_extractor *e) { free_device(e->grid.start, e->grid.items); }
void search_local_release(jsorb_extractor *e) { free_device(e->sl.cand, e->sl.stats, e->sl.out); }
void search_last_release(jsorb_extractor *e) { free_device(e->lf.ws, e->lf.pts, e->lf.out); }
void search_init_release(jsorb_extractor *e) { free_device(e->si.cand, e->si.ws, e->si.out, e->si.ref); }
void search_kf_release(jsorb_extractor *e) { free_device(e->kf.cand, e->kf.stats, e->kf.out); }

} // namespace jsorb_host

namespace {

// The map's entries at pitch round_up(W, 4) (one 16-byte + one 8-byte load per lane of k_rectify), entries beyond W point outside the source, then
// the per-tile source boxes.  The handle's work in flight is waited for first: its k_rectify launches read the buffer that is overwritten.
int rectify_upload(jsorb_extractor *e, const int16_t *xy, const uint16_t *a, int xy_step, int a_step)
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
    RCCHK(jsorb_sync(e));
    RCCHK(reserve_device(e, e->rect.buf, xy_bytes + a_bytes + t_bytes));
    uint8_t *base = static_cast<uint8_t *>(e->rect.buf);
    HIPCHK(e, hipMemcpy(base, hxy.data(), xy_bytes, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(base + xy_bytes, ha.data(), (size_t)2 * MP * H, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(base + xy_bytes + a_bytes, tiles.data(), t_bytes, hipMemcpyHostToDevice));
    e->rect.map = RectMap{reinterpret_cast<const int *>(base), reinterpret_cast<const uint16_t *>(base + xy_bytes), reinterpret_cast<const int4 *>(base + xy_bytes + a_bytes),
                          MP, ntx, nty};
    e->rect.on = true;
    frame_graph_drop(e);        // the single-frame graph starts with k_rectify now: captured again on the next frame
    return JSORB_OK;
}

// ---- camera: Frame::UndistortKeyPoints / ComputeImageBounds (Frame.cpp:718-778) ----
UndistortCam to_cam(const jsorb_camera &c) { return UndistortCam{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3}; }

// ---- RGB-D: Frame::ComputeStereoFromRGBD (Frame.cpp:996-1017) + Tracking.cpp:333-334 ----
int rgbd_check(jsorb_extractor *e, const void *depth, int format, size_t step_bytes, size_t image_stride, int n_images)
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
    RCCHK(reserve_device(e, e->rgbd.out, (size_t)e->B * 2 * T * sizeof(float)));
    return reserve_pinned(e, e->rgbd.h_out, 2 * T * sizeof(float));
}

RgbdArgs rgbd_args(int format, float factor, float mbf)
{
    // Tracking.cpp:333: if ((fabs(mDepthMapFactor - 1.0f) > 1e-5) || imDepth.type() != CV_32F) imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)
    const bool scale = format == JSORB_DEPTH_U16 || std::fabs(factor - 1.0f) > 1e-5;
    return RgbdArgs{format, scale ? 1 : 0, factor, mbf};
}

// The grid CSR for `n_cells` cells (grown on demand) and one item per keypoint slot of the handle.
int grid_reserve(jsorb_extractor *e, int n_cells)
{
    RCCHK(reserve_device(e, e->grid.start, (size_t)(n_cells + 1) * sizeof(int32_t), &e->grid.cells, n_cells));
    return reserve_device(e, e->grid.items, (size_t)e->g.T * sizeof(int32_t));
}

} // namespace

extern "C" {

int jsorb_rectify_convert_maps(const float *mapx, const float *mapy, int n, int16_t *xy, uint16_t *a)
{
    if (!mapx || !mapy || !xy || !a || n < 0) return JSORB_ERR_INVALID;
    rectify_convert_maps(mapx, mapy, (size_t)n, xy, a);
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
    if (!e->rect.on) return JSORB_OK;
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(jsorb_sync(e));
    e->rect.on = false;
    frame_graph_drop(e);
    return JSORB_OK;
}

int jsorb_rectify_enabled(const jsorb_extractor *e) { return e ? (e->rect.on ? 1 : 0) : JSORB_ERR_INVALID; }

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
    if (!on && !e->cam.on) return JSORB_OK;          // nothing to undo, nothing to allocate
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(jsorb_sync(e));
    frame_graph_drop(e);          // the single-frame graph carries the camera as a kernel argument (or lacks k_undistort): captured again
    e->cam.un_valid = false;
    e->cam.un_mirror = false;
    rgbd_invalidate(e);           // its uRight used the old mvKeysUn
    e->cam.on = on;
    if (!on) return JSORB_OK;
    e->cam.c = to_cam(*camera);
    const size_t T = (size_t)e->g.T;
    RCCHK(reserve_device(e, e->cam.un, (size_t)e->B * 2 * T * sizeof(float)));
    RCCHK(reserve_pinned(e, e->cam.h_un, 2 * T * sizeof(float)));
    if (e->extracted && e->n_images > 0) {      // the results already there are undistorted with the new camera (device copy only)
        mark_main_stream(e);
        launch_undistort(e->cam.c, e->out_kp, e->counts, (int)T, e->cam.un, nullptr, e->n_images, e->stream);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipStreamSynchronize(e->stream));
        e->cam.un_valid = true;
    }
    return JSORB_OK;
}

int jsorb_camera_enabled(const jsorb_extractor *e) { return e ? (e->cam.on ? 1 : 0) : JSORB_ERR_INVALID; }

const float *jsorb_keypoints_un_device(const jsorb_extractor *e, int image) { return (check_image(e, image) && e->cam.un_valid) ? e->cam.un + (size_t)image * 2 * e->g.T : nullptr; }

int jsorb_copy_keypoints_un(const jsorb_extractor *e, int image, float *xy)
{
    if (!check_image(e, image) || !xy) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    if (n <= 0) return JSORB_OK;
    if (!e->cam.un_valid) {           // mvKeysUn = mvKeys: the keypoint coordinates as floats
        std::vector<int32_t> kp((size_t)6 * n);
        RCCHK(jsorb_copy_keypoints(e, image, kp.data()));
        for (size_t i = 0; i < (size_t)2 * n; i++) xy[i] = (float)kp[i];
        return JSORB_OK;
    }
    return copy_result(xy, e->res.mirror_valid && e->cam.un_mirror && image == 0 ? e->cam.h_un : nullptr, jsorb_keypoints_un_device(e, image), n, 2 * sizeof(float));
}

int jsorb_rgbd_depth_batch_device_async(jsorb_extractor *e, const void *dev_depths, size_t image_stride, size_t step_bytes, int format, float factor,
                                        float mbf, int n_images)
{
    if (!e) return JSORB_ERR_INVALID;
    if (n_images != e->n_images) { e->err = "RGB-D batch: n_images must be the last batch's"; return JSORB_ERR_INVALID; }
    RCCHK(rgbd_check(e, dev_depths, format, step_bytes, image_stride, n_images));
    const size_t T = (size_t)e->g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    const RgbdArgs a = rgbd_args(format, factor, mbf);
    // the depth images may come from work the caller enqueued on the main stream after the extract call (e.g. torch's current stream through
    // jsorb_set_stream): every lane that is not the main stream starts after a fork event recorded there
    RCCHK(fork_lanes(e, e->stream, {e}));
    for (int j = 0; j < e->lanes.K; j++) {        // lane j samples its own images, behind its extraction (and k_undistort) on its stream
        hipStream_t st = lane_stream(e, j);
        const int f = e->lanes.first[j], m = e->lanes.first[j + 1] - f;
        TIMED(e, JSORB_K_RGBD, launch_rgbd(e->out_kp + f * T * 6, e->counts + f * CW, (int)T, e->cam.un_valid ? e->cam.un + f * T * 2 : nullptr,
                                           static_cast<const uint8_t *>(dev_depths) + (size_t)f * image_stride, image_stride, step_bytes, e->g.lv[0].W,
                                           e->g.lv[0].H, a, e->rgbd.out + f * T, e->rgbd.out + (size_t)e->B * T + f * T, nullptr, nullptr, m, st));
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->lanes.done[j], st));
    }
    // ... and whatever the caller enqueues on its main stream next (reading jsorb_rgbd_uright_device, say) runs after every lane, as behind an extract
    if (e->stream != e->own_stream) RCCHK(wait_lanes(e, e->stream, e));
    e->rgbd.images = n_images;
    e->rgbd.mirror = false;
    e->counts_synced = false;
    return JSORB_OK;
}

int jsorb_rgbd_depth(jsorb_extractor *e, const void *host_depth, int format, size_t step_bytes, float factor, float mbf, float *u_right, float *depth)
{
    if (!e) return JSORB_ERR_INVALID;
    RCCHK(rgbd_check(e, host_depth, format, step_bytes, 0, 1));
    if (e->n_images < 1) return JSORB_ERR_STATE;
    const int W = e->g.lv[0].W, H = e->g.lv[0].H;
    const size_t bpp = format == JSORB_DEPTH_U16 ? 2 : 4, row = (size_t)W * bpp, T = (size_t)e->g.T;
    RCCHK(reserve_pinned(e, e->rgbd.h_depth, (size_t)H * W * 4));
    // the host image reaches the device the way a single host image does: copied into a pinned buffer of the handle by the calling thread,
    // then read in place over PCIe by the kernel - which reads only the N sampled pixels
    const uint8_t *src = static_cast<const uint8_t *>(host_depth);
    if (step_bytes == row) memcpy(e->rgbd.h_depth, src, row * H);
    else
        for (int y = 0; y < H; y++) memcpy(e->rgbd.h_depth + row * y, src + step_bytes * y, row);
    hipStream_t st = lane_stream(e, 0);
    if (e->lanes.K != 1 || !st) st = e->stream;
    RCCHK(wait_lanes(e, st, e));
    TIMED(e, JSORB_K_RGBD, launch_rgbd(e->out_kp, e->counts, (int)T, e->cam.un_valid ? e->cam.un : nullptr, e->rgbd.h_depth, 0, row, W, H, rgbd_args(format, factor, mbf),
                                       e->rgbd.out, e->rgbd.out + (size_t)e->B * T, e->rgbd.h_out, e->rgbd.h_out + T, 1, st));
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->lanes.done[0], st));
    if (st != lane_stream(e, 0)) for (int j = 1; j < e->lanes.K; j++) HIPCHK(e, hipEventRecord(e->lanes.done[j], st));
    RCCHK(e->tm.on || e->lanes.K != 1 ? jsorb_sync(e) : wait_event(e, e->lanes.done[0], e->spin_wait != 0));
    e->rgbd.images = 1;           // image 0 only
    e->rgbd.mirror = true;
    const int n = e->h_counts[JSORB_MAX_LEVELS];
    if (u_right && n > 0) memcpy(u_right, e->rgbd.h_out, (size_t)n * sizeof(float));
    if (depth && n > 0) memcpy(depth, e->rgbd.h_out + T, (size_t)n * sizeof(float));
    return JSORB_OK;
}

const float *jsorb_rgbd_uright_device(const jsorb_extractor *e, int image) { return (check_image(e, image) && image < e->rgbd.images) ? e->rgbd.out + (size_t)image * e->g.T : nullptr; }
const float *jsorb_rgbd_depth_device(const jsorb_extractor *e, int image)
{
    return (check_image(e, image) && image < e->rgbd.images) ? e->rgbd.out + (size_t)e->B * e->g.T + (size_t)image * e->g.T : nullptr;
}
int jsorb_copy_rgbd(const jsorb_extractor *e, int image, float *u_right, float *depth)
{
    if (!check_image(e, image) || image >= e->rgbd.images) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(e, image);
    const bool mirror = e->rgbd.mirror && image == 0;
    RCCHK(copy_result(u_right, mirror ? e->rgbd.h_out : nullptr, jsorb_rgbd_uright_device(e, image), n, sizeof(float)));
    return copy_result(depth, mirror ? e->rgbd.h_out + e->g.T : nullptr, jsorb_rgbd_depth_device(e, image), n, sizeof(float));
}

int jsorb_assign_features_to_grid(jsorb_extractor *e, int image, float min_x, float min_y, float grid_element_width_inv,
                                  float grid_element_height_inv, int cols, int rows, int32_t *cell_start, int32_t *cell_items)
{
    if (!check_image(e, image) || !cell_start || !cell_items) return JSORB_ERR_STATE;
    if (cols < 1 || rows < 1 || (long long)cols * rows > 16384) { e->err = "grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image), n_cells = cols * rows;
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(grid_reserve(e, n_cells));
    mark_main_stream(e);
    launch_assign_grid(jsorb_keypoints_device(e, image), jsorb_keypoints_un_device(e, image), n, min_x, min_y, grid_element_width_inv, grid_element_height_inv, cols, rows,
                       e->grid.start, e->grid.items, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(cell_start, e->grid.start, (size_t)(n_cells + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const int in_grid = cell_start[n_cells];
    if (in_grid > 0) HIPCHK(e, hipMemcpy(cell_items, e->grid.items, (size_t)in_grid * sizeof(int32_t), hipMemcpyDeviceToHost));
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
    RCCHK(grid_reserve(e, n_cells));
    RCCHK(reserve_device(e, e->sl.cand, (size_t)n_points * (cap + 1) * sizeof(int), &e->sl.points, n_points));
    RCCHK(reserve_device(e, e->sl.stats, 4 * sizeof(int)));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the frame (and its uRight) may come from the lanes of a batch
    mark_main_stream(e);               // ... and the next batch's lanes must not rewrite it before these kernels have read it
    const float *xy_un = jsorb_keypoints_un_device(e, image);
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(jsorb_keypoints_device(e, image), xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows,
                                                     e->grid.start, e->grid.items, st));
    HIPCHK(e, hipGetLastError());
    SearchLocalArgs a{};
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = xy_un;
    a.desc = jsorb_descriptors_device(e, image);
    a.u_right = u_right;
    a.blocked = blocked_in;
    a.n_kp = n;
    a.cell_start = e->grid.start;
    a.cell_items = e->grid.items;
    a.min_x = p.min_x; a.min_y = p.min_y; a.inv_w = p.inv_w; a.inv_h = p.inv_h;
    a.cols = p.cols; a.rows = p.rows;
    a.n_points = n_points;
    a.u = u; a.v = v; a.invz = invz; a.view_cos = view_cos; a.level = predicted_level; a.in_frustum = in_frustum; a.mp_desc = mp_descriptors;
    a.th = p.th; a.nn_ratio = p.nn_ratio; a.mbf = p.mbf; a.th_high = p.th_high;
    a.n_levels = e->g.L;
    for (int l = 0; l < e->g.L; l++) a.scale[l] = e->g.lv[l].scale;
    a.cand = e->sl.cand;
    a.cand_n = e->sl.cand + (size_t)e->sl.points * cap;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    a.stats = e->sl.stats;
    TIMED(e, JSORB_K_LOCAL_CANDIDATES, launch_local_candidates(a, st));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_LOCAL_RESOLVE, launch_local_resolve(a, st));
    HIPCHK(e, hipGetLastError());
    e->sl.done = true;
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
    if (!e->sl.done) { e->err = "search_local_stats before jsorb_search_local_points"; return JSORB_ERR_STATE; }
    int32_t s[4] = {0, 0, 0, 0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(s, e->sl.stats, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (rounds) *rounds = s[0];
    if (n_candidates) *n_candidates = s[1];
    if (n_overflow) *n_overflow = s[2];
    return JSORB_OK;
}

// ---- motion-model matching: ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cpp:1647-1963), k_search_last.hip ----
#define LF_CTL 8                   // control and statistics words behind the owner array: run the second pass, passes, candidates, ind1..3
int jsorb_search_last_frame_async(jsorb_extractor *e, int image, const jsorb_last_frame_params *params, int n_points, const float *Px, const float *Py,
                                  const float *Pz, const int32_t *last_octave, const float *last_angle, const uint8_t *mp_descriptors,
                                  const float *u_right, int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) { e->err = "search_last_frame: no extract result for this image"; return JSORB_ERR_STATE; }
    if (!params || !n_matches_dev) { e->err = "search_last_frame: NULL params or n_matches"; return JSORB_ERR_INVALID; }
    const jsorb_last_frame_params &p = *params;
    if (p.cols < 1 || p.rows < 1 || (long long)p.cols * p.rows > 16384) { e->err = "search_last_frame: grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    if (p.direction < -1 || p.direction > 1) { e->err = "search_last_frame: direction must be -1, 0 or 1"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_last_frame: n_points < 0"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image);
    if (n >= (1 << 18)) { e->err = "search_last_frame: more than 262143 keypoints"; return JSORB_ERR_UNSUPPORTED; }
    if (n_points > 0 && (!Px || !Py || !Pz || !last_octave || !last_angle || !mp_descriptors || !match_kp || !match_dist)) {
        e->err = "search_last_frame: NULL point array or output";
        return JSORB_ERR_INVALID;
    }
    if (n > 0 && !kp_match) { e->err = "search_last_frame: NULL kp_match"; return JSORB_ERR_INVALID; }
    if ((uintptr_t)mp_descriptors % 16) { e->err = "search_last_frame: mp_descriptors must be 16-byte aligned"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    RCCHK(grid_reserve(e, p.cols * p.rows));
    if (!e->lf.ws) {                   // owner starts at -1; afterwards every k_last_resolve leaves it so
        RCCHK(reserve_device(e, e->lf.ws, ((size_t)e->g.T + LF_CTL) * sizeof(int)));
        HIPCHK(e, hipMemsetAsync(e->lf.ws, 0xff, ((size_t)e->g.T + LF_CTL) * sizeof(int), st));
    }
    RCCHK(reserve_device(e, e->lf.pts, (size_t)2 * std::max(n_points, 1) * sizeof(int), &e->lf.points, std::max(n_points, 1)));
    RCCHK(wait_lanes(e, st, e));       // the frame (and its uRight) may come from the lanes of a batch
    mark_main_stream(e);               // ... and the next batch's lanes must not rewrite it before these kernels have read it
    const float *xy_un = jsorb_keypoints_un_device(e, image);
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(jsorb_keypoints_device(e, image), xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows,
                                                     e->grid.start, e->grid.items, st));
    HIPCHK(e, hipGetLastError());
    LastFrameArgs a{};
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = xy_un;
    a.desc = jsorb_descriptors_device(e, image);
    a.u_right = u_right;
    a.n_kp = n;
    a.cell_start = e->grid.start;
    a.cell_items = e->grid.items;
    a.n_points = n_points;
    a.Px = Px; a.Py = Py; a.Pz = Pz; a.angle = last_angle; a.octave = last_octave; a.mp_desc = mp_descriptors;
    a.p = p;
    a.n_levels = e->g.L;
    for (int l = 0; l < e->g.L; l++) a.scale[l] = e->g.lv[l].scale;
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
    if (!n_matches) { e->err = "search_last_frame: NULL n_matches"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_last_frame: n_points < 0"; return JSORB_ERR_INVALID; }
    if (!check_image(e, image)) { e->err = "search_last_frame: no extract result for this image"; return JSORB_ERR_STATE; }
    const int N = jsorb_n_keypoints(e, image);
    if (N > 0 && !kp_match_host) { e->err = "search_last_frame: NULL host output"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int pts = std::max(n_points, 1);
    RCCHK(reserve_device(e, e->lf.out, ((size_t)2 * pts + e->g.T + 1) * sizeof(int32_t), &e->lf.out_points, pts));
    int32_t *cnt = e->lf.out, *km = cnt + 1, *mk = km + e->g.T, *md = mk + e->lf.out_points;
    RCCHK(jsorb_search_last_frame_async(e, image, params, n_points, Px, Py, Pz, last_octave, last_angle, mp_descriptors, u_right, mk, md, km, cnt));
    std::vector<int32_t> h((size_t)N + 1);
    HIPCHK(e, hipMemcpyAsync(h.data(), cnt, ((size_t)N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));      // count and kp_match in one copy
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *n_matches = h[0];
    if (N > 0) memcpy(kp_match_host, h.data() + 1, (size_t)N * sizeof(int32_t));
    return JSORB_OK;
}

int jsorb_search_last_frame_stats(jsorb_extractor *e, int *passes, int *n_candidates, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    if (!e->lf.done) { e->err = "search_last_frame_stats before jsorb_search_last_frame"; return JSORB_ERR_STATE; }
    int32_t s[LF_CTL] = {0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(s, e->lf.ws + e->g.T, sizeof(s), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (passes) *passes = s[1];
    if (n_candidates) *n_candidates = s[2];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[3 + b];
    return JSORB_OK;
}

// ---- relocalisation matching: ORBmatcher::SearchByProjection(CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cpp:1968-2095), k_search_kf.hip ----
#define KF_STATS 8                 // statistics words: rounds, candidates, overflowed points, ind1..3
int jsorb_search_by_projection_kf_async(jsorb_extractor *e, int image, const jsorb_kf_projection_params *params, int n_points, const float *Px,
                                        const float *Py, const float *Pz, const float *max_distance, const float *max_dist_inv,
                                        const float *min_dist_inv, const float *kf_angle, const uint8_t *mp_descriptors, const uint8_t *blocked_in,
                                        int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) { e->err = "search_by_projection_kf: no extract result for this image"; return JSORB_ERR_STATE; }
    if (!params || !n_matches_dev) { e->err = "search_by_projection_kf: NULL params or n_matches"; return JSORB_ERR_INVALID; }
    const jsorb_kf_projection_params &p = *params;
    if (p.cols < 1 || p.rows < 1 || (long long)p.cols * p.rows > 16384) { e->err = "search_by_projection_kf: grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_by_projection_kf: n_points < 0"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image);
    if (n >= (1 << 18)) { e->err = "search_by_projection_kf: more than 262143 keypoints"; return JSORB_ERR_UNSUPPORTED; }
    if (n_points > 0 && (!Px || !Py || !Pz || !max_distance || !max_dist_inv || !min_dist_inv || !kf_angle || !mp_descriptors || !match_kp || !match_dist)) {
        e->err = "search_by_projection_kf: NULL point array or output";
        return JSORB_ERR_INVALID;
    }
    if (n > 0 && !kp_match) { e->err = "search_by_projection_kf: NULL kp_match"; return JSORB_ERR_INVALID; }
    if ((uintptr_t)mp_descriptors % 16) { e->err = "search_by_projection_kf: mp_descriptors must be 16-byte aligned"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int cap = search_kf_cap(), pts = std::max(n_points, 1);
    RCCHK(grid_reserve(e, p.cols * p.rows));
    RCCHK(reserve_device(e, e->kf.cand, (size_t)pts * (cap + 1) * sizeof(int), &e->kf.points, pts));
    RCCHK(reserve_device(e, e->kf.stats, KF_STATS * sizeof(int)));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the frame may come from the lanes of a batch
    mark_main_stream(e);               // ... and the next batch's lanes must not rewrite it before these kernels have read it
    const float *xy_un = jsorb_keypoints_un_device(e, image);
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(jsorb_keypoints_device(e, image), xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows,
                                                     e->grid.start, e->grid.items, st));
    HIPCHK(e, hipGetLastError());
    SearchKfArgs a{};
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = xy_un;
    a.desc = jsorb_descriptors_device(e, image);
    a.blocked = blocked_in;
    a.n_kp = n;
    a.cell_start = e->grid.start;
    a.cell_items = e->grid.items;
    a.n_points = n_points;
    a.Px = Px; a.Py = Py; a.Pz = Pz; a.max_distance = max_distance; a.max_dist_inv = max_dist_inv; a.min_dist_inv = min_dist_inv;
    a.angle = kf_angle; a.mp_desc = mp_descriptors;
    a.p = p;
    a.n_levels = e->g.L;
    for (int l = 0; l < e->g.L; l++) a.scale[l] = e->g.lv[l].scale;
    a.cand = e->kf.cand;
    a.cand_n = e->kf.cand + (size_t)e->kf.points * cap;
    a.match_kp = match_kp; a.match_dist = match_dist; a.kp_match = kp_match; a.n_matches = n_matches_dev;
    a.stats = e->kf.stats;
    TIMED(e, JSORB_K_KF_CANDIDATES, launch_kf_candidates(a, st));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_KF_RESOLVE, launch_kf_resolve(a, st));
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
    if (!n_matches) { e->err = "search_by_projection_kf: NULL n_matches"; return JSORB_ERR_INVALID; }
    if (n_points < 0) { e->err = "search_by_projection_kf: n_points < 0"; return JSORB_ERR_INVALID; }
    if (!check_image(e, image)) { e->err = "search_by_projection_kf: no extract result for this image"; return JSORB_ERR_STATE; }
    const int N = jsorb_n_keypoints(e, image);
    if (N > 0 && !kp_match_host) { e->err = "search_by_projection_kf: NULL host output"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int pts = std::max(n_points, 1);
    RCCHK(reserve_device(e, e->kf.out, ((size_t)2 * pts + e->g.T + 1) * sizeof(int32_t), &e->kf.out_points, pts));
    int32_t *cnt = e->kf.out, *km = cnt + 1, *mk = km + e->g.T, *md = mk + e->kf.out_points;
    RCCHK(jsorb_search_by_projection_kf_async(e, image, params, n_points, Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle, mp_descriptors,
                                              blocked_in, mk, md, km, cnt));
    std::vector<int32_t> h((size_t)N + 1);
    HIPCHK(e, hipMemcpyAsync(h.data(), cnt, ((size_t)N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));      // count and kp_match in one copy
    HIPCHK(e, hipStreamSynchronize(e->stream));
    *n_matches = h[0];
    if (N > 0) memcpy(kp_match_host, h.data() + 1, (size_t)N * sizeof(int32_t));
    return JSORB_OK;
}

int jsorb_search_by_projection_kf_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    if (!e->kf.done) { e->err = "search_by_projection_kf_stats before jsorb_search_by_projection_kf"; return JSORB_ERR_STATE; }
    int32_t s[KF_STATS] = {0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(s, e->kf.stats, sizeof(s), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
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
#define SI_STATS 8                 // statistics words behind state and owner: rounds, candidates, overflowed points, displaced claims, ind1..3
int jsorb_search_for_initialization_async(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave,
                                          const float *f1_angle, const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12,
                                          int32_t *matches21, int32_t *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) { e->err = "search_for_initialization: no extract result for this image"; return JSORB_ERR_STATE; }
    if (!params || !n_matches_dev) { e->err = "search_for_initialization: NULL params or n_matches"; return JSORB_ERR_INVALID; }
    const jsorb_init_params &p = *params;
    if (p.cols < 1 || p.rows < 1 || (long long)p.cols * p.rows > 16384) { e->err = "search_for_initialization: grid size out of range (cols*rows <= 16384)"; return JSORB_ERR_INVALID; }
    if (n1 < 0) { e->err = "search_for_initialization: n1 < 0"; return JSORB_ERR_INVALID; }
    const int n = jsorb_n_keypoints(e, image);
    if (n >= (1 << 18)) { e->err = "search_for_initialization: more than 262143 keypoints"; return JSORB_ERR_UNSUPPORTED; }
    if (n1 > 0 && (!f1_octave || !f1_angle || !f1_descriptors || !prev_matched || !matches12)) {
        e->err = "search_for_initialization: NULL F1 array or output";
        return JSORB_ERR_INVALID;
    }
    if ((uintptr_t)f1_descriptors % 16) { e->err = "search_for_initialization: f1_descriptors must be 16-byte aligned"; return JSORB_ERR_INVALID; }
    HIPCHK(e, hipSetDevice(e->device));
    const int cap = search_init_cap(), pts = std::max(n1, 1);
    const size_t T = (size_t)e->g.T;
    RCCHK(grid_reserve(e, p.cols * p.rows));
    RCCHK(reserve_device(e, e->si.cand, (size_t)pts * (cap + 2) * sizeof(int), &e->si.points, pts));
    RCCHK(reserve_device(e, e->si.ws, (2 * T + SI_STATS) * sizeof(int)));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the frame may come from the lanes of a batch
    mark_main_stream(e);
    const float *xy_un = jsorb_keypoints_un_device(e, image);
    TIMED(e, JSORB_K_ASSIGN_GRID, launch_assign_grid(jsorb_keypoints_device(e, image), xy_un, n, p.min_x, p.min_y, p.inv_w, p.inv_h, p.cols, p.rows,
                                                     e->grid.start, e->grid.items, st));
    HIPCHK(e, hipGetLastError());
    SearchInitArgs a{};
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = xy_un;
    a.desc = jsorb_descriptors_device(e, image);
    a.n_kp = n;
    a.cell_start = e->grid.start;
    a.cell_items = e->grid.items;
    a.p = p;
    a.n1 = n1;
    a.octave = f1_octave; a.angle = f1_angle; a.f1_desc = f1_descriptors; a.prev = prev_matched;
    a.cand = e->si.cand;
    a.cand_n = e->si.cand + (size_t)e->si.points * cap;
    a.order = a.cand_n + e->si.points;
    a.state = e->si.ws;
    a.owner = e->si.ws + T;
    a.stats = e->si.ws + 2 * T;
    a.matches12 = matches12; a.matches21 = matches21; a.n_matches = n_matches_dev;
    launch_init_candidates(a, st);
    HIPCHK(e, hipGetLastError());
    launch_init_resolve(a, st);
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
    if (!e->si.done) { e->err = "search_for_initialization_stats before jsorb_search_for_initialization"; return JSORB_ERR_STATE; }
    int32_t s[SI_STATS] = {0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(s, e->si.ws + 2 * (size_t)e->g.T, sizeof(s), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
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
