// jsorb_frame.hip - host side of the Frame-side features around an extract: rectification maps, the camera (undistorted keypoints, image
// bounds), RGB-D depth and the feature grid (the grid matchers are in jsorb_search.hip).  Each feature keeps its state in its own part of the
// handle (jsorb_handle.h); run_pipeline and jsorb_destroy reach it through the *_after_extract / *_release functions here.
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

// The grid CSR for `n_cells` cells (grown on demand) and one item per keypoint slot of the handle.
int grid_reserve(jsorb_extractor *e, int n_cells)
{
    RCCHK(reserve_device(e, e->grid.start, (size_t)(n_cells + 1) * sizeof(int32_t), &e->grid.cells, n_cells));
    return reserve_device(e, e->grid.items, (size_t)e->g.T * sizeof(int32_t));
}

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

} // extern "C"
