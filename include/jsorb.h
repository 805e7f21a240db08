/*
 * jsorb.h - C ABI of libjsorb: the MI355X-native (HIP, gfx950) ORB front-end + stereo matcher that
 * replaces Jetson-SLAM's CUDA hot path.  Plain pointers and sizes only; no C++/torch types.
 *
 * Reference interfaces replaced (paths under the reference tree, ashishkumar822/Jetson-SLAM @ 2024-12-18):
 *   jsorb_create / jsorb_destroy   <- orb_cuda::ORB_GPU::ORB_GPU / ~ORB_GPU   include/cuda/orb_gpu.hpp:26-36, src/cuda/orb_gpu.cpp:22-451
 *                                     (built by Jetson_SLAM::ORBExtractor::ORBExtractor, include/ORBextractor.h:25-35, src/ORBextractor.cpp:75-87)
 *   jsorb_extract*                 <- ORBExtractor::extract -> ORB_GPU::extract   include/ORBextractor.h:40-42, src/cuda/orb_gpu.cpp:489-841
 *   jsorb_keypoints_* / jsorb_descriptors_* <- SyncedMem<int>/<unsigned char>::gpu_data()/to_cpu()  include/cuda/synced_mem_holder.hpp:10-65 (Frame.cpp:119-122)
 *   jsorb_level_* / jsorb_scale_*  <- public members height_, width_, image_, scale_, inv_scale_  include/cuda/orb_gpu.hpp:240-250 (used by Frame.cpp:784-801)
 *   jsorb_stereo_match*            <- Frame::ComputeStereoMatches -> ORB_GPU::ORB_compute_stereo_match  src/Frame.cpp:780-803, include/cuda/orb_gpu.hpp:218-229,
 *                                     src/cuda/orb_stereo_match.cu:105-580
 *
 * Output layout is the reference's: keypoints = 6N int32 in six consecutive blocks x[N] y[N] score[N] angle[N] (degrees, f32 bit
 * pattern) octave[N] size[N]; descriptors = 32N bytes; keypoint order = level-major, tile-raster within a level.
 * All functions return JSORB_OK (0) or a negative error; nothing throws across this boundary.
 * Threading: distinct handles may be used concurrently from different host threads (the reference runs the left and right
 * extractors in two std::threads, Frame.cpp:107-110); one handle is single-threaded.  There is no CPU fallback: if no gfx950
 * device / code object is available the calls fail with JSORB_ERR_HIP.
 */
#ifndef JSORB_H
#define JSORB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JSORB_OK 0
#define JSORB_ERR_INVALID (-1)      /* bad argument / unsupported parameter combination */
#define JSORB_ERR_HIP (-2)          /* a HIP runtime call failed (see jsorb_last_error) */
#define JSORB_ERR_UNSUPPORTED (-3)  /* parameter combination outside what this build supports */
#define JSORB_ERR_STATE (-4)        /* call order violation (e.g. stereo before extract) */

#define JSORB_MAX_LEVELS 16

typedef struct jsorb_extractor jsorb_extractor;

/* Mirrors the ORB_GPU / ORBExtractor constructor arguments (include/cuda/orb_gpu.hpp:26-36). */
typedef struct jsorb_params {
    int height, width;               /* level-0 image size */
    int n_levels;                    /* ORBextractor.nLevels */
    float scale_factor;              /* ORBextractor.scaleFactor */
    int fast_n_min, fast_n_max;      /* ORBextractor.FAST_N_MIN / FAST_N_MAX : bounded arc length */
    int th_fast_min, th_fast_max;    /* th_FAST_MIN is accepted and ignored exactly as the reference does (orb_gpu.cpp:42-47) */
    int tile_h, tile_w;              /* ORBextractor.tile_h / tile_w (level 0) */
    int fixed_multi_scale_tile_size;
    int apply_nms_ms, nms_ms_mode_gpu;
    int device_id;                   /* reference hard-wires 0 (ORBextractor.cpp:87) */
    int max_batch;                   /* images one extract call may process (>=1); 1 = reference behaviour - such a handle lays its launches out for the
                                        latency of ONE image (many short workgroups), a handle with max_batch > 1 for throughput */
} jsorb_params;

typedef struct jsorb_stereo_stats {
    int n_left, n_right;
    int n_candidate_pairs;           /* (iL,iR) pairs whose Hamming distance was evaluated */
    int n_corr_match;                /* matches refined by the 11x11 L1 window search */
    int n_depth;                     /* matches with a depth before the median cut */
    int n_final;                     /* after the 2.1 x median cut */
} jsorb_stereo_stats;

/* kernel ids for jsorb_kernel_time */
enum { JSORB_K_PYRAMID = 0, JSORB_K_DETECT, JSORB_K_COMPACT, JSORB_K_BLUR, JSORB_K_DESCRIBE, JSORB_K_STEREO, JSORB_K_MEDIAN, JSORB_K_NMS_MS, JSORB_K_RECTIFY, JSORB_K_COUNT };
/* kernels of the mono / RGB-D Frame steps (jsorb_set_camera, jsorb_rgbd_depth*): ids after the pipeline's; JSORB_K_COUNT_ALL ids in all */
enum { JSORB_K_UNDISTORT = JSORB_K_COUNT, JSORB_K_RGBD, JSORB_K_COUNT_ALL };
/* kernels of jsorb_search_local_points*: ids after JSORB_K_COUNT_ALL, which stays the end of the extract / Frame ids above and names no kernel
 * (jsorb_kernel_name gives ""); JSORB_K_ID_END is one past the last id */
enum { JSORB_K_ASSIGN_GRID = JSORB_K_COUNT_ALL + 1, JSORB_K_LOCAL_CANDIDATES, JSORB_K_LOCAL_RESOLVE, JSORB_K_ID_END };
/* kernels of jsorb_search_last_frame*: ids from JSORB_K_ID_END on (the grid is JSORB_K_ASSIGN_GRID again); JSORB_K_ID_COUNT is one past the last id */
enum { JSORB_K_LAST_MATCH = JSORB_K_ID_END, JSORB_K_LAST_RESOLVE, JSORB_K_ID_COUNT };
/* kernels of jsorb_bow_transform* / jsorb_search_by_bow*: ids after JSORB_K_ID_COUNT, which stays the end of the ids above and names no kernel;
 * JSORB_K_ID_ALL is one past the last id */
enum { JSORB_K_BOW_TRANSFORM = JSORB_K_ID_COUNT + 1, JSORB_K_BOW_GROUP, JSORB_K_BOW_MATCH, JSORB_K_BOW_RESOLVE, JSORB_K_ID_ALL };
/* kernels of jsorb_search_by_projection_kf*: ids after JSORB_K_ID_ALL, which stays the end of the ids above and names no kernel (the grid is
 * JSORB_K_ASSIGN_GRID again); JSORB_K_ID_LAST is one past the last id */
enum { JSORB_K_KF_CANDIDATES = JSORB_K_ID_ALL + 1, JSORB_K_KF_RESOLVE, JSORB_K_ID_LAST };

/* ---- lifetime ---- */
/* mask: NULL (no mask => all 255) or a height*width u8 level-0 mask in host memory. */
int jsorb_create(const jsorb_params *params, const uint8_t *mask, jsorb_extractor **out);
/* The mask at ITS OWN size (mask_width x mask_height, any size): every level, level 0 included, is resized from it directly with
 * cv::resize(INTER_NN)'s index rule - what orb_gpu.cpp:77-81 does with whatever image the yaml names.  jsorb_create is this call with
 * the level-0 size. */
int jsorb_create_masked(const jsorb_params *params, const uint8_t *mask, int mask_width, int mask_height, jsorb_extractor **out);
void jsorb_destroy(jsorb_extractor *e);
const char *jsorb_last_error(const jsorb_extractor *e);
const char *jsorb_version(void);
/* Host-only, touches no device: the launch plan a handle created with these parameters gets (no counterpart in the reference, whose launch shapes
 * are literals in its .cu files, e.g. src/cuda/orb_FAST_apply_NMS_G.cu:1405-1434).  out[0..7] = levels, k_detect form (1: compact, 0: full plane),
 * k_detect LDS bytes, spill chunks in the handle's arena, k_pyramid LDS bytes, k_detect workgroups per image, entries per spill chunk, 0 (reserved);
 * then 8 ints per level: tile rows per k_detect workgroup, tiles per workgroup, LDS pool entries, score-plane stride, survivor-list capacity,
 * 16-byte loads per lane and row of k_pyramid, the load count its kernel instantiates for that, tile rows of the level.  capacity >= 8 + 8 * levels. */
int jsorb_plan_launch(const jsorb_params *params, int32_t *out, int capacity);

/* Compaction launches (slot 1 of jsorb_plan_forms / jsorb_handle_forms): k_compact_flat with the candidates in registers (1024 threads: single
 * images, or small workgroups: batches; T <= 4096), k_compact_flat re-reading the tile list (small workgroups: batches, T <= 8192; 1024 threads:
 * T <= 65536), and k_compact, which compacts level by level and builds no scan-line buckets (T > 65536). */
enum { JSORB_COMPACT_REG_1024 = 0, JSORB_COMPACT_REG_BATCH, JSORB_COMPACT_FLAT_BATCH, JSORB_COMPACT_FLAT_1024, JSORB_COMPACT_LEVELS_1024 };
/* Host-only, touches no device (like jsorb_plan_launch): the kernel forms a handle with these parameters selects from its geometry alone.
 * out[0..7] = k_detect form (1: compact, 0: full plane - before jsorb_create's device checks), compaction launch (JSORB_COMPACT_*), stereo
 * candidate scan (1: scan-line buckets, 0: tile rows), k_blur_compact possible for a batch (0 / 1), single frames run k_detect and k_blur as one
 * launch (0 / 1), levels that replay K3's literal horizontal tree, NMS-MS CPU mode possible (0 / 1), 0 (reserved).  capacity >= 8. */
int jsorb_plan_forms(const jsorb_params *params, int32_t *out, int capacity);
/* The same for a created handle, as it actually runs (k_detect's form after any fall-back in jsorb_create), then what the LAST extract call ran:
 * out[8..11] = lanes K (0: no extract yet), lane order (0: plain order, k_blur_compact where possible; 1: odd lanes run k_blur first; 2: plain
 * order, nothing fused; -1: no extract yet), bit mask of the lanes that ran k_blur_compact, bit mask of the lanes that ran k_blur before
 * k_detect.  capacity >= 12. */
int jsorb_handle_forms(const jsorb_extractor *e, int32_t *out, int capacity);

/* The mask image the reference loads with cv::imread(str_mask) + cvtColor(BGR2GRAY) (orb_gpu.cpp:64-75; yaml keys mask.left / mask.right):
 * decodes a PNG (non-interlaced; gray, gray+alpha, RGB, RGBA, palette; 1-16 bit) or a binary PGM / PPM file to one gray byte per pixel, for
 * callers that do not link OpenCV.  Call with gray_out = NULL to obtain the size first.  JSORB_ERR_STATE: the file cannot be opened (the
 * reference then runs without a mask); JSORB_ERR_UNSUPPORTED: not one of these formats (text in jsorb_mask_image_last_error). */
int jsorb_read_mask_image(const char *path, int *width, int *height, uint8_t *gray_out, size_t capacity);
const char *jsorb_mask_image_last_error(void);

/* ---- extraction ---- */
/* Reference-shaped call: one host image (step = bytes per row), results stay on the device; *n_keypoints = N.  Synchronous. */
int jsorb_extract(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints);
/* Same, and the results are ALSO delivered into caller-owned device buffers (6*T int32 and 32*T bytes, T = jsorb_total_tiles, the
 * keypoint cap) in the same stream round trip: what the reference's extract() does with the caller's SyncedMem (orb_gpu.cpp:779-831
 * writes into out_keypoints.gpu_data() / out_keypoints_desc.gpu_data()).  Either destination may be NULL. */
int jsorb_extract_into(jsorb_extractor *e, const uint8_t *host_image, int step, int *n_keypoints, int32_t *dev_keypoints_dst, uint8_t *dev_descriptors_dst);
/* Same with the image already in device memory. */
int jsorb_extract_device(jsorb_extractor *e, const uint8_t *dev_image, int step, int *n_keypoints);
/* Batch mode: n_images (<= max_batch) images at dev_images + i*image_stride, rows `step` bytes apart.  Enqueues only; the
 * input buffer must stay valid until jsorb_sync (level 0 is read in place).  Results per image via the accessors below. */
int jsorb_extract_batch_device_async(jsorb_extractor *e, const uint8_t *dev_images, size_t image_stride, int step, int n_images);
/* Batch mode from host memory (pinned for asynchronous uploads; pageable works, the copy then blocks the caller).  Dense input
 * (image_stride == H*W, step == W, W a multiple of 16): one hipMemcpyAsync per batch on the device's upload stream into one of two
 * landing buffers that the kernels read in place, so that the upload of batch k+1 runs under the kernels of batch k; the host buffer may
 * be reused once the upload has run (jsorb_sync, or any later call that returned after it).  One image (n_images == 1) from any host
 * memory: copied into a pinned buffer of the handle by the calling thread and pulled over PCIe by the first kernel.  Strided input:
 * hipMemcpy2DAsync per image into the level-0 slab. */
int jsorb_extract_batch_host_async(jsorb_extractor *e, const uint8_t *host_images, size_t image_stride, int step, int n_images);
/* Wait for everything enqueued on this handle and refresh the host-side counts. */
int jsorb_sync(jsorb_extractor *e);

/* ---- rectification of raw images (Examples/Stereo/stereo_euroc.cpp:106-107 build the maps with cv::initUndistortRectifyMap, :145-146 run
 * cv::remap(INTER_LINEAR) on the host for both images of every frame before TrackStereo) ----
 * Once a handle has maps, every extract entry point above reads the caller's RAW image and level 0 is the remapped image: OpenCV's
 * remap(src, dst, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit gray in its fixed-point form (INTER_BITS = 5, taps outside the
 * source count as 0), computed on the device (k_rectify).  Everything downstream - pyramid, detection, descriptors, stereo, the mask (in
 * rectified coordinates), jsorb_level_image_device / jsorb_copy_level_image at level 0 - sees the rectified image.  Maps are per handle (left and
 * right differ) and have the handle's image size (source size == rectified size).  Setting or clearing maps waits for the handle's work in
 * flight, converts and uploads once: it is a set-up call, not meant to be made per frame.  A handle without maps behaves as before. */
/* Float maps (CV_32FC1, as stereo_euroc.cpp:106-107 builds them): map_step_floats floats between rows.  JSORB_ERR_INVALID unless width x height is
 * the handle's image size. */
int jsorb_set_rectify_maps(jsorb_extractor *e, const float *mapx, const float *mapy, int width, int height, int map_step_floats);
/* Maps already in the fixed-point form of cv::convertMaps: xy = CV_16SC2 (ix, iy), a = CV_16UC1 (fy << 5 | fx, masked to 10 bits); steps in
 * elements (xy_step in int16 pairs, a_step in uint16). */
int jsorb_set_rectify_maps_fixed(jsorb_extractor *e, const int16_t *xy, const uint16_t *a, int width, int height, int xy_step, int a_step);
int jsorb_clear_rectify_maps(jsorb_extractor *e);
int jsorb_rectify_enabled(const jsorb_extractor *e);   /* 1: maps set, 0: none, negative: bad handle */
/* Host-only, touches no device (like jsorb_plan_launch): the float -> fixed-point conversion jsorb_set_rectify_maps applies, for n map entries.
 * X = round-half-even(mapx * 32); NaN, inf or an X outside the int range -> X = INT_MIN (a pixel outside the source); xy[2i] = saturate_int16(X >> 5),
 * xy[2i+1] likewise from mapy, a[i] = (Y & 31) << 5 | (X & 31). */
int jsorb_rectify_convert_maps(const float *mapx, const float *mapy, int n, int16_t *xy, uint16_t *a);

/* ---- camera: keypoint undistortion of the mono / RGB-D Frame (Frame::UndistortKeyPoints, src/Frame.cpp:718-748; ComputeImageBounds :750-778) ----
 * The camera is Tracking's mK (fx, fy, cx, cy; CV_32F, zero skew) and mDistCoef (k1, k2, p1, p2[, k3]; CV_32F, k3 = 0 in the 4-coefficient form),
 * src/Tracking.cpp:80-91.  Undistortion is ACTIVE only when k1 != 0: the reference tests mDistCoef.at<float>(0) == 0.0 - k1 alone - and then takes
 * mvKeysUn = mvKeys and the bounds 0, cols, 0, rows even if p1, p2 or k3 are nonzero.
 * Arithmetic: OpenCV 4's undistortPoints(src, dst, K, D, noArray(), K) with the default criteria (5 iterations, no epsilon test), all in double:
 *   fx, fy, cx, cy, k* = (double) of the floats; ifx = 1./fx; ify = 1./fy; u, v = (double) keypoint x, y
 *   x = (u - cx)*ifx; y = (v - cy)*ify; x0 = x; y0 = y
 *   5 times: r2 = x*x + y*y; icdist = 1/(1 + ((k3*r2 + k2)*r2 + k1)*r2)
 *            if icdist < 0: x = (u - cx)*ifx; y = (v - cy)*ify; stop
 *            deltaX = 2*p1*x*y + p2*(r2 + 2*x*x); deltaY = p1*(r2 + 2*y*y) + 2*p2*x*y   (left to right)
 *            x = (x0 - deltaX)*icdist; y = (y0 - deltaY)*icdist
 *   x_un = (float)(fx*x + cx); y_un = (float)(fy*y + cy)
 * With an active camera every extract entry point also runs k_undistort behind the extraction (inside the single-frame graph, on every lane of a
 * batch) and jsorb_assign_features_to_grid bins (x_un, y_un).  Setting or clearing the camera waits for the handle's work in flight; results of an
 * extract made before the call are undistorted with the new camera right away.  A handle that never sets a camera allocates and launches nothing. */
typedef struct jsorb_camera { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } jsorb_camera;
int jsorb_set_camera(jsorb_extractor *e, const jsorb_camera *camera);        /* NULL clears */
int jsorb_camera_enabled(const jsorb_extractor *e);                          /* 1: undistortion active (k1 != 0), 0: not, negative: bad handle */
/* Host-only, touches no device (like jsorb_plan_launch): Frame::ComputeImageBounds (Frame.cpp:750-778) - the corners (0,0), (W,0), (0,H), (W,H)
 * undistorted as above; out = {minX = min(c0.x, c2.x), maxX = max(c1.x, c3.x), minY = min(c0.y, c1.y), maxY = max(c2.y, c3.y)}, or {0, W, 0, H}
 * when k1 == 0. */
int jsorb_image_bounds(const jsorb_camera *camera, int width, int height, float out[4]);
/* mvKeysUn of one image of the last batch: x_un[N] then y_un[N] (device: at image * 2T floats; NULL without an active camera).  The copy without
 * an active camera returns the keypoint coordinates as floats (mvKeysUn = mvKeys). */
const float *jsorb_keypoints_un_device(const jsorb_extractor *e, int image);
int jsorb_copy_keypoints_un(const jsorb_extractor *e, int image, float *xy /* 2N: x[N] then y[N] */);

/* ---- RGB-D: Frame::ComputeStereoFromRGBD (src/Frame.cpp:996-1017) with Tracking's depth conversion (src/Tracking.cpp:333-334) ----
 * Per keypoint i: d = depth at the DISTORTED keypoint (row y, column x), converted like imDepth.convertTo(CV_32F, factor) would convert it:
 *   JSORB_DEPTH_U16: d = (float)raw * factor (one rounding);  JSORB_DEPTH_F32: d = raw * factor if |factor - 1| > 1e-5, else d = raw.
 * factor is Tracking's mDepthMapFactor (already inverted, Tracking.cpp:230-234).  If d > 0 (NaN never passes): depth = d, uRight = x_un - mbf/d
 * (float, correctly rounded; x_un = kpU.pt.x, the keypoint's own x without an active camera), else both are -1.  Only the sampled pixels are read. */
#define JSORB_DEPTH_F32 0
#define JSORB_DEPTH_U16 1
/* Synchronous, image 0 of the last extract; host depth image (step_bytes between rows); u_right / depth: N host floats each (either may be NULL). */
int jsorb_rgbd_depth(jsorb_extractor *e, const void *host_depth, int format, size_t step_bytes, float factor, float mbf, float *u_right, float *depth);
/* Batch: image i of the last batch against the depth image at dev_depths + i * image_stride (device memory, valid until jsorb_sync); enqueues only.
 * n_images must be the last batch's; image_stride >= height * step_bytes.  Ordered after the work enqueued so far on the handle's main stream
 * (jsorb_set_stream), and work enqueued there afterwards runs after it. */
int jsorb_rgbd_depth_batch_device_async(jsorb_extractor *e, const void *dev_depths, size_t image_stride, size_t step_bytes, int format, float factor,
                                        float mbf, int n_images);
/* N floats of image `image` from the last RGB-D call since the last extract; NULL (copy: JSORB_ERR_STATE) for images it did not cover - the
 * synchronous call covers image 0 only. */
const float *jsorb_rgbd_uright_device(const jsorb_extractor *e, int image);
const float *jsorb_rgbd_depth_device(const jsorb_extractor *e, int image);
int jsorb_copy_rgbd(const jsorb_extractor *e, int image, float *u_right, float *depth);

/* ---- results (valid after a synchronous call or jsorb_sync, until the next extract on the handle) ----
 * Work the library enqueued on the handle that reads an extract's results (the matchers, jsorb_bow_transform_async, jsorb_init_reference_set, ...)
 * completes before the next extract overwrites them, with no wait needed from the caller: extract, matcher, next extract - of any batch size, on
 * the handle's own stream or on one given with jsorb_set_stream - may be enqueued back to back.  (Buffers the CALLER reads on a stream of its own
 * are the caller's to order: jsorb_stream_wait_done.) */
int jsorb_n_images(const jsorb_extractor *e);
int jsorb_n_keypoints(const jsorb_extractor *e, int image);
int jsorb_level_n_keypoints(const jsorb_extractor *e, int image, int level);
const int32_t *jsorb_keypoints_device(const jsorb_extractor *e, int image);   /* 6N int32, layout above */
const uint8_t *jsorb_descriptors_device(const jsorb_extractor *e, int image); /* 32N bytes */
int jsorb_copy_keypoints(const jsorb_extractor *e, int image, int32_t *host_dst /* 6N */);
int jsorb_copy_descriptors(const jsorb_extractor *e, int image, uint8_t *host_dst /* 32N */);

/* ---- geometry / tables (mirrors ORB_GPU::height_, width_, scale_, inv_scale_, tile grid) ---- */
int jsorb_n_levels(const jsorb_extractor *e);
int jsorb_level_dims(const jsorb_extractor *e, int level, int *height, int *width, int *pitch);
int jsorb_level_tiles(const jsorb_extractor *e, int level, int *tile_h, int *tile_w, int *n_tile_h, int *n_tile_w, int *level_offset);
int jsorb_total_tiles(const jsorb_extractor *e);
float jsorb_scale(const jsorb_extractor *e, int level);
float jsorb_inv_scale(const jsorb_extractor *e, int level);
/* Device pointer to the un-blurred (blurred=0) or 7x7-blurred (blurred=1) pyramid level of an image (ORB_GPU::image_/image_gaussian_). */
const uint8_t *jsorb_level_image_device(const jsorb_extractor *e, int image, int level, int blurred);
int jsorb_copy_level_image(const jsorb_extractor *e, int image, int level, int blurred, uint8_t *host_dst /* H*W, pitch W */);
/* The per-level feature mask (ORB_GPU::masks_[level], orb_gpu.cpp:64-91: cv::resize(INTER_NN) of the level-0 mask, then
 * threshold(10)): H*W bytes 0 / 255, pitch W; all 255 when the handle has no mask. */
int jsorb_copy_level_mask(const jsorb_extractor *e, int level, uint8_t *host_dst);
/* Per-tile candidates before compaction (x,y,score), T entries each: debugging / stage-level parity. */
int jsorb_copy_tile_candidates(const jsorb_extractor *e, int image, int32_t *x, int32_t *y, int32_t *score);
/* Per-keypoint orientation in radians in output order (N floats). */
int jsorb_copy_angles(const jsorb_extractor *e, int image, float *host_dst);

/* ---- stereo ---- */
/* Reference-shaped call on image 0 of each handle: fills u_right[N_left], depth[N_left] (host, -1 = no match).  Synchronous.
 * mb is passed explicitly (the reference reads Frame::mb before it is assigned - SURVEY Appendix C-5); th_high/th_low are
 * ORBmatcher::TH_HIGH/TH_LOW = 100/50 (ORBmatcher.cpp:24-25). */
int jsorb_stereo_match(jsorb_extractor *left, jsorb_extractor *right, float mb, float mbf, int th_high, int th_low,
                       float *u_right, float *depth, jsorb_stereo_stats *stats);
/* Speculative match: OFF unless asked for - jsorb_set_speculative_stereo(left, 1), which include/jsorb_compat.hpp calls when it sees the
 * Frame stereo call shape (ORB_compute_stereo_match / ComputeStereoMatches), or JSORB_SPECULATE=1; JSORB_SPECULATE=0 forbids it whatever
 * the caller asks for.  A mono / RGB-D flow (one extractor, no match) never arms it.  After one jsorb_stereo_match on a (left, right)
 * pair of single-image handles, the library enqueues the same match, with the same mb / mbf / thresholds, right behind the NEXT pair of
 * single-image extracts on the GPU (the extract call that arrives second does it), so that the following jsorb_stereo_match on that
 * pair finds its result finished instead of paying a host round trip between extract and match.  The result is adopted only when the
 * call names the same pair and parameters and neither handle has extracted again; otherwise it is dropped and the call runs as if
 * the feature did not exist.  Same kernels, same inputs, same outputs.  The two extract calls may come from two threads (as in
 * Frame.cpp:107-110); calls on ONE handle must not overlap, as before. */
int jsorb_set_speculative_stereo(jsorb_extractor *left, int on);
int jsorb_speculative_stereo_stats(const jsorb_extractor *left, long *n_adopted, long *n_dropped);
/* Batch mode: image i of `left` against image i of `right`; enqueues on left's stream after right's work. */
int jsorb_stereo_match_batch_async(jsorb_extractor *left, jsorb_extractor *right, float mb, float mbf, int th_high, int th_low);
const float *jsorb_stereo_uright_device(const jsorb_extractor *left, int image);
const float *jsorb_stereo_depth_device(const jsorb_extractor *left, int image);
int jsorb_copy_stereo(const jsorb_extractor *left, int image, float *u_right, float *depth, jsorb_stereo_stats *stats);
/* Inspection (tests): the L1 window distance of the accepted sub-pixel refinement per left keypoint, -1 = none - the values the median
 * cut of orb_stereo_match.cu:560-580 sorts (vDistIdx[].first), N_left int32. */
int jsorb_copy_stereo_l1(const jsorb_extractor *left, int image, int32_t *host_dst);
/* Inspection (tests): keep the intermediate results of the matcher the reference holds on the host between its two kernels -
 * per left keypoint 13 int32 = { best right index of K12's arg-min (-1: no candidate closer than th_high), its Hamming distance (th_high then),
 * the 11 L1 window sums of K13 + cublasSgemv (-1 where no window search ran) } - orb_stereo_match.cu:241-256, 294-470.  Off by default
 * (B x T x 52 bytes of device memory); while on, a speculative single-frame match is never adopted. */
int jsorb_set_stereo_diagnostics(jsorb_extractor *left, int on);
int jsorb_copy_stereo_diagnostics(const jsorb_extractor *left, int image, int32_t *host_dst /* 13 * N_left */);
/* Multi-GPU batch mode: write (N_left, N_right, N_matched) of every pair of the last batch, 3 int32 per pair, to a DEVICE
 * buffer (enqueued on left's stream) - the payload of the one collective of this path, an all-gather of per-pair counts. */
int jsorb_gather_counts_async(jsorb_extractor *left, jsorb_extractor *right, int32_t *dev_dst);

/* ---- Tracking-side GPU helpers: device pointers in and out, synchronous like the reference ---- */
/* orb_cuda::ORB_Search_by_projection_project_on_frame  include/cuda/orb_matcher.hpp:12-18, src/cuda/orb_matcher.cu:17-89 */
int jsorb_project_points(void *hip_stream, int n_points, const float *Px, const float *Py, const float *Pz, const float *Rcw, const float *tcw,
                         float fx, float fy, float cx, float cy, float minX, float maxX, float minY, float maxY,
                         float *u, float *v, float *invz, unsigned char *is_valid);
/* orb_cuda::ORB_compute_distances  include/cuda/orb_matcher.hpp:20-24, src/cuda/orb_matcher.cu:95-144 (descriptor bases 16-byte aligned) */
int jsorb_hamming_pairs(void *hip_stream, int n_pairs, const int *idx_left, const int *idx_right, const unsigned char *descriptor_left,
                        const unsigned char *descriptor_right, int *distance);
/* tracking_cuda::compute_isInFrustum_GPU  include/cuda/tracking_gpu.hpp, src/cuda/tracking_isinfrustum.cu:19-160
 * (u, v, invz, predictedlevel, viewCos are written only where is_infrustum becomes 1, as in the reference).  predictedlevel =
 * ceil(logf(MaxDistance / dist) / logScaleFactor), converted as the reference's device code does (saturating, NaN -> 0), clamped to
 * [0, nScaleLevels - 1]: a ratio of +inf gives the last level.  JSORB_ERR_INVALID: n_points < 0, or a NULL array with n_points > 0. */
int jsorb_is_in_frustum(void *hip_stream, int n_points, const float *Px, const float *Py, const float *Pz, const float *Pnx, const float *Pny,
                        const float *Pnz, const float *MaxDistance, const float *invariance_maxDistance, const float *invariance_minDistance,
                        const float *Rcw, const float *tcw, const float *Ow, float fx, float fy, float cx, float cy, int minX, int maxX, int minY,
                        int maxY, int nScaleLevels, float logScaleFactor, float viewCosAngle, float *invz, float *u, float *v, int *predictedlevel,
                        float *viewCos, unsigned char *is_infrustum);

/* ---- Frame-side unpacking: what Frame::Frame does on the host right after the two extract() calls ---- */
/* The memory layout of cv::KeyPoint (OpenCV 4: Point2f pt; float size, angle, response; int octave, class_id), 28 bytes. */
typedef struct jsorb_keypoint { float x, y, size, angle, response; int32_t octave, class_id; } jsorb_keypoint;
/* Frame.cpp:119-196: the keypoint SoA of one image of the last batch as cv::KeyPoint records + its descriptor rows (N x 32).
 * A device kernel interleaves the SoA; both arrays then come back with two asynchronous copies and ONE synchronisation (the
 * reference: four blocking SyncedMem::to_cpu() per stereo frame, then a host loop).  Either destination may be NULL. */
int jsorb_unpack_frame(jsorb_extractor *e, int image, jsorb_keypoint *keypoints, uint8_t *descriptors);
/* jsorb_unpack_frame plus mvKeysUn as cv::KeyPoint records (mvKeys with pt replaced, Frame.cpp:741-747) when the handle has an
 * active camera (jsorb_set_camera), mvKeys again otherwise.  Any destination may be NULL;
 * one synchronisation (none after a synchronous single-frame extract: the kernels wrote pinned host mirrors). */
int jsorb_unpack_frame_un(jsorb_extractor *e, int image, jsorb_keypoint *keys, jsorb_keypoint *keys_un, uint8_t *descriptors);
/* Frame::AssignFeaturesToGrid + Frame::PosInGrid (Frame.cpp:463-479, 696-706) on the device, as CSR over cols x rows cells:
 * cell (i, j) has index i*rows + j (mGrid[i][j]); cell_start has cols*rows + 1 entries; cell_items lists keypoint indices,
 * ascending inside a cell (the reference's push_back order).  Bins mvKeysUn: the undistorted coordinates when the handle has an active
 * camera (jsorb_set_camera), else the extracted keypoint coordinates (mvKeysUn == mvKeys: rectified stereo, k1 == 0).  Host destinations;
 * cols*rows <= 16384. */
int jsorb_assign_features_to_grid(jsorb_extractor *e, int image, float min_x, float min_y, float grid_element_width_inv,
                                  float grid_element_height_inv, int cols, int rows, int32_t *cell_start, int32_t *cell_items);

/* ---- local map matching: ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cpp:32-116) as called by
 * Tracking::SearchLocalPoints (src/Tracking.cpp:1346-1805) right after the frustum test ----
 * Map points i = 0 .. n_points-1 in the order the caller passed them to jsorb_is_in_frustum (the reference's map_points, a subsequence of
 * mvpLocalMapPoints whose other points have mbTrackInView = false); keypoints k of image `image` of the handle's last extract.  Per point, in order:
 *   skip i unless in_frustum[i]; L = predicted_level[i] (outside [0, n_levels): no candidate - outside the contract, reads nothing out of bounds)
 *   r = view_cos[i] >= 0.998f ? 2.5f : 4.0f (RadiusByViewingCos compares the float with the double 0.998, which is this test); if th != 1: r *= th;
 *   R = r * jsorb_scale(e, L) (mvScaleFactors; every step one float rounding)
 *   candidates = GetFeaturesInArea(u[i], v[i], R, L-1, L) (src/Frame.cpp:641-694) over the grid min_x, min_y, inv_w, inv_h, cols x rows that
 *     jsorb_assign_features_to_grid builds: cells max(0, (int)floorf(((x - min_x) - R) * inv_w)) .. min(cols-1, (int)ceilf(((x - min_x) + R) * inv_w)),
 *     likewise in y, with the reference's early returns (first >= cols / last < 0: none); ix outer, iy inner, a cell's keypoints ascending; kept
 *     when octave in [L-1, L] and |x_un - x| < R && |y_un - y| < R (x_un, y_un: jsorb_keypoints_un_device with an active camera, else the keypoint)
 *   dropped: blocked_in[k] != 0 (the caller's F.mvpMapPoints[k] && Observations() > 0 before the call; NULL: none), or a point j < i of this call
 *     matched k (the reference's F.mvpMapPoints[bestIdx] = pMP: every map point that is not bad has observations - the assumption this rests on)
 *   dropped: u_right[k] > 0 && fabsf(xr - u_right[k]) > R, xr = u[i] - mbf * invz[i] unfused (two roundings; a reference build that contracts it
 *     into an FMA - GCC on aarch64 does by default - can differ by one ulp in xr); u_right NULL: monocular, never applies
 *   dist = popcount Hamming distance of mp_descriptors[32 i ..] and the keypoint's descriptor; best / second best with the reference's strict <
 *     updates: best = min (dist, candidate position) over dist < 256, second = the same min over the rest; bestLevel / bestLevel2 their octaves
 *   match iff bestDist <= th_high && !(bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2)
 * All arrays are DEVICE pointers, in the layouts jsorb_is_in_frustum writes (u, v, invz, view_cos float; predicted_level int32; in_frustum u8) and
 * mp_descriptors n_points x 32 bytes, 16-byte aligned; u_right / blocked_in have one entry per keypoint (u_right: jsorb_stereo_uright_device or
 * jsorb_rgbd_uright_device).  Outputs: match_kp[i] = matched keypoint or -1, match_dist[i] = its distance or -1, kp_match[k] = map point matched
 * to k in this call or -1 (N entries), *n_matches_dev = nmatches.  The host applies F.mvpMapPoints[match_kp[i]] = map_points[i].
 * Enqueued on the handle's stream (jsorb_set_stream) behind the last extract; inputs written on other streams must be complete (jsorb_is_in_frustum
 * returns after its kernel).  Three kernels: the grid (k_assign_grid, into the handle's grid buffers), k_local_candidates, k_local_resolve.
 * cols * rows <= 16384, N < 262144.  n_points == 0 or N == 0: no match (kp_match all -1). */
typedef struct jsorb_search_params {
    float th;                        /* Tracking's th: 1, 3 for RGB-D, 5 right after a relocalisation (Tracking.cpp:1786-1791) */
    float nn_ratio;                  /* ORBmatcher(0.8) */
    int th_high;                     /* ORBmatcher::TH_HIGH = 100 */
    float mbf;
    float min_x, min_y, inv_w, inv_h; /* Frame::mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* FRAME_GRID_COLS, FRAME_GRID_ROWS */
} jsorb_search_params;
int jsorb_search_local_points_async(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                                    const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                                    const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp,
                                    int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the handle; *n_matches = nmatches and match_kp_host[n_points] (host) = match_kp. */
int jsorb_search_local_points(jsorb_extractor *e, int image, const jsorb_search_params *params, int n_points, const float *u, const float *v,
                              const float *invz, const int32_t *predicted_level, const float *view_cos, const uint8_t *in_frustum,
                              const uint8_t *mp_descriptors, const float *u_right, const uint8_t *blocked_in, int32_t *match_kp_host, int *n_matches);
/* Diagnostics of the last call (waits for it): fixed-point rounds of k_local_resolve, candidates over all points, points whose candidates
 * overflowed the per-point list (the resolver rescans the grid for them).  Any pointer may be NULL. */
int jsorb_search_local_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow);

/* ---- motion-model matching: ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (src/ORBmatcher.cpp:1314-1965)
 * as Tracking::TrackWithMotionModel calls it (src/Tracking.cpp:1030-1066), retry included.  The reference runs its GPU branch (use_gpu_ = true,
 * :1319; the branch :1647-1963), which this restates bit for bit ----
 * Points i = 0 .. n_points-1: the last frame's keypoints with a map point that are not outliers, in ascending last-frame index (the reference's
 * idx_map_point_last_frame, :1714-1731; the order matters: the last writer wins below).  Per point: the map point's world position Px, Py, Pz
 * (GetWorldPosExp), the last frame's octave (mvKeys[].octave) and angle (mvKeysUn[].angle), and the map point's descriptor (GetDescriptorExp,
 * 32 bytes).  The current frame is image `image` of the handle's last extract (mvKeysUn from k_undistort with an active camera, else the keypoints).
 * One pass with threshold th:
 *   project with K14's arithmetic (jsorb_project_points, :1753-1764): Pc = tcw + Rcw P per row as fma(z,R2,fma(x,R0,y*R1)) + t, invz = 1.0f/Pcz,
 *     u = fma(Pcx*fx, invz, cx), v likewise; no candidate when Pcz <= 0 or (u < min_x || u > max_x || v < min_y || v > max_y)
 *   R = th * jsorb_scale(e, octave_i) (:1797, one float product); an octave outside [0, n_levels) is outside the contract: no candidate, nothing read
 *   candidates = GetFeaturesInArea(u, v, invz, R, minLevel, maxLevel) (src/Frame.cpp:569-639) with (minLevel, maxLevel) = (oct, -1) when
 *     direction = +1 (bForward), (0, oct) when -1 (bBackward), (oct-1, oct+1) when 0 (:1801-1810).  The caller computes direction from its poses
 *     as :1657-1668 does: bForward = tlc.z > mb && !bMono, bBackward = -tlc.z > mb && !bMono.  Levels are checked only when minLevel > 0 ||
 *     maxLevel >= 0 (forward with oct == 0 checks none), octave < minLevel or (maxLevel >= 0 and octave > maxLevel) dropped.  Cells, early returns
 *     and walk order as jsorb_search_local_points (ix outer, iy inner, a cell's keypoints ascending); kept when |x_un - u| < R && |y_un - v| < R;
 *     dropped when u_right[k] > 0 && fabsf((u - mbf*invz) - u_right[k]) > R (two roundings; u_right NULL: monocular).  No keypoint is blocked:
 *     TrackWithMotionModel clears mvpMapPoints before each pass (Tracking.cpp:1047, 1063) and every point's candidates are gathered before any
 *     assignment, so the Observations() test never drops one and points do not claim keypoints from each other
 *   best = popcount Hamming distance with strict < updates in walk order from bestDist = 256 (:1898-1911): the minimum of (distance, walk position)
 *     over distances < 256; the point matches iff bestDist <= th_high (TH_HIGH = 100)
 *   assign in point order (:1913-1916): mvpMapPoints[best] = point i, nmatches++ (two points on one keypoint: both count, the larger i stays)
 *   check_orientation (ORBmatcher(0.9, true), :1918-1952): rot = last_angle - cur_angle (the current angle: keypoint SoA row 3, float bits),
 *     rot += 360.0f when rot < 0; bin = (int)roundf(rot * (1.0f/30)) (half away from zero), bin == 30 -> 0 (factor 1/30: only bins 0..12 occur);
 *     every matched point pushes its keypoint into its bin, duplicates included; ComputeThreeMaxima (:2097-2138: strict >, the earlier bin wins a
 *     tie; then max2 < 0.1f*(float)max1 drops ind2 and ind3, else max3 < 0.1f*(float)max1 drops ind3); every entry of every other bin sets
 *     mvpMapPoints[k] = NULL and nmatches-- (a keypoint is nulled when any point that chose it is in a culled bin, even if a later point in a kept
 *     bin holds it; nmatches can differ from the non-null slots).  A bin outside [0, 30) - angles outside [0, 360) - is never kept
 * Retry (Tracking.cpp:1056-1064): when retry_below > 0 and the pass returns nmatches < retry_below, a second pass from scratch with 2*th replaces
 *   the first entirely (TrackWithMotionModel: retry_below = 20).  The device decides: the second pass's kernels are always enqueued (retry_below > 0)
 *   and return at once when the first pass's count says so - no host decision, capturable into a graph.
 * All arrays are DEVICE pointers: Px, Py, Pz, last_angle float[n]; last_octave int32[n]; mp_descriptors n x 32 bytes, 16-byte aligned; u_right
 * float[N] or NULL (jsorb_stereo_uright_device / jsorb_rgbd_uright_device).  Outputs: match_kp[i] / match_dist[i] = the point's best keypoint and
 * distance when it matched (before culling), -1 otherwise; kp_match[k] = the final mvpMapPoints[k] as a point index or -1 (N entries);
 * *n_matches_dev = the reference's return value.  Enqueued on the handle's stream behind the last extract (and the lanes of a batch): the grid
 * (k_assign_grid, into the handle's grid buffers) and k_last_match + k_last_resolve per pass.  cols * rows <= 16384, N < 262144, direction in
 * {-1, 0, 1}.  n_points == 0 or N == 0: no match, kp_match all -1. */
typedef struct jsorb_last_frame_params {
    float th;                        /* 7 stereo / RGB-D, 15 monocular (Tracking.cpp:1051-1054) */
    int th_high;                     /* ORBmatcher::TH_HIGH = 100 */
    int check_orientation;           /* ORBmatcher(0.9, true): 1 */
    int direction;                   /* +1 bForward, -1 bBackward, 0 neither */
    int retry_below;                 /* a second pass with 2 th when the first finds fewer (20); 0: none */
    float fx, fy, cx, cy;            /* K14's camera: CurrentFrame.fx .. cy */
    float min_x, max_x, min_y, max_y; /* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY: K14's bounds and the grid origin */
    float inv_w, inv_h;              /* mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* FRAME_GRID_COLS, FRAME_GRID_ROWS */
    float mbf;
    float Rcw[9], tcw[3];            /* CurrentFrame.mTcw, row-major rotation and translation */
} jsorb_last_frame_params;
int jsorb_search_last_frame_async(jsorb_extractor *e, int image, const jsorb_last_frame_params *params, int n_points, const float *Px, const float *Py,
                                  const float *Pz, const int32_t *last_octave, const float *last_angle, const uint8_t *mp_descriptors,
                                  const float *u_right, int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the handle; kp_match_host[N] (host) = kp_match and *n_matches = nmatches, with one copy back. */
int jsorb_search_last_frame(jsorb_extractor *e, int image, const jsorb_last_frame_params *params, int n_points, const float *Px, const float *Py,
                            const float *Pz, const int32_t *last_octave, const float *last_angle, const uint8_t *mp_descriptors, const float *u_right,
                            int32_t *kp_match_host, int *n_matches);
/* Diagnostics of the last call (waits for it): passes that ran (1 or 2) and, for the pass whose results stand, the candidates over all points
 * (the reference's to_be_matched_count) and ComputeThreeMaxima's ind1..3 (-1: none, all -1 without check_orientation).  Any pointer may be NULL. */
int jsorb_search_last_frame_stats(jsorb_extractor *e, int *passes, int *n_candidates, int kept_bins[3]);

/* ---- monocular initialisation matching: ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cpp:392-507) as Tracking::MonocularInitialization calls it on every frame until the map exists (src/Tracking.cpp:724-794:
 * ORBmatcher matcher(0.9, true), windowSize 50) ----
 * F2 is image `image` of the handle's last extract: N keypoints, mvKeysUn from k_undistort with an active camera, else the keypoints; its angle
 * is keypoint SoA row 3 (float bits), its octave row 4.  F1 is given by the caller, one entry per F1 keypoint i1 = 0 .. n1-1: f1_octave int32,
 * f1_angle float (mvKeysUn[].angle), f1_descriptors n1 x 32 bytes (16-byte aligned), prev_matched float x[n1] then y[n1] (vbPrevMatched, read
 * and written).  matched_distance[k] = INT_MAX, matches21[k] = -1 per F2 keypoint, matches12[i1] = -1, nmatches = 0; then for i1 in order:
 *   skip i1 when f1_octave[i1] > 0.  A NEGATIVE octave is not skipped (the reference skips only > 0) and, as in the reference's
 *     GetFeaturesInArea(x, y, r, level1, level1) with level1 < 0, switches the level check off: keypoints of every F2 octave qualify
 *   candidates = GetFeaturesInArea(prev_x[i1], prev_y[i1], window, 0, 0) (src/Frame.cpp:641-694): cells, early returns and walk order exactly as
 *     jsorb_search_local_points (ix outer, iy inner, a cell's keypoints ascending) over the grid min_x, min_y, inv_w, inv_h, cols x rows; kept
 *     when its octave is 0 and |x_un - x| < window && |y_un - y| < window.  No candidate: next point
 *   dist = popcount Hamming distance of the two descriptors; a candidate with matched_distance[k] <= dist is skipped
 *   over the rest, in walk order: if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = k; } else if (dist < bestDist2)
 *     bestDist2 = dist; from INT_MAX both - bestDist and bestDist2 are the two smallest of the multiset (a tie with the best lowers the second),
 *     bestIdx2 the first in walk order with the minimum
 *   claim iff bestDist <= th_low (TH_LOW = 50) && (float)bestDist < (float)bestDist2 * nn_ratio (a float product; bestDist2 = INT_MAX without a
 *     second candidate).  On a claim of k = bestIdx2: when matches21[k] >= 0 that earlier point loses it (matches12[matches21[k]] = -1,
 *     nmatches--); then matches12[i1] = k, matches21[k] = i1, matched_distance[k] = bestDist, nmatches++; with check_orientation i1 is pushed
 *     into the bin of rot = f1_angle[i1] - angle2[k] (+ 360.0f when negative; bin = (int)roundf(rot * (1.0f/30)), 30 -> 0: the arithmetic of
 *     jsorb_search_last_frame; a bin outside [0, 30) is never kept)
 * then, with check_orientation, ComputeThreeMaxima (:2097-2138, as for jsorb_search_last_frame) over the bins' sizes - a displaced point still
 * sits in its bin - and for every entry i1 of every other bin: if matches12[i1] >= 0 it becomes -1 and nmatches--.  Last (:501-504): for every
 * i1 with matches12[i1] >= 0, prev_matched[i1] = F2's mvKeysUn[matches12[i1]].
 * All pointers are DEVICE pointers.  Outputs: matches12[n1]; matches21[N] (may be NULL) = the LAST claimant of each F2 keypoint or -1, as the
 * reference's vnMatches21 stands at its return: it is not touched by the orientation culling, so matches21[k] = i1 does not imply
 * matches12[i1] = k; *n_matches_dev = the reference's return value; prev_matched updated in place.
 * Enqueued on the handle's stream behind the last extract (and the lanes of a batch), no host decision, no allocation after the first call of a
 * size: the grid (k_assign_grid, into the handle's grid buffers), k_init_candidates, k_init_resolve.  cols * rows <= 16384, N < 262144.
 * n1 == 0 or N == 0: no match, prev_matched untouched. */
typedef struct jsorb_init_params {
    float window;                    /* windowSize: np_min = 50 (Tracking.cpp:762) */
    float nn_ratio;                  /* ORBmatcher(0.9, true) */
    int th_low;                      /* ORBmatcher::TH_LOW = 50 */
    int check_orientation;           /* 1 */
    float min_x, min_y, inv_w, inv_h; /* Frame::mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv of F2 */
    int cols, rows;                  /* FRAME_GRID_COLS, FRAME_GRID_ROWS */
} jsorb_init_params;
int jsorb_search_for_initialization_async(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave,
                                          const float *f1_angle, const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12,
                                          int32_t *matches21, int32_t *n_matches_dev);
/* Synchronous: the same with matches12 in a buffer of the handle; matches12_host[n1] and prev_matched_host[2 n1] (host, either may be NULL)
 * receive matches12 and the updated prev_matched, *n_matches the count, with one synchronisation.  prev_matched stays a device pointer. */
int jsorb_search_for_initialization(jsorb_extractor *e, int image, const jsorb_init_params *params, int n1, const int32_t *f1_octave,
                                    const float *f1_angle, const uint8_t *f1_descriptors, float *prev_matched, int32_t *matches12_host,
                                    float *prev_matched_host, int *n_matches);
/* Diagnostics of the last call (waits for it): fixed-point rounds of k_init_resolve summed over its chunks, candidates over all points, points
 * whose candidates overflowed the per-point list (rescanned from the grid), claims that took a keypoint from an earlier point, and
 * ComputeThreeMaxima's ind1..3 (-1: none, all -1 without check_orientation).  Any pointer may be NULL. */
int jsorb_search_for_initialization_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow, int *n_displaced, int kept_bins[3]);
/* Keeping the initial frame (Tracking's mInitialFrame lives for many frames, the handle's results only until the next extract):
 * jsorb_init_reference_set copies image `image`'s octave row, angle row, descriptors and mvKeysUn into buffers of the handle (device to
 * device, on the handle's stream; grown on demand, freed in jsorb_destroy) and sets the stored prev_matched to mvKeysUn (Tracking.cpp:735-737).
 * jsorb_init_reference_clear drops the copy (the buffers stay), jsorb_init_reference_n returns its keypoint count (-1: none).
 * jsorb_search_initial_frame runs jsorb_search_for_initialization_async with the stored arrays as F1 against image `image` of the last
 * extract - the stored prev_matched is consumed and updated - and returns matches12_host[n], prev_matched_host[2 n] (may be NULL) and the count. */
int jsorb_init_reference_set(jsorb_extractor *e, int image);
int jsorb_init_reference_clear(jsorb_extractor *e);
int jsorb_init_reference_n(const jsorb_extractor *e);
int jsorb_search_initial_frame(jsorb_extractor *e, int image, const jsorb_init_params *params, int32_t *matches12_host, float *prev_matched_host,
                               int *n_matches);

/* ---- bag of words: Frame::ComputeBoW (src/Frame.cpp:709-716) and ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 * (src/ORBmatcher.cpp:146-275) as Tracking::TrackReferenceKeyFrame (src/Tracking.cpp:919-932) and the first half of Tracking::Relocalization
 * (:1954-2004) call them ----
 * A jsorb_vocabulary is DBoW2's vocabulary tree (m_nodes, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) on one device, shared by any number of
 * handles on that device.  It is created from flat HOST arrays: node 0 is the root; the children of node i are
 * children[child_start[i] .. child_start[i + 1]) in the order of m_nodes[i].children (that order decides ties); a node without children is a leaf
 * (isLeaf(), :328); descriptors n_nodes x 32 bytes (the root's row is unused); word_id per node (-1 for inner nodes); weight per node, used only
 * as weight > 0 (a word with weight 0 is stopped, :1157).  The tree need not be uniform.  levels_up is the 4 of Frame::ComputeBoW, fixed per object.
 * JSORB_ERR_INVALID unless: n_nodes >= 2; every child id lies in [1, n_nodes) and appears exactly once and every node is reached from the root (a
 * tree rooted at 0); every leaf has word_id >= 0; depth_L in [1, 16]; levels_up >= 0; the tree is no deeper than depth_L; no node has 2^22 or
 * more children.  Nothing faults later on what creation accepted. */
typedef struct jsorb_vocabulary jsorb_vocabulary;
int jsorb_vocabulary_create(int device_id, int n_nodes, int depth_L, int levels_up, const int32_t *child_start, const int32_t *children,
                            const uint8_t *descriptors, const int32_t *word_id, const double *weight, jsorb_vocabulary **out);
void jsorb_vocabulary_destroy(jsorb_vocabulary *v);
/* n_words: the leaves.  Any pointer may be NULL. */
int jsorb_vocabulary_info(const jsorb_vocabulary *v, int *n_nodes, int *n_words, int *depth_L, int *levels_up, int *max_children);
/* The transform, TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (:1217-1259) per descriptor: from the root, at every level the
 * popcount Hamming distance to every child in child order, the smallest wins with a strict < (the first child wins a tie), until a leaf.
 *   word_id[i] = the leaf's word id
 *   node_id[i] = the node reached at level depth_L - levels_up (level 1: the root's children), with three cases defined here:
 *     root case      depth_L - levels_up <= 0: node_id = 0, the root (:1227)
 *     shallow leaf   the leaf lies above that level (the reference leaves nid uninitialised): node_id = the leaf's own node id; counted in
 *                    jsorb_bow_transform_stats' n_shallow.  Does not occur with a full tree
 *     stopped word   the leaf's weight is not > 0: word_id as usual, node_id = -1 - the keypoint is in no FeatureVector entry (:1157-1161)
 * Two things the reference leaves UNDEFINED are stated here, not reproduced:
 *   - the shallow leaf above: the vector form of transform declares `NodeId nid;` without a value (:1151, :1179), the per-feature form writes it
 *     only at level depth_L - levelsup, and `fv.addFeature(nid, i)` then reads whatever the stack held.  Here: the leaf's own id, counted.
 *   - loadFromTextFile's `while(!f.eof()) getline` (:1378-1420) reads one more, empty, line after a final newline - which every file
 *     saveToTextFile writes has (:1445) - and makes a node of it whose parent and leaf flag were never read.  Here (vocabulary.load_text):
 *     empty lines are skipped, the tree has the file's nodes and no other.  A line without children that is flagged isLeaf = 0 is
 *     a leaf to the reference's isLeaf() with the constructor's word id 0 (it counts as word 0); here it is a leaf without a word and creation
 *     refuses the tree (JSORB_ERR_INVALID).
 * What the reference does define - the first of equal children, the level of nid, levelsup >= L, a stopped word, the BowVector fold of the four
 * weightings, the order of m_nodes[i].children and of the word ids in a text file - is held to DBoW2's own code, compiled unmodified, by
 * tests/golden/ref_matcher_bow_transform.npz (tools/ref_bow/, tests/test_ref_bow.py, tests/test_gpu_ref_bow.py).
 * The host folds word_id into mBowVec with the vocabulary's own double weights in feature order (BowVector::addWeight / addIfNotExist), and node_id
 * into mFeatVec (addFeature(node_id[i], i) for node_id[i] >= 0, ascending i).
 * jsorb_bow_transform_descriptors: n descriptors at a DEVICE pointer (n x 32, 16-byte aligned) -> word_id[n], node_id[n] (device, either may be
 * NULL), enqueued on hip_stream (a hipStream_t on the vocabulary's device, NULL: the null stream); n == 0 launches nothing.
 * jsorb_bow_transform_async: image `image` of the handle's last extract (-1: every image, one launch) into buffers of the handle, on the handle's
 * stream behind the extract (and the lanes of a batch).  The buffers are allocated on the first call, freed in jsorb_destroy and stay valid until
 * the next extract; jsorb_bow_word_device / jsorb_bow_node_device return image `image`'s N entries (NULL before a transform of that image since the
 * last extract), jsorb_copy_bow waits and copies them to the host (either may be NULL).  JSORB_ERR_INVALID when the vocabulary lives on another
 * device than the handle. */
int jsorb_bow_transform_descriptors(void *hip_stream, const jsorb_vocabulary *v, int n, const uint8_t *descriptors, int32_t *word_id, int32_t *node_id);
int jsorb_bow_transform_async(jsorb_extractor *e, int image, const jsorb_vocabulary *v);
const int32_t *jsorb_bow_word_device(const jsorb_extractor *e, int image);
const int32_t *jsorb_bow_node_device(const jsorb_extractor *e, int image);
int jsorb_copy_bow(const jsorb_extractor *e, int image, int32_t *word_host, int32_t *node_host);
/* descriptors of the last jsorb_bow_transform_async whose leaf lay above the node level (waits for it) */
int jsorb_bow_transform_stats(jsorb_extractor *e, int *n_shallow);
/* The matcher: ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) for n_keyframes >= 0 keyframes (at most 256) against one frame, F = image `image`
 * of the handle's last extract with N keypoints: its descriptors, its angle (keypoint SoA row 3 as float bits, F.mvKeys[k].angle) and f_node[k], the
 * FeatureVector node of keypoint k or -1 (NULL: what the handle's last jsorb_bow_transform_async of this image wrote).  The keyframes are
 * concatenated: keyframe i is the entries kf_start[i] .. kf_start[i + 1] (HOST array of n_keyframes + 1 ascending offsets) of kf_node (its
 * FeatureVector node or -1), kf_valid (pMP && !pMP->isBad()), kf_angle (mvKeysUn[j].angle) and kf_descriptors (32 bytes each, 16-byte aligned) -
 * DEVICE arrays.  Node ids are arbitrary non-negative int32: they need not come from a jsorb_vocabulary.
 * The per-keypoint form equals DBoW2's FeatureVector by two facts, which are the contract: addFeature appends i_feature in ascending order
 * (FeatureVector.cpp:31-44, TemplatedVocabulary.h:1148-1161), and every keypoint is in at most one node - so nodes are independent and the order in
 * which they are processed changes no output.  Per keyframe, with j local to the keyframe (0 .. kf_start[i+1] - kf_start[i] - 1):
 *   match_kf[k] = -1 for all k, nmatches = 0 (:150-154)
 *   for every node id present on both sides (:167-251), for the keyframe's keypoints j of that node in ascending j (:174):
 *     skip j when !kf_valid[j] (:178-184)
 *     over the frame's keypoints k of that node in ascending k, skipping those with match_kf[k] >= 0 (:196), from bestDist1 = bestDist2 = 256,
 *       bestIdxF = -1: if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = k; } else if (d < bestDist2) bestDist2 = d; (:203-212)
 *       - the two smallest of the multiset (a tie with the best lowers the second), the index the first in walk order with the minimum
 *     claim iff bestDist1 <= th_low && (float)bestDist1 < nn_ratio * (float)bestDist2 (one float product, :215-217) - and bestIdxF >= 0, which the
 *       reference implies for th_low < 256: match_kf[bestIdxF] = j, nmatches++, and with check_orientation bestIdxF goes into the bin of
 *       rot = kf_angle[j] - angle_F[bestIdxF] (+ 360.0f when negative; bin = (int)roundf(rot * (1.0f/30)), 30 -> 0: the arithmetic of
 *       jsorb_search_last_frame) (:219-234)
 *   then, with check_orientation, ComputeThreeMaxima (:2097-2138, as for jsorb_search_last_frame) over the bins' sizes; every entry k of every
 *   other bin: match_kf[k] = -1, nmatches-- (:254-272).  A bin outside [0, 30) is never kept.
 * Outputs (DEVICE): match_kf n_keyframes x N (row i: keyframe i), n_matches_dev[n_keyframes].  Enqueued on the handle's stream behind the last
 * extract (and the lanes of a batch), no host decision, no allocation after the first call of a size: k_bow_group, k_bow_match, k_bow_resolve.
 * N < 262144, every keyframe shorter than 262144.  N == 0, n_keyframes == 0 and empty keyframes write -1 / 0 and launch nothing that reads. */
typedef struct jsorb_bow_params {
    float nn_ratio;                  /* 0.7 TrackReferenceKeyFrame, 0.75 Relocalization */
    int th_low;                      /* ORBmatcher::TH_LOW = 50 */
    int check_orientation;           /* 1 */
} jsorb_bow_params;
int jsorb_search_by_bow_async(jsorb_extractor *e, int image, const jsorb_bow_params *params, const int32_t *f_node, int n_keyframes,
                              const int32_t *kf_start, const int32_t *kf_node, const uint8_t *kf_valid, const float *kf_angle,
                              const uint8_t *kf_descriptors, int32_t *match_kf, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the handle; match_kf_host[n_keyframes x N] and n_matches_host[n_keyframes] (host), one synchronisation. */
int jsorb_search_by_bow(jsorb_extractor *e, int image, const jsorb_bow_params *params, const int32_t *f_node, int n_keyframes,
                        const int32_t *kf_start, const int32_t *kf_node, const uint8_t *kf_valid, const float *kf_angle,
                        const uint8_t *kf_descriptors, int32_t *match_kf_host, int *n_matches_host);
/* Diagnostics of the last call (waits for it): (keyframe, node) pairs present on both sides, Hamming distances computed, the most frame keypoints in
 * a node of such a pair, and keyframe 0's ComputeThreeMaxima ind1..3 (-1: none, all -1 without check_orientation).  Any pointer may be NULL. */
int jsorb_search_by_bow_stats(jsorb_extractor *e, int *n_node_pairs, int *n_distances, int *largest_node, int kept_bins[3]);
/* The compile-time caps of this build's matcher kernels (no device needed): frame entries of a node a lane of k_bow_match keeps in registers
 * (2; beyond 64 x that a node's entries are re-read per keyframe keypoint) and the keys k_bow_group sorts in LDS (4096; longer sides are sorted in
 * global memory).  Test builds lower them (jetson_slam_amd/build.py VARIANTS) and assert on these values.  Either pointer may be NULL. */
int jsorb_bow_build_caps(int *node_regs, int *sort_lds);

/* ---- relocalisation matching: ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th,
 * const int ORBdist) (src/ORBmatcher.cpp:1968-2095) as Tracking::Relocalization calls it twice per pose hypothesis (src/Tracking.cpp:2062-2092:
 * (.., 10, 100), PoseOptimization, (.., 3, 64)) ----
 * The frame is image `image` of the handle's last extract: N keypoints, mvKeysUn from k_undistort with an active camera, else the keypoints; its
 * angle is keypoint SoA row 3 (float bits), its octave row 4.  Points i = 0 .. n_points-1 are the keyframe's slots with pMP && !pMP->isBad() &&
 * !sAlreadyFound.count(pMP) in ascending slot index, compacted by the caller - the order decides the result.  Per point: the map point's world
 * position Px, Py, Pz (GetWorldPos), max_distance (mfMaxDistance), max_dist_inv / min_dist_inv (GetMaxDistanceInvariance / GetMinDistanceInvariance),
 * kf_angle (pKF->mvKeysUn[slot].angle) and the map point's descriptor (GetDescriptor, 32 bytes).  Per point, in order:
 *   1. project with K14's arithmetic (jsorb_project_points): Pc = tcw + Rcw P per row as fma(z,R2,fma(x,R0,y*R1)) + t, invz = 1.0f/Pcz,
 *      u = fma(Pcx*fx, invz, cx), v likewise; no candidate when Pcz <= 0 or (u < min_x || u > max_x || v < min_y || v > max_y)
 *   2. gate and level with K16's arithmetic (jsorb_is_in_frustum): o = P - Ow, dist = sqrtf(fma(oz,oz,fma(ox,ox,oy*oy))); no candidate when
 *      dist < min_dist_inv[i] || dist > max_dist_inv[i] (written so: a NaN passes, as in K16);
 *      L = clamp(cvt_rzi_s32(ceilf(logf(max_distance[i] / dist) / log_scale_factor)), 0, n_levels-1) with K16's logf and the device's float -> int
 *      rule (truncate, saturate, NaN -> 0): MapPoint::PredictScale with mfMaxDistance itself
 *   3. R = th * jsorb_scale(e, L) (one float product); candidates = GetFeaturesInArea(u, v, R, L-1, L+1) (src/Frame.cpp:641-694): cells, early returns
 *      and walk order as jsorb_search_local_points (ix outer, iy inner, a cell's keypoints ascending); kept when octave in [L-1, L+1] and
 *      |x_un - u| < R && |y_un - v| < R.  There is no uRight test
 *   4. dropped: blocked_in[k] != 0 (the caller's CurrentFrame.mvpMapPoints[k] != NULL before the call; NULL: none), or a point j < i of this call
 *      matched k (:2037, :2053) - also when that match is culled in step 6: culling comes after the loop
 *   5. best = popcount Hamming distance with strict < updates in walk order from bestDist = 256: the minimum of (distance, walk position) over
 *      distances < 256; point i matches iff bestDist <= orb_dist: mvpMapPoints[best] = point i, nmatches++
 *   6. check_orientation: rot = kf_angle[i] - frame angle, + 360.0f when negative; bin = (int)roundf(rot * (1.0f/30)), 30 -> 0 (the arithmetic of
 *      jsorb_search_last_frame; a bin outside [0, 30) is never kept).  A keypoint is matched at most once, so a bin holds each keypoint at most
 *      once.  After all points ComputeThreeMaxima (:2097-2138, as for jsorb_search_last_frame); every entry of every other bin:
 *      mvpMapPoints[k] = NULL, nmatches--
 * The reference's host code does steps 1 and 2 through cv::Mat products, cv::norm and the host's log, whose rounding depends on the OpenCV build and
 * is pinned by nothing in its tree; this library defines them as the arithmetic of K14 and K16, which the reference's own GPU branches use for the
 * same quantities (SearchByProjection(CurrentFrame, LastFrame, ..), isInFrustum).  Two differences from the host text follow:
 *   - K14's Pcz > 0 rule: the host code would project a point behind the camera through the centre; here it has no candidate
 *   - the level is converted with the device's float -> int rule (cvt_rzi_s32), as in jsorb_is_in_frustum: a ratio of +inf (max_distance = inf or
 *     dist = 0) gives the last level and NaN level 0, where the host's cast is undefined
 * Control flow, order, ties and the claim rule are the reference's.
 * All arrays are DEVICE pointers: Px, Py, Pz, max_distance, max_dist_inv, min_dist_inv, kf_angle float[n]; mp_descriptors n x 32 bytes, 16-byte
 * aligned; blocked_in uint8[N] or NULL.  Outputs: match_kp[i] / match_dist[i] = the point's keypoint and distance when it matched (before culling),
 * -1 otherwise; kp_match[k] = the point index finally matched to k or -1 (N entries); *n_matches_dev = the reference's return value.  Enqueued on
 * the handle's stream behind the last extract (and the lanes of a batch), no host wait: the grid (k_assign_grid, into the handle's grid buffers),
 * k_kf_candidates, k_kf_resolve.  cols * rows <= 16384, N < 262144.  n_points == 0 or N == 0: no match, kp_match all -1. */
typedef struct jsorb_kf_projection_params {
    float th;                        /* 10, then 3 (Tracking.cpp:2065, 2079) */
    int orb_dist;                    /* 100, then 64 */
    int check_orientation;           /* ORBmatcher matcher2(0.9, true): 1 */
    float fx, fy, cx, cy;            /* K14's camera: CurrentFrame.fx .. cy */
    float min_x, max_x, min_y, max_y; /* Frame::mnMinX, mnMaxX, mnMinY, mnMaxY: K14's bounds and the grid origin */
    float inv_w, inv_h;              /* mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* FRAME_GRID_COLS, FRAME_GRID_ROWS */
    float log_scale_factor;          /* Frame::mfLogScaleFactor */
    float Rcw[9], tcw[3], Ow[3];     /* CurrentFrame.mTcw, row-major rotation and translation; the camera centre -Rcw^T tcw */
} jsorb_kf_projection_params;
int jsorb_search_by_projection_kf_async(jsorb_extractor *e, int image, const jsorb_kf_projection_params *params, int n_points, const float *Px,
                                        const float *Py, const float *Pz, const float *max_distance, const float *max_dist_inv,
                                        const float *min_dist_inv, const float *kf_angle, const uint8_t *mp_descriptors, const uint8_t *blocked_in,
                                        int32_t *match_kp, int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the handle; kp_match_host[N] (host) = kp_match and *n_matches = nmatches, with one copy back. */
int jsorb_search_by_projection_kf(jsorb_extractor *e, int image, const jsorb_kf_projection_params *params, int n_points, const float *Px,
                                  const float *Py, const float *Pz, const float *max_distance, const float *max_dist_inv, const float *min_dist_inv,
                                  const float *kf_angle, const uint8_t *mp_descriptors, const uint8_t *blocked_in, int32_t *kp_match_host,
                                  int *n_matches);
/* Diagnostics of the last call (waits for it): fixed-point rounds of k_kf_resolve, candidates over all points (step 3's survivors that blocked_in
 * does not drop), points whose candidates overflowed the per-point list (the resolver walks their windows again) and ComputeThreeMaxima's ind1..3
 * (-1: none, all -1 without check_orientation).  Any pointer may be NULL. */
int jsorb_search_by_projection_kf_stats(jsorb_extractor *e, int *rounds, int *n_candidates, int *n_overflow, int kept_bins[3]);
/* The compile-time caps of this build's k_search_kf.hip (no device needed): keys kept per point (128) and the keypoint count up to which
 * k_kf_resolve keeps its claims in LDS (16384; beyond it they live in kp_match).  Test builds lower them (jetson_slam_amd/build.py VARIANTS) and
 * assert on these values.  Either pointer may be NULL. */
int jsorb_search_kf_build_caps(int *list_cap, int *lds_claims);

/* ---- triangulation matching: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (src/ORBmatcher.cpp:644-810) with
 * CheckDistEpipolarLine (:127-144), as LocalMapping::CreateNewMapPoints calls it once per covisible neighbour of a new keyframe
 * (src/LocalMapping.cpp:216-274: 10 neighbours with a stereo or RGB-D sensor, 20 with a monocular one) - all neighbours in one call ----
 * LocalMapping runs beside Tracking on its own thread, so this matcher belongs to no extractor handle: a jsorb_keyframe_matcher owns a non-blocking
 * stream and its scratch (sorted keys, statistics, the synchronous form's outputs; allocated on the first call of a size, never inside a later call
 * of the same or a smaller size; the first call of a LARGER size frees the old buffer with hipFree, which waits for the whole device once - the
 * extractors' streams included).  One matcher is single-threaded; distinct matchers and extractor handles may be used concurrently from different
 * host threads.  jsorb_keyframe_matcher_set_stream / _get_stream work like jsorb_set_stream (NULL restores the matcher's own stream).
 *
 * One fact about the reference decides the form: vbMatched2 is declared (:664) and read (:712) but NEVER SET in this tree (ORB-SLAM3 later added
 * vbMatched2[bestIdx2]=true; this reference does not have it).  So the result of a KF1 keypoint depends on no other KF1 keypoint, two of them may
 * take the same KF2 keypoint, and there is no sequential claim rule.  The device form reproduces exactly that.  An "exclusive" mode would be a
 * different algorithm pinned by nothing in the reference; it is out of scope.
 *
 * Inputs, DEVICE arrays unless said otherwise.  KF1, n1 entries: node1 int32 (the FeatureVector node of the keypoint or -1), free1 uint8
 * (GetMapPoint(idx1) == NULL), stereo1 uint8 (mvuRight[idx1] >= 0), x1, y1, angle1 float (mvKeysUn), desc1 n1 x 32 bytes, 16-byte aligned.  The
 * KF2s are concatenated: keyframe i is the entries kf_start[i] .. kf_start[i + 1] (HOST array of n_keyframes + 1 ascending offsets) of node2, free2,
 * stereo2, x2, y2, octave2 int32, angle2, desc2.  Per keyframe i, HOST arrays copied into the launch arguments: F12[9 i ..] row-major float from
 * ComputeF12, and epipole[2 i ..] = ex, ey of :651-657 - the caller computes both from cv::Mat as the reference does; the library does not redo
 * cv::Mat products whose rounding nothing pins.  params: th_low (TH_LOW = 50), check_orientation, only_stereo, n_levels in [1, JSORB_MAX_LEVELS]
 * (as jsorb_params), scale_factor[] and level_sigma2[] = the floats mvScaleFactors and mvLevelSigma2 of the KF2s.
 * Per keyframe, with j local to the keyframe:
 *   1. match12[k] = -1 for all k, nmatches = 0
 *   2. the two facts of jsorb_search_by_bow_async hold here too: ascending indices within a node, every keypoint in at most one node - so nodes
 *      are independent
 *   3. for every node on both sides and every idx1 of it: skip when !free1[idx1]; skip when only_stereo && !stereo1[idx1]
 *   4. walk the KF2 keypoints idx2 of the node in ascending order from bestDist = th_low, bestIdx2 = -1:
 *        skip when !free2; skip when only_stereo && !stereo2
 *        d = popcount Hamming distance; skip when d > th_low || d > bestDist - d == bestDist GOES ON, so among equal distances the last one in
 *          walk order that passes the geometry wins
 *        epipole gate, only when !stereo1 && !stereo2: skip when distex*distex + distey*distey < 100.0f * scale_factor[octave2] with
 *          distex = ex - x2, distey = ey - y2: two float products, one float add, no contraction, strict <, one float product on the right
 *        epipolar line (CheckDistEpipolarLine): a = x1*F00 + y1*F10 + F20, b = x1*F01 + y1*F11 + F21, c = x1*F02 + y1*F12 + F22,
 *          num = a*x2 + b*y2 + c, den = a*a + b*b - all float, left to right, separate multiplies and adds, no fma; den == 0 rejects;
 *          dsqr = num*num/den (one float product, one correctly rounded float division); accept iff
 *          (double)dsqr < 3.84 * (double)level_sigma2[octave2] - a DOUBLE comparison, as the C++ promotes it.  A NaN anywhere rejects
 *        on accept bestIdx2 = idx2, bestDist = d; a geometry failure leaves bestDist unchanged
 *      net rule: the winner is the minimum distance <= th_low over the entries that pass the geometry, ties to the largest walk position
 *   5. if bestIdx2 >= 0: match12[idx1] = bestIdx2, nmatches++, and with check_orientation idx1 goes into the bin of
 *      rot = angle1[idx1] - angle2[bestIdx2] (+ 360.0f when negative; bin = (int)roundf(rot * (1.0f/30)), 30 -> 0: the arithmetic of
 *      jsorb_search_last_frame).  A bin outside [0, 30) is never kept
 *   6. then, with check_orientation, ComputeThreeMaxima (:2097-2138, as for jsorb_search_last_frame); every idx1 of every other bin:
 *      match12[idx1] = -1, nmatches--
 *   7. vMatchedPairs is the (idx1, match12[idx1]) with match12 >= 0 in ascending idx1; the shim (include/jsorb_compat.hpp) builds it
 *   8. octave2 outside [0, n_levels): the entry never passes (after its distance was computed).  Defined here - the reference would read out of
 *      bounds.  Nothing faults on any device input
 *   9. n1 == 0, n_keyframes == 0 and empty keyframes write -1 / 0 and launch nothing that reads
 *  10. JSORB_ERR_INVALID: a NULL required pointer, descending (or negative) kf_start, more than 256 keyframes, n1 or a keyframe of 2^18 = 262144
 *      or more, n_levels out of range, descriptors not 16-byte aligned
 * Outputs (DEVICE): match12 n_keyframes x n1 (row i: keyframe i), n_matches_dev[n_keyframes].  Enqueued on the matcher's stream, no host decision
 * after the argument checks, capturable once the scratch has its size: k_bow_group (KF1 as the frame side), k_tri_match (32 keyframes per launch),
 * k_tri_resolve. */
typedef struct jsorb_keyframe_matcher jsorb_keyframe_matcher;
typedef struct jsorb_triangulation_params {
    int th_low;                      /* ORBmatcher::TH_LOW = 50 */
    int check_orientation;           /* 0 in CreateNewMapPoints: ORBmatcher matcher(0.6, false), LocalMapping.cpp:221 */
    int only_stereo;                 /* bOnlyStereo: false in LocalMapping::CreateNewMapPoints */
    int n_levels;                    /* pKF2->mnScaleLevels */
    float scale_factor[JSORB_MAX_LEVELS];   /* mvScaleFactors */
    float level_sigma2[JSORB_MAX_LEVELS];   /* mvLevelSigma2 */
} jsorb_triangulation_params;
int jsorb_keyframe_matcher_create(int device_id, jsorb_keyframe_matcher **out);
void jsorb_keyframe_matcher_destroy(jsorb_keyframe_matcher *m);
int jsorb_keyframe_matcher_set_stream(jsorb_keyframe_matcher *m, void *hip_stream);
void *jsorb_keyframe_matcher_get_stream(const jsorb_keyframe_matcher *m);
const char *jsorb_keyframe_matcher_last_error(const jsorb_keyframe_matcher *m);
int jsorb_search_for_triangulation_async(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, int n1, const int32_t *node1,
                                         const uint8_t *free1, const uint8_t *stereo1, const float *x1, const float *y1, const float *angle1,
                                         const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2, const uint8_t *free2,
                                         const uint8_t *stereo2, const float *x2, const float *y2, const int32_t *octave2, const float *angle2,
                                         const uint8_t *desc2, const float *F12, const float *epipole, int32_t *match12, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the matcher; match12_host[n_keyframes x n1] and n_matches_host[n_keyframes] (host), one copy back. */
int jsorb_search_for_triangulation(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, int n1, const int32_t *node1,
                                   const uint8_t *free1, const uint8_t *stereo1, const float *x1, const float *y1, const float *angle1,
                                   const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2, const uint8_t *free2,
                                   const uint8_t *stereo2, const float *x2, const float *y2, const int32_t *octave2, const float *angle2,
                                   const uint8_t *desc2, const float *F12, const float *epipole, int32_t *match12_host, int *n_matches_host);
/* Diagnostics of the last call (waits for it): n_node_pairs = (keyframe, node) pairs present on both sides; n_distances = Hamming distances
 * computed (step 3's KF1 keypoints x step 4's entries that pass the flags); n_line_tests = of those, the candidates that come to the epipolar-line
 * test in the order-free sense: d <= th_low, octave2 in range and the epipole gate passed or not applied (the `d > bestDist` skip of step 4, which
 * only drops entries that cannot win and depends on the walk so far, is not counted off); largest_node = the most KF2 keypoints in a node of such
 * a pair; kept_bins = keyframe 0's ComputeThreeMaxima ind1..3 (-1: none, all -1 without check_orientation).  Any pointer may be NULL. */
int jsorb_search_for_triangulation_stats(jsorb_keyframe_matcher *m, int *n_node_pairs, int *n_distances, int *n_line_tests, int *largest_node,
                                         int kept_bins[3]);

/* ---- fusing map points into keyframes: ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th)
 * (src/ORBmatcher.cpp:812-962) and its loop-closing overload Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:964-1087), with
 * KeyFrame::GetFeaturesInArea and KeyFrame::IsInImage (src/KeyFrame.cpp:573-617), as LocalMapping::SearchInNeighbors calls it
 * (src/LocalMapping.cpp:460-540): once per target keyframe with the current keyframe's map points (10 neighbours plus up to 5 second neighbours each
 * with a stereo sensor, 20 plus up to 5 each with a monocular one), then once into the current keyframe with every map point of all those keyframes -
 * each direction in ONE call of the keyframe matcher above, on its stream ----
 * What runs here is the search, :839-936: per (keyframe, point) the keypoint bestIdx and its distance bestDist, a pure function of the arrays as
 * they are before the call - there is no claim rule and no rotation check.  What touches the map stays with the caller: the head test
 * `!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)` (:833-837) and the tail :938-958 (Replace, AddObservation, AddMapPoint).  The caller walks the
 * keyframes and points in the reference's order, evaluates the head test on the LIVE map and applies the tail to best_idx.  ONE THING THE TAIL
 * MUTATES FEEDS THE SEARCH, and the caller has to follow it:
 *   - MapPoint::Replace ends with ComputeDistinctiveDescriptors() on the surviving point (src/MapPoint.cpp:243), which picks mDescriptor again
 *     from all the observations the survivor has just inherited (:273-338); SearchInNeighbors (LocalMapping.cpp:490-496) and SearchAndFuse
 *     (LoopClosing.cpp:596-617) search that point in the NEXT keyframe with the new descriptor.  Position, normal and distance range do not change
 *     (UpdateNormalAndDepth runs after all fusing).  So, after replaying keyframe k, every point of the list that is still good and whose 32
 *     descriptor bytes differ from those it was last searched with is searched again - one more call of this function over those points and the
 *     keyframes k+1.., `skip` set where the head test fails - and its best_idx / best_dist for those keyframes are replaced.  Within keyframe k
 *     nothing is searched again: the survivor of a Replace is either the point at hand, whose search there is over, or the point in the
 *     keyframe's slot, which the head test skips there.  Without this step the replay differs from the reference's loop (run against the
 *     reference's own ORBmatcher.cpp: tests/fuse_replay.py, tests/test_ref_matcher.py).
 * (A caller that keeps the map on the device takes jsorb_fuse_map_async below instead: the search, the head test and the tail in one call.)
 * With it the replay equals the sequential loop, because
 *   - vpMapPointMatches is a copy taken before the loop, so the point list of a call does not change under it;
 *   - the head test only ever goes from pass to skip while the loops run: isBad never reverts, and in a map whose slots and observations agree a
 *     point leaves a keyframe only by becoming bad.  So a pair the device searched and the replay skips costs work, never a result; `skip` lets
 *     the caller leave out what is known before the call.
 * Inputs, DEVICE arrays unless said otherwise.  Points i = 0 .. n_points-1: Px, Py, Pz (GetWorldPos), Nx, Ny, Nz (GetNormal), max_distance
 * (mfMaxDistance), min_dist_inv / max_dist_inv (GetMinDistanceInvariance / GetMaxDistanceInvariance) float[n_points]; desc n_points x 32 bytes
 * (GetDescriptor), 16-byte aligned.  The keyframes are concatenated: keyframe k is the entries kf_start[k] .. kf_start[k + 1] (HOST array of
 * n_keyframes + 1 ascending offsets) of x, y (mvKeysUn), octave int32, uright (mvuRight; NULL: every keyframe is monocular, as uright < 0
 * everywhere) and kf_desc.  Per keyframe, HOST arrays copied into the launch arguments like F12 and epipole above: Rcw[9 k ..] row-major, tcw[3 k ..],
 * Ow[3 k ..] (GetRotation, GetTranslation, GetCameraCenter; the loop-closing overload passes the rotation, translation and centre it derives from
 * Scw, :967-974).  skip: NULL or n_keyframes x n_points bytes; a nonzero byte gives -1 with no work done and no statistics.
 * The reference computes the projection, the distance and the level through cv::Mat products, cv::norm, cv::Mat::dot and the host's log, whose
 * rounding nothing in its tree pins; as for jsorb_search_by_projection_kf this library defines them as the arithmetic of the reference's own device
 * kernels where one exists.  Per (keyframe, point), all in float unless said otherwise:
 *   1. projection with K14's arithmetic (jsorb_project_points): Pc = tcw + Rcw P per row as fma(z,R2,fma(x,R0,y*R1)) + t, invz = 1.0f/Pcz,
 *      u = fma(Pcx*fx, invz, cx), v likewise.  No candidate unless Pcz > 0 (in the reference's text Pcz == 0 reaches an infinite invz and fails
 *      IsInImage; a NaN fails too)
 *   2. KeyFrame::IsInImage's own gate, half open: u >= min_x && u < max_x && v >= min_y && v < max_y; a NaN fails.  (Not K14's closed gate)
 *   3. ur = u - bf*invz: the product rounded, then the difference rounded - no fma
 *   4. distance gate with K16's arithmetic (jsorb_is_in_frustum): o = P - Ow, dist = sqrtf(fma(oz,oz,fma(ox,ox,oy*oy))); no candidate when
 *      dist < min_dist_inv[i] || dist > max_dist_inv[i] (written so: a NaN passes, as in the reference's comparison)
 *   5. viewing angle: dot = fma(oz,nz,fma(ox,nx,oy*ny)) (K16's chain); no candidate when dot < 0.5f*dist (a NaN passes)
 *   6. L = clamp(cvt_rzi_s32(ceilf(logf(max_distance[i] / dist) / log_scale_factor)), 0, n_levels-1) with K16's logf and the device's float -> int
 *      rule: MapPoint::PredictScale with mfMaxDistance itself
 *   7. radius = th * scale_factor[L] (one float product); cells, early returns and walk order of KeyFrame::GetFeaturesInArea as for
 *      jsorb_search_local_points (ix outer, iy inner, a cell's keypoints ascending) over the grid PosInGrid builds from x, y with roundf
 *   8. per keypoint k of the window, in walk order, from bestDist = 256:
 *        window: fabsf(x[k] - u) < radius && fabsf(y[k] - v) < radius
 *        level: octave[k] in [L-1, L]; an octave outside [0, n_levels) is never a candidate (at L = 0 the reference would read
 *          mvInvLevelSigma2[-1] there)
 *        with check_reprojection: ex = u - x[k], ey = v - y[k]; when uright[k] >= 0: er = ur - uright[k], e2 = ex*ex + ey*ey + er*er, dropped when
 *          (double)(e2 * inv_level_sigma2[octave]) > 7.8; otherwise e2 = ex*ex + ey*ey, dropped when (double)(e2 * inv_level_sigma2[octave]) > 5.99.
 *          Every product and sum rounded to float on its own, left to right; the comparison in DOUBLE, as the C++ promotes it; a NaN passes
 *        d = popcount Hamming distance; strict < updates bestDist, bestIdx: the first in walk order wins a tie
 *   9. nothing in 3 and 8 is contracted into an fma (the kernel writes them with __fmul_rn / __fadd_rn / __fsub_rn)
 *  10. a match iff bestDist <= th_low: best_idx = bestIdx (the keypoint's index WITHIN its keyframe), best_dist = bestDist; otherwise both -1
 * Outputs (DEVICE): best_idx, best_dist int32[n_keyframes x n_points] (row k: keyframe k; every entry is written), n_matched_dev[n_keyframes] = the
 * matches of each keyframe (nFused before the replay's head test).  Enqueued on the matcher's stream, no host decision after the argument checks,
 * capturable once the scratch has its size: k_fuse_grids (one workgroup per keyframe), k_fuse_match (32 keyframes per launch).
 * Limits: n_keyframes in [0, 256]; the keypoints of all keyframes of a call below 2^18 = 262144; cols * rows <= 4096 (what k_fuse_grids holds in
 * LDS); JSORB_ERR_INVALID for these, a NULL required pointer, descending or negative kf_start, th_low outside [0, 255], n_levels outside
 * [1, JSORB_MAX_LEVELS], descriptors not 16-byte aligned, a negative n_points.  n_points == 0 or n_keyframes == 0 is a valid call: the counts are
 * cleared, nothing else runs.  The statistics words and the "done" mark of a fuse are its own: a fuse leaves
 * jsorb_search_for_triangulation_stats as it was, and a triangulation leaves jsorb_fuse_stats as it was. */
typedef struct jsorb_fuse_params {
    float th;                        /* 3 in LocalMapping::SearchInNeighbors (the default), 4 in loop closing */
    int th_low;                      /* ORBmatcher::TH_LOW = 50; [0, 255] */
    int check_reprojection;          /* 1: Fuse(pKF, vpMapPoints, th) (:812); 0: the loop-closing overload (:964), which has no chi-square gate */
    float fx, fy, cx, cy, bf;        /* pKF->fx .. cy, mbf */
    float min_x, max_x, min_y, max_y; /* KeyFrame::mnMinX, mnMaxX, mnMinY, mnMaxY: IsInImage's bounds and the grid origin */
    float inv_w, inv_h;              /* mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* mnGridCols, mnGridRows */
    float log_scale_factor;          /* KeyFrame::mfLogScaleFactor */
    int n_levels;                    /* mnScaleLevels, [1, JSORB_MAX_LEVELS] */
    float scale_factor[JSORB_MAX_LEVELS];        /* mvScaleFactors */
    float inv_level_sigma2[JSORB_MAX_LEVELS];    /* mvInvLevelSigma2 */
} jsorb_fuse_params;
int jsorb_fuse_async(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int n_points, const float *Px, const float *Py, const float *Pz,
                     const float *Nx, const float *Ny, const float *Nz, const float *max_distance, const float *min_dist_inv,
                     const float *max_dist_inv, const uint8_t *desc, int n_keyframes, const int32_t *kf_start, const float *x, const float *y,
                     const int32_t *octave, const float *uright, const uint8_t *kf_desc, const float *Rcw, const float *tcw, const float *Ow,
                     const uint8_t *skip, int32_t *best_idx, int32_t *best_dist, int32_t *n_matched_dev);
/* Synchronous: the same into buffers of the matcher; best_idx_host, best_dist_host [n_keyframes x n_points] and n_matched_host[n_keyframes] (host),
 * one copy back.  JSORB_ERR_UNSUPPORTED when n_keyframes x n_points exceeds INT_MAX - 256. */
int jsorb_fuse(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int n_points, const float *Px, const float *Py, const float *Pz,
               const float *Nx, const float *Ny, const float *Nz, const float *max_distance, const float *min_dist_inv, const float *max_dist_inv,
               const uint8_t *desc, int n_keyframes, const int32_t *kf_start, const float *x, const float *y, const int32_t *octave,
               const float *uright, const uint8_t *kf_desc, const float *Rcw, const float *tcw, const float *Ow, const uint8_t *skip,
               int32_t *best_idx_host, int32_t *best_dist_host, int *n_matched_host);
/* Diagnostics of the last fuse (waits for it): n_windows = (keyframe, point) pairs that reached a window (passed steps 1-6 and the early returns
 * of step 7); n_walked = keypoints of those windows' cells; n_distances = Hamming distances computed (step 8's survivors); largest_window = the
 * most keypoints in the cells of one window.  A skipped pair and a keyframe without keypoints count nothing.  JSORB_ERR_STATE before the first fuse.
 * Any pointer may be NULL. */
int jsorb_fuse_stats(jsorb_keyframe_matcher *m, int *n_windows, int *n_walked, int *n_distances, int *largest_window);

/* ---- the map points' descriptors between two matcher calls: MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cpp:273-338), as LocalMapping
 * calls it for every map point it touches - ProcessNewKeyFrame (src/LocalMapping.cpp:158-159), CreateNewMapPoints (:448), SearchInNeighbors
 * (:532) - and as MapPoint::Replace (MapPoint.cpp:243), LoopClosing (src/LoopClosing.cpp:537) and Tracking's map initialisations do, for MANY
 * points in one call of the keyframe matcher above, on its stream ----
 * The descriptor it picks is the `desc` input of jsorb_fuse, jsorb_search_local_points, jsorb_search_last_frame, jsorb_search_by_projection_kf and
 * jsorb_search_by_projection_sim3; it is the recomputation the contract of jsorb_fuse_async asks for after the replay of keyframe k, and `changed`
 * below is that contract's "32 descriptor bytes differ from those it was last searched with".  What touches the map stays with the caller: the
 * reference walks mObservations, a std::map<KeyFrame*, size_t>, in pointer order and leaves out the keyframes that are bad (:292-298); the caller
 * lists each point's observations in the order its own map iteration gives, the bad keyframes left out (dropping entries changes no order).
 * For one point with the descriptors D[0 .. N-1] of its observations, in that order:
 *   1. N == 0: nothing happens, mDescriptor stays what it was (:287, :300)
 *   2. dist[i][j] = the popcount Hamming distance of D[i] and D[j] (ORBmatcher::DescriptorDistance), dist[i][i] = 0 (:306-316).  The reference
 *      keeps them in a float array and reads them back into ints: exact for values up to 256
 *   3. per row i the median is the element at index (size_t)(0.5*(N-1)) = (N-1)/2 of the ascending row (:323-325); the row INCLUDES the
 *      self-distance 0.  So every median is 0 for N = 1 and 2, the smaller of the two real distances for N = 3, the LOWER middle for an even N
 *   4. BestIdx is the FIRST i with the smallest median: strict < from INT_MAX, i ascending (:319-332).  The observations' order matters through
 *      this rule alone
 *   5. mDescriptor = D[BestIdx] (:336)
 * Inputs: DEVICE arrays, the sizes host values.  obs_start int32[n_points + 1]: the CSR of the observations, point p has obs_start[p] ..
 * obs_start[p + 1]; obs_row int32[n_obs]: each a row of kf_desc; kf_desc n_rows x 32 bytes, 16-byte aligned: the keyframes' descriptor matrices
 * concatenated as for jsorb_fuse / jsorb_search_for_triangulation (the caller adds its kf_start[k] to the keypoint index).  out_row: NULL (point p
 * writes row p) or int32[n_points], distinct rows of desc_out; read only with desc_out.
 * Outputs (DEVICE), every entry of the first two written: best_obs int32[n_points] = BestIdx within the point's own list, -1 for an empty or
 * invalid point; best_median int32[n_points] = the winning median, or -1.  desc_out (may be NULL) n_out_rows x 32 bytes, 16-byte aligned: the
 * point's row is overwritten with the winner's 32 bytes ONLY when best_obs[p] >= 0 (rule 1: the old descriptor stays); it must not overlap kf_desc
 * and may be the very `desc` array a following jsorb_fuse_async on the same matcher reads - the stream orders the two calls.  changed (may be NULL,
 * needs desc_out) uint8[n_points]: 1 when the row was written with bytes that differ from what it held, else 0.
 * Defined for every device input, nothing faults: a point is INVALID - -1 / -1, its row untouched, changed 0 - when obs_start[p] or
 * obs_start[p + 1] lies outside [0, n_obs], obs_start descends at p, one of its obs_row entries lies outside [0, n_rows), or (with desc_out) its
 * output row lies outside [0, n_out_rows).  The same row twice in one point is legal (distance 0), and so are points whose
 * ranges overlap (each point alone is judged).  There is no limit on N.
 * Enqueued on the matcher's stream, no host decision after the argument checks, launch shapes from the host sizes alone, capturable once the
 * scratch has its size: k_distinct_plan (the checks, the points binned by N), k_distinct_lanes (16 lanes a point for N <= 16, a wave a point for
 * N <= 64), k_distinct_block (a workgroup a point beyond, its descriptors in LDS up to 1024 of them) - jsorb_distinct_build_caps reports the three
 * numbers of the library in use.  JSORB_ERR_INVALID for a NULL required pointer, a negative size, kf_desc or desc_out not 16-byte aligned, changed
 * without desc_out.  n_points == 0 is a valid call that launches nothing.  The statistics words and the "done" mark are the call's own, as for fuse
 * and triangulation. */
int jsorb_distinctive_descriptors_async(jsorb_keyframe_matcher *m, int n_points, const int32_t *obs_start, int n_obs, const int32_t *obs_row,
                                        const uint8_t *kf_desc, int n_rows, const int32_t *out_row, int n_out_rows, uint8_t *desc_out,
                                        uint8_t *changed, int32_t *best_obs, int32_t *best_median);
/* Synchronous: the same with best_obs_host, best_median_host [n_points] on the host, one copy back; desc_out and changed stay DEVICE arrays. */
int jsorb_distinctive_descriptors(jsorb_keyframe_matcher *m, int n_points, const int32_t *obs_start, int n_obs, const int32_t *obs_row,
                                  const uint8_t *kf_desc, int n_rows, const int32_t *out_row, int n_out_rows, uint8_t *desc_out, uint8_t *changed,
                                  int32_t *best_obs_host, int32_t *best_median_host);
/* Diagnostics of the last call (waits for it): n_group, n_wave, n_block = the points whose CSR entry is valid with N in [1, group_lanes],
 * (group_lanes, wave_max], beyond; n_beyond_lds = those of n_block with more than lds_descriptors observations; n_empty = N == 0; n_invalid = the
 * invalid points; n_changed = rows written with other bytes than they held; largest_n = the largest N of a point with a valid CSR entry.
 * JSORB_ERR_STATE before the first call.  Any pointer may be NULL. */
int jsorb_distinctive_descriptors_stats(jsorb_keyframe_matcher *m, int *n_group, int *n_wave, int *n_block, int *n_beyond_lds, int *n_empty,
                                        int *n_invalid, int *n_changed, int *largest_n);
/* The compile-time caps of the library in use: lanes per point of the group tier (16), the largest N of the wave tier (64), descriptors the block
 * tier holds in LDS (1024).  Any pointer may be NULL. */
int jsorb_distinct_build_caps(int *group_lanes, int *wave_max, int *lds_descriptors);

/* ---- the local map on the device: Tracking::UpdateLocalPoints (src/Tracking.cpp:1818-1841), the frame marks and the map_points list of
 * Tracking::SearchLocalPoints (:1352-1367, :1410-1420) and K16 (src/cuda/tracking_isinfrustum.cu:19-117) over that list, in ONE call on the
 * handle's stream whose outputs are the inputs of jsorb_search_local_points_async ----
 * The map points live in a DEVICE table of n_rows rows chosen by the caller - the rows of desc_out in jsorb_distinctive_descriptors, which
 * writes `desc` in place; jsorb_map_points_scatter_async below writes the rest.  A keyframe's GetMapPointMatches() is its run of kf_point_row (one
 * row per keypoint, -1 = NULL); the local keyframes are concatenated under kf_start as for the keyframe matchers, in the order of
 * mvpLocalKeyFrames.  E = kf_start[n_keyframes] - kf_start[0] entries; entry j is kf_point_row[kf_start[0] + j].  frame_point_row[k] is the row of
 * mCurrentFrame.mvpMapPoints[k] (-1 = NULL) for the N keypoints of image `image` of the last extract.  In this order:
 *   1. frame marks (:1352-1367): keypoint k with r = frame_point_row[k] in [0, n_rows) and bad[r] == 0 marks row r as seen (mnLastFrameSeen) and
 *      gets blocked_in[k] = 1; every other keypoint - -1, any other row outside the table, a bad row (the reference sets it to NULL) - gets
 *      blocked_in[k] = 0.  frame_point_row NULL: no row is seen, blocked_in all 0.  blocked_in NULL: not written.
 *   2. mvpLocalMapPoints (:1822-1840): the entries in order; an entry is dropped when its row is negative (!pMP, n_null), when its row is
 *      >= n_rows (n_invalid_rows: counted, the table is never read there), when bad[row] != 0 (n_bad), or when an earlier entry that is not
 *      dropped has the same row (mnTrackReferenceForFrame, n_duplicates).  counts[0] = the entries kept.
 *   3. map_points (:1410-1420): those without the rows seen in step 1 (n_seen of them).  counts[1] = its size.
 *   4. K16 for each of them with the host values `prm` (the arguments of jsorb_is_in_frustum, Rcw / tcw / Ow by value): the same device function
 *      k_is_in_frustum runs, so u, v, invz, predicted_level, view_cos and the verdict are bit-equal to jsorb_is_in_frustum on the gathered
 *      arrays.  counts[2] = the points inside (nToMatch).
 *   5. output: the points inside, in list order, compacted: slot i < min(counts[2], capacity) holds point_row[i] = the table row, u, v, invz,
 *      predicted_level, view_cos, in_frustum[i] = 1 and mp_descriptors[32 i ..] = desc[32 row ..].  Every slot from there to `capacity` holds
 *      in_frustum = 0, point_row = -1, zeros in the other arrays.  counts[3] = the slots written, counts[4] = 1 when counts[2] > capacity: the
 *      points kept are then the first `capacity` of the list, a prefix.
 * jsorb_search_local_points_async(e, image, params, n_points = capacity, u, v, invz, predicted_level, view_cos, in_frustum, mp_descriptors,
 * u_right, blocked_in, ...) on these arrays gives the reference's matches, match_kp[i] belonging to row point_row[i]: SearchByProjection skips the
 * points outside the frustum (src/ORBmatcher.cpp:43-47), so leaving them out changes nothing, and the order is kept.
 * All arrays are DEVICE pointers except kf_start (HOST, n_keyframes + 1, ascending, >= 0); the outputs have `capacity` entries, blocked_in N,
 * counts_dev 5; table->desc and mp_descriptors 16-byte aligned.  Defined for every device input: a row is range-checked before anything is read
 * through it.  UpdateLocalKeyFrames' graph walk and the concatenation are jsorb_local_keyframes_async below (n_keyframes = 1 over its
 * local_point_row).  What stays on the host: IncreaseVisible over point_row, mbTrackInView, applying match_kp.
 * Enqueued on the handle's stream behind the last extract, no host decision after the argument checks, launch shapes from E, N and capacity
 * alone, capturable once the scratch has its size (a call with the same or larger n_rows, E and capacity has run); the call does not
 * synchronise.  Four kernels: k_lm_marks, k_lm_list, k_lm_scan, k_lm_write.  The scratch is one word per table row in the handle, grown only,
 * and every call restores the words it touched through its own entries and keypoints: the cost follows E + N + capacity, not n_rows.
 * JSORB_ERR_INVALID: NULL table, prm, kf_start (with n_keyframes > 0), counts_dev, a NULL table array with n_rows > 0, kf_point_row NULL with
 * E > 0, a NULL output with capacity > 0; n_rows < 0, n_keyframes < 0, capacity < 0; kf_start negative or descending; desc or mp_descriptors not
 * 16-byte aligned; E >= 2^24.  JSORB_ERR_STATE: no extract result for `image`.  n_keyframes == 0 or E == 0 is a valid call: the padding and
 * zero counts are written (and blocked_in, from the frame marks). */
typedef struct jsorb_map_point_table {       /* DEVICE arrays of n_rows entries */
    int n_rows;
    const float *Px, *Py, *Pz, *Pnx, *Pny, *Pnz;                                   /* MapPoint::GetWorldPosNormalExp */
    const float *MaxDistance, *invariance_maxDistance, *invariance_minDistance;    /* MapPoint::GetDistanceInvariances */
    const uint8_t *desc;                                                           /* n_rows x 32, 16-byte aligned: mDescriptor */
    const uint8_t *bad;                                                            /* isBad() */
} jsorb_map_point_table;
typedef struct jsorb_frustum_params {        /* host values, the arguments of jsorb_is_in_frustum */
    float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy;
    int minX, maxX, minY, maxY, nScaleLevels;
    float logScaleFactor, viewCosAngle;
} jsorb_frustum_params;
int jsorb_local_map_points_async(jsorb_extractor *e, int image, const jsorb_map_point_table *table, const jsorb_frustum_params *prm, int n_keyframes,
                                 const int32_t *kf_start, const int32_t *kf_point_row, const int32_t *frame_point_row, int capacity,
                                 int32_t *point_row, float *u, float *v, float *invz, int32_t *predicted_level, float *view_cos, uint8_t *in_frustum,
                                 uint8_t *mp_descriptors, uint8_t *blocked_in, int32_t *counts_dev);
/* Synchronous: the same, then point_row_host[capacity] and counts_host[5] (host) in one copy back.  point_row and counts_dev may be NULL here
 * (buffers of the handle take their place); when given they are written too. */
int jsorb_local_map_points(jsorb_extractor *e, int image, const jsorb_map_point_table *table, const jsorb_frustum_params *prm, int n_keyframes,
                           const int32_t *kf_start, const int32_t *kf_point_row, const int32_t *frame_point_row, int capacity, int32_t *point_row,
                           float *u, float *v, float *invz, int32_t *predicted_level, float *view_cos, uint8_t *in_frustum, uint8_t *mp_descriptors,
                           uint8_t *blocked_in, int32_t *counts_dev, int32_t *point_row_host, int32_t counts_host[5]);
/* Diagnostics of the last call (waits for it): E and the entries dropped by each rule of steps 2 and 3.  JSORB_ERR_STATE before the first call.
 * Any pointer may be NULL. */
int jsorb_local_map_stats(jsorb_extractor *e, int *n_entries, int *n_null, int *n_invalid_rows, int *n_duplicates, int *n_bad, int *n_seen);
/* The compile-time cap of the library in use: entries per chunk of the order-preserving compaction (1024). */
int jsorb_local_map_build_caps(int *scan_chunk);
/* Keeping the table current: everything a local BA, MapPoint::UpdateNormalAndDepth (src/MapPoint.cpp:367-408) or SetBadFlag (:182-206) changed,
 * in one kernel from one upload.  records[i] is written to row rows[i] of the nine float arrays and of `bad` (DEVICE arrays of n_rows entries;
 * rows and records DEVICE, n entries); a row outside [0, n_rows) is skipped; with the same row twice each field takes the value of one of
 * those records (the caller lists a row once).
 * Descriptors are not part of it: jsorb_distinctive_descriptors_async writes those in place.  Enqueued on hip_stream, does not synchronise.
 * JSORB_ERR_INVALID: n < 0, n_rows < 0, or a NULL array with n > 0. */
typedef struct jsorb_map_point_record {
    float P[3], Pn[3], MaxDistance, invariance_maxDistance, invariance_minDistance;
    uint8_t bad, pad[3];
} jsorb_map_point_record;
int jsorb_map_points_scatter_async(void *hip_stream, int n_rows, float *Px, float *Py, float *Pz, float *Pnx, float *Pny, float *Pnz, float *MaxDistance,
                                   float *invariance_maxDistance, float *invariance_minDistance, uint8_t *bad, int n, const int32_t *rows,
                                   const jsorb_map_point_record *records);

/* ---- the local keyframes on the device: Tracking::UpdateLocalKeyFrames (src/Tracking.cpp:1844-1952) and the concatenation of their
 * GetMapPointMatches() that jsorb_local_map_points_async reads, in ONE call on the handle's stream ----
 * With it TrackLocalMap runs from the frame's rows to the matches with no host list in between:
 *   jsorb_local_keyframes_async(e, graph, table, frame_point_row, n_frame, kf_capacity, entry_capacity, local_kf_slot, state_io, local_kf_start,
 *                               local_point_row, counts) and then
 *   jsorb_local_map_points_async(e, image, table, prm, 1, kf_start = {0, entry_capacity}, local_point_row, ...): the -1 padding behind E_total is
 *   dropped there as NULL entries (only n_null of its statistics grows by it) and the order is the reference's.
 * The graph is a struct of DEVICE arrays over S = max_keyframes slots chosen by the caller, as for the keyframe database:
 *   state[s]       0 = absent (a free slot, or a keyframe in no point's observations that LocalMapping::ProcessNewKeyFrame has not seen),
 *                  1 = in the map and good, anything else = isBad()
 *   order_key[s]   the order of std::map<KeyFrame*, int> (:1847): the binding writes (intptr_t)pKF; equal keys are ordered by slot
 *   point_off[s], point_len[s] into point_pool[pool_entries]: GetMapPointMatches() as table rows, -1 = NULL - the run the caller keeps for
 *                  kf_point_row.  registered[pool_entries], or NULL = all 1: 1 where that entry's point holds the keyframe in mObservations.  The
 *                  reference votes over observations (:1855), and a keyframe made by CreateNewKeyFrame is in its tracked points' observations
 *                  only after ProcessNewKeyFrame (src/LocalMapping.cpp:158).
 *   neighbours[s][10]   GetBestCovisibilityKeyFrames(10) as slots in its order, -1 padded: the keyframe database's table
 *   child_off[s], child_len[s] into child_pool[child_entries]: GetChilds() as slots in std::set<KeyFrame*> order;  parent[s]: -1 = none
 * A run with len < 0, off < 0 or off + len > entries is an empty run; nothing is read through it.  n_invalid_runs counts the point runs and the
 * child runs of that kind over the slots with state != 0.  A slot reference is USABLE when it lies in [0, S) and state != 0; every other one
 * (-1, out of range, absent) is skipped.  This is the one difference from the reference, which would read through the pointer.
 * In this order, `table` giving n_rows and bad (nothing else of it is read):
 *   1. mult[r] = the keypoints k < n_frame with frame_point_row[k] == r, 0 <= r < n_rows, bad[r] == 0 (:1848-1864; a point at two keypoints votes
 *      twice; the mvpMapPoints[i] = NULL of :1861 is what blocked_in of jsorb_local_map_points_async reports).  frame_point_row NULL or n_frame == 0:
 *      all 0.
 *   2. vote[s], for state[s] != 0: the sum of mult[row] over the entries of the slot's point run with registered != 0 and row in [0, n_rows)
 *      (:1855-1857; a run that lists a row twice counts it twice - the caller lists a row once).  n_counter = the slots with vote > 0.
 *   3. n_counter == 0 (:1866): local_kf_slot, n_local and ref_slot stay, counts[7] = 1, and step 6 runs over the kept list.
 *   4. the first list (:1876-1891): the slots with state == 1 and vote > 0 in ascending (order_key, slot) order, n_first of them; ref_slot = the
 *      first in that order whose vote is greater than every earlier one's, unchanged when the list is empty.  n_first > kf_capacity: the first
 *      kf_capacity are kept, counts[5] = 1 (ref_slot is still that of the whole list).
 *   5. the expansion (:1895-1945), over the elements of the first list in order: stop when the list holds more than 80; append the first usable
 *      slot of the element's neighbour row with state == 1 that is not in the list; the same for its child run; its parent, if usable and not in
 *      the list, is appended whatever its state and ENDS the expansion (the break of :1941 leaves the outer loop).  What an earlier element
 *      appended is in the list for the later ones.
 *   6. local_kf_start[i], i <= kf_capacity = the running sum of the point-run lengths of the list (an absent slot or an invalid run counts 0;
 *      E_total from n_local on); local_point_row[local_kf_start[i] + j] = the run's entries unchanged; -1 from E_total to entry_capacity;
 *      E_total > entry_capacity: the prefix is kept, counts[6] = 1.
 *   counts[8] = n_counter, n_first, n_local, ref_slot, E_total, kf_overflow, entry_overflow, kept_previous.
 * local_kf_slot[kf_capacity] and state_io[2] = {n_local, ref_slot} are IN/OUT (step 3): the caller sets state_io = {0, -1} once.
 * mpReferenceKF is the keyframe of ref_slot.  All arrays are DEVICE pointers.  Defined for every device input: a slot, a row or a run is
 * range-checked before anything is read through it.  Enqueued on the handle's stream, no host decision after the argument checks, launch shapes
 * from S, n_frame and the capacities alone, capturable once the scratch has its size; the call does not synchronise.  Five kernels: k_lk_marks,
 * k_lk_votes, k_lk_rank, k_lk_expand, k_lk_gather.  mult lives in the row words of jsorb_local_map_points_async and every call sets back the
 * words it touched, so the two calls follow each other on one handle in either order.
 * JSORB_ERR_INVALID: NULL graph, table, local_kf_slot, state_io, local_kf_start or counts_dev; a NULL graph array (other than registered, and
 * the pools of 0 entries) with S > 0; table->bad NULL with n_rows > 0; local_point_row NULL with entry_capacity > 0; a negative size;
 * S >= 2^24; kf_capacity < 84; entry_capacity >= 2^24. */
typedef struct jsorb_keyframe_graph {
    int max_keyframes, pool_entries, child_entries;
    const uint8_t *state;
    const int64_t *order_key;
    const int32_t *point_off, *point_len, *point_pool;
    const uint8_t *registered;
    const int32_t *neighbours, *child_off, *child_len, *child_pool, *parent;
} jsorb_keyframe_graph;
int jsorb_local_keyframes_async(jsorb_extractor *e, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                                const int32_t *frame_point_row, int n_frame, int kf_capacity, int entry_capacity, int32_t *local_kf_slot,
                                int32_t *state_io, int32_t *local_kf_start, int32_t *local_point_row, int32_t *counts_dev);
/* Synchronous: the same, then local_kf_slot_host[kf_capacity], state_host[2] and counts_host[8] (host) in one copy back
 * (src/Tracking.cpp:1947-1951: mpReferenceKF from state_host[1]). */
int jsorb_local_keyframes(jsorb_extractor *e, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table, const int32_t *frame_point_row,
                          int n_frame, int kf_capacity, int entry_capacity, int32_t *local_kf_slot, int32_t *state_io, int32_t *local_kf_start,
                          int32_t *local_point_row, int32_t *counts_dev, int32_t *local_kf_slot_host, int32_t state_host[2], int32_t counts_host[8]);
/* Diagnostics of the last call (waits for it): steps 2-5 of src/Tracking.cpp:1844-1952 - n_counter, n_first, n_local, the keyframes appended as
 * a neighbour, as a child and as a parent, n_invalid_runs, and what ended the expansion (0 the list's end, 1 more than 80, 2 a parent).
 * JSORB_ERR_STATE before the first call.  Any pointer may be NULL. */
int jsorb_local_keyframes_stats(jsorb_extractor *e, int *n_counter, int *n_first, int *n_local, int *n_neighbours, int *n_children, int *n_parents,
                                int *n_invalid_runs, int *end_reason);
/* The compile-time caps of the library in use (the walk of src/Tracking.cpp:1895-1945): slots whose membership bit lives in LDS (32768; beyond,
 * a byte in global memory) and child candidates held in LDS (4096; a run that does not fit is read from global memory). */
int jsorb_local_keyframes_build_caps(int *member_lds_slots, int *child_lds_entries);

/* ---- the frame's pose on the device: Optimizer::PoseOptimization (src/Optimizer.cpp:244-456), the call Tracking makes after every matcher
 * (src/Tracking.cpp:937, :1077, :1140; :2053, :2069, :2084 per relocalisation candidate), in ONE launch on the handle's stream ----
 * n_problems problems over image `image` of the last extract (N keypoints): one problem is a tracked frame, several are the relocalisation
 * candidates, which share the image and each have their own frame_point_row (mvpMapPoints as table rows, -1 = NULL) and Tcw (mTcw, 4x4 row-major).
 * EDGES (:285-365).  Keypoint k has an edge iff r = frame_point_row[k] lies in [0, n_rows).  bad[r] is not read: the reference does not test
 *   isBad() here (:287-288).  A row outside the table gives no edge and nothing is read through it (n_outside_rows of the statistics counts the
 *   rows >= n_rows).  Xw = the table's Px, Py, Pz[r], float widened to double (:315-318).  The observation is mvKeysUn[k].pt: x_un, y_un of
 *   jsorb_keypoints_un_device with an active camera, else the keypoint's x, y.  The information is inv_level_sigma2[octave of the keypoint], float
 *   widened to double (:304-305; an octave outside [0, 16) is clamped into it).  The edge is monocular when u_right is NULL or u_right[k] < 0 (:291),
 *   otherwise stereo with u_right[k] as the third measurement.  nInitialCorrespondences = the edges.
 * ARITHMETIC: a transcription of the chain, in double unless the reference says float, built with -ffp-contract=off.
 *   errors and Jacobians: Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:266-364 (e = obs - cam_project(T.map(Xw)); the stereo edge's
 *     const float invz = 1.0f/z of :300 is a float); chi2 = e . (info e).
 *   the robust kernel: Huber, Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp:78-91, its deltas the FLOATS sqrt(5.991) and sqrt(7.815)
 *     (src/Optimizer.cpp:278-279); robustInformation is rho[1] Omega only.
 *   the quadratic form: Thirdparty/g2o/g2o/core/base_unary_edge.hpp:56-66 (b -= rho[1] A^T Omega e, H += A^T (rho[1] Omega) A).
 *   the LM step: Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189 - lambda0 = 1e-5 max |H_jj| at iteration 0 of each optimize(),
 *     the trial loop with computeScale() + 1e-3, alpha = 1 - (2 rho - 1)^3 clamped to [1/3, 2/3], _ni doubling, Terminate on 10 failed trials or
 *     rho == 0, the (iniChi - currentChi) * 1e3 < iniChi counter with its limit of 3.  The outer loop is SparseOptimizer::optimize's
 *     (Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:376-414): it stops at the first result that is not OK.
 *   the update: SE3Quat::exp(dx) * estimate with the theta < 1e-5 branch and the quaternion normalisation (Thirdparty/g2o/g2o/types/se3quat.h:223-257,
 *     :104-110, :280-285), the rotations through Eigen's quaternion formulas.
 *   the solve: the 6x6 solve of Thirdparty/g2o/g2o/solvers/linear_solver_dense.h:65-113 as an LDL^T WITHOUT pivoting; a pivot that is not > 0 is
 *     "not positive definite": a failed trial (tempChi = DBL_MAX) whose dx is the last solved one (zero at the start of an optimize()).
 *   The sums over the edges are ONE fixed tree (a butterfly over each wave of 64 edges-in-thread-order, then the waves in order): no floating-point
 *   atomics; a problem's result depends on its inputs alone, not on the run, on n_problems or on its index in the batch.  It is NOT bit-equal to
 *   g2o: the tree is not Eigen's order, and sin, cos and pow are the device's.
 * THE FOUR ROUNDS (:379-447), quirks kept.  Every round restarts from Tcw_in (:382: setEstimate(toSE3Quat(pFrame->mTcw)), src/Converter.cpp:38-51).
 *   The edges flagged as outliers are left out (level 1) and re-tested each round on a freshly computed error at the round's estimate; an INLIER's
 *   chi2() reads the error its last computeError left, which is the LAST TRIAL's pose - after a rejected last trial the rejected pose, not the
 *   restored one.  The test is (float)chi2 > 5.991f, for a stereo edge > 7.815f.  The kernel comes off after round index 2.  The loop breaks after
 *   a round when the TOTAL number of edges is below 10.  A round with no active edge leaves the estimate at the initial one (g2o's optimize
 *   returns -1) and classifies all the same.
 * OUTPUTS, per problem.  counts[4] = nInitialCorrespondences, nBad of the last round run, the return value (nInitialCorrespondences - nBad; 0
 *   with fewer than 3 edges, :369-370), the rounds run.  With fewer than 3 edges Tcw_out = Tcw_in bit for bit, pose_out = its R and t widened, and the
 *   flags are 0.  Otherwise Tcw_out = Converter::toCvMat of the estimate (src/Converter.cpp:53-57): the doubles rounded to float, last row 0 0 0 1; and
 *   pose_out[12] = R row-major, t in double.  outlier[k] = mvbOutlier[k], 0 for a keypoint without an edge.  point_row_out[k] =
 *   frame_point_row[k], or -1 where outlier[k]: the discard of src/Tracking.cpp:1086-1103 (TrackLocalMap's caller uses it only for stereo,
 *   :1159-1160).
 * All arrays are DEVICE pointers: frame_point_row and outlier n_problems x N, u_right N or NULL, Tcw_in and Tcw_out n_problems x 16, pose_out
 * n_problems x 12 (8-byte aligned) or NULL, point_row_out n_problems x N or NULL, counts_dev n_problems x 4; `prm` and `table` are host structs (of
 * the table, n_rows, Px, Py, Pz and the alignment of desc are looked at).  Defined for every device input: a row is range-checked before
 * anything is read through it, and every loop is bounded (4 rounds x 10 iterations x 10 trials), so no input makes it spin.  Enqueued on the
 * handle's stream behind the last extract, no host decision after the argument checks, launch shapes from N and n_problems alone, capturable once
 * the scratch has its size (a call with the same or larger n_problems x N has run); the call does not synchronise.  One kernel:
 * k_pose_optimize, a workgroup a problem.
 * JSORB_ERR_INVALID: NULL prm or table; n_problems < 0 or n_rows < 0; NULL Px, Py or Pz with n_rows > 0; desc not 16-byte aligned; with
 * n_problems > 0 a NULL Tcw_in, Tcw_out or counts_dev, and with N > 0 a NULL frame_point_row or outlier; pose_out not 8-byte aligned.
 * JSORB_ERR_UNSUPPORTED: n_problems x N >= 2^31.  JSORB_ERR_STATE: no extract result for `image`.  Nothing is launched then. */
typedef struct jsorb_pose_params {           /* pFrame->fx, fy, cx, cy, mbf, mvInvLevelSigma2 */
    float fx, fy, cx, cy, bf;
    float inv_level_sigma2[JSORB_MAX_LEVELS];
} jsorb_pose_params;
int jsorb_pose_optimization_async(jsorb_extractor *e, int image, const jsorb_pose_params *prm, const jsorb_map_point_table *table, int n_problems,
                                  const int32_t *frame_point_row, const float *u_right, const float *Tcw_in, float *Tcw_out, double *pose_out,
                                  uint8_t *outlier, int32_t *point_row_out, int32_t *counts_dev);
/* Synchronous: the poses from the host (Tcw_host, n_problems x 16), then Tcw_out_host (n_problems x 16), pose_out_host (n_problems x 12, or NULL),
 * outlier_host (n_problems x N) and counts_host (n_problems x 4) on the host; buffers of the handle hold them on the device.  frame_point_row,
 * u_right and point_row_out (or NULL) stay DEVICE arrays.  The return value of src/Optimizer.cpp:455 is counts_host[4 p + 2]. */
int jsorb_pose_optimization(jsorb_extractor *e, int image, const jsorb_pose_params *prm, const jsorb_map_point_table *table, int n_problems,
                            const int32_t *frame_point_row, const float *u_right, const float *Tcw_host, float *Tcw_out_host,
                            double *pose_out_host, uint8_t *outlier_host, int32_t *point_row_out, int32_t *counts_host);
/* Diagnostics of the last call (waits for it), summed over its problems: n_outside_rows, monocular edges, stereo edges, LM iterations, trials,
 * rejected trials, failed solves, rounds without an active edge.  They are diagnostics: at convergence rho is rounding noise, so the iteration and
 * trial counts may differ between builds.  JSORB_ERR_STATE before the first call. */
int jsorb_pose_optimization_stats(jsorb_extractor *e, int32_t stats[8]);
/* The compile-time caps of the library in use: threads of a problem's workgroup (256) and edges a thread keeps in registers (4; the edges
 * beyond threads x registers are read again every pass). */
int jsorb_pose_optimization_build_caps(int *threads, int *edge_registers);
/* F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cpp:107) between a matcher and the optimisation: frame_point_row[match_kp[i]] = point_row[i]
 * wherever 0 <= match_kp[i] < N and point_row[i] >= 0; every other entry of frame_point_row stays.  The matchers give distinct match_kp; with a
 * duplicate ONE of the writers wins, which one is not defined.  DEVICE arrays: point_row and match_kp n_points, frame_point_row N.  With it
 * jsorb_local_map_points_async -> jsorb_search_local_points_async -> this -> jsorb_pose_optimization_async has no host hop.  Enqueued on
 * hip_stream, does not synchronise.  JSORB_ERR_INVALID: n_points < 0, N < 0, or a NULL array that would be read or written. */
int jsorb_apply_matches_async(void *hip_stream, int n_points, const int32_t *point_row, const int32_t *match_kp, int N, int32_t *frame_point_row);

/* ---- the covisibility graph on the device: KeyFrame::UpdateConnections (src/KeyFrame.cpp:293-383), AddConnection / UpdateBestCovisibles
 * (:127-161), EraseConnection (:557-571) and the getters over them, on a keyframe matcher (its stream, its scratch; LocalMapping and LoopClosing
 * each own one; no extractor handle is involved) ----
 * jsorb_covisibility is a struct of DEVICE arrays over the graph's S = max_keyframes slots, owned by the binding like jsorb_keyframe_graph, with
 * conn_capacity = C entries per slot, C within jsorb_covisibility_build_caps (16 to 2048):
 *   conn_len[S], conn_slot[S*C], conn_weight[S*C]   mConnectedKeyFrameWeights in ascending (order_key, slot) order - std::map<KeyFrame*, int>'s
 *   ord_len[S], ord_slot[S*C], ord_weight[S*C]      mvpOrderedConnectedKeyFrames / mvOrderedWeights.  Separate state, not a function of the map:
 *                  after a keyframe's own UpdateConnections they hold only the entries at or above the threshold, after an
 *                  UpdateBestCovisibles the whole map
 *   first_connection[S]   one byte: mbFirstConnection && mnId != 0; the binding writes 1 when it creates a keyframe other than the first
 * All of it starts as zeros.  The definitions of jsorb_local_keyframes_async hold: USABLE slot, valid run, (order_key, slot) order.
 *
 * jsorb_update_connections_async is UpdateConnections() of the keyframes update_slot[0 .. n_update) (a DEVICE array, n_update <= 32; a longer
 * list is the caller's to split, the state persists) one after the other in that order.  `table` gives n_rows and bad; nothing else is read.
 *   Valid members.  A = update_slot[i] is processed when it is usable and its point run is valid.  A slot that occurred earlier in the list is
 *     skipped and counted (the caller lists a slot once).
 *   rows(A): the rows r of A's run with 0 <= r < n_rows and bad[r] == 0 (:306-314).  A's own `registered` bytes are not read: the reference
 *     walks mvpMapPoints.  STATED DIFFERENCE: a row that A's run lists more than once counts once (the binding lists a row once).
 *   cnt(A, B), for B != A with state[B] != 0 and a valid run: the entries of B's run with registered != 0 (or registered == NULL) whose row is
 *     in rows(A) (:316-323).
 *   K(A) = {B : cnt > 0}.  Empty: the member does nothing at all (:327).
 *   T(A) = the members of K(A) with cnt >= 15; if there are none, the single slot with the largest cnt, the lowest (order_key, slot) among equals
 *     (the first strict maximum of :338-344 and :352-356).
 *   A's own state: conn(A) := K(A) with its counts; ord(A) := T(A) by (weight, order_key, slot) DESCENDING (sort() of pair<int, KeyFrame*>, then
 *     push_front, :358-365).  first_connection[A] set: parent_out[i] = ord(A)[0] and the byte is cleared (:375-380); else parent_out[i] = -1.
 *     AddChild / set_parent / set_children stay with the binding.
 *   A's effect on others: for every B in T(A), AddConnection(A, cnt(A, B)) on B (:127-140): if conn(B) lacks A or holds another weight it is
 *     set and ord(B) becomes ALL of conn(B) sorted as above, entries below the threshold included; if the weight is there already nothing
 *     changes and ord(B) keeps its form - the early return is behaviour.
 *   neighbours: a writable int32[S][10] or NULL - the array jsorb_keyframe_graph.neighbours and the database point at.  Every slot whose ord
 *     list was rewritten gets its row rewritten (the first 10, -1 padded); other rows are untouched.
 *   conn_snapshot (or NULL): slot[n_update][C], weight[n_update][C], len[n_update]: K(update_slot[i]) as the member's own update left it,
 *     before later members touch it - what src/LoopClosing.cpp:560 reads inside its loop.  len = -1 for a member that was skipped or had an
 *     empty K (its map is whatever it was).
 *   Capacity.  T(A) and the AddConnections come from the full K(A).  A stored map keeps the C lowest entries in (order_key, slot) order of the
 *     merge (its base - K of its own update, or its stored map - and the incoming connections); a re-sorted list is that stored map sorted, a
 *     member's own list the first C of T(A).  counts says how many slots overflowed.  Past capacity the result is defined and deterministic
 *     (tests/covis_cases.py restates it), no longer the reference's.
 *   counts_dev[8] = the members processed, skipped (unusable, invalid run, repeated), empty (K empty), the AddConnection calls (the sum of
 *     |T(A)|), the slots whose list ends as a full re-sort, the members that took the fallback, the slots whose merge exceeded C, 0.
 * Enqueued on the matcher's stream, no host decision after the argument checks, launch shapes from S, n_update and C alone, capturable once the
 * scratch has its size (a call with the same or larger S and n_rows has run); the call does not synchronise.  Five kernels: k_cv_marks,
 * k_cv_counts, k_cv_select, k_cv_apply, k_cv_reset.  The scratch is one word per table row, all zero between calls (every call sets back the
 * words it touched), and 128 words per slot.  Every slot, row and run read from device memory is range-checked before anything is read through it.
 * JSORB_ERR_INVALID: NULL graph, table, cov or counts_dev; a NULL graph array (other than registered, neighbours, the child arrays, parent and
 * the pool of 0 entries) or covisibility array with S > 0; cov->max_keyframes != graph->max_keyframes; conn_capacity outside the build caps;
 * n_update outside [0, 32]; update_slot NULL with n_update > 0; table->bad NULL with n_rows > 0; a snapshot with a NULL array; a negative size;
 * S >= 2^24. */
typedef struct jsorb_covisibility {
    int max_keyframes, conn_capacity;
    int32_t *conn_len, *conn_slot, *conn_weight, *ord_len, *ord_slot, *ord_weight;
    uint8_t *first_connection;
} jsorb_covisibility;
typedef struct jsorb_conn_snapshot {
    int32_t *slot, *weight, *len;
} jsorb_conn_snapshot;
int jsorb_update_connections_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                                   const jsorb_covisibility *cov, int n_update, const int32_t *update_slot, int32_t *neighbours, int32_t *parent_out,
                                   const jsorb_conn_snapshot *conn_snapshot, int32_t *counts_dev);
/* Synchronous: the same, then parent_host[n_update] (may be NULL when parent_out is) and counts_host[8] in one copy back. */
int jsorb_update_connections(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                             const jsorb_covisibility *cov, int n_update, const int32_t *update_slot, int32_t *neighbours, int32_t *parent_out,
                             const jsorb_conn_snapshot *conn_snapshot, int32_t *counts_dev, int32_t *parent_host, int32_t counts_host[8]);
/* Diagnostics of the last jsorb_update_connections* (waits for it): counts_dev's first seven words.  JSORB_ERR_STATE before the first call.
 * Any pointer may be NULL. */
int jsorb_update_connections_stats(jsorb_keyframe_matcher *m, int *n_processed, int *n_skipped, int *n_empty, int *n_add_connection, int *n_resorted,
                                   int *n_fallback, int *n_overflow);
/* The row words of the matcher's scratch (waits for the last call): how many there are and how many are not zero - 0 between calls.  For tests.
 * JSORB_ERR_STATE before the first call. */
int jsorb_update_connections_scratch(jsorb_keyframe_matcher *m, int *n_words, int *n_nonzero);
/* SetBadFlag's :470-471 and :480-481 for `slot` (a host int in [0, S)): for every key B of the slot's map, if conn(B) holds the slot it is
 * erased from it and ord(B) becomes the whole of conn(B) re-sorted, with its neighbours row (EraseConnection, :557-571); a keyframe whose map
 * did not hold the slot is left alone, lists included.  Afterwards the slot's own map and lists are empty and its neighbours row is -1.
 * graph gives order_key only.  counts_dev[2] = the keys walked, the maps that held the slot.  Two kernels: k_cv_erase, k_cv_erase_clear.  This
 * entry repairs no spanning tree (:483-541): jsorb_cull_keyframes_async below runs the whole of SetBadFlag, the repair of parent[] included, for
 * the keyframes it culls; a caller that erases a keyframe for another reason repairs the tree over jsorb_covisibility_copy. */
int jsorb_erase_connections_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_covisibility *cov, int slot,
                                  int32_t *neighbours, int32_t *counts_dev);
/* GetConnectedKeyFrames() (:163-170) of `slot` as the byte per slot that jsorb_detect_loop_candidates takes: mask[S], DEVICE. */
int jsorb_connected_mask_async(jsorb_keyframe_matcher *m, const jsorb_covisibility *cov, int slot, uint8_t *mask);
/* GetBestCovisibilityKeyFrames(N) (:178-186) of slots[0 .. n) (DEVICE): out[n*N] -1 padded, out_len[n] (or NULL); an unusable slot gives an
 * empty list. */
int jsorb_best_covisibles_async(jsorb_keyframe_matcher *m, const jsorb_covisibility *cov, int n, const int32_t *slots, int N, int32_t *out,
                                int32_t *out_len);
/* One slot's map and ordered lists to the host, behind everything the device has been given (it waits for the device): lens[2] = {conn_len,
 * ord_len}, the four arrays C entries each (any may be NULL).  GetVectorCovisibleKeyFrames / GetWeight for the spanning-tree repair. */
int jsorb_covisibility_copy(const jsorb_covisibility *cov, int slot, int32_t lens[2], int32_t *conn_slot, int32_t *conn_weight, int32_t *ord_slot,
                            int32_t *ord_weight);
/* The compile-time bounds on conn_capacity of the library in use (16 and 2048: a map of C entries and 32 incoming ones are sorted in one
 * workgroup's LDS). */
int jsorb_covisibility_build_caps(int *min_capacity, int *max_capacity);

/* ---- culling redundant keyframes on the device: LocalMapping::KeyFrameCulling (src/LocalMapping.cpp:638-702) with KeyFrame::SetBadFlag
 * (src/KeyFrame.cpp:457-549) and MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cpp:142-168, :182-199), on a keyframe matcher ----
 * The candidates cand_slot[0 .. n_cand) (a DEVICE array, n_cand a host count) are what jsorb_best_covisibles_async(cov, {current}, N =
 * conn_capacity) wrote BEFORE the call - the reference's copy of GetVectorCovisibleKeyFrames() (:644).  They are processed one after the other
 * in that order, and a culled keyframe's SetBadFlag is complete before the next candidate is examined: it can take a later candidate below
 * three qualifying observers, and it can turn rows bad, which lowers a later candidate's n_mps and pushes it over 0.9.
 * jsorb_keyframe_views holds DEVICE arrays parallel to graph->point_pool (pool_entries entries): octave = mvKeysUn[i].octave, stereo =
 * mvuRight[i] >= 0, depth = mvDepth[i] (or NULL), and th_depth[S] = mThDepth per slot (read only with depth).  monocular != 0 turns the depth
 * test off: depth is not read and may be NULL.
 * jsorb_culling_state holds the arrays the call WRITES: the same device arrays graph->state, registered, point_pool, parent and table->bad
 * point at, handed over once more as writable pointers (another address is JSORB_ERR_INVALID), and not_erase[S] = mbNotErase (or NULL = none),
 * to_be_erased[S] = mbToBeErased (NULL only with not_erase NULL), ref_slot[n_rows] = the slot of mpRefKF (or NULL).
 * The definitions of jsorb_local_keyframes_async hold: USABLE slot, valid run, (order_key, slot) order.
 *   An OBSERVATION of row r is an entry e of the run of a slot B with state[B] == 1, a valid run, point_pool[e] == r, 0 <= r < n_rows,
 *     bad[r] == 0 and registered[e] != 0.  Observations(r) = the sum of 1 + (stereo[e] != 0) over them (nObs, MapPoint.cpp:129-140).
 *     STATED DIFFERENCES: a run that lists a row twice makes two observations (the binding lists a row once); nObs is recomputed from the
 *     observations, not stored - the two are equal wherever AddObservation / EraseObservation can reach.
 *   Candidate A = cand_slot[i]:
 *   1. SKIPPED (decision 3): not usable (-1 padding included), state != 1, an invalid run, A == first_slot (mnId == 0, :649; -1 = none), or a
 *      slot that occurred earlier in the list.
 *   2. over the entries e of A's run whose row r is in range with bad[r] == 0, registered or not (:657-662 walks mvpMapPoints): unless monocular
 *      the entry is dropped when depth[e] > th_depth[A] || depth[e] < 0 in float (:666; depth == th_depth, -0.0f and a NaN pass); n_mps++; if
 *      Observations(r) > 3, q = the observations of r in slots other than A with octave[e'] <= octave[e] + 1 (:671-689); q >= 3: n_redundant++.
 *   3. CULLED if (double)n_redundant > 0.9 * (double)n_mps (:699); n_mps == 0 is not culled.
 *   4. kept: decision 0, nothing changes.
 *   5. culled with not_erase[A] != 0: decision 2, to_be_erased[A] = 1, nothing else changes (:463-467).
 *   6. otherwise decision 1: EraseConnection on every key of conn(A) exactly as jsorb_erase_connections_async does it, the neighbours rows of
 *      the rewritten lists, conn(A) and ord(A) emptied and A's neighbours row -1 (:470-471, :480-481).
 *   7. for every observation e of A with row r (:473-475): registered[e] = 0; if ref_slot[r] == A it becomes the observer of r lowest in
 *      (order_key, slot) among those left, -1 if none is (MapPoint.cpp:157-158); if Observations(r) <= 2 afterwards bad[r] = 1 and every remaining
 *      observation e' of r gets point_pool[e'] = -1 and registered[e'] = 0 (EraseMapPointMatch, :182-199).  A's own point_pool[e] stays r.
 *   8. state[A] = 2.
 *   9. the spanning tree (:483-541) in parent[] only.  Ch = the slots with parent == A and state != 0 in (order_key, slot) order; P =
 *      {parent[A]} if that slot is usable, else empty.  Repeat: over the members c of Ch with state[c] == 1 in order, over the entries j of
 *      ord(c) in list order, whenever ord_slot(c)[j] is in P take w = its weight in conn(c), 0 when conn(c) lacks it (GetWeight); the FIRST pair
 *      (c, p) whose w is strictly greater than every earlier one (and than -1) wins: parent[c] = p, c joins P and leaves Ch.  Stop when a pass
 *      finds nothing or Ch is empty; every slot left in Ch, bad ones included, gets parent = parent[A].  Each assignment is appended to
 *      reparent_out[reparent_cap][2] = (child, new parent) in the order it is made.  parent[A] is kept.  STATED DIFFERENCE: Ch is read from
 *      parent[], so a keyframe culled earlier stays a child of its parent (the reference's EraseChild, :541, has removed it) and is handed on
 *      by the fallback.  The child runs (child_off / child_len / child_pool) and mTcp stay with the binding.
 *   10. after the max_cull-th decision 1 the call stops: later candidates keep decision -1, and the state is the reference's at that point of
 *      its loop.  A second call with cand_slot + next and n_cand - next continues (the caller passes first_slot again; a slot decided in the
 *      earlier call is no longer state 1 when culled, and the reference's list holds a slot once).
 * Outputs (DEVICE): decision[n_cand] (-1 not reached, 0 kept, 1 culled, 2 deferred, 3 skipped), n_mps[n_cand] and n_redundant[n_cand] as seen at
 * the candidate's turn (0 where skipped or not reached), culled_slot[max_cull] -1 padded, reparent_out -1 padded, counts_dev[10] = next (the
 * first candidate not decided), kept, culled, deferred, skipped, rows turned bad, observations erased, ref_slot entries moved, reparent records
 * (all of them), 1 when they exceeded reparent_cap (the parent[] writes are complete regardless; the log is a prefix).
 * Enqueued on the matcher's stream, no host decision after the argument checks, launch shapes from S, n_rows, n_cand, max_cull and C
 * alone, capturable once the scratch has its size (a call with the same or larger sizes has run); the call does not synchronise.
 * The observations are grouped by row once (k_kc_count, k_kc_scan_blocks, k_kc_scan_top, k_kc_scatter), then max_cull rounds of k_kc_eval (a
 * workgroup per undecided candidate on the current state), k_kc_pick (the first cull at or behind the cursor; every decision before it is final),
 * k_cv_erase_dev and k_kc_apply (steps 6-9 for that slot).  Order comes from the launches alone.  The scratch is the call's own: the row words of
 * jsorb_update_connections_async are not touched, and the two calls follow each other on one matcher in either order.
 * JSORB_ERR_INVALID: NULL graph, table, cov, views, state, an output or counts_dev; a NULL graph array (other than neighbours and the child
 * arrays) or covisibility array with S > 0; graph->registered NULL (the call writes those bytes); a state array that is not the graph's or the
 * table's; views->octave or stereo NULL with pool_entries > 0; views->pool_entries != graph->pool_entries; monocular == 0 with depth or
 * th_depth NULL; to_be_erased NULL with not_erase given; cov->max_keyframes != graph->max_keyframes; conn_capacity outside the build caps;
 * max_cull outside [1, 16]; n_cand < 0 or above jsorb_cull_keyframes_build_caps (4096); cand_slot NULL with n_cand > 0; reparent_cap < 0 or
 * reparent_out NULL with reparent_cap > 0; first_slot outside [-1, S); table->bad NULL with n_rows > 0; a negative size; S >= 2^24. */
typedef struct jsorb_keyframe_views {
    int pool_entries;
    const uint8_t *octave, *stereo;
    const float *depth, *th_depth;
} jsorb_keyframe_views;
typedef struct jsorb_culling_state {
    uint8_t *state, *registered, *bad;
    int32_t *point_pool, *parent;
    const uint8_t *not_erase;
    uint8_t *to_be_erased;
    int32_t *ref_slot;
} jsorb_culling_state;
int jsorb_cull_keyframes_async(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                               const jsorb_covisibility *cov, const jsorb_keyframe_views *views, const jsorb_culling_state *state, int monocular,
                               int first_slot, int n_cand, const int32_t *cand_slot, int max_cull, int32_t *neighbours, int reparent_cap,
                               int32_t *decision, int32_t *n_mps, int32_t *n_redundant, int32_t *culled_slot, int32_t *reparent_out,
                               int32_t *counts_dev);
/* Synchronous: the same, then the outputs and the counts in one copy back (host arrays of the same sizes; reparent_host may be NULL when
 * reparent_cap is 0). */
int jsorb_cull_keyframes(jsorb_keyframe_matcher *m, const jsorb_keyframe_graph *graph, const jsorb_map_point_table *table,
                         const jsorb_covisibility *cov, const jsorb_keyframe_views *views, const jsorb_culling_state *state, int monocular,
                         int first_slot, int n_cand, const int32_t *cand_slot, int max_cull, int32_t *neighbours, int reparent_cap, int32_t *decision,
                         int32_t *n_mps, int32_t *n_redundant, int32_t *culled_slot, int32_t *reparent_out, int32_t *counts_dev,
                         int32_t *decision_host, int32_t *n_mps_host, int32_t *n_redundant_host, int32_t *culled_slot_host, int32_t *reparent_host,
                         int32_t counts_host[10]);
/* The counts of the last jsorb_cull_keyframes* (waits for it): counts[10] as above.  JSORB_ERR_STATE before the first call. */
int jsorb_cull_keyframes_stats(jsorb_keyframe_matcher *m, int32_t counts[10]);
/* The compile-time caps of the library in use: the candidates of one call (4096, twice the largest conn_capacity) and max_cull (16). */
int jsorb_cull_keyframes_build_caps(int *max_candidates, int *max_cull);

/* ---- Fuse applied to the map on the device: ORBmatcher::Fuse(pKF, vpMapPoints, th) WITH its tail (src/ORBmatcher.cpp:812-962) as
 * LocalMapping::SearchInNeighbors runs it (src/LocalMapping.cpp:490-531), and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:964-1087) with the
 * Replace loop of LoopClosing::SearchAndFuse (src/LoopClosing.cpp:596-617), over the state the calls above keep - the graph's point_pool and
 * registered, the table's bad and desc - for ALL target keyframes in one call on the keyframe matcher's stream, in the reference's order: keyframe
 * t is searched from the map as it is then, its tail runs, then keyframe t + 1 (tests/fuse_replay.py, mode "sequential").  No host decision between
 * the argument checks and the result.  params->check_reprojection picks the overload as for jsorb_fuse: 1 the first, 0 the one with Scw (Rcw, tcw,
 * Ow derived from it, :967-974); replace_loop is read only with 0.
 * The definitions of jsorb_local_keyframes_async and jsorb_cull_keyframes_async hold: USABLE slot, valid run, (order_key, slot) order.  kp: DEVICE
 * arrays parallel to graph->point_pool (a keypoint's index within its keyframe is its index within the run).  The keyframe of target t is the run
 * point_off[A], point_len[A] of A = target_slot[t], read on the device.  An ENTRY OF ROW r is an entry e with point_pool[e] == r, registered[e] != 0,
 * 0 <= r < n_rows, in a valid run of a slot with state != 0 (an entry inside two overlapping runs belongs to one of them); it is an OBSERVATION
 * when that slot has state == 1.  Observations(r) = the sum of 1 + (uright[e] >= 0) over the observations (uright NULL: 1 each), recomputed, not
 * stored.  list_row (DEVICE) int32[n_list]: the points' rows, -1 = NULL.  target_slot, Rcw, tcw, Ow: HOST arrays per target as for jsorb_fuse.
 * Per target t, in order:
 *   0. A not usable, state[A] != 1, an invalid run or one of 262144 entries or more: n_fused[t] = 0, row t of best_idx, best_dist and replace_point is
 *      -1, the target is counted, nothing else happens.
 *   1. Overload 2: the snapshot = the rows in A's run that are in range and not bad at this moment (:980).
 *   2. Every list point whose head test (below) passes at this moment is searched in A with the arithmetic of jsorb_fuse_async items 1-10 over the
 *      table's fields as they are now, desc included; every other pair gets -1 / -1.
 *   3. i = 0 .. n_list-1 in order, r = list_row[i].  The head test, evaluated at i's turn: r in [0, n_rows), bad[r] == 0, and - overload 1 - r has no
 *      observation in A (IsInKeyFrame, :835), - overload 2 - r not in the snapshot (:992).  Failed, or best_idx[t][i] < 0: the next point.
 *      Otherwise e = point_off[A] + best_idx[t][i], q = point_pool[e], n_fused[t] += 1 and
 *        q outside [-1, n_rows): the pair is dropped and counted (the reference would read through the pointer)
 *        q == -1: point_pool[e] = r, registered[e] = 1 (AddObservation, AddMapPoint), logged as (3, r, A, best_idx)
 *        overload 1, q >= 0 (:941-956): bad[q] != 0: nothing; else Observations(q) > Observations(r): Replace(r -> q); else Replace(q -> r)
 *        overload 2, q >= 0 (:1071-1081): replace_point[t][i] = q when bad[q] == 0 (else it stays -1)
 *   4. Overload 2 with replace_loop: for i in order with replace_point[t][i] >= 0, Replace(replace_point[t][i] -> list_row[i]).
 *   5. Every row that was the target q of a Replace in 3-4, is not bad now and has an observation gets desc[q] = ComputeDistinctiveDescriptors by
 *      rules 1-5 of jsorb_distinctive_descriptors_async over its observations in (order_key, slot) order, from kp->desc.  (The reference does this
 *      inside every Replace; within one target the set at the end is the set at q's last Replace, and nothing reads the descriptor in between:
 *      tests/test_fuse_apply_host.py holds this against the immediate recomputation.)
 *   Replace(p -> q) (src/MapPoint.cpp:208-246): nothing when p == q.  Otherwise every entry e of p, in slot B: q has no entry in B (as the map is
 *   before this Replace): point_pool[e] = q; it has one: point_pool[e] = -1, registered[e] = 0.  Then bad[p] = 1, replaced[p] = q, found[q] +=
 *   found[p], visible[q] += visible[p], logged as (2, p, q, -1).  Entries that hold p with registered == 0 stay as they are.  (Entries in slots of
 *   state 2 move with the others, as mObservations keeps a bad keyframe until it erases itself; they count for neither Observations() nor step 5.)
 * state: what the call WRITES - point_pool, registered (the graph's arrays), bad, desc (the table's), handed over writable: another address is
 * JSORB_ERR_INVALID, as for jsorb_culling_state; replaced int32[n_rows] (mpReplaced as a row; may be NULL); visible, found int32[n_rows] (both NULL
 * or both given).
 * Outputs (DEVICE): best_idx, best_dist int32[n_targets x n_list], every entry written; replace_point int32[n_targets x n_list] (needed for overload 2,
 * else may be NULL: when given every entry is written); n_fused int32[n_targets]; log_out int32[log_cap][4], -1 padded: the events in the order they
 * are made, codes 2 and 3 above - the map writes are complete whatever log_cap is; counts_dev int32[10] = fused, Replace calls, AddMapPoint calls,
 * matches whose slot held a bad point, rows turned bad, descriptors written with other bytes, skipped targets, dropped pairs, log records made, 1
 * when they exceed log_cap.
 * What stays on the host: Map::EraseMapPoint and the host objects' mirrors (from log_out and replaced), UpdateNormalAndDepth
 * (jsorb_map_points_scatter_async), the candidate list of SearchInNeighbors' second direction (LocalMapping.cpp:498-516).
 * Enqueued on the matcher's stream, launch shapes from the host sizes alone, no synchronisation, capturable once the scratch has its size.
 * JSORB_ERR_INVALID for a NULL required pointer, the parameter limits of jsorb_fuse_async, negative sizes, n_targets outside [0, 256],
 * kp->pool_entries != graph->pool_entries, a state array that is not the graph's or the table's, graph->registered NULL, kp->desc or the table's desc
 * not 16-byte aligned, visible without found or the reverse, overload 2 without replace_point; JSORB_ERR_UNSUPPORTED when n_targets x n_list exceeds
 * INT_MAX - 256.  n_list == 0 and n_targets == 0 are valid calls. */
typedef struct jsorb_keyframe_keypoints {   /* DEVICE arrays parallel to graph->point_pool */
    int pool_entries;
    const float *x, *y;                     /* mvKeysUn */
    const int32_t *octave;
    const float *uright;                    /* mvuRight; NULL: monocular everywhere */
    const uint8_t *desc;                    /* pool_entries x 32, 16-byte aligned */
} jsorb_keyframe_keypoints;
typedef struct jsorb_fuse_state {
    int32_t *point_pool;
    uint8_t *registered;
    uint8_t *bad, *desc;
    int32_t *replaced;
    int32_t *visible, *found;
} jsorb_fuse_state;
int jsorb_fuse_map_async(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int replace_loop, const jsorb_keyframe_graph *graph,
                         const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_fuse_state *state, int n_list,
                         const int32_t *list_row, int n_targets, const int32_t *target_slot, const float *Rcw, const float *tcw, const float *Ow,
                         int32_t *best_idx, int32_t *best_dist, int32_t *replace_point, int32_t *n_fused, int log_cap, int32_t *log_out,
                         int32_t *counts_dev);
/* Synchronous: the same, then the outputs in one copy back (host arrays of the same sizes; replace_point_host may be NULL when replace_point is). */
int jsorb_fuse_map(jsorb_keyframe_matcher *m, const jsorb_fuse_params *params, int replace_loop, const jsorb_keyframe_graph *graph,
                   const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_fuse_state *state, int n_list,
                   const int32_t *list_row, int n_targets, const int32_t *target_slot, const float *Rcw, const float *tcw, const float *Ow,
                   int32_t *best_idx, int32_t *best_dist, int32_t *replace_point, int32_t *n_fused, int log_cap, int32_t *log_out, int32_t *counts_dev,
                   int32_t *best_idx_host, int32_t *best_dist_host, int32_t *replace_point_host, int32_t *n_fused_host, int32_t *log_host,
                   int32_t counts_host[10]);
/* The counts of the last jsorb_fuse_map* (waits for it): counts[10] as above.  JSORB_ERR_STATE before the first call. */
int jsorb_fuse_map_stats(jsorb_keyframe_matcher *m, int32_t counts[10]);
/* The compile-time cap of the library in use: the entries of an observation list the applying workgroup stages at a time (256). */
int jsorb_fuse_map_build_caps(int *list_chunk);

/* ---- new map points on the device: the loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:243-457) for ALL given neighbours in one
 * call on the keyframe matcher's stream, over the state the calls above keep: SearchForTriangulation per neighbour, the triangulation of every
 * matched pair with its gates (:297-437), and for every accepted pair new MapPoint, two AddObservation, two AddMapPoint,
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth (:440-450; MapPoint.cpp:37-49, :385-406) - the one step that adds rows to the table.
 * THE NEIGHBOURS ARE NOT INDEPENDENT in the reference: ORBmatcher.cpp:686-690 skips a KF1 keypoint that has a map point, and :445 gives it one as
 * soon as a neighbour triangulates it, so the next neighbour never sees that keypoint.  With check_orientation == 0 (what :221 uses) the dependency
 * has a closed form: a keypoint's best match in neighbour i depends on no other keypoint, a pair's verdict on nothing but the pair, so idx1 belongs
 * to the FIRST neighbour, in list order, whose pair is accepted.
 * The definitions of jsorb_local_keyframes_async hold: USABLE slot, valid run, (order_key, slot) order.  kp: as for jsorb_fuse_map_async, x, y =
 * mvKeysUn.  extra: DEVICE arrays parallel to the pool - node int32 (the mFeatVec node of the keypoint, -1: none), depth (mvDepth), raw_x, raw_y
 * (mvKeys, which KeyFrame::UnprojectStereo reads, KeyFrame.cpp:624-625; NULL: kp->x, kp->y), cos_stereo = cos(2*atan2(mb/2, mvDepth[i])) as the
 * host's libm gives it, computed once when the keyframe is made (the device calls neither cos nor atan2); depth and cos_stereo may be NULL when
 * kp->uright is.  state: what the call WRITES, the graph's and the table's own arrays handed over writable (another address is
 * JSORB_ERR_INVALID), and five optional int32[n_rows] arrays: ref_slot, replaced, visible, found (both or neither), first_kf_id.
 * HOST values: current_slot; n1 = the current keyframe's keypoints (its run's length as the caller knows it); run_capacity = a bound on the
 * neighbours' run lengths; n_neighbours in [0, 256]; neighbour_slot[] in GetBestCovisibilityKeyFrames(nn) order after the caller's baseline tests
 * (:250-267); pose[1 + n_neighbours], the current keyframe first; F12[9 t ..] row-major and epipole[2 t ..] per neighbour as for
 * jsorb_search_for_triangulation_async; params with check_orientation == 0 (else JSORB_ERR_UNSUPPORTED); ratio_factor = 1.5f * mfScaleFactor;
 * current_kf_id = mnId.  new_row: DEVICE int32[row_capacity], the free table rows in the order they are to be used, each listed once.
 *   1. The current keyframe: current_slot usable with state 1, a valid run of exactly n1 entries; otherwise EVERY neighbour is skipped.  Neighbour t
 *      is SKIPPED and counted when its slot is not usable, its state is not 1, its run is invalid or longer than run_capacity, or its slot equals
 *      current_slot (SetBadFlag removes a bad keyframe from every covisibility list: the reference's list holds none).  A slot that an earlier position of
 *      the list holds is skipped too (the reference's list holds a keyframe once).
 *   2. e1 = point_off[current] + idx1, e2 = point_off[neighbour] + idx2.  free(e) is point_pool[e] == -1: a bad row is not free, as GetMapPoint
 *      returns it; any other value is not free either and nothing is read through it.  stereo(e) is uright[e] >= 0 (uright NULL: never).
 *   3. match12[t][idx1] is jsorb_search_for_triangulation_async's over (node, free, stereo, x, y, desc) of the two runs AS THEY ARE AT THE START
 *      OF THE CALL, only_stereo and th_low from params.  A pair whose KF1 octave lies outside [0, n_levels) counts as no match (the reference
 *      would read mvLevelSigma2 out of bounds).
 *   4. The verdict of a pair with a match, the reference's arithmetic in its order.  Float unless said otherwise, every operation rounded on its
 *      own, no fma, divisions and square roots correctly rounded; a float matrix product is summed left to right; norm = sqrtf of the float sum
 *      of squares (as double where the reference multiplies or divides by it); Mat / double and double * Mat go through (float)s; Mat::dot
 *      accumulates (double)a * (double)b left to right from the first product and returns double; .t() is exact.
 *        xn = ((x - cx) * invfx, (y - cy) * invfy, 1); ray = Rwc xn with Rwc = Rcw^T; cosRays = (float)(dot(ray1, ray2) / (norm1 * norm2)) in double
 *        cosS1 = cosS2 = cosRays + 1; stereo(e1): cosS1 = cos_stereo[e1]; ELSE stereo(e2): cosS2 = cos_stereo[e2]; cosS = cosS2 < cosS1 ? cosS2 : cosS1
 *        cosRays < cosS && cosRays > 0 && (stereo(e1) || stereo(e2) || (double)cosRays < 0.9998): PATH 1, the linear triangulation.
 *          A (4x4 float), rows xn1[0]*T1[2] - T1[0], xn1[1]*T1[2] - T1[1], xn2[0]*T2[2] - T2[0], xn2[1]*T2[2] - T2[1] with T = [Rcw | tcw].
 *          cv::SVD::compute is DEFINED here (nothing in the reference pins it): A widened to double; one-sided (Hestenes) Jacobi on its columns,
 *          V from the identity, EIGHT sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  Per pair (p, q), every sum over k = 0..3 from the
 *          first product, left to right: alpha = sum A[k][p]^2, beta = sum A[k][q]^2, gamma = sum A[k][p]*A[k][q]; gamma == 0.0: no rotation;
 *          zeta = (beta - alpha) / (2.0 * gamma); t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta*zeta)); c = 1.0 / sqrt(1.0 + t*t);
 *          s = c * t; for A and then V, k = 0..3: (x[k][p], x[k][q]) = (c*x[k][p] - s*x[k][q], s*x[k][p] + c*x[k][q]).  vt.row(3) = the column j of V
 *          with the smallest sum A[k][j]^2 after the last sweep (j from 0, replaced by a later j whose sum is <=), each entry rounded to float.
 *          Its entry 3 == 0: verdict 4; else x3D = the first three entries, each divided by entry 3 (float).
 *        else stereo(e1) && cosS1 < cosS2: PATH 2, UnprojectStereo(idx1) of the current keyframe; else stereo(e2) && cosS2 < cosS1: PATH 3, of the
 *          neighbour: z = depth[e]; z <= 0 (or NaN): verdict 12; xc = ((raw_x - cx) * z * invfx, (raw_y - cy) * z * invfy, z); x3D = Rwc xc + Ow
 *        else verdict 3 (no stereo and low parallax)
 *        z1 = (float)(dot(Rcw1 row 2, x3D) + (double)tcw1[2]); z1 <= 0: verdict 5.  z2 likewise from the neighbour: verdict 6
 *        x1c, y1c likewise from rows 0 and 1; invz1 = (float)(1.0 / (double)z1); u = fx*x1c*invz1 + cx, v = fy*y1c*invz1 + cy; ex = u - x, ey = v - y;
 *        not stereo(e1): (double)(ex*ex + ey*ey) > 5.991 * (double)level_sigma2[octave1]: verdict 7; stereo(e1): ur = u - mbf*invz1, er = ur - uright,
 *        (double)(ex*ex + ey*ey + er*er) > 7.8 * (double)level_sigma2[octave1]: verdict 7.  The neighbour likewise with its own camera, octave2 and
 *        THE CURRENT KEYFRAME'S mbf (the reference's :412): verdict 8
 *        dist1 = norm(x3D - Ow1), dist2 = norm(x3D - Ow2); either == 0: verdict 9.  ratioDist = dist2 / dist1, ratioOctave = scale_factor[octave1] /
 *        scale_factor[octave2]; ratioDist * ratio_factor < ratioOctave || ratioDist > ratioOctave * ratio_factor: verdict 10.  Otherwise ACCEPTED
 *   5. idx1 goes to the first neighbour in order whose pair is accepted; its pairs (matches) with later neighbours get verdict 2 (taken), path 0
 *      and x3D 0, as the reference never looks at them.
 *   6. The accepted owning pairs are numbered k = 0, 1, .. in (neighbour, ascending idx1) order, the order of :292.  Pair k gets r = new_row[k].
 *      k >= row_capacity or r outside [0, n_rows): verdict 11 (no row), counted and dropped, nothing is written through it - but it still owns its
 *      idx1.  (The reference always has memory for a point: the caller sizes the list.)  Every other one has verdict 1 (created).
 *   7. Per created pair, row r: P = x3D; bad = 0; ref_slot = current_slot, replaced = -1, visible = found = 1, first_kf_id = current_kf_id (where
 *      given); point_pool[e1] = r, registered[e1] = 1, and the same for e2 (8.); desc[r] = rule 4 of jsorb_distinctive_descriptors_async for the two
 *      observations in (order_key, slot) order: kp->desc of whichever of the two keyframes comes first; UpdateNormalAndDepth over the same two in
 *      that order: normal = 0 + n_a / norm(n_a) + n_b / norm(n_b) per component with n_i = P - Ow_i, Pn = normal / 2.0f; dist = norm(P - Ow1);
 *      MaxDistance = dist * scale_factor[octave1]; invariance_maxDistance = 1.2f * MaxDistance; invariance_minDistance = 0.8f * (MaxDistance /
 *      scale_factor[n_levels - 1]).
 *   8. vbMatched2 is never set in the reference, so two created pairs of one neighbour may share idx2; pKF2->AddMapPoint overwrites, so the pair
 *      LATER in order gets point_pool[e2].  The earlier point's fields are what the reference computed at its creation, but it loses its KF2
 *      observation in the pool where the reference's mObservations keeps it: a stated difference, counted (counts[4]).  The rule is an atomicMax
 *      of the pair's position t * n1 + idx1 per (t, idx2): one word per gathered KF2 keypoint, no sort.
 *   9. CheckNewKeyFrames() (:245) cannot be polled from inside a call: the call does all the neighbours it is given.
 * Outputs (DEVICE, every entry written): verdict int32[n_neighbours x n1]: 0 no match, 1 created, 2 taken, 3 low parallax, 4 w == 0, 5 z1 <= 0,
 * 6 z2 <= 0, 7 reprojection in KF1, 8 reprojection in KF2, 9 zero distance, 10 scale ratio, 11 no row, 12 empty unprojection, 13 skipped neighbour;
 * path uint8[n_neighbours x n1]: 0 none, 1 SVD, 2 UnprojectStereo of KF1, 3 of KF2; x3D float[n_neighbours x n1 x 3] (0 where path is 0);
 * log_out int32[log_cap][4], -1 padded: record k = (row or -1 for a pair with no row, idx1, neighbour, idx2) of owning pair k - the map writes are
 * complete whatever log_cap is; counts_dev int32[12] = pairs with a match, accepted pairs (before 5.), owning pairs, created, shared KF2
 * keypoints (8.), pairs with no row, taken, skipped neighbours, 1 when the owning pairs exceed log_cap, pairs on path 1, on paths 2 and 3, 1 when
 * the current keyframe failed 1.
 * Enqueued on the matcher's stream, no host decision after the argument checks, launch shapes from the host sizes alone, capturable once the
 * scratch has its size; every slot, run and row is range-checked before use.  Kernels: k_np_gather, k_bow_group, k_tri_match (as they are),
 * k_np_verdict (16 neighbours' poses per launch), k_np_own, k_np_count, k_np_scan, k_np_write, k_np_link, k_np_finish.
 * JSORB_ERR_INVALID: a NULL required pointer, a state array that is not the graph's or the table's, graph->registered NULL, descriptors not 16-byte
 * aligned, n_neighbours outside [0, 256], kp->pool_entries != graph->pool_entries, depth or cos_stereo NULL while kp->uright is given, visible
 * without found, n_levels, th_low out of range, a negative size, n1 or run_capacity of 262144 or more.  JSORB_ERR_UNSUPPORTED: check_orientation
 * != 0, n_neighbours x max(n1, run_capacity) of 2^24 or more.  n_neighbours == 0 and an empty current run are valid calls. */
typedef struct jsorb_keyframe_pose {
    float Rcw[9], tcw[3], Ow[3];             /* GetRotation (row-major), GetTranslation, GetCameraCenter */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} jsorb_keyframe_pose;
typedef struct jsorb_new_point_keypoints {  /* DEVICE arrays parallel to graph->point_pool */
    const int32_t *node;
    const float *depth, *raw_x, *raw_y, *cos_stereo;
} jsorb_new_point_keypoints;
typedef struct jsorb_new_point_state {
    int32_t *point_pool;
    uint8_t *registered;
    uint8_t *bad, *desc;
    float *Px, *Py, *Pz, *Pnx, *Pny, *Pnz, *MaxDistance, *invariance_maxDistance, *invariance_minDistance;
    int32_t *ref_slot, *replaced, *visible, *found, *first_kf_id;
} jsorb_new_point_state;
int jsorb_create_new_map_points_async(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, const jsorb_keyframe_graph *graph,
                                      const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_new_point_keypoints *extra,
                                      const jsorb_new_point_state *state, int current_slot, int n1, int run_capacity, int n_neighbours,
                                      const int32_t *neighbour_slot, const jsorb_keyframe_pose *pose, const float *F12, const float *epipole,
                                      float ratio_factor, int current_kf_id, int row_capacity, const int32_t *new_row, int log_cap, int32_t *verdict,
                                      uint8_t *path, float *x3D, int32_t *log_out, int32_t *counts_dev);
/* Synchronous: the same, then the outputs in one wait (host arrays of the same sizes). */
int jsorb_create_new_map_points(jsorb_keyframe_matcher *m, const jsorb_triangulation_params *params, const jsorb_keyframe_graph *graph,
                                const jsorb_map_point_table *table, const jsorb_keyframe_keypoints *kp, const jsorb_new_point_keypoints *extra,
                                const jsorb_new_point_state *state, int current_slot, int n1, int run_capacity, int n_neighbours,
                                const int32_t *neighbour_slot, const jsorb_keyframe_pose *pose, const float *F12, const float *epipole,
                                float ratio_factor, int current_kf_id, int row_capacity, const int32_t *new_row, int log_cap, int32_t *verdict,
                                uint8_t *path, float *x3D, int32_t *log_out, int32_t *counts_dev, int32_t *verdict_host, uint8_t *path_host,
                                float *x3D_host, int32_t *log_host, int32_t counts_host[12]);
/* The counts of the last jsorb_create_new_map_points* (waits for it): counts[12] as above.  JSORB_ERR_STATE before the first call. */
int jsorb_create_new_map_points_stats(jsorb_keyframe_matcher *m, int32_t counts[12]);
/* The compile-time cap of the library in use: pairs per chunk of the order-preserving compaction (1024). */
int jsorb_create_new_map_points_build_caps(int *scan_chunk);

/* ---- the keyframe database: KeyFrameDatabase (src/KeyFrameDatabase.cpp:44-313) with DBoW2's BowVector fold (BowVector.cpp:34-84 as
 * TemplatedVocabulary.h:1148-1193 drives it) and L1Scoring::score (ScoringObject.cpp:23-68), for the ORB vocabulary's combination only: TF-IDF
 * weights, L1 norm, L1 score.  An object of its own like the keyframe matcher: its stream, its scratch, its error text; whoever creates none
 * allocates and launches nothing.  Everything is enqueued on the database's stream with no host decision between kernels (capturable); the
 * calls of one database must not run concurrently on the host.
 *   1. A BowVector on the device is three arrays: `word` int32 (distinct word ids ascending - std::map's order), `value` double, and a device
 *      count.  Every reader clamps the count to [0, cap], the arrays' capacity (a host value).
 *   2. jsorb_bow_vector_async: n word ids at a DEVICE pointer (for a frame: jsorb_bow_word_device; n known on the host) -> bow_word / bow_value of
 *      capacity n and *bow_n_dev.  An id outside [0, n_words) or whose word_weight is not > 0 contributes nothing (:1157).  A word with c
 *      occurrences has the value w added to itself c - 1 times in sequence (BowVector::addWeight; NOT c * w); BowVector::normalize(L1): norm =
 *      the sequential double sum of fabs(value) in ascending word order from 0.0, and when norm > 0.0 every value becomes value / norm (IEEE
 *      division).  The result has the host's bits.  n = 0 writes the count 0 and launches nothing that reads.
 *   3. A keyframe is a caller-chosen slot in [0, max_keyframes).  add copies a device BowVector of at most `cap` entries into the database's own
 *      pool (the count is read on the device), marks the slot present, gives it the next add sequence number and the KeyFrame constructor's query
 *      state (KeyFrame.cpp:39): loop_query = reloc_query = 0, loop_words = reloc_words = 0 - and loop_score = reloc_score = 0.0f, which the
 *      reference leaves uninitialised.  Adding to a present slot is JSORB_ERR_INVALID.  The pool may grow in add (which then waits for the
 *      stream); no query allocates.  erase marks the slot absent (an absent slot: nothing); a later add of it is a new keyframe with fresh state
 *      and a new sequence number.  clear empties all slots.  JSORB_ERR_UNSUPPORTED after 2^32 - 1 adds since the last clear.
 *   4. No inverted file: the reference's lists are appended in add order and erase keeps the others' order, so a keyframe's position in
 *      lKFsSharingWords is the ascending order of the key (its lowest word id in common with the query, its add sequence number).
 *   5. score (the minScore loop, LoopClosing.cpp:129-143): for each entry of the DEVICE list `slots` that is present, score_f64 = L1Scoring::score:
 *      over the words of both vectors in ascending word order s += fabs(vi - wi) - fabs(vi) - fabs(wi) from 0.0 in double, then -s / 2.0; score =
 *      its cast to float; *min_score_dev = the minimum from 1.0f with `<`.  An absent (or out-of-range) slot is skipped like an isBad()
 *      keyframe: its outputs are -1.  score_f64 may be NULL.
 *   6. The two queries.  query_id is pKF->mnId / F->mnId.  neighbours: DEVICE int32 [max_keyframes x 10], row s = GetBestCovisibilityKeyFrames(10)
 *      of slot s in its order; -1 pads and stands for a keyframe that is not in the database.  Loop form: connected = a DEVICE byte per slot
 *      (spConnectedKeyFrames.count) or NULL; min_score is the host value unless min_score_dev, a DEVICE pointer, is given (5.'s output: no wait
 *      in between).  candidates: DEVICE int32 of capacity max_keyframes, the slots in the reference's output order; *n_candidates_dev their count.
 *      With c = a present slot's count of words in common with the query (c = 0: untouched):
 *        loop (:90-108): loop_query != id and connected: loop_words = 1, not listed; loop_query != id otherwise: loop_query = id, loop_words = c,
 *        listed; else loop_words += c, not listed.  reloc (:211-226): reloc_query != id: reloc_query = id, reloc_words = c, listed; else
 *        reloc_words += c, not listed.
 *      maxCommonWords over the listed slots; minCommonWords = (int)(maxCommonWords * 0.8f).  A listed slot with words > minCommonWords is scored
 *      as in 5.: si = (float)score into loop_score / reloc_score (nothing else writes these); the loop form keeps si >= min_score.  Per kept
 *      entry in list order: acc = best = si, best slot = the slot; for the neighbours in row order, skipping -1, absent and out-of-range
 *      slots: loop counts a neighbour iff loop_query == id && loop_words > minCommonWords, reloc iff reloc_query == id (no words test: the
 *      reloc_score an earlier query left is read); a counting neighbour adds its score in float and takes over the best slot when its score >
 *      best.  bestAcc from min_score (loop) / 0 (reloc) rises on acc > bestAcc; the entries with acc > 0.75f * bestAcc output their best slot in
 *      list order, a slot once, at its first occurrence.  Empty stages give zero candidates.
 *      The one difference: the reference reads the fields of any KeyFrame* a neighbour list returns; a neighbour outside the database is skipped
 *      here (it matters for query_id == 0, or an erased keyframe still listed as a neighbour, which SetBadFlag prevents).
 *   7. JSORB_ERR_INVALID: a NULL required pointer, a negative size, a slot outside [0, max_keyframes), add to a present slot - with a text in
 *      jsorb_keyframe_database_last_error and nothing launched. ---- */
typedef struct jsorb_keyframe_database jsorb_keyframe_database;
/* word_weight: a HOST array of the n_words leaf weights by word id (copied). */
int jsorb_keyframe_database_create(int device_id, int max_keyframes, int n_words, const double *word_weight, jsorb_keyframe_database **out);
void jsorb_keyframe_database_destroy(jsorb_keyframe_database *db);
int jsorb_keyframe_database_set_stream(jsorb_keyframe_database *db, void *hip_stream);      /* NULL: the database's own */
void *jsorb_keyframe_database_get_stream(const jsorb_keyframe_database *db);
const char *jsorb_keyframe_database_last_error(const jsorb_keyframe_database *db);
int jsorb_keyframe_database_size(const jsorb_keyframe_database *db);                         /* present slots */
int jsorb_bow_vector_async(jsorb_keyframe_database *db, const int32_t *word_id, int n, int32_t *bow_word, double *bow_value, int32_t *bow_n_dev);
int jsorb_keyframe_database_add_async(jsorb_keyframe_database *db, int slot, const int32_t *bow_word, const double *bow_value, int cap,
                                      const int32_t *bow_n_dev);
int jsorb_keyframe_database_erase(jsorb_keyframe_database *db, int slot);
int jsorb_keyframe_database_clear(jsorb_keyframe_database *db);
int jsorb_keyframe_database_score_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                        const int32_t *slots, int n_slots, float *score, double *score_f64, float *min_score_dev);
int jsorb_detect_loop_candidates_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                       uint64_t query_id, const uint8_t *connected, const int32_t *neighbours, float min_score,
                                       const float *min_score_dev, int32_t *candidates, int32_t *n_candidates_dev);
int jsorb_detect_relocalization_candidates_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap,
                                                 const int32_t *q_n_dev, uint64_t query_id, const int32_t *neighbours, int32_t *candidates,
                                                 int32_t *n_candidates_dev);
/* The synchronous forms: the same, then a wait; candidates_host (capacity max_keyframes) and *n_candidates_host are HOST outputs. */
int jsorb_detect_loop_candidates(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                 uint64_t query_id, const uint8_t *connected, const int32_t *neighbours, float min_score, const float *min_score_dev,
                                 int32_t *candidates_host, int *n_candidates_host);
int jsorb_detect_relocalization_candidates(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                           uint64_t query_id, const int32_t *neighbours, int32_t *candidates_host, int *n_candidates_host);
/* Diagnostics of the last query of either form (waits for it): keyframes sharing a word (lKFsSharingWords.size()), maxCommonWords, minCommonWords,
 * keyframes scored (nscores), entries kept by minScore (lScoreAndMatch.size()), bestAccScore (its start value when nothing was kept) and the
 * candidates.  JSORB_ERR_STATE before the first query.  Any pointer may be NULL. */
int jsorb_detect_candidates_stats(jsorb_keyframe_database *db, int *n_sharing, int *max_common_words, int *min_common_words, int *n_scored, int *n_kept,
                                  float *best_acc_score, int *n_candidates);
/* The persistent per-slot state, max_keyframes entries each, into HOST arrays (waits for the stream).  Any pointer may be NULL. */
int jsorb_keyframe_database_copy_state(jsorb_keyframe_database *db, int32_t *present, uint64_t *loop_query, uint64_t *reloc_query, int32_t *loop_words,
                                       int32_t *reloc_words, float *loop_score, float *reloc_score);
/* The compile-time caps of the library in use: query entries the kernels stage in LDS (4096; a longer query is searched in global memory), word
 * ids jsorb_bow_vector_async sorts in LDS (8192).  Any pointer may be NULL. */
int jsorb_kfdb_build_caps(int *query_lds, int *sort_lds);

/* ---- training a vocabulary: TemplatedVocabulary::create(training_features, k, L, weighting, scoring)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996) with FORB::meanValue / FORB::distance (FORB.cpp:28-101) ----
 * Hierarchical k-means++ and Lloyd iterations under the Hamming distance, on the device, one level of the tree at a time.  The result is the
 * tree the reference returns - node order, word ids, weights - as the flat arrays jsorb_vocabulary_create takes.
 * Input: `descriptors` n x 32 bytes at a DEVICE pointer, 16-byte aligned: DBoW2's `features` in the order of getFeatures (:620-637), the documents
 *   concatenated.  doc_start: a HOST array of n_docs + 1 ascending offsets, doc_start[0] = 0, doc_start[n_docs] = n (document i is
 *   training_features[i]; it matters only for the weights).  weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring 0..5 (kept for the text file).
 * JSORB_ERR_INVALID (nothing is launched): n = 0 (the reference leaves only the root, jsorb_vocabulary_create needs two nodes), n < 0 or
 *   n > 2^30; k outside [2, 32]; depth_L outside [1, 16]; 1 + k + ... + k^depth_L beyond 2^31 - 1 (the reference's expected_nodes, :565);
 *   weighting outside [0, 3], scoring outside [0, 5]; n_docs < 1, offsets that are not ascending from 0, doc_start[n_docs] != n; max_iterations < 0;
 *   a NULL or misaligned pointer.
 * One k-means run (HKmeansStep, :641-819) works on a node's descriptors, always a subsequence of the input in ascending input order (:749):
 *   trivial (:660-670)  at most k descriptors: one cluster per descriptor, no draw
 *   seeding (:832-913)  the first centre is RandomInt(0, size - 1); then, until k centres exist, min_dists is lowered by the last centre
 *                       (:872-880), dist_sum is their sum - at 0 the seeding ends with fewer than k centres (:908) -, cut_d =
 *                       RandomValue<double>(0, dist_sum) is drawn again while it is 0.0, and the next centre is the first index whose running sum is
 *                       >= cut_d (the last feature when none is, :893-903).  The distances are integers and the sums stay below 2^53: every sum
 *                       is exact in any order, and `running >= cut_d` is `running >= ceil(cut_d)` in integers
 *   association (:732-751)  the nearest centre, the first of equals (strict <)
 *   means (FORB::meanValue)  bit set iff its count >= N / 2 + N % 2; N = 1 copies the member.  N = 0 is undefined in the reference (the mean is
 *                       released and the next distance reads through a null pointer): here the cluster keeps its previous centre
 *   end (:755-779)      when a pass leaves every association as it was.  A converged run is a fixed point, so all runs of a level iterate
 *                       together until none moves; the runs that had converged earlier stay what they were
 * Random draws.  The reference calls rand() (seeded from the clock) in depth-first order; here the j-th 31-bit value a run consumes (j = 0, 1, ...,
 *   the redraws included) is a function of the seed, the input index `first` of the run's first descriptor, the run's size and j:
 *       mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31
 *       r = mix(mix(seed ^ ((uint64)first << 32 | size)) + j) >> 33
 *   with the reference's formulas and RAND_MAX = 2^31 - 1: RandomInt(0, size - 1) = int(((double)r / 2147483648.0) * size) (Random.cpp:47-50),
 *   RandomValue<double>(0, s) = ((double)r / 2147483647.0) * s (Random.h:55-69).
 * The tree.  A run's clusters become consecutive nodes (:785-793); the recursion goes on only below level depth_L and only into children with more
 *   than one descriptor, in child order (:796-818): node ids are depth-first by blocks of siblings, word ids the leaves in id order (:917-938).
 * Weights (:942-996).  Ni[w]: the documents with at least one descriptor whose transform (:1217-1259, jsorb_bow_transform_descriptors on the
 *   finished tree) ends in word w - computed for every weighting.  TF_IDF and IDF: weight = log((double)n_docs / (double)Ni) with the host's libm,
 *   0 where Ni = 0; TF and BINARY: 1.  Inner nodes: weight 0, Ni 0.
 * max_iterations: the reference loops for ever when Lloyd cycles.  Here a level ends after max_iterations association passes (0: 1000); the runs a
 *   descriptor of which moved in the last pass are counted in n_unconverged, their nodes are the centres that pass measured against, their
 *   children's members that pass's association.  The status stays JSORB_OK.
 * Synchronous: the work is enqueued on hip_stream (a hipStream_t on the device, NULL: the null stream) and waited for; the host reads one word
 *   per association pass, and per level the centres and member counts of the level's runs.  Nothing faults on any content of `descriptors`.
 * The result is a host object.  copy: parent int32[n_nodes] (parent[0] = -1), child_start int32[n_nodes + 1], children int32[n_nodes - 1],
 *   descriptors uint8[n_nodes x 32] (row 0 zero), word_id int32[n_nodes] (-1 for inner nodes), weight double[n_nodes], Ni int32[n_nodes]; any
 *   pointer may be NULL.  copy_assignment: per input descriptor the node its path of associations ended in (a leaf), int32[n].
 * stats: k-means runs (the runs that seeded: more than k descriptors), draws consumed, clusters of those runs without a member in the last pass,
 *   n_unconverged, and the association passes per level (lloyd_passes[16], 0 for a level without a seeded run). */
typedef struct jsorb_vocab_train_result jsorb_vocab_train_result;
int jsorb_vocabulary_train(int device_id, void *hip_stream, const uint8_t *descriptors, int n, const int32_t *doc_start, int n_docs, int k, int depth_L,
                           int weighting, int scoring, uint64_t seed, int max_iterations, jsorb_vocab_train_result **out);
const char *jsorb_vocabulary_train_last_error(void);                 /* text of the last failed jsorb_vocabulary_train of this thread */
void jsorb_vocab_train_result_destroy(jsorb_vocab_train_result *r);
int jsorb_vocab_train_result_info(const jsorb_vocab_train_result *r, int *n_nodes, int *n_words, int *n, int *k, int *depth_L, int *weighting, int *scoring);
int jsorb_vocab_train_result_copy(const jsorb_vocab_train_result *r, int32_t *parent, int32_t *child_start, int32_t *children, uint8_t *descriptors,
                                  int32_t *word_id, double *weight, int32_t *Ni);
int jsorb_vocab_train_result_copy_assignment(const jsorb_vocab_train_result *r, int32_t *node_of_descriptor);
int jsorb_vocab_train_stats(const jsorb_vocab_train_result *r, int *n_kmeans_runs, long long *n_draws, int *n_empty_clusters, int *n_unconverged,
                            int *lloyd_passes);
/* The compile-time caps of the library in use: positions per chunk of the kernels' chunk sums (1024), chunk sums the scan kernel takes per tile
 * (1024).  Any pointer may be NULL. */
int jsorb_vocab_train_build_caps(int *chunk, int *scan_threads);

/* ---- loop-closure candidates by BoW: ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12)
 * (src/ORBmatcher.cpp:509-642) with ComputeThreeMaxima (:2097-2138), as LoopClosing::ComputeSim3 calls it once per consistent loop candidate with
 * ORBmatcher matcher(0.75, true) (src/LoopClosing.cpp:244, :270) - the current keyframe against ALL candidates in one call of the keyframe matcher
 * above (LoopClosing is a thread of its own and creates its own matcher) ----
 * This is not jsorb_search_by_bow with other arguments: there the many-keyframe side is the ordered outer walk and the single frame is claimed;
 * here the single side (KF1) is the ordered outer walk and each candidate is claimed (vbMatched2), and the threshold comparison is strict.
 * Inputs, DEVICE arrays unless said otherwise.  KF1, the current keyframe, n1 entries: node1 int32 (the FeatureVector node of the keypoint or -1),
 * valid1 uint8 (pMP1 && !pMP1->isBad()), angle1 float (mvKeysUn[].angle), desc1 n1 x 32 bytes, 16-byte aligned.  The candidates are concatenated:
 * candidate i is the entries kf_start[i] .. kf_start[i + 1] (HOST array of n_keyframes + 1 ascending offsets; kf_start[0] need not be 0) of node2,
 * valid2, angle2, desc2.  params: jsorb_bow_params; ComputeSim3 uses nn_ratio 0.75, th_low 50, check_orientation 1.
 * Per candidate, with j local to the candidate:
 *   1. match12[k] = -1 for all k < n1, matched2[j] = false, nmatches = 0 (:521-522)
 *   2. the two facts of jsorb_search_by_bow_async hold: ascending indices within a node, every keypoint in at most one node - so nodes are
 *      independent.  For every node on both sides the KF1 keypoints idx1 of the node are walked in ascending order (:541); skip when !valid1[idx1]
 *   3. walk the candidate's keypoints idx2 of the node in ascending order: skip when matched2[idx2] || !valid2[idx2] (:563-567); from
 *      bestDist1 = bestDist2 = 256, bestIdx2 = -1 the two-smallest rule of :573-582 - a tie with the best lowers the second, the index is the first
 *      in walk order with the minimum
 *   4. claim iff bestDist1 < th_low AND (float)bestDist1 < nn_ratio * (float)bestDist2: the first comparison is STRICT (:585), unlike the <= of
 *      SearchByBoW(KeyFrame*, Frame&) at :215; the second is one float product.  On a claim match12[idx1] = bestIdx2, matched2[bestIdx2] = true,
 *      nmatches++, and with check_orientation idx1 goes into the bin of rot = angle1[idx1] - angle2[bestIdx2] (the arithmetic of
 *      jsorb_search_last_frame).  No entry below 256 (bestIdx2 = -1): no claim, whatever th_low
 *   5. with check_orientation: ComputeThreeMaxima, then every idx1 of every other bin: match12[idx1] = -1, nmatches--.  A bin outside [0, 30) is
 *      never kept.  matched2 is not undone - it is read only inside the loop
 * Outputs (DEVICE): match12 n_keyframes x n1 (row i: candidate i, values local to the candidate), n_matches_dev[n_keyframes].  Enqueued on the
 * matcher's stream, no host decision after the argument checks, no allocation after the first call of a size: k_bow_group (KF1 as the frame
 * side), k_loop_bow_match (one wave per candidate and node), k_tri_resolve.
 * Limits and errors as for jsorb_search_for_triangulation_async: at most 256 candidates, n1 and every candidate below 2^18; JSORB_ERR_INVALID for
 * NULL required pointers, a bad kf_start or misaligned descriptors.  Empty sides write -1 / 0 and launch nothing that reads.  The statistics
 * words and the "done" mark are the call's own: it leaves the triangulation and fuse statistics as they were, and the reverse. */
int jsorb_search_by_bow_kf_async(jsorb_keyframe_matcher *m, const jsorb_bow_params *params, int n1, const int32_t *node1, const uint8_t *valid1,
                                 const float *angle1, const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2,
                                 const uint8_t *valid2, const float *angle2, const uint8_t *desc2, int32_t *match12, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the matcher; match12_host[n_keyframes x n1] and n_matches_host[n_keyframes] (host), one copy back. */
int jsorb_search_by_bow_kf(jsorb_keyframe_matcher *m, const jsorb_bow_params *params, int n1, const int32_t *node1, const uint8_t *valid1,
                           const float *angle1, const uint8_t *desc1, int n_keyframes, const int32_t *kf_start, const int32_t *node2,
                           const uint8_t *valid2, const float *angle2, const uint8_t *desc2, int32_t *match12_host, int *n_matches_host);
/* Diagnostics of the last call (waits for it): n_node_pairs = (candidate, node) pairs present on both sides; n_distances = the Hamming distances
 * step 3 computes; largest_node = the most candidate keypoints in a node of such a pair; kept_bins = candidate 0's ComputeThreeMaxima ind1..3
 * (-1: none, all -1 without check_orientation).  JSORB_ERR_STATE before the first call.  Any pointer may be NULL. */
int jsorb_search_by_bow_kf_stats(jsorb_keyframe_matcher *m, int *n_node_pairs, int *n_distances, int *largest_node, int kept_bins[3]);
/* The compile-time cap of this build's k_loop.hip (no device needed): candidate entries of a node a lane of k_loop_bow_match keeps in registers (2;
 * the entries beyond 64 x that are read again for every KF1 keypoint).  A test build lowers it (jetson_slam_amd/build.py VARIANTS). */
int jsorb_loop_build_caps(int *node_regs);

/* ---- loop-closure matches by projection: ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cpp:1089-1313), as
 * LoopClosing::ComputeSim3 calls it after a successful Sim3Solver (src/LoopClosing.cpp:328, th = 7.5): the map points of each keyframe projected
 * into the other one, a best keypoint per point, and the pairs on which both directions agree ----
 * Both keyframes share the camera and the grid, as in the reference (fx .. cy of pKF1 serve both directions, :1092-1095).  Per side s in {1, 2},
 * n entries aligned with the keyframe's keypoints, slot i = keypoint i and map point vpMapPoints_s[i], DEVICE arrays: x, y (mvKeysUn), octave
 * int32, kp_desc n x 32 bytes; Px, Py, Pz (GetWorldPos), max_distance (mfMaxDistance), min_dist_inv / max_dist_inv (GetMinDistanceInvariance /
 * GetMaxDistanceInvariance), mp_desc n x 32 bytes (GetDescriptor); search uint8 = pMP && !vbAlreadyMatched_s[i] && !pMP->isBad() (:1116-1129,
 * :1139-1143), which the caller evaluates, GetIndexInKeyFrame included, because that is map state.  Both descriptor arrays 16-byte aligned.  In
 * the side struct itself, HOST values copied into the launch arguments: the keyframe's own Rw[9] row-major and tw[3], and the similarity into the
 * OTHER camera sR[9], t[3] (side 1: sR21, t21; side 2: sR12, t12) - the caller computes them from cv::Mat as :1106-1108 does; the library does not
 * redo cv::Mat products whose rounding nothing pins (the rule stated for F12 above).
 * Per searched slot of side 1 into keyframe 2, and symmetrically, in the arithmetic jsorb_fuse_async defines:
 *   1. Pc_own = tw + Rw P, then Pc = t + sR Pc_own, every row in K14's form fma(z,R2,fma(x,R0,y*R1)) + t
 *   2. no candidate unless Pc.z > 0.  That equals the reference, whose own test is z < 0: z == 0 reaches an infinite invz and fails IsInImage, and
 *      so does a NaN
 *   3. invz = 1.0f / Pc.z, u = fma(Pc.x*fx, invz, cx), v likewise
 *   4. KeyFrame::IsInImage, half open: u >= min_x && u < max_x && v >= min_y && v < max_y
 *   5. dist3D = sqrtf(fma(z,z,fma(x,x,y*y))) of Pc: K16's chain with a zero centre
 *   6. no candidate when dist3D < min_dist_inv || dist3D > max_dist_inv (a NaN passes, as written).  There is NO viewing-angle test
 *   7. L = the predicted level of jsorb_fuse_async item 6
 *   8. radius = th * scale_factor[L], one float product
 *   9. KeyFrame::GetFeaturesInArea over the other keyframe's grid: cells, early returns and walk order as jsorb_fuse_async item 7; kept when
 *      |x-u| < radius && |y-v| < radius and octave in [L-1, L] - a plain integer comparison as in :1194, no table is indexed by the octave
 *  10. d = popcount Hamming distance of mp_desc against kp_desc; strict < best in walk order
 *  11. vnMatch = bestIdx iff bestDist <= th_high, else -1 (the reference starts at INT_MAX; for th_high <= 255 that equals starting at 256)
 * Agreement (:1294-1310): match12[i1] = idx2 iff vnMatch1[i1] == idx2 >= 0 && vnMatch2[idx2] == i1, else -1; n_found = their count.  The caller
 * writes vpMatches12[i1] = vpMapPoints2[idx2] where match12[i1] >= 0 and leaves the rest of vpMatches12 alone.
 * Outputs (DEVICE): match1[n1], match2[n2] (the two vnMatch arrays; every entry is written), match12[n1], *n_found_dev.  Enqueued on the matcher's
 * stream, no host decision after the argument checks: k_fuse_grids per keyframe, k_sim3_match (both directions in one launch), k_sim3_agree.
 * Limits: n1 + n2 < 2^18; cols * rows <= 4096; th_high in [0, 255]; n_levels in [1, JSORB_MAX_LEVELS]; JSORB_ERR_INVALID for these, a NULL required
 * pointer or misaligned descriptors.  n1 == 0 or n2 == 0 is valid: everything is -1 / 0.  Statistics and "done" mark are the call's own. */
typedef struct jsorb_sim3_params {
    float th;                        /* 7.5 in LoopClosing::ComputeSim3 */
    int th_high;                     /* ORBmatcher::TH_HIGH = 100; [0, 255] */
    float fx, fy, cx, cy;            /* pKF1->fx .. cy */
    float min_x, max_x, min_y, max_y; /* KeyFrame::mnMinX, mnMaxX, mnMinY, mnMaxY: IsInImage's bounds and the grid origin */
    float inv_w, inv_h;              /* mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* mnGridCols, mnGridRows */
    float log_scale_factor;          /* KeyFrame::mfLogScaleFactor */
    int n_levels;                    /* mnScaleLevels, [1, JSORB_MAX_LEVELS] */
    float scale_factor[JSORB_MAX_LEVELS];        /* mvScaleFactors */
} jsorb_sim3_params;
typedef struct jsorb_sim3_side {
    int n;                           /* keypoints (= map point slots) of the keyframe */
    const float *x, *y;              /* DEVICE from here ... */
    const int32_t *octave;
    const uint8_t *kp_desc;
    const float *Px, *Py, *Pz, *max_distance, *min_dist_inv, *max_dist_inv;
    const uint8_t *mp_desc;
    const uint8_t *search;           /* ... to here */
    float Rw[9], tw[3];              /* HOST: the keyframe's GetRotation (row-major), GetTranslation */
    float sR[9], t[3];               /* HOST: the similarity into the other camera */
} jsorb_sim3_side;
int jsorb_search_by_sim3_async(jsorb_keyframe_matcher *m, const jsorb_sim3_params *params, const jsorb_sim3_side *side1, const jsorb_sim3_side *side2,
                               int32_t *match1, int32_t *match2, int32_t *match12, int32_t *n_found_dev);
/* Synchronous: the same into buffers of the matcher; match1_host[n1], match2_host[n2] (either may be NULL), match12_host[n1] and *n_found (host),
 * one copy back. */
int jsorb_search_by_sim3(jsorb_keyframe_matcher *m, const jsorb_sim3_params *params, const jsorb_sim3_side *side1, const jsorb_sim3_side *side2,
                         int32_t *match1_host, int32_t *match2_host, int32_t *match12_host, int *n_found);
/* Diagnostics of the last call (waits for it): those of jsorb_fuse_stats summed over both directions (slots that reached a window, keypoints of
 * those windows' cells, Hamming distances, the most keypoints in the cells of one window) and n_agree = the agreements.  JSORB_ERR_STATE before
 * the first call.  Any pointer may be NULL. */
int jsorb_search_by_sim3_stats(jsorb_keyframe_matcher *m, int *n_windows, int *n_walked, int *n_distances, int *largest_window, int *n_agree);

/* ---- the loop's acceptance test: ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints,
 * vector<MapPoint*> &vpMatched, int th) (src/ORBmatcher.cpp:277-390), as LoopClosing::ComputeSim3 calls it on the accepted candidate with the map
 * points of the loop keyframe and its neighbours (src/LoopClosing.cpp:380, th = 10) before it counts nTotalMatches against 40 ----
 * The search of one point is that of Fuse(pKF, Scw, ...) (:964-1087, jsorb_fuse_async with check_reprojection = 0).  What is new is state: a
 * keypoint with vpMatched[idx] != NULL is hidden (:362), and a point that matches sets vpMatched[bestIdx] (:383) and so hides that keypoint from
 * every LATER point of the call.  The result is that of the sequential loop.
 * params->th is a float; the reference's is an int converted to float before its one product (:347), so whole numbers behave the same.  Rcw[9]
 * (row-major), tcw[3] and Ow[3] are HOST values in the struct: the caller decomposes Scw as :286-290 does; the library does not redo cv::Mat
 * products whose rounding nothing pins (the rule stated for F12 and for Fuse above).
 * Inputs, DEVICE arrays.  Points i = 0 .. n_points-1 are the points the reference would search, in vpPoints order: the caller drops isBad() points
 * and members of spAlreadyFound (:293-305), which are map state; dropping them changes no order.  Per point Px, Py, Pz (GetWorldPos), Nx, Ny, Nz
 * (GetNormal), max_distance (mfMaxDistance), min_dist_inv / max_dist_inv (GetMinDistanceInvariance / GetMaxDistanceInvariance) float[n_points];
 * desc n_points x 32 bytes (GetDescriptor), 16-byte aligned.  The keyframe, n_keypoints = N entries: x, y (mvKeysUn), octave int32, kf_desc N x 32
 * bytes, 16-byte aligned; blocked uint8[N] = vpMatched[k] != NULL before the call (NULL: nothing is blocked).
 * Per point, in index order, in the arithmetic jsorb_fuse_async defines (its item numbers):
 *   items 1 and 2: K14's projection, no candidate unless Pcz > 0 (the reference's own test is Pcz < 0: Pcz == 0 reaches an infinite invz and fails
 *     IsInImage, and so does a NaN), and KeyFrame::IsInImage, half open
 *   items 4 and 5: K16's distance gate with Ow, and the viewing angle dot < 0.5f*dist; a NaN passes, as written
 *   items 6 and 7: the predicted level, radius = th * scale_factor[L], cells and walk order
 *   there is no ur (item 3) and no chi-square gate
 * then per keypoint k of the window, in walk order, from bestDist = 256:
 *   k is hidden when blocked[k] is set, or when an EARLIER point of this call matched k (:362)
 *   window: that of item 8, fabsf(x[k] - u) < radius && fabsf(y[k] - v) < radius
 *   level: octave[k] in [L-1, L], a plain integer comparison (:367); no table is indexed by the octave
 *   d = popcount Hamming distance; strict < updates bestDist, bestIdx: the first in walk order wins a tie (:374)
 * The point matches iff bestDist <= th_low (:381).  Only a matching point hides its keypoint: one whose best lies above th_low claims nothing.
 * Outputs (DEVICE, every entry written): match_kp[n_points] = the keypoint or -1; match_dist[n_points] = bestDist of a match or -1;
 * kp_match[N] = the point that holds keypoint k after the call or -1 - keypoints blocked before the call stay -1; the caller writes
 * vpMatched[k] = vpPoints[kp_match[k]] where it is >= 0 and leaves the rest alone; *n_matches_dev = the return value.
 * Enqueued on the matcher's stream, no host decision after the argument checks, capturable once the scratch has its size: k_fuse_grids over the
 * one keyframe, k_scw_candidates (per point the keys distance << 18 | walk position of the candidates at or below th_low - no other key can
 * become a match, whatever is hidden), k_scw_resolve (one workgroup: the claim rule as a fixed point).
 * Limits: N < 2^18 = 262144; cols * rows <= 4096; n_levels in [1, JSORB_MAX_LEVELS]; th_low in [0, 255]; JSORB_ERR_INVALID for these, a NULL
 * required pointer, descriptors not 16-byte aligned, a negative n_points.  n_points == 0 or N == 0 is a valid call: it writes -1 / 0 and launches
 * nothing that reads.  The statistics words and the "done" mark are the call's own: the other calls of the keyframe matcher leave them alone, and
 * this one leaves theirs. */
typedef struct jsorb_scw_params {
    float th;                        /* 10 in LoopClosing::ComputeSim3 */
    int th_low;                      /* ORBmatcher::TH_LOW = 50; [0, 255] */
    float fx, fy, cx, cy;            /* pKF->fx .. cy */
    float min_x, max_x, min_y, max_y; /* KeyFrame::mnMinX, mnMaxX, mnMinY, mnMaxY: IsInImage's bounds and the grid origin */
    float inv_w, inv_h;              /* mfGridElementWidthInv, mfGridElementHeightInv */
    int cols, rows;                  /* mnGridCols, mnGridRows */
    float log_scale_factor;          /* KeyFrame::mfLogScaleFactor */
    int n_levels;                    /* mnScaleLevels, [1, JSORB_MAX_LEVELS] */
    float scale_factor[JSORB_MAX_LEVELS];        /* mvScaleFactors */
    float Rcw[9], tcw[3], Ow[3];     /* HOST: Scw decomposed as :286-290 - sRcw / scw row-major, Scw's translation / scw, -Rcw^T tcw */
} jsorb_scw_params;
int jsorb_search_by_projection_sim3_async(jsorb_keyframe_matcher *m, const jsorb_scw_params *params, int n_points, const float *Px, const float *Py,
                                          const float *Pz, const float *Nx, const float *Ny, const float *Nz, const float *max_distance,
                                          const float *min_dist_inv, const float *max_dist_inv, const uint8_t *desc, int n_keypoints, const float *x,
                                          const float *y, const int32_t *octave, const uint8_t *kf_desc, const uint8_t *blocked, int32_t *match_kp,
                                          int32_t *match_dist, int32_t *kp_match, int32_t *n_matches_dev);
/* Synchronous: the same into buffers of the matcher; match_kp_host[n_points], match_dist_host[n_points] and kp_match_host[N] (the last two may be
 * NULL) and *n_matches (host), one copy back. */
int jsorb_search_by_projection_sim3(jsorb_keyframe_matcher *m, const jsorb_scw_params *params, int n_points, const float *Px, const float *Py,
                                    const float *Pz, const float *Nx, const float *Ny, const float *Nz, const float *max_distance,
                                    const float *min_dist_inv, const float *max_dist_inv, const uint8_t *desc, int n_keypoints, const float *x,
                                    const float *y, const int32_t *octave, const uint8_t *kf_desc, const uint8_t *blocked, int32_t *match_kp_host,
                                    int32_t *match_dist_host, int32_t *kp_match_host, int *n_matches);
/* Diagnostics of the last call (waits for it): rounds = the rounds of the fixed point (at most n_points + 1); n_kept = the keys kept over all
 * points (candidates that passed the window, blocked and level filters with a distance <= th_low); n_overflow = points with more kept keys than the
 * build's list cap, which walk their window again; n_windows = points that reached a window; n_distances = Hamming distances k_scw_candidates
 * computed (the filters' survivors, kept or not); largest_window = the most keypoints in the cells of one window.  JSORB_ERR_STATE before the
 * first call.  Any pointer may be NULL. */
int jsorb_search_by_projection_sim3_stats(jsorb_keyframe_matcher *m, int *rounds, int *n_kept, int *n_overflow, int *n_windows, int *n_distances,
                                          int *largest_window);
/* The compile-time caps of this build's k_scw.hip (no device needed): keys k_scw_candidates keeps per point (32), keypoints up to which
 * k_scw_resolve keeps its claims in LDS (16384).  A test build lowers both (jetson_slam_amd/build.py VARIANTS). */
int jsorb_scw_build_caps(int *cap, int *lds_claims);

/* ---- memory: what orb_cuda::SyncedMem<T> needs (include/cuda/synced_mem_holder.hpp:10-65, src/cuda/synced_mem_holder.cpp:8-199) ----
 * The reference's untouched host code (ORBmatcher.cpp:1673-1877, Tracking.cpp:1427-1600, orb_stereo_match.cu statics) allocates
 * pinned-host + device buffer pairs and moves data with cudaMemcpy(Async) on a private stream; these calls are the HIP side of
 * that, so that include/jsorb_compat.hpp can offer the full SyncedMem surface without the consumer including a HIP header.
 * They act on the calling thread's current device (jsorb_mem_set_device), like the CUDA runtime calls they replace.
 * `stream` is a hipStream_t as void*; NULL = the null stream (blocking calls) / synchronous copy. */
int jsorb_mem_set_device(int device_id);
int jsorb_mem_alloc_host(size_t bytes, void **host_pinned);                  /* cudaMallocHost  (synced_mem_holder.cpp:63) */
int jsorb_mem_alloc_device(size_t bytes, void **device);                     /* cudaMalloc      (:67) */
int jsorb_mem_alloc_device_pitched(size_t width_bytes, size_t height, void **device, size_t *pitch);   /* cudaMallocPitch (:50) */
int jsorb_mem_free_host(void *host_pinned);                                  /* cudaFreeHost */
int jsorb_mem_free_device(void *device);                                     /* cudaFree */
int jsorb_mem_stream_create(void **stream);                                  /* cudaStreamCreate (:19) */
int jsorb_mem_stream_destroy(void *stream);
int jsorb_mem_stream_sync(void *stream);                                     /* cudaStreamSynchronize (:190) */
int jsorb_mem_device_sync(void);                                             /* the device-wide wait cudaFree / cudaFreeHost imply (:31-44): before a buffer is recycled */
int jsorb_mem_buffer_sync(const void *device);                               /* the same wait on the device that owns `device` (cudaFree waits for the buffer's device, not the caller's current one) */
int jsorb_mem_h2d(void *device_dst, const void *host_src, size_t bytes);     /* cudaMemcpy HostToDevice (:96) */
int jsorb_mem_d2h(void *host_dst, const void *device_src, size_t bytes);     /* cudaMemcpy DeviceToHost (:90) */
int jsorb_mem_d2d(void *device_dst, const void *device_src, size_t bytes);
int jsorb_mem_h2d_async(void *device_dst, const void *host_src, size_t bytes, void *stream);   /* cudaMemcpyAsync (:128) */
int jsorb_mem_d2h_async(void *host_dst, const void *device_src, size_t bytes, void *stream);   /* cudaMemcpyAsync (:122) */
int jsorb_mem_d2d_async(void *device_dst, const void *device_src, size_t bytes, void *stream);
int jsorb_mem_set_zero(void *device, size_t bytes);                          /* cudaMemset (:109) */
int jsorb_mem_set_zero_async(void *device, size_t bytes, void *stream);      /* cudaMemsetAsync (:115) */
const char *jsorb_mem_last_error(void);                                      /* text of the last failed jsorb_mem_* call of this thread */

/* ---- plumbing ---- */
/* Use an external HIP stream (hipStream_t as void*) instead of the handle's own, e.g. torch's current stream. NULL restores. */
int jsorb_set_stream(jsorb_extractor *e, void *hip_stream);
void *jsorb_get_stream(const jsorb_extractor *e);
/* Make another HIP stream (e.g. the one a collective will be issued on) wait for everything enqueued so far on this handle. */
int jsorb_stream_wait_done(jsorb_extractor *e, void *other_hip_stream);
/* Per-kernel hipEvent timing (off by default: it serialises launches). Accumulates until reset. */
int jsorb_enable_kernel_timing(jsorb_extractor *e, int on);
int jsorb_kernel_time(jsorb_extractor *e, int kernel_id, double *total_ms, long *launches);
int jsorb_reset_kernel_timing(jsorb_extractor *e);
const char *jsorb_kernel_name(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* JSORB_H */
