// jsorb_launch.h - host-callable launchers of the gfx950 kernels (one translation unit per stage).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/jsorb.h"
#include "jsorb_device.h"
#include "jsorb_env.h"
#include "undistort.h"

namespace jsorb {

struct StereoArgs {
    float maxD;        // mbf / mb                 (orb_stereo_match.cu:146)
    float mbf;
    int th_high;       // ORBmatcher::TH_HIGH
    int th_orb;        // (TH_HIGH + TH_LOW) / 2    (orb_stereo_match.cu:226)
};

// dynamic LDS bytes the detect kernel needs for the given geometry (max over levels)
size_t detect_lds_bytes(const Geometry &g);

size_t pyramid_lds_bytes(const Geometry &g);
int pyramid_ns_dispatched(int ns16);      // the NS template argument k_pyramid runs for a level that needs ns16 loads per row (1, 2 or 4)
int pyramid_loads_per_row(float s, int W); // 16-byte loads per lane and level-0 row in k_pyramid for a level of scale s and width W (exact, by enumeration)
int detect_swar6_threshold(int threshold);   // k_detect: threshold of the 6-bit early rejects if they provably accept a superset of the exact ones (exhaustive check), else 0
void fill_pyramid_layout(Geometry &g);     // rows per k_pyramid tile (pyr_th), sparse windows, workgroup table offsets (host side, once per handle)
void launch_upload_level0(const uint8_t *host_pinned, uint8_t *dst, size_t bytes, hipStream_t s);      // bytes: a multiple of 16
void launch_copy_level0(const uint8_t *src, size_t image_stride, int step, uint8_t *slab, size_t slab_bytes, int pitch, int W, int H, int n_images, hipStream_t s);
// k_rectify (k_rectify.hip): a handle's rectification map in the fixed-point form, on the device
#define RECT_TW 64                         // output tile of a workgroup: 64 columns (16 lanes x 4 pixels) x 32 rows (16 lane rows x RECT_RPL)
#define RECT_TH 32
#define RECT_RPL 2
#define RECT_LDS_W 128                     // largest source box (bytes x rows) a workgroup stages in LDS; larger footprints take global taps
#define RECT_LDS_H 64
struct RectMap {
    const int *xy;                         // per output pixel: (ix, iy) as two int16 (CV_16SC2), rows `pitch` entries apart
    const uint16_t *a;                     // per output pixel: fy << 5 | fx (CV_16UC1 masked to 10 bits)
    const int4 *tiles;                     // per output tile: source box x0, y0, rows, staged (rectify_tile_table)
    int pitch;                             // entries per map row (a multiple of 4)
    int ntx, nty;                          // output tiles per row / column
};
void launch_rectify(const RectMap &m, const uint8_t *src, size_t src_stride, int src_step, uint8_t *dst, size_t dst_stride, int dst_pitch, int W, int H,
                    int n_images, hipStream_t s);
void rectify_convert_maps(const float *mapx, const float *mapy, size_t n, int16_t *xy, uint16_t *a);      // host only
void rectify_tile_table(const int16_t *xy, const uint16_t *a, int W, int H, int map_pitch, int ntx, int nty, int32_t *tiles);      // host only
void launch_pyramid(const Geometry &g, const ImageSrc &src, uint8_t *slab, const uint32_t *ctab, int n_images, size_t lds_bytes, hipStream_t s);
int detect_ring_bit_of_pixel(int k);       // bit of ring pixel k in the index of the arc LUT as k_detect forms it (the host stores the LUT in that order)
// images with up to this many tiles: k_compact as a launch of its own runs its re-reading form with 256-thread workgroups on batch handles (k_compact.hip), and a
// batch of one lane takes the fused k_blur_compact launch (jsorb_extract.hip: run_pipeline)
#ifndef CMP_MID_T
#define CMP_MID_T 8192
#endif
void fill_detect_layout(Geometry &g);      // tile rows per workgroup (det_R), workgroup table offsets and per-level LDS layout of k_detect (host side, once per handle)
void launch_detect(const Geometry &g, const ImageSrc &src, const uint8_t *slab, const uint8_t *mask_slab,
                   const uint32_t *lut_bits, unsigned long long *tile_out, int n_images, size_t lds_bytes, hipStream_t s,
                   unsigned *spill = nullptr, unsigned *spill_flags = nullptr);      // compact handles: the arena of spill chunks and its busy flags
int detect_spill_chunk_entries(const Geometry &g);      // u32 entries of one spill chunk (the handle's largest band region)
size_t detect_arena_bytes(const Geometry &g);           // the whole arena: 8 XCDs x slots x chunk
size_t detect_arena_flag_words();                       // one busy flag per chunk
bool detect_arena_covers(int compute_units);           // the arena has a chunk for every workgroup of the compact k_detect that can be resident on a device of this size (8 XCDs of <= 32 CUs)
int detect_pos_cap(const Geometry &g, int level);   // entries of a k_detect workgroup's pool of positives on that level (compact form)
void launch_nms_ms(const Geometry &g, unsigned long long *tile_out, int *ms_grid, int *ms_scratch, int mode_gpu, int n_images, hipStream_t s);
int compact_form(const Geometry &g);      // which of launch_compact's launches compacts this geometry's images (JSORB_COMPACT_*, include/jsorb.h)
void launch_compact(const Geometry &g, const unsigned long long *tile_out, unsigned long long *kp, int *counts,
                    int *row_tab, int n_images, hipStream_t s, int *counts_host = nullptr);
// single image: k_detect and k_blur fit one launch (full-plane k_detect; k_blur's 10 KB of static LDS come on top of k_detect's request)
inline bool detect_blur_fusable(const Geometry &g, size_t detect_lds) { return g.blur_blocks > 0 && !g.det_compact && detect_lds + 12 * 1024 <= 64 * 1024; }
void launch_detect_blur(const Geometry &g, const ImageSrc &src, const uint8_t *slab, const uint8_t *mask_slab, const uint32_t *lut_bits,
                        unsigned long long *tile_out, uint8_t *blur_slab, size_t lds_bytes, hipStream_t s);      // single image: k_detect and k_blur as one launch
void fill_blur_layout(Geometry &g);        // k_blur: strips x bands per level, workgroups per level (host side, once per handle)
int blur_level_blocks(const LevelDesc &lv);
void launch_blur(const Geometry &g, const ImageSrc &src, const uint8_t *slab, uint8_t *blur_slab, const uint32_t *ctab, int n_images, hipStream_t s);
bool blur_compact_fusable(const Geometry &g);      // batches: k_compact as workgroup 0 of every image of the k_blur launch (k_blur.hip)
void launch_blur_compact(const Geometry &g, const ImageSrc &src, const uint8_t *slab, uint8_t *blur_slab, const uint32_t *ctab, int n_images, hipStream_t s,
                         const unsigned long long *tile_out, unsigned long long *kp, int *counts, int *row_tab, int *counts_host);
void launch_describe(const Geometry &g, const ImageSrc &src, const uint8_t *slab, const uint8_t *blur_slab,
                     const unsigned long long *kp, const int *counts, float *angles, uint8_t *desc, int32_t *out_kp,
                     int n_images, hipStream_t s, Deliver dl = Deliver{nullptr, nullptr, nullptr, nullptr, nullptr});
const void *describe_kernel_address();    // host-side address of k_describe (identifies its node in a captured graph)
int describe_kernel_deliver_arg();         // index of its `Deliver dl` argument
void launch_stereo(const Geometry &g, const ImageSrc &srcL, const uint8_t *slabL, const ImageSrc &srcR, const uint8_t *slabR,
                   const int32_t *outL, const int *countsL, const uint8_t *descL,
                   const int32_t *outR, const int *countsR, const uint8_t *descR, const int *row_tabR,
                   float *u_right, float *depth, int *best_l1, unsigned *aux, StereoArgs a, int n_pairs, hipStream_t s, int *diag = nullptr);
#define JSORB_STEREO_DIAG_INTS 13          // per left keypoint: best right index, its Hamming distance, 11 L1 window sums (jsorb_copy_stereo_diagnostics)
void launch_unpack_keypoints(const int32_t *soa, int n, jsorb_keypoint *out, hipStream_t s);
void launch_assign_grid(const int32_t *soa, const float *xy_un, int n, float min_x, float min_y, float inv_w, float inv_h, int cols, int rows,
                        int32_t *cell_start, int32_t *cell_items, hipStream_t s);      // xy_un: x_un[N] y_un[N] to bin instead of the keypoints (NULL: the keypoints)
// k_undistort / k_rgbd (k_undistort.hip): per-image outputs at the handle's stride T (x_un[N] y_un[N] in 2T floats; uRight / depth in T floats each)
struct RgbdArgs {
    int format;                            // JSORB_DEPTH_U16 / JSORB_DEPTH_F32
    int scale;                             // f32: 1 = multiply by factor (Tracking.cpp:333: |factor - 1| > 1e-5); u16 always converts
    float factor, mbf;
};
void launch_undistort(const UndistortCam &cam, const int32_t *soa, const int *counts, int T, float *un, float *un_host, int n_images, hipStream_t s);
void launch_rgbd(const int32_t *soa, const int *counts, int T, const float *un, const uint8_t *depth, size_t image_stride, size_t step, int W, int H,
                 const RgbdArgs &a, float *u_out, float *d_out, float *u_host, float *d_host, int n_images, hipStream_t s);
// The frame side of the four grid matchers: one image of a handle and the grid CSR the call built over it (jsorb_search.hip: search_begin)
struct FrameView {
    const int32_t *soa;                          // keypoint SoA (6N): x, y, ., angle (float bits), octave, .
    const float *xy_un;                          // mvKeysUn as x_un[N] y_un[N] (NULL: the keypoints themselves)
    const uint8_t *desc;
    const float *u_right;                        // mvuRight (NULL: monocular, or a matcher that does not read it)
    const uint8_t *blocked;                      // blocked_in (NULL: none)
    int n_kp;
    const int32_t *cell_start, *cell_items;      // grid CSR (k_assign_grid)
    int n_levels;
    float scale[JSORB_MAX_LEVELS];               // mvScaleFactors
    __device__ __forceinline__ float x(int k) const { return xy_un ? xy_un[k] : (float)soa[k]; }      // mvKeysUn[k].pt
    __device__ __forceinline__ float y(int k) const { return xy_un ? xy_un[n_kp + k] : (float)soa[n_kp + k]; }
    __device__ __forceinline__ float angle(int k) const { return __int_as_float(soa[3 * (size_t)n_kp + k]); }
    __device__ __forceinline__ int octave(int k) const { return soa[4 * (size_t)n_kp + k]; }
};
// k_local_candidates / k_local_resolve (k_search_local.hip): ORBmatcher::SearchByProjection(Frame&, map points, th) over one image of a handle
struct SearchLocalArgs {
    FrameView f;
    float min_x, min_y, inv_w, inv_h;
    int cols, rows;
    // the map points, in the caller's order
    int n_points;
    const float *u, *v, *invz, *view_cos;
    const int32_t *level;
    const uint8_t *in_frustum, *mp_desc;
    float th, nn_ratio, mbf;
    int th_high;
    // workspace and outputs
    int *cand, *cand_n;                          // n_points x search_local_cap() packed candidates, n_points counts
    int32_t *match_kp, *match_dist, *kp_match, *n_matches;
    int *stats;                                  // rounds, candidates, points over the capacity
};
int search_local_cap();
void launch_local_candidates(const SearchLocalArgs &a, hipStream_t s);
void launch_local_resolve(const SearchLocalArgs &a, hipStream_t s);
// k_last_match / k_last_resolve (k_search_last.hip): ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono), its GPU branch, over one image
struct LastFrameArgs {
    FrameView f;                                 // the current frame (blocked unused)
    // the last frame's points, in ascending last-frame index
    int n_points;
    const float *Px, *Py, *Pz, *angle;
    const int32_t *octave;
    const uint8_t *mp_desc;
    jsorb_last_frame_params p;                   // threshold, direction, camera, bounds, grid, pose
    // workspace and outputs
    int *owner;                                  // N: largest point index that chose keypoint k (-1 between calls: k_last_resolve resets it)
    int *bin, *cand;                             // per point: rotation bin (-1: no match), candidates
    int *ctl;                                    // run the second pass, passes, candidates, ind1, ind2, ind3
    int32_t *match_kp, *match_dist, *kp_match, *n_matches;
};
void launch_last_match(const LastFrameArgs &a, int pass, hipStream_t s);
void launch_last_resolve(const LastFrameArgs &a, int pass, hipStream_t s);
// k_kf_candidates / k_kf_resolve (k_search_kf.hip): ORBmatcher::SearchByProjection(CurrentFrame, KeyFrame*, sAlreadyFound, th, ORBdist) over one image
struct SearchKfArgs {
    FrameView f;                                 // the current frame (u_right unused)
    // the keyframe's points, in ascending keyframe slot
    int n_points;
    const float *Px, *Py, *Pz, *max_distance, *max_dist_inv, *min_dist_inv, *angle;
    const uint8_t *mp_desc;
    jsorb_kf_projection_params p;                // window, threshold, camera, bounds, grid, pose
    // workspace and outputs
    int *cand, *cand_n;                          // n_points x search_kf_cap() keys (distance << 18 | CSR position) in walk order, n_points counts
    int32_t *match_kp, *match_dist, *kp_match, *n_matches;
    int *stats;                                  // rounds, candidates, points over the capacity, ind1, ind2, ind3
};
int search_kf_cap();                            // the compile-time caps of k_search_kf.hip (jsorb_search_kf_build_caps)
int search_kf_lds_claims();
void launch_kf_candidates(const SearchKfArgs &a, hipStream_t s);
void launch_kf_resolve(const SearchKfArgs &a, hipStream_t s);
// k_init_candidates / k_init_resolve (k_search_init.hip): ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
struct SearchInitArgs {
    FrameView f;                                 // F2 (u_right, blocked and the levels unused)
    jsorb_init_params p;                         // window, ratio, threshold, grid
    // F1, in keypoint order
    int n1;
    const int32_t *octave;
    const float *angle;
    const uint8_t *f1_desc;
    float *prev;                                 // vbPrevMatched: x[n1] y[n1], read by k_init_candidates, updated by k_init_resolve
    // workspace
    int *cand, *cand_n;                          // n1 x search_init_cap() packed candidates in walk order, n1 counts
    int *order;                                  // n1: the points with candidates, ascending
    int *state;                                  // N: matched_distance << 8 | chunk mark, when it does not fit the LDS
    int *owner;                                  // N: last claimant (vnMatches21)
    int *stats;                                  // rounds, candidates, points over the capacity, displaced claims, ind1, ind2, ind3
    // outputs
    int32_t *matches12, *matches21, *n_matches;  // matches21 may be NULL
};
int search_init_cap();
void launch_init_candidates(const SearchInitArgs &a, hipStream_t s);
void launch_init_resolve(const SearchInitArgs &a, hipStream_t s);
void launch_init_keys_un(const int32_t *soa, const float *xy_un, int n, float *dst, hipStream_t s);      // mvKeysUn points: x[n] y[n]
// k_bow_transform / k_bow_group / k_bow_match / k_bow_resolve (k_bow.hip): Frame::ComputeBoW's descent and ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...)
struct BowVocab {
    const int32_t *child_start, *children;       // CSR of the tree: the children of node i are children[child_start[i] .. child_start[i + 1]), in the caller's order
    const uint8_t *child_desc;                   // the descriptor of children[c] at 32 c: a node's children lie next to each other
    const int32_t *word;                         // per node: word id (leaves)
    const uint8_t *live;                         // per node: weight > 0
    int depth_L, nid_level;                      // nid_level = depth_L - levels_up
};
#define JSORB_BOW_MAX_KEYFRAMES 256
struct BowMatchArgs {
    // the frame: descriptors, node per keypoint (-1: in none)
    const uint8_t *desc;
    const int32_t *f_node;
    int N;
    // the keyframes, concatenated; keyframe i is kf_start[i] .. kf_start[i + 1] (relative to the pointers below)
    int n_kf;
    const int32_t *kf_node;
    const uint8_t *kf_valid;
    const uint8_t *kf_desc;
    jsorb_bow_params p;
    // workspace and outputs
    unsigned long long *f_sorted, *kf_sorted;    // keys node << 18 | index, ascending; keypoints in no node last
    int32_t *match_kf;                           // n_kf x N (cleared to -1)
    int *stats;                                  // node pairs, distances, largest frame node of a pair; then k_bow_resolve's kept bins (cleared to 0)
    int kf_start[JSORB_BOW_MAX_KEYFRAMES + 1];
};
int bow_node_regs();                            // the compile-time caps of k_bow.hip (jsorb_bow_build_caps)
int bow_sort_lds();
void launch_bow_transform(const BowVocab &v, const uint8_t *desc, size_t desc_stride, const int *counts, int counts_stride, int n, int32_t *word,
                          int32_t *node, size_t out_stride, int *n_shallow, int n_images, hipStream_t s);      // counts NULL: n descriptors; else a grid for n, counts[img * counts_stride] of them per image
void launch_bow_group(const BowMatchArgs &a, hipStream_t s);
void launch_bow_match(const BowMatchArgs &a, hipStream_t s);
// k_bow_resolve (k_bow.hip) and k_tri_resolve (k_triangulate.hip): the rotation check over rows of matches (k_search_common.h: row_resolve).  Row kf is
// match[kf * n .. + n); entry k holds j relative to kf_start[kf], or -1
struct RowResolveArgs {
    int n_kf, n;                                 // rows, entries of a row
    const float *row_angle;                      // the angle of row position k (n of them)
    const float *kf_angle;                       // the angle of entry kf_start[kf] + j of the concatenated side
    int check_orientation;
    int32_t *match, *n_matches;                  // n_kf x n (culled in place), n_kf (every non-empty keyframe's count written)
    int *kept;                                   // three statistics words: ind1 + 1, ind2 + 1, ind3 + 1 of keyframe 0 (cleared to 0)
    int kf_start[JSORB_BOW_MAX_KEYFRAMES + 1];
};
void launch_bow_resolve(const RowResolveArgs &a, hipStream_t s);      // rot_bin(kf_angle, row_angle): SearchByBoW(KeyFrame*, Frame&)
// k_tri_match / k_tri_resolve (k_triangulate.hip): ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) for several KF2;
// the grouping is launch_bow_group over a BowMatchArgs whose frame side is KF1
struct TriArgs {
    // KF1: n1 keypoints
    int n1;
    const uint8_t *free1, *stereo1;
    const float *x1, *y1;
    const uint8_t *desc1;
    // the KF2s, concatenated; keyframe i is kf_start[i] .. kf_start[i + 1] (relative to the pointers below)
    int n_kf;
    const uint8_t *free2, *stereo2;
    const float *x2, *y2;
    const int32_t *octave2;
    const uint8_t *desc2;
    int th_low, only_stereo, n_levels;
    float gate[JSORB_MAX_LEVELS];                // 100.0f * mvScaleFactors[l]: the epipole gate's right side
    double line[JSORB_MAX_LEVELS];               // 3.84 * (double)mvLevelSigma2[l]: the line test's right side
    // workspace and outputs
    const unsigned long long *sorted1, *sorted2; // k_bow_group's keys
    int32_t *match12;                            // n_kf x n1 (cleared to -1)
    int *stats;                                  // node pairs, distances, line tests, largest KF2 node of a pair; then k_tri_resolve's kept bins (cleared to 0)
    int kf_start[JSORB_BOW_MAX_KEYFRAMES + 1];
};
#define TR_KF_CHUNK 32                          // keyframes whose geometry one k_tri_match launch carries in its arguments
struct TriGeom {
    int kf0, n;                                  // the launch's keyframes kf0 .. kf0 + n
    float f[TR_KF_CHUNK][11];                    // F12 row-major, ex, ey
};
void launch_tri_match(const TriArgs &a, const TriGeom &g, hipStream_t s);
void launch_tri_resolve(const RowResolveArgs &a, hipStream_t s);      // rot_bin(row_angle, kf_angle): SearchForTriangulation, SearchByBoW(KF, KF)
// k_fuse_grids / k_fuse_match (k_fuse.hip): ORBmatcher::Fuse(pKF, vpMapPoints, th) and its loop-closing overload for several keyframes in one call
#define FUSE_MAX_CELLS 4096                      // cols * rows k_fuse_grids holds in LDS (counts and cursors of every cell, 1024 scan words)
struct FuseGridArgs {
    const float *x, *y;                          // mvKeysUn of the keyframes, concatenated
    float min_x, min_y, inv_w, inv_h;
    int cols, rows;
    int32_t *cell_start, *cell_items;            // per keyframe cols * rows + 1 starts (relative to the keyframe); items at the keyframe's offset
    int kf_start[JSORB_BOW_MAX_KEYFRAMES + 1];
};
struct FuseArgs {
    jsorb_fuse_params p;
    // the map points, in the caller's order
    int n_points;
    const float *Px, *Py, *Pz, *Nx, *Ny, *Nz, *max_distance, *min_dist_inv, *max_dist_inv;
    const uint8_t *mp_desc;
    // the keyframes, concatenated (the launch's FusePose has their offsets)
    const float *x, *y, *uright;                 // uright NULL: every keyframe monocular
    const int32_t *octave;
    const uint8_t *kf_desc;
    const uint8_t *skip;                         // n_kf x n_points or NULL
    const int32_t *cell_start, *cell_items;      // k_fuse_grids' CSRs
    // outputs
    int32_t *best_idx, *best_dist, *n_matched;   // n_kf x n_points each (every entry written), n_kf (cleared to 0)
    int *stats;                                  // pairs with a window, keypoints walked, distances, largest window (cleared to 0)
};
#define FUSE_KF_CHUNK 32                        // keyframes whose pose and offsets one k_fuse_match launch carries in its arguments
struct FusePose {
    int kf0, n;                                  // the launch's keyframes kf0 .. kf0 + n
    int start[FUSE_KF_CHUNK + 1];                // their kf_start
    float pose[FUSE_KF_CHUNK][15];               // Rcw row-major, tcw, Ow
};
void launch_fuse_grids(const FuseGridArgs &g, int n_kf, hipStream_t s);
void launch_fuse_match(const FuseArgs &a, const FusePose &g, hipStream_t s);
// k_fuse_match_run (k_fuse.hip): k_fuse_match over one keyframe of a jsorb_keyframe_graph, its run read on the device
struct FuseRun {
    int row, slot;                               // the row of best_idx / best_dist (the target's number), the target's slot
    int n_slots, pool_entries;
    const uint8_t *state;                        // the graph's arrays
    const int32_t *point_off, *point_len;
    float pose[15];                              // Rcw row-major, tcw, Ow
};
void launch_fuse_match_run(const FuseArgs &a, const FuseRun &r, hipStream_t s);
// k_fa_* (k_fuse_apply.hip): ORBmatcher::Fuse with its map mutations over the device state (jsorb_fuse_map_async)
#define FM_COUNTS 10
struct FuseMapArgs {
    jsorb_keyframe_graph g;
    jsorb_keyframe_keypoints kp;
    jsorb_fuse_state st;
    jsorb_fuse_params p;
    int n_rows;
    const float *tab[9];                         // the table's Px .. invariance_minDistance in FuseArgs' order (Px Py Pz Nx Ny Nz max_distance min_dist_inv max_dist_inv)
    int n_list, n_targets, sim3, replace_loop, log_cap;
    const int32_t *list_row;
    // the observation index: the lists threaded through the pool (cleared per call: head and ent_slot to -1)
    int32_t *head, *next, *ent_slot;             // [n_rows] first entry of the row's list, [pool] the next one, [pool] the slot whose run holds the entry
    int32_t *mark, *snap, *slot_mark;            // stamps (cleared to 0 per call): [n_rows] Replace target in target t (t + 1), [n_rows] in vpMatched's set of
                                                 // target t (t + 1), [S] the survivor observes this slot (the Replace's number)
    int32_t *grid_start, *grid_items;            // the target's grid: cells + 1 starts, its run's items
    float *gf;                                   // [9][n_list] the list points' floats for k_fuse_match_run
    uint8_t *gdesc, *skip;                       // [n_list][32], [n_list]
    int32_t *marked, *obs_start, *out_row, *csr_ent;     // the target's Replace targets, their observations as a CSR ([n_list + 1], [pool]) for k_distinct
    int32_t *ctl;                                // 0 Replace calls so far, 1 marked rows of this target
    int32_t *ds;                                 // k_distinct's statistics words of this call
    int32_t *best_idx, *replace_point, *n_fused, *log_out, *counts_dev;
    int *stats;                                  // FM_COUNTS words (cleared to 0)
};
int fuse_map_list_chunk();                       // the compile-time cap of k_fuse_apply.hip (jsorb_fuse_map_build_caps)
void launch_fuse_map_index(const FuseMapArgs &a, hipStream_t s);
void launch_fuse_map_head(const FuseMapArgs &a, int t, int slot, hipStream_t s);      // the snapshot, the grid, the head tests and the gather
void launch_fuse_map_apply(const FuseMapArgs &a, int t, int slot, hipStream_t s);     // the walk, the Replace loop, the CSR of the marked rows
void launch_fuse_map_finish(const FuseMapArgs &a, hipStream_t s);
// k_np_* (k_new_points.hip): LocalMapping::CreateNewMapPoints' loop over the device state (jsorb_create_new_map_points_async); the matching is
// launch_bow_group / launch_tri_match over the sides k_np_gather copies out of the pool runs
#define NP_COUNTS 12
#define NP_KF_CHUNK 16                          // neighbours whose poses one k_np_verdict launch carries in its arguments
struct NewPointsArgs {
    jsorb_keyframe_graph g;
    jsorb_keyframe_keypoints kp;
    jsorb_new_point_keypoints ex;
    jsorb_new_point_state st;
    int n_rows, current_slot, n1, cap, n_nb;     // cap: run_capacity, the stride of a neighbour in the gathered KF2 side
    int row_capacity, log_cap, current_kf_id, n_levels;
    float ratio_factor;
    float scale_factor[JSORB_MAX_LEVELS];
    double chi2_mono[JSORB_MAX_LEVELS], chi2_stereo[JSORB_MAX_LEVELS];      // 5.991 * (double)mvLevelSigma2[l], 7.8 * (double)mvLevelSigma2[l]
    const int32_t *new_row;
    // the gathered sides (TriArgs' inputs): KF1's n1 entries, neighbour t at t * cap
    int32_t *node1, *node2, *octave2;
    uint8_t *free1, *free2, *stereo1, *stereo2, *desc1, *desc2;
    float *x1, *y1, *x2, *y2;
    int32_t *info;                               // [0] the current run's offset, [1 + t] neighbour t's; -1: skipped
    int32_t *nb_slot;                            // [n_nb] the neighbours' slots
    float *ow;                                   // [3 (n_nb + 1)] the neighbours' camera centres, then the current keyframe's (k_np_verdict writes them from its poses, k_np_write reads them)
    int32_t *match12;                            // n_nb x n1 (cleared to -1)
    int32_t *claim;                              // n_nb x cap (cleared to -1): the last creating pair of a KF2 keypoint
    int32_t *pair_row;                           // n_nb x n1: the table row of a created pair
    unsigned *chunk_sum, *chunk_pre;             // the compaction: creating pairs per chunk, their exclusive prefix (chunks + 1)
    int32_t *verdict;
    uint8_t *path;
    float *x3D;
    int32_t *log_out, *counts_dev;
    int *stats;                                  // NP_COUNTS words (cleared to 0)
};
struct NewPointsSlots { int32_t slot[JSORB_BOW_MAX_KEYFRAMES]; };
struct NewPointsPoses {
    int kf0, n;                                  // the launch's neighbours kf0 .. kf0 + n
    jsorb_keyframe_pose cur, nb[NP_KF_CHUNK];
};
int new_points_chunk();                          // the compile-time cap of k_new_points.hip (jsorb_create_new_map_points_build_caps)
void launch_new_points_gather(const NewPointsArgs &a, const NewPointsSlots &s, hipStream_t st);
void launch_new_points_verdict(const NewPointsArgs &a, const NewPointsPoses &p, hipStream_t st);
void launch_new_points_apply(const NewPointsArgs &a, hipStream_t st);      // ownership, compaction, the rows' writes, the KF2 entries, the counts
// k_pose_optimize / k_apply_matches (k_pose.hip): Optimizer::PoseOptimization (Optimizer.cpp:244-456) for n_problems problems over one image, one
// workgroup a problem for the whole four-round loop; and the F.mvpMapPoints[bestIdx] = pMP of the matchers' callers
#define PO_STATS 8
struct PoseArgs {
    jsorb_pose_params prm;
    float delta_mono, delta_stereo;              // the FLOATS sqrt(5.991), sqrt(7.815) (Optimizer.cpp:278-279)
    const int32_t *soa;                          // keypoint SoA (6N): x, y, ., ., octave, .
    const float *xy_un;                          // mvKeysUn as x_un[N] y_un[N] (NULL: the keypoints themselves)
    int N, n_rows, n_problems;
    const float *Px, *Py, *Pz;                   // the table's positions
    const int32_t *frame_row;                    // n_problems x N
    const float *u_right;                        // N or NULL
    const float *Tcw_in;                         // n_problems x 16
    float *Tcw_out;
    double *pose_out;                            // n_problems x 12 or NULL
    uint8_t *outlier;                            // n_problems x N: the edges' flags between the rounds, too
    int32_t *row_out;                            // n_problems x N or NULL
    int32_t *counts;                             // n_problems x 4
    int32_t *edge_kp;                            // scratch, n_problems x N: a problem's edges as keypoints in ascending order, bit 31 = stereo
    int *stats;                                  // PO_STATS words (cleared to 0), jsorb_pose_optimization_stats' order
};
int pose_threads();                              // the compile-time caps of k_pose.hip (jsorb_pose_optimization_build_caps)
int pose_edge_regs();
void launch_pose_optimize(const PoseArgs &a, hipStream_t s);
void launch_apply_matches(int n_points, const int32_t *point_row, const int32_t *match_kp, int N, int32_t *frame_point_row, hipStream_t s);
// k_loop_bow_match (k_loop.hip): ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) for several candidates KF2 of LoopClosing::ComputeSim3; the grouping
// is launch_bow_group over a BowMatchArgs whose frame side is KF1, the resolver launch_tri_resolve over the same rows
struct LoopBowArgs {
    // KF1: n1 keypoints
    int n1;
    const uint8_t *valid1;
    const uint8_t *desc1;
    // the candidates, concatenated; candidate i is kf_start[i] .. kf_start[i + 1] (relative to the pointers below)
    int n_kf;
    const uint8_t *valid2;
    const uint8_t *desc2;
    jsorb_bow_params p;
    // workspace and outputs
    const unsigned long long *sorted1, *sorted2; // k_bow_group's keys
    uint8_t *matched2;                           // vbMatched2 of the entries beyond the register cap: one byte per candidate keypoint (cleared to 0)
    int32_t *match12;                            // n_kf x n1 (cleared to -1)
    int *stats;                                  // node pairs, distances, ., largest candidate node of a pair, ind1 + 1, ind2 + 1, ind3 + 1 of candidate 0 (k_tri_resolve's layout)
    int kf_start[JSORB_BOW_MAX_KEYFRAMES + 1];
};
int loop_node_regs();                           // the compile-time cap of k_loop.hip (jsorb_loop_build_caps)
void launch_loop_bow_match(const LoopBowArgs &a, hipStream_t s);
// k_sim3_match / k_sim3_agree (k_loop.hip): ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th); the grids are launch_fuse_grids'
struct Sim3Side {
    int n;
    const float *x, *y;                          // mvKeysUn
    const int32_t *octave;
    const uint8_t *kp_desc;
    const float *Px, *Py, *Pz, *max_distance, *min_dist_inv, *max_dist_inv;
    const uint8_t *mp_desc, *search;
    float T[24];                                 // Rw row-major, tw, then sR row-major, t into the OTHER camera
    const int32_t *cell_start, *cell_items;      // this keyframe's grid CSR
    int32_t *match;                              // vnMatch of this side: n entries, every one written
};
struct Sim3Args {
    jsorb_sim3_params p;
    Sim3Side s[2];
    int32_t *match12, *n_found;                  // n1 entries (every one written), one count (cleared to 0)
    int *stats;                                  // slots with a window, keypoints walked, distances, largest window, agreements (cleared to 0)
};
void launch_sim3_match(const Sim3Args &a, hipStream_t s);
void launch_sim3_agree(const Sim3Args &a, hipStream_t s);
// k_scw_candidates / k_scw_resolve (k_scw.hip): ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th); the grid is launch_fuse_grids'
struct ScwArgs {
    jsorb_scw_params p;                          // window, threshold, camera, bounds, grid, levels, pose
    // the loop points, in vpPoints order
    int n_points;
    const float *Px, *Py, *Pz, *Nx, *Ny, *Nz, *max_distance, *min_dist_inv, *max_dist_inv;
    const uint8_t *mp_desc;
    // the keyframe
    int n_kp;
    const float *x, *y;                          // mvKeysUn
    const int32_t *octave;
    const uint8_t *kf_desc;
    const uint8_t *blocked;                      // vpMatched[k] != NULL before the call (NULL: none)
    const int32_t *cell_start, *cell_items;      // k_fuse_grids' CSR
    // workspace and outputs
    int *cand, *cand_n;                          // n_points x scw_cap() kept keys (distance << 18 | CSR position, distance <= th_low) in walk order, n_points counts
    int32_t *match_kp, *match_dist, *kp_match, *n_matches;
    int *stats;                                  // rounds, keys kept, points over the capacity, points with a window, distances, largest window (cleared to 0)
};
int scw_cap();                                  // the compile-time caps of k_scw.hip (jsorb_scw_build_caps)
int scw_lds_claims();
void launch_scw_candidates(const ScwArgs &a, hipStream_t s);
void launch_scw_resolve(const ScwArgs &a, hipStream_t s);
// k_distinct_plan / k_distinct_lanes / k_distinct_block (k_distinct.hip): MapPoint::ComputeDistinctiveDescriptors for n_points map points
struct DistinctArgs {
    int n_points, n_obs, n_rows, n_out_rows;
    const int32_t *obs_start, *obs_row;          // the observations' CSR (n_points + 1) and their rows of kf_desc (n_obs)
    const uint8_t *kf_desc;                      // n_rows x 32 bytes
    const int32_t *out_row;                      // NULL: point p writes row p
    // workspace and outputs
    int *list;                                   // 3 x n_points: the points of the group, wave and block tier (stats[0 .. 2] of them)
    int32_t *best_obs, *best_median;             // n_points each, every entry written
    uint8_t *desc_out, *changed;                 // n_out_rows x 32 bytes or NULL; n_points bytes or NULL
    int *stats;                                  // points per tier (3), block-tier points beyond the LDS cap, empty, invalid, changed, largest N (cleared to 0)
};
int distinct_group_lanes();                     // the compile-time caps of k_distinct.hip (jsorb_distinct_build_caps)
int distinct_wave_lanes();
int distinct_lds_desc();
void launch_distinct(const DistinctArgs &a, hipStream_t s);
// k_kfdb.hip: the keyframe database (KeyFrameDatabase.cpp:44-313, DBoW2's BowVector / L1Scoring).  A BowVector is (word, value, n): sorted distinct
// word ids, their L1-normalised values, the count on the device.
struct KfdbVector {
    const int32_t *word;
    const double *value;
    const int32_t *n;                            // device count, clamped to [0, cap] by every reader
    int cap;
};
struct KfdbState {                               // per slot, `slots` of them; the BowVectors live in the pool at off[s] .. off[s] + len[s]
    int slots;                                   // the slots the kernels walk: the highest slot ever added + 1
    int32_t *present, *off, *len;
    uint32_t *seq;                               // add sequence number
    unsigned long long *loop_query, *reloc_query;
    int32_t *loop_words, *reloc_words;
    float *loop_score, *reloc_score;
    int32_t *pool_word;
    double *pool_value;
};
#define KFDB_CTRL 16                             // control words of a query, zeroed in front of it (see k_kfdb.hip)
#define KFDB_NEIGHBOURS 10                       // GetBestCovisibilityKeyFrames(10)
struct KfdbQueryArgs {
    KfdbState st;
    KfdbVector q;
    unsigned long long id;
    int reloc;                                   // 0: DetectLoopCandidates, 1: DetectRelocalizationCandidates
    const uint8_t *connected;                    // loop: a byte per slot, or NULL
    const int32_t *neighbours;                   // slots x KFDB_NEIGHBOURS
    float min_score;                             // loop: the host value, unless ...
    const float *min_score_dev;                  // ... this is not NULL
    unsigned long long *key;                     // scratch per slot: the list key (lowest common word << 32 | seq), ~0 when not listed
    float *tscore;                               // scratch per slot: (float)score of the slots with a common word
    int32_t *first_pos;                          // scratch per slot: the first retained list position whose best slot it is
    int32_t *list, *ent_flag, *ent_best;         // scratch per list position: the slot, kept, its best slot
    float *ent_acc;                              // ... its accumulated score
    int32_t *ctrl;                               // KFDB_CTRL words
    int32_t *candidates, *n_candidates;          // outputs
};
struct KfdbScoreArgs {
    KfdbState st;
    KfdbVector q;
    const int32_t *slot_list;
    int n_slots;
    float *score;
    double *score_f64;                           // or NULL
    float *min_score;
};
int kfdb_query_lds();                            // the compile-time caps of k_kfdb.hip (jsorb_kfdb_build_caps)
int kfdb_sort_lds();
void launch_kfdb_bow_vector(const int32_t *word_id, int n, const double *weight, int n_words, uint32_t *sort_scratch, int32_t *bow_word, double *bow_value,
                            int32_t *bow_n, hipStream_t s);
void launch_kfdb_add(const KfdbState &st, int slot, uint32_t seq, int off, const KfdbVector &v, hipStream_t s);
void launch_kfdb_score(const KfdbScoreArgs &a, hipStream_t s);
void launch_kfdb_query(const KfdbQueryArgs &a, hipStream_t s);
// k_vocab_train.hip: TemplatedVocabulary::create, one level of the tree at a time.  The nodes of a level are the S segments seg_start[s] ..
// seg_start[s + 1] of the m positions; position p holds input descriptor perm[p], whose 32 bytes are rows[perm[p]].
struct VocabTrainArgs {
    int m, S, k;
    unsigned long long seed;
    const uint8_t *rows;                         // the caller's n x 32 bytes, read through perm
    const int32_t *perm;                         // m
    const int32_t *seg_start;                    // S + 1
    const int32_t *cslot;                        // S: the segment's slot in `counters`, -1 for the trivial segments (size <= k)
    int32_t *seg_of;                             // m
    int32_t *seg_nc, *seg_j, *seg_changed;       // S: centres, draws consumed, the last pass that moved a descriptor
    uint32_t *centres;                           // S x k x 8 dwords
    uint32_t *cnt;                               // S x k members of the last pass
    uint32_t *counters;                          // slots x k x 256 bit counts
    uint8_t *assoc;                              // m
    uint32_t *mind;                              // m: min_dists
    uint32_t *chunk_sum;                         // chunks
    unsigned long long *chunk_pre;               // chunks + 1
    int32_t *level_word;                         // the last pass that moved any descriptor
    // regrouping
    uint32_t *hist, *hist_pre;                   // chunks x k, (chunks + 1) x k
    uint32_t *seg_rank;                          // S x k: positions before the segment with each cluster index
    const int32_t *dest_base;                    // S x k: the child's first position on the next level, -1 when it ends here
    const int32_t *node_base;                    // S: the level-order node number of the segment's first child
    int m_next;
    int32_t *perm_out;                           // m_next
    int32_t *leaf;                               // n: per input descriptor the level-order node its path ended in
};
int vocab_train_chunk();                        // the compile-time caps of k_vocab_train.hip (jsorb_vocab_train_build_caps)
int vocab_train_scan_threads();
inline int vocab_train_chunks(int m) { return (m + vocab_train_chunk() - 1) / vocab_train_chunk(); }
void launch_vocab_train_iota(int32_t *perm, int n, hipStream_t s);
void launch_vocab_train_seed(const VocabTrainArgs &a, hipStream_t s);             // seg_of, the first centre, then k - 1 kmeans++ steps
void launch_vocab_train_assign(const VocabTrainArgs &a, int pass, hipStream_t s);
void launch_vocab_train_means(const VocabTrainArgs &a, hipStream_t s);
void launch_vocab_train_regroup(const VocabTrainArgs &a, hipStream_t s);
void launch_vocab_train_doc_words(const int32_t *word_id, int i0, int i1, const int32_t *doc_start, int d0, int d1, int n_words, uint32_t *bitmap,
                                  int32_t *ni, hipStream_t s);
// k_lm_marks / k_lm_list / k_lm_scan / k_lm_write (k_local_map.hip): Tracking::UpdateLocalPoints, the frame marks and map_points of
// SearchLocalPoints and K16 over them, compacted in order into the arrays jsorb_search_local_points_async reads
struct LocalMapArgs {
    jsorb_map_point_table t;
    jsorb_frustum_params p;
    int E, N, capacity;
    const int32_t *entry_row;                    // E: kf_point_row from the first keyframe's offset on
    const int32_t *frame_row;                    // N, or NULL
    // scratch
    uint32_t *word;                              // t.n_rows: bit 31 = not seen, the low bits the first entry with the row; all ones between calls
    uint8_t *keep;                               // E: the entry is a point inside the frustum
    uint32_t *chunk_sum, *chunk_pre;             // chunks, chunks + 1
    int32_t *stats;                              // E, null, invalid rows, duplicates, bad, seen
    // outputs
    int32_t *point_row, *level;
    float *u, *v, *invz, *view_cos;
    uint8_t *in_frustum, *mp_desc, *blocked_in;
    int32_t *counts;                             // 5
};
int local_map_chunk();                           // the compile-time cap of k_local_map.hip (jsorb_local_map_build_caps)
inline int local_map_chunks(int E) { return (E + local_map_chunk() - 1) / local_map_chunk(); }
void launch_local_map(const LocalMapArgs &a, hipStream_t s);      // the four kernels
void launch_map_points_scatter(int n_rows, float *const dst[9], uint8_t *bad, int n, const int32_t *rows, const jsorb_map_point_record *records, hipStream_t s);
// k_lk_marks / k_lk_votes / k_lk_rank / k_lk_expand / k_lk_gather (k_local_keyframes.hip): Tracking::UpdateLocalKeyFrames over the keyframe graph's
// device arrays, and the local keyframes' rows concatenated for launch_local_map
struct LocalKfArgs {
    jsorb_keyframe_graph g;
    int n_rows;                                  // of the map-point table
    const uint8_t *bad;                          // n_rows
    const int32_t *frame_row;                    // n_frame, or NULL
    int n_frame, kf_capacity, entry_capacity;
    // scratch
    uint32_t *word;                              // n_rows: all ones minus the row's multiplicity in the frame; all ones between calls
    int32_t *vote;                               // S
    uint8_t *first;                              // S: state == 1 && vote > 0 - the first list, and the membership beyond the LDS bitmap
    int32_t *order;                              // S: the first list in (order_key, slot) order
    unsigned long long *best;                    // 1: vote << 32 | ~rank of the voter with the largest vote, the lowest rank among equals
    int32_t *stats;                              // LK_STATS words, jsorb_local_keyframes_stats' order
    // in / out
    int32_t *local_kf_slot, *state_io;           // kf_capacity, 2
    // outputs
    int32_t *local_kf_start, *local_point_row, *counts;      // kf_capacity + 1, entry_capacity, 8
};
enum { LK_STATS = 8 };
int local_kf_member_lds();                       // the compile-time caps of k_local_keyframes.hip (jsorb_local_keyframes_build_caps)
int local_kf_child_lds();
void launch_local_keyframes(const LocalKfArgs &a, hipStream_t s);      // the five kernels
// k_cv_* (k_covisibility.hip): KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles / EraseConnection over the covisibility state's
// device arrays
enum { CV_MAX_UPDATE = 32 };
struct CovisArgs {
    jsorb_keyframe_graph g;
    jsorb_covisibility cv;
    int n_rows;                                  // of the map-point table
    const uint8_t *bad;                          // n_rows
    int n_update;
    const int32_t *update_slot;                  // n_update
    int32_t *neighbours;                         // S x 10, or NULL
    int32_t *parent_out;                         // n_update, or NULL
    int32_t *snap_slot, *snap_weight, *snap_len; // n_update x C twice and n_update, or all NULL
    int32_t *counts;                             // 8
    // scratch
    uint32_t *word;                              // n_rows: bit i = the row is in rows(update_slot[i]); all zero between calls
    int32_t *count;                              // 32 x S: cnt(update_slot[i], B)
    int32_t *kraw, *klist, *tlist;               // 32 x S each: K as found, K in (order_key, slot) order, T in the ordered list's order
    int32_t *minfo;                              // 32 x 4: the member's slot (-1 = skipped), |K|, |T|, the fallback slot or -1
    int32_t *stats;                              // KF_STATS words: the counts of the last call
};
int covis_cap_min();                             // the compile-time caps of k_covisibility.hip (jsorb_covisibility_build_caps)
int covis_cap_max();
void launch_update_connections(const CovisArgs &a, hipStream_t s);       // the five kernels
void launch_erase_connections(const jsorb_covisibility &cv, int32_t *neighbours, const int64_t *order_key, int slot, int32_t *counts, hipStream_t s);
void launch_erase_connections_dev(const jsorb_covisibility &cv, int32_t *neighbours, const int64_t *order_key, const int32_t *slot_dev, int32_t *counts,
                                  hipStream_t s);              // k_cv_erase for a slot in device memory (< 0: nothing); the slot's own map stays
void launch_connected_mask(const jsorb_covisibility &cv, int slot, uint8_t *mask, hipStream_t s);
void launch_best_covisibles(const jsorb_covisibility &cv, int n, const int32_t *slots, int N, int32_t *out, int32_t *out_len, hipStream_t s);
// k_kc_* (k_kf_culling.hip): LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag and MapPoint::EraseObservation / SetBadFlag over the keyframe
// graph, the map-point table and the covisibility state
enum { KC_MAX_CULL = 16, KC_MAX_CAND = 4096, KC_COUNTS = 10, KC_SCAN = 256 };
struct CullArgs {
    jsorb_keyframe_graph g;                      // order_key, point_off, point_len and the sizes; the arrays the call writes are read through `st`
    jsorb_covisibility cv;
    jsorb_keyframe_views v;
    jsorb_culling_state st;
    int n_rows, monocular, first_slot, n_cand, max_cull, reparent_cap;
    const int32_t *cand_slot;                    // n_cand
    int32_t *neighbours;                         // S x 10, or NULL
    // outputs
    int32_t *decision, *n_mps, *n_redundant;     // n_cand each
    int32_t *culled_slot, *reparent_out, *counts;// max_cull, reparent_cap x 2, 10
    // scratch
    int32_t *cnt, *fill, *off, *bsum;            // n_rows each: a row's observations, the scatter's cursor, the start inside its block of 256 rows;
                                                 // the blocks' starts
    int32_t *csr_slot, *csr_ent, *was_obs;       // pool_entries each: the observations grouped by row; the culled keyframe's erased entries
    int32_t *pmark, *ch_raw, *ch, *ch_done;      // S each: the parent candidates' stamp, the children as found, in (order_key, slot) order, reparented
    int32_t *ev;                                 // n_cand x 3: verdict (0 kept, 1 culled, 3 skipped), n_mps, n_redundant on the state of this round
    int32_t *ctl;                                // 8: the cursor, done, the slot culled in this round or -1, the keyframes culled so far
    int32_t *erase_counts;                       // 2: k_cv_erase's counts (not reported)
    int32_t *stats;                              // KC_COUNTS words: the counts of the last call
};
void launch_cull_keyframes(const CullArgs &a, hipStream_t s);
void launch_gather_counts(const int *countsL, const int *countsR, const int *stats, int32_t *dst, int n_pairs, hipStream_t s);
void launch_median(const Geometry &g, const int *countsL, float *u_right, float *depth, const int *best_l1, const unsigned *aux,
                   int *stats, int n_pairs, hipStream_t s, DeliverStereo dl = DeliverStereo{nullptr, nullptr, nullptr});

} // namespace jsorb
