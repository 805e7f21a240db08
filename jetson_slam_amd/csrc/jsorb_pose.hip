// jsorb_pose.hip - host side of Optimizer::PoseOptimization on the device: jsorb_pose_optimization* (Optimizer.cpp:244-456, one launch of
// k_pose_optimize for all problems of a call, k_pose.hip) on the extractor's handle and stream, and jsorb_apply_matches_async, the
// F.mvpMapPoints[bestIdx] = pMP between a matcher and the optimisation.  The scratch (a problem's edge list) and the synchronous form's buffers are
// the handle's (struct po, jsorb_handle.h), grown only.
#include "jsorb_handle.h"

namespace jsorb_host __attribute__((visibility("hidden"))) {

void pose_release(jsorb_extractor *e) { free_device(e->po.edges.p, e->po.stats, e->po.io.p); }

} // namespace jsorb_host

namespace {

const char *const PO = "pose_optimization";

} // namespace

extern "C" {

int jsorb_pose_optimization_async(jsorb_extractor *e, int image, const jsorb_pose_params *prm, const jsorb_map_point_table *table, int n_problems,
                                  const int32_t *frame_point_row, const float *u_right, const float *Tcw_in, float *Tcw_out, double *pose_out,
                                  uint8_t *outlier, int32_t *point_row_out, int32_t *counts_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return kf_fail(e, PO, "no extract result for this image", JSORB_ERR_STATE);
    if (!prm || !table) return kf_fail(e, PO, "NULL prm or table");
    if (n_problems < 0 || table->n_rows < 0) return kf_fail(e, PO, "n_problems and n_rows must not be negative");
    if (table->n_rows > 0 && (!table->Px || !table->Py || !table->Pz)) return kf_fail(e, PO, "NULL table array");
    if ((uintptr_t)table->desc % 16) return kf_fail(e, PO, "desc must be 16-byte aligned");
    const int N = jsorb_n_keypoints(e, image);
    if (n_problems > 0 && (!Tcw_in || !Tcw_out || !counts_dev)) return kf_fail(e, PO, "NULL Tcw_in, Tcw_out or counts_dev");
    if (n_problems > 0 && N > 0 && (!frame_point_row || !outlier)) return kf_fail(e, PO, "NULL frame_point_row or outlier");
    if ((uintptr_t)pose_out % sizeof(double)) return kf_fail(e, PO, "pose_out must be 8-byte aligned");
    if ((long long)n_problems * std::max(N, 1) >= (1ll << 31)) return kf_fail(e, PO, "n_problems x N too large", JSORB_ERR_UNSUPPORTED);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    RCCHK(reserve_words(e, e->po.edges, std::max((long long)n_problems * N, 1ll)));
    RCCHK(reserve_device(e, e->po.stats, PO_STATS * sizeof(int)));
    RCCHK(wait_lanes(e, st, e));       // the frame may come from the lanes of a batch
    mark_main_stream(e);
    PoseArgs a{};
    a.prm = *prm;
    a.delta_mono = (float)std::sqrt(5.991);          // Optimizer.cpp:278-279
    a.delta_stereo = (float)std::sqrt(7.815);
    a.soa = jsorb_keypoints_device(e, image);
    a.xy_un = jsorb_keypoints_un_device(e, image);
    a.N = N; a.n_rows = table->n_rows; a.n_problems = n_problems;
    a.Px = table->Px; a.Py = table->Py; a.Pz = table->Pz;
    a.frame_row = frame_point_row; a.u_right = u_right; a.Tcw_in = Tcw_in;
    a.Tcw_out = Tcw_out; a.pose_out = pose_out; a.outlier = outlier; a.row_out = point_row_out; a.counts = counts_dev;
    a.edge_kp = e->po.edges.p;
    a.stats = e->po.stats;
    HIPCHK(e, hipMemsetAsync(e->po.stats, 0, PO_STATS * sizeof(int), st));
    e->po.done = true;
    launch_pose_optimize(a, st);
    HIPCHK(e, hipGetLastError());
    return JSORB_OK;
}

int jsorb_pose_optimization(jsorb_extractor *e, int image, const jsorb_pose_params *prm, const jsorb_map_point_table *table, int n_problems,
                            const int32_t *frame_point_row, const float *u_right, const float *Tcw_host, float *Tcw_out_host,
                            double *pose_out_host, uint8_t *outlier_host, int32_t *point_row_out, int32_t *counts_host)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return kf_fail(e, PO, "no extract result for this image", JSORB_ERR_STATE);
    if (n_problems < 0) return kf_fail(e, PO, "n_problems and n_rows must not be negative");
    const int N = jsorb_n_keypoints(e, image);
    if (n_problems > 0 && (!Tcw_host || !Tcw_out_host || !counts_host || (N > 0 && !outlier_host))) return kf_fail(e, PO, "NULL host pose, flags or counts");
    if ((long long)n_problems * std::max(N, 1) >= (1ll << 31)) return kf_fail(e, PO, "n_problems x N too large", JSORB_ERR_UNSUPPORTED);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // the handle's buffer: the poses in double first (8-byte aligned), then Tcw_in, Tcw_out, the counts, the flags
    const long long np = std::max(n_problems, 1), flag_words = ((long long)n_problems * N + 3) / 4;
    RCCHK(reserve_words(e, e->po.io, np * (24 + 16 + 16 + 4) + flag_words));
    double *pose = (double *)e->po.io.p;
    float *tin = (float *)(e->po.io.p + np * 24), *tout = tin + np * 16;
    int32_t *cnt = (int32_t *)(tout + np * 16);
    uint8_t *flags = (uint8_t *)(cnt + np * 4);
    if (n_problems > 0) HIPCHK(e, hipMemcpyAsync(tin, Tcw_host, (size_t)n_problems * 16 * sizeof(float), hipMemcpyHostToDevice, st));
    RCCHK(jsorb_pose_optimization_async(e, image, prm, table, n_problems, frame_point_row, u_right, tin, tout, pose, flags, point_row_out, cnt));
    if (n_problems == 0) return JSORB_OK;
    HIPCHK(e, hipMemcpyAsync(Tcw_out_host, tout, (size_t)n_problems * 16 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (pose_out_host) HIPCHK(e, hipMemcpyAsync(pose_out_host, pose, (size_t)n_problems * 12 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(counts_host, cnt, (size_t)n_problems * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (N > 0) HIPCHK(e, hipMemcpyAsync(outlier_host, flags, (size_t)n_problems * N, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return JSORB_OK;
}

int jsorb_pose_optimization_stats(jsorb_extractor *e, int32_t stats[8])
{
    if (!e) return JSORB_ERR_INVALID;
    if (!stats) return kf_fail(e, PO, "NULL stats");
    return read_stats(e, e->po.done, "pose_optimization_stats before jsorb_pose_optimization", e->po.stats, stats, PO_STATS);
}

int jsorb_pose_optimization_build_caps(int *threads, int *edge_registers)
{
    if (threads) *threads = pose_threads();
    if (edge_registers) *edge_registers = pose_edge_regs();
    return JSORB_OK;
}

int jsorb_apply_matches_async(void *hip_stream, int n_points, const int32_t *point_row, const int32_t *match_kp, int N, int32_t *frame_point_row)
{
    if (n_points < 0 || N < 0) return JSORB_ERR_INVALID;
    if (n_points > 0 && (!point_row || !match_kp)) return JSORB_ERR_INVALID;
    if (n_points > 0 && N > 0 && !frame_point_row) return JSORB_ERR_INVALID;
    launch_apply_matches(n_points, point_row, match_kp, N, frame_point_row, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

} // extern "C"
