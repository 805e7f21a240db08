// jsorb_mappoints.hip - host side of what LocalMapping does to map points between two matcher calls, on the keyframe matcher (its stream, scratch
// of its own): jsorb_distinctive_descriptors* - MapPoint::ComputeDistinctiveDescriptors (MapPoint.cpp:273-338) for many points in one call.  The
// kernels are in k_distinct.hip.  The map itself (observations, isBad, Replace) stays with the caller, who hands the observations over as a CSR.
#include "jsorb_handle.h"      // struct jsorb_keyframe_matcher: shared with jsorb_keyframes.hip and jsorb_loop.hip

namespace {

const char *const DD = "distinctive_descriptors";

// the argument checks both forms share; outputs are checked by the form that owns them
int distinct_check(jsorb_keyframe_matcher *m, int n_points, const int32_t *obs_start, int n_obs, const int32_t *obs_row, const uint8_t *kf_desc, int n_rows,
                   int n_out_rows, const uint8_t *desc_out, const uint8_t *changed)
{
    if (n_points < 0 || n_obs < 0 || n_rows < 0 || n_out_rows < 0) return kf_fail(m, DD, "n_points, n_obs, n_rows and n_out_rows must not be negative");
    if (n_points > 0 && !obs_start) return kf_fail(m, DD, "NULL obs_start");
    if (n_points > 0 && n_obs > 0 && (!obs_row || !kf_desc)) return kf_fail(m, DD, "NULL obs_row or kf_desc");
    if ((uintptr_t)kf_desc % 16 || (uintptr_t)desc_out % 16) return kf_fail(m, DD, "descriptors must be 16-byte aligned");
    if (changed && !desc_out) return kf_fail(m, DD, "changed needs desc_out");
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_distinctive_descriptors_async(jsorb_keyframe_matcher *m, int n_points, const int32_t *obs_start, int n_obs, const int32_t *obs_row,
                                        const uint8_t *kf_desc, int n_rows, const int32_t *out_row, int n_out_rows, uint8_t *desc_out,
                                        uint8_t *changed, int32_t *best_obs, int32_t *best_median)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(distinct_check(m, n_points, obs_start, n_obs, obs_row, kf_desc, n_rows, n_out_rows, desc_out, changed));
    if (n_points > 0 && (!best_obs || !best_median)) return kf_fail(m, DD, "NULL best_obs or best_median");
    HIPCHK(m, hipSetDevice(m->device));
    KfCall &c = m->call[jsorb_keyframe_matcher::DISTINCT];
    RCCHK(reserve_device(m, c.stats, KF_STATS * sizeof(int)));
    const int want = std::max(n_points, 1);
    RCCHK(reserve_device(m, m->distinct.list, (size_t)3 * want * sizeof(int), &m->distinct.list_cap, want));
    hipStream_t st = m->stream;
    HIPCHK(m, hipMemsetAsync(c.stats, 0, KF_STATS * sizeof(int), st));
    c.done = true;
    DistinctArgs a{};
    a.n_points = n_points; a.n_obs = n_obs; a.n_rows = n_rows; a.n_out_rows = n_out_rows;
    a.obs_start = obs_start; a.obs_row = obs_row; a.kf_desc = kf_desc; a.out_row = out_row;
    a.list = m->distinct.list;
    a.best_obs = best_obs; a.best_median = best_median; a.desc_out = desc_out; a.changed = changed;
    a.stats = c.stats;
    launch_distinct(a, st);
    HIPCHK(m, hipGetLastError());
    return JSORB_OK;
}

int jsorb_distinctive_descriptors(jsorb_keyframe_matcher *m, int n_points, const int32_t *obs_start, int n_obs, const int32_t *obs_row,
                                  const uint8_t *kf_desc, int n_rows, const int32_t *out_row, int n_out_rows, uint8_t *desc_out, uint8_t *changed,
                                  int32_t *best_obs_host, int32_t *best_median_host)
{
    if (!m) return JSORB_ERR_INVALID;
    RCCHK(distinct_check(m, n_points, obs_start, n_obs, obs_row, kf_desc, n_rows, n_out_rows, desc_out, changed));
    if (n_points > 0 && (!best_obs_host || !best_median_host)) return kf_fail(m, DD, "NULL host output");
    HIPCHK(m, hipSetDevice(m->device));
    KfCall &c = m->call[jsorb_keyframe_matcher::DISTINCT];
    const int want = std::max(n_points, 1);
    RCCHK(reserve_device(m, c.out, (size_t)2 * want * sizeof(int32_t), &c.out_cap, want));
    RCCHK(jsorb_distinctive_descriptors_async(m, n_points, obs_start, n_obs, obs_row, kf_desc, n_rows, out_row, n_out_rows, desc_out, changed, c.out,
                                              c.out + want));
    if (n_points > 0) {
        HIPCHK(m, hipMemcpyAsync(best_obs_host, c.out, (size_t)n_points * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipMemcpyAsync(best_median_host, c.out + want, (size_t)n_points * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return JSORB_OK;
}

int jsorb_distinctive_descriptors_stats(jsorb_keyframe_matcher *m, int *n_group, int *n_wave, int *n_block, int *n_beyond_lds, int *n_empty, int *n_invalid,
                                        int *n_changed, int *largest_n)
{
    if (!m) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(m, m->call[jsorb_keyframe_matcher::DISTINCT], "distinctive_descriptors_stats before jsorb_distinctive_descriptors", s));
    int *const out[KF_STATS] = {n_group, n_wave, n_block, n_beyond_lds, n_empty, n_invalid, n_changed, largest_n};
    for (int i = 0; i < KF_STATS; i++)
        if (out[i]) *out[i] = s[i];
    return JSORB_OK;
}

int jsorb_distinct_build_caps(int *group_lanes, int *wave_max, int *lds_descriptors)
{
    if (group_lanes) *group_lanes = distinct_group_lanes();
    if (wave_max) *wave_max = distinct_wave_lanes();
    if (lds_descriptors) *lds_descriptors = distinct_lds_desc();
    return JSORB_OK;
}

} // extern "C"
