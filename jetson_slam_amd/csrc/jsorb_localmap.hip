// jsorb_localmap.hip - host side of the local map of Tracking::TrackLocalMap: jsorb_local_map_points* (UpdateLocalPoints, the frame marks, the
// map_points list and K16 in one call on the handle's stream, k_local_map.hip) and jsorb_map_points_scatter_async, which keeps the map-point table
// current.  The scratch is the handle's (struct lm, jsorb_handle.h): one word per table row, all ones between calls - every call sets back what it
// touched, so nothing here clears the table except after growth or a call whose launches were cut short.
#include "jsorb_handle.h"

namespace jsorb_host __attribute__((visibility("hidden"))) {

void local_map_release(jsorb_extractor *e) { free_device(e->lm.row.word, e->lm.keep, e->lm.chunk, e->lm.stats, e->lm.out); }

} // namespace jsorb_host

namespace {

const char *const LM = "local_map_points";

} // namespace

extern "C" {

int jsorb_local_map_points_async(jsorb_extractor *e, int image, const jsorb_map_point_table *table, const jsorb_frustum_params *prm, int n_keyframes,
                                 const int32_t *kf_start, const int32_t *kf_point_row, const int32_t *frame_point_row, int capacity,
                                 int32_t *point_row, float *u, float *v, float *invz, int32_t *predicted_level, float *view_cos, uint8_t *in_frustum,
                                 uint8_t *mp_descriptors, uint8_t *blocked_in, int32_t *counts_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return kf_fail(e, LM, "no extract result for this image", JSORB_ERR_STATE);
    if (!table || !prm || !counts_dev) return kf_fail(e, LM, "NULL table, prm or counts_dev");
    const jsorb_map_point_table &t = *table;
    if (t.n_rows < 0 || n_keyframes < 0 || capacity < 0) return kf_fail(e, LM, "n_rows, n_keyframes and capacity must not be negative");
    if (t.n_rows > 0 && (!t.Px || !t.Py || !t.Pz || !t.Pnx || !t.Pny || !t.Pnz || !t.MaxDistance || !t.invariance_maxDistance || !t.invariance_minDistance ||
                         !t.desc || !t.bad))
        return kf_fail(e, LM, "NULL table array");
    if (n_keyframes > 0 && !kf_start) return kf_fail(e, LM, "NULL kf_start");
    for (int i = 0; i < n_keyframes; i++)
        if (kf_start[i] < 0 || kf_start[i + 1] < kf_start[i]) return kf_fail(e, LM, "kf_start must be ascending offsets");
    const int first = n_keyframes > 0 ? kf_start[0] : 0, E = n_keyframes > 0 ? kf_start[n_keyframes] - first : 0;
    if (E >= (1 << 24)) return kf_fail(e, LM, "more than 16777215 entries");
    if (E > 0 && !kf_point_row) return kf_fail(e, LM, "NULL kf_point_row");
    if (capacity > 0 && (!point_row || !u || !v || !invz || !predicted_level || !view_cos || !in_frustum || !mp_descriptors)) return kf_fail(e, LM, "NULL output");
    if ((uintptr_t)t.desc % 16 || (uintptr_t)mp_descriptors % 16) return kf_fail(e, LM, "desc and mp_descriptors must be 16-byte aligned");
    const int N = jsorb_n_keypoints(e, image);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = e->stream;
    RCCHK(reserve_row_words(e, e->lm.row, t.n_rows, 0xff, st));      // the scratch: grown only; a word is all ones between calls
    const int chunks = local_map_chunks(E);
    RCCHK(reserve_device(e, e->lm.keep, (size_t)std::max(E, 1), &e->lm.entries, std::max(E, 1)));
    RCCHK(reserve_device(e, e->lm.chunk, ((size_t)2 * (chunks + 1) + 1) * sizeof(uint32_t), &e->lm.chunks, chunks + 1));
    RCCHK(reserve_device(e, e->lm.stats, 8 * sizeof(int32_t)));
    RCCHK(wait_lanes(e, st, e));       // the frame may come from the lanes of a batch
    mark_main_stream(e);
    LocalMapArgs a{};
    a.t = t; a.p = *prm;
    a.E = E; a.N = N; a.capacity = capacity;
    a.entry_row = E > 0 ? kf_point_row + first : nullptr;
    a.frame_row = frame_point_row;
    a.word = e->lm.row.word; a.keep = e->lm.keep;
    a.chunk_sum = e->lm.chunk; a.chunk_pre = e->lm.chunk + e->lm.chunks;
    a.stats = e->lm.stats;
    a.point_row = point_row; a.level = predicted_level; a.u = u; a.v = v; a.invz = invz; a.view_cos = view_cos;
    a.in_frustum = in_frustum; a.mp_desc = mp_descriptors; a.blocked_in = blocked_in;
    a.counts = counts_dev;
    e->lm.row.dirty = true;            // until all four kernels are enqueued: k_lm_write is the one that sets the words back
    launch_local_map(a, st);
    HIPCHK(e, hipGetLastError());
    e->lm.row.dirty = false;
    e->lm.done = true;
    return JSORB_OK;
}

int jsorb_local_map_points(jsorb_extractor *e, int image, const jsorb_map_point_table *table, const jsorb_frustum_params *prm, int n_keyframes,
                           const int32_t *kf_start, const int32_t *kf_point_row, const int32_t *frame_point_row, int capacity, int32_t *point_row,
                           float *u, float *v, float *invz, int32_t *predicted_level, float *view_cos, uint8_t *in_frustum, uint8_t *mp_descriptors,
                           uint8_t *blocked_in, int32_t *counts_dev, int32_t *point_row_host, int32_t counts_host[5])
{
    if (!e) return JSORB_ERR_INVALID;
    if (!counts_host || (capacity > 0 && !point_row_host)) return kf_fail(e, LM, "NULL host output");
    if (capacity < 0) return kf_fail(e, LM, "n_rows, n_keyframes and capacity must not be negative");
    HIPCHK(e, hipSetDevice(e->device));
    // The other way round than read_back: the asynchronous form writes into the staging buffer, and the results are copied out to the caller's
    // device arrays (point_row and counts_dev may be NULL here).  Left as it is.
    const int cap = std::max(capacity, 1);
    RCCHK(reserve_device(e, e->lm.out, ((size_t)8 + cap) * sizeof(int32_t), &e->lm.out_cap, cap));
    int32_t *cnt = e->lm.out, *rows = cnt + 8;
    RCCHK(jsorb_local_map_points_async(e, image, table, prm, n_keyframes, kf_start, kf_point_row, frame_point_row, capacity, rows, u, v, invz,
                                       predicted_level, view_cos, in_frustum, mp_descriptors, blocked_in, cnt));
    hipStream_t st = e->stream;
    if (point_row && capacity > 0) HIPCHK(e, hipMemcpyAsync(point_row, rows, (size_t)capacity * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    if (counts_dev) HIPCHK(e, hipMemcpyAsync(counts_dev, cnt, 5 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    std::vector<int32_t> h((size_t)8 + capacity);
    HIPCHK(e, hipMemcpyAsync(h.data(), cnt, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    memcpy(counts_host, h.data(), 5 * sizeof(int32_t));
    if (capacity > 0) memcpy(point_row_host, h.data() + 8, (size_t)capacity * sizeof(int32_t));
    return JSORB_OK;
}

int jsorb_local_map_stats(jsorb_extractor *e, int *n_entries, int *n_null, int *n_invalid_rows, int *n_duplicates, int *n_bad, int *n_seen)
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[6] = {0};
    RCCHK(read_stats(e, e->lm.done, "local_map_stats before jsorb_local_map_points", e->lm.stats, s, 6));
    int *const out[6] = {n_entries, n_null, n_invalid_rows, n_duplicates, n_bad, n_seen};
    for (int i = 0; i < 6; i++)
        if (out[i]) *out[i] = s[i];
    return JSORB_OK;
}

int jsorb_local_map_build_caps(int *scan_chunk)
{
    if (scan_chunk) *scan_chunk = local_map_chunk();
    return JSORB_OK;
}

int jsorb_map_points_scatter_async(void *hip_stream, int n_rows, float *Px, float *Py, float *Pz, float *Pnx, float *Pny, float *Pnz, float *MaxDistance,
                                   float *invariance_maxDistance, float *invariance_minDistance, uint8_t *bad, int n, const int32_t *rows,
                                   const jsorb_map_point_record *records)
{
    float *const dst[9] = {Px, Py, Pz, Pnx, Pny, Pnz, MaxDistance, invariance_maxDistance, invariance_minDistance};
    if (n < 0 || n_rows < 0) return JSORB_ERR_INVALID;
    if (n == 0) return JSORB_OK;
    if (n > 0 && (!rows || !records || !bad)) return JSORB_ERR_INVALID;
    for (int i = 0; i < 9 && n > 0; i++)
        if (!dst[i]) return JSORB_ERR_INVALID;
    launch_map_points_scatter(n_rows, dst, bad, n, rows, records, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

} // extern "C"
