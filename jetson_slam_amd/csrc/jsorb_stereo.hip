// jsorb_stereo.hip - host side of the stereo match (ComputeStereoMatches, orb_stereo_match.cu): batch and synchronous calls, their outputs
// and diagnostics, the speculative match of the single-frame call shape (struct jsorb_spec_state) and jsorb_gather_counts_async.
#include "jsorb_handle.h"

namespace {

StereoArgs make_stereo_args(float mb, float mbf, int th_high, int th_low)
{
    StereoArgs sa;
    sa.maxD = mbf / mb;                  // const float maxD = mbf/minZ  (orb_stereo_match.cu:144-146)
    sa.mbf = mbf;
    sa.th_high = th_high;
    sa.th_orb = (th_high + th_low) / 2;
    return sa;
}

// Called by a synchronous single-pair jsorb_stereo_match that ran the normal path: from now on the pair is matched speculatively.
int spec_arm(jsorb_extractor *l, jsorb_extractor *r, float mb, float mbf, int th_high, int th_low)
{
    if (l->st.spec && (l->st.spec->l != l || l->st.spec->r != r)) spec_detach(l->st.spec);
    if (r->st.spec && (r->st.spec->l != l || r->st.spec->r != r)) spec_detach(r->st.spec);
    if (!l->st.spec) {
        const size_t B = (size_t)l->B, T = (size_t)l->g.T;
        RCCHK(reserve_device(l, l->st.sp_u, B * T * 4));
        RCCHK(reserve_device(l, l->st.sp_d, B * T * 4));
        RCCHK(reserve_device(l, l->st.sp_stats, B * 8 * sizeof(int)));
        RCCHK(reserve_device(l, l->st.sp_l1, T * 4));
        RCCHK(reserve_device(l, l->st.sp_aux, T * 4));
        RCCHK(reserve_pinned(l, l->st.h_sp_u, T * sizeof(float)));
        RCCHK(reserve_pinned(l, l->st.h_sp_d, T * sizeof(float)));
        RCCHK(reserve_pinned(l, l->st.h_sp_stats, B * 8 * sizeof(int)));
        jsorb_spec_state *S = new (std::nothrow) jsorb_spec_state;
        if (!S) { l->err = "out of memory (speculative stereo)"; return JSORB_ERR_HIP; }
        if (hipEventCreateWithFlags(&S->ev_done, hipEventDisableTiming) != hipSuccess) { delete S; l->err = "hipEventCreate (speculative stereo)"; return JSORB_ERR_HIP; }
        S->l = l; S->r = r;
        l->st.spec = r->st.spec = S;
    }
    jsorb_spec_state *S = l->st.spec;
    std::lock_guard<std::mutex> lk(S->mu);
    S->armed = true;
    S->mb = mb; S->mbf = mbf; S->th_high = th_high; S->th_low = th_low;
    S->l_base = l->st.spec_seq;
    S->r_base = r->st.spec_seq;
    if (S->inflight) { S->inflight = false; S->n_dropped++; }
    return JSORB_OK;
}

} // namespace

namespace jsorb_host __attribute__((visibility("hidden"))) {

// The stereo outputs of a batch (allocated with the handle) and the pinned mirrors of a single pair.
int stereo_create(jsorb_extractor *e)
{
    const size_t B = (size_t)e->B, T = (size_t)e->g.T;
    HIPCHK(e, hipMalloc(&e->st.u, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st.d, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st.l1, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st.aux, B * T * 4));
    HIPCHK(e, hipMalloc(&e->st.stats, B * 8 * sizeof(int)));
    HIPCHK(e, hipHostMalloc(&e->st.h_stats, B * 8 * sizeof(int)));
    HIPCHK(e, hipHostMalloc(&e->st.h_u, T * sizeof(float)));
    HIPCHK(e, hipHostMalloc(&e->st.h_d, T * sizeof(float)));
    return JSORB_OK;
}

void stereo_after_extract(jsorb_extractor *e) { e->st.done = false; }

void stereo_release(jsorb_extractor *e)
{
    free_device(e->st.u, e->st.d, e->st.l1, e->st.stats, e->st.aux, e->st.diag, e->st.sp_u, e->st.sp_d, e->st.sp_stats, e->st.sp_l1, e->st.sp_aux);
    free_pinned(e->st.h_stats, e->st.h_u, e->st.h_d, e->st.h_sp_u, e->st.h_sp_d, e->st.h_sp_stats);
}

// ---- speculative stereo (struct jsorb_spec_state) ----
// Before a handle's buffers are rewritten: the speculative kernels of the previous frame read them (both handles' keypoints,
// descriptors, row tables and level images, the landing buffers included).  A single image is ordered on the GPU (its copy and
// kernels go to e->stream); a batch, whose copies and lanes use other streams, waits on the host (rare: a pair that alternates
// between the two call shapes).  Any new extract also invalidates a result nobody has asked for.
int spec_guard(jsorb_extractor *e, int n)
{
    jsorb_spec_state *S = e->st.spec;
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
    jsorb_spec_state *S = e->st.spec;
    if (!S) { e->st.spec_seq++; return; }
    std::lock_guard<std::mutex> lk(S->mu);
    e->st.spec_seq++;
    e->st.spec_single = n == 1 && !e->tm.on;
    jsorb_extractor *l = S->l, *r = S->r;
    if (!S->armed || !l->st.spec_single || !r->st.spec_single) return;
    if (l->st.spec_seq - S->l_base != r->st.spec_seq - S->r_base || l->st.spec_seq == S->l_base) return;     // not the same new frame on both sides (yet)
    // on the stream of the extract that was enqueued LAST (this one): it is the one that finishes last, so the match follows it in stream
    // order and the event of the other extract has usually fired by then (a cross-stream wait that is still pending when the GPU
    // reaches it costs ~20 us of idle time on this path).  Own scratch: a normal match on l's stream may follow while this one runs.
    jsorb_extractor *other = e == l ? r : l;
    hipStream_t st = e->lanes.used[0];
    bool ok = true;
    if (other->lanes.used[0] != st) ok = hipStreamWaitEvent(st, other->lanes.done[0], 0) == hipSuccess;
    if (ok) {
        const StereoArgs sa = make_stereo_args(S->mb, S->mbf, S->th_high, S->th_low);
        launch_stereo(l->g, l->src, l->slab, r->src, r->slab, l->out_kp, l->counts, l->desc, r->out_kp, r->counts, r->desc, r->row_tab,
                      l->st.sp_u, l->st.sp_d, l->st.sp_l1, l->st.sp_aux, sa, 1, st, nullptr);
        launch_median(l->g, l->counts, l->st.sp_u, l->st.sp_d, l->st.sp_l1, l->st.sp_aux, l->st.sp_stats, 1, st, DeliverStereo{l->st.h_sp_u, l->st.h_sp_d, l->st.h_sp_stats});
        ok = hipGetLastError() == hipSuccess && hipEventRecord(S->ev_done, st) == hipSuccess;
        // whatever went out on the stream reads both handles' buffers: their next extracts are ordered after it in any case
        S->wait_l = S->wait_r = true;
    }
    if (!ok) { S->armed = false; return; }
    S->inflight = true;
    S->l_seq = l->st.spec_seq;
    S->r_seq = r->st.spec_seq;
}

void spec_detach(jsorb_spec_state *S)
{
    if (!S) return;
    {
        std::lock_guard<std::mutex> lk(S->mu);
        S->armed = false;
        if (S->wait_l || S->wait_r || S->inflight) (void)hipEventSynchronize(S->ev_done);
    }
    if (S->l) S->l->st.spec = nullptr;
    if (S->r) S->r->st.spec = nullptr;
    if (S->ev_done) (void)hipEventDestroy(S->ev_done);
    delete S;
}

} // namespace jsorb_host

extern "C" {

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
    const bool aligned = l->lanes.K == r->lanes.K;
    const bool direct = n == 1;          // one pair: k_median writes uRight, depth and the statistics straight into the pinned host mirrors
    const size_t T = (size_t)l->g.T;
    const int CW = JSORB_MAX_LEVELS + 1;
    for (int j = 0; j < l->lanes.K; j++) {
        hipStream_t st = lane_stream(l, j);
        if (r != l) RCCHK(aligned ? wait_events(l, st, r->lanes.used + j, r->lanes.done + j, 1) : wait_lanes(l, st, r));
        const int f = l->lanes.first[j], m = l->lanes.first[j + 1] - f;
        ImageSrc srcL = l->src, srcR = r->src;
        srcL.l0 += (size_t)f * srcL.l0_stride;
        srcR.l0 += (size_t)f * srcR.l0_stride;
        const int skip_mask_st = experiment_env("JSORB_SKIP_KERNELS") ? atoi(experiment_env("JSORB_SKIP_KERNELS")) : 0;
        if (!((skip_mask_st >> JSORB_K_STEREO) & 1))
        TIMED(l, JSORB_K_STEREO, launch_stereo(l->g, srcL, l->slab + (size_t)f * l->g.slab_bytes, srcR, r->slab + (size_t)f * r->g.slab_bytes,
                                              l->out_kp + f * T * 6, l->counts + f * CW, l->desc + f * T * 32,
                                              r->out_kp + f * T * 6, r->counts + f * CW, r->desc + f * T * 32, r->row_tab + (size_t)f * r->g.row_tab_stride,
                                              l->st.u + f * T, l->st.d + f * T, l->st.l1 + f * T, l->st.aux + f * T, sa, m, st,
                                              l->st.diag ? l->st.diag + f * T * JSORB_STEREO_DIAG_INTS : nullptr));
        TIMED(l, JSORB_K_MEDIAN, launch_median(l->g, l->counts + f * CW, l->st.u + f * T, l->st.d + f * T, l->st.l1 + f * T, l->st.aux + f * T,
                                              l->st.stats + f * 8, m, st, direct ? DeliverStereo{l->st.h_u, l->st.h_d, l->st.h_stats} : DeliverStereo{nullptr, nullptr, l->st.h_stats + f * 8}));
        HIPCHK(l, hipGetLastError());
        HIPCHK(l, hipEventRecord(l->lanes.done[j], st));
        if (r != l) { HIPCHK(l, hipEventRecord(r->lanes.readers_done[j], st)); r->lanes.readers_stream[j] = st; }
        // the L1 refinement reads both level-0 planes in place: a landing buffer is free for the next upload only after this point
        if (l->land.last >= 0) HIPCHK(l, hipEventRecord(l->land.ev_consumed[l->land.last][j], st));
        if (r != l && r->land.last >= 0) HIPCHK(l, hipEventRecord(r->land.ev_consumed[r->land.last][j], st));
    }
    if (r != l) {
        r->lanes.has_readers = true;
        r->lanes.readers_K = l->lanes.K;
        r->lanes.readers_n = n;
        // the right handle's extract kernels finished before the left lanes started matching (waits above), so the left lanes'
        // events are the ones a refill of the right landing buffer has to wait for
        if (r->land.last >= 0) r->land.consumed_K[r->land.last] = l->lanes.K;
    }
    l->st.done = true;
    l->st.l1_view = l->st.l1;
    l->st.mirror_valid = false;
    l->st.mirror_pending = direct;
    l->st.pairs = n;
    l->counts_synced = false;
    return JSORB_OK;
}

const float *jsorb_stereo_uright_device(const jsorb_extractor *l, int image) { return (check_image(l, image) && l->st.done) ? l->st.u + (size_t)image * l->g.T : nullptr; }
const float *jsorb_stereo_depth_device(const jsorb_extractor *l, int image) { return (check_image(l, image) && l->st.done) ? l->st.d + (size_t)image * l->g.T : nullptr; }

int jsorb_copy_stereo(const jsorb_extractor *l, int image, float *u_right, float *depth, jsorb_stereo_stats *stats)
{
    if (!check_image(l, image) || !l->st.done) return JSORB_ERR_STATE;
    const int n = jsorb_n_keypoints(l, image);
    const bool mirror = l->st.mirror_valid && image == 0;
    RCCHK(copy_result(u_right, mirror ? l->st.h_u : nullptr, jsorb_stereo_uright_device(l, image), n, 4));
    RCCHK(copy_result(depth, mirror ? l->st.h_d : nullptr, jsorb_stereo_depth_device(l, image), n, 4));
    if (stats) {
        const int *s = l->st.h_stats + image * 8;
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
    if (!check_image(l, image) || !l->st.done || !dst || !l->st.l1_view) return JSORB_ERR_STATE;
    return copy_result(dst, nullptr, l->st.l1_view + (size_t)image * l->g.T, jsorb_n_keypoints(l, image), 4);
}

int jsorb_set_stereo_diagnostics(jsorb_extractor *l, int on)
{
    if (!l) return JSORB_ERR_INVALID;
    HIPCHK(l, hipSetDevice(l->device));
    if (on && !l->st.diag) {
        const size_t n = (size_t)l->B * l->g.T * JSORB_STEREO_DIAG_INTS * sizeof(int);
        HIPCHK(l, hipMalloc(&l->st.diag, n));
        HIPCHK(l, hipMemset(l->st.diag, 0xFF, n));
        // hipMemset on device memory returns before the fill has run, and the fill is ordered with the NULL stream only - the handles' streams are non-blocking.
        // Without this wait the fill could land on top of what the next k_stereo had already written: the arg-min / window-list diagnostics of a few hundred
        // keypoints read back as -1 while every product output was right (caught by tools/micro/chain_stress.py in round 5: 1 iteration in ~6 000; in all
        // likelihood also the "unexplained failure of the full GPU suite" of round 4, the round that introduced this hook and the test that reads it)
        HIPCHK(l, hipDeviceSynchronize());
    } else if (!on && l->st.diag) {
        HIPCHK(l, hipDeviceSynchronize());
        HIPCHK(l, hipFree(l->st.diag));
        l->st.diag = nullptr;
    }
    return JSORB_OK;
}
int jsorb_copy_stereo_diagnostics(const jsorb_extractor *l, int image, int32_t *dst)
{
    if (!check_image(l, image) || !l->st.done || !dst || !l->st.diag) return JSORB_ERR_STATE;
    return copy_result(dst, nullptr, l->st.diag + (size_t)image * l->g.T * JSORB_STEREO_DIAG_INTS, jsorb_n_keypoints(l, image), JSORB_STEREO_DIAG_INTS * 4);
}

int jsorb_gather_counts_async(jsorb_extractor *l, jsorb_extractor *r, int32_t *dev_dst)
{
    if (!l || !r || !dev_dst) return JSORB_ERR_INVALID;
    if (!l->st.done || l->n_images != r->n_images) { l->err = "gather_counts needs a finished stereo batch"; return JSORB_ERR_STATE; }
    HIPCHK(l, hipSetDevice(l->device));
    RCCHK(wait_lanes(l, l->stream, l));      // all lanes' statistics
    RCCHK(wait_lanes(l, l->stream, r));
    launch_gather_counts(l->counts, r->counts, l->st.stats, dev_dst, l->n_images, l->stream);
    HIPCHK(l, hipGetLastError());
    HIPCHK(l, hipEventRecord(l->lanes.done[0], l->stream));      // "everything of this handle so far" now includes the gather (it waited for every lane)
    // the next batch of either handle rewrites the count tables the gather kernel reads: their lanes continue after it
    return fork_lanes(l, l->stream, {l, r});
}

int jsorb_stereo_match(jsorb_extractor *l, jsorb_extractor *r, float mb, float mbf, int th_high, int th_low, float *u_right,
                       float *depth, jsorb_stereo_stats *stats)
{
    if (!l || !r) return JSORB_ERR_INVALID;
    const double t0 = l->trace.on ? now_us() : 0.0;
    bool adopt = false;
    if (jsorb_spec_state *S = l->st.spec) {
        // this very match may already be on the GPU, enqueued behind the two extracts (struct jsorb_spec_state)
        std::lock_guard<std::mutex> lk(S->mu);
        adopt = !l->st.diag && S->l == l && S->r == r && S->inflight && S->l_seq == l->st.spec_seq && S->r_seq == r->st.spec_seq && S->mb == mb && S->mbf == mbf &&
                S->th_high == th_high && S->th_low == th_low && l->extracted && r->extracted && l->n_images == 1 && r->n_images == 1 && !l->st.done;
        if (adopt) { S->inflight = false; S->n_adopted++; }
    }
    if (adopt) {
        HIPCHK(l, hipSetDevice(l->device));
        const double t1 = l->trace.on ? now_us() : 0.0;
        RCCHK(wait_event(l, l->st.spec->ev_done, l->spin_wait != 0));
        if (!l->counts_synced) RCCHK(jsorb_sync(l));          // extracts enqueued through the asynchronous calls
        std::swap(l->st.u, l->st.sp_u); std::swap(l->st.d, l->st.sp_d); std::swap(l->st.stats, l->st.sp_stats);
        std::swap(l->st.h_u, l->st.h_sp_u); std::swap(l->st.h_d, l->st.h_sp_d); std::swap(l->st.h_stats, l->st.h_sp_stats);
        l->st.done = true;
        l->st.l1_view = l->st.sp_l1;
        l->st.pairs = 1;
        l->st.mirror_valid = true;
        l->st.mirror_pending = false;
        if (l->trace.on) { l->trace.st_enq += t1 - t0; l->trace.st_wait += now_us() - t1; l->trace.st_n++; }
    } else {
        RCCHK(jsorb_stereo_match_batch_async(l, r, mb, mbf, th_high, th_low));
        const double t1 = l->trace.on ? now_us() : 0.0;
        RCCHK(jsorb_sync(l));
        if (l->trace.on) { l->trace.st_enq += t1 - t0; l->trace.st_wait += now_us() - t1; l->trace.st_n++; }
        if (l != r && l->st.speculate && l->n_images == 1 && !l->tm.on && !r->tm.on) RCCHK(spec_arm(l, r, mb, mbf, th_high, th_low));
    }
    RCCHK(jsorb_copy_stereo(l, 0, u_right, depth, stats));
    if (stats) stats->n_right = jsorb_n_keypoints(r, 0);
    return JSORB_OK;
}

int jsorb_set_speculative_stereo(jsorb_extractor *l, int on)
{
    if (!l) return JSORB_ERR_INVALID;
    l->st.speculate = l->st.speculate_env >= 0 ? l->st.speculate_env : (on ? 1 : 0);
    if (!l->st.speculate && l->st.spec) { (void)hipSetDevice(l->device); spec_detach(l->st.spec); }
    return JSORB_OK;
}

int jsorb_speculative_stereo_stats(const jsorb_extractor *l, long *n_adopted, long *n_dropped)
{
    if (!l) return JSORB_ERR_INVALID;
    long a = 0, d = 0;
    if (jsorb_spec_state *S = l->st.spec) { std::lock_guard<std::mutex> lk(S->mu); a = S->n_adopted; d = S->n_dropped; }
    if (n_adopted) *n_adopted = a;
    if (n_dropped) *n_dropped = d;
    return JSORB_OK;
}

} // extern "C"
