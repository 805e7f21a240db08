// jsorb_bow.hip - host side of the bag-of-words features: the device vocabulary (jsorb_vocabulary_*), the transform of a frame's descriptors
// (jsorb_bow_transform*) and the keyframe-to-frame matcher (jsorb_search_by_bow*, over jsorb_handle.h's kf_* frames).  The kernels are in k_bow.hip; the handle's part is `bow`
// (jsorb_handle.h), reset by every extract and released in jsorb_destroy.
#include "jsorb_handle.h"

// DBoW2's m_nodes on one device: the CSR of the children, their descriptors in child order, word id and weight > 0 per node - one allocation
struct jsorb_vocabulary {
    int device = 0;
    int n_nodes = 0, n_words = 0, depth_L = 0, levels_up = 0, max_children = 0;
    void *buf = nullptr;
    BowVocab dv{};
};

namespace jsorb_host __attribute__((visibility("hidden"))) {

void bow_after_extract(jsorb_extractor *e)
{
    std::fill(e->bow.have.begin(), e->bow.have.end(), 0);
}
void bow_release(jsorb_extractor *e) { free_device(e->bow.ids, e->bow.fsort, e->bow.ksort, e->bow.search.stats, e->bow.search.out); }

} // namespace jsorb_host

namespace {

const char *const BOW = "search_by_bow";

// the tree rooted at 0: every child id in [1, n) exactly once, every node reached, leaves with a word; its depth and widest node
bool vocabulary_check(int n, const int32_t *child_start, const int32_t *children, const int32_t *word_id, int *depth, int *max_children, int *n_words)
{
    if (child_start[0] != 0) return false;
    for (int i = 0; i < n; i++)
        if (child_start[i + 1] < child_start[i]) return false;
    if (child_start[n] != n - 1) return false;       // n - 1 child entries, each id once: every node but the root has one parent
    std::vector<char> seen((size_t)n, 0);
    for (int c = 0; c < n - 1; c++) {
        const int id = children[c];
        if (id < 1 || id >= n || seen[id]) return false;
        seen[id] = 1;
    }
    std::vector<int> level((size_t)n, -1), queue;
    queue.reserve((size_t)n);
    queue.push_back(0);
    level[0] = 0;
    *depth = 0; *max_children = 0; *n_words = 0;
    for (size_t h = 0; h < queue.size(); h++) {
        const int i = queue[h], b = child_start[i], e = child_start[i + 1];
        *max_children = std::max(*max_children, e - b);
        if (b == e) {
            if (word_id[i] < 0) return false;
            ++*n_words;
        }
        for (int c = b; c < e; c++) {
            level[children[c]] = level[i] + 1;
            *depth = std::max(*depth, level[i] + 1);
            queue.push_back(children[c]);
        }
    }
    return queue.size() == (size_t)n;                // a cycle among the other nodes is never reached from the root
}

int bow_reserve_ids(jsorb_extractor *e)
{
    const size_t BT = (size_t)e->B * e->g.T;
    RCCHK(reserve_device(e, e->bow.ids, (2 * BT + 2) * sizeof(int32_t)));
    if (e->bow.have.size() != (size_t)e->B) e->bow.have.assign((size_t)e->B, 0);
    return JSORB_OK;
}
int32_t *bow_words(const jsorb_extractor *e, int image) { return e->bow.ids + (size_t)image * e->g.T; }
int32_t *bow_nodes(const jsorb_extractor *e, int image) { return e->bow.ids + ((size_t)e->B + image) * e->g.T; }
int *bow_shallow(const jsorb_extractor *e) { return e->bow.ids + 2 * (size_t)e->B * e->g.T; }
bool bow_have(const jsorb_extractor *e, int image) { return check_image(e, image) && e->bow.ids && (size_t)image < e->bow.have.size() && e->bow.have[image]; }

} // namespace

extern "C" {

int jsorb_vocabulary_create(int device_id, int n_nodes, int depth_L, int levels_up, const int32_t *child_start, const int32_t *children,
                            const uint8_t *descriptors, const int32_t *word_id, const double *weight, jsorb_vocabulary **out)
{
    if (!out) return JSORB_ERR_INVALID;
    *out = nullptr;
    if (n_nodes < 2 || depth_L < 1 || depth_L > 16 || levels_up < 0 || device_id < 0 || !child_start || !children || !descriptors || !word_id || !weight)
        return JSORB_ERR_INVALID;
    int depth = 0, widest = 0, words = 0;
    const size_t n = (size_t)n_nodes, nc = n - 1;
    // the device image: child descriptors (32 nc), child_start (n + 1), children (nc), word (n) as int32, live (n bytes)
    const size_t o_start = 32 * nc, o_children = o_start + 4 * (n + 1), o_word = o_children + 4 * nc, o_live = o_word + 4 * n, bytes = o_live + n;
    std::vector<uint8_t> img;
    try {                                            // the host buffers are tens of megabytes at the ORB vocabulary's size: no exception leaves the C ABI
        if (!vocabulary_check(n_nodes, child_start, children, word_id, &depth, &widest, &words)) return JSORB_ERR_INVALID;
        if (depth > depth_L || widest >= (1 << 22)) return JSORB_ERR_INVALID;
        img.resize(bytes);
    } catch (const std::bad_alloc &) {
        return JSORB_ERR_HIP;
    }
    for (size_t c = 0; c < nc; c++) memcpy(&img[32 * c], descriptors + 32 * (size_t)children[c], 32);
    memcpy(&img[o_start], child_start, 4 * (n + 1));
    memcpy(&img[o_children], children, 4 * nc);
    memcpy(&img[o_word], word_id, 4 * n);
    for (size_t i = 0; i < n; i++) img[o_live + i] = weight[i] > 0 ? 1 : 0;
    jsorb_vocabulary *v = new (std::nothrow) jsorb_vocabulary;
    if (!v) return JSORB_ERR_HIP;
    v->device = device_id;
    v->n_nodes = n_nodes; v->n_words = words; v->depth_L = depth_L; v->levels_up = levels_up; v->max_children = widest;
    if (hipSetDevice(device_id) != hipSuccess || hipMalloc(&v->buf, bytes) != hipSuccess ||
        hipMemcpy(v->buf, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (v->buf) (void)hipFree(v->buf);
        delete v;
        return JSORB_ERR_HIP;
    }
    const uint8_t *base = static_cast<const uint8_t *>(v->buf);
    v->dv = BowVocab{reinterpret_cast<const int32_t *>(base + o_start), reinterpret_cast<const int32_t *>(base + o_children), base,
                     reinterpret_cast<const int32_t *>(base + o_word), base + o_live, depth_L, depth_L - levels_up};
    *out = v;
    return JSORB_OK;
}

void jsorb_vocabulary_destroy(jsorb_vocabulary *v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->buf) (void)hipFree(v->buf);               // (waits for the device: a transform may still read it)
    delete v;
}

int jsorb_vocabulary_info(const jsorb_vocabulary *v, int *n_nodes, int *n_words, int *depth_L, int *levels_up, int *max_children)
{
    if (!v) return JSORB_ERR_INVALID;
    if (n_nodes) *n_nodes = v->n_nodes;
    if (n_words) *n_words = v->n_words;
    if (depth_L) *depth_L = v->depth_L;
    if (levels_up) *levels_up = v->levels_up;
    if (max_children) *max_children = v->max_children;
    return JSORB_OK;
}

int jsorb_bow_build_caps(int *node_regs, int *sort_lds)
{
    if (node_regs) *node_regs = bow_node_regs();
    if (sort_lds) *sort_lds = bow_sort_lds();
    return JSORB_OK;
}

int jsorb_bow_transform_descriptors(void *hip_stream, const jsorb_vocabulary *v, int n, const uint8_t *descriptors, int32_t *word_id, int32_t *node_id)
{
    if (!v || n < 0 || (n > 0 && !descriptors) || (uintptr_t)descriptors % 16) return JSORB_ERR_INVALID;
    if (n == 0) return JSORB_OK;
    if (hipSetDevice(v->device) != hipSuccess) return JSORB_ERR_HIP;
    launch_bow_transform(v->dv, descriptors, 0, nullptr, 0, n, word_id, node_id, 0, nullptr, 1, (hipStream_t)hip_stream);
    return hipGetLastError() == hipSuccess ? JSORB_OK : JSORB_ERR_HIP;
}

int jsorb_bow_transform_async(jsorb_extractor *e, int image, const jsorb_vocabulary *v)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!v) { e->err = "bow_transform: NULL vocabulary"; return JSORB_ERR_INVALID; }
    if (v->device != e->device) { e->err = "bow_transform: the vocabulary lives on another device than the handle"; return JSORB_ERR_INVALID; }
    if (!e->extracted || image < -1 || image >= e->n_images) { e->err = "bow_transform: no extract result for this image"; return JSORB_ERR_STATE; }
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(bow_reserve_ids(e));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the descriptors may come from the lanes of a batch
    mark_main_stream(e);               // ... and the next batch's lanes must not rewrite them before the kernel has read them
    const int first = image < 0 ? 0 : image, count = image < 0 ? e->n_images : 1, CW = JSORB_MAX_LEVELS + 1;
    const size_t T = (size_t)e->g.T;
    HIPCHK(e, hipMemsetAsync(bow_shallow(e), 0, sizeof(int), st));
    // the keypoint counts are read on the device (a batch may not have been waited for); a count the host already has sizes the grid
    int n = (int)T;
    if (count == 1 && e->counts_synced) n = jsorb_n_keypoints(e, first);
    if (n > 0) {
        TIMED(e, JSORB_K_BOW_TRANSFORM, launch_bow_transform(v->dv, e->desc + first * T * 32, T * 32, e->counts + (size_t)first * CW + JSORB_MAX_LEVELS, CW, n,
                                                             bow_words(e, first), bow_nodes(e, first), T, bow_shallow(e), count, st));
        HIPCHK(e, hipGetLastError());
    }
    for (int i = first; i < first + count; i++) e->bow.have[i] = 1;
    e->bow.transformed = true;
    return JSORB_OK;
}

const int32_t *jsorb_bow_word_device(const jsorb_extractor *e, int image) { return bow_have(e, image) ? bow_words(e, image) : nullptr; }
const int32_t *jsorb_bow_node_device(const jsorb_extractor *e, int image) { return bow_have(e, image) ? bow_nodes(e, image) : nullptr; }

int jsorb_copy_bow(const jsorb_extractor *e, int image, int32_t *word_host, int32_t *node_host)
{
    if (!bow_have(e, image)) return JSORB_ERR_STATE;
    if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return JSORB_ERR_HIP;
    const int n = jsorb_n_keypoints(e, image);
    RCCHK(copy_result(word_host, nullptr, bow_words(e, image), n, sizeof(int32_t)));
    return copy_result(node_host, nullptr, bow_nodes(e, image), n, sizeof(int32_t));
}

int jsorb_bow_transform_stats(jsorb_extractor *e, int *n_shallow)
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s = 0;
    RCCHK(read_stats(e, e->bow.transformed, "bow_transform_stats before jsorb_bow_transform_async", bow_shallow(e), &s, 1));
    if (n_shallow) *n_shallow = s;
    return JSORB_OK;
}

int jsorb_search_by_bow_async(jsorb_extractor *e, int image, const jsorb_bow_params *params, const int32_t *f_node, int n_keyframes,
                              const int32_t *kf_start, const int32_t *kf_node, const uint8_t *kf_valid, const float *kf_angle,
                              const uint8_t *kf_descriptors, int32_t *match_kf, int32_t *n_matches_dev)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return kf_fail(e, BOW, "no extract result for this image", JSORB_ERR_STATE);
    if (!params) return kf_fail(e, BOW, "NULL params");
    RCCHK(kf_check_sizes(e, BOW, n_keyframes, 0, 0, nullptr));
    if (n_keyframes > 0 && (!kf_start || !n_matches_dev)) return kf_fail(e, BOW, "NULL kf_start or n_matches");
    const int N = jsorb_n_keypoints(e, image);
    if (N >= (1 << 18)) return kf_fail(e, BOW, "more than 262143 keypoints", JSORB_ERR_UNSUPPORTED);
    int rel[JSORB_BOW_MAX_KEYFRAMES + 1] = {0}, base = 0, total = 0;
    RCCHK(kf_rebase(e, BOW, kf_start, n_keyframes, rel, &base, &total, true));
    if (total > 0 && (!kf_node || !kf_valid || !kf_angle || !kf_descriptors)) return kf_fail(e, BOW, "NULL keyframe array");
    if ((uintptr_t)kf_descriptors % 16) return kf_fail(e, BOW, "kf_descriptors must be 16-byte aligned");
    if (n_keyframes > 0 && N > 0 && !match_kf) return kf_fail(e, BOW, "NULL match_kf");
    if (!f_node && N > 0 && n_keyframes > 0) {
        if (!bow_have(e, image)) return kf_fail(e, BOW, "f_node is NULL and this image has no jsorb_bow_transform_async since the last extract", JSORB_ERR_STATE);
        f_node = bow_nodes(e, image);
    }
    HIPCHK(e, hipSetDevice(e->device));
    RCCHK(reserve_device(e, e->bow.fsort, (size_t)std::max(e->g.T, 1) * sizeof(unsigned long long)));
    RCCHK(reserve_device(e, e->bow.ksort, (size_t)std::max(total, 1) * sizeof(unsigned long long), &e->bow.kf_cap, std::max(total, 1)));
    hipStream_t st = e->stream;
    RCCHK(wait_lanes(e, st, e));       // the frame may come from the lanes of a batch
    mark_main_stream(e);
    KfCall &c = e->bow.search;
    bool run = false;
    RCCHK(kf_clear(e, c, st, n_keyframes, N, total, n_matches_dev, match_kf, &run));
    if (!run) return JSORB_OK;
    BowMatchArgs a = bow_group_args(rel, f_node, N, n_keyframes, kf_node + base, e->bow.fsort, e->bow.ksort);
    a.desc = jsorb_descriptors_device(e, image);
    a.kf_valid = kf_valid + base; a.kf_desc = kf_descriptors + (size_t)32 * base;
    a.p = *params;
    a.match_kf = match_kf;
    a.stats = c.stats;
    TIMED(e, JSORB_K_BOW_GROUP, launch_bow_group(a, st));
    HIPCHK(e, hipGetLastError());
    TIMED(e, JSORB_K_BOW_MATCH, launch_bow_match(a, st));
    HIPCHK(e, hipGetLastError());
    // the rotation check: the keyframe's angle against the frame keypoint's (the angle plane of the keypoint SoA), the kept bins behind the three match words
    const float *f_angle = reinterpret_cast<const float *>(jsorb_keypoints_device(e, image) + 3 * (size_t)N);
    TIMED(e, JSORB_K_BOW_RESOLVE, launch_bow_resolve(row_resolve_args(rel, n_keyframes, N, f_angle, kf_angle + base, params->check_orientation, match_kf,
                                                                      n_matches_dev, c.stats + 3), st));
    HIPCHK(e, hipGetLastError());
    return JSORB_OK;
}

int jsorb_search_by_bow(jsorb_extractor *e, int image, const jsorb_bow_params *params, const int32_t *f_node, int n_keyframes,
                        const int32_t *kf_start, const int32_t *kf_node, const uint8_t *kf_valid, const float *kf_angle,
                        const uint8_t *kf_descriptors, int32_t *match_kf_host, int *n_matches_host)
{
    if (!e) return JSORB_ERR_INVALID;
    if (!check_image(e, image)) return kf_fail(e, BOW, "no extract result for this image", JSORB_ERR_STATE);      // (before n_keyframes: kept as it is)
    RCCHK(kf_check_sizes(e, BOW, n_keyframes, 0, 0, nullptr));
    const int N = jsorb_n_keypoints(e, image);
    return kf_sync(e, BOW, e->bow.search, n_keyframes, N, "N", !n_matches_host || (N > 0 && !match_kf_host), 1, match_kf_host, nullptr, n_matches_host,
                   [&](int32_t *cnt, int32_t *mk, int32_t *) {
                       return jsorb_search_by_bow_async(e, image, params, f_node, n_keyframes, kf_start, kf_node, kf_valid, kf_angle, kf_descriptors, mk, cnt);
                   });
}

int jsorb_search_by_bow_stats(jsorb_extractor *e, int *n_node_pairs, int *n_distances, int *largest_node, int kept_bins[3])
{
    if (!e) return JSORB_ERR_INVALID;
    int32_t s[KF_STATS] = {0};
    RCCHK(kf_stats(e, e->bow.search, "search_by_bow_stats before jsorb_search_by_bow", s));
    if (n_node_pairs) *n_node_pairs = s[0];
    if (n_distances) *n_distances = s[1];
    if (largest_node) *largest_node = s[2];
    if (kept_bins) for (int b = 0; b < 3; b++) kept_bins[b] = s[3 + b] - 1;
    return JSORB_OK;
}

} // extern "C"
