// jsorb_vocab_train.hip - host side of jsorb_vocabulary_train (include/jsorb.h): TemplatedVocabulary::create level by level.  The host keeps the
// tree (it reads the centres and member counts of every level), decides which children go on (:796-818), renumbers the nodes depth-first by
// blocks of siblings (:785-793) and takes the logarithms; the device does everything per descriptor (k_vocab_train.hip).  One word comes back per
// association pass.  The call owns its device memory and frees it before it returns; the result is a host object.
#include "jsorb_handle.h"

struct jsorb_vocab_train_result {
    int n = 0, k = 0, L = 0, weighting = 0, scoring = 0, n_nodes = 0, n_words = 0;
    std::vector<int32_t> parent, child_start, children, word_id, ni, leaf;
    std::vector<uint8_t> desc;
    std::vector<double> weight;
    int runs = 0, empty = 0, unconverged = 0;
    long long draws = 0;
    int passes[16] = {0};
};

namespace {

thread_local std::string vt_error;

struct Buf {                                     // a device array that only grows
    void *p = nullptr;
    size_t cap = 0;
};

struct Trainer {
    std::string err;
    hipStream_t stream = nullptr;
    std::vector<Buf *> bufs;                     // owned: the call's device memory
    jsorb_vocabulary *voc = nullptr;
    ~Trainer()
    {
        for (Buf *b : bufs) {
            if (b->p) (void)hipFree(b->p);
            delete b;
        }
        if (voc) jsorb_vocabulary_destroy(voc);
    }
    Buf &buf()
    {
        bufs.push_back(nullptr);
        return *(bufs.back() = new Buf);
    }
    int need(Buf &b, size_t bytes)
    {
        bytes = std::max<size_t>(bytes, 16);
        if (b.cap >= bytes) return JSORB_OK;
        if (b.p) { HIPCHK(this, hipStreamSynchronize(stream)); (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
        HIPCHK(this, hipMalloc(&b.p, bytes));
        b.cap = bytes;
        return JSORB_OK;
    }
    template <class T> int up(Buf &b, const std::vector<T> &v)
    {
        RCCHK(need(b, v.size() * sizeof(T)));
        if (!v.empty()) HIPCHK(this, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        return JSORB_OK;
    }
    template <class T> int down(std::vector<T> &v, const Buf &b, size_t count)
    {
        v.resize(count);
        if (count) HIPCHK(this, hipMemcpyAsync(v.data(), b.p, count * sizeof(T), hipMemcpyDeviceToHost, stream));
        return JSORB_OK;
    }
};

struct Segment { int parent, start, size; };

int train(Trainer &t, int device_id, const uint8_t *descriptors, int n, const int32_t *doc_start, int n_docs, int k, int L, unsigned long long seed,
          int max_iterations, jsorb_vocab_train_result &r)
{
    const size_t N = (size_t)n, chunks = (size_t)vocab_train_chunks(n);
    Buf *perm[2] = {&t.buf(), &t.buf()};
    Buf &seg_of = t.buf(), &assoc = t.buf(), &mind = t.buf(), &leaf = t.buf(), &chunk_sum = t.buf(), &chunk_pre = t.buf(), &hist = t.buf(),
        &hist_pre = t.buf(), &seg_start = t.buf(), &cslot = t.buf(), &seg_nc = t.buf(), &seg_j = t.buf(), &seg_changed = t.buf(), &centres = t.buf(),
        &cnt = t.buf(), &counters = t.buf(), &seg_rank = t.buf(), &dest_base = t.buf(), &node_base = t.buf(), &level_word = t.buf();
    RCCHK(t.need(*perm[0], N * 4)); RCCHK(t.need(*perm[1], N * 4)); RCCHK(t.need(seg_of, N * 4)); RCCHK(t.need(assoc, N)); RCCHK(t.need(mind, N * 4));
    RCCHK(t.need(leaf, N * 4)); RCCHK(t.need(chunk_sum, chunks * 4)); RCCHK(t.need(chunk_pre, (chunks + 1) * 8)); RCCHK(t.need(hist, chunks * k * 4));
    RCCHK(t.need(hist_pre, (chunks + 1) * k * 4)); RCCHK(t.need(level_word, 4));
    hipStream_t s = t.stream;
    launch_vocab_train_iota((int32_t *)perm[0]->p, n, s);
    HIPCHK(&t, hipMemsetAsync(leaf.p, 0, N * 4, s));

    // the tree in level order: node 0 the root
    std::vector<int32_t> tparent{-1}, tfirst{0}, tcount{0};
    std::vector<uint8_t> tdesc(32, 0);
    std::vector<Segment> segs{{0, 0, n}}, next;
    std::vector<int32_t> h_start, h_slot, h_nc, h_j, h_changed, h_dest, h_base;
    std::vector<uint32_t> h_cnt, h_centres;
    int cur = 0, m = n;
    for (int level = 1; !segs.empty(); level++) {
        const int S = (int)segs.size();
        h_start.resize((size_t)S + 1); h_slot.resize(S);
        int slots = 0;
        for (int i = 0; i < S; i++) {
            h_start[i] = segs[i].start;
            h_slot[i] = segs[i].size > k ? slots++ : -1;
        }
        h_start[S] = m;
        const size_t SK = (size_t)S * k;
        RCCHK(t.up(seg_start, h_start)); RCCHK(t.up(cslot, h_slot));
        RCCHK(t.need(seg_nc, (size_t)S * 4)); RCCHK(t.need(seg_j, (size_t)S * 4)); RCCHK(t.need(seg_changed, (size_t)S * 4));
        RCCHK(t.need(centres, SK * 32)); RCCHK(t.need(cnt, SK * 4)); RCCHK(t.need(counters, (size_t)slots * k * 1024));
        RCCHK(t.need(seg_rank, SK * 4));
        HIPCHK(&t, hipMemsetAsync(cnt.p, 0, SK * 4, s));
        HIPCHK(&t, hipMemsetAsync(centres.p, 0, SK * 32, s));
        if (slots) HIPCHK(&t, hipMemsetAsync(counters.p, 0, (size_t)slots * k * 1024, s));
        HIPCHK(&t, hipMemsetAsync(assoc.p, 0xff, (size_t)m, s));
        HIPCHK(&t, hipMemsetAsync(level_word.p, 0, 4, s));
        VocabTrainArgs a{};
        a.m = m; a.S = S; a.k = k; a.seed = seed;
        a.rows = descriptors; a.perm = (const int32_t *)perm[cur]->p; a.seg_start = (const int32_t *)seg_start.p; a.cslot = (const int32_t *)cslot.p;
        a.seg_of = (int32_t *)seg_of.p; a.seg_nc = (int32_t *)seg_nc.p; a.seg_j = (int32_t *)seg_j.p; a.seg_changed = (int32_t *)seg_changed.p;
        a.centres = (uint32_t *)centres.p; a.cnt = (uint32_t *)cnt.p; a.counters = (uint32_t *)counters.p; a.assoc = (uint8_t *)assoc.p;
        a.mind = (uint32_t *)mind.p; a.chunk_sum = (uint32_t *)chunk_sum.p; a.chunk_pre = (unsigned long long *)chunk_pre.p;
        a.level_word = (int32_t *)level_word.p; a.hist = (uint32_t *)hist.p; a.hist_pre = (uint32_t *)hist_pre.p; a.seg_rank = (uint32_t *)seg_rank.p;
        a.leaf = (int32_t *)leaf.p;
        launch_vocab_train_seed(a, s);
        HIPCHK(&t, hipGetLastError());
        int pass = 0;
        bool capped = false;
        for (;;) {
            launch_vocab_train_assign(a, ++pass, s);
            HIPCHK(&t, hipGetLastError());
            if (!slots) break;                   // only trivial runs: nothing iterates
            int32_t word = 0;
            HIPCHK(&t, hipMemcpyAsync(&word, level_word.p, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(&t, hipStreamSynchronize(s));
            if (word != pass) break;             // :764-771 for every run of the level
            if (pass == max_iterations) { capped = true; break; }
            launch_vocab_train_means(a, s);
        }
        r.passes[level - 1] = slots ? pass : 0;
        RCCHK(t.down(h_nc, seg_nc, S)); RCCHK(t.down(h_j, seg_j, S)); RCCHK(t.down(h_cnt, cnt, SK)); RCCHK(t.down(h_centres, centres, SK * 8));
        if (capped) RCCHK(t.down(h_changed, seg_changed, S));
        HIPCHK(&t, hipStreamSynchronize(s));
        // the level's nodes (:785-793) and the runs of the next one (:796-818)
        h_dest.assign(SK, -1); h_base.resize(S);
        next.clear();
        long long m_next = 0;
        for (int i = 0; i < S; i++) {
            const int nc = h_nc[i];
            long long members = 0;
            if (nc < 1 || nc > k) return kf_fail(&t, "vocabulary_train", "the device's centre count is out of range", JSORB_ERR_STATE);
            h_base[i] = (int32_t)tparent.size();
            tfirst[segs[i].parent] = h_base[i]; tcount[segs[i].parent] = nc;
            for (int c = 0; c < nc; c++) {
                const uint32_t cn = h_cnt[(size_t)i * k + c];
                const int id = (int)tparent.size();
                members += cn;
                tparent.push_back(segs[i].parent); tfirst.push_back(0); tcount.push_back(0);
                const uint8_t *d = reinterpret_cast<const uint8_t *>(&h_centres[((size_t)i * k + c) * 8]);
                tdesc.insert(tdesc.end(), d, d + 32);
                if (h_slot[i] >= 0 && cn == 0) r.empty++;
                if (level < L && cn > 1) {
                    h_dest[(size_t)i * k + c] = (int32_t)m_next;
                    next.push_back(Segment{id, (int)m_next, (int)cn});
                    m_next += cn;
                }
            }
            if (members != segs[i].size) return kf_fail(&t, "vocabulary_train", "the device's member counts do not add up", JSORB_ERR_STATE);
            if (h_slot[i] >= 0) { r.runs++; r.draws += h_j[i]; }
            if (capped && h_slot[i] >= 0 && h_changed[i] == pass) r.unconverged++;
        }
        RCCHK(t.up(dest_base, h_dest)); RCCHK(t.up(node_base, h_base));
        a.dest_base = (const int32_t *)dest_base.p; a.node_base = (const int32_t *)node_base.p; a.m_next = (int)m_next;
        a.perm_out = (int32_t *)perm[1 - cur]->p;
        launch_vocab_train_regroup(a, s);
        HIPCHK(&t, hipGetLastError());
        HIPCHK(&t, hipStreamSynchronize(s));
        cur = 1 - cur;
        m = (int)m_next;
        segs.swap(next);
    }

    // DBoW2's node ids: a run's clusters are consecutive, then the recursion into each of them in turn
    const int n_nodes = (int)tparent.size();
    std::vector<int32_t> new_id((size_t)n_nodes, 0), old_id((size_t)n_nodes, 0);
    {
        int next_id = 1;
        std::vector<std::pair<int, int>> stack{{0, -1}};     // (node, the child the recursion is at; -1: number the children first)
        while (!stack.empty()) {
            auto &[u, i] = stack.back();
            if (i < 0) {
                for (int c = 0; c < tcount[u]; c++) new_id[tfirst[u] + c] = next_id++;
                i = 0;
            }
            while (i < tcount[u] && tcount[tfirst[u] + i] == 0) i++;
            if (i == tcount[u]) { stack.pop_back(); continue; }
            const int child = tfirst[u] + i++;
            stack.push_back({child, -1});
        }
        for (int u = 0; u < n_nodes; u++) old_id[new_id[u]] = u;
    }
    r.n_nodes = n_nodes;
    r.parent.assign(n_nodes, -1); r.child_start.assign((size_t)n_nodes + 1, 0); r.children.resize((size_t)n_nodes - 1); r.word_id.assign(n_nodes, -1);
    r.desc.assign((size_t)n_nodes * 32, 0); r.weight.assign(n_nodes, 0.0); r.ni.assign(n_nodes, 0);
    int words = 0, filled = 0;
    for (int v = 0; v < n_nodes; v++) {
        const int u = old_id[v];
        if (v > 0) {
            r.parent[v] = new_id[tparent[u]];
            memcpy(&r.desc[(size_t)v * 32], &tdesc[(size_t)u * 32], 32);
            if (tcount[u] == 0) r.word_id[v] = words++;
        }
        r.child_start[v] = filled;
        for (int c = 0; c < tcount[u]; c++) r.children[filled++] = new_id[tfirst[u] + c];
    }
    r.child_start[n_nodes] = filled;
    r.n_words = words;
    RCCHK(t.down(r.leaf, leaf, N));

    // Ni (:962-983): the transform of every training descriptor on the finished tree, then one bit per (document, word)
    std::vector<double> ones((size_t)n_nodes, 1.0);
    if (jsorb_vocabulary_create(device_id, n_nodes, L, 0, r.child_start.data(), r.children.data(), r.desc.data(), r.word_id.data(), ones.data(), &t.voc) != JSORB_OK)
        return kf_fail(&t, "vocabulary_train", "the trained tree was refused by jsorb_vocabulary_create", JSORB_ERR_STATE);
    int32_t *word_dev = (int32_t *)seg_of.p;
    if (jsorb_bow_transform_descriptors(s, t.voc, n, descriptors, word_dev, nullptr) != JSORB_OK)
        return kf_fail(&t, "vocabulary_train", "jsorb_bow_transform_descriptors failed", JSORB_ERR_HIP);
    Buf &ni = t.buf(), &bitmap = t.buf(), &docs = t.buf();
    const size_t row_bytes = ((size_t)words + 31) / 32 * 4;
    const int batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_docs, ((size_t)256 << 20) / row_bytes));
    RCCHK(t.need(ni, (size_t)words * 4)); RCCHK(t.need(bitmap, (size_t)batch * row_bytes)); RCCHK(t.need(docs, ((size_t)n_docs + 1) * 4));
    HIPCHK(&t, hipMemsetAsync(ni.p, 0, (size_t)words * 4, s));
    HIPCHK(&t, hipMemcpyAsync(docs.p, doc_start, ((size_t)n_docs + 1) * 4, hipMemcpyHostToDevice, s));
    for (int d0 = 0; d0 < n_docs; d0 += batch) {
        const int d1 = std::min(n_docs, d0 + batch);
        HIPCHK(&t, hipMemsetAsync(bitmap.p, 0, (size_t)(d1 - d0) * row_bytes, s));
        launch_vocab_train_doc_words(word_dev, doc_start[d0], doc_start[d1], (const int32_t *)docs.p, d0, d1, words, (uint32_t *)bitmap.p, (int32_t *)ni.p, s);
        HIPCHK(&t, hipGetLastError());
    }
    std::vector<int32_t> h_ni;
    RCCHK(t.down(h_ni, ni, words));
    HIPCHK(&t, hipStreamSynchronize(s));
    for (size_t i = 0; i < N; i++) {
        if (r.leaf[i] < 0 || r.leaf[i] >= n_nodes) return kf_fail(&t, "vocabulary_train", "the device's leaf of a descriptor is out of range", JSORB_ERR_STATE);
        r.leaf[i] = new_id[r.leaf[i]];
    }
    for (int v = 1; v < n_nodes; v++) {
        const int w = r.word_id[v];
        if (w < 0) continue;
        r.ni[v] = h_ni[w];
        if (r.weighting == 1 || r.weighting == 3) r.weight[v] = 1;                                            // :949-954
        else if (h_ni[w] > 0) r.weight[v] = log((double)n_docs / (double)h_ni[w]);                            // :990
    }
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_vocabulary_train(int device_id, void *hip_stream, const uint8_t *descriptors, int n, const int32_t *doc_start, int n_docs, int k, int depth_L,
                           int weighting, int scoring, uint64_t seed, int max_iterations, jsorb_vocab_train_result **out)
{
    const auto refuse = [](const char *what) { vt_error = std::string("vocabulary_train: ") + what; return JSORB_ERR_INVALID; };
    if (!out) return refuse("NULL out");
    *out = nullptr;
    if (device_id < 0) return refuse("device_id must not be negative");
    if (n < 1 || n > (1 << 30)) return refuse("n must be in [1, 2^30]");
    if (!descriptors || (uintptr_t)descriptors % 16) return refuse("descriptors must be a 16-byte aligned device pointer");
    if (k < 2 || k > 32) return refuse("k must be in [2, 32]");
    if (depth_L < 1 || depth_L > 16) return refuse("depth_L must be in [1, 16]");
    long long expected = 1, power = 1;           // :565 in integers
    for (int l = 1; l <= depth_L; l++) {
        power *= k;
        expected += power;
        if (expected > INT_MAX) return refuse("1 + k + ... + k^depth_L does not fit int32");
    }
    if (weighting < 0 || weighting > 3 || scoring < 0 || scoring > 5) return refuse("weighting must be in [0, 3] and scoring in [0, 5]");
    if (max_iterations < 0) return refuse("max_iterations must not be negative");
    if (!doc_start || n_docs < 1) return refuse("doc_start must hold n_docs + 1 >= 2 offsets");
    if (doc_start[0] != 0 || doc_start[n_docs] != n) return refuse("doc_start must run from 0 to n");
    for (int d = 0; d < n_docs; d++)
        if (doc_start[d + 1] < doc_start[d]) return refuse("doc_start must ascend");
    if (hipSetDevice(device_id) != hipSuccess) { (void)hipGetLastError(); vt_error = "vocabulary_train: hipSetDevice failed"; return JSORB_ERR_HIP; }
    jsorb_vocab_train_result *r = nullptr;
    int rc;
    try {                                        // the host arrays grow with the tree: no exception leaves the C ABI
        r = new jsorb_vocab_train_result;
        r->n = n; r->k = k; r->L = depth_L; r->weighting = weighting; r->scoring = scoring;
        Trainer t;
        t.stream = (hipStream_t)hip_stream;
        rc = train(t, device_id, descriptors, n, doc_start, n_docs, k, depth_L, seed, max_iterations ? max_iterations : 1000, *r);
        if (rc != JSORB_OK) {
            vt_error = t.err;
            (void)hipStreamSynchronize(t.stream);    // nothing of the call is in flight when its memory goes
            (void)hipGetLastError();
        }
    } catch (const std::bad_alloc &) {
        vt_error = "vocabulary_train: out of host memory";
        rc = JSORB_ERR_HIP;
    }
    if (rc != JSORB_OK) { delete r; return rc; }
    *out = r;
    return JSORB_OK;
}

const char *jsorb_vocabulary_train_last_error(void) { return vt_error.c_str(); }

void jsorb_vocab_train_result_destroy(jsorb_vocab_train_result *r) { delete r; }

int jsorb_vocab_train_result_info(const jsorb_vocab_train_result *r, int *n_nodes, int *n_words, int *n, int *k, int *depth_L, int *weighting, int *scoring)
{
    if (!r) return JSORB_ERR_INVALID;
    if (n_nodes) *n_nodes = r->n_nodes;
    if (n_words) *n_words = r->n_words;
    if (n) *n = r->n;
    if (k) *k = r->k;
    if (depth_L) *depth_L = r->L;
    if (weighting) *weighting = r->weighting;
    if (scoring) *scoring = r->scoring;
    return JSORB_OK;
}

int jsorb_vocab_train_result_copy(const jsorb_vocab_train_result *r, int32_t *parent, int32_t *child_start, int32_t *children, uint8_t *descriptors,
                                  int32_t *word_id, double *weight, int32_t *Ni)
{
    if (!r) return JSORB_ERR_INVALID;
    const size_t nn = (size_t)r->n_nodes;
    if (parent) memcpy(parent, r->parent.data(), nn * 4);
    if (child_start) memcpy(child_start, r->child_start.data(), (nn + 1) * 4);
    if (children) memcpy(children, r->children.data(), (nn - 1) * 4);
    if (descriptors) memcpy(descriptors, r->desc.data(), nn * 32);
    if (word_id) memcpy(word_id, r->word_id.data(), nn * 4);
    if (weight) memcpy(weight, r->weight.data(), nn * 8);
    if (Ni) memcpy(Ni, r->ni.data(), nn * 4);
    return JSORB_OK;
}

int jsorb_vocab_train_result_copy_assignment(const jsorb_vocab_train_result *r, int32_t *node_of_descriptor)
{
    if (!r || !node_of_descriptor) return JSORB_ERR_INVALID;
    memcpy(node_of_descriptor, r->leaf.data(), (size_t)r->n * 4);
    return JSORB_OK;
}

int jsorb_vocab_train_stats(const jsorb_vocab_train_result *r, int *n_kmeans_runs, long long *n_draws, int *n_empty_clusters, int *n_unconverged,
                            int *lloyd_passes)
{
    if (!r) return JSORB_ERR_INVALID;
    if (n_kmeans_runs) *n_kmeans_runs = r->runs;
    if (n_draws) *n_draws = r->draws;
    if (n_empty_clusters) *n_empty_clusters = r->empty;
    if (n_unconverged) *n_unconverged = r->unconverged;
    if (lloyd_passes) memcpy(lloyd_passes, r->passes, sizeof r->passes);
    return JSORB_OK;
}

int jsorb_vocab_train_build_caps(int *chunk, int *scan_threads)
{
    if (chunk) *chunk = vocab_train_chunk();
    if (scan_threads) *scan_threads = vocab_train_scan_threads();
    return JSORB_OK;
}

} // extern "C"
