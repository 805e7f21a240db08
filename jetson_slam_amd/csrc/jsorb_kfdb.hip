// jsorb_kfdb.hip - host side of the keyframe database (jsorb_keyframe_database_*, jsorb_bow_vector_async, jsorb_detect_*_candidates*): KeyFrameDatabase
// (KeyFrameDatabase.cpp:44-313) with DBoW2's BowVector fold and L1 score, on the device.  The database is an object of its own - its stream, its
// scratch, its error text - in the manner of the keyframe matcher; the kernels are in k_kfdb.hip.  Everything per slot is allocated at create
// (max_keyframes is fixed), so no query allocates; the pool of the keyframes' BowVectors grows in add, and the sort scratch of
// jsorb_bow_vector_async with the largest n beyond the LDS cap.
#include "jsorb_handle.h"

struct jsorb_keyframe_database {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev_switch = nullptr;
    bool used = false;                           // something was enqueued: a new stream continues after the old one
    int max_kf = 0, n_words = 0;
    double *weight = nullptr;                    // n_words leaf weights by word id (device)
    void *slab = nullptr;                        // everything per slot, carved below
    KfdbState st{};
    unsigned long long *key = nullptr;
    float *tscore = nullptr, *ent_acc = nullptr;
    int32_t *first_pos = nullptr, *list = nullptr, *ent_flag = nullptr, *ent_best = nullptr, *cand = nullptr, *ctrl = nullptr;
    // the pool (host bookkeeping: the device only sees offsets)
    int pool_cap = 0, pool_top = 0;
    std::vector<std::pair<int, int>> holes;      // (offset, entries) of erased keyframes below pool_top
    std::vector<char> present;                   // host mirror of st.present
    std::vector<int> slot_off, slot_cap;
    uint32_t next_seq = 0;
    uint32_t *sort = nullptr;                    // k_kfdb_bow_vector's keys beyond the LDS cap: grown only
    int sort_cap = 0;
    bool queried = false;
    std::string err;
};

namespace {

const char *const KD = "keyframe_database", *const BV = "bow_vector", *const SC = "keyframe_database_score", *const DL = "detect_loop_candidates",
           *const DR = "detect_relocalization_candidates";

int vector_check(jsorb_keyframe_database *db, const char *name, const int32_t *word, const double *value, int cap, const int32_t *n_dev)
{
    if (cap < 0) return kf_fail(db, name, "a BowVector's capacity must not be negative");
    if (!n_dev) return kf_fail(db, name, "NULL BowVector count");
    if (cap > 0 && (!word || !value)) return kf_fail(db, name, "NULL BowVector array");
    return JSORB_OK;
}

int query(jsorb_keyframe_database *db, const char *name, int reloc, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
          unsigned long long id, const uint8_t *connected, const int32_t *neighbours, float min_score, const float *min_score_dev, int32_t *candidates,
          int32_t *n_candidates_dev)
{
    RCCHK(vector_check(db, name, q_word, q_value, q_cap, q_n_dev));
    if (!neighbours || !candidates || !n_candidates_dev) return kf_fail(db, name, "NULL neighbours, candidates or n_candidates");
    HIPCHK(db, hipSetDevice(db->device));
    hipStream_t s = db->stream;
    HIPCHK(db, hipMemsetAsync(db->ctrl, 0, KFDB_CTRL * sizeof(int32_t), s));
    HIPCHK(db, hipMemsetAsync(n_candidates_dev, 0, sizeof(int32_t), s));
    db->used = db->queried = true;
    KfdbQueryArgs a{};
    a.st = db->st;
    a.q = KfdbVector{q_word, q_value, q_n_dev, q_cap};
    a.id = id; a.reloc = reloc; a.connected = connected; a.neighbours = neighbours; a.min_score = min_score; a.min_score_dev = min_score_dev;
    a.key = db->key; a.tscore = db->tscore; a.first_pos = db->first_pos; a.list = db->list; a.ent_flag = db->ent_flag; a.ent_best = db->ent_best;
    a.ent_acc = db->ent_acc; a.ctrl = db->ctrl; a.candidates = candidates; a.n_candidates = n_candidates_dev;
    launch_kfdb_query(a, s);                     // nothing for a database no keyframe was added to
    HIPCHK(db, hipGetLastError());
    return JSORB_OK;
}

int query_host(jsorb_keyframe_database *db, const char *name, int32_t *candidates_host, int *n_candidates_host)
{
    int32_t n = 0;
    HIPCHK(db, hipMemcpyAsync(&n, db->cand + db->max_kf, sizeof(int32_t), hipMemcpyDeviceToHost, db->stream));
    HIPCHK(db, hipStreamSynchronize(db->stream));
    if (n < 0 || n > db->max_kf) return kf_fail(db, name, "the device count is out of range", JSORB_ERR_STATE);
    if (n > 0) HIPCHK(db, hipMemcpy(candidates_host, db->cand, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_candidates_host = n;
    return JSORB_OK;
}

} // namespace

extern "C" {

int jsorb_keyframe_database_create(int device_id, int max_keyframes, int n_words, const double *word_weight, jsorb_keyframe_database **out)
{
    if (!out) return JSORB_ERR_INVALID;
    *out = nullptr;
    if (device_id < 0 || max_keyframes < 1 || max_keyframes > (1 << 24) || n_words < 1 || !word_weight) return JSORB_ERR_INVALID;
    jsorb_keyframe_database *db = new (std::nothrow) jsorb_keyframe_database;
    if (!db) return JSORB_ERR_HIP;
    db->device = device_id; db->max_kf = max_keyframes; db->n_words = n_words;
    const size_t M = (size_t)max_keyframes;
    // the carve: 8-byte arrays first, every array a multiple of 16 bytes
    const auto r16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t b8 = r16(M * 8), b4 = r16(M * 4), bytes = 3 * b8 + 14 * b4 + r16((M + 1) * 4) + r16(KFDB_CTRL * 4);
    bool ok = hipSetDevice(device_id) == hipSuccess && hipStreamCreateWithFlags(&db->own_stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreateWithFlags(&db->ev_switch, hipEventDisableTiming) == hipSuccess &&
              hipMalloc(&db->weight, (size_t)n_words * sizeof(double)) == hipSuccess && hipMalloc(&db->slab, bytes) == hipSuccess &&
              hipMemcpy(db->weight, word_weight, (size_t)n_words * sizeof(double), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(db->slab, 0, bytes) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        free_device(db->weight, db->slab);
        destroy_event(db->ev_switch);
        if (db->own_stream) (void)hipStreamDestroy(db->own_stream);
        delete db;
        return JSORB_ERR_HIP;
    }
    char *p = (char *)db->slab;
    const auto take = [&p](auto *&dst, size_t b) { dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(p); p += b; };
    take(db->st.loop_query, b8); take(db->st.reloc_query, b8); take(db->key, b8);
    take(db->st.present, b4); take(db->st.off, b4); take(db->st.len, b4); take(db->st.seq, b4);
    take(db->st.loop_words, b4); take(db->st.reloc_words, b4); take(db->st.loop_score, b4); take(db->st.reloc_score, b4);
    take(db->tscore, b4); take(db->ent_acc, b4); take(db->first_pos, b4); take(db->list, b4); take(db->ent_flag, b4); take(db->ent_best, b4);
    take(db->cand, r16((M + 1) * 4));            // the synchronous forms' candidates, then their count
    take(db->ctrl, r16(KFDB_CTRL * 4));
    db->present.assign(M, 0); db->slot_off.assign(M, 0); db->slot_cap.assign(M, 0);
    db->stream = db->own_stream;
    *out = db;
    return JSORB_OK;
}

void jsorb_keyframe_database_destroy(jsorb_keyframe_database *db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    (void)hipStreamSynchronize(db->stream);
    free_device(db->weight, db->slab, db->st.pool_word, db->st.pool_value, db->sort);
    destroy_event(db->ev_switch);
    if (db->own_stream) (void)hipStreamDestroy(db->own_stream);
    delete db;
}

int jsorb_keyframe_database_set_stream(jsorb_keyframe_database *db, void *hip_stream)
{
    if (!db) return JSORB_ERR_INVALID;
    hipStream_t ns = hip_stream ? (hipStream_t)hip_stream : db->own_stream;
    if (ns != db->stream && db->used) {          // the new stream continues after what the old one still carries (the same state and scratch)
        HIPCHK(db, hipSetDevice(db->device));
        HIPCHK(db, hipEventRecord(db->ev_switch, db->stream));
        HIPCHK(db, hipStreamWaitEvent(ns, db->ev_switch, 0));
    }
    db->stream = ns;
    return JSORB_OK;
}
void *jsorb_keyframe_database_get_stream(const jsorb_keyframe_database *db) { return db ? (void *)db->stream : nullptr; }
const char *jsorb_keyframe_database_last_error(const jsorb_keyframe_database *db) { return db ? db->err.c_str() : "NULL database"; }
int jsorb_keyframe_database_size(const jsorb_keyframe_database *db)
{
    return db ? (int)std::count(db->present.begin(), db->present.end(), 1) : 0;
}

int jsorb_bow_vector_async(jsorb_keyframe_database *db, const int32_t *word_id, int n, int32_t *bow_word, double *bow_value, int32_t *bow_n_dev)
{
    if (!db) return JSORB_ERR_INVALID;
    if (n < 0) return kf_fail(db, BV, "n must not be negative");
    if (!bow_n_dev) return kf_fail(db, BV, "NULL bow_n");
    if (n > 0 && (!word_id || !bow_word || !bow_value)) return kf_fail(db, BV, "NULL word_id, bow_word or bow_value");
    HIPCHK(db, hipSetDevice(db->device));
    if (n > kfdb_sort_lds()) RCCHK(reserve_device(db, db->sort, (size_t)n * sizeof(uint32_t), &db->sort_cap, n));
    db->used = true;
    if (n == 0) {                                // an empty vector: nothing reads
        HIPCHK(db, hipMemsetAsync(bow_n_dev, 0, sizeof(int32_t), db->stream));
        return JSORB_OK;
    }
    launch_kfdb_bow_vector(word_id, n, db->weight, db->n_words, db->sort, bow_word, bow_value, bow_n_dev, db->stream);
    HIPCHK(db, hipGetLastError());
    return JSORB_OK;
}

int jsorb_keyframe_database_add_async(jsorb_keyframe_database *db, int slot, const int32_t *bow_word, const double *bow_value, int cap,
                                      const int32_t *bow_n_dev)
{
    if (!db) return JSORB_ERR_INVALID;
    if (slot < 0 || slot >= db->max_kf) return kf_fail(db, KD, "add: slot outside [0, max_keyframes)");
    if (db->present[slot]) return kf_fail(db, KD, "add: the slot holds a keyframe (erase it first)");
    RCCHK(vector_check(db, KD, bow_word, bow_value, cap, bow_n_dev));
    if (db->next_seq == 0xffffffffu) return kf_fail(db, KD, "add: 2^32 - 1 keyframes were added (clear the database)", JSORB_ERR_UNSUPPORTED);
    HIPCHK(db, hipSetDevice(db->device));
    // the keyframe's place in the pool: an erased keyframe's, or the top (the pool grows: a copy on the stream, a wait, the old one freed)
    int off = -1;
    for (size_t h = 0; h < db->holes.size() && off < 0; h++)
        if (db->holes[h].second >= cap) {
            off = db->holes[h].first;
            db->holes[h].first += cap; db->holes[h].second -= cap;
            if (db->holes[h].second == 0) db->holes.erase(db->holes.begin() + h);
        }
    if (off < 0) {
        if ((long long)db->pool_top + cap > INT_MAX) return kf_fail(db, KD, "add: the pool would exceed 2^31 - 1 entries", JSORB_ERR_UNSUPPORTED);
        if (db->pool_top + cap > db->pool_cap) {
            const int want = (int)std::min<long long>(INT_MAX, std::max<long long>({2LL * db->pool_cap, (long long)db->pool_top + cap, 1 << 16}));
            int32_t *nw = nullptr;
            double *nv = nullptr;
            HIPCHK(db, hipMalloc(&nw, (size_t)want * sizeof(int32_t)));
            if (hipMalloc(&nv, (size_t)want * sizeof(double)) != hipSuccess) { (void)hipFree(nw); db->err = "keyframe_database: add: hipMalloc failed"; return JSORB_ERR_HIP; }
            if (db->pool_top > 0) {
                HIPCHK(db, hipMemcpyAsync(nw, db->st.pool_word, (size_t)db->pool_top * sizeof(int32_t), hipMemcpyDeviceToDevice, db->stream));
                HIPCHK(db, hipMemcpyAsync(nv, db->st.pool_value, (size_t)db->pool_top * sizeof(double), hipMemcpyDeviceToDevice, db->stream));
            }
            HIPCHK(db, hipStreamSynchronize(db->stream));
            free_device(db->st.pool_word, db->st.pool_value);
            db->st.pool_word = nw; db->st.pool_value = nv; db->pool_cap = want;
        }
        off = db->pool_top;
        db->pool_top += cap;
    }
    db->present[slot] = 1; db->slot_off[slot] = off; db->slot_cap[slot] = cap;
    db->st.slots = std::max(db->st.slots, slot + 1);
    db->used = true;
    launch_kfdb_add(db->st, slot, db->next_seq++, off, KfdbVector{bow_word, bow_value, bow_n_dev, cap}, db->stream);
    HIPCHK(db, hipGetLastError());
    return JSORB_OK;
}

int jsorb_keyframe_database_erase(jsorb_keyframe_database *db, int slot)
{
    if (!db) return JSORB_ERR_INVALID;
    if (slot < 0 || slot >= db->max_kf) return kf_fail(db, KD, "erase: slot outside [0, max_keyframes)");
    if (!db->present[slot]) return JSORB_OK;
    HIPCHK(db, hipSetDevice(db->device));
    HIPCHK(db, hipMemsetAsync(db->st.present + slot, 0, sizeof(int32_t), db->stream));
    db->present[slot] = 0;
    if (db->slot_off[slot] + db->slot_cap[slot] == db->pool_top) db->pool_top = db->slot_off[slot];
    else if (db->slot_cap[slot] > 0) db->holes.emplace_back(db->slot_off[slot], db->slot_cap[slot]);
    return JSORB_OK;
}

int jsorb_keyframe_database_clear(jsorb_keyframe_database *db)
{
    if (!db) return JSORB_ERR_INVALID;
    HIPCHK(db, hipSetDevice(db->device));
    if (db->st.slots > 0) HIPCHK(db, hipMemsetAsync(db->st.present, 0, (size_t)db->st.slots * sizeof(int32_t), db->stream));
    std::fill(db->present.begin(), db->present.end(), 0);
    db->holes.clear();
    db->pool_top = 0; db->st.slots = 0; db->next_seq = 0;
    return JSORB_OK;
}

int jsorb_keyframe_database_score_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                        const int32_t *slots, int n_slots, float *score, double *score_f64, float *min_score_dev)
{
    if (!db) return JSORB_ERR_INVALID;
    RCCHK(vector_check(db, SC, q_word, q_value, q_cap, q_n_dev));
    if (n_slots < 0) return kf_fail(db, SC, "n_slots must not be negative");
    if (!min_score_dev) return kf_fail(db, SC, "NULL min_score");
    if (n_slots > 0 && (!slots || !score)) return kf_fail(db, SC, "NULL slots or score");
    HIPCHK(db, hipSetDevice(db->device));
    db->used = true;
    if (n_slots == 0) {                          // :128 `float minScore = 1`
        const float one = 1.0f;
        uint32_t bits;
        memcpy(&bits, &one, 4);
        HIPCHK(db, hipMemsetD32Async((hipDeviceptr_t)min_score_dev, (int)bits, 1, db->stream));
        return JSORB_OK;
    }
    KfdbScoreArgs a{};
    a.st = db->st;
    a.q = KfdbVector{q_word, q_value, q_n_dev, q_cap};
    a.slot_list = slots; a.n_slots = n_slots; a.score = score; a.score_f64 = score_f64; a.min_score = min_score_dev;
    launch_kfdb_score(a, db->stream);
    HIPCHK(db, hipGetLastError());
    return JSORB_OK;
}

int jsorb_detect_loop_candidates_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                       uint64_t query_id, const uint8_t *connected, const int32_t *neighbours, float min_score,
                                       const float *min_score_dev, int32_t *candidates, int32_t *n_candidates_dev)
{
    if (!db) return JSORB_ERR_INVALID;
    return query(db, DL, 0, q_word, q_value, q_cap, q_n_dev, query_id, connected, neighbours, min_score, min_score_dev, candidates, n_candidates_dev);
}

int jsorb_detect_relocalization_candidates_async(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap,
                                                 const int32_t *q_n_dev, uint64_t query_id, const int32_t *neighbours, int32_t *candidates,
                                                 int32_t *n_candidates_dev)
{
    if (!db) return JSORB_ERR_INVALID;
    return query(db, DR, 1, q_word, q_value, q_cap, q_n_dev, query_id, nullptr, neighbours, 0.0f, nullptr, candidates, n_candidates_dev);
}

int jsorb_detect_loop_candidates(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                 uint64_t query_id, const uint8_t *connected, const int32_t *neighbours, float min_score, const float *min_score_dev,
                                 int32_t *candidates_host, int *n_candidates_host)
{
    if (!db) return JSORB_ERR_INVALID;
    if (!candidates_host || !n_candidates_host) return kf_fail(db, DL, "NULL host output");
    RCCHK(query(db, DL, 0, q_word, q_value, q_cap, q_n_dev, query_id, connected, neighbours, min_score, min_score_dev, db->cand, db->cand + db->max_kf));
    return query_host(db, DL, candidates_host, n_candidates_host);
}

int jsorb_detect_relocalization_candidates(jsorb_keyframe_database *db, const int32_t *q_word, const double *q_value, int q_cap, const int32_t *q_n_dev,
                                           uint64_t query_id, const int32_t *neighbours, int32_t *candidates_host, int *n_candidates_host)
{
    if (!db) return JSORB_ERR_INVALID;
    if (!candidates_host || !n_candidates_host) return kf_fail(db, DR, "NULL host output");
    RCCHK(query(db, DR, 1, q_word, q_value, q_cap, q_n_dev, query_id, nullptr, neighbours, 0.0f, nullptr, db->cand, db->cand + db->max_kf));
    return query_host(db, DR, candidates_host, n_candidates_host);
}

int jsorb_detect_candidates_stats(jsorb_keyframe_database *db, int *n_sharing, int *max_common_words, int *min_common_words, int *n_scored, int *n_kept,
                                  float *best_acc_score, int *n_candidates)
{
    if (!db) return JSORB_ERR_INVALID;
    int32_t s[KFDB_CTRL] = {0};
    RCCHK(read_stats(db, db->queried, "detect_candidates_stats before a query", db->ctrl, s, KFDB_CTRL));
    if (n_sharing) *n_sharing = s[0];
    if (max_common_words) *max_common_words = s[1];
    if (n_scored) *n_scored = s[2];
    if (n_kept) *n_kept = s[3];
    if (n_candidates) *n_candidates = s[6];
    if (min_common_words) *min_common_words = s[7];
    if (best_acc_score) memcpy(best_acc_score, &s[8], sizeof(float));
    return JSORB_OK;
}

int jsorb_keyframe_database_copy_state(jsorb_keyframe_database *db, int32_t *present, uint64_t *loop_query, uint64_t *reloc_query, int32_t *loop_words,
                                       int32_t *reloc_words, float *loop_score, float *reloc_score)
{
    if (!db) return JSORB_ERR_INVALID;
    HIPCHK(db, hipSetDevice(db->device));
    HIPCHK(db, hipStreamSynchronize(db->stream));
    const size_t M = (size_t)db->max_kf;
    const struct { void *dst; const void *src; size_t elem; } c[] = {
        {present, db->st.present, 4}, {loop_query, db->st.loop_query, 8}, {reloc_query, db->st.reloc_query, 8}, {loop_words, db->st.loop_words, 4},
        {reloc_words, db->st.reloc_words, 4}, {loop_score, db->st.loop_score, 4}, {reloc_score, db->st.reloc_score, 4}};
    for (const auto &x : c)
        if (x.dst) HIPCHK(db, hipMemcpy(x.dst, x.src, M * x.elem, hipMemcpyDeviceToHost));
    return JSORB_OK;
}

int jsorb_kfdb_build_caps(int *query_lds, int *sort_lds)
{
    if (query_lds) *query_lds = kfdb_query_lds();
    if (sort_lds) *sort_lds = kfdb_sort_lds();
    return JSORB_OK;
}

} // extern "C"
