// detect_loop.cpp - LoopClosing::DetectLoop up to its candidate list (LoopClosing.cpp:105-146) and Tracking::Relocalization up to SearchByBoW
// (Tracking.cpp:1954-1961) with the keyframe database ON THE DEVICE, through the shim (include/jsorb_compat.hpp), on a small map of the example's
// own: 40 keyframes that walk through eight places and come back to the first, word ids as jsorb_bow_transform_async would leave them (here:
// drawn from each place's words and uploaded).  Per keyframe one ComputeBowVector and one add; for the last keyframe LoopMinScore over its
// covisible keyframes and DetectLoopCandidates reading that minimum on the device, no wait in between; for a new frame of place 3
// DetectRelocalizationCandidates.  The binding code is the slot map (here: slot = keyframe id), the neighbour table (row s = the best covisible
// keyframes of s, -1 padded) and the connected mask.
// The example checks itself against a host loop: KeyFrameDatabase's text over std::map BowVectors and an inverted file of std::list, the same
// covisibility lists - candidates in the same order, every BowVector bit for bit.
// Usage: detect_loop
// Build: g++ -std=c++17 -I include examples/detect_loop.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <set>
#include <vector>

#include "jsorb_compat.hpp"

namespace {

const int N_WORDS = 4000, N_KF = 40, PLACES = 8, PLACE_WORDS = 150, FEATURES = 300, MAX_KF = 64;

typedef std::map<unsigned, double> Bow;

struct HostKF {
    int id = 0;
    Bow bow;
    unsigned long loop_query = 0, reloc_query = 0;
    int loop_words = 0, reloc_words = 0;
    float loop_score = 0, reloc_score = 0;
    std::vector<int> neighbours;                 // GetBestCovisibilityKeyFrames(10)
};

unsigned rng_state = 12345;
unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

Bow fold(const std::vector<int32_t> &ids, const std::vector<double> &weight)      // TemplatedVocabulary.h:1148-1193, BowVector.cpp:34-84
{
    Bow v;
    for (int id : ids)
        if (weight[id] > 0) {
            Bow::iterator it = v.lower_bound(id);
            if (it != v.end() && it->first == (unsigned)id) it->second += weight[id]; else v.insert(it, Bow::value_type(id, weight[id]));
        }
    double norm = 0.0;
    for (auto &e : v) norm += fabs(e.second);
    if (norm > 0.0) for (auto &e : v) e.second /= norm;
    return v;
}

double l1(const Bow &a, const Bow &b)            // ScoringObject.cpp:23-68
{
    Bow::const_iterator i = a.begin(), j = b.begin();
    double s = 0;
    while (i != a.end() && j != b.end()) {
        if (i->first == j->first) { s += fabs(i->second - j->second) - fabs(i->second) - fabs(j->second); ++i; ++j; }
        else if (i->first < j->first) i = a.lower_bound(j->first);
        else j = b.lower_bound(i->first);
    }
    return -s / 2.0;
}

// KeyFrameDatabase.cpp:80-201 (loop) and :203-313 (reloc) over the example's keyframes
std::vector<int> host_detect(bool reloc, std::vector<HostKF> &kfs, std::vector<std::list<HostKF *>> &inverted, const Bow &q, unsigned long id,
                             const std::set<int> &connected, float min_score)
{
    std::list<HostKF *> sharing;
    for (auto &e : q)
        for (HostKF *k : inverted[e.first]) {
            unsigned long &query = reloc ? k->reloc_query : k->loop_query;
            int &words = reloc ? k->reloc_words : k->loop_words;
            if (query != id) {
                words = 0;
                if (reloc || !connected.count(k->id)) { query = id; sharing.push_back(k); }
            }
            words++;
        }
    std::vector<int> out;
    if (sharing.empty()) return out;
    int maxw = 0;
    for (HostKF *k : sharing) maxw = std::max(maxw, reloc ? k->reloc_words : k->loop_words);
    const int minw = maxw * 0.8f;
    std::list<std::pair<float, HostKF *>> scored;
    for (HostKF *k : sharing)
        if ((reloc ? k->reloc_words : k->loop_words) > minw) {
            const float si = l1(q, k->bow);
            (reloc ? k->reloc_score : k->loop_score) = si;
            if (reloc || si >= min_score) scored.push_back(std::make_pair(si, k));
        }
    if (scored.empty()) return out;
    std::list<std::pair<float, HostKF *>> acc;
    float best_acc = reloc ? 0 : min_score;
    for (auto &e : scored) {
        float best = e.first, a = e.first;
        HostKF *bk = e.second;
        for (int n : e.second->neighbours) {
            HostKF *k2 = &kfs[n];
            if (reloc ? k2->reloc_query != id : !(k2->loop_query == id && k2->loop_words > minw)) continue;
            const float s2 = reloc ? k2->reloc_score : k2->loop_score;
            a += s2;
            if (s2 > best) { bk = k2; best = s2; }
        }
        acc.push_back(std::make_pair(a, bk));
        if (a > best_acc) best_acc = a;
    }
    const float retain = 0.75f * best_acc;
    std::set<HostKF *> seen;
    for (auto &e : acc)
        if (e.first > retain && !seen.count(e.second)) { out.push_back(e.second->id); seen.insert(e.second); }
    return out;
}

template <class T> T *upload(const std::vector<T> &v)
{
    void *p = nullptr;
    if (jsorb_mem_alloc_device(std::max<size_t>(v.size(), 1) * sizeof(T), &p) != JSORB_OK) { fprintf(stderr, "device allocation failed\n"); exit(1); }
    if (!v.empty() && jsorb_mem_h2d(p, v.data(), v.size() * sizeof(T)) != JSORB_OK) { fprintf(stderr, "upload failed\n"); exit(1); }
    return (T *)p;
}

jsorb::DeviceBowVector device_vector(int cap)
{
    jsorb::DeviceBowVector v;
    v.cap = cap;
    v.word = upload(std::vector<int32_t>(cap, 0));
    v.value = upload(std::vector<double>(cap, 0.0));
    v.n = upload(std::vector<int32_t>(1, 0));
    return v;
}

bool same_vector(const jsorb::DeviceBowVector &d, const Bow &h)
{
    int32_t n = -1;
    jsorb_mem_d2h(&n, d.n, sizeof(n));
    if (n != (int)h.size()) return false;
    std::vector<int32_t> w(n);
    std::vector<double> v(n);
    if (n) { jsorb_mem_d2h(w.data(), d.word, n * sizeof(int32_t)); jsorb_mem_d2h(v.data(), d.value, n * sizeof(double)); }
    int i = 0;
    for (auto &e : h) {
        if (w[i] != (int)e.first || memcmp(&v[i], &e.second, sizeof(double)) != 0) return false;
        i++;
    }
    return true;
}

}  // namespace

int main()
{
    // the vocabulary's leaf weights (a real system: ORBVocabulary's nodes) and the places' words
    std::vector<double> weight(N_WORDS);
    for (double &w : weight) w = rnd() % 100 == 0 ? 0.0 : 0.5 + (rnd() % 8500) / 1000.0;
    std::vector<std::vector<int>> place(PLACES, std::vector<int>(PLACE_WORDS));
    for (auto &p : place) for (int &w : p) w = rnd() % N_WORDS;
    auto frame_of = [&](int pl) {
        std::vector<int32_t> ids(FEATURES);
        for (int32_t &id : ids) id = place[pl][std::min(rnd() % PLACE_WORDS, rnd() % PLACE_WORDS)];
        return ids;
    };

    jsorb::KeyframeDatabase db(MAX_KF, N_WORDS, weight.data());
    std::vector<HostKF> kfs(N_KF);
    std::vector<std::list<HostKF *>> inverted(N_WORDS);
    std::vector<int32_t> neighbours((size_t)MAX_KF * 10, -1);
    bool ok = true;
    jsorb::DeviceBowVector last{};
    for (int k = 0; k < N_KF; k++) {
        const int pl = k < N_KF - 4 ? k / 5 % PLACES : 0;                 // the last four keyframes are back in place 0
        const std::vector<int32_t> ids = frame_of(pl);
        int32_t *ids_gpu = upload(ids);
        jsorb::DeviceBowVector v = device_vector(FEATURES);
        Jetson_SLAM::ComputeBowVector(db, ids_gpu, FEATURES, v);           // pKF->ComputeBoW()
        kfs[k].id = k;
        kfs[k].bow = fold(ids, weight);
        if (k < N_KF - 1) {                                               // (the current keyframe enters the database after DetectLoop, LoopClosing.cpp:149)
            db.add(k, v);                                                 // mpKeyFrameDB->add(pKF): slot = keyframe id
            for (auto &e : kfs[k].bow) inverted[e.first].push_back(&kfs[k]);
        }
        for (int j = 1; j <= 3; j++)                                      // covisibility: the three keyframes before and after
            for (int n : {k - j, k + j})
                if (n >= 0 && n < N_KF) kfs[k].neighbours.push_back(n);
        for (size_t j = 0; j < kfs[k].neighbours.size(); j++) neighbours[(size_t)k * 10 + j] = kfs[k].neighbours[j];
        jsorb_mem_stream_sync(db.stream());
        ok = ok && same_vector(v, kfs[k].bow);
        jsorb_mem_free_device(ids_gpu);
        if (k == N_KF - 1) last = v;
        else { jsorb_mem_free_device(v.word); jsorb_mem_free_device(v.value); jsorb_mem_free_device(v.n); }      // the database keeps its own copy
    }
    if (!ok) { printf("a device BowVector differs from the host fold\n"); return 1; }
    int32_t *neighbours_gpu = upload(neighbours);

    // ---- DetectLoop for the last keyframe: minScore over its covisible keyframes, then the candidates ----
    HostKF &cur = kfs[N_KF - 1];
    std::set<int> connected(cur.neighbours.begin(), cur.neighbours.end());
    std::vector<unsigned char> mask(MAX_KF, 0);
    std::vector<int32_t> cov(cur.neighbours.begin(), cur.neighbours.end());
    for (int n : cov) mask[n] = 1;
    unsigned char *mask_gpu = upload(mask);
    int32_t *cov_gpu = upload(cov);
    float *score_gpu = upload(std::vector<float>(cov.size(), 0.f)), *min_gpu = upload(std::vector<float>(1, 0.f));
    Jetson_SLAM::LoopMinScore(db, last, cov_gpu, (int)cov.size(), score_gpu, min_gpu);                       // LoopClosing.cpp:129-143
    const std::vector<int> loop = Jetson_SLAM::DetectLoopCandidates(db, last, cur.id, mask_gpu, neighbours_gpu, 0.f, min_gpu);   // :146
    float min_score = 1;
    for (int n : cov) { const float s = l1(cur.bow, kfs[n].bow); if (s < min_score) min_score = s; }
    float min_dev = -1;
    jsorb_mem_d2h(&min_dev, min_gpu, sizeof(float));
    const std::vector<int> loop_host = host_detect(false, kfs, inverted, cur.bow, cur.id, connected, min_score);
    ok = memcmp(&min_dev, &min_score, sizeof(float)) == 0 && loop == loop_host;
    printf("loop: minScore=%.6f candidates=%zu first=%d\n", min_dev, loop.size(), loop.empty() ? -1 : loop[0]);
    if (!ok) { printf("the loop candidates differ from the host loop\n"); return 1; }
    db.add(cur.id, last);                                                                                    // :149 mpKeyFrameDB->add(mpCurrentKF)
    for (auto &e : cur.bow) inverted[e.first].push_back(&cur);

    // ---- Relocalization: a new frame of place 3 ----
    const std::vector<int32_t> ids = frame_of(3);
    int32_t *ids_gpu = upload(ids);
    jsorb::DeviceBowVector fv = device_vector(FEATURES);
    Jetson_SLAM::ComputeBowVector(db, ids_gpu, FEATURES, fv);                                               // mCurrentFrame.ComputeBoW()
    const std::vector<int> reloc = Jetson_SLAM::DetectRelocalizationCandidates(db, fv, 1000, neighbours_gpu);   // Tracking.cpp:1961
    const std::vector<int> reloc_host = host_detect(true, kfs, inverted, fold(ids, weight), 1000, std::set<int>(), 0.f);
    printf("relocalization: candidates=%zu first=%d\n", reloc.size(), reloc.empty() ? -1 : reloc[0]);
    if (reloc != reloc_host) { printf("the relocalisation candidates differ from the host loop\n"); return 1; }
    bool loop_found = false, reloc_found = false;
    for (int s : loop) loop_found = loop_found || s < 5;                         // a keyframe of place 0, where the walk began
    for (int s : reloc) reloc_found = reloc_found || s / 5 == 3;                 // a keyframe of place 3
    if (!loop_found || !reloc_found) { printf("no candidate in the revisited place\n"); return 1; }
    printf("self-check ok\n");
    return 0;
}
