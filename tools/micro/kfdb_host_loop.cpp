// tools/micro/kfdb_host_loop.cpp - the host loop tools/kfdb_bench.py sets the device queries beside: KeyFrameDatabase's method on the CPU - an
// inverted file of std::list per word, BowVectors as std::map<unsigned, double>, the walk that counts common words, maxCommonWords, the L1 score of
// the keyframes above minCommonWords by a merge walk with lower_bound, the 0.75 retain - for a relocalisation query without covisibility
// neighbours, and the BowVector fold of the query's word ids.  Input: n_kf, n_words, the keyframes' vectors as a CSR, the query's word ids and the
// leaf weights of the words that occur.  Prints the medians over `reps` passes and a checksum of the candidates.
// Build: g++ -O2 -std=c++17 tools/micro/kfdb_host_loop.cpp
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <vector>

typedef std::map<unsigned, double> Bow;
struct KF {
    Bow v;
    unsigned long query = 0;
    int words = 0;
    float score = 0;
    int slot = 0;
};

static double l1(const Bow &a, const Bow &b)
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

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) exit(2);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int reps = atoi(argv[2]);
    const std::vector<int32_t> head = take<int32_t>(f, 4);
    const int n_kf = head[0], n_words = head[1], total = head[2], nq = head[3];
    const std::vector<int32_t> start = take<int32_t>(f, n_kf + 1), word = take<int32_t>(f, total);
    const std::vector<double> value = take<double>(f, total);
    const std::vector<int32_t> q_ids = take<int32_t>(f, nq);
    const std::vector<double> q_weight = take<double>(f, nq);
    fclose(f);
    std::vector<KF> kfs(n_kf);
    std::vector<std::list<KF *>> inverted(n_words);
    for (int k = 0; k < n_kf; k++) {
        kfs[k].slot = k;
        for (int i = start[k]; i < start[k + 1]; i++) { kfs[k].v[word[i]] = value[i]; inverted[word[i]].push_back(&kfs[k]); }
    }
    std::vector<double> t_fold, t_query;
    long checksum = 0;
    for (int r = 0; r < reps; r++) {
        auto t0 = std::chrono::steady_clock::now();
        Bow q;
        for (int i = 0; i < nq; i++)
            if (q_weight[i] > 0) {
                Bow::iterator it = q.lower_bound(q_ids[i]);
                if (it != q.end() && it->first == (unsigned)q_ids[i]) it->second += q_weight[i]; else q.insert(it, Bow::value_type(q_ids[i], q_weight[i]));
            }
        double norm = 0;
        for (auto &e : q) norm += fabs(e.second);
        if (norm > 0) for (auto &e : q) e.second /= norm;
        auto t1 = std::chrono::steady_clock::now();
        const unsigned long id = r + 1;
        std::list<KF *> sharing;
        for (auto &e : q)
            for (KF *k : inverted[e.first]) {
                if (k->query != id) { k->words = 0; k->query = id; sharing.push_back(k); }
                k->words++;
            }
        int maxw = 0;
        for (KF *k : sharing) maxw = std::max(maxw, k->words);
        const int minw = maxw * 0.8f;
        std::list<std::pair<float, KF *>> scored;
        float best = 0;
        for (KF *k : sharing)
            if (k->words > minw) {
                k->score = l1(q, k->v);
                scored.push_back(std::make_pair(k->score, k));
                if (k->score > best) best = k->score;
            }
        const float retain = 0.75f * best;
        checksum = 0;
        for (auto &e : scored)
            if (e.first > retain) checksum = (checksum * 31 + e.second->slot + 1) % 1000000007L;
        auto t2 = std::chrono::steady_clock::now();
        t_fold.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        t_query.push_back(std::chrono::duration<double, std::micro>(t2 - t1).count());
    }
    std::sort(t_fold.begin(), t_fold.end());
    std::sort(t_query.begin(), t_query.end());
    printf("host_fold_us=%.2f host_query_us=%.2f checksum=%ld\n", t_fold[reps / 2], t_query[reps / 2], checksum);
    return 0;
}
