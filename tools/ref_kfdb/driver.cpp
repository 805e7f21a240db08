// tools/ref_kfdb/driver.cpp - plays a world of tests/kfdb_cases.py through the reference's own KeyFrameDatabase (src/KeyFrameDatabase.cpp), BowVector
// (BowVector.cpp) and L1Scoring (ScoringObject.cpp), all compiled unmodified, and writes what they computed.  The BowVector fold calls the
// reference's addWeight / normalize in the order of TemplatedVocabulary.h:1148-1193 (TF-IDF: `if(w > 0) v.addWeight(id, w)`, then
// `if(must) v.normalize(norm)` with `must` and `norm` from the scoring object's mustNormalize).  The minScore loop is LoopClosing.cpp:129-143 with
// the vocabulary's score.  A neighbour row names slots; -1 and slots that hold no keyframe are left out of the list a keyframe returns (the
// contract's one stated difference).  AUTHORING TOOLING ONLY: tools/ref_kfdb_goldens.py and tests/test_ref_kfdb.py build and run it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "KeyFrameDatabase.h"

using namespace Jetson_SLAM;

namespace {

enum { ADD, ERASE, LOOP, RELOC, SCORE, CLEAR };
const int NEIGHBOURS = 10;

template <class T> std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "ref_kfdb: short input\n"); exit(2); }
    return v;
}
template <class T> void put(FILE *f, const std::vector<T> &v)
{
    if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "ref_kfdb: short output\n"); exit(2); }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: ref_kfdb world.bin out.bin\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    const std::vector<int32_t> head = take<int32_t>(in, 5);
    const int W = head[0], M = head[1], n_ops = head[2], n_feat = head[3], n_list = head[4];
    const std::vector<double> weight = take<double>(in, W);
    const std::vector<int32_t> op_kind = take<int32_t>(in, n_ops), op_slot = take<int32_t>(in, n_ops);
    const std::vector<uint64_t> op_id = take<uint64_t>(in, n_ops);
    const std::vector<float> op_min_score = take<float>(in, n_ops);
    const std::vector<int32_t> feat_start = take<int32_t>(in, n_ops + 1), feat = take<int32_t>(in, n_feat);
    const std::vector<int32_t> list_start = take<int32_t>(in, n_ops + 1), lst = take<int32_t>(in, n_list);
    const std::vector<uint8_t> conn = take<uint8_t>(in, (size_t)n_ops * M);
    const std::vector<int32_t> neigh = take<int32_t>(in, (size_t)n_ops * M * NEIGHBOURS);
    fclose(in);

    ORBVocabulary voc((unsigned)W);
    KeyFrameDatabase db(voc);
    std::vector<KeyFrame *> kf(M, nullptr);      // the keyframe a slot holds (an erased one stays allocated: the reference only forgets it)

    std::vector<int32_t> bow_start(1, 0), bow_word, cand_start(1, 0), cand;
    std::vector<double> bow_value, score_f64;
    std::vector<float> score, min_score(n_ops, 0.f);
    std::vector<int32_t> present, loop_words, reloc_words;
    std::vector<uint64_t> loop_query, reloc_query;
    std::vector<float> loop_score, reloc_score;

    for (int i = 0; i < n_ops; i++) {
        const int kind = op_kind[i], slot = op_slot[i];
        DBoW2::BowVector v;
        if (kind == ADD || kind == LOOP || kind == RELOC || kind == SCORE) {
            DBoW2::LNorm norm;
            const bool must = voc.scoring.mustNormalize(norm);                   // TemplatedVocabulary.h:1140-1141
            for (int f = feat_start[i]; f < feat_start[i + 1]; f++) {            // :1148
                const int id = feat[f];
                const DBoW2::WordValue w = id >= 0 && id < W ? weight[id] : 0;
                if (w > 0) v.addWeight((DBoW2::WordId)id, w);                    // :1157-1159
            }
            if (must) v.normalize(norm);                                         // :1193
            for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
                bow_word.push_back((int32_t)it->first);
                bow_value.push_back(it->second);
            }
        }
        if (kind == ADD) {
            kf[slot] = new KeyFrame();
            kf[slot]->slot = slot;
            kf[slot]->mBowVec = v;
            db.add(kf[slot]);
        } else if (kind == ERASE) {
            if (kf[slot]) db.erase(kf[slot]);
            kf[slot] = nullptr;
        } else if (kind == CLEAR) {
            db.clear();
            for (int s = 0; s < M; s++) kf[s] = nullptr;
        } else if (kind == SCORE) {
            float minScore = 1;                                                  // LoopClosing.cpp:128
            for (int j = list_start[i]; j < list_start[i + 1]; j++) {
                KeyFrame *pKF = lst[j] >= 0 && lst[j] < M ? kf[lst[j]] : nullptr;
                if (!pKF) {                                                      // :132 isBad(): continue
                    score_f64.push_back(-1.0);
                    score.push_back(-1.f);
                    continue;
                }
                const double d = voc.score(v, pKF->mBowVec);
                float s = d;                                                     // :137 `float score = mpORBVocabulary->score(...)`
                score_f64.push_back(d);
                score.push_back(s);
                if (s < minScore) minScore = s;                                  // :139-140
            }
            min_score[i] = minScore;
        } else if (kind == LOOP || kind == RELOC) {
            for (int s = 0; s < M; s++) {
                if (!kf[s]) continue;
                kf[s]->neighbours.clear();
                for (int k = 0; k < NEIGHBOURS; k++) {
                    const int n = neigh[((size_t)i * M + s) * NEIGHBOURS + k];
                    if (n >= 0 && n < M && kf[n]) kf[s]->neighbours.push_back(kf[n]);
                }
            }
            std::vector<KeyFrame *> out;
            if (kind == LOOP) {
                KeyFrame q;
                q.mnId = op_id[i];
                q.mBowVec = v;
                for (int s = 0; s < M; s++)
                    if (kf[s] && conn[(size_t)i * M + s]) q.connected.insert(kf[s]);
                out = db.DetectLoopCandidates(&q, op_min_score[i]);
            } else {
                Frame q;
                q.mnId = op_id[i];
                q.mBowVec = v;
                out = db.DetectRelocalizationCandidates(&q);
            }
            for (size_t k = 0; k < out.size(); k++) cand.push_back(out[k]->slot);
        }
        bow_start.push_back((int32_t)bow_word.size());
        cand_start.push_back((int32_t)cand.size());
        for (int s = 0; s < M; s++) {
            const KeyFrame *k = kf[s];
            present.push_back(k ? 1 : 0);
            loop_query.push_back(k ? k->mnLoopQuery : 0);
            reloc_query.push_back(k ? k->mnRelocQuery : 0);
            loop_words.push_back(k ? k->mnLoopWords : 0);
            reloc_words.push_back(k ? k->mnRelocWords : 0);
            loop_score.push_back(k ? k->mLoopScore : 0.f);
            reloc_score.push_back(k ? k->mRelocScore : 0.f);
        }
    }

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    const std::vector<int32_t> counts = {(int32_t)bow_word.size(), (int32_t)cand.size()};
    put(out, counts); put(out, bow_start); put(out, bow_word); put(out, bow_value); put(out, cand_start); put(out, cand); put(out, score_f64);
    put(out, score); put(out, min_score); put(out, present); put(out, loop_query); put(out, reloc_query); put(out, loop_words);
    put(out, reloc_words); put(out, loop_score); put(out, reloc_score);
    fclose(out);
    return 0;
}
