// tools/ref_bow/driver.cpp - one world of tests/bow_ref_cases.py through the reference's own TemplatedVocabulary::loadFromTextFile,
// saveToTextFile and both forms of transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259, :1338-1449), compiled unmodified with
// FORB.cpp, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp, DUtils/Random.cpp and DUtils/Timestamp.cpp against the stand-in
// opencv2/core/core.hpp of tools/ref_vocab.  AUTHORING TOOLING ONLY: built into oracle/_ref/ref_bow by tests/bow_ref_cases.py:build_driver where
// the reference tree is present.
//   ref_bow world.bin out.bin [vocabulary.txt saved.txt]
//   world: int32 mode (0: loadFromTextFile(vocabulary.txt); 1: m_nodes and m_words filled from the flat arrays below), n_nodes, k, L, scoring,
//          weighting, n_sets, n_levelsup, phantom, 0
//          mode 1: int32 child_start[n_nodes + 1], children[n_nodes - 1]; uint8 descriptor[n_nodes x 32]; int32 word_id[n_nodes]; double weight[n_nodes]
//          int32 levelsup[n_levelsup], set_start[n_sets + 1]; uint8 feature[set_start[n_sets] x 32]
//   out:   records (uint32 name length, name, uint8 type 'i' int32 / 'u' uint32 / 'q' uint64 / 'b' uint8, uint64 count, data):
//          mode 0: meta (k, L, scoring, weighting, n_nodes, n_words), parent, child_start, children, descriptors, weight_bits, word_id (as the
//                  node holds it: 0 in a node no leaf line numbered), is_leaf (isLeaf()), words (m_words as node ids), saved (saveToTextFile's bytes)
//          phantom (a file that ends in a newline, n_nodes is the number of its node lines): meta with the reference's count, and the first
//                  n_nodes nodes only - parent, descriptors, weight_bits, word_id, and child_start / children without ids >= n_nodes.  Nothing
//                  of the node past them is read.
//          transforms, in the order (levelsup, set, feature): t_word, t_weight_bits, t_nid of transform(feature, word_id, weight, &nid, levelsup)
//                  with nid preset to SENTINEL; per (levelsup, set): v_ran (no non-stopped feature of the set kept the sentinel: only then is the
//                  vector form called, whose `NodeId nid;` has no value of its own), and for those the BowVector in map order (bow_start,
//                  bow_word, bow_bits) and the FeatureVector in map order (fvn_start: nodes per call; fv_node; fv_fstart, fv_feat)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"

static const uint32_t SENTINEL = 0xFFFFFFFFu;

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;

template <class T> static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "ref_bow: short input\n"); exit(2); }
    return v;
}
template <class T> static void put(FILE *f, const char *name, char type, const std::vector<T> &v)
{
    const uint32_t len = (uint32_t)strlen(name);
    const uint64_t n = v.size();
    fwrite(&len, 4, 1, f); fwrite(name, 1, len, f); fwrite(&type, 1, 1, f); fwrite(&n, 8, 1, f);
    if (n && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "ref_bow: short output\n"); exit(2); }
}
static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }

class Vocabulary : public Base {
public:
    void fill(int n, int k, int L, int scoring, int weighting, const int32_t *child_start, const int32_t *children, const uint8_t *desc,
              const int32_t *word_id, const double *weight)
    {
        m_k = k; m_L = L;
        m_scoring = (DBoW2::ScoringType)scoring;
        m_weighting = (DBoW2::WeightingType)weighting;
        createScoringObject();
        m_nodes.clear(); m_words.clear();
        m_nodes.resize((size_t)n);
        int n_words = 0;
        for (int i = 0; i < n; i++) {
            m_nodes[i].id = (DBoW2::NodeId)i;
            m_nodes[i].weight = weight[i];
            for (int c = child_start[i]; c < child_start[i + 1]; c++) {
                m_nodes[i].children.push_back((DBoW2::NodeId)children[c]);
                m_nodes[children[c]].parent = (DBoW2::NodeId)i;
            }
            if (i) {
                m_nodes[i].descriptor.create(1, 32, CV_8U);
                memcpy(m_nodes[i].descriptor.ptr<unsigned char>(), desc + 32 * (size_t)i, 32);
            }
            if (word_id[i] >= 0) { m_nodes[i].word_id = (DBoW2::WordId)word_id[i]; if (word_id[i] + 1 > n_words) n_words = word_id[i] + 1; }
        }
        m_words.resize((size_t)n_words);
        for (int i = 0; i < n; i++)
            if (word_id[i] >= 0) m_words[word_id[i]] = &m_nodes[i];
    }

    void write_tree(FILE *f, int first) const          // first < 0: every node; else the first `first` nodes of a file that ended in a newline
    {
        const int total = (int)m_nodes.size(), n = first < 0 ? total : first;
        std::vector<int32_t> meta = {m_k, m_L, (int32_t)m_scoring, (int32_t)m_weighting, total, first < 0 ? (int32_t)m_words.size() : -1};
        std::vector<int32_t> parent, child_start, children, words;
        std::vector<uint8_t> desc((size_t)n * 32, 0), is_leaf;
        std::vector<uint64_t> weight;
        std::vector<uint32_t> word_id;
        for (int i = 0; i < n; i++) {
            const Node &v = m_nodes[i];
            parent.push_back(i ? (int32_t)v.parent : -1);
            child_start.push_back((int32_t)children.size());
            for (size_t c = 0; c < v.children.size(); c++)
                if ((int)v.children[c] < n) children.push_back((int32_t)v.children[c]);
            if (i && !v.descriptor.empty()) memcpy(&desc[(size_t)i * 32], v.descriptor.ptr<unsigned char>(), 32);
            weight.push_back(bits(v.weight));
            word_id.push_back(v.word_id);
            is_leaf.push_back(v.isLeaf() ? 1 : 0);
        }
        child_start.push_back((int32_t)children.size());
        put(f, "meta", 'i', meta); put(f, "parent", 'i', parent); put(f, "child_start", 'i', child_start); put(f, "children", 'i', children);
        put(f, "descriptors", 'b', desc); put(f, "weight_bits", 'q', weight); put(f, "word_id", 'u', word_id);
        if (first >= 0) return;
        for (size_t w = 0; w < m_words.size(); w++) words.push_back((int32_t)m_words[w]->id);
        put(f, "is_leaf", 'b', is_leaf); put(f, "words", 'i', words);
    }

    void write_transforms(FILE *f, const std::vector<int32_t> &levelsup, const std::vector<int32_t> &set_start, const std::vector<uint8_t> &rows) const
    {
        const int n_sets = (int)set_start.size() - 1;
        std::vector<std::vector<cv::Mat> > sets((size_t)n_sets);
        for (int s = 0; s < n_sets; s++)
            for (int i = set_start[s]; i < set_start[s + 1]; i++) {
                cv::Mat m;
                m.create(1, 32, CV_8U);
                memcpy(m.ptr<unsigned char>(), &rows[(size_t)i * 32], 32);
                sets[s].push_back(m);
            }
        std::vector<uint32_t> t_word, t_nid, bow_word, fv_node, fv_feat;
        std::vector<uint64_t> t_weight, bow_bits;
        std::vector<uint8_t> v_ran;
        std::vector<int32_t> bow_start(1, 0), fvn_start(1, 0), fv_fstart(1, 0);
        for (size_t j = 0; j < levelsup.size(); j++)
            for (int s = 0; s < n_sets; s++) {
                bool defined = true;
                for (size_t i = 0; i < sets[s].size(); i++) {
                    DBoW2::WordId id = 0;
                    DBoW2::WordValue w = 0;
                    DBoW2::NodeId nid = SENTINEL;
                    transform(sets[s][i], id, w, &nid, levelsup[j]);             // :1217-1259
                    t_word.push_back(id); t_weight.push_back(bits(w)); t_nid.push_back(nid);
                    if (w > 0 && nid == SENTINEL) defined = false;
                }
                v_ran.push_back(defined ? 1 : 0);
                if (defined) {
                    DBoW2::BowVector bv;
                    DBoW2::FeatureVector fv;
                    Base::transform(sets[s], bv, fv, levelsup[j]);               // :1127-1194, as Frame::ComputeBoW calls it (src/Frame.cpp:709-716)
                    for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it) { bow_word.push_back(it->first); bow_bits.push_back(bits(it->second)); }
                    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
                        fv_node.push_back(it->first);
                        for (size_t q = 0; q < it->second.size(); q++) fv_feat.push_back(it->second[q]);
                        fv_fstart.push_back((int32_t)fv_feat.size());
                    }
                }
                bow_start.push_back((int32_t)bow_word.size());
                fvn_start.push_back((int32_t)fv_node.size());
            }
        put(f, "t_word", 'u', t_word); put(f, "t_weight_bits", 'q', t_weight); put(f, "t_nid", 'u', t_nid); put(f, "v_ran", 'b', v_ran);
        put(f, "bow_start", 'i', bow_start); put(f, "bow_word", 'u', bow_word); put(f, "bow_bits", 'q', bow_bits);
        put(f, "fvn_start", 'i', fvn_start); put(f, "fv_node", 'u', fv_node); put(f, "fv_fstart", 'i', fv_fstart); put(f, "fv_feat", 'u', fv_feat);
    }
};

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: ref_bow world.bin out.bin [vocabulary.txt saved.txt]\n"); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    const std::vector<int32_t> head = take<int32_t>(in, 10);
    const int mode = head[0], n = head[1], n_sets = head[6], n_lu = head[7], phantom = head[8];
    Vocabulary voc;
    if (mode == 1) {
        const std::vector<int32_t> child_start = take<int32_t>(in, (size_t)n + 1), children = take<int32_t>(in, (size_t)n - 1);
        const std::vector<uint8_t> desc = take<uint8_t>(in, (size_t)n * 32);
        const std::vector<int32_t> word_id = take<int32_t>(in, (size_t)n);
        const std::vector<double> weight = take<double>(in, (size_t)n);
        voc.fill(n, head[2], head[3], head[4], head[5], child_start.data(), children.data(), desc.data(), word_id.data(), weight.data());
    } else {
        if (argc != 5) return 2;
        if (!voc.loadFromTextFile(argv[3])) { fprintf(stderr, "ref_bow: loadFromTextFile refused %s\n", argv[3]); return 3; }
    }
    const std::vector<int32_t> levelsup = take<int32_t>(in, (size_t)n_lu), set_start = take<int32_t>(in, (size_t)n_sets + 1);
    const std::vector<uint8_t> rows = take<uint8_t>(in, (size_t)set_start[n_sets] * 32);
    fclose(in);

    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    if (mode == 0) {
        voc.write_tree(out, phantom ? n : -1);
        if (!phantom) {
            voc.saveToTextFile(argv[4]);
            FILE *s = fopen(argv[4], "rb");
            if (!s) { perror(argv[4]); return 2; }
            std::vector<uint8_t> saved;
            for (int c; (c = fgetc(s)) != EOF;) saved.push_back((uint8_t)c);
            fclose(s);
            put(out, "saved", 'b', saved);
        }
    }
    if (n_sets > 0 && !phantom) voc.write_transforms(out, levelsup, set_start, rows);
    return fclose(out) ? 2 : 0;
}
