// tools/ref_vocab/driver.cpp - one training world through the reference's own TemplatedVocabulary::create
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996, compiled unmodified with FORB.cpp, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp,
// DUtils/Random.cpp and DUtils/Timestamp.cpp against the stand-in opencv2/core/core.hpp next to this file).  AUTHORING TOOLING ONLY: built into
// oracle/_ref/ref_vocab by tests/vocab_train_cases.py:build_driver where the reference tree is present.
// The one thing replaced is the SOURCE of the random values (include/jsorb.h): rand() is defined here as the contract's function of (seed, the
// run's first input index, the run's size, j), and the virtual initiateClusters is overridden to set that key before it calls the reference's
// own initiateClustersKMpp.  DUtils::Random::SeedRandOnce(0) runs first, so the clock seed never does.
//   ref_vocab world.bin out.bin
//   world: int32 n, n_docs, k, L, weighting, scoring; uint64 seed; int32 doc_start[n_docs + 1]; uint8 descriptors[n x 32]
//   out:   int32 n_nodes, runs; int64 draws; int32 parent[n_nodes]; uint8 descriptor[n_nodes x 32]; double weight[n_nodes];
//          int32 word_id[n_nodes] (-1: inner); int32 child_start[n_nodes + 1]; int32 children[n_nodes - 1]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "DUtils/Random.h"

static uint64_t g_seed, g_first, g_size, g_j, g_draws;
static int g_runs;

static uint64_t mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

extern "C" int rand(void)
{
    g_draws++;
    return (int)(mix(mix(g_seed ^ (g_first << 32 | g_size)) + g_j++) >> 33);
}

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;

class Vocabulary : public Base {
public:
    const std::vector<std::vector<cv::Mat> > *features;
    const int32_t *doc_start;
    virtual void initiateClusters(const std::vector<const cv::Mat *> &descriptors, std::vector<cv::Mat> &clusters) const
    {
        const cv::Mat *p = descriptors[0];
        for (size_t d = 0; d < features->size(); d++) {
            const std::vector<cv::Mat> &doc = (*features)[d];
            if (!doc.empty() && p >= &doc[0] && p <= &doc[doc.size() - 1]) g_first = (uint64_t)doc_start[d] + (uint64_t)(p - &doc[0]);
        }
        g_size = descriptors.size();
        g_j = 0;
        g_runs++;
        initiateClustersKMpp(descriptors, clusters);
    }
    void write(FILE *f) const
    {
        const int32_t n = (int32_t)m_nodes.size();
        const int64_t draws = (int64_t)g_draws;
        fwrite(&n, 4, 1, f); fwrite(&g_runs, 4, 1, f); fwrite(&draws, 8, 1, f);
        for (int i = 0; i < n; i++) { const int32_t p = i ? (int32_t)m_nodes[i].parent : -1; fwrite(&p, 4, 1, f); }
        for (int i = 0; i < n; i++) {
            unsigned char row[32] = {0};
            if (i && !m_nodes[i].descriptor.empty()) memcpy(row, m_nodes[i].descriptor.ptr<unsigned char>(), 32);
            fwrite(row, 1, 32, f);
        }
        for (int i = 0; i < n; i++) { const double w = m_nodes[i].weight; fwrite(&w, 8, 1, f); }
        for (int i = 0; i < n; i++) { const int32_t w = i && m_nodes[i].isLeaf() ? (int32_t)m_nodes[i].word_id : -1; fwrite(&w, 4, 1, f); }
        int32_t at = 0;
        for (int i = 0; i < n; i++) { fwrite(&at, 4, 1, f); at += (int32_t)m_nodes[i].children.size(); }
        fwrite(&at, 4, 1, f);
        for (int i = 0; i < n; i++)
            for (size_t c = 0; c < m_nodes[i].children.size(); c++) { const int32_t id = (int32_t)m_nodes[i].children[c]; fwrite(&id, 4, 1, f); }
    }
};

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    if (fread(head, 4, 6, f) != 6 || fread(&g_seed, 8, 1, f) != 1) return 2;
    const int n = head[0], n_docs = head[1];
    std::vector<int32_t> doc_start((size_t)n_docs + 1);
    std::vector<unsigned char> rows((size_t)n * 32);
    if (fread(doc_start.data(), 4, doc_start.size(), f) != doc_start.size() || (n && fread(rows.data(), 32, (size_t)n, f) != (size_t)n)) return 2;
    fclose(f);
    std::vector<std::vector<cv::Mat> > features((size_t)n_docs);
    for (int d = 0; d < n_docs; d++)
        for (int i = doc_start[d]; i < doc_start[d + 1]; i++) {
            cv::Mat m;
            m.create(1, 32, CV_8U);
            memcpy(m.ptr<unsigned char>(), &rows[(size_t)i * 32], 32);
            features[d].push_back(m);
        }
    DUtils::Random::SeedRandOnce(0);
    Vocabulary voc;
    voc.features = &features;
    voc.doc_start = doc_start.data();
    voc.create(features, head[2], head[3], (DBoW2::WeightingType)head[4], (DBoW2::ScoringType)head[5]);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    voc.write(f);
    return fclose(f) ? 2 : 0;
}
