// train_vocabulary.cpp - ORBVocabulary::create on the descriptors THIS extractor produces, without leaving the device, through the shim
// (include/jsorb_compat.hpp): six synthetic frames are extracted, their descriptors copied device to device into one array (one document per
// frame), jsorb::TrainVocabulary builds the tree DBoW2's create(training_features, k = 8, L = 3, TF_IDF, L1_NORM) would build from them,
// jsorb::MakeVocabulary puts it on the device and the frames are transformed with it.
// The example checks itself: every training descriptor's word must have been seen in at least one document (Ni >= 1, so its weight is
// log(N / Ni), never the 0 of an unseen word), word ids must be the leaves in node order, and a second call with the same seed must give
// the same tree.  The tree is saved in the ORB-SLAM text format (ORBvoc.txt's).
// Usage: train_vocabulary out.txt
// Build: g++ -std=c++17 -I include examples/train_vocabulary.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jsorb_compat.hpp"

namespace {

const int H = 240, W = 320, FRAMES = 6, K = 8, DEPTH = 3;

unsigned rng_state = 2024;
unsigned rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// a frame of overlapping bright and dark rectangles on a gradient: corners for FAST
std::vector<unsigned char> frame()
{
    std::vector<unsigned char> im((size_t)H * W);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) im[(size_t)y * W + x] = (unsigned char)(64 + (x + 2 * y) % 64);
    for (int r = 0; r < 120; r++) {
        const int x0 = rnd() % (W - 8), y0 = rnd() % (H - 8), w = 6 + rnd() % 40, h = 6 + rnd() % 40;
        const unsigned char v = (unsigned char)(rnd() % 256);
        for (int y = y0; y < y0 + h && y < H; y++)
            for (int x = x0; x < x0 + w && x < W; x++) im[(size_t)y * W + x] = v;
    }
    return im;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s out.txt\n", argv[0]); return 2; }
    try {
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, 3, 9, 14, 7, 20, "", 15, 15, false, false, false, true);
        orb_cuda::SyncedMem<int> keys;
        orb_cuda::SyncedMem<unsigned char> desc;
        // the training set on the device: frame after frame behind each other, as getFeatures concatenates the documents (:620-637)
        const size_t cap = (size_t)FRAMES * 20000;
        void *all = nullptr;
        if (jsorb_mem_alloc_device(cap * 32, &all) != JSORB_OK) { fprintf(stderr, "no device memory\n"); return 1; }
        std::vector<int32_t> doc_start{0};
        for (int f = 0; f < FRAMES; f++) {
            const std::vector<unsigned char> im = frame();
            ex.extract(im.data(), W, keys, desc);
            const int n = jsorb_n_keypoints(ex.handle(), 0);
            if (n < 0 || (size_t)doc_start.back() + n > cap) { fprintf(stderr, "unexpected keypoint count\n"); return 3; }
            if (n && jsorb_mem_d2d((unsigned char *)all + (size_t)32 * doc_start.back(), jsorb_descriptors_device(ex.handle(), 0), (size_t)32 * n) != JSORB_OK) {
                fprintf(stderr, "device copy failed\n");
                return 1;
            }
            doc_start.push_back(doc_start.back() + n);
        }
        const int n = doc_start.back();
        if (n < 200) { fprintf(stderr, "too few descriptors to train on: %d\n", n); return 3; }
        const jsorb::TrainedVocabulary t = jsorb::TrainVocabulary((const unsigned char *)all, n, doc_start, K, DEPTH, 0, 0, 7);
        const jsorb::TrainedVocabulary again = jsorb::TrainVocabulary((const unsigned char *)all, n, doc_start, K, DEPTH, 0, 0, 7);
        if (t.parent != again.parent || t.descriptors != again.descriptors || t.weight != again.weight || t.Ni != again.Ni) {
            fprintf(stderr, "two calls with one seed gave two trees\n");
            return 3;
        }
        int words = 0;
        for (int i = 1; i < t.n_nodes; i++)
            if (t.child_start[i] == t.child_start[i + 1] && t.word_id[i] != words++) { fprintf(stderr, "word ids are not the leaves in node order\n"); return 3; }
        // the device vocabulary, and the training frames through it
        std::unique_ptr<jsorb::Vocabulary> voc = jsorb::MakeVocabulary(t);
        void *word_dev = nullptr;
        if (jsorb_mem_alloc_device((size_t)4 * n, &word_dev) != JSORB_OK) return 1;
        if (jsorb_bow_transform_descriptors(nullptr, voc->handle(), n, (const unsigned char *)all, (int32_t *)word_dev, nullptr) != JSORB_OK) return 1;
        std::vector<int32_t> word((size_t)n);
        if (jsorb_mem_device_sync() != JSORB_OK || jsorb_mem_d2h(word.data(), word_dev, (size_t)4 * n) != JSORB_OK) return 1;
        std::vector<int> node_of_word((size_t)t.n_words, 0);
        for (int i = 1; i < t.n_nodes; i++)
            if (t.word_id[i] >= 0) node_of_word[t.word_id[i]] = i;
        for (int i = 0; i < n; i++) {
            if (word[i] < 0 || word[i] >= t.n_words) { fprintf(stderr, "descriptor %d has no word\n", i); return 3; }
            const int node = node_of_word[word[i]];
            if (t.Ni[node] < 1 || t.Ni[node] > FRAMES) { fprintf(stderr, "word %d of descriptor %d has Ni = %d\n", word[i], i, t.Ni[node]); return 3; }
        }
        jsorb_mem_free_device(word_dev);
        jsorb_mem_free_device(all);
        if (!jsorb::SaveVocabularyText(t, argv[1])) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
        printf("descriptors=%d documents=%d nodes=%d words=%d kmeans_runs=%d draws=%lld passes=%d/%d/%d empty=%d unconverged=%d\n", n, FRAMES, t.n_nodes,
               t.n_words, t.n_kmeans_runs, t.n_draws, t.lloyd_passes[0], t.lloyd_passes[1], t.lloyd_passes[2], t.n_empty_clusters, t.n_unconverged);
        printf("every training descriptor's word has Ni >= 1; saved %s\n", argv[1]);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
