// track_reference_keyframe.cpp - the matching step of Tracking::TrackReferenceKeyFrame (Tracking.cpp:919-932) through the C++ shim: the first
// image plays the reference keyframe (every keypoint carries a good map point), the second the current frame.  mCurrentFrame.ComputeBoW() is
// Jetson_SLAM::ComputeBoW - the descent of the vocabulary tree on the device, the node ids stay there - and matcher.SearchByBoW(mpReferenceKF,
// mCurrentFrame, vpMapPointMatches) is ONE call, Jetson_SLAM::SearchByBoW, with one copy back of the matches.  What stays on the host is DBoW2
// (loading the vocabulary, BowVector, KeyFrameDatabase) and the pose optimisation behind the count.
// Usage: track_reference_keyframe H W L tile th_fast keyframe.raw current.raw vocabulary.bin out.bin
//   keyframe.raw / current.raw: H*W bytes each
//   vocabulary.bin: int32 n_nodes, depth_L, levels_up; int32 child_start[n_nodes + 1], children[n_nodes - 1]; uint8 descriptors[n_nodes * 32];
//                   int32 word_id[n_nodes]; double weight[n_nodes]  (m_nodes flattened)
//   out.bin: int32 nmatches, N, match_kf[N], n_kf, kf_node[n_kf]
// Build: g++ -std=c++17 -I include examples/track_reference_keyframe.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jsorb_compat.hpp"

using orb_cuda::SyncedMem;

template <class T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s H W L tile th_fast keyframe.raw current.raw vocabulary.bin out.bin\n", argv[0]); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th_fast = atoi(argv[5]);
    std::vector<unsigned char> first((size_t)H * W), second((size_t)H * W);
    FILE *f = fopen(argv[6], "rb");
    if (!f || !rd(f, first)) { fprintf(stderr, "cannot read %s\n", argv[6]); return 2; }
    fclose(f);
    f = fopen(argv[7], "rb");
    if (!f || !rd(f, second)) { fprintf(stderr, "cannot read %s\n", argv[7]); return 2; }
    fclose(f);
    f = fopen(argv[8], "rb");
    std::vector<int> head(3);
    if (!f || !rd(f, head) || head[0] < 2) { fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
    const size_t n_nodes = (size_t)head[0];
    std::vector<int> child_start(n_nodes + 1), children(n_nodes - 1), word_id(n_nodes);
    std::vector<unsigned char> node_desc(32 * n_nodes);
    std::vector<double> weight(n_nodes);
    if (!rd(f, child_start) || !rd(f, children) || !rd(f, node_desc) || !rd(f, word_id) || !rd(f, weight)) { fprintf(stderr, "short vocabulary file\n"); return 2; }
    fclose(f);
    try {
        jsorb::Vocabulary voc(head[0], head[1], head[2], child_start.data(), children.data(), node_desc.data(), word_id.data(), weight.data());
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        SyncedMem<int> keys;
        SyncedMem<unsigned char> desc;
        // the reference keyframe: its FeatureVector node per keypoint (KeyFrame::ComputeBoW), angles and descriptors, uploaded once
        ex.extract(first.data(), W, keys, desc);
        const int n_kf = jsorb_n_keypoints(ex.handle(), 0);
        std::vector<int> kf_node;
        Jetson_SLAM::ComputeBoW(ex, voc, nullptr, &kf_node);
        SyncedMem<int> node;
        SyncedMem<unsigned char> valid, kf_desc;
        SyncedMem<float> angle;
        node.resize(n_kf); valid.resize(n_kf); angle.resize(n_kf); kf_desc.resize(32 * n_kf);
        const float *angles = reinterpret_cast<const float *>(keys.cpu_data() + 3 * (size_t)n_kf);      // keypoint SoA row 3: the angle's float bits
        for (int i = 0; i < n_kf; i++) {
            node.cpu_data()[i] = kf_node[i];
            valid.cpu_data()[i] = 1;                                     // pMP && !pMP->isBad()
            angle.cpu_data()[i] = angles[i];
        }
        for (int i = 0; i < 32 * n_kf; i++) kf_desc.cpu_data()[i] = desc.cpu_data()[i];
        node.to_gpu(); valid.to_gpu(); angle.to_gpu(); kf_desc.to_gpu();
        // the current frame
        ex.extract(second.data(), W, keys, desc);
        Jetson_SLAM::ComputeBoW(ex, voc);                               // mCurrentFrame.ComputeBoW(), Tracking.cpp:922
        jsorb_bow_params prm{};
        prm.nn_ratio = 0.7f; prm.th_low = 50; prm.check_orientation = 1;       // ORBmatcher matcher(0.7, true), Tracking.cpp:925
        std::vector<int> match_kf;
        const int nmatches = Jetson_SLAM::SearchByBoW(ex, prm, n_kf, node, valid, angle, kf_desc, match_kf);
        const int N = (int)match_kf.size();
        FILE *out = fopen(argv[9], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
        fwrite(&nmatches, 4, 1, out);
        fwrite(&N, 4, 1, out);
        fwrite(match_kf.data(), 4, match_kf.size(), out);
        fwrite(&n_kf, 4, 1, out);
        fwrite(kf_node.data(), 4, kf_node.size(), out);
        fclose(out);
        printf("ok n_kf=%d N=%d nmatches=%d\n", n_kf, N, nmatches);
        if (nmatches < 15) printf("fewer than 15 matches: TrackReferenceKeyFrame fails (Tracking.cpp:931)\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
