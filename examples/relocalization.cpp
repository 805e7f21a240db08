// relocalization.cpp - the matching steps of Tracking::Relocalization for one candidate keyframe (Tracking.cpp:1975-2092) through the C++ shim: the
// first image plays the candidate keyframe (every keypoint carries a good map point, read from points.bin), the second the current frame.
//   matcher.SearchByBoW(pKF, mCurrentFrame, vvpMapPointMatches[i])                      Jetson_SLAM::SearchByBoW            (:1995)
//   the inliers into mCurrentFrame.mvpMapPoints and sFound                              host, as in the reference           (:2038-2051)
//   matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, 10, 100)      Jetson_SLAM::SearchByProjection     (:2065)
//   sFound = every map point of the frame                                               host                                (:2075-2078)
//   matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i], sFound, 3, 64)        Jetson_SLAM::SearchByProjection     (:2079)
// Every matcher call reads the descriptors the extract left on the device; one copy back each.  What stays on the host is what the reference keeps
// there as well: the PnP solver and PoseOptimization (here: the pose comes from points.bin and every second BoW match counts as an inlier) and the
// count tests between the calls (here: both projection calls always run).
// Usage: relocalization H W L tile th_fast keyframe.raw current.raw vocabulary.bin points.bin out.bin
//   vocabulary.bin: as for track_reference_keyframe
//   points.bin: int32 n_kf (the keyframe's keypoints); float32 Px[n_kf] Py Pz max_distance max_dist_inv min_dist_inv; float32 Rcw[9] tcw[3] Ow[3];
//               float32 fx fy cx cy log_scale_factor
//   out.bin: int32 n_bow, n_inliers, nadditional (10, 100), nadditional (3, 64), N, mvpMapPoints[N] as keyframe slots (-1: NULL)
// Build: g++ -std=c++17 -I include examples/relocalization.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jsorb_compat.hpp"

using orb_cuda::SyncedMem;

template <class T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

struct KeyFramePoints {                       // per keyframe slot: GetWorldPos, mfMaxDistance, its invariance bounds, mvKeysUn[].angle, GetDescriptor
    std::vector<float> P[6], angle;
    std::vector<unsigned char> desc;
};

// one matcher2.SearchByProjection call: the slots whose map point is not in sFound, compacted in ascending order; the frame's map points as blocked_in
static int search(Jetson_SLAM::ORBExtractor &ex, jsorb_kf_projection_params prm, float th, int orb_dist, const KeyFramePoints &kf,
                  const std::vector<char> &found, std::vector<int> &mvpMapPoints)
{
    const int n_kf = (int)kf.angle.size(), N = (int)mvpMapPoints.size();
    std::vector<int> slot;
    for (int j = 0; j < n_kf; j++)
        if (!found[j]) slot.push_back(j);
    const int n = (int)slot.size();
    SyncedMem<float> a[6], angle;
    SyncedMem<unsigned char> desc, blocked;
    for (auto &m : a) m.resize(n > 0 ? n : 1);
    angle.resize(n > 0 ? n : 1); desc.resize(n > 0 ? 32 * n : 32); blocked.resize(N > 0 ? N : 1);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 6; k++) a[k].cpu_data()[i] = kf.P[k][slot[i]];
        angle.cpu_data()[i] = kf.angle[slot[i]];
        for (int b = 0; b < 32; b++) desc.cpu_data()[32 * i + b] = kf.desc[32 * (size_t)slot[i] + b];
    }
    for (int k = 0; k < N; k++) blocked.cpu_data()[k] = mvpMapPoints[k] >= 0;
    for (auto &m : a) m.to_gpu();
    angle.to_gpu(); desc.to_gpu(); blocked.to_gpu();
    prm.th = th; prm.orb_dist = orb_dist;
    std::vector<int> kp_match;
    const int nadditional = Jetson_SLAM::SearchByProjection(ex, prm, n, a[0], a[1], a[2], a[3], a[4], a[5], angle, desc, blocked.gpu_data(), kp_match);
    for (int k = 0; k < N; k++)
        if (kp_match[k] >= 0) mvpMapPoints[k] = slot[kp_match[k]];
    return nadditional;
}

int main(int argc, char **argv)
{
    if (argc != 11) { fprintf(stderr, "usage: %s H W L tile th_fast keyframe.raw current.raw vocabulary.bin points.bin out.bin\n", argv[0]); return 2; }
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
        // the candidate keyframe: FeatureVector nodes, angles and descriptors for SearchByBoW; its map points from points.bin
        ex.extract(first.data(), W, keys, desc);
        const int n_kf = jsorb_n_keypoints(ex.handle(), 0);
        std::vector<int> kf_node;
        Jetson_SLAM::ComputeBoW(ex, voc, nullptr, &kf_node);
        KeyFramePoints kf;
        std::vector<int> n_file(1);
        std::vector<float> pose(15), cam(5);
        f = fopen(argv[9], "rb");
        if (!f || !rd(f, n_file) || n_file[0] != n_kf) { fprintf(stderr, "%s does not describe the keyframe's %d keypoints\n", argv[9], n_kf); return 2; }
        for (auto &v : kf.P) {
            v.resize(n_kf);
            if (!rd(f, v)) { fprintf(stderr, "short points file\n"); return 2; }
        }
        if (!rd(f, pose) || !rd(f, cam)) { fprintf(stderr, "short points file\n"); return 2; }
        fclose(f);
        const float *angles = reinterpret_cast<const float *>(keys.cpu_data() + 3 * (size_t)n_kf);      // keypoint SoA row 3: the angle's float bits
        kf.angle.assign(angles, angles + n_kf);
        kf.desc.assign(desc.cpu_data(), desc.cpu_data() + 32 * (size_t)n_kf);      // the map point's descriptor: its observation in the keyframe
        SyncedMem<int> node;
        SyncedMem<unsigned char> valid, kf_desc;
        SyncedMem<float> angle;
        node.resize(n_kf); valid.resize(n_kf); angle.resize(n_kf); kf_desc.resize(32 * n_kf);
        for (int i = 0; i < n_kf; i++) {
            node.cpu_data()[i] = kf_node[i];
            valid.cpu_data()[i] = 1;                                     // pMP && !pMP->isBad()
            angle.cpu_data()[i] = kf.angle[i];
        }
        for (int i = 0; i < 32 * n_kf; i++) kf_desc.cpu_data()[i] = kf.desc[i];
        node.to_gpu(); valid.to_gpu(); angle.to_gpu(); kf_desc.to_gpu();
        // the current frame
        ex.extract(second.data(), W, keys, desc);
        Jetson_SLAM::ComputeBoW(ex, voc);                               // mCurrentFrame.ComputeBoW(), Tracking.cpp:1957
        jsorb_bow_params bow{};
        bow.nn_ratio = 0.75f; bow.th_low = 50; bow.check_orientation = 1;      // ORBmatcher matcher(0.75, true), Tracking.cpp:1975
        std::vector<int> match_kf;
        const int n_bow = Jetson_SLAM::SearchByBoW(ex, bow, n_kf, node, valid, angle, kf_desc, match_kf);
        const int N = (int)match_kf.size();
        // :2038-2051: the inliers become the frame's map points and sFound (stand-in for the PnP solver: every second match, in keypoint order)
        std::vector<int> mvpMapPoints(N, -1);
        std::vector<char> found(n_kf, 0);
        int n_inliers = 0, seen = 0;
        for (int k = 0; k < N; k++)
            if (match_kf[k] >= 0 && seen++ % 2 == 0) {
                mvpMapPoints[k] = match_kf[k];
                found[match_kf[k]] = 1;
                n_inliers++;
            }
        jsorb_kf_projection_params prm{};
        prm.check_orientation = 1;                                      // ORBmatcher matcher2(0.9, true), Tracking.cpp:1976
        prm.fx = cam[0]; prm.fy = cam[1]; prm.cx = cam[2]; prm.cy = cam[3]; prm.log_scale_factor = cam[4];
        prm.min_x = 0.0f; prm.max_x = (float)W; prm.min_y = 0.0f; prm.max_y = (float)H;      // no distortion: the image itself (Frame::ComputeImageBounds)
        prm.cols = 64; prm.rows = 48;
        prm.inv_w = (float)prm.cols / (prm.max_x - prm.min_x);
        prm.inv_h = (float)prm.rows / (prm.max_y - prm.min_y);
        for (int i = 0; i < 9; i++) prm.Rcw[i] = pose[i];
        for (int i = 0; i < 3; i++) { prm.tcw[i] = pose[9 + i]; prm.Ow[i] = pose[12 + i]; }
        const int first_pass = search(ex, prm, 10.0f, 100, kf, found, mvpMapPoints);        // :2065
        std::fill(found.begin(), found.end(), 0);                                          // :2075-2078
        for (int k = 0; k < N; k++)
            if (mvpMapPoints[k] >= 0) found[mvpMapPoints[k]] = 1;
        const int second_pass = search(ex, prm, 3.0f, 64, kf, found, mvpMapPoints);         // :2079
        FILE *out = fopen(argv[10], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[10]); return 2; }
        const int headw[5] = {n_bow, n_inliers, first_pass, second_pass, N};
        fwrite(headw, 4, 5, out);
        fwrite(mvpMapPoints.data(), 4, mvpMapPoints.size(), out);
        fclose(out);
        printf("ok n_kf=%d N=%d bow=%d inliers=%d first=%d second=%d\n", n_kf, N, n_bow, n_inliers, first_pass, second_pass);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
