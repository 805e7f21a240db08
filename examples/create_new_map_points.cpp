// create_new_map_points.cpp - the matching step of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-275) through the C++ shim: the first
// image plays the new keyframe, the other three its covisible neighbours.  The reference calls matcher.SearchForTriangulation(mpCurrentKeyFrame,
// pKF2, F12, vMatchedIndices, false) once per neighbour inside the loop; here it is ONE call before the loop, Jetson_SLAM::SearchForTriangulation
// on a jsorb::KeyframeMatcher (a stream and scratch of its own: LocalMapping never touches Tracking's extractors), and the loop body reads
// vMatchedPairs[i].  The images are the views of rectified pairs, so F12 is the fundamental matrix of a sideways baseline (x1^T F12 x2 = y2 - y1)
// and the epipole lies far outside the image.  The example then walks the same inputs with a sequential loop of its own - the contract of
// include/jsorb.h on the host, timed - and fails unless pairs and counts agree.
// Usage: create_new_map_points H W L tile th_fast check_orientation keyframe.raw n0.raw n1.raw n2.raw vocabulary.bin out.bin
//   *.raw: H*W bytes each; vocabulary.bin as examples/track_reference_keyframe.cpp reads it
//   out.bin: int32 n1, counts[3], then per neighbour match12[n1]
// Build: g++ -std=c++17 -I include examples/create_new_map_points.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "jsorb_compat.hpp"

using orb_cuda::SyncedMem;

template <class T> static bool rd(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

// one keyframe on the host: what KeyFrame keeps of its Frame
struct Side {
    std::vector<int> node, octave;
    std::vector<unsigned char> is_free, stereo, desc;
    std::vector<float> x, y, angle;
    int n() const { return (int)node.size(); }
};

static int hamming(const unsigned char *a, const unsigned char *b)
{
    int d = 0;
    for (int w = 0; w < 4; w++) {
        unsigned long long p, q;
        memcpy(&p, a + 8 * w, 8);
        memcpy(&q, b + 8 * w, 8);
        d += __builtin_popcountll(p ^ q);
    }
    return d;
}

static int rot_bin(float a1, float a2)
{
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    const float r = roundf(rot * (1.0f / 30));
    int bin = (r > -1e9f && r < 1e9f) ? (int)r : -1;
    if (bin == 30) bin = 0;
    return bin >= 0 && bin < 30 ? bin : 30;          // 30: never kept
}

// the contract of jsorb_search_for_triangulation_async for one neighbour, sequentially: match12[n1], returns nmatches
static int search_sequential(const jsorb_triangulation_params &p, const Side &k1, const Side &k2, const float *F, float ex, float ey, std::vector<int> &match12)
{
    match12.assign(k1.n(), -1);
    int nmatches = 0;
    std::map<int, std::vector<int>> fv1, fv2;        // DBoW2::FeatureVector: ascending indices per node
    for (int i = 0; i < k1.n(); i++) if (k1.node[i] >= 0) fv1[k1.node[i]].push_back(i);
    for (int i = 0; i < k2.n(); i++) if (k2.node[i] >= 0) fv2[k2.node[i]].push_back(i);
    std::vector<int> hist[31];
    auto it1 = fv1.begin(), it2 = fv2.begin();
    while (it1 != fv1.end() && it2 != fv2.end()) {
        if (it1->first < it2->first) { it1 = fv1.lower_bound(it2->first); continue; }
        if (it2->first < it1->first) { it2 = fv2.lower_bound(it1->first); continue; }
        for (int idx1 : it1->second) {
            if (!k1.is_free[idx1] || (p.only_stereo && !k1.stereo[idx1])) continue;
            const float x1 = k1.x[idx1], y1 = k1.y[idx1];
            const float a = x1 * F[0] + y1 * F[3] + F[6], b = x1 * F[1] + y1 * F[4] + F[7], c = x1 * F[2] + y1 * F[5] + F[8];
            const float den = a * a + b * b;
            int best_dist = p.th_low, best = -1;
            for (int idx2 : it2->second) {
                if (!k2.is_free[idx2] || (p.only_stereo && !k2.stereo[idx2])) continue;
                const int d = hamming(&k1.desc[32 * (size_t)idx1], &k2.desc[32 * (size_t)idx2]);
                if (d > p.th_low || d > best_dist) continue;
                const int oct = k2.octave[idx2];
                if (oct < 0 || oct >= p.n_levels) continue;
                if (!k1.stereo[idx1] && !k2.stereo[idx2]) {
                    const float dx = ex - k2.x[idx2], dy = ey - k2.y[idx2];
                    if (dx * dx + dy * dy < 100.0f * p.scale_factor[oct]) continue;
                }
                const float num = a * k2.x[idx2] + b * k2.y[idx2] + c;
                if (den == 0) continue;
                const float dsqr = num * num / den;
                if (!((double)dsqr < 3.84 * (double)p.level_sigma2[oct])) continue;
                best = idx2;
                best_dist = d;
            }
            if (best < 0) continue;
            match12[idx1] = best;
            nmatches++;
            if (p.check_orientation) hist[rot_bin(k1.angle[idx1], k2.angle[best])].push_back(idx1);
        }
        ++it1;
        ++it2;
    }
    if (p.check_orientation) {                       // ComputeThreeMaxima and the cull
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < 30; i++) {
            const int s = (int)hist[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
        for (int i = 0; i <= 30; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int idx1 : hist[i]) { match12[idx1] = -1; nmatches--; }
        }
    }
    return nmatches;
}

template <class T, class U> static void upload(SyncedMem<T> &m, const std::vector<U> &v)
{
    m.resize(v.empty() ? 1 : v.size());
    for (size_t i = 0; i < v.size(); i++) m.cpu_data()[i] = (T)v[i];
    m.to_gpu();
}

// the device arrays of one side (several keyframes one after the other)
struct DeviceSide {
    SyncedMem<int> node, octave;
    SyncedMem<unsigned char> is_free, stereo, desc;
    SyncedMem<float> x, y, angle;
    jsorb::KeyframeSide side;
    void set(const Side &s)
    {
        upload(node, s.node); upload(octave, s.octave); upload(is_free, s.is_free); upload(stereo, s.stereo); upload(desc, s.desc);
        upload(x, s.x); upload(y, s.y); upload(angle, s.angle);
        side.n = s.n();
        side.node = node.gpu_data(); side.octave = octave.gpu_data(); side.is_free = is_free.gpu_data(); side.stereo = stereo.gpu_data();
        side.descriptors = desc.gpu_data(); side.x = x.gpu_data(); side.y = y.gpu_data(); side.angle = angle.gpu_data();
    }
};

int main(int argc, char **argv)
{
    if (argc != 13) { fprintf(stderr, "usage: %s H W L tile th_fast check_orientation keyframe.raw n0.raw n1.raw n2.raw vocabulary.bin out.bin\n", argv[0]); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th_fast = atoi(argv[5]), rot = atoi(argv[6]);
    std::vector<std::vector<unsigned char>> images(4, std::vector<unsigned char>((size_t)H * W));
    for (int i = 0; i < 4; i++) {
        FILE *f = fopen(argv[7 + i], "rb");
        if (!f || !rd(f, images[i])) { fprintf(stderr, "cannot read %s\n", argv[7 + i]); return 2; }
        fclose(f);
    }
    FILE *f = fopen(argv[11], "rb");
    std::vector<int> head(3);
    if (!f || !rd(f, head) || head[0] < 2) { fprintf(stderr, "cannot read %s\n", argv[11]); return 2; }
    const size_t n_nodes = (size_t)head[0];
    std::vector<int> child_start(n_nodes + 1), children(n_nodes - 1), word_id(n_nodes);
    std::vector<unsigned char> node_desc(32 * n_nodes);
    std::vector<double> weight(n_nodes);
    if (!rd(f, child_start) || !rd(f, children) || !rd(f, node_desc) || !rd(f, word_id) || !rd(f, weight)) { fprintf(stderr, "short vocabulary file\n"); return 2; }
    fclose(f);
    try {
        jsorb::Vocabulary voc(head[0], head[1], head[2], child_start.data(), children.data(), node_desc.data(), word_id.data(), weight.data());
        Jetson_SLAM::ORBExtractor ex(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        // the four keyframes: what each kept of its frame (mvKeysUn, mFeatVec as a node per keypoint, descriptors); every fifth keypoint already
        // has a map point, every second one a stereo measurement
        std::vector<Side> kfs(4);
        for (int k = 0; k < 4; k++) {
            SyncedMem<int> keys;
            SyncedMem<unsigned char> desc;
            ex.extract(images[k].data(), W, keys, desc);
            const int n = jsorb_n_keypoints(ex.handle(), 0);
            Side &s = kfs[k];
            Jetson_SLAM::ComputeBoW(ex, voc, nullptr, &s.node);
            const int *soa = keys.cpu_data();
            const float *angles = reinterpret_cast<const float *>(soa + 3 * (size_t)n);      // keypoint SoA row 3: the angle's float bits
            for (int i = 0; i < n; i++) {
                s.x.push_back((float)soa[i]);
                s.y.push_back((float)soa[(size_t)n + i]);
                s.angle.push_back(angles[i]);
                s.octave.push_back(soa[4 * (size_t)n + i]);
                s.is_free.push_back(i % 5 != 4);
                s.stereo.push_back(i % 2);
            }
            s.desc.assign(desc.cpu_data(), desc.cpu_data() + 32 * (size_t)n);
        }
        // the neighbours one after the other
        Side all;
        std::vector<int32_t> kf_start(1, 0);
        for (int k = 1; k < 4; k++) {
            const Side &s = kfs[k];
            all.node.insert(all.node.end(), s.node.begin(), s.node.end()); all.octave.insert(all.octave.end(), s.octave.begin(), s.octave.end());
            all.is_free.insert(all.is_free.end(), s.is_free.begin(), s.is_free.end()); all.stereo.insert(all.stereo.end(), s.stereo.begin(), s.stereo.end());
            all.desc.insert(all.desc.end(), s.desc.begin(), s.desc.end()); all.x.insert(all.x.end(), s.x.begin(), s.x.end());
            all.y.insert(all.y.end(), s.y.begin(), s.y.end()); all.angle.insert(all.angle.end(), s.angle.begin(), s.angle.end());
            kf_start.push_back(all.n());
        }
        DeviceSide d1, d2;
        d1.set(kfs[0]);
        d2.set(all);
        jsorb_triangulation_params prm{};
        prm.th_low = 50; prm.check_orientation = rot; prm.only_stereo = 0; prm.n_levels = L;      // ORBmatcher matcher(0.6, false): rot = 0
        float scale = 1.0f;
        for (int l = 0; l < L; l++) { prm.scale_factor[l] = scale; prm.level_sigma2[l] = scale * scale; scale *= 1.2f; }
        // ComputeF12 and the epipole per neighbour, from the poses: here every neighbour is a rectified view (a sideways baseline)
        std::vector<float> F12s, epipoles;
        for (int k = 0; k < 3; k++) {
            const float F[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
            F12s.insert(F12s.end(), F, F + 9);
            epipoles.push_back(1e9f);
            epipoles.push_back((float)H / 2);
        }
        jsorb::KeyframeMatcher matcher;
        std::vector<std::vector<std::pair<size_t, size_t>>> vMatchedPairs;
        const std::vector<int> counts = Jetson_SLAM::SearchForTriangulation(matcher, prm, d1.side, 3, kf_start.data(), d2.side, F12s.data(), epipoles.data(), vMatchedPairs);
        // the sequential loop over the same inputs
        const int n1 = kfs[0].n();
        std::vector<std::vector<int>> rows(3);
        int host_counts[3];
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < 3; k++) host_counts[k] = search_sequential(prm, kfs[0], kfs[k + 1], &F12s[9 * k], epipoles[2 * k], epipoles[2 * k + 1], rows[k]);
        const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        bool same = true;
        for (int k = 0; k < 3; k++) {
            std::vector<int> dev_row(n1, -1);
            for (const auto &pr : vMatchedPairs[k]) dev_row[pr.first] = (int)pr.second;
            same = same && counts[k] == host_counts[k] && (int)vMatchedPairs[k].size() == counts[k] && dev_row == rows[k];
        }
        FILE *out = fopen(argv[12], "wb");
        if (!out) { fprintf(stderr, "cannot write %s\n", argv[12]); return 2; }
        fwrite(&n1, 4, 1, out);
        fwrite(counts.data(), 4, 3, out);
        for (int k = 0; k < 3; k++) fwrite(rows[k].data(), 4, rows[k].size(), out);
        fclose(out);
        printf("ok n1=%d neighbours=%d,%d,%d nmatches=%d,%d,%d host_sequential_us=%.1f\n", n1, kfs[1].n(), kfs[2].n(), kfs[3].n(), counts[0], counts[1],
               counts[2], host_us);
        if (!same) { fprintf(stderr, "the device and the sequential loop disagree: host %d,%d,%d\n", host_counts[0], host_counts[1], host_counts[2]); return 1; }
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
