// stereo_rectify_frame.cpp - the stereo frame loop of stereo_frame.cpp fed RAW camera images: the rectification maps are set once per
// extractor (Jetson_SLAM::SetRectifyMaps) and the host cv::remap of Examples/Stereo/stereo_euroc.cpp:145-146 disappears; level 0 of each
// extractor is the remapped image, computed on the device.
// Usage: stereo_rectify_frame H W L tile th fx bf left.raw right.raw mapxL.f32 mapyL.f32 mapxR.f32 mapyR.f32 frames out.bin
//   *.raw: H*W bytes; map*.f32: H*W float32 (what cv::initUndistortRectifyMap returns as CV_32FC1, stereo_euroc.cpp:106-107)
// out.bin: int32 N_l, N_r, then kp_l[6N_l] desc_l[32N_l] kp_r[6N_r] desc_r[32N_r] uRight[N_l] depth[N_l] of the LAST frame (every frame
//          extracts the same raw pair: the results must not change from frame to frame - checked here).
// Build: g++ -std=c++17 -I include examples/stereo_rectify_frame.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "jsorb_compat.hpp"

template <typename T>
static std::vector<T> read_file(const char *path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 16) {
        fprintf(stderr, "usage: %s H W L tile th fx bf left.raw right.raw mapxL mapyL mapxR mapyR frames out.bin\n", argv[0]);
        return 2;
    }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th = atoi(argv[5]), frames = atoi(argv[14]);
    const float fx = (float)atof(argv[6]), mbf = (float)atof(argv[7]);
    const size_t n = (size_t)H * W;
    auto imL = read_file<unsigned char>(argv[8], n), imR = read_file<unsigned char>(argv[9], n);
    auto mxL = read_file<float>(argv[10], n), myL = read_file<float>(argv[11], n), mxR = read_file<float>(argv[12], n), myR = read_file<float>(argv[13], n);
    try {
        Jetson_SLAM::ORBExtractor exL(H, W, 1.2f, L, 9, 14, 7, th, "", tile, tile, false, false, false, true);
        Jetson_SLAM::ORBExtractor exR(H, W, 1.2f, L, 9, 14, 7, th, "", tile, tile, false, false, false, true);
        // once, where stereo_euroc.cpp:106-107 computes the maps (the maps of each camera go to its own extractor)
        Jetson_SLAM::SetRectifyMaps(exL, mxL.data(), myL.data());
        Jetson_SLAM::SetRectifyMaps(exR, mxR.data(), myR.data());
        orb_cuda::SyncedMem<int> kpL, kpR;
        orb_cuda::SyncedMem<unsigned char> dL, dR;
        std::vector<float> mvuRight, mvDepth;
        std::vector<int> first_kp;
        const float mb = mbf / fx;
        for (int frame = 0; frame < frames; frame++) {
            // stereo_euroc.cpp:145-146 remapped imLeft / imRight here; the raw images go straight to the extractors
            std::thread tl([&] { exL.extract(imL.data(), W, kpL, dL); });     // Frame.cpp:107-110
            std::thread tr([&] { exR.extract(imR.data(), W, kpR, dR); });
            tl.join(); tr.join();
            kpL.to_cpu(); kpR.to_cpu(); dL.to_cpu(); dR.to_cpu();             // Frame.cpp:119-122
            Jetson_SLAM::ComputeStereoMatches(exL, exR, mb, mbf, mvuRight, mvDepth);
            std::vector<int> kp(kpL.cpu_data(), kpL.cpu_data() + kpL.count_);
            if (frame == 0) first_kp = kp;
            else if (kp != first_kp) { fprintf(stderr, "frame %d: keypoints differ from frame 0\n", frame); return 3; }
        }
        const int nl = kpL.count_ / 6, nr = kpR.count_ / 6;
        FILE *f = fopen(argv[15], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[15]); return 2; }
        fwrite(&nl, 4, 1, f); fwrite(&nr, 4, 1, f);
        fwrite(kpL.cpu_data(), 4, 6 * (size_t)nl, f); fwrite(dL.cpu_data(), 1, 32 * (size_t)nl, f);
        fwrite(kpR.cpu_data(), 4, 6 * (size_t)nr, f); fwrite(dR.cpu_data(), 1, 32 * (size_t)nr, f);
        fwrite(mvuRight.data(), 4, nl, f); fwrite(mvDepth.data(), 4, nl, f);
        fclose(f);
        int matched = 0;
        for (float d : mvDepth) matched += d > 0;
        printf("N_left=%d N_right=%d matched=%d frames=%d (raw input, rectified on the device)\n", nl, nr, matched, frames);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
