// track_motion_model.cpp - the matching step of Tracking::TrackWithMotionModel (Tracking.cpp:1030-1066) of a stereo frame through the C++ shim:
// extract both images, ComputeStereoMatches (mvuRight stays on the device), then matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, bMono)
// with its retry at 2 th as ONE call, Jetson_SLAM::SearchLastFrame - the reference's K14 / K15 round trips and its host window and histogram
// loops are gone - and one copy of the result.
// Usage: track_motion_model H W L tile th_fast left.raw right.raw in.bin out.bin
//   left.raw / right.raw: H*W bytes each (rectified)
//   in.bin : int32 n; float P[3][n] (world positions of the last frame's map points), angle[n]; int32 octave[n]; float R[9], t[3] (mTcw of the
//            current frame), cam[4] (fx fy cx cy), mbf, th; int32 direction; uint8 descriptors[n][32]
//   out.bin: int32 nmatches, N, kp_match[N]
// Build: g++ -std=c++17 -I include examples/track_motion_model.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

using orb_cuda::SyncedMem;

static void rd(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 10) { fprintf(stderr, "usage: %s H W L tile th_fast left.raw right.raw in.bin out.bin\n", argv[0]); return 2; }
    const int H = atoi(argv[1]), W = atoi(argv[2]), L = atoi(argv[3]), tile = atoi(argv[4]), th_fast = atoi(argv[5]);
    std::vector<unsigned char> left((size_t)H * W), right((size_t)H * W);
    FILE *f = fopen(argv[6], "rb");
    if (!f) return 2;
    rd(f, left.data(), left.size()); fclose(f);
    f = fopen(argv[7], "rb");
    if (!f) return 2;
    rd(f, right.data(), right.size()); fclose(f);
    f = fopen(argv[8], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[8]); return 2; }
    int n_points, direction;
    rd(f, &n_points, 4);
    std::vector<float> P(3 * (size_t)n_points), ang(n_points);
    std::vector<int> oct(n_points);
    float R[9], t[3], cam[4], mbf, th;
    rd(f, P.data(), 12 * (size_t)n_points); rd(f, ang.data(), 4 * (size_t)n_points); rd(f, oct.data(), 4 * (size_t)n_points);
    rd(f, R, sizeof R); rd(f, t, sizeof t); rd(f, cam, sizeof cam); rd(f, &mbf, 4); rd(f, &th, 4); rd(f, &direction, 4);
    std::vector<unsigned char> mp_desc(32 * (size_t)n_points);
    rd(f, mp_desc.data(), mp_desc.size());
    fclose(f);
    try {
        Jetson_SLAM::ORBExtractor exl(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        Jetson_SLAM::ORBExtractor exr(H, W, 1.2f, L, 9, 14, 7, th_fast, std::string(), tile, tile, false, false, false, true);
        SyncedMem<int> kl, kr;
        SyncedMem<unsigned char> dl, dr;
        exl.extract(left.data(), W, kl, dl);
        exr.extract(right.data(), W, kr, dr);
        std::vector<float> mvuRight, mvDepth;
        Jetson_SLAM::ComputeStereoMatches(exl, exr, mbf / cam[0], mbf, mvuRight, mvDepth);
        // Frame::ComputeImageBounds without distortion (Frame.cpp:772-777) and the grid constants of Frame.cpp:60-61
        const float mnMinX = 0.0f, mnMaxX = (float)W, mnMinY = 0.0f, mnMaxY = (float)H;
        const float inv_w = (float)FRAME_GRID_COLS / (mnMaxX - mnMinX), inv_h = (float)FRAME_GRID_ROWS / (mnMaxY - mnMinY);
        // the last frame's points (GetWorldPosExp, mvKeys[].octave, mvKeysUn[].angle, GetDescriptorExp), uploaded once
        SyncedMem<float> Px, Py, Pz, angle;
        SyncedMem<int> octave;
        SyncedMem<unsigned char> descriptors;
        Px.resize(n_points); Py.resize(n_points); Pz.resize(n_points); angle.resize(n_points); octave.resize(n_points); descriptors.resize(32 * n_points);
        for (int i = 0; i < n_points; i++) {
            Px.cpu_data()[i] = P[i]; Py.cpu_data()[i] = P[n_points + i]; Pz.cpu_data()[i] = P[2 * (size_t)n_points + i];
            angle.cpu_data()[i] = ang[i]; octave.cpu_data()[i] = oct[i];
        }
        for (size_t i = 0; i < mp_desc.size(); i++) descriptors.cpu_data()[i] = mp_desc[i];
        Px.to_gpu(); Py.to_gpu(); Pz.to_gpu(); angle.to_gpu(); octave.to_gpu(); descriptors.to_gpu();
        // Tracking.cpp:1045-1064: th (7 for stereo), ORBmatcher(0.9, true), a second pass at 2 th below 20 matches
        jsorb_last_frame_params prm{};
        prm.th = th; prm.th_high = 100; prm.check_orientation = 1; prm.direction = direction; prm.retry_below = 20;
        prm.fx = cam[0]; prm.fy = cam[1]; prm.cx = cam[2]; prm.cy = cam[3];
        prm.min_x = mnMinX; prm.max_x = mnMaxX; prm.min_y = mnMinY; prm.max_y = mnMaxY;
        prm.inv_w = inv_w; prm.inv_h = inv_h; prm.cols = FRAME_GRID_COLS; prm.rows = FRAME_GRID_ROWS; prm.mbf = mbf;
        for (int i = 0; i < 9; i++) prm.Rcw[i] = R[i];
        for (int i = 0; i < 3; i++) prm.tcw[i] = t[i];
        std::vector<int> kp_match;
        const int nmatches = Jetson_SLAM::SearchLastFrame(exl, prm, n_points, Px, Py, Pz, octave, angle, descriptors,
                                                          jsorb_stereo_uright_device(exl.handle(), 0), kp_match);
        const int N = (int)kp_match.size();
        FILE *out = fopen(argv[9], "wb");
        fwrite(&nmatches, 4, 1, out);
        fwrite(&N, 4, 1, out);
        fwrite(kp_match.data(), 4, N, out);
        fclose(out);
        printf("ok n=%d N=%d nmatches=%d\n", n_points, N, nmatches);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
