// search_local_points.cpp - Tracking::SearchLocalPoints (Tracking.cpp:1346-1805) of a stereo frame through the C++ shim: extract both images,
// ComputeStereoMatches (mvuRight stays on the device too), the frustum test on function-static SyncedMem (Tracking.cpp:1427-1600), then
// matcher.SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) as Jetson_SLAM::SearchLocalPoints over the SAME device buffers - the
// reference's copy back of u, v, invz, predictedlevel, viewCos, isinfrustum and its host matching loop are gone - and one copy of the matches.
// Usage: search_local_points H W L tile th_fast left.raw right.raw in.bin out.bin
//   left.raw / right.raw: H*W bytes each (rectified)
//   in.bin : int32 n; float P[3][n], Pn[3][n], dist[3][n] (MaxDistance, invariance max / min), R[9], t[3], Ow[3], cam[4] (fx fy cx cy), logsf,
//            mbf, th; uint8 descriptors[n][32]
//   out.bin: int32 nmatches, match_kp[n]; float u[n], v[n], invz[n], viewCos[n]; int32 level[n]; uint8 in[n] (the frustum outputs, for checking)
// Build: g++ -std=c++17 -I include examples/search_local_points.cpp -L jetson_slam_amd -ljsorb -lpthread
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
    int n_points;
    rd(f, &n_points, 4);
    std::vector<float> P(3 * n_points), Pn(3 * n_points), D(3 * n_points);
    float R[9], t[3], Ow_[3], cam[4], logsf, mbf, th;
    rd(f, P.data(), 12 * n_points); rd(f, Pn.data(), 12 * n_points); rd(f, D.data(), 12 * n_points);
    rd(f, R, sizeof R); rd(f, t, sizeof t); rd(f, Ow_, sizeof Ow_); rd(f, cam, sizeof cam); rd(f, &logsf, 4); rd(f, &mbf, 4); rd(f, &th, 4);
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
        // Tracking.cpp:1427-1600: the frustum test on function-static SyncedMem
        static SyncedMem<float> Px, Py, Pz, Pnx, Pny, Pnz, invz, u, v, viewCos, invariance_maxDistance, invariance_minDistance, MaxDistance, Rcw, tcw, Ow;
        static SyncedMem<int> predictedlevel;
        static SyncedMem<unsigned char> isinfrustum, descriptors;
        SyncedMem<float> *in[] = {&Px, &Py, &Pz, &Pnx, &Pny, &Pnz, &MaxDistance, &invariance_maxDistance, &invariance_minDistance};
        const float *src[] = {P.data(), P.data() + n_points, P.data() + 2 * n_points, Pn.data(), Pn.data() + n_points, Pn.data() + 2 * n_points,
                              D.data(), D.data() + n_points, D.data() + 2 * n_points};
        for (int k = 0; k < 9; k++) {
            in[k]->resize(n_points);
            for (int i = 0; i < n_points; i++) in[k]->cpu_data()[i] = src[k][i];
            in[k]->to_gpu_async();
        }
        Rcw.resize(9); tcw.resize(3); Ow.resize(3);
        for (int i = 0; i < 9; i++) Rcw.cpu_data()[i] = R[i];
        for (int i = 0; i < 3; i++) { tcw.cpu_data()[i] = t[i]; Ow.cpu_data()[i] = Ow_[i]; }
        Rcw.to_gpu(); tcw.to_gpu(); Ow.to_gpu();
        invz.resize(n_points); u.resize(n_points); v.resize(n_points); viewCos.resize(n_points); predictedlevel.resize(n_points);
        isinfrustum.resize(n_points);
        // the map points' descriptors (pMP->GetDescriptor(), map_points order), uploaded with the positions
        descriptors.resize(32 * n_points);
        for (size_t i = 0; i < mp_desc.size(); i++) descriptors.cpu_data()[i] = mp_desc[i];
        descriptors.to_gpu_async();
        for (int k = 0; k < 9; k++) in[k]->sync_stream();
        descriptors.sync_stream();
        float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], viewCosAngle = 0.5f;
        int minX = (int)mnMinX, maxX = (int)mnMaxX, minY = (int)mnMinY, maxY = (int)mnMaxY, nScaleLevels = L;
        tracking_cuda::compute_isInFrustum_GPU(n_points, Px.gpu_data(), Py.gpu_data(), Pz.gpu_data(), Pnx.gpu_data(), Pny.gpu_data(), Pnz.gpu_data(),
                                               MaxDistance.gpu_data(), invariance_maxDistance.gpu_data(), invariance_minDistance.gpu_data(),
                                               Rcw.gpu_data(), tcw.gpu_data(), Ow.gpu_data(), fx, fy, cx, cy, minX, maxX, minY, maxY, nScaleLevels,
                                               logsf, viewCosAngle, invz.gpu_data(), u.gpu_data(), v.gpu_data(), predictedlevel.gpu_data(),
                                               viewCos.gpu_data(), isinfrustum.gpu_data());
        // Tracking.cpp:1782-1791 -> the device matcher on the same buffers; mvpMapPoints of a fresh stereo frame hold nothing yet (blocked: none)
        jsorb_search_params prm{th, 0.8f, 100, mbf, mnMinX, mnMinY, inv_w, inv_h, FRAME_GRID_COLS, FRAME_GRID_ROWS};
        std::vector<int> match_kp;
        const int nmatches = Jetson_SLAM::SearchLocalPoints(exl, prm, n_points, u, v, invz, predictedlevel, viewCos, isinfrustum, descriptors,
                                                            jsorb_stereo_uright_device(exl.handle(), 0), nullptr, match_kp);
        // the frustum outputs, copied back only so that the caller can check the matches against a host restatement
        u.to_cpu(); v.to_cpu(); invz.to_cpu(); viewCos.to_cpu(); predictedlevel.to_cpu(); isinfrustum.to_cpu();
        FILE *out = fopen(argv[9], "wb");
        fwrite(&nmatches, 4, 1, out);
        fwrite(match_kp.data(), 4, n_points, out);
        for (auto *o : {&u, &v, &invz, &viewCos}) fwrite(o->cpu_data(), 4, n_points, out);
        fwrite(predictedlevel.cpu_data(), 4, n_points, out);
        fwrite(isinfrustum.cpu_data(), 1, n_points, out);
        fclose(out);
        printf("ok n=%d nmatches=%d\n", n_points, nmatches);
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
