// track_local_map.cpp - one Tracking::TrackLocalMap step of a stereo frame through the C++ shim, twice: the host loops the reference runs
// (UpdateLocalPoints, Tracking.cpp:1818-1841; the frame marks, map_points, the gathers, the uploads and compute_isInFrustum_GPU of
// SearchLocalPoints, :1352-1600; then the matcher) and the device path that replaces them - Jetson_SLAM::UpdateLocalPoints over a
// jsorb::MapPointTable, then Jetson_SLAM::SearchLocalPoints on its outputs - and checks that both give every keypoint the same map point.
// Usage: track_local_map H W L tile th_fast left.raw right.raw in.bin
//   left.raw / right.raw: H*W bytes each (rectified)
//   in.bin : int32 n_rows; float table[9][n_rows] (P, Pn, MaxDistance, invariance max / min); uint8 desc[n_rows][32]; uint8 bad[n_rows];
//            int32 n_kf, kf_start[n_kf + 1], kf_point_row[kf_start[n_kf]]; int32 n_frame (the frame's keypoints, or -1: no marks), frame_row[n_frame];
//            float R[9], t[3], Ow[3], cam[4] (fx fy cx cy), logsf, mbf, th
// Exit status 0: the two paths agree (and something matched); 1: they differ; 2: bad input.
// Build: g++ -std=c++17 -I include examples/track_local_map.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

using orb_cuda::SyncedMem;

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

// the reference's per-point fields the loops use
struct MapPoint {
    bool bad = false;
    long mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
};

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s H W L tile th_fast left.raw right.raw in.bin\n", argv[0]); return 2; }
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
    int n_rows, n_kf, n_frame;
    rd(f, &n_rows, 4);
    if (n_rows < 1) return 2;
    std::vector<float> T(9 * (size_t)n_rows);
    std::vector<unsigned char> desc(32 * (size_t)n_rows), bad(n_rows);
    rd(f, T.data(), 4 * T.size()); rd(f, desc.data(), desc.size()); rd(f, bad.data(), bad.size());
    rd(f, &n_kf, 4);
    if (n_kf < 0) return 2;
    std::vector<int32_t> kf_start(n_kf + 1, 0);
    rd(f, kf_start.data(), 4 * kf_start.size());
    std::vector<int32_t> kf_point_row(kf_start[n_kf]);
    rd(f, kf_point_row.data(), 4 * kf_point_row.size());
    rd(f, &n_frame, 4);
    std::vector<int32_t> frame_row(n_frame > 0 ? n_frame : 0);
    rd(f, frame_row.data(), 4 * frame_row.size());
    float R[9], t[3], Ow_[3], cam[4], logsf, mbf, th;
    rd(f, R, sizeof R); rd(f, t, sizeof t); rd(f, Ow_, sizeof Ow_); rd(f, cam, sizeof cam); rd(f, &logsf, 4); rd(f, &mbf, 4); rd(f, &th, 4);
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
        const int N = jsorb_n_keypoints(exl.handle(), 0);
        if (n_frame >= 0 && n_frame != N) { fprintf(stderr, "the frame has %d keypoints, the input %d\n", N, n_frame); return 2; }
        const float mnMinX = 0.0f, mnMaxX = (float)W, mnMinY = 0.0f, mnMaxY = (float)H;
        const float inv_w = (float)FRAME_GRID_COLS / (mnMaxX - mnMinX), inv_h = (float)FRAME_GRID_ROWS / (mnMaxY - mnMinY);
        jsorb_search_params prm{th, 0.8f, 100, mbf, mnMinX, mnMinY, inv_w, inv_h, FRAME_GRID_COLS, FRAME_GRID_ROWS};
        const float *u_right_gpu = jsorb_stereo_uright_device(exl.handle(), 0);

        // ---- the host path: Tracking.cpp:1352-1367, :1818-1841, :1410-1600 ----
        const long frame_id = 7;
        std::vector<MapPoint> mps(n_rows);
        for (int r = 0; r < n_rows; r++) mps[r].bad = bad[r] != 0;
        auto lookup = [&](int r) -> MapPoint * { return r >= 0 && r < n_rows ? &mps[r] : nullptr; };
        std::vector<unsigned char> blocked_host(N > 0 ? N : 1, 0);
        for (int k = 0; k < N && n_frame >= 0; k++) {
            MapPoint *pMP = lookup(frame_row[k]);
            if (pMP && !pMP->bad) { pMP->mnLastFrameSeen = frame_id; blocked_host[k] = 1; }
        }
        std::vector<int> mvpLocalMapPoints, map_points;
        for (int k = 0; k < n_kf; k++)
            for (int j = kf_start[k]; j < kf_start[k + 1]; j++) {
                MapPoint *pMP = lookup(kf_point_row[j]);
                if (!pMP) continue;
                if (pMP->mnTrackReferenceForFrame == frame_id) continue;
                if (!pMP->bad) { mvpLocalMapPoints.push_back(kf_point_row[j]); pMP->mnTrackReferenceForFrame = frame_id; }
            }
        for (int r : mvpLocalMapPoints)
            if (mps[r].mnLastFrameSeen != frame_id && !mps[r].bad) map_points.push_back(r);
        const int n_points = (int)map_points.size();
        static SyncedMem<float> in[9], invz, u, v, viewCos, Rcw, tcw, Ow;
        static SyncedMem<int> predictedlevel;
        static SyncedMem<unsigned char> isinfrustum, descriptors, blocked;
        for (int a = 0; a < 9; a++) {
            in[a].resize(n_points > 0 ? n_points : 1);
            for (int i = 0; i < n_points; i++) in[a].cpu_data()[i] = T[(size_t)a * n_rows + map_points[i]];
            in[a].to_gpu();
        }
        descriptors.resize(32 * (n_points > 0 ? n_points : 1));
        for (int i = 0; i < n_points; i++) memcpy(descriptors.cpu_data() + 32 * (size_t)i, desc.data() + 32 * (size_t)map_points[i], 32);
        descriptors.to_gpu();
        blocked.resize((int)blocked_host.size());
        memcpy(blocked.cpu_data(), blocked_host.data(), blocked_host.size());
        blocked.to_gpu();
        Rcw.resize(9); tcw.resize(3); Ow.resize(3);
        for (int i = 0; i < 9; i++) Rcw.cpu_data()[i] = R[i];
        for (int i = 0; i < 3; i++) { tcw.cpu_data()[i] = t[i]; Ow.cpu_data()[i] = Ow_[i]; }
        Rcw.to_gpu(); tcw.to_gpu(); Ow.to_gpu();
        for (auto *o : {&invz, &u, &v, &viewCos}) o->resize(n_points > 0 ? n_points : 1);
        predictedlevel.resize(n_points > 0 ? n_points : 1); isinfrustum.resize(n_points > 0 ? n_points : 1);
        float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], viewCosAngle = 0.5f;
        int minX = (int)mnMinX, maxX = (int)mnMaxX, minY = (int)mnMinY, maxY = (int)mnMaxY, nScaleLevels = L;
        tracking_cuda::compute_isInFrustum_GPU(n_points, in[0].gpu_data(), in[1].gpu_data(), in[2].gpu_data(), in[3].gpu_data(), in[4].gpu_data(),
                                               in[5].gpu_data(), in[6].gpu_data(), in[7].gpu_data(), in[8].gpu_data(), Rcw.gpu_data(), tcw.gpu_data(),
                                               Ow.gpu_data(), fx, fy, cx, cy, minX, maxX, minY, maxY, nScaleLevels, logsf,
                                               viewCosAngle, invz.gpu_data(), u.gpu_data(), v.gpu_data(), predictedlevel.gpu_data(), viewCos.gpu_data(),
                                               isinfrustum.gpu_data());
        isinfrustum.to_cpu();
        int nToMatch = 0;
        for (int i = 0; i < n_points; i++) nToMatch += isinfrustum.cpu_data()[i] != 0;
        std::vector<int> match_host;
        const int nmatches_host = Jetson_SLAM::SearchLocalPoints(exl, prm, n_points, u, v, invz, predictedlevel, viewCos, isinfrustum, descriptors, u_right_gpu,
                                                                 blocked.gpu_data(), match_host);
        std::vector<int> row_of_kp_host(N > 0 ? N : 1, -1);
        for (int i = 0; i < n_points; i++)
            if (match_host[i] >= 0) row_of_kp_host[match_host[i]] = map_points[i];

        // ---- the device path: the table once, then one call for the local map and one for the search ----
        jsorb::MapPointTable table(n_rows);
        std::vector<int32_t> rows(n_rows);
        std::vector<jsorb_map_point_record> rec(n_rows);
        for (int r = 0; r < n_rows; r++) {
            rows[r] = r;
            auto col = [&](int a) { return T[(size_t)a * n_rows + r]; };
            for (int a = 0; a < 3; a++) { rec[r].P[a] = col(a); rec[r].Pn[a] = col(3 + a); }
            rec[r].MaxDistance = col(6); rec[r].invariance_maxDistance = col(7); rec[r].invariance_minDistance = col(8);
            rec[r].bad = bad[r];
            rec[r].pad[0] = rec[r].pad[1] = rec[r].pad[2] = 0;
        }
        table.scatter(rows, rec, jsorb_get_stream(exl.handle()));
        table.set_descriptors(0, n_rows, desc.data());
        SyncedMem<int> kf_rows_gpu, frame_rows_gpu;
        kf_rows_gpu.resize((int)kf_point_row.size() > 0 ? (int)kf_point_row.size() : 1);
        memcpy(kf_rows_gpu.cpu_data(), kf_point_row.data(), 4 * kf_point_row.size());
        kf_rows_gpu.to_gpu();
        frame_rows_gpu.resize(N > 0 ? N : 1);
        if (n_frame >= 0) { memcpy(frame_rows_gpu.cpu_data(), frame_row.data(), 4 * frame_row.size()); frame_rows_gpu.to_gpu(); }
        jsorb_frustum_params fp{};
        memcpy(fp.Rcw, R, sizeof R); memcpy(fp.tcw, t, sizeof t); memcpy(fp.Ow, Ow_, sizeof Ow_);
        fp.fx = fx; fp.fy = fy; fp.cx = cx; fp.cy = cy;
        fp.minX = minX; fp.maxX = maxX; fp.minY = minY; fp.maxY = maxY; fp.nScaleLevels = nScaleLevels;
        fp.logScaleFactor = logsf; fp.viewCosAngle = viewCosAngle;
        jsorb::LocalMapPoints pts;
        const int capacity = (int)kf_point_row.size() > 0 ? (int)kf_point_row.size() : 1;      // never overflows: at most one slot per entry
        const int nToMatch_dev = Jetson_SLAM::UpdateLocalPoints(exl, table, fp, kf_start, kf_rows_gpu.gpu_data(), n_frame >= 0 ? frame_rows_gpu.gpu_data() : nullptr,
                                                                capacity, pts);
        std::vector<int> match_dev;
        const int nmatches_dev = Jetson_SLAM::SearchLocalPoints(exl, prm, pts, u_right_gpu, match_dev);
        std::vector<int> row_of_kp_dev(N > 0 ? N : 1, -1);
        for (int i = 0; i < capacity; i++)
            if (match_dev[i] >= 0) row_of_kp_dev[match_dev[i]] = pts.point_row[i];

        const bool same = nToMatch == nToMatch_dev && nmatches_host == nmatches_dev && row_of_kp_host == row_of_kp_dev &&
                          pts.counts[0] == (int)mvpLocalMapPoints.size() && pts.counts[1] == n_points && pts.counts[4] == 0;
        printf("%s local=%d map_points=%d nToMatch=%d/%d nmatches=%d/%d\n", same ? "ok" : "MISMATCH", (int)mvpLocalMapPoints.size(), n_points, nToMatch,
               nToMatch_dev, nmatches_host, nmatches_dev);
        return same && nmatches_dev > 0 ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
