// triangulate_new_map_points.cpp - the whole loop of LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-457) on the device state through the C++
// shim (Jetson_SLAM::CreateNewMapPoints), against the path it replaces: ONE Jetson_SLAM::SearchForTriangulation for all neighbours, the rows copied
// back, and the loop body from :276 on the host - the contract's arithmetic of include/jsorb.h written out here, with the rule the reference's loop
// implies: a KF1 keypoint that an earlier neighbour has triangulated is skipped (ORBmatcher.cpp:686-690 would not have matched it).
// The map is made here: a current keyframe of 200 keypoints and four neighbours with identity rotations, two with a wide and two with a narrow baseline, 300 points,
// every second keypoint with a stereo measurement, every seventh with a map point already.
// Usage: triangulate_new_map_points            (no input)
// Exit status 0: the device created the points the host loop creates, at the same rows, with the same bits; 1: any difference.
// Build: g++ -std=c++17 -I include examples/triangulate_new_map_points.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "jsorb_compat.hpp"

using orb_cuda::SyncedMem;

namespace {

#ifndef N_KP                                     // (tools/new_points_bench.py builds this file once more at a C2 keyframe's size)
#define N_KP 200
#endif
#ifndef N_NB
#define N_NB 4
#endif
const int N_PTS = N_KP * 3 / 2, S = N_NB + 1, N_NODES = N_KP < 1000 ? 12 : 250, N_LEVELS = 8;
const float FX = 500.0f, FY = 480.0f, CX = 320.0f, CY = 240.0f, MB = 0.1f;

struct Keyframe {                                // what KeyFrame keeps of its Frame, on the host
    std::vector<float> x, y, uright, depth, cos_stereo;
    std::vector<int32_t> octave, node, rows;
    std::vector<unsigned char> desc;
    jsorb_keyframe_pose pose{};
};

double dot3(const float *r, const float *x) { double s = (double)r[0] * (double)x[0]; s = s + (double)r[1] * (double)x[1]; s = s + (double)r[2] * (double)x[2]; return s; }
float norm3(const float *v) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
void rwc(const float *R, const float *v, float *o) { for (int i = 0; i < 3; i++) o[i] = R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2]; }

// the contract's cv::SVD::compute: eight sweeps of one-sided Jacobi in double, vt.row(3) rounded to float
void null_vector(const float Af[4][4], float out[4])
{
    double A[4][4], V[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) { A[i][j] = (double)Af[i][j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 8; sweep++)
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double alpha = A[0][p] * A[0][p], beta = A[0][q] * A[0][q], gamma = A[0][p] * A[0][q];
                for (int k = 1; k < 4; k++) { alpha = alpha + A[k][p] * A[k][p]; beta = beta + A[k][q] * A[k][q]; gamma = gamma + A[k][p] * A[k][q]; }
                if (gamma == 0.0) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 4; k++) { const double a = A[k][p], b = A[k][q]; A[k][p] = c * a - s * b; A[k][q] = s * a + c * b; }
                for (int k = 0; k < 4; k++) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
            }
    int best = 0;
    double least = 0.0;
    for (int j = 0; j < 4; j++) {
        double n = A[0][j] * A[0][j];
        for (int k = 1; k < 4; k++) n = n + A[k][j] * A[k][j];
        if (j == 0 || n <= least) { least = n; best = j; }
    }
    for (int k = 0; k < 4; k++) out[k] = (float)V[k][best];
}

bool reprojection_rejects(const jsorb_keyframe_pose &P, const float *X, float z, float kx, float ky, float ur, bool stereo, float mbf, float sigma2)
{
    const float xc = (float)(dot3(P.Rcw, X) + (double)P.tcw[0]), yc = (float)(dot3(P.Rcw + 3, X) + (double)P.tcw[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = P.fx * xc * invz + P.cx, v = P.fy * yc * invz + P.cy, ex = u - kx, ey = v - ky;
    if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
    const float u_r = u - mbf * invz, er = u_r - ur;
    return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// LocalMapping.cpp:297-437 for one pair: true = the triangulation is successful
bool triangulate(const Keyframe &k1, int i1, const Keyframe &k2, int i2, const jsorb_triangulation_params &prm, float ratio_factor, float *X)
{
    const jsorb_keyframe_pose &P1 = k1.pose, &P2 = k2.pose;
    const bool st1 = k1.uright[i1] >= 0, st2 = k2.uright[i2] >= 0;
    const float xn1[3] = {(k1.x[i1] - P1.cx) * P1.invfx, (k1.y[i1] - P1.cy) * P1.invfy, 1.0f};
    const float xn2[3] = {(k2.x[i2] - P2.cx) * P2.invfx, (k2.y[i2] - P2.cy) * P2.invfy, 1.0f};
    float ray1[3], ray2[3];
    rwc(P1.Rcw, xn1, ray1);
    rwc(P2.Rcw, xn2, ray2);
    const float cos_rays = (float)(dot3(ray1, ray2) / ((double)norm3(ray1) * (double)norm3(ray2)));
    float cos1 = cos_rays + 1.0f, cos2 = cos1;
    if (st1) cos1 = k1.cos_stereo[i1];
    else if (st2) cos2 = k2.cos_stereo[i2];
    const float cos_stereo = cos2 < cos1 ? cos2 : cos1;
    if (cos_rays < cos_stereo && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {
        float A[4][4], h[4];
        for (int j = 0; j < 4; j++) {
            const float a0 = j < 3 ? P1.Rcw[j] : P1.tcw[0], a1 = j < 3 ? P1.Rcw[3 + j] : P1.tcw[1], a2 = j < 3 ? P1.Rcw[6 + j] : P1.tcw[2];
            const float b0 = j < 3 ? P2.Rcw[j] : P2.tcw[0], b1 = j < 3 ? P2.Rcw[3 + j] : P2.tcw[1], b2 = j < 3 ? P2.Rcw[6 + j] : P2.tcw[2];
            A[0][j] = xn1[0] * a2 - a0; A[1][j] = xn1[1] * a2 - a1; A[2][j] = xn2[0] * b2 - b0; A[3][j] = xn2[1] * b2 - b1;
        }
        null_vector(A, h);
        if (h[3] == 0.0f) return false;
        for (int c = 0; c < 3; c++) X[c] = h[c] / h[3];
    } else if ((st1 && cos1 < cos2) || (st2 && cos2 < cos1)) {
        const bool first = st1 && cos1 < cos2;
        const Keyframe &k = first ? k1 : k2;
        const int i = first ? i1 : i2;
        const float z = k.depth[i];
        if (!(z > 0.0f)) return false;
        const float xc[3] = {(k.x[i] - k.pose.cx) * z * k.pose.invfx, (k.y[i] - k.pose.cy) * z * k.pose.invfy, z};      // (mvKeys = mvKeysUn here)
        float r[3];
        rwc(k.pose.Rcw, xc, r);
        for (int c = 0; c < 3; c++) X[c] = r[c] + k.pose.Ow[c];
    } else {
        return false;
    }
    const float z1 = (float)(dot3(P1.Rcw + 6, X) + (double)P1.tcw[2]);
    if (z1 <= 0.0f) return false;
    const float z2 = (float)(dot3(P2.Rcw + 6, X) + (double)P2.tcw[2]);
    if (z2 <= 0.0f) return false;
    if (reprojection_rejects(P1, X, z1, k1.x[i1], k1.y[i1], k1.uright[i1], st1, P1.mbf, prm.level_sigma2[k1.octave[i1]])) return false;
    if (reprojection_rejects(P2, X, z2, k2.x[i2], k2.y[i2], k2.uright[i2], st2, P1.mbf, prm.level_sigma2[k2.octave[i2]])) return false;
    const float n1[3] = {X[0] - P1.Ow[0], X[1] - P1.Ow[1], X[2] - P1.Ow[2]}, n2[3] = {X[0] - P2.Ow[0], X[1] - P2.Ow[1], X[2] - P2.Ow[2]};
    const float dist1 = norm3(n1), dist2 = norm3(n2);
    if (dist1 == 0.0f || dist2 == 0.0f) return false;
    const float ratio_dist = dist2 / dist1, ratio_octave = prm.scale_factor[k1.octave[i1]] / prm.scale_factor[k2.octave[i2]];
    return !(ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor);
}

template <class T, class U> void upload(SyncedMem<T> &m, const std::vector<U> &v)
{
    m.resize(v.empty() ? 1 : v.size());
    for (size_t i = 0; i < v.size(); i++) m.cpu_data()[i] = (T)v[i];
    m.to_gpu();
}

struct DeviceSide {                              // the arrays of Jetson_SLAM::SearchForTriangulation, several keyframes one after the other
    SyncedMem<int> node, octave;
    SyncedMem<unsigned char> is_free, stereo, desc;
    SyncedMem<float> x, y, angle;
    jsorb::KeyframeSide side;
    void set(const std::vector<const Keyframe *> &kfs)
    {
        std::vector<int> n, o;
        std::vector<unsigned char> f, s, d;
        std::vector<float> xs, ys;
        for (const Keyframe *k : kfs)
            for (size_t i = 0; i < k->x.size(); i++) {
                n.push_back(k->node[i]); o.push_back(k->octave[i]); f.push_back(k->rows[i] == -1); s.push_back(k->uright[i] >= 0);
                xs.push_back(k->x[i]); ys.push_back(k->y[i]);
                d.insert(d.end(), k->desc.begin() + 32 * i, k->desc.begin() + 32 * (i + 1));
            }
        const std::vector<float> zero(n.size(), 0.0f);
        upload(node, n); upload(octave, o); upload(is_free, f); upload(stereo, s); upload(desc, d); upload(x, xs); upload(y, ys); upload(angle, zero);
        side.n = (int)n.size();
        side.node = node.gpu_data(); side.octave = octave.gpu_data(); side.is_free = is_free.gpu_data(); side.stereo = stereo.gpu_data();
        side.descriptors = desc.gpu_data(); side.x = x.gpu_data(); side.y = y.gpu_data(); side.angle = angle.gpu_data();
    }
};

} // namespace

int main()
{
    try {
        std::mt19937 rng(2024);
        std::uniform_real_distribution<double> uni(0.0, 1.0);
        std::normal_distribution<double> gauss(0.0, 1.0);
        // the points, and what every keyframe sees of them
        std::vector<std::array<double, 3>> Xw(N_PTS);
        std::vector<std::array<unsigned char, 32>> pdesc(N_PTS);
        for (int p = 0; p < N_PTS; p++) {
            const double z = 3.0 + 5.0 * uni(rng);
            Xw[p] = {(uni(rng) - 0.5) * 0.8 * z, (uni(rng) - 0.5) * 0.6 * z, z};
            for (unsigned char &b : pdesc[p]) b = (unsigned char)(rng() & 255);
        }
        double centre[S][3] = {{0, 0, 0}};       // odd neighbours: a wide baseline to either side; even ones: a narrow one
        for (int s = 1; s < S; s++) {
            const double wide[3] = {(s % 4 == 1 ? 0.4 : -0.4) - 0.01 * s, 0.02 * (s % 3), 0.01 * (s % 5)}, narrow[3] = {0.012, 0.001 * s, s % 4 ? 0.0 : 0.002};
            for (int c = 0; c < 3; c++) centre[s][c] = s % 2 ? wide[c] : narrow[c];
        }
        std::vector<Keyframe> kf(S);
        for (int s = 0; s < S; s++) {
            Keyframe &k = kf[s];
            jsorb_keyframe_pose &P = k.pose;
            const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            memcpy(P.Rcw, I, sizeof(I));
            for (int c = 0; c < 3; c++) { P.tcw[c] = (float)-centre[s][c]; P.Ow[c] = -P.tcw[c]; }
            P.fx = FX; P.fy = FY; P.cx = CX; P.cy = CY; P.invfx = 1.0f / FX; P.invfy = 1.0f / FY; P.mb = MB; P.mbf = MB * FX;
            for (int i = 0; i < N_KP; i++) {
                const int p = (int)((i * 7 + s * 31) % N_PTS);
                const double x = Xw[p][0] - centre[s][0], y = Xw[p][1] - centre[s][1], z = Xw[p][2] - centre[s][2];
                const float u = (float)(FX * x / z + CX + 0.2 * gauss(rng)), v = (float)(FY * y / z + CY + 0.2 * gauss(rng));
                const bool stereo = (i + s) % 2 == 0;
                k.x.push_back(u); k.y.push_back(v);
                k.uright.push_back(stereo ? u - MB * FX / (float)z : -1.0f);
                k.depth.push_back(stereo ? (float)z : -1.0f);
                k.cos_stereo.push_back(stereo ? cosf(2 * atan2f(MB / 2, (float)z)) : 1.0f);      // LocalMapping.cpp:318, once per keypoint
                k.octave.push_back(p % 3 + (i + s) % 2);
                k.node.push_back(p % N_NODES);
                k.rows.push_back(p % 7 == 0 ? p / 7 : -1);
                std::array<unsigned char, 32> d = pdesc[p];
                for (int b = 0; b < 3; b++) { const unsigned bit = rng() & 255; d[bit / 8] ^= (unsigned char)(1u << (bit % 8)); }
                k.desc.insert(k.desc.end(), d.begin(), d.end());
            }
        }
        jsorb_triangulation_params prm{};
        prm.th_low = 50; prm.check_orientation = 0; prm.only_stereo = 0; prm.n_levels = N_LEVELS;
        float scale = 1.0f;
        for (int l = 0; l < N_LEVELS; l++) { prm.scale_factor[l] = scale; prm.level_sigma2[l] = scale * scale; scale *= 1.2f; }
        const float ratio_factor = 1.5f * 1.2f;
        // ComputeF12 and the epipole per neighbour (identity rotations: t12 = t1 - t2)
        std::vector<float> F12, epipole;
        for (int t = 1; t < S; t++) {
            const double tx = centre[t][0] - centre[0][0], ty = centre[t][1] - centre[0][1], tz = centre[t][2] - centre[0][2];
            const double Tx[3][3] = {{0, -tz, ty}, {tz, 0, -tx}, {-ty, tx, 0}}, Ki[3][3] = {{1.0 / FX, 0, -CX / FX}, {0, 1.0 / FY, -CY / FY}, {0, 0, 1}};
            double M[3][3] = {{0}}, F[3][3] = {{0}};
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) M[i][j] += Ki[k][i] * Tx[k][j];
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) F[i][j] += M[i][k] * Ki[k][j];
            for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) F12.push_back((float)F[i][j]);
            const double cz = -tz;               // the current keyframe's centre in the neighbour's frame
            epipole.push_back(cz != 0 ? (float)(FX * -tx / cz + CX) : 1e9f);
            epipole.push_back(cz != 0 ? (float)(FY * -ty / cz + CY) : CY);
        }
        const int n_rows = N_PTS / 7 + 1 + N_KP, pool = S * N_KP;
        std::vector<int32_t> new_rows;
        for (int r = n_rows - 1; r > N_PTS / 7; r--) new_rows.push_back(r);      // the free rows, from the end

        // ---- the device map and the one call ----
        jsorb::KeyframeGraph graph(S, pool, 1);
        jsorb::MapPointTable table(n_rows);
        jsorb::KeyframeKeypoints kp(graph, true);
        jsorb::NewPointKeypoints extra(graph, true);
        for (int s = 0; s < S; s++) {
            graph.set_keyframe(s, kf[s].rows, 100 + s);
            kp.set_keyframe(graph, s, kf[s].x, kf[s].y, kf[s].octave, &kf[s].uright, kf[s].desc);
            extra.set_keyframe(graph, s, kf[s].node, &kf[s].depth, &kf[s].cos_stereo, &kf[s].x, &kf[s].y);
        }
        jsorb::NewPointState state(graph, table);
        jsorb::KeyframeMatcher matcher;
        std::vector<int32_t> neighbours;
        std::vector<jsorb_keyframe_pose> poses(1, kf[0].pose);
        for (int t = 1; t < S; t++) { neighbours.push_back(t); poses.push_back(kf[t].pose); }
        jsorb::NewMapPoints dev;
        const int created = Jetson_SLAM::CreateNewMapPoints(matcher, prm, graph, table, kp, extra, state, 0, N_KP, N_KP, neighbours, poses, F12.data(),
                                                            epipole.data(), ratio_factor, 42, new_rows, dev);

        // ---- the path it replaces: one SearchForTriangulation, then the loop body on the host ----
        DeviceSide d1, d2;
        d1.set({&kf[0]});
        std::vector<const Keyframe *> others;
        for (int t = 1; t < S; t++) others.push_back(&kf[t]);
        d2.set(others);
        std::vector<int32_t> kf_start;
        for (int t = 0; t <= N_NB; t++) kf_start.push_back(t * N_KP);
        std::vector<std::vector<std::pair<size_t, size_t>>> pairs;
        const auto t0 = std::chrono::steady_clock::now();
        Jetson_SLAM::SearchForTriangulation(matcher, prm, d1.side, N_NB, kf_start.data(), d2.side, F12.data(), epipole.data(), pairs);
        std::vector<std::array<int32_t, 4>> host;
        std::vector<std::array<float, 3>> host_x;
        std::vector<char> has_point(N_KP, 0);
        int second_points = 0;
        for (int t = 0; t < N_NB; t++)
            for (const auto &pr : pairs[t]) {
                float X[3];
                if (!triangulate(kf[0], (int)pr.first, kf[1 + t], (int)pr.second, prm, ratio_factor, X)) continue;
                if (has_point[pr.first]) { second_points++; continue; }      // :686-690: the reference would not have matched this keypoint again
                has_point[pr.first] = 1;
                host.push_back({host.size() < new_rows.size() ? new_rows[host.size()] : -1, (int32_t)pr.first, t, (int32_t)pr.second});
                host_x.push_back({X[0], X[1], X[2]});
            }
        const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        bool same = created == (int)host.size() && dev.created == host;
        for (size_t i = 0; same && i < host.size(); i++)
            same = memcmp(&dev.x3D[3 * ((size_t)host[i][2] * N_KP + host[i][1])], host_x[i].data(), 12) == 0 && state.ref_slot(host[i][0]) == 0 &&
                   state.first_kf_id(host[i][0]) == 42;
        printf("created=%d host=%zu second_points_a_literal_loop_would_make=%d matches=%d taken=%d svd=%d unprojected=%d host_path_us=%.0f %s\n", created,
               host.size(), second_points, dev.counts[0], dev.counts[6], dev.counts[9], dev.counts[10], host_us, same ? "ok" : "DIFFERENT");
        if (created < 50 || second_points < 10) { fprintf(stderr, "degenerate example map\n"); return 1; }
        return same ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
