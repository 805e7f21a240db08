// pose_optimization.cpp - the tail of one Tracking::TrackLocalMap step of a stereo frame (Tracking.cpp:1123-1140) with no host hop: the local map
// (Jetson_SLAM::UpdateLocalPoints), the matcher with its match_kp left on the device (jsorb_search_local_points_async), F.mvpMapPoints[bestIdx] = pMP
// on the device (Jetson_SLAM::ApplyMatches) and Optimizer::PoseOptimization on the device (Jetson_SLAM::PoseOptimization) - checked against the path
// it replaces: match_kp copied back, applied on the host, and a plain C++ double loop of the same algorithm (Optimizer.cpp:244-456 with g2o's
// Levenberg-Marquardt over the one SE3 vertex, sums in keypoint order), whose frame rows would then be uploaded again.
// Usage: pose_optimization H W L tile th_fast left.raw right.raw in.bin      (the inputs of examples/track_local_map.cpp)
//        pose_optimization bench EDGES KEYPOINTS      only the replaced path on a synthetic frame of KEYPOINTS keypoints with EDGES matches, timed
//                                                     (tools/pose_optimization_bench.py): "bench edges=.. host_us=.." with the median of 9 runs
// Prints "ok ..." with the time of the replaced path (download, host apply, host loop, upload) in microseconds.
// Exit status 0: the two paths agree - the same return value and outlier flags, Tcw within one float step; 1: they differ; 2: bad input.
// Build: g++ -O2 -std=c++17 -I include examples/pose_optimization.cpp -L jetson_slam_amd -ljsorb -lpthread
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jsorb_compat.hpp"

#define FRAME_GRID_COLS 64
#define FRAME_GRID_ROWS 48

using orb_cuda::SyncedMem;

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } }

// ---- the host loop: g2o::SE3Quat with Eigen's quaternion formulas written out ----
struct Pose { double qx, qy, qz, qw, tx, ty, tz; };

static void normalize(Pose &T)
{
    if (T.qw < 0) { T.qx = -T.qx; T.qy = -T.qy; T.qz = -T.qz; T.qw = -T.qw; }
    const double n = std::sqrt(T.qx * T.qx + T.qy * T.qy + T.qz * T.qz + T.qw * T.qw);
    T.qx /= n; T.qy /= n; T.qz /= n; T.qw /= n;
}

static void quat_of(const double R[3][3], Pose &T)
{
    double t = R[0][0] + R[1][1] + R[2][2], q[4];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[2][1] - R[1][2]) * t; q[1] = (R[0][2] - R[2][0]) * t; q[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[k][j] - R[j][k]) * t; q[j] = (R[j][i] + R[i][j]) * t; q[k] = (R[k][i] + R[i][k]) * t;
    }
    T.qx = q[0]; T.qy = q[1]; T.qz = q[2]; T.qw = q[3];
}

static void matrix_of(const Pose &T, double R[3][3])
{
    const double tx = 2 * T.qx, ty = 2 * T.qy, tz = 2 * T.qz, twx = tx * T.qw, twy = ty * T.qw, twz = tz * T.qw;
    const double txx = tx * T.qx, txy = ty * T.qx, txz = tz * T.qx, tyy = ty * T.qy, tyz = tz * T.qy, tzz = tz * T.qz;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

static void rotate(const Pose &T, double vx, double vy, double vz, double &x, double &y, double &z)
{
    double ux = T.qy * vz - T.qz * vy, uy = T.qz * vx - T.qx * vz, uz = T.qx * vy - T.qy * vx;
    ux += ux; uy += uy; uz += uz;
    x = (vx + T.qw * ux) + (T.qy * uz - T.qz * uy);
    y = (vy + T.qw * uy) + (T.qz * ux - T.qx * uz);
    z = (vz + T.qw * uz) + (T.qx * uy - T.qy * ux);
}

// SE3Quat::exp(dx) * T (se3quat.h:223-257, :104-110)
static Pose oplus(const double dx[6], const Pose &T)
{
    const double o0 = dx[0], o1 = dx[1], o2 = dx[2], theta = std::sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double Om[3][3] = {{0, -o2, o1}, {o2, 0, -o0}, {-o1, o0, 0}};
    double Om2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Om2[i][j] = (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j];
    double ka = 1, kb = 1, kc = 1;
    if (!(theta < 0.00001)) {
        const double s = std::sin(theta), c = std::cos(theta);
        ka = s / theta; kb = (1 - c) / (theta * theta); kc = (theta - s) / std::pow(theta, 3.0);
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double id = i == j ? 1.0 : 0.0;
            if (theta < 0.00001) { V[i][j] = R[i][j] = (id + Om[i][j]) + Om2[i][j]; continue; }
            R[i][j] = (id + ka * Om[i][j]) + kb * Om2[i][j];
            V[i][j] = (id + kb * Om[i][j]) + kc * Om2[i][j];
        }
    Pose E, P;
    quat_of(R, E);
    E.tx = (V[0][0] * dx[3] + V[0][1] * dx[4]) + V[0][2] * dx[5];
    E.ty = (V[1][0] * dx[3] + V[1][1] * dx[4]) + V[1][2] * dx[5];
    E.tz = (V[2][0] * dx[3] + V[2][1] * dx[4]) + V[2][2] * dx[5];
    normalize(E);
    double rx, ry, rz;
    rotate(E, T.tx, T.ty, T.tz, rx, ry, rz);
    P.tx = E.tx + rx; P.ty = E.ty + ry; P.tz = E.tz + rz;
    P.qw = E.qw * T.qw - E.qx * T.qx - E.qy * T.qy - E.qz * T.qz;
    P.qx = E.qw * T.qx + E.qx * T.qw + E.qy * T.qz - E.qz * T.qy;
    P.qy = E.qw * T.qy + E.qy * T.qw + E.qz * T.qx - E.qx * T.qz;
    P.qz = E.qw * T.qz + E.qz * T.qw + E.qx * T.qy - E.qy * T.qx;
    normalize(P);
    return P;
}

struct Edge { double X, Y, Z, ox, oy, our, info; int kp; bool stereo, out; };
struct Cam { double fx, fy, cx, cy, bf, delta_mono, delta_stereo; };

// computeError and chi2() (types_six_dof_expmap.h:153-157, :184-188)
static double edge_error(const Pose &T, const Cam &c, const Edge &ed, double e[3], double p[3])
{
    double rx, ry, rz;
    rotate(T, ed.X, ed.Y, ed.Z, rx, ry, rz);
    const double x = p[0] = rx + T.tx, y = p[1] = ry + T.ty, z = p[2] = rz + T.tz;
    if (!ed.stereo) {
        e[0] = ed.ox - ((x / z) * c.fx + c.cx);
        e[1] = ed.oy - ((y / z) * c.fy + c.cy);
        e[2] = 0;
        return e[0] * (ed.info * e[0]) + e[1] * (ed.info * e[1]);
    }
    const float invz_f = (float)(1.0 / z);
    const double invz = invz_f, r0 = x * invz * c.fx + c.cx, r1 = y * invz * c.fy + c.cy, r2 = r0 - c.bf * invz;
    e[0] = ed.ox - r0; e[1] = ed.oy - r1; e[2] = ed.our - r2;
    return (e[0] * (ed.info * e[0]) + e[1] * (ed.info * e[1])) + e[2] * (ed.info * e[2]);
}

static double robust_rho(const Cam &c, const Edge &ed, bool robust, double chi2, double *rho1)
{
    const double delta = ed.stereo ? c.delta_stereo : c.delta_mono, dsqr = delta * delta;
    if (rho1) *rho1 = 1.0;
    if (!robust || chi2 <= dsqr) return chi2;
    const double sq = std::sqrt(chi2);
    if (rho1) *rho1 = delta / sq;
    return 2 * sq * delta - dsqr;
}

static bool solve6(const double H[6][6], const double b[6], double lambda, double x[6])
{
    double L[6][6] = {}, d[6];
    bool ok = true;
    for (int j = 0; j < 6; j++) {
        double s = H[j][j] + lambda;
        for (int k = 0; k < j; k++) s -= (L[j][k] * L[j][k]) * d[k];
        d[j] = s;
        ok = ok && s > 0;
        for (int i = j + 1; i < 6; i++) {
            double t = H[i][j];
            for (int k = 0; k < j; k++) t -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    if (!ok) return false;
    double y[6];
    for (int i = 0; i < 6; i++) { double s = b[i]; for (int k = 0; k < i; k++) s -= L[i][k] * y[k]; y[i] = s; }
    for (int i = 0; i < 6; i++) y[i] = y[i] / d[i];
    for (int i = 5; i >= 0; i--) { double s = y[i]; for (int k = i + 1; k < 6; k++) s -= L[k][i] * y[k]; y[i] = s; }
    for (int i = 0; i < 6; i++) x[i] = y[i];
    return true;
}

// Optimizer::PoseOptimization over the edges; Tcw in and out; returns nInitialCorrespondences - nBad
static int pose_optimization_host(std::vector<Edge> &E, const Cam &c, float Tcw[16])
{
    const int nE = (int)E.size();
    if (nE < 3) return 0;
    Pose T0;
    double R0[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R0[i][j] = Tcw[i * 4 + j];
    quat_of(R0, T0);
    T0.tx = Tcw[3]; T0.ty = Tcw[7]; T0.tz = Tcw[11];
    normalize(T0);
    Pose est = T0, last = T0;
    int nBad = 0;
    for (int round = 0; round < 4; round++) {
        est = last = T0;
        const bool robust = round < 3;
        if (nE - nBad > 0) {
            double lambda = 0, ni = 2, x[6] = {0, 0, 0, 0, 0, 0};
            int n_small = 0;
            for (int it = 0; it < 10; it++) {
                double chi = 0, g[6] = {0, 0, 0, 0, 0, 0}, H[6][6] = {};
                for (const Edge &ed : E) {
                    if (ed.out) continue;
                    double e[3], p[3], rho1;
                    const double chi2 = edge_error(est, c, ed, e, p);
                    chi += robust_rho(c, ed, robust, chi2, &rho1);
                    const double x_ = p[0], y_ = p[1], invz = 1.0 / p[2], invz_2 = invz * invz;
                    double J[3][6];
                    J[0][0] = x_ * y_ * invz_2 * c.fx; J[0][1] = -(1 + (x_ * x_ * invz_2)) * c.fx; J[0][2] = y_ * invz * c.fx;
                    J[0][3] = -invz * c.fx; J[0][4] = 0; J[0][5] = x_ * invz_2 * c.fx;
                    J[1][0] = (1 + y_ * y_ * invz_2) * c.fy; J[1][1] = -x_ * y_ * invz_2 * c.fy; J[1][2] = -x_ * invz * c.fy;
                    J[1][3] = 0; J[1][4] = -invz * c.fy; J[1][5] = y_ * invz_2 * c.fy;
                    J[2][0] = J[0][0] - c.bf * y_ * invz_2; J[2][1] = J[0][1] + c.bf * x_ * invz_2; J[2][2] = J[0][2];
                    J[2][3] = J[0][3]; J[2][4] = 0; J[2][5] = J[0][5] - c.bf * invz_2;
                    const double w = rho1 * ed.info, ie[3] = {ed.info * e[0], ed.info * e[1], ed.info * e[2]};
                    for (int i = 0; i < 6; i++) {
                        double s = J[0][i] * ie[0] + J[1][i] * ie[1];
                        if (ed.stereo) s += J[2][i] * ie[2];
                        g[i] += rho1 * s;
                        for (int j = i; j < 6; j++) {
                            double h = J[0][i] * (w * J[0][j]) + J[1][i] * (w * J[1][j]);
                            if (ed.stereo) h += J[2][i] * (w * J[2][j]);
                            H[i][j] += h;
                        }
                    }
                }
                double b[6], currentChi = chi;
                const double iniChi = chi;
                for (int i = 0; i < 6; i++) { b[i] = -g[i]; for (int j = 0; j < i; j++) H[i][j] = H[j][i]; }
                if (it == 0) {
                    double mx = 0;
                    for (int j = 0; j < 6; j++) mx = std::fmax(std::fabs(H[j][j]), mx);
                    lambda = 1e-5 * mx; ni = 2; n_small = 0;
                }
                double rho = 0;
                int qmax = 0;
                do {
                    const Pose backup = est;
                    const bool ok2 = solve6(H, b, lambda, x);
                    est = last = oplus(x, est);
                    double tempChi = 0;
                    for (const Edge &ed : E) {
                        if (ed.out) continue;
                        double e[3], p[3];
                        tempChi += robust_rho(c, ed, robust, edge_error(est, c, ed, e, p), nullptr);
                    }
                    if (!ok2) tempChi = DBL_MAX;
                    rho = currentChi - tempChi;
                    double scale = 0;
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    if (rho > 0 && std::isfinite(tempChi)) {
                        double alpha = 1. - std::pow(2 * rho - 1, 3.0);
                        alpha = std::fmin(alpha, 2. / 3.);
                        lambda *= std::fmax(1. / 3., alpha);
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni; ni *= 2; est = backup;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                if (qmax == 10 || rho == 0) break;
                if ((iniChi - currentChi) * 1e3 < iniChi) n_small++;
                else n_small = 0;
                if (n_small >= 3) break;
            }
        }
        nBad = 0;
        for (Edge &ed : E) {
            double e[3], p[3];
            const float chi2 = (float)edge_error(ed.out ? est : last, c, ed, e, p);
            ed.out = ed.stereo ? chi2 > 7.815f : chi2 > 5.991f;
            nBad += ed.out ? 1 : 0;
        }
        if (nE < 10) break;
    }
    double R[3][3];
    matrix_of(est, R);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Tcw[i * 4 + j] = (float)R[i][j];
    Tcw[3] = (float)est.tx; Tcw[7] = (float)est.ty; Tcw[11] = (float)est.tz;
    Tcw[12] = Tcw[13] = Tcw[14] = 0.f; Tcw[15] = 1.f;
    return nE - nBad;
}

// the replaced path alone, on a synthetic frame: match_kp back, applied on the host, the host loop, the rows up again
static int bench(int n_edges, int N)
{
    if (n_edges < 3 || N < n_edges) return 2;
    unsigned long long seed = 12345;
    auto uni = [&]() { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0; };
    const Cam c{435.2f, 435.2f, 376.0f, 240.0f, 47.906f, (double)(float)std::sqrt(5.991), (double)(float)std::sqrt(7.815)};
    std::vector<float> X(n_edges), Y(n_edges), Z(n_edges), kx(N), ky(N), ur(N, -1.0f);
    std::vector<int32_t> match_kp(n_edges), point_row(n_edges);
    for (int k = 0; k < N; k++) { kx[k] = (float)(int)(uni() * 752); ky[k] = (float)(int)(uni() * 480); }
    for (int i = 0; i < n_edges; i++) {
        const int k = (int)((long long)i * N / n_edges);          // distinct keypoints
        const double z = 2 + 13 * uni(), gross = uni() < 0.1 ? 40.0 : 0.0;
        X[i] = (float)((kx[k] + uni() - 0.5 + gross - c.cx) * z / c.fx); Y[i] = (float)((ky[k] + uni() - 0.5 - c.cy) * z / c.fy); Z[i] = (float)z;
        if (i & 1) ur[k] = (float)(kx[k] - c.bf / z);
        match_kp[i] = k; point_row[i] = i;
    }
    jsorb::detail::DeviceArray<int32_t> mk_gpu("bench", (size_t)n_edges), rows_gpu("bench", (size_t)N);
    mk_gpu.upload(0, match_kp.data(), (size_t)n_edges);
    std::vector<double> us;
    int ret = 0;
    for (int rep = 0; rep < 9; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> mk(n_edges), fr(N, -1);
        jsorb::detail::check(jsorb_mem_d2h(mk.data(), mk_gpu.ptr(), 4 * (size_t)n_edges), "bench", "copy back");
        for (int i = 0; i < n_edges; i++)
            if (mk[i] >= 0 && mk[i] < N) fr[mk[i]] = point_row[i];
        std::vector<Edge> E;
        for (int k = 0; k < N; k++) {
            const int r = fr[k];
            if (r < 0) continue;
            E.push_back(Edge{X[r], Y[r], Z[r], kx[k], ky[k], ur[k], 1.0 / (1.0 + (k % 8) * 0.44), k, !(ur[k] < 0), false});
        }
        float Tcw[16] = {1, 0, 0, 0.02f, 0, 1, 0, -0.01f, 0, 0, 1, 0.03f, 0, 0, 0, 1};
        ret = pose_optimization_host(E, c, Tcw);
        rows_gpu.upload(0, fr.data(), (size_t)N);
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("bench edges=%d keypoints=%d inliers=%d host_us=%.1f\n", n_edges, N, ret, us[us.size() / 2]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "bench")) {
        try { return bench(atoi(argv[2]), atoi(argv[3])); } catch (const std::exception &e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    }
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
        if (N < 1) { fprintf(stderr, "the frame has no keypoint\n"); return 2; }
        if (n_frame >= 0 && n_frame != N) { fprintf(stderr, "the frame has %d keypoints, the input %d\n", N, n_frame); return 2; }
        if (n_frame < 0) frame_row.assign(N, -1);
        const float inv_w = (float)FRAME_GRID_COLS / (float)W, inv_h = (float)FRAME_GRID_ROWS / (float)H;
        jsorb_search_params sp{th, 0.8f, 100, mbf, 0.0f, 0.0f, inv_w, inv_h, FRAME_GRID_COLS, FRAME_GRID_ROWS};
        const float *u_right_gpu = jsorb_stereo_uright_device(exl.handle(), 0);
        void *stream = jsorb_get_stream(exl.handle());

        // the table, the local keyframes' rows and the frame's rows on the device
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
        table.scatter(rows, rec, stream);
        table.set_descriptors(0, n_rows, desc.data());
        jsorb::detail::DeviceArray<int32_t> kf_rows_gpu("example", kf_point_row.size()), frame_rows_gpu("example", (size_t)N);
        kf_rows_gpu.upload(0, kf_point_row.data(), kf_point_row.size());
        frame_rows_gpu.upload(0, frame_row.data(), (size_t)N);
        jsorb_frustum_params fp{};
        memcpy(fp.Rcw, R, sizeof R); memcpy(fp.tcw, t, sizeof t); memcpy(fp.Ow, Ow_, sizeof Ow_);
        fp.fx = cam[0]; fp.fy = cam[1]; fp.cx = cam[2]; fp.cy = cam[3];
        fp.minX = 0; fp.maxX = W; fp.minY = 0; fp.maxY = H; fp.nScaleLevels = L;
        fp.logScaleFactor = logsf; fp.viewCosAngle = 0.5f;

        // ---- the device path: local map, search, apply, optimise; nothing but the pose, the flags and the counts comes back ----
        jsorb::LocalMapPoints pts;
        const int capacity = kf_point_row.empty() ? 1 : (int)kf_point_row.size();
        Jetson_SLAM::UpdateLocalPoints(exl, table, fp, kf_start, kf_rows_gpu.ptr(), frame_rows_gpu.ptr(), capacity, pts);
        jsorb::detail::DeviceArray<int32_t> match_kp("example", (size_t)capacity), match_dist("example", (size_t)capacity), kp_match("example", (size_t)N), n_matches("example", 1);
        if (jsorb_search_local_points_async(exl.handle(), 0, &sp, capacity, pts.u.gpu_data(), pts.v.gpu_data(), pts.invz.gpu_data(), pts.predictedlevel.gpu_data(),
                                            pts.viewCos.gpu_data(), pts.isinfrustum.gpu_data(), pts.descriptors.gpu_data(), u_right_gpu, pts.blocked.gpu_data(),
                                            match_kp.ptr(), match_dist.ptr(), kp_match.ptr(), n_matches.ptr()) != JSORB_OK)
            throw std::runtime_error(std::string("jsorb_search_local_points_async: ") + jsorb_last_error(exl.handle()));
        Jetson_SLAM::ApplyMatches(exl, capacity, pts.point_row_gpu.gpu_data(), match_kp.ptr(), frame_rows_gpu.ptr());
        std::vector<float> inv_sigma2(L);
        for (int l = 0; l < L; l++) { const float s = jsorb_scale(exl.handle(), l); inv_sigma2[l] = 1.0f / (s * s); }
        const jsorb::PoseParams pp(cam[0], cam[1], cam[2], cam[3], mbf, inv_sigma2);
        float Tcw_dev[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1}, Tcw_host[16];
        memcpy(Tcw_host, Tcw_dev, sizeof Tcw_dev);
        std::vector<unsigned char> outlier_dev;
        int32_t counts[4];
        const int ret_dev = Jetson_SLAM::PoseOptimization(exl, table, frame_rows_gpu.ptr(), Tcw_dev, outlier_dev, pp, u_right_gpu, nullptr, counts);

        // ---- the path it replaces: match_kp back, applied on the host, the host loop, the rows up again ----
        jsorb::detail::DeviceArray<int32_t> rows_up("example", (size_t)N);
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> mk(capacity);
        jsorb::detail::check(jsorb_mem_d2h(mk.data(), match_kp.ptr(), 4 * (size_t)capacity), "example", "copy back");
        std::vector<int32_t> fr = frame_row;
        for (int i = 0; i < capacity; i++)
            if (mk[i] >= 0 && mk[i] < N && pts.point_row[i] >= 0) fr[mk[i]] = pts.point_row[i];
        const int *soa = kl.cpu_data();
        const Cam c{cam[0], cam[1], cam[2], cam[3], mbf, (double)(float)std::sqrt(5.991), (double)(float)std::sqrt(7.815)};
        std::vector<Edge> E;
        for (int k = 0; k < N; k++) {
            const int r = fr[k];
            if (r < 0 || r >= n_rows) continue;
            const int o = soa[4 * (size_t)N + k];
            Edge ed{T[r], T[(size_t)n_rows + r], T[2 * (size_t)n_rows + r], (double)(float)soa[k], (double)(float)soa[(size_t)N + k], mvuRight[k],
                    inv_sigma2[o < 0 ? 0 : o >= L ? L - 1 : o], k, !(mvuRight[k] < 0), false};
            E.push_back(ed);
        }
        const int ret_host = pose_optimization_host(E, c, Tcw_host);
        rows_up.upload(0, fr.data(), (size_t)N);
        const double host_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();

        std::vector<unsigned char> outlier_host(N, 0);
        for (const Edge &ed : E) outlier_host[ed.kp] = ed.out ? 1 : 0;
        double worst = 0, tmax = 1;
        for (int i = 0; i < 3; i++) tmax = std::fmax(tmax, std::fabs((double)Tcw_host[i * 4 + 3]));
        for (int i = 0; i < 16; i++) worst = std::fmax(worst, std::fabs((double)Tcw_dev[i] - (double)Tcw_host[i]) / (i % 4 == 3 && i < 12 ? tmax : 1.0));
        const bool same = ret_dev == ret_host && counts[0] == (int)E.size() && outlier_dev == outlier_host && worst <= 1.1920928955078125e-07;
        printf("%s edges=%d inliers=%d/%d rounds=%d pose_gap=%.3g host_us=%.1f\n", same ? "ok" : "MISMATCH", (int)E.size(), ret_dev, ret_host, counts[3], worst, host_us);
        return same && ret_dev >= 10 ? 0 : 1;
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
