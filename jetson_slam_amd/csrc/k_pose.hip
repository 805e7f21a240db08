// k_pose.hip - Optimizer::PoseOptimization (src/Optimizer.cpp:244-456) on the device: the reprojection edges of a frame, g2o's Levenberg-Marquardt
// over the one SE3 vertex and the four rounds of inlier / outlier classification, for n_problems problems over one image in ONE launch.
//
// k_pose_optimize runs one workgroup a problem for the whole four-round loop.  A problem is a few hundred to a few thousand edges of ~100 flops a
// pass and up to 4 x 10 x 11 passes that depend on each other: it is bound by the latency of a pass, and a pass that crosses workgroups would pay
// a grid-wide barrier each time.  So: the workgroup compacts the problem's edges in keypoint order (a ballot scan over chunks of PO_THREADS
// keypoints), thread t takes the edges t, t + PO_THREADS, ... and keeps the first PO_EDGE_REGS of them in registers (the rest are read again from
// the table every pass), every pass ends in ONE fixed reduction tree - a butterfly over the wave, then the waves' sums in wave order from LDS -
// and EVERY thread runs the 6x6 solve, the exponential and the accept / reject on the reduced sums: the same instructions on the same bits, so
// the decisions are uniform without a broadcast, and a pass costs one barrier.  No floating-point atomics: a problem's result depends on its
// inputs alone, not on the run, on n_problems or on its index in the batch.
//
// The arithmetic is a transcription of the chain the contract cites (include/jsorb.h), in double unless the reference says float, built with
// -ffp-contract=off; tests/pose_optimization_cases.py is the same chain in numpy with sequential sums.
#include "jsorb_launch.h"

#include <cfloat>

namespace jsorb {

#ifndef PO_THREADS
#define PO_THREADS 256                 // threads of a problem's workgroup (a multiple of 64)
#endif
#ifndef PO_EDGE_REGS
#define PO_EDGE_REGS 4                 // edges a thread keeps in registers
#endif
#define PO_WAVES (PO_THREADS / 64)
#define PO_SUMS 28                     // a linearising pass reduces the robust chi2, b (6) and the upper triangle of H (21)

static_assert(PO_THREADS % 64 == 0 && PO_THREADS >= 64 && PO_THREADS <= 1024, "PO_THREADS: whole waves");
static_assert(PO_EDGE_REGS >= 1 && PO_EDGE_REGS <= 8, "PO_EDGE_REGS");

namespace {

struct PoEdge {                        // one edge as the reference builds it (Optimizer.cpp:285-365)
    float X, Y, Z;                     // pMP->GetWorldPos()
    float ox, oy, our;                 // kpUn.pt, mvuRight
    float info;                        // mvInvLevelSigma2[kpUn.octave]
    int kp;                            // the keypoint, bit 31 = stereo
};

struct PoPose { double qx, qy, qz, qw, tx, ty, tz; };      // g2o::SE3Quat: _r, _t

struct PoCam { double fx, fy, cx, cy, bf, delta_mono, delta_stereo; };      // the deltas: the FLOATS sqrt(5.991), sqrt(7.815) (Optimizer.cpp:278-279)

__device__ __forceinline__ PoEdge po_load_edge(const PoseArgs &a, size_t row0, int code)
{
    PoEdge e;
    e.kp = code;
    const int k = code & 0x7fffffff;
    const int r = a.frame_row[row0 + k];       // in [0, n_rows): the compaction kept only those
    e.X = a.Px[r]; e.Y = a.Py[r]; e.Z = a.Pz[r];
    e.ox = a.xy_un ? a.xy_un[k] : (float)a.soa[k];
    e.oy = a.xy_un ? a.xy_un[(size_t)a.N + k] : (float)a.soa[(size_t)a.N + k];
    e.our = code < 0 ? a.u_right[k] : -1.0f;
    const int o = a.soa[4 * (size_t)a.N + k];
    e.info = a.prm.inv_level_sigma2[min(max(o, 0), JSORB_MAX_LEVELS - 1)];
    return e;
}

// Eigen: Quaternion(Matrix3) then SE3Quat::normalizeRotation (se3quat.h:280-285)
__device__ __forceinline__ void po_normalize(PoPose &T)
{
    if (T.qw < 0) { T.qx = -T.qx; T.qy = -T.qy; T.qz = -T.qz; T.qw = -T.qw; }
    const double n = sqrt(T.qx * T.qx + T.qy * T.qy + T.qz * T.qz + T.qw * T.qw);
    T.qx /= n; T.qy /= n; T.qz /= n; T.qw /= n;
}

__device__ __forceinline__ void po_quat_of(const double R[3][3], PoPose &T)
{
    double t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0) {
        t = sqrt(t + 1.0);
        T.qw = 0.5 * t;
        t = 0.5 / t;
        T.qx = (R[2][1] - R[1][2]) * t;
        T.qy = (R[0][2] - R[2][0]) * t;
        T.qz = (R[1][0] - R[0][1]) * t;
    } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {       // i = 0, j = 1, k = 2
        t = sqrt(R[0][0] - R[1][1] - R[2][2] + 1.0);
        T.qx = 0.5 * t;
        t = 0.5 / t;
        T.qw = (R[2][1] - R[1][2]) * t;
        T.qy = (R[1][0] + R[0][1]) * t;
        T.qz = (R[2][0] + R[0][2]) * t;
    } else if (R[1][1] > R[0][0] && R[1][1] >= R[2][2]) {        // i = 1, j = 2, k = 0
        t = sqrt(R[1][1] - R[2][2] - R[0][0] + 1.0);
        T.qy = 0.5 * t;
        t = 0.5 / t;
        T.qw = (R[0][2] - R[2][0]) * t;
        T.qz = (R[2][1] + R[1][2]) * t;
        T.qx = (R[0][1] + R[1][0]) * t;
    } else {                                                     // i = 2, j = 0, k = 1
        t = sqrt(R[2][2] - R[0][0] - R[1][1] + 1.0);
        T.qz = 0.5 * t;
        t = 0.5 / t;
        T.qw = (R[1][0] - R[0][1]) * t;
        T.qx = (R[0][2] + R[2][0]) * t;
        T.qy = (R[1][2] + R[2][1]) * t;
    }
}

// Eigen: Quaternion::toRotationMatrix
__device__ __forceinline__ void po_matrix_of(const PoPose &T, double R[3][3])
{
    const double tx = 2 * T.qx, ty = 2 * T.qy, tz = 2 * T.qz;
    const double twx = tx * T.qw, twy = ty * T.qw, twz = tz * T.qw;
    const double txx = tx * T.qx, txy = ty * T.qx, txz = tz * T.qx, tyy = ty * T.qy, tyz = tz * T.qy, tzz = tz * T.qz;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

// Eigen: Quaternion * Vector3 - uv = 2 vec x v; v + w uv + vec x uv
__device__ __forceinline__ void po_rotate(const PoPose &T, double vx, double vy, double vz, double &x, double &y, double &z)
{
    double ux = T.qy * vz - T.qz * vy, uy = T.qz * vx - T.qx * vz, uz = T.qx * vy - T.qy * vx;
    ux += ux; uy += uy; uz += uz;
    x = (vx + T.qw * ux) + (T.qy * uz - T.qz * uy);
    y = (vy + T.qw * uy) + (T.qz * ux - T.qx * uz);
    z = (vz + T.qw * uz) + (T.qx * uy - T.qy * ux);
}

// SE3Quat::exp(dx) * T (se3quat.h:223-257, :104-110): VertexSE3Expmap::oplusImpl
__device__ __forceinline__ PoPose po_oplus(const double dx[6], const PoPose &T)
{
    const double o0 = dx[0], o1 = dx[1], o2 = dx[2];
    const double theta = sqrt(o0 * o0 + o1 * o1 + o2 * o2);
    const double Om[3][3] = {{0, -o2, o1}, {o2, 0, -o0}, {-o1, o0, 0}};
    double Om2[3][3], R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Om2[i][j] = (Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) V[i][j] = R[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j];
    } else {
        const double s = sin(theta), c = cos(theta);
        const double ka = s / theta, kb = (1 - c) / (theta * theta), kc = (theta - s) / pow(theta, 3.0);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double id = i == j ? 1.0 : 0.0;
                R[i][j] = (id + ka * Om[i][j]) + kb * Om2[i][j];
                V[i][j] = (id + kb * Om[i][j]) + kc * Om2[i][j];
            }
    }
    PoPose E;
    po_quat_of(R, E);
    E.tx = (V[0][0] * dx[3] + V[0][1] * dx[4]) + V[0][2] * dx[5];
    E.ty = (V[1][0] * dx[3] + V[1][1] * dx[4]) + V[1][2] * dx[5];
    E.tz = (V[2][0] * dx[3] + V[2][1] * dx[4]) + V[2][2] * dx[5];
    po_normalize(E);
    PoPose P;
    double rx, ry, rz;
    po_rotate(E, T.tx, T.ty, T.tz, rx, ry, rz);
    P.tx = E.tx + rx; P.ty = E.ty + ry; P.tz = E.tz + rz;
    P.qw = E.qw * T.qw - E.qx * T.qx - E.qy * T.qy - E.qz * T.qz;
    P.qx = E.qw * T.qx + E.qx * T.qw + E.qy * T.qz - E.qz * T.qy;
    P.qy = E.qw * T.qy + E.qy * T.qw + E.qz * T.qx - E.qx * T.qz;
    P.qz = E.qw * T.qz + E.qz * T.qw + E.qx * T.qy - E.qy * T.qx;
    po_normalize(P);
    return P;
}

// computeError and chi2() of the two edges (types_six_dof_expmap.h:153-157, :184-188; .cpp:290-306): e = obs - cam_project(T.map(Xw)), chi2 = e . (info e).
// x, y, z: the point in the camera.
__device__ __forceinline__ double po_error(const PoPose &T, const PoCam &c, const PoEdge &ed, double e[3], double &x, double &y, double &z)
{
    double rx, ry, rz;
    po_rotate(T, (double)ed.X, (double)ed.Y, (double)ed.Z, rx, ry, rz);
    x = rx + T.tx; y = ry + T.ty; z = rz + T.tz;
    const double info = (double)ed.info;
    if (ed.kp >= 0) {
        e[0] = (double)ed.ox - ((x / z) * c.fx + c.cx);
        e[1] = (double)ed.oy - ((y / z) * c.fy + c.cy);
        e[2] = 0;
        return e[0] * (info * e[0]) + e[1] * (info * e[1]);
    }
    const float invz_f = (float)(1.0 / z);       // :300: const float invz = 1.0f/trans_xyz[2]
    const double invz = (double)invz_f;
    const double r0 = x * invz * c.fx + c.cx, r1 = y * invz * c.fy + c.cy, r2 = r0 - c.bf * invz;
    e[0] = (double)ed.ox - r0;
    e[1] = (double)ed.oy - r1;
    e[2] = (double)ed.our - r2;
    return (e[0] * (info * e[0]) + e[1] * (info * e[1])) + e[2] * (info * e[2]);
}

// One edge of buildSystem: linearizeOplus (types_six_dof_expmap.cpp:266-288, :335-364), RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
// and constructQuadraticForm (base_unary_edge.hpp:56-66) into acc: [0] the robust chi2, [1..6] A^T (rho1 Omega e), the upper triangle of A^T (rho1 Omega) A
__device__ __forceinline__ void po_linearize(const PoPose &T, const PoCam &c, const PoEdge &ed, bool robust, double acc[PO_SUMS])
{
    double e[3], x, y, z;
    const double chi2 = po_error(T, c, ed, e, x, y, z);
    const bool stereo = ed.kp < 0;
    const double delta = stereo ? c.delta_stereo : c.delta_mono, dsqr = delta * delta;
    double rho0 = chi2, rho1 = 1.0;
    if (robust && !(chi2 <= dsqr)) {
        const double sq = sqrt(chi2);
        rho0 = 2 * sq * delta - dsqr;
        rho1 = delta / sq;
    }
    acc[0] += rho0;
    const double invz = 1.0 / z, invz_2 = invz * invz;
    double J[3][6];
    J[0][0] = x * y * invz_2 * c.fx;
    J[0][1] = -(1 + (x * x * invz_2)) * c.fx;
    J[0][2] = y * invz * c.fx;
    J[0][3] = -invz * c.fx;
    J[0][4] = 0;
    J[0][5] = x * invz_2 * c.fx;
    J[1][0] = (1 + y * y * invz_2) * c.fy;
    J[1][1] = -x * y * invz_2 * c.fy;
    J[1][2] = -x * invz * c.fy;
    J[1][3] = 0;
    J[1][4] = -invz * c.fy;
    J[1][5] = y * invz_2 * c.fy;
    J[2][0] = J[0][0] - c.bf * y * invz_2;
    J[2][1] = J[0][1] + c.bf * x * invz_2;
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0;
    J[2][5] = J[0][5] - c.bf * invz_2;
    const double info = (double)ed.info, w = rho1 * info;
    const double ie0 = info * e[0], ie1 = info * e[1], ie2 = info * e[2];
    int at = 7;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = J[0][i] * ie0 + J[1][i] * ie1;
        if (stereo) s += J[2][i] * ie2;
        acc[1 + i] += rho1 * s;
#pragma unroll
        for (int j = i; j < 6; j++, at++) {
            double h = J[0][i] * (w * J[0][j]) + J[1][i] * (w * J[1][j]);
            if (stereo) h += J[2][i] * (w * J[2][j]);
            acc[at] += h;
        }
    }
}

// The fixed tree: a butterfly over the wave (every lane ends with the same bits: an addition's operands only swap), then the waves' sums in wave
// order.  red: two buffers of PO_WAVES x PO_SUMS, used in turn, so that a pass costs one barrier.
template <int n> __device__ __forceinline__ void po_reduce(double (&v)[n], double *red, unsigned &turn)
{
#pragma unroll
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[i] += __shfl_xor(v[i], off, 64);
    if (PO_WAVES > 1) {
        double *buf = red + (turn & 1) * (PO_WAVES * PO_SUMS);
        turn++;
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int i = 0; i < n; i++) buf[wave * PO_SUMS + i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < n; i++) {
            double s = buf[i];
#pragma unroll
            for (int w = 1; w < PO_WAVES; w++) s += buf[w * PO_SUMS + i];
            v[i] = s;
        }
    }
}

// linear_solver_dense.h:65-113 for the one 6x6 block: (H + lambda I) x = b by an LDL^T without pivoting; a pivot that is not positive is "not
// positive definite" - x keeps what it held
__device__ __forceinline__ bool po_solve(const double Hu[21], const double b[6], double lambda, double x[6])
{
    double L[6][6], d[6];
    bool ok = true;
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, at++) L[j][i] = Hu[at] + (i == j ? lambda : 0.0);      // the lower triangle of the symmetric matrix
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double s = L[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= (L[j][k] * L[j][k]) * d[k];
        d[j] = s;
        ok = ok && s > 0;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double t = L[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) t -= (L[i][k] * L[j][k]) * d[k];
            L[i][j] = t / s;
        }
    }
    if (!ok) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) y[i] = y[i] / d[i];
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k][i] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) x[i] = y[i];
    return true;
}

// the test of Optimizer.cpp:398-400 / :427-429 on a freshly computed error at T: (float)chi2 > 5.991f, 7.815f for a stereo edge
__device__ __forceinline__ bool po_outlier(const PoPose &T, const PoCam &c, const PoEdge &ed)
{
    double e[3], x, y, z;
    const float chi2 = (float)po_error(T, c, ed, e, x, y, z);
    return ed.kp < 0 ? chi2 > 7.815f : chi2 > 5.991f;
}

__device__ __forceinline__ bool po_uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

} // namespace

__global__ void __launch_bounds__(PO_THREADS) k_pose_optimize(PoseArgs a)
{
    __shared__ double red[2 * PO_WAVES * PO_SUMS];
    __shared__ int wave_n[PO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.x, N = a.N;
    const size_t row0 = (size_t)p * N;
    unsigned turn = 0;

    // ---- the edges, in keypoint order (Optimizer.cpp:285-365): keypoint k has one iff its row lies in the table; bad[] is not read (:287-288) ----
    int nE = 0, n_outside = 0, n_mono = 0, n_stereo = 0;
    for (int base = 0; base < N; base += PO_THREADS) {
        const int k = base + tid;
        const int r = k < N ? a.frame_row[row0 + k] : -1;
        const bool has = r >= 0 && r < a.n_rows;
        const bool stereo = has && a.u_right != nullptr && !(a.u_right[k] < 0);      // :291: mvuRight[i] < 0 is the monocular edge
        if (k < N) {
            a.outlier[row0 + k] = 0;
            if (a.row_out) a.row_out[row0 + k] = r;
        }
        const unsigned long long m = __ballot(has);
        n_outside += __popcll(__ballot(k < N && r >= a.n_rows));
        n_stereo += __popcll(__ballot(stereo));
        n_mono += __popcll(__ballot(has && !stereo));
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PO_WAVES; w++) {
            const int c = wave_n[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (has) a.edge_kp[row0 + nE + before + __popcll(m & ((1ull << lane) - 1))] = k | (stereo ? (int)0x80000000 : 0);
        nE += total;
        __syncthreads();
    }
    if (lane == 0) {                   // this wave's keypoints
        if (n_outside) atomicAdd(&a.stats[0], n_outside);
        if (n_mono) atomicAdd(&a.stats[1], n_mono);
        if (n_stereo) atomicAdd(&a.stats[2], n_stereo);
    }

    const float *Tin = a.Tcw_in + (size_t)p * 16;
    float *Tout = a.Tcw_out + (size_t)p * 16;
    if (nE < 3) {          // :369-370: return 0, the pose untouched
        if (tid < 16) Tout[tid] = Tin[tid];
        if (a.pose_out && tid < 12) a.pose_out[(size_t)p * 12 + tid] = (double)(tid < 9 ? Tin[(tid / 3) * 4 + tid % 3] : Tin[(tid - 9) * 4 + 3]);
        if (tid == 0) {
            int32_t *c = a.counts + (size_t)p * 4;
            c[0] = nE; c[1] = 0; c[2] = 0; c[3] = 0;
        }
        return;
    }

    // ---- this thread's edges: t, t + PO_THREADS, ...; the first PO_EDGE_REGS stay in registers, with their flags in held_out ----
    PoEdge held[PO_EDGE_REGS];
    unsigned held_out = 0;
#pragma unroll
    for (int s = 0; s < PO_EDGE_REGS; s++) {
        const int i = tid + s * PO_THREADS;
        held[s].kp = 0; held[s].X = held[s].Y = held[s].Z = held[s].ox = held[s].oy = held[s].our = held[s].info = 0.f;
        if (i < nE) held[s] = po_load_edge(a, row0, a.edge_kp[row0 + i]);
    }
    const PoCam cam = {(double)a.prm.fx, (double)a.prm.fy, (double)a.prm.cx, (double)a.prm.cy, (double)a.prm.bf, (double)a.delta_mono, (double)a.delta_stereo};

    // Converter::toSE3Quat(pFrame->mTcw) (Converter.cpp:38-51)
    PoPose T0;
    {
        double R[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R[i][j] = (double)Tin[i * 4 + j];
        po_quat_of(R, T0);
        T0.tx = (double)Tin[3]; T0.ty = (double)Tin[7]; T0.tz = (double)Tin[11];
        po_normalize(T0);
    }

    // the ACTIVE edges of this thread (level 0: not flagged), the held ones first: the statements see `ed`
#define PO_FOR_ACTIVE(...)                                                                              \
    do {                                                                                                \
        _Pragma("unroll") for (int s_ = 0; s_ < PO_EDGE_REGS; s_++)                                     \
            if (tid + s_ * PO_THREADS < nE && !((held_out >> s_) & 1)) { const PoEdge &ed = held[s_]; __VA_ARGS__ }   \
        for (int i_ = tid + PO_EDGE_REGS * PO_THREADS; i_ < nE; i_ += PO_THREADS) {                     \
            const int code_ = a.edge_kp[row0 + i_];                                                     \
            if (a.outlier[row0 + (code_ & 0x7fffffff)]) continue;                                       \
            const PoEdge ed = po_load_edge(a, row0, code_);                                             \
            __VA_ARGS__                                                                                 \
        }                                                                                               \
    } while (0)

    PoPose est = T0, last = T0;
    int nBad = 0, rounds = 0, n_iter = 0, n_trials = 0, n_rejected = 0, n_failed = 0, n_idle = 0;
    for (int round = 0; round < 4; round++) {
        // :382-384: setEstimate(mTcw), initializeOptimization(0), optimize(10) - level 0 are the edges not flagged
        est = T0;
        last = T0;
        const bool robust = round < 3;                     // :412-413: the kernel comes off after round index 2
        rounds++;
        if (nE - nBad > 0) {
            double lambda = 0, ni = 2, x[6] = {0, 0, 0, 0, 0, 0};
            int n_small = 0;
            for (int it = 0; it < 10; it++) {              // SparseOptimizer::optimize (sparse_optimizer.cpp:376-414)
                // OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-164)
                double acc[PO_SUMS];
#pragma unroll
                for (int i = 0; i < PO_SUMS; i++) acc[i] = 0;
                PO_FOR_ACTIVE(po_linearize(est, cam, ed, robust, acc););
                po_reduce(acc, red, turn);
                double currentChi = acc[0];
                const double iniChi = currentChi;
                double b[6];
#pragma unroll
                for (int i = 0; i < 6; i++) b[i] = -acc[1 + i];
                const double *Hu = acc + 7;
                if (it == 0) {                             // computeLambdaInit (:166-180): _tau = 1e-5
                    double mx = 0;
                    mx = fmax(fabs(Hu[0]), mx); mx = fmax(fabs(Hu[6]), mx); mx = fmax(fabs(Hu[11]), mx);
                    mx = fmax(fabs(Hu[15]), mx); mx = fmax(fabs(Hu[18]), mx); mx = fmax(fabs(Hu[20]), mx);
                    lambda = 1e-5 * mx;
                    ni = 2;
                    n_small = 0;
                }
                n_iter++;
                double rho = 0;
                int qmax = 0;
                bool again;
                do {
                    const PoPose backup = est;
                    const bool ok2 = po_solve(Hu, b, lambda, x);
                    est = po_oplus(x, est);
                    last = est;
                    double chi[1] = {0};
                    PO_FOR_ACTIVE(
                        double e[3], px, py, pz;
                        const double c2 = po_error(est, cam, ed, e, px, py, pz);
                        const double delta = ed.kp < 0 ? cam.delta_stereo : cam.delta_mono, dsqr = delta * delta;
                        chi[0] += (robust && !(c2 <= dsqr)) ? 2 * sqrt(c2) * delta - dsqr : c2;
                    );
                    po_reduce(chi, red, turn);
                    double tempChi = chi[0];
                    if (!ok2) tempChi = DBL_MAX;
                    rho = currentChi - tempChi;
                    double scale = 0;                      // computeScale (:182-189)
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    scale += 1e-3;
                    rho /= scale;
                    n_trials++;
                    n_failed += ok2 ? 0 : 1;
                    if (po_uniform(rho > 0 && isfinite(tempChi))) {
                        double alpha = 1. - pow(2 * rho - 1, 3.0);
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha);
                        ni = 2;
                        currentChi = tempChi;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = backup;
                        n_rejected++;
                    }
                    qmax++;
                    again = po_uniform(rho < 0 && qmax < 10);
                } while (again);
                if (po_uniform(qmax == 10 || rho == 0)) break;         // Terminate
                if ((iniChi - currentChi) * 1e3 < iniChi) n_small++;   // :155-161
                else n_small = 0;
                if (po_uniform(n_small >= 3)) break;
            }
        } else {
            n_idle++;                                      // optimize() returns -1 (sparse_optimizer.cpp:356-359): the estimate stays
        }
        // :386-443: an edge flagged before this round is tested on a fresh error at the estimate, every other one on the error its last
        // computeError left - the last trial's pose, rejected or not
        double bad[1] = {0};
#pragma unroll
        for (int s = 0; s < PO_EDGE_REGS; s++)
            if (tid + s * PO_THREADS < nE) {
                const bool out = po_outlier((held_out >> s) & 1 ? est : last, cam, held[s]);
                held_out = (held_out & ~(1u << s)) | ((out ? 1u : 0u) << s);
                a.outlier[row0 + (held[s].kp & 0x7fffffff)] = out ? 1 : 0;
                bad[0] += out ? 1.0 : 0.0;
            }
        for (int i = tid + PO_EDGE_REGS * PO_THREADS; i < nE; i += PO_THREADS) {
            const int code = a.edge_kp[row0 + i];
            const size_t at = row0 + (code & 0x7fffffff);
            const bool out = po_outlier(a.outlier[at] ? est : last, cam, po_load_edge(a, row0, code));
            a.outlier[at] = out ? 1 : 0;
            bad[0] += out ? 1.0 : 0.0;
        }
        po_reduce(bad, red, turn);
        nBad = (int)bad[0];
        if (nE < 10) break;                                // :445-446: optimizer.edges().size() < 10
    }
#undef PO_FOR_ACTIVE

    // :449-455: Converter::toCvMat(SE3quat_recov) (Converter.cpp:53-57), the discard of Tracking.cpp:1086-1103 on the rows
    if (a.row_out)
        for (int i = tid; i < nE; i += PO_THREADS) {
            const size_t at = row0 + (a.edge_kp[row0 + i] & 0x7fffffff);
            if (a.outlier[at]) a.row_out[at] = -1;
        }
    if (tid == 0) {
        double R[3][3];
        po_matrix_of(est, R);
        const double t[3] = {est.tx, est.ty, est.tz};
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) {
                Tout[i * 4 + j] = (float)R[i][j];
                if (a.pose_out) a.pose_out[(size_t)p * 12 + i * 3 + j] = R[i][j];
            }
            Tout[i * 4 + 3] = (float)t[i];
            if (a.pose_out) a.pose_out[(size_t)p * 12 + 9 + i] = t[i];
        }
        Tout[12] = 0.f; Tout[13] = 0.f; Tout[14] = 0.f; Tout[15] = 1.f;
        int32_t *c = a.counts + (size_t)p * 4;
        c[0] = nE; c[1] = nBad; c[2] = nE - nBad; c[3] = rounds;
        atomicAdd(&a.stats[3], n_iter);
        atomicAdd(&a.stats[4], n_trials);
        atomicAdd(&a.stats[5], n_rejected);
        atomicAdd(&a.stats[6], n_failed);
        atomicAdd(&a.stats[7], n_idle);
    }
}

// F.mvpMapPoints[bestIdx] = pMP (ORBmatcher.cpp:107, Tracking.cpp's use of the matchers): match i assigns its point's row to its keypoint
__global__ void __launch_bounds__(256) k_apply_matches(int n_points, const int32_t *point_row, const int32_t *match_kp, int N, int32_t *frame_point_row)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_points) return;
    const int k = match_kp[i], r = point_row[i];
    if (k >= 0 && k < N && r >= 0) frame_point_row[k] = r;
}

int pose_threads() { return PO_THREADS; }
int pose_edge_regs() { return PO_EDGE_REGS; }

void launch_pose_optimize(const PoseArgs &a, hipStream_t s)
{
    if (a.n_problems <= 0) return;
    hipLaunchKernelGGL(k_pose_optimize, dim3(a.n_problems), dim3(PO_THREADS), 0, s, a);
}

void launch_apply_matches(int n_points, const int32_t *point_row, const int32_t *match_kp, int N, int32_t *frame_point_row, hipStream_t s)
{
    if (n_points <= 0 || N <= 0) return;
    hipLaunchKernelGGL(k_apply_matches, dim3((n_points + 255) / 256), dim3(256), 0, s, n_points, point_row, match_kp, N, frame_point_row);
}

} // namespace jsorb
