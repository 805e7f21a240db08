"""The yardstick and the worlds of jsorb_pose_optimization (include/jsorb.h), shared by tests/test_pose_optimization_host.py and
tests/test_gpu_pose_optimization.py.  Not a test module.

reference() is a literal numpy float64 transcription of Optimizer::PoseOptimization (src/Optimizer.cpp:244-456) and of the g2o chain under it, every
sum over the edges SEQUENTIAL in edge order (np.cumsum), float exactly where the reference uses it: the Huber deltas (float)sqrt(5.991) and
(float)sqrt(7.815) (:278-279), the thresholds 5.991f / 7.815f and the (float)chi2 of the test (:374-375, :398, :427), the stereo edge's
const float invz (types_six_dof_expmap.cpp:300), invSigma2 (:304), Xw (:316-318) and the observations (:298, :334).
  errors, Jacobians    Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:266-364, .h:153-157, :184-188
  robust kernel        Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp:78-91
  quadratic form       Thirdparty/g2o/g2o/core/base_unary_edge.hpp:56-66
  LM step              Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
  outer loop           Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:376-414
  update               Thirdparty/g2o/g2o/types/se3quat.h:223-257, :104-110, :280-285 (Eigen's quaternion formulas written out)
  solve                Thirdparty/g2o/g2o/solvers/linear_solver_dense.h:65-113, as an LDL^T without pivoting (include/jsorb.h says so)
  poses in and out     src/Converter.cpp:38-57
Iteration counts, lambda and trial counts are DIAGNOSTICS (`diag`): at convergence rho is rounding noise or exactly 0, so they are never compared
between implementations.  What is compared is what the contract promises: counts, flags, rows and the pose within a tolerance.

It also returns, per world, two margins: the smallest relative margin |chi2 - th| / th over every classification of every round, and the smallest
|rho| of an accept / reject decision.  The worlds are CONDITIONED on the first (>= MARGIN, checked on the CPU by the host test on the transcription
alone; a seed that fails is replaced in the list, never excluded at comparison time); the second has no condition."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
MARGIN = 1e-4
DELTA_MONO, DELTA_STEREO = f64(f32(math.sqrt(5.991))), f64(f32(math.sqrt(7.815)))
TH_MONO, TH_STEREO = f32(5.991), f32(7.815)
FRAME_CONFIG, FRAME_SEED = "c2", 31
N_ROWS = 1500


# ---------------------------------------------------------------- SE3Quat (q = x, y, z, w; t)
def quat_of(R):
    """Eigen: Quaternion(Matrix3)"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
        return q
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q[i] = 0.5 * t
    t = 0.5 / t
    q[3] = (R[k, j] - R[j, k]) * t
    q[j] = (R[j, i] + R[i, j]) * t
    q[k] = (R[k, i] + R[i, k]) * t
    return q


def normalized(q):
    """SE3Quat::normalizeRotation (se3quat.h:280-285)"""
    if q[3] < 0:
        q = -q
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / n


def matrix_of(q):
    """Eigen: Quaternion::toRotationMatrix"""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def rotate(q, v):
    """Eigen: Quaternion * Vector3 on the columns of v (3 x n or 3): uv = 2 vec x v; v + w uv + vec x uv"""
    qx, qy, qz, qw = q
    ux, uy, uz = qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.array([(v[0] + qw * ux) + (qy * uz - qz * uy), (v[1] + qw * uy) + (qz * ux - qx * uz), (v[2] + qw * uz) + (qx * uy - qy * ux)])


def to_se3quat(Tcw):
    """Converter::toSE3Quat (Converter.cpp:38-51): float entries widened"""
    T = np.asarray(Tcw, f32).reshape(4, 4).astype(f64)
    return normalized(quat_of(T[:3, :3])), T[:3, 3].copy()


def oplus(dx, T):
    """SE3Quat::exp(dx) * T: VertexSE3Expmap::oplusImpl.  Returns (pose, theta < 1e-5)"""
    q, t = T
    o0, o1, o2 = dx[0], dx[1], dx[2]
    theta = math.sqrt(o0 * o0 + o1 * o1 + o2 * o2)
    Om = np.array([[0, -o2, o1], [o2, 0, -o0], [-o1, o0, 0]])
    Om2 = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            Om2[i, j] = (Om[i, 0] * Om[0, j] + Om[i, 1] * Om[1, j]) + Om[i, 2] * Om[2, j]
    eye = np.eye(3)
    small = theta < 0.00001
    if small:
        R = (eye + Om) + Om2
        V = R
    else:
        s, c = math.sin(theta), math.cos(theta)
        ka, kb, kc = s / theta, (1 - c) / (theta * theta), (theta - s) / math.pow(theta, 3.0)
        R = (eye + ka * Om) + kb * Om2
        V = (eye + kb * Om) + kc * Om2
    et = np.array([(V[i, 0] * dx[3] + V[i, 1] * dx[4]) + V[i, 2] * dx[5] for i in range(3)])
    eq = normalized(quat_of(R))
    nt = et + rotate(eq, t)
    ax, ay, az, aw = eq
    bx, by, bz, bw = q
    nq = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                   aw * bw - ax * bx - ay * by - az * bz])
    return (normalized(nq), nt), small


# ---------------------------------------------------------------- the edges
def edges_of(W):
    """The edge list in keypoint order (Optimizer.cpp:285-365): dict of arrays over the edges"""
    rows = np.asarray(W["rows"], np.int64)
    has = (rows >= 0) & (rows < W["n_rows"])
    kp = np.nonzero(has)[0]
    r = rows[kp]
    ur = W["u_right"]
    stereo = np.zeros(len(kp), bool) if ur is None else ~(ur[kp] < 0)
    return dict(kp=kp, Xw=W["P"][r].astype(f64).T.copy(), ox=W["x"][kp].astype(f64), oy=W["y"][kp].astype(f64),
                our=(np.full(len(kp), -1.0) if ur is None else ur[kp].astype(f64)), info=W["prm"]["inv_level_sigma2"][np.clip(W["octave"][kp], 0, 15)].astype(f64),
                stereo=stereo, n_outside=int((rows >= W["n_rows"]).sum()))


def camera_of(W):
    p = W["prm"]
    return tuple(f64(f32(p[k])) for k in ("fx", "fy", "cx", "cy", "bf"))


def edge_error(T, cam, E, sel=slice(None)):
    """computeError and chi2() of the selected edges at T: (e 3 x n with e[2] = 0 for a monocular edge, chi2 n, the points in the camera 3 x n)"""
    fx, fy, cx, cy, bf = cam
    q, t = T
    with np.errstate(all="ignore"):
        pc = rotate(q, E["Xw"][:, sel]) + t[:, None]
        x, y, z = pc
        st = E["stereo"][sel]
        ox, oy, our, info = E["ox"][sel], E["oy"][sel], E["our"][sel], E["info"][sel]
        e0m = ox - ((x / z) * fx + cx)
        e1m = oy - ((y / z) * fy + cy)
        invz = (1.0 / z).astype(f32).astype(f64)                 # types_six_dof_expmap.cpp:300: const float invz = 1.0f/trans_xyz[2]
        r0 = x * invz * fx + cx
        r1 = y * invz * fy + cy
        r2 = r0 - bf * invz
        e = np.array([np.where(st, ox - r0, e0m), np.where(st, oy - r1, e1m), np.where(st, our - r2, 0.0)])
        c2 = e[0] * (info * e[0]) + e[1] * (info * e[1])
        chi2 = np.where(st, c2 + e[2] * (info * e[2]), c2)
    return e, chi2, pc


def edge_jacobian(cam, pc, stereo):
    """linearizeOplus (types_six_dof_expmap.cpp:266-288, :335-364): J 3 x 6 x n, the third row zero for a monocular edge"""
    fx, fy, cx, cy, bf = cam
    x, y, z = pc
    with np.errstate(all="ignore"):
        invz = 1.0 / z
        invz_2 = invz * invz
        zero = np.zeros_like(x)
        J0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
        J1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
        J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
        J2 = [np.where(stereo, v, 0.0) for v in J2]
    return np.array([J0, J1, J2])


def robustify(chi2, stereo, robust):
    """RobustKernelHuber::robustify: (rho[0], rho[1]); without the kernel (chi2, 1)"""
    delta = np.where(stereo, DELTA_STEREO, DELTA_MONO)
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = robust & ~(chi2 <= dsqr)
        return np.where(out, 2 * sq * delta - dsqr, chi2), np.where(out, delta / sq, 1.0)


def seq_sum(rows):
    """the sum of the rows of an n x m array, sequential in row order, from 0"""
    if len(rows) == 0:
        return np.zeros(rows.shape[1])
    return np.cumsum(rows, axis=0)[-1]


def linearize(T, cam, E, sel, robust):
    """buildSystem over the selected edges: (robust chi2, b 6, H 6 x 6)"""
    e, chi2, pc = edge_error(T, cam, E, sel)
    st, info = E["stereo"][sel], E["info"][sel]
    rho0, rho1 = robustify(chi2, st, robust)
    J = edge_jacobian(cam, pc, st)
    w = rho1 * info
    ie = info * e
    cols = [rho0]
    with np.errstate(all="ignore"):
        for i in range(6):
            s = J[0, i] * ie[0] + J[1, i] * ie[1]
            cols.append(rho1 * np.where(st, s + J[2, i] * ie[2], s))
        for i in range(6):
            for j in range(i, 6):
                h = J[0, i] * (w * J[0, j]) + J[1, i] * (w * J[1, j])
                cols.append(np.where(st, h + J[2, i] * (w * J[2, j]), h))
        tot = seq_sum(np.stack(cols, axis=1))
    H = np.zeros((6, 6))
    at = 7
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = tot[at]
            at += 1
    return tot[0], -tot[1:7], H


def robust_chi2(T, cam, E, sel, robust):
    _, chi2, _ = edge_error(T, cam, E, sel)
    return seq_sum(robustify(chi2, E["stereo"][sel], robust)[0][:, None])[0]


def ldl_solve(H, b, lam):
    """(H + lam I) x = b by an LDL^T without pivoting; None when a pivot is not > 0"""
    L = np.zeros((6, 6))
    d = np.zeros(6)
    ok = True
    A = H.copy()
    for i in range(6):
        A[i, i] = H[i, i] + lam
    with np.errstate(all="ignore"):
        for j in range(6):
            s = A[j, j]
            for k in range(j):
                s -= (L[j, k] * L[j, k]) * d[k]
            d[j] = s
            ok = ok and bool(s > 0)
            for i in range(j + 1, 6):
                t = A[i, j]
                for k in range(j):
                    t -= (L[i, k] * L[j, k]) * d[k]
                L[i, j] = t / s
        if not ok:
            return None
        y = np.zeros(6)
        for i in range(6):
            s = b[i]
            for k in range(i):
                s -= L[i, k] * y[k]
            y[i] = s
        y = y / d
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s -= L[k, i] * y[k]
            y[i] = s
    return y


# ---------------------------------------------------------------- the call
def reference(W, order=None):
    """jsorb_pose_optimization for one problem.  order: a permutation of the edge list - the order of every sum (None: keypoint order).
    Returns dict(counts, outlier, row_out, pose (12: R row-major, t), Tcw_out (16 float32), class_margin, rho_margin, diag, inliers (edge mask
    after the last round), E)"""
    E = edges_of(W)
    nE, N = len(E["kp"]), W["N"]
    Tin = np.asarray(W["Tcw"], f32).reshape(4, 4)
    rows = np.asarray(W["rows"], np.int32)
    diag = dict(n_outside_rows=E["n_outside"], n_mono=int((~E["stereo"]).sum()), n_stereo=int(E["stereo"].sum()), iterations=0, trials=0, rejected=0,
                failed=0, idle_rounds=0, small_theta=0, readmitted=0, sets=[])
    if nE < 3:
        return dict(counts=np.array([nE, 0, 0, 0], np.int32), outlier=np.zeros(N, np.uint8), row_out=rows.copy(),
                    pose=np.concatenate([Tin[:3, :3].astype(f64).ravel(), Tin[:3, 3].astype(f64)]), Tcw_out=Tin.ravel().copy(), class_margin=np.inf,
                    rho_margin=np.inf, diag=diag, inliers=np.ones(nE, bool), E=E)
    cam = camera_of(W)
    order = np.arange(nE) if order is None else np.asarray(order)
    T0 = to_se3quat(Tin)
    flagged = np.zeros(nE, bool)
    class_margin = rho_margin = np.inf
    n_bad = rounds = 0
    est = T0
    for rnd in range(4):
        est = last = T0
        robust = rnd < 3
        rounds += 1
        act = order[~flagged[order]]
        if len(act) > 0:
            lam, ni, n_small, x = 0.0, 2.0, 0, np.zeros(6)
            for it in range(10):
                current, b, H = linearize(est, cam, E, act, robust)
                ini = current
                if it == 0:
                    lam, ni, n_small = 1e-5 * max(abs(H[j, j]) for j in range(6)), 2.0, 0
                diag["iterations"] += 1
                rho, qmax = 0.0, 0
                while True:
                    backup = est
                    sol = ldl_solve(H, b, lam)
                    if sol is not None:
                        x = sol
                    est, small = oplus(x, est)
                    diag["small_theta"] += int(small)
                    last = est
                    temp = robust_chi2(est, cam, E, act, robust)
                    if sol is None:
                        temp = np.finfo(f64).max
                        diag["failed"] += 1
                    with np.errstate(all="ignore"):
                        rho = current - temp
                        scale = 0.0
                        for j in range(6):
                            scale += x[j] * (lam * x[j] + b[j])
                        scale += 1e-3
                        rho = rho / scale
                    diag["trials"] += 1
                    if not math.isnan(rho):
                        rho_margin = min(rho_margin, abs(rho))
                    if rho > 0 and math.isfinite(temp):
                        alpha = 1.0 - math.pow(2 * rho - 1, 3.0)
                        alpha = min(alpha, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        current = temp
                    else:
                        lam *= ni
                        ni *= 2
                        est = backup
                        diag["rejected"] += 1
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                if qmax == 10 or rho == 0:
                    break
                n_small = n_small + 1 if (ini - current) * 1e3 < ini else 0
                if n_small >= 3:
                    break
        else:
            diag["idle_rounds"] += 1
        # Optimizer.cpp:386-443
        chi_est = edge_error(est, cam, E)[1]
        chi_last = edge_error(last, cam, E)[1]
        chi2 = np.where(flagged, chi_est, chi_last)
        th = np.where(E["stereo"], TH_STEREO, TH_MONO)
        with np.errstate(all="ignore"):
            out = chi2.astype(f32) > th
            m = np.abs(chi2 - th.astype(f64)) / th.astype(f64)
        class_margin = min(class_margin, float(np.min(np.where(np.isnan(m), 0.0, m))))
        diag["readmitted"] += int((flagged & ~out).sum())
        flagged = out
        diag["sets"].append(out.copy())
        n_bad = int(out.sum())
        if nE < 10:
            break
    outlier = np.zeros(N, np.uint8)
    outlier[E["kp"]] = flagged
    row_out = rows.copy()
    row_out[outlier == 1] = -1
    R = matrix_of(est[0])
    Tout = np.zeros((4, 4), f32)
    Tout[:3, :3], Tout[:3, 3], Tout[3, 3] = R.astype(f32), est[1].astype(f32), 1
    return dict(counts=np.array([nE, n_bad, nE - n_bad, rounds], np.int32), outlier=outlier, row_out=row_out, pose=np.concatenate([R.ravel(), est[1]]),
                Tcw_out=Tout.ravel(), class_margin=class_margin, rho_margin=rho_margin, diag=diag, inliers=~flagged, E=E)


def pose_difference(a, b):
    """(max |dR|, |dt|_inf / (1 + |t|_inf)) of two poses of 12 doubles"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return float(np.max(np.abs(a[:9] - b[:9]))), float(np.max(np.abs(a[9:] - b[9:])) / (1 + np.max(np.abs(b[9:]))))


def apply_matches(frame_rows, point_row, match_kp):
    """jsorb_apply_matches_async in numpy (distinct match_kp)"""
    out = np.array(frame_rows, np.int32)
    k, r = np.asarray(match_kp), np.asarray(point_row)
    ok = (k >= 0) & (k < len(out)) & (r >= 0)
    out[k[ok]] = r[ok]
    return out


# ---------------------------------------------------------------- the frames and the worlds
@functools.lru_cache(maxsize=None)
def frame(kind="main"):
    """The frame whose keypoints the worlds hang their edges on: the oracle's extraction, bit-equal to the device's.  kind "blank": no keypoint."""
    from conftest import CONFIGS
    from jetson_slam_amd.synth import synth_image
    from oracle import pyoracle as po
    po.build()
    c = CONFIGS[FRAME_CONFIG if kind == "main" else "tiny"]
    image = synth_image(FRAME_SEED, c["h"], c["w"]) if kind == "main" else np.full((c["h"], c["w"]), 128, np.uint8)
    o = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"])
    o.extract(image)
    kp = np.array(o.keypoints())
    N = len(kp) // 6
    scale = np.array(o.scales(), f32)[:c["L"]]
    sigma2 = (scale * scale).astype(f32)
    inv = np.zeros(16, f32)
    inv[:c["L"]] = (f32(1.0) / sigma2).astype(f32)                # mvInvLevelSigma2 (ORBextractor.cpp: 1.0f / mvLevelSigma2[i])
    return dict(c=c, image=image, kp=kp, N=N, x=kp[:N].astype(f32), y=kp[N:2 * N].astype(f32), octave=kp[4 * N:5 * N].astype(np.int64), inv_level_sigma2=inv)


def small_pose(rng, rot, trans):
    a = rng.normal(0, rot, 3)
    th = np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + (math.sin(th) / th) * K + ((1 - math.cos(th)) / (th * th)) * (K @ K) if th > 0 else np.eye(3)
    return R, rng.normal(0, trans, 3)


def make_world(seed, n_edges, stereo=0.0, noise=0.7, gross=0.0, start=(0.01, 0.05), invalid=0, kind="main", n_rows=N_ROWS, gross_px=(15.0, 80.0)):
    """A problem over the frame `kind`: n_edges keypoints (drawn without replacement) observe table rows made from a true pose with pixel noise
    `noise`; a share `gross` of them is off by gross_px pixels; a share `stereo` has a right coordinate; the initial pose is the true one moved by
    start = (sigma of the rotation vector, sigma of the translation).  invalid: further keypoints with rows outside the table (-1 stays NULL)."""
    F = frame(kind)
    rng = np.random.default_rng(1000 + seed)
    N = F["N"]
    c = F["c"]
    prm = dict(fx=f32(c["fx"]), fy=f32(c["fx"]), cx=f32(c["w"] / 2), cy=f32(c["h"] / 2), bf=f32(c["bf"]), inv_level_sigma2=F["inv_level_sigma2"])
    Rt, tt = small_pose(rng, 0.05, 0.3)
    P = rng.normal(0, 5, (n_rows, 3)).astype(f32)
    bad = (rng.random(n_rows) < 0.2).astype(np.uint8)
    rows = np.full(N, -1, np.int32)
    u_right = np.full(N, -1, f32)
    pick = rng.choice(N, n_edges + invalid, replace=False) if N else np.zeros(0, np.int64)
    kps, extra = pick[:n_edges], pick[n_edges:]
    r = rng.choice(n_rows, n_edges, replace=False)
    z = rng.uniform(2.0, 15.0, n_edges)
    is_gross = rng.random(n_edges) < gross
    off = rng.uniform(gross_px[0], gross_px[1], n_edges) * rng.choice([-1.0, 1.0], n_edges)
    du = rng.normal(0, noise, n_edges) + np.where(is_gross, off, 0.0)
    dv = rng.normal(0, noise, n_edges) + np.where(is_gross, off[::-1], 0.0)
    fx, fy, cx, cy, bf = (f64(prm[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    Pc = np.stack([(F["x"][kps] + du - cx) * z / fx, (F["y"][kps] + dv - cy) * z / fy, z])
    P[r] = (Rt.T @ (Pc - tt[:, None])).T.astype(f32)
    rows[kps] = r
    is_stereo = rng.random(n_edges) < stereo
    ur = (F["x"][kps] - bf / z + rng.normal(0, noise, n_edges)).astype(f32)
    u_right[kps[is_stereo]] = ur[is_stereo]
    if invalid:
        rows[extra] = rng.choice(np.array([n_rows, n_rows + 7, 2 ** 31 - 1, -2, -1000], np.int64), invalid).astype(np.int32)
    dR, dt = small_pose(rng, start[0], start[1])
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = dR @ Rt, dR @ tt + dt
    T_true = np.eye(4)
    T_true[:3, :3], T_true[:3, 3] = Rt, tt
    return dict(kind=kind, N=N, x=F["x"], y=F["y"], octave=F["octave"], u_right=u_right if stereo > 0 else None, rows=rows, n_rows=n_rows, P=P, bad=bad,
                Tcw=Tcw.astype(f32), prm=prm, T_true=T_true, gross=is_gross, kps=kps)


def _bad_row_world():
    W = make_world(21, 40, stereo=0.5)
    W["bad"][W["rows"][W["kps"]]] = 1                 # every observed row is bad: each still gets its edge (Optimizer.cpp:287-288)
    return W


# one world per exit or edge of shape; "claim" is what the host test holds the transcription's diagnostics to
NAMED = {
    "n0": (lambda: make_world(1, 0, kind="blank"), "no_keypoint"),
    "two_edges": (lambda: make_world(2, 2, stereo=0.5), "untouched"),
    "three_mono": (lambda: make_world(3, 3), "one_round"),
    "nine_edges": (lambda: make_world(4, 9, stereo=0.5), "one_round"),
    "ten_edges": (lambda: make_world(5, 10, stereo=0.5), "four_rounds"),
    "all_mono": (lambda: make_world(6, 200, gross=0.1), "four_rounds"),
    "all_stereo": (lambda: make_world(7, 200, stereo=1.0, gross=0.1), "four_rounds"),
    "mixed": (lambda: make_world(8, 200, stereo=0.5, gross=0.1), "four_rounds"),
    "e63": (lambda: make_world(9, 63, stereo=0.5, gross=0.1), "four_rounds"),
    "e64": (lambda: make_world(10, 64, stereo=0.5, gross=0.1), "four_rounds"),
    "e65": (lambda: make_world(11, 65, stereo=0.5, gross=0.1), "four_rounds"),
    "e255": (lambda: make_world(12, 255, stereo=0.5, gross=0.1), "four_rounds"),
    "e256": (lambda: make_world(13, 256, stereo=0.5, gross=0.1), "four_rounds"),
    "e257": (lambda: make_world(14, 257, stereo=0.5, gross=0.1), "four_rounds"),
    "e1000": (lambda: make_world(15, 1000, stereo=0.5, gross=0.15), "four_rounds"),
    "e1100": (lambda: make_world(16, 1100, stereo=0.3, gross=0.1), "four_rounds"),      # beyond threads x registers of the shipped build
    "rows_mixed": (lambda: make_world(17, 120, stereo=0.5, gross=0.1, invalid=60), "outside_rows"),
    "bad_row": (_bad_row_world, "bad_rows"),
    "all_gross": (lambda: make_world(18, 30, stereo=0.5, gross=1.0, gross_px=(1000.0, 3000.0)), "idle_round"),
    "readmit": (lambda: make_world(19, 300, stereo=0.5, gross=0.6), "readmitted"),
    "far_start": (lambda: make_world(31, 150, stereo=0.5, gross=0.05, start=(0.25, 1.5)), "rejected_trials"),
    "tiny_step": (lambda: make_world(22, 80, stereo=0.5, noise=0.0, start=(1e-9, 1e-9)), "small_theta"),
}
# seeded worlds on top: (seed, edges, stereo share, gross share)
SEEDED = [(100, 37, 0.3, 0.2), (101, 130, 0.0, 0.3), (102, 421, 1.0, 0.25), (103, 777, 0.6, 0.4), (104, 1000, 0.5, 0.05), (105, 513, 0.8, 0.5)]
WORLDS = list(NAMED) + ["seed%d" % s[0] for s in SEEDED]
# noise-free and outlier-free: the generating pose must come back
CLEAN = {"clean_mono": lambda: make_world(40, 120, noise=0.0), "clean_stereo": lambda: make_world(41, 120, stereo=1.0, noise=0.0),
         "clean_mixed": lambda: make_world(42, 300, stereo=0.5, noise=0.0, start=(0.03, 0.2))}


@functools.lru_cache(maxsize=None)
def world(name):
    if name in NAMED:
        return NAMED[name][0]()
    if name in CLEAN:
        return CLEAN[name]()
    s = SEEDED[[("seed%d" % x[0]) for x in SEEDED].index(name)]
    return make_world(s[0], s[1], stereo=s[2], gross=s[3])


@functools.lru_cache(maxsize=None)
def expected(name):
    """the transcription's result for a world, computed once and shared"""
    return reference(world(name))


# the largest pose spread the transcription shows under eight seeded permutations of the edge order, over all worlds (measured by
# tests/test_pose_optimization_host.py::test_permutation_spread, which asserts it), and the device tolerance it sets: the
# device differs from the transcription in its summation tree AND in sin / cos / pow and the quaternion's rounding, hence the factor
PERMUTATION_SPREAD = 1.7e-10
DEVICE_FACTOR = 64
