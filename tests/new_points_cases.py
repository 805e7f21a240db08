"""The worlds and the yardstick of jsorb_create_new_map_points (include/jsorb.h): a literal, SEQUENTIAL numpy transcription of the loop of
LocalMapping::CreateNewMapPoints (LocalMapping.cpp:243-457) with MapPoint's constructor, AddObservation / AddMapPoint, ComputeDistinctiveDescriptors
for two observations and UpdateNormalAndDepth (MapPoint.cpp:37-49, :385-406) in float32 / float64 scalars in the contract's order.  The loop runs the
neighbours one after the other and matches each with the KF1 flags as the neighbours before it left them (ORBmatcher.cpp:686-690 through
tests/test_triangulation_host.py's transcription of SearchForTriangulation): the closed form the device uses - a keypoint belongs to the first
neighbour whose pair is accepted - is what this file CHECKS, not what it assumes.  No code is shared with the kernels.  Used by
tests/test_new_points_host.py and tests/test_gpu_new_points.py."""
import math

import numpy as np

from test_triangulation_host import scale_tables, search_for_triangulation_reference, skew

f32 = np.float32
VERDICTS = ("no_match", "created", "taken", "low_parallax", "w_zero", "z1", "z2", "reprojection1", "reprojection2", "zero_distance", "scale_ratio",
            "no_row", "empty_unprojection", "skipped_neighbour")
V = {k: i for i, k in enumerate(VERDICTS)}
COUNTS = ("n_matches", "n_accepted", "n_owning", "n_created", "n_shared_kf2", "n_no_row", "n_taken", "n_skipped_neighbours", "log_overflow", "n_svd",
          "n_unprojected", "no_current")
OUTPUTS = ("verdict", "path", "x3D", "log", "counts")
STATE = ("point_pool", "registered", "floats", "tdesc", "bad", "ref_slot", "replaced", "visible", "found", "first_kf_id")
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
CHUNKS = (1024, 64)                              # the compaction's chunk: the shipped build, the tiny_new_points variant
POSE_KEYS = ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")


# ---- the contract's cv:: operations ----
def dot3(r, x):
    """Mat::dot: double products summed left to right, a double"""
    s = float(r[0]) * float(x[0])
    s = s + float(r[1]) * float(x[1])
    s = s + float(r[2]) * float(x[2])
    return s


def norm3(v):
    """cv::norm: sqrtf of the float sum of squares"""
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def rwc_times(R, v):
    """Rcw.t() * v: every row summed left to right in float"""
    return [R[i] * v[0] + R[3 + i] * v[1] + R[6 + i] * v[2] for i in range(3)]


def ddiv(a, b):
    """IEEE double division (Python raises where IEEE gives inf / nan)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def null_vector(A32):
    """the contract's cv::SVD::compute(A): vt.row(3) as four float32, and the double column for tests/test_new_points_host.py"""
    A = [[float(A32[i][j]) for j in range(4)] for i in range(4)]
    Vm = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            alpha = A[0][p] * A[0][p]
            beta = A[0][q] * A[0][q]
            gamma = A[0][p] * A[0][q]
            for k in range(1, 4):
                alpha = alpha + A[k][p] * A[k][p]
                beta = beta + A[k][q] * A[k][q]
                gamma = gamma + A[k][p] * A[k][q]
            if gamma == 0.0:
                continue
            zeta = ddiv(beta - alpha, 2.0 * gamma)
            t = ddiv(-1.0 if zeta < 0.0 else 1.0, abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = ddiv(1.0, math.sqrt(1.0 + t * t))
            s = c * t
            for M in (A, Vm):
                for k in range(4):
                    mp, mq = M[k][p], M[k][q]
                    M[k][p] = c * mp - s * mq
                    M[k][q] = s * mp + c * mq
    best, least = 0, 0.0
    for j in range(4):
        n = A[0][j] * A[0][j]
        for k in range(1, 4):
            n = n + A[k][j] * A[k][j]
        if j == 0 or n <= least:
            least, best = n, j
    col = [Vm[k][best] for k in range(4)]
    return [f32(c) for c in col], col


def pose_of(W, i):
    """keyframe i of W['poses'] as float32 scalars and lists"""
    p = W["poses"][i]
    d = dict(R=[f32(v) for v in p["Rcw"]], t=[f32(v) for v in p["tcw"]], Ow=[f32(v) for v in p["Ow"]])
    d.update({k: f32(p[k]) for k in POSE_KEYS})
    return d


def reprojection_rejects(W, P, X, z, kx, ky, ur, stereo, mbf, octave):
    """:368-419 for one keyframe; mbf is the CURRENT keyframe's for both (:412)"""
    s2 = float(W["prm"]["level_sigma2"][octave])
    xc = f32(dot3(P["R"][0:3], X) + float(P["t"][0]))
    yc = f32(dot3(P["R"][3:6], X) + float(P["t"][1]))
    invz = f32(ddiv(1.0, float(z)))
    u = P["fx"] * xc * invz + P["cx"]
    v = P["fy"] * yc * invz + P["cy"]
    ex, ey = u - kx, v - ky
    if not stereo:
        return float(ex * ex + ey * ey) > 5.991 * s2
    u_r = u - mbf * invz
    er = u_r - ur
    return float(ex * ex + ey * ey + er * er) > 7.8 * s2


def pair_verdict(W, P1, P2, e1, e2, svd_log=None):
    """:297-437 for one matched pair: (verdict, path, x3D[3])"""
    kx1, ky1, kx2, ky2 = f32(W["x"][e1]), f32(W["y"][e1]), f32(W["x"][e2]), f32(W["y"][e2])
    ur1 = f32(W["uright"][e1]) if W["uright"] is not None else f32(-1)
    ur2 = f32(W["uright"][e2]) if W["uright"] is not None else f32(-1)
    st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
    o1, o2 = int(W["octave"][e1]), int(W["octave"][e2])
    one = f32(1)
    xn1 = [(kx1 - P1["cx"]) * P1["invfx"], (ky1 - P1["cy"]) * P1["invfy"], one]
    xn2 = [(kx2 - P2["cx"]) * P2["invfx"], (ky2 - P2["cy"]) * P2["invfy"], one]
    ray1, ray2 = rwc_times(P1["R"], xn1), rwc_times(P2["R"], xn2)
    cos_rays = f32(ddiv(dot3(ray1, ray2), float(norm3(ray1)) * float(norm3(ray2))))
    cos1 = cos2 = cos_rays + one
    if st1:
        cos1 = f32(W["cos_stereo"][e1])
    elif st2:
        cos2 = f32(W["cos_stereo"][e2])
    cos_stereo = cos2 if cos2 < cos1 else cos1
    zero = [f32(0)] * 3
    if cos_rays < cos_stereo and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
        path = 1
        T1 = [[P1["R"][3 * r + j] for j in range(3)] + [P1["t"][r]] for r in range(3)]
        T2 = [[P2["R"][3 * r + j] for j in range(3)] + [P2["t"][r]] for r in range(3)]
        A = [[xn1[0] * T1[2][j] - T1[0][j] for j in range(4)], [xn1[1] * T1[2][j] - T1[1][j] for j in range(4)],
             [xn2[0] * T2[2][j] - T2[0][j] for j in range(4)], [xn2[1] * T2[2][j] - T2[1][j] for j in range(4)]]
        h, col = null_vector(A)
        if svd_log is not None:
            svd_log.append((np.array(A, np.float32), np.array(col, np.float64)))
        if h[3] == 0:
            return V["w_zero"], path, zero
        X = [h[0] / h[3], h[1] / h[3], h[2] / h[3]]
    elif (st1 and cos1 < cos2) or (st2 and cos2 < cos1):
        first = st1 and cos1 < cos2
        path, P, e = (2, P1, e1) if first else (3, P2, e2)
        z = f32(W["depth"][e])
        if not z > 0:
            return V["empty_unprojection"], path, zero
        u = f32(W["raw_x"][e]) if W["raw_x"] is not None else f32(W["x"][e])
        v = f32(W["raw_y"][e]) if W["raw_y"] is not None else f32(W["y"][e])
        xc = [(u - P["cx"]) * z * P["invfx"], (v - P["cy"]) * z * P["invfy"], z]
        r = rwc_times(P["R"], xc)
        X = [r[0] + P["Ow"][0], r[1] + P["Ow"][1], r[2] + P["Ow"][2]]
    else:
        return V["low_parallax"], 0, zero
    z1 = f32(dot3(P1["R"][6:9], X) + float(P1["t"][2]))
    if z1 <= 0:
        return V["z1"], path, X
    z2 = f32(dot3(P2["R"][6:9], X) + float(P2["t"][2]))
    if z2 <= 0:
        return V["z2"], path, X
    if reprojection_rejects(W, P1, X, z1, kx1, ky1, ur1, st1, P1["mbf"], o1):
        return V["reprojection1"], path, X
    if reprojection_rejects(W, P2, X, z2, kx2, ky2, ur2, st2, P1["mbf"], o2):
        return V["reprojection2"], path, X
    dist1 = norm3([X[c] - P1["Ow"][c] for c in range(3)])
    dist2 = norm3([X[c] - P2["Ow"][c] for c in range(3)])
    if dist1 == 0 or dist2 == 0:
        return V["zero_distance"], path, X
    sf = W["prm"]["scale_factor"]
    ratio_dist, ratio_octave, rf = dist2 / dist1, f32(sf[o1]) / f32(sf[o2]), f32(W["ratio_factor"])
    if ratio_dist * rf < ratio_octave or ratio_dist > ratio_octave * rf:
        return V["scale_ratio"], path, X
    return V["created"], path, X


def usable_run(W, s, longest=None):
    """the run of a slot that is usable with state 1 and has a valid run (of at most `longest` entries), else None"""
    if not 0 <= s < W["S"] or W["state"][s] != 1:
        return None
    off, n = int(W["point_off"][s]), int(W["point_len"][s])
    if off < 0 or n < 0 or off + n > W["pool"] or (longest is not None and n > longest):
        return None
    return off, n


def side(W, off, n, free, first):
    """a keyframe's run as tests/test_triangulation_host.py's transcription takes it"""
    e = slice(off, off + n)
    node = np.array(W["node"][e], np.int64)
    if first:                                    # the contract: a KF1 keypoint with an octave out of range is in no node
        node[(W["octave"][e] < 0) | (W["octave"][e] >= W["prm"]["n_levels"])] = -1
    stereo = np.zeros(n, bool) if W["uright"] is None else W["uright"][e] >= 0
    return dict(node=node, free=free, stereo=stereo, x=W["x"][e], y=W["y"][e], angle=np.zeros(n, np.float32), desc=W["desc"][e], octave=W["octave"][e])


def restate(W, svd_log=None):
    """The sequential loop over W; returns the outputs (OUTPUTS) and everything the call writes (STATE)."""
    T, n1 = len(W["neighbours"]), W["n1"]
    res = {k: (None if W[k] is None else np.array(W[k])) for k in STATE}
    pool, reg = res["point_pool"], res["registered"]
    verdict = np.zeros((T, n1), np.int32)
    path = np.zeros((T, n1), np.uint8)
    x3D = np.zeros((T, n1, 3), np.float32)
    log = np.full((max(W["log_cap"], 0), 4), -1, np.int32)
    c = dict.fromkeys(COUNTS, 0)
    cur = usable_run(W, W["current_slot"])
    if cur is not None and cur[1] != n1:
        cur = None
    c["no_current"] = int(cur is None)
    P1 = pose_of(W, 0)
    prm = dict(W["prm"], check_orientation=0)
    pool0 = np.array(pool)
    owned = np.zeros(n1, bool)                   # the KF1 keypoints this call gave a point (or would have, had there been a row)
    written = set()                              # the KF2 entries this call wrote
    k = 0
    with np.errstate(all="ignore"):
        for t, s2 in enumerate(W["neighbours"]):
            run2 = None if cur is None or s2 == W["current_slot"] or s2 in W["neighbours"][:t] else usable_run(W, s2, W["run_capacity"])
            if run2 is None:
                verdict[t] = V["skipped_neighbour"]
                c["n_skipped_neighbours"] += 1
                continue
            (off1, _), (off2, n2) = cur, run2
            geom = dict(F12=W["F12"][t], ex=W["epipole"][t][0], ey=W["epipole"][t][1])
            KF2 = side(W, off2, n2, pool[off2:off2 + n2] == -1, False)
            # what the device computes: the matches over the pool as it is at the START of the call
            m0 = search_for_triangulation_reference(side(W, off1, n1, pool0[off1:off1 + n1] == -1, True),
                                                    side(W, off2, n2, pool0[off2:off2 + n2] == -1, False), geom, prm)[0]
            # what the reference computes: the matches of the keypoints that are free NOW (:686-690)
            m_now, _, pairs, _ = search_for_triangulation_reference(side(W, off1, n1, (pool[off1:off1 + n1] == -1) & ~owned, True), KF2, geom, prm)
            P2 = pose_of(W, 1 + t)
            c["n_matches"] += int((m0 >= 0).sum())
            for idx1 in range(n1):
                if m_now[idx1] < 0 and m0[idx1] >= 0:
                    assert owned[idx1] or pool[off1 + idx1] != -1, "a match was lost though the keypoint is still free"
                    verdict[t, idx1] = V["taken"]
                    c["n_taken"] += 1
                    # (the device judged this pair before it knew: its accepted count includes it where the gates pass)
                    v0 = pair_verdict(W, P1, P2, off1 + idx1, off2 + int(m0[idx1]))
                    c["n_accepted"] += v0[0] == V["created"]
                    c["n_svd"] += v0[1] == 1
                    c["n_unprojected"] += v0[1] >= 2
            for idx1, idx2 in pairs:             # :292, ascending idx1
                assert m0[idx1] == idx2, "the closed form fails: a free keypoint's match depends on the other keypoints"
                e1, e2 = off1 + idx1, off2 + idx2
                v, pth, X = pair_verdict(W, P1, P2, e1, e2, svd_log)
                path[t, idx1] = pth
                x3D[t, idx1] = X
                c["n_svd"] += pth == 1
                c["n_unprojected"] += pth >= 2
                if v != V["created"]:
                    verdict[t, idx1] = v
                    continue
                c["n_accepted"] += 1
                r = int(W["new_row"][k]) if k < len(W["new_row"]) else -1
                ok = 0 <= r < W["n_rows"]
                if k < W["log_cap"]:
                    log[k] = (r if ok else -1, idx1, t, idx2)
                k += 1
                owned[idx1] = True
                if not ok:
                    verdict[t, idx1] = V["no_row"]
                    c["n_no_row"] += 1
                    continue
                verdict[t, idx1] = V["created"]
                c["n_created"] += 1
                # new MapPoint(x3D, mpCurrentKeyFrame, mpMap) (MapPoint.cpp:37-49)
                for j in range(3):
                    res["floats"][j, r] = X[j]
                res["bad"][r] = 0
                for name, val in (("ref_slot", W["current_slot"]), ("replaced", -1), ("visible", 1), ("found", 1), ("first_kf_id", W["current_kf_id"])):
                    if res[name] is not None:
                        res[name][r] = val
                # AddObservation x 2, AddMapPoint x 2 (:442-446)
                pool[e1], reg[e1] = r, 1
                if e2 in written:
                    c["n_shared_kf2"] += 1       # pKF2->AddMapPoint overwrites: the earlier point loses the entry
                pool[e2], reg[e2] = r, 1
                written.add(e2)
                # ComputeDistinctiveDescriptors (:448): two observations, every median 0, the first in std::map order wins
                key1, key2 = (int(W["order_key"][W["current_slot"]]), W["current_slot"]), (int(W["order_key"][s2]), s2)
                obs = [(P1, e1), (P2, e2)] if key1 < key2 else [(P2, e2), (P1, e1)]
                res["tdesc"][r] = W["desc"][obs[0][1]]
                # UpdateNormalAndDepth (:450; MapPoint.cpp:385-406)
                normal = [f32(0)] * 3
                for P, _ in obs:
                    ni = [X[j] - P["Ow"][j] for j in range(3)]
                    d = f32(float(norm3(ni)))
                    normal = [normal[j] + ni[j] / d for j in range(3)]
                dist = norm3([X[j] - P1["Ow"][j] for j in range(3)])
                sf = W["prm"]["scale_factor"]
                max_d = dist * f32(sf[int(W["octave"][e1])])
                min_d = max_d / f32(sf[W["prm"]["n_levels"] - 1])
                for j in range(3):
                    res["floats"][3 + j, r] = normal[j] / f32(2)
                res["floats"][6, r] = max_d
                res["floats"][7, r] = f32(1.2) * max_d
                res["floats"][8, r] = f32(0.8) * min_d
    c["n_owning"] = k
    c["log_overflow"] = int(k > W["log_cap"])
    x3D[(verdict == V["taken"])] = 0
    res.update(verdict=verdict, path=path, x3D=x3D, log=log, counts=np.array([c[n] for n in COUNTS], np.int32))
    return res


def same(want, got, what):
    """bit equality of every output and every array the call writes"""
    for k in OUTPUTS + STATE:
        a, b = want[k], got[k]
        if a is None:
            assert b is None, (what, k)
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError("%s: %s differs at %d places, first %s: want %s got %s" % (what, k, len(bad), bad[0], want[k][tuple(bad[0])], got[k][tuple(bad[0])]))


# ---- worlds ----
CAM = dict(fx=500.0, fy=480.0, cx=320.0, cy=240.0)
MB = 0.1


def small_rotation(rng, sigma):
    w = rng.normal(0, sigma, 3)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    Kx = skew(w / th)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose_record(R, t, mb=MB, mbf=None, Ow=None):
    """a pose as jetson_slam_amd.orb.make_keyframe_pose builds it, without importing the package"""
    R32, t32 = np.asarray(R, np.float32).reshape(3, 3), np.asarray(t, np.float32).reshape(3)
    if Ow is None:
        Ow = np.array([-((R32[0, i] * t32[0] + R32[1, i] * t32[1]) + R32[2, i] * t32[2]) for i in range(3)], np.float32)
    fx, fy = f32(CAM["fx"]), f32(CAM["fy"])
    d = dict(Rcw=R32.ravel(), tcw=t32, Ow=np.asarray(Ow, np.float32), fx=fx, fy=fy, cx=f32(CAM["cx"]), cy=f32(CAM["cy"]), invfx=f32(1) / fx, invfy=f32(1) / fy,
             mb=f32(mb), mbf=f32(mb * CAM["fx"] if mbf is None else mbf))
    return d


def f12_epipole(P1, P2):
    """LocalMapping::ComputeF12 and the epipole of ORBmatcher.cpp:651-657 from two poses, computed in double and handed over as float32 inputs"""
    R1, t1 = P1["Rcw"].reshape(3, 3).astype(np.float64), P1["tcw"].astype(np.float64)
    R2, t2 = P2["Rcw"].reshape(3, 3).astype(np.float64), P2["tcw"].astype(np.float64)
    K = np.array([[CAM["fx"], 0, CAM["cx"]], [0, CAM["fy"], CAM["cy"]], [0, 0, 1]])
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    F = np.linalg.inv(K).T @ skew(t12) @ R12 @ np.linalg.inv(K)
    C2 = R2 @ (-R1.T @ t1) + t2
    with np.errstate(all="ignore"):
        ep = np.array([CAM["fx"] * C2[0] / C2[2] + CAM["cx"], CAM["fy"] * C2[1] / C2[2] + CAM["cy"]])
    return F.astype(np.float32).reshape(9), np.nan_to_num(ep, nan=1e9, posinf=1e9, neginf=-1e9).astype(np.float32)


def cos_of_stereo(mb, depth):
    """cos(2 * atan2(mb / 2, depth)) as LocalMapping.cpp:318 computes it once: float arguments, the value rounded to float"""
    with np.errstate(all="ignore"):
        return np.cos(f32(2) * np.arctan2(f32(mb) / f32(2), np.asarray(depth, np.float32))).astype(np.float32)


def finish_world(W, n_rows, rng, stereo=True, raw=True, side_arrays=True, new_row=None, log_cap=None):
    """the table, the free rows and the side arrays of a world whose graph and keypoints are set"""
    n_levels = 8
    sf, s2 = scale_tables(n_levels)
    W.setdefault("prm", dict(th_low=50, check_orientation=0, only_stereo=0, n_levels=n_levels, scale_factor=sf, level_sigma2=s2))
    W["n_rows"] = n_rows
    W["floats"] = rng.normal(0, 3, (9, max(n_rows, 1))).astype(np.float32)[:, :n_rows]
    W["tdesc"] = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    W.setdefault("bad", np.zeros(n_rows, np.uint8))
    for k, lo, hi in (("ref_slot", 0, W["S"]), ("replaced", -1, 0), ("visible", 1, 50), ("found", 1, 50), ("first_kf_id", 0, 1000)):
        W[k] = rng.integers(lo, hi, n_rows).astype(np.int32) if side_arrays else None
    if not stereo:
        W["uright"] = W["depth"] = W["cos_stereo"] = None
    if not raw:
        W["raw_x"] = W["raw_y"] = None
    used = set(int(r) for r in W["point_pool"] if r >= 0)
    free_rows = np.array([r for r in range(n_rows) if r not in used], np.int32)
    W["new_row"] = rng.permutation(free_rows).astype(np.int32) if new_row is None else np.asarray(new_row, np.int32)
    W["log_cap"] = len(W["new_row"]) if log_cap is None else log_cap
    W.setdefault("ratio_factor", f32(1.5) * f32(1.2))
    W.setdefault("current_kf_id", 77)
    W["run_capacity"] = W.get("run_capacity", int(max(W["point_len"])) if len(W["point_len"]) else 0)
    return W


def scene(seed, n1=65, n_nb=5, n_kp2=80, stereo=0.5, raw=True, side_arrays=True, duplicates=0, n_nodes=6, baselines=None, old=0.25, depth_nonpositive=0.0,
          name=None, narrow=(0.01, 0.02), narrow_axis=(1, 0.3, 0.2), **kw):
    """A seeded world: points in front of a current keyframe of n1 keypoints and n_nb neighbours of about n_kp2 keypoints, wide and narrow baselines
    in turn (narrow: two mono keypoints have too little parallax, a stereo one is unprojected), a share of points that already have a row."""
    rng = np.random.default_rng(seed)
    S = n_nb + 3
    slots = rng.permutation(S)                   # the slots of the current keyframe, the neighbours, two unrelated keyframes
    n_pts = max(n1, n_kp2) + 20
    ang = rng.uniform(-0.4, 0.4, (n_pts, 2))
    depth = rng.uniform(3.0, 8.0, n_pts)
    Xw = np.stack([np.tan(ang[:, 0]) * depth, np.tan(ang[:, 1]) * depth * 0.7, depth], 1)
    pt_desc = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    pt_oct = rng.integers(0, 3, n_pts)
    pt_row = np.where(rng.random(n_pts) < old, np.arange(n_pts), -1)     # an old point's row is its number
    poses = []
    for i in range(1 + n_nb):
        wide = i == 0 or (baselines[i - 1] if baselines is not None else i % 2 == 1)
        R = small_rotation(rng, 0.03)
        c = np.zeros(3) if i == 0 else rng.normal(0, 1, 3) * np.array([1, 0.3, 0.2] if wide else narrow_axis)
        if i:
            c = c / np.linalg.norm(c) * (rng.uniform(0.4, 0.7) if wide else rng.uniform(*narrow))
        poses.append(pose_record(R, -R @ c, mb=MB))
    arrays = {k: [] for k in ("x", "y", "octave", "uright", "desc", "node", "depth", "raw_x", "raw_y", "point_pool")}
    point_off, point_len = np.zeros(S, np.int32), np.zeros(S, np.int32)
    at = 0
    for i in range(1 + n_nb + 2):
        want = n1 if i == 0 else int(n_kp2 * rng.uniform(0.7, 1.0)) if i <= n_nb else 10
        ids = rng.permutation(n_pts)[:max(want - (duplicates if i == 0 else 0), 0)]
        if i == 0 and duplicates and len(ids):
            ids = np.concatenate([ids, ids[:duplicates]])[:want]         # a point seen twice in KF1: two keypoints that take the same KF2 keypoint
        P = poses[min(i, n_nb)]
        R, t = P["Rcw"].reshape(3, 3).astype(np.float64), P["tcw"].astype(np.float64)
        Xc = Xw[ids] @ R.T + t
        z = Xc[:, 2]
        u = CAM["fx"] * Xc[:, 0] / z + CAM["cx"] + rng.normal(0, 0.25, len(ids))
        v = CAM["fy"] * Xc[:, 1] / z + CAM["cy"] + rng.normal(0, 0.25, len(ids))
        is_st = rng.random(len(ids)) < stereo
        d = np.where(is_st, z + rng.normal(0, 0.01, len(ids)), -1.0)
        d = np.where(is_st & (rng.random(len(ids)) < depth_nonpositive), 0.0, d)          # mvDepth <= 0 with mvuRight >= 0
        ur = np.where(is_st, u - MB * CAM["fx"] / z, -1.0)
        desc = pt_desc[ids].copy()
        for j in range(len(ids)):
            for b in rng.integers(0, 256, 4):
                desc[j, b // 8] ^= 1 << (b % 8)
        node = np.where(rng.random(len(ids)) < 0.95, ids % n_nodes, -1)
        pp = pt_row[ids].copy()
        point_off[slots[i]], point_len[slots[i]] = at, len(ids)
        at += len(ids)
        for k, a in (("x", u), ("y", v), ("octave", pt_oct[ids] + rng.integers(0, 2, len(ids))), ("uright", ur), ("desc", desc), ("node", node),
                     ("depth", d), ("raw_x", u + 0.5), ("raw_y", v - 0.25), ("point_pool", pp)):
            arrays[k].append(a)
    W = dict(name=name or "scene%d" % seed, S=S, pool=at + 7, current_slot=int(slots[0]), neighbours=[int(s) for s in slots[1:1 + n_nb]], n1=n1,
             state=np.ones(S, np.uint8), order_key=rng.integers(0, 4, S).astype(np.int64) * 1000, point_off=point_off, point_len=point_len)
    pad = {"point_pool": -1, "uright": -1.0, "node": -1}
    for k, dt in (("x", np.float32), ("y", np.float32), ("octave", np.int32), ("uright", np.float32), ("node", np.int32), ("depth", np.float32),
                  ("raw_x", np.float32), ("raw_y", np.float32), ("point_pool", np.int32)):
        W[k] = np.concatenate(arrays[k] + [np.full(7, pad.get(k, 0))]).astype(dt)
    W["desc"] = np.concatenate(arrays["desc"] + [np.zeros((7, 32), np.uint8)])
    W["registered"] = (W["point_pool"] >= 0).astype(np.uint8)
    W["cos_stereo"] = cos_of_stereo(MB, W["depth"])
    W["poses"] = poses
    fe = [f12_epipole(poses[0], poses[1 + t]) for t in range(n_nb)]
    W["F12"] = np.array([f for f, _ in fe], np.float32).reshape(n_nb, 9)
    W["epipole"] = np.array([e for _, e in fe], np.float32).reshape(n_nb, 2)
    n_rows = n_pts + n1 * 2 + 5
    W["bad"] = (np.random.default_rng(seed + 1).random(n_rows) < 0.05).astype(np.uint8)
    return finish_world(W, n_rows, rng, stereo=stereo > 0, raw=raw, side_arrays=side_arrays, **kw)


def unit(kind):
    """A world of two keyframes with one keypoint each, built by hand so that the pair leaves at ONE named exit.  F12 and the epipole follow from the
    poses, except in the two degenerate worlds (w_zero, zero_distance), where F12 is the sideways-baseline matrix (x1^T F12 x2 = y2 - y1) whatever the
    poses say - an input like any other - so that the matcher accepts the pair and the exit is the triangulation's."""
    rng = np.random.default_rng(sum(map(ord, kind)))
    I = np.eye(3)
    kp1 = dict(x=CAM["cx"], y=CAM["cy"], octave=0, uright=-1.0, depth=-1.0, cos=1.0)
    kp2 = dict(kp1)
    P1, P2 = pose_record(I, [0, 0, 0]), pose_record(I, [-0.5, 0, 0])
    Xw = None

    def project(P, X):
        R, t = P["Rcw"].reshape(3, 3).astype(np.float64), P["tcw"].astype(np.float64)
        Xc = R @ np.asarray(X, np.float64) + t
        return CAM["fx"] * Xc[0] / Xc[2] + CAM["cx"], CAM["fy"] * Xc[1] / Xc[2] + CAM["cy"], Xc[2]

    if kind == "w_zero":
        # both keypoints at the principal point of parallel cameras: the rays are parallel, the null vector is a point at infinity and column 2 of A is
        # exactly zero.  cosRays is exactly 1, which :325 lets through only against a cos_stereo above 1 - no true cosine, but a device input
        kp1.update(uright=300.0, depth=5.0, cos=2.0)
    elif kind == "z1":
        Xw = [0.3, 0.2, -3.0]                    # behind both cameras: the lines meet there
    elif kind == "z2":
        Xw, P2 = [0.3, 0.2, 3.0], pose_record(I, [-0.1, 0, -5.0])      # the neighbour stands beyond the point
    elif kind in ("created", "scale_ratio", "reprojection1", "reprojection2"):
        Xw = [0.3, 0.2, 4.0]
    elif kind == "empty_unprojection":
        P2 = pose_record(I, [-0.01, 0, 0])
        Xw = [0.3, 0.2, 4.0]
    elif kind == "zero_distance":
        # UnprojectStereo of KF1 at a depth of 1e-23 from a camera at the origin: z1 > 0, the reprojections are exact, and |x3D - Ow1|^2 underflows
        P1, P2 = pose_record(I, [0, 0, 0], mb=0.0, mbf=0.0), pose_record(I, [0, 0, 1.0], mb=0.0, mbf=0.0)
        kp1.update(uright=CAM["cx"], depth=1e-23, cos=0.5)
    if Xw is not None:
        for kp, P in ((kp1, P1), (kp2, P2)):
            kp["x"], kp["y"], kp["z"] = project(P, Xw)
    if kind == "scale_ratio":
        kp2["octave"] = 7
    if kind == "reprojection1":                  # a right-image coordinate that contradicts the triangulated depth
        kp1.update(uright=kp1["x"] - 30.0, depth=kp1["z"], cos=float(cos_of_stereo(MB, kp1["z"])))
    if kind == "reprojection2":
        kp2.update(uright=kp2["x"] - 30.0, depth=kp2["z"], cos=float(cos_of_stereo(MB, kp2["z"])))
    if kind == "empty_unprojection":             # mvuRight >= 0 with mvDepth <= 0, and too little parallax for the linear method
        kp1.update(uright=kp1["x"] - 10.0, depth=0.0, cos=0.9)
    kps = [kp1, kp2]
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    W = dict(name=kind, S=2, pool=2, current_slot=0, neighbours=[1], n1=1, state=np.ones(2, np.uint8), order_key=np.array([5, 3], np.int64),
             point_off=np.array([0, 1], np.int32), point_len=np.array([1, 1], np.int32), point_pool=np.full(2, -1, np.int32),
             registered=np.zeros(2, np.uint8), node=np.zeros(2, np.int32), desc=np.stack([d, d]), poses=[P1, P2],
             F12=np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0]], np.float32), epipole=np.array([[1e9, CAM["cy"]]], np.float32))
    if Xw is not None:
        F, ep = f12_epipole(P1, P2)
        W["F12"], W["epipole"] = F.reshape(1, 9), ep.reshape(1, 2)
    for k, src in (("x", "x"), ("y", "y"), ("uright", "uright"), ("depth", "depth"), ("cos_stereo", "cos")):
        W[k] = np.array([kp[src] for kp in kps], np.float32)
    W["raw_x"], W["raw_y"] = W["x"].copy(), W["y"].copy()
    W["octave"] = np.array([kp["octave"] for kp in kps], np.int32)
    return finish_world(W, 3, rng)


UNITS = ("created", "w_zero", "z1", "z2", "reprojection1", "reprojection2", "zero_distance", "scale_ratio", "empty_unprojection")


def edited(W, name, **changes):
    """a copy of W with some entries replaced (arrays are copied)"""
    W2 = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in W.items()}
    W2.update(changes)
    W2["name"] = name
    return W2


_CASES = {}


def named():
    """{name: world}: the cases the issue lists, made once"""
    if _CASES:
        return _CASES
    C = {}
    for k in UNITS:
        C["unit_" + k] = unit(k)
    C["mixed"] = scene(11, name="mixed", depth_nonpositive=0.1)
    C["neighbour_mbf"] = edited(C["mixed"], "neighbour_mbf", poses=[C["mixed"]["poses"][0]] + [dict(p, mbf=f32(p["mbf"] * 4), mb=f32(p["mb"] * 4))
                                                                                              for p in C["mixed"]["poses"][1:]])
    C["mono"] = scene(12, name="mono", stereo=0.0, side_arrays=False, n_nb=4)
    C["no_raw"] = scene(13, name="no_raw", raw=False, n_nb=3, n1=64)
    C["shared_kf2"] = scene(14, name="shared_kf2", duplicates=12, n_nb=3, old=0.0)
    C["twenty"] = scene(15, name="twenty", n_nb=20, n1=63, n_kp2=40)
    for n1 in (0, 1):
        C["n1_%d" % n1] = scene(16 + n1, name="n1_%d" % n1, n1=n1, n_nb=3)
    C["no_neighbours"] = scene(18, name="no_neighbours", n_nb=0)
    base = scene(19, name="base", n_nb=4, old=0.1)
    C["base"] = base
    full = restate(base)
    made = int(full["counts"][COUNTS.index("n_owning")])
    assert made >= 8
    C["rows_one_short"] = edited(base, "rows_one_short", new_row=base["new_row"][:made - 1])
    rows = base["new_row"][:made].copy()
    rows[2], rows[5] = -3, base["n_rows"]
    C["rows_out_of_range"] = edited(base, "rows_out_of_range", new_row=rows)
    C["log_cap_0"] = edited(base, "log_cap_0", log_cap=0)
    C["log_one_short"] = edited(base, "log_one_short", log_cap=made - 1)
    st = base["state"].copy()
    st[base["neighbours"][1]] = 2
    C["bad_neighbour_in_the_middle"] = edited(base, "bad_neighbour_in_the_middle", state=st)
    nb = list(base["neighbours"])
    C["odd_neighbours"] = edited(base, "odd_neighbours", neighbours=[nb[0], -1, base["current_slot"], nb[1], base["S"], nb[2]],
                                 poses=[base["poses"][i] for i in (0, 1, 2, 2, 2, 2, 3)], F12=base["F12"][[0, 1, 1, 1, 1, 2]],
                                 epipole=base["epipole"][[0, 1, 1, 1, 1, 2]])
    C["repeated_neighbour"] = edited(base, "repeated_neighbour", neighbours=[nb[0], nb[1], nb[0], nb[2]], poses=[base["poses"][i] for i in (0, 1, 2, 1, 3)],
                                     F12=base["F12"][[0, 1, 0, 2]], epipole=base["epipole"][[0, 1, 0, 2]])
    C["run_longer_than_capacity"] = edited(base, "run_longer_than_capacity", run_capacity=int(sorted(base["point_len"][nb])[1]))
    st = base["state"].copy()
    st[base["current_slot"]] = 2
    C["bad_current"] = edited(base, "bad_current", state=st)
    C["wrong_n1"] = edited(base, "wrong_n1", n1=base["n1"] - 1)
    pp = base["point_pool"].copy()
    o = int(base["point_off"][base["current_slot"]])
    pp[o], pp[o + 1] = -5, base["n_rows"] + 9    # values outside [-1, n_rows): not free, nothing read through them
    oc = base["octave"].copy()
    oc[o + 2], oc[o + 3] = -1, 8                 # KF1 octaves out of range: no match
    C["odd_pool_values"] = edited(base, "odd_pool_values", point_pool=pp, octave=oc)
    _CASES.update(C)
    return _CASES


_RESTATED = {}


def restated(name):
    if name not in _RESTATED:
        _RESTATED[name] = restate(named()[name])
    return _RESTATED[name]


# ---- the second yardstick: the reference's own LocalMapping.cpp, KeyFrame.cpp and MapPoint.cpp (tools/ref_newpoints) ----
# The reference's loop has its own baseline test (:255-259, baseline >= mb for a stereo map), no skipped neighbours, always a free row, and it
# reads through an empty UnprojectStereo result: the recorded worlds keep inside that - every baseline is at least mb, no mvDepth <= 0 with
# mvuRight >= 0 - and are otherwise the generator's.  Their cos_stereo is what the driver's libm gave (recorded with the result).
REF_SEEDS = (31, 32, 33, 34, 35, 36)
STAND_INS = ("Frame.h", "Map.h", "KeyFrameDatabase.h", "Converter.h", "ORBmatcher.h", "ORBextractor.h", "ORBVocabulary.h", "Optimizer.h", "LoopClosing.h",
             "Tracking.h")
RECORD_WORDS = 25


def _root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_path():
    import os
    return os.path.join(_root(), "tests", "golden", "ref_matcher_newpoints.npz")


def ref_scene(seed):
    """a world the reference's loop can run: baselines between 1.05 and 6 times mb = 0.2, partly along the axis (little parallax), up to 10 neighbours"""
    global MB
    rng = np.random.default_rng(seed)
    keep = MB
    MB = 0.2
    try:
        W = scene(seed, n1=int(rng.integers(40, 90)), n_nb=int(rng.integers(2, 7)), n_kp2=60, stereo=float(rng.choice([0.0, 0.5, 0.8])), duplicates=int(rng.integers(0, 6)),
                  name="ref_seed_%d" % seed, narrow=(0.21, 0.26), narrow_axis=(0.1, 0.05, 1), raw=bool(seed % 2))
    finally:
        MB = keep
    return W


def golden_worlds(recorded=None):
    """{name: world}; with the recording, cos_stereo is the driver's"""
    out = {}
    for seed in REF_SEEDS:
        W = ref_scene(seed)
        if recorded is not None and W["cos_stereo"] is not None:
            W["cos_stereo"] = unpack(W, recorded[W["name"]]["raw"])["cos_stereo"]
        out[W["name"]] = W
    return out


def start_matches(W):
    """the candidates the stubbed matcher draws from: every neighbour's matches over the map as it is before the loop (tests/test_triangulation_host.py's
    transcription of ORBmatcher::SearchForTriangulation)"""
    off1, n1 = int(W["point_off"][W["current_slot"]]), W["n1"]
    prm = dict(W["prm"], check_orientation=0)
    rows = []
    for t, s2 in enumerate(W["neighbours"]):
        off2, n2 = int(W["point_off"][s2]), int(W["point_len"][s2])
        geom = dict(F12=W["F12"][t], ex=W["epipole"][t][0], ey=W["epipole"][t][1])
        rows.append(search_for_triangulation_reference(side(W, off1, n1, W["point_pool"][off1:off1 + n1] == -1, True),
                                                       side(W, off2, n2, W["point_pool"][off2:off2 + n2] == -1, False), geom, prm)[0])
    return np.array(rows, np.int32).reshape(len(W["neighbours"]), n1)


def world_bytes(W):
    """the driver's input (tools/ref_newpoints/driver.cpp)"""
    T, z = len(W["neighbours"]), np.zeros(W["pool"], np.float32)
    f = lambda k: z if W[k] is None else np.asarray(W[k], np.float32)
    pose_slot = np.full(W["S"], -1, np.int32)
    pose_slot[W["current_slot"]] = 0
    for t, s in enumerate(W["neighbours"]):
        pose_slot[s] = 1 + t
    poses = np.array([np.concatenate([p["Rcw"], p["tcw"], [p["fx"], p["fy"], p["cx"], p["cy"], p["mb"], p["mbf"]]]) for p in W["poses"]], np.float32)
    parts = [np.array([W["S"], W["n_rows"], W["pool"], W["current_slot"], W["n1"], T, W["prm"]["n_levels"], W["current_kf_id"]], np.int32),
             W["state"].astype(np.int32), W["order_key"].astype(np.int64), W["point_off"].astype(np.int32), W["point_len"].astype(np.int32),
             W["point_pool"].astype(np.int32), W["octave"].astype(np.int32), f("x"), f("y"), np.full(W["pool"], -1, np.float32) if W["uright"] is None else f("uright"),
             f("depth"), f("x") if W["raw_x"] is None else f("raw_x"), f("y") if W["raw_y"] is None else f("raw_y"), W["desc"].astype(np.uint8),
             W["bad"].astype(np.int32), np.asarray(W["neighbours"], np.int32), pose_slot, poses, np.asarray(W["prm"]["scale_factor"], np.float32),
             np.asarray(W["prm"]["level_sigma2"], np.float32), np.array([1.2], np.float32), start_matches(W)]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts)


def reference_tree():
    import os
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if all(os.path.exists(os.path.join(ref, "src", f)) for f in ("LocalMapping.cpp", "KeyFrame.cpp", "MapPoint.cpp")) else None


def driver_path():
    import os
    return os.path.join(_root(), "oracle", "_ref", "ref_newpoints")


def build_driver(reference):
    """the reference's src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp, unmodified, against tools/ref_newpoints' opencv2/core/core.hpp and
    tools/ref_culling's stand-in headers, force-included so that their guards shut out the reference's headers of the same names"""
    import os
    import subprocess
    here, shadow = os.path.join(_root(), "tools", "ref_newpoints"), os.path.join(_root(), "tools", "ref_culling")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-w", "-ffp-contract=off", "-I" + here, "-I" + shadow, "-I" + os.path.join(reference, "include"),
           "-I" + reference]
    for h in STAND_INS:
        cmd += ["-include", os.path.join(shadow, h)]
    dbow = os.path.join(reference, "Thirdparty", "DBoW2", "DBoW2")
    cmd += ["-o", driver_path(), os.path.join(here, "driver.cpp")] + [os.path.join(reference, "src", f) for f in ("LocalMapping.cpp", "KeyFrame.cpp", "MapPoint.cpp")]
    cmd += [os.path.join(dbow, "BowVector.cpp"), os.path.join(dbow, "FeatureVector.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    return driver_path()


def run_driver(W, workdir):
    """a world through the reference -> dict of `raw` (the driver's int32 output) and `crc` of its input"""
    import os
    import subprocess
    import zlib
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    raw_in = world_bytes(W)
    with open(src, "wb") as f:
        f.write(raw_in)
    subprocess.check_call([driver_path(), src, dst], timeout=120)
    return dict(raw=np.fromfile(dst, np.int32), crc=np.array(zlib.crc32(raw_in), np.uint32))


def unpack(W, raw):
    """the driver's output: per created point (idx1, neighbour, idx2, first_kf_id, ref_slot, visible, found, nine floats, eight descriptor words,
    bad), then point_pool (a new point as n_rows + its creation number), registered, cos_stereo"""
    n, pool = int(raw[0]), W["pool"]
    assert len(raw) == 1 + RECORD_WORDS * n + 3 * pool
    rec = raw[1:1 + RECORD_WORDS * n].reshape(n, RECORD_WORDS)
    rest = raw[1 + RECORD_WORDS * n:]
    return dict(ints=rec[:, :7], floats=rec[:, 7:16].copy().view(np.float32), desc=rec[:, 16:24].copy().view(np.uint8).reshape(n, 32), bad=rec[:, 24],
                point_pool=rest[:pool], registered=rest[pool:2 * pool], cos_stereo=rest[2 * pool:].copy().view(np.float32))


def same_as_recorded(W, res, raw, what=""):
    """a yardstick's (or the device's) result against the reference's recording: the points created, in order, with every field the reference holds of
    them - position, normal, distance range, descriptor, flags and counters - and every keyframe's map points.  (The verdicts of the pairs that create
    nothing, and x3D of those, are not observable in the reference's run.)"""
    R = unpack(W, raw)
    log = res["log"][res["log"][:, 1] >= 0]
    assert (log[:, 0] >= 0).all() and len(log) == len(R["ints"]) == int(res["counts"][COUNTS.index("n_created")]), (what, len(log), len(R["ints"]))
    rows = log[:, 0]
    assert np.array_equal(log[:, 1:], R["ints"][:, :3]), (what, "the pairs that create a point, in order")
    assert np.array_equal(res["floats"][:, rows].T.view(np.uint32), R["floats"].view(np.uint32)), (what, "P, Pn, MaxDistance, the invariances")
    assert np.array_equal(res["tdesc"][rows], R["desc"]) and np.array_equal(res["bad"][rows], R["bad"].astype(np.uint8)), (what, "desc, bad")
    t = np.arange(len(rows))
    assert np.array_equal(res["x3D"][log[:, 2], log[:, 1]].view(np.uint32), R["floats"][:, :3].view(np.uint32)), (what, "x3D")
    for i, k in enumerate(("first_kf_id", "ref_slot", "visible", "found")):
        if res[k] is not None:
            assert np.array_equal(res[k][rows], R["ints"][:, 3 + i]), (what, k)
    want_pool = R["point_pool"].copy()
    new = want_pool >= W["n_rows"]
    want_pool[new] = rows[want_pool[new] - W["n_rows"]]
    assert np.array_equal(res["point_pool"], want_pool), (what, "point_pool")
    assert (res["registered"][new] == 1).all() and (R["registered"][new] == 1).all(), (what, "registered")
    return len(t)


def write_golden(recorded):
    """recorded: name -> dict(raw, crc); members in a fixed order with a fixed date, so that the file is reproducible"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w") as z:
        for name, rec in recorded.items():
            for k in ("raw", "crc"):
                buf = io.BytesIO()
                np.save(buf, rec[k])
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, k), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


def load_golden():
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, k = member.rsplit(".", 1)
            out.setdefault(name, {})[k] = z[member]
    return out
