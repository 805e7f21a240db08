"""CPU: the yardstick of jsorb_pose_optimization (tests/pose_optimization_cases.py, a transcription of Optimizer::PoseOptimization and the g2o chain
under it) held to things that are not the transcription - central differences, the generating pose, scipy's optimum - and the conditions on its
worlds (classification margins, the exits the named worlds claim, the permutation spread that sets the device tolerance).  The figures asserted
here are ten times what DESIGN.md section 32 records, measured against scipy's optimum and the generating pose, never against the device."""
import os
import re

import numpy as np
import pytest

import pose_optimization_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64

# recorded: the largest differences seen, as (max |dR|, |dt|_inf / (1 + |t|_inf))
CLEAN_RECORDED = (4.6e-9, 4.4e-8)          # (b) the final pose against the generating pose, noise-free worlds (the table is float32)
SCIPY_RECORDED = (1.7e-10, 1.6e-9)       # (c) the final pose against scipy's optimum over the edges round 3 optimised


def true_pose(W):
    T = W["T_true"]
    return np.concatenate([T[:3, :3].ravel(), T[:3, 3]])


# ---- (a) the analytic Jacobians against central differences of the transcription's own error function under exp(d) . T ----
def jacobian_gap(W, sel, h):
    """the largest |numeric - analytic| / (1 + |analytic|) over the selected edges: g2o's _jacobianOplusXi is d(error) / d(delta)"""
    E, cam = pc.edges_of(W), pc.camera_of(W)
    T = pc.to_se3quat(W["Tcw"])
    J = pc.edge_jacobian(cam, pc.edge_error(T, cam, E, sel)[2], E["stereo"][sel])
    worst = 0.0
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        num = (pc.edge_error(pc.oplus(d, T)[0], cam, E, sel)[0] - pc.edge_error(pc.oplus(-d, T)[0], cam, E, sel)[0]) / (2 * h)
        worst = max(worst, float(np.max(np.abs(num - J[:, i, :]) / (1.0 + np.abs(J[:, i, :])))))
    return worst


@pytest.mark.parametrize("name", ["mixed", "far_start"])
def test_jacobians_against_central_differences(name):
    W = pc.world(name)
    stereo = pc.edges_of(W)["stereo"]
    assert stereo.sum() > 20 and (~stereo).sum() > 20
    mono_gap = jacobian_gap(W, ~stereo, 1e-6)
    # the stereo edge's float invz (types_six_dof_expmap.cpp:300) quantises a projection of up to `width` pixels to 2^-24 of its size: each of
    # the two samples is off by up to half of that, so the quotient over 2h by up to width 2^-24 / (2h); the bound is twice that.  A wrong
    # entry would be off by the entry itself, a gap of ~1
    h = 1e-3
    stereo_gap = jacobian_gap(W, stereo, h)
    print("%s: mono %.3g stereo %.3g" % (name, mono_gap, stereo_gap))
    assert mono_gap < 1e-6 and stereo_gap < pc.frame("main")["c"]["w"] * 2.0 ** -24 / h, (mono_gap, stereo_gap)


# ---- (b) noise-free, outlier-free worlds give the generating pose back ----
@pytest.mark.parametrize("name", list(pc.CLEAN))
def test_clean_worlds_return_the_generating_pose(name):
    W, r = pc.world(name), pc.expected(name)
    assert r["counts"].tolist() == [len(W["kps"]), 0, len(W["kps"]), 4] and not r["outlier"].any()
    dR, dt = pc.pose_difference(r["pose"], true_pose(W))
    print("%s: dR %.3g dt %.3g" % (name, dR, dt))
    assert dR <= 10 * CLEAN_RECORDED[0] and dt <= 10 * CLEAN_RECORDED[1], (dR, dt)


# ---- (c) the final pose against scipy.optimize.least_squares over the inlier set round 3 left, without a kernel ----
def scipy_optimum(W, r):
    from scipy.optimize import least_squares
    E, cam = r["E"], pc.camera_of(W)
    active = ~r["diag"]["sets"][2]                         # the edges round 3 optimised over: not flagged by round 2
    q = pc.normalized(pc.quat_of(r["pose"][:9].reshape(3, 3)))
    T = (q, r["pose"][9:].copy())

    info = np.sqrt(E["info"][active])

    # the analytic Jacobian at the moved pose (exact at d = 0; the pose is re-centred three times, so d ends at rounding size): finite
    # differences of a few 1e-8 would only see the quantisation of the stereo edge's float invz
    def residuals(d, T):
        return (pc.edge_error(pc.oplus(d, T)[0], cam, E, active)[0] * info).ravel()

    def jacobian(d, T):
        J = pc.edge_jacobian(cam, pc.edge_error(pc.oplus(d, T)[0], cam, E, active)[2], E["stereo"][active])
        return (J * info[None, None, :]).transpose(0, 2, 1).reshape(-1, 6)

    for _ in range(3):
        s = least_squares(residuals, np.zeros(6), jac=jacobian, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, args=(T,))
        T = pc.oplus(s.x, T)[0]
    return np.concatenate([pc.matrix_of(T[0]).ravel(), T[1]])


@pytest.mark.parametrize("name", ["all_mono", "all_stereo", "mixed", "e1000", "readmit", "far_start", "seed103"])
def test_final_pose_against_scipy(name):
    W, r = pc.world(name), pc.expected(name)
    assert r["counts"][3] == 4
    dR, dt = pc.pose_difference(r["pose"], scipy_optimum(W, r))
    print("%s: dR %.3g dt %.3g" % (name, dR, dt))
    assert dR <= 10 * SCIPY_RECORDED[0] and dt <= 10 * SCIPY_RECORDED[1], (dR, dt)


# ---- (d) the permutation spread per world: eight seeded permutations of the edge order; it sets the device tolerance ----
def test_permutation_spread():
    worst = 0.0
    for name in pc.WORLDS:
        r = pc.expected(name)
        nE = int(r["counts"][0])
        if nE < 3:
            continue
        rng = np.random.default_rng(7)
        for _ in range(8):
            q = pc.reference(pc.world(name), order=rng.permutation(nE))
            assert np.array_equal(q["outlier"], r["outlier"]) and np.array_equal(q["counts"], r["counts"]) and np.array_equal(q["row_out"], r["row_out"]), name
            worst = max(worst, *pc.pose_difference(q["pose"], r["pose"]))
    print("largest pose spread under permutation: %.3g" % worst)
    assert worst <= pc.PERMUTATION_SPREAD, worst
    assert pc.DEVICE_FACTOR == 64


# ---- the conditions on the worlds: margins, shapes, and the exit each named world claims ----
@pytest.mark.parametrize("name", pc.WORLDS + list(pc.CLEAN))
def test_world_conditions(name):
    W, r = pc.world(name), pc.expected(name)
    d = r["diag"]
    assert r["class_margin"] >= pc.MARGIN, r["class_margin"]          # a seed that fails is replaced in the list
    assert W["N"] <= 2500 and r["counts"][0] <= 1100
    claim = pc.NAMED[name][1] if name in pc.NAMED else "four_rounds"
    if claim == "no_keypoint":
        assert W["N"] == 0 and r["counts"].tolist() == [0, 0, 0, 0]
    elif claim == "untouched":
        assert r["counts"].tolist() == [2, 0, 0, 0] and np.array_equal(r["Tcw_out"].view(np.uint32), W["Tcw"].ravel().view(np.uint32))
    elif claim == "one_round":
        assert 3 <= r["counts"][0] < 10 and r["counts"][3] == 1
    else:
        assert r["counts"][0] >= 10 and r["counts"][3] == 4
    if claim == "outside_rows":
        assert d["n_outside_rows"] >= 10 and (W["rows"] < -1).sum() >= 5
    if claim == "bad_rows":
        assert W["bad"][W["rows"][W["kps"]]].all() and r["counts"][0] == len(W["kps"])
    if claim == "idle_round":
        assert d["idle_rounds"] >= 1 and r["counts"][1] == r["counts"][0]
    if claim == "readmitted":
        assert d["readmitted"] >= 1 and any(not np.array_equal(d["sets"][i], d["sets"][i + 1]) for i in range(3))
    if claim == "rejected_trials":
        assert d["rejected"] >= 5
    if claim == "small_theta":
        assert d["small_theta"] >= 1
    if name in ("all_mono",):
        assert d["n_stereo"] == 0
    if name in ("all_stereo",):
        assert d["n_mono"] == 0
    if name == "mixed":
        assert d["n_mono"] > 20 and d["n_stereo"] > 20
    assert int(r["counts"][0]) == d["n_mono"] + d["n_stereo"]


def test_edge_counts_cover_the_kernel_paths():
    """63 / 64 / 65 and 255 / 256 / 257 edges, 1 000 (several per thread), and more than threads x registers of the shipped build"""
    n = {name: int(pc.expected(name)["counts"][0]) for name in pc.WORLDS}
    for want in (63, 64, 65, 255, 256, 257, 1000):
        assert want in n.values()
    assert max(n.values()) > 256 * 4


# ---- apply_matches and the point_row_out rule in numpy ----
def test_apply_matches_and_the_discard_rule():
    frame = np.array([-1, 5, -1, 7, -1], np.int32)
    out = pc.apply_matches(frame, point_row=[10, 11, -1, 13, 14], match_kp=[0, -1, 2, 9, 4])
    assert out.tolist() == [10, 5, -1, 7, 14] and frame.tolist() == [-1, 5, -1, 7, -1]
    r, W = pc.expected("rows_mixed"), pc.world("rows_mixed")
    flagged = r["outlier"] == 1
    assert flagged.any() and (r["row_out"][flagged] == -1).all() and np.array_equal(r["row_out"][~flagged], W["rows"][~flagged])
    assert (r["outlier"][(W["rows"] < 0) | (W["rows"] >= W["n_rows"])] == 0).all()


# ---- the product's side: the header, the bindings, the build ----
def test_header_bindings_and_variant():
    from jetson_slam_amd import build as jb
    from jetson_slam_amd import orb
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    for name in ("jsorb_pose_optimization_async", "jsorb_pose_optimization", "jsorb_pose_optimization_stats", "jsorb_pose_optimization_build_caps",
                 "jsorb_apply_matches_async"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in orb.EXPORTS, name
    assert re.search(r"typedef struct jsorb_pose_params \{\s*float fx, fy, cx, cy, bf;\s*float inv_level_sigma2\[JSORB_MAX_LEVELS\];\s*\} jsorb_pose_params;", hdr)
    import ctypes
    assert ctypes.sizeof(orb.JsorbPoseParams) == 4 * 21
    p = orb.make_pose_params((1, 2, 3, 4), 5, [0.5, 0.25])
    assert (p.fx, p.fy, p.cx, p.cy, p.bf) == (1, 2, 3, 4, 5) and list(p.inv_level_sigma2)[:3] == [0.5, 0.25, 0.0]
    assert jb.VARIANTS["tiny_pose"] == (["-DPO_THREADS=64", "-DPO_EDGE_REGS=1"], ["k_pose.hip"])
    assert "k_pose.hip" in jb.SOURCES and "jsorb_pose.hip" in jb.SOURCES and "pose_optimization" in jb.EXAMPLES
    raw = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    for cite in ("src/Optimizer.cpp:244-456", "types_six_dof_expmap.cpp:266-364", "robust_kernel_impl.cpp:78-91", "base_unary_edge.hpp:56-66",
                 "optimization_algorithm_levenberg.cpp:61-189", "se3quat.h:223-257", "linear_solver_dense.h", "src/Converter.cpp:53-57",
                 "src/Tracking.cpp:1086-1103"):
        assert cite in raw, cite
