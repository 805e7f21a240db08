"""CPU: the yardstick of jsorb_create_new_map_points (tests/new_points_cases.py) - that its named cases reach every exit of the loop, that the
contract's cv::SVD::compute is an SVD, that the sequential loop agrees with the closed form the device uses - and the declarations of the new
entry points in the header, the binding and the build."""
import ctypes
import os
import re

import numpy as np
import pytest

import new_points_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jsorb_create_new_map_points_async", "jsorb_create_new_map_points", "jsorb_create_new_map_points_stats", "jsorb_create_new_map_points_build_caps")
# The largest relative difference of x3D between the contract's Jacobi and numpy.linalg.svd in float64 over every A of the named cases, measured on
# the CPU: 8.4e-14, with singular-value ratios s0/s2 up to 15 - seven orders below float epsilon times that ratio.  The bound is four times the
# figure: the margin covers LAPACK builds that differ in the last bits.
SVD_MEASURED = 8.4e-14


def test_the_named_cases_reach_every_verdict_and_every_path():
    verdicts, paths = np.zeros(len(nc.VERDICTS), int), np.zeros(4, int)
    for name in nc.named():
        r = nc.restated(name)
        verdicts += np.bincount(r["verdict"].ravel(), minlength=len(nc.VERDICTS))
        paths += np.bincount(r["path"].ravel(), minlength=4)
    assert (verdicts > 0).all(), dict(zip(nc.VERDICTS, verdicts.tolist()))
    assert (paths > 0).all(), paths
    for k in nc.UNITS:                           # every hand-built world leaves at the exit it is named after
        r = nc.restated("unit_" + k)
        assert r["verdict"].tolist() == [[nc.V[k]]], (k, r["verdict"])


def test_the_named_cases_hold_the_situations_they_are_named_after():
    C, V = nc.named(), nc.V
    count = lambda name, key: int(nc.restated(name)["counts"][nc.COUNTS.index(key)])
    gates = [V[k] for k in ("low_parallax", "w_zero", "z1", "z2", "reprojection1", "reprojection2", "zero_distance", "scale_ratio", "empty_unprojection")]
    v = nc.restated("mixed")["verdict"]
    # an idx1 matched by two acceptable neighbours: the first owns it, the later pair is taken
    assert any(V["created"] in col and V["taken"] in col[list(col).index(V["created"]):] for col in v.T)
    # an idx1 whose first pair fails a gate and whose second is accepted
    assert sum(1 for col in v.T if V["created"] in col and any(g in col[:list(col).index(V["created"])] for g in gates)) >= 3
    assert count("shared_kf2", "n_shared_kf2") >= 3
    r = nc.restated("shared_kf2")
    rows = r["log"][r["log"][:, 0] >= 0]
    assert len({(int(t), int(i2)) for _, _, t, i2 in rows}) == len(rows) - count("shared_kf2", "n_shared_kf2")
    assert count("rows_one_short", "n_no_row") == 1 and count("rows_out_of_range", "n_no_row") == 2
    assert count("log_cap_0", "log_overflow") == 1 and count("log_one_short", "log_overflow") == 1 and (nc.restated("log_one_short")["log"] >= 0).all()
    assert nc.restated("bad_neighbour_in_the_middle")["verdict"][1].tolist() == [V["skipped_neighbour"]] * C["base"]["n1"]
    assert count("odd_neighbours", "n_skipped_neighbours") == 3 and count("run_longer_than_capacity", "n_skipped_neighbours") == 2
    assert count("repeated_neighbour", "n_skipped_neighbours") == 1 and (nc.restated("repeated_neighbour")["verdict"][2] == V["skipped_neighbour"]).all()
    assert count("bad_current", "no_current") == 1 and count("wrong_n1", "no_current") == 1
    assert sorted(C[k]["n1"] for k in ("n1_0", "n1_1", "twenty", "no_raw", "mixed")) == [0, 1, 63, 64, 65]
    assert len(C["no_neighbours"]["neighbours"]) == 0 and len(C["twenty"]["neighbours"]) == 20 and len(C["unit_created"]["neighbours"]) == 1
    assert C["mono"]["uright"] is None and C["mono"]["ref_slot"] is None and C["no_raw"]["raw_x"] is None
    # a stereo, a monocular and a mixed pair among the created ones, and mvDepth <= 0 with mvuRight >= 0
    W, r = C["mixed"], nc.restated("mixed")
    kinds = set()
    for row, idx1, t, idx2 in r["log"]:
        if row >= 0:
            e1 = W["point_off"][W["current_slot"]] + idx1
            e2 = W["point_off"][W["neighbours"][t]] + idx2
            kinds.add((bool(W["uright"][e1] >= 0), bool(W["uright"][e2] >= 0)))
    assert len(kinds) == 4
    assert ((W["uright"] >= 0) & (W["depth"] <= 0)).sum() >= 3 and count("mixed", "n_unprojected") >= 10
    # rows that were bad or held other values are reused: the call rewrites every field
    assert any(W["bad"][row] for row, *_ in r["log"] if row >= 0)
    # the values outside [-1, n_rows) in the pool are not free, the KF1 octaves out of range match nothing
    W, r = C["odd_pool_values"], nc.restated("odd_pool_values")
    assert (r["verdict"][:, :4] == V["no_match"]).all() and np.array_equal(r["point_pool"][W["point_off"][W["current_slot"]]:][:2], [-5, W["n_rows"] + 9])


def test_the_world_sizes_stay_small():
    for name, W in nc.named().items():
        assert W["S"] <= 24 and max(W["point_len"], default=0) <= 200 and len(W["neighbours"]) <= 20, name


def test_the_contracts_svd_is_an_svd():
    """the null vector of every A of the named cases against numpy.linalg.svd in float64: x3D within four times the measured difference"""
    worst, n, ratios = 0.0, 0, []
    for name in nc.named():
        log = []
        nc.restate(nc.named()[name], log)
        for A, col in log:
            s, vt = np.linalg.svd(A.astype(np.float64))[1:]
            if col[3] == 0.0:                    # (unit_w_zero: the point at infinity, exactly)
                assert abs(vt[3][3]) < 1e-15
                continue
            rel = np.abs(col[:3] / col[3] - vt[3][:3] / vt[3][3]).max() / np.abs(vt[3][:3] / vt[3][3]).max()
            print("%s: s0/s2 %.3g, x3D differs by %.3g" % (name, s[0] / s[2], rel))
            worst, n = max(worst, rel), n + 1
            ratios.append(rel / (np.finfo(np.float32).eps * s[0] / s[2]))
    print("largest relative difference of x3D over %d matrices: %.3g" % (n, worst))
    assert n >= 500
    assert worst <= 4 * SVD_MEASURED
    assert max(ratios) < 1e-5                    # far below float epsilon times the condition number


def test_eight_sweeps_are_twice_what_the_cases_need(monkeypatch):
    log = []
    for name in ("mixed", "twenty", "mono"):
        nc.restate(nc.named()[name], log)
    monkeypatch.setattr(nc, "SWEEPS", 4)
    assert all(nc.null_vector(A)[1] == col.tolist() for A, col in log)
    monkeypatch.setattr(nc, "SWEEPS", 2)
    assert any(nc.null_vector(A)[1] != col.tolist() for A, col in log)


def test_the_neighbours_mbf_is_not_read():
    """:412 takes mpCurrentKeyFrame->mbf for KF2's right-image error: a world whose neighbours carry another mbf and mb gives the same result, and
    one whose current keyframe does gives another"""
    want, W = nc.restated("mixed"), nc.named()["mixed"]
    nc.same(want, nc.restated("neighbour_mbf"), "neighbour_mbf")
    assert all(p["mbf"] != W["poses"][0]["mbf"] for p in nc.named()["neighbour_mbf"]["poses"][1:])
    poses = [dict(p) for p in W["poses"]]
    poses[0]["mbf"] = np.float32(poses[0]["mbf"] * 4)
    with pytest.raises(AssertionError):
        nc.same(want, nc.restate(nc.edited(W, "current_mbf", poses=poses)), "current_mbf")


def test_header_binding_and_build_declare_the_new_entry_points(orb):
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    bound = orb.load_library()
    full = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    src = open(orb.__file__).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in orb.EXPORTS and '"%s": (' % n in src, n
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert decl, n
        n_args = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(getattr(bound, n).argtypes), (n, n_args)
    assert ctypes.sizeof(orb.JsorbNewPointKeypoints) == 5 * 8 and ctypes.sizeof(orb.JsorbNewPointState) == 18 * 8
    assert orb.KEYFRAME_POSE_DTYPE.itemsize == 23 * 4
    fields = re.search(r"typedef struct jsorb_new_point_state \{(.*?)\} jsorb_new_point_state;", hdr, re.S).group(1)
    assert re.findall(r"\*(\w+)", fields) == [f for f, _ in orb.JsorbNewPointState._fields_]
    fields = re.search(r"typedef struct jsorb_keyframe_pose \{(.*?)\} jsorb_keyframe_pose;", hdr, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?[,;]", fields) == list(orb.KEYFRAME_POSE_DTYPE.names)
    assert tuple(orb.NEW_POINTS_VERDICTS) == nc.VERDICTS and tuple(orb.NEW_POINTS_COUNTS) == nc.COUNTS and tuple(orb.NEW_POINTS_OUTPUTS) == nc.OUTPUTS
    for m in ("create_new_map_points", "create_new_map_points_host", "create_new_map_points_stats"):
        assert callable(getattr(orb.KeyframeMatcher, m))
    from jetson_slam_amd import build as jb
    assert "k_new_points.hip" in jb.SOURCES and "jsorb_new_points.hip" in jb.SOURCES and "triangulate_new_map_points" in jb.EXAMPLES
    assert jb.VARIANTS["tiny_new_points"] == (["-DNP_CHUNK=%d" % nc.CHUNKS[1]], ["k_new_points.hip"])
    ksrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_new_points.hip")).read()
    assert re.search(r"#define NP_CHUNK %d\b" % nc.CHUNKS[0], ksrc) and re.search(r"#define NP_SWEEPS %d\b" % nc.SWEEPS, ksrc)
    assert "fma" not in re.sub(r"//.*", "", ksrc)                        # the contract's arithmetic has no fused multiply-add
    assert "EIGHT sweeps" in full and "THE NEIGHBOURS ARE NOT INDEPENDENT" in full


def test_the_pose_helper_matches_the_worlds(orb):
    W = nc.named()["mixed"]
    for p in W["poses"]:
        rec = orb.make_keyframe_pose(p["Rcw"], p["tcw"], (p["fx"], p["fy"], p["cx"], p["cy"]), mb=p["mb"], mbf=p["mbf"])
        for k in orb.KEYFRAME_POSE_DTYPE.names:
            assert np.array_equal(np.asarray(rec[k], np.float32).view(np.uint32), np.asarray(p[k], np.float32).view(np.uint32)), k


def test_validation_without_a_device(orb):
    """a NULL matcher is refused by every entry point"""
    lib = orb.load_library()
    assert lib.jsorb_create_new_map_points_async(*[None] * 7, 0, 0, 0, 0, None, None, None, None, 1.8, 0, 0, None, 0, *[None] * 5) == -1
    assert lib.jsorb_create_new_map_points(*[None] * 7, 0, 0, 0, 0, None, None, None, None, 1.8, 0, 0, None, 0, *[None] * 10) == -1
    assert lib.jsorb_create_new_map_points_stats(None, None) == -1
    chunk = ctypes.c_int()
    assert lib.jsorb_create_new_map_points_build_caps(ctypes.byref(chunk)) == 0 and chunk.value == nc.CHUNKS[0]


def test_shim_and_example_compile_with_and_without_the_opencv_double(orb, tmp_path):
    """include/jsorb_compat.hpp: jsorb::NewPointKeypoints, jsorb::NewPointState and Jetson_SLAM::CreateNewMapPoints compile with plain g++ and link"""
    from jetson_slam_amd import build as jb
    for i, extra in enumerate(([], ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")])):
        assert os.path.exists(jb.build_example("triangulate_new_map_points", str(tmp_path / ("example%d" % i)), extra))
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert re.search(r"class NewPointKeypoints \{", shim) and re.search(r"class NewPointState \{", shim) and re.search(r"inline int CreateNewMapPoints\(", shim)
