"""CPU: the loop's acceptance matcher of jsorb_search_by_projection_sim3 (include/jsorb.h) - ORBmatcher::SearchByProjection(pKF, Scw, vpPoints,
vpMatched, th) (ORBmatcher.cpp:277-390), as LoopClosing::ComputeSim3 calls it (LoopClosing.cpp:380).  Two yardsticks (tests/scw_cases.py): a literal,
sequential transcription in float32 with the contract's arithmetic, cited line by line, and a numpy restatement of what the two kernels compute -
k_scw_candidates' lists of the keys at or below th_low with their cap, k_scw_resolve's fixed point and its walk of the window for a point over the
cap.  The two must agree bit for bit at the caps 2 and 32, on random blocks - each of which has to show every counter of the claim rule - and on
constructed cases, one per decision, each of which asserts the vpMatched it is about.  tests/test_gpu_search_scw.py holds the device to both."""
import ctypes
import os
import re

import numpy as np
import pytest

import scw_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CONSTRUCTED = sc.constructed()


@pytest.mark.parametrize("seed", sc.BLOCK_SEEDS)
def test_restatement_equals_the_transcription_on_random_blocks(po, seed):
    """200 points, 150 clustered keypoints, about a third blocked; at the caps 2 and 32; and every block shows blocked keypoints met inside a
    window, points displaced from their unconstrained best that matched their next key, such points that ended unmatched, points above th_low
    whose keypoint a LATER point then took, at least 4 rounds, and at least one list over the cap of 2"""
    c = sc.block(seed)
    assert len(c["list"]) == 200 and len(c["K"]["x"]) == 150 and 45 <= int((c["matched_in"] >= 0).sum()) <= 55
    assert sc.prove(c) >= 100
    ref, res = sc.both(po, c)
    tr = ref[4]
    for k in sc.COVERAGE:
        assert tr[k] >= 1, (k, dict(tr))
    for cap in (sc.SC_CAP, sc.TINY[0]):
        assert res[cap][4][0] >= 4, res[cap][4]
    assert res[sc.TINY[0]][4][2] >= 1 and res[sc.SC_CAP][4][2] == 0
    assert res[sc.SC_CAP][4][1] == res[sc.TINY[0]][4][1] < res[sc.SC_CAP][4][4]      # keys kept: the same count at both caps, fewer than the distances


@pytest.mark.parametrize("name", list(CONSTRUCTED))
def test_constructed_cases(po, name):
    c, want, count = CONSTRUCTED[name]
    sc.prove(c)
    ref, _ = sc.both(po, c)
    assert list(ref[0]) == want and ref[1] == count, (name, list(ref[0]), ref[1])


def test_trace_shows_what_the_cases_are_about(po):
    tr = lambda name: sc.scw_reference(po, CONSTRUCTED[name][0])[4]
    assert tr("u_at_max_x_and_min_x")["image"] == 1 and tr("a_quarter_pixel_inside_max_x")["image"] == 0 and tr("a_quarter_pixel_outside_min_x")["image"] == 1
    assert tr("depth_zero_and_negative")["depth"] == 2 and tr("dist_at_both_bounds")["distance"] == 2
    assert tr("dot_at_half_the_distance")["angle"] == 0 and tr("dot_below_half_the_distance")["angle"] == 1
    assert tr("octaves_around_the_level")["level"] == 1 and tr("octaves_around_the_level")["distances"] == 2 and tr("only_the_octave_above")["level"] == 1
    assert tr("best_at_th_low_and_one_more")["th_low"] == 1 and tr("a_blocked_keypoint")["blocked_met"] == 1
    assert tr("a_tie_at_two_walk_positions")["distances"] == 2
    assert tr("a_chain_of_four")["displaced_matched"] == 3 and tr("a_non_matching_point_hides_nothing")["later_took"] == 1
    b = tr("bad_and_already_found")
    assert (b["bad_skipped"], b["found_skipped"], b["matches"]) == (1, 1, 1)


def test_the_chain_needs_a_round_per_link_and_its_order_decides(po):
    c, want, _ = CONSTRUCTED["a_chain_of_four"]
    _, res = sc.both(po, c)
    assert res[sc.SC_CAP][4][0] == 5 and res[sc.TINY[0]][4][0] == 5         # four links and the round that changes nothing
    assert res[sc.TINY[0]][4][2] == 4 and res[sc.SC_CAP][4][2] == 0           # five keys a point: over the cap of 2
    r, rwant, _ = CONSTRUCTED["the_chain_reversed"]
    assert want != rwant and np.array_equal(c["K"]["x"], r["K"]["x"]) and list(c["list"]) == list(r["list"])[::-1]


@pytest.mark.parametrize("n", sc.POINT_COUNTS)
def test_point_counts_around_a_workgroup(po, n):
    c = sc.count_case(n)
    sc.prove(c)
    ref, _ = sc.both(po, c)
    assert len(ref[2]) == n and len(c["K"]["x"]) > sc.TINY[1]
    assert n < 15 or ref[1] >= 5


def test_scw_from_pose_is_the_transcriptions_decomposition(orb):
    rng = np.random.default_rng(3)
    for _ in range(50):
        S = rng.normal(size=(4, 4)).astype(np.float32)
        S[3] = [0, 0, 0, 1]
        for a, b in zip(orb.scw_from_pose(S), sc.decompose(S)):
            assert np.array_equal(np.asarray(a, np.float32) + f32(0), np.asarray(b, np.float32))
    c = sc.block(sc.BLOCK_SEEDS[1])
    R, t, O = orb.scw_from_pose(c["Scw"])
    assert np.array_equal(np.abs(R).reshape(3, 3).sum(0), np.ones(3, np.float32))      # a signed permutation again, whatever the scale


# =====================================================================================================================================
# the declarations
# =====================================================================================================================================
NAMES = ("jsorb_search_by_projection_sim3_async", "jsorb_search_by_projection_sim3", "jsorb_search_by_projection_sim3_stats", "jsorb_scw_build_caps")


def test_header_binding_and_build_declare_the_new_entry_points(orb):
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    bound = orb.load_library()
    raw = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(orb.__file__).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in orb.EXPORTS and '"%s": (' % n in src, n
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert decl, n
        n_args = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(getattr(bound, n).argtypes), (n, n_args)
    # JsorbScwParams is the header's field list, in its order, and its size
    body = re.search(r"typedef struct jsorb_scw_params \{(.*?)\} jsorb_scw_params;", hdr, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(re.sub(r"\[.*", "", v.strip()), ctype, "[" in v) for v in names.split(",")]
    assert [f[0] for f in fields] == [f[0] for f in orb.JsorbScwParams._fields_]
    for (name, ctype, arr), (_, t) in zip(fields, orb.JsorbScwParams._fields_):
        base = t._type_ if arr else t
        assert arr == hasattr(t, "_length_") and base is {"float": ctypes.c_float, "int": ctypes.c_int}[ctype], name
    assert ctypes.sizeof(orb.JsorbScwParams) == 64 + 4 * orb.MAX_LEVELS + 15 * 4 and orb.JsorbScwParams.Rcw.offset == 64 + 4 * orb.MAX_LEVELS
    assert "ORBmatcher.cpp:277-390" in raw and "LoopClosing.cpp:380" in raw
    for m in ("search_by_projection_sim3", "search_by_projection_sim3_stats"):
        assert callable(getattr(orb.KeyframeMatcher, m))
    assert callable(orb.scw_params) and callable(orb.scw_from_pose) and orb.scw_build_caps() == (sc.SC_CAP, sc.SC_LDS_CLAIMS)
    from jetson_slam_amd import build as jb
    assert "k_scw.hip" in jb.SOURCES and jb.VARIANTS["tiny_scw_cap"] == (["-DSC_CAP=%d" % sc.TINY[0], "-DSC_LDS_CLAIMS=%d" % sc.TINY[1]], ["k_scw.hip"])
    ksrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_scw.hip")).read()
    csrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_search_common.h")).read()
    for name, val, text in (("SC_CAP", sc.SC_CAP, ksrc), ("SC_LDS_CLAIMS", sc.SC_LDS_CLAIMS, ksrc), ("SL_LANES", sc.SL_LANES, csrc)):
        assert re.search(r"#define %s %d\b" % (name, val), text), name
    assert "claim_resolve<SC_CAP>" in ksrc and "compact_window<SC_CAP>" in ksrc and "<= a.p.th_low" in ksrc


def test_params_helper(orb):
    prm = sc.tf.default_params(check=0, th=f32(10))
    R, t, O = sc.decompose(sc.cases.scw_of(sc.tf.IDENTITY, 2.0))
    p = orb.scw_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]),
                       (prm["inv_w"], prm["inv_h"]), prm["log_sf"], prm["scale"], R, t, O)
    assert (p.th, p.th_low, p.cols, p.rows, p.n_levels) == (10.0, 50, 64, 48, 8) and p.max_x == 320 and p.inv_h == prm["inv_h"]
    assert np.array_equal(np.array(p.scale_factor[:8], np.float32), prm["scale"]) and f32(p.log_scale_factor) == prm["log_sf"]
    assert list(p.Rcw) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.tcw) == [0, 0, 0] and list(p.Ow) == [0, 0, 0]
    with pytest.raises(orb.JsorbError):
        orb.scw_params((1, 1, 0, 0), (0, 1, 0, 1), (1, 1), 0.18, [1.0], np.zeros(8), t, O)


def test_validation_without_a_device(orb):
    """a NULL matcher is refused by every entry point, and the binding refuses what it can see without a device: a params object of another
    class, a host array, a wrong dtype or shape, a strided tensor, a misaligned descriptor"""
    import torch
    from kf_refusal_cases import FakeTensor
    lib = orb.load_library()
    p = orb.JsorbScwParams()
    args = [ctypes.byref(p), 0] + [None] * 10 + [0] + [None] * 5
    assert lib.jsorb_search_by_projection_sim3_async(None, *args, None, None, None, None) == -1
    assert lib.jsorb_search_by_projection_sim3(None, *args, None, None, None, None) == -1
    assert lib.jsorb_search_by_projection_sim3_stats(None, None, None, None, None, None, None) == -1
    assert lib.jsorb_scw_build_caps(None, None) == 0
    K = orb.KeyframeMatcher
    dt = dict(octave=torch.int32, desc=torch.uint8, blocked=torch.uint8)
    side = lambda keys, n: {k: FakeTensor(dt.get(k, torch.float32), (n, 32) if k.endswith("desc") else (n,)) for k in keys}

    def refused(points, keyframe, params=p):
        with pytest.raises(orb.JsorbError) as e:
            K._scw_args(None, points, keyframe, params)
        return str(e.value)
    pts, kf = side(K.POINT_KEYS, 3), side(K.SCW_KF_KEYS, 5)
    assert K._scw_args(None, pts, kf, p)[1:3] == (3, 5)
    assert K._scw_args(None, pts, dict(kf, blocked=None), p)[3][-1] is None            # nothing blocked: a NULL pointer
    assert "params must come from scw_params" in refused(pts, kf, orb.JsorbSim3Params())
    assert "must be a device tensor" in refused(dict(pts, Nx=np.zeros(3, np.float32)), kf)
    assert "must be a device tensor" in refused(pts, dict(kf, y=FakeTensor(torch.float32, (5,), is_cuda=False)))
    assert "must be a contiguous" in refused(pts, dict(kf, octave=FakeTensor(torch.float32, (5,))))
    assert "must be a contiguous" in refused(dict(pts, max_distance=FakeTensor(torch.float32, (4,))), kf)
    assert "must be a contiguous" in refused(pts, dict(kf, blocked=FakeTensor(torch.uint8, (5,), contiguous=False)))
    assert "16-byte aligned" in refused(dict(pts, desc=FakeTensor(torch.uint8, (3, 32), ptr=4104)), kf)
    assert "16-byte aligned" in refused(pts, dict(kf, desc=FakeTensor(torch.uint8, (5, 32), ptr=4100)))


def test_shim_compiles_with_and_without_the_opencv_double(orb, tmp_path):
    """include/jsorb_compat.hpp: Jetson_SLAM::SearchByProjection(jsorb::KeyframeMatcher&, ...) in the reference's argument shape compiles with plain
    g++ and links"""
    import subprocess
    src = tmp_path / "scw_shim.cpp"
    src.write_text('#include "jsorb_compat.hpp"\n'
                   "int main(int argc, char **) {\n"
                   "    if (argc < 100) return 0;                // compiled and linked, not run: no device here\n"
                   "    jsorb::KeyframeMatcher m; jsorb::ScwKeyframe kf; jsorb_scw_params p{}; const float Scw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};\n"
                   "    std::vector<jsorb::ScwPoint> table(2); std::vector<const jsorb::ScwPoint *> vpPoints{&table[0], &table[1]}, vpMatched;\n"
                   "    return Jetson_SLAM::SearchByProjection(m, p, kf, Scw, vpPoints, vpMatched, 10);\n}\n")
    lib = os.path.join(ROOT, "jetson_slam_amd")
    for extra in ([], ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")]):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                              [str(src), "-L", lib, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib, "-o", str(tmp_path / "scw_shim")])


def test_example_compiles_against_the_opencv_double(orb, tmp_path):
    from jetson_slam_amd import build as jb
    exe = jb.build_example("compute_sim3", str(tmp_path / "compute_sim3"), ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")])
    assert os.path.exists(exe)
    text = open(os.path.join(ROOT, "examples", "compute_sim3.cpp")).read()
    assert "SearchByProjection(" in text and "nTotalMatches" in text
