"""-m "not gpu": the sequential transcription of tests/new_points_cases.py against the reference's own src/LocalMapping.cpp, src/KeyFrame.cpp and
src/MapPoint.cpp - the worlds recorded in tests/golden/ref_matcher_newpoints.npz (tools/ref_newpoints_goldens.py; ORBmatcher::SearchForTriangulation
stubbed by the rule of ORBmatcher.cpp:686-690 over recorded candidates) - and, where the reference tree is present, the driver rebuilt and compared
live.  The SVD definition is checked over every A of the recorded worlds."""
import numpy as np
import pytest

import new_points_cases as nc
from test_new_points_host import SVD_MEASURED

GOLDEN = nc.load_golden()
WORLDS = nc.golden_worlds(GOLDEN)


def test_the_file_holds_the_worlds_and_what_they_are_for():
    assert list(GOLDEN) == list(WORLDS) and len(WORLDS) == len(nc.REF_SEEDS)
    totals, paths = np.zeros(len(nc.COUNTS), int), np.zeros(4, int)
    for name, rec in GOLDEN.items():
        W = WORLDS[name]
        assert sorted(rec) == ["crc", "raw"] and rec["raw"].dtype == np.int32
        assert W["S"] <= 16 and max(W["point_len"]) <= 200 and 1 <= len(W["neighbours"]) <= 10
        r = nc.restate(W)
        totals += r["counts"]
        for row, idx1, t, _ in r["log"]:
            paths[r["path"][t, idx1]] += row >= 0
    c = dict(zip(nc.COUNTS, totals.tolist()))
    # the first-owner rule, shared KF2 keypoints and all three paths occur in what the reference ran
    assert c["n_created"] >= 200 and c["n_taken"] >= 100 and c["n_shared_kf2"] >= 3 and (paths[1:] >= 10).all(), (c, paths)
    assert any(W["uright"] is None for W in WORLDS.values()) and any(W["raw_x"] is None for W in WORLDS.values())


@pytest.mark.parametrize("name", list(WORLDS))
def test_the_transcription_reproduces_the_reference(name):
    W = WORLDS[name]
    nc.same_as_recorded(W, nc.restate(W), GOLDEN[name]["raw"], name)


def test_a_misreading_is_told_apart(monkeypatch):
    """the recording has teeth where a shared misreading could hide: KF2's own mbf at :412, `if` for `else if` at :318-322, the observations'
    order, a float dot"""
    name = next(n for n, W in WORLDS.items() if W["uright"] is not None)
    W = WORLDS[name]
    poses = [dict(p) for p in W["poses"]]
    poses[0]["mbf"] = np.float32(poses[0]["mbf"] * 2)
    with pytest.raises(AssertionError):
        nc.same_as_recorded(W, nc.restate(nc.edited(W, "mbf", poses=poses)), GOLDEN[name]["raw"])
    with pytest.raises(AssertionError):
        nc.same_as_recorded(W, nc.restate(nc.edited(W, "order", order_key=-W["order_key"])), GOLDEN[name]["raw"])
    failed = 0
    for n2, W2 in WORLDS.items():
        monkeypatch.setattr(nc, "norm3", lambda v: np.sqrt(np.float32(np.float64(v[0]) ** 2 + np.float64(v[1]) ** 2 + np.float64(v[2]) ** 2)))
        try:
            nc.same_as_recorded(W2, nc.restate(W2), GOLDEN[n2]["raw"])
        except AssertionError:
            failed += 1
        monkeypatch.undo()
    assert failed >= 1                           # a norm summed in double is not the reference's


def test_the_contracts_svd_over_the_recorded_matrices():
    worst, n = 0.0, 0
    for W in WORLDS.values():
        log = []
        nc.restate(W, log)
        for A, col in log:
            vt = np.linalg.svd(A.astype(np.float64))[2]
            want = vt[3][:3] / vt[3][3]
            worst, n = max(worst, np.abs(col[:3] / col[3] - want).max() / np.abs(want).max()), n + 1
    print("largest relative difference of x3D over %d recorded matrices: %.3g" % (n, worst))
    assert n >= 150 and worst <= 4 * SVD_MEASURED


def test_the_driver_rebuilt_gives_the_recorded_arrays(tmp_path):
    ref = nc.reference_tree()
    if ref is None:
        pytest.skip("the reference tree is not here")
    nc.build_driver(ref)
    for name, W in nc.golden_worlds().items():
        rec = nc.run_driver(W, str(tmp_path))
        for k in ("raw", "crc"):
            assert np.array_equal(rec[k], GOLDEN[name][k]), (name, k)
