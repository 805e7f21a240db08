"""-m gpu: the device matchers against the reference's OWN src/ORBmatcher.cpp - the stored outputs of tests/golden/ref_matcher_<name>.npz
(tools/ref_matcher_goldens.py; tests/test_ref_matcher.py holds the host yardsticks to the same files), bit for bit, in the synchronous and the
asynchronous form of each entry point, with the call's statistics against the transcription's trace counters stored next to the outputs.
No test here reads the reference tree or oracle/_ref.

The entry points of jsorb_keyframe_matcher take their keyframes as arrays, so every case of their files runs as stored: the random blocks in the
call shape they were drawn for (one keyframe against 3 loop candidates, one keyframe against 4 neighbours), the constructed cases one by one.
jsorb_search_by_bow matches keyframes given as arrays against the handle's frame, of which it reads descriptors, angles and the nodes the caller
passes: every case of its file runs too, its frame side written over the first keypoints of an extracted frame (tests/test_gpu_bow.py: poke_frame).
The other entry points of a frame handle match against the frame the handle extracted.  Of their files the blocks drawn on an extracted frame
("real": 484 keypoints, 500 - 800 points a case) run against that extraction: the test extracts the same synthetic image (ref_matcher_cases.SYNTH)
and requires the stored frame.  Every other case - the generators' random blocks and the constructed chains - is stored as a handle can hold it
(ref_matcher_cases.on_handle: integer coordinates, padded to the keypoint count of the POKE handle) and is written over that handle's keypoints
(tests/test_gpu_search_kf.py: poke_keypoints); the grid comes from the caller's parameters.  No case of any file is left out.
The two Fuse overloads return bestIdx / bestDist per (keyframe, point) and leave the map to the caller: their files hold the reference's run on a
live map (event log, final map, nFused per keyframe), and the device's results go through the caller's replay of tests/fuse_replay.py - the first
call in the stored shape, then the follow-up calls for points whose descriptor a Replace changed - before they are compared."""
import numpy as np
import pytest

import fuse_replay
import ref_matcher_cases as cases
from oracle import pyref_matcher as rm
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED
from test_gpu_bow import bow_params, concat as concat_bow, padded, poke_frame
from test_gpu_fuse import concat as concat_fuse, dev_keyframes, dev_points, fuse_params, pose_arrays
from test_gpu_loop import bow_prm, dev_bow, dev_sim3, sim3_prm
from test_gpu_search_init import init_params
from test_gpu_search_kf import POINT_KEYS as KF_POINT_KEYS, c_params as kf_c_params, poke_keypoints
from test_gpu_search_last_frame import run_device as run_last_frame
from test_gpu_search_local import _dev, _mk, run_device as run_local
from test_gpu_triangulation import KF1_DT, KF2_DT, concat, dev_side, tri_params
from test_loop_host import concat_sides

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(orb):
    m = orb.KeyframeMatcher()
    yield m
    m.close()


def plain(prm):
    """numpy scalars of a stored prm as Python numbers (the binding's parameter structs are ctypes)"""
    return {k: v.item() if isinstance(v, np.generic) else v for k, v in prm.items()}


def calls_of(golden, same_side="KF1"):
    """the cases of a file grouped into device calls: consecutive random cases of one block that share the first keyframe and the parameters form one
    call, every other case is a call of its own"""
    calls = []
    for name, c in golden.items():
        prev = calls[-1] if calls else None
        if (prev and cases.block_of(name) and cases.block_of(prev[0][0]) == cases.block_of(name)
                and all(np.array_equal(np.asarray(c[same_side][k]), np.asarray(prev[0][1][same_side][k])) for k in c[same_side])
                and all(np.array_equal(np.asarray(c["prm"][k]), np.asarray(prev[0][1]["prm"][k])) for k in c["prm"])):
            prev.append((name, c))
        else:
            calls.append([(name, c)])
    return calls


def test_search_by_bow_kf(orb, matcher):
    golden = rm.load_golden("search_by_bow_kf")
    calls = calls_of(golden)
    assert max(len(call) for call in calls) == 3 and sum(len(call) for call in calls) == len(golden)
    for call in calls:
        KF1, prm = call[0][1]["KF1"], plain(call[0][1]["prm"])
        cat, start = concat_sides([c["KF2"] for _, c in call])
        want = np.stack([c["out"]["matches12"] for _, c in call])
        count = np.array([int(c["out"]["nmatches"]) for _, c in call])
        ctr = [c["counters"] for _, c in call]
        stats = (sum(int(t["node_pairs"]) for t in ctr), sum(int(t["distances"]) for t in ctr), max(int(t["largest_node"]) for t in ctr),
                 tuple(int(v) for v in ctr[0]["ind"]))
        for sync in (False, True):
            d1, d2 = dev_bow(KF1), dev_bow(cat)
            if sync:
                mk, cnt = matcher.search_by_bow_kf_host(d1, start, d2, bow_prm(orb, prm))
            else:
                mk, cnt = matcher.search_by_bow_kf(d1, start, d2, bow_prm(orb, prm))
                mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
            names = [n for n, _ in call]
            assert mk.shape == want.shape and np.array_equal(mk, want) and np.array_equal(np.asarray(cnt).ravel(), count), (names, sync)
            assert matcher.search_by_bow_kf_stats() == stats, (names, matcher.search_by_bow_kf_stats(), stats)


def test_search_for_triangulation(orb, matcher):
    golden = rm.load_golden("search_for_triangulation")
    calls = calls_of(golden)
    assert max(len(call) for call in calls) == 4 and sum(len(call) for call in calls) == len(golden)
    for call in calls:
        KF1, prm = call[0][1]["KF1"], plain(call[0][1]["prm"])
        n1 = len(KF1["node"])
        start, cat = concat([c["KF2"] for _, c in call])
        F = np.stack([np.asarray(c["geom"]["F12"], np.float32).reshape(9) for _, c in call])
        E = np.array([[c["geom"]["ex"], c["geom"]["ey"]] for _, c in call], np.float32).reshape(-1, 2)
        want = np.full((len(call), n1), -1, np.int64)
        for i, (_, c) in enumerate(call):
            pairs = np.asarray(c["out"]["pairs"], np.int64).reshape(-1, 2)
            want[i, pairs[:, 0]] = pairs[:, 1]
        count = np.array([int(c["out"]["nmatches"]) for _, c in call])
        ctr = [c["counters"] for _, c in call]
        live = [t for (_, c), t in zip(call, ctr) if n1 and len(c["KF2"]["node"])]      # (an empty side: no work and no statistics)
        stats = (sum(int(t["node_pairs"]) for t in live), sum(int(t["distances"]) for t in live), sum(int(t["line_tests"]) for t in live),
                 max([int(t["largest_node"]) for t in live] + [0]), tuple(int(v) for v in ctr[0]["ind"]) if live else (-1, -1, -1))
        for sync in (False, True):
            d1, d2 = dev_side(KF1, KF1_DT), dev_side(cat, KF2_DT)
            if sync:
                mk, cnt = matcher.search_for_triangulation_host(d1, start, d2, F, E, tri_params(orb, prm))
            else:
                mk, cnt = matcher.search_for_triangulation(d1, start, d2, F, E, tri_params(orb, prm))
                mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
            names = [n for n, _ in call]
            assert mk.shape == want.shape and np.array_equal(mk, want) and np.array_equal(np.asarray(cnt).ravel(), count), (names, sync)
            assert matcher.stats() == stats, (names, matcher.stats(), stats)


# ---- the two Fuse overloads: the device's best_idx / best_dist through the caller's replay, against the reference's run on a live map ----
def device_fuse_search(orb, matcher, c, sync):
    """fuse_replay's search on the device: one jsorb_fuse call per search, over the target keyframes and list points asked for, in the stored call
    shape (all keyframes of a case in the first call), with the descriptors the map holds at that moment"""
    prm = fuse_params(orb, cases.fuse_prm(c))

    def search(ts, idxs, desc, skip):
        sides = [cases.kf_side(c, int(c["targets"][t])) for t in ts]
        start, cat = concat_fuse([K for K, _ in sides])
        R, t, O = pose_arrays([pose for _, pose in sides])
        dp, dk = dev_points(cases.list_points(c, idxs, desc)), dev_keyframes(cat)
        if sync:
            bi, bd, cnt = matcher.fuse_host(dp, start, dk, R, t, O, prm, skip=_dev(skip))
        else:
            bi, bd, cnt = matcher.fuse(dp, start, dk, R, t, O, prm, skip=_dev(skip))
            bi, bd, cnt = bi.cpu().numpy(), bd.cpu().numpy(), cnt.cpu().numpy()
        assert np.array_equal(np.asarray(cnt).ravel(), (bi >= 0).sum(1))
        return bi, bd, matcher.fuse_stats()
    return search


@pytest.mark.parametrize("name", ["fuse", "fuse_sim3"])
def test_fuse_through_the_replay(orb, matcher, name):
    """every case of the file, check_reprojection 1 (Fuse(pKF, vpMapPoints, th)) and 0 (the overload with Scw): the events, the final map and nFused
    per keyframe that the caller's replay makes of the device's results are the stored reference's, and the statistics of every device call - the
    first over all target keyframes, then one per keyframe after which a descriptor changed - are the transcription's"""
    golden = rm.load_golden(name)
    m = cases.MATCHERS[name]
    fused = n_calls = 0
    for cname, c in golden.items():
        c = m.prepare(c)
        assert int(c["prm"]["check"]) == (name == "fuse")
        for sync in (False, True):
            got, calls, _ = fuse_replay.replay(c, device_fuse_search(orb, matcher, c, sync), "research")
            try:
                fuse_replay.same_map(got, c["out"])
            except AssertionError as e:
                raise AssertionError("%s / %s (sync %s): the replay of the device's result is not the reference's run" % (name, cname, sync)) from e
            assert np.array_equal(np.asarray(calls, np.int64).reshape(-1, 4), c["counters"]["calls"]), (cname, sync, calls)
        fused += int(c["out"]["nmatches"])
        n_calls += len(calls)
    assert fused > 500 and n_calls > len(golden)                   # not vacuous: the reference fused, and descriptors changed between keyframes
    assert max(len(c["targets"]) for c in golden.values()) == 33   # one call crosses FUSE_KF_CHUNK


def test_search_by_sim3(orb, matcher):
    """every case, both call forms: the new entries of vpMatches12 (as keypoints of keyframe 2; the reference leaves the pre-filled ones as they
    were), nFound and the statistics tuple"""
    golden = rm.load_golden("search_by_sim3")
    m = cases.MATCHERS["search_by_sim3"]
    total = 0
    for cname, c in golden.items():
        c = m.prepare(c)
        S1, S2 = cases.sim3_sides(c)
        want, found, ctr = m.expected_m12(c), int(c["out"]["nmatches"]), c["counters"]
        stats = tuple(int(ctr[k]) for k in ("windows", "walked", "distances", "largest")) + (found,)
        for sync in (False, True):
            d1, d2 = dev_sim3(S1), dev_sim3(S2)
            if sync:
                m1, m2, m12, n = matcher.search_by_sim3_host(d1, d2, sim3_prm(orb, cases.fuse_prm_sim3(c)))
            else:
                m1, m2, m12, n = matcher.search_by_sim3(d1, d2, sim3_prm(orb, cases.fuse_prm_sim3(c)))
                m12, n = m12.cpu().numpy(), int(n.cpu()[0])
            assert np.array_equal(m12, want) and int(n) == found, (cname, sync)
            assert matcher.search_by_sim3_stats() == stats, (cname, matcher.search_by_sim3_stats(), stats)
        total += found
    assert total > 100


# ---- the entry points of a frame handle ----
@pytest.fixture(scope="module")
def frame(orb, configs):
    c = configs[cases.SYNTH["config"]]
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(cases.SYNTH["seed"], c["h"], c["w"])[0])
    yield g
    g.close()


def same_frame(g, F, angle):
    """the handle's frame is the stored one"""
    kp, (xu, yu) = g.keypoints(0), g.keypoints_undistorted(0)
    n = len(kp) // 6
    assert np.array_equal(F["kx"], xu) and np.array_equal(F["ky"], yu) and np.array_equal(F["octave"], kp[4 * n:5 * n])
    assert np.array_equal(F["desc"], g.descriptors(0))
    assert not angle or np.array_equal(F["angle"].view(np.int32), kp[3 * n:4 * n])


@pytest.fixture(scope="module")
def poked(orb):
    c = cases.POKE
    g = _mk(orb, c)
    g.extract(synth_stereo_pair(c["seed"], c["h"], c["w"])[0])
    yield g
    g.close()


def handle_cases(orb, name, frame, poked, angle=False):
    """every case of a file with the handle that holds its frame: for the real cases the extraction itself (frame 0: the SYNTH image; frame 1: the
    POKE handle's own image, extracted again), for all others the POKE handle with the case's frame written over its keypoints"""
    golden = rm.load_golden(name)
    n_real = 0
    for cname, c in golden.items():
        F = c["F"] if "F" in c else c["F2"]
        if cases.is_real(cname):
            g = frame
            if int(c["frame"]) == 1:
                g = poked
                g.extract(synth_stereo_pair(cases.POKE["seed"], cases.POKE["h"], cases.POKE["w"])[0])
            same_frame(g, F, angle)
            n_real += 1
            yield cname, c, g
            continue
        N = poked.n_keypoints(0)
        assert len(F["kx"]) == N, "the stored frames are padded to the POKE handle's keypoint count"
        if "scale" in F:
            assert np.array_equal(poked.get_scale_factors()[:len(F["scale"])], F["scale"])
        poke_keypoints(orb, poked, F["kx"], F["ky"], F["octave"], F["angle"] if "angle" in F else np.zeros(N, np.float32), F["desc"])
        yield cname, c, poked
    assert 0 < n_real < len(golden)


def grid_ints(F):
    return dict(F, cols=int(F["cols"]), rows=int(F["rows"]))


def test_search_local_points(orb, frame, poked):
    total = 0
    for name, c, g in handle_cases(orb, "search_local", frame, poked):
        prm, F = plain(c["prm"]), grid_ints(c["F"])
        ur = None if F["u_right"] is None else _dev(np.asarray(F["u_right"], np.float32))
        m, d, km, cnt = run_local(g, F, c["P"], prm["th"], ur, nn_ratio=prm["nn_ratio"], th_high=cases.TH_HIGH)
        want = np.where(c["out"]["kp_match"] == -2, -1, c["out"]["kp_match"])
        assert np.array_equal(km, want) and cnt == int(c["out"]["nmatches"]), name
        assert cnt > 100 or not cases.is_real(name), name
        held = {int(i): k for k, i in enumerate(want) if i >= 0}
        assert all(int(m[i]) == held.get(i, -1) for i in range(len(m))), name
        ctr = c["counters"]
        assert g.search_local_stats() == (int(ctr["rounds"]), int(ctr["candidates"]), int(ctr["overflow"])), (name, g.search_local_stats())
        total += cnt
    assert total > 1000


def test_search_last_frame(orb, frame, poked):
    total = 0
    for name, c, g in handle_cases(orb, "search_last_frame", frame, poked, angle=True):
        prm, F = plain(c["prm"]), grid_ints(c["F"])
        ur = None if F["u_right"] is None else _dev(np.asarray(F["u_right"], np.float32))
        m, d, km, cnt = run_last_frame(orb, g, F, c["P"], prm, ur)
        assert np.array_equal(km, c["out"]["kp_match"]) and cnt == int(c["out"]["nmatches"]), name
        assert cnt > 100 or not cases.is_real(name), name
        ctr = c["counters"]
        # (the first field counts the passes of TrackWithMotionModel's retry, which is Tracking.cpp: the cases are drawn with retry_below = 0, one pass)
        assert g.search_last_frame_stats() == (1, int(ctr["candidates"]), tuple(int(v) for v in ctr["ind"])), (name, g.search_last_frame_stats())
        total += cnt
    assert total > 1000


def test_search_for_initialization(orb, frame, poked):
    import torch
    total = 0
    for name, c, g in handle_cases(orb, "search_init", frame, poked, angle=True):
        F1, F2, prm = c["F1"], grid_ints(c["F2"]), plain(c["prm"])
        pm = _dev(np.ascontiguousarray(c["prev"], np.float32))
        m12, m21, cnt = g.search_for_initialization(_dev(F1["octave"]), _dev(F1["angle"]), _dev(F1["desc"]), pm, init_params(orb, F2, prm))
        torch.cuda.synchronize()
        o, ctr = c["out"], c["counters"]
        assert np.array_equal(m12.cpu().numpy(), o["matches12"]) and int(cnt.item()) == int(o["nmatches"]), name
        assert int(cnt.item()) > 50 or not cases.is_real(name), name
        assert np.array_equal(pm.cpu().numpy().view(np.uint32), np.asarray(o["prev"], np.float32).reshape(2, -1).view(np.uint32)), name
        # candidates, displaced claims and the kept bins are the transcription's trace; rounds and overflowed lists exist only in the kernels'
        # formulation and are the restatement's on the same inputs
        want = (int(ctr["rounds"]), int(ctr["candidates"]), int(ctr["overflow"]), int(ctr["displaced"]), tuple(int(v) for v in ctr["ind"]))
        st = g.search_for_initialization_stats()
        assert (st[0], st[1], st[2], st[3], tuple(st[4])) == want, (name, st, want)
        total += int(cnt.item())
    assert total > 500


def test_search_by_projection_kf(orb, frame, poked):
    """every case through handle_cases (the extracted frames and the POKE handle), both call forms: kp_match as slot numbers, the count and the
    statistics.  The device gets the slots the caller would hand it (a live point that is not already found).  A stated difference
    (ref_matcher_cases.STATED_DIFFERENCES) is asserted at the contract's value."""
    import torch
    m = cases.MATCHERS["search_kf"]
    total = 0
    for name, c, g in handle_cases(orb, "search_kf", frame, poked, angle=True):
        F, prm = cases.kf_frame(c), cases.kf_prm(c)
        P, idx = cases.kf_live(c)
        blocked = _dev(np.asarray(F["blocked"], np.uint8))
        stated = cases.STATED_DIFFERENCES.get(("search_kf", name), {})
        want = np.where(c["out"]["kp_match"] == -2, -1, c["out"]["kp_match"])
        count = int(c["out"]["nmatches"])
        if "contract" in stated:
            k = len(stated["contract"]["kp_match"])
            want = np.concatenate([stated["contract"]["kp_match"], np.full(len(want) - k, -1)])
            count = stated["contract"]["nmatches"]
        ctr = c["counters"]
        for sync in (False, True):
            args = [_dev(P[k]) for k in KF_POINT_KEYS]
            if sync:
                km, cnt = g.search_by_projection_kf_host(*args, kf_c_params(orb, F, prm), blocked=blocked)
            else:
                mk, md, km, cnt = g.search_by_projection_kf(*args, kf_c_params(orb, F, prm), blocked=blocked)
                torch.cuda.synchronize()
                km, cnt = km.cpu().numpy(), int(cnt.cpu().numpy()[0])
            km = np.asarray(km, np.int64)
            slots = np.where(km >= 0, idx[np.maximum(km, 0)] if len(idx) else -1, -1)
            assert np.array_equal(slots, want) and cnt == count, (name, sync)
            st = g.search_by_projection_kf_stats()
            assert st == (int(ctr["rounds"]), int(ctr["candidates"]), int(ctr["overflow"]), tuple(int(v) for v in ctr["ind"])), (name, st)
        assert cnt > 100 or not cases.is_real(name), name
        total += cnt
    assert total > 1000


def test_search_by_bow(orb, configs):
    import torch
    c2 = configs["c2"]
    g = _mk(orb, c2)
    g.extract(synth_stereo_pair(REAL_SEED, c2["h"], c2["w"])[0])
    N = g.n_keypoints()
    golden = rm.load_golden("search_by_bow")
    assert N >= max(len(c["F"]["node"]) for c in golden.values())
    for name, c in golden.items():
        KF, F, prm = c["KF"], c["F"], plain(c["prm"])
        n = len(F["node"])
        if n:
            poke_frame(orb, g, F["desc"], F["angle"])
        Fp = padded(dict(F, node=np.asarray(F["node"], np.int32)), N)
        want, ctr = c["out"]["match_kf"], c["counters"]
        stats = (int(ctr["node_pairs"]), int(ctr["distances"]), int(ctr["largest_node"]), tuple(int(v) for v in ctr["ind"]))
        for sync in (False, True):
            start, *arrs = concat_bow([KF])
            fn = _dev(Fp["node"].astype(np.int32))
            if sync:
                mk, cnt = g.search_by_bow_host(start, *arrs, bow_params(orb, prm), f_node=fn)
            else:
                mk, cnt = g.search_by_bow(start, *arrs, bow_params(orb, prm), f_node=fn)
                torch.cuda.synchronize()
                mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
            assert np.array_equal(mk[0][:n], want) and (mk[0][n:] == -1).all() and int(cnt[0]) == int(c["out"]["nmatches"]), (name, sync)
            if len(KF["node"]):
                assert g.search_by_bow_stats() == stats, (name, g.search_by_bow_stats(), stats)
    g.close()
