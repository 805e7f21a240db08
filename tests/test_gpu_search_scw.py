"""-m gpu: jsorb_search_by_projection_sim3* (k_fuse_grids + k_scw_candidates + k_scw_resolve) on a jsorb_keyframe_matcher against the sequential
transcription of ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cpp:277-390) and the kernels' restatement of
tests/scw_cases.py - match_kp, match_dist, kp_match, the count and every statistics word, bit for bit, in the synchronous and the asynchronous
form, with the shipped caps and under the tiny_scw_cap build (2 keys a point, 64 claims in LDS)."""
import ctypes
import subprocess

import numpy as np
import pytest

import scw_cases as sc
import test_gpu_fuse as fuse
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED, frame_side, sampled_voc
from test_fuse_host import keyframe, random_case as fuse_random_case, scale_tables
from test_gpu_loop import check_sim3
from test_gpu_search_local import _dev, _mk
from test_loop_host import random_sim3_case

pytestmark = pytest.mark.gpu
f32 = np.float32
P_MAP = dict(Px="Px", Py="Py", Pz="Pz", Nx="Nx", Ny="Ny", Nz="Nz", max_distance="maxd", min_dist_inv="mindi", max_dist_inv="maxdi")
CONSTRUCTED = sc.constructed()


@pytest.fixture(scope="module")
def matcher(orb):
    m = orb.KeyframeMatcher()
    yield m
    m.close()


@pytest.fixture
def tiny(orb, monkeypatch):
    """the tiny_scw_cap build as the library behind `orb`, and a matcher of it"""
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_scw_cap", *jb.VARIANTS["tiny_scw_cap"])))
    assert orb.scw_build_caps() == sc.TINY                                 # the library in use is the build the test means
    m = orb.KeyframeMatcher()
    yield m
    m.close()


def scw_prm(orb, prm, pose):
    return orb.scw_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]),
                          (prm["inv_w"], prm["inv_h"]), float(prm["log_sf"]), prm["scale"], *pose, th=float(prm["th"]), th_low=prm["th_low"],
                          cols=prm["cols"], rows=prm["rows"])


def dev_sides(K, Pd, blocked):
    pts = {k: _dev(np.asarray(Pd[v], np.float32)) for k, v in P_MAP.items()}
    pts["desc"] = _dev(np.asarray(Pd["desc"], np.uint8).reshape(-1, 32))
    kf = dict(x=_dev(np.asarray(K["x"], np.float32)), y=_dev(np.asarray(K["y"], np.float32)), octave=_dev(np.asarray(K["octave"], np.int32)),
              desc=_dev(np.asarray(K["desc"], np.uint8).reshape(-1, 32)), blocked=None if blocked is None else _dev(np.asarray(blocked, np.uint8)))
    return pts, kf


def check_scw(po, orb, m, c, sync=False, cap=sc.SC_CAP, host=None):
    """one device call of a case, held to both host functions, statistics included; returns (transcription, restatement at the cap)"""
    if host is None:
        ref, res = sc.both(po, c, caps=(cap,))
        host = (ref, res[cap])
    ref, res = host
    K, pose, Pd, blocked, sel = sc.device_inputs(c)
    pts, kf = dev_sides(K, Pd, blocked)
    out = m.search_by_projection_sim3(pts, kf, scw_prm(orb, sc.params_of(c), pose), sync=sync)
    if sync:
        mk, md, km, cnt = out
    else:
        mk, md, km, cnt = (o.cpu().numpy() for o in out)
        cnt = int(cnt[0])
    assert mk.shape == (len(sel),) and km.shape == (len(K["x"]),)
    assert np.array_equal(mk, res[0]) and np.array_equal(md, res[1]) and np.array_equal(km, res[2]) and cnt == res[3] == ref[1], (cnt, res[3])
    assert np.array_equal(sc.matched_out(c, sel, km), ref[0])              # vpMatched after the call, as the reference leaves it
    assert m.search_by_projection_sim3_stats() == res[4], (m.search_by_projection_sim3_stats(), res[4])
    return host


def both_forms(po, orb, m, c, cap=sc.SC_CAP):
    host = check_scw(po, orb, m, c, sync=False, cap=cap)
    return check_scw(po, orb, m, c, sync=True, cap=cap, host=host)


def test_constructed_cases_through_the_device(po, orb, matcher):
    assert orb.scw_build_caps() == (sc.SC_CAP, sc.SC_LDS_CLAIMS)
    for name, (c, want, count) in CONSTRUCTED.items():
        ref, _ = both_forms(po, orb, matcher, c)
        assert list(ref[0]) == want and ref[1] == count, name


@pytest.mark.parametrize("seed", sc.BLOCK_SEEDS)
def test_random_blocks(po, orb, matcher, seed):
    ref, res = both_forms(po, orb, matcher, sc.block(seed))
    assert ref[1] >= 50 and res[4][0] >= 4 and res[4][2] == 0


@pytest.mark.parametrize("n", sc.POINT_COUNTS)
def test_point_counts(po, orb, matcher, n):
    both_forms(po, orb, matcher, sc.count_case(n))


def test_under_the_lowered_caps(po, orb, tiny):
    """2 keys a point: the overflow walk; 64 claims in LDS: claim[] in global memory for the keyframes of 70 and 150 keypoints, in LDS for the
    constructed ones"""
    for name, (c, want, count) in CONSTRUCTED.items():
        ref, _ = both_forms(po, orb, tiny, c, cap=sc.TINY[0])
        assert list(ref[0]) == want and ref[1] == count, name
    over = 0
    for c in [sc.block(s) for s in sc.BLOCK_SEEDS] + [sc.count_case(n) for n in sc.POINT_COUNTS]:
        assert len(c["K"]["x"]) > sc.TINY[1]
        _, res = both_forms(po, orb, tiny, c, cap=sc.TINY[0])
        over += res[4][2]
    assert over >= 300
    # exactly 64 and 65 keypoints: the last size in LDS and the first in global memory
    for N in (64, 65):
        c = sc.random_block(np.random.default_rng(9300 + N), n=40, N=N, n_clusters=4, skips=False)
        _, res = both_forms(po, orb, tiny, c, cap=sc.TINY[0])
        assert res[3] >= 5 and res[4][2] >= 1


def real_case(orb, c, rng, s=1.02):
    """one extracted frame as the current keyframe; its keypoints back-projected at depth 4 as the loop points, in a shuffled order with a tenth of them
    bad; a third of the keypoints hold a point before the call, some of them loop points"""
    left, _ = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    kp = g.keypoints()
    F = frame_side(kp, g.descriptors())
    n = len(F["angle"])
    prm = sc.tf.default_params(check=0, th=f32(10), fx=f32(c["fx"]), fy=f32(c["fx"]), cx=f32(c["w"] / 2), cy=f32(c["h"] / 2), max_x=f32(c["w"]),
                               max_y=f32(c["h"]), scale=scale_tables(c["L"])[0])
    K = keyframe(kp[:n].astype(np.float32), kp[n:2 * n].astype(np.float32), kp[4 * n:5 * n].astype(np.int32), F["desc"], prm)
    pose = fuse.shifted([0.02, -0.01, 0.03])
    P = fuse.map_points_of(K, pose, prm, 4.0)
    P["mind"] = (P["maxd"] / prm["scale"][-1]).astype(np.float32)
    m = n // 3
    holders = rng.permutation(n)[:m]
    matched_in = np.full(n, -1, np.int32)
    matched_in[holders[:10]] = rng.permutation(n)[:10]
    matched_in[holders[10:]] = n + np.arange(m - 10)
    full = {k: np.concatenate([np.asarray(v), np.zeros((m - 10,) + np.shape(v)[1:], np.asarray(v).dtype)]) for k, v in P.items()}
    full["bad"] = np.concatenate([(rng.random(n) < 0.1).astype(np.uint8), np.zeros(m - 10, np.uint8)])
    return sc.make_case(prm, K, full, lst=rng.permutation(n), matched_in=matched_in, pose=pose, s=s)


def test_a_real_frame(po, orb, configs, matcher):
    c = real_case(orb, configs["c1"], np.random.default_rng(14))
    assert len(c["K"]["x"]) > 300
    ref, res = both_forms(po, orb, matcher, c)
    tr = ref[4]
    assert ref[1] >= 100 and tr["blocked_met"] >= 100 and tr["bad_skipped"] >= 10 and 5 <= tr["found_skipped"] <= 10, (ref[1], dict(tr))


def test_a_real_frame_under_the_lowered_caps(po, orb, configs, tiny):
    c = real_case(orb, configs["c1"], np.random.default_rng(15))
    _, res = both_forms(po, orb, tiny, c, cap=sc.TINY[0])
    assert res[4][2] >= 1


def sized_case(rng, n, N):
    if n and N:
        return sc.random_block(rng, n=n, N=N, n_clusters=max(1, N // 12), skips=bool(n % 2))
    prm = sc.tf.default_params(check=0, th=f32(10))                        # an empty side: n points at one pixel, N keypoints in a row
    at = sc.tf.points_at([(100, 100)] * n, prm)
    P = dict(at, Nx=np.zeros(n, np.float32), Ny=np.zeros(n, np.float32), Nz=np.ones(n, np.float32))
    return sc.make_case(prm, sc.tf.kps([(100 + 3 * i, 100, 0, 10) for i in range(N)], prm), P)


def test_twenty_calls_with_changing_sizes(po, orb):
    m = orb.KeyframeMatcher()
    rng = np.random.default_rng(78)
    for call in range(20):
        n, N = int(rng.choice([0, 1, 30, 120, 300])), int(rng.choice([0, 5, 66, 200]))
        check_scw(po, orb, m, sized_case(rng, n, N), sync=call % 3 == 0)
    m.close()


def test_async_on_an_external_stream(po, orb):
    import torch
    m = orb.KeyframeMatcher()
    own = m.get_stream()
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    c = sc.block(sc.BLOCK_SEEDS[0])
    ref, res = sc.both(po, c, caps=(sc.SC_CAP,))
    K, pose, Pd, blocked, sel = sc.device_inputs(c)
    with torch.cuda.stream(st):
        pts, kf = dev_sides(K, Pd, blocked)                          # uploaded on the stream the matcher runs on: ordered without a wait
        out = m.search_by_projection_sim3(pts, kf, scw_prm(orb, sc.params_of(c), pose), wait=False)
        out = [o.cpu().numpy() for o in out]
    st.synchronize()
    r = res[sc.SC_CAP]
    assert all(np.array_equal(out[k], r[k]) for k in range(3)) and int(out[3][0]) == r[3] > 0
    m.set_stream(None)
    assert m.get_stream() == own
    check_scw(po, orb, m, c, host=(ref, r))
    m.close()


def test_interleaved_with_fuse_and_search_by_sim3(po, orb):
    """the three calls share the matcher's grid scratch; each one's statistics and "done" mark are its own"""
    m = orb.KeyframeMatcher()
    lib = orb.load_library()
    rng = np.random.default_rng(22)
    null6 = [None] * 6
    assert lib.jsorb_search_by_projection_sim3_stats(m.handle, *null6) == -4                    # before any call
    K, pose, P, fprm = fuse_random_case(rng, n=60, N=120)
    fuse_host = fuse.check_fuse(po, orb, m, [K], [pose], P, fprm)
    S1, S2, sprm = random_sim3_case(rng, n1=70, n2=80)
    hs = check_sim3(po, orb, m, S1, S2, sprm)
    sim3_stats = m.search_by_sim3_stats()
    assert lib.jsorb_search_by_projection_sim3_stats(m.handle, *null6) == -4                    # neither is this call
    c = sc.block(sc.BLOCK_SEEDS[2])
    host = check_scw(po, orb, m, c)
    scw_stats = m.search_by_projection_sim3_stats()
    assert m.fuse_stats() == fuse_host[3] and m.search_by_sim3_stats() == sim3_stats
    for call in range(6):
        which = call % 3
        if which == 0:
            fuse.check_fuse(po, orb, m, [K], [pose], P, fprm, sync=bool(call % 2), host=fuse_host)
        elif which == 1:
            check_scw(po, orb, m, c, sync=bool(call % 2), host=host)
        else:
            check_sim3(po, orb, m, S1, S2, sprm, sync=bool(call % 2), host=hs)
        assert m.fuse_stats() == fuse_host[3] and m.search_by_sim3_stats() == sim3_stats and m.search_by_projection_sim3_stats() == scw_stats
    m.close()


def test_edges_and_validation(po, orb, matcher):
    import torch
    lib = orb.load_library()
    c = sc.count_case(17)
    K, pose, Pd, blocked, sel = sc.device_inputs(c)
    pts, kf = dev_sides(K, Pd, blocked)
    n, N = len(sel), len(K["x"])
    p = scw_prm(orb, sc.params_of(c), pose)
    out = [torch.zeros(N + 8, dtype=torch.int32, device="cuda") for _ in range(4)]
    ptrs = [o.data_ptr() for o in out]
    pp = [pts[k].data_ptr() for k in orb.KeyframeMatcher.POINT_KEYS]
    pk = [kf[k].data_ptr() for k in orb.KeyframeMatcher.SCW_KF_KEYS]

    def call(prm_=p, n_=n, a1=pp, N_=N, a2=pk, o=ptrs):
        return lib.jsorb_search_by_projection_sim3_async(matcher.handle, ctypes.byref(prm_) if prm_ is not None else None, n_, *a1, N_, *a2, *o)
    assert call() == 0
    matcher.sync()
    ref, res = sc.both(po, c, caps=(sc.SC_CAP,))
    assert np.array_equal(out[0].cpu().numpy()[:n], ref[2]) and int(out[3].cpu()[0]) == ref[1]
    assert call(prm_=None) == -1 and call(n_=-1) == -1 and call(N_=-1) == -1 and call(N_=1 << 18) == -1
    assert b"n_keypoints" in lib.jsorb_keyframe_matcher_last_error(matcher.handle)
    for j in range(10):
        assert call(a1=pp[:j] + [None] + pp[j + 1:]) == -1, j
    for j in range(4):
        assert call(a2=pk[:j] + [None] + pk[j + 1:]) == -1, j
    assert call(a2=pk[:4] + [None]) == 0                                   # blocked may be NULL
    matcher.sync()
    assert call(a1=pp[:9] + [pp[9] + 8]) == -1 and call(a2=pk[:3] + [pk[3] + 8, pk[4]]) == -1      # misaligned descriptors
    for j in range(4):
        assert call(o=ptrs[:j] + [None] + ptrs[j + 1:]) == -1, j
    for field, bad in (("th_low", 256), ("th_low", -1), ("n_levels", 0), ("n_levels", 17), ("cols", 0), ("cols", 4097), ("rows", 0)):
        q = scw_prm(orb, sc.params_of(c), pose)
        setattr(q, field, bad)
        assert call(prm_=q) == -1, field
    # empty sides are valid calls: -1 / 0, nothing launched
    for o in out:
        o.fill_(-7)
    assert call(n_=0) == 0
    matcher.sync()
    assert (out[2].cpu().numpy()[:N] == -1).all() and int(out[3].cpu()[0]) == 0 and (out[0].cpu().numpy() == -7).all()
    assert matcher.search_by_projection_sim3_stats() == (0, 0, 0, 0, 0, 0)
    assert call(N_=0) == 0
    matcher.sync()
    assert (out[0].cpu().numpy()[:n] == -1).all() and (out[1].cpu().numpy()[:n] == -1).all() and int(out[3].cpu()[0]) == 0
    with pytest.raises(orb.JsorbError):
        matcher.search_by_projection_sim3(dict(pts, Px=pts["Px"].double()), kf, p)
    with pytest.raises(orb.JsorbError):
        matcher.search_by_projection_sim3(pts, kf, orb.make_bow_params())


# ---- the C++ example through the compat shim: ComputeSim3 to its end, checked against its own sequential loops ----
def test_compute_sim3_example_reaches_the_acceptance_test(orb, configs, tmp_path):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("compute_sim3", str(tmp_path / "compute_sim3"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    other = synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[1]
    g = _mk(orb, c)
    g.extract(left)
    tree = sampled_voc(frame_side(g.keypoints(), g.descriptors())["desc"])
    paths = [str(tmp_path / ("kf%d.raw" % i)) for i in range(4)]
    for img, p in zip([left, right, left, other], paths):
        img.tofile(p)
    vp, op = str(tmp_path / "vocabulary.bin"), str(tmp_path / "out.bin")
    with open(vp, "wb") as f:
        f.write(np.array([tree["n_nodes"], tree["depth_L"], 1], np.int32).tobytes())
        for key in ("child_start", "children", "descriptors", "word_id", "weight"):
            f.write(np.ascontiguousarray(tree[key]).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"])] + paths + [vp, op], timeout=300, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stderr + out.stdout
    line = [l for l in out.stdout.splitlines() if l.startswith("scw ")]
    assert len(line) == 1, out.stdout
    f = dict(kv.split("=") for kv in line[0].split()[1:])
    blob = np.fromfile(op, np.int32)
    n1 = int(blob[0])
    before = int(((blob[10:10 + n1] >= 0) | (blob[10 + n1:10 + 2 * n1] >= 0)).sum())      # candidate 0's BoW and Sim3 matches: mvpCurrentMatchedPoints
    assert int(f["candidate"]) == 0 and int(f["loop_points"]) > n1 and int(f["nmatches"]) >= 1
    assert int(f["nTotalMatches"]) == before + int(f["nmatches"]) and f["loop"] == ("accepted" if int(f["nTotalMatches"]) >= 40 else "rejected")
