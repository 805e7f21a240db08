"""-m gpu: jsorb_search_by_bow_kf* (k_bow_group + k_loop_bow_match + k_tri_resolve) and jsorb_search_by_sim3* (k_fuse_grids + k_sim3_match +
k_sim3_agree) on a jsorb_keyframe_matcher against the sequential transcriptions of ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) and
ORBmatcher::SearchBySim3 and the kernels' restatements of tests/test_loop_host.py - matches, counts and statistics, bit for bit."""
import ctypes
import subprocess

import numpy as np
import pytest

import test_gpu_fuse as fuse
import test_gpu_triangulation as tri
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED, both_transforms, frame_side, sampled_voc
from test_fuse_host import keyframe, random_case as fuse_random_case, scale_tables
from test_gpu_search_local import _dev, _mk
from test_loop_host import (BOW_CONSTRUCTED, BOW_KEPT, LB_NODE_REGS, SIM3_CONSTRUCTED, bow_candidates, bow_params, bow_sides, concat_sides, node_size_case,
                            random_bow_sides, random_sim3_case, sim3_both, sim3_params, sim3_side)
from test_triangulation_host import random_case as tri_random_case

pytestmark = pytest.mark.gpu
f32 = np.float32
BOW_DT = dict(node=np.int32, valid=np.uint8, angle=np.float32, desc=np.uint8)
P_MAP = dict(Px="Px", Py="Py", Pz="Pz", max_distance="maxd", min_dist_inv="mindi", max_dist_inv="maxdi")


@pytest.fixture(scope="module")
def matcher(orb):
    m = orb.KeyframeMatcher()
    yield m
    m.close()


# ---- the two calls, each held to both host functions ----
def dev_bow(side):
    return {k: _dev(np.asarray(side[k], dt).reshape((-1, 32) if k == "desc" else (-1,))) for k, dt in BOW_DT.items()}


def bow_prm(orb, prm):
    return orb.make_bow_params(nn_ratio=float(prm["nn_ratio"]), th_low=prm["th_low"], check_orientation=prm["check_orientation"])


def check_bow(orb, m, KF1, cands, prm, sync=False, pad=0, regs=LB_NODE_REGS, host=None):
    """one device call of KF1 against the candidates, held to both host functions, statistics included; returns the host's (match12, counts, stats)"""
    cat, start = concat_sides(cands, pad)
    d1, d2 = dev_bow(KF1), dev_bow(cat)
    if sync:
        mk, cnt = m.search_by_bow_kf_host(d1, start, d2, bow_prm(orb, prm))
    else:
        mk, cnt = m.search_by_bow_kf(d1, start, d2, bow_prm(orb, prm))        # (waits for its own work)
        mk, cnt = mk.cpu().numpy(), cnt.cpu().numpy()
    if host is None:
        host = bow_candidates(KF1, cands, prm, regs)
    assert mk.shape == host[0].shape and np.array_equal(mk, host[0]) and np.array_equal(cnt, host[1]), (cnt, host[1])
    assert m.search_by_bow_kf_stats() == host[2], (m.search_by_bow_kf_stats(), host[2])
    return host


def dev_sim3(S):
    K, P = S["K"], S["P"]
    d = dict(x=_dev(K["x"]), y=_dev(K["y"]), octave=_dev(K["octave"].astype(np.int32)), kp_desc=_dev(K["desc"].reshape(-1, 32)),
             mp_desc=_dev(P["desc"].reshape(-1, 32)), search=_dev(S["search"]))
    d.update({k: _dev(np.asarray(P[v], np.float32)) for k, v in P_MAP.items()})
    d.update({k: S[k] for k in ("Rw", "tw", "sR", "t")})
    return d


def sim3_prm(orb, prm):
    return orb.make_sim3_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]),
                                (prm["inv_w"], prm["inv_h"]), float(prm["log_sf"]), prm["scale"], th=float(prm["th"]), th_high=prm["th_high"],
                                cols=prm["cols"], rows=prm["rows"])


def check_sim3(po, orb, m, S1, S2, prm, sync=False, host=None):
    """one device call, held to both host functions, statistics included; returns the host's (match1, match2, match12, nFound, trace)"""
    d1, d2 = dev_sim3(S1), dev_sim3(S2)
    if sync:
        m1, m2, m12, found = m.search_by_sim3_host(d1, d2, sim3_prm(orb, prm))
    else:
        m1, m2, m12, found = m.search_by_sim3(d1, d2, sim3_prm(orb, prm))      # (waits for its own work)
        m1, m2, m12, found = m1.cpu().numpy(), m2.cpu().numpy(), m12.cpu().numpy(), int(found.cpu()[0])
    if host is None:
        host = sim3_both(po, S1, S2, prm)
    assert np.array_equal(m1, host[0]) and np.array_equal(m2, host[1]) and np.array_equal(m12, host[2]) and found == host[3], (found, host[3])
    tr = host[4]
    want = (tr["windows"], tr["walked"], tr["distances"], tr["largest"], host[3])
    assert m.search_by_sim3_stats() == want, (m.search_by_sim3_stats(), want)
    return host


# =====================================================================================================================================
# SearchByBoW(KF, KF)
# =====================================================================================================================================
def test_bow_constructed_cases_through_the_device(orb, matcher):
    for name in sorted(BOW_CONSTRUCTED):
        (KF1, KF2), prm, want, count = BOW_CONSTRUCTED[name]
        for sync in (False, True):
            h = check_bow(orb, matcher, KF1, [KF2], prm, sync=sync)
            assert list(h[0][0]) == want and h[1][0] == count, name
            assert name not in BOW_KEPT or matcher.search_by_bow_kf_stats()[3] == tuple(BOW_KEPT[name]), name


# ---- the lane and register-cap edges: candidate nodes of 1, 63, 64, 65, 128 and 129 entries ----
@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 129])
def test_bow_node_sizes(orb, matcher, m):
    assert orb.loop_build_caps() == LB_NODE_REGS
    KF1, KF2 = node_size_case(m)
    for rot in (0, 1):
        h = check_bow(orb, matcher, KF1, [KF2], bow_params(check_orientation=rot), sync=bool(rot))
        assert h[2][2] == m and (rot or h[0][0][0] == m - 1)


# ---- 65 (and 129) entries again with one register entry per lane: the entries beyond 64 take the loop that reads them and their matched bytes ----
@pytest.mark.parametrize("m", [65, 129])
def test_bow_node_sizes_under_the_lowered_cap(orb, monkeypatch, m):
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_loop_wave", *jb.VARIANTS["tiny_loop_wave"])))
    assert orb.loop_build_caps() == 1                                       # the library in use is the build the test means
    mt = orb.KeyframeMatcher()
    KF1, KF2 = node_size_case(m)
    for rot in (0, 1):
        h = check_bow(orb, mt, KF1, [KF2], bow_params(check_orientation=rot), sync=bool(rot), regs=1)
        assert h[2][2] == m and (rot or h[0][0][0] == m - 1)            # KF1's first keypoint claims the last entry: an overflow entry
    mt.close()


# ---- 0, 1, 3 and 256 candidates of at most a dozen keypoints, an empty one in the middle, kf_start[0] > 0 ----
@pytest.mark.parametrize("n_kf", [0, 1, 3, 256])
def test_bow_candidate_counts(orb, matcher, n_kf):
    rng = np.random.default_rng(100 + n_kf)
    KF1 = random_bow_sides(rng, 40, 0, n_nodes=4)[0]
    cands = []
    for i in range(n_kf):
        n2 = 0 if i == 1 else int(rng.integers(1, 13))
        K2 = random_bow_sides(rng, 0, n2, n_nodes=4)[1]
        src = rng.integers(0, 40, n2)
        K2["desc"], K2["node"] = KF1["desc"][src].copy(), KF1["node"][src].copy()      # it observes KF1's keypoints
        cands.append(K2)
    for sync in (False, True):
        h = check_bow(orb, matcher, KF1, cands, bow_params(check_orientation=int(sync)), sync=sync, pad=5)
    if n_kf >= 3:
        assert h[1][1] == 0 and h[1].sum() > 0


# ---- real frames: two extracts of a synthetic stereo pair through the BoW transform with a sampled vocabulary ----
def real_sides(orb, c, rng):
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    frames = []
    for img in (left, right):
        g.extract(img)
        kp = g.keypoints()
        s = frame_side(kp, g.descriptors())
        n = len(s["angle"])
        s.update(x=kp[:n].astype(np.float32), y=kp[n:2 * n].astype(np.float32), octave=kp[4 * n:5 * n].astype(np.int32),
                 valid=(rng.random(n) < 0.9).astype(np.uint8))
        frames.append(s)
    return frames


def test_bow_real_frames(orb, configs, matcher):
    c = configs["tiny"]
    L, R = real_sides(orb, c, np.random.default_rng(12))
    tree = sampled_voc(L["desc"])
    voc = orb.Vocabulary(tree, levels_up=1)
    for s in (L, R):
        s["node"] = orb.bow_transform_descriptors(voc, _dev(s["desc"]))[1].cpu().numpy()
        assert np.array_equal(s["node"], both_transforms(tree, s["desc"], 1)[1])
    empty = bow_sides([], [])[0]
    for ratio, rot in ((0.75, 1), (0.75, 0), (0.9, 1)):
        h = check_bow(orb, matcher, L, [R, empty, L], bow_params(nn_ratio=f32(ratio), check_orientation=rot), sync=bool(rot), pad=3)
        assert h[1][0] >= 5 and h[1][2] > h[1][0] and h[2][0] > 10, (ratio, rot, h[1], h[2])


# =====================================================================================================================================
# SearchBySim3
# =====================================================================================================================================
def test_sim3_constructed_cases_through_the_device(po, orb, matcher):
    for name in sorted(SIM3_CONSTRUCTED):
        (S1, S2, prm), m1, m2, m12 = SIM3_CONSTRUCTED[name]
        for sync in (False, True):
            h = check_sim3(po, orb, matcher, S1, S2, prm, sync=sync)
            assert list(h[0]) == m1 and list(h[1]) == m2 and list(h[2]) == m12, name


# ---- n1 of 1, 15, 16, 17 and 257 against a keyframe of about 150 keypoints: the group, wave and workgroup edges of both kernels ----
@pytest.mark.parametrize("n1", [1, 15, 16, 17, 257])
def test_sim3_slot_counts(po, orb, matcher, n1):
    S1, S2, prm = random_sim3_case(np.random.default_rng(40 + n1), n1=n1, n2=150, s12=1.1)
    S1["search"][-1] = 1                                                     # the last slot of the last group is searched
    for sync in (False, True):
        h = check_sim3(po, orb, matcher, S1, S2, prm, sync=sync)
    assert (h[1] >= 0).sum() >= 1 and (n1 < 15 or (h[0] >= 0).sum() >= 1)


def test_sim3_real_frames(po, orb, configs, matcher):
    c = configs["tiny"]
    L, R = real_sides(orb, c, np.random.default_rng(13))
    s = scale_tables(c["L"])[0]
    prm = sim3_params(fx=f32(c["fx"]), fy=f32(c["fx"]), cx=f32(c["w"] / 2), cy=f32(c["h"] / 2), max_x=f32(c["w"]), max_y=f32(c["h"]), scale=s)
    base = c["bf"] / c["fx"]
    eye = np.eye(3, dtype=np.float32).ravel()
    sides = []
    # the left camera at the origin, the right one a baseline to its right; every keypoint carries a map point at depth 4 with its own descriptor;
    # the similarity between the cameras is the baseline itself, slightly off, with a scale near 1
    for F, tw, s_other, t_other in ((L, [0, 0, 0], 1 / 1.02, [-base / 1.02 + 0.002, 0.001, 0]), (R, [-base, 0, 0], 1.02, [base - 0.002, -0.001, 0])):
        K = keyframe(F["x"], F["y"], F["octave"], F["desc"], prm)
        pose = (eye, np.asarray(tw, np.float32), -np.asarray(tw, np.float32))
        P = fuse.map_points_of(K, pose, prm, 4.0)
        P = {k: P[k] for k in ("Px", "Py", "Pz", "maxd", "mindi", "maxdi", "desc")}
        sides.append(sim3_side(K, P, F["valid"], dict(Rw=eye, tw=pose[1], sR=f32(s_other) * eye, t=np.asarray(t_other, np.float32))))
    for sync in (False, True):
        h = check_sim3(po, orb, matcher, sides[0], sides[1], prm, sync=sync)
    assert h[3] >= 5 and h[4]["windows"] > 20, (h[3], dict(h[4]))


# =====================================================================================================================================
# both
# =====================================================================================================================================
def test_twenty_calls_with_changing_sizes(po, orb):
    m = orb.KeyframeMatcher()
    rng = np.random.default_rng(77)
    for call in range(20):
        n1, n_kf = int(rng.choice([0, 3, 60, 200])), int(rng.choice([1, 2, 5]))
        KF1 = random_bow_sides(rng, n1, 0, n_nodes=3)[0]
        cands = []
        for _ in range(n_kf):
            n2 = int(rng.choice([0, 7, 90, 300]))
            K2 = random_bow_sides(rng, 0, n2, n_nodes=3)[1]
            if n1 and n2:
                src = rng.integers(0, n1, n2)
                K2["desc"], K2["node"] = KF1["desc"][src].copy(), KF1["node"][src].copy()
            cands.append(K2)
        check_bow(orb, m, KF1, cands, bow_params(check_orientation=call % 2), sync=call % 3 == 0, pad=int(rng.choice([0, 9])))
        S1, S2, prm = random_sim3_case(rng, n1=int(rng.choice([0, 5, 40, 130])), n2=int(rng.choice([0, 9, 120])))
        check_sim3(po, orb, m, S1, S2, prm, sync=call % 3 == 1)
    m.close()


def test_async_on_an_external_stream(po, orb):
    import torch
    m = orb.KeyframeMatcher()
    own = m.get_stream()
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    assert m.get_stream() == st.cuda_stream
    rng = np.random.default_rng(5)
    KF1, KF2 = random_bow_sides(rng, 150, 170, n_nodes=6)
    cat, start = concat_sides([KF2])
    S1, S2, prm = random_sim3_case(rng, n1=90, n2=110)
    with torch.cuda.stream(st):
        d1, d2 = dev_bow(KF1), dev_bow(cat)                          # uploaded on the stream the matcher runs on: ordered without a wait
        mk, cnt = m.search_by_bow_kf(d1, start, d2, bow_prm(orb, bow_params()), wait=False)
        e1, e2 = dev_sim3(S1), dev_sim3(S2)
        out = m.search_by_sim3(e1, e2, sim3_prm(orb, prm), wait=False)
        mk, cnt = mk.cpu(), cnt.cpu()
        out = [o.cpu().numpy() for o in out]
    st.synchronize()
    hb = bow_candidates(KF1, [KF2], bow_params())
    assert np.array_equal(mk.numpy(), hb[0]) and np.array_equal(cnt.numpy(), hb[1]) and hb[1][0] > 0 and m.search_by_bow_kf_stats() == hb[2]
    hs = sim3_both(po, S1, S2, prm)
    assert all(np.array_equal(out[k], hs[k]) for k in range(3)) and int(out[3][0]) == hs[3] > 0
    m.set_stream(None)
    assert m.get_stream() == own
    check_bow(orb, m, KF1, [KF2], bow_params(), host=hb)
    check_sim3(po, orb, m, S1, S2, prm, host=hs)
    m.close()


def test_interleaved_with_fuse_and_triangulation(po, orb):
    """the four matchers of one keyframe matcher: each one's statistics and "done" mark are its own"""
    m = orb.KeyframeMatcher()
    lib = orb.load_library()
    rng = np.random.default_rng(21)
    null5 = [None] * 5
    assert lib.jsorb_search_by_bow_kf_stats(m.handle, *null5[:4]) == -4 and lib.jsorb_search_by_sim3_stats(m.handle, *null5) == -4      # before any call
    T1, T2, geom, tprm = tri_random_case(rng, 60, 80, 5)
    tri_hosts = tri.check_search(orb, m, T1, [T2], [geom], tprm)
    tri_stats = m.stats()
    K, pose, P, fprm = fuse_random_case(rng, n=60, N=120)
    fuse_host = fuse.check_fuse(po, orb, m, [K], [pose], P, fprm)
    assert lib.jsorb_search_by_bow_kf_stats(m.handle, *null5[:4]) == -4 and lib.jsorb_search_by_sim3_stats(m.handle, *null5) == -4      # neither is a loop call
    KF1, KF2 = random_bow_sides(rng, 120, 140, n_nodes=5)
    S1, S2, sprm = random_sim3_case(rng, n1=70, n2=80)
    hb = check_bow(orb, m, KF1, [KF2, KF2], bow_params())
    assert lib.jsorb_search_by_sim3_stats(m.handle, *null5) == -4
    hs = check_sim3(po, orb, m, S1, S2, sprm)
    sim3_stats = m.search_by_sim3_stats()
    assert m.stats() == tri_stats and m.fuse_stats() == fuse_host[3] and m.search_by_bow_kf_stats() == hb[2]
    for call in range(6):
        which = call % 4
        if which == 0:
            fuse.check_fuse(po, orb, m, [K], [pose], P, fprm, sync=bool(call % 3), host=fuse_host)      # (it rebuilds the grid scratch the Sim3 search shares)
        elif which == 1:
            check_sim3(po, orb, m, S1, S2, sprm, sync=bool(call % 3), host=hs)
        elif which == 2:
            tri.check_search(orb, m, T1, [T2], [geom], tprm, sync=bool(call % 3), hosts=tri_hosts)      # (it rebuilds the sorted keys the BoW search shares)
        else:
            check_bow(orb, m, KF1, [KF2, KF2], bow_params(), sync=bool(call % 3), host=hb)
        assert m.stats() == tri_stats and m.fuse_stats() == fuse_host[3] and m.search_by_bow_kf_stats() == hb[2] and m.search_by_sim3_stats() == sim3_stats
    m.close()


def test_edges_and_validation(po, orb, matcher):
    import torch
    lib = orb.load_library()
    rng = np.random.default_rng(3)
    KF1, KF2 = random_bow_sides(rng, 50, 60, n_nodes=3)
    p = bow_prm(orb, bow_params())
    cat, start = concat_sides([KF2])
    d1, d2 = dev_bow(KF1), dev_bow(cat)
    mk = torch.zeros(2 * 50 + 8, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    p1 = [d1[k].data_ptr() for k in orb.KeyframeMatcher.BOW_KF_KEYS]
    p2 = [d2[k].data_ptr() for k in orb.KeyframeMatcher.BOW_KF_KEYS]

    def call(prm_=p, n1=50, a1=p1, nk=1, ks=start, a2=p2, o=(mk.data_ptr(), cnt.data_ptr())):
        return lib.jsorb_search_by_bow_kf_async(matcher.handle, ctypes.byref(prm_) if prm_ is not None else None, n1, *a1, nk,
                                                ks.ctypes.data if ks is not None else None, *a2, *o)
    assert call() == 0
    matcher.sync()
    assert np.array_equal(mk.cpu().numpy()[:50], bow_candidates(KF1, [KF2], bow_params())[0][0])
    assert call(prm_=None) == -1 and call(nk=-1) == -1 and call(nk=257) == -1 and call(ks=None) == -1 and call(n1=-1) == -1 and call(n1=1 << 18) == -1
    for j in range(4):
        assert call(a1=p1[:j] + [None] + p1[j + 1:]) == -1 and call(a2=p2[:j] + [None] + p2[j + 1:]) == -1, j
    assert call(a1=p1[:3] + [p1[3] + 8]) == -1 and call(a2=p2[:3] + [p2[3] + 8]) == -1            # misaligned descriptors
    assert call(o=(None, cnt.data_ptr())) == -1 and call(o=(mk.data_ptr(), None)) == -1
    assert call(ks=np.array([5, 2], np.int32)) == -1 and call(ks=np.array([-1, 2], np.int32)) == -1 and call(ks=np.array([0, 1 << 18], np.int32)) != 0
    with pytest.raises(orb.JsorbError):
        matcher.search_by_bow_kf(dict(d1, node=d1["node"].long()), start, d2, p)
    with pytest.raises(orb.JsorbError):
        matcher.search_by_bow_kf(d1, start, d2, orb.make_triangulation_params(scale_tables()[0]))
    # SearchBySim3
    S1, S2, prm = random_sim3_case(rng, n1=20, n2=30)
    e1, e2, sp = dev_sim3(S1), dev_sim3(S2), sim3_prm(orb, prm)
    s1, s2, args = matcher._sim3_args(e1, e2, sp)
    out = [torch.zeros(40, dtype=torch.int32, device="cuda") for _ in range(4)]
    ptrs = [o.data_ptr() for o in out]
    assert lib.jsorb_search_by_sim3_async(matcher.handle, *args, *ptrs) == 0
    matcher.sync()
    assert lib.jsorb_search_by_sim3_async(matcher.handle, None, args[1], args[2], *ptrs) == -1
    assert lib.jsorb_search_by_sim3_async(matcher.handle, args[0], None, args[2], *ptrs) == -1
    for j in range(4):
        assert lib.jsorb_search_by_sim3_async(matcher.handle, *args, *(ptrs[:j] + [None] + ptrs[j + 1:])) == -1, j
    for field, bad in (("th_high", 256), ("th_high", -1), ("n_levels", 0), ("n_levels", 17), ("cols", 0), ("cols", 4097)):
        q = sim3_prm(orb, prm)
        setattr(q, field, bad)
        assert lib.jsorb_search_by_sim3_async(matcher.handle, ctypes.byref(q), args[1], args[2], *ptrs) == -1, field
    for key in orb.KeyframeMatcher.SIM3_KEYS:
        bad = orb.JsorbSim3Side.from_buffer_copy(s1)
        setattr(bad, key, None)
        assert lib.jsorb_search_by_sim3_async(matcher.handle, args[0], ctypes.byref(bad), args[2], *ptrs) == -1, key
    bad = orb.JsorbSim3Side.from_buffer_copy(s1)
    bad.mp_desc = s1.mp_desc + 8
    assert lib.jsorb_search_by_sim3_async(matcher.handle, args[0], ctypes.byref(bad), args[2], *ptrs) == -1
    bad = orb.JsorbSim3Side.from_buffer_copy(s1)
    bad.n = (1 << 18) - 30
    assert lib.jsorb_search_by_sim3_async(matcher.handle, args[0], ctypes.byref(bad), args[2], *ptrs) == -1
    assert b"n1 + n2" in lib.jsorb_keyframe_matcher_last_error(matcher.handle)
    with pytest.raises(orb.JsorbError):
        matcher.search_by_sim3(dict(e1, octave=e1["octave"].long()), e2, sp)
    with pytest.raises(orb.JsorbError):
        matcher.search_by_sim3(dict(e1, sR=np.zeros(8, np.float32)), e2, sp)


# ---- the C++ example through the compat shim: ComputeSim3's loops over one keyframe and three candidates, checked against its own sequential loops ----
def test_compute_sim3_example(orb, configs, tmp_path):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("compute_sim3", str(tmp_path / "compute_sim3"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    other = synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[1]
    images = [left, right, left, other]
    g = _mk(orb, c)
    g.extract(left)
    tree = sampled_voc(frame_side(g.keypoints(), g.descriptors())["desc"])
    paths = [str(tmp_path / ("kf%d.raw" % i)) for i in range(4)]
    for img, p in zip(images, paths):
        img.tofile(p)
    vp, op = str(tmp_path / "vocabulary.bin"), str(tmp_path / "out.bin")
    with open(vp, "wb") as f:
        f.write(np.array([tree["n_nodes"], tree["depth_L"], 1], np.int32).tobytes())
        for key in ("child_start", "children", "descriptors", "word_id", "weight"):
            f.write(np.ascontiguousarray(tree[key]).tobytes())
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"])] + paths + [vp, op], timeout=300, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stderr + out.stdout
    blob = np.fromfile(op, np.int32)
    n1, ns, nmatches, found = int(blob[0]), blob[1:4], blob[4:7], blob[7:10]
    assert n1 == g.n_keypoints() and len(blob) == 10 + 6 * n1
    # the candidate that is the current keyframe's own image keeps the most BoW matches (and leaves SearchBySim3 little to add); the unrelated image
    # keeps fewer than 20 and is discarded before SearchBySim3 (LoopClosing.cpp:272-276)
    assert nmatches[1] > nmatches[0] >= 20 > nmatches[2] and found[0] >= 1 and found[1] >= 0 and found[2] == -1, (nmatches, found)
    # the BoW rows through the Python path
    sides_ = []
    for img in images:
        g.extract(img)
        s = frame_side(g.keypoints(), g.descriptors())
        n = len(s["angle"])
        s.update(valid=(np.arange(n) % 5 != 4).astype(np.uint8), node=both_transforms(tree, s["desc"], 1)[1])
        sides_.append(s)
    h = bow_candidates(sides_[0], sides_[1:], bow_params())
    assert list(h[1]) == list(nmatches)
    for k in range(3):
        assert np.array_equal(blob[10 + 2 * k * n1:10 + (2 * k + 1) * n1], h[0][k]), k
        row = blob[10 + (2 * k + 1) * n1:10 + (2 * k + 2) * n1]
        assert (row >= 0).sum() == max(found[k], 0) and not ((row >= 0) & (h[0][k] >= 0)).any()      # SearchBySim3 searches only what BoW left unmatched
