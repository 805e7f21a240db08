"""GPU: jsorb_fuse* (k_fuse_grids, k_fuse_match) against the two host functions of tests/test_fuse_host.py - the sequential transcription of
ORBmatcher::Fuse's search and the restatement of the kernels, which must agree with each other first.  Every test compares best_idx, best_dist, the
per-keyframe counts and the statistics bit for bit."""
import ctypes
import subprocess
import threading

import numpy as np
import pytest

import test_gpu_triangulation as tri
from jetson_slam_amd.synth import synth_stereo_pair
from test_bow_host import REAL_SEED
from test_fuse_host import (CONSTRUCTED, FUSE_KF_CHUNK, IDENTITY, default_params, fuse_keyframes, keyframe, observe, random_case, random_keyframe, random_pose,
                            scale_tables)
from test_gpu_search_local import _dev, _mk
from test_triangulation_host import random_case as tri_random_case

pytestmark = pytest.mark.gpu
f32 = np.float32
POINT_MAP = dict(Px="Px", Py="Py", Pz="Pz", Nx="Nx", Ny="Ny", Nz="Nz", max_distance="maxd", min_dist_inv="mindi", max_dist_inv="maxdi")


def fuse_params(orb, prm):
    return orb.make_fuse_params((prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]),
                                (prm["inv_w"], prm["inv_h"]), float(prm["log_sf"]), prm["scale"], prm["inv_sigma2"], th=float(prm["th"]),
                                th_low=prm["th_low"], check_reprojection=prm["check"], bf=float(prm["bf"]), cols=prm["cols"], rows=prm["rows"])


def dev_points(P):
    d = {k: _dev(np.asarray(P[v], np.float32)) for k, v in POINT_MAP.items()}
    d["desc"] = _dev(np.asarray(P["desc"], np.uint8).reshape(-1, 32))
    return d


def concat(kfs, lead=0):
    """the keyframes as the concatenated arrays of jsorb_fuse_async, behind `lead` entries that belong to no keyframe (kf_start[0] = lead); uright
    None when every keyframe is monocular"""
    start = (lead + np.cumsum([0] + [len(k["x"]) for k in kfs])).astype(np.int32)
    pad = lambda dt, w=(): np.full((lead,) + w, 77, dt)
    cat = dict(x=np.concatenate([pad(np.float32)] + [k["x"] for k in kfs]), y=np.concatenate([pad(np.float32)] + [k["y"] for k in kfs]),
               octave=np.concatenate([pad(np.int32)] + [k["octave"] for k in kfs]).astype(np.int32),
               desc=np.concatenate([pad(np.uint8, (32,))] + [k["desc"].reshape(-1, 32) for k in kfs]))
    cat["uright"] = None
    if any(k["uright"] is not None for k in kfs):
        cat["uright"] = np.concatenate([pad(np.float32)] + [k["uright"] if k["uright"] is not None else np.full(len(k["x"]), -1, np.float32) for k in kfs])
    return start, cat


def dev_keyframes(cat):
    d = {k: _dev(cat[k]) for k in ("x", "y", "octave", "desc")}
    d["uright"] = None if cat["uright"] is None else _dev(cat["uright"])
    return d


def pose_arrays(poses):
    n = len(poses)
    return (np.array([p[0] for p in poses], np.float32).reshape(n, 9), np.array([p[1] for p in poses], np.float32).reshape(n, 3),
            np.array([p[2] for p in poses], np.float32).reshape(n, 3))


def check_fuse(po, orb, m, kfs, poses, P, prm, skip=None, sync=False, lead=0, host=None):
    """one device call of the points against the keyframes, held to both host functions, statistics included; returns the host's results"""
    start, cat = concat(kfs, lead)
    R, t, O = pose_arrays(poses)
    dp, dk = dev_points(P), dev_keyframes(cat)
    sk = None if skip is None else _dev(np.asarray(skip, np.uint8).reshape(len(kfs), -1))
    if sync:
        bi, bd, cnt = m.fuse_host(dp, start, dk, R, t, O, fuse_params(orb, prm), skip=sk)
    else:
        bi, bd, cnt = m.fuse(dp, start, dk, R, t, O, fuse_params(orb, prm), skip=sk)      # (waits for its own work)
        bi, bd, cnt = bi.cpu().numpy(), bd.cpu().numpy(), cnt.cpu().numpy()
    if host is None:
        host = fuse_keyframes(po, kfs, poses, P, prm, skip)
    n = len(P["Px"])
    assert bi.shape == (len(kfs), n) and bd.shape == (len(kfs), n)
    assert np.array_equal(bi, host[0]) and np.array_equal(bd, host[1]) and np.array_equal(cnt, host[2]), (cnt, host[2])
    assert m.fuse_stats() == host[3], (m.fuse_stats(), host[3])
    return host


@pytest.fixture(scope="module")
def matcher(orb):
    m = orb.KeyframeMatcher()
    yield m
    m.close()


# ---- 1. every constructed case of the host test, both forms ----
def test_constructed_cases_through_the_device(po, orb, matcher):
    for name in sorted(CONSTRUCTED):
        K, pose, P, prm, want = CONSTRUCTED[name]
        for sync in (False, True):
            h = check_fuse(po, orb, matcher, [K], [pose], P, prm, sync=sync)
            assert list(h[0][0]) == want, name


# ---- 2. lane and block edges: windows of 0 .. 33 candidates are constructed cases; here 1, 15, 16, 17 and 257 points (16 points per workgroup) ----
@pytest.mark.parametrize("n", [1, 15, 16, 17, 257])
def test_point_counts_at_the_workgroup_edges(po, orb, matcher, n):
    rng = np.random.default_rng(n)
    K, pose, P, prm = random_case(rng, n=n, N=150)
    h = check_fuse(po, orb, matcher, [K], [pose], P, prm, sync=bool(n % 2))
    assert n < 15 or h[2][0] > 0
    # the last point alone decides: every point but the last skipped
    skip = np.ones(n, np.uint8)
    skip[-1] = 0
    hs = check_fuse(po, orb, matcher, [K], [pose], P, prm, skip=skip)
    assert hs[0][0][-1] == h[0][0][-1] and (hs[0][0][:-1] == -1).all()


# ---- 3. 0, 1, 3 and 256 keyframes of at most a dozen keypoints, an empty one in the middle, kf_start not starting at 0 ----
@pytest.mark.parametrize("n_kf", [0, 1, 3, 256])
def test_keyframe_counts(po, orb, matcher, n_kf):
    rng = np.random.default_rng(100 + n_kf)
    prm = default_params(fx=f32(300), fy=f32(295), cx=f32(158.5), cy=f32(121.25), bf=f32(38.7))
    pose = random_pose(rng)
    first = random_keyframe(rng, prm, 12)
    P = observe(rng, first, pose, prm, 12)
    kfs, poses = [], []
    for i in range(n_kf):
        N = 0 if i == 1 else int(rng.integers(1, 13))
        K = random_keyframe(rng, prm, N)
        if N and i != 1:                                  # most keyframes see some of the first one's keypoints, in its pose
            src = rng.integers(0, 12, N)
            K = keyframe(first["x"][src], first["y"][src], first["octave"][src], first["desc"][src], prm, first["uright"][src])
        kfs.append(K)
        poses.append(pose if i % 3 else random_pose(rng, 0.01))
    assert n_kf <= FUSE_KF_CHUNK or n_kf > 2 * FUSE_KF_CHUNK
    h = None
    for sync, lead in ((False, 0), (True, 5)):
        h = check_fuse(po, orb, matcher, kfs, poses, P, prm, sync=sync, lead=lead, host=h)
    if n_kf >= 3:
        assert h[2][1] == 0 and h[2].sum() > 0


# ---- 4. grid edges: every keypoint in one cell; keypoints outside the grid ----
def test_grid_edges(po, orb, matcher):
    rng = np.random.default_rng(4)
    prm = default_params()
    n = 40
    one_cell = keyframe(100 + rng.uniform(-2, 2, n), 100 + rng.uniform(-2, 2, n), rng.integers(0, 2, n), rng.integers(0, 256, (n, 32), dtype=np.uint8), prm)
    assert (np.diff(one_cell["start"]) > 0).sum() == 1
    P = observe(rng, one_cell, IDENTITY, prm, 30)
    h = check_fuse(po, orb, matcher, [one_cell], [IDENTITY], P, prm)
    assert h[3][3] == n and h[2][0] > 0
    x = np.array([-50, 400, 100, 100, np.nan, 1e20, 100, 319.9], np.float32)
    y = np.array([100, 100, -50, 300, 100, 100, 100, 239.9], np.float32)
    outside = keyframe(x, y, np.zeros(8), rng.integers(0, 256, (8, 32), dtype=np.uint8), prm)
    assert outside["start"][-1] == 1                      # only (100, 100) has a cell: roundf puts (319.9, 239.9) into column 64, row 48
    P = observe(rng, outside, IDENTITY, prm, 24)
    h = check_fuse(po, orb, matcher, [outside, one_cell], [IDENTITY, IDENTITY], P, prm, sync=True)
    assert set(h[0][0][h[0][0] >= 0]) <= {6}


# ---- 5. skip: NULL, all zero and a random mask; skipped pairs give -1 and count nothing ----
def test_skip_mask(po, orb, matcher):
    rng = np.random.default_rng(5)
    K, pose, P, prm = random_case(rng, n=90, N=200)
    K2 = random_keyframe(rng, prm, 60)
    kfs, poses = [K, K2], [pose, pose]
    none = check_fuse(po, orb, matcher, kfs, poses, P, prm)
    zero = check_fuse(po, orb, matcher, kfs, poses, P, prm, skip=np.zeros((2, 90), np.uint8), host=none)
    mask = (rng.random((2, 90)) < 0.4).astype(np.uint8)
    some = check_fuse(po, orb, matcher, kfs, poses, P, prm, skip=mask, sync=True)
    assert (some[0][mask != 0] == -1).all() and np.array_equal(some[0][mask == 0], none[0][mask == 0]) and some[3][0] < zero[3][0]
    full = check_fuse(po, orb, matcher, kfs, poses, P, prm, skip=np.full((2, 90), 255, np.uint8))
    assert full[3] == (0, 0, 0, 0) and (full[0] == -1).all()


# ---- 6. real frames: two extracts of a synthetic stereo pair ----
def map_points_of(K, pose, prm, z):
    """the map points of a keyframe's keypoints, back-projected at depth z through its pose, as MapPoint keeps them (UpdateNormalAndDepth)"""
    R, t, Ow = (np.asarray(a, np.float64) for a in pose)
    R = R.reshape(3, 3)
    Pc = np.stack([(K["x"] - float(prm["cx"])) * z / float(prm["fx"]), (K["y"] - float(prm["cy"])) * z / float(prm["fy"]), z * np.ones(len(K["x"]))])
    Pw = R.T @ (Pc - t[:, None])
    o = Pw - Ow[:, None]
    dist = np.sqrt((o * o).sum(0))
    maxd = (dist * prm["scale"][np.clip(K["octave"], 0, len(prm["scale"]) - 1)]).astype(np.float32)
    nrm = o / dist
    return dict(Px=Pw[0].astype(np.float32), Py=Pw[1].astype(np.float32), Pz=Pw[2].astype(np.float32), Nx=nrm[0].astype(np.float32),
                Ny=nrm[1].astype(np.float32), Nz=nrm[2].astype(np.float32), maxd=maxd, maxdi=(f32(1.2) * maxd).astype(np.float32),
                mindi=(f32(0.8) * (maxd / prm["scale"][-1])).astype(np.float32), desc=K["desc"])


def shifted(t):
    t = np.asarray(t, np.float32)
    return np.eye(3, dtype=np.float32).ravel(), t, -t


def test_real_frames(po, orb, configs, matcher):
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    gl, gr = _mk(orb, c), _mk(orb, c)
    s, i2 = scale_tables(c["L"])
    prm = default_params(fx=f32(c["fx"]), fy=f32(c["fx"]), cx=f32(c["w"] / 2), cy=f32(c["h"] / 2), bf=f32(c["bf"]), max_x=f32(c["w"]), max_y=f32(c["h"]),
                         scale=s, inv_sigma2=i2)
    frames = []
    for g, img in ((gl, left), (gr, right)):
        g.extract(img)
        kp = g.keypoints()
        n = len(kp) // 6
        frames.append((kp[:n].astype(np.float32), kp[n:2 * n].astype(np.float32), kp[4 * n:5 * n].astype(np.int32), g.descriptors().reshape(n, 32)))
    ur, _, _ = orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"])
    assert (ur >= 0).sum() > 30
    base = c["bf"] / c["fx"]
    for stereo in (True, False):
        A = keyframe(*frames[0], prm, ur if stereo else None)
        B = keyframe(*frames[1], prm)
        poseA, poseB = shifted([0, 0, 0]), shifted([-base, 0, 0])              # the right camera: Pc = Pw - (b, 0, 0)
        with np.errstate(divide="ignore"):
            zA = np.where(ur >= 0, c["bf"] / np.maximum(frames[0][0] - ur, 1e-3), 4.0)      # the depth the stereo match implies
        PA = map_points_of(A, poseA, prm, zA)
        PB = map_points_of(B, poseB, prm, 4.0)
        # both directions, each into the other frame and into its own frame at a slightly moved pose
        hA = check_fuse(po, orb, matcher, [B, A], [poseB, shifted([0.002, -0.001, 0.001])], PA, prm, sync=stereo)
        hB = check_fuse(po, orb, matcher, [A, B], [poseA, shifted([-base + 0.002, 0.001, 0])], PB, prm, sync=not stereo)
        assert hA[2][0] >= 15 and hA[2][1] >= 15 and hB[2][1] >= 15, (hA[2], hB[2])


# ---- 7. twenty calls with changing sizes on one matcher, interleaved with search_for_triangulation: no leaked state, independent statistics ----
def test_twenty_calls_interleaved_with_triangulation(po, orb):
    m = orb.KeyframeMatcher()
    lib = orb.load_library()
    rng = np.random.default_rng(77)
    KF1, KF2, geom, tprm = tri_random_case(rng, 60, 80, 5)
    assert lib.jsorb_fuse_stats(m.handle, None, None, None, None) == -4
    tri_hosts = tri.check_search(orb, m, KF1, [KF2], [geom], tprm)
    tri_stats = m.stats()
    assert lib.jsorb_fuse_stats(m.handle, None, None, None, None) == -4      # a triangulation is no fuse
    last = None
    for call in range(20):
        n, n_kf = int(rng.choice([0, 3, 40, 130])), int(rng.choice([1, 2, 5]))
        K, pose, P, prm = random_case(rng, n=n, N=int(rng.choice([9, 120, 300])), check=int(call % 4 != 3))
        kfs = [K] + [random_keyframe(rng, prm, int(rng.choice([0, 7, 90]))) for _ in range(n_kf - 1)]
        last = check_fuse(po, orb, m, kfs, [pose] * n_kf, P, prm, sync=call % 3 == 0)
        assert m.stats() == tri_stats                                         # a fuse leaves the triangulation statistics alone
        if call % 5 == 4:
            tri.check_search(orb, m, KF1, [KF2], [geom], tprm, sync=bool(call % 2), hosts=tri_hosts)
            assert m.fuse_stats() == last[3]                                  # ... and a triangulation the fuse statistics
    m.close()


# ---- 8. the async form on an external stream; a matcher thread beside an extracting handle ----
def test_async_on_an_external_stream(po, orb):
    import torch
    m = orb.KeyframeMatcher()
    own = m.get_stream()
    st = torch.cuda.Stream()
    m.set_stream(st.cuda_stream)
    rng = np.random.default_rng(8)
    K, pose, P, prm = random_case(rng, n=120, N=200)
    start, cat = concat([K])
    R, t, O = pose_arrays([pose])
    with torch.cuda.stream(st):
        dp, dk = dev_points(P), dev_keyframes(cat)                  # uploaded on the stream the matcher runs on: ordered without a wait
        bi, bd, cnt = m.fuse(dp, start, dk, R, t, O, fuse_params(orb, prm), wait=False)
        bi, bd, cnt = bi.cpu(), bd.cpu(), cnt.cpu()
    st.synchronize()
    h = fuse_keyframes(po, [K], [pose], P, prm)
    assert np.array_equal(bi.numpy(), h[0]) and np.array_equal(bd.numpy(), h[1]) and int(cnt[0]) == h[2][0] > 0 and m.fuse_stats() == h[3]
    m.set_stream(None)
    assert m.get_stream() == own
    check_fuse(po, orb, m, [K], [pose], P, prm, host=h)
    m.close()


def test_matcher_thread_beside_an_extractor(po, orb, configs):
    c = configs["c1"]
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    g = _mk(orb, c)
    g.extract(left)
    alone_kp, alone_desc = g.keypoints().copy(), g.descriptors().copy()
    rng = np.random.default_rng(9)
    K, pose, P, prm = random_case(rng, n=150, N=250)
    host = fuse_keyframes(po, [K], [pose], P, prm)
    m = orb.KeyframeMatcher()
    check_fuse(po, orb, m, [K], [pose], P, prm, host=host)
    errors = []

    def matching():
        try:
            for i in range(10):
                check_fuse(po, orb, m, [K], [pose], P, prm, sync=bool(i % 2), host=host)
        except BaseException as e:      # noqa: BLE001 - reported on the main thread
            errors.append(e)

    th = threading.Thread(target=matching)
    th.start()
    for i in range(10):
        g.extract(right if i % 2 else left)
        if i % 2 == 0:
            assert np.array_equal(g.keypoints(), alone_kp) and np.array_equal(g.descriptors(), alone_desc)
    th.join()
    assert not errors, errors
    m.close()


# ---- 9. validation: one assertion per rule ----
def test_edges_and_validation(po, orb, matcher):
    import torch
    lib = orb.load_library()
    fresh = orb.KeyframeMatcher()
    assert lib.jsorb_fuse_stats(fresh.handle, None, None, None, None) == -4      # before any fuse
    fresh.close()
    rng = np.random.default_rng(3)
    K, pose, P, prm = random_case(rng, n=50, N=60)
    p = fuse_params(orb, prm)
    start, cat = concat([K])
    dp, dk = dev_points(P), dev_keyframes(cat)
    R, t, O = pose_arrays([pose])
    bi = torch.zeros(2 * 50 + 8, dtype=torch.int32, device="cuda")
    bd = torch.zeros(2 * 50 + 8, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    pp = [dp[k].data_ptr() for k in orb.KeyframeMatcher.POINT_KEYS]
    pk = [dk[k].data_ptr() for k in orb.KeyframeMatcher.FUSE_KF_KEYS]
    host_o = (np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(256, np.int32))

    def call(prm_=p, n=50, a1=pp, nk=1, ks=start, a2=pk, r=R, tt=t, o=O, sk=None, out=(bi.data_ptr(), bd.data_ptr(), cnt.data_ptr()), fn=lib.jsorb_fuse_async):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return fn(matcher.handle, ctypes.byref(prm_) if prm_ is not None else None, n, *a1, nk, ptr(ks), *a2, ptr(r), ptr(tt), ptr(o), sk, *out)
    assert call() == 0
    matcher.sync()
    h = fuse_keyframes(po, [K], [pose], P, prm)
    assert np.array_equal(bi.cpu().numpy()[:50], h[0][0]) and np.array_equal(bd.cpu().numpy()[:50], h[1][0]) and cnt.cpu().numpy()[0] == h[2][0]
    assert call(prm_=None) == -1
    assert call(nk=-1) == -1 and call(nk=257) == -1
    assert call(n=-1) == -1
    assert call(ks=None) == -1 and call(r=None) == -1 and call(tt=None) == -1 and call(o=None) == -1
    for j in range(10):
        assert call(a1=pp[:j] + [None] + pp[j + 1:]) == -1, j
    for j in (0, 1, 2, 4):
        assert call(a2=pk[:j] + [None] + pk[j + 1:]) == -1, j
    assert call(a2=pk[:3] + [None] + pk[4:]) == 0                               # uright may be NULL
    assert call(a1=pp[:9] + [pp[9] + 8]) == -1 and call(a2=pk[:4] + [pk[4] + 8]) == -1      # misaligned descriptors
    for j in range(3):
        o = [bi.data_ptr(), bd.data_ptr(), cnt.data_ptr()]
        o[j] = None
        assert call(out=tuple(o)) == -1, j
    assert call(ks=np.array([5, 2], np.int32)) == -1 and call(ks=np.array([-1, 2], np.int32)) == -1
    assert call(ks=np.array([0, 1 << 18], np.int32)) == -1                      # a keyframe of 2^18 keypoints
    big = np.array([0, 1 << 17, 1 << 18], np.int32)                             # two keyframes of 2^17: 2^18 keypoints in the call
    assert call(nk=2, ks=big, r=np.tile(R, (2, 1)), tt=np.tile(t, (2, 1)), o=np.tile(O, (2, 1))) == -1
    assert b"262144" in lib.jsorb_keyframe_matcher_last_error(matcher.handle)
    many = np.zeros(257, np.int32)
    R256, t256, O256 = np.tile(R, (256, 1)), np.tile(t, (256, 1)), np.tile(O, (256, 1))
    host_ptrs = tuple(a.ctypes.data for a in host_o)
    assert call(n=1 << 23, nk=256, ks=many, r=R256, tt=t256, o=O256) == -3      # n_keyframes x n_points beyond INT_MAX - 256
    assert call(n=1 << 23, nk=256, ks=many, r=R256, tt=t256, o=O256, out=host_ptrs, fn=lib.jsorb_fuse) == -3
    for field, bad in (("n_levels", 0), ("n_levels", 17), ("th_low", -1), ("th_low", 256), ("cols", 0), ("rows", 0), ("cols", 100)):      # 100 x 48 > 4096
        q = fuse_params(orb, prm)
        setattr(q, field, bad)
        assert call(prm_=q) == -1, (field, bad)
    assert b"grid size" in lib.jsorb_keyframe_matcher_last_error(matcher.handle)
    for j in range(3):
        o = list(host_ptrs)
        o[j] = None
        assert call(out=tuple(o), fn=lib.jsorb_fuse) == -1, j
    # valid empty calls: no points, no keyframes - the counts are cleared
    cnt.fill_(9)
    assert call(n=0) == 0
    matcher.sync()
    assert cnt.cpu().numpy()[0] == 0 and matcher.fuse_stats() == (0, 0, 0, 0)
    assert call(nk=0, ks=None, r=None, tt=None, o=None) == 0 and call(nk=0, ks=None, r=None, tt=None, o=None, out=host_ptrs, fn=lib.jsorb_fuse) == 0
    assert call(n=0, a1=[None] * 10, out=(None, None, cnt.data_ptr())) == 0
    # 64 x 64 = 4096 cells is the largest grid
    q = default_params(cols=64, rows=64)
    Kq = keyframe(K["x"], K["y"], K["octave"], K["desc"], q, K["uright"])
    check_fuse(po, orb, matcher, [Kq], [pose], P, q)
    with pytest.raises(orb.JsorbError):
        matcher.fuse(dict(dp, Px=dp["Px"].double()), start, dk, R, t, O, p)
    with pytest.raises(orb.JsorbError):
        matcher.fuse(dp, start, dk, R, t, O, orb.make_bow_params())
    with pytest.raises(orb.JsorbError):
        matcher.fuse(dp, start, dk, R[:0], t, O, p)


# ---- 10. the C++ example through the compat shim: both directions, checked against its own sequential loop and the Python path ----
@pytest.mark.parametrize("check", [1, 0])
def test_search_in_neighbors_example(po, orb, configs, tmp_path, matcher, check):
    from jetson_slam_amd import build as jb
    c = configs["c1"]
    exe = jb.build_example("search_in_neighbors", str(tmp_path / "search_in_neighbors"))
    left, right = synth_stereo_pair(REAL_SEED, c["h"], c["w"])
    other = synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[1]
    images = [left, right, left, other]
    paths = [str(tmp_path / ("kf%d.raw" % i)) for i in range(4)]
    for img, p in zip(images, paths):
        img.tofile(p)
    op = str(tmp_path / "out.bin")
    out = subprocess.run([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), str(check)] + paths + [op], timeout=300,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    blob = np.fromfile(op, np.int32)
    nA, nB, fusedA, fusedB = (int(v) for v in blob[:4])
    ns = [int(v) for v in blob[4:8]]
    pos = [8]

    def take(n, dt=np.int32):
        a = blob[pos[0]:pos[0] + n].view(dt)
        pos[0] += n
        return a
    poses = [take(15, np.float32) for _ in range(4)]
    poses = [(T[:9], T[9:12], T[12:15]) for T in poses]
    uright = [take(n, np.float32) for n in ns]
    s, i2 = scale_tables(c["L"])
    w, hgt = c["w"], c["h"]
    prm = default_params(th=f32(3 if check else 4), check=check, fx=f32(w), fy=f32(w), cx=f32(0.5 * w), cy=f32(0.5 * hgt), bf=f32(f32(0.1) * f32(w)),
                         max_x=f32(w), max_y=f32(hgt), scale=s, inv_sigma2=i2)
    g = _mk(orb, c)
    kfs = []
    for img, n_k, u in zip(images, ns, uright):
        g.extract(img)
        kp = g.keypoints()
        n = len(kp) // 6
        assert n == n_k
        kfs.append(keyframe(kp[:n].astype(np.float32), kp[n:2 * n].astype(np.float32), kp[4 * n:5 * n].astype(np.int32), g.descriptors().reshape(n, 32), prm, u))
    total = 0
    for n, targets, tposes, whole in ((nA, kfs[1:], poses[1:], True), (nB, kfs[:1], poses[:1], False)):
        f = [take(n, np.float32) for _ in range(9)]
        P = dict(Px=f[0], Py=f[1], Pz=f[2], Nx=f[3], Ny=f[4], Nz=f[5], maxd=f[6], mindi=f[7], maxdi=f[8], desc=take(8 * n).view(np.uint8).reshape(n, 32))
        bi, bd = take(len(targets) * n).reshape(len(targets), n), take(len(targets) * n).reshape(len(targets), n)
        # the first direction skips nothing (no point of the current keyframe is in a target yet), so the file is the whole result; the second
        # skips what the first one's replay put into the current keyframe or replaced, and its mask is not in the file: there the Python path is
        # held to the file where the file has a match, and to the host functions everywhere
        h = check_fuse(po, orb, matcher, targets, tposes, P, prm, sync=True)
        found = bi >= 0
        assert not whole or (np.array_equal(bi, h[0]) and np.array_equal(bd, h[1]))
        assert np.array_equal(bi[found], h[0][found]) and np.array_equal(bd[found], h[1][found])
        total += int(found.sum())
    assert pos[0] == len(blob) and total >= 15 and fusedA >= 15 and fusedB >= 0
    assert ("fused=%d,%d" % (fusedA, fusedB)) in out.stdout and "host_sequential_us=" in out.stdout and "researched=" in out.stdout
