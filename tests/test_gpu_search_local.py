"""-m gpu: jsorb_search_local_points (k_assign_grid + k_local_candidates + k_local_resolve) on real extracted frames against the sequential
transcription of ORBmatcher::SearchByProjection and the fixed-point restatement of tests/test_search_local_host.py - match_kp, match_dist,
kp_match and the count, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair
from frame_builders import frame_of, points_near_keypoints
from test_search_local_host import build_grid, search_by_projection, search_local_restated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EUROC = ((458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480))


def _mk(orb, c):
    return orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _from_device_ptr(orb, ptr, n):
    """n floats at a device pointer of the library (jsorb_*_uright_device) into a torch tensor, device to device"""
    import torch
    t = torch.empty(max(n, 1), dtype=torch.float32, device="cuda")
    assert ptr and orb.load_library().jsorb_mem_d2d(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(4 * n)) == 0
    return t[:n]


def run_device(g, F, P, th, u_right_t=None, nn_ratio=0.8, th_high=100):
    import torch
    blocked = None if F["blocked"] is None else _dev(F["blocked"].astype(np.uint8))
    mk, md, km, cnt = g.search_local_points(_dev(P["u"]), _dev(P["v"]), _dev(P["invz"]), _dev(P["level"]), _dev(P["view_cos"]),
                                            _dev(P["in_frustum"]), _dev(P["desc"]), (float(F["min_x"]), float(F["min_y"]), float(F["inv_w"]),
                                                                                     float(F["inv_h"])),
                                            th=th, mbf=float(F["mbf"]), u_right=u_right_t, blocked=blocked, nn_ratio=nn_ratio, th_high=th_high,
                                            cols=F["cols"], rows=F["rows"])
    torch.cuda.synchronize()
    return mk.cpu().numpy(), md.cpu().numpy(), km.cpu().numpy(), int(cnt.cpu().numpy()[0])


def check(g, F, P, th, u_right_t=None, nn_ratio=0.8, th_high=100):
    m, d, km, cnt = run_device(g, F, P, th, u_right_t, nn_ratio, th_high)
    rm, rd, rkm, rcnt = search_by_projection(F, P, th, nn_ratio, th_high)
    sm, sd, skm, scnt, rounds = search_local_restated(F, P, th, nn_ratio, th_high)
    assert np.array_equal(m, rm) and np.array_equal(d, rd) and np.array_equal(km, rkm) and cnt == rcnt
    assert np.array_equal(m, sm) and np.array_equal(km, skm)
    dev_rounds, n_cand, n_over = g.search_local_stats()
    assert dev_rounds == rounds
    return cnt, (dev_rounds, n_cand, n_over)


def _stereo(orb, c, seed):
    left, right = synth_stereo_pair(seed, c["h"], c["w"])
    gl, gr = _mk(orb, c), _mk(orb, c)
    gl.extract(left)
    gr.extract(right)
    u, _, _ = orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"])
    return gl, gr, u, (left, right)


# ---- stereo C1 / C2: uRight from jsorb_stereo_uright_device, th 1, blocked keypoints, ties, levels 0 and L-1, view_cos both sides of 0.998 ----
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_stereo_frames_match_the_reference(orb, configs, name):
    c = configs[name]
    gl, gr, u, _ = _stereo(orb, c, 11)
    lib = orb.load_library()
    ur_t = _from_device_ptr(orb, lib.jsorb_stereo_uright_device(gl.handle, 0), len(u))
    assert np.array_equal(ur_t.cpu().numpy().view(np.uint32), u.view(np.uint32))
    rng = np.random.default_rng(3)
    N = len(u)
    F = frame_of(gl, c, u_right=u, blocked=(rng.random(N) < 0.05).astype(np.uint8))
    P, src = points_near_keypoints(rng, F, 3000 if name == "c2" else 800, c["L"])
    P["desc"][1::50] = P["desc"][0::50][:len(P["desc"][1::50])]            # identical descriptors: exact-tie distances
    P["level"][::37] = 0
    P["level"][5::37] = c["L"] - 1
    cnt, (rounds, n_cand, _) = check(gl, F, P, 1.0, ur_t)
    assert cnt > len(P["u"]) // 4 and n_cand > cnt
    assert (P["level"] == 0).any() and (P["level"] == c["L"] - 1).any()


# ---- monocular with a camera: mvKeysUn from k_undistort, no uRight ----
def test_monocular_with_camera(orb, configs):
    c = configs["c2"]
    (fx, fy, cx, cy), dist, _ = EUROC
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    g = _mk(orb, c)
    g.set_camera(K, dist)
    img, _ = synth_stereo_pair(5, c["h"], c["w"])
    g.extract(img)
    b = orb.image_bounds(K, dist, c["w"], c["h"])
    F = frame_of(g, c, bounds=(b[0], b[1], b[2], b[3]))
    assert not np.array_equal(F["kx"], g.keypoints(0)[:len(F["kx"])].astype(np.float32))      # the undistorted coordinates are binned
    rng = np.random.default_rng(4)
    P, _ = points_near_keypoints(rng, F, 2000, c["L"])
    cnt, _ = check(g, F, P, 1.0)
    assert cnt > 500


# ---- RGB-D, th = 3: uRight from jsorb_rgbd_uright_device ----
def test_rgbd_th3(orb, configs):
    c = dict(configs["c2"])
    g = _mk(orb, c)
    img, _ = synth_stereo_pair(8, c["h"], c["w"])
    g.extract(img)
    rng = np.random.default_rng(8)
    depth = rng.integers(0, 20000, (c["h"], c["w"])).astype(np.uint16)
    depth[rng.random(depth.shape) < 0.2] = 0
    u, _ = g.rgbd_depth(depth, 40.0, 1.0 / 5000)
    ur_t = _from_device_ptr(orb, orb.load_library().jsorb_rgbd_uright_device(g.handle, 0), len(u))
    c["bf"] = 40.0
    F = frame_of(g, c, u_right=u)
    P, _ = points_near_keypoints(rng, F, 2000, c["L"])
    cnt, _ = check(g, F, P, 3.0, ur_t)
    assert cnt > 300


# ---- th = 5 (after relocalisation): wide windows; the tiny_local_cap build overflows the per-point list on most points ----
def test_th5_and_candidate_overflow(orb, configs, monkeypatch):
    from jetson_slam_amd import build as jb
    c = configs["c2"]
    gl, _, u, _ = _stereo(orb, c, 21)
    ur_t = _from_device_ptr(orb, orb.load_library().jsorb_stereo_uright_device(gl.handle, 0), len(u))
    rng = np.random.default_rng(5)
    F = frame_of(gl, c, u_right=u)
    P, _ = points_near_keypoints(rng, F, 2000, c["L"])
    P["level"][::10] = c["L"] - 1
    cnt, (_, n_cand, n_over) = check(gl, F, P, 5.0, ur_t)
    assert cnt > 200 and n_cand > 3 * len(P["u"])
    # the same frame and points through the build with 2 candidates per point: the resolver rescans the grid for the rest
    lib = orb.load_library(jb.build_variant("tiny_local_cap", *jb.VARIANTS["tiny_local_cap"]))
    monkeypatch.setattr(orb, "_lib", lib)
    g2, _, u2, _ = _stereo(orb, c, 21)
    assert np.array_equal(u2.view(np.uint32), u.view(np.uint32))
    ur2 = _from_device_ptr(orb, lib.jsorb_stereo_uright_device(g2.handle, 0), len(u2))
    cnt2, (_, n_cand2, n_over2) = check(g2, F, P, 5.0, ur2)
    assert cnt2 == cnt and n_cand2 == n_cand and n_over2 > len(P["u"]) // 2


# ---- the shared compaction at a group's width and at the list's end: 15, 16, 17 and (on the small build) cap + 1 survivors in one window, the points
# in the first and last group of a wave, the first of the next wave and the last of the block ----
@pytest.mark.parametrize("variant", [None, "tiny_local_cap"])
def test_survivor_counts_at_the_group_and_list_edges(orb, configs, monkeypatch, variant):
    from jetson_slam_amd import build as jb
    from test_gpu_search_kf import constructed_on_device
    from test_search_kf_host import COMPACTION_AT, compaction_case
    from test_search_local_host import candidate_lists
    if variant:
        monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant(variant, *jb.VARIANTS[variant])))
    cap = 2 if variant else 128
    c = configs["c1"]
    F0, _, _ = compaction_case()
    g, Fk = constructed_on_device(orb, c, F0)
    F = dict(Fk, mbf=f32(c["bf"]), u_right=None)
    u = [40.0 if i in (0, 15) else 120.0 if i == 3 else 200.0 if i == 4 else 280.0 for i in range(16)]
    v = [140.0 if i == 15 else 40.0 if i in COMPACTION_AT else 100.0 for i in range(16)]
    P = dict(u=np.array(u, np.float32), v=np.array(v, np.float32), invz=np.ones(16, np.float32), level=np.zeros(16, np.int32),
             view_cos=np.ones(16, np.float32), in_frustum=np.ones(16, np.uint8), desc=np.zeros((16, 32), np.uint8))
    assert [len(l) for l in candidate_lists(F, P, 2.0)] == [COMPACTION_AT.get(i, 0) for i in range(16)]      # radius 2.5 * th = 5
    cnt, (rounds, n_cand, n_over) = check(g, F, P, 2.0)
    assert n_cand == sum(COMPACTION_AT.values()) and n_over == sum(k > cap for k in COMPACTION_AT.values()) == (4 if variant else 0)
    assert cnt == 4


# ---- a claim chain: every point at the same spot with the same descriptor; point i takes the i-th keypoint of the shared order ----
def test_claim_chain_needs_many_rounds(orb, configs):
    c = configs["c2"]
    g = _mk(orb, c)
    img, _ = synth_stereo_pair(13, c["h"], c["w"])
    g.extract(img)
    F = frame_of(g, c)
    rng = np.random.default_rng(13)
    best, best_n = None, 0
    for j in rng.integers(0, len(F["kx"]), 200):         # the keypoint whose th = 5 window holds most candidates
        P = dict(u=F["kx"][[j]], v=F["ky"][[j]], invz=np.ones(1, np.float32), level=F["octave"][[j]].astype(np.int32), view_cos=np.ones(1, np.float32),
                 in_frustum=np.ones(1, np.uint8), desc=F["desc"][[j]])
        from test_search_local_host import candidate_lists
        k = len(candidate_lists(F, P, 5.0)[0])
        if k > best_n:
            best, best_n = j, k
    assert best_n >= 10
    n = best_n + 3
    P = dict(u=np.full(n, F["kx"][best], np.float32), v=np.full(n, F["ky"][best], np.float32), invz=np.ones(n, np.float32),
             level=np.full(n, F["octave"][best], np.int32), view_cos=np.ones(n, np.float32), in_frustum=np.ones(n, np.uint8),
             desc=np.tile(F["desc"][best], (n, 1)))
    cnt, (rounds, _, _) = check(g, F, P, 5.0, None, nn_ratio=1.0, th_high=255)
    assert cnt >= 10 and rounds >= 9                      # a chain at least 8 deep


# ---- empty inputs, out-of-range levels, validation ----
def test_edges_and_validation(orb, configs):
    import torch
    c = configs["c1"]
    g = _mk(orb, c)
    img, _ = synth_stereo_pair(2, c["h"], c["w"])
    g.extract(img)
    F = frame_of(g, c)
    e = torch.empty(0, device="cuda")
    mk, md, km, cnt = g.search_local_points(e.float(), e.float(), e.float(), e.int(), e.float(), e.byte(), torch.empty((0, 32), dtype=torch.uint8, device="cuda"),
                                            (0.0, 0.0, float(F["inv_w"]), float(F["inv_h"])))
    assert len(mk) == 0 and int(cnt.item()) == 0 and (km.cpu().numpy() == -1).all() and len(km) == len(F["kx"])
    rng = np.random.default_rng(1)
    P, _ = points_near_keypoints(rng, F, 300, c["L"])
    P["level"][::3] = rng.choice([-1, c["L"], 1000, -(2 ** 31)], len(P["level"][::3]))
    P["u"][::7] = np.float32(1e30)
    P["v"][1::7] = np.float32(np.nan)
    m, _, _, cnt = run_device(g, F, P, 1.0)
    assert (m[::3] == -1).all() and cnt > 0
    check(g, F, P, 1.0)
    lib = orb.load_library()
    prm = orb.JsorbSearchParams(1.0, 0.8, 100, 40.0, 0, 0, 0.2, 0.2, 200, 100)       # cols * rows > 16384
    d = torch.zeros(64, dtype=torch.int32, device="cuda")
    n_out = ctypes.c_int()
    assert lib.jsorb_search_local_points_async(g.handle, 0, ctypes.byref(prm), 0, *([None] * 9), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr()) == -1
    prm = orb.JsorbSearchParams(1.0, 0.8, 100, 40.0, 0, 0, 0.2, 0.2, 64, 48)
    assert lib.jsorb_search_local_points_async(g.handle, 3, ctypes.byref(prm), 0, *([None] * 9), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr()) != 0
    assert lib.jsorb_search_local_points_async(g.handle, 0, ctypes.byref(prm), -1, *([None] * 9), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr()) == -1
    assert lib.jsorb_search_local_points_async(g.handle, 0, ctypes.byref(prm), 5, *([None] * 9), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr()) == -1
    assert lib.jsorb_search_local_points(g.handle, 0, ctypes.byref(prm), 0, *([None] * 9), None, ctypes.byref(n_out)) == 0 and n_out.value == 0
    with pytest.raises(orb.JsorbError):
        g.search_local_points(_dev(P["u"]), _dev(P["v"]), _dev(P["invz"]), _dev(P["level"].astype(np.int64)), _dev(P["view_cos"]),
                              _dev(P["in_frustum"]), _dev(P["desc"]), (0.0, 0.0, 0.2, 0.2))
    # kernel timing reports the three kernels
    g.enable_kernel_timing(True)
    run_device(g, F, P, 1.0)
    t = g.search_local_kernel_times()
    assert all(t[k][1] == 1 and t[k][0] > 0 for k in ("k_assign_grid", "k_local_candidates", "k_local_resolve"))


# ---- the Tracking chain: map points back-projected from stereo depth, jsorb_is_in_frustum on the device, its outputs fed straight in ----
def _local_map(rng, gl, u, depth, c, n):
    kp = gl.keypoints(0)
    N = len(kp) // 6
    x, y = kp[:N].astype(np.float32), kp[N:2 * N].astype(np.float32)
    ok = np.nonzero(depth > 0)[0]
    src = rng.choice(ok, min(n, len(ok)), replace=False)
    fx = fy = f32(c["fx"])
    cx, cy = f32(c["w"] / 2), f32(c["h"] / 2)
    z = depth[src].astype(np.float32)
    P = np.stack([(x[src] - cx) * z / fx, (y[src] - cy) * z / fy, z]).astype(np.float32)
    dist = np.linalg.norm(P, axis=0).astype(np.float32)
    Pn = (P / dist).astype(np.float32)                        # mean viewing direction from the camera centre (Ow = 0): viewCos ~ 1
    lvl = kp[4 * N:5 * N][src]
    scale = gl.get_scale_factors()
    maxd = (dist * scale[lvl] * f32(0.999)).astype(np.float32)      # MapPoint::UpdateNormalAndDepth: PredictScale gives the keypoint's level
    mind = (maxd / scale[-1]).astype(np.float32)
    D = np.stack([maxd, maxd * f32(1.2), mind * f32(0.8)]).astype(np.float32)   # MaxDistance, its invariance bounds (MapPoint.cpp)
    return src, P, Pn, D, (float(fx), float(fy), float(cx), float(cy))


def test_frustum_outputs_feed_the_matcher(orb, configs):
    import torch
    c = configs["c2"]
    gl, gr, u, _ = _stereo(orb, c, 17)
    _, depth, _ = orb.stereo_result(gl)
    rng = np.random.default_rng(17)
    src, P, Pn, D, (fx, fy, cx, cy) = _local_map(rng, gl, u, depth, c, 1500)
    n = P.shape[1]
    lib = orb.load_library()
    R = _dev(np.eye(3, dtype=np.float32).ravel())
    t = _dev(np.zeros(3, np.float32))
    Ow = _dev(np.zeros(3, np.float32))
    Pd, Pnd, Dd = _dev(P), _dev(Pn), _dev(D)
    zz, uu, vv, vc = (torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(4))
    lvl = torch.zeros(n, dtype=torch.int32, device="cuda")
    inside = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert lib.jsorb_is_in_frustum(None, n, Pd[0].data_ptr(), Pd[1].data_ptr(), Pd[2].data_ptr(), Pnd[0].data_ptr(), Pnd[1].data_ptr(), Pnd[2].data_ptr(),
                                   Dd[0].data_ptr(), Dd[1].data_ptr(), Dd[2].data_ptr(), R.data_ptr(), t.data_ptr(), Ow.data_ptr(), fx, fy, cx, cy,
                                   0, c["w"], 0, c["h"], c["L"], float(np.log(f32(1.2))), 0.5, zz.data_ptr(), uu.data_ptr(), vv.data_ptr(),
                                   lvl.data_ptr(), vc.data_ptr(), inside.data_ptr()) == 0
    F = frame_of(gl, c, u_right=u)
    desc = _dev(F["desc"][src])
    ur_t = _from_device_ptr(orb, lib.jsorb_stereo_uright_device(gl.handle, 0), len(u))
    mk, md, km, cnt = gl.search_local_points(uu, vv, zz, lvl, vc, inside, desc, (0.0, 0.0, float(F["inv_w"]), float(F["inv_h"])), th=1.0,
                                             mbf=c["bf"], u_right=ur_t)
    Ph = dict(u=uu.cpu().numpy(), v=vv.cpu().numpy(), invz=zz.cpu().numpy(), level=lvl.cpu().numpy(), view_cos=vc.cpu().numpy(),
              in_frustum=inside.cpu().numpy(), desc=F["desc"][src])
    rm, rd, rkm, rcnt = search_by_projection(F, Ph, 1.0)
    m = mk.cpu().numpy()
    assert np.array_equal(m, rm) and np.array_equal(md.cpu().numpy(), rd) and np.array_equal(km.cpu().numpy(), rkm) and int(cnt.item()) == rcnt
    assert Ph["in_frustum"].mean() > 0.9 and (m == src).mean() > 0.7          # most points find the keypoint they were made from


# ---- the C++ example through the compat shim ----
def test_search_local_points_example(orb, configs, tmp_path):
    c = configs["c2"]
    exe = str(tmp_path / "search_local_points")
    lib_dir = os.path.join(ROOT, "jetson_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "search_local_points.cpp"),
                           "-L", lib_dir, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib_dir, "-o", exe])
    gl, gr, u, (left, right) = _stereo(orb, c, 23)
    _, depth, _ = orb.stereo_result(gl)
    rng = np.random.default_rng(23)
    src, P, Pn, D, cam = _local_map(rng, gl, u, depth, c, 1200)
    n = P.shape[1]
    desc = gl.descriptors(0)[src]
    lp, rp, ip, op = (str(tmp_path / s) for s in ("l.raw", "r.raw", "in.bin", "out.bin"))
    left.tofile(lp)
    right.tofile(rp)
    with open(ip, "wb") as f:
        f.write(np.int32(n).tobytes())
        for a in (P, Pn, D, np.eye(3, dtype=np.float32).ravel(), np.zeros(3, np.float32), np.zeros(3, np.float32), np.array(cam, np.float32),
                  np.array([np.log(f32(1.2)), c["bf"], 1.0], np.float32)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(desc).tobytes())
    subprocess.check_call([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, ip, op], timeout=300)
    blob = np.fromfile(op, np.uint8)
    cnt = int(blob[:4].view(np.int32)[0])
    o = 4
    m = blob[o:o + 4 * n].view(np.int32); o += 4 * n
    fu, fv, fz, fc = (blob[o + 4 * n * k:o + 4 * n * (k + 1)].view(np.float32) for k in range(4)); o += 16 * n
    lv = blob[o:o + 4 * n].view(np.int32); o += 4 * n
    inside = blob[o:o + n]
    F = frame_of(gl, c, u_right=u)
    Ph = dict(u=fu, v=fv, invz=fz, level=lv, view_cos=fc, in_frustum=inside, desc=desc)
    rm, _, _, rcnt = search_by_projection(F, Ph, 1.0)
    sm, _, _, _, _ = search_local_restated(F, Ph, 1.0)
    assert np.array_equal(m, rm.astype(np.int32)) and np.array_equal(m, sm.astype(np.int32)) and cnt == rcnt
    assert (m == src).mean() > 0.7
