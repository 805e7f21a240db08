"""-m gpu: jsorb_search_last_frame (k_assign_grid + k_last_match + k_last_resolve, a second pass on the device) on real extracted frames against
the sequential transcription of the reference's GPU branch and the kernels' restatement of tests/test_search_last_frame_host.py - match_kp,
match_dist, kp_match, the count and the statistics, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from frame_builders import last_frame_of, params, points_of  # noqa: F401  (other GPU tests import them from here)
from jetson_slam_amd.synth import synth_stereo_pair
from test_gpu_search_local import EUROC, _dev, _from_device_ptr, _mk, _stereo, frame_of
from test_search_last_frame_host import (HISTO_LENGTH, ROTATION_CULL, rot_bin, rotation_cull_expected, search_by_projection_last, search_last_restated,
                                         track_with_motion_model)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INT_MIN = -2 ** 31


def run_device(orb, g, F, P, prm, u_right_t=None, image=0):
    import torch
    cols, rows = F["cols"], F["rows"]
    p = orb.make_last_frame_params(prm["Rcw"], prm["tcw"], (prm["fx"], prm["fy"], prm["cx"], prm["cy"]),
                                   (prm["min_x"], prm["max_x"], prm["min_y"], prm["max_y"]), (F["inv_w"], F["inv_h"]), th=float(prm["th"]),
                                   direction=prm["direction"], mbf=float(F["mbf"]), check_orientation=prm["check_orientation"],
                                   retry_below=prm["retry_below"], th_high=prm["th_high"], cols=cols, rows=rows)
    mk, md, km, cnt = g.search_last_frame(_dev(P["Px"]), _dev(P["Py"]), _dev(P["Pz"]), _dev(P["octave"]), _dev(P["angle"]), _dev(P["desc"]), p,
                                          u_right=u_right_t, image=image)
    torch.cuda.synchronize()
    return mk.cpu().numpy(), md.cpu().numpy(), km.cpu().numpy(), int(cnt.cpu().numpy()[0])


def check(po, orb, g, F, P, prm, u_right_t=None, image=0):
    m, d, km, cnt = run_device(orb, g, F, P, prm, u_right_t, image)
    ref = track_with_motion_model(po, F, P, prm)
    res = track_with_motion_model(po, F, P, prm, search_last_restated)
    for r in (ref, res):
        assert np.array_equal(m, r[0]) and np.array_equal(d, r[1]) and np.array_equal(km, r[2]) and cnt == r[3]
    passes, n_cand, ind = g.search_last_frame_stats()
    assert (passes, n_cand, ind) == (ref[6], ref[4], tuple(ref[5])) == (res[6], res[4], tuple(res[5]))
    return m, km, cnt, passes, ind


def culled_bins(F, P, m, ind):
    bins = {rot_bin(P["angle"][i], F["angle"][m[i]]) for i in np.nonzero(m >= 0)[0]}
    return bins - set(ind)


# ---- stereo C1 / C2: uRight from jsorb_stereo_uright_device, th 7, each direction ----
@pytest.mark.parametrize("name", ["c1", "c2"])
@pytest.mark.parametrize("direction", [1, -1, 0])
def test_stereo_frames_match_the_reference(po, orb, configs, name, direction):
    c = configs[name]
    gl, gr, u, _ = _stereo(orb, c, 41)
    ur_t = _from_device_ptr(orb, orb.load_library().jsorb_stereo_uright_device(gl.handle, 0), len(u))
    F = last_frame_of(gl, c, u_right=u)
    rng = np.random.default_rng(50 + direction)
    prm = params(c, F, 7, direction=direction, seed=direction + 2)
    P, src = points_of(rng, F, prm, 1500 if name == "c2" else 500, c["L"])
    m, km, cnt, passes, ind = check(po, orb, gl, F, P, prm, ur_t)
    mk = m[m >= 0]
    assert cnt > len(m) // 4 and passes == 1
    assert culled_bins(F, P, m, ind)                                  # at least one culled bin
    assert (np.bincount(mk) > 1).any()                                # at least one keypoint chosen twice
    assert (P["octave"][m >= 0] == 0).any()


# ---- monocular with a camera: mvKeysUn from k_undistort, th 15, direction 0, no uRight ----
def test_monocular_with_camera(po, orb, configs):
    c = configs["c2"]
    (fx, fy, cx, cy), dist, _ = EUROC
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
    g = _mk(orb, c)
    g.set_camera(K, dist)
    img, _ = synth_stereo_pair(5, c["h"], c["w"])
    g.extract(img)
    b = orb.image_bounds(K, dist, c["w"], c["h"])
    F = last_frame_of(g, c, bounds=(b[0], b[1], b[2], b[3]))
    prm = params(c, F, 15, bounds=b, cam=(fx, fy, cx, cy), seed=9)
    P, _ = points_of(np.random.default_rng(9), F, prm, 1500, c["L"])
    m, _, cnt, _, _ = check(po, orb, g, F, P, prm)
    assert cnt > 300


# ---- RGB-D: uRight from k_rgbd ----
def test_rgbd(po, orb, configs):
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
    F = last_frame_of(g, c, u_right=u)
    prm = params(c, F, 7, direction=1, seed=8)
    P, _ = points_of(rng, F, prm, 1500, c["L"])
    _, _, cnt, _, _ = check(po, orb, g, F, P, prm, ur_t)
    assert cnt > 50


# ---- the retry: forced, not at exactly 20, off ----
def test_retry(po, orb, configs):
    c = configs["c2"]
    gl, _, u, _ = _stereo(orb, c, 61)
    ur_t = _from_device_ptr(orb, orb.load_library().jsorb_stereo_uright_device(gl.handle, 0), len(u))
    F = last_frame_of(gl, c, u_right=u)
    rng = np.random.default_rng(61)
    prm = params(c, F, 7, seed=61)
    P, _ = points_of(rng, F, prm, 400, c["L"], outliers=0.0)
    # forced: most descriptors complemented (no match at any radius): the first pass finds fewer than 20
    far = rng.random(400) < 0.97
    Pf = dict(P, desc=np.where(far[:, None], ~P["desc"], P["desc"]))
    prm0 = dict(prm, retry_below=0)
    assert search_last_restated(po, F, Pf, prm0, prm["th"])[3] < 20
    m, km, cnt, passes, _ = check(po, orb, gl, F, Pf, prm, ur_t)
    assert passes == 2
    r2 = search_by_projection_last(po, F, Pf, prm, f32(14))
    assert np.array_equal(m, r2[0]) and np.array_equal(km, r2[2]) and cnt == r2[3]
    # exactly 20 first-pass matches: no retry
    for k in range(20, 400):
        Q = {key: val[:k] for key, val in P.items()}
        if search_last_restated(po, F, Q, prm0, prm["th"])[3] == 20:
            break
    else:
        pytest.fail("no prefix with exactly 20 matches")
    _, _, cnt, passes, _ = check(po, orb, gl, F, Q, prm, ur_t)
    assert cnt == 20 and passes == 1
    # retry off: one pass however few
    _, _, _, passes, _ = check(po, orb, gl, F, Pf, prm0, ur_t)
    assert passes == 1


# ---- the rotation check at its edges: four equal bins, a lone match at and below a tenth, an angle outside [0, 360), the check off ----
def test_rotation_cull_cases(po, orb, configs):
    from test_gpu_search_kf import constructed_on_device
    from test_search_kf_host import lattice_case
    c = configs["c1"]
    for name, rots in sorted(ROTATION_CULL.items()):
        F0, Pk, pk = lattice_case(rots)
        g, Fk = constructed_on_device(orb, c, F0)
        F = dict(Fk, mbf=f32(c["bf"]), u_right=None)
        n, own = len(rots), np.arange(len(rots))
        P = dict(Px=Pk["Px"], Py=Pk["Py"], Pz=Pk["Pz"], octave=np.zeros(n, np.int32), angle=Pk["angle"], desc=Pk["desc"])
        prm = dict(th=f32(5), th_high=100, direction=0, retry_below=0, fx=pk["fx"], fy=pk["fy"], cx=pk["cx"], cy=pk["cy"], min_x=f32(0), max_x=f32(c["w"]),
                   min_y=f32(0), max_y=f32(c["h"]), Rcw=pk["Rcw"], tcw=pk["tcw"])
        for on in (1, 0):
            ind, kept = rotation_cull_expected(rots, on)
            m, km, cnt, passes, got = check(po, orb, g, F, P, dict(prm, check_orientation=on))
            assert np.array_equal(m, own) and np.array_equal(km[:n], np.where(kept, own, -1)) and (km[n:] == -1).all(), (name, on)
            assert cnt == kept.sum() and got == ind and passes == 1, (name, on)


# ---- edges, validation, kernel timing ----
def test_edges_and_validation(po, orb, configs):
    import torch
    c = configs["c1"]
    gl, _, u, _ = _stereo(orb, c, 71)
    ur_t = _from_device_ptr(orb, orb.load_library().jsorb_stereo_uright_device(gl.handle, 0), len(u))
    F = last_frame_of(gl, c, u_right=u)
    rng = np.random.default_rng(71)
    prm = params(c, F, 7, seed=71)
    P, _ = points_of(rng, F, prm, 400, c["L"])
    P["Pz"][0:10] = -P["Pz"][0:10]                                   # behind the camera
    P["Px"][10:20] = P["Px"][10:20] + f32(100)                       # outside the bounds
    P["Px"][20:25] = np.nan
    P["Py"][25:30] = np.nan
    P["Px"][30:35] = f32(3e38)                                       # Pcz overflows: invz 0, u = cx or NaN
    P["Pz"][35:40] = f32(3e38)
    P["Pz"][40:45] = f32(-3e38)
    P["Px"][45:48] = f32(3e38)
    P["Pz"][45:48] = f32(3e38)
    P["octave"][50:60] = -1
    P["octave"][60:70] = c["L"]
    P["octave"][70:80] = INT_MIN
    m, _, cnt, _, _ = check(po, orb, gl, F, P, prm, ur_t)
    assert (m[:20] == -1).all() and (m[50:80] == -1).all() and cnt > 50
    check(po, orb, gl, F, P, dict(prm, check_orientation=0), ur_t)
    _, _, _, _, ind = check(po, orb, gl, dict(F, u_right=None), P, dict(prm, check_orientation=0, retry_below=0), None)
    assert ind == (-1, -1, -1)
    # n_points = 0
    e = torch.empty(0, device="cuda")
    p = orb.make_last_frame_params(prm["Rcw"], prm["tcw"], (prm["fx"], prm["fy"], prm["cx"], prm["cy"]), (0, c["w"], 0, c["h"]), (F["inv_w"], F["inv_h"]))
    mk, md, km, cnt = gl.search_last_frame(e.float(), e.float(), e.float(), e.int(), e.float(), torch.empty((0, 32), dtype=torch.uint8, device="cuda"), p)
    assert len(mk) == 0 and int(cnt.item()) == 0 and len(km) == len(F["kx"]) and (km.cpu().numpy() == -1).all()
    assert gl.search_last_frame_stats()[:2] == (2, 0)                # 0 < 20: the second pass ran too
    # validation
    lib = orb.load_library()
    d = torch.zeros(2, dtype=torch.int32, device="cuda")
    desc = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    fv = torch.zeros(2, dtype=torch.float32, device="cuda")
    o = [torch.zeros(len(F["kx"]) + 64, dtype=torch.int32, device="cuda") for _ in range(4)]       # every output its own buffer, N entries and more
    outs = [t.data_ptr() for t in o]
    ins = [fv.data_ptr()] * 3 + [d.data_ptr(), fv.data_ptr(), desc.data_ptr(), None]
    call = lambda prm_, n=2, image=0, i=ins, out=outs: lib.jsorb_search_last_frame_async(gl.handle, image, ctypes.byref(prm_), n, *i, *out)
    assert call(p) == 0
    assert call(p, n=-1) == -1
    assert call(p, image=3) != 0
    for j in range(6):                                               # NULL arrays
        assert call(p, i=ins[:j] + [None] + ins[j + 1:]) == -1, j
    for j in range(3):
        assert call(p, out=outs[:j] + [None] + outs[j + 1:]) == -1, j
    assert lib.jsorb_search_last_frame_async(gl.handle, 0, ctypes.byref(p), 2, *ins, *outs[:3], None) == -1
    assert call(p, i=ins[:5] + [desc.data_ptr() + 8, None]) == -1   # misaligned descriptors
    for bad in (dict(cols=200, rows=100), dict(cols=0), dict(direction=2), dict(direction=-2)):
        q = orb.make_last_frame_params(prm["Rcw"], prm["tcw"], (1, 1, 1, 1), (0, 1, 0, 1), (1, 1))
        for k, v in bad.items():
            setattr(q, k, v)
        assert call(q) == -1, bad
    n_out = ctypes.c_int()
    km_host = np.zeros(len(F["kx"]), np.int32)
    assert lib.jsorb_search_last_frame(gl.handle, 0, ctypes.byref(p), 0, *([None] * 7), km_host.ctypes.data, ctypes.byref(n_out)) == 0 and n_out.value == 0
    assert (km_host == -1).all()
    fresh = _mk(orb, c)
    assert lib.jsorb_search_last_frame_async(fresh.handle, 0, ctypes.byref(p), 0, *([None] * 7), *outs) != 0      # no extract yet
    assert fresh.handle and lib.jsorb_search_last_frame_stats(fresh.handle, None, None, None) != 0
    with pytest.raises(orb.JsorbError):
        gl.search_last_frame(_dev(P["Px"]), _dev(P["Py"]), _dev(P["Pz"]), _dev(P["octave"].astype(np.int64)), _dev(P["angle"]), _dev(P["desc"]), p)
    # kernel timing reports the grid and both passes' kernels
    gl.enable_kernel_timing(True)
    gl.reset_kernel_timing()
    run_device(orb, gl, F, P, prm, ur_t)
    t = gl.search_last_frame_kernel_times()
    assert t["k_assign_grid"][1] == 1 and t["k_last_match"][1] == 2 and t["k_last_resolve"][1] == 2
    assert all(t[k][0] > 0 for k in t)


# ---- image 5 of an 8-image device batch equals that image extracted alone ----
def test_batch_image_equals_single(po, orb, configs):
    import torch
    c = configs["c2"]
    imgs = [synth_stereo_pair(80 + i, c["h"], c["w"])[0] for i in range(8)]
    g = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=8)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 8, keep=dev)
    s = _mk(orb, c)
    s.extract(imgs[5])
    F = last_frame_of(s, c)
    prm = params(c, F, 7, seed=5)
    P, _ = points_of(np.random.default_rng(5), F, prm, 1000, c["L"])
    single = run_device(orb, s, F, P, prm)
    batch = run_device(orb, g, F, P, prm, image=5)
    assert all(np.array_equal(a, b) for a, b in zip(single[:3], batch[:3])) and single[3] == batch[3] > 100
    check(po, orb, g, F, P, prm, image=5)


# ---- the C++ example through the compat shim ----
def test_track_motion_model_example(po, orb, configs, tmp_path):
    c = configs["c2"]
    exe = str(tmp_path / "track_motion_model")
    lib_dir = os.path.join(ROOT, "jetson_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "track_motion_model.cpp"),
                           "-L", lib_dir, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib_dir, "-o", exe])
    gl, gr, u, (left, right) = _stereo(orb, c, 91)
    F = last_frame_of(gl, c, u_right=u)
    prm = params(c, F, 7, direction=1, seed=91)
    P, _ = points_of(np.random.default_rng(91), F, prm, 1200, c["L"])
    lp, rp, ip, op = (str(tmp_path / s) for s in ("l.raw", "r.raw", "in.bin", "out.bin"))
    left.tofile(lp)
    right.tofile(rp)
    n = len(P["Px"])
    with open(ip, "wb") as f:
        f.write(np.int32(n).tobytes())
        for a in (P["Px"], P["Py"], P["Pz"], P["angle"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(P["octave"], np.int32).tobytes())
        for a in (prm["Rcw"].ravel(), prm["tcw"], np.array([prm["fx"], prm["fy"], prm["cx"], prm["cy"], c["bf"], 7.0], np.float32)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.int32(1).tobytes())
        f.write(np.ascontiguousarray(P["desc"]).tobytes())
    subprocess.check_call([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), lp, rp, ip, op], timeout=300)
    blob = np.fromfile(op, np.int32)
    cnt, N = int(blob[0]), int(blob[1])
    km = blob[2:2 + N]
    prm = dict(prm, direction=1, th=f32(7))
    ref = track_with_motion_model(po, F, P, prm)
    assert N == len(F["kx"]) and np.array_equal(km, ref[2].astype(np.int32)) and cnt == ref[3] > 200
    assert HISTO_LENGTH == 30
