"""-m gpu: keypoint undistortion (k_undistort, jsorb_set_camera), the grid over mvKeysUn and the RGB-D depth sample (k_rgbd) on the device,
against numpy float64 / float32 restatements of the contract in include/jsorb.h - all bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jetson_slam_amd.synth import synth_stereo_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Examples/RGB-D/TUM1.yaml and Examples/Monocular/EuRoC.yaml: (fx, fy, cx, cy), (k1, k2, p1, p2, k3), calibrated image size
TUM1 = ((517.306408, 516.469215, 318.643040, 255.313989), (0.262383, -0.953104, -0.005358, 0.002628, 1.163314), (640, 480))
EUROC = ((458.654, 457.296, 367.215, 248.375), (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0), (752, 480))


# ---- numpy restatement of the contract (float64 element-wise: numpy does not fuse) ----
def undistort_ref(intr, dist, u, v):
    fx, fy, cx, cy = (np.float64(np.float32(a)) for a in intr)
    k1, k2, p1, p2, k3 = (np.float64(np.float32(a)) for a in dist)
    ifx, ify = np.float64(1.0) / fx, np.float64(1.0) / fy
    u = np.asarray(u, np.float32).astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    x, y = (u - cx) * ifx, (v - cy) * ify
    x0, y0 = x.copy(), y.copy()
    done = np.zeros(u.shape, bool)
    exits = np.zeros(u.shape, bool)
    for _ in range(5):
        r2 = x * x + y * y
        with np.errstate(divide="ignore"):
            icdist = np.float64(1.0) / (np.float64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2)
        ex = ~done & (icdist < 0)
        x = np.where(ex, (u - cx) * ifx, x)
        y = np.where(ex, (v - cy) * ify, y)
        exits |= ex
        done |= ex
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(done, x, (x0 - dx) * icdist)
        y = np.where(done, y, (y0 - dy) * icdist)
    return (fx * x + cx).astype(np.float32), (fy * y + cy).astype(np.float32), exits


def roundf(v):
    """C's roundf (half away from zero) of float32 values: exact in float64"""
    v = np.asarray(v, np.float32).astype(np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def grid_ref(x, y, bounds, cols=64, rows=48):
    """Frame::AssignFeaturesToGrid + PosInGrid in float32: cell = (round((x - minX) * invW), round((y - minY) * invH))"""
    minx, maxx, miny, maxy = (np.float32(b) for b in bounds)
    inv_w = np.float32(cols) / np.float32(maxx - minx)
    inv_h = np.float32(rows) / np.float32(maxy - miny)
    px = roundf((np.asarray(x, np.float32) - minx) * inv_w)
    py = roundf((np.asarray(y, np.float32) - miny) * inv_h)
    cells = [[] for _ in range(cols * rows)]
    for i, (a, b) in enumerate(zip(px, py)):
        if 0 <= a < cols and 0 <= b < rows:
            cells[int(a) * rows + int(b)].append(i)
    start = np.zeros(cols * rows + 1, np.int32)
    start[1:] = np.cumsum([len(c) for c in cells])
    return start, np.array([i for c in cells for i in c], np.int32), (px, py)


def rgbd_ref(x, y, x_un, depth, fmt, factor, mbf):
    """Frame::ComputeStereoFromRGBD after Tracking.cpp:333-334's conversion, in float32"""
    raw = depth[np.asarray(y, np.int64), np.asarray(x, np.int64)]
    f = np.float32(factor)
    if fmt == "u16" or abs(np.float32(f - np.float32(1.0))) > 1e-5:
        d = raw.astype(np.float32) * f
    else:
        d = raw.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = d > 0
        u = np.where(ok, np.asarray(x_un, np.float32) - np.float32(mbf) / np.where(ok, d, np.float32(1)), np.float32(-1)).astype(np.float32)
    return u, np.where(ok, d, np.float32(-1)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mk(orb, c, max_batch=1):
    return orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=max_batch)


def camera_for(cal, c):
    """the calibration scaled to the handle's image size (intrinsics only; the distortion is the dataset's)"""
    (fx, fy, cx, cy), dist, (w, h) = cal
    s, t = c["w"] / w, c["h"] / h
    return (fx * s, fy * t, cx * s, cy * t), dist


def K_of(intr):
    fx, fy, cx, cy = intr
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def _xy(kp):
    n = len(kp) // 6
    return kp[:n], kp[n:2 * n]


def _check_un(g, intr, dist, image=0):
    kp = g.keypoints(image)
    x, y = _xy(kp)
    xu, yu = g.keypoints_undistorted(image)
    rx, ry, _ = undistort_ref(intr, dist, x, y)
    assert np.array_equal(bits(xu), bits(rx)) and np.array_equal(bits(yu), bits(ry))
    return kp, xu, yu


# ---- 1. single frame, TUM1 / EuRoC cameras ----
@pytest.mark.parametrize("name", ["tiny", "c1", "c2"])
@pytest.mark.parametrize("cal", ["tum1", "euroc"])
def test_single_frame_undistortion_matches_numpy(orb, configs, name, cal):
    c = configs[name]
    intr, dist = camera_for(TUM1 if cal == "tum1" else EUROC, c)
    img, _ = synth_stereo_pair(21, c["h"], c["w"])
    plain, cam = _mk(orb, c), _mk(orb, c)
    cam.set_camera(K_of(intr), dist)
    assert cam.camera_enabled() and not plain.camera_enabled()
    pk, pd = plain.extract(img)
    ck, cd = cam.extract(img)
    assert np.array_equal(pk, ck) and np.array_equal(pd, cd) and np.array_equal(bits(plain.angles()), bits(cam.angles()))
    kp, xu, yu = _check_un(cam, intr, dist)
    x, y = _xy(kp)
    assert len(x) > 20 and not np.array_equal(xu, x.astype(np.float32))
    # unpack with mvKeysUn: mvKeys as jsorb_unpack_frame gives them, mvKeysUn = mvKeys with pt replaced
    keys, keys_un, desc = cam.unpack_frame_undistorted()
    k0, d0 = plain.unpack_frame()
    assert np.array_equal(keys, k0) and np.array_equal(desc, d0)
    assert np.array_equal(bits(keys_un["x"]), bits(xu)) and np.array_equal(bits(keys_un["y"]), bits(yu))
    for f in ("size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(keys_un[f], keys[f]), f
    # the device pointer holds the same x_un[N] y_un[N]
    import torch
    p = cam._lib.jsorb_keypoints_un_device(cam.handle, 0)
    assert p and plain._lib.jsorb_keypoints_un_device(plain.handle, 0) is None
    n = len(x)
    dev = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    orb.load_library().jsorb_mem_d2d(ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(p), 8 * n)
    assert np.array_equal(bits(dev.cpu().numpy()), bits(np.concatenate([xu, yu])))


# ---- 2. device batch with lanes ----
def test_device_batch_with_lanes_matches_numpy_and_single_frames(orb, configs):
    import torch
    c, B = configs["c2"], 64
    intr, dist = camera_for(TUM1, c)
    imgs = [synth_stereo_pair(600 + (i % 9), c["h"], c["w"])[i % 2] for i in range(B)]
    g = _mk(orb, c, max_batch=B)
    g.set_camera(K_of(intr), dist)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], B, keep=dev)
    g.sync()
    s = _mk(orb, c)
    s.set_camera(K_of(intr), dist)
    for i in range(0, B, 5):
        kp, xu, yu = _check_un(g, intr, dist, i)
        if i < 20:
            sk, _ = s.extract(imgs[i])
            sx, sy = s.keypoints_undistorted()
            assert np.array_equal(sk, kp) and np.array_equal(bits(sx), bits(xu)) and np.array_equal(bits(sy), bits(yu))
    # host-streamed batch as well
    h = _mk(orb, c, max_batch=8)
    h.set_camera(K_of(intr), dist)
    h.extract_batch_host_async(np.stack(imgs[:8]))
    h.sync()
    for i in (0, 7):
        _check_un(h, intr, dist, i)


# ---- 3. k1 == 0: the reference's k1-only test ----
def test_k1_zero_camera_is_inactive(orb, configs):
    c = configs["c1"]
    intr, _ = camera_for(TUM1, c)
    img, _ = synth_stereo_pair(22, c["h"], c["w"])
    g = _mk(orb, c)
    g.set_camera(K_of(intr), (0.0, -0.9, 0.004, -0.003, 1.2))
    assert not g.camera_enabled()
    kp, _ = g.extract(img)
    x, y = _xy(kp)
    xu, yu = g.keypoints_undistorted()
    assert np.array_equal(bits(xu), bits(x.astype(np.float32))) and np.array_equal(bits(yu), bits(y.astype(np.float32)))
    keys, keys_un, _ = g.unpack_frame_undistorted()
    assert np.array_equal(keys, keys_un)
    assert g._lib.jsorb_keypoints_un_device(g.handle, 0) is None


# ---- 4. the icdist < 0 exit ----
def test_negative_icdist_exit_matches(orb, configs):
    c = configs["c2"]
    intr, _ = camera_for(TUM1, c)
    dist = (-1.0, 0.0, 0.001, -0.002, 0.0)
    img, _ = synth_stereo_pair(23, c["h"], c["w"])
    g = _mk(orb, c)
    g.set_camera(K_of(intr), dist)
    kp, _ = g.extract(img)
    x, y = _xy(kp)
    _, _, exits = undistort_ref(intr, dist, x, y)
    assert exits.sum() > 0 and (~exits).sum() > 0
    _check_un(g, intr, dist)


# ---- 5. the grid over mvKeysUn ----
def test_grid_bins_undistorted_keypoints(orb, configs):
    c = configs["c2"]
    intr, dist = camera_for(TUM1, c)
    img, _ = synth_stereo_pair(24, c["h"], c["w"])
    g, plain = _mk(orb, c), _mk(orb, c)
    g.set_camera(K_of(intr), dist)
    kp, _ = g.extract(img)
    plain.extract(img)
    bounds = orb.image_bounds(K_of(intr), dist, c["w"], c["h"])
    xu, yu = g.keypoints_undistorted()
    want_s, want_i, _ = grid_ref(xu, yu, bounds)
    inv_w, inv_h = float(np.float32(64) / (bounds[1] - bounds[0])), float(np.float32(48) / (bounds[3] - bounds[2]))
    start, items = g.assign_features_to_grid(float(bounds[0]), float(bounds[2]), inv_w, inv_h)
    assert np.array_equal(start, want_s) and np.array_equal(items, want_i)
    # without a camera: the keypoint coordinates, as before
    x, y = _xy(kp)
    ps, pi = plain.assign_features_to_grid(0.0, 0.0, float(np.float32(64) / np.float32(c["w"])), float(np.float32(48) / np.float32(c["h"])))
    ws, wi, _ = grid_ref(x.astype(np.float32), y.astype(np.float32), (0, c["w"], 0, c["h"]))
    assert np.array_equal(ps, ws) and np.array_equal(pi, wi)
    assert not np.array_equal(start, ps)


# ---- 6. RGB-D ----
def _depth_u16(c, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 40000, (c["h"], c["w"])).astype(np.uint16)
    d[rng.random((c["h"], c["w"])) < 0.2] = 0
    return d


def _depth_f32(c, seed):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-2, 8, (c["h"], c["w"])).astype(np.float32)
    r = rng.random((c["h"], c["w"]))
    d[r < 0.1] = 0.0
    d[(r >= 0.1) & (r < 0.2)] = np.nan
    d[(r >= 0.2) & (r < 0.25)] = np.inf
    d[(r >= 0.25) & (r < 0.3)] = -np.inf
    d[(r >= 0.3) & (r < 0.35)] = 1e-37        # tiny positive: mbf / d overflows to inf
    return d


@pytest.mark.parametrize("with_camera", [False, True])
def test_rgbd_single_frame_matches_numpy(orb, configs, with_camera):
    c = configs["c2"]
    intr, dist = camera_for(TUM1, c)
    mbf = 40.0
    g = _mk(orb, c)
    if with_camera:
        g.set_camera(K_of(intr), dist)
    img, _ = synth_stereo_pair(25, c["h"], c["w"])
    kp, _ = g.extract(img)
    x, y = _xy(kp)
    xu, _ = g.keypoints_undistorted()
    cases = [(_depth_u16(c, 1), "u16", np.float32(1.0) / np.float32(5000.0)), (_depth_f32(c, 2), "f32", 1.0), (_depth_f32(c, 3), "f32", 1.000004),
             (_depth_f32(c, 4), "f32", 1.00002), (_depth_f32(c, 5), "f32", 0.5)]
    for depth, fmt, factor in cases:
        u, d = g.rgbd_depth(depth, mbf, factor)
        ru, rd = rgbd_ref(x, y, xu, depth, fmt, factor, mbf)
        assert np.array_equal(bits(u), bits(ru)) and np.array_equal(bits(d), bits(rd)), (fmt, factor)
        assert (rd > 0).sum() > 10 and (rd == -1).sum() > 10
        u2, d2 = g.rgbd_result(0)
        assert np.array_equal(bits(u2), bits(u)) and np.array_equal(bits(d2), bits(d))
    # a strided host depth image (step > W elements)
    wide = np.zeros((c["h"], c["w"] + 24), np.uint16)
    wide[:, :c["w"]] = cases[0][0]
    n = g.n_keypoints(0)
    u, d = np.zeros(n, np.float32), np.zeros(n, np.float32)
    g._chk(g._lib.jsorb_rgbd_depth(g.handle, wide.ctypes.data, orb.DEPTH_U16, wide.strides[0], cases[0][2], mbf, u.ctypes.data, d.ctypes.data))
    ru, rd = rgbd_ref(x, y, xu, cases[0][0], "u16", cases[0][2], mbf)
    assert np.array_equal(bits(u), bits(ru)) and np.array_equal(bits(d), bits(rd))


def test_rgbd_device_batch_matches_numpy(orb, configs):
    import torch
    c, B = configs["c2"], 24
    intr, dist = camera_for(TUM1, c)
    mbf, factor = 40.0, np.float32(1.0) / np.float32(5000.0)
    imgs = [synth_stereo_pair(700 + i, c["h"], c["w"])[0] for i in range(B)]
    deps16 = np.stack([_depth_u16(c, 100 + i) for i in range(B)])
    deps32 = np.stack([_depth_f32(c, 200 + i) for i in range(B)])
    g = _mk(orb, c, max_batch=B)
    g.set_camera(K_of(intr), dist)
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], B, keep=dev)
    d16 = torch.from_numpy(deps16.view(np.int16)).cuda()
    g.rgbd_depth(d16, mbf, factor)
    g.sync()
    single = _mk(orb, c)
    single.set_camera(K_of(intr), dist)
    for i in range(0, B, 4):
        x, y = _xy(g.keypoints(i))
        xu, _ = g.keypoints_undistorted(i)
        u, d = g.rgbd_result(i)
        ru, rd = rgbd_ref(x, y, xu, deps16[i], "u16", factor, mbf)
        assert np.array_equal(bits(u), bits(ru)) and np.array_equal(bits(d), bits(rd))
        if i < 12:
            single.extract(imgs[i])
            su, sd = single.rgbd_depth(deps16[i], mbf, factor)
            assert np.array_equal(bits(su), bits(u)) and np.array_equal(bits(sd), bits(d))
    d32 = torch.from_numpy(deps32).cuda()
    g.rgbd_depth(d32, mbf, 1.000004)
    g.sync()
    for i in (0, 11, B - 1):
        x, y = _xy(g.keypoints(i))
        xu, _ = g.keypoints_undistorted(i)
        u, d = g.rgbd_result(i)
        ru, rd = rgbd_ref(x, y, xu, deps32[i], "f32", 1.000004, mbf)
        assert np.array_equal(bits(u), bits(ru)) and np.array_equal(bits(d), bits(rd))


# ---- 7. graph replay, camera changes between frames ----
def test_graph_replay_and_camera_changes_between_frames(orb, configs):
    c = configs["c1"]
    t_intr, t_dist = camera_for(TUM1, c)
    e_intr, e_dist = camera_for(EUROC, c)
    frames = [synth_stereo_pair(30 + i, c["h"], c["w"])[0] for i in range(3)]
    g = _mk(orb, c)
    g.set_camera(K_of(t_intr), t_dist)
    for _ in range(2):
        for img in frames:                       # captured, then replayed with other inputs
            g.extract(img)
            _check_un(g, t_intr, t_dist)
            keys, keys_un, _ = g.unpack_frame_undistorted()
            xu, yu = g.keypoints_undistorted()
            assert np.array_equal(bits(keys_un["x"]), bits(xu))
    g.clear_camera()
    assert not g.camera_enabled()
    g.extract(frames[0])
    x, y = _xy(g.keypoints())
    xu, _ = g.keypoints_undistorted()
    assert np.array_equal(bits(xu), bits(x.astype(np.float32)))
    g.set_camera(K_of(e_intr), e_dist)          # results already there are undistorted with the new camera at once
    _check_un(g, e_intr, e_dist)
    for img in frames:
        g.extract(img)
        _check_un(g, e_intr, e_dist)
    g.set_camera(K_of(t_intr), t_dist)
    g.extract(frames[1])
    _check_un(g, t_intr, t_dist)


# ---- 8. kernel timing: nothing new without a camera ----
def test_no_camera_launches_no_undistort(orb, configs):
    c = configs["c1"]
    intr, dist = camera_for(TUM1, c)
    img, _ = synth_stereo_pair(26, c["h"], c["w"])
    plain, cam = _mk(orb, c), _mk(orb, c)
    cam.set_camera(K_of(intr), dist)
    for g in (plain, cam):
        g.enable_kernel_timing(True)
        g.extract(img); g.extract(img)
    assert plain.undistort_kernel_time()[1] == 0 and plain.rgbd_kernel_time()[1] == 0
    ms, n = cam.undistort_kernel_time()
    assert n == 2 and ms > 0
    _check_un(cam, intr, dist)
    cam.rgbd_depth(_depth_u16(c, 9), 40.0, 1.0 / 5000)
    assert cam.rgbd_kernel_time()[1] == 1


# ---- 9. the C++ example ----
def test_rgbd_frame_example_matches_python(orb, configs, tmp_path):
    c = dict(configs["c2"])
    c.update(h=480, w=640)
    (fx, fy, cx, cy), dist, _ = TUM1
    exe = str(tmp_path / "rgbd_frame")
    lib_dir = os.path.join(ROOT, "jetson_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "rgbd_frame.cpp"),
                           "-L", lib_dir, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib_dir, "-o", exe])
    img, _ = synth_stereo_pair(27, c["h"], c["w"])
    depth = _depth_u16(c, 27)
    gp, dp = str(tmp_path / "g.raw"), str(tmp_path / "d.u16")
    img.tofile(gp)
    depth.tofile(dp)
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), gp, dp] +
                          [repr(v) for v in (fx, fy, cx, cy) + dist] + ["40.0", "5000.0", "3", out], timeout=300)
    blob = np.fromfile(out, np.uint8)
    n = int(np.frombuffer(blob[:4].tobytes(), np.int32)[0])
    o = 4
    keys = np.frombuffer(blob[o:o + 28 * n].tobytes(), orb.KEYPOINT_DTYPE); o += 28 * n
    keys_un = np.frombuffer(blob[o:o + 28 * n].tobytes(), orb.KEYPOINT_DTYPE); o += 28 * n
    desc = blob[o:o + 32 * n].reshape(n, 32); o += 32 * n
    u = np.frombuffer(blob[o:o + 4 * n].tobytes(), np.float32); o += 4 * n
    d = np.frombuffer(blob[o:o + 4 * n].tobytes(), np.float32); o += 4 * n
    bnd = np.frombuffer(blob[o:o + 16].tobytes(), np.float32); o += 16
    start = np.frombuffer(blob[o:o + 4 * (64 * 48 + 1)].tobytes(), np.int32); o += 4 * (64 * 48 + 1)
    items = np.frombuffer(blob[o:].tobytes(), np.int32)
    g = _mk(orb, c)
    K = K_of((fx, fy, cx, cy))
    g.set_camera(K, dist)
    g.extract(img)
    pk, pku, pd = g.unpack_frame_undistorted()
    factor = np.float32(1.0) / np.float32(5000.0)
    pu, pdd = g.rgbd_depth(depth, 40.0, factor)
    pb = orb.image_bounds(K, dist, c["w"], c["h"])
    ps, pi = g.assign_features_to_grid(float(pb[0]), float(pb[2]), float(np.float32(64) / (pb[1] - pb[0])), float(np.float32(48) / (pb[3] - pb[2])))
    assert n == len(pk) and np.array_equal(keys, pk) and np.array_equal(keys_un, pku) and np.array_equal(desc, pd)
    assert np.array_equal(bits(u), bits(pu)) and np.array_equal(bits(d), bits(pdd)) and np.array_equal(bits(bnd), bits(pb))
    assert np.array_equal(start, ps) and np.array_equal(items, pi)


# ---- RGB-D batch on a caller's stream (jsorb_set_stream): ordered after the caller's work, and the caller's next work after it ----
def test_rgbd_batch_follows_the_callers_stream(orb, configs):
    import torch
    c, B = configs["c2"], 48                      # two lanes: the kernels run on pool streams, not on the caller's
    intr, dist = camera_for(TUM1, c)
    mbf, factor = 40.0, np.float32(1.0) / np.float32(5000.0)
    imgs = np.stack([synth_stereo_pair(800 + i, c["h"], c["w"])[0] for i in range(B)])
    deps = np.stack([_depth_u16(c, 300 + i) for i in range(B)])
    dev = torch.from_numpy(imgs).cuda()
    src = torch.from_numpy(deps.view(np.int16)).cuda()
    depth = torch.zeros_like(src)
    g = _mk(orb, c, max_batch=B)
    T = g.T
    out = torch.full((B, 2, T), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g.set_camera(K_of(intr), dist)
    g.set_stream(s.cuda_stream)
    g.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], B, keep=dev)
    assert g._lib.jsorb_n_images(g.handle) == B
    with torch.cuda.stream(s):
        a = torch.randn(3072, 3072, device="cuda")
        for _ in range(6):                        # the depth images arrive late on the caller's stream
            a = a @ a / 3072.0
        depth.copy_(src)
    g.rgbd_depth(depth, mbf, factor)
    lib = orb.load_library()
    for i in range(B):                            # read the results back on the caller's stream, right behind the call
        up = lib.jsorb_rgbd_uright_device(g.handle, i)
        dp = lib.jsorb_rgbd_depth_device(g.handle, i)
        assert up and dp
        for k, p in ((0, up), (1, dp)):
            g._chk(lib.jsorb_mem_d2d_async(ctypes.c_void_p(out[i, k].data_ptr()), ctypes.c_void_p(p), ctypes.c_size_t(4 * T), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    g.sync()
    res = out.cpu().numpy()
    for i in range(B):
        x, y = _xy(g.keypoints(i))
        xu, _ = g.keypoints_undistorted(i)
        ru, rd = rgbd_ref(x, y, xu, deps[i], "u16", factor, mbf)
        m = len(x)
        assert np.array_equal(bits(res[i, 0, :m]), bits(ru)) and np.array_equal(bits(res[i, 1, :m]), bits(rd)), i
        assert (rd > 0).sum() > 10


# ---- what an RGB-D call covers, and what it rejects ----
def test_rgbd_results_cover_only_the_images_computed(orb, configs):
    import torch
    c, B = configs["c1"], 4
    g = _mk(orb, c, max_batch=B)
    imgs = np.stack([synth_stereo_pair(900 + i, c["h"], c["w"])[0] for i in range(B)])
    g.extract_batch_host_async(imgs)
    g.sync()
    lib = orb.load_library()
    assert lib.jsorb_rgbd_uright_device(g.handle, 0) is None                 # no RGB-D call since the extract
    depth = _depth_u16(c, 5)
    u, d = g.rgbd_depth(depth, 40.0, 1.0 / 5000)                           # synchronous: image 0 only
    assert lib.jsorb_rgbd_uright_device(g.handle, 0) and lib.jsorb_rgbd_depth_device(g.handle, 0)
    for i in range(1, B):
        assert lib.jsorb_rgbd_uright_device(g.handle, i) is None and lib.jsorb_rgbd_depth_device(g.handle, i) is None
        with pytest.raises(orb.JsorbError):
            g.rgbd_result(i)
    u0, d0 = g.rgbd_result(0)
    assert np.array_equal(bits(u0), bits(u)) and np.array_equal(bits(d0), bits(d))
    dd = torch.from_numpy(np.stack([_depth_u16(c, 10 + i) for i in range(B)]).view(np.int16)).cuda()
    g.rgbd_depth(dd, 40.0, 1.0 / 5000)
    g.sync()
    assert all(lib.jsorb_rgbd_uright_device(g.handle, i) for i in range(B))
    # overlapping depth images are refused: image_stride below H * step
    step = c["w"] * 2
    for stride in (0, step * (c["h"] - 1)):
        rc = lib.jsorb_rgbd_depth_batch_device_async(g.handle, dd.data_ptr(), stride, step, orb.DEPTH_U16, 1.0 / 5000, 40.0, B)
        assert rc == -1
    # the binding refuses host tensors and element types it cannot read
    with pytest.raises(orb.JsorbError):
        g.rgbd_depth(dd.cpu(), 40.0, 1.0 / 5000)
    for bad in (dd.to(torch.int32), dd.to(torch.float64)):
        with pytest.raises(orb.JsorbError):
            g.rgbd_depth(bad, 40.0, 1.0 / 5000)
    with pytest.raises(orb.JsorbError):
        g.rgbd_depth(depth.astype(np.int32), 40.0, 1.0 / 5000)
    g.extract_batch_host_async(imgs)
    g.sync()
    assert lib.jsorb_rgbd_uright_device(g.handle, 0) is None                 # a new extract drops the old results
