"""-m gpu: rectification of raw images on the device (k_rectify, jsorb_set_rectify_maps).  Level 0 is checked against a numpy restatement of
cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) in OpenCV's fixed-point form, the rest of the pipeline against the CPU oracle run on the numpy-
rectified images, and identity maps against the same handle configuration without maps - all bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from jetson_slam_amd.rectify import undistort_rectify_map
from jetson_slam_amd.synth import synth_stereo_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- numpy restatement of the contract ----
def convert_ref(mapx, mapy):
    def fixed(m):
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.asarray(m, np.float32) * np.float32(32)
            ok = np.isfinite(f) & (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
        return np.where(ok, np.rint(np.where(ok, f, 0)).astype(np.float64), -2147483648.0).astype(np.int64)
    X, Y = fixed(mapx), fixed(mapy)
    xy = np.stack([np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    return xy, (((Y & 31) << 5) | (X & 31)).astype(np.uint16)


def remap_ref(src, xy, a):
    """out = (sum of in-source taps src * wx * wy + 512) >> 10, wx = {32 - fx, fx}, wy = {32 - fy, fy}"""
    H, W = src.shape
    ix, iy = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    a = a.astype(np.int64) & 1023
    fx, fy = a & 31, a >> 5
    acc = np.zeros(ix.shape, np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            sx, sy = ix + dx, iy + dy
            inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            v = src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64)
            acc += np.where(inside, v * wx * wy, 0)
    return ((acc + 512) >> 10).astype(np.uint8)


def remap_float(src, mapx, mapy):
    return remap_ref(src, *convert_ref(mapx, mapy))


def identity_maps(h, w):
    gy, gx = np.mgrid[0:h, 0:w]
    return gx.astype(np.float32), gy.astype(np.float32)


def calib_maps(h, w, right=False):
    """EuRoC-like made-up calibration scaled to the image size; the right camera differs (intrinsics, distortion, rotation)"""
    s = w / 752.0
    if not right:
        K = np.array([[458.7 * s, 0, 367.4 * s], [0, 457.3 * s, 248.6 * h / 480.0], [0, 0, 1]])
        D = [-0.283, 0.0741, 1.9e-4, 1.7e-5]
        ang = np.deg2rad([0.4, -0.7, 0.25])
    else:
        K = np.array([[457.6 * s, 0, 379.9 * s], [0, 456.1 * s, 255.2 * h / 480.0], [0, 0, 1]])
        D = [-0.284, 0.0745, -1.0e-4, -3.5e-5]
        ang = np.deg2rad([0.3, -0.5, 0.3])
    c, si = np.cos(ang), np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, c[0], -si[0]], [0, si[0], c[0]]])
    Ry = np.array([[c[1], 0, si[1]], [0, 1, 0], [-si[1], 0, c[1]]])
    Rz = np.array([[c[2], -si[2], 0], [si[2], c[2], 0], [0, 0, 1]])
    P = np.array([[435.2 * s, 0, 367.2 * s, 0], [0, 435.2 * s, 252.1 * h / 480.0, 0], [0, 0, 1, 0]])
    return undistort_rectify_map(K, D, Rz @ Ry @ Rx, P, w, h)


# ---- handles ----
def _mk(orb, c, max_batch=1):
    return orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=max_batch)


def _mko(po, c):
    return po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"], fast_n_min=9, fast_n_max=14,
                              th_fast_max=c["th"])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _outputs(g, c, image=0, levels=True):
    out = {"kp": g.keypoints(image), "desc": g.descriptors(image), "ang": g.angles(image).view(np.uint32).copy()}
    if levels:
        for lv in range(c["L"]):
            out["l%d" % lv] = g.level_image(lv, image)
            out["b%d" % lv] = g.level_image(lv, image, blurred=True)
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _stereo_single(orb, gl, gr, c):
    u, d, st = orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"])
    return u, d, {k: st[k] for k in ("n_candidate_pairs", "n_corr_match", "n_depth", "n_final")}


def _check_oracle(po, c, g, rect_l, rect_r, orb, gr=None, image=0, stereo=None):
    ol, orr = _mko(po, c), _mko(po, c)
    ol.extract(rect_l)
    if gr is not None:
        orr.extract(rect_r)
    assert np.array_equal(g.level_image(0, image), rect_l)
    assert g.n_keypoints(image) == ol.n
    assert np.array_equal(g.keypoints(image), ol.keypoints()) and np.array_equal(g.descriptors(image), ol.descriptors())
    if gr is not None:
        assert np.array_equal(gr.level_image(0, image), rect_r)
        assert np.array_equal(gr.keypoints(image), orr.keypoints()) and np.array_equal(gr.descriptors(image), orr.descriptors())
        u, d, st = stereo
        ou, od, ost = po.stereo_match(ol, orr, c["bf"] / c["fx"], c["bf"])
        assert _same_bits(u, ou) and _same_bits(d, od)
        for k in ("n_candidate_pairs", "n_corr_match", "n_depth", "n_final"):
            assert st[k] == ost[k]
        assert st["n_final"] > 10


# ---- identity maps: a no-op, bit for bit ----
@pytest.mark.parametrize("name", ["tiny", "c1", "c2", "c3"])
def test_identity_maps_single_frame_are_a_no_op(orb, configs, name):
    c = configs[name]
    l, r = synth_stereo_pair(3, c["h"], c["w"])
    mx, my = identity_maps(c["h"], c["w"])
    res = []
    for with_maps in (False, True):
        gl, gr = _mk(orb, c), _mk(orb, c)
        if with_maps:
            gl.set_rectify_maps(mx, my); gr.set_rectify_maps(mx, my)
            assert gl.rectify_enabled() and gr.rectify_enabled()
        frames = []
        for _ in range(3):                      # the single-frame graph: captured, then replayed
            gl.extract(l); gr.extract(r)
            frames.append((_outputs(gl, c), _outputs(gr, c), _stereo_single(orb, gl, gr, c)))
        for f in frames[1:]:
            _assert_same(f[0], frames[0][0]); _assert_same(f[1], frames[0][1])
        res.append(frames[0])
    (a_l, a_r, (au, ad, ast)), (b_l, b_r, (bu, bd, bst)) = res
    _assert_same(a_l, b_l); _assert_same(a_r, b_r)
    assert _same_bits(au, bu) and _same_bits(ad, bd) and ast == bst


def _extract_into(orb, torch, g, img, c):
    """jsorb_extract_into with caller-owned device destinations"""
    T = g.T
    kp_d = torch.zeros(6 * T, dtype=torch.int32, device="cuda")
    de_d = torch.zeros(32 * T, dtype=torch.uint8, device="cuda")
    img = np.ascontiguousarray(img)
    n = ctypes.c_int()
    g._chk(g._lib.jsorb_extract_into(g.handle, img.ctypes.data, img.strides[0], ctypes.byref(n), kp_d.data_ptr(), de_d.data_ptr()))
    torch.cuda.synchronize()
    return kp_d[:6 * n.value].cpu().numpy(), de_d[:32 * n.value].cpu().numpy()


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_identity_maps_extract_into_and_device_are_a_no_op(orb, configs, name):
    import torch
    c = configs[name]
    l, _ = synth_stereo_pair(4, c["h"], c["w"])
    mx, my = identity_maps(c["h"], c["w"])
    dev = torch.from_numpy(l).cuda()
    res = []
    for with_maps in (False, True):
        g = _mk(orb, c)
        if with_maps:
            g.set_rectify_maps(mx, my)
        into = _extract_into(orb, torch, g, l, c)
        n = ctypes.c_int()
        g._chk(g._lib.jsorb_extract_device(g.handle, dev.data_ptr(), c["w"], ctypes.byref(n)))
        res.append((into, _outputs(g, c)))
    assert np.array_equal(res[0][0][0], res[1][0][0]) and np.array_equal(res[0][0][1], res[1][0][1])
    _assert_same(res[0][1], res[1][1])


def _device_batch(orb, torch, c, B, lefts, rights, maps=None):
    gl, gr = _mk(orb, c, max_batch=B), _mk(orb, c, max_batch=B)
    if maps is not None:
        gl.set_rectify_maps(*maps[0]); gr.set_rectify_maps(*maps[1])
    ld, rd = torch.from_numpy(np.stack(lefts)).cuda(), torch.from_numpy(np.stack(rights)).cuda()
    gl.extract_batch_device_async(ld.data_ptr(), c["h"] * c["w"], c["w"], B, keep=ld)
    gr.extract_batch_device_async(rd.data_ptr(), c["h"] * c["w"], c["w"], B, keep=rd)
    orb.stereo_match_batch_async(gl, gr, c["bf"] / c["fx"], c["bf"])
    gl.sync(); gr.sync()
    return gl, gr


def test_identity_maps_device_batch_with_lanes_is_a_no_op(orb, configs):
    import torch
    c, B = configs["c2"], 64
    pairs = [synth_stereo_pair(100 + i, c["h"], c["w"]) for i in range(8)]
    lefts = [pairs[i % 8][0] for i in range(B)]
    rights = [pairs[i % 8][1] for i in range(B)]
    ident = identity_maps(c["h"], c["w"])
    a = _device_batch(orb, torch, c, B, lefts, rights)
    b = _device_batch(orb, torch, c, B, lefts, rights, maps=(ident, ident))
    assert a[0]._lib.jsorb_n_images(a[0].handle) == B
    for i in range(0, B, 7):
        _assert_same(_outputs(a[0], c, i, levels=i < 8), _outputs(b[0], c, i, levels=i < 8))
        _assert_same(_outputs(a[1], c, i, levels=False), _outputs(b[1], c, i, levels=False))
        ua, da, sa = orb.stereo_result(a[0], i)
        ub, db, sb = orb.stereo_result(b[0], i)
        assert _same_bits(ua, ub) and _same_bits(da, db) and sa == sb


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_identity_maps_host_batch_is_a_no_op(orb, configs, name):
    c, B = configs[name], 6
    imgs = np.stack([synth_stereo_pair(200 + i, c["h"], c["w"])[0] for i in range(B)])
    res = []
    for with_maps in (False, True):
        g = _mk(orb, c, max_batch=B)
        if with_maps:
            g.set_rectify_maps(*identity_maps(c["h"], c["w"]))
        g.extract_batch_host_async(imgs); g.sync()
        res.append([_outputs(g, c, i, levels=i < 2) for i in range(B)])
    for x, y in zip(*res):
        _assert_same(x, y)


# ---- non-trivial maps against the oracle on numpy-rectified images ----
@pytest.mark.parametrize("name", ["c2", "c3"])
def test_calibrated_maps_single_frame_match_oracle(orb, po, configs, name):
    c = configs[name]
    ml, mr = calib_maps(c["h"], c["w"]), calib_maps(c["h"], c["w"], right=True)
    gl, gr = _mk(orb, c), _mk(orb, c)
    gl.set_rectify_maps(*ml); gr.set_rectify_maps(*mr)
    for seed in (5, 6):
        l, r = synth_stereo_pair(seed, c["h"], c["w"])
        rl, rr = remap_float(l, *ml), remap_float(r, *mr)
        assert not np.array_equal(rl, l)
        gl.extract(l); gr.extract(r)
        _check_oracle(po, c, gl, rl, rr, orb, gr=gr, stereo=orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"]))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_calibrated_maps_batches_match_oracle(orb, po, configs, name):
    import torch
    c, B = configs[name], 16
    ml, mr = calib_maps(c["h"], c["w"]), calib_maps(c["h"], c["w"], right=True)
    pairs = [synth_stereo_pair(300 + i, c["h"], c["w"]) for i in range(B)]
    gl, gr = _device_batch(orb, torch, c, B, [p[0] for p in pairs], [p[1] for p in pairs], maps=(ml, mr))
    for i in (0, 5, B - 1):
        rl, rr = remap_float(pairs[i][0], *ml), remap_float(pairs[i][1], *mr)
        _check_oracle(po, c, gl, rl, rr, orb, gr=gr, image=i, stereo=orb.stereo_result(gl, i))
    # the host-streamed batch reads the same raw images from host memory
    hl = _mk(orb, c, max_batch=B)
    hl.set_rectify_maps(*ml)
    hl.extract_batch_host_async(np.stack([p[0] for p in pairs])); hl.sync()
    for i in (0, 9):
        _check_oracle(po, c, hl, remap_float(pairs[i][0], *ml), None, orb, image=i)


def test_fixed_point_entry_gives_the_float_entry_bits(orb, configs):
    c = configs["c2"]
    ml = calib_maps(c["h"], c["w"])
    xy, a = orb.convert_maps(*ml)
    rxy, ra = convert_ref(*ml)
    assert np.array_equal(xy, rxy) and np.array_equal(a, ra)
    l, _ = synth_stereo_pair(8, c["h"], c["w"])
    g1, g2 = _mk(orb, c), _mk(orb, c)
    g1.set_rectify_maps(*ml)
    g2.set_rectify_maps_fixed(xy, a | np.uint16(0xFC00))          # bits above the 10-bit index are ignored, as in OpenCV (masked)
    g1.extract(l); g2.extract(l)
    _assert_same(_outputs(g1, c), _outputs(g2, c))


@pytest.mark.parametrize("name", ["tiny", "c3"])
def test_maps_outside_the_source_give_zeros_and_partial_taps(orb, configs, name):
    c = configs[name]
    h, w = c["h"], c["w"]
    l, _ = synth_stereo_pair(9, h, w)
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float32)
    cases = [
        (gx - w / 2 - 0.3, gy + 0.4),                 # left half wholly outside, a partial column of taps at x = -1 / 0
        (gx + 0.25, gy - h * 0.75 + 0.6),             # most rows above the source
        (gx + 3 * w, gy),                             # everything outside: zeros
        (gx * 1.01 - 0.5, gy * 0.99 - 0.5),           # the border ring straddles the edge (two taps inside, two outside)
        (np.full_like(gx, -1e9), gy),                 # far out of range
    ]
    nanx = gx.copy(); nanx[::3, ::5] = np.nan        # NaN / inf entries: those pixels are 0
    nany = gy.copy(); nany[1::4, ::7] = np.inf
    cases.append((nanx, nany))
    g = _mk(orb, c)
    for mx, my in cases:
        mx, my = mx.astype(np.float32), my.astype(np.float32)
        g.set_rectify_maps(mx, my)
        g.extract(l)
        want = remap_float(l, mx, my)
        assert np.array_equal(g.level_image(0), want)
    g.set_rectify_maps(gx + 3 * w, gy)
    g.extract(l)
    assert not g.level_image(0).any() and g.n_keypoints(0) == 0


def test_permutation_map_takes_the_global_fallback_and_matches(orb, po, configs):
    """a random permutation of the source pixels defeats every tile's LDS box (k_rectify gathers its taps from global memory); the lower
    half of the second map is the identity (staged tiles) - both forms in one launch"""
    c = configs["c2"]
    h, w = c["h"], c["w"]
    rng = np.random.default_rng(11)
    perm = rng.permutation(h * w)
    px = (perm % w).astype(np.float32).reshape(h, w) + rng.integers(0, 32, (h, w)).astype(np.float32) / 32
    py = (perm // w).astype(np.float32).reshape(h, w) + rng.integers(0, 32, (h, w)).astype(np.float32) / 32
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float32)
    mixed_x, mixed_y = px.copy(), py.copy()
    mixed_x[h // 2:], mixed_y[h // 2:] = gx[h // 2:] + 0.5, gy[h // 2:] - 0.25
    l, r = synth_stereo_pair(12, h, w)
    for mx, my in ((px, py), (mixed_x, mixed_y)):
        g = _mk(orb, c)
        g.set_rectify_maps(mx, my)
        g.extract(l)
        _check_oracle(po, c, g, remap_float(l, mx, my), None, orb)
    # the same through a batch with lanes (all images share the map)
    import torch
    B = 24
    gl, gr = _device_batch(orb, torch, c, B, [l] * B, [r] * B, maps=((px, py), (mixed_x, mixed_y)))
    want_l, want_r = remap_float(l, px, py), remap_float(r, mixed_x, mixed_y)
    for i in (0, 11, B - 1):
        assert np.array_equal(gl.level_image(0, i), want_l) and np.array_equal(gr.level_image(0, i), want_r)


def test_clear_restores_unrectified_outputs(orb, configs):
    c = configs["c1"]
    l, r = synth_stereo_pair(13, c["h"], c["w"])
    ref = _mk(orb, c)
    ref.extract(l)
    want = _outputs(ref, c)
    g = _mk(orb, c)
    assert not g.rectify_enabled()
    g.extract(l)
    g.set_rectify_maps(*calib_maps(c["h"], c["w"]))
    g.extract(l)
    assert not np.array_equal(g.level_image(0), l)
    g.clear_rectify_maps()
    assert not g.rectify_enabled()
    for _ in range(2):
        g.extract(l)
        _assert_same(_outputs(g, c), want)


def test_maps_must_have_the_handle_size(orb, configs):
    c = configs["tiny"]
    g = _mk(orb, c)
    mx, my = identity_maps(c["h"] + 1, c["w"])
    with pytest.raises(orb.JsorbError):
        g.set_rectify_maps(mx, my)
    assert not g.rectify_enabled()


def test_maps_set_between_host_batches_in_flight(orb, configs):
    c, B = configs["c2"], 8
    imgs1 = np.stack([synth_stereo_pair(400 + i, c["h"], c["w"])[0] for i in range(B)])
    imgs2 = np.stack([synth_stereo_pair(500 + i, c["h"], c["w"])[0] for i in range(B)])
    mA, mB = calib_maps(c["h"], c["w"]), calib_maps(c["h"], c["w"], right=True)
    g = _mk(orb, c, max_batch=B)
    g.set_rectify_maps(*mA)
    g.extract_batch_host_async(imgs1)                 # in flight on landing buffer 0
    g.set_rectify_maps(*mB)                           # waits for it; the next batch lands in buffer 1 with the new maps
    for i in (0, B - 1):
        assert np.array_equal(g.level_image(0, i), remap_float(imgs1[i], *mA))
    first = [g.keypoints(i) for i in range(B)]
    g.extract_batch_host_async(imgs2)
    g.extract_batch_host_async(imgs1)                 # back to buffer 0, maps B
    g.sync()
    for i in (0, 3, B - 1):
        assert np.array_equal(g.level_image(0, i), remap_float(imgs1[i], *mB))
    ref = _mk(orb, c, max_batch=B)
    ref.set_rectify_maps(*mA)
    ref.extract_batch_host_async(imgs1); ref.sync()
    assert all(np.array_equal(first[i], ref.keypoints(i)) for i in range(B))


def test_rectify_kernel_timing(orb, configs):
    c = configs["c2"]
    l, _ = synth_stereo_pair(14, c["h"], c["w"])
    g = _mk(orb, c)
    g.set_rectify_maps(*calib_maps(c["h"], c["w"]))
    g.enable_kernel_timing(True)
    g.extract(l); g.extract(l)
    ms, n = g.rectify_kernel_time()
    assert n == 2 and ms > 0
    assert g.kernel_times()["k_pyramid"][1] == 2


def test_stereo_rectify_frame_example_matches_python(orb, configs, tmp_path):
    c = configs["c2"]
    exe = str(tmp_path / "stereo_rectify_frame")
    lib_dir = os.path.join(ROOT, "jetson_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "stereo_rectify_frame.cpp"),
                           "-L", lib_dir, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib_dir, "-o", exe])
    l, r = synth_stereo_pair(15, c["h"], c["w"])
    ml, mr = calib_maps(c["h"], c["w"]), calib_maps(c["h"], c["w"], right=True)
    files = []
    for name, arr in (("l.raw", l), ("r.raw", r), ("mxl", ml[0]), ("myl", ml[1]), ("mxr", mr[0]), ("myr", mr[1])):
        p = str(tmp_path / name)
        np.ascontiguousarray(arr).tofile(p)
        files.append(p)
    out = str(tmp_path / "out.bin")
    subprocess.check_call([exe, str(c["h"]), str(c["w"]), str(c["L"]), str(c["tile"]), str(c["th"]), str(c["fx"]), str(c["bf"])] + files + ["3", out],
                          timeout=300)
    blob = np.fromfile(out, np.uint8)
    nl, nr = np.frombuffer(blob[:8].tobytes(), np.int32)
    o = 8
    kl = np.frombuffer(blob[o:o + 24 * nl].tobytes(), np.int32); o += 24 * nl
    dl = blob[o:o + 32 * nl].reshape(nl, 32); o += 32 * nl
    kr = np.frombuffer(blob[o:o + 24 * nr].tobytes(), np.int32); o += 24 * nr
    dr = blob[o:o + 32 * nr].reshape(nr, 32); o += 32 * nr
    u = np.frombuffer(blob[o:o + 4 * nl].tobytes(), np.float32); o += 4 * nl
    d = np.frombuffer(blob[o:o + 4 * nl].tobytes(), np.float32)
    gl, gr = _mk(orb, c), _mk(orb, c)
    gl.set_rectify_maps(*ml); gr.set_rectify_maps(*mr)
    pk, pd = gl.extract(l)
    qk, qd = gr.extract(r)
    pu, pdp, _ = orb.compute_stereo_matches(gl, gr, c["bf"] / c["fx"], c["bf"])
    assert np.array_equal(kl, pk) and np.array_equal(dl, pd) and np.array_equal(kr, qk) and np.array_equal(dr, qd)
    assert _same_bits(u, pu) and _same_bits(d, pdp)
