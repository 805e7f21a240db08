"""CPU-side checks of the rectification input stage: the float -> fixed-point map conversion of jsorb_rectify_convert_maps against a numpy
restatement of OpenCV's rule, its index layout, the numpy map builder (jetson_slam_amd.rectify) and the binding's new symbols.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orb():
    import __graft_entry__ as g
    g.build()
    from jetson_slam_amd import orb as _orb
    return _orb


def convert_ref(mapx, mapy):
    """OpenCV's float -> CV_16SC2 + CV_16UC1 conversion: X = round-half-even(m * 32), invalid (NaN, inf, outside int) -> INT_MIN,
    ix = saturate_int16(X >> 5), a = (Y & 31) << 5 | (X & 31)."""
    def fixed(m):
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.asarray(m, np.float32) * np.float32(32)        # exact in f32 (overflow -> inf -> invalid)
            ok = np.isfinite(f) & (f >= np.float32(-2147483648.0)) & (f < np.float32(2147483648.0))
        X = np.where(ok, np.rint(np.where(ok, f, 0)).astype(np.float64), -2147483648.0).astype(np.int64)
        return X
    X, Y = fixed(mapx), fixed(mapy)
    xy = np.stack([np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    a = (((Y & 31) << 5) | (X & 31)).astype(np.uint16)
    return xy, a


def _check(orb, mx, my):
    xy, a = orb.convert_maps(mx, my)
    rxy, ra = convert_ref(mx, my)
    assert np.array_equal(xy, rxy)
    assert np.array_equal(a, ra)
    return xy, a


def test_convert_random_maps(orb):
    rng = np.random.default_rng(5)
    mx = rng.uniform(-20, 800, (37, 53)).astype(np.float32)
    my = rng.uniform(-20, 500, (37, 53)).astype(np.float32)
    _check(orb, mx, my)


def test_convert_round_half_even_boundaries(orb):
    k = np.arange(-200, 200, dtype=np.float64)
    vals = np.concatenate([k / 32, k / 32 + 1 / 64, k / 32 - 1 / 64, k / 32 + 3 / 64]).astype(np.float32)
    mx = vals.reshape(16, -1)
    my = vals[::-1].copy().reshape(16, -1)
    xy, a = _check(orb, mx, my)
    # half-way cases go to the even 1/32 step: 1/64 -> 0, 3/64 -> 2/32, -1/64 -> 0
    xy1, a1 = orb.convert_maps(np.array([[1 / 64, 3 / 64, -1 / 64, 5 / 64]], np.float32), np.zeros((1, 4), np.float32))
    assert xy1[0, :, 0].tolist() == [0, 0, 0, 0] and (a1[0] & 31).tolist() == [0, 2, 0, 2]


def test_convert_negatives_below_zero_and_minus_one(orb):
    v = np.array([-1e-7, -1 / 64, -1 / 32, -0.5, -0.999, -1.0, -1.0 - 1 / 64, -1.0 - 1e-6, -1.02, -1.5, -2.0 + 1 / 128], np.float32)
    xy, a = _check(orb, v[None, :], v[::-1].copy()[None, :])
    # floor semantics of the arithmetic shift: -1/32 -> ix -1, fx 31
    xy2, a2 = orb.convert_maps(np.array([[-1 / 32]], np.float32), np.array([[0.0]], np.float32))
    assert xy2[0, 0, 0] == -1 and (a2[0, 0] & 31) == 31


def test_convert_out_of_range_nan_inf(orb):
    v = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 6.7e7, -6.7e7, 67108863.0, -67108864.0, 40000.0, -40000.0, 1024.0,
                  3.0e38, -3.0e38, 1023.97], np.float32)
    xy, a = _check(orb, v[None, :], np.flip(v).copy()[None, :])
    # an invalid coordinate is INT_MIN: ix saturates to -32768 and the fraction is 0
    xyn, an = orb.convert_maps(np.array([[np.nan]], np.float32), np.array([[np.inf]], np.float32))
    assert xyn[0, 0].tolist() == [-32768, -32768] and an[0, 0] == 0
    # in range but beyond int16 after the shift: saturated
    xys, _ = orb.convert_maps(np.array([[40000.0]], np.float32), np.array([[-40000.0]], np.float32))
    assert xys[0, 0].tolist() == [32767, -32768]


def test_fixed_point_round_trips_through_index_layout(orb):
    rng = np.random.default_rng(9)
    mx = rng.uniform(-3, 300, (20, 24)).astype(np.float32)
    my = rng.uniform(-3, 200, (20, 24)).astype(np.float32)
    xy, a = orb.convert_maps(mx, my)
    assert a.max() < 1024
    fx, fy = (a & 31).astype(np.float64), (a >> 5).astype(np.float64)
    back_x = xy[..., 0] + fx / 32
    back_y = xy[..., 1] + fy / 32
    assert np.all(np.abs(back_x - mx) <= 1 / 64 + 1e-6) and np.all(np.abs(back_y - my) <= 1 / 64 + 1e-6)
    # re-encoding the decoded value exactly reproduces the fixed point form
    xy2, a2 = orb.convert_maps(back_x.astype(np.float32), back_y.astype(np.float32))
    assert np.array_equal(xy2, xy) and np.array_equal(a2, a)


def test_convert_rejects_bad_arguments(orb):
    lib = orb.load_library()
    assert lib.jsorb_rectify_convert_maps(None, None, 4, None, None) != 0


def _euroc_like_calibration():
    # made-up numbers of the EuRoC kind (752 x 480 grey camera with strong barrel distortion, a small rectifying rotation)
    K = np.array([[458.7, 0.0, 367.4], [0.0, 457.3, 248.6], [0.0, 0.0, 1.0]])
    D = np.array([-0.283, 0.0741, 1.9e-4, 1.7e-5])
    ang = np.deg2rad([0.4, -0.7, 0.25])
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    P = np.array([[435.2, 0.0, 367.2, 0.0], [0.0, 435.2, 252.1, 0.0], [0.0, 0.0, 1.0, 0.0]])
    return K, D, R, P


def test_undistort_rectify_map_identity_is_the_pixel_grid():
    from jetson_slam_amd.rectify import undistort_rectify_map
    K = np.array([[458.7, 0.0, 367.4], [0.0, 457.3, 248.6], [0.0, 0.0, 1.0]])
    mx, my = undistort_rectify_map(K, np.zeros(5), np.eye(3), K, 752, 480)
    assert mx.dtype == np.float32 and mx.shape == (480, 752)
    gy, gx = np.mgrid[0:480, 0:752]
    assert np.array_equal(mx, gx.astype(np.float32)) and np.array_equal(my, gy.astype(np.float32))


def test_undistort_rectify_map_forward_projects_to_the_grid():
    from jetson_slam_amd.rectify import undistort_rectify_map
    K, D, R, P = _euroc_like_calibration()
    W, H = 752, 480
    mx, my = undistort_rectify_map(K, D, R, P, W, H)
    # forward: raw pixel -> normalised distorted -> undistort (fixed-point iteration) -> rotate by R -> project with P
    xd = (mx.astype(np.float64) - K[0, 2]) / K[0, 0]
    yd = (my.astype(np.float64) - K[1, 2]) / K[1, 1]
    k1, k2, p1, p2 = D
    x, y = xd.copy(), yd.copy()
    for _ in range(200):
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 * r2
        x = (xd - (2 * p1 * x * y + p2 * (r2 + 2 * x * x))) / rad
        y = (yd - (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)) / rad
    pts = np.stack([x, y, np.ones_like(x)], axis=-1) @ R.T
    pr = pts @ P[:3, :3].T
    u, v = pr[..., 0] / pr[..., 2], pr[..., 1] / pr[..., 2]
    gy, gx = np.mgrid[0:H, 0:W]
    assert np.max(np.abs(u - gx)) <= 1e-3 and np.max(np.abs(v - gy)) <= 1e-3
    # a non-trivial map: the corners move by many pixels
    assert abs(float(mx[0, 0]) - 0.0) > 5 and abs(float(my[H - 1, W - 1]) - (H - 1)) > 5


def test_rectify_module_never_imports_the_oracle():
    src = open(os.path.join(ROOT, "jetson_slam_amd", "rectify.py")).read()
    assert "oracle" not in src


def test_binding_exports_the_rectify_symbols(orb):
    names = ("jsorb_set_rectify_maps", "jsorb_set_rectify_maps_fixed", "jsorb_clear_rectify_maps", "jsorb_rectify_enabled", "jsorb_rectify_convert_maps")
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    for n in names:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr)
    for m in ("set_rectify_maps", "set_rectify_maps_fixed", "clear_rectify_maps", "rectify_enabled", "rectify_kernel_time"):
        assert callable(getattr(orb.ORBExtractor, m))
    # the kernel-timing id of k_rectify sits after the eight pipeline stages, which orb.KERNELS keeps listing
    lib.jsorb_kernel_name.restype = ctypes.c_char_p
    assert lib.jsorb_kernel_name(orb.K_RECTIFY) == b"k_rectify" and len(orb.KERNELS) == 8
    assert "JSORB_K_NMS_MS, JSORB_K_RECTIFY, JSORB_K_COUNT" in hdr
