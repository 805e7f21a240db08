"""Rectification maps for ORBExtractor.set_rectify_maps, for Python users without OpenCV.

The reference's stereo driver builds its maps with cv::initUndistortRectifyMap (Examples/Stereo/stereo_euroc.cpp:106-107) and remaps both
images on the host every frame (:145-146); libjsorb does the remap on the device once the maps are set on a handle.
"""
import numpy as np


def undistort_rectify_map(K, D, R, P, width, height):
    """(mapx, mapy) float32 (height, width): for every pixel (u, v) of the rectified image, the position in the raw image it is sampled from.

    The pinhole + radial-tangential model of OpenCV's initUndistortRectifyMap, written from its documented equations in float64:
        [X, Y, W]^T = (P[:3, :3] @ R)^-1 [u, v, 1]^T,  x = X / W,  y = Y / W,  r^2 = x^2 + y^2
        x'' = x (1 + k1 r^2 + k2 r^4 + k3 r^6) + 2 p1 x y + p2 (r^2 + 2 x^2)
        y'' = y (1 + k1 r^2 + k2 r^4 + k3 r^6) + p1 (r^2 + 2 y^2) + 2 p2 x y
        mapx = fx x'' + s y'' + cx,  mapy = fy y'' + cy      (fx, s, cx, fy, cy from K)
    K: 3x3 camera matrix of the raw camera, D: (k1, k2, p1, p2[, k3]), R: 3x3 rectifying rotation (None = identity), P: 3x3 or 3x4 new
    camera matrix (None = K).  Not claimed to be bit-identical to OpenCV's function (which evaluates in its own order and precision): the maps
    agree to well below a thousandth of a pixel (both are float32 in the end; this one is snapped to a 2^-20 px grid first), but a value that lands within rounding of a 1/32-pixel step can be converted differently.
    """
    K = np.asarray(K, np.float64).reshape(3, 3)
    d = np.zeros(5, np.float64)
    if D is not None:
        dv = np.asarray(D, np.float64).ravel()
        if dv.size not in (0, 4, 5):
            raise ValueError("D must hold (k1, k2, p1, p2[, k3])")
        d[:dv.size] = dv
    k1, k2, p1, p2, k3 = d
    R = np.eye(3) if R is None else np.asarray(R, np.float64).reshape(3, 3)
    Pk = K if P is None else np.asarray(P, np.float64)[:3, :3]
    iR = np.linalg.inv(Pk @ R)
    v, u = np.mgrid[0:height, 0:width].astype(np.float64)
    X = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    Y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    Wh = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    x, y = X / Wh, Y / Wh
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    mapx = K[0, 0] * xd + K[0, 1] * yd + K[0, 2]
    mapy = K[1, 1] * yd + K[1, 2]
    # float64 round-off of the inverse (~1e-13 px) would survive the float32 cast next to 0: the maps are snapped to a 2^-20 px grid first, so that
    # exact inputs give exact maps (R = I, P = K, D = 0 -> the pixel grid itself)
    q = float(1 << 20)
    return (np.round(mapx * q) / q).astype(np.float32), (np.round(mapy * q) / q).astype(np.float32)
