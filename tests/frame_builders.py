"""Frame and point builders shared by the matchers' GPU tests and by tools/ref_matcher_goldens.py (through tests/ref_matcher_cases.py): a frame dict
in the vocabulary of the host tests from an extractor's accessors (the product's ORBExtractor on the device, or the oracle's extraction behind the
same accessors), and map points drawn next to its keypoints.  numpy only: nothing here needs a GPU.  Not a test module."""
import numpy as np

from test_search_local_host import build_grid

f32 = np.float32


def frame_of(g, c, u_right=None, blocked=None, cols=64, rows=48, bounds=None):
    kp = g.keypoints(0)
    n = len(kp) // 6
    xu, yu = g.keypoints_undistorted(0)
    min_x, max_x, min_y, max_y = bounds if bounds is not None else (f32(0), f32(c["w"]), f32(0), f32(c["h"]))
    inv_w, inv_h = f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y)
    grid, start, items = build_grid(xu, yu, min_x, min_y, inv_w, inv_h, cols, rows)
    return dict(kx=xu, ky=yu, octave=kp[4 * n:5 * n].astype(np.int64), desc=g.descriptors(0), grid=grid, start=start, items=items, cols=cols,
                rows=rows, min_x=f32(min_x), min_y=f32(min_y), inv_w=inv_w, inv_h=inv_h, scale=g.get_scale_factors(), mbf=f32(c["bf"]),
                u_right=u_right, blocked=blocked)


def points_near_keypoints(rng, F, n, n_levels, noise=2.0, desc_noise=0.06):
    """map points projected next to keypoints, with their descriptors a few bits off: most have a match, some conflict"""
    N = len(F["kx"])
    src = rng.integers(0, N, n)
    u = (F["kx"][src] + rng.normal(0, noise, n)).astype(np.float32)
    v = (F["ky"][src] + rng.normal(0, noise, n)).astype(np.float32)
    level = np.clip(F["octave"][src] + rng.integers(0, 2, n), 0, n_levels - 1).astype(np.int32)
    desc = F["desc"][src].copy()
    flip = rng.random((n, 32)) < desc_noise
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    view_cos = rng.choice(np.array([0.3, 0.99799996, 0.998, 0.9980001, 1.0], np.float32), n)
    if F["u_right"] is not None:
        ur = F["u_right"][src]
        invz = np.where(ur > 0, (u - ur) / F["mbf"], rng.uniform(0.05, 0.5, n)).astype(np.float32) + rng.normal(0, 0.01, n).astype(np.float32)
    else:
        invz = rng.uniform(0.05, 0.5, n).astype(np.float32)
    return dict(u=u, v=v, invz=invz.astype(np.float32), level=level, view_cos=view_cos, in_frustum=(rng.random(n) < 0.95).astype(np.uint8),
                desc=desc), src


def last_frame_of(g, c, u_right=None, bounds=None):
    F = frame_of(g, c, u_right=u_right, bounds=bounds)
    kp = g.keypoints(0)
    N = len(kp) // 6
    F["angle"] = kp[3 * N:4 * N].astype(np.int32).view(np.float32)
    return F


def params(c, F, th, direction=0, bounds=None, cam=None, retry_below=20, check_orientation=1, seed=0):
    """a current pose a little off the one the points were made with (points_of): K14 lands them next to their keypoints"""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 0.002, 3)
    R = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], np.float32)
    t = rng.normal(0, 0.01, 3).astype(np.float32)
    fx, fy, cx, cy = cam if cam is not None else (f32(c["fx"]), f32(c["fx"]), f32(c["w"] / 2), f32(c["h"] / 2))
    b = bounds if bounds is not None else (f32(0), f32(c["w"]), f32(0), f32(c["h"]))
    return dict(th=f32(th), th_high=100, check_orientation=check_orientation, direction=direction, retry_below=retry_below, fx=f32(fx), fy=f32(fy),
                cx=f32(cx), cy=f32(cy), min_x=f32(b[0]), max_x=f32(b[1]), min_y=f32(b[2]), max_y=f32(b[3]), Rcw=R, tcw=t)


def points_of(rng, F, prm, n, n_levels, outliers=0.3):
    """the last frame's map points: keypoints of this frame back-projected through the slightly perturbed pose of prm (sources drawn with
    replacement: keypoints chosen twice), descriptors a few bits off, octaves +-0..2, angles offset by one rotation plus ~30 % outliers"""
    N = len(F["kx"])
    src = rng.integers(0, N, n)
    z = rng.uniform(1.0, 15.0, n)
    Pc = np.stack([(F["kx"][src] + rng.normal(0, 1.0, n) - prm["cx"]) * z / prm["fx"], (F["ky"][src] + rng.normal(0, 1.0, n) - prm["cy"]) * z / prm["fy"], z])
    Pw = np.linalg.solve(prm["Rcw"].astype(np.float64), Pc - prm["tcw"].astype(np.float64)[:, None]).astype(np.float32)
    desc = F["desc"][src].copy()
    flip = rng.random((n, 32)) < 0.03
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    octave = np.clip(F["octave"][src] + rng.integers(-2, 3, n), 0, n_levels - 1).astype(np.int32)
    octave[rng.random(n) < 0.1] = 0
    off = np.where(rng.random(n) < outliers, rng.uniform(0, 360, n), f32(12.0)).astype(np.float32)
    angle = np.mod(F["angle"][src] + off, f32(360)).astype(np.float32)
    return dict(Px=Pw[0].copy(), Py=Pw[1].copy(), Pz=Pw[2].copy(), octave=octave, angle=angle, desc=desc), src
