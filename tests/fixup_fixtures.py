"""Shared by tests/test_fixup_rule_host.py and tests/test_gpu_fixup_stores.py: a numpy restatement of the certified fast paths and the exact chains of
k_blur (k_blur_body.h) and k_pyramid (k_pyramid.hip), and the images whose undecided pixels are of both kinds - the exact byte differs from the byte the
fast pass stored ("changed"), or it does not.  An exact-path pixel is stored only in the first case; the side bit that tells the two apart is restated
here as the kernels evaluate it (bit 7 of floor(256 A) mod 256)."""
import functools

import numpy as np

from jetson_slam_amd.synth import synth_stereo_pair
from oracle import host_restatement as hr

F32, F64 = np.float32, np.float64
BORDER = 20
H, W, LEVELS = 240, 320, 4          # geometry of the GPU test

# k_blur_body.h c_sep_v / c_sep_h
SEP_V = np.array([1.0, 0.99501247919268232, 0.98019867330675525, 0.95599748183309996], F32)
SEP_H = np.array([1.0 / 47.092777252197266, 0.99501247919268232 / 47.092777252197266, 0.98019867330675525 / 47.092777252197266,
                  0.95599748183309996 / 47.092777252197266]).astype(F32)


def _fma(a, b, c):
    """f32 fma through f64 (the product of two f32 values is exact in f64; one extra rounding far below every margin)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def fraction_rule(A, C):
    """-> (flagged, side, floor_a, stored_by_rule, floor_c): what the fast pass stores and flags, and the byte the fix-up lane infers it stored"""
    q = np.floor(A.astype(F64) * 256.0).astype(np.int64)                 # A + 49152 rounded down: low 16 mantissa bits
    frac, floor_a = q & 0xFF, q >> 8
    flagged = (frac == 0) | (frac == 255)
    side = frac >> 7
    return flagged, side, floor_a, np.rint(C).astype(np.int64) - side, np.floor(C).astype(np.int64)


# ---- k_blur ----
def blur_windows(P, up=False):
    """P: (n, 7, 7) uint8 windows -> (A, C); `up`: the vertical stage runs bottom row first (odd bands walk up)"""
    w = hr.CtorTables._gauss().reshape(7, 7).astype(F32)
    Pf = P.astype(F32)
    C = np.zeros(P.shape[0], F32)
    for j in range(7):
        for k in range(7):
            C = _fma(np.full(1, w[j, k], F32), Pf[:, j, k], C)
    gh = np.array([SEP_H[abs(k)] for k in range(-3, 4)], F32)
    gv = np.array([SEP_V[abs(j)] for j in range(-3, 4)], F32)
    Hs = np.zeros((P.shape[0], 7), F32)
    for k in range(7):
        Hs = _fma(np.full(1, gh[k], F32), Pf[:, :, k], Hs)
    A = np.zeros(P.shape[0], F32)
    for j in (range(6, -1, -1) if up else range(7)):
        A = _fma(np.full(1, gv[j], F32), Hs[:, j], A)
    return A, C


def blur_plane(img, up=False):
    """(A, C) of every ROI pixel [20, H-20) x [20, W-20) of a plane, as planes of the ROI's shape"""
    h, w = img.shape
    win = np.lib.stride_tricks.sliding_window_view(img, (7, 7))[BORDER - 3:h - BORDER - 3, BORDER - 3:w - BORDER - 3]
    A, C = blur_windows(win.reshape(-1, 7, 7), up)
    return A.reshape(h - 2 * BORDER, w - 2 * BORDER), C.reshape(h - 2 * BORDER, w - 2 * BORDER)


@functools.lru_cache(None)
def flat_levels():
    """-> (grey levels whose flat window's exact byte differs from the fast pass's byte, the others): every flat window is undecided"""
    P = np.arange(256, dtype=np.uint8).reshape(-1, 1, 1).repeat(7, 1).repeat(7, 2)
    changed = np.zeros(256, bool)
    for up in (False, True):
        flagged, _, floor_a, _, floor_c = fraction_rule(*blur_windows(P, up))
        assert flagged.all()
        ch = floor_a != floor_c
        assert up is False or np.array_equal(ch, changed)      # both walking directions agree on flat windows
        changed = ch
    return tuple(np.flatnonzero(changed)), tuple(np.flatnonzero(~changed))


# ---- k_pyramid ----
def level_geometry(h0, w0, n_levels, sf):
    """[(h, w, s)] of levels 1 .. n_levels - 1, in the f32 arithmetic of the library's build_geometry"""
    scale, out = F32(1), []
    for _ in range(1, n_levels):
        scale = F32(F32(sf) * scale)
        inv = F32(F32(1) / scale)
        out.append((int(F32(h0) * inv), int(F32(w0) * inv), F32(F32(1) / inv)))
    return out


def bilinear_weights(s, n):
    """wl, wr (or wyt, wyb) of coordinates 0 .. n - 1 and the left (top) tap index"""
    f = (F32(s) * np.arange(n, dtype=F32)).astype(F32)
    lo = np.floor(f)
    wl = ((lo + F32(1)) - f).astype(F32)
    return wl, (F32(1) - wl).astype(F32), lo.astype(np.int64)


def pyramid_taps(wxl, wxr, wyt, wyb, tl, tr, bl, br):
    """-> (A, C, needs_certificate) of pixels given by their weights and taps (f32 arrays of one shape)"""
    C = ((wxr * wyt).astype(F32) * tr).astype(F32)
    for wgt, p in (((wxl * wyt).astype(F32), tl), ((wxl * wyb).astype(F32), bl), ((wxr * wyb).astype(F32), br)):
        C = _fma(wgt, p, C)
    t = _fma(wxl, tl, (wxr * tr).astype(F32))
    b = _fma(wxl, bl, (wxr * br).astype(F32))
    A = _fma(wyb, b, (wyt * t).astype(F32))
    return A, C, (wxr != 0) & (wyb != 0)            # rows with wyb == 0 and columns with wxr == 0 are masked out in the kernel: A is the chain's value


def pyramid_level(img, h, w, s):
    """(A, C, needs_certificate) of one level (h x w, level scale s) resampled from level 0"""
    h0, w0 = img.shape
    wl, wr, xl = bilinear_weights(s, w)
    wt, wb, yt = bilinear_weights(s, h)
    f = img.astype(F32)
    xr, yb = np.minimum(xl + 1, w0 - 1), np.minimum(yt + 1, h0 - 1)      # (a tap past the plane only ever meets a zero weight)
    g = lambda yy, xx: f[yy[:, None], xx[None, :]]
    B = lambda v, axis: np.broadcast_to(v[:, None] if axis == 0 else v[None, :], (h, w)).astype(F32)
    return pyramid_taps(B(wl, 1), B(wr, 1), B(wt, 0), B(wb, 0), g(yt, xl), g(yt, xr), g(yb, xl), g(yb, xr))


# ---- the images of the GPU test ----
def texture(seed=1):
    return synth_stereo_pair(seed, H, W)[0]


def squares():
    """the texture with 40 flat 9 x 9 squares (a 3 x 3 core of exactly flat windows each), grey levels alternating between the two sets; their rows fall
    into even and into odd blur bands of 16 and of 8 rows: sparse changed pixels on the listed path, in bands walking both ways"""
    changed, same = flat_levels()
    img = texture(1).copy()
    n = 0
    for i in range(5):
        for j in range(8):
            y0, x0 = 24 + 40 * i, 24 + 36 * j
            img[y0:y0 + 9, x0:x0 + 9] = changed[(7 * n) % len(changed)] if n % 2 == 0 else same[(11 * n) % len(same)]
            n += 1
    return img


def square_core_rows():
    return [24 + 40 * i + 4 for i in range(5)]


def mosaic():
    """40 x 40 flat blocks cycling through grey levels of both sets: most windows flat, the dense exact paths"""
    changed, same = flat_levels()
    img = np.zeros((H, W), np.uint8)
    n = 0
    for i in range(H // 40):
        for j in range(W // 40):
            img[40 * i:40 * i + 40, 40 * j:40 * j + 40] = changed[(5 * n) % len(changed)] if n % 2 == 0 else same[(3 * n) % len(same)]
            n += 1
    return img


def pm1_noise():
    rng = np.random.default_rng(120)
    return (120 + rng.integers(-1, 2, (H, W))).astype(np.uint8)


def images():
    return {"squares": squares(), "mosaic": mosaic(), "pm1_noise": pm1_noise(), "texture": texture(1)}


def other_image():
    """what is extracted in between two runs of one image on the same handle"""
    return synth_stereo_pair(9, H, W)[1]
