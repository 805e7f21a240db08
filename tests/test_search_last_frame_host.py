"""CPU: the motion-model matcher of jsorb_search_last_frame (include/jsorb.h) - the GPU branch of ORBmatcher::SearchByProjection(CurrentFrame,
LastFrame, th, bMono) (ORBmatcher.cpp:1647-1963) with the invz variant of Frame::GetFeaturesInArea (Frame.cpp:569-639), ComputeThreeMaxima
(ORBmatcher.cpp:2097-2138) and TrackWithMotionModel's retry (Tracking.cpp:1056-1064).  A literal, sequential float32 transcription is the yardstick
(K14 through the oracle's orc_project_points); the numpy restatement of what the kernels compute (a parallel best over the CSR, the max-owner per
keypoint, an integer histogram, the culled set) must equal it on random cases, keypoints chosen by several points across culled and kept bins, exact
distance ties, every direction with octave 0, rotations exactly at k + 0.5 bins, ComputeThreeMaxima ties and its 0.1 cut, and the retry boundary.
tests/test_gpu_search_last_frame.py holds the device to both."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_search_local_host import _roundf, _to_int, build_grid, popcount_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HISTO_LENGTH = 30


def k14(po, P, prm):
    """ORB_Search_by_projection_project_on_GPU through the oracle (jsorb_oracle.c: orc_project_points): u, v, invz, is_valid"""
    n = len(P["Px"])
    u, v, z = (np.zeros(max(n, 1), np.float32) for _ in range(3))
    ok = np.zeros(max(n, 1), np.uint8)
    Px, Py, Pz = (np.ascontiguousarray(P[k], np.float32) for k in ("Px", "Py", "Pz"))
    R, t = np.ascontiguousarray(prm["Rcw"], np.float32).ravel(), np.ascontiguousarray(prm["tcw"], np.float32).ravel()
    if n:
        po.lib().orc_project_points(n, Px.ctypes.data, Py.ctypes.data, Pz.ctypes.data, R.ctypes.data, t.ctypes.data, *(float(prm[k]) for k in (
            "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y")), u.ctypes.data, v.ctypes.data, z.ctypes.data, ok.ctypes.data)
    return u[:n], v[:n], z[:n], ok[:n]


def level_window(direction, oct):
    """ORBmatcher.cpp:1801-1810: (minLevel, maxLevel) of the GetFeaturesInArea call"""
    return (oct, -1) if direction > 0 else (0, oct) if direction < 0 else (oct - 1, oct + 1)


def rot_bin(last, cur):
    """ORBmatcher.cpp:1918-1929 (bins outside [0, 30) - angles outside [0, 360) - are HISTO_LENGTH: never kept)"""
    rot = f32(f32(last) - f32(cur))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = _to_int(_roundf(f32(rot * (f32(1.0) / f32(HISTO_LENGTH)))))
    if b == HISTO_LENGTH:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else HISTO_LENGTH


def compute_three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cpp:2097-2138)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(HISTO_LENGTH):
        s = sizes[i]
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif f32(max3) < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


# The rotation check at its edges, the same inputs through every matcher that has one (the GPU tests of each): the rotations (angle of the point's
# side - angle of the frame's keypoint, the latter 0) of up to 40 matches, in match order.
ROTATION_CULL = {
    "four_equal_bins": [33.0] * 10 + [63.0] * 10 + [93.0] * 10 + [123.0] * 10,      # bins 1..4, ten each: the three earliest stay, the fourth goes
    "ten_and_one": [3.0] * 10 + [153.0],                                            # (float)1 < 0.1f * 10 is false: the lone one stays
    "eleven_and_one": [3.0] * 11 + [153.0],                                         # 1 < 0.1f * 11: it goes
    "outside_360": [3.0] * 5 + [1000.0],                                            # bin 33 -> HISTO_LENGTH: never kept
}


def rotation_cull_expected(rots, check_orientation=1):
    """(kept_bins, which of the matches stay) from rot_bin and compute_three_maxima"""
    bins = [rot_bin(r, 0.0) for r in rots]
    if not check_orientation:
        return (-1, -1, -1), np.ones(len(rots), bool)
    ind = compute_three_maxima(np.bincount(bins, minlength=HISTO_LENGTH + 1))
    return ind, np.array([b in ind for b in bins])


def test_rotation_cull_cases_are_what_they_say():
    want = {"four_equal_bins": ((1, 2, 3), 30), "ten_and_one": ((0, 5, -1), 11), "eleven_and_one": ((0, -1, -1), 11), "outside_360": ((0, -1, -1), 5)}
    for name, rots in ROTATION_CULL.items():
        ind, kept = rotation_cull_expected(rots)
        assert (ind, int(kept.sum())) == want[name] and len(rots) <= 40, name
        assert rotation_cull_expected(rots, 0)[1].all()


# ---- the yardstick: a literal transcription of the GPU branch, sequential, float32 ----
def get_features_in_area_invz(F, x, y, invzc, r, min_level, max_level):
    """Frame::GetFeaturesInArea(x, y, invzc, r, indices, minLevel, maxLevel) (Frame.cpp:569-639) with mvpMapPoints all NULL"""
    x, y, invzc, r = f32(x), f32(y), f32(invzc), f32(r)
    idx = []
    nMinCellX = max(0, _to_int(np.floor(f32(f32(f32(x - F["min_x"]) - r) * F["inv_w"]))))
    if nMinCellX >= F["cols"]:
        return idx
    nMaxCellX = min(F["cols"] - 1, _to_int(np.ceil(f32(f32(f32(x - F["min_x"]) + r) * F["inv_w"]))))
    if nMaxCellX < 0:
        return idx
    nMinCellY = max(0, _to_int(np.floor(f32(f32(f32(y - F["min_y"]) - r) * F["inv_h"]))))
    if nMinCellY >= F["rows"]:
        return idx
    nMaxCellY = min(F["rows"] - 1, _to_int(np.ceil(f32(f32(f32(y - F["min_y"]) + r) * F["inv_h"]))))
    if nMaxCellY < 0:
        return idx
    bCheckLevels = min_level > 0 or max_level >= 0
    for ix in range(nMinCellX, nMaxCellX + 1):
        for iy in range(nMinCellY, nMaxCellY + 1):
            for k in F["grid"][ix][iy]:
                if bCheckLevels:
                    if F["octave"][k] < min_level:
                        continue
                    if max_level >= 0 and F["octave"][k] > max_level:
                        continue
                distx = f32(F["kx"][k] - x)
                disty = f32(F["ky"][k] - y)
                if abs(distx) < r and abs(disty) < r:
                    if F["u_right"] is not None and F["u_right"][k] > 0:
                        ur = f32(x - f32(F["mbf"] * invzc))
                        er = abs(f32(ur - F["u_right"][k]))
                        if er > r:
                            continue
                    idx.append(k)
    return idx


def search_by_projection_last(po, F, P, prm, th):
    """one call of the GPU branch (ORBmatcher.cpp:1647-1963): (match, dist, kp_match, nmatches, to_be_matched_count, (ind1, ind2, ind3))"""
    n, N = len(P["Px"]), len(F["kx"])
    u, v, invz, is_valid = k14(po, P, prm)
    nbr = [[] for _ in range(n)]
    to_be_matched_count = 0
    for i in range(n):
        if is_valid[i]:
            oct = int(P["octave"][i])
            if oct < 0 or oct >= len(F["scale"]):         # outside the contract (mvScaleFactors would be read out of bounds)
                continue
            radius = f32(f32(th) * F["scale"][oct])
            lo, hi = level_window(prm["direction"], oct)
            nbr[i] = get_features_in_area_invz(F, u[i], v[i], invz[i], radius, lo, hi)
            to_be_matched_count += len(nbr[i])
    mvpMapPoints = np.full(N, -1, np.int64)
    match = np.full(n, -1, np.int64)
    mdist = np.full(n, -1, np.int64)
    rotHist = [[] for _ in range(HISTO_LENGTH + 1)]
    nmatches = 0
    for i in range(n):
        bestDist, bestIdx2 = 256, -1
        for k in nbr[i]:
            dist = popcount_dist(P["desc"][i], F["desc"][k])
            if dist < bestDist:
                bestDist, bestIdx2 = dist, k
        if bestDist <= prm["th_high"]:
            mvpMapPoints[bestIdx2] = i
            nmatches += 1
            match[i], mdist[i] = bestIdx2, bestDist
            if prm["check_orientation"]:
                rotHist[rot_bin(P["angle"][i], F["angle"][bestIdx2])].append(bestIdx2)
    ind = (-1, -1, -1)
    if prm["check_orientation"]:
        ind = compute_three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH + 1):
            if b not in ind:
                for k in rotHist[b]:
                    mvpMapPoints[k] = -1
                    nmatches -= 1
    return match, mdist, mvpMapPoints, nmatches, to_be_matched_count, ind


def track_with_motion_model(po, F, P, prm, search=search_by_projection_last):
    """Tracking.cpp:1045-1064: a pass at th, and from scratch at 2 th when it found fewer than retry_below; + the number of passes"""
    r = search(po, F, P, prm, f32(prm["th"]))
    if prm["retry_below"] > 0 and r[3] < prm["retry_below"]:
        return search(po, F, P, prm, f32(2 * f32(prm["th"]))) + (2,)
    return r + (1,)


# ---- the restatement of the kernels ----
def search_last_restated(po, F, P, prm, th):
    """k_last_match: per point the minimum of (distance << 18 | CSR position) over the window's CSR ranges, the max point index per chosen keypoint,
    the point's bin; k_last_resolve: integer histogram, ComputeThreeMaxima, kp_match = owner with culled entries' keypoints nulled"""
    n, N = len(P["Px"]), len(F["kx"])
    u, v, invz, is_valid = k14(po, P, prm)
    start, items, rows, cols = F["start"], F["items"], F["rows"], F["cols"]
    kx, ky, octv = np.asarray(F["kx"], np.float32), np.asarray(F["ky"], np.float32), np.asarray(F["octave"], np.int64)
    bits = np.unpackbits(np.asarray(F["desc"], np.uint8), axis=1) if N else np.zeros((0, 256), np.uint8)
    match = np.full(n, -1, np.int64)
    mdist = np.full(n, -1, np.int64)
    pbin = np.full(n, -1, np.int64)
    owner = np.full(N, -1, np.int64)
    cand = 0
    for i in range(n):
        L = int(P["octave"][i])
        if not is_valid[i] or L < 0 or L >= len(F["scale"]):
            continue
        R = f32(f32(th) * F["scale"][L])
        x, y = f32(u[i]), f32(v[i])
        x0 = max(0, _to_int(np.floor(f32(f32(x - F["min_x"]) - R) * F["inv_w"])))
        x1 = min(cols - 1, _to_int(np.ceil(f32(f32(x - F["min_x"]) + R) * F["inv_w"])))
        y0 = max(0, _to_int(np.floor(f32(f32(y - F["min_y"]) - R) * F["inv_h"])))
        y1 = min(rows - 1, _to_int(np.ceil(f32(f32(y - F["min_y"]) + R) * F["inv_h"])))
        if x0 >= cols or x1 < 0 or y0 >= rows or y1 < 0:
            continue
        js = np.concatenate([np.arange(start[ix * rows + y0], start[ix * rows + y1 + 1]) for ix in range(x0, x1 + 1)]).astype(np.int64)
        ks = items[js].astype(np.int64)
        lo, hi = level_window(prm["direction"], L)
        ok = (np.abs(kx[ks] - x) < R) & (np.abs(ky[ks] - y) < R)
        if lo > 0 or hi >= 0:
            ok &= (octv[ks] >= lo) & ((hi < 0) | (octv[ks] <= hi))
        if F["u_right"] is not None:
            ur = np.asarray(F["u_right"], np.float32)[ks]
            xr = f32(x - f32(f32(F["mbf"]) * f32(invz[i])))
            with np.errstate(invalid="ignore"):
                ok &= ~((ur > 0) & (np.abs(xr - ur) > R))
        js, ks = js[ok], ks[ok]
        cand += len(ks)
        if not len(ks):
            continue
        d = (bits[ks] != np.unpackbits(np.asarray(P["desc"][i], np.uint8))).sum(1).astype(np.int64)
        key = int((d << 18 | js).min())
        if (key >> 18) < 256 and (key >> 18) <= prm["th_high"]:
            k = int(items[key & ((1 << 18) - 1)])
            match[i], mdist[i] = k, key >> 18
            owner[k] = max(owner[k], i)
            if prm["check_orientation"]:
                pbin[i] = rot_bin(P["angle"][i], F["angle"][k])
    matched = match >= 0
    ind = (-1, -1, -1)
    kp_match = owner.copy()
    culled = 0
    if prm["check_orientation"]:
        hist = np.bincount(pbin[matched], minlength=HISTO_LENGTH + 1)
        ind = compute_three_maxima(hist)
        cut = matched & ~np.isin(pbin, [b for b in ind if b >= 0])
        kp_match[match[cut]] = -1
        culled = int(cut.sum())
    return match, mdist, kp_match, int(matched.sum()) - culled, cand, ind


# ---- random cases ----
def half_bin_rotations():
    """float32 rotations whose rot * (1.0f/30) is exactly k + 0.5 (k = 0..11): roundf takes them away from zero"""
    factor = f32(1.0) / f32(HISTO_LENGTH)
    out = []
    for k in range(12):
        r = f32((k + 0.5) * 30)
        for c in (r, np.nextafter(r, f32(0)), np.nextafter(r, f32(1e9))):
            if f32(c * factor) == f32(k + 0.5):
                out.append(f32(c))
    return np.array(out, np.float32)


def random_case(rng, mono=False, dense=False):
    W, H = 320, 240
    n_levels = int(rng.integers(1, 9))
    scale = np.ones(n_levels, np.float32)
    for l in range(1, n_levels):
        scale[l] = f32(scale[l - 1] * f32(1.2))
    N = int(rng.integers(0, 140))
    kx = rng.uniform(-5, W + 5, N).astype(np.float32)
    ky = rng.uniform(-5, H + 5, N).astype(np.float32)
    if rng.random() < 0.5:
        kx, ky = np.round(kx).astype(np.float32), np.round(ky).astype(np.float32)
    octave = rng.integers(0, n_levels, N)
    octave[rng.random(N) < 0.3] = 0
    angle = rng.choice(np.array([0, 10, 90, 180, 359.5], np.float32), N) if rng.random() < 0.5 else rng.uniform(0, 360, N).astype(np.float32)
    pool = rng.integers(0, 256, (5, 32), dtype=np.uint8)                  # few distinct descriptors: exact distance ties
    desc = pool[rng.integers(0, 5, N)].copy() if N else np.zeros((0, 32), np.uint8)
    flip = rng.random((N, 32)) < 0.04
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    cols, rows = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    min_x, max_x, min_y, max_y = f32(rng.uniform(-5, 2)), f32(W + rng.uniform(-3, 5)), f32(rng.uniform(-5, 2)), f32(H + rng.uniform(-3, 5))
    inv_w, inv_h = f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y)
    grid, start, items = build_grid(kx, ky, min_x, min_y, inv_w, inv_h, cols, rows)
    mbf = f32(rng.uniform(20, 60))
    u_right = None
    if not mono and N:
        u_right = (kx - rng.uniform(-2, 30, N)).astype(np.float32)
        u_right[rng.random(N) < 0.3] = f32(-1)
    F = dict(kx=kx, ky=ky, octave=octave, angle=angle, desc=desc, grid=grid, start=start, items=items, cols=cols, rows=rows, min_x=min_x,
             min_y=min_y, inv_w=inv_w, inv_h=inv_h, scale=scale, mbf=mbf, u_right=u_right)
    fx, fy, cx, cy = f32(rng.uniform(150, 400)), f32(rng.uniform(150, 400)), f32(W / 2 + rng.uniform(-5, 5)), f32(H / 2 + rng.uniform(-5, 5))
    a = rng.normal(0, 0.01, 3)
    Rcw = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], np.float64)
    tcw = rng.normal(0, 0.05, 3)
    n = int(rng.integers(0, 80 if not dense else 40))
    src = rng.integers(0, max(N, 1), n)
    su = (kx[src] if N else rng.uniform(0, W, n)) + rng.normal(0, 2.0, n)
    sv = (ky[src] if N else rng.uniform(0, H, n)) + rng.normal(0, 2.0, n)
    z = rng.uniform(0.5, 20, n)
    if u_right is not None:                                              # depth that agrees with uRight where there is one: the gate passes and fails
        disp = su - u_right[src]
        z = np.where((u_right[src] > 0) & (disp > 0.5), mbf / np.maximum(disp, 0.5), z) * rng.choice([1.0, 1.02, 1.5], n)
    Pc = np.stack([(su - cx) * z / fx, (sv - cy) * z / fy, z])
    Pw = np.linalg.solve(Rcw, Pc - tcw[:, None]).astype(np.float32)
    Pw[:, rng.random(n) < 0.05] *= -1                                    # some behind the camera
    oct_p = (octave[src] if N else rng.integers(0, n_levels, n)) + rng.integers(-2, 3, n)
    oct_p = np.clip(oct_p, 0, n_levels - 1)
    oct_p[rng.random(n) < 0.3] = 0
    oct_p[rng.random(n) < 0.04] = rng.choice([-1, n_levels, -(2 ** 31)])   # outside the contract: no candidate
    halves = half_bin_rotations()
    base = angle[src] if N else rng.uniform(0, 360, n).astype(np.float32)
    offs = rng.choice(np.concatenate([np.array([0, 1, 45, 60, 200], np.float32), halves]), n) if rng.random() < 0.7 else \
        rng.choice(np.array([0, 5, 14.9], np.float32), n)              # mostly one rotation: ComputeThreeMaxima's 0.1 cut
    pangle = np.mod(base + offs, f32(360)).astype(np.float32)
    pdesc = desc[src].copy() if N else rng.integers(0, 256, (n, 32), dtype=np.uint8)
    noise = rng.random((n, 32)) < 0.05
    pdesc[noise] ^= rng.integers(1, 256, int(noise.sum()), dtype=np.uint8)
    far = rng.random(n) < 0.05
    pdesc[far] = ~pdesc[far]
    P = dict(Px=Pw[0].copy(), Py=Pw[1].copy(), Pz=Pw[2].copy(), octave=oct_p.astype(np.int32), angle=pangle, desc=pdesc)
    prm = dict(th=f32(rng.choice([3, 7, 15])), th_high=100, check_orientation=int(rng.random() < 0.85), direction=int(rng.integers(-1, 2)),
               retry_below=int(rng.choice([0, 20, 5])), fx=fx, fy=fy, cx=cx, cy=cy, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y,
               Rcw=Rcw.astype(np.float32), tcw=tcw.astype(np.float32))
    return F, P, prm


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("part", range(4))
def test_kernels_formulation_equals_the_sequential_reference(po, part):
    rng = np.random.default_rng(100 + part)
    seen = dict(matches=0, shared=0, shared_culled=0, culled=0, cut=0, tie=0, half=0, retried=0, oct0=set(), mono=0)
    halves = set(half_bin_rotations().tolist())
    for case in range(500):
        F, P, prm = random_case(rng, mono=case % 5 == 0, dense=case % 3 == 0)
        ref = track_with_motion_model(po, F, P, prm)
        res = track_with_motion_model(po, F, P, prm, search_last_restated)
        assert _same(ref, res), case
        m, d, km, cnt, cand, ind, passes = ref
        seen["matches"] += cnt
        seen["retried"] += passes == 2
        seen["mono"] += F["u_right"] is None and cnt > 0
        mk = m[m >= 0]
        dup = np.unique(mk)[np.bincount(mk)[np.unique(mk)] > 1] if len(mk) else []
        seen["shared"] += len(dup)
        seen["culled"] += int(((km == -1) & np.isin(np.arange(len(km)), mk)).sum())
        seen["shared_culled"] += int(sum(km[k] == -1 for k in dup))
        seen["cut"] += prm["check_orientation"] and ind[1] == -1 and len(mk) > 0
        seen["tie"] += len(mk) > 1 and len(set(d[m >= 0].tolist())) < len(mk)
        seen["half"] += sum(float(f32(f32(P["angle"][i]) - f32(F["angle"][m[i]]))) % 360 in halves for i in np.nonzero(m >= 0)[0])
        for i in np.nonzero(m >= 0)[0]:
            if P["octave"][i] == 0:
                seen["oct0"].add(prm["direction"])
    # not vacuous: matches, keypoints chosen twice (culled and kept), cuts, ties, half bins, retries, every direction at octave 0
    assert seen["matches"] > 2000 and seen["shared"] > 50 and seen["shared_culled"] > 5 and seen["culled"] > 50, seen
    assert seen["cut"] > 10 and seen["tie"] > 50 and seen["half"] > 5 and seen["retried"] > 10 and seen["mono"] > 20, seen
    assert seen["oct0"] == {-1, 0, 1}, seen


def test_retry_boundary(po):
    """retry_below = first-pass count - 1, count, count + 1 around 19 / 20 / 21: the second pass runs only below"""
    rng = np.random.default_rng(7)
    hit = set()
    for case in range(400):
        F, P, prm = random_case(rng)
        prm["retry_below"] = 0
        c1 = search_last_restated(po, F, P, prm, prm["th"])[3]
        if c1 not in (19, 20, 21):
            continue
        for rb in (19, 20, 21):
            prm["retry_below"] = rb
            ref = track_with_motion_model(po, F, P, prm)
            assert _same(ref, track_with_motion_model(po, F, P, prm, search_last_restated))
            assert ref[-1] == (2 if c1 < rb else 1)
            if c1 < rb:
                assert _same(ref[:-1], search_by_projection_last(po, F, P, prm, f32(2 * prm["th"])))
        hit.add(c1)
    assert hit == {19, 20, 21}, hit


def test_compute_three_maxima_ties_and_cut():
    h = [0] * 30
    assert compute_three_maxima(h) == (-1, -1, -1)
    h[3], h[5], h[7] = 4, 4, 4
    assert compute_three_maxima(h) == (3, 5, 7)                  # strict >: the earlier bin wins a tie
    h = [0] * 30
    h[2], h[9], h[11] = 20, 2, 1
    assert compute_three_maxima(h) == (2, 9, -1)                # 1 < 0.1 * 20
    h[9] = 1
    assert compute_three_maxima(h) == (2, -1, -1)               # 1 < 2: ind2 and ind3 go
    assert rot_bin(10, 10) == 0 and rot_bin(0, 15) == 12 and rot_bin(f32(345.0), 0) == 12 and rot_bin(f32(344.99), 0) == 11


def test_header_binding_and_enum_declare_the_new_entry_points(orb):
    names = ("jsorb_search_last_frame_async", "jsorb_search_last_frame", "jsorb_search_last_frame_stats")
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    src = open(orb.__file__).read()
    for n in names:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    assert "enum { JSORB_K_LAST_MATCH = JSORB_K_ID_END, JSORB_K_LAST_RESOLVE, JSORB_K_ID_COUNT };" in hdr
    assert "enum { JSORB_K_ASSIGN_GRID = JSORB_K_COUNT_ALL + 1, JSORB_K_LOCAL_CANDIDATES, JSORB_K_LOCAL_RESOLVE, JSORB_K_ID_END };" in hdr
    lib.jsorb_kernel_name.restype = ctypes.c_char_p
    assert [lib.jsorb_kernel_name(k) for k in (orb.K_LAST_MATCH, orb.K_LAST_RESOLVE, orb.K_LAST_RESOLVE + 1)] == [b"k_last_match", b"k_last_resolve", b""]
    assert ctypes.sizeof(orb.JsorbLastFrameParams) == 120 and ctypes.sizeof(orb.JsorbSearchParams) == 40 and len(orb.KERNELS) == 8
    for m in ("search_last_frame", "search_last_frame_stats", "search_last_frame_kernel_times"):
        assert callable(getattr(orb.ORBExtractor, m))
    from jetson_slam_amd import build as jb
    assert "k_search_last.hip" in jb.SOURCES and "k_search_common.h" in jb.HEADERS
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert re.search(r"inline int SearchLastFrame\(", shim)


def test_validation_without_a_device(orb):
    """argument checks that need no GPU: a null handle"""
    lib = orb.load_library()
    prm = orb.make_last_frame_params(np.eye(3), np.zeros(3), (400, 400, 160, 120), (0, 320, 0, 240), (0.2, 0.2))
    assert lib.jsorb_search_last_frame_async(None, 0, ctypes.byref(prm), 0, *([None] * 11)) != 0
    n = ctypes.c_int()
    assert lib.jsorb_search_last_frame(None, 0, ctypes.byref(prm), 0, *([None] * 8), ctypes.byref(n)) != 0
    assert lib.jsorb_search_last_frame_stats(None, None, None, None) != 0
