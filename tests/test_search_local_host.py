"""CPU: the local map matching of jsorb_search_local_points (include/jsorb.h) - ORBmatcher::SearchByProjection(Frame&, map points, th)
(ORBmatcher.cpp:32-116) with Frame::GetFeaturesInArea (Frame.cpp:641-694).  A literal, sequential float32 transcription of the reference is the
yardstick; the numpy restatement of what the kernels compute (candidate lists from the grid CSR, the claim rule as a fixed point) must equal it on
random cases, ties, blocked keypoints, uRight on and off, th 1 / 3 / 5 and adversarial claim chains.  tests/test_gpu_search_local.py holds the
device to both."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INT_MIN = -2 ** 31


# ---- the frame: grid as Frame::AssignFeaturesToGrid / PosInGrid build it (float32, roundf) ----
def _roundf(v):
    v = np.asarray(v, np.float32).astype(np.float64)
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def build_grid(kx, ky, min_x, min_y, inv_w, inv_h, cols, rows):
    """mGrid[cols][rows] as lists, and the CSR k_assign_grid writes (cell (i, j) at i*rows + j, items ascending)"""
    px = _roundf((np.asarray(kx, np.float32) - f32(min_x)) * f32(inv_w))
    py = _roundf((np.asarray(ky, np.float32) - f32(min_y)) * f32(inv_h))
    grid = [[[] for _ in range(rows)] for _ in range(cols)]
    for k, (a, b) in enumerate(zip(px, py)):
        if 0 <= a < cols and 0 <= b < rows:
            grid[int(a)][int(b)].append(k)
    start = np.zeros(cols * rows + 1, np.int64)
    start[1:] = np.cumsum([len(grid[i][j]) for i in range(cols) for j in range(rows)])
    items = np.array([k for i in range(cols) for j in range(rows) for k in grid[i][j]], np.int64)
    return grid, start, items


def _to_int(f):
    """(int) of a float as x86 truncates it (out of range / NaN -> INT_MIN): the reference's cast, undefined only outside the contract"""
    f = float(f)
    return int(f) if -2147483648.0 < f < 2147483648.0 else INT_MIN


def popcount_dist(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


# ---- the yardstick: a literal transcription of the reference, sequential, float32 ----
def get_features_in_area(F, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cpp:641-694)"""
    x, y, r = f32(x), f32(y), f32(r)
    idx = []
    nMinCellX = max(0, _to_int(np.floor((x - F["min_x"] - r) * F["inv_w"])))
    if nMinCellX >= F["cols"]:
        return idx
    nMaxCellX = min(F["cols"] - 1, _to_int(np.ceil((x - F["min_x"] + r) * F["inv_w"])))
    if nMaxCellX < 0:
        return idx
    nMinCellY = max(0, _to_int(np.floor((y - F["min_y"] - r) * F["inv_h"])))
    if nMinCellY >= F["rows"]:
        return idx
    nMaxCellY = min(F["rows"] - 1, _to_int(np.ceil((y - F["min_y"] + r) * F["inv_h"])))
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
                distx = F["kx"][k] - x
                disty = F["ky"][k] - y
                if abs(distx) < r and abs(disty) < r:
                    idx.append(k)
    return idx


def search_by_projection(F, P, th, nn_ratio=0.8, th_high=100):
    """ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th) (ORBmatcher.cpp:32-116), the claim as
    F.mvpMapPoints[bestIdx] = i; blocked keypoints are F.mvpMapPoints[k] with Observations() > 0 before the call."""
    N = len(F["kx"])
    owner = np.where(np.asarray(F["blocked"]) != 0, -2, -1) if F["blocked"] is not None else np.full(N, -1)   # -2: an earlier frame's point
    match = np.full(len(P["u"]), -1, np.int64)
    mdist = np.full(len(P["u"]), -1, np.int64)
    th = f32(th)
    bFactor = th != 1.0
    nmatches = 0
    for i in range(len(P["u"])):
        if not P["in_frustum"][i]:
            continue
        L = int(P["level"][i])
        if L < 0 or L >= len(F["scale"]):        # outside the contract (the reference would read mvScaleFactors out of bounds)
            continue
        r = f32(2.5) if float(P["view_cos"][i]) > 0.998 else f32(4.0)        # RadiusByViewingCos: float against the double 0.998
        if bFactor:
            r = f32(r * th)
        R = f32(r * F["scale"][L])
        vIndices = get_features_in_area(F, P["u"][i], P["v"][i], R, L - 1, L)
        if not vIndices:
            continue
        bestDist, bestLevel, bestDist2, bestLevel2, bestIdx = 256, -1, 256, -1, -1
        xr = f32(f32(P["u"][i]) - f32(f32(F["mbf"]) * f32(P["invz"][i])))      # mTrackProjXR (Tracking.cpp:1617)
        for idx in vIndices:
            if owner[idx] != -1:
                continue
            if F["u_right"] is not None and F["u_right"][idx] > 0:
                er = abs(f32(xr - F["u_right"][idx]))
                if er > R:
                    continue
            dist = popcount_dist(P["desc"][i], F["desc"][idx])
            if dist < bestDist:
                bestDist2, bestDist = bestDist, dist
                bestLevel2, bestLevel = bestLevel, int(F["octave"][idx])
                bestIdx = idx
            elif dist < bestDist2:
                bestLevel2 = int(F["octave"][idx])
                bestDist2 = dist
        if bestDist <= th_high and bestIdx >= 0:
            if bestLevel == bestLevel2 and f32(bestDist) > f32(f32(nn_ratio) * f32(bestDist2)):
                continue
            owner[bestIdx] = i
            match[i], mdist[i] = bestIdx, bestDist
            nmatches += 1
    kp_match = np.where(owner >= 0, owner, -1)
    return match, mdist, kp_match, nmatches


# ---- the restatement of the kernels: candidate lists over the CSR, then the claim rule as a fixed point ----
def candidate_lists(F, P, th):
    """k_local_candidates: per point the (keypoint, octave, distance) survivors of the level / window / blocked_in / uRight filters in the
    reference's order (cells of one ix are one contiguous CSR range)"""
    n, N = len(P["u"]), len(F["kx"])
    start, items = F["start"], F["items"]
    rows, cols = F["rows"], F["cols"]
    kx, ky, octv = np.asarray(F["kx"], np.float32), np.asarray(F["ky"], np.float32), np.asarray(F["octave"], np.int64)
    blocked = np.asarray(F["blocked"]) != 0 if F["blocked"] is not None else np.zeros(N, bool)
    bits = np.unpackbits(np.asarray(F["desc"], np.uint8), axis=1) if N else np.zeros((0, 256), np.uint8)
    out = []
    for i in range(n):
        L = int(P["level"][i])
        if not P["in_frustum"][i] or L < 0 or L >= len(F["scale"]):
            out.append(np.zeros((0, 3), np.int64))
            continue
        r = f32(2.5) if f32(P["view_cos"][i]) >= f32(0.998) else f32(4.0)
        if f32(th) != f32(1.0):
            r = f32(r * f32(th))
        R = f32(r * F["scale"][L])
        x, y = f32(P["u"][i]), f32(P["v"][i])
        xr = f32(x - f32(f32(F["mbf"]) * f32(P["invz"][i])))
        x0 = max(0, _to_int(np.floor(f32(f32(x - F["min_x"]) - R) * F["inv_w"])))
        x1 = min(cols - 1, _to_int(np.ceil(f32(f32(x - F["min_x"]) + R) * F["inv_w"])))
        y0 = max(0, _to_int(np.floor(f32(f32(y - F["min_y"]) - R) * F["inv_h"])))
        y1 = min(rows - 1, _to_int(np.ceil(f32(f32(y - F["min_y"]) + R) * F["inv_h"])))
        if x0 >= cols or x1 < 0 or y0 >= rows or y1 < 0:
            out.append(np.zeros((0, 3), np.int64))
            continue
        ks = np.concatenate([items[start[ix * rows + y0]:start[ix * rows + y1 + 1]] for ix in range(x0, x1 + 1)]).astype(np.int64)
        ok = (octv[ks] >= L - 1) & (octv[ks] <= L) & (np.abs(kx[ks] - x) < R) & (np.abs(ky[ks] - y) < R) & ~blocked[ks]
        if F["u_right"] is not None:
            ur = np.asarray(F["u_right"], np.float32)[ks]
            with np.errstate(invalid="ignore"):
                ok &= ~((ur > 0) & (np.abs(xr - ur) > R))
        ks = ks[ok]
        pb = np.unpackbits(np.asarray(P["desc"][i], np.uint8))
        d = (bits[ks] != pb).sum(1).astype(np.int64)
        out.append(np.stack([ks, octv[ks], d], 1))
    return out


def resolve_fixed_point(cands, N, nn_ratio=0.8, th_high=100):
    """k_local_resolve: every round each point takes its top two over the candidates no earlier point claimed in the previous round, then
    claim[k] = min i whose choice is k; until nothing changes.  Returns match, dist, kp_match, nmatches, rounds."""
    n = len(cands)
    INF = np.iinfo(np.int64).max
    claim = np.full(N, INF, np.int64)
    match = np.full(n, -2, np.int64)
    mdist = np.full(n, -1, np.int64)
    rounds = 0
    while True:
        rounds += 1
        changed = False
        for i, c in enumerate(cands):
            m, d = -1, -1
            if len(c):
                c = c[claim[c[:, 0]] >= i]
                keep = c[c[:, 2] < 256]
                if len(keep):
                    b = int(np.argmin(keep[:, 2]))                 # first position of the minimum: the strict-< update order
                    rest = np.delete(keep, b, 0)
                    bd, bl, bk = int(keep[b, 2]), int(keep[b, 1]), int(keep[b, 0])
                    if len(rest):
                        s = int(np.argmin(rest[:, 2]))
                        bd2, bl2 = int(rest[s, 2]), int(rest[s, 1])
                    else:
                        bd2, bl2 = 256, -1
                    if bd <= th_high and not (bl == bl2 and f32(bd) > f32(f32(nn_ratio) * f32(bd2))):
                        m, d = bk, bd
            if m != match[i]:
                changed = True
                match[i] = m
            mdist[i] = d
        if not changed or rounds > n:
            break
        claim[:] = INF
        for i in range(n - 1, -1, -1):
            if match[i] >= 0:
                claim[match[i]] = i
    kp_match = np.where(claim == INF, -1, claim)
    return match, mdist, kp_match, int((match >= 0).sum()), rounds


def search_local_restated(F, P, th, nn_ratio=0.8, th_high=100):
    return resolve_fixed_point(candidate_lists(F, P, th), len(F["kx"]), nn_ratio, th_high)


# ---- random cases ----
def random_case(rng, th, stereo, chain=False):
    W, H = 320, 240
    n_levels = int(rng.integers(1, 9))
    scale = np.ones(n_levels, np.float32)
    for l in range(1, n_levels):
        scale[l] = f32(scale[l - 1] * f32(1.2))
    N = int(rng.integers(0, 160))
    integer = rng.random() < 0.5                       # keypoint coordinates (no camera) or undistorted floats
    kx = rng.integers(0, W, N).astype(np.float32) if integer else rng.uniform(-10, W + 10, N).astype(np.float32)
    ky = rng.integers(0, H, N).astype(np.float32) if integer else rng.uniform(-10, H + 10, N).astype(np.float32)
    octave = rng.integers(0, n_levels, N)
    pool = rng.integers(0, 256, (6, 32), dtype=np.uint8)     # few distinct descriptors: exact ties
    desc = pool[rng.integers(0, 6, N)].copy() if N else np.zeros((0, 32), np.uint8)
    flip = rng.random(N) < 0.5
    desc[flip] ^= (rng.random((int(flip.sum()), 32)) < 0.05).astype(np.uint8) * rng.integers(1, 256, (int(flip.sum()), 32), dtype=np.uint8)
    cols, rows = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    min_x, min_y = f32(rng.uniform(-5, 5)), f32(rng.uniform(-5, 5))
    inv_w, inv_h = f32(cols) / f32(W + 3 - min_x), f32(rows) / f32(H + 2 - min_y)
    grid, start, items = build_grid(kx, ky, min_x, min_y, inv_w, inv_h, cols, rows)
    mbf = f32(rng.uniform(20, 60))
    u_right = None
    if stereo and N:
        u_right = (kx - rng.uniform(-2, 30, N)).astype(np.float32)
        u_right[rng.random(N) < 0.3] = f32(-1)
    blocked = (rng.random(N) < 0.1).astype(np.uint8) if rng.random() < 0.7 else None
    F = dict(kx=kx, ky=ky, octave=octave, desc=desc, grid=grid, start=start, items=items, cols=cols, rows=rows, min_x=min_x, min_y=min_y,
             inv_w=inv_w, inv_h=inv_h, scale=scale, mbf=mbf, u_right=u_right, blocked=blocked)
    n = int(rng.integers(0, 60))
    src = rng.integers(0, max(N, 1), n)
    u = (kx[src] + rng.normal(0, 3, n)).astype(np.float32) if N else rng.uniform(0, W, n).astype(np.float32)
    v = (ky[src] + rng.normal(0, 3, n)).astype(np.float32) if N else rng.uniform(0, H, n).astype(np.float32)
    level = (octave[src] + rng.integers(0, 2, n)).astype(np.int32) if N else rng.integers(0, n_levels, n).astype(np.int32)
    level[rng.random(n) < 0.05] = rng.choice([-1, n_levels, 99])        # outside the contract: no match
    view_cos = rng.choice(np.array([0.5, 0.998, 0.99799996, 0.9980001, 1.0], np.float32), n)
    invz = rng.uniform(0.05, 1.0, n).astype(np.float32)
    if stereo and N:                                                     # so that the uRight gate passes and fails
        invz = ((u - u_right[src]) / mbf + rng.normal(0, 0.05, n)).astype(np.float32)
    pdesc = desc[src].copy() if N else rng.integers(0, 256, (n, 32), dtype=np.uint8)
    noise = rng.random((n, 32)) < 0.08
    pdesc[noise] ^= rng.integers(1, 256, int(noise.sum()), dtype=np.uint8)
    far = rng.random(n) < 0.05
    pdesc[far] = ~pdesc[far]                                             # complements: distance 256 to their source
    P = dict(u=u, v=v, invz=invz, level=level, view_cos=view_cos, in_frustum=(rng.random(n) < 0.9).astype(np.uint8), desc=pdesc)
    if chain and N:
        # every point at the same spot with the same descriptor: point i takes the i-th keypoint of a shared preference order
        j = int(rng.integers(0, N))
        P["u"][:] = kx[j]
        P["v"][:] = ky[j]
        P["level"][:] = octave[j]
        P["desc"][:] = desc[j]
        P["in_frustum"][:] = 1
    return F, P


@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
@pytest.mark.parametrize("stereo", [False, True])
def test_fixed_point_equals_the_sequential_reference(th, stereo):
    rng = np.random.default_rng(int(th * 10) + stereo)
    n_matched = n_rounds_gt1 = 0
    for case in range(350):
        F, P = random_case(rng, th, stereo, chain=case % 7 == 0)
        nn, thh = (1.0, 255) if case % 7 == 0 else (0.8, 100)
        m, d, km, cnt = search_by_projection(F, P, th, nn, thh)
        m2, d2, km2, cnt2, rounds = search_local_restated(F, P, th, nn, thh)
        assert np.array_equal(m, m2) and np.array_equal(d, d2) and np.array_equal(km, km2) and cnt == cnt2, case
        assert rounds <= len(P["u"]) + 1
        n_matched += cnt
        n_rounds_gt1 += rounds > 2
    assert n_matched > 500 and n_rounds_gt1 > 20          # not vacuous: matches and conflicts that take several rounds


def test_claim_chain_takes_one_round_per_link():
    """point i+1's best is point i's: each round settles one more point; 12 points -> 13 rounds"""
    N, n = 12, 12
    base = np.zeros(32, np.uint8)
    desc = np.zeros((N, 32), np.uint8)
    for m in range(N):                                   # distance 10 + 10 m to the shared descriptor
        bits = np.zeros(256, np.uint8)
        bits[:10 + 10 * m] = 1
        desc[m] = np.packbits(bits)
    kx = np.full(N, 100.0, np.float32) + np.arange(N, dtype=np.float32) * 0.1
    ky = np.full(N, 50.0, np.float32)
    octave = np.arange(N) % 2                            # alternating levels: no ratio test between neighbours
    grid, start, items = build_grid(kx, ky, 0, 0, f32(64) / f32(320), f32(48) / f32(240), 64, 48)
    F = dict(kx=kx, ky=ky, octave=octave, desc=desc, grid=grid, start=start, items=items, cols=64, rows=48, min_x=f32(0), min_y=f32(0),
             inv_w=f32(64) / f32(320), inv_h=f32(48) / f32(240), scale=np.array([1, 1.2], np.float32), mbf=f32(40), u_right=None, blocked=None)
    P = dict(u=np.full(n, 100.5, np.float32), v=np.full(n, 50, np.float32), invz=np.full(n, 0.5, np.float32), level=np.ones(n, np.int32),
             view_cos=np.full(n, 0.5, np.float32), in_frustum=np.ones(n, np.uint8), desc=np.tile(base, (n, 1)))
    m, d, km, cnt = search_by_projection(F, P, 1.0, 0.8, 255)
    m2, d2, km2, cnt2, rounds = search_local_restated(F, P, 1.0, 0.8, 255)
    assert list(m) == list(range(N)) and list(d) == [10 + 10 * i for i in range(N)]
    assert np.array_equal(m, m2) and np.array_equal(d, d2) and np.array_equal(km, km2) and cnt == cnt2 == N
    assert rounds == n + 1


def test_view_cos_threshold_is_the_double_comparison():
    """RadiusByViewingCos: viewCos > 0.998 with a double literal - 0.998f itself (0.99800002...) is above it; the float just below is not"""
    assert float(f32(0.998)) > 0.998 and not float(np.nextafter(f32(0.998), f32(0))) > 0.998


def test_header_and_binding_declare_the_new_entry_points(orb):
    names = ("jsorb_search_local_points_async", "jsorb_search_local_points", "jsorb_search_local_stats")
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    for n in names:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
    src = open(orb.__file__).read()
    for n in names:
        assert '"%s": (' % n in src                     # in the binding's prototype table
    assert "enum { JSORB_K_ASSIGN_GRID = JSORB_K_COUNT_ALL + 1, JSORB_K_LOCAL_CANDIDATES, JSORB_K_LOCAL_RESOLVE, JSORB_K_ID_END };" in hdr
    lib.jsorb_kernel_name.restype = ctypes.c_char_p
    assert [lib.jsorb_kernel_name(k) for k in (orb.K_ASSIGN_GRID, orb.K_LOCAL_CANDIDATES, orb.K_LOCAL_RESOLVE)] == \
        [b"k_assign_grid", b"k_local_candidates", b"k_local_resolve"]
    assert ctypes.sizeof(orb.JsorbSearchParams) == 40
    for m in ("search_local_points", "search_local_stats", "search_local_kernel_times"):
        assert callable(getattr(orb.ORBExtractor, m))
    from jetson_slam_amd import build as jb
    assert "k_search_local.hip" in jb.SOURCES and "-ffp-contract=off" in jb.FLAGS


def test_validation_without_a_device(orb):
    """argument checks that need no GPU: a null handle"""
    lib = orb.load_library()
    prm = orb.JsorbSearchParams(1.0, 0.8, 100, 40.0, 0, 0, 0.2, 0.2, 64, 48)
    assert lib.jsorb_search_local_points_async(None, 0, ctypes.byref(prm), 0, *([None] * 13)) != 0
    n = ctypes.c_int()
    assert lib.jsorb_search_local_points(None, 0, ctypes.byref(prm), 0, *([None] * 10), ctypes.byref(n)) != 0
    assert lib.jsorb_search_local_stats(None, None, None, None) != 0
