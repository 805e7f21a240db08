"""CPU: the monocular initialisation matcher of jsorb_search_for_initialization (include/jsorb.h) - ORBmatcher::SearchForInitialization
(ORBmatcher.cpp:392-507) with Frame::GetFeaturesInArea (Frame.cpp:641-694) and ComputeThreeMaxima (ORBmatcher.cpp:2097-2138).  A literal,
sequential float32 transcription is the yardstick and records a trace (displaced claims, candidates hidden by vMatchedDistance, culled entries,
choices and ratio tests that the hiding changed).  The numpy restatement of what the kernels compute (candidate lists from the grid CSR with a
capacity and a rescan, the claim rule as a fixed point over index-ordered chunks, the last owner per keypoint, the histogram over all claims, the
culled set) must equal it on random cases and on constructed dependency chains.  tests/test_gpu_search_init.py holds the device to both."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_search_last_frame_host import HISTO_LENGTH, compute_three_maxima, rot_bin
from test_search_local_host import _to_int, build_grid, get_features_in_area, popcount_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INT_MAX = 2 ** 31 - 1
SI_CAP, SI_CHUNK = 192, 64                     # k_search_init.hip: candidates kept per point, points per chunk of the resolver


def default_params(**kw):
    """ORBmatcher matcher(0.9, true), windowSize 50 (Tracking.cpp:724-794), TH_LOW = 50"""
    p = dict(window=f32(50), nn_ratio=f32(0.9), th_low=50, check_orientation=1)
    p.update(kw)
    return p


# ---- the yardstick: a literal transcription, sequential, float32 ----
def search_for_initialization(F1, F2, prev_matched, prm):
    """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize): (vnMatches12, vnMatches21, nmatches, vbPrevMatched
    as float32[2, n1], trace).  F1: octave, angle, desc; F2: the frame dict of test_search_local_host (kx, ky = mvKeysUn) with angle."""
    n1, N = len(F1["octave"]), len(F2["kx"])
    prev = np.array(prev_matched, np.float32).reshape(2, n1).copy()
    window, ratio = f32(prm["window"]), f32(prm["nn_ratio"])
    nmatches = 0
    vnMatches12 = np.full(n1, -1, np.int64)
    rotHist = [[] for _ in range(HISTO_LENGTH + 1)]
    vMatchedDistance = np.full(N, INT_MAX, np.int64)
    vnMatches21 = np.full(N, -1, np.int64)
    tr = dict(candidates=0, displaced=0, hidden=0, choice_changed=0, ratio_flip=0, culled=0, displaced_kept=0, displaced_culled=0, claims=0,
              ind=(-1, -1, -1))
    displaced_points = []
    for i1 in range(n1):
        level1 = int(F1["octave"][i1])
        if level1 > 0:
            continue
        vIndices2 = get_features_in_area(F2, prev[0, i1], prev[1, i1], window, level1, level1)
        if not vIndices2:
            continue
        tr["candidates"] += len(vIndices2)
        bestDist, bestDist2, bestIdx2 = INT_MAX, INT_MAX, -1
        freeDist, freeDist2, freeIdx = INT_MAX, INT_MAX, -1          # trace only: the same without vMatchedDistance
        hidden = 0
        for i2 in vIndices2:
            dist = popcount_dist(F1["desc"][i1], F2["desc"][i2])
            if dist < freeDist:
                freeDist2, freeDist, freeIdx = freeDist, dist, i2
            elif dist < freeDist2:
                freeDist2 = dist
            if vMatchedDistance[i2] <= dist:
                hidden += 1
                continue
            if dist < bestDist:
                bestDist2 = bestDist
                bestDist = dist
                bestIdx2 = i2
            elif dist < bestDist2:
                bestDist2 = dist
        tr["hidden"] += hidden
        claim = bestDist <= prm["th_low"] and f32(bestDist) < f32(f32(bestDist2) * ratio)
        free_claim = freeDist <= prm["th_low"] and f32(freeDist) < f32(f32(freeDist2) * ratio)
        tr["choice_changed"] += bool(claim and free_claim and freeIdx != bestIdx2)
        tr["ratio_flip"] += bool(claim != free_claim and freeDist <= prm["th_low"] and bestDist <= prm["th_low"])
        if bestDist <= prm["th_low"]:
            if f32(bestDist) < f32(f32(bestDist2) * ratio):
                if vnMatches21[bestIdx2] >= 0:
                    vnMatches12[vnMatches21[bestIdx2]] = -1
                    nmatches -= 1
                    tr["displaced"] += 1
                    displaced_points.append(int(vnMatches21[bestIdx2]))
                vnMatches12[i1] = bestIdx2
                vnMatches21[bestIdx2] = i1
                vMatchedDistance[bestIdx2] = bestDist
                nmatches += 1
                tr["claims"] += 1
                if prm["check_orientation"]:
                    rotHist[rot_bin(F1["angle"][i1], F2["angle"][bestIdx2])].append(i1)
    if prm["check_orientation"]:
        ind = compute_three_maxima([len(h) for h in rotHist])
        tr["ind"] = tuple(ind)
        for i in range(HISTO_LENGTH + 1):
            if i in ind:
                tr["displaced_kept"] += len(set(rotHist[i]) & set(displaced_points))
                continue
            tr["displaced_culled"] += len(set(rotHist[i]) & set(displaced_points))
            for idx1 in rotHist[i]:
                if vnMatches12[idx1] >= 0:
                    vnMatches12[idx1] = -1
                    nmatches -= 1
                    tr["culled"] += 1
    for i1 in range(n1):
        if vnMatches12[i1] >= 0:
            prev[0, i1] = F2["kx"][vnMatches12[i1]]
            prev[1, i1] = F2["ky"][vnMatches12[i1]]
    return vnMatches12, vnMatches21, nmatches, prev, tr


# ---- the restatement of the kernels ----
def window_candidates(F1, F2, prev, prm, i):
    """k_init_candidates for point i: (keypoints, distances) in walk order over the CSR, all of them"""
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    oct1 = int(F1["octave"][i])
    if oct1 > 0:
        return none
    start, items, rows, cols = F2["start"], F2["items"], F2["rows"], F2["cols"]
    x, y, R = f32(prev[0, i]), f32(prev[1, i]), f32(prm["window"])
    x0 = max(0, _to_int(np.floor(f32(f32(x - F2["min_x"]) - R) * F2["inv_w"])))
    if x0 >= cols:
        return none
    x1 = min(cols - 1, _to_int(np.ceil(f32(f32(x - F2["min_x"]) + R) * F2["inv_w"])))
    if x1 < 0:
        return none
    y0 = max(0, _to_int(np.floor(f32(f32(y - F2["min_y"]) - R) * F2["inv_h"])))
    if y0 >= rows:
        return none
    y1 = min(rows - 1, _to_int(np.ceil(f32(f32(y - F2["min_y"]) + R) * F2["inv_h"])))
    if y1 < 0:
        return none
    js = np.concatenate([np.arange(start[ix * rows + y0], start[ix * rows + y1 + 1]) for ix in range(x0, x1 + 1)]).astype(np.int64)
    ks = np.asarray(items, np.int64)[js]
    kx, ky = np.asarray(F2["kx"], np.float32), np.asarray(F2["ky"], np.float32)
    ok = (np.abs(kx[ks] - x) < R) & (np.abs(ky[ks] - y) < R)
    if oct1 >= 0:                                        # a negative octave switches the level check off
        ok &= np.asarray(F2["octave"], np.int64)[ks] == 0
    ks = ks[ok]
    d = (F2["bits"][ks] != np.unpackbits(np.asarray(F1["desc"][i], np.uint8))).sum(1).astype(np.int64)
    return ks, d


def search_init_restated(F1, F2, prev_matched, prm, cap=SI_CAP, chunk=SI_CHUNK):
    """k_init_candidates + k_init_resolve: (matches12, matches21, nmatches, prev_matched, stats, points with candidates) with stats = (rounds,
    candidates, overflowed points, displaced claims, (ind1, ind2, ind3))"""
    n1, N = len(F1["octave"]), len(F2["kx"])
    prev = np.array(prev_matched, np.float32).reshape(2, n1).copy()
    F2 = dict(F2, bits=np.unpackbits(np.asarray(F2["desc"], np.uint8), axis=1) if N else np.zeros((0, 256), np.uint8))
    ratio = f32(prm["nn_ratio"])
    full = [window_candidates(F1, F2, prev, prm, i) for i in range(n1)]
    cand_n = np.array([len(c[0]) for c in full], np.int64)
    lists = [(c[0][:cap], c[1][:cap]) for c in full]    # what k_init_candidates stores
    order = [i for i in range(n1) if cand_n[i] > 0]
    md = np.full(N, 511, np.int64)                      # finished chunks: vMatchedDistance (511: INT_MAX)
    owner = np.full(N, -1, np.int64)
    claim = np.full(n1, -1, np.int64)
    rounds = 0
    for base in range(0, len(order), chunk):
        pts = order[base:base + chunk]
        cands = [lists[i] if cand_n[i] <= cap else window_candidates(F1, F2, prev, prm, i) for i in pts]      # overflow: the rescan
        sk, sd = [-1] * len(pts), [0] * len(pts)
        prev_k = [-2] * len(pts)
        for r in range(chunk + 1):
            rounds += 1
            nk, nd = [], []
            for p in range(len(pts)):
                ks, ds = cands[p]
                m = md[ks].copy()
                for l in range(p):                       # the lower points of the chunk, as they chose in the previous round
                    if sk[l] >= 0:
                        sel = ks == sk[l]
                        m[sel] = np.minimum(m[sel], sd[l])
                vis = m > ds
                k, d = -1, 0
                if vis.any():
                    dv, kv = ds[vis], ks[vis]
                    t = int(np.argmin(dv))               # the first in walk order with the minimum
                    d1 = int(dv[t])
                    rest = np.delete(dv, t)
                    d2 = int(rest.min()) if len(rest) else INT_MAX
                    if d1 <= prm["th_low"] and f32(d1) < f32(f32(d2) * ratio):
                        k, d = int(kv[t]), d1
                nk.append(k)
                nd.append(d)
            if nk == prev_k:
                break
            sk, sd, prev_k = nk, nd, nk
        for p, i in enumerate(pts):
            if sk[p] >= 0:
                md[sk[p]] = min(md[sk[p]], sd[p])
                owner[sk[p]] = max(owner[sk[p]], i)
                claim[i] = sk[p]
    claimed = claim >= 0
    owned = np.array([claimed[i] and owner[claim[i]] == i for i in range(n1)], bool)      # a claim stands while its point is the last claimant
    matches12 = np.where(owned, claim, -1)
    ind = (-1, -1, -1)
    culled = 0
    if prm["check_orientation"]:
        pbin = np.array([rot_bin(F1["angle"][i], F2["angle"][claim[i]]) if claimed[i] else -1 for i in range(n1)], np.int64)
        ind = compute_three_maxima(np.bincount(pbin[claimed], minlength=HISTO_LENGTH + 1))
        cut = owned & ~np.isin(pbin, [b for b in ind if b >= 0])
        matches12[cut] = -1
        culled = int(cut.sum())
    for i in np.nonzero(matches12 >= 0)[0]:
        prev[0, i] = F2["kx"][matches12[i]]
        prev[1, i] = F2["ky"][matches12[i]]
    stats = (rounds, int(cand_n.sum()), int((cand_n > cap).sum()), int(claimed.sum() - owned.sum()), tuple(int(b) for b in ind))
    return matches12, owner, int(owned.sum()) - culled, prev, stats, len(order)


def agree(ref, res):
    """matches12, matches21, count, prev_matched (bit for bit) and the statistics both sides have"""
    m12, m21, cnt, prev, tr = ref
    s12, s21, scnt, sprev, st = res[:5]
    assert np.array_equal(m12, s12) and np.array_equal(m21, s21) and cnt == scnt
    assert np.array_equal(prev.view(np.uint32), sprev.view(np.uint32))
    assert (tr["candidates"], tr["displaced"], tr["ind"]) == (st[1], st[3], st[4])
    return st


# ---- random cases ----
def random_case(rng, big=False):
    W, H = 320, 240
    N = int(rng.integers(0, 140)) if rng.random() < 0.97 else 0
    kx = rng.uniform(-5, W + 5, N).astype(np.float32)
    ky = rng.uniform(-5, H + 5, N).astype(np.float32)
    if rng.random() < 0.5:
        kx, ky = np.round(kx).astype(np.float32), np.round(ky).astype(np.float32)
    if N and rng.random() < 0.5:                          # clusters: many keypoints in one window
        c = rng.integers(0, N, N)
        kx = (kx[c] + rng.normal(0, 6, N)).astype(np.float32)
        ky = (ky[c] + rng.normal(0, 6, N)).astype(np.float32)
    octave = rng.integers(0, 4, N)
    octave[rng.random(N) < 0.7] = 0
    angle = rng.choice(np.array([0, 10, 90, 180, 359.5], np.float32), N) if rng.random() < 0.5 else rng.uniform(0, 360, N).astype(np.float32)
    n_pool = int(rng.choice([2, 5, 20, 60]))
    pool = rng.integers(0, 256, (n_pool, 32), dtype=np.uint8)
    desc = pool[rng.integers(0, n_pool, N)].copy() if N else np.zeros((0, 32), np.uint8)
    flip = rng.random((N, 32)) < 0.03
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    cols, rows = int(rng.integers(1, 70)), int(rng.integers(1, 50))
    min_x, max_x, min_y, max_y = f32(rng.uniform(-5, 2)), f32(W + rng.uniform(-3, 5)), f32(rng.uniform(-5, 2)), f32(H + rng.uniform(-3, 5))
    inv_w, inv_h = f32(cols) / f32(max_x - min_x), f32(rows) / f32(max_y - min_y)
    grid, start, items = build_grid(kx, ky, min_x, min_y, inv_w, inv_h, cols, rows)
    F2 = dict(kx=kx, ky=ky, octave=octave, angle=angle, desc=desc, grid=grid, start=start, items=items, cols=cols, rows=rows, min_x=min_x,
              min_y=min_y, inv_w=inv_w, inv_h=inv_h)
    n1 = int(rng.integers(0, 260 if big else 90)) if rng.random() < 0.97 else 0
    few = rng.integers(0, max(N, 1), max(1, int(rng.integers(1, 12))))
    src = rng.choice(few, n1) if rng.random() < 0.4 else rng.integers(0, max(N, 1), n1)      # duplicate targets
    px = (kx[src] if N else rng.uniform(0, W, n1)) + rng.normal(0, rng.choice([0.5, 4.0, 30.0]), n1)
    py = (ky[src] if N else rng.uniform(0, H, n1)) + rng.normal(0, rng.choice([0.5, 4.0, 30.0]), n1)
    far = rng.random(n1) < 0.05                           # windows that are empty or off the grid
    px[far] += rng.choice([-900.0, 900.0, 1e9], int(far.sum()))
    prev = np.stack([px, py]).astype(np.float32)
    oct1 = np.zeros(n1, np.int32)
    hi = rng.random(n1) < rng.choice([0.0, 0.2, 0.6])
    oct1[hi] = rng.integers(1, 5, int(hi.sum()))
    oct1[rng.random(n1) < 0.02] = rng.choice([-1, -(2 ** 31)])
    base = angle[src] if N else rng.uniform(0, 360, n1).astype(np.float32)
    offs = np.where(rng.random(n1) < 0.35, rng.uniform(0, 360, n1), f32(12.0)).astype(np.float32)
    angle1 = np.mod(base + offs, f32(360)).astype(np.float32)
    desc1 = desc[src].copy() if N else rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    noise = rng.random((n1, 32)) < rng.choice([0.01, 0.05, 0.12], n1)[:, None]
    desc1[noise] ^= rng.integers(1, 256, int(noise.sum()), dtype=np.uint8)
    away = rng.random(n1) < 0.04
    desc1[away] = ~desc1[away]
    F1 = dict(octave=oct1, angle=angle1, desc=desc1)
    prm = default_params(window=f32(rng.choice([50, 50, 12, 3, 400])), check_orientation=int(rng.random() < 0.8),
                         nn_ratio=f32(rng.choice([0.9, 0.9, 0.6])), th_low=int(rng.choice([50, 50, 30, 100])))
    if rng.random() < 0.1:
        oct1[:] = rng.integers(1, 4)                      # an all-octave>0 F1
    return F1, F2, prev, prm


@pytest.mark.parametrize("part", range(4))
def test_kernels_formulation_equals_the_sequential_reference(part):
    rng = np.random.default_rng(300 + part)
    seen = dict(matches=0, displaced=0, hidden=0, choice_changed=0, ratio_flip=0, culled=0, displaced_kept=0, displaced_culled=0, overflow=0,
                chunks=0, deep=0, empty=0, n1_zero=0, N_zero=0, all_high=0, negative=0)
    for case in range(520):
        F1, F2, prev, prm = random_case(rng, big=case % 8 == 0)
        cap, chunk = [(SI_CAP, SI_CHUNK), (2, SI_CHUNK), (SI_CAP, 4), (3, 7)][case % 4]
        ref = search_for_initialization(F1, F2, prev, prm)
        res = search_init_restated(F1, F2, prev, prm, cap, chunk)
        st = agree(ref, res)
        tr = ref[4]
        n_chunks = (res[5] + chunk - 1) // chunk
        seen["matches"] += ref[2]
        for k in ("displaced", "hidden", "choice_changed", "ratio_flip", "culled", "displaced_kept", "displaced_culled"):
            seen[k] += tr[k]
        seen["overflow"] += st[2]
        seen["chunks"] += n_chunks > 1
        seen["deep"] += st[0] > 2 * n_chunks              # some chunk needed a third round
        seen["empty"] += tr["candidates"] == 0 and len(F1["octave"]) > 0 and len(F2["kx"]) > 0
        seen["n1_zero"] += len(F1["octave"]) == 0
        seen["N_zero"] += len(F2["kx"]) == 0
        seen["all_high"] += len(F1["octave"]) > 0 and (F1["octave"] > 0).all()
        seen["negative"] += int((F1["octave"] < 0).sum())
        if len(F1["octave"]) == 0 or len(F2["kx"]) == 0:
            assert ref[2] == 0 and np.array_equal(ref[3].view(np.uint32), prev.view(np.uint32))
    # the set cannot silently go soft: every event of the claim rule occurs
    assert seen["matches"] > 2000 and seen["displaced"] > 100 and seen["hidden"] > 300 and seen["culled"] > 100, seen
    assert seen["choice_changed"] > 5 and seen["ratio_flip"] > 5 and seen["displaced_kept"] > 20 and seen["displaced_culled"] > 5, seen
    assert seen["overflow"] > 100 and seen["chunks"] > 50 and seen["deep"] > 20, seen
    assert min(seen["empty"], seen["n1_zero"], seen["N_zero"], seen["all_high"], seen["negative"]) > 0, seen


# ---- constructed chains: the dependency the random cases rarely stress ----
def _bits(d):
    """a descriptor with exactly d bits set: its distance to the zero descriptor is d"""
    b = np.zeros(256, np.uint8)
    b[:d] = 1
    return np.packbits(b)


def line_frame(n_kp, spacing=20.0, width=None):
    """F2: n_kp keypoints on a line (x = spacing * j + 10, y = 50), octave 0, the zero descriptor, angle 0"""
    kx = (np.arange(n_kp) * spacing + 10).astype(np.float32)
    ky = np.full(n_kp, 50, np.float32)
    W = f32(width if width is not None else max(spacing * (n_kp + 1), 64))
    cols, rows = 64, 4
    inv_w, inv_h = f32(cols) / W, f32(rows) / f32(100)
    grid, start, items = build_grid(kx, ky, f32(0), f32(0), inv_w, inv_h, cols, rows)
    return dict(kx=kx, ky=ky, octave=np.zeros(n_kp, np.int64), angle=np.zeros(n_kp, np.float32), desc=np.zeros((n_kp, 32), np.uint8), grid=grid,
                start=start, items=items, cols=cols, rows=rows, min_x=f32(0), min_y=f32(0), inv_w=inv_w, inv_h=inv_h)


def one_target(dists, angles=None):
    """n F1 points on one F2 keypoint with the given distances"""
    n = len(dists)
    F2 = line_frame(1)
    F1 = dict(octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32) if angles is None else np.asarray(angles, np.float32),
              desc=np.stack([_bits(d) for d in dists]))
    prev = np.stack([np.full(n, 11, np.float32), np.full(n, 49, np.float32)])
    return F1, F2, prev


@pytest.mark.parametrize("n", [5, 64, 65, 150])
def test_one_keypoint_chains(n):
    prm = default_params(th_low=256, check_orientation=0)
    # strictly decreasing distances: every point displaces the one before, the last one stands
    F1, F2, prev = one_target(list(range(n + 20, 20, -1)))
    ref = search_for_initialization(F1, F2, prev, prm)
    st = agree(ref, search_init_restated(F1, F2, prev, prm))
    assert ref[2] == 1 and ref[0][n - 1] == 0 and (ref[0][:n - 1] == -1).all() and ref[1][0] == n - 1
    assert ref[4]["displaced"] == n - 1 == st[3] and ref[4]["hidden"] == 0
    # increasing: all but the first are hidden by vMatchedDistance
    F1, F2, prev = one_target(list(range(21, n + 21)))
    ref = search_for_initialization(F1, F2, prev, prm)
    agree(ref, search_init_restated(F1, F2, prev, prm))
    assert ref[2] == 1 and ref[0][0] == 0 and ref[1][0] == 0 and ref[4]["hidden"] == n - 1 and ref[4]["displaced"] == 0
    # equal: <= hides
    F1, F2, prev = one_target([30] * n)
    ref = search_for_initialization(F1, F2, prev, prm)
    agree(ref, search_init_restated(F1, F2, prev, prm))
    assert ref[2] == 1 and ref[0][0] == 0 and ref[4]["hidden"] == n - 1


def domino(n):
    """Keypoints K_0 .. K_n on a line, all with the zero descriptor; point p sits between K_p and K_p+1 at distance 10 from both, so with both
    visible its ratio test fails (10 < 0.9 * 10 is false) and with K_p hidden it claims K_p+1 with 10 - which hides K_p+1 from point p + 1.
    Point 0 sees K_1 only.  Every point claims, and only because the one before it did: a chunk of 64 needs its 65 rounds."""
    F2 = line_frame(n + 1)
    px = (np.arange(n) * 20.0 + 20).astype(np.float32)
    px[0] = 35
    prev = np.stack([px, np.full(n, 50, np.float32)])
    F1 = dict(octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32), desc=np.stack([_bits(10)] * n))
    return F1, F2, prev, default_params(window=f32(12), check_orientation=0)


@pytest.mark.parametrize("n", [3, 64, 70, 150])
def test_domino_chain_needs_every_round(n):
    F1, F2, prev, prm = domino(n)
    ref = search_for_initialization(F1, F2, prev, prm)
    st = agree(ref, search_init_restated(F1, F2, prev, prm))
    assert ref[2] == n and np.array_equal(ref[0], np.arange(1, n + 1)) and ref[4]["ratio_flip"] == n - 1 and ref[4]["hidden"] == n - 1
    chunks = [min(SI_CHUNK, n - b) for b in range(0, n, SI_CHUNK)]
    assert st[0] == sum(c + 1 for c in chunks)          # the stated worst case: points + 1 rounds per chunk
    assert max(c + 1 for c in chunks) <= SI_CHUNK + 1
    # a smaller chunk: the chain crosses every boundary
    agree(ref, search_init_restated(F1, F2, prev, prm, chunk=5))
    # broken at its start (point 0 sees both K_0 and K_1): nobody claims
    prev2 = prev.copy()
    prev2[0, 0] = 20
    ref = search_for_initialization(F1, F2, prev2, prm)
    agree(ref, search_init_restated(F1, F2, prev2, prm))
    assert ref[2] == 0


def test_hiding_changes_the_choice():
    """two keypoints in the window: A (the zero descriptor) and B (bits 0..39 set).  Point 0 (bits 8..39) is 32 from A and 8 from B: it claims B
    with 8.  Point 1 (bits 10..39) is 30 from A and 10 from B: alone it would claim B, behind point 0 B is hidden (8 <= 10) and it claims A."""
    F2 = line_frame(2, spacing=6.0, width=64)
    F2["desc"][1] = _bits(40)
    p0, p1 = _bits(40) ^ _bits(8), _bits(40) ^ _bits(10)
    assert [popcount_dist(p, F2["desc"][k]) for p in (p0, p1) for k in (0, 1)] == [32, 8, 30, 10]
    F1 = dict(octave=np.zeros(2, np.int32), angle=np.zeros(2, np.float32), desc=np.stack([p0, p1]))
    prev = np.stack([np.full(2, 13, np.float32), np.full(2, 50, np.float32)])
    prm = default_params(check_orientation=0)
    ref = search_for_initialization(F1, F2, prev, prm)
    agree(ref, search_init_restated(F1, F2, prev, prm))
    assert list(ref[0]) == [1, 0] and ref[2] == 2 and ref[4]["choice_changed"] == 1 and ref[4]["hidden"] == 1
    alone = search_for_initialization({k: v[1:] for k, v in F1.items()}, F2, prev[:, 1:], prm)
    assert list(alone[0]) == [1]


def test_candidate_list_over_the_cap():
    """one window with more keypoints than SI_CAP: the resolver's rescan gives what the full list gives"""
    rng = np.random.default_rng(5)
    N = SI_CAP + 60
    kx = rng.uniform(20, 60, N).astype(np.float32)
    ky = rng.uniform(20, 60, N).astype(np.float32)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    inv = f32(16) / f32(80)
    grid, start, items = build_grid(kx, ky, f32(0), f32(0), inv, inv, 16, 16)
    F2 = dict(kx=kx, ky=ky, octave=np.zeros(N, np.int64), angle=rng.uniform(0, 360, N).astype(np.float32), desc=desc, grid=grid, start=start,
              items=items, cols=16, rows=16, min_x=f32(0), min_y=f32(0), inv_w=inv, inv_h=inv)
    src = rng.integers(0, N, 100)
    d1 = desc[src].copy()
    d1[:, 0] ^= rng.integers(0, 256, 100, dtype=np.uint8)
    F1 = dict(octave=np.zeros(100, np.int32), angle=F2["angle"][src].copy(), desc=d1)
    prev = np.stack([np.full(100, 40, np.float32), np.full(100, 40, np.float32)])
    prm = default_params()
    ref = search_for_initialization(F1, F2, prev, prm)
    st = agree(ref, search_init_restated(F1, F2, prev, prm))
    assert st[2] == 100 and ref[2] > 30 and ref[4]["displaced"] > 0


def test_displaced_point_in_a_kept_and_in_a_culled_bin():
    """points 0..29 claim K_0..K_29 at rotation 0 (the kept bin); point 30 (rotation 90: a culled bin) takes K_0 from point 0 and is culled; point
    31 claims K_30 at rotation 90 and point 32 (rotation 0) takes it: the displaced point 31 sits in a culled bin and no longer counts"""
    F2 = line_frame(31)
    tgt = list(range(30)) + [0, 30, 30]
    dist = [20] * 30 + [5, 20, 5]
    ang = [0] * 30 + [90, 90, 0]
    F1 = dict(octave=np.zeros(33, np.int32), angle=np.asarray(ang, np.float32), desc=np.stack([_bits(d) for d in dist]))
    prev = np.stack([F2["kx"][tgt] + f32(1), np.full(33, 50, np.float32)])
    prm = default_params(window=f32(5))
    ref = search_for_initialization(F1, F2, prev, prm)
    agree(ref, search_init_restated(F1, F2, prev, prm))
    tr = ref[4]
    assert tr["ind"] == (0, -1, -1)
    assert tr["displaced"] == 2 and tr["displaced_kept"] == 1 and tr["displaced_culled"] == 1 and tr["culled"] == 1
    assert ref[0][0] == -1 and ref[0][30] == -1 and ref[0][31] == -1 and ref[0][32] == 30 and ref[2] == 30
    assert ref[1][0] == 30                               # vnMatches21 keeps the last claimant although the culling removed its match
    assert ref[3][0, 0] == prev[0, 0] and ref[3][0, 32] == F2["kx"][30]


# ---- real frames: the inputs of tests/test_gpu_search_init.py, built from an extraction's arrays ----
def frame_from_extract(kp, desc, xu, yu, w, h, cols=64, rows=48, bounds=None):
    """F2 from a keypoint SoA (6N int32), descriptors and mvKeysUn coordinates: the grid as Frame::AssignFeaturesToGrid builds it"""
    n = len(kp) // 6
    min_x, max_x, min_y, max_y = bounds if bounds is not None else (f32(0), f32(w), f32(0), f32(h))
    inv_w, inv_h = f32(cols) / f32(f32(max_x) - f32(min_x)), f32(rows) / f32(f32(max_y) - f32(min_y))
    xu, yu = np.asarray(xu, np.float32), np.asarray(yu, np.float32)
    grid, start, items = build_grid(xu, yu, min_x, min_y, inv_w, inv_h, cols, rows)
    return dict(kx=xu, ky=yu, octave=kp[4 * n:5 * n].astype(np.int64), angle=kp[3 * n:4 * n].astype(np.int32).view(np.float32),
                desc=np.asarray(desc, np.uint8).reshape(n, 32), grid=grid, start=start, items=items, cols=cols, rows=rows, min_x=f32(min_x),
                min_y=f32(min_y), inv_w=inv_w, inv_h=inv_h)


def f1_from_frame(F):
    """a kept frame as F1, and vbPrevMatched = its mvKeysUn (Tracking.cpp:735-737)"""
    return dict(octave=F["octave"].astype(np.int32), angle=F["angle"].copy(), desc=F["desc"].copy()), np.stack([F["kx"], F["ky"]]).astype(np.float32)


def f1_drawn_from(rng, F2, n1):
    """F1 arrays drawn from F2's own keypoints with replacement, mostly from octave 0, a few descriptor bits flipped (0 .. 12 per point): duplicate
    targets make later points displace earlier ones (fewer bits flipped) or find the keypoint hidden (more)"""
    N = len(F2["kx"])
    lvl0 = np.nonzero(F2["octave"] == 0)[0]
    src = np.where(rng.random(n1) < 0.85, rng.choice(lvl0, n1), rng.integers(0, N, n1))
    desc = F2["desc"][src].copy()
    bits = np.unpackbits(desc, axis=1)
    for i, nb in enumerate(rng.integers(0, 13, n1)):
        bits[i, rng.choice(256, int(nb), replace=False)] ^= 1
    desc = np.packbits(bits, axis=1)
    octave = F2["octave"][src].astype(np.int32)
    octave[rng.random(n1) < 0.03] = -1
    angle = np.mod(F2["angle"][src] + np.where(rng.random(n1) < 0.3, rng.uniform(0, 360, n1), f32(12.0)).astype(np.float32), f32(360)).astype(np.float32)
    prev = np.stack([F2["kx"][src] + rng.normal(0, 2.0, n1), F2["ky"][src] + rng.normal(0, 2.0, n1)]).astype(np.float32)
    return dict(octave=octave, angle=angle, desc=desc), prev


def test_real_frame_inputs_show_the_events_on_the_oracle_extraction(po, configs):
    """the conditions tests/test_gpu_search_init.py asserts on the device's extraction, on the CPU oracle's extraction of the same images: drawn F1
    arrays give displaced claims, hidden candidates and at least np_min = 50 matches; a kept left view against its right view gives 50 too"""
    from jetson_slam_amd.synth import synth_stereo_pair
    c = configs["c1"]
    left, right = synth_stereo_pair(41, c["h"], c["w"])
    frames = []
    for img in (left, right):
        o = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"], th_fast_max=c["th"])
        o.extract(img)
        kp = o.keypoints().copy()
        n = len(kp) // 6
        frames.append(frame_from_extract(kp, o.descriptors().copy(), kp[:n].astype(np.float32), kp[n:2 * n].astype(np.float32), c["w"], c["h"]))
    F2 = frames[1]
    F1, prev = f1_drawn_from(np.random.default_rng(1), F2, 2 * int((F2["octave"] == 0).sum()))
    for rot in (1, 0):
        prm = default_params(check_orientation=rot)
        ref = search_for_initialization(F1, F2, prev, prm)
        agree(ref, search_init_restated(F1, F2, prev, prm))
        assert ref[2] >= 50 and ref[4]["displaced"] > 0 and ref[4]["hidden"] > 0, (ref[2], ref[4])
    assert ref[4]["culled"] == 0 and search_for_initialization(F1, F2, prev, default_params())[4]["culled"] > 0
    K1, prev1 = f1_from_frame(frames[0])
    ref = search_for_initialization(K1, F2, prev1, default_params())
    st = agree(ref, search_init_restated(K1, F2, prev1, default_params()))
    assert ref[2] >= 50 and st[1] > ref[2], (ref[2], st)
    # the second call consumes the first one's vbPrevMatched
    again = search_for_initialization(K1, frames[0], ref[3], default_params())
    agree(again, search_init_restated(K1, frames[0], ref[3], default_params()))
    assert again[2] >= 50


# ---- the declarations ----
def test_header_binding_and_build_declare_the_new_entry_points(orb):
    names = ("jsorb_search_for_initialization_async", "jsorb_search_for_initialization", "jsorb_search_for_initialization_stats",
             "jsorb_init_reference_set", "jsorb_init_reference_clear", "jsorb_init_reference_n", "jsorb_search_initial_frame")
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    src = open(orb.__file__).read()
    for n in names:
        assert hasattr(lib, n) and n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
    assert ctypes.sizeof(orb.JsorbInitParams) == 40
    for m in ("search_for_initialization", "search_for_initialization_stats", "set_initial_frame", "clear_initial_frame", "search_initial_frame"):
        assert callable(getattr(orb.ORBExtractor, m))
    from jetson_slam_amd import build as jb
    assert "k_search_init.hip" in jb.SOURCES and jb.VARIANTS["tiny_init_cap"] == (["-DSI_CAP=2"], ["k_search_init.hip"])
    assert "search_for_initialization" in jb.EXAMPLES
    ksrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_search_init.hip")).read()
    assert re.search(r"#define SI_CAP %d\b" % SI_CAP, ksrc) and re.search(r"#define SI_CHUNK %d\b" % SI_CHUNK, ksrc)
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert re.search(r"inline int SearchForInitialization\(", shim)


def test_example_compiles_against_the_opencv_double(orb, tmp_path):
    from jetson_slam_amd import build as jb
    exe = jb.build_example("search_for_initialization", str(tmp_path / "search_for_initialization"),
                           ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")])
    assert os.path.exists(exe)


def test_validation_without_a_device(orb):
    """argument checks that need no GPU: a null handle"""
    lib = orb.load_library()
    prm = orb.make_init_params((0.0, 0.0, 0.2, 0.2))
    assert (prm.window, prm.th_low, prm.check_orientation, prm.cols, prm.rows) == (50.0, 50, 1, 64, 48) and abs(prm.nn_ratio - 0.9) < 1e-7
    n = ctypes.c_int()
    assert lib.jsorb_search_for_initialization_async(None, 0, ctypes.byref(prm), 0, *([None] * 7)) != 0
    assert lib.jsorb_search_for_initialization(None, 0, ctypes.byref(prm), 0, *([None] * 6), ctypes.byref(n)) != 0
    assert lib.jsorb_search_for_initialization_stats(None, None, None, None, None, None) != 0
    assert lib.jsorb_init_reference_set(None, 0) != 0 and lib.jsorb_init_reference_clear(None) != 0 and lib.jsorb_init_reference_n(None) < 0
    assert lib.jsorb_search_initial_frame(None, 0, ctypes.byref(prm), None, None, ctypes.byref(n)) != 0
