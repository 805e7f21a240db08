"""CPU: the keyframe-to-keyframe matcher of jsorb_search_for_triangulation* (include/jsorb.h) - ORBmatcher::SearchForTriangulation
(ORBmatcher.cpp:644-810) with CheckDistEpipolarLine (:127-144) and ComputeThreeMaxima (:2097-2138), one KF2 at a time.  A literal, sequential
transcription in numpy float32 / float64 scalars is the yardstick: a dict-of-lists FeatureVector walked with the two-iterator lower_bound loop,
bestDist falling in walk order, vbMatched2 read and never set.  The restatement is the kernels' formulation: the keys node << 18 | index sorted
ascending, 16 lanes per sorted KF1 position that each keep the minimum of d << 18 | (2^18 - 1 - t) over their entries lane, lane + 16, ..., the
minimum over the lanes, an integer histogram over idx1.  They must agree on random and on constructed cases.  tests/test_gpu_triangulation.py holds
the device to both."""
import ctypes
import os
import re
from bisect import bisect_left

import numpy as np
import pytest

from test_bow_host import as_ints, dist, feature_vector, flip_bits, sort_keys
from test_search_last_frame_host import HISTO_LENGTH, ROTATION_CULL, compute_three_maxima, rot_bin, rotation_cull_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
TR_LANES, TR_IDX, TR_KF_CHUNK = 16, 18, 32         # k_triangulate.hip / jsorb_launch.h
NOKEY = 2 ** 64 - 1
NOMATCH = 2 ** 32 - 1


def scale_tables(n_levels=8, factor=1.2):
    """mvScaleFactors / mvLevelSigma2 as ORBextractor.cpp:43-71 builds them: float32 recurrence, sigma2 = scale * scale"""
    s = np.ones(n_levels, np.float32)
    for i in range(1, n_levels):
        s[i] = f32(s[i - 1] * f32(factor))
    return s, (s * s).astype(np.float32)


def default_params(**kw):
    """ORBmatcher matcher(0.6, false) of CreateNewMapPoints (LocalMapping.cpp:221) has check_orientation = 0; the tests mostly switch it on"""
    s, s2 = scale_tables()
    p = dict(th_low=50, check_orientation=1, only_stereo=0, n_levels=len(s), scale_factor=s, level_sigma2=s2)
    p.update(kw)
    return p


def geometry(F12, ex, ey):
    return dict(F12=np.ascontiguousarray(F12, np.float32).reshape(9), ex=f32(ex), ey=f32(ey))


# ---- the yardstick: a literal transcription, sequential ----
def check_dist_epipolar_line(x1, y1, x2, y2, F12, sigma2, float_threshold=False):
    """ORBmatcher::CheckDistEpipolarLine (:127-144): float32 left to right, the comparison in double (float_threshold: the variant that would
    compare against the float product 3.84f * sigma2 - NOT the reference; the tests show that it differs)"""
    F = F12
    a = x1 * F[0] + y1 * F[3] + F[6]
    b = x1 * F[1] + y1 * F[4] + F[7]
    c = x1 * F[2] + y1 * F[5] + F[8]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    dsqr = num * num / den
    assert all(isinstance(t, np.float32) for t in (a, b, c, num, den, dsqr))
    if float_threshold:
        return bool(dsqr < f32(3.84) * sigma2)
    return bool(float(dsqr) < 3.84 * float(sigma2))


def search_for_triangulation_reference(KF1, KF2, geom, prm, float_threshold=False):
    """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo): (vMatches12[n1], nmatches, vMatchedPairs, trace).
    KF1: node, free, stereo, x, y, angle, desc; KF2: the same and octave; geom: F12[9], ex, ey."""
    n1, n2 = len(KF1["node"]), len(KF2["node"])
    d1s, d2s = as_ints(KF1["desc"]), as_ints(KF2["desc"])
    F12, ex, ey = np.asarray(geom["F12"], np.float32), f32(geom["ex"]), f32(geom["ey"])
    TH_LOW, bOnlyStereo = int(prm["th_low"]), bool(prm["only_stereo"])
    x1s, y1s, x2s, y2s = (np.asarray(a, np.float32) for a in (KF1["x"], KF1["y"], KF2["x"], KF2["y"]))
    sf, s2 = np.asarray(prm["scale_factor"], np.float32), np.asarray(prm["level_sigma2"], np.float32)
    nmatches = 0
    vbMatched2 = [False] * n2                        # :664 - read at :712, never set in this reference
    vMatches12 = np.full(n1, -1, np.int64)
    rotHist = [[] for _ in range(HISTO_LENGTH + 1)]
    keys1, vFeatVec1 = feature_vector(KF1["node"])
    keys2, vFeatVec2 = feature_vector(KF2["node"])
    tr = dict(node_pairs=0, distances=0, line_tests=0, largest_node=0, ind=(-1, -1, -1), gate_skips=0, line_fails=0, line_passes=0, culled=0,
              ties_replaced=0, pruned=0, bad_octave=0)
    f1it, f2it = 0, 0
    with np.errstate(all="ignore"):
        while f1it != len(keys1) and f2it != len(keys2):
            if keys1[f1it] == keys2[f2it]:
                idxs1, idxs2 = vFeatVec1[keys1[f1it]], vFeatVec2[keys2[f2it]]
                tr["node_pairs"] += 1
                tr["largest_node"] = max(tr["largest_node"], len(idxs2))
                for idx1 in idxs1:
                    if not KF1["free"][idx1]:            # pMP1
                        continue
                    bStereo1 = bool(KF1["stereo"][idx1])
                    if bOnlyStereo and not bStereo1:
                        continue
                    bestDist, bestIdx2 = TH_LOW, -1
                    for idx2 in idxs2:
                        if vbMatched2[idx2] or not KF2["free"][idx2]:
                            continue
                        bStereo2 = bool(KF2["stereo"][idx2])
                        if bOnlyStereo and not bStereo2:
                            continue
                        d = dist(d1s[idx1], d2s[idx2])
                        tr["distances"] += 1
                        octave = int(KF2["octave"][idx2])
                        in_range = 0 <= octave < prm["n_levels"]
                        gate = False                         # the epipole gate skips this entry (:730-736)
                        if in_range and not bStereo1 and not bStereo2:
                            distex = ex - x2s[idx2]
                            distey = ey - y2s[idx2]
                            gate = bool(distex * distex + distey * distey < f32(100) * sf[octave])
                        # trace only: the entries that come to the line test whatever the walk so far made of bestDist
                        tr["line_tests"] += d <= TH_LOW and in_range and not gate
                        if d > TH_LOW or d > bestDist:
                            tr["pruned"] += d <= TH_LOW
                            continue
                        if not in_range:                     # defined by include/jsorb.h: the entry never passes
                            tr["bad_octave"] += 1
                            continue
                        if gate:
                            tr["gate_skips"] += 1
                            continue
                        if check_dist_epipolar_line(x1s[idx1], y1s[idx1], x2s[idx2], y2s[idx2], F12, s2[octave], float_threshold):
                            tr["ties_replaced"] += bestIdx2 >= 0 and d == bestDist
                            bestIdx2 = idx2
                            bestDist = d
                            tr["line_passes"] += 1
                        else:
                            tr["line_fails"] += 1
                    if bestIdx2 >= 0:
                        vMatches12[idx1] = bestIdx2
                        nmatches += 1
                        if prm["check_orientation"]:
                            rotHist[rot_bin(KF1["angle"][idx1], KF2["angle"][bestIdx2])].append(idx1)
                f1it += 1
                f2it += 1
            elif keys1[f1it] < keys2[f2it]:
                f1it = bisect_left(keys1, keys2[f2it])       # vFeatVec1.lower_bound(f2it->first)
            else:
                f2it = bisect_left(keys2, keys1[f1it])
    if prm["check_orientation"]:
        ind = compute_three_maxima([len(h) for h in rotHist])
        tr["ind"] = tuple(ind)
        for i in range(HISTO_LENGTH + 1):
            if i in ind:
                continue
            for idx1 in rotHist[i]:
                vMatches12[idx1] = -1
                nmatches -= 1
                tr["culled"] += 1
    vMatchedPairs = [(i, int(vMatches12[i])) for i in range(n1) if vMatches12[i] >= 0]
    return vMatches12, nmatches, vMatchedPairs, tr


# ---- the restatement of the kernels ----
def search_for_triangulation_restated(KF1, KF2, geom, prm, lanes=TR_LANES, network=False):
    """k_bow_group (KF1 as the frame side) + k_tri_match + k_tri_resolve for one keyframe:
    (match12[n1], nmatches, (node pairs, distances, line tests, largest node, (ind1..3)))"""
    n1, n2 = len(KF1["node"]), len(KF2["node"])
    row = np.full(n1, -1, np.int64)
    if n1 == 0 or n2 == 0:
        return row, 0, (0, 0, 0, 0, (-1, -1, -1))
    d1s, d2s = as_ints(KF1["desc"]), as_ints(KF2["desc"])
    G = np.concatenate([np.asarray(geom["F12"], np.float32), [f32(geom["ex"]), f32(geom["ey"])]]).astype(np.float32)
    th_low, only_stereo, n_levels = int(prm["th_low"]), bool(prm["only_stereo"]), int(prm["n_levels"])
    gate = [f32(100.0) * f32(s) for s in prm["scale_factor"]]                    # the host's tables
    line = [3.84 * float(f32(s)) for s in prm["level_sigma2"]]
    x1s, y1s, x2s, y2s = (np.asarray(a, np.float32) for a in (KF1["x"], KF1["y"], KF2["x"], KF2["y"]))
    mask = 2 ** TR_IDX - 1
    s1, s2 = sort_keys(KF1["node"], network), sort_keys(KF2["node"], network)
    pairs = n_dist = n_line = largest = 0
    with np.errstate(all="ignore"):
        for p in range(n1):                              # one group of lanes per sorted position, in any order
            k1 = s1[p]
            if k1 == NOKEY:
                continue
            v, idx1 = k1 >> TR_IDX, k1 & mask
            head = p == 0 or s1[p - 1] >> TR_IDX != v
            stereo1 = bool(KF1["stereo"][idx1])
            take = bool(KF1["free"][idx1]) and (not only_stereo or stereo1)
            if not (head or take):
                continue
            fb = bisect_left(s2, v << TR_IDX)
            m = bisect_left(s2, (v + 1) << TR_IDX) - fb
            if head and m > 0:
                pairs += 1
                largest = max(largest, m)
            if not take or m == 0:
                continue
            x1, y1 = x1s[idx1], y1s[idx1]
            la = x1 * G[0] + y1 * G[3] + G[6]
            lb = x1 * G[1] + y1 * G[4] + G[7]
            lc = x1 * G[2] + y1 * G[5] + G[8]
            den = la * la + lb * lb
            key = NOMATCH
            for lane in range(min(lanes, m)):
                lkey = NOMATCH
                for t in range(lane, m, lanes):
                    j = s2[fb + t] & mask
                    if not KF2["free"][j]:
                        continue
                    stereo2 = bool(KF2["stereo"][j])
                    if only_stereo and not stereo2:
                        continue
                    d = dist(d1s[idx1], d2s[j])
                    n_dist += 1
                    if d > th_low:
                        continue
                    octave = int(KF2["octave"][j])
                    if not 0 <= octave < n_levels:
                        continue
                    x2, y2 = x2s[j], y2s[j]
                    if not stereo1 and not stereo2:
                        distex, distey = G[9] - x2, G[10] - y2
                        if distex * distex + distey * distey < gate[octave]:
                            continue
                    n_line += 1
                    if d > lkey >> TR_IDX:
                        continue
                    num = la * x2 + lb * y2 + lc
                    if den == 0:
                        continue
                    dsqr = num * num / den
                    if not float(dsqr) < line[octave]:
                        continue
                    lkey = min(lkey, d << TR_IDX | (mask - t))
                key = min(key, lkey)
            if key != NOMATCH:
                row[idx1] = s2[fb + (mask - (key & mask))] & mask
    ind = (-1, -1, -1)
    nmatches = int((row >= 0).sum())
    if prm["check_orientation"]:
        bins = {int(k): rot_bin(KF1["angle"][k], KF2["angle"][row[k]]) for k in np.nonzero(row >= 0)[0]}
        hist = [0] * (HISTO_LENGTH + 1)
        for b in bins.values():
            hist[b] += 1
        ind = tuple(compute_three_maxima(hist))
        for k, b in bins.items():
            if b not in ind:
                row[k] = -1
                nmatches -= 1
    return row, nmatches, (pairs, n_dist, n_line, largest, ind)


def agree(ref, res):
    assert np.array_equal(ref[0], res[0]) and ref[1] == res[1], (ref[1], res[1])
    tr = ref[3]
    assert (tr["node_pairs"], tr["distances"], tr["line_tests"], tr["largest_node"], tr["ind"]) == res[2], (tr, res[2])
    assert ref[2] == [(int(i), int(ref[0][i])) for i in np.nonzero(ref[0] >= 0)[0]] and len(ref[2]) == ref[1]
    return res[2]


def both_searches(KF1, KF2, geom, prm, network=False):
    ref = search_for_triangulation_reference(KF1, KF2, geom, prm)
    agree(ref, search_for_triangulation_restated(KF1, KF2, geom, prm, network=network))
    return ref


# ---- random cases: two views of one cloud of landmarks ----
K_CAM = (f32(458.0), f32(457.0), f32(367.0), f32(248.0))      # fx, fy, cx, cy


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def relative_pose(rng, forward=False):
    """R12, t12 with X1 = R12 X2 + t12: a small rotation, a baseline mostly sideways (forward: mostly along the axis - the epipole in the image)"""
    w = rng.normal(0, 0.05, 3)
    th = np.linalg.norm(w)
    Kx = skew(w / th)
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = np.array([0.02, 0.01, 0.5]) if forward else np.array([0.4, 0.03, 0.05])
    return R, t * rng.uniform(0.5, 1.5) + rng.normal(0, 0.01, 3)


def f12_and_epipole(R12, t12):
    """LocalMapping::ComputeF12 (F12 = K1^-T [t12]x R12 K2^-1) and the epipole of :651-657 (C2 = camera centre of KF1 in KF2), as float32 inputs"""
    fx, fy, cx, cy = (float(v) for v in K_CAM)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    Kinv = np.linalg.inv(K)
    F12 = (Kinv.T @ skew(t12) @ R12 @ Kinv).astype(np.float32)
    C2 = (-R12.T @ t12).astype(np.float32)
    invz = f32(1.0) / C2[2]
    return geometry(F12, K_CAM[0] * C2[0] * invz + K_CAM[2], K_CAM[1] * C2[1] * invz + K_CAM[3])


def random_case(rng, n1, n2, n_nodes, only_stereo=0, check_orientation=1, free=0.8, stereo=0.3, forward=False, noise=1.0, near_epipole=0.0,
                n_levels=8, th_low=50):
    """KF1 and KF2 observe one cloud of landmarks: a landmark has a node, a descriptor and a 3-D position; every keypoint takes a landmark, flips
    0..12 bits of its descriptor and sees its projection with pixel noise (which a real share of the candidates fails the line test by)"""
    fx, fy, cx, cy = (float(v) for v in K_CAM)
    R12, t12 = relative_pose(rng, forward)
    geom = f12_and_epipole(R12, t12)
    P = max(1, (n1 + n2) // 3)
    X2 = np.stack([rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(2, 10, P)], axis=1)
    X1 = X2 @ R12.T + t12
    pool = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    node = rng.integers(0, n_nodes, P)
    base_angle = rng.uniform(0, 360, P)
    s, s2 = scale_tables(n_levels)
    sides = []
    for n, X in ((n1, X1), (n2, X2)):
        src = rng.integers(0, P, n)
        octave = rng.integers(0, n_levels, n).astype(np.int32)
        sig = noise * np.asarray(s, np.float64)[octave] if n else np.zeros(0)
        x = fx * X[src, 0] / X[src, 2] + cx + rng.normal(0, 1, n) * sig
        y = fy * X[src, 1] / X[src, 2] + cy + rng.normal(0, 1, n) * sig
        nd = np.where(rng.random(n) < 0.05, -1, np.where(rng.random(n) < 0.1, rng.integers(0, n_nodes, n), node[src]))
        sides.append(dict(node=nd.astype(np.int32), free=(rng.random(n) < free).astype(np.uint8), stereo=(rng.random(n) < stereo).astype(np.uint8),
                          x=x.astype(np.float32), y=y.astype(np.float32), octave=octave,
                          angle=np.mod(base_angle[src] + np.where(rng.random(n) < 0.25, rng.uniform(0, 360, n), 14.0), 360.0).astype(np.float32),
                          desc=flip_bits(rng, pool[src], 0, 13) if n else np.zeros((0, 32), np.uint8)))
    KF1, KF2 = sides
    if near_epipole and n2:                                  # some KF2 keypoints around the epipole: on both sides of the gate's radius
        near = rng.random(n2) < near_epipole
        r = np.sqrt(100.0 * np.asarray(s, np.float64)[KF2["octave"]]) * rng.uniform(0.5, 1.5, n2)
        phi = rng.uniform(0, 2 * np.pi, n2)
        KF2["x"] = np.where(near, float(geom["ex"]) + r * np.cos(phi), KF2["x"]).astype(np.float32)
        KF2["y"] = np.where(near, float(geom["ey"]) + r * np.sin(phi), KF2["y"]).astype(np.float32)
    prm = default_params(th_low=th_low, check_orientation=check_orientation, only_stereo=only_stereo, n_levels=n_levels, scale_factor=s, level_sigma2=s2)
    return KF1, KF2, geom, prm


def draw_case(rng, case):
    n1, n2 = (int(250 * rng.random() ** 3) for _ in range(2))
    if case % 50 == 0:
        n1, n2 = 250, 250
    if case % 50 == 1:
        n2 = 0
    if case % 50 == 2:
        n1 = 0
    return random_case(rng, n1, n2, n_nodes=int(rng.choice([1, 2, 5, 12, 40])), only_stereo=int(rng.random() < 0.25),
                       check_orientation=int(rng.random() < 0.6), free=float(rng.choice([0.3, 0.8, 1.0])), stereo=float(rng.choice([0.0, 0.3, 0.7, 1.0])),
                       forward=bool(rng.random() < 0.4), noise=float(rng.choice([0.3, 1.0, 3.0])), near_epipole=float(rng.choice([0.0, 0.0, 0.3])),
                       n_levels=int(rng.choice([1, 3, 8])), th_low=int(rng.choice([50, 30, 80])))


@pytest.mark.parametrize("block", range(8))
def test_restatement_equals_the_transcription_on_random_cases(block):
    """8 x 250 = 2000 seeded cases: 1..40 nodes, 0..250 keypoints, shares of free and stereo keypoints, only_stereo, check_orientation, sideways and
    forward baselines, pixel noise below and above the line test's bound, keypoints around the epipole"""
    rng = np.random.default_rng(2000 + block)
    seen = dict(matches=0, gate_skips=0, line_fails=0, line_passes=0, culled=0, ties_replaced=0, pruned=0, shared=0, big_node=0)
    for case in range(250):
        KF1, KF2, geom, prm = draw_case(rng, case)
        ref = search_for_triangulation_reference(KF1, KF2, geom, prm)
        st = agree(ref, search_for_triangulation_restated(KF1, KF2, geom, prm, network=case % 5 == 0))
        seen["matches"] += ref[1]
        seen["big_node"] += st[3] > TR_LANES
        taken = ref[0][ref[0] >= 0]
        seen["shared"] += len(taken) - len(set(taken.tolist()))      # KF2 keypoints that more than one KF1 keypoint took
        for k in ("gate_skips", "line_fails", "line_passes", "culled", "ties_replaced", "pruned"):
            seen[k] += ref[3][k]
    assert all(v > 0 for v in seen.values()), seen
    assert seen["line_fails"] > seen["line_passes"] // 20 and seen["line_passes"] > seen["line_fails"] // 20, seen


# ---- constructed cases ----
def bits(d, start=0):
    """a descriptor with d bits set from bit `start`: Hamming distance d to the zero descriptor"""
    b = np.zeros(256, np.uint8)
    b[start:start + d] = 1
    return np.packbits(b, bitorder="little")


# the line x2 = 0: a = 1, b = 0, c = 0 for every x1, y1 - num = x2, den = 1, dsqr = x2 * x2
F_LINE = np.array([0, 0, 0, 0, 0, 0, 1, 0, 0], np.float32)
FAR = (f32(1e4), f32(1e4))                                   # an epipole no keypoint is near


def sides(kf2_dist, kf1_n=1, node1=None, node2=None, x2=None, y2=None, octave=None, free1=None, free2=None, stereo1=None, stereo2=None, angle1=None,
          angle2=None, x1=None, y1=None):
    """KF1: kf1_n zero descriptors; KF2: descriptors at the given distances from zero; everything in node 0, free, monocular, on the line, level 0"""
    n2 = len(kf2_dist)
    arr = lambda v, n, dt, fill: np.full(n, fill, dt) if v is None else np.asarray(v, dt)
    KF1 = dict(node=arr(node1, kf1_n, np.int32, 0), free=arr(free1, kf1_n, np.uint8, 1), stereo=arr(stereo1, kf1_n, np.uint8, 0),
               x=arr(x1, kf1_n, np.float32, 0), y=arr(y1, kf1_n, np.float32, 0), angle=arr(angle1, kf1_n, np.float32, 0),
               desc=np.zeros((kf1_n, 32), np.uint8))
    KF2 = dict(node=arr(node2, n2, np.int32, 0), free=arr(free2, n2, np.uint8, 1), stereo=arr(stereo2, n2, np.uint8, 0),
               x=arr(x2, n2, np.float32, 0), y=arr(y2, n2, np.float32, 0), octave=arr(octave, n2, np.int32, 0), angle=arr(angle2, n2, np.float32, 0),
               desc=np.stack([bits(d) for d in kf2_dist]) if n2 else np.zeros((0, 32), np.uint8))
    return KF1, KF2


def threshold_cases():
    """(num, sigma2) with dsqr = num * num (den = 1) next to the double bound 3.84 * (double)sigma2.  3.84f lies below 3.84, so the float product
    3.84f * sigma2 can only fall short of the double bound, and no float lies between the two when it is rounded up past it: the comparisons
    differ exactly on dsqr == 3.84f * sigma2 < 3.84 * (double)sigma2, which the double comparison accepts and the float one rejects ("below").
    "above" is the next float dsqr, on the other side of the double bound: both reject."""
    rng = np.random.default_rng(5)
    found = {}
    for _ in range(4000):
        s2 = f32(rng.uniform(1, 20))
        bound_d, bound_f = 3.84 * float(s2), f32(3.84) * s2
        up = np.nextafter(bound_f, f32(np.inf))
        if not (float(bound_f) < bound_d <= float(up)):
            continue
        got = {}
        for name, dsqr in (("below", bound_f), ("above", up)):
            num = np.sqrt(dsqr)
            for _ in range(8):
                num = np.nextafter(num, f32(0))
            for _ in range(16):
                if num * num == dsqr:
                    got[name] = (num, s2)
                num = np.nextafter(num, f32(np.inf))
        if len(got) == 2:
            found = got
            break
    assert len(found) == 2
    return found


ROTATION_KEPT = {"rotation_cull_removes_a_match": (0, -1, -1), "angle_outside_360_never_kept": (0, -1, -1)}      # case -> kept_bins


def _constructed():
    c = {}
    g = geometry(F_LINE, *FAR)
    prm = default_params(check_orientation=0)
    # name: (KF1, KF2, geom, prm, expected match12 of KF1, expected count)
    # vbMatched2 is never set: both KF1 keypoints take KF2 keypoint 1
    c["two_take_the_same"] = (*sides([30, 10, 20], kf1_n=2), g, prm, [1, 1], 2)
    # equal distances: the last in walk order that passes wins
    c["last_equal_wins"] = (*sides([20, 20, 25, 20]), g, prm, [3], 1)
    # ... but a later equal one that fails the line test (x2 = 5: dsqr = 25) does not, and leaves bestDist as it was
    c["later_equal_fails_the_line"] = (*sides([20, 20, 20], x2=[0, 0, 5]), g, prm, [1], 1)
    # a better one that fails the line leaves the worse passer
    c["better_fails_the_line"] = (*sides([30, 10], x2=[0, 5]), g, prm, [0], 1)
    c["th_low_accepted"] = (*sides([50]), g, prm, [0], 1)
    c["th_low_plus_one_not"] = (*sides([51]), g, prm, [-1], 0)
    # 17 entries with the winner tied between the first and the last lane, 33 with the tie between two entries of lane 0
    c["tie_across_lanes_17"] = (*sides([12] + [40] * 14 + [12, 40]), g, prm, [15], 1)
    c["tie_within_a_lane_33"] = (*sides([12] + [40] * 15 + [12] + [40] * 15 + [13]), g, prm, [16], 1)
    # the epipole gate: 10 px from the epipole at level 0 is 100 < 100 - not skipped; just inside is skipped; level 1 (scale 1.2) needs more
    ge = geometry(F_LINE, 10.0, 0.0)
    c["gate_at_equality_not_skipped"] = (*sides([10]), ge, prm, [0], 1)
    c["gate_inside_skipped"] = (*sides([10, 20], x2=[0.5, 0], y2=[0, -10]), ge, prm, [1], 1)
    c["gate_level_1_skipped"] = (*sides([10], octave=[1]), ge, prm, [-1], 0)
    # a stereo keypoint on either side skips the gate (x2 = 0.5 is 9.5 px from the epipole and passes the line: 0.25 < 3.84)
    c["both_stereo_skip_the_gate"] = (*sides([10], x2=[0.5], stereo1=[1], stereo2=[1]), ge, prm, [0], 1)
    c["stereo1_only_skips_the_gate"] = (*sides([10], x2=[0.5], stereo1=[1]), ge, prm, [0], 1)
    c["stereo2_only_skips_the_gate"] = (*sides([10], x2=[0.5], stereo2=[1]), ge, prm, [0], 1)
    c["mono_pair_is_gated"] = (*sides([10], x2=[0.5]), ge, prm, [-1], 0)
    # only_stereo: monocular keypoints of either side are skipped
    ps = default_params(check_orientation=0, only_stereo=1)
    c["only_stereo"] = (*sides([10, 20, 30], kf1_n=2, stereo1=[0, 1], stereo2=[0, 1, 1]), g, ps, [-1, 1], 1)
    # keypoints with a map point on either side
    c["not_free"] = (*sides([10, 20], kf1_n=2, free1=[0, 1], free2=[0, 1]), g, prm, [-1, 1], 1)
    # den == 0: F12 all zero
    c["den_zero"] = (*sides([10]), geometry(np.zeros(9), *FAR), prm, [-1], 0)
    # NaN and inf in F12, in the epipole and in the points: nothing passes through a NaN; a NaN epipole does not gate
    nanF = F_LINE.copy(); nanF[6] = np.nan
    infF = F_LINE.copy(); infF[6] = np.inf
    c["nan_in_f12"] = (*sides([10, 20]), geometry(nanF, *FAR), prm, [-1], 0)
    c["inf_in_f12"] = (*sides([10, 20]), geometry(infF, *FAR), prm, [-1], 0)             # num = inf, den = inf: NaN
    c["nan_epipole_does_not_gate"] = (*sides([10]), geometry(F_LINE, np.nan, 0.0), prm, [0], 1)
    c["nan_and_inf_points"] = (*sides([10, 11, 12, 13], x2=[np.nan, np.inf, 0, 0], y2=[0, 0, np.nan, 0]), g, prm, [3], 1)
    c["nan_x1"] = (*sides([10], x1=[np.nan]), geometry(np.array([1, 0, 0, 0, 0, 0, 1, 0, 0], np.float32), *FAR), prm, [-1], 0)
    # octave outside [0, n_levels): never passes
    c["octave_out_of_range"] = (*sides([10, 11, 30], octave=[-1, 8, 7]), g, prm, [2], 1)
    # nodes: one side only, interleaved ids, keypoints in no node
    c["node_on_one_side_only"] = (*sides([10, 10], kf1_n=2, node1=[3, 5], node2=[4, 5]), g, prm, [-1, 1], 1)
    c["no_node"] = (*sides([10, 10], kf1_n=2, node1=[-1, 2], node2=[-1, 2]), g, prm, [-1, 1], 1)
    c["large_node_ids"] = (*sides([10, 12], kf1_n=2, node1=[2 ** 31 - 1, 0], node2=[2 ** 31 - 1, 2 ** 31 - 2]), g, prm, [0, -1], 1)
    # all keypoints in one node: 40 x 40, everyone takes the best that lies on the line
    c["all_in_one_node"] = (*sides([40 - i for i in range(40)], kf1_n=40, x2=[0] * 39 + [5]), g, prm, [38] * 40, 40)
    # empty sides
    c["empty_kf2"] = (*sides([], kf1_n=3), g, prm, [-1, -1, -1], 0)
    c["empty_kf1"] = (*sides([10], kf1_n=0), g, prm, [], 0)
    # the rotation cull removes the lone match of another bin: rot 0 three times (bin 0), rot 300 once (bin 10; 1 >= 0.1 * 3 keeps it), and
    # with eleven in bin 0 the lone one is below a tenth and goes
    pr = default_params()
    c["rotation_cull_keeps_a_tenth"] = (*sides([10] * 4, kf1_n=4, node1=[0, 1, 2, 3], node2=[0, 1, 2, 3], angle1=[0, 0, 0, 300]), g, pr, [0, 1, 2, 3], 4)
    n = 12
    c["rotation_cull_removes_a_match"] = (*sides([10] * n, kf1_n=n, node1=list(range(n)), node2=list(range(n)), angle1=[0] * (n - 1) + [300]), g, pr,
                                         list(range(n - 1)) + [-1], n - 1)
    c["angle_outside_360_never_kept"] = (*sides([10, 10], kf1_n=2, node1=[0, 1], node2=[0, 1], angle1=[0, 1000]), g, pr, [0, -1], 1)
    # the rotation check's edges (ROTATION_CULL; its "eleven_and_one" and "outside_360" are the two cases above): four equal bins, ten and one, and
    # the check switched off
    for name, on in (("four_equal_bins", 1), ("ten_and_one", 1), ("four_equal_bins", 0)):
        rots = ROTATION_CULL[name]
        n = len(rots)
        ind, kept = rotation_cull_expected(rots, on)
        key = "rotation_%s%s" % (name, "" if on else "_check_off")
        c[key] = (*sides([10] * n, kf1_n=n, node1=list(range(n)), node2=list(range(n)), angle1=rots), g, default_params(check_orientation=on),
                  [i if kept[i] else -1 for i in range(n)], int(kept.sum()))
        ROTATION_KEPT[key] = ind
    # the double threshold: dsqr on either side of 3.84 * (double)sigma2, the lower one equal to the float product 3.84f * sigma2
    th = threshold_cases()
    for name, want in (("below", [0]), ("above", [-1])):
        num, s2 = th[name]
        p = default_params(check_orientation=0, n_levels=1, scale_factor=np.ones(1, np.float32), level_sigma2=np.array([s2], np.float32))
        c["threshold_" + name] = (*sides([10], x2=[num]), g, p, want, len([w for w in want if w >= 0]))
    return c


CONSTRUCTED = _constructed()


@pytest.mark.parametrize("name", sorted(CONSTRUCTED))
def test_constructed_cases(name):
    KF1, KF2, geom, prm, want, count = CONSTRUCTED[name]
    ref = both_searches(KF1, KF2, geom, prm)
    assert list(ref[0]) == want and ref[1] == count, (name, list(ref[0]), ref[1])
    assert name not in ROTATION_KEPT or tuple(ref[3]["ind"]) == ROTATION_KEPT[name]
    both_searches(KF1, KF2, geom, prm, network=True)


def test_the_threshold_cases_tell_the_double_from_the_float_comparison():
    """not vacuous: on the lower case the transcription with the float product 3.84f * sigma2 decides the other way; on the upper one both reject"""
    KF1, KF2, geom, prm, want, count = CONSTRUCTED["threshold_below"]
    ref = search_for_triangulation_reference(KF1, KF2, geom, prm)
    var = search_for_triangulation_reference(KF1, KF2, geom, prm, float_threshold=True)
    assert (ref[1], list(ref[0])) == (1, [0]) and (var[1], list(var[0])) == (0, [-1])
    KF1, KF2, geom, prm, want, count = CONSTRUCTED["threshold_above"]
    assert search_for_triangulation_reference(KF1, KF2, geom, prm)[1] == 0 and search_for_triangulation_reference(KF1, KF2, geom, prm, float_threshold=True)[1] == 0


def test_trace_shows_what_the_cases_are_about():
    tr = lambda name: search_for_triangulation_reference(*CONSTRUCTED[name][:4])[3]
    assert tr("last_equal_wins")["ties_replaced"] == 2 and tr("later_equal_fails_the_line")["line_fails"] == 1
    assert tr("gate_inside_skipped")["gate_skips"] == 1 and tr("gate_at_equality_not_skipped")["gate_skips"] == 0
    assert tr("mono_pair_is_gated")["gate_skips"] == 1 and tr("both_stereo_skip_the_gate")["gate_skips"] == 0
    assert tr("octave_out_of_range")["bad_octave"] == 2 and tr("rotation_cull_removes_a_match")["culled"] == 1
    assert tr("all_in_one_node")["largest_node"] == 40 and tr("all_in_one_node")["node_pairs"] == 1
    t = tr("tie_within_a_lane_33")
    assert (t["distances"], t["line_tests"], t["pruned"]) == (33, 33, 31)      # the walk prunes 31 entries; the order-free count takes all 33


# ---- the declarations ----
NAMES = ("jsorb_keyframe_matcher_create", "jsorb_keyframe_matcher_destroy", "jsorb_keyframe_matcher_set_stream", "jsorb_keyframe_matcher_get_stream",
         "jsorb_keyframe_matcher_last_error", "jsorb_search_for_triangulation_async", "jsorb_search_for_triangulation",
         "jsorb_search_for_triangulation_stats")


def test_header_binding_and_build_declare_the_new_entry_points(orb):
    lib = ctypes.CDLL(os.path.join(ROOT, "jetson_slam_amd", "libjsorb.so"))
    bound = orb.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsorb.h")).read(), flags=re.S)
    src = open(orb.__file__).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in orb.EXPORTS and '"%s": (' % n in src, n
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, hdr)
        assert decl, n
        n_args = len([a for a in decl.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(getattr(bound, n).argtypes), (n, n_args)
    assert len(orb.load_library().jsorb_search_for_triangulation_async.argtypes) == 24
    assert ctypes.sizeof(orb.JsorbTriangulationParams) == 16 + 2 * 4 * orb.MAX_LEVELS
    assert re.search(r"typedef struct jsorb_keyframe_matcher jsorb_keyframe_matcher;", hdr) and "vbMatched2" in open(os.path.join(ROOT, "include", "jsorb.h")).read()
    for m in ("search_for_triangulation", "search_for_triangulation_host", "stats", "set_stream", "get_stream", "close"):
        assert callable(getattr(orb.KeyframeMatcher, m))
    assert callable(orb.make_triangulation_params) and callable(orb.matched_pairs)
    from jetson_slam_amd import build as jb
    assert "k_triangulate.hip" in jb.SOURCES and "jsorb_keyframes.hip" in jb.SOURCES and "create_new_map_points" in jb.EXAMPLES
    ksrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_triangulate.hip")).read()
    lsrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "jsorb_launch.h")).read()
    csrc = open(os.path.join(ROOT, "jetson_slam_amd", "csrc", "k_search_common.h")).read()      # k_bow_group's key layout, shared with k_bow.hip
    for name, val, text in (("TR_LANES", TR_LANES, ksrc), ("BW_IDX", TR_IDX, csrc), ("TR_KF_CHUNK", TR_KF_CHUNK, lsrc)):
        assert re.search(r"#define %s %d\b" % (name, val), text), name
    assert "fma" not in re.sub(r"//.*", "", ksrc)                        # the contract's arithmetic has no fused multiply-add
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    assert re.search(r"class KeyframeMatcher \{", shim) and re.search(r"inline std::vector<int> SearchForTriangulation\(", shim)


def test_params_and_pairs_helpers(orb):
    s, s2 = scale_tables()
    p = orb.make_triangulation_params(s)
    assert (p.th_low, p.check_orientation, p.only_stereo, p.n_levels) == (50, 1, 0, 8)
    assert np.array_equal(np.array(p.scale_factor[:8], np.float32), s) and np.array_equal(np.array(p.level_sigma2[:8], np.float32), s2)
    with pytest.raises(orb.JsorbError):
        orb.make_triangulation_params(s, s2[:3])
    assert orb.matched_pairs(np.array([-1, 4, -1, 0])).tolist() == [[1, 4], [3, 0]] and orb.matched_pairs(np.full(3, -1)).shape == (0, 2)


def test_shim_compiles_with_and_without_the_opencv_double(orb, tmp_path):
    """include/jsorb_compat.hpp: jsorb::KeyframeMatcher, jsorb::KeyframeSide and Jetson_SLAM::SearchForTriangulation compile with plain g++ and link"""
    import subprocess
    src = tmp_path / "triangulation_shim.cpp"
    src.write_text('#include "jsorb_compat.hpp"\n'
                   "int main(int argc, char **) {\n"
                   "    if (argc < 100) return 0;                // compiled and linked, not run: no device here\n"
                   "    jsorb::KeyframeMatcher m; jsorb::KeyframeSide a, b; jsorb_triangulation_params p{}; const int32_t ks[2] = {0, 0};\n"
                   "    const float F[9] = {0}, e[2] = {0}; std::vector<std::vector<std::pair<size_t, size_t>>> pairs;\n"
                   "    return (int)Jetson_SLAM::SearchForTriangulation(m, p, a, 1, ks, b, F, e, pairs).size();\n}\n")
    lib = os.path.join(ROOT, "jetson_slam_amd")
    for extra in ([], ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")]):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + extra +
                              [str(src), "-L", lib, "-ljsorb", "-lpthread", "-Wl,-rpath," + lib, "-o", str(tmp_path / "triangulation_shim")])


def test_example_compiles_against_the_opencv_double(orb, tmp_path):
    from jetson_slam_amd import build as jb
    exe = jb.build_example("create_new_map_points", str(tmp_path / "create_new_map_points"), ["-I", os.path.join(ROOT, "tests", "cpp", "opencv_double")])
    assert os.path.exists(exe)


def test_validation_without_a_device(orb):
    """argument checks that need no GPU: a NULL matcher is refused by every entry point"""
    lib = orb.load_library()
    prm = orb.make_triangulation_params(scale_tables()[0])
    ks = np.zeros(2, np.int32)
    assert lib.jsorb_keyframe_matcher_create(0, None) == -1
    out = ctypes.c_void_p()
    assert lib.jsorb_keyframe_matcher_create(-1, ctypes.byref(out)) == -1 and not out.value
    lib.jsorb_keyframe_matcher_destroy(None)
    assert lib.jsorb_keyframe_matcher_set_stream(None, None) != 0 and not lib.jsorb_keyframe_matcher_get_stream(None)
    args = [ctypes.byref(prm), 0] + [None] * 7 + [1, ks.ctypes.data] + [None] * 12
    assert lib.jsorb_search_for_triangulation_async(None, *args) == -1 and lib.jsorb_search_for_triangulation(None, *args) == -1
    assert lib.jsorb_search_for_triangulation_stats(None, None, None, None, None, None) == -1
