"""Cases and restatements for jsorb_local_map_points (include/jsorb.h), shared by tests/test_local_map_host.py and tests/test_gpu_local_map.py.
numpy and the CPU oracle only: nothing here needs a GPU.  Not a test module.

* update_local_points_restated: a literal transcription of the reference's three loops - the frame marks of Tracking::SearchLocalPoints
  (Tracking.cpp:1352-1367), Tracking::UpdateLocalPoints (:1818-1841) and the map_points list (:1410-1420) - over map-point objects with the
  reference's own fields (mnTrackReferenceForFrame, mnLastFrameSeen), so the dedupe is its mechanism and not a set;
* update_local_points_numpy: the same lists from array operations;
* the world: a synth stereo frame at the c1 configuration through the oracle, a table of N_ROWS map points back-projected from its keypoints the
  way tests/test_gpu_search_local.py::_local_map does, a share of them moved behind the camera, outside the image, outside the distance range and
  beyond the view angle, so that every exit of K16 is taken;
* the cases: keyframes as runs of table rows with everything the contract names - see CASES and build_case."""
import functools

import numpy as np

f32 = np.float32
N_ROWS = 2048
CHUNKS = (1024, 64)                              # LM_CHUNK of the shipped library and of the tiny_local_map build (jetson_slam_amd/build.py VARIANTS)
WORLD_CONFIG, WORLD_SEED = "c1", 17
REASONS = ("n_null", "n_invalid_rows", "n_duplicates", "n_bad", "n_seen")


# ---------------------------------------------------------------- the reference's loops, literally
class MapPoint:
    __slots__ = ("row", "bad", "mnTrackReferenceForFrame", "mnLastFrameSeen", "mbTrackInView", "nVisible")

    def __init__(self, row, bad):
        self.row, self.bad = row, bool(bad)
        self.mnTrackReferenceForFrame = 0
        self.mnLastFrameSeen = 0
        self.mbTrackInView = False
        self.nVisible = 1

    def isBad(self):
        return self.bad


MUTANTS = ("filter_dropped", "marks_for_bad_frame_points", "list_by_row", "duplicate_after_bad")


def update_local_points_restated(bad, keyframes, frame_rows, frame_id=7, mutant=None):
    """bad: uint8[n_rows]; keyframes: the local keyframes in order, each the int rows of its GetMapPointMatches(); frame_rows: the rows of
    mCurrentFrame.mvpMapPoints or None.  A negative row is the NULL pointer; a row >= n_rows names no map point: dropped and counted.
    Returns dict(blocked_in, local, map_points, stats): the rows of mvpLocalMapPoints and of map_points in order.  mutant: one of MUTANTS, a
    decision of the reference's text flipped (tests/test_ref_tracking.py shows that the recorded reference output notices each but the last)."""
    assert mutant is None or mutant in MUTANTS
    n_rows = len(bad)
    points = [MapPoint(r, bad[r]) for r in range(n_rows)]
    lookup = lambda r: points[r] if 0 <= r < n_rows else None
    stats = dict(n_entries=int(sum(len(k) for k in keyframes)), n_null=0, n_invalid_rows=0, n_duplicates=0, n_bad=0, n_seen=0)
    # Tracking.cpp:1352-1367
    mvpMapPoints = [lookup(int(r)) for r in frame_rows] if frame_rows is not None else []
    for i, pMP in enumerate(mvpMapPoints):
        if pMP:
            if pMP.isBad() and mutant != "marks_for_bad_frame_points":
                mvpMapPoints[i] = None
            else:
                pMP.nVisible += 1
                pMP.mnLastFrameSeen = frame_id
                pMP.mbTrackInView = False
    # Tracking.cpp:1818-1841
    mvpLocalMapPoints = []
    for vpMPs in keyframes:
        for r in vpMPs:
            r = int(r)
            if r >= n_rows:
                stats["n_invalid_rows"] += 1
                continue
            pMP = lookup(r)
            if not pMP:
                stats["n_null"] += 1
                continue
            if mutant == "duplicate_after_bad" and pMP.isBad():
                stats["n_bad"] += 1
                continue
            if pMP.mnTrackReferenceForFrame == frame_id:
                stats["n_duplicates"] += 1
                continue
            if not pMP.isBad():
                mvpLocalMapPoints.append(pMP)
                pMP.mnTrackReferenceForFrame = frame_id
            else:
                stats["n_bad"] += 1
    if mutant == "list_by_row":
        mvpLocalMapPoints.sort(key=lambda p: p.row)
    # Tracking.cpp:1410-1420
    map_points = []
    for pMP in mvpLocalMapPoints:
        if pMP.mnLastFrameSeen == frame_id and mutant != "filter_dropped":
            stats["n_seen"] += 1
            continue
        if pMP.isBad():
            continue
        map_points.append(pMP)
    return dict(blocked_in=np.array([1 if p else 0 for p in mvpMapPoints], np.uint8), local=np.array([p.row for p in mvpLocalMapPoints], np.int32),
                map_points=np.array([p.row for p in map_points], np.int32), stats=stats)


def update_local_points_numpy(bad, keyframes, frame_rows):
    n_rows = len(bad)
    e = np.concatenate([np.asarray(k, np.int64) for k in keyframes]) if len(keyframes) else np.zeros(0, np.int64)
    null, invalid = e < 0, e >= n_rows
    inside = ~null & ~invalid
    is_bad = np.zeros(len(e), bool)
    is_bad[inside] = bad[e[inside]] != 0
    cand = np.nonzero(inside & ~is_bad)[0]
    _, first = np.unique(e[cand], return_index=True)
    keep = np.zeros(len(e), bool)
    keep[cand[first]] = True
    local = e[keep]
    seen_row = np.zeros(n_rows, bool)
    blocked = np.zeros(0, np.uint8)
    if frame_rows is not None:
        fr = np.asarray(frame_rows, np.int64)
        ok = (fr >= 0) & (fr < n_rows)
        ok[ok] = bad[fr[ok]] == 0
        seen_row[fr[ok]] = True
        blocked = ok.astype(np.uint8)
    seen = seen_row[local]
    stats = dict(n_entries=len(e), n_null=int(null.sum()), n_invalid_rows=int(invalid.sum()), n_duplicates=int((inside & ~is_bad & ~keep).sum()),
                 n_bad=int(is_bad.sum()), n_seen=int(seen.sum()))
    return dict(blocked_in=blocked, local=local.astype(np.int32), map_points=local[~seen].astype(np.int32), stats=stats)


# ---------------------------------------------------------------- the world
@functools.lru_cache(maxsize=None)
def world():
    """The frame (oracle extraction, bit-equal to the device's) and the table.  Everything float32, as the library takes it."""
    from conftest import CONFIGS
    from jetson_slam_amd.synth import synth_stereo_pair
    from oracle import pyoracle as po
    c = CONFIGS[WORLD_CONFIG]
    left, right = synth_stereo_pair(WORLD_SEED, c["h"], c["w"])
    ol = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"])
    orr = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"])
    ol.extract(left)
    orr.extract(right)
    u_right, depth, _ = po.stereo_match(ol, orr, c["bf"] / c["fx"], c["bf"])
    kp = np.array(ol.keypoints())
    N = len(kp) // 6
    x, y, octave = kp[:N].astype(f32), kp[N:2 * N].astype(f32), kp[4 * N:5 * N].astype(np.int64)
    desc = np.array(ol.descriptors()).reshape(N, 32)
    scale = np.array(ol.scales(), f32)[:c["L"]]
    rng = np.random.default_rng(WORLD_SEED)
    ok = np.nonzero(np.asarray(depth) > 0)[0]
    assert len(ok) >= 100
    src = rng.choice(ok, N_ROWS, replace=True)
    fx = fy = f32(c["fx"])
    cx, cy = f32(c["w"] / 2), f32(c["h"] / 2)
    # the current pose, a little off the identity the points are made with
    a = rng.normal(0, 0.002, 3)
    R = np.array([[1, -a[2], a[1]], [a[2], 1, -a[0]], [-a[1], a[0], 1]], f32)
    t = rng.normal(0, 0.01, 3).astype(f32)
    Ow = (-(R.T @ t)).astype(f32)
    z = np.asarray(depth, f32)[src]
    P = np.stack([(x[src] + rng.normal(0, 0.5, N_ROWS).astype(f32) - cx) * z / fx, (y[src] + rng.normal(0, 0.5, N_ROWS).astype(f32) - cy) * z / fy, z]).astype(f32)
    kind = rng.choice(6, N_ROWS, p=[0.6, 0.08, 0.08, 0.08, 0.08, 0.08])      # 0 visible, 1 behind, 2 outside the image, 3 too far, 4 too near, 5 view angle
    P[2, kind == 1] *= f32(-1)
    P[0, kind == 2] += f32(50.0) * np.abs(P[2, kind == 2])
    dist = np.linalg.norm(P - Ow[:, None], axis=0).astype(f32)
    Pn = ((P - Ow[:, None]) / dist).astype(f32)
    Pn[:, kind == 5] *= f32(-1)
    maxd = (dist * scale[octave[src]] * f32(0.999)).astype(f32)          # MapPoint::UpdateNormalAndDepth: PredictScale gives the keypoint's level
    mind = (maxd / scale[-1]).astype(f32)
    D = np.stack([maxd, maxd * f32(1.2), mind * f32(0.8)]).astype(f32)      # MaxDistance, invariance_maxDistance, invariance_minDistance
    D[1, kind == 3] = dist[kind == 3] * f32(0.5)
    D[2, kind == 4] = dist[kind == 4] * f32(2.0)
    d = desc[src].copy()
    flip = rng.random((N_ROWS, 32)) < 0.03
    d[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    bad = (rng.random(N_ROWS) < 0.05).astype(np.uint8)
    return dict(c=c, left=left, right=right, kp=kp, N=N, x=x, y=y, octave=octave, kp_desc=desc, u_right=np.asarray(u_right, f32), depth=np.asarray(depth, f32),
                scale=scale, src=src, kind=kind, floats=np.concatenate([P, Pn, D]).astype(f32), desc=np.ascontiguousarray(d), bad=bad, R=R, t=t, Ow=Ow,
                cam=(float(fx), float(fy), float(cx), float(cy)), bounds=(0, c["w"], 0, c["h"]), n_levels=c["L"], logsf=float(np.log(f32(1.2))), vca=0.5)


def frustum_block(W, rows):
    """the points `rows` of the table as tests/test_tracking_edges.py::k16_restated takes them"""
    F = W["floats"][:, rows]
    return dict(P=F[0:3], Pn=F[3:6], dist=F[6:9], R=W["R"].ravel(), t=W["t"], Ow=W["Ow"], cam=W["cam"], bounds=W["bounds"], logsf=W["logsf"], vca=W["vca"],
                n=len(rows))


# ---------------------------------------------------------------- the cases
# name: (keyframe sizes, frame marks?)  Keyframes hold 0-300 entries except in the chunk-edge cases of the shipped chunk, whose E = 2 * 1024 + 1
# does not fit six keyframes of 300.
CASES = {
    "six": ([300, 211, 64, 1, 129, 77], True),
    "empty_first_middle_last": ([0, 200, 0, 150, 300, 0], True),
    "zero_keyframes": ([], True),
    "only_empty_keyframes": ([0, 0], True),
    "no_frame": ([180, 90, 33], False),
}
for _chunk in CHUNKS:
    for _E in (_chunk - 1, _chunk, _chunk + 1, 2 * _chunk + 1):
        _k = 5 if _chunk > 64 else 2
        _sizes = [_E // _k] * (_k - 1)
        CASES["edge_%d_%d" % (_chunk, _E)] = (_sizes + [_E - sum(_sizes)], True)
EMPTY = ("zero_keyframes", "only_empty_keyframes")


def edge_cases(chunk):
    return [n for n in CASES if n.startswith("edge_%d_" % chunk)]


@functools.lru_cache(maxsize=None)
def build_case(name):
    """dict(keyframes, kf_start, entries, frame_rows, claims): claims = the drop reasons the case must show (checked in tests/test_local_map_host.py)"""
    import zlib
    W = world()
    sizes, with_frame = CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    good = np.nonzero(W["bad"] == 0)[0]
    bad_rows = np.nonzero(W["bad"] != 0)[0]
    kfs = []
    for n in sizes:
        k = rng.choice(good, n, replace=True).astype(np.int64)          # (repeats inside a keyframe and across keyframes occur by themselves, too)
        m = rng.random(n)
        k[m < 0.10] = -1
        k[(m >= 0.10) & (m < 0.13)] = rng.choice([N_ROWS, N_ROWS + 5, 2 ** 31 - 1], int(((m >= 0.10) & (m < 0.13)).sum()))
        k[(m >= 0.13) & (m < 0.15)] = rng.choice([-2, -1000, -2 ** 31], int(((m >= 0.13) & (m < 0.15)).sum()))
        k[(m >= 0.15) & (m < 0.22)] = rng.choice(bad_rows, int(((m >= 0.15) & (m < 0.22)).sum()))
        kfs.append(k)
    full = [i for i, k in enumerate(kfs) if len(k) >= 30]
    claims = ()
    if full:
        visible = good[W["kind"][good] == 0]
        shared, twice, seen_first = (int(r) for r in rng.choice(visible, 3, replace=False))
        for j, i in enumerate((full * 3)[:3]):                           # one row in three keyframes (more than once in one, when there are fewer)
            kfs[i][20 + j] = shared
        kfs[full[0]][[2, 17]] = twice                                    # one row twice in one keyframe
        kfs[full[-1]][5] = N_ROWS                                        # the first row past the table, -1, a row below it, a bad row
        kfs[full[-1]][6], kfs[full[-1]][7], kfs[full[-1]][8] = -1, -2, int(bad_rows[0])
        kfs[full[0]][1] = seen_first                                     # a row the frame has seen, here for the first time ...
        kfs[full[-1]][9] = seen_first                                    # ... and again
        claims = REASONS if with_frame else REASONS[:-1]
    entries = np.concatenate(kfs).astype(np.int64) if kfs else np.zeros(0, np.int64)
    frame_rows = None
    if with_frame:
        N = W["N"]
        frame_rows = np.full(N, -1, np.int64)
        m = rng.random(N)
        pool = entries[(entries >= 0) & (entries < N_ROWS)] if len(entries) else good
        pick = m < (0.25 if len(entries) > 300 else 0.03)                # (a small local map: few keypoints, or the frame has seen all of it)
        frame_rows[pick] = rng.choice(pool if len(pool) else good, int(pick.sum()))      # rows of the local map, the bad ones among them
        frame_rows[(m >= 0.25) & (m < 0.30)] = rng.choice(good, int(((m >= 0.25) & (m < 0.30)).sum()))
        frame_rows[(m >= 0.30) & (m < 0.32)] = rng.choice([N_ROWS, -5, 2 ** 31 - 1], int(((m >= 0.30) & (m < 0.32)).sum()))
        if full:
            frame_rows[0], frame_rows[N - 1] = seen_first, int(bad_rows[0])
            frame_rows[(frame_rows == shared) | (frame_rows == twice)] = -1      # these two stay in the list
    kf_start = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int32)
    return dict(name=name, keyframes=[k.astype(np.int32) for k in kfs], kf_start=kf_start, entries=entries.astype(np.int32),
                frame_rows=None if frame_rows is None else frame_rows.astype(np.int32), claims=claims, shared=shared if full else None,
                twice=twice if full else None, seen_first=seen_first if full else None)


def capacities(n_inside):
    """the capacities every case runs with: one short (overflow, a prefix is kept), exact, one more (a padding slot), none"""
    return sorted({max(n_inside - 1, 0), n_inside, n_inside + 1, 0})


def expected_outputs(rows_inside, k16, desc, capacity):
    """The contract's step 5 from the map_points inside the frustum, in list order: rows_inside their table rows, k16 = (u, v, invz, level, view_cos)
    of them, desc the table's descriptors."""
    n = min(len(rows_inside), capacity)
    out = dict(point_row=np.full(capacity, -1, np.int32), in_frustum=np.zeros(capacity, np.uint8), mp_descriptors=np.zeros((capacity, 32), np.uint8),
               predicted_level=np.zeros(capacity, np.int32))
    for k in ("u", "v", "invz", "view_cos"):
        out[k] = np.zeros(capacity, f32)
    out["point_row"][:n] = rows_inside[:n]
    out["in_frustum"][:n] = 1
    out["mp_descriptors"][:n] = desc[rows_inside[:n]]
    u, v, invz, level, view_cos = k16
    out["u"][:n], out["v"][:n], out["invz"][:n], out["view_cos"][:n], out["predicted_level"][:n] = u[:n], v[:n], invz[:n], view_cos[:n], level[:n]
    return out
