"""The caller's side of jsorb_fuse (include/jsorb.h): the head test and the tail of ORBmatcher::Fuse replayed on a live map over the best_idx /
best_dist a search returned, keyframe by keyframe, as the header describes it - with this project's restatements of MapPoint::AddObservation,
Replace and ComputeDistinctiveDescriptors (MapPoint.cpp:129-140, :208-246, :273-338), the same ones oracle/ref_matcher/harness.cpp puts under the
reference's own ORBmatcher.cpp.  Not a test module and not a conftest: tests/test_ref_matcher.py and tests/test_gpu_ref_matcher.py import it.

A case is a dict of tests/ref_matcher_cases.py's fuse vocabulary: KF (all keyframes of the map; each with x, y, octave, desc, uright, the pose and
mps, its mvpMapPoints as point ids or -1), P (all points: position, normal, distance range, descriptor, bad), obs (the initial observations as
(point, keyframe, keypoint) rows), targets (the keyframes Fuse runs into, in order), list (the ids every call gets, -1: NULL), prm and, for the
overload with Scw, Scw and replace_loop.  What a replay returns has the keys of the reference driver's output (oracle/pyref_matcher.py)."""
import numpy as np

EV_ADD_OBSERVATION, EV_REPLACE, EV_ADD_MAP_POINT, EV_REPLACE_MATCH, EV_ERASE_MATCH, EV_DESCRIPTOR = 1, 2, 3, 4, 5, 6
MODES = ("sequential", "batched", "research")


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


class LiveMap:
    """points, observations and the keyframes' slots; every mutating member appends to `events` as the harness's members do"""

    def __init__(self, case):
        KF, P = case["KF"], case["P"]
        n = len(P["Px"])
        self.stereo = [np.asarray(K["uright"], np.float32) >= 0 for K in KF]
        self.kf_desc = [np.asarray(K["desc"], np.uint8).reshape(-1, 32) for K in KF]
        self.mps = [[int(v) for v in K["mps"]] for K in KF]
        self.bad = [bool(b) for b in P["bad"]]
        self.replaced, self.nobs = [-1] * n, [0] * n
        self.obs = [dict() for _ in range(n)]             # keyframe -> keypoint; walked in ascending keyframe index (the drivers' pointer order)
        self.desc = np.array(P["desc"], np.uint8).reshape(n, 32).copy()
        self.events, self.ev_desc = [], []
        self.logging = False
        for p, k, idx in np.asarray(case["obs"], np.int64).reshape(-1, 3):
            self.add_observation(int(p), int(k), int(idx))
        self.logging = True

    def log(self, *e):
        if self.logging:
            self.events.append(e)

    def add_observation(self, p, k, idx):                 # MapPoint.cpp:129-140
        if k in self.obs[p]:
            return
        self.obs[p][k] = idx
        self.nobs[p] += 2 if self.stereo[k][idx] else 1
        self.log(EV_ADD_OBSERVATION, p, k, idx)

    def replace(self, p, q):                              # p->Replace(q), :208-246
        if p == q:
            return
        self.log(EV_REPLACE, p, q, -1)
        mine, self.obs[p] = self.obs[p], dict()
        self.bad[p], self.replaced[p] = True, q
        for k in sorted(mine):
            if k not in self.obs[q]:
                self.mps[k][mine[k]] = q
                self.log(EV_REPLACE_MATCH, q, k, mine[k])
                self.add_observation(q, k, mine[k])
            else:
                self.mps[k][mine[k]] = -1
                self.log(EV_ERASE_MATCH, -1, k, mine[k])
        self.compute_distinctive_descriptors(q)

    def compute_distinctive_descriptors(self, q):         # :273-338
        if self.bad[q] or not self.obs[q]:
            return
        seen = [(k, self.obs[q][k]) for k in sorted(self.obs[q])]
        d = [self.kf_desc[k][i] for k, i in seen]
        N = len(d)
        dist = [[hamming(d[i], d[j]) for j in range(N)] for i in range(N)]
        best_median, best = 2 ** 31 - 1, 0
        for i in range(N):
            median = sorted(dist[i])[int(0.5 * (N - 1))]
            if median < best_median:
                best_median, best = median, i
        if not np.array_equal(d[best], self.desc[q]):
            self.log(EV_DESCRIPTOR, q, seen[best][0], seen[best][1])
            if self.logging:
                self.ev_desc.append(d[best].copy())
        self.desc[q] = d[best]

    def head_passes(self, p, k):                          # ORBmatcher.cpp:833-837
        return p >= 0 and not self.bad[p] and k not in self.obs[p]

    def tail(self, k, p, best_idx):                       # :941-956
        in_kf = self.mps[k][best_idx]
        if in_kf >= 0:
            if not self.bad[in_kf]:
                if self.nobs[in_kf] > self.nobs[p]:
                    self.replace(p, in_kf)
                else:
                    self.replace(in_kf, p)
        else:
            self.add_observation(p, k, best_idx)
            self.mps[k][best_idx] = p
            self.log(EV_ADD_MAP_POINT, p, k, best_idx)

    def tail_sim3(self, k, p, best_idx):                  # :1071-1081: the point vpReplacePoint gets, or -1
        in_kf = self.mps[k][best_idx]
        if in_kf >= 0:
            return in_kf if not self.bad[in_kf] else -1
        self.add_observation(p, k, best_idx)
        self.mps[k][best_idx] = p
        self.log(EV_ADD_MAP_POINT, p, k, best_idx)
        return -1


def replay(case, search, mode="research"):
    """search(ts, idxs, desc, skip) -> (best_idx, best_dist[, statistics[, probes]]): positions ts in case["targets"], positions idxs in case["list"],
    their descriptors as the map holds them now, skip [len(ts), len(idxs)]; the results have that shape; probes (only the transcription has them)
    is {(t, i): rows}.
    mode "sequential": the reference's order - each keyframe is searched just before it is replayed, from the map as it is then.
    mode "batched": ONE search of all target keyframes from the map as it is before the call, then the replay - what include/jsorb.h described
      before the descriptor question was run (tests/test_ref_matcher.py shows where it differs from the reference).
    mode "research": the batched search, and after the replay of a keyframe every list point that is still good and whose 32 descriptor bytes
      differ from those it was searched with is searched again against the keyframes not yet replayed, where its head test passes - the contract."""
    assert mode in MODES
    m = LiveMap(case)
    targets, lst = [int(k) for k in case["targets"]], [int(p) for p in case["list"]]
    sim3 = case.get("Scw") is not None
    T, n = len(targets), len(lst)
    best = np.full((T, n), -1, np.int64)
    bdist = np.full((T, n), -1, np.int64)
    probes, calls = {}, []
    searched_with = np.zeros((n, 32), np.uint8)
    list_desc = lambda idxs: m.desc[[max(lst[i], 0) for i in idxs]].reshape(len(idxs), 32)

    def found(k):                                          # :980, the live points in the keyframe's slots
        return {p for p in m.mps[k] if p >= 0 and not m.bad[p]}

    def head_now(t, i, already=None):
        if sim3:                                           # :992
            return lst[i] >= 0 and not m.bad[lst[i]] and lst[i] not in (found(targets[t]) if already is None else already)
        return m.head_passes(lst[i], targets[t])

    def run(ts, idxs):
        if not ts or not idxs:
            return
        skip = np.array([[0 if head_now(t, i, al) else 1 for i in idxs] for t, al in ((t, found(targets[t]) if sim3 else None) for t in ts)], np.uint8)
        res = search(ts, idxs, list_desc(idxs), skip)
        best[np.ix_(ts, idxs)], bdist[np.ix_(ts, idxs)] = res[0], res[1]
        searched_with[idxs] = list_desc(idxs)
        if len(res) > 2:
            calls.append(tuple(int(v) for v in res[2]))
        if len(res) > 3:
            probes.update(res[3])

    everything = list(range(n))
    if mode != "sequential":
        run(list(range(T)), everything)
    nfused = np.zeros(T, np.int32)
    replace = np.full((T, n), -1, np.int32)
    probe_log = []
    for t, k in enumerate(targets):
        if mode == "sequential":
            run([t], everything)
        already = found(k) if sim3 else None
        for i, p in enumerate(lst):
            if not head_now(t, i, already):
                continue
            probe_log.extend(probes.get((t, i), []))
            if best[t, i] < 0:
                continue
            if sim3:
                replace[t, i] = m.tail_sim3(k, p, int(best[t, i]))
            else:
                m.tail(k, p, int(best[t, i]))
            nfused[t] += 1
        if sim3 and int(case["replace_loop"]):             # LoopClosing.cpp:609-616
            for i, p in enumerate(lst):
                if replace[t, i] >= 0:
                    m.replace(int(replace[t, i]), p)
        if mode == "research" and t + 1 < T:
            changed = [i for i, p in enumerate(lst) if p >= 0 and not m.bad[p] and not np.array_equal(m.desc[p], searched_with[i])]
            run(list(range(t + 1, T)), changed)
    n_pts = len(m.bad)
    out = dict(nfused=nfused, nmatches=np.int32(nfused.sum()), events=np.array(m.events, np.int32).reshape(-1, 4),
               ev_desc=np.array(m.ev_desc, np.uint8).reshape(-1, 32), kf_mps=np.array([p for s in m.mps for p in s], np.int32),
               pt_bad=np.array(m.bad, np.uint8).reshape(n_pts), pt_replaced=np.array(m.replaced, np.int32).reshape(n_pts),
               pt_nobs=np.array(m.nobs, np.int32).reshape(n_pts), pt_desc=m.desc.copy(), probe=np.array(probe_log, np.float32).reshape(-1, 5))
    if sim3:
        out["replace"] = replace
    return out, calls, (best, bdist)


MAP_KEYS = ("nfused", "events", "ev_desc", "kf_mps", "pt_bad", "pt_replaced", "pt_nobs", "pt_desc")


def same_map(got, want, keys=MAP_KEYS):
    """the replay's events, map and counts are the reference's"""
    for key in keys + (("replace",) if "replace" in want else ()):
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and np.array_equal(a, b), key
