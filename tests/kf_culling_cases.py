"""Worlds and yardsticks for jsorb_cull_keyframes (include/jsorb.h), shared by tests/test_kf_culling_host.py and tests/test_gpu_kf_culling.py.
numpy only: nothing here needs a GPU.  Not a test module.

* run_literal: a literal sequential transcription of LocalMapping::KeyFrameCulling (LocalMapping.cpp:638-702), KeyFrame::SetBadFlag
  (KeyFrame.cpp:457-549, with EraseConnection / UpdateBestCovisibles) and MapPoint::EraseObservation / SetBadFlag (MapPoint.cpp:142-168,
  :182-199) over KeyFrame / MapPoint objects with real mObservations maps (dicts iterated in key order) and a STORED nObs.  The stated
  differences of the contract are in it and marked: an unusable or bad candidate is skipped, the children are read from parent[] (no EraseChild),
  a missing parent is an empty candidate set.
* run_restated: the contract over the arrays, with Observations() recomputed from the observations.  `mutant` breaks it in one named way; each
  mutant must fail a named case.
* a world: the graph's arrays (state, order_key, point runs, registered, parent), the table's bad bytes, the views (octave, stereo, depth or
  None, th_depth), the covisibility state with the neighbours table, not_erase / to_be_erased / ref_slot (or None), and the call's arguments
  (monocular, first_slot, cand, max_cull, cap).  A result: every array the call writes and every output."""
import numpy as np

import covis_cases as cc

COUNTS = ("next", "n_kept", "n_culled", "n_deferred", "n_skipped", "n_rows_bad", "n_observations_erased", "n_ref_moved", "n_reparent",
          "reparent_overflow")
KEPT, CULLED, DEFERRED, SKIPPED, NOT_REACHED = 0, 1, 2, 3, -1
MAX_CULL = 16
WRITTEN = ("state", "registered", "point_pool", "parent")       # of the graph
OUTPUTS = ("decision", "n_mps", "n_redundant", "culled_slot", "reparent_out", "counts")
MUTANTS = {                                      # name -> the case it must fail
    "ratio_at_least": "nine_of_ten_ten_of_ten_and_none",
    "th_obs_2": "observations_3_4_and_two_stereo_observers",
    "octave_plus_2": "q_2_3_and_the_octave_bound",
    "candidate_counts_in_q": "q_2_3_and_the_octave_bound",
    "stale_state": "a_cull_takes_the_third_observer_away",
    "stereo_erased_as_one": "a_stereo_observation_erased_crosses_two",
    "ref_highest_key": "ref_slot_moves_to_the_lowest_key_then_slot",
    "tree_at_least": "tree_tie_takes_the_first_pair",
}


def copy_world_arrays(W):
    G = {k: (None if v is None else v.copy()) for k, v in W["G"].items()}
    opt = lambda k: None if W[k] is None else W[k].copy()
    return G, W["bad"].copy(), cc.copy_state(W["cov"]), opt("to_be_erased"), opt("ref_slot")


def _result(G, bad, cov, tbe, ref, out):
    res = {k: G[k].copy() for k in WRITTEN}
    res.update(bad=bad.copy(), cov=cc.normalised(cov), to_be_erased=tbe, ref_slot=ref)
    res.update(out)
    return res


def _outputs(W):
    n = len(W["cand"])
    return dict(decision=np.full(n, NOT_REACHED, np.int32), n_mps=np.zeros(n, np.int32), n_redundant=np.zeros(n, np.int32),
                culled_slot=np.full(W["max_cull"], -1, np.int32), reparent_out=np.full((W["cap"], 2), -1, np.int32), counts=np.zeros(10, np.int32))


def _log(out, W, child, parent):
    n = int(out["counts"][8])
    if n < W["cap"]:
        out["reparent_out"][n] = (child, parent)
    else:
        out["counts"][9] = 1
    out["counts"][8] = n + 1


def _depth_drops(W, A, e):
    """LocalMapping.cpp:666 in float, literally"""
    d, th = np.float32(W["views"]["depth"][e]), np.float32(W["views"]["th_depth"][A])
    return bool(d > th or d < np.float32(0))


# ---------------------------------------------------------------- the reference's functions, literally
class MapPoint:
    def __init__(self, row, bad):
        self.row, self.mbBad, self.mObservations, self.nObs, self.mpRefKF = row, bool(bad), {}, 0, None
        self.ref_raw = -1                        # what ref_slot held where it names no observer object the literal form would follow

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def GetObservations(self):                   # std::map<KeyFrame*, size_t>
        return sorted(self.mObservations.items(), key=lambda kv: kv[0].order())

    def AddObservation(self, pKF, idx):          # :129-140
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx
        self.nObs += 2 if pKF.mvuRight[idx] >= 0 else 1

    def EraseObservation(self, pKF, tally):      # :142-168
        bBad = False
        if pKF in self.mObservations:
            idx = self.mObservations[pKF]
            self.nObs -= 2 if pKF.mvuRight[idx] >= 0 else 1
            del self.mObservations[pKF]
            tally["n_observations_erased"] += 1
            if self.mpRefKF is pKF:
                obs = self.GetObservations()
                self.mpRefKF = obs[0][0] if obs else None      # (begin() of an empty map is undefined in the reference: -1 here)
                self.ref_raw = -1
                tally["n_ref_moved"] += 1
            if self.nObs <= 2:
                bBad = True
        if bBad:
            self.SetBadFlag(tally)

    def SetBadFlag(self, tally):                 # :182-199
        self.mbBad = True
        obs, self.mObservations = self.mObservations, {}
        for pKF, idx in obs.items():
            pKF.EraseMapPointMatch(idx)
        tally["n_rows_bad"] += 1


class KeyFrame:
    def __init__(self, slot, key, mnId):
        self.slot, self.key, self.mnId = slot, int(key), mnId
        self.mvpMapPoints, self.octave, self.mvuRight, self.mvDepth, self.mThDepth = [], [], [], [], 0.0
        self.erased = []                         # the indices EraseMapPointMatch set to NULL
        self.mConnectedKeyFrameWeights, self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = {}, [], []
        self.mbBad = self.mbNotErase = self.mbToBeErased = False
        self.parent_slot, self.list_written = -1, False

    def order(self):
        return (self.key, self.slot)

    def isBad(self):
        return self.mbBad

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None
        self.erased.append(idx)

    def items_in_key_order(self):
        return sorted(self.mConnectedKeyFrameWeights.items(), key=lambda kv: kv[0].order())

    def GetWeight(self, pKF):                    # KeyFrame.cpp:205-212
        return self.mConnectedKeyFrameWeights.get(pKF, 0)

    def UpdateBestCovisibles(self):              # :142-161
        vPairs = sorted(((w, kf) for kf, w in self.items_in_key_order()), key=lambda p: (p[0], p[1].order()))
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [kf for _, kf in reversed(vPairs)], [w for w, _ in reversed(vPairs)]
        self.list_written = True

    def EraseConnection(self, pKF):              # :557-571
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            self.UpdateBestCovisibles()

    def SetBadFlag(self, kfs, W, out, tally):    # :457-549
        if self.mnId == 0:
            return KEPT
        if self.mbNotErase:
            self.mbToBeErased = True
            return DEFERRED
        for kf, _ in self.items_in_key_order():  # :470-471
            if kf is not self:
                kf.EraseConnection(self)
        for pMP in list(self.mvpMapPoints):      # :473-475
            if pMP is not None:
                pMP.EraseObservation(self, tally)
        self.mConnectedKeyFrameWeights, self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = {}, [], []      # :480-481
        self.list_written = True
        # :483-541.  Stated differences: mspChildrens is every keyframe whose parent is this one (state != 0; a keyframe culled earlier has not
        # been erased from it, there is no EraseChild), and a parent that is no usable slot gives an empty candidate set
        children = sorted((kf for kf in kfs.values() if kf.present and kf.parent_slot == self.slot and kf is not self), key=KeyFrame.order)
        mpParent = kfs.get(self.parent_slot)
        sParentCandidates = [mpParent] if mpParent is not None and mpParent.present and mpParent is not self else []
        while children:
            bContinue, mx, pC, pP = False, -1, None, None
            for pKF in children:
                if pKF.isBad():
                    continue
                for con in pKF.mvpOrderedConnectedKeyFrames:
                    for cand in sParentCandidates:
                        if con.mnId == cand.mnId:
                            w = pKF.GetWeight(con)
                            if w > mx:
                                pC, pP, mx, bContinue = pKF, con, w, True
            if not bContinue:
                break
            pC.parent_slot = pP.slot             # ChangeParent
            _log(out, W, pC.slot, pP.slot)
            sParentCandidates.append(pC)
            children.remove(pC)
        for kf in children:                      # :535-539
            kf.parent_slot = self.parent_slot
            _log(out, W, kf.slot, self.parent_slot)
        self.mbBad = True
        return CULLED


def _objects(W):
    G, bad, V = W["G"], W["bad"], W["views"]
    S = len(G["state"])
    kfs = {s: KeyFrame(s, G["order_key"][s], 0 if s == W["first_slot"] else s + 1) for s in range(S)}
    points = [MapPoint(r, b) for r, b in enumerate(bad)]
    for s, kf in kfs.items():
        kf.present, kf.mbBad = G["state"][s] != 0, G["state"][s] not in (0, 1)
        kf.valid = cc.valid_run(G, s)
        kf.parent_slot = int(G["parent"][s])
        kf.mbNotErase = W["not_erase"] is not None and bool(W["not_erase"][s])
        kf.mbToBeErased = W["to_be_erased"] is not None and bool(W["to_be_erased"][s])
        kf.mThDepth = V["th_depth"][s]
        if not (kf.present and kf.valid):
            continue
        off = int(G["point_off"][s])
        for j, r in enumerate(cc.run_of(G, s)):
            e = off + j
            ok = 0 <= r < len(bad)
            kf.mvpMapPoints.append(points[r] if ok else None)
            kf.octave.append(int(V["octave"][e]))
            kf.mvuRight.append(1.0 if V["stereo"][e] else -1.0)
            kf.mvDepth.append(e)                 # the entry: the depth gate reads the float through it
            if ok and not bad[r] and G["state"][s] == 1 and G["registered"][e]:
                points[r].AddObservation(kf, j)
    for r, p in enumerate(points):
        if W["ref_slot"] is not None:
            p.ref_raw = int(W["ref_slot"][r])
            p.mpRefKF = kfs.get(p.ref_raw)
    cov = W["cov"]
    for s, kf in kfs.items():
        for j in range(int(cov["conn_len"][s])):
            kf.mConnectedKeyFrameWeights[kfs[int(cov["conn_slot"][s, j])]] = int(cov["conn_weight"][s, j])
        for j in range(int(cov["ord_len"][s])):
            kf.mvpOrderedConnectedKeyFrames.append(kfs[int(cov["ord_slot"][s, j])])
            kf.mvOrderedWeights.append(int(cov["ord_weight"][s, j]))
    return kfs, points


def run_literal(W):
    G, bad, cov, tbe, ref = copy_world_arrays(W)
    kfs, points = _objects(W)
    out = _outputs(W)
    tally = dict.fromkeys(COUNTS, 0)
    seen, n_culled, nxt = set(), 0, len(W["cand"])
    for i, A in enumerate(W["cand"]):            # :646
        A = int(A)
        pKF = kfs.get(A)
        # the contract's skips (the reference would read through the pointer); mnId == 0 is :649
        if pKF is None or not pKF.present or G["state"][A] != 1 or pKF.mbBad or not pKF.valid or A in seen or pKF.mnId == 0:
            out["decision"][i] = SKIPPED
            continue
        seen.add(A)
        thObs, nRedundantObservations, nMPs = 3, 0, 0
        for idx, pMP in enumerate(pKF.mvpMapPoints):
            if pMP is None or pMP.isBad():
                continue
            if not W["monocular"] and _depth_drops(W, A, pKF.mvDepth[idx]):
                continue
            nMPs += 1
            if pMP.Observations() > thObs:
                scaleLevel, nObs = pKF.octave[idx], 0
                for pKFi, idx_i in pMP.GetObservations():
                    if pKFi is pKF:
                        continue
                    if pKFi.octave[idx_i] <= scaleLevel + 1:
                        nObs += 1
                        if nObs >= thObs:
                            break
                if nObs >= thObs:
                    nRedundantObservations += 1
        out["n_mps"][i], out["n_redundant"][i] = nMPs, nRedundantObservations
        d = KEPT
        if nRedundantObservations > 0.9 * nMPs:  # :699
            d = pKF.SetBadFlag(kfs, W, out, tally)
        out["decision"][i] = d
        if d == CULLED:
            out["culled_slot"][n_culled] = A
            n_culled += 1
            if n_culled == W["max_cull"]:
                nxt = i + 1
                break
    # the objects back into the arrays
    for s, kf in kfs.items():
        if kf.mbBad and G["state"][s] == 1:
            G["state"][s] = 2
        G["parent"][s] = kf.parent_slot
        if tbe is not None and kf.mbToBeErased:
            tbe[s] = 1
        if not (kf.present and kf.valid):
            continue
        off = int(G["point_off"][s])
        for j in kf.erased:
            G["point_pool"][off + j] = -1
        for j, r in enumerate(cc.run_of(W["G"], s)):
            e = off + j
            was = 0 <= r < len(bad) and not W["bad"][r] and W["G"]["state"][s] == 1 and W["G"]["registered"][e]
            if was and points[r].mObservations.get(kf) != j:
                G["registered"][e] = 0
    for r, p in enumerate(points):
        bad[r] = p.mbBad
        if ref is not None:
            ref[r] = p.ref_raw if p.mpRefKF is None else p.mpRefKF.slot
        # the stated equality: the stored nObs is the sum over the observations wherever AddObservation / EraseObservation reach
        assert p.mbBad or p.nObs == sum(2 if kf.mvuRight[idx] >= 0 else 1 for kf, idx in p.mObservations.items())
    width = max([W["C"]] + [len(kf.mConnectedKeyFrameWeights) for kf in kfs.values()])
    assert width == W["C"]                       # (culling only shrinks the maps)
    for s, kf in kfs.items():
        if kf.list_written:
            items = [(o.slot, w) for o, w in kf.items_in_key_order()]
            cc._write(cov, s, items, list(zip((o.slot for o in kf.mvpOrderedConnectedKeyFrames), kf.mvOrderedWeights)))
    d = out["decision"]
    out["counts"][:8] = [nxt, (d == KEPT).sum(), (d == CULLED).sum(), (d == DEFERRED).sum(), (d == SKIPPED).sum(), tally["n_rows_bad"],
                         tally["n_observations_erased"], tally["n_ref_moved"]]
    return _result(G, bad, cov, tbe, ref, out)


# ---------------------------------------------------------------- the contract over the arrays
def run_restated(W, mutant=None):
    G, bad, cov, tbe, ref = copy_world_arrays(W)
    V, cand, out = W["views"], [int(a) for a in W["cand"]], _outputs(W)
    S, n_rows, entries = len(G["state"]), len(bad), len(G["point_pool"])
    state, reg, pool, parent, key = G["state"], G["registered"], G["point_pool"], G["parent"], G["order_key"]
    run = lambda s: range(int(G["point_off"][s]), int(G["point_off"][s]) + int(G["point_len"][s]))
    order = lambda s: (int(key[s]), int(s))
    lists = {}                                   # the observations grouped by row once; every use checks the current state
    for B in range(S):
        if state[B] == 1 and cc.valid_run(G, B):
            for e in run(B):
                r = int(pool[e])
                if 0 <= r < n_rows and not bad[r] and reg[e]:
                    lists.setdefault(r, []).append((B, e))

    def observations(r):
        return [(B, e) for B, e in lists.get(r, ()) if state[B] == 1 and reg[e] and pool[e] == r]

    def n_obs(obs):
        return sum(1 + (V["stereo"][e] != 0) for _, e in obs)

    def evaluate(A):
        th_obs = 2 if mutant == "th_obs_2" else 3
        n_mps = n_red = 0
        for e in run(A):
            r = int(pool[e])
            if not 0 <= r < n_rows or bad[r]:
                continue
            if not W["monocular"] and _depth_drops(W, A, e):
                continue
            n_mps += 1
            obs = observations(r)
            if n_obs(obs) > th_obs:
                bound = int(V["octave"][e]) + (2 if mutant == "octave_plus_2" else 1)
                q = sum((B != A or mutant == "candidate_counts_in_q") and int(V["octave"][e2]) <= bound for B, e2 in obs)
                n_red += q >= th_obs
        # 0.9 * n_mps in double, as the reference writes it; equal to 10 * n_red > 9 * n_mps for every n_mps < 2^31
        cull = float(n_red) >= 0.9 * float(n_mps) if mutant == "ratio_at_least" else float(n_red) > 0.9 * float(n_mps)
        assert mutant is not None or cull == (10 * n_red > 9 * n_mps)
        return n_mps, n_red, cull

    def skipped(i, A):
        return not (0 <= A < S) or state[A] != 1 or not cc.valid_run(G, A) or A == W["first_slot"] or A in cand[:i]

    stale = {i: evaluate(A) for i, A in enumerate(cand) if not skipped(i, A)} if mutant == "stale_state" else None
    n_culled, nxt = 0, len(cand)
    for i, A in enumerate(cand):
        if skipped(i, A):
            out["decision"][i] = SKIPPED
            continue
        n_mps, n_red, cull = stale[i] if stale is not None else evaluate(A)
        out["n_mps"][i], out["n_redundant"][i] = n_mps, n_red
        if not cull:
            out["decision"][i] = KEPT
            continue
        if W["not_erase"] is not None and W["not_erase"][A]:
            out["decision"][i] = DEFERRED
            tbe[A] = 1
            continue
        out["decision"][i] = CULLED
        out["culled_slot"][n_culled] = A
        n_culled += 1
        cc.erase_restated(dict(G=G), cov, A)     # step 6
        mine = [e for e in run(A) if 0 <= pool[e] < n_rows and not bad[pool[e]] and reg[e]]      # step 7: the entries first, then each row once
        for e in mine:
            reg[e] = 0
        out["counts"][6] += len(mine)
        for r in sorted({int(pool[e]) for e in mine}):
            obs = observations(r)
            if ref is not None and ref[r] == A:
                pick = max if mutant == "ref_highest_key" else min
                ref[r] = pick((B for B, _ in obs), key=order) if obs else -1
                out["counts"][7] += 1
            left = n_obs(obs)
            if mutant == "stereo_erased_as_one":
                left += sum(int(V["stereo"][e] != 0) for e in mine if pool[e] == r)
            if left <= 2:
                bad[r] = 1
                out["counts"][5] += 1
                for _, e2 in obs:
                    pool[e2], reg[e2] = -1, 0
        state[A] = 2                             # step 8
        par = int(parent[A])                     # step 9
        ch = sorted((s for s in range(S) if s != A and parent[s] == A and state[s] != 0), key=order)
        P = {par} if 0 <= par < S and state[par] != 0 and par != A else set()
        while ch:
            best = None
            for c in ch:
                if state[c] != 1:
                    continue
                conn = dict(cc._stored(cov, c, S))
                for j in range(min(max(int(cov["ord_len"][c]), 0), W["C"])):
                    p = int(cov["ord_slot"][c, j])
                    if p in P:
                        w = conn.get(p, 0)
                        if best is None and w > -1 or best is not None and (w >= best[0] if mutant == "tree_at_least" else w > best[0]):
                            best = (w, c, p)
            if best is None:
                break
            _, c, p = best
            parent[c] = p
            _log(out, W, c, p)
            P.add(c)
            ch.remove(c)
        for c in ch:
            parent[c] = par
            _log(out, W, c, par)
        if n_culled == W["max_cull"]:            # step 10
            nxt = i + 1
            break
    d = out["decision"]
    out["counts"][:5] = [nxt, (d == KEPT).sum(), (d == CULLED).sum(), (d == DEFERRED).sum(), (d == SKIPPED).sum()]
    return _result(G, bad, cov, tbe, ref, out)


def same(a, b, what=""):
    for k in a:
        if k == "cov":
            for kk in a[k]:
                assert np.array_equal(a[k][kk], b[k][kk]), (what, "cov", kk, np.argwhere(a[k][kk] != b[k][kk])[:4].tolist())
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k, np.asarray(a[k]).ravel()[:24].tolist(), np.asarray(b[k]).ravel()[:24].tolist())


def continued(W, run, max_cull):
    """the call with `max_cull`, repeated on what it left until next == n_cand; the outputs joined"""
    W = dict(W, max_cull=max_cull)
    total, done, culled, recs, tail = None, 0, [], [], np.zeros(9, np.int64)
    while True:
        res = run(W)
        nxt = int(res["counts"][0])
        if total is None:
            total = {k: res[k].copy() for k in ("decision", "n_mps", "n_redundant")}
        for k in ("decision", "n_mps", "n_redundant"):
            total[k][done:done + nxt] = res[k][:nxt]
        culled += [int(s) for s in res["culled_slot"] if s >= 0]
        recs += [tuple(x) for x in res["reparent_out"][:int(res["counts"][8])].tolist()]
        tail += res["counts"][1:]
        done += nxt
        if done >= len(total["decision"]):
            break
        G = dict(W["G"], **{k: res[k] for k in WRITTEN})
        W = dict(W, G=G, bad=res["bad"], cov=res["cov"], to_be_erased=res["to_be_erased"], ref_slot=res["ref_slot"], cand=W["cand"][nxt:])
    return res, total, culled, recs, tail


# ---------------------------------------------------------------- worlds
class Maker:
    """a world put together keyframe by keyframe; keys ascend with the slot unless given"""

    def __init__(self, S=12, n_rows=64, C=16, depth=False, ref=False):
        self.S, self.n_rows, self.C = S, n_rows, C
        self.runs, self.links, self.ord_only = {}, {}, {}
        self.state, self.key, self.parent = np.zeros(S, np.uint8), 1000 + 8 * np.arange(S, dtype=np.int64), np.full(S, -1, np.int32)
        self.bad, self.th = np.zeros(n_rows, np.uint8), np.full(S, 40.0, np.float32)
        self.not_erase, self.depth = None, depth
        self.ref = np.full(n_rows, -1, np.int32) if ref else None
        self.bad_run = set()

    def kf(self, slot, rows, octave=0, stereo=0, depth=1.0, registered=1, key=None, state=1, parent=None):
        n = len(rows)
        parent = (0 if slot else -1) if parent is None else parent       # (the reference reads through mpParent: slot 0 unless a case says otherwise)
        b = lambda v, dt: np.broadcast_to(np.asarray(v, dt), (n,)).copy()
        self.runs[slot] = (np.asarray(rows, np.int32), b(octave, np.uint8), b(stereo, np.uint8), b(depth, np.float32), b(registered, np.uint8))
        self.state[slot], self.parent[slot] = state, parent
        if key is not None:
            self.key[slot] = key
        return self

    def link(self, a, b, w, both=True, conn=True):
        """b in a's map and list with weight w (and a in b's); conn=False: in the list only"""
        (self.links if conn else self.ord_only).setdefault(a, {})[b] = w
        if both:
            self.link(b, a, w, both=False, conn=conn)
        return self

    def world(self, name, cand, first_slot=0, monocular=True, max_cull=MAX_CULL, cap=32):
        S = self.S
        off, ln = np.zeros(S, np.int32), np.zeros(S, np.int32)
        pool, octv, ster, dep, reg = [], [], [], [], []
        for s in sorted(self.runs):
            rows, o, st, d, rg = self.runs[s]
            off[s], ln[s] = len(pool), len(rows)
            pool += rows.tolist(); octv += o.tolist(); ster += st.tolist(); dep += d.tolist(); reg += rg.tolist()
        pool += [-1] * 3                         # (entries behind the last run)
        n = len(pool)
        pad = lambda v, dt: np.array(list(v) + [0] * (n - len(v)), dt)
        for s in self.bad_run:
            off[s], ln[s] = n - 1, 5
        G = dict(state=self.state.copy(), order_key=self.key.copy(), point_off=off, point_len=ln, point_pool=np.array(pool, np.int32),
                 registered=pad(reg, np.uint8), parent=self.parent.copy())
        cov = cc.empty_state(S, self.C)
        for s in range(S):
            conn = sorted(self.links.get(s, {}).items(), key=lambda it: cc._key(G, it[0]))
            both = {**self.links.get(s, {}), **self.ord_only.get(s, {})}
            cc._write(cov, s, conn, cc._ord_sorted(G, list(both.items())))
        cov["neighbours"][:] = cc.UNTOUCHED
        tbe = None if self.not_erase is None else np.zeros(S, np.uint8)
        return dict(name=name, G=G, bad=self.bad.copy(), views=dict(octave=pad(octv, np.uint8), stereo=pad(ster, np.uint8),
                    depth=pad(dep, np.float32) if self.depth else None, th_depth=self.th.copy()), C=self.C, cov=cov, not_erase=self.not_erase,
                    to_be_erased=tbe, ref_slot=self.ref, monocular=bool(monocular), first_slot=first_slot, cand=np.array(cand, np.int32),
                    max_cull=max_cull, cap=cap)


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _observers(m, rows, slots=(8, 9, 10), **kw):
    """three keyframes that observe `rows`: with a fourth observer every one of these rows has Observations 4 and q 3"""
    for s in slots:
        m.kf(s, rows, **kw)
    return m


@case
def observations_3_4_and_two_stereo_observers():
    m = Maker().kf(0, [])
    m.kf(1, [0, 1, 2], stereo=[0, 0, 1])                        # row 0: 3 observations; row 1: 4; row 2: 4 made of two stereo observers, q = 1
    m.kf(8, [0, 1]).kf(9, [0, 1]).kf(10, [1]).kf(11, [2], stereo=1)
    return m.world("observations_3_4", [1]), dict(decision=[KEPT], n_mps=[3], n_redundant=[1])


@case
def q_2_3_and_the_octave_bound():
    m = Maker().kf(0, [])
    m.kf(1, [0, 1, 2, 3], octave=2)
    m.kf(8, [0, 1, 2, 3], octave=[2, 2, 3, 3]).kf(9, [0, 1, 2, 3], octave=[0, 2, 3, 3]).kf(10, [0, 1, 2, 3], octave=[4, 2, 3, 4])
    # row 0: 4 observations, q = 2 (one observer at octave + 2); row 1: q = 3; row 2: all at octave + 1, q = 3; row 3: one at octave + 2, q = 2
    return m.world("q_2_3", [1]), dict(decision=[KEPT], n_mps=[4], n_redundant=[2])


@case
def an_unregistered_entry_still_counts_in_n_mps():
    m = Maker().kf(0, [])
    m.kf(1, [0], registered=0)
    _observers(m, [0], slots=(8, 9, 10, 11))
    return m.world("unregistered", [1]), dict(decision=[CULLED], n_mps=[1], n_redundant=[1], counts={6: 0, 5: 0})


@case
def nine_of_ten_ten_of_ten_and_none():
    m = Maker(n_rows=64).kf(0, [])
    m.kf(1, list(range(10)))                     # row 9: the others sit at octave 7, q = 0
    m.kf(2, [-1, 70, 40])                        # NULL, out of range, a bad row: n_mps = 0
    m.bad[40] = 1
    m.kf(3, list(range(10, 20)))
    _observers(m, list(range(20)), octave=[0] * 9 + [7] + [0] * 10)
    return m.world("nine_of_ten", [1, 2, 3]), dict(decision=[KEPT, KEPT, CULLED], n_mps=[10, 0, 10], n_redundant=[9, 0, 10])


def _depth_world(monocular):
    m = Maker(depth=not monocular).kf(0, [])
    th = np.float32(40.0)
    m.kf(1, list(range(6)), depth=[th, np.nextafter(th, np.float32(np.inf)), -1.0, -0.0, np.nan, 3.0])
    _observers(m, list(range(6)))
    return m.world("depth", [1], monocular=monocular)


@case
def the_depth_gate_at_its_edges():
    return _depth_world(False), dict(decision=[CULLED], n_mps=[4], n_redundant=[4])


@case
def the_depth_gate_is_ignored_when_monocular():
    return _depth_world(True), dict(decision=[CULLED], n_mps=[6], n_redundant=[6])


@case
def a_cull_takes_the_third_observer_away():
    m = Maker().kf(0, [])
    rows = list(range(12))
    m.kf(1, rows).kf(2, rows).kf(8, rows).kf(9, rows)           # 4 observations each: 1 goes, and 2 is left with 3 - kept, though it was redundant
    return m.world("third_observer", [1, 2]), dict(decision=[CULLED, KEPT], n_mps=[12, 12], n_redundant=[12, 0], counts={6: 12, 5: 0})


@case
def a_cull_turns_rows_bad_and_pushes_the_next_over():
    m = Maker(n_rows=64).kf(0, [])
    m.kf(1, [8, 9] + list(range(20, 50)))        # 30 of 32 redundant: culled; rows 8 and 9 are left with 2 observations and turn bad
    m.kf(2, list(range(10)))                     # 8 of 10 before, 8 of 8 after
    m.kf(8, list(range(50))).kf(9, list(range(8)) + list(range(20, 50))).kf(10, list(range(8)) + list(range(20, 50)))
    return m.world("rows_turn_bad", [1, 2]), dict(decision=[CULLED, CULLED], n_mps=[32, 8], n_redundant=[30, 8], counts={5: 2}, bad_rows=[8, 9],
                                                  nulled=[(2, 8), (2, 9), (8, 8), (8, 9)])


@case
def a_stereo_observation_erased_crosses_two():
    m = Maker(n_rows=64).kf(0, [])
    m.kf(1, [30] + list(range(10)), stereo=[1] + [0] * 10)      # row 30: 2 + 1 + 1 = 4 observations, q = 2; erased as 2 it falls to 2 and turns bad
    m.kf(8, [30] + list(range(10))).kf(9, [30] + list(range(10))).kf(10, list(range(10)))
    return m.world("stereo_erased", [1]), dict(decision=[CULLED], n_mps=[11], n_redundant=[10], counts={5: 1, 6: 11}, bad_rows=[30])


@case
def not_erase_defers_and_the_next_still_sees_it():
    m = Maker().kf(0, [])
    rows = list(range(10))
    m.kf(1, rows).kf(2, rows).kf(8, rows).kf(9, rows)
    m.not_erase = np.zeros(m.S, np.uint8)
    m.not_erase[1] = 1
    return m.world("not_erase", [1, 2]), dict(decision=[DEFERRED, CULLED], n_mps=[10, 10], n_redundant=[10, 10], counts={3: 1, 6: 10}, to_be_erased=[1],
                                              untouched=[1])


@case
def skipped_candidates():
    m = Maker().kf(0, list(range(10)))
    m.kf(1, list(range(10))).kf(6, list(range(10))).kf(5, list(range(10)), state=2)
    m.bad_run.add(6)
    _observers(m, list(range(10)))
    # the first keyframe, padding, a slot twice, an absent slot, an invalid run, a bad keyframe, out of range
    return m.world("skips", [0, -1, 1, 1, 7, 6, 5, 99]), dict(decision=[SKIPPED, SKIPPED, CULLED] + [SKIPPED] * 5, counts={4: 7, 0: 8})


@case
def ref_slot_moves_to_the_lowest_key_then_slot():
    m = Maker(ref=True).kf(0, [])
    rows = list(range(10))
    m.kf(1, rows + [20])
    m.kf(8, rows, key=5000).kf(9, rows, key=3000).kf(10, rows, key=3000).kf(11, rows, key=4000)      # equal keys: the lower slot
    m.ref[:5] = 1
    m.ref[5:10] = 8
    m.ref[20] = 1                                # no observer is left: -1, and the row turns bad
    return m.world("ref_slot", [1]), dict(decision=[CULLED], counts={7: 6, 5: 1}, ref={0: 9, 4: 9, 5: 8, 20: -1})


def _tree(links, parent_of_a=2, bad_children=(), n_children=3, ord_only=()):
    """slot 1 is culled; its children are slots 4, 5, 6 (keys ascending), its parent slot 2"""
    m = Maker().kf(0, [])
    rows = list(range(10))
    m.kf(1, rows, parent=parent_of_a).kf(2, [], parent=0)
    for c in range(4, 4 + n_children):
        m.kf(c, [], parent=1, state=2 if c in bad_children else 1)
    _observers(m, rows)
    for a, b, w in links:
        m.link(a, b, w)
    for a, b, w in ord_only:
        m.link(a, b, w, both=False, conn=False)
    return m


@case
def tree_weight_maximum():
    m = _tree([(4, 2, 5), (5, 2, 9), (4, 5, 7), (6, 4, 3), (1, 4, 2)])
    return m.world("tree_max", [1]), dict(decision=[CULLED], reparent=[(5, 2), (4, 5), (6, 4)])


@case
def tree_tie_takes_the_first_pair():
    m = _tree([(4, 2, 5), (5, 2, 5), (6, 2, 5)])
    return m.world("tree_tie", [1]), dict(decision=[CULLED], reparent=[(4, 2), (5, 2), (6, 2)])


@case
def tree_chain_through_a_reparented_child():
    m = _tree([(6, 2, 4), (5, 6, 1), (4, 5, 8)])
    return m.world("tree_chain", [1]), dict(decision=[CULLED], reparent=[(6, 2), (5, 6), (4, 5)])


@case
def tree_fallback_and_a_bad_child():
    # 5 is bad: skipped in the walk although it is linked to the parent, handed to the original parent; 6 has no link at all
    m = _tree([(4, 2, 3), (5, 2, 9), (5, 4, 9)], bad_children=(5,))
    return m.world("tree_fallback", [1]), dict(decision=[CULLED], reparent=[(4, 2), (5, 2), (6, 2)], parents={5: 2, 6: 2})


@case
def tree_without_a_parent():
    m = _tree([(4, 5, 3)], parent_of_a=-1)
    return m.world("tree_no_parent", [1]), dict(decision=[CULLED], reparent=[(4, -1), (5, -1), (6, -1)])


@case
def tree_listed_but_not_in_the_map():
    # 4 lists the parent without holding it in its map: weight 0, which still beats -1, so 4 becomes a candidate and 5 can take it
    m = _tree([(5, 4, 6)], ord_only=[(4, 2, 0)], n_children=2)
    return m.world("tree_ord_only", [1]), dict(decision=[CULLED], reparent=[(4, 2), (5, 4)])


@case
def max_cull_stops_the_call():
    m = Maker().kf(0, [])
    for s in (1, 2, 3):
        m.kf(s, list(range(10 * s, 10 * s + 10)))
    _observers(m, list(range(10, 40)))
    return m.world("max_cull", [1, 2, 3], max_cull=2), dict(decision=[CULLED, CULLED, NOT_REACHED], counts={0: 2, 2: 2}, culled=[1, 2])


@case
def reparent_log_overflows():
    m = _tree([(4, 2, 5), (5, 2, 5), (6, 2, 5)])
    return m.world("log_overflow", [1], cap=2), dict(decision=[CULLED], reparent=[(4, 2), (5, 2)], counts={8: 3, 9: 1}, parents={6: 2})


@case
def a_run_longer_than_a_workgroup():
    m = Maker(n_rows=700).kf(0, [])
    rows = list(range(600))
    m.kf(1, rows)
    _observers(m, rows)
    return m.world("long_run", [1]), dict(decision=[CULLED], n_mps=[600], n_redundant=[600], counts={6: 600})


def build_case(name):
    world, expect = CASES[name]()
    world["name"] = name
    return world, expect


def check_expect(res, expect, world=None):
    for k in ("decision", "n_mps", "n_redundant"):
        if k in expect:
            assert res[k].tolist() == expect[k], (k, res[k].tolist())
    for i, v in expect.get("counts", {}).items():
        assert res["counts"][i] == v, (COUNTS[i], res["counts"].tolist())
    if "reparent" in expect:
        n = min(int(res["counts"][8]), len(res["reparent_out"]))
        assert [tuple(x) for x in res["reparent_out"][:n].tolist()] == expect["reparent"], res["reparent_out"][:n].tolist()
        for c, p in expect["reparent"]:
            assert res["parent"][c] == p
    for c, p in expect.get("parents", {}).items():
        assert res["parent"][c] == p, (c, res["parent"].tolist())
    for r in expect.get("bad_rows", ()):
        assert res["bad"][r] == 1, r
    if "bad_rows" in expect:
        assert int(res["bad"].sum()) == len(expect["bad_rows"]) + expect.get("bad_before", 0)
    for r, s in expect.get("ref", {}).items():
        assert res["ref_slot"][r] == s, (r, res["ref_slot"].tolist())
    if "to_be_erased" in expect:
        assert np.nonzero(res["to_be_erased"])[0].tolist() == expect["to_be_erased"]
    if "culled" in expect:
        assert [int(s) for s in res["culled_slot"] if s >= 0] == expect["culled"]
    for s in expect.get("untouched", ()):
        assert res["state"][s] == 1
        if world is not None:
            run = slice(int(world["G"]["point_off"][s]), int(world["G"]["point_off"][s]) + int(world["G"]["point_len"][s]))
            assert all(np.array_equal(res[k][run], world["G"][k][run]) for k in ("registered", "point_pool"))
    for s, r in expect.get("nulled", ()) if world is not None else ():
        off, run = int(world["G"]["point_off"][s]), cc.run_of(world["G"], s)
        assert res["point_pool"][off + run.index(r)] == -1 and res["registered"][off + run.index(r)] == 0, (s, r)


# ---------------------------------------------------------------- seeded random worlds
def random_world(seed, S=24, max_run=48, C=32, n_rows=None):
    """S <= 24 slots, runs of at most 48 entries, octaves 0-7.  Clusters of keyframes that see the same rows at close octaves plant redundant
    keyframes; rows seen by three or four of them make a cull change what the next candidate sees."""
    rng = np.random.default_rng(seed)
    n_rows = int(rng.integers(60, 140)) if n_rows is None else n_rows
    live = sorted(rng.choice(S, int(rng.integers(8, S - 1)), replace=False).tolist())
    m = Maker(S=S, n_rows=n_rows, C=C, depth=bool(seed % 3 == 0), ref=bool(seed % 2))
    m.key = rng.permutation(S).astype(np.int64) // 2 * 16 + 4096           # equal keys occur
    m.bad[rng.random(n_rows) < 0.03] = 1
    rows_of = {s: set() for s in live}
    hub = int(rng.choice(live))                  # the current keyframe: in every cluster, so that its list names their members
    for _ in range(int(rng.integers(2, 5))):     # clusters of four to six: one cull leaves the others with three observers
        members = set(rng.choice(live, min(len(live), int(rng.integers(3, 6))), replace=False).tolist()) | {hub}
        shared = rng.choice(n_rows, int(rng.integers(8, 20)), replace=False).tolist()
        for s in members:
            rows_of[s].update(r for r in shared if rng.random() < 0.96)
    for s in live:
        rows_of[s].update(rng.choice(n_rows, int(rng.integers(0, 3)), replace=False).tolist())
    order = rng.permutation(live).tolist()
    for i, s in enumerate(order):
        rows = rng.permutation(sorted(rows_of[s]))[:max_run - 2].tolist()
        rows_of[s] = set(rows)
        for _ in range(int(rng.integers(0, 3))):  # NULL entries and rows out of range
            rows.insert(int(rng.integers(0, len(rows) + 1)), int(rng.choice([-1, -1, n_rows + 3])))
        n = len(rows)
        base = int(rng.integers(0, 7))
        close = [t for t in order[:i] if len(rows_of[t] & rows_of[s]) >= 3]
        m.kf(s, rows, octave=np.clip(base + rng.integers(-1, 2, n), 0, 7), stereo=rng.random(n) < 0.3,
             depth=np.where(rng.random(n) < 0.1, rng.choice([-1.0, 50.0, 40.0, np.nan]), rng.uniform(0.5, 39.0, n)),
             registered=rng.random(n) > 0.03, state=2 if s != hub and rng.random() < 0.05 else 1,
             parent=int(rng.choice(close if close and rng.random() < 0.8 else order[:i])) if i and rng.random() < 0.95 else -1)
    for a in live:                               # covisibility as UpdateConnections would leave it, with a threshold of 3
        for b in live:
            w = len(rows_of[a] & rows_of[b])
            if a < b and w >= 3 and m.state[a] == 1 and m.state[b] == 1:
                m.link(a, b, w)
    if seed % 5 == 0:
        m.not_erase = (rng.random(S) < 0.15).astype(np.uint8)
    if m.ref is not None:
        for r in range(n_rows):
            seen = [s for s in live if r in rows_of[s]]
            m.ref[r] = int(rng.choice(seen)) if seen and rng.random() < 0.9 else int(rng.integers(-1, S))
    good = [s for s in live if m.state[s] == 1]
    cur = hub
    first = int(min(good, key=lambda s: (m.key[s], s)))
    W = m.world("seed_%d" % seed, [], first_slot=first, monocular=not m.depth or seed % 6 == 3, max_cull=MAX_CULL if seed % 4 else int(rng.integers(1, 4)))
    cand = [int(s) for s in W["cov"]["ord_slot"][cur, :W["cov"]["ord_len"][cur]]]
    if seed % 7 == 0:
        cand = rng.permutation(good).tolist()    # (another order than the list's)
    if seed % 4 == 1 and cand:
        cand.insert(int(rng.integers(0, len(cand))), int(rng.choice(cand + [-1, S + 1])))
    W["cand"] = np.array(cand + [-1] * int(rng.integers(0, 3)), np.int32)
    return W


def verdict_changed_by_a_cull(W):
    """a candidate's verdict differs from its verdict on the INITIAL state: up to the first difference the two runs saw the same state"""
    return run_restated(W)["decision"].tolist() != run_restated(W, "stale_state")["decision"].tolist()


# ---------------------------------------------------------------- the reference's own LocalMapping.cpp, KeyFrame.cpp and MapPoint.cpp
GOLDEN_SEEDS = tuple(range(1, 61))               # the first 20 of these whose world the reference can express are recorded
GOLDEN_WORLDS = 20
STAND_INS = ("Frame.h", "Map.h", "KeyFrameDatabase.h", "Converter.h", "ORBmatcher.h", "ORBextractor.h", "ORBVocabulary.h", "Optimizer.h", "LoopClosing.h",
             "Tracking.h")
RECORDED = ("state", "parent", "to_be_erased", "point_pool", "registered", "bad", "n_obs", "n_obs_sum", "ref_slot")


def golden_path():
    import os
    return os.path.join(cc._root(), "tests", "golden", "ref_matcher_culling.npz")


def reference_tree():
    """the reference tree, or None where it is absent"""
    import os
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if all(os.path.exists(os.path.join(ref, "src", f)) for f in ("LocalMapping.cpp", "KeyFrame.cpp", "MapPoint.cpp")) else None


def driver_path():
    import os
    return os.path.join(cc._root(), "oracle", "_ref", "ref_culling")


def build_driver(reference):
    """the reference's src/LocalMapping.cpp, src/KeyFrame.cpp and src/MapPoint.cpp with its include/LocalMapping.h, KeyFrame.h and MapPoint.h,
    unmodified, with tools/ref_culling's stand-ins force-included so that their guards shut out the reference's headers of the same names"""
    import os
    import subprocess
    shadow = os.path.join(cc._root(), "tools", "ref_culling")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-w", "-I" + shadow, "-I" + os.path.join(reference, "include"), "-I" + reference]
    for h in STAND_INS:
        cmd += ["-include", os.path.join(shadow, h)]
    dbow = os.path.join(reference, "Thirdparty", "DBoW2", "DBoW2")       # (KeyFrame holds a BowVector and a FeatureVector)
    cmd += ["-o", driver_path(), os.path.join(shadow, "driver.cpp")] + [os.path.join(reference, "src", f) for f in ("LocalMapping.cpp", "KeyFrame.cpp", "MapPoint.cpp")]
    cmd += [os.path.join(dbow, "BowVector.cpp"), os.path.join(dbow, "FeatureVector.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    return driver_path()


def expressible(W):
    """The world as the reference can run it, or None.  Its loop has no max_cull and no skips but keyframe 0: candidates the contract skips are
    taken out of the list.  It reads through mpParent, so every culled keyframe needs a usable parent; and where a culled keyframe's parent is
    culled too, the stated difference about EraseChild shows, so such a world is left out."""
    G = W["G"]
    S = len(G["state"])
    cand, seen = [], set()
    for a in (int(a) for a in W["cand"]):
        if 0 <= a < S and G["state"][a] == 1 and cc.valid_run(G, a) and a not in seen:
            cand.append(a)
            seen.add(a)
    W = dict(W, cand=np.array(cand, np.int32), max_cull=MAX_CULL, cap=4 * S)
    res = run_restated(W)
    culled = [int(s) for s in res["culled_slot"] if s >= 0]
    if res["counts"][0] != len(cand) or res["counts"][9]:
        return None
    for a in culled:
        p0, p1 = int(G["parent"][a]), int(res["parent"][a])
        if not (0 <= p0 < S and G["state"][p0] != 0 and p0 != a) or p0 in culled or p1 in culled:
            return None
    return W


def world_bytes(W):
    """the driver's input, which is also what `crc` is taken over"""
    G, V, cov, C = W["G"], W["views"], W["cov"], W["C"]
    S, n_rows, pool = len(G["state"]), len(W["bad"]), len(G["point_pool"])
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    zero = lambda n: np.zeros(n, np.int32)
    parts = [i32([S, n_rows, pool, C, len(W["cand"]), int(W["monocular"]), W["first_slot"], int(W["ref_slot"] is not None)]), i32(G["state"]),
             np.ascontiguousarray(G["order_key"], np.int64).tobytes(), i32(G["point_off"]), i32(G["point_len"]), i32(G["point_pool"]), i32(G["registered"]),
             i32(G["parent"]), i32(W["bad"]), i32(V["octave"]), i32(V["stereo"]), f32(np.zeros(pool) if V["depth"] is None else V["depth"]), f32(V["th_depth"]),
             i32(zero(S) if W["not_erase"] is None else W["not_erase"]), i32(zero(n_rows) if W["ref_slot"] is None else W["ref_slot"])]
    parts += [i32(cov[k]) for k in ("conn_len", "conn_slot", "conn_weight", "ord_len", "ord_slot", "ord_weight")]
    return b"".join(parts + [i32(W["cand"])])


def run_driver(W, workdir):
    """a world through the reference -> dict of `raw` (the driver's int32 output) and `crc`"""
    import os
    import subprocess
    import zlib
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    raw_in = world_bytes(W)
    with open(src, "wb") as f:
        f.write(raw_in)
    subprocess.check_call([driver_path(), src, dst], timeout=120)
    return dict(raw=np.fromfile(dst, np.int32), crc=np.array(zlib.crc32(raw_in), np.uint32))


def unpack(W, raw):
    """the driver's output as the yardsticks' arrays: RECORDED and the covisibility lists"""
    S, n_rows, pool, C = len(W["G"]["state"]), len(W["bad"]), len(W["G"]["point_pool"]), W["C"]
    assert len(raw) == 3 * S + 2 * pool + 4 * n_rows + 2 * (S + 2 * S * C)
    at, out = 0, {}
    for k, n in (("state", S), ("parent", S), ("to_be_erased", S), ("point_pool", pool), ("registered", pool), ("bad", n_rows), ("n_obs", n_rows),
                 ("n_obs_sum", n_rows), ("ref_slot", n_rows)):
        out[k] = raw[at:at + n]
        at += n
    cov = {}
    for kind in ("conn", "ord"):
        cov[kind + "_len"] = raw[at:at + S]
        cov[kind + "_slot"] = raw[at + S:at + S + S * C].reshape(S, C)
        cov[kind + "_weight"] = raw[at + S + S * C:at + S + 2 * S * C].reshape(S, C)
        at += S + 2 * S * C
    out["cov"] = cov
    return out


def n_obs_recomputed(W, res):
    """Observations() of every row from the arrays a yardstick left: the contract's sum"""
    G, n = W["G"], np.zeros(len(W["bad"]), np.int32)
    for B in range(len(G["state"])):
        if res["state"][B] == 1 and cc.valid_run(G, B):
            for e in range(int(G["point_off"][B]), int(G["point_off"][B]) + int(G["point_len"][B])):
                r = int(res["point_pool"][e])
                if 0 <= r < len(n) and not res["bad"][r] and res["registered"][e]:
                    n[r] += 1 + int(W["views"]["stereo"][e] != 0)
    return n


def same_as_recorded(W, res, raw):
    """a yardstick's result against what the reference's own code left"""
    rec = unpack(W, raw)
    for k in ("state", "parent", "point_pool", "registered", "bad"):
        assert np.array_equal(res[k], rec[k]), (W["name"], k, np.argwhere(np.asarray(res[k]) != rec[k])[:6].ravel().tolist())
    if res["to_be_erased"] is not None:
        assert np.array_equal(res["to_be_erased"], rec["to_be_erased"]), (W["name"], "to_be_erased")
    if res["ref_slot"] is not None:
        assert np.array_equal(res["ref_slot"], rec["ref_slot"]), (W["name"], "ref_slot", np.argwhere(res["ref_slot"] != rec["ref_slot"])[:6].ravel().tolist())
    for k, v in rec["cov"].items():
        assert np.array_equal(res["cov"][k], v), (W["name"], "cov", k)
    good = rec["bad"] == 0                       # the stated difference: the stored nObs is the sum over the observations, and the contract's recomputed one
    assert np.array_equal(rec["n_obs"][good], rec["n_obs_sum"][good]) and np.array_equal(n_obs_recomputed(W, res)[good], rec["n_obs"][good]), (W["name"], "nObs")


def golden_worlds():
    """name -> world: the named cases the reference can express, then GOLDEN_WORLDS seeded worlds of at most 16 slots"""
    out = {}
    for name in CASES:
        W = expressible(build_case(name)[0])
        if W is not None:
            out[name] = W
    n = 0
    for seed in GOLDEN_SEEDS:
        W = expressible(random_world(seed, S=16))
        if W is not None and n < GOLDEN_WORLDS:
            out[W["name"]] = W
            n += 1
    assert n == GOLDEN_WORLDS
    return out


def write_golden(recorded):
    """recorded: name -> dict(raw, crc); members in a fixed order with a fixed date, so that the file is reproducible"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w") as z:
        for name, rec in recorded.items():
            for k in ("raw", "crc"):
                buf = io.BytesIO()
                np.save(buf, rec[k])
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, k), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


def load_golden():
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, k = member.rsplit(".", 1)
            out.setdefault(name, {})[k] = z[member]
    return out
