"""jsorb_fuse_map (include/jsorb.h): Fuse with its map mutations over the device state - the converter from a case of tests/fuse_replay.py's
vocabulary to the device arrays, the restatement of the contract's steps 0-5 over those arrays (descriptors deferred to the end of a target), the
immediate-recomputation run on fuse_replay.LiveMap it is held to, the constructed cases and the restatement's mutants.  Not a test module and
not a conftest: tests/test_fuse_apply_host.py and tests/test_gpu_fuse_apply.py import it.

A WORLD is a dict of numpy arrays in the layouts of jsorb_keyframe_graph / jsorb_map_point_table / jsorb_keyframe_keypoints: state, order_key,
point_off, point_len [S]; point_pool, registered, x, y, octave, uright, desc [pool]; floats [9, n_rows] (Px Py Pz Pnx Pny Pnz MaxDistance
invariance_maxDistance invariance_minDistance), tdesc [n_rows, 32], bad [n_rows]; visible, found [n_rows] or None; list [n]; targets [T] (slots),
Rcw, tcw, Ow per target; sim3, replace_loop, log_cap; case: the case it came from (the search runs on it) and slot_of [keyframes]."""
from collections import OrderedDict

import numpy as np

import fuse_replay
import ref_matcher_cases as cases
import test_fuse_host as tf
from fuse_replay import EV_ADD_MAP_POINT, EV_REPLACE

f32 = np.float32
FILES = ("fuse", "fuse_sim3")
COUNTS = ("n_fused", "n_replace", "n_add", "n_bad_in_slot", "n_rows_bad", "n_descriptors_changed", "n_skipped_targets", "n_dropped", "n_log", "log_overflow")
WRITTEN = ("point_pool", "registered", "bad", "tdesc", "replaced", "visible", "found")
OUTPUTS = ("best_idx", "best_dist", "replace_point", "n_fused", "log", "counts")
REFERENCE_KEYS = ("nfused", "kf_mps", "pt_bad", "pt_replaced", "pt_nobs", "pt_desc")
CHUNKS = (256, 4)                                # FA_CHUNK of the shipped library and of tiny_fuse_apply (jetson_slam_amd/build.py)
MUTANTS = ("observations_ge", "observations_ignore_stereo", "replace_without_erase", "head_from_the_start", "no_descriptor", "descriptor_over_bad_keyframes",
           "descriptor_by_slot")


def stored(name):
    """the cases of tests/golden/ref_matcher_<name>.npz, as tests/test_ref_matcher.py loads them"""
    from oracle import pyref_matcher as rm
    m = cases.MATCHERS[name]
    return OrderedDict((k, cases.named(m.prepare(c), m.driver, k)) for k, c in rm.load_golden(name).items())


def permutation(c, seed):
    """a seeded slot permutation of the case's keyframes and one absent slot; None: the identity"""
    S = len(c["KF"]) + 1
    return np.arange(S) if seed is None else np.random.default_rng(seed).permutation(S)


# ------------------------------------------------------------------ the converter
def to_world(c, perm=None):
    KF, P = c["KF"], c["P"]
    nkf, n_rows = len(KF), len(P["Px"])
    S = nkf + 1
    perm = np.arange(S) if perm is None else np.asarray(perm)
    assert sorted(perm.tolist()) == list(range(S))
    slot_of = perm[:nkf].astype(np.int64)
    kf_state = np.asarray(c.get("_kf_state", np.ones(nkf, np.uint8)), np.uint8)
    state, order_key = np.zeros(S, np.uint8), np.zeros(S, np.int64)
    point_off, point_len = np.zeros(S, np.int32), np.zeros(S, np.int32)
    lens = [len(K["mps"]) for K in KF]
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for k in range(nkf):
        s = slot_of[k]
        state[s], order_key[s], point_off[s], point_len[s] = kf_state[k], k, starts[k], lens[k]
    pool = int(starts[-1])
    cat = lambda key, dt, shape=(): np.concatenate([np.asarray(K[key], dt).reshape((-1,) + shape) for K in KF]) if nkf else np.zeros((0,) + shape, dt)
    point_pool = cat("mps", np.int32)
    registered = np.zeros(pool, np.uint8)
    obs = np.asarray(c["obs"], np.int64).reshape(-1, 3)
    # the case is expressible: every observation's slot holds its point, one observation per (point, keyframe), no run holds a row twice
    assert len({(int(p), int(k)) for p, k, _ in obs}) == len(obs), "two observations of one point in one keyframe"
    for p, k, i in obs:
        assert KF[k]["mps"][i] == p, ("an observation whose slot holds another point", p, k, i)
        registered[starts[k] + i] = 1
    for k, K in enumerate(KF):
        held = np.asarray(K["mps"])[np.asarray(K["mps"]) >= 0]
        assert len(set(held.tolist())) == len(held), ("a run holds a row twice", k)
    floats = np.stack([np.asarray(P[k], np.float32) for k in ("Px", "Py", "Pz", "Nx", "Ny", "Nz", "maxd", "maxdi", "mindi")]) if n_rows else np.zeros((9, 0), np.float32)
    targets = [int(k) for k in c["targets"]]
    sim3 = c.get("Scw") is not None
    assert sim3 == (int(c["prm"]["check"]) == 0)
    opt = lambda key: None if c.get(key) is None else np.asarray(c[key], np.int32).copy()
    lst = np.asarray(c["list"], np.int32)
    return dict(S=S, n_rows=n_rows, pool=pool, state=state, order_key=order_key, point_off=point_off, point_len=point_len, point_pool=point_pool,
                registered=registered, x=cat("x", np.float32), y=cat("y", np.float32), octave=cat("octave", np.int32), uright=cat("uright", np.float32),
                desc=cat("desc", np.uint8, (32,)), floats=floats, tdesc=np.asarray(P["desc"], np.uint8).reshape(n_rows, 32).copy(),
                bad=np.asarray(P["bad"], np.uint8).copy(), visible=opt("_visible"), found=opt("_found"), list=lst,
                targets=np.array([slot_of[k] for k in targets], np.int32),
                Rcw=np.array([KF[k]["Rcw"] for k in targets], np.float32).reshape(len(targets), 9),
                tcw=np.array([KF[k]["tcw"] for k in targets], np.float32).reshape(len(targets), 3),
                Ow=np.array([KF[k]["Ow"] for k in targets], np.float32).reshape(len(targets), 3),
                sim3=sim3, replace_loop=int(c.get("replace_loop", 0)) if sim3 else 0,
                log_cap=int(c["_log_cap"]) if "_log_cap" in c else max(len(targets) * len(lst), 1), case=c, slot_of=slot_of, name=c.get("_name", "?"))


# ------------------------------------------------------------------ the restatement
def distinctive(D):
    """rules 2-5 of jsorb_distinctive_descriptors_async: the index of the first row with the least median distance"""
    bits = np.unpackbits(np.asarray(D, np.uint8).reshape(len(D), 32), axis=1).astype(np.int32)
    dist = (bits[:, None, :] != bits[None, :, :]).sum(axis=2)
    med = np.sort(dist, axis=1)[:, (len(D) - 1) // 2]
    return int(np.argmin(med))


def entry_slots(W):
    """ent_slot: the slot whose run holds each entry (valid runs of slots with state != 0), -1 elsewhere"""
    ent = np.full(W["pool"], -1, np.int64)
    for s in range(W["S"]):
        o, n = int(W["point_off"][s]), int(W["point_len"][s])
        if W["state"][s] != 0 and o >= 0 and n >= 0 and o + n <= W["pool"]:
            assert (ent[o:o + n] < 0).all(), "overlapping runs"
            ent[o:o + n] = s
    return ent


def restate(po, W, mutant=None, search=None):
    """steps 0-5 of jsorb_fuse_map_async over the world's arrays.  search(t, desc[n, 32], skip[n]) -> (best_idx, best_dist)[n]: by default the
    numpy restatement of k_fuse_match on the world's case, one target at a time"""
    assert mutant is None or mutant in MUTANTS
    c = W["case"]
    if search is None:
        inner = cases.fuse_search(po, c, "restatement")

        def search(t, desc, skip):
            r = inner([t], list(range(len(skip))), desc, skip[None, :])
            return r[0][0], r[1][0]
    S, n_rows, state, key = W["S"], W["n_rows"], W["state"], W["order_key"]
    pool, reg, bad, tdesc = W["point_pool"].copy(), W["registered"].copy(), W["bad"].copy(), W["tdesc"].copy()
    replaced = np.full(n_rows, -1, np.int32)
    visible, found = (None if W[k] is None else W[k].copy() for k in ("visible", "found"))
    ent = entry_slots(W)
    stereo = W["uright"] >= 0
    lst, T, n, sim3 = W["list"], len(W["targets"]), len(W["list"]), W["sim3"]
    best_idx, best_dist, replace_point = (np.full((T, n), -1, np.int32) for _ in range(3))
    n_fused, log, cnt = np.zeros(T, np.int32), [], dict.fromkeys(COUNTS, 0)
    nobs_dead = {}
    row_ok = lambda r: 0 <= r < n_rows
    entries = lambda r: np.nonzero((pool == r) & (reg != 0) & (ent >= 0))[0]
    observations = lambda r: [e for e in entries(r) if state[ent[e]] == 1]

    def n_observations(r):
        return sum(1 + (0 if mutant == "observations_ignore_stereo" else int(stereo[e])) for e in observations(r))

    def replace(p, q, marked):
        if p == q:
            return
        log.append((EV_REPLACE, p, q, -1))
        cnt["n_replace"] += 1
        q_slots = {int(ent[e]) for e in entries(q)}
        dying = n_observations(p)
        for e in entries(p):
            if int(ent[e]) in q_slots and mutant != "replace_without_erase":
                pool[e], reg[e] = -1, 0
            else:
                pool[e] = q
        if not bad[p]:
            cnt["n_rows_bad"] += 1
            nobs_dead[p] = dying
        bad[p], replaced[p] = 1, q
        if found is not None:
            found[q] += found[p]
            visible[q] += visible[p]
        if q not in marked:
            marked.append(q)

    for t in range(T):
        A = int(W["targets"][t])
        o, ln = (int(W["point_off"][A]), int(W["point_len"][A])) if 0 <= A < S else (0, 0)
        if not (0 <= A < S and state[A] == 1 and o >= 0 and ln >= 0 and o + ln <= W["pool"] and ln < (1 << 18)):
            cnt["n_skipped_targets"] += 1
            continue
        snapshot = {int(r) for r in pool[o:o + ln] if row_ok(r) and not bad[r]} if sim3 else None

        def head(r):
            if not row_ok(r) or bad[r]:
                return False
            return r not in snapshot if sim3 else not any(ent[e] == A for e in observations(r))
        at_start = np.array([head(int(r)) for r in lst], bool)
        bi, bd = search(t, tdesc[np.clip(lst, 0, max(n_rows - 1, 0))].reshape(n, 32) if n_rows else np.zeros((n, 32), np.uint8), (~at_start).astype(np.uint8))
        best_idx[t], best_dist[t] = bi, bd
        marked = []
        for i in range(n):
            r = int(lst[i])
            if not (at_start[i] if mutant == "head_from_the_start" else head(r)) or best_idx[t, i] < 0:
                continue
            e = o + int(best_idx[t, i])
            q = int(pool[e])
            n_fused[t] += 1
            if q < -1 or q >= n_rows:
                cnt["n_dropped"] += 1
            elif q == -1:
                pool[e], reg[e] = r, 1
                log.append((EV_ADD_MAP_POINT, r, A, int(best_idx[t, i])))
                cnt["n_add"] += 1
            elif bad[q]:
                cnt["n_bad_in_slot"] += 1
            elif sim3:
                replace_point[t, i] = q
            else:
                nq, nr = n_observations(q), n_observations(r)
                if (nq >= nr) if mutant == "observations_ge" else (nq > nr):
                    replace(r, q, marked)
                else:
                    replace(q, r, marked)
        if sim3 and W["replace_loop"]:
            for i in range(n):
                if replace_point[t, i] >= 0:
                    replace(int(replace_point[t, i]), int(lst[i]), marked)
        for q in marked:                                       # step 5
            if bad[q] or mutant == "no_descriptor":
                continue
            seen = [e for e in entries(q) if state[ent[e]] == 1 or (mutant == "descriptor_over_bad_keyframes" and state[ent[e]] == 2)]
            if not seen:
                continue
            seen.sort(key=(lambda e: int(ent[e])) if mutant == "descriptor_by_slot" else (lambda e: (int(key[ent[e]]), int(ent[e]))))
            d = W["desc"][seen[distinctive(W["desc"][seen])]]
            if not np.array_equal(d, tdesc[q]):
                cnt["n_descriptors_changed"] += 1
            tdesc[q] = d
    cnt["n_fused"], cnt["n_log"] = int(n_fused.sum()), len(log)
    cnt["log_overflow"] = int(len(log) > W["log_cap"])
    log_out = np.full((W["log_cap"], 4), -1, np.int32)
    kept = np.array(log[:W["log_cap"]], np.int32).reshape(-1, 4)
    log_out[:len(kept)] = kept
    return dict(point_pool=pool, registered=reg, bad=bad, tdesc=tdesc, replaced=replaced, visible=visible, found=found, best_idx=best_idx, best_dist=best_dist,
                replace_point=replace_point, n_fused=n_fused, log=log_out, counts=np.array([cnt[k] for k in COUNTS], np.int32),
                events=np.array(log, np.int32).reshape(-1, 4), nobs_dead=nobs_dead, nobs={r: n_observations(r) for r in range(n_rows)} if n_rows <= 4096 else None)


def same(want, got, what=""):
    """every array the call writes and every output, bit for bit"""
    for k in WRITTEN + OUTPUTS:
        a, b = want[k], got[k]
        assert (a is None and b is None) or (a is not None and b is not None and np.asarray(a).shape == np.asarray(b).shape and np.array_equal(a, b)), (what, k)


def as_reference(W, res):
    """a restated (or device) result under the keys of the reference driver's output (oracle/pyref_matcher.py), keyframes in the case's order"""
    c = W["case"]
    off, ln = W["point_off"], W["point_len"]
    mps = [res["point_pool"][off[s]:off[s] + ln[s]] for s in W["slot_of"]]
    nobs = np.array([res["nobs_dead"].get(r, res["nobs"][r]) for r in range(W["n_rows"])], np.int32).reshape(W["n_rows"])
    T = len(W["targets"])
    out = dict(nfused=res["n_fused"].astype(np.int32), kf_mps=np.concatenate(mps).astype(np.int32) if mps else np.zeros(0, np.int32),
               pt_bad=res["bad"].astype(np.uint8), pt_replaced=res["replaced"].astype(np.int32), pt_nobs=nobs, pt_desc=res["tdesc"])
    if c.get("Scw") is not None:
        out["replace"] = res["replace_point"].reshape(T, len(W["list"]))
    return out


def events_as_reference(W, ev):
    """the log's records with an AddMapPoint's slot as the case's keyframe index"""
    kf_of = {int(s): k for k, s in enumerate(W["slot_of"])}
    ev = np.array(ev, np.int32).reshape(-1, 4)
    for row in ev:
        if row[0] == EV_ADD_MAP_POINT:
            row[2] = kf_of[int(row[2])]
    return ev


# ------------------------------------------------------------------ the immediate recomputation on fuse_replay.LiveMap
class Live(fuse_replay.LiveMap):
    """LiveMap with what the stored cases do not have: keyframes that are bad (their observations stay with the point, move in a Replace, and count
    for neither Observations() - the header's definition - nor the descriptor, MapPoint.cpp:292-298), mnVisible / mnFound"""

    def __init__(self, case):
        self.kf_state = np.asarray(case.get("_kf_state", np.ones(len(case["KF"]), np.uint8)))
        self.visible, self.found = (None if case.get(k) is None else [int(v) for v in case[k]] for k in ("_visible", "_found"))
        super().__init__(case)

    def add_observation(self, p, k, idx):
        before = self.nobs[p]
        super().add_observation(p, k, idx)
        if self.kf_state[k] != 1:
            self.nobs[p] = before

    def replace(self, p, q):
        if p != q and self.found is not None:
            self.found[q] += self.found[p]
            self.visible[q] += self.visible[p]
        super().replace(p, q)

    def compute_distinctive_descriptors(self, q):
        keep, self.obs[q] = self.obs[q], {k: i for k, i in self.obs[q].items() if self.kf_state[k] == 1}
        try:
            super().compute_distinctive_descriptors(q)
        finally:
            self.obs[q] = keep


def live_run(po, c):
    """fuse_replay.replay(..., "sequential") over Live, with the targets that are not good keyframes skipped: descriptors recomputed inside every
    Replace, as the reference does"""
    m = Live(c)
    search = cases.fuse_search(po, c, "restatement")
    targets, lst = [int(k) for k in c["targets"]], [int(p) for p in c["list"]]
    sim3 = c.get("Scw") is not None
    T, n = len(targets), len(lst)
    best, nfused, rp = np.full((T, n), -1, np.int32), np.zeros(T, np.int32), np.full((T, n), -1, np.int32)
    for t, k in enumerate(targets):
        if m.kf_state[k] != 1:
            continue
        already = {p for p in m.mps[k] if p >= 0 and not m.bad[p]} if sim3 else None
        head = lambda p: (p >= 0 and not m.bad[p] and p not in already) if sim3 else m.head_passes(p, k)
        skip = np.array([[0 if head(p) else 1 for p in lst]], np.uint8)
        best[t] = search([t], list(range(n)), m.desc[[max(p, 0) for p in lst]].reshape(n, 32), skip)[0][0]
        for i, p in enumerate(lst):
            if not head(p) or best[t, i] < 0:
                continue
            if sim3:
                rp[t, i] = m.tail_sim3(k, p, int(best[t, i]))
            else:
                m.tail(k, p, int(best[t, i]))
            nfused[t] += 1
        if sim3 and int(c["replace_loop"]):
            for i, p in enumerate(lst):
                if rp[t, i] >= 0:
                    m.replace(int(rp[t, i]), p)
    ev = np.array(m.events, np.int32).reshape(-1, 4)
    n_pts = len(m.bad)
    out = dict(nfused=nfused, kf_mps=np.array([p for s in m.mps for p in s], np.int32), pt_bad=np.array(m.bad, np.uint8).reshape(n_pts),
               pt_replaced=np.array(m.replaced, np.int32).reshape(n_pts), pt_nobs=np.array(m.nobs, np.int32).reshape(n_pts), pt_desc=m.desc.copy(),
               events=ev[np.isin(ev[:, 0], (EV_REPLACE, EV_ADD_MAP_POINT))], best_idx=best, visible=m.visible, found=m.found)
    if sim3:
        out["replace"] = rp
    return out


def check_against_live(po, c, W, res):
    """the restatement's (or the device's) result is the immediate recomputation's: map, counts per target, the log, the searched keypoints"""
    live = live_run(po, c)
    got = as_reference(W, res)
    # the one stated difference of the deferred descriptors: a row that inherited and then died within one target keeps the descriptor it had (the
    # reference leaves the one of its last inheritance); a bad row's descriptor is never read
    ev = res["events"]
    for r in np.nonzero((got["pt_desc"] != live["pt_desc"]).any(axis=1))[0]:
        was_q, was_p = np.nonzero((ev[:, 0] == EV_REPLACE) & (ev[:, 2] == r))[0], np.nonzero((ev[:, 0] == EV_REPLACE) & (ev[:, 1] == r))[0]
        assert got["pt_bad"][r] and len(was_q) and len(was_p) and was_q[0] < was_p[0], ("descriptor of row", r)
        got["pt_desc"][r] = live["pt_desc"][r]
    fuse_replay.same_map(got, live, REFERENCE_KEYS)
    assert np.array_equal(events_as_reference(W, res["events"]), live["events"]) and np.array_equal(res["best_idx"], live["best_idx"])
    for k in ("visible", "found"):
        assert (res[k] is None and live[k] is None) or res[k].tolist() == live[k]
    return live


# ------------------------------------------------------------------ constructed cases
def _prm(check):
    return tf.default_params(check=check, th=f32(3 if check else 4))


def _at(prm, uv):
    return dict(tf.points_at(uv, prm), Nx=np.zeros(len(uv), np.float32), Ny=np.zeros(len(uv), np.float32), Nz=np.ones(len(uv), np.float32))


def _holder(prm, bits, stereo=()):
    """an observer that is no target: keypoint i at (40 + 20 i, 200) - no list point projects there - at distance bits[i] from the zero descriptor"""
    return tf.kps([(40 + 20 * i, 200, 0, b) + ((30.0 + 20 * i,) if i in stereo else ()) for i, b in enumerate(bits)], prm)


def _case(check, kfs, uv, mps, obs, targets, lst, replace_loop=0, bad=(), **extra):
    prm, I = _prm(check), tf.IDENTITY
    P = _at(prm, uv)
    P["bad"] = np.array([int(i in bad) for i in range(len(uv))], np.uint8)
    kw = {} if check else dict(Scw=np.concatenate([cases.scw_of(I, 1.0)] * len(targets)), replace_loop=replace_loop)
    c = cases.fuse_case(prm, [k(prm) for k in kfs], [I] * len(kfs), P, mps, obs, targets=targets, lst=lst, **kw)
    c.update({"_" + k: v for k, v in extra.items()})
    return c


def constructed():
    """name -> case.  Identity poses and depth 4: a point at pixel (u, v) finds the target's keypoint at that pixel.  Rows are point ids."""
    out = OrderedDict()
    tgt = lambda *kp: (lambda prm: tf.kps(list(kp), prm))
    hold = lambda bits, stereo=(): (lambda prm: _holder(prm, bits, stereo))
    far = (10, 10)
    # 0, 1: two list points at the pixel of target keypoint 0, whose point 2 has more observations than either: Replace(0 -> 2), Replace(1 -> 2).
    # 2 inherits twice in one target; 0 and 2 both observe keyframe 1, so 0's entry there is erased.  The descriptor comes from five observers.
    out["a_survivor_inherits_twice"] = _case(
        1, [tgt((100, 100, 0, 10)), hold([20, 4, 30]), hold([22]), hold([24, 26]), hold([28])], [(100, 100), (100, 100), far],
        [[2], [2, 0, -1], [2], [0, 1], [1]], [(2, 0, 0), (2, 1, 0), (2, 2, 0), (0, 1, 1), (0, 3, 0), (1, 3, 1), (1, 4, 0)], [0], [0, 1])
    # point 0 takes the slot of 2 (one observation against two), then 1 (three) takes it from 0: the survivor of the first Replace dies in the second
    out["a_survivor_is_replaced_later"] = _case(
        1, [tgt((100, 100, 0, 10)), hold([20, 21]), hold([22, 23]), hold([24]), hold([26])], [(100, 100), (100, 100), far],
        [[2], [0, 1], [0, 1], [1], [-1]], [(2, 0, 0), (0, 1, 0), (0, 2, 0), (1, 1, 1), (1, 2, 1), (1, 3, 0)], [0], [0, 1])
    # one observation each: the slot's point loses
    out["equal_observations"] = _case(1, [tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far], [[1], [0]], [(1, 0, 0), (0, 1, 0)], [0], [0])
    # two observations each, one of the slot's point's a stereo one: 3 > 2, the list point loses
    out["a_stereo_observation_flips_it"] = _case(
        1, [tgt((100, 100, 0, 10)), hold([20, 21], stereo=(1,)), hold([22])], [(100, 100), far],
        [[1], [0, 1], [0]], [(1, 0, 0), (1, 1, 1), (0, 1, 0), (0, 2, 0)], [0], [0])
    # a bad point in the slot: counted as fused, nothing changes
    out["a_bad_point_in_the_slot"] = _case(1, [tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far], [[1], [0]], [(0, 1, 0)], [0], [0], bad=(1,))
    # the slot holds the point at hand without an observation: the head test passes, Replace(0 -> 0) does nothing; point 1 adds itself next to it
    c = _case(1, [tgt((100, 100, 0, 10), (140, 100, 0, 10)), hold([20, 21])], [(100, 100), (140, 100)], [[-1, -1], [0, 1]], [(0, 1, 0), (1, 1, 1)], [0], [0, 1])
    c["KF"][0]["mps"][0] = 0
    out["an_unregistered_entry_holds_the_point_at_hand"] = c
    # keyframe 0 is bad and holds an observation of 2, which therefore counts one observation, as many as 0: Replace(2 -> 0) moves both entries.
    # The good observers (bits 10, 20: N = 2, the first wins) give bits 10; with the bad keyframe's bits 30 in front, N = 3 would give bits 30
    out["an_observation_in_a_bad_keyframe"] = _case(
        1, [hold([30]), tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far, far],
        [[2], [2], [0]], [(2, 0, 0), (2, 1, 0), (0, 2, 0)], [1], [0], kf_state=np.array([2, 1, 1], np.uint8))
    # the same row twice: the second visit fails the live head test (overload 1), or is Replace(0 -> 0) (overload 2)
    for check in (1, 0):
        out["a_duplicate_list_row_overload_%d" % (2 - check)] = _case(
            check, [tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far], [[-1], [0]], [(0, 1, 0)], [0], [0, 0], replace_loop=1)
    out["a_null_list_entry"] = _case(1, [tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far], [[-1], [0]], [(0, 1, 0)], [0], [-1, 0])
    # overload 2: the slot's point 1 is handed back, and the loop replaces it by 0
    out["the_replace_loop"] = _case(0, [tgt((100, 100, 0, 10)), hold([20]), hold([22])], [(100, 100), far], [[1], [0], [1]],
                                    [(1, 0, 0), (0, 1, 0), (1, 2, 0)], [0], [0], replace_loop=1, visible=[5, 7], found=[2, 3])
    # a bad keyframe between two good targets: skipped, its row of the outputs -1
    out["a_skipped_target_between_two"] = _case(
        1, [tgt((100, 100, 0, 10)), tgt((100, 100, 0, 10)), tgt((100, 100, 0, 10)), hold([20])], [(100, 100), far],
        [[-1], [-1], [-1], [0]], [(0, 3, 0)], [0, 1, 2], [0], kf_state=np.array([1, 2, 1, 1], np.uint8))
    # three events, room for one
    out["log_cap_smaller_than_the_log"] = _case(
        1, [tgt((100, 100, 0, 10), (140, 100, 0, 10), (180, 100, 0, 10)), hold([20, 21, 22]), hold([24])], [(100, 100), (140, 100), (180, 100), far],
        [[-1, 3, -1], [0, 1, 2], [3]], [(0, 1, 0), (1, 1, 1), (2, 1, 2), (3, 0, 1), (3, 2, 0)], [0], [0, 1, 2], log_cap=1)
    out["visible_and_found_sums"] = dict(out["equal_observations"], _visible=[10, 3], _found=[4, 2])
    for name, c in out.items():
        cases.named(c, "fuse_sim3" if c.get("Scw") is not None else "fuse", name)
    return out


# mutant -> the constructed case that must notice it (descriptor_by_slot: under REVERSED slots)
MUTANT_CASES = {"observations_ge": "equal_observations", "observations_ignore_stereo": "a_stereo_observation_flips_it",
                "replace_without_erase": "a_survivor_inherits_twice", "head_from_the_start": "a_duplicate_list_row_overload_1",
                "no_descriptor": "a_survivor_inherits_twice", "descriptor_over_bad_keyframes": "an_observation_in_a_bad_keyframe",
                "descriptor_by_slot": "equal_observations"}


def reversed_slots(c):
    return np.arange(len(c["KF"]) + 1)[::-1].copy()


# ------------------------------------------------------------------ a world that crosses the index build's block edges
def padded_world(po, seed, S=200, run=400, n_rows=70000, n_targets=8):
    """A random block of the fuse file's generator (tests/ref_matcher_cases.py) inside a map of S slots with `run` entries each and n_rows rows: the
    extra keyframes hold rows of the block (the list's and the slots' points: more observers, in other blocks of the index build) and rows beyond it"""
    rng = np.random.default_rng(seed)
    c = cases.with_grids(cases.Fuse.random_block(rng, n_targets=n_targets, n=120, N=run, stereo=0.5, n_world=3 * run))
    W = to_world(cases.named(c, "fuse", "padded%d" % seed), rng.permutation(len(c["KF"]) + 1))
    S0, rows0, pool0 = W["S"], W["n_rows"], W["pool"]
    extra = S - S0
    assert extra > 0 and n_rows > rows0
    pool = pool0 + extra * run
    grow = lambda a, n, fill: np.concatenate([a, np.full((n,) + a.shape[1:], fill, a.dtype)])
    slots = rng.permutation(S)                                  # the block's slots spread over all S
    remap = slots[:S0]
    state, order_key, point_off, point_len = np.zeros(S, np.uint8), np.zeros(S, np.int64), np.zeros(S, np.int32), np.zeros(S, np.int32)
    state[remap], order_key[remap], point_off[remap], point_len[remap] = W["state"], W["order_key"], W["point_off"], W["point_len"]
    keys = rng.permutation(extra) + S0
    live_rows = np.nonzero(W["bad"] == 0)[0]
    point_pool, registered = grow(W["point_pool"], extra * run, -1), grow(W["registered"], extra * run, 0)
    for j, s in enumerate(slots[S0:]):
        state[s], order_key[s], point_off[s], point_len[s] = (2 if j % 23 == 5 else 1), keys[j], pool0 + j * run, run
        rows = np.concatenate([rng.choice(live_rows, min(12, len(live_rows)), replace=False), rng.choice(np.arange(rows0, n_rows), run // 2, replace=False)])
        at = pool0 + j * run + rng.choice(run, len(rows), replace=False)
        point_pool[at] = rows
        registered[at] = rng.random(len(rows)) < 0.9
    x, y = grow(W["x"], extra * run, 0), grow(W["y"], extra * run, 0)
    x[pool0:], y[pool0:] = rng.uniform(0, 320, extra * run), rng.uniform(0, 240, extra * run)
    octave, uright = grow(W["octave"], extra * run, 0), grow(W["uright"], extra * run, -1)
    uright[pool0:] = np.where(rng.random(extra * run) < 0.5, 1.0, -1.0)
    desc = np.concatenate([W["desc"], rng.integers(0, 256, (extra * run, 32), dtype=np.uint8)])
    floats = np.concatenate([W["floats"], np.ones((9, n_rows - rows0), np.float32)], axis=1)
    tdesc, bad = grow(W["tdesc"], n_rows - rows0, 0), grow(W["bad"], n_rows - rows0, 0)
    W.update(S=S, n_rows=n_rows, pool=pool, state=state, order_key=order_key, point_off=point_off, point_len=point_len, point_pool=point_pool,
             registered=registered, x=x, y=y, octave=octave, uright=uright, desc=desc, floats=floats, tdesc=tdesc, bad=bad,
             targets=remap[W["targets"]].astype(np.int32), slot_of=remap[W["slot_of"]],
             visible=rng.integers(0, 50, n_rows).astype(np.int32), found=rng.integers(0, 50, n_rows).astype(np.int32))
    return W
