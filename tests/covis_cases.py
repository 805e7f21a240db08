"""Worlds and yardsticks for jsorb_update_connections / jsorb_erase_connections (include/jsorb.h), shared by tests/test_covis_host.py,
tests/test_ref_covis.py and tests/test_gpu_covis.py.  numpy only: nothing here needs a GPU.  Not a test module.

* run_literal: a literal sequential transcription of KeyFrame::AddConnection / UpdateBestCovisibles (KeyFrame.cpp:127-161), UpdateConnections
  (:293-383) and EraseConnection with SetBadFlag's walk (:557-571, :470-471, :480-481) over KeyFrame / MapPoint objects whose maps are Python
  dicts iterated in key order.  It knows no capacity.  The one stated difference of the contract is in it: a row the keyframe's run lists more
  than once is walked once.
* run_restated: the parallel form the kernels implement, over the arrays of jsorb_covisibility, with the capacity rule: counts from the runs
  alone, then per slot a base (K of its own update as member q, or its stored map), the AddConnections of the members behind q, and the full
  re-sort exactly when one of them changed the map.  `mutant` breaks it in one named way; each mutant must fail a named case.
* a world: the graph's arrays (state, order_key, point runs, registered or None), the table's bad bytes, C, the state before (zeros, or what a
  `before` script left), first_connection, and a script of steps ("update", slots) / ("erase", slot).  A result per step: the arrays of ALL
  slots (entries at and behind a length are 0), the neighbours table, and for an update parent_out, the snapshot and counts."""
import zlib

import numpy as np

S, N_ROWS, POOL = 96, 320, 96 * 100
TH, NEIGH, MAX_UPDATE = 15, 10, 32
CAPS = ((16, 2048), (16, 24))                    # the bounds on conn_capacity of the shipped library and of tiny_covis (jetson_slam_amd/build.py)
COUNTS = ("n_processed", "n_skipped", "n_empty", "n_add_connection", "n_resorted", "n_fallback", "n_overflow")
UNTOUCHED = -7                                   # what the neighbours table holds before the first step
MUTANTS = {                                      # name -> the case it must fail
    "threshold_14": "counts_14_15_16",
    "tie_by_highest_key": "fallback_tie_by_key_then_slot",
    "no_early_return": "unchanged_weight_keeps_the_list",
    "own_list_is_the_whole_map": "counts_14_15_16",
    "earlier_members_still_applied": "member_targeted_by_an_earlier_member",
    "equal_weights_ascending": "equal_weights_by_key_then_slot",
}


def run_ok(off, length, entries):
    return off >= 0 and length >= 0 and off + length <= entries


def usable(G, s):
    return 0 <= s < len(G["state"]) and G["state"][s] != 0


def valid_run(G, s):
    return run_ok(int(G["point_off"][s]), int(G["point_len"][s]), len(G["point_pool"]))


def run_of(G, s):
    return [int(r) for r in G["point_pool"][G["point_off"][s]:G["point_off"][s] + G["point_len"][s]]]


def empty_state(n_slots, C):
    z = lambda *shape: np.zeros(shape, np.int32)
    return dict(conn_len=z(n_slots), conn_slot=z(n_slots, C), conn_weight=z(n_slots, C), ord_len=z(n_slots), ord_slot=z(n_slots, C),
                ord_weight=z(n_slots, C), first_connection=np.zeros(n_slots, np.uint8), neighbours=np.full((n_slots, NEIGH), UNTOUCHED, np.int32))


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def normalised(st):
    """entries at and behind a length carry no meaning: 0"""
    out = copy_state(st)
    C = out["conn_slot"].shape[1]
    for ln, arrs in (("conn_len", ("conn_slot", "conn_weight")), ("ord_len", ("ord_slot", "ord_weight"))):
        behind = np.arange(C)[None, :] >= out[ln][:, None]
        for a in arrs:
            out[a][behind] = 0
    return out


# ---------------------------------------------------------------- the reference's functions, literally
class MapPoint:
    def __init__(self, bad):
        self.bad, self.observations, self._sorted = bool(bad), [], None

    def isBad(self):
        return self.bad

    def GetObservations(self):
        if self._sorted is None or len(self._sorted) != len(self.observations):
            self._sorted = sorted(self.observations, key=lambda kf: (kf.key, kf.slot))   # std::map<KeyFrame*, size_t>; an entry per registered entry
        return self._sorted


class KeyFrame:
    def __init__(self, slot, key):
        self.slot, self.key = slot, int(key)
        self.mvpMapPoints = []
        self.mConnectedKeyFrameWeights = {}      # KeyFrame -> weight, iterated through items_in_key_order
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [], []
        self.mbFirstConnection, self.mpParent = False, None
        self.list_from = None                    # what wrote the ordered list last in this call: "own" or "best"

    def order(self):
        return (self.key, self.slot)

    def items_in_key_order(self):
        return sorted(self.mConnectedKeyFrameWeights.items(), key=lambda kv: kv[0].order())

    def AddConnection(self, pKF, weight):        # :127-140
        if pKF not in self.mConnectedKeyFrameWeights:
            self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight:
            self.mConnectedKeyFrameWeights[pKF] = weight
        else:
            return False
        self.UpdateBestCovisibles()
        return True

    def UpdateBestCovisibles(self):              # :142-161
        vPairs = [(w, kf) for kf, w in self.items_in_key_order()]
        vPairs.sort(key=lambda p: (p[0], p[1].order()))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs
        self.list_from = "best"

    def UpdateConnections(self, tally):          # :293-383
        KFcounter = {}
        seen = set()
        for pMP in self.mvpMapPoints:
            if pMP is None:
                continue
            if id(pMP) in seen:                  # the stated difference: a row listed twice counts once
                continue
            seen.add(id(pMP))
            if pMP.isBad():
                continue
            for kf in pMP.GetObservations():
                if kf.slot == self.slot:
                    continue
                KFcounter[kf] = KFcounter.get(kf, 0) + 1
        if not KFcounter:
            tally["n_empty"] += 1
            return False
        nmax, pKFmax, th = 0, None, TH
        vPairs = []
        for kf, n in sorted(KFcounter.items(), key=lambda kv: kv[0].order()):
            if n > nmax:
                nmax, pKFmax = n, kf
            if n >= th:
                vPairs.append((n, kf))
                tally["n_add_connection"] += 1
                tally["n_early"] += not kf.AddConnection(self, n)
        if not vPairs:
            vPairs.append((nmax, pKFmax))
            tally["n_add_connection"] += 1
            tally["n_fallback"] += 1
            tally["n_early"] += not pKFmax.AddConnection(self, nmax)
        vPairs.sort(key=lambda p: (p[0], p[1].order()))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            lKFs.insert(0, kf)
            lWs.insert(0, w)
        self.mConnectedKeyFrameWeights = dict(KFcounter)
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs
        self.list_from = "own"
        if self.mbFirstConnection:               # (the byte is mbFirstConnection && mnId != 0)
            self.mpParent = self.mvpOrderedConnectedKeyFrames[0]
            self.mbFirstConnection = False
            return True
        return False

    def EraseConnection(self, pKF):              # :557-571
        if pKF in self.mConnectedKeyFrameWeights:
            del self.mConnectedKeyFrameWeights[pKF]
            self.UpdateBestCovisibles()
            return True
        return False


def _objects(world, state):
    G, bad = world["G"], world["bad"]
    n_slots = len(G["state"])
    kfs = {s: KeyFrame(s, G["order_key"][s]) for s in range(n_slots)}       # an object per slot: a stored map may name any slot
    points = [MapPoint(b) for b in bad]
    for s, kf in kfs.items():
        if usable(G, s) and valid_run(G, s):
            off = int(G["point_off"][s])
            for j, r in enumerate(run_of(G, s)):
                ok = 0 <= r < len(bad)
                kf.mvpMapPoints.append(points[r] if ok else None)
                if ok and (G["registered"] is None or G["registered"][off + j]):
                    points[r].observations.append(kf)
    for s, kf in kfs.items():
        kf.mbFirstConnection = bool(state["first_connection"][s])
        for j in range(int(state["conn_len"][s])):
            kf.mConnectedKeyFrameWeights[kfs[int(state["conn_slot"][s, j])]] = int(state["conn_weight"][s, j])
        for j in range(int(state["ord_len"][s])):
            kf.mvpOrderedConnectedKeyFrames.append(kfs[int(state["ord_slot"][s, j])])
            kf.mvOrderedWeights.append(int(state["ord_weight"][s, j]))
    return kfs


def _arrays(kfs, state, C):
    """the objects back into arrays wide enough for the largest map (the literal form knows no capacity)"""
    n_slots = len(kfs)
    width = max([C] + [len(kf.mConnectedKeyFrameWeights) for kf in kfs.values()])
    out = empty_state(n_slots, width)
    out["neighbours"] = state["neighbours"].copy()
    for s, kf in kfs.items():
        items = kf.items_in_key_order()
        out["conn_len"][s] = len(items)
        for j, (o, w) in enumerate(items):
            out["conn_slot"][s, j], out["conn_weight"][s, j] = o.slot, w
        out["ord_len"][s] = len(kf.mvpOrderedConnectedKeyFrames)
        for j, (o, w) in enumerate(zip(kf.mvpOrderedConnectedKeyFrames, kf.mvOrderedWeights)):
            out["ord_slot"][s, j], out["ord_weight"][s, j] = o.slot, w
        out["first_connection"][s] = kf.mbFirstConnection
        if kf.list_from is not None:
            row = [o.slot for o in kf.mvpOrderedConnectedKeyFrames[:NEIGH]]
            out["neighbours"][s] = row + [-1] * (NEIGH - len(row))
    return out


def run_literal(world):
    """the script over objects; the state is rebuilt from arrays between steps only to keep both yardsticks' results in one form"""
    G, C = world["G"], world["C"]
    state = copy_state(world["state"])
    results = []
    for kind, arg in world["script"]:
        kfs = _objects(world, state)
        res = {}
        if kind == "update":
            tally = dict.fromkeys(COUNTS + ("n_early",), 0)
            parent, snap, done = [], [], set()
            for A in arg:
                A = int(A)
                if not (usable(G, A) and valid_run(G, A)) or A in done:
                    tally["n_skipped"] += 1
                    parent.append(-1)
                    snap.append(None)
                    continue
                done.add(A)
                kf = kfs[A]
                empty_before = tally["n_empty"]
                first = kf.UpdateConnections(tally)
                parent.append(kf.mpParent.slot if first else -1)
                if tally["n_empty"] == empty_before:
                    tally["n_processed"] += 1
                    snap.append([(o.slot, w) for o, w in kf.items_in_key_order()])
                else:
                    snap.append(None)
            tally["n_resorted"] = sum(kf.list_from == "best" for kf in kfs.values())
            res = dict(parent_out=np.array(parent, np.int32).reshape(-1), snapshot=snap, counts=np.array([tally[k] for k in COUNTS] + [0], np.int32),
                       n_early=tally["n_early"])
        else:
            A = kfs[int(arg)]
            walked = held = 0
            for o, _ in A.items_in_key_order():  # :470-471
                if o is A:
                    continue
                walked += 1
                held += o.EraseConnection(A)
            A.mConnectedKeyFrameWeights, A.mvpOrderedConnectedKeyFrames, A.mvOrderedWeights = {}, [], []      # :480-481
            A.list_from = "best"
            res = dict(counts=np.array([walked, held], np.int32))
        state = _arrays(kfs, state, C)
        res["state"] = normalised(state)
        results.append(res)
    return results


# ---------------------------------------------------------------- the parallel form, with the capacity rule
def _key(G, s):
    return (int(G["order_key"][s]), int(s))


def _ord_sorted(G, items, ascending_ties=False):
    """(slot, weight) pairs by (weight, key, slot) descending"""
    if ascending_ties:
        return sorted(items, key=lambda it: (-it[1], _key(G, it[0])))
    return sorted(items, key=lambda it: (it[1], _key(G, it[0])), reverse=True)


def _write(state, s, conn=None, ordered=None):
    C = state["conn_slot"].shape[1]
    if conn is not None:
        conn = conn[:C]
        state["conn_len"][s] = len(conn)
        for j, (o, w) in enumerate(conn):
            state["conn_slot"][s, j], state["conn_weight"][s, j] = o, w
    if ordered is not None:
        ordered = ordered[:C]
        state["ord_len"][s] = len(ordered)
        for j, (o, w) in enumerate(ordered):
            state["ord_slot"][s, j], state["ord_weight"][s, j] = o, w
        row = [o for o, _ in ordered[:NEIGH]]
        state["neighbours"][s] = row + [-1] * (NEIGH - len(row))


def _stored(state, s, n_slots):
    n = min(max(int(state["conn_len"][s]), 0), state["conn_slot"].shape[1])
    return [(int(state["conn_slot"][s, j]), int(state["conn_weight"][s, j])) for j in range(n) if 0 <= state["conn_slot"][s, j] < n_slots]


def update_restated(world, state, slots, mutant=None):
    G, bad, C = world["G"], world["bad"], world["C"]
    n_slots, th = len(G["state"]), 14 if mutant == "threshold_14" else TH
    tally = dict.fromkeys(COUNTS + ("n_early",), 0)
    # the members and their rows
    members, rows = [], []
    for i, A in enumerate(int(a) for a in slots):
        ok = usable(G, A) and valid_run(G, A) and A not in [int(a) for a in slots[:i]]
        members.append(A if ok else -1)
        rows.append({r for r in run_of(G, A) if 0 <= r < len(bad) and not bad[r]} if ok else set())
    # the counts: from the runs alone
    count = np.zeros((len(slots), n_slots), np.int64)
    holders = {}                                 # row -> the members whose rows() hold it
    for i, rs in enumerate(rows):
        for r in rs:
            holders.setdefault(r, []).append(i)
    for B in range(n_slots):
        if not (usable(G, B) and valid_run(G, B)):
            continue
        off = int(G["point_off"][B])
        for j, r in enumerate(run_of(G, B)):
            if G["registered"] is None or G["registered"][off + j]:
                for i in holders.get(r, ()):
                    if members[i] != B:
                        count[i, B] += 1
    # per member: K in key order, T, the fallback
    K, T, parent, snap = {}, {}, [], []
    for i, A in enumerate(members):
        if A < 0:
            tally["n_skipped"] += 1
            parent.append(-1)
            snap.append(None)
            continue
        k = sorted([(B, int(count[i, B])) for B in range(n_slots) if count[i, B] > 0], key=lambda it: _key(G, it[0]))
        if not k:
            tally["n_empty"] += 1
            members[i] = -1
            parent.append(-1)
            snap.append(None)
            continue
        t = [it for it in k if it[1] >= th]
        if not t:
            best = max(w for _, w in k)
            ties = [it for it in k if it[1] == best]
            t = [ties[-1] if mutant == "tie_by_highest_key" else ties[0]]
            tally["n_fallback"] += 1
        K[i], T[i] = k, t
        tally["n_processed"] += 1
        tally["n_add_connection"] += len(t)
        front = _ord_sorted(G, t)[0][0]
        parent.append(front if state["first_connection"][A] else -1)
        state["first_connection"][A] = 0
        snap.append(k[:C])
    # per slot: the base, the connections that reach it, the re-sort
    for B in range(n_slots):
        q = members.index(B) if B in members else -1
        start = 0 if mutant == "earlier_members_still_applied" else q + 1
        incoming = [(members[j], dict(T[j])[B]) for j in range(start, len(members)) if members[j] >= 0 and j != q and B in dict(T[j])]
        if q < 0 and not incoming:
            continue
        full = dict(K[q]) if q >= 0 else dict(_stored(state, B, n_slots))       # what AddConnection compares against
        base = dict(K[q][:C]) if q >= 0 else dict(full)
        changed, n_new = False, 0
        for A, w in incoming:
            if A in full and full[A] == w:
                tally["n_early"] += 1
                continue
            changed = True
            n_new += A not in full
            if A in base or A not in full:
                base[A] = w
        if mutant == "no_early_return" and incoming:
            changed = True
        if q < 0 and not changed:
            continue
        merged = sorted(base.items(), key=lambda it: _key(G, it[0]))
        if (len(full) + n_new if q >= 0 else len(merged)) > C:
            tally["n_overflow"] += 1
        conn = merged[:C]
        if changed:
            tally["n_resorted"] += 1
            _write(state, B, conn, _ord_sorted(G, conn, mutant == "equal_weights_ascending"))
        else:
            own = K[q] if mutant == "own_list_is_the_whole_map" else T[q]
            _write(state, B, conn, _ord_sorted(G, own, mutant == "equal_weights_ascending"))
    return dict(parent_out=np.array(parent, np.int32).reshape(-1), snapshot=snap, counts=np.array([tally[k] for k in COUNTS] + [0], np.int32),
                n_early=tally["n_early"])


def erase_restated(world, state, slot):
    G = world["G"]
    n_slots, walked, held = len(G["state"]), 0, 0
    seen = set()
    for B, _ in _stored(state, slot, n_slots):
        if B == slot or B in seen:
            continue
        seen.add(B)
        walked += 1
        mine = _stored(state, B, n_slots)
        if slot not in dict(mine):
            continue
        held += 1
        conn = sorted([it for it in mine if it[0] != slot], key=lambda it: _key(G, it[0]))
        _write(state, B, conn, _ord_sorted(G, conn))
    _write(state, slot, [], [])
    return dict(counts=np.array([walked, held], np.int32))


def run_restated(world, mutant=None):
    state = copy_state(world["state"])
    results = []
    for kind, arg in world["script"]:
        res = update_restated(world, state, [int(a) for a in arg], mutant) if kind == "update" else erase_restated(world, state, int(arg))
        res["state"] = normalised(state)
        results.append(res)
    return results


def same(a, b, what=""):
    """two yardsticks' results, step by step; arrays of different widths agree when the wider one's surplus is 0"""
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["counts"], y["counts"]), (what, i, x["counts"], y["counts"])
        for k in x["state"]:
            u, v = x["state"][k], y["state"][k]
            if u.ndim == 2 and u.shape[1] != v.shape[1]:
                w = max(u.shape[1], v.shape[1])
                u, v = (np.pad(t, ((0, 0), (0, w - t.shape[1]))) for t in (u, v))
            assert np.array_equal(u, v), (what, i, k, np.argwhere(u != v)[:4].tolist())
        if "parent_out" in x:
            assert np.array_equal(x["parent_out"], y["parent_out"]), (what, i, "parent_out")
            assert x["snapshot"] == y["snapshot"], (what, i, "snapshot")


def overflowed(results):
    return any("parent_out" in r and r["counts"][6] for r in results)


# ---------------------------------------------------------------- worlds
class Builder:
    """keyframes over rows handed out front to back: share(a, b, n) gives both n rows of their own"""

    def __init__(self, C=24, n_slots=S, keys=None, registered=False):
        self.C, self.n_slots = C, n_slots
        self.runs = {s: [] for s in range(n_slots)}
        self.reg = {s: [] for s in range(n_slots)} if registered else None
        self.state = np.zeros(n_slots, np.uint8)
        self.keys = np.arange(n_slots, dtype=np.int64) * 16 + 4096 if keys is None else np.asarray(keys, np.int64)
        self.bad = np.zeros(N_ROWS, np.uint8)
        self.next_row = 0
        self.before, self.script = [], []
        self.first = np.zeros(n_slots, np.uint8)
        self.off_override, self.len_override = {}, {}

    def kf(self, *slots, state=1):
        for s in slots:
            self.state[s] = state
        return self

    def fresh(self, n):
        r = list(range(self.next_row, self.next_row + n))
        self.next_row += n
        assert self.next_row <= N_ROWS
        return r

    def add(self, s, rows, registered=1):
        self.kf(s, state=self.state[s] or 1)
        self.runs[s] += list(rows)
        if self.reg is not None:
            self.reg[s] += [registered] * len(rows)
        return self

    def share(self, a, b, n, reg_a=1, reg_b=1):
        rows = self.fresh(n)
        self.add(a, rows, reg_a)
        self.add(b, rows, reg_b)
        return rows

    def world(self, name):
        off, ln, pool, reg = np.zeros(self.n_slots, np.int32), np.zeros(self.n_slots, np.int32), [], []
        for s in range(self.n_slots):
            off[s], ln[s] = len(pool), len(self.runs[s])
            pool += self.runs[s]
            if self.reg is not None:
                reg += self.reg[s]
        for s, v in self.off_override.items():
            off[s] = v
        for s, v in self.len_override.items():
            ln[s] = v
        assert len(pool) <= POOL and max(len(r) for r in self.runs.values()) <= 100
        pool_a = np.full(POOL, -1, np.int32)
        pool_a[:len(pool)] = pool
        reg_a = None
        if self.reg is not None:
            reg_a = np.ones(POOL, np.uint8)
            reg_a[:len(reg)] = reg
        G = dict(state=self.state.copy(), order_key=self.keys.copy(), point_off=off, point_len=ln, point_pool=pool_a, registered=reg_a)
        w = dict(name=name, G=G, bad=self.bad.copy(), C=self.C, script=list(self.before), state=empty_state(self.n_slots, self.C))
        w["state"]["first_connection"][:] = self.first
        if self.before:                          # the state the world starts from is what `before` leaves (no overflow there)
            left = run_restated(w)[-1]["state"]
            assert not overflowed(run_restated(w))
            left["neighbours"][:] = UNTOUCHED
            w["state"] = left
        w["script"] = list(self.script)
        return w


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


@case
def counts_14_15_16():
    b = Builder()
    for other, n in ((1, 14), (2, 15), (3, 16)):
        b.share(0, other, n)
    b.script = [("update", [0])]
    return b.world("counts_14_15_16"), dict(ord_of={0: [3, 2]}, conn_of={0: [1, 2, 3], 1: [], 2: [0]})


@case
def fallback_tie_by_key_then_slot():
    # no count reaches the threshold; 7 is shared with slots 5 and 2 (equal keys, so by slot) and with slot 9 whose key is lower still
    keys = np.arange(S, dtype=np.int64) * 16 + 4096
    keys[5] = keys[2] = 900
    keys[9] = 100
    b = Builder(keys=keys)
    for other, n in ((5, 7), (2, 7), (11, 6)):
        b.share(0, other, n)
    b.share(20, 9, 7)
    b.share(20, 5, 7)
    b.share(20, 2, 7)
    b.script = [("update", [0]), ("update", [20])]
    return b.world("fallback_tie_by_key_then_slot"), dict(ord_of={0: [2], 20: [9], 2: [0], 9: [20], 5: []}, counts={5: 1})


@case
def equal_weights_by_key_then_slot():
    keys = np.arange(S, dtype=np.int64) * 16 + 4096
    keys[4] = keys[6] = 5000                     # equal keys: by slot
    b = Builder(keys=keys)
    for other in (1, 4, 6, 8):
        b.share(0, other, 18)
    b.share(0, 3, 19)
    b.script = [("update", [0])]
    return b.world("equal_weights_by_key_then_slot"), dict(ord_of={0: [3, 6, 4, 8, 1]})


@case
def unchanged_weight_keeps_the_list():
    # after the first two steps slots 1 and 2 each hold the thresholded list [3, 0] and a map {0, 3: 20, 4: 5}.  cnt(0, 1) = cnt(1, 0) = 15, but
    # cnt(0, 2) = 16 while cnt(2, 0) = 17 (a row both list, registered in 0's run only).  Then 0 is updated again: towards 1 its weight is
    # unchanged (the early return: 1's list must NOT grow to the whole map), towards 2 it differs (2's list becomes its whole map)
    b = Builder(registered=True)
    for t in (1, 2):
        b.share(t, 3, 20)
        b.share(t, 4, 5)
    b.share(0, 1, 15)
    b.share(0, 2, 16)
    b.share(0, 2, 1, reg_a=1, reg_b=0)
    b.script = [("update", [0]), ("update", [1, 2]), ("update", [0])]
    return b.world("unchanged_weight_keeps_the_list"), dict(ord_of={1: [3, 0], 2: [3, 0, 4]}, min_early=1, counts={4: 1})


@case
def member_targeted_by_a_later_member():
    b = Builder()
    b.share(0, 1, 16)
    b.share(0, 2, 3)
    b.share(1, 2, 18)
    b.before = [("update", [2])]                 # 2's update leaves 0 out of the lists of 0's own view: 0 holds nothing yet
    b.script = [("update", [0, 1])]              # 1, behind 0, adds itself to 0 with the weight 0's own update already gave: no re-sort
    return b.world("member_targeted_by_a_later_member"), dict(ord_of={0: [1], 1: [2, 0]})


@case
def member_targeted_by_an_earlier_member():
    # 0 targets 1 with cnt(0, 1) = 15 while cnt(1, 0) = 17 (two rows both list, registered in 0's run only): 1's own update behind it
    # overwrites the connection, and nothing of 0's AddConnection is left
    b = Builder(registered=True)
    b.share(0, 1, 15)
    b.share(0, 1, 2, reg_a=1, reg_b=0)           # rows both list; 1's entries are not registered: cnt(0, 1) = 15, cnt(1, 0) = 17
    b.share(1, 2, 4)
    b.script = [("update", [0, 1])]
    return b.world("member_targeted_by_an_earlier_member"), dict(ord_of={1: [0], 0: [1]}, weight={(1, 0): 17, (0, 1): 17}, conn_of={1: [0, 2]})


@case
def repeated_member():
    b = Builder()
    b.share(0, 1, 15)
    b.script = [("update", [0, 1, 0])]
    return b.world("repeated_member"), dict(counts={0: 2, 1: 1}, parent=[-1, -1, -1])


@case
def empty_k():
    b = Builder()
    b.add(0, b.fresh(20))
    b.share(1, 2, 15)
    b.first[0] = 1
    b.script = [("update", [0, 1])]
    return b.world("empty_k"), dict(counts={0: 1, 2: 1}, first={0: 1}, conn_of={0: []})


@case
def first_connection_set_and_clear():
    b = Builder()
    b.share(0, 1, 15)
    b.share(0, 2, 30)
    b.share(3, 1, 16)
    b.first[0] = 1
    b.script = [("update", [0, 3]), ("update", [0])]
    return b.world("first_connection_set_and_clear"), dict(step0=dict(parent=[2, -1]), parent=[-1], first={0: 0, 3: 0})


@case
def run_longer_than_a_wave():
    b = Builder()
    b.share(0, 1, 70)
    b.share(0, 2, 29)
    b.add(1, b.fresh(30))
    b.script = [("update", [0, 1])]
    return b.world("run_longer_than_a_wave"), dict(ord_of={0: [1, 2]}, weight={(0, 1): 70})


@case
def more_than_64_connected():
    b = Builder(C=80)
    rows = b.fresh(20)
    b.add(0, rows)
    for s in range(1, 71):
        b.add(s, rows[:15 + s % 6])
    b.script = [("update", [0]), ("update", [70, 69])]
    return b.world("more_than_64_connected"), dict(conn_len={0: 70})


def _capacity(n_own, C=16):
    b = Builder(C=C)
    rows = b.fresh(4)
    b.add(0, rows)
    for s in range(1, n_own + 1):                # 0's own K: n_own slots, all below the threshold but one
        b.add(s, rows[:3])
    b.share(0, n_own, 15)
    return b


@case
def map_of_exactly_c():
    b = _capacity(16)
    b.script = [("update", [0])]
    return b.world("map_of_exactly_c"), dict(conn_len={0: 16}, counts={6: 0})


@case
def map_of_c_plus_one_by_its_own_update():
    b = _capacity(17)
    b.script = [("update", [0])]
    return b.world("map_of_c_plus_one_by_its_own_update"), dict(conn_len={0: 16}, counts={6: 1})


@case
def map_of_c_plus_one_by_an_incoming_connection():
    b = _capacity(16)
    b.before = [("update", [0])]
    w0 = b.world("before")
    b.share(50, 0, 15)                           # a new keyframe: its rows are 0's too, but 0 is not updated again
    b.before = []
    b.script = [("update", [50])]
    w = b.world("map_of_c_plus_one_by_an_incoming_connection")
    w["state"] = w0["state"]
    return w, dict(conn_len={0: 16}, counts={6: 1})


@case
def registered_bytes():
    b = Builder(registered=True)
    b.share(0, 1, 20, reg_b=1)
    b.share(0, 1, 6, reg_b=0)
    b.share(0, 2, 15, reg_a=0)                   # 0's own bytes are not read
    b.script = [("update", [0])]
    return b.world("registered_bytes"), dict(weight={(0, 1): 20, (0, 2): 15})


@case
def bad_rows_rows_out_of_range_invalid_runs_absent_and_bad_slots():
    b = Builder()
    rows = b.share(0, 1, 20)
    b.bad[rows[:4]] = 1                          # 16 left
    b.add(0, [-1, N_ROWS, N_ROWS + 5, -3])
    b.add(1, [N_ROWS, -1])
    b.share(0, 2, 15)
    b.kf(2, state=2)                             # a bad keyframe still counts (it is in the observations)
    b.share(0, 3, 15)
    b.state[3] = 0                               # absent
    b.share(0, 4, 15)
    b.share(0, 5, 15)
    b.share(6, 1, 15)
    b.share(7, 1, 15)
    b.script = [("update", [0, 4, 5, 6, 7, -1, S, 3])]
    w = b.world("bad_rows_rows_out_of_range_invalid_runs_absent_and_bad_slots")
    w["G"]["point_len"][4] = POOL + 1            # invalid runs: as a target, as a member
    w["G"]["point_off"][6] = -2
    w["G"]["point_off"][7] = POOL - 3
    w["G"]["point_len"][7] = 4
    return w, dict(weight={(0, 1): 16}, conn_of={0: [1, 2, 5]}, counts={1: 6})


@case
def n_update_0():
    b = Builder()
    b.share(0, 1, 15)
    b.script = [("update", [])]
    return b.world("n_update_0"), dict(counts={0: 0, 1: 0})


@case
def n_update_32():
    b = Builder(C=48)
    rows = b.fresh(40)
    for s in range(40):
        b.add(s, rows[s % 7:s % 7 + 14 + s % 9])
    b.first[1:40] = 1
    b.script = [("update", list(range(31, -1, -1))), ("update", list(range(8, 40)))]
    return b.world("n_update_32"), dict(counts={0: 32})


@case
def erase_with_an_asymmetric_map():
    b = Builder()
    b.share(0, 1, 20)
    b.share(0, 2, 5)
    b.share(0, 3, 16)
    b.share(3, 4, 17)
    b.before = [("update", [0]), ("update", [3])]
    # 0's map holds 1, 2 and 3; 2's map does not hold 0 (below the threshold, and 2 was never updated): left alone, lists included
    b.script = [("erase", 0), ("erase", 0), ("update", [3])]
    return b.world("erase_with_an_asymmetric_map"), dict(step0=dict(erase_counts=[3, 2], conn_of={0: []}), conn_of={0: [3], 2: []}, ord_of={3: [4, 0], 1: []})


def build_case(name):
    world, expect = CASES[name]()
    world["name"] = name
    return world, expect


def random_world(seed):
    """keyframes in a few clusters of rows, so that counts lie on both sides of the threshold; a script of updates (some repeating a slot of an
    earlier step: the early return) and erases.  Every fourth seed has C = 16 and overflows now and then; the others cannot (C = S)."""
    rng = np.random.RandomState(zlib.crc32(b"covis%d" % seed))
    C = 16 if seed % 4 == 0 else S
    keys = rng.permutation(S).astype(np.int64) * 8 + 1000
    if seed % 3 == 0:
        keys[rng.choice(S, 10, replace=False)] = 1000 + 8 * int(rng.randint(S))
    b = Builder(C=C, keys=keys, registered=seed % 2 == 1)
    n_kf = int(rng.randint(12, 60))
    slots = rng.choice(S, n_kf, replace=False)
    n_clusters = int(rng.randint(2, 6))
    width = N_ROWS // n_clusters
    for s in slots:
        c = int(rng.randint(n_clusters))
        n = int(rng.randint(1, 60))
        rows = c * width + rng.choice(width, min(n, width), replace=False)
        if rng.rand() < 0.3:
            rows = np.concatenate([rows, rng.choice(N_ROWS, int(rng.randint(1, 30)), replace=False)])
            rows = np.unique(rows)[:100]
            rng.shuffle(rows)
        b.add(int(s), [int(r) for r in rows])
        if b.reg is not None:
            b.reg[int(s)] = [int(x) for x in (rng.rand(len(rows)) < 0.85)]
        b.state[s] = 1 if rng.rand() < 0.9 else 2
    b.bad[rng.choice(N_ROWS, 20, replace=False)] = 1
    b.first[:] = rng.rand(S) < 0.5
    script = []
    for _ in range(int(rng.randint(3, 7))):
        if rng.rand() < 0.2:
            script.append(("erase", int(rng.choice(slots))))
        else:
            n = int(rng.choice([1, 2, 5, 32, int(rng.randint(1, 33))]))
            pick = [int(x) for x in rng.choice(slots, min(n, n_kf), replace=False)]
            if rng.rand() < 0.3 and pick:
                pick.append(pick[0])
            if rng.rand() < 0.2:
                pick.insert(0, int(rng.randint(-2, S + 2)))
            script.append(("update", pick[:MAX_UPDATE]))
    b.script = script
    return b.world("random_%d" % seed)


GOLDEN_SEEDS = tuple(s for s in range(40) if s % 4 != 0)[:24]      # the recorded worlds: none can overflow
GOLDEN_CASES = ("counts_14_15_16", "fallback_tie_by_key_then_slot", "equal_weights_by_key_then_slot", "unchanged_weight_keeps_the_list",
                "member_targeted_by_a_later_member", "first_connection_set_and_clear", "more_than_64_connected", "n_update_32",
                "erase_with_an_asymmetric_map", "run_longer_than_a_wave")


def golden_worlds():
    for n in GOLDEN_CASES:
        yield build_case(n)[0]
    for s in GOLDEN_SEEDS:
        yield random_world(s)


def check_expect(results, expect):
    """what a case is named for, on its last step (and on its first under `step0`)"""
    def apply(res, e):
        st = res["state"]
        for s, want in e.get("ord_of", {}).items():
            assert st["ord_slot"][s, :st["ord_len"][s]].tolist() == want, ("ord", s, st["ord_slot"][s, :st["ord_len"][s]].tolist(), want)
        for s, want in e.get("conn_of", {}).items():
            assert st["conn_slot"][s, :st["conn_len"][s]].tolist() == want, ("conn", s, st["conn_slot"][s, :st["conn_len"][s]].tolist(), want)
        for s, want in e.get("conn_len", {}).items():
            assert st["conn_len"][s] == want, ("conn_len", s, int(st["conn_len"][s]), want)
        for (s, o), want in e.get("weight", {}).items():
            have = dict(zip(st["conn_slot"][s, :st["conn_len"][s]].tolist(), st["conn_weight"][s, :st["conn_len"][s]].tolist()))
            assert have.get(o) == want, ("weight", s, o, have)
        for i, want in e.get("counts", {}).items():
            assert res["counts"][i] == want, ("counts", i, res["counts"].tolist(), want)
        for s, want in e.get("first", {}).items():
            assert st["first_connection"][s] == want, ("first_connection", s)
        if "parent" in e:
            assert res["parent_out"].tolist() == e["parent"], ("parent_out", res["parent_out"].tolist())
        if "erase_counts" in e:
            assert res["counts"].tolist() == e["erase_counts"], ("erase counts", res["counts"].tolist())
        if "min_early" in e and "n_early" in res:
            assert res["n_early"] >= e["min_early"], ("n_early", res["n_early"])
    apply(results[-1], {k: v for k, v in expect.items() if k != "step0"})
    if "step0" in expect:
        apply(results[0], expect["step0"])


# ---------------------------------------------------------------- the recorded worlds: the reference's own src/KeyFrame.cpp (tools/ref_covis)
GOLDEN_KEYS = ("lens", "wide", "parent_out", "crc")       # lens[step][5][S]: conn_len, ord_len, first_connection, parent, child_len;
                                                          # wide[step][5][S][W]: conn_slot, conn_weight, ord_slot, ord_weight, child_slot


def _root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_path():
    import os
    return os.path.join(_root(), "tests", "golden", "ref_matcher_covis.npz")


def reference_tree():
    """the reference tree, or None where it is absent"""
    import os
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if os.path.exists(os.path.join(ref, "src", "KeyFrame.cpp")) else None


def driver_path():
    import os
    return os.path.join(_root(), "oracle", "_ref", "ref_covis")


STAND_INS = ("Frame.h", "MapPoint.h", "Map.h", "KeyFrameDatabase.h", "Converter.h", "ORBmatcher.h", "ORBextractor.h", "ORBVocabulary.h")


def build_driver(reference):
    """the reference's src/KeyFrame.cpp with its include/KeyFrame.h, unmodified, with tools/ref_covis's stand-ins force-included so that their
    guards shut out the reference's headers of the same names"""
    import os
    import subprocess
    shadow = os.path.join(_root(), "tools", "ref_covis")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-w", "-I" + shadow, "-I" + os.path.join(reference, "include"), "-I" + reference]
    for h in STAND_INS:
        cmd += ["-include", os.path.join(shadow, h)]
    dbow = os.path.join(reference, "Thirdparty", "DBoW2", "DBoW2")       # (KeyFrame holds a BowVector and a FeatureVector)
    cmd += ["-o", driver_path(), os.path.join(shadow, "driver.cpp"), os.path.join(reference, "src", "KeyFrame.cpp"), os.path.join(dbow, "BowVector.cpp"),
            os.path.join(dbow, "FeatureVector.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    return driver_path()


def world_bytes(w):
    """the driver's input, which is also what `crc` is taken over"""
    G, st, C = w["G"], w["state"], w["C"]
    n_slots = len(G["state"])
    reg = np.ones(len(G["point_pool"]), np.int32) if G["registered"] is None else G["registered"].astype(np.int32)
    kind, start, args = [], [0], []
    for k, a in w["script"]:
        kind.append(0 if k == "update" else 1)
        args += [int(x) for x in a] if k == "update" else [int(a)]
        start.append(len(args))
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()
    parts = [i32([n_slots, len(w["bad"]), len(G["point_pool"]), C, len(kind), len(args)]), i32(G["state"]), np.ascontiguousarray(G["order_key"], np.int64).tobytes(),
             i32(G["point_off"]), i32(G["point_len"]), i32(G["point_pool"]), i32(reg), i32(w["bad"]), i32(st["first_connection"])]
    parts += [i32(st[k]) for k in ("conn_len", "conn_slot", "conn_weight", "ord_len", "ord_slot", "ord_weight")]
    parts += [i32(kind), i32(start), i32(args)]
    return b"".join(parts)


def run_driver(w, workdir):
    """a world through the reference -> dict of GOLDEN_KEYS"""
    import os
    import subprocess
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    raw_in = world_bytes(w)
    with open(src, "wb") as f:
        f.write(raw_in)
    subprocess.check_call([driver_path(), src, dst], timeout=120)
    n_slots, C, n = len(w["G"]["state"]), w["C"], len(w["script"])
    raw = np.fromfile(dst, np.int32)
    per = 5 * n_slots + 5 * n_slots * C + 32
    assert len(raw) == n * per
    raw = raw.reshape(n, per)
    lens = raw[:, :5 * n_slots].reshape(n, 5, n_slots)
    wide = raw[:, 5 * n_slots:5 * n_slots + 5 * n_slots * C].reshape(n, 5, n_slots, C)
    width = max(1, int(lens[:, [0, 1, 4]].max()))
    assert not wide[..., width:].any()
    return dict(lens=lens.copy(), wide=wide[..., :width].copy(), parent_out=raw[:, -32:].copy(), crc=np.array(zlib.crc32(raw_in), np.uint32))


def write_golden(recorded):
    """recorded: name -> dict of GOLDEN_KEYS; members in a fixed order with a fixed date, so that the file is reproducible"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w") as z:
        for name, rec in recorded.items():
            for key in GOLDEN_KEYS:
                buf = io.BytesIO()
                np.save(buf, rec[key])
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, key), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


def load_golden():
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, key = member.rsplit(".", 1)
            out.setdefault(name, {})[key] = z[member]
    return out


def same_as_recorded(world, results, rec):
    """a yardstick's (or the device's) results against what the reference left after each step"""
    assert int(rec["crc"]) == zlib.crc32(world_bytes(world)), (world["name"], "the world is not the recorded one")
    assert len(results) == len(rec["lens"]) == len(world["script"])
    W = rec["wide"].shape[-1]
    for t, (res, (kind, arg)) in enumerate(zip(results, world["script"])):
        st = res["state"]
        for i, k in ((0, "conn_len"), (1, "ord_len"), (2, "first_connection")):
            assert np.array_equal(st[k], rec["lens"][t, i]), (world["name"], t, k)
        for i, k in enumerate(("conn_slot", "conn_weight", "ord_slot", "ord_weight")):
            assert not st[k][:, W:].any() and np.array_equal(st[k][:, :W], rec["wide"][t, i][:, :st[k].shape[1]]), (world["name"], t, k)
        if kind == "update":
            assert np.array_equal(res["parent_out"], rec["parent_out"][t, :len(arg)]), (world["name"], t, "parent_out")
            assert (rec["parent_out"][t, len(arg):] == -2).all()
