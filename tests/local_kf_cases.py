"""Cases and restatements for jsorb_local_keyframes (include/jsorb.h), shared by tests/test_local_kf_host.py and tests/test_gpu_local_kf.py.
numpy only: nothing here needs a GPU.  Not a test module.

* update_local_keyframes_restated: a literal transcription of Tracking::UpdateLocalKeyFrames (Tracking.cpp:1844-1952) over KeyFrame / MapPoint
  objects with the reference's own fields (mnTrackReferenceForFrame, an observations container ordered by key, a child set ordered by key,
  GetBestCovisibilityKeyFrames, GetParent, isBad), with the early return, the end iterator taken once and the break that leaves the outer loop;
  then the contract's gather.  The observations are built from the graph's runs and `registered`; a run that lists a row twice puts the keyframe
  twice into that point's container (the contract counts it twice - a std::map could not hold it).  An unusable slot reference has no object.
* update_local_keyframes_numpy: the same from array operations.
* the cases: graphs of S slots over a table of N_ROWS rows, each a list of steps (a step = the graph's arrays, the table's bad bytes, the frame's
  rows) run one after the other with the persistent list, and what the case is named for in `expect`, a subset of the stats."""
import zlib

import numpy as np

S, N_ROWS, POOL, CHILD_POOL = 128, 512, 128 * 40 + 64, 1024
BAD_ROWS = np.arange(480, N_ROWS)                # the table's bad rows; rows 0 .. S-1: row s is slot s's own point; 128 .. 479 filler
CAPS = ((32768, 4096), (64, 16))                 # LK_MEMBER_LDS, LK_CHILD_LDS of the shipped library and of tiny_local_kf (jetson_slam_amd/build.py)
COUNTS = ("n_counter", "n_first", "n_local", "ref_slot", "E_total", "kf_overflow", "entry_overflow", "kept_previous")
STATS = ("n_counter", "n_first", "n_local", "n_neighbours", "n_children", "n_parents", "n_invalid_runs", "end_reason")
LIMIT = 80


def run_ok(off, length, entries):
    return off >= 0 and length >= 0 and off + length <= entries


# ---------------------------------------------------------------- the reference's loops, literally
class MapPoint:
    def __init__(self, row, bad):
        self.row, self.bad, self.observations = row, bool(bad), []

    def isBad(self):
        return self.bad

    def GetObservations(self):
        return sorted(self.observations, key=lambda kf: (kf.key, kf.slot))       # std::map<KeyFrame*, size_t>


class KeyFrame:
    def __init__(self, slot, key, state):
        self.slot, self.key, self.bad = slot, int(key), state != 1
        self.mnTrackReferenceForFrame = 0
        self.neighbours, self.children, self.parent, self.matches = [], [], None, []

    def isBad(self):
        return self.bad

    def GetBestCovisibilityKeyFrames(self, n):
        return self.neighbours[:n]

    def GetChilds(self, by_slot=False):
        return sorted(set(self.children), key=lambda kf: kf.slot if by_slot else (kf.key, kf.slot))      # std::set<KeyFrame*>

    def GetParent(self):
        return self.parent


def build_objects(G, bad):
    """the map the arrays describe: KeyFrame objects for the usable slots, MapPoint objects with their observations"""
    n_slots = len(G["state"])
    kfs = {s: KeyFrame(s, G["order_key"][s], int(G["state"][s])) for s in range(n_slots) if G["state"][s] != 0}
    points = [MapPoint(r, bad[r]) for r in range(len(bad))]
    n_invalid = 0
    for s, kf in kfs.items():
        off, ln = int(G["point_off"][s]), int(G["point_len"][s])
        if run_ok(off, ln, len(G["point_pool"])):
            kf.matches = [int(r) for r in G["point_pool"][off:off + ln]]
            for j, r in enumerate(kf.matches):
                if 0 <= r < len(bad) and (G["registered"] is None or G["registered"][off + j]):
                    points[r].observations.append(kf)
        else:
            n_invalid += 1
        kf.neighbours = [kfs[int(c)] for c in G["neighbours"][s] if int(c) in kfs]
        off, ln = int(G["child_off"][s]), int(G["child_len"][s])
        if run_ok(off, ln, len(G["child_pool"])):
            kf.children = [kfs[int(c)] for c in G["child_pool"][off:off + ln] if int(c) in kfs]
        else:
            n_invalid += 1
        kf.parent = kfs.get(int(G["parent"][s]))
    return kfs, points, n_invalid


def gather(G, slots, kf_capacity, entry_capacity):
    """step 6 of the contract over the list `slots`"""
    start = np.zeros(kf_capacity + 1, np.int64)
    rows = []
    for i, s in enumerate(slots):
        ln = 0
        if 0 <= s < len(G["state"]) and G["state"][s] != 0 and run_ok(int(G["point_off"][s]), int(G["point_len"][s]), len(G["point_pool"])):
            ln = int(G["point_len"][s])
            rows.append(G["point_pool"][G["point_off"][s]:G["point_off"][s] + ln])
        start[i + 1] = start[i] + ln
    start[len(slots) + 1:] = start[len(slots)]
    e = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    out = np.full(entry_capacity, -1, np.int32)
    n = min(len(e), entry_capacity)
    out[:n] = e[:n]
    return start.astype(np.int32), out, len(e)


MUTANTS = ("votes_at_least", "end_reevaluated", "size_at_least_80", "parent_bad_tested", "parent_break_inner", "bad_voters_not_counted", "children_slot_order")


def update_local_keyframes_restated(G, bad, frame_rows, kf_capacity, entry_capacity, prev_list=(), prev_ref=-1, frame_id=7, mutant=None):
    """G: the arrays of jsorb_keyframe_graph (numpy; registered may be None); prev_list, prev_ref: mvpLocalKeyFrames (slots) and mpReferenceKF before
    the call.  Returns dict(list, ref_slot, local_kf_start, local_point_row, counts, stats).  mutant: one of MUTANTS, a decision of the reference's
    text flipped (tests/test_ref_tracking.py shows that the recorded reference output notices each)."""
    assert mutant is None or mutant in MUTANTS
    kfs, points, n_invalid = build_objects(G, bad)
    lookup = lambda r: points[r] if 0 <= r < len(points) else None
    mvpMapPoints = [lookup(int(r)) for r in frame_rows] if frame_rows is not None else []
    mvpLocalKeyFrames, mpReferenceKF = None, None
    st = dict.fromkeys(STATS, 0)
    st["n_invalid_runs"] = n_invalid
    overflow = 0

    def walk():
        nonlocal mvpLocalKeyFrames, mpReferenceKF, overflow
        # Each map point vote for the keyframes in which it has been observed (:1846-1864)
        keyframeCounter = {}
        for i in range(len(mvpMapPoints)):
            if mvpMapPoints[i]:
                pMP = mvpMapPoints[i]
                if not pMP.isBad():
                    observations = pMP.GetObservations()
                    for kf in observations:
                        if mutant == "bad_voters_not_counted" and kf.isBad():
                            continue
                        keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
                else:
                    mvpMapPoints[i] = None
        st["n_counter"] = len(keyframeCounter)
        if not keyframeCounter:                                              # :1866
            return
        maxv, pKFmax = 0, None
        mvpLocalKeyFrames = []
        for pKF, votes in sorted(keyframeCounter.items(), key=lambda it: (it[0].key, it[0].slot)):      # :1876-1891, std::map's order
            if pKF.isBad():
                continue
            if votes > maxv or (mutant == "votes_at_least" and votes >= maxv):
                maxv, pKFmax = votes, pKF
            mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = frame_id
        st["n_first"] = len(mvpLocalKeyFrames)
        if len(mvpLocalKeyFrames) > kf_capacity:                             # the contract's cut: a prefix is kept
            del mvpLocalKeyFrames[kf_capacity:]
            overflow = 1
        itEndKF = len(mvpLocalKeyFrames)                                     # taken once
        it = -1
        while True:                                                          # :1895-1945
            it += 1
            if it >= (len(mvpLocalKeyFrames) if mutant == "end_reevaluated" else itEndKF):
                break
            if len(mvpLocalKeyFrames) > LIMIT or (mutant == "size_at_least_80" and len(mvpLocalKeyFrames) >= LIMIT):
                st["end_reason"] = 1
                break
            pKF = mvpLocalKeyFrames[it]
            for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != frame_id:
                        mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = frame_id
                        st["n_neighbours"] += 1
                        break
            for pChildKF in pKF.GetChilds(by_slot=mutant == "children_slot_order"):
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != frame_id:
                        mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = frame_id
                        st["n_children"] += 1
                        break
            pParent = pKF.GetParent()
            if pParent and not (mutant == "parent_bad_tested" and pParent.isBad()):
                if pParent.mnTrackReferenceForFrame != frame_id:
                    mvpLocalKeyFrames.append(pParent)
                    pParent.mnTrackReferenceForFrame = frame_id
                    st["n_parents"] += 1
                    if mutant == "parent_break_inner":
                        continue
                    st["end_reason"] = 2
                    break
        if pKFmax:                                                           # :1947-1951
            mpReferenceKF = pKFmax

    walk()
    kept = mvpLocalKeyFrames is None
    slots = [int(s) for s in prev_list] if kept else [kf.slot for kf in mvpLocalKeyFrames]
    ref = mpReferenceKF.slot if mpReferenceKF else int(prev_ref)
    st["n_local"] = len(slots)
    start, rows, e_total = gather(G, slots, kf_capacity, entry_capacity)
    counts = [st["n_counter"], st["n_first"], len(slots), ref, e_total, overflow, int(e_total > entry_capacity), int(kept)]
    return dict(list=np.array(slots, np.int32), ref_slot=ref, local_kf_start=start, local_point_row=rows, counts=np.array(counts, np.int32), stats=st)


def update_local_keyframes_numpy(G, bad, frame_rows, kf_capacity, entry_capacity, prev_list=(), prev_ref=-1):
    n_slots, n_rows = len(G["state"]), len(bad)
    state = np.asarray(G["state"])
    mult = np.zeros(n_rows, np.int64)
    if frame_rows is not None and len(frame_rows):
        fr = np.asarray(frame_rows, np.int64)
        fr = fr[(fr >= 0) & (fr < n_rows)]
        mult = np.bincount(fr[bad[fr] == 0], minlength=n_rows)
    off, ln = np.asarray(G["point_off"], np.int64), np.asarray(G["point_len"], np.int64)
    p_ok = (off >= 0) & (ln >= 0) & (off + ln <= len(G["point_pool"]))
    coff, cln = np.asarray(G["child_off"], np.int64), np.asarray(G["child_len"], np.int64)
    c_ok = (coff >= 0) & (cln >= 0) & (coff + cln <= len(G["child_pool"]))
    present = state != 0
    vote = np.zeros(n_slots, np.int64)
    for s in np.nonzero(present & p_ok)[0]:
        r = np.asarray(G["point_pool"][off[s]:off[s] + ln[s]], np.int64)
        m = (r >= 0) & (r < n_rows)
        if G["registered"] is not None:
            m &= np.asarray(G["registered"][off[s]:off[s] + ln[s]]) != 0
        vote[s] = mult[r[m]].sum()
    st = dict.fromkeys(STATS, 0)
    st["n_invalid_runs"] = int((present & ~p_ok).sum() + (present & ~c_ok).sum())
    st["n_counter"] = int((vote > 0).sum())
    kept = st["n_counter"] == 0
    slots, ref, overflow = [int(s) for s in prev_list], int(prev_ref), 0
    if not kept:
        first = np.nonzero((state == 1) & (vote > 0))[0]
        first = first[np.lexsort((first, np.asarray(G["order_key"])[first]))]
        st["n_first"] = len(first)
        if len(first):
            ref = int(first[np.argmax(vote[first])])                         # the first of the largest
        overflow = int(len(first) > kf_capacity)
        slots = [int(s) for s in first[:kf_capacity]]
        member = np.zeros(n_slots, bool)
        member[slots] = True
        usable = lambda c: (c >= 0) & (c < n_slots) & present[np.clip(c, 0, n_slots - 1)]
        good = lambda c: usable(c) & (state[np.clip(c, 0, n_slots - 1)] == 1)
        for s in list(slots):
            if len(slots) > LIMIT:
                st["end_reason"] = 1
                break
            for kind, cand in (("n_neighbours", np.asarray(G["neighbours"][s], np.int64)),
                               ("n_children", np.asarray(G["child_pool"][coff[s]:coff[s] + cln[s]], np.int64) if c_ok[s] else np.zeros(0, np.int64))):
                ok = np.nonzero(good(cand) & ~member[np.clip(cand, 0, n_slots - 1)])[0] if len(cand) else []
                if len(ok):
                    c = int(cand[ok[0]])
                    slots.append(c)
                    member[c] = True
                    st[kind] += 1
            p = np.int64(G["parent"][s])
            if usable(p) and not member[p]:
                slots.append(int(p))
                member[p] = True
                st["n_parents"], st["end_reason"] = st["n_parents"] + 1, 2
                break
    st["n_local"] = len(slots)
    start, rows, e_total = gather(G, slots, kf_capacity, entry_capacity)
    counts = [st["n_counter"], st["n_first"], len(slots), ref, e_total, overflow, int(e_total > entry_capacity), int(kept)]
    return dict(list=np.array(slots, np.int32), ref_slot=ref, local_kf_start=start, local_point_row=rows, counts=np.array(counts, np.int32), stats=st)


def run_steps(fn, case):
    """the case's steps one after the other with the persistent list; the results, one per step"""
    prev_list, prev_ref, out = [], -1, []
    for step in case["steps"]:
        r = fn(step["G"], step["bad"], step["frame_rows"], case["kf_capacity"], case["entry_capacity"], prev_list, prev_ref)
        prev_list, prev_ref = r["list"].tolist(), r["ref_slot"]
        out.append(r)
    return out


# ---------------------------------------------------------------- building graphs
class Builder:
    """A graph under construction.  kf(): a keyframe whose run holds its own row (the row = its slot) among filler rows; the frame votes for a
    keyframe by naming that row."""

    def __init__(self, name, expressible=False):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.expressible = expressible               # runs the reference's containers can hold: rows of the table or -1, no row twice in a run
        self.state, self.key = np.zeros(S, np.uint8), np.zeros(S, np.int64)
        self.runs, self.reg, self.children = {}, {}, {}
        self.neigh = np.full((S, 10), -1, np.int32)
        self.parent = np.full(S, -1, np.int32)
        self.bad = np.zeros(N_ROWS, np.uint8)
        self.bad[BAD_ROWS] = 1
        self.frame = []
        self.raw = {}                                # (array, slot) -> value written after packing: invalid runs

    def kf(self, slot, state=1, key=None, n=None, rows=None, registered=None, vote=0, own=None):
        own = slot if own is None else own           # (two keyframes may share a row: one keypoint then votes for both)
        self.state[slot] = state
        self.key[slot] = 4096 + 16 * slot if key is None else key
        if rows is None:
            n = int(self.rng.integers(1, 41)) if n is None else n
            rows = (self.rng.choice(np.arange(S, 480), n, replace=False) if self.expressible else self.rng.integers(S, 480, n)).astype(np.int32)
            m = self.rng.random(n)
            rows[m < 0.1] = -1
            exotic = self.rng.choice([N_ROWS, -7, 2 ** 31 - 1, int(BAD_ROWS[3])])
            if self.expressible:
                exotic = [-1, int(BAD_ROWS[3])][int(exotic == BAD_ROWS[3] and ((m >= 0.1) & (m < 0.15)).sum() == 1)]
            rows[(m >= 0.1) & (m < 0.15)] = exotic
            if n:
                rows[int(self.rng.integers(0, n))] = own
        self.runs[slot] = np.asarray(rows, np.int32)
        if registered is not None:
            self.reg[slot] = np.asarray(registered, np.uint8)
        self.frame += [own] * vote
        return self

    def many(self, slots, **kw):
        for s in slots:
            self.kf(s, **kw)
        return self

    def nb(self, slot, slots):
        self.neigh[slot, :len(slots)] = slots
        return self

    def ch(self, slot, slots):
        self.children[slot] = list(slots)            # (step() puts them into std::set<KeyFrame*> order)
        return self

    def par(self, slot, p):
        self.parent[slot] = p
        return self

    def step(self, frame=True):
        """the arrays: the runs packed into the pools in a shuffled slot order with gaps"""
        pool, regs = np.full(POOL, -1, np.int32), np.ones(POOL, np.uint8)
        poff, plen, coff, clen = (np.zeros(S, np.int32) for _ in range(4))
        cpool = np.full(CHILD_POOL, -1, np.int32)
        at = 3
        for s in self.rng.permutation(sorted(self.runs)):
            r = self.runs[s]
            pool[at:at + len(r)] = r
            if s in self.reg:
                regs[at:at + len(r)] = self.reg[s]
            poff[s], plen[s] = at, len(r)
            at += len(r) + int(self.rng.integers(0, 3))
        assert at <= POOL
        at = 1
        for s in sorted(self.children):
            c = sorted(self.children[s], key=lambda c: (int(self.key[c]) if 0 <= c < S else c, c))
            cpool[at:at + len(c)] = c
            coff[s], clen[s] = at, len(c)
            at += len(c) + 1
        assert at <= CHILD_POOL
        G = dict(state=self.state.copy(), order_key=self.key.copy(), point_off=poff, point_len=plen, point_pool=pool,
                 registered=regs if self.reg else None, neighbours=self.neigh.copy(), child_off=coff, child_len=clen, child_pool=cpool,
                 parent=self.parent.copy())
        for (name, s), v in self.raw.items():
            G[name][s] = v
        fr = None
        if frame:
            fr = np.array(self.frame, np.int32)
            self.rng.shuffle(fr)
        return dict(G=G, bad=self.bad.copy(), frame_rows=fr)


def e_total_of(step, kf_capacity=84):
    return int(update_local_keyframes_numpy(step["G"], step["bad"], step["frame_rows"], kf_capacity, 0)["counts"][4])


def _case(name, steps, expect, kf_capacity=84, entry_capacity=None, expect_list=None, expect_ref=None, check_step=-1):
    if entry_capacity is None:
        entry_capacity = max(e_total_of(s, kf_capacity) for s in steps) + 5
    return dict(name=name, steps=steps, kf_capacity=kf_capacity, entry_capacity=entry_capacity, expect=expect, expect_list=expect_list, expect_ref=expect_ref,
                check_step=check_step)


def _full(b, n_first, first_slot=0):
    """n_first voters in slots first_slot .. with one vote each, two keyframes to a row (n_frame stays below 64); no graph links yet"""
    for i in range(n_first):
        b.kf(first_slot + i, own=first_slot + i // 2 * 2, vote=1 - i % 2)
    return b


def _make_cases():
    C = {}

    def add(name, b_or_steps, expect, **kw):
        steps = b_or_steps if isinstance(b_or_steps, list) else [b_or_steps.step()]
        C[name] = _case(name, steps, expect, **kw)

    # ---- order and the reference keyframe
    b = Builder("order_keys_against_slots")
    for s in range(10, 20):
        b.kf(s, key=9000 - 50 * s, vote=1 + (s in (12, 17)) * 2)           # keys descend as slots ascend; 12 and 17 tie for the highest vote
    add("order_keys_against_slots", b, dict(n_first=10, end_reason=0), expect_list=list(range(19, 9, -1)), expect_ref=17)      # 17 has the lower key
    b = Builder("equal_keys_by_slot")
    for s in (30, 5, 77, 41):
        b.kf(s, key=123, vote=2)
    b.kf(50, key=-5, vote=1).kf(51, key=2 ** 62, vote=1)
    add("equal_keys_by_slot", b, dict(n_first=6), expect_list=[50, 5, 30, 41, 77, 51], expect_ref=5)
    # ---- the frame's rows
    b = Builder("frame_row_twice").kf(3, vote=1).kf(4, vote=2).kf(5, vote=1)
    add("frame_row_twice", b, dict(n_first=3), expect_ref=4)                # a point at two keypoints votes twice: 4 leads
    b = Builder("frame_rows_invalid").kf(3, vote=1).kf(4, vote=1)
    b.kf(6, rows=[int(BAD_ROWS[0]), 200, 6], vote=0)                         # seen through a bad row and a row the frame names as 6 + N_ROWS: no vote
    b.frame += [-1, N_ROWS, N_ROWS + 6, -2 ** 31, 2 ** 31 - 1, int(BAD_ROWS[0]), int(BAD_ROWS[0])]
    add("frame_rows_invalid", b, dict(n_counter=2, n_first=2), expect_list=[3, 4])
    b = Builder("frame_null").kf(3, vote=1).kf(4, vote=1)
    add("frame_null", [b.step(frame=False)], dict(n_counter=0), expect_list=[])
    b = Builder("frame_empty").kf(3).kf(4)
    add("frame_empty", b, dict(n_counter=0), expect_list=[])
    # ---- bad voters
    b = Builder("top_voter_bad").kf(8, state=2, vote=5).kf(9, vote=2).kf(10, vote=3).kf(11, vote=3)
    add("top_voter_bad", b, dict(n_counter=4, n_first=3), expect_list=[9, 10, 11], expect_ref=10)
    good = Builder("all_voters_bad_before").kf(20, vote=1).kf(21, vote=2)
    b = Builder("all_voters_bad").kf(8, state=2, vote=5).kf(9, state=2, vote=2).kf(20).kf(21)
    add("all_voters_bad", [good.step(), b.step()], dict(n_counter=2, n_first=0, n_local=0), expect_list=[], expect_ref=21)      # the list empty, ref_slot kept
    # ---- the empty counter: the list is kept and its rows gathered again
    b = Builder("empty_counter_keeps_the_list").kf(3, n=7, vote=1).kf(4, n=0, vote=0).kf(5, n=9, vote=2).nb(3, [4])
    s1 = b.step()
    b.frame = []
    s2 = b.step()
    s2["G"]["point_pool"][s2["G"]["point_off"][5] + 2] = 333                 # ReplaceMapPointMatch in between
    s2["G"]["state"][3] = 0                                                  # ... and a keyframe of the list erased: its run counts 0
    b.frame = [5, 4]
    add("empty_counter_keeps_the_list", [s1, s2, b.step()], dict(n_counter=0, n_local=3), expect_list=[3, 5, 4], expect_ref=5,
        check_step=1)
    # ---- registered
    b = Builder("registered")
    b.kf(3, rows=[3, 200, 3, 201], registered=[1, 1, 0, 1], vote=1)           # half registered: one of its two entries of row 3 counts
    b.kf(4, rows=[4, 202], registered=[0, 1], vote=3)                         # its votes vanish
    b.kf(5, vote=1)
    add("registered", b, dict(n_counter=2, n_first=2), expect_list=[3, 5], expect_ref=3)
    # ---- runs
    b = Builder("row_twice_in_a_run").kf(3, vote=1).kf(4, vote=1).kf(5, rows=[5, 250, 5], vote=1)
    add("row_twice_in_a_run", b, dict(n_first=3), expect_ref=5)              # counted twice: 5 leads although 3 and 4 have the same frame votes
    b = Builder("invalid_runs").many([3, 4, 5, 6, 7], vote=1).kf(8, n=0, vote=0).nb(3, [8]).ch(4, [9, 10]).ch(5, [11]).many([9, 10, 11])
    b.raw = {("point_len", 4): -1, ("point_off", 5): POOL - 2, ("point_off", 6): -3, ("child_len", 4): -2, ("child_off", 5): CHILD_POOL}
    b.runs[5] = np.array([5, 300, 301], np.int32)
    add("invalid_runs", b, dict(n_invalid_runs=5, n_first=2, n_children=0), expect_list=[3, 7, 8])      # 8: a zero-length run in the middle
    b = Builder("zero_length_run_in_the_middle").kf(3, vote=1).kf(4, n=0).kf(5, vote=1).nb(3, [4]).nb(5, [6]).kf(6)
    add("zero_length_run_in_the_middle", b, dict(n_first=2, n_neighbours=2), expect_list=[3, 5, 4, 6])
    # ---- neighbours
    b = Builder("neighbour_first_bad").kf(3, vote=1).kf(4, state=2).kf(5).nb(3, [4, 5])
    add("neighbour_first_bad", b, dict(n_neighbours=1), expect_list=[3, 5])
    b = Builder("neighbour_first_in_list").kf(3, vote=1).kf(4, vote=1).kf(5).nb(3, [4, 5])
    add("neighbour_first_in_list", b, dict(n_neighbours=1), expect_list=[3, 4, 5])
    b = Builder("neighbour_appended_earlier").kf(3, vote=1).kf(4, vote=1).kf(5).kf(6).nb(3, [5]).nb(4, [5, 6])
    add("neighbour_appended_earlier", b, dict(n_neighbours=2), expect_list=[3, 4, 5, 6])
    b = Builder("neighbour_unusable").kf(3, vote=1).kf(9).nb(3, [-1, S, -2 ** 31, 2 ** 31 - 1, 8, 9])      # 8 is absent
    add("neighbour_unusable", b, dict(n_neighbours=1), expect_list=[3, 9])
    b = Builder("neighbour_none_eligible").kf(3, vote=1).kf(4, vote=1).kf(5, state=2).nb(3, [4, 5, -1]).nb(4, [3])
    add("neighbour_none_eligible", b, dict(n_neighbours=0, n_local=2, end_reason=0), expect_list=[3, 4])
    # ---- children, in key order
    b = Builder("children_key_order").kf(3, vote=1).kf(40, key=50).kf(41, key=40).kf(42, key=30, state=2).ch(3, [40, 41, 42])
    add("children_key_order", b, dict(n_children=1), expect_list=[3, 41])    # 42 has the lowest key but is bad
    b = Builder("child_first_in_list").kf(3, vote=1).kf(4, vote=1).kf(5).ch(3, [4, 5])
    add("child_first_in_list", b, dict(n_children=1), expect_list=[3, 4, 5])
    b = Builder("child_appended_earlier").kf(3, vote=1).kf(4, vote=1).kf(5).kf(6).nb(3, [5]).ch(4, [5, 6])
    add("child_appended_earlier", b, dict(n_neighbours=1, n_children=1), expect_list=[3, 4, 5, 6])
    b = Builder("child_unusable").kf(3, vote=1).kf(9)
    b.children[3] = [-1, S + 4, 8, 2 ** 31 - 1, 9]
    add("child_unusable", b, dict(n_children=1), expect_list=[3, 9])
    b = Builder("child_none_eligible").kf(3, vote=1).kf(4, state=2).ch(3, [4])
    add("child_none_eligible", b, dict(n_children=0, n_local=1), expect_list=[3])
    b = Builder("long_child_run").kf(3, vote=1).kf(4, vote=1).many(range(20, 100)).kf(100)
    b.many(range(20, 100), state=2).ch(3, list(range(20, 100)) + [100]).ch(4, list(range(30, 99)) + [100, 101]).kf(101)
    add("long_child_run", b, dict(n_children=2), expect_list=[3, 4, 100, 101])      # 81 and 71 entries: beyond one wave and beyond the tiny LDS cap
    # ---- parents
    b = Builder("parent_ends_the_loop").kf(3, vote=1).kf(4, vote=1).kf(5).kf(6).par(3, 5).nb(4, [6])
    add("parent_ends_the_loop", b, dict(n_parents=1, n_neighbours=0, end_reason=2), expect_list=[3, 4, 5])      # 4 still had an eligible neighbour
    b = Builder("parent_bad").kf(3, vote=1).kf(5, state=2, vote=1).par(3, 5)
    add("parent_bad", b, dict(n_parents=1, end_reason=2, n_counter=2, n_first=1), expect_list=[3, 5])      # appended whatever its state
    b = Builder("parent_absent").kf(3, vote=1).kf(4, vote=1).kf(6).par(3, 5).par(4, S).nb(4, [6])
    add("parent_absent", b, dict(n_parents=0, n_neighbours=1, end_reason=0), expect_list=[3, 4, 6])
    b = Builder("parent_in_list").kf(3, vote=1).kf(4, vote=1).kf(6).par(3, 4).par(4, 6).nb(3, [6])
    add("parent_in_list", b, dict(n_parents=0, n_neighbours=1, end_reason=0), expect_list=[3, 4, 6])      # 6 came in as 3's neighbour
    # ---- the 80 rule: every element could add three
    for n_first in (78, 79, 80, 81):
        b = _full(Builder("limit_%d" % n_first), n_first).many(range(90, 128))
        for s in range(n_first):
            b.nb(s, [90 + s % 12]).ch(s, [102 + s % 12]).par(s, 114 + s % 12)
        exp = dict(n_first=n_first, n_local=n_first + 3, n_parents=1, end_reason=2) if n_first <= LIMIT else dict(n_first=n_first, n_local=n_first, end_reason=1)
        add("limit_%d" % n_first, b, exp)
    b = _full(Builder("limit_crossed_mid_loop"), 77).many(range(90, 128))
    for s in range(77):
        b.nb(s, [90 + s]).ch(s, [110 + s % 18])
    add("limit_crossed_mid_loop", b, dict(n_first=77, n_local=81, n_neighbours=2, n_children=2, end_reason=1))
    b = _full(Builder("first_list_over_capacity"), 90).many(range(90, 128))
    for s in range(90):
        b.nb(s, [100]).par(s, 101)
    add("first_list_over_capacity", b, dict(n_first=90, n_local=84, end_reason=1), expect_list=list(range(84)))
    b = _full(Builder("capacity_128"), 100, first_slot=10).many(range(0, 10))
    for s in range(10, 110):
        b.nb(s, [s - 10])
    add("capacity_128", b, dict(n_first=100, n_local=100, end_reason=1), kf_capacity=128, expect_list=list(range(10, 110)))
    # ---- the entry capacity
    b = Builder("entries").kf(3, vote=1).kf(4, vote=1).kf(5, n=0, vote=0).kf(6, n=33).nb(3, [5]).nb(4, [6])
    step = b.step()
    e = e_total_of(step)
    for cap, label in ((e - 1, "one_short"), (e, "exact"), (e + 7, "seven_more"), (0, "zero")):
        add("entries_" + label, [step], dict(n_local=4), entry_capacity=cap, expect_list=[3, 4, 5, 6])
    # ---- more voters than every cap of the tiny build, and everything at once
    b = _full(Builder("tiny_caps"), 75, first_slot=40).many(range(0, 40), state=1)
    b.many(range(0, 30, 3), state=2)
    for s in range(40, 115):
        b.nb(s, [127, s - 40, (s * 7) % 40]).ch(s, [(s * 3 + k) % 40 for k in range(5)] + [125])
    b.kf(125, key=0).kf(127)                                                 # 125: the lowest key, first among the children
    add("tiny_caps", b, dict(n_first=75, end_reason=1))
    return C


CASES = _make_cases()


def random_case(seed, n_slots=S, expressible=False):
    """a seeded random graph at the cases' shapes, in the first n_slots slots.  expressible: every slot reference names a present keyframe, every
    row a row of the table or -1 and no run holds a row twice, so that the reference's own containers can hold the graph (tests/tracking_cases.py)"""
    rng = np.random.default_rng(seed)
    b = Builder("random_%d" % seed, expressible)
    present = rng.choice(n_slots, int(rng.integers(1, n_slots + 1)), replace=False)
    n_voters = int(rng.integers(0, min(len(present), [4, 30, 90][seed % 3]) + 1))
    for i, s in enumerate(present):
        reg = None
        n = int(rng.integers(0, 41))
        b.kf(int(s), state=1 if rng.random() < 0.85 else 2, key=int(rng.integers(-50, 50)) if seed % 5 == 0 else int(rng.integers(-2 ** 62, 2 ** 62)), n=n,
             vote=int(rng.integers(1, 4)) if i < n_voters else 0)
        if seed % 2 and n and rng.random() < 0.3:
            b.reg[int(s)] = (rng.random(n) < 0.6).astype(np.uint8)
    for s in present:
        slots = (lambda n: rng.choice(present, n)) if expressible else None
        b.nb(int(s), (slots(int(rng.integers(0, 11))) if expressible else rng.integers(-2, S + 2, int(rng.integers(0, 11)))).tolist())
        if rng.random() < 0.6:
            drawn = slots(int(rng.integers(0, 6))) if expressible else rng.integers(-1, S + 1, int(rng.integers(0, 6)))
            b.children[int(s)] = sorted({int(c) for c in drawn}, key=lambda c: (int(b.key[c]) if 0 <= c < S else c, c))
        if rng.random() < (0.1 if seed % 3 else 0.6):
            b.par(int(s), int(slots(1)[0]) if expressible else int(rng.integers(-1, S + 1)))
    b.frame += (rng.integers(-1, N_ROWS, int(rng.integers(0, 20))) if expressible else rng.integers(-3, N_ROWS + 3, int(rng.integers(0, 20)))).tolist()
    b.frame = b.frame[:64]
    steps = [b.step()]
    if seed % 4 == 0:
        b.frame = []
        steps.append(b.step())
    kc = 84 if seed % 2 else 128
    e = e_total_of(steps[0], kc)
    return _case("random_%d" % seed, steps, {}, kf_capacity=kc, entry_capacity=[e + 3, max(e - 2, 0), e][seed % 3])
