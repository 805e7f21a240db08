"""KeyFrameDatabase (src/KeyFrameDatabase.cpp:44-313 of the reference) with DBoW2's BowVector fold (BowVector.cpp:34-84 in the order of
TemplatedVocabulary.h:1148-1193) and L1Scoring::score (ScoringObject.cpp:23-68) on the host, twice:
  Transcription  the sequential text, line by line: std::map as a dict walked in key order, the inverted file as lists of keyframe objects, the
                 persistent mnLoopQuery / mnLoopWords / mLoopScore / mnReloc* fields on the objects, float as numpy.float32;
  Restatement    the method of k_kfdb.hip in numpy over per-slot arrays: common words by intersection, the list as the ascending order of the key
                 (lowest common word, add sequence number), the first list position per best slot, an ordered compaction - for given build caps,
                 which only decide what is searched or sorted in LDS (counted in `paths`).
A WORLD is what the tests, the device and the reference driver (tools/ref_kfdb/) share: a vocabulary's leaf weights and a script of operations over
at most `M` slots, as flat arrays.  run(world, impl) plays it and returns every output as flat arrays, doubles as they are (compared as bits)."""
import os

import numpy as np

SHIPPED = (4096, 8192)                           # KD_QUERY_LDS, KD_SORT_LDS of k_kfdb.hip
TINY = (16, 64)                                  # the tiny_kfdb build (jetson_slam_amd/build.py VARIANTS)
NEIGHBOURS = 10
ADD, ERASE, LOOP, RELOC, SCORE, CLEAR = range(6)
GOLDEN = "ref_matcher_kfdb"                      # (the ref_matcher_ prefix: the fixture tests that walk tests/golden/*.npz leave such files to their own tests)
BLOCK_SEEDS = (21, 22, 23)
f32 = np.float32
MUTANTS = ("pairwise_sum", "c_times_w", "ge_words", "ge_best", "ge_retain", "slot_order", "reloc_words_test", "scores_reset")
COUNTERS = ("connected_skipped", "loop_same_id", "reloc_same_id", "at_min_words", "above_min_words", "below_min_score", "equal_min_score",
            "neighbour_takes_over", "neighbour_tie_or_less", "duplicate_best_slot", "not_retained", "order_differs", "readded_listed",
            "stale_reloc_score", "connected_neighbour", "neighbour_skipped", "stopped_word", "repeated_word", "no_candidates", "loop_neighbour_fails_words")


def bits(a):
    """float64 / float32 arrays as integers: what `equal` means for them"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def pairwise_sum(terms):
    """the tree sum a wave reduction would give: NOT the reference's order"""
    t = [float(x) for x in terms]
    if not t:
        return 0.0
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


# ---- the sequential text ----
def fold(weight, feats, mutant=None, count=None):
    """TemplatedVocabulary.h:1148-1193 with BowVector::addWeight and normalize(L1) -> (words int32[n] ascending, values float64[n])"""
    v = {}
    for wid in feats:                                                # :1148
        wid = int(wid)
        w = float(weight[wid]) if 0 <= wid < len(weight) else 0.0    # (an id outside the vocabulary: the library's "contributes nothing")
        if w > 0:                                                    # :1157 not stopped
            if wid in v:                                             # BowVector.cpp:38
                v[wid] += w                                          # :40
                if count is not None:
                    count["repeated_word"] += 1
            else:
                v[wid] = w                                           # :44
        elif count is not None:
            count["stopped_word"] += 1
    if mutant == "c_times_w":
        n = {}
        for wid in feats:
            n[int(wid)] = n.get(int(wid), 0) + 1
        v = {k: n[k] * float(weight[k]) for k in v}
    words = sorted(v)
    if mutant == "pairwise_sum":
        norm = pairwise_sum([abs(v[k]) for k in words])
    else:
        norm = 0.0                                                   # :64
        for k in words:                                              # :69
            norm += abs(v[k])                                        # :70
    if norm > 0.0:                                                   # :79
        for k in words:
            v[k] /= norm                                             # :82
    return np.array(words, np.int32), np.array([v[k] for k in words], np.float64)


def l1_terms(q, k):
    """the terms of ScoringObject.cpp:41 in the merge walk's order"""
    (qw, qv), (kw, kv) = q, k
    i = j = 0
    out = []
    while i < len(qw) and j < len(kw):                               # :34
        if qw[i] == kw[j]:                                           # :39
            vi, wi = float(qv[i]), float(kv[j])
            out.append(abs(vi - wi) - abs(vi) - abs(wi))             # :41
            i += 1; j += 1
        elif qw[i] < kw[j]:
            i += 1                                                   # (lower_bound lands where stepping does)
        else:
            j += 1
    return out


def l1_score(q, k, mutant=None):
    """L1Scoring::score -> a Python float (double)"""
    terms = l1_terms(q, k)
    if mutant == "pairwise_sum":
        score = pairwise_sum(terms)
    else:
        score = 0.0                                                  # :32
        for t in terms:
            score += t
    return -score / 2.0                                              # :65


class _KF:
    def __init__(self, slot, vec):
        self.slot, self.vec = slot, vec
        self.loop_query = self.reloc_query = 0                       # KeyFrame.cpp:39
        self.loop_words = self.reloc_words = 0
        self.loop_score = self.reloc_score = f32(0)                  # (uninitialised there: zero by this library's definition)


class Transcription:
    def __init__(self, world, mutant=None):
        self.weight, self.M, self.mutant = world["weight"], int(world["M"]), mutant
        self.inverted = [[] for _ in range(len(self.weight))]        # :40
        self.kf = [None] * self.M
        self.count = dict.fromkeys(COUNTERS, 0)
        self.readded = set()
        self.adds = []

    def fold(self, feats):
        return fold(self.weight, feats, self.mutant, self.count)

    def add(self, slot, vec):
        assert self.kf[slot] is None
        k = _KF(slot, vec)
        self.kf[slot] = k
        self.adds.append(slot)
        for w in vec[0]:                                             # :48
            self.inverted[w].append(k)                               # :49

    def erase(self, slot):
        k = self.kf[slot]
        if k is None:
            return
        for w in k.vec[0]:                                           # :57
            self.inverted[w].remove(k)                               # :62-68
        self.kf[slot] = None
        self.adds.remove(slot)
        self.readded.add(slot)

    def clear(self):
        self.inverted = [[] for _ in range(len(self.weight))]        # :75-76
        self.kf = [None] * self.M
        self.adds = []

    def score(self, q, slots):
        """LoopClosing.cpp:129-143 -> (score_f64, score float32, min_score float32)"""
        d, f, m = [], [], f32(1)
        for s in slots:
            k = self.kf[s] if 0 <= s < self.M else None
            if k is None:                                            # isBad(): continue
                d.append(-1.0); f.append(f32(-1))
                continue
            sc = l1_score(q, k.vec, self.mutant)
            d.append(sc); f.append(f32(sc))
            if f32(sc) < m:
                m = f32(sc)
        return np.array(d, np.float64), np.array(f, np.float32), m

    def _neighbours(self, row):
        """GetBestCovisibilityKeyFrames(10) of a slot as the contract defines it: -1 and keyframes outside the database are not there"""
        out = []
        for n in row[:NEIGHBOURS]:
            if 0 <= n < self.M and self.kf[n] is not None:
                out.append(self.kf[n])
            else:
                self.count["neighbour_skipped"] += 1
        return out

    def detect(self, reloc, q, qid, connected, neigh, min_score):
        """DetectLoopCandidates (:80-201) / DetectRelocalizationCandidates (:203-313) -> (candidate slots, stats)"""
        mu, cnt = self.mutant, self.count
        ge = lambda name, a, b: a >= b if mu == name else a > b
        min_score = f32(min_score)
        sharing = []
        if mu == "scores_reset":
            for k in self.kf:
                if k is not None:
                    k.loop_score = k.reloc_score = f32(0)
        for w in q[0]:                                               # :90 / :211
            for k in self.inverted[w]:                               # :94
                if reloc:
                    if k.reloc_query != qid:                         # :218
                        k.reloc_words = 0
                        k.reloc_query = qid
                        sharing.append(k)
                    else:
                        cnt["reloc_same_id"] += 1
                    k.reloc_words += 1                               # :224
                else:
                    if k.loop_query != qid:                          # :97
                        k.loop_words = 0                             # :99
                        if not connected[k.slot]:                    # :100
                            k.loop_query = qid
                            sharing.append(k)
                        else:
                            cnt["connected_skipped"] += 1
                    else:
                        cnt["loop_same_id"] += 1
                    k.loop_words += 1                                # :106
        words = (lambda k: k.reloc_words) if reloc else (lambda k: k.loop_words)
        start = f32(0) if reloc else min_score
        stats = dict(n_sharing=len(sharing), max_common=0, min_common=0, n_scored=0, n_kept=0, best_acc=start, order=[k.slot for k in sharing])
        if not sharing:                                              # :111
            cnt["no_candidates"] += 1
            return [], stats
        if mu == "slot_order":
            sharing.sort(key=lambda k: k.slot)
        order = [k.slot for k in sharing]
        if order != sorted(order) and order != [s for s in self.adds if s in order]:
            cnt["order_differs"] += 1
        cnt["readded_listed"] += sum(s in self.readded for s in order)
        max_common = 0
        for k in sharing:                                            # :118
            if words(k) > max_common:
                max_common = words(k)
        min_common = int(f32(max_common) * f32(0.8))                 # :124
        stats.update(max_common=max_common, min_common=min_common)
        kept = []
        for k in sharing:                                            # :129
            cnt["at_min_words"] += words(k) == min_common
            cnt["above_min_words"] += words(k) == min_common + 1
            if ge("ge_words", words(k), min_common):                 # :133
                stats["n_scored"] += 1
                si = f32(l1_score(q, k.vec, mu))                     # :137
                if reloc:
                    k.reloc_score = si
                    kept.append((si, k))
                else:
                    k.loop_score = si                                # :139
                    cnt["equal_min_score"] += si == min_score
                    if si >= min_score:                              # :140
                        kept.append((si, k))
                    else:
                        cnt["below_min_score"] += 1
        stats["n_kept"] = len(kept)
        if not kept:                                                 # :145
            cnt["no_candidates"] += 1
            return [], stats
        acc_list = []
        best_acc = start                                             # :149 / :263
        for si, k in kept:                                           # :152
            best, acc, best_kf = si, si, k
            for k2 in self._neighbours(neigh[k.slot]):               # :160
                if reloc:
                    if k2.reloc_query != qid:                        # :277
                        continue
                    if mu == "reloc_words_test" and not k2.reloc_words > min_common:
                        continue
                    cnt["stale_reloc_score"] += k2.reloc_words <= min_common
                    s2 = k2.reloc_score
                else:
                    cnt["connected_neighbour"] += bool(connected[k2.slot])
                    if not (k2.loop_query == qid and k2.loop_words > min_common):      # :163
                        cnt["loop_neighbour_fails_words"] += k2.loop_query == qid
                        continue
                    s2 = k2.loop_score
                acc = f32(acc + s2)                                  # :165
                if ge("ge_best", s2, best):                          # :166
                    best_kf, best = k2, s2
                    cnt["neighbour_takes_over"] += 1
                else:
                    cnt["neighbour_tie_or_less"] += 1
            acc_list.append((acc, best_kf))                          # :174
            if acc > best_acc:                                       # :175
                best_acc = acc
        stats["best_acc"] = best_acc
        retain = f32(f32(0.75) * best_acc)                           # :180
        seen, out = set(), []
        for acc, k in acc_list:                                      # :186
            if ge("ge_retain", acc, retain):                         # :188
                if k.slot not in seen:                               # :191
                    out.append(k.slot)
                    seen.add(k.slot)
                else:
                    cnt["duplicate_best_slot"] += 1
            else:
                cnt["not_retained"] += 1
        return out, stats

    def state(self):
        z = lambda dt: np.zeros(self.M, dt)
        st = dict(present=z(np.int32), loop_query=z(np.uint64), reloc_query=z(np.uint64), loop_words=z(np.int32), reloc_words=z(np.int32),
                  loop_score=z(np.float32), reloc_score=z(np.float32))
        for s, k in enumerate(self.kf):
            if k is not None:
                st["present"][s] = 1
                for key in list(st)[1:]:
                    st[key][s] = getattr(k, key)
        return st


# ---- the kernels' method ----
class Restatement:
    def __init__(self, world, caps=SHIPPED):
        self.weight, self.M, self.caps = world["weight"], int(world["M"]), caps
        M = self.M
        self.vec = [None] * M
        self.seq = np.zeros(M, np.int64)
        self.next_seq = 0
        self.st = dict(present=np.zeros(M, np.int32), loop_query=np.zeros(M, np.uint64), reloc_query=np.zeros(M, np.uint64),
                       loop_words=np.zeros(M, np.int32), reloc_words=np.zeros(M, np.int32), loop_score=np.zeros(M, np.float32),
                       reloc_score=np.zeros(M, np.float32))
        self.paths = dict(sort_lds=0, sort_global=0, query_lds=0, query_global=0)

    def fold(self, feats):
        """k_kfdb_bow_vector: sort, run heads, w added run - 1 times, the norm added in ascending order, one division each"""
        feats = np.asarray(feats, np.int64)
        self.paths["sort_lds" if len(feats) <= self.caps[1] else "sort_global"] += 1
        ok = (feats >= 0) & (feats < len(self.weight))
        ok[ok] &= self.weight[feats[ok]] > 0
        keys = np.sort(feats[ok])
        words, runs = np.unique(keys, return_counts=True)
        values = np.empty(len(words), np.float64)
        for i, (w, c) in enumerate(zip(words, runs)):
            values[i] = np.add.accumulate(np.full(c, self.weight[w]))[-1]          # sequential: w + w + ...
        norm = float(np.add.accumulate(np.abs(values))[-1]) if len(values) else 0.0  # np.add.accumulate is the running (sequential) sum
        if norm > 0.0:
            values = values / norm
        return words.astype(np.int32), values

    def _common(self, q, s):
        """kd_common: (count, lowest common word, -sum / 2 with the terms added in ascending word order)"""
        kw, kv = self.vec[s]
        hit = np.isin(kw, q[0])
        c = int(hit.sum())
        if c == 0:
            return 0, -1, -0.0
        vi = q[1][np.searchsorted(q[0], kw[hit])]
        wi = kv[hit]
        t = np.abs(vi - wi) - np.abs(vi) - np.abs(wi)
        return c, int(kw[hit][0]), -float(np.add.accumulate(t)[-1]) / 2.0

    def add(self, slot, vec):
        assert not self.st["present"][slot]
        self.vec[slot] = vec
        self.seq[slot] = self.next_seq
        self.next_seq += 1
        for k in self.st:
            self.st[k][slot] = 0
        self.st["present"][slot] = 1

    def erase(self, slot):
        self.st["present"][slot] = 0

    def clear(self):
        self.st["present"][:] = 0
        self.next_seq = 0

    def score(self, q, slots):
        self.paths["query_lds" if len(q[0]) <= self.caps[0] else "query_global"] += 1
        d = np.array([self._common(q, s)[2] if 0 <= s < self.M and self.st["present"][s] else -1.0 for s in slots], np.float64)
        f = d.astype(np.float32)
        ok = np.array([0 <= s < self.M and bool(self.st["present"][s]) for s in slots], bool)
        m = f32(1)
        if ok.any() and f[ok].min() < m:
            m = f[ok][np.argmax(f[ok] == f[ok].min())]                # the first of the values that compare equal to the least
        return d, f, m

    def detect(self, reloc, q, qid, connected, neigh, min_score):
        self.paths["query_lds" if len(q[0]) <= self.caps[0] else "query_global"] += 1
        st, M = self.st, self.M
        qk, wk, sk = ("reloc_query", "reloc_words", "reloc_score") if reloc else ("loop_query", "loop_words", "loop_score")
        start = f32(0) if reloc else f32(min_score)
        keys, tscore = {}, {}
        for s in np.nonzero(st["present"])[0]:                      # k_kfdb_common
            c, first, sc = self._common(q, s)
            if c == 0:
                continue
            if st[qk][s] != qid:
                if not reloc and connected[s]:
                    st[wk][s] = 1
                else:
                    st[qk][s] = qid; st[wk][s] = c
                    keys[s] = (first, int(self.seq[s])); tscore[s] = f32(sc)
            else:
                st[wk][s] += c
        lst = sorted(keys, key=keys.get)                             # k_kfdb_rank
        max_common = max([int(st[wk][s]) for s in lst], default=0)
        min_common = int(f32(max_common) * f32(0.8))
        flag = []
        n_scored = 0
        for s in lst:
            scored = st[wk][s] > min_common
            if scored:
                st[sk][s] = tscore[s]
                n_scored += 1
            flag.append(bool(scored and (reloc or tscore[s] >= start)))
        acc, best = {}, {}
        for i, s in enumerate(lst):                                  # k_kfdb_accumulate
            if not flag[i]:
                continue
            a = b = st[sk][s]
            bs = s
            for n in neigh[s][:NEIGHBOURS]:
                if not (0 <= n < M) or not st["present"][n]:
                    continue
                if st[qk][n] != qid or (not reloc and not st[wk][n] > min_common):
                    continue
                a = f32(a + st[sk][n])
                if st[sk][n] > b:
                    b, bs = st[sk][n], n
            acc[i], best[i] = a, bs
        best_acc = start                                             # the maximum, the earliest among equals (the start first of all)
        for i in sorted(acc):
            if acc[i] > best_acc:
                best_acc = acc[i]
        retain = f32(f32(0.75) * best_acc)
        first_pos = {}                                               # k_kfdb_emit
        for i in acc:
            if acc[i] > retain:
                first_pos[best[i]] = min(first_pos.get(best[i], i), i)
        out = [best[i] for i in sorted(acc) if acc[i] > retain and first_pos[best[i]] == i]
        return out, dict(n_sharing=len(lst), max_common=max_common, min_common=min_common, n_scored=n_scored, n_kept=sum(flag), best_acc=best_acc,
                         order=[int(s) for s in lst])

    def state(self):
        out = {k: v.copy() for k, v in self.st.items()}
        for k in out:
            if k != "present":
                out[k][self.st["present"] == 0] = 0
        return out


# ---- worlds ----
class Script:
    """builds a world: the operations in order"""

    def __init__(self, weight, M):
        self.weight, self.M = np.asarray(weight, np.float64), M
        self.ops = []

    def _op(self, kind, slot=-1, qid=0, min_score=0.0, feats=(), lst=(), connected=(), neigh=None):
        conn = np.zeros(self.M, np.uint8)
        if len(connected):
            conn[list(connected)] = 1
        nb = np.full((self.M, NEIGHBOURS), -1, np.int32)
        for s, row in (neigh or {}).items():
            nb[s, :len(row)] = row
        self.ops.append(dict(kind=kind, slot=slot, id=qid, min_score=f32(min_score), feats=list(feats), lst=list(lst), conn=conn, neigh=nb))
        return self

    def add(self, slot, feats): return self._op(ADD, slot, feats=feats)
    def erase(self, slot): return self._op(ERASE, slot)
    def clear(self): return self._op(CLEAR)
    def loop(self, feats, qid, min_score, connected=(), neigh=None): return self._op(LOOP, qid=qid, min_score=min_score, feats=feats, connected=connected, neigh=neigh)
    def reloc(self, feats, qid, neigh=None): return self._op(RELOC, qid=qid, feats=feats, neigh=neigh)
    def score(self, feats, slots): return self._op(SCORE, feats=feats, lst=slots)

    def vec(self, feats):
        return fold(self.weight, feats)

    def si(self, q_feats, kf_feats):
        return f32(l1_score(self.vec(q_feats), self.vec(kf_feats)))

    def world(self):
        o = self.ops
        cat = lambda key, dt: np.array([x for op in o for x in op[key]], dt)
        starts = lambda key: np.concatenate([[0], np.cumsum([len(op[key]) for op in o])]).astype(np.int32)
        return dict(weight=self.weight, M=np.int32(self.M), op_kind=np.array([op["kind"] for op in o], np.int32),
                    op_slot=np.array([op["slot"] for op in o], np.int32), op_id=np.array([op["id"] for op in o], np.uint64),
                    op_min_score=np.array([op["min_score"] for op in o], np.float32), op_feat_start=starts("feats"), feat=cat("feats", np.int32),
                    op_list_start=starts("lst"), lst=cat("lst", np.int32), conn=np.stack([op["conn"] for op in o]),
                    neigh=np.stack([op["neigh"] for op in o]))


OUT_KEYS = ("bow_start", "bow_word", "bow_value", "cand_start", "cand", "score_f64", "score", "min_score", "present", "loop_query", "reloc_query",
            "loop_words", "reloc_words", "loop_score", "reloc_score")
STAT_KEYS = ("n_sharing", "max_common", "min_common", "n_scored", "n_kept")


def run(world, impl):
    """the script through `impl` (a Transcription, a Restatement, or anything with their methods) -> dict of OUT_KEYS, then `stats` int32[n_ops, 5],
    `best_acc` float32[n_ops] and `order` (per op the listed slots) - the reference's file has OUT_KEYS only"""
    n = len(world["op_kind"])
    M = int(world["M"])
    bw, bv, bs, cd, cs, sd, sf = [], [], [0], [], [0], [], []
    mins = np.zeros(n, np.float32)
    states = {k: [] for k in OUT_KEYS[8:]}
    stats, best_acc, orders = np.zeros((n, 5), np.int32), np.zeros(n, np.float32), []
    for i in range(n):
        kind, slot = int(world["op_kind"][i]), int(world["op_slot"][i])
        feats = world["feat"][world["op_feat_start"][i]:world["op_feat_start"][i + 1]]
        vec, order = None, []
        if kind in (ADD, LOOP, RELOC, SCORE):
            vec = impl.fold(feats)
            bw.extend(vec[0]); bv.extend(vec[1])
        if kind == ADD:
            impl.add(slot, vec)
        elif kind == ERASE:
            impl.erase(slot)
        elif kind == CLEAR:
            impl.clear()
        elif kind == SCORE:
            d, f, m = impl.score(vec, [int(s) for s in world["lst"][world["op_list_start"][i]:world["op_list_start"][i + 1]]])
            sd.extend(d); sf.extend(f); mins[i] = m
        else:
            out, s = impl.detect(kind == RELOC, vec, int(world["op_id"][i]), world["conn"][i], world["neigh"][i], world["op_min_score"][i])
            cd.extend(out)
            stats[i] = [s[k] for k in STAT_KEYS]
            best_acc[i] = s["best_acc"]
            order = s["order"]
        orders.append(order)
        bs.append(len(bw)); cs.append(len(cd))
        st = impl.state()
        for k in states:
            states[k].append(st[k])
    out = dict(bow_start=np.array(bs, np.int32), bow_word=np.array(bw, np.int32), bow_value=np.array(bv, np.float64), cand_start=np.array(cs, np.int32),
               cand=np.array(cd, np.int32), score_f64=np.array(sd, np.float64), score=np.array(sf, np.float32), min_score=mins)
    for k in states:
        out[k] = np.stack(states[k]) if n else np.zeros((0, M))
    out.update(stats=stats, best_acc=best_acc, order=orders)
    return out


def same(a, b, keys=OUT_KEYS):
    """the first key in which two outputs differ (floating point by bits), or None"""
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return k
        if not np.array_equal(bits(x) if x.dtype.kind == "f" else x, bits(y) if y.dtype.kind == "f" else y):
            return k
    return None


def candidates(out, op):
    return [int(x) for x in out["cand"][out["cand_start"][op]:out["cand_start"][op + 1]]]


def small_weights(W, seed, zeros=()):
    w = np.random.RandomState(seed).uniform(0.5, 9.0, W)
    w[list(zeros)] = 0.0
    return w


def _words(k, base=0):
    return list(range(base, base + k))


def constructed():
    """name -> (world, check(out of the transcription) -> None or raises): one world per decision.  Vocabulary of 64 words; word 63 is stopped."""
    W = small_weights(64, 5, zeros=(63,))
    C = {}

    def case(name, script, check):
        C[name] = (script.world(), check)

    def expect(op, want, **stats):
        def check(out):
            assert candidates(out, op) == want, (candidates(out, op), want)
            for k, v in stats.items():
                assert out["stats"][op][STAT_KEYS.index(k)] == v, (k, out["stats"][op], v)
        return check

    q10 = _words(10)
    case("empty_database", Script(W, 4).loop(q10, 7, 0.0).reloc(q10, 8).score(q10, [0, 3]), expect(0, [], n_sharing=0))
    case("no_shared_word", Script(W, 4).add(0, _words(5, 20)).add(1, _words(5, 30)).loop(q10, 7, 0.0).reloc(q10, 8), expect(2, [], n_sharing=0))
    case("everything_connected", Script(W, 4).add(0, _words(5)).add(1, _words(3, 2)).loop(q10, 7, 0.0, connected=[0, 1]),
         lambda out: (expect(2, [], n_sharing=0)(out), np.testing.assert_array_equal(out["loop_words"][2][:2], [1, 1]),
                      np.testing.assert_array_equal(out["loop_query"][2][:2], [0, 0])))
    for mx, at in ((4, 3), (5, 4), (10, 8)):                         # (int)(max * 0.8f) = 3, 4, 8
        s = Script(W, 4).add(0, _words(mx)).add(1, _words(at)).add(2, _words(at + 1)).loop(_words(mx), 7, 0.0).reloc(_words(mx), 9)

        def check(out, mx=mx, at=at):
            for op, words, score in ((3, "loop_words", "loop_score"), (4, "reloc_words", "reloc_score")):
                assert list(out["stats"][op][:4]) == [3, mx, at, 2], out["stats"][op]
                assert list(out[words][op][:3]) == [mx, at, at + 1]
                assert out[score][op][1] == 0 and out[score][op][0] > 0 and out[score][op][2] > 0      # exactly at minCommonWords: not scored
        case("max_common_words_%d" % mx, s, check)
    b = _words(6, 3)
    s = Script(W, 4).add(0, b).add(1, b)
    case("si_equals_min_score_kept", s.loop(q10, 7, s.si(q10, b)), expect(2, [0, 1], n_scored=2, n_kept=2))
    s = Script(W, 4).add(0, b).add(1, b)
    case("si_below_min_score_dropped", s.loop(q10, 7, np.nextafter(s.si(q10, b), f32(2))), expect(2, [], n_scored=2, n_kept=0))
    a = _words(6)
    # four keyframes with the query's own vector, so every score is 1.0f: acc = 4, 3, 1, 1 and 0.75f * 4 == 3, so entry 1 is NOT retained; no
    # neighbour's equal score takes the best slot over
    same4 = Script(W, 6)
    for k in range(4):
        same4.add(k, a)
    nb = {0: [1, 2, 3], 1: [0, 2]}
    case("acc_equals_retain_dropped", same4.loop(a, 7, 0.0, neigh=nb).reloc(a, 8, neigh=nb),
         lambda out: (expect(4, [0], n_kept=4)(out), expect(5, [0])(out)))
    weak, strong = _words(8) + _words(6, 30), _words(9)
    case("neighbour_takes_over", Script(W, 4).add(0, weak).add(1, strong).loop(q10, 7, 0.0, neigh={0: [1]}).reloc(q10, 8, neigh={0: [1]}),
         lambda out: (expect(2, [1])(out), expect(3, [1])(out)))
    case("two_entries_same_best_slot", Script(W, 4).add(0, weak).add(2, weak).add(1, strong).loop(q10, 7, 0.0, neigh={0: [1], 2: [1]}),
         expect(3, [1], n_kept=3))
    # list order: slot 2 shares word 0 (added last), slot 0 shares from word 1 (added second), slot 1 from word 1 (added first): 2, 1, 0
    order = Script(W, 4).add(1, _words(9, 1)).add(0, _words(9, 1)).add(2, _words(9))
    case("list_order_is_neither_slot_nor_add_order", order.loop(q10, 7, 0.0).reloc(q10, 8),
         lambda out: (np.testing.assert_equal(out["order"][3], [2, 1, 0]), expect(3, [2, 1, 0])(out), expect(4, [2, 1, 0])(out)))
    er = Script(W, 4).add(0, _words(9)).add(1, _words(9)).add(2, _words(9)).loop(q10, 7, 0.0).erase(0).loop(q10, 8, 0.0).add(0, _words(9)).loop(q10, 9, 0.0)
    case("erase_and_readd_change_the_order", er, lambda out: (expect(3, [0, 1, 2])(out), expect(5, [1, 2])(out), expect(7, [1, 2, 0])(out),
                                                                np.testing.assert_equal(int(out["loop_query"][6][0]), 0)))
    rep = Script(W, 4).add(0, _words(9)).add(1, _words(5)).loop(q10, 7, 0.0).loop(q10, 7, 0.0).reloc(q10, 3).reloc(q10, 3)
    case("same_query_id_twice", rep, lambda out: (expect(2, [0])(out), expect(3, [], n_sharing=0)(out), expect(5, [], n_sharing=0)(out),
                                                  np.testing.assert_array_equal(out["loop_words"][3][:2], [18, 10]),
                                                  np.testing.assert_array_equal(out["reloc_words"][5][:2], [18, 10])))
    # query A scores slot 1 (9 of 9 words); query B shares 2 words with slot 1 (below minCommonWords) and 9 with slot 0, whose neighbour slot 1 is:
    # reloc adds the score query A left in slot 1 (here the larger one: slot 1 takes over), loop's words test shuts it out
    qa, qb = _words(9, 20), _words(9) + [20, 21]
    stale = Script(W, 4).add(0, _words(9)).add(1, _words(9, 20)).reloc(qa, 5).reloc(qb, 6, neigh={0: [1]}).loop(qa, 5, 0.0).loop(qb, 6, 0.0, neigh={0: [1]})
    case("stale_reloc_score_is_read", stale, lambda out: (expect(3, [1], n_scored=1)(out), expect(5, [0], n_scored=1)(out)))
    cn = Script(W, 4).add(0, weak).add(1, strong).loop(q10, 7, 0.0, connected=[1], neigh={0: [1]})
    case("connected_keyframe_as_neighbour", cn, expect(2, [0], n_sharing=1))
    z = Script(W, 4).add(0, _words(9)).add(1, _words(9)).loop(q10, 0, 0.0).reloc(q10, 0).loop(q10, 1, 0.0, neigh={0: [3, -1, 1]})
    case("query_id_zero_on_fresh_slots", z, lambda out: (expect(2, [], n_sharing=0)(out), expect(3, [], n_sharing=0)(out), expect(4, [0])(out)))
    st = Script(W, 4).add(0, [63, 1, 2, 63]).add(1, [63]).score([1, 63], [0, 1, 2]).reloc([63], 4)
    case("stopped_word", st, lambda out: (np.testing.assert_array_equal(out["bow_word"][:2], [1, 2]), np.testing.assert_equal(int(out["bow_start"][2]), 2)))
    mult = Script(W, 4).add(0, [5] + [6] * 2 + [7] * 7).add(1, [7, 5, 7, 6, 7, 7, 6, 7, 7, 7]).score([5, 6, 7], [0, 1])
    case("word_occurring_1_2_and_7_times", mult, lambda out: np.testing.assert_array_equal(bits(out["bow_value"][:3]), bits(out["bow_value"][3:6])))
    # sums whose sequential value differs from the pairwise one in its bits (asserted by check_summation_cases)
    rs = np.random.RandomState(3)
    big = Script(small_weights(512, 9), 4)
    for k in range(3):
        big.add(k, rs.randint(0, 512, 300))
    qf = rs.randint(0, 512, 300)
    case("sequential_sum_differs_from_pairwise", big.score(qf, [0, 1, 2]).loop(qf, 7, 0.0).reloc(qf, 8), lambda out: check_summation_case(big.world()))
    return C


def check_summation_case(world):
    """at least one vector and one score of the world whose sequential double sum differs in its bits from the pairwise sum of the same terms"""
    t, m = run(world, Transcription(world)), run(world, Transcription(world, "pairwise_sum"))
    assert not np.array_equal(bits(t["bow_value"]), bits(m["bow_value"])) and not np.array_equal(bits(t["score_f64"]), bits(m["score_f64"]))


def block(seed, n_ops=110, M=24):
    """a random script: a small vocabulary so that words are shared, duplicated keyframes so that scores tie, repeated ids, erases and re-adds"""
    rs = np.random.RandomState(seed)
    nw = int(rs.choice([32, 48, 96]))
    s = Script(small_weights(nw, seed, zeros=rs.choice(nw, 3, replace=False)), M)
    present, feats_of, ids = {}, [], [0, 1]

    def feats():
        if feats_of and rs.rand() < 0.25:
            return list(feats_of[rs.randint(len(feats_of))])
        lo = rs.randint(0, nw - 8)
        f = list(rs.randint(lo, min(nw, lo + rs.randint(8, 40)), rs.randint(0, 60)))
        if rs.rand() < 0.1:
            f = list(rs.randint(0, nw, rs.randint(200, 301)))
        feats_of.append(f)
        return f

    def neigh():
        return {k: list(rs.choice(np.arange(-1, M), rs.randint(0, NEIGHBOURS + 1))) for k in range(M) if rs.rand() < 0.8}

    for _ in range(n_ops):
        r = rs.rand()
        free = [k for k in range(M) if k not in present]
        if (r < 0.3 or len(present) < 6) and free:
            k = int(rs.choice(free))
            present[k] = feats()
            s.add(k, present[k])
        elif r < 0.38 and present:
            k = int(rs.choice(list(present)))
            del present[k]
            s.erase(k)
        elif r < 0.45:
            s.score(feats(), list(rs.choice(np.arange(-1, M + 1), rs.randint(0, 12))))
        else:
            q = list(present[int(rs.choice(list(present)))]) + list(rs.randint(0, nw, rs.randint(0, 10))) if present and rs.rand() < 0.6 else feats()
            if rs.rand() < 0.7:
                ids.append(int(rs.randint(2, 1 << 40)))
            qid = ids[rs.randint(len(ids))] if rs.rand() < 0.35 else ids[-1]
            if rs.rand() < 0.5:
                s.reloc(q, qid, neigh())
            else:
                ms = 0.0
                if present and rs.rand() < 0.6:
                    ms = s.si(q, present[int(rs.choice(list(present)))])
                    if rs.rand() < 0.3:
                        ms = ms * f32(0.5)
                s.loop(q, qid, ms, connected=[k for k in range(M) if rs.rand() < 0.15], neigh=neigh())
    return s.world()


def fixture_worlds():
    """name -> world: what tests/golden/ref_matcher_kfdb.npz holds, inputs as generated here"""
    worlds = {"c_" + name: w for name, (w, _) in constructed().items()}
    for seed in BLOCK_SEEDS:
        worlds["random_%d" % seed] = block(seed)
    return worlds


def counters(world):
    t = Transcription(world)
    run(world, t)
    return t.count


# ---- the fixture and the reference driver ----
def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_path():
    return os.path.join(_root(), "tests", "golden", GOLDEN + ".npz")


def save_golden(worlds):
    """name -> flat dict of arrays, as an npz with a fixed member order and no timestamps: regenerating gives the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w", zipfile.ZIP_DEFLATED) as z:
        for name in worlds:
            for key in sorted(worlds[name]):
                buf = io.BytesIO()
                np.save(buf, np.ascontiguousarray(worlds[name][key]), allow_pickle=False)
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, key), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


def load_golden():
    """name -> dict of arrays (the world's inputs and out_<key> for OUT_KEYS), in the file's order"""
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, key = member.rsplit(".", 1)
            out.setdefault(name, {})[key] = z[member] if key != "M" else z[member].reshape(())[()]
    return out


def reference_tree():
    """the reference tree, or None where it is absent"""
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if os.path.exists(os.path.join(ref, "src", "KeyFrameDatabase.cpp")) else None


def driver_path():
    return os.path.join(_root(), "oracle", "_ref", "ref_kfdb")


def build_driver(reference):
    """the reference's src/KeyFrameDatabase.cpp and DBoW2's BowVector.cpp and ScoringObject.cpp, unmodified, with tools/ref_kfdb's stand-ins
    force-included so that their guards shut out the reference's KeyFrame.h / Frame.h / ORBVocabulary.h"""
    import subprocess
    shadow = os.path.join(_root(), "tools", "ref_kfdb")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    dbow = os.path.join(reference, "Thirdparty", "DBoW2", "DBoW2")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-fno-fast-math", "-ffp-contract=off", "-w", "-I" + shadow, "-I" + os.path.join(reference, "include"),
           "-I" + reference]
    for h in ("KeyFrame.h", "Frame.h", "ORBVocabulary.h"):
        cmd += ["-include", os.path.join(shadow, h)]
    cmd += ["-o", driver_path(), os.path.join(shadow, "driver.cpp"), os.path.join(reference, "src", "KeyFrameDatabase.cpp"),
            os.path.join(dbow, "BowVector.cpp"), os.path.join(dbow, "ScoringObject.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    return driver_path()


IN_ORDER = (("weight", np.float64), ("op_kind", np.int32), ("op_slot", np.int32), ("op_id", np.uint64), ("op_min_score", np.float32),
            ("op_feat_start", np.int32), ("feat", np.int32), ("op_list_start", np.int32), ("lst", np.int32), ("conn", np.uint8), ("neigh", np.int32))


def run_driver(w, workdir):
    """a world through the reference -> dict of OUT_KEYS"""
    import subprocess
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    n, M = len(w["op_kind"]), int(w["M"])
    with open(src, "wb") as f:
        f.write(np.array([len(w["weight"]), M, n, len(w["feat"]), len(w["lst"])], np.int32).tobytes())
        for key, dt in IN_ORDER:
            f.write(np.ascontiguousarray(w[key], dt).tobytes())
    subprocess.check_call([driver_path(), src, dst], timeout=120)
    raw = open(dst, "rb").read()
    n_bow, n_cand = np.frombuffer(raw, np.int32, 2)
    pos, out = 8, {}
    L = len(w["lst"])
    shapes = dict(bow_start=(np.int32, n + 1), bow_word=(np.int32, n_bow), bow_value=(np.float64, n_bow), cand_start=(np.int32, n + 1),
                  cand=(np.int32, n_cand), score_f64=(np.float64, L), score=(np.float32, L), min_score=(np.float32, n), present=(np.int32, n * M),
                  loop_query=(np.uint64, n * M), reloc_query=(np.uint64, n * M), loop_words=(np.int32, n * M), reloc_words=(np.int32, n * M),
                  loop_score=(np.float32, n * M), reloc_score=(np.float32, n * M))
    for key in OUT_KEYS:
        dt, cnt = shapes[key]
        out[key] = np.frombuffer(raw, dt, cnt, pos).copy()
        pos += cnt * np.dtype(dt).itemsize
        if key in OUT_KEYS[8:]:
            out[key] = out[key].reshape(n, M)
    assert pos == len(raw)
    return out
