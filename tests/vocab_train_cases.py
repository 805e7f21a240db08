"""Vocabulary training (jsorb_vocabulary_train, include/jsorb.h) without the library: worlds, and TemplatedVocabulary::create twice over.

  transcribe(...)  Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:557-996 line by line: the recursion of HKmeansStep, node ids as m_nodes grows,
                   createWords, setNodeWeights - with the contract's two changes: the draws come from draw(seed, first, size, j), and a cluster
                   without members keeps its centre (the reference's meanValue releases it and the next distance reads through a null pointer)
  levelwise(...)   the device's method restated in numpy: all runs of a level iterate together until no descriptor of the level moves, the nodes
                   are made in level order and renumbered afterwards.  `mutant` breaks one rule at a time (tests/test_vocab_train_host.py).
Both return the arrays of jsorb_vocab_train_result_copy, the statistics of jsorb_vocab_train_stats and `leaf`, the node each descriptor's path ends
in.  The line numbers are TemplatedVocabulary.h's unless a file is named."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
RAND_MAX = 2 ** 31 - 1
DEFAULT_MAX_ITERATIONS = 1000
TINY = (64, 64)                                  # the tiny_vocab_train build (jetson_slam_amd/build.py VARIANTS): chunk, scan tile
_M = (1 << 64) - 1
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)
MUTANTS = ("assoc_le", "mean_gt", "mean_half", "cut_gt", "shared_draws", "bfs_ids", "ni_per_descriptor")


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M
    return x ^ (x >> 31)


def draw(seed, first, size, j):
    """the j-th 31-bit value of the run whose first descriptor is input index `first` (include/jsorb.h)"""
    return mix((mix((seed ^ ((first << 32) | size)) & _M) + j) & _M) >> 33


def random_int(r, lo, hi):
    """DUtils/Random.cpp:47-50"""
    d = hi - lo + 1
    return int((float(r) / (float(RAND_MAX) + 1.0)) * d) + lo


def random_value(r, lo, hi):
    """DUtils/Random.h:55-69"""
    return (float(r) / float(RAND_MAX)) * (hi - lo) + lo


def distance(rows, centre):
    """FORB::distance (FORB.cpp:81-101) of every row to one descriptor"""
    return _POP[rows ^ centre[None, :]].sum(axis=1)


def mean_value(rows, mutant=None):
    """FORB::meanValue (FORB.cpp:28-77); None for no rows (the reference releases the mean).  Second value: a bit's count was exactly N2."""
    n = len(rows)
    if n == 0:
        return None, False
    if n == 1:
        return rows[0].copy(), False
    s = np.unpackbits(rows, axis=1).sum(axis=0)
    n2 = n // 2 + n % 2
    if mutant == "mean_half":
        n2 = n // 2
    bits = s > n2 if mutant == "mean_gt" else s >= n2
    return np.packbits(bits.astype(np.uint8)), bool((s == n2).any())


class _Draws:
    """the j-th value of a run; `shared`: one counter over all runs (a mutant)"""

    def __init__(self, seed, shared):
        self.seed, self.shared, self.j_all, self.total = seed, shared, 0, 0

    def run(self, first, size):
        state = {"j": 0}

        def nxt():
            j = self.j_all if self.shared else state["j"]
            state["j"] += 1
            self.j_all += 1
            self.total += 1
            return draw(self.seed, first, size, j)
        return nxt


def seed_clusters(D, k, nxt, cov, mutant=None):
    """initiateClustersKMpp (:832-913) on the run's descriptors D (ascending input order)"""
    n = len(D)
    clusters = [D[random_int(nxt(), 0, n - 1)].copy()]                 # :855-858
    min_dists = distance(D, clusters[-1]).astype(np.float64)           # :864-867
    redraw = False
    while len(clusters) < k:                                           # :869
        dist = distance(D, clusters[-1])
        min_dists = np.minimum(min_dists, dist)                        # :872-880 (the > 0 test is a shortcut: a distance is never negative)
        dist_sum = float(min_dists.sum())                              # :883, exact: integers below 2^53
        if not dist_sum > 0:
            cov["seeding_stops_early"] += 1
            break                                                      # :908-909
        while True:                                                    # :888-891
            cut_d = random_value(nxt(), 0, dist_sum)
            if cut_d != 0.0:
                break
            redraw = True
        up = np.cumsum(min_dists)                                      # :893-898
        hit = np.nonzero(up > cut_d if mutant == "cut_gt" else up >= cut_d)[0]
        ifeature = n - 1 if len(hit) == 0 else int(hit[0])             # :900-903
        clusters.append(D[ifeature].copy())
    if len(clusters) == k and not redraw:
        cov["seeding_full_no_redraw"] += 1
    return clusters


def associate(D, clusters, cov, mutant=None):
    """:732-751: the nearest cluster, the first of equals"""
    dist = np.stack([distance(D, c) for c in clusters], axis=1)
    best = dist.min(axis=1)
    if ((dist == best[:, None]).sum(axis=1) > 1).any():
        cov["association_tie"] += 1
    if mutant == "assoc_le":
        return dist.shape[1] - 1 - np.argmin(dist[:, ::-1], axis=1)
    return np.argmin(dist, axis=1)


def new_cov():
    return {key: 0 for key in ("seeding_full_no_redraw", "seeding_stops_early", "trivial", "n_is_k_plus_1", "leaf_above_L", "single_child_chain",
                               "association_tie", "mean_bit_at_threshold", "four_passes", "word_in_fewer_docs", "empty_cluster")}


def kmeans_run(D, first, k, draws, max_iterations, cov, mutant=None):
    """the while loop of HKmeansStep (:675-781) -> clusters, association, passes, moved in the last pass"""
    nxt = draws.run(first, len(D))
    clusters = seed_clusters(D, k, nxt, cov, mutant)
    last, passes = None, 0
    while True:
        if last is not None:                                           # :692-717
            for c in range(len(clusters)):
                mean, at = mean_value(D[last == c], mutant)
                cov["mean_bit_at_threshold"] += int(at)
                if mean is not None:
                    clusters[c] = mean
        cur = associate(D, clusters, cov, mutant)
        passes += 1
        goon = last is None or bool((cur != last).any())               # :756-772
        if not goon or passes == max_iterations:
            break
        last = cur                                                     # :774-779
    if passes >= 4:
        cov["four_passes"] += 1
    return clusters, cur, passes, goon


def _finish(parent, desc, feats, doc_start, k, L, weighting, leaf_of, stats, cov, mutant=None):
    """createWords (:917-938) and setNodeWeights (:942-996) on nodes given by parent ids (every parent before its children)"""
    n = len(parent)
    parent = np.asarray(parent, np.int32)
    order = np.argsort(parent[1:], kind="stable") + 1
    counts = np.bincount(parent[1:], minlength=n)
    child_start = np.zeros(n + 1, np.int32)
    child_start[1:] = np.cumsum(counts)
    children = order.astype(np.int32)
    is_leaf = counts == 0
    is_leaf[0] = False
    word_id = np.full(n, -1, np.int32)
    word_id[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.int32)
    desc = np.asarray(desc, np.uint8).reshape(n, 32)
    # transform (:1217-1259) of every training descriptor
    word = np.zeros(len(feats), np.int64)
    stack = [(0, np.arange(len(feats)))]
    while stack:
        node, idx = stack.pop()
        ch = children[child_start[node]:child_start[node + 1]]
        if len(ch) == 0:
            word[idx] = word_id[node]
            continue
        near = np.argmin(np.stack([distance(feats[idx], desc[c]) for c in ch], axis=1), axis=1)
        for i, c in enumerate(ch):
            if (near == i).any():
                stack.append((int(c), idx[near == i]))
    n_words, n_docs = int(is_leaf.sum()), len(doc_start) - 1
    ni_word = np.zeros(n_words, np.int64)
    for d in range(n_docs):                                            # :968-983
        w = word[doc_start[d]:doc_start[d + 1]]
        if mutant == "ni_per_descriptor":
            ni_word += np.bincount(w, minlength=n_words)
        else:
            ni_word[np.unique(w)] += 1
    if (ni_word < n_docs).any() and n_docs >= 3:
        cov["word_in_fewer_docs"] += 1
    weight, ni = np.zeros(n, np.float64), np.zeros(n, np.int32)
    for v in np.nonzero(is_leaf)[0]:
        c = int(ni_word[word_id[v]])
        ni[v] = c
        if weighting in (TF, BINARY):
            weight[v] = 1.0                                            # :949-954
        elif c > 0:
            weight[v] = math.log(float(n_docs) / float(c))             # :990
    out = dict(n_nodes=n, depth_L=int(L), k=int(k), parent=parent, child_start=child_start, children=children, descriptors=desc, word_id=word_id,
               weight=weight, Ni=ni, leaf=np.asarray(leaf_of, np.int32), transform_word=word.astype(np.int32), coverage=cov)
    out["parent"][0] = -1
    out.update(stats)
    return out


def transcribe(feats, doc_start, k, L, weighting=TF_IDF, seed=0, max_iterations=0, mutant=None):
    feats = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
    max_iterations = max_iterations or DEFAULT_MAX_ITERATIONS
    cov = new_cov()
    draws = _Draws(seed, mutant == "shared_draws")
    parent, desc, level_of, single = [-1], [np.zeros(32, np.uint8)], [0], [False]
    leaf_of = np.zeros(len(feats), np.int64)
    stats = dict(n_kmeans_runs=0, n_empty_clusters=0, n_unconverged=0, lloyd_passes=[0] * 16)

    def step(parent_id, idx, level):                                   # HKmeansStep (:641-819)
        D = feats[idx]
        if len(idx) <= k:                                              # :660-670
            cov["trivial"] += 1
            clusters, assoc = [D[i].copy() for i in range(len(idx))], np.arange(len(idx))
        else:
            if len(idx) == k + 1:
                cov["n_is_k_plus_1"] += 1
            clusters, assoc, passes, moving = kmeans_run(D, int(idx[0]), k, draws, max_iterations, cov, mutant)
            stats["n_kmeans_runs"] += 1
            stats["n_unconverged"] += int(moving)
            stats["lloyd_passes"][level - 1] = max(stats["lloyd_passes"][level - 1], passes)
            empty = sum(1 for c in range(len(clusters)) if not (assoc == c).any())
            stats["n_empty_clusters"] += empty
            cov["empty_cluster"] += empty
        ids = []
        for c in clusters:                                             # :785-793
            ids.append(len(parent))
            parent.append(parent_id); desc.append(c); level_of.append(level)
        single.extend([len(ids) == 1] * len(ids))
        if len(ids) == 1 and single[parent_id]:
            cov["single_child_chain"] += 1
        for c, node in enumerate(ids):                                 # :796-818
            members = idx[assoc == c]
            if level < L and len(members) > 1:
                step(node, members, level + 1)
            else:
                leaf_of[members] = node
                if level < L:
                    cov["leaf_above_L"] += 1
    step(0, np.arange(len(feats)), 1)
    stats["n_draws"] = draws.total
    return _finish(parent, desc, feats, doc_start, k, L, weighting, leaf_of, stats, cov, mutant)


def levelwise(feats, doc_start, k, L, weighting=TF_IDF, seed=0, max_iterations=0, mutant=None):
    """the device's order of work: a level's runs side by side, one association pass of all of them at a time"""
    feats = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
    max_iterations = max_iterations or DEFAULT_MAX_ITERATIONS
    cov = new_cov()
    draws = _Draws(seed, mutant == "shared_draws")
    tparent, tdesc, tchildren = [-1], [np.zeros(32, np.uint8)], [[]]
    leaf_t = np.zeros(len(feats), np.int64)
    stats = dict(n_kmeans_runs=0, n_empty_clusters=0, n_unconverged=0, lloyd_passes=[0] * 16)
    segs = [(0, np.arange(len(feats)))]
    level = 1
    while segs:
        runs = []
        for node, idx in segs:
            D = feats[idx]
            if len(idx) <= k:
                runs.append(dict(D=D, clusters=[D[i].copy() for i in range(len(idx))], assoc=np.arange(len(idx)), seeded=False, moved=False))
            else:
                nxt = draws.run(int(idx[0]), len(idx))
                runs.append(dict(D=D, clusters=seed_clusters(D, k, nxt, cov, mutant), assoc=None, seeded=True, moved=True))
        seeded = [r for r in runs if r["seeded"]]
        passes = 0
        while seeded:
            passes += 1
            for r in seeded:
                cur = associate(r["D"], r["clusters"], cov, mutant)
                r["moved"] = r["assoc"] is None or bool((cur != r["assoc"]).any())
                r["assoc"] = cur
            if not any(r["moved"] for r in seeded) or passes == max_iterations:
                break
            for r in seeded:
                for c in range(len(r["clusters"])):
                    mean, _ = mean_value(r["D"][r["assoc"] == c], mutant)
                    if mean is not None:
                        r["clusters"][c] = mean
        stats["lloyd_passes"][level - 1] = passes
        nxt_segs = []
        for (node, idx), r in zip(segs, runs):
            if r["seeded"]:
                stats["n_kmeans_runs"] += 1
                stats["n_unconverged"] += int(r["moved"])
                stats["n_empty_clusters"] += sum(1 for c in range(len(r["clusters"])) if not (r["assoc"] == c).any())
            for c, centre in enumerate(r["clusters"]):
                child = len(tparent)
                tparent.append(node); tdesc.append(centre); tchildren.append([]); tchildren[node].append(child)
                members = idx[r["assoc"] == c]
                if level < L and len(members) > 1:
                    nxt_segs.append((child, members))
                else:
                    leaf_t[members] = child
        segs = nxt_segs
        level += 1
    # DBoW2's ids: a run's clusters are consecutive, then the recursion into each in turn (:785-818)
    new_id = np.zeros(len(tparent), np.int64)
    if mutant == "bfs_ids":
        new_id = np.arange(len(tparent))
    else:
        nxt_id = [1]

        def number(u):
            for c in tchildren[u]:
                new_id[c] = nxt_id[0]
                nxt_id[0] += 1
            for c in tchildren[u]:
                if tchildren[c]:
                    number(c)
        number(0)
    old = np.argsort(new_id)
    parent = [-1] + [int(new_id[tparent[u]]) for u in old[1:]]
    desc = [tdesc[u] for u in old]
    stats["n_draws"] = draws.total
    return _finish(parent, desc, feats, doc_start, k, L, weighting, new_id[leaf_t], stats, cov, mutant)


TREE_KEYS = ("parent", "child_start", "children", "descriptors", "word_id", "Ni")
STAT_KEYS = ("n_kmeans_runs", "n_draws", "n_empty_clusters", "n_unconverged", "lloyd_passes")


def same_tree(a, b, stats=True):
    """None, or the first thing in which two results differ (the weights by their bits)"""
    if a["n_nodes"] != b["n_nodes"]:
        return "n_nodes %d != %d" % (a["n_nodes"], b["n_nodes"])
    for key in TREE_KEYS:
        if not np.array_equal(np.asarray(a[key]), np.asarray(b[key])):
            return key
    if not np.array_equal(np.asarray(a["weight"], np.float64).view(np.uint64), np.asarray(b["weight"], np.float64).view(np.uint64)):
        return "weight"
    if stats:
        for key in STAT_KEYS:
            if list(np.atleast_1d(a[key])) != list(np.atleast_1d(b[key])):
                return key
    return None


# ---- worlds ----
def clustered(seed, n, nb, flips):
    """n descriptors, each one of nb random bases (drawn with replacement) with f random bits flipped, f uniform in [0, flips]"""
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    rows = bases[rng.integers(0, nb, n)]
    if flips > 0:
        f = rng.integers(0, flips + 1, n)
        rank = rng.random((n, 256)).argsort(axis=1).argsort(axis=1)
        rows = rows ^ np.packbits((rank < f[:, None]).astype(np.uint8), axis=1)
    return np.ascontiguousarray(rows, np.uint8)


def documents(seed, n, n_docs):
    """n_docs + 1 ascending offsets from 0 to n (documents may be empty)"""
    rng = np.random.default_rng(seed + 77)
    cuts = np.sort(rng.integers(0, n + 1, n_docs - 1))
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


# the families the reference's own create() survives on (n, k, L, nb, flips), and the tight ones it dies on (an empty cluster)
SURVIVING = [(600, 3, 3, 600, 0), (2000, 10, 2, 2000, 0), (20000, 10, 3, 20000, 0), (4000, 4, 3, 200, 30), (4000, 4, 3, 400, 60), (1500, 3, 4, 100, 80),
             (1500, 5, 2, 300, 20)]
TIGHT = [(600, 3, 3, 8, 40), (600, 3, 3, 8, 120), (2000, 4, 3, 20, 100), (5000, 10, 3, 50, 128), (300, 2, 4, 6, 60)]


def degenerate():
    """name -> (descriptors, k, L): the degenerate cases the reference survives"""
    rng = np.random.default_rng(5)
    one = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    vals = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    return {
        "identical_50": (np.repeat(one, 50, axis=0), 3, 3),
        "two_values": (vals[rng.integers(0, 2, 40)], 3, 3),
        "three_values": (vals[rng.integers(0, 3, 60)], 5, 3),
        "n_below_k": (rng.integers(0, 256, (5, 32), dtype=np.uint8), 10, 3),
        "eleven_of_seven": (vals[np.array([0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3])], 10, 2),
        "four_identical": (np.repeat(one, 4, axis=0), 3, 3),
        "single": (one.copy(), 4, 2),
    }


def world(name):
    """name -> dict(feats, doc_start, k, L, weighting, seed): every world the tests run"""
    if name.startswith(("surv", "tight")):
        fam, i, s = name.split("_")
        n, k, L, nb, flips = (SURVIVING if fam == "surv" else TIGHT)[int(i)]
        feats = clustered(1000 * int(i) + int(s), n, nb, flips)
        return dict(feats=feats, doc_start=documents(int(s), n, 7), k=k, L=L, weighting=(int(i) + int(s)) % 4, seed=0x1234 + int(s))
    feats, k, L = degenerate()[name]
    n = len(feats)
    return dict(feats=feats, doc_start=documents(1, n, min(4, n)), k=k, L=L, weighting=TF_IDF, seed=99)


def empty_cluster_world():
    """a world in which a cluster loses all its members: the first of 64 seeds of the tightest family for which the transcription counts one"""
    for s in range(64):
        w = world("tight_0_%d" % s)
        if transcribe(**w)["n_empty_clusters"] > 0:
            return w
    raise AssertionError("no world with an empty cluster among 64 seeds of the tight family")


def constructed():
    """name -> world: cases built around one decision each.
    cut_is_sum: the seed whose second draw of the run (0, 3) is RAND_MAX, so cut_d == dist_sum exactly: over a, b, a with the first centre at index 2
                min_dists is 0, d, 0 and `>=` picks b (index 1) where `>` finds nothing and takes the last feature, a again
    redraw:     the seed whose second draw of the run (0, 3) is 0: cut_d == 0.0 and a third value is drawn"""
    rng = np.random.default_rng(11)
    a, b, c = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    docs = np.array([0, 1, 2, 3], np.int32)
    return {
        "cut_is_sum": dict(feats=np.stack([a, b, a]), doc_start=docs, k=2, L=1, weighting=TF_IDF, seed=894004914),
        "redraw": dict(feats=np.stack([a, b, c]), doc_start=docs, k=2, L=1, weighting=IDF, seed=145830026),
    }


def world_any(name):
    c = constructed()
    return c[name] if name in c else world(name)


RECORDED = ["surv_%d_%d" % (i, s) for i in range(len(SURVIVING)) for s in (0, 1)] + list(degenerate()) + list(constructed())
TIGHT_NAMES = ["tight_%d_0" % i for i in range(len(TIGHT))]


# ---- the reference's own create(), authoring machines only (tools/ref_vocab/) ----
def _root():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_path():
    import os
    return os.path.join(_root(), "tests", "golden", "ref_matcher_vocab_create.npz")


def reference_tree():
    """the reference tree, or None where it is absent"""
    import os
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if os.path.exists(os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2", "TemplatedVocabulary.h")) else None


def driver_path():
    import os
    return os.path.join(_root(), "oracle", "_ref", "ref_vocab")


def build_driver(reference):
    """DBoW2's TemplatedVocabulary.h, FORB.cpp, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp and DUtils' Random.cpp and Timestamp.cpp,
    unmodified, with tools/ref_vocab's driver and its stand-in for <opencv2/core/core.hpp>"""
    import os
    import subprocess
    shadow = os.path.join(_root(), "tools", "ref_vocab")
    dbow = os.path.join(reference, "Thirdparty", "DBoW2")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-fno-fast-math", "-ffp-contract=off", "-w", "-I" + shadow, "-I" + dbow, "-o", driver_path(),
           os.path.join(shadow, "driver.cpp")]
    cmd += [os.path.join(dbow, "DBoW2", f) for f in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp")]
    cmd += [os.path.join(dbow, "DUtils", f) for f in ("Random.cpp", "Timestamp.cpp")]
    subprocess.check_call(cmd)
    return driver_path()


REF_KEYS = ("parent", "descriptors", "weight", "word_id", "child_start", "children")


def run_driver(w, workdir):
    """a world through the reference in a process of its own -> dict(REF_KEYS, n_nodes, n_kmeans_runs, n_draws), or None when it died"""
    import os
    import subprocess
    src, dst = os.path.join(workdir, "world.bin"), os.path.join(workdir, "out.bin")
    feats = np.ascontiguousarray(w["feats"], np.uint8).reshape(-1, 32)
    ds = np.ascontiguousarray(w["doc_start"], np.int32)
    with open(src, "wb") as f:
        f.write(np.array([len(feats), len(ds) - 1, w["k"], w["L"], w["weighting"], 0], np.int32).tobytes())
        f.write(np.array([w["seed"]], np.uint64).tobytes())
        f.write(ds.tobytes())
        f.write(feats.tobytes())
    if os.path.exists(dst):
        os.remove(dst)
    if subprocess.run([driver_path(), src, dst], timeout=600).returncode != 0:
        return None
    raw = open(dst, "rb").read()
    n, runs = (int(x) for x in np.frombuffer(raw, np.int32, 2))
    out = dict(n_nodes=n, n_kmeans_runs=runs, n_draws=int(np.frombuffer(raw, np.int64, 1, 8)[0]))
    pos = 16
    for key, dt, cnt in (("parent", np.int32, n), ("descriptors", np.uint8, 32 * n), ("weight", np.float64, n), ("word_id", np.int32, n),
                         ("child_start", np.int32, n + 1), ("children", np.int32, n - 1)):
        out[key] = np.frombuffer(raw, dt, cnt, pos).copy()
        pos += cnt * np.dtype(dt).itemsize
    assert pos == len(raw)
    out["descriptors"] = out["descriptors"].reshape(n, 32)
    return out


def ni_from_weights(ref, w):
    """Ni per node from the reference's idf weights, checked: math.log(NDocs / Ni) must give the weight's bits.  -1 where the weight is 0, which
    Ni = NDocs and Ni = 0 (:988-991) both give.  None for TF and BINARY."""
    if w["weighting"] in (TF, BINARY):
        return None
    n_docs = len(w["doc_start"]) - 1
    ni = np.zeros(ref["n_nodes"], np.int32)
    for v in np.nonzero(ref["word_id"] >= 0)[0]:
        if ref["weight"][v] == 0:
            ni[v] = -1
            continue
        c = int(round(n_docs / math.exp(ref["weight"][v])))
        assert 1 <= c <= n_docs and np.float64(math.log(float(n_docs) / float(c))).view(np.uint64) == ref["weight"][v:v + 1].view(np.uint64)[0], (v, c)
        ni[v] = c
    return ni


def same_as_reference(ref, got):
    """None, or the first of the reference's outputs a result differs in (weights as bits, Ni where the weighting shows it)"""
    if ref["n_nodes"] != got["n_nodes"]:
        return "n_nodes"
    for key in REF_KEYS:
        a, b = np.asarray(ref[key]), np.asarray(got[key])
        if key == "weight":
            a, b = a.astype(np.float64).view(np.uint64), b.astype(np.float64).view(np.uint64)
        if not np.array_equal(a.reshape(-1), b.reshape(-1)):
            return key
    if "Ni" in ref and not np.array_equal(ref["Ni"][ref["Ni"] >= 0], np.asarray(got["Ni"])[ref["Ni"] >= 0]):
        return "Ni"
    for key in ("n_kmeans_runs", "n_draws"):
        if int(ref[key]) != int(got[key]):
            return key
    return None


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
    """name -> dict of the reference's outputs (REF_KEYS, Ni where the weighting shows it, the scalars as ints), in the file's order"""
    out = {}
    with np.load(golden_path()) as z:
        for member in z.files:
            name, key = member.rsplit(".", 1)
            v = z[member]
            out.setdefault(name, {})[key] = int(v.reshape(-1)[0]) if key in ("n_nodes", "n_kmeans_runs", "n_draws") else v
    return out
