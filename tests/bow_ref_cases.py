"""The BoW transform and the text vocabulary against the reference's own DBoW2 (tools/ref_bow/, tests/golden/ref_matcher_bow_transform.npz): the
worlds, the driver's file format, and the vector form of transform transcribed.

  world(name)       every world the recording holds (RECORDED): dict(mode "load" | "fill", text (the vocabulary file's bytes) | tree (flat
                    arrays, filled straight into m_nodes: the reference's loader refuses a header k > 20, :1359, and divides 0 by 0 for k = 1,
                    :1370-1372), scoring, weighting, levelsup [..], sets [uint8[n, 32], ..], phantom, n_file_nodes, shallow_ok, and what the
                    construction knows of the answer)
  run_driver(...)   a world through oracle/_ref/ref_bow in a process of its own -> the arrays tools/ref_bow/driver.cpp documents
  vector_form(...)  TemplatedVocabulary.h:1143-1193 for the four weightings with BowVector::addWeight / addIfNotExist / normalize and
                    FeatureVector::addFeature, literal and sequential, over the per-feature form's (word, weight, nid)
Two things the reference leaves undefined are kept out of every recorded value.  (1) `while(!f.eof()) getline` (:1378-1420) reads an empty line
after a final newline - which every file saveToTextFile writes has (:1445) - and makes a node of it whose parent and leaf flag were never read:
every vocabulary file here is written WITHOUT the final newline, and the one world with it records only the node count and the nodes before that
one.  (2) the vector form declares `NodeId nid;` without a value (:1151, :1179) and the per-feature form does not write it when the leaf lies above
level m_L - levelsup: the per-feature form is recorded with nid preset to SENTINEL, and the vector form is called only for sets in which no
non-stopped feature kept it.  The line numbers are TemplatedVocabulary.h's unless a file is named."""
import math
import os

import numpy as np

from jetson_slam_amd import vocabulary as V

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3                                 # BowVector.h:36-42
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)        # BowVector.h:45-53
# ScoringObject.h:74-89: (mustNormalize, the norm)
MUST_NORMALIZE = {L1_NORM: (True, 1), L2_NORM: (True, 2), CHI_SQUARE: (True, 1), KL: (True, 1), BHATTACHARYYA: (True, 1), DOT_PRODUCT: (False, 1)}
SENTINEL = 0xFFFFFFFF
COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 257)        # four descriptors per wave, sixteen per workgroup of k_bow_transform
MAX_BYTES = 500000
_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)


# ---- the vector form, :1143-1193 ----
def normalize(v, norm):
    """BowVector::normalize (BowVector.cpp:62-84) on a dict read in key order"""
    keys = sorted(v)
    total = 0.0                                                      # :64
    if norm == 1:
        for key in keys:
            total += abs(v[key])                                     # :70
    else:
        for key in keys:
            total += v[key] * v[key]                                 # :75
        total = math.sqrt(total)                                     # :76
    if total > 0.0:                                                  # :79
        for key in keys:
            v[key] /= total                                          # :82


def vector_form(word, weight, nid, weighting, scoring):
    """transform(features, v, fv, levelsup) given what transform(*fit, id, w, &nid, levelsup) returned per feature ->
    (words uint32[], values float64[], [(node, [feature indices])] in map order)"""
    must, norm = MUST_NORMALIZE[scoring]                             # :1140-1141
    v, fv = {}, {}
    if weighting in (TF, TF_IDF):                                    # :1145
        for i in range(len(word)):                                   # :1148
            wid, w = int(word[i]), float(weight[i])
            if w > 0:                                                # :1157
                if wid in v:                                         # addWeight, BowVector.cpp:34-46
                    v[wid] += w
                else:
                    v[wid] = w
                fv.setdefault(int(nid[i]), []).append(i)             # :1160, FeatureVector.cpp:31-45
        if v and not must:                                           # :1164
            nd = float(len(v))                                       # :1167
            for key in sorted(v):
                v[key] /= nd                                         # :1169
    else:                                                            # :1173
        for i in range(len(word)):                                   # :1176
            wid, w = int(word[i]), float(weight[i])
            if w > 0:                                                # :1185
                if wid not in v:                                     # addIfNotExist, BowVector.cpp:50-58
                    v[wid] = w
                fv.setdefault(int(nid[i]), []).append(i)             # :1188
    if must:
        normalize(v, norm)                                           # :1193
    keys = sorted(v)
    return np.array(keys, np.uint32), np.array([v[k] for k in keys], np.float64), [(k, fv[k]) for k in sorted(fv)]


# ---- building blocks of the worlds ----
def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _set_bits(positions):
    b = np.zeros(256, np.uint8)
    b[list(positions)] = 1
    return np.packbits(b)


def descend(tree, feats):
    """the leaf every feature ends in (the first of equal children) - used to CHOOSE inputs, never as an expectation"""
    cs, ch, D = tree["child_start"], tree["children"], tree["descriptors"]
    leaf = np.zeros(len(feats), np.int64)
    for i, f in enumerate(feats):
        cur = 0
        while cs[cur] != cs[cur + 1]:
            c = ch[cs[cur]:cs[cur + 1]]
            cur = int(c[np.argmin(_POP[D[c] ^ f[None, :]].sum(axis=1))])
        leaf[i] = cur
    return leaf


def flip(rng, rows, lo, hi):
    """every row with lo .. hi - 1 random bits flipped"""
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    nb = rng.integers(lo, hi, len(rows))
    rank = rng.random((len(rows), 256)).argsort(axis=1).argsort(axis=1)
    return rows ^ np.packbits((rank < nb[:, None]).astype(np.uint8), axis=1)


def near_features(rng, tree, n):
    """n descriptors, seven in ten of them a node's descriptor with 0..8 bits flipped"""
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n:
        near = rng.random(n) < 0.7
        src = tree["descriptors"][rng.integers(1, tree["n_nodes"], n)]
        desc[near] = flip(rng, src[near], 0, 9)
    return desc


def depths(tree):
    d = np.zeros(tree["n_nodes"], np.int64)
    for i in range(tree["n_nodes"]):                                 # ids ascend from parent to child in every tree built here
        d[tree["children"][tree["child_start"][i]:tree["child_start"][i + 1]]] = d[i] + 1
    return d


def parents(tree):
    p = np.full(tree["n_nodes"], -1, np.int32)
    for i in range(tree["n_nodes"]):
        p[tree["children"][tree["child_start"][i]:tree["child_start"][i + 1]]] = i
    return p


def no_shallow_leaf(tree):
    """every leaf lies at depth_L: no levelsup makes a shallow leaf"""
    leaf = tree["child_start"][1:] == tree["child_start"][:-1]
    return bool((depths(tree)[leaf] == tree["depth_L"]).all())


def text_of(tree, scoring, weighting, weight_text=None, final_newline=False):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "voc.txt")
        V.save_text(p, tree, scoring=scoring, weighting=weighting, weight_text=weight_text, final_newline=final_newline)
        return open(p, "rb").read()


def loader_fits(tree):
    """the loader reserves (k^(L+1) - 1) / (k - 1) nodes (:1370-1372); m_words points into m_nodes, so a file with more would leave them dangling"""
    k, L = tree["k"], tree["depth_L"]
    return 2 <= k <= 20 and 1 <= L <= 10 and tree["n_nodes"] <= (k ** (L + 1) - 1) // (k - 1)


def _world(mode, tree, sets, levelsup, scoring=L1_NORM, weighting=TF_IDF, shallow_ok=False, text=None, **more):
    w = dict(mode=mode, tree=tree, sets=[np.ascontiguousarray(s, np.uint8).reshape(-1, 32) for s in sets], levelsup=[int(x) for x in levelsup],
             scoring=scoring, weighting=weighting, shallow_ok=shallow_ok, phantom=False, text=None)
    if mode == "load":
        assert tree is None or loader_fits(tree)
        w["text"] = text if text is not None else text_of(tree, scoring, weighting)
    w.update(more)
    return w


# ---- tie worlds: every child of a node differs from d0 in one bit of its own, a feature in the bits of the children it is to tie ----
TIE_BASE = _set_bits(range(17, 117))
TIE_LEVEL_BIT = (0, 40)                          # child p at depth d differs from d0 in bit TIE_LEVEL_BIT[d - 1] + p


def tie_patterns(k):
    """sets of child positions a feature is equally near to: equal minima in different lanes (p % 16) and in the same lane, the first child in
    and out of them"""
    cand = [(0, k - 1), (1, 2), (3, k - 1), (2, 18), (1, 17, 32), (5, 21), (16, 32), (4, 9, 14), (k - 2, k - 1), (7,), (0, 16), (15, 16, 31)]
    out = []
    for c in cand:
        c = tuple(sorted(set(c)))
        if c and c[0] >= 0 and c[-1] < k and c not in out:
            out.append(c)
    return out or [(0,)]


def tie_tree(k):
    t = V.random_tree(3, k, 2)
    d = depths(t)
    for i in range(t["n_nodes"]):
        c = t["children"][t["child_start"][i]:t["child_start"][i + 1]]
        for p, node in enumerate(c):
            t["descriptors"][node] = TIE_BASE ^ _set_bits([TIE_LEVEL_BIT[d[node] - 1] + p])
    return t


def tie_world(k):
    """features d0 ^ (the bits of P1 at level 1) ^ (the bits of P2 at level 2) ^ 0..8 bits above 128: at level d the children in Pd are |Pd| - 1
    bits nearer than every other child and equally near - the first of them, min(Pd), must win.  expect_word: the word that choice leads to;
    chosen: (P1, P2) per feature."""
    t = tie_tree(k)
    rng = np.random.default_rng(100 + k)
    pats = tie_patterns(k)
    sets, expect, chosen = [], [], []
    for n in COUNTS[:-1]:
        rows, words = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint32)
        for i in range(n):
            p1, p2 = pats[rng.integers(len(pats))], pats[rng.integers(len(pats))]
            chosen.append((p1, p2))
            high = 128 + rng.choice(128, int(rng.integers(0, 9)), replace=False)
            rows[i] = TIE_BASE ^ _set_bits([TIE_LEVEL_BIT[0] + p for p in p1]) ^ _set_bits([TIE_LEVEL_BIT[1] + p for p in p2]) ^ _set_bits(high)
            n1 = t["children"][t["child_start"][0] + min(p1)]
            words[i] = t["word_id"][t["children"][t["child_start"][n1] + min(p2)]]
        sets.append(rows)
        expect.append(words)
    assert no_shallow_leaf(t)
    if loader_fits(t):
        return _world("load", t, sets, range(0, 4), expect_word=expect, chosen=chosen)
    return _world("fill", t, sets, range(0, 4), expect_word=expect, chosen=chosen)


# ---- trees with stopped words and shallow leaves ----
def ragged_world():
    t = V.random_tree(5, 7, 4, ragged=True, tie=0.4, zero_weight=0.2, max_nodes=300)
    rng = np.random.default_rng(205)
    return _world("load", t, [near_features(rng, t, n) for n in COUNTS], range(0, t["depth_L"] + 2), shallow_ok=True)


def chain_tree():
    """root -> 1 (one child) -> 2 -> 3 (leaf, depth 3); root -> 4 (leaf at depth 1, stopped); root -> 5 (leaf at depth 1)"""
    desc = np.stack([_set_bits([]), _set_bits([]), _set_bits(range(7)), _set_bits(range(9)), _set_bits(range(64, 128)), _set_bits(range(160, 224))])
    return V._finish([0, 0, 1, 2, 0, 0], [False, False, False, True, True, True], desc, np.array([0, 0, 0, 2.5, 0.0, 1.0]), 3, 3)


def chain_world():
    t = chain_tree()
    three = np.stack([_set_bits(range(3)), _set_bits(range(64, 124)), _set_bits(range(160, 220))])      # down the chain, the stopped leaf, the shallow leaf
    rng = np.random.default_rng(206)
    return _world("load", t, [three, three[:1], three[1:2], near_features(rng, t, 17)], (0, 1, 2, 3, 4, 9), shallow_ok=True)


# ---- the full tree, in every weighting, under an L1 norm, an L2 norm and no norm ----
FULL = [("tfidf_l1", TF_IDF, L1_NORM), ("tfidf_l2", TF_IDF, L2_NORM), ("tfidf_dot", TF_IDF, DOT_PRODUCT), ("tf_l1", TF, L1_NORM), ("tf_dot", TF, DOT_PRODUCT),
        ("idf_l2", IDF, L2_NORM), ("idf_dot", IDF, DOT_PRODUCT), ("binary_l1", BINARY, L1_NORM), ("binary_dot", BINARY, DOT_PRODUCT)]


def full_tree():
    return V.random_tree(21, 4, 3, zero_weight=0.15)


_full = []


def full_sets():
    """(built once) the COUNTS, then a set with a word once, a word twice and a word five times, then a set of stopped words only"""
    if _full:
        return _full[0]
    t = full_tree()
    rng = np.random.default_rng(207)
    sets = [near_features(rng, t, n) for n in COUNTS]
    pool = near_features(rng, t, 3000)
    leaf = descend(t, pool)
    live = [v for v in np.unique(leaf) if t["weight"][v] > 0 and (leaf == v).sum() >= 5]
    dead = [v for v in np.unique(leaf) if not t["weight"][v] > 0]
    assert len(live) >= 3 and len(dead) >= 2
    a, b, c = live[:3]
    pick = np.concatenate([np.nonzero(leaf == a)[0][:1], np.nonzero(leaf == c)[0][:3], np.nonzero(leaf == b)[0][:2], np.nonzero(leaf == c)[0][3:5]])
    sets.append(pool[pick])
    sets.append(pool[np.concatenate([np.nonzero(leaf == v)[0][:3] for v in dead[:2]])])
    _full.append((t, sets))
    return t, sets


def full_world(weighting, scoring):
    t, sets = full_sets()
    assert no_shallow_leaf(t)
    return _world("load", t, sets, (0, 1, 2, 3, 4), scoring=scoring, weighting=weighting, counted_set=len(COUNTS), stopped_set=len(COUNTS) + 1)


# ---- loader worlds ----
LOADER_A_WEIGHTS = {3: "0.5", 4: "0.1", 5: "1e-05", 6: "2.2204460492503131e-16", 7: "0.30000000000000004", 8: "0", 9: "123456.78901234567", 10: "7.5",
                    11: "0.69314718055994529"}


def loader_a_tree():
    """children in non-adjacent lines (the root's: 1, 2, 6; node 1's: 3, 5, 10; node 2's: 4, 9; node 3's: 7, 8, 11), a leaf above level L at depth
    1 (6) and at depth 2 (4, 5, 9, 10), an inner node that carries a weight (3), weights whose decimal strings are awkward"""
    parent = [0, 0, 0, 1, 2, 1, 0, 3, 3, 2, 1, 3]
    n = len(parent)
    is_leaf = ~np.isin(np.arange(n), parent[1:])
    is_leaf[0] = False
    rng = np.random.default_rng(208)
    text = ["0"] * n
    for i, s in LOADER_A_WEIGHTS.items():
        text[i] = s
    t = V._finish(parent, is_leaf, rng.integers(0, 256, (n, 32), dtype=np.uint8), np.array([float(s) for s in text]), 3, 3)
    return t, text


def loader_a_world(final_newline=False):
    t, wt = loader_a_tree()
    rng = np.random.default_rng(209)
    text = text_of(t, L2_NORM, IDF, weight_text=wt, final_newline=final_newline)
    if final_newline:
        return _world("load", t, [], [], scoring=L2_NORM, weighting=IDF, text=text, phantom=True, n_file_nodes=t["n_nodes"], shallow_ok=True)
    return _world("load", t, [near_features(rng, t, n) for n in (5, 17)], range(0, 5), scoring=L2_NORM, weighting=IDF, text=text, shallow_ok=True)


def preorder(t):
    """the same tree with its nodes numbered in depth-first order: a parent's children no longer lie in adjacent lines of the file"""
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        stack.extend(reversed([int(c) for c in t["children"][t["child_start"][i]:t["child_start"][i + 1]]]))
    new = np.zeros(t["n_nodes"], np.int64)
    new[order] = np.arange(t["n_nodes"])
    old_parent = parents(t)
    parent = [0] + [int(new[old_parent[i]]) for i in order[1:]]
    leaf = (t["child_start"][1:] == t["child_start"][:-1])[order]
    leaf[0] = False
    return V._finish(parent, leaf, t["descriptors"][order], t["weight"][order], t["k"], t["depth_L"])


def loader_b_world():
    t = preorder(V.random_tree(8, 5, 3, ragged=True, zero_weight=0.2, max_nodes=120))
    rng = np.random.default_rng(210)
    return _world("load", t, [near_features(rng, t, n) for n in (4, 16, 17)], (0, 1, 3), shallow_ok=True)


def flag_world():
    """node 4 has no children and is flagged isLeaf = 0: the reference's isLeaf() (:328) is true of it and its word_id stays the constructor's 0
    (:316), the id of node 2's word"""
    z = lambda seed: " ".join(str(int(b)) for b in np.random.default_rng(seed).integers(0, 256, 32))
    text = "2 2 0 0\n0 0 %s 0\n0 1 %s 1.5\n1 1 %s 0.25\n0 0 %s 0.75" % (z(1), z(2), z(3), z(4))
    return _world("load", None, [], [], text=text.encode(), shallow_ok=True)


# ---- a trained tree, and real frames ----
TRAINED = "surv_0_0"                             # the tests/vocab_train_cases.py world whose tree is written, loaded and walked


def trained_sets(w):
    """the training descriptors, a document a set (cut where a document holds more than 257)"""
    sets = []
    for d in range(len(w["doc_start"]) - 1):
        rows = w["feats"][w["doc_start"][d]:w["doc_start"][d + 1]]
        sets.extend(rows[i:i + 257] for i in range(0, max(len(rows), 1), 257))
    return sets


def trained_world(tree=None):
    """tree: the result of training (None: the reference's own tree of that world, tests/golden/ref_matcher_vocab_create.npz)"""
    import vocab_train_cases as vc
    w = vc.world(TRAINED)
    if tree is None:
        ref = vc.load_golden()[TRAINED]
        tree = dict(n_nodes=ref["n_nodes"], depth_L=w["L"], k=w["k"], child_start=ref["child_start"], children=ref["children"],
                    descriptors=ref["descriptors"].reshape(-1, 32), word_id=ref["word_id"], weight=ref["weight"])
    assert no_shallow_leaf(tree)
    return _world("load", tree, trained_sets(w), (0, 1, 3), scoring=L1_NORM, weighting=w["weighting"])


FRAME = dict(seed=3, h=120, w=160, L=4, tile=12, th=20)              # tiny_160x120_L4_t12 (tools/make_golden.py)
FRAME_TREE = dict(seed=7, k=4, L=3)


def frame_descriptors(po):
    """what the CPU oracle extracts from both images of the pair"""
    from jetson_slam_amd.synth import synth_stereo_pair
    c = FRAME
    out = []
    for img in synth_stereo_pair(c["seed"], c["h"], c["w"]):
        o = po.OracleExtractor(height=c["h"], width=c["w"], n_levels=c["L"], tile_h=c["tile"], tile_w=c["tile"], th_fast_max=c["th"])
        o.extract(img)
        out.append(np.asarray(o.descriptors(), np.uint8).reshape(-1, 32).copy())
    return out


def frame_world(descs=None):
    """descs: [left, right] (None: the file's in_desc_left / in_desc_right).  The tree is sampled from both images' descriptors; the weights
    are drawn (TF-IDF), one word in twenty stopped."""
    if descs is None:
        g = load_golden()["frame"]
        descs = [g["in_desc_left"], g["in_desc_right"]]
    t = V.sampled_tree(FRAME_TREE["seed"], np.concatenate(descs), FRAME_TREE["k"], FRAME_TREE["L"])
    rs = np.random.RandomState(4)
    leaf = t["word_id"] >= 0
    t["weight"] = np.where(leaf, rs.uniform(0.5, 9.0, len(leaf)) * (rs.rand(len(leaf)) > 0.05), 0.0)
    assert no_shallow_leaf(t)
    return _world("load", t, descs, (0, 1, 2, 3, 4))


BUILDERS = dict([("tie%d" % k, (lambda k=k: tie_world(k))) for k in (15, 16, 17, 33, 1)] +
                [("ragged", ragged_world), ("chain", chain_world)] +
                [("full_" + name, (lambda wt=wt, sc=sc: full_world(wt, sc))) for name, wt, sc in FULL] +
                [("loader_a", loader_a_world), ("loader_b", loader_b_world), ("newline", lambda: loader_a_world(final_newline=True)), ("flag", flag_world),
                 ("trained", trained_world), ("frame", frame_world)])
RECORDED = list(BUILDERS)
NO_SHALLOW = [n for n in RECORDED if n.startswith(("tie", "full_")) or n in ("trained", "frame")]       # nothing of these may be skipped
_cache = {}


def world(name):
    """built once per process; nobody changes a world"""
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def set_start(w):
    return np.cumsum([0] + [len(s) for s in w["sets"]]).astype(np.int32)


def runs(w):
    """(index of the (levelsup, set) pair, levelsup, set index, first feature, end) in the order of the recording"""
    ss, total = set_start(w), int(set_start(w)[-1])
    for j, lu in enumerate(w["levelsup"]):
        for s in range(len(w["sets"])):
            yield j * len(w["sets"]) + s, lu, s, j * total + int(ss[s]), j * total + int(ss[s + 1])


def recorded_vectors(rec, r):
    """the BowVector and FeatureVector of run r -> (words, value bits, [(node, [features])])"""
    b, e = rec["bow_start"][r], rec["bow_start"][r + 1]
    fv = []
    for q in range(rec["fvn_start"][r], rec["fvn_start"][r + 1]):
        fv.append((int(rec["fv_node"][q]), [int(x) for x in rec["fv_feat"][rec["fv_fstart"][q]:rec["fv_fstart"][q + 1]]]))
    return rec["bow_word"][b:e], rec["bow_bits"][b:e], fv


def tree_of_record(rec, depth_L=None):
    """the flat arrays of a recorded tree as orb.Vocabulary and load_text have them (word_id -1 where isLeaf() is false)"""
    k, L, scoring, weighting, n, n_words = (int(x) for x in rec["meta"])
    word = np.where(rec["is_leaf"] > 0, rec["word_id"].astype(np.int64), -1).astype(np.int32)
    word[0] = -1
    return dict(n_nodes=n, depth_L=L, k=k, scoring=scoring, weighting=weighting, child_start=rec["child_start"], children=rec["children"],
                descriptors=rec["descriptors"].reshape(n, 32), word_id=word, weight=rec["weight_bits"].view(np.float64))


def expected_nodes(rec, leaf_of_word):
    """the node ids of include/jsorb.h from the recording: -1 for a stopped word, the recorded nid where the reference wrote one (0 in the root
    case), the leaf's own id where the sentinel survived"""
    w = rec["t_weight_bits"].view(np.float64)
    nid = rec["t_nid"].astype(np.int64)
    own = np.asarray(leaf_of_word, np.int64)[rec["t_word"].astype(np.int64)] if len(nid) else nid
    return np.where(w > 0, np.where(nid == SENTINEL, own, nid), -1).astype(np.int32)


def leaf_of_word(tree):
    out = np.zeros(int(tree["word_id"].max()) + 1, np.int64)
    leaf = np.nonzero(tree["word_id"] >= 0)[0]
    out[tree["word_id"][leaf]] = leaf
    return out


# ---- the reference's own code, authoring machines only (tools/ref_bow/) ----
def _root():
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_path():
    return os.path.join(_root(), "tests", "golden", "ref_matcher_bow_transform.npz")


def reference_tree():
    """the reference tree, or None where it is absent"""
    ref = os.environ.get("JSORB_REFERENCE", "/root/reference")
    return ref if os.path.exists(os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2", "TemplatedVocabulary.h")) else None


def driver_path():
    return os.path.join(_root(), "oracle", "_ref", "ref_bow")


def build_driver(reference):
    """DBoW2's TemplatedVocabulary.h, FORB.cpp, BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp and DUtils' Random.cpp and Timestamp.cpp,
    unmodified, with tools/ref_bow's driver and tools/ref_vocab's stand-in for <opencv2/core/core.hpp>"""
    import subprocess
    tools = os.path.join(_root(), "tools")
    dbow = os.path.join(reference, "Thirdparty", "DBoW2")
    os.makedirs(os.path.dirname(driver_path()), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++14", "-O2", "-fno-fast-math", "-ffp-contract=off", "-w", "-I" + os.path.join(tools, "ref_vocab"), "-I" + dbow,
           "-o", driver_path(), os.path.join(tools, "ref_bow", "driver.cpp")]
    cmd += [os.path.join(dbow, "DBoW2", f) for f in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp")]
    cmd += [os.path.join(dbow, "DUtils", f) for f in ("Random.cpp", "Timestamp.cpp")]
    subprocess.check_call(cmd)
    return driver_path()


_TYPES = {b"i": np.int32, b"u": np.uint32, b"q": np.uint64, b"b": np.uint8}


def run_driver(w, workdir):
    """a world through the reference in a process of its own -> name -> array (tools/ref_bow/driver.cpp), or None when it died"""
    import subprocess
    src, dst, voc, saved = (os.path.join(workdir, f) for f in ("world.bin", "out.bin", "voc.txt", "saved.txt"))
    fill = w["mode"] == "fill"
    t = w["tree"]
    ss = set_start(w)
    n = w.get("n_file_nodes", t["n_nodes"] if t is not None else 0)
    with open(src, "wb") as f:
        f.write(np.array([int(fill), n, t["k"] if fill else 0, t["depth_L"] if fill else 0, w["scoring"], w["weighting"], len(w["sets"]), len(w["levelsup"]),
                          int(w["phantom"]), 0], np.int32).tobytes())
        if fill:
            for key, dt in (("child_start", np.int32), ("children", np.int32), ("descriptors", np.uint8), ("word_id", np.int32), ("weight", np.float64)):
                f.write(np.ascontiguousarray(t[key], dt).tobytes())
        f.write(np.array(w["levelsup"], np.int32).tobytes())
        f.write(ss.tobytes())
        f.write(np.concatenate([np.zeros((0, 32), np.uint8)] + w["sets"]).tobytes())
    for p in (dst, saved):
        if os.path.exists(p):
            os.remove(p)
    cmd = [driver_path(), src, dst]
    if not fill:
        open(voc, "wb").write(w["text"])
        cmd += [voc, saved]
    if subprocess.run(cmd, timeout=600).returncode != 0:
        return None
    raw, pos, out = open(dst, "rb").read(), 0, {}
    while pos < len(raw):
        ln = int(np.frombuffer(raw, np.uint32, 1, pos)[0])
        name = raw[pos + 4:pos + 4 + ln].decode()
        dt = _TYPES[raw[pos + 4 + ln:pos + 5 + ln]]
        cnt = int(np.frombuffer(raw, np.uint64, 1, pos + 5 + ln)[0])
        pos += 13 + ln
        out[name] = np.frombuffer(raw, dt, cnt, pos).copy()
        pos += cnt * np.dtype(dt).itemsize
    assert pos == len(raw)
    return out


def same_record(a, b):
    """None, or the first array in which two recordings differ"""
    if sorted(a) != sorted(b):
        return "keys %s" % sorted(set(a) ^ set(b))
    for key in sorted(a):
        if a[key].dtype != b[key].dtype or not np.array_equal(a[key], b[key]):
            return key
    return None


def save_golden(worlds):
    """name -> dict of arrays, as an npz with a fixed member order and no timestamps: regenerating gives the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(golden_path(), "w", zipfile.ZIP_DEFLATED) as z:
        for name in worlds:
            for key in sorted(worlds[name]):
                buf = io.BytesIO()
                np.save(buf, np.ascontiguousarray(worlds[name][key]), allow_pickle=False)
                z.writestr(zipfile.ZipInfo("%s.%s.npy" % (name, key), date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    return golden_path()


_golden = {}


def load_golden():
    """name -> dict of the reference's outputs (and, for the frame world, in_desc_left / in_desc_right), in the file's order; read once"""
    if not _golden:
        with np.load(golden_path()) as z:
            for member in z.files:
                name, key = member.split(".", 1)
                _golden.setdefault(name, {})[key] = z[member]
    return _golden


def outputs(g):
    """a world's entry of the file without its inputs"""
    return {k: v for k, v in g.items() if not k.startswith("in_")}
