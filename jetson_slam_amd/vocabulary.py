"""Vocabulary trees as flat host arrays, without DBoW2: what jsorb_vocabulary_create (include/jsorb.h) and orb.Vocabulary take.

A tree is a dict: n_nodes, depth_L, k, child_start int32[n_nodes + 1], children int32[n_nodes - 1], descriptors uint8[n_nodes, 32] (row 0, the
root's, unused), word_id int32[n_nodes] (-1 for inner nodes), weight float64[n_nodes].  Node 0 is the root; the children of node i are
children[child_start[i]:child_start[i + 1]] in the order of DBoW2's m_nodes[i].children.
  load_text(path)    the ORB-SLAM text format (TemplatedVocabulary::loadFromTextFile, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424)
  save_text(path, t) the same format written back (saveToTextFile, :1428-1457), for tests
  random_tree(...)   synthetic vocabularies for tests and tools/bow_bench.py
  sampled_tree(...)  a vocabulary built from a sample of real descriptors (random centres, Hamming assignment)
"""
import numpy as np


def _finish(parent, is_leaf, desc, weight, k, L):
    """the flat arrays from per-node parent ids (node ids 1.. in order, parent[0] unused): children in ascending node id, word ids in leaf order"""
    n = len(parent)
    parent = np.asarray(parent, np.int64)
    order = np.argsort(parent[1:], kind="stable") + 1            # children grouped by parent, ascending id inside a group
    counts = np.bincount(parent[1:], minlength=n)
    child_start = np.zeros(n + 1, np.int32)
    child_start[1:] = np.cumsum(counts)
    is_leaf = np.asarray(is_leaf, bool)
    word_id = np.full(n, -1, np.int32)
    word_id[is_leaf] = np.arange(int(is_leaf.sum()), dtype=np.int32)
    desc = np.array(desc, np.uint8).reshape(n, 32)
    desc[0] = 0                                                   # the root has no descriptor
    return dict(n_nodes=n, depth_L=int(L), k=int(k), child_start=child_start, children=order.astype(np.int32),
                descriptors=desc, word_id=word_id, weight=np.asarray(weight, np.float64))


def load_text(path):
    """first line `k L scoring weighting`; every further non-empty line `parent isLeaf b0 .. b31 weight`, node ids 1, 2, .. in line order, word ids
    in the order of the leaves (:1338-1424)"""
    with open(path) as f:
        head = f.readline().split()
        k, L = int(head[0]), int(head[1])
        rows = [ln.split() for ln in f if ln.strip()]
    n = len(rows) + 1
    parent = np.zeros(n, np.int64)
    is_leaf = np.zeros(n, bool)
    desc = np.zeros((n, 32), np.uint8)
    weight = np.zeros(n, np.float64)
    for i, r in enumerate(rows, 1):
        if len(r) != 35:
            raise ValueError("%s: line %d has %d fields, not 35" % (path, i + 1, len(r)))
        parent[i], is_leaf[i] = int(r[0]), int(r[1]) > 0
        desc[i] = [int(b) for b in r[2:34]]
        weight[i] = float(r[34])
    t = _finish(parent, is_leaf, desc, weight, k, L)
    t["scoring"], t["weighting"] = int(head[2]), int(head[3])
    return t


def save_text(path, t, scoring=0, weighting=0, weight_text=None, final_newline=True):
    """the text format of saveToTextFile; the tree's node ids must be in the format's order (every parent before its children).  The weights are
    written with repr (17 significant digits where a double needs them: load_text gives back the bits; saveToTextFile itself writes six), or as
    the strings weight_text[i] where given.  final_newline=False leaves the last line open: the reference's loader reads one more, empty, line
    after a final newline and makes a node of it (tests/bow_ref_cases.py)."""
    n = t["n_nodes"]
    parent = np.zeros(n, np.int64)
    for i in range(n):
        parent[t["children"][t["child_start"][i]:t["child_start"][i + 1]]] = i
    leaf = t["child_start"][1:] == t["child_start"][:-1]
    lines = ["%d %d %d %d" % (t["k"], t["depth_L"], scoring, weighting)]
    for i in range(1, n):
        w = weight_text[i] if weight_text is not None else repr(float(t["weight"][i]))
        lines.append("%d %d %s %s" % (parent[i], int(leaf[i]), " ".join(str(int(b)) for b in t["descriptors"][i]), w))
    with open(path, "w") as f:
        f.write("\n".join(lines) + ("\n" if final_newline else ""))


def random_tree(seed, k, L, ragged=False, tie=0.0, zero_weight=0.0, leaf_prob=0.25, max_nodes=None):
    """A vocabulary with random descriptors.  Uniform (ragged=False): every inner node has k children and every leaf lies at depth L - k = 10,
    L = 6 gives the ORB vocabulary's 1 111 111 nodes - built level by level, node ids in breadth-first order.  ragged: every inner node draws 1..k
    children and a node above depth L becomes a leaf with probability leaf_prob.  tie: the probability that a child's descriptor repeats an
    earlier sibling's (equal distances, decided by child order).  zero_weight: the probability that a leaf's weight is 0 (a stopped word).
    max_nodes (ragged): once the tree has this many nodes every new node is a leaf."""
    rng = np.random.default_rng(seed)
    if not ragged:
        sizes = [k ** l for l in range(L + 1)]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        n = int(offs[-1])
        parent = np.zeros(n, np.int64)
        for l in range(1, L + 1):
            parent[offs[l]:offs[l + 1]] = offs[l - 1] + np.arange(sizes[l]) // k
        is_leaf = np.zeros(n, bool)
        is_leaf[offs[L]:] = True
    else:
        parent, depth, is_leaf = [0], [0], [False]
        i = 0
        while i < len(parent):
            if not is_leaf[i]:
                for _ in range(int(rng.integers(1, k + 1))):
                    d = depth[i] + 1
                    parent.append(i)
                    depth.append(d)
                    is_leaf.append(d == L or rng.random() < leaf_prob or (max_nodes is not None and len(parent) >= max_nodes))
            i += 1
        n = len(parent)
        parent, is_leaf = np.asarray(parent, np.int64), np.asarray(is_leaf, bool)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if tie > 0:
        first = np.zeros(n, np.int64)              # the first child of each node's parent
        seen = {}
        for i in range(1, n):
            first[i] = seen.setdefault(int(parent[i]), i)
        dup = np.nonzero((rng.random(n) < tie) & (np.arange(n) > 0) & (first != np.arange(n)))[0]
        desc[dup] = desc[first[dup]]
    weight = np.where(is_leaf, rng.uniform(0.5, 9.0, n), 0.0)
    if zero_weight > 0:
        weight[is_leaf & (rng.random(n) < zero_weight)] = 0.0
    return _finish(parent, is_leaf, desc, weight, k, L)


def _hamming(a, b):
    """distances uint8[n, 32] x uint8[m, 32] -> int[n, m]"""
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(axis=2)


def sampled_tree(seed, descriptors, k, L):
    """A vocabulary from real descriptors: at every node k of the node's descriptors (distinct ones, drawn at random) become the children's
    descriptors and every descriptor goes to its nearest child (first wins a tie); a node at depth L or with fewer than two distinct descriptors
    is a leaf.  All weights 1."""
    rng = np.random.default_rng(seed)
    descriptors = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 32)
    parent, depth, desc, members = [0], [0], [np.zeros(32, np.uint8)], [np.arange(len(descriptors))]
    is_leaf = [False]
    i = 0
    while i < len(parent):
        m = members[i]
        uniq = np.unique(descriptors[m], axis=0) if len(m) else np.zeros((0, 32), np.uint8)
        if i > 0 and (depth[i] == L or len(uniq) < 2):
            is_leaf[i] = True
        else:
            if len(uniq) == 0:
                uniq = rng.integers(0, 256, (1, 32), dtype=np.uint8)
            centres = uniq[rng.choice(len(uniq), min(k, len(uniq)), replace=False)]
            near = np.argmin(_hamming(descriptors[m], centres), axis=1) if len(m) else np.zeros(0, np.int64)
            for c in range(len(centres)):
                parent.append(i)
                depth.append(depth[i] + 1)
                desc.append(centres[c])
                members.append(m[near == c])
                is_leaf.append(False)
        i += 1
    n = len(parent)
    return _finish(parent, is_leaf, np.stack(desc), np.where(np.asarray(is_leaf), 1.0, 0.0), k, L)
