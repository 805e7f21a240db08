"""tests/golden/ref_matcher_bow_transform.npz - what the reference's own TemplatedVocabulary::loadFromTextFile, saveToTextFile and both forms of
transform computed (DBoW2 compiled unmodified: tools/ref_bow/) - against the project's host side: the two statements of the per-feature form in
tests/test_bow_host.py, the vector form transcribed in tests/bow_ref_cases.py, kfdb_cases' BowVector fold, and vocabulary.load_text / save_text.
Where the reference tree is present the driver is built and run again, every world in a process of its own, and must reproduce the file.
Integers and f64 bit patterns only; no GPU."""
import os

import numpy as np
import pytest

import bow_ref_cases as bc
import kfdb_cases as kc
from jetson_slam_amd import vocabulary as V
from test_bow_host import transform_reference, transform_restated

TREE_KEYS = ["meta", "parent", "child_start", "children", "descriptors", "weight_bits", "word_id"]
LOAD_KEYS = TREE_KEYS + ["is_leaf", "words", "saved"]
TRANSFORM_KEYS = ["t_word", "t_weight_bits", "t_nid", "v_ran", "bow_start", "bow_word", "bow_bits", "fvn_start", "fv_node", "fv_fstart", "fv_feat"]


@pytest.fixture(scope="module")
def golden():
    return bc.load_golden()


def transformed(golden):
    return [n for n in golden if "t_word" in golden[n]]


def loaded(golden):
    return [n for n in golden if "saved" in golden[n]]


def same_tree(t, rec, n=None):
    """None, or the first thing in which load_text's tree differs from a recorded one (its first n nodes: the newline world)"""
    n = t["n_nodes"] if n is None else n
    if n != len(rec["parent"]):
        return "n_nodes"
    for key, a, b in (("parent", bc.parents(t), rec["parent"]), ("child_start", t["child_start"], rec["child_start"]), ("children", t["children"], rec["children"]),
                      ("descriptors", t["descriptors"].reshape(-1), rec["descriptors"]), ("weight", bc.bits(t["weight"]), rec["weight_bits"])):
        if not np.array_equal(np.asarray(a), b):
            return key
    return None


def test_the_file_is_small_and_holds_exactly_the_worlds_the_module_generates(golden):
    assert list(golden) == bc.RECORDED and os.path.getsize(bc.golden_path()) < bc.MAX_BYTES
    for name, g in golden.items():
        w = bc.world(name)
        want = (TREE_KEYS if w["phantom"] else LOAD_KEYS) if w["mode"] == "load" else []
        want = want + (TRANSFORM_KEYS if w["sets"] else []) + (["in_desc_left", "in_desc_right"] if name == "frame" else [])
        assert sorted(g) == sorted(want), name
        if w["sets"]:
            total, pairs = int(bc.set_start(w)[-1]), len(w["levelsup"]) * len(w["sets"])
            assert len(g["t_word"]) == len(g["t_nid"]) == len(g["t_weight_bits"]) == total * len(w["levelsup"]) and len(g["v_ran"]) == pairs, name
            assert max(len(s) for s in w["sets"]) <= 257 and w["tree"]["n_nodes"] <= (1 + 33 + 33 * 33 if name == "tie33" else 400), name
    assert {len(s) for n in ("ragged", "full_tfidf_l1") for s in bc.world(n)["sets"]} >= set(bc.COUNTS)
    assert {len(s) for s in bc.world("tie33")["sets"]} == set(bc.COUNTS[:-1])
    # the worlds that go past the loader are the ones it cannot read
    assert [n for n in golden if bc.world(n)["mode"] == "fill"] == ["tie33", "tie1"]


def test_the_driver_reproduces_the_file(golden, tmp_path):
    reference = bc.reference_tree()
    if reference is None:
        return                                   # no reference tree here: the file stands for it
    bc.build_driver(reference)
    for name, g in golden.items():
        got = bc.run_driver(bc.world(name), str(tmp_path))
        assert got is not None, name
        assert bc.same_record(bc.outputs(g), got) is None, (name, bc.same_record(bc.outputs(g), got))


def test_the_frame_worlds_descriptors_are_the_oracles(golden, po):
    for mine, stored in zip(bc.frame_descriptors(po), (golden["frame"]["in_desc_left"], golden["frame"]["in_desc_right"])):
        assert np.array_equal(mine, stored) and len(stored) > 100


def test_no_feature_is_skipped_where_none_may_be(golden):
    """the sentinel survives in no feature of the full-tree, tie, trained and frame worlds, and the vector form ran for every set of them; the
    ragged and chain worlds do hold shallow leaves, stopped words and the root case"""
    for name in bc.NO_SHALLOW:
        g = golden[name]
        assert int((g["t_nid"] == bc.SENTINEL).sum()) == 0 and g["v_ran"].all() and len(g["t_nid"]) > 0, name
    assert sorted(set(golden) - set(bc.NO_SHALLOW)) == ["chain", "flag", "loader_a", "loader_b", "newline", "ragged"]
    for name in ("ragged", "chain"):
        g, w = golden[name], bc.world(name)
        live = g["t_weight_bits"].view(np.float64) > 0
        kept = g["t_nid"] == bc.SENTINEL
        assert (kept & live).any() and (kept & ~live).any() and (~kept & ~live).any() and not g["v_ran"].all() and g["v_ran"].any(), name
        assert min(w["levelsup"]) == 0 and max(w["levelsup"]) > w["tree"]["depth_L"], name


def test_both_host_statements_give_the_recorded_words_and_nodes(golden):
    """word ids; node ids under the header's three definitions; n_shallow = the surviving sentinels - of the whole set (the statistic counts
    descriptors, stopped ones too) and, on the non-stopped features alone, of those"""
    full = [n for n in golden if n.startswith("full_")]
    for name in full[1:]:                            # one tree and one list of sets: the per-feature form knows no weighting
        for key in ("t_word", "t_weight_bits", "t_nid"):
            assert np.array_equal(golden[name][key], golden[full[0]][key]), (name, key)
    for name in transformed(golden):
        if name in full[1:]:
            continue
        g, w = golden[name], bc.world(name)
        tree = dict(w["tree"])
        want_node = bc.expected_nodes(g, bc.leaf_of_word(tree))
        weight = g["t_weight_bits"].view(np.float64)
        for r, lu, s, b, e in bc.runs(w):
            kept = g["t_nid"][b:e] == bc.SENTINEL
            live = weight[b:e] > 0
            for how in (transform_reference, transform_restated):
                word, node, n_shallow = how(tree, w["sets"][s], lu)
                assert np.array_equal(word, g["t_word"][b:e].astype(np.int32)), (name, lu, s, how.__name__)
                assert np.array_equal(node, want_node[b:e]), (name, lu, s, how.__name__)
                assert n_shallow == int(kept.sum()), (name, lu, s, how.__name__)
                assert how(tree, w["sets"][s][live], lu)[2] == int((kept & live).sum()), (name, lu, s, how.__name__)
            if tree["depth_L"] - lu <= 0:
                assert (g["t_nid"][b:e] == 0).all()                              # the root case is the reference's own (:1227)
        assert np.array_equal(g["t_weight_bits"], bc.bits(tree["weight"][bc.leaf_of_word(tree)[g["t_word"].astype(np.int64)]])), name


def test_only_the_first_of_equal_children_gives_the_recorded_words(golden):
    """the tie worlds by construction: the word under min(P1), min(P2); and each rule that is not `first wins` would give another word somewhere"""
    for k in (15, 16, 17, 33, 1):
        name = "tie%d" % k
        g, w = golden[name], bc.world(name)
        t = w["tree"]
        expect = np.concatenate(w["expect_word"])
        assert np.array_equal(g["t_word"], np.tile(expect, len(w["levelsup"]))), name
        if k == 1:
            continue
        pats = bc.tie_patterns(k)
        assert any(len(p) > 1 and len({q % 16 for q in p}) == len(p) for p in pats) and any(p[0] > 0 for p in pats), name
        if k > 16:
            assert any(len(p) > len({q % 16 for q in p}) for p in pats), name      # equal minima in one lane
        last = lambda P1, P2: t["word_id"][t["children"][t["child_start"][t["children"][t["child_start"][0] + max(P1)]] + max(P2)]]
        other = [last(p1, p2) for p1, p2 in w["chosen"]]
        assert (np.asarray(other) != expect).sum() > len(expect) // 2, name        # `last wins` is another answer for most features


def test_the_vector_form_transcribed_gives_the_recorded_vectors(golden):
    seen = set()
    for name in transformed(golden):
        g, w = golden[name], bc.world(name)
        weight = g["t_weight_bits"].view(np.float64)
        for r, lu, s, b, e in bc.runs(w):
            if not g["v_ran"][r]:
                assert name not in bc.NO_SHALLOW and g["bow_start"][r] == g["bow_start"][r + 1] and g["fvn_start"][r] == g["fvn_start"][r + 1]
                continue
            words, values, fv = bc.vector_form(g["t_word"][b:e], weight[b:e], g["t_nid"][b:e], w["weighting"], w["scoring"])
            rw, rb, rfv = bc.recorded_vectors(g, r)
            assert np.array_equal(words, rw) and np.array_equal(bc.bits(values), rb) and fv == rfv, (name, lu, s)
            if len(words):
                seen.add((w["weighting"], w["scoring"]))
            if w["weighting"] == bc.TF_IDF and w["scoring"] == bc.L1_NORM:           # the keyframe database's fold (tests/kfdb_cases.py) is this one
                ww = np.zeros(int(w["tree"]["word_id"].max()) + 1)
                leaf = w["tree"]["word_id"] >= 0
                ww[w["tree"]["word_id"][leaf]] = w["tree"]["weight"][leaf]
                kw, kv = kc.Transcription(dict(weight=ww, M=1)).fold(g["t_word"][b:e].astype(np.int32))
                assert np.array_equal(kw, rw.astype(np.int32)) and np.array_equal(bc.bits(kv), rb), (name, lu, s)
    assert seen == {(wt, sc) for _, wt, sc in bc.FULL} | {(bc.IDF, bc.L2_NORM), (bc.TF_IDF, bc.L1_NORM)}


def test_the_full_tree_worlds_hold_what_they_were_built_for(golden):
    for short, weighting, scoring in bc.FULL:
        g, w = golden["full_" + short], bc.world("full_" + short)
        per = len(w["sets"])
        assert bc.COUNTS[0] == 0 and g["bow_start"][0] == g["bow_start"][1]          # the empty set: an empty vector
        r = w["stopped_set"]
        b, e = int(bc.set_start(w)[r]), int(bc.set_start(w)[r + 1])
        assert e - b >= 4 and not (g["t_weight_bits"][b:e].view(np.float64) > 0).any() and g["bow_start"][r] == g["bow_start"][r + 1]
        assert g["fvn_start"][r] == g["fvn_start"][r + 1]
        r = w["counted_set"]
        b, e = int(bc.set_start(w)[r]), int(bc.set_start(w)[r + 1])
        counts = sorted(np.unique(g["t_word"][b:e], return_counts=True)[1])
        assert counts == [1, 2, 5] and (g["t_weight_bits"][b:e].view(np.float64) > 0).all()
        rw, rb, _ = bc.recorded_vectors(g, r)
        values = rb.view(np.float64)
        assert len(rw) == 3
        if scoring == bc.DOT_PRODUCT and weighting in (bc.TF, bc.TF_IDF):
            weight = {int(k): float(v) for k, v in zip(g["t_word"][b:e], g["t_weight_bits"][b:e].view(np.float64))}
            assert any(v != weight[int(k)] for k, v in zip(rw, values))              # /nd ran (:1164-1170)
        if scoring == bc.DOT_PRODUCT and weighting in (bc.IDF, bc.BINARY):
            weight = {int(k): float(v) for k, v in zip(g["t_word"][b:e], g["t_weight_bits"][b:e].view(np.float64))}
            assert all(v == weight[int(k)] for k, v in zip(rw, values))              # no norm at all: the weight once
        assert per == len(bc.COUNTS) + 2


def write(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(bytes(data))
    return p


def test_load_text_gives_the_tree_the_references_loader_built(golden, tmp_path):
    names = [n for n in loaded(golden) if n != "flag"]
    assert "loader_a" in names and "loader_b" in names and "trained" in names and "frame" in names and "tie17" in names and "tie33" not in names
    for name in names:
        g, w = golden[name], bc.world(name)
        t = V.load_text(write(tmp_path, name + ".txt", w["text"]))
        assert not w["text"].endswith(b"\n") and same_tree(t, g) is None, (name, same_tree(t, g))
        assert [t["k"], t["depth_L"], t["scoring"], t["weighting"], t["n_nodes"], int((t["word_id"] >= 0).sum())] == [int(x) for x in g["meta"]], name
        assert np.array_equal(t["child_start"][1:] == t["child_start"][:-1], g["is_leaf"] > 0), name       # here the flags agree with the structure
        assert np.array_equal(t["word_id"], bc.tree_of_record(g)["word_id"]) and np.array_equal(bc.leaf_of_word(t), g["words"]), name
        assert same_tree(w["tree"], g) is None and np.array_equal(w["tree"]["word_id"], t["word_id"]), name
    # the awkward weights arrive as the nearest doubles of their strings
    t, text = bc.loader_a_tree()
    assert [float(s) for s in text] == list(golden["loader_a"]["weight_bits"].view(np.float64)) and "2.2204460492503131e-16" in text
    assert float("2.2204460492503131e-16") == 2.0 ** -52 and float("0.30000000000000004") != 0.3
    d = bc.depths(t)
    leaf = t["word_id"] >= 0
    assert (d[leaf] < t["depth_L"]).any() and list(t["children"][:3]) == [1, 2, 6]            # a leaf above level L; children in non-adjacent lines


def test_load_text_of_what_the_reference_saved(golden, tmp_path):
    """saveToTextFile's own bytes: the same tree, the weights as their six significant digits parse; and the final newline it writes (:1445)"""
    for name in loaded(golden):
        g = golden[name]
        saved = bytes(g["saved"])
        assert saved.endswith(b"\n") and saved.count(b"\n") == int(g["meta"][4])
        t = V.load_text(write(tmp_path, name + ".saved.txt", saved))
        want = dict(g, weight_bits=bc.bits([float("%g" % x) for x in g["weight_bits"].view(np.float64)]))
        assert same_tree(t, want) is None, (name, same_tree(t, want))
        assert [t["k"], t["depth_L"], t["scoring"], t["weighting"]] == [int(x) for x in g["meta"][:4]], name
        # the reference writes isLeaf() (:1440), so its own files never disagree with the structure
        assert np.array_equal(t["word_id"] >= 0, g["is_leaf"] > 0), name
    assert (golden["loader_a"]["weight_bits"] != bc.bits([float("%g" % x) for x in golden["loader_a"]["weight_bits"].view(np.float64)])).sum() >= 3


def test_save_text_then_load_text_is_the_identity_on_bits(golden, tmp_path):
    for name in loaded(golden):
        if name == "flag":
            continue
        w = bc.world(name)
        t = V.load_text(write(tmp_path, name + ".txt", w["text"]))
        for final_newline in (False, True):
            p = str(tmp_path / (name + ".again.txt"))
            V.save_text(p, t, scoring=t["scoring"], weighting=t["weighting"], final_newline=final_newline)
            assert open(p, "rb").read().endswith(b"\n") == final_newline
            u = V.load_text(p)
            assert same_tree(u, golden[name]) is None and np.array_equal(u["word_id"], t["word_id"]), name
            assert [u[k] for k in ("k", "depth_L", "scoring", "weighting", "n_nodes")] == [t[k] for k in ("k", "depth_L", "scoring", "weighting", "n_nodes")]


def test_a_final_newline_gives_the_reference_one_node_more(golden, tmp_path):
    """the loader reads the empty line after the last newline as a node (:1378-1420): one node more than the file has, the nodes before it the
    file's.  Nothing of that node is recorded; load_text skips empty lines"""
    g, w = golden["newline"], bc.world("newline")
    n = w["n_file_nodes"]
    assert w["text"].endswith(b"\n") and w["text"][:-1] == bc.world("loader_a")["text"]
    assert int(g["meta"][4]) == n + 1 and int(g["meta"][5]) == -1
    t = V.load_text(write(tmp_path, "newline.txt", w["text"]))
    assert t["n_nodes"] == n and same_tree(t, g) is None, same_tree(t, g)
    a = golden["loader_a"]
    for key in ("parent", "child_start", "children", "descriptors", "weight_bits", "word_id"):
        assert np.array_equal(g[key], a[key]), key


def test_a_childless_line_flagged_inner(golden, tmp_path, orb):
    """the reference: isLeaf() is true of node 4 and its word_id is the constructor's 0, node 2's word - a descriptor that ends there is counted
    as word 0.  load_text keeps the flag (no word), and the library refuses such a tree rather than walk it"""
    g, w = golden["flag"], bc.world("flag")
    assert list(g["is_leaf"]) == [0, 0, 1, 1, 1] and list(g["word_id"]) == [0, 0, 0, 1, 0] and list(g["words"]) == [2, 3] and int(g["meta"][5]) == 2
    assert list(g["parent"]) == [-1, 0, 0, 1, 0] and g["weight_bits"][4] == bc.bits([0.75])[0]
    t = V.load_text(write(tmp_path, "flag.txt", w["text"]))
    assert list(t["word_id"]) == [-1, -1, 0, 1, -1] and t["child_start"][4] == t["child_start"][5] and same_tree(t, g) is None
    with pytest.raises(orb.JsorbError, match="rc=-1"):                           # JSORB_ERR_INVALID: a leaf without a word - before any device is touched
        orb.Vocabulary(t, levels_up=0)
