"""-m gpu: k_bow_transform (jsorb_bow_transform_descriptors, jsorb_bow_transform_async) and the BowVector fold behind it (jsorb_bow_vector_async)
against what the reference's own TemplatedVocabulary::transform computed on vocabularies its own loadFromTextFile built
(tests/golden/ref_matcher_bow_transform.npz, DBoW2 compiled unmodified: tools/ref_bow/).  Every tree reaches the device through
orb.Vocabulary(load_text(the file the reference read)) - flat arrays where the reference's loader cannot read the tree (k > 20, k = 1).  Word ids,
node ids (include/jsorb.h's three definitions applied to the recorded nid), BowVector words and value bits: integers and f64 bit patterns."""
import numpy as np
import pytest

import bow_ref_cases as bc
from jetson_slam_amd import vocabulary as V
from test_gpu_search_local import _dev

pytestmark = pytest.mark.gpu

FULL_SAME = ["full_" + name for name, _, _ in bc.FULL[1:]]          # the first full world's tree and sets again: the per-feature form knows no weighting


@pytest.fixture(scope="module")
def golden():
    return bc.load_golden()


def device_tree(w, tmp_path):
    """the world's tree as the device gets it"""
    if w["mode"] == "fill":
        return w["tree"]
    p = str(tmp_path / "voc.txt")
    open(p, "wb").write(w["text"])
    return V.load_text(p)


def check_world(orb, w, g, tree, sets=None):
    """every recorded (levelsup, set): bow_transform_descriptors' ids, and for a TF-IDF / L1 world the device's BowVector of the device's word ids"""
    import torch
    want_node = bc.expected_nodes(g, bc.leaf_of_word(tree))
    fold = w["weighting"] == bc.TF_IDF and w["scoring"] == bc.L1_NORM
    voc = {lu: orb.Vocabulary(tree, levels_up=lu) for lu in sorted(set(w["levelsup"]))}
    db = orb.KeyframeDatabase(voc[w["levelsup"][0]], 1) if fold else None
    folded = 0
    try:
        for r, lu, s, b, e in bc.runs(w):
            desc = w["sets"][s]
            n = len(desc)
            word, node = orb.bow_transform_descriptors(voc[lu], _dev(desc) if n else torch.empty((0, 32), dtype=torch.uint8, device="cuda"))
            assert np.array_equal(word.cpu().numpy(), g["t_word"][b:e].astype(np.int32)), (lu, s)
            assert np.array_equal(node.cpu().numpy(), want_node[b:e]), (lu, s)
            if fold and g["v_ran"][r]:
                dw, dv, dc = db.bow_vector(word.contiguous() if n else torch.zeros(0, dtype=torch.int32, device="cuda"))
                rw, rb, _ = bc.recorded_vectors(g, r)
                cnt = int(dc.cpu()[0])
                assert cnt == len(rw) and np.array_equal(dw.cpu().numpy()[:cnt], rw.astype(np.int32)), (lu, s)
                assert np.array_equal(bc.bits(dv.cpu().numpy()[:cnt]), rb), (lu, s)
                folded += 1
    finally:
        if db is not None:
            db.close()
        for v in voc.values():
            v.close()
    return folded


@pytest.mark.parametrize("name", [n for n in bc.RECORDED if n not in FULL_SAME + ["newline", "flag", "trained"]])
def test_recorded_worlds(orb, golden, tmp_path, name):
    w, g = bc.world(name), golden[name]
    tree = device_tree(w, tmp_path)
    folded = check_world(orb, w, g, tree)
    assert (folded > 0) == (w["weighting"] == bc.TF_IDF and w["scoring"] == bc.L1_NORM), name


def test_the_other_full_worlds_are_the_first_again(golden):
    for name in FULL_SAME:
        for key in ("t_word", "t_weight_bits", "t_nid", "descriptors", "children", "child_start"):
            assert np.array_equal(golden[name][key], golden["full_" + bc.FULL[0][0]][key]), (name, key)


def test_a_childless_line_flagged_inner_is_refused(orb, tmp_path):
    t = device_tree(bc.world("flag"), tmp_path)
    with pytest.raises(orb.JsorbError, match="rc=-1"):
        orb.Vocabulary(t, levels_up=0)


def test_a_trained_tree_written_loaded_and_walked(orb, golden, tmp_path):
    """jsorb_vocabulary_train's tree through save_text is the very file the reference loaded; load_text, orb.Vocabulary and the transform of the
    training set give what the reference recorded for that file"""
    import vocab_train_cases as vc
    tw = vc.world(bc.TRAINED)
    trained = orb.train_vocabulary(tw["feats"], tw["doc_start"], tw["k"], tw["L"], weighting=tw["weighting"], seed=tw["seed"])
    w = bc.trained_world(trained)
    assert w["text"] == bc.world("trained")["text"]
    tree = device_tree(w, tmp_path)
    assert check_world(orb, w, golden["trained"], tree) > 0


def test_the_frame_world_through_the_handle(orb, golden, tmp_path):
    """both images extracted as a batch, jsorb_bow_transform_async(image = -1), jsorb_bow_vector_async on jsorb_bow_word_device: the reference's
    BowVector of each image, and the statistics"""
    import torch
    from jetson_slam_amd.synth import synth_stereo_pair
    c, g, w = bc.FRAME, golden["frame"], bc.world("frame")
    tree = device_tree(w, tmp_path)
    lu = 1
    j = w["levelsup"].index(lu)
    imgs = np.stack(synth_stereo_pair(c["seed"], c["h"], c["w"]))
    e = orb.ORBExtractor(c["h"], c["w"], 1.2, c["L"], 9, 14, 7, c["th"], None, c["tile"], c["tile"], max_batch=2)
    voc = orb.Vocabulary(tree, levels_up=lu)
    db = orb.KeyframeDatabase(voc, 2)
    try:
        dev = torch.from_numpy(imgs).cuda()
        e.extract_batch_device_async(dev.data_ptr(), c["h"] * c["w"], c["w"], 2, keep=dev)
        e.bow_transform(voc, image=-1)                                   # behind the lanes, before anything was waited for
        e.sync()
        want_node = bc.expected_nodes(g, bc.leaf_of_word(tree))
        db.set_stream(orb.load_library().jsorb_get_stream(e.handle))
        for i in range(2):
            assert np.array_equal(e.descriptors(i), w["sets"][i]), i     # the device's extract gives the descriptors the reference walked
            r = j * 2 + i
            b = j * int(bc.set_start(w)[-1]) + int(bc.set_start(w)[i])
            n = e.n_keypoints(i)
            word, node = e.bow(i)
            assert np.array_equal(word, g["t_word"][b:b + n].astype(np.int32)) and np.array_equal(node, want_node[b:b + n]), i
            vec = db.bow_vector(e.bow_device_pointers(i)[0], n=n, wait=False)
            db.sync()
            rw, rb, _ = bc.recorded_vectors(g, r)
            cnt = int(vec[2].cpu()[0])
            assert g["v_ran"][r] and cnt == len(rw) > 20 and np.array_equal(vec[0].cpu().numpy()[:cnt], rw.astype(np.int32)), i
            assert np.array_equal(bc.bits(vec[1].cpu().numpy()[:cnt]), rb), i
        total = int(bc.set_start(w)[-1])
        assert e.bow_transform_stats() == int((g["t_nid"][j * total:(j + 1) * total] == bc.SENTINEL).sum()) == 0
    finally:
        db.close(); voc.close(); e.close()
