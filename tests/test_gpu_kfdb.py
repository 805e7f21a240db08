"""-m gpu: the keyframe database on the device (jsorb_keyframe_database_*, jsorb_bow_vector_async, jsorb_detect_*_candidates*; k_kfdb.hip) against
what the reference's own KeyFrameDatabase.cpp, BowVector.cpp and ScoringObject.cpp computed (tests/golden/ref_matcher_kfdb.npz) and against the
sequential transcription of tests/kfdb_cases.py: every world's whole script - BowVectors (words, value bits, count), scores as float and as double,
min_score, candidates in order, the statistics and the persistent state after every operation - bit for bit, with the shipped caps and under the
tiny_kfdb build, whose queries are searched in global memory and whose word ids are sorted there."""
import ctypes

import numpy as np
import pytest

import kfdb_cases as kc
from test_gpu_search_local import _dev

pytestmark = pytest.mark.gpu


class DevVec(tuple):
    """a device BowVector that reads like the host pair (words, values): what kfdb_cases.run stores"""
    dev = None


class Device:
    """the library behind the methods kfdb_cases.run plays a world through"""

    def __init__(self, orb, world, sync=False, chain=False):
        import torch
        self.torch, self.M, self.sync, self.chain = torch, int(world["M"]), sync, chain
        self.db = orb.KeyframeDatabase(world["weight"], self.M)

    def close(self):
        self.db.close()

    def fold(self, feats):
        word, value, count = self.db.bow_vector(_dev(np.asarray(feats, np.int32)) if len(feats) else self.torch.zeros(0, dtype=self.torch.int32, device="cuda"))
        n = int(count.cpu()[0])
        assert 0 <= n <= len(feats)
        v = DevVec((word.cpu().numpy()[:n].copy(), value.cpu().numpy()[:n].copy()))
        v.dev = (word, value, count)
        return v

    def add(self, slot, vec):
        self.db.add(slot, vec.dev)

    def erase(self, slot):
        self.db.erase(slot)

    def clear(self):
        self.db.clear()

    def score(self, vec, slots):
        s, d, m = self.db.score(vec.dev, _dev(np.asarray(slots, np.int32)) if len(slots) else self.torch.zeros(0, dtype=self.torch.int32, device="cuda"))
        return d.cpu().numpy(), s.cpu().numpy(), m.cpu().numpy()[0]

    def detect(self, reloc, vec, qid, connected, neigh, min_score):
        nb = _dev(np.asarray(neigh, np.int32))
        if reloc:
            r = self.db.detect_relocalization_candidates(vec.dev, qid, nb, sync=self.sync)
        else:
            ms = _dev(np.array([min_score], np.float32)) if self.chain else float(min_score)
            r = self.db.detect_loop_candidates(vec.dev, qid, nb, min_score=ms, connected=_dev(np.asarray(connected, np.uint8)), sync=self.sync)
        out = [int(x) for x in r] if self.sync else [int(x) for x in r[0].cpu().numpy()[:int(r[1].cpu()[0])]]
        st = self.db.stats()
        assert st["n_candidates"] == len(out)
        st["order"] = []
        return out, st

    def state(self):
        st = self.db.state()
        for k in st:
            if k != "present":
                st[k][st["present"] == 0] = 0
        return st


@pytest.fixture(scope="module")
def golden():
    """name -> (the world, the reference's outputs, the transcription's outputs): read and computed once, never changed"""
    out = {}
    for name, g in kc.load_golden().items():
        out[name] = (g, {k: g["out_" + k] for k in kc.OUT_KEYS}, kc.run(g, kc.Transcription(g)))
    return out


@pytest.fixture
def tiny(orb, monkeypatch):
    """the tiny_kfdb build as the library behind `orb`"""
    from jetson_slam_amd import build as jb
    monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_kfdb", *jb.VARIANTS["tiny_kfdb"])))
    assert orb.kfdb_build_caps() == kc.TINY                              # the library in use is the build the test means
    return orb


def worlds_through(orb, golden, names, **kw):
    for name in names:
        world, ref, mine = golden[name]
        d = Device(orb, world, **kw)
        try:
            got = kc.run(world, d)
        finally:
            d.close()
        assert kc.same(ref, got) is None, (name, kc.same(ref, got))
        assert kc.same(mine, got, ("stats", "best_acc")) is None, (name, kc.same(mine, got, ("stats", "best_acc")))


def test_constructed_worlds_give_the_reference(orb, golden):
    assert orb.kfdb_build_caps() == kc.SHIPPED
    names = [n for n in golden if n.startswith("c_")]
    assert len(names) == len(kc.constructed())
    worlds_through(orb, golden, names)


def test_constructed_worlds_tiny(tiny, golden):
    worlds_through(tiny, golden, [n for n in golden if n.startswith("c_")])


@pytest.mark.parametrize("seed", kc.BLOCK_SEEDS)
def test_random_block_gives_the_reference(orb, golden, seed):
    worlds_through(orb, golden, ["random_%d" % seed])


@pytest.mark.parametrize("seed", kc.BLOCK_SEEDS)
def test_random_block_tiny(tiny, golden, seed):
    """queries of more than 16 words are searched in global memory, frames of more than 64 features sorted there: most of a block's"""
    world = golden["random_%d" % seed][0]
    r = kc.Restatement(world, kc.TINY)
    kc.run(world, r)
    assert min(r.paths.values()) > 0, r.paths
    worlds_through(tiny, golden, ["random_%d" % seed])


def test_synchronous_forms_and_device_min_score(orb, golden):
    """the host-output forms, and min_score read from a device pointer, give what the asynchronous host-value forms give"""
    worlds_through(orb, golden, ["random_%d" % kc.BLOCK_SEEDS[0], "c_si_equals_min_score_kept", "c_acc_equals_retain_dropped"], sync=True)
    worlds_through(orb, golden, ["random_%d" % kc.BLOCK_SEEDS[1], "c_si_equals_min_score_kept", "c_si_below_min_score_dropped"], chain=True)


def test_min_score_chains_into_the_loop_query_with_no_wait(orb, golden):
    """DetectLoop's shape: score over the covisible keyframes, then the query reading min_score_dev - enqueued back to back on the database's
    stream, one wait at the end - against the two calls with a host value in between"""
    world = golden["random_%d" % kc.BLOCK_SEEDS[2]][0]
    t = kc.Transcription(world)
    d = Device(orb, world)
    try:
        adds = [i for i in range(len(world["op_kind"])) if world["op_kind"][i] == kc.ADD][:12]
        for i in adds:
            feats = world["feat"][world["op_feat_start"][i]:world["op_feat_start"][i + 1]]
            d.add(int(world["op_slot"][i]), d.fold(feats))
            t.add(int(world["op_slot"][i]), t.fold(feats))
        slots = [int(world["op_slot"][i]) for i in adds]
        i = adds[3]
        feats = world["feat"][world["op_feat_start"][i]:world["op_feat_start"][i + 1]]
        q, tq = d.fold(feats), t.fold(feats)
        cov, connected = slots[:4], np.zeros(d.M, np.uint8)
        connected[cov] = 1
        nb = np.full((d.M, 10), -1, np.int32)
        nb[slots[5], :3] = slots[6:9]
        _, _, want_min = t.score(tq, cov)
        want, _ = t.detect(False, tq, 77, connected, nb, want_min)
        s, _, m = d.db.score(q.dev, _dev(np.array(cov, np.int32)), wait=False)
        cand, n = d.db.detect_loop_candidates(q.dev, 77, _dev(nb), min_score=m, connected=_dev(connected), wait=False)
        d.db.sync()
        assert kc.bits(m.cpu().numpy())[0] == kc.bits(np.array([want_min]))[0]
        assert [int(x) for x in cand.cpu().numpy()[:int(n.cpu()[0])]] == want and len(want) > 0
    finally:
        d.close()


def test_query_behind_the_bow_transform_of_an_extracted_frame(orb, configs):
    """pixels to candidates: extract, jsorb_bow_transform_async, jsorb_bow_vector_async on the frame's device word ids, the relocalisation query -
    the word ids never cross to the host on the way; the host fold of the copied ids gives the same vector and the same candidates"""
    import torch
    from jetson_slam_amd.synth import synth_stereo_pair
    from test_bow_host import REAL_SEED, sampled_voc
    from test_gpu_search_local import _mk
    c = configs["c1"]
    images = list(synth_stereo_pair(REAL_SEED, c["h"], c["w"])) + [synth_stereo_pair(REAL_SEED + 1, c["h"], c["w"])[0]]
    e = _mk(orb, c)
    e.extract(images[0])
    tree = sampled_voc(e.descriptors())
    leaf = tree["word_id"] >= 0
    rs = np.random.RandomState(4)
    tree["weight"] = np.where(leaf, rs.uniform(0.5, 9.0, len(leaf)) * (rs.rand(len(leaf)) > 0.05), 0.0)      # TF-IDF weights, some words stopped
    v = orb.Vocabulary(tree, levels_up=1)
    db = orb.KeyframeDatabase(v, 8)
    try:
        vecs = []
        db.set_stream(orb.load_library().jsorb_get_stream(e.handle))      # the database's work goes behind the handle's
        for k in range(3):
            e.extract(images[k])
            assert orb.load_library().jsorb_bow_transform_async(e.handle, 0, v.handle) == 0
            n = e.n_keypoints()
            vec = db.bow_vector(e.bow_device_pointers()[0], n=n, wait=False)
            db.add(k, vec, wait=False)
            db.sync()
            words, _ = e.bow()
            hw, hv = kc.fold(v.word_weight, words)
            cnt = int(vec[2].cpu()[0])
            assert n > 100 and cnt == len(hw) and np.array_equal(vec[0].cpu().numpy()[:cnt], hw)
            assert np.array_equal(kc.bits(vec[1].cpu().numpy()[:cnt]), kc.bits(hv))
            vecs.append((words, vec))
        nb = torch.full((8, 10), -1, dtype=torch.int32, device="cuda")
        got = db.detect_relocalization_candidates(vecs[1][1], 5, nb, sync=True)
        w = kc.Script(v.word_weight, 8)
        for k in range(3):
            w.add(k, vecs[k][0])
        w = w.reloc(vecs[1][0], 5).world()
        want = kc.candidates(kc.run(w, kc.Transcription(w)), 3)
        assert list(got) == want and 1 in want
    finally:
        db.close(); e.close(); v.close()


def test_detect_loop_example(orb, tmp_path):
    """examples/detect_loop.cpp: DetectLoop up to the candidates and Relocalization up to SearchByBoW through the shim, checked against its host loop"""
    import subprocess
    from jetson_slam_amd import build as jb
    exe = jb.build_example("detect_loop", str(tmp_path / "detect_loop"))
    out = subprocess.run([exe], timeout=120, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "self-check ok" in out.stdout and "loop: minScore=" in out.stdout and "relocalization: candidates=" in out.stdout


def test_argument_errors_launch_nothing(orb):
    import torch
    lib = orb.load_library()
    db = orb.KeyframeDatabase(np.ones(16), 4)
    try:
        vec = db.bow_vector(_dev(np.array([1, 2, 2, 5], np.int32)))
        db.add(1, vec)
        before = db.state()
        nb = torch.full((4, 10), -1, dtype=torch.int32, device="cuda")
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        out, n = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.full((1,), -7, dtype=torch.int32, device="cuda")
        h = db.handle
        bad = [
            lambda: lib.jsorb_keyframe_database_add_async(h, 1, P(vec[0]), P(vec[1]), 4, P(vec[2])),         # a present slot
            lambda: lib.jsorb_keyframe_database_add_async(h, 4, P(vec[0]), P(vec[1]), 4, P(vec[2])),         # slots outside [0, 4)
            lambda: lib.jsorb_keyframe_database_add_async(h, -1, P(vec[0]), P(vec[1]), 4, P(vec[2])),
            lambda: lib.jsorb_keyframe_database_add_async(h, 2, None, P(vec[1]), 4, P(vec[2])),              # NULL arrays
            lambda: lib.jsorb_keyframe_database_add_async(h, 2, P(vec[0]), P(vec[1]), 4, None),
            lambda: lib.jsorb_keyframe_database_erase(h, 9),
            lambda: lib.jsorb_bow_vector_async(h, None, 3, P(vec[0]), P(vec[1]), P(vec[2])),
            lambda: lib.jsorb_bow_vector_async(h, P(vec[0]), -1, P(vec[0]), P(vec[1]), P(vec[2])),
            lambda: lib.jsorb_keyframe_database_score_async(h, P(vec[0]), P(vec[1]), 4, P(vec[2]), None, 2, None, None, P(n)),
            lambda: lib.jsorb_keyframe_database_score_async(h, P(vec[0]), P(vec[1]), 4, P(vec[2]), P(out), 2, P(out), None, None),
            lambda: lib.jsorb_detect_loop_candidates_async(h, P(vec[0]), P(vec[1]), 4, P(vec[2]), 3, None, None, 0.0, None, P(out), P(n)),
            lambda: lib.jsorb_detect_loop_candidates_async(h, P(vec[0]), P(vec[1]), 4, P(vec[2]), 3, None, P(nb), 0.0, None, None, P(n)),
            lambda: lib.jsorb_detect_relocalization_candidates_async(h, P(vec[0]), P(vec[1]), 4, None, 3, P(nb), P(out), P(n)),
            lambda: lib.jsorb_detect_relocalization_candidates(h, P(vec[0]), P(vec[1]), 4, P(vec[2]), 3, P(nb), None, None),
        ]
        for i, call in enumerate(bad):
            assert call() == -1, i                                    # JSORB_ERR_INVALID
            assert len(lib.jsorb_keyframe_database_last_error(h)) > 10, i
        db.sync()
        after = db.state()
        assert all(np.array_equal(before[k], after[k]) for k in before) and int(n.cpu()[0]) == -7 and db.size() == 1
        with pytest.raises(orb.JsorbError):
            db.stats()                                                # no query has run: JSORB_ERR_STATE
    finally:
        db.close()


def test_empty_database_and_empty_inputs(orb):
    """n = 0, an empty query and a database nothing was added to: counts of zero, min_score 1, nothing read"""
    import torch
    db = orb.KeyframeDatabase(np.ones(16), 4)
    try:
        empty = db.bow_vector(torch.zeros(0, dtype=torch.int32, device="cuda"))
        assert int(empty[2].cpu()[0]) == 0
        nb = torch.full((4, 10), -1, dtype=torch.int32, device="cuda")
        vec = db.bow_vector(_dev(np.array([3, 3, 9], np.int32)))
        for q in (empty, vec):
            assert list(db.detect_loop_candidates(q, 1, nb, sync=True)) == [] and list(db.detect_relocalization_candidates(q, 1, nb, sync=True)) == []
            assert db.stats()["n_sharing"] == 0
            s, d, m = db.score(q, torch.zeros(0, dtype=torch.int32, device="cuda"))
            assert float(m.cpu()[0]) == 1.0
        db.add(0, empty)
        db.add(2, vec)
        assert list(db.detect_relocalization_candidates(empty, 2, nb, sync=True)) == []
        assert list(db.detect_relocalization_candidates(vec, 3, nb, sync=True)) == [2]
        db.clear()
        assert db.size() == 0 and list(db.detect_relocalization_candidates(vec, 4, nb, sync=True)) == []
    finally:
        db.close()
