"""-m gpu: jsorb_vocabulary_train (k_vocab_train.hip, jsorb_vocab_train.hip) against the line-by-line transcription of TemplatedVocabulary::create in
tests/vocab_train_cases.py, bit for bit - the tree, Ni, the weights, the node every descriptor ends in and the statistics - with the shipped library
and under the tiny_vocab_train build (chunks of 64 positions, 64 chunk sums per scan tile): the tight families the reference dies on, a world with
an empty cluster, the iteration cap, the text round trip, training on the extractor's own device-resident descriptors, an external stream, and
every refusal.  The worlds the reference itself survives are in tests/test_gpu_ref_vocab.py."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import vocab_train_cases as vc
from jetson_slam_amd.synth import synth_image

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["shipped", "tiny"])
def lib_orb(request, orb, monkeypatch):
    """`orb` with the shipped library or the tiny_vocab_train build behind it"""
    from jetson_slam_amd import build as jb
    if request.param == "tiny":
        monkeypatch.setattr(orb, "_lib", orb.load_library(jb.build_variant("tiny_vocab_train", *jb.VARIANTS["tiny_vocab_train"])))
        assert orb.vocab_train_build_caps() == vc.TINY                  # the library in use is the build the test means
    else:
        assert orb.vocab_train_build_caps() == (1024, 1024)
    return orb


def train(orb, w, **kw):
    args = dict(w, **kw)
    return orb.train_vocabulary(args.pop("feats"), args.pop("doc_start"), args.pop("k"), args.pop("L"), **args)


def check(got, want, name):
    assert vc.same_tree(want, got) is None, (name, vc.same_tree(want, got))
    assert np.array_equal(got["leaf"], want["leaf"]), name
    leaf = got["word_id"] >= 0
    n_docs = None
    for v in np.nonzero(leaf)[0]:                                        # the weights against math.log on this machine
        if got["weighting"] in (vc.TF, vc.BINARY):
            assert got["weight"][v] == 1.0
        else:
            n_docs = n_docs or want["n_docs"]
            assert got["weight"][v] == (math.log(float(n_docs) / float(got["Ni"][v])) if got["Ni"][v] > 0 else 0.0), (name, v)
    assert not got["weight"][~leaf].any() and not got["Ni"][~leaf].any()


def expected(w, **kw):
    t = vc.transcribe(**dict(w, **kw))
    t["n_docs"] = len(w["doc_start"]) - 1
    return t


def test_tight_families_and_an_empty_cluster(lib_orb):
    worlds = {name: vc.world(name) for name in vc.TIGHT_NAMES}
    worlds["empty_cluster"] = vc.empty_cluster_world()
    empties = 0
    for name, w in worlds.items():
        want = expected(w)
        got = train(lib_orb, w)
        check(got, want, name)
        empties += got["n_empty_clusters"]
    assert empties > 0 and train(lib_orb, worlds["empty_cluster"])["n_empty_clusters"] > 0


def test_iteration_cap(lib_orb):
    for cap in (1, 3):
        w = vc.world("surv_0_0")
        want = expected(w, max_iterations=cap)
        got = train(lib_orb, w, max_iterations=cap)
        check(got, want, cap)
        assert got["n_unconverged"] > 0 and max(got["lloyd_passes"]) == cap


def test_text_round_trip_and_the_transform(lib_orb, tmp_path):
    """save_text -> load_text -> orb.Vocabulary; the transform of the training set ends in the leaves of the final association (a converged
    run is a fixed point; the worlds have no duplicate descriptors in a trivial run) and gives Ni again"""
    import torch
    from jetson_slam_amd import vocabulary as voc
    for name in ("surv_5_0", "surv_3_1"):
        w = vc.world(name)
        t = train(lib_orb, w)
        assert t["n_unconverged"] == 0
        path = str(tmp_path / (name + ".txt"))
        voc.save_text(path, t, scoring=t["scoring"], weighting=t["weighting"])
        back = voc.load_text(path)
        for key in ("child_start", "children", "descriptors", "word_id"):
            assert np.array_equal(back[key], t[key]), key
        assert np.array_equal(back["weight"].view(np.uint64), t["weight"].view(np.uint64)) and back["weighting"] == w["weighting"]
        v = lib_orb.Vocabulary(back, levels_up=0)
        word, _ = lib_orb.bow_transform_descriptors(v, torch.from_numpy(w["feats"]).cuda())
        word = word.cpu().numpy()
        v.close()
        assert np.array_equal(word, t["word_id"][t["leaf"]])
        ds = w["doc_start"]
        ni = np.zeros(t["n_words"], np.int64)
        for d in range(len(ds) - 1):
            ni[np.unique(word[ds[d]:ds[d + 1]])] += 1
        assert np.array_equal(ni, t["Ni"][t["word_id"] >= 0])


def extracted(orb, seeds):
    """the descriptors of synthetic frames, device to device from the handle's buffers into one tensor; one document per image"""
    import torch
    lib = orb.load_library()
    g = orb.ORBExtractor(240, 320, 1.2, 3, 9, 14, 7, 20, None, 15, 15)
    parts, doc_start = [], [0]
    for s in seeds:
        g.extract(synth_image(s, 240, 320))
        n = g.n_keypoints(0)
        part = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
        assert lib.jsorb_mem_d2d(ctypes.c_void_p(part.data_ptr()), ctypes.c_void_p(lib.jsorb_descriptors_device(g.handle, 0)), ctypes.c_size_t(32 * n)) == 0
        parts.append(part)
        doc_start.append(doc_start[-1] + n)
    lib.jsorb_mem_device_sync()
    return torch.cat(parts).contiguous(), np.asarray(doc_start, np.int32)


def test_extractor_descriptors_and_seeds(lib_orb):
    import torch
    desc, doc_start = extracted(lib_orb, (3, 4, 5, 6))
    assert len(desc) > 400
    a = lib_orb.train_vocabulary(desc, doc_start, 6, 3, seed=17)
    b = lib_orb.train_vocabulary(desc, doc_start, 6, 3, seed=17)
    c = lib_orb.train_vocabulary(desc, doc_start, 6, 3, seed=18)
    assert vc.same_tree(a, b) is None and np.array_equal(a["leaf"], b["leaf"])
    assert vc.same_tree(a, c, stats=False) is not None
    want = vc.transcribe(desc.cpu().numpy(), doc_start, 6, 3, seed=17)
    want["n_docs"] = 4
    check(a, want, "extracted")
    stream = torch.cuda.Stream()                                         # the same call on an external stream
    d = lib_orb.train_vocabulary(desc, doc_start, 6, 3, seed=17, stream_ptr=ctypes.c_void_p(stream.cuda_stream))
    assert vc.same_tree(a, d) is None


def test_refusals(orb):
    import torch
    lib = orb.load_library()
    desc = torch.zeros((40, 32), dtype=torch.uint8, device="cuda")
    ok = np.array([0, 10, 40], np.int32)

    def rc(n=40, ds=ok, k=4, L=2, weighting=0, scoring=0, max_it=0, ptr=None, n_docs=None):
        out = ctypes.c_void_p()
        ds = np.ascontiguousarray(ds, np.int32)
        r = lib.jsorb_vocabulary_train(0, None, ctypes.c_void_p(desc.data_ptr() if ptr is None else ptr), n, ds.ctypes.data,
                                       len(ds) - 1 if n_docs is None else n_docs, k, L, weighting, scoring, 1, max_it, ctypes.byref(out))
        if r == 0:
            lib.jsorb_vocab_train_result_destroy(out)
        else:
            assert not out.value and lib.jsorb_vocabulary_train_last_error()
        return r
    assert rc() == 0
    assert rc(n=0, ds=[0, 0, 0]) == -1 and rc(n=-1) == -1 and rc(n=2 ** 30 + 1, ds=[0, 2 ** 30 + 1]) == -1
    assert rc(k=1) == -1 and rc(k=33) == -1 and rc(k=2) == 0 and rc(k=32, L=6) == 0
    assert rc(L=0) == -1 and rc(L=17) == -1
    assert rc(k=32, L=7) == -1 and rc(k=4, L=16) == -1 and rc(k=2, L=16) == 0       # 1 + k + ... + k^L against 2^31 - 1
    assert rc(ds=[0, 30, 20, 40]) == -1 and rc(ds=[0, 10, 39]) == -1 and rc(ds=[1, 10, 40]) == -1 and rc(n_docs=0) == -1
    assert rc(weighting=4) == -1 and rc(weighting=-1) == -1 and rc(scoring=6) == -1 and rc(max_it=-1) == -1
    assert rc(ptr=desc.data_ptr() + 8, n=30, ds=[0, 30]) == -1 and rc(ptr=0) == -1
    assert lib.jsorb_vocabulary_train(0, None, ctypes.c_void_p(desc.data_ptr()), 40, ok.ctypes.data, 2, 4, 2, 0, 0, 1, 0, None) == -1
    with pytest.raises(orb.JsorbError):
        orb.train_vocabulary(np.zeros((0, 32), np.uint8), [0], 4, 2)
    with pytest.raises(orb.JsorbError):
        orb.train_vocabulary(torch.zeros((4, 31), dtype=torch.uint8, device="cuda"), [0, 4], 4, 2)
    assert lib.jsorb_vocab_train_result_info(None, *[None] * 7) == -1 and lib.jsorb_vocab_train_stats(None, None, None, None, None, None) == -1


def test_train_vocabulary_example(orb, tmp_path):
    from jetson_slam_amd import build as jb
    from jetson_slam_amd import vocabulary as voc
    exe = jb.build_example("train_vocabulary", str(tmp_path / "train_vocabulary"))
    path = str(tmp_path / "trained.txt")
    out = subprocess.run([exe, path], timeout=300, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    t = voc.load_text(path)
    assert t["k"] == 8 and t["depth_L"] == 3 and ("nodes=%d" % t["n_nodes"]) in out.stdout and "every training descriptor's word has Ni >= 1" in out.stdout
    v = orb.Vocabulary(t)
    assert v.info()["n_words"] == int((t["word_id"] >= 0).sum())
    v.close()
