"""Vocabulary training on the host (tests/vocab_train_cases.py): the line-by-line transcription of TemplatedVocabulary::create and the numpy
restatement of the device's level-wise method against what the reference's own create() computed (tests/golden/ref_matcher_vocab_create.npz), the
mutants, the coverage counters, and the two statements against each other on the tight families the reference dies on.  No GPU."""
import os
import re

import numpy as np
import pytest

import vocab_train_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return vc.load_golden()


@pytest.fixture(scope="module")
def transcribed():
    """name -> the transcription's result of every recorded world: computed once, never changed"""
    return {name: vc.transcribe(**vc.world_any(name)) for name in vc.RECORDED}


def test_the_draw_function_is_the_header_s():
    """r = mix(mix(seed ^ (first << 32 | size)) + j) >> 33 (include/jsorb.h), on values worked out by hand from the definition"""
    assert vc.mix(0) == 0xE220A8397B1DCDAF                      # splitmix64's first output from state 0
    assert 0 <= vc.draw(5, 7, 9, 3) < 2 ** 31 and vc.draw(5, 7, 9, 3) != vc.draw(5, 7, 9, 4)
    assert vc.draw(894004914, 0, 3, 1) == vc.RAND_MAX and vc.draw(145830026, 0, 3, 1) == 0
    assert vc.random_int(vc.RAND_MAX, 0, 9) == 9 and vc.random_int(0, 0, 9) == 0 and vc.random_value(vc.RAND_MAX, 0, 12.0) == 12.0
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    for const in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB"):
        assert const in hdr


def test_transcription_gives_the_reference(golden, transcribed):
    assert list(golden) == vc.RECORDED
    for name in vc.RECORDED:
        assert vc.same_as_reference(golden[name], transcribed[name]) is None, (name, vc.same_as_reference(golden[name], transcribed[name]))
        assert transcribed[name]["n_empty_clusters"] == 0 and transcribed[name]["n_unconverged"] == 0, name


def test_levelwise_restatement_gives_the_reference_and_the_transcription(golden, transcribed):
    for name in vc.RECORDED:
        got = vc.levelwise(**vc.world_any(name))
        assert vc.same_as_reference(golden[name], got) is None, (name, vc.same_as_reference(golden[name], got))
        assert vc.same_tree(transcribed[name], got) is None and np.array_equal(transcribed[name]["leaf"], got["leaf"]), name


def test_coverage_counters(transcribed):
    total = vc.new_cov()
    for name in vc.RECORDED:
        for key, v in transcribed[name]["coverage"].items():
            total[key] += v
    assert all(v > 0 for key, v in total.items() if key != "empty_cluster"), total
    assert total["empty_cluster"] == 0
    assert {vc.world_any(name)["weighting"] for name in vc.RECORDED} == {0, 1, 2, 3}
    # the constructed cases decide what they name
    assert transcribed["cut_is_sum"]["n_draws"] == 2 and transcribed["redraw"]["n_draws"] == 3
    assert transcribed["identical_50"]["n_nodes"] == 4 and transcribed["n_below_k"]["lloyd_passes"] == [0] * 16


@pytest.mark.parametrize("mutant,name", [("assoc_le", "surv_0_0"), ("mean_gt", "surv_0_0"), ("mean_half", "surv_0_0"), ("cut_gt", "cut_is_sum"),
                                         ("shared_draws", "surv_0_0"), ("bfs_ids", "surv_0_0"), ("ni_per_descriptor", "surv_0_0")])
def test_every_mutant_fails_its_world(golden, mutant, name):
    assert mutant in vc.MUTANTS
    assert vc.same_as_reference(golden[name], vc.levelwise(mutant=mutant, **vc.world_any(name))) is not None


def test_tight_families_and_the_iteration_cap():
    """where the reference dies (an empty cluster) the two statements still agree, and so they do when the cap ends a level"""
    empties = 0
    for name in vc.TIGHT_NAMES:
        w = vc.world(name)
        a, b = vc.transcribe(**w), vc.levelwise(**w)
        assert vc.same_tree(a, b) is None and np.array_equal(a["leaf"], b["leaf"]), (name, vc.same_tree(a, b))
        empties += a["n_empty_clusters"]
    assert empties > 0 and vc.transcribe(**vc.empty_cluster_world())["n_empty_clusters"] > 0
    w = dict(vc.world("surv_0_0"), max_iterations=1)
    a, b = vc.transcribe(**w), vc.levelwise(**w)
    assert vc.same_tree(a, b) is None and a["n_unconverged"] == a["n_kmeans_runs"] > 0 and a["lloyd_passes"][:3] == [1, 1, 1]


def test_text_file_has_the_reference_s_line_order(tmp_path, transcribed):
    """vocabulary.save_text of a result: node ids 1, 2, ... in line order, every parent before its children (saveToTextFile, :1428-1457)"""
    from jetson_slam_amd import vocabulary as voc
    t = transcribed["surv_5_0"]
    path = str(tmp_path / "voc.txt")
    voc.save_text(path, t, scoring=0, weighting=vc.world("surv_5_0")["weighting"])
    back = voc.load_text(path)
    for key in ("child_start", "children", "descriptors", "word_id"):
        assert np.array_equal(back[key], t[key]), key
    assert np.array_equal(back["weight"].view(np.uint64), t["weight"].view(np.uint64))
    rows = open(path).read().splitlines()[1:]
    assert [int(r.split()[0]) for r in rows] == [int(p) for p in t["parent"][1:]]


def test_build_lists_and_abi():
    from jetson_slam_amd import build as jb
    from jetson_slam_amd import orb
    assert "k_vocab_train.hip" in jb.SOURCES and "jsorb_vocab_train.hip" in jb.SOURCES and "train_vocabulary" in jb.EXAMPLES
    assert jb.VARIANTS["tiny_vocab_train"] == (["-DVT_CHUNK=%d" % vc.TINY[0], "-DVT_SCAN_THREADS=%d" % vc.TINY[1]], ["k_vocab_train.hip"])
    hdr = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    src = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    for n in ("jsorb_vocabulary_train", "jsorb_vocabulary_train_last_error", "jsorb_vocab_train_result_destroy", "jsorb_vocab_train_result_info",
              "jsorb_vocab_train_result_copy", "jsorb_vocab_train_result_copy_assignment", "jsorb_vocab_train_stats", "jsorb_vocab_train_build_caps"):
        assert n in orb.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr) and '"%s": (' % n in src, n
