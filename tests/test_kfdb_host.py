"""The two host statements of tests/kfdb_cases.py against each other - the sequential transcription of KeyFrameDatabase.cpp / BowVector.cpp /
ScoringObject.cpp and the numpy restatement of k_kfdb.hip's method - on every world, for the shipped and the tiny caps; the constructed worlds decide
what they name; every mutant of the transcription fails a named world; the new entries are declared in the three interfaces.  No GPU."""
import os
import re

import numpy as np
import pytest

import kfdb_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALSO = ("stats", "best_acc")


@pytest.fixture(scope="module")
def worlds():
    """name -> (world, the transcription's outputs, its coverage counters): computed once, never changed"""
    out = {}
    for name, w in kc.fixture_worlds().items():
        t = kc.Transcription(w)
        out[name] = (w, kc.run(w, t), t.count)
    return out


def test_restatement_equals_transcription_on_every_world(worlds):
    seen = set()
    for name, (w, mine, _) in worlds.items():
        for caps in (kc.SHIPPED, kc.TINY):
            r = kc.Restatement(w, caps)
            got = kc.run(w, r)
            assert kc.same(mine, got, kc.OUT_KEYS + ALSO) is None and mine["order"] == got["order"], (name, caps, kc.same(mine, got, kc.OUT_KEYS + ALSO))
            if caps == kc.TINY:
                seen |= {k for k, v in r.paths.items() if v}
        seen.add(name)
    assert set(worlds) <= seen and {"sort_lds", "sort_global", "query_lds", "query_global"} <= seen      # no world left out, both paths of both caps


def test_constructed_worlds_decide_what_they_name(worlds):
    cases = kc.constructed()
    assert len(cases) >= 20
    for name, (_, check) in cases.items():
        check(worlds["c_" + name][1])


def test_random_blocks_cover_every_decision(worlds):
    for seed in kc.BLOCK_SEEDS:
        w, _, count = worlds["random_%d" % seed]
        assert not [k for k in kc.COUNTERS if count[k] == 0], (seed, count)
        n_feat = np.diff(w["op_feat_start"])
        assert int(w["M"]) <= 40 and n_feat.max() <= 300 and n_feat.min() == 0 and 32 <= len(w["weight"]) <= 4096 and (w["weight"] == 0).any()


def test_sequential_sums_differ_from_pairwise_sums(worlds):
    kc.check_summation_case(worlds["c_sequential_sum_differs_from_pairwise"][0])
    # addWeight's w + w + ... is not c * w either: some word of some block has other bits
    w = worlds["random_%d" % kc.BLOCK_SEEDS[0]][0]
    assert kc.same(kc.run(w, kc.Transcription(w)), kc.run(w, kc.Transcription(w, "c_times_w")), ("bow_value",)) == "bow_value"


# the constructed world each mutant must fail (and may fail others)
MUTANT_FAILS = {"pairwise_sum": "c_sequential_sum_differs_from_pairwise", "c_times_w": "random_%d" % kc.BLOCK_SEEDS[0],
                "ge_words": "c_max_common_words_5", "ge_best": "c_acc_equals_retain_dropped", "ge_retain": "c_acc_equals_retain_dropped",
                "slot_order": "c_list_order_is_neither_slot_nor_add_order", "reloc_words_test": "c_stale_reloc_score_is_read",
                "scores_reset": "c_stale_reloc_score_is_read"}


@pytest.mark.parametrize("mutant", kc.MUTANTS)
def test_every_mutant_fails_its_named_world(worlds, mutant):
    w, mine, _ = worlds[MUTANT_FAILS[mutant]]
    assert kc.same(mine, kc.run(w, kc.Transcription(w, mutant))) is not None, mutant
    assert set(MUTANT_FAILS) == set(kc.MUTANTS)


def test_the_new_entries_are_declared_in_the_three_interfaces():
    names = ("jsorb_keyframe_database_create", "jsorb_keyframe_database_destroy", "jsorb_keyframe_database_set_stream", "jsorb_keyframe_database_last_error",
             "jsorb_bow_vector_async", "jsorb_keyframe_database_add_async", "jsorb_keyframe_database_erase", "jsorb_keyframe_database_clear",
             "jsorb_keyframe_database_score_async", "jsorb_detect_loop_candidates_async", "jsorb_detect_relocalization_candidates_async",
             "jsorb_detect_loop_candidates", "jsorb_detect_relocalization_candidates", "jsorb_detect_candidates_stats", "jsorb_kfdb_build_caps")
    header = open(os.path.join(ROOT, "include", "jsorb.h")).read()
    binding = open(os.path.join(ROOT, "jetson_slam_amd", "orb.py")).read()
    shim = open(os.path.join(ROOT, "include", "jsorb_compat.hpp")).read()
    for n in names:
        assert re.search(r"\b%s\(" % n, header), n
        assert '"%s"' % n in binding, n
    assert "class KeyframeDatabase" in binding and "def kfdb_build_caps" in binding
    for n in ("class KeyframeDatabase", "DetectLoopCandidates", "DetectRelocalizationCandidates", "ComputeBowVector"):
        assert n in shim, n
    from jetson_slam_amd import build as jb
    assert "k_kfdb.hip" in jb.SOURCES and "jsorb_kfdb.hip" in jb.SOURCES and jb.VARIANTS["tiny_kfdb"][1] == ["k_kfdb.hip"]
