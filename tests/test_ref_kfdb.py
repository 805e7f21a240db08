"""Both host statements of tests/kfdb_cases.py against what the reference's own KeyFrameDatabase (src/KeyFrameDatabase.cpp:44-313), BowVector.cpp and
ScoringObject.cpp, compiled unmodified (tools/ref_kfdb/), computed, as tests/golden/ref_matcher_kfdb.npz records it: BowVectors and scores as bits,
candidates in order, the persistent fields after every operation.  Where the reference tree is present the driver is built and run again and must
reproduce the file.  No GPU."""
import numpy as np
import pytest

import kfdb_cases as kc

WORLD_KEYS = ("weight", "M", "op_kind", "op_slot", "op_id", "op_min_score", "op_feat_start", "feat", "op_list_start", "lst", "conn", "neigh")


@pytest.fixture(scope="module")
def golden():
    return kc.load_golden()


def recorded(g):
    return {k: g["out_" + k] for k in kc.OUT_KEYS}


def test_the_file_holds_the_worlds_the_tests_generate(golden):
    worlds = kc.fixture_worlds()
    assert list(golden) == list(worlds)
    for name, w in worlds.items():
        for k in WORLD_KEYS:
            assert np.array_equal(golden[name][k], w[k]) and golden[name][k].dtype == np.asarray(w[k]).dtype, (name, k)
        if name.startswith("random"):
            assert (golden[name]["counters"] > 0).all(), name


def test_transcription_and_restatement_give_the_reference(golden):
    for name, g in golden.items():
        ref = recorded(g)
        mine = kc.run(g, kc.Transcription(g))
        assert kc.same(ref, mine) is None, (name, kc.same(ref, mine))
        for caps in (kc.SHIPPED, kc.TINY):
            got = kc.run(g, kc.Restatement(g, caps))
            assert kc.same(ref, got) is None, (name, caps, kc.same(ref, got))


def test_the_driver_reproduces_the_file(golden, tmp_path):
    reference = kc.reference_tree()
    if reference is None:
        return                                   # no reference tree here: the file stands for it (the tests above hold both statements to it)
    kc.build_driver(reference)
    for name, g in golden.items():
        got = kc.run_driver(g, str(tmp_path))
        assert kc.same(recorded(g), got) is None, (name, kc.same(recorded(g), got))
