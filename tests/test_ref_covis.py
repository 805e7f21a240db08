"""-m "not gpu": the two yardsticks of tests/covis_cases.py against the reference's own src/KeyFrame.cpp - the worlds recorded in
tests/golden/ref_matcher_covis.npz (tools/ref_covis_goldens.py), and, where the reference tree is present, the driver rebuilt and compared
live."""
import numpy as np
import pytest

import covis_cases as cc

WORLDS = {w["name"]: w for w in cc.golden_worlds()}
GOLDEN = cc.load_golden()


def test_the_file_holds_the_worlds_and_nothing_else():
    assert list(GOLDEN) == list(WORLDS) and len(WORLDS) == len(cc.GOLDEN_CASES) + len(cc.GOLDEN_SEEDS) >= 30
    n_erase = n_parent = 0
    for name, rec in GOLDEN.items():
        assert sorted(rec) == sorted(cc.GOLDEN_KEYS) and rec["lens"].dtype == rec["wide"].dtype == rec["parent_out"].dtype == np.int32
        assert rec["lens"].shape == (len(WORLDS[name]["script"]), 5, cc.S) and rec["wide"].shape[-1] <= WORLDS[name]["C"]
        n_erase += sum(kind == "erase" for kind, _ in WORLDS[name]["script"])
        n_parent += int((rec["parent_out"] >= 0).sum())
    assert n_erase >= 10 and n_parent >= 100


@pytest.mark.parametrize("name", list(WORLDS))
def test_both_yardsticks_reproduce_the_reference(name):
    w = WORLDS[name]
    r = cc.run_restated(w)
    assert not cc.overflowed(r)                  # (overflow is the restatement's alone: no recorded world has any)
    cc.same_as_recorded(w, r, GOLDEN[name])
    cc.same_as_recorded(w, cc.run_literal(w), GOLDEN[name])


def test_the_driver_rebuilt_gives_the_recorded_arrays(tmp_path):
    ref = cc.reference_tree()
    if ref is None:
        pytest.skip("the reference tree is not here")
    cc.build_driver(ref)
    for name, w in WORLDS.items():
        rec = cc.run_driver(w, str(tmp_path))
        for k in cc.GOLDEN_KEYS:
            assert np.array_equal(rec[k], GOLDEN[name][k]), (name, k)
