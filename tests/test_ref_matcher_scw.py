"""CPU: jsorb_search_by_projection_sim3's two yardsticks held to the reference's own ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)
(ORBmatcher.cpp:277-390).  tests/golden/ref_matcher_search_scw.npz holds, per case of tests/scw_cases.py, the inputs in the reference's argument shape
(vpPoints with its bad and already-found points, vpMatched pre-filled) and what the reference returned - written by
tools/ref_matcher_scw_goldens.py on an authoring machine through tools/ref_matcher_scw_driver.cpp.  The sequential transcription and the numpy
restatement of the kernels must give those outputs on every case; every mutant of the transcription must fail the constructed case that is about
its decision.  Only outputs are stored: the probe log of oracle/ref_matcher/harness.cpp cannot be switched on from outside it."""
import numpy as np
import pytest

import scw_cases as sc
from oracle import pyref_matcher as rm


@pytest.fixture(scope="module")
def stored():
    return rm.load_golden(sc.GOLDEN)


def test_the_file_holds_every_case(stored):
    built = sc.fixture_cases()
    assert list(stored) == list(built)
    for name, c in built.items():
        s = stored[name]
        for key in ("list", "matched_in", "Scw"):
            assert np.array_equal(np.asarray(s[key]), np.asarray(c[key])), (name, key)
        for key in ("x", "y", "octave", "desc", "start", "items"):
            assert np.array_equal(np.asarray(s["K"][key]), np.asarray(c["K"][key])), (name, key)
        for key in c["P"]:
            assert np.asarray(s["P"][key]).tobytes() == np.asarray(c["P"][key]).tobytes(), (name, key)
    blocks = [n for n in stored if n.startswith("random")]
    assert len(blocks) == len(sc.BLOCK_SEEDS)
    for n in blocks:                                    # every coverage counter, on every random block
        cnt = stored[n]["counters"]
        assert all(int(cnt[k]) >= 1 for k in sc.COVERAGE) and int(cnt["rounds"]) >= 4 and int(cnt["overflow_at_2"]) >= 1, (n, cnt)
        assert int(cnt["proved"]) >= 100


def _names():
    return list(sc.fixture_cases())


@pytest.mark.parametrize("name", _names())
def test_transcription_and_restatement_equal_the_reference(po, stored, name):
    c = stored[name]
    sc.prove(c)
    ref, res = sc.both(po, c)                           # (asserts that the restatement at both caps equals the transcription)
    assert np.array_equal(ref[0], c["out"]["matched"]) and ref[1] == int(c["out"]["nmatches"]), name
    if "want" in c:
        assert np.array_equal(c["want"], c["out"]["matched"]) and int(c["want_count"]) == int(c["out"]["nmatches"])
    assert {k: int(v) for k, v in sc.trace_of(ref[4]).items()} == {k: int(c["counters"][k]) for k in sc.COVERAGE}


def test_the_driver_gives_the_stored_outputs_again(stored):
    if not sc.driver_available():
        pytest.skip("oracle/_ref/libref_matcher_scw.so is built by tools/ref_matcher_scw_goldens.py on authoring machines only")
    for name, c in stored.items():
        out = sc.run_driver(c)
        assert np.array_equal(out["matched"], c["out"]["matched"]) and int(out["nmatches"]) == int(c["out"]["nmatches"]), name


@pytest.mark.parametrize("mutant", list(sc.MUTANTS))
def test_every_mutant_fails_its_constructed_case(po, stored, mutant):
    """dist <= bestDist, bestDist < th_low, a closed IsInImage, the level window [L-1, L+1], claims ignored, blocked ignored, a non-matching point
    that claims: each differs from the reference's stored output on the case that is about it - and the transcription itself does not"""
    c = stored[sc.MUTANTS[mutant]]
    good, bad = sc.scw_reference(po, c), sc.scw_reference(po, c, mutant=mutant)
    assert np.array_equal(good[0], c["out"]["matched"]) and good[1] == int(c["out"]["nmatches"])
    assert not np.array_equal(bad[0], c["out"]["matched"]), mutant
