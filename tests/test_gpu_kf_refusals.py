"""-m gpu: every refusal of the five keyframe-set entry-point pairs and their `_stats` readers (tests/kf_refusal_cases.py) answers the (rc, text)
recorded in tests/golden/kf_matcher_refusals.json from the commit before their host frames were shared - never what the tree itself answers -
and after each refused call the entry point's valid call at n1 = 1 against one keyframe of one keypoint returns its recorded result."""
import json

import pytest

import kf_refusal_cases as cases

pytestmark = pytest.mark.gpu
ENTRY_POINTS = ["search_by_bow", "search_for_triangulation", "fuse", "search_by_bow_kf", "search_by_sim3"]


@pytest.fixture(scope="module")
def recorded():
    with open(cases.GOLDEN) as f:
        return cases.unpack(json.load(f))      # (the valid call's result is stored once per entry point and form)


@pytest.fixture(scope="module")
def answered(orb):
    return json.loads(json.dumps(cases.run()))      # (through JSON: tuples and lists compare as the recording holds them)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_refusals_answer_as_recorded(recorded, answered, name):
    rec, got = recorded[name], answered[name]
    assert sorted(got) == sorted(rec)                # the same rows: none dropped, none new without a recording
    for row in rec:
        assert got[row]["refusal"] == rec[row]["refusal"], (row, got[row]["refusal"], rec[row]["refusal"])
        assert got[row]["refusal"][0] != 0, row
        assert got[row]["after"] == rec[row]["after"], (row, got[row]["after"], rec[row]["after"])


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_the_earlier_of_two_violated_checks_answers(recorded, name):
    rec = recorded[name]
    pairs = [row for row in rec if rec[row]["same_as"]]
    assert len(pairs) >= 6, pairs
    for row in pairs:
        assert rec[row]["refusal"] == rec[rec[row]["same_as"]]["refusal"], row


def test_the_two_quirks_are_rows(recorded):
    long_kf = "a keyframe with more than 262143 keypoints"
    for name in ("search_for_triangulation", "search_by_bow_kf", "fuse"):
        for form in ("async", "sync"):
            assert recorded[name]["%s/kf_long_is_invalid" % form]["refusal"] == [-1, "%s: %s" % (name, long_kf)]
    for form in ("async", "sync"):
        assert recorded["search_by_bow"]["%s/kf_long_is_unsupported" % form]["refusal"] == [-3, "search_by_bow: " + long_kf]
    assert recorded["search_by_bow"]["sync/image_before_n_keyframes"]["refusal"] == [-4, "search_by_bow: no extract result for this image"]
    assert recorded["search_by_bow"]["sync/n_keyframes"]["refusal"] == [-1, "search_by_bow: n_keyframes must be in [0, 256]"]
